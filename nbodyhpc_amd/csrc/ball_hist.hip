// Radius histogram (NEW, nbkd_query_ball_hist): the radius count of ball.hip
// for nr ascending radii in one tree walk.  Thresholds t[j] = r[j]^2 (f32);
// the count of a query at radius j is the number of points with d2 <= t[j],
// the same d2 and the same test as the single-radius count, so column j equals
// nbkd_query_ball_count(q, r[j]) bit for bit.
//
// 64-query packets, one query per lane, behind the shared prologue and on the
// shared packet walk (packet.hpp packet_query, packet_plain, walk_next_leaf,
// stage_points) with the bound t[nr-1].  Each lane keeps a differential histogram in LDS,
// hist[bin][lane] (64 four-byte banks: the wave's accesses to one bin never
// conflict): a point goes to bin j = the number of thresholds below its d2,
// points beyond t[nr-1] to a dump row nr that nothing reads.  At a leaf a lane
// compares the bounds lb <= d2 <= ub of the tight box with the thresholds: a
// threshold below lb has every point of the leaf beyond it, one at or above ub
// has every point within it, and only a threshold with lb <= t[j] < ub can
// split the leaf's points.  A lane with no such threshold (and no padding
// points in the leaf) adds the leaf's whole count to its bin without
// evaluating a point.  The others evaluate the staged points against the
// thresholds some lane of the wave needs (a wave-uniform mask, so the
// thresholds are read once per step for the 64 lanes); a threshold a lane does
// not need gives that lane the answer its bounds already fixed.  At the end of
// the walk each lane prefix-sums its bins into cumulative counts.
#include <algorithm>

#include "internal.hpp"
#include "metric.hpp"
#include "packet.hpp"

namespace nbkd {
namespace {
using namespace dev;

constexpr int TB = 256;
constexpr int WPB = TB / 64;
constexpr int EV = 8;     // staged points evaluated per step of the threshold loop

// one wave's LDS: the staged points, hist[(nr + 1)][64], the thresholds
__host__ __device__ constexpr uint32_t hist_wave_bytes(int nr) {
    return (uint32_t)(CHUNK * 16 + (nr + 1) * 64 * 4 + NBKD_MAX_RADII * 4);
}

// the staged points against the thresholds in tmask: bin = base + the number
// of those thresholds below d2 (written !(d2 <= t): the count's own test)
template <bool M>
__device__ __forceinline__ void hist_chunk(const float4 *p4s, uint32_t cn, uint32_t *hist,
                                           const float *thr, uint32_t tmask, uint32_t base,
                                           bool ev, int lane, float qx, float qy, float qz,
                                           float L) {
#pragma unroll 1
    for (uint32_t u = 0; u < cn; u += EV) {
        float d[EV];
        uint32_t b[EV];
#pragma unroll
        for (int i = 0; i < EV; ++i) {
            const float4 a = p4s[u + i];
            d[i] = point_d2_fast<M>(qx, qy, qz, a.x, a.y, a.z, L);
            b[i] = base;
        }
        // (tmask != 0 here; the next threshold is read, an LDS broadcast,
        // while this one is compared)
        uint32_t mk = tmask;
        float tj = thr[__builtin_ctz(mk)];
        for (;;) {
            mk &= mk - 1;
            const float tn = thr[mk ? __builtin_ctz(mk) : 0];
#pragma unroll
            for (int i = 0; i < EV; ++i) b[i] += !(d[i] <= tj) ? 1u : 0u;
            if (!mk) break;
            tj = tn;
        }
        if (ev) {
#pragma unroll
            for (int i = 0; i < EV; ++i)
                if (u + i < cn) atomicAdd(&hist[b[i] * 64u + lane], 1u);
        }
    }
}

template <bool PER, bool M>
__device__ __forceinline__ void ball_hist_walk(const DevTree &t, const uint32_t *__restrict__ linfo,
                                               const PadLeaves &pad, float4 *p4s, uint32_t *hist,
                                               const float *thr, const int nr, const int lane,
                                               const float qx, const float qy, const float qz,
                                               const float kth) {
    const float L = t.box;
    const cnode_ptr cnodes = (cnode_ptr)t.nodes;
    const cbox_ptr cboxes = (cbox_ptr)t.nbox;
    PacketWalk w;
    walk_begin(w);
    uint32_t lpos = 0, lend = 0, visits = 0;
    while (walk_next_leaf<M, false, false>(w, cnodes, cboxes, qx, qy, qz, kth, L, lpos, lend,
                                           visits)) {
        float tb[6];
        leaf_tight_box(linfo, w.node, tb);
        const float lb = box_lb2<M>(qx, qy, qz, tb, L);
        const bool need = lb <= kth;
        if (!__any(need)) continue;
        // (a leaf holding padding points, in no bin, is always evaluated)
        const bool padded = leaf_padded(pad, w.node);
        const float ub = box_ub2<PER>(qx, qy, qz, tb);
        // jall: the thresholds below lb (the bin of a leaf no threshold splits);
        // tmask: the thresholds that may split the leaf for some lane; base:
        // the thresholds below lb that are not in tmask
        uint32_t jall = 0, base = 0, tmask = 0;
        bool split = false;
        for (int j = 0; j < nr; ++j) {
            const float tj = thr[j];
            const bool below = !(lb <= tj);
            const bool sj = need && (padded || (!below && !(ub <= tj)));
            split |= sj;
            jall += below ? 1u : 0u;
            if (__any(sj))
                tmask |= 1u << j;
            else
                base += below ? 1u : 0u;
        }
        // need: lb <= t[nr-1], so jall < nr
        if (need && !split) atomicAdd(&hist[jall * 64u + lane], lend - lpos);
        const bool ev = need && split;
        if (tmask == 0) continue;
        // the plain d2 where no evaluating lane wraps around (wrap_free)
        const bool plain_leaf = !M || __all(!ev || wrap_free(qx, qy, qz, tb, L));
        for (uint32_t c0 = lpos; c0 < lend; c0 += CHUNK) {
            const uint32_t cn = min((uint32_t)CHUNK, lend - c0);
            stage_points(t.p4, c0, p4s, lane, cn);
            if (plain_leaf)
                hist_chunk<false>(p4s, cn, hist, thr, tmask, base, ev, lane, qx, qy, qz, L);
            else
                hist_chunk<M>(p4s, cn, hist, thr, tmask, base, ev, lane, qx, qy, qz, L);
        }
    }
}

template <bool PER>
__global__ void __launch_bounds__(TB, 8)
ball_hist_kernel(DevTree t, const uint32_t *__restrict__ linfo, const float *__restrict__ q,
                 const uint32_t *__restrict__ order, uint32_t m, HistThr T, int nr, PadLeaves pad,
                 uint32_t *__restrict__ out_counts, unsigned long long *__restrict__ totals) {
    extern __shared__ float4 hist_lds[];
    const int lane = threadIdx.x & 63, wave = wave_id();
    char *const wbase = (char *)hist_lds + (size_t)wave * hist_wave_bytes(nr);
    float4 *const p4s = (float4 *)wbase;
    uint32_t *const hist = (uint32_t *)(wbase + CHUNK * 16);
    float *const thr = (float *)(wbase + CHUNK * 16 + (nr + 1) * 64 * 4);
    if (lane < nr) thr[lane] = T.t[lane];
    for (int j = 0; j <= nr; ++j) hist[j * 64 + lane] = 0;
    wave_sync();
    const uint32_t gq = (xcd_block(blockIdx.x, gridDim.x) * WPB + wave) * 64u + lane;
    const float L = t.box;
    const PacketQuery p = packet_query<PER>(q, order, gq, m, L);
    const uint32_t qo = p.qo;
    const float qx = p.x, qy = p.y, qz = p.z;
    const bool active = p.valid && p.inside;
    const float r2 = unif(thr[nr - 1]);
    const float kth = active ? r2 : -INFINITY;
    // every active lane's ball of the largest radius clears the box faces:
    // the plain formulas
    if (packet_plain<PER>(active, r2, qx, qy, qz, L))
        ball_hist_walk<PER, false>(t, linfo, pad, p4s, hist, thr, nr, lane, qx, qy, qz, kth);
    else
        ball_hist_walk<PER, PER>(t, linfo, pad, p4s, hist, thr, nr, lane, qx, qy, qz, kth);
    wave_sync();
    // cumulative counts: the lane's row, and the wave's sums into the totals
    uint32_t c = 0;
    for (int j = 0; j < nr; ++j) {
        c += hist[j * 64 + lane];
        if (out_counts && active) out_counts[(size_t)qo * nr + j] = c;
        if (totals) {
            unsigned long long v = active ? c : 0u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if (lane == 0 && v) atomicAdd(&totals[j], v);
        }
    }
}

// Periodic queries outside [0, L]^3 (listed by outside_box_kernel, the length
// in device memory): every point tested with the reference-exact metric, as in
// ball_brute_dev_kernel; the cumulative count at threshold j is counted
// directly.  Rows and totals accumulate with atomics (rows zeroed first).
__global__ void __launch_bounds__(TB)
hist_zero_dev_kernel(const uint32_t *__restrict__ list, const uint32_t *__restrict__ nout, int nr,
                     uint32_t *__restrict__ out_counts) {
    const uint64_t c = (uint64_t)*nout * (uint32_t)nr;
    for (uint64_t e = blockIdx.x * TB + threadIdx.x; e < c; e += gridDim.x * TB) {
        const uint32_t j = (uint32_t)(e / (uint32_t)nr), k = (uint32_t)(e - (uint64_t)j * nr);
        out_counts[(size_t)list[j] * nr + k] = 0;
    }
}

__global__ void __launch_bounds__(TB)
hist_brute_dev_kernel(DevTree t, const float *__restrict__ q, const uint32_t *__restrict__ list,
                      const uint32_t *__restrict__ nout, uint32_t ntiles, HistThr T, int nr,
                      uint32_t *__restrict__ out_counts, unsigned long long *__restrict__ totals) {
    __shared__ float thr[WPB][NBKD_MAX_RADII];
    const int lane = threadIdx.x & 63, wave = wave_id();
    if (lane < nr) thr[wave][lane] = T.t[lane];
    wave_sync();
    const uint64_t total = (uint64_t)__builtin_amdgcn_readfirstlane(*nout) * ntiles;
    const float L = t.box;
    for (uint64_t w = blockIdx.x; w < total; w += gridDim.x) {
        const BruteTile b = brute_tile<TB>(w, ntiles, list, q);
        const uint32_t qo = b.qo;
        float d[BR_ITEMS];
#pragma unroll
        for (int u = 0; u < BR_ITEMS; ++u) {
            const uint32_t p = b.base + u * TB;
            d[u] = p < t.n8 ? point_d2<true>(b.qx, b.qy, b.qz, t.x[p], t.y[p], t.z[p], L) : INFINITY;
        }
        for (int k = 0; k < nr; ++k) {
            const float tk = thr[wave][k];
            uint32_t c = 0;
#pragma unroll
            for (int u = 0; u < BR_ITEMS; ++u) c += d[u] <= tk ? 1u : 0u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
            if (lane == 0 && c) {
                if (out_counts) atomicAdd(&out_counts[(size_t)qo * nr + k], c);
                if (totals) atomicAdd(&totals[k], (unsigned long long)c);
            }
        }
    }
}

} // namespace

void launch_ball_hist(const Tree &t, const float *q, const uint32_t *order, uint32_t m,
                      const HistThr &thr, int nr, uint32_t *out_counts,
                      unsigned long long *totals, hipStream_t s) {
    const PadLeaves pad = pad_leaves_of(t);
    const unsigned blocks = (unsigned)(((uint64_t)m + TB - 1) / TB);
    const size_t lds = (size_t)WPB * hist_wave_bytes(nr);
    if (t.periodic)
        ball_hist_kernel<true><<<blocks, TB, lds, s>>>(view(t), t.leafinfo, q, order, m, thr, nr,
                                                       pad, out_counts, totals);
    else
        ball_hist_kernel<false><<<blocks, TB, lds, s>>>(view(t), t.leafinfo, q, order, m, thr, nr,
                                                        pad, out_counts, totals);
}

void launch_ball_hist_outside_dev(const Tree &t, const float *q, const uint32_t *list,
                                  const uint32_t *nout, const HistThr &thr, int nr,
                                  uint32_t *out_counts, unsigned long long *totals,
                                  hipStream_t s) {
    const uint32_t ntiles = (uint32_t)((t.n8 + TB * BR_ITEMS - 1) / (TB * BR_ITEMS));
    if (out_counts) hist_zero_dev_kernel<<<64, TB, 0, s>>>(list, nout, nr, out_counts);
    hist_brute_dev_kernel<<<2048, TB, 0, s>>>(view(t), q, list, nout, ntiles, thr, nr, out_counts,
                                              totals);
}

} // namespace nbkd
