// Weighted radial profiles (NEW, nbkd_query_ball_profile: the reference has
// neither a radius search nor a reduction over neighbours):
//   out_sum[i, b, c] = sum_j values[j, c]  over the points j of bin b of query i,
// bin b = the number of thresholds t_ik = fl(e_ik * e_ik), e_ik = fl(radii[k] *
// scale[i]), with !(d2(i, j) <= t_ik): ball_hist.hip's binning against each
// lane's own thresholds, with ball_sum.hip's staged values (packet.hpp
// stage_values) where the histogram counts.  The threshold classification of a
// leaf and the binning step of a chunk are ball_hist.hip's statements with the
// lane's own thresholds (thr[j * 64 + lane] for thr[j]); they are written out
// in both files: as shared functions they compile to other loop bodies here
// (DESIGN.md section 3).
//
// ball_profile_kernel: 64-query packets, one wave each, the packet walk
// (packet.hpp, the macro form NBKD_GWALK) with the lane's own bound t_i,nr-1.  Per wave in LDS: the staged
// chunk of Tree::p4, its rows of the values in tree order (vt, written once per
// call by launch_ball_sum_gather), acc[(nr + 1)][NV][64] and thr[nr][64].  Lane
// l owns column l of every row of acc and thr (64 four-byte banks: the wave's
// accesses to one row never conflict), so a bin is a plain LDS read-add-write
// by its owner: no atomics, and each (query, bin, channel) is one f32
// accumulator summed in the walk's order (prof_add4 does four points' updates
// with one LDS round trip and the same bits).  Row nr of acc takes the points
// beyond the last threshold; nothing reads it.
//
// At a leaf a lane compares the bounds lb <= d2 <= ub of the tight box with its
// thresholds (ball_hist.hip): one below lb has every point of the leaf beyond
// it, one at or above ub has every point within it, the others may split the
// leaf.  A lane no threshold splits (and whose leaf holds no padding) adds the
// staged values to its one bin without evaluating d2, in ascending tree
// position: the order of the evaluating lanes, so the bits are the same.  The
// others test the staged points against the thresholds that split the leaf for
// some lane (a wave-uniform mask); a threshold a lane does not need gives that
// lane the answer its bounds already fixed.
//
// The block holds 4, 2 or 1 waves, the most whose LDS fits 64 KiB (chosen on
// the host from nr and NV).  Periodic queries outside [0, L]^3 are excluded here
// (their minimum-image pruning is not a bound) and answered by
// ball_profile_brute_kernel below.
#include <algorithm>

#include "internal.hpp"
#include "metric.hpp"
#include "packet.hpp"

namespace nbkd {
namespace {
using namespace dev;

constexpr int TBMAX = 256;
constexpr int EV = 8;     // staged points binned per step of the threshold loop
constexpr uint32_t LDS_BLOCK = 64u * 1024u;

// one wave's LDS: the staged points, their value rows, acc[(nr + 1)][nv][64],
// thr[nr][64]
__host__ __device__ constexpr uint32_t prof_wave_bytes(int nr, int nv) {
    return (uint32_t)(CHUNK * 16 + CHUNK * nv * 4 + (nr + 1) * nv * 64 * 4 + nr * 64 * 4);
}

// the squared edge fl(e * e), e = fl(r * sc); an overflowing product counts as
// FLT_MAX, so the padding points (d2 = inf) are in no bin.  -inf for a query
// without bins (ok = false)
__device__ __forceinline__ float prof_thr(float r, float sc, bool ok) {
    const float e = r * sc;
    return ok ? fminf(e * e, FLT_MAX) : -INFINITY;
}
__device__ __forceinline__ bool scale_ok(float sc) { return sc >= 0.0f && sc <= FLT_MAX; }

// four staged points' values into their bins, in the points' order: the four
// bins' words are read together (one LDS round trip), a point whose bin an
// earlier one of the four shares continues from that one's sum, and the four
// results are written in order, so the last write of a bin holds every term:
// the bits of four read-add-writes one after the other
template <int NV>
__device__ __forceinline__ void prof_add4(float *acc, const float *vs, uint32_t u0,
                                          const uint32_t (&b)[4], int lane) {
    float v[4][NV], a[4][NV];
    float *row[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        row[i] = acc + (b[i] * NV) * 64u + lane;
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            v[i][c] = vs[(u0 + i) * NV + c];
            a[i][c] = row[i][c * 64];
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < i; ++j) {
            const bool same = b[j] == b[i];
#pragma unroll
            for (int c = 0; c < NV; ++c) a[i][c] = same ? a[j][c] : a[i][c];
        }
#pragma unroll
        for (int c = 0; c < NV; ++c) a[i][c] += v[i][c];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int c = 0; c < NV; ++c) row[i][c * 64] = a[i][c];
    }
}

// the staged points against the lane's thresholds in tmask: bin = base + the
// number of those thresholds below d2 (written !(d2 <= t): the count's own
// test); the evaluating lanes add the point's values to that bin, in order.
// A slot past the chunk's end goes to the dump row nr.
template <bool M, int NV>
__device__ __forceinline__ void prof_chunk(const float4 *p4s, const float *vs, uint32_t cn,
                                           float *acc, const float *thr, uint32_t tmask,
                                           uint32_t base, bool ev, uint32_t nr, int lane, float qx,
                                           float qy, float qz, float L) {
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
        // (tmask != 0 here; the lane's next threshold is read while this one
        // is compared)
        uint32_t mk = tmask;
        float tj = thr[__builtin_ctz(mk) * 64 + lane];
        for (;;) {
            mk &= mk - 1;
            const float tn = thr[(mk ? __builtin_ctz(mk) : 0) * 64 + lane];
#pragma unroll
            for (int i = 0; i < EV; ++i) b[i] += !(d[i] <= tj) ? 1u : 0u;
            if (!mk) break;
            tj = tn;
        }
        if (ev) {
#pragma unroll
            for (int g = 0; g < EV; g += 4) {
                const uint32_t b4[4] = {u + g < cn ? b[g] : nr, u + g + 1 < cn ? b[g + 1] : nr,
                                        u + g + 2 < cn ? b[g + 2] : nr,
                                        u + g + 3 < cn ? b[g + 3] : nr};
                prof_add4<NV>(acc, vs, u + g, b4, lane);
            }
        }
    }
}

// M: the metric's formulas, plain for a packet whose largest balls all clear
// the box faces (ball.hip ball_fill_kernel)
template <bool PER, bool M, int NV>
__device__ __forceinline__ void ball_profile_walk(const DevTree &t,
                                                  const uint32_t *__restrict__ linfo,
                                                  const PadLeaves &pad,
                                                  const float *__restrict__ vt, float4 *p4s,
                                                  float *vs, float *acc, const float *thr,
                                                  const int nr, const int lane, const float qx,
                                                  const float qy, const float qz, const float kth) {
    const float L = t.box;
    uint32_t sk_node = 0;
    int sp = 0;
    const cnode_ptr cnodes = (cnode_ptr)t.nodes;
    const cbox_ptr cboxes = (cbox_ptr)t.nbox;
    uint32_t node = 0;
    float bx[6];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        bx[2 * a] = PER ? 0.0f : -FLT_MAX;
        bx[2 * a + 1] = PER ? L : FLT_MAX;
    }
    float tm[3] = {box_lb_axis<M>(qx, bx[0], bx[1], L), box_lb_axis<M>(qy, bx[2], bx[3], L),
                   box_lb_axis<M>(qz, bx[4], bx[5], L)};
    uint64_t wm = __ballot((tm[0] + tm[1]) + tm[2] <= kth);
    bool have = wm != 0;
    nbkd_node nd = cnodes[0]; // record of `node` while `have`
    // the packet walk in its macro form (packet.hpp says why this kernel keeps
    // it), its bound each lane's own kth
    constexpr bool STATS = false;
    uint32_t st[1] = {0};
    (void)st;
    for (;;) {
        bool found;
        uint32_t lpos = 0, lend = 0;
        NBKD_GWALK(found, lpos, lend);
        if (!found) break;
        float tb[6];
        leaf_tight_box(linfo, node, tb);
        const float lb = box_lb2<M>(qx, qy, qz, tb, L);
        const bool need = lb <= kth;
        if (!__any(need)) continue;
        // a leaf holding padding points (FLT_MAX, in no bin) is always evaluated
        bool padded = false;
#pragma unroll
        for (int j = 0; j < NBKD_PAD_LEAVES; ++j) padded |= pad.id[j] == node;
        const float ub = box_ub2<PER>(qx, qy, qz, tb);
        // jall: the lane's thresholds below lb (the bin of a leaf no threshold
        // splits); tmask: the thresholds that may split the leaf for some lane;
        // base: the thresholds below lb that are not in tmask
        uint32_t jall = 0, base = 0, tmask = 0;
        bool split = false;
        for (int j = 0; j < nr; ++j) {
            const float tj = thr[j * 64 + lane];
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
        const bool full = need && !split, ev = need && split;
        // the plain d2 where no evaluating lane wraps around (wrap_free)
        const bool plain_leaf = !M || __all(!ev || wrap_free(qx, qy, qz, tb, L));
        float *const frow = acc + (jall * NV) * 64u + lane;
        for (uint32_t c0 = lpos; c0 < lend; c0 += CHUNK) {
            const uint32_t cn = min((uint32_t)CHUNK, lend - c0);
            wave_sync();
            if (tmask) glds_f4(t.p4 + c0, p4s, lane, cn);
            stage_values<NV>(vt, c0, vs, lane, cn);
            wait_vm0();
            wave_sync();
            if (full) {
                float a[NV];
#pragma unroll
                for (int c = 0; c < NV; ++c) a[c] = frow[c * 64];
#pragma unroll 1
                for (uint32_t u = 0; u < cn; ++u) {
#pragma unroll
                    for (int c = 0; c < NV; ++c) a[c] += vs[u * NV + c];
                }
#pragma unroll
                for (int c = 0; c < NV; ++c) frow[c * 64] = a[c];
            }
            if (tmask) {
                if (plain_leaf)
                    prof_chunk<false, NV>(p4s, vs, cn, acc, thr, tmask, base, ev, (uint32_t)nr, lane,
                                          qx, qy, qz, L);
                else
                    prof_chunk<M, NV>(p4s, vs, cn, acc, thr, tmask, base, ev, (uint32_t)nr, lane, qx,
                                      qy, qz, L);
            }
        }
    }
}

template <bool PER, int NV>
__global__ void __launch_bounds__(TBMAX)
ball_profile_kernel(DevTree t, const uint32_t *__restrict__ linfo, const float *__restrict__ q,
                    const float *__restrict__ scale, const uint32_t *__restrict__ order,
                    uint32_t m, ProfRadii R, int nr, PadLeaves pad, const float *__restrict__ vt,
                    float *__restrict__ out_sum) {
    extern __shared__ float4 prof_lds[];
    const int lane = threadIdx.x & 63, wave = wave_id();
    const uint32_t wpb = blockDim.x >> 6;
    char *const wbase = (char *)prof_lds + (size_t)wave * prof_wave_bytes(nr, NV);
    float4 *const p4s = (float4 *)wbase;
    float *const vs = (float *)(wbase + CHUNK * 16);
    float *const acc = vs + CHUNK * NV;
    float *const thr = acc + (nr + 1) * NV * 64;
    const uint32_t gq = (xcd_block(blockIdx.x, gridDim.x) * wpb + wave) * 64u + lane;
    const float L = t.box;
    const PacketQuery p = packet_query<PER>(q, order, gq, m, L);
    const float qx = p.x, qy = p.y, qz = p.z;
    const bool valid = p.valid, inside = p.inside;
    const float sc = (valid && scale) ? scale[p.qo] : 1.0f;
    // a lane without a query, outside the box or with a NaN, infinite or
    // negative scale walks nothing: every threshold and the bound are -inf
    const bool ok = valid && inside && scale_ok(sc);
    float kth = -INFINITY;
    for (int k = 0; k < nr; ++k) {
        kth = prof_thr(R.r[k], sc, ok);
        thr[k * 64 + lane] = kth;
    }
    for (int j = 0; j < (nr + 1) * NV; ++j) acc[j * 64 + lane] = 0.0f;
    wave_sync();
    // every lane's own largest ball clears the box faces by a margin r' > e_i,nr-1
    // (a lane without bins clears them too): the plain formulas then give the
    // periodic ones' bits for every point within it and fail the test for every
    // point beyond (ball.hip ball_fill_kernel), so the packet walks and tests
    // with them
    const bool plain = packet_plain<PER>(!(kth < 0.0f), kth, qx, qy, qz, L);
    if (plain)
        ball_profile_walk<PER, false, NV>(t, linfo, pad, vt, p4s, vs, acc, thr, nr, lane, qx, qy,
                                          qz, kth);
    else
        ball_profile_walk<PER, PER, NV>(t, linfo, pad, vt, p4s, vs, acc, thr, nr, lane, qx, qy, qz,
                                        kth);
    wave_sync();
    // the lane's nr * NV bin sums; a query without bins gets its zero rows; a
    // periodic query outside the box is the brute kernel's.  (The id again: not
    // kept live through the walk.)
    if (valid && inside) {
        const uint32_t qo = order[gq];
        float *const row = out_sum + (size_t)qo * (uint32_t)(nr * NV);
        for (int j = 0; j < nr * NV; ++j) row[j] = acc[j * 64 + lane];
    }
}

// Periodic queries outside [0, L]^3 (unvalidated input): no box bound is valid
// for the per-axis metric there, so every point is tested, with the
// reference-exact point_d2.  One wave per listed query (the list's length is in
// device memory; a fixed grid strides over it): lane l bins the tree positions
// l, l + 64, ... in order into column l of acc[(nr + 1)][nv][64], then the
// columns are added in a fixed pairwise order, so the result does not depend on
// scheduling.
__global__ void __launch_bounds__(64)
ball_profile_brute_kernel(const float *__restrict__ px, const float *__restrict__ py,
                          const float *__restrict__ pz, uint32_t n8, float L,
                          const float *__restrict__ q, const float *__restrict__ scale, const uint32_t *__restrict__ list,
                          const uint32_t *__restrict__ nout, ProfRadii R, int nr,
                          const float *__restrict__ vt, int nv, float *__restrict__ out_sum) {
    extern __shared__ float4 prof_lds[];
    float *const acc = (float *)prof_lds;
    float *const thr = acc + (nr + 1) * nv * 64;
    const int lane = threadIdx.x;
    const uint32_t total = __builtin_amdgcn_readfirstlane(*nout);
    const int ne = nr * nv;
    for (uint32_t j = blockIdx.x; j < total; j += gridDim.x) {
        const uint32_t qo = list[j];
        const float qx = q[3 * (size_t)qo], qy = q[3 * (size_t)qo + 1], qz = q[3 * (size_t)qo + 2];
        const float sc = scale ? scale[qo] : 1.0f;
        const bool ok = scale_ok(sc);
#pragma unroll 1
        for (int k = 0; k < nr; ++k) {
            const float tk = prof_thr(R.r[k], sc, ok);
            if (lane == 0) thr[k] = tk;
        }
#pragma unroll 1
        for (int e = 0; e < ne + nv; ++e) acc[e * 64 + lane] = 0.0f;
        __syncthreads();
        if (ok) {
            for (uint32_t p = lane; p < n8; p += 64) {
                const float d2 = point_d2<true>(qx, qy, qz, px[p], py[p], pz[p], L);
                uint32_t b = 0;
#pragma unroll 1
                for (int k = 0; k < nr; ++k) b += !(d2 <= thr[k]) ? 1u : 0u;
                float *const row = acc + (b * (uint32_t)nv) * 64u + lane;
#pragma unroll 1
                for (int c = 0; c < nv; ++c) row[c * 64] += vt[(size_t)p * (uint32_t)nv + c];
            }
        }
        __syncthreads();
#pragma unroll 1
        for (int o = 32; o > 0; o >>= 1) {
            if (lane < o)
#pragma unroll 1
                for (int e = 0; e < ne; ++e) acc[e * 64 + lane] += acc[e * 64 + lane + o];
            __syncthreads();
        }
        for (int e = lane; e < ne; e += 64) out_sum[(size_t)qo * (uint32_t)ne + e] = acc[e * 64];
        __syncthreads(); // acc is read before the next query's zeros land
    }
}

template <int NV>
void launch_profile_n(const Tree &t, const float *q, const float *scale, const uint32_t *order,
                      uint32_t m, const ProfRadii &R, int nr, const PadLeaves &pad,
                      const float *vt, float *out_sum, hipStream_t s) {
    const uint32_t wb = prof_wave_bytes(nr, NV);
    const uint32_t wpb = 4 * wb <= LDS_BLOCK ? 4u : 2 * wb <= LDS_BLOCK ? 2u : 1u;
    const unsigned blocks = (unsigned)(((uint64_t)m + 64 * wpb - 1) / (64 * wpb));
    if (t.periodic)
        ball_profile_kernel<true, NV><<<blocks, 64 * wpb, wpb * wb, s>>>(
            view(t), t.leafinfo, q, scale, order, m, R, nr, pad, vt, out_sum);
    else
        ball_profile_kernel<false, NV><<<blocks, 64 * wpb, wpb * wb, s>>>(
            view(t), t.leafinfo, q, scale, order, m, R, nr, pad, vt, out_sum);
}

} // namespace

void launch_ball_profile(const Tree &t, const float *q, const float *scale, const uint32_t *order,
                         uint32_t m, const ProfRadii &R, int nr, const float *vt, int nv,
                         float *out_sum, hipStream_t s) {
    if (m == 0) return;
    const PadLeaves pad = pad_leaves_of(t);
    with_constant<1, 2, 3, 4>(nv, [&](auto NV) {
        launch_profile_n<NV()>(t, q, scale, order, m, R, nr, pad, vt, out_sum, s);
    });
}

void launch_ball_profile_outside_dev(const Tree &t, const float *q, const float *scale,
                                     const uint32_t *list, const uint32_t *nout,
                                     const ProfRadii &R, int nr, const float *vt, int nv,
                                     float *out_sum, hipStream_t s) {
    const size_t lds = (size_t)((nr + 1) * nv * 64 + NBKD_MAX_RADII) * 4;
    ball_profile_brute_kernel<<<1024, 64, lds, s>>>(t.x, t.y, t.z, (uint32_t)t.n8, t.box, q, scale,
                                                   list, nout, R, nr, vt, nv, out_sum);
}

} // namespace nbkd
