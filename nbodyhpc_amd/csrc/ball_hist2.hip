// Anisotropic pair counts (NEW, nbkd_query_ball_hist2): every (query, point)
// pair classified on two coordinates in one tree walk, (rp, pi) or (s, mu)
// about a line of sight along one axis.  The sibling of ball_hist.hip: 64-query
// packets, one query per lane, on the shared packet walk (packet.hpp), leaves
// staged with glds_f4 from p4, the per-axis squares of metric.hpp
// (point_axes_fast: the terms point_d2_fast adds up, so s2 is the tree's d2).
//
// Bins.  With T1[k] = fl(e1[k]^2) and T2[l] = fl(e2[l]^2) (formed on the host):
//   RPPI  b1 = #{k : !(rp2 <= T1[k])},  b2 = #{l : !(pi2 <= T2[l])}
//   SMU   b1 = #{k : !(s2  <= T1[k])},  b2 = #{l : !(pi2 <= fl(T2[l] * s2))}
// pi2 = a_los, rp2 = fl(a_u + a_v) (u < v the other two axes), s2 =
// fl(fl(ax + ay) + az).  A pair counts iff b1 < n1 and b2 < n2.
//
// Histogram.  n1 * n2 bins cannot be kept per lane (32 * 64 * 64 lanes * 4 B =
// 512 KiB), so a wave keeps R interleaved copies of one histogram in LDS, word
// (bin * R + (lane & (R - 1))), R a power of two with n1 * n2 * R <= 2048 words
// (8 KiB); lanes add with LDS integer atomics whose result is not used
// (ds_add_u32).  Neighbouring queries put the same staged point into the same
// bin most of the time, and the copies cut that same-address serialisation by
// R, but they cost LDS and with it waves per CU: measured at 16 x 16 bins, R = 1
// and 2 run alike and R = 8 (the whole 8 KiB) 38 to 49 % slower, so R = 2 is the
// default (nbkd_set_tuning("hist2_copies")).
// At the end of the packet (and whenever the wrap bound below is near) the wave
// folds the copies and adds the nonzero bins to the device totals with 64-bit
// integer atomics.  Counts are integers everywhere: the result does not depend
// on R, the flush interval, the grid or the order of the adds.
//
// Per leaf a lane compares the per-axis bounds of the tight box, lb_a <= a_a <=
// ub_a (box_lb_axis and the larger end value; both monotone in the roundings
// the point formula uses), combined in the association of the coordinate they
// bound, with the thresholds: thresholds below the lower bound fail for every
// point of the leaf, thresholds at or above the upper bound hold for every
// point.  A leaf whose lower bounds pass the last threshold of either axis
// cannot reach a bin for that lane (this is what keeps an elongated cylinder
// from evaluating its bounding ball); a leaf no lane needs is not staged.  A
// lane whose bounds leave one bin on both axes (and a leaf without padding
// points) adds the leaf's count to that bin without evaluating a point.  The
// others evaluate the staged points against the thresholds between the
// wave-wide smallest lower and largest upper index only.
//
// Observer frame (nbkd_query_ball_hist2_obs, LOS == HIST2_LOS_OBS): the line of
// sight of a pair runs from the observer o through the pair's midpoint.  With
// s = p - q and l = fl(fl(p - o) + fl(q - o)) (twice the midpoint's offset),
// pi2 = min(fl(fl(dot(s, l)^2) / l2), s2) and rp2 = fl(s2 - pi2): hist2_coords_obs,
// the header's formulas operation by operation.  Non-periodic trees only.  The
// per-axis cylinder bounds above do not hold for it; per leaf only
// lb_s2 <= s2 <= ub_s2 and 0 <= rp2, pi2 <= s2 do (the clamp and s2 - pi2 with
// 0 <= pi2 <= s2 keep both in float32), so a lane needs a leaf iff lb_s2 <= the
// walk's bound, every lower index but SMU's first axis is 0 and every upper
// bound is ub_s2.
#include <algorithm>
#include <cfloat>

#include "internal.hpp"
#include "metric.hpp"
#include "packet.hpp"

namespace nbkd {
namespace {
using namespace dev;

constexpr int TB = 256;
constexpr int WPB = TB / 64;
constexpr int EV = 4;     // staged points evaluated per step of the threshold loops
// T1, T2 and the ids of the padded leaves (in LDS, not in NBKD_PAD_LEAVES SGPRs:
// with them the periodic instances spilled scalar registers)
constexpr uint32_t THR_WORDS = NBKD_MAX_RADII + NBKD_MAX_LOS_BINS + NBKD_PAD_LEAVES;

// one wave's LDS: the staged points, the histogram copies, the thresholds and
// padded-leaf ids
__host__ __device__ constexpr uint32_t hist2_wave_bytes(uint32_t words) {
    // (the words rounded up to 16 B: the next wave's staged float4s stay aligned)
    return (uint32_t)(CHUNK * 16 + ((words + 3u) & ~3u) * 4 + THR_WORDS * 4);
}
static_assert(WPB * hist2_wave_bytes(HIST2_LDS_WORDS) <= 64 * 1024,
              "one block shape serves every bin count: 4 waves stay below 64 KiB");

// A wave's LDS words are uint32 and must not wrap between two flushes.  Every
// add is counted against `room` before it is made: a leaf visit adds at most
// one per (lane, point of the leaf) = 64 * count, over all bins and copies
// together.  The wave flushes before a visit whose 64 * count exceeds the room
// left of 2^32 - 1, so the sum of all words, and with it every word and every
// fold of R copies, stays below 2^32.  (A leaf holds fewer than 2^26 points:
// positions are 32-bit and 64 * count is formed in 64 bits and compared first.)
constexpr uint32_t ROOM = 0xFFFFFFFFu;

struct Hist2Ctx {
    uint32_t *hist;             // LDS: (nbins << rshift) words
    const float *thr1, *thr2;   // LDS: T1[n1], T2[n2]
    const uint32_t *padl;       // LDS: the padded leaves' ids
    unsigned long long *totals; // device: nbins counters
    int n1, n2, rshift;
    uint32_t flush_visits; // 0: by the wrap bound only
};

// fold the copies, add the nonzero bins to the totals, zero the words
__device__ __forceinline__ void hist2_flush(const Hist2Ctx &c, const int lane) {
    wave_sync();
    const int nbins = c.n1 * c.n2, R = 1 << c.rshift;
    for (int e = lane; e < nbins; e += 64) {
        uint32_t v = 0;
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
        for (int r = 0; r < R; ++r) {
            v += c.hist[(e << c.rshift) + r];
            c.hist[(e << c.rshift) + r] = 0;
        }
        if (v) atomicAdd(&c.totals[e], (unsigned long long)v);
    }
    wave_sync();
}

// (the line of sight is a template parameter: as a run-time value its selects
// compile to branches on lane masks kept in SGPR pairs, which spilled)
template <int MODE, int LOS>
__device__ __forceinline__ void hist2_coords(const float ax, const float ay, const float az,
                                             float &x1, float &pi2) {
    pi2 = LOS == 0 ? ax : (LOS == 1 ? ay : az);
    if constexpr (MODE == NBKD_HIST2_RPPI)
        x1 = LOS == 0 ? ay + az : (LOS == 1 ? ax + az : ax + ay);
    else
        x1 = (ax + ay) + az;
}

// the observer frame: the lane's query relative to the observer, fl(q - o),
// formed once per lane, and the observer (wave-uniform)
struct Hist2Obs {
    float ox, oy, oz, qox, qoy, qoz;
};

// (x1, pi2) of one pair in the observer frame, the operations of include/nbkd.h
// in their order (no contraction: -ffp-contract=off; x / l2 is the correctly
// rounded division).  fminf takes s2 where the quotient is NaN (inf / inf).
template <int MODE>
__device__ __forceinline__ void hist2_coords_obs(const float qx, const float qy, const float qz,
                                                 const float px, const float py, const float pz,
                                                 const Hist2Obs &o, float &x1, float &pi2) {
    const float sx = px - qx, sy = py - qy, sz = pz - qz;
    const float s2 = (sx * sx + sy * sy) + sz * sz;
    const float lx = (px - o.ox) + o.qox, ly = (py - o.oy) + o.qoy, lz = (pz - o.oz) + o.qoz;
    const float dot = (sx * lx + sy * ly) + sz * lz;
    const float l2 = (lx * lx + ly * ly) + lz * lz;
    const float x = dot * dot;
    pi2 = l2 > 0.0f ? fminf(x / l2, s2) : 0.0f;
    x1 = MODE == NBKD_HIST2_RPPI ? s2 - pi2 : s2;
}

// the staged points against the thresholds [k0, k1) and [l0, l1) (every
// evaluating lane fails the ones below and passes the ones above)
template <bool M, int MODE, int LOS>
__device__ __forceinline__ void hist2_chunk(const float4 *p4s, const uint32_t cn,
                                            const Hist2Ctx &c, const int k0, const int k1,
                                            const int l0, const int l1, const bool ev,
                                            const uint32_t copy, const float qx, const float qy,
                                            const float qz, const float L, const Hist2Obs &o) {
#pragma unroll 1
    for (uint32_t u = 0; u < cn; u += EV) {
        float x1[EV], pi2[EV];
        uint32_t b1[EV], b2[EV];
#pragma unroll
        for (int i = 0; i < EV; ++i) {
            const float4 a = p4s[u + i];
            if constexpr (LOS == HIST2_LOS_OBS) {
                hist2_coords_obs<MODE>(qx, qy, qz, a.x, a.y, a.z, o, x1[i], pi2[i]);
            } else {
                float ax, ay, az;
                point_axes_fast<M>(qx, qy, qz, a.x, a.y, a.z, L, ax, ay, az);
                hist2_coords<MODE, LOS>(ax, ay, az, x1[i], pi2[i]);
            }
            b1[i] = (uint32_t)k0;
            b2[i] = (uint32_t)l0;
        }
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
        for (int k = k0; k < k1; ++k) {
            const float t = c.thr1[k];
#pragma unroll
            for (int i = 0; i < EV; ++i) b1[i] += !(x1[i] <= t) ? 1u : 0u;
        }
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
        for (int l = l0; l < l1; ++l) {
            const float t = c.thr2[l];
#pragma unroll
            for (int i = 0; i < EV; ++i) {
                const float tl = MODE == NBKD_HIST2_SMU ? t * x1[i] : t;
                b2[i] += !(pi2[i] <= tl) ? 1u : 0u;
            }
        }
        if (ev) {
#pragma unroll
            for (int i = 0; i < EV; ++i)
                if (u + i < cn && b1[i] < (uint32_t)c.n1 && b2[i] < (uint32_t)c.n2)
                    atomicAdd(&c.hist[((b1[i] * (uint32_t)c.n2 + b2[i]) << c.rshift) + copy], 1u);
        }
    }
}

template <bool PER, bool M, int MODE, int LOS>
__device__ __forceinline__ void hist2_walk(const DevTree &t, const uint32_t *__restrict__ linfo,
                                           float4 *p4s, const Hist2Ctx &c,
                                           const int lane, const float qx, const float qy,
                                           const float qz, const float kth, const bool active,
                                           const Hist2Obs &o) {
    static_assert(LOS != HIST2_LOS_OBS || (!PER && !M), "pairwise lines of sight: no periodic tree");
    const float L = t.box;
    const cnode_ptr cnodes = (cnode_ptr)t.nodes;
    const cbox_ptr cboxes = (cbox_ptr)t.nbox;
    const int n1 = c.n1, n2 = c.n2;
    const float t1max = c.thr1[n1 - 1], t2max = c.thr2[n2 - 1];
    const uint32_t copy = (uint32_t)lane & ((1u << c.rshift) - 1u);
    PacketWalk w;
    walk_begin(w);
    uint32_t lpos = 0, lend = 0, visits = 0, room = ROOM, since = 0;
    while (walk_next_leaf<M, false, false>(w, cnodes, cboxes, qx, qy, qz, kth, L, lpos, lend,
                                           visits)) {
        float tb[6];
        leaf_tight_box(linfo, w.node, tb);
        // per-axis bounds of the squares, then of the two coordinates, each in
        // the association of the coordinate it bounds
        const float lx = box_lb_axis<M>(qx, tb[0], tb[1], L);
        const float ly = box_lb_axis<M>(qy, tb[2], tb[3], L);
        const float lz = box_lb_axis<M>(qz, tb[4], tb[5], L);
        float lb1, lbp;
        bool need;
        if constexpr (LOS == HIST2_LOS_OBS) {
            // lb_s2 <= s2 for every point (box_lb2's association); rp2 and pi2
            // reach down to 0 whatever the leaf.  kth is the walk's bound on s2
            // for an active lane, -inf otherwise.
            const float lbs = (lx + ly) + lz;
            lb1 = MODE == NBKD_HIST2_SMU ? lbs : 0.0f;
            lbp = 0.0f;
            need = lbs <= kth;
        } else {
            hist2_coords<MODE, LOS>(lx, ly, lz, lb1, lbp);
            need = active && lb1 <= t1max;
            if constexpr (MODE == NBKD_HIST2_RPPI) need = need && lbp <= t2max;
        }
        if (!__any(need)) continue;
        // (a leaf holding padding points, in no bin, is always evaluated, against
        // every threshold: the upper bounds do not hold for them)
        const bool padded =
            __any(lane < NBKD_PAD_LEAVES && c.padl[lane & (NBKD_PAD_LEAVES - 1)] == w.node);
        const float hx = fmaxf(fabsf(tb[0] - qx), fabsf(tb[1] - qx));
        const float hy = fmaxf(fabsf(tb[2] - qy), fabsf(tb[3] - qy));
        const float hz = fmaxf(fabsf(tb[4] - qz), fabsf(tb[5] - qz));
        float ub1, ubp;
        if constexpr (LOS == HIST2_LOS_OBS) // rp2 <= s2 and pi2 <= s2 <= ub_s2 (box_ub2)
            ub1 = ubp = (hx * hx + hy * hy) + hz * hz;
        else
            hist2_coords<MODE, LOS>(hx * hx, hy * hy, hz * hz, ub1, ubp);
        // lo <= b <= hi for every point of the leaf, on both axes.  SMU: a
        // threshold l fails for every point when lbp > fl(T2[l] * ub1) (the
        // product is monotone in s2 <= ub1) and holds when ubp <= fl(T2[l] * lb1).
        uint32_t lo1 = 0, hi1 = 0, lo2 = 0, hi2 = 0;
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
        for (int k = 0; k < n1; ++k) {
            const float tk = c.thr1[k];
            lo1 += !(lb1 <= tk) ? 1u : 0u;
            hi1 += !(ub1 <= tk) ? 1u : 0u;
        }
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
        for (int l = 0; l < n2; ++l) {
            const float tl = c.thr2[l];
            // (ub1 clamped: an upper bound that overflowed times a zero mu edge
            // would be NaN and fail the threshold for points with pi2 == 0; a
            // point whose own s2 is infinite has b1 == n1, whatever b2)
            const float tlo = MODE == NBKD_HIST2_SMU ? tl * fminf(ub1, FLT_MAX) : tl;
            const float thi = MODE == NBKD_HIST2_SMU ? tl * lb1 : tl;
            lo2 += !(lbp <= tlo) ? 1u : 0u;
            hi2 += !(ubp <= thi) ? 1u : 0u;
        }
        const uint32_t cnt = lend - lpos;
        // the wrap bound: this visit adds at most 64 * cnt
        const uint64_t adds = 64ull * cnt;
        if (adds > room || (c.flush_visits != 0 && since >= c.flush_visits)) {
            hist2_flush(c, lane);
            room = ROOM;
            since = 0;
        }
        room -= adds < room ? (uint32_t)adds : room;
        ++since;
        const bool whole = need && !padded && lo1 == hi1 && lo2 == hi2;
        if (whole && lo1 < (uint32_t)n1 && lo2 < (uint32_t)n2)
            atomicAdd(&c.hist[((lo1 * (uint32_t)n2 + lo2) << c.rshift) + copy], cnt);
        const bool ev = need && !whole;
        if (!__any(ev)) continue;
        // the wave's threshold ranges: the smallest lo and the largest hi of
        // the evaluating lanes (all of them for a padded leaf)
        int k0 = 0, k1 = n1, l0 = 0, l1 = n2;
        if (!padded) {
            while (!__any(ev && lo1 <= (uint32_t)k0)) ++k0;
            while (k1 > k0 && !__any(ev && hi1 >= (uint32_t)k1)) --k1;
            while (!__any(ev && lo2 <= (uint32_t)l0)) ++l0;
            while (l1 > l0 && !__any(ev && hi2 >= (uint32_t)l1)) --l1;
        }
        // the plain squares where no evaluating lane wraps around (wrap_free)
        const bool plain_leaf = !M || __all(!ev || wrap_free(qx, qy, qz, tb, L));
        for (uint32_t c0 = lpos; c0 < lend; c0 += CHUNK) {
            const uint32_t cn = min((uint32_t)CHUNK, lend - c0);
            stage_points(t.p4, c0, p4s, lane, cn);
            if (plain_leaf)
                hist2_chunk<false, MODE, LOS>(p4s, cn, c, k0, k1, l0, l1, ev, copy, qx, qy, qz, L,
                                              o);
            else
                hist2_chunk<M, MODE, LOS>(p4s, cn, c, k0, k1, l0, l1, ev, copy, qx, qy, qz, L, o);
        }
    }
}

template <bool PER, int MODE, int LOS>
__global__ void __launch_bounds__(TB, 8)
ball_hist2_kernel(DevTree t, const uint32_t *__restrict__ linfo, const float *__restrict__ q,
                  const uint32_t *__restrict__ order, uint32_t m, Hist2Thr T, Hist2Par P,
                  PadLeaves pad, unsigned long long *__restrict__ totals) {
    extern __shared__ float4 hist2_lds[];
    const int lane = threadIdx.x & 63, wave = wave_id();
    const uint32_t words = (uint32_t)(P.n1 * P.n2) << P.rshift;
    char *const wbase = (char *)hist2_lds + (size_t)wave * hist2_wave_bytes(words);
    float4 *const p4s = (float4 *)wbase;
    uint32_t *const hist = (uint32_t *)(wbase + CHUNK * 16);
    float *const thr1 = (float *)(wbase + CHUNK * 16 + ((words + 3u) & ~3u) * 4);
    float *const thr2 = thr1 + NBKD_MAX_RADII;
    uint32_t *const padl = (uint32_t *)(thr2 + NBKD_MAX_LOS_BINS);
    if (lane < P.n1) thr1[lane] = T.t1[lane];
    if (lane < P.n2) thr2[lane] = T.t2[lane];
    if (lane < NBKD_PAD_LEAVES) padl[lane] = pad.id[lane];
    for (uint32_t e = lane; e < words; e += 64) hist[e] = 0;
    wave_sync();
    const Hist2Ctx c{hist, thr1, thr2, padl, totals, P.n1, P.n2, P.rshift, P.flush_visits};
    const uint32_t gq = (xcd_block(blockIdx.x, gridDim.x) * WPB + wave) * 64u + lane;
    // (packet.hpp packet_query written out: through the helper the periodic
    // instances take other SGPRs and the 16 x 40 (rp, pi) case ran 0.25 % slower,
    // profiles/r12a_radius_helpers_ab.txt)
    const bool valid = gq < m;
    const uint32_t qo = valid ? order[gq] : 0u;
    const float qx = valid ? q[3 * (size_t)qo] : 0.0f;
    const float qy = valid ? q[3 * (size_t)qo + 1] : 0.0f;
    const float qz = valid ? q[3 * (size_t)qo + 2] : 0.0f;
    const float L = t.box;
    const bool inside =
        !PER || (qx >= 0.0f && qx <= L && qy >= 0.0f && qy <= L && qz >= 0.0f && qz <= L);
    const bool active = valid && inside;
    // the walk's bound on s2 (formed on the host, launch_ball_hist2)
    const float r2 = P.bound;
    const float kth = active ? r2 : -INFINITY;
    // every active lane's ball of the bound clears the box faces: the plain
    // formulas (the per-axis squares are then the periodic ones' bits for every
    // point inside the ball, and a point outside it is in no bin either way)
    const bool plain = packet_plain<PER>(active, r2, qx, qy, qz, L);
    // (read by the observer-frame instances only)
    const Hist2Obs o{P.obs[0], P.obs[1], P.obs[2], qx - P.obs[0], qy - P.obs[1], qz - P.obs[2]};
    if (plain)
        hist2_walk<PER, false, MODE, LOS>(t, linfo, p4s, c, lane, qx, qy, qz, kth, active, o);
    else
        hist2_walk<PER, PER, MODE, LOS>(t, linfo, p4s, c, lane, qx, qy, qz, kth, active, o);
    hist2_flush(c, lane);
}

// Periodic queries outside [0, L]^3 (listed by outside_box_kernel, the length
// in device memory): every point tested with the reference-exact three-image
// squares (point_axes<true>), as hist_brute_dev_kernel does; each pair in a bin
// adds to the totals directly.
template <int MODE, int LOS>
__global__ void __launch_bounds__(TB)
hist2_brute_dev_kernel(DevTree t, const float *__restrict__ q, const uint32_t *__restrict__ list,
                       const uint32_t *__restrict__ nout, uint32_t ntiles, Hist2Thr T,
                       Hist2Par P, unsigned long long *__restrict__ totals) {
    __shared__ float thr1[NBKD_MAX_RADII], thr2[NBKD_MAX_LOS_BINS];
    if (threadIdx.x < (uint32_t)P.n1) thr1[threadIdx.x] = T.t1[threadIdx.x];
    if (threadIdx.x < (uint32_t)P.n2) thr2[threadIdx.x] = T.t2[threadIdx.x];
    __syncthreads();
    const uint64_t total = (uint64_t)__builtin_amdgcn_readfirstlane(*nout) * ntiles;
    const float L = t.box;
    for (uint64_t w = blockIdx.x; w < total; w += gridDim.x) {
        const BruteTile b = brute_tile<TB>(w, ntiles, list, q);
        for (int u = 0; u < BR_ITEMS; ++u) {
            const uint32_t p = b.base + u * TB;
            if (p >= t.n8) continue;
            float ax, ay, az, x1, pi2;
            point_axes<true>(b.qx, b.qy, b.qz, t.x[p], t.y[p], t.z[p], L, ax, ay, az);
            hist2_coords<MODE, LOS>(ax, ay, az, x1, pi2);
            // (padding points: x1 is infinite, b1 == n1)
            uint32_t b1 = 0, b2 = 0;
            for (int k = 0; k < P.n1; ++k) b1 += !(x1 <= thr1[k]) ? 1u : 0u;
            if (b1 >= (uint32_t)P.n1) continue;
            for (int l = 0; l < P.n2; ++l) {
                const float tl = MODE == NBKD_HIST2_SMU ? thr2[l] * x1 : thr2[l];
                b2 += !(pi2 <= tl) ? 1u : 0u;
            }
            if (b2 < (uint32_t)P.n2) atomicAdd(&totals[b1 * (uint32_t)P.n2 + b2], 1ull);
        }
    }
}

} // namespace

// The walk's bound on s2 = fl(fl(ax + ay) + az) of a pair that is in some bin.
// SMU: s2 <= T1[n1-1] is the bin test itself.  RPPI, A = T1[n1-1], B = T2[n2-1]:
//   los = 2: rp2 = fl(ax + ay) <= A and az <= B, and s2 = fl(rp2 + az) is that
//     very association, so s2 <= fl(A + B) by monotone rounding.
//   los = 0 or 1 (say 0: ax <= B, fl(ay + az) <= A): the association differs
//     and s2 can lie above fl(A + B).  With u = 2^-24 every float32 sum is
//     (x + y)(1 + d), |d| <= u (sums never lose bits to underflow), so
//     ay + az <= A / (1 - u), the exact sum S = ax + ay + az <= (A + B) / (1 - u)
//     and s2 <= S (1 + u)^2 <= (A + B)(1 + u)^2 / (1 - u) < (A + B)(1 + 4u).
//     The bound W = fl(fl(A + B) * (1 + 2^-21)) >= (A + B)(1 - u)(1 + 8u)(1 - u)
//     > (A + B)(1 + 5u) covers it.  Where the product underflows (A + B below
//     2^-126) every sum involved is exact, s2 = S <= A + B = fl(A + B), and W >=
//     fl(A + B) because a product by a factor >= 1 rounds monotonically.
//   observer frame (los = HIST2_LOS_OBS): rp2 = fl(s2 - pi2) <= A and pi2 <= B.
//     The difference rounds as (s2 - pi2)(1 + d), |d| <= u (exactly in the
//     subnormal range: a float32 difference loses no bits to underflow), so
//     s2 - pi2 <= A / (1 - u), s2 <= A / (1 - u) + B <= (A + B) / (1 - u) <
//     (A + B)(1 + 2u), below the (A + B)(1 + 5u) that W exceeds; where the
//     product underflows the difference is exact and s2 <= A + B = fl(A + B) <= W.
//     SMU is the bin test itself there too.
// An overflowing bound is infinite: every leaf is then walked, which is valid.
static float hist2_walk_bound(const Hist2Thr &thr, const Hist2Par &par) {
    const float A = thr.t1[par.n1 - 1];
    if (par.mode == NBKD_HIST2_SMU) return A;
    const float ab = A + thr.t2[par.n2 - 1];
    if (par.los == 2) return ab;
    const float w = ab * (1.0f + 0x1p-21f);
    return w;
}

int hist2_copies_shift(int nbins, int copies) {
    int rshift = 0;
    const int want = copies > 0 ? copies : HIST2_DEFAULT_COPIES;
    while ((2 << rshift) <= want && ((uint32_t)nbins << (rshift + 1)) <= HIST2_LDS_WORDS) ++rshift;
    return rshift;
}

void launch_ball_hist2(const Tree &t, const float *q, const uint32_t *order, uint32_t m,
                       const Hist2Thr &thr, Hist2Par par, unsigned long long *totals,
                       hipStream_t s) {
    const PadLeaves pad = pad_leaves_of(t);
    par.bound = hist2_walk_bound(thr, par);
    const unsigned blocks = (unsigned)(((uint64_t)m + TB - 1) / TB);
    const uint32_t words = (uint32_t)(par.n1 * par.n2) << par.rshift;
    // (one block shape: 4 waves of at most 8 KiB of histogram, 38 KiB in all)
    const size_t lds = (size_t)WPB * hist2_wave_bytes(words);
    const auto launch = [&](auto PERV, auto MODE, auto LOS) {
        ball_hist2_kernel<PERV() != 0, MODE(), LOS()><<<blocks, TB, lds, s>>>(
            view(t), t.leafinfo, q, order, m, thr, par, pad, totals);
    };
    with_constant<NBKD_HIST2_SMU, NBKD_HIST2_RPPI>(par.mode, [&](auto MODE) {
        if (par.los == HIST2_LOS_OBS) // (non-periodic trees only: checked by the C entry point)
            launch(std::false_type{}, MODE, std::integral_constant<int, HIST2_LOS_OBS>{});
        else
            with_constant<0, 1, 2>(par.los, [&](auto LOS) {
                with_constant<1, 0>(t.periodic, [&](auto PERV) { launch(PERV, MODE, LOS); });
            });
    });
}

void launch_ball_hist2_outside_dev(const Tree &t, const float *q, const uint32_t *list,
                                   const uint32_t *nout, const Hist2Thr &thr, Hist2Par par,
                                   unsigned long long *totals, hipStream_t s) {
    const uint32_t ntiles = (uint32_t)((t.n8 + TB * BR_ITEMS - 1) / (TB * BR_ITEMS));
    with_constant<NBKD_HIST2_SMU, NBKD_HIST2_RPPI>(par.mode, [&](auto MODE) {
        with_constant<0, 1, 2>(par.los, [&](auto LOS) {
            hist2_brute_dev_kernel<MODE(), LOS()><<<2048, TB, 0, s>>>(view(t), q, list, nout, ntiles,
                                                                      thr, par, totals);
        });
    });
}

} // namespace nbkd
