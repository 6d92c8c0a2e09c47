// Kernel-weighted sums over per-query balls (NEW, nbkd_query_ball_sum: the
// reference has neither a radius search nor a reduction over neighbours):
//   out_sum[i, c] = sum_j values[j, c] * K(d_ij / h_i)  over  d2(i, j) <= h_i*h_i,
// the gather form of SPH.  The membership test is ball.hip's (the f32 point
// metric against a squared radius), with each lane's bound its own h_i*h_i:
// the packet walk's bound `kth` is per lane already.
//
// ball_sum_kernel is ball.hip's CSR fill (ball_fill_walk) with a register
// accumulate where the fill stores an id: 64-query packets, one wave each, the
// shared packet walk behind packet.hpp's prologue (packet_query, packet_plain),
// leaf chunks staged into LDS from Tree::p4 and, beside them, the chunk's rows
// of the values in tree order (vt, written once per call by
// ball_sum_gather_kernel; stage_values); each lane loops over the staged points.
// Every (query, channel) is summed by one lane into one f32 accumulator in the
// walk's order: no floating-point atomics, identical calls give identical bits.
//
// Periodic queries outside [0, L]^3 are excluded here (their minimum-image
// pruning is not a bound) and answered by ball_sum_brute_kernel below.
#include <algorithm>

#include "internal.hpp"
#include "metric.hpp"
#include "packet.hpp"

namespace nbkd {
namespace {
using namespace dev;

constexpr int TB = 256;
constexpr int WPB = TB / 64;

// 64 * (16 + 4 NV) bytes per wave
template <int NV> struct alignas(16) SumLds {
    float4 p4[CHUNK];    // the staged points: x, y, z, id bits (Tree::p4)
    float v[CHUNK * NV]; // their rows of vt
};

// K(u), u = min(sqrt(d2) / h, 1), in the f32 steps nbkd.h states (the build is
// -ffp-contract=off: no multiply is fused into an add)
template <int KERN> __device__ __forceinline__ float sph_kernel(float d2, float inv) {
    if constexpr (KERN == NBKD_KERNEL_TOPHAT) {
        return 1.0f;
    } else {
        const float u = fminf(sqrtf(d2) * inv, 1.0f);
        const float w = 1.0f - u;
        if constexpr (KERN == NBKD_KERNEL_CUBIC) {
            const float uu = u * u;
            const float inner = (1.0f - 6.0f * uu) + 6.0f * (uu * u);
            const float outer = 2.0f * ((w * w) * w);
            return u <= 0.5f ? inner : outer;
        } else {
            const float w2 = w * w;
            return (w2 * w2) * (1.0f + 4.0f * u);
        }
    }
}

// the lane's squared radius, or -inf for a radius that is NaN, infinite or
// negative (an empty ball); an overflowing square counts as FLT_MAX, so the
// padding points (d2 = inf) are never inside
__device__ __forceinline__ float ball_thr(float h, bool ok) {
    return (ok && h >= 0.0f && h <= FLT_MAX) ? fminf(h * h, FLT_MAX) : -INFINITY;
}
__device__ __forceinline__ float ball_inv(float h) { return h > 0.0f ? 1.0f / h : 0.0f; }

// vt[p, :] = values[row(p), :] (perm: tree position -> input row); padding
// positions hold 0, so they add nothing whatever the test says
__global__ void __launch_bounds__(TB)
ball_sum_gather_kernel(const uint32_t *__restrict__ perm, const float *__restrict__ values,
                       uint32_t n, uint32_t n8, int nv, float *__restrict__ vt) {
    const uint64_t e = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (e >= (uint64_t)n8 * (uint32_t)nv) return;
    const uint32_t p = (uint32_t)(e / (uint32_t)nv), c = (uint32_t)(e - (uint64_t)p * (uint32_t)nv);
    const uint32_t row = perm[p];
    float v = 0.0f;
    if (row < n) v = values ? values[(size_t)row * (uint32_t)nv + c] : 1.0f;
    vt[e] = v;
}

// M: the metric's formulas, plain for a packet whose balls all clear the box
// faces (ball.hip ball_fill_kernel)
template <bool PER, bool M, int KERN, int NV>
__device__ __forceinline__ void ball_sum_walk(const DevTree &t, const uint32_t *__restrict__ linfo,
                                              const PadLeaves &pad, const float *__restrict__ vt,
                                              SumLds<NV> &W, const int lane, const float qx,
                                              const float qy, const float qz, const float thr,
                                              const float inv, float (&acc)[NV], uint32_t &cnt) {
    const float L = t.box;
    const cnode_ptr cnodes = (cnode_ptr)t.nodes;
    const cbox_ptr cboxes = (cbox_ptr)t.nbox;
    // the packet walk (packet.hpp), its bound each lane's own thr
    PacketWalk w;
    walk_begin(w);
    uint32_t lpos = 0, lend = 0, visits = 0;
    while (walk_next_leaf<M, false, false>(w, cnodes, cboxes, qx, qy, qz, thr, L, lpos, lend,
                                           visits)) {
        float tb[6];
        leaf_tight_box(linfo, w.node, tb);
        const bool need = box_lb2<M>(qx, qy, qz, tb, L) <= thr;
        if (!__any(need)) continue;
        // top-hat only: a lane whose ball contains the leaf's tight box adds
        // the leaf's values without the d2 test (never a leaf with padding
        // points); for the other kernels every point's d2 is needed anyway
        bool full = false;
        if constexpr (KERN == NBKD_KERNEL_TOPHAT)
            full = need && !leaf_padded(pad, w.node) && box_ub2<PER>(qx, qy, qz, tb) <= thr;
        const bool part = need && !full;
        for (uint32_t c0 = lpos; c0 < lend; c0 += CHUNK) {
            const uint32_t cn = min((uint32_t)CHUNK, lend - c0);
            wave_sync();
            glds_f4(t.p4 + c0, W.p4, lane, cn);
            stage_values<NV>(vt, c0, W.v, lane, cn);
            wait_vm0();
            wave_sync();
            if (full) {
#pragma unroll 1
                for (uint32_t u = 0; u < cn; ++u) {
#pragma unroll
                    for (int c = 0; c < NV; ++c) acc[c] += W.v[u * NV + c];
                }
                cnt += cn;
            }
            if (part) {
#pragma unroll 2
                for (uint32_t u = 0; u < cn; ++u) {
                    const float4 a = W.p4[u];
                    const float d2 = point_d2_fast<M>(qx, qy, qz, a.x, a.y, a.z, L);
                    if (d2 <= thr) {
                        const float k = sph_kernel<KERN>(d2, inv);
#pragma unroll
                        for (int c = 0; c < NV; ++c) acc[c] += W.v[u * NV + c] * k;
                        ++cnt;
                    }
                }
            }
        }
    }
}

template <bool PER, int KERN, int NV>
__global__ void __launch_bounds__(TB, 8)
ball_sum_kernel(DevTree t, const uint32_t *__restrict__ linfo, const float *__restrict__ q,
                const float *__restrict__ h, const uint32_t *__restrict__ order, uint32_t m,
                PadLeaves pad, const float *__restrict__ vt, float *__restrict__ out_sum,
                uint32_t *__restrict__ out_count) {
    __shared__ SumLds<NV> Wl[WPB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    SumLds<NV> &W = Wl[wave];
    const uint32_t gq = (xcd_block(blockIdx.x, gridDim.x) * WPB + wave) * 64u + lane;
    const float L = t.box;
    const PacketQuery p = packet_query<PER>(q, order, gq, m, L);
    const float qx = p.x, qy = p.y, qz = p.z;
    const bool valid = p.valid, inside = p.inside;
    const float hq = valid ? h[p.qo] : -1.0f;
    const float thr = ball_thr(hq, valid && inside);
    const float inv = ball_inv(hq);
    // every lane's own ball clears the box faces (an empty ball clears them
    // too): the plain formulas
    const bool plain = packet_plain<PER>(!(thr < 0.0f), thr, qx, qy, qz, L);
    float acc[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c) acc[c] = 0.0f;
    uint32_t cnt = 0;
    if (plain)
        ball_sum_walk<PER, false, KERN, NV>(t, linfo, pad, vt, W, lane, qx, qy, qz, thr, inv, acc,
                                            cnt);
    else
        ball_sum_walk<PER, PER, KERN, NV>(t, linfo, pad, vt, W, lane, qx, qy, qz, thr, inv, acc,
                                          cnt);
    // a query with an empty ball gets its zero row; a periodic query outside
    // the box is the brute kernel's.  (The id again: not kept live through the
    // walk.)
    if (valid && inside) {
        const uint32_t qo = order[gq];
        if (out_sum) {
#pragma unroll
            for (int c = 0; c < NV; ++c) out_sum[(size_t)qo * NV + c] = acc[c];
        }
        if (out_count) out_count[qo] = cnt;
    }
}

// Periodic queries outside [0, L]^3 (unvalidated input): no box bound is valid
// for the per-axis metric there, so every point is tested, with the
// reference-exact point_d2.  One block per listed query (the list's length is
// in device memory; a fixed grid strides over it): thread i sums the tree
// positions i, i + TB, ... in order, then the partial sums are added in a fixed
// pairwise order, so the result does not depend on scheduling.
template <int KERN>
__device__ __forceinline__ void brute_accumulate(const DevTree &t, const float *__restrict__ vt,
                                                 int nv, float qx, float qy, float qz, float thr,
                                                 float inv, float (&acc)[NBKD_MAX_VALUES],
                                                 uint32_t &cnt) {
    for (uint32_t p = threadIdx.x; p < t.n8; p += TB) {
        const float d2 = point_d2<true>(qx, qy, qz, t.x[p], t.y[p], t.z[p], t.box);
        if (d2 <= thr) {
            const float k = sph_kernel<KERN>(d2, inv);
#pragma unroll
            for (int c = 0; c < NBKD_MAX_VALUES; ++c)
                if (c < nv) acc[c] += vt[(size_t)p * (uint32_t)nv + c] * k;
            ++cnt;
        }
    }
}

__global__ void __launch_bounds__(TB)
ball_sum_brute_kernel(DevTree t, const float *__restrict__ q, const float *__restrict__ h,
                      const uint32_t *__restrict__ list, const uint32_t *__restrict__ nout,
                      const float *__restrict__ vt, int nv, int kernel,
                      float *__restrict__ out_sum, uint32_t *__restrict__ out_count) {
    __shared__ float red[NBKD_MAX_VALUES][TB];
    __shared__ uint32_t redc[TB];
    const uint32_t total = __builtin_amdgcn_readfirstlane(*nout);
    for (uint32_t j = blockIdx.x; j < total; j += gridDim.x) {
        const uint32_t qo = list[j];
        const float qx = q[3 * (size_t)qo], qy = q[3 * (size_t)qo + 1], qz = q[3 * (size_t)qo + 2];
        const float hq = h[qo];
        const float thr = ball_thr(hq, true), inv = ball_inv(hq);
        float acc[NBKD_MAX_VALUES] = {0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t cnt = 0;
        if (kernel == NBKD_KERNEL_TOPHAT)
            brute_accumulate<NBKD_KERNEL_TOPHAT>(t, vt, nv, qx, qy, qz, thr, inv, acc, cnt);
        else if (kernel == NBKD_KERNEL_CUBIC)
            brute_accumulate<NBKD_KERNEL_CUBIC>(t, vt, nv, qx, qy, qz, thr, inv, acc, cnt);
        else
            brute_accumulate<NBKD_KERNEL_WENDLAND>(t, vt, nv, qx, qy, qz, thr, inv, acc, cnt);
#pragma unroll
        for (int c = 0; c < NBKD_MAX_VALUES; ++c) red[c][threadIdx.x] = acc[c];
        redc[threadIdx.x] = cnt;
        __syncthreads();
        for (int o = TB / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) {
#pragma unroll
                for (int c = 0; c < NBKD_MAX_VALUES; ++c)
                    red[c][threadIdx.x] += red[c][threadIdx.x + o];
                redc[threadIdx.x] += redc[threadIdx.x + o];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            if (out_sum)
                for (int c = 0; c < nv; ++c) out_sum[(size_t)qo * (uint32_t)nv + c] = red[c][0];
            if (out_count) out_count[qo] = redc[0];
        }
        __syncthreads(); // red is read before the next query's partial sums land
    }
}

template <int KERN, int NV>
void launch_sum_kn(const Tree &t, const float *q, const float *h, const uint32_t *order,
                   uint32_t m, const PadLeaves &pad, const float *vt, float *out_sum,
                   uint32_t *out_count, hipStream_t s) {
    const unsigned blocks = (unsigned)((m + TB - 1) / TB);
    if (t.periodic)
        ball_sum_kernel<true, KERN, NV><<<blocks, TB, 0, s>>>(view(t), t.leafinfo, q, h, order, m,
                                                              pad, vt, out_sum, out_count);
    else
        ball_sum_kernel<false, KERN, NV><<<blocks, TB, 0, s>>>(view(t), t.leafinfo, q, h, order, m,
                                                               pad, vt, out_sum, out_count);
}

} // namespace

void launch_ball_sum_gather(const Tree &t, const float *values, int nv, float *vt, hipStream_t s) {
    const uint64_t e = t.n8 * (uint64_t)nv;
    if (e == 0) return;
    const uint32_t *perm = t.sidx ? t.sidx : t.idx;
    ball_sum_gather_kernel<<<(unsigned)((e + TB - 1) / TB), TB, 0, s>>>(
        perm, values, (uint32_t)t.n, (uint32_t)t.n8, nv, vt);
}

void launch_ball_sum(const Tree &t, const float *q, const float *h, const uint32_t *order,
                     uint32_t m, const float *vt, int nv, int kernel, float *out_sum,
                     uint32_t *out_count, hipStream_t s) {
    if (m == 0) return;
    const PadLeaves pad = pad_leaves_of(t);
    with_constant<NBKD_KERNEL_TOPHAT, NBKD_KERNEL_CUBIC, NBKD_KERNEL_WENDLAND>(kernel, [&](auto K) {
        with_constant<1, 2, 3, 4>(nv, [&](auto NV) {
            launch_sum_kn<K(), NV()>(t, q, h, order, m, pad, vt, out_sum, out_count, s);
        });
    });
}

void launch_ball_sum_outside_dev(const Tree &t, const float *q, const float *h,
                                 const uint32_t *list, const uint32_t *nout, const float *vt,
                                 int nv, int kernel, float *out_sum, uint32_t *out_count,
                                 hipStream_t s) {
    ball_sum_brute_kernel<<<1024, TB, 0, s>>>(view(t), q, h, list, nout, vt, nv, kernel, out_sum,
                                              out_count);
}

} // namespace nbkd
