// Barnes-Hut potentials and accelerations (NEW, nbkd_gravity: the reference
// has no force calculation).  G = 1, Plummer softening eps:
//   phi_i = -sum_j m_j / sqrt(d_ij^2 + eps^2),
//   acc_i =  sum_j m_j d_ij / (d_ij^2 + eps^2)^(3/2),   d_ij = p_j - q_i,
// with a far node replaced by its monopole (mass M at the centre of mass c)
// when its tight box is small against its distance: s2 <= theta^2 * |c - q|^2
// (s2 = the squared diagonal of the box).  nbkd.h states every step.
//
// Two parts, both per call:
//   moments  a 32-B record (M, c, s2) per node, read by the walk like the cell
//            boxes (Tree::nbox): wave-uniformly through the scalar cache.  The
//            leaves sum their real points in float64 in tree order; the
//            internal nodes add their children's sums, one level of the tree
//            per launch, bottom-up (a node is combined in the launch after its
//            later child was: the done word holds the launch number, so a word
//            written in the running launch never counts).  No wave waits for
//            another one.
//   walk     64-query packets, one wave each.  Unlike the radius kernels' walk
//            (packet.hpp) there is no bound to prune with and no near / far
//            order: the walk is depth-first and always left-first, and carries
//            the 64-bit mask of the lanes that have not accepted an ancestor.
//            At a node the masked lanes run the opening test; those that accept
//            add the monopole from the uniform record and leave the mask.  An
//            internal node pushes (right child, mask) and enters the left one;
//            a leaf is staged into LDS (points from Tree::p4, masses in tree
//            order beside them) and the masked lanes loop over it.  The terms
//            of a query, and their order, so depend on the tree and the query
//            alone, not on the other 63 lanes: every query is summed by one
//            lane into one f32 register per component, no floating-point
//            atomics, identical bits from every path, batch size and grid.
#include <algorithm>

#include "gravity_dev.hpp"

namespace nbkd {
namespace {
using namespace dev;
using namespace grav;

// the call's scratch (launch_gravity_moments lays it out): per node the
// record, the float64 sums (M64, S64.xyz), the tight box (lo.xyz, hi.xyz, 0, 0)
// and the done word
struct GravScratch {
    GravRec *rec;
    double *sums;
    float *box;
    uint32_t *done;
};

// M = (float)M64, c = (float)(S64 / M64) (the box centre for a massless node),
// s2 from the box edges; f32 steps as nbkd.h states them
__device__ __forceinline__ void grav_finish(const GravScratch &g, uint32_t node, double M64,
                                            double sx, double sy, double sz, const float (&lo)[3],
                                            const float (&hi)[3], uint32_t stamp) {
    double *sm = g.sums + 4 * (size_t)node;
    sm[0] = M64;
    sm[1] = sx;
    sm[2] = sy;
    sm[3] = sz;
    float *bx = g.box + 8 * (size_t)node;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        bx[a] = lo[a];
        bx[3 + a] = hi[a];
    }
    bx[6] = bx[7] = 0.0f;
    GravRec r;
    r.M = (float)M64;
    if (M64 == 0.0) {
        r.cx = 0.5f * (lo[0] + hi[0]);
        r.cy = 0.5f * (lo[1] + hi[1]);
        r.cz = 0.5f * (lo[2] + hi[2]);
    } else {
        r.cx = (float)(sx / M64);
        r.cy = (float)(sy / M64);
        r.cz = (float)(sz / M64);
    }
    const float ex = hi[0] - lo[0], ey = hi[1] - lo[1], ez = hi[2] - lo[2];
    r.s2 = (ex * ex + ey * ey) + ez * ez;
    r.pad0 = r.pad1 = r.pad2 = 0.0f;
    g.rec[node] = r;
    g.done[node] = stamp;
}

// one thread per node; a leaf sums its real points (perm[p] < n) by ascending
// tree position into one accumulator per sum
__global__ void __launch_bounds__(TB)
gravity_leaf_kernel(DevTree t, const uint32_t *__restrict__ perm, uint32_t n,
                    const float *__restrict__ mt, GravScratch g) {
    const uint32_t node = blockIdx.x * TB + threadIdx.x;
    if (node >= t.nnodes) return;
    const nbkd_node nd = t.nodes[node];
    if (nd.dimension >= 0) {
        g.done[node] = 0u;
        return;
    }
    double M64 = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    const uint32_t end = min(nd.right, t.n8);
    for (uint32_t p = nd.left; p < end; ++p) {
        if (perm[p] >= n) continue; // a padding point
        const float4 a = t.p4[p];
        const double mj = (double)mt[p];
        M64 += mj;
        sx += mj * (double)a.x;
        sy += mj * (double)a.y;
        sz += mj * (double)a.z;
        lo[0] = fminf(lo[0], a.x);
        lo[1] = fminf(lo[1], a.y);
        lo[2] = fminf(lo[2], a.z);
        hi[0] = fmaxf(hi[0], a.x);
        hi[1] = fmaxf(hi[1], a.y);
        hi[2] = fmaxf(hi[2], a.z);
    }
    grav_finish(g, node, M64, sx, sy, sz, lo, hi, 1u);
}

// launch `it` (1, 2, ...): an internal node whose children were both done in
// an earlier launch (stamp <= it; this launch writes it + 1) adds their sums,
// left + right, and joins their boxes
__global__ void __launch_bounds__(TB)
gravity_combine_kernel(DevTree t, GravScratch g, uint32_t it) {
    const uint32_t node = blockIdx.x * TB + threadIdx.x;
    if (node >= t.nnodes) return;
    if (g.done[node] != 0u) return;
    const nbkd_node nd = t.nodes[node];
    if (nd.left >= t.nnodes || nd.right >= t.nnodes) return;
    const uint32_t dl = g.done[nd.left], dr = g.done[nd.right];
    if (dl == 0u || dl > it || dr == 0u || dr > it) return;
    const double *a = g.sums + 4 * (size_t)nd.left, *b = g.sums + 4 * (size_t)nd.right;
    const float *ba = g.box + 8 * (size_t)nd.left, *bb = g.box + 8 * (size_t)nd.right;
    float lo[3], hi[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        lo[c] = fminf(ba[c], bb[c]);
        hi[c] = fmaxf(ba[3 + c], bb[3 + c]);
    }
    grav_finish(g, node, a[0] + b[0], a[1] + b[1], a[2] + b[2], a[3] + b[3], lo, hi, it + 1u);
}

__global__ void __launch_bounds__(TB, 8)
gravity_walk_kernel(DevTree t, const GravRec *__restrict__ rec, const float *__restrict__ q,
                    const uint32_t *__restrict__ order, uint32_t m,
                    const float *__restrict__ mt, float th2, float eps2,
                    float *__restrict__ out_phi, float *__restrict__ out_acc) {
    __shared__ GravLds Wl[WPB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    GravLds &W = Wl[wave];
    const uint32_t gq = (xcd_block(blockIdx.x, gridDim.x) * WPB + wave) * 64u + lane;
    const PacketQuery p = packet_query<false>(q, order, gq, m, 0.0f);
    const float qx = p.x, qy = p.y, qz = p.z;
    const bool valid = p.valid;
    const cnode_ptr cnodes = (cnode_ptr)t.nodes;
    const crec_ptr crec = (crec_ptr)rec;
    const bool open_all = !(th2 > 0.0f); // theta = 0: the direct sum
    float phi = 0.0f, ax = 0.0f, ay = 0.0f, az = 0.0f;
    // the wave stack: lane sp holds a pushed right child and the two halves
    // of the mask it was pushed with
    uint32_t sk_node = 0, sk_lo = 0, sk_hi = 0;
    int sp = 0;
    uint32_t node = 0;
    uint64_t mask = __ballot(valid); // the lanes that want the subtree of `node`
    for (;;) {
        if (mask == 0) {
            if (sp == 0) break;
            --sp;
            node = (uint32_t)__builtin_amdgcn_readlane((int)sk_node, sp);
            mask = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)sk_lo, sp) |
                   ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)sk_hi, sp) << 32);
        }
        const GravRec r = crec[node];
        const nbkd_node nd = cnodes[node];
        {
            const bool in = ((mask >> lane) & 1ull) != 0;
            const float dx = r.cx - qx, dy = r.cy - qy, dz = r.cz - qz;
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            const bool ok = in && !open_all && r.s2 <= th2 * d2;
            if (ok) grav_term(r.M, dx, dy, dz, d2, eps2, phi, ax, ay, az);
            mask &= ~__ballot(ok);
        }
        if (mask == 0) continue;
        if (nd.dimension < 0) {
            const bool in = ((mask >> lane) & 1ull) != 0;
            const uint32_t lend = min(nd.right, t.n8);
            for (uint32_t c0 = nd.left; c0 < lend; c0 += CHUNK) {
                const uint32_t cn = min((uint32_t)CHUNK, lend - c0);
                wave_sync();
                glds_f4(t.p4 + c0, W.p4, lane, cn);
                glds_f32(mt + c0, W.m, lane, cn);
                wait_vm0();
                wave_sync();
                if (in) {
                    // (a padding point has mass 0 and d2 = inf: it adds 0)
#pragma unroll 2
                    for (uint32_t u = 0; u < cn; ++u) {
                        const float4 a = W.p4[u];
                        const float mu = W.m[u];
                        const float dx = a.x - qx, dy = a.y - qy, dz = a.z - qz;
                        const float d2 = (dx * dx + dy * dy) + dz * dz;
                        grav_term(mu, dx, dy, dz, d2, eps2, phi, ax, ay, az);
                    }
                }
            }
            mask = 0;
        } else {
            const uint64_t pmask = 1ull << sp;
            sk_node = lane_set(sk_node, nd.right, pmask);
            sk_lo = lane_set(sk_lo, (uint32_t)mask, pmask);
            sk_hi = lane_set(sk_hi, (uint32_t)(mask >> 32), pmask);
            ++sp;
            node = nd.left;
        }
    }
    // (the id again: not kept live through the walk)
    if (valid) {
        const uint32_t qo = order[gq];
        if (out_phi) out_phi[qo] = phi;
        if (out_acc) {
            out_acc[3 * (size_t)qo] = ax;
            out_acc[3 * (size_t)qo + 1] = ay;
            out_acc[3 * (size_t)qo + 2] = az;
        }
    }
}

} // namespace

size_t gravity_scratch_bytes(const Tree &t) { return (size_t)t.nnodes * 100 + 64; }

const void *launch_gravity_moments(const Tree &t, const float *mt, void *scratch, hipStream_t s) {
    const size_t nn = (size_t)t.nnodes;
    char *base = (char *)scratch;
    GravScratch g;
    g.rec = (GravRec *)base;
    g.sums = (double *)(base + nn * 32);
    g.box = (float *)(base + nn * 64);
    g.done = (uint32_t *)(base + nn * 96);
    if (nn == 0) return g.rec;
    const unsigned blocks = (unsigned)((nn + TB - 1) / TB);
    const uint32_t *perm = t.sidx ? t.sidx : t.idx;
    gravity_leaf_kernel<<<blocks, TB, 0, s>>>(view(t), perm, (uint32_t)t.n, mt, g);
    for (int it = 1; it <= t.depth; ++it)
        gravity_combine_kernel<<<blocks, TB, 0, s>>>(view(t), g, (uint32_t)it);
    return g.rec;
}

void launch_gravity_walk(const Tree &t, const void *rec, const float *q, const uint32_t *order,
                         uint32_t m, const float *mt, float th2, float eps2, float *out_phi,
                         float *out_acc, hipStream_t s) {
    if (m == 0) return;
    const unsigned blocks = (unsigned)((m + TB - 1) / TB);
    gravity_walk_kernel<<<blocks, TB, 0, s>>>(view(t), (const GravRec *)rec, q, order, m, mt, th2,
                                              eps2, out_phi, out_acc);
}

} // namespace nbkd
