// Friends-of-friends groups (NEW, nbkd_fof: the reference has no group
// finder): two of the tree's points are friends when d2 <= b*b in the tree's
// f32 metric (the predicate of nbkd_query_ball_count), groups are the connected
// components, and every point gets the smallest input row of its group.
//
// Four launches over the tree positions p = 0 .. n8-1, with the scratch
// parent[n8], minid[n8] (uint32 each, 8 B per particle):
//   init     parent[p] = p, minid[p] = 0xFFFFFFFF
//   hook     the CSR fill's packet walk (ball.hip ball_fill_walk) with bound
//            b*b, the queries being the tree's own points in tree order: at
//            every leaf a lane needs, each friend j joins the lane's set in a
//            lock-free union-find over the tree positions
//   flatten  parent[p] = root(p); minid[root] = min over the set of the input
//            rows; the number of roots among the real points
//   label    out_label[row(p)] = minid[parent[p]], out_size[label] += 1
//
// Memory model.  On MI355X a CU's L1 is never refreshed by other CUs' stores
// and the per-XCD L2s are not coherent with each other (MI355X_MICROARCH.md,
// "inter-workgroup visibility"), so the hook kernel is written to be correct
// even if every non-atomic load of `parent` is arbitrarily stale.  Three rules:
//   1. a root is only ever changed by atomicCAS(&parent[r], r, smaller);
//   2. any other store to parent[x] (path halving) writes a value that an
//      earlier read returned as an ancestor of x;
//   3. a failed CAS continues from the value it returned, never from a re-read.
// A root is hooked under a smaller position only, and a position that stopped
// being a root never becomes one again (rule 1: the CAS expects r itself, rule
// 2: halving only stores to an x whose parent was read as != x).  Hence every
// value ever seen in parent[x] is a member of x's set and <= x, chains strictly
// descend (no cycle, every find ends), a stale "equal roots" test compares two
// members of the same set and so never reports different sets as joined, and a
// stale "I am a root" view is corrected by the CAS, which acts on the memory
// value.  A unite ends either on equal members (same set) or on a successful
// CAS (the sets are joined at that moment); each retry replaces the larger of
// the two positions by a strictly smaller one, so the loop is bounded by
// construction.  Nothing waits for another wave: no spin, no flag, no fence.
// The find loads are relaxed agent-scope atomic loads: they bypass L1, so the
// chains a wave follows stay short.  The halving stores are plain stores (A/B
// against relaxed agent-scope atomic stores and atomicMin: DESIGN.md §3,
// "Friends-of-friends").  Flatten and label run in later launches and see the
// final values.  Integer atomics only; no inline assembly.
#include <algorithm>
#include <cmath>

#include "internal.hpp"
#include "metric.hpp"
#include "packet.hpp"

namespace nbkd {
namespace {
using namespace dev;

constexpr int TB = 256;
constexpr int WPB = TB / 64;

struct alignas(16) FofLds {
    float4 p4[CHUNK]; // the staged points (Tree::p4; .w is not used here)
};

// halving store variants (HV): 0 plain store (the production choice: 3-6 %
// faster hook kernel past percolation, equal below, profiles/fof.json), 1
// relaxed agent-scope atomic store, 2 atomicMin.  A halving store is only a
// shortcut: one that is delayed, dropped or overtaken changes no result.
constexpr int FOF_HV_DEFAULT = 0;

__device__ __forceinline__ uint32_t par_load(const uint32_t *parent, uint32_t x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x as far as this wave can see (a member of x's set, <= x), with
// path halving: parent[x] = its grandparent, then on from there
template <int HV>
__device__ __forceinline__ uint32_t fof_find(uint32_t *parent, uint32_t x) {
    for (;;) {
        const uint32_t p = par_load(parent, x);
        if (p == x) return x;
        const uint32_t g = par_load(parent, p);
        if (g == p) return p;
        // rule 2: g was read as an ancestor of x (and x is no root: p != x)
        if constexpr (HV == 0)
            parent[x] = g;
        else if constexpr (HV == 1)
            __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else
            atomicMin(parent + x, g);
        x = g;
    }
}

// join the set of rq (a member of the lane's own set) with j's; returns the
// member of the joined set the lane goes on with (the smaller root it saw)
template <int HV>
__device__ __forceinline__ uint32_t fof_unite(uint32_t *parent, uint32_t rq, uint32_t j) {
    uint32_t rj = fof_find<HV>(parent, j);
    // most pairs are already joined: one find and a compare
    if (rj == rq) return rq;
    uint32_t ri = fof_find<HV>(parent, rq);
    while (ri != rj) {
        if (ri < rj) {
            const uint32_t tmp = ri;
            ri = rj;
            rj = tmp;
        }
        // rule 1: succeeds only on a true root, hooked under the smaller position
        const uint32_t old = atomicCAS(parent + ri, ri, rj);
        if (old == ri) break;
        // rule 3: on from the value the CAS returned (an ancestor of ri, < ri)
        ri = fof_find<HV>(parent, old);
    }
    return min(ri, rj);
}

// The hook walk: ball_fill_walk with unions in place of the id stores.  Only
// friends at smaller tree positions (j < gq) are joined: the metric is
// symmetric bit for bit (fl(a - b) = -fl(b - a), then absolute values) and the
// pruning never drops a leaf holding a point within the bound, so the pair
// (i, j) is always met by the walk of its larger end; handling it there alone
// halves the finds and loses no pair.
template <bool PER, bool M, int HV>
__device__ __forceinline__ void fof_hook_walk(const DevTree &t, const uint32_t *__restrict__ linfo,
                                              const PadLeaves &pad, uint32_t *parent, FofLds &W,
                                              const int lane, const uint32_t gq, const float qx,
                                              const float qy, const float qz, const float thr) {
    const float L = t.box;
    const cnode_ptr cnodes = (cnode_ptr)t.nodes;
    const cbox_ptr cboxes = (cbox_ptr)t.nbox;
    uint32_t rq = gq; // a member of the lane's set: the smallest root it has seen
    PacketWalk w;
    walk_begin(w);
    uint32_t lpos = 0, lend = 0, visits = 0;
    while (walk_next_leaf<M, false, false>(w, cnodes, cboxes, qx, qy, qz, thr, L, lpos, lend,
                                           visits)) {
        float tb[6];
        leaf_tight_box(linfo, w.node, tb);
        // a leaf that starts at or after the lane's own position holds no j < gq
        const bool need = lpos < gq && box_lb2<M>(qx, qy, qz, tb, L) <= thr;
        if (!__any(need)) continue;
        const bool padded = leaf_padded(pad, w.node);
        const bool full = need && !padded && box_ub2<PER>(qx, qy, qz, tb) <= thr;
        const bool part = need && !full;
        // whole-leaf lanes need no coordinates: a leaf only they need is not staged
        const bool stage = __any(part);
        for (uint32_t c0 = lpos; c0 < lend; c0 += CHUNK) {
            const uint32_t cn = min((uint32_t)CHUNK, lend - c0);
            // the lane's friends in this chunk are at positions c0 .. c0 + lim - 1 < gq
            const uint32_t lim = gq > c0 ? min(cn, gq - c0) : 0u;
            if (stage) stage_points(t.p4, c0, W.p4, lane, cn);
            if (full) {
#pragma unroll 1
                for (uint32_t u = 0; u < lim; ++u) rq = fof_unite<HV>(parent, rq, c0 + u);
            }
            if (part) {
#pragma unroll 1
                for (uint32_t u = 0; u < lim; ++u) {
                    const float4 a = W.p4[u];
                    if (point_d2_fast<M>(qx, qy, qz, a.x, a.y, a.z, L) <= thr)
                        rq = fof_unite<HV>(parent, rq, c0 + u);
                }
            }
        }
    }
}

template <bool PER, int HV>
__global__ void __launch_bounds__(TB, 8)
fof_hook_kernel(DevTree t, const uint32_t *__restrict__ linfo, const uint32_t *__restrict__ perm,
                uint32_t n, float b2, PadLeaves pad, uint32_t *parent) {
    __shared__ FofLds Wl[WPB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    FofLds &W = Wl[wave];
    // the lane's query is the point at tree position gq
    const uint32_t gq = (xcd_block(blockIdx.x, gridDim.x) * WPB + wave) * 64u + lane;
    // padding points (permutation id >= n) are in no group
    const bool active = gq < t.n8 && perm[gq] < n;
    float qx = 0.0f, qy = 0.0f, qz = 0.0f;
    if (active) {
        const float4 p = t.p4[gq];
        qx = p.x;
        qy = p.y;
        qz = p.z;
    }
    const float L = t.box;
    const float thr = active ? b2 : -INFINITY;
    // every active lane's ball clears the box faces: the plain formulas
    if (packet_plain<PER>(active, b2, qx, qy, qz, L))
        fof_hook_walk<PER, false, HV>(t, linfo, pad, parent, W, lane, gq, qx, qy, qz, thr);
    else
        fof_hook_walk<PER, PER, HV>(t, linfo, pad, parent, W, lane, gq, qx, qy, qz, thr);
}

__global__ void __launch_bounds__(TB)
fof_init_kernel(uint32_t n8, uint32_t *__restrict__ parent, uint32_t *__restrict__ minid) {
    const uint32_t p = blockIdx.x * TB + threadIdx.x;
    if (p >= n8) return;
    parent[p] = p;
    minid[p] = 0xFFFFFFFFu;
}

// parent[p] = the root of p (no hook runs any more: the chains are final; a
// concurrent store here only replaces an ancestor by the root), the smallest
// input row of each set at its root, and the number of roots among real points
__global__ void __launch_bounds__(TB)
fof_flatten_kernel(uint32_t n8, uint32_t n, const uint32_t *__restrict__ perm, uint32_t *parent,
                   uint32_t *minid, unsigned long long *ngroups) {
    const uint32_t p = blockIdx.x * TB + threadIdx.x;
    bool is_root = false;
    if (p < n8) {
        uint32_t r = p;
        for (;;) {
            const uint32_t q = par_load(parent, r);
            if (q == r) break;
            r = q;
        }
        if (r != p) __hip_atomic_store(parent + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t id = perm[p];
        if (id < n) {
            atomicMin(minid + r, id);
            is_root = r == p;
        }
    }
    const uint64_t roots = __ballot(is_root);
    if (ngroups && roots != 0 && (threadIdx.x & 63) == 0)
        atomicAdd(ngroups, (unsigned long long)__popcll(roots));
}

__global__ void __launch_bounds__(TB)
fof_label_kernel(uint32_t n8, uint32_t n, const uint32_t *__restrict__ perm,
                 const uint32_t *__restrict__ parent, const uint32_t *__restrict__ minid,
                 uint32_t *__restrict__ out_label, uint32_t *out_size) {
    const uint32_t p = blockIdx.x * TB + threadIdx.x;
    const uint32_t id = p < n8 ? perm[p] : 0xFFFFFFFFu;
    const bool real = id < n; // padding points are never written
    uint32_t l = 0xFFFFFFFFu;
    if (real) {
        l = minid[parent[p]];
        out_label[id] = l;
    }
    if (!out_size) return;
    // neighbours in tree order mostly share a group: the lanes holding the
    // first real lane's label add their number once, the others one by one
    const uint64_t rm = __ballot(real);
    if (rm == 0) return;
    const int first = __builtin_ctzll(rm);
    const uint32_t l0 = (uint32_t)__builtin_amdgcn_readlane((int)l, first);
    const uint64_t same = __ballot(real && l == l0);
    if ((int)(threadIdx.x & 63) == first)
        atomicAdd(out_size + l0, (uint32_t)__popcll(same));
    else if (real && l != l0)
        atomicAdd(out_size + l, 1u);
}

template <int HV>
void launch_hook(const Tree &t, const uint32_t *perm, float b2, const PadLeaves &pad,
                 uint32_t *parent, hipStream_t s) {
    const unsigned blocks = (unsigned)((t.n8 + TB - 1) / TB);
    if (t.periodic)
        fof_hook_kernel<true, HV><<<blocks, TB, 0, s>>>(view(t), t.leafinfo, perm, (uint32_t)t.n,
                                                        b2, pad, parent);
    else
        fof_hook_kernel<false, HV><<<blocks, TB, 0, s>>>(view(t), t.leafinfo, perm, (uint32_t)t.n,
                                                         b2, pad, parent);
}

} // namespace

nbkd_status fof(const Tree &t, float b, uint32_t *out_label, uint32_t *out_size,
                uint64_t *out_ngroups, uint32_t flags, hipStream_t s) {
    if (out_ngroups) *out_ngroups = 0;
    if (t.n == 0) return NBKD_OK;
    const uint32_t n8 = (uint32_t)t.n8, n = (uint32_t)t.n; // n8 <= UINT32_MAX (build)
    const float b2 = radius_thr(b); // the count's threshold expression
    const bool dev_out = flags & NBKD_OUTPUT_DEVICE;
    Workspace &ws = acquire_ws(t);
    WsCall call(ws, s, std::adopt_lock);
    NBKD_HIP(call.err);
    uint32_t *parent = (uint32_t *)ws.get(WS_KEYS, (size_t)n8 * 4, s);
    uint32_t *minid = (uint32_t *)ws.get(WS_KEYS2, (size_t)n8 * 4, s);
    if (!parent || !minid) return NBKD_ENOMEM;
    unsigned long long *ng = nullptr;
    if (out_ngroups) {
        ng = (unsigned long long *)ws.get(WS_HTOT, 8, s);
        if (!ng) return NBKD_ENOMEM;
        NBKD_HIP(hipMemsetAsync(ng, 0, 8, s));
    }
    uint32_t *lab = out_label, *siz = out_size;
    if (!dev_out) { // host outputs are staged, as the radius count's
        lab = (uint32_t *)ws.get(WS_OUTI, (size_t)n * 4, s);
        if (!lab) return NBKD_ENOMEM;
        if (out_size) {
            siz = (uint32_t *)ws.get(WS_COUNT, (size_t)n * 4, s);
            if (!siz) return NBKD_ENOMEM;
        }
    }
    if (siz) NBKD_HIP(hipMemsetAsync(siz, 0, (size_t)n * 4, s));
    // the build permutation (tree position -> input row): labels are input
    // rows also on a tree whose ids nbkd_set_ids replaced
    const uint32_t *perm = t.sidx ? t.sidx : t.idx;
    const PadLeaves pad = pad_leaves_of(t);
    const unsigned blocks = (unsigned)((t.n8 + TB - 1) / TB);
    fof_init_kernel<<<blocks, TB, 0, s>>>(n8, parent, minid);
    {
        TimedScope ts("fof_hook", s);
#ifdef NBKD_EXPERIMENTS
        // NBKD_FOF_HALVE (experiments build): the halving store, A/B
        const char *e = knob("NBKD_FOF_HALVE");
        const int hv = e ? atoi(e) : FOF_HV_DEFAULT;
        if (hv == 1)
            launch_hook<1>(t, perm, b2, pad, parent, s);
        else if (hv == 2)
            launch_hook<2>(t, perm, b2, pad, parent, s);
        else
#endif
            launch_hook<FOF_HV_DEFAULT>(t, perm, b2, pad, parent, s);
    }
    {
        TimedScope ts("fof_flatten", s);
        fof_flatten_kernel<<<blocks, TB, 0, s>>>(n8, n, perm, parent, minid, ng);
    }
    {
        TimedScope ts("fof_label", s);
        fof_label_kernel<<<blocks, TB, 0, s>>>(n8, n, perm, parent, minid, lab, siz);
    }
    NBKD_HIP(hipGetLastError());
    if (!dev_out) {
        NBKD_HIP(hipMemcpyAsync(out_label, lab, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        if (out_size)
            NBKD_HIP(hipMemcpyAsync(out_size, siz, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    }
    if (out_ngroups) {
        static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "");
        NBKD_HIP(hipMemcpyAsync(out_ngroups, ng, 8, hipMemcpyDeviceToHost, s));
    }
    if (!dev_out || out_ngroups) NBKD_HIP(hipStreamSynchronize(s));
    return NBKD_OK;
}

} // namespace nbkd
