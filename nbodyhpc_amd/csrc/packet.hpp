// Device helpers shared by the packet kernels (knn_collect.hip, ball.hip,
// ball_hist.hip, ball_hist2.hip, ball_sum.hip, ball_profile.hip, fof.hip, the
// gravity walks): direct-to-LDS loads, wave-local sync and the staging of a
// leaf chunk's points and value rows (stage_points, stage_values), the
// scalar-cache view of the node table, LDS-staged row stores and the fallback
// listing, what a radius kernel does before its walk (packet_query: the lane's
// query and whether it is walked; packet_plain: the packet's vote for the plain
// formulas), the per-leaf idioms (tight box, padding leaves), the head of the
// brute kernels' work items (brute_tile), and the packet walk (walk_begin /
// walk_next_leaf; the kNN collect's hand-scheduled descent; the macro form
// ball_profile.hip keeps).
#pragma once

#include "metric.hpp"

namespace nbkd {
namespace dev {

typedef __attribute__((address_space(1))) const void *gas_ptr;
typedef __attribute__((address_space(3))) void *las_ptr;

// lanes < n copy src[lane] into dst[lane] (LDS) without passing through VGPRs
__device__ __forceinline__ void glds_f32(const float *src, float *dst, int lane, uint32_t n) {
    if ((uint32_t)lane < n)
        __builtin_amdgcn_global_load_lds((gas_ptr)(src + lane), (las_ptr)dst, 4, 0, 0);
}

// lanes < n copy the 16-B src[lane] into dst[lane] (LDS), one instruction for 64 points
__device__ __forceinline__ void glds_f4(const float4 *src, float4 *dst, int lane, uint32_t n) {
    if ((uint32_t)lane < n)
        __builtin_amdgcn_global_load_lds((gas_ptr)(src + lane), (las_ptr)dst, 16, 0, 0);
}

// s_waitcnt vmcnt(0) (expcnt / lgkmcnt untouched): the direct-to-LDS loads have landed
__device__ __forceinline__ void wait_vm0() { __builtin_amdgcn_s_waitcnt(0x0F70); }

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// points staged per step: one chunk per leaf up to leafsize 64 (a leaf of
// 65..128 points takes two)
constexpr int CHUNK = 64;

// the chunk's points p4[c0 .. c0 + cn) into dst (LDS), between two wave syncs:
// the previous chunk's readers are done before the loads, the loads have
// landed before the next read
__device__ __forceinline__ void stage_points(const float4 *p4, uint32_t c0, float4 *dst, int lane,
                                             uint32_t cn) {
    wave_sync();
    glds_f4(p4 + c0, dst, lane, cn);
    wait_vm0();
    wave_sync();
}

// the chunk's NV-channel value rows vt[c0 .. c0 + cn) (tree order) into dst
// (LDS).  Loads only: the caller issues them after its wave sync, beside the
// points', and waits once (wait_vm0) before the second sync.
template <int NV>
__device__ __forceinline__ void stage_values(const float *vt, uint32_t c0, float *dst, int lane,
                                             uint32_t cn) {
    if constexpr (NV == 4) {
        glds_f4(reinterpret_cast<const float4 *>(vt) + c0, reinterpret_cast<float4 *>(dst), lane,
                cn);
    } else {
        // the chunk's cn * NV consecutive floats of vt, 64 per load
        const uint32_t nf = cn * NV;
#pragma unroll
        for (int c = 0; c < NV; ++c)
            glds_f32(vt + (size_t)c0 * NV + c * 64, dst + c * 64, lane,
                     nf > (uint32_t)c * 64u ? nf - (uint32_t)c * 64u : 0u);
    }
}

constexpr int pow2_floor(int v) { return v >= 64 ? 64 : v >= 32 ? 32 : v >= 16 ? 16 : v >= 8 ? 8 : 4; }
constexpr int pow2_ceil(int v) { return v <= 4 ? 4 : v <= 8 ? 8 : v <= 16 ? 16 : v <= 32 ? 32 : 64; }

// node records through the scalar cache: a constant-address-space view of the
// (read-only, wave-uniformly indexed) node table lowers to s_load_dwordx4
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) nbkd_node *cnode_ptr;
#else
typedef const nbkd_node *cnode_ptr;
#endif

// Staged registers j = 0..CC-1 of the 64 lanes (word (j, row) at j*64 + (row ^ j))
// are output columns c = c0 + j of row `row` (query rowq[row]; 0xFFFFFFFF = no
// query); columns outside [0, k) are skipped.  Consecutive lanes store
// consecutive columns of a row: whole rows per store instruction.
// remap != nullptr: the staged words are tree positions, stored as remap[pos]
// (0xFFFFFFFF = no neighbour, stored as is).
template <int CC>
__device__ __forceinline__ void store_rows(const uint32_t *stage, const uint32_t *rowq,
                                           uint32_t *__restrict__ dst, int k, int c0, int lane,
                                           const uint32_t *__restrict__ remap = nullptr) {
    const int jlo = c0 < 0 ? -c0 : 0;           // first staged register in [0, k)
    const int nc = min(CC, k - c0) - jlo;       // staged registers in [0, k)
    if (nc <= 0) return;
    if (nc == CC) {
        // every staged register is an output column (jlo == 0): the row and
        // column of element e = it*64 + lane are shifts of a constant, and the
        // unrolled iterations keep their LDS reads in flight together (the
        // generic loop below divides by a runtime nc and waits on each read)
        constexpr int RPI = 64 / CC; // rows per store instruction
        const int j = lane % CC, r0 = lane / CC;
#pragma unroll 8
        for (int it = 0; it < CC; ++it) {
            const int row = it * RPI + r0;
            const uint32_t qr = rowq[row];
            uint32_t v = stage[j * 64 + (row ^ j)];
            if (qr != 0xFFFFFFFFu) {
                if (remap && v != 0xFFFFFFFFu) v = remap[v];
                // rows are written once: non-temporal stores (with the
                // select's non-temporal column loads, select 14.95 -> 14.83 ms
                // per 1e8 queries, same rows, profiles/r05i_ab.txt)
                __builtin_nontemporal_store(v, &dst[(size_t)qr * k + c0 + j]);
            }
        }
        return;
    }
    for (int e = lane; e < 64 * nc; e += 64) {
        const int row = e / nc, j = jlo + (e - row * nc);
        const uint32_t qr = rowq[row];
        if (qr != 0xFFFFFFFFu) {
            uint32_t v = stage[j * 64 + (row ^ j)];
            if (remap && v != 0xFFFFFFFFu) v = remap[v];
            dst[(size_t)qr * k + c0 + j] = v;
        }
    }
}

// a seeded lane whose k-th slot still holds the sentinel id found fewer than k
// points inside its seed radius: list it for the exact kernel.  Periodic
// queries outside [0, L]^3 are already listed (outside_box_kernel), so each
// query is listed at most once.
template <bool PER>
__device__ __forceinline__ void knn_fail_check(bool valid, bool seeded, uint32_t kth_id, float qx,
                                               float qy, float qz, float L, uint32_t qo,
                                               uint32_t *fail_list, uint32_t *fail_count) {
    const bool listed =
        PER && !(qx >= 0.0f && qx <= L && qy >= 0.0f && qy <= L && qz >= 0.0f && qz <= L);
    if (valid && seeded && !listed && kth_id == 0xFFFFFFFFu)
        fail_list[atomicAdd(fail_count, 1u)] = qo;
}


// the ids of the leaves that hold padding points (Tree::pad_leaves), passed to
// the radius kernels by value
struct PadLeaves {
    uint32_t id[NBKD_PAD_LEAVES];
};
// (a tree with more padded leaves than the list holds passes none)
inline PadLeaves pad_leaves_of(const Tree &t) {
    PadLeaves pad;
    for (int j = 0; j < NBKD_PAD_LEAVES; ++j)
        pad.id[j] = t.npad_leaves <= NBKD_PAD_LEAVES ? t.pad_leaves[j] : 0xFFFFFFFFu;
    return pad;
}
// leaf `node` holds padding points (FLT_MAX, inside no ball): always evaluated
__device__ __forceinline__ bool leaf_padded(const PadLeaves &pad, const uint32_t node) {
    bool padded = false;
#pragma unroll
    for (int j = 0; j < NBKD_PAD_LEAVES; ++j) padded |= pad.id[j] == node;
    return padded;
}

// The lane's ball of squared radius r2 clears the faces of the periodic box
// by a margin r' > r.  When that holds for every lane that walks, the plain
// formulas give the periodic ones' bits for every point within r and fail the
// test for every point beyond (knn_collect.hip collect_packet), so the packet
// walks and tests with them.  packet_plain below adds the guard for the lanes
// that do not walk, and the vote.
__device__ __forceinline__ bool ball_clears_faces(const float r2, const float qx, const float qy,
                                                  const float qz, const float L) {
    const float r1 = sqrtf(fmaxf(r2, 0.0f)) * 1.01f + L * 1e-6f;
    return r1 <= 0.25f * L && qx >= r1 && L - qx >= r1 && qy >= r1 && L - qy >= r1 && qz >= r1 &&
           L - qz >= r1;
}

// One lane's query of a packet: sorted position gq of the m queries is input
// row qo = order[gq] (a lane past the end holds row 0 at the origin).  inside:
// the query lies in [0, L]^3, always true on a non-periodic tree; a periodic
// query outside the box is not walked (its minimum-image pruning is not a
// bound) and is answered by the kernel family's brute kernel.
struct PacketQuery {
    uint32_t qo;
    float x, y, z;
    bool valid, inside;
};
template <bool PER>
__device__ __forceinline__ PacketQuery packet_query(const float *q, const uint32_t *order,
                                                    const uint32_t gq, const uint32_t m,
                                                    const float L) {
    PacketQuery p;
    p.valid = gq < m;
    p.qo = p.valid ? order[gq] : 0u;
    p.x = p.valid ? q[3 * (size_t)p.qo] : 0.0f;
    p.y = p.valid ? q[3 * (size_t)p.qo + 1] : 0.0f;
    p.z = p.valid ? q[3 * (size_t)p.qo + 2] : 0.0f;
    p.inside = !PER || (p.x >= 0.0f && p.x <= L && p.y >= 0.0f && p.y <= L && p.z >= 0.0f &&
                        p.z <= L);
    return p;
}

// The packet's vote: every lane that walks (`walks`; a lane without a query,
// outside the box or with an empty ball does not) has a ball that clears the
// box faces, so the packet walks and tests with the plain formulas.
// Wave-uniform; false on a non-periodic tree, whose formulas are plain already.
template <bool PER>
__device__ __forceinline__ bool packet_plain(const bool walks, const float r2, const float qx,
                                             const float qy, const float qz, const float L) {
    bool plain = false;
    if constexpr (PER) plain = __all(!walks || ball_clears_faces(r2, qx, qy, qz, L));
    return plain;
}

// ------------------------------------------------------------------ brute kernels
// The kernels that answer the periodic queries outside [0, L]^3 stride over
// (listed query, point tile) pairs, a tile BR_ITEMS points per thread of the
// block: work item w is tile w % ntiles of listed query w / ntiles; the thread's
// points are base + u * TB, u < BR_ITEMS.
constexpr int BR_ITEMS = 8;
struct BruteTile {
    uint32_t qo;
    float qx, qy, qz;
    uint32_t base;
};
template <int TB>
__device__ __forceinline__ BruteTile brute_tile(const uint64_t w, const uint32_t ntiles,
                                                const uint32_t *__restrict__ list,
                                                const float *__restrict__ q) {
    const uint32_t j = (uint32_t)(w / ntiles), tile = (uint32_t)(w - (uint64_t)j * ntiles);
    const uint32_t qo = list[j];
    return {qo, q[3 * (size_t)qo], q[3 * (size_t)qo + 1], q[3 * (size_t)qo + 2],
            tile * (uint32_t)(TB * BR_ITEMS) + threadIdx.x};
}

// ------------------------------------------------------------------ packet walk
// v = lanes in `mask` ? val : old, as one v_cndmask (a select of a uniform
// value into one lane otherwise compiles to exec-masked branches)
__device__ __forceinline__ float lane_set(float old, float val, uint64_t mask) {
    float r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(old), "v"(val), "s"(mask));
    return r;
}
__device__ __forceinline__ uint32_t lane_set(uint32_t old, uint32_t val, uint64_t mask) {
    uint32_t r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(old), "v"(val), "s"(mask));
    return r;
}

// The wave stack holds node ids only: a pushed far child's id in lane sp of
// sk_node.  A popped node's box is read back from the tree's per-node cell
// boxes (Tree::nbox: the root box cut by the splits on the node's path, the
// values the walk's box held when the node was pushed), one s_load_dwordx8
// beside the node record.  Round 2 kept the box in six more stack VGPRs (six
// selects per push, six readlanes per pop): collect 50.03 -> 48.80 ms, radius
// count 126.1 -> 121.8 ms at 1e8, same output SHA
// (profiles/r03_ab7_node_stack.txt); the collect kernel needs 58 VGPRs instead
// of 64.
struct NodeBox {
    float b[8];
};
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) NodeBox *cbox_ptr;
#else
typedef const NodeBox *cbox_ptr;
#endif

// the tight box of leaf `node` (leafinfo lo.xyz, hi.xyz: one s_load_dwordx8)
// as lo.x, hi.x, lo.y, hi.y, lo.z, hi.z
__device__ __forceinline__ void leaf_tight_box(const uint32_t *__restrict__ linfo,
                                               const uint32_t node, float (&tb)[6]) {
    const NodeBox lb = ((cbox_ptr)linfo)[node];
    tb[0] = lb.b[0];
    tb[1] = lb.b[3];
    tb[2] = lb.b[1];
    tb[3] = lb.b[4];
    tb[4] = lb.b[2];
    tb[5] = lb.b[5];
}

// The wave's depth-first walk over a packet of 64 queries, one per lane, each
// with its own bound kth (knn_collect.hip, ball.hip's CSR fill, ball_hist.hip,
// ball_sum.hip, fof.hip):
//     PacketWalk w;
//     walk_begin(w);
//     while (walk_next_leaf<M, STATS, NARROW>(w, cnodes, cboxes, qx, qy, qz, kth, L,
//                                             lpos, lend, visits)) {
//         ... leaf w.node holds the points [lpos, lend) ...
//     }
// At an internal node (walk_step, split axis D a compile-time constant) both
// children are tested for every lane; a single wanted child is entered, and
// only when both are wanted the lanes vote which one is near (entered) and
// which far (pushed).  The walk branches on the node's axis, so no per-lane
// selects pick the axis.  Against the form that voted and ran the push's
// selects at every node: collect 51.96 -> 49.4 ms at 1e8 with knn_collect's
// clamped stores (profiles/r03_ab1_collect_variants.txt,
// r03_ab3_lazy_vote.txt), radius count 129.0 -> 126.1 ms (r03_ab2_push_ball.txt).
//
// Tried and dropped (r04s): 64-B node blocks (a node's record and its
// children's) so a descent waits on one scalar load per two levels: collect
// 46.7 -> 50.1 ms, radius count 112.3 -> 124.5 ms at 1e8
// (profiles/r04s_ab_seg_wide.txt).  The node loads mostly hit the scalar
// cache; four times the bytes per record and 12 more live SGPRs (spilled
// kernel arguments) cost more than the shorter chains save.
//
// The form is one the compiler keeps scalar:
//   - the node record's four words, the popped id and the popped box are
//     pinned to SGPRs where they are loaded (readfirstlane of a value that is
//     uniform already costs nothing), and the box is kept as bit patterns:
//     a uniform select of integers is an s_cselect, one of floats a
//     v_cndmask that drags the whole box into VGPRs.  The leaf test and the
//     axis dispatch are s_cmp on SGPRs, the split a scalar VALU operand;
//   - one loop with one exit.  The compiler gives every loop with several
//     exits (a return or break out of a nested step, a found flag) a guard
//     variable and re-dispatches on it after the loop, and carries a
//     "record loaded" flag as a 64-bit lane mask from block to block (the
//     macro walk this replaced did both: collect step 52.83 -> 51.29 ms,
//     profiles/r07a_walk_ab.txt; CSR fill, histogram and sums 2 to 14 %
//     faster, FoF hook 11 to 12 %, profiles/r09a_walk_port_ab.txt).  Here
//     the state is explicit and scalar: the node, whether its record is
//     loaded, and the stack pointer; an iteration pops (when no record is
//     loaded) and then looks at one record, and ends in exactly one of enter
//     child, pop, leaf found, done;
//   - every call starts with a pop: the root is pushed before the first call
//     (walk_begin), and its cell box cboxes[0] is the root box ([0, L]^3
//     periodic, [-FLT_MAX, FLT_MAX]^3 otherwise);
//   - a pop issues the node's record load beside its box load, one wait for
//     both (for a popped node no lane wants any more that is 16 B of scalar
//     cache traffic for nothing; the record is not looked at).
// The axis dispatch stays a scalar three-way branch over three step bodies
// with a compile-time axis.  Tried and dropped: one body whose split-axis
// coordinate, box faces and bound term are picked by scalar-controlled
// selects (10 branches and 42 VALU in the plain walk loop instead of 21 and
// 70): step 52.61 ms against 51.29 with three bodies, same rows
// (profiles/r07a_walk_ab.txt).
//
// Two other walks remain.  ball_count2_kernel's is local to ball.hip: packets
// of 128 queries, two per lane, with two bound sets and a joint vote
// (NBKD_GWALK2).  ball_profile.hip still runs the macro form of this walk
// (NBKD_GWALK, further down, which says why).

struct PacketWalk {
    uint32_t node;    // the node the walk stands on (after a found leaf: its id)
    int sp;           // entries on the wave stack
    uint32_t sk_node; // the wave stack: entry i in lane i
    uint32_t bx[6];   // the cell box of `node`, as float bits (SGPRs)
    float tm[3];      // per lane: the box's per-axis bound terms
};

// the walk stands before the root: one stack entry, node 0 (in lane 0)
__device__ __forceinline__ void walk_begin(PacketWalk &w) {
    w.node = 0;
    w.sp = 1;
    w.sk_node = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) w.bx[a] = 0u;
#pragma unroll
    for (int a = 0; a < 3; ++a) w.tm[a] = 0.0f;
}

// A node's record or cell box through the scalar cache.  NARROW: the byte
// offset is formed in 32 bits (one s_lshl_b32) and given to the load as its
// SGPR offset beside the table's base; otherwise the load takes a 64-bit
// address (a 64-bit shift, an add and an add with carry).  NARROW needs every
// node's box offset, id * 32 B, to fit 32 bits (walk_narrow_ok).
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) char *cbyte_ptr;
#else
typedef const char *cbyte_ptr;
#endif
template <bool NARROW>
__device__ __forceinline__ nbkd_node walk_load_node(const cnode_ptr cnodes, const uint32_t id) {
    if constexpr (NARROW)
        return *reinterpret_cast<cnode_ptr>(reinterpret_cast<cbyte_ptr>(cnodes) +
                                            id * (uint32_t)sizeof(nbkd_node));
    else
        return cnodes[id];
}
template <bool NARROW>
__device__ __forceinline__ NodeBox walk_load_box(const cbox_ptr cboxes, const uint32_t id) {
    if constexpr (NARROW)
        return *reinterpret_cast<cbox_ptr>(reinterpret_cast<cbyte_ptr>(cboxes) +
                                           id * (uint32_t)sizeof(NodeBox));
    else
        return cboxes[id];
}
// the node count below which every 32-bit offset of the NARROW loads is exact
constexpr uint64_t WALK_NARROW_NODES = (1ull << 32) / sizeof(NodeBox);
inline bool walk_narrow_ok(uint64_t nnodes) { return nnodes < WALK_NARROW_NODES; }

// One internal node with split axis D (a constant after inlining): true = the walk entered a child (w.node, its box, bounds and
// wanted mask wm); false = no lane wants either child, the state is dead and
// the next pop rewrites all of it.
template <bool M>
__device__ __forceinline__ bool walk_step(PacketWalk &w, const int D, const uint32_t split_bits,
                                          const uint32_t left, const uint32_t right, uint64_t &wm,
                                          const float qx, const float qy, const float qz,
                                          const float kth, const float L) {
    const float split = __uint_as_float(split_bits);
    const float qd = D == 0 ? qx : (D == 1 ? qy : qz);
    float tl, tr;
    if constexpr (M) {
        const uint32_t lo = D == 0 ? w.bx[0] : (D == 1 ? w.bx[2] : w.bx[4]);
        const uint32_t hi = D == 0 ? w.bx[1] : (D == 1 ? w.bx[3] : w.bx[5]);
        tl = box_lb_axis<M>(qd, __uint_as_float(lo), split, L);
        tr = box_lb_axis<M>(qd, split, __uint_as_float(hi), L);
    } else {
        // plain: the child on q's side keeps the slab's bound tm[D] (the same
        // bits box_lb_axis gives), the other one is (q - split)^2
        const float tmd = D == 0 ? w.tm[0] : (D == 1 ? w.tm[1] : w.tm[2]);
        const float dd = qd - split;
        const float m2 = dd * dd;
        tl = dd > 0.0f ? m2 : tmd;
        tr = dd > 0.0f ? tmd : m2;
    }
    const float dl = ((D == 0 ? tl : w.tm[0]) + (D == 1 ? tl : w.tm[1])) + (D == 2 ? tl : w.tm[2]);
    const float dr = ((D == 0 ? tr : w.tm[0]) + (D == 1 ? tr : w.tm[1])) + (D == 2 ? tr : w.tm[2]);
    const uint64_t wl = __ballot(dl <= kth), wr = __ballot(dr <= kth);
    bool go_right = wr != 0;
    // both wanted: the lanes that want the node vote which child is near
    // (entered) and which far (pushed)
    if (wl != 0 && wr != 0) {
        const uint32_t right_votes = (uint32_t)__popcll(wm & __ballot(qd > split));
        go_right = 2 * right_votes > (uint32_t)__popcll(wm);
        w.sk_node = lane_set(w.sk_node, go_right ? left : right, 1ull << w.sp);
        ++w.sp;
    }
    w.node = go_right ? right : left;
    const float tn = go_right ? tr : tl;
    w.tm[0] = D == 0 ? tn : w.tm[0];
    w.tm[1] = D == 1 ? tn : w.tm[1];
    w.tm[2] = D == 2 ? tn : w.tm[2];
    // the entered child's box: the split replaces the face on the other side
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        w.bx[2 * a] = (D == a && go_right) ? split_bits : w.bx[2 * a];
        w.bx[2 * a + 1] = (D == a && !go_right) ? split_bits : w.bx[2 * a + 1];
    }
    wm = go_right ? wr : wl;
    return (wl | wr) != 0;
}

// advance the walk to the next leaf some lane wants: true = leaf w.node holds
// the points [lpos, lend); false = the walk is over.  visits counts the node
// records looked at (the work counter node_visits).
template <bool M, bool STATS, bool NARROW>
__device__ __forceinline__ bool walk_next_leaf(PacketWalk &w, const cnode_ptr cnodes,
                                               const cbox_ptr cboxes, const float qx,
                                               const float qy, const float qz, const float kth,
                                               const float L, uint32_t &lpos, uint32_t &lend,
                                               uint32_t &visits) {
    enum : int { RUN = 0, LEAF = 1, DONE = 2 };
    bool loaded = false; // the record of w.node is in nd
    int end = RUN;
    int dim = 0;
    uint32_t split_bits = 0, left = 0, right = 0;
    uint64_t wm = 0;
    do {
        if (!loaded) {
            if (w.sp == 0) {
                end = DONE;
            } else {
                --w.sp;
                w.node = (uint32_t)__builtin_amdgcn_readlane((int)w.sk_node, w.sp);
                const NodeBox nb = walk_load_box<NARROW>(cboxes, w.node);
                const nbkd_node nd = walk_load_node<NARROW>(cnodes, w.node);
#pragma unroll
                for (int a = 0; a < 6; ++a) w.bx[a] = uni(__float_as_uint(nb.b[a]));
                dim = (int)uni((uint32_t)nd.dimension);
                split_bits = uni(__float_as_uint(nd.split));
                left = uni(nd.left);
                right = uni(nd.right);
                w.tm[0] = box_lb_axis<M>(qx, __uint_as_float(w.bx[0]), __uint_as_float(w.bx[1]), L);
                w.tm[1] = box_lb_axis<M>(qy, __uint_as_float(w.bx[2]), __uint_as_float(w.bx[3]), L);
                w.tm[2] = box_lb_axis<M>(qz, __uint_as_float(w.bx[4]), __uint_as_float(w.bx[5]), L);
                wm = __ballot((w.tm[0] + w.tm[1]) + w.tm[2] <= kth);
                loaded = wm != 0;
            }
        }
        if (loaded) {
            if constexpr (STATS) ++visits;
            if (dim < 0) {
                lpos = left;
                lend = right;
                end = LEAF;
            } else {
                if (dim == 0)
                    loaded = walk_step<M>(w, 0, split_bits, left, right, wm, qx, qy, qz, kth, L);
                else if (dim == 1)
                    loaded = walk_step<M>(w, 1, split_bits, left, right, wm, qx, qy, qz, kth, L);
                else
                    loaded = walk_step<M>(w, 2, split_bits, left, right, wm, qx, qy, qz, kth, L);
                // the child's record (asked for also when no child was
                // entered: no branch, and the pop that follows overwrites it)
                const nbkd_node nd = walk_load_node<NARROW>(cnodes, w.node);
                dim = (int)uni((uint32_t)nd.dimension);
                split_bits = uni(__float_as_uint(nd.split));
                left = uni(nd.left);
                right = uni(nd.right);
            }
        }
    } while (end == RUN);
    return end == LEAF;
}

// ------------------------------------------------------------------ macro walk (ball_profile.hip only)
// The form walk_next_leaf replaced, kept for ball_profile_walk alone: on the
// function walk its four-channel instance ran 48.88 ms at 1e7 points against
// 48.74 with these macros, whose own spread over five runs is 0.11 ms (the
// other instances were 1.2 to 2 % faster), and the listing (fewer
// instructions of every class, 75 -> 71 VGPRs) does not explain it
// (profiles/r09a_walk_port_ab.txt).  The same
// traversal as walk_step / walk_next_leaf.  The macros expect in scope: lane,
// qx/qy/qz, the bound kth, L, cnodes, the walk state node / nd (its record
// while `have`) / have / wm / bx[6] / tm[3], the wave stack sp / sk_node, the
// cell boxes cboxes, the metric switch M and STATS / st (node visits in st[0]).
#define NBKD_GSTEP(D)                                                                              \
    {                                                                                              \
        const float split = nd.split;                                                              \
        const float qd = (D) == 0 ? qx : ((D) == 1 ? qy : qz);                                     \
        float tl, tr;                                                                              \
        if constexpr (M) {                                                                         \
            tl = box_lb_axis<M>(qd, bx[2 * (D)], split, L);                                        \
            tr = box_lb_axis<M>(qd, split, bx[2 * (D) + 1], L);                                    \
        } else {                                                                                   \
            /* plain: the child on q's side keeps the slab's bound tm[D] (the   */                 \
            /* same bits box_lb_axis gives), the other one is (q - split)^2    */                 \
            const float dd_ = qd - split;                                                          \
            const float m2_ = dd_ * dd_;                                                           \
            tl = dd_ > 0.0f ? m2_ : tm[D];                                                         \
            tr = dd_ > 0.0f ? tm[D] : m2_;                                                         \
        }                                                                                          \
        const float dl = (((D) == 0 ? tl : tm[0]) + ((D) == 1 ? tl : tm[1])) + ((D) == 2 ? tl : tm[2]); \
        const float dr = (((D) == 0 ? tr : tm[0]) + ((D) == 1 ? tr : tm[1])) + ((D) == 2 ? tr : tm[2]); \
        const uint64_t wl = __ballot(dl <= kth), wr = __ballot(dr <= kth);                         \
        bool go_right = wr != 0;                                                                   \
        if (wl != 0 && wr != 0) {                                                                  \
            const uint32_t right_votes = (uint32_t)__popcll(wm & __ballot(qd > split));            \
            const bool right_first = 2 * right_votes > (uint32_t)__popcll(wm);                     \
            const uint64_t pmask = 1ull << sp;                                                     \
            sk_node = lane_set(sk_node, right_first ? nd.left : nd.right, pmask);                  \
            ++sp;                                                                                  \
            go_right = right_first;                                                                \
        } else if (wl == 0 && wr == 0) {                                                           \
            continue;                                                                              \
        }                                                                                          \
        node = go_right ? nd.right : nd.left;                                                      \
        nd = cnodes[node];                                                                         \
        tm[D] = go_right ? tr : tl;                                                                \
        if (go_right)                                                                              \
            bx[2 * (D)] = unif(split);                                                             \
        else                                                                                       \
            bx[2 * (D) + 1] = unif(split);                                                         \
        wm = go_right ? wr : wl;                                                                   \
        have = true;                                                                               \
    }

// advance the packet walk to the next leaf some lane wants (FOUND = false: done)
#define NBKD_GWALK(FOUND, LPOS, LEND)                                                              \
    FOUND = false;                                                                                 \
    for (;;) {                                                                                     \
        if (!have) {                                                                               \
            if (sp == 0) break;                                                                    \
            --sp;                                                                                  \
            node = (uint32_t)__builtin_amdgcn_readlane((int)sk_node, sp);                          \
            {                                                                                      \
                const NodeBox nb_ = cboxes[node];                                                  \
                _Pragma("unroll") for (int a = 0; a < 6; ++a) bx[a] = nb_.b[a];                    \
            }                                                                                      \
            tm[0] = box_lb_axis<M>(qx, bx[0], bx[1], L);                                           \
            tm[1] = box_lb_axis<M>(qy, bx[2], bx[3], L);                                           \
            tm[2] = box_lb_axis<M>(qz, bx[4], bx[5], L);                                           \
            wm = __ballot((tm[0] + tm[1]) + tm[2] <= kth);                                         \
            if (wm == 0) continue;                                                                 \
            nd = cnodes[node];                                                                     \
        }                                                                                          \
        have = false;                                                                              \
        if constexpr (STATS) ++st[0];                                                              \
        if (nd.dimension < 0) {                                                                    \
            LPOS = nd.left;                                                                        \
            LEND = nd.right;                                                                       \
            FOUND = true;                                                                          \
            break;                                                                                 \
        }                                                                                          \
        if (nd.dimension == 0)                                                                     \
            NBKD_GSTEP(0)                                                                          \
        else if (nd.dimension == 1)                                                                \
            NBKD_GSTEP(1)                                                                          \
        else                                                                                       \
            NBKD_GSTEP(2)                                                                          \
    }

// ------------------------------------------------------------------ hand-scheduled descent
// The descent of the plain-metric walk with 32-bit offsets (96 % of the
// bench's packets), from a wanted node whose record is loaded down to a leaf
// or to a node neither of whose children any lane wants: the arithmetic of
// walk_step<false> instruction for instruction (same operands, same
// association, so the same bits and the same leaf sequence), with the control
// flow the compiler does not produce from any C++ form tried
// (profiles/r08a_walk_static.txt).  The state is where the code stands: the
// wanted tests are s_cmp_lg_u64 on the two compare masks and branches on SCC,
// each outcome (left only, right only, both wanted and the vote's two sides)
// has its own few moves, and nothing is copied on the back edge.  A visit
// that enters the only wanted child is 8 SALU, 5 to 7 branches, one s_load and
// 12 VALU (the compiled loop: 28, 7, 1, 16).
//
// The record lives in s[68:71] (dimension, split, left, right): an
// s_load_dwordx4 needs an aligned register quadruple, which an inline-assembly
// operand cannot name the words of, so the block owns these four registers.
// They lie inside the 74 SGPRs (80 with VCC and its kin) that the compiler
// itself keeps a kernel of 8 waves per SIMD under, so the register allocator
// works around them and the kernel's count cannot pass that bound on their
// account: it is 78 for the first-pass instance (scripts/asm_counts.py
// --max-sgprs 80 checks a listing).  Higher numbers do pass it, and cost a
// wave: owning s[88:91] the kernel counted 98 SGPRs and was 1.9 ms slower
// than the parent; owning s[76:79] (86, registers the compiler holds back and
// warns about) 0.4 to 1.0 ms faster, at 7 waves per SIMD by the counters where
// the compiler reported 8; owning these, 2.2 ms faster (step 50.01 -> 47.78 ms,
// profiles/r08a_collect_ab.txt, r08a_pmc_sq.txt).  The
// block reads the node table through the
// scalar cache only and writes registers only.  Wait states gfx950 wants by hand: two between a VALU write
// of VCC and the v_cndmask that reads it.
//
// in:  dim / split / left / right = the record of w.node, wm = the lanes that
//      want it (nonzero)
// out: dim < 0: the walk stands on leaf w.node, left / right = its point range;
//      dim == 0: no lane wants either child of the last node, the state is dead
// the per-axis bound arithmetic; tl in %[c], tr in %[b], then the two ballots
#define NBKD_WD_AXIS(Q, TM, A, B)                                                                  \
    "v_subrev_f32_e32 %[a], s69, " Q "\n"                                                          \
    "v_cmp_lt_f32_e32 vcc, 0, %[a]\n"                                                              \
    "v_mul_f32_e32 %[b], %[a], %[a]\n"                                                             \
    "s_nop 0\n"                                                                                    \
    "v_cndmask_b32_e32 %[c], " TM ", %[b], vcc\n"                                                  \
    "v_cndmask_b32_e32 %[b], %[b], " TM ", vcc\n"                                                  \
    "v_add_f32_e32 %[a], %[c], " A "\n"                                                            \
    "v_add_f32_e32 %[d], %[b], " A "\n"                                                            \
    "v_add_f32_e32 %[a], %[a], " B "\n"                                                            \
    "v_add_f32_e32 %[d], %[d], " B "\n"                                                            \
    "v_cmp_le_f32_e64 %[wl], %[a], %[kth]\n"                                                       \
    "v_cmp_le_f32_e64 %[wr], %[d], %[kth]\n"
// axis 2: (tm0 + tm1) + t; the sum of the other two terms fills the wait states
#define NBKD_WD_AXIS2(Q, TM, A, B)                                                                 \
    "v_subrev_f32_e32 %[a], s69, " Q "\n"                                                          \
    "v_cmp_lt_f32_e32 vcc, 0, %[a]\n"                                                              \
    "v_mul_f32_e32 %[b], %[a], %[a]\n"                                                             \
    "v_add_f32_e32 %[d], " A ", " B "\n"                                                           \
    "v_cndmask_b32_e32 %[c], " TM ", %[b], vcc\n"                                                  \
    "v_cndmask_b32_e32 %[b], %[b], " TM ", vcc\n"                                                  \
    "v_add_f32_e32 %[a], %[d], %[c]\n"                                                             \
    "v_add_f32_e32 %[d], %[d], %[b]\n"                                                             \
    "v_cmp_le_f32_e64 %[wl], %[a], %[kth]\n"                                                       \
    "v_cmp_le_f32_e64 %[wr], %[d], %[kth]\n"
// which children are wanted; both: the vote, the push of the far child into
// lane sp of the stack; then the entered child's bound term, mask and id
#define NBKD_WD_DECIDE(T, Q, TM)                                                                   \
    "s_cmp_lg_u64 %[wr], 0\n"                                                                      \
    "s_cbranch_scc0 .Lwd_" T "nr_%=\n"                                                             \
    "s_cmp_lg_u64 %[wl], 0\n"                                                                      \
    "s_cbranch_scc0 .Lwd_" T "R_%=\n"                                                              \
    "v_cmp_lt_f32_e32 vcc, s69, " Q "\n"                                                           \
    "s_and_b64 vcc, vcc, %[wm]\n"                                                                  \
    "s_bcnt1_i32_b64 %[s0], vcc\n"                                                                 \
    "s_bcnt1_i32_b64 %[s1], %[wm]\n"                                                               \
    "s_lshl_b32 %[s0], %[s0], 1\n"                                                                 \
    "s_lshl_b64 %[pm], 1, %[sp]\n"                                                                 \
    "s_add_i32 %[sp], %[sp], 1\n"                                                                  \
    "s_cmp_gt_u32 %[s0], %[s1]\n"                                                                  \
    "s_cbranch_scc1 .Lwd_" T "pR_%=\n"                                                             \
    "v_mov_b32_e32 %[a], s71\n"                                                                    \
    "v_cndmask_b32_e64 %[sk], %[sk], %[a], %[pm]\n"                                                \
    ".Lwd_" T "L_%=:\n"                                                                            \
    "v_mov_b32_e32 " TM ", %[c]\n"                                                                 \
    "s_mov_b64 %[wm], %[wl]\n"                                                                     \
    "s_mov_b32 %[nd], s70\n"                                                                       \
    "s_branch .Lwd_load_%=\n"                                                                      \
    ".Lwd_" T "nr_%=:\n"                                                                           \
    "s_cmp_lg_u64 %[wl], 0\n"                                                                      \
    "s_cbranch_scc1 .Lwd_" T "L_%=\n"                                                              \
    "s_branch .Lwd_none_%=\n"                                                                      \
    ".Lwd_" T "pR_%=:\n"                                                                           \
    "v_mov_b32_e32 %[a], s70\n"                                                                    \
    "v_cndmask_b32_e64 %[sk], %[sk], %[a], %[pm]\n"                                                \
    ".Lwd_" T "R_%=:\n"                                                                            \
    "v_mov_b32_e32 " TM ", %[b]\n"                                                                 \
    "s_mov_b64 %[wm], %[wr]\n"                                                                     \
    "s_mov_b32 %[nd], s71\n"
#define NBKD_WD_BODY(VISIT)                                                                        \
    "s_mov_b32 s68, %[dim]\n"                                                                      \
    "s_mov_b32 s69, %[spl]\n"                                                                      \
    "s_mov_b32 s70, %[lf]\n"                                                                       \
    "s_mov_b32 s71, %[rt]\n"                                                                       \
    ".Lwd_top_%=:\n" VISIT                                                                         \
    "s_cmp_lt_i32 s68, 0\n"                                                                        \
    "s_cbranch_scc1 .Lwd_leaf_%=\n"                                                                \
    "s_cmp_eq_u32 s68, 1\n"                                                                        \
    "s_cbranch_scc1 .Lwd_y_%=\n"                                                                   \
    "s_cmp_eq_u32 s68, 0\n"                                                                        \
    "s_cbranch_scc1 .Lwd_x_%=\n"                                                                   \
    NBKD_WD_AXIS2("%[qz]", "%[tm2]", "%[tm0]", "%[tm1]")                                           \
    NBKD_WD_DECIDE("z", "%[qz]", "%[tm2]")                                                         \
    "s_branch .Lwd_load_%=\n"                                                                      \
    ".Lwd_y_%=:\n"                                                                                 \
    NBKD_WD_AXIS("%[qy]", "%[tm1]", "%[tm0]", "%[tm2]")                                            \
    NBKD_WD_DECIDE("y", "%[qy]", "%[tm1]")                                                         \
    "s_branch .Lwd_load_%=\n"                                                                      \
    ".Lwd_x_%=:\n"                                                                                 \
    NBKD_WD_AXIS("%[qx]", "%[tm0]", "%[tm1]", "%[tm2]")                                            \
    NBKD_WD_DECIDE("x", "%[qx]", "%[tm0]")                                                         \
    ".Lwd_load_%=:\n"                                                                              \
    "s_lshl_b32 %[s0], %[nd], 4\n"                                                                 \
    "s_load_dwordx4 s[68:71], %[base], %[s0] offset:0x0\n"                                         \
    "s_waitcnt lgkmcnt(0)\n"                                                                       \
    "s_branch .Lwd_top_%=\n"                                                                       \
    ".Lwd_none_%=:\n"                                                                              \
    "s_mov_b32 %[dim], 0\n"                                                                        \
    "s_branch .Lwd_end_%=\n"                                                                       \
    ".Lwd_leaf_%=:\n"                                                                              \
    "s_mov_b32 %[dim], s68\n"                                                                      \
    "s_mov_b32 %[lf], s70\n"                                                                       \
    "s_mov_b32 %[rt], s71\n"                                                                       \
    ".Lwd_end_%=:\n"
#define NBKD_WD_OPERANDS                                                                           \
    [dim] "+s"(dim), [lf] "+s"(left), [rt] "+s"(right), [nd] "+s"(w.node), [sp] "+s"(w.sp),        \
        [wm] "+s"(wm), [tm0] "+v"(w.tm[0]), [tm1] "+v"(w.tm[1]), [tm2] "+v"(w.tm[2]),              \
        [sk] "+v"(w.sk_node), [a] "=&v"(ta), [b] "=&v"(tb), [c] "=&v"(tc), [d] "=&v"(td),          \
        [wl] "=&s"(wl), [wr] "=&s"(wr), [pm] "=&s"(pm), [s0] "=&s"(s0), [s1] "=&s"(s1)
template <bool STATS>
__device__ __forceinline__ void walk_descend(PacketWalk &w, const cnode_ptr cnodes, uint32_t &dim,
                                             const uint32_t split_bits, uint32_t &left,
                                             uint32_t &right, uint64_t wm, const float qx,
                                             const float qy, const float qz, const float kth,
                                             uint32_t &visits) {
    float ta, tb, tc, td;
    uint64_t wl, wr, pm;
    uint32_t s0, s1;
    const uint64_t base = (uint64_t)cnodes;
    if constexpr (STATS)
        asm volatile(NBKD_WD_BODY("s_add_u32 %[vis], %[vis], 1\n")
                     : NBKD_WD_OPERANDS, [vis] "+s"(visits)
                     : [spl] "s"(split_bits), [base] "s"(base), [qx] "v"(qx), [qy] "v"(qy),
                       [qz] "v"(qz), [kth] "v"(kth)
                     : "s68", "s69", "s70", "s71", "vcc", "scc");
    else
        asm volatile(NBKD_WD_BODY("")
                     : NBKD_WD_OPERANDS
                     : [spl] "s"(split_bits), [base] "s"(base), [qx] "v"(qx), [qy] "v"(qy),
                       [qz] "v"(qz), [kth] "v"(kth)
                     : "s68", "s69", "s70", "s71", "vcc", "scc");
}
#undef NBKD_WD_OPERANDS
#undef NBKD_WD_BODY
#undef NBKD_WD_DECIDE
#undef NBKD_WD_AXIS2
#undef NBKD_WD_AXIS

// walk_next_leaf<false, STATS, true> around the hand-scheduled descent: the
// pop in C++ (every call starts with one), the descent from the popped node
// in walk_descend; one loop with one exit block
template <bool STATS>
__device__ __forceinline__ bool walk_next_leaf_plain(PacketWalk &w, const cnode_ptr cnodes,
                                                     const cbox_ptr cboxes, const float qx,
                                                     const float qy, const float qz,
                                                     const float kth, const float L,
                                                     uint32_t &lpos, uint32_t &lend,
                                                     uint32_t &visits) {
    uint32_t found = 0, dim = 0, left = 0, right = 0;
    while (w.sp != 0) {
        --w.sp;
        w.node = (uint32_t)__builtin_amdgcn_readlane((int)w.sk_node, w.sp);
        const NodeBox nb = walk_load_box<true>(cboxes, w.node);
        const nbkd_node nd = walk_load_node<true>(cnodes, w.node);
#pragma unroll
        for (int a = 0; a < 6; ++a) w.bx[a] = uni(__float_as_uint(nb.b[a]));
        // the record is pinned here, before the wanted test, so that its load
        // is issued beside the box load and one wait covers both
        dim = uni((uint32_t)nd.dimension);
        const uint32_t split_bits = uni(__float_as_uint(nd.split));
        left = uni(nd.left);
        right = uni(nd.right);
        w.tm[0] = box_lb_axis<false>(qx, __uint_as_float(w.bx[0]), __uint_as_float(w.bx[1]), L);
        w.tm[1] = box_lb_axis<false>(qy, __uint_as_float(w.bx[2]), __uint_as_float(w.bx[3]), L);
        w.tm[2] = box_lb_axis<false>(qz, __uint_as_float(w.bx[4]), __uint_as_float(w.bx[5]), L);
        const uint64_t wm = __ballot((w.tm[0] + w.tm[1]) + w.tm[2] <= kth);
        if (wm == 0) continue;
        walk_descend<STATS>(w, cnodes, dim, split_bits, left, right, wm, qx, qy, qz, kth, visits);
        if ((int)dim < 0) {
            asm volatile(""); // keeps this a branch: as a select it costs two lane masks per pop
            found = 1;
            break;
        }
    }
    lpos = left;
    lend = right;
    return found != 0;
}

} // namespace dev
} // namespace nbkd
