// Group catalogue (NEW, nbkd_group_catalog: the reference has no group finder):
// from a canonical labelling of the tree's points (label[i] = the smallest input
// row of i's group, the output of nbkd_fof) the kept groups' heads, sizes,
// member lists (CSR, rows ascending) and float64 moments about the head.
//
// Pipeline, all on the device (n rows, G kept groups, K rows in them):
//   hist      validate the labels, cnt[label[i]] += 1 (integer atomics)
//   flag      rowflag[i] = cnt[label[i]] >= min_members, headflag[i] = rowflag[i]
//             and label[i] == i; G and K (read by the host: the only wait
//             before the outputs are complete)
//   scan x 2  pos[i] = kept rows before i, gidx[i] = kept heads before i
//   compact   keys[pos[i]] = gidx[label[i]], members[pos[i]] = i: ascending
//             rows; head[g], size[g]
//   sort      radix_sort (stable LSD radix) on the low ceil(log2 G) key bits:
//             groups ascending by head, rows ascending inside each: out_members
//   offsets   off[g] = the first sorted position with key g
//   inv       row -> tree position (one scatter of the build permutation)
//   moments   each wave takes 64 consecutive sorted members, forms the float64
//             terms and reduces them per group with a log-step segmented scan
//             over the lanes; a group inside one wave is stored directly, the
//             others leave one partial per wave they touch
//   combine   one block per group that crosses a wave boundary (each wave
//             notes the group that leaves it, no list is appended) sums its
//             partials: thread t takes partials t, t + 256, ... in order, then
//             a fixed butterfly over the lanes and the four waves in order
//
// Determinism.  No floating-point atomics.  The terms are functions of the
// inputs alone; which lane of which wave holds a member is its position in the
// sorted member list, and the shapes of the segmented scan and of the combine
// depend on those positions only.  The list itself (groups by ascending head,
// rows ascending) does not depend on the tree, so neither do the sums: trees of
// the same points with different leaf sizes give moments equal under ==.  dmax
// is a maximum (order-independent, exact) and travels with the sums.  The only
// atomics are the integer ones of the size histogram and of the counters.
#include <algorithm>
#include <string>

#include "internal.hpp"

namespace nbkd {
namespace {

constexpr int TB = 256;
constexpr int WPB = TB / 64;
constexpr uint32_t COMBINE_BLOCKS = 4096; // grid of the combine: strides over the list

// counters (uint64 words of WS_HTOT)
enum { C_BAD = 0, C_GROUPS, C_ROWS, C_N };

// cnt[label[i]] += 1 through a per-block hash table in LDS: a block's rows that
// share a label (past percolation most rows of the input share one) cost one
// global atomic per block, not one per row on a single address.  Open
// addressing over twice as many slots as the block has rows, so a probe always
// ends.  Rows whose label is not canonical are counted and left out.
constexpr int HIST_ITEMS = 4;
constexpr int HIST_TILE = TB * HIST_ITEMS;
constexpr uint32_t HIST_SLOTS = 2 * HIST_TILE; // a power of two
constexpr uint32_t HIST_EMPTY = 0xFFFFFFFFu;   // (no label: l < n <= 0xFFFFFFFF)

__global__ void __launch_bounds__(TB)
group_hist_kernel(const uint32_t *__restrict__ label, uint32_t n, uint32_t *cnt,
                  unsigned long long *ctr) {
    __shared__ uint32_t key[HIST_SLOTS], val[HIST_SLOTS];
    __shared__ uint32_t nbad;
    for (uint32_t q = threadIdx.x; q < HIST_SLOTS; q += TB) {
        key[q] = HIST_EMPTY;
        val[q] = 0u;
    }
    if (threadIdx.x == 0) nbad = 0u;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * HIST_TILE;
#pragma unroll
    for (int j = 0; j < HIST_ITEMS; ++j) {
        const uint64_t i = base + (uint32_t)(j * TB) + threadIdx.x;
        if (i >= n) continue;
        const uint32_t l = label[i];
        if (l >= n || label[l] != l) { // (l >= n is tested first: no read past the array)
            atomicAdd(&nbad, 1u);
            continue;
        }
        uint32_t h = (l * 2654435761u) >> 21; // 11 bits: HIST_SLOTS
        static_assert(HIST_SLOTS == 1u << 11, "the hash keeps log2(HIST_SLOTS) bits");
        for (;;) {
            const uint32_t prev = atomicCAS(&key[h], HIST_EMPTY, l);
            if (prev == HIST_EMPTY || prev == l) break;
            h = (h + 1u) & (HIST_SLOTS - 1u);
        }
        atomicAdd(&val[h], 1u);
    }
    __syncthreads();
    for (uint32_t q = threadIdx.x; q < HIST_SLOTS; q += TB)
        if (key[q] != HIST_EMPTY) atomicAdd(cnt + key[q], val[q]);
    if (threadIdx.x == 0 && nbad != 0u) atomicAdd(ctr + C_BAD, (unsigned long long)nbad);
}

// the kept rows and heads, flagged for the two scans and counted: a fixed grid
// strides over the rows, one pair of global atomics per block
constexpr uint32_t FLAG_BLOCKS = 1024;

__global__ void __launch_bounds__(TB)
group_flag_kernel(const uint32_t *__restrict__ label, uint32_t n, const uint32_t *__restrict__ cnt,
                  uint32_t mm, uint32_t *__restrict__ rowflag, uint32_t *__restrict__ headflag,
                  unsigned long long *ctr) {
    __shared__ uint32_t tot[2];
    if (threadIdx.x == 0) tot[0] = tot[1] = 0u;
    __syncthreads();
    uint32_t nh = 0, nr = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * TB) {
        const uint32_t l = label[i];
        // (an invalid labelling is reported by the host after this launch)
        const bool row = l < n && cnt[l] >= mm;
        const bool head = row && l == (uint32_t)i;
        rowflag[i] = row ? 1u : 0u;
        headflag[i] = head ? 1u : 0u;
        nr += row ? 1u : 0u;
        nh += head ? 1u : 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nh += __shfl_xor(nh, o, 64);
        nr += __shfl_xor(nr, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&tot[0], nh);
        atomicAdd(&tot[1], nr);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (tot[0]) atomicAdd(ctr + C_GROUPS, (unsigned long long)tot[0]);
        if (tot[1]) atomicAdd(ctr + C_ROWS, (unsigned long long)tot[1]);
    }
}

__global__ void __launch_bounds__(TB)
group_compact_kernel(const uint32_t *__restrict__ label, uint32_t n,
                     const uint32_t *__restrict__ cnt, uint32_t mm,
                     const uint32_t *__restrict__ pos, const uint32_t *__restrict__ gidx,
                     uint32_t *__restrict__ keys, uint32_t *__restrict__ vals,
                     uint32_t *__restrict__ head, uint32_t *__restrict__ size) {
    const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const uint32_t l = label[i];
    const uint32_t c = cnt[l];
    if (c < mm) return;
    const uint32_t g = gidx[l], p = pos[i];
    keys[p] = g;
    vals[p] = (uint32_t)i;
    if (l == (uint32_t)i) {
        head[g] = l;
        size[g] = c;
    }
}

// off[g] = the first sorted position of group g (every kept group has a member)
__global__ void __launch_bounds__(TB)
group_offsets_kernel(const uint32_t *__restrict__ keys, uint32_t K, uint32_t G,
                     uint32_t *__restrict__ off, uint64_t *__restrict__ off64) {
    const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= K) return;
    const uint32_t g = keys[i];
    if (i == 0 || keys[i - 1] != g) {
        off[g] = (uint32_t)i;
        if (off64) off64[g] = i;
    }
    if (i == (uint64_t)K - 1) {
        off[G] = K;
        if (off64) off64[G] = K;
    }
}

// inv[row] = the tree position of input row `row` (padding points: no row)
__global__ void __launch_bounds__(TB)
group_inv_kernel(const uint32_t *__restrict__ perm, uint32_t n8, uint32_t n,
                 uint32_t *__restrict__ inv) {
    const uint64_t p = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (p >= n8) return;
    const uint32_t r = perm[p];
    if (r < n) inv[r] = (uint32_t)p;
}

// the image of d nearest to 0 among d, fl(d - L), fl(d + L): ties to the earlier
__device__ __forceinline__ float nearest_image(float d, float L) {
    const float dm = d - L, dp = d + L;
    float r = d;
    if (fabsf(dm) < fabsf(r)) r = dm;
    if (fabsf(dp) < fabsf(r)) r = dp;
    return r;
}

struct MomentArgs {
    const float4 *__restrict__ p4;
    const uint32_t *__restrict__ inv;
    const uint32_t *__restrict__ keys;    // sorted: the group of each member
    const uint32_t *__restrict__ members; // sorted: the member rows
    const uint32_t *__restrict__ head;
    const uint32_t *__restrict__ off;
    const float *__restrict__ weight; // or nullptr: 1
    const float *__restrict__ values; // (n, NV) or nullptr
    uint32_t K;
    float L;
    double *__restrict__ moments; // (G, NT)
    float *__restrict__ dmax;     // (G,)
    double *__restrict__ partial; // (2 waves, NT): slot 2w = the group entering
                                  // wave w from the left, 2w + 1 = the one leaving it
    float *__restrict__ pdmax;    // (2 waves,): the same slots' |d|max
    uint32_t *__restrict__ cross; // (waves,): the group that starts in wave w and
                                  // goes on past it, or CROSS_NONE
    uint32_t nwaves;
};
constexpr uint32_t CROSS_NONE = 0xFFFFFFFFu;

// The segmented moment kernel.  Lane = one sorted member; the NT = 5 + 2 NV
// float64 terms and |d|max are scanned over the lanes in log2(64) steps, a
// lane adding its o-th left neighbour's value only when that lane holds the
// same group (the keys are sorted, so equal keys are one contiguous segment).
// The last lane of a segment then holds the segment's sum within this wave.
template <int NV, bool PER>
__global__ void __launch_bounds__(TB) group_moments_kernel(MomentArgs a) {
    constexpr int NT = NBKD_GROUP_MOMENTS(NV);
    const int lane = threadIdx.x & 63;
    const uint32_t w = blockIdx.x * WPB + (threadIdx.x >> 6);
    const uint64_t i = (uint64_t)w * 64u + (uint32_t)lane;
    const bool active = i < a.K;
    uint32_t g = 0xFFFFFFFFu; // (no group: g < G <= 0xFFFFFFFF)
    double t[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) t[k] = 0.0;
    float dm = 0.0f;
    if (active) {
        const uint32_t row = a.members[i];
        g = a.keys[i];
        const float4 p = a.p4[a.inv[row]];
        const float4 h = a.p4[a.inv[a.head[g]]];
        float dx = p.x - h.x, dy = p.y - h.y, dz = p.z - h.z;
        if constexpr (PER) {
            dx = nearest_image(dx, a.L);
            dy = nearest_image(dy, a.L);
            dz = nearest_image(dz, a.L);
        }
        dm = fmaxf(fmaxf(fabsf(dx), fabsf(dy)), fabsf(dz));
        const double wt = a.weight ? (double)a.weight[row] : 1.0;
        const double x = (double)dx, y = (double)dy, z = (double)dz;
        t[0] = wt;
        t[1] = wt * x;
        t[2] = wt * y;
        t[3] = wt * z;
        t[4] = wt * ((x * x + y * y) + z * z);
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            const double v = (double)a.values[(size_t)row * NV + c];
            t[5 + c] = wt * v;
            t[5 + NV + c] = wt * (v * v);
        }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t gl = __shfl_up(g, o, 64);
        const bool same = lane >= o && gl == g;
        const float dl = __shfl_up(dm, o, 64);
        if (same) dm = fmaxf(dm, dl);
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            const double y = __shfl_up(t[k], o, 64);
            if (same) t[k] += y;
        }
    }
    const uint32_t gr = __shfl_down(g, 1, 64);
    if (!active || (lane != 63 && gr == g)) return;
    // the last lane of its group in this wave
    const uint32_t wa = a.off[g] >> 6, wb = (a.off[g + 1] - 1u) >> 6;
    // the wave's last member says whether its group goes on into the next wave
    if (lane == 63 || i == (uint64_t)a.K - 1) a.cross[w] = wa != wb && w == wa ? g : CROSS_NONE;
    if (wa == wb) { // the whole group is in this wave
#pragma unroll
        for (int k = 0; k < NT; ++k) a.moments[(size_t)g * NT + k] = t[k];
        a.dmax[g] = dm;
        return;
    }
    const size_t slot = 2 * (size_t)w + (w == wa ? 1u : 0u);
#pragma unroll
    for (int k = 0; k < NT; ++k) a.partial[slot * NT + k] = t[k];
    a.pdmax[slot] = dm;
}

// The blocks stride over the waves of the moment kernel; a block whose wave
// is the first of a crossing group combines that group.  Its partials are slot
// 2 wa + 1 (the wave it starts in) and slots 2 w, wa < w <= wb.  Thread t sums
// partials t, t + TB, ... in that order; the 64 lanes of a wave are joined by
// a butterfly, the waves in order.
template <int NT>
__global__ void __launch_bounds__(TB) group_combine_kernel(MomentArgs a) {
    __shared__ double sh[WPB][NT];
    __shared__ float shd[WPB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t c = blockIdx.x; c < a.nwaves; c += gridDim.x) {
        const uint32_t g = a.cross[c];
        if (g == CROSS_NONE) continue; // (the same for every thread of the block)
        const uint32_t wa = a.off[g] >> 6, wb = (a.off[g + 1] - 1u) >> 6;
        const uint32_t np = wb - wa + 1u;
        double t[NT];
#pragma unroll
        for (int k = 0; k < NT; ++k) t[k] = 0.0;
        float dm = 0.0f;
        for (uint32_t j = threadIdx.x; j < np; j += TB) {
            const size_t slot = j == 0 ? 2 * (size_t)wa + 1 : 2 * ((size_t)wa + j);
#pragma unroll
            for (int k = 0; k < NT; ++k) t[k] += a.partial[slot * NT + k];
            dm = fmaxf(dm, a.pdmax[slot]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
            for (int k = 0; k < NT; ++k) t[k] += __shfl_xor(t[k], o, 64);
            dm = fmaxf(dm, __shfl_xor(dm, o, 64));
        }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < NT; ++k) sh[wave][k] = t[k];
            shd[wave] = dm;
        }
        __syncthreads();
        if (threadIdx.x < NT) {
            double s = sh[0][threadIdx.x];
            for (int v = 1; v < WPB; ++v) s += sh[v][threadIdx.x];
            a.moments[(size_t)g * NT + threadIdx.x] = s;
        }
        if (threadIdx.x == 0) {
            float d = shd[0];
            for (int v = 1; v < WPB; ++v) d = fmaxf(d, shd[v]);
            a.dmax[g] = d;
        }
        __syncthreads();
    }
}

template <int NV>
void launch_moments_nv(const MomentArgs &a, bool periodic, unsigned blocks, hipStream_t s) {
    if (periodic)
        group_moments_kernel<NV, true><<<blocks, TB, 0, s>>>(a);
    else
        group_moments_kernel<NV, false><<<blocks, TB, 0, s>>>(a);
}

void launch_moments(const MomentArgs &a, int nv, bool periodic, unsigned blocks, hipStream_t s) {
    switch (nv) {
    case 0: launch_moments_nv<0>(a, periodic, blocks, s); break;
    case 1: launch_moments_nv<1>(a, periodic, blocks, s); break;
    case 2: launch_moments_nv<2>(a, periodic, blocks, s); break;
    case 3: launch_moments_nv<3>(a, periodic, blocks, s); break;
    default: launch_moments_nv<4>(a, periodic, blocks, s); break;
    }
}

void launch_combine(const MomentArgs &a, int nv, unsigned blocks, hipStream_t s) {
    switch (nv) {
    case 0: group_combine_kernel<NBKD_GROUP_MOMENTS(0)><<<blocks, TB, 0, s>>>(a); break;
    case 1: group_combine_kernel<NBKD_GROUP_MOMENTS(1)><<<blocks, TB, 0, s>>>(a); break;
    case 2: group_combine_kernel<NBKD_GROUP_MOMENTS(2)><<<blocks, TB, 0, s>>>(a); break;
    case 3: group_combine_kernel<NBKD_GROUP_MOMENTS(3)><<<blocks, TB, 0, s>>>(a); break;
    default: group_combine_kernel<NBKD_GROUP_MOMENTS(4)><<<blocks, TB, 0, s>>>(a); break;
    }
}

unsigned blocks_for(uint64_t n) { return (unsigned)((n + TB - 1) / TB); }

} // namespace

void launch_group_inv(const Tree &t, uint32_t *inv, hipStream_t s) {
    if (t.n8 == 0) return;
    const uint32_t *perm = t.sidx ? t.sidx : t.idx;
    group_inv_kernel<<<blocks_for(t.n8), TB, 0, s>>>(perm, (uint32_t)t.n8, (uint32_t)t.n, inv);
}

nbkd_status group_catalog(const Tree &t, const uint32_t *label, const float *weight,
                          const float *values, int nv, uint32_t min_members,
                          uint64_t group_capacity, uint64_t member_capacity,
                          uint64_t *out_ngroups, uint64_t *out_nmembers, uint32_t *out_head,
                          uint32_t *out_size, uint64_t *out_offsets, uint32_t *out_members,
                          double *out_moments, float *out_dmax, uint32_t flags, hipStream_t s) {
    *out_ngroups = 0;
    *out_nmembers = 0;
    if (t.n == 0) return NBKD_OK;
    const uint32_t n = (uint32_t)t.n, n8 = (uint32_t)t.n8; // n8 <= UINT32_MAX (build)
    const uint32_t mm = std::max(min_members, 1u);
    const bool in_dev = (flags & NBKD_INPUT_DEVICE) != 0;
    const bool out_dev = (flags & NBKD_OUTPUT_DEVICE) != 0;
    const int nt = NBKD_GROUP_MOMENTS(nv);
    Workspace &ws = acquire_ws(t);
    WsCall call(ws, s, std::adopt_lock);
    NBKD_HIP(call.err);

    // ---- the inputs on the device
    const uint32_t *dlabel = label;
    const float *dweight = weight, *dvalues = values;
    uint32_t *cnt = (uint32_t *)ws.get(WS_COUNT, (size_t)n * 4, s);
    uint32_t *pos = (uint32_t *)ws.get(WS_OFF, (size_t)n * 4, s);
    uint32_t *gidx = (uint32_t *)ws.get(WS_IDX, (size_t)n * 4, s);
    unsigned long long *ctr = (unsigned long long *)ws.get(WS_HTOT, C_N * 8, s);
    if (!cnt || !pos || !gidx || !ctr) return NBKD_ENOMEM;
    if (!in_dev) {
        uint32_t *ul = (uint32_t *)ws.get(WS_Q, (size_t)n * 4, s);
        float *uw = weight ? (float *)ws.get(WS_HRAD, (size_t)n * 4, s) : nullptr;
        float *uv = values ? (float *)ws.get(WS_VALS, (size_t)n * (size_t)nv * 4, s) : nullptr;
        if (!ul || (weight && !uw) || (values && !uv)) return NBKD_ENOMEM;
        NBKD_HIP(hipMemcpyAsync(ul, label, (size_t)n * 4, hipMemcpyHostToDevice, s));
        if (weight) NBKD_HIP(hipMemcpyAsync(uw, weight, (size_t)n * 4, hipMemcpyHostToDevice, s));
        if (values)
            NBKD_HIP(hipMemcpyAsync(uv, values, (size_t)n * (size_t)nv * 4, hipMemcpyHostToDevice,
                                    s));
        NBKD_HIP(hipStreamSynchronize(s)); // the caller's arrays have been read
        dlabel = ul;
        dweight = uw;
        dvalues = uv;
    }

    // ---- validate, count, flag; G and K
    NBKD_HIP(hipMemsetAsync(cnt, 0, (size_t)n * 4, s));
    NBKD_HIP(hipMemsetAsync(ctr, 0, C_N * 8, s));
    group_hist_kernel<<<(unsigned)(((uint64_t)n + HIST_TILE - 1) / HIST_TILE), TB, 0, s>>>(
        dlabel, n, cnt, ctr);
    group_flag_kernel<<<std::min(blocks_for(n), FLAG_BLOCKS), TB, 0, s>>>(dlabel, n, cnt, mm, pos,
                                                                         gidx, ctr);
    NBKD_HIP(hipGetLastError());
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "");
    uint64_t hc[3];
    NBKD_HIP(hipMemcpyAsync(hc, ctr, sizeof hc, hipMemcpyDeviceToHost, s));
    NBKD_HIP(hipStreamSynchronize(s));
    if (hc[C_BAD] != 0) {
        set_error("nbkd_group_catalog: " + std::to_string(hc[C_BAD]) +
                  " labels are not canonical (label[i] < n and label[label[i]] == label[i])");
        return NBKD_EINVAL;
    }
    const uint64_t G64 = hc[C_GROUPS], K64 = hc[C_ROWS];
    *out_ngroups = G64;
    *out_nmembers = K64;
    if (G64 > group_capacity || K64 > member_capacity || G64 == 0) return NBKD_OK;
    const uint32_t G = (uint32_t)G64, K = (uint32_t)K64;
    const uint32_t nwaves = (K + 63u) / 64u;

    // ---- scratch and outputs (device outputs are written in place)
    uint32_t *k0 = (uint32_t *)ws.get(WS_KEYS, (size_t)K * 4, s);
    uint32_t *k1 = (uint32_t *)ws.get(WS_KEYS2, (size_t)K * 4, s);
    uint32_t *v0 = (uint32_t *)ws.get(WS_ORDER, (size_t)K * 4, s);
    uint32_t *v1 = (uint32_t *)ws.get(WS_TMP, (size_t)K * 4, s);
    uint32_t *off = (uint32_t *)ws.get(WS_LIST, ((size_t)G + 1) * 4, s);
    double *partial = (double *)ws.get(WS_CAND, (size_t)nwaves * 2 * (size_t)nt * 8, s);
    uint32_t *cross = (uint32_t *)ws.get(WS_CCOUNT, (size_t)nwaves * 4, s);
    if (!k0 || !k1 || !v0 || !v1 || !off || !partial || !cross) return NBKD_ENOMEM;
    uint32_t *head = out_dev && out_head ? out_head : (uint32_t *)ws.get(WS_OUTI, (size_t)G * 4, s);
    uint32_t *size = out_dev && out_size ? out_size : (uint32_t *)ws.get(WS_OUTD, (size_t)G * 4, s);
    float *dmax = out_dev && out_dmax ? out_dmax : (float *)ws.get(WS_KTHD, (size_t)G * 4, s);
    float *pdmax = (float *)ws.get(WS_KB, (size_t)nwaves * 2 * 4, s);
    double *mom = out_dev && out_moments ? out_moments
                                         : (double *)ws.get(WS_VT, (size_t)G * (size_t)nt * 8, s);
    uint64_t *off64 = nullptr;
    if (out_offsets) {
        off64 = out_dev ? out_offsets : (uint64_t *)ws.get(WS_LIST2, ((size_t)G + 1) * 8, s);
        if (!off64) return NBKD_ENOMEM;
    }
    if (!head || !size || !dmax || !pdmax || !mom) return NBKD_ENOMEM;

    // ---- the sorted member list
    uint32_t *keys = k0, *members = v0;
    {
        TimedScope ts("group_sort", s);
        nbkd_status rc = device_excl_scan(ws, pos, n, s);
        if (rc) return rc;
        rc = device_excl_scan(ws, gidx, n, s);
        if (rc) return rc;
        group_compact_kernel<<<blocks_for(n), TB, 0, s>>>(dlabel, n, cnt, mm, pos, gidx, k0, v0,
                                                         head, size);
        NBKD_HIP(hipGetLastError());
        if (G > 1) { // (one group: the compaction's row order is the result)
            const int nbits = 32 - __builtin_clz(G - 1);
            rc = radix_sort(ws, k0, v0, k1, v1, K, nbits, s, &members);
            if (rc) return rc;
            keys = members == v0 ? k0 : k1;
        }
        group_offsets_kernel<<<blocks_for(K), TB, 0, s>>>(keys, K, G, off, off64);
        NBKD_HIP(hipGetLastError());
    }

    // ---- moments: pos is free now and holds row -> tree position
    uint32_t *inv = pos;
    const uint32_t *perm = t.sidx ? t.sidx : t.idx;
    MomentArgs a{t.p4, inv, keys,  members, head,  off,   dweight, dvalues,
                 K,    t.box, mom, dmax,    partial, pdmax, cross,   nwaves};
    {
        TimedScope ts("group_moments", s);
        group_inv_kernel<<<blocks_for(n8), TB, 0, s>>>(perm, n8, n, inv);
        launch_moments(a, nv, t.periodic != 0, (nwaves + WPB - 1) / WPB, s);
        NBKD_HIP(hipGetLastError());
    }
    {
        TimedScope ts("group_combine", s);
        launch_combine(a, nv, std::min(nwaves, COMBINE_BLOCKS), s);
        NBKD_HIP(hipGetLastError());
    }

    // ---- the outputs
    const hipMemcpyKind kind = out_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (out_members) NBKD_HIP(hipMemcpyAsync(out_members, members, (size_t)K * 4, kind, s));
    if (!out_dev) {
        if (out_head) NBKD_HIP(hipMemcpyAsync(out_head, head, (size_t)G * 4, kind, s));
        if (out_size) NBKD_HIP(hipMemcpyAsync(out_size, size, (size_t)G * 4, kind, s));
        if (out_dmax) NBKD_HIP(hipMemcpyAsync(out_dmax, dmax, (size_t)G * 4, kind, s));
        if (out_offsets)
            NBKD_HIP(hipMemcpyAsync(out_offsets, off64, ((size_t)G + 1) * 8, kind, s));
        if (out_moments)
            NBKD_HIP(hipMemcpyAsync(out_moments, mom, (size_t)G * (size_t)nt * 8, kind, s));
    }
    NBKD_HIP(hipStreamSynchronize(s));
    return NBKD_OK;
}

} // namespace nbkd
