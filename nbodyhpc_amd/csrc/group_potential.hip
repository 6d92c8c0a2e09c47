// Per-group potentials (NEW, nbkd_group_potential: the reference has no force
// calculation): for every entry e of a list of row groups (CSR: offsets,
// members, as nbkd_group_catalog writes them) the potential of its own group's
// other entries at its position, a direct sum under the tree's metric (the
// minimum image on a periodic tree), and per group the entry of lowest
// potential.  G = 1, Plummer softening eps; a term is the potential part of
// gravity.hip's grav_term.  nbkd.h states every step.
//
// Pipeline (K entries, G groups, n rows):
//   validate  counts offsets[0] != 0, offsets[G] != K, decreasing offsets and
//             members[e] >= n; the host reads the count before anything else
//             runs, so no later kernel indexes with an unchecked row or offset
//   inv       row -> tree position (group.hip's scatter of the build permutation)
//   gather    pm[e] = (x, y, z of row members[e], its mass), gid[e] = the
//             entry's group (an upper-bound search in offsets: empty groups
//             are stepped over)
//   sum       lane = one entry, wave = 64 consecutive entries.  The wave stages
//             pm from the start of its first lane's group to the end of its
//             last lane's group into LDS, TILE entries per step with the 16-B
//             direct-to-LDS load, and every lane adds the staged entries of its
//             own [start, end) in list order: LDS is read at a wave-uniform
//             address (a broadcast).  A tile every lane wants whole (a wave
//             inside one large group) runs without the range test.  Four
//             entries per step; gpot_inv_fast shortens 1.0f / sqrtf(r2) where
//             every lane's radicands allow it, with the same bits.
//   argmin    keys[g] = min over the group's entries of (fkey(phi) << 32 | e),
//             a 64-bit integer atomicMin per entry, or one per wave when the
//             wave lies in one group; then minpos[g] = the low word
//
// Determinism.  One lane sums one entry into one float64 accumulator in list
// order; a masked term adds +0.0, which changes no bit.  Which wave holds an
// entry, the tile bounds and the grid change only what is staged when, never a
// term or its place in the order.  The integer minimum commutes.  No
// floating-point atomics.
#include <algorithm>
#include <string>

#include "internal.hpp"
#include "metric.hpp"
#include "packet.hpp"

namespace nbkd {
namespace {
using namespace dev;

constexpr int TB = 256;
constexpr int WPB = TB / 64;
constexpr uint32_t TILE = 256; // staged entries per step: 4 KiB of LDS per wave
constexpr uint32_t VALIDATE_BLOCKS = 1024;
constexpr uint32_t NO_ENTRY = 0xFFFFFFFFu;

unsigned blocks_for(uint64_t n) { return (unsigned)((n + TB - 1) / TB); }

// a fixed grid strides over the offsets and the members; one global integer
// atomic per block that saw a violation
__global__ void __launch_bounds__(TB)
gpot_validate_kernel(const uint64_t *__restrict__ off, const uint32_t *__restrict__ members,
                     uint32_t G, uint32_t K, uint32_t n, unsigned long long *bad) {
    __shared__ uint32_t tot;
    if (threadIdx.x == 0) tot = 0u;
    __syncthreads();
    uint32_t nb = 0;
    const uint64_t stride = (uint64_t)gridDim.x * TB;
    for (uint64_t g = (uint64_t)blockIdx.x * TB + threadIdx.x; g <= G; g += stride) {
        const uint64_t o = off[g];
        if (g == 0 && o != 0) ++nb;
        if (g == G && o != K) ++nb;
        if (g < G && o > off[g + 1]) ++nb;
    }
    for (uint64_t e = (uint64_t)blockIdx.x * TB + threadIdx.x; e < K; e += stride)
        if (members[e] >= n) ++nb;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nb += __shfl_xor(nb, o, 64);
    if ((threadIdx.x & 63) == 0 && nb) atomicAdd(&tot, nb);
    __syncthreads();
    if (threadIdx.x == 0 && tot) atomicAdd(bad, (unsigned long long)tot);
}

// (validated: members[e] < n; offsets non-decreasing from 0 to K, so the group
// with off[g] <= e < off[g + 1] exists and the search stays inside off[0 .. G])
__global__ void __launch_bounds__(TB)
gpot_gather_kernel(const float4 *__restrict__ p4, const uint32_t *__restrict__ inv,
                   const uint64_t *__restrict__ off, const uint32_t *__restrict__ members,
                   const float *__restrict__ mass, uint32_t G, uint32_t K,
                   float4 *__restrict__ pm, uint32_t *__restrict__ gid) {
    const uint64_t e = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (e >= K) return;
    const uint32_t row = members[e];
    const float4 p = p4[inv[row]];
    pm[e] = make_float4(p.x, p.y, p.z, mass ? mass[row] : 1.0f);
    // the first g in [1, G] with off[g] > e (off[G] = K > e); its predecessor
    // holds e, and is never an empty group
    uint32_t lo = 1, hi = G;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] > e)
            hi = mid;
        else
            lo = mid + 1;
    }
    gid[e] = lo - 1u;
}

// 1.0f / sqrtf(r2) for r2 in [2^-96, FLT_MAX]: the correctly rounded square root
// and division as the compiler expands them, without the parts this range
// never needs (the 2^32 pre-scaling of a tiny radicand, the division's operand
// scaling and its fix-up of zeros, infinities and denormal quotients: s lies
// in [2^-48, 2^64], 1/s in [2^-64, 2^48]).  Same operations on the same values,
// so the same bits.  The hardware square root is within one ulp; the two
// residuals pick the neighbour that is correctly rounded.
__device__ __forceinline__ float gpot_inv_fast(float r2) {
    float s = __builtin_amdgcn_sqrtf(r2);
    const float sd = __builtin_bit_cast(float, __builtin_bit_cast(int, s) - 1);
    const float su = __builtin_bit_cast(float, __builtin_bit_cast(int, s) + 1);
    const float vd = __builtin_fmaf(-sd, s, r2), vu = __builtin_fmaf(-su, s, r2);
    s = vd <= 0.0f ? sd : s;
    s = vu > 0.0f ? su : s;
    float r = __builtin_amdgcn_rcpf(s);
    r = __builtin_fmaf(__builtin_fmaf(-s, r, 1.0f), r, r);
    float q = r; // (the numerator 1 times r)
    q = __builtin_fmaf(__builtin_fmaf(-s, q, 1.0f), r, q);
    return __builtin_fmaf(__builtin_fmaf(-s, q, 1.0f), r, q);
}
constexpr float INV_FAST_MIN = 0x1p-96f;

// cn staged entries W[0 .. cn): the potential terms of the entries u with
// u - ua < un (MASKED), or of all of them.  Four entries per step: when every
// lane's four radicands are in gpot_inv_fast's range (a wave-uniform branch;
// the exceptions are a lane's own entry and coincident points at eps = 0) the
// short form runs, else the plain expression; both give the same bits.
template <bool PER, bool MASKED>
__device__ __forceinline__ void gpot_tile(const float4 *W, uint32_t cn, uint32_t ua, uint32_t un,
                                          float px, float py, float pz, float eps2, float L,
                                          double &acc) {
    uint32_t u = 0;
    for (; u + 4 <= cn; u += 4) {
        float r2[4], mu[4], inv[4];
        bool on[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float4 a = W[u + k];
            const float d2 = point_d2<PER>(px, py, pz, a.x, a.y, a.z, L);
            on[k] = !(d2 == 0.0f); // the entry itself, a repeated row, a coincident point
            if constexpr (MASKED) on[k] = on[k] && (u + k - ua) < un;
            r2[k] = d2 + eps2;
            mu[k] = a.w;
        }
        const float mn = fminf(fminf(r2[0], r2[1]), fminf(r2[2], r2[3]));
        const float mx = fmaxf(fmaxf(r2[0], r2[1]), fmaxf(r2[2], r2[3]));
        if (__all(mn >= INV_FAST_MIN && mx <= FLT_MAX)) {
#pragma unroll
            for (int k = 0; k < 4; ++k) inv[k] = gpot_inv_fast(r2[k]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) inv[k] = 1.0f / sqrtf(r2[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float t = mu[k] * inv[k];
            acc += (double)(on[k] ? t : 0.0f);
        }
    }
    for (; u < cn; ++u) {
        const float4 a = W[u];
        const float d2 = point_d2<PER>(px, py, pz, a.x, a.y, a.z, L);
        const float r2 = d2 + eps2;
        const float inv = 1.0f / sqrtf(r2);
        const float t = a.w * inv;
        bool on = !(d2 == 0.0f);
        if constexpr (MASKED) on = on && (u - ua) < un;
        acc += (double)(on ? t : 0.0f);
    }
}

template <bool PER>
__global__ void __launch_bounds__(TB)
gpot_sum_kernel(const float4 *__restrict__ pm, const uint32_t *__restrict__ gid,
                const uint64_t *__restrict__ off, uint32_t K, uint32_t max_members, float eps2,
                float L, float *__restrict__ out_phi) {
    __shared__ float4 Wl[WPB][TILE];
    const int lane = threadIdx.x & 63;
    float4 *W = Wl[wave_id()];
    const uint64_t e = ((uint64_t)xcd_block(blockIdx.x, gridDim.x) * WPB + (threadIdx.x >> 6)) * 64u +
                       (uint32_t)lane;
    bool active = e < K;
    uint32_t s0 = 0, s1 = 0;
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (active) {
        const uint32_t g = gid[e];
        s0 = (uint32_t)off[g];
        s1 = (uint32_t)off[g + 1];
        if (max_members != 0u && s1 - s0 > max_members) { // a skipped group
            out_phi[e] = __builtin_nanf("");
            active = false;
        } else {
            const float4 p = pm[e];
            px = p.x;
            py = p.y;
            pz = p.z;
        }
    }
    const uint64_t am = __ballot(active);
    if (am == 0) return; // (the same for the whole wave)
    // the entries are in list order: the wave's range runs from its first
    // active lane's group start to its last active lane's group end
    if (!active) s0 = s1 = 0u;
    const uint32_t lo = uni((uint32_t)__shfl((int)s0, __builtin_ctzll(am), 64));
    const uint32_t hi = uni((uint32_t)__shfl((int)s1, 63 - __builtin_clzll(am), 64));
    double acc = 0.0;
    for (uint32_t c0 = lo; c0 < hi; c0 += TILE) {
        const uint32_t cn = min(TILE, hi - c0);
        wave_sync();
#pragma unroll
        for (uint32_t k = 0; k < TILE; k += 64)
            if (k < cn) glds_f4(pm + c0 + k, W + k, lane, cn - k);
        wait_vm0();
        wave_sync();
        // this lane's part of the tile: u in [ua, ua + un)
        const uint32_t a = max(s0, c0), b = min(s1, c0 + cn);
        const uint32_t ua = a - c0, un = b > a ? b - a : 0u;
        if (__all(un == cn))
            gpot_tile<PER, false>(W, cn, 0u, 0u, px, py, pz, eps2, L, acc);
        else
            gpot_tile<PER, true>(W, cn, ua, un, px, py, pz, eps2, L, acc);
    }
    if (active) out_phi[e] = (float)(-acc);
}

// the key of entry e: the order of the float32 values written (-0 and +0 are
// equal: one key), then the smaller e
__device__ __forceinline__ unsigned long long gpot_key(float phi, uint32_t e) {
    return ((unsigned long long)fkey(phi + 0.0f) << 32) | e;
}

__global__ void __launch_bounds__(TB)
gpot_argmin_kernel(const float *__restrict__ phi, const uint32_t *__restrict__ gid,
                   const uint64_t *__restrict__ off, uint32_t K, uint32_t max_members,
                   unsigned long long *keys) {
    const uint64_t e = (uint64_t)blockIdx.x * TB + threadIdx.x;
    const bool active = e < K;
    uint32_t g = NO_ENTRY;
    unsigned long long key = ~0ull;
    if (active) {
        g = gid[e];
        // (a skipped group keeps its key of all ones)
        if (max_members == 0u || (uint32_t)(off[g + 1] - off[g]) <= max_members)
            key = gpot_key(phi[e], (uint32_t)e);
    }
    if (__all(g == uni(g))) { // one group (or nothing) in the wave: one atomic
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long y = __shfl_xor(key, o, 64);
            key = y < key ? y : key;
        }
        if ((threadIdx.x & 63) == 0 && key != ~0ull) atomicMin(keys + g, key);
    } else if (key != ~0ull) {
        atomicMin(keys + g, key);
    }
}

// minpos[g] = the entry in the low word of the group's key (all ones: no entry)
__global__ void __launch_bounds__(TB)
gpot_minpos_kernel(const unsigned long long *__restrict__ keys, uint32_t G,
                   uint32_t *__restrict__ minpos) {
    const uint64_t g = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (g < G) minpos[g] = (uint32_t)keys[g];
}

} // namespace

nbkd_status group_potential(const Tree &t, const uint64_t *offsets, const uint32_t *members,
                            uint64_t ngroups, uint64_t nmembers, const float *mass, float eps,
                            uint32_t max_members, float *out_phi, uint32_t *out_minpos,
                            uint32_t flags, hipStream_t s) {
    const uint32_t G = (uint32_t)ngroups, K = (uint32_t)nmembers;
    const uint32_t n = (uint32_t)t.n; // n <= n8 <= UINT32_MAX (build)
    const bool in_dev = (flags & NBKD_INPUT_DEVICE) != 0;
    const bool out_dev = (flags & NBKD_OUTPUT_DEVICE) != 0;
    Workspace &ws = acquire_ws(t);
    WsCall call(ws, s, std::adopt_lock);
    NBKD_HIP(call.err);

    // ---- the inputs on the device
    const uint64_t *doff = offsets;
    const uint32_t *dmem = members;
    const float *dmass = mass;
    unsigned long long *bad = (unsigned long long *)ws.get(WS_HTOT, 8, s);
    if (!bad) return NBKD_ENOMEM;
    if (!in_dev) {
        uint64_t *uo = (uint64_t *)ws.get(WS_LIST2, ((size_t)G + 1) * 8, s);
        uint32_t *um = (uint32_t *)ws.get(WS_Q, (size_t)K * 4, s);
        float *uw = mass ? (float *)ws.get(WS_HRAD, (size_t)n * 4, s) : nullptr;
        if (!uo || !um || (mass && !uw)) return NBKD_ENOMEM;
        NBKD_HIP(hipMemcpyAsync(uo, offsets, ((size_t)G + 1) * 8, hipMemcpyHostToDevice, s));
        NBKD_HIP(hipMemcpyAsync(um, members, (size_t)K * 4, hipMemcpyHostToDevice, s));
        if (mass && n) NBKD_HIP(hipMemcpyAsync(uw, mass, (size_t)n * 4, hipMemcpyHostToDevice, s));
        NBKD_HIP(hipStreamSynchronize(s)); // the caller's arrays have been read
        doff = uo;
        dmem = um;
        dmass = uw;
    }

    // ---- validate: the count is read before anything is indexed or written
    {
        TimedScope ts("gpot_validate", s);
        NBKD_HIP(hipMemsetAsync(bad, 0, 8, s));
        const uint64_t items = std::max<uint64_t>((uint64_t)G + 1, K);
        gpot_validate_kernel<<<std::min(blocks_for(items), VALIDATE_BLOCKS), TB, 0, s>>>(
            doff, dmem, G, K, n, bad);
        NBKD_HIP(hipGetLastError());
    }
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "");
    uint64_t nbad = 0;
    NBKD_HIP(hipMemcpyAsync(&nbad, bad, 8, hipMemcpyDeviceToHost, s));
    NBKD_HIP(hipStreamSynchronize(s));
    if (nbad != 0) {
        set_error("nbkd_group_potential: " + std::to_string(nbad) +
                  " violations (offsets[0] == 0, offsets non-decreasing, offsets[ngroups] == "
                  "nmembers, members[e] < n)");
        return NBKD_EINVAL;
    }

    // ---- scratch and outputs (device outputs are written in place)
    float4 *pm = (float4 *)ws.get(WS_CAND, (size_t)K * 16, s);
    uint32_t *gid = (uint32_t *)ws.get(WS_KEYS, (size_t)K * 4, s);
    uint32_t *inv = (uint32_t *)ws.get(WS_OFF, (size_t)n * 4, s);
    if (!pm || !gid || !inv) return NBKD_ENOMEM;
    float *phi = out_dev && out_phi ? out_phi : (float *)ws.get(WS_OUTD, (size_t)K * 4, s);
    if (!phi) return NBKD_ENOMEM;
    unsigned long long *keys = nullptr;
    uint32_t *minpos = nullptr;
    if (out_minpos) {
        keys = (unsigned long long *)ws.get(WS_VT, (size_t)G * 8, s);
        minpos = out_dev ? out_minpos : (uint32_t *)ws.get(WS_OUTI, (size_t)G * 4, s);
        if (!keys || !minpos) return NBKD_ENOMEM;
    }

    {
        TimedScope ts("gpot_gather", s);
        launch_group_inv(t, inv, s);
        gpot_gather_kernel<<<blocks_for(K), TB, 0, s>>>(t.p4, inv, doff, dmem, dmass, G, K, pm,
                                                        gid);
        NBKD_HIP(hipGetLastError());
    }
    {
        TimedScope ts("gpot_sum", s);
        const unsigned blocks = (unsigned)(((uint64_t)K + TB - 1) / TB);
        const float eps2 = eps * eps;
        if (t.periodic)
            gpot_sum_kernel<true><<<blocks, TB, 0, s>>>(pm, gid, doff, K, max_members, eps2,
                                                        t.box, phi);
        else
            gpot_sum_kernel<false><<<blocks, TB, 0, s>>>(pm, gid, doff, K, max_members, eps2,
                                                         t.box, phi);
        NBKD_HIP(hipGetLastError());
    }
    if (out_minpos) {
        TimedScope ts("gpot_argmin", s);
        NBKD_HIP(hipMemsetAsync(keys, 0xFF, (size_t)G * 8, s));
        gpot_argmin_kernel<<<blocks_for(K), TB, 0, s>>>(phi, gid, doff, K, max_members, keys);
        gpot_minpos_kernel<<<blocks_for(G), TB, 0, s>>>(keys, G, minpos);
        NBKD_HIP(hipGetLastError());
    }

    // ---- the outputs
    if (!out_dev) {
        if (out_phi) NBKD_HIP(hipMemcpyAsync(out_phi, phi, (size_t)K * 4, hipMemcpyDeviceToHost, s));
        if (out_minpos)
            NBKD_HIP(hipMemcpyAsync(out_minpos, minpos, (size_t)G * 4, hipMemcpyDeviceToHost, s));
    }
    NBKD_HIP(hipStreamSynchronize(s));
    return NBKD_OK;
}

} // namespace nbkd
