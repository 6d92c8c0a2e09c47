// The sorting primitives of libnbkd.so for gfx950: the LSD radix sort of
// (key, value) pairs (one-sweep, or histogram + scan + scatter per pass) and
// the exclusive scan of a uint32 array.  query.hip sorts the queries by leaf
// with them and compacts its failure bitmaps; group.hip orders group members.
#include <algorithm>

#include "internal.hpp"
#include "metric.hpp"

namespace nbkd {
namespace {
using namespace dev;

constexpr int TB = 256;
constexpr int WPB = TB / 64; // waves per block

// ------------------------------------------------------------------ LSD radix sort (keys + values)
constexpr int RS_ITEMS = 8;
constexpr int RS_TILE = TB * RS_ITEMS; // 2048

__global__ void __launch_bounds__(TB)
rs_hist_kernel(const uint32_t *__restrict__ keys, uint32_t n, int shift, uint32_t ntiles,
               uint32_t *__restrict__ hist) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * RS_TILE;
#pragma unroll
    for (int r = 0; r < RS_ITEMS; ++r) {
        uint32_t e = base + r * TB + threadIdx.x;
        if (e < n) atomicAdd(&h[(keys[e] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * ntiles + blockIdx.x] = h[threadIdx.x];
}

__global__ void __launch_bounds__(TB)
rs_scatter_kernel(const uint32_t *__restrict__ kin, const uint32_t *__restrict__ vin, uint32_t n,
                  int shift, uint32_t ntiles, const uint32_t *__restrict__ hist_scanned,
                  uint32_t *__restrict__ kout, uint32_t *__restrict__ vout) {
    __shared__ uint16_t cnt[RS_ITEMS][WPB][256];
    __shared__ uint32_t gofs[256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int j = threadIdx.x; j < RS_ITEMS * WPB * 256; j += TB) (&cnt[0][0][0])[j] = 0;
    gofs[threadIdx.x] = hist_scanned[(size_t)threadIdx.x * ntiles + blockIdx.x];
    __syncthreads();
    const uint32_t base = blockIdx.x * RS_TILE;
    uint32_t kk[RS_ITEMS], vv[RS_ITEMS], rk[RS_ITEMS];
#pragma unroll
    for (int r = 0; r < RS_ITEMS; ++r) {
        uint32_t e = base + r * TB + threadIdx.x;
        bool valid = e < n;
        kk[r] = valid ? kin[e] : 0u;
        vv[r] = valid ? vin[e] : 0u;
        uint32_t d = (kk[r] >> shift) & 255u;
        uint64_t same = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            uint64_t bb = __ballot((d >> b) & 1u);
            same &= ((d >> b) & 1u) ? bb : ~bb;
        }
        uint32_t below = mbcnt64(same);
        rk[r] = below;
        if (valid && below == 0) cnt[r][wave][d] = (uint16_t)__popcll(same);
    }
    __syncthreads();
    { // per digit: exclusive prefix over (round, wave) in element order
        uint32_t acc = 0;
        const int d = threadIdx.x;
        for (int r = 0; r < RS_ITEMS; ++r)
            for (int w = 0; w < WPB; ++w) {
                uint32_t v = cnt[r][w][d];
                cnt[r][w][d] = (uint16_t)acc;
                acc += v;
            }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RS_ITEMS; ++r) {
        uint32_t e = base + r * TB + threadIdx.x;
        if (e < n) {
            uint32_t d = (kk[r] >> shift) & 255u;
            uint32_t dst = gofs[d] + cnt[r][wave][d] + rk[r];
            kout[dst] = kk[r];
            vout[dst] = vv[r];
        }
    }
    (void)lane;
}

// exclusive scan of a uint32 array, 3 kernels
constexpr int SC_ITEMS = 16;
constexpr int SC_TILE = TB * SC_ITEMS;

__device__ __forceinline__ uint32_t block_scan_excl(uint32_t v, uint32_t *sh, uint32_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nw = blockDim.x / 64;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) sh[wave] = x;
    __syncthreads();
    uint32_t base = 0, tot = 0;
    for (int w = 0; w < nw; ++w) {
        uint32_t s = sh[w];
        if (w < wave) base += s;
        tot += s;
    }
    if (total) *total = tot;
    __syncthreads();
    return base + x - v;
}

__global__ void __launch_bounds__(TB)
scan_up_kernel(const uint32_t *__restrict__ a, uint64_t n, uint32_t *__restrict__ sums) {
    __shared__ uint32_t sh[WPB];
    const uint64_t base = (uint64_t)blockIdx.x * SC_TILE + (uint64_t)threadIdx.x * SC_ITEMS;
    uint32_t s = 0;
#pragma unroll
    for (int j = 0; j < SC_ITEMS; ++j)
        if (base + j < n) s += a[base + j];
    uint32_t tot;
    block_scan_excl(s, sh, &tot);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(1024) scan_mid_kernel(uint32_t *__restrict__ sums, uint32_t nb) {
    __shared__ uint32_t sh[16];
    const uint32_t per = (nb + 1023) / 1024;
    const uint32_t b0 = threadIdx.x * per, b1 = min(b0 + per, nb);
    uint32_t s = 0;
    for (uint32_t b = b0; b < b1; ++b) s += sums[b];
    uint32_t ex = block_scan_excl(s, sh, nullptr);
    for (uint32_t b = b0; b < b1; ++b) {
        uint32_t v = sums[b];
        sums[b] = ex;
        ex += v;
    }
}

__global__ void __launch_bounds__(TB)
scan_down_kernel(uint32_t *__restrict__ a, uint64_t n, const uint32_t *__restrict__ sums) {
    __shared__ uint32_t sh[WPB];
    const uint64_t base = (uint64_t)blockIdx.x * SC_TILE + (uint64_t)threadIdx.x * SC_ITEMS;
    uint32_t v[SC_ITEMS], s = 0;
#pragma unroll
    for (int j = 0; j < SC_ITEMS; ++j) {
        v[j] = base + j < n ? a[base + j] : 0u;
        s += v[j];
    }
    uint32_t ex = block_scan_excl(s, sh, nullptr) + sums[blockIdx.x];
#pragma unroll
    for (int j = 0; j < SC_ITEMS; ++j) {
        if (base + j < n) a[base + j] = ex;
        ex += v[j];
    }
}

} // namespace

nbkd_status device_excl_scan(Workspace &ws, uint32_t *a, uint64_t n, hipStream_t s) {
    if (n == 0) return NBKD_OK;
    uint64_t nb = (n + SC_TILE - 1) / SC_TILE;
    uint32_t *sums = (uint32_t *)ws.get(WS_SUMS, nb * 4, s);
    if (!sums) return NBKD_ENOMEM;
    scan_up_kernel<<<(unsigned)nb, TB, 0, s>>>(a, n, sums);
    scan_mid_kernel<<<1, 1024, 0, s>>>(sums, (uint32_t)nb);
    scan_down_kernel<<<(unsigned)nb, TB, 0, s>>>(a, n, sums);
    NBKD_HIP(hipGetLastError());
    return NBKD_OK;
}

namespace {

// ------------------------------------------------------------------ one-sweep LSD radix sort
// One histogram read of the keys for all passes, then per 8-bit pass ONE kernel:
// each 4096-item tile ranks its items (stable), publishes its digit counts,
// finds its global digit offsets by decoupled look-back over the tiles before
// it (tiles are numbered in start order by an atomic ticket, so every tile it
// waits on is running), stages the tile digit-sorted in LDS and writes it out
// in digit runs.  Per pass: 8 B read + 8 B written per item.
constexpr int OS_ITEMS = 16;
constexpr int OS_TILE = TB * OS_ITEMS; // 4096
constexpr uint32_t OS_AGG = 1u << 30, OS_PRE = 2u << 30, OS_VAL = OS_AGG - 1;
constexpr int OS_MAXP = 4;

__global__ void __launch_bounds__(TB)
os_hist_kernel(const uint32_t *__restrict__ keys, uint32_t n, int passes,
               uint32_t *__restrict__ ghist) {
    __shared__ uint32_t h[OS_MAXP][256];
    for (int j = threadIdx.x; j < OS_MAXP * 256; j += TB) (&h[0][0])[j] = 0;
    __syncthreads();
    for (uint32_t i = blockIdx.x * TB + threadIdx.x; i < n; i += gridDim.x * TB) {
        const uint32_t k = keys[i];
        for (int p = 0; p < passes; ++p) atomicAdd(&h[p][(k >> (8 * p)) & 255u], 1u);
    }
    __syncthreads();
    for (int p = 0; p < passes; ++p) {
        const uint32_t v = h[p][threadIdx.x];
        if (v) atomicAdd(&ghist[p * 256 + threadIdx.x], v);
    }
}

// exclusive scan of each pass's 256 counts, in place (one block)
__global__ void __launch_bounds__(TB) os_scan_kernel(uint32_t *__restrict__ ghist, int passes) {
    __shared__ uint32_t sh[WPB];
    for (int p = 0; p < passes; ++p) {
        const uint32_t v = ghist[p * 256 + threadIdx.x];
        ghist[p * 256 + threadIdx.x] = block_scan_excl(v, sh, nullptr);
    }
}

__global__ void __launch_bounds__(TB)
os_pass_kernel(const uint32_t *__restrict__ kin, const uint32_t *__restrict__ vin, uint32_t n,
               int shift, const uint32_t *__restrict__ gexcl, uint32_t *__restrict__ status,
               uint32_t *__restrict__ ticket, uint32_t *__restrict__ kout,
               uint32_t *__restrict__ vout) {
    __shared__ uint32_t wh[WPB][256]; // per wave digit counts, then wave-exclusive offsets
    __shared__ uint32_t ls[256];      // tile-local digit start
    __shared__ uint32_t gofs[256];    // global position of local index 0 of digit d
    __shared__ uint32_t sk[OS_TILE], sv[OS_TILE];
    __shared__ uint32_t sh[WPB];
    __shared__ uint32_t tile_sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) tile_sh = atomicAdd(ticket, 1u);
    for (int j = tid; j < WPB * 256; j += TB) (&wh[0][0])[j] = 0;
    __syncthreads();
    const uint32_t tile = tile_sh;
    const uint32_t t0 = tile * (uint32_t)OS_TILE;
    const uint32_t base = t0 + (uint32_t)wave * (OS_ITEMS * 64);
    uint32_t kk[OS_ITEMS], vv[OS_ITEMS], rk[OS_ITEMS];
#pragma unroll
    for (int r = 0; r < OS_ITEMS; ++r) {
        const uint32_t e = base + r * 64 + lane;
        kk[r] = e < n ? kin[e] : 0xFFFFFFFFu;
        vv[r] = e < n ? vin[e] : 0u;
    }
    // stable rank: items of wave w in element order, round by round
#pragma unroll
    for (int r = 0; r < OS_ITEMS; ++r) {
        const uint32_t e = base + r * 64 + lane;
        const uint32_t d = (kk[r] >> shift) & 255u;
        uint64_t same = __ballot(e < n);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const uint64_t bb = __ballot((d >> b) & 1u);
            same &= ((d >> b) & 1u) ? bb : ~bb;
        }
        const uint32_t below = mbcnt64(same);
        const uint32_t old = wh[wave][d];
        rk[r] = old + below;
        if (e < n && below == 0) wh[wave][d] = old + (uint32_t)__popcll(same);
    }
    __syncthreads();
    {
        const int d = tid;
        uint32_t c = 0;
#pragma unroll
        for (int w = 0; w < WPB; ++w) {
            const uint32_t x = wh[w][d];
            wh[w][d] = c;
            c += x;
        }
        uint32_t *st = status + (size_t)tile * 256 + d;
        __hip_atomic_store(st, (tile == 0 ? OS_PRE : OS_AGG) | c, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t lsd = block_scan_excl(c, sh, nullptr);
        ls[d] = lsd;
        uint32_t acc = 0;
        if (tile > 0) {
            uint32_t tt = tile - 1;
            for (;;) {
                const uint32_t v = __hip_atomic_load(status + (size_t)tt * 256 + d, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT);
                if ((v >> 30) == 0) {
                    __builtin_amdgcn_s_sleep(1);
                    continue;
                }
                acc += v & OS_VAL;
                if (v & OS_PRE) break;
                --tt;
            }
            __hip_atomic_store(st, OS_PRE | (acc + c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        gofs[d] = gexcl[d] + acc - lsd;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < OS_ITEMS; ++r) {
        const uint32_t e = base + r * 64 + lane;
        if (e < n) {
            const uint32_t d = (kk[r] >> shift) & 255u;
            const uint32_t pos = ls[d] + wh[wave][d] + rk[r];
            sk[pos] = kk[r];
            sv[pos] = vv[r];
        }
    }
    __syncthreads();
    const uint32_t cnt = min((uint32_t)OS_TILE, n - t0);
#pragma unroll
    for (int r = 0; r < OS_ITEMS; ++r) {
        const uint32_t i = r * TB + tid;
        if (i < cnt) {
            const uint32_t k = sk[i];
            const uint32_t dst = gofs[(k >> shift) & 255u] + i;
            kout[dst] = k;
            vout[dst] = sv[i];
        }
    }
}

nbkd_status onesweep_sort(Workspace &ws, uint32_t *k0, uint32_t *v0, uint32_t *k1, uint32_t *v1,
                          uint32_t n, int passes, hipStream_t s) {
    const uint32_t ntiles = (n + OS_TILE - 1) / OS_TILE;
    // [passes][256] histogram | [passes] tickets (padded to 64 words) | [passes][ntiles][256] status
    const size_t words = (size_t)passes * 256 + 64 + (size_t)passes * ntiles * 256;
    uint32_t *w = (uint32_t *)ws.get(WS_HIST, words * 4, s);
    if (!w) return NBKD_ENOMEM;
    NBKD_HIP(hipMemsetAsync(w, 0, words * 4, s));
    uint32_t *ghist = w, *tickets = w + passes * 256, *status = tickets + 64;
    const unsigned hb = (unsigned)std::min<uint32_t>((n + TB - 1) / TB, 2048);
    os_hist_kernel<<<hb, TB, 0, s>>>(k0, n, passes, ghist);
    os_scan_kernel<<<1, TB, 0, s>>>(ghist, passes);
    for (int p = 0; p < passes; ++p) {
        uint32_t *ki = (p & 1) ? k1 : k0, *vi = (p & 1) ? v1 : v0;
        uint32_t *ko = (p & 1) ? k0 : k1, *vo = (p & 1) ? v0 : v1;
        os_pass_kernel<<<ntiles, TB, 0, s>>>(ki, vi, n, 8 * p, ghist + p * 256, status +
                                             (size_t)p * ntiles * 256, tickets + p, ko, vo);
    }
    NBKD_HIP(hipGetLastError());
    return NBKD_OK;
}

} // namespace

// sorts (keys, vals) by the low `nbits` of keys, ceil(nbits/8) LSD passes
// ping-ponging between (k0, v0) and (k1, v1); *vout = the sorted values
nbkd_status radix_sort(Workspace &ws, uint32_t *k0, uint32_t *v0, uint32_t *k1, uint32_t *v1,
                       uint32_t n, int nbits, hipStream_t s, uint32_t **vout) {
    *vout = v0;
    if (n <= 1) return NBKD_OK;
    {
        static const bool old_sort = knob("NBKD_OLD_SORT") != nullptr; // A/B only
        const int passes = (nbits + 7) / 8;
        if (!old_sort && n < OS_VAL && passes <= OS_MAXP) {
            *vout = (passes & 1) ? v1 : v0;
            return onesweep_sort(ws, k0, v0, k1, v1, n, passes, s);
        }
    }
    const uint32_t ntiles = (n + RS_TILE - 1) / RS_TILE;
    uint32_t *hist = (uint32_t *)ws.get(WS_HIST, (size_t)256 * ntiles * 4, s);
    if (!hist) return NBKD_ENOMEM;
    const int passes = (nbits + 7) / 8;
    *vout = (passes & 1) ? v1 : v0;
    for (int p = 0; p < passes; ++p) {
        const int shift = 8 * p;
        uint32_t *ki = (p & 1) ? k1 : k0, *vi = (p & 1) ? v1 : v0;
        uint32_t *ko = (p & 1) ? k0 : k1, *vo = (p & 1) ? v0 : v1;
        rs_hist_kernel<<<ntiles, TB, 0, s>>>(ki, n, shift, ntiles, hist);
        nbkd_status st = device_excl_scan(ws, hist, (uint64_t)256 * ntiles, s);
        if (st) return st;
        rs_scatter_kernel<<<ntiles, TB, 0, s>>>(ki, vi, n, shift, ntiles, hist, ko, vo);
        NBKD_HIP(hipGetLastError());
    }
    return NBKD_OK;
}

} // namespace nbkd
