// Barnes-Hut potentials and accelerations on a periodic tree (NEW,
// nbkd_gravity_ewald: the reference has no force calculation).  The sum over a
// point's periodic images is the nearest image's Newtonian term (gravity.hip's
// grav_term, Plummer softening on this part only) plus the Ewald correction
// (C_phi, C_a) of that offset, read from a table.  nbkd.h states every step.
//
// Three parts:
//   table    (NBKD_EWALD_N + 1)^3 nodes over [0, 1/2]^3 in units of the box, four
//            float32 each (C_phi, C_ax, C_ay, C_az), the node index of x
//            slowest.  Computed on the host in float64 once per process (the
//            real-space sum cut where erfc is far below the 2e-9 target, the
//            reciprocal sum from per-axis cos / sin tables, rows of the grid
//            handed to at most 16 host threads), uploaded once per device and
//            kept outside the workspaces.
//   moments  launch_gravity_moments, unchanged: the moments do not depend on
//            periodicity.
//   walk     gravity_walk_kernel's packet walk (mask stack, leaf staging, one
//            lane per query), with every offset wrapped per axis to its nearest
//            image (group.hip's rule) before the opening test and the term, and
//            the correction added after the Newtonian part: eight 16-B corner
//            loads at lane-divergent addresses per term, interpolated
//            trilinearly.  A query outside [0, L]^3 (or NaN) takes no part in
//            the walk and gets quiet NaNs.
#include <atomic>
#include <cmath>
#include <thread>

#include "gravity_dev.hpp"

namespace nbkd {
namespace {
using namespace dev;
using namespace grav;

constexpr int EN = NBKD_EWALD_N;      // intervals per axis over [0, 1/2]
constexpr int NN = EN + 1;            // nodes per axis
constexpr size_t TAB_NODES = (size_t)NN * NN * NN;

// ------------------------------------------------------------------ the table
// psi(x) = sum_n erfc(a|x-n|)/|x-n| + (1/pi) sum_{h != 0} exp(-pi^2 h^2/a^2)/h^2 cos(2 pi h.x)
//          - pi/a^2,   C_phi = psi - 1/|x|,   C_a = -grad psi - x/|x|^3  (a = ALPHA)
constexpr double ALPHA = 2.0;
// real space: erfc(ALPHA * RCUT) = 2e-13; the images beyond it, a density of
// one per unit volume, sum to 4 pi int r erfc(ALPHA r) dr < 1e-12
constexpr double RCUT = 2.6;
constexpr int NLO = -2, NHI = 3; // images with |x - n| < RCUT for x in [0, 1/2]
constexpr int NIMG = NHI - NLO + 1;
// reciprocal space: exp(-pi^2 h^2 / ALPHA^2) = 7e-18 at h^2 = 16
constexpr int HMAX = 4, H2MAX = 16;

struct EwaldHost {
    std::vector<float> tab; // TAB_NODES * 4
    // per axis node i: the offsets x_i - n and their squares
    double off[NN][NIMG], off2[NN][NIMG];
    // cos / sin (2 pi h x_i), h = 0 .. HMAX
    double cs[HMAX + 1][NN], sn[HMAX + 1][NN];
    // the reciprocal terms with h >= 0 per axis: mirror images folded in
    struct HTerm {
        int hx, hy, hz;
        double wphi, wx, wy, wz;
    };
    std::vector<HTerm> hs;

    void row(int i, int j) {
        const double pi = 3.14159265358979323846;
        const double g0 = 2.0 * ALPHA / std::sqrt(pi);
        for (int k = 0; k < NN; ++k) {
            double phi = -pi / (ALPHA * ALPHA), fx = 0.0, fy = 0.0, fz = 0.0;
            for (int a = 0; a < NIMG; ++a) {
                for (int b = 0; b < NIMG; ++b) {
                    const double rxy = off2[i][a] + off2[j][b];
                    if (rxy >= RCUT * RCUT) continue;
                    for (int c = 0; c < NIMG; ++c) {
                        const double r2 = rxy + off2[k][c];
                        if (r2 >= RCUT * RCUT) continue;
                        const bool self = a == -NLO && b == -NLO && c == -NLO;
                        if (r2 == 0.0) {
                            // (only the node at the origin, n = 0): the limit of
                            // erfc(a r)/r - 1/r; no force
                            phi -= g0;
                            continue;
                        }
                        const double r = std::sqrt(r2);
                        const double g = g0 * std::exp(-ALPHA * ALPHA * r2);
                        // n = 0 carries the nearest image's -1/r and -x/r^3
                        const double e = self ? -std::erf(ALPHA * r) : std::erfc(ALPHA * r);
                        const double w = (e + g * r) / (r2 * r);
                        phi += e / r;
                        fx += w * off[i][a];
                        fy += w * off[j][b];
                        fz += w * off[k][c];
                    }
                }
            }
            for (const HTerm &h : hs) {
                const double cx = cs[h.hx][i], cy = cs[h.hy][j], cz = cs[h.hz][k];
                phi += h.wphi * ((cx * cy) * cz);
                fx += h.wx * ((sn[h.hx][i] * cy) * cz);
                fy += h.wy * ((cx * sn[h.hy][j]) * cz);
                fz += h.wz * ((cx * cy) * sn[h.hz][k]);
            }
            // component a is odd in axis a: exactly 0 on the plane x_a = 0
            float *o = tab.data() + 4 * (((size_t)i * NN + j) * NN + k);
            o[0] = (float)phi;
            o[1] = i == 0 ? 0.0f : (float)fx;
            o[2] = j == 0 ? 0.0f : (float)fy;
            o[3] = k == 0 ? 0.0f : (float)fz;
        }
    }

    void build(int workers) {
        const double pi = 3.14159265358979323846;
        tab.resize(TAB_NODES * 4);
        for (int i = 0; i < NN; ++i) {
            const double x = (double)i / (2.0 * EN);
            for (int a = 0; a < NIMG; ++a) {
                off[i][a] = x - (double)(NLO + a);
                off2[i][a] = off[i][a] * off[i][a];
            }
            for (int h = 0; h <= HMAX; ++h) {
                cs[h][i] = std::cos(2.0 * pi * h * x);
                sn[h][i] = std::sin(2.0 * pi * h * x);
            }
            // (x = 1/2: the sines of the integer multiples of pi are exactly 0)
            if (i == EN)
                for (int h = 0; h <= HMAX; ++h) sn[h][i] = 0.0;
        }
        for (int hx = 0; hx <= HMAX; ++hx)
            for (int hy = 0; hy <= HMAX; ++hy)
                for (int hz = 0; hz <= HMAX; ++hz) {
                    const int h2 = hx * hx + hy * hy + hz * hz;
                    if (h2 == 0 || h2 > H2MAX) continue;
                    const double mult = (hx ? 2.0 : 1.0) * (hy ? 2.0 : 1.0) * (hz ? 2.0 : 1.0);
                    const double e = mult * std::exp(-pi * pi * h2 / (ALPHA * ALPHA)) / h2;
                    hs.push_back(HTerm{hx, hy, hz, e / pi, 2.0 * e * hx, 2.0 * e * hy, 2.0 * e * hz});
                }
        std::atomic<int> next{0};
        auto work = [&] {
            for (int r; (r = next.fetch_add(1)) < NN * NN;) row(r / NN, r % NN);
        };
        std::vector<std::thread> th;
        for (int w = 1; w < workers; ++w) th.emplace_back(work);
        work();
        for (std::thread &t : th) t.join();
        // the limit at the origin, as nbkd.h states it
        tab[0] = -2.8372975f;
    }
};

const std::vector<float> &ewald_host() {
    static const EwaldHost *h = [] {
        EwaldHost *e = new EwaldHost();
        e->build(std::max(1, std::min(host_workers(), 16)));
        return e;
    }();
    return h->tab;
}

// one copy per device, uploaded on first use and kept for the process
constexpr int MAX_DEV = 64;
std::mutex g_tab_mu;
const float4 *g_tab_dev[MAX_DEV] = {};

// ------------------------------------------------------------------ the walk
// the image of d nearest to 0 among d, fl(d - L), fl(d + L): ties to the
// earlier (group.hip's nearest_image)
__device__ __forceinline__ float wrap_image(float d, float L) {
    const float dm = d - L, dp = d + L;
    float r = d;
    if (fabsf(dm) < fabsf(r)) r = dm;
    if (fabsf(dp) < fabsf(r)) r = dp;
    return r;
}

// a table node as one 16-B vector (a plain float4 is loaded as 12 + 4 bytes:
// C_phi and C_a go to different sums)
typedef float node4 __attribute__((ext_vector_type(4)));

struct EwaldArgs {
    const node4 *__restrict__ tab;
    float L, sc, iL, iL2;
};

// a + f*(b - a) per channel
__device__ __forceinline__ node4 lerp4(const node4 a, const node4 b, float f) {
    return a + f * (b - a);
}

// one term: the Newtonian part of the nearest image, then the correction.  The
// cell index is clamped before the conversion, so every corner lies inside the
// table whatever d holds (a padding point: d2 = inf, which adds nothing).
__device__ __forceinline__ void ewald_term(const EwaldArgs &E, float mu, float dx, float dy,
                                           float dz, float d2, float eps2, float &phi, float &ax,
                                           float &ay, float &az) {
    grav_term(mu, dx, dy, dz, d2, eps2, phi, ax, ay, az);
    const float tx = fabsf(dx) * E.sc, ty = fabsf(dy) * E.sc, tz = fabsf(dz) * E.sc;
    const int ix = (int)fminf(tx, (float)(EN - 1));
    const int iy = (int)fminf(ty, (float)(EN - 1));
    const int iz = (int)fminf(tz, (float)(EN - 1));
    const float fx = tx - (float)ix, fy = ty - (float)iy, fz = tz - (float)iz;
    const node4 *c = E.tab + ((ix * NN + iy) * NN + iz);
    const node4 c000 = c[0], c100 = c[NN * NN];
    const node4 c010 = c[NN], c110 = c[NN * NN + NN];
    const node4 c001 = c[1], c101 = c[NN * NN + 1];
    const node4 c011 = c[NN + 1], c111 = c[NN * NN + NN + 1];
    // along x, then y, then z
    const node4 v00 = lerp4(c000, c100, fx), v10 = lerp4(c010, c110, fx);
    const node4 v01 = lerp4(c001, c101, fx), v11 = lerp4(c011, c111, fx);
    const node4 w0 = lerp4(v00, v10, fy), w1 = lerp4(v01, v11, fy);
    const node4 C = lerp4(w0, w1, fz);
    const float cx = dx < 0.0f ? -C.y : C.y;
    const float cy = dy < 0.0f ? -C.z : C.z;
    const float cz = dz < 0.0f ? -C.w : C.w;
    const float mp = mu * E.iL, ma = mu * E.iL2;
    const bool on = !(d2 == 0.0f) && d2 <= FLT_MAX;
    phi = on ? phi - mp * C.x : phi;
    ax = on ? ax + ma * cx : ax;
    ay = on ? ay + ma * cy : ay;
    az = on ? az + ma * cz : az;
}

__global__ void __launch_bounds__(TB, 4)
gravity_ewald_walk_kernel(DevTree t, const GravRec *__restrict__ rec, const float *__restrict__ q,
                          const uint32_t *__restrict__ order, uint32_t m,
                          const float *__restrict__ mt, float th2, float eps2, EwaldArgs E,
                          float *__restrict__ out_phi, float *__restrict__ out_acc) {
    __shared__ GravLds Wl[WPB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    GravLds &W = Wl[wave];
    const uint32_t gq = (xcd_block(blockIdx.x, gridDim.x) * WPB + wave) * 64u + lane;
    // (packet.hpp packet_query written out: through the helper the compares
    // come out in another order and the walk ran 0.85 % slower,
    // profiles/r12a_radius_helpers_ab.txt)
    const bool valid = gq < m;
    const uint32_t qo0 = valid ? order[gq] : 0u;
    const float qx = valid ? q[3 * (size_t)qo0] : 0.0f;
    const float qy = valid ? q[3 * (size_t)qo0 + 1] : 0.0f;
    const float qz = valid ? q[3 * (size_t)qo0 + 2] : 0.0f;
    const float L = E.L;
    // a query outside [0, L]^3 (or NaN) takes no part in the walk
    const bool inside = valid && qx >= 0.0f && qx <= L && qy >= 0.0f && qy <= L && qz >= 0.0f &&
                        qz <= L;
    const cnode_ptr cnodes = (cnode_ptr)t.nodes;
    const crec_ptr crec = (crec_ptr)rec;
    const bool open_all = !(th2 > 0.0f); // theta = 0: the direct sum
    float phi = 0.0f, ax = 0.0f, ay = 0.0f, az = 0.0f;
    // the wave stack: lane sp holds a pushed right child and the two halves
    // of the mask it was pushed with
    uint32_t sk_node = 0, sk_lo = 0, sk_hi = 0;
    int sp = 0;
    uint32_t node = 0;
    uint64_t mask = __ballot(inside); // the lanes that want the subtree of `node`
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
            const float dx = wrap_image(r.cx - qx, L), dy = wrap_image(r.cy - qy, L),
                        dz = wrap_image(r.cz - qz, L);
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            const bool ok = in && !open_all && r.s2 <= th2 * d2;
            if (ok) ewald_term(E, r.M, dx, dy, dz, d2, eps2, phi, ax, ay, az);
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
                    // (a padding point has mass 0 and d2 = inf: it adds nothing)
#pragma unroll 2
                    for (uint32_t u = 0; u < cn; ++u) {
                        const float4 a = W.p4[u];
                        const float mu = W.m[u];
                        const float dx = wrap_image(a.x - qx, L), dy = wrap_image(a.y - qy, L),
                                    dz = wrap_image(a.z - qz, L);
                        const float d2 = (dx * dx + dy * dy) + dz * dz;
                        ewald_term(E, mu, dx, dy, dz, d2, eps2, phi, ax, ay, az);
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
        if (!inside) phi = ax = ay = az = __builtin_nanf("");
        if (out_phi) out_phi[qo] = phi;
        if (out_acc) {
            out_acc[3 * (size_t)qo] = ax;
            out_acc[3 * (size_t)qo + 1] = ay;
            out_acc[3 * (size_t)qo + 2] = az;
        }
    }
}

} // namespace

const float *ewald_table_host() { return ewald_host().data(); }

nbkd_status ewald_table_device(int device, const void **out) {
    if (device < 0 || device >= MAX_DEV) {
        set_error("nbkd_gravity_ewald: device index out of range");
        return NBKD_EINVAL;
    }
    std::lock_guard<std::mutex> lk(g_tab_mu);
    if (!g_tab_dev[device]) {
        const std::vector<float> &h = ewald_host();
        void *p = nullptr;
        NBKD_HIP(malloc_or_release(&p, h.size() * 4));
        const hipError_t e = hipMemcpy(p, h.data(), h.size() * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(p);
            return hip_fail(e, "hipMemcpy (the Ewald table)");
        }
        g_tab_dev[device] = (const float4 *)p;
    }
    *out = g_tab_dev[device];
    return NBKD_OK;
}

void launch_gravity_ewald_walk(const Tree &t, const void *rec, const void *table, const float *q,
                               const uint32_t *order, uint32_t m, const float *mt, float th2,
                               float eps2, float *out_phi, float *out_acc, hipStream_t s) {
    if (m == 0) return;
    const unsigned blocks = (unsigned)((m + TB - 1) / TB);
    EwaldArgs E;
    E.tab = (const node4 *)table;
    E.L = t.box;
    E.iL = 1.0f / t.box;
    E.sc = (float)(2 * EN) * E.iL;
    E.iL2 = E.iL * E.iL;
    gravity_ewald_walk_kernel<<<blocks, TB, 0, s>>>(view(t), (const GravRec *)rec, q, order, m, mt,
                                                    th2, eps2, E, out_phi, out_acc);
}

} // namespace nbkd
