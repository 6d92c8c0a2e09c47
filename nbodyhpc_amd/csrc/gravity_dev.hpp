// Device pieces shared by the two gravity walks (gravity.hip: nbkd_gravity,
// gravity_ewald.hip: nbkd_gravity_ewald): the per-wave LDS staging area, the
// node record the moments pass writes, and the Newtonian term.
#pragma once

#include "internal.hpp"
#include "metric.hpp"
#include "packet.hpp"

namespace nbkd {
namespace grav {

constexpr int TB = 256;
constexpr int WPB = TB / 64;
using dev::CHUNK;

// 64 * 20 bytes per wave
struct alignas(16) GravLds {
    float4 p4[CHUNK]; // the staged points: x, y, z, id bits (Tree::p4)
    float m[CHUNK];   // their masses (mt)
};

// a node's monopole and the squared diagonal of its tight box
struct GravRec {
    float M, cx, cy, cz, s2, pad0, pad1, pad2;
};
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) GravRec *crec_ptr;
#else
typedef const GravRec *crec_ptr;
#endif

// one term: mass mu at offset d (d2 = |d|^2 as the caller summed it); d2 == 0
// (the query itself, a coincident point) adds nothing
__device__ __forceinline__ void grav_term(float mu, float dx, float dy, float dz, float d2,
                                          float eps2, float &phi, float &ax, float &ay,
                                          float &az) {
    const float r2 = d2 + eps2;
    const float inv = 1.0f / sqrtf(r2);
    const float w = mu * ((inv * inv) * inv);
    const bool on = !(d2 == 0.0f);
    phi = on ? phi - mu * inv : phi;
    ax = on ? ax + w * dx : ax;
    ay = on ? ay + w * dy : ay;
    az = on ? az + w * dz : az;
}

} // namespace grav
} // namespace nbkd
