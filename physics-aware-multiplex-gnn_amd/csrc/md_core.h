// Device helpers shared by the molecular-dynamics kernels (md.hip, md_npt.hip): the wavefront sum, the counter-based generator,
// the finiteness test, a free atom at the velocities that belong to its position, and the flag check of the entry points.
// Every statement here is what md.hip held before md_npt.hip existed: the kernels that include it compute what they computed.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct Normals {
    double x, y, z;
};
// Philox4x32-10 (Salmon et al., SC 2011) on the counter (i, step, stream, 0) under the key (k0, k1), then Box-Muller on
// u_j = (x_j + 0.5) 2^-32, which lies inside (0, 1): the logarithm is finite.  cos / sin of 2 pi u are taken as cospi / sinpi of 2 u.
__device__ __forceinline__ Normals normals(uint32_t k0, uint32_t k1, uint32_t i, uint32_t step, uint32_t stream) {
    uint32_t c0 = i, c1 = step, c2 = stream, c3 = 0u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0, c1 = l1, c2 = h0 ^ c3 ^ k1, c3 = l0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    const double s = 1.0 / 4294967296.0;
    const double u0 = ((double)c0 + 0.5) * s, u1 = ((double)c1 + 0.5) * s, u2 = ((double)c2 + 0.5) * s, u3 = ((double)c3 + 0.5) * s;
    const double r0 = sqrt(-2.0 * log(u0)), r1 = sqrt(-2.0 * log(u2));
    Normals t;
    t.x = r0 * cospi(2.0 * u1), t.y = r0 * sinpi(2.0 * u1), t.z = r1 * cospi(2.0 * u3);
    return t;
}

__host__ __device__ inline bool finite(double v) { return v >= -1.79769313486231570815e+308 && v <= 1.79769313486231570815e+308; }

struct Atom {
    double ax, ay, az, vx, vy, vz, m;             // a = f / m, f = -dE/dpos
};
// a free atom at the velocities that belong to pos: v_n = v + kick_in (dt / 2) f / m (both passes call the same statements)
__device__ __forceinline__ Atom load_atom(const float* __restrict__ vel, const float* __restrict__ dpos,
                                          const float* __restrict__ mass, int64_t a, bool kick_in, double h) {
    Atom t;
    t.m = mass ? (double)mass[a] : 1.0;
    t.ax = -(double)dpos[3 * a] / t.m, t.ay = -(double)dpos[3 * a + 1] / t.m, t.az = -(double)dpos[3 * a + 2] / t.m;
    t.vx = (double)vel[3 * a], t.vy = (double)vel[3 * a + 1], t.vz = (double)vel[3 * a + 2];
    if (kick_in) t.vx = t.vx + h * t.ax, t.vy = t.vy + h * t.ay, t.vz = t.vz + h * t.az;
    return t;
}

inline bool flag(int32_t v) { return v == 0 || v == 1; }

}  // namespace
