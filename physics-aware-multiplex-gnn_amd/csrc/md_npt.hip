// Constant-pressure molecular dynamics: one BAOAB step (md.hip) with the stochastic cell rescaling barostat (Bernetti & Bussi,
// J. Chem. Phys. 153, 114107, 2020), isotropic, for every graph of a batch in one launch -- pamnet_md_npt_step_f32
// (include/pamnet_hip.h states the rule).  The barostat is first order: its state per graph is eps = ln(V / V0) alone.
//
// The form of md_step_kernel: one workgroup of 256 threads per graph g, the threads striding over the atoms gptr[g] .. gptr[g + 1]
// (kept inside [0, n]), in two passes -- the sums, then the stores; what the second pass needs is recomputed, not kept, the
// normals included.  Every thread reads the same four wavefront partials from LDS and adds them in the same order, and forms the
// determinant of cell0, the pressure, the volume change d and the scale s = exp(d / 3) from them alike: nothing is broadcast and
// every exit is uniform.  Sums in a fixed order, no atomics.  Arithmetic in fp64 from the fp32 inputs, one rounding at each fp32
// store.  Thread 0 writes the graph's scalars after every thread has read them (the reads stand before the barrier of pass 1).
//
// A graph whose cell_dof is 0 has no barostat: `baro` is false, and the statements that remain are those of md_step_kernel, so
// that its results are bitwise those of pamnet_md_step_f32.  The flag is uniform over the workgroup.
#include "md_core.h"

namespace {

struct NptRule {
    double dt, kT, gamma, pressure, rate;
    int32_t kick_in, advance;
};

__global__ __launch_bounds__(256) void md_npt_step_kernel(
    float* __restrict__ pos, float* __restrict__ vel, const float* __restrict__ dpos, const float* __restrict__ dstrain,
    const float* __restrict__ mass, const uint8_t* __restrict__ fixed, const int32_t* __restrict__ gptr, int64_t n,
    const float* __restrict__ cell0_g, float* __restrict__ cell_g, double* __restrict__ eps_g,
    const uint8_t* __restrict__ cell_dof, const int64_t* __restrict__ seed_g, int32_t* __restrict__ steps_g,
    int32_t* __restrict__ status_g, double* __restrict__ ke_g, double* __restrict__ pint_g, double* __restrict__ vol_g,
    const double* __restrict__ dt_g, const double* __restrict__ kT_g, const double* __restrict__ gamma_g,
    const double* __restrict__ pressure_g, const double* __restrict__ rate_g, NptRule rule) {
    __shared__ double part[4][2];
    const int64_t g = blockIdx.x;
    if (status_g[g] != 0) return;                                 // step 1 (uniform over the workgroup): g is left alone
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t lo = gptr[g], hi = gptr[g + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n ? n : hi;
    const double dt = dt_g ? dt_g[g] : rule.dt, kT = kT_g ? kT_g[g] : rule.kT, gamma = gamma_g ? gamma_g[g] : rule.gamma;
    const double h = 0.5 * dt;
    const uint32_t step = (uint32_t)steps_g[g];                   // (read by every thread before thread 0 writes it, below)
    const bool baro = !(cell_dof && cell_dof[g] == 0);            // (uniform)
    const bool thermostat = gamma > 0.0;
    const bool cell_noise = baro && kT > 0.0;
    const uint64_t seed = (thermostat || cell_noise) ? (uint64_t)seed_g[g] : 0u;
    const int32_t kick_in = rule.kick_in, advance = rule.advance;

    // what belongs to the barostat is read here, before the barrier: eps by every thread, written by thread 0 at the end
    double eps = 0.0, V = 0.0, trW = 0.0, p0 = 0.0, rate = 0.0;
    if (baro) {
        const float* c = cell0_g + 9 * g;
        const double c0 = (double)c[0], c1 = (double)c[1], c2 = (double)c[2], c3 = (double)c[3], c4 = (double)c[4],
                     c5 = (double)c[5], c6 = (double)c[6], c7 = (double)c[7], c8 = (double)c[8];
        const double det = c0 * (c4 * c8 - c5 * c7) - c1 * (c3 * c8 - c5 * c6) + c2 * (c3 * c7 - c4 * c6);
        eps = eps_g[g];
        V = fabs(det) * exp(eps);
        trW = ((double)dstrain[9 * g] + (double)dstrain[9 * g + 4]) + (double)dstrain[9 * g + 8];
        p0 = pressure_g ? pressure_g[g] : rule.pressure;
        rate = rate_g ? rate_g[g] : rule.rate;
    }

    // ---- pass 1: steps 2 and 3
    double F2 = 0.0, KE = 0.0;
    for (int64_t a = lo + tid; a < hi; a += 256) {
        if (fixed && fixed[a]) continue;
        const Atom t = load_atom(vel, dpos, mass, a, kick_in != 0, h);
        const double fx = (double)dpos[3 * a], fy = (double)dpos[3 * a + 1], fz = (double)dpos[3 * a + 2];
        F2 += fx * fx + fy * fy + fz * fz;
        KE += t.m * (t.vx * t.vx + t.vy * t.vy + t.vz * t.vz);
    }
    F2 = wave_sum(F2), KE = wave_sum(KE);
    if (lane == 0) part[wave][0] = F2, part[wave][1] = KE;
    __syncthreads();
    F2 = (part[0][0] + part[1][0]) + (part[2][0] + part[3][0]);
    KE = 0.5 * ((part[0][1] + part[1][1]) + (part[2][1] + part[3][1]));
    bool failed = !finite(F2) || !finite(KE);
    double d = 0.0;
    if (baro) {                                                   // steps 3 and 4: the pressure and the volume change
        failed = failed || !finite(trW) || !finite(V) || V == 0.0;
        const double pint = (2.0 * KE - trW) / (3.0 * V);
        if (tid == 0) pint_g[g] = pint, vol_g[g] = V;
        if (!failed) {
            d = -rate * (p0 - pint) * dt;
            if (cell_noise) {
                const Normals xi = normals((uint32_t)seed, (uint32_t)(seed >> 32), 0u, step, 2u);
                d = d + sqrt(2.0 * kT * rate * dt / V) * xi.x;
            }
            failed = !finite(d);
        }
    }
    if (tid == 0) {
        ke_g[g] = KE;
        if (failed) status_g[g] = 2;
    }
    if (failed) return;                                           // (uniform)

    // ---- pass 2: the stores (an atom is read and written by one thread only)
    if (!advance) {                                               // step 4: the closing half kick alone
        if (!kick_in) return;                                     // (v_n is v: nothing to store)
        for (int64_t a = lo + tid; a < hi; a += 256) {
            if (fixed && fixed[a]) continue;
            const Atom t = load_atom(vel, dpos, mass, a, true, h);
            vel[3 * a] = (float)t.vx, vel[3 * a + 1] = (float)t.vy, vel[3 * a + 2] = (float)t.vz;
        }
        return;
    }
    const double c1 = thermostat ? exp(-gamma * dt) : 1.0;
    const double c2 = thermostat ? sqrt(1.0 - c1 * c1) : 0.0;
    const double s = exp(d / 3.0);                                // (1 where there is no barostat, and not used there)
    for (int64_t a = lo + tid; a < hi; a += 256) {                // step 5
        if (fixed && fixed[a]) {
            if (baro) {                                           // a fixed atom keeps its fractional coordinates
                pos[3 * a] = (float)(s * (double)pos[3 * a]);
                pos[3 * a + 1] = (float)(s * (double)pos[3 * a + 1]);
                pos[3 * a + 2] = (float)(s * (double)pos[3 * a + 2]);
            }
            continue;
        }
        const Atom t = load_atom(vel, dpos, mass, a, kick_in != 0, h);
        const double v1x = t.vx + h * t.ax, v1y = t.vy + h * t.ay, v1z = t.vz + h * t.az;
        double v2x = v1x, v2y = v1y, v2z = v1z;
        if (thermostat) {
            const Normals xi = normals((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)(a - lo), step, 0u);
            const double sg = c2 * sqrt(kT / t.m);
            v2x = c1 * v1x + sg * xi.x, v2y = c1 * v1y + sg * xi.y, v2z = c1 * v1z + sg * xi.z;
        }
        double x = (double)pos[3 * a] + h * (v1x + v2x);
        double y = (double)pos[3 * a + 1] + h * (v1y + v2y);
        double z = (double)pos[3 * a + 2] + h * (v1z + v2z);
        if (baro) {
            x = s * x, y = s * y, z = s * z;
            v2x = v2x / s, v2y = v2y / s, v2z = v2z / s;
        }
        pos[3 * a] = (float)x, pos[3 * a + 1] = (float)y, pos[3 * a + 2] = (float)z;
        vel[3 * a] = (float)v2x, vel[3 * a + 1] = (float)v2y, vel[3 * a + 2] = (float)v2z;
    }
    if (tid == 0) {
        if (baro) {                                               // always from cell0: the cell accumulates no fp32 rounding
            const double eps_new = eps + d;
            const double sc = exp(eps_new / 3.0);
            eps_g[g] = eps_new;
#pragma unroll
            for (int i = 0; i < 9; ++i) cell_g[9 * g + i] = (float)((double)cell0_g[9 * g + i] * sc);
        }
        steps_g[g] += 1;                                          // step 6
    }
}

}  // namespace

extern "C" int pamnet_md_npt_step_f32(float* pos, float* vel, const float* dpos, const float* dstrain, const float* mass,
                                      const uint8_t* fixed, const int32_t* gptr, int64_t n, int64_t n_graphs,
                                      const float* cell0, float* cell, double* eps, const uint8_t* cell_dof, const int64_t* seed,
                                      int32_t* steps, int32_t* status, double* ke, double* pint, double* vol,
                                      const double* dt_g, const double* kT_g, const double* gamma_g, const double* pressure_g,
                                      const double* rate_g, double dt, double kT, double gamma, double pressure, double rate,
                                      int32_t kick_in, int32_t advance, pamnet_stream_t stream) {
    if (n < 0 || n_graphs < 0 || n_graphs > 0x7fffffff || !flag(kick_in) || !flag(advance)) return PAMNET_EINVAL;
    if (!dt_g && !(dt > 0.0 && finite(dt))) return PAMNET_EINVAL;
    if (!kT_g && !(kT >= 0.0 && finite(kT))) return PAMNET_EINVAL;
    if (!gamma_g && !(gamma >= 0.0 && finite(gamma))) return PAMNET_EINVAL;
    if (!pressure_g && !finite(pressure)) return PAMNET_EINVAL;
    if (!rate_g && !(rate > 0.0 && finite(rate))) return PAMNET_EINVAL;
    if (!pos || !vel || !dpos || !dstrain || !gptr || !cell0 || !cell || !eps || !steps || !status || !ke || !pint || !vol)
        return PAMNET_ENULL;
    if (!seed && (gamma_g || kT_g || gamma != 0.0 || kT != 0.0)) return PAMNET_ENULL;
    if (n_graphs == 0) return PAMNET_OK;
    const NptRule rule{dt, kT, gamma, pressure, rate, kick_in, advance};
    hipLaunchKernelGGL(md_npt_step_kernel, dim3((unsigned)n_graphs), dim3(256), 0, as_stream(stream), pos, vel, dpos, dstrain, mass,
                       fixed, gptr, n, cell0, cell, eps, cell_dof, seed, steps, status, ke, pint, vol, dt_g, kT_g, gamma_g,
                       pressure_g, rate_g, rule);
    PAMNET_LAUNCH_CHECK();
    return PAMNET_OK;
}
