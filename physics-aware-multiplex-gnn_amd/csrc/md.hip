// Molecular dynamics: one BAOAB step (Leimkuhler & Matthews, J. Chem. Phys. 138, 174102, 2013; gamma = 0: velocity Verlet) for
// every graph of a batch in one launch -- pamnet_md_step_f32 -- and Maxwell-Boltzmann velocities -- pamnet_md_init_velocities_f32
// (include/pamnet_hip.h states both rules and the generator).
//
// Both kernels take the form of fire_step_kernel (relax.hip): one workgroup of 256 threads per graph g, the threads striding over
// the atoms gptr[g] .. gptr[g + 1] (kept inside [0, n]); every thread reads the same four wavefront partials from LDS and adds
// them in the same order, so what the graph decides (failed or not, the centre-of-mass velocity, the scale) is formed by every
// thread alike: nothing is broadcast and no thread diverges from its workgroup.  Sums in a fixed order -- a thread's atoms
// ascending, the wavefront butterfly, the four wavefronts in wave order -- and no atomics.  Arithmetic in fp64 from the fp32
// inputs, one rounding at each store of pos and vel.  What a later pass needs is recomputed, not kept, the normals included (a
// graph may have any number of atoms).
//
// The noise is Philox4x32-10 keyed by the graph's seed and counted by (the atom's offset in its graph, the graph's step counter,
// the stream): it depends on nothing else, so a graph's trajectory is bitwise the same alone or in any batch, from run to run.
#include "md_core.h"                              // wave_sum, normals, finite, Atom / load_atom, flag

namespace {

__global__ __launch_bounds__(256) void md_step_kernel(float* __restrict__ pos, float* __restrict__ vel,
                                                      const float* __restrict__ dpos, const float* __restrict__ mass,
                                                      const uint8_t* __restrict__ fixed, const int32_t* __restrict__ gptr,
                                                      int64_t n, const int64_t* __restrict__ seed_g,
                                                      int32_t* __restrict__ steps_g, int32_t* __restrict__ status_g,
                                                      double* __restrict__ ke_g, const double* __restrict__ dt_g,
                                                      const double* __restrict__ kT_g, const double* __restrict__ gamma_g,
                                                      double dt_all, double kT_all, double gamma_all, int32_t kick_in,
                                                      int32_t advance) {
    __shared__ double part[4][2];
    const int64_t g = blockIdx.x;
    if (status_g[g] != 0) return;                                 // step 1 (uniform over the workgroup): g is left alone
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t lo = gptr[g], hi = gptr[g + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n ? n : hi;
    const double dt = dt_g ? dt_g[g] : dt_all, kT = kT_g ? kT_g[g] : kT_all, gamma = gamma_g ? gamma_g[g] : gamma_all;
    const double h = 0.5 * dt;
    const uint32_t step = (uint32_t)steps_g[g];                   // (read by every thread before thread 0 writes it, below)
    const bool thermostat = gamma > 0.0;
    const uint64_t seed = thermostat ? (uint64_t)seed_g[g] : 0u;

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
    const bool failed = !finite(F2) || !finite(KE);
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
    for (int64_t a = lo + tid; a < hi; a += 256) {                // step 5
        if (fixed && fixed[a]) continue;
        const Atom t = load_atom(vel, dpos, mass, a, kick_in != 0, h);
        const double v1x = t.vx + h * t.ax, v1y = t.vy + h * t.ay, v1z = t.vz + h * t.az;
        double v2x = v1x, v2y = v1y, v2z = v1z;
        if (thermostat) {
            const Normals xi = normals((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)(a - lo), step, 0u);
            const double s = c2 * sqrt(kT / t.m);
            v2x = c1 * v1x + s * xi.x, v2y = c1 * v1y + s * xi.y, v2z = c1 * v1z + s * xi.z;
        }
        pos[3 * a] = (float)((double)pos[3 * a] + h * (v1x + v2x));
        pos[3 * a + 1] = (float)((double)pos[3 * a + 1] + h * (v1y + v2y));
        pos[3 * a + 2] = (float)((double)pos[3 * a + 2] + h * (v1z + v2z));
        vel[3 * a] = (float)v2x, vel[3 * a + 1] = (float)v2y, vel[3 * a + 2] = (float)v2z;
    }
    if (tid == 0) steps_g[g] += 1;                                // step 6
}

struct Drawn {
    double vx, vy, vz, m;
};
// v = sqrt(kT / m) xi of a free atom (the three passes call the same statements)
__device__ __forceinline__ Drawn draw_atom(const float* __restrict__ mass, int64_t a, int64_t lo, uint64_t seed, double kT) {
    Drawn t;
    t.m = mass ? (double)mass[a] : 1.0;
    const Normals xi = normals((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)(a - lo), 0u, 1u);
    const double s = sqrt(kT / t.m);
    t.vx = s * xi.x, t.vy = s * xi.y, t.vz = s * xi.z;
    return t;
}

__global__ __launch_bounds__(256) void md_init_velocities_kernel(float* __restrict__ vel, const float* __restrict__ mass,
                                                                 const uint8_t* __restrict__ fixed,
                                                                 const int32_t* __restrict__ gptr, int64_t n,
                                                                 const int64_t* __restrict__ seed_g,
                                                                 const double* __restrict__ kT_g, double kT_all,
                                                                 int32_t remove_com, int32_t rescale, double* __restrict__ ke_g) {
    __shared__ double part[4][5];
    __shared__ double part_ke[4];
    const int64_t g = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t lo = gptr[g], hi = gptr[g + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n ? n : hi;
    const double kT = kT_g ? kT_g[g] : kT_all;
    const uint64_t seed = (uint64_t)seed_g[g];

    // ---- pass 1: the mass, the momentum and the number of free atoms
    double M = 0.0, Px = 0.0, Py = 0.0, Pz = 0.0, nf = 0.0;
    for (int64_t a = lo + tid; a < hi; a += 256) {
        if (fixed && fixed[a]) continue;
        const Drawn t = draw_atom(mass, a, lo, seed, kT);
        M += t.m, Px += t.m * t.vx, Py += t.m * t.vy, Pz += t.m * t.vz, nf += 1.0;
    }
    M = wave_sum(M), Px = wave_sum(Px), Py = wave_sum(Py), Pz = wave_sum(Pz), nf = wave_sum(nf);
    if (lane == 0) part[wave][0] = M, part[wave][1] = Px, part[wave][2] = Py, part[wave][3] = Pz, part[wave][4] = nf;
    __syncthreads();
    M = (part[0][0] + part[1][0]) + (part[2][0] + part[3][0]);
    Px = (part[0][1] + part[1][1]) + (part[2][1] + part[3][1]);
    Py = (part[0][2] + part[1][2]) + (part[2][2] + part[3][2]);
    Pz = (part[0][3] + part[1][3]) + (part[2][3] + part[3][3]);
    nf = (part[0][4] + part[1][4]) + (part[2][4] + part[3][4]);
    const bool com = remove_com && nf > 0.0;
    const double ux = com ? Px / M : 0.0, uy = com ? Py / M : 0.0, uz = com ? Pz / M : 0.0;

    // ---- pass 2: the kinetic energy without the centre-of-mass motion
    double KE = 0.0;
    for (int64_t a = lo + tid; a < hi; a += 256) {
        if (fixed && fixed[a]) continue;
        const Drawn t = draw_atom(mass, a, lo, seed, kT);
        const double x = t.vx - ux, y = t.vy - uy, z = t.vz - uz;
        KE += t.m * (x * x + y * y + z * z);
    }
    KE = wave_sum(KE);
    if (lane == 0) part_ke[wave] = KE;
    __syncthreads();
    KE = 0.5 * ((part_ke[0] + part_ke[1]) + (part_ke[2] + part_ke[3]));
    const double dof = 3.0 * nf - (remove_com ? 3.0 : 0.0);
    const double s = (rescale && dof > 0.0 && KE > 0.0) ? sqrt(dof * kT / (2.0 * KE)) : 1.0;

    // ---- pass 3: the stores
    for (int64_t a = lo + tid; a < hi; a += 256) {
        if (fixed && fixed[a]) continue;
        const Drawn t = draw_atom(mass, a, lo, seed, kT);
        vel[3 * a] = (float)(s * (t.vx - ux)), vel[3 * a + 1] = (float)(s * (t.vy - uy)), vel[3 * a + 2] = (float)(s * (t.vz - uz));
    }
    if (tid == 0) ke_g[g] = (s * s) * KE;
}

}  // namespace

extern "C" int pamnet_md_step_f32(float* pos, float* vel, const float* dpos, const float* mass, const uint8_t* fixed,
                                  const int32_t* gptr, int64_t n, int64_t n_graphs, const int64_t* seed, int32_t* steps,
                                  int32_t* status, double* ke, const double* dt_g, const double* kT_g, const double* gamma_g,
                                  double dt, double kT, double gamma, int32_t kick_in, int32_t advance, pamnet_stream_t stream) {
    if (n < 0 || n_graphs < 0 || n_graphs > 0x7fffffff || !flag(kick_in) || !flag(advance)) return PAMNET_EINVAL;
    if (!dt_g && !(dt > 0.0 && finite(dt))) return PAMNET_EINVAL;
    if (!kT_g && !(kT >= 0.0 && finite(kT))) return PAMNET_EINVAL;
    if (!gamma_g && !(gamma >= 0.0 && finite(gamma))) return PAMNET_EINVAL;
    if (!pos || !vel || !dpos || !gptr || !steps || !status || !ke) return PAMNET_ENULL;
    if (!seed && (gamma_g || gamma != 0.0)) return PAMNET_ENULL;
    if (n_graphs == 0) return PAMNET_OK;
    hipLaunchKernelGGL(md_step_kernel, dim3((unsigned)n_graphs), dim3(256), 0, as_stream(stream), pos, vel, dpos, mass, fixed, gptr,
                       n, seed, steps, status, ke, dt_g, kT_g, gamma_g, dt, kT, gamma, kick_in, advance);
    PAMNET_LAUNCH_CHECK();
    return PAMNET_OK;
}

extern "C" int pamnet_md_init_velocities_f32(float* vel, const float* mass, const uint8_t* fixed, const int32_t* gptr, int64_t n,
                                             int64_t n_graphs, const int64_t* seed, const double* kT_g, double kT,
                                             int32_t remove_com, int32_t rescale, double* ke, pamnet_stream_t stream) {
    if (n < 0 || n_graphs < 0 || n_graphs > 0x7fffffff || !flag(remove_com) || !flag(rescale)) return PAMNET_EINVAL;
    if (!kT_g && !(kT >= 0.0 && finite(kT))) return PAMNET_EINVAL;
    if (!vel || !gptr || !seed || !ke) return PAMNET_ENULL;
    if (n_graphs == 0) return PAMNET_OK;
    hipLaunchKernelGGL(md_init_velocities_kernel, dim3((unsigned)n_graphs), dim3(256), 0, as_stream(stream), vel, mass, fixed, gptr,
                       n, seed, kT_g, kT, remove_com, rescale, ke);
    PAMNET_LAUNCH_CHECK();
    return PAMNET_OK;
}
