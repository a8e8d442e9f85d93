// Structure relaxation: one FIRE step (Bitzek et al., Phys. Rev. Lett. 97, 170201, 2006) for every graph of a batch in one
// launch -- pamnet_fire_step_f32 (include/pamnet_hip.h states the rule and the order of its updates).
//
// One workgroup of 256 threads per graph g, the threads striding over the atoms gptr[g] .. gptr[g + 1] (kept inside [0, n]) as
// virial_reduce_kernel (forces.hip) does, in three passes:
//   1. F2 = sum |f|^2, P = sum f.v, V2 = sum |v|^2 and max |f|^2;
//   2. max |dr|^2 of the new velocities, which are recomputed, not kept (a graph may have any number of atoms);
//   3. the stores of vel and pos.
// Every thread reads the same four wavefront partials from LDS and adds them in the same order, so the graph's decision
// (converged / failed / uphill / downhill, the new dt and a) is formed by every thread alike: nothing is broadcast and no
// thread diverges from its workgroup.  Sums in a fixed order -- a thread's atoms in ascending order, the wavefront butterfly,
// the four wavefronts in wave order -- and no atomics: a graph's result is bitwise the same from run to run, and the same
// whatever else the batch holds (the order depends on the atom's offset in its graph only).  Arithmetic in fp64 from the fp32
// inputs, one rounding at each store of vel and pos.
#include "common.h"

namespace {

struct FireRule {
    double fmax_tol, dt_max, max_step, f_inc, f_dec, a0, f_a;
    int32_t n_min;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {           // (operands >= 0 or NaN; NaN never reaches a use, see F2)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

struct Atom {
    double fx, fy, fz, vx, vy, vz;
};
// f = -dE/dpos and v of a free atom
__device__ __forceinline__ Atom load_atom(const float* __restrict__ vel, const float* __restrict__ dpos, int64_t a) {
    Atom t;
    t.fx = -(double)dpos[3 * a], t.fy = -(double)dpos[3 * a + 1], t.fz = -(double)dpos[3 * a + 2];
    t.vx = (double)vel[3 * a], t.vy = (double)vel[3 * a + 1], t.vz = (double)vel[3 * a + 2];
    return t;
}
// steps 3 and 4 for one atom: v <- c_v v + c_f f, then v <- v + dt f (passes 2 and 3 call the same statements)
__device__ __forceinline__ void new_velocity(Atom& t, double c_v, double c_f, double dt) {
    t.vx = (c_v * t.vx + c_f * t.fx) + dt * t.fx;
    t.vy = (c_v * t.vy + c_f * t.fy) + dt * t.fy;
    t.vz = (c_v * t.vz + c_f * t.fz) + dt * t.fz;
}

__global__ __launch_bounds__(256) void fire_step_kernel(float* __restrict__ pos, float* __restrict__ vel,
                                                        const float* __restrict__ dpos, const uint8_t* __restrict__ fixed,
                                                        const int32_t* __restrict__ gptr, int64_t n, double* __restrict__ dt_g,
                                                        double* __restrict__ a_g, int32_t* __restrict__ n_pos_g,
                                                        int32_t* __restrict__ steps_g, int32_t* __restrict__ status_g,
                                                        float* __restrict__ fmax_g, const float* __restrict__ fmax_tol_g,
                                                        FireRule rule) {
    __shared__ double part[4][4];
    __shared__ double part_dr[4];
    const int64_t g = blockIdx.x;
    if (status_g[g] != 0) return;                                 // step 1 (uniform over the workgroup): g is left alone
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t lo = gptr[g], hi = gptr[g + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n ? n : hi;
    double dt = dt_g[g], mix = a_g[g];                            // (read by every thread before thread 0 writes them, below)
    int32_t n_pos = n_pos_g[g];
    const double tol = fmax_tol_g ? (double)fmax_tol_g[g] : rule.fmax_tol;

    // ---- pass 1: step 2 and the sums of step 3
    double F2 = 0.0, P = 0.0, V2 = 0.0, fm2 = 0.0;
    for (int64_t a = lo + tid; a < hi; a += 256) {
        if (fixed && fixed[a]) continue;
        const Atom t = load_atom(vel, dpos, a);
        const double f2 = t.fx * t.fx + t.fy * t.fy + t.fz * t.fz;
        F2 += f2;
        fm2 = fmax(fm2, f2);
        P += t.fx * t.vx + t.fy * t.vy + t.fz * t.vz;
        V2 += t.vx * t.vx + t.vy * t.vy + t.vz * t.vz;
    }
    F2 = wave_sum(F2), P = wave_sum(P), V2 = wave_sum(V2), fm2 = wave_max(fm2);
    if (lane == 0) part[wave][0] = F2, part[wave][1] = P, part[wave][2] = V2, part[wave][3] = fm2;
    __syncthreads();
    F2 = (part[0][0] + part[1][0]) + (part[2][0] + part[3][0]);
    P = (part[0][1] + part[1][1]) + (part[2][1] + part[3][1]);
    V2 = (part[0][2] + part[1][2]) + (part[2][2] + part[3][2]);
    fm2 = fmax(fmax(part[0][3], part[1][3]), fmax(part[2][3], part[3][3]));
    // F2 is a sum of squares: NaN where a component is NaN, +inf where one is infinite and none NaN -- which is also what a
    // NaN-propagating maximum of |f| gives, so the failed graph reports sqrt(F2)
    const bool failed = !(F2 <= 1.79769313486231570815e+308);
    const double fm = failed ? sqrt(F2) : sqrt(fm2);
    const bool converged = !failed && fm < tol;
    if (failed || converged) {
        if (tid == 0) {
            fmax_g[g] = (float)fm;
            status_g[g] = failed ? 2 : 1;
        }
        return;                                                   // (uniform)
    }

    // ---- the graph's decision (step 3): the new n_pos, dt and a first, then the mixing with the new a
    double c_v = 1.0, c_f = 0.0;
    if (V2 != 0.0) {
        if (P > 0.0) {
            n_pos += 1;
            if (n_pos > rule.n_min) {
                dt = fmin(dt * rule.f_inc, rule.dt_max);
                mix *= rule.f_a;
            }
            c_v = 1.0 - mix;
            c_f = F2 > 0.0 ? mix * sqrt(V2 / F2) : 0.0;
        } else {
            c_v = 0.0;
            mix = rule.a0;
            dt *= rule.f_dec;
            n_pos = 0;
        }
    }

    // ---- pass 2: the largest displacement of step 5
    double dr2 = 0.0;
    for (int64_t a = lo + tid; a < hi; a += 256) {
        if (fixed && fixed[a]) continue;
        Atom t = load_atom(vel, dpos, a);
        new_velocity(t, c_v, c_f, dt);
        const double dx = dt * t.vx, dy = dt * t.vy, dz = dt * t.vz;
        dr2 = fmax(dr2, dx * dx + dy * dy + dz * dz);
    }
    dr2 = wave_max(dr2);
    if (lane == 0) part_dr[wave] = dr2;
    __syncthreads();
    const double dr = sqrt(fmax(fmax(part_dr[0], part_dr[1]), fmax(part_dr[2], part_dr[3])));
    const double s = dr > rule.max_step ? rule.max_step / dr : 1.0;

    // ---- pass 3: the stores (an atom is read and written by one thread only)
    for (int64_t a = lo + tid; a < hi; a += 256) {
        if (fixed && fixed[a]) continue;
        Atom t = load_atom(vel, dpos, a);
        new_velocity(t, c_v, c_f, dt);
        vel[3 * a] = (float)t.vx, vel[3 * a + 1] = (float)t.vy, vel[3 * a + 2] = (float)t.vz;
        pos[3 * a] = (float)((double)pos[3 * a] + s * (dt * t.vx));
        pos[3 * a + 1] = (float)((double)pos[3 * a + 1] + s * (dt * t.vy));
        pos[3 * a + 2] = (float)((double)pos[3 * a + 2] + s * (dt * t.vz));
    }
    if (tid == 0) {
        fmax_g[g] = (float)fm;
        dt_g[g] = dt;
        a_g[g] = mix;
        n_pos_g[g] = n_pos;
        steps_g[g] += 1;
    }
}

inline bool positive(double v) { return v > 0.0 && v <= 1.79769313486231570815e+308; }

}  // namespace

extern "C" int pamnet_fire_step_f32(float* pos, float* vel, const float* dpos, const uint8_t* fixed, const int32_t* gptr,
                                    int64_t n, int64_t n_graphs, double* dt, double* a, int32_t* n_pos, int32_t* steps,
                                    int32_t* status, float* fmax, const float* fmax_tol_g, double fmax_tol, double dt_max,
                                    double max_step, int32_t n_min, double f_inc, double f_dec, double a0, double f_a,
                                    pamnet_stream_t stream) {
    if (n < 0 || n_graphs < 0 || n_graphs > 0x7fffffff || n_min < 0) return PAMNET_EINVAL;
    if (!positive(dt_max) || !positive(max_step) || !positive(f_inc) || !positive(f_dec) || !positive(a0) || !positive(f_a) ||
        fmax_tol != fmax_tol)
        return PAMNET_EINVAL;
    if (!pos || !vel || !dpos || !gptr || !dt || !a || !n_pos || !steps || !status || !fmax) return PAMNET_ENULL;
    if (n_graphs == 0) return PAMNET_OK;
    const FireRule rule{fmax_tol, dt_max, max_step, f_inc, f_dec, a0, f_a, n_min};
    hipLaunchKernelGGL(fire_step_kernel, dim3((unsigned)n_graphs), dim3(256), 0, as_stream(stream), pos, vel, dpos, fixed, gptr, n,
                       dt, a, n_pos, steps, status, fmax, fmax_tol_g, rule);
    PAMNET_LAUNCH_CHECK();
    return PAMNET_OK;
}
