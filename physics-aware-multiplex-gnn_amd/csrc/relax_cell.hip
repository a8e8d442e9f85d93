// Cell relaxation: one FIRE step over the atoms and the cell of every graph of a batch in one launch --
// pamnet_fire_cell_step_f32 (include/pamnet_hip.h states the rule, the convention and the order of its updates).
//
// The form of the fixed-cell step kernel (relax.hip): one workgroup of 256 threads per graph g, the threads striding over the
// atoms gptr[g] .. gptr[g + 1] (kept inside [0, n]), in three passes:
//   1. F2 = sum |g_a|^2, P = sum g_a.v~_a, V2 = sum |v~_a|^2 and max |f|^2 over the free atoms (g_a = f_a F^T);
//   2. max |dt v~_a|^2 of the new generalised velocities, which are recomputed, not kept;
//   3. the stores of vel and pos, fixed atoms included (they follow the cell).
// The 3 x 3 algebra -- the cell C = cell0 F, F^-1, the stress S, the cell force, the new cell velocity, F_new and D = F^-1 F_new
// -- is formed by every thread from the same inputs and the same four wavefront partials, so the graph's decision is taken by
// every thread alike: nothing is broadcast, every exit is uniform.  Sums in a fixed order (a thread's atoms ascending, the
// wavefront butterfly, the four wavefronts in wave order, then the nine cell terms in index order), no atomics.  Arithmetic in
// fp64 from the fp32 inputs, one rounding at each fp32 store.  Thread 0 writes the graph's state after every thread has read it.
//
// A graph whose cell_dof is 0 takes fixed_cell_step below: the statements of the fixed-cell kernel, so that its results are
// bitwise those of pamnet_fire_step_f32.  The branch is uniform over the workgroup.
#include "common.h"

namespace {

struct FireRule {
    double fmax_tol, dt_max, max_step, f_inc, f_dec, a0, f_a;
    int32_t n_min;
};
struct CellRule {
    double smax_tol, pressure;
    int32_t hydrostatic;
};

constexpr double DBL_MAX_ = 1.79769313486231570815e+308;

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
// v <- c_v v + c_f f, then v <- v + dt f (passes 2 and 3 call the same statements)
__device__ __forceinline__ void new_velocity(Atom& t, double c_v, double c_f, double dt) {
    t.vx = (c_v * t.vx + c_f * t.fx) + dt * t.fx;
    t.vy = (c_v * t.vy + c_f * t.fy) + dt * t.fy;
    t.vz = (c_v * t.vz + c_f * t.fz) + dt * t.fz;
}
// the generalised force of a free atom in place of its force: g = f F^T
__device__ __forceinline__ Atom load_generalised(const float* __restrict__ vel, const float* __restrict__ dpos, int64_t a,
                                                 const double (&F)[9]) {
    Atom t = load_atom(vel, dpos, a);
    const double gx = t.fx * F[0] + t.fy * F[1] + t.fz * F[2];
    const double gy = t.fx * F[3] + t.fy * F[4] + t.fz * F[5];
    const double gz = t.fx * F[6] + t.fy * F[7] + t.fz * F[8];
    t.fx = gx, t.fy = gy, t.fz = gz;
    return t;
}

// ---- 3 x 3, row-major, fully unrolled (registers only)
__device__ __forceinline__ double det3(const double (&m)[9]) {
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
__device__ __forceinline__ void inv3(const double (&m)[9], double (&r)[9]) {
    const double id = 1.0 / det3(m);
    r[0] = (m[4] * m[8] - m[5] * m[7]) * id, r[1] = (m[2] * m[7] - m[1] * m[8]) * id, r[2] = (m[1] * m[5] - m[2] * m[4]) * id;
    r[3] = (m[5] * m[6] - m[3] * m[8]) * id, r[4] = (m[0] * m[8] - m[2] * m[6]) * id, r[5] = (m[2] * m[3] - m[0] * m[5]) * id;
    r[6] = (m[3] * m[7] - m[4] * m[6]) * id, r[7] = (m[1] * m[6] - m[0] * m[7]) * id, r[8] = (m[0] * m[4] - m[1] * m[3]) * id;
}
__device__ __forceinline__ void mul3(const double (&a)[9], const double (&b)[9], double (&c)[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

struct GraphState {
    double* __restrict__ dt;
    double* __restrict__ a;
    int32_t* __restrict__ n_pos;
    int32_t* __restrict__ steps;
    int32_t* __restrict__ status;
    float* __restrict__ fmax;
};

// The graph's decision (step 3 of the fixed-cell rule, step 4 of this one): the new n_pos, dt and a first, then the mixing
// coefficients from the new a.
__device__ __forceinline__ void fire_decision(const FireRule& rule, double F2, double P, double V2, double& dt, double& mix,
                                              int32_t& n_pos, double& c_v, double& c_f) {
    c_v = 1.0, c_f = 0.0;
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
}

// A graph that keeps its cell: the fixed-cell step, statement for statement (relax.hip), so that the results are bitwise those
// of pamnet_fire_step_f32.  Called by every thread of the workgroup (it holds barriers).
__device__ __forceinline__ void fixed_cell_step(float* __restrict__ pos, float* __restrict__ vel, const float* __restrict__ dpos,
                                                const uint8_t* __restrict__ fixed, int64_t lo, int64_t hi, int64_t g,
                                                const GraphState& st, double tol, const FireRule& rule, double (&part)[4][4],
                                                double (&part_dr)[4]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double dt = st.dt[g], mix = st.a[g];
    int32_t n_pos = st.n_pos[g];
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
    const bool failed = !(F2 <= DBL_MAX_);
    const double fm = failed ? sqrt(F2) : sqrt(fm2);
    const bool converged = !failed && fm < tol;
    if (failed || converged) {
        if (tid == 0) {
            st.fmax[g] = (float)fm;
            st.status[g] = failed ? 2 : 1;
        }
        return;                                                   // (uniform)
    }
    double c_v, c_f;
    fire_decision(rule, F2, P, V2, dt, mix, n_pos, c_v, c_f);

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
        st.fmax[g] = (float)fm;
        st.dt[g] = dt;
        st.a[g] = mix;
        st.n_pos[g] = n_pos;
        st.steps[g] += 1;
    }
}

__global__ __launch_bounds__(256) void fire_cell_kernel(
    float* __restrict__ pos, float* __restrict__ vel, const float* __restrict__ dpos, const float* __restrict__ dstrain,
    const uint8_t* __restrict__ fixed, const int32_t* __restrict__ gptr, int64_t n, const float* __restrict__ cell0_g,
    float* __restrict__ cell_g, double* __restrict__ F_g, double* __restrict__ vcell_g, const uint8_t* __restrict__ cell_dof,
    const double* __restrict__ cell_factor, GraphState st, float* __restrict__ smax_g, const float* __restrict__ fmax_tol_g,
    const float* __restrict__ smax_tol_g, const double* __restrict__ pressure_g, FireRule rule, CellRule crule) {
    __shared__ double part[4][4];
    __shared__ double part_dr[4];
    const int64_t g = blockIdx.x;
    if (st.status[g] != 0) return;                                // step 0 (uniform over the workgroup): g is left alone
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t lo = gptr[g], hi = gptr[g + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n ? n : hi;
    const double tol = fmax_tol_g ? (double)fmax_tol_g[g] : rule.fmax_tol;
    if (cell_dof && cell_dof[g] == 0) {                           // (uniform)
        fixed_cell_step(pos, vel, dpos, fixed, lo, hi, g, st, tol, rule, part, part_dr);
        return;
    }
    double dt = st.dt[g], mix = st.a[g];                          // (read by every thread before thread 0 writes them, below)
    int32_t n_pos = st.n_pos[g];
    const double stol = smax_tol_g ? (double)smax_tol_g[g] : crule.smax_tol;
    const double p = pressure_g ? pressure_g[g] : crule.pressure;
    const double L = cell_factor[g];

    // ---- step 1, by every thread: F, F^-1, the volume, the stress and the cell force
    double F[9], Fi[9], S[9], vc[9];
    double V;
    {
        double c0[9], C[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) F[i] = F_g[9 * g + i], vc[i] = vcell_g[9 * g + i], c0[i] = (double)cell0_g[9 * g + i];
        mul3(c0, F, C);
        V = fabs(det3(C));
        inv3(F, Fi);
        double W[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) W[i] = (double)dstrain[9 * g + i];
        const double pV = p * V;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) S[3 * i + j] = 0.5 * (W[3 * i + j] + W[3 * j + i]) + (i == j ? pV : 0.0);
        if (crule.hydrostatic) {
            const double tr = (S[0] + S[4] + S[8]) / 3.0;
#pragma unroll
            for (int i = 0; i < 9; ++i) S[i] = (i % 4 == 0) ? tr : 0.0;
        }
    }
    double sabs = 0.0, snan = 0.0;                                // a NaN-propagating maximum (fmax alone drops a NaN): the graph
#pragma unroll                                                    // then fails on F2 below and reports sm = NaN beside fmax
    for (int i = 0; i < 9; ++i) {
        sabs = fmax(sabs, fabs(S[i]));
        snan = S[i] != S[i] ? S[i] : snan;
    }
    const double sm = (snan != snan ? snan : sabs) / V;
    double gc[9];                                                 // g_c = -(F^-T S) / L
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) gc[3 * i + j] = -(Fi[i] * S[j] + Fi[3 + i] * S[3 + j] + Fi[6 + i] * S[6 + j]) / L;

    // ---- pass 1: steps 2 - 4 over the free atoms
    double F2 = 0.0, P = 0.0, V2 = 0.0, fm2 = 0.0;
    for (int64_t a = lo + tid; a < hi; a += 256) {
        if (fixed && fixed[a]) continue;
        Atom t = load_atom(vel, dpos, a);
        fm2 = fmax(fm2, t.fx * t.fx + t.fy * t.fy + t.fz * t.fz);
        t = load_generalised(vel, dpos, a, F);
        F2 += t.fx * t.fx + t.fy * t.fy + t.fz * t.fz;
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
#pragma unroll
    for (int i = 0; i < 9; ++i) F2 += gc[i] * gc[i], P += gc[i] * vc[i], V2 += vc[i] * vc[i];
    // F2 is NaN or +inf where a force, the virial, F or cell0 is not finite or F is singular; V is checked beside it
    const bool failed = !(F2 <= DBL_MAX_) || !(V <= DBL_MAX_) || V == 0.0;
    const double fm = failed ? sqrt(F2) : sqrt(fm2);
    const bool converged = !failed && fm < tol && sm < stol;
    if (failed || converged) {
        if (tid == 0) {
            st.fmax[g] = (float)fm;
            smax_g[g] = (float)sm;
            st.status[g] = failed ? 2 : 1;
        }
        return;                                                   // (uniform)
    }
    double c_v, c_f;
    fire_decision(rule, F2, P, V2, dt, mix, n_pos, c_v, c_f);

    // ---- step 5 for the cell, pass 2: the largest row of step 6
#pragma unroll
    for (int i = 0; i < 9; ++i) vc[i] = (c_v * vc[i] + c_f * gc[i]) + dt * gc[i];
    double dr2 = 0.0;
    for (int64_t a = lo + tid; a < hi; a += 256) {
        if (fixed && fixed[a]) continue;
        Atom t = load_generalised(vel, dpos, a, F);
        new_velocity(t, c_v, c_f, dt);
        const double dx = dt * t.vx, dy = dt * t.vy, dz = dt * t.vz;
        dr2 = fmax(dr2, dx * dx + dy * dy + dz * dz);
    }
    dr2 = wave_max(dr2);
    if (lane == 0) part_dr[wave] = dr2;
    __syncthreads();
    dr2 = fmax(fmax(part_dr[0], part_dr[1]), fmax(part_dr[2], part_dr[3]));
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double dx = dt * vc[3 * i], dy = dt * vc[3 * i + 1], dz = dt * vc[3 * i + 2];
        dr2 = fmax(dr2, dx * dx + dy * dy + dz * dz);
    }
    const double dr = sqrt(dr2);
    const double s = dr > rule.max_step ? rule.max_step / dr : 1.0;

    // ---- steps 7 and 8
    double Fn[9], D[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) Fn[i] = F[i] + s * (dt * vc[i]) / L;
    const double dn = det3(Fn);
    if (!(dn > 0.0 && dn <= DBL_MAX_)) {                          // (uniform) the step would invert or flatten the cell
        if (tid == 0) {
            st.fmax[g] = (float)fm;
            smax_g[g] = (float)sm;
            st.status[g] = 2;
        }
        return;
    }
    mul3(Fi, Fn, D);

    // ---- pass 3: the stores (an atom is read and written by one thread only)
    for (int64_t a = lo + tid; a < hi; a += 256) {
        const double x = (double)pos[3 * a], y = (double)pos[3 * a + 1], z = (double)pos[3 * a + 2];
        double nx = x * D[0] + y * D[3] + z * D[6];
        double ny = x * D[1] + y * D[4] + z * D[7];
        double nz = x * D[2] + y * D[5] + z * D[8];
        if (!(fixed && fixed[a])) {
            Atom t = load_generalised(vel, dpos, a, F);
            new_velocity(t, c_v, c_f, dt);
            vel[3 * a] = (float)t.vx, vel[3 * a + 1] = (float)t.vy, vel[3 * a + 2] = (float)t.vz;
            const double ux = s * (dt * t.vx), uy = s * (dt * t.vy), uz = s * (dt * t.vz);
            nx += ux * Fn[0] + uy * Fn[3] + uz * Fn[6];
            ny += ux * Fn[1] + uy * Fn[4] + uz * Fn[7];
            nz += ux * Fn[2] + uy * Fn[5] + uz * Fn[8];
        }
        pos[3 * a] = (float)nx, pos[3 * a + 1] = (float)ny, pos[3 * a + 2] = (float)nz;
    }
    if (tid == 0) {
        double c0[9], C[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) c0[i] = (double)cell0_g[9 * g + i];
        mul3(c0, Fn, C);
#pragma unroll
        for (int i = 0; i < 9; ++i) cell_g[9 * g + i] = (float)C[i], F_g[9 * g + i] = Fn[i], vcell_g[9 * g + i] = vc[i];
        st.fmax[g] = (float)fm;
        smax_g[g] = (float)sm;
        st.dt[g] = dt;
        st.a[g] = mix;
        st.n_pos[g] = n_pos;
        st.steps[g] += 1;
    }
}

inline bool positive(double v) { return v > 0.0 && v <= DBL_MAX_; }
inline bool is_finite(double v) { return v >= -DBL_MAX_ && v <= DBL_MAX_; }

}  // namespace

extern "C" int pamnet_fire_cell_step_f32(float* pos, float* vel, const float* dpos, const float* dstrain, const uint8_t* fixed,
                                         const int32_t* gptr, int64_t n, int64_t n_graphs, const float* cell0, float* cell,
                                         double* F, double* vcell, const uint8_t* cell_dof, const double* cell_factor,
                                         double* dt, double* a, int32_t* n_pos, int32_t* steps, int32_t* status, float* fmax,
                                         float* smax, const float* fmax_tol_g, const float* smax_tol_g,
                                         const double* pressure_g, double fmax_tol, double smax_tol, double pressure,
                                         int32_t hydrostatic, double dt_max, double max_step, int32_t n_min, double f_inc,
                                         double f_dec, double a0, double f_a, pamnet_stream_t stream) {
    if (n < 0 || n_graphs < 0 || n_graphs > 0x7fffffff || n_min < 0 || (hydrostatic != 0 && hydrostatic != 1))
        return PAMNET_EINVAL;
    if (!positive(dt_max) || !positive(max_step) || !positive(f_inc) || !positive(f_dec) || !positive(a0) || !positive(f_a) ||
        fmax_tol != fmax_tol || smax_tol != smax_tol || !is_finite(pressure))
        return PAMNET_EINVAL;
    if (!pos || !vel || !dpos || !dstrain || !gptr || !cell0 || !cell || !F || !vcell || !cell_factor || !dt || !a || !n_pos ||
        !steps || !status || !fmax || !smax)
        return PAMNET_ENULL;
    if (n_graphs == 0) return PAMNET_OK;
    const FireRule rule{fmax_tol, dt_max, max_step, f_inc, f_dec, a0, f_a, n_min};
    const CellRule crule{smax_tol, pressure, hydrostatic};
    const GraphState st{dt, a, n_pos, steps, status, fmax};
    hipLaunchKernelGGL(fire_cell_kernel, dim3((unsigned)n_graphs), dim3(256), 0, as_stream(stream), pos, vel, dpos, dstrain, fixed,
                       gptr, n, cell0, cell, F, vcell, cell_dof, cell_factor, st, smax, fmax_tol_g, smax_tol_g, pressure_g, rule,
                       crule);
    PAMNET_LAUNCH_CHECK();
    return PAMNET_OK;
}
