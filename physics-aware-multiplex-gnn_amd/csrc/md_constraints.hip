// Constrained molecular dynamics: one g-BAOAB step (Leimkuhler & Matthews, Proc. R. Soc. A 472, 20160138, 2016; one geodesic
// sub-step per half drift) under distance constraints for every graph of a batch in one launch --
// pamnet_md_constrained_step_f32 -- and the projection of positions / velocities onto the constraints --
// pamnet_md_project_constraints_f32 (include/pamnet_hip.h states both rules).
//
// The form of md_step_kernel (md.hip): one workgroup of 256 threads per graph g; every thread reads the same four wavefront
// partials from LDS and forms the same decisions from them, so every exit and every loop count is uniform over the workgroup.
// Sums in a fixed order, no atomics, fp64 arithmetic, one rounding at each store of pos and vel.
//
// A constrained graph works on the fp64 workspace (x0, x, v: three blocks of 3 n doubles): an atom's rows are written by the
// thread that owns the atom (a = lo + tid + 256 k) between the solves, and by the thread that owns a constraint inside a solve.
// The constraints of a graph arrive sorted by colour; inside a colour no two share an atom, so the threads stride over a colour's
// constraints and a barrier separates the colours: a sweep is the Gauss-Seidel sweep in the order (colour, position), whatever
// the schedule.  The workspace is exchanged between threads across __syncthreads() and is therefore not __restrict__.  pos and
// vel are read once at the start and stored once at the end, by the owner of the atom.
//
// A graph without constraints takes the statements of md_step_kernel, repeated here: its results are bitwise those of
// pamnet_md_step_f32.
#include "md_core.h"

namespace {

struct StepRule {
    double dt, kT, gamma;
    int32_t kick_in, advance;
};

struct Cons {                                     // the constraints of the batch, sorted by (graph, colour)
    const int32_t* i;
    const int32_t* j;
    const double* d;
    const int32_t* gcol;                          // [G + 1]: the colours of a graph
    const int32_t* colptr;                        // [K + 1]: the constraints of a colour
    int64_t n_cons;
    double* work;                                 // [9 n]: x0, x, v
    int32_t* sweeps;
    double tol;
    int32_t max_sweeps;
};

struct Graph {                                    // what a solve needs of its graph (the same in every thread)
    int64_t lo, hi;
    int32_t k0, k1;
    const float* mass;
    const uint8_t* fixed;
    int tid, lane, wave;
};

enum { CONVERGED = 0, NOT_YET = 1, BROKEN = 2 };

// w_a = 0 for a fixed atom, 1 / m_a otherwise
__device__ __forceinline__ double inv_mass(const Graph& q, int64_t a) {
    if (q.fixed && q.fixed[a]) return 0.0;
    return 1.0 / (q.mass ? (double)q.mass[a] : 1.0);
}

// The verdict of a sweep, the same in every thread: BROKEN if any constraint was, else NOT_YET if any was above tol.  Its barrier
// closes the sweep's last colour.  `flags` alternates with the sweep's parity, so the verdict barrier of the next sweep lies
// between a thread's reads here and the next write of the same row; the barrier that opens every solve (sweeps, below) keeps the
// last reads of one solve apart from the first write of the next.
__device__ __forceinline__ int sweep_verdict(bool not_yet, bool broken, int (*flags)[4], int parity, const Graph& q) {
    const bool wb = __ballot(broken) != 0, wn = __ballot(not_yet) != 0;
    if (q.lane == 0) flags[parity][q.wave] = wb ? BROKEN : (wn ? NOT_YET : CONVERGED);
    __syncthreads();
    const int a = flags[parity][0], b = flags[parity][1], c = flags[parity][2], d = flags[parity][3];
    const int ab = a > b ? a : b, cd = c > d ? c : d;
    return ab > cd ? ab : cd;
}

// One solve: Gauss-Seidel sweeps over the graph's constraints in the order (colour, position) until a sweep finds every error
// within tol (CONVERGED), one is broken, or max_sweeps have run.  body(i, j, d, not_yet, broken) measures and corrects one
// constraint whose rows lie inside the graph.  Self-contained: it opens with a barrier, which settles what the owners of the
// atoms wrote to the workspace and separates this solve's use of `flags` from the solve before, and it ends behind the barrier
// of its last verdict, so the workspace is settled when it returns.  Entered by the whole workgroup; every count is uniform.
// Returns true on convergence; `most` takes the sweeps run.
template <class Body>
__device__ __forceinline__ bool sweeps(const Cons& c, const Graph& q, int (*flags)[4], int& most, Body body) {
    int it = 0, verdict = NOT_YET;
    __syncthreads();
    while (it < c.max_sweeps) {
        bool not_yet = false, broken = false;
        for (int32_t k = q.k0; k < q.k1; ++k) {
            if (k != q.k0) __syncthreads();
            int64_t c0 = c.colptr[k], c1 = c.colptr[k + 1];
            c0 = c0 < 0 ? 0 : c0;
            c1 = c1 > c.n_cons ? c.n_cons : c1;
            for (int64_t e = c0 + q.tid; e < c1; e += 256) {
                const int64_t i = c.i[e], j = c.j[e];
                if (i < q.lo || i >= q.hi || j < q.lo || j >= q.hi) {          // (a row outside the graph: never touched)
                    broken = true;
                    continue;
                }
                body(i, j, c.d[e], not_yet, broken);
            }
        }
        verdict = sweep_verdict(not_yet, broken, flags, it & 1, q);
        ++it;
        if (verdict != NOT_YET) break;                            // (uniform)
    }
    most = it > most ? it : most;
    return verdict == CONVERGED;
}

// RATTLE_V: r = x_i - x_j, kappa = r.(v_i - v_j) / ((w_i + w_j) r.r), v_i -= w_i kappa r, v_j += w_j kappa r, swept until a sweep
// finds max_k |r.(v_i - v_j)| dt / d^2 <= tol (measured on each constraint as the sweep reaches it).
__device__ __forceinline__ bool rattle(const Cons& c, const Graph& q, const double* x, double* v, double dt, int (*flags)[4],
                                       int& most) {
    return sweeps(c, q, flags, most, [&](int64_t i, int64_t j, double d, bool& not_yet, bool& broken) {
        const double rx = x[3 * i] - x[3 * j], ry = x[3 * i + 1] - x[3 * j + 1], rz = x[3 * i + 2] - x[3 * j + 2];
        const double ux = v[3 * i] - v[3 * j], uy = v[3 * i + 1] - v[3 * j + 1], uz = v[3 * i + 2] - v[3 * j + 2];
        const double rv = rx * ux + ry * uy + rz * uz, rr = rx * rx + ry * ry + rz * rz;
        const double err = fabs(rv) * dt / (d * d);
        if (!(err <= c.tol)) not_yet = true;
        if (!finite(err)) {
            broken = true;
            return;
        }
        const double wi = inv_mass(q, i), wj = inv_mass(q, j);
        if (!(wi + wj > 0.0) || !(rr > 0.0)) return;
        const double kappa = rv / ((wi + wj) * rr);
        const double ki = wi * kappa, kj = wj * kappa;
        v[3 * i] -= ki * rx, v[3 * i + 1] -= ki * ry, v[3 * i + 2] -= ki * rz;
        v[3 * j] += kj * rx, v[3 * j + 1] += kj * ry, v[3 * j + 2] += kj * rz;
    });
}

// SHAKE: s = x_i - x_j, r0 = x0_i - x0_j, g = (s.s - d^2) / (2 (w_i + w_j) (s.r0)), x_i -= w_i g r0, x_j += w_j g r0, swept until a
// sweep finds max_k |s.s - d^2| / (2 d^2) <= tol.  s.r0 <= 0 or an error that is not finite breaks the solve.
__device__ __forceinline__ bool shake(const Cons& c, const Graph& q, const double* x0, double* x, int (*flags)[4], int& most) {
    return sweeps(c, q, flags, most, [&](int64_t i, int64_t j, double d, bool& not_yet, bool& broken) {
        const double sx = x[3 * i] - x[3 * j], sy = x[3 * i + 1] - x[3 * j + 1], sz = x[3 * i + 2] - x[3 * j + 2];
        const double rx = x0[3 * i] - x0[3 * j], ry = x0[3 * i + 1] - x0[3 * j + 1], rz = x0[3 * i + 2] - x0[3 * j + 2];
        const double diff = (sx * sx + sy * sy + sz * sz) - d * d, sr = sx * rx + sy * ry + sz * rz;
        const double err = fabs(diff) / (2.0 * (d * d));
        if (!(err <= c.tol)) not_yet = true;
        if (!finite(err) || !(sr > 0.0)) {
            broken = true;
            return;
        }
        const double wi = inv_mass(q, i), wj = inv_mass(q, j);
        if (!(wi + wj > 0.0)) return;
        const double gk = diff / (2.0 * (wi + wj) * sr);
        const double gi = wi * gk, gj = wj * gk;
        x[3 * i] -= gi * rx, x[3 * i + 1] -= gi * ry, x[3 * i + 2] -= gi * rz;
        x[3 * j] += gj * rx, x[3 * j + 1] += gj * ry, x[3 * j + 2] += gj * rz;
    });
}

// sum m |v|^2 over the free atoms, from the workspace, in the order of md_step_kernel; a barrier stands before the partials
// are written, so that no thread still reads the sum before
__device__ __forceinline__ double twice_kinetic(const Graph& q, const double* v, double (*part)[2]) {
    double KE = 0.0;
    for (int64_t a = q.lo + q.tid; a < q.hi; a += 256) {
        if (q.fixed && q.fixed[a]) continue;
        const double m = q.mass ? (double)q.mass[a] : 1.0;
        KE += m * (v[3 * a] * v[3 * a] + v[3 * a + 1] * v[3 * a + 1] + v[3 * a + 2] * v[3 * a + 2]);
    }
    KE = wave_sum(KE);
    __syncthreads();
    if (q.lane == 0) part[q.wave][1] = KE;
    __syncthreads();
    return (part[0][1] + part[1][1]) + (part[2][1] + part[3][1]);
}

// half drift with SHAKE: x0 = x, x += h v, the solve, v = (x - x0) / h.  The rows of v are written by the owners of the atoms
// last: the solve that follows (RATTLE_V, always) opens with the barrier that settles them.
__device__ __forceinline__ bool drift(const Cons& c, const Graph& q, double* x0, double* x, double* v, double h, int (*flags)[4],
                                      int& most) {
    for (int64_t a = q.lo + q.tid; a < q.hi; a += 256) {
        const bool fx = q.fixed && q.fixed[a];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double xa = x[3 * a + k];
            x0[3 * a + k] = xa;
            if (!fx) x[3 * a + k] = xa + h * v[3 * a + k];
        }
    }
    if (!shake(c, q, x0, x, flags, most)) return false;
    for (int64_t a = q.lo + q.tid; a < q.hi; a += 256) {
        if (q.fixed && q.fixed[a]) continue;
#pragma unroll
        for (int k = 0; k < 3; ++k) v[3 * a + k] = (x[3 * a + k] - x0[3 * a + k]) / h;
    }
    return true;
}

__global__ __launch_bounds__(256) void md_constrained_step_kernel(
    float* __restrict__ pos, float* __restrict__ vel, const float* __restrict__ dpos, const float* __restrict__ mass,
    const uint8_t* __restrict__ fixed, const int32_t* __restrict__ gptr, int64_t n, const int64_t* __restrict__ seed_g,
    int32_t* __restrict__ steps_g, int32_t* __restrict__ status_g, double* __restrict__ ke_g, const double* __restrict__ dt_g,
    const double* __restrict__ kT_g, const double* __restrict__ gamma_g, StepRule rule, Cons cons) {
    __shared__ double part[4][2];
    __shared__ int flags[2][4];
    const int64_t g = blockIdx.x;
    if (status_g[g] != 0) return;                                 // step 1 (uniform over the workgroup): g is left alone
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t lo = gptr[g], hi = gptr[g + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n ? n : hi;
    const double dt = dt_g ? dt_g[g] : rule.dt, kT = kT_g ? kT_g[g] : rule.kT, gamma = gamma_g ? gamma_g[g] : rule.gamma;
    const double h = 0.5 * dt;
    const uint32_t step = (uint32_t)steps_g[g];                   // (read by every thread before thread 0 writes it, below)
    const bool thermostat = gamma > 0.0;
    const uint64_t seed = thermostat ? (uint64_t)seed_g[g] : 0u;
    const int32_t kick_in = rule.kick_in, advance = rule.advance;
    const int32_t k0 = cons.gcol ? cons.gcol[g] : 0, k1 = cons.gcol ? cons.gcol[g + 1] : 0;

    if (k1 <= k0) {
        // ================= a graph without constraints: the statements of md_step_kernel (md.hip), bit for bit
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
            cons.sweeps[g] = 0;
            if (failed) status_g[g] = 2;
        }
        if (failed) return;                                       // (uniform)
        if (!advance) {
            if (!kick_in) return;
            for (int64_t a = lo + tid; a < hi; a += 256) {
                if (fixed && fixed[a]) continue;
                const Atom t = load_atom(vel, dpos, mass, a, true, h);
                vel[3 * a] = (float)t.vx, vel[3 * a + 1] = (float)t.vy, vel[3 * a + 2] = (float)t.vz;
            }
            return;
        }
        const double c1 = thermostat ? exp(-gamma * dt) : 1.0;
        const double c2 = thermostat ? sqrt(1.0 - c1 * c1) : 0.0;
        for (int64_t a = lo + tid; a < hi; a += 256) {
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
        if (tid == 0) steps_g[g] += 1;
        return;
    }

    // ================= a constrained graph: g-BAOAB on the workspace
    double* x0 = cons.work;
    double* x = cons.work + 3 * n;
    double* v = cons.work + 6 * n;
    const Graph q{lo, hi, k0, k1, mass, fixed, tid, lane, wave};
    int most = 0;

    // ---- the load: x = pos, v = v_n before its projection (0 for a fixed atom); F2 and the kinetic energy of the inputs
    double F2 = 0.0, KE = 0.0;
    for (int64_t a = lo + tid; a < hi; a += 256) {
        x[3 * a] = (double)pos[3 * a], x[3 * a + 1] = (double)pos[3 * a + 1], x[3 * a + 2] = (double)pos[3 * a + 2];
        if (fixed && fixed[a]) {
            v[3 * a] = 0.0, v[3 * a + 1] = 0.0, v[3 * a + 2] = 0.0;
            continue;
        }
        const Atom t = load_atom(vel, dpos, mass, a, kick_in != 0, h);
        const double fx = (double)dpos[3 * a], fy = (double)dpos[3 * a + 1], fz = (double)dpos[3 * a + 2];
        F2 += fx * fx + fy * fy + fz * fz;
        KE += t.m * (t.vx * t.vx + t.vy * t.vy + t.vz * t.vz);
        v[3 * a] = t.vx, v[3 * a + 1] = t.vy, v[3 * a + 2] = t.vz;
    }
    F2 = wave_sum(F2), KE = wave_sum(KE);
    if (lane == 0) part[wave][0] = F2, part[wave][1] = KE;
    __syncthreads();
    F2 = (part[0][0] + part[1][0]) + (part[2][0] + part[3][0]);
    KE = 0.5 * ((part[0][1] + part[1][1]) + (part[2][1] + part[3][1]));
    if (!finite(F2) || !finite(KE)) {                             // (uniform) inputs that are not finite: failed, as in md_step
        if (tid == 0) ke_g[g] = KE, status_g[g] = 2, cons.sweeps[g] = 0;
        return;
    }
    bool ok = true;
    if (kick_in) {                                                // the closing half kick changed v: RATTLE_V, and KE again
        ok = rattle(cons, q, x, v, dt, flags, most);
        if (ok) KE = 0.5 * twice_kinetic(q, v, part);
    }
    if (ok && !finite(KE)) {
        if (tid == 0) ke_g[g] = KE, status_g[g] = 2, cons.sweeps[g] = most;
        return;
    }
    if (ok && tid == 0) ke_g[g] = KE;
    if (ok && !advance) {
        if (kick_in)
            for (int64_t a = lo + tid; a < hi; a += 256) {
                if (fixed && fixed[a]) continue;
                vel[3 * a] = (float)v[3 * a], vel[3 * a + 1] = (float)v[3 * a + 1], vel[3 * a + 2] = (float)v[3 * a + 2];
            }
        if (tid == 0) cons.sweeps[g] = most;
        return;
    }
    if (ok) {                                                     // B: half kick, RATTLE_V
        for (int64_t a = lo + tid; a < hi; a += 256) {
            if (fixed && fixed[a]) continue;
            const double m = mass ? (double)mass[a] : 1.0;
            v[3 * a] = v[3 * a] + h * (-(double)dpos[3 * a] / m);
            v[3 * a + 1] = v[3 * a + 1] + h * (-(double)dpos[3 * a + 1] / m);
            v[3 * a + 2] = v[3 * a + 2] + h * (-(double)dpos[3 * a + 2] / m);
        }
        ok = rattle(cons, q, x, v, dt, flags, most);
    }
    if (ok) ok = drift(cons, q, x0, x, v, h, flags, most);        // A: half drift with SHAKE, RATTLE_V
    if (ok) ok = rattle(cons, q, x, v, dt, flags, most);
    if (ok && thermostat) {                                       // O: the noise of md_step (same key, counter and stream)
        const double c1 = exp(-gamma * dt);
        const double c2 = sqrt(1.0 - c1 * c1);
        for (int64_t a = lo + tid; a < hi; a += 256) {
            if (fixed && fixed[a]) continue;
            const double m = mass ? (double)mass[a] : 1.0;
            const Normals xi = normals((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)(a - lo), step, 0u);
            const double s = c2 * sqrt(kT / m);
            v[3 * a] = c1 * v[3 * a] + s * xi.x, v[3 * a + 1] = c1 * v[3 * a + 1] + s * xi.y, v[3 * a + 2] = c1 * v[3 * a + 2] + s * xi.z;
        }
        ok = rattle(cons, q, x, v, dt, flags, most);
    }
    if (ok) ok = drift(cons, q, x0, x, v, h, flags, most);        // A
    if (ok) ok = rattle(cons, q, x, v, dt, flags, most);
    if (!ok) {                                                    // (uniform) a solve did not converge: pos, vel, steps stay
        if (tid == 0) status_g[g] = 3, cons.sweeps[g] = most;
        return;
    }
    for (int64_t a = lo + tid; a < hi; a += 256) {                // the stores: one rounding each
        if (fixed && fixed[a]) continue;
        pos[3 * a] = (float)x[3 * a], pos[3 * a + 1] = (float)x[3 * a + 1], pos[3 * a + 2] = (float)x[3 * a + 2];
        vel[3 * a] = (float)v[3 * a], vel[3 * a + 1] = (float)v[3 * a + 1], vel[3 * a + 2] = (float)v[3 * a + 2];
    }
    if (tid == 0) steps_g[g] += 1, cons.sweeps[g] = most;
}

__global__ __launch_bounds__(256) void md_project_constraints_kernel(
    float* __restrict__ pos, float* __restrict__ vel, const float* __restrict__ mass, const uint8_t* __restrict__ fixed,
    const int32_t* __restrict__ gptr, int64_t n, int32_t* __restrict__ status_g, double* __restrict__ ke_g,
    const double* __restrict__ dt_g, double dt_all, int32_t do_pos, int32_t do_vel, Cons cons) {
    __shared__ double part[4][2];
    __shared__ int flags[2][4];
    const int64_t g = blockIdx.x;
    if (status_g[g] != 0) return;                                 // (uniform) g is left alone
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t lo = gptr[g], hi = gptr[g + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n ? n : hi;
    const double dt = do_vel ? (dt_g ? dt_g[g] : dt_all) : 0.0;
    const int32_t k0 = cons.gcol ? cons.gcol[g] : 0, k1 = cons.gcol ? cons.gcol[g + 1] : 0;
    const Graph q{lo, hi, k0, k1, mass, fixed, tid, lane, wave};
    int most = 0;
    if (k1 <= k0) {                                               // no constraints: nothing moves; ke of vel as it stands
        if (do_vel) {
            double KE = 0.0;
            for (int64_t a = lo + tid; a < hi; a += 256) {
                if (fixed && fixed[a]) continue;
                const double m = mass ? (double)mass[a] : 1.0;
                const double vx = (double)vel[3 * a], vy = (double)vel[3 * a + 1], vz = (double)vel[3 * a + 2];
                KE += m * (vx * vx + vy * vy + vz * vz);
            }
            KE = wave_sum(KE);
            if (lane == 0) part[wave][1] = KE;
            __syncthreads();
            KE = 0.5 * ((part[0][1] + part[1][1]) + (part[2][1] + part[3][1]));
            if (tid == 0) ke_g[g] = KE;
        }
        if (tid == 0) cons.sweeps[g] = 0;
        return;
    }
    double* x0 = cons.work;
    double* x = cons.work + 3 * n;
    double* v = cons.work + 6 * n;
    for (int64_t a = lo + tid; a < hi; a += 256) {
        const bool fx = fixed && fixed[a];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double xa = (double)pos[3 * a + k];
            x0[3 * a + k] = xa, x[3 * a + k] = xa;
            if (do_vel) v[3 * a + k] = fx ? 0.0 : (double)vel[3 * a + k];
        }
    }
    bool ok = true;                                               // (every solve opens with the barrier that settles the rows)
    if (do_pos) ok = shake(cons, q, x0, x, flags, most);
    if (ok && do_vel) ok = rattle(cons, q, x, v, dt, flags, most);
    if (!ok) {                                                    // (uniform) pos and vel stay
        if (tid == 0) status_g[g] = 3, cons.sweeps[g] = most;
        return;
    }
    double KE = 0.0;
    if (do_vel) KE = 0.5 * twice_kinetic(q, v, part);
    for (int64_t a = lo + tid; a < hi; a += 256) {
        if (fixed && fixed[a]) continue;
        if (do_pos) pos[3 * a] = (float)x[3 * a], pos[3 * a + 1] = (float)x[3 * a + 1], pos[3 * a + 2] = (float)x[3 * a + 2];
        if (do_vel) vel[3 * a] = (float)v[3 * a], vel[3 * a + 1] = (float)v[3 * a + 1], vel[3 * a + 2] = (float)v[3 * a + 2];
    }
    if (tid == 0) {
        if (do_vel) ke_g[g] = KE;
        cons.sweeps[g] = most;
    }
}

// what both entry points ask of the constraint arguments
inline int check_cons(const int32_t* cons_i, const int32_t* cons_j, const double* cons_d, const int32_t* gcol, const int32_t* colptr,
                      int64_t n_cons, const double* work, const int32_t* sweeps, double tol, int32_t max_sweeps) {
    if (n_cons < 0 || n_cons > 0x7fffffff || !(tol > 0.0 && finite(tol)) || max_sweeps < 1) return PAMNET_EINVAL;
    if (!sweeps) return PAMNET_ENULL;
    if (n_cons > 0 && (!cons_i || !cons_j || !cons_d || !gcol || !colptr || !work)) return PAMNET_ENULL;
    return PAMNET_OK;
}

}  // namespace

extern "C" int pamnet_md_constrained_step_f32(float* pos, float* vel, const float* dpos, const float* mass, const uint8_t* fixed,
                                              const int32_t* gptr, int64_t n, int64_t n_graphs, const int64_t* seed,
                                              int32_t* steps, int32_t* status, double* ke, const double* dt_g, const double* kT_g,
                                              const double* gamma_g, double dt, double kT, double gamma, int32_t kick_in,
                                              int32_t advance, const int32_t* cons_i, const int32_t* cons_j, const double* cons_d,
                                              const int32_t* gcol, const int32_t* colptr, int64_t n_cons, double* work,
                                              int32_t* sweeps, double tol, int32_t max_sweeps, pamnet_stream_t stream) {
    if (n < 0 || n_graphs < 0 || n_graphs > 0x7fffffff || !flag(kick_in) || !flag(advance)) return PAMNET_EINVAL;
    if (!dt_g && !(dt > 0.0 && finite(dt))) return PAMNET_EINVAL;
    if (!kT_g && !(kT >= 0.0 && finite(kT))) return PAMNET_EINVAL;
    if (!gamma_g && !(gamma >= 0.0 && finite(gamma))) return PAMNET_EINVAL;
    if (!pos || !vel || !dpos || !gptr || !steps || !status || !ke) return PAMNET_ENULL;
    if (!seed && (gamma_g || gamma != 0.0)) return PAMNET_ENULL;
    const int rc = check_cons(cons_i, cons_j, cons_d, gcol, colptr, n_cons, work, sweeps, tol, max_sweeps);
    if (rc != PAMNET_OK) return rc;
    if (n_graphs == 0) return PAMNET_OK;
    const StepRule rule{dt, kT, gamma, kick_in, advance};
    const Cons cons{cons_i, cons_j, cons_d, n_cons > 0 ? gcol : nullptr, colptr, n_cons, work, sweeps, tol, max_sweeps};
    hipLaunchKernelGGL(md_constrained_step_kernel, dim3((unsigned)n_graphs), dim3(256), 0, as_stream(stream), pos, vel, dpos, mass,
                       fixed, gptr, n, seed, steps, status, ke, dt_g, kT_g, gamma_g, rule, cons);
    PAMNET_LAUNCH_CHECK();
    return PAMNET_OK;
}

extern "C" int pamnet_md_project_constraints_f32(float* pos, float* vel, const float* mass, const uint8_t* fixed,
                                                 const int32_t* gptr, int64_t n, int64_t n_graphs, int32_t* status, double* ke,
                                                 const double* dt_g, double dt, const int32_t* cons_i, const int32_t* cons_j,
                                                 const double* cons_d, const int32_t* gcol, const int32_t* colptr, int64_t n_cons,
                                                 double* work, int32_t* sweeps, double tol, int32_t max_sweeps, int32_t do_pos,
                                                 int32_t do_vel, pamnet_stream_t stream) {
    if (n < 0 || n_graphs < 0 || n_graphs > 0x7fffffff || !flag(do_pos) || !flag(do_vel)) return PAMNET_EINVAL;
    if (do_vel && !dt_g && !(dt > 0.0 && finite(dt))) return PAMNET_EINVAL;
    if (!pos || !gptr || !status) return PAMNET_ENULL;
    if (do_vel && (!vel || !ke)) return PAMNET_ENULL;
    const int rc = check_cons(cons_i, cons_j, cons_d, gcol, colptr, n_cons, work, sweeps, tol, max_sweeps);
    if (rc != PAMNET_OK) return rc;
    if (n_graphs == 0) return PAMNET_OK;
    const Cons cons{cons_i, cons_j, cons_d, n_cons > 0 ? gcol : nullptr, colptr, n_cons, work, sweeps, tol, max_sweeps};
    hipLaunchKernelGGL(md_project_constraints_kernel, dim3((unsigned)n_graphs), dim3(256), 0, as_stream(stream), pos, vel, mass,
                       fixed, gptr, n, status, ke, dt_g, dt, do_pos, do_vel, cons);
    PAMNET_LAUNCH_CHECK();
    return PAMNET_OK;
}
