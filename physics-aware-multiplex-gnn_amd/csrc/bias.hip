// Biased dynamics over collective variables: harmonic restraints (umbrella windows, walls) and well-tempered metadynamics
// (Barducci, Bussi & Parrinello, Phys. Rev. Lett. 100, 020603, 2008) with multiple walkers (Raiteri et al., J. Phys. Chem. B 110,
// 3533, 2006) -- pamnet_bias_apply_f64, one launch per step between the model evaluation and the step launch, and
// pamnet_bias_grid_f64, the bias of one hill table on a set of points (include/pamnet_hip.h states the rule).
//
// A bias group is a run of consecutive graphs that share one hill table: one graph is an ordinary simulation, W graphs are W
// walkers.  One workgroup of 256 threads per group handles its walkers one after another:
//   A. thread k forms collective variable k of the graph and its gradient (up to 12 numbers) in LDS, in fp64;
//   B. the workgroup strides over the hills [0, n0) -- n0 is read once, before anything is deposited --: every thread adds its
//      hills in hill order, wave_sum adds the lanes, the four wave partials are added in wave order from LDS;
//   C. thread 0 walks the variables of the graph in order and the atoms of each in order and adds c_k ds_k/dx to dpos, one
//      rounding to fp32 per component: atoms shared by two variables are handled by that order, not by atomics.
// Behind the last walker thread 0 appends the hills of the walkers in graph order.  Every loop count (the walkers, the variables
// of a graph, the hills) is read by all threads alike and no thread leaves before the last barrier.  No atomics and no sum whose
// order depends on the batch: a group reads and writes its own entries only, so its outputs are bitwise repeatable and the same
// alone or inside any batch.
#include "md_core.h"                              // wave_sum, finite

namespace {

constexpr int BIAS_MAX_WALKERS = 256;             // the graphs of one group at most: one LDS entry per walker
constexpr int BIAS_MAX_CVS = 16;                  // the collective variables of one graph at most: one thread and one LDS row each
constexpr int CV_DISTANCE = 0, CV_ANGLE = 1, CV_DIHEDRAL = 2;
constexpr double TWO_PI = 6.283185307179586476925286766559;

struct V3 {
    double x, y, z;
};
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 load3(const float* __restrict__ pos, int64_t a) {
    return {(double)pos[3 * a], (double)pos[3 * a + 1], (double)pos[3 * a + 2]};
}
__device__ __forceinline__ void put(double* g, int a, V3 v, double s) { g[3 * a] = s * v.x, g[3 * a + 1] = s * v.y, g[3 * a + 2] = s * v.z; }
__device__ __forceinline__ void put2(double* g, int a, V3 u, double s, V3 v, double t) {
    g[3 * a] = s * u.x + t * v.x, g[3 * a + 1] = s * u.y + t * v.y, g[3 * a + 2] = s * u.z + t * v.z;
}
__device__ __forceinline__ int atoms_of(int kind) { return kind == CV_DISTANCE ? 2 : kind == CV_ANGLE ? 3 : kind == CV_DIHEDRAL ? 4 : 0; }
// a difference of two values of a variable: a dihedral is periodic
__device__ __forceinline__ double diff(double s, double c, bool periodic) {
    const double d = s - c;
    return periodic ? d - TWO_PI * rint(d / TWO_PI) : d;
}

// The variable of `kind` on the atoms at[0 .. 3] and its gradient g[3 a + c] = ds / dx_{a, c}; returns s.
__device__ __forceinline__ double form_cv(const float* __restrict__ pos, int kind, const int64_t* at, double* g) {
    if (kind == CV_DISTANCE) {
        const V3 r = sub(load3(pos, at[1]), load3(pos, at[0]));
        const double d = sqrt(dot(r, r));
        put(g, 0, r, -1.0 / d), put(g, 1, r, 1.0 / d);
        return d;
    }
    if (kind == CV_ANGLE) {                       // theta = atan2(|a x b|, a . b) at the middle atom: well conditioned at 0 and pi
        const V3 xj = load3(pos, at[1]);
        const V3 a = sub(load3(pos, at[0]), xj), b = sub(load3(pos, at[2]), xj);
        const V3 nn = cross(a, b);
        const double n1 = sqrt(dot(nn, nn));
        const V3 gi = cross(a, nn), gk = cross(nn, b);
        const double si = 1.0 / (dot(a, a) * n1), sk = 1.0 / (dot(b, b) * n1);
        put(g, 0, gi, si), put(g, 2, gk, sk), put2(g, 1, gi, -si, gk, -sk);
        return atan2(n1, dot(a, b));
    }
    // the dihedral and its gradient (Blondel & Karplus, J. Comput. Chem. 17, 1132, 1996) in b1, b2, b3
    const V3 xi = load3(pos, at[0]), xj = load3(pos, at[1]), xk = load3(pos, at[2]), xl = load3(pos, at[3]);
    const V3 b1 = sub(xj, xi), b2 = sub(xk, xj), b3 = sub(xl, xk);
    const V3 m = cross(b1, b2), nn = cross(b2, b3);
    const double l2 = sqrt(dot(b2, b2)), m2 = dot(m, m), n2 = dot(nn, nn);
    const double p = dot(b1, b2) / (m2 * l2), q = dot(b3, b2) / (n2 * l2);
    put(g, 0, m, -l2 / m2), put(g, 3, nn, l2 / n2);
    put2(g, 1, m, l2 / m2 + p, nn, q), put2(g, 2, m, -p, nn, -q - l2 / n2);
    return atan2(l2 * dot(b1, nn), dot(m, nn));
}

__global__ __launch_bounds__(256) void bias_apply_kernel(
    const float* __restrict__ pos, float* __restrict__ dpos, int32_t* __restrict__ status, const int32_t* __restrict__ gptr,
    const int32_t* __restrict__ bptr, const int32_t* __restrict__ cvptr, const int32_t* __restrict__ kind,
    const int32_t* __restrict__ atoms, const double* __restrict__ kappa, const double* __restrict__ centre,
    const double* __restrict__ halfwidth, const int32_t* __restrict__ ndim, const double* __restrict__ sigma,
    const double* __restrict__ height0, const double* __restrict__ inv_dT, double* __restrict__ hill_c,
    double* __restrict__ hill_w, int32_t* __restrict__ n_hills, int32_t* __restrict__ dropped, double* __restrict__ cv,
    double* __restrict__ ebias, int64_t n, int64_t n_graphs, int64_t n_cvs, int64_t h_cap, int deposit) {
    __shared__ double s_cv[BIAS_MAX_CVS];                         // phase A: the variables of the graph ...
    __shared__ double s_grad[BIAS_MAX_CVS][12];                   // ... their gradients ...
    __shared__ int32_t s_kind[BIAS_MAX_CVS], s_ok[BIAS_MAX_CVS];  // ... their kinds, and whether all of it is finite
    __shared__ int64_t s_atom[BIAS_MAX_CVS][4];
    __shared__ double s_part[4][3];                               // phase B: (V, dV/ds_0, dV/ds_1) of every wave
    __shared__ double w_s[BIAS_MAX_WALKERS][2], w_v[BIAS_MAX_WALKERS];   // what a walker deposits: its centre and its V ...
    __shared__ int32_t w_dep[BIAS_MAX_WALKERS];                   // ... and whether it does (thread 0 writes and reads these)
    const int64_t t = blockIdx.x;
    const int tid = threadIdx.x;
    int64_t lo = bptr[t], hi = bptr[t + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n_graphs ? n_graphs : hi;
    const int64_t W = hi - lo;
    if (W > BIAS_MAX_WALKERS) return;             // (uniform; the entry point and the driver refuse such a group)
    int nd = ndim[t];
    nd = nd < 0 ? 0 : nd > 2 ? 2 : nd;
    int64_t n0 = n_hills[t];                      // (read by every thread before thread 0 writes it, behind the last barrier)
    n0 = n0 < 0 ? 0 : n0 > h_cap ? h_cap : n0;
    const double sg0 = sigma[2 * t], sg1 = sigma[2 * t + 1];
    const double* __restrict__ hc = hill_c + 2 * t * h_cap;
    const double* __restrict__ hw = hill_w + t * h_cap;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);

    for (int64_t w = 0; w < W; ++w) {
        const int64_t g = lo + w;
        int64_t k0 = cvptr[g], k1 = cvptr[g + 1];
        k0 = k0 < 0 ? 0 : k0;
        k1 = k1 > n_cvs ? n_cvs : k1;
        const int64_t nk = k1 > k0 ? k1 - k0 : 0;
        if (status[g] != 0 || nk > BIAS_MAX_CVS) {                // skipped (uniform: every thread reads the same entries)
            for (int64_t k = k0 + tid; k < k1; k += 256) cv[k] = nan;
            if (tid == 0) ebias[g] = nan, w_dep[w] = 0;
            continue;
        }
        int64_t alo = gptr[g], ahi = gptr[g + 1];
        alo = alo < 0 ? 0 : alo;
        ahi = ahi > n ? n : ahi;

        // ---- phase A: thread k forms variable k
        if (tid < nk) {
            const int kd = kind[k0 + tid];
            const int na = atoms_of(kd);
            int64_t at[4];
            bool ok = na > 0;
            for (int a = 0; a < 4; ++a) {
                at[a] = a < na ? (int64_t)atoms[4 * (k0 + tid) + a] : alo;
                ok = ok && at[a] >= alo && at[a] < ahi;           // (an atom outside the graph: nothing of pos is read)
                s_atom[tid][a] = at[a];
            }
            double gr[12];
#pragma unroll
            for (int c = 0; c < 12; ++c) gr[c] = 0.0;
            double s = nan;
            if (ok) {
                s = form_cv(pos, kd, at, gr);
                ok = finite(s);
#pragma unroll
                for (int c = 0; c < 12; ++c) ok = ok && finite(gr[c]);
            }
#pragma unroll
            for (int c = 0; c < 12; ++c) s_grad[tid][c] = gr[c];
            s_cv[tid] = s, s_kind[tid] = kd, s_ok[tid] = ok ? 1 : 0;
        }
        __syncthreads();
        bool good = true;
        for (int k = 0; k < (int)nk; ++k) good = good && s_ok[k] != 0;       // (uniform: every thread reads the same entries)
        const int nde = !good ? 0 : nd < (int)nk ? nd : (int)nk;             // the dimensions of the hills this graph feels

        // ---- phase B: the hills [0, n0) against (s_0, s_1)
        double v = 0.0, d0 = 0.0, d1 = 0.0;
        if (nde > 0) {
            const double s0 = s_cv[0], s1 = nde > 1 ? s_cv[1] : 0.0;
            const bool p0 = s_kind[0] == CV_DIHEDRAL, p1 = nde > 1 && s_kind[1] == CV_DIHEDRAL;
            for (int64_t h = tid; h < n0; h += 256) {
                const double u0 = diff(s0, hc[2 * h], p0) / sg0;
                const double u1 = nde > 1 ? diff(s1, hc[2 * h + 1], p1) / sg1 : 0.0;
                const double e = hw[h] * exp(-0.5 * (u0 * u0 + u1 * u1));
                v += e, d0 -= e * u0 / sg0;
                if (nde > 1) d1 -= e * u1 / sg1;
            }
        }
        v = wave_sum(v), d0 = wave_sum(d0), d1 = wave_sum(d1);
        if ((tid & 63) == 0) s_part[tid >> 6][0] = v, s_part[tid >> 6][1] = d0, s_part[tid >> 6][2] = d1;
        __syncthreads();

        // ---- phase C: the energy, the forces and the record of the walker
        if (tid < nk) cv[k0 + tid] = good ? s_cv[tid] : nan;
        if (tid == 0) {
            if (!good) {
                status[g] = 2, ebias[g] = nan, w_dep[w] = 0;
            } else {
                const double V = ((s_part[0][0] + s_part[1][0]) + s_part[2][0]) + s_part[3][0];
                const double dV0 = ((s_part[0][1] + s_part[1][1]) + s_part[2][1]) + s_part[3][1];
                const double dV1 = ((s_part[0][2] + s_part[1][2]) + s_part[2][2]) + s_part[3][2];
                double E = V;
                for (int k = 0; k < (int)nk; ++k) {
                    double c = k >= nde ? 0.0 : k == 0 ? dV0 : dV1;
                    const double kap = kappa[k0 + k];
                    if (kap != 0.0) {
                        const double d = diff(s_cv[k], centre[k0 + k], s_kind[k] == CV_DIHEDRAL);
                        const double a = fabs(d) - halfwidth[k0 + k];
                        if (a > 0.0) E += 0.5 * kap * a * a, c += d < 0.0 ? -kap * a : kap * a;
                    }
                    if (c == 0.0) continue;                       // nothing to add: the rows stay bitwise
                    const int na = atoms_of(s_kind[k]);
                    for (int a = 0; a < na; ++a) {
                        const int64_t at = s_atom[k][a];
#pragma unroll
                        for (int x = 0; x < 3; ++x)
                            dpos[3 * at + x] = (float)((double)dpos[3 * at + x] + c * s_grad[k][3 * a + x]);
                    }
                }
                ebias[g] = E;
                w_s[w][0] = nde > 0 ? s_cv[0] : 0.0, w_s[w][1] = nde > 1 ? s_cv[1] : 0.0, w_v[w] = V;
                w_dep[w] = nde > 0 ? 1 : 0;
            }
        }
        __syncthreads();                          // (the LDS rows of this walker are free for the next)
    }

    // ---- deposit: the walkers in graph order, against the V of the old hills
    if (tid == 0 && deposit && nd > 0) {
        int64_t cnt = n0;
        int32_t lost = 0;
        const double h0 = height0[t], idt = inv_dT[t];
        for (int64_t w = 0; w < W; ++w) {
            if (!w_dep[w]) continue;
            if (cnt >= h_cap) {
                ++lost;
                continue;
            }
            hill_c[2 * (t * h_cap + cnt)] = w_s[w][0], hill_c[2 * (t * h_cap + cnt) + 1] = w_s[w][1];
            hill_w[t * h_cap + cnt] = h0 * exp(-w_v[w] * idt);
            ++cnt;
        }
        n_hills[t] = (int32_t)cnt;
        if (lost) dropped[t] += lost;
    }
}

__global__ __launch_bounds__(256) void bias_grid_kernel(const double* __restrict__ hill_c, const double* __restrict__ hill_w,
                                                        const int32_t* __restrict__ n_hills, const double* __restrict__ sigma,
                                                        const int32_t* __restrict__ periodic, const double* __restrict__ points,
                                                        double* __restrict__ out, int64_t t, int64_t h_cap, int64_t m, int nd) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;                           // (no barrier follows)
    int64_t n0 = n_hills[t];
    n0 = n0 < 0 ? 0 : n0 > h_cap ? h_cap : n0;
    const double sg0 = sigma[2 * t], sg1 = sigma[2 * t + 1];
    const bool p0 = periodic[2 * t] != 0, p1 = nd > 1 && periodic[2 * t + 1] != 0;
    const double* __restrict__ hc = hill_c + 2 * t * h_cap;
    const double* __restrict__ hw = hill_w + t * h_cap;
    const double s0 = points[nd * i], s1 = nd > 1 ? points[nd * i + 1] : 0.0;
    double v = 0.0;
    for (int64_t h = 0; h < n0; ++h) {            // the hills in order
        const double u0 = diff(s0, hc[2 * h], p0) / sg0;
        const double u1 = nd > 1 ? diff(s1, hc[2 * h + 1], p1) / sg1 : 0.0;
        v += hw[h] * exp(-0.5 * (u0 * u0 + u1 * u1));
    }
    out[i] = v;
}

}  // namespace

extern "C" int pamnet_bias_apply_f64(const float* pos, float* dpos, int32_t* status, const int32_t* gptr, const int32_t* bptr,
                                     const int32_t* cvptr, const int32_t* kind, const int32_t* atoms, const double* kappa,
                                     const double* centre, const double* halfwidth, const int32_t* ndim, const double* sigma,
                                     const double* height0, const double* inv_dT, double* hill_c, double* hill_w,
                                     int32_t* n_hills, int32_t* dropped, double* cv, double* ebias, int64_t n, int64_t n_graphs,
                                     int64_t n_groups, int64_t n_cvs, int64_t h_cap, int32_t deposit, pamnet_stream_t stream) {
    if (n < 0 || n_graphs < 0 || n_groups < 0 || n_cvs < 0 || h_cap < 0 || n_graphs > 0x7fffffff || n_groups > 0x7fffffff ||
        n_cvs > 0x7fffffff || h_cap > 0x7fffffff || !flag(deposit))
        return PAMNET_EINVAL;
    if (!pos || !dpos || !status || !gptr || !bptr || !cvptr || !kind || !atoms || !kappa || !centre || !halfwidth || !ndim ||
        !sigma || !height0 || !inv_dT || !hill_c || !hill_w || !n_hills || !dropped || !cv || !ebias)
        return PAMNET_ENULL;
    if (n_groups == 0) return PAMNET_OK;
    // bptr and cvptr live on the device and are not read here: what the counts alone prove is refused -- n_groups groups of at
    // most BIAS_MAX_WALKERS graphs, n_graphs graphs of at most BIAS_MAX_CVS variables
    if (n_graphs > n_groups * (int64_t)BIAS_MAX_WALKERS || n_cvs > n_graphs * (int64_t)BIAS_MAX_CVS) return PAMNET_EINVAL;
    hipLaunchKernelGGL(bias_apply_kernel, dim3((unsigned)n_groups), dim3(256), 0, as_stream(stream), pos, dpos, status, gptr, bptr,
                       cvptr, kind, atoms, kappa, centre, halfwidth, ndim, sigma, height0, inv_dT, hill_c, hill_w, n_hills, dropped,
                       cv, ebias, n, n_graphs, n_cvs, h_cap, (int)deposit);
    PAMNET_LAUNCH_CHECK();
    return PAMNET_OK;
}

extern "C" int pamnet_bias_grid_f64(const double* hill_c, const double* hill_w, const int32_t* n_hills, const double* sigma,
                                    const int32_t* periodic, const double* points, double* out, int64_t table, int64_t n_groups,
                                    int64_t h_cap, int64_t n_points, int32_t ndim, pamnet_stream_t stream) {
    if (n_groups < 0 || h_cap < 0 || n_points < 0 || table < 0 || table >= n_groups || n_groups > 0x7fffffff ||
        h_cap > 0x7fffffff || n_points > 0x7fffffff * (int64_t)256 || ndim < 1 || ndim > 2)
        return PAMNET_EINVAL;
    if (!hill_c || !hill_w || !n_hills || !sigma || !periodic || !points || !out) return PAMNET_ENULL;
    if (n_points == 0) return PAMNET_OK;
    hipLaunchKernelGGL(bias_grid_kernel, dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, as_stream(stream), hill_c, hill_w,
                       n_hills, sigma, periodic, points, out, table, h_cap, n_points, (int)ndim);
    PAMNET_LAUNCH_CHECK();
    return PAMNET_OK;
}
