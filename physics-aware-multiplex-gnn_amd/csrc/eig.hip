// Batched symmetric eigensolver in fp64: cyclic Jacobi with the round-robin schedule, one workgroup per matrix --
// pamnet_sym_eig_f64 (include/pamnet_hip.h states the rule: symmetrisation, schedule, rotation, stop, order and sign).
//
// A matrix of up to 192 x 192 (288 KiB) does not fit the CU's 160 KiB of LDS, so the general form works on A and V in place in
// global memory, where a workgroup's 2 x 288 KiB stay in L2.  Up to d = 96 (72 KiB: two workgroups per CU) A is staged in dynamic
// LDS instead -- the same code on another pointer, the same bits; V stays in global memory, and the consumed `a` serves as the
// workspace of the final row permutation either way.  The launch always reserves the 72 KiB: the host knows no dimension.
// (Interleaved same-process A/B, profiles/vib.txt: 27 - 45 % less time at d = 54 and 87, alone and in batches; d = 192 equal.)
// Static LDS carries the round's rotations (p, q, c, s and the two new diagonal entries of each of the m / 2 disjoint pairs),
// the diagonal for the final ranking, and the reduction slots.  A round is three phases with a workgroup barrier after each:
//   1. parameters: thread k forms pair k of the round from a_pp, a_qq, a_pq as they stand;
//   2. columns, A <- A J: the items (row r, pair k) are dealt out with k fastest -- the two elements of a pair lie in the same
//      row, so a wavefront reads and writes whole rows (a row is at most 12 cache lines) and no element is touched twice;
//   3. rows, A <- J^T A and V <- J^T V: the items (pair k, column r) with r fastest -- rows p and q are read and written
//      contiguously.  The items at columns p and q store the exact values a_pp - t a_pq, a_qq + t a_pq and the two zeros.
// The items of a phase are independent, so a thread issues the loads of a batch of its items before the first store of the
// batch: the phase is a few memory round trips, not one per item.
// Every element of a phase is computed by exactly one thread from values no other thread writes in that phase, so the result does
// not depend on how the work is dealt out.  The only sums (|A0|_F^2 and off^2) are taken in a fixed order: a thread's elements
// ascending, the wavefront butterfly, the wavefronts in order through LDS; every thread reads the same total, so every exit is
// uniform.  No atomics, nothing exchanged between workgroups: a matrix's result is bitwise the same from run to run, alone or
// in any batch.  (Workgroup-scope visibility of the global stores comes with the barrier: one CU, one L1.)
#include "common.h"

namespace {

constexpr int kEigMax = 192;                      // the largest dimension: 64 free atoms
constexpr int kThreads = 512, kWaves = kThreads / 64;
constexpr int kColBatch = 4, kRowBatch = 2;       // items whose loads a thread issues before the first store: 8 loads in flight
constexpr double kDblMax = 1.79769313486231570815e+308;

__device__ __forceinline__ double wave_sum(double v) {            // (as relax.hip)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The sum of v over the workgroup, the same bits in every thread.  (Two barriers: the slots are free again on return.)
__device__ __forceinline__ double block_sum(double v, double* slots) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = slots[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) s += slots[w];
    __syncthreads();
    return s;
}

constexpr int kStageMax = 96;                     // A of a matrix up to this dimension is staged in dynamic LDS (72 KiB)
struct Shared {
    double c[kEigMax / 2], s[kEigMax / 2], pp[kEigMax / 2], qq[kEigMax / 2], diag[kEigMax], slots[kWaves];
    int p[kEigMax / 2], q[kEigMax / 2];
};

template <bool kStaged>
__device__ __forceinline__ void solve(double* ga, double* v, double* w, int32_t* status, int32_t* sweeps, int64_t g, int d,
                                      double tol, int32_t max_sweeps, Shared& sh, double* staged) {
    double *s_c = sh.c, *s_s = sh.s, *s_pp = sh.pp, *s_qq = sh.qq, *s_diag = sh.diag, *s_slots = sh.slots;
    int *s_p = sh.p, *s_q = sh.q;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = (d + 1) & ~1, half = m >> 1, dd = d * d;
    double* a = kStaged ? staged : ga;
    // a thread's first item of the column phase (r, k) and of the row phase (k, r), and the step of kThreads items
    const int col_r0 = tid / half, col_k0 = tid - col_r0 * half, col_dr = kThreads / half, col_dk = kThreads - col_dr * half;
    const int row_k0 = tid / d, row_r0 = tid - row_k0 * d, row_dk = kThreads / d, row_dr = kThreads - row_dk * d;

    // ---- A <- (A + A^T) / 2, V <- I, |A0|_F^2, and the test for a non-finite entry
    double acc = 0.0;
    int bad = 0;
    for (int i = tid; i < dd; i += kThreads) {
        const int p = i / d, q = i - p * d;
        v[i] = p == q ? 1.0 : 0.0;
        if (p == q) {
            const double x = ga[i];
            if (kStaged) a[i] = x;                                // (ga is the caller's array, a the working copy: LDS or ga)
            bad |= !(fabs(x) <= kDblMax);
            acc += x * x;
        } else if (p < q) {
            const double x = ga[i], y = ga[q * d + p];
            bad |= !(fabs(x) <= kDblMax) || !(fabs(y) <= kDblMax);
            const double z = (x + y) * 0.5;
            a[i] = z, a[q * d + p] = z;
            acc += 2.0 * (z * z);
        }
    }
    bad = __syncthreads_or(bad);
    if (bad) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        for (int i = tid; i < dd; i += kThreads) v[i] = nan;
        for (int i = tid; i < d; i += kThreads) w[i] = nan;
        if (tid == 0) status[g] = 2, sweeps[g] = 0;
        return;
    }
    const double norm0 = sqrt(block_sum(acc, s_slots));           // (its barriers also publish A and V)

    int done = 0, converged = 0;
    while (done < max_sweeps && !converged) {
        for (int rho = 0; rho < m - 1; ++rho) {
            // ---- 1. the round's pairs and rotations, from the matrix as it stands
            if (tid < half) {
                int p, q;
                if (tid == 0) {
                    p = m - 1, q = rho;
                } else {
                    p = rho + tid;
                    p = p >= m - 1 ? p - (m - 1) : p;
                    q = rho - tid;
                    q = q < 0 ? q + (m - 1) : q;
                }
                if (p > q) {
                    const int x = p;
                    p = q, q = x;
                }
                int active = -1;
                if (q < d) {
                    const double apq = a[p * d + q];
                    if (apq != 0.0) {
                        const double app = a[p * d + p], aqq = a[q * d + q];
                        const double theta = (aqq - app) / (2.0 * apq);
                        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                        const double c = 1.0 / sqrt(t * t + 1.0);
                        s_c[tid] = c, s_s[tid] = t * c;
                        s_pp[tid] = app - t * apq, s_qq[tid] = aqq + t * apq;
                        s_q[tid] = q;
                        active = p;
                    }
                }
                s_p[tid] = active;
            }
            __syncthreads();
            // ---- 2. columns: (a_rp, a_rq) <- (c a_rp - s a_rq, s a_rp + c a_rq) for every row r.  Item (r, k), k fastest.
            for (int r = col_r0, k = col_k0; r < d;) {
                double x[kColBatch], y[kColBatch], c[kColBatch], s[kColBatch];
                int at_p[kColBatch], at_q[kColBatch];
#pragma unroll
                for (int u = 0; u < kColBatch; ++u) {             // the loads of the batch first: the items are independent
                    at_p[u] = -1;
                    if (r < d) {
                        const int p = s_p[k];
                        if (p >= 0) {
                            at_p[u] = r * d + p, at_q[u] = r * d + s_q[k];
                            c[u] = s_c[k], s[u] = s_s[k];
                            x[u] = a[at_p[u]], y[u] = a[at_q[u]];
                        }
                    }
                    r += col_dr, k += col_dk;
                    if (k >= half) k -= half, ++r;
                }
#pragma unroll
                for (int u = 0; u < kColBatch; ++u) {
                    if (at_p[u] < 0) continue;
                    a[at_p[u]] = c[u] * x[u] - s[u] * y[u];
                    a[at_q[u]] = s[u] * x[u] + c[u] * y[u];
                }
            }
            __syncthreads();
            // ---- 3. rows of A and of V: (a_pr, a_qr) <- (c a_pr - s a_qr, s a_pr + c a_qr) for every column r.  Item (k, r),
            //         r fastest.
            for (int k = row_k0, r = row_r0; k < half;) {
                double x[kRowBatch], y[kRowBatch], vx[kRowBatch], vy[kRowBatch];
                int at_p[kRowBatch], at_q[kRowBatch], pair[kRowBatch];
#pragma unroll
                for (int u = 0; u < kRowBatch; ++u) {
                    at_p[u] = -1;
                    if (k < half) {
                        const int p = s_p[k];
                        if (p >= 0) {
                            at_p[u] = p * d + r, at_q[u] = s_q[k] * d + r, pair[u] = k;
                            x[u] = a[at_p[u]], y[u] = a[at_q[u]], vx[u] = v[at_p[u]], vy[u] = v[at_q[u]];
                        }
                    }
                    k += row_dk, r += row_dr;
                    if (r >= d) r -= d, ++k;
                }
#pragma unroll
                for (int u = 0; u < kRowBatch; ++u) {
                    if (at_p[u] < 0) continue;
                    const int kk = pair[u], p = s_p[kk], q = s_q[kk], col = at_p[u] - p * d;
                    const double c = s_c[kk], s = s_s[kk];
                    double nx = c * x[u] - s * y[u], ny = s * x[u] + c * y[u];
                    if (col == p) nx = s_pp[kk], ny = 0.0;
                    if (col == q) nx = 0.0, ny = s_qq[kk];
                    a[at_p[u]] = nx, a[at_q[u]] = ny;
                    v[at_p[u]] = c * vx[u] - s * vy[u];
                    v[at_q[u]] = s * vx[u] + c * vy[u];
                }
            }
            __syncthreads();
        }
        // ---- the sweep's off-diagonal norm
        double off2 = 0.0;
        for (int i = tid; i < dd; i += kThreads) {
            const int p = i / d;
            if (i - p * d != p) {
                const double x = a[i];
                off2 += x * x;
            }
        }
        const double off = sqrt(block_sum(off2, s_slots));
        ++done;
        converged = off <= tol * norm0;
    }

    // ---- ascending order by counting, ties by the diagonal index; the rows of V go through A (free now) to their places
    for (int i = tid; i < d; i += kThreads) s_diag[i] = a[i * d + i];
    __syncthreads();
    for (int k = wave; k < d; k += kWaves) {
        const double wk = s_diag[k];
        int rank = 0;
        for (int j = 0; j < d; ++j) {
            const double wj = s_diag[j];
            rank += (wj < wk || (wj == wk && j < k)) ? 1 : 0;
        }
        // the component of largest magnitude (the lowest index on a tie) is made positive
        const double* src = v + k * d;
        double best = -1.0;
        int at = 0x7fffffff;
        for (int r = lane; r < d; r += 64) {
            const double x = fabs(src[r]);
            if (x > best) best = x, at = r;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const double ob = __shfl_xor(best, o, 64);
            const int oa = __shfl_xor(at, o, 64);
            if (ob > best || (ob == best && oa < at)) best = ob, at = oa;
        }
        const double sign = (at < d && src[at] < 0.0) ? -1.0 : 1.0;
        double* dst = ga + rank * d;
        for (int r = lane; r < d; r += 64) dst[r] = sign * src[r];
        if (lane == 0) w[rank] = wk;
    }
    __syncthreads();
    for (int i = tid; i < dd; i += kThreads) v[i] = ga[i];
    if (tid == 0) status[g] = converged ? 0 : 1, sweeps[g] = done;
}


__global__ __launch_bounds__(kThreads) void sym_eig_kernel(double* a_all, double* v_all, double* w_all, int32_t* status,
                                                           int32_t* sweeps, const int64_t* __restrict__ moff,
                                                           const int64_t* __restrict__ dptr, double tol, int32_t max_sweeps) {
    __shared__ Shared sh;
    extern __shared__ double staged[];
    const int64_t g = blockIdx.x;
    const int64_t d64 = dptr[g + 1] - dptr[g];
    if (d64 <= 0) return;                                         // (uniform, as every exit of the workgroup)
    if (d64 > kEigMax) {
        if (threadIdx.x == 0) status[g] = 3;
        return;
    }
    if (d64 <= kStageMax)
        solve<true>(a_all + moff[g], v_all + moff[g], w_all + dptr[g], status, sweeps, g, (int)d64, tol, max_sweeps, sh, staged);
    else
        solve<false>(a_all + moff[g], v_all + moff[g], w_all + dptr[g], status, sweeps, g, (int)d64, tol, max_sweeps, sh, staged);
}

}  // namespace

extern "C" int pamnet_sym_eig_f64(double* a, double* v, double* w, int32_t* status, int32_t* sweeps, const int64_t* moff,
                                  const int64_t* dptr, int64_t n_mat, double tol, int32_t max_sweeps, pamnet_stream_t stream) {
    if (n_mat < 0 || n_mat > 0x7fffffff || !(tol >= 0.0) || max_sweeps < 1) return PAMNET_EINVAL;
    if (!a || !v || !w || !status || !sweeps || !moff || !dptr) return PAMNET_ENULL;
    if (n_mat == 0) return PAMNET_OK;
    constexpr int kBytes = kStageMax * kStageMax * (int)sizeof(double);
    static const hipError_t raised = hipFuncSetAttribute(reinterpret_cast<const void*>(sym_eig_kernel),
                                                        hipFuncAttributeMaxDynamicSharedMemorySize, kBytes);   // (above 64 KiB)
    if (raised != hipSuccess) return (int)raised;
    hipLaunchKernelGGL(sym_eig_kernel, dim3((unsigned)n_mat), dim3(kThreads), kBytes, as_stream(stream), a, v, w, status, sweeps, moff,
                       dptr, tol, max_sweeps);
    PAMNET_LAUNCH_CHECK();
    return PAMNET_OK;
}
