// Structure relaxation, quasi-Newton: one limited-memory BFGS step for every graph of a batch in one launch --
// pamnet_lbfgs_step_f32 (include/pamnet_hip.h states the rule and the order of its updates).
//
// The shape is fire_step_kernel's (relax.hip): one workgroup of 256 threads per graph g, the threads striding over the atoms
// gptr[g] .. gptr[g + 1] (kept inside [0, n]).  The passes, each ending in one workgroup reduction:
//   1. F2, max |gr|^2 and, where the graph has a previous step, ss, yy, ys of the new pair;
//   2. q = gr into `work` (and the new pair into its ring slot), with s_0 . q -- or, without a history, z = q / alpha with D and
//      max |z|^2 at once;
//   3. for every pair, newest first: q -= a_j y_j with the next pair's s . q; the oldest pair's pass also forms z = h0 q and y . z;
//   4. for every pair, oldest first: z += (a_j - b) s_j with the next pair's y . z; the newest pair's pass also forms D = z . gr
//      and max |z|^2;
//   5. the stores of prev_pos, prev_dpos and pos (no reduction).
// That is 2 count + 2 reductions.  q and z live in `work`, and an atom's rows of work, hist_s and hist_y are read and written by
// the one thread that owns the atom -- the pair stored in pass 2 included, which passes 3 and 4 read back -- so no global
// memory is handed from thread to thread and nothing is kept per thread that a large graph could outgrow.
// Every thread reads the same four wavefront partials from LDS and adds them in the same order, so every decision of the graph
// (converged / failed, store or skip the pair, reset, the cap) and every a_j and b is formed by every thread alike: nothing is
// broadcast and every exit is uniform.  Consecutive reductions ALTERNATE between two sets of LDS partials, with one barrier
// each: a wavefront that writes the partials of round k + 2 has passed the barrier of round k + 1, which every wavefront
// reaches only after it has read round k -- with one set, a fast wavefront could overwrite what a slow one still reads.  The
// a_j are the same in every thread but indexed by the loop counter of pass 4, so they are kept in LDS (thread 0 writes a_j
// before the barrier of its pass; pass 4 reads it after), not in a per-thread array that would live in scratch.
// Sums in a fixed order -- a thread's atoms ascending, the wavefront butterfly, the four wavefronts in wave order -- and no
// atomics: a graph's result is bitwise the same from run to run and whatever else the batch holds.  Thread 0 writes the graph's
// state at the end, after every thread has read it (the reads are before the first barrier, rho's before the last).
#include "common.h"

namespace {

constexpr int kMaxMemory = 32;
constexpr double kDblMax = 1.79769313486231570815e+308;

struct LbfgsRule {
    double fmax_tol, alpha, max_step, skip_tol;
    int32_t memory;
};

struct V3 {
    double x, y, z;
};
__device__ __forceinline__ V3 load3(const float* __restrict__ p, int64_t row) {
    return V3{(double)p[3 * row], (double)p[3 * row + 1], (double)p[3 * row + 2]};
}
__device__ __forceinline__ V3 load3(const double* __restrict__ p, int64_t row) {
    return V3{p[3 * row], p[3 * row + 1], p[3 * row + 2]};
}
__device__ __forceinline__ void store3(double* __restrict__ p, int64_t row, const V3& v) {
    p[3 * row] = v.x, p[3 * row + 1] = v.y, p[3 * row + 2] = v.z;
}
__device__ __forceinline__ double dot(const V3& a, const V3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 sub(const V3& a, const V3& b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
// a + c b
__device__ __forceinline__ V3 axpy(const V3& a, double c, const V3& b) { return V3{a.x + c * b.x, a.y + c * b.y, a.z + c * b.z}; }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {           // (operands >= 0 or NaN; a NaN never reaches a use, see F2)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// One workgroup reduction of NS sums and, where MAX, one maximum: every thread returns with the same values.  `round` picks
// the set of partials and is advanced; it is the same in every thread.
template <int NS, bool MAX>
__device__ __forceinline__ void block_reduce(double (&s)[NS], double& mx, double (*part)[4][5], int& round, int lane, int wave) {
    double(*p)[5] = part[round & 1];
    round += 1;
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = wave_sum(s[k]);
    if (MAX) mx = wave_max(mx);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NS; ++k) p[wave][k] = s[k];
        if (MAX) p[wave][4] = mx;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = (p[0][k] + p[1][k]) + (p[2][k] + p[3][k]);
    if (MAX) mx = fmax(fmax(p[0][4], p[1][4]), fmax(p[2][4], p[3][4]));
}

__global__ __launch_bounds__(256) void lbfgs_step_kernel(
    float* __restrict__ pos, const float* __restrict__ dpos, const uint8_t* __restrict__ fixed, const int32_t* __restrict__ gptr,
    int64_t n, float* __restrict__ prev_pos, float* __restrict__ prev_dpos, double* __restrict__ hist_s,
    double* __restrict__ hist_y, double* __restrict__ work, double* __restrict__ rho_g, double* __restrict__ gamma_g,
    int32_t* __restrict__ head_g, int32_t* __restrict__ count_g, int32_t* __restrict__ has_prev_g, int32_t* __restrict__ skipped_g,
    int32_t* __restrict__ resets_g, int32_t* __restrict__ steps_g, int32_t* __restrict__ status_g, float* __restrict__ fmax_g,
    const float* __restrict__ fmax_tol_g, LbfgsRule rule) {
    __shared__ double part[2][4][5];
    __shared__ double a_lds[kMaxMemory];
    const int64_t g = blockIdx.x;
    if (status_g[g] != 0) return;                                 // step 1 (uniform over the workgroup): g is left alone
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t lo = gptr[g], hi = gptr[g + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n ? n : hi;
    const int m = rule.memory;
    // the graph's state (read by every thread before thread 0 writes it, at the end); head and count kept inside the ring
    int head = head_g[g] % m, count = count_g[g];
    head = head < 0 ? head + m : head;
    count = count < 0 ? 0 : (count > m ? m : count);
    const bool has_prev = has_prev_g[g] != 0;
    double gamma = gamma_g[g];
    const double tol = fmax_tol_g ? (double)fmax_tol_g[g] : rule.fmax_tol;
    double* __restrict__ rho = rho_g + g * m;
    int round = 0;

    // ---- pass 1: step 2 and the sums of step 3
    double sums[4] = {0.0, 0.0, 0.0, 0.0}, fm2 = 0.0;            // F2, ss, yy, ys
    for (int64_t a = lo + tid; a < hi; a += 256) {
        if (fixed && fixed[a]) continue;
        const V3 gr = load3(dpos, a);
        const double g2 = dot(gr, gr);
        sums[0] += g2;
        fm2 = fmax(fm2, g2);
        if (has_prev) {
            const V3 s = sub(load3(pos, a), load3(prev_pos, a)), y = sub(gr, load3(prev_dpos, a));
            sums[1] += dot(s, s);
            sums[2] += dot(y, y);
            sums[3] += dot(s, y);
        }
    }
    block_reduce<4, true>(sums, fm2, part, round, lane, wave);
    const double F2 = sums[0], ss = sums[1], yy = sums[2], ys = sums[3];
    // F2 is a sum of squares: NaN where a component is NaN, +inf where one is infinite and none NaN -- the failed graph
    // reports sqrt(F2), as fire_step_kernel does
    const bool failed = !(F2 <= kDblMax);
    const double fm = failed ? sqrt(F2) : sqrt(fm2);
    const bool converged = !failed && fm < tol;
    if (failed || converged) {
        if (tid == 0) {
            fmax_g[g] = (float)fm;
            status_g[g] = failed ? 2 : 1;
        }
        return;                                                   // (uniform)
    }

    // ---- step 3: the curvature test of the new pair
    const bool store = has_prev && ys > rule.skip_tol * sqrt(ss * yy);
    const int slot_new = head;
    double rho_new = 0.0;
    if (store) {
        rho_new = 1.0 / ys;
        gamma = ys / yy;
        head = head + 1 == m ? 0 : head + 1;
        count = count < m ? count + 1 : m;
    }
    // pair j of the recursion: slot (head - 1 - j) mod m; its rho is the new one where the slot was just filled
    auto slot_of = [&](int j) {
        const int k = head - 1 - j;
        return k < 0 ? k + m : k;
    };
    auto rho_of = [&](int k) { return store && k == slot_new ? rho_new : rho[k]; };
    const double h0 = count > 0 ? gamma : 1.0 / rule.alpha;

    // ---- pass 2: q = gr, the new pair into its slot; s_0 . q, or without a history z = h0 q, D and max |z|^2
    double acc[1] = {0.0}, L2 = 0.0;
    {
        const int64_t s0 = count > 0 ? (int64_t)slot_of(0) * n : 0;
        for (int64_t a = lo + tid; a < hi; a += 256) {
            if (fixed && fixed[a]) continue;
            const V3 gr = load3(dpos, a);
            if (store) {
                store3(hist_s, (int64_t)slot_new * n + a, sub(load3(pos, a), load3(prev_pos, a)));
                store3(hist_y, (int64_t)slot_new * n + a, sub(gr, load3(prev_dpos, a)));
            }
            if (count > 0) {
                acc[0] += dot(load3(hist_s, s0 + a), gr);
                store3(work, a, gr);
            } else {
                const V3 z{h0 * gr.x, h0 * gr.y, h0 * gr.z};
                acc[0] += dot(z, gr);
                L2 = fmax(L2, dot(z, z));
                store3(work, a, z);
            }
        }
    }
    if (count > 0)
        block_reduce<1, false>(acc, L2, part, round, lane, wave);
    else
        block_reduce<1, true>(acc, L2, part, round, lane, wave);

    if (count > 0) {
        // ---- pass 3: newest pair first
        for (int j = 0; j < count; ++j) {
            const int k = slot_of(j);
            const double a_j = rho_of(k) * acc[0];
            if (tid == 0) a_lds[j] = a_j;
            const bool last = j == count - 1;
            const int64_t yk = (int64_t)k * n, sn = last ? 0 : (int64_t)slot_of(j + 1) * n;
            acc[0] = 0.0;
            for (int64_t a = lo + tid; a < hi; a += 256) {
                if (fixed && fixed[a]) continue;
                const V3 y = load3(hist_y, yk + a);
                V3 q = axpy(load3(work, a), -a_j, y);
                if (last) {
                    q = V3{h0 * q.x, h0 * q.y, h0 * q.z};         // z
                    acc[0] += dot(y, q);
                } else {
                    acc[0] += dot(load3(hist_s, sn + a), q);
                }
                store3(work, a, q);
            }
            block_reduce<1, false>(acc, L2, part, round, lane, wave);
        }
        // ---- pass 4: oldest pair first
        for (int j = count - 1; j >= 0; --j) {
            const int k = slot_of(j);
            const double coef = a_lds[j] - rho_of(k) * acc[0];
            const bool last = j == 0;
            const int64_t sk = (int64_t)k * n, yn = last ? 0 : (int64_t)slot_of(j - 1) * n;
            acc[0] = 0.0;
            for (int64_t a = lo + tid; a < hi; a += 256) {
                if (fixed && fixed[a]) continue;
                const V3 z = axpy(load3(work, a), coef, load3(hist_s, sk + a));
                if (last) {
                    acc[0] += dot(z, load3(dpos, a));
                    L2 = fmax(L2, dot(z, z));
                } else {
                    acc[0] += dot(load3(hist_y, yn + a), z);
                }
                store3(work, a, z);
            }
            if (last)
                block_reduce<1, true>(acc, L2, part, round, lane, wave);
            else
                block_reduce<1, false>(acc, L2, part, round, lane, wave);
        }
    }

    // ---- step 5: the descent check; step 6: the cap
    const bool reset = !(acc[0] > 0.0);
    const double L = reset ? fm / rule.alpha : sqrt(L2);
    const double c = L > rule.max_step ? rule.max_step / L : 1.0;
    if (reset) head = 0, count = 0;

    // ---- pass 5: the stores (an atom is read and written by one thread only)
    for (int64_t a = lo + tid; a < hi; a += 256) {
        if (fixed && fixed[a]) continue;
        const V3 gr = load3(dpos, a);
        const V3 z = reset ? V3{gr.x / rule.alpha, gr.y / rule.alpha, gr.z / rule.alpha} : load3(work, a);
        const float px = pos[3 * a], py = pos[3 * a + 1], pz = pos[3 * a + 2];
        prev_pos[3 * a] = px, prev_pos[3 * a + 1] = py, prev_pos[3 * a + 2] = pz;
        prev_dpos[3 * a] = dpos[3 * a], prev_dpos[3 * a + 1] = dpos[3 * a + 1], prev_dpos[3 * a + 2] = dpos[3 * a + 2];
        pos[3 * a] = (float)((double)px - c * z.x);
        pos[3 * a + 1] = (float)((double)py - c * z.y);
        pos[3 * a + 2] = (float)((double)pz - c * z.z);
    }
    if (tid == 0) {
        fmax_g[g] = (float)fm;
        if (store) {
            rho[slot_new] = rho_new;
            gamma_g[g] = gamma;
        } else if (has_prev) {
            skipped_g[g] += 1;
        }
        if (reset) resets_g[g] += 1;
        head_g[g] = head;
        count_g[g] = count;
        has_prev_g[g] = 1;
        steps_g[g] += 1;
    }
}

inline bool positive(double v) { return v > 0.0 && v <= kDblMax; }

}  // namespace

extern "C" int pamnet_lbfgs_step_f32(float* pos, const float* dpos, const uint8_t* fixed, const int32_t* gptr, int64_t n,
                                     int64_t n_graphs, float* prev_pos, float* prev_dpos, double* hist_s, double* hist_y,
                                     double* work, double* rho, double* gamma, int32_t* head, int32_t* count, int32_t* has_prev,
                                     int32_t* skipped, int32_t* resets, int32_t* steps, int32_t* status, float* fmax,
                                     const float* fmax_tol_g, double fmax_tol, int32_t memory, double alpha, double max_step,
                                     double skip_tol, pamnet_stream_t stream) {
    if (n < 0 || n_graphs < 0 || n_graphs > 0x7fffffff || memory < 1 || memory > kMaxMemory) return PAMNET_EINVAL;
    if (!positive(alpha) || !positive(max_step) || !(skip_tol >= 0.0 && skip_tol <= kDblMax) || fmax_tol != fmax_tol)
        return PAMNET_EINVAL;
    if (!pos || !dpos || !gptr || !prev_pos || !prev_dpos || !hist_s || !hist_y || !work || !rho || !gamma || !head || !count ||
        !has_prev || !skipped || !resets || !steps || !status || !fmax)
        return PAMNET_ENULL;
    if (n_graphs == 0) return PAMNET_OK;
    const LbfgsRule rule{fmax_tol, alpha, max_step, skip_tol, memory};
    hipLaunchKernelGGL(lbfgs_step_kernel, dim3((unsigned)n_graphs), dim3(256), 0, as_stream(stream), pos, dpos, fixed, gptr, n,
                       prev_pos, prev_dpos, hist_s, hist_y, work, rho, gamma, head, count, has_prev, skipped, resets, steps, status,
                       fmax, fmax_tol_g, rule);
    PAMNET_LAUNCH_CHECK();
    return PAMNET_OK;
}
