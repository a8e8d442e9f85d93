// Finite-difference Hessians: the two bookkeeping launches around an evaluation of displaced copies of a batch --
// pamnet_vib_displace_f32 and pamnet_vib_rows_f64 (include/pamnet_hip.h states the layout and both rules).
//
// An evaluation holds `pairs` central-difference pairs per graph: the evaluated batch is 2 pairs copies of the original one,
// copy 2c the + and copy 2c + 1 the - displacement of pair c.  In evaluation t, pair c of graph g has job j = t pairs + c and
// displaces component j % 3 of free atom j / 3 of the graph where j < 3 F_g; otherwise it is idle.
//   displace: one workgroup per (graph, copy) copies the graph's rows of pos0 into the copy; the one thread that holds the
//             displaced coordinate stores x0 +- delta instead (no second pass, so no element is stored twice).
//   rows:     one workgroup per (graph, pair) stores row j of the graph's matrix from the two copies' dE/dpos, divided by the
//             displacement as it was realised in fp32 and by sqrt(m m').
// Every element is stored exactly once, by one thread, from values no thread writes: no atomics, no sums, nothing to order.
#include "common.h"

namespace {

constexpr int kThreads = 64;

struct Job {
    int32_t atom, comp;                                           // atom < 0: the pair is idle
    int64_t row;                                                  // 3 f + comp
};
// job j = t pairs + c of graph g (all threads of the workgroup alike)
__device__ __forceinline__ Job job_of(const int32_t* __restrict__ fptr, const int32_t* __restrict__ free_idx, int64_t g, int64_t t,
                                      int64_t pairs, int64_t c) {
    const int64_t f0 = fptr[g], nf = (int64_t)fptr[g + 1] - f0, j = t * pairs + c;
    if (j >= 3 * nf) return Job{-1, 0, 0};
    return Job{free_idx[f0 + j / 3], (int32_t)(j % 3), j};
}

__global__ __launch_bounds__(kThreads) void vib_displace_kernel(const float* __restrict__ pos0, const int32_t* __restrict__ gptr,
                                                                const int32_t* __restrict__ fptr,
                                                                const int32_t* __restrict__ free_idx, int64_t n, int64_t pairs,
                                                                int64_t t, double delta, float* __restrict__ pos_out) {
    const int64_t g = blockIdx.x, k = blockIdx.y;
    int64_t lo = gptr[g], hi = gptr[g + 1];                       // the graph's atoms, kept inside [0, n]
    lo = lo < 0 ? 0 : lo;
    hi = hi > n ? n : hi;
    const Job job = job_of(fptr, free_idx, g, t, pairs, k >> 1);
    const int64_t hit = job.atom < 0 ? -1 : 3 * (int64_t)job.atom + job.comp;
    const double step = (k & 1) ? -delta : delta;
    float* out = pos_out + 3 * k * n;
    for (int64_t e = 3 * lo + threadIdx.x; e < 3 * hi; e += kThreads) {
        const float x = pos0[e];
        out[e] = e == hit ? (float)((double)x + step) : x;
    }
}

__global__ __launch_bounds__(kThreads) void vib_rows_kernel(const float* __restrict__ dpos, const float* __restrict__ pos0,
                                                            const float* __restrict__ masses, const int32_t* __restrict__ fptr,
                                                            const int32_t* __restrict__ free_idx, const int64_t* __restrict__ moff,
                                                            int64_t n, int64_t pairs, int64_t t, double delta,
                                                            double* __restrict__ h) {
    const int64_t g = blockIdx.x, c = blockIdx.y;
    const Job job = job_of(fptr, free_idx, g, t, pairs, c);
    if (job.atom < 0 || job.atom >= n) return;                    // idle (uniform); an index outside the batch is not followed
    const int64_t f0 = fptr[g], nf = (int64_t)fptr[g + 1] - f0, d = 3 * nf;
    const double x0 = (double)pos0[3 * (int64_t)job.atom + job.comp];
    const double sep = (double)(float)(x0 + delta) - (double)(float)(x0 - delta);   // the realised displacement
    const double ma = masses ? (double)masses[job.atom] : 1.0;
    const float* plus = dpos + 3 * (2 * c) * n;
    const float* minus = dpos + 3 * (2 * c + 1) * n;
    double* row = h + moff[g] + job.row * d;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int64_t e = threadIdx.x; e < d; e += kThreads) {
        const int64_t a = free_idx[f0 + e / 3];
        if (a < 0 || a >= n) {
            row[e] = nan;
            continue;
        }
        const int64_t at = 3 * a + e % 3;
        const double mb = masses ? (double)masses[a] : 1.0;
        row[e] = ((double)plus[at] - (double)minus[at]) / sep / sqrt(ma * mb);
    }
}

}  // namespace

static int vib_args(int64_t n, int64_t n_graphs, int64_t pairs, int64_t t, double delta) {
    if (n < 0 || n_graphs < 0 || n_graphs > 0x7fffffff || pairs < 1 || 2 * pairs > 65535 || t < 0) return PAMNET_EINVAL;
    if (!(delta > 0.0) || !(delta <= 1.79769313486231570815e+308)) return PAMNET_EINVAL;
    return PAMNET_OK;
}

extern "C" int pamnet_vib_displace_f32(const float* pos0, const int32_t* gptr, const int32_t* fptr, const int32_t* free_idx,
                                       int64_t n, int64_t n_graphs, int64_t pairs, int64_t t, double delta, float* pos_out,
                                       pamnet_stream_t stream) {
    if (vib_args(n, n_graphs, pairs, t, delta)) return PAMNET_EINVAL;
    if (!pos0 || !gptr || !fptr || !free_idx || !pos_out) return PAMNET_ENULL;
    if (n_graphs == 0 || n == 0) return PAMNET_OK;
    hipLaunchKernelGGL(vib_displace_kernel, dim3((unsigned)n_graphs, (unsigned)(2 * pairs)), dim3(kThreads), 0, as_stream(stream),
                       pos0, gptr, fptr, free_idx, n, pairs, t, delta, pos_out);
    PAMNET_LAUNCH_CHECK();
    return PAMNET_OK;
}

extern "C" int pamnet_vib_rows_f64(const float* dpos, const float* pos0, const float* masses, const int32_t* fptr,
                                   const int32_t* free_idx, const int64_t* moff, int64_t n, int64_t n_graphs, int64_t pairs,
                                   int64_t t, double delta, double* h, pamnet_stream_t stream) {
    if (vib_args(n, n_graphs, pairs, t, delta)) return PAMNET_EINVAL;
    if (!dpos || !pos0 || !fptr || !free_idx || !moff || !h) return PAMNET_ENULL;
    if (n_graphs == 0 || n == 0) return PAMNET_OK;
    hipLaunchKernelGGL(vib_rows_kernel, dim3((unsigned)n_graphs, (unsigned)pairs), dim3(kThreads), 0, as_stream(stream), dpos, pos0,
                       masses, fptr, free_idx, moff, n, pairs, t, delta, h);
    PAMNET_LAUNCH_CHECK();
    return PAMNET_OK;
}
