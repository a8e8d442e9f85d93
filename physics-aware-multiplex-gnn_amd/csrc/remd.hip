// Replica-exchange molecular dynamics (parallel tempering, Sugita & Okamoto, Chem. Phys. Lett. 314, 141, 1999): one exchange
// attempt of every temperature ladder of a batch in one launch -- pamnet_remd_exchange_f64 (include/pamnet_hip.h states the rule).
//
// A ladder is a run of consecutive graphs; an exchange swaps the TEMPERATURES two graphs hold, never their configurations: no
// position, graph or neighbour structure moves, only kT_g (which the step launch reads), the rung tables and a scale of the
// velocities.  One workgroup of 256 threads per ladder, two phases:
//   1. thread r decides the pair (r, r + 1) where r has the parity of the ladder's attempt counter: the Metropolis test, the
//      tables, kT_g, ke and the counters of its two graphs -- which no other thread touches -- and, through LDS, which graph
//      takes which velocity scale;
//   2. behind a barrier the whole workgroup strides over the atoms of every graph whose scale was set.  The loop counts (the
//      rungs of the ladder, a graph's atoms) are read from LDS and gptr by every thread alike: no thread diverges.
// No atomics and no floating-point sums: a ladder reads and writes its own entries only, so its outputs are bitwise repeatable
// and the same alone or inside any batch.
//
// The uniform number is Philox4x32-10 keyed by the ladder's seed on the counter (rung, attempt, stream 3, 0); streams 0, 1 and
// 2 belong to the thermostat, the initial velocities and the barostat (md_core.h `normals` holds the same rounds fused with its
// Box-Muller transform; the raw rounds are restated here, md_core.h keeps every statement it has).
#include "md_core.h"                              // finite (wave_sum is not needed: nothing is summed)

namespace {

constexpr int REMD_MAX_RUNGS = 256;               // the rungs of one ladder at most: one thread and one LDS entry per rung
constexpr uint32_t REMD_STREAM = 3u;

// u = (x0 + 0.5) 2^-32 of Philox4x32-10 on the counter (c0, c1, c2, 0) under the key (k0, k1): inside (0, 1)
__device__ __forceinline__ double uniform01(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2) {
    uint32_t c3 = 0u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0, c1 = l1, c2 = h0 ^ c3 ^ k1, c3 = l0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return ((double)c0 + 0.5) * (1.0 / 4294967296.0);
}

__global__ __launch_bounds__(256) void remd_exchange_kernel(
    const double* __restrict__ energy, float* __restrict__ vel, const uint8_t* __restrict__ fixed,
    const int32_t* __restrict__ gptr, const int32_t* __restrict__ lptr, const double* __restrict__ kT_ladder,
    double* __restrict__ kT_g, int32_t* __restrict__ rung, int32_t* __restrict__ slot, const int32_t* __restrict__ status,
    double* __restrict__ ke, const int64_t* __restrict__ seed_l, int32_t* __restrict__ attempts, int32_t* __restrict__ tried,
    int32_t* __restrict__ accepted, int64_t n, int64_t n_graphs) {
    __shared__ double scale_r[REMD_MAX_RUNGS];    // entry r: the velocity scale of the graph that HELD rung r ...
    __shared__ int32_t graph_r[REMD_MAX_RUNGS];   // ... and that graph; -1: nothing to scale
    const int64_t l = blockIdx.x;
    const int tid = threadIdx.x;
    int64_t lo = lptr[l], hi = lptr[l + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n_graphs ? n_graphs : hi;
    const int64_t R = hi - lo;
    if (R > REMD_MAX_RUNGS) return;               // (uniform; the entry point and the driver refuse such a ladder)
    const int32_t a = attempts[l];                // (read by every thread before thread 0 writes it, below)
    const int r = tid;
    graph_r[tid] = -1;
    __syncthreads();

    // ---- phase 1: thread r decides the pair (r, r + 1)
    if ((r & 1) == (a & 1) && r + 1 < R) {
        const int64_t i = slot[lo + r], j = slot[lo + r + 1];
        if (i >= lo && i < hi && j >= lo && j < hi && i != j && status[i] == 0 && status[j] == 0) {
            const double ei = energy[i], ej = energy[j];
            if (finite(ei) && finite(ej)) {                       // step 1: else the pair is skipped
                const double kr = kT_ladder[lo + r], kq = kT_ladder[lo + r + 1];
                const double delta = (1.0 / kr - 1.0 / kq) * (ei - ej);       // step 2
                tried[lo + r] += 1;
                bool accept = delta >= 0.0;
                if (!accept) {
                    const uint64_t seed = (uint64_t)seed_l[l];
                    accept = uniform01((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)r, (uint32_t)a, REMD_STREAM) < exp(delta);
                }
                if (accept) {                                     // step 3
                    slot[lo + r] = (int32_t)j, slot[lo + r + 1] = (int32_t)i;
                    rung[i] = r + 1, rung[j] = r;
                    kT_g[i] = kq, kT_g[j] = kr;
                    accepted[lo + r] += 1;
                    ke[i] *= kq / kr, ke[j] *= kr / kq;
                    graph_r[r] = (int32_t)i, scale_r[r] = sqrt(kq / kr);
                    graph_r[r + 1] = (int32_t)j, scale_r[r + 1] = sqrt(kr / kq);
                }
            }
        }
    }
    if (tid == 0) attempts[l] = a + 1;                            // step 4
    __syncthreads();

    // ---- phase 2: the velocities of the graphs that changed their temperature (an atom is read and written by one thread)
    for (int q = 0; q < (int)R; ++q) {
        const int32_t g = graph_r[q];
        if (g < 0) continue;                                      // (uniform: every thread reads the same entry)
        const double s = scale_r[q];
        int64_t alo = gptr[g], ahi = gptr[g + 1];
        alo = alo < 0 ? 0 : alo;
        ahi = ahi > n ? n : ahi;
        for (int64_t at = alo + tid; at < ahi; at += 256) {
            if (fixed && fixed[at]) continue;
            vel[3 * at] = (float)((double)vel[3 * at] * s);
            vel[3 * at + 1] = (float)((double)vel[3 * at + 1] * s);
            vel[3 * at + 2] = (float)((double)vel[3 * at + 2] * s);
        }
    }
}

}  // namespace

extern "C" int pamnet_remd_exchange_f64(const double* energy, float* vel, const uint8_t* fixed, const int32_t* gptr,
                                        const int32_t* lptr, const double* kT_ladder, double* kT_g, int32_t* rung,
                                        int32_t* slot, const int32_t* status, double* ke, const int64_t* seed,
                                        int32_t* attempts, int32_t* tried, int32_t* accepted, int64_t n, int64_t n_graphs,
                                        int64_t n_ladders, pamnet_stream_t stream) {
    if (n < 0 || n_graphs < 0 || n_ladders < 0 || n_graphs > 0x7fffffff || n_ladders > 0x7fffffff) return PAMNET_EINVAL;
    if (!energy || !vel || !gptr || !lptr || !kT_ladder || !kT_g || !rung || !slot || !status || !ke || !seed || !attempts ||
        !tried || !accepted)
        return PAMNET_ENULL;
    if (n_ladders == 0) return PAMNET_OK;
    // lptr lives on the device and is not read here: what the counts alone prove is refused -- n_ladders ladders of at most
    // REMD_MAX_RUNGS rungs cannot hold more graphs than this
    if (n_graphs > n_ladders * (int64_t)REMD_MAX_RUNGS) return PAMNET_EINVAL;
    hipLaunchKernelGGL(remd_exchange_kernel, dim3((unsigned)n_ladders), dim3(256), 0, as_stream(stream), energy, vel, fixed, gptr,
                       lptr, kT_ladder, kT_g, rung, slot, status, ke, seed, attempts, tried, accepted, n, n_graphs);
    PAMNET_LAUNCH_CHECK();
    return PAMNET_OK;
}
