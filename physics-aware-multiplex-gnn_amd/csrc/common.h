// Shared helpers for libpamnet_hip (gfx950 only; wave = 64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pamnet_hip.h"

#define PAMNET_WAVE 64

#define PAMNET_LAUNCH_CHECK()                                  \
    do {                                                       \
        hipError_t e__ = hipGetLastError();                    \
        if (e__ != hipSuccess) return (int)e__;                \
    } while (0)

// Clears the thread's sticky last-error (torch's own probing calls can leave one behind) and returns the stream.
static inline hipStream_t as_stream(pamnet_stream_t s) {
    (void)hipGetLastError();
    return reinterpret_cast<hipStream_t>(s);
}

static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// The narrow-width (d = 16 / 32 / 64) half of the pamnet_stack_* entry points, defined in narrow_engine.hip; engine.hip
// dispatches on d.  Arguments as the entry points' less those the narrow engine ignores.  Not exported.
#pragma GCC visibility push(hidden)
namespace narrow_stack {
int pack_floats(int64_t n_layer, int64_t d, int64_t* floats);
int workspace(int64_t n, int64_t eg, int64_t el, int64_t tp, int64_t n_layer, int64_t d, int64_t* saved_floats,
              int64_t* temp_floats);
int layout(int64_t n, int64_t eg, int64_t el, int64_t tp, int64_t d, int64_t* layout);
int fwd(const int64_t* sizes, const int32_t* const* graph_idx, int64_t n_layer, int64_t d, const float* x0,
        const float* e_g, const float* rbf_e, const float* e_sbf, const float* const* gparams,
        const float* const* lparams, float* saved, float* temp, float* outs, float* atts, pamnet_stream_t stream);
int bwd(const int64_t* sizes, const int32_t* const* graph_idx, int64_t n_layer, int64_t d, const float* x0,
        const float* e_g, const float* rbf_e, const float* e_sbf, const float* const* gparams,
        const float* const* lparams, const float* saved, float* temp, const float* d_outs, const float* d_atts,
        float* const* ggrads, float* const* lgrads, float* d_x0, float* d_eg, float* d_rbf, float* d_sbf,
        void* const* layer_done, pamnet_stream_t stream);
}  // namespace narrow_stack
#pragma GCC visibility pop

__device__ __forceinline__ float silu_f(float z) { return z * __builtin_amdgcn_rcpf(1.0f + __expf(-z)); }
