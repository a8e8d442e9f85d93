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

// Size bounds of the d = 128 launch plans, shared by the engine (engine.hip make_plan) and the kernels' own launchers.
constexpr int64_t NODE_TILE_ROWS = 16;          // rows per workgroup of a node-chain launch (node_tail.hip BMN)
// Row tiles up to which a node-chain launch is a single round (one workgroup per CU of the 256): the parked chain forms
// (bf16x6, segment sums / local aggregation formed by the launch's own tiles).  Above it the lean forms, which read
// their planes (node_tail.hip LEAN_FROM_TILES).
constexpr int64_t PARKED_TILES_MAX = 256;
// Global edges from which a workgroup streams enough rows (512 each) to fill its pipeline: the ping-pong edge forward
// (edge_agg.hip agg_pp) and the edge backward that forms its own weight gradients (engine.hip).
constexpr int64_t STREAMED_EDGES_FROM = 256 * 512;

// Slots of the layer-stack engine's parameter tables (pamnet_hip.h `gparams` / `lparams`; pamnet_amd/stack.py
// global_params / local_params produce them in this order).  Both engines index the tables by these names.
namespace pslot {
enum Global { G_WX1, G_BX1, G_WM, G_BM, G_WEA, G_TAIL, G_COUNT = 28 };       // mlp_x1 W b | mlp_m W [d,3d] b | W_edge_attr
enum Local {                                                                 // mlp_x1 | mlp_m_ji | mlp_m_kj | mlp_sbf 0, 1 |
    L_WX1, L_BX1, L_WJI, L_BJI, L_WKJ, L_BKJ, L_WS1, L_BS1, L_WS2, L_BS2, L_WLR, L_WLO, L_TAIL, L_COUNT = 35   // lin_rbf, lin_rbf_out
};
// the 23-pointer tail block both tables end with (fused.py tail_params): W[10], b[10], W_out.weight, W_out.bias, W
enum Tail { T_W = 0, T_B = 10, T_WOUT = 20, T_BOUT, T_WATT, T_COUNT };
static_assert(G_TAIL + T_COUNT == G_COUNT && L_TAIL + T_COUNT == L_COUNT, "parameter tables end with the tail block");
}  // namespace pslot

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

// Launchers of the narrow-width row kernels (narrow_core.h) that both the pamnet_narrow_* entry points and the narrow engine
// use, defined in narrow.hip.  Each owns its kernel's grid, block and LDS bytes; the arguments are the kernel's, with the
// width first and the stream last.  A backward kernel leaves bwd_row_grid(m, d) partial rows of n*_bwd_stride(d) floats in
// `partial` (nlinear_bwd: of `stride` floats, so that several blocks can share a row); the caller reduces them.  Not exported.
namespace narrow_rows {
int global_fwd(int d, const float* e, int64_t m, const int32_t* tgt, const int32_t* src, const float* P, const float* We,
               int ldwe, const float* bias, const float* Wea, int ldwea, float* msg, hipStream_t st);
int global_bwd(int d, const float* e, int64_t m, const int32_t* tgt, const int32_t* src, const float* P, const float* We,
               int ldwe, const float* bias, const float* Wea, int ldwea, const float* dagg, float* dz, float* de,
               float* partial, int acc_de, hipStream_t st);
int mlp2_fwd(int d, const float* x, int64_t m, const float* W1, const float* b1, const float* W2, const float* b2, int res_x,
             const float* res, float* y, hipStream_t st);
int mlp2_bwd(int d, const float* x, int64_t m, const float* W1, const float* b1, const float* W2, const float* b2,
             const float* dy, int res_x, float* dx, float* partial, int acc_dx, hipStream_t st);
int linear_bwd(int d, const float* x, int64_t m, const float* W, int ldw, const float* b, int act, const float* dy,
               int64_t lddy, float* dx, int accumulate, float* partial, int stride, hipStream_t st);
int local_gate_bwd(int d, const float* P, const float* Q, const int32_t* tgt, const int32_t* src, const float* b_ji,
                   const float* b_kj, int64_t m, const float* g_ji, const float* g_nb, float* dz, float* dQ, int zero_q3,
                   hipStream_t st);
}  // namespace narrow_rows
#pragma GCC visibility pop

__device__ __forceinline__ float silu_f(float z) { return z * __builtin_amdgcn_rcpf(1.0f + __expf(-z)); }
