// Argument records of the node-chain launches (node_tail.hip), one per direction, filled by field name by the C entry points
// (pamnet_node_tail_fwd*_f32, pamnet_node_tail_main_bwd_f32, pamnet_node_pre_tail_bwd*_f32) and by the layer-stack engine.
// node_chain_fwd / node_chain_bwd check a record once -- every PAMNET_EINVAL / PAMNET_ENULL is returned before anything is
// launched -- ask the launch plan (node_tail.hip plan_fwd / plan_bwd) and launch.  Operands: see include/pamnet_hip.h.
#pragma once
#include "common.h"

#pragma GCC visibility push(hidden)
namespace node_chain {

struct NextHead {                    // the following layer's head on the x_out tile (nblk = 0: none); wp [nblk]; Zx1 nullable
    const float *Wx1, *bx1;
    const float* const* wp;
    int64_t ldwp, nblk;
    float *Zx1, *x1, *P;
};
struct MlpRider {                    // row tiles [tile0, tile0 + ntiles) of a two-layer MLP on `wgs` extra workgroups (either 0: none)
    const float* x;
    int64_t rows, tile0, ntiles, wgs;
    const float* const* mlp;         // W1 b1 W2 b2
    float* const* out;               // z1 z2 (nullable saves) y
};
struct ChainFwd {
    const float *x2, *res_x;         // x2 is written when `agg` is given
    int64_t n;
    const float *const *W, *const *b;                         // [10] each; W: matrices, or images with `packed`
    const float *w_out, *b_out, *w_att;
    float *Z, *R, *x_out, *out, *att;                         // Z, R: nullable saves; out = att = null: deferred heads
    NextHead next;
    MlpRider rider;
    const pamnet_local_agg* agg;     // nullable: x2 = the local aggregation of these operands
    int32_t packed;                  // 0 row-major matrices, 1 fp32 images, 2 bf16x3 images
    pamnet_stream_t stream;
};

struct HeadBwd {                     // backward of the next layer's head ahead of the chain, on the same row tiles (nblk 1..4)
    float* dP;                       // [nblk] planes; plane b is written where gather_src[b] is given: the segment sum of
    const float* const* gather_src;  // gather_src[b] over (gather_ptr[b], gather_perm[b]); the three and their entries nullable
    const int32_t *const *gather_ptr, *const *gather_perm;
    const float *dx1_direct, *d_add, *Wx1, *Zx1;
    const float* const* wp;
    int64_t nblk;
    float* dZx1;
};
struct ChainBwd {
    const float *d_xout, *g_head;    // d_xout nullable; with `head` null: the head's d x takes its place
    int64_t n;
    const float* const* W;           // [7]
    const float* Z;
    float *dZ, *d_x2, *d_resx;
    int32_t packed;                  // as ChainFwd's; with `head`: 1, or 2 (PAMNET_CHAIN_PIECES)
    const HeadBwd* head;             // nullable
    const void* rider;               // nullable, with `head` only: a plan of pamnet_wgrad_rider_plan_f32
    pamnet_stream_t stream;
};

int node_chain_fwd(const ChainFwd& a);
int node_chain_bwd(const ChainBwd& a);

}  // namespace node_chain
#pragma GCC visibility pop
