// Layer-stack engine for the narrow widths (dim = 16 / 32 / 64: the reference's RNA configurations,
// inference_rna_puzzles.py:29-30, main_rna_puzzles.py:52-53): the n_layer x (global, local) loop of PAMNet.forward
// (models.py:196-204) as ONE call per direction, the counterpart of engine.hip for dim = 128: pamnet_stack_* (engine.hip)
// dispatches here on d.
//
// Per layer the node-side chains are single launches (narrow_chain.h), the edge / triplet-row work uses the row kernels
// of narrow_core.h, every weight gradient goes from the kernels' partial rows straight into the caller's gradient
// buffers (column blocks of the 3d-wide message weights included), and gradients of the tensors that feed every layer
// (e_g, rbf_e, e_sbf) are accumulated inside the kernels that produce them.  Against the per-operator path this removes
// the host work of ~50 autograd nodes per layer pair (the d = 16 step was bound by it) and ~70 % of the launches.
//
// Forward, global layer k (layers/global_message_passing.py:33-56):
//   npre_fwd      x -> x1 = SiLU(mlp_x1 x), P = [W_i x1 | W_j x1]
//   nglobal_fwd   msg = SiLU(P_i[tgt] + P_j[src] + W_e e + b) * (W_ea e)          (E_g rows)
//   segment_sum   x2 = x1 + sum_{e -> i} msg
//   ntail_fwd     x2, x -> x_out, out, att
// local layer k (layers/local_message_passing.py:36-66):
//   npre_fwd      x -> x1, P = [ji_i | kj_i | ji_j | kj_j]
//   npre_fwd      rbf_e -> Q = [ji_e | kj_e | lin_rbf | lin_rbf_out]               (E_l rows, no first layer)
//   nlocal_gate   m_ji = SiLU(..), m_nb = SiLU(..) * Q_2
//   nmlp2_fwd     s = mlp_sbf(e_sbf)                                               (T+P rows)
//   segment_sum   m_other = sum_{rows of edge} m_nb[col] * s
//   nlocal_msg    m = Q_3 * (m_ji + m_other);  segment_sum x2 = x1 + sum m;  ntail_fwd
// The backward runs the same list in reverse with the backward kernels.
#include "narrow_chain.h"

namespace {

#define TRY(x)                              \
    do {                                    \
        const int rc_ = (x);                \
        if (rc_ != PAMNET_OK) return rc_;   \
    } while (0)

// m = Q[:, 3d:4d] * (m_ji + m_other)   (local_message_passing.py:53), one float4 per thread
__global__ __launch_bounds__(256) void nlocal_msg_fwd_kernel(const float4* __restrict__ Q, const float4* __restrict__ m_ji,
                                                             const float4* __restrict__ m_other, int64_t el, int d4,
                                                             float4* __restrict__ msg) {
    const int64_t total = el * d4;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int64_t q = t / d4;
        const int c = (int)(t - q * d4);
        const float4 g = Q[q * (4 * d4) + 3 * d4 + c], a = m_ji[t], b = m_other[t];
        msg[t] = make_float4(g.x * (a.x + b.x), g.y * (a.y + b.y), g.z * (a.z + b.z), g.w * (a.w + b.w));
    }
}

// gm = d_x2[tgt[q]];  dQ[:, 3d:4d] = gm * (m_ji + m_other);  dmm = gm * Q[:, 3d:4d]  (= d m_ji = d m_other)
__global__ __launch_bounds__(256) void nlocal_msg_bwd_kernel(const float4* __restrict__ d_x2, const int32_t* __restrict__ tgt,
                                                             const float4* __restrict__ Q, const float4* __restrict__ m_ji,
                                                             const float4* __restrict__ m_other, int64_t el, int d4,
                                                             float4* __restrict__ dQ, float4* __restrict__ dmm) {
    const int64_t total = el * d4;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int64_t q = t / d4;
        const int c = (int)(t - q * d4);
        const float4 gm = d_x2[(int64_t)tgt[q] * d4 + c];
        const float4 g = Q[q * (4 * d4) + 3 * d4 + c], a = m_ji[t], b = m_other[t];
        dQ[q * (4 * d4) + 3 * d4 + c] = make_float4(gm.x * (a.x + b.x), gm.y * (a.y + b.y), gm.z * (a.z + b.z), gm.w * (a.w + b.w));
        dmm[t] = make_float4(gm.x * g.x, gm.y * g.y, gm.z * g.z, gm.w * g.w);
    }
}

// ---- launches: take the kernel's partial rows from the Reducer, launch, register where the rows' segments are summed to ----
int launch_tail_fwd(int d, const NTailFwd& p, hipStream_t st) {
    if (p.m == 0) return PAMNET_OK;
    return narrow_dispatch(d, [&](auto D) {
        return narrow_launch(ntail_fwd_kernel<D>, chain_grid(p.m), 64 * CHW, ntail_fwd_lds<D>(), st, p);
    });
}

inline int tail_stride(int d) { return d == 16 ? TailRow<16>::STRIDE : (d == 32 ? TailRow<32>::STRIDE : TailRow<64>::STRIDE); }

// gW / gb: 10 + 10 gradient buffers in chain order, head gradients gw_out [d], gb_out [1], gw_att [d]
int launch_tail_bwd(int d, NTailBwd p, float* const* gW, float* const* gb, float* gw_out, float* gb_out, float* gw_att,
                    Reducer& R, hipStream_t st) {
    if (p.m == 0) return PAMNET_EINVAL;
    const int grid = chain_grid(p.m);
    p.stride = tail_stride(d);
    TRY(R.take(grid, p.stride, 23, &p.partial));
    TRY(narrow_dispatch(d, [&](auto D) {
        return narrow_launch(ntail_bwd_kernel<D>, grid, 64 * CHW, ntail_bwd_lds<D>(), st, p);
    }));
    const int MAT = d * d, LIN = MAT + d, MLP = 2 * MAT + 2 * d;
    SegTable& T = R.T;
    T.mat(gW[0], 0, d, d, d, d);
    T.vec(gb[0], MAT, d);
    for (int k = 0; k < 4; ++k) {
        const int off = LIN + k * MLP;
        T.mat(gW[2 + 2 * k], off, d, d, d, d);                 // segment layout: [dW2][db2][dW1][db1]
        T.vec(gb[2 + 2 * k], off + MAT, d);
        T.mat(gW[1 + 2 * k], off + LIN, d, d, d, d);
        T.vec(gb[1 + 2 * k], off + LIN + MAT, d);
    }
    const int l5 = LIN + 4 * MLP;
    T.mat(gW[9], l5, d, d, d, d);
    T.vec(gb[9], l5 + MAT, d);
    const int h = l5 + LIN;
    T.vec(gw_out, h, d);
    T.vec(gw_att, h + d, d);
    T.vec(gb_out, h + 2 * d, 1);
    return PAMNET_OK;
}

int launch_pre_fwd(int d, const NPreFwd& p, hipStream_t st) {
    if (p.m == 0) return PAMNET_OK;
    return narrow_dispatch(d, [&](auto D) {
        return narrow_launch(npre_fwd_kernel<D>, fwd_row_grid(p.m, D), NWG, npre_fwd_lds<D>(), st, p);
    });
}

// gWp[k]: gradient destination of projection block k (row stride ldg[k]); gW1 [d, d], gb1 [d]
int launch_pre_bwd(int d, NPreBwd p, float* const* gWp, const int* ldg, float* gW1, float* gb1, Reducer& R, hipStream_t st) {
    if (p.m == 0) return PAMNET_EINVAL;
    const int grid = chain_grid(p.m);
    const int MAT = d * d;
    p.stride = npre_bwd_stride(d, p.nb);
    TRY(R.take(grid, p.stride, p.nb + 2, &p.partial));
    TRY(narrow_dispatch(d, [&](auto D) {
        return narrow_launch(npre_bwd_kernel<D>, grid, 64 * CHW, npre_bwd_lds<D>(), st, p);
    }));
    SegTable& T = R.T;
    for (int k = 0; k < p.nb; ++k) T.mat(gWp[k], k * MAT, d, d, d, ldg[k]);
    T.mat(gW1, p.nb * MAT, d, d, d, d);
    T.vec(gb1, (p.nb + 1) * MAT, d);
    return PAMNET_OK;
}

int launch_global_bwd(int d, const float* e, int64_t m, const int32_t* tgt, const int32_t* src, const float* P,
                      const float* We, int ldwe, const float* bias, const float* Wea, int ldwea, const float* dagg,
                      float* dz, float* de, int acc_de, Reducer& R, float* gWe, int ldgwe, float* gWea, float* gb,
                      hipStream_t st) {
    float* partial = nullptr;
    TRY(R.take(bwd_row_grid(m, d), nglobal_bwd_stride(d), 3, &partial));
    TRY(narrow_rows::global_bwd(d, e, m, tgt, src, P, We, ldwe, bias, Wea, ldwea, dagg, dz, de, partial, acc_de, st));
    SegTable& T = R.T;
    T.mat(gWe, 0, d, d, d, ldgwe);
    T.mat(gWea, d * d, d, d, d, d);
    T.vec(gb, 2 * d * d, d);
    return PAMNET_OK;
}

int launch_mlp2_bwd(int d, const float* x, int64_t m, const float* W1, const float* b1, const float* W2, const float* b2,
                    const float* dy, float* dx, int acc_dx, Reducer& R, float* gW1, float* gb1, float* gW2, float* gb2,
                    hipStream_t st) {
    float* partial = nullptr;
    TRY(R.take(bwd_row_grid(m, d), nmlp2_bwd_stride(d), 4, &partial));
    TRY(narrow_rows::mlp2_bwd(d, x, m, W1, b1, W2, b2, dy, 0, dx, partial, acc_dx, st));
    SegTable& T = R.T;
    T.mat(gW1, 0, d, d, d, d);
    T.mat(gW2, d * d, d, d, d, d);
    T.vec(gb1, 2 * d * d, d);
    T.vec(gb2, 2 * d * d + d, d);
    return PAMNET_OK;
}

// The four bias-free projection blocks of the edge-side Q = rbf [W_0 | W_1 | W_2 | W_3]^T: dW_k and (blocks whose gradient
// is the pre-activation gradient of a biased layer) the bias gradient = column sums of dQ_k; d rbf accumulated unless
// `overwrite`.  The blocks' partial rows interleave so that one reduce serves all: gW[k] (row stride ldg[k]), gb[k] nullable.
int launch_qblocks_bwd(int d, const float* rbf, int64_t m, const float* const* W, const int* ldw, const float* dQ,
                       float* d_rbf, bool overwrite, Reducer& R, float* const* gW, const int* ldg, float* const* gb,
                       hipStream_t st) {
    const int qs = nlinear_bwd_stride(d), stride = nqblock4_bwd_stride(d);
    float* partial = nullptr;
    TRY(R.take(bwd_row_grid(m, d), stride, 6, &partial));
    TRY(narrow_dispatch(d, [&](auto D) {
        if constexpr (D <= 32) {                              // one pass over the rows for the four blocks (narrow_core.h)
            return narrow_launch(nqblock4_bwd_kernel<D>, bwd_row_grid(m, D), 64 * lin_bwd_waves(D), nqblock4_bwd_lds<D>(), st,
                                 rbf, m, W[0], W[1], W[2], W[3], ldw[0], ldw[1], ldw[2], ldw[3], dQ, 4 * D, d_rbf,
                                 overwrite ? 0 : 1, partial, stride);
        } else {
            for (int b = 0; b < 4; ++b)
                TRY(narrow_rows::linear_bwd(D, rbf, m, W[b], ldw[b], nullptr, 0, dQ + b * D, 4 * D, d_rbf,
                                            (overwrite && b == 0) ? 0 : 1, partial + b * qs, stride, st));
            return PAMNET_OK;
        }
    }));
    SegTable& T = R.T;
    for (int b = 0; b < 4; ++b) {
        T.mat(gW[b], b * qs, d, d, d, ldg[b]);
        T.vec(gb[b], b * qs + d * d, d);
    }
    return PAMNET_OK;
}

// ---- arenas ------------------------------------------------------------------------------------------------------------
inline int64_t up64(int64_t v) { return (v + 63) & ~(int64_t)63; }

struct Lay {
    int64_t n, eg, el, tp, d;
    // saved, per layer pair (g_t / l_t: what the tail chain of the global / local layer reads and saves)
    struct Tail {
        int64_t x2, H0, R1, R2, R3, T, O;
    };
    int64_t g_x1, g_P, l_x1, l_P, l_Q, l_mji, l_mnb, l_mother, l_s;
    Tail g_t, l_t;
    int64_t pair;
    // temp
    int64_t t_msg, t_dz, t_ds, t_dQ, t_dzl, t_dmm, t_dmnb, t_dpi, t_dpj, t_dx2, t_dresx, t_gx0, t_gx1, t_partial, t_pack, temp;
    int64_t partial_floats;
};

Lay make_layout(int64_t n, int64_t eg, int64_t el, int64_t tp, int64_t d, int64_t n_layer = 1) {
    Lay L;
    L.n = n, L.eg = eg, L.el = el, L.tp = tp, L.d = d;
    int64_t o = 0;
    auto take = [&](int64_t floats) {
        const int64_t at = o;
        o += up64(floats);
        return at;
    };
    const int64_t nd = n * d;
    auto take_tail = [&](Lay::Tail& t) {
        t.x2 = take(nd), t.H0 = take(nd), t.R1 = take(nd), t.R2 = take(nd), t.R3 = take(nd), t.T = take(nd), t.O = take(nd);
    };
    L.g_x1 = take(nd), L.g_P = take(2 * nd), take_tail(L.g_t);
    L.l_x1 = take(nd), L.l_P = take(4 * nd), take_tail(L.l_t);
    L.l_Q = take(4 * el * d), L.l_mji = take(el * d), L.l_mnb = take(el * d), L.l_mother = take(el * d), L.l_s = take(tp * d);
    L.pair = o;
    o = 0;
    const int64_t big = eg > el ? eg : el;
    L.t_msg = take(big * d);                 // forward: messages of the layer being aggregated
    L.t_dz = take(eg * d), L.t_ds = take(tp * d), L.t_dQ = take(4 * el * d), L.t_dzl = take(2 * el * d);
    L.t_dmm = take(el * d), L.t_dmnb = take(el * d), L.t_dpi = take(2 * nd), L.t_dpj = take(2 * nd);
    L.t_dx2 = take(nd), L.t_dresx = take(nd), L.t_gx0 = take(nd), L.t_gx1 = take(nd);
    const int64_t chain = (int64_t)chain_grid(n) * tail_stride((int)d);
    const int64_t pre = (int64_t)chain_grid(n) * npre_bwd_stride((int)d, NPB);
    const int64_t erow = (int64_t)NARROW_BLOCKS * nmlp2_bwd_stride((int)d);
    const int64_t qb = (int64_t)NARROW_BLOCKS * nqblock4_bwd_stride((int)d);
    static_assert(nglobal_bwd_stride(64) <= nmlp2_bwd_stride(64), "the global row kernel's rows fit an `erow`");
    // every backward kernel of a layer pair keeps its partial rows until the pair's reductions run (Reducer): two chain
    // tails, two heads, the global row kernel, the triplet / pair MLP and the four projection blocks
    const int64_t pf = 2 * (chain + 64) + 2 * (pre + 64) + 2 * (erow + 64) + (qb + 64);
    L.partial_floats = pf;
    L.t_partial = take(pf);
    L.t_pack = take(n_layer * 2 * PACK_SLOTS * d * d);       // weight images of every layer pair (npack_kernel)
    L.temp = o;
    return L;
}

struct Idx {
    const int32_t *g_ptr, *g_row, *g_col, *gT_ptr, *gT_perm, *l_ptr, *l_row, *l_col, *lT_ptr, *lT_perm, *tp_ptr, *tp_row,
        *tp_col, *tpT_ptr, *tpT_perm;
};

inline Idx make_idx(const int32_t* const* g) {
    return Idx{g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[8], g[9], g[10], g[11], g[12], g[13], g[14]};
}

namespace ps = pslot;                     // slots of the parameter / gradient tables (common.h)

// slots of a layer pair's [d, d] weight blocks in the packed-image area
enum Slot { G_W1 = 0, G_P = 1, G_TAIL = 3, L_W1 = 13, L_P = 14, L_Q = 18, L_TAIL = 22 };

struct Images {
    const float* base;
    int d;
    const float4* at(int64_t pair, int slot, int transposed) const {
        return reinterpret_cast<const float4*>(base + ((pair * PACK_SLOTS + slot) * 2 + transposed) * (int64_t)d * d);
    }
};

int pack_all(int d, int64_t n_layer, const float* const* gparams, const float* const* lparams, float* out, hipStream_t st) {
    for (int64_t k = 0; k < n_layer; ++k) {
        const float* const* g = gparams + k * ps::G_COUNT;
        const float* const* l = lparams + k * ps::L_COUNT;
        PackJobs J;
        auto set = [&](int slot, const float* W, int ld) { J.W[slot] = W, J.ld[slot] = ld; };
        set(G_W1, g[ps::G_WX1], d), set(G_P, g[ps::G_WM], 3 * d), set(G_P + 1, g[ps::G_WM] + d, 3 * d);
        for (int i = 0; i < 10; ++i) set(G_TAIL + i, g[ps::G_TAIL + i], d), set(L_TAIL + i, l[ps::L_TAIL + i], d);
        set(L_W1, l[ps::L_WX1], d);
        set(L_P, l[ps::L_WJI], 3 * d), set(L_P + 1, l[ps::L_WKJ], 3 * d);
        set(L_P + 2, l[ps::L_WJI] + d, 3 * d), set(L_P + 3, l[ps::L_WKJ] + d, 3 * d);
        set(L_Q, l[ps::L_WJI] + 2 * d, 3 * d), set(L_Q + 1, l[ps::L_WKJ] + 2 * d, 3 * d);
        set(L_Q + 2, l[ps::L_WLR], d), set(L_Q + 3, l[ps::L_WLO], d);
        float4* dst = reinterpret_cast<float4*>(out + k * 2 * PACK_SLOTS * (int64_t)d * d);
        TRY(narrow_dispatch(d, [&](auto D) { return narrow_launch(npack_kernel<D>, dim3(PACK_SLOTS, 2), 256, 0, st, J, dst); }));
    }
    return PAMNET_OK;
}

// the tail chain of one layer: parameters `tp` (the table's tail block), images from slot0 on, saved tensors at S + o.*
inline NTailFwd tail_fwd_params(const float* const* tp, const Images& im, int64_t pair, int slot0, float* S, const Lay::Tail& o) {
    NTailFwd t = {};
    for (int i = 0; i < 10; ++i) t.img[i] = im.at(pair, slot0 + i, 0), t.b[i] = tp[ps::T_B + i];
    t.w_out = tp[ps::T_WOUT], t.b_out = tp[ps::T_BOUT], t.w_att = tp[ps::T_WATT];
    t.x2 = S + o.x2, t.H0 = S + o.H0, t.R1 = S + o.R1, t.R2 = S + o.R2, t.R3 = S + o.R3, t.T = S + o.T, t.O = S + o.O;
    return t;
}

inline NTailBwd tail_bwd_params(const float* const* tp, const Images& im, int64_t pair, int slot0, const float* S,
                                const Lay::Tail& o) {
    NTailBwd t = {};
    for (int i = 0; i < 10; ++i)
        t.img[i] = im.at(pair, slot0 + i, 0), t.imgt[i] = im.at(pair, slot0 + i, 1), t.b[i] = tp[ps::T_B + i];
    t.w_out = tp[ps::T_WOUT], t.w_att = tp[ps::T_WATT];
    t.x2 = S + o.x2, t.H0 = S + o.H0, t.R1 = S + o.R1, t.R2 = S + o.R2, t.R3 = S + o.R3, t.T = S + o.T, t.O = S + o.O;
    return t;
}

}  // namespace

// ---- the narrow-width half of the pamnet_stack_* entry points (engine.hip dispatches here for d != 128) --------------

// the weight images live inside `temp`: no `wpack` arena
int narrow_stack::pack_floats(int64_t n_layer, int64_t d, int64_t* floats) {
    if (n_layer < 1 || !floats || !width_ok(d)) return PAMNET_EINVAL;
    *floats = 0;
    return PAMNET_OK;
}

int narrow_stack::workspace(int64_t n, int64_t eg, int64_t el, int64_t tp, int64_t n_layer, int64_t d,
                            int64_t* saved_floats, int64_t* temp_floats) {
    if (n < 0 || eg < 0 || el < 0 || tp < 0 || n_layer < 1 || !width_ok(d)) return PAMNET_EINVAL;
    if (!saved_floats || !temp_floats) return PAMNET_ENULL;
    const Lay L = make_layout(n, eg, el, tp, d, n_layer);
    *saved_floats = L.pair * n_layer;
    *temp_floats = L.temp;
    return PAMNET_OK;
}

// layout[0] = floats per layer pair in `saved`; [1], [2] = offsets of the global / local layer's node output in a pair
int narrow_stack::layout(int64_t n, int64_t eg, int64_t el, int64_t tp, int64_t d, int64_t* layout) {
    if (!width_ok(d)) return PAMNET_EINVAL;
    if (!layout) return PAMNET_ENULL;
    const Lay L = make_layout(n, eg, el, tp, d);
    layout[0] = L.pair, layout[1] = L.g_t.R3, layout[2] = L.l_t.R3;
    return PAMNET_OK;
}

int narrow_stack::fwd(const int64_t* sizes, const int32_t* const* graph_idx, int64_t n_layer, int64_t d, const float* x0,
                      const float* e_g, const float* rbf_e, const float* e_sbf, const float* const* gparams,
                      const float* const* lparams, float* saved, float* temp, float* outs, float* atts,
                      pamnet_stream_t stream) {
    if (!sizes || !graph_idx || !gparams || !lparams) return PAMNET_ENULL;
    const int64_t n = sizes[0], eg = sizes[1], el = sizes[2], tp = sizes[3];
    if (n < 0 || eg < 0 || el < 0 || tp < 0 || n_layer < 1 || !width_ok(d)) return PAMNET_EINVAL;
    if (n == 0) return PAMNET_OK;
    if (!x0 || !saved || !temp || !outs || !atts || (eg > 0 && !e_g) || (el > 0 && !rbf_e) || (tp > 0 && !e_sbf)) return PAMNET_ENULL;
    const Lay L = make_layout(n, eg, el, tp, d, n_layer);
    const Idx ix = make_idx(graph_idx);
    hipStream_t st = as_stream(stream);
    const int D = (int)d;
    TRY(pack_all(D, n_layer, gparams, lparams, temp + L.t_pack, st));
    const Images im{temp + L.t_pack, D};
    const float* x = x0;
    for (int64_t k = 0; k < n_layer; ++k) {
        float* S = saved + k * L.pair;
        const float* const* g = gparams + k * ps::G_COUNT;
        const float* const* l = lparams + k * ps::L_COUNT;
        // ---------------- global layer
        {
            NPreFwd p = {};
            p.x = x, p.img1 = im.at(k, G_W1, 0), p.b1 = g[ps::G_BX1], p.nb = 2, p.imgp[0] = im.at(k, G_P, 0), p.imgp[1] = im.at(k, G_P + 1, 0);
            p.x1 = S + L.g_x1, p.P = S + L.g_P, p.m = n;
            TRY(launch_pre_fwd(D, p, st));
            TRY(narrow_rows::global_fwd(D, e_g, eg, ix.g_row, ix.g_col, S + L.g_P, g[ps::G_WM] + 2 * D, 3 * D, g[ps::G_BM],
                                        g[ps::G_WEA], D, temp + L.t_msg, st));
            TRY(pamnet_segment_sum_f32(S + L.g_t.x2, S + L.g_x1, temp + L.t_msg, nullptr, nullptr, nullptr, nullptr, ix.g_ptr, n,
                                       d, stream));
            NTailFwd t = tail_fwd_params(g + ps::G_TAIL, im, k, G_TAIL, S, L.g_t);
            t.res_x = x, t.out = outs + (2 * k) * n, t.att = atts + (2 * k) * n, t.m = n;
            TRY(launch_tail_fwd(D, t, st));
            x = S + L.g_t.R3;
        }
        // ---------------- local layer
        {
            NPreFwd p = {};
            p.x = x, p.img1 = im.at(k, L_W1, 0), p.b1 = l[ps::L_BX1], p.nb = 4, p.m = n, p.x1 = S + L.l_x1, p.P = S + L.l_P;
            for (int b = 0; b < 4; ++b) p.imgp[b] = im.at(k, L_P + b, 0);
            TRY(launch_pre_fwd(D, p, st));
            NPreFwd q = {};
            q.x = rbf_e, q.nb = 4, q.m = el, q.P = S + L.l_Q;
            for (int b = 0; b < 4; ++b) q.imgp[b] = im.at(k, L_Q + b, 0);
            TRY(launch_pre_fwd(D, q, st));
            TRY(pamnet_narrow_local_gate_fwd_f32(S + L.l_P, S + L.l_Q, ix.l_row, ix.l_col, l[ps::L_BJI], l[ps::L_BKJ], el, d, S + L.l_mji,
                                                 S + L.l_mnb, stream));
            TRY(narrow_rows::mlp2_fwd(D, e_sbf, tp, l[ps::L_WS1], l[ps::L_BS1], l[ps::L_WS2], l[ps::L_BS2], 0, nullptr, S + L.l_s,
                                      st));
            TRY(pamnet_segment_sum_f32(S + L.l_mother, nullptr, S + L.l_mnb, ix.tp_col, S + L.l_s, nullptr, nullptr, ix.tp_ptr,
                                       el, d, stream));
            if (el > 0)
                TRY(narrow_launch(nlocal_msg_fwd_kernel, ew_grid(el * (d / 4)), 256, 0, st, (const float4*)(S + L.l_Q),
                                  (const float4*)(S + L.l_mji), (const float4*)(S + L.l_mother), el, d / 4,
                                  (float4*)(temp + L.t_msg)));
            TRY(pamnet_segment_sum_f32(S + L.l_t.x2, S + L.l_x1, temp + L.t_msg, nullptr, nullptr, nullptr, nullptr, ix.l_ptr, n,
                                       d, stream));
            NTailFwd t = tail_fwd_params(l + ps::L_TAIL, im, k, L_TAIL, S, L.l_t);
            t.res_x = x, t.out = outs + (2 * k + 1) * n, t.att = atts + (2 * k + 1) * n, t.m = n;
            TRY(launch_tail_fwd(D, t, st));
            x = S + L.l_t.R3;
        }
    }
    return PAMNET_OK;
}

int narrow_stack::bwd(const int64_t* sizes, const int32_t* const* graph_idx, int64_t n_layer, int64_t d, const float* x0,
                      const float* e_g, const float* rbf_e, const float* e_sbf, const float* const* gparams,
                      const float* const* lparams, const float* saved, float* temp, const float* d_outs,
                      const float* d_atts, float* const* ggrads, float* const* lgrads, float* d_x0, float* d_eg,
                      float* d_rbf, float* d_sbf, void* const* layer_done, pamnet_stream_t stream) {
    if (!sizes || !graph_idx || !gparams || !lparams || !ggrads || !lgrads) return PAMNET_ENULL;
    const int64_t n = sizes[0], eg = sizes[1], el = sizes[2], tp = sizes[3];
    if (n <= 0 || eg <= 0 || el <= 0 || tp <= 0 || n_layer < 1 || !width_ok(d)) return PAMNET_EINVAL;   // (empty parts: the
    //                                                     caller zero-fills; a batch without edges has nothing to train on)
    if (!x0 || !e_g || !rbf_e || !e_sbf || !saved || !temp || !d_outs || !d_atts || !d_x0 || !d_eg || !d_rbf || !d_sbf)
        return PAMNET_ENULL;
    const Lay L = make_layout(n, eg, el, tp, d, n_layer);
    const Idx ix = make_idx(graph_idx);
    hipStream_t st = as_stream(stream);
    const int D = (int)d;
    TRY(pack_all(D, n_layer, gparams, lparams, temp + L.t_pack, st));
    const Images im{temp + L.t_pack, D};
    Reducer R(temp + L.t_partial, L.partial_floats, st);    // partial rows of the backward kernels: reduced a few kernels at a time
    float* d_x2 = temp + L.t_dx2;
    float* d_resx = temp + L.t_dresx;
    float* gx[2] = {temp + L.t_gx0, temp + L.t_gx1};
    const float* g_x = nullptr;              // gradient w.r.t. the node output of the layer being differentiated
    for (int64_t k = n_layer - 1; k >= 0; --k) {
        const float* S = saved + k * L.pair;
        const float* const* g = gparams + k * ps::G_COUNT;
        const float* const* l = lparams + k * ps::L_COUNT;
        float* const* gg = ggrads + k * ps::G_COUNT;
        float* const* lg = lgrads + k * ps::L_COUNT;
        const bool first = k == n_layer - 1;                 // first layer pair to be differentiated: overwrite d e_*
        const float* x_glob = k == 0 ? x0 : saved + (k - 1) * L.pair + L.l_t.R3;       // input of global layer k
        const float* x_loc = S + L.g_t.R3;                                              // input of local layer k
        // ---------------- local layer
        {
            NTailBwd t = tail_bwd_params(l + ps::L_TAIL, im, k, L_TAIL, S, L.l_t);
            t.g_x = g_x, t.g_out = d_outs + (2 * k + 1) * n, t.g_att = d_atts + (2 * k + 1) * n;
            t.d_x2 = d_x2, t.d_resx = d_resx, t.m = n;
            float* const* lt = lg + ps::L_TAIL;
            TRY(launch_tail_bwd(D, t, lt, lt + ps::T_B, lt[ps::T_WOUT], lt[ps::T_BOUT], lt[ps::T_WATT], R, st));
            // x2 = x1 + sum m,  m = Q_3 (m_ji + m_other)
            float* dQ = temp + L.t_dQ;
            float* dmm = temp + L.t_dmm;
            TRY(narrow_launch(nlocal_msg_bwd_kernel, ew_grid(el * (d / 4)), 256, 0, st, (const float4*)d_x2, ix.l_row,
                              (const float4*)(S + L.l_Q), (const float4*)(S + L.l_mji), (const float4*)(S + L.l_mother), el,
                              d / 4, (float4*)dQ, (float4*)dmm));
            // m_other[r] = sum_{q in row r} m_nb[col q] * s[q]
            float* ds = temp + L.t_ds;
            float* dmnb = temp + L.t_dmnb;
            TRY(pamnet_gather_mul_f32(ds, S + L.l_mnb, ix.tp_col, dmm, ix.tp_row, tp, d, stream));
            TRY(pamnet_segment_sum_f32(dmnb, nullptr, S + L.l_s, nullptr, dmm, ix.tp_row, ix.tpT_perm, ix.tpT_ptr, el, d, stream));
            TRY(launch_mlp2_bwd(D, e_sbf, tp, l[ps::L_WS1], l[ps::L_BS1], l[ps::L_WS2], l[ps::L_BS2], ds, d_sbf, first ? 0 : 1, R,
                                lg[ps::L_WS1], lg[ps::L_BS1], lg[ps::L_WS2], lg[ps::L_BS2], st));
            // gates: dz_l [el, 2d] and dQ blocks 0..2 (block 3 is already there)
            float* dzl = temp + L.t_dzl;
            TRY(narrow_rows::local_gate_bwd(D, S + L.l_P, S + L.l_Q, ix.l_row, ix.l_col, l[ps::L_BJI], l[ps::L_BKJ], el, dmm, dmnb,
                                            dzl, dQ, 0, st));
            // node side: d P_i over the edges into i, d P_j over the edges out of j
            float* dpi = temp + L.t_dpi;
            float* dpj = temp + L.t_dpj;
            TRY(pamnet_segment_sum_f32(dpi, nullptr, dzl, nullptr, nullptr, nullptr, nullptr, ix.l_ptr, n, 2 * d, stream));
            TRY(pamnet_segment_sum_f32(dpj, nullptr, dzl, nullptr, nullptr, nullptr, ix.lT_perm, ix.lT_ptr, n, 2 * d, stream));
            // edge side: the four projection blocks of Q (d b_ji, d b_kj = column sums of d z_ji, d z_kj)
            const float* Wq[4] = {l[ps::L_WJI] + 2 * D, l[ps::L_WKJ] + 2 * D, l[ps::L_WLR], l[ps::L_WLO]};
            float* const gWq[4] = {lg[ps::L_WJI] + 2 * D, lg[ps::L_WKJ] + 2 * D, lg[ps::L_WLR], lg[ps::L_WLO]};
            float* const gbq[4] = {lg[ps::L_BJI], lg[ps::L_BKJ], nullptr, nullptr};
            const int ldq[4] = {3 * D, 3 * D, D, D};
            TRY(launch_qblocks_bwd(D, rbf_e, el, Wq, ldq, dQ, d_rbf, first, R, gWq, ldq, gbq, st));
            NPreBwd p = {};
            p.x = x_loc, p.x1 = S + L.l_x1, p.img1 = im.at(k, L_W1, 0), p.img1t = im.at(k, L_W1, 1), p.b1 = l[ps::L_BX1], p.nb = 4, p.m = n;
            for (int b = 0; b < 4; ++b) p.imgpt[b] = im.at(k, L_P + b, 1);
            p.dP[0] = dpi, p.dP[1] = dpi + D, p.dP[2] = dpj, p.dP[3] = dpj + D;
            p.lddp[0] = p.lddp[1] = p.lddp[2] = p.lddp[3] = 2 * D;
            p.d_direct = d_x2, p.d_add = d_resx, p.dx = gx[0];
            float* gWp[4] = {lg[ps::L_WJI], lg[ps::L_WKJ], lg[ps::L_WJI] + D, lg[ps::L_WKJ] + D};
            const int ldg[4] = {3 * D, 3 * D, 3 * D, 3 * D};
            TRY(launch_pre_bwd(D, p, gWp, ldg, lg[ps::L_WX1], lg[ps::L_BX1], R, st));
        }
        // ---------------- global layer
        {
            NTailBwd t = tail_bwd_params(g + ps::G_TAIL, im, k, G_TAIL, S, L.g_t);
            t.g_x = gx[0], t.g_out = d_outs + (2 * k) * n, t.g_att = d_atts + (2 * k) * n;
            t.d_x2 = d_x2, t.d_resx = d_resx, t.m = n;
            float* const* gt = gg + ps::G_TAIL;
            TRY(launch_tail_bwd(D, t, gt, gt + ps::T_B, gt[ps::T_WOUT], gt[ps::T_BOUT], gt[ps::T_WATT], R, st));
            float* dz = temp + L.t_dz;
            TRY(launch_global_bwd(D, e_g, eg, ix.g_row, ix.g_col, S + L.g_P, g[ps::G_WM] + 2 * D, 3 * D, g[ps::G_BM], g[ps::G_WEA], D,
                                  d_x2, dz, d_eg, first ? 0 : 1, R, gg[ps::G_WM] + 2 * D, 3 * D, gg[ps::G_WEA], gg[ps::G_BM], st));
            float* dpi = temp + L.t_dpi;
            float* dpj = temp + L.t_dpj;
            TRY(pamnet_segment_sum_f32(dpi, nullptr, dz, nullptr, nullptr, nullptr, nullptr, ix.g_ptr, n, d, stream));
            TRY(pamnet_segment_sum_f32(dpj, nullptr, dz, nullptr, nullptr, nullptr, ix.gT_perm, ix.gT_ptr, n, d, stream));
            NPreBwd p = {};
            p.x = x_glob, p.x1 = S + L.g_x1, p.img1 = im.at(k, G_W1, 0), p.img1t = im.at(k, G_W1, 1), p.b1 = g[ps::G_BX1], p.nb = 2, p.m = n;
            p.imgpt[0] = im.at(k, G_P, 1), p.imgpt[1] = im.at(k, G_P + 1, 1);
            p.dP[0] = dpi, p.dP[1] = dpj, p.lddp[0] = p.lddp[1] = D;
            p.d_direct = d_x2, p.d_add = d_resx, p.dx = k == 0 ? d_x0 : gx[1];
            float* gWp[2] = {gg[ps::G_WM], gg[ps::G_WM] + D};
            const int ldg[2] = {3 * D, 3 * D};
            TRY(launch_pre_bwd(D, p, gWp, ldg, gg[ps::G_WX1], gg[ps::G_BX1], R, st));
            g_x = gx[1];
        }
        TRY(R.flush());                   // this pair's gradients are complete before its event is recorded
        if (layer_done) {
            const hipError_t e_ = hipEventRecord(static_cast<hipEvent_t>(layer_done[k]), st);
            if (e_ != hipSuccess) return (int)e_;
        }
    }
    return PAMNET_OK;
}
