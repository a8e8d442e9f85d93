// C entry points of the narrow-width (dim = 16 / 32 / 64) row kernels, and the launchers of those the narrow-width
// layer-stack engine (narrow_engine.hip) uses too; the kernels themselves are in narrow_core.h.
#include "narrow_core.h"

// ---- launchers shared with the engine (declared in common.h): grid, block and LDS bytes of a kernel are decided here only
int narrow_rows::global_fwd(int d, const float* e, int64_t m, const int32_t* tgt, const int32_t* src, const float* P,
                            const float* We, int ldwe, const float* bias, const float* Wea, int ldwea, float* msg,
                            hipStream_t st) {
    if (m == 0) return PAMNET_OK;
    return narrow_dispatch(d, [&](auto D) {
        return narrow_launch(nglobal_fwd_kernel<D>, fwd_row_grid(m, D), NWG, nglobal_fwd_lds<D>(), st, e, m, tgt, src, P, We,
                             ldwe, bias, Wea, ldwea, msg);
    });
}

int narrow_rows::global_bwd(int d, const float* e, int64_t m, const int32_t* tgt, const int32_t* src, const float* P,
                            const float* We, int ldwe, const float* bias, const float* Wea, int ldwea, const float* dagg,
                            float* dz, float* de, float* partial, int acc_de, hipStream_t st) {
    return narrow_dispatch(d, [&](auto D) {
        return narrow_launch(nglobal_bwd_kernel<D>, bwd_row_grid(m, D), 64 * bwd_waves(D), nglobal_bwd_lds<D>(), st, e, m, tgt,
                             src, P, We, ldwe, bias, Wea, ldwea, dagg, dz, de, partial, nglobal_bwd_stride(D), acc_de);
    });
}

int narrow_rows::mlp2_fwd(int d, const float* x, int64_t m, const float* W1, const float* b1, const float* W2,
                          const float* b2, int res_x, const float* res, float* y, hipStream_t st) {
    if (m == 0) return PAMNET_OK;
    return narrow_dispatch(d, [&](auto D) {
        return narrow_launch(nmlp2_fwd_kernel<D>, fwd_row_grid(m, D), NWG, nmlp2_fwd_lds<D>(), st, x, m, W1, b1, W2, b2, res_x,
                             res, y);
    });
}

int narrow_rows::mlp2_bwd(int d, const float* x, int64_t m, const float* W1, const float* b1, const float* W2,
                          const float* b2, const float* dy, int res_x, float* dx, float* partial, int acc_dx,
                          hipStream_t st) {
    return narrow_dispatch(d, [&](auto D) {
        return narrow_launch(nmlp2_bwd_kernel<D>, bwd_row_grid(m, D), 64 * bwd_waves(D), nmlp2_bwd_lds<D>(), st, x, m, W1, b1, W2,
                             b2, dy, res_x, dx, partial, nmlp2_bwd_stride(D), acc_dx);
    });
}

int narrow_rows::linear_bwd(int d, const float* x, int64_t m, const float* W, int ldw, const float* b, int act,
                            const float* dy, int64_t lddy, float* dx, int accumulate, float* partial, int stride,
                            hipStream_t st) {
    return narrow_dispatch(d, [&](auto D) {
        return narrow_launch(nlinear_bwd_kernel<D>, bwd_row_grid(m, D), 64 * lin_bwd_waves(D), nlinear_bwd_lds<D>(), st, x, m, W,
                             ldw, b, act, dy, lddy, dx, accumulate, partial, stride);
    });
}

int narrow_rows::local_gate_bwd(int d, const float* P, const float* Q, const int32_t* tgt, const int32_t* src,
                                const float* b_ji, const float* b_kj, int64_t m, const float* g_ji, const float* g_nb,
                                float* dz, float* dQ, int zero_q3, hipStream_t st) {
    if (m == 0) return PAMNET_OK;
    return narrow_dispatch(d, [&](auto D) {
        return narrow_launch(nlocal_gate_bwd_kernel<D>, ew_grid(m * (D / 4)), 256, 0, st, P, Q, tgt, src, b_ji, b_kj, m, g_ji,
                             g_nb, dz, dQ, zero_q3);
    });
}

namespace {

#define TRY(x)                              \
    do {                                    \
        const int rc_ = (x);                \
        if (rc_ != PAMNET_OK) return rc_;   \
    } while (0)

// The entry points reduce their `nblk` partial rows at once: `nmat` [d, kp] matrices in fragment order (columns < kvalid
// kept) to `mats`, the `nbias` floats after them to `bias`.
int reduce_rows(const float* partial, int nblk, int stride, int nmat, int d, int kp, int kvalid, int nbias, float* mats,
                float* bias, hipStream_t st) {
    const int total = nmat * d * kp + nbias;
    return narrow_launch(narrow_reduce_kernel, (total + 63) / 64, dim3(64, 8), 0, st, partial, nblk, stride, nmat, d, kp,
                         kvalid, nbias, mats, bias);
}

// f(K, TWO) with the feature width of an embedding (16 / 42) and "two weight sets" as compile-time constants
template <typename F>
int embed_dispatch(int64_t k, bool two, F&& f) {
    using K16 = std::integral_constant<int, 16>;
    using K42 = std::integral_constant<int, 42>;
    if (k == 16) return two ? f(K16{}, std::true_type{}) : f(K16{}, std::false_type{});
    return two ? f(K42{}, std::true_type{}) : f(K42{}, std::false_type{});
}

}  // namespace

extern "C" int pamnet_narrow_blocks(int64_t rows, int64_t* blocks) {
    if (rows < 0) return PAMNET_EINVAL;
    if (!blocks) return PAMNET_ENULL;
    *blocks = NARROW_BLOCKS;                                 // backward kernels: at most one workgroup per CU
    return PAMNET_OK;
}

extern "C" int pamnet_narrow_global_fwd_f32(const float* e, int64_t m, int64_t d, const int32_t* tgt, const int32_t* src,
                                            const float* P, const float* We, int64_t ldwe, const float* bias,
                                            const float* Wea, int64_t ldwea, float* msg, pamnet_stream_t stream) {
    if (m < 0 || !width_ok(d) || ldwe < d || ldwea < d || (ldwe & 3) || (ldwea & 3)) return PAMNET_EINVAL;
    if (m == 0) return PAMNET_OK;
    if (!e || !tgt || !src || !P || !We || !bias || !Wea || !msg) return PAMNET_ENULL;
    return narrow_rows::global_fwd((int)d, e, m, tgt, src, P, We, (int)ldwe, bias, Wea, (int)ldwea, msg, as_stream(stream));
}

extern "C" int pamnet_narrow_global_bwd_f32(const float* e, int64_t m, int64_t d, const int32_t* tgt, const int32_t* src,
                                            const float* P, const float* We, int64_t ldwe, const float* bias,
                                            const float* Wea, int64_t ldwea, const float* dagg, float* dz, float* de,
                                            float* partial, float* dWe, float* dWea, float* db,
                                            pamnet_stream_t stream) {
    if (m <= 0 || !width_ok(d) || ldwe < d || ldwea < d || (ldwe & 3) || (ldwea & 3)) return PAMNET_EINVAL;
    if (!e || !tgt || !src || !P || !We || !bias || !Wea || !dagg || !dz || !de || !partial || !dWe || !dWea || !db)
        return PAMNET_ENULL;
    hipStream_t st = as_stream(stream);
    const int D = (int)d;
    TRY(narrow_rows::global_bwd(D, e, m, tgt, src, P, We, (int)ldwe, bias, Wea, (int)ldwea, dagg, dz, de, partial, 0, st));
    // dWe and dWea are separate outputs: two reduce launches over the same partial rows (matrix 0 / matrix 1 + bias)
    const int grid = bwd_row_grid(m, d), stride = nglobal_bwd_stride(D);
    TRY(reduce_rows(partial, grid, stride, 1, D, D, D, 0, dWe, nullptr, st));
    return reduce_rows(partial + D * D, grid, stride, 1, D, D, D, D, dWea, db, st);
}

extern "C" int pamnet_narrow_mlp2_fwd_f32(const float* x, int64_t m, int64_t d, const float* W1, const float* b1,
                                          const float* W2, const float* b2, int32_t res_x, const float* res, float* y,
                                          pamnet_stream_t stream) {
    if (m < 0 || !width_ok(d)) return PAMNET_EINVAL;
    if (m == 0) return PAMNET_OK;
    if (!x || !W1 || !b1 || !W2 || !b2 || !y) return PAMNET_ENULL;
    return narrow_rows::mlp2_fwd((int)d, x, m, W1, b1, W2, b2, res_x, res, y, as_stream(stream));
}

extern "C" int pamnet_narrow_mlp2_bwd_f32(const float* x, int64_t m, int64_t d, const float* W1, const float* b1,
                                          const float* W2, const float* b2, const float* dy, int32_t res_x, float* dx,
                                          float* partial, float* dW /* [2, d, d] */, float* db /* [2, d] */,
                                          pamnet_stream_t stream) {
    if (m <= 0 || !width_ok(d)) return PAMNET_EINVAL;
    if (!x || !W1 || !b1 || !W2 || !b2 || !dy || !partial || !dW || !db) return PAMNET_ENULL;
    hipStream_t st = as_stream(stream);
    const int D = (int)d;
    TRY(narrow_rows::mlp2_bwd(D, x, m, W1, b1, W2, b2, dy, res_x, dx, partial, 0, st));
    return reduce_rows(partial, bwd_row_grid(m, d), nmlp2_bwd_stride(D), 2, D, D, D, 2 * D, dW, db, st);
}

extern "C" int pamnet_narrow_linear_fwd_f32(const float* x, int64_t m, int64_t d, const float* W, int64_t ldw,
                                            const float* b, int32_t act, float* y, int64_t ldy,
                                            pamnet_stream_t stream) {
    if (m < 0 || !width_ok(d) || ldw < d || ldy < d) return PAMNET_EINVAL;
    if (m == 0) return PAMNET_OK;
    if (!x || !W || !y) return PAMNET_ENULL;
    hipStream_t st = as_stream(stream);
    return narrow_dispatch(d, [&](auto D) {
        return narrow_launch(nlinear_fwd_kernel<D>, fwd_row_grid(m, D), NWG, nlinear_fwd_lds<D>(), st, x, m, W, ldw, b, act, y,
                             ldy);
    });
}

/* dx optional; accumulate != 0: dx += ...; dW [d, d] dense, db [d] (null when the layer has no bias) */
extern "C" int pamnet_narrow_linear_bwd_f32(const float* x, int64_t m, int64_t d, const float* W, int64_t ldw,
                                            const float* b, int32_t act, const float* dy, int64_t lddy, float* dx,
                                            int32_t accumulate, float* partial, float* dW, float* db,
                                            pamnet_stream_t stream) {
    if (m <= 0 || !width_ok(d) || ldw < d || lddy < d) return PAMNET_EINVAL;
    if (!x || !W || !dy || !partial || !dW) return PAMNET_ENULL;
    hipStream_t st = as_stream(stream);
    const int D = (int)d, stride = nlinear_bwd_stride(D);
    TRY(narrow_rows::linear_bwd(D, x, m, W, (int)ldw, b, act, dy, lddy, dx, accumulate, partial, stride, st));
    return reduce_rows(partial, bwd_row_grid(m, d), stride, 1, D, D, D, db ? D : 0, dW, db, st);
}

extern "C" int pamnet_narrow_heads_fwd_f32(const float* o, int64_t m, int64_t d, const float* w_out, const float* b_out,
                                           const float* w_att, float* out, float* att, pamnet_stream_t stream) {
    if (m < 0 || !width_ok(d)) return PAMNET_EINVAL;
    if (m == 0) return PAMNET_OK;
    if (!o || !w_out || !b_out || !w_att || !out || !att) return PAMNET_ENULL;
    hipStream_t st = as_stream(stream);
    const int rpb = 256 / (int)(d / 4);
    const int64_t want = (m + rpb - 1) / rpb;
    const int grid = (int)(want < 1024 ? want : 1024);
    return narrow_dispatch(d, [&](auto D) {
        return narrow_launch(nheads_fwd_kernel<D>, grid, 256, 0, st, o, m, w_out, b_out, w_att, out, att);
    });
}

/* dvec [2 d + 1] = [d w_out | d w_att | d b_out]; partial: pamnet_narrow_blocks x (2 d + 1) floats */
extern "C" int pamnet_narrow_heads_bwd_f32(const float* o, int64_t m, int64_t d, const float* w_out, const float* w_att,
                                           const float* g_out, const float* g_att, float* d_o, float* partial,
                                           float* dvec, pamnet_stream_t stream) {
    if (m <= 0 || !width_ok(d)) return PAMNET_EINVAL;
    if (!o || !w_out || !w_att || !g_out || !g_att || !d_o || !partial || !dvec) return PAMNET_ENULL;
    hipStream_t st = as_stream(stream);
    const int D = (int)d;
    const int rpb = 256 / (D / 4);
    const int64_t want = (m + rpb - 1) / rpb;
    const int grid = (int)(want < NARROW_BLOCKS ? want : NARROW_BLOCKS);
    TRY(narrow_dispatch(d, [&](auto DD) {
        return narrow_launch(nheads_bwd_kernel<DD>, grid, 256, 0, st, o, m, w_out, w_att, g_out, g_att, d_o, partial);
    }));
    const int total = nheads_bwd_stride(D);
    return reduce_rows(partial, grid, total, 0, D, D, D, total, nullptr, dvec, st);
}

extern "C" int pamnet_narrow_local_gate_fwd_f32(const float* P, const float* Q, const int32_t* tgt, const int32_t* src,
                                                const float* b_ji, const float* b_kj, int64_t m, int64_t d, float* m_ji,
                                                float* m_nb, pamnet_stream_t stream) {
    if (m < 0 || !width_ok(d)) return PAMNET_EINVAL;
    if (m == 0) return PAMNET_OK;
    if (!P || !Q || !tgt || !src || !b_ji || !b_kj || !m_ji || !m_nb) return PAMNET_ENULL;
    hipStream_t st = as_stream(stream);
    return narrow_dispatch(d, [&](auto D) {
        return narrow_launch(nlocal_gate_fwd_kernel<D>, ew_grid(m * (D / 4)), 256, 0, st, P, Q, tgt, src, b_ji, b_kj, m, m_ji,
                             m_nb);
    });
}

extern "C" int pamnet_narrow_local_gate_bwd_f32(const float* P, const float* Q, const int32_t* tgt, const int32_t* src,
                                                const float* b_ji, const float* b_kj, int64_t m, int64_t d,
                                                const float* g_ji, const float* g_nb, float* dz, float* dQ,
                                                pamnet_stream_t stream) {
    if (m < 0 || !width_ok(d)) return PAMNET_EINVAL;
    if (m == 0) return PAMNET_OK;
    if (!P || !Q || !tgt || !src || !b_ji || !b_kj || !g_ji || !g_nb || !dz || !dQ) return PAMNET_ENULL;
    return narrow_rows::local_gate_bwd((int)d, P, Q, tgt, src, b_ji, b_kj, m, g_ji, g_nb, dz, dQ, 1, as_stream(stream));
}

extern "C" int pamnet_narrow_embed_fwd_f32(const float* F, int64_t m, int64_t k, int64_t d, const int32_t* kind,
                                           const float* Wa, const float* ba, const float* Wb, const float* bb, float* y,
                                           pamnet_stream_t stream) {
    if (m < 0 || !width_ok(d) || (k != 16 && k != 42)) return PAMNET_EINVAL;
    if (m == 0) return PAMNET_OK;
    if (!F || !Wa || !ba || !y || (kind && (!Wb || !bb))) return PAMNET_ENULL;
    hipStream_t st = as_stream(stream);
    return narrow_dispatch(d, [&](auto D) {
        return embed_dispatch(k, kind != nullptr, [&](auto K, auto TWO) {
            return narrow_launch(nembed_fwd_kernel<D, K, TWO>, fwd_row_grid(m, D), NWG, nembed_fwd_lds<D, K, TWO>(), st, F, m,
                                 kind, Wa, ba, Wb, bb, y, nullptr, 0.f);
        });
    });
}

/* The 16-wide edge embedding (models.py:185-186) on Bessel rows formed inside the kernel (forward only: inference):
 * dist [m], freq [16], cutoff as for pamnet_rbf_fwd_f32; the same floats as pamnet_rbf_fwd_f32 + pamnet_narrow_embed_fwd_f32. */
extern "C" int pamnet_narrow_embed_rbf_fwd_f32(const float* dist, const float* freq, float cutoff, int64_t m, int64_t d,
                                               const float* Wa, const float* ba, float* y, pamnet_stream_t stream) {
    if (m < 0 || !width_ok(d) || !(cutoff > 0.f)) return PAMNET_EINVAL;
    if (m == 0) return PAMNET_OK;
    if (!dist || !freq || !Wa || !ba || !y) return PAMNET_ENULL;
    hipStream_t st = as_stream(stream);
    return narrow_dispatch(d, [&](auto D) {
        return narrow_launch(nembed_fwd_kernel<D, 16, false, true>, fwd_row_grid(m, D), NWG, nembed_fwd_lds<D, 16, false>(), st,
                             dist, m, nullptr, Wa, ba, nullptr, nullptr, y, freq, 1.0f / cutoff);
    });
}

/* dW: [sets, d, k] (set 0 = Wa, set 1 = Wb when `kind` is given), db: [sets, d]; df [m, 16] optional (k = 16, one set) */
extern "C" int pamnet_narrow_embed_bwd_f32(const float* F, int64_t m, int64_t k, int64_t d, const int32_t* kind,
                                           const float* Wa, const float* ba, const float* Wb, const float* bb,
                                           const float* dy, float* df, float* partial, float* dW, float* db,
                                           pamnet_stream_t stream) {
    if (m <= 0 || !width_ok(d) || (k != 16 && k != 42)) return PAMNET_EINVAL;
    if (!F || !Wa || !ba || !dy || !partial || !dW || !db || (kind && (!Wb || !bb))) return PAMNET_ENULL;
    if (df && (k != 16 || kind)) return PAMNET_EINVAL;
    hipStream_t st = as_stream(stream);
    const int D = (int)d, grid = bwd_row_grid(m, d);
    const int kp = (k == 16) ? 16 : 48;
    const int sets = kind ? 2 : 1;
    const int stride = nembed_bwd_stride(D, kp, sets);
    TRY(narrow_dispatch(d, [&](auto DD) {
        return embed_dispatch(k, kind != nullptr, [&](auto K, auto TWO) {
            auto launch = [&](auto DX) {
                return narrow_launch(nembed_bwd_kernel<DD, K, TWO, DX>, grid, 64 * bwd_waves(DD), nembed_bwd_lds<DD, K, TWO, DX>(),
                                     st, F, m, kind, Wa, ba, Wb, bb, dy, df, partial, stride, nullptr, 0.f);
            };
            if constexpr (K == 16 && !TWO) {                 // the only form that can return df
                if (df) return launch(std::true_type{});
            }
            return launch(std::false_type{});
        });
    }));
    return reduce_rows(partial, grid, stride, sets, D, kp, (int)k, sets * D, dW, db, st);
}

/* Backward of pamnet_narrow_embed_rbf_fwd_f32: dW [d, 16], db_dfreq [d + 16] = the bias gradient followed by the gradient of
 * the 16 Bessel frequencies (layers/basic.py:65-76); partial: blocks x (d * 16 + d + 16) floats.  The [m, 16] rows and their
 * gradient never exist. */
extern "C" int pamnet_narrow_embed_rbf_bwd_f32(const float* dist, const float* freq, float cutoff, int64_t m, int64_t d,
                                               const float* Wa, const float* ba, const float* dy, float* partial, float* dW,
                                               float* db_dfreq, pamnet_stream_t stream) {
    if (m <= 0 || !width_ok(d) || !(cutoff > 0.f)) return PAMNET_EINVAL;
    if (!dist || !freq || !Wa || !ba || !dy || !partial || !dW || !db_dfreq) return PAMNET_ENULL;
    hipStream_t st = as_stream(stream);
    const int D = (int)d, grid = bwd_row_grid(m, d);
    const int stride = nembed_bwd_stride(D, 16, 1, true);
    TRY(narrow_dispatch(d, [&](auto DD) {
        return narrow_launch(nembed_bwd_kernel<DD, 16, false, true, true>, grid, 64 * bwd_waves(DD),
                             nembed_bwd_lds<DD, 16, false, true>(), st, dist, m, nullptr, Wa, ba, nullptr, nullptr, dy, nullptr,
                             partial, stride, freq, 1.0f / cutoff);
    }));
    return reduce_rows(partial, grid, stride, 1, D, 16, 16, D + 16, dW, db_dfreq, st);
}
