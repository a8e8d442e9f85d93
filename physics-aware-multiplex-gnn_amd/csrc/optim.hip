// Optimiser tail of the training step as ONE pass over the flat fp32 buffers (train.FlatParams):
//   clip_grad_norm_(max_norm, L2)  ->  Adam(lr, betas, eps, weight_decay, amsgrad=False)  ->  EMA  [-> zero the gradient]
// i.e. main_qm9.py:111-112,116 + utils/ema.py:13-20.  The reference issues ~10 small launches per parameter tensor
// (~3 000 per step at L=6); here every element is read and written once: 5 reads + 4 (5) writes of n floats, HBM-bound.
// The pre-clip gradient norm is read from device memory (no host round trip between the norm reduction and the update).
#include "common.h"

namespace {

struct AdamArgs {
    float lr, beta1, beta2, eps, weight_decay;
    float bias1, bias2_sqrt;          // 1 - beta1^t,  sqrt(1 - beta2^t)
    float ema_decay, max_norm;
    int zero_grad;
};

template <bool EMA>
__global__ __launch_bounds__(256) void adam_ema_kernel(float4* __restrict__ p, float4* __restrict__ g,
                                                       float4* __restrict__ m, float4* __restrict__ v,
                                                       float4* __restrict__ shadow, int64_t n4,
                                                       const float* __restrict__ grad_norm,
                                                       const double* __restrict__ sumsq_partials,
                                                       float* __restrict__ norm_out, AdamArgs a) {
    float clip = 1.0f;
    if (sumsq_partials) {
        // 256 fp64 partial sums of squares (pamnet_sumsq_partials_f32): every workgroup adds them in index order itself
        // (2 KB of L2 hits) -- no finish launch, no cross-workgroup synchronisation
        __shared__ double red[256];
        red[threadIdx.x] = sumsq_partials[threadIdx.x];
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
            __syncthreads();
        }
        const float nrm = (float)sqrt(red[0]);
        if (norm_out && blockIdx.x == 0 && threadIdx.x == 0) norm_out[0] = nrm;
        clip = fminf(a.max_norm / (nrm + 1e-6f), 1.0f);
    } else if (grad_norm) {
        clip = fminf(a.max_norm / (grad_norm[0] + 1e-6f), 1.0f);                  // torch clip_grad_norm_
    }
    const float step = a.lr / a.bias1;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 pp = p[i], gg = g[i], mm = m[i], vv = v[i], ss = EMA ? shadow[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        float* pf = &pp.x;
        float* gf = &gg.x;
        float* mf = &mm.x;
        float* vf = &vv.x;
        float* sf = &ss.x;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float gr = gf[c] * clip;
            if (a.weight_decay != 0.0f) gr = fmaf(a.weight_decay, pf[c], gr);
            mf[c] = fmaf(a.beta1, mf[c], (1.0f - a.beta1) * gr);                      // exp_avg.lerp_(grad, 1-beta1)
            vf[c] = fmaf(a.beta2, vf[c], (1.0f - a.beta2) * gr * gr);                 // exp_avg_sq
            const float denom = sqrtf(vf[c]) / a.bias2_sqrt + a.eps;
            pf[c] -= step * (mf[c] / denom);
            if (EMA) sf[c] = fmaf(a.ema_decay, sf[c], (1.0f - a.ema_decay) * pf[c]);
        }
        p[i] = pp;
        m[i] = mm;
        v[i] = vv;
        if (EMA) shadow[i] = ss;
        if (a.zero_grad) g[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// Parameter groups (train.Trainer(param_groups=...)): train.FlatParams starts every tensor on a 64-float boundary, so one
// byte per 64-float chunk names an element's group; the per-group values travel in the kernel arguments (by value) and are
// staged in LDS once per workgroup.  An id is taken modulo 16 (never an index outside the table) and the entries past the
// caller's n_groups are frozen.
constexpr int MAX_GROUPS = PAMNET_MAX_PARAM_GROUPS;
static_assert(MAX_GROUPS == 16, "a group id is masked to 4 bits");

struct GroupTable {
    float step[MAX_GROUPS];           // lr_g / (1 - beta1^t)
    float wd[MAX_GROUPS];             // L2: weight_decay_g;  decoupled: 1 - lr_g * weight_decay_g (the factor on p)
    uint32_t frozen;                  // bit g: group g is never updated
};

template <bool EMA, bool DECOUPLED>
__global__ __launch_bounds__(256) void adam_ema_groups_kernel(float4* __restrict__ p, float4* __restrict__ g,
                                                              float4* __restrict__ m, float4* __restrict__ v,
                                                              float4* __restrict__ shadow, int64_t n4,
                                                              const uint8_t* __restrict__ chunk_group,
                                                              const double* __restrict__ sumsq_partials,
                                                              float* __restrict__ norm_out, AdamArgs a, GroupTable t) {
    __shared__ double red[256];
    __shared__ float s_step[MAX_GROUPS], s_wd[MAX_GROUPS];
    if (threadIdx.x < MAX_GROUPS) s_step[threadIdx.x] = t.step[threadIdx.x], s_wd[threadIdx.x] = t.wd[threadIdx.x];
    red[threadIdx.x] = sumsq_partials[threadIdx.x];       // as adam_ema_kernel: every workgroup finishes the norm itself
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const float nrm = (float)sqrt(red[0]);
    if (norm_out && blockIdx.x == 0 && threadIdx.x == 0) norm_out[0] = nrm;
    const float clip = fminf(a.max_norm / (nrm + 1e-6f), 1.0f);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const int grp = chunk_group[i >> 4] & (MAX_GROUPS - 1);        // 16 float4 per chunk
        if ((t.frozen >> grp) & 1u) {
            if (a.zero_grad) g[i] = zero;
            continue;
        }
        float4 pp = p[i], gg = g[i], mm = m[i], vv = v[i], ss = EMA ? shadow[i] : zero;
        const float step = s_step[grp], wd = s_wd[grp];
        float* pf = &pp.x;
        float* gf = &gg.x;
        float* mf = &mm.x;
        float* vf = &vv.x;
        float* sf = &ss.x;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float gr = gf[c] * clip;
            if (DECOUPLED) {
                pf[c] *= wd;                                                          // param.mul_(1 - lr * weight_decay)
            } else if (wd != 0.0f) {
                gr = fmaf(wd, pf[c], gr);
            }
            mf[c] = fmaf(a.beta1, mf[c], (1.0f - a.beta1) * gr);
            vf[c] = fmaf(a.beta2, vf[c], (1.0f - a.beta2) * gr * gr);
            const float denom = sqrtf(vf[c]) / a.bias2_sqrt + a.eps;
            pf[c] -= step * (mf[c] / denom);
            if (EMA) sf[c] = fmaf(a.ema_decay, sf[c], (1.0f - a.ema_decay) * pf[c]);
        }
        p[i] = pp;
        m[i] = mm;
        v[i] = vv;
        if (EMA) shadow[i] = ss;
        if (a.zero_grad) g[i] = zero;
    }
}

// n must be a multiple of 4 and the buffers 16-byte aligned (train.FlatParams pads every tensor to 64 floats).
// step_count = t >= 1 of this update.  grad_norm: device scalar holding the pre-clip L2 norm (nullable = no clipping).
int adam_launch(float* p, float* g, float* m, float* v, float* shadow, int64_t n, float lr, float beta1, float beta2,
                float eps, float weight_decay, int64_t step_count, float ema_decay, const float* grad_norm,
                const double* sumsq_partials, float* norm_out, float max_norm, int32_t zero_grad, pamnet_stream_t stream) {
    if (n < 0 || (n & 3) || step_count < 1) return PAMNET_EINVAL;
    if (n == 0) return PAMNET_OK;
    if (!p || !g || !m || !v) return PAMNET_ENULL;
    AdamArgs a;
    a.lr = lr, a.beta1 = beta1, a.beta2 = beta2, a.eps = eps, a.weight_decay = weight_decay;
    a.bias1 = (float)(1.0 - pow((double)beta1, (double)step_count));
    a.bias2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step_count));
    a.ema_decay = ema_decay, a.max_norm = max_norm, a.zero_grad = zero_grad;
    const int64_t n4 = n / 4;
    int64_t blocks = ceil_div(n4, 256);
    if (blocks > 4096) blocks = 4096;
    if (shadow)
        hipLaunchKernelGGL(adam_ema_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), (float4*)p,
                           (float4*)g, (float4*)m, (float4*)v, (float4*)shadow, n4, grad_norm, sumsq_partials, norm_out, a);
    else                                   // no EMA (main_pdbbind.py / main_rna_puzzles.py): 4 reads + 3 (4) writes per element
        hipLaunchKernelGGL(adam_ema_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), (float4*)p,
                           (float4*)g, (float4*)m, (float4*)v, (float4*)nullptr, n4, grad_norm, sumsq_partials, norm_out, a);
    PAMNET_LAUNCH_CHECK();
    return PAMNET_OK;
}
}  // namespace

extern "C" int pamnet_adam_ema_f32(float* p, float* g, float* m, float* v, float* shadow, int64_t n, float lr,
                                   float beta1, float beta2, float eps, float weight_decay, int64_t step_count,
                                   float ema_decay, const float* grad_norm, float max_norm, int32_t zero_grad,
                                   pamnet_stream_t stream) {
    return adam_launch(p, g, m, v, shadow, n, lr, beta1, beta2, eps, weight_decay, step_count, ema_decay, grad_norm,
                       nullptr, nullptr, max_norm, zero_grad, stream);
}

// Same update with the gradient norm taken from the 256 fp64 partial sums of squares of pamnet_sumsq_partials_f32
// (clip on); norm_out[0] (nullable) receives the pre-clip L2 norm.
extern "C" int pamnet_adam_ema_norm_f32(float* p, float* g, float* m, float* v, float* shadow, int64_t n, float lr,
                                        float beta1, float beta2, float eps, float weight_decay, int64_t step_count,
                                        float ema_decay, const double* sumsq_partials, float* norm_out, float max_norm,
                                        int32_t zero_grad, pamnet_stream_t stream) {
    if (!sumsq_partials) return PAMNET_ENULL;
    return adam_launch(p, g, m, v, shadow, n, lr, beta1, beta2, eps, weight_decay, step_count, ema_decay, nullptr,
                       sumsq_partials, norm_out, max_norm, zero_grad, stream);
}

// Parameter groups: see include/pamnet_hip.h.  lr_scale / weight_decay / frozen are host arrays of n_groups entries.
extern "C" int pamnet_adam_ema_groups_f32(float* p, float* g, float* m, float* v, float* shadow, int64_t n,
                                          const uint8_t* chunk_group, int64_t n_groups, const float* lr_scale,
                                          const float* weight_decay, const int32_t* frozen, float lr, float beta1,
                                          float beta2, float eps, int32_t decoupled, int64_t step_count, float ema_decay,
                                          const double* sumsq_partials, float* norm_out, float max_norm,
                                          int32_t zero_grad, pamnet_stream_t stream) {
    if (n < 0 || (n & 63) || step_count < 1 || n_groups < 1 || n_groups > MAX_GROUPS) return PAMNET_EINVAL;
    if (!lr_scale || !weight_decay || !frozen) return PAMNET_ENULL;
    for (int64_t k = 0; k < n_groups; ++k)
        if (!(lr_scale[k] >= 0.0f) || !(weight_decay[k] >= 0.0f)) return PAMNET_EINVAL;       // (refuses NaN too)
    if (n == 0) return PAMNET_OK;
    if (!p || !g || !m || !v || !chunk_group || !sumsq_partials) return PAMNET_ENULL;
    AdamArgs a;
    a.lr = lr, a.beta1 = beta1, a.beta2 = beta2, a.eps = eps, a.weight_decay = 0.0f;
    a.bias1 = (float)(1.0 - pow((double)beta1, (double)step_count));
    a.bias2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step_count));
    a.ema_decay = ema_decay, a.max_norm = max_norm, a.zero_grad = zero_grad;
    GroupTable t;
    t.frozen = 0xffffffffu;
    for (int k = 0; k < MAX_GROUPS; ++k) t.step[k] = 0.0f, t.wd[k] = decoupled ? 1.0f : 0.0f;
    for (int64_t k = 0; k < n_groups; ++k) {
        const float lr_g = (float)((double)lr * (double)lr_scale[k]);
        t.step[k] = lr_g / a.bias1;
        t.wd[k] = decoupled ? 1.0f - lr_g * weight_decay[k] : weight_decay[k];
        if (!frozen[k]) t.frozen &= ~(1u << k);
    }
    const int64_t n4 = n / 4;
    int64_t blocks = ceil_div(n4, 256);
    if (blocks > 4096) blocks = 4096;
#define PAMNET_GROUPS_LAUNCH(EMA, DEC)                                                                                    \
    hipLaunchKernelGGL((adam_ema_groups_kernel<EMA, DEC>), dim3((unsigned)blocks), dim3(256), 0, as_stream(stream),       \
                       (float4*)p, (float4*)g, (float4*)m, (float4*)v, (float4*)shadow, n4, chunk_group, sumsq_partials, \
                       norm_out, a, t)
    if (shadow) {
        if (decoupled) PAMNET_GROUPS_LAUNCH(true, true);
        else PAMNET_GROUPS_LAUNCH(true, false);
    } else {
        if (decoupled) PAMNET_GROUPS_LAUNCH(false, true);
        else PAMNET_GROUPS_LAUNCH(false, false);
    }
#undef PAMNET_GROUPS_LAUNCH
    PAMNET_LAUNCH_CHECK();
    return PAMNET_OK;
}
