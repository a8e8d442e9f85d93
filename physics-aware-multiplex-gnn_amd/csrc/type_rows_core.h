// Per-type row sums (gradient of `embeddings[x]`, models.py:107,140) as device bodies, shared by the stand-alone entry
// (reduce.hip) and the input-embedding launches (embed.hip):
//   out[t, :] = sum_{r: idx[r] = t} g[r, :],  t < n_types <= 8 (grad_body / finish_body); 9 .. 128 rows: the wide bodies below.
// Lane group (d4 lanes) per row slot; a workgroup owns a contiguous slice of rows, slot s walks rows s, s + slots, ...
// (fixed), slots meet in LDS in slot order, workgroups in finish_body in workgroup order -- deterministic.
#pragma once
#include "common.h"

namespace {
namespace type_rows {

constexpr int TYPE_MAX = 8, TYPE_BLOCKS = 64;

inline int blocks_for_rows(int64_t n) {
    int64_t blocks = (n + 127) / 128;                        // >= 128 rows per workgroup: few partials for the finish
    return (int)(blocks < 1 ? 1 : (blocks > TYPE_BLOCKS ? TYPE_BLOCKS : blocks));
}

// 256 threads; red: 256 float4 of LDS
__device__ __forceinline__ void grad_body(const float4* __restrict__ g, const int32_t* __restrict__ idx, int64_t n,
                                          int n_types, int d4, float4* __restrict__ partial, int bid, int nblk,
                                          float4* red) {
    const int c = threadIdx.x % d4, slot = threadIdx.x / d4, slots = 256 / d4;
    const int64_t per = (n + nblk - 1) / nblk;
    const int64_t beg = bid * per, end = beg + per < n ? beg + per : n;
    float4 acc[TYPE_MAX];
#pragma unroll
    for (int t = 0; t < TYPE_MAX; ++t) acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t r = beg + slot; r < end; r += slots) {
        const int ty = idx[r];
        const float4 v = g[r * d4 + c];
#pragma unroll
        for (int t = 0; t < TYPE_MAX; ++t) {
            const float m = ty == t ? 1.f : 0.f;
            acc[t].x = fmaf(m, v.x, acc[t].x), acc[t].y = fmaf(m, v.y, acc[t].y);
            acc[t].z = fmaf(m, v.z, acc[t].z), acc[t].w = fmaf(m, v.w, acc[t].w);
        }
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < TYPE_MAX; ++t) {
        if (t >= n_types) break;
        red[threadIdx.x] = acc[t];
        __syncthreads();
        if (slot == 0) {
            float4 s = red[c];
            for (int k = 1; k < slots; ++k) {
                const float4 v = red[k * d4 + c];
                s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
            }
            partial[((int64_t)bid * n_types + t) * d4 + c] = s;
        }
        __syncthreads();
    }
}

// one workgroup (256 threads): out[e] = sum over workgroup partials, in workgroup order
__device__ __forceinline__ void finish_body(const float4* __restrict__ partial, int blocks, int cells,
                                            float4* __restrict__ out) {
    for (int e = threadIdx.x; e < cells; e += 256) {
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        int b = 0;
        for (; b + 8 <= blocks; b += 8) {                  // 8 independent loads in flight, added in workgroup order
            float4 v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = partial[(int64_t)(b + k) * cells + e];
#pragma unroll
            for (int k = 0; k < 8; ++k) s.x += v[k].x, s.y += v[k].y, s.z += v[k].z, s.w += v[k].w;
        }
        for (; b < blocks; ++b) {
            const float4 v = partial[(int64_t)b * cells + e];
            s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
        }
        out[e] = s;
    }
}

// ---- tables of 9 .. 128 rows ----------------------------------------------------------------------------------------------
// The same slices, slots and orders as above, with the eight accumulators dealt to the types that OCCUR in the workgroup's
// slice: the workgroup forms the 128-bit set of its types (integer atomicOr in LDS: the result does not depend on the order),
// walks the set in ascending order eight types at a time -- grad_body's loop with the compare value taken from that list --
// and writes partial[bid][t][:] for the types of its set only, and the set itself.  finish_wide_body adds, per cell, the
// partials of the workgroups whose set holds the type, in workgroup order (none: an exact zero).  A slice of one to eight
// types is one pass with grad_body's arithmetic, term by term.
// scratch: TYPE_BLOCKS float4 (four mask words per workgroup), then partial[TYPE_BLOCKS][n_types][d4].
constexpr int TYPE_ROWS_MAX = 128;

inline int64_t wide_scratch_bytes(int64_t n_types, int64_t d4) { return 16 * (TYPE_BLOCKS + TYPE_BLOCKS * n_types * d4); }

// the lowest set bit of the four words leaves the set; its index (-1: the set was empty)
__device__ __forceinline__ int take_lowest(uint32_t (&m)[4]) {
    int r = -1;
#pragma unroll
    for (int w = 3; w >= 0; --w) r = m[w] ? 32 * w + __builtin_ctz(m[w]) : r;
#pragma unroll
    for (int w = 0; w < 4; ++w) m[w] &= (r >> 5) == w ? m[w] - 1 : ~0u;        // (r = -1: r >> 5 = -1, no word)
    return r;
}

// 256 threads; red: 256 float4 of LDS; seen: 4 words of LDS.  masks + 4 bid .. + 3: this workgroup's set.
__device__ __forceinline__ void grad_wide_body(const float4* __restrict__ g, const int32_t* __restrict__ idx, int64_t n,
                                               int n_types, int d4, uint32_t* __restrict__ masks,
                                               float4* __restrict__ partial, int bid, int nblk, float4* red,
                                               uint32_t* seen) {
    const int c = threadIdx.x % d4, slot = threadIdx.x / d4, slots = 256 / d4;
    const int64_t per = (n + nblk - 1) / nblk;
    const int64_t beg = bid * per, end = beg + per < n ? beg + per : n;
    if (threadIdx.x < 4) seen[threadIdx.x] = 0u;
    __syncthreads();
    for (int64_t r = beg + threadIdx.x; r < end; r += 256) {
        const int ty = idx[r];
        if (ty >= 0 && ty < n_types) atomicOr(&seen[ty >> 5], 1u << (ty & 31));
    }
    __syncthreads();
    uint32_t m[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) m[w] = __builtin_amdgcn_readfirstlane(seen[w]);
    if (threadIdx.x < 4) masks[4 * bid + threadIdx.x] = seen[threadIdx.x];
    while (m[0] | m[1] | m[2] | m[3]) {
        int lst[TYPE_MAX];                                   // this pass's types, ascending; -1: no type (never matches)
#pragma unroll
        for (int t = 0; t < TYPE_MAX; ++t) lst[t] = take_lowest(m);
        float4 acc[TYPE_MAX];
#pragma unroll
        for (int t = 0; t < TYPE_MAX; ++t) acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int64_t r = beg + slot; r < end; r += slots) {
            const int raw = idx[r];
            const int ty = raw >= 0 ? raw : -2;
            const float4 v = g[r * d4 + c];
#pragma unroll
            for (int t = 0; t < TYPE_MAX; ++t) {
                const float w = ty == lst[t] ? 1.f : 0.f;
                acc[t].x = fmaf(w, v.x, acc[t].x), acc[t].y = fmaf(w, v.y, acc[t].y);
                acc[t].z = fmaf(w, v.z, acc[t].z), acc[t].w = fmaf(w, v.w, acc[t].w);
            }
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < TYPE_MAX; ++t) {
            if (lst[t] < 0) break;
            red[threadIdx.x] = acc[t];
            __syncthreads();
            if (slot == 0) {
                float4 s = red[c];
                for (int k = 1; k < slots; ++k) {
                    const float4 v = red[k * d4 + c];
                    s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
                }
                partial[((int64_t)bid * n_types + lst[t]) * d4 + c] = s;
            }
            __syncthreads();
        }
    }
}

// cell e = (t, c) of this thread: out[e] = sum over the workgroups whose set holds t, in workgroup order.  A partial that
// was not written is not read; a workgroup without the type adds +0, which changes no bit of the sum.
__device__ __forceinline__ void finish_wide_body(const uint32_t* __restrict__ masks, const float4* __restrict__ partial,
                                                 int blocks, int n_types, int d4, float4* __restrict__ out, int bid) {
    const int cells = n_types * d4, e = bid * 256 + (int)threadIdx.x;
    if (e >= cells) return;
    const int t = e / d4, w = t >> 5;
    const uint32_t bit = 1u << (t & 31);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int b = 0; b < blocks; b += 4) {                  // 4 independent loads in flight, added in workgroup order
        float4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool has = b + k < blocks && (masks[4 * (b + k) + w] & bit);
            v[k] = has ? partial[(int64_t)(b + k) * cells + e] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) s.x += v[k].x, s.y += v[k].y, s.z += v[k].z, s.w += v[k].w;
    }
    out[e] = s;
}

}  // namespace type_rows
}  // namespace
