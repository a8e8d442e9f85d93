// Edge lengths and angles of graph construction, shared by the step-by-step kernels (graph.hip) and the molecule-local
// builder (graph_mol.hip) so that both produce the same floats.
#pragma once
#include "common.h"

__device__ __forceinline__ float dist3_xyz(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    // same association as (pos_i - pos_j).pow(2).sum(-1).sqrt() (models.py:65); no fma contraction
    const float s = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
    return __fsqrt_rn(s);
}

__device__ __forceinline__ float dist3(const float* __restrict__ pos, int64_t a, int64_t b) {
    return dist3_xyz(pos[3 * a + 0], pos[3 * a + 1], pos[3 * a + 2], pos[3 * b + 0], pos[3 * b + 1], pos[3 * b + 2]);
}

__device__ __forceinline__ float angle3(float ax, float ay, float az, float bx, float by, float bz) {
    // atan2(|a x b|, a.b)  (models.py:165-168); every product and sum rounded on its own (no contraction), so that the
    // value does not depend on the kernel the expression is inlined into
    const float dot = __fadd_rn(__fadd_rn(__fmul_rn(ax, bx), __fmul_rn(ay, by)), __fmul_rn(az, bz));
    const float cx = __fsub_rn(__fmul_rn(ay, bz), __fmul_rn(az, by));
    const float cy = __fsub_rn(__fmul_rn(az, bx), __fmul_rn(ax, bz));
    const float cz = __fsub_rn(__fmul_rn(ax, by), __fmul_rn(ay, bx));
    const float n2 = __fadd_rn(__fadd_rn(__fmul_rn(cx, cx), __fmul_rn(cy, cy)), __fmul_rn(cz, cz));
    return atan2f(__fsqrt_rn(n2), dot);
}

// ---- periodic cells: the one image rule ------------------------------------------------------------------------------
// A graph's row of the cell table (pamnet_cell_prepare_f64): 18 doubles, the cell (row k = lattice vector a_k) and then its
// inverse.  Every periodic kernel takes the displacement between two atoms of one graph from min_image() below and from
// nowhere else, with cell and inverse out of that one row, so no two kernels can choose different images of a pair.
constexpr int PBC_ROW = 18;
constexpr int PBC_BIT = 128;          // flag-word bit: a cell is singular or too small for the cutoff

struct PbcCell {
    double c[9], inv[9];
};

__device__ __forceinline__ PbcCell load_cell(const double* __restrict__ table, int64_t g) {
    PbcCell t;
#pragma unroll
    for (int k = 0; k < 9; ++k) t.c[k] = table[PBC_ROW * g + k], t.inv[k] = table[PBC_ROW * g + 9 + k];
    return t;
}

struct Disp {
    double x, y, z;
};

// Minimum-image displacement a - b: the fp64 difference of the two fp32 positions (exact), times the inverse cell, the three
// fractional components rounded to the nearest integer (the image n), n @ cell subtracted -- all in fp64, every step an
// explicit fma / product, so the value does not depend on the kernel the function is inlined into.  Every step is odd in
// (a - b): n(a, b) == -n(b, a) and the result negates exactly.  With n = 0 the result is the exact difference, whose
// rounding to fp32 is what the fp32 subtraction of the non-periodic kernels gives.
__device__ __forceinline__ Disp min_image(const PbcCell& t, float ax, float ay, float az, float bx, float by, float bz) {
    const double dx = (double)ax - (double)bx, dy = (double)ay - (double)by, dz = (double)az - (double)bz;
    const double n0 = rint(fma(dz, t.inv[6], fma(dy, t.inv[3], __dmul_rn(dx, t.inv[0]))));
    const double n1 = rint(fma(dz, t.inv[7], fma(dy, t.inv[4], __dmul_rn(dx, t.inv[1]))));
    const double n2 = rint(fma(dz, t.inv[8], fma(dy, t.inv[5], __dmul_rn(dx, t.inv[2]))));
    Disp d;
    d.x = fma(-n2, t.c[6], fma(-n1, t.c[3], fma(-n0, t.c[0], dx)));
    d.y = fma(-n2, t.c[7], fma(-n1, t.c[4], fma(-n0, t.c[1], dy)));
    d.z = fma(-n2, t.c[8], fma(-n1, t.c[5], fma(-n0, t.c[2], dz)));
    return d;
}

__device__ __forceinline__ Disp min_image(const PbcCell& t, const float* __restrict__ pos, int64_t a, int64_t b) {
    return min_image(t, pos[3 * a], pos[3 * a + 1], pos[3 * a + 2], pos[3 * b], pos[3 * b + 1], pos[3 * b + 2]);
}

// ---- all images (a global graph over every image within the cutoff) -------------------------------------------------------
// The displacement a - b - n @ cell for a GIVEN image n: min_image's statements with the rounding left out, in the same fma
// order, so with n = nearest_image(a, b) it returns min_image(a, b) bit for bit, and it negates exactly under (a, b, n) ->
// (b, a, -n).  n holds integers (exact in fp64 up to 2^53; the edge lists store them as int32).
__device__ __forceinline__ Disp image_disp(const PbcCell& t, float ax, float ay, float az, float bx, float by, float bz, double n0,
                                           double n1, double n2) {
    const double dx = (double)ax - (double)bx, dy = (double)ay - (double)by, dz = (double)az - (double)bz;
    Disp d;
    d.x = fma(-n2, t.c[6], fma(-n1, t.c[3], fma(-n0, t.c[0], dx)));
    d.y = fma(-n2, t.c[7], fma(-n1, t.c[4], fma(-n0, t.c[1], dy)));
    d.z = fma(-n2, t.c[8], fma(-n1, t.c[5], fma(-n0, t.c[2], dz)));
    return d;
}

// image_disp with the image read from row q of an edge list's [E, 3] int32 array
__device__ __forceinline__ Disp image_disp(const PbcCell& t, float ax, float ay, float az, float bx, float by, float bz,
                                           const int32_t* __restrict__ img, int64_t q) {
    return image_disp(t, ax, ay, az, bx, by, bz, (double)img[3 * q], (double)img[3 * q + 1], (double)img[3 * q + 2]);
}

// The image min_image() subtracts: its three rounding statements.  The all-image search centres its box of candidates here.
__device__ __forceinline__ void nearest_image(const PbcCell& t, float ax, float ay, float az, float bx, float by, float bz,
                                              double& n0, double& n1, double& n2) {
    const double dx = (double)ax - (double)bx, dy = (double)ay - (double)by, dz = (double)az - (double)bz;
    n0 = rint(fma(dz, t.inv[6], fma(dy, t.inv[3], __dmul_rn(dx, t.inv[0]))));
    n1 = rint(fma(dz, t.inv[7], fma(dy, t.inv[4], __dmul_rn(dx, t.inv[1]))));
    n2 = rint(fma(dz, t.inv[8], fma(dy, t.inv[5], __dmul_rn(dx, t.inv[2]))));
}

constexpr int IMG_BOX_MAX = 4;        // largest half-width of the candidate box per lattice direction (9^3 images per pair)

// How a kernel of graph construction turns two atoms into a displacement: open space (the raw difference, the arithmetic
// the kernels always had) or a periodic cell (the image rule, rounded once to fp32).  bind(): once per thread, for the graph
// its atoms belong to.
struct OpenSpace {
    __device__ __forceinline__ void bind(int) {}
    __device__ __forceinline__ float dist(const float* __restrict__ pos, int64_t a, int64_t b) const { return dist3(pos, a, b); }
    __device__ __forceinline__ float dist(float ax, float ay, float az, float bx, float by, float bz) const {
        return dist3_xyz(ax, ay, az, bx, by, bz);
    }
    __device__ __forceinline__ void sub(float ax, float ay, float az, float bx, float by, float bz, float& x, float& y,
                                        float& z) const {
        x = ax - bx, y = ay - by, z = az - bz;
    }
};

struct Periodic {
    const double* __restrict__ table;
    PbcCell t;
    __device__ __forceinline__ void bind(int g) { t = load_cell(table, g); }
    __device__ __forceinline__ float dist(const float* __restrict__ pos, int64_t a, int64_t b) const {
        const Disp d = min_image(t, pos, a, b);
        return dist3_xyz((float)d.x, (float)d.y, (float)d.z, 0.f, 0.f, 0.f);
    }
    __device__ __forceinline__ float dist(float ax, float ay, float az, float bx, float by, float bz) const {
        const Disp d = min_image(t, ax, ay, az, bx, by, bz);  // (the same statements on positions held in registers)
        return dist3_xyz((float)d.x, (float)d.y, (float)d.z, 0.f, 0.f, 0.f);
    }
    __device__ __forceinline__ void sub(float ax, float ay, float az, float bx, float by, float bz, float& x, float& y,
                                        float& z) const {
        const Disp d = min_image(t, ax, ay, az, bx, by, bz);
        x = (float)d.x, y = (float)d.y, z = (float)d.z;
    }
};
