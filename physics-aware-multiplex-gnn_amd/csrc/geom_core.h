// The geometry every kernel shares: edge lengths and angles of graph construction (the step-by-step kernels of graph.hip and the
// molecule-local builder of graph_mol.hip produce the same floats from them), the image rule of periodic cells, the policies
// that choose between open space and a cell in the construction kernels and in the position backward (forces.hip), and the
// cell's adjugate and heights.
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

// The batch's space as a kernel argument carries it: pointers only, each null where the policy does not read it.
struct Space {
    const double* cells;          // [n_graphs, 18] cell table (periodic policies)
    const int32_t* node_graph;    // [n] graph of every atom
    const int32_t* img;           // [eg, 3] image of every global edge (ImageDiff)
};

// The geometry policies.  A kernel default-constructs its policy, attach()es the launch's Space and bind()s the graph its
// atoms belong to, once per thread; bind() is where a periodic policy loads the graph's 18 doubles, so they never travel
// as a kernel argument.  Two families on purpose: graph construction needs the fp32 LENGTH the reference computes (rounded
// once from the image rule), the backward needs the fp64 VECTOR the derivative is taken along.

// Graph construction: open space (the raw difference, the arithmetic the kernels always had) or a periodic cell (the image
// rule, rounded once to fp32).
struct OpenSpace {
    __device__ __forceinline__ void attach(const Space&) {}
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
    __device__ __forceinline__ void attach(const Space& s) { table = s.cells; }
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

// The backward (forces.hip): p_a - p_b in fp64 -- the exact difference in open space, or the minimum-image displacement of a
// periodic cell: min_image, the function the forward's kernels chose the image with, not rounded to fp32 here.  The image
// integers do not depend on the positions differentiably, so every derivative is the open-space one.
struct V3 {
    double x, y, z;
};
__device__ __forceinline__ V3 v3(double x, double y, double z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 operator*(double s, V3 a) { return v3(s * a.x, s * a.y, s * a.z); }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
// every product rounded on its own (no fma contraction): for b = -a each component is then exactly 0, so |a x b| = 0
// takes the exact-zero branch of angle_grads instead of a residue whose direction is noise
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
    return v3(__dsub_rn(__dmul_rn(a.y, b.z), __dmul_rn(a.z, b.y)), __dsub_rn(__dmul_rn(a.z, b.x), __dmul_rn(a.x, b.z)),
              __dsub_rn(__dmul_rn(a.x, b.y), __dmul_rn(a.y, b.x)));
}
__device__ __forceinline__ V3 load_pos(const float* __restrict__ pos, int64_t i) {
    return v3((double)pos[3 * i], (double)pos[3 * i + 1], (double)pos[3 * i + 2]);
}

struct OpenDiff {
    __device__ __forceinline__ void attach(const Space&) {}
    __device__ __forceinline__ void bind(int) {}
    __device__ __forceinline__ V3 diff(const float* __restrict__ pos, int64_t a, int64_t b) const {
        return load_pos(pos, a) - load_pos(pos, b);
    }
    __device__ __forceinline__ V3 from(V3 pa, const float* __restrict__ pos, int64_t b) const { return pa - load_pos(pos, b); }
    // global edge q seen from atom a: its row (towards the column b), its column (towards the row b)
    __device__ __forceinline__ V3 row_edge(V3 pa, const float* __restrict__ pos, int64_t b, int64_t) const { return from(pa, pos, b); }
    __device__ __forceinline__ V3 col_edge(V3 pa, const float* __restrict__ pos, int64_t b, int64_t) const { return from(pa, pos, b); }
};
struct PeriodicDiff {
    const double* __restrict__ table;
    PbcCell t;
    __device__ __forceinline__ void attach(const Space& s) { table = s.cells; }
    __device__ __forceinline__ void bind(int g) { t = load_cell(table, g); }
    __device__ __forceinline__ V3 diff(const float* __restrict__ pos, int64_t a, int64_t b) const {
        const Disp d = min_image(t, pos, a, b);
        return v3(d.x, d.y, d.z);
    }
    // pa: an fp32 position held as doubles (load_pos)
    __device__ __forceinline__ V3 from(V3 pa, const float* __restrict__ pos, int64_t b) const {
        const Disp d = min_image(t, (float)pa.x, (float)pa.y, (float)pa.z, pos[3 * b], pos[3 * b + 1], pos[3 * b + 2]);
        return v3(d.x, d.y, d.z);
    }
    __device__ __forceinline__ V3 row_edge(V3 pa, const float* __restrict__ pos, int64_t b, int64_t) const { return from(pa, pos, b); }
    __device__ __forceinline__ V3 col_edge(V3 pa, const float* __restrict__ pos, int64_t b, int64_t) const { return from(pa, pos, b); }
};
// A periodic graph whose GLOBAL list holds every image within the cutoff (pamnet_radius_img_fill_i32): global edge q is the vector
// v_q = p_row - p_col - img[q] @ cell of its stored image, not a rounded one (image_disp).  Seen from its column the edge is
// -v_q.  Local edges, and so diff / from, stay minimum-image.
struct ImageDiff : PeriodicDiff {
    const int32_t* __restrict__ img;
    __device__ __forceinline__ void attach(const Space& s) { table = s.cells, img = s.img; }
    __device__ __forceinline__ V3 row_edge(V3 pa, const float* __restrict__ pos, int64_t b, int64_t q) const {
        const Disp d = image_disp(t, (float)pa.x, (float)pa.y, (float)pa.z, pos[3 * b], pos[3 * b + 1], pos[3 * b + 2], img, q);
        return v3(d.x, d.y, d.z);
    }
    __device__ __forceinline__ V3 col_edge(V3 pa, const float* __restrict__ pos, int64_t b, int64_t q) const {
        const Disp d = image_disp(t, pos[3 * b], pos[3 * b + 1], pos[3 * b + 2], (float)pa.x, (float)pa.y, (float)pa.z, img, q);
        return v3(-d.x, -d.y, -d.z);
    }
};

// ---- the cell's perpendicular heights ------------------------------------------------------------------------------------
// x[k] = a_{k+1} x a_{k+2}: column k of the adjugate of the cell a (row k = lattice vector a_k); returns det = a_0 . x[0].
__device__ __forceinline__ double cell_adjugate(const double* a, double (&x)[3][3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double* u = a + 3 * ((k + 1) % 3);
        const double* v = a + 3 * ((k + 2) % 3);
        x[k][0] = u[1] * v[2] - u[2] * v[1];
        x[k][1] = u[2] * v[0] - u[0] * v[2];
        x[k][2] = u[0] * v[1] - u[1] * v[0];
    }
    const double det = a[0] * x[0][0] + a[1] * x[0][1] + a[2] * x[0][2];
    return det;
}

// h_k = |det| / |a_{k+1} x a_{k+2}|: the cell's extent perpendicular to the faces that lattice direction k crosses.  The
// one height rule: the cell table judges h_k > 2 * cutoff with it, the image box takes N_k = ceil(cutoff / h_k) from it.
__device__ __forceinline__ double cell_height(const double (&x)[3][3], double det, int k) {
    const double area = sqrt(x[k][0] * x[k][0] + x[k][1] * x[k][1] + x[k][2] * x[k][2]);
    return fabs(det) / area;
}

// workgroups of 256 threads for n items, `per` items a workgroup (a wavefront per item: per = 4); never an empty grid
inline unsigned blocks_for(int64_t n, int per = 256) { return (unsigned)(n > 0 ? ceil_div(n, per) : 1); }
