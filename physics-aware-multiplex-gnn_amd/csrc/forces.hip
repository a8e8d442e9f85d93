// Geometric backward of graph construction: gradients of the edge lengths and triplet / pair angles (models.py:65,
// 165-177) with respect to the atom positions -- what d prediction / d pos (the negated forces) needs after the basis
// backward (pamnet_rbf_ddist_f32, pamnet_sbf_bwd_f32) has turned the embedding input gradients into d dist / d angle.
//
// Every row t of the triplet / pair list angles two bond vectors.  With u_e = p[src e] - p[dst e] for local edge e, row t of
// target edge e and source edge e' has a = u_e (triplet: p_j - p_i) or a = -u_e (pair: p_i - p_j), and b = u_e' (p_k - p_j,
// resp. p_j' - p_i): the forward's own operands (graph.hip triplet_fill_kernel).  So the angle gradients fold into one
// 3-vector per local edge, and the positions gather those per atom.  No atomics: every sum runs over a CSR row or a
// transposed row list in a fixed order, so the result is bitwise the same from run to run.  Arithmetic in fp64.
//
// Periodic cells also give the virial W[g] = d prediction / d strain at zero strain (pamnet_pos_bwd_pbc_virial_f32): the sum over
// every directed edge of (minimum-image vector) (x) (gradient with respect to that vector).  Both factors exist only here, in
// fp64 and per wavefront, so the atom's wavefront of the position backward forms its rows' share beside dpos (the VIRIAL
// instantiation of pos_grad) and one workgroup per graph adds the atoms' shares in a fixed-order tree (virial_reduce_kernel).
// pos^T dE/dpos + cell^T dE/dcell is the same number but cancels: its terms grow with every lattice vector an atom is
// displaced by, the edge form does not see where an atom was wrapped to.
#include "common.h"
#include "geom_core.h"

namespace {

// (V3 and its algebra, load_pos and the policies OpenDiff / PeriodicDiff / ImageDiff: geom_core.h)

// The lists of the backward, as the kernels take them (by value, inside the records below).
struct Csr {                      // rows by pointer, one (row, col) per entry
    const int32_t *ptr, *row, *col;
};
struct CsrT {                     // its transpose: rows by pointer, the entries' positions in the list
    const int32_t *ptr, *perm;
};
struct BondGradArgs {
    const float* pos;
    Space space;
    Csr l;                        // local edges (ptr unused)
    const float* ddist;
    int64_t el;
    Csr t;                        // triplet / pair rows: ptr by target edge, row = target edge, col = source edge
    const int32_t* t_kind;
    CsrT tt;
    const float* dangle;
    double* G;                    // [el, 3] out
};
struct PosGradArgs {
    const float* pos;
    Space space;
    int64_t n;
    Csr g;
    CsrT gt;
    const float* ddist_g;
    Csr l;                        // (row unused)
    CsrT lt;
    const double* G;
    float* dpos;
    double* atom_work;            // VIRIAL: [n, 9] out
};

// u_e = p[src] - p[dst] of local edge e (loc: rows = dst, col = src)
template <class GEOM>
__device__ __forceinline__ V3 bond(const GEOM& geom, const float* __restrict__ pos, const int32_t* __restrict__ l_row,
                                   const int32_t* __restrict__ l_col, int64_t e) {
    return geom.diff(pos, l_col[e], l_row[e]);
}

// theta = atan2(|a x b|, a.b):  d theta / d a = (a.b (b x c) / |c| - |c| b) / s,  d theta / d b = (a.b (c x a) / |c| - |c| a) / s,
// c = a x b, s = |c|^2 + (a.b)^2.  Where |c| = 0 (every pair row whose two bonds are the same edge: b = -a, theta = pi) the
// cross-product term is exactly 0, as torch's norm backward makes it; s = 0 (a zero bond) gives 0 too.
__device__ __forceinline__ void angle_grads(V3 a, V3 b, double g, V3* ga, V3* gb) {
    const V3 c = cross(a, b);
    const double cn = sqrt(dot(c, c)), d = dot(a, b);
    const double s = cn * cn + d * d;
    if (!(s > 0.0)) {
        *ga = *gb = v3(0.0, 0.0, 0.0);
        return;
    }
    const double k = g / s;
    V3 ta = (-cn) * b, tb = (-cn) * a;
    if (cn > 0.0) {
        const double kc = d / cn;
        ta = ta + kc * cross(b, c);
        tb = tb + kc * cross(c, a);
    }
    *ga = k * ta;
    *gb = k * tb;
}

// fixed-order butterfly over the 64 lanes of a wavefront (every lane ends with the same sum): deterministic
__device__ __forceinline__ V3 wave_sum(V3 v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = v3(v.x + __shfl_xor(v.x, o, 64), v.y + __shfl_xor(v.y, o, 64), v.z + __shfl_xor(v.z, o, 64));
    return v;
}

// One wavefront per local edge e: G_e = d/d u_e of everything that depends on u_e -- its length, the rows of e (operand a)
// and the rows that gather e (operand b, transposed row list); the lanes stride over the rows.
template <class GEOM>
__device__ __forceinline__ void bond_grad(GEOM geom, const int32_t* __restrict__ node_graph, const float* __restrict__ pos,
                                          const int32_t* __restrict__ l_row, const int32_t* __restrict__ l_col,
                                          const float* __restrict__ ddist, int64_t el, const int32_t* __restrict__ t_ptr,
                                          const int32_t* __restrict__ t_row, const int32_t* __restrict__ t_col,
                                          const int32_t* __restrict__ t_kind, const int32_t* __restrict__ tt_ptr,
                                          const int32_t* __restrict__ tt_perm, const float* __restrict__ dangle,
                                          double* __restrict__ G) {
    const int64_t e = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (e >= el) return;                                          // (uniform over the wavefront)
    if (node_graph) geom.bind(node_graph[l_row[e]]);              // (every bond of e's rows lies in e's graph)
    const V3 u = bond(geom, pos, l_row, l_col, e);
    V3 acc = v3(0.0, 0.0, 0.0);
    if (lane == 0) {
        const double r = sqrt(dot(u, u));
        if (r > 0.0) acc = ((double)ddist[e] / r) * u;
    }
    for (int t = t_ptr[e] + lane; t < t_ptr[e + 1]; t += 64) {   // rows of e: a = +-u_e
        const double sg = t_kind[t] == 0 ? 1.0 : -1.0;
        V3 ga, gb;
        angle_grads(sg * u, bond(geom, pos, l_row, l_col, t_col[t]), (double)dangle[t], &ga, &gb);
        acc = acc + sg * ga;
    }
    for (int k = tt_ptr[e] + lane; k < tt_ptr[e + 1]; k += 64) { // rows gathering e: b = u_e
        const int64_t t = tt_perm[k];
        const double sg = t_kind[t] == 0 ? 1.0 : -1.0;
        V3 ga, gb;
        angle_grads(sg * bond(geom, pos, l_row, l_col, t_row[t]), u, (double)dangle[t], &ga, &gb);
        acc = acc + gb;
    }
    acc = wave_sum(acc);
    if (lane == 0) {
        G[3 * e] = acc.x;
        G[3 * e + 1] = acc.y;
        G[3 * e + 2] = acc.z;
    }
}

template <class GEOM>
__global__ __launch_bounds__(256) void bond_grad_kernel(BondGradArgs a) {
    GEOM geom;
    geom.attach(a.space);
    bond_grad(geom, a.space.node_graph, a.pos, a.l.row, a.l.col, a.ddist, a.el, a.t.ptr, a.t.row, a.t.col, a.t_kind, a.tt.ptr,
              a.tt.perm, a.dangle, a.G);
}

// One wavefront per atom a, the lanes striding over: the global edges of row a and of column a (transposed list), then the
// bond gradients of the local edges leaving a (+G) and arriving at a (-G).
// VIRIAL: the wavefront also sums v (x) dE/dv over the edges of ROW a alone (each directed edge belongs to one row, so each is
// counted once): w (x) (ddist_g / r) w of its global edges -- symmetric, six products -- and u_e (x) G_e of its local edges, and
// writes the nine sums to atom_work[a].  dpos comes from the same statements in the same order either way.
template <class GEOM, bool VIRIAL>
__device__ __forceinline__ void pos_grad(GEOM geom, const int32_t* __restrict__ node_graph, const float* __restrict__ pos,
                                         int64_t n, const int32_t* __restrict__ g_ptr, const int32_t* __restrict__ g_row,
                                         const int32_t* __restrict__ g_col, const int32_t* __restrict__ gt_ptr,
                                         const int32_t* __restrict__ gt_perm, const float* __restrict__ ddist_g,
                                         const int32_t* __restrict__ l_ptr, const int32_t* __restrict__ lt_ptr,
                                         const int32_t* __restrict__ lt_perm, const double* __restrict__ G,
                                         float* __restrict__ dpos, const int32_t* __restrict__ l_col = nullptr,
                                         double* __restrict__ atom_work = nullptr) {
    const int64_t a = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (a >= n) return;                                           // (uniform over the wavefront)
    if (node_graph) geom.bind(node_graph[a]);
    const V3 pa = load_pos(pos, a);
    V3 acc = v3(0.0, 0.0, 0.0);
    V3 vx = v3(0.0, 0.0, 0.0), vy = vx, vz = vx;                  // VIRIAL: rows of the 3 x 3 sum
    for (int q = g_ptr[a] + lane; q < g_ptr[a + 1]; q += 64) {
        const V3 w = geom.row_edge(pa, pos, g_col[q], q);
        const double r = sqrt(dot(w, w));
        if (r > 0.0) {
            const V3 f = ((double)ddist_g[q] / r) * w;
            acc = acc + f;
            if constexpr (VIRIAL) {
                const double xy = w.x * f.y, xz = w.x * f.z, yz = w.y * f.z;
                vx = vx + v3(w.x * f.x, xy, xz);
                vy = vy + v3(xy, w.y * f.y, yz);
                vz = vz + v3(xz, yz, w.z * f.z);
            }
        }
    }
    for (int k = gt_ptr[a] + lane; k < gt_ptr[a + 1]; k += 64) {
        const int64_t q = gt_perm[k];
        const V3 w = geom.col_edge(pa, pos, g_row[q], q);
        const double r = sqrt(dot(w, w));
        if (r > 0.0) acc = acc + ((double)ddist_g[q] / r) * w;
    }
    for (int k = lt_ptr[a] + lane; k < lt_ptr[a + 1]; k += 64) {
        const int64_t e = lt_perm[k];
        acc = acc + v3(G[3 * e], G[3 * e + 1], G[3 * e + 2]);
    }
    for (int e = l_ptr[a] + lane; e < l_ptr[a + 1]; e += 64) {
        const V3 ge = v3(G[3 * e], G[3 * e + 1], G[3 * e + 2]);
        acc = acc - ge;
        if constexpr (VIRIAL) {
            const V3 u = geom.diff(pos, l_col[e], a);             // u_e = p[src] - p[dst], dst = a
            vx = vx + u.x * ge;
            vy = vy + u.y * ge;
            vz = vz + u.z * ge;
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) {
        dpos[3 * a] = (float)acc.x;
        dpos[3 * a + 1] = (float)acc.y;
        dpos[3 * a + 2] = (float)acc.z;
    }
    if constexpr (VIRIAL) {
        vx = wave_sum(vx), vy = wave_sum(vy), vz = wave_sum(vz);
        if (lane == 0) {
            double* __restrict__ o = atom_work + 9 * a;
            o[0] = vx.x, o[1] = vx.y, o[2] = vx.z;
            o[3] = vy.x, o[4] = vy.y, o[5] = vy.z;
            o[6] = vz.x, o[7] = vz.y, o[8] = vz.z;
        }
    }
}

template <class GEOM, bool VIRIAL>
__global__ __launch_bounds__(256) void pos_grad_kernel(PosGradArgs a) {
    GEOM geom;
    geom.attach(a.space);
    pos_grad<GEOM, VIRIAL>(geom, a.space.node_graph, a.pos, a.n, a.g.ptr, a.g.row, a.g.col, a.gt.ptr, a.gt.perm, a.ddist_g, a.l.ptr,
                           a.lt.ptr, a.lt.perm, a.G, a.dpos, a.l.col, a.atom_work);
}

// One workgroup of 256 threads per graph g: the threads stride over the atoms gptr[g] .. gptr[g + 1] of atom_work (kept inside
// [0, n]) with nine fp64 sums each, then a fixed-order tree -- the wavefront butterfly, the four wavefronts through LDS -- and
// thread 0 rounds the nine values once to fp32.  A graph without atoms or without edges gets exact zeros.
__global__ __launch_bounds__(256) void virial_reduce_kernel(const double* __restrict__ atom_work,
                                                            const int32_t* __restrict__ gptr, int64_t n,
                                                            float* __restrict__ dstrain) {
    __shared__ double part[4][9];
    const int64_t g = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t lo = gptr[g], hi = gptr[g + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n ? n : hi;
    V3 vx = v3(0.0, 0.0, 0.0), vy = vx, vz = vx;
    for (int64_t a = lo + tid; a < hi; a += 256) {
        const double* __restrict__ w = atom_work + 9 * a;
        vx = vx + v3(w[0], w[1], w[2]);
        vy = vy + v3(w[3], w[4], w[5]);
        vz = vz + v3(w[6], w[7], w[8]);
    }
    vx = wave_sum(vx), vy = wave_sum(vy), vz = wave_sum(vz);
    if (lane == 0) {
        double* o = part[wave];
        o[0] = vx.x, o[1] = vx.y, o[2] = vx.z;
        o[3] = vy.x, o[4] = vy.y, o[5] = vy.z;
        o[6] = vz.x, o[7] = vz.y, o[8] = vz.z;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) dstrain[9 * g + k] = (float)((part[0][k] + part[1][k]) + (part[2][k] + part[3][k]));
    }
}

// Everything a position backward reads and writes; the five entry points fill it.
struct PosBwdArgs {
    const float* pos;
    Space space;
    int64_t n;
    Csr g;
    CsrT gt;
    const float* ddist_g;
    int64_t eg;
    Csr l;
    CsrT lt;
    const float* ddist_l;
    int64_t el;
    Csr t;
    const int32_t* t_kind;
    CsrT tt;
    const float* dangle;
    int64_t tp;
    double* bond_work;
    float* dpos;
    const int32_t* gptr;          // the virial forms' four, else null / 0
    int64_t n_graphs;
    double* atom_work;
    float* dstrain;
};

enum class SpaceKind { Open, Periodic, Images };

bool has(const Csr& c) { return c.ptr && c.row && c.col; }
bool has(const CsrT& c) { return c.ptr && c.perm; }

// bond_grad (when there are local edges) -> pos_grad -> virial_reduce (the virial forms; also without atoms: every graph's
// atom range is then empty and dstrain becomes zeros).  A null pointer is PAMNET_EINVAL here, judged before n == 0.
int pos_bwd(const PosBwdArgs& a, SpaceKind kind, bool virial, pamnet_stream_t stream) {
    if (a.n < 0 || a.eg < 0 || a.el < 0 || a.tp < 0 || a.n_graphs < 0) return PAMNET_EINVAL;
    if (!a.pos || !has(a.g) || !has(a.gt) || !a.ddist_g || !has(a.l) || !has(a.lt) || !a.ddist_l || !has(a.t) || !a.t_kind ||
        !has(a.tt) || !a.dangle || !a.bond_work || !a.dpos)
        return PAMNET_EINVAL;
    if (kind != SpaceKind::Open && (!a.space.cells || !a.space.node_graph)) return PAMNET_EINVAL;
    if (kind == SpaceKind::Images && !a.space.img) return PAMNET_EINVAL;
    if (virial && (!a.gptr || !a.atom_work || !a.dstrain)) return PAMNET_EINVAL;
    hipStream_t st = as_stream(stream);
    const bool open = kind == SpaceKind::Open, img = kind == SpaceKind::Images;
    if (a.n > 0) {
        if (a.el > 0) {                                           // (local edges are minimum-image in both periodic spaces)
            const BondGradArgs b{a.pos, a.space, a.l, a.ddist_l, a.el, a.t, a.t_kind, a.tt, a.dangle, a.bond_work};
            void (*kernel)(BondGradArgs) = open ? bond_grad_kernel<OpenDiff> : bond_grad_kernel<PeriodicDiff>;
            hipLaunchKernelGGL(kernel, dim3(blocks_for(a.el, 4)), dim3(256), 0, st, b);
            PAMNET_LAUNCH_CHECK();
        }
        const PosGradArgs p{a.pos, a.space, a.n, a.g, a.gt, a.ddist_g, a.l, a.lt, a.bond_work, a.dpos, a.atom_work};
        void (*kernel)(PosGradArgs) = open     ? pos_grad_kernel<OpenDiff, false>
                                      : virial ? (img ? pos_grad_kernel<ImageDiff, true> : pos_grad_kernel<PeriodicDiff, true>)
                                               : (img ? pos_grad_kernel<ImageDiff, false> : pos_grad_kernel<PeriodicDiff, false>);
        hipLaunchKernelGGL(kernel, dim3(blocks_for(a.n, 4)), dim3(256), 0, st, p);
        PAMNET_LAUNCH_CHECK();
    }
    if (virial && a.n_graphs > 0) {
        hipLaunchKernelGGL(virial_reduce_kernel, dim3((unsigned)a.n_graphs), dim3(256), 0, st, a.atom_work, a.gptr, a.n, a.dstrain);
        PAMNET_LAUNCH_CHECK();
    }
    return PAMNET_OK;
}

}  // namespace

extern "C" int pamnet_pos_bwd_f32(const float* pos, int64_t n, const int32_t* g_ptr, const int32_t* g_row,
                                  const int32_t* g_col, const int32_t* gt_ptr, const int32_t* gt_perm, const float* ddist_g,
                                  int64_t eg, const int32_t* l_ptr, const int32_t* l_row, const int32_t* l_col,
                                  const int32_t* lt_ptr, const int32_t* lt_perm, const float* ddist_l, int64_t el,
                                  const int32_t* t_ptr, const int32_t* t_row, const int32_t* t_col, const int32_t* t_kind,
                                  const int32_t* tt_ptr, const int32_t* tt_perm, const float* dangle, int64_t tp,
                                  double* bond_work, float* dpos, pamnet_stream_t stream) {
    const PosBwdArgs a{pos, {}, n, {g_ptr, g_row, g_col}, {gt_ptr, gt_perm}, ddist_g, eg,
                       {l_ptr, l_row, l_col}, {lt_ptr, lt_perm}, ddist_l, el,
                       {t_ptr, t_row, t_col}, t_kind, {tt_ptr, tt_perm}, dangle, tp, bond_work, dpos};
    return pos_bwd(a, SpaceKind::Open, false, stream);
}

extern "C" int pamnet_pos_bwd_pbc_f32(const float* pos, const double* cell_table, const int32_t* node_graph, int64_t n,
                                      const int32_t* g_ptr, const int32_t* g_row, const int32_t* g_col, const int32_t* gt_ptr,
                                      const int32_t* gt_perm, const float* ddist_g, int64_t eg, const int32_t* l_ptr,
                                      const int32_t* l_row, const int32_t* l_col, const int32_t* lt_ptr, const int32_t* lt_perm,
                                      const float* ddist_l, int64_t el, const int32_t* t_ptr, const int32_t* t_row,
                                      const int32_t* t_col, const int32_t* t_kind, const int32_t* tt_ptr, const int32_t* tt_perm,
                                      const float* dangle, int64_t tp, double* bond_work, float* dpos, pamnet_stream_t stream) {
    const PosBwdArgs a{pos, {cell_table, node_graph, nullptr}, n, {g_ptr, g_row, g_col}, {gt_ptr, gt_perm}, ddist_g, eg,
                       {l_ptr, l_row, l_col}, {lt_ptr, lt_perm}, ddist_l, el,
                       {t_ptr, t_row, t_col}, t_kind, {tt_ptr, tt_perm}, dangle, tp, bond_work, dpos};
    return pos_bwd(a, SpaceKind::Periodic, false, stream);
}

extern "C" int pamnet_pos_bwd_pbc_virial_f32(const float* pos, const double* cell_table, const int32_t* node_graph, int64_t n,
                                             const int32_t* g_ptr, const int32_t* g_row, const int32_t* g_col,
                                             const int32_t* gt_ptr, const int32_t* gt_perm, const float* ddist_g, int64_t eg,
                                             const int32_t* l_ptr, const int32_t* l_row, const int32_t* l_col,
                                             const int32_t* lt_ptr, const int32_t* lt_perm, const float* ddist_l, int64_t el,
                                             const int32_t* t_ptr, const int32_t* t_row, const int32_t* t_col,
                                             const int32_t* t_kind, const int32_t* tt_ptr, const int32_t* tt_perm,
                                             const float* dangle, int64_t tp, double* bond_work, float* dpos, const int32_t* gptr,
                                             int64_t n_graphs, double* atom_work, float* dstrain, pamnet_stream_t stream) {
    const PosBwdArgs a{pos, {cell_table, node_graph, nullptr}, n, {g_ptr, g_row, g_col}, {gt_ptr, gt_perm}, ddist_g, eg,
                       {l_ptr, l_row, l_col}, {lt_ptr, lt_perm}, ddist_l, el,
                       {t_ptr, t_row, t_col}, t_kind, {tt_ptr, tt_perm}, dangle, tp, bond_work, dpos,
                       gptr, n_graphs, atom_work, dstrain};
    return pos_bwd(a, SpaceKind::Periodic, true, stream);
}

extern "C" int pamnet_pos_bwd_img_f32(const float* pos, const double* cell_table, const int32_t* node_graph, int64_t n,
                                      const int32_t* g_ptr, const int32_t* g_row, const int32_t* g_col, const int32_t* g_img,
                                      const int32_t* gt_ptr, const int32_t* gt_perm, const float* ddist_g, int64_t eg,
                                      const int32_t* l_ptr, const int32_t* l_row, const int32_t* l_col, const int32_t* lt_ptr,
                                      const int32_t* lt_perm, const float* ddist_l, int64_t el, const int32_t* t_ptr,
                                      const int32_t* t_row, const int32_t* t_col, const int32_t* t_kind, const int32_t* tt_ptr,
                                      const int32_t* tt_perm, const float* dangle, int64_t tp, double* bond_work, float* dpos,
                                      pamnet_stream_t stream) {
    const PosBwdArgs a{pos, {cell_table, node_graph, g_img}, n, {g_ptr, g_row, g_col}, {gt_ptr, gt_perm}, ddist_g, eg,
                       {l_ptr, l_row, l_col}, {lt_ptr, lt_perm}, ddist_l, el,
                       {t_ptr, t_row, t_col}, t_kind, {tt_ptr, tt_perm}, dangle, tp, bond_work, dpos};
    return pos_bwd(a, SpaceKind::Images, false, stream);
}

extern "C" int pamnet_pos_bwd_img_virial_f32(const float* pos, const double* cell_table, const int32_t* node_graph, int64_t n,
                                             const int32_t* g_ptr, const int32_t* g_row, const int32_t* g_col,
                                             const int32_t* g_img, const int32_t* gt_ptr, const int32_t* gt_perm,
                                             const float* ddist_g, int64_t eg, const int32_t* l_ptr, const int32_t* l_row,
                                             const int32_t* l_col, const int32_t* lt_ptr, const int32_t* lt_perm,
                                             const float* ddist_l, int64_t el, const int32_t* t_ptr, const int32_t* t_row,
                                             const int32_t* t_col, const int32_t* t_kind, const int32_t* tt_ptr,
                                             const int32_t* tt_perm, const float* dangle, int64_t tp, double* bond_work, float* dpos,
                                             const int32_t* gptr, int64_t n_graphs, double* atom_work, float* dstrain,
                                             pamnet_stream_t stream) {
    const PosBwdArgs a{pos, {cell_table, node_graph, g_img}, n, {g_ptr, g_row, g_col}, {gt_ptr, gt_perm}, ddist_g, eg,
                       {l_ptr, l_row, l_col}, {lt_ptr, lt_perm}, ddist_l, el,
                       {t_ptr, t_row, t_col}, t_kind, {tt_ptr, tt_perm}, dangle, tp, bond_work, dpos,
                       gptr, n_graphs, atom_work, dstrain};
    return pos_bwd(a, SpaceKind::Images, true, stream);
}
