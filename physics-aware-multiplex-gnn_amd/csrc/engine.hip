// Layer-stack engine: the whole n_layer x (global, local) message-passing loop of PAMNet.forward (models.py:196-204)
// -- forward or backward -- enqueued by ONE C call.
//
// The reference drives this loop from Python, one small op at a time (~150 launches per layer pair); even with fused
// kernels a Python-level loop leaves the MI355X idle behind the interpreter.  Here the host side is a straight C++
// sequence of ~7 (forward) / ~16 (backward) kernel launches per layer pair on the caller's stream, working out of two
// caller-owned arenas:
//   saved : activations the backward needs (pre-activations, gates, residual taps), one slab per layer
//   temp  : scratch reused by every layer (projections, messages, gradient staging, split-K partials)
// Nothing is allocated, no state is kept, nothing synchronises: the caller sizes the arenas with
// pamnet_stack_workspace and keeps them alive until the backward has been enqueued.
// The shared edge embeddings (e_g, rbf_e, e_sbf feed all layers) get their gradients accumulated in place by the
// backward kernels themselves (accumulate flag), in a fixed layer order -> deterministic.
//
// Three pieces of bookkeeping, each stated once: Switches (everything this file reads from the environment), Plan (which
// kernel forms a call runs: make_plan) and Arena (where every slab of the two arenas lies: make_arena, the one walk the
// reported sizes come from as well).  Parameter-table slots go by the names of common.h (pslot).

#include <stdlib.h>

#include <vector>

#include "common.h"
#include "node_chain_args.h"

namespace {

using namespace pslot;

constexpr int64_t D = 128;

struct Graph {
    int64_t n, eg, el, tp;
    const int32_t *g_ptr, *g_row, *g_col, *gT_ptr, *gT_perm;
    const int32_t *l_ptr, *l_row, *l_col, *lT_ptr, *lT_perm;
    const int32_t *t_ptr, *t_row, *t_col, *tT_ptr, *tT_perm;
    const int32_t* cuts;      // nullable: the fused global-edge kernels' work split, made with the graph (pamnet_seg_cuts_i32)
    const int32_t *tT_edge, *tT_node;   // nullable pair: pamnet_triplet_transpose_aux_i32 (the local aggregation's backward gather)
};

#define CK(call)                 \
    do {                         \
        int rc__ = (call);       \
        if (rc__) return rc__;   \
    } while (0)

#define HK(call)                                   \
    do {                                           \
        const hipError_t e__ = (call);             \
        if (e__ != hipSuccess) return (int)e__;    \
    } while (0)

// ---- switches -----------------------------------------------------------------------------------------------------------
// Every developer switch of this file, read once (on the first engine call of the process).  All are A/B aids: each form
// they select gives the same step, most of them bit for bit (tests/test_hip_model.py).
inline int64_t env_num(const char* name, int64_t unset) {
    const char* e = getenv(name);
    return e ? (int64_t)atoll(e) : unset;
}
struct Switches {
    // PAMNET_EDGE_RECOMPUTE=1 ("backward by recompute"): the training forward of the fused global-edge step saves nothing of
    // edge size (it runs the inference form: no z, no ea), only the two node planes P_i, P_j it gathered from; the backward
    // re-runs the forward kernel for z and ea into scratch right ahead of the fused backward kernel.  Same numbers bit for bit
    // (the same kernel computes them), 2 x E_g x 512 bytes less per layer in the saved arena; it is not faster
    // (profiles/r06_edge_recompute_ab.txt).  Only where the backward takes its fused weight-gradient form (the scratch it
    // frees holds the recomputed rows).
    bool edge_recompute = env_num("PAMNET_EDGE_RECOMPUTE", 0) != 0;
    // PAMNET_EDGE_WGRAD=0 / 1: the weight gradients of the global edge step (dW_e = dz^T e_g, dW_ea = dea^T e_g) as two
    // E_g-row jobs of the split-K launches / formed inside the fused backward edge kernel (edge_agg.hip
    // global_edge_agg_bwd_wg_kernel).  Unset (-1): the latter where a workgroup has enough rows to amortise its two 64 KB
    // partial tiles (STREAMED_EDGES_FROM).
    int edge_wgrad = (int)env_num("PAMNET_EDGE_WGRAD", -1);
    // PAMNET_EDGE_IMAGES=0: the edge-level kernels split their fp32 weight slices themselves instead of reading the step's
    // bf16x3 fragment images.  The images need the 8-wave geometry of the local edge kernel (PAMNET_EDGE_WAVES=4 forces the
    // other one: no images then).
    bool edge_images = env_num("PAMNET_EDGE_IMAGES", 1) != 0 && env_num("PAMNET_EDGE_WAVES", 0) != 4;
    // PAMNET_FUSE_SEGSUM=0: the segment sums that feed a fused head + chain backward launch (the source-side sum of the global
    // layer's d z, the four sums of the local layer) as launches of their own ahead of it, instead of formed by that launch's
    // own row tiles (node_tail.hip gather_begin / gather_finish): two launches more per layer pair on the dependent chain.
    bool fuse_segsum = env_num("PAMNET_FUSE_SEGSUM", 1) != 0;
    // PAMNET_FUSE_LOCAL_AGG=0: the local layer's two chained aggregations as a launch of their own (pamnet_local_agg_fwd_f32)
    // instead of formed by the row tiles of the chain launch that consumes them (node_tail.hip local_agg_rows).
    bool fuse_local_agg = env_num("PAMNET_FUSE_LOCAL_AGG", 1) != 0;
    // PAMNET_CHAIN_BF16=0: the chains of single-round batches on fp32 MFMAs; 2: only the forward ones on the bf16 pipe.
    // Default: both directions as bf16x6 piece products at fp32 accuracy (node_tail_fwd_bf16_kernel /
    // node_tail_bwd_bf16_kernel, bf16x3 weight images): 768 instead of 2 048 matrix-pipe cycles per layer; a 7-layer chain is
    // 23 500 cycles against 27 500 and the QM9 step 1.954 against 1.989 ms same box (profiles/r06_chain_bf16.txt); same
    // outputs to 3e-7 (tests/test_hip_fused.py::test_node_tail_fwd_bf16x6).
    int chain_bf16 = (int)env_num("PAMNET_CHAIN_BF16", 1);
    // PAMNET_CHAIN_BF16_TILES=N: row tiles up to which the bf16x6 chains run (default PARKED_TILES_MAX: they park a tile's
    // state in LDS, one workgroup per CU -- single-round batches); for measurements.
    int64_t bf16_tiles = env_num("PAMNET_CHAIN_BF16_TILES", PARKED_TILES_MAX);
    // PAMNET_TT_AUX=0: ignore the precomputed gather indices of the local aggregation's backward (A/B timing)
    bool tt_aux = env_num("PAMNET_TT_AUX", 1) != 0;
};
inline const Switches& switches() {
    static const Switches s;
    return s;
}

// ---- launch plan --------------------------------------------------------------------------------------------------------
// Riders: work that does not depend on a node-chain launch runs as extra workgroups of it, on the CUs its ceil(n/16) row
// tiles leave idle.  They pay when the chain leaves enough CUs for slots of a few hundred rows: <= 176 row tiles.
constexpr int RIDER_MAX_SLOTS = 256;
constexpr int RIDER_JOBS = 10;      // all ten tail jobs of a chain ride (fewer riders, the rest in the layer's own launch, measured slower)

enum Dir { FWD, BWD };

// Which kernel forms one engine call runs.  Filled once at the top of the call from the sizes, the caller's arenas and
// the switches; edge_wgrad and recompute also shape the arenas (make_arena), so the size queries fill one too.
struct Plan {
    int64_t tiles;        // row tiles of a node-chain launch = its workgroups
    int64_t idle;         // CUs such a launch leaves to riders
    bool packed;          // the caller gave a weight-image arena: the chains read fragment images, and the backward runs a
                          // layer's head inside the launch of the chain that produced the layer's input
    bool forked;          // forward: the triplet/pair MLPs run on the caller's auxiliary stream
    bool edge_wgrad;      // the global edge backward forms its own weight gradients
    bool recompute;       // ... and recomputes z / ea instead of reading saved ones
    bool ride;            // the chain launches carry riders (see make_plan: the two directions carry different work)
    bool bf16;            // this direction's chains run as bf16x6 piece products (bf16x3 images)
    bool gimg, limg;      // the global / the local edge step of this direction reads fragment images
    bool agg_in;          // forward: the local aggregations are formed by the chain launch that consumes them
    bool gather;          // backward: the segment sums are formed by the fused head + chain launch that consumes them
    int32_t pk, pkc;      // what a launch is told about its weights: 0 raw, 1 fp32 images; the chains' own: 2 = bf16x3 images
};

inline Plan make_plan(const Graph& g, bool packed, bool forked, Dir dir) {
    const Switches& sw = switches();
    Plan p{};
    p.tiles = ceil_div(g.n, NODE_TILE_ROWS);
    p.idle = RIDER_MAX_SLOTS - p.tiles;
    p.packed = packed, p.forked = forked;
    const bool fits = g.eg > 0 && g.eg < (int64_t(1) << 23) && g.n < (int64_t(1) << 23);   // (32-bit byte offsets in that kernel)
    p.edge_wgrad = fits && (sw.edge_wgrad >= 0 ? sw.edge_wgrad != 0 : g.eg >= STREAMED_EDGES_FROM);
    p.recompute = sw.edge_recompute && p.edge_wgrad;
    // The lean chain kernels of batches above PARKED_TILES_MAX read their planes: those keep the stand-alone segment sums
    // and aggregations.
    const bool parked = p.tiles <= PARKED_TILES_MAX;
    const bool room = p.tiles <= RIDER_MAX_SLOTS - 80;
    // The directions differ in what rides.  Forward: the row tiles of the triplet/pair MLPs -- there must be rows, and the
    // fork runs them on its own stream instead.  Backward: the ten tail weight-gradient jobs of the previous chain, which
    // every batch has.
    p.ride = packed && room && (dir == BWD || (g.tp > 0 && !forked));
    p.bf16 = packed && sw.chain_bf16 != 0 && !(dir == BWD && sw.chain_bf16 == 2) && p.tiles <= sw.bf16_tiles;
    // The forward packs the images of both edge steps or of neither.  The backward packs each step's where the kernel that
    // reads them runs: the weight-gradient-forming global kernel keeps its own two-pieces-in-registers loader, and the
    // local layer's paired launch exists only with edges and rows.
    const bool images = packed && sw.edge_images;
    p.gimg = images && !(dir == BWD && p.edge_wgrad);
    p.limg = images && (dir == FWD || (g.tp > 0 && g.el > 0));
    p.agg_in = packed && sw.fuse_local_agg && parked;
    p.gather = packed && sw.fuse_segsum && parked;
    p.pk = packed ? 1 : 0;
    p.pkc = p.bf16 ? 2 : p.pk;
    return p;
}

// ---- arenas -------------------------------------------------------------------------------------------------------------
inline int64_t al(int64_t x) { return (x + 63) / 64 * 64; }       // 256-byte aligned slabs

// what a node chain leaves for the backward.  hdz / gh / hp: backward scratch of the chain's head branch (dz7..dz9, its
// d x_out contribution, head-vector partials), filled for all layers by one launch at the start of the backward
struct ChainSaved { float *x2, *Z, *R, *xout, *hdz, *gh, *hp; };
struct GlobalSaved { float *Zx1, *z, *ea, *Pg; ChainSaved c; };       // (z, ea) or Pg (recompute), the other(s) null
struct LocalSaved { float *Zx1, *zji, *zkj, *q2, *q3, *mnb, *mt, *s, *z1, *z2; ChainSaved c; };
struct Pair { GlobalSaved s; LocalSaved q; };
static_assert(sizeof(Pair) == 28 * sizeof(float*), "Pair is shifted as an array of float*");

// temp arena (forward and backward share it; the backward needs more)
struct Temp {
    float *x1, *P, *msg, *mji;                                         // forward
    float *dZ, *dZ2, *dx2, *dresx, *head, *dz, *dea, *dP, *dZx1, *dxa, *dxb;    // backward (global + shared)
    float *dPg, *dZx1g;          // the global layer's own d P (2 planes) / d Zx1: the local layer's stay alive until the pair's
                                 // merged weight-gradient launch
    float *dzji, *dzkj, *dq2, *dmt, *dq3, *dmnb, *ds, *dz1, *dz2;      // backward (local)
    float *partial, *partial2;   // split-K scratch of two consecutive weight-gradient batches (the reduction of one runs
                                 // inside the launch of the next)
    float* rider_partial;        // split-K scratch of the rider batch (10 node-level jobs in a node-chain launch)
    float* dump;                 // recompute: node output of the recompute launch (discarded); else null
    float* edge_partial;         // partial tiles of the fused global-edge backward's own weight gradients (2 x <= 256 slots)
    int32_t* cuts;               // node-aligned work split of the fused global-edge kernels (<= 257 ints)
};

constexpr int WJOBS = 24;
constexpr int64_t SLOT_FLOATS = D * D + 2 * D;      // one split-K partial tile with its two bias parts

// split-K scratch of the largest weight-gradient batch of a layer pair (<= 256 slots per job; 128 rows: the smallest chunk
// a plan may use, wgrad.hip); a pair's merged batch holds both layers' own jobs
inline int64_t wgrad_floats(const Graph& g) {
    auto slots = [](int64_t rows) { int64_t s = (rows + 127) / 128; return s < 1 ? 1 : (s > 256 ? 256 : s); };
    return (30 * slots(g.n) + 2 * slots(g.eg) + 4 * slots(g.el) + 2 * slots(g.tp)) * SLOT_FLOATS;
}
// the 10 tail jobs of a chain riding in the next chain launch (256-row slots); two chains' riders wait for the pair's
// merged launch
inline int64_t rider_floats(const Graph& g) {
    int64_t s = (g.n + 255) / 256;
    s = s < 1 ? 1 : (s > 256 ? 256 : s);
    return 2 * RIDER_JOBS * s * SLOT_FLOATS;
}

// Both arenas of a call.  ONE walk hands out every slab and counts the floats: what pamnet_stack_workspace /
// pamnet_stack_layout report are this walk's end offsets (null arenas: sizes only).
struct Arena {
    Pair pair0;                   // the slabs of layer pair 0 in `saved`: global layer, then local layer
    Temp t;
    int64_t pair_floats, temp_floats;
    int64_t g_xout, l_xout;       // offsets of the two layers' node outputs within a pair
    Pair at(int64_t k) const {    // the slabs of layer pair k
        Pair p = pair0;
        float** f = reinterpret_cast<float**>(&p);
        for (size_t i = 0; i < sizeof(Pair) / sizeof(float*); ++i)
            if (f[i]) f[i] += k * pair_floats;
        return p;
    }
};

inline Arena make_arena(const Graph& g, const Plan& P, float* saved, float* temp) {
    Arena A{};
    float* base = saved;
    int64_t o = 0;
    auto take = [&](int64_t floats, int64_t count = 1) -> float* {     // `count` planes of `floats` (already padded) each
        const int64_t at = o;
        o += floats * count;
        return base ? base + at : nullptr;
    };
    // NB: the planes of a multi-plane slab are n*D apart (not padded): count * nd >= count * n * D
    const int64_t nd = al(g.n * D), gd = al(g.eg * D), ld = al(g.el * D), td = al(g.tp * D);
    const int64_t hp = al(P.tiles * 257);                              // head-vector partials: 257 floats per row tile
    auto chain = [&](ChainSaved& c, int64_t& xout_at) {
        c.x2 = take(nd), c.Z = take(nd, 10), c.R = take(nd, 2);
        xout_at = o;
        c.xout = take(nd), c.hdz = take(nd, 3), c.gh = take(nd), c.hp = take(hp);
    };
    GlobalSaved& s = A.pair0.s;
    s.Zx1 = take(nd);
    if (P.recompute) s.Pg = take(nd, 2);
    else s.z = take(gd), s.ea = take(gd);
    chain(s.c, A.g_xout);
    LocalSaved& q = A.pair0.q;
    q.Zx1 = take(nd);
    q.zji = take(ld), q.zkj = take(ld), q.q2 = take(ld), q.q3 = take(ld), q.mnb = take(ld), q.mt = take(ld);
    q.s = take(td), q.z1 = take(td), q.z2 = take(td);
    chain(q.c, A.l_xout);
    A.pair_floats = o;

    base = temp, o = 0;
    Temp& t = A.t;
    t.x1 = take(nd), t.P = take(nd, 4), t.msg = take(gd), t.mji = take(ld);
    t.dZ = take(nd, 10);
    t.dZ2 = take(nd, 7);         // second chain-gradient buffer: a fused head+chain launch writes the next chain's dZ
                                 // while the previous chain's is still waiting for its weight-gradient launch
    t.dx2 = take(nd), t.dresx = take(nd), t.head = take(hp), t.dz = take(gd), t.dea = take(gd);
    t.dP = take(nd, 4), t.dZx1 = take(nd), t.dPg = take(nd, 2), t.dZx1g = take(nd), t.dxa = take(nd), t.dxb = take(nd);
    t.dzji = take(ld), t.dzkj = take(ld), t.dq2 = take(ld), t.dmt = take(ld), t.dq3 = take(ld), t.dmnb = take(ld);
    t.ds = take(td), t.dz1 = take(td), t.dz2 = take(td);
    t.partial = take(wgrad_floats(g)), t.partial2 = take(wgrad_floats(g));
    t.rider_partial = take(rider_floats(g));
    int64_t edge_partial = 0;    // (the plain edge backward leaves no partial tiles: nothing to reserve)
    if (P.edge_wgrad) pamnet_global_edge_agg_wg_floats(g.eg, &edge_partial, nullptr);
    t.edge_partial = take(edge_partial);
    if (P.recompute) t.dump = take(nd);
    t.cuts = reinterpret_cast<int32_t*>(take(320));
    A.temp_floats = o;
    return A;
}

// ---- weight images ------------------------------------------------------------------------------------------------------
// fragment-ordered weight images for the node chains (kind 0: fp32 fragments, or bf16x3 images with `pieces`) and for the
// edge-level kernels (kind 1: the bf16x3 fragments a wave would split out of its slice itself, edge_core.h load_wfragb1; in
// their own region `ebase` of the arena) -- all of a direction's images in one launch (pamnet_pack_weights_mixed_f32, <= 224
// matrices per launch)
constexpr int64_t EDGE_IMG = 3 * D * D / 2;
// edge-level images per layer pair: forward W_e, W_ea + the local edge step's four slices; backward W_e, W_ea, mlp_sbf's two and
// the local edge step's four (transposed)
constexpr int64_t EDGE_PACK_PER_PAIR = 8;
constexpr int64_t PACK_PER_PAIR = 28;       // forward: 10 + 5 (global chain + local head) + 10 + 3 (local chain + next global head)
constexpr int64_t PACK_FLOATS_PER_PAIR = PACK_PER_PAIR * (3 * D * D / 2);     // sized for bf16x3 images throughout

// What the launches of a layer pair multiply by: the images when the call packs them, else the parameters themselves, so
// that a launch is spelled once whatever the plan.
struct PairImg {
    const float *gt[10], *lt[10];   // the two chains' matrices
    const float *gh[3], *lh[5];     // the two heads: Wx1, then the projection blocks (2 global: W_i W_j; 4 local: ji_i kj_i ji_j kj_j)
};
struct EdgeMat {
    const float* W;
    int64_t ld;                     // row stride; 0: W is a fragment image
};
struct EdgeImg {
    EdgeMat we, wea;                // global edge step: the e_g slice of mlp_m, W_edge_attr
    EdgeMat w1, w2;                 // backward: mlp_sbf
    const float* wq[4];             // local edge step: the rbf slices of mlp_m_ji / mlp_m_kj, lin_rbf, lin_rbf_out
    int64_t ldq[4];
};
struct PackList {
    static constexpr int CAP = 224;
    const float* src[CAP];
    int64_t ld[CAP], off[CAP];
    int32_t kind[CAP];
    int n = 0;
    bool packed, bf16x3;           // images are made at all; the chain images are bf16x3 ones
    float *base, *ebase;           // the arena; its edge-image region
    int64_t done = 0, edone = 0;   // chain / edge images handed out so far
    int32_t transposed;
    pamnet_stream_t st;
    int rc = 0;
    int64_t img;                   // floats per chain image: fp32 fragment images, or bf16x3 images (3 pieces x 2 bytes: 1.5 x)
    PackList(float* wpack, int64_t n_layer, int32_t t, const Plan& P, pamnet_stream_t s)
        : packed(P.packed), bf16x3(P.bf16), base(wpack), ebase(P.packed ? wpack + n_layer * PACK_FLOATS_PER_PAIR : nullptr),
          transposed(t), st(s), img(P.bf16 ? 3 * D * D / 2 : D * D) {}
    // a chain / head matrix: the image it will occupy (fp32: an fp32 fragment image whatever the list's kind)
    const float* chain(const float* W, int64_t ldw, bool fp32 = false) {
        if (!packed) return W;
        if (n == CAP) flush();
        src[n] = W, ld[n] = ldw, kind[n] = (bf16x3 && !fp32) ? 1 : 0, off[n] = done * img;
        ++n;
        return base + done++ * img;
    }
    EdgeMat edge(bool image, const float* W, int64_t ldw) {
        if (!image) return EdgeMat{W, ldw};
        if (n == CAP) flush();
        src[n] = W, ld[n] = ldw, kind[n] = 1, off[n] = (ebase - base) + edone * EDGE_IMG;
        ++n;
        return EdgeMat{ebase + edone++ * EDGE_IMG, 0};
    }
    void local_edge(bool image, const float* const* lp, EdgeImg& e) {
        const EdgeMat m[4] = {edge(image, lp[L_WJI] + 2 * D, 3 * D), edge(image, lp[L_WKJ] + 2 * D, 3 * D),
                              edge(image, lp[L_WLR], D), edge(image, lp[L_WLO], D)};
        for (int i = 0; i < 4; ++i) e.wq[i] = m[i].W, e.ldq[i] = m[i].ld;
    }
    int flush() {
        if (n && !rc) rc = pamnet_pack_weights_mixed_f32(n, src, ld, kind, off, transposed, base, st);
        n = 0;
        return rc;
    }
};

// ---- head branches ------------------------------------------------------------------------------------------------------
// The head branch (mlp_out + W_out / W) of all 2 n_layer chains runs as one launch per direction, 2L x ceil(n/16)
// workgroups; these are its per-chain tables (row l = 2 k + side: global_0, local_0, global_1, ...).
struct Heads {
    std::vector<const float*> x, w, b, wo, bo, wa;     // x_out; matrices 7..9 and their biases (3 per chain); W_out, its bias, W
    std::vector<float*> Z, hdz, gh, hp, o, a;          // pre-activations (null rows: not saved); backward scratch; out / att rows
    Heads(const Arena& A, const std::vector<PairImg>& img, const float* const* gparams, const float* const* lparams,
          int64_t n_layer, int64_t n, bool keep, float* outs, float* atts) {
        const size_t nh = (size_t)(2 * n_layer);
        for (auto* v : {&x, &wo, &bo, &wa}) v->resize(nh);
        for (auto* v : {&w, &b}) v->resize(3 * nh);
        for (auto* v : {&Z, &hdz, &gh, &hp, &o, &a}) v->resize(nh);
        for (int64_t k = 0; k < n_layer; ++k) {
            const Pair pr = A.at(k);
            for (int side = 0; side < 2; ++side) {
                const int64_t l = 2 * k + side;
                const float* const* tb = side ? lparams + k * L_COUNT + L_TAIL : gparams + k * G_COUNT + G_TAIL;
                const float* const* W = side ? img[k].lt : img[k].gt;
                const ChainSaved& c = side ? pr.q.c : pr.s.c;
                for (int i = 0; i < 3; ++i) w[3 * l + i] = W[7 + i], b[3 * l + i] = tb[T_B + 7 + i];
                x[l] = c.xout, wo[l] = tb[T_WOUT], bo[l] = tb[T_BOUT], wa[l] = tb[T_WATT];
                Z[l] = keep ? c.Z : nullptr, hdz[l] = c.hdz, gh[l] = c.gh, hp[l] = c.hp;
                o[l] = outs + l * n, a[l] = atts + l * n;
            }
        }
    }
};

// ---- forward chain launch -----------------------------------------------------------------------------------------------
// the head of the layer after a chain, run by the chain's launch on the x_out tile still on chip
struct NextHead {
    const float* const* img;     // Wx1, then its nblk projection blocks
    const float* bx1;
    int64_t nblk;
    float *Zx1, *P;              // its saves: pre-activation (backward only), node planes
};
// row tiles [tile0, tile0 + ntiles) of a local layer's triplet/pair MLP riding in a chain launch
struct MlpTiles {
    const float* mlp[4];         // W1 b1 W2 b2
    float* out[3];               // z1 z2 (backward only) s
    int64_t tile0, ntiles;
};
struct Forward {
    const Graph& g;
    const Plan& P;
    const Temp& t;
    bool keep;                   // a training forward: the backward-only saves are written
    const float* e_sbf;
    pamnet_stream_t st;
    float* sv(float* p) const { return keep ? p : nullptr; }
    // One node chain: c.x2 (+ residual res_x) -> c.xout and the saves, through matrices W and the biases / head vectors
    // of the tail block tb; deferred heads.  `next`: the following layer's head in the same launch.  `ride`: MLP row
    // tiles on the idle CUs.  `agg`: x2 itself is formed by the launch's row tiles (the local layer's aggregations).
    // Each nullable.
    int chain(const ChainSaved& c, const float* res_x, const float* const* W, const float* const* tb, const NextHead* next,
              const MlpTiles* ride, const pamnet_local_agg* agg) const {
        node_chain::ChainFwd a{};
        a.x2 = c.x2, a.res_x = res_x, a.n = g.n;
        a.W = W, a.b = tb + T_B, a.w_out = tb[T_WOUT], a.b_out = tb[T_BOUT], a.w_att = tb[T_WATT];
        a.Z = sv(c.Z), a.R = sv(c.R), a.x_out = c.xout;      // (out = att = null: deferred heads)
        if (next) {
            a.next.Wx1 = next->img[0], a.next.bx1 = next->bx1, a.next.wp = next->img + 1, a.next.ldwp = 3 * D;
            a.next.nblk = next->nblk, a.next.Zx1 = sv(next->Zx1), a.next.x1 = t.x1, a.next.P = next->P;
        }
        if (ride) {
            a.rider.x = e_sbf, a.rider.rows = g.tp, a.rider.tile0 = ride->tile0, a.rider.ntiles = ride->ntiles;
            a.rider.mlp = ride->mlp, a.rider.out = ride->out, a.rider.wgs = P.idle;
        }
        a.agg = agg, a.packed = P.pkc, a.stream = st;
        return node_chain::node_chain_fwd(a);
    }
};

// ---- weight gradients ---------------------------------------------------------------------------------------------------
struct Jobs {
    const float* dZ[WJOBS];
    const float* A[WJOBS];
    float* dW[WJOBS];
    float* db[WJOBS];
    int64_t ld_dz[WJOBS], ld_a[WJOBS], ld_dw[WJOBS], rows[WJOBS];
    int32_t mode[WJOBS];
    int n = 0;
    void add(const float* dz, const float* a, int mode_, int64_t rows_, float* dw, int64_t ld_dw_, float* db_) {
        dZ[n] = dz; A[n] = a; dW[n] = dw; db[n] = db_;
        ld_dz[n] = D; ld_a[n] = D; ld_dw[n] = ld_dw_; rows[n] = rows_; mode[n] = mode_;
        ++n;
    }
};

// jobs [k0, k1) of a chain's ten; gt: the tail block of the layer's gradient table
inline void tail_jobs(Jobs& j, const Graph& g, const float* dZ, const ChainSaved& c, float* const* gt, int k0 = 0, int k1 = 10) {
    const int64_t pl = g.n * D;
    const float* src[10] = {c.x2, c.Z, c.Z + pl, c.R, c.Z + 3 * pl, c.R + pl, c.Z + 5 * pl, c.xout, c.Z + 7 * pl, c.Z + 8 * pl};
    const int mode[10] = {0, 1, 1, 0, 1, 0, 1, 0, 1, 1};
    for (int k = k0; k < k1; ++k)         // dz7..dz9 come from the batched head-branch backward
        j.add(k < 7 ? dZ + k * pl : c.hdz + (k - 7) * pl, src[k], mode[k], g.n, gt[T_W + k], D, gt[T_B + k]);
}

// the head-vector gradients of a node chain, summed from the partials its backward left (null: none)
struct HeadGrads {
    const float* partial;
    float *d_wout, *d_watt, *d_bout;
};
inline HeadGrads head_grads(const ChainSaved& c, float* const* gt) { return HeadGrads{c.hp, gt[T_WOUT], gt[T_WATT], gt[T_BOUT]}; }

// the previous chain's tail jobs riding in a fused backward launch: with packed weights they do not go into their layer's
// weight-gradient launch (which keeps the jobs whose operands that next launch overwrites -- dZx1, dP -- and the edge-level
// ones)
struct Riding {
    const float* dZ;             // that chain's gradients
    const ChainSaved* c;
    float* const* gt;            // tail block of its layer's gradient table
    float* partial;              // its split-K slots
    int64_t* slots;              // nullable: out, slots taken
};
struct HeadBwd {
    float* dP;                   // [nblk] planes: gradients of the head's projections
    const float* const* img;     // Wx1, then the projection blocks (transposed images)
    int64_t nblk;
    const float* Zx1;
    float* dZx1;
};
struct Backward {
    const Graph& g;
    const Plan& P;
    const Temp& t;
    void *wctx, *rider;
    pamnet_stream_t st;
    // all weight gradients of a layer + the head-vector gradients of up to two chains
    int run(Jobs& j, float* partial, const HeadGrads& h, const HeadGrads& h2) const {
        return pamnet_wgrad_deferred_f32(j.n, j.dZ, j.ld_dz, j.A, j.ld_a, j.mode, j.rows, j.dW, j.ld_dw, j.db, partial, h.partial,
                                         P.tiles, h.d_wout, h.d_watt, h.d_bout, h2.partial, h2.d_wout, h2.d_watt, h2.d_bout,
                                         wctx, st);
    }
    // Backward of a layer's head fused into the backward of the chain that produced the layer's input (same row tiles, the
    // head's d x stays on chip): h -> t.dx2 / t.dresx -> chain c through W -> dz (and t.dx2 / t.dresx for the next stage).
    // `src` (nullable): segment sums formed by the launch, block b of dP = sum of src[b]'s rows over the CSR (ptr[b], perm[b]),
    // null src[b]: as given.  `ride`: nullable.
    int fused(const HeadBwd& h, const ChainSaved& c, const float* const* W, float* dz, const float* const* src,
              const int32_t* const* ptr, const int32_t* const* perm, const Riding* ride) const {
        if (ride) {
            Jobs jr;
            tail_jobs(jr, g, ride->dZ, *ride->c, ride->gt, 0, RIDER_JOBS);
            CK(pamnet_wgrad_rider_plan_f32(jr.n, jr.dZ, jr.ld_dz, jr.A, jr.ld_a, jr.mode, jr.rows, jr.dW, jr.ld_dw, jr.db,
                                           ride->partial, P.idle, rider, ride->slots));
        }
        node_chain::HeadBwd hb{};
        hb.dP = h.dP, hb.gather_src = src, hb.gather_ptr = src ? ptr : nullptr, hb.gather_perm = src ? perm : nullptr;
        hb.dx1_direct = t.dx2, hb.d_add = t.dresx, hb.Wx1 = h.img[0], hb.wp = h.img + 1, hb.nblk = h.nblk;
        hb.Zx1 = h.Zx1, hb.dZx1 = h.dZx1;
        node_chain::ChainBwd a{};
        a.g_head = c.gh, a.n = g.n, a.W = W, a.Z = c.Z, a.dZ = dz, a.d_x2 = t.dx2, a.d_resx = t.dresx;
        a.packed = P.pkc, a.head = &hb, a.rider = ride ? rider : nullptr, a.stream = st;
        CK(node_chain::node_chain_bwd(a));
        if (ride) CK(pamnet_wgrad_rider_enqueue_f32(wctx, rider));
        return PAMNET_OK;
    }
    // the head's backward alone -> dx (no packed weights, or no chain ahead of the first layer)
    int head(const HeadBwd& h, float* dx) const {
        return pamnet_node_pre_bwd_f32(h.dP, t.dx2, t.dresx, g.n, h.img[0], h.img + 1, 3 * D, h.nblk, h.Zx1, h.dZx1, dx, P.pk, st);
    }
};

// graph_desc: 4 x int64 sizes {n, eg, el, tp}; graph_idx: 18 device pointers in the order of struct Graph (the last three nullable).
int fill_graph(Graph& g, const int64_t* sizes, const int32_t* const* idx) {
    if (!sizes || !idx) return PAMNET_ENULL;
    g.n = sizes[0]; g.eg = sizes[1]; g.el = sizes[2]; g.tp = sizes[3];
    const int32_t** f = &g.g_ptr;
    for (int k = 0; k < 18; ++k) f[k] = idx[k];
    if (!switches().tt_aux || !g.tT_edge || !g.tT_node) g.tT_edge = g.tT_node = nullptr;
    return PAMNET_OK;
}

// work split of the fused global-edge kernels: made with the graph (a side-stream launch of graph construction) or here
int edge_cuts(const Graph& g, const Temp& t, pamnet_stream_t st, const int32_t** cuts) {
    *cuts = g.cuts;
    if (!*cuts) {
        CK(pamnet_seg_cuts_i32(g.g_ptr, g.g_row, g.n, g.eg, t.cuts, nullptr, st));
        *cuts = t.cuts;
    }
    return PAMNET_OK;
}

// the layout for sizes alone (null arenas): what the size queries report
inline Arena sizes_only(int64_t n, int64_t eg, int64_t el, int64_t tp) {
    Graph g{};
    g.n = n; g.eg = eg; g.el = el; g.tp = tp;
    return make_arena(g, make_plan(g, false, false, FWD), nullptr, nullptr);
}

}  // namespace

// The entry points serve every model width: d = 128 runs the loops below, d = 16 / 32 / 64 the narrow engine's
// (narrow_engine.hip), which checks d itself.

// floats of the optional weight-image arena (`wpack`) of pamnet_stack_fwd_f32 / pamnet_stack_bwd_f32
extern "C" int pamnet_stack_pack_floats(int64_t n_layer, int64_t d, int64_t* floats) {
    if (d != D) return narrow_stack::pack_floats(n_layer, d, floats);
    if (n_layer < 1 || !floats) return PAMNET_EINVAL;
    *floats = n_layer * (PACK_FLOATS_PER_PAIR + EDGE_PACK_PER_PAIR * EDGE_IMG);
    return PAMNET_OK;
}

extern "C" int pamnet_stack_workspace(int64_t n, int64_t eg, int64_t el, int64_t tp, int64_t n_layer, int64_t d,
                                      int64_t* saved_floats, int64_t* temp_floats_out) {
    if (d != D) return narrow_stack::workspace(n, eg, el, tp, n_layer, d, saved_floats, temp_floats_out);
    if (n < 0 || eg < 0 || el < 0 || tp < 0 || n_layer < 1 || !saved_floats || !temp_floats_out) return PAMNET_EINVAL;
    const Arena A = sizes_only(n, eg, el, tp);
    *saved_floats = n_layer * A.pair_floats;
    *temp_floats_out = A.temp_floats;
    return PAMNET_OK;
}

// layout[0] = floats per layer pair in `saved`; layout[1] / layout[2] = offset of the global / local layer's output
// node features x_out inside a pair's slab (for inspection: x after every layer).
extern "C" int pamnet_stack_layout(int64_t n, int64_t eg, int64_t el, int64_t tp, int64_t d, int64_t* layout) {
    if (d != D) return narrow_stack::layout(n, eg, el, tp, d, layout);
    if (n < 0 || eg < 0 || el < 0 || tp < 0 || !layout) return PAMNET_EINVAL;
    const Arena A = sizes_only(n, eg, el, tp);
    layout[0] = A.pair_floats, layout[1] = A.g_xout, layout[2] = A.l_xout;
    return PAMNET_OK;
}

extern "C" int pamnet_stack_fwd_f32(const int64_t* sizes, const int32_t* const* graph_idx, int64_t n_layer, int64_t d,
                                    const float* x0, const float* e_g, const float* rbf_e, const float* e_sbf,
                                    const float* const* gparams, const float* const* lparams, float* saved, float* temp,
                                    float* outs, float* atts, int32_t save_for_backward, float* wpack,
                                    pamnet_stream_t aux, void* const* aux_events, pamnet_stream_t st) {
    if (d != D)
        return narrow_stack::fwd(sizes, graph_idx, n_layer, d, x0, e_g, rbf_e, e_sbf, gparams, lparams, saved, temp, outs,
                                 atts, st);
    Graph g;
    CK(fill_graph(g, sizes, graph_idx));
    if (n_layer < 1) return PAMNET_EINVAL;
    if (!x0 || !e_g || !rbf_e || !e_sbf || !gparams || !lparams || !saved || !temp || !outs || !atts) return PAMNET_ENULL;
    // The triplet/pair MLP s_k = mlp_sbf_k(e_sbf) does not depend on the node features: with an auxiliary stream (the
    // fork) all n_layer of them are enqueued up front and run beside the node-level kernels of the first layers, which
    // occupy only ceil(n/16) of the 256 CUs.  Event 0 = inputs ready, event 1+k = s_k ready.
    const Plan P = make_plan(g, wpack != nullptr, aux && aux_events && g.tp > 0, FWD);
    const Arena A = make_arena(g, P, saved, temp);
    const Temp& t = A.t;
    // Inference mode (save_for_backward = 0): tensors only the backward reads (pre-activations, gates, residual taps)
    // are not written at all -- about half of the forward's HBM writes.  `sv(p)` = p or null.
    const Forward F{g, P, t, save_for_backward != 0, e_sbf, st};
    auto sv = [&F](float* p) { return F.sv(p); };
    auto mlp_of = [&](int64_t k, int64_t tile0, int64_t ntiles) {      // row tiles of layer k's triplet/pair MLP, with its operands
        const float* const* lp = lparams + k * L_COUNT;
        const LocalSaved q = A.at(k).q;
        return MlpTiles{{lp[L_WS1], lp[L_BS1], lp[L_WS2], lp[L_BS2]}, {sv(q.z1), sv(q.z2), q.s}, tile0, ntiles};
    };
    auto mlp_rows = [&](const MlpTiles& m, int64_t rows, pamnet_stream_t on) {      // its first `rows` rows as a launch of their own
        return pamnet_mlp2_fwd_f32(e_sbf, rows, m.mlp[0], m.mlp[1], m.mlp[2], m.mlp[3], m.out[0], m.out[1], m.out[2], on);
    };
    // Riders: the triplet/pair MLP of layer k >= 1 rides in the two node-chain launches that precede its use -- first half
    // of its row tiles in the local chain of pair k-1, second half in the global chain of pair k; only layer 0's first
    // half runs as a launch of its own ahead of the loop.  With the bf16x6 chains' 8-wave riders the first chain launch
    // carries all of layer 0's tiles: +6.6 us there against the 14 us of that launch (profiles/r06_chain_bf16.txt).
    const int64_t mlp_tiles = ceil_div(g.tp, 16), mlp_half = mlp_tiles / 2;
    const bool all_ride = P.ride && P.bf16;
    if (P.ride) {
        if (mlp_half > 0 && !all_ride) CK(mlp_rows(mlp_of(0, 0, 0), mlp_half * 16, st));
    } else if (P.forked) {
        hipStream_t a = as_stream(aux);
        HK(hipEventRecord(reinterpret_cast<hipEvent_t>(aux_events[0]), as_stream(st)));
        HK(hipStreamWaitEvent(a, reinterpret_cast<hipEvent_t>(aux_events[0]), 0));
        for (int64_t k = 0; k < n_layer; ++k) {
            CK(mlp_rows(mlp_of(k, 0, 0), g.tp, aux));
            HK(hipEventRecord(reinterpret_cast<hipEvent_t>(aux_events[1 + k]), a));
        }
    } else if (g.tp > 0) {
        // neither: the MLPs of up to 8 layers at a time as one launch ahead of the layer loop
        for (int64_t k0 = 0; k0 < n_layer; k0 += 8) {
            const int64_t nk = n_layer - k0 < 8 ? n_layer - k0 : 8;
            const float* prm[32];
            float* out[24];
            for (int64_t k = 0; k < nk; ++k) {
                const MlpTiles m = mlp_of(k0 + k, 0, 0);
                for (int i = 0; i < 4; ++i) prm[4 * k + i] = m.mlp[i];
                for (int i = 0; i < 3; ++i) out[3 * k + i] = m.out[i];
            }
            CK(pamnet_mlp2_fwd_multi_f32(e_sbf, g.tp, nk, prm, out, st));
        }
    }
    // Weight images (optional `wpack` arena): one pack launch for all layers.  bf16x3 images for everything the chains
    // multiply by (matrices 0..6 + the fused heads of the next layers), fp32 images for the mlp_out matrices 7..9
    // (node_heads_fwd_kernel); the edge-level images in the region behind them.
    std::vector<PairImg> img((size_t)n_layer);
    std::vector<EdgeImg> eimg((size_t)n_layer);
    {
        PackList im(wpack, n_layer, 0, P, st);
        for (int64_t k = 0; k < n_layer; ++k) {
            const float* const* gp = gparams + k * G_COUNT;
            const float* const* lp = lparams + k * L_COUNT;
            for (int i = 0; i < 10; ++i) img[k].gt[i] = im.chain(gp[G_TAIL + i], D, i >= 7);
            img[k].lh[0] = im.chain(lp[L_WX1], D);
            img[k].lh[1] = im.chain(lp[L_WJI], 3 * D), img[k].lh[2] = im.chain(lp[L_WKJ], 3 * D);
            img[k].lh[3] = im.chain(lp[L_WJI] + D, 3 * D), img[k].lh[4] = im.chain(lp[L_WKJ] + D, 3 * D);
            for (int i = 0; i < 10; ++i) img[k].lt[i] = im.chain(lp[L_TAIL + i], D, i >= 7);
            if (k + 1 < n_layer) {          // (the first layer's head runs alone, on the parameters themselves)
                const float* const* gn = gparams + (k + 1) * G_COUNT;
                img[k + 1].gh[0] = im.chain(gn[G_WX1], D);
                img[k + 1].gh[1] = im.chain(gn[G_WM], 3 * D), img[k + 1].gh[2] = im.chain(gn[G_WM] + D, 3 * D);
            }
            eimg[k].we = im.edge(P.gimg, gp[G_WM] + 2 * D, 3 * D), eimg[k].wea = im.edge(P.gimg, gp[G_WEA], D);
            im.local_edge(P.limg, lp, eimg[k]);
        }
        CK(im.flush());
    }
    const int32_t* cuts = nullptr;
    CK(edge_cuts(g, t, st, &cuts));
    const float* x = x0;
    Pair next = A.at(0);
    for (int64_t k = 0; k < n_layer; ++k) {
        const bool more = k + 1 < n_layer;
        const Pair pr = next;
        if (more) next = A.at(k + 1);
        const GlobalSaved& s = pr.s;
        const LocalSaved& q = pr.q;
        const float* const* gp = gparams + k * G_COUNT;
        const float* const* lp = lparams + k * L_COUNT;
        // ---------------- global layer (layers/global_message_passing.py:33-56)
        // the head of every layer but the first runs inside the preceding layer's node chain (x_out tile still on chip)
        // (recompute: the node planes of a training forward go to the saved arena instead of the scratch)
        float* const Pk = (F.keep && s.Pg) ? s.Pg : t.P;
        if (k == 0) {
            const float* wpg[2] = {gp[G_WM], gp[G_WM] + D};
            CK(pamnet_node_pre_fwd_f32(x, g.n, gp[G_WX1], gp[G_BX1], wpg, 3 * D, 2, sv(s.Zx1), t.x1, Pk, st));
        }
        // message MLP + add-aggregation in one kernel: x2 = x1 + sum_{e -> i} msg_e, the messages never leave the chip
        CK(pamnet_global_edge_agg_fwd_f32(e_g, g.eg, g.n, eimg[k].we.W, eimg[k].we.ld, gp[G_BM], eimg[k].wea.W, eimg[k].wea.ld,
                                          Pk, Pk + g.n * D, g.g_ptr, g.g_row, g.g_col, cuts, t.x1, sv(s.z), sv(s.ea), s.c.x2, st));
        // its chain, the local layer's head, and the rest of this layer's MLP row tiles
        {
            const NextHead lh{img[k].lh, lp[L_BX1], 4, q.Zx1, t.P};
            const int64_t tile0 = (k == 0 && all_ride) ? 0 : mlp_half;
            const MlpTiles rd = mlp_of(k, tile0, mlp_tiles - tile0);
            CK(F.chain(s.c, x, img[k].gt, gp + G_TAIL, &lh, P.ride ? &rd : nullptr, nullptr));
        }
        x = s.c.xout;
        // ---------------- local layer (layers/local_message_passing.py:36-66); its head ran in the chain above
        const float* planes[4] = {t.P, t.P + g.n * D, t.P + 2 * g.n * D, t.P + 3 * g.n * D};
        CK(pamnet_local_edge_fwd_f32(rbf_e, g.el, eimg[k].wq, eimg[k].ldq, lp[L_BJI], lp[L_BKJ], planes, g.l_row, g.l_col,
                                     sv(q.zji), sv(q.zkj), sv(q.q2), q.q3, t.mji, q.mnb, st));
        if (P.forked) HK(hipStreamWaitEvent(as_stream(st), reinterpret_cast<hipEvent_t>(aux_events[1 + k]), 0));
        // both aggregations of the local layer (rows -> edges -> nodes) in one launch, or formed by the chain launch's own
        // tiles; m_t is a backward-only save
        const pamnet_local_agg la{t.mji, q.mnb, q.s, q.q3, t.x1, g.t_ptr, g.t_col, g.l_ptr, sv(q.mt)};
        if (!P.agg_in)
            CK(pamnet_local_agg_fwd_f32(t.mji, q.mnb, q.s, q.q3, g.t_ptr, g.t_col, g.l_ptr, t.x1, g.n, sv(q.mt), q.c.x2, st));
        // its chain and, while layers follow, the next global layer's head and the first half of the next MLP's row tiles
        if (more) {
            const NextHead gh{img[k + 1].gh, gparams[(k + 1) * G_COUNT + G_BX1], 2, next.s.Zx1,
                              (F.keep && next.s.Pg) ? next.s.Pg : t.P};
            const MlpTiles rd = mlp_of(k + 1, 0, mlp_half);
            CK(F.chain(q.c, x, img[k].lt, lp + L_TAIL, &gh, P.ride ? &rd : nullptr, P.agg_in ? &la : nullptr));
        } else {
            CK(F.chain(q.c, x, img[k].lt, lp + L_TAIL, nullptr, nullptr, P.agg_in ? &la : nullptr));
        }
        x = q.c.xout;
    }
    const Heads H(A, img, gparams, lparams, n_layer, g.n, F.keep, outs, atts);
    return pamnet_node_heads_fwd_f32(2 * n_layer, H.x.data(), H.w.data(), H.b.data(), H.wo.data(), H.bo.data(), H.wa.data(),
                                     H.Z.data(), H.o.data(), H.a.data(), g.n, P.pk, st);
}

// d_outs / d_atts: [2L][n].  ggrads / lgrads: gradient buffers in the same tables as the parameters (written, not
// accumulated).  d_x0 [n,128] written; d_eg, d_rbf, d_sbf written (first layer processed) then accumulated.
extern "C" int pamnet_stack_bwd_f32(const int64_t* sizes, const int32_t* const* graph_idx, int64_t n_layer, int64_t d,
                                    const float* x0, const float* e_g, const float* rbf_e, const float* e_sbf,
                                    const float* const* gparams, const float* const* lparams, const float* saved,
                                    float* temp, const float* d_outs, const float* d_atts, float* const* ggrads,
                                    float* const* lgrads, float* d_x0, float* d_eg, float* d_rbf, float* d_sbf,
                                    float* wpack, void* const* layer_done, pamnet_stream_t st) {
    if (d != D)
        return narrow_stack::bwd(sizes, graph_idx, n_layer, d, x0, e_g, rbf_e, e_sbf, gparams, lparams, saved, temp, d_outs,
                                 d_atts, ggrads, lgrads, d_x0, d_eg, d_rbf, d_sbf, layer_done, st);
    Graph g;
    CK(fill_graph(g, sizes, graph_idx));
    if (n_layer < 1) return PAMNET_EINVAL;
    if (!x0 || !e_g || !rbf_e || !e_sbf || !gparams || !lparams || !saved || !temp || !d_outs || !d_atts || !ggrads ||
        !lgrads || !d_x0 || !d_eg || !d_rbf || !d_sbf)
        return PAMNET_ENULL;
    const Plan P = make_plan(g, wpack != nullptr, false, BWD);
    const Arena A = make_arena(g, P, const_cast<float*>(saved), temp);      // (the backward writes only its scratch slabs: hdz, gh, hp)
    const Temp& t = A.t;
    // Transposed weight images (optional `wpack` arena), one pack launch: bf16x3 images for everything a bf16 plan's chain
    // launches multiply by; fp32 images for the heads' matrices 7..9 and for the first layer's stand-alone head backward.
    std::vector<PairImg> img((size_t)n_layer);
    std::vector<EdgeImg> eimg((size_t)n_layer);
    {
        PackList im(wpack, n_layer, 1, P, st);
        for (int64_t k = n_layer - 1; k >= 0; --k) {
            const float* const* lp = lparams + k * L_COUNT;
            const float* const* gp = gparams + k * G_COUNT;
            for (int i = 0; i < 10; ++i) img[k].lt[i] = im.chain(lp[L_TAIL + i], D, i >= 7);
            img[k].lh[1] = im.chain(lp[L_WJI], 3 * D), img[k].lh[2] = im.chain(lp[L_WKJ], 3 * D);
            img[k].lh[3] = im.chain(lp[L_WJI] + D, 3 * D), img[k].lh[4] = im.chain(lp[L_WKJ] + D, 3 * D);
            img[k].lh[0] = im.chain(lp[L_WX1], D);
            for (int i = 0; i < 10; ++i) img[k].gt[i] = im.chain(gp[G_TAIL + i], D, i >= 7);
            img[k].gh[1] = im.chain(gp[G_WM], 3 * D, k == 0), img[k].gh[2] = im.chain(gp[G_WM] + D, 3 * D, k == 0);
            img[k].gh[0] = im.chain(gp[G_WX1], D, k == 0);
            eimg[k].we = im.edge(P.gimg, gp[G_WM] + 2 * D, 3 * D), eimg[k].wea = im.edge(P.gimg, gp[G_WEA], D);
            eimg[k].w1 = im.edge(P.limg, lp[L_WS1], D), eimg[k].w2 = im.edge(P.limg, lp[L_WS2], D);
            im.local_edge(P.limg, lp, eimg[k]);
        }
        CK(im.flush());
    }
    // head branch of all 2 n_layer chains first, in one launch: it needs only d out / d att
    {
        const Heads H(A, img, gparams, lparams, n_layer, g.n, true, const_cast<float*>(d_outs), const_cast<float*>(d_atts));
        CK(pamnet_node_heads_bwd_f32(2 * n_layer, H.o.data(), H.a.data(), H.w.data(), H.wo.data(), H.wa.data(), H.Z.data(),
                                     H.hdz.data(), H.gh.data(), H.hp.data(), g.n, P.pk, st));
    }
    // Chain backward launches.  With packed weights the backward of a layer's head (node_pre_bwd) is fused into the
    // backward of the chain that produced that layer's input: per layer pair
    //   [chain L_k] local edges [head L_k + chain G_k] wgrad L_k  global edges [head G_k + chain L_{k-1}] wgrad G_k.
    // The chain gradients alternate between two buffers because a fused launch writes the next chain's dZ before the
    // previous chain's weight-gradient launch (which also needs that launch's dZx1) has consumed its own.
    // weight-gradient batches: the fixed-order reduction of each batch rides in the next batch's launch
    int64_t ctx_bytes = 0, rider_bytes = 0;
    CK(pamnet_wgrad_ctx_bytes(&ctx_bytes));
    CK(pamnet_wgrad_rider_bytes(&rider_bytes));
    std::vector<char> wctx((size_t)ctx_bytes, 0), rider((size_t)rider_bytes, 0);
    const Backward B{g, P, t, wctx.data(), rider.data(), st};
    const int32_t* cuts = nullptr;
    CK(edge_cuts(g, t, st, &cuts));
    const HeadGrads none{nullptr, nullptr, nullptr, nullptr};
    auto done = [&](int64_t k) {          // every gradient of layer pair k has been enqueued
        return (k < n_layer && layer_done && layer_done[k])
                   ? (int)hipEventRecord(reinterpret_cast<hipEvent_t>(layer_done[k]), as_stream(st)) : PAMNET_OK;
    };
    const int64_t pl = g.n * D;
    float* parts[2] = {t.partial, t.partial2};
    int pflip = 0;
    Jobs pair_jobs;                       // a pair's local-layer jobs waiting for its merged launch
    HeadGrads pair_head = none;
    int64_t rider_a_slots = 0;            // slots of the local chain's riders (the global chain's start behind them)
    const float* d_xout = nullptr;        // nothing consumes the last layer's node features (models.py:196-224)
    float* dx_bufs[2] = {t.dxa, t.dxb};
    float* dz_bufs[2] = {t.dZ, t.dZ2};
    int flip = 0, zflip = 0;
    float* dz_local = dz_bufs[zflip];     // dZ of the local chain of the current pair
    Pair prev = A.at(n_layer - 1);
    if (P.packed)
        CK(pamnet_node_tail_main_bwd_f32(nullptr, prev.q.c.gh, g.n, img[n_layer - 1].lt, prev.q.c.Z, dz_local, t.dx2, t.dresx,
                                         P.pkc, st));
    for (int64_t k = n_layer - 1; k >= 0; --k) {
        const Pair pr = prev;
        if (k > 0) prev = A.at(k - 1);
        const GlobalSaved& s = pr.s;
        const LocalSaved& q = pr.q;
        const int acc = (k != n_layer - 1) ? 1 : 0;
        // With riders a layer pair's own jobs -- 11 of the local layer, 5 of the global one -- are ONE launch behind the
        // pair's second chain launch (k >= 1; the last pair's global layer keeps its ten tail jobs: two launches there):
        // a weight-gradient launch at this batch size is ~14 us of work in ~30 us (prologue, partial stores, the riding
        // reductions), and the local layer's operands (t.dP, t.dZx1, the edge / row gradients) stay untouched until the
        // next pair's local phase -- the global phase writes its own d P / d Zx1 (t.dPg, t.dZx1g).
        const bool merged = P.ride && k > 0;
        float* dz_global = nullptr;
        // ================= local layer backward
        {
            const float* const* lp = lparams + k * L_COUNT;
            float* const* lg = lgrads + k * L_COUNT;
            const float* x_in = s.c.xout;         // input of the local layer = output of this pair's global layer
            if (!P.packed) {
                dz_local = t.dZ;
                CK(pamnet_node_tail_main_bwd_f32(d_xout, q.c.gh, g.n, img[k].lt, q.c.Z, dz_local, t.dx2, t.dresx, P.pk, st));
            }
            // d m_t = d x2[i] * q3,  d q3 = d x2[i] * m_t,  d s = m_nb[idx] * d m_t[e],  d m_nb = transposed sum: one launch
            CK(pamnet_local_agg_bwd_f32(t.dx2, g.l_row, q.q3, q.mt, q.mnb, q.s, g.t_ptr, g.t_col, g.t_row, g.tT_ptr,
                                        g.tT_perm, g.tT_edge, g.tT_node, g.el, t.dmt, t.dq3, t.ds, t.dmnb, st));
            // the triplet / pair MLP's backward and the local edge stage's: independent of each other, one launch
            CK(pamnet_local_bwd_pair_f32(t.ds, g.tp, q.z1, q.z2, eimg[k].w1.W, eimg[k].w2.W, t.dz1, t.dz2, d_sbf,
                                         acc | (P.limg ? PAMNET_WEIGHT_IMAGES : 0), t.dmt, t.dmnb, t.dq3, g.el, q.zji, q.zkj,
                                         q.q2, eimg[k].wq, eimg[k].ldq, t.dzji, t.dzkj, t.dq2, d_rbf, acc, st));
            // d P of the local head: four segment sums, by a launch of their own or inside the fused launch below
            const float* sa[4] = {t.dzji, t.dzkj, t.dzji, t.dzkj};
            const int32_t* sp[4] = {nullptr, nullptr, g.lT_perm, g.lT_perm};
            const int32_t* sr[4] = {g.l_ptr, g.l_ptr, g.lT_ptr, g.lT_ptr};
            if (!P.gather) {
                float* so[4] = {t.dP, t.dP + pl, t.dP + 2 * pl, t.dP + 3 * pl};
                CK(pamnet_segment_sum_multi_f32(4, so, sa, sp, sr, g.n, D, st));
            }
            const HeadBwd head{t.dP, img[k].lh, 4, q.Zx1, t.dZx1};
            if (P.packed) {
                // head of the local layer + the global chain of this pair; this layer's chain gradients ride
                zflip ^= 1;
                dz_global = dz_bufs[zflip];
                const Riding rd{dz_local, &q.c, lg + L_TAIL, t.rider_partial, &rider_a_slots};
                CK(B.fused(head, s.c, img[k].gt, dz_global, P.gather ? sa : nullptr, sr, sp, P.ride ? &rd : nullptr));
            } else {
                float* dx = dx_bufs[flip];
                CK(B.head(head, dx));
                d_xout = dx;
                flip ^= 1;
            }
            Jobs j;
            tail_jobs(j, g, dz_local, q.c, lg + L_TAIL, P.ride ? RIDER_JOBS : 0, 10);
            j.add(t.dZx1, x_in, 0, g.n, lg[L_WX1], D, lg[L_BX1]);
            j.add(t.dP, q.Zx1, 1, g.n, lg[L_WJI], 3 * D, nullptr);
            j.add(t.dP + pl, q.Zx1, 1, g.n, lg[L_WKJ], 3 * D, nullptr);
            j.add(t.dP + 2 * pl, q.Zx1, 1, g.n, lg[L_WJI] + D, 3 * D, nullptr);
            j.add(t.dP + 3 * pl, q.Zx1, 1, g.n, lg[L_WKJ] + D, 3 * D, nullptr);
            j.add(t.dzji, rbf_e, 0, g.el, lg[L_WJI] + 2 * D, 3 * D, lg[L_BJI]);
            j.add(t.dzkj, rbf_e, 0, g.el, lg[L_WKJ] + 2 * D, 3 * D, lg[L_BKJ]);
            j.add(t.dq2, rbf_e, 0, g.el, lg[L_WLR], D, nullptr);
            j.add(t.dq3, rbf_e, 0, g.el, lg[L_WLO], D, nullptr);
            j.add(t.dz2, q.z1, 1, g.tp, lg[L_WS2], D, lg[L_BS2]);
            j.add(t.dz1, e_sbf, 0, g.tp, lg[L_WS1], D, lg[L_BS1]);
            const HeadGrads hl = head_grads(q.c, lg + L_TAIL);
            if (!merged) {
                CK(B.run(j, parts[pflip], hl, none));
                pflip ^= 1;
                // that launch also reduced the weight gradients of the previous pair's global layer: pair k+1 is complete
                CK(done(k + 1));
            } else {
                pair_jobs = j;
                pair_head = hl;
            }
        }
        // ================= global layer backward
        {
            const float* const* gp = gparams + k * G_COUNT;
            float* const* gg = ggrads + k * G_COUNT;
            const float* x_in = (k == 0) ? x0 : prev.q.c.xout;
            if (!P.packed) {
                dz_global = t.dZ;
                CK(pamnet_node_tail_main_bwd_f32(d_xout, s.c.gh, g.n, img[k].gt, s.c.Z, dz_global, t.dx2, t.dresx, P.pk, st));
            }
            // d z, d ea, d e and the target-side reduction d P_i in one kernel; the source-side one walks the transposed CSR
            if (P.edge_wgrad) {
                // ... and the step's own weight gradients: partial tiles per workgroup, summed by the next weight-gradient launch
                int64_t efloats = 0, eslots = 0;
                CK(pamnet_global_edge_agg_wg_floats(g.eg, &efloats, &eslots));
                const float *zk = s.z, *eak = s.ea;
                if (s.Pg) {
                    // recompute: z and ea of this layer once more, by the kernel that made them in the forward, into scratch
                    // the fused backward does not use (the forward's message buffer, the d ea rows it no longer writes)
                    CK(pamnet_global_edge_agg_fwd_f32(e_g, g.eg, g.n, gp[G_WM] + 2 * D, 3 * D, gp[G_BM], gp[G_WEA], D, s.Pg,
                                                      s.Pg + g.n * D, g.g_ptr, g.g_row, g.g_col, cuts, nullptr, t.msg, t.dea,
                                                      t.dump, st));
                    zk = t.msg, eak = t.dea;
                }
                CK(pamnet_global_edge_agg_bwd_wg_f32(t.dx2, g.eg, g.n, g.g_ptr, g.g_row, cuts, zk, eak, e_g, gp[G_WM] + 2 * D,
                                                     3 * D, gp[G_WEA], D, t.dz, d_eg, acc, t.dPg, t.edge_partial, st));
                CK(pamnet_wgrad_edge_enqueue_f32(B.wctx, eslots, gg[G_WM] + 2 * D, 3 * D, gg[G_BM], gg[G_WEA], D, t.edge_partial));
            } else {
                CK(pamnet_global_edge_agg_bwd_f32(t.dx2, g.eg, g.n, g.g_ptr, g.g_row, cuts, s.z, s.ea, eimg[k].we.W, eimg[k].we.ld,
                                                  eimg[k].wea.W, eimg[k].wea.ld, t.dz, t.dea, d_eg, acc, t.dPg, st));
            }
            const bool chained = P.packed && k > 0;     // a chain lies ahead: its backward takes this layer's head along
            const bool gather_g = chained && P.gather;   // ... and the source-side sum
            if (!gather_g)
                CK(pamnet_segment_sum_f32(t.dPg + pl, nullptr, t.dz, nullptr, nullptr, nullptr, g.gT_perm, g.gT_ptr, g.n, D, st));
            const HeadBwd head{t.dPg, img[k].gh, 2, s.Zx1, t.dZx1g};
            if (chained) {
                // head of the global layer + the local chain of the previous pair; this layer's chain gradients ride, their
                // slots right behind the local chain's riders: both wait for the pair's merged launch
                zflip ^= 1;
                dz_local = dz_bufs[zflip];
                const float* ga[2] = {nullptr, t.dz};
                const int32_t* gr[2] = {nullptr, g.gT_ptr};
                const int32_t* gq[2] = {nullptr, g.gT_perm};
                const Riding rd{dz_global, &s.c, gg + G_TAIL, t.rider_partial + rider_a_slots * SLOT_FLOATS, nullptr};
                CK(B.fused(head, prev.q.c, img[k - 1].lt, dz_local, gather_g ? ga : nullptr, gr, gq, P.ride ? &rd : nullptr));
            } else {
                float* dx = (k == 0) ? d_x0 : dx_bufs[flip];
                CK(B.head(head, dx));
                d_xout = dx;
                flip ^= 1;
            }
            Jobs j;
            if (merged) j = pair_jobs;                        // the local layer's own jobs, parked above
            tail_jobs(j, g, dz_global, s.c, gg + G_TAIL, merged ? RIDER_JOBS : 0, 10);
            j.add(t.dZx1g, x_in, 0, g.n, gg[G_WX1], D, gg[G_BX1]);
            j.add(t.dPg, s.Zx1, 1, g.n, gg[G_WM], 3 * D, nullptr);
            j.add(t.dPg + pl, s.Zx1, 1, g.n, gg[G_WM] + D, 3 * D, nullptr);
            if (!P.edge_wgrad) {
                j.add(t.dz, e_g, 0, g.eg, gg[G_WM] + 2 * D, 3 * D, gg[G_BM]);
                j.add(t.dea, e_g, 0, g.eg, gg[G_WEA], D, nullptr);
            }
            CK(B.run(j, parts[pflip], head_grads(s.c, gg + G_TAIL), merged ? pair_head : none));
            pflip ^= 1;
            // (merged: that launch also reduced the previous pair's merged batch: pair k+1 is complete)
            if (merged) CK(done(k + 1));
        }
    }
    CK(pamnet_wgrad_flush_f32(B.wctx, st));
    return done(0);
}
