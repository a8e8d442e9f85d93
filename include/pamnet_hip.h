/*
 * pamnet_hip.h -- C ABI of libpamnet_hip.so: PAMNet's multiplex message-passing hot path as gfx950 (MI355X) kernels.
 *
 * The reference (XieResearchGroup/Physics-aware-Multiplex-GNN) has no FFI of its own: its hot path reaches native code
 * through four third-party wheels (torch_scatter, torch_sparse, torch_cluster, torch_geometric) and torch ATen.  Each
 * entry point below replaces one of those native call sites; the reference file:line it stands in for is cited.
 *
 * Conventions (every function):
 *   - arguments are raw DEVICE pointers, 64-bit sizes and a hipStream_t (passed as void*); no torch types;
 *   - the caller owns every device buffer; the library allocates no device memory, keeps no mutable state between calls
 *     and never synchronises (the pamnet_stack_* engine calls build small host-side pointer tables on the stack / heap per
 *     call).  The only process-wide data are fifteen developer switches taken from the environment (kernel-variant selection
 *     for measurements; INTEGRATION.md section 5 lists them).  Fourteen are read once, on first use (C++11 static
 *     initialisation, thread-safe, constant afterwards): the layer-stack engine's nine in one block (csrc/engine.hip
 *     Switches: PAMNET_EDGE_RECOMPUTE, PAMNET_EDGE_WGRAD, PAMNET_EDGE_IMAGES with PAMNET_EDGE_WAVES, PAMNET_FUSE_SEGSUM,
 *     PAMNET_FUSE_LOCAL_AGG, PAMNET_CHAIN_BF16, PAMNET_CHAIN_BF16_TILES, PAMNET_TT_AUX), and PAMNET_EDGE_WAVES
 *     (edge_chain.hip), PAMNET_CHAIN_LEAN, PAMNET_CHAIN_WAVES (node_tail.hip), PAMNET_AGG_PIECES (edge_agg.hip),
 *     PAMNET_SMALL_FORMS, PAMNET_HIST_LDS (graph.hip) where they are used.  PAMNET_AGG_PP (edge_agg.hip) is read by every call;
 *   - work is enqueued on `stream`; return value 0 = OK, >0 = hipError_t of the failed launch, <0 = argument error
 *     (PAMNET_EINVAL: bad size / unsupported width; PAMNET_ENULL: required pointer is null);
 *   - float tensors are fp32 row-major [rows, d]; index tensors are int32; CSR pointers have rows+1 entries;
 *   - re-entrant and thread-safe: nothing mutable is shared between calls.  Segment reductions are sorted-CSR, atomics-free, deterministic.
 */
#ifndef PAMNET_HIP_H
#define PAMNET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PAMNET_OK 0
#define PAMNET_EINVAL (-1)
#define PAMNET_ENULL (-2)
/* flag bit of pamnet_local_bwd_pair_f32's accumulate_dx (bit 0 = accumulate): W1 / W2 are fragment images, see
 * pamnet_pack_weights_mixed_f32 */
#define PAMNET_WEIGHT_IMAGES 2
/* flag bit of `nblk` of pamnet_node_pre_tail_bwd(_gather)_f32: every weight image of the call is a bf16x3 (kind-1, transposed)
 * one, and the launch runs its GEMMs as bf16x6 piece products (single-round batches; pamnet_node_tail_main_bwd_f32 takes
 * packed == 2 for the same) */
#define PAMNET_CHAIN_PIECES 16

typedef void* pamnet_stream_t; /* hipStream_t */

/* Library / ABI version (bumped on any signature change).  pamnet_abi_version() returns the PAMNET_ABI_VERSION the library
 * was built against; a binding compares it with this header's (pamnet_amd/lib.py load(): a stale .so fails loudly). */
#define PAMNET_ABI_VERSION 18
int pamnet_abi_version(void);

/* ------------------------------------------------------------------------------------------------------------------
 * Segment reduction / gather  (torch_scatter.scatter(src, index, dim=0, dim_size, reduce='add'):
 *   layers/local_message_passing.py:50,54,107,111;  PyG MessagePassing aggregate: layers/global_message_passing.py:38;
 *   global_add_pool / global_mean_pool: models.py:216,219,221,351;  row gathers x[i], m[idx]: local...:46,49)
 *
 * out[r, :] = (init ? init[r, :] : 0) + sum_{q = ptr[r] .. ptr[r+1]-1}  A[ia(k), :] * (B ? B[ib(k), :] : 1),
 *             k = perm ? perm[q] : q,   ia(k) = ia ? ia[k] : k,   ib(k) = ib ? ib[k] : k.
 * With ia=ib=perm=B=init=NULL this is exactly scatter(src=A, index=sorted segment ids) -- the scatter-add roofline
 * kernel.  The same entry serves every backward (gather^T) through a transposed CSR (`perm`).
 * d must be a multiple of 4.  `out` may not alias A or B.
 * ------------------------------------------------------------------------------------------------------------------ */
int pamnet_segment_sum_f32(float* out, const float* init, const float* A, const int32_t* ia, const float* B,
                           const int32_t* ib, const int32_t* perm, const int32_t* ptr, int64_t rows, int64_t d,
                           pamnet_stream_t stream);

/* out[k, :] = A[ia ? ia[k] : k, :] * (B ? B[ib ? ib[k] : k, :] : 1)   for k < m.   (x[i], x[j], m_neighbor[idx]) */
int pamnet_gather_mul_f32(float* out, const float* A, const int32_t* ia, const float* B, const int32_t* ib,
                          int64_t m, int64_t d, pamnet_stream_t stream);

/* Batched forms used by the layer backward (d = 128): up to 4 plain segment sums over the same number of rows in one
 * launch (host arrays of device pointers; perm[j] nullable), and one gather feeding two products
 * (out1 = A[ia]*B1, out2 = A[ia]*B2: d m_t and d q3 of layers/local_message_passing.py:53). */
int pamnet_segment_sum_multi_f32(int64_t njobs, float* const* out, const float* const* A, const int32_t* const* perm,
                                 const int32_t* const* ptr, int64_t rows, int64_t d, pamnet_stream_t stream);
int pamnet_gather_mul2_f32(float* out1, float* out2, const float* A, const int32_t* ia, const float* B1,
                           const float* B2, int64_t m, int64_t d, pamnet_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Index plumbing for graph construction (torch_sparse.SparseTensor CSR build: models.py:71-73, 267-269)
 * ------------------------------------------------------------------------------------------------------------------ */
/* out[0]=0, out[i+1]=sum_{j<=i} in[j]  (n inputs -> n+1 outputs).  `tmp` needs ceil(n/4096)+1 ints. */
int pamnet_exclusive_scan_i32(const int32_t* in, int32_t* out, int64_t n, int32_t* tmp, pamnet_stream_t stream);
/* two arrays of the same length, one launch when they are short */
int pamnet_exclusive_scan_pair_i32(const int32_t* in_a, int32_t* out_a, const int32_t* in_b, int32_t* out_b, int64_t n,
                                   int32_t* tmp, pamnet_stream_t stream);

/* flag[0] = 1 when the index inputs of a batch are out of range (the reference would raise an IndexError): node_graph not
 * sorted / not in [0, n_graphs), a type (float, element i at types[i * type_stride]; nullable) not in [0, n_types), an
 * edge endpoint (src / dst, nullable with n_edges = 0) not in [0, n).  One launch; flag is zeroed by the call. */
int pamnet_validate_inputs_i32(const int32_t* node_graph, int64_t n, int64_t n_graphs, const float* types,
                               int64_t type_stride, int64_t n_types, const int32_t* src, const int32_t* dst,
                               int64_t n_edges, int32_t* flag, pamnet_stream_t stream);
/* Stable counting sort of m keys in [0, rows): ptr[rows+1] (CSR) and perm[m] with keys[perm[q]] non-decreasing and
 * perm ascending inside a row.  Scratch: `cursor` rows + 1 ints (the rows' counters plus one flag: an already
 * non-decreasing key sequence takes the identity-permutation path), `perm_tmp` m ints, `tmp` ceil(rows/4096)+1 ints (the
 * scan's chunk sums).  Deterministic. */
int pamnet_csr_from_keys_i32(const int32_t* keys, int64_t m, int64_t rows, int32_t* ptr, int32_t* perm,
                             int32_t* cursor, int32_t* perm_tmp, int32_t* tmp, pamnet_stream_t stream);
/* The same with `cursor` already zero-filled by the caller (no fill launch of its own). */
int pamnet_csr_from_keys_z_i32(const int32_t* keys, int64_t m, int64_t rows, int32_t* ptr, int32_t* perm,
                               int32_t* cursor, int32_t* perm_tmp, int32_t* tmp, pamnet_stream_t stream);

/* row_of[q] = r for q in [ptr[r], ptr[r+1])  (repeat_interleave of row ids, models.py:76-77, 88-89).
 * `cap` = entries the output holds (the *_fill entry points take one too): nothing is written at or beyond it.  With sizes
 * read back from the device cap = ptr[rows] and never binds; it makes the zero-host-sync path (sizes assumed by the host,
 * verified later: pamnet_check_sizes_i32) memory-safe when the assumption is wrong. */
int pamnet_expand_rows_i32(const int32_t* ptr, int64_t rows, int32_t* row_of, int64_t cap, pamnet_stream_t stream);

/* CSR row filter: keep entries with nbr >= 0 and dist <= cut  (the cutoff masks, models.py:131-134, 147-156).
 * count -> (caller scans) -> fill. */
int pamnet_csr_filter_count_i32(const int32_t* ptr_in, const int32_t* nbr, const float* dist, int64_t rows, float cut,
                                int32_t* count, pamnet_stream_t stream);
int pamnet_csr_filter_fill_i32(const int32_t* ptr_in, const int32_t* nbr, const float* dist, int64_t rows, float cut,
                               const int32_t* ptr_out, int32_t* nbr_out, float* dist_out, int64_t cap,
                               pamnet_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Neighbour search (torch_cluster.radius / knn: models.py:110,128,143,301), self loops removed (models.py:63).
 * `gptr[b..b+1]` = node range of graph b (batch sorted).  Two-pass: count -> (caller scans) -> fill.
 * radius: neighbours j != i of the same graph with ||pos_i - pos_j|| <= r, ascending j.  Symmetric by construction --
 * unless max_neighbors binds.  max_neighbors (0 = unlimited; models.py:110,128 pass 1000, :301 passes 500): a query keeps
 * the first max_neighbors points of its graph within r in ascending index order, itself included in that count (the search
 * returns the query; remove_self_loops follows, models.py:63); the count pass ORs 64 into *cap_flag (nullable) when a row
 * was truncated -- the graph is then not symmetric and the caller must build general transposes.
 * n_graphs (0 = unknown) only selects the launch shape: one thread per node for molecule-sized graphs, one wavefront per
 * node from ~100 nodes per graph on; the output is the same.
 * ------------------------------------------------------------------------------------------------------------------ */
int pamnet_radius_count_i32(const float* pos, const int32_t* node_graph, const int32_t* gptr, int64_t n,
                            int64_t n_graphs, float r, int64_t max_neighbors, int32_t* count, int32_t* cap_flag,
                            pamnet_stream_t stream);
int pamnet_radius_fill_i32(const float* pos, const int32_t* node_graph, const int32_t* gptr, int64_t n,
                           int64_t n_graphs, float r, int64_t max_neighbors, const int32_t* ptr, int32_t* nbr, float* dist,
                           int32_t* row_of /* nullable: the query node of every entry */, int64_t cap,
                           pamnet_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Periodic cells (QM9-schema batches that carry `cell`): every displacement between two atoms of one graph is the
 * minimum-image one.  ONE image rule (csrc/geom_core.h min_image), used by every *_pbc_* entry point: the fp64 difference of
 * the two fp32 positions times the graph's inverse cell, the three fractional components rounded to the nearest integer
 * (the image n), n @ cell subtracted in fp64; the fp32 kernels round the three components once to fp32 and go on with the
 * arithmetic of their open-space twins.  n(i, j) == -n(j, i) exactly, so both directions of an edge carry bitwise equal
 * lengths, and with n = 0 the values are bitwise the open-space kernels'.
 *   pamnet_cell_prepare_f64: cell fp32 [n_graphs, 9] (row k of a graph's 3 x 3 = lattice vector a_k; an image of an atom is
 *     pos + n @ cell) -> cell_table [n_graphs, 18] doubles: the cell and its inverse (adjugate / determinant, fp64).  ORs 128
 *     into *flag (not zeroed here: the batch's validity word) when a cell is singular, not finite, or one of its three
 *     perpendicular heights |det| / |a_i x a_j| does not exceed 2 * cutoff -- the condition under which every ordered pair has
 *     at most one image within the cutoff and nearest-integer rounding finds it for any triclinic cell.  cutoff: the larger
 *     of the model's two.
 *   pamnet_radius_pbc_count/fill_i32: pamnet_radius_count/fill_i32 with the distance taken by the image rule: the same row
 *     order (ascending j), max_neighbors / cap_flag semantics, cap guard and launch-shape selection.  An atom never sees itself.
 * Argument order: the twin's, with cell_table (and node_graph where the twin has none) behind pos.
 * ------------------------------------------------------------------------------------------------------------------ */
int pamnet_cell_prepare_f64(const float* cell, int64_t n_graphs, float cutoff, double* cell_table, int32_t* flag,
                            pamnet_stream_t stream);
int pamnet_radius_pbc_count_i32(const float* pos, const double* cell_table, const int32_t* node_graph, const int32_t* gptr,
                                int64_t n, int64_t n_graphs, float r, int64_t max_neighbors, int32_t* count,
                                int32_t* cap_flag, pamnet_stream_t stream);
int pamnet_radius_pbc_fill_i32(const float* pos, const double* cell_table, const int32_t* node_graph, const int32_t* gptr,
                               int64_t n, int64_t n_graphs, float r, int64_t max_neighbors, const int32_t* ptr, int32_t* nbr,
                               float* dist, int32_t* row_of /* nullable */, int64_t cap, pamnet_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Periodic cells below twice the global cutoff: a global graph over ALL images (part of ABI 18: nothing existing changed).
 * Row i holds every pair (j, n) -- j any atom of i's graph, i itself included, n an integer triple -- with
 * |pos_i - pos_j - n @ cell| <= r, except the one entry j == i, n == 0; ascending (j, n0, n1, n2).  A multigraph: several edges
 * between the same two atoms, and from an atom to its own images.  Symmetric as a multiset: (i, j, n) has the reverse (j, i, -n),
 * with a bitwise equal length (csrc/geom_core.h image_disp: min_image with the image given instead of rounded).
 *   pamnet_cell_images_i32: cell_table [n_graphs, 18] (pamnet_cell_prepare_f64) -> img_box [n_graphs, 3]: N_k = ceil(cutoff /
 *     h_k), h_k the perpendicular height along lattice direction k (fp64).  The search tries, per pair, the images
 *     rint(fractional displacement) + m with |m_k| <= N_k: a superset of those within the cutoff.  ORs 128 into *flag when some
 *     N_k > 4 (a height below cutoff / 4) or the cell has no heights; that graph's box is then 0 0 0.
 *   pamnet_radius_img_count/fill_i32: the argument lists of pamnet_radius_pbc_count/fill_i32 with img_box behind cell_table and,
 *     in the fill, img [cap, 3] int32 behind row_of: the image of every entry, v = pos_row - pos_col - img @ cell (min_image's
 *     sign).  One wavefront per atom whatever n_graphs says.  max_neighbors never cuts a row (a cut multigraph is not symmetric):
 *     the count pass ORs 64 into *cap_flag when a row's entries, the query itself counted, exceed it.  Same cap guard and return
 *     codes as the twins.
 * ------------------------------------------------------------------------------------------------------------------ */
int pamnet_cell_images_i32(const double* cell_table, int64_t n_graphs, float cutoff, int32_t* img_box, int32_t* flag,
                           pamnet_stream_t stream);
int pamnet_radius_img_count_i32(const float* pos, const double* cell_table, const int32_t* img_box, const int32_t* node_graph,
                                const int32_t* gptr, int64_t n, int64_t n_graphs, float r, int64_t max_neighbors, int32_t* count,
                                int32_t* cap_flag, pamnet_stream_t stream);
int pamnet_radius_img_fill_i32(const float* pos, const double* cell_table, const int32_t* img_box, const int32_t* node_graph,
                               const int32_t* gptr, int64_t n, int64_t n_graphs, float r, int64_t max_neighbors, const int32_t* ptr,
                               int32_t* nbr, float* dist, int32_t* row_of /* nullable */, int32_t* img, int64_t cap,
                               pamnet_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Per-axis periodicity: slabs, wires and isolated molecules beside bulk cells (part of ABI 18: nothing existing changed).
 * pbc [n_graphs, 3] bytes: graph g repeats along lattice vector k when pbc[3 g + k] != 0.  The two entry points below are
 * pamnet_cell_prepare_f64 / pamnet_cell_images_i32 with that argument -- one kernel serves each pair, the entry points without
 * pbc are the case of three periodic axes; every other periodic entry point takes the table they make as it is.
 *   pamnet_cell_prepare_axes_f64: the table of the COMPLETED cell.  The vector handed over along an open axis is
 *     not used (it may be zero, short, or make the matrix singular); in its place stands a unit vector orthogonal to the
 *     periodic ones -- two periodic axes i, j: a_k' = a_i x a_j / |a_i x a_j|; one periodic axis i: a_j' = a_i x e normalised, e
 *     the coordinate unit vector along a_i's component of smallest magnitude (lowest index on ties), and a_k' = a_i x a_j'
 *     normalised; none: the identity.  cell_table holds the completed cell and its inverse, with the three inverse entries that
 *     form fractional component k of every open axis k set to +0.0: the image rule then rounds that component to 0 for every
 *     pair, so nothing is wrapped along k.  ORs 128 into *flag when the periodic vectors are degenerate (zero, parallel, not
 *     finite) or the height |det'| / |a_i' x a_j'| of a PERIODIC axis does not exceed 2 * cutoff; open axes are not tested.  A
 *     row with all three flags set is the cell as given: pamnet_cell_prepare_f64's 18 doubles and verdict bit for bit.  A null
 *     pbc is refused (PAMNET_ENULL).
 *   pamnet_cell_images_axes_i32: the box of that table with N_k = 0 and no verdict along open axes; null pbc refused likewise.
 * ------------------------------------------------------------------------------------------------------------------ */
int pamnet_cell_prepare_axes_f64(const float* cell, const uint8_t* pbc, int64_t n_graphs, float cutoff, double* cell_table,
                                 int32_t* flag, pamnet_stream_t stream);
int pamnet_cell_images_axes_i32(const double* cell_table, const uint8_t* pbc, int64_t n_graphs, float cutoff, int32_t* img_box,
                                int32_t* flag, pamnet_stream_t stream);

/* knn: for every query node its k nearest nodes of the same graph (itself included, as torch_cluster.knn does),
 * ordered by (distance, index); then the self entry is dropped and entries with dist > cutoff are masked out:
 * nbr[i*k + s] = neighbour index or -1, dist[i*k + s] = distance.  (models.py:143-150)
 * Ties in distance go to the lower index: the order is by (fp32 squared distance, index), exactly.  A masked entry (the
 * self entry, dist > cutoff) keeps its slot and its dist.  A graph with fewer than k nodes fills the slots it has; the
 * slots behind them are padding: nbr = -1, dist = +inf.  1 <= k <= 64 (PAMNET_EINVAL otherwise, nothing launched). */
int pamnet_knn_i32(const float* pos, const int32_t* node_graph, const int32_t* gptr, int64_t n, int32_t k,
                   float cutoff, int32_t* nbr, float* dist, pamnet_stream_t stream);
/* The kNN table (no cutoff: every entry but the self entry kept) together with what its two cuts keep per query -- cnt_a[i] /
 * cnt_b[i] = entries of row i with dist <= cut_a / cut_b (models.py:147-156: the global and the local graph of the RNA path
 * are cuts of one kNN search) -- and, after the caller's scans (pamnet_exclusive_scan_pair_i32), both cut lists written in
 * one pass: kept entries of row i at raw[i] + rank with the query id beside them (capped at cap), pointers clamped to cap
 * into ptr_a / ptr_b [n + 1].  The same arrays as pamnet_csr_filter_count/fill_i32 + pamnet_expand_rows_i32 per cut. */
int pamnet_knn_cut_i32(const float* pos, const int32_t* node_graph, const int32_t* gptr, int64_t n, int32_t k, float cut_a,
                       float cut_b, int32_t* nbr, float* dist, int32_t* cnt_a, int32_t* cnt_b, pamnet_stream_t stream);
/* total[0] (int64, zero on entry) = triplet + pair rows (models.py:68-98) of the graph the entries within `cut` of a kNN table
 * define (query -> neighbour, aggregated at the neighbour), before that graph is built: the kNN path's sizes in ONE host
 * read-back.  indeg: [n] int32 scratch, zero on entry. */
int pamnet_knn_tp_total_i64(const int32_t* nbr, const float* dist, int64_t n, int32_t k, float cut, int32_t with_triplets,
                            int32_t* indeg, int64_t* total, pamnet_stream_t stream);
int pamnet_knn_cut_fill_i32(const int32_t* nbr, const float* dist, int64_t n, int32_t k, float cut_a, const int32_t* raw_a,
                            int64_t cap_a, int32_t* nbr_a, float* dist_a, int32_t* row_a, int32_t* ptr_a, float cut_b,
                            const int32_t* raw_b, int64_t cap_b, int32_t* nbr_b, float* dist_b, int32_t* row_b, int32_t* ptr_b,
                            pamnet_stream_t stream);

/* Edge distances  dist[e] = ||pos[a[e]] - pos[b[e]]||   (PAMNet.get_edge_info, models.py:62-66) */
int pamnet_edge_dist_f32(const float* pos, const int32_t* a, const int32_t* b, int64_t m, float* dist,
                         pamnet_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Triplet / pair enumeration + angles  (PAMNet.indices, models.py:68-98, 263-281; angles models.py:165-177)
 * Local edges e = (src[e] -> dst[e]) are stored CSR by dst (lptr[n+1]).  For every edge e=(j->i) the combined row list
 * [tp_ptr[e], tp_ptr[e+1]) holds
 *   its triplets: every e'=(k->j), k != i       kind 0, tp_idx = e' (= idx_kj), tp_edge = e (= idx_ji), angle2
 *   its pairs:    every e'=(j'->i) incl. e'=e    kind 1, tp_idx = e' (= idx_jj_pair), tp_edge = e (= idx_ji_pair), angle1
 * i.e. the reference's cat(idx_kj, idx_jj_pair) / cat(idx_ji, idx_ji_pair) (local_message_passing.py:38-39) regrouped
 * by target edge.  with_triplets = 0 enumerates pairs only (PAMNet_s).  count -> (caller scans tpcount) -> fill.
 * ------------------------------------------------------------------------------------------------------------------ */
int pamnet_triplet_count_i32(const int32_t* lptr, const int32_t* src, const int32_t* dst, int64_t n_edges,
                             int32_t with_triplets, int32_t* tcount, int32_t* tpcount, pamnet_stream_t stream);
int pamnet_triplet_fill_f32(const float* pos, const int32_t* lptr, const int32_t* src, const int32_t* dst,
                            int64_t n_edges, int32_t with_triplets, const int32_t* tp_ptr, int32_t* tp_idx,
                            int32_t* tp_edge, float* tp_angle, int32_t* tp_kind, int64_t cap, pamnet_stream_t stream);
/* The same with both bond vectors of every row by the image rule of the periodic cells (see pamnet_cell_prepare_f64);
 * node_graph [n]: the graph of every atom. */
int pamnet_triplet_fill_pbc_f32(const float* pos, const double* cell_table, const int32_t* node_graph, const int32_t* lptr,
                                const int32_t* src, const int32_t* dst, int64_t n_edges, int32_t with_triplets,
                                const int32_t* tp_ptr, int32_t* tp_idx, int32_t* tp_edge, float* tp_angle, int32_t* tp_kind,
                                int64_t cap, pamnet_stream_t stream);
/* Transposed triplet / pair row list (for every source bond the rows that gather it, ascending: the (ptr, perm) that
 * pamnet_csr_from_keys_i32 returns for keys = tp_idx over n_edges rows) from the graph's structure instead of a counting sort
 * over the rows: count -> caller scans -> fill.  lt_ptr [n + 1] / lt_perm [n_edges]: the transposed bond list (bonds by source
 * atom, any order inside a row); tp_ptr / tcount as pamnet_triplet_count_i32 / the scan produced them; tt_ptr = the scanned
 * counts; cap = entries tt_perm holds.  No self loops. */
int pamnet_triplet_transpose_count_i32(const int32_t* lptr, const int32_t* src, const int32_t* dst, const int32_t* lt_ptr,
                                       const int32_t* lt_perm, int64_t n_edges, int32_t with_triplets, int32_t* count,
                                       pamnet_stream_t stream);
int pamnet_triplet_transpose_fill_i32(const int32_t* lptr, const int32_t* src, const int32_t* dst, const int32_t* lt_ptr,
                                      const int32_t* lt_perm, int64_t n_edges, int32_t with_triplets, const int32_t* tp_ptr,
                                      const int32_t* tcount, const int32_t* tt_ptr, int32_t* tt_perm, int64_t cap,
                                      pamnet_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Zero-host-sync graph construction (models.py:62-98,104-157 read their data-dependent sizes back to the
 * host through boolean masks / repeat_interleave).
 * check_sizes: up to 4 device-side totals (actual[k][0], e.g. the last element of a CSR pointer) against the values the
 *   host assumed; bit (2 << k) of flag[0] is set on a mismatch, bit 32 when *all_kept (a device bool, nullable) is false
 *   or *self_loops (int32, nullable) is non-zero.
 *   flag is NOT zeroed (pamnet_validate_inputs_i32 owns bit 1 of the same word).
 * collate: batch of n_graphs graphs sel[k] of a dataset kept resident as concatenated arrays (prefix sums src_nptr /
 *   src_eptr, bonds with graph-local endpoints): node features [n_out, x_width], positions (nullable), int32 batch
 *   vector, bonds with batch-level endpoints, the graphs' targets.  out_nptr / out_eptr: the batch's prefix sums (device,
 *   n_graphs + 1).
 * ------------------------------------------------------------------------------------------------------------------ */
/* Transposed CSR of a SYMMETRIC graph stored by target with ascending columns (radius graphs): rev[e] = position of the
 * reverse edge of e; (ptr, rev) equals what pamnet_csr_from_keys_i32(col) returns as (ptr, perm).  flag (nullable):
 * bit 64 is set if an edge has no reverse. */
int pamnet_reverse_edges_i32(const int32_t* ptr, const int32_t* row_of, const int32_t* col, int64_t m, int32_t* rev,
                             int32_t* flag, pamnet_stream_t stream);
/* out[k] (device int64) = *src[k], read as int32 (kind 0), bool / uint8 (1) or int64 (2); n <= 8.  The data-dependent sizes
 * of a batch in one launch, ahead of the one device->host copy graph construction makes. */
int pamnet_gather_scalars_i64(int64_t n, const void* const* src /* host array of device ptrs */,
                              const int32_t* kind /* host */, int64_t* out, pamnet_stream_t stream);
int pamnet_check_sizes_i32(int64_t n_checks, const int32_t* const* actual /* host array of device ptrs */,
                           const int64_t* expected /* host */, const void* all_kept, const int32_t* self_loops,
                           int32_t* flag, pamnet_stream_t stream);
/* The reference's index tensors (`x`, `edge_index`, `batch` of models.py:104-110; `j, i = edge_index` models.py:64) in
 * ONE launch: each is read as int64 (kind 1, what PyG hands over), int32 (2) or fp32 (3; kind 0 = no `x`) and written as
 * int32 -- node_graph [n], types [n] (element i read at x[i * x_stride]), src / dst [n_edges].  gptr_flag holds
 * n_graphs + 7 ints, zeroed by the call (the last four are spare zeroed words for the caller: the molecule-local builder's
 * batch totals live there), gptr_flag[0 .. n_graphs] = first node of every graph (the CSR pointer of the
 * sorted batch vector), gptr_flag[n_graphs + 1] = 1 when an index is out of range (batch unsorted / not in [0, n_graphs),
 * type not in [0, n_types), edge endpoint not in [0, n): the reference raises IndexError; offending entries are written
 * as 0 so that later kernels stay in bounds), gptr_flag[n_graphs + 2] = 1 when the edge list has a self loop
 * (remove_self_loops, models.py:63, would then not be a no-op). */
int pamnet_ingest_indices_i32(const void* batch, int32_t batch_kind, int64_t n, int64_t n_graphs, const void* x,
                              int32_t x_kind, int64_t x_stride, int64_t n_types, const void* edge_src,
                              const void* edge_dst, int32_t edge_kind, int64_t n_edges, int32_t* node_graph,
                              int32_t* gptr_flag, int32_t* types, int32_t* src, int32_t* dst, pamnet_stream_t stream);
/* out_a[q] = a[perm[q]], out_b[q] = b[perm[q]]: the bond list in CSR order of its targets (models.py:71-73); with
 * dist (nullable; then pos [n,3] is required) also dist[q] = ||pos[out_b[q]] - pos[out_a[q]]|| (models.py:65). */
int pamnet_gather2_i32(const int32_t* perm, const int32_t* a, const int32_t* b, int64_t m, int32_t* out_a,
                       int32_t* out_b, const float* pos, float* dist, pamnet_stream_t stream);
/* An edge list stored by query node, re-stored by neighbour (models.py:147-156 aggregate the kNN edges at the neighbour):
 * with perm = the stable counting sort of the neighbour column, out_q[e'] = q[perm[e']], out_dist[e'] = dist[perm[e']],
 * and inv[perm[e']] = e' (nullable) -- the positions of the query-ordered edges in the new list, i.e. together with the
 * query-ordered CSR pointer the transposed CSR the backward gathers d x[j] with. */
int pamnet_transpose_gather_i32(const int32_t* perm, const int32_t* q, const float* dist, int64_t m, int32_t* out_q,
                                float* out_dist, int32_t* inv, pamnet_stream_t stream);
int pamnet_collate_f32(int64_t n_graphs, const int32_t* sel, const int32_t* out_nptr, const int32_t* out_eptr,
                       const int32_t* src_nptr, const int32_t* src_eptr, const float* x, int64_t x_width,
                       const float* pos, const int32_t* esrc, const int32_t* edst, int64_t n_out, int64_t e_out,
                       float* out_x, float* out_pos, int32_t* out_batch, int32_t* out_esrc, int32_t* out_edst,
                       const float* y /* [graphs of the dataset] targets, nullable */, float* out_y /* [n_graphs] */,
                       pamnet_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Graph-construction engine: everything of PAMNet.forward that does not depend on the parameters -- index ingestion,
 * remove_self_loops, radius / knn graphs, cutoff masks, the SparseTensor CSRs, triplets / pairs and their angles
 * (models.py:62-98, 104-177), the transposed index lists of the backward and the spherical basis
 * (layers/basic.py:107-116) -- enqueued by ONE call (csrc/graph_engine.hip) for a batch whose data-dependent sizes the host
 * already knows (eg, el, tp: per-graph constants, pamnet_amd/store.py).  Same kernels, same order, same results as the
 * step-by-step entry points above; fills are capped by the sizes, and the device-side counts are compared with them by
 * pamnet_check_sizes_i32 into the flag word (field PAMNET_GF_FLAG), to be read whenever the host next synchronises.
 * `arena`: caller-owned int32 buffer of *arena_ints entries (pamnet_graph_plan); layout[f] = offset (in ints) of field f
 * inside it, or -1 when the batch has no such array (float fields are stored in place: reinterpret).  Batches with an
 * empty node / edge / row list are rejected (PAMNET_EINVAL): they take the step-by-step entry points.
 * ------------------------------------------------------------------------------------------------------------------ */
#define PAMNET_SCHEMA_QM9 0     /* x = atom types, pos, bond list (models.py:104-113) */
#define PAMNET_SCHEMA_PDBBIND 1 /* rows = xyz + features; radius graphs at both cutoffs (models.py:115-136) */
#define PAMNET_SCHEMA_RNA 2     /* rows = xyz + type; kNN graph cut at both cutoffs (models.py:138-157) */
typedef struct pamnet_graph_desc {
    int64_t n, n_graphs, n_bonds; /* nodes, graphs, directed bonds (QM9; 0 otherwise) */
    int64_t eg, el, tp;           /* sizes the host assumes: global edges, local edges, triplet + pair rows */
    const void* batch;            /* [n] graph id per node, sorted; int64 / int32 / fp32 by batch_kind (1 / 2 / 3) */
    const void* types;            /* QM9 / RNA: atom type of node i at types[i * types_stride], kind as above */
    int64_t types_stride, n_types;
    const float* pos;             /* QM9: [n, 3] */
    const float* rows;            /* PDBbind / RNA: [n, rows_width] fp32, xyz first */
    int64_t rows_width;
    const void* edge_src;         /* QM9: edge_index[0], edge_index[1] ([n_bonds] each), kind edge_kind */
    const void* edge_dst;
    int32_t schema, batch_kind, types_kind, edge_kind;
    int32_t with_triplets;        /* 0: pairs only (PAMNet_s) */
    int32_t need_grad;            /* 1: also build the transposed index lists the backward gathers with, and the two index hops of
                                     the dim-128 engine's local aggregation backward (TT_EDGE / TT_NODE); 2: the lists only */
    int32_t aggregate_at_query;   /* RNA: flow == 'target_to_source' (the global layer aggregates at the kNN query) */
    int32_t knn_k;                /* RNA: neighbours per query (models.py:143: 50) */
    float cutoff_l, cutoff_g;
    int32_t max_neighbors;        /* radius searches: torch_cluster's max_num_neighbors (models.py:110,128: 1000; :301: 500;
                                     0 = unlimited).  A batch in which it binds is flagged (bit 64 of the flag word): the one-call
                                     graph assumes symmetric radius graphs */
    int32_t mol_local;            /* QM9: 1 = the molecule-local builder (pamnet_mol_graph_*: the caller vouches for <= 64 atoms,
                                     <= 256 directed bonds per molecule and bonds grouped by molecule in batch order; a batch
                                     that is not so is flagged as a local-edge size mismatch) */
} pamnet_graph_desc;
enum {
    PAMNET_GF_NODE_GRAPH = 0, /* int32 [n] */
    PAMNET_GF_GPTR,           /* int32 [n_graphs + 1] first node of every graph */
    PAMNET_GF_FLAG,           /* int32 [1]: bit 1 invalid index inputs, bits 2 / 4 / 8 size mismatch (eg / el / tp), 32 self loops, 64 neighbour cap binds */
    PAMNET_GF_LOOPS,          /* int32 [1] */
    PAMNET_GF_TYPES,          /* int32 [n] */
    PAMNET_GF_POS,            /* fp32 [n, 3] (PDBbind / RNA; QM9 uses the caller's) */
    PAMNET_GF_SIGN,           /* fp32 [n] pooling sign (PDBbind, models.py:124) */
    PAMNET_GF_G_PTR, PAMNET_GF_G_ROW, PAMNET_GF_G_COL, PAMNET_GF_G_DIST,   /* global graph, CSR by aggregation target */
    PAMNET_GF_GT_PTR, PAMNET_GF_GT_PERM,                                     /* its transposed CSR (need_grad) */
    PAMNET_GF_L_PTR, PAMNET_GF_L_ROW, PAMNET_GF_L_COL, PAMNET_GF_L_DIST,   /* local graph */
    PAMNET_GF_LT_PTR, PAMNET_GF_LT_PERM,
    PAMNET_GF_T_PTR, PAMNET_GF_T_ROW, PAMNET_GF_T_COL, PAMNET_GF_T_ANGLE, PAMNET_GF_T_KIND,   /* triplet + pair rows */
    PAMNET_GF_TT_PTR, PAMNET_GF_TT_PERM,
    PAMNET_GF_CUTS,           /* int32 [<= 257] node-aligned work split of the fused global-edge kernels */
    PAMNET_GF_TT_EDGE, PAMNET_GF_TT_NODE,   /* int32 [tp] each: pamnet_triplet_transpose_aux_i32 (need_grad) */
    PAMNET_GRAPH_FIELDS
};
/* Molecule-local graph construction for the QM9 schema (positions + bond list given; models.py:62-98, 104-118, 165-177) --
 * bond CSR by target + bond lengths, triplet / pair rows + angles, radius graph at cutoff_g, and (need_grad) the transposed
 * index lists of the backward -- one wavefront per molecule, two launches instead of the ~14 of the step-by-step entry points
 * above, bit-identical arrays.  For batches of small molecules: <= 64 atoms and <= 256 directed bonds per molecule; bonds
 * grouped by molecule in batch order (torch_geometric collation, pamnet_collate_f32) with both ends in one molecule; no
 * self loops.  gptr [n_graphs + 1], src / dst int32 [n_bonds] as pamnet_ingest_indices_i32 returns them.
 *   count: mol_tot [n_graphs, 4] = (global edges, triplet + pair rows, first bond, violation bits) per molecule;
 *          totals [4] (zeroed by the caller) += (global edges, triplet + pair rows, violation bits (OR), bonds) over the
 *          molecules without a violation (bits: 1 atoms, 2 bonds, 4 a bond leaving its molecule / bonds not grouped);
 *   fill:  every array of `out`; eg_cap / tp_cap = what the buffers hold (writes beyond are dropped, pointers clamped).
 * Array sizes: *_ptr over nodes [n + 1] (g, l, lT) or over bonds [n_bonds + 1] (t, tT); g_* / gT_perm [eg_cap];
 * l_* / lT_perm [n_bonds]; t_* / tT_perm [tp_cap].  gT_ptr = g_ptr (a radius graph is symmetric: the transposed list is the
 * reverse-edge index).  The transposed lists are written only with need_grad. */
typedef struct pamnet_mol_graph_out {
    int32_t *g_ptr, *g_row, *g_col;
    float* g_dist;
    int32_t* gT_perm;
    int32_t *l_ptr, *l_row, *l_col;
    float* l_dist;
    int32_t *lT_ptr, *lT_perm;
    int32_t *t_ptr, *t_row, *t_col;
    float* t_angle;
    int32_t* t_kind;
    int32_t *tT_ptr, *tT_perm;
} pamnet_mol_graph_out;
int pamnet_mol_graph_count_i32(const float* pos, const int32_t* gptr, int64_t n, int64_t n_graphs, const int32_t* src,
                               const int32_t* dst, int64_t n_bonds, float cutoff_g, int32_t with_triplets, int32_t* mol_tot,
                               int32_t* totals, pamnet_stream_t stream);
int pamnet_mol_graph_fill_i32(const float* pos, const int32_t* gptr, int64_t n, int64_t n_graphs, const int32_t* src,
                              const int32_t* dst, int64_t n_bonds, float cutoff_g, int32_t with_triplets, int32_t need_grad,
                              const int32_t* mol_tot, int64_t eg_cap, int64_t tp_cap, const pamnet_mol_graph_out* out,
                              pamnet_stream_t stream);
/* Bond-free form of the same builder: no bond list is given, the local graph is the radius graph at cutoff_l inside every
 * molecule -- all ordered pairs (j -> i), i != j, |pos_i - pos_j| <= cutoff_l, by the rule and fp32 arithmetic of
 * pamnet_radius_count/fill_i32, no neighbour cap -- stored by target i, then source j; the global graph is the one at
 * cutoff_g as above (either cutoff may be the larger; both must be positive).  Limits as above: <= 64 atoms and <= 256
 * directed LOCAL edges per molecule (violation bits 1 / 2).  Every array is bit-identical to what the step-by-step entry
 * points give for that edge list (the transposed local list is the reverse-edge index: lT_ptr = l_ptr).
 *   count: mol_tot [n_graphs, 4] = (global edges, triplet + pair rows, LOCAL EDGES, violation bits) per molecule;
 *          totals [4] (zeroed by the caller) += (global edges, triplet + pair rows, violation bits (OR), local edges);
 *   fill:  n_local = totals[3] of the count launch over the same inputs; sizes as above with n_bonds = n_local.  A molecule's
 *          first local edge is the sum of the preceding molecules' counts in mol_tot; a molecule whose edges would not fit
 *          in n_local writes nothing. */
int pamnet_mol_graph_free_count_i32(const float* pos, const int32_t* gptr, int64_t n, int64_t n_graphs, float cutoff_l,
                                    float cutoff_g, int32_t with_triplets, int32_t* mol_tot, int32_t* totals,
                                    pamnet_stream_t stream);
int pamnet_mol_graph_free_fill_i32(const float* pos, const int32_t* gptr, int64_t n, int64_t n_graphs, int64_t n_local,
                                   float cutoff_l, float cutoff_g, int32_t with_triplets, int32_t need_grad,
                                   const int32_t* mol_tot, int64_t eg_cap, int64_t tp_cap, const pamnet_mol_graph_out* out,
                                   pamnet_stream_t stream);
/* The bond-free form under periodic cells: cell_table [n_graphs, 18] from pamnet_cell_prepare_f64 (prepared for max(cutoff_l,
 * cutoff_g): under that minimum-image condition both graphs are still simple symmetric graphs on the molecule's atoms).  Every
 * distance is the minimum-image one by the rule and arithmetic of pamnet_radius_pbc_count/fill_i32, every angle that of
 * pamnet_triplet_fill_pbc_f32; everything else -- arguments, validation, limits, mol_tot / totals, violation bits -- as in
 * the two entry points above, and every array bit-identical to what the step-by-step periodic entry points give.  The
 * kernels stay inside their arrays for any table content (a singular cell's inf / NaN distances pass no cutoff test). */
int pamnet_mol_graph_pbc_count_i32(const float* pos, const double* cell_table, const int32_t* gptr, int64_t n, int64_t n_graphs,
                                   float cutoff_l, float cutoff_g, int32_t with_triplets, int32_t* mol_tot, int32_t* totals,
                                   pamnet_stream_t stream);
int pamnet_mol_graph_pbc_fill_i32(const float* pos, const double* cell_table, const int32_t* gptr, int64_t n, int64_t n_graphs,
                                  int64_t n_local, float cutoff_l, float cutoff_g, int32_t with_triplets, int32_t need_grad,
                                  const int32_t* mol_tot, int64_t eg_cap, int64_t tp_cap, const pamnet_mol_graph_out* out,
                                  pamnet_stream_t stream);

int pamnet_graph_plan(const pamnet_graph_desc* desc, int64_t* layout /* [PAMNET_GRAPH_FIELDS] */, int64_t* arena_ints);
int pamnet_graph_build_i32(const pamnet_graph_desc* desc, int32_t* arena, float* sbf /* [tp, 42], nullable */,
                           pamnet_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Basis functions  (layers/basic.py:36-51 Envelope, :59-76 BesselBasisLayer, :79-116 SphericalBasisLayer; utils/sbf.py)
 * ------------------------------------------------------------------------------------------------------------------ */
/* rbf[e, n] = env(d_e/c) * sin(freq[n] * d_e/c),  n < 16, envelope exponent p = 5 */
int pamnet_rbf_fwd_f32(const float* dist, const float* freq, float cutoff, int64_t m, float* rbf,
                       pamnet_stream_t stream);
/* dfreq[n] = sum_e grad[e, n] * env(x_e) * x_e * cos(freq[n] x_e)   (freq is trainable: basic.py:65-72).
 * `partial` needs 16*2048 floats of scratch. */
int pamnet_rbf_bwd_f32(const float* dist, const float* freq, float cutoff, int64_t m, const float* grad,
                       float* dfreq, float* partial, pamnet_stream_t stream);
/* radial table rad[e, l*6+n] = env(x) * N_ln * j_l(z_ln x), x = d_e/c, evaluated in fp64 and rounded once to fp32 */
int pamnet_sbf_radial_f32(const float* dist, float cutoff, int64_t m, float* rad, pamnet_stream_t stream);
/* sbf[t, l*6+n] = rad[idx[t], l*6+n] * Y_l0(angle[t]) */
int pamnet_sbf_combine_f32(const float* rad, const int32_t* idx, const float* angle, int64_t m, float* sbf,
                           pamnet_stream_t stream);
/* The same basis layers for any PAMNet(config, num_spherical, num_radial, envelope_exponent) (models.py:22; the entries
 * above are specialised for the default (7, 6, 5) every script of the reference uses): num_spherical <= 16, num_radial <= 64,
 * envelope exponent p >= 1 (layers/basic.py:36-51).  zeros [ns * nr] (float32: utils/sbf.py:15-26 stores them so) and norm
 * [ns * nr] (float64: N_ln = 1 / sqrt(0.5 j_{l+1}(z_ln)^2), utils/sbf.py:43-49) are device tables the caller computes once
 * per model.  rad / sbf rows have ns * nr entries, index l * nr + n. */
int pamnet_rbf_fwd_env_f32(const float* dist, const float* freq, float cutoff, int32_t envelope_exponent, int64_t m,
                           float* rbf, pamnet_stream_t stream);
int pamnet_rbf_bwd_env_f32(const float* dist, const float* freq, float cutoff, int32_t envelope_exponent, int64_t m,
                           const float* grad, float* dfreq, float* partial, pamnet_stream_t stream);
int pamnet_sbf_radial_tab_f32(const float* dist, float cutoff, int64_t m, int32_t num_spherical, int32_t num_radial,
                              int32_t envelope_exponent, const float* zeros, const double* norm, float* rad,
                              pamnet_stream_t stream);
int pamnet_sbf_combine_tab_f32(const float* rad, const int32_t* idx, const float* angle, int64_t m, int32_t num_spherical,
                               int32_t num_radial, float* sbf, pamnet_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Geometric backward: d prediction / d positions (forces; the reference differentiates its geometry ops, models.py:62-66,
 * 165-177, layers/basic.py).  Default basis only (7, 6, envelope exponent 5).  Derivatives in fp64, rounded once; zero
 * beyond the cutoff (where the reference's envelope is cut to zero).  No atomics: fixed-order sums over CSR rows and
 * transposed row lists, bitwise reproducible.  Every pointer is required: a null pointer or a negative count returns
 * PAMNET_EINVAL.
 *   pamnet_rbf_ddist_f32:  ddist[e] = sum_n grad[e, n] d/dd [env(d/c) sin(freq[n] d/c)]          (grad: [m, 16])
 *   pamnet_sbf_bwd_f32:    gsbf [n_rows, 42] -> dangle[t] = sum_{l,n} gsbf[t, l, n] rad[idx[t], l, n] dY_l0/dtheta(angle[t]);
 *                          ddist[e] = sum_{l,n} (sum_{t in tt row e} gsbf[t, l, n] Y_l0(angle[t])) d rad[e, l, n] / dd,
 *                          with j_l' = j_{l-1} - (l+1)/u j_l.  tt_ptr [n_edges+1] / tt_perm [n_rows]: the rows that gather
 *                          each edge (pamnet_triplet_transpose_*).  rad: [n_edges, 42] scratch (the forward's table).
 *                          Rows gather edges: n_rows > 0 with n_edges == 0 returns PAMNET_EINVAL.
 *   pamnet_pos_bwd_f32:    dpos [n, 3] from d dist_g [eg], d dist_l [el] and d angle [tp]: global CSR g_* (rows = targets,
 *                          col = neighbour; dist = |p_row - p_col|) with its transposed list gt_*; local CSR l_* (rows = dst,
 *                          col = src) with lt_*; triplet / pair rows t_* (row = target edge e, col = source edge e', kind 0 =
 *                          triplet: theta = angle(p_j - p_i, p_k - p_j), kind 1 = pair: angle(p_i - p_j, p_j' - p_i)) with
 *                          tt_*.  Where |a x b| = 0 (theta = 0 or pi) the cross-product term contributes exactly 0.
 *                          bond_work: [el, 3] doubles of scratch.
 * ------------------------------------------------------------------------------------------------------------------ */
int pamnet_rbf_ddist_f32(const float* dist, const float* freq, float cutoff, int64_t m, const float* grad, float* ddist,
                         pamnet_stream_t stream);
int pamnet_sbf_bwd_f32(const float* gsbf, const float* dist, float cutoff, int64_t n_edges, const int32_t* idx,
                       const float* angle, int64_t n_rows, const int32_t* tt_ptr, const int32_t* tt_perm, float* rad,
                       float* dangle, float* ddist, pamnet_stream_t stream);
int pamnet_pos_bwd_f32(const float* pos, int64_t n, const int32_t* g_ptr, const int32_t* g_row, const int32_t* g_col,
                       const int32_t* gt_ptr, const int32_t* gt_perm, const float* ddist_g, int64_t eg, const int32_t* l_ptr,
                       const int32_t* l_row, const int32_t* l_col, const int32_t* lt_ptr, const int32_t* lt_perm,
                       const float* ddist_l, int64_t el, const int32_t* t_ptr, const int32_t* t_row, const int32_t* t_col,
                       const int32_t* t_kind, const int32_t* tt_ptr, const int32_t* tt_perm, const float* dangle, int64_t tp,
                       double* bond_work, float* dpos, pamnet_stream_t stream);

/* pamnet_pos_bwd_f32 for a graph built under periodic cells: every bond and global-edge vector is the minimum-image
 * displacement (the image integer from the function the forward's kernels used, the vector kept in fp64; the image does not
 * depend on the positions differentiably).  Same sums in the same fixed order, no atomics, same return codes. */
int pamnet_pos_bwd_pbc_f32(const float* pos, const double* cell_table, const int32_t* node_graph, int64_t n,
                           const int32_t* g_ptr, const int32_t* g_row, const int32_t* g_col, const int32_t* gt_ptr,
                           const int32_t* gt_perm, const float* ddist_g, int64_t eg, const int32_t* l_ptr, const int32_t* l_row,
                           const int32_t* l_col, const int32_t* lt_ptr, const int32_t* lt_perm, const float* ddist_l, int64_t el,
                           const int32_t* t_ptr, const int32_t* t_row, const int32_t* t_col, const int32_t* t_kind,
                           const int32_t* tt_ptr, const int32_t* tt_perm, const float* dangle, int64_t tp, double* bond_work,
                           float* dpos, pamnet_stream_t stream);

/* pamnet_pos_bwd_pbc_f32 that also returns the virial of every graph: dstrain[g][a][b] = sum over the directed global edges
 * and local bonds of graph g of v_e[a] * (d prediction / d v_e)[b], v_e the minimum-image vector -- the derivative under the
 * homogeneous deformation pos -> pos (I + eps_g), cell[g] -> cell[g] (I + eps_g) at eps = 0 with the image integers held fixed.
 * The argument list of pamnet_pos_bwd_pbc_f32, then gptr [n_graphs + 1] (first atom of every graph), n_graphs, atom_work
 * [n, 9] doubles of scratch and dstrain [n_graphs, 9] fp32.  dpos is bitwise what pamnet_pos_bwd_pbc_f32 writes.  Three
 * launches (bond gradients, positions + per-atom virial rows, one workgroup per graph adding them in a fixed order), no
 * atomics; a graph without edges gets exact zeros; n == 0 zero-fills dstrain.  Same return codes (part of ABI 18: nothing
 * existing changed). */
int pamnet_pos_bwd_pbc_virial_f32(const float* pos, const double* cell_table, const int32_t* node_graph, int64_t n,
                                  const int32_t* g_ptr, const int32_t* g_row, const int32_t* g_col, const int32_t* gt_ptr,
                                  const int32_t* gt_perm, const float* ddist_g, int64_t eg, const int32_t* l_ptr,
                                  const int32_t* l_row, const int32_t* l_col, const int32_t* lt_ptr, const int32_t* lt_perm,
                                  const float* ddist_l, int64_t el, const int32_t* t_ptr, const int32_t* t_row,
                                  const int32_t* t_col, const int32_t* t_kind, const int32_t* tt_ptr, const int32_t* tt_perm,
                                  const float* dangle, int64_t tp, double* bond_work, float* dpos, const int32_t* gptr,
                                  int64_t n_graphs, double* atom_work, float* dstrain, pamnet_stream_t stream);

/* The two periodic forms for a graph whose global list holds all images (pamnet_radius_img_fill_i32): the argument lists of
 * pamnet_pos_bwd_pbc_f32 / pamnet_pos_bwd_pbc_virial_f32 with g_img [eg, 3] behind g_col.  Global edge q is the vector of its
 * stored image, p_row - p_col - g_img[q] @ cell, in both the row and the transposed loop (there negated); gt_* is the general
 * transposed list of g_col.  An edge from an atom to its own image cancels in dpos and enters the virial once, through its row.
 * Local bonds and angles stay minimum-image: the same bond-gradient launch.  dpos of the virial form is bitwise the plain
 * form's.  Same sums in a fixed order, no atomics, same return codes (part of ABI 18: nothing existing changed). */
int pamnet_pos_bwd_img_f32(const float* pos, const double* cell_table, const int32_t* node_graph, int64_t n,
                           const int32_t* g_ptr, const int32_t* g_row, const int32_t* g_col, const int32_t* g_img,
                           const int32_t* gt_ptr, const int32_t* gt_perm, const float* ddist_g, int64_t eg, const int32_t* l_ptr,
                           const int32_t* l_row, const int32_t* l_col, const int32_t* lt_ptr, const int32_t* lt_perm,
                           const float* ddist_l, int64_t el, const int32_t* t_ptr, const int32_t* t_row, const int32_t* t_col,
                           const int32_t* t_kind, const int32_t* tt_ptr, const int32_t* tt_perm, const float* dangle, int64_t tp,
                           double* bond_work, float* dpos, pamnet_stream_t stream);
int pamnet_pos_bwd_img_virial_f32(const float* pos, const double* cell_table, const int32_t* node_graph, int64_t n,
                                  const int32_t* g_ptr, const int32_t* g_row, const int32_t* g_col, const int32_t* g_img,
                                  const int32_t* gt_ptr, const int32_t* gt_perm, const float* ddist_g, int64_t eg,
                                  const int32_t* l_ptr, const int32_t* l_row, const int32_t* l_col, const int32_t* lt_ptr,
                                  const int32_t* lt_perm, const float* ddist_l, int64_t el, const int32_t* t_ptr,
                                  const int32_t* t_row, const int32_t* t_col, const int32_t* t_kind, const int32_t* tt_ptr,
                                  const int32_t* tt_perm, const float* dangle, int64_t tp, double* bond_work, float* dpos,
                                  const int32_t* gptr, int64_t n_graphs, double* atom_work, float* dstrain,
                                  pamnet_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Structure relaxation: one FIRE step (Bitzek et al., Phys. Rev. Lett. 97, 170201, 2006; unit masses) of every graph of a
 * batch, in one launch (csrc/relax.hip; the reference has no optimiser of structures).  Each graph carries its own state, so
 * its trajectory does not depend on what else the batch holds.
 *   pos, vel [n, 3] fp32, updated in place;  dpos [n, 3] fp32 = dE/dpos, f = -dpos;  fixed [n] uint8 or NULL: an atom
 *   with fixed[a] != 0 has f = v = 0, enters no sum and no maximum, and its rows of pos and vel are neither read nor
 *   written;  gptr [n_graphs + 1]: first atom of every graph (kept inside [0, n]).
 *   Per graph: dt, a [n_graphs] fp64;  n_pos, steps, status [n_graphs] int32 (status 0 = running, 1 = converged, 2 = failed);
 *   fmax [n_graphs] fp32 (output).  The caller starts with vel = 0, dt = dt0, a = a0, n_pos = steps = status = 0.
 *   fmax_tol_g [n_graphs] fp32 or NULL: the convergence threshold of every graph; NULL: fmax_tol for all.
 * The step of graph g, all sums and maxima over the free atoms of g:
 *   1. status[g] != 0: nothing that belongs to g is read-modified or written.
 *   2. F2 = sum |f|^2, fm = max |f| (NaN-propagating); fmax[g] = fm.  F2 not finite: status[g] = 2, nothing else changes.
 *      Else fm < tolerance: status[g] = 1, nothing else changes (a graph without free atoms has fm = 0).
 *   3. P = sum f.v, V2 = sum |v|^2.  V2 == 0 (the first step): nothing.  Else P > 0: n_pos += 1; if n_pos > n_min then
 *      dt = min(dt f_inc, dt_max) and a *= f_a; then v <- (1 - a) v + a sqrt(V2 / F2) f.  Else (P <= 0): v <- 0, a = a0,
 *      dt *= f_dec, n_pos = 0.
 *   4. v <- v + dt f.
 *   5. dr = dt v, s = min(1, max_step / max |dr|) (s = 1 where the maximum is 0), pos <- pos + s dr.  v is not scaled.
 *   6. steps[g] += 1.
 * THE ORDER: the graph's decision comes first -- n_pos, dt and a are updated before any atom moves -- so the mixing of step 3
 * uses the updated a and steps 4 and 5 the updated dt.
 * Arithmetic in fp64 from the fp32 inputs, one rounding to fp32 at each store of pos and vel.  Sums in a fixed order (a
 * thread's atoms ascending, wavefront butterfly, the wavefronts in order through LDS), no atomics: the outputs of a graph
 * are bitwise repeatable and bitwise the same whether it is stepped alone or inside any batch.  One workgroup per graph.
 * Returns PAMNET_ENULL for a null required pointer; PAMNET_EINVAL for a negative count, n_graphs above 2^31 - 1, n_min < 0, a NaN fmax_tol, or one of
 * dt_max, max_step, f_inc, f_dec, a0, f_a that is not positive and finite.  n_graphs == 0 launches nothing.  (Part of ABI 18:
 * nothing existing changed.)
 * ------------------------------------------------------------------------------------------------------------------ */
int pamnet_fire_step_f32(float* pos, float* vel, const float* dpos, const uint8_t* fixed, const int32_t* gptr, int64_t n,
                         int64_t n_graphs, double* dt, double* a, int32_t* n_pos, int32_t* steps, int32_t* status, float* fmax,
                         const float* fmax_tol_g, double fmax_tol, double dt_max, double max_step, int32_t n_min, double f_inc,
                         double f_dec, double a0, double f_a, pamnet_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Structure relaxation, quasi-Newton: one limited-memory BFGS step (Nocedal, Math. Comp. 35, 773, 1980; the two-loop recursion
 * with the scaled initial matrix gamma I of Liu and Nocedal, Math. Program. 45, 503, 1989; no line search) of every graph of
 * a batch, in one launch (csrc/lbfgs.hip).  Every piece of optimiser state -- the history of pairs, its ring position, the
 * curvature test, the scaling, the descent check and the step cap -- is per graph, so a graph's trajectory does not depend on
 * what else the batch holds.
 *   pos [n, 3] fp32, updated in place;  dpos [n, 3] fp32 = gr = dE/dpos;  fixed, gptr, fmax_tol_g / fmax_tol, status, steps, fmax:
 *   as for pamnet_fire_step_f32.  An atom with fixed[a] != 0 enters no sum and no maximum, and its rows of pos, prev_pos,
 *   prev_dpos, hist_s, hist_y and work are neither read nor written.
 *   memory: m, the pairs a graph keeps, 1 .. 32, one value per launch (it is the leading extent of hist_s / hist_y and the row
 *   length of rho, so it stays the same over a relaxation).
 *   prev_pos, prev_dpos [n, 3] fp32: the positions and the gradient of the graph's last step.
 *   hist_s, hist_y [m, n, 3] fp64: ring slot k of atom a is row k n + a.  work [n, 3] fp64: the vector of the two-loop
 *   recursion (q, then z); its contents on return are unspecified.
 *   Per graph: rho [n_graphs, m] fp64 (1 / y.s of the pair in each slot);  gamma [n_graphs] fp64;  head (the slot the next pair
 *   goes to), count (the pairs held), has_prev, skipped, resets [n_graphs] int32.  The caller starts with all of them 0 (a
 *   head outside [0, m) is taken modulo m and a count outside [0, m] clamped, so that no slot index leaves the arrays).
 * The step of graph g, all sums and maxima over the free atoms of g, |.| of an atom the norm of its three components:
 *   1. status[g] != 0: nothing that belongs to g is read-modified or written.
 *   2. F2 = sum |gr|^2, fm = max |gr|; fmax[g] = fm.  F2 not finite: status[g] = 2 and fmax[g] = sqrt(F2) (NaN or +inf, as
 *      pamnet_fire_step_f32 reports it), nothing else changes.  Else fm < tolerance: status[g] = 1, nothing else changes (a
 *      graph without free atoms has fm = 0).
 *   3. If has_prev[g]: s = pos - prev_pos and y = gr - prev_dpos, one fp64 subtraction per component from the fp32 operands;
 *      ss = sum s.s, yy = sum y.y, ys = sum s.y.  If ys > skip_tol sqrt(ss yy): s and y are stored in slot head[g] of hist_s /
 *      hist_y, rho[g][head] = 1 / ys, gamma[g] = ys / yy, head = (head + 1) mod m, count = min(count + 1, m).  Otherwise (a NaN
 *      included) skipped[g] += 1 and the history stays as it is.  skipped is diagnostic only.
 *   4. The two-loop recursion over the count pairs held, pair j = 0 .. count - 1 in slot (head - 1 - j) mod m (newest first):
 *      q = gr;  for j = 0 .. count - 1: a_j = rho_j (s_j . q), q -= a_j y_j;  z = h0 q with h0 = gamma[g] if count > 0, else
 *      1 / alpha;  for j = count - 1 .. 0 (oldest first): b = rho_j (y_j . z), z += (a_j - b) s_j.
 *   5. D = sum z . gr.  If not D > 0 (a NaN included): the history is cleared, count = head = 0 (has_prev and gamma stay; gamma
 *      is not read while count = 0), z = gr / alpha, resets[g] += 1, and the largest |z| is taken as fm / alpha.
 *   6. L = max |z|, c = L > max_step ? max_step / L : 1;  prev_pos <- pos, prev_dpos <- gr, has_prev = 1;
 *      pos <- (float)(pos - c z);  steps[g] += 1.
 * The next step's s is the difference of the fp32 positions as they were stored: the history sees the move that was made,
 * rounding and cap included.
 * Arithmetic in fp64 from the fp32 inputs, one rounding to fp32 at the store of pos.  Sums in the fixed order of
 * pamnet_fire_step_f32 (a thread's atoms ascending, wavefront butterfly, the wavefronts in order through LDS), no atomics, and an
 * atom's rows of hist_s, hist_y and work are touched by one thread only: the outputs of a graph are bitwise repeatable and
 * bitwise the same whether it is stepped alone or inside any batch.  One workgroup per graph, 2 count + 2 workgroup
 * reductions.
 * Returns PAMNET_ENULL for a null required pointer (fixed and fmax_tol_g may be null); PAMNET_EINVAL for a negative count,
 * n_graphs above 2^31 - 1, memory outside 1 .. 32, a NaN fmax_tol, alpha or max_step not positive and finite, or skip_tol
 * negative or not finite.  n_graphs == 0 launches nothing.  (Part of ABI 18: nothing existing changed.)
 * ------------------------------------------------------------------------------------------------------------------ */
int pamnet_lbfgs_step_f32(float* pos, const float* dpos, const uint8_t* fixed, const int32_t* gptr, int64_t n, int64_t n_graphs,
                          float* prev_pos, float* prev_dpos, double* hist_s, double* hist_y, double* work, double* rho,
                          double* gamma, int32_t* head, int32_t* count, int32_t* has_prev, int32_t* skipped, int32_t* resets,
                          int32_t* steps, int32_t* status, float* fmax, const float* fmax_tol_g, double fmax_tol, int32_t memory,
                          double alpha, double max_step, double skip_tol, pamnet_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Cell relaxation: one FIRE step over the atoms AND the cell of every graph of a batch, in one launch (csrc/relax_cell.hip).
 * The unit-cell-filter formulation (Tadmor et al., Phys. Rev. B 59, 235, 1999; ASE's UnitCellFilter, whose deformation gradient
 * is the transpose of this one) in the project's row-vector convention, pos -> pos (I + eps), cell -> cell (I + eps):
 *   per graph a reference cell cell0 (rows = lattice vectors, never written) and a deformation gradient F (starts at I);
 *   the current cell is C = cell0 F, the generalised atom coordinates are x~ = pos F^-1, the generalised cell coordinate is
 *   L F with L the graph's cell factor.  vel holds the generalised velocities v~ of the atoms, vcell those of L F.
 * Arguments beyond those of pamnet_fire_step_f32 (all [n_graphs, 9] row-major 3 x 3 unless noted):
 *   dstrain fp32: the virial W = dE/d eps at zero strain;  cell0 fp32, read only;  cell fp32, written: fp32(cell0 F) of the new
 *   geometry;  F, vcell fp64: state (the caller starts with F = I, vcell = 0);  cell_dof [n_graphs] uint8 or NULL: 0 = the
 *   graph keeps its cell, NULL = every graph relaxes its cell;  cell_factor [n_graphs] fp64: L (positive; the caller's to keep
 *   so);  pressure_g [n_graphs] fp64 or NULL: NULL means the scalar pressure p holds for every graph, and likewise smax_tol_g
 *   [n_graphs] fp32 / smax_tol, the stress threshold (as fmax_tol_g / fmax_tol: the scalar beside a given array is not looked
 *   at);  hydrostatic: 0 / 1, for the whole launch;  smax [n_graphs] fp32 (output, beside fmax).
 * The step of graph g with cell_dof[g] != 0; "free" = the atoms of g that are not fixed, f = -dpos, M^T = transpose:
 *   0. status[g] != 0: nothing that belongs to g is read-modified or written.
 *   1. V = |det(cell0 F)|.  S = (W + W^T) / 2 + p V I.  hydrostatic: S <- (tr S / 3) I.  sm = max_ij |S_ij| / V (NaN-propagating).
 *   2. fm = max |f| over the free atoms.  Atom force g_a = f_a F^T, cell force g_c = -(F^-T S) / L (nine entries).
 *   3. F2 = sum_free |g_a|^2 + sum g_c^2, the nine cell terms added after the sum over the atoms, in index order (and so for P
 *      and V2 below).  F2 or V not finite, or V == 0: status[g] = 2, fmax[g] = sqrt(F2), smax[g] = sm, nothing else is written.
 *      Else fm < fmax tolerance and sm < smax tolerance: status[g] = 1, fmax[g] = fm, smax[g] = sm, nothing else is written.
 *   4. P = sum g_a . v~_a + sum g_c v_c, V2 = sum |v~_a|^2 + sum v_c^2, and the decision of pamnet_fire_step_f32, step 3,
 *      verbatim: V2 == 0: nothing.  Else P > 0: n_pos += 1; if n_pos > n_min then dt = min(dt f_inc, dt_max) and a *= f_a; then
 *      c_v = 1 - a, c_f = a sqrt(V2 / F2).  Else c_v = 0 (c_f = 0), a = a0, dt *= f_dec, n_pos = 0.  (n_pos, dt, a first.)
 *   5. v~ <- (c_v v~ + c_f g) + dt g, for the rows of the free atoms and the three rows of the cell alike.
 *   6. s = min(1, max_step / m), m the largest norm among the rows dt v~_a of the free atoms and the three rows of dt v_c (s = 1
 *      where m is 0): the cell moves by at most max_step / L in strain per step.
 *   7. F_new = F + s dt v_c / L.  det F_new not positive and finite: status[g] = 2, fmax[g] = fm, smax[g] = sm, nothing else is
 *      written.
 *   8. D = F^-1 F_new.
 *   9. Every atom of g, fixed ones included: pos_a <- pos_a D, and for a free atom + s dt v~_a F_new (one rounding).  A fixed
 *      atom keeps its generalised coordinate and so follows the cell; its row of vel is neither read nor written.  vel <- v~.
 *  10. cell[g] = fp32(cell0 F_new), F[g] = F_new, vcell[g] = v_c (not scaled), steps[g] += 1; fmax[g] = fm, smax[g] = sm, and
 *      dt, a, n_pos are written.
 * A graph with cell_dof[g] == 0 takes the rule of pamnet_fire_step_f32 exactly: its pos, vel, dt, a, n_pos, steps, status and
 * fmax are bitwise what that entry point gives (convergence on fm alone; its fixed atoms do not move), and its cell, F, vcell
 * and smax are not written; dstrain, cell0, cell_factor and the pressure of that graph are not read.
 * Arithmetic in fp64 from the fp32 inputs, one rounding at each fp32 store; sums in the fixed order of pamnet_fire_step_f32,
 * every thread of the graph's workgroup forming the 3 x 3 algebra and the decision alike; no atomics: the outputs of a graph
 * are bitwise repeatable and bitwise the same alone or inside any batch.  One workgroup per graph.
 * Returns PAMNET_ENULL for a null required pointer (fixed, cell_dof, fmax_tol_g, smax_tol_g, pressure_g may be NULL);
 * PAMNET_EINVAL for a negative count, n_graphs above 2^31 - 1, n_min < 0, hydrostatic other than 0 / 1, a NaN fmax_tol or
 * smax_tol, a pressure that is not finite, or one of dt_max, max_step, f_inc, f_dec, a0, f_a that is not positive and finite.
 * n_graphs == 0 launches nothing.  (Part of ABI 18: nothing existing changed.)
 * ------------------------------------------------------------------------------------------------------------------ */
int pamnet_fire_cell_step_f32(float* pos, float* vel, const float* dpos, const float* dstrain, const uint8_t* fixed,
                              const int32_t* gptr, int64_t n, int64_t n_graphs, const float* cell0, float* cell, double* F,
                              double* vcell, const uint8_t* cell_dof, const double* cell_factor, double* dt, double* a,
                              int32_t* n_pos, int32_t* steps, int32_t* status, float* fmax, float* smax,
                              const float* fmax_tol_g, const float* smax_tol_g, const double* pressure_g, double fmax_tol,
                              double smax_tol, double pressure, int32_t hydrostatic, double dt_max, double max_step,
                              int32_t n_min, double f_inc, double f_dec, double a0, double f_a, pamnet_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Nudged elastic band: the projected force of every image of every band of a batch, in one launch (csrc/neb.hip; the
 * reference has no path method).  Improved tangent: Henkelman & Jonsson, J. Chem. Phys. 113, 9978 (2000); climbing image:
 * Henkelman, Uberuaga & Jonsson, J. Chem. Phys. 113, 9901 (2000).  An image is a graph; a band is a run of consecutive graphs.
 *   pos, dpos [n, 3] fp32: positions (unwrapped: the entry point takes no cell) and dE/dpos, F = -dpos;  energy [n_graphs]
 *   fp32;  fixed [n] uint8 or NULL;  gptr [n_graphs + 1]: first atom of every graph (kept inside [0, n]);  band_ptr
 *   [n_bands + 1]: band b is the graphs band_ptr[b] .. band_ptr[b + 1] - 1 (kept inside [0, n_graphs));  band_of [n_graphs]:
 *   the band of every graph (a graph whose entry is outside [0, n_bands) is left alone);  band_status [n_bands] int32 or NULL:
 *   nonzero = nothing that belongs to an image of the band is written (the status vector of pamnet_fire_step_f32 over the
 *   bands);  climb [n_bands] uint8 or NULL: nonzero = the band has a climbing image;  k_b [n_bands] fp64 or NULL: the spring
 *   constant of every band; NULL: k for all (the scalar beside a given array is not looked at).
 *   Outputs: dneb [n, 3] fp32 = -F_neb, in the sign convention of dpos, so that it feeds pamnet_fire_step_f32 unchanged (it
 *   must not alias dpos);  seg [n_graphs] fp64 or NULL: |d-|, the distance to the previous image of the band, 0 on a band's
 *   first image;  fpar [n_graphs] fp64 or NULL: F . t^, 0 on a band's first and last image.
 * The rule of image i = graph g of band b.  Its neighbours -/+ are the graphs g - 1 / g + 1, atoms matched by their offset
 * inside the graph.  An atom of g is free where fixed[a] == 0 (the image's own row decides).  All sums run over the free atoms
 * of g; the rows of pos and dpos of a fixed atom, and the neighbours' rows at its offset, are never read; its row of dneb is 0.
 *   1. The first and the last image of a band write 0 to all their rows of dneb.  (A band of one or two images is all
 *      endpoints.)  The last image still reports seg.
 *   2. An interior image whose atom count differs from either neighbour's: every free row of dneb is NaN, fpar = seg = NaN.  On
 *      a band's last image seg is NaN where the count differs from the previous image's.
 *   3. d+ = R_{i+1} - R_i, d- = R_i - R_{i-1}.  The six sums Spp = |d+|^2, Smm = |d-|^2, Spm = d+ . d-, Fp = F . d+,
 *      Fm = F . d-, F2 = |F|^2.  seg = sqrt(Smm).
 *   4. E-, E0, E+ = the fp32 energies widened to fp64.  Any of them or any of the six sums not finite: every free row of dneb
 *      is NaN and fpar = NaN (so that pamnet_fire_step_f32 fails the band).
 *   5. The tangent t = cp d+ + cm d-:  E+ > E0 > E-: (cp, cm) = (1, 0).  E+ < E0 < E-: (0, 1).  Otherwise, with
 *      hi = max(|E+ - E0|, |E- - E0|) and lo = the min of the two: E+ > E-: (hi, lo), else (lo, hi).
 *      |t|^2 = cp^2 Spp + 2 cp cm Spm + cm^2 Smm and F . t = cp Fp + cm Fm.  |t|^2 > 0: t^ = t / |t| and fpar = F . t / |t|;
 *      else t^ = 0 and fpar = 0: the image feels its plain force.
 *   6. The climbing image of a band with climb[b] != 0 is its interior image of largest energy, found by scanning the interior
 *      images upward with `>` from -infinity: a tie goes to the lowest index, a NaN or -infinity never climbs.  On it
 *      F_neb = F - 2 fpar t^.
 *   7. Every other interior image: F_neb = F - fpar t^ + k (sqrt(Spp) - sqrt(Smm)) t^.
 * Arithmetic in fp64 from the fp32 inputs, one rounding at each store of dneb.  Sums in the fixed order of
 * pamnet_fire_step_f32 (a thread's atoms ascending, wavefront butterfly, the wavefronts in order through LDS); every thread of
 * the image's workgroup forms the decision and scans the band's energies itself; no atomics and nothing exchanged between
 * workgroups: the outputs of a band are bitwise repeatable and bitwise the same alone or inside any batch.  One workgroup per
 * image.
 * Returns PAMNET_ENULL for a null required pointer (fixed, band_status, climb, k_b, seg and fpar may be NULL); PAMNET_EINVAL for
 * a negative count, n_graphs or n_bands above 2^31 - 1, or, where k_b is NULL, a k that is negative or NaN.  n_graphs == 0
 * launches nothing.  (Part of ABI 18: nothing existing changed.)
 * ------------------------------------------------------------------------------------------------------------------ */
int pamnet_neb_force_f32(const float* pos, const float* dpos, const float* energy, const uint8_t* fixed, const int32_t* gptr,
                         int64_t n, int64_t n_graphs, const int32_t* band_ptr, const int32_t* band_of, int64_t n_bands,
                         const int32_t* band_status, const uint8_t* climb, const double* k_b, double k, float* dneb,
                         double* seg, double* fpar, pamnet_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Vibrational analysis: mass-weighted Hessians by central differences of dE/dpos, and their eigenvalues and eigenvectors
 * (csrc/vib.hip, csrc/eig.hip; the reference has neither second derivatives nor an eigensolver).  The model has no second
 * derivatives, so the displaced copies of a structure are graphs of one batch and one evaluation differentiates many of them.
 *
 * THE LAYOUT, shared by the three entry points.  Graph g has F_g free atoms, their batch-wide atom indices ascending in
 * free_idx[fptr[g] .. fptr[g + 1]) (both int32).  Its matrix has dimension d_g = 3 F_g and is stored row-major at moff[g] in a
 * packed fp64 array; moff is int64 [n_graphs + 1], the prefix sum of d_g^2, and dptr is int64 [n_graphs + 1], the prefix sum of
 * d_g.  Row and column 3 f + c is free atom f, component c.  Rows of fixed atoms do not exist.
 * ONE EVALUATION handles `pairs` = r central-difference pairs per graph: the evaluated batch is 2 r copies of the original
 * batch of n atoms and n_graphs graphs, copy-major: copy 2 c is the + and copy 2 c + 1 the - displacement of pair c; graph g
 * of copy k is graph k n_graphs + g, its atoms start at k n + gptr[g].  In evaluation t, pair c of graph g has job
 * j = t r + c: where j < 3 F_g it displaces component j % 3 of free atom f = j / 3, a = free_idx[fptr[g] + f]; otherwise the
 * pair is idle.
 *
 * pamnet_vib_displace_f32: writes pos_out [2 r n, 3] fp32 in one launch.  Every copy is pos0 [n, 3], bit for bit, except the
 * one displaced coordinate of an active pair: x+- = (float)((double)x0 +- delta).  Idle pairs are plain copies.  gptr
 * [n_graphs + 1] int32: first atom of every graph (kept inside [0, n]; rows of pos_out that belong to no graph are not
 * written).  One workgroup per (graph, copy); each element is stored once.
 *
 * pamnet_vib_rows_f64: reads dpos [2 r n, 3] fp32 (the evaluation's dE/dpos), pos0 and masses (fp32 [n], or NULL: unit
 * masses), and for every active pair stores row 3 f + c of graph g's matrix in h, once:
 *   h(3 f + c, 3 f' + c') = ((double)dE+[a', c'] - (double)dE-[a', c']) / ((double)x+ - (double)x-) / sqrt((double)m_a (double)m_a')
 * with a' = free_idx[fptr[g] + f'], dE+- the rows of copies 2 c and 2 c + 1, and x+- recomputed exactly as by the displace
 * launch: the divisor is the displacement as it was realised in fp32, not 2 delta.  Nothing is written for an idle pair.  No
 * atomics, no accumulation: over the sweep t = 0 .. ceil(3 max F_g / r) - 1 every element of every matrix is stored exactly
 * once.  An entry of free_idx outside [0, n) is not followed (its elements are NaN).  One workgroup per (graph, pair).
 *
 * Both return PAMNET_ENULL for a null required pointer (masses may be NULL); PAMNET_EINVAL for a negative n, n_graphs or t,
 * n_graphs above 2^31 - 1, pairs < 1 or above 32767, or a delta that is not positive and finite.  n_graphs == 0 or n == 0
 * launches nothing.
 *
 * pamnet_sym_eig_f64: eigenvalues and eigenvectors of n_mat packed symmetric matrices, one workgroup per matrix, by cyclic
 * Jacobi in fp64.  a, v: packed fp64 of moff[n_mat] elements; w: fp64 of dptr[n_mat]; status, sweeps: int32 [n_mat].  For a
 * matrix of dimension d (1 <= d <= 192):
 *   Input.    A_pq <- (a_pq + a_qp) / 2 (finite-difference Hessians are not exactly symmetric; this is part of the rule); A0 is
 *             this matrix.  V <- I.  a is the workspace: its contents are unspecified on return.
 *   Schedule. m = d rounded up to even.  A sweep is the rounds rho = 0 .. m - 2; round rho holds the m / 2 disjoint pairs
 *             (m - 1, rho) and ((rho + k) mod (m - 1), (rho - k) mod (m - 1)) for k = 1 .. m / 2 - 1, each ordered as p < q.  A
 *             pair with q >= d is a bye.  Every pair p < q < d occurs exactly once per sweep.
 *   Rotation. All rotations of a round are formed from the matrix as it stands at the start of the round, with a_pq the
 *             element of the upper triangle.  a_pq == 0: no rotation.  Otherwise theta = (a_qq - a_pp) / (2 a_pq),
 *             t = sign(theta) / (|theta| + sqrt(theta^2 + 1)) with sign(0) = +1, c = 1 / sqrt(t^2 + 1), s = t c.  First all
 *             column updates, (a_rp, a_rq) <- (c a_rp - s a_rq, s a_rp + c a_rq) for every row r and every pair; then all row
 *             updates, (a_pr, a_qr) <- (c a_pr - s a_qr, s a_pr + c a_qr) for every column r, after which a_pp = a_pp - t a_pq,
 *             a_qq = a_qq + t a_pq (from the values at the start of the round) and a_pq = a_qp = 0 are set exactly.  The rows
 *             p and q of V are rotated like the rows of A.
 *   Stop.     After each sweep off = sqrt(sum_{p != q} a_pq^2); the solver stops when off <= tol |A0|_F or after max_sweeps
 *             sweeps.  (So at least one sweep is taken; a diagonal matrix takes one without a rotation.)  Both sums are taken
 *             in a fixed order -- a thread's elements ascending, the wavefront butterfly, the wavefronts in order through LDS --
 *             and every thread of the workgroup reads the same number, so every exit is uniform.
 *   Output.   w[dptr[g] ..] ascending: eigenvalue k of the final diagonal goes to the position that counts the entries below
 *             it, ties by the diagonal index.  Row k of the matrix at v + moff[g] is the unit eigenvector of w[k]; its
 *             component of largest magnitude is positive, the lowest index on a tie.  sweeps[g] = the sweeps taken.
 *             status[g] = 0 converged; 1 max_sweeps reached (w and v are still written); 2 a non-finite entry in the input (w
 *             and v of that matrix are NaN, sweeps[g] = 0); 3 d > 192 (nothing else of that matrix is written).  d <= 0: nothing
 *             is written at all.  d = 1 is one sweep of one bye: w = a, v = 1.
 * No atomics, nothing exchanged between workgroups, every element of a phase computed by one thread: the results of a matrix
 * are bitwise repeatable and bitwise the same alone or inside any batch, at any position.  A and V are worked on in place in
 * global memory (192^2 fp64 is 288 KiB, more than the 160 KiB of LDS), with workgroup barriers between the parameter, column
 * and row phases of a round; the round's rotations go through LDS, and so does A itself where d <= 96 (72 KiB, reserved by every
 * launch; the same arithmetic, the same bits).  192 = 3 x 64 is the 64-atom bound of the per-cell graph builder.
 * Returns PAMNET_ENULL for a null pointer; PAMNET_EINVAL for n_mat negative or above 2^31 - 1, a tol that is negative or NaN,
 * or max_sweeps < 1.  n_mat == 0 launches nothing.  (All three: part of ABI 18: nothing existing changed.)
 * ------------------------------------------------------------------------------------------------------------------ */
int pamnet_vib_displace_f32(const float* pos0, const int32_t* gptr, const int32_t* fptr, const int32_t* free_idx, int64_t n,
                            int64_t n_graphs, int64_t pairs, int64_t t, double delta, float* pos_out, pamnet_stream_t stream);
int pamnet_vib_rows_f64(const float* dpos, const float* pos0, const float* masses, const int32_t* fptr, const int32_t* free_idx,
                        const int64_t* moff, int64_t n, int64_t n_graphs, int64_t pairs, int64_t t, double delta, double* h,
                        pamnet_stream_t stream);
int pamnet_sym_eig_f64(double* a, double* v, double* w, int32_t* status, int32_t* sweeps, const int64_t* moff,
                       const int64_t* dptr, int64_t n_mat, double tol, int32_t max_sweeps, pamnet_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Molecular dynamics: one step of every graph of a batch in one launch, and Maxwell-Boltzmann velocities (csrc/md.hip; the
 * reference has no integrator).  Each graph carries its own step counter, status and seed, and optionally its own time step,
 * temperature and friction, so its trajectory does not depend on what else the batch holds.  Units are the caller's.
 *   pos, vel [n, 3] fp32, updated in place;  dpos [n, 3] fp32 = dE/dpos, f = -dpos;  mass [n] fp32 (positive) or NULL: unit
 *   masses;  fixed [n] uint8 or NULL: an atom with fixed[a] != 0 enters no sum and its rows of pos and vel are neither read
 *   nor written;  gptr [n_graphs + 1]: first atom of every graph (kept inside [0, n]).
 *   Per graph: seed [n_graphs] int64;  steps, status [n_graphs] int32 (status 0 = running, 2 = failed; a graph whose status is
 *   not 0 is left alone);  ke [n_graphs] fp64 (output).  dt_g, kT_g, gamma_g [n_graphs] fp64 or NULL: NULL means the scalar
 *   dt / kT / gamma holds for every graph (as fmax_tol_g / fmax_tol above); the scalar beside a given array is not looked at.
 *   Values inside the arrays are the caller's to keep sensible: dt > 0, kT >= 0; a graph whose gamma is not > 0 has no thermostat.
 *
 * THE GENERATOR, shared by both entry points: Philox4x32-10 (Salmon et al., SC 2011; multipliers 0xD2511F53, 0xCD9E8D57, key
 * increments 0x9E3779B9, 0xBB67AE85).  Key = (low 32 bits, high 32 bits) of seed[g].  Counter = (i, step, stream, 0): i the atom's
 * offset inside its graph (a - gptr[g], fixed atoms counted), step the graph's step counter, stream 0 for the thermostat and 1
 * for the initial velocities.  From the four outputs x0 .. x3: u_j = (x_j + 0.5) 2^-32 in fp64, r0 = sqrt(-2 ln u0),
 * r1 = sqrt(-2 ln u2), and the atom's three normals are xi = (r0 cos 2 pi u1, r0 sin 2 pi u1, r1 cos 2 pi u3).  Nothing else feeds the
 * noise: it depends on the graph's seed, its step count and the atom's offset only.
 *
 * pamnet_md_step_f32: BAOAB (Leimkuhler & Matthews, J. Chem. Phys. 138, 174102, 2013) with one force evaluation per step; the
 * closing half kick of step n - 1 is fused into the launch of step n.  Per graph g, the sums over its free atoms:
 *   1. status[g] != 0: nothing that belongs to g is read-modified or written.
 *   2. v_n = v + kick_in (dt / 2) f / m: the velocities that belong to pos.
 *   3. F2 = sum |f|^2, KE = 1/2 sum m |v_n|^2; ke[g] = KE.  F2 or KE not finite: status[g] = 2, nothing else of g is written.
 *   4. advance == 0: vel <- fp32(v_n); steps[g] stays.  Done.
 *   5. v1 = v_n + (dt / 2) f / m.  gamma > 0: v2 = c1 v1 + c2 sqrt(kT / m) xi with c1 = exp(-gamma dt), c2 = sqrt(1 - c1^2) and
 *      xi from (seed[g], steps[g], stream 0, i).  Else v2 = v1 and neither seed nor generator is touched: velocity Verlet,
 *      exactly.  pos <- fp32(pos + (dt / 2) (v1 + v2)); vel <- fp32(v2).
 *   6. steps[g] += 1.
 * A trajectory is: (kick_in 0, advance 1) after the first evaluation, (1, 1) after every later one, and (1, 0) after the
 * evaluation at the last positions, which leaves vel and ke[g] belonging to pos.  Two passes: the sums, then the stores.
 *
 * pamnet_md_init_velocities_f32: per graph g, over its free atoms (rows of fixed atoms are not written):
 *   1. v = sqrt(kT / m) xi(seed[g], step 0, stream 1, i).
 *   2. remove_com: v -= sum m v / sum m.
 *   3. rescale: dof = 3 n_free - 3 remove_com; if dof > 0 and KE = 1/2 sum m |v|^2 > 0: v *= sqrt(dof kT / (2 KE)).
 *   4. vel <- fp32(v); ke[g] = the kinetic energy of v, in fp64 before that rounding.
 * Three passes (momentum, kinetic energy, stores); the normals are regenerated in each.
 *
 * Both: arithmetic in fp64 from the fp32 inputs, one rounding to fp32 at each store of pos and vel.  Sums in a fixed order (a
 * thread's atoms ascending, wavefront butterfly, the wavefronts in order through LDS), no atomics: the outputs of a graph are
 * bitwise repeatable and bitwise the same whether it is handled alone or inside any batch.  One workgroup per graph.
 * Returns PAMNET_EINVAL for a negative count, n_graphs above 2^31 - 1, a flag (kick_in, advance, remove_com, rescale) other
 * than 0 / 1, and, where the per-graph array is NULL, a scalar dt that is not positive and finite or a scalar kT / gamma that is
 * negative or not finite; PAMNET_ENULL for a null required pointer: mass, fixed, dt_g, kT_g and gamma_g may be NULL, and the
 * step's seed where gamma_g is NULL and gamma == 0.  n_graphs == 0 launches nothing.  (Part of ABI 18: nothing existing changed.)
 * ------------------------------------------------------------------------------------------------------------------ */
int pamnet_md_step_f32(float* pos, float* vel, const float* dpos, const float* mass, const uint8_t* fixed, const int32_t* gptr,
                       int64_t n, int64_t n_graphs, const int64_t* seed, int32_t* steps, int32_t* status, double* ke,
                       const double* dt_g, const double* kT_g, const double* gamma_g, double dt, double kT, double gamma,
                       int32_t kick_in, int32_t advance, pamnet_stream_t stream);
int pamnet_md_init_velocities_f32(float* vel, const float* mass, const uint8_t* fixed, const int32_t* gptr, int64_t n,
                                  int64_t n_graphs, const int64_t* seed, const double* kT_g, double kT, int32_t remove_com,
                                  int32_t rescale, double* ke, pamnet_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Constant-pressure molecular dynamics (isotropic NPT): the BAOAB step above with the stochastic cell rescaling barostat
 * (Bernetti & Bussi, J. Chem. Phys. 153, 114107, 2020; GROMACS's c-rescale) fused into the same launch (csrc/md_npt.hip; the
 * reference has no integrator).  The barostat is first order and carries no cell velocity: its state per graph is one fp64
 * number, eps = ln(V / V0), V0 = |det cell0|.  It samples the isothermal-isobaric ensemble to first order in dt; with kT = 0 it
 * is a deterministic Berendsen-like relaxation towards the target pressure.
 * Conventions are those of pamnet_fire_cell_step_f32: row vectors, pos -> pos (I + e), cell -> cell (I + e), and the virial
 * W = dE/de at zero strain.  Arguments beyond those of pamnet_md_step_f32:
 *   dstrain [n_graphs, 9] fp32: W;  cell0 [n_graphs, 9] fp32, read only;  cell [n_graphs, 9] fp32, written: the cell of the new
 *   geometry;  eps [n_graphs] fp64: state (the caller starts with 0);  cell_dof [n_graphs] uint8 or NULL: 0 = the graph has no
 *   barostat, NULL = every graph has one;  pint, vol [n_graphs] fp64 (outputs beside ke);  pressure_g, rate_g [n_graphs] fp64
 *   or NULL: NULL means the scalar pressure P0 / rate holds for every graph (the scalar beside a given array is not looked
 *   at).  rate = beta_T / tau_p, the isothermal compressibility over the coupling time, positive (in an array: the caller's
 *   to keep so).  Units are the caller's: pressure in energy / length^3.
 * The step of graph g with cell_dof[g] != 0; "free" = the atoms of g that are not fixed, f = -dpos:
 *   1. status[g] != 0: nothing that belongs to g is read-modified or written.
 *   2. v_n = v + kick_in (dt / 2) f / m.
 *   3. F2 = sum |f|^2 and KE = 1/2 sum m |v_n|^2 over the free atoms, in the fixed order of pamnet_md_step_f32;
 *      trW = (W00 + W11) + W22;  V = |det cell0[g]| exp(eps[g]);  P_int = (2 KE - trW) / (3 V).
 *      ke[g] = KE, pint[g] = P_int, vol[g] = V: they belong to pos, also when advance == 0.
 *      F2, KE, trW or V not finite, or V == 0: status[g] = 2, nothing else of g is written.
 *   4. d = -rate (P0 - P_int) dt + sqrt(2 kT rate dt / V) xi_c, the change of eps.  xi_c is the first normal of THE GENERATOR
 *      above at counter (0, steps[g], 2, 0) under the graph's key: stream 2 is the barostat's (0: the thermostat, 1: the
 *      initial velocities).  Where kT == 0 the noise term is exactly 0 and the generator is not run.  d is formed from the sums
 *      of step 3 alone, before any store.  d not finite: status[g] = 2, nothing else of g is written.
 *      advance == 0: vel <- fp32(v_n); eps, cell, pos and steps[g] stay.  Done.
 *   5. v1, v2 and the thermostat noise exactly as step 5 of pamnet_md_step_f32.  With s = exp(d / 3):
 *      a free atom:  pos <- fp32(s (pos + (dt / 2) (v1 + v2))),  vel <- fp32(v2 / s);
 *      a fixed atom: pos <- fp32(s pos): it keeps its fractional coordinates, as under pamnet_fire_cell_step_f32; its row of vel
 *      is neither read nor written.
 *      eps[g] += d;  cell[g] = fp32(cell0[g] exp(eps_new / 3)), always from cell0: the cell accumulates no fp32 rounding.
 *   6. steps[g] += 1.
 * The pressure of step n (at x_n, v_n) scales the geometry that step n produces, so the next evaluation sees positions and a
 * cell that belong together and forces are never used on a geometry they were not computed for.  The drift of eps has no
 * kT / V term: in eps = ln V the diffusion coefficient is kT beta_T / (V tau_p), and its eps-derivative cancels against the
 * Jacobian V of the eps-measure.
 * A graph with cell_dof[g] == 0 takes the rule of pamnet_md_step_f32 exactly: its pos, vel, ke, steps and status are bitwise
 * what that entry point gives; its eps, cell, pint and vol are not written; its dstrain, cell0, pressure and rate are not read.
 * Arithmetic, order of the sums and form as pamnet_md_step_f32; the determinant, d and s are formed by every thread of the
 * graph's workgroup alike.  No atomics: the outputs of a graph are bitwise repeatable and the same alone or inside any batch.
 * Returns PAMNET_EINVAL as pamnet_md_step_f32, and, where the per-graph array is NULL, for a scalar pressure that is not finite
 * or a scalar rate that is not positive and finite; PAMNET_ENULL for a null required pointer: mass, fixed, cell_dof and the
 * five _g arrays may be NULL, and seed only where neither thermostat nor barostat noise can occur (gamma_g and kT_g NULL,
 * gamma == 0 and kT == 0).  n_graphs == 0 launches nothing.  (Part of ABI 18: nothing existing changed.)
 * ------------------------------------------------------------------------------------------------------------------ */
int pamnet_md_npt_step_f32(float* pos, float* vel, const float* dpos, const float* dstrain, const float* mass,
                           const uint8_t* fixed, const int32_t* gptr, int64_t n, int64_t n_graphs, const float* cell0,
                           float* cell, double* eps, const uint8_t* cell_dof, const int64_t* seed, int32_t* steps,
                           int32_t* status, double* ke, double* pint, double* vol, const double* dt_g, const double* kT_g,
                           const double* gamma_g, const double* pressure_g, const double* rate_g, double dt, double kT,
                           double gamma, double pressure, double rate, int32_t kick_in, int32_t advance,
                           pamnet_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Constrained molecular dynamics: the BAOAB step of pamnet_md_step_f32 under distance constraints |x_i - x_j| = d -- g-BAOAB
 * (Leimkuhler & Matthews, Proc. R. Soc. A 472, 20160138, 2016) with one geodesic sub-step per half drift, SHAKE for the
 * positions and RATTLE for the velocities (csrc/md_constraints.hip; the reference has no integrator).
 * Arguments beyond those of pamnet_md_step_f32:
 *   cons_i, cons_j [n_cons] int32: the two atom rows of a constraint, both inside one graph;  cons_d [n_cons] fp64: its length;
 *   gcol [n_graphs + 1] int32, colptr [K + 1] int32: a two-level CSR -- graph g owns the colours gcol[g] .. gcol[g + 1], colour
 *   k the constraints colptr[k] .. colptr[k + 1].  The constraints are sorted by (graph, colour), and no two constraints of a
 *   colour share an atom (the caller colours them; pamnet_amd.md.Constraints does).  work [9 n] fp64: workspace (x0, x, v).
 *   sweeps [n_graphs] int32, output: the most sweeps any solve of this launch took for the graph (0 without constraints).
 *   tol: the convergence bound of both solves;  max_sweeps: the sweeps a solve may take.
 * With w_a = 0 for a fixed atom and 1 / m_a otherwise, and a fixed atom's velocity taken as 0:
 *   RATTLE_V:  a sweep visits the constraints in the order (colour, position): r = x_i - x_j, u = v_i - v_j,
 *     err = |r.u| dt / d^2, kappa = r.u / ((w_i + w_j) r.r), v_i -= w_i kappa r, v_j += w_j kappa r.  The solve has converged
 *     after the first sweep in which every err, measured as the sweep reaches the constraint, is <= tol.
 *   SHAKE (x0: the positions before the drift):  s = x_i - x_j, r0 = x0_i - x0_j, err = |s.s - d^2| / (2 d^2),
 *     g = (s.s - d^2) / (2 (w_i + w_j) (s.r0)), x_i -= w_i g r0, x_j += w_j g r0; converged as above.
 *   A solve is broken by an err that is not finite, by s.r0 <= 0 and by a row outside the graph, and has failed after
 *   max_sweeps sweeps without convergence.  A constraint with w_i + w_j == 0 is measured but not corrected.
 * The step of a graph g with constraints, f = -dpos, sums over its free atoms in the order of pamnet_md_step_f32:
 *   1. status[g] != 0: nothing that belongs to g is read-modified or written.
 *   2. v = v + kick_in (dt / 2) f / m;  F2 = sum |f|^2, KE = 1/2 sum m |v|^2.  Either not finite: ke[g] = KE, status[g] = 2,
 *      nothing else of g changes (sweeps[g] = 0).
 *   3. kick_in: RATTLE_V, and KE = 1/2 sum m |v|^2 again.  ke[g] = KE (not finite: status[g] = 2).
 *   4. advance == 0: vel <- fp32(v) if kick_in; done.
 *   5. v += (dt / 2) f / m, RATTLE_V;   x0 = x, x += (dt / 2) v, SHAKE, v = (x - x0) / (dt / 2), RATTLE_V;
 *      gamma > 0: v = c1 v + c2 sqrt(kT / m) xi with c1, c2 and xi exactly those of pamnet_md_step_f32, RATTLE_V;
 *      the half drift with SHAKE and RATTLE_V once more.
 *   6. pos <- fp32(x), vel <- fp32(v) for the free atoms; steps[g] += 1.
 *   Any solve that fails: status[g] = 3, sweeps[g] is written, and pos, vel and steps of g stay bit for bit (ke[g] may hold
 *   the KE of step 3).  Positions are never wrapped: differences are plain, a constrained pair sits in one image.
 * A graph without constraints takes the rule of pamnet_md_step_f32 exactly: its pos, vel, ke, steps and status are bitwise
 * what that entry point gives.  One workgroup per graph, every loop count uniform over it, fp64, fixed order, no atomics: the
 * outputs of a graph are bitwise repeatable and the same alone or inside any batch.
 *
 * pamnet_md_project_constraints_f32: per graph g with status[g] == 0 and constraints, x = pos, v = vel (0 for a fixed atom):
 *   do_pos: SHAKE with x0 = x (r0 is the current difference);  do_vel: RATTLE_V at the projected x with the graph's dt.
 *   Then pos <- fp32(x) (do_pos) and vel <- fp32(v), ke[g] = 1/2 sum m |v|^2 (do_vel) for the free atoms; sweeps[g] as above.
 *   A solve that fails: status[g] = 3, pos and vel stay.  A graph without constraints: ke[g] of vel as it stands (do_vel).
 *
 * Both return PAMNET_EINVAL as pamnet_md_step_f32 (the projection: dt only where do_vel), and for n_cons < 0, a tol that is
 * not positive and finite, max_sweeps < 1 and a flag other than 0 / 1; PAMNET_ENULL for a null required pointer: sweeps always,
 * cons_i, cons_j, cons_d, gcol, colptr and work where n_cons > 0 (with n_cons == 0 no graph has constraints and none of them
 * is read); the projection needs vel and ke only where do_vel.  Rows inside cons_i / cons_j are the caller's to keep inside
 * their graph.  (Part of ABI 18: nothing existing changed.)
 * ------------------------------------------------------------------------------------------------------------------ */
int pamnet_md_constrained_step_f32(float* pos, float* vel, const float* dpos, const float* mass, const uint8_t* fixed,
                                   const int32_t* gptr, int64_t n, int64_t n_graphs, const int64_t* seed, int32_t* steps,
                                   int32_t* status, double* ke, const double* dt_g, const double* kT_g, const double* gamma_g,
                                   double dt, double kT, double gamma, int32_t kick_in, int32_t advance, const int32_t* cons_i,
                                   const int32_t* cons_j, const double* cons_d, const int32_t* gcol, const int32_t* colptr,
                                   int64_t n_cons, double* work, int32_t* sweeps, double tol, int32_t max_sweeps,
                                   pamnet_stream_t stream);
int pamnet_md_project_constraints_f32(float* pos, float* vel, const float* mass, const uint8_t* fixed, const int32_t* gptr,
                                      int64_t n, int64_t n_graphs, int32_t* status, double* ke, const double* dt_g, double dt,
                                      const int32_t* cons_i, const int32_t* cons_j, const double* cons_d, const int32_t* gcol,
                                      const int32_t* colptr, int64_t n_cons, double* work, int32_t* sweeps, double tol,
                                      int32_t max_sweeps, int32_t do_pos, int32_t do_vel, pamnet_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Replica-exchange molecular dynamics (parallel tempering; Sugita & Okamoto, Chem. Phys. Lett. 314, 141, 1999): one exchange
 * attempt of every temperature ladder of a batch in one launch (csrc/remd.hip; the reference has no integrator).  A ladder is a
 * run of consecutive graphs that hold the same atoms, one graph per temperature.  An exchange swaps the TEMPERATURES two graphs
 * hold, not their configurations: no position, graph or neighbour structure moves; kT_g -- the array pamnet_md_step_f32 reads --
 * the two rung tables and a scale of the velocities change.
 *   energy [n_graphs] fp64, read only: the potential energy of every graph at its current positions;
 *   vel [n, 3] fp32, in place;  fixed [n] uint8 or NULL;  gptr [n_graphs + 1] int32: as for pamnet_md_step_f32;
 *   lptr [n_ladders + 1] int32: ladder l is the graphs lptr[l] .. lptr[l + 1] - 1 (kept inside [0, n_graphs]); it starts at 0,
 *   does not decrease and ends at n_graphs.  A ladder of one graph (or of none) is legal and never exchanges;
 *   kT_ladder [n_graphs] fp64, read only: entry lptr[l] + r is the temperature of rung r of ladder l (positive);
 *   kT_g [n_graphs] fp64, in place: entry g is the temperature graph g holds;
 *   rung [n_graphs] int32, in place: the rung graph g holds;  slot [n_graphs] int32, in place: entry lptr[l] + r is the graph
 *   that holds rung r of ladder l -- the inverse of rung (slot[lptr[l] + rung[g]] == g);
 *   status [n_graphs] int32, read only: the status of the step launch;  ke [n_graphs] fp64, in place;
 *   seed [n_ladders] int64;  attempts [n_ladders] int32, in place: the exchange launches the ladder has seen;
 *   tried, accepted [n_graphs] int32, in place: entry lptr[l] + r counts the pair (r, r + 1); the last entry of a ladder is
 *   never written.
 * The rule of ladder l, with lo = lptr[l], R its number of rungs, a = attempts[l] and parity p = a & 1:
 *   1. For every r with r = p (mod 2) and r + 1 < R: i = slot[lo + r], j = slot[lo + r + 1].  status[i] != 0, status[j] != 0, or
 *      energy[i] or energy[j] not finite: the pair is skipped -- not counted in tried, nothing of it is written.
 *   2. D = (1 / kT_r - 1 / kT_{r+1}) (E_i - E_j) with kT from kT_ladder;  tried[lo + r] += 1.  Accept if D >= 0, or if
 *      u < exp(D) with u = (x0 + 0.5) 2^-32 in fp64, x0 the first output of THE GENERATOR of the molecular-dynamics section
 *      (Philox4x32-10) under the key (low 32 bits, high 32 bits) of seed[l] at the counter (r, a, 3, 0): stream 3 is the
 *      exchange's (0: the thermostat, 1: the initial velocities, 2: the barostat).  Nothing else feeds the decision: it depends
 *      on the ladder's seed, its attempt count, the rung and the two energies only.
 *   3. On acceptance: slot[lo + r] = j, slot[lo + r + 1] = i;  rung[i] = r + 1, rung[j] = r;  kT_g[i] = kT_{r+1}, kT_g[j] = kT_r;
 *      accepted[lo + r] += 1;  the velocities of the free atoms of i are multiplied by sqrt(kT_{r+1} / kT_r), those of j by
 *      sqrt(kT_r / kT_{r+1}) -- fp64 arithmetic on the fp32 value, one rounding at the store; rows of fixed atoms are neither
 *      read nor written --;  ke[i] *= kT_{r+1} / kT_r, ke[j] *= kT_r / kT_{r+1}.
 *   4. attempts[l] += 1, also where no pair was tried.
 * With the canonical weights exp(-E / kT) the acceptance min(1, exp(D)) keeps every rung's ensemble; the scale hands each
 * graph velocities at its new temperature.  It is uniform over a graph, so velocities that satisfy distance constraints still do.
 * The decision needs the ensemble of a thermostat at kT_g: call it between a closing step launch (kick_in 1, advance 0), which
 * leaves vel and ke belonging to pos, and an opening one (kick_in 0, advance 1) on the same forces.
 * One workgroup per ladder: one thread per pair decides, LDS carries (graph, scale) per rung behind a barrier, then the whole
 * workgroup strides over the atoms of the graphs whose temperature changed.  No atomics and no floating-point sums: a ladder
 * reads and writes its own entries only, so its outputs are bitwise repeatable and the same alone or inside any batch.
 * A ladder has at most 256 rungs.
 * Returns PAMNET_EINVAL for a negative count, n_graphs or n_ladders above 2^31 - 1, and n_graphs > 256 n_ladders (some ladder
 * would have more than 256 rungs); PAMNET_ENULL for a null pointer: only fixed may be NULL.  n_ladders == 0 launches nothing.
 * lptr lives on the device and the entry point does not read it: that it starts at 0, does not decrease, ends at n_graphs and
 * holds no ladder above 256 rungs is the caller's to check (pamnet_amd.remd does, on the host); the kernel keeps every ladder
 * inside [0, n_graphs], leaves a ladder of more than 256 rungs wholly alone (attempts included) and skips a pair whose slot
 * entries do not name two graphs of its ladder.  (Part of ABI 18: nothing existing changed.)
 * ------------------------------------------------------------------------------------------------------------------ */
int pamnet_remd_exchange_f64(const double* energy, float* vel, const uint8_t* fixed, const int32_t* gptr, const int32_t* lptr,
                             const double* kT_ladder, double* kT_g, int32_t* rung, int32_t* slot, const int32_t* status,
                             double* ke, const int64_t* seed, int32_t* attempts, int32_t* tried, int32_t* accepted, int64_t n,
                             int64_t n_graphs, int64_t n_ladders, pamnet_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Biased dynamics over collective variables: harmonic restraints (umbrella windows, walls) and well-tempered metadynamics
 * (Barducci, Bussi & Parrinello, Phys. Rev. Lett. 100, 020603, 2008) with multiple walkers (Raiteri et al., J. Phys. Chem. B
 * 110, 3533, 2006); csrc/bias.hip, the reference has no integrator.  pamnet_bias_apply_f64 is one launch per step, between
 * the model evaluation and pamnet_md_step_f32 / pamnet_md_constrained_step_f32: it adds the gradient of the bias to dpos.
 * A bias GROUP is a run of consecutive graphs that share one hill table: one graph is an ordinary simulation, W graphs are W
 * walkers on one table.
 *   pos [n, 3] fp32, read only;  dpos [n, 3] fp32, in place;  status [n_graphs] int32, in place: the status of the step launch;
 *   gptr [n_graphs + 1] int32: as for pamnet_md_step_f32;
 *   bptr [n_groups + 1] int32: group t is the graphs bptr[t] .. bptr[t + 1] - 1 (kept inside [0, n_graphs]), as lptr of
 *   pamnet_remd_exchange_f64;
 *   cvptr [n_graphs + 1] int32: graph g owns the collective variables (CVs) cvptr[g] .. cvptr[g + 1] - 1, at most 16;
 *   kind [n_cvs] int32: 0 distance (2 atoms), 1 angle (3 atoms, radians, at the middle atom), 2 dihedral (4 atoms);
 *   atoms [n_cvs, 4] int32: atom rows, all inside the graph of the CV; the entries beyond the kind's count are not read;
 *   kappa, centre, halfwidth [n_cvs] fp64: the restraint of every CV;
 *   ndim [n_groups] int32 in {0, 1, 2}: the first ndim CVs of every graph of the group carry the hills;
 *   sigma [n_groups, 2] fp64 (positive where used), height0 [n_groups] fp64, inv_dT [n_groups] fp64: 1 / (kT (gamma - 1)) of
 *   the bias factor gamma, 0 for plain metadynamics;
 *   hill_c [n_groups, h_cap, 2] fp64, hill_w [n_groups, h_cap] fp64, n_hills [n_groups] int32, dropped [n_groups] int32: the
 *   hill tables, in place;  deposit: 0 or 1;
 *   cv [n_cvs] fp64, ebias [n_graphs] fp64: written.
 * The CVs, in fp64 from the fp32 positions as they are (never wrapped: the atoms of a CV must sit in one image):
 *   distance  d = |x_j - x_i|;  dd/dx_j = (x_j - x_i) / d = -dd/dx_i;
 *   angle     theta = atan2(|a x b|, a . b), a = x_i - x_j, b = x_k - x_j, nn = a x b;
 *             dtheta/dx_i = a x nn / (|a|^2 |nn|), dtheta/dx_k = nn x b / (|b|^2 |nn|), dtheta/dx_j = -(the two);
 *   dihedral  phi = atan2(|b2| b1 . (b2 x b3), (b1 x b2) . (b2 x b3)), b1 = x_j - x_i, b2 = x_k - x_j, b3 = x_l - x_k; with
 *             m = b1 x b2, nn = b2 x b3 (Blondel & Karplus, J. Comput. Chem. 17, 1132, 1996):
 *             dphi/dx_i = -|b2| m / |m|^2, dphi/dx_l = |b2| nn / |nn|^2,
 *             dphi/dx_j = (|b2| / |m|^2 + p) m + q nn, dphi/dx_k = -p m - (q + |b2| / |nn|^2) nn,
 *             p = b1 . b2 / (|m|^2 |b2|), q = b3 . b2 / (|nn|^2 |b2|).
 *   A dihedral is periodic: every difference s - c it enters (hill and restraint) is d - 2 pi rint(d / (2 pi)).
 * The rule of graph g of group t, with n0 = n_hills[t] read once at the start of the launch (kept inside [0, h_cap]):
 *   1. status[g] != 0 (or more than 16 CVs): the graph is skipped -- its dpos rows stay bitwise, its cv entries and ebias[g]
 *      are NaN, it deposits nothing.
 *   2. Every CV s_k and its gradient are formed.  If one of these numbers is not finite (collinear atoms of an angle or a
 *      dihedral, coincident atoms, a non-finite position), the kind is unknown or an atom lies outside the graph:
 *      status[g] = 2, dpos stays untouched, cv and ebias[g] are NaN, nothing is deposited.
 *   3. V = sum_{h < n0} w_h exp(-1/2 sum_{d < ndim} u_hd^2), u_hd = (s_d - c_hd) / sigma_d;  dV/ds_d = -sum_h e_h u_hd /
 *      sigma_d.  The order of the sum is fixed: thread q of 256 adds the hills q, q + 256, ... in that order; the 64 lanes of a
 *      wavefront are added by the butterfly v += v[lane ^ o], o = 32, 16, ..., 1; the four wavefront sums are added in order.
 *   4. Restraint of CV k where kappa_k != 0: a = |s_k - centre_k| - halfwidth_k; where a > 0, E_k = 1/2 kappa_k a^2 and
 *      dE_k/ds_k = kappa_k a sign(s_k - centre_k).  halfwidth 0: an umbrella window; > 0: a pair of walls.
 *   5. ebias[g] = V + sum_k E_k in the order of k;  c_k = (k < ndim ? dV/ds_k : 0) + dE_k/ds_k.
 *   6. For k in order, where c_k != 0, for the atoms of the CV in order, per component:
 *      dpos = (float)((double)dpos + c_k ds_k/dx) -- one thread, one rounding per addition: atoms that two CVs share (phi / psi)
 *      are handled by this order, not by atomics.
 *   7. deposit == 1, ndim > 0, after every graph of the group: the graphs that passed 2, in graph order, append the centre
 *      (s_0, s_1) (s_1 = 0 where ndim is 1) and the height height0 exp(-V inv_dT), with the V of step 3 -- against the n0 old
 *      hills, so the walkers of one launch do not see each other -- at n_hills[t], which rises by one each.  Where the table is
 *      full nothing is written and dropped[t] counts it.
 * One workgroup of 256 threads per group takes its walkers one after another; every loop count is read by all threads alike.
 * No atomics: a group reads and writes its own entries only, so its outputs are bitwise repeatable and the same alone or
 * inside any batch.  A group has at most 256 graphs.
 * Returns PAMNET_EINVAL for a negative count, a count above 2^31 - 1, deposit outside {0, 1}, n_graphs > 256 n_groups and
 * n_cvs > 16 n_graphs; PAMNET_ENULL for a null pointer (none may be NULL).  n_groups == 0 launches nothing.  bptr and cvptr
 * live on the device and are not read by the entry point: the kernel leaves a group of more than 256 graphs wholly alone.
 *
 * pamnet_bias_grid_f64: out[i] = V of table `table` at points[i, 0 .. ndim) (fp64 [n_points, ndim], ndim 1 or 2), summed over
 * the hills [0, n_hills[table]) in hill order by one thread per point; periodic [n_groups, 2] int32 says which dimensions wrap.
 * It serves the free-energy estimate.  PAMNET_EINVAL for a negative count, table outside [0, n_groups), ndim outside {1, 2};
 * PAMNET_ENULL for a null pointer; n_points == 0 launches nothing.  (Both are part of ABI 18: nothing existing changed.)
 * ------------------------------------------------------------------------------------------------------------------ */
int pamnet_bias_apply_f64(const float* pos, float* dpos, int32_t* status, const int32_t* gptr, const int32_t* bptr,
                          const int32_t* cvptr, const int32_t* kind, const int32_t* atoms, const double* kappa,
                          const double* centre, const double* halfwidth, const int32_t* ndim, const double* sigma,
                          const double* height0, const double* inv_dT, double* hill_c, double* hill_w, int32_t* n_hills,
                          int32_t* dropped, double* cv, double* ebias, int64_t n, int64_t n_graphs, int64_t n_groups,
                          int64_t n_cvs, int64_t h_cap, int32_t deposit, pamnet_stream_t stream);
int pamnet_bias_grid_f64(const double* hill_c, const double* hill_w, const int32_t* n_hills, const double* sigma,
                         const int32_t* periodic, const double* points, double* out, int64_t table, int64_t n_groups,
                         int64_t h_cap, int64_t n_points, int32_t ndim, pamnet_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Attention fusion + per-graph pooling  (models.py:206-224)
 * outs/atts: [2L, n] rows ordered (global_0, local_0, global_1, local_1, ...).
 *   node_out[n] = sign[n] * sum_l sum_c outs[l,c,n] * softmax_c(leaky_relu(atts[l,c,n], 0.2))
 *   graph_out[b] = (mean ? 1/|b| : 1) * sum_{n in b} node_out[n];  sign may be NULL (=1).
 * A graph without nodes gets 0 (sum and mean).  n == 0 with n_graphs > 0 is valid: graph_out[0 .. n_graphs) is written as
 * zeros and no other pointer is read; the backward with n == 0 writes nothing.
 * ------------------------------------------------------------------------------------------------------------------ */
int pamnet_fuse_pool_fwd_f32(const float* outs, const float* atts, int64_t n_layer, int64_t n, const float* sign,
                             const int32_t* gptr, int64_t n_graphs, int32_t mean, float* node_out, float* graph_out,
                             pamnet_stream_t stream);
int pamnet_fuse_pool_bwd_f32(const float* outs, const float* atts, int64_t n_layer, int64_t n, const float* sign,
                             const int32_t* node_graph, const int32_t* gptr, int32_t mean, const float* grad_graph,
                             float* grad_outs, float* grad_atts, pamnet_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Fused dense chains (dim = 128 only), fp32 MFMA.  Weight pointers are HOST arrays of DEVICE pointers to row-major
 * [out=128][in] blocks (the layout of an nn.Linear weight; row stride 128 unless an ld is given).
 *
 * node_tail: the 10-Linear update stack + heads shared by both layer kinds
 *   (layers/global_message_passing.py:39-50, layers/local_message_passing.py:55-66; Res: layers/basic.py:25-33):
 *   weights/biases order: mlp_x2, res1.0, res1.1, res2.0, res2.1, res3.0, res3.1, mlp_out.0, mlp_out.1, mlp_out.2.
 *   Saves Z[10][n][128] (pre-activations) and R[2][n][128] (r1, r2) for the backward.
 *   next_* (next_nblk = 0: none): the node_pre of the FOLLOWING layer applied to x_out while its tile is still on chip
 *   (same outputs as pamnet_node_pre_fwd_f32 on x_out) -- the layer loop then needs one node-level launch per layer.
 * node_pre: x1 = SiLU(mlp_x1 x) and the node-level halves P = x1 * Wp_b^T (b < nblk <= 4) of the split message MLPs
 *   (mlp_m / mlp_m_ji / mlp_m_kj on [x_i | x_j | e]: layers/global_message_passing.py:52-56, local...:46-48).
 * wgrad_batched: dW_j = dZ_j^T * A_j (A_j optionally SiLU'd on load), db_j = colsum(dZ_j) for up to 24 jobs, in two
 *   launches (split-K partial tiles, then one fixed-order reduction).  The reduction launch can also finish a node_tail
 *   backward: pass that call's head_partial / workgroup count (= ceil(n/16)) and the three head-gradient outputs here and
 *   give node_tail_bwd null d_wout/d_watt/d_bout (then it launches no reduction of its own).
 * ------------------------------------------------------------------------------------------------------------------ */
int pamnet_node_tail_fwd_f32(const float* x2, const float* res_x, int64_t n, const float* const* weights,
                             const float* const* biases, const float* w_out, const float* b_out, const float* w_att,
                             float* Z, float* R, float* x_out, float* out, float* att, const float* next_Wx1,
                             const float* next_bx1, const float* const* next_wp, int64_t next_ldwp, int64_t next_nblk,
                             float* next_Zx1, float* next_x1, float* next_P, int32_t packed, pamnet_stream_t stream);
/* pamnet_node_tail_fwd_f32 (packed weight images, deferred heads) with a RIDER: row tiles [mlp_tile0, mlp_tile0 + mlp_ntiles)
 * (16 rows each) of the two-layer MLP of pamnet_mlp2_fwd_f32 over mlp_x [mlp_rows,128] run as `rider_wgs` extra workgroups
 * of the launch -- the chain occupies only ceil(n/16) of the 256 CUs, the triplet/pair MLPs of the next layers do not
 * depend on the node features.  mlp = {W1, b1, W2, b2}; mlp_out = {z1, z2, y} (z1 / z2 nullable saves). */
int pamnet_node_tail_fwd_rider_f32(const float* x2, const float* res_x, int64_t n, const float* const* weights,
                                   const float* const* biases, const float* w_out, const float* b_out,
                                   const float* w_att, float* Z, float* R, float* x_out, const float* next_Wx1,
                                   const float* next_bx1, const float* const* next_wp, int64_t next_ldwp,
                                   int64_t next_nblk, float* next_Zx1, float* next_x1, float* next_P, const float* mlp_x,
                                   int64_t mlp_rows, int64_t mlp_tile0, int64_t mlp_ntiles, const float* const* mlp,
                                   float* const* mlp_out, int64_t rider_wgs, int32_t packed /* 1 or 2 */,
                                   pamnet_stream_t stream);
/* out = att = null in pamnet_node_tail_fwd_f32 leaves the head branch of the chain (mlp_out, W_out, W:
 * layers/global_message_passing.py:46-50) to this call, which runs it for n_layers chains in one launch (nothing
 * downstream of a layer depends on its heads): per layer l  x_out[l] [n,128] -> out[l] [n], att[l] [n], and slots 7..9
 * of that layer's pre-activation block Z[l] ([10][n][128]; Z or Z[l] null: not saved).  weights / biases: 3 per layer
 * (mlp_out), fragment images when `packed`. */
int pamnet_node_heads_fwd_f32(int64_t n_layers, const float* const* x_out, const float* const* weights,
                              const float* const* biases, const float* const* w_out, const float* const* b_out,
                              const float* const* w_att, float* const* Z, float* const* out, float* const* att, int64_t n,
                              int32_t packed, pamnet_stream_t stream);
int pamnet_node_tail_bwd_f32(const float* d_xout, const float* d_out, const float* d_att, int64_t n,
                             const float* const* weights, const float* w_out, const float* w_att, const float* Z,
                             float* dZ, float* d_x2, float* d_resx, float* head_partial, float* d_wout, float* d_watt,
                             float* d_bout, int32_t packed, pamnet_stream_t stream);
/* Backward counterparts of the deferred head branch.  heads_bwd (all layers, one launch; needs only d out / d att):
 * per layer l the head-vector partials (head_partial[l]: ceil(n/16) x 257 floats, reduced by pamnet_wgrad_batched_f32),
 * dZ3[l] = [dz7, dz8, dz9] ([3][n][128]) and g_head[l] = the branch's contribution to d x_out ([n][128]); weights: the
 * mlp_out matrices 7, 8, 9 of every layer (transposed-orientation images when `packed`).  tail_main_bwd: the rest of
 * the chain (layers 6..0) from d x_out = d_xout (may be null) + g_head; writes dZ slots 0..6. */
int pamnet_node_heads_bwd_f32(int64_t n_layers, const float* const* d_out, const float* const* d_att,
                              const float* const* weights, const float* const* w_out, const float* const* w_att,
                              const float* const* Z, float* const* dZ3, float* const* g_head, float* const* head_partial,
                              int64_t n, int32_t packed, pamnet_stream_t stream);
int pamnet_node_tail_main_bwd_f32(const float* d_xout, const float* g_head, int64_t n, const float* const* weights,
                                  const float* Z, float* dZ, float* d_x2, float* d_resx, int32_t packed,
                                  pamnet_stream_t stream);
/* pamnet_node_pre_bwd_f32 (backward of a layer's head: dP [nblk][n][128], d x1_direct, d_add -> dZx1 and d x) fused
 * with pamnet_node_tail_main_bwd_f32 of the chain that produced that layer's input: the head's d x becomes the chain's
 * d x_out on chip.  All weights are transposed-orientation images (pamnet_pack_weights_f32; with nblk | PAMNET_CHAIN_PIECES:
 * bf16x3 images, the chain on the bf16 matrix pipe at fp32 accuracy). */
int pamnet_node_pre_tail_bwd_f32(const float* dP, const float* dx1_direct, const float* d_add, int64_t n,
                                 const float* Wx1, const float* const* wp, int64_t nblk, const float* Zx1, float* dZx1,
                                 const float* g_head, const float* const* weights, const float* Z, float* dZ,
                                 float* d_x2, float* d_resx, const void* rider /* host, nullable */,
                                 pamnet_stream_t stream);
/* The operands of pamnet_local_agg_fwd_f32 as one argument (round 6): pamnet_node_tail_fwd_agg_f32 is
 * pamnet_node_tail_fwd_rider_f32 (mlp_ntiles = 0: without riders) whose chain input x2 is formed by the launch's own row tiles --
 * the two chained aggregations of layers/local_message_passing.py:49-54, bit for bit pamnet_local_agg_fwd_f32's rows -- and
 * written to x2 (and m_t) as well; chain forms that read their input run the aggregation as a launch of its own first. */
typedef struct pamnet_local_agg {
    const float *m_ji, *m_nb, *s, *q3, *init; /* init nullable = 0 */
    const int32_t *t_ptr, *t_col, *l_ptr;
    float* m_t;                               /* nullable: backward-only save */
} pamnet_local_agg;
int pamnet_node_tail_fwd_agg_f32(float* x2, const float* res_x, int64_t n, const float* const* weights,
                                 const float* const* biases, const float* w_out, const float* b_out, const float* w_att,
                                 float* Z, float* R, float* x_out, const float* next_Wx1, const float* next_bx1,
                                 const float* const* next_wp, int64_t next_ldwp, int64_t next_nblk, float* next_Zx1,
                                 float* next_x1, float* next_P, const float* mlp_x, int64_t mlp_rows, int64_t mlp_tile0,
                                 int64_t mlp_ntiles, const float* const* mlp, float* const* mlp_out, int64_t rider_wgs,
                                 int32_t packed, const pamnet_local_agg* agg, pamnet_stream_t stream);
/* The same with planes of dP formed inside the launch (round 6): gather_src[b] != null -> plane b, row i = the sum of
 * gather_src[b][gather_perm[b] ? gather_perm[b][q] : q] over q in [gather_ptr[b][i], gather_ptr[b][i+1]) in that order, used and
 * also written to dP + b n 128 -- the pamnet_segment_sum(_multi)_f32 launches that otherwise run ahead of this one. */
int pamnet_node_pre_tail_bwd_gather_f32(float* dP, const float* const* gather_src, const int32_t* const* gather_ptr,
                                        const int32_t* const* gather_perm, const float* dx1_direct, const float* d_add,
                                        int64_t n, const float* Wx1, const float* const* wp, int64_t nblk, const float* Zx1,
                                        float* dZx1, const float* g_head, const float* const* weights, const float* Z,
                                        float* dZ, float* d_x2, float* d_resx, const void* rider /* host, nullable */,
                                        pamnet_stream_t stream);
/* Fragment-ordered weight images for the node chains: n (<= 192) 128x128 matrices (row stride ld[i]) -> images[i*16384..],
 * transposed = 0 for the forward (Y = X W^T), 1 for the backward (Y = X W).  With packed != 0 the `weights` (and, in the
 * forward, next_Wx1 / next_wp) arguments of node_tail_fwd / node_tail_bwd, and Wx1 / wp of node_pre_bwd (transposed
 * images), are such images: every weight-slice request of
 * a wave is then one contiguous 1 KB read instead of 16 half-used cache lines of the row-major matrix. */
int pamnet_pack_weights_f32(int64_t n, const float* const* W, const int64_t* ld, int32_t transposed, float* images,
                            pamnet_stream_t stream);
/* The same matrices as bf16x3 fragment images (images[i*24576..], 96 KB each): every weight split exactly into three bf16
 * pieces, laid out as operand fragments of v_mfma_f32_16x16x32_bf16 (the kind-1 images of pamnet_pack_weights_mixed_f32 below,
 * one after the other).  With packed == 2, pamnet_node_tail_fwd_f32 (deferred
 * heads: out = att = null) and pamnet_node_tail_fwd_rider_f32 take such images for weights[0..6], next_Wx1 and next_wp and
 * run the chain on the bf16 matrix pipe at fp32 accuracy (six piece products per product: csrc/gemm_core.h "bf16x6"). */
int pamnet_pack_weights_bf16x3(int64_t n, const float* const* W, const int64_t* ld, int32_t transposed, float* images,
                               pamnet_stream_t stream);
/* Round 6 (ABI 14): all weight images of a step direction in one launch, n <= 224.  kind[i] = 0: the chains' fp32 fragment
 * image of pamnet_pack_weights_f32 (16 384 floats); kind[i] = 1: the EDGE-LEVEL kernels' bf16x3 fragment image (24 576 floats):
 * uint4 image[((tile * 4 + q) * 3 + piece) * 64 + lane] = the exact bf16 pieces lane `lane` of the wave that owns output
 * columns [16 tile, 16 tile + 16) holds for k-step q (csrc/edge_core.h load_wfragb1) -- what every workgroup of
 * pamnet_global_edge_agg_fwd_f32 / _fwd_pp_f32 / _bwd_f32 and pamnet_local_edge_fwd_f32 otherwise makes of its slices itself
 * (64-128 loads and ~300 vector instructions per lane ahead of the first row: 2 us of a 30 us launch at the QM9 batch).  Those
 * four entry points take such an image in place of a weight matrix when its row stride argument is 0 (all of a call's strides
 * zero or none; pamnet_local_edge_fwd_f32: 8-wave geometry only); the results are bitwise those of the fp32 matrices.
 * offset[i]: where image i starts in `images`, in floats (a multiple of 4).  transposed as in pamnet_pack_weights_f32
 * (0: Y = X W^T, the forward entries; 1: Y = X W, pamnet_global_edge_agg_bwd_f32). */
int pamnet_pack_weights_mixed_f32(int64_t n, const float* const* W, const int64_t* ld, const int32_t* kind,
                                  const int64_t* offset, int32_t transposed, float* images, pamnet_stream_t stream);
int pamnet_node_pre_fwd_f32(const float* x, int64_t n, const float* Wx1, const float* bx1, const float* const* wp,
                            int64_t ldwp, int64_t nblk, float* Zx1, float* x1, float* P, pamnet_stream_t stream);
int pamnet_node_pre_bwd_f32(const float* dP, const float* dx1_direct, const float* d_add, int64_t n, const float* Wx1,
                            const float* const* wp, int64_t ldwp, int64_t nblk, const float* Zx1, float* dZx1,
                            float* dx, int32_t packed, pamnet_stream_t stream);
int pamnet_wgrad_scratch_floats(int64_t njobs, const int64_t* rows, int64_t* floats);
int pamnet_wgrad_batched_f32(int64_t njobs, const float* const* dZ, const int64_t* ld_dz, const float* const* A,
                             const int64_t* ld_a, const int32_t* a_mode, const int64_t* rows, float* const* dW,
                             const int64_t* ld_dw, float* const* db, float* partial, const float* head_partial,
                             int64_t head_blocks, float* d_wout, float* d_watt, float* d_bout, pamnet_stream_t stream);
/* Deferred form for a sequence of batches (the layers of one backward pass): the fixed-order reduction of batch i runs
 * inside the launch of batch i+1's split-K pass; pamnet_wgrad_flush_f32 reduces the last one.  ctx: caller-owned HOST
 * memory of *bytes (pamnet_wgrad_ctx_bytes) bytes, zeroed before the first call -- the library keeps no state of its
 * own.  Consecutive calls must pass different `partial` buffers. */
int pamnet_wgrad_ctx_bytes(int64_t* bytes /* host */);
int pamnet_wgrad_deferred_f32(int64_t njobs, const float* const* dZ, const int64_t* ld_dz, const float* const* A,
                              const int64_t* ld_a, const int32_t* a_mode, const int64_t* rows, float* const* dW,
                              const int64_t* ld_dw, float* const* db, float* partial, const float* head_partial,
                              int64_t head_blocks, float* d_wout, float* d_watt, float* d_bout,
                              const float* head2_partial /* nullable: a second chain's head-vector partials (same head_blocks):
                                                            a layer pair's merged batch carries the local and the global chain's */,
                              float* d_wout2, float* d_watt2, float* d_bout2, void* ctx /* host */,
                              pamnet_stream_t stream);
int pamnet_wgrad_flush_f32(void* ctx /* host */, pamnet_stream_t stream);
/* Riders: weight-gradient slots as extra workgroups of a node-chain backward launch (the chain owns ceil(n/16) workgroups,
 * 143 of the 256 CUs at the QM9 batch; the riders take the idle CUs and the layer's own weight-gradient launch shrinks).
 *   pamnet_wgrad_rider_plan_f32   : lay a batch (<= 16 jobs) out over njobs <= *slots_out <= max_slots slots (rows per slot: 256,
 *                                   growing in steps of 64 until the batch fits; max_slots < njobs: PAMNET_EINVAL); the plan
 *                                   goes to `rider` (caller-owned HOST memory of pamnet_wgrad_rider_bytes bytes)
 *   pamnet_node_pre_tail_bwd_f32  : takes the plan (`rider` argument) and appends the slots to its grid
 *   pamnet_wgrad_rider_enqueue_f32: registers the batch with a deferred context so that the next pamnet_wgrad_deferred_f32
 *                                   launch (or the flush) reduces its slots in the usual fixed order.  A second rider batch
 *                                   before that launch is appended to the first (<= 24 jobs together); its `partial` must
 *                                   start right behind the first one's slots in the same buffer. */
int pamnet_wgrad_rider_bytes(int64_t* bytes);
int pamnet_wgrad_rider_plan_f32(int64_t njobs, const float* const* dZ, const int64_t* ld_dz, const float* const* A,
                                const int64_t* ld_a, const int32_t* a_mode, const int64_t* rows, float* const* dW,
                                const int64_t* ld_dw, float* const* db, float* partial, int64_t max_slots,
                                void* rider /* host */, int64_t* slots_out);
int pamnet_wgrad_rider_enqueue_f32(void* ctx /* host */, const void* rider /* host */);

/* ------------------------------------------------------------------------------------------------------------------
 * Fused edge-level kernels (dim = 128), fp32 MFMA.  P planes are node_pre outputs ([N][128] each).
 * global edge (layers/global_message_passing.py:52-56 + PyG propagate gathers):
 *     z = W_e e + b_m + Pi[row_of] + Pj[col];  ea = W_ea e;  msg = SiLU(z) * ea          (z, ea saved for backward)
 *   bwd: dm = d_agg[row_of]; dz = dm*ea*SiLU'(z); dea = dm*SiLU(z); d_e (+)= dz W_e + dea W_ea
 * local edge (layers/local_message_passing.py:46-48,53):  Wq = {W_ji[:,2d:], W_kj[:,2d:], lin_rbf, lin_rbf_out},
 *     P = {ji_i, kj_i, ji_j, kj_j}:  z_ji, z_kj, q2 = lin_rbf r, q3 = lin_rbf_out r, m_ji = SiLU(z_ji),
 *     m_nb = SiLU(z_kj) * q2
 * mlp2 (layers/local_message_passing.py:49 `mlp_sbf`): y = SiLU(W2 SiLU(W1 x + b1) + b2); z1, z2 saved.
 * `accumulate` != 0: the input-gradient output is added to (edge embeddings are shared by all layers).
 * ------------------------------------------------------------------------------------------------------------------ */
int pamnet_global_edge_fwd_f32(const float* e, int64_t n_edges, const float* We, int64_t ld_we, const float* bm,
                               const float* Wea, int64_t ld_wea, const float* Pi, const float* Pj,
                               const int32_t* row_of, const int32_t* col, float* z, float* ea, float* msg,
                               pamnet_stream_t stream);
int pamnet_global_edge_bwd_f32(const float* d_agg, const int32_t* row_of, int64_t n_edges, const float* z,
                               const float* ea, const float* We, int64_t ld_we, const float* Wea, int64_t ld_wea,
                               float* dz, float* dea, float* d_e, int32_t accumulate, pamnet_stream_t stream);
int pamnet_local_edge_fwd_f32(const float* rbf, int64_t n_edges, const float* const* Wq, const int64_t* ldq,
                              const float* b_ji, const float* b_kj, const float* const* P, const int32_t* row_of,
                              const int32_t* col, float* z_ji, float* z_kj, float* q2, float* q3, float* m_ji,
                              float* m_nb, pamnet_stream_t stream);
int pamnet_local_edge_bwd_f32(const float* d_mji, const float* d_mnb, const float* d_q3, int64_t n_edges,
                              const float* z_ji, const float* z_kj, const float* q2, const float* const* Wq,
                              const int64_t* ldq, float* dz_ji, float* dz_kj, float* dq2, float* d_rbf,
                              int32_t accumulate, pamnet_stream_t stream);
/* Edge MLP -> node segment-sum as ONE kernel (csrc/edge_agg.hip; layers/global_message_passing.py:38,52-56): the
 * message tile is reduced over its target node from LDS, the [E,128] message tensor is never written.
 *   fwd: out[i] = init[i] + sum_{e -> i} SiLU(W_e e + b_m + Pi[i] + Pj[col[e]]) * (W_ea e)  for all i < n_nodes
 *        (init nullable = 0; z / ea [E,128]: optional saves for the backward; ptr [n_nodes+1], row_of, col: CSR by target)
 *   bwd: dz, dea, d_e as pamnet_global_edge_bwd_f32, plus dPi[i] = sum_{e -> i} dz[e] (the target-side reduction).
 * Node-aligned work split: every output row has one owner and a fixed CSR summation order (no atomics, no carries;
 * results do not depend on the launch geometry).
 * pamnet_local_agg_fwd_f32 (layers/local_message_passing.py:49-54, one launch for both aggregations):
 *   m_t[e] = m_ji[e] + sum_{r in [t_ptr[e], t_ptr[e+1])} m_nb[t_col[r]] * s[r]     (m_t nullable: backward-only save)
 *   out[i] = init[i] + sum_{e in [l_ptr[i], l_ptr[i+1])} q3[e] * m_t[e] */
int pamnet_global_edge_agg_fwd_f32(const float* e, int64_t n_edges, int64_t n_nodes, const float* We, int64_t ld_we,
                                   const float* bm, const float* Wea, int64_t ld_wea, const float* Pi, const float* Pj,
                                   const int32_t* ptr, const int32_t* row_of, const int32_t* col,
                                   const int32_t* cuts /* nullable: pamnet_seg_cuts_i32 */, const float* init, float* z,
                                   float* ea, float* out, pamnet_stream_t stream);
/* The same operator with the two halves of every workgroup in opposite phases (matrix pipe beside vector units: the form
 * pamnet_global_edge_agg_fwd_f32 takes by itself from 131 072 edges; PAMNET_AGG_PP=0/1 forces either).  Same arguments, the
 * same results bit for bit, whatever the size. */
int pamnet_global_edge_agg_fwd_pp_f32(const float* e, int64_t n_edges, int64_t n_nodes, const float* We, int64_t ld_we,
                                      const float* bm, const float* Wea, int64_t ld_wea, const float* Pi, const float* Pj,
                                      const int32_t* ptr, const int32_t* row_of, const int32_t* col,
                                      const int32_t* cuts /* nullable */, const float* init, float* z, float* ea, float* out,
                                      pamnet_stream_t stream);
/* cuts[0 .. G] = the node-aligned work split of the fused kernels for this graph (node boundary nearest to edge row
 * k * n_edges / G), G = *grid_out <= 256: computed once per graph, handed to every pamnet_global_edge_agg_fwd_f32 launch
 * (without it every workgroup derives its cuts itself: two dependent loads ahead of everything else). */
int pamnet_seg_cuts_i32(const int32_t* ptr, const int32_t* row_of, int64_t n_nodes, int64_t n_edges, int32_t* cuts,
                        int64_t* grid_out, pamnet_stream_t stream);
int pamnet_global_edge_agg_bwd_f32(const float* d_agg, int64_t n_edges, int64_t n_nodes, const int32_t* ptr,
                                   const int32_t* row_of, const int32_t* cuts /* nullable */, const float* z,
                                   const float* ea, const float* We,
                                   int64_t ld_we, const float* Wea, int64_t ld_wea, float* dz, float* dea, float* d_e,
                                   int32_t accumulate, float* dPi, pamnet_stream_t stream);
/* The same backward WITH the step's two weight gradients (layers/global_message_passing.py:52-56: the gradients of the
 * e-block of mlp_m and of W_edge_attr): d ea is not written; every workgroup forms its rows' share of dW_e = dz^T e,
 * dW_ea = dea^T e and of the bias gradient (column sums of dz) and leaves them in `partial`: 2 * G slots of 128 * 128 + 256
 * floats (pamnet_global_edge_agg_wg_floats: *floats, *slots = G), slots [0, G) = dW_e shares + bias parts, [G, 2 G) = dW_ea
 * shares.  pamnet_wgrad_edge_enqueue_f32 registers them with a deferred weight-gradient context: the next
 * pamnet_wgrad_deferred_f32 launch (or pamnet_wgrad_flush_f32) sums them in slot order into dW_e / db / dW_ea.
 * dz, d_e, dPi: bitwise the values of pamnet_global_edge_agg_bwd_f32. */
int pamnet_global_edge_agg_wg_floats(int64_t n_edges, int64_t* floats /* host */, int64_t* slots /* host, nullable */);
int pamnet_global_edge_agg_bwd_wg_f32(const float* d_agg, int64_t n_edges, int64_t n_nodes, const int32_t* ptr,
                                      const int32_t* row_of, const int32_t* cuts /* nullable */, const float* z,
                                      const float* ea, const float* e, const float* We, int64_t ld_we, const float* Wea,
                                      int64_t ld_wea, float* dz, float* d_e, int32_t accumulate, float* dPi, float* partial,
                                      pamnet_stream_t stream);
int pamnet_wgrad_edge_enqueue_f32(void* ctx /* host */, int64_t slots, float* dW_e, int64_t ld_e, float* db /* nullable */,
                                  float* dW_ea, int64_t ld_ea, const float* partial);
int pamnet_local_agg_fwd_f32(const float* m_ji, const float* m_nb, const float* s, const float* q3,
                             const int32_t* t_ptr, const int32_t* t_col, const int32_t* l_ptr, const float* init,
                             int64_t n_nodes, float* m_t, float* out, pamnet_stream_t stream);
/* backward of pamnet_local_agg_fwd_f32, one launch: d_mt[e] = d_x2[l_row[e]] * q3[e];  d_q3[e] = d_x2[l_row[e]] * m_t[e];
 * d_s[r] = m_nb[t_col[r]] * d_mt[t_row[r]];  d_mnb[e'] = sum_{r: t_col[r] = e'} s[r] * d_mt[t_row[r]]
 * (tT_ptr / tT_perm: transposed CSR of t_col over the local edges). */
int pamnet_local_agg_bwd_f32(const float* d_x2, const int32_t* l_row, const float* q3, const float* m_t,
                             const float* m_nb, const float* s, const int32_t* t_ptr, const int32_t* t_col,
                             const int32_t* t_row, const int32_t* tT_ptr, const int32_t* tT_perm,
                             const int32_t* tT_edge /* nullable */, const int32_t* tT_node /* nullable */, int64_t n_edges,
                             float* d_mt, float* d_q3, float* d_s, float* d_mnb, pamnet_stream_t stream);
/* tT_edge[q] = t_row[tT_perm[q]], tT_node[q] = l_row[tT_edge[q]] for the n_rows entries of the transposed triplet / pair list:
 * made once per graph, they turn the gather half of pamnet_local_agg_bwd_f32 from three dependent index reads per term into
 * one level of independent ones (both or neither may be given). */
int pamnet_triplet_transpose_aux_i32(const int32_t* tT_perm, const int32_t* t_row, const int32_t* l_row, int64_t n_rows,
                                     int32_t* out_edge, int32_t* out_node, pamnet_stream_t stream);
int pamnet_mlp2_fwd_f32(const float* x, int64_t rows, const float* W1, const float* b1, const float* W2,
                        const float* b2, float* z1, float* z2, float* y, pamnet_stream_t stream);
/* nsets <= 8 such MLPs on the same input rows in one launch: params[4k..4k+3] = {W1, b1, W2, b2} of set k,
 * outs[3k..3k+2] = {z1, z2, y} (host arrays of device pointers).  The per-layer mlp_sbf of all layers take the same input. */
int pamnet_mlp2_fwd_multi_f32(const float* x, int64_t rows, int64_t nsets, const float* const* params,
                              float* const* outs, pamnet_stream_t stream);
int pamnet_mlp2_bwd_f32(const float* dy, int64_t rows, const float* z1, const float* z2, const float* W1,
                        const float* W2, float* dz1, float* dz2, float* dx, int32_t accumulate,
                        pamnet_stream_t stream);
/* pamnet_mlp2_bwd_f32 + pamnet_local_edge_bwd_f32 -- both depend on pamnet_local_agg_bwd_f32 only, not on each other -- as ONE
 * launch, the CUs split between the two plans by their work (layers/local_message_passing.py:46-53 backward).  Arguments
 * and results are those of the two calls.  Round 6 (ABI 14): accumulate_dx | PAMNET_WEIGHT_IMAGES: W1, W2 are transposed kind-1
 * images of pamnet_pack_weights_mixed_f32; ldq[0..3] all 0 (here and in pamnet_local_edge_bwd_f32): Wq[0..3] are transposed
 * kind-1 images too (the four dX GEMMs of the local edge stage run on the bf16 matrix pipe at fp32 accuracy, like the MLP's).
 * Same bits as with the matrices. */
int pamnet_local_bwd_pair_f32(const float* dy, int64_t rows, const float* z1, const float* z2, const float* W1,
                              const float* W2, float* dz1, float* dz2, float* dx, int32_t accumulate_dx,
                              const float* d_mji, const float* d_mnb, const float* d_q3, int64_t n_edges,
                              const float* z_ji, const float* z_kj, const float* q2, const float* const* Wq,
                              const int64_t* ldq, float* dz_ji, float* dz_kj, float* dq2, float* d_rbf,
                              int32_t accumulate_rbf, pamnet_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Input-embedding layers (128 outputs, K = 16 / 18 / 42 inputs):
 *   out[r, :] = act( W_{kind[r]} x[r, :] + b_{kind[r]} ),  act = SiLU when `act` != 0, identity otherwise.
 * Replaces mlp_rbf_g / mlp_rbf_l (K=16), mlp_sbf1 / mlp_sbf2 (K=42; `kind[r]` = 0 selects (W0,b0), 1 selects (W1,b1) on
 * the combined triplet/pair row list) and init_linear (K=18, no bias, act=0): models.py:119,185-188, layers/basic.py:19-22.
 * W*: [128, K] row-major (out, in); b* nullable; kind nullable (then only W0/b0 are used).
 * Backward writes dW0/db0 (and dW1/db1 when kind != null) = sums over rows, reduced in a fixed order through `partial`
 * (pamnet_embed_scratch_floats floats); dx [rows, K] (nullable) is only available for kind == null, K == 16.
 * (One-job forms of pamnet_embed_multi_*_f32 below.)
 * ------------------------------------------------------------------------------------------------------------------ */
int pamnet_embed_scratch_floats(int64_t rows, int64_t K, int64_t* floats);
int pamnet_embed_fwd_f32(const float* x, int64_t rows, int64_t K, const int32_t* kind, const float* W0,
                         const float* b0, const float* W1, const float* b1, int32_t act, float* out,
                         pamnet_stream_t stream);
int pamnet_embed_bwd_f32(const float* x, int64_t rows, int64_t K, const int32_t* kind, const float* W0,
                         const float* b0, const float* W1, const float* b1, int32_t act, const float* gout,
                         float* dW0, float* db0, float* dW1, float* db1, float* dx, float* partial,
                         pamnet_stream_t stream);

/* All input embeddings of a PAMNet forward (models.py:107/119/140, 185-188) in ONE launch, their backward in TWO (main +
 * fixed-order reduce): up to 4 embedding layers plus the rows of the atom-type table.
 * A job with `dist` != null is a K = 16 layer whose input rows are the Bessel basis of those distances
 * (layers/basic.py:59-76: u(d/c) sin(freq_n d/c), u = the p = 5 envelope): the rows are formed while staging, so neither
 * the [rows, 16] basis nor -- in the backward, where d freq is accumulated in the same pass -- its gradient ever exists.
 * Forward reads x|dist, kind, W*, b*, writes out.  Backward reads the same plus gout and OVERWRITES dW0/db0 (dW1/db1
 * with `kind`), dfreq (with `dist`), dx (nullable; plain K = 16 layer only) through `partial`
 * (pamnet_embed_scratch_floats(rows, K) floats per job).  Unused pointers are null. */
typedef struct pamnet_embed_job {
    const float* x;          /* [rows, K] input rows, or null with `dist` */
    const float* dist;       /* [rows] distances, or null */
    const float* freq;       /* [16] Bessel frequencies (with `dist`) */
    float cutoff;            /* c (with `dist`) */
    int32_t K;               /* 16 | 18 | 42 */
    int32_t act;             /* != 0: SiLU */
    int64_t rows;
    const int32_t* kind;     /* [rows] 0 -> (W0, b0), 1 -> (W1, b1); nullable */
    const float *W0, *b0, *W1, *b1;
    float* out;              /* forward: [rows, 128] */
    const float* gout;       /* backward: d out [rows, 128] */
    float *dW0, *db0, *dW1, *db1, *dfreq, *dx;
    float* partial;
} pamnet_embed_job;
/* rows of the atom-type table: forward out[r, :] = table[idx[r], :] (zeros for idx outside [0, n_types)); backward
 * dtable[t, :] = sum_{r: idx[r] = t} g[r, :] through `scratch` (pamnet_type_rows_scratch_bytes(n_types, 128) bytes; up to 8
 * rows that is pamnet_reduce_scratch_bytes).  Width 128. */
typedef struct pamnet_type_rows_job {
    const float* table;      /* [n_types, 128] */
    const int32_t* idx;      /* [n] */
    int64_t n;
    int64_t n_types;         /* 1 .. 128 (above 8: the wide type-row kernels, csrc/type_rows_core.h) */
    float* out;              /* forward [n, 128] */
    const float* g;          /* backward [n, 128] */
    void* scratch;           /* backward */
    float* dtable;           /* backward [n_types, 128] */
} pamnet_type_rows_job;
int pamnet_embed_multi_fwd_f32(const pamnet_embed_job* jobs, int32_t n_jobs, const pamnet_type_rows_job* types,
                               pamnet_stream_t stream);
int pamnet_embed_multi_bwd_f32(const pamnet_embed_job* jobs, int32_t n_jobs, const pamnet_type_rows_job* types,
                               pamnet_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Layer-stack engine: the n_layer x (global, local) loop of PAMNet.forward (models.py:196-204) in ONE call per
 * direction.  Host-side C++ enqueues ~10 (fwd) / ~20 (bwd) fused launches per layer pair on `stream`.
 *   d          : model width.  128: csrc/engine.hip; 16 / 32 / 64: csrc/narrow_engine.hip (node-side chains as single
 *                launches); any other width -> PAMNET_EINVAL
 *   sizes      : {n, e_g, e_l, tp}
 *   graph_idx  : 18 device index arrays {g_ptr, g_row, g_col, gT_ptr, gT_perm, l_ptr, l_row, l_col, lT_ptr, lT_perm,
 *                tp_ptr, tp_row, tp_col, tpT_ptr, tpT_perm, cuts, tpT_edge, tpT_node}  (the *T_* entries are only read by
 *                the backward; cuts: nullable -- the work split of pamnet_seg_cuts_i32 made with the graph, else computed per
 *                call; tpT_edge / tpT_node: nullable pair -- pamnet_triplet_transpose_aux_i32; the narrow-width engine reads
 *                the first 15)
 *   gparams    : n_layer x 28 device pointers  {mlp_x1.W, .b, mlp_m.W [d,3d], .b, W_edge_attr.W, tail W[10], b[10],
 *                W_out.weight, W_out.bias, W}
 *   lparams    : n_layer x 35 device pointers  {mlp_x1.W, .b, mlp_m_ji.W, .b, mlp_m_kj.W, .b, mlp_sbf.0.W, .b,
 *                mlp_sbf.1.W, .b, lin_rbf.W, lin_rbf_out.W, tail ...}
 *                (the slots of both tables by name: csrc/common.h, namespace pslot)
 *   saved/temp : caller-owned arenas sized by pamnet_stack_workspace (floats); `saved` must survive until the backward
 *   outs/atts  : [2*n_layer, n] rows ordered (global_0, local_0, global_1, ...)
 * pamnet_stack_layout: layout[0] = floats per layer pair in `saved`, layout[1] / [2] = offset of the global / local
 * layer's node output [n, d] within a pair.
 * At d = 16 / 32 / 64, save_for_backward, wpack, aux_stream and aux_events are ignored (every save is written, the
 * weight images are packed inside `temp`, no fork; pamnet_stack_pack_floats reports 0), and the backward needs
 * n, e_g, e_l, tp > 0.
 * wpack (nullable, both directions): scratch of pamnet_stack_pack_floats(n_layer, d) floats; when given, the call first
 * re-packs the node chains' weight matrices into fragment-ordered images (pamnet_pack_weights_f32, one launch) and the
 * chains read those.  Contents need not survive the call.
 * Forward, save_for_backward = 0 (inference): tensors only the backward reads are not written (the single kernels take
 * null for those outputs: z / ea, z_ji / z_kj / q2, z1 / z2, Z / R, Zx1); `saved` still holds the forward's own
 * intermediates and the per-layer node features.
 * Forward, optional fork: `aux_stream` + `aux_events` (n_layer + 1 hipEvent_t handles, both nullable): the per-layer
 * triplet/pair MLPs (independent of the node features) are enqueued on aux_stream up front and joined by event where
 * each layer consumes them; event 0 marks the inputs ready on `stream`.
 * Backward: ggrads / lgrads are gradient buffers laid out like the parameter tables (written, not accumulated);
 * d_x0, d_eg, d_rbf, d_sbf are written.  `layer_done` (nullable): n_layer hipEvent_t handles; event k is recorded on
 * `stream` once every gradient of layer pair k (global_layer.k, local_layer.k) has been enqueued -- the backward runs
 * k = n_layer-1 .. 0, so a data-parallel caller can start reducing the last layers' gradients on another stream while
 * the earlier layers are still being differentiated.
 * ------------------------------------------------------------------------------------------------------------------ */
int pamnet_stack_workspace(int64_t n, int64_t eg, int64_t el, int64_t tp, int64_t n_layer, int64_t d,
                           int64_t* saved_floats, int64_t* temp_floats);
int pamnet_stack_pack_floats(int64_t n_layer, int64_t d, int64_t* floats);
int pamnet_stack_layout(int64_t n, int64_t eg, int64_t el, int64_t tp, int64_t d, int64_t* layout);
int pamnet_stack_fwd_f32(const int64_t* sizes, const int32_t* const* graph_idx, int64_t n_layer, int64_t d,
                         const float* x0, const float* e_g, const float* rbf_e, const float* e_sbf,
                         const float* const* gparams, const float* const* lparams, float* saved, float* temp, float* outs,
                         float* atts, int32_t save_for_backward, float* wpack, pamnet_stream_t aux_stream,
                         void* const* aux_events, pamnet_stream_t stream);
int pamnet_stack_bwd_f32(const int64_t* sizes, const int32_t* const* graph_idx, int64_t n_layer, int64_t d,
                         const float* x0, const float* e_g, const float* rbf_e, const float* e_sbf,
                         const float* const* gparams, const float* const* lparams, const float* saved, float* temp,
                         const float* d_outs, const float* d_atts, float* const* ggrads, float* const* lgrads,
                         float* d_x0, float* d_eg, float* d_rbf, float* d_sbf, float* wpack, void* const* layer_done,
                         pamnet_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Small whole-buffer reductions of the training step (csrc/reduce.hip), fixed summation order.
 *   pamnet_sumsq_partials_f32 : partials[0:256] (fp64) = sums of squares of 256 contiguous slices of g[0:n]; the L2 norm
 *                               (clip_grad_norm_, main_qm9.py:111) is finished inside pamnet_adam_ema_norm_f32
 *   pamnet_l1_loss_f32        : loss[0] = mean|out - y|; d_out[i] = grad_scale * sign(out[i] - y[i]) / n  (main_qm9.py:108)
 *   pamnet_mse_loss_f32       : loss[0] = mean (out - y)^2; d_out[i] = grad_scale * 2 (out[i] - y[i]) / n  (main_pdbbind.py:93)
 *   pamnet_smooth_l1_loss_f32 : loss[0] = mean h(out - y), h(d) = d^2/2 if |d| < 1 else |d| - 1/2 (beta = 1);
 *                               d_out[i] = grad_scale * clamp(out[i] - y[i], -1, 1) / n       (main_rna_puzzles.py:92)
 *                               (all three: one launch, d_out nullable)
 *   pamnet_type_rows_grad_f32 : out[t,:] = sum_{r: idx[r] = t} g[r,:], t < n_types <= 128   (gradient of embeddings[x],
 *                               models.py:107,140); d in {4, 8, 16, ..., 256}; idx outside [0, n_types) adds nothing, a type
 *                               that never occurs gets a zero row; no float atomics, fixed order.  scratch:
 *                               pamnet_type_rows_scratch_bytes(n_types, d) bytes of device memory, no initialisation needed
 *                               (n_types <= 8: the pamnet_reduce_scratch_bytes bytes; above: 1 KB of type sets + 64 partial
 *                               tables, up to 8 MB at 128 x 256)
 * ------------------------------------------------------------------------------------------------------------------ */
int pamnet_reduce_scratch_bytes(int64_t* bytes);
int pamnet_type_rows_scratch_bytes(int64_t n_types, int64_t d, int64_t* bytes);
/* dst[0:n] = src[0:n], 16 bytes per lane, non-temporal (n % 4 == 0): the memory-system calibration beside bench.py's roofline */
int pamnet_stream_copy_f32(const float* src, float* dst, int64_t n, pamnet_stream_t stream);
int pamnet_sumsq_partials_f32(const float* g, int64_t n, double* partials, pamnet_stream_t stream);
int pamnet_l1_loss_f32(const float* out, const float* y, int64_t n, float grad_scale, float* loss, float* d_out,
                       pamnet_stream_t stream);
int pamnet_mse_loss_f32(const float* out, const float* y, int64_t n, float grad_scale, float* loss, float* d_out,
                        pamnet_stream_t stream);
int pamnet_smooth_l1_loss_f32(const float* out, const float* y, int64_t n, float grad_scale, float* loss, float* d_out,
                              pamnet_stream_t stream);
int pamnet_type_rows_grad_f32(const float* g, const int32_t* idx, int64_t n, int64_t n_types, int64_t d, void* scratch,
                              float* out, pamnet_stream_t stream);
/* Chunked forms for parameter groups (pamnet_adam_ema_groups_f32 below).  chunk_group[c] (device, one byte per chunk of 64
 * floats, n / 64 entries) is the group of g[64 c : 64 c + 64]; frozen[0:n_groups] is a HOST array, 1 <= n_groups <=
 * PAMNET_MAX_PARAM_GROUPS; n % 64 == 0.
 *   pamnet_sumsq_partials_masked_f32 : pamnet_sumsq_partials_f32 where chunks of a frozen group contribute nothing (same 256
 *                                      slices, same order: with no frozen group the partials are bit for bit the unmasked ones)
 *   pamnet_grad_accumulate_f32       : acc[0:n] += g[0:n]; g[0:n] = 0 -- one pass, no atomics (gradient accumulation over
 *                                      micro-batches: the update then takes `acc` as its gradient); n % 4 == 0
 *   pamnet_chunk_groups_check        : host-side validation of a chunk map BEFORE it is uploaded (chunk_group_host: HOST array):
 *                                      PAMNET_EINVAL when an id is >= n_groups.  (The kernels themselves take an id modulo 16 and so never index
 *                                      beyond their 16-entry table; table entries past n_groups are frozen.) */
#define PAMNET_MAX_PARAM_GROUPS 16
int pamnet_chunk_groups_check(const uint8_t* chunk_group_host, int64_t n_chunks, int64_t n_groups);
int pamnet_sumsq_partials_masked_f32(const float* g, int64_t n, const uint8_t* chunk_group, int64_t n_groups,
                                     const int32_t* frozen, double* partials, pamnet_stream_t stream);
int pamnet_grad_accumulate_f32(float* acc, float* g, int64_t n, pamnet_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Optimiser tail of the reference loop on flat fp32 buffers, one pass (main_qm9.py:111-112,116; utils/ema.py:13-20):
 *   g *= min(1, max_norm / (*grad_norm + 1e-6))                      clip_grad_norm_ (grad_norm: device scalar, nullable)
 *   Adam(lr, betas, eps, weight_decay, amsgrad=False), update number `step_count` >= 1
 *   shadow = ema_decay * shadow + (1 - ema_decay) * p_new            (shadow nullable: no EMA -- the loops of
 *                                                                     main_pdbbind.py:88-95, main_rna_puzzles.py:86-93)
 *   g = 0 when zero_grad != 0 (the next step's zero_grad, main_qm9.py:105)
 * n % 4 == 0; buffers 16-byte aligned.
 * ------------------------------------------------------------------------------------------------------------------ */
int pamnet_adam_ema_f32(float* p, float* g, float* m, float* v, float* shadow, int64_t n, float lr, float beta1,
                        float beta2, float eps, float weight_decay, int64_t step_count, float ema_decay,
                        const float* grad_norm, float max_norm, int32_t zero_grad, pamnet_stream_t stream);
/* same update, gradient norm = sqrt(sum of the 256 fp64 partials of pamnet_sumsq_partials_f32) added inside the kernel;
 * norm_out[0] (nullable) receives the pre-clip norm */
int pamnet_adam_ema_norm_f32(float* p, float* g, float* m, float* v, float* shadow, int64_t n, float lr, float beta1,
                             float beta2, float eps, float weight_decay, int64_t step_count, float ema_decay,
                             const double* sumsq_partials, float* norm_out, float max_norm, int32_t zero_grad,
                             pamnet_stream_t stream);
/* The same pass with per-element hyper-parameters taken from parameter groups (one launch).  Element i belongs to group
 * chunk_group[i / 64] (device bytes, see pamnet_sumsq_partials_masked_f32); lr_scale / weight_decay / frozen are HOST arrays of
 * n_groups entries (1 <= n_groups <= PAMNET_MAX_PARAM_GROUPS; lr_scale, weight_decay >= 0), copied into the kernel's arguments:
 *   group rate lr_g = lr * lr_scale[g], decay wd_g = weight_decay[g]
 *   decoupled == 0 : g_clipped += wd_g * p          (L2 decay -- as pamnet_adam_ema_norm_f32)
 *   decoupled != 0 : p *= 1 - lr_g * wd_g, then the Adam step on the clipped gradient      (AdamW)
 *   frozen[g] != 0 : p, m, v and shadow of the chunk are neither read nor written; its g is zeroed when zero_grad != 0
 * sumsq_partials: the 256 partials of pamnet_sumsq_partials_masked_f32 with the same map (frozen chunks outside the norm).
 * n % 64 == 0.  With one group {1, wd, not frozen} and decoupled == 0 the result is bit for bit pamnet_adam_ema_norm_f32's. */
int pamnet_adam_ema_groups_f32(float* p, float* g, float* m, float* v, float* shadow, int64_t n, const uint8_t* chunk_group,
                               int64_t n_groups, const float* lr_scale, const float* weight_decay, const int32_t* frozen,
                               float lr, float beta1, float beta2, float eps, int32_t decoupled, int64_t step_count,
                               float ema_decay, const double* sumsq_partials, float* norm_out, float max_norm,
                               int32_t zero_grad, pamnet_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Narrow widths (d = 16 / 32 / 64: the reference's RNA configurations, inference_rna_puzzles.py:29-30,
 * main_rna_puzzles.py:52-53).  Row-wise kernels, one wavefront per 16-row tile; backward kernels recompute the forward
 * pre-activations and return weight gradients reduced in fixed order.  `partial` scratch: *blocks (from
 * pamnet_narrow_blocks(rows, &blocks)) rows of the stride given per call.
 * ------------------------------------------------------------------------------------------------------------------ */
int pamnet_narrow_blocks(int64_t rows, int64_t* blocks /* host */);

/* Global message (layers/global_message_passing.py:52-53, W_m split into node / edge blocks):
 *   msg[q] = SiLU(P[tgt[q], :d] + P[src[q], d:] + e[q] We^T + b) * (e[q] Wea^T);  P is [N, 2d], We/Wea [d, d] with row
 *   strides ldwe / ldwea (multiples of 4).  The caller segment-sums msg over tgt. */
int pamnet_narrow_global_fwd_f32(const float* e, int64_t m, int64_t d, const int32_t* tgt, const int32_t* src,
                                 const float* P, const float* We, int64_t ldwe, const float* bias, const float* Wea,
                                 int64_t ldwea, float* msg, pamnet_stream_t stream);
/* dagg [N, d] = gradient of the aggregated message (d msg[q] = dagg[tgt[q]]).  Outputs: dz [m, d] (the caller
 * segment-sums it over tgt and over src into dP), de [m, d], dWe/dWea [d, d] dense, db [d].
 * partial: pamnet_narrow_blocks(m) x (2 d^2 + d) floats. */
int pamnet_narrow_global_bwd_f32(const float* e, int64_t m, int64_t d, const int32_t* tgt, const int32_t* src,
                                 const float* P, const float* We, int64_t ldwe, const float* bias, const float* Wea,
                                 int64_t ldwea, const float* dagg, float* dz, float* de, float* partial, float* dWe,
                                 float* dWea, float* db, pamnet_stream_t stream);

/* y = SiLU(W2 SiLU(W1 x + b1) + b2) on [m, d] rows (mlp_sbf, layers/local_message_passing.py:24,49); dense [d, d]. */
/* res_x != 0 adds x (the Res block of layers/basic.py:25-33); `res` (optional, [m, d]) adds one more residual row. */
int pamnet_narrow_mlp2_fwd_f32(const float* x, int64_t m, int64_t d, const float* W1, const float* b1, const float* W2,
                               const float* b2, int32_t res_x, const float* res, float* y, pamnet_stream_t stream);
/* dx optional (null: not needed; with res_x it includes the + dy of the skip); dW [2, d, d], db [2, d];
 * partial: blocks x (2 d^2 + 2 d) floats. */
int pamnet_narrow_mlp2_bwd_f32(const float* x, int64_t m, int64_t d, const float* W1, const float* b1, const float* W2,
                               const float* b2, const float* dy, int32_t res_x, float* dx, float* partial, float* dW,
                               float* db, pamnet_stream_t stream);

/* One dense layer y = act(x W^T + b) (layers/basic.py:19-22): W is a [d, d] block with row stride ldw (a column slice of
 * the [d, 3d] message weights included), b optional, act 1 = SiLU / 0 = identity, y with row stride ldy (blocks of a
 * [m, n d] projection).  Backward: dy with row stride lddy; dx optional, accumulate != 0 adds into dx; dW [d, d], db [d]
 * (null without bias); partial: blocks x (d^2 + d) floats. */
int pamnet_narrow_linear_fwd_f32(const float* x, int64_t m, int64_t d, const float* W, int64_t ldw, const float* b,
                                 int32_t act, float* y, int64_t ldy, pamnet_stream_t stream);
int pamnet_narrow_linear_bwd_f32(const float* x, int64_t m, int64_t d, const float* W, int64_t ldw, const float* b,
                                 int32_t act, const float* dy, int64_t lddy, float* dx, int32_t accumulate,
                                 float* partial, float* dW, float* db, pamnet_stream_t stream);

/* Layer heads (layers/global_message_passing.py:47-50): out[n] = o[n] . w_out + b_out, att[n] = o[n] . w_att.
 * Backward: d_o [m, d] and dvec [2 d + 1] = [d w_out | d w_att | d b_out]; partial: blocks x (2 d + 1) floats. */
int pamnet_narrow_heads_fwd_f32(const float* o, int64_t m, int64_t d, const float* w_out, const float* b_out,
                                const float* w_att, float* out, float* att, pamnet_stream_t stream);
int pamnet_narrow_heads_bwd_f32(const float* o, int64_t m, int64_t d, const float* w_out, const float* w_att,
                                const float* g_out, const float* g_att, float* d_o, float* partial, float* dvec,
                                pamnet_stream_t stream);

/* Local-edge gates (layers/local_message_passing.py:46-48 with the split message weights): for local edge q = (src -> tgt)
 *   m_ji[q] = SiLU(P[tgt, 0:d] + P[src, 2d:3d] + Q[q, 0:d] + b_ji)
 *   m_nb[q] = SiLU(P[tgt, d:2d] + P[src, 3d:4d] + Q[q, d:2d] + b_kj) * Q[q, 2d:3d]
 * P [N, 4d], Q [m, 4d].  Backward: dz [m, 2d] (segment-summed by the caller into dP, column-summed into the biases)
 * and dQ [m, 4d] (last block zero). */
int pamnet_narrow_local_gate_fwd_f32(const float* P, const float* Q, const int32_t* tgt, const int32_t* src,
                                     const float* b_ji, const float* b_kj, int64_t m, int64_t d, float* m_ji,
                                     float* m_nb, pamnet_stream_t stream);
int pamnet_narrow_local_gate_bwd_f32(const float* P, const float* Q, const int32_t* tgt, const int32_t* src,
                                     const float* b_ji, const float* b_kj, int64_t m, int64_t d, const float* g_ji,
                                     const float* g_nb, float* dz, float* dQ, pamnet_stream_t stream);

/* Edge-embedding MLPs (models.py:185-188): y = SiLU(W f + b), f [m, k], k = 16 or 42, W [d, k] dense.  With `kind`
 * [m] rows of kind 0 use (Wa, ba) and rows of kind != 0 use (Wb, bb); kind null: one set. */
int pamnet_narrow_embed_fwd_f32(const float* F, int64_t m, int64_t k, int64_t d, const int32_t* kind, const float* Wa,
                                const float* ba, const float* Wb, const float* bb, float* y, pamnet_stream_t stream);
/* dW [sets, d, k], db [sets, d]; df [m, 16] optional (k = 16, one set: the Bessel frequencies are trainable).
 * partial: blocks x sets (d * kp + d) floats, kp = 16 or 48. */
int pamnet_narrow_embed_bwd_f32(const float* F, int64_t m, int64_t k, int64_t d, const int32_t* kind, const float* Wa,
                                const float* ba, const float* Wb, const float* bb, const float* dy, float* df,
                                float* partial, float* dW, float* db, pamnet_stream_t stream);
/* Forward of the 16-wide embedding on Bessel rows formed inside the kernel (BesselBasisLayer, layers/basic.py:59-76, fused
 * into models.py:185-186): dist [m], freq [16], cutoff as for pamnet_rbf_fwd_f32.  The same floats as
 * pamnet_rbf_fwd_f32 followed by pamnet_narrow_embed_fwd_f32 (k = 16); the [m, 16] basis tensor never exists. */
int pamnet_narrow_embed_rbf_fwd_f32(const float* dist, const float* freq, float cutoff, int64_t m, int64_t d,
                                    const float* Wa, const float* ba, float* y, pamnet_stream_t stream);
/* ... and its backward: dW [d, 16]; db_dfreq [d + 16] = the bias gradient followed by the gradient of the 16 frequencies;
 * partial: blocks x (d * 16 + d + 16) floats (blocks = pamnet_narrow_blocks).  Neither the rows nor their gradient exist. */
int pamnet_narrow_embed_rbf_bwd_f32(const float* dist, const float* freq, float cutoff, int64_t m, int64_t d,
                                    const float* Wa, const float* ba, const float* dy, float* partial, float* dW,
                                    float* db_dfreq, pamnet_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Dense layers of any width (csrc/dense.hip): Sequential(Linear, SiLU) of layers/basic.py:19-22 and the bare F.linear
 * projections, for hidden sizes above 128 (models.py:25) and input widths no engine is built for (models.py:187-188 with
 * a non-default num_spherical * num_radial; models.py:119 at such a dim).  fp32-accurate GEMMs on the bf16 matrix pipe
 * (three exact bf16 pieces per operand, six products); no transposed copies, no library GEMM.
 *   fwd:  Z = X W^T + bias (X [n][k] row stride ldx, W [m][k] row stride ldw, bias [m] nullable);
 *         Y [n][m] = act ? SiLU(Z) : Z;  Z [n][m] nullable (the backward of an activated layer needs it).
 *   bwd:  dZ = act ? G * SiLU'(Z) : G (G, Z [n][m]; formed while staging, never stored);
 *         dX [n][k] (nullable) = dZ W;  dW [m][k] (nullable) = dZ^T X;  db [m] (nullable, with dW) = column sums of dZ.
 *         The row sum of dW is split over the grid and reduced in a fixed order (deterministic); `partial`:
 *         pamnet_dense_scratch_floats(n, k, m) floats of caller-owned scratch, required with dW.
 * ------------------------------------------------------------------------------------------------------------------ */
int pamnet_dense_fwd_f32(const float* X, int64_t ldx, const float* W, int64_t ldw, const float* bias, int64_t n,
                         int64_t k, int64_t m, int32_t act, float* Z, float* Y, pamnet_stream_t stream);
int pamnet_dense_scratch_floats(int64_t n, int64_t k, int64_t m, int64_t* floats);
int pamnet_dense_bwd_f32(const float* G, const float* Z, const float* X, int64_t ldx, const float* W, int64_t ldw,
                         int64_t n, int64_t k, int64_t m, int32_t act, float* dX, float* dW, float* db, float* partial,
                         pamnet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PAMNET_HIP_H */
