"""Device-side graph construction for PAMNet.forward (reference models.py:62-98, 104-177).

Everything here runs as HIP kernels from libpamnet_hip.so (csrc/graph.hip, csrc/basis.hip); torch only allocates the
buffers and reads the data-dependent sizes back (E_g, E_l, T+P) -- the reference has the same host round trips hidden in
`repeat_interleave` / boolean masks (models.py:76-96).

Edge storage differs from the reference on purpose: edges are kept in CSR order of the node they are *aggregated at*
(deterministic, atomics-free segment sums), i.e. a permutation of the reference's edge list.  Results are invariant to
that permutation up to fp32 summation order.
"""
import ctypes
import os
from collections import namedtuple

import torch

from . import lib

I32 = torch.int32


def _i32(n, dev):
    return torch.empty(int(n), dtype=I32, device=dev)


def _f32(n, dev):
    return torch.empty(int(n), dtype=torch.float32, device=dev)


class _ZeroArena(object):
    """Index / geometry buffers of the zero-host-sync path come zero-filled out of ONE allocation (one fill launch):
    should the size the host assumed turn out too large, the unwritten tails hold valid indices (row 0) and finite
    values instead of garbage until the deferred check raises."""

    def __init__(self, ints, dev):
        self.buf = torch.zeros(int(ints) + 64, dtype=I32, device=dev)
        self.off = 0

    def take(self, n, dtype=I32):
        n = int(n)
        v = self.buf[self.off:self.off + n]
        self.off += (n + 3) // 4 * 4                      # 16-byte aligned slices
        return v if dtype == I32 else v.view(dtype)


def _alloc_i32(n, dev, zeroed):
    return zeroed.take(n) if zeroed else _i32(n, dev)


def _alloc_f32(n, dev, zeroed):
    return zeroed.take(n, torch.float32) if zeroed else _f32(n, dev)


def exclusive_scan(counts):
    n = counts.numel()
    out = _i32(n + 1, counts.device)
    tmp = _i32((n + 4095) // 4096 + 1, counts.device)
    lib.call('pamnet_exclusive_scan_i32', lib.ptr(counts), lib.ptr(out), n, lib.ptr(tmp), lib.stream_of(counts))
    return out


def csr_from_keys(keys, rows):
    """Stable counting sort: (ptr [rows+1], perm [m]) with keys[perm] non-decreasing."""
    m = keys.numel()
    dev = keys.device
    ptr, perm = _i32(rows + 1, dev), _i32(m, dev)
    cursor, perm_tmp, tmp = _i32(rows + 1, dev), _i32(m, dev), _i32((rows + 4095) // 4096 + 1, dev)
    lib.call('pamnet_csr_from_keys_i32', lib.ptr(keys), m, rows, lib.ptr(ptr), lib.ptr(perm), lib.ptr(cursor),
             lib.ptr(perm_tmp), lib.ptr(tmp), lib.stream_of(keys))
    return ptr, perm


def expand_rows(ptr, total, zeroed=False):
    rows = ptr.numel() - 1
    out = _alloc_i32(total, ptr.device, zeroed)
    lib.call('pamnet_expand_rows_i32', lib.ptr(ptr), rows, lib.ptr(out), int(total), lib.stream_of(ptr))
    return out


_SCALAR_KINDS = {torch.int32: 0, torch.bool: 1, torch.uint8: 1, torch.int64: 2}


def host_ints(*scalars):
    """Data-dependent sizes come back to the host in ONE round trip: every call is a stream synchronisation that drains
    the launch queue, and forward-only runs are bound by exactly these."""
    n = len(scalars)
    ts = [s.reshape(-1)[:1] for s in scalars]
    kinds = [_SCALAR_KINDS.get(t.dtype) for t in ts]
    if None in kinds:
        raise TypeError('host_ints: unsupported dtype %s' % ts[kinds.index(None)].dtype)
    out = torch.empty(n, dtype=torch.int64, device=ts[0].device)
    lib.call('pamnet_gather_scalars_i64', n, (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts]),
             (ctypes.c_int32 * n)(*kinds), lib.ptr(out), lib.stream_of(out))
    return [int(v) for v in out.tolist()]


def _filter_count(ptr_in, nbr, dist, cut):
    rows = ptr_in.numel() - 1
    count = _i32(rows, nbr.device)
    lib.call('pamnet_csr_filter_count_i32', lib.ptr(ptr_in), lib.ptr(nbr), lib.ptr(dist), rows, float(cut),
             lib.ptr(count), lib.stream_of(nbr))
    return exclusive_scan(count)


def _filter_fill(ptr_in, nbr, dist, cut, ptr, total, zeroed=False):
    rows = ptr_in.numel() - 1
    nbr_out, dist_out = _alloc_i32(total, nbr.device, zeroed), _alloc_f32(total, nbr.device, zeroed)
    lib.call('pamnet_csr_filter_fill_i32', lib.ptr(ptr_in), lib.ptr(nbr), lib.ptr(dist), rows, float(cut),
             lib.ptr(ptr), lib.ptr(nbr_out), lib.ptr(dist_out), int(total), lib.stream_of(nbr))
    return ptr, nbr_out, dist_out


def csr_filter(ptr_in, nbr, dist, cut, flag=None):
    ptr = _filter_count(ptr_in, nbr, dist, cut)
    if flag is None:
        return _filter_fill(ptr_in, nbr, dist, cut, ptr, int(ptr[-1]))
    total, bad = host_ints(ptr[-1], flag)
    if bad:
        _raise_bad_inputs()
    return _filter_fill(ptr_in, nbr, dist, cut, ptr, total)


def csr_filter2(ptr_in, nbr, dist, cut_a, cut_b, flag=None):
    """Two cutoffs on the same table (the RNA global / local graphs, models.py:147-156): both counts first, one host
    round trip for the two sizes (and the input-validity flag)."""
    pa, pb = _filter_count(ptr_in, nbr, dist, cut_a), _filter_count(ptr_in, nbr, dist, cut_b)
    if flag is None:
        ta, tb = host_ints(pa[-1], pb[-1])
    else:
        ta, tb, bad = host_ints(pa[-1], pb[-1], flag)
        if bad:
            _raise_bad_inputs()
    return _filter_fill(ptr_in, nbr, dist, cut_a, pa, ta), _filter_fill(ptr_in, nbr, dist, cut_b, pb, tb)


class CSR(object):
    """Rows = aggregation targets.  ptr [rows+1]; row_of [m] (expanded row id); col [m] (the other endpoint)."""
    __slots__ = ('ptr', 'row_of', 'col', 'm', 'rows')

    def __init__(self, ptr, row_of, col):
        self.ptr, self.row_of, self.col = ptr, row_of, col
        self.m, self.rows = int(row_of.numel()), int(ptr.numel() - 1)


class Transpose(object):
    """Transposed CSR of an index list idx [m] over `rows`: entries q of row r are perm[ptr[r]:ptr[r+1]], idx[perm]=r."""
    __slots__ = ('ptr', 'perm', 'rows')

    def __init__(self, idx, rows):
        self.ptr, self.perm = csr_from_keys(idx, rows)
        self.rows = rows


class _Given(object):
    """Transposed CSR whose (ptr, perm) were written by the launch that built the graph (molecule-local builder)."""
    __slots__ = ('ptr', 'perm', 'rows')

    def __init__(self, ptr, perm, rows):
        self.ptr, self.perm, self.rows = ptr, perm, rows


class SymmetricTranspose(object):
    """Transposed CSR of a symmetric graph (a radius graph: rows = targets, ascending columns): the pointer array is
    the graph's own, the permutation is the reverse-edge index -- one bisection per edge (pamnet_reverse_edges_i32)
    instead of a counting sort over the edges.  Same (ptr, perm) as Transpose(csr.col, rows)."""
    __slots__ = ('ptr', 'perm', 'rows')

    def __init__(self, csr):
        self.ptr, self.rows = csr.ptr, csr.rows
        self.perm = _i32(csr.m, csr.ptr.device)
        lib.call('pamnet_reverse_edges_i32', lib.ptr(csr.ptr), lib.ptr(csr.row_of), lib.ptr(csr.col), csr.m,
                 lib.ptr(self.perm), None, lib.stream_of(csr.ptr))


class _NoTransposeT(object):
    ptr = perm = None


_NoTranspose = _NoTransposeT()


class Graph(object):
    """All index / geometry tensors one forward needs (int32 / fp32 on the device)."""

    capped = False        # max_num_neighbors cut a row of the radius graph: not symmetric, general transposes (build_graph)
    cell_tab = None       # periodic batch: the cell table [num_graphs, 18] fp64 every *_pbc_* kernel reads (cell_table)
    img_g = None          # periodic batch with cell_images='all': the image [E_g, 3] int32 of every global edge (radius_img_fill)
    pos_grad = False      # geometry linked to positions that require grad (differentiable_geometry)

    # Row lists / counts per kind are only needed by the generic (non-fused) path and by tests: built on first use so
    # the fused path (which selects weights per row from `tp_kind` inside the kernel) pays no host sync for them.
    @property
    def trip_rows(self):                              # rows fed to mlp_sbf2 (models.py:188)
        if '_trip_rows' not in self.__dict__:
            self._trip_rows = (self.tp_kind == 0).nonzero().view(-1)
        return self._trip_rows

    @property
    def pair_rows(self):                              # rows fed to mlp_sbf1 (models.py:187)
        if '_pair_rows' not in self.__dict__:
            self._pair_rows = (self.tp_kind == 1).nonzero().view(-1)
        return self._pair_rows

    @property
    def n_trip(self):
        return int(self.trip_rows.numel())

    @property
    def n_pair(self):
        return int(self.pair_rows.numel())


PBC_BIT = 128         # flag-word bit: a periodic cell is singular or too small for the cutoffs (csrc/geom_core.h)


_PBC_ROWS = {}        # (three bools, device) -> uint8 [1, 3] on the device: a `pbc` tuple is uploaded once


def _pbc_bytes(pbc, ng, dev):
    """`pbc` as the kernels read it: uint8 [ng, 3], contiguous, on `dev`.  None for None and for the all-true tuple (the twins'
    entry points); a tuple is uploaded once per device and expanded on the device; a bool tensor is viewed as bytes."""
    if pbc is None:
        return None
    if isinstance(pbc, torch.Tensor):
        return pbc.contiguous().view(torch.uint8)
    key = tuple(bool(v) for v in pbc)
    if all(key):
        return None
    row = _PBC_ROWS.get((key, dev))
    if row is None:
        row = _PBC_ROWS[(key, dev)] = torch.tensor([key], dtype=torch.uint8).to(dev)
    return row.expand(ng, 3).contiguous()


def cell_table(cell, cutoff, flag, pbc=None):
    """The table every periodic kernel reads (pamnet_cell_prepare_f64): per graph the cell and its inverse, fp64 [G, 18].  ORs
    PBC_BIT into `flag` (the batch's validity word) when a cell is singular or has a perpendicular height <= 2 * cutoff.
    `pbc` (a bool tensor [G, 3] or three bools, not all true): pamnet_cell_prepare_axes_f64 -- the cell completed with unit
    vectors orthogonal to the periodic ones in place of the open axes' vectors, those axes' inverse entries +0.0 (no kernel
    that reads the table wraps along them), the height condition on the periodic axes only."""
    ng = int(cell.size(0))
    tab = torch.empty((ng, 18), dtype=torch.float64, device=cell.device)
    axes = _pbc_bytes(pbc, ng, cell.device)
    if axes is None:
        lib.call('pamnet_cell_prepare_f64', lib.ptr(cell), ng, float(cutoff), lib.ptr(tab), lib.ptr(flag), lib.stream_of(cell))
    else:
        lib.call('pamnet_cell_prepare_axes_f64', lib.ptr(cell), lib.ptr(axes), ng, float(cutoff), lib.ptr(tab), lib.ptr(flag),
                 lib.stream_of(cell))
    return tab


def cell_images(cell_tab, cutoff_g, flag, pbc=None):
    """The candidate box of the all-image search (pamnet_cell_images_i32): per graph N_k = ceil(cutoff_g / height_k), int32 [G, 3].
    ORs PBC_BIT into `flag` when some N_k > 4 (a height below cutoff_g / 4).  `pbc` as in cell_table
    (pamnet_cell_images_axes_i32): N_k = 0 and no verdict along open axes."""
    ng = int(cell_tab.size(0))
    box = torch.empty((ng, 3), dtype=I32, device=cell_tab.device)
    axes = _pbc_bytes(pbc, ng, cell_tab.device)
    if axes is None:
        lib.call('pamnet_cell_images_i32', lib.ptr(cell_tab), ng, float(cutoff_g), lib.ptr(box), lib.ptr(flag),
                 lib.stream_of(cell_tab))
    else:
        lib.call('pamnet_cell_images_axes_i32', lib.ptr(cell_tab), lib.ptr(axes), ng, float(cutoff_g), lib.ptr(box), lib.ptr(flag),
                 lib.stream_of(cell_tab))
    return box


def radius_img_count(pos, cell_tab, box, node_graph, gptr, r, max_neighbors=0, cap_flag=None):
    """Scanned row sizes of the radius search over all images of a periodic cell (pamnet_radius_img_count_i32): row i counts every
    (atom j, image n) within r of atom i, i's own images included.  No row is ever cut: max_neighbors > 0 only ORs CAP_BIT into
    `cap_flag` for a row whose hits, the query itself counted, exceed it."""
    n = pos.size(0)
    count = _i32(n, pos.device)
    lib.call('pamnet_radius_img_count_i32', lib.ptr(pos), lib.ptr(cell_tab), lib.ptr(box), lib.ptr(node_graph), lib.ptr(gptr), n,
             int(gptr.numel()) - 1, float(r), int(max_neighbors or 0), lib.ptr(count), lib.ptr(cap_flag), lib.stream_of(pos))
    return exclusive_scan(count)


def radius_img_fill(pos, cell_tab, box, node_graph, gptr, r, ptr, total, max_neighbors=0):
    """(ptr, nbr, dist, row_of, img) of that search: ascending (neighbour, image) inside a row; img [total, 3] int32 with
    pos_row - pos_col - img @ cell the edge's vector."""
    dev = pos.device
    nbr, dist, row_of = _i32(total, dev), _f32(total, dev), _i32(total, dev)
    img = torch.empty((total, 3), dtype=I32, device=dev)
    lib.call('pamnet_radius_img_fill_i32', lib.ptr(pos), lib.ptr(cell_tab), lib.ptr(box), lib.ptr(node_graph), lib.ptr(gptr),
             pos.size(0), int(gptr.numel()) - 1, float(r), int(max_neighbors or 0), lib.ptr(ptr), lib.ptr(nbr), lib.ptr(dist),
             lib.ptr(row_of), lib.ptr(img), int(total), lib.stream_of(pos))
    return ptr, nbr, dist, row_of, img


def _call_in_cell(open_sym, pbc_sym, pos, pbc, *rest):
    """lib.call of a kernel that has a periodic twin.  `pbc` None: the open-space symbol; else the tensors the twin takes
    behind `pos` -- (cell_tab,) for the searches, (cell_tab, node_graph) where the kernel has no batch vector of its own."""
    if pbc is None:
        return lib.call(open_sym, lib.ptr(pos), *rest)
    return lib.call(pbc_sym, lib.ptr(pos), *[lib.ptr(t) for t in pbc], *rest)


def radius_count(pos, node_graph, gptr, r, max_neighbors=0, cap_flag=None, cell_tab=None):
    """Scanned neighbour counts of the radius search.  max_neighbors > 0: torch_cluster's max_num_neighbors (first hits in
    index order, the query itself counted); a truncated row ORs CAP_BIT into `cap_flag` (an int32 device word).
    `cell_tab` (cell_table): the search under periodic cells, distances by the minimum image."""
    n = pos.size(0)
    count = _i32(n, pos.device)
    _call_in_cell('pamnet_radius_count_i32', 'pamnet_radius_pbc_count_i32', pos, None if cell_tab is None else (cell_tab,),
                  lib.ptr(node_graph), lib.ptr(gptr), n, int(gptr.numel()) - 1, float(r), int(max_neighbors or 0),
                  lib.ptr(count), lib.ptr(cap_flag), lib.stream_of(pos))
    return exclusive_scan(count)


def radius_fill(pos, node_graph, gptr, r, ptr, total, zeroed=False, rows_out=None, max_neighbors=0, cell_tab=None):
    """`rows_out`: a one-element list that receives the expanded row ids (the query node of every entry), written by the
    same launch."""
    nbr = _alloc_i32(total, pos.device, zeroed)
    dist = _alloc_f32(total, pos.device, zeroed)
    row_of = _alloc_i32(total, pos.device, zeroed) if rows_out is not None else None
    _call_in_cell('pamnet_radius_fill_i32', 'pamnet_radius_pbc_fill_i32', pos, None if cell_tab is None else (cell_tab,),
                  lib.ptr(node_graph), lib.ptr(gptr), pos.size(0), int(gptr.numel()) - 1, float(r), int(max_neighbors or 0),
                  lib.ptr(ptr), lib.ptr(nbr), lib.ptr(dist), lib.ptr(row_of), int(total), lib.stream_of(pos))
    if rows_out is not None:
        rows_out.append(row_of)
    return ptr, nbr, dist


def radius_graph(pos, node_graph, gptr, r):
    ptr = radius_count(pos, node_graph, gptr, r)
    return radius_fill(pos, node_graph, gptr, r, ptr, int(ptr[-1]))


def knn_table(pos, node_graph, gptr, k, cutoff):
    n = pos.size(0)
    nbr, dist = _i32(n * k, pos.device), _f32(n * k, pos.device)
    lib.call('pamnet_knn_i32', lib.ptr(pos), lib.ptr(node_graph), lib.ptr(gptr), n, k, float(cutoff), lib.ptr(nbr),
             lib.ptr(dist), lib.stream_of(pos))
    ptr = (torch.arange(n + 1, device=pos.device, dtype=torch.int64) * k).to(I32)
    return ptr, nbr, dist


# PAMNET_KNN_TP_TOTAL=1: the RNA path's triplet / pair total travels with the two cut sizes in ONE read-back (round 6, verdict item 8).
# Measured SLOWER on the host-bound plain-tensor step (profiles/r06_rna_one_roundtrip_ab.txt: 1.24-1.38 against 1.08-1.10 ms): a fill and
# two launches cost the host more than the second read-back, which the input pipeline hides anyway.  Off by default; kept for A/B.
KNN_TP_TOTAL = os.environ.get('PAMNET_KNN_TP_TOTAL', '0') != '0'


def knn_cuts(pos, node_graph, gptr, k, cut_a, cut_b, flag=None, tp_of_b=None):
    """The kNN search with both cuts of its table (models.py:143-156) in three launches and one host round trip (the two
    sizes + the input-validity flag): the search counts what each cut keeps per query on the way, one launch scans both count
    vectors, one writes both cut lists with their query ids.  Returns ((ptr, nbr, dist, query) of cut a, the same of cut b) --
    the arrays of knn_table + csr_filter2 + expand_rows.  tp_of_b = with_triplets (bool): the triplet + pair row total of the
    graph cut b defines travels in the same round trip (pamnet_knn_tp_total_i64) and is returned third."""
    n, dev = int(pos.size(0)), pos.device
    st = lib.stream_of(pos)
    kn, kd = _i32(n * k, dev), _f32(n * k, dev)
    cnt = _i32(2 * n + 2 * (n + 1) + (n + 4095) // 4096 + 1, dev)
    ca, cb, ra, rb, tmp = cnt[:n], cnt[n:2 * n], cnt[2 * n:3 * n + 1], cnt[3 * n + 1:4 * n + 2], cnt[4 * n + 2:]
    lib.call('pamnet_knn_cut_i32', lib.ptr(pos), lib.ptr(node_graph), lib.ptr(gptr), n, int(k), float(cut_a), float(cut_b),
             lib.ptr(kn), lib.ptr(kd), lib.ptr(ca), lib.ptr(cb), st)
    lib.call('pamnet_exclusive_scan_pair_i32', lib.ptr(ca), lib.ptr(ra), lib.ptr(cb), lib.ptr(rb), n, lib.ptr(tmp), st)
    want = [ra[-1], rb[-1]]
    if tp_of_b is not None:
        buf = torch.zeros((n + 1) // 2 + 1, dtype=torch.int64, device=dev)   # one fill: [n] int32 in-degrees, then the int64 total
        tot = buf[-1:]
        lib.call('pamnet_knn_tp_total_i64', lib.ptr(kn), lib.ptr(kd), n, int(k), float(cut_b), 1 if tp_of_b else 0,
                 lib.ptr(buf), lib.ptr(tot), st)
        want.append(tot)
    if flag is not None:
        want.append(flag)
    got = host_ints(*want)
    ta, tb = got[0], got[1]
    tp_total = got[2] if tp_of_b is not None else None
    if flag is not None and got[-1]:
        _raise_bad_inputs()
    outs = [(_i32(t, dev), _f32(t, dev), _i32(t, dev), _i32(n + 1, dev)) for t in (ta, tb)]
    lib.call('pamnet_knn_cut_fill_i32', lib.ptr(kn), lib.ptr(kd), n, int(k), float(cut_a), lib.ptr(ra), ta, lib.ptr(outs[0][0]),
             lib.ptr(outs[0][1]), lib.ptr(outs[0][2]), lib.ptr(outs[0][3]), float(cut_b), lib.ptr(rb), tb, lib.ptr(outs[1][0]),
             lib.ptr(outs[1][1]), lib.ptr(outs[1][2]), lib.ptr(outs[1][3]), st)
    res = tuple((o[3], o[0], o[1], o[2]) for o in outs)
    return res if tp_of_b is None else res + (tp_total,)


class InverseTranspose(object):
    """Transposed CSR of an edge list that was itself produced by transposing a query-ordered list (the RNA kNN graphs):
    row r = query r holds the new positions of r's original edges -- the query-ordered pointer and the inverse of the
    transposition's permutation, both by-products of _transpose_edges.  Same rows as Transpose(csr.col, n), entries in the
    original (kNN) order inside a row instead of ascending."""
    __slots__ = ('ptr', 'perm', 'rows')

    def __init__(self, ptr, inv):
        self.ptr, self.perm, self.rows = ptr, inv, int(ptr.numel() - 1)


def _transpose_edges(ptr, nbr, dist, n, zeroed=False, want_inverse=False, q=None):
    """CSR by query (q -> nbr) turned into CSR by nbr (aggregate at nbr, other endpoint q).  Returns (ptr, q, dist) of the
    new list and, with want_inverse, the InverseTranspose that gathers along it in the backward."""
    total = int(nbr.numel())
    if q is None:                                 # (query id of every entry: given by the launch that wrote the list)
        q = expand_rows(ptr, total, zeroed=zeroed)
    tptr, perm = csr_from_keys(nbr, n)
    out_q, out_d = _i32(total, nbr.device), _f32(total, nbr.device)
    inv = _i32(total, nbr.device) if want_inverse else None
    lib.call('pamnet_transpose_gather_i32', lib.ptr(perm), lib.ptr(q), lib.ptr(dist), total, lib.ptr(out_q), lib.ptr(out_d),
             lib.ptr(inv), lib.stream_of(nbr))
    return tptr, out_q, out_d, (InverseTranspose(ptr, inv) if want_inverse else None)


def _triplet_ptr(lp, l_src, l_dst, with_triplets):
    """CSR pointer of the combined triplet / pair rows per local edge (models.py:68-98), on the device."""
    e_l = l_src.numel()
    tcount, tpcount = _i32(e_l, l_src.device), _i32(e_l, l_src.device)
    lib.call('pamnet_triplet_count_i32', lib.ptr(lp), lib.ptr(l_src), lib.ptr(l_dst), e_l, 1 if with_triplets else 0,
             lib.ptr(tcount), lib.ptr(tpcount), lib.stream_of(l_src))
    return exclusive_scan(tpcount), tcount


class TripletTranspose(object):
    """Transposed CSR of the triplet / pair rows (for every source bond the rows that gather it): the same (ptr, perm) as
    Transpose(tp.col, e_l), from the structure of the local graph -- two light launches and a scan over the bonds
    (pamnet_triplet_transpose_*_i32) instead of a counting sort over the T + P rows."""
    __slots__ = ('ptr', 'perm', 'rows')

    def __init__(self, loc, loc_T, tp_ptr, tcount, total, with_triplets, zeroed=False):
        e_l, dev = loc.m, loc.ptr.device
        st = lib.stream_of(loc.ptr)
        wt = 1 if with_triplets else 0
        cnt = _i32(e_l, dev)
        lib.call('pamnet_triplet_transpose_count_i32', lib.ptr(loc.ptr), lib.ptr(loc.col), lib.ptr(loc.row_of), lib.ptr(loc_T.ptr),
                 lib.ptr(loc_T.perm), e_l, wt, lib.ptr(cnt), st)
        self.ptr = exclusive_scan(cnt)
        if zeroed:                                    # sizes from the host: capped like every other fill (see build_graph)
            self.ptr = torch.clamp(self.ptr, max=total)
        self.perm = _alloc_i32(total, dev, zeroed)
        lib.call('pamnet_triplet_transpose_fill_i32', lib.ptr(loc.ptr), lib.ptr(loc.col), lib.ptr(loc.row_of), lib.ptr(loc_T.ptr),
                 lib.ptr(loc_T.perm), e_l, wt, lib.ptr(tp_ptr), lib.ptr(tcount), lib.ptr(self.ptr), lib.ptr(self.perm), total, st)
        self.rows = max(e_l, 1)


def _input_flag(node_graph, n_graphs, types=None, n_types=None, src=None, dst=None):
    """Device-side validity flag of the index inputs (the kernels index with whatever they are given): `node_graph`
    (int32) sorted with ids in [0, n_graphs), atom types (a float column, possibly strided) in [0, n_types), edge
    endpoints (int32) in [0, N).  One launch; the flag travels back with the data-dependent sizes in the SAME host round
    trip."""
    flag = _i32(1, node_graph.device)
    ne = 0 if src is None else int(src.numel())
    stride = 0
    if types is not None and n_types is not None:
        assert types.dtype == torch.float32 and types.dim() == 1
        stride = types.stride(0) if types.numel() > 1 else 1
    else:
        types = None
    lib.call('pamnet_validate_inputs_i32', lib.ptr(node_graph), node_graph.numel(), int(n_graphs),
             None if types is None else types.data_ptr(), stride, int(n_types or 0), lib.ptr(src) if ne else None,
             lib.ptr(dst) if ne else None, ne, lib.ptr(flag), lib.stream_of(node_graph))
    return flag


_KINDS = {torch.int64: 1, torch.int32: 2, torch.float32: 3}


def _type_column(x, n):
    """`x` as the flat column of `n` atom types that the ingest launch and the graph engine read, or None."""
    xcol = x.reshape(-1) if (x.dim() == 1 or (x.dim() == 2 and x.size(1) == 1)) else None
    return None if (xcol is None or xcol.dtype not in _KINDS or xcol.numel() != n) else xcol


def _edge_rows(edge_index):
    """The two rows of `edge_index` as the ingest launch and the graph engine read them (contiguous each), or None."""
    if edge_index.dim() != 2 or edge_index.size(0) != 2 or edge_index.dtype not in _KINDS:
        return None
    es, ed = edge_index[0], edge_index[1]
    return (es, ed) if (es.is_contiguous() and ed.is_contiguous()) else None


# totals: four zeroed words behind the flags (the molecule-local builder's counters)
Ingested = namedtuple('Ingested', 'node_graph gptr types src dst flag loops totals')


def ingest(batch, n_graphs, x=None, n_types=None, edge_index=None):
    """The reference's index tensors as the kernels want them, in one launch (pamnet_ingest_indices_i32): int32 batch
    vector, per-graph node pointer, int32 atom types, int32 bond endpoints, and a two-word flag (invalid index / self
    loops in the bond list).  Returns None when a tensor has a layout the launch does not read (the caller then takes
    the tensor-op route)."""
    n = int(batch.numel())
    if batch.dtype not in _KINDS or not batch.is_contiguous() or batch.dim() != 1:
        return None
    xk, xs, xcol = 0, 1, None
    if x is not None and n_types is not None:
        xcol = _type_column(x, n)
        if xcol is None:
            return None
        xk, xs = _KINDS[xcol.dtype], (xcol.stride(0) if n > 1 else 1)
        if xs < 1:
            return None
    ne, ek, es, ed = 0, 0, None, None
    if edge_index is not None:
        rows = _edge_rows(edge_index)
        if rows is None:
            return None
        es, ed = rows
        ne, ek = int(es.numel()), _KINDS[edge_index.dtype]
    dev = batch.device
    na, ea = (n + 3) // 4 * 4, (ne + 3) // 4 * 4          # 16-byte aligned sections of one allocation
    buf = _i32(2 * na + 2 * ea + n_graphs + 7, dev)
    node_graph, types = buf[:n], buf[na:na + n]
    src, dst = buf[2 * na:2 * na + ne], buf[2 * na + ea:2 * na + ea + ne]
    gf = buf[2 * na + 2 * ea:]
    lib.call('pamnet_ingest_indices_i32', batch.data_ptr() if n else None, _KINDS[batch.dtype], n, int(n_graphs),
             xcol.data_ptr() if (xk and n) else None, xk, xs, int(n_types or 1), es.data_ptr() if ne else None,
             ed.data_ptr() if ne else None, ek, ne, node_graph.data_ptr() if n else None, gf.data_ptr(),
             types.data_ptr() if n else None, src.data_ptr() if ne else None, dst.data_ptr() if ne else None,
             lib.stream_of(batch))
    return Ingested(node_graph, gf[:n_graphs + 1], (types if xk else None), src, dst, gf[n_graphs + 1:n_graphs + 2],
                    gf[n_graphs + 2:n_graphs + 3], gf[n_graphs + 3:n_graphs + 7])


def _check_sizes(flag, checks, all_kept=None, loops=None):
    """One launch: OR the size-mismatch bits into the validity flag word (pamnet_check_sizes_i32)."""
    n = len(checks)
    actual = (ctypes.c_void_p * n)(*[lib.ptr(t) for t, _ in checks])
    expected = (ctypes.c_int64 * n)(*[int(v) for _, v in checks])
    lib.call('pamnet_check_sizes_i32', n, actual, expected, None if all_kept is None else lib.ptr(all_kept),
             None if loops is None else lib.ptr(loops), lib.ptr(flag), lib.stream_of(flag))


CAP_BIT = 64          # flag-word bit: max_num_neighbors truncated a row of the radius graph (csrc/graph.hip)


def _raise_bad_inputs():
    raise IndexError('index out of range in the batch handed to PAMNet.forward: `batch` must be sorted with ids in '
                     '[0, num_graphs), atom types in [0, embeddings.size(0)), edge_index in [0, num_nodes)')


_PER_AXIS = ('periodic cell too small or singular%s: with `pbc` the rule holds per axis -- the lattice vectors of the PERIODIC axes of '
             'every graph must be finite and linearly independent, and the height of each periodic axis within the lattice those '
             'axes span (the in-plane heights of a slab, the length of a wire\'s one vector) must lie %s; the vector of an '
             'open axis is not used and has no condition -- replicate the cell along its short periodic directions, lower the '
             'cutoffs, or open the axis (pbc[g, k] = False) if the structure does not repeat along it')


def _raise_bad_cell(cutoff_l, cutoff_g, all_images=False, per_axis=False):
    if per_axis and all_images:
        raise ValueError(_PER_AXIS % (" for cell_images='all'", 'above 2 * cutoff_l = %g and not below cutoff_g / 4 = %g'
                                      % (2 * float(cutoff_l), float(cutoff_g) / 4)))
    if per_axis:
        raise ValueError(_PER_AXIS % ('', 'above 2 * max(cutoff_l, cutoff_g) = %g'
                                      % (2 * max(float(cutoff_l), float(cutoff_g)),)))
    if all_images:
        raise ValueError('periodic cell too small or singular for cell_images=\'all\': every cell of the batch must be non-singular '
                         'with each of its three perpendicular heights |det| / |a_i x a_j| above 2 * cutoff_l = %g (the local graph '
                         'keeps one image per pair) and not below cutoff_g / 4 = %g (the global search tries at most 4 images to '
                         'either side per lattice direction) -- replicate the cell along its short directions, or lower the '
                         'cutoffs' % (2 * float(cutoff_l), float(cutoff_g) / 4))
    rc = max(float(cutoff_l), float(cutoff_g))
    raise ValueError('periodic cell too small or singular: every cell of the batch must be non-singular with each of its three '
                     'perpendicular heights |det| / |a_i x a_j| above 2 * max(cutoff_l, cutoff_g) = %g (each pair then has at '
                     'most one image within the cutoffs) -- replicate the cell into a supercell, or lower the cutoffs' % (2 * rc))


def _checked_cell(cell, dataset, edge_index, sizes, n_graphs, pos):
    """`data.cell` as the kernels read it (fp32 [num_graphs, 9], contiguous), or the refusal that says what to do instead."""
    if dataset != 'QM9':
        raise ValueError('periodic cells (`cell`) are implemented for the QM9 schema (pos + atom types) only, not for %r: drop '
                         '`cell`, or hand the structure over as a QM9-schema batch' % (dataset,))
    if edge_index is not None:
        raise ValueError('periodic batches are bond-free: hand over `cell` without `edge_index` (the local graph is then the '
                         'minimum-image radius graph at cutoff_l), or drop `cell` for a bonded molecule in open space')
    if sizes is not None:
        raise ValueError('a batch that carries host-side `sizes` (store.MoleculeStore) has no periodic path: hand the periodic '
                         'batch over as plain tensors (x, pos, batch, cell) without `sizes`')
    if pos is None:
        raise ValueError('`cell` needs `pos`')
    if not isinstance(cell, torch.Tensor) or cell.dtype != torch.float32 or tuple(cell.shape) != (int(n_graphs), 3, 3):
        raise ValueError('`cell` must be a float32 tensor of shape [num_graphs, 3, 3] = [%d, 3, 3] (row k of cell[g] = lattice '
                         'vector a_k of graph g); got %s %s' % (int(n_graphs), getattr(cell, 'dtype', type(cell)),
                                                                tuple(getattr(cell, 'shape', ()))))
    if cell.device != pos.device:
        raise ValueError('`cell` must live on the device of `pos` (%s); it is on %s -- move it with cell.to(pos.device)'
                         % (pos.device, cell.device))
    if cell.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError('a raw gradient with respect to `cell` is not implemented: detach the cell (cell.detach()) '
                                  'and, for the stress / virial, attach `data.strain = torch.zeros(num_graphs, 3, 3, device=..., '
                                  'requires_grad=True)` and differentiate with respect to it (torch.autograd.grad(E.sum(), '
                                  '[data.pos, data.strain])); forces with respect to `pos` are available')
    return cell.detach().contiguous().view(int(n_graphs), 9)


def _checked_cell_images(cell_images, cell):
    """`data.cell_images`: which images the GLOBAL graph of a periodic batch holds.  Returns True for 'all'."""
    if cell_images is None:
        return False
    if cell_images not in ('minimum', 'all'):
        raise ValueError("`cell_images` must be None, 'minimum' (one image per pair: every cell height above 2 * max(cutoff_l, "
                         "cutoff_g)) or 'all' (every image within cutoff_g in the global graph: heights above 2 * cutoff_l); got %r"
                         % (cell_images,))
    if cell is None:
        raise ValueError('`cell_images` belongs to periodic batches (`cell`): drop it, or hand the structure over with its `cell`')
    return cell_images == 'all'


def _checked_pbc(pbc, cell, n_graphs, pos):
    """`data.pbc`: along which lattice vectors each graph of a periodic batch repeats.  Returns None (absent, or the tuple of
    three True: the fully periodic path and its entry points), the tuple of three bools, or the bool tensor [num_graphs, 3];
    or raises the refusal that says what to do instead."""
    if pbc is None:
        return None
    if cell is None:
        raise ValueError('`pbc` belongs to periodic batches (`cell`): hand the structure over with its `cell` ([num_graphs, 3, '
                         '3]; the vector of an open axis may be zero), or drop `pbc` for molecules in open space')
    if isinstance(pbc, torch.Tensor):
        if pbc.dtype != torch.bool or tuple(pbc.shape) != (int(n_graphs), 3):
            raise ValueError('`pbc` must be a torch.bool tensor of shape [num_graphs, 3] = [%d, 3] (pbc[g, k]: graph g repeats '
                             'along cell[g, k]) or a tuple of three bools for every graph; got %s %s -- convert with '
                             'pbc.to(torch.bool), one row per graph' % (int(n_graphs), pbc.dtype, tuple(pbc.shape)))
        if pbc.device != pos.device:
            raise ValueError('`pbc` must live on the device of `pos` (%s); it is on %s -- move it with pbc.to(pos.device)'
                             % (pos.device, pbc.device))
        return pbc.detach()
    if not isinstance(pbc, (tuple, list)) or len(pbc) != 3 or not all(isinstance(v, bool) for v in pbc):
        raise ValueError('`pbc` must be a tuple or list of three Python bools (the same for every graph) or a torch.bool tensor '
                         'of shape [num_graphs, 3]; got %r -- e.g. pbc = (True, True, False) for a slab whose third lattice '
                         'vector is open' % (pbc,))
    return None if all(pbc) else tuple(pbc)


def _raise_cap_binds(max_nb):
    raise ValueError("max_num_neighbors = %d is below the largest row of the all-image global graph (the atom itself counted), and "
                     "with cell_images='all' no row is cut (a cut multigraph is not symmetric): raise model.max_num_neighbors, or "
                     "set it to None" % max_nb)


def _checked_strain(strain, cell, n_graphs, pos):
    """`data.strain` names the variable of the virial: fp32 zeros [num_graphs, 3, 3] on the device of `pos`, on a periodic batch.
    Returns its count of non-zero entries as a device scalar (it travels with the sizes' round trip, _Sizes.read), or raises the
    refusal that says what to do instead."""
    if cell is None:
        raise ValueError('`strain` belongs to periodic batches (`cell`): drop it -- for an isolated molecule the virial is '
                         'sum_a pos_a (x) dE/dpos_a, from the forces alone -- or hand the structure over with its `cell`')
    if not isinstance(strain, torch.Tensor) or strain.dtype != torch.float32 or tuple(strain.shape) != (int(n_graphs), 3, 3):
        raise ValueError('`strain` must be a float32 tensor of zeros of shape [num_graphs, 3, 3] = [%d, 3, 3] (one strain tensor '
                         'per cell); got %s %s' % (int(n_graphs), getattr(strain, 'dtype', type(strain)),
                                                   tuple(getattr(strain, 'shape', ()))))
    if strain.device != pos.device:
        raise ValueError('`strain` must be a float32 tensor [num_graphs, 3, 3] on the device of `pos` (%s); it is on %s -- create '
                         'it there (torch.zeros(num_graphs, 3, 3, device=pos.device, requires_grad=True))'
                         % (pos.device, strain.device))
    return strain.detach().count_nonzero()


def _raise_nonzero_strain(count):
    raise ValueError('`strain` has %d non-zero entries: it only names the variable of differentiation.  The derivative is taken '
                     'at the geometry given: deform `pos` and `cell` yourself (pos @ (I + eps), cell @ (I + eps)) and pass zeros'
                     % count)


class GraphCheckError(IndexError):
    pass


_CHECK_STREAMS = {}


def read_flags(flags, completed=False):
    """OR of the flag words (int32 device scalars) of some prepared graphs: one readback.  completed=True: the caller
    knows the forwards that wrote them have finished (it has waited for an event recorded behind them) -- the copy then
    runs on a stream of its own instead of queueing behind every step already enqueued on the current one."""
    if not flags:
        return 0
    if completed and flags[0].is_cuda:
        dev = flags[0].device
        st = _CHECK_STREAMS.get(dev)
        if st is None:
            st = _CHECK_STREAMS[dev] = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(st):
            vals = torch.stack(flags).reshape(-1).tolist()
    else:
        vals = torch.stack(flags).reshape(-1).tolist()
    bits = 0
    for v in vals:
        bits |= int(v)
    return bits


def raise_for_flag(bits):
    """Raise for a non-zero flag word of a prepared graph (bit 1: invalid index inputs; the rest: the sizes the host
    assumed in the zero-host-sync path were wrong)."""
    if bits & 1:
        _raise_bad_inputs()
    if bits:
        what = [n for k, n in ((1, 'global edges'), (2, 'local edges'), (3, 'triplet / pair rows'), (4, 'size 4')) if bits & (2 << k - 1)]
        if bits & 32:
            what.append('self loops in edge_index')
        if bits & CAP_BIT:
            raise GraphCheckError('max_num_neighbors binds in this batch (a node has more points within cutoff_g than the '
                                  'radius search keeps, models.py:110,128,301): the one-call graph assumes symmetric radius '
                                  'graphs -- hand the batch over without `sizes` (the plain path builds the capped graph)')
        raise GraphCheckError('the data-dependent sizes handed to PAMNet.forward (`data.sizes`) do not match the batch: '
                              + ', '.join(what) + ' -- results of this batch are invalid')


ENGINE = os.environ.get('PAMNET_GRAPH_ENGINE', '1') != '0'    # measurement aid: 0 = the step-by-step path
# QM9 schema, small molecules: the molecule-local builder (csrc/graph_mol.hip, two launches); False = the step-by-step
# launches (the tests compare the two bit by bit)
MOL_LOCAL = True
KNN_K = 50            # neighbours of the RNA kNN graph (models.py:143): the one value the models and the store's size tables use
MOL_ATOMS, MOL_BONDS = 64, 256                       # per-molecule limits of the builder (graph_mol.hip)


class _Facade(object):
    """CSR / transposed-CSR view of an EngineGraph: `ptr`, `row_of` / `perm`, `col` are arena slices created on first
    access (the engines read raw addresses; tensors are for tests, the per-operator paths and inspection)."""

    def __init__(self, g, fields, m, rows):
        self.__dict__['_g'], self.__dict__['_fields'] = g, fields
        self.m, self.rows = int(m), int(rows)

    def __getattr__(self, name):
        spec = self.__dict__['_fields'].get(name)
        if spec is None:
            raise AttributeError(name)
        v = self.__dict__['_g']._view(*spec)
        self.__dict__[name] = v
        return v


class EngineGraph(Graph):
    """Graph built by ONE call of the graph-construction engine (csrc/graph_engine.hip): every index / geometry array is a
    slice of one int32 arena; Python-side tensors are created lazily, the layer-stack engines get raw addresses."""

    def _view(self, field, count, is_float=False):
        off = self._layout[field]
        if off < 0:
            return None
        v = self._arena[off:off + int(count)]
        return v.view(torch.float32) if is_float else v

    def _addr(self, field):
        off = self._layout[field]
        return None if off < 0 else self._base + 4 * off

    def __getattr__(self, name):                     # only reached when the attribute is not materialised yet
        mk = self.__dict__.get('_lazy', {}).get(name)
        if mk is None:
            raise AttributeError(name)
        v = mk()
        self.__dict__[name] = v
        return v


def _engine_graph(dataset, cutoff_l, cutoff_g, flow, x_raw, batch, pos, edge_index, n_graphs, need_grad, knn_k,
                  with_triplets, n_types, sizes, default_basis=True, mol_local=False, max_nb=0, aux_tables=True):
    """The zero-host-sync graph as one engine call, or None when this batch does not qualify (empty lists, layouts the
    ingest launch does not read): the step-by-step path below then builds it."""
    rna = dataset[:3].lower() == 'rna'
    n = int(batch.numel())
    eg, el, tp = (int(v) for v in sizes)
    if not (ENGINE and batch.is_cuda and n > 0 and min(eg, el, tp) > 0 and batch.dim() == 1 and batch.is_contiguous()
            and batch.dtype in _KINDS):
        return None
    d = lib.GraphDesc()
    d.n, d.n_graphs, d.eg, d.el, d.tp = n, int(n_graphs), eg, el, tp
    d.batch, d.batch_kind = batch.data_ptr(), _KINDS[batch.dtype]
    d.with_triplets, d.knn_k = (1 if with_triplets else 0), int(knn_k)
    d.need_grad = (1 if aux_tables else 2) if need_grad else 0          # 2: transposed lists without the dim-128 engine's aux tables
    d.cutoff_l, d.cutoff_g = float(cutoff_l), float(cutoff_g)
    d.max_neighbors = int(max_nb)
    d.n_types = int(n_types or 0)
    keep = [batch]
    if dataset == 'QM9':
        if pos is None or edge_index is None or n_types is None:
            return None
        xcol, rows = _type_column(x_raw, n), _edge_rows(edge_index)
        if xcol is None or rows is None or int(rows[0].numel()) != el:
            return None
        es, ed = rows
        pos = pos if (pos.dtype == torch.float32 and pos.is_contiguous()) else pos.to(torch.float32).contiguous()
        d.schema, d.n_bonds = 0, el
        d.mol_local = 1 if (mol_local and MOL_LOCAL and not 0 < max_nb <= MOL_ATOMS) else 0
        d.types, d.types_kind, d.types_stride = xcol.data_ptr(), _KINDS[xcol.dtype], (xcol.stride(0) if n > 1 else 1)
        d.pos, d.edge_src, d.edge_dst, d.edge_kind = pos.data_ptr(), es.data_ptr(), ed.data_ptr(), _KINDS[edge_index.dtype]
        keep += [xcol, pos, edge_index]
    else:
        if x_raw.dim() != 2 or x_raw.dtype != torch.float32 or not x_raw.is_contiguous() or x_raw.size(1) < 4:
            return None
        w = int(x_raw.size(1))
        d.rows, d.rows_width, d.n_bonds = x_raw.data_ptr(), w, 0
        if rna:
            if n_types is None or not 1 <= int(knn_k) <= 64:        # (pamnet_graph_plan rejects k > 64: the step-by-step
                return None                                          #  path below has its own guard and message)
            d.schema, d.types, d.types_kind, d.types_stride = 2, x_raw.data_ptr() + 4 * (w - 1), 3, w
            d.aggregate_at_query = 1 if flow == 'target_to_source' else 0
        elif dataset == 'PDBbind':
            if not cutoff_l <= cutoff_g:
                return None
            d.schema = 1
        else:
            return None
        keep.append(x_raw)
    layout = (ctypes.c_int64 * lib.GRAPH_FIELDS)()
    need = ctypes.c_int64(0)
    lib.call('pamnet_graph_plan', ctypes.addressof(d), ctypes.addressof(layout), ctypes.addressof(need))
    dev = batch.device
    arena = torch.empty(int(need.value), dtype=I32, device=dev)
    # the engine forms the default (7, 6, 5) basis in the same call; any other size is the model's own launch pair
    sbf = torch.empty((tp, 42), dtype=torch.float32, device=dev) if default_basis else None
    lib.call('pamnet_graph_build_i32', ctypes.addressof(d), arena.data_ptr(), lib.ptr(sbf), lib.stream_of(batch))
    F = lib.GF
    g = EngineGraph()
    g._arena, g._layout, g._base, g._inputs = arena, list(layout), arena.data_ptr(), keep
    g.n, g.n_graphs, g.need_grad_built = n, int(n_graphs), bool(need_grad)
    g.sbf, g._sbf_cutoff = sbf, float(cutoff_l)
    g.check = g._view(F['FLAG'], 1)
    g.pos = pos if dataset == 'QM9' else None
    ng = int(n_graphs)
    lazy = {
        'node_graph': lambda: g._view(F['NODE_GRAPH'], n), 'gptr': lambda: g._view(F['GPTR'], ng + 1),
        'types': lambda: g._view(F['TYPES'], n), 'sign': lambda: g._view(F['SIGN'], n, True),
        'loops': lambda: g._view(F['LOOPS'], 1),
        'dist_g': lambda: g._view(F['G_DIST'], eg, True), 'dist_l': lambda: g._view(F['L_DIST'], el, True),
        'tp_angle': lambda: g._view(F['T_ANGLE'], tp, True), 'tp_kind': lambda: g._view(F['T_KIND'], tp),
        'cuts': lambda: g._view(F['CUTS'], 257),
        'glob': lambda: _Facade(g, {'ptr': (F['G_PTR'], n + 1), 'row_of': (F['G_ROW'], eg), 'col': (F['G_COL'], eg)}, eg, n),
        'loc': lambda: _Facade(g, {'ptr': (F['L_PTR'], n + 1), 'row_of': (F['L_ROW'], el), 'col': (F['L_COL'], el)}, el, n),
        'tp': lambda: _Facade(g, {'ptr': (F['T_PTR'], el + 1), 'row_of': (F['T_ROW'], tp), 'col': (F['T_COL'], tp)}, tp, el),
    }
    if dataset != 'QM9':
        lazy['pos'] = lambda: g._view(F['POS'], 3 * n, True).view(n, 3)
        del g.__dict__['pos']
    if need_grad:
        lazy['glob_T'] = lambda: _Facade(g, {'ptr': (F['GT_PTR'], n + 1), 'perm': (F['GT_PERM'], eg)}, eg, n)
        lazy['loc_T'] = lambda: _Facade(g, {'ptr': (F['LT_PTR'], n + 1), 'perm': (F['LT_PERM'], el)}, el, n)
        lazy['tp_T'] = lambda: _Facade(g, {'ptr': (F['TT_PTR'], el + 1), 'perm': (F['TT_PERM'], tp)}, tp, el)
    else:
        g.glob_T = g.loc_T = g.tp_T = _NoTranspose
    g.__dict__['_lazy'] = lazy
    # pointer tables of the layer-stack engine (stack._graph_tables): raw addresses, no tensors
    order = ('G_PTR', 'G_ROW', 'G_COL', 'GT_PTR', 'GT_PERM', 'L_PTR', 'L_ROW', 'L_COL', 'LT_PTR', 'LT_PERM',
             'T_PTR', 'T_ROW', 'T_COL', 'TT_PTR', 'TT_PERM', 'CUTS', 'TT_EDGE', 'TT_NODE')
    idx = (ctypes.c_void_p * 18)()
    for k, name in enumerate(order):
        idx[k] = g._addr(F[name])
    g._tables = ((ctypes.c_int64 * 4)(n, eg, el, tp), idx)
    g._sizes = (n, eg, el, tp)
    return g


def _mol_local_graph(g, pos, ing, cutoff_g, with_triplets, need_grad, cutoff_l=None, cell_tab=None, strain_nz=None,
                     per_axis=False):
    """QM9 schema, plain tensors: the molecule-local builder (csrc/graph_mol.hip) -- count launch, ONE host round trip for
    the sizes / validity / qualification, fill launch.  Fills `g` and returns True; False when the batch does not qualify
    (a molecule over the builder's limits, bonds not grouped by molecule, self loops): nothing of `g` was touched.
    `cutoff_l`: the bond-free form -- `ing` carries no bonds, the local graph is the radius graph at cutoff_l and its size
    comes back with the other totals.  `cell_tab` (cell_table; bond-free form only): the periodic form -- the same two launches
    with every displacement the minimum-image one (pamnet_mol_graph_pbc_*); the table's verdict (PBC_BIT of the flag word) and
    `strain_nz` (_checked_strain) travel in the same round trip and raise in _Sizes.read's order.  `per_axis`: the table was
    made with `pbc` (the wording of a bad cell's refusal)."""
    gptr, src0, dst0, flag, loops, totals = ing.gptr, ing.src, ing.dst, ing.flag, ing.loops, ing.totals
    dev = pos.device
    free = cutoff_l is not None
    n, ng, m = g.n, g.n_graphs, int(src0.numel())
    st = lib.stream_of(pos)
    mol_tot = _i32(4 * ng, dev)
    wt = 1 if with_triplets else 0
    local = (float(cutoff_l),) if free else (lib.ptr(src0), lib.ptr(dst0), m)      # what defines the local graph
    pbc = None if cell_tab is None else (cell_tab,)
    assert free or pbc is None                        # (periodic batches are bond-free: _checked_cell)
    _call_in_cell('pamnet_mol_graph_free_count_i32' if free else 'pamnet_mol_graph_count_i32', 'pamnet_mol_graph_pbc_count_i32',
                  pos, pbc, lib.ptr(gptr), n, ng, *local, float(cutoff_g), wt, lib.ptr(mol_tot), lib.ptr(totals), st)
    got = host_ints(totals[0], totals[1], totals[2], totals[3], flag, loops, *(() if strain_nz is None else (strain_nz,)))
    nz = 0 if strain_nz is None else got.pop()
    eg, tp, viol, counted, bad, lp_ = got
    if bad & ~(PBC_BIT if pbc else 0):
        _raise_bad_inputs()
    if bad:
        _raise_bad_cell(cutoff_l, cutoff_g, per_axis=per_axis)
    if nz:
        _raise_nonzero_strain(nz)
    if free:
        m = counted
    if viol or lp_ or counted != m or eg <= 0 or tp <= 0:
        return False
    def carve(sizes):                                 # one int32 allocation, 16-byte aligned slices
        offs, tot = [], 0
        for k in sizes:
            offs.append(tot)
            tot += (k + 3) // 4 * 4
        buf = _i32(tot, dev)
        return [buf[o:o + k] for o, k in zip(offs, sizes)]

    (g_ptr, l_ptr, lT_ptr, l_row, l_col, lT_perm, t_ptr, tT_ptr, g_row, g_col, gT_perm, t_row, t_col, t_kind,
     tT_perm) = carve([n + 1] * 3 + [m] * 3 + [m + 1] * 2 + [eg] * 3 + [tp] * 4)
    l_dist, g_dist, t_angle = _f32(m, dev), _f32(eg, dev), _f32(tp, dev)
    o = lib.MolGraphOut()
    o.g_ptr, o.g_row, o.g_col, o.g_dist = g_ptr.data_ptr(), g_row.data_ptr(), g_col.data_ptr(), g_dist.data_ptr()
    o.l_ptr, o.l_row, o.l_col, o.l_dist = l_ptr.data_ptr(), l_row.data_ptr(), l_col.data_ptr(), l_dist.data_ptr()
    o.t_ptr, o.t_row, o.t_col = t_ptr.data_ptr(), t_row.data_ptr(), t_col.data_ptr()
    o.t_angle, o.t_kind = t_angle.data_ptr(), t_kind.data_ptr()
    if need_grad:
        o.gT_perm, o.lT_ptr, o.lT_perm = gT_perm.data_ptr(), lT_ptr.data_ptr(), lT_perm.data_ptr()
        o.tT_ptr, o.tT_perm = tT_ptr.data_ptr(), tT_perm.data_ptr()
    local = (m, float(cutoff_l)) if free else (lib.ptr(src0), lib.ptr(dst0), m)
    _call_in_cell('pamnet_mol_graph_free_fill_i32' if free else 'pamnet_mol_graph_fill_i32', 'pamnet_mol_graph_pbc_fill_i32',
                  pos, pbc, lib.ptr(gptr), n, ng, *local, float(cutoff_g), wt, 1 if need_grad else 0, lib.ptr(mol_tot), eg, tp,
                  ctypes.addressof(o), st)
    if cell_tab is not None:
        g.cell_tab = cell_tab
    g.loops = loops
    g.pos = pos
    g.glob, g.dist_g = CSR(g_ptr, g_row, g_col), g_dist
    g.loc, g.dist_l = CSR(l_ptr, l_row, l_col), l_dist
    g.tp = CSR(t_ptr, t_row, t_col)
    g.tp_angle, g.tp_kind = t_angle, t_kind
    g.glob_T = g.loc_T = g.tp_T = _NoTranspose
    if need_grad:
        g.glob_T = _Given(g_ptr, gT_perm, n)
        g.loc_T = _Given(lT_ptr, lT_perm, n)
        g.tp_T = _Given(tT_ptr, tT_perm, max(m, 1))
    return True


class _Sizes(object):
    """Where the data-dependent sizes of one build come from (build_graph, `sizes`).  None: from the device, in host round
    trips that carry the validity flag word along (read).  Host numbers: the buffers come zero-filled out of `arena` (what the
    `zeroed=` parameters take), every device total is expected to be its host number (expect), one launch checks them at the end."""
    __slots__ = ('flag', 'known', 'arena', 'checks')

    def __init__(self, flag, sizes):
        self.flag, self.arena = flag, False
        self.known = None if sizes is None else tuple(int(v) for v in sizes)
        self.checks = []                          # (device total, value the host assumed)

    def reserve(self, ints, dev):
        self.arena = _ZeroArena(ints, dev)

    def expect(self, ptr, k, clamp=True):
        """The scanned pointer `ptr` is expected to end at `k`.  Returns it capped at k, what the buffers hold: with sizes that
        turn out too small every kernel that walks it still stays inside its arrays (such a batch is invalid and flagged)."""
        self.checks.append((ptr[-1:], k))
        return torch.clamp(ptr, max=k) if clamp else ptr

    def read(self, *scalars, allow=0, cutoffs=None, strain_nz=None):
        """The device scalars and the flag word in ONE host round trip: (integers, capped).  Raises for a flag bit outside
        `allow` (CAP_BIT: the neighbour cap bound, no error; PBC_BIT: a bad cell, raised second, with `cutoffs`).  `strain_nz`
        (_checked_strain): one more device scalar of the same read, raised last when it is not zero."""
        if strain_nz is None:
            got, nz = host_ints(*scalars, self.flag), 0
        else:
            got = host_ints(*scalars, self.flag, strain_nz)
            nz = got.pop()
        bad = got.pop()
        if bad & ~allow:
            _raise_bad_inputs()
        if bad & PBC_BIT:
            _raise_bad_cell(*cutoffs)
        if nz:
            _raise_nonzero_strain(nz)
        return got, bool(bad & CAP_BIT)


class _Lists(object):
    """What a schema's list builder hands to the common tail (_finish): the global list by aggregation row (gp, gn, gd; g_rows
    = the expanded row ids when the fill wrote them), the local one (lp, l_src, l_dst, l_dist), and what the builder happens
    to know already."""
    sign = cell_tab = None                        # PDBbind: +1 pocket / -1 ligand per node; periodic batch: cell_table
    img_g = None                                  # periodic batch, cell_images='all': the image of every global edge
    gp = gn = gd = g_rows = lp = l_src = l_dst = l_dist = None
    tp_ptr = tp_total = tcount = None             # triplet / pair pointer, total and triplet counts, if made already
    tp_hint = None                                # triplet + pair rows already known on the host
    capped = False                                # max_num_neighbors cut a row: the global list is not symmetric
    glob_inv = loc_inv = None                     # InverseTranspose of a list that was stored by query and then transposed
    loc_radius = False                            # the local list is an uncapped radius graph (symmetric)
    loops = all_kept = None                       # bonded QM9: the self-loop words the size check folds in

    def __init__(self, pos, sz):
        self.pos, self.sz = pos, sz

    def global_by_neighbour(self, n, need_grad, zeroed=False):
        """edge_index_g = (query, neighbour) and the layer aggregates at edge_index[1] = the NEIGHBOUR
        (global_message_passing.py:38 with flow = source_to_target): a symmetric list can be read either way, a capped or
        kNN one has to be stored by neighbour."""
        self.gp, self.gn, self.gd, self.glob_inv = _transpose_edges(self.gp, self.gn, self.gd, n, zeroed=zeroed,
                                                                    want_inverse=need_grad, q=self.g_rows)
        self.g_rows = None


_Args = namedtuple('_Args', 'cutoff_l cutoff_g flow x_raw pos edge_index need_grad knn_k with_triplets n_types sizes mol_local '
                            'max_nb cell strain_nz all_images pbc')
_Bonds = namedtuple('_Bonds', 'ptr src dst dist tp_ptr tcount raw')


def _flag(g, ing, types=None, n_types=None, src=None, dst=None):
    """The validity flag word of the batch: the ingest launch's, or a validation launch of its own (tensor-op route)."""
    if ing is not None:
        return ing.flag
    if types is not None:
        types = types.to(torch.float32).reshape(-1)
    return _input_flag(g.node_graph, g.n_graphs, types, n_types, src, dst)


def _builder_applies(g, ing, a):
    """Plain QM9-schema tensors that the molecule-local builder may take: the ingest launch's outputs, no host sizes, and
    small molecules on average unless the caller vouches for every one."""
    return (a.sizes is None and ing is not None and MOL_LOCAL and a.mol_local is not False
            and not 0 < a.max_nb <= MOL_ATOMS            # (a molecule of <= MOL_ATOMS atoms cannot reach a larger cap)
            and (a.mol_local is True or g.n <= MOL_ATOMS * g.n_graphs // 2))


def _symmetric_tp_total(ptr, with_triplets):
    """Triplet + pair rows of a symmetric graph from its degrees alone (a device scalar): every edge (j -> i) has deg(j) - 1
    triplets (edges k -> j, k != i) and deg(i) pairs (edges j' -> i, itself included; models.py:68-98)."""
    deg = (ptr[1:] - ptr[:-1]).long()
    return (deg * deg + (deg * (deg - 1) if with_triplets else 0)).sum()


def _bond_lists(pos, n, with_triplets, ei=None, raw=None):
    """The bond graph by target with its lengths and its triplet / pair pointer; j, i = edge_index (models.py:64)."""
    src0, dst0 = raw if raw is not None else (ei[0].to(I32).contiguous(), ei[1].to(I32).contiguous())
    ptr, perm = csr_from_keys(dst0, n)
    m, dev = int(src0.numel()), pos.device
    src, dst, dist = _i32(m, dev), _i32(m, dev), _f32(m, dev)
    lib.call('pamnet_gather2_i32', lib.ptr(perm), lib.ptr(src0), lib.ptr(dst0), m, lib.ptr(src), lib.ptr(dst),
             lib.ptr(pos), lib.ptr(dist), lib.stream_of(src0))                    # + the bond lengths (models.py:65)
    tp_ptr, tcount = _triplet_ptr(ptr, src, dst, with_triplets)
    return _Bonds(ptr, src, dst, dist, tp_ptr, tcount, (src0, dst0))


def _qm9_bond_free(g, ing, a):
    """Bond-free molecules: the local graph is the radius graph at cutoff_l inside every molecule (what the reference's
    forward, models.py:104-115, computes when handed edge_index = radius(pos, pos, cutoff_l, batch, batch): get_edge_info
    strips the self loops) -- a search of its own, without a neighbour cap, so cutoff_l may lie on either side of cutoff_g
    and a cap that binds in the global search leaves it alone.  Returns None when the molecule-local builder has filled `g`.

    A periodic batch takes the builder only when the caller vouches for it (mol_local=True): the cell table, the count launch,
    the one round trip, the fill launch.  One that does not qualify after all (a cell over the builder's limits, an empty list)
    goes on below with the table already prepared.  cell_images='all' never does: the all-image global graph is a multigraph
    whose rows repeat columns and may exceed 64 entries, not an adjacency mask per atom."""
    pos = a.pos.to(torch.float32).contiguous()
    flag = _flag(g, ing, a.x_raw, a.n_types)
    tab = None
    if _builder_applies(g, ing, a) and (a.cell is None or (a.mol_local is True and not a.all_images)):
        if a.cell is not None:
            tab = cell_table(a.cell, max(float(a.cutoff_l), float(a.cutoff_g)), flag, a.pbc)
        if _mol_local_graph(g, pos, ing, a.cutoff_g, a.with_triplets, a.need_grad, cutoff_l=a.cutoff_l, cell_tab=tab,
                            strain_nz=a.strain_nz, per_axis=a.pbc is not None):
            return None
    r = _Lists(pos, _Sizes(flag, a.sizes))
    sz, r.loc_radius = r.sz, True
    if a.all_images:
        return _all_image_lists(g, a, r, flag)
    # Periodic cells: the same sequence with the minimum-image forms of the two searches and of the angle fill.  The table is
    # prepared first; its verdict (PBC_BIT) travels in the validity word with the sizes' round trip.
    if a.cell is not None and tab is None:
        tab = cell_table(a.cell, max(float(a.cutoff_l), float(a.cutoff_g)), flag, a.pbc)
    r.cell_tab = tab
    gptr_g = radius_count(pos, g.node_graph, g.gptr, a.cutoff_g, a.max_nb, flag, cell_tab=tab)
    lp = radius_count(pos, g.node_graph, g.gptr, a.cutoff_l, cell_tab=tab)
    if sz.known is not None:
        total_g, total_l, r.tp_hint = sz.known
        sz.reserve(3 * total_g + 3 * total_l + 5 * r.tp_hint + 64, pos.device)
        gptr_g, lp = sz.expect(gptr_g, total_g), sz.expect(lp, total_l)
    else:
        (total_g, total_l, r.tp_hint), r.capped = sz.read(gptr_g[-1], lp[-1], _symmetric_tp_total(lp, a.with_triplets),
                                                          allow=CAP_BIT | PBC_BIT,
                                                          cutoffs=(a.cutoff_l, a.cutoff_g, False, a.pbc is not None),
                                                          strain_nz=a.strain_nz)
    rows = []
    r.gp, r.gn, r.gd = radius_fill(pos, g.node_graph, g.gptr, a.cutoff_g, gptr_g, total_g, zeroed=sz.arena, rows_out=rows,
                                   max_neighbors=a.max_nb, cell_tab=tab)
    r.g_rows = rows.pop()
    if r.capped and a.flow != 'target_to_source':
        r.global_by_neighbour(g.n, a.need_grad)
    r.lp, r.l_src, r.l_dist = radius_fill(pos, g.node_graph, g.gptr, a.cutoff_l, lp, total_l, zeroed=sz.arena, rows_out=rows,
                                          cell_tab=tab)
    r.l_dst = rows.pop()
    return r


def _all_image_lists(g, a, r, flag):
    """cell_images='all': the local graph as ever -- the minimum-image radius graph at cutoff_l, which alone has to be a simple
    graph, so the cells need heights above 2 * cutoff_l only -- and the global graph over every image within cutoff_g, a
    multigraph with an image per edge (radius_img_fill).  The same single round trip: the cell's verdict (both conditions raise
    PBC_BIT) and the cap's travel in the validity word with the sizes.  No row is cut, so a cap that binds is an error."""
    pos, sz = r.pos, r.sz
    assert sz.known is None                       # (periodic batches carry no host sizes: _checked_cell)
    tab = r.cell_tab = cell_table(a.cell, float(a.cutoff_l), flag, a.pbc)
    box = cell_images(tab, a.cutoff_g, flag, a.pbc)
    gptr_g = radius_img_count(pos, tab, box, g.node_graph, g.gptr, a.cutoff_g, a.max_nb, flag)
    lp = radius_count(pos, g.node_graph, g.gptr, a.cutoff_l, cell_tab=tab)
    (total_g, total_l, r.tp_hint), capped = sz.read(gptr_g[-1], lp[-1], _symmetric_tp_total(lp, a.with_triplets),
                                                    allow=CAP_BIT | PBC_BIT,
                                                    cutoffs=(a.cutoff_l, a.cutoff_g, True, a.pbc is not None),
                                                    strain_nz=a.strain_nz)
    if capped:
        _raise_cap_binds(a.max_nb)
    r.gp, r.gn, r.gd, r.g_rows, r.img_g = radius_img_fill(pos, tab, box, g.node_graph, g.gptr, a.cutoff_g, gptr_g, total_g,
                                                          max_neighbors=a.max_nb)
    rows = []
    r.lp, r.l_src, r.l_dist = radius_fill(pos, g.node_graph, g.gptr, a.cutoff_l, lp, total_l, rows_out=rows, cell_tab=tab)
    r.l_dst = rows.pop()
    return r


def _qm9_bonded(g, ing, a):
    """One host round trip for all three data-dependent sizes: the bond graph's CSR and its triplet / pair counts do not
    depend on the radius graph, so they are computed first, on the assumption that the bond list has no self loops
    (remove_self_loops, models.py:63, is a no-op for QM9 bond graphs); the flag that verifies it comes back with the sizes,
    and a batch that does have self loops is redone the slow way.  Returns None when the molecule-local builder has filled `g`."""
    pos = a.pos.to(torch.float32).contiguous()
    n, ei = g.n, a.edge_index
    if ei.size(1) > 0 and _builder_applies(g, ing, a):
        if _mol_local_graph(g, pos, ing, a.cutoff_g, a.with_triplets, a.need_grad):
            return None
    b = _bond_lists(pos, n, a.with_triplets, ei, None if ing is None else (ing.src, ing.dst))
    flag = _flag(g, ing, a.x_raw, a.n_types, *b.raw)
    r = _Lists(pos, _Sizes(flag, a.sizes))
    sz = r.sz
    if ing is not None:                           # self loops were noted by the ingest launch: non-zero = NOT all kept
        kept = r.loops = ing.loops
    else:
        kept = (ei[0] != ei[1]).all()
    gptr_g = radius_count(pos, g.node_graph, g.gptr, a.cutoff_g, a.max_nb, flag)    # symmetric (unless the cap binds): agg = query
    tp_ptr = b.tp_ptr
    if sz.known is not None:
        total_g, total_l, tp_total = sz.known
        if ing is None:
            r.all_kept = kept
        sz.reserve(3 * total_g + 5 * tp_total + 64, pos.device)
        gptr_g = sz.expect(gptr_g, total_g)
        sz.expect(b.ptr, total_l, clamp=False)    # (the bond count is an input size: nothing is sized by it)
        tp_ptr = sz.expect(tp_ptr, tp_total)
    else:
        (total_g, k, tp_total), r.capped = sz.read(gptr_g[-1], kept, tp_ptr[-1], allow=CAP_BIT)
        if (k != 0) if ing is not None else (not k):                            # the bond list has self loops
            b = _bond_lists(pos, n, a.with_triplets, ei[:, ei[0] != ei[1]])
            tp_ptr, tp_total = b.tp_ptr, int(b.tp_ptr[-1])
    rows = []
    r.gp, r.gn, r.gd = radius_fill(pos, g.node_graph, g.gptr, a.cutoff_g, gptr_g, total_g, zeroed=sz.arena, rows_out=rows,
                                   max_neighbors=a.max_nb)
    r.g_rows = rows.pop()
    if r.capped and a.flow != 'target_to_source':
        r.global_by_neighbour(n, a.need_grad)
    r.lp, r.l_src, r.l_dst, r.l_dist = b.ptr, b.src, b.dst, b.dist
    r.tp_ptr, r.tp_total, r.tcount = tp_ptr, tp_total, b.tcount
    return r


def _pdbbind(g, ing, a):
    """ONE host round trip for all three data-dependent sizes.  The local graph (global edges with dist <= cutoff_l,
    models.py:131-134) is the radius graph at cutoff_l, so its per-node degrees come from a second count pass over the
    positions instead of from the filled global graph; and because a radius graph is symmetric, the number of triplet / pair
    rows follows from the degrees alone (_symmetric_tp_total)."""
    xr = a.x_raw.unsqueeze(-1) if a.x_raw.dim() == 1 else a.x_raw
    pos = xr[:, :3].to(torch.float32).contiguous()
    n, ng, gptr = g.n, g.node_graph, g.gptr
    sign = torch.where(pos[:, 0] > 40.0, -torch.ones_like(pos[:, 0]), torch.ones_like(pos[:, 0])).contiguous()
    flag = _flag(g, ing)
    gptr_g = radius_count(pos, ng, gptr, a.cutoff_g, a.max_nb, flag)
    local = a.cutoff_l <= a.cutoff_g
    r = _Lists(pos, _Sizes(flag, a.sizes if local else None))
    sz, r.sign = r.sz, sign
    fill_nb = a.max_nb
    if local:
        lp = radius_count(pos, ng, gptr, a.cutoff_l)
    if sz.known is not None:
        total_g, total_l, r.tp_hint = sz.known
        sz.reserve(3 * total_g + 3 * total_l + 5 * r.tp_hint + 64, pos.device)
        gptr_g, lp = sz.expect(gptr_g, total_g), sz.expect(lp, total_l)
        fill_nb = 0                               # (a cap that binds is flagged by the count pass, the batch invalid: see raise_for_flag)
    elif local:
        (total_g, total_l, tp_total), r.capped = sz.read(gptr_g[-1], lp[-1], _symmetric_tp_total(lp, a.with_triplets),
                                                         allow=CAP_BIT)
        r.tp_hint = None if r.capped else tp_total
    else:                                         # (a local cutoff above the global one: the general, dependent order)
        (total_g,), r.capped = sz.read(gptr_g[-1], allow=CAP_BIT)
    rows = [] if local else None
    r.gp, r.gn, r.gd = radius_fill(pos, ng, gptr, a.cutoff_g, gptr_g, total_g, zeroed=sz.arena, rows_out=rows,
                                   max_neighbors=fill_nb)
    if local and not r.capped:
        r.lp, r.l_src, r.l_dist = _filter_fill(r.gp, r.gn, r.gd, a.cutoff_l, lp, total_l, zeroed=sz.arena)
    else:                  # a cut of the filled global graph, sized by a read-back of its own (models.py:131-134): the degrees of
        r.lp, r.l_src, r.l_dist = csr_filter(r.gp, r.gn, r.gd, a.cutoff_l)        # a CAPPED graph's cut are not the radius degrees
    r.g_rows = rows.pop() if rows else None
    r.loc_radius = not r.capped
    if r.capped:
        # (query, neighbour) lists, as the RNA kNN cuts: the local layer aggregates at the neighbour
        # (local_message_passing.py:39,54), the global one too unless flow = target_to_source
        r.lp, r.l_src, r.l_dist, r.loc_inv = _transpose_edges(r.lp, r.l_src, r.l_dist, n, want_inverse=a.need_grad)
        if a.flow != 'target_to_source':
            r.global_by_neighbour(n, a.need_grad)
        r.g_rows = None                           # (a capped list's row ids only ever serve as that transposition's queries)
    r.l_dst = expand_rows(r.lp, r.l_src.numel(), zeroed=sz.arena)
    return r


def _rna(g, ing, a):
    """The kNN graph with both its cuts, models.py:147-150 (global) and 153-156 (local: j = query, i = nbr)."""
    xr = a.x_raw.unsqueeze(-1) if a.x_raw.dim() == 1 else a.x_raw
    pos = xr[:, :3].to(torch.float32).contiguous()
    n, ng, gptr = g.n, g.node_graph, g.gptr
    flag = _flag(g, ing, xr[:, -1], a.n_types)
    r = _Lists(pos, _Sizes(flag, a.sizes))
    sz = r.sz
    gq = qq = None                                # query ids of the entries, when the launch that wrote the lists gave them
    if sz.known is not None:
        kp, kn, kd = knn_table(pos, ng, gptr, a.knn_k, float('inf'))             # (query, neighbour) rows, self dropped
        total_g, total_l, r.tp_hint = sz.known
        pa, pb = _filter_count(kp, kn, kd, a.cutoff_g), _filter_count(kp, kn, kd, a.cutoff_l)
        sz.reserve(4 * total_g + 4 * total_l + 5 * r.tp_hint + 64, pos.device)
        pa, pb = sz.expect(pa, total_g), sz.expect(pb, total_l)
        r.gp, r.gn, r.gd = _filter_fill(kp, kn, kd, a.cutoff_g, pa, total_g, zeroed=sz.arena)
        qp, qn, qd = _filter_fill(kp, kn, kd, a.cutoff_l, pb, total_l, zeroed=sz.arena)
    elif n > 0 and a.knn_k <= 64:                 # one search, both cuts, one host round trip
        if KNN_TP_TOTAL:                          # ... and the triplet / pair total of the local cut with them
            (r.gp, r.gn, r.gd, gq), (qp, qn, qd, qq), r.tp_hint = knn_cuts(pos, ng, gptr, a.knn_k, a.cutoff_g, a.cutoff_l, flag,
                                                                           tp_of_b=bool(a.with_triplets))
        else:
            (r.gp, r.gn, r.gd, gq), (qp, qn, qd, qq) = knn_cuts(pos, ng, gptr, a.knn_k, a.cutoff_g, a.cutoff_l, flag)
    else:
        kp, kn, kd = knn_table(pos, ng, gptr, a.knn_k, float('inf'))
        (r.gp, r.gn, r.gd), (qp, qn, qd) = csr_filter2(kp, kn, kd, a.cutoff_g, a.cutoff_l, flag)
    r.g_rows = gq                                 # rows = queries: the expanded row ids are the query ids
    if a.flow != 'target_to_source':              # aggregate at edge_index[1] = neighbour
        r.global_by_neighbour(n, a.need_grad, zeroed=sz.arena)
    # (the local layer always aggregates at i)
    r.lp, r.l_src, r.l_dist, r.loc_inv = _transpose_edges(qp, qn, qd, n, zeroed=sz.arena, want_inverse=a.need_grad, q=qq)
    r.l_dst = expand_rows(r.lp, r.l_src.numel(), zeroed=sz.arena)
    return r


def _finish(g, r, dataset, a):
    """The common tail: the CSR objects of the lists `r`, the triplet / pair rows with their angles (models.py:68-98,
    165-177; combined rows grouped by target edge), the deferred size check and the backward's transposed lists."""
    sz, pos, n, dev = r.sz, r.pos, g.n, r.pos.device
    zeroed = sz.arena
    g.pos, g.sign, g.capped = pos, r.sign, r.capped
    if r.cell_tab is not None:
        g.cell_tab = r.cell_tab
    if r.img_g is not None:
        g.img_g = r.img_g
    if sz.known is not None:
        g.check = sz.flag
    if r.loops is not None:
        g.loops = r.loops
    if r.all_kept is not None:
        g.all_kept = r.all_kept
    g.glob = CSR(r.gp, r.g_rows if r.g_rows is not None else expand_rows(r.gp, r.gn.numel(), zeroed=zeroed), r.gn)
    g.dist_g = r.gd
    g.loc = CSR(r.lp, r.l_dst, r.l_src)
    g.dist_l = r.l_dist
    e_l = g.loc.m
    wt = 1 if a.with_triplets else 0
    tp_ptr, tot, tcount = r.tp_ptr, r.tp_total, r.tcount
    if tp_ptr is None:
        tp_ptr, tcount = _triplet_ptr(r.lp, r.l_src, r.l_dst, a.with_triplets)
        tot = r.tp_hint if r.tp_hint is not None else int(tp_ptr[-1])
        if zeroed:
            tp_ptr = sz.expect(tp_ptr, tot)
    tp_idx, tp_edge, tp_kind = (_alloc_i32(tot, dev, zeroed) for _ in range(3))
    tp_angle = _alloc_f32(tot, dev, zeroed)
    _call_in_cell('pamnet_triplet_fill_f32', 'pamnet_triplet_fill_pbc_f32', pos,
                  None if r.cell_tab is None else (r.cell_tab, g.node_graph), lib.ptr(r.lp), lib.ptr(r.l_src), lib.ptr(r.l_dst),
                  e_l, wt, lib.ptr(tp_ptr), lib.ptr(tp_idx), lib.ptr(tp_edge), lib.ptr(tp_angle), lib.ptr(tp_kind), tot,
                  lib.stream_of(pos))
    if sz.checks:                                 # one launch: size mismatches join the validity flag (PAMNet.verify)
        _check_sizes(sz.flag, sz.checks, r.all_kept, r.loops)
    g.tp = CSR(tp_ptr, tp_edge, tp_idx)           # rows = target edge e, col = source edge e'
    g.tp_angle, g.tp_kind = tp_angle, tp_kind
    g.glob_T = g.loc_T = g.tp_T = _NoTranspose    # forward-only: backward index structures are not built
    if a.need_grad:
        # d x[j] of the global gather: the reverse-edge index of a radius graph (symmetric by construction, unless the
        # neighbour cap cut it); for a list stored by neighbour the inverse of that transposition; a counting sort otherwise
        # -- but for the all-image multigraph, whose rows repeat columns: the counting sort of its columns.  (It is symmetric
        # as a multiset, so its rows aggregate at the neighbour as they stand: never stored by neighbour.)
        radius_g = dataset in ('QM9', 'PDBbind') and not r.capped and r.img_g is None
        g.glob_T = SymmetricTranspose(g.glob) if radius_g else (r.glob_inv if r.glob_inv is not None
                                                               else Transpose(g.glob.col, n))
        # d x[j] of the local gather: a radius graph for PDBbind and bond-free QM9, the inverse transposition for RNA;
        # user-supplied bonds (QM9) take the counting sort
        g.loc_T = SymmetricTranspose(g.loc) if r.loc_radius else (r.loc_inv if r.loc_inv is not None
                                                                  else Transpose(g.loc.col, n))
        # d m_neighbor[e'] of the triplet/pair gather
        g.tp_T = (TripletTranspose(g.loc, g.loc_T, tp_ptr, tcount, tot, a.with_triplets, zeroed=zeroed)
                  if (e_l > 0 and tot > 0) else Transpose(tp_idx, max(e_l, 1)))


def build_graph(dataset, cutoff_l, cutoff_g, flow, x_raw, batch, pos=None, edge_index=None, num_graphs=None,
                need_grad=True, knn_k=None, with_triplets=True, n_types=None, sizes=None, default_basis=True, mol_local=None,
                max_num_neighbors=None, aux_tables=True, cell=None, strain=None, cell_images=None, pbc=None):
    """Graph-construction part of PAMNet.forward (models.py:104-177).  Returns a Graph.

    `cell` (QM9 schema, bond-free, no `sizes`): fp32 [num_graphs, 3, 3] on the device, row k of cell[g] = lattice vector a_k of
    graph g.  Every displacement between two atoms of a graph is then the minimum-image one (csrc/geom_core.h min_image): both
    radius searches, the bond lengths, both angle kinds and the position backward.  Positions need not be wrapped.  Each cell
    must be non-singular with all three perpendicular heights above 2 * max(cutoff_l, cutoff_g) (ValueError otherwise, with the
    sizes' round trip).  mol_local=None (the default) and False take the step-by-step launches; mol_local=True takes the periodic
    form of the molecule-local builder (cell table, count launch, one round trip, fill launch: the same arrays bit for bit) and
    falls through to the step-by-step launches when a cell turns out to hold over MOL_ATOMS atoms or MOL_BONDS directed local edges.

    `cell_images` (periodic batches): None / 'minimum' = the above.  'all': the GLOBAL graph holds every image within cutoff_g --
    row i every (atom j, integer triple n) with |pos_i - pos_j - n @ cell| <= cutoff_g, i's own images included, ascending (j, n),
    the triple of every edge in g.img_g -- while the local graph stays the minimum-image one.  The cells then need heights above
    2 * cutoff_l only (and not below cutoff_g / 4).  max_num_neighbors cuts no row of that graph: a cap that binds is a
    ValueError.  Always the step-by-step launches, whatever `mol_local` says: the rows of that multigraph repeat columns and may
    hold more than 64 entries, which the builder's adjacency masks (one bit per atom of the cell) cannot express.

    `pbc` (periodic batches): a torch.bool tensor [num_graphs, 3] on the device, or three Python bools for every graph --
    pbc[g, k]: graph g repeats along cell[g, k].  None or (True, True, True): the above, by the same entry points.  Along an open
    axis the user's vector is not used (it may be zero, short or make the matrix singular), no displacement is wrapped, no height
    condition applies and the all-image search tries no image (img_g[:, k] == 0); a graph with three open axes is an isolated
    molecule whose arrays are bit for bit those of the open-space build.  The height conditions hold for the periodic axes, in
    the lattice those axes span (cell_table).  Only the cell table and the image box are made differently; every kernel that
    reads them is the fully periodic one.

    `strain` (periodic batches): the tensor that names the variable of the virial (differentiable_geometry) -- fp32 zeros
    [num_graphs, 3, 3] on the device.  Only validated here; its count of non-zero entries rides in the sizes' round trip.

    `sizes`: (global edges, local edges, triplet + pair rows) of this batch as host integers -- what a batch collated by
    pamnet_amd.store.MoleculeStore carries.  With them no value is read back from the device: buffers are sized from
    the host numbers, the fills are capped by them, and one launch compares them with the device-side counts (and
    folds in the input-validity flag); the result waits in `g.check` (an int32 device scalar) for the caller's next
    synchronisation (PAMNet.verify).  Without them: one host round trip for the sizes and the flag.

    `edge_index` None (QM9 schema): bond-free molecules -- the local graph is the radius graph at cutoff_l inside every molecule
    (self excluded, no neighbour cap), stored by target, then source.

    `mol_local` (QM9 schema): True = the caller vouches that every molecule is within the molecule-local builder's limits
    (MOL_ATOMS / MOL_BONDS) with its bonds grouped by molecule (a resident store knows); None = try it when the
    average molecule is small (a batch that does not qualify is found out with the sizes' round trip and takes the
    step-by-step launches); False = never.

    `max_num_neighbors`: the cap of the reference's radius searches (models.py:110,128: 1000; :301: 500; None = no cap).  It
    binds only in graphs with more than that many nodes within cutoff_g of one node; the count pass notes it in the flag
    word, and such a batch is built with the capped -- no longer symmetric -- global graph and general transposes (plain
    tensors), or flagged (a batch carrying `sizes`: the one-call graph assumes symmetric radius graphs).

    `aux_tables`: also make what only the dim = 128 layer engine reads (the node-aligned work split of its fused global-edge
    kernels, the two index hops of its local aggregation's backward); a model of a narrow width passes False."""
    n_graphs = None if num_graphs is None else int(num_graphs)
    if cell is not None:                          # (before anything is built: every refusal of a periodic batch)
        if n_graphs is None:
            n_graphs = int(batch[-1]) + 1
        cell = _checked_cell(cell, dataset, edge_index, sizes, n_graphs, pos)
    all_images = _checked_cell_images(cell_images, cell)
    pbc = _checked_pbc(pbc, cell, n_graphs, pos)
    strain_nz = None if strain is None else _checked_strain(strain, cell, n_graphs, pos)
    max_nb = int(max_num_neighbors or 0)
    knn_k = KNN_K if knn_k is None else int(knn_k)
    if sizes is not None and knn_k != KNN_K:
        raise ValueError('host-side sizes (store.MoleculeStore) are counted for k = %d neighbours; got knn_k = %d' % (KNN_K, knn_k))
    if sizes is not None and num_graphs is not None:
        eng = _engine_graph(dataset, cutoff_l, cutoff_g, flow, x_raw, batch, pos, edge_index, n_graphs, need_grad, knn_k,
                            with_triplets, n_types, sizes, default_basis, mol_local=bool(mol_local), max_nb=max_nb,
                            aux_tables=aux_tables)
        if eng is not None:
            return eng
    g = Graph()
    g.sign = g.check = None                       # (check: device flag word of the zero-host-sync path, see `sizes`)
    n = g.n = int(batch.numel())
    g.n_graphs = n_graphs if n_graphs is not None else int(batch[-1]) + 1
    rna = dataset[:3].lower() == 'rna'
    ing = None
    if batch.is_cuda and n > 0:
        if dataset == 'QM9':
            if n_types is not None:               # (edge_index None: the bond-free batch, validated without edges)
                ing = ingest(batch, g.n_graphs, x_raw, n_types, edge_index)
        elif rna and n_types is not None and x_raw.dim() == 2:                  # the type id is x's last column
            ing = ingest(batch, g.n_graphs, x_raw[:, -1], n_types)
        elif rna or dataset == 'PDBbind':
            ing = ingest(batch, g.n_graphs)
    if ing is not None:                           # (types: int32 atom types, QM9 / RNA, a by-product of the ingest launch)
        g.node_graph, g.gptr, g.types = ing.node_graph, ing.gptr, ing.types
    else:
        g.node_graph, g.types = batch.to(I32).contiguous(), None
        g.gptr, _ = csr_from_keys(g.node_graph, g.n_graphs)
    lists = _rna if rna else {'QM9': _qm9_bond_free if edge_index is None else _qm9_bonded, 'PDBbind': _pdbbind}.get(dataset)
    if lists is None:
        raise ValueError("Invalid dataset. If you are using any dataset related to RNA 3D structure prediction, "
                         "be sure to use 'rna' as the first 3 characters of the dataset name.")
    a = _Args(cutoff_l, cutoff_g, flow, x_raw, pos, edge_index, need_grad, knn_k, with_triplets, n_types, sizes, mol_local,
              max_nb, cell, strain_nz, all_images, pbc)
    r = lists(g, ing, a)
    if r is not None:                             # (None: the molecule-local builder has made everything)
        _finish(g, r, dataset, a)
    return _with_seg_cuts(g, dataset) if aux_tables else g


def _with_seg_cuts(g, dataset):
    """The node-aligned work split of the fused global-edge kernels (csrc/edge_agg.hip), made WITH the graph -- one small launch
    on the stream that builds it (the input pipeline's side stream) instead of one per direction on the main stream inside the
    layer-stack calls.  The one-call graph engine does the same (field CUTS)."""
    if dataset in ('QM9', 'PDBbind') and g.n > 0:
        g.seg_cuts = _i32(260, g.glob.ptr.device)
        lib.call('pamnet_seg_cuts_i32', lib.ptr(g.glob.ptr), lib.ptr(g.glob.row_of), g.n, g.glob.m, lib.ptr(g.seg_cuts), None,
                 lib.stream_of(g.glob.ptr))
        # the local aggregation's backward gathers through tT_perm -> t_row -> l_row (pamnet_local_agg_bwd_f32): both hops once
        # per graph, with the graph
        if g.tp_T is not _NoTranspose and g.tp.m > 0 and g.loc.m > 0:
            dev = g.glob.ptr.device
            g.tT_edge, g.tT_node = _i32(g.tp.m, dev), _i32(g.tp.m, dev)
            lib.call('pamnet_triplet_transpose_aux_i32', lib.ptr(g.tp_T.perm), lib.ptr(g.tp.row_of), lib.ptr(g.loc.row_of), g.tp.m,
                     lib.ptr(g.tT_edge), lib.ptr(g.tT_node), lib.stream_of(g.glob.ptr))
    return g


def spherical_basis_tab(g, cutoff_l, num_spherical, num_radial, envelope_exponent, zeros, norm):
    """SphericalBasisLayer for any (num_spherical, num_radial, envelope_exponent) (layers/basic.py:79-116): zeros (float32)
    / norm (float64) are the model's device tables (models.SphericalBasis).  Returns [T+P, num_spherical * num_radial]."""
    dev = g.pos.device
    st = lib.stream_of(g.pos)
    e_l, tot, w = g.loc.m, g.tp.m, int(num_spherical) * int(num_radial)
    # the kernels read the tables through raw pointers: element types, sizes and residence are checked here
    if not (zeros.dtype == torch.float32 and norm.dtype == torch.float64 and zeros.numel() == w and norm.numel() == w
            and zeros.device == dev and norm.device == dev):
        raise TypeError('spherical basis tables: zeros must be float32 [%d], norm float64 [%d], both on %s (got %s %s on %s, '
                        '%s %s on %s)' % (w, w, dev, zeros.dtype, tuple(zeros.shape), zeros.device, norm.dtype,
                                          tuple(norm.shape), norm.device))
    rad = _f32(e_l * w, dev)
    lib.call('pamnet_sbf_radial_tab_f32', lib.ptr(g.dist_l), float(cutoff_l), e_l, int(num_spherical), int(num_radial),
             int(envelope_exponent), lib.ptr(zeros), lib.ptr(norm), lib.ptr(rad), st)
    sbf = torch.empty((tot, w), dtype=torch.float32, device=dev)
    lib.call('pamnet_sbf_combine_tab_f32', lib.ptr(rad), lib.ptr(g.tp.col), lib.ptr(g.tp_angle), tot, int(num_spherical),
             int(num_radial), lib.ptr(sbf), st)
    return sbf


def spherical_basis(g, cutoff_l):
    """SphericalBasisLayer on the combined triplet/pair rows (layers/basic.py:107-116): returns [T+P, 42]."""
    if getattr(g, '_sbf_cutoff', None) == float(cutoff_l) and g.__dict__.get('sbf') is not None:
        return g.sbf                                  # built by the graph-construction engine in the same call
    dev = g.pos.device
    st = lib.stream_of(g.pos)
    e_l = g.loc.m
    rad = _f32(e_l * 42, dev)
    lib.call('pamnet_sbf_radial_f32', lib.ptr(g.dist_l), float(cutoff_l), e_l, lib.ptr(rad), st)
    tot = g.tp.m
    sbf = torch.empty((tot, 42), dtype=torch.float32, device=dev)
    lib.call('pamnet_sbf_combine_f32', lib.ptr(rad), lib.ptr(g.tp.col), lib.ptr(g.tp_angle), tot, lib.ptr(sbf), st)
    return sbf


# ---- differentiable geometry: forces (d prediction / d positions) ------------------------------------------------------
_SECOND_ORDER = ('PAMNet: second derivatives through the positions are not supported (the kernels\' backward passes are not '
                 'themselves differentiable): torch.autograd.grad(..., create_graph=True) cannot give forces with a grad_fn')


def _index_lists(g):
    """The index tensors of `g` that pamnet_pos_bwd_f32 reads, with the sizes.  The geometry Functions keep these on ctx, not
    the graph: the graph object is where their outputs end up, and ctx -> graph -> output -> node would be a cycle."""
    glob, loc, tp = g.glob, g.loc, g.tp
    return (g.n, (glob.ptr, glob.row_of, glob.col, g.glob_T.ptr, g.glob_T.perm), glob.m,
            (loc.ptr, loc.row_of, loc.col, g.loc_T.ptr, g.loc_T.perm), loc.m,
            (tp.ptr, tp.row_of, tp.col, g.tp_kind, g.tp_T.ptr, g.tp_T.perm), tp.m)


class _Geometry(torch.autograd.Function):
    """pos [N, 3] (, strain [G, 3, 3] of zeros, periodic graphs) -> (dist_g, dist_l, tp_angle) of a graph built from these
    positions (models.py:62-66,165-177).  The forward hands out the values graph construction already computed; the backward is
    pamnet_pos_bwd_f32 -- or, when the gradient with respect to the strain is asked for, pamnet_pos_bwd_pbc_virial_f32, which
    writes the same dpos and the virial of every graph; a graph with an all-image global list (g.img_g) takes the *_img_* forms.
    Everything the backward reads is kept (pos through save_for_backward, so an in-place change of it is caught): a graph that is
    retained can be walked again."""

    @staticmethod
    def forward(ctx, pos, strain, g):
        ctx.save_for_backward(pos)
        ctx.idx = _index_lists(g)
        ctx.pbc = None if g.cell_tab is None else (g.cell_tab, g.node_graph)      # periodic graph: the image rule's inputs
        ctx.img = g.img_g                                                          # all-image global list: its edges' images
        ctx.graphs = None if strain is None else (g.gptr, int(g.n_graphs))        # what the virial's reduction reads
        return g.dist_g.clone(), g.dist_l.clone(), g.tp_angle.clone()

    @staticmethod
    def backward(ctx, d_dg, d_dl, d_ang):
        if torch.is_grad_enabled():
            raise RuntimeError(_SECOND_ORDER)
        pos, = ctx.saved_tensors
        n, glob, eg, loc, el, trip, tp = ctx.idx      # (each list: ptr, row, col, [kind,] transposed ptr, perm)
        pos = pos.contiguous()
        d_dg, d_dl, d_ang = d_dg.contiguous(), d_dl.contiguous(), d_ang.contiguous()
        work = torch.empty(3 * max(el, 1), dtype=torch.float64, device=pos.device)
        dpos = torch.empty((n, 3), dtype=torch.float32, device=pos.device)
        P = lib.ptr
        img = ctx.img is not None
        if img:                                       # (the *_img_* forms: g_img behind g_col)
            glob = glob[:3] + (ctx.img,) + glob[3:]
        if not (ctx.graphs is not None and ctx.needs_input_grad[1]):
            _call_in_cell('pamnet_pos_bwd_f32', 'pamnet_pos_bwd_img_f32' if img else 'pamnet_pos_bwd_pbc_f32', pos, ctx.pbc, n,
                          *map(P, glob), P(d_dg), eg, *map(P, loc), P(d_dl), el, *map(P, trip), P(d_ang), tp, P(work), P(dpos),
                          lib.stream_of(pos))
            return dpos, None, None
        gptr, n_graphs = ctx.graphs
        atom_work = torch.empty(9 * max(n, 1), dtype=torch.float64, device=pos.device)
        dstrain = torch.empty((max(n_graphs, 1), 9), dtype=torch.float32, device=pos.device)[:n_graphs]
        lib.call('pamnet_pos_bwd_img_virial_f32' if img else 'pamnet_pos_bwd_pbc_virial_f32', P(pos), *map(P, ctx.pbc), n,
                 *map(P, glob), P(d_dg), eg, *map(P, loc), P(d_dl), el, *map(P, trip), P(d_ang), tp, P(work), P(dpos), P(gptr),
                 n_graphs, P(atom_work), P(dstrain), lib.stream_of(pos))
        return (dpos if ctx.needs_input_grad[0] else None), dstrain.view(n_graphs, 3, 3), None


class _SphericalBasis(torch.autograd.Function):
    """(dist_l, tp_angle) -> the default spherical basis rows [T+P, 42] (layers/basic.py:107-116).  The forward hands out
    the rows graph construction / spherical_basis already formed; the backward is pamnet_sbf_bwd_f32 (inputs through
    save_for_backward, index lists on ctx: see _Geometry)."""

    @staticmethod
    def forward(ctx, dist_l, angle, g, cutoff_l, sbf):
        ctx.save_for_backward(dist_l, angle)
        ctx.idx = (g.tp.col, g.tp_T.ptr, g.tp_T.perm, g.loc.m, g.tp.m)
        ctx.cutoff = float(cutoff_l)
        return sbf.clone()

    @staticmethod
    def backward(ctx, gs):
        if torch.is_grad_enabled():
            raise RuntimeError(_SECOND_ORDER)
        dist_l, angle = ctx.saved_tensors
        t_col, tt_ptr, tt_perm, e_l, tot = ctx.idx
        gs = gs.contiguous()
        rad = torch.empty(max(e_l, 1) * 42, dtype=torch.float32, device=gs.device)
        dangle, ddist = torch.empty_like(angle), torch.empty_like(dist_l)
        lib.call('pamnet_sbf_bwd_f32', lib.ptr(gs), lib.ptr(dist_l), ctx.cutoff, e_l, lib.ptr(t_col), lib.ptr(angle), tot,
                 lib.ptr(tt_ptr), lib.ptr(tt_perm), lib.ptr(rad), lib.ptr(dangle), lib.ptr(ddist), lib.stream_of(gs))
        return ddist, dangle, None, None, None


class _DiffGraph(object):
    """Graph `g` seen with its geometry replaced by differentiable tensors (differentiable_geometry); every other attribute
    is g's own.  g itself keeps the plain tensors, so what caches it (models: the inspection hooks) holds no autograd
    graph."""

    pos_grad = True

    def __init__(self, g, **geometry):
        self.__dict__.update(geometry)
        self.__dict__['_plain'] = g

    def __getattr__(self, name):
        return getattr(self.__dict__['_plain'], name)


def differentiable_geometry(g, pos, cutoff_l, strain=None):
    """Graph `g` (built from `pos`, fp32 [N, 3], with the backward index lists: need_grad) seen with its geometry linked to
    `pos`: dist_g, dist_l, tp_angle and the default-basis rows sbf are outputs of autograd Functions whose backward passes
    are HIP kernels.  Values are unchanged (the same tensors' contents); `g` itself is not modified.

    `strain` (a periodic graph; fp32 zeros [num_graphs, 3, 3], validated by build_graph(strain=)): the geometry is linked to it
    as well.  Its gradient is the virial per cell, W[g][a][b] = sum over the directed global edges and local bonds of graph g of
    v_e[a] * (dE / dv_e)[b] with v_e the minimum-image vector: the derivative under pos -> pos @ (I + eps_g), cell[g] -> cell[g]
    @ (I + eps_g) at eps = 0, image integers held fixed.  Sign, volume, symmetrisation and Voigt order are the caller's."""
    if g.glob_T is _NoTranspose or g.loc_T is _NoTranspose or g.tp_T is _NoTranspose:
        raise RuntimeError('differentiable geometry needs a graph built with need_grad=True')
    if strain is not None and g.cell_tab is None:
        raise ValueError('`strain` belongs to periodic graphs (build_graph(cell=)): this graph was built in open space')
    dist_g, dist_l, angle = _Geometry.apply(pos, strain, g)
    sbf = _SphericalBasis.apply(dist_l, angle, g, cutoff_l, g.sbf)
    return _DiffGraph(g, dist_g=dist_g, dist_l=dist_l, tp_angle=angle, sbf=sbf)
