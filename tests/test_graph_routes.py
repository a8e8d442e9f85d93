"""Every route through pamnet_amd.graph.build_graph, in one place: for each kind of input the library calls one build makes
(symbols, in order), its host synchronisations, whether the neighbour cap bound, and the classes of the three backward
transposes.  The expected values (ROUTES) were recorded with `observe` below at the commit before build_graph became a
dispatcher over per-schema list builders: a change of the host orchestration that adds a launch, reorders two, or adds a
read-back shows up here as a diff of one row.  (What the arrays hold is pinned elsewhere: tests/test_hip_kernels.py,
test_graph_engine.py, test_bondfree.py, test_pbc.py.)"""
import warnings

import pytest
import torch

from graph_cases import case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs an MI355X'
    from pamnet_amd import lib
    lib.load()
    return torch.device('cuda:0')


# name -> (batch of graph_cases.case, changes to the batch, keywords of build_graph beyond the case's own, module switches)
# changes: 'free' = no edge_index; 'loop' = one (0, 0) bond appended; 'view' = `batch` as a strided view; 'cell' = a cube of
# edge 12 > 2 * 5 per graph; 'sizes' = the three totals of the batch, as a store hands them over
CASES = {
    'qm9_builder':          ('qm9', (), dict(), {}),
    'qm9_builder_fwd_only': ('qm9', (), dict(need_grad=False), {}),
    'qm9_steps':            ('qm9', (), dict(mol_local=False), {}),
    'qm9_steps_pairs_only': ('qm9', (), dict(mol_local=False, with_triplets=False), {}),
    'qm9_sizes':            ('qm9', ('sizes',), dict(), {'ENGINE': False}),
    'qm9_self_loop_redo':   ('qm9_ragged', ('loop',), dict(mol_local=False), {}),
    'qm9_capped_s2t':       ('qm9', (), dict(max_num_neighbors=4), {}),
    'qm9_capped_t2s':       ('qm9', (), dict(max_num_neighbors=4, flow='target_to_source'), {}),
    'qm9_free_builder':     ('qm9', ('free',), dict(cutoff_l=1.7), {}),
    'qm9_free_declined':    ('qm9', ('free',), dict(), {}),       # (over 256 local edges per molecule at cutoff_l = 5)
    'qm9_free_steps':       ('qm9', ('free',), dict(mol_local=False), {}),
    'qm9_free_sizes':       ('qm9', ('free', 'sizes'), dict(), {}),
    'qm9_free_wide_local':  ('qm9', ('free',), dict(cutoff_l=5.0, cutoff_g=3.0), {}),
    'qm9_free_cell':        ('qm9', ('free', 'cell'), dict(), {}),
    'qm9_strided_batch':    ('qm9', ('view',), dict(), {}),
    'pdbbind':              ('pdbbind', (), dict(), {}),
    'pdbbind_sizes':        ('pdbbind', ('sizes',), dict(), {'ENGINE': False}),
    'pdbbind_wide_local':   ('pdbbind', (), dict(cutoff_l=7.0), {}),
    'pdbbind_capped_s2t':   ('pdbbind', (), dict(max_num_neighbors=8), {}),
    'pdbbind_capped_t2s':   ('pdbbind', (), dict(max_num_neighbors=8, flow='target_to_source'), {}),
    'rna_s2t':              ('rna_s2t', (), dict(), {}),
    'rna_t2s':              ('rna_t2s', (), dict(), {}),
    'rna_sizes':            ('rna_s2t', ('sizes',), dict(), {'ENGINE': False}),
    'rna_k65':              ('rna_s2t', (), dict(knn_k=65), {}),
    'rna_tp_total':         ('rna_s2t', (), dict(), {'KNN_TP_TOTAL': True}),
}
MUST_CAP = ('qm9_capped_s2t', 'qm9_capped_t2s', 'pdbbind_capped_s2t', 'pdbbind_capped_t2s')
BUILDER = ('qm9_builder', 'qm9_builder_fwd_only', 'qm9_free_builder')         # the molecule-local builder makes the graph


def _call(G, b, kw):
    kw = dict(kw)
    return G.build_graph(kw.pop('dataset'), kw.pop('cutoff_l'), kw.pop('cutoff_g'), kw.pop('flow'), b.x, b.batch,
                         getattr(b, 'pos', None), getattr(b, 'edge_index', None), num_graphs=b.num_graphs, **kw)


SYNC_SITES = []                                   # (file, line) of the last observed call's host synchronisations


def observe(G, name, dev):
    """One build_graph call of `G` (the graph module) on case `name`: (the route record, the graph).  A call that raises is
    recorded with the exception's class and message in place of the graph's properties (and None for the graph)."""
    from pamnet_amd import lib, synth
    kind, changes, extra, switches = CASES[name]
    b, kw = case(kind, dev)
    kw = dict(kw, **extra)
    if 'free' in changes:
        b = synth.Batch(**{k: v for k, v in b.__dict__.items() if k != 'edge_index'})
    if 'loop' in changes:
        b.edge_index = torch.cat([b.edge_index, torch.zeros((2, 1), dtype=b.edge_index.dtype, device=dev)], 1).contiguous()
    if 'view' in changes:
        b.batch = torch.stack([b.batch, b.batch], 1)[:, 0]
        assert not b.batch.is_contiguous()
    if 'cell' in changes:
        kw['cell'] = (12.0 * torch.eye(3, device=dev)).expand(b.num_graphs, 3, 3).contiguous()
    if 'sizes' in changes:
        ref = _call(G, b, kw)
        kw['sizes'] = (ref.glob.m, ref.loc.m, ref.tp.m)
    saved = {k: getattr(G, k) for k in switches}
    calls, real = [], lib.call

    def rec(sym, *args):
        calls.append(sym)
        return real(sym, *args)
    torch.cuda.synchronize()
    try:
        for k, v in switches.items():
            setattr(G, k, v)
        lib.call = rec
        torch.cuda.set_sync_debug_mode('warn')
        try:
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter('always')
                try:
                    g, outcome = _call(G, b, kw), None
                except Exception as e:            # noqa: BLE001  (recorded, compared by the caller)
                    g, outcome = None, (type(e).__name__, str(e))
        finally:
            torch.cuda.set_sync_debug_mode('default')
    finally:
        lib.call = real
        for k, v in saved.items():
            setattr(G, k, v)
    SYNC_SITES[:] = [(w.filename, w.lineno) for w in caught if 'synchroniz' in str(w.message)]
    short = ' '.join(c[len('pamnet_'):] if c.startswith('pamnet_') else c for c in calls)
    if outcome is None:
        outcome = (bool(g.capped), type(g.glob_T).__name__, type(g.loc_T).__name__, type(g.tp_T).__name__)
    return (short, len(SYNC_SITES)) + outcome, g


# name -> (library calls without their 'pamnet_' prefix, host synchronisations, capped, class of glob_T, loc_T, tp_T), or
# (library calls up to the one that refused, host synchronisations, exception class, message)
ROUTES = {
    'qm9_builder': (
        'ingest_indices_i32 mol_graph_count_i32 gather_scalars_i64 mol_graph_fill_i32 seg_cuts_i32 '
        'triplet_transpose_aux_i32',
        1, False, '_Given', '_Given', '_Given'),
    'qm9_builder_fwd_only': (
        'ingest_indices_i32 mol_graph_count_i32 gather_scalars_i64 mol_graph_fill_i32 seg_cuts_i32',
        1, False, '_NoTransposeT', '_NoTransposeT', '_NoTransposeT'),
    'qm9_steps': (
        'ingest_indices_i32 csr_from_keys_i32 gather2_i32 triplet_count_i32 exclusive_scan_i32 '
        'radius_count_i32 exclusive_scan_i32 gather_scalars_i64 radius_fill_i32 triplet_fill_f32 '
        'reverse_edges_i32 csr_from_keys_i32 triplet_transpose_count_i32 exclusive_scan_i32 '
        'triplet_transpose_fill_i32 seg_cuts_i32 triplet_transpose_aux_i32',
        1, False, 'SymmetricTranspose', 'Transpose', 'TripletTranspose'),
    'qm9_steps_pairs_only': (
        'ingest_indices_i32 csr_from_keys_i32 gather2_i32 triplet_count_i32 exclusive_scan_i32 '
        'radius_count_i32 exclusive_scan_i32 gather_scalars_i64 radius_fill_i32 triplet_fill_f32 '
        'reverse_edges_i32 csr_from_keys_i32 triplet_transpose_count_i32 exclusive_scan_i32 '
        'triplet_transpose_fill_i32 seg_cuts_i32 triplet_transpose_aux_i32',
        1, False, 'SymmetricTranspose', 'Transpose', 'TripletTranspose'),
    'qm9_sizes': (
        'ingest_indices_i32 csr_from_keys_i32 gather2_i32 triplet_count_i32 exclusive_scan_i32 '
        'radius_count_i32 exclusive_scan_i32 radius_fill_i32 triplet_fill_f32 check_sizes_i32 '
        'reverse_edges_i32 csr_from_keys_i32 triplet_transpose_count_i32 exclusive_scan_i32 '
        'triplet_transpose_fill_i32 seg_cuts_i32 triplet_transpose_aux_i32',
        0, False, 'SymmetricTranspose', 'Transpose', 'TripletTranspose'),
    'qm9_self_loop_redo': (
        'ingest_indices_i32 csr_from_keys_i32 gather2_i32 triplet_count_i32 exclusive_scan_i32 '
        'radius_count_i32 exclusive_scan_i32 gather_scalars_i64 csr_from_keys_i32 gather2_i32 '
        'triplet_count_i32 exclusive_scan_i32 radius_fill_i32 triplet_fill_f32 reverse_edges_i32 '
        'csr_from_keys_i32 triplet_transpose_count_i32 exclusive_scan_i32 triplet_transpose_fill_i32 '
        'seg_cuts_i32 triplet_transpose_aux_i32',
        3, False, 'SymmetricTranspose', 'Transpose', 'TripletTranspose'),
    'qm9_capped_s2t': (
        'ingest_indices_i32 csr_from_keys_i32 gather2_i32 triplet_count_i32 exclusive_scan_i32 '
        'radius_count_i32 exclusive_scan_i32 gather_scalars_i64 radius_fill_i32 csr_from_keys_i32 '
        'transpose_gather_i32 expand_rows_i32 triplet_fill_f32 csr_from_keys_i32 triplet_transpose_count_i32 '
        'exclusive_scan_i32 triplet_transpose_fill_i32 seg_cuts_i32 triplet_transpose_aux_i32',
        1, True, 'InverseTranspose', 'Transpose', 'TripletTranspose'),
    'qm9_capped_t2s': (
        'ingest_indices_i32 csr_from_keys_i32 gather2_i32 triplet_count_i32 exclusive_scan_i32 '
        'radius_count_i32 exclusive_scan_i32 gather_scalars_i64 radius_fill_i32 triplet_fill_f32 '
        'csr_from_keys_i32 csr_from_keys_i32 triplet_transpose_count_i32 exclusive_scan_i32 '
        'triplet_transpose_fill_i32 seg_cuts_i32 triplet_transpose_aux_i32',
        1, True, 'Transpose', 'Transpose', 'TripletTranspose'),
    'qm9_free_builder': (
        'ingest_indices_i32 mol_graph_free_count_i32 gather_scalars_i64 mol_graph_free_fill_i32 seg_cuts_i32 '
        'triplet_transpose_aux_i32',
        1, False, '_Given', '_Given', '_Given'),
    'qm9_free_declined': (
        'ingest_indices_i32 mol_graph_free_count_i32 gather_scalars_i64 radius_count_i32 exclusive_scan_i32 '
        'radius_count_i32 exclusive_scan_i32 gather_scalars_i64 radius_fill_i32 radius_fill_i32 '
        'triplet_count_i32 exclusive_scan_i32 triplet_fill_f32 reverse_edges_i32 reverse_edges_i32 '
        'triplet_transpose_count_i32 exclusive_scan_i32 triplet_transpose_fill_i32 seg_cuts_i32 '
        'triplet_transpose_aux_i32',
        2, False, 'SymmetricTranspose', 'SymmetricTranspose', 'TripletTranspose'),
    'qm9_free_steps': (
        'ingest_indices_i32 radius_count_i32 exclusive_scan_i32 radius_count_i32 exclusive_scan_i32 '
        'gather_scalars_i64 radius_fill_i32 radius_fill_i32 triplet_count_i32 exclusive_scan_i32 '
        'triplet_fill_f32 reverse_edges_i32 reverse_edges_i32 triplet_transpose_count_i32 exclusive_scan_i32 '
        'triplet_transpose_fill_i32 seg_cuts_i32 triplet_transpose_aux_i32',
        1, False, 'SymmetricTranspose', 'SymmetricTranspose', 'TripletTranspose'),
    'qm9_free_sizes': (
        'ingest_indices_i32 radius_count_i32 exclusive_scan_i32 radius_count_i32 exclusive_scan_i32 '
        'radius_fill_i32 radius_fill_i32 triplet_count_i32 exclusive_scan_i32 triplet_fill_f32 '
        'check_sizes_i32 reverse_edges_i32 reverse_edges_i32 triplet_transpose_count_i32 exclusive_scan_i32 '
        'triplet_transpose_fill_i32 seg_cuts_i32 triplet_transpose_aux_i32',
        0, False, 'SymmetricTranspose', 'SymmetricTranspose', 'TripletTranspose'),
    'qm9_free_wide_local': (
        'ingest_indices_i32 mol_graph_free_count_i32 gather_scalars_i64 radius_count_i32 exclusive_scan_i32 '
        'radius_count_i32 exclusive_scan_i32 gather_scalars_i64 radius_fill_i32 radius_fill_i32 '
        'triplet_count_i32 exclusive_scan_i32 triplet_fill_f32 reverse_edges_i32 reverse_edges_i32 '
        'triplet_transpose_count_i32 exclusive_scan_i32 triplet_transpose_fill_i32 seg_cuts_i32 '
        'triplet_transpose_aux_i32',
        2, False, 'SymmetricTranspose', 'SymmetricTranspose', 'TripletTranspose'),
    'qm9_free_cell': (
        'ingest_indices_i32 cell_prepare_f64 radius_pbc_count_i32 exclusive_scan_i32 radius_pbc_count_i32 '
        'exclusive_scan_i32 gather_scalars_i64 radius_pbc_fill_i32 radius_pbc_fill_i32 triplet_count_i32 '
        'exclusive_scan_i32 triplet_fill_pbc_f32 reverse_edges_i32 reverse_edges_i32 '
        'triplet_transpose_count_i32 exclusive_scan_i32 triplet_transpose_fill_i32 seg_cuts_i32 '
        'triplet_transpose_aux_i32',
        1, False, 'SymmetricTranspose', 'SymmetricTranspose', 'TripletTranspose'),
    'qm9_strided_batch': (
        'csr_from_keys_i32 csr_from_keys_i32 gather2_i32 triplet_count_i32 exclusive_scan_i32 '
        'validate_inputs_i32 radius_count_i32 exclusive_scan_i32 gather_scalars_i64 radius_fill_i32 '
        'triplet_fill_f32 reverse_edges_i32 csr_from_keys_i32 triplet_transpose_count_i32 exclusive_scan_i32 '
        'triplet_transpose_fill_i32 seg_cuts_i32 triplet_transpose_aux_i32',
        1, False, 'SymmetricTranspose', 'Transpose', 'TripletTranspose'),
    'pdbbind': (
        'ingest_indices_i32 radius_count_i32 exclusive_scan_i32 radius_count_i32 exclusive_scan_i32 '
        'gather_scalars_i64 radius_fill_i32 csr_filter_fill_i32 expand_rows_i32 triplet_count_i32 '
        'exclusive_scan_i32 triplet_fill_f32 reverse_edges_i32 reverse_edges_i32 triplet_transpose_count_i32 '
        'exclusive_scan_i32 triplet_transpose_fill_i32 seg_cuts_i32 triplet_transpose_aux_i32',
        1, False, 'SymmetricTranspose', 'SymmetricTranspose', 'TripletTranspose'),
    'pdbbind_sizes': (
        'ingest_indices_i32 radius_count_i32 exclusive_scan_i32 radius_count_i32 exclusive_scan_i32 '
        'radius_fill_i32 csr_filter_fill_i32 expand_rows_i32 triplet_count_i32 exclusive_scan_i32 '
        'triplet_fill_f32 check_sizes_i32 reverse_edges_i32 reverse_edges_i32 triplet_transpose_count_i32 '
        'exclusive_scan_i32 triplet_transpose_fill_i32 seg_cuts_i32 triplet_transpose_aux_i32',
        0, False, 'SymmetricTranspose', 'SymmetricTranspose', 'TripletTranspose'),
    'pdbbind_wide_local': (
        'ingest_indices_i32 radius_count_i32 exclusive_scan_i32 gather_scalars_i64 radius_fill_i32 '
        'csr_filter_count_i32 exclusive_scan_i32 csr_filter_fill_i32 expand_rows_i32 expand_rows_i32 '
        'triplet_count_i32 exclusive_scan_i32 triplet_fill_f32 reverse_edges_i32 reverse_edges_i32 '
        'triplet_transpose_count_i32 exclusive_scan_i32 triplet_transpose_fill_i32 seg_cuts_i32 '
        'triplet_transpose_aux_i32',
        3, False, 'SymmetricTranspose', 'SymmetricTranspose', 'TripletTranspose'),
    'pdbbind_capped_s2t': (
        'ingest_indices_i32 radius_count_i32 exclusive_scan_i32 radius_count_i32 exclusive_scan_i32 '
        'gather_scalars_i64 radius_fill_i32 csr_filter_count_i32 exclusive_scan_i32 csr_filter_fill_i32 '
        'expand_rows_i32 csr_from_keys_i32 transpose_gather_i32 csr_from_keys_i32 transpose_gather_i32 '
        'expand_rows_i32 expand_rows_i32 triplet_count_i32 exclusive_scan_i32 triplet_fill_f32 '
        'triplet_transpose_count_i32 exclusive_scan_i32 triplet_transpose_fill_i32 seg_cuts_i32 '
        'triplet_transpose_aux_i32',
        3, True, 'InverseTranspose', 'InverseTranspose', 'TripletTranspose'),
    'pdbbind_capped_t2s': (
        'ingest_indices_i32 radius_count_i32 exclusive_scan_i32 radius_count_i32 exclusive_scan_i32 '
        'gather_scalars_i64 radius_fill_i32 csr_filter_count_i32 exclusive_scan_i32 csr_filter_fill_i32 '
        'expand_rows_i32 csr_from_keys_i32 transpose_gather_i32 expand_rows_i32 expand_rows_i32 '
        'triplet_count_i32 exclusive_scan_i32 triplet_fill_f32 csr_from_keys_i32 triplet_transpose_count_i32 '
        'exclusive_scan_i32 triplet_transpose_fill_i32 seg_cuts_i32 triplet_transpose_aux_i32',
        3, True, 'Transpose', 'InverseTranspose', 'TripletTranspose'),
    'rna_s2t': (
        'ingest_indices_i32 knn_cut_i32 exclusive_scan_pair_i32 gather_scalars_i64 knn_cut_fill_i32 '
        'csr_from_keys_i32 transpose_gather_i32 csr_from_keys_i32 transpose_gather_i32 expand_rows_i32 '
        'expand_rows_i32 triplet_count_i32 exclusive_scan_i32 triplet_fill_f32 triplet_transpose_count_i32 '
        'exclusive_scan_i32 triplet_transpose_fill_i32',
        2, False, 'InverseTranspose', 'InverseTranspose', 'TripletTranspose'),
    'rna_t2s': (
        'ingest_indices_i32 knn_cut_i32 exclusive_scan_pair_i32 gather_scalars_i64 knn_cut_fill_i32 '
        'csr_from_keys_i32 transpose_gather_i32 expand_rows_i32 triplet_count_i32 exclusive_scan_i32 '
        'triplet_fill_f32 csr_from_keys_i32 triplet_transpose_count_i32 exclusive_scan_i32 '
        'triplet_transpose_fill_i32',
        2, False, 'Transpose', 'InverseTranspose', 'TripletTranspose'),
    'rna_sizes': (
        'ingest_indices_i32 knn_i32 csr_filter_count_i32 exclusive_scan_i32 csr_filter_count_i32 '
        'exclusive_scan_i32 csr_filter_fill_i32 csr_filter_fill_i32 expand_rows_i32 csr_from_keys_i32 '
        'transpose_gather_i32 expand_rows_i32 csr_from_keys_i32 transpose_gather_i32 expand_rows_i32 '
        'expand_rows_i32 triplet_count_i32 exclusive_scan_i32 triplet_fill_f32 check_sizes_i32 '
        'triplet_transpose_count_i32 exclusive_scan_i32 triplet_transpose_fill_i32',
        0, False, 'InverseTranspose', 'InverseTranspose', 'TripletTranspose'),
    'rna_k65': (
        'ingest_indices_i32 knn_i32',
        0, 'RuntimeError', 'pamnet_knn_i32 failed: PAMNET_EINVAL (bad size / unsupported width)'),
    'rna_tp_total': (
        'ingest_indices_i32 knn_cut_i32 exclusive_scan_pair_i32 knn_tp_total_i64 gather_scalars_i64 '
        'knn_cut_fill_i32 csr_from_keys_i32 transpose_gather_i32 csr_from_keys_i32 transpose_gather_i32 '
        'expand_rows_i32 expand_rows_i32 triplet_count_i32 exclusive_scan_i32 triplet_fill_f32 '
        'triplet_transpose_count_i32 exclusive_scan_i32 triplet_transpose_fill_i32',
        1, False, 'InverseTranspose', 'InverseTranspose', 'TripletTranspose'),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_route(dev, name):
    from pamnet_amd import graph as G
    got, g = observe(G, name, dev)
    torch.cuda.synchronize()
    if g is not None and g.check is not None:
        G.raise_for_flag(G.read_flags([g.check]))
    if name in MUST_CAP:
        assert g.capped
    assert (name in BUILDER) == ('mol_graph_fill_i32' in got[0] or 'mol_graph_free_fill_i32' in got[0]), got[0]
    want = ROUTES[name]
    assert got[0].split() == want[0].split(), (name, got[0])
    assert got[1:] == want[1:], (name, got[1:], want[1:], SYNC_SITES)
