"""Periodic cells on the molecule-local builder: build_graph(cell=, mol_local=True) -- csrc/graph_mol.hip mol_graph_kernel<FILL, FREE,
Periodic>, entry points pamnet_mol_graph_pbc_count/fill_i32, pamnet_amd/graph.py _mol_local_graph(cell_tab=).

The yardstick is never the builder itself: the unchanged step-by-step periodic route (mol_local=False; tests/test_pbc.py pins it
to fp64 brute force) bit for bit, and that brute force directly.  Inputs are made once on the CPU and never modified; their
preconditions are asserted in fp64 by a test that needs no GPU."""
import pytest
import torch

from test_pbc import (BOX, CUBE, TRI_A, TRI_B, _arrays, _assert_margin, _brute, _brute_lists, _heights, _record, _scatter)

NEW = ('pamnet_mol_graph_pbc_count_i32', 'pamnet_mol_graph_pbc_fill_i32')
STEPS = ('pamnet_radius_pbc_count_i32', 'pamnet_radius_pbc_fill_i32', 'pamnet_triplet_fill_pbc_f32')
PREPARE = 'pamnet_cell_prepare_f64'
CUTOFF_L, CUTOFF_G = 2.0, 5.0
COUNTS = (64, 1, 37, 2, 63, 20)                  # a full wavefront, a lone atom, odd sizes, a pair, one below the limit
CELLS = (CUBE, BOX, TRI_A, TRI_B, BOX, TRI_B)
UNWRAPPED = 2                                    # this graph's atoms are displaced by lattice vectors (unwrapped input)
SEED = 13
MOL_ATOMS, MOL_BONDS = 64, 256


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs an MI355X'
    from pamnet_amd import lib
    lib.load()
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------------------- inputs
_MADE = {}


def _cat(counts, pos, cells, gen):
    batch = torch.cat([torch.full((n,), g, dtype=torch.long) for g, n in enumerate(counts)])
    x = torch.randint(0, 5, (batch.numel(),), generator=gen).float()
    return x, batch, torch.cat(pos).float(), torch.tensor(cells, dtype=torch.float32)


def _batch6():
    """(x, batch, pos fp32, cell fp32 [6, 3, 3]): six cells of 64, 1, 37, 2, 63 and 20 atoms, minimum separation 0.8."""
    if 'six' not in _MADE:
        gen = torch.Generator().manual_seed(SEED)
        pos = [_scatter(gen, n, c, 0.8) for n, c in zip(COUNTS, CELLS)]
        shift = torch.randint(-3, 4, (COUNTS[UNWRAPPED], 3), generator=gen).double()
        assert int(shift.abs().max()) == 3
        pos[UNWRAPPED] = pos[UNWRAPPED] + shift @ torch.tensor(CELLS[UNWRAPPED], dtype=torch.float64)
        _MADE['six'] = _cat(COUNTS, pos, CELLS, gen)
    return _MADE['six']


def _batch7():
    """The same batch with a seventh cell of 65 atoms: one over the builder's limit."""
    if 'seven' not in _MADE:
        x, batch, pos, cell = _batch6()
        gen = torch.Generator().manual_seed(SEED + 1)
        extra = _scatter(gen, 65, BOX, 0.8).float()
        _MADE['seven'] = (torch.cat([x, torch.randint(0, 5, (65,), generator=gen).float()]),
                          torch.cat([batch, torch.full((65,), 6, dtype=torch.long)]), torch.cat([pos, extra]),
                          torch.cat([cell, torch.tensor([BOX], dtype=torch.float32)]))
    return _MADE['seven']


def _brute6():
    if 'brute' not in _MADE:
        x, batch, pos, cell = _batch6()
        _MADE['brute'] = _brute(pos, batch, cell)
    return _MADE['brute']


def _margin(brute, r):
    """test_pbc._assert_margin over the cells that hold a pair (a lone atom has no distance to compare)."""
    _assert_margin([b for b in brute if b[3].size(0) > 1], r)


def _local_edges(brute, r):
    """Directed local edges per cell at r (fp64 brute force)."""
    return [int((d <= r).sum()) - d.size(0) for s, v, n, d in brute]


def test_inputs_meet_their_preconditions():
    """(No GPU.)  What the GPU tests assume about the batch, in fp64 on the CPU."""
    x, batch, pos, cell = _batch6()
    brute = _brute6()
    assert [d.size(0) for s, v, n, d in brute] == list(COUNTS) and max(COUNTS) <= MOL_ATOMS
    edges = _local_edges(brute, CUTOFF_L)
    deg_g = (int((brute[0][3] <= CUTOFF_G).sum()) - 64) / 64.0
    print('directed local edges per cell', edges, 'global neighbours per atom of the 64-atom cube %.1f' % deg_g)
    assert max(edges) <= MOL_BONDS
    _margin(brute, CUTOFF_L), _margin(brute, CUTOFF_G)
    assert min(min(_heights(c)) for c in CELLS) >= 10.4
    big = [k for k, c in enumerate(COUNTS) if c >= 2]
    crossing_g = [k for k in big if bool(((brute[k][3] <= CUTOFF_G) & (brute[k][2].abs().sum(-1) > 0)).any())]
    assert 2 * len(crossing_g) >= len(big), crossing_g
    off = lambda d: ~torch.eye(d.size(0), dtype=torch.bool)
    assert any(bool(((d <= CUTOFF_L) & off(d) & (n.abs().sum(-1) > 0)).any()) for s, v, n, d in brute)
    # the fall-back cases: the 64-atom cube holds over 256 directed local edges at cutoff_l = 3.0; a cell of 65 atoms
    assert _local_edges(brute, 3.0)[0] > MOL_BONDS
    x7, batch7, pos7, cell7 = _batch7()
    assert int(torch.bincount(batch7).max()) == 65 and torch.equal(pos7[:pos.size(0)], pos)


def _build(dev, inputs, cutoff_l=CUTOFF_L, **kw):
    from pamnet_amd import graph as G
    x, batch, pos, cell = inputs
    kw.setdefault('cell', cell.to(dev))
    return G.build_graph('QM9', cutoff_l, CUTOFF_G, 'source_to_target', x.to(dev), batch.to(dev), pos.to(dev), None,
                         num_graphs=int(cell.size(0)), n_types=5, **kw)


def _assert_same_graph(ga, gb):
    xa, xb = _arrays(ga), _arrays(gb)
    assert xa.keys() == xb.keys()
    for k in xa:
        assert xa[k].dtype == xb[k].dtype and torch.equal(xa[k], xb[k]), k
    assert ga.cell_tab is not None and gb.cell_tab is not None and torch.equal(ga.cell_tab, gb.cell_tab)


# ------------------------------------------------------------------------------------------------------ 1. bit identity
@pytest.mark.gpu
@pytest.mark.parametrize('need_grad', [True, False])
@pytest.mark.parametrize('with_triplets', [True, False])
def test_builder_equals_the_step_by_step_route_and_is_taken(dev, monkeypatch, with_triplets, need_grad):
    calls = _record(monkeypatch)
    gb = _build(dev, _batch6(), mol_local=True, with_triplets=with_triplets, need_grad=need_grad)
    took = [c for c in calls if c in NEW or c in STEPS or c == PREPARE]
    assert took == [PREPARE, NEW[0], NEW[1]], calls
    del calls[:]
    gs = _build(dev, _batch6(), mol_local=False, with_triplets=with_triplets, need_grad=need_grad)
    assert not [c for c in calls if c in NEW] and [c for c in calls if c in STEPS], calls
    _assert_same_graph(gb, gs)
    assert ('glob_T.perm' in _arrays(gb)) == need_grad and gb.glob.m > 0 and gb.loc.m > 0 and gb.tp.m > 0


# ------------------------------------------------------------------------------------------------------- 2. brute force
@pytest.mark.gpu
def test_builder_lists_match_brute_force(dev):
    brute = _brute6()
    _margin(brute, CUTOFF_L), _margin(brute, CUTOFF_G)
    g = _build(dev, _batch6(), mol_local=True)
    for csr, r in ((g.glob, CUTOFF_G), (g.loc, CUTOFF_L)):
        (ptr, rows, cols, dist), _ = _brute_lists(brute, r)
        assert torch.equal(csr.ptr.cpu().long(), ptr), r
        assert torch.equal(csr.row_of.cpu().long(), rows) and torch.equal(csr.col.cpu().long(), cols), r


# --------------------------------------------------------------------------------------------------------- 3. fallbacks
@pytest.mark.gpu
@pytest.mark.parametrize('case', ['65 atoms', 'over 256 local edges'])
def test_a_cell_over_the_builders_limits_takes_the_step_by_step_route(dev, monkeypatch, case):
    inputs, cutoff_l = (_batch7(), CUTOFF_L) if case == '65 atoms' else (_batch6(), 3.0)
    calls = _record(monkeypatch)
    gb = _build(dev, inputs, cutoff_l=cutoff_l, mol_local=True)
    took = [c for c in calls if c in NEW or c in STEPS or c == PREPARE]
    assert took == [PREPARE, NEW[0], STEPS[0], STEPS[0], STEPS[1], STEPS[1], STEPS[2]], calls       # the table is made once
    gs = _build(dev, inputs, cutoff_l=cutoff_l, mol_local=False)
    _assert_same_graph(gb, gs)


@pytest.mark.gpu
def test_all_images_stay_step_by_step(dev, monkeypatch):
    calls = _record(monkeypatch)
    g = _build(dev, _batch6(), mol_local=True, cell_images='all')
    assert g.img_g is not None and not [c for c in calls if c in NEW], calls


# ---------------------------------------------------------------------------------------------------------- 4. refusals
@pytest.mark.gpu
def test_refusals_on_the_builder_route(dev, monkeypatch):
    x, batch, pos, cell = _batch6()
    calls = _record(monkeypatch)

    def valid():
        del calls[:]
        g = _build(dev, _batch6(), mol_local=True)
        assert NEW[1] in calls and g.loc.m > 0

    low = cell.clone()
    low[3] = torch.eye(3) * 10.0                                                     # heights 10.0 <= 2 * 5.0
    flat = cell.clone()
    flat[0, 2] = flat[0, 0]
    for bad in (low, flat):
        del calls[:]
        with pytest.raises(ValueError, match='too small or singular'):
            _build(dev, _batch6(), mol_local=True, cell=bad.to(dev))
        assert NEW[0] in calls and NEW[1] not in calls and not [c for c in calls if c in STEPS], calls
        valid()
    strain = torch.zeros(6, 3, 3)
    strain[4, 1, 2] = 1e-3
    with pytest.raises(ValueError, match='non-zero'):
        _build(dev, _batch6(), mol_local=True, strain=strain.to(dev))
    valid()
    _build(dev, _batch6(), mol_local=True, strain=torch.zeros(6, 3, 3, device=dev))  # (zeros pass)
    wrong = x.clone()
    wrong[70] = 5.0
    with pytest.raises(IndexError):
        _build(dev, (wrong, batch, pos, cell), mol_local=True)
    # the input error outranks the cell's, as in the step-by-step route
    with pytest.raises(IndexError):
        _build(dev, (wrong, batch, pos, cell), mol_local=True, cell=low.to(dev))
    valid()


# ------------------------------------------------------------------------------------------------------- 5. model level
@pytest.mark.gpu
@pytest.mark.parametrize('small,dim', [(False, 128), (True, 32)])
def test_model_outputs_forces_virial_and_gradients_are_the_same_bits(dev, monkeypatch, small, dim):
    import models
    from pamnet_amd import synth
    torch.manual_seed(0)
    cfg = models.Config(dataset='QM9', dim=dim, n_layer=2, cutoff_l=CUTOFF_L, cutoff_g=CUTOFF_G)
    model = (models.PAMNet_s if small else models.PAMNet)(cfg).to(dev)
    x, batch, pos, cell = _batch6()
    calls = _record(monkeypatch)

    def run(vouch):
        data = synth.Batch(x=x, batch=batch, pos=pos, cell=cell, num_graphs=6).to(dev)
        if vouch:
            data.mol_local = True
        data.pos.requires_grad_(True)
        data.strain = torch.zeros(6, 3, 3, device=dev, requires_grad=True)
        model.zero_grad(set_to_none=True)
        del calls[:]
        out = model(data)
        out.sum().backward()
        used = [c for c in calls if c in NEW]
        grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
        return out.detach().clone(), data.pos.grad.clone(), data.strain.grad.clone(), grads, used

    out_b, f_b, w_b, gr_b, used_b = run(True)
    out_s, f_s, w_s, gr_s, used_s = run(False)
    assert used_b == list(NEW) and not used_s
    assert torch.isfinite(out_s).all() and float(f_s.abs().max()) > 0 and float(w_s.abs().max()) > 0
    assert torch.equal(out_b, out_s) and torch.equal(f_b, f_s) and torch.equal(w_b, w_s)
    assert gr_b.keys() == gr_s.keys() and len(gr_b) > 0
    for k in gr_b:
        assert torch.equal(gr_b[k], gr_s[k]), k


# ------------------------------------------------------------------------------------------------------ 7. entry points
@pytest.mark.gpu
def test_new_entry_points_validate_their_arguments(dev):
    """EINVAL / ENULL with nothing launched."""
    import ctypes
    from pamnet_amd import lib
    pos = torch.zeros((4, 3), device=dev)
    gptr = torch.tensor([0, 4], dtype=torch.int32, device=dev)
    tab = torch.full((1, 18), 7.0, dtype=torch.float64, device=dev)
    mol_tot = torch.full((4,), 7, dtype=torch.int32, device=dev)
    totals = torch.zeros(4, dtype=torch.int32, device=dev)
    st = lib.stream_of(pos)
    P = lib.ptr

    def count(pos_=pos, tab_=tab, gptr_=gptr, n=4, ng=1, cl=1.0, cg=2.0, mt=mol_tot, tot=totals):
        lib.call(NEW[0], P(pos_), P(tab_), P(gptr_), n, ng, cl, cg, 1, P(mt), P(tot), st)

    for kw in (dict(n=-1), dict(ng=0), dict(ng=-3), dict(cl=0.0), dict(cl=-1.0), dict(cg=0.0), dict(cl=float('nan')),
               dict(n=-1, tab_=None)):
        with pytest.raises(RuntimeError, match='EINVAL'):
            count(**kw)
    for kw in (dict(pos_=None), dict(tab_=None), dict(gptr_=None), dict(mt=None), dict(tot=None)):
        with pytest.raises(RuntimeError, match='ENULL'):
            count(**kw)
    o = lib.MolGraphOut()
    buf = torch.zeros(64, dtype=torch.int32, device=dev)
    for name, _ in lib.MolGraphOut._fields_:
        setattr(o, name, buf.data_ptr())

    def fill(pos_=pos, tab_=tab, gptr_=gptr, n=4, ng=1, nl=0, cl=1.0, cg=2.0, mt=mol_tot, eg=0, tp=0, out=o):
        lib.call(NEW[1], P(pos_), P(tab_), P(gptr_), n, ng, nl, cl, cg, 1, 1, P(mt), eg, tp,
                 None if out is None else ctypes.addressof(out), st)

    for kw in (dict(n=-1), dict(ng=0), dict(nl=-1), dict(cl=0.0), dict(cg=-2.0), dict(eg=-1), dict(tp=-1)):
        with pytest.raises(RuntimeError, match='EINVAL'):
            fill(**kw)
    missing = lib.MolGraphOut()
    for name, _ in lib.MolGraphOut._fields_:
        setattr(missing, name, buf.data_ptr())
    missing.l_ptr = None
    for kw in (dict(pos_=None), dict(tab_=None), dict(gptr_=None), dict(mt=None), dict(out=None), dict(out=missing)):
        with pytest.raises(RuntimeError, match='ENULL'):
            fill(**kw)
    torch.cuda.synchronize()
    assert int(mol_tot.min()) == 7 and int(totals.abs().max()) == 0 and int(buf.abs().max()) == 0     # nothing was launched


def test_header_declares_the_builder_entry_points_at_abi_18():
    """(No GPU: the header and the built library.)  The bond-free signatures with the cell table behind pos."""
    import ctypes
    import re
    from pamnet_amd import build, lib
    decl = lib.declared_functions()
    assert all(n in decl for n in NEW)
    assert len(decl['pamnet_mol_graph_free_count_i32']) == 10 and len(decl['pamnet_mol_graph_free_fill_i32']) == 14
    assert len(decl[NEW[0]]) == 11 and len(decl[NEW[1]]) == 15
    assert int(re.search(r'#define\s+PAMNET_ABI_VERSION\s+(\d+)', open(lib.HEADER).read()).group(1)) == 18
    h = ctypes.CDLL(build.build())
    assert h.pamnet_abi_version() == 18 and all(hasattr(h, n) for n in NEW)


# ------------------------------------------------------------------------------------------------- 8. open-space batches
@pytest.mark.gpu
def test_a_batch_without_cell_calls_neither_new_entry_point(dev, monkeypatch):
    from pamnet_amd import synth
    calls = _record(monkeypatch)
    b = synth.qm9_batch(0, 0, 8)
    for mol_local in (None, True, False):
        for inputs in ((b.x, b.batch, b.pos, torch.zeros(8, 3, 3)),):
            g = _build(dev, inputs, cutoff_l=1.7, cell=None, mol_local=mol_local)
            assert g.cell_tab is None
    assert 'pamnet_mol_graph_free_fill_i32' in calls and not [c for c in calls if c in NEW or c == PREPARE], calls
