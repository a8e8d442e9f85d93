"""Periodic cells: the virial W[g] = d prediction / d strain at zero strain, through `data.strain` (fp32 zeros [num_graphs, 3, 3],
requires_grad) -- csrc/forces.hip pamnet_pos_bwd_pbc_virial_f32, pamnet_amd/graph.py differentiable_geometry(strain=), models.py.

W[g][a][b] = sum over the directed global edges and local bonds e of graph g of v_e[a] * (dE / dv_e)[b], v_e the minimum-image
vector: the derivative under pos -> pos @ (I + eps_g), cell[g] -> cell[g] @ (I + eps_g) at eps = 0, image integers held fixed.
The kernel-level reference is exactly that statement: fp64 torch autograd through an explicit strain on test_pbc._geometry64.

Inputs, brute force and the parity protocol come from tests/test_pbc.py and tests/test_hip_forces.py (KTOL, _ok)."""
import pytest
import torch

from conftest import maxnorm_err
from test_pbc import (BOX, CUBE, TRI_A, _assert_margin, _brute, _brute_lists, _brute_of, _geometry64, _inputs, _record, _slices,
                      _split_batch, _supercell_batches, _with_cell)

VIRIAL = 'pamnet_pos_bwd_pbc_virial_f32'
TWIN = 'pamnet_pos_bwd_pbc_f32'


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs an MI355X'
    from pamnet_amd import lib
    lib.load()
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------------------- inputs
def _scatter_clear(gen, n, cell, min_sep, cutoffs=(2.0, 5.0), margin=2e-4):
    """n points uniform in the cell (fp64, then rounded to fp32) whose pairwise minimum-image distances are >= min_sep and
    stay `margin` away from every cutoff: at 300 atoms some of the 45 000 pairs would otherwise land within 1e-4 of 5.0."""
    cell = torch.as_tensor(cell, dtype=torch.float64)
    pts = torch.empty((0, 3), dtype=torch.float64)
    while pts.size(0) < n:
        p = (torch.rand(3, generator=gen, dtype=torch.float64) @ cell).float().double()
        if pts.size(0):
            d = p - pts
            d = d - torch.round(d @ torch.linalg.inv(cell)) @ cell
            r = d.pow(2).sum(-1).sqrt()
            if float(r.min()) < min_sep or any(float((r - c).abs().min()) < margin for c in cutoffs):
                continue
        pts = torch.cat([pts, p[None]])
    return pts


_CASES = {}


def _case(name):
    """(x, batch, pos fp32, cell fp32 [G, 3, 3]).  'a', 'b': test_pbc's.  'c': 300 atoms in TRI_A (the reduction strides past its
    256 threads; rows of > 64 global edges: the lanes stride more than once), 2 atoms 7 A apart on the diagonal of CUBE (no edge
    at all), 37 atoms in BOX."""
    if name in ('a', 'b'):
        return _inputs(name)
    if name not in _CASES:
        assert name == 'c'
        gen = torch.Generator().manual_seed(11)
        s = 7.0 / 3.0 ** 0.5
        pair = torch.tensor([[1.0, 1.0, 1.0], [1.0 + s, 1.0 + s, 1.0 + s]], dtype=torch.float64)
        pos = torch.cat([_scatter_clear(gen, 300, TRI_A, 0.8), pair, _scatter_clear(gen, 37, BOX, 0.8)]).float()
        counts = (300, 2, 37)
        batch = torch.cat([torch.full((n,), g, dtype=torch.long) for g, n in enumerate(counts)])
        x = torch.randint(0, 5, (batch.numel(),), generator=gen).float()
        _CASES[name] = (x, batch, pos, torch.tensor([TRI_A, CUBE, BOX], dtype=torch.float32))
    return _CASES[name]


def _brute_case(name):
    if name in ('a', 'b'):
        return _brute_of(name)
    key = name + '/brute'
    if key not in _CASES:
        x, batch, pos, cell = _case(name)
        _CASES[key] = _brute(pos, batch, cell)
    return _CASES[key]


def _graph(name, dev, cutoff_l=2.0):
    from pamnet_amd import graph as G
    x, batch, pos, cell = _case(name)
    return G.build_graph('QM9', cutoff_l, 5.0, 'source_to_target', x.to(dev), batch.to(dev), pos.to(dev), None,
                         num_graphs=int(cell.size(0)), n_types=5, cell=cell.to(dev), need_grad=True)


# ---------------------------------------------------------------------------------------------------------- CPU tests
def test_header_declares_the_virial_entry_point_at_abi_18():
    """(No GPU: the header and the built library.)  The twin's 29 parameters plus gptr, n_graphs, atom_work, dstrain."""
    import ctypes
    import re
    from pamnet_amd import build, lib
    decl = lib.declared_functions()
    assert VIRIAL in decl
    assert len(decl[TWIN]) == 29 and len(decl[VIRIAL]) == 33
    assert decl[VIRIAL][:3] == decl[TWIN][:3] and decl[VIRIAL][3:28] == decl[TWIN][3:28]
    assert decl[VIRIAL][28:] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert int(re.search(r'#define\s+PAMNET_ABI_VERSION\s+(\d+)', open(lib.HEADER).read()).group(1)) == 18
    h = ctypes.CDLL(build.build())
    assert h.pamnet_abi_version() == 18 and hasattr(h, VIRIAL)


def test_virial_inputs_meet_their_preconditions():
    """(No GPU.)  fp64 brute force: no pair within 1e-4 of either cutoff, minimum separation > 0, global edges, local edges and
    triplets that cross a face in every case, and the middle graph of case c has no pair within 5.0."""
    for name in ('a', 'b', 'c'):
        brute = _brute_case(name)
        for r in (2.0, 5.0):
            _assert_margin(brute, r)                              # (asserts the minimum separation > 0 as well)
        _assert_margin(brute, 0.5)
        cross_g = cross_l = cross_t = 0
        for s, v, n, d in brute:
            wraps = n.abs().sum(-1) > 0
            off = ~torch.eye(d.size(0), dtype=torch.bool)
            cross_g += int((wraps & (d <= 5.0) & off).sum())
            bond = (d <= 2.0) & off
            cross_l += int((wraps & bond).sum())
            # triplets k -> j -> i (k != i) with a bond across a face: all of them less those of two bonds that stay inside
            deg, inside = bond.long().sum(0), (bond & ~wraps).long().sum(0)
            cross_t += int((deg * (deg - 1)).sum() - (inside * (inside - 1)).sum())
        print(name, 'crossing: global', cross_g, 'local', cross_l, 'triplets (either bond)', cross_t)
        assert cross_g > 0 and cross_l > 0 and cross_t > 0
    for s, v, n, d in _brute_case('a'):
        assert float(d[~torch.eye(d.size(0), dtype=torch.bool)].min()) >= 0.8 - 1e-6          # cutoff_l = 0.5: no local edge
    s, v, n, d = _brute_case('c')[1]
    assert d.size(0) == 2 and abs(float(d[0, 1]) - 7.0) < 1e-5 and float(d[0, 1]) > 5.0
    x, batch, pos, cell = _case('c')
    assert [e - s for s, e in _slices(batch)] == [300, 2, 37]
    (ptr, rows, cols, _), _ = _brute_lists(_brute_case('c'), 5.0)
    assert int((ptr[1:301] - ptr[:300]).max()) > 64               # the lanes of a row stride more than once


# ------------------------------------------------------------------------------------------------- kernel-level, fp64
def _virial_reference(g, batch, pos, cell, ddg, ddl, dang):
    """d/d eps of sum ddg * dist_g + sum ddl * dist_l + sum dang * angle at eps = 0, fp64 autograd, pos -> pos @ (I + eps[batch]),
    cell -> cell @ (I + eps), with the image integers of the undeformed geometry held fixed."""
    p64, c64 = pos.double(), cell.double()
    images = _geometry64(g, p64, batch, c64)[3]
    eps = torch.zeros(c64.size(0), 3, 3, dtype=torch.float64, requires_grad=True)
    deform = torch.eye(3, dtype=torch.float64) + eps
    dg, dl, ang, _ = _geometry64(g, torch.einsum('ni,nij->nj', p64, deform[batch]), batch, c64 @ deform, images=images)
    total = (dg * ddg.cpu().double()).sum() + (dl * ddl.cpu().double()).sum() + (ang * dang.cpu().double()).sum()
    return torch.autograd.grad(total, eps)[0]


def _lists(g):
    from pamnet_amd import lib
    P = lib.ptr
    glob = [P(t) for t in (g.glob.ptr, g.glob.row_of, g.glob.col, g.glob_T.ptr, g.glob_T.perm)]
    loc = [P(t) for t in (g.loc.ptr, g.loc.row_of, g.loc.col, g.loc_T.ptr, g.loc_T.perm)]
    trip = [P(t) for t in (g.tp.ptr, g.tp.row_of, g.tp.col, g.tp_kind, g.tp_T.ptr, g.tp_T.perm)]
    return glob, loc, trip


@pytest.mark.gpu
@pytest.mark.parametrize('name,cutoff_l', [('a', 2.0), ('b', 2.0), ('c', 2.0), ('a', 0.5)])
def test_virial_kernel_vs_fp64_autograd_through_a_strain(dev, name, cutoff_l):
    """pamnet_pos_bwd_pbc_virial_f32 called directly with random upstream gradients: dpos bitwise the twin's, a second run
    bitwise the first, dstrain per graph within KTOL = 1e-6 of the fp64 reference (normalised by the graph's largest reference
    component), its antisymmetric part within the same bound, and exact zeros for a graph without edges."""
    from pamnet_amd import lib
    from test_hip_forces import KTOL
    assert KTOL == 1e-6
    x, batch, pos, cell = _case(name)
    g = _graph(name, dev, cutoff_l)
    n, ng, eg, el, tp = g.n, g.n_graphs, g.glob.m, g.loc.m, g.tp.m
    print(name, cutoff_l, 'atoms', n, 'global', eg, 'local', el, 'rows', tp)
    assert (el == 0 and tp == 0) == (cutoff_l == 0.5) and eg > 0
    torch.manual_seed(2)
    ddg, ddl, dang = torch.randn(eg, device=dev), torch.randn(el, device=dev), torch.randn(tp, device=dev)
    glob, loc, trip = _lists(g)
    P, st = lib.ptr, lib.stream_of(g.pos)
    work = torch.empty(3 * max(el, 1), dtype=torch.float64, device=dev)
    head = [P(g.pos), P(g.cell_tab), P(g.node_graph), n, *glob, P(ddg), eg, *loc, P(ddl), el, *trip, P(dang), tp, P(work)]

    def run():
        dpos = torch.full((n, 3), float('nan'), device=dev)
        atom_work = torch.full((n, 9), float('nan'), dtype=torch.float64, device=dev)
        dstrain = torch.full((ng, 9), float('nan'), device=dev)
        lib.call(VIRIAL, *head, P(dpos), P(g.gptr), ng, P(atom_work), P(dstrain), st)
        torch.cuda.synchronize()
        return dpos, dstrain

    twin = torch.full((n, 3), float('nan'), device=dev)
    lib.call(TWIN, *head, P(twin), st)
    torch.cuda.synchronize()
    dpos, dstrain = run()
    assert torch.isfinite(dpos).all() and torch.isfinite(dstrain).all()
    assert torch.equal(dpos, twin)                                # bit for bit what the position kernel writes
    dpos2, dstrain2 = run()
    assert torch.equal(dpos2, dpos) and torch.equal(dstrain2, dstrain)
    ref = _virial_reference(g, batch, pos, cell, ddg, ddl, dang)
    W = dstrain.cpu().double().view(ng, 3, 3)
    degree = (g.glob.ptr[1:] - g.glob.ptr[:-1]).cpu().long()
    for k, (s, e) in enumerate(_slices(batch)):
        scale = float(ref[k].abs().max())
        if int(degree[s:e].sum()) == 0:
            assert scale == 0.0 and bool((dstrain[k] == 0).all())                     # no edges: exactly 0.0 nine times
            continue
        err = float((W[k] - ref[k]).abs().max()) / scale
        asym = float((W[k] - W[k].t()).abs().max()) / 2 / scale
        print(name, cutoff_l, 'graph', k, 'scale', scale, 'virial err', err, 'antisymmetric part', asym)
        assert err <= KTOL, (k, err)
        assert asym <= KTOL, (k, asym)
    if name == 'c':
        assert bool((dstrain[1] == 0).all()) and int(degree[300:302].sum()) == 0


@pytest.mark.gpu
def test_virial_entry_point_validates_its_arguments(dev):
    """Every negative count and every null pointer answers EINVAL with nothing launched: the sentinel-filled outputs stay."""
    from pamnet_amd import lib
    P = lib.ptr
    i32 = lambda n, v=0: torch.full((n,), v, dtype=torch.int32, device=dev)
    pos = torch.zeros((4, 3), device=dev)
    tab = torch.eye(3, dtype=torch.float64, device=dev).mul(20).view(1, 9).repeat(1, 2).contiguous()
    ng, gptr, ptr, idx = i32(4), torch.tensor([0, 4], dtype=torch.int32, device=dev), i32(5), i32(8)
    grad = torch.zeros(8, device=dev)
    work = torch.full((24,), 7.0, dtype=torch.float64, device=dev)
    dpos, atom_work = torch.full((4, 3), 7.0, device=dev), torch.full((4, 9), 7.0, dtype=torch.float64, device=dev)
    dstrain = torch.full((1, 9), 7.0, device=dev)
    names = ['pos', 'cell_table', 'node_graph', 'n', 'g_ptr', 'g_row', 'g_col', 'gt_ptr', 'gt_perm', 'ddist_g', 'eg', 'l_ptr',
             'l_row', 'l_col', 'lt_ptr', 'lt_perm', 'ddist_l', 'el', 't_ptr', 't_row', 't_col', 't_kind', 'tt_ptr', 'tt_perm',
             'dangle', 'tp', 'bond_work', 'dpos', 'gptr', 'n_graphs', 'atom_work', 'dstrain']
    good = [P(pos), P(tab), P(ng), 4, P(ptr), P(idx), P(idx), P(ptr), P(idx), P(grad), 2, P(ptr), P(idx), P(idx), P(ptr),
            P(idx), P(grad), 2, P(ptr), P(idx), P(idx), P(idx), P(ptr), P(idx), P(grad), 2, P(work), P(dpos), P(gptr), 1,
            P(atom_work), P(dstrain)]
    assert len(names) == len(good) == len(lib.declared_functions()[VIRIAL]) - 1
    st = lib.stream_of(pos)
    tried = 0
    for k, name in enumerate(names):
        args = list(good)
        args[k] = -1 if name in ('n', 'eg', 'el', 'tp', 'n_graphs') else None
        with pytest.raises(RuntimeError, match='EINVAL'):
            lib.call(VIRIAL, *args, st)
        tried += 1
    assert tried == 32
    torch.cuda.synchronize()
    for t in (work, dpos, atom_work, dstrain):
        assert bool((t == 7).all())


# -------------------------------------------------------------------------------------------------------- end to end
def _strained(batch, dev, pos_grad=True, strain_grad=True, strain=True):
    """The batch on the device with fresh leaves: positions, and (strain=True) the zero strain tensor."""
    data = batch.to(dev)
    data.pos = data.pos.detach().clone().requires_grad_(pos_grad)
    if strain:
        data.strain = torch.zeros(int(data.cell.size(0)), 3, 3, device=dev, requires_grad=strain_grad)
    return data


@pytest.mark.gpu
@pytest.mark.parametrize('small,dim', [(False, 128), (False, 64), (True, 128)])
def test_split_molecules_have_the_virial_of_the_isolated_molecule(dev, small, dim):
    """16 molecules wrapped across faces, none seeing an image of itself: W[g] = sum_a pos_u[a] (x) dE/dpos_u[a] of the oracle
    fed the unwrapped coordinates (fp64), by test_hip_forces._ok with scale = max |W_ref| and the floor from the oracle's fp32
    forces.  In the same run: the forces are torch.equal to a run without `strain`, and no p.grad is touched."""
    import models
    from oracle import pamnet_oracle as O
    from test_hip_forces import TOL, _ok
    assert TOL == 1e-5
    periodic, ob, split = _split_batch()
    cfg = models.Config(dataset='QM9', dim=dim, n_layer=2, cutoff_l=1.7, cutoff_g=5.0)
    fwd = O.pamnet_s_forward if small else O.pamnet_forward
    sd = O.init_state_dict(cfg, seed=7, small=small)
    model = (models.PAMNet_s if small else models.PAMNet)(cfg)
    model.load_state_dict(sd, strict=True)
    model = model.to(dev)

    def oracle_virial(dtype):
        p = O.as_params({k: v.detach().to(dtype) for k, v in sd.items()})
        pos = ob.pos.to(dtype).clone().requires_grad_(True)
        fwd(p, cfg, ob.x, ob.batch, pos, ob.edge_index, dtype=dtype).sum().backward()
        outer = ob.pos.double()[:, :, None] * pos.grad.double()[:, None, :]          # [N, 3, 3], summed in fp64
        return torch.zeros(16, 3, 3, dtype=torch.float64).index_add_(0, ob.batch, outer)

    # parameter gradients of an ordinary step, to be found untouched afterwards
    torch.nn.functional.l1_loss(model(periodic.to(dev)), periodic.y.to(dev)).backward()
    before = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    assert before
    plain = periodic.to(dev)
    plain.pos.requires_grad_(True)
    f_plain, = torch.autograd.grad(model(plain).sum(), plain.pos)
    data = _strained(periodic, dev)
    f, W = torch.autograd.grad(model(data).sum(), [data.pos, data.strain])
    assert tuple(W.shape) == (16, 3, 3) and W.dtype == torch.float32 and torch.isfinite(W).all()
    assert torch.equal(f, f_plain)
    after = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    assert after.keys() == before.keys() and all(torch.equal(after[k], before[k]) for k in before)
    w32, w64 = oracle_virial(torch.float32), oracle_virial(torch.float64)
    scale = float(w64.abs().max())
    ok, info = _ok(W.cpu().numpy(), w32.numpy(), w64.numpy(), scale=scale)
    print('virial err / floor', info, 'scale', scale)
    assert ok, ('virial', info)


@pytest.mark.gpu
@pytest.mark.parametrize('dim,n_layer', [(128, 2), (16, 1)])
def test_a_supercell_has_twice_the_virial(dev, dim, n_layer):
    """Real cross-boundary interaction: W of the 2 x 1 x 1 supercell is 2 W per graph, the translated unwrapped copy has the
    same W, and per-graph weights on the energies scale each graph's W -- max-normalised per graph at 1e-5, the bound of
    test_pbc's supercell test for comparisons of this code against itself."""
    import models
    torch.manual_seed(1)
    a, a_moved, b = _supercell_batches()
    cfg = models.Config(dataset='QM9', dim=dim, n_layer=n_layer, cutoff_l=2.0, cutoff_g=5.0)
    model = models.PAMNet(cfg).to(dev)

    def run(bt, weights=None):
        data = _strained(bt, dev)
        out = model(data)
        if weights is not None:
            out = out * torch.tensor(weights, device=dev)
        return torch.autograd.grad(out.sum(), data.strain)[0].cpu().double()

    w_a, w_b, w_m, w_w = run(a), run(b), run(a_moved), run(a, [1.0, -2.5])
    assert torch.isfinite(w_a).all() and float(w_a.abs().min(0).values.max()) > 0
    for k, weight in enumerate((1.0, -2.5)):
        errs = (maxnorm_err(w_b[k].numpy(), (2 * w_a[k]).numpy()), maxnorm_err(w_m[k].numpy(), w_a[k].numpy()),
                maxnorm_err(w_w[k].numpy(), (weight * w_a[k]).numpy()))
        print('graph', k, 'supercell / translation / weight errs', errs)
        assert max(errs) <= 1e-5, (k, errs)


# --------------------------------------------------------------------------------------------------------- interface
def _free4():
    from pamnet_amd import synth
    b = synth.qm9_batch(0, 0, 4)
    return b, synth.Batch(**{k: v for k, v in b.__dict__.items() if k != 'edge_index'})


@pytest.mark.gpu
@pytest.mark.parametrize('small,dim', [(False, 128), (True, 32)])
def test_only_a_strain_that_requires_grad_takes_the_new_entry_point(dev, monkeypatch, small, dim):
    import models
    torch.manual_seed(0)
    a, _, _ = _supercell_batches()
    cfg = models.Config(dataset='QM9', dim=dim, n_layer=1, cutoff_l=2.0, cutoff_g=5.0)
    model = (models.PAMNet_s if small else models.PAMNet)(cfg).to(dev)
    calls = _record(monkeypatch)

    def forces(data):
        del calls[:]
        out = model(data)
        f, = torch.autograd.grad(out.sum(), data.pos)
        return out.detach(), f, list(calls)

    forces(_strained(a, dev, strain=False))                       # (first run: the engine packs its plan, once per model)
    out0, f0, used0 = forces(_strained(a, dev, strain=False))
    assert TWIN in used0 and VIRIAL not in used0                  # no strain at all
    out1, f1, used1 = forces(_strained(a, dev, strain_grad=False))
    assert used1 == used0 and torch.equal(out1, out0) and torch.equal(f1, f0)         # a strain that does not require grad
    with torch.no_grad():
        del calls[:]
        out2 = model(_strained(a, dev))
        assert VIRIAL not in calls and TWIN not in calls and torch.equal(out2, out0)  # no-grad mode
        plain = a.to(dev)
        model(plain)                                              # (first run in this mode, as above)
        del calls[:]
        assert torch.equal(model(plain), out0)
        used_plain = list(calls)
        del calls[:]
        model(_strained(a, dev))
        assert calls == used_plain                               # exactly the entry points of a batch without strain
    # the joint call, the strain-only call and prepare + forward give the same bits
    data = _strained(a, dev)
    del calls[:]
    out3 = model(data)
    f3, w3 = torch.autograd.grad(out3.sum(), [data.pos, data.strain])
    assert calls.count(VIRIAL) == 1 and TWIN not in calls
    assert torch.equal(out3.detach(), out0) and torch.equal(f3, f0) and float(w3.abs().max()) > 0
    only = _strained(a, dev, pos_grad=False)
    out4 = model(only)
    w4, = torch.autograd.grad(out4.sum(), only.strain)
    assert torch.equal(out4.detach(), out0) and torch.equal(w4, w3)
    pre = _strained(a, dev)
    model.prepare(pre)
    out5 = model(pre)
    f5, w5 = torch.autograd.grad(out5.sum(), [pre.pos, pre.strain])
    assert torch.equal(out5.detach(), out0) and torch.equal(f5, f0) and torch.equal(w5, w3)
    model.train(not model.training)                               # the other mode: the same numbers
    flip = _strained(a, dev)
    w6, = torch.autograd.grad(model(flip).sum(), flip.strain)
    assert torch.equal(w6, w3)


@pytest.mark.gpu
def test_strain_refusals_say_what_to_do_instead(dev):
    import models
    cfg = models.Config(dataset='QM9', dim=16, n_layer=1, cutoff_l=1.7, cutoff_g=5.0)
    torch.manual_seed(0)
    model = models.PAMNet(cfg).to(dev)
    b, free = _free4()
    cell = (torch.eye(3) * 40.0).expand(4, 3, 3).contiguous()
    periodic = _with_cell(free, cell)

    def with_strain(batch, strain):
        data = batch.to(dev)
        data.strain = strain
        return data

    zeros = lambda *shape, **kw: torch.zeros(*shape, device=kw.pop('device', dev), requires_grad=True, **kw)
    for open_space in (free, b):                                  # no cell: strain belongs to periodic batches
        with pytest.raises(ValueError, match='isolated molecule'):
            model(with_strain(open_space, zeros(4, 3, 3)))
    for bad in (zeros(3, 3, 3), zeros(4, 9), zeros(4, 3, 3, dtype=torch.float64), zeros(4, 3, 3, device='cpu')):
        with pytest.raises(ValueError, match=r'\[num_graphs, 3, 3\]'):
            model(with_strain(periodic, bad))
    nonzero = torch.zeros(4, 3, 3, device=dev)
    nonzero[2, 0, 1] = 1e-3
    for strain in (nonzero.clone().requires_grad_(True), nonzero):                    # refused whether or not it requires grad
        with pytest.raises(ValueError, match='deform `pos` and `cell` yourself'):
            model(with_strain(periodic, strain))
    with pytest.raises(ValueError, match='deform `pos` and `cell` yourself'):
        model.prepare(with_strain(periodic, nonzero.clone().requires_grad_(True)))
    late = periodic.to(dev)
    model.prepare(late)
    late.strain = zeros(4, 3, 3)
    with pytest.raises(ValueError, match='prepare'):
        model(late)
    other = models.PAMNet(cfg, num_spherical=5, num_radial=4).to(dev)                 # default basis only
    with pytest.raises(NotImplementedError, match='default basis'):
        other(with_strain(periodic, zeros(4, 3, 3)))
    data = with_strain(periodic, zeros(4, 3, 3))                                      # no second derivatives
    with pytest.raises(RuntimeError, match='second derivatives'):
        torch.autograd.grad(model(data).sum(), data.strain, create_graph=True)
    grad_cell = periodic.to(dev)
    grad_cell.cell.requires_grad_(True)
    with pytest.raises(NotImplementedError, match='stress') as info:
        model(grad_cell)
    assert 'strain' in str(info.value)                            # ... and points at the strain input
    good = with_strain(periodic, zeros(4, 3, 3))                                      # and the accepted form works
    w, = torch.autograd.grad(model(good).sum(), good.strain)
    assert tuple(w.shape) == (4, 3, 3) and torch.isfinite(w).all()
