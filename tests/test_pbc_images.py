"""Periodic cells below twice the global cutoff: `data.cell_images = 'all'` gives a GLOBAL graph over every image within cutoff_g
(a multigraph with an integer triple per edge) beside the unchanged minimum-image local graph -- pamnet_amd/graph.py
build_graph(cell_images=), csrc/geom_core.h image_disp, and the five entry points pamnet_cell_images_i32,
pamnet_radius_img_count/fill_i32, pamnet_pos_bwd_img_f32, pamnet_pos_bwd_img_virial_f32.

Conventions of tests/test_pbc.py: the fp64 references are brute-force torch written here (every image of every pair inside a box
one wider than the kernels' own), the inputs are made once on the CPU by rejection sampling on a 1/128 grid and never modified,
and every list test asserts its precondition first: no (pair, image) distance within 1e-4 of the cutoff under test.

Tolerances: TOL, GRAD_TOL, KTOL of tests/test_hip_forces.py."""
import itertools
import math

import pytest
import torch

from conftest import maxnorm_err
from test_pbc import _assert_margin, _brute_of, _heights, _inputs, _record, _slices

NEW = ('pamnet_cell_images_i32', 'pamnet_radius_img_count_i32', 'pamnet_radius_img_fill_i32', 'pamnet_pos_bwd_img_f32',
       'pamnet_pos_bwd_img_virial_f32')
PBC_BIT, CAP_BIT = 128, 64
CUT_G, CUT_L = 5.0, 2.0
GRID = 1.0 / 128
SEP = 0.9
# (name, cell, atoms); every entry a multiple of 1/8: integer lattice sums of grid positions are exact in fp32
CELLS = (('cube', [[4.5, 0.0, 0.0], [0.0, 4.5, 0.0], [0.0, 0.0, 4.5]], 7),
         ('tri', [[4.5, 0.0, 0.0], [1.0, 4.75, 0.0], [-0.75, 0.875, 5.0]], 9),
         ('slab', [[4.25, 0.0, 0.0], [0.0, 6.5, 0.0], [0.0, 0.0, 12.0]], 20),
         ('one', [[4.25, 0.0, 0.0], [0.0, 4.25, 0.0], [0.0, 0.0, 4.25]], 1))
SEED = 0


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs an MI355X'
    from pamnet_amd import lib
    lib.load()
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------ fp64 brute force (CPU)
def _box(cell, r, extra=1):
    """Half-widths ceil(r / height_k) + extra of the image box, and its triples m in ascending (m0, m1, m2) order [M, 3]."""
    half = [int(math.ceil(r / h)) + extra for h in _heights(cell)]
    m = torch.tensor(list(itertools.product(*[range(-k, k + 1) for k in half])), dtype=torch.float64)
    return half, m


def _all_images(p, cell, r):
    """p [n, 3], cell [3, 3] (fp64) -> (images nn [n, n, M, 3], vectors v[a, b, m] = p_a - p_b - nn @ cell, lengths d): the
    images of every ordered pair inside a box one wider than ceil(r / height) around the rounded fractional displacement,
    ascending in (n0, n1, n2).  The set of images within r does not depend on where the box is centred."""
    _, m = _box(cell, r)
    d0 = p[:, None, :] - p[None, :, :]
    nn = torch.round(d0 @ torch.linalg.inv(cell))[:, :, None, :] + m[None, None]
    v = d0[:, :, None, :] - nn @ cell
    return nn, v, v.pow(2).sum(-1).sqrt()


def _brute_images(pos, batch, cell, r):
    """Per graph: (first node, nn, v, d, keep) with keep[a, b, m] = the entry belongs to the all-image graph at r (within r, and
    not the atom's own zero image)."""
    out = []
    for g, (s, e) in enumerate(_slices(batch)):
        nn, v, d = _all_images(pos[s:e].double(), cell[g].double(), r)
        own = torch.eye(e - s, dtype=torch.bool)[:, :, None] & (nn.abs().sum(-1) == 0)
        out.append((s, nn, v, d, (d <= r) & ~own))
    return out


def _assert_image_margin(brute, r):
    for s, nn, v, d, keep in brute:
        own = torch.eye(d.size(0), dtype=torch.bool)[:, :, None] & (nn.abs().sum(-1) == 0)
        off = d[~own]
        assert float((off - r).abs().min()) > 1e-4, (s, r, float((off - r).abs().min()))
        assert float(off.min()) >= SEP - 1e-9, (s, float(off.min()))


def _brute_image_lists(brute):
    """(ptr, row_of, nbr, img, dist) in the stated order: rows by query, then ascending (neighbour, n0, n1, n2)."""
    rows, cols, img, dist = [], [], [], []
    for s, nn, v, d, keep in brute:
        q, j, m = keep.nonzero(as_tuple=True)                     # (ascending (q, j, m): m ascends with the image)
        rows.append(q + s), cols.append(j + s), img.append(nn[q, j, m].long()), dist.append(d[q, j, m])
    rows, cols, img, dist = torch.cat(rows), torch.cat(cols), torch.cat(img), torch.cat(dist)
    total = sum(d.size(0) for _, _, _, d, _ in brute)
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.bincount(rows, minlength=total).cumsum(0)])
    return ptr, rows, cols, img, dist


# ------------------------------------------------------------------------------------------------------------- inputs
def _scatter(gen, n, cell):
    """n points of the 1/128 grid in the cell, every image of every pair (an atom's own images too) at least SEP away."""
    pts = []
    while len(pts) < n:
        p = torch.round((torch.rand(3, generator=gen, dtype=torch.float64) @ cell) / GRID) * GRID
        _, _, d = _all_images(torch.stack(pts + [p]), cell, SEP)
        near = d[-1]
        if float(near[near > 0].min()) < SEP:
            continue
        pts.append(p)
    return torch.stack(pts)


_SMALL = {}


def _small(with_one=True):
    """(x, batch, pos fp32, cell fp32 [G, 3, 3]) of the small cells, made once: a 4.5 cube with 7 atoms, a triclinic cell with 9
    whose atoms are displaced by up to +-3 lattice vectors (unwrapped input), a 4.25 x 6.5 x 12 slab with 20 and (with_one) a
    4.25 cube with one atom, whose only edges are its six images.  with_one=False: the same first three graphs."""
    if not _SMALL:
        gen = torch.Generator().manual_seed(SEED)
        cells = [torch.tensor(c, dtype=torch.float64) for _, c, _ in CELLS]
        pos = [_scatter(gen, n, c) for (_, _, n), c in zip(CELLS, cells)]
        shift = torch.randint(-3, 4, (CELLS[1][2], 3), generator=gen).double()
        assert int(shift.abs().max()) == 3
        pos[1] = pos[1] + shift @ cells[1]
        x = [torch.randint(0, 5, (n,), generator=gen).float() for _, _, n in CELLS]
        for t in pos + cells:
            assert torch.equal(torch.round(t / GRID) * GRID, t) and float(t.abs().max()) < 64.0
        _SMALL['parts'] = (x, pos, cells)
    x, pos, cells = _SMALL['parts']
    k = len(CELLS) if with_one else len(CELLS) - 1
    if k not in _SMALL:
        batch = torch.cat([torch.full((p.size(0),), g, dtype=torch.long) for g, p in enumerate(pos[:k])])
        p32, c32 = torch.cat(pos[:k]).float(), torch.stack(cells[:k]).float()
        assert torch.equal(p32.double(), torch.cat(pos[:k])) and torch.equal(c32.double(), torch.stack(cells[:k]))
        _SMALL[k] = (torch.cat(x[:k]), batch, p32, c32)
    return _SMALL[k]


_BRUTE = {}


def _brute_small(r):
    if r not in _BRUTE:
        x, batch, pos, cell = _small()
        _BRUTE[r] = _brute_images(pos, batch, cell, r)
    return _BRUTE[r]


def _batch(x, batch, pos, cell, **kw):
    from pamnet_amd import synth
    return synth.Batch(x=x, batch=batch, pos=pos, cell=cell, num_graphs=int(cell.size(0)), **kw)


def _supercell(x, batch, pos, cell, k=3):
    """The k x k x k replication of every graph as one graph: replica (a, b, c) = the atoms moved by a a_0 + b a_1 + c a_2, replica-
    major; cell k times as long.  Exact in fp32 (grid inputs)."""
    xs, ps, bs = [], [], []
    for g, (s, e) in enumerate(_slices(batch)):
        c = cell[g].double()
        for t in itertools.product(range(k), repeat=3):
            ps.append(pos[s:e].double() + torch.tensor(t, dtype=torch.float64) @ c)
            xs.append(x[s:e]), bs.append(torch.full((e - s,), g, dtype=torch.long))
    p64 = torch.cat(ps)
    assert torch.equal(p64.float().double(), p64)
    return torch.cat(xs), torch.cat(bs), p64.float(), cell * k


# -------------------------------------------------------------------------------------------------- CPU: preconditions
def test_image_inputs_meet_their_preconditions():
    """(No GPU.)  What the GPU tests state about their inputs, in fp64."""
    x, batch, pos, cell = _small()
    assert [e - s for s, e in _slices(batch)] == [n for _, _, n in CELLS]
    for g, (name, c, n) in enumerate(CELLS):
        h = _heights(c)
        assert min(h) > 2 * CUT_L and min(h) < 2 * CUT_G, (name, h)       # fine for the local graph, refused by the old rule
        half, m = _box(torch.tensor(c, dtype=torch.float64), CUT_G, extra=0)
        assert max(half) <= 4 and min(half) >= 1
        assert (m.size(0) * n) % 64 != 0                                  # candidates per row: no multiple of the wavefront
        print(name, 'heights', [round(v, 3) for v in h], 'box', half, 'candidates per row', m.size(0) * n)
    for r in (CUT_G, CUT_L):
        _assert_image_margin(_brute_small(r), r)
    for (name, _, n), (s, nn, v, d, keep) in zip(CELLS, _brute_small(CUT_G)):
        eye = torch.eye(n, dtype=torch.bool)
        self_edges = keep[eye].sum(-1)
        per_pair = keep.sum(-1)
        rows = keep.sum((1, 2))
        print(name, 'rows', int(rows.min()), '..', int(rows.max()), 'self-image edges per atom', self_edges.tolist()[:3],
              'most images of one pair', int(per_pair.max()))
        assert int(self_edges.min()) >= 1 and int(per_pair.max()) >= 2
        # the cubes: the six face neighbours; the triclinic cell: +-a_0 and +-a_1 (|a_2| = 5.14); the slab: +-a_0
        assert self_edges.tolist() == [{'cube': 6, 'tri': 4, 'slab': 2, 'one': 6}[name]] * n
        if name == 'one':
            assert int(keep.sum()) == 6
    for s, nn, v, d, keep in _brute_small(CUT_L):                         # the local graph is a simple graph
        assert int(keep.sum(-1).max()) <= 1 and not bool(keep[torch.eye(d.size(0), dtype=torch.bool)].any())
    # the large cells of tests/test_pbc.py: one image per pair at most, and empty rows at r = 2.0 exist
    for name in ('a', 'b'):
        for r in (CUT_L, CUT_G):
            _assert_margin(_brute_of(name), r)
        bx, bbatch, bpos, bcell = _inputs(name)
        assert min(min(_heights(c)) for c in bcell.double()) >= 10.4
    rows2 = torch.cat([((d <= CUT_L).sum(-1) - 1) for _, _, _, d in _brute_of('a')])
    assert int((rows2 == 0).sum()) > 0
    # the supercell of the first three graphs goes through the minimum-image path
    sx, sbatch, spos, scell = _supercell(*_small(with_one=False))
    assert min(min(_heights(c)) for c in scell.double()) >= 12.75 > 2 * CUT_G
    assert [e - s for s, e in _slices(sbatch)] == [27 * n for _, _, n in CELLS[:3]]


def test_header_declares_the_image_entry_points_at_abi_18():
    """(No GPU: the header and the built library.)  The *_pbc_* argument lists with img_box behind cell_table, img behind
    row_of, g_img behind g_col; the ABI number stays."""
    import ctypes
    import re
    from pamnet_amd import build, lib
    decl = lib.declared_functions()
    assert all(n in decl for n in NEW)
    assert [len(decl[n]) for n in NEW] == [6, 12, 16, 30, 34]
    assert len(decl['pamnet_radius_pbc_count_i32']) == 11 and len(decl['pamnet_radius_pbc_fill_i32']) == 14
    assert len(decl['pamnet_pos_bwd_pbc_f32']) == 29 and len(decl['pamnet_pos_bwd_pbc_virial_f32']) == 33
    assert int(re.search(r'#define\s+PAMNET_ABI_VERSION\s+(\d+)', open(lib.HEADER).read()).group(1)) == 18
    h = ctypes.CDLL(build.build())
    assert h.pamnet_abi_version() == 18 and all(hasattr(h, n) for n in NEW)


# ------------------------------------------------------------------------------------------ 1. lists against brute force
def _search(x, batch, pos, cell, r, dev, max_nb=0, cutoff_l=CUT_L):
    """pamnet_cell_images_i32 and pamnet_radius_img_count/fill_i32 called directly: (ptr, row_of, nbr, img, dist) on the CPU,
    the box and the flag word."""
    from pamnet_amd import graph as G
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    tab = G.cell_table(cell.to(dev).contiguous().view(-1, 9), cutoff_l, flag)
    box = G.cell_images(tab, r, flag)
    node_graph = batch.to(dev).to(torch.int32)
    gptr = torch.tensor([s for s, _ in _slices(batch)] + [int(batch.numel())], dtype=torch.int32, device=dev)
    p = pos.to(dev).contiguous()
    ptr = G.radius_img_count(p, tab, box, node_graph, gptr, r, max_nb, flag)
    ptr, nbr, dist, rows, img = G.radius_img_fill(p, tab, box, node_graph, gptr, r, ptr, int(ptr[-1]), max_neighbors=max_nb)
    torch.cuda.synchronize()
    return (ptr.cpu().long(), rows.cpu().long(), nbr.cpu().long(), img.cpu().long(), dist.cpu()), box.cpu(), int(flag)


def _assert_lists(got, want):
    g_ptr, g_rows, g_nbr, g_img, g_dist = got
    ptr, rows, cols, img, dist = want
    assert torch.equal(g_ptr, ptr) and torch.equal(g_rows, rows) and torch.equal(g_nbr, cols) and torch.equal(g_img, img)
    rel = float(((g_dist.double() - dist).abs() / dist).max())
    assert rel <= 1e-6, rel
    # the reverse of (i, j, n) is (j, i, -n), with a bitwise equal length
    where = {(int(i), int(j)) + tuple(n): k for k, (i, j, n) in enumerate(zip(g_rows, g_nbr, g_img.tolist()))}
    assert len(where) == int(g_rows.numel())                      # (no entry twice)
    back = torch.tensor([where[(int(j), int(i), -n[0], -n[1], -n[2])] for i, j, n in zip(g_rows, g_nbr, g_img.tolist())])
    assert torch.equal(g_dist.view(torch.int32)[back], g_dist.view(torch.int32))
    return rel


@pytest.mark.gpu
def test_image_lists_match_brute_force(dev, monkeypatch):
    """The four small cells at 5.0: ptr / row_of / nbr / img exactly in ascending (j, n0, n1, n2), lengths within 1e-6 relative of
    fp64, every edge with its reverse (j, i, -n) at a bitwise equal length; the box is ceil(cutoff / height)."""
    x, batch, pos, cell = _small()
    brute = _brute_small(CUT_G)
    _assert_image_margin(brute, CUT_G)
    calls = _record(monkeypatch)
    got, box, flag = _search(x, batch, pos, cell, CUT_G, dev)
    assert [c for c in calls if c in NEW] == list(NEW[:3]), calls
    assert flag == 0
    assert box.tolist() == [_box(torch.tensor(c, dtype=torch.float64), CUT_G, extra=0)[0] for _, c, _ in CELLS]
    want = _brute_image_lists(brute)
    rel = _assert_lists(got, want)
    ptr, rows, cols, img, dist = want
    sizes = ptr[1:] - ptr[:-1]
    print('edges', int(rows.numel()), 'rows', int(sizes.min()), '..', int(sizes.max()), 'self-image edges', int((rows == cols).sum()),
          'length rel err', rel)
    assert int((rows == cols).sum()) == 6 * 7 + 4 * 9 + 2 * 20 + 6 and int(sizes[-1]) == 6
    assert int(img[batch[rows] == 1].abs().max()) >= 3            # the unwrapped graph: images far from the first shell


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['a', 'b'])
def test_image_lists_of_large_cells_at_the_local_cutoff(dev, name):
    """r = 2.0 in cells of height >= 10.4 (box 1 1 1, 27 candidates per pair): against brute force; some rows are empty."""
    x, batch, pos, cell = _inputs(name)
    brute = _brute_images(pos, batch, cell, CUT_L)
    _assert_image_margin_large(brute, CUT_L)
    got, box, flag = _search(x, batch, pos, cell, CUT_L, dev)
    assert flag == 0 and box.tolist() == [[1, 1, 1]] * 2
    want = _brute_image_lists(brute)
    _assert_lists(got, want)
    sizes = want[0][1:] - want[0][:-1]
    if name == 'a':
        assert int((sizes == 0).sum()) > 0
    assert int(sizes.max()) > 0


def _assert_image_margin_large(brute, r):
    for s, nn, v, d, keep in brute:
        own = torch.eye(d.size(0), dtype=torch.bool)[:, :, None] & (nn.abs().sum(-1) == 0)
        assert float((d[~own] - r).abs().min()) > 1e-4


# ------------------------------------------------------------------------- 2. large cells agree between the two modes
def _build(inputs, dev, **kw):
    from pamnet_amd import graph as G
    x, batch, pos, cell = inputs
    return G.build_graph('QM9', CUT_L, CUT_G, 'source_to_target', x.to(dev), batch.to(dev), pos.to(dev), None,
                         num_graphs=int(cell.size(0)), n_types=5, cell=cell.to(dev), **kw)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['a', 'b'])
def test_large_cells_have_the_same_lists_in_both_modes(dev, monkeypatch, name):
    """Heights >= 10.4: every array of the graph is torch.equal between cell_images='all' and the minimum-image build (the
    general transpose of a simple symmetric list is its reverse-edge index), and img is the rounded fractional displacement."""
    from test_pbc import _arrays
    inputs = _inputs(name)
    x, batch, pos, cell = inputs
    for r in (CUT_L, CUT_G):
        _assert_margin(_brute_of(name), r)
    calls = _record(monkeypatch)
    g_min = _build(inputs, dev, need_grad=True, cell_images='minimum')
    assert not [c for c in calls if c in NEW], calls
    del calls[:]
    g_all = _build(inputs, dev, need_grad=True, cell_images='all')
    assert [c for c in calls if c in NEW] == list(NEW[:3]), calls
    assert 'pamnet_radius_pbc_count_i32' in calls and 'pamnet_radius_pbc_fill_i32' in calls          # the local graph
    assert 'pamnet_reverse_edges_i32' in calls and 'pamnet_transpose_gather_i32' not in calls
    xa, xb = _arrays(g_min), _arrays(g_all)
    assert xa.keys() == xb.keys()
    for k in xa:
        assert xa[k].dtype == xb[k].dtype and torch.equal(xa[k], xb[k]), k
    assert g_min.img_g is None and g_all.img_g.dtype == torch.int32 and tuple(g_all.img_g.shape) == (g_all.glob.m, 3)
    rows, cols = g_all.glob.row_of.cpu().long(), g_all.glob.col.cpu().long()
    c = cell.double()[batch]
    frac = torch.einsum('ei,eij->ej', pos.double()[rows] - pos.double()[cols], torch.linalg.inv(c)[rows])
    assert float((frac - torch.round(frac)).abs().max()) < 0.49   # (no tie: within 5.0 of a cell of height >= 10.4)
    assert torch.equal(g_all.img_g.cpu().long(), torch.round(frac).long())
    assert int(g_all.img_g.abs().max()) > 0


MODELS = [(False, 16, 1), (False, 128, 2), (True, 32, 2)]


def _model(small, dim, n_layer, dev, seed=0):
    import models
    torch.manual_seed(seed)
    cfg = models.Config(dataset='QM9', dim=dim, n_layer=n_layer, cutoff_l=CUT_L, cutoff_g=CUT_G)
    return (models.PAMNet_s if small else models.PAMNet)(cfg).to(dev)


def _run(model, bt, dev, forces, **attrs):
    """One forward + backward.  forces: positions and a zero strain require grad (out.sum().backward(): forces, virial and the
    parameter gradients of the geometry route); else the training route (the layer engines).  Returns CPU-side clones."""
    data = bt.to(dev)
    for k, v in attrs.items():
        setattr(data, k, v)
    model.zero_grad(set_to_none=True)
    if forces:
        data.pos = data.pos.detach().clone().requires_grad_(True)
        data.strain = torch.zeros(int(data.cell.size(0)), 3, 3, device=dev, requires_grad=True)
    out = model(data)
    (out * torch.linspace(0.5, 1.5, out.numel(), device=dev)).sum().backward() if not forces else out.sum().backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    assert len(grads) > 0
    return (out.detach().clone(), data.pos.grad.detach().clone() if forces else None,
            data.strain.grad.detach().clone() if forces else None, grads)


@pytest.mark.gpu
@pytest.mark.parametrize('small,dim,n_layer', MODELS)
def test_large_cells_give_the_same_bits_in_both_modes(dev, monkeypatch, small, dim, n_layer):
    """Outputs, pos.grad, the virial through `strain` and every parameter gradient are torch.equal between the two modes, with
    the 'all' run on the new entry points and the other on none of them."""
    model = _model(small, dim, n_layer, dev)
    calls = _record(monkeypatch)
    for name in ('a', 'b'):
        bt = _batch(*_inputs(name))
        for forces in (True, False):
            del calls[:]
            o_min, f_min, w_min, g_min = _run(model, bt, dev, forces)
            assert not [c for c in calls if c in NEW], calls
            del calls[:]
            o_all, f_all, w_all, g_all = _run(model, bt, dev, forces, cell_images='all')
            used = [c for c in calls if c in NEW]
            assert used == list(NEW[:3]) + ([NEW[4]] if forces else []), used
            assert torch.isfinite(o_all).all() and torch.equal(o_min, o_all)
            if forces:
                assert float(f_all.abs().max()) > 0 and float(w_all.abs().max()) > 0
                assert torch.equal(f_min, f_all) and torch.equal(w_min, w_all)
            assert g_min.keys() == g_all.keys()
            for k in g_min:
                assert torch.equal(g_min[k], g_all[k]), k


# ----------------------------------------------------------------------------------- 3. a small cell equals its supercell
@pytest.mark.gpu
@pytest.mark.parametrize('small,dim,n_layer', [(False, 128, 2), (False, 16, 1), (True, 32, 2)])
def test_a_small_cell_equals_its_supercell(dev, monkeypatch, small, dim, n_layer):
    """The three small cells under cell_images='all' against their 3 x 3 x 3 replication under the minimum-image rule (heights
    >= 12.75): E_super = 27 E_cell, every replica carries the base atom's force, W_super = 27 W_cell; and moving the small cells'
    atoms by lattice vectors without wrapping changes nothing.  Max-normalised at TOL = 1e-5, the bound of
    test_pbc.test_a_supercell_has_twice_the_energy_and_the_same_forces: the same code in fp32 with other summation orders."""
    from test_hip_forces import TOL
    assert TOL == 1e-5
    base = _small(with_one=False)
    x, batch, pos, cell = base
    for r in (CUT_L, CUT_G):
        _assert_image_margin(_brute_small(r)[:3], r)
    sup = _supercell(*base)
    model = _model(small, dim, n_layer, dev, seed=1)
    calls = _record(monkeypatch)
    e_c, f_c, w_c, _ = _run(model, _batch(*base), dev, True, cell_images='all')
    assert NEW[4] in calls
    g_c = model._graph_cache
    del calls[:]
    e_s, f_s, w_s, _ = _run(model, _batch(*sup), dev, True)
    assert not [c for c in calls if c in NEW], calls
    g_s = model._graph_cache
    assert g_s.glob.m == 27 * g_c.glob.m and g_s.loc.m == 27 * g_c.loc.m and g_s.tp.m == 27 * g_c.tp.m
    assert g_c.loc.m > 0 and g_c.tp.m > 0
    e_c, f_c, w_c, e_s, f_s, w_s = (t.cpu().double() for t in (e_c, f_c, w_c, e_s, f_s, w_s))
    assert torch.isfinite(e_c).all() and float(e_c.abs().min()) > 0 and float(f_c.abs().max()) > 0 and float(w_c.abs().max()) > 0
    f_ref = torch.cat([f_c[s:e].repeat(27, 1) for s, e in _slices(batch)])
    err_e, err_f = maxnorm_err(e_s.numpy(), (27 * e_c).numpy()), maxnorm_err(f_s.numpy(), f_ref.numpy())
    err_w = maxnorm_err(w_s.numpy(), (27 * w_c).numpy())
    gen = torch.Generator().manual_seed(9)
    shift = torch.randint(-3, 4, (pos.size(0), 3), generator=gen).double()
    moved = pos.double() + torch.einsum('ni,nij->nj', shift, cell.double()[batch])
    assert torch.equal(moved.float().double(), moved) and int(shift.abs().max()) == 3
    e_m, f_m, w_m, _ = _run(model, _batch(x, batch, moved.float(), cell), dev, True, cell_images='all')
    err_te, err_tf = maxnorm_err(e_m.cpu().numpy(), e_c.numpy()), maxnorm_err(f_m.cpu().numpy(), f_c.numpy())
    print('supercell: energy err', err_e, 'force err', err_f, 'virial err', err_w, '; translation: energy err', err_te,
          'force err', err_tf)
    assert err_e <= TOL and err_f <= TOL and err_w <= TOL, (err_e, err_f, err_w)
    assert err_te <= TOL and err_tf <= TOL, (err_te, err_tf)


# ---------------------------------------------------------------------------------- 4. backward kernels against fp64 torch
def _geometry64(g, pos, batch, cell, eps=None):
    """fp64 torch statement of the geometry on g's lists: the global edges through their stored images, the local ones through
    the rounded image (held fixed).  eps [G, 3, 3]: every edge vector v -> v @ (I + eps[graph]) -- the homogeneous deformation of
    positions and cell with the images held fixed.  Returns (dist_g, dist_l, angles)."""
    from oracle import pamnet_oracle as O
    c = cell.double()[batch]
    inv = torch.linalg.inv(c)
    gi, gc = g.glob.row_of.long().cpu(), g.glob.col.long().cpu()
    li, lj = g.loc.row_of.long().cpu(), g.loc.col.long().cpu()
    e, q, kind = g.tp.row_of.long().cpu(), g.tp.col.long().cpu(), g.tp_kind.cpu()
    w = pos[gi] - pos[gc] - torch.einsum('ei,eij->ej', g.img_g.cpu().double(), c[gi])
    d = pos[lj] - pos[li]
    u = d - torch.einsum('ei,eij->ej', torch.round(torch.einsum('ei,eij->ej', d.detach(), inv[lj])), c[lj])
    if eps is not None:
        w = w + torch.einsum('ei,eij->ej', w, eps[batch[gi]])
        u = u + torch.einsum('ei,eij->ej', u, eps[batch[li]])
    a = torch.where((kind == 0).unsqueeze(1), u[e], -u[e])
    return w.pow(2).sum(-1).sqrt(), u.pow(2).sum(-1).sqrt(), O.angle_between(a, u[q])


@pytest.mark.gpu
def test_image_backward_kernels_vs_fp64_torch(dev):
    """pamnet_pos_bwd_img_f32 and pamnet_pos_bwd_img_virial_f32 called directly on the graph of the four small cells with random
    upstream gradients, against fp64 autograd through the explicit image vectors: dpos within KTOL = 1e-6 of the largest
    reference value, the virial of every graph within KTOL of its largest reference component, dpos of the virial form bitwise
    the plain form's, a second run bitwise the first.  The one-atom graph: zero force, non-zero virial."""
    from pamnet_amd import lib
    from test_hip_forces import KTOL
    assert KTOL == 1e-6
    inputs = _small()
    x, batch, pos, cell = inputs
    for r in (CUT_L, CUT_G):
        _assert_image_margin(_brute_small(r), r)
    g = _build(inputs, dev, need_grad=True, cell_images='all')
    want = _brute_image_lists(_brute_small(CUT_G))
    assert torch.equal(g.glob.ptr.cpu().long(), want[0]) and torch.equal(g.glob.col.cpu().long(), want[2])
    assert torch.equal(g.img_g.cpu().long(), want[3])
    n, ng, eg, el, tp = g.n, g.n_graphs, g.glob.m, g.loc.m, g.tp.m
    # the general transpose: entries grouped by column, a pointer array of its own
    assert torch.equal(g.glob.col[g.glob_T.perm.long()].cpu(), torch.sort(g.glob.col.cpu())[0])
    assert g.glob_T.ptr is not g.glob.ptr and torch.equal(g.glob_T.ptr, g.glob.ptr)      # (symmetric as a multiset: equal values)
    print('atoms', n, 'global', eg, 'local', el, 'rows', tp)
    assert el > 0 and tp > 0
    torch.manual_seed(2)
    ddg, ddl, dang = torch.randn(eg, device=dev), torch.randn(el, device=dev), torch.randn(tp, device=dev)
    P, st = lib.ptr, lib.stream_of(g.pos)
    work = torch.empty(3 * el, dtype=torch.float64, device=dev)
    head = [P(g.pos), P(g.cell_tab), P(g.node_graph), n, P(g.glob.ptr), P(g.glob.row_of), P(g.glob.col), P(g.img_g),
            P(g.glob_T.ptr), P(g.glob_T.perm), P(ddg), eg, P(g.loc.ptr), P(g.loc.row_of), P(g.loc.col), P(g.loc_T.ptr),
            P(g.loc_T.perm), P(ddl), el, P(g.tp.ptr), P(g.tp.row_of), P(g.tp.col), P(g.tp_kind), P(g.tp_T.ptr), P(g.tp_T.perm),
            P(dang), tp, P(work)]

    def plain():
        dpos = torch.full((n, 3), float('nan'), device=dev)
        lib.call(NEW[3], *head, P(dpos), st)
        torch.cuda.synchronize()
        return dpos

    def virial():
        dpos = torch.full((n, 3), float('nan'), device=dev)
        atom_work = torch.full((n, 9), float('nan'), dtype=torch.float64, device=dev)
        dstrain = torch.full((ng, 9), float('nan'), device=dev)
        lib.call(NEW[4], *head, P(dpos), P(g.gptr), ng, P(atom_work), P(dstrain), st)
        torch.cuda.synchronize()
        return dpos, dstrain

    dpos = plain()
    assert torch.equal(plain(), dpos)                             # fixed-order sums: bitwise reproducible
    dpos_v, dstrain = virial()
    again = virial()
    assert torch.equal(dpos_v, dpos) and torch.equal(again[0], dpos) and torch.equal(again[1], dstrain)
    assert torch.isfinite(dpos).all() and torch.isfinite(dstrain).all()
    p64 = pos.double().requires_grad_(True)
    eps = torch.zeros(ng, 3, 3, dtype=torch.float64, requires_grad=True)
    dg, dl, ang = _geometry64(g, p64, batch, cell, eps)
    e_dg, e_dl = maxnorm_err(g.dist_g.cpu().numpy(), dg.detach().numpy()), maxnorm_err(g.dist_l.cpu().numpy(), dl.detach().numpy())
    e_ang = maxnorm_err(g.tp_angle.cpu().numpy(), ang.detach().numpy())
    assert e_dg <= KTOL and e_dl <= KTOL and e_ang <= KTOL, (e_dg, e_dl, e_ang)
    total = (dg * ddg.cpu().double()).sum() + (dl * ddl.cpu().double()).sum() + (ang * dang.cpu().double()).sum()
    ref_p, ref_w = torch.autograd.grad(total, [p64, eps])
    e_pos = maxnorm_err(dpos.cpu().double().numpy(), ref_p.numpy())
    print('pos bwd err', e_pos)
    assert e_pos <= KTOL, e_pos
    W = dstrain.cpu().double().view(ng, 3, 3)
    for k in range(ng):
        scale = float(ref_w[k].abs().max())
        err = float((W[k] - ref_w[k]).abs().max()) / scale
        print('graph', k, 'virial scale', scale, 'err', err)
        assert scale > 0 and err <= KTOL, (k, err)
    assert bool((dpos[-1] == 0).all()) and float(ref_p[-1].abs().max()) < 1e-12 and float(W[-1].abs().max()) > 0


# -------------------------------------------------------------------------------------------- 5. interface and errors
def _free4():
    from pamnet_amd import synth
    b = synth.qm9_batch(0, 0, 4)
    return b, synth.Batch(**{k: v for k, v in b.__dict__.items() if k != 'edge_index'})


@pytest.mark.gpu
def test_image_refusals_say_what_to_do_instead(dev):
    import models
    from pamnet_amd import synth
    model = _model(False, 16, 1, dev)
    b, free = _free4()
    with torch.no_grad():
        for open_space in (b, free):                              # cell_images without cell
            data = open_space.to(dev)
            data.cell_images = 'all'
            with pytest.raises(ValueError, match='belongs to periodic batches'):
                model(data)
        periodic = _batch(*_small())
        for bad in ('every', 'ALL', 1, True):
            with pytest.raises(ValueError, match="'minimum'"):
                model(synth.Batch(cell_images=bad, **periodic.__dict__).to(dev))
        x, batch, pos, cell = _small()
        ok = synth.Batch(cell_images='all', **periodic.__dict__)
        assert torch.isfinite(model(ok.to(dev))).all()
        with pytest.raises(ValueError, match='heights'):          # without the attribute the old rule refuses these cells
            model(periodic.to(dev))
        low = cell.clone()
        low[0] = torch.eye(3) * 4.0                               # a height at 2 * cutoff_l
        with pytest.raises(ValueError, match=r'heights.*2 \* cutoff_l = 4.*cutoff_g / 4 = 1.25') as info:
            model(synth.Batch(cell_images='all', **_batch(x, batch, pos, low).__dict__).to(dev))
        assert 'all' in str(info.value)
        with pytest.raises(ValueError, match='heights'):
            model.prepare(synth.Batch(cell_images='all', **_batch(x, batch, pos, low).__dict__).to(dev), need_grad=False)
        # a height above 2 * cutoff_l and below cutoff_g / 4: only the image box refuses it
        thin_model = models.PAMNet(models.Config(dataset='QM9', dim=16, n_layer=1, cutoff_l=0.5, cutoff_g=CUT_G)).to(dev)
        thin = torch.tensor([[[1.2, 0.0, 0.0], [0.0, 20.0, 0.0], [0.0, 0.0, 20.0]]])
        one = synth.Batch(x=torch.zeros(1), batch=torch.zeros(1, dtype=torch.long), pos=torch.zeros(1, 3), cell=thin, num_graphs=1,
                          cell_images='all')
        with pytest.raises(ValueError, match=r'cutoff_g / 4 = 1.25'):
            thin_model(one.to(dev))
        # a cap that binds
        want = _brute_image_lists(_brute_small(CUT_G))
        most = int((want[0][1:] - want[0][:-1]).max())
        assert most > 8
        for cap in (8, most):
            model.max_num_neighbors = cap
            with pytest.raises(ValueError, match='raise model.max_num_neighbors'):
                model(ok.to(dev))
        model.max_num_neighbors = most + 1                        # (the atom itself counts)
        assert torch.isfinite(model(ok.to(dev))).all()
        sized = ok.to(dev)
        sized.sizes = (10, 10, 10)
        with pytest.raises(ValueError, match='sizes'):
            model(sized)


@pytest.mark.gpu
def test_the_box_and_the_cap_bit(dev):
    """pamnet_cell_images_i32 on its own: ceil(cutoff / height) per direction; a height below cutoff / 4 raises bit 128 and
    empties that graph's box, the word is ORed into; the count pass raises bit 64 for a row above the cap and cuts nothing."""
    from pamnet_amd import graph as G
    cells = torch.tensor([[[4.5, 0, 0], [0, 12.0, 0], [0, 0, 1.3]], [[1.2, 0, 0], [0, 6.0, 0], [0, 0, 6.0]],
                          [[4.5, 0, 0], [1.0, 4.75, 0], [-0.75, 0.875, 5.0]], [[5.0, 0, 0], [0, 2.5, 0], [0, 0, 1.25]]])
    flag = torch.tensor([1], dtype=torch.int32, device=dev)
    tab = G.cell_table(cells.to(dev).view(-1, 9), 0.5, flag)
    assert int(flag) == 1
    box = G.cell_images(tab, CUT_G, flag)
    assert int(flag) == (1 | PBC_BIT)
    assert box.cpu().tolist() == [[2, 1, 4], [0, 0, 0], [2, 2, 1], [1, 2, 4]]
    flag.zero_()
    G.cell_images(tab[2:], CUT_G, flag)
    assert int(flag) == 0
    x, batch, pos, cell = _small()
    want = _brute_image_lists(_brute_small(CUT_G))
    most = int((want[0][1:] - want[0][:-1]).max())
    for cap, bit in ((most, CAP_BIT), (most + 1, 0), (0, 0)):     # (the query itself counts: most + 1 hits)
        got, _, flag = _search(x, batch, pos, cell, CUT_G, dev, max_nb=cap)
        assert flag == bit, (cap, flag)
        assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])


@pytest.mark.gpu
def test_without_the_attribute_none_of_the_new_entry_points_is_called(dev, monkeypatch):
    """A periodic batch without `cell_images`, with None or with 'minimum', and a batch without cell: the same entry points and
    the same bits; prepare + forward gives the bits of the forward alone, in 'all' mode too."""
    from pamnet_amd import synth
    b, free = _free4()
    cell = (torch.eye(3) * 40.0).expand(4, 3, 3).contiguous()
    calls = _record(monkeypatch)
    for dim in (128, 16):
        model = _model(False, dim, 1, dev)
        ref = None
        for attrs in ({}, {'cell_images': None}, {'cell_images': 'minimum'}):
            bt = synth.Batch(cell=cell, **free.__dict__)
            del calls[:]
            out = _run(model, bt, dev, True, **attrs)
            seen = list(calls)
            assert not [c for c in seen if c in NEW] and 'pamnet_pos_bwd_pbc_virial_f32' in seen, seen
            if ref is None:
                ref = out
            assert all(torch.equal(u, v) for u, v in zip(out[:3], ref[:3]))
        del calls[:]
        for bt in (b, free):
            data = bt.to(dev)
            data.pos.requires_grad_(True)
            model(data).sum().backward()
        assert 'pamnet_pos_bwd_f32' in calls and not [c for c in calls if c in NEW], calls
        # prepare + forward = forward
        small = synth.Batch(cell_images='all', **_batch(*_small()).__dict__)
        o1, f1, w1, _ = _run(model, small, dev, True)
        data = small.to(dev)
        data.pos = data.pos.detach().clone().requires_grad_(True)
        data.strain = torch.zeros(4, 3, 3, device=dev, requires_grad=True)
        del calls[:]
        model.prepare(data)
        assert [c for c in calls if c in NEW] == list(NEW[:3])
        out = model(data)
        f2, w2 = torch.autograd.grad(out.sum(), [data.pos, data.strain])
        assert torch.equal(out.detach(), o1) and torch.equal(f2, f1) and torch.equal(w2, w1)
        with torch.no_grad():
            model.prepare(small.to(dev), need_grad=False)
            assert torch.equal(model(small.to(dev)), o1)


@pytest.mark.gpu
def test_trainer_and_predict_take_such_batches(dev):
    """Trainer.step(next_data=) (graphs built on the side stream), Trainer.evaluate and train.predict on the small cells: the
    losses of the prefetched steps equal those of plain steps, predictions equal the model's own forward."""
    import models
    from oracle import pamnet_oracle as O
    from pamnet_amd import synth, train
    cfg = models.Config(dataset='QM9', dim=128, n_layer=1, cutoff_l=CUT_L, cutoff_g=CUT_G)
    sd = O.init_state_dict(cfg, seed=3)
    y = torch.linspace(-1.0, 1.0, 4)
    batches = [synth.Batch(cell_images='all', y=y * (k + 1), **_batch(*_small()).__dict__) for k in range(3)]

    def run(prefetch):
        model = models.PAMNet(cfg)
        model.load_state_dict(sd, strict=True)
        model = model.to(dev)
        tr = train.Trainer(model, lr=1e-3)
        data = [bt.to(dev) for bt in batches]
        losses = [float(tr.step(data[k], next_data=data[k + 1] if (prefetch and k + 1 < len(data)) else None))
                  for k in range(len(data))]
        tr.close()
        torch.cuda.synchronize()
        return losses, model

    losses_p, model = run(True)
    losses_o, _ = run(False)
    assert all(math.isfinite(v) for v in losses_p) and losses_p == losses_o, (losses_p, losses_o)
    with torch.no_grad():
        want = model(batches[0].to(dev))
    outs = [out.clone() for _, out in train.predict(model, [bt.to(dev) for bt in batches])]
    assert len(outs) == 3 and all(torch.equal(o, want) for o in outs)                 # (the three batches share x, pos, cell)
    tr = train.Trainer(model, lr=1e-3)
    mae = tr.evaluate([bt.to(dev) for bt in batches[:2]])
    tr.close()
    assert abs(mae - float(((want.cpu() - batches[0].y).abs().sum() + (want.cpu() - batches[1].y).abs().sum()) / 8)) < 1e-5


@pytest.mark.gpu
def test_image_entry_points_validate_their_arguments(dev):
    """EINVAL / ENULL with nothing launched (the two backward forms answer EINVAL for a null pointer, as their twins do)."""
    from pamnet_amd import lib
    P = lib.ptr
    i32 = lambda n, v=7: torch.full((n,), v, dtype=torch.int32, device=dev)
    pos = torch.zeros((4, 3), device=dev)
    tab = torch.full((1, 18), 7.0, dtype=torch.float64, device=dev)
    box, flag, ng, gptr = i32(3), i32(1, 0), i32(4, 0), torch.tensor([0, 4], dtype=torch.int32, device=dev)
    count, ptr, nbr, img = i32(4), i32(5, 0), i32(8), i32(24)
    dist = torch.full((8,), 7.0, device=dev)
    st = lib.stream_of(pos)

    def images(t=tab, n=1, r=5.0, b=box, f=flag):
        lib.call(NEW[0], P(t), n, r, P(b), P(f), st)

    def count_(p=pos, t=tab, b=box, g=ng, gp=gptr, n=4, n_g=1, mx=0, c=count):
        lib.call(NEW[1], P(p), P(t), P(b), P(g), P(gp), n, n_g, 5.0, mx, P(c), P(flag), st)

    def fill(p=pos, t=tab, b=box, g=ng, gp=gptr, n=4, n_g=1, mx=0, pt=ptr, nb=nbr, d=dist, im=img, cap=8):
        lib.call(NEW[2], P(p), P(t), P(b), P(g), P(gp), n, n_g, 5.0, mx, P(pt), P(nb), P(d), None, P(im), cap, st)

    work, dpos = torch.full((24,), 7.0, dtype=torch.float64, device=dev), torch.full((4, 3), 7.0, device=dev)
    atom_work, dstrain = torch.full((36,), 7.0, dtype=torch.float64, device=dev), torch.full((1, 9), 7.0, device=dev)

    def head(p, t, g, n, im, eg, el, tp, w, o):
        return [P(p), P(t), P(g), n, P(ptr), P(nbr), P(nbr), P(im), P(ptr), P(nbr), P(dist), eg, P(ptr), P(nbr), P(nbr), P(ptr),
                P(nbr), P(dist), el, P(ptr), P(nbr), P(nbr), P(nbr), P(ptr), P(nbr), P(dist), tp, P(w), P(o)]

    def bwd(p=pos, t=tab, g=ng, n=4, im=img, eg=2, el=2, tp=2, w=work, o=dpos):
        lib.call(NEW[3], *head(p, t, g, n, im, eg, el, tp, w, o), st)

    def bwd_v(p=pos, t=tab, g=ng, n=4, im=img, eg=2, el=2, tp=2, w=work, o=dpos, gp=gptr, n_g=1, aw=atom_work, ds=dstrain):
        lib.call(NEW[4], *head(p, t, g, n, im, eg, el, tp, w, o), P(gp), n_g, P(aw), P(ds), st)

    cases = [(images, [dict(n=-1), dict(r=0.0), dict(r=-1.0), dict(r=float('nan')), dict(r=float('inf'))], 'EINVAL'),
             (images, [dict(t=None), dict(b=None), dict(f=None)], 'ENULL'),
             (count_, [dict(n=-1), dict(n_g=-1), dict(mx=-1), dict(mx=1 << 31)], 'EINVAL'),
             (count_, [dict(p=None), dict(t=None), dict(b=None), dict(g=None), dict(gp=None), dict(c=None)], 'ENULL'),
             (fill, [dict(n=-1), dict(n_g=-1), dict(mx=-1), dict(cap=-1)], 'EINVAL'),
             (fill, [dict(p=None), dict(t=None), dict(b=None), dict(g=None), dict(gp=None), dict(pt=None), dict(nb=None),
                     dict(d=None), dict(im=None)], 'ENULL'),
             (bwd, [dict(n=-1), dict(eg=-1), dict(el=-1), dict(tp=-1), dict(p=None), dict(t=None), dict(g=None), dict(im=None),
                    dict(w=None), dict(o=None)], 'EINVAL'),
             (bwd_v, [dict(n=-1), dict(eg=-1), dict(el=-1), dict(tp=-1), dict(n_g=-1), dict(p=None), dict(t=None), dict(g=None),
                      dict(im=None), dict(w=None), dict(o=None), dict(gp=None), dict(aw=None), dict(ds=None)], 'EINVAL')]
    for fn, kws, what in cases:
        for kw in kws:
            with pytest.raises(RuntimeError, match=what):
                fn(**kw)
    torch.cuda.synchronize()
    for t in (tab, box, count, nbr, img, dist, work, dpos, atom_work, dstrain):       # nothing was launched
        assert bool((t == 7).all())
    assert int(flag) == 0
