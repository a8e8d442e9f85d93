"""Periodic cells: a bond-free QM9-schema batch that carries `cell` (fp32 [num_graphs, 3, 3], row k = lattice vector a_k) gets
minimum-image graphs and forces -- pamnet_amd/graph.py build_graph(cell=), csrc/geom_core.h min_image, and the five entry points
pamnet_cell_prepare_f64, pamnet_radius_pbc_count/fill_i32, pamnet_triplet_fill_pbc_f32, pamnet_pos_bwd_pbc_f32.

The fp64 references are brute-force torch written here: the minimum image of every pair by rounding its fractional displacement
(torch.round: half to even, as rint).  The oracle has no periodic path; test 4 feeds it unwrapped coordinates.  Every list
test asserts its precondition first: no pair within 1e-4 of the cutoff under test, so that fp32 and fp64 agree on the edge set.

Parity protocol and constants: tests/test_hip_forces.py (TOL, GRAD_TOL, CANCEL_TOL, KTOL, _ok, _check_gradients)."""
import numpy as np
import pytest
import torch

from conftest import maxnorm_err

NEW = ('pamnet_cell_prepare_f64', 'pamnet_radius_pbc_count_i32', 'pamnet_radius_pbc_fill_i32', 'pamnet_triplet_fill_pbc_f32',
       'pamnet_pos_bwd_pbc_f32')
PBC_BIT, CAP_BIT = 128, 64
CUBE = [[10.5, 0.0, 0.0], [0.0, 10.5, 0.0], [0.0, 0.0, 10.5]]
BOX = [[10.5, 0.0, 0.0], [0.0, 12.0, 0.0], [0.0, 0.0, 11.0]]
# off-diagonal components of both signs; every entry a multiple of 1/8 (test 5 needs lattice sums that are exact in fp32)
TRI_A = [[11.5, 0.0, 0.0], [2.0, 11.5, 0.0], [-1.5, 1.75, 11.5]]
TRI_B = [[12.0, 0.0, 0.0], [-2.5, 11.75, 0.0], [1.75, -2.25, 11.625]]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs an MI355X'
    from pamnet_amd import lib
    lib.load()
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------ fp64 brute force (CPU)
def _heights(cell):
    c = torch.as_tensor(cell, dtype=torch.float64)
    det = torch.linalg.det(c).abs()
    return [float(det / torch.linalg.cross(c[(k + 1) % 3], c[(k + 2) % 3]).norm()) for k in range(3)]


def _min_image(p, cell):
    """p [n, 3], cell [3, 3] (fp64) -> (v [n, n, 3] with v[a, b] = minimum image of p_a - p_b, image integers [n, n, 3])."""
    d = p[:, None, :] - p[None, :, :]
    n = torch.round(d @ torch.linalg.inv(cell))
    return d - n @ cell, n


def _slices(batch):
    cnt = torch.bincount(batch)
    ptr = torch.cat([cnt.new_zeros(1), cnt.cumsum(0)]).tolist()
    return list(zip(ptr[:-1], ptr[1:]))


def _brute(pos, batch, cell):
    """Per graph: (first node, minimum-image vectors, image integers, distances), all fp64 from the fp32 inputs."""
    out = []
    for g, (s, e) in enumerate(_slices(batch)):
        v, n = _min_image(pos[s:e].double(), cell[g].double())
        out.append((s, v, n, v.pow(2).sum(-1).sqrt()))
    return out


def _assert_margin(brute, r):
    for s, v, n, d in brute:
        off = d[~torch.eye(d.size(0), dtype=torch.bool)]
        assert float((off - r).abs().min()) > 1e-4, (s, r, float((off - r).abs().min()))
        assert float(off.min()) > 0.0


def _brute_lists(brute, r, max_nb=0):
    """(ptr, row_of, nbr, dist) of the radius graph at r: rows by query, ascending neighbour, self excluded; max_nb > 0: a
    query keeps its first max_nb hits in ascending index order, itself counted.  Third value: whether the cap cut a row."""
    rows, cols, dist, cut = [], [], [], False
    for s, v, n, d in brute:
        hit = d <= r
        hit.fill_diagonal_(True)                              # the query is a hit of its own search
        if max_nb:
            keep = hit & (hit.long().cumsum(1) <= max_nb)
            cut = cut or bool((keep != hit).any())
            hit = keep
        hit.fill_diagonal_(False)
        q, j = hit.nonzero(as_tuple=True)
        rows.append(q + s), cols.append(j + s), dist.append(d[q, j])
    rows, cols, dist = torch.cat(rows), torch.cat(cols), torch.cat(dist)
    total = sum(v.size(0) for _, v, _, _ in brute)
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.bincount(rows, minlength=total).cumsum(0)])
    return (ptr, rows, cols, dist), cut


# ------------------------------------------------------------------------------------------------------------- inputs
def _scatter(gen, n, cell, min_sep, grid=None):
    """n points uniform in the cell with pairwise minimum-image separation >= min_sep (rejection, fp64); `grid`: coordinates
    rounded to multiples of it."""
    cell = torch.as_tensor(cell, dtype=torch.float64)
    pts = []
    while len(pts) < n:
        p = torch.rand(3, generator=gen, dtype=torch.float64) @ cell
        if grid:
            p = torch.round(p / grid) * grid
        if pts:
            q = torch.stack(pts + [p])
            v, _ = _min_image(q, cell)
            if float(v[-1, :-1].pow(2).sum(-1).sqrt().min()) < min_sep:
                continue
        pts.append(p)
    return torch.stack(pts)


_INPUTS = {}


def _inputs(name):
    """(x, batch, pos fp32, cell fp32 [G, 3, 3]) of the kernel-level cases, made once on the CPU and never modified.
    'a': 37 + 50 atoms (one thread per node) in a 10.5 cube and a 10.5 x 12 x 11 box; 'b': 150 + 101 atoms (one wavefront per
    node: the average is >= 96, neither count a multiple of 64) in two triclinic cells, the second graph's atoms displaced by
    several lattice vectors (unwrapped input)."""
    if name in _INPUTS:
        return _INPUTS[name]
    counts, cells, seed = {'a': ((37, 50), (CUBE, BOX), 3), 'b': ((150, 101), (TRI_A, TRI_B), 5)}[name]
    gen = torch.Generator().manual_seed(seed)
    pos = [_scatter(gen, n, c, 0.8) for n, c in zip(counts, cells)]
    cell = torch.tensor(cells, dtype=torch.float32)
    if name == 'b':
        assert min(min(_heights(c)) for c in cells) >= 10.4
        assert all(any(c[i][j] > 0 for i in range(3) for j in range(3) if i != j)
                   and any(c[i][j] < 0 for i in range(3) for j in range(3) if i != j) for c in cells)
        shift = torch.randint(-3, 4, (counts[1], 3), generator=gen).double()
        assert int(shift.abs().max()) == 3
        pos[1] = pos[1] + shift @ cell[1].double()
    pos = torch.cat(pos).float()
    batch = torch.cat([torch.full((n,), g, dtype=torch.long) for g, n in enumerate(counts)])
    x = torch.randint(0, 5, (batch.numel(),), generator=gen).float()
    n_total, n_graphs = int(batch.numel()), len(counts)
    assert (n_total >= 96 * n_graphs) == (name == 'b') and all(n % 64 for n in counts)
    _INPUTS[name] = (x, batch, pos, cell)
    return _INPUTS[name]


_BRUTE = {}


def _brute_of(name):
    if name not in _BRUTE:
        x, batch, pos, cell = _inputs(name)
        _BRUTE[name] = _brute(pos, batch, cell)
    return _BRUTE[name]


def _table(cell, cutoff, dev):
    """(cell table, flag word after the prepare launch) for a cell tensor on the CPU."""
    from pamnet_amd import graph as G
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    tab = G.cell_table(cell.to(dev).contiguous().view(-1, 9), cutoff, flag)
    return tab, flag


def _search(name, r, dev, max_nb=0):
    """pamnet_radius_pbc_count/fill_i32 called directly: (ptr, row_of, nbr, dist) on the CPU and the flag word."""
    from pamnet_amd import graph as G
    x, batch, pos, cell = _inputs(name)
    tab, flag = _table(cell, r, dev)
    node_graph = batch.to(dev).to(torch.int32)
    gptr = torch.tensor([s for s, _ in _slices(batch)] + [int(batch.numel())], dtype=torch.int32, device=dev)
    p = pos.to(dev).contiguous()
    ptr = G.radius_count(p, node_graph, gptr, r, max_nb, flag, cell_tab=tab)
    rows = []
    ptr, nbr, dist = G.radius_fill(p, node_graph, gptr, r, ptr, int(ptr[-1]), rows_out=rows, max_neighbors=max_nb, cell_tab=tab)
    torch.cuda.synchronize()
    return ptr.cpu().long(), rows[0].cpu().long(), nbr.cpu().long(), dist.cpu(), int(flag)


# ------------------------------------------------------------------------------------------ 1. lists against brute force
@pytest.mark.gpu
@pytest.mark.parametrize('name', ['a', 'b'])
@pytest.mark.parametrize('r', [5.0, 2.0])
def test_radius_lists_match_brute_force(dev, monkeypatch, name, r):
    """ptr / nbr / row_of exactly, lengths within 1e-6 relative of fp64, and every edge has its reverse with a bitwise equal
    length -- the thread-per-node form ('a') and the wavefront form ('b', unwrapped input in one graph)."""
    brute = _brute_of(name)
    _assert_margin(brute, r)
    (ptr, rows, cols, dist), _ = _brute_lists(brute, r)
    calls = _record(monkeypatch)
    g_ptr, g_rows, g_nbr, g_dist, flag = _search(name, r, dev)
    assert [c for c in calls if c in NEW] == list(NEW[:3]), calls
    assert flag == 0
    assert torch.equal(g_ptr, ptr) and torch.equal(g_rows, rows) and torch.equal(g_nbr, cols)
    rel = float(((g_dist.double() - dist).abs() / dist).max())
    print(name, r, 'edges', int(rows.numel()), 'length rel err', rel)
    assert rel <= 1e-6, rel
    n = int(ptr.numel()) - 1
    order = (cols * n + rows).argsort()                      # the reverse edge of (row, col) is (col, row)
    assert torch.equal(rows[order], cols) and torch.equal(cols[order], rows)          # (row-major lists: symmetric graph)
    assert torch.equal(g_dist.view(torch.int32)[order], g_dist.view(torch.int32))
    crossing = sum(int((nn[(d <= r)].abs().sum(-1) > 0).sum()) for _, _, nn, d in brute)
    assert crossing > 0                                      # (edges across a face exist)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['a', 'b'])
def test_capped_search_keeps_the_first_hits_and_raises_the_cap_bit(dev, name):
    """max_neighbors = 8 at r = 5.0: every row is the first 8 hits in ascending index order, the query itself counted."""
    brute = _brute_of(name)
    _assert_margin(brute, 5.0)
    (ptr, rows, cols, dist), cut = _brute_lists(brute, 5.0, max_nb=8)
    assert cut
    g_ptr, g_rows, g_nbr, g_dist, flag = _search(name, 5.0, dev, max_nb=8)
    assert flag == CAP_BIT
    assert torch.equal(g_ptr, ptr) and torch.equal(g_rows, rows) and torch.equal(g_nbr, cols)
    assert float(((g_dist.double() - dist).abs() / dist).max()) <= 1e-6


@pytest.mark.gpu
def test_cell_table_and_its_verdict(dev):
    """The table holds the cell and its fp64 inverse; a too-small cell and a singular cell raise bit 128 and nothing else."""
    good = torch.tensor([CUBE, TRI_A, TRI_B], dtype=torch.float32)
    tab, flag = _table(good, 5.0, dev)
    assert int(flag) == 0
    t = tab.cpu().view(3, 2, 3, 3)
    assert torch.equal(t[:, 0], good.double())
    assert float((t[:, 1] - torch.linalg.inv(good.double())).abs().max()) < 1e-15
    assert min(_heights(TRI_A)) > 10.4 > 10.0
    for r, want in ((5.2, 0), (5.25, PBC_BIT), (5.3, PBC_BIT)):          # the cube's heights are 10.5: 2 r must stay below
        assert int(_table(good, r, dev)[1]) == want, r
    small = torch.tensor([CUBE, [[9.0, 0, 0], [0, 30.0, 0], [0, 0, 30.0]]], dtype=torch.float32)
    assert int(_table(small, 5.0, dev)[1]) == PBC_BIT
    sheared = torch.tensor([[[30.0, 0, 0], [29.0, 9.0, 0], [0, 0, 30.0]]], dtype=torch.float32)      # long vectors, height 9
    assert int(_table(sheared, 5.0, dev)[1]) == PBC_BIT
    singular = torch.tensor([CUBE, [[10.5, 0, 0], [21.0, 0, 0], [0, 0, 10.5]]], dtype=torch.float32)
    tab, flag = _table(singular, 5.0, dev)
    assert int(flag) == PBC_BIT and bool(torch.isfinite(tab).all())
    nan = torch.tensor([[[float('nan'), 0, 0], [0, 20.0, 0], [0, 0, 20.0]]], dtype=torch.float32)
    assert int(_table(nan, 5.0, dev)[1]) == PBC_BIT
    pre = torch.tensor([1 | CAP_BIT], dtype=torch.int32, device=dev)                  # ORed into the word, never zeroed
    from pamnet_amd import graph as G
    G.cell_table(small.to(dev).view(-1, 9), 5.0, pre)
    assert int(pre) == (1 | CAP_BIT | PBC_BIT)


# ------------------------------------------------------------------------- 2. angles and position backward, fp64 torch
KTOL = 1e-6


def _build(name, dev, cutoff_l=2.0, cutoff_g=5.0, **kw):
    from pamnet_amd import graph as G
    x, batch, pos, cell = _inputs(name)
    return G.build_graph('QM9', cutoff_l, cutoff_g, 'source_to_target', x.to(dev), batch.to(dev), pos.to(dev), None,
                         num_graphs=int(cell.size(0)), n_types=5, cell=cell.to(dev), **kw)


def _geometry64(g, pos, batch, cell, images=None):
    """fp64 torch statement of the periodic geometry on g's index lists: (dist_g, dist_l, angles, image integers of the
    global edges / of the local edges).  `images`: hold these integers fixed instead of recomputing them (the backward's
    reference: the image does not depend on the positions differentiably)."""
    from oracle import pamnet_oracle as O
    c = cell.double()[batch]                                 # [N, 3, 3]: the cell of every atom's graph
    inv = torch.linalg.inv(c)

    def disp(a, b, n=None):                                  # minimum image of p_a - p_b
        d = pos[a] - pos[b]
        if n is None:
            n = torch.round(torch.einsum('ei,eij->ej', d.detach(), inv[a]))
        return d - torch.einsum('ei,eij->ej', n, c[a]), n

    gi, gc = g.glob.row_of.long().cpu(), g.glob.col.long().cpu()
    li, lj = g.loc.row_of.long().cpu(), g.loc.col.long().cpu()
    e, q, kind = g.tp.row_of.long().cpu(), g.tp.col.long().cpu(), g.tp_kind.cpu()
    w, n_g = disp(gi, gc, None if images is None else images[0])
    u, n_l = disp(lj, li, None if images is None else images[1])
    a = torch.where((kind == 0).unsqueeze(1), u[e], -u[e])
    return w.pow(2).sum(-1).sqrt(), u.pow(2).sum(-1).sqrt(), O.angle_between(a, u[q]), (n_g, n_l)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['a', 'b'])
def test_angles_and_position_backward_vs_fp64_torch(dev, name):
    """pamnet_triplet_fill_pbc_f32 against atan2(|a x b|, a.b) of the fp64 minimum-image vectors, pamnet_pos_bwd_pbc_f32
    against torch.autograd.grad of that geometry (image integers held fixed) with random upstream gradients; both within
    KTOL = 1e-6 of the largest reference value, the bound of the non-periodic twins (tests/test_hip_forces.py)."""
    from pamnet_amd import graph as G, lib
    from test_hip_forces import KTOL as TWIN_KTOL
    assert KTOL == TWIN_KTOL == 1e-6
    x, batch, pos, cell = _inputs(name)
    brute = _brute_of(name)
    _assert_margin(brute, 2.0), _assert_margin(brute, 5.0)
    g = _build(name, dev, need_grad=True)
    (lptr, lrows, lcols, _), _ = _brute_lists(brute, 2.0)
    assert torch.equal(g.loc.ptr.cpu().long(), lptr) and torch.equal(g.loc.col.cpu().long(), lcols)
    (gptr, grows, gcols, _), _ = _brute_lists(brute, 5.0)
    assert torch.equal(g.glob.ptr.cpu().long(), gptr) and torch.equal(g.glob.col.cpu().long(), gcols)
    p64 = pos.double().requires_grad_(True)
    dg, dl, ang, (n_g, n_l) = _geometry64(g, p64, batch, cell)
    # some local edges, and some triplets, cross a cell face
    e, q, kind = g.tp.row_of.long().cpu(), g.tp.col.long().cpu(), g.tp_kind.cpu()
    cross_l = n_l.abs().sum(-1) > 0
    cross_t = (kind == 0) & (cross_l[e] | cross_l[q])
    print(name, 'local edges', g.loc.m, 'crossing', int(cross_l.sum()), 'triplets', int((kind == 0).sum()), 'crossing',
          int(cross_t.sum()), 'global crossing', int((n_g.abs().sum(-1) > 0).sum()))
    assert int(cross_l.sum()) > 0 and int(cross_t.sum()) > 0 and int((n_g.abs().sum(-1) > 0).sum()) > 0
    # the fill called directly on g's lists
    tot = g.tp.m
    tp_idx, tp_edge, tp_kind = (torch.empty(tot, dtype=torch.int32, device=dev) for _ in range(3))
    angle = torch.empty(tot, device=dev)
    lib.call('pamnet_triplet_fill_pbc_f32', lib.ptr(g.pos), lib.ptr(g.cell_tab), lib.ptr(g.node_graph), lib.ptr(g.loc.ptr),
             lib.ptr(g.loc.col), lib.ptr(g.loc.row_of), g.loc.m, 1, lib.ptr(g.tp.ptr), lib.ptr(tp_idx), lib.ptr(tp_edge),
             lib.ptr(angle), lib.ptr(tp_kind), tot, lib.stream_of(angle))
    torch.cuda.synchronize()
    assert torch.equal(angle, g.tp_angle) and torch.equal(tp_idx, g.tp.col) and torch.equal(tp_kind, g.tp_kind)
    e_ang = maxnorm_err(angle.cpu().numpy(), ang.detach().numpy())
    e_dl = maxnorm_err(g.dist_l.cpu().numpy(), dl.detach().numpy())
    e_dg = maxnorm_err(g.dist_g.cpu().numpy(), dg.detach().numpy())
    print(name, 'angle err', e_ang, 'dist_l err', e_dl, 'dist_g err', e_dg)
    assert e_ang <= KTOL and e_dl <= KTOL and e_dg <= KTOL, (e_ang, e_dl, e_dg)
    # the backward
    torch.manual_seed(2)
    ddg, ddl, dang = torch.randn(g.glob.m, device=dev), torch.randn(g.loc.m, device=dev), torch.randn(tot, device=dev)
    work = torch.empty(3 * g.loc.m, dtype=torch.float64, device=dev)
    dpos = torch.empty(g.n, 3, device=dev)

    def run(out):
        lib.call('pamnet_pos_bwd_pbc_f32', lib.ptr(g.pos), lib.ptr(g.cell_tab), lib.ptr(g.node_graph), g.n, lib.ptr(g.glob.ptr),
                 lib.ptr(g.glob.row_of), lib.ptr(g.glob.col), lib.ptr(g.glob_T.ptr), lib.ptr(g.glob_T.perm), lib.ptr(ddg),
                 g.glob.m, lib.ptr(g.loc.ptr), lib.ptr(g.loc.row_of), lib.ptr(g.loc.col), lib.ptr(g.loc_T.ptr),
                 lib.ptr(g.loc_T.perm), lib.ptr(ddl), g.loc.m, lib.ptr(g.tp.ptr), lib.ptr(g.tp.row_of), lib.ptr(g.tp.col),
                 lib.ptr(g.tp_kind), lib.ptr(g.tp_T.ptr), lib.ptr(g.tp_T.perm), lib.ptr(dang), tot, lib.ptr(work), lib.ptr(out),
                 lib.stream_of(out))
        torch.cuda.synchronize()
    run(dpos)
    again = torch.empty_like(dpos)
    run(again)
    assert torch.equal(dpos, again)                          # fixed-order sums: bitwise reproducible
    ref, = torch.autograd.grad((dg * ddg.cpu().double()).sum() + (dl * ddl.cpu().double()).sum()
                               + (ang * dang.cpu().double()).sum(), p64)
    assert torch.isfinite(dpos).all() and torch.isfinite(ref).all()
    e_pos = maxnorm_err(dpos.cpu().double().numpy(), ref.numpy())
    print(name, 'pos bwd err', e_pos)
    assert e_pos <= KTOL, e_pos


# ----------------------------------------------------------------------------------------- 3. no wrap means the same bits
def _arrays(g):
    """Every index / geometry array of a graph, by name."""
    out = {'dist_g': g.dist_g, 'dist_l': g.dist_l, 'tp_angle': g.tp_angle, 'tp_kind': g.tp_kind}
    for name in ('glob', 'loc', 'tp'):
        c = getattr(g, name)
        out.update({name + '.ptr': c.ptr, name + '.row_of': c.row_of, name + '.col': c.col})
    for name in ('glob_T', 'loc_T', 'tp_T'):
        t = getattr(g, name)
        if t.ptr is not None:
            out.update({name + '.ptr': t.ptr, name + '.perm': t.perm})
    for name in ('tT_edge', 'tT_node', 'types', 'gptr', 'node_graph'):
        if getattr(g, name, None) is not None:
            out[name] = getattr(g, name)
    return out


def _free16():
    """synth.qm9_batch(0, 0, 16) without its bond list (|pos| <= 4.57: inside a 40 A cube no pair wraps)."""
    from pamnet_amd import synth
    b = synth.qm9_batch(0, 0, 16)
    assert float(b.pos.abs().max()) <= 4.57
    return synth.Batch(**{k: v for k, v in b.__dict__.items() if k != 'edge_index'})


def _with_cell(b, cell):
    from pamnet_amd import synth
    return synth.Batch(cell=cell, **b.__dict__)


def _record(monkeypatch):
    """Record the symbols passed to lib.call from here on."""
    from pamnet_amd import lib
    calls, real = [], lib.call

    def rec(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(lib, 'call', rec)
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize('small,dim', [(False, 128), (True, 32)])
def test_cells_nothing_wraps_in_give_the_same_bits(dev, monkeypatch, small, dim):
    """40 A cubes around molecules of |pos| <= 4.57: every array of the Graph, the output, the forces and all parameter
    gradients are torch.equal to the run without `cell` -- and the periodic run really took the periodic kernels."""
    import models
    from pamnet_amd import graph as G
    torch.manual_seed(0)
    cfg = models.Config(dataset='QM9', dim=dim, n_layer=2, cutoff_l=1.7, cutoff_g=5.0)
    model = (models.PAMNet_s if small else models.PAMNet)(cfg).to(dev)
    plain = _free16()
    cell = (torch.eye(3) * 40.0).expand(16, 3, 3).contiguous()
    calls = _record(monkeypatch)

    def graph(b):
        d = b.to(dev)
        return G.build_graph('QM9', 1.7, 5.0, 'source_to_target', d.x, d.batch, d.pos, None, num_graphs=16, n_types=5,
                             with_triplets=not small, cell=getattr(d, 'cell', None))
    ga = graph(plain)
    assert not [c for c in calls if c in NEW], calls
    del calls[:]
    gb = graph(_with_cell(plain, cell))
    assert [c for c in calls if c in NEW] == [NEW[0], NEW[1], NEW[1], NEW[2], NEW[2], NEW[3]], calls
    assert not [c for c in calls if c in ('pamnet_radius_count_i32', 'pamnet_radius_fill_i32', 'pamnet_triplet_fill_f32')
                or c.startswith('pamnet_mol_graph') or c.startswith('pamnet_graph_')], calls
    xa, xb = _arrays(ga), _arrays(gb)
    assert xa.keys() == xb.keys()
    for k in xa:
        assert xa[k].dtype == xb[k].dtype and torch.equal(xa[k], xb[k]), k
    assert ga.cell_tab is None and gb.cell_tab is not None

    def run(b, forces):
        data = b.to(dev)
        model.zero_grad(set_to_none=True)
        del calls[:]
        if forces:
            data.pos.requires_grad_(True)
            out = model(data)
            out.sum().backward()
        else:
            out = model(data)
            torch.nn.functional.l1_loss(out, data.y).backward()
        used = [c for c in calls if c in NEW]
        grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
        return out.detach().clone(), (data.pos.grad.detach().clone() if forces else None), grads, used

    for forces in (True, False):
        out_a, f_a, gr_a, used_a = run(plain, forces)
        out_b, f_b, gr_b, used_b = run(_with_cell(plain, cell), forces)
        assert not used_a and (NEW[4] in used_b) == forces and NEW[3] in used_b, (used_a, used_b)
        assert torch.equal(out_a, out_b)
        if forces:
            assert torch.isfinite(f_a).all() and float(f_a.abs().max()) > 0 and torch.equal(f_a, f_b)
        assert gr_a.keys() == gr_b.keys() and len(gr_a) > 0
        for k in gr_a:
            assert torch.equal(gr_a[k], gr_b[k]), k


@pytest.mark.gpu
def test_trainer_steps_under_such_cells_leave_the_same_parameters(dev):
    """Three Trainer.step calls with next_data= (graphs built on the side stream): a state_dict torch.equal to the run
    without cells."""
    import models
    from oracle import pamnet_oracle as O
    from pamnet_amd import synth, train
    cfg = models.Config(dataset='QM9', dim=128, n_layer=2, cutoff_l=1.7, cutoff_g=5.0)
    sd = O.init_state_dict(cfg, seed=3)
    batches = []
    for k in range(3):
        b = synth.qm9_batch(0, 16 * k, 16)
        assert float(b.pos.abs().max()) < 10.0                        # (40 A cubes: nothing wraps)
        batches.append(synth.Batch(**{key: v for key, v in b.__dict__.items() if key != 'edge_index'}))
    cell = (torch.eye(3) * 40.0).expand(16, 3, 3).contiguous()

    def run(periodic):
        model = models.PAMNet(cfg)
        model.load_state_dict(sd, strict=True)
        model = model.to(dev)
        tr = train.Trainer(model, lr=1e-3)
        data = [(_with_cell(b, cell) if periodic else b).to(dev) for b in batches]
        losses = [tr.step(data[k], next_data=data[k + 1] if k + 1 < len(data) else None) for k in range(len(data))]
        tr.close()
        torch.cuda.synchronize()
        return [float(v) for v in losses], {k: v.detach().clone() for k, v in model.state_dict().items()}

    losses_p, sd_p = run(True)
    losses_o, sd_o = run(False)
    assert all(np.isfinite(losses_p)) and losses_p == losses_o, (losses_p, losses_o)
    for k in sd_p:
        assert torch.equal(sd_p[k], sd_o[k]), k
    assert not torch.equal(sd_p['embeddings'].cpu(), sd['embeddings'])                # (the steps did update)


# ------------------------------------------------------- 4. a molecule split across the faces is the isolated molecule
_SPLIT = {}


def _split_batch():
    """The 16 molecules of synth.qm9_batch(0, 0, 16), each translated (fp32) and wrapped into its cell: 16 A cubes for even
    graphs, triclinic cells with all heights >= 16 for odd ones.  Returns (periodic batch with fp32 wrapped positions, oracle
    batch with the unwrapped coordinates rebuilt in fp64 from the wrapped fp32 ones plus integer lattice vectors, edge_index
    of the oracle = radius(pos, pos, cutoff_l) without self loops)."""
    if _SPLIT:
        return _SPLIT['v']
    from oracle import pamnet_oracle as O
    from pamnet_amd import synth
    b = synth.qm9_batch(0, 0, 16)
    cube = torch.eye(3, dtype=torch.float64) * 16.0
    tri = torch.tensor([[17.0, 0.0, 0.0], [3.0, 17.0, 0.0], [-2.5, 2.0, 17.0]], dtype=torch.float64)
    assert min(_heights(tri)) >= 16.0
    cell64 = torch.stack([cube if g % 2 == 0 else tri for g in range(16)])
    gen = torch.Generator().manual_seed(4)
    wrapped, unwrapped = [], []
    for g, (s, e) in enumerate(_slices(b.batch)):
        p = b.pos[s:e].double()
        span = (p[:, None] - p[None]).pow(2).sum(-1).sqrt().max()
        assert float(span) <= 8.38 + 1e-2
        t = (torch.rand(3, generator=gen, dtype=torch.float64) @ cell64[g]).float()
        moved = (b.pos[s:e] + t).double()                                            # fp32 translation
        m = torch.floor(moved @ torch.linalg.inv(cell64[g]))
        w32 = (moved - m @ cell64[g]).float()                                        # wrapped into the cell, fp32: the input
        wrapped.append(w32)
        unwrapped.append(w32.double() + m @ cell64[g])                               # exact rebuild: w32 + integer lattice vectors
    pos_w, pos_u = torch.cat(wrapped), torch.cat(unwrapped)
    cell = cell64.float()
    assert torch.equal(cell.double(), cell64)
    # at least 8 molecules have a pair whose raw and minimum-image displacements differ; none sees an image of itself
    split = 0
    for s, v, n, d in _brute(pos_w, b.batch, cell):
        split += int(bool((n.abs().sum(-1) > 0).any()))
        pu = pos_u[s:s + v.size(0)]
        true_d = (pu[:, None] - pu[None]).pow(2).sum(-1).sqrt()
        near = true_d <= 5.0 + 1e-3
        assert float((d[near] - true_d[near]).abs().max()) < 1e-9                   # within the cutoffs: the molecule's own pair
        assert bool((d[~near] > 5.0 + 1e-3).all())                                   # beyond: no image comes closer
        off = true_d[~torch.eye(v.size(0), dtype=torch.bool)]
        assert float((off - 1.7).abs().min()) > 1e-4 and float((off - 5.0).abs().min()) > 1e-4
    assert split >= 8, split
    periodic = synth.Batch(x=b.x, batch=b.batch, pos=pos_w, cell=cell, y=b.y, num_graphs=16)
    ei = O.radius_graph(pos_u, b.batch, 1.7)
    ei = ei[:, ei[0] != ei[1]]
    ob = synth.Batch(x=b.x, batch=b.batch, pos=pos_u, edge_index=ei, y=b.y, num_graphs=16)
    _SPLIT['v'] = (periodic, ob, split)
    return _SPLIT['v']


@pytest.mark.gpu
@pytest.mark.parametrize('small,dim', [(False, 128), (False, 64), (True, 128)])
def test_split_molecules_match_the_oracle_on_unwrapped_coordinates(dev, small, dim):
    """Output, forces and every parameter gradient against the oracle fed the unwrapped molecules, by the protocol of
    tests/test_hip_forces.py: err(hip, oracle_fp64) <= max(1e-5, 2 * err(oracle_fp32, oracle_fp64))."""
    import models
    from oracle import pamnet_oracle as O
    from pamnet_amd import train
    from test_hip_forces import CANCEL_TOL, GRAD_TOL, TOL, _check_gradients, _ok
    assert (TOL, GRAD_TOL, CANCEL_TOL) == (1e-5, 1e-5, 1e-4)
    periodic, ob, split = _split_batch()
    print('molecules split across a face:', split)
    cfg = models.Config(dataset='QM9', dim=dim, n_layer=2, cutoff_l=1.7, cutoff_g=5.0)
    fwd = O.pamnet_s_forward if small else O.pamnet_forward
    sd = O.init_state_dict(cfg, seed=7, small=small)
    model = (models.PAMNet_s if small else models.PAMNet)(cfg)
    model.load_state_dict(sd, strict=True)
    model = model.to(dev)

    def oracle(dtype, forces):
        p = O.as_params({k: v.detach().to(dtype) for k, v in sd.items()})
        pos = ob.pos.to(dtype).clone().requires_grad_(forces)
        out = fwd(p, cfg, ob.x, ob.batch, pos, ob.edge_index, dtype=dtype)
        if forces:
            out.sum().backward()
            return out.detach(), pos.grad
        torch.nn.functional.l1_loss(out, ob.y.to(dtype)).backward()
        return out.detach(), p

    data = periodic.to(dev)
    data.pos.requires_grad_(True)
    out = model(data)
    out.sum().backward()
    F = data.pos.grad
    assert torch.isfinite(F).all()
    assert model._graph_cache.loc.m == ob.edge_index.size(1)
    ref32, F32 = oracle(torch.float32, True)
    ref64, F64 = oracle(torch.float64, True)
    ok, info = _ok(out.detach().cpu().numpy(), ref32.numpy(), ref64.numpy())
    print('out err / floor', info)
    assert ok, ('out', info)
    ok, info = _ok(F.cpu().numpy(), F32.numpy(), F64.numpy())
    print('force err / floor', info)
    assert ok, ('forces', info)
    model.zero_grad(set_to_none=True)
    tr = train.Trainer(model, lr=1e-4)
    assert model._one_node()
    tr.forward_backward(periodic.to(dev))
    _, p32 = oracle(torch.float32, False)
    _, p64 = oracle(torch.float64, False)
    worst = _check_gradients(model, p64, fwd, sd, cfg, ob, p32=p32)
    print('parameter gradient worst', worst)
    tr.close()


# ------------------------------------------------------------- 5. real cross-boundary interaction: a supercell is twice
GRID = 2.0 ** -12
_SUPER = {}


def _supercell_batches():
    """A: 48 atoms (pairwise minimum-image separation >= 0.9 A, types 0..4) in a 10.5 A cube and 48 in a triclinic cell, two
    graphs.  B: the 2 x 1 x 1 supercell of each as one graph (the atoms, then their copies at + a_0).  A': A with every atom
    moved by one vector, not wrapped.  Coordinates, lattice vectors and the translation are multiples of 2^-12 below 64, so
    the copies' and the translated positions are exact in fp32: the fp64 differences the image rule starts from are the same
    numbers in A, A' and B, and what is compared is the code, not the rounding of the inputs."""
    if _SUPER:
        return _SUPER['v']
    from pamnet_amd import synth
    gen = torch.Generator().manual_seed(6)
    cells = [torch.tensor(CUBE, dtype=torch.float64), torch.tensor(TRI_A, dtype=torch.float64)]
    assert min(_heights(TRI_A)) >= 10.4
    pos = [_scatter(gen, 48, c, 0.9, grid=GRID) for c in cells]
    x = [torch.randint(0, 5, (48,), generator=gen).float() for _ in cells]
    assert all(sorted(set(t.long().tolist())) == [0, 1, 2, 3, 4] for t in x)
    shift = torch.tensor([13.2578125, -7.60546875, 21.3125], dtype=torch.float64)
    for t in pos + cells + [shift]:
        assert torch.equal(torch.round(t / GRID) * GRID, t) and float(t.abs().max()) < 64.0
    batch_a = torch.arange(2).repeat_interleave(48)
    a = synth.Batch(x=torch.cat(x), batch=batch_a, pos=torch.cat(pos).float(), cell=torch.stack(cells).float(), num_graphs=2)
    a_moved = synth.Batch(x=a.x, batch=a.batch, pos=(torch.cat(pos) + shift).float(), cell=a.cell, num_graphs=2)
    assert torch.equal(a.pos.double(), torch.cat(pos)) and torch.equal(a_moved.pos.double(), torch.cat(pos) + shift)
    pos_b = torch.cat([torch.cat([p, p + c[0]]) for p, c in zip(pos, cells)])
    cell_b = torch.stack([torch.stack([2 * c[0], c[1], c[2]]) for c in cells])
    b = synth.Batch(x=torch.cat([torch.cat([t, t]) for t in x]), batch=torch.arange(2).repeat_interleave(96),
                    pos=pos_b.float(), cell=cell_b.float(), num_graphs=2)
    assert torch.equal(b.pos.double(), pos_b) and torch.equal(b.cell.double(), cell_b)
    for bt in (a, b):
        br = _brute(bt.pos, bt.batch, bt.cell)
        _assert_margin(br, 2.0), _assert_margin(br, 5.0)
        for s, v, n, d in br:
            assert float(d[~torch.eye(d.size(0), dtype=torch.bool)].min()) >= 0.9 - 1e-9
    _SUPER['v'] = (a, a_moved, b)
    return _SUPER['v']


@pytest.mark.gpu
@pytest.mark.parametrize('dim,n_layer', [(128, 2), (16, 1)])
def test_a_supercell_has_twice_the_energy_and_the_same_forces(dev, dim, n_layer):
    """E_B = 2 E_A and the forces of both copies equal A's; translating every atom of A by one vector without wrapping
    changes nothing.  Max-normalised at 1e-5, the project's parity bound: both sides are this code in fp32, with different
    summation orders (and A / B take different launch shapes of the search: 48 against 96 atoms per graph)."""
    import models
    torch.manual_seed(1)
    a, a_moved, b = _supercell_batches()
    cfg = models.Config(dataset='QM9', dim=dim, n_layer=n_layer, cutoff_l=2.0, cutoff_g=5.0)
    model = models.PAMNet(cfg).to(dev)

    def run(bt):
        data = bt.to(dev)
        data.pos.requires_grad_(True)
        out = model(data)
        g = model._graph_cache
        out.sum().backward()
        return out.detach().cpu().double(), data.pos.grad.cpu().double(), g

    e_a, f_a, g_a = run(a)
    # global edges, local edges and triplets all cross faces
    _, _, _, (n_g, n_l) = _geometry64(g_a, a.pos.double(), a.batch, a.cell)
    cross_l = n_l.abs().sum(-1) > 0
    e, q, kind = g_a.tp.row_of.long().cpu(), g_a.tp.col.long().cpu(), g_a.tp_kind.cpu()
    cross_t = (kind == 0) & (cross_l[e] | cross_l[q])
    print('crossing: global', int((n_g.abs().sum(-1) > 0).sum()), 'of', g_a.glob.m, 'local', int(cross_l.sum()), 'of', g_a.loc.m,
          'triplets', int(cross_t.sum()), 'of', int((kind == 0).sum()))
    assert int((n_g.abs().sum(-1) > 0).sum()) > 0 and int(cross_l.sum()) > 0 and int(cross_t.sum()) > 0
    e_b, f_b, g_b = run(b)
    assert g_b.glob.m == 2 * g_a.glob.m and g_b.loc.m == 2 * g_a.loc.m and g_b.tp.m == 2 * g_a.tp.m
    assert torch.isfinite(e_a).all() and float(e_a.abs().max()) > 0 and float(f_a.abs().max()) > 0
    err_e = maxnorm_err(e_b.numpy(), (2 * e_a).numpy())
    f_b = f_b.view(2, 2, 48, 3)                               # [graph, copy, atom, xyz]
    f_ref = f_a.view(2, 1, 48, 3).expand(2, 2, 48, 3)
    err_f = maxnorm_err(f_b.numpy(), f_ref.numpy())
    e_m, f_m, _ = run(a_moved)
    err_te, err_tf = maxnorm_err(e_m.numpy(), e_a.numpy()), maxnorm_err(f_m.numpy(), f_a.numpy())
    print('supercell: energy err', err_e, 'force err', err_f, '; translation: energy err', err_te, 'force err', err_tf)
    assert err_e <= 1e-5 and err_f <= 1e-5, (err_e, err_f)
    assert err_te <= 1e-5 and err_tf <= 1e-5, (err_te, err_tf)


# -------------------------------------------------------------------------------------------- 6. interface and errors
@pytest.mark.gpu
def test_refusals_say_what_to_do_instead(dev):
    import models
    from pamnet_amd import synth
    cfg = models.Config(dataset='QM9', dim=16, n_layer=1, cutoff_l=1.7, cutoff_g=5.0)
    torch.manual_seed(0)
    model = models.PAMNet(cfg).to(dev)
    b = synth.qm9_batch(0, 0, 4)
    free = synth.Batch(**{k: v for k, v in b.__dict__.items() if k != 'edge_index'})
    cell = (torch.eye(3) * 40.0).expand(4, 3, 3).contiguous()
    with torch.no_grad():
        assert torch.isfinite(model(_with_cell(free, cell).to(dev))).all()
        with pytest.raises(ValueError, match='bond-free'):
            model(_with_cell(b, cell).to(dev))                                       # cell together with edge_index
        for bad in (cell[:3], cell.view(4, 9), cell.double(), cell.to(torch.int32)):
            with pytest.raises(ValueError, match=r'\[num_graphs, 3, 3\]'):
                model(_with_cell(free, bad).to(dev))
        data = free.to(dev)
        data.cell = cell                                                             # left on the CPU
        with pytest.raises(ValueError, match='device'):
            model(data)
        sized = _with_cell(free, cell).to(dev)
        sized.sizes = (10, 10, 10)
        with pytest.raises(ValueError, match='sizes'):
            model(sized)
        tiny = cell.clone()
        tiny[2] = torch.eye(3) * 9.9                                                 # heights 9.9 <= 2 * 5.0
        with pytest.raises(ValueError, match='heights'):
            model(_with_cell(free, tiny).to(dev))
        flat = cell.clone()
        flat[1, 2] = flat[1, 0]
        with pytest.raises(ValueError, match='singular'):
            model(_with_cell(free, flat).to(dev))
        with pytest.raises(ValueError, match='heights'):
            model.prepare(_with_cell(free, tiny).to(dev), need_grad=False)
    for ds, mk in (('PDBbind', lambda: synth.pdbbind_batch(9, 0, 2, n_pocket=40, n_ligand=8)),
                   ('rna_native', lambda: synth.rna_batch(2, 0, 2))):
        other = models.PAMNet(models.Config(dataset=ds, dim=16, n_layer=1, cutoff_l=2.0, cutoff_g=6.0)).to(dev)
        ob = mk()
        ob.cell = (torch.eye(3) * 80.0).expand(2, 3, 3).contiguous()
        with torch.no_grad():
            with pytest.raises(ValueError, match='QM9 schema'):
                other(ob.to(dev))
    grad_cell = _with_cell(free, cell).to(dev)
    grad_cell.cell.requires_grad_(True)
    with pytest.raises(NotImplementedError, match='stress'):
        model(grad_cell)
    with torch.no_grad():
        assert torch.isfinite(model(grad_cell)).all()                                # (no grad mode: nothing to refuse)


@pytest.mark.gpu
def test_a_batch_without_cell_calls_none_of_the_new_entry_points(dev, monkeypatch):
    import models
    from pamnet_amd import synth
    torch.manual_seed(0)
    b = synth.qm9_batch(0, 0, 4)
    free = synth.Batch(**{k: v for k, v in b.__dict__.items() if k != 'edge_index'})
    calls = _record(monkeypatch)
    for dim in (128, 16):
        model = models.PAMNet(models.Config(dataset='QM9', dim=dim, n_layer=1, cutoff_l=1.7, cutoff_g=5.0)).to(dev)
        for bt in (b, free):
            data = bt.to(dev)
            data.pos.requires_grad_(True)
            model(data).sum().backward()
            model(bt.to(dev)).sum().backward()
    assert 'pamnet_pos_bwd_f32' in calls and not [c for c in calls if c in NEW], calls


@pytest.mark.gpu
def test_new_entry_points_validate_their_arguments(dev):
    """EINVAL / ENULL with nothing launched (pamnet_pos_bwd_pbc_f32 answers EINVAL for a null pointer, as its twin does)."""
    from pamnet_amd import lib
    P = lib.ptr
    i32 = lambda n, v=7: torch.full((n,), v, dtype=torch.int32, device=dev)
    pos = torch.zeros((4, 3), device=dev)
    cell = torch.eye(3, device=dev).view(1, 9).contiguous() * 20
    tab = torch.full((1, 18), 7.0, dtype=torch.float64, device=dev)
    flag, ng, gptr, count, ptr, nbr = i32(1, 0), i32(4, 0), torch.tensor([0, 4], dtype=torch.int32, device=dev), i32(4), i32(5, 0), i32(8)
    dist = torch.full((8,), 7.0, device=dev)
    st = lib.stream_of(pos)

    def prepare(c=cell, n=1, r=5.0, t=tab, f=flag):
        lib.call('pamnet_cell_prepare_f64', P(c), n, r, P(t), P(f), st)

    def count_(p=pos, t=tab, g=ng, gp=gptr, n=4, n_g=1, mx=0, c=count):
        lib.call('pamnet_radius_pbc_count_i32', P(p), P(t), P(g), P(gp), n, n_g, 5.0, mx, P(c), P(flag), st)

    def fill(p=pos, t=tab, g=ng, gp=gptr, n=4, n_g=1, mx=0, pt=ptr, nb=nbr, d=dist, cap=8):
        lib.call('pamnet_radius_pbc_fill_i32', P(p), P(t), P(g), P(gp), n, n_g, 5.0, mx, P(pt), P(nb), P(d), None, cap, st)

    def angles(p=pos, t=tab, g=ng, lp=ptr, s=nbr, d=nbr, ne=2, tp=ptr, o=nbr, a=dist, cap=8):
        lib.call('pamnet_triplet_fill_pbc_f32', P(p), P(t), P(g), P(lp), P(s), P(d), ne, 1, P(tp), P(o), P(o), P(a), P(o), cap, st)

    work, dpos = torch.full((24,), 7.0, dtype=torch.float64, device=dev), torch.full((4, 3), 7.0, device=dev)

    def bwd(p=pos, t=tab, g=ng, n=4, eg=2, el=2, tp=2, w=work, o=dpos):
        lib.call('pamnet_pos_bwd_pbc_f32', P(p), P(t), P(g), n, P(ptr), P(nbr), P(nbr), P(ptr), P(nbr), P(dist), eg, P(ptr), P(nbr),
                 P(nbr), P(ptr), P(nbr), P(dist), el, P(ptr), P(nbr), P(nbr), P(nbr), P(ptr), P(nbr), P(dist), tp, P(w), P(o), st)

    cases = [(prepare, [dict(n=-1), dict(r=0.0), dict(r=-1.0), dict(r=float('nan')), dict(r=float('inf'))], 'EINVAL'),
             (prepare, [dict(c=None), dict(t=None), dict(f=None)], 'ENULL'),
             (count_, [dict(n=-1), dict(n_g=-1), dict(mx=-1), dict(mx=1 << 31)], 'EINVAL'),
             (count_, [dict(p=None), dict(t=None), dict(g=None), dict(gp=None), dict(c=None)], 'ENULL'),
             (fill, [dict(n=-1), dict(n_g=-1), dict(mx=-1), dict(cap=-1)], 'EINVAL'),
             (fill, [dict(p=None), dict(t=None), dict(g=None), dict(gp=None), dict(pt=None), dict(nb=None), dict(d=None)], 'ENULL'),
             (angles, [dict(ne=-1), dict(cap=-1)], 'EINVAL'),
             (angles, [dict(p=None), dict(t=None), dict(g=None), dict(lp=None), dict(s=None), dict(tp=None), dict(o=None),
                       dict(a=None)], 'ENULL'),
             (bwd, [dict(n=-1), dict(eg=-1), dict(el=-1), dict(tp=-1), dict(p=None), dict(t=None), dict(g=None), dict(w=None),
                    dict(o=None)], 'EINVAL')]
    for fn, kws, what in cases:
        for kw in kws:
            with pytest.raises(RuntimeError, match=what):
                fn(**kw)
    torch.cuda.synchronize()
    for t in (tab, count, nbr, dist, work, dpos):                                    # nothing was launched
        assert bool((t == 7).all())
    assert int(flag) == 0


def test_header_declares_the_periodic_entry_points_at_abi_18():
    """(No GPU: the header and the built library.)"""
    import ctypes
    import re
    from pamnet_amd import build, lib
    decl = lib.declared_functions()
    assert all(n in decl for n in NEW)
    assert [len(decl[n]) for n in NEW] == [6, 11, 14, 15, 29]
    # the twins' argument lists with the cell table (and node_graph) behind pos
    assert len(decl['pamnet_radius_count_i32']) == 10 and len(decl['pamnet_radius_fill_i32']) == 13
    assert len(decl['pamnet_triplet_fill_f32']) == 13 and len(decl['pamnet_pos_bwd_f32']) == 27
    assert int(re.search(r'#define\s+PAMNET_ABI_VERSION\s+(\d+)', open(lib.HEADER).read()).group(1)) == 18
    h = ctypes.CDLL(build.build())
    assert h.pamnet_abi_version() == 18 and all(hasattr(h, n) for n in NEW)


def test_inputs_meet_their_preconditions():
    """(No GPU.)  The conditions the GPU tests state about their inputs, checked in fp64 on the CPU."""
    for name in ('a', 'b'):
        brute = _brute_of(name)
        for r in (2.0, 5.0):
            _assert_margin(brute, r)
        assert _brute_lists(brute, 5.0, max_nb=8)[1]
    assert _split_batch()[2] >= 8
    _supercell_batches()
