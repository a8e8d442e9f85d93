"""The narrow-width (dim 16 / 32 / 64) row kernels of csrc/narrow_core.h at row counts where a wave walks several
16-row tiles, against the fp64 restatements of tests/narrow_refs.py.

Every row kernel walks `for (t = blockIdx.x * NW + wave; t < ntiles; t += gridDim.x * NW)` over a capped grid.  Below
the cap the loop body runs once per wave (all test_hip_narrow.py reaches, its node tail apart); above it the loop hands
prefetched tiles and weight-gradient accumulators from one tile to the next, the ragged last tile is some wave's second
or third, and a wave's last pass takes the "last tile again" prefetch branch.  The row counts below are derived from the
grid constants (restated in the table, guarded by a CPU test that reads the header and by pamnet_narrow_blocks):

    cap_bwd(d) + 5            one backward wave walks a second, ragged tile; no forward wave walks
    cap_fwd(d) + 5            the same state for the forward kernels; backward waves walk 2 to 3 tiles
    2 cap_fwd(d) + 16*7 + 3   forward waves walk 2 or 3 tiles, backward waves 4 to 5; ragged tile mid-workgroup
    cap_ew(d) + 3             local_gate only: its element-wise grid starts to stride

Bounds: forward outputs, per-row gradients and dP (summed over a node's own edges) are held to the 1e-5 of
test_hip_narrow.py.  Gradients summed over all m rows (weights, biases, frequencies) are held to max(1e-5, 4 * err32),
err32 being the error of plain fp32 torch autograd of the same formula on the same inputs against the same fp64
reference: both are fp32 sums of the same m products in different orders.  Measured figures: profiles/narrow_walk_errors.txt
(each check prints its line; run with -s to collect them)."""
import os
import re
import types

import numpy as np
import pytest
import torch

import narrow_refs as R
from test_hip_narrow import dev                             # noqa: F401  (the module-scoped fixture of the narrow tests)

TOL = 1e-5
WIDTHS = (16, 32, 64)

# ---- the grid constants of csrc/narrow_core.h, restated ---------------------------------------------------------------
BWD_WAVES = {16: 16, 32: 8, 64: 4}        # bwd_waves(d): waves per backward workgroup
FWD_PER_CU = {16: 8, 32: 4, 64: 2}        # fwd_per_cu(d): forward workgroups (of FWD_WAVES waves) per grid block slot
BLOCKS = 256                              # NARROW_BLOCKS
FWD_WAVES = 4                             # grid_for's default `waves` (NWG = 256 threads)
EW_BLOCKS = 4096                          # ew_grid: 256 threads, one float4 each, grid-stride beyond this many workgroups


def cap_bwd(d):
    return 16 * BLOCKS * BWD_WAVES[d]


def cap_fwd(d):
    return 16 * BLOCKS * FWD_PER_CU[d] * FWD_WAVES


def cap_ew(d):
    return 4 * EW_BLOCKS * 256 // d


def row_counts(d):
    return [cap_bwd(d) + 5, cap_fwd(d) + 5, 2 * cap_fwd(d) + 16 * 7 + 3]


def gate_row_counts(d):
    return [cap_ew(d) + 3, cap_bwd(d) + 5]


ROWS = [(d, m) for d in WIDTHS for m in row_counts(d)]
GATE_ROWS = [(d, m) for d in WIDTHS for m in gate_row_counts(d)]


def _largest(d, m, counts=row_counts):
    return m == max(counts(d))


# ---- CPU guards: the table against the header, the row counts against the states they are meant to reach -------------
def _c_ternary(expr, d):
    """Value at d of `d == A ? X : (d == B ? Y : Z)`."""
    expr = expr.strip()
    while expr.startswith('(') and expr.endswith(')'):
        expr = expr[1:-1].strip()
    mt = re.fullmatch(r'd == (\d+) \? (\d+) : (.+)', expr)
    if mt:
        return int(mt.group(2)) if d == int(mt.group(1)) else _c_ternary(mt.group(3), d)
    assert expr.isdigit(), 'narrow_core.h: %r is not the chain of `d == A ? X : Y` this test reads' % expr
    return int(expr)


def header_constants(text):
    """The grid constants as csrc/narrow_core.h states them; raises if a definition no longer has the form read here."""
    def one(pattern):
        found = re.findall(pattern, text)
        assert len(found) == 1, 'narrow_core.h: expected exactly one match of %r, found %d' % (pattern, len(found))
        return found[0]
    blocks = int(one(r'constexpr int NARROW_BLOCKS = (\d+);'))
    bwd = one(r'constexpr int bwd_waves\(int d\) \{ return ([^;]+); \}')
    fwd = one(r'constexpr int fwd_per_cu\(int64_t d\) \{ return ([^;]+); \}')
    one(r'constexpr int lin_bwd_waves\(int d\) \{ return bwd_waves\(d\); \}')
    fwd_waves = int(one(r'constexpr int grid_for\(int64_t m, int per_cu, int waves = (\d+)\)'))
    one(r'const int64_t tiles = \(m \+ 15\) / 16;')
    one(r'const int64_t cap = NARROW_BLOCKS \* \(int64_t\)per_cu;')
    one(r'constexpr int fwd_row_grid\(int64_t m, int64_t d\) \{ return grid_for\(m, fwd_per_cu\(d\)\); \}')
    one(r'constexpr int bwd_row_grid\(int64_t m, int64_t d\) \{ return grid_for\(m, 1, bwd_waves\(\(int\)d\)\); \}')
    nwg = int(one(r'constexpr int NWG = (\d+);'))
    ew = re.search(r'constexpr int ew_grid\(int64_t total\) \{\s*const int64_t want = \(total \+ 255\) / 256;\s*'
                   r'return \(int\)\(want < 1 \? 1 : \(want > (\d+) \? (\d+) : want\)\);', text)
    assert ew, 'narrow_core.h: ew_grid no longer has the form this test reads'
    assert ew.group(1) == ew.group(2)
    return dict(blocks=blocks, bwd_waves={d: _c_ternary(bwd, d) for d in WIDTHS},
                fwd_per_cu={d: _c_ternary(fwd, d) for d in WIDTHS}, fwd_waves=fwd_waves, nwg=nwg, ew_blocks=int(ew.group(1)))


def check_table(text):
    got = header_constants(text)
    want = dict(blocks=BLOCKS, bwd_waves=BWD_WAVES, fwd_per_cu=FWD_PER_CU, fwd_waves=FWD_WAVES, nwg=64 * FWD_WAVES,
                ew_blocks=EW_BLOCKS)
    assert got == want, ('the grids of csrc/narrow_core.h were retuned: restate them in the table of this file, so that its '
                         'row counts move with the caps', got, want)


def test_table_matches_the_header():
    here = os.path.dirname(os.path.abspath(__file__))
    path = os.path.join(here, '..', 'physics-aware-multiplex-gnn_amd', 'csrc', 'narrow_core.h')
    with open(path) as f:
        check_table(f.read())


def test_row_counts():
    assert [cap_bwd(d) for d in WIDTHS] == [65536, 32768, 16384]
    assert [cap_fwd(d) for d in WIDTHS] == [131072, 65536, 32768]
    assert [cap_ew(d) for d in WIDTHS] == [262144, 131072, 65536]
    assert max(m for _, m in ROWS) == 262259
    for d in WIDTHS:
        tiles = lambda m: -(-m // 16)
        waves_b, waves_f = BLOCKS * BWD_WAVES[d], BLOCKS * FWD_PER_CU[d] * FWD_WAVES
        m0, m1, m2 = row_counts(d)
        assert tiles(m0) == waves_b + 1 and tiles(m0) <= waves_f and m0 % 16 == 5      # one backward wave, a ragged tile
        assert tiles(m1) == waves_f + 1 and m1 % 16 == 5
        assert 2 * waves_f < tiles(m2) < 3 * waves_f and m2 % 16 == 3                   # forward: 3 tiles or 2
        assert 4 * waves_b < tiles(m2) < 5 * waves_b
        assert 0 < (tiles(m2) - 1) % waves_f < waves_f - 1 and 0 < (tiles(m2) - 1) % waves_b < waves_b - 1   # ragged tile: mid-grid
        for m in gate_row_counts(d):                                                   # (no case is a duplicate)
            assert m not in row_counts(d) or m == cap_bwd(d) + 5
        assert cap_ew(d) + 3 not in row_counts(d)
        assert (cap_ew(d) + 3) * (d // 4) > EW_BLOCKS * 256 >= (cap_ew(d)) * (d // 4)


def split_rows(rng, m, n):
    """n row lengths that sum to exactly m: ragged, a fifth of the rows empty, the first and the last row at least 2 long."""
    w = rng.integers(1, 17, n) * (rng.random(n) > 0.2)
    w[0] = w[-1] = 16
    lens = rng.multinomial(m, w / w.sum())
    for end in (0, n - 1):
        short = 2 - int(lens[end])
        if short > 0:
            lens[int(np.argmax(lens))] -= short
            lens[end] += short
    assert int(lens.sum()) == m and lens.min() == 0 and lens[0] >= 2 and lens[-1] >= 2
    return lens


@pytest.mark.parametrize('m,n', [(1000, 125), (65541, 8192), (262259, 32782)])
def test_split_rows(m, n):
    lens = split_rows(np.random.default_rng(m), m, n)
    assert lens.shape == (n,) and int(lens.sum()) == m
    assert (lens == 0).any() and len(set(lens.tolist())) > 2


# ---- the comparison --------------------------------------------------------------------------------------------------
def _err(a, ref):
    """max|a - ref| / max|ref| in fp64 on the device (conftest.maxnorm_err without the host copy of [m, 4d] operands)."""
    ref = ref.detach().double()
    return float((a.detach().double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def _log(kernel, d, m, name, err, err32=None, bound=TOL):
    e32 = '        -' if err32 is None else '%9.3e' % err32
    print('WALK %-18s d=%-2d m=%-6d %-6s err32=%s err=%9.3e bound=%9.3e' % (kernel, d, m, name, e32, err, bound))


def _walk_case(kernel, d, m, tensors, per_row, summed, run, ref, twice):
    """tensors: name -> fp32 tensor; the names in per_row + summed are differentiated.  run(t) -> the kernel's outputs
    (through the autograd wrappers of pamnet_amd.narrow), ref(t) -> the same outputs by the formulas of narrow_refs in
    the dtype of t.  Forward and per-row gradients against fp64 at TOL; summed gradients at max(TOL, 4 err32)."""
    wanted = tuple(per_row) + tuple(summed)
    leaf = lambda dtype, names: {k: v.detach().to(dtype).requires_grad_(k in names) if v.is_floating_point() else v
                                 for k, v in tensors.items()}
    t = leaf(torch.float32, wanted)
    outs = run(t)
    gs = [torch.randn_like(o) for o in outs]
    torch.autograd.backward(outs, gs)
    t64 = leaf(torch.float64, wanted)
    outs64 = ref(t64)
    torch.autograd.backward(outs64, [g.double() for g in gs])
    t32 = leaf(torch.float32, summed)
    torch.autograd.backward(ref(t32), gs)
    failures = []
    for k, (o, o64) in enumerate(zip(outs, outs64)):
        assert o.shape == o64.shape
        err = _err(o, o64)
        _log(kernel, d, m, 'out%d' % k, err)
        if not err < TOL:
            failures.append(('out%d' % k, err, TOL))
    for name in per_row:
        assert t[name].grad is not None, name
        err = _err(t[name].grad, t64[name].grad)
        _log(kernel, d, m, 'd' + name, err)
        if not err < TOL:
            failures.append(('d' + name, err, TOL))
    for name in summed:
        assert t[name].grad is not None, name
        err32 = _err(t32[name].grad, t64[name].grad)
        err = _err(t[name].grad, t64[name].grad)
        bound = max(TOL, 4 * err32)
        _log(kernel, d, m, 'd' + name, err, err32, bound)
        if not err < bound:
            failures.append(('d' + name, err, bound))
    assert not failures, (kernel, d, m, failures)
    if twice:                                                # the partial-row reduction is fixed-order: bitwise repeatable
        first = {k: t[k].grad.clone() for k in wanted}
        for k in wanted:
            t[k].grad = None
        torch.autograd.backward(run(t), gs)
        for k in wanted:
            assert torch.equal(first[k], t[k].grad), (kernel, d, m, k)
    return t


def _rand(dev, scale, *shape):
    return torch.randn(*shape, device=dev) * scale


def _walk_graph(rng, m, dev):
    """Exactly m edges over n = m / 8 nodes as CSR over targets + the transposed CSR over sources: ragged degrees with
    zero-degree nodes; the first and the last (ragged) 16-row tile hold node 0 and node n - 1 as sources, and the last
    tile's targets end at node n - 1 (targets are sorted, so node 0 as a target sits in the first tile)."""
    from pamnet_amd import graph as G
    n = m // 8
    lens = split_rows(rng, m, n)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    row_of = np.repeat(np.arange(n), lens).astype(np.int32)
    col = rng.integers(0, n, m).astype(np.int32)
    col[0], col[1] = n - 1, 0
    col[m - 1], col[m - 2] = 0, n - 1
    assert m % 16 >= 2 and row_of[0] == row_of[1] == 0 and row_of[m - 1] == row_of[m - 2] == n - 1
    csr = G.CSR(torch.from_numpy(ptr).to(dev), torch.from_numpy(row_of).to(dev), torch.from_numpy(col).to(dev))
    return csr, G.Transpose(csr.col, n), n


@pytest.mark.gpu
def test_blocks_match_the_table(dev):
    from pamnet_amd import narrow
    for m in sorted({1, 4099} | {m for _, m in ROWS + GATE_ROWS}):
        assert narrow._blocks(m) == BLOCKS


@pytest.mark.gpu
@pytest.mark.parametrize('d,m', ROWS)
def test_global_message(dev, d, m):
    from pamnet_amd import narrow
    rng = np.random.default_rng(d * 7 + m)
    csr, tr, n = _walk_graph(rng, m, dev)
    assert csr.m == m
    i, j = csr.row_of.long(), csr.col.long()
    torch.manual_seed(d + m)
    tensors = dict(x1=_rand(dev, 0.5, n, d), P=_rand(dev, 0.5, n, 2 * d), e=_rand(dev, 0.5, m, d),
                   wm=_rand(dev, 0.5, d, 3 * d), bm=_rand(dev, 0.5, d), wea=_rand(dev, 0.5, d, d))
    order = ('x1', 'P', 'e', 'wm', 'bm', 'wea')
    t = _walk_case('global_message', d, m, tensors, ('x1', 'P', 'e'), ('wm', 'bm', 'wea'),
                   lambda t: (narrow.global_message(*[t[k] for k in order], csr, tr),),
                   lambda t: (R.global_message(*[t[k] for k in order], i, j),), _largest(d, m))
    assert torch.equal(t['wm'].grad[:, :2 * d], torch.zeros_like(t['wm'].grad[:, :2 * d]))   # node blocks: P's producer


@pytest.mark.gpu
@pytest.mark.parametrize('d,m', ROWS)
@pytest.mark.parametrize('res_x,with_r', [(False, False), (True, False), (True, True)])
def test_mlp2(dev, d, m, res_x, with_r):
    from pamnet_amd import narrow
    torch.manual_seed(d * 3 + m)
    tensors = dict(x=_rand(dev, 0.4, m, d), w1=_rand(dev, 0.4, d, d), b1=_rand(dev, 0.4, d), w2=_rand(dev, 0.4, d, d),
                   b2=_rand(dev, 0.4, d))
    if with_r:
        tensors['r'] = _rand(dev, 0.4, m, d)
    w = ('w1', 'b1', 'w2', 'b2')
    _walk_case('mlp2 res_x=%d r=%d' % (res_x, with_r), d, m, tensors, ('x', 'r') if with_r else ('x',), w,
               lambda t: (narrow._Mlp2.apply(t['x'], *[t[k] for k in w], res_x, t.get('r')),),
               lambda t: (R.mlp2(t['x'], *[t[k] for k in w], res_x, t.get('r')),), _largest(d, m))


@pytest.mark.gpu
@pytest.mark.parametrize('d,m', ROWS)
@pytest.mark.parametrize('act', [True, False])
def test_linear(dev, d, m, act):
    from pamnet_amd import narrow
    torch.manual_seed(d + m + act)
    tensors = dict(x=_rand(dev, 0.4, m, d), w=_rand(dev, 0.4, d, d), b=_rand(dev, 0.4, d))
    _walk_case('linear act=%d' % act, d, m, tensors, ('x',), ('w', 'b'),
               lambda t: (narrow.linear(t['x'], types.SimpleNamespace(weight=t['w'], bias=t['b']), act=act),),
               lambda t: (R.linear(t['x'], t['w'], t['b'], act),), _largest(d, m))


@pytest.mark.gpu
@pytest.mark.parametrize('d,m', ROWS)
def test_project(dev, d, m):
    """The four strided [d, d] blocks of two 3d-wide weights: output and its gradient at row stride 4d, dx accumulated
    over the four launches."""
    from pamnet_amd import narrow
    torch.manual_seed(d + m + 2)
    tensors = dict(x=_rand(dev, 0.4, m, d), wj=_rand(dev, 0.4, d, 3 * d), wk=_rand(dev, 0.4, d, 3 * d))
    t = _walk_case('project', d, m, tensors, ('x',), ('wj', 'wk'),
                   lambda t: (narrow.project(t['x'], ((0, 0), (1, 0), (0, d), (1, d)), t['wj'], t['wk']),),
                   lambda t: (R.project4(t['x'], t['wj'], t['wk']),), _largest(d, m))
    for k in ('wj', 'wk'):
        assert torch.equal(t[k].grad[:, 2 * d:], torch.zeros_like(t[k].grad[:, 2 * d:]))      # the edge block is not projected


def _kinds(rng, d, m):
    """Random weight-set choices, except two runs of 64 consecutive rows: all 0 in the first pass of tiles, all 1 beyond
    cap_bwd(d) (at m = cap_bwd(d) + 5 the run ends with the five rows beyond it).  A kind fetched for another tile of
    the walk changes the result."""
    kind = rng.integers(0, 2, m).astype(np.int32)
    a = 16 * 3 + 5
    b = min(cap_bwd(d) + 16 * 2 + 7, m - 64)
    assert a + 64 < cap_bwd(d) and b + 64 > cap_bwd(d)
    kind[a:a + 64] = 0
    kind[b:b + 64] = 1
    return kind


@pytest.mark.gpu
@pytest.mark.parametrize('d,m', ROWS)
@pytest.mark.parametrize('k,two', [(16, False), (42, False), (42, True)])
def test_embed(dev, d, m, k, two):
    from pamnet_amd import narrow
    torch.manual_seed(d + k + m)
    rng = np.random.default_rng(m + k)
    tensors = dict(f=_rand(dev, 1.0, m, k), wa=_rand(dev, 0.3, d, k), ba=_rand(dev, 0.3, d))
    summed = ('wa', 'ba')
    if two:
        tensors.update(wb=_rand(dev, 0.3, d, k), bb=_rand(dev, 0.3, d))
        summed += ('wb', 'bb')
    kind = torch.from_numpy(_kinds(rng, d, m)).to(dev) if two else None
    _walk_case('embed k=%d sets=%d' % (k, 1 + two), d, m, tensors, ('f',) if k == 16 else (), summed,
               lambda t: (narrow._Embed.apply(t['f'], kind, t['wa'], t['ba'], t.get('wb'), t.get('bb')),),
               lambda t: (R.embed(t['f'], kind, t['wa'], t['ba'], t.get('wb'), t.get('bb')),), _largest(d, m))


@pytest.mark.gpu
@pytest.mark.parametrize('d,m', ROWS)
def test_embed_rbf(dev, d, m):
    """The Bessel rows formed in the kernels: the forward returns the floats of the two-step form; the gradients of the
    frequencies, W and b against fp64.  Distances on both sides of the cutoff."""
    from pamnet_amd import narrow, ops
    torch.manual_seed(d + m + 5)
    dist = torch.rand(m, device=dev) * 5.6 + 0.3
    freq = (torch.arange(1, 17, dtype=torch.float32, device=dev) * np.pi) + torch.randn(16, device=dev) * 0.01
    tensors = dict(dist=dist, freq=freq, w=_rand(dev, 0.25, d, 16), b=_rand(dev, 0.25, d))
    assert int((dist > 5.0).sum()) > 64 and int((dist < 5.0).sum()) > 64
    _walk_case('embed_rbf', d, m, tensors, (), ('freq', 'w', 'b'),
               lambda t: (narrow._EmbedRbf.apply(t['dist'], t['freq'], 5.0, t['w'], t['b']),),
               lambda t: (R.embed_rbf(t['dist'], t['freq'], t['w'], t['b'], 5.0),), _largest(d, m))
    with torch.no_grad():
        y1 = narrow._EmbedRbf.apply(dist, freq, 5.0, tensors['w'], tensors['b'])
        y2 = narrow._Embed.apply(ops.rbf(dist, freq, 5.0), None, tensors['w'], tensors['b'], None, None)
    assert torch.equal(y1, y2)


@pytest.mark.gpu
@pytest.mark.parametrize('d,m', GATE_ROWS)
def test_local_gate(dev, d, m):
    from pamnet_amd import narrow
    rng = np.random.default_rng(d + m)
    csr, tr, n = _walk_graph(rng, m, dev)
    i, j = csr.row_of.long(), csr.col.long()
    torch.manual_seed(d * 5 + m)
    tensors = dict(P=_rand(dev, 0.6, n, 4 * d), Q=_rand(dev, 0.6, m, 4 * d), b1=_rand(dev, 0.6, d), b2=_rand(dev, 0.6, d))
    order = ('P', 'Q', 'b1', 'b2')
    t = _walk_case('local_gate', d, m, tensors, ('P', 'Q'), ('b1', 'b2'),
                   lambda t: narrow.local_gate(*[t[k] for k in order], csr, tr),
                   lambda t: R.local_gate(*[t[k] for k in order], i, j), _largest(d, m, gate_row_counts))
    assert torch.equal(t['Q'].grad[:, 3 * d:], torch.zeros_like(t['Q'].grad[:, 3 * d:]))        # lin_rbf_out: not the gate's
