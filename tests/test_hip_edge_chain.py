"""Kernel-level tests of the edge-chain kernels (csrc/edge_chain.hip, csrc/edge_core.h) through the C ABI: the triplet / pair MLP
(pamnet_mlp2_fwd_f32, _fwd_multi_f32, _bwd_f32), the global edge stage (pamnet_global_edge_fwd_f32 / _bwd_f32), the local edge
stage (pamnet_local_edge_fwd_f32 / _bwd_f32) and the paired backward launch (pamnet_local_bwd_pair_f32), at the row counts where
the host-side launch plan changes regime: one or two workgroups, an uneven deal of the 16-row tiles, every template instance,
two and three chunks per workgroup, a short last chunk, both clamps of the paired launch's CU split.

Reference everywhere: fp64 torch on the same fp32 inputs, the formulas of include/pamnet_hip.h ("Fused edge-level kernels");
the local edge backward is differentiated by torch autograd in fp64.  Tolerance: the rule of test_hip_fused.py::_ok, per output
tensor, err = max|a - b| / max|b|:   err(hip, fp64) <= max(2e-6, 2 x err(torch fp32 on the same inputs, fp64)).

Operands are NaN-guarded: weight slices are column blocks of wider NaN tensors (ld 384 for W_e and W_ji[:, 2d:] / W_kj[:, 2d:],
128 otherwise) between NaN rows, every row operand has a NaN row behind its last row, every output starts as NaN between NaN
guard rows that must stay NaN.  Every form runs twice (same bits), forwards also without their optional saves (same bits in the
required outputs), backwards with accumulate 0 and 1.  The forms the engine runs -- mlp2_fwd_multi, local_edge_fwd /
local_edge_bwd / local_bwd_pair on pamnet_pack_weights_mixed_f32 images -- are compared with fp64 directly.

plan8 / plan4 below MIRROR the host-side plan of csrc/edge_chain.hip (the header does not expose it) and must follow it: every
parametrised row count is first checked against the regime its table entry names (grid, uneven deal, tiles per chunk, template
instance, the chunk walk of each kind of workgroup), so that a changed plan makes the table fail as stale instead of quietly
testing something else.

The library reads PAMNET_EDGE_WAVES once per process: test_four_wave_geometry re-runs this file in one child process with the
paired 4-wave geometry forced; the tables below are picked by that variable.

Worst measured (err, floor = torch fp32's error) per entry point on an MI355X over all cases, the saturated ones included
(8-wave geometry | forced 4-wave geometry); the 2e-6 floor of the rule decided every case, 2 x torch's error never exceeded it:
    mlp2_fwd         (7.1e-7, 5.2e-7) | (5.6e-7, 5.1e-7)        mlp2_fwd_multi   (5.2e-7, 5.3e-7) | (5.2e-7, 5.3e-7)
    mlp2_bwd         (6.8e-7, 6.8e-7) | (7.2e-7, 7.9e-7)        global_edge_fwd  (7.7e-7, 7.7e-7) | (5.1e-7, 5.1e-7)
    global_edge_bwd  (7.7e-7, 4.1e-7) | (6.9e-7, 4.2e-7)        local_edge_fwd   (4.7e-7, 5.4e-7) | (5.8e-7, 5.8e-7)
    local_edge_bwd   (6.8e-7, 4.5e-7) | (6.8e-7, 4.5e-7)        local_bwd_pair   (1.0e-6, 4.5e-7) | (1.0e-6, 4.5e-7)
(equal pairs: both evaluations are off by the final rounding to fp32 of the same element.)  A build whose CHUNK_LOOP skips one
tile between chunks fails exactly the 23 cases in which a workgroup walks more than one chunk and passes the other 42; one whose
8-wave deal forgets the `pb` offset of the later workgroups fails exactly the 44 cases with an uneven deal.
"""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
D = 128
NAN = float('nan')
N_CU = 256                              # edge_core.h
PAIR_EDGE_COST = 3.1                    # edge_chain.hip: a local edge row in triplet / pair MLP rows, for the pair's CU split
IMG = 3 * D * D // 2                    # floats of a kind-1 (bf16x3 fragment) weight image
WAVES4 = os.environ.get('PAMNET_EDGE_WAVES') == '4'
WORST = {}                              # entry point -> (err, floor, tag) of the case nearest to its bound


# ------------------------------------------------------------------------------------------ 1. the plan, restated
def _cd(a, b):
    return -(-a // b)


def plan8(rows, cap, target=N_CU):
    """edge_chain.hip plan8: one wave of 8-wave workgroups; workgroup b owns pa (+1 for b < pb) consecutive 16-row tiles and walks
    them in chunks of cmt <= cap."""
    tiles = _cd(rows, 16)
    per = _cd(tiles, target)
    grid = _cd(tiles, per)
    return dict(grid=grid, pa=tiles // grid, pb=tiles % grid, pc=0, cmt=_cd(per, _cd(per, cap)), per=per, paired=False)


def plan4(rows, cap, target=N_CU):
    """edge_chain.hip plan4: pairs of 4-wave workgroups; pair c owns pa tiles, workgroup c the first pc, workgroup pb + c the rest."""
    tiles = _cd(rows, 16)
    per = _cd(tiles, target)
    pairs = _cd(tiles, per)
    hi = (per + 1) // 2
    return dict(grid=2 * pairs if per > hi else pairs, pa=per, pb=pairs, pc=hi, cmt=_cd(hi, _cd(hi, cap)), per=per, paired=True)


def _walks(p):
    """Tiles per chunk as each kind of workgroup of the plan walks them: (the larger share, the smaller share)."""
    if p['paired']:
        shares = [p['pc'], p['pa'] - p['pc']]
    else:
        shares = [p['pa'] + 1] * (p['pb'] != 0) + [p['pa']]
    return tuple(tuple(min(p['cmt'], s - k) for k in range(0, s, p['cmt'])) for s in shares)


CAPS = {'mlp2': (7, 3, N_CU), 'global': (8, 3, N_CU), 'lfwd': (5, 2, N_CU // 2)}     # (8-wave cap, 4-wave cap, target)


def _plan(kind, rows):
    if kind == 'lbwd':                                      # the local edge backward: always 8 waves, <= 3 tiles per chunk
        return plan8(rows, 3)
    cap8, cap4, target = CAPS[kind]
    return plan4(rows, cap4, target) if WAVES4 else plan8(rows, cap8, target)


def _instance(kind, p):
    """The template instance <MTX, NW> the launch macros of edge_chain.hip pick for the plan."""
    c = p['cmt']
    if p['paired']:
        return (2 if c <= 2 or kind == 'lfwd' else 3, 4)
    if kind == 'lbwd' or c <= 3:
        return (3, 8)
    if c <= 5 or kind == 'lfwd':
        return (5, 8)
    return (7 if kind == 'mlp2' else 8, 8)


ONE = ((1,),)
# rows -> (grid, tiles per chunk, MTX of the template instance, chunk walks)
TABLE8 = {
    'mlp2': {1: (1, 1, 3, ONE), 15: (1, 1, 3, ONE), 16: (1, 1, 3, ONE), 17: (2, 1, 3, ONE),
             4097: (129, 2, 3, ((2,), (1,))), 4111: (129, 2, 3, ((2,), (1,))),
             12289: (193, 4, 5, ((4,), (3,))), 20481: (214, 6, 7, ((6,), (5,))),
             28673: (225, 4, 5, ((4, 4), (4, 3))), 61441: (241, 6, 7, ((6, 6, 4), (6, 6, 3)))},
    'global': {1: (1, 1, 3, ONE), 17: (2, 1, 3, ONE), 4097: (129, 2, 3, ((2,), (1,))), 12289: (193, 4, 5, ((4,), (3,))),
               28673: (225, 8, 8, ((8,), (7,))), 32769: (228, 5, 5, ((5, 4), (5, 3)))},
    'lbwd': {1: (1, 1, 3, ONE), 17: (2, 1, 3, ONE), 4097: (129, 2, 3, ((2,), (1,))), 12289: (193, 2, 3, ((2, 2), (2, 1))),
             28673: (225, 3, 3, ((3, 3, 2), (3, 3, 1)))},
    'lfwd': {1: (1, 1, 3, ONE), 17: (2, 1, 3, ONE), 4097: (86, 3, 3, ((3,), (2,))), 8193: (103, 5, 5, ((5,), (4,))),
             12289: (110, 4, 5, ((4, 3), (4, 2))), 20481: (117, 4, 5, ((4, 4, 3), (4, 4, 2)))},
}
PAIRED = {17: (2, 1, 2, ((1,), ())), 4097: (258, 1, 2, ((1,), (1,))), 8193: (342, 2, 2, ((2,), (1,))),
          16385: (410, 3, 3, ((3,), (2,))), 24577: (440, 2, 2, ((2, 2), (2, 1)))}
TABLE4 = {
    'mlp2': PAIRED, 'global': PAIRED, 'lbwd': TABLE8['lbwd'],
    'lfwd': {17: (2, 1, 2, ((1,), ())), 4097: (172, 2, 2, ((2,), (1,))), 8193: (206, 2, 2, ((2, 1), (2,))),
             16385: (228, 2, 2, ((2, 2, 1), (2, 2))), 24577: (238, 2, 2, ((2, 2, 2, 1), (2, 2, 2)))},
}
TABLE = TABLE4 if WAVES4 else TABLE8
SAT_ROWS = {'mlp2': 24577 if WAVES4 else 28673, 'global': 24577 if WAVES4 else 32769, 'lfwd': 24577 if WAVES4 else 12289,
            'lbwd': 12289}              # two chunks per workgroup (lfwd under 4 waves: four)


def _regime(kind, rows):
    """Assert that `rows` lands in the regime its table entry names."""
    p = _plan(kind, rows)
    grid, cmt, mtx, walks = TABLE[kind][rows]
    inst = _instance(kind, p)
    assert (p['grid'], p['cmt'], inst[0], _walks(p)) == (grid, cmt, mtx, walks), (kind, rows, p, inst, _walks(p))
    assert inst[1] == (4 if p['paired'] else 8) and p['cmt'] <= inst[0]
    if not p['paired']:
        assert (p['pb'] != 0) == (len(walks) == 2)          # the uneven deal: pb workgroups carry one tile more
    return p


def _pair_plans(rows, edges):
    """edge_chain.hip pamnet_local_bwd_pair_f32: (edge share before the clamps, edge plan, MLP plan)."""
    we, wm = PAIR_EDGE_COST * edges, float(rows)
    raw = int(N_CU * we / (we + wm) + 0.5)
    pe = plan8(edges, 3, min(max(raw, 8), N_CU - 8))
    return raw, pe, plan8(rows, 7, N_CU - pe['grid'])


# (rows, n_edges) -> (clamp of the edge share, chunks per workgroup of the edge half, MLP half: tiles per chunk, chunks)
PAIR_CASES = {
    (700, 9000): ('high', 1, 1, 1),            # MLP half <3>
    (4000, 9000): (None, 1, 4, 1),             # <5>
    (17640, 4316): (None, 1, 7, 1),            # <7>: the QM9 batch
    (40000, 100): ('low', 1, 6, 2),            # <7>, two chunks of the MLP half
    (100, 40000): ('high', 4, 1, 1),           # four chunks of the edge half
    (60000, 3000): (None, 2, 6, 3),            # several chunks on both halves
    (40, 0): None, (0, 33): None,              # nothing to pair: the entry makes the one launch that has rows
}


# ------------------------------------------------------------------------------------------ operands
@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs an MI355X'
    from pamnet_amd import lib
    lib.load()                                    # fail loudly if the HIP library is missing
    return torch.device('cuda:0')


def _gen(dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return g


def _nan(dev, *shape):
    return torch.full(shape, NAN, device=dev)


def _st(dev):
    from pamnet_amd import lib
    return lib.stream_of(torch.empty(1, device=dev))


def _rows_in(values):
    """A row operand [rows, 128] with a NaN row behind its last row."""
    rows = values.shape[0]
    buf = _nan(values.device, rows + 1, D)
    buf[:rows] = values
    return buf[:rows]


class _Out:
    """An output [rows, 128]: NaN (or `start`, for accumulation) between two NaN guard rows on either side."""

    def __init__(self, dev, rows, start=None):
        self.rows, self.buf = rows, _nan(dev, rows + 4, D)
        self.v = self.buf[2:2 + rows]
        if start is not None:
            self.v.copy_(start)
        self.p = self.buf.data_ptr() + 4 * 2 * D

    def guards_intact(self):
        return bool(torch.isnan(self.buf[:2]).all()) and bool(torch.isnan(self.buf[2 + self.rows:]).all())

    def untouched(self):
        return bool(torch.isnan(self.buf).all())


class _W:
    """A [128, 128] weight as the last column block of rows 1..128 of a NaN [130, ld] tensor; .w: the clean matrix."""

    def __init__(self, g, dev, ld=D, scale=0.08):
        self.w, self.ld = scale * torch.randn(D, D, generator=g, device=dev), ld
        self.buf = _nan(dev, D + 2, ld)
        self.buf[1:D + 1, ld - D:] = self.w
        self.p = self.buf.data_ptr() + 4 * (ld + ld - D)


class _B:
    """A bias [128] as elements 4..131 of a NaN vector."""

    def __init__(self, g, dev):
        self.b, self.buf = 0.1 * torch.randn(D, generator=g, device=dev), _nan(dev, D + 8)
        self.buf[4:4 + D] = self.b
        self.p = self.buf.data_ptr() + 16


def _rn(g, dev, rows, scale=0.5):
    return scale * torch.randn(rows, D, generator=g, device=dev)


def _saturated(g, dev, rows):
    """Saved pre-activations: half spread over [-100, 100] (exp overflows, SiLU saturates on both sides), the rest around +-2."""
    far = (torch.rand(rows, D, generator=g, device=dev) * 2 - 1) * 100
    return torch.where(torch.rand(rows, D, generator=g, device=dev) < 0.5, far, 2 * torch.randn(rows, D, generator=g, device=dev))


def _graph(g, dev, rows):
    """row_of sorted by target with a long run of node 0 and the first and the last node present, col arbitrary; few enough nodes
    that rows repeat inside a 16-row tile -> (n_nodes, row_of, col)"""
    n = max(1, min(rows // 8, 4096)) + 1
    ids = torch.cat([torch.zeros(rows // 4, dtype=torch.int64, device=dev),
                     torch.randint(0, n, (rows - rows // 4,), generator=g, device=dev)])
    row_of = ids.sort()[0]
    row_of[-1] = n - 1
    col = torch.randint(0, n, (rows,), generator=g, device=dev)
    return n, row_of.to(torch.int32), col.to(torch.int32)


def _parr(ps):
    return (ctypes.c_void_p * len(ps))(*ps)


def _iarr(vs):
    return (ctypes.c_int64 * len(vs))(*vs)


def _images(dev, ws, transposed):
    """pamnet_pack_weights_mixed_f32 kind-1 images of the slices `ws` (as they sit in their wide tensors) -> (addresses, keepalive)"""
    from pamnet_amd import lib
    n = len(ws)
    images = _nan(dev, (n + 1) * IMG)
    lib.call('pamnet_pack_weights_mixed_f32', n, _parr([w.p for w in ws]), _iarr([w.ld for w in ws]),
             (ctypes.c_int32 * n)(*([1] * n)), _iarr([i * IMG for i in range(n)]), transposed, images.data_ptr(), _st(dev))
    assert bool(torch.isnan(images[n * IMG:]).all())
    assert not bool(torch.isnan(images[:n * IMG]).any())        # every word written (no bf16 piece of a finite weight is NaN)
    return [images.data_ptr() + 4 * i * IMG for i in range(n)], images


# ------------------------------------------------------------------------------------------ the rule
def _silu(z):
    return z * torch.sigmoid(z)


def _dsilu(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def _both(fn, *tensors):
    """fn on the tensors as fp64 and as fp32 -> [(fp64 result, fp32 result), ...]"""
    r64 = fn(*[t.double() if t.is_floating_point() else t for t in tensors])
    r32 = fn(*tensors)
    return list(zip(r64, r32))


def _check(entry, name, got, ref, tag):
    """The fp64 rule for one output tensor; ref = (fp64 result, torch's fp32 result)."""
    r64, r32 = ref
    assert got.shape == r64.shape, (entry, name, tag)
    if got.numel() == 0:
        return
    assert bool(torch.isfinite(got).all()), (entry, name, tag)
    scale = max(float(r64.abs().max()), 1e-300)
    e = float((got.double() - r64).abs().max()) / scale
    f = float((r32.double() - r64).abs().max()) / scale
    bound = max(2e-6, 2 * f)
    if entry not in WORST or e / bound > WORST[entry][0] / max(2e-6, 2 * WORST[entry][1]):
        WORST[entry] = (e, f, '%s %s' % (name, tag))
    assert e <= bound, (entry, name, tag, e, f)


def _report(entry):
    if entry in WORST:
        print('edge-chain %s (%s waves): worst (err, floor) so far = (%.2e, %.2e) at %s'
              % (entry, 4 if WAVES4 else 8, WORST[entry][0], WORST[entry][1], WORST[entry][2]))


def _same_bits(a, b):
    return all(torch.equal(x.v, y.v) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------ the triplet / pair MLP
class _Mlp2Set:
    def __init__(self, g, dev):
        self.W1, self.b1, self.W2, self.b2 = _W(g, dev), _B(g, dev), _W(g, dev), _B(g, dev)

    def params(self):
        return [self.W1.p, self.b1.p, self.W2.p, self.b2.p]

    def ref(self, x):
        def f(x, W1, b1, W2, b2):
            z1 = x @ W1.t() + b1
            z2 = _silu(z1) @ W2.t() + b2
            return z1, z2, _silu(z2)
        return _both(f, x, self.W1.w, self.b1.b, self.W2.w, self.b2.b)


def _mlp2_fwd_case(dev, rows, xscale=0.5):
    from pamnet_amd import lib
    _regime('mlp2', rows)
    g = _gen(dev, 11 + rows)
    x, s = _rows_in(_rn(g, dev, rows, xscale)), _Mlp2Set(g, dev)
    ref = s.ref(x)

    def run(save):
        outs = [_Out(dev, rows) for _ in range(3)]
        lib.call('pamnet_mlp2_fwd_f32', x.data_ptr(), rows, *s.params(), outs[0].p if save else None,
                 outs[1].p if save else None, outs[2].p, _st(dev))
        assert all(o.guards_intact() for o in outs), rows
        return outs

    a, b, c = run(True), run(True), run(False)
    for name, o, r in zip(('z1', 'z2', 'y'), a, ref):
        _check('mlp2_fwd', name, o.v, r, 'rows %d x %.1f' % (rows, xscale))
    assert _same_bits(a, b) and torch.equal(a[2].v, c[2].v) and c[0].untouched() and c[1].untouched()
    _report('mlp2_fwd')


@pytest.mark.parametrize('rows', sorted(TABLE['mlp2']))
def test_mlp2_fwd(dev, rows):
    """pamnet_mlp2_fwd_f32: z1, z2, y against fp64 with and without the saves, twice."""
    _mlp2_fwd_case(dev, rows)


def _mlp2_multi_case(dev, rows, nsets, xscale=0.5):
    from pamnet_amd import lib
    _regime('mlp2', rows)
    g = _gen(dev, 17 + rows + nsets)
    x = _rows_in(_rn(g, dev, rows, xscale))
    sets = [_Mlp2Set(g, dev) for _ in range(nsets)]
    # saves: set k % 3 == 0 both, 1 neither, 2 z1 only
    given = [(k % 3 != 1, k % 3 == 0, True) for k in range(nsets)]

    def run():
        outs = [[_Out(dev, rows) for _ in range(3)] for _ in range(nsets)]
        lib.call('pamnet_mlp2_fwd_multi_f32', x.data_ptr(), rows, nsets, _parr([p for s in sets for p in s.params()]),
                 _parr([o.p if w else None for os_, ws in zip(outs, given) for o, w in zip(os_, ws)]), _st(dev))
        return outs

    a, b = run(), run()
    for k, s in enumerate(sets):
        ref = s.ref(x)
        for name, o, o2, r, w in zip(('z1', 'z2', 'y'), a[k], b[k], ref, given[k]):
            if w:
                assert o.guards_intact(), (rows, nsets, k, name)
                _check('mlp2_fwd_multi', name, o.v, r, 'rows %d set %d of %d' % (rows, k, nsets))
                assert torch.equal(o.v, o2.v), (rows, nsets, k, name)
            else:
                assert o.untouched(), (rows, nsets, k, name)
    if nsets > 1:
        assert not torch.equal(a[0][2].v, a[1][2].v)        # distinct weights per set
    _report('mlp2_fwd_multi')


@pytest.mark.parametrize('nsets', [1, 3, 8])
@pytest.mark.parametrize('rows', [17, SAT_ROWS['mlp2']])
def test_mlp2_fwd_multi(dev, rows, nsets):
    """pamnet_mlp2_fwd_multi_f32 (the form the engine runs): nsets weight sets on the same rows as grid.y, z1 / z2 null for
    some sets; every set against fp64."""
    _mlp2_multi_case(dev, rows, nsets)


class _Mlp2Bwd:
    """Operands and references of the MLP's backward (either entry point that runs it)."""

    def __init__(self, g, dev, rows, sat=False):
        r1 = max(rows, 1)
        mk = (lambda: _saturated(g, dev, r1)) if sat else (lambda: _rn(g, dev, r1))
        self.rows, self.dev = rows, dev
        self.dy, self.z1, self.z2 = _rows_in(_rn(g, dev, r1)[:rows]), _rows_in(mk()[:rows]), _rows_in(mk()[:rows])
        self.W1, self.W2, self.dx0 = _W(g, dev), _W(g, dev), _rn(g, dev, r1)[:rows]
        self._ref = None

    def ref(self, acc):
        if self._ref is None:
            def f(dy, z1, z2, W1, W2, dx0):
                dz2 = dy * _dsilu(z2)
                dz1 = (dz2 @ W2) * _dsilu(z1)
                dx = dz1 @ W1
                return dz1, dz2, dx, dx + dx0
            self._ref = _both(f, self.dy, self.z1, self.z2, self.W1.w, self.W2.w, self.dx0)
        return self._ref[:2] + [self._ref[3 if acc else 2]]

    def outs(self, acc):
        return [_Out(self.dev, self.rows), _Out(self.dev, self.rows), _Out(self.dev, self.rows, self.dx0 if acc else None)]

    def args(self, outs, W=None):
        W = W or (self.W1.p, self.W2.p)
        return [self.dy.data_ptr(), self.rows, self.z1.data_ptr(), self.z2.data_ptr(), W[0], W[1]] + [o.p for o in outs]

    def check(self, entry, outs, acc, tag):
        assert all(o.guards_intact() for o in outs), tag
        for name, o, r in zip(('dz1', 'dz2', 'dx'), outs, self.ref(acc)):
            _check(entry, name, o.v, r, tag)


def _mlp2_bwd_case(dev, rows, sat=False):
    from pamnet_amd import lib
    _regime('mlp2', rows)
    m = _Mlp2Bwd(_gen(dev, 23 + rows), dev, rows, sat)
    for acc in (0, 1):
        runs = []
        for _ in range(2):
            outs = m.outs(acc)
            lib.call('pamnet_mlp2_bwd_f32', *m.args(outs), acc, _st(dev))
            runs.append(outs)
        m.check('mlp2_bwd', runs[0], acc, 'rows %d acc %d%s' % (rows, acc, ' saturated' if sat else ''))
        assert _same_bits(*runs), (rows, acc)
    _report('mlp2_bwd')


@pytest.mark.parametrize('rows', sorted(TABLE['mlp2']))
def test_mlp2_bwd(dev, rows):
    """pamnet_mlp2_bwd_f32: dz1, dz2, dx against fp64, overwriting and accumulating into a random dx, twice each."""
    _mlp2_bwd_case(dev, rows)


# ------------------------------------------------------------------------------------------ global edges
def _global_fwd_case(dev, rows, escale=0.5):
    from pamnet_amd import lib
    _regime('global', rows)
    g = _gen(dev, 31 + rows)
    n, row_of, col = _graph(g, dev, rows)
    e, Pi, Pj = _rows_in(_rn(g, dev, rows, escale)), _rows_in(_rn(g, dev, n)), _rows_in(_rn(g, dev, n))
    We, bm, Wea = _W(g, dev, 3 * D), _B(g, dev), _W(g, dev)

    def f(e, We, bm, Wea, Pi, Pj, row_of, col):
        z = e @ We.t() + bm + Pi[row_of.long()] + Pj[col.long()]
        ea = e @ Wea.t()
        return z, ea, _silu(z) * ea
    ref = _both(f, e, We.w, bm.b, Wea.w, Pi, Pj, row_of, col)

    def run(save):
        outs = [_Out(dev, rows) for _ in range(3)]
        lib.call('pamnet_global_edge_fwd_f32', e.data_ptr(), rows, We.p, We.ld, bm.p, Wea.p, Wea.ld, Pi.data_ptr(), Pj.data_ptr(),
                 row_of.data_ptr(), col.data_ptr(), outs[0].p if save else None, outs[1].p if save else None, outs[2].p, _st(dev))
        assert all(o.guards_intact() for o in outs), rows
        return outs

    a, b, c = run(True), run(True), run(False)
    for name, o, r in zip(('z', 'ea', 'msg'), a, ref):
        _check('global_edge_fwd', name, o.v, r, 'rows %d e x %.1f' % (rows, escale))
    assert _same_bits(a, b) and torch.equal(a[2].v, c[2].v) and c[0].untouched() and c[1].untouched()
    _report('global_edge_fwd')


@pytest.mark.parametrize('rows', sorted(TABLE['global']))
def test_global_edge_fwd(dev, rows):
    """pamnet_global_edge_fwd_f32: z, ea, msg against fp64 (W_e a column block with ld 384), with and without the saves, twice."""
    _global_fwd_case(dev, rows)


def _global_bwd_case(dev, rows, sat=False):
    from pamnet_amd import lib
    _regime('global', rows)
    g = _gen(dev, 37 + rows)
    n, row_of, _ = _graph(g, dev, rows)
    d_agg, ea = _rows_in(_rn(g, dev, n)), _rows_in(_rn(g, dev, rows))
    z = _rows_in(_saturated(g, dev, rows) if sat else _rn(g, dev, rows))
    We, Wea, de0 = _W(g, dev, 3 * D), _W(g, dev), _rn(g, dev, rows)

    def f(d_agg, row_of, z, ea, We, Wea, de0):
        dm = d_agg[row_of.long()]
        dz = dm * ea * _dsilu(z)
        dea = dm * _silu(z)
        d_e = dz @ We + dea @ Wea
        return dz, dea, d_e, d_e + de0
    ref = _both(f, d_agg, row_of, z, ea, We.w, Wea.w, de0)
    for acc in (0, 1):
        runs = []
        for _ in range(2):
            outs = [_Out(dev, rows), _Out(dev, rows), _Out(dev, rows, de0 if acc else None)]
            lib.call('pamnet_global_edge_bwd_f32', d_agg.data_ptr(), row_of.data_ptr(), rows, z.data_ptr(), ea.data_ptr(), We.p,
                     We.ld, Wea.p, Wea.ld, *[o.p for o in outs], acc, _st(dev))
            assert all(o.guards_intact() for o in outs), (rows, acc)
            runs.append(outs)
        for name, o, r in zip(('dz', 'dea', 'd_e'), runs[0], ref[:2] + [ref[3 if acc else 2]]):
            _check('global_edge_bwd', name, o.v, r, 'rows %d acc %d%s' % (rows, acc, ' saturated' if sat else ''))
        assert _same_bits(*runs), (rows, acc)
    _report('global_edge_bwd')


@pytest.mark.parametrize('rows', sorted(TABLE['global']))
def test_global_edge_bwd(dev, rows):
    """pamnet_global_edge_bwd_f32: dz, dea, d_e against fp64, overwriting and accumulating, twice each."""
    _global_bwd_case(dev, rows)


# ------------------------------------------------------------------------------------------ local edges
class _LocalW:
    """Wq = {W_ji[:, 2d:], W_kj[:, 2d:] (ld 384), lin_rbf, lin_rbf_out (ld 128)} and their images (made on first use)."""

    def __init__(self, g, dev):
        self.dev, self.W = dev, [_W(g, dev, 3 * D), _W(g, dev, 3 * D), _W(g, dev), _W(g, dev)]
        self._img = {}

    def plain(self):
        return _parr([w.p for w in self.W]), _iarr([w.ld for w in self.W])

    def images(self, transposed):
        if transposed not in self._img:
            self._img[transposed] = _images(self.dev, self.W, transposed)
        return _parr(self._img[transposed][0]), _iarr([0, 0, 0, 0])


def _local_fwd_case(dev, rows, rscale=0.5):
    from pamnet_amd import lib
    _regime('lfwd', rows)
    g = _gen(dev, 41 + rows)
    n, row_of, col = _graph(g, dev, rows)
    rbf, P = _rows_in(_rn(g, dev, rows, rscale)), [_rows_in(_rn(g, dev, n)) for _ in range(4)]
    lw, b_ji, b_kj = _LocalW(g, dev), _B(g, dev), _B(g, dev)

    def f(r, W0, W1, W2, W3, b_ji, b_kj, P0, P1, P2, P3, row_of, col):
        i, j = row_of.long(), col.long()
        z_ji = r @ W0.t() + b_ji + P0[i] + P2[j]
        z_kj = r @ W1.t() + b_kj + P1[i] + P3[j]
        q2, q3 = r @ W2.t(), r @ W3.t()
        return z_ji, z_kj, q2, q3, _silu(z_ji), _silu(z_kj) * q2
    ref = _both(f, rbf, *[w.w for w in lw.W], b_ji.b, b_kj.b, *P, row_of, col)
    names = ('z_ji', 'z_kj', 'q2', 'q3', 'm_ji', 'm_nb')

    def run(w, save):
        outs = [_Out(dev, rows) for _ in range(6)]
        lib.call('pamnet_local_edge_fwd_f32', rbf.data_ptr(), rows, w[0], w[1], b_ji.p, b_kj.p, _parr([p.data_ptr() for p in P]),
                 row_of.data_ptr(), col.data_ptr(), *[o.p if save or k >= 3 else None for k, o in enumerate(outs)], _st(dev))
        assert all(o.guards_intact() for o in outs), rows
        return outs

    for form in ('matrices', 'images'):
        w = lw.plain() if form == 'matrices' else lw.images(0)
        if form == 'images' and WAVES4:                     # the paired 4-wave geometry multiplies fp32 fragments
            with pytest.raises(RuntimeError, match='EINVAL'):
                run(w, True)
            continue
        a, b, c = run(w, True), run(w, True), run(w, False)
        for name, o, r in zip(names, a, ref):
            _check('local_edge_fwd', name, o.v, r, 'rows %d %s r x %.1f' % (rows, form, rscale))
        assert _same_bits(a, b) and _same_bits(a[3:], c[3:]) and all(o.untouched() for o in c[:3]), (rows, form)
    _report('local_edge_fwd')


@pytest.mark.parametrize('rows', sorted(TABLE['lfwd']))
def test_local_edge_fwd(dev, rows):
    """pamnet_local_edge_fwd_f32 (grid.y = 2, half the CUs per half) on strided matrices and on fragment images (the engine's
    form; refused under the forced 4-wave geometry): six outputs against fp64, with and without the saves, twice."""
    _local_fwd_case(dev, rows)


class _LocalBwd:
    """Operands and references of the local edge backward (either entry point that runs it)."""

    def __init__(self, g, dev, rows, sat=False):
        r1 = max(rows, 1)
        mk = (lambda: _saturated(g, dev, r1)) if sat else (lambda: _rn(g, dev, r1))
        self.rows, self.dev = rows, dev
        self.d_mji, self.d_mnb, self.d_q3 = (_rows_in(_rn(g, dev, r1)[:rows]) for _ in range(3))
        self.z_ji, self.z_kj, self.q2 = _rows_in(mk()[:rows]), _rows_in(mk()[:rows]), _rows_in(_rn(g, dev, r1)[:rows])
        self.lw, self.d0 = _LocalW(g, dev), _rn(g, dev, r1)[:rows]
        self._ref = None

    def ref(self, acc):
        """Autograd through the forward's formulas: with r = 0 and the saved values as the additive terms, z_ji, z_kj and q2 ARE
        the saved values, and the gradient with respect to r is d_rbf."""
        if self._ref is None:
            def f(d_mji, d_mnb, d_q3, z_ji, z_kj, q2, W0, W1, W2, W3, d0):
                with torch.enable_grad():
                    r = torch.zeros_like(z_ji, requires_grad=True)
                    zji, zkj, qq2, qq3 = r @ W0.t() + z_ji, r @ W1.t() + z_kj, r @ W2.t() + q2, r @ W3.t()
                    loss = (d_mji * _silu(zji)).sum() + (d_mnb * (_silu(zkj) * qq2)).sum() + (d_q3 * qq3).sum()
                    dzji, dzkj, dq2, dr = torch.autograd.grad(loss, [zji, zkj, qq2, r])
                return dzji, dzkj, dq2, dr, dr + d0
            self._ref = _both(f, self.d_mji, self.d_mnb, self.d_q3, self.z_ji, self.z_kj, self.q2, *[w.w for w in self.lw.W],
                              self.d0)
        return self._ref[:3] + [self._ref[4 if acc else 3]]

    def outs(self, acc):
        return [_Out(self.dev, self.rows) for _ in range(3)] + [_Out(self.dev, self.rows, self.d0 if acc else None)]

    def args(self, outs, w):
        return [self.d_mji.data_ptr(), self.d_mnb.data_ptr(), self.d_q3.data_ptr(), self.rows, self.z_ji.data_ptr(),
                self.z_kj.data_ptr(), self.q2.data_ptr(), w[0], w[1]] + [o.p for o in outs]

    def check(self, entry, outs, acc, tag):
        assert all(o.guards_intact() for o in outs), tag
        for name, o, r in zip(('dz_ji', 'dz_kj', 'dq2', 'd_rbf'), outs, self.ref(acc)):
            _check(entry, name, o.v, r, tag)


def _local_bwd_case(dev, rows, sat=False):
    from pamnet_amd import lib
    _regime('lbwd', rows)
    m = _LocalBwd(_gen(dev, 43 + rows), dev, rows, sat)
    for form in ('matrices', 'images'):
        w = m.lw.plain() if form == 'matrices' else m.lw.images(1)
        for acc in (0, 1):
            runs = []
            for _ in range(2):
                outs = m.outs(acc)
                lib.call('pamnet_local_edge_bwd_f32', *m.args(outs, w), acc, _st(dev))
                runs.append(outs)
            m.check('local_edge_bwd', runs[0], acc, 'rows %d %s acc %d%s' % (rows, form, acc, ' saturated' if sat else ''))
            assert _same_bits(*runs), (rows, form, acc)
    _report('local_edge_bwd')


@pytest.mark.parametrize('rows', sorted(TABLE['lbwd']))
def test_local_edge_bwd(dev, rows):
    """pamnet_local_edge_bwd_f32 (always 8 waves, <= 3 tiles per chunk) on strided matrices and on transposed fragment images:
    dz_ji, dz_kj, dq2, d_rbf against fp64 autograd, overwriting and accumulating, twice each."""
    _local_bwd_case(dev, rows)


# ------------------------------------------------------------------------------------------ the paired backward launch
def _pair_case(dev, rows, edges, sat=False):
    from pamnet_amd import lib
    want = PAIR_CASES[(rows, edges)]
    if want is not None and not WAVES4:                     # (forced 4-wave geometry: two launches, planned as the plain entries)
        raw, pe, pm = _pair_plans(rows, edges)
        clamp = 'low' if raw < 8 else ('high' if raw > N_CU - 8 else None)
        got = (clamp, len(_walks(pe)[0]), pm['cmt'], len(_walks(pm)[0]))
        assert got == want and pe['cmt'] <= 3 and pe['grid'] + pm['grid'] <= N_CU, (rows, edges, raw, pe, pm)
    g = _gen(dev, 47 + rows + edges)
    mm, ml = _Mlp2Bwd(g, dev, rows, sat), _LocalBwd(g, dev, edges, sat)
    for form in ('matrices', 'images'):
        if form == 'images' and want is None:
            continue                                        # (images: the paired launch only)
        if form == 'matrices':
            W, w, flag = None, ml.lw.plain(), 0
        else:
            W, keep = _images(dev, [mm.W1, mm.W2], 1)
            w, flag = ml.lw.images(1), 2                    # PAMNET_WEIGHT_IMAGES
        for acc_dx, acc_rbf in ((0, 1), (1, 0)):
            runs = []
            for _ in range(2):
                om, ol = mm.outs(acc_dx), ml.outs(acc_rbf)
                call = lambda: lib.call('pamnet_local_bwd_pair_f32', *mm.args(om, W), acc_dx | flag, *ml.args(ol, w), acc_rbf,
                                        _st(dev))
                if form == 'images' and WAVES4:             # images: the paired 8-wave launch only
                    with pytest.raises(RuntimeError, match='EINVAL'):
                        call()
                    break
                call()
                runs.append(om + ol)
            if not runs:
                continue
            tag = 'rows %d edges %d %s acc %d/%d%s' % (rows, edges, form, acc_dx, acc_rbf, ' saturated' if sat else '')
            if rows:
                mm.check('local_bwd_pair', runs[0][:3], acc_dx, tag)
            else:
                assert all(o.untouched() for o in runs[0][:3])
            if edges:
                ml.check('local_bwd_pair', runs[0][3:], acc_rbf, tag)
            else:
                assert all(o.untouched() for o in runs[0][3:])
            assert _same_bits(*runs), tag
    _report('local_bwd_pair')


@pytest.mark.parametrize('rows,edges', sorted(PAIR_CASES))
def test_local_bwd_pair(dev, rows, edges):
    """pamnet_local_bwd_pair_f32 on matrices and on weight images (PAMNET_WEIGHT_IMAGES + four zero strides: the engine's form;
    refused under the forced 4-wave geometry, where the entry makes two launches): all seven outputs against fp64, the two
    accumulate flags set differently (0 / 1 and 1 / 0), twice each; a half without rows leaves its outputs untouched."""
    _pair_case(dev, rows, edges)


# ------------------------------------------------------------------------------------------ 5. value edges
@pytest.mark.parametrize('entry', ['mlp2_fwd', 'mlp2_fwd_multi', 'global_edge_fwd', 'local_edge_fwd'])
def test_saturated_forward(dev, entry):
    """Inputs scaled (x 30) so that the pre-activations reach +-100 and beyond: exp overflows, SiLU saturates on both sides.
    Finite outputs, the same rule."""
    if entry == 'mlp2_fwd':
        _mlp2_fwd_case(dev, SAT_ROWS['mlp2'], 30.0)
    elif entry == 'mlp2_fwd_multi':
        _mlp2_multi_case(dev, SAT_ROWS['mlp2'], 3, 30.0)
    elif entry == 'global_edge_fwd':
        _global_fwd_case(dev, SAT_ROWS['global'], 30.0)
    else:
        _local_fwd_case(dev, SAT_ROWS['lfwd'], 30.0)


@pytest.mark.parametrize('entry', ['mlp2_bwd', 'global_edge_bwd', 'local_edge_bwd', 'local_bwd_pair'])
def test_saturated_backward(dev, entry):
    """Half of the saved pre-activations (z1, z2 / z / z_ji, z_kj) spread over [-100, 100], the rest around +-2.  Finite outputs,
    the same rule."""
    if entry == 'mlp2_bwd':
        _mlp2_bwd_case(dev, SAT_ROWS['mlp2'], True)
    elif entry == 'global_edge_bwd':
        _global_bwd_case(dev, SAT_ROWS['global'], True)
    elif entry == 'local_edge_bwd':
        _local_bwd_case(dev, SAT_ROWS['lbwd'], True)
    else:
        _pair_case(dev, 17640, 4316, True)


# ------------------------------------------------------------------------------------------ 6. the 4-wave geometry
def test_four_wave_geometry():
    """Every test of this file again in ONE fresh child process with PAMNET_EDGE_WAVES=4 (the library reads the switch once per
    process): the paired 4-wave tables above, pamnet_local_edge_fwd_f32 and pamnet_local_bwd_pair_f32 refuse images,
    the pair entry makes two launches and meets the same rule."""
    here = os.path.abspath(__file__)
    env = dict(os.environ, PAMNET_EDGE_WAVES='4')
    out = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-s', '-m', 'gpu', here, '-k', 'not four_wave_geometry'],
                         capture_output=True, text=True, env=env, timeout=600, cwd=os.path.dirname(os.path.dirname(here)))
    last = {}
    for line in out.stdout.splitlines():
        if 'edge-chain ' in line:
            line = line[line.index('edge-chain '):]
            last[line.split()[1]] = line
    print('\n'.join(last[k] for k in sorted(last)))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-1000:]
