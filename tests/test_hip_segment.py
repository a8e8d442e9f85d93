"""Kernel-level tests of csrc/segment.hip: every launch form of pamnet_segment_sum_f32 (wide / split / striding split /
plain / generic) with every operand set, pamnet_gather_mul_f32, pamnet_gather_mul2_f32 and pamnet_segment_sum_multi_f32,
against fp64 torch on the device.

Two kinds of input:
  * integer-valued fp32 data (torch.randint(-8, 9)): every product is at most 64 in magnitude, every segment has at most
    100 000 terms, so every partial sum stays below 2^24 and the fp32 result is exact in ANY summation order -- the fp64
    index_add_ reference cast to fp32 must be equal bit for bit (a dropped, duplicated or mis-indexed term cannot hide);
  * randn data against fp64: maxnorm_err < 2e-6 where no segment exceeds 70 terms (the bound of test_hip_kernels.py);
    max(2e-6, 2 x floor) where one does, floor = the error of torch's own fp32 index_add_ on the same operands
    (the rule of test_hip_dense.py:_bound).  One such case per kernel form; both figures are printed.
Every case runs twice (bitwise equal: the file promises a fixed summation order) into the middle of a NaN-filled buffer
(the guard rows stay NaN, every row inside is finite).

The GPU tests carry the `gpu` mark one by one, not through a module-level `pytestmark`: the two tests at the bottom pin
the shape table to the dispatch constants of segment.hip and run without a GPU (a third checks that no other test of
this file lacks the mark)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import maxnorm_err

gpu = pytest.mark.gpu

# ---- the shape table, derived from the dispatch rule of launch_segment_sum (csrc/segment.hip) ---------------------------
# With LPR = d / 4 lanes per row (a power of two <= 64) and 256 / LPR lane groups ("slots") in a workgroup:
#   wide   segment_sum_split_kernel<LPR, 256 / LPR>   rows <= 64 and 256 / LPR > 4: a whole workgroup per row
#   split  segment_sum_split_kernel<LPR, 4>           rows * LPR <= SPLIT_MAX_LANES, i.e. rows <= T(d)
#   plain  segment_sum_kernel                         rows > T(d)
# The grid is capped at 256 * 64 blocks.  A plain block owns 256 / LPR rows, so one grid pass covers CAP(d) = 4 T(d) rows
# and the plain kernel grid-strides above that.  A split block owns 256 / LPR / 4 rows: T(d) rows are exactly 256 * 64
# blocks, so through this entry point neither the split nor the wide kernel ever takes a second pass of its row loop.
#   d       4          8        16       32       64      128     256
#   T(d)    1 048 576  524 288  262 144  131 072  65 536  32 768  16 384
#   CAP(d)  4 194 304  2 097 152  1 048 576  524 288  262 144  131 072  65 536
SPLIT_MAX_LANES = 256 * 4 * 64 * 4 * 4        # = 1 048 576
WIDE_MAX_ROWS = 64
GRID_CAP = 256 * 64                           # blocks (gather_mul / gather_mul2: blocks of 256 float4)
GENERIC_CAP_ROWS = 256 * 32 * 4               # generic kernel: 256 * 32 blocks of four waves, one wave per row
POW2 = (4, 8, 16, 32, 64, 128, 256)
LONG = (0, 3001, 1, 449, 64)                  # the wide form's rows: hundreds to thousands of terms


def T(d):
    """Largest row count of the split kernel at width d; the plain kernel runs above it."""
    return SPLIT_MAX_LANES // (d // 4)


def CAP(d):
    """Rows of one full grid pass of the plain kernel."""
    return GRID_CAP * (256 // (d // 4))


def plain_rows(d):
    """A partial second grid pass of the plain kernel and a ragged last block."""
    return CAP(d) + CAP(d) // 4 + 3


def route(d, rows):
    """The launch form pamnet_segment_sum_f32 picks -- launch_segment_sum restated."""
    lpr = d // 4
    if lpr > 64 or lpr & (lpr - 1):
        return 'generic-stride' if rows > GENERIC_CAP_ROWS else 'generic'
    slots = 256 // lpr
    split = 4 if slots >= 4 else 1
    if slots > split and rows <= WIDE_MAX_ROWS:
        return 'wide'
    if split > 1 and rows * lpr <= SPLIT_MAX_LANES:
        assert -(-rows // (slots // split)) <= GRID_CAP          # (never strides: see above)
        return 'split'
    return 'plain-stride' if -(-rows // slots) > GRID_CAP else 'plain'


GM_STRIDE = GRID_CAP * 256 // 32 + 40001      # gather_mul rows at d = 128: 131 072 fill the capped grid once

# (group, d, rows, expected form)
CASES = (
    [('A', d, plain_rows(d), 'plain-stride') for d in POW2]
    + [('B', d, plain_rows(d), 'plain-stride') for d in (128, 16)]
    # every key: the plain kernel in a single grid pass (49 155 and 24 579 rows), the split kernel at a small grid and at
    # its largest, with a ragged last block
    + [('C', 128, 49155, 'plain'), ('C', 256, 24579, 'plain'), ('C', 32, 5000, 'split'),
       ('C', 128, T(128) - 3, 'split'), ('C', 256, T(256) - 3, 'split')]
    + [('D', 16, 5, 'wide'), ('D', 128, 5, 'wide'), ('D', 64, 64, 'wide'), ('D', 64, 65, 'split'), ('D', 256, 5, 'split')]
    # either side of the split / plain line and of the plain kernel's one-pass / grid-stride line
    + [('E', d, rows, form) for d in (256, 128)
       for rows, form in ((T(d), 'split'), (T(d) + 1, 'plain'), (CAP(d), 'plain'), (CAP(d) + 1, 'plain-stride'))]
    + [('F', 128, 3000, 'split'), ('F', 128, plain_rows(128), 'plain-stride')]
    + [('G', 12, 40003, 'generic-stride'), ('G', 160, 40003, 'generic-stride'), ('G', 260, 3000, 'generic')]
    # every power-of-two width in every form it has (A adds the striding plain form)
    + [('W', d, 5, 'wide') for d in POW2 if d < 256]
    + [('W', d, 5000, 'split') for d in POW2]
    + [('W', d, T(d), 'split') for d in POW2]
    + [('W', d, T(d) + T(d) // 4 + 3, 'plain') for d in POW2]
)


def _cases(group):
    return [(d, rows) for g, d, rows, _ in CASES if g == group]


KEYS = (0, 1, 4, 5, 6, 7, 8, 9, 12, 13, 14, 15)      # ia = 8, B = 4, ib (with B) = 2, perm = 1
INIT_KEYS = (1, 5, 7, 8, 12, 14)                      # `init` on half of them
GM_KEYS = (0, 2, 3, 4, 6, 7)                          # gather_mul: ia = 4, B = 2, ib (with B) = 1
RA, RB = 1000, 777                                    # rows of the tables ia / ib index


# ---- inputs, built on the device ------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs an MI355X'
    from pamnet_amd import lib
    lib.load()
    return torch.device('cuda:0')


class _Csr(object):
    def __init__(self, lens):
        self.rows = lens.numel()
        ptr = torch.zeros(self.rows + 1, dtype=torch.int64, device=lens.device)
        ptr[1:] = lens.cumsum(0)
        self.ptr = ptr.to(torch.int32)
        self.seg = torch.repeat_interleave(torch.arange(self.rows, device=lens.device), lens)
        self.m, self.max_len = int(ptr[-1]), int(lens.max())
        assert self.max_len <= 100000 and self.seg.numel() == self.m


_CSRS = {}


def _csr(dev, kind, rows, arg=None):
    """kind 'big': 97 % of the rows 0..2 terms, 3 % 0..27 (mean ~1.4: the 8-deep, the 4-deep and the scalar loop all run),
    first and last row empty; 'uniform': 0..arg terms; 'list': arg; 'long': 'big' with 20 000 terms in the middle row and
    in the second-to-last row."""
    key = (kind, rows, arg)
    if key not in _CSRS:
        torch.manual_seed(rows * 7 + len(kind))
        if kind == 'list':
            lens = torch.tensor(arg, device=dev)
        elif kind == 'uniform':
            lens = torch.randint(0, arg + 1, (rows,), device=dev)
        else:
            lens = torch.where(torch.rand(rows, device=dev) < 0.03, torch.randint(0, 28, (rows,), device=dev),
                               torch.randint(0, 3, (rows,), device=dev))
            lens[0] = lens[-1] = 0
            if kind == 'long':
                lens[rows // 2] = lens[rows - 2] = 20000
        assert lens.numel() == rows
        _CSRS[key] = _Csr(lens)
    return _CSRS[key]


def _draw(kind, n, d, dev):
    if kind == 'int':
        return torch.randint(-8, 9, (n, d), dtype=torch.float32, device=dev)
    return torch.randn(n, d, device=dev)


class _Operands(object):
    """Operands of one segment-sum key over m terms, with the rows each one needs and no more."""

    def __init__(self, key, m, rows, d, dev, kind, with_init):
        i32 = dict(dtype=torch.int32, device=dev)
        self.ia = torch.randint(0, RA, (m,), **i32) if key & 8 else None
        self.A = _draw(kind, RA if key & 8 else m, d, dev)
        self.B = self.ib = None
        if key & 4:
            self.ib = torch.randint(0, RB, (m,), **i32) if key & 2 else None
            self.B = _draw(kind, RB if key & 2 else m, d, dev)
        self.perm = torch.randperm(m, **i32) if key & 1 else None
        self.init = _draw(kind, rows, d, dev) if with_init else None

    def terms(self, dtype):
        k = self.perm.long() if self.perm is not None else None
        ra = self.ia.long() if self.ia is not None else None
        if ra is not None and k is not None:
            ra = ra[k]
        elif ra is None:
            ra = k
        t = self.A.to(dtype) if ra is None else self.A.to(dtype)[ra]
        if self.B is not None:
            rb = self.ib.long() if self.ib is not None else None
            if rb is not None and k is not None:
                rb = rb[k]
            elif rb is None:
                rb = k
            t = t * (self.B.to(dtype) if rb is None else self.B.to(dtype)[rb])
        return t

    def reference(self, csr, dtype):
        d = self.A.size(1)
        base = self.init.to(dtype).clone() if self.init is not None else \
            torch.zeros(csr.rows, d, dtype=dtype, device=self.A.device)
        return base.index_add_(0, csr.seg, self.terms(dtype))


def _guarded(n, d, dev):
    buf = torch.full((n + 2, d), float('nan'), device=dev)
    return buf, buf[1:-1]


def _guards_hold(buf):
    return bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all()) and bool(torch.isfinite(buf[1:-1]).all())


def _segment_sum(o, csr, d):
    """Two runs into the middle of NaN-filled buffers: guards intact, rows finite, runs bitwise equal."""
    from pamnet_amd import ops
    outs = []
    for _ in range(2):
        buf, out = _guarded(csr.rows, d, o.A.device)
        ops.segment_sum_raw(out, o.init, o.A, o.ia, o.B, o.ib, o.perm, csr.ptr, csr.rows, d)
        assert _guards_hold(buf), 'a guard row was written or a row inside was not'
        outs.append(out)
    assert torch.equal(outs[0], outs[1]), 'two runs differ: the summation order is not fixed'
    return outs[0]


def _exact(dev, d, csr, key, with_init):
    torch.manual_seed(d * 1000003 + csr.rows * 17 + key)
    o = _Operands(key, csr.m, csr.rows, d, dev, 'int', with_init)
    out = _segment_sum(o, csr, d)
    ref = o.reference(csr, torch.float64).float()
    if not torch.equal(out, ref):
        bad = (out != ref).any(1).nonzero().view(-1)
        lens = (csr.ptr[1:] - csr.ptr[:-1])[bad[:8]].tolist()
        raise AssertionError('%s d=%d rows=%d key=%d init=%s: %d rows differ, first %s of %s terms'
                             % (route(d, csr.rows), d, csr.rows, key, with_init, bad.numel(), bad[:8].tolist(), lens))


def _close(dev, d, csr, key, with_init, label):
    torch.manual_seed(d * 1000003 + csr.rows * 17 + key + 1)
    o = _Operands(key, csr.m, csr.rows, d, dev, 'randn', with_init)
    out = _segment_sum(o, csr, d)
    ref = o.reference(csr, torch.float64).cpu()
    err = maxnorm_err(out.cpu(), ref)
    floor = maxnorm_err(o.reference(csr, torch.float32).cpu(), ref)
    bound = 2e-6 if csr.max_len <= 70 else max(2e-6, 2 * floor)
    print('segment randn %s (%s) d=%d rows=%d longest=%d: err %.3e  fp32 floor %.3e  bound %.3e'
          % (label, route(d, csr.rows), d, csr.rows, csr.max_len, err, floor, bound))
    assert err < bound, (err, floor, bound)


# ---- A. plain kernel, every width -----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('with_init', [False, True])
@pytest.mark.parametrize('d,rows', _cases('A'))
def test_plain_every_width(dev, d, rows, with_init):
    _exact(dev, d, _csr(dev, 'big', rows), 0, with_init)


@gpu
@pytest.mark.parametrize('d', [128, 16])
def test_plain_randn(dev, d):
    _close(dev, d, _csr(dev, 'big', plain_rows(d)), 0, True, 'plain')


# ---- B. plain kernel, every operand key -----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('key', KEYS)
@pytest.mark.parametrize('d,rows', _cases('B'))
def test_plain_every_key(dev, d, rows, key):
    _exact(dev, d, _csr(dev, 'big', rows), key, key in INIT_KEYS)


# ---- C. split kernel up to its largest grid, plain kernel in a single pass: every operand key ---------------------------
@gpu
@pytest.mark.parametrize('key', KEYS)
@pytest.mark.parametrize('d,rows', _cases('C'))
def test_split_and_single_pass_plain_every_key(dev, d, rows, key):
    _exact(dev, d, _csr(dev, 'uniform', rows, 40), key, key in INIT_KEYS)


# ---- D. wide kernel (a workgroup per row), long rows; the wide / split line -------------------------------------------------
@gpu
@pytest.mark.parametrize('key', KEYS)
@pytest.mark.parametrize('d', [16, 128])
def test_wide_every_key(dev, d, key):
    _exact(dev, d, _csr(dev, 'list', len(LONG), LONG), key, key in INIT_KEYS)


@gpu
def test_wide_randn(dev):
    _close(dev, 128, _csr(dev, 'list', len(LONG), LONG), 0, True, 'wide')


@gpu
@pytest.mark.parametrize('key', [0, 15])
@pytest.mark.parametrize('rows', [64, 65])
def test_wide_split_line(dev, rows, key):
    _exact(dev, 64, _csr(dev, 'uniform', rows, 300), key, key == 15)


@gpu
@pytest.mark.parametrize('key', [0, 15])
def test_few_long_rows_at_256(dev, key):
    """d = 256: a workgroup holds four lane groups, SPLIT_WIDE == SPLIT -- the split form runs however few the rows."""
    _exact(dev, 256, _csr(dev, 'list', len(LONG), LONG), key, key == 0)


# ---- E. the split / plain line (T, T + 1 rows) and the plain kernel's grid-stride line (CAP, CAP + 1 rows) -----------------
@gpu
@pytest.mark.parametrize('key', [0, 15])
@pytest.mark.parametrize('d,rows', _cases('E'))
def test_split_plain_and_stride_lines(dev, d, rows, key):
    _exact(dev, d, _csr(dev, 'big', rows), key, key == 15)


# ---- F. a long segment among many short ones --------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('key', [0, 15])
@pytest.mark.parametrize('d,rows', _cases('F'))
def test_long_segment_among_short(dev, d, rows, key):
    _exact(dev, d, _csr(dev, 'long', rows), key, key == 15)


@gpu
@pytest.mark.parametrize('d,rows', _cases('F'))
def test_long_segment_randn(dev, d, rows):
    _close(dev, d, _csr(dev, 'long', rows), 0, False, 'long segment')


# ---- G. generic kernel (d / 4 not a power of two) ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('key', [0, 1, 7, 8, 15])
@pytest.mark.parametrize('d,rows', _cases('G'))
def test_generic(dev, d, rows, key):
    _exact(dev, d, _csr(dev, 'uniform', rows, 20), key, key in (1, 15))


@gpu
def test_generic_randn(dev):
    _close(dev, 160, _csr(dev, 'uniform', 40003, 20), 0, True, 'generic')


# ---- every power-of-two width in every form it has --------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('key', [0, 15])
@pytest.mark.parametrize('d,rows', _cases('W'))
def test_every_width_every_form(dev, d, rows, key):
    form = route(d, rows)
    csr = _csr(dev, 'list', len(LONG), LONG) if form == 'wide' else \
        _csr(dev, 'uniform', rows, 40) if rows == 5000 else _csr(dev, 'big', rows)
    _exact(dev, d, csr, key, key == 15)


# ---- H. gather_mul ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('key', GM_KEYS)
@pytest.mark.parametrize('d,m', [(128, GM_STRIDE), (16, 1000), (12, 5003), (260, 5003)])
def test_gather_mul(dev, d, m, key):
    """out[k] = A[ia[k]] * B[ib[k]]: one rounding per element, so equal to the same expression in torch fp32."""
    from pamnet_amd import ops
    torch.manual_seed(d * 31 + key)
    i32 = dict(dtype=torch.int32, device=dev)
    ia = torch.randint(0, RA, (m,), **i32) if key & 4 else None
    A = torch.randn(RA if key & 4 else m, d, device=dev)
    B = ib = None
    if key & 2:
        ib = torch.randint(0, RB, (m,), **i32) if key & 1 else None
        B = torch.randn(RB if key & 1 else m, d, device=dev)
    want = A if ia is None else A[ia.long()]
    if B is not None:
        want = want * (B if ib is None else B[ib.long()])
    outs = []
    for _ in range(2):
        buf, out = _guarded(m, d, dev)
        ops.gather_mul_raw(out, A, ia, B, ib, m, d)
        assert _guards_hold(buf)
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], want)


# ---- I. gather_mul2 -----------------------------------------------------------------------------------------------------------
@gpu
def test_gather_mul2_strides(dev):
    from pamnet_amd import lib
    torch.manual_seed(3)
    m, d = GM_STRIDE, 128
    ia = torch.randint(0, RA, (m,), dtype=torch.int32, device=dev)
    A, B1, B2 = torch.randn(RA, d, device=dev), torch.randn(m, d, device=dev), torch.randn(m, d, device=dev)
    outs = []
    for _ in range(2):
        (buf1, o1), (buf2, o2) = _guarded(m, d, dev), _guarded(m, d, dev)
        lib.call('pamnet_gather_mul2_f32', lib.ptr(o1), lib.ptr(o2), lib.ptr(A), lib.ptr(ia), lib.ptr(B1), lib.ptr(B2),
                 m, d, lib.stream_of(A))
        assert _guards_hold(buf1) and _guards_hold(buf2)
        outs.append((o1, o2))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][0], A[ia.long()] * B1) and torch.equal(outs[0][1], A[ia.long()] * B2)


# ---- J. segment_sum_multi -----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('njobs', [1, 3, 4])
def test_segment_sum_multi_long_segment(dev, njobs):
    """One segment of 20 000 terms per job (a different row in each) among segments of 0..30; jobs 1 and 3 walk a
    permutation.  Outputs of the jobs beyond njobs are not written."""
    from pamnet_amd import lib
    torch.manual_seed(njobs)
    rows, d = 2286, 128
    jobs = []
    for j in range(4):
        lens = torch.randint(0, 31, (rows,), device=dev)
        lens[(rows // 5) * (j + 1)] = 20000
        csr = _Csr(lens)
        A = _draw('int', csr.m, d, dev)
        perm = torch.randperm(csr.m, dtype=torch.int32, device=dev) if j % 2 else None
        jobs.append((csr, A, perm))
    P = ctypes.c_void_p * 4
    runs = []
    for _ in range(2):
        bufs = [_guarded(rows, d, dev) for _ in range(4)]
        lib.call('pamnet_segment_sum_multi_f32', njobs, P(*[lib.ptr(b[1]) for b in bufs]), P(*[lib.ptr(jb[1]) for jb in jobs]),
                 P(*[None if jb[2] is None else lib.ptr(jb[2]) for jb in jobs]), P(*[lib.ptr(jb[0].ptr) for jb in jobs]),
                 rows, d, lib.stream_of(jobs[0][1]))
        for j, (buf, out) in enumerate(bufs):
            assert _guards_hold(buf) if j < njobs else bool(torch.isnan(buf).all()), j
        runs.append([b[1] for b in bufs[:njobs]])
    for j, (csr, A, perm) in enumerate(jobs[:njobs]):
        src = A.double() if perm is None else A.double()[perm.long()]
        ref = torch.zeros(rows, d, dtype=torch.float64, device=dev).index_add_(0, csr.seg, src).float()
        assert torch.equal(runs[0][j], runs[1][j]), j
        assert torch.equal(runs[0][j], ref), j


# ---- K. the autograd wrappers on the plain kernel -----------------------------------------------------------------------------
_AUTOGRAD = {}


def _autograd_graph(dev):
    """CSR of plain_rows(128) rows whose columns index a table of as many rows: its transpose is that large as well."""
    from pamnet_amd import graph as G
    if not _AUTOGRAD:
        base = _csr(dev, 'big', plain_rows(128))
        torch.manual_seed(11)
        col = torch.randint(0, base.rows, (base.m,), dtype=torch.int32, device=dev)
        _AUTOGRAD['g'] = (base, G.CSR(base.ptr, base.seg.to(torch.int32), col), G.Transpose(col, base.rows))
    return _AUTOGRAD['g']


def _leaf(*shape, dev):
    x = torch.randn(*shape, device=dev)
    return x.clone().requires_grad_(True), x.double().requires_grad_(True)


def _same(pairs):
    for name, got, want in pairs:
        err = maxnorm_err(got.detach().cpu(), want.detach().cpu())
        assert err < 2e-6, (name, err)


@gpu
def test_autograd_aggregate_plain(dev):
    from pamnet_amd import ops
    base, csr, _ = _autograd_graph(dev)
    torch.manual_seed(21)
    d = 128
    (src, src64), (init, init64) = _leaf(base.m, d, dev=dev), _leaf(base.rows, d, dev=dev)
    w = torch.randn(base.rows, d, device=dev)
    y = ops.aggregate(src, csr, init=init)
    (y * w).sum().backward()
    y64 = init64 + torch.zeros_like(init64).index_add(0, base.seg, src64)
    (y64 * w.double()).sum().backward()
    _same([('y', y, y64), ('d src', src.grad, src64.grad), ('d init', init.grad, init64.grad)])


@gpu
def test_autograd_gather_plain(dev):
    from pamnet_amd import ops
    base, csr, tr = _autograd_graph(dev)
    torch.manual_seed(22)
    d = 128
    x, x64 = _leaf(base.rows, d, dev=dev)
    w = torch.randn(base.m, d, device=dev)
    y = ops.gather(x, csr.col, tr.ptr, tr.perm)
    (y * w).sum().backward()
    y64 = x64[csr.col.long()]
    (y64 * w.double()).sum().backward()
    assert torch.equal(y.detach(), x.detach()[csr.col.long()])
    _same([('d x', x.grad, x64.grad)])


@gpu
def test_autograd_gather_mul_aggregate_plain(dev):
    from pamnet_amd import ops
    base, csr, tr = _autograd_graph(dev)
    torch.manual_seed(23)
    d = 128
    (A, A64), (B, B64) = _leaf(base.rows, d, dev=dev), _leaf(base.m, d, dev=dev)
    w = torch.randn(base.rows, d, device=dev)
    y = ops.gather_mul_aggregate(A, B, csr, tr)
    (y * w).sum().backward()
    y64 = torch.zeros(base.rows, d, dtype=torch.float64, device=dev).index_add(0, base.seg, A64[csr.col.long()] * B64)
    (y64 * w.double()).sum().backward()
    _same([('y', y, y64), ('d A', A.grad, A64.grad), ('d B', B.grad, B64.grad)])


# ---- L. contract edges, through lib.call on an explicit stream --------------------------------------------------------------
@gpu
@pytest.mark.parametrize('with_init', [False, True])
@pytest.mark.parametrize('d,rows', [(128, 5), (128, 5000), (12, 5000), (256, plain_rows(256))])
def test_all_segments_empty_without_a_source(dev, d, rows, with_init):
    """Every segment empty and A = NULL: OK, and the rows are zeros (or init) in every launch form."""
    from pamnet_amd import lib
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        ptr = torch.zeros(rows + 1, dtype=torch.int32, device=dev)
        init = _draw('int', rows, d, dev) if with_init else None
        buf, out = _guarded(rows, d, dev)
        lib.call('pamnet_segment_sum_f32', lib.ptr(out), lib.ptr(init), None, None, None, None, None, lib.ptr(ptr), rows, d,
                 stream.cuda_stream)
    stream.synchronize()
    assert _guards_hold(buf)
    assert torch.equal(out, init if with_init else torch.zeros(rows, d, device=dev))


@gpu
def test_unsupported_sizes_are_refused(dev):
    from pamnet_amd import lib
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        m = rows = 8
        x = torch.zeros(m, 128, device=dev)
        o1, o2 = torch.zeros(m, 128, device=dev), torch.zeros(m, 128, device=dev)
        idx = torch.zeros(m, dtype=torch.int32, device=dev)
        ptr = torch.zeros(rows + 1, dtype=torch.int32, device=dev)
        P = ctypes.c_void_p * 5
        arrays = [P(*[lib.ptr(t)] * 5) for t in (o1, x, idx, ptr)]
        st = stream.cuda_stream
        for njobs, d in ((5, 128), (1, 64)):
            with pytest.raises(RuntimeError, match='PAMNET_EINVAL'):
                lib.call('pamnet_segment_sum_multi_f32', njobs, arrays[0], arrays[1], arrays[2], arrays[3], rows, d, st)
        with pytest.raises(RuntimeError, match='PAMNET_EINVAL'):
            lib.call('pamnet_gather_mul2_f32', lib.ptr(o1), lib.ptr(o2), lib.ptr(x), lib.ptr(idx), lib.ptr(x), lib.ptr(x), m, 64, st)
        with pytest.raises(RuntimeError, match='PAMNET_EINVAL'):
            lib.call('pamnet_gather_mul_f32', lib.ptr(o1), lib.ptr(x), lib.ptr(idx), None, None, m, 6, st)
    stream.synchronize()
    assert not bool(o1.any()) and not bool(o2.any())          # nothing was launched


# ---- CPU: the table above is only meaningful while the dispatch constants hold -----------------------------------------------
CPU_TESTS = ('test_dispatch_constants_still_hold', 'test_case_table_reaches_every_form', 'test_gpu_tests_are_marked')


def test_dispatch_constants_still_hold():
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(os.path.dirname(here), 'physics-aware-multiplex-gnn_amd', 'csrc', 'segment.hip')).read()
    text = re.sub(r'\s+', ' ', text)
    for what, needle in (('SPLIT_MAX_LANES', 'SPLIT_MAX_LANES = 256 * 4 * 64 * 4 * 4;'),
                         ('the wide rule', 'SPLIT_WIDE > SPLIT && rows <= 64;'),
                         ('the split rule', 'rows * LPR <= (int64_t)SPLIT_MAX_LANES;'),
                         ('the 256 * 64 grid cap', 'if (grid > 256 * 64) grid = 256 * 64;'),
                         ('the 256 * 32 grid cap', 'if (grid > 256 * 32) grid = 256 * 32;')):
        assert needle in text, ('csrc/segment.hip no longer contains %s (`%s`): the dispatch of pamnet_segment_sum_f32 has '
                                'changed -- re-derive the shape table at the top of tests/test_hip_segment.py (T, plain_rows, '
                                'route, CASES) from the new rule' % (what, needle))
    assert SPLIT_MAX_LANES == 1048576 and [T(d) for d in POW2] == [1048576, 524288, 262144, 131072, 65536, 32768, 16384]
    assert [CAP(d) for d in POW2] == [4 * T(d) for d in POW2]


def test_case_table_reaches_every_form():
    for group, d, rows, form in CASES:
        assert route(d, rows) == form, (group, d, rows, route(d, rows), form)
    for d in POW2:
        forms = set(form for _, dd, _, form in CASES if dd == d)
        want = {'split', 'plain', 'plain-stride'} | ({'wide'} if d < 256 else set())     # d = 256: SPLIT_WIDE == SPLIT
        assert want <= forms, (d, sorted(want - forms))
    assert {'generic', 'generic-stride'} <= set(form for _, _, _, form in CASES)
    for d in POW2:                                             # (the split kernel's largest grid is exactly the cap)
        assert route(d, T(d)) == 'split' and route(d, T(d) + 1) == 'plain'
        assert route(d, CAP(d)) == 'plain' and route(d, CAP(d) + 1) == 'plain-stride'
    assert route(64, 64) == 'wide' and route(64, 65) == 'split'
    assert GM_STRIDE * 32 > GRID_CAP * 256                      # gather_mul / gather_mul2 at d = 128 take a second pass


def test_gpu_tests_are_marked():
    """This file marks its GPU tests one by one: none may be forgotten."""
    for name, fn in sorted(globals().items()):
        if name.startswith('test_') and name not in CPU_TESTS:
            assert any(mk.name == 'gpu' for mk in getattr(fn, 'pytestmark', [])), name
