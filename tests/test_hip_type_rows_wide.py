"""The type-row gradient for tables of 9 .. 128 rows (csrc/type_rows_core.h grad_wide_body / finish_wide_body; entry points
pamnet_type_rows_grad_f32 and the types job of pamnet_embed_multi_fwd/bwd_f32) against fp64 index_add_ on the device.

Row counts: 1 and 127 (one workgroup), 129 (two), 8 197 and 20 000 (all 64 workgroups, the first with a ragged last slice).
Index patterns, each where the kernel can go wrong:
  uniform   every type, most slices hold more than eight: several passes
  last      every row the type T - 1
  cycle     idx[r] = r % T: a slice holds min(T, rows) types, ceil(T / 8) passes
  nine      {0 .. 8}: the second pass holds a single type
  words     {3, 11, 12, 31, 32, 63, 64, T - 1} clipped to T: one pass across the words of the 128-bit set
  sorted    ascending: a workgroup sees one or two types, the finish must skip the workgroups that never saw a type
  stray     uniform with -1 and T mixed in: they contribute nothing
Bound: maxnorm_err < 2e-6, as tests/test_hip_kernels.py::test_type_rows_gather_and_grad for the same sums."""
import ctypes
import math

import pytest
import torch

from conftest import maxnorm_err

pytestmark = pytest.mark.gpu

ROWS = (1, 127, 129, 8197, 20000)
PATTERNS = ('uniform', 'last', 'cycle', 'nine', 'words', 'sorted', 'stray')
SHAPES = [(T, d) for T in (9, 17, 64, 95, 128) for d in (16, 128, 256)] + [(95, 32), (95, 64)]
EINVAL = 'PAMNET_EINVAL'


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs an MI355X'
    from pamnet_amd import lib
    lib.load()
    return torch.device('cuda:0')


def _indices(pattern, n, T, gen):
    r = torch.arange(n)
    if pattern == 'uniform':
        idx = torch.randint(0, T, (n,), generator=gen)
    elif pattern == 'last':
        idx = torch.full((n,), T - 1)
    elif pattern == 'cycle':
        idx = r % T
    elif pattern == 'nine':
        idx = r % 9
    elif pattern == 'words':
        idx = torch.tensor([3, 11, 12, 31, 32, 63, 64, T - 1]).clamp(max=T - 1)[r % 8]
    elif pattern == 'sorted':
        idx = torch.randint(0, T, (n,), generator=gen).sort().values
    else:
        idx = torch.randint(0, T, (n,), generator=gen)
        bad = torch.rand(n, generator=gen)
        idx = torch.where(bad < 0.05, torch.full_like(idx, -1), idx)
        idx = torch.where(bad > 0.95, torch.full_like(idx, T), idx)
        if n == 1:
            idx = torch.tensor([T])
    return idx.to(torch.int32)


def _reference(g, idx, T):
    ok = (idx >= 0) & (idx < T)
    return torch.zeros(T, g.size(1), dtype=torch.float64, device=g.device).index_add_(0, idx[ok].long(), g[ok].double())


def _grad_c(g, idx, T, out=None):
    """pamnet_type_rows_grad_f32 into a NaN-filled table, with the scratch the query asks for filled with NaN bits: the
    kernels may rely on nothing in it."""
    from pamnet_amd import lib
    n, d = g.shape
    need = ctypes.c_int64(0)
    lib.call('pamnet_type_rows_scratch_bytes', T, d, ctypes.addressof(need))
    assert need.value % 16 == 0 and need.value > 0
    scratch = torch.full((need.value // 4,), -1, dtype=torch.int32, device=g.device)        # 0xffffffff: NaNs, full masks
    out = torch.full((T, d), float('nan'), device=g.device) if out is None else out
    lib.call('pamnet_type_rows_grad_f32', lib.ptr(g), lib.ptr(idx), n, T, d, lib.ptr(scratch), lib.ptr(out), lib.stream_of(g))
    return out


@pytest.mark.parametrize('T,d', SHAPES)
def test_wide_gradient_against_fp64(dev, T, d):
    from pamnet_amd import ops
    gen = torch.Generator().manual_seed(1000 * T + d)
    for n in ROWS:
        g = torch.randn(n, d, generator=gen).to(dev)
        for pattern in PATTERNS:
            idx = _indices(pattern, n, T, gen).to(dev)
            ref = _reference(g, idx, T)
            out = _grad_c(g, idx, T)
            where = (T, d, n, pattern)
            assert torch.isfinite(out).all(), where
            err = maxnorm_err(out.cpu(), ref.cpu()) if float(ref.abs().max()) > 0 else float(out.abs().max())
            assert err < 2e-6, (where, err)
            absent = torch.ones(T, dtype=torch.bool, device=dev)
            absent[idx[(idx >= 0) & (idx < T)].long()] = False
            assert float(out[absent].abs().max()) == 0.0 if bool(absent.any()) else True, where     # exact zero rows
            assert bool((out[~absent].abs().amax(1) > 0).all()), where
            assert torch.equal(out, _grad_c(g, idx, T)), where                                         # bitwise repeatable
            if pattern == 'stray':
                continue                               # (the autograd route gathers: its indices must be inside the table)
            table = torch.randn(T, d, generator=gen).to(dev).requires_grad_()
            rows = ops.type_rows(table, idx)
            assert torch.equal(rows, table.detach()[idx.long()]), where
            (rows * g).sum().backward()
            assert torch.equal(table.grad, out), where
            buf = torch.full((T, d), float('nan'), device=dev)                   # direct-gradient mode: all T rows written
            t2 = table.detach().clone().requires_grad_()
            (ops.type_rows(t2, idx, buf) * g).sum().backward()
            assert t2.grad is None and torch.equal(buf, out), where


@pytest.mark.parametrize('d', [128, 16])
@pytest.mark.parametrize('n', [129, 8197])
def test_gradient_does_not_depend_on_the_table_size(dev, n, d):
    """Indices below 8: rows 0 .. 7 of the 95-row gradient are the 8-row kernels' gradient bit for bit (the same slices, slots
    and orders; a slice of up to eight types is one pass of the same loop), the other rows zero."""
    gen = torch.Generator().manual_seed(n + d)
    g = torch.randn(n, d, generator=gen).to(dev)
    for pattern in ('uniform', 'sorted', 'some'):
        idx = torch.randint(0, 8, (n,), generator=gen)
        idx = idx.sort().values if pattern == 'sorted' else (idx.clamp(max=3) * 2 if pattern == 'some' else idx)
        idx = idx.to(torch.int32).to(dev)
        narrow, wide = _grad_c(g, idx, 8), _grad_c(g, idx, 95)
        assert torch.equal(wide[:8], narrow), pattern
        assert float(wide[8:].abs().max()) == 0.0
        assert maxnorm_err(narrow.cpu(), _reference(g, idx, 8).cpu()) < 2e-6


def _stage(dev, table, idx, seed, sizes=(700, 1500, 900)):
    """fused.input_stage with three embedding jobs beside the table: (outs, parameter gradients)."""
    import torch.nn as nn
    from pamnet_amd import fused
    torch.manual_seed(seed)
    e_l, e_g, tp = sizes
    dist_l, dist_g = torch.rand(e_l, device=dev) * 1.9 + 0.05, torch.rand(e_g, device=dev) * 4.9 + 0.05
    sbf = torch.randn(tp, 42, device=dev)
    kind = (torch.rand(tp, device=dev) < 0.4).to(torch.int32)
    freq_l = nn.Parameter((torch.arange(1, 17, device=dev) * math.pi).float())
    freq_g = nn.Parameter((torch.arange(1, 17, device=dev) * math.pi).float())
    lins = [nn.Linear(16, 128).to(dev), nn.Linear(16, 128).to(dev), nn.Linear(42, 128).to(dev), nn.Linear(42, 128).to(dev)]
    layers = [(None, dist_l, 2.0, None, True, True), (None, dist_g, 5.0, None, True, True), (sbf, None, None, kind, True, True)]
    table = table.detach().clone().requires_grad_()
    params = [freq_l, lins[0].weight, lins[0].bias, freq_g, lins[1].weight, lins[1].bias, lins[2].weight, lins[2].bias,
              lins[3].weight, lins[3].bias, table]
    ws = [torch.randn(r, 128, device=dev) for r in (e_l, e_g, tp, idx.numel())]
    outs = fused.input_stage(fused.InputSpec(layers, idx), params)
    sum((o * w).sum() for o, w in zip(outs, ws)).backward()
    return [o.detach() for o in outs], [p.grad for p in params], ws[3]


@pytest.mark.parametrize('n', [129, 2286])
def test_wide_table_in_the_one_launch_input_stage(dev, n):
    from pamnet_amd import ops
    gen = torch.Generator().manual_seed(n)
    t95 = torch.randn(95, 128, generator=gen).to(dev)
    # (a) every row of the table in use
    idx = torch.randint(0, 95, (n,), generator=gen).to(torch.int32).to(dev)
    outs, grads, w = _stage(dev, t95, idx, 5)
    assert torch.equal(outs[3], t95[idx.long()])
    t = t95.clone().requires_grad_()
    (ops.type_rows(t, idx) * w).sum().backward()
    assert torch.equal(grads[-1], t.grad)
    assert maxnorm_err(grads[-1].cpu(), _reference(w, idx, 95).cpu()) < 2e-6
    outs2, grads2, _ = _stage(dev, t95, idx, 5)
    assert all(torch.equal(a, b) for a, b in zip(outs + grads, outs2 + grads2))
    # (b) indices below 8: the other jobs and the eight rows are those of the launch with the 8-row table of the same rows
    idx = torch.randint(0, 8, (n,), generator=gen).to(torch.int32).to(dev)
    wide_o, wide_g, w = _stage(dev, t95, idx, 6)
    narrow_o, narrow_g, _ = _stage(dev, t95[:8].contiguous(), idx, 6)
    assert all(torch.equal(a, b) for a, b in zip(wide_o, narrow_o))
    assert all(torch.equal(a, b) for a, b in zip(wide_g[:-1], narrow_g[:-1]))
    assert torch.equal(wide_g[-1][:8], narrow_g[-1]) and float(wide_g[-1][8:].abs().max()) == 0.0
    t = t95.clone().requires_grad_()
    (ops.type_rows(t, idx) * w).sum().backward()
    assert torch.equal(wide_g[-1], t.grad)


def test_types_job_alone_and_out_of_range_rows(dev):
    """The types job without embedding jobs (the finish then sizes the second launch), indices outside the table: zero rows
    forward, nothing backward."""
    from pamnet_amd import lib, ops
    gen = torch.Generator().manual_seed(4)
    for T, n in ((128, 700), (9, 1), (95, 8197)):
        table = torch.randn(T, 128, generator=gen).to(dev)
        idx = _indices('stray', n, T, gen).to(dev)
        ok = (idx >= 0) & (idx < T)
        out = torch.full((n, 128), float('nan'), device=dev)
        tj = lib.TypeRowsJob(lib.ptr(table), lib.ptr(idx), n, T, lib.ptr(out), None, None, None)
        lib.call('pamnet_embed_multi_fwd_f32', None, 0, ctypes.addressof(tj), lib.stream_of(table))
        want = torch.zeros(n, 128, device=dev)
        want[ok] = table[idx[ok].long()]
        assert torch.equal(out, want)
        g = torch.randn(n, 128, generator=gen).to(dev)
        dtable = torch.full((T, 128), float('nan'), device=dev)
        scratch = ops.reduce_scratch(dev, T, 128)
        tj = lib.TypeRowsJob(None, lib.ptr(idx), n, T, None, lib.ptr(g), lib.ptr(scratch), lib.ptr(dtable))
        lib.call('pamnet_embed_multi_bwd_f32', None, 0, ctypes.addressof(tj), lib.stream_of(table))
        assert torch.equal(dtable, _grad_c(g, idx, T))
        assert maxnorm_err(dtable.cpu(), _reference(g, idx, T).cpu()) < 2e-6 or not bool(ok.any())


def test_c_abi(dev):
    from pamnet_amd import lib, ops
    h = lib.load()
    assert hasattr(h, 'pamnet_type_rows_scratch_bytes') and 'pamnet_type_rows_scratch_bytes' in lib.declared_functions()
    assert int(h.pamnet_abi_version()) == 18
    need, old = ctypes.c_int64(0), ctypes.c_int64(0)
    lib.call('pamnet_reduce_scratch_bytes', ctypes.addressof(old))
    assert old.value == 64 * 8 * 64 * 16
    for T in (1, 5, 8):
        lib.call('pamnet_type_rows_scratch_bytes', T, 128, ctypes.addressof(need))
        assert need.value == old.value
    lib.call('pamnet_type_rows_scratch_bytes', 128, 256, ctypes.addressof(need))
    assert 8 << 20 <= need.value <= (8 << 20) + 4096
    lib.call('pamnet_type_rows_scratch_bytes', 9, 16, ctypes.addressof(need))
    assert need.value >= 64 * 9 * 16 * 4 + 64 * 16
    for T, d in ((0, 128), (129, 128), (95, 260), (95, 6), (95, 512)):
        with pytest.raises(RuntimeError, match=EINVAL):
            lib.call('pamnet_type_rows_scratch_bytes', T, d, ctypes.addressof(need))
    g = torch.randn(10, 128, device=dev)
    g260 = torch.randn(10, 260, device=dev)
    idx = torch.zeros(10, dtype=torch.int32, device=dev)
    scratch = ops.reduce_scratch(dev, 128, 256)
    out = torch.full((129, 260), 7.0, device=dev)
    st = lib.stream_of(g)
    for T, d, src in ((0, 128, g), (129, 128, g), (95, 260, g260)):
        with pytest.raises(RuntimeError, match=EINVAL):
            lib.call('pamnet_type_rows_grad_f32', lib.ptr(src), lib.ptr(idx), 10, T, d, lib.ptr(scratch), lib.ptr(out), st)
    for T in (0, 129):
        tj = lib.TypeRowsJob(lib.ptr(out), lib.ptr(idx), 10, T, lib.ptr(out), None, None, None)
        with pytest.raises(RuntimeError, match=EINVAL):
            lib.call('pamnet_embed_multi_fwd_f32', None, 0, ctypes.addressof(tj), st)
        tj = lib.TypeRowsJob(None, lib.ptr(idx), 10, T, None, lib.ptr(g), lib.ptr(scratch), lib.ptr(out))
        with pytest.raises(RuntimeError, match=EINVAL):
            lib.call('pamnet_embed_multi_bwd_f32', None, 0, ctypes.addressof(tj), st)
    assert float((out - 7.0).abs().max()) == 0.0                              # nothing was launched
    # zero rows: nothing to sum, the table is still written
    for T in (8, 95):
        table = torch.full((T, 128), float('nan'), device=dev)
        lib.call('pamnet_type_rows_grad_f32', None, None, 0, T, 128, lib.ptr(scratch), lib.ptr(table), st)
        assert float(table.abs().max()) == 0.0


def test_scratch_grows_by_need(dev):
    """ops.reduce_scratch: the 512 KB of the 8-row kernels until a wide table asks for more; never smaller than a caller needs."""
    from pamnet_amd import ops
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        a = ops.reduce_scratch(dev, 9, 16)
        assert a.numel() * 4 >= 64 * 9 * 16 * 4 + 1024
        b = ops.reduce_scratch(dev)
        assert b.numel() * 4 >= 64 * 8 * 64 * 16
        c = ops.reduce_scratch(dev, 5, 128)
        assert c is b
        e = ops.reduce_scratch(dev, 128, 256)
        assert e.numel() * 4 >= 8 << 20
        assert ops.reduce_scratch(dev) is e and ops.reduce_scratch(dev, 95, 128) is e
    s.synchronize()
    del ops._SCRATCH[(dev, s.cuda_stream)]
