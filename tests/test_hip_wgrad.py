"""Kernel-level tests of the weight-gradient launches (csrc/wgrad.hip, csrc/wgrad_core.h) through the C ABI: the split-K slot
kernel at its shape and stride edges, the fixed-order reduction with head vectors, every branch of the deferred launcher, and the
rider slots of the node-chain backward launches (the 8-wave slot body).

Reference everywhere: fp64 torch on the same inputs -- dW = dZ^T A (A -> SiLU(A) for a_mode 1), db = colsum(dZ).  Tolerance:
the rule of test_hip_kernels.py::test_wgrad_batched_vs_fp64, unchanged -- the max-normalised error may not exceed
max(2e-7, 2 x the error of torch's fp32 matmul on the same inputs), db within 2e-6.  Sums of stored partials (head vectors, the
edge kernel's tiles) are held to the worst case of ANY fp32 summation order, n * 2^-24 * sum |x| per element.

Every output buffer starts as NaN with NaN guards around the block the library may write; operands that are column blocks of
wider tensors have NaN in the neighbouring columns and a NaN row behind the last one, so an ignored stride or row bound poisons
the result."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import maxnorm_err

pytestmark = pytest.mark.gpu
D = 128
SLOT = D * D + 2 * D                    # floats per partial tile: the tile and two bias parts
NAN = float('nan')
PIECES = 16                             # PAMNET_CHAIN_PIECES
U32 = 2.0 ** -24                        # unit roundoff of fp32


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


def _block(values, rows, ld, dev):
    """`values` [rows, 128] as the middle column block of a NaN tensor [rows + 1, ld] -> (keepalive, address, view)."""
    c0 = (ld - D) // 2 // 4 * 4                   # 16-byte aligned: float4 loads
    buf = _nan(dev, rows + 1, ld)
    buf[:rows, c0:c0 + D] = values[:rows]
    return buf, buf.data_ptr() + 4 * c0, buf[:rows, c0:c0 + D]


class _Job:
    """Operands of one job and its references.  a_mode 1: half of A is spread over [-100, 100] (exp overflows, SiLU saturates on
    both sides), the rest sits where SiLU bends."""

    def __init__(self, dev, g, rows, mode, ld_dz=D, ld_a=D):
        r1 = max(rows, 1)
        scale = torch.exp2(torch.randint(-2, 3, (r1, 1), generator=g, device=dev).float())
        dz = torch.randn(r1, D, generator=g, device=dev) * scale
        if mode:
            far = (torch.rand(r1, D, generator=g, device=dev) * 2 - 1) * 100
            a = torch.where(torch.rand(r1, D, generator=g, device=dev) < 0.5, far, 2 * torch.randn(r1, D, generator=g, device=dev))
        else:
            a = 1.5 * torch.randn(r1, D, generator=g, device=dev)
        self.rows, self.mode, self.ld_dz, self.ld_a = rows, mode, ld_dz, ld_a
        self.zbuf, self.pz, self.dz = _block(dz, rows, ld_dz, dev)
        self.abuf, self.pa, self.a = _block(a, rows, ld_a, dev)
        self._ref = None

    def ref(self):
        """(dW fp64, db fp64, error of torch's fp32 matmul)"""
        if self._ref is None:
            a64 = self.a.double()
            a64 = a64 * torch.sigmoid(a64) if self.mode else a64
            a32 = torch.nn.functional.silu(self.a) if self.mode else self.a
            w64 = self.dz.double().t() @ a64
            floor = maxnorm_err((self.dz.t() @ a32).cpu(), w64.cpu()) if self.rows else 0.0
            self._ref = (w64, self.dz.double().sum(0), floor)
        return self._ref


class _Out:
    """dW as rows 1..128, columns 128..255 of a NaN [130, 384] tensor (ld_dw = 384); db as elements 4..131 of a NaN vector."""

    def __init__(self, dev, with_db=True):
        self.wide = _nan(dev, D + 2, 3 * D)
        self.pw = self.wide.data_ptr() + 4 * (3 * D + D)
        self.dbuf = _nan(dev, D + 8) if with_db else None
        self.pdb = self.dbuf.data_ptr() + 16 if with_db else None

    @property
    def dW(self):
        return self.wide[1:D + 1, D:2 * D]

    @property
    def db(self):
        return None if self.dbuf is None else self.dbuf[4:4 + D]

    def guards_intact(self):
        m = torch.ones_like(self.wide, dtype=torch.bool)
        m[1:D + 1, D:2 * D] = False
        ok = bool(torch.isnan(self.wide[m]).all())
        if self.dbuf is not None:
            ok = ok and bool(torch.isnan(self.dbuf[:4]).all()) and bool(torch.isnan(self.dbuf[4 + D:]).all())
        return ok

    def same_bits(self, other):
        return torch.equal(self.dW, other.dW) and (self.dbuf is None or other.dbuf is None or torch.equal(self.db, other.db))


def _check(job, out, tag=''):
    """The fp64 rule; returns err / max(floor, 1e-7)."""
    assert out.guards_intact(), tag
    if job.rows == 0:                                            # a job without rows: exact zeros
        assert bool((out.dW == 0).all()) and (out.dbuf is None or bool((out.db == 0).all())), tag
        return 0.0
    w64, b64, floor = job.ref()
    assert bool(torch.isfinite(out.dW).all()), tag
    e = maxnorm_err(out.dW.cpu(), w64.cpu())
    assert e <= max(2e-7, 2 * floor), (tag, job.rows, e, floor)
    if out.dbuf is not None:
        assert maxnorm_err(out.db.cpu(), b64.cpu()) < 2e-6, (tag, job.rows)
    return e / max(floor, 1e-7)


class _Head:
    """Head-vector partials [blocks][257] (d w_out | d w_att | d b_out per chain workgroup) behind a NaN row."""

    def __init__(self, dev, g, blocks):
        self.blocks = blocks
        self.part = _nan(dev, blocks + 1, 257)
        self.part[:blocks] = (torch.randn(blocks + 1, 257, generator=g, device=dev) *
                              torch.exp2(torch.randint(-4, 5, (1, 257), generator=g, device=dev).float()))[:blocks]


class _HeadOut:
    def __init__(self, dev):
        self.buf = _nan(dev, 3, D + 8)                           # rows: d_wout, d_watt, d_bout at elements 4..
        self.p = [self.buf.data_ptr() + 4 * (k * (D + 8) + 4) for k in range(3)]

    def args(self):
        return self.p

    def check(self, head, tag=''):
        b = self.buf
        assert bool(torch.isnan(b[:, :4]).all()) and bool(torch.isnan(b[:2, 4 + D:]).all()) and bool(torch.isnan(b[2, 5:]).all()), tag
        got = torch.cat([b[0, 4:4 + D], b[1, 4:4 + D], b[2, 4:5]]).double()
        x = head.part[:head.blocks].double()
        ref, bound = x.sum(0), head.blocks * U32 * x.abs().sum(0)     # worst case of any fp32 summation order
        assert bool(torch.isfinite(got).all()), tag
        assert bool(((got - ref).abs() <= bound).all()), (tag, head.blocks, float(((got - ref).abs() - bound).max()))
        if head.blocks == 0:
            assert bool((got == 0).all()), tag


def _args(pairs):
    """The ten leading arguments of the batched / deferred / rider-plan entries for [(job, out), ...]."""
    from pamnet_amd.fused import _iarr, _parr
    js = [j for j, _ in pairs]
    os_ = [o for _, o in pairs]
    return [len(pairs), _parr([j.pz for j in js]), _iarr([j.ld_dz for j in js]), _parr([j.pa for j in js]),
            _iarr([j.ld_a for j in js]), _iarr([j.mode for j in js], ctypes.c_int32), _iarr([j.rows for j in js]),
            _parr([o.pw for o in os_]), _iarr([3 * D] * len(pairs)), _parr([o.pdb for o in os_])]


def _scratch(dev, rows):
    """NaN scratch for a batch (pamnet_wgrad_scratch_floats) with a guard slot behind it -> (tensor, floats needed)."""
    from pamnet_amd import lib
    need = ctypes.c_int64(0)
    lib.call('pamnet_wgrad_scratch_floats', len(rows), (ctypes.c_int64 * len(rows))(*rows), ctypes.addressof(need))
    return _nan(dev, int(need.value) + SLOT), int(need.value)


def _st(dev):
    from pamnet_amd import lib
    return lib._raw_stream(dev.index) if lib._raw_stream else lib.stream_of(torch.empty(1, device=dev))


def _batched(dev, pairs, head=None, hout=None):
    from pamnet_amd import lib
    part, need = _scratch(dev, [j.rows for j, _ in pairs])
    tail = [head.part.data_ptr(), head.blocks] + hout.args() if head else [None, 0, None, None, None]
    lib.call('pamnet_wgrad_batched_f32', *_args(pairs), part.data_ptr(), *tail, _st(dev))
    assert bool(torch.isnan(part[need:]).all())                  # nothing behind the scratch the library asked for
    return part


def _ctx():
    from pamnet_amd import lib
    n = ctypes.c_int64(0)
    lib.call('pamnet_wgrad_ctx_bytes', ctypes.addressof(n))
    return (ctypes.c_char * int(n.value))()                      # caller-owned host memory, zeroed


def _deferred(dev, ctx, pairs, heads=(None, None), houts=(None, None)):
    """One pamnet_wgrad_deferred_f32 launch on a scratch buffer of its own -> (scratch, floats needed)."""
    from pamnet_amd import lib
    part, need = _scratch(dev, [j.rows for j, _ in pairs])
    h1, h2 = heads
    blocks = h1.blocks if h1 else (h2.blocks if h2 else 0)
    t1 = [h1.part.data_ptr(), blocks] + houts[0].args() if h1 else [None, blocks, None, None, None]
    t2 = [h2.part.data_ptr()] + houts[1].args() if h2 else [None, None, None, None]
    lib.call('pamnet_wgrad_deferred_f32', *_args(pairs), part.data_ptr(), *t1, *t2, ctypes.addressof(ctx), _st(dev))
    return part, need


def _flush(dev, ctx):
    from pamnet_amd import lib
    lib.call('pamnet_wgrad_flush_f32', ctypes.addressof(ctx), _st(dev))


# ------------------------------------------------------------------------------------------ a. the batched launch
def test_batched_single_job_row_counts(dev):
    """One job per launch: row counts on both sides of the 32-row block and of the 64-row chunk multiple, of the 256-row
    slot, and two above 65 536 rows (the slot count clamps at 256 and every workgroup recomputes its chunk: 320 / 1 216 rows);
    each count with contiguous operands (a_mode 0) and as column blocks of wider tensors (ld_dz 384, ld_a 256, a_mode 1)."""
    worst = 0.0
    for rows in (31, 32, 33, 63, 64, 65, 255, 256, 257, 70001, 300000):
        for strided in (False, True):
            g = _gen(dev, rows + strided)
            job = _Job(dev, g, rows, int(strided), 3 * D if strided else D, 2 * D if strided else D)
            out = _Out(dev)
            _batched(dev, [(job, out)])
            worst = max(worst, _check(job, out, (rows, strided)))
            del job, out
    print('wgrad single jobs: worst error / fp32-matmul error = %.2f' % worst)


BATCHES = {
    # 24 jobs (MAXJ), rows on both sides of every boundary, without rows, with one row
    'limit24': [0, 1, 31, 32, 33, 64, 65, 255, 256, 257, 300, 511, 512, 513, 700, 1000, 1023, 1025, 2286, 2816, 4316, 17, 129, 5000],
    # 200 + 100 + 150 + 62 = 512 slots of 256 rows: the largest batch that keeps the 256-row chunk
    'slots512': [51200, 25345, 38400, 15617],
    # one slot more: the chunk grows to 320 rows (410 slots)
    'slots513': [51200, 25345, 38400, 15617, 1],
    # a job clamped to 256 slots (chunk 1 216) beside 23 small ones planned at 256 rows
    'big_among_small': [300, 40, 1000, 2286, 64, 300000, 1, 700, 33, 512, 2816, 255, 96, 1500, 17, 800, 257, 0, 128, 640, 2000, 5, 333, 1024],
}


def _slots(rows, chunk):
    return sum(min(max(-(-r // chunk), 1), 256) for r in rows)


@pytest.mark.parametrize('name', sorted(BATCHES))
def test_batched_shapes_and_strides(dev, name):
    """pamnet_wgrad_batched_f32 on whole batches: every operand a middle column block of a wider NaN tensor (ld_dz 384, ld_a 256,
    ld_dw 384), db = NULL on alternate jobs, both a_modes, a job without rows -> exact zeros, a second run bit for bit the first."""
    rows = BATCHES[name]
    assert len(rows) <= 24
    if name == 'slots512':
        assert _slots(rows, 256) == 512
    if name == 'slots513':
        assert _slots(rows, 256) == 513 and _slots(rows, 320) <= 512
    g = _gen(dev, len(rows) * 1000 + sum(rows) % 997)
    pairs = [(_Job(dev, g, r, (j // 2) % 2, 3 * D, 2 * D), _Out(dev, with_db=j % 2 == 0)) for j, r in enumerate(rows)]
    _batched(dev, pairs)
    first = [(o.dW.clone(), None if o.dbuf is None else o.db.clone()) for _, o in pairs]
    worst = 0.0
    for k, (job, out) in enumerate(pairs):
        worst = max(worst, _check(job, out, (name, k)))
    _batched(dev, pairs)
    for (w1, b1), (_, o) in zip(first, pairs):
        assert torch.equal(w1, o.dW) and (b1 is None or torch.equal(b1, o.db))
    print('wgrad batch %s: worst error / fp32-matmul error = %.2f' % (name, worst))


# ------------------------------------------------------------------------------------------ b. head vectors
HEAD_BLOCKS = [0, 1, 15, 16, 17, 176, 257]


@pytest.mark.parametrize('blocks', HEAD_BLOCKS)
def test_head_vectors_through_the_batched_launch(dev, blocks):
    """The extra row of the reduction grid: column sums of a chain's head-vector partials [blocks][257] -> d_wout[128],
    d_watt[128], d_bout[1], each within blocks * 2^-24 * sum |x| of the fp64 sum; no blocks: exact zeros."""
    g = _gen(dev, 40 + blocks)
    pairs = [(_Job(dev, g, 40, 0), _Out(dev)), (_Job(dev, g, 300, 1), _Out(dev))]
    head, hout = _Head(dev, g, blocks), _HeadOut(dev)
    _batched(dev, pairs, head, hout)
    hout.check(head)
    for job, out in pairs:
        _check(job, out)


@pytest.mark.parametrize('blocks', HEAD_BLOCKS)
def test_two_head_vectors_through_the_deferred_launch(dev, blocks):
    """Both HeadJob slots of pamnet_wgrad_deferred_f32 (a layer pair's merged batch carries two chains' partials), different
    data, reduced by the flush."""
    g = _gen(dev, 90 + blocks)
    pairs = [(_Job(dev, g, 40, 0), _Out(dev)), (_Job(dev, g, 300, 1), _Out(dev))]
    heads, houts = (_Head(dev, g, blocks), _Head(dev, g, blocks)), (_HeadOut(dev), _HeadOut(dev))
    ctx = _ctx()
    keep = _deferred(dev, ctx, pairs, heads, houts)               # (the scratch lives until its reduction has run)
    _flush(dev, ctx)
    for h, o in zip(heads, houts):
        o.check(h)
    assert blocks == 0 or not torch.equal(houts[0].buf[:, 4], houts[1].buf[:, 4])
    for job, out in pairs:
        _check(job, out)
    # the second slot alone
    houts2 = (None, _HeadOut(dev))
    keep = _deferred(dev, ctx, pairs, (None, heads[1]), houts2)
    _flush(dev, ctx)
    houts2[1].check(heads[1])
    assert torch.equal(houts2[1].buf.view(torch.int32), houts[1].buf.view(torch.int32))      # same order of sums: same bits
    del keep


# ------------------------------------------------------------------------------------------ the node chain that carries riders
class _Chain:
    """pamnet_node_pre_tail_bwd_f32 on random operands (the set-up of test_hip_fused.py::test_backward_chain_on_the_bf16_pipe):
    fp32 fragment images, or bf16x3 images with nblk | PAMNET_CHAIN_PIECES."""

    def __init__(self, dev, n, nblk, pieces, seed=0):
        from pamnet_amd import lib
        from pamnet_amd.fused import _iarr, _parr
        g = _gen(dev, 23 + nblk + n + seed)
        rn = lambda *s: torch.randn(*s, generator=g, device=dev)
        NW = 12
        W = [rn(D, D) * 0.08 for _ in range(NW)]
        images = torch.empty(NW, 3 * D * D // 2 if pieces else D * D, device=dev)
        lib.call('pamnet_pack_weights_bf16x3' if pieces else 'pamnet_pack_weights_f32', NW, _parr(W), _iarr([D] * NW), 1,
                 lib.ptr(images), lib.stream_of(images))
        self.dev, self.n, self.nblk, self.pieces, self.images = dev, n, nblk, pieces, images
        self.Z, self.g_head, self.dP = rn(10, n, D), rn(n, D), rn(4, n, D)[:nblk].contiguous()
        self.dx1, self.dadd, self.zx1 = rn(n, D), rn(n, D), rn(n, D)

    def run(self, rider=None):
        """-> (dZ[:7], d_x2, d_resx, dZx1); rider: a planned _Rider whose slots run as extra workgroups of the launch."""
        from pamnet_amd import lib
        from pamnet_amd.fused import _parr
        n, dev = self.n, self.dev
        img = [self.images[i] for i in range(12)]
        dZ, dzx1 = _nan(dev, 10, n, D), _nan(dev, n, D)
        dx2, drx = self.dx1.clone(), self.dadd.clone()          # in place, as the engine calls it
        lib.call('pamnet_node_pre_tail_bwd_f32', lib.ptr(self.dP), lib.ptr(dx2), lib.ptr(drx), n, lib.ptr(img[7]),
                 _parr(img[8:8 + self.nblk]), self.nblk | (PIECES if self.pieces else 0), lib.ptr(self.zx1), lib.ptr(dzx1),
                 lib.ptr(self.g_head), _parr(img[:7]), lib.ptr(self.Z), lib.ptr(dZ), lib.ptr(dx2), lib.ptr(drx),
                 ctypes.addressof(rider.mem) if rider else None, lib.stream_of(self.Z))
        return dZ[:7], dx2, drx, dzx1


class _Rider:
    """pamnet_wgrad_rider_plan_f32 for [(job, out), ...] into `partial` (an address; default: a NaN buffer of max_slots slots
    and a guard slot of its own)."""

    def __init__(self, dev, pairs, max_slots, partial=None):
        from pamnet_amd import lib
        n = ctypes.c_int64(0)
        lib.call('pamnet_wgrad_rider_bytes', ctypes.addressof(n))
        self.mem = (ctypes.c_char * int(n.value))()
        self.pairs, self.buf = pairs, None
        if partial is None:
            self.buf = _nan(dev, (max_slots + 1) * SLOT)
            partial = self.buf.data_ptr()
        self.partial = partial
        out = ctypes.c_int64(-1)
        lib.call('pamnet_wgrad_rider_plan_f32', *_args(pairs), partial, max_slots, ctypes.addressof(self.mem), ctypes.addressof(out))
        self.slots = int(out.value)
        assert len(pairs) <= self.slots <= max_slots
        # 256 rows per slot: the plan pamnet_wgrad_batched_f32 makes for the same jobs (<= 512 slots), so the same sums in the
        # same order
        self.same_plan_as_batched = self.slots == _slots([j.rows for j, _ in pairs], 256)

    def enqueue(self, ctx):
        from pamnet_amd import lib
        lib.call('pamnet_wgrad_rider_enqueue_f32', ctypes.addressof(ctx), ctypes.addressof(self.mem))

    def check_scratch(self):
        if self.buf is not None:
            used = self.buf[:self.slots * SLOT]
            assert bool(torch.isfinite(used).all()) and bool(torch.isnan(self.buf[self.slots * SLOT:]).all())


def _batched_twin(dev, pairs):
    """The same jobs through pamnet_wgrad_batched_f32 into fresh outputs."""
    twins = [(j, _Out(dev, with_db=o.dbuf is not None)) for j, o in pairs]
    _batched(dev, twins)
    return twins


# ------------------------------------------------------------------------------------------ the edge kernel's partial tiles
class _EdgeTiles:
    """The 2 G partial tiles pamnet_global_edge_agg_bwd_wg_f32 leaves behind (as tests/test_hip_edge_agg.py makes them): slots
    [0, G) shares of dW_e with the bias parts, [G, 2 G) shares of dW_ea.  What wgrad.hip owes them is their sum in slot order;
    the reference is the fp64 sum of the stored tiles, the bound the worst case of any fp32 order (the bias: fp64 in the
    kernel, 2e-6).  The edge kernel's own arithmetic is test_hip_edge_agg.py's subject."""

    def __init__(self, dev):
        from pamnet_amd import lib
        rng = np.random.default_rng(3)
        deg = rng.integers(5, 30, size=700)
        n, m = len(deg), int(deg.sum())
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.int32).to(dev)
        ptr, row_of = t(np.concatenate([[0], np.cumsum(deg)])), t(np.repeat(np.arange(n), deg))
        g = _gen(dev, 13)
        mk = lambda *s: 0.5 * torch.randn(*s, generator=g, device=dev)
        e, z, ea, d_agg = mk(m, D), mk(m, D), mk(m, D), mk(n, D)
        Wm, Wea = mk(D, 3 * D) / 4, mk(D, D) / 4
        need, slots = ctypes.c_int64(0), ctypes.c_int64(0)
        lib.call('pamnet_global_edge_agg_wg_floats', m, ctypes.addressof(need), ctypes.addressof(slots))
        self.G = G = int(slots.value)
        assert 1 <= G <= 256 and need.value >= 2 * G * SLOT
        self.partial = _nan(dev, int(need.value))
        dz, de, dPi = _nan(dev, m, D), _nan(dev, m, D), _nan(dev, n, D)
        lib.call('pamnet_global_edge_agg_bwd_wg_f32', lib.ptr(d_agg), m, n, lib.ptr(ptr), lib.ptr(row_of), None, lib.ptr(z),
                 lib.ptr(ea), lib.ptr(e), Wm.data_ptr() + 8 * D, 3 * D, lib.ptr(Wea), D, lib.ptr(dz), lib.ptr(de), 0,
                 lib.ptr(dPi), lib.ptr(self.partial), lib.stream_of(e))
        P = self.partial[:2 * G * SLOT].view(2, G, SLOT).double()
        assert bool(torch.isfinite(P[0]).all()) and bool(torch.isfinite(P[1, :, :D * D]).all())     # (dW_ea has no bias parts)
        self.ref = [P[0, :, :D * D].sum(0).view(D, D), P[1, :, :D * D].sum(0).view(D, D), P[0, :, D * D:].sum(0).view(2, D).sum(0)]
        self.bound = [G * U32 * P[k, :, :D * D].abs().sum(0).view(D, D) for k in range(2)]
        self.dev = dev
        ctx = _ctx()
        self.alone = self.enqueue(ctx)                          # reduced by a flush of their own: the bits to reproduce
        _flush(dev, ctx)
        self.check(self.alone, bits=False)

    def enqueue(self, ctx):
        """pamnet_wgrad_edge_enqueue_f32 with fresh NaN outputs -> (d mlp_m [128, 384] (e-block written), dW_ea, db)."""
        from pamnet_amd import lib
        dev = self.dev
        outs = (_nan(dev, D, 3 * D), _nan(dev, D + 2, D), _nan(dev, D + 8))
        lib.call('pamnet_wgrad_edge_enqueue_f32', ctypes.addressof(ctx), self.G, outs[0].data_ptr() + 8 * D, 3 * D,
                 outs[2].data_ptr() + 16, outs[1].data_ptr() + 4 * D, D, lib.ptr(self.partial))
        return outs

    def check(self, outs, bits=True, tag=''):
        gm, gea, db = outs
        assert bool(torch.isnan(gm[:, :2 * D]).all()) and bool(torch.isnan(gea[0]).all()) and bool(torch.isnan(gea[-1]).all()), tag
        assert bool(torch.isnan(db[:4]).all()) and bool(torch.isnan(db[4 + D:]).all()), tag
        got = (gm[:, 2 * D:], gea[1:D + 1], db[4:4 + D])
        for k in range(2):
            assert bool(torch.isfinite(got[k]).all()), tag
            assert bool(((got[k].double() - self.ref[k]).abs() <= self.bound[k]).all()), (tag, k)
        assert maxnorm_err(got[2].cpu(), self.ref[2].cpu()) < 2e-6, tag
        if bits:
            for a, b in zip(outs, self.alone):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), tag


@pytest.fixture(scope='module')
def edge_tiles(dev):
    return _EdgeTiles(dev)


@pytest.fixture(scope='module')
def small_chain(dev):
    return _Chain(dev, 37, 2, False)


# ------------------------------------------------------------------------------------------ c. deferred sequences
# steps: ('launch', njobs) | ('rider', njobs) | ('edge',) | ('flush',).  ('edge',) steps marked optional run in the with-edge
# variant only.
OPT_EDGE = ('edge', 'optional')
SCRIPTS = {
    1: [('launch', 5), OPT_EDGE, ('launch', 16), ('flush',)],
    2: [('launch', 20), OPT_EDGE, ('launch', 20), ('flush',)],
    3: [('launch', 6), ('rider', 10), OPT_EDGE, ('launch', 8), ('flush',)],
    4: [('launch', 6), ('rider', 10), OPT_EDGE, ('launch', 17), ('flush',)],
    5: [('launch', 20), ('rider', 10), OPT_EDGE, ('launch', 8), ('flush',)],
    6: [('rider', 10), OPT_EDGE, ('launch', 8), ('flush',)],
    7: [('launch', 6), ('rider', 10), ('edge',), ('flush',)],
    8: [('edge',), ('launch', 8), ('flush',)],
}
CASES = [(s, e) for s in (1, 2, 3, 4, 5, 6) for e in (False, True)] + [(7, True), (8, True)]


@pytest.mark.parametrize('script,with_edge', CASES, ids=['script%d%s' % (s, '-edge' if e else '') for s, e in CASES])
def test_deferred_sequences(dev, edge_tiles, small_chain, script, with_edge):
    """The branches of pamnet_wgrad_deferred_f32's launcher, by what is pending when a step runs (main = an earlier launch's
    batch, rider = slots that ran inside a node-chain launch, edge = the fused edge backward's tiles):

      script  step                      pending                 branch
      1       launch 5 jobs             nothing                 plain wgrad_kernel
              launch 16 jobs            main(5)                 wgrad_fused_wide_kernel
      2       launch 20 jobs            main(20)                wgrad_fused_wide_kernel (wide descriptors: > 16 jobs each)
      3       launch 8 jobs             main(6) + rider(10)     wgrad_fused_kernel, compact descriptors
      4       launch 17 jobs            main(6) + rider(10)     does not fit (> 16 jobs): finish_pending, plain launch
      5       launch 8 jobs             main(20) + rider(10)    does not fit (pending main > 16 jobs): finish_pending, plain
      6       launch 8 jobs             rider(10)               wgrad_fused_kernel without an earlier main batch
      7       flush                     main + rider + edge     pamnet_wgrad_flush_f32: three reductions
      8       launch 8 jobs             edge                    wgrad_fused_kernel with the edge tiles alone
      all     final flush               main(last launch)       pamnet_wgrad_flush_f32

    Scripts 1-6 run with and without edge tiles pending at the last launch (the edge reduction takes the last blocks of the
    fused grids, or a launch of its own in finish_pending).  Every batch has its own row counts (up to 40 000), data, a_modes,
    strides and head vectors; every output of every batch is checked after the final flush against fp64 and, bit for bit,
    against the same jobs through pamnet_wgrad_batched_f32 (same slot plan, same order of sums)."""
    rng = np.random.default_rng(100 * script + with_edge)
    g = _gen(dev, 7000 + 10 * script + with_edge)
    ctx = _ctx()
    done = []                                                    # (kind, pairs, heads, houts, scratch)
    edge_outs = []
    for k, step in enumerate(SCRIPTS[script]):
        if step[0] == 'launch':
            rows = [int(r) for r in rng.integers(1, 3000, size=step[1])]
            rows[0] = (40000, 17001, 9000)[k % 3]
            if step[1] > 2:
                rows[2] = 0
            pairs = [(_Job(dev, g, r, int(rng.integers(0, 2)), *((3 * D, 2 * D) if j % 3 == 0 else (D, D))),
                      _Out(dev, with_db=j % 4 != 3)) for j, r in enumerate(rows)]
            blocks = int(rng.choice([3, 37, 143, 176]))
            heads = (_Head(dev, g, blocks), _Head(dev, g, blocks) if k % 2 == 0 else None)
            houts = (_HeadOut(dev), _HeadOut(dev) if heads[1] else None)
            part, need = _deferred(dev, ctx, pairs, heads, houts)
            done.append(('launch', pairs, heads, houts, (part, need)))
        elif step[0] == 'rider':
            rows = [int(r) for r in rng.integers(1, 1500, size=step[1])]
            rows[0], rows[1] = 2816, 256
            pairs = [(_Job(dev, g, r, j % 2), _Out(dev, with_db=j % 3 != 2)) for j, r in enumerate(rows)]
            rider = _Rider(dev, pairs, 80)
            assert rider.same_plan_as_batched
            small_chain.run(rider)
            rider.enqueue(ctx)
            done.append(('rider', pairs, (), (), rider))
        elif step[0] == 'edge':
            if len(step) > 1 and not with_edge:
                continue
            edge_outs.append(edge_tiles.enqueue(ctx))
        else:
            _flush(dev, ctx)
    worst = 0.0
    for kind, pairs, heads, houts, extra in done:
        for j, (job, out) in enumerate(pairs):
            worst = max(worst, _check(job, out, (script, kind, j)))
        for h, o in zip(heads, houts):
            if h is not None:
                o.check(h, (script, kind))
        if kind == 'launch':
            part, need = extra
            assert bool(torch.isnan(part[need:]).all())
        else:
            extra.check_scratch()
        for (job, out), (_, twin) in zip(pairs, _batched_twin(dev, pairs)):
            assert out.same_bits(twin), (script, kind, job.rows)
    for outs in edge_outs:
        edge_tiles.check(outs, tag=script)
    print('wgrad deferred script %d%s: worst error / fp32-matmul error = %.2f' % (script, ' + edge' if with_edge else '', worst))


# ------------------------------------------------------------------------------------------ d. riders
RIDER_BATCHES = {
    # (rows, max_slots)
    'one': ([2816], 80),                                                         # 11 slots of 256 rows
    'ten_grown': ([0, 1, 255, 256, 257, 2816, 20000, 300, 64, 33], 80),          # 100 slots at 256 rows: the chunk grows to 320
    'sixteen': ([0, 1, 255, 256, 257, 2816, 31, 32, 33, 63, 64, 65, 512, 700, 1000, 129], 80),     # MAXJ_S jobs, 33 slots
}


@pytest.mark.parametrize('batch', sorted(RIDER_BATCHES))
@pytest.mark.parametrize('pieces', [False, True], ids=['fp32', 'bf16x3'])
@pytest.mark.parametrize('nblk', [2, 4])
@pytest.mark.parametrize('n', [37, 2286, 2816])
def test_riders_of_the_backward_chain(dev, n, nblk, pieces, batch):
    """Weight-gradient slots as extra workgroups of pamnet_node_pre_tail_bwd_f32 (grid ceil(n/16) + slots; wgrad_body<8>: eight
    waves, 32x64 wave tiles) in both chain forms: the chain's own outputs are the bits of the launch without riders; after
    pamnet_wgrad_rider_enqueue_f32 and a flush the riders' dW / db meet the fp64 rule, and where the plan has 256 rows per slot
    they are the bits of pamnet_wgrad_batched_f32 (wgrad_body<4>): both bodies stage with the same four waves and feed every
    accumulator the same six piece products per 32-row block in the same order."""
    rows, max_slots = RIDER_BATCHES[batch]
    g = _gen(dev, 500 + n + nblk + len(rows))
    chain = _Chain(dev, n, nblk, pieces)
    pairs = [(_Job(dev, g, r, (j + len(rows)) % 2, *((3 * D, 2 * D) if j % 2 else (D, D))), _Out(dev, with_db=j % 4 != 1))
             for j, r in enumerate(rows)]
    rider = _Rider(dev, pairs, max_slots)
    assert rider.same_plan_as_batched == (batch != 'ten_grown')
    assert rider.slots == (80 if batch == 'ten_grown' else _slots(rows, 256))
    plain, ridden = chain.run(None), chain.run(rider)
    for name, a, b in zip(['dZ', 'd_x2', 'd_resx', 'dZx1'], plain, ridden):
        assert not bool(torch.isnan(a).any()), name
        assert torch.equal(a, b), name
    ctx = _ctx()
    rider.enqueue(ctx)
    _flush(dev, ctx)
    rider.check_scratch()
    worst = 0.0
    for j, (job, out) in enumerate(pairs):
        worst = max(worst, _check(job, out, (batch, j)))
    if rider.same_plan_as_batched:
        for (job, out), (_, twin) in zip(pairs, _batched_twin(dev, pairs)):
            assert out.same_bits(twin), (batch, job.rows)
    print('wgrad riders %s: worst error / fp32-matmul error = %.2f' % (batch, worst))


@pytest.mark.parametrize('how', ['launch', 'flush'])
def test_two_rider_batches_are_reduced_together(dev, how):
    """Two chain launches (one per chain form) each carry a rider batch, the second one's slots right behind the first one's in
    the same scratch buffer: pamnet_wgrad_rider_enqueue_f32 appends it (10 + 12 jobs), and one following deferred launch (the
    compact fused kernel; the rider descriptor is the wide one) or the flush reduces both."""
    g = _gen(dev, 31 + len(how))
    chains = (_Chain(dev, 2286, 4, True), _Chain(dev, 37, 2, False))
    rows = ([700, 256, 33, 2816, 1, 0, 512, 1000, 64, 300], [2286, 2286, 37, 255, 257, 0, 96, 1024, 320, 5, 128, 1500])
    buf = _nan(dev, (80 + 80 + 1) * SLOT)
    batches, behind = [], 0
    ctx = _ctx()
    for chain, rw in zip(chains, rows):
        pairs = [(_Job(dev, g, r, j % 2, *((3 * D, 2 * D) if j % 3 == 1 else (D, D))), _Out(dev, with_db=j % 3 != 0))
                 for j, r in enumerate(rw)]
        rider = _Rider(dev, pairs, 80, partial=buf.data_ptr() + 4 * behind * SLOT)
        assert rider.same_plan_as_batched
        behind += rider.slots
        chain.run(rider)
        rider.enqueue(ctx)
        batches.append(pairs)
    assert bool(torch.isfinite(buf[:behind * SLOT]).all()) and bool(torch.isnan(buf[behind * SLOT:]).all())
    if how == 'launch':
        last = [(_Job(dev, g, r, j % 2), _Out(dev)) for j, r in enumerate([900, 17, 4000, 256, 0, 2286, 31, 640])]
        keep = _deferred(dev, ctx, last)                          # (the scratch lives until its reduction has run)
        batches.append(last)
    _flush(dev, ctx)
    for pairs in batches:
        for j, (job, out) in enumerate(pairs):
            _check(job, out, (how, j))
        for (job, out), (_, twin) in zip(pairs, _batched_twin(dev, pairs)):
            assert out.same_bits(twin), (how, job.rows)
