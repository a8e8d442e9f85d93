"""Kernel-level tests of the node-chain kernels (csrc/node_tail.hip, csrc/node_chain.hip) through the C ABI: the forward chain
(pamnet_node_tail_fwd_f32, _fwd_rider_f32, _fwd_agg_f32), the deferred head branch (pamnet_node_heads_fwd_f32 / _bwd_f32), the
backward chains (pamnet_node_tail_bwd_f32 with head_reduce_kernel, pamnet_node_tail_main_bwd_f32, pamnet_node_pre_tail_bwd_f32,
pamnet_node_pre_tail_bwd_gather_f32) and the head's own backward (pamnet_node_pre_bwd_f32), in every form the host code picks.

Reference everywhere: plain torch fp64 on the kernels' fp32 inputs, the formulas of include/pamnet_hip.h ("Fused dense chains")
and of the header comments of node_chain.hip, written out below (ref_*).  The backward kernels take the saved pre-activations
as an INPUT, so their references are explicit formulas on random Z; test_backward_formulas_match_autograd (CPU, no GPU needed)
validates those formulas against torch autograd on Z produced by the forward reference, to 1e-12.

Tolerance, per output tensor (every Z / dZ slot, every P plane on its own), err = max|a - b| / max|b|:
    err(hip, fp64) <= max(floor, 2 x err(torch fp32 of the same formulas on the same inputs, fp64))
floor 2e-6 for forward outputs, 5e-6 for backward outputs (the floors of test_hip_fused.py::test_node_tail_and_pre).
The bf16x6 forms (packed = 2, nblk | PAMNET_CHAIN_PIECES) were to get 2e-6 on top (what test_hip_fused.py asserts between them and
the fp32-MFMA chains); measured, they stay inside the plain rule by a factor of four, so they get nothing on top (BF16X6_EXTRA = 0).
The head sums (out, att, d b_out: one number per row or per launch) are drawn well conditioned, see HEAD_BIAS below.

Operands are NaN-guarded: every row operand has a NaN row behind its last row, every output starts as NaN between NaN guard rows
that must stay NaN, row-major weights are column blocks of wider NaN tensors (next_wp: ld 384, as the engine passes the [d, 3d]
message weights; 128 otherwise), weight images are packed from those strided slices.  Every form runs twice (same bits),
forwards also without their optional saves (same bits in the required outputs), backwards with the next head in front both in
place (d_x2 is dx1_direct, d_resx is d_add: the engine's call) and with separate buffers (same bits).

Regimes.  fwd_kernel / agg_in_kernel / main_bwd_kernel / pre_tail_bwd_kernel below MIRROR the launch plans of node_tail.hip
(plan_fwd and plan_bwd, with the launches of node_chain_fwd / node_chain_bwd); the tables FWD_TABLE / BWD_TABLE name the kernel every
parametrised row count is meant to reach and are asserted first, with the bound itself (common.h PARKED_TILES_MAX = 256 row
tiles, read from the source; PLAN_BOUNDS of test_hip_model.py): a changed bound makes the tables fail as stale.
    rows <= 4096 (256 tiles)      packed = 1, deferred heads: node_tail_fwd_kernel<true, false> (parked);  backward: node_tail_bwd_kernel
    rows >= 4097 (257 tiles)      ... node_tail_fwd_lean_kernel / node_tail_bwd_lean_kernel; the aggregation and the gathered planes
                                  of the _agg / _gather entry points are then launches of their own
    packed = 2 / PIECES           node_tail_fwd_bf16_kernel<., 8> (4 under PAMNET_CHAIN_WAVES=4) / node_tail_bwd_bf16_kernel, any size
    packed = 0, heads in chain    never lean
The library reads PAMNET_CHAIN_LEAN and PAMNET_CHAIN_WAVES once per process: two tests re-run the cases they change in one
child process each.

Measured on an MI355X, worst (err, torch fp32's err) per entry point and form over all cases, the two child processes included;
the floor of the rule (2e-6 forward, 5e-6 backward) decided every case, 2 x torch's error never exceeded it:
    tail_fwd rowmajor / images, heads in the chain or deferred (parked and lean)  (8.3e-7, 5.2e-7)   bf16x6  (5.1e-7, 5.2e-7)
    tail_fwd_rider images   (4.7e-7, 4.7e-7)     tail_fwd_agg images  (6.5e-7, 4.3e-7)              bf16x6  (4.8e-7, 4.8e-7)
    heads_fwd rowmajor / images  (6.9e-7, 6.9e-7)                      heads_bwd rowmajor / images  (4.8e-7, 4.7e-7)
    tail_bwd rowmajor / images (head_reduce included)  (4.4e-7, 5.3e-7)     pre_bwd rowmajor / images  (7.3e-7, 2.9e-7)
    main_bwd rowmajor / images (parked and lean)  (3.8e-7, 4.4e-7)                                  bf16x6  (3.2e-7, 6.0e-7)
    pre_tail_bwd images (parked and lean)  (3.9e-7, 4.8e-7)                                         bf16x6  (3.3e-7, 4.6e-7)
    pre_tail_bwd_gather images  (3.6e-7, 3.8e-7)                                                    bf16x6  (3.6e-7, 5.8e-7)
(row-major matrices and images gave the same worst figures throughout.)  The whole file: 134 tests, 15 s.

FOUND BY test_gathered_planes (all four cases; with PAMNET_CHAIN_LEAN=0 also by test_gathered_planes_4097): the planes
pamnet_node_pre_tail_bwd_gather_f32 forms inside its launch met fp64 but were not the bits of pamnet_segment_sum_multi_f32 in
rows of more than four entries -- 15 of 37 rows (exactly those of degree 5 and 9), by up to 2.1e-7 of the plane's scale; 1 639 of
4 097 rows in the parked form at 4 097 rows.  The launch adds a row's entries one after the other in CSR order (what
include/pamnet_hip.h states), pamnet_segment_sum_multi_f32 added a row as four contiguous quarters, so a plane depended on the
launch plan that made it.  Fixed in segment.hip: segment_sum_multi_kernel now adds in CSR order as well (one 32-lane group per row,
16 rows of A in flight); the chain kernels are unchanged.  (The other way round -- four lanes in the in-launch gather -- takes
node_tail_bwd_bf16_kernel<true> from 210 to 256 VGPRs with spills.)

Sensitivity, on scratch builds of the library (not committed): (a) node_heads_fwd_kernel reading hb.l[blockIdx.y & 7] fails exactly
the six test_heads_forward cases with 16, 17 and 33 layers (out / att / Z of layer 8 and later stay NaN) and nothing else; (b)
gather_finish advancing gs.q[b] by GU + 1 fails the fp64 check of the gathered planes (err 0.32 / 0.43) in the four
test_gathered_planes cases and in the PAMNET_CHAIN_LEAN=0 child's test_gathered_planes_4097 (which ends that child test), and
nothing else (the default plan's test_gathered_planes_4097 does not gather in the launch and passes).
"""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

D = 128
NAN = float('nan')
IMG32, IMG16 = D * D, 3 * D * D // 2          # floats of an fp32 fragment image / of a bf16x3 one
PIECES = 16                                   # PAMNET_CHAIN_PIECES
MAX_HEAD_LAYERS = 16                          # node_tail.hip
PARKED_TILES_MAX = 256                        # common.h
GU = 4                                        # node_tail.hip: rows in flight per plane and step of the in-launch gather
FWD_FLOOR, BWD_FLOOR = 2e-6, 5e-6
BF16X6_EXTRA = 0.0                            # (on top of the rule for the bf16x6 forms: not needed, see above)
# out[i] = w_out . o3[i] + b_out, att[i] = w_att . o3[i] and d b_out = sum_i d_out[i] are single sums; with n = 1 such an output
# tensor is ONE number, and max|a - b| / max|b| of one cancelling sum measures its conditioning, not the kernel (zero-mean operands:
# |sum| / sum|.| ~ 1 / sqrt(128) on average and arbitrarily small by chance).  The operands of those sums therefore do not cancel:
# the last head bias has mean +1 (o3 = SiLU(z9) mostly positive), the head vectors and d_out have a mean of +-0.5 beside their
# unit spread -- |sum| / sum|.| ~ 0.4 for every row, whatever the seed.
HEAD_BIAS, HEAD_MEAN = 1.0, 0.5
LEAN = int(os.environ.get('PAMNET_CHAIN_LEAN', '2'))
WAVES = 4 if os.environ.get('PAMNET_CHAIN_WAVES', '').strip() == '4' else 8
HERE = os.path.abspath(__file__)
REPO = os.path.dirname(os.path.dirname(HERE))
WORST = {}                                    # entry point and form -> (err, torch fp32's err, bound, tag) nearest to its bound


# ------------------------------------------------------------------------------------------ 1. the host code, restated
def _tiles(n):
    return -(-n // 16)


def fwd_kernel(packed, heads, n, rider=False):
    """node_tail.hip plan_fwd and the launch of node_chain_fwd: the kernel a forward launch gets."""
    if packed == 2:
        return 'node_tail_fwd_bf16_kernel<%s, %d>' % ('true' if rider else 'false', WAVES)
    if rider:
        return 'node_tail_fwd_kernel<true, false, true>'
    if packed and heads:
        return 'node_tail_fwd_kernel<true, true>'
    if packed and _tiles(n) > PARKED_TILES_MAX and LEAN >= 1:
        return 'node_tail_fwd_lean_kernel'
    if packed:
        return 'node_tail_fwd_kernel<true, false>'
    return 'node_tail_fwd_kernel<false, %s>' % ('true' if heads else 'false')


def agg_in_kernel(packed, n, rider=False):
    """node_tail.hip plan_fwd (`agg_in_kernel`, for packed images and deferred heads): does the chain launch form x2 itself?"""
    return packed == 2 or not (_tiles(n) > PARKED_TILES_MAX and LEAN >= 1 and not rider)


def main_bwd_kernel(packed, n):
    """node_tail.hip plan_bwd and the launch of node_chain_bwd, without a head (pamnet_node_tail_main_bwd_f32)."""
    if packed == 2:
        return 'node_tail_bwd_bf16_kernel<false>'
    if packed and _tiles(n) > PARKED_TILES_MAX and LEAN >= 2:
        return 'node_tail_bwd_lean_kernel<false>'
    return 'node_tail_bwd_kernel<%s, false>' % ('true' if packed else 'false')


def pre_tail_bwd_kernel(pieces, n):
    """node_tail.hip plan_bwd and the launch of node_chain_bwd, with a head and no riders (pamnet_node_pre_tail_bwd_f32)."""
    if pieces:
        return 'node_tail_bwd_bf16_kernel<true>'
    if _tiles(n) > PARKED_TILES_MAX and LEAN >= 2:
        return 'node_tail_bwd_lean_kernel<true>'
    return 'node_tail_bwd_kernel<true, false, true>'


FORMS = {'rowmajor+heads': (0, True), 'rowmajor': (0, False), 'images+heads': (1, True), 'images': (1, False),
         'bf16x6': (2, False)}
FWD_ROWS = [1, 15, 16, 17, 37, 4096, 4097]
BWD_ROWS = [1, 16, 17, 37, 4096, 4097]
LEAN_ROWS = (4097,)                           # of the row counts above: more than 256 row tiles
_PARKED, _BWD = 'node_tail_fwd_kernel<true, false>', 'node_tail_bwd_kernel<true, false>'
FWD_TABLE = {(f, n): {'rowmajor+heads': 'node_tail_fwd_kernel<false, true>', 'rowmajor': 'node_tail_fwd_kernel<false, false>',
                      'images+heads': 'node_tail_fwd_kernel<true, true>',
                      'images': 'node_tail_fwd_lean_kernel' if n in LEAN_ROWS and LEAN >= 1 else _PARKED,
                      'bf16x6': 'node_tail_fwd_bf16_kernel<false, %d>' % WAVES}[f] for f in FORMS for n in FWD_ROWS}
BWD_TABLE = {}
for _n in BWD_ROWS:
    _lean = _n in LEAN_ROWS and LEAN >= 2
    BWD_TABLE[('main', 0, _n)] = 'node_tail_bwd_kernel<false, false>'
    BWD_TABLE[('main', 1, _n)] = 'node_tail_bwd_lean_kernel<false>' if _lean else _BWD
    BWD_TABLE[('main', 2, _n)] = 'node_tail_bwd_bf16_kernel<false>'
    BWD_TABLE[('pre', 0, _n)] = 'node_tail_bwd_lean_kernel<true>' if _lean else 'node_tail_bwd_kernel<true, false, true>'
    BWD_TABLE[('pre', 1, _n)] = 'node_tail_bwd_bf16_kernel<true>'
AGG_TABLE = {(1, 37): True, (2, 37): True, (1, 4097): LEAN < 1}        # (packed, rows) -> x2 formed inside the chain launch


def _bounds_current():
    """The bound the tables were written for is the one the sources state."""
    from test_hip_model import PLAN_BOUNDS
    src = open(os.path.join(REPO, 'physics-aware-multiplex-gnn_amd', 'csrc', 'common.h')).read()
    stated = int(re.search(r'PARKED_TILES_MAX\s*=\s*(\d+)', src).group(1))
    assert stated == PARKED_TILES_MAX == PLAN_BOUNDS['lean_from_tiles'] == PLAN_BOUNDS['bf16_tiles'], stated
    assert _tiles(4096) == PARKED_TILES_MAX and _tiles(4097) == PARKED_TILES_MAX + 1


# ------------------------------------------------------------------------------------------ 2. the references
def _silu(z):
    return z * torch.sigmoid(z)


def _dsilu(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def ref_chain_fwd(x2, rx, W, b, w_out, b_out, w_att):
    """node_chain.hip header: the 10-Linear stack and both heads -> (Z[0..9], R[0..1], x_out, out, att)."""
    z = [None] * 10
    z[0] = x2 @ W[0].t() + b[0]
    h0 = _silu(z[0])
    z[1] = h0 @ W[1].t() + b[1]
    z[2] = _silu(z[1]) @ W[2].t() + b[2]
    r1 = _silu(z[2]) + h0 + rx
    z[3] = r1 @ W[3].t() + b[3]
    z[4] = _silu(z[3]) @ W[4].t() + b[4]
    r2 = _silu(z[4]) + r1
    z[5] = r2 @ W[5].t() + b[5]
    z[6] = _silu(z[5]) @ W[6].t() + b[6]
    r3 = _silu(z[6]) + r2
    z[7:], out, att = ref_heads_fwd(r3, W[7:], b[7:], w_out, b_out, w_att)
    return z, [r1, r2], r3, out, att


def ref_heads_fwd(x_out, W, b, w_out, b_out, w_att):
    """o3 = mlp_out(x_out); out = W_out . o3 + b_out; att = W . o3 -> ([z7, z8, z9], out, att)"""
    z7 = x_out @ W[0].t() + b[0]
    z8 = _silu(z7) @ W[1].t() + b[1]
    z9 = _silu(z8) @ W[2].t() + b[2]
    o3 = _silu(z9)
    return [z7, z8, z9], o3 @ w_out + b_out, o3 @ w_att


def ref_pre_fwd(x, Wx1, bx1, wp):
    """The next head: Zx1 = x Wx1^T + bx1, x1 = SiLU(Zx1), P_b = x1 Wp_b^T -> (Zx1, x1, [P_b])"""
    zx1 = x @ Wx1.t() + bx1
    x1 = _silu(zx1)
    return zx1, x1, [x1 @ w.t() for w in wp]


def ref_heads_bwd(d_out, d_att, W, w_out, w_att, Z3):
    """The head branch from d out / d att and z7, z8, z9 -> ([dz7, dz8, dz9], g_head, d w_out, d w_att, d b_out)"""
    o3 = _silu(Z3[2])
    dz9 = (d_out[:, None] * w_out + d_att[:, None] * w_att) * _dsilu(Z3[2])
    dz8 = (dz9 @ W[2]) * _dsilu(Z3[1])
    dz7 = (dz8 @ W[1]) * _dsilu(Z3[0])
    return [dz7, dz8, dz9], dz7 @ W[0], (d_out[:, None] * o3).sum(0), (d_att[:, None] * o3).sum(0), d_out.sum().reshape(1)


def ref_main_bwd(d_xout, g_head, W, Z):
    """Layers 6..0 from d x_out = d_xout (None: 0) + g_head -> ([dz0 .. dz6], d_x2, d_resx)"""
    dr3 = g_head if d_xout is None else d_xout + g_head
    dz = [None] * 7
    dz[6] = dr3 * _dsilu(Z[6])
    dz[5] = (dz[6] @ W[6]) * _dsilu(Z[5])
    dr2 = dz[5] @ W[5] + dr3
    dz[4] = dr2 * _dsilu(Z[4])
    dz[3] = (dz[4] @ W[4]) * _dsilu(Z[3])
    dr1 = dz[3] @ W[3] + dr2
    dz[2] = dr1 * _dsilu(Z[2])
    dz[1] = (dz[2] @ W[2]) * _dsilu(Z[1])
    dh0 = dz[1] @ W[1] + dr1
    dz[0] = dh0 * _dsilu(Z[0])
    return dz, dz[0] @ W[0], dr1


def ref_tail_bwd(d_xout, d_out, d_att, W, w_out, w_att, Z):
    """The whole chain with its heads -> ([dz0 .. dz9], d_x2, d_resx, d w_out, d w_att, d b_out)"""
    dz3, g, dwo, dwa, dbo = ref_heads_bwd(d_out, d_att, W[7:], w_out, w_att, Z[7:])
    dz, dx2, drx = ref_main_bwd(d_xout, g, W, Z)
    return dz + dz3, dx2, drx, dwo, dwa, dbo


def ref_pre_bwd(dP, dx1_direct, d_add, Wx1, wp, Zx1):
    """node_chain.hip: d x1 = sum_b dP_b Wp_b + d x1_direct; dZx1 = d x1 SiLU'(Zx1); d x = dZx1 Wx1 + d_add -> (dZx1, d x)"""
    dx1 = sum(p @ w for p, w in zip(dP, wp))
    if dx1_direct is not None:
        dx1 = dx1 + dx1_direct
    dzx1 = dx1 * _dsilu(Zx1)
    dx = dzx1 @ Wx1
    return dzx1, dx if d_add is None else dx + d_add


def ref_pre_tail_bwd(dP, dx1_direct, d_add, Wx1, wp, Zx1, g_head, W, Z):
    """The head's backward feeding the chain's d x_out -> (dZx1, [dz0 .. dz6], d_x2, d_resx)"""
    dzx1, dx = ref_pre_bwd(dP, dx1_direct, d_add, Wx1, wp, Zx1)
    return (dzx1,) + ref_main_bwd(dx, g_head, W, Z)


def _row_ids(ptr):
    cnt = (ptr[1:] - ptr[:-1]).long()
    return torch.repeat_interleave(torch.arange(cnt.numel(), device=ptr.device), cnt)


def ref_segsum(src, ptr, perm, rows):
    """A CSR segment sum: out[i] = sum over q in [ptr[i], ptr[i + 1]) of src[perm ? perm[q] : q]"""
    m = int(ptr[-1])
    picked = src[perm.long()] if perm is not None else src[:m]
    return torch.zeros(rows, src.shape[1], dtype=src.dtype, device=src.device).index_add_(0, _row_ids(ptr), picked)


def ref_local_agg(m_ji, m_nb, s, q3, t_ptr, t_col, l_ptr, init):
    """pamnet_local_agg_fwd_f32 (header): m_t[e] = m_ji[e] + sum_r m_nb[t_col[r]] s[r];  out[i] = init[i] + sum_e q3[e] m_t[e]"""
    m_t = m_ji.clone().index_add_(0, _row_ids(t_ptr), m_nb[t_col.long()] * s)
    out = torch.zeros(l_ptr.numel() - 1, D, dtype=m_ji.dtype, device=m_ji.device) if init is None else init.clone()
    return m_t, out.index_add_(0, _row_ids(l_ptr), q3 * m_t)


def _cast(a, dt):
    if isinstance(a, (list, tuple)):
        return [_cast(x, dt) for x in a]
    return a.to(dt) if torch.is_tensor(a) and a.is_floating_point() else a


def _flat(r):
    if torch.is_tensor(r):
        return [r]
    out = []
    for x in r:
        out.extend(_flat(x) if isinstance(x, (list, tuple)) else [x])
    return out


def _both(fn, *args):
    """fn on the operands as fp64 and as they are (fp32) -> [(fp64 result, fp32 result), ...], nested lists flattened"""
    return list(zip(_flat(fn(*_cast(args, torch.float64))), _flat(fn(*args))))


def test_backward_formulas_match_autograd():
    """The hand-written backward formulas (ref_heads_bwd, ref_main_bwd, ref_tail_bwd, ref_pre_bwd, ref_pre_tail_bwd) against torch
    autograd through the forward references, in fp64 on the CPU at n = 5, Z as the forward produces it: 1e-12."""
    g = torch.Generator().manual_seed(5)
    n = 5

    def rn(*shape, scale=1.0):
        return scale * torch.randn(*shape, generator=g, dtype=torch.float64)
    W, b = [rn(D, D, scale=0.08) for _ in range(10)], [rn(D, scale=0.1) for _ in range(10)]
    Wx1, bx1, wp = rn(D, D, scale=0.08), rn(D, scale=0.1), [rn(D, D, scale=0.08) for _ in range(4)]
    w_out, b_out, w_att = rn(D).requires_grad_(), rn(1).requires_grad_(), rn(D).requires_grad_()
    x2, rx = rn(n, D, scale=0.5).requires_grad_(), rn(n, D, scale=0.5).requires_grad_()
    d_add, d_out, d_att, dP, dx1 = rn(n, D), rn(n), rn(n), [rn(n, D) for _ in range(4)], rn(n, D)
    Z, _, x_out, out, att = ref_chain_fwd(x2, rx, W, b, w_out, b_out, w_att)
    zx1, x1, P = ref_pre_fwd(x_out, Wx1, bx1, wp)
    loss = (d_add * x_out).sum() + (d_out * out).sum() + (d_att * att).sum() + (dx1 * x1).sum() + sum((a * p).sum()
                                                                                                      for a, p in zip(dP, P))
    want = torch.autograd.grad(loss, Z + [zx1, x2, rx, w_out, w_att, b_out, x_out])
    Zd, zx1d = [z.detach() for z in Z], zx1.detach()

    def close(name, a, c):
        assert a.shape == c.shape, name
        assert float((a - c).abs().max()) <= 1e-12 * float(c.abs().max()), name
    with torch.no_grad():
        dzx1, dx = ref_pre_bwd(dP, dx1, d_add, Wx1, wp, zx1d)
        dz3, g_head, dwo, dwa, dbo = ref_heads_bwd(d_out, d_att, W[7:], w_out, w_att, Zd[7:])
        dz, dx2, drx = ref_main_bwd(dx, g_head, W, Zd)
        for k in range(10):
            close('dz%d' % k, (dz + dz3)[k], want[k])
        close('dZx1', dzx1, want[10])
        close('d_x2', dx2, want[11])
        close('d_resx', drx, want[12])
        close('d_wout', dwo, want[13])
        close('d_watt', dwa, want[14])
        close('d_bout', dbo, want[15])
        close('d x_out', dx + g_head, want[16])
        for a, c in zip(_flat(ref_tail_bwd(dx, d_out, d_att, W, w_out, w_att, Zd)), list(want[:10]) + list(want[11:16])):
            close('tail_bwd', a, c)
        for a, c in zip(_flat(ref_pre_tail_bwd(dP, dx1, d_add, Wx1, wp, zx1d, g_head, W, Zd)), [want[10]] + list(want[:7]) +
                        list(want[11:13])):
            close('pre_tail_bwd', a, c)
        # the nullable operands: zero terms
        zero = torch.zeros(n, D, dtype=torch.float64)
        for a, c in zip(_flat(ref_main_bwd(None, g_head, W, Zd)), _flat(ref_main_bwd(zero, g_head, W, Zd))):
            close('d_xout null', a, c)
        for a, c in zip(ref_pre_bwd(dP[:2], None, None, Wx1, wp[:2], zx1d), ref_pre_bwd(dP[:2] + [zero], zero, zero, Wx1, wp[:3],
                                                                                        zx1d)):
            close('pre_bwd nulls', a, c)


# ------------------------------------------------------------------------------------------ 3. operands
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


def _call(name, *args):
    from pamnet_amd import lib
    lib.call(name, *args)


def _in(values):
    """An input operand (rows of 128 floats, planes of rows, or a vector) with a NaN row (element) behind its last one."""
    tail = D if values.dim() > 1 else 1
    buf = _nan(values.device, values.numel() + tail)
    buf[:values.numel()] = values.reshape(-1)
    return buf[:values.numel()].view(values.shape)


class _Out:
    """An output of `shape`: NaN (or `start`, for in-place operands) between 256 NaN guard floats (two rows) on either side."""
    G = 2 * D

    def __init__(self, dev, *shape, start=None):
        self.numel = 1
        for s in shape:
            self.numel *= s
        self.buf = _nan(dev, self.numel + 2 * self.G)
        self.v = self.buf[self.G:self.G + self.numel].view(shape)
        if start is not None:
            self.v.copy_(start)
        self.p = self.buf.data_ptr() + 4 * self.G

    def guards_intact(self):
        return bool(torch.isnan(self.buf[:self.G]).all()) and bool(torch.isnan(self.buf[self.G + self.numel:]).all())

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
    """A vector of `n` floats (bias, head vector, b_out) as elements 4..4+n of a NaN vector; .b: the clean values."""

    def __init__(self, g, dev, n=D, scale=0.1, mean=0.0):
        self.b, self.buf = mean + scale * torch.randn(n, generator=g, device=dev), _nan(dev, n + 8)
        self.buf[4:4 + n] = self.b
        self.p = self.buf.data_ptr() + 16


def _rn(g, dev, *shape, scale=0.5):
    return scale * torch.randn(*shape, generator=g, device=dev)


def _parr(ps):
    return (ctypes.c_void_p * len(ps))(*ps)


def _pack(dev, ws, transposed, bf16):
    """Fragment images of the slices `ws` as they sit in their wide tensors (pamnet_pack_weights_f32 / _bf16x3) ->
    (addresses, keepalive)"""
    n, stride = len(ws), IMG16 if bf16 else IMG32
    images = _nan(dev, (n + 1) * stride)
    _call('pamnet_pack_weights_bf16x3' if bf16 else 'pamnet_pack_weights_f32', n, _parr([w.p for w in ws]),
          (ctypes.c_int64 * n)(*[w.ld for w in ws]), transposed, images.data_ptr(), _st(dev))
    assert bool(torch.isnan(images[n * stride:]).all()) and not bool(torch.isnan(images[:n * stride]).any())
    return [images.data_ptr() + 4 * i * stride for i in range(n)], images


class _Weights:
    """The matrices of one chain and of the head behind / in front of it: W[0..9] (ld 128), Wx1 (ld 128), wp[0..3] (ld 384),
    as strided slices and as images (made on first use)."""

    def __init__(self, g, dev):
        self.dev = dev
        self.W, self.Wx1, self.wp = [_W(g, dev) for _ in range(10)], _W(g, dev), [_W(g, dev, 3 * D) for _ in range(4)]
        self._img = {}

    def ptrs(self, packed, transposed):
        """-> (W[0..9], Wx1, wp[0..3]) addresses for `packed` (0: the slices, 1: fp32 images, 2: bf16x3 images)"""
        if not packed:
            p = [w.p for w in self.W + [self.Wx1] + self.wp]
        else:
            key = (packed, transposed)
            if key not in self._img:
                self._img[key] = _pack(self.dev, self.W + [self.Wx1] + self.wp, transposed, packed == 2)
            p = self._img[key][0]
        return p[:10], p[10], p[11:15]


# ------------------------------------------------------------------------------------------ 4. the rule
def _check(entry, name, got, ref, tag, floor, extra=0.0):
    """The fp64 rule for one output tensor; ref = (fp64 result, torch's fp32 result)."""
    r64, r32 = ref
    assert got.shape == r64.shape, (entry, name, tag, got.shape, r64.shape)
    assert bool(torch.isfinite(got).all()), (entry, name, tag)
    scale = max(float(r64.abs().max()), 1e-300)
    e = float((got.double() - r64).abs().max()) / scale
    f = float((r32.double() - r64).abs().max()) / scale
    bound = max(floor, 2 * f) + extra
    if entry not in WORST or e / bound > WORST[entry][0] / WORST[entry][2]:
        WORST[entry] = (e, f, bound, '%s %s' % (name, tag))
    assert e <= bound, (entry, name, tag, e, f, bound)


def _check_planes(entry, name, got, refs, tag, floor, extra=0.0):
    """One tensor per plane: got [planes, rows, 128] against refs[plane]."""
    assert got.shape[0] == len(refs), (entry, name, tag)
    for k, r in enumerate(refs):
        _check(entry, '%s[%d]' % (name, k), got[k], r, tag, floor, extra)


def _report(*entries):
    for entry in entries:
        if entry in WORST:
            e, f, bound, tag = WORST[entry]
            print('node-chain %-22s worst (err, floor, bound) so far = (%.2e, %.2e, %.2e) at %s' % (entry, e, f, bound, tag))


def _eq(x, y):
    """The same bits (NaN fill included)."""
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def _same_bits(a, b, names):
    return [k for k in names if not _eq(a[k].v, b[k].v)] == []


# ------------------------------------------------------------------------------------------ 5. the forward chain
class _FwdSet:
    """Operands of a forward chain over n rows with the next head behind it, and their references (shared by the forms)."""

    def __init__(self, dev, n, x2=None):
        g = _gen(dev, 100 + n)
        self.dev, self.n = dev, n
        self.x2, self.rx = _in(_rn(g, dev, n, D) if x2 is None else x2), _in(_rn(g, dev, n, D))
        self.wt = _Weights(g, dev)
        self.b, self.bx1 = [_B(g, dev, mean=HEAD_BIAS if k == 9 else 0.0) for k in range(10)], _B(g, dev)
        self.w_out, self.w_att = _B(g, dev, scale=1.0, mean=HEAD_MEAN), _B(g, dev, scale=1.0, mean=-HEAD_MEAN)
        self.b_out = _B(g, dev, 1, scale=0.5)
        self._ref = {}

    def ref(self, x2=None):
        """-> dict of (fp64, fp32) references; x2: another chain input (a pair (fp64, fp32), for the forms that make it)"""
        if x2 is not None or 'own' not in self._ref:
            def f(x2, rx, W, b, w_out, b_out, w_att, Wx1, bx1, wp):
                Z, R, x_out, out, att = ref_chain_fwd(x2, rx, W, b, w_out, b_out, w_att)
                return Z, R, x_out, out, att, ref_pre_fwd(x_out, Wx1, bx1, wp)
            rest = (self.rx, [w.w for w in self.wt.W], [b.b for b in self.b], self.w_out.b, self.b_out.b[0], self.w_att.b,
                    self.wt.Wx1.w, self.bx1.b, [w.w for w in self.wt.wp])
            if x2 is None:
                r = _both(f, self.x2, *rest)
            else:
                r = list(zip(_flat(f(x2[0], *_cast(rest, torch.float64))), _flat(f(x2[1], *rest))))
            r = dict(Z=r[:10], R=r[10:12], x_out=r[12], out=r[13], att=r[14], Zx1=r[15], x1=r[16], P=r[17:21])
            if x2 is not None:
                return r
            self._ref['own'] = r
        return self._ref['own']


_FWD_SETS = {}


def _fwd_set(dev, n):
    if n not in _FWD_SETS:
        _FWD_SETS[n] = _FwdSet(dev, n)
    return _FWD_SETS[n]


class _Agg(ctypes.Structure):
    """pamnet_local_agg (include/pamnet_hip.h)."""
    _fields_ = [(k, ctypes.c_void_p) for k in ('m_ji', 'm_nb', 's', 'q3', 'init', 't_ptr', 't_col', 'l_ptr', 'm_t')]


def _fwd_run(s, packed, heads, nblk, save=True, entry='pamnet_node_tail_fwd_f32', x2=None, rider=None, agg=None):
    """One forward launch on the operand set -> dict of _Out.  rider: the nine rider arguments; agg: an _Agg."""
    dev, n = s.dev, s.n
    o = dict(Z=_Out(dev, 10, n, D), R=_Out(dev, 2, n, D), x_out=_Out(dev, n, D), out=_Out(dev, n), att=_Out(dev, n),
             Zx1=_Out(dev, n, D), x1=_Out(dev, n, D), P=_Out(dev, 4, n, D))
    W, Wx1, wp = s.wt.ptrs(packed, 0)
    args = [s.x2.data_ptr() if x2 is None else x2, s.rx.data_ptr(), n, _parr(W), _parr([b.p for b in s.b]), s.w_out.p, s.b_out.p,
            s.w_att.p, o['Z'].p if save else None, o['R'].p if save else None, o['x_out'].p]
    if entry == 'pamnet_node_tail_fwd_f32':
        args += [o['out'].p if heads else None, o['att'].p if heads else None]
    if nblk:
        args += [Wx1, s.bx1.p, _parr(wp[:nblk] + [None] * (4 - nblk)), 3 * D, nblk, o['Zx1'].p if save else None, o['x1'].p, o['P'].p]
    else:
        args += [None, None, None, 0, 0, None, None, None]
    if entry != 'pamnet_node_tail_fwd_f32':
        args += rider if rider is not None else [None, 0, 0, 0, None, None, 0]
    args.append(packed)
    if agg is not None:
        args.append(ctypes.addressof(agg))
    _call(entry, *args, _st(dev))
    assert all(v.guards_intact() for v in o.values()), (entry, n, packed, heads, nblk)
    return o


def _fwd_check(entry, s, o, ref, packed, heads, nblk, save, tag):
    """Every output of a forward launch against fp64; what the form does not write stays NaN."""
    extra = BF16X6_EXTRA if packed == 2 else 0.0
    nz = 10 if heads else 7
    if save:
        _check_planes(entry, 'Z', o['Z'].v[:nz], ref['Z'][:nz], tag, FWD_FLOOR, extra)
        assert bool(torch.isnan(o['Z'].v[nz:]).all()), tag
        _check_planes(entry, 'R', o['R'].v, ref['R'], tag, FWD_FLOOR, extra)
    else:
        assert o['Z'].untouched() and o['R'].untouched() and o['Zx1'].untouched(), tag
    _check(entry, 'x_out', o['x_out'].v, ref['x_out'], tag, FWD_FLOOR, extra)
    if heads:
        _check(entry, 'out', o['out'].v, ref['out'], tag, FWD_FLOOR, extra)
        _check(entry, 'att', o['att'].v, ref['att'], tag, FWD_FLOOR, extra)
    else:
        assert o['out'].untouched() and o['att'].untouched(), tag
    if nblk:
        if save:
            _check(entry, 'Zx1', o['Zx1'].v, ref['Zx1'], tag, FWD_FLOOR, extra)
        _check(entry, 'x1', o['x1'].v, ref['x1'], tag, FWD_FLOOR, extra)
        _check_planes(entry, 'P', o['P'].v[:nblk], ref['P'][:nblk], tag, FWD_FLOOR, extra)
        assert bool(torch.isnan(o['P'].v[nblk:]).all()), tag
    else:
        assert o['Zx1'].untouched() and o['x1'].untouched() and o['P'].untouched(), tag


ALL_OUT = ('Z', 'R', 'x_out', 'out', 'att', 'Zx1', 'x1', 'P')
REQUIRED = ('x_out', 'out', 'att', 'x1', 'P')


@pytest.mark.gpu
@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('n', FWD_ROWS)
def test_forward_chain(dev, n, form):
    """pamnet_node_tail_fwd_f32 in the five forms of FORMS, next_nblk 0..4 at 17 and 4 097 rows (2 elsewhere): Z, R, x_out, out /
    att, Zx1, x1 and every plane of P against fp64; twice, and without the saves."""
    packed, heads = FORMS[form]
    _bounds_current()
    assert fwd_kernel(packed, heads, n) == FWD_TABLE[(form, n)], (form, n)
    s, entry = _fwd_set(dev, n), 'tail_fwd ' + form
    for nblk in (range(5) if n in (17, 4097) else (2,)):
        tag = 'rows %d nblk %d' % (n, nblk)
        a, b, c = _fwd_run(s, packed, heads, nblk), _fwd_run(s, packed, heads, nblk), _fwd_run(s, packed, heads, nblk, save=False)
        _fwd_check(entry, s, a, s.ref(), packed, heads, nblk, True, tag)
        _fwd_check(entry, s, c, s.ref(), packed, heads, nblk, False, tag + ' no saves')
        assert _same_bits(a, b, ALL_OUT) and _same_bits(a, c, REQUIRED), tag
    _report(entry)


@pytest.mark.gpu
@pytest.mark.parametrize('packed', [1, 2])
@pytest.mark.parametrize('n', [17, 4097])
def test_forward_entry_points_agree(dev, n, packed):
    """pamnet_node_tail_fwd_f32 with out = att = null and pamnet_node_tail_fwd_rider_f32 with mlp_ntiles = 0 fill the same record
    (node_chain_args.h ChainFwd) and reach the same launch: every output has the same bits.  17 rows: a partial tile in the parked
    plan; 4 097: the first row count of the lean plan."""
    s = _fwd_set(dev, n)
    a = _fwd_run(s, packed, False, 2)
    b = _fwd_run(s, packed, False, 2, entry='pamnet_node_tail_fwd_rider_f32')
    assert not bool(torch.isnan(a['x_out'].v).any()) and not bool(torch.isnan(a['P'].v[:2]).any())
    for k in ('Z', 'R', 'x_out', 'Zx1', 'x1', 'P'):
        assert _eq(a[k].v, b[k].v), (n, packed, k)


# ------------------------------------------------------------------------------------------ 6. riders on the fp32 chain
@pytest.mark.gpu
@pytest.mark.parametrize('tile0,ntiles,wgs', [(0, 7, 3), (3, 4, 9), (6, 1, 1)])
def test_riders_on_the_fp32_chain(dev, tile0, ntiles, wgs):
    """pamnet_node_tail_fwd_rider_f32 with packed = 1 (node_tail_fwd_kernel<true, false, true>): 37 chain rows, an MLP over 100
    rows (7 tiles, the last ragged); (3, 4, 9) has more workgroups than tiles.  Chain outputs against fp64 and the bits of the
    launch without riders; rider rows against fp64 and the bits of pamnet_mlp2_fwd_f32; other rows untouched; z1 / z2 null and
    given."""
    n, rows, entry = 37, 100, 'tail_fwd_rider images'
    assert fwd_kernel(1, False, n, rider=True) == 'node_tail_fwd_kernel<true, false, true>'
    s, g = _fwd_set(dev, n), _gen(dev, 61)
    x, W1, b1, W2, b2 = _in(_rn(g, dev, rows, D)), _W(g, dev), _B(g, dev), _W(g, dev), _B(g, dev)

    def f(x, W1, b1, W2, b2):
        z1 = x @ W1.t() + b1
        z2 = _silu(z1) @ W2.t() + b2
        return z1, z2, _silu(z2)
    ref = _both(f, x, W1.w, b1.b, W2.w, b2.b)
    alone = [_Out(dev, rows, D) for _ in range(3)]
    _call('pamnet_mlp2_fwd_f32', x.data_ptr(), rows, W1.p, b1.p, W2.p, b2.p, *[o.p for o in alone], _st(dev))
    plain = _fwd_run(s, 1, False, 2, entry='pamnet_node_tail_fwd_rider_f32')
    r0, r1 = tile0 * 16, min(rows, (tile0 + ntiles) * 16)
    for given in (True, False):
        mo = [_Out(dev, rows, D) for _ in range(3)]
        rider = [x.data_ptr(), rows, tile0, ntiles, _parr([W1.p, b1.p, W2.p, b2.p]),
                 _parr([mo[0].p if given else None, mo[1].p if given else None, mo[2].p]), wgs]
        tag = 'tiles [%d, %d) on %d workgroups%s' % (tile0, tile0 + ntiles, wgs, '' if given else ' z1 = z2 = null')
        o = _fwd_run(s, 1, False, 2, entry='pamnet_node_tail_fwd_rider_f32', rider=rider)
        _fwd_check(entry, s, o, s.ref(), 1, False, 2, True, tag)
        assert _same_bits(o, plain, ALL_OUT), tag
        for k, name in enumerate(('z1', 'z2', 'y')):
            assert mo[k].guards_intact(), tag
            if k < 2 and not given:
                assert mo[k].untouched(), tag
                continue
            _check(entry, 'rider ' + name, mo[k].v[r0:r1], (ref[k][0][r0:r1], ref[k][1][r0:r1]), tag, FWD_FLOOR)
            assert _eq(mo[k].v[r0:r1], alone[k].v[r0:r1]), (name, tag)
            assert bool(torch.isnan(mo[k].v[:r0]).all()) and bool(torch.isnan(mo[k].v[r1:]).all()), (name, tag)
    _report(entry)


# ------------------------------------------------------------------------------------------ 7. the chain that forms its input
def _csr(dev, counts):
    ptr = torch.zeros(len(counts) + 1, dtype=torch.int64)
    ptr[1:] = torch.tensor(counts, dtype=torch.int64).cumsum(0)
    return ptr.to(torch.int32).to(dev)


class _LocalGraph:
    """A hand-made local graph over n nodes: in-degrees cycle through {0, 1, 2, 3, 5}, triplet rows per edge through the same set
    with another period; node n - 2 (in the last tile of 37 rows) has degree 5, node n - 1 (the very last row) degree 0."""

    def __init__(self, dev, n):
        g = _gen(dev, 71 + n)
        pat = (0, 1, 2, 3, 5)
        deg = [pat[i % 5] for i in range(n)]
        if n > 1:
            deg[n - 2] = 5
        deg[n - 1] = 0
        self.E = sum(deg)
        tdeg = [pat[(3 * e + 1) % 5] for e in range(self.E)]
        self.T = sum(tdeg)
        self.n, self.l_ptr, self.t_ptr = n, _csr(dev, deg), _csr(dev, tdeg)
        self.t_col = torch.randint(0, self.E, (self.T,), generator=g, device=dev).to(torch.int32)
        self.m_ji, self.m_nb, self.q3 = (_in(_rn(g, dev, self.E, D)) for _ in range(3))
        self.s, self.init = _in(_rn(g, dev, self.T, D)), _in(_rn(g, dev, n, D))
        self._ref = {}

    def ref(self, with_init):
        """-> [(m_t fp64, fp32), (x2 fp64, fp32)]"""
        if with_init not in self._ref:
            self._ref[with_init] = _both(ref_local_agg, self.m_ji, self.m_nb, self.s, self.q3, self.t_ptr, self.t_col, self.l_ptr,
                                         self.init if with_init else None)
        return self._ref[with_init]


def _agg_case(dev, n, packed, combos):
    entry = 'tail_fwd_agg ' + ('bf16x6' if packed == 2 else 'images')
    _bounds_current()
    assert agg_in_kernel(packed, n) == AGG_TABLE[(packed, n)], (packed, n)
    assert fwd_kernel(packed, False, n) == FWD_TABLE[('bf16x6' if packed == 2 else 'images', 37 if n == 37 else 4097)]
    s, lg = _fwd_set(dev, n), _LocalGraph(dev, n)
    for with_init, with_mt in combos:
        tag = 'rows %d init %s m_t %s' % (n, 'given' if with_init else 'null', 'given' if with_mt else 'null')
        r_mt, r_x2 = lg.ref(with_init)
        alone_mt, alone_x2 = _Out(dev, lg.E, D), _Out(dev, n, D)
        _call('pamnet_local_agg_fwd_f32', lg.m_ji.data_ptr(), lg.m_nb.data_ptr(), lg.s.data_ptr(), lg.q3.data_ptr(),
              lg.t_ptr.data_ptr(), lg.t_col.data_ptr(), lg.l_ptr.data_ptr(), lg.init.data_ptr() if with_init else None, n, alone_mt.p,
              alone_x2.p, _st(dev))
        runs = []
        for _ in range(2):
            x2, m_t = _Out(dev, n, D), _Out(dev, lg.E, D)
            agg = _Agg(lg.m_ji.data_ptr(), lg.m_nb.data_ptr(), lg.s.data_ptr(), lg.q3.data_ptr(),
                       lg.init.data_ptr() if with_init else None, lg.t_ptr.data_ptr(), lg.t_col.data_ptr(), lg.l_ptr.data_ptr(),
                       m_t.p if with_mt else None)
            o = _fwd_run(s, packed, False, 2, entry='pamnet_node_tail_fwd_agg_f32', x2=x2.p, agg=agg)
            o['x2'], o['m_t'] = x2, m_t
            assert x2.guards_intact() and m_t.guards_intact(), tag
            runs.append(o)
        a = runs[0]
        _check(entry, 'x2', a['x2'].v, r_x2, tag, FWD_FLOOR)
        assert _eq(a['x2'].v, alone_x2.v), tag          # "bit for bit pamnet_local_agg_fwd_f32's rows"
        if with_mt:
            _check(entry, 'm_t', a['m_t'].v, r_mt, tag, FWD_FLOOR)
            assert _eq(a['m_t'].v, alone_mt.v), tag
        else:
            assert a['m_t'].untouched(), tag
        _fwd_check(entry, s, a, s.ref(r_x2), packed, False, 2, True, tag)
        assert _same_bits(a, runs[1], ALL_OUT + ('x2', 'm_t')), tag
    _report(entry)


@pytest.mark.gpu
@pytest.mark.parametrize('packed', [1, 2])
def test_chain_that_forms_its_input(dev, packed):
    """pamnet_node_tail_fwd_agg_f32 at 37 nodes (edges two at a time, triplet rows two at a time, inside the chain launch): x2,
    m_t and the chain's outputs against fp64, x2 / m_t the bits of pamnet_local_agg_fwd_f32; init and m_t null and given."""
    _agg_case(dev, 37, packed, [(True, True), (True, False), (False, True), (False, False)])


@pytest.mark.gpu
def test_chain_that_forms_its_input_4097(dev):
    """The same graph pattern over 4 097 nodes with packed = 1: the lean chain reads its input, the aggregation is a launch of
    its own ahead of it."""
    _agg_case(dev, 4097, 1, [(True, True), (False, False)])


@pytest.mark.gpu
@pytest.mark.parametrize('packed', [1, 2])
def test_chain_that_forms_its_input_without_edges(dev, packed):
    """agg->m_ji = null with init given (a batch without local edges): x2 = init, the chain on it against fp64."""
    n, entry = 37, 'tail_fwd_agg ' + ('bf16x6' if packed == 2 else 'images')
    s, g = _fwd_set(dev, n), _gen(dev, 83)
    init = _in(_rn(g, dev, n, D))
    l_ptr, t_ptr = torch.zeros(n + 1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    x2 = _Out(dev, n, D)
    agg = _Agg(None, None, None, None, init.data_ptr(), t_ptr.data_ptr(), None, l_ptr.data_ptr(), None)
    o = _fwd_run(s, packed, False, 2, entry='pamnet_node_tail_fwd_agg_f32', x2=x2.p, agg=agg)
    assert x2.guards_intact() and _eq(x2.v, init)
    _fwd_check(entry, s, o, s.ref((init.double(), init)), packed, False, 2, True, 'rows 37 no local edges')
    _report(entry)


# ------------------------------------------------------------------------------------------ 8. deferred heads
class _HeadSet:
    """n_layers head branches over n rows, every layer with its own weights (b_out != 0) and inputs."""

    def __init__(self, dev, L, n):
        g = _gen(dev, 300 + 7 * L + n)
        self.dev, self.L, self.n, self.tiles = dev, L, n, _tiles(n)
        self.W = [_W(g, dev) for _ in range(3 * L)]
        self.b = [_B(g, dev, mean=HEAD_BIAS if k % 3 == 2 else 0.0) for k in range(3 * L)]
        self.w_out = [_B(g, dev, scale=1.0, mean=HEAD_MEAN) for _ in range(L)]
        self.w_att = [_B(g, dev, scale=1.0, mean=-HEAD_MEAN) for _ in range(L)]
        self.b_out = [_B(g, dev, 1, scale=0.5) for _ in range(L)]
        self.x_out = [_in(_rn(g, dev, n, D)) for _ in range(L)]
        self.d_out = [_in(HEAD_MEAN + _rn(g, dev, n, scale=1.0)) for _ in range(L)]
        self.d_att = [_in(_rn(g, dev, n, scale=1.0)) for _ in range(L)]
        self.Z = []                                           # backward input: slots 7..9 random, 0..6 NaN (never read)
        for _ in range(L):
            z = _nan(dev, 10, n, D)
            z[7:] = _rn(g, dev, 3, n, D, scale=1.0)
            self.Z.append(_in(z))
        self._img, self._rf, self._rb = {}, {}, {}

    def weights(self, packed, transposed):
        if not packed:
            return [w.p for w in self.W]
        if transposed not in self._img:
            imgs = [_pack(self.dev, self.W[k:k + 96], transposed, False) for k in range(0, 3 * self.L, 96)]
            self._img[transposed] = ([p for i in imgs for p in i[0]], imgs)
        return self._img[transposed][0]

    def ref_fwd(self, l):
        if l not in self._rf:
            self._rf[l] = _both(ref_heads_fwd, self.x_out[l], [w.w for w in self.W[3 * l:3 * l + 3]],
                                [b.b for b in self.b[3 * l:3 * l + 3]], self.w_out[l].b, self.b_out[l].b[0], self.w_att[l].b)
        return self._rf[l]

    def ref_bwd(self, l):
        if l not in self._rb:
            self._rb[l] = _both(ref_heads_bwd, self.d_out[l], self.d_att[l], [w.w for w in self.W[3 * l:3 * l + 3]],
                                self.w_out[l].b, self.w_att[l].b, [self.Z[l][7], self.Z[l][8], self.Z[l][9]])
        return self._rb[l]


_HEAD_SETS = {}
HEAD_CASES = [(1, 37), (6, 37), (16, 37), (17, 37), (33, 37), (6, 1), (6, 16), (6, 4097)]


def _head_set(dev, L, n):
    if (L, n) not in _HEAD_SETS:
        _HEAD_SETS.clear()                                    # (one set at a time: the cases of one shape run back to back)
        _HEAD_SETS[(L, n)] = _HeadSet(dev, L, n)
    return _HEAD_SETS[(L, n)]


@pytest.mark.gpu
@pytest.mark.parametrize('packed', [0, 1])
@pytest.mark.parametrize('L,n', HEAD_CASES)
def test_heads_forward(dev, L, n, packed):
    """pamnet_node_heads_fwd_f32 over 1 .. 33 layers (batches of MAX_HEAD_LAYERS = 16: one, two and three passes of the host
    loop): every layer's out, att and Z[l][7..9] against fp64, Z[l] null for every third layer and Z null altogether."""
    h, entry = _head_set(dev, L, n), 'heads_fwd ' + ('images' if packed else 'rowmajor')
    assert -(-L // MAX_HEAD_LAYERS) == {1: 1, 6: 1, 16: 1, 17: 2, 33: 3}[L]
    saved = [l % 3 != 1 for l in range(L)]

    def run(with_z):
        Z, out, att = [_Out(dev, 10, n, D) for _ in range(L)], [_Out(dev, n) for _ in range(L)], [_Out(dev, n) for _ in range(L)]
        _call('pamnet_node_heads_fwd_f32', L, _parr([x.data_ptr() for x in h.x_out]), _parr(h.weights(packed, 0)),
              _parr([b.p for b in h.b]), _parr([w.p for w in h.w_out]), _parr([b.p for b in h.b_out]),
              _parr([w.p for w in h.w_att]), _parr([z.p if k else None for z, k in zip(Z, saved)]) if with_z else None,
              _parr([o.p for o in out]), _parr([o.p for o in att]), n, packed, _st(dev))
        assert all(o.guards_intact() for o in Z + out + att), (L, n)
        return Z, out, att

    a, b, c = run(True), run(True), run(False)
    for l in range(L):
        tag = 'layer %d of %d rows %d' % (l, L, n)
        r = h.ref_fwd(l)
        if saved[l]:
            _check_planes(entry, 'Z', a[0][l].v[7:], r[:3], tag, FWD_FLOOR)
            assert bool(torch.isnan(a[0][l].v[:7]).all()), tag
        else:
            assert a[0][l].untouched(), tag
        assert c[0][l].untouched(), tag
        _check(entry, 'out', a[1][l].v, r[3], tag, FWD_FLOOR)
        _check(entry, 'att', a[2][l].v, r[4], tag, FWD_FLOOR)
        assert all(_eq(a[k][l].v, b[k][l].v) for k in range(3)), tag
        assert _eq(a[1][l].v, c[1][l].v) and _eq(a[2][l].v, c[2][l].v), tag
    if L > 1:
        assert not torch.equal(a[1][0].v, a[1][1].v)          # distinct weights and inputs per layer
    _report(entry)


@pytest.mark.gpu
@pytest.mark.parametrize('packed', [0, 1])
@pytest.mark.parametrize('L,n', HEAD_CASES)
def test_heads_backward(dev, L, n, packed):
    """pamnet_node_heads_bwd_f32 over 1 .. 33 layers: every layer's dZ3, g_head and head_partial[l] (ceil(n / 16) x 257, summed
    in fp64) against d w_out, d w_att, d b_out."""
    h, entry = _head_set(dev, L, n), 'heads_bwd ' + ('images' if packed else 'rowmajor')

    def run():
        dZ3, gh = [_Out(dev, 3, n, D) for _ in range(L)], [_Out(dev, n, D) for _ in range(L)]
        hp = [_Out(dev, h.tiles, 257) for _ in range(L)]
        _call('pamnet_node_heads_bwd_f32', L, _parr([x.data_ptr() for x in h.d_out]), _parr([x.data_ptr() for x in h.d_att]),
              _parr(h.weights(packed, 1)), _parr([w.p for w in h.w_out]), _parr([w.p for w in h.w_att]),
              _parr([z.data_ptr() for z in h.Z]), _parr([o.p for o in dZ3]), _parr([o.p for o in gh]), _parr([o.p for o in hp]), n,
              packed, _st(dev))
        assert all(o.guards_intact() for o in dZ3 + gh + hp), (L, n)
        return dZ3, gh, hp

    a, b = run(), run()
    for l in range(L):
        tag = 'layer %d of %d rows %d' % (l, L, n)
        r = h.ref_bwd(l)
        _check_planes(entry, 'dZ3', a[0][l].v, r[:3], tag, BWD_FLOOR)
        _check(entry, 'g_head', a[1][l].v, r[3], tag, BWD_FLOOR)
        tot = a[2][l].v.double().sum(0)
        _check(entry, 'sum head_partial: d_wout', tot[:D], r[4], tag, BWD_FLOOR)
        _check(entry, 'sum head_partial: d_watt', tot[D:2 * D], r[5], tag, BWD_FLOOR)
        _check(entry, 'sum head_partial: d_bout', tot[2 * D:], r[6], tag, BWD_FLOOR)
        assert all(_eq(a[k][l].v, b[k][l].v) for k in range(3)), tag
    _report(entry)


# ------------------------------------------------------------------------------------------ 9. the backward chains
class _BwdSet:
    """Operands of a backward chain over n rows (random saved pre-activations: a legal operand), shared by the entry points."""

    def __init__(self, dev, n):
        g = _gen(dev, 500 + n)
        self.dev, self.n, self.tiles = dev, n, _tiles(n)
        self.wt = _Weights(g, dev)
        self.w_out, self.w_att = _B(g, dev, scale=1.0), _B(g, dev, scale=1.0)
        self.Z, self.Zx1 = _in(_rn(g, dev, 10, n, D, scale=1.0)), _in(_rn(g, dev, n, D, scale=1.0))
        self.d_xout, self.g_head, self.dx1, self.d_add = (_in(_rn(g, dev, n, D, scale=1.0)) for _ in range(4))
        self.dP = _in(_rn(g, dev, 4, n, D, scale=1.0))
        self.d_out, self.d_att = _in(HEAD_MEAN + _rn(g, dev, n, scale=1.0)), _in(_rn(g, dev, n, scale=1.0))
        self._ref = {}

    def _w(self):
        return [w.w for w in self.wt.W]

    def ref_main(self, with_dxout):
        key = ('main', with_dxout)
        if key not in self._ref:
            r = _both(ref_main_bwd, self.d_xout if with_dxout else None, self.g_head, self._w(), list(self.Z))
            self._ref[key] = dict(dZ=r[:7], d_x2=r[7], d_resx=r[8])
        return self._ref[key]

    def ref_tail(self, with_dxout):
        key = ('tail', with_dxout)
        if key not in self._ref:
            r = _both(ref_tail_bwd, self.d_xout if with_dxout else None, self.d_out, self.d_att, self._w(), self.w_out.b,
                      self.w_att.b, list(self.Z))
            self._ref[key] = dict(dZ=r[:10], d_x2=r[10], d_resx=r[11], d_wout=r[12], d_watt=r[13], d_bout=r[14])
        return self._ref[key]

    def ref_pre(self, nblk, with_dx1, with_add):
        key = ('pre', nblk, with_dx1, with_add)
        if key not in self._ref:
            r = _both(ref_pre_bwd, list(self.dP[:nblk]), self.dx1 if with_dx1 else None, self.d_add if with_add else None,
                      self.wt.Wx1.w, [w.w for w in self.wt.wp[:nblk]], self.Zx1)
            self._ref[key] = dict(dZx1=r[0], dx=r[1])
        return self._ref[key]

    def ref_pre_tail(self, nblk, dP=None):
        """dP: the planes as a pair (fp64, fp32) when some of them are formed by the launch"""
        key = ('pre_tail', nblk)
        if dP is not None or key not in self._ref:
            rest = (self.dx1, self.d_add, self.wt.Wx1.w, [w.w for w in self.wt.wp[:nblk]], self.Zx1, self.g_head, self._w(),
                    list(self.Z))
            if dP is None:
                r = _both(ref_pre_tail_bwd, list(self.dP[:nblk]), *rest)
            else:
                r = list(zip(_flat(ref_pre_tail_bwd(dP[0], *_cast(rest, torch.float64))), _flat(ref_pre_tail_bwd(dP[1], *rest))))
            r = dict(dZx1=r[0], dZ=r[1:8], d_x2=r[8], d_resx=r[9])
            if dP is not None:
                return r
            self._ref[key] = r
        return self._ref[key]


_BWD_SETS = {}


def _bwd_set(dev, n):
    if n not in _BWD_SETS:
        _BWD_SETS[n] = _BwdSet(dev, n)
    return _BWD_SETS[n]


def _chain_bwd_check(entry, o, ref, nz, tag, extra=0.0):
    """dZ[0 .. nz), d_x2, d_resx (and dZx1) of a backward chain against fp64; the slots the form does not write stay NaN."""
    assert all(v.guards_intact() for v in o.values()), tag
    _check_planes(entry, 'dZ', o['dZ'].v[:nz], ref['dZ'][:nz], tag, BWD_FLOOR, extra)
    assert bool(torch.isnan(o['dZ'].v[nz:]).all()), tag
    for k in ('d_x2', 'd_resx', 'dZx1'):
        if k in ref:
            _check(entry, k, o[k].v, ref[k], tag, BWD_FLOOR, extra)


@pytest.mark.gpu
@pytest.mark.parametrize('packed', [0, 1])
@pytest.mark.parametrize('n', [1, 17, 4097])
def test_tail_backward_with_heads(dev, n, packed):
    """pamnet_node_tail_bwd_f32 (heads inside the chain; never lean): dZ[0..9], d_x2, d_resx against fp64 with d_xout null and
    given; with d_wout / d_watt / d_bout given head_reduce_kernel sums 1, 2 and 257 partial rows over its 16 row slices, with all
    three null head_partial is summed in fp64."""
    s, entry = _bwd_set(dev, n), 'tail_bwd ' + ('images' if packed else 'rowmajor')
    assert s.tiles == {1: 1, 17: 2, 4097: 257}[n]
    W = s.wt.ptrs(packed, 1)[0]
    for with_dxout in (False, True):
        ref = s.ref_tail(with_dxout)
        for reduce in (True, False):
            runs = []
            for _ in range(2):
                o = dict(dZ=_Out(dev, 10, n, D), d_x2=_Out(dev, n, D), d_resx=_Out(dev, n, D), hp=_Out(dev, s.tiles, 257),
                         d_wout=_Out(dev, D), d_watt=_Out(dev, D), d_bout=_Out(dev, 1))
                _call('pamnet_node_tail_bwd_f32', s.d_xout.data_ptr() if with_dxout else None, s.d_out.data_ptr(),
                      s.d_att.data_ptr(), n, _parr(W), s.w_out.p, s.w_att.p, s.Z.data_ptr(), o['dZ'].p, o['d_x2'].p, o['d_resx'].p,
                      o['hp'].p, *[o[k].p if reduce else None for k in ('d_wout', 'd_watt', 'd_bout')], packed, _st(dev))
                runs.append(o)
            a = runs[0]
            tag = 'rows %d d_xout %s%s' % (n, 'given' if with_dxout else 'null', ' + head_reduce' if reduce else '')
            _chain_bwd_check(entry, a, ref, 10, tag)
            tot = a['hp'].v.double().sum(0)
            for k, part in (('d_wout', tot[:D]), ('d_watt', tot[D:2 * D]), ('d_bout', tot[2 * D:])):
                _check(entry, 'sum head_partial: ' + k, part, ref[k], tag, BWD_FLOOR)
                if reduce:
                    _check(entry, 'head_reduce ' + k, a[k].v, ref[k], tag, BWD_FLOOR)
                else:
                    assert a[k].untouched(), tag
            assert _same_bits(a, runs[1], ('dZ', 'd_x2', 'd_resx', 'hp') + (('d_wout', 'd_watt', 'd_bout') if reduce else ())), tag
    _report(entry)


@pytest.mark.gpu
@pytest.mark.parametrize('packed', [0, 1, 2])
@pytest.mark.parametrize('n', BWD_ROWS)
def test_main_backward(dev, n, packed):
    """pamnet_node_tail_main_bwd_f32 on row-major matrices, fp32 images (lean from 4 097 rows) and bf16x3 images: dZ[0..6], d_x2,
    d_resx against fp64 with d_xout null and given; slots 7..9 of dZ are not written."""
    _bounds_current()
    assert main_bwd_kernel(packed, n) == BWD_TABLE[('main', packed, n)], (packed, n)
    s, entry = _bwd_set(dev, n), 'main_bwd ' + ('rowmajor', 'images', 'bf16x6')[packed]
    W = s.wt.ptrs(packed, 1)[0][:7]
    for with_dxout in (False, True):
        runs = []
        for _ in range(2):
            o = dict(dZ=_Out(dev, 10, n, D), d_x2=_Out(dev, n, D), d_resx=_Out(dev, n, D))
            _call('pamnet_node_tail_main_bwd_f32', s.d_xout.data_ptr() if with_dxout else None, s.g_head.data_ptr(), n, _parr(W),
                  s.Z.data_ptr(), o['dZ'].p, o['d_x2'].p, o['d_resx'].p, packed, _st(dev))
            runs.append(o)
        tag = 'rows %d d_xout %s' % (n, 'given' if with_dxout else 'null')
        _chain_bwd_check(entry, runs[0], s.ref_main(with_dxout), 7, tag, BF16X6_EXTRA if packed == 2 else 0.0)
        assert _same_bits(runs[0], runs[1], ('dZ', 'd_x2', 'd_resx')), tag
    _report(entry)


def _pre_tail_run(s, nblk, pieces, in_place, dP_ptr=None, gather=None):
    """One pamnet_node_pre_tail_bwd_f32 (gather: (src, ptr, perm) address lists -> _gather_f32) launch -> dict of _Out"""
    dev, n = s.dev, s.n
    W, Wx1, wp = s.wt.ptrs(2 if pieces else 1, 1)
    o = dict(dZ=_Out(dev, 10, n, D), dZx1=_Out(dev, n, D))
    if in_place:                                              # d_x2 is dx1_direct, d_resx is d_add: the engine's call
        o['d_x2'], o['d_resx'] = _Out(dev, n, D, start=s.dx1), _Out(dev, n, D, start=s.d_add)
        dx1, d_add = o['d_x2'].p, o['d_resx'].p
    else:
        o['d_x2'], o['d_resx'] = _Out(dev, n, D), _Out(dev, n, D)
        dx1, d_add = s.dx1.data_ptr(), s.d_add.data_ptr()
    head = [s.dP.data_ptr() if dP_ptr is None else dP_ptr]
    if gather is not None:
        head += [_parr(g) for g in gather]
    _call('pamnet_node_pre_tail_bwd_gather_f32' if gather is not None else 'pamnet_node_pre_tail_bwd_f32', *head, dx1, d_add, n, Wx1,
          _parr(wp[:nblk]), nblk | (PIECES if pieces else 0), s.Zx1.data_ptr(), o['dZx1'].p, s.g_head.data_ptr(), _parr(W[:7]),
          s.Z.data_ptr(), o['dZ'].p, o['d_x2'].p, o['d_resx'].p, None, _st(dev))
    return o


PRE_TAIL_OUT = ('dZ', 'dZx1', 'd_x2', 'd_resx')


@pytest.mark.gpu
@pytest.mark.parametrize('pieces', [0, 1])
@pytest.mark.parametrize('n', BWD_ROWS)
def test_pre_tail_backward(dev, n, pieces):
    """pamnet_node_pre_tail_bwd_f32 (rider = null) with nblk 1..4 at 17 and 4 097 rows (2 and 4 elsewhere), on fp32 images (lean
    from 4 097 rows) and with PAMNET_CHAIN_PIECES: dZx1, dZ[0..6], d_x2, d_resx against fp64; in place and with separate
    buffers, twice each, the same bits."""
    _bounds_current()
    assert pre_tail_bwd_kernel(pieces, n) == BWD_TABLE[('pre', pieces, n)], (pieces, n)
    s, entry = _bwd_set(dev, n), 'pre_tail_bwd ' + ('bf16x6' if pieces else 'images')
    for nblk in ((1, 2, 3, 4) if n in (17, 4097) else (2, 4)):
        tag = 'rows %d nblk %d' % (n, nblk)
        runs = [_pre_tail_run(s, nblk, pieces, in_place) for in_place in (True, True, False, False)]
        _chain_bwd_check(entry, runs[0], s.ref_pre_tail(nblk), 7, tag, BF16X6_EXTRA if pieces else 0.0)
        for r in runs[1:]:
            assert all(v.guards_intact() for v in r.values()) and _same_bits(runs[0], r, PRE_TAIL_OUT), tag
    _report(entry)


@pytest.mark.gpu
@pytest.mark.parametrize('pieces', [False, True])
@pytest.mark.parametrize('n', [17, 4097])
def test_backward_entry_points_agree(dev, n, pieces):
    """pamnet_node_pre_tail_bwd_f32 and pamnet_node_pre_tail_bwd_gather_f32 with every gather_src[b] null fill the same record
    (node_chain_args.h ChainBwd) and reach the same launch: dZ, dZx1, d_x2 and d_resx have the same bits (nblk = 2)."""
    s = _bwd_set(dev, n)
    a = _pre_tail_run(s, 2, pieces, False)
    b = _pre_tail_run(s, 2, pieces, False, gather=([None, None], [None, None], [None, None]))
    assert all(v.guards_intact() for v in list(a.values()) + list(b.values()))
    assert not bool(torch.isnan(a['d_x2'].v).any()) and not bool(torch.isnan(a['dZ'].v[:7]).any())
    for k in PRE_TAIL_OUT:
        assert _eq(a[k].v, b[k].v), (n, pieces, k)


@pytest.mark.gpu
@pytest.mark.parametrize('packed', [0, 1])
@pytest.mark.parametrize('n', [1, 17, 37])
def test_pre_backward(dev, n, packed):
    """pamnet_node_pre_bwd_f32 on the strided slices (wp: ld 384) and on images, nblk 1..4 at 17 rows (2 and 4 elsewhere), d_add
    and dx1_direct null and given: dZx1 and d x against fp64."""
    s, entry = _bwd_set(dev, n), 'pre_bwd ' + ('images' if packed else 'rowmajor')
    _, Wx1, wp = s.wt.ptrs(packed, 1)
    for nblk in ((1, 2, 3, 4) if n == 17 else (2, 4)):
        for with_dx1, with_add in ((True, True), (False, False), (True, False), (False, True)):
            runs = []
            for _ in range(2):
                o = dict(dZx1=_Out(dev, n, D), dx=_Out(dev, n, D))
                _call('pamnet_node_pre_bwd_f32', s.dP.data_ptr(), s.dx1.data_ptr() if with_dx1 else None,
                      s.d_add.data_ptr() if with_add else None, n, Wx1, _parr(wp[:nblk]), 3 * D, nblk, s.Zx1.data_ptr(), o['dZx1'].p,
                      o['dx'].p, packed, _st(dev))
                assert all(v.guards_intact() for v in o.values()), (n, nblk)
                runs.append(o)
            tag = 'rows %d nblk %d dx1_direct %s d_add %s' % (n, nblk, 'given' if with_dx1 else 'null', 'given' if with_add else 'null')
            ref = s.ref_pre(nblk, with_dx1, with_add)
            _check(entry, 'dZx1', runs[0]['dZx1'].v, ref['dZx1'], tag, BWD_FLOOR)
            _check(entry, 'dx', runs[0]['dx'].v, ref['dx'], tag, BWD_FLOOR)
            assert _same_bits(runs[0], runs[1], ('dZx1', 'dx')), tag
    _report(entry)


# ------------------------------------------------------------------------------------------ 10. planes formed in the launch
class _Plane:
    """The CSR of one gathered plane over n rows: degrees cycle through {0, 1, 4, 5, 9} (the steps of GU = 4) from `phase`, row
    n - 2 (in the last tile of 37 rows) has degree 9, the last row degree 0; with or without a permutation."""

    def __init__(self, g, dev, n, phase, permuted):
        pat = (0, 1, 4, 5, 9)
        assert pat == (0, 1, GU, GU + 1, 2 * GU + 1)
        deg = [pat[(i + phase) % 5] for i in range(n)]
        if n > 1:
            deg[n - 2] = 9
        deg[n - 1] = 0
        self.m = sum(deg)
        self.ptr = _csr(dev, deg)
        self.perm = torch.randperm(self.m, generator=g, device=dev).to(torch.int32) if permuted else None
        self.src = _in(_rn(g, dev, self.m, D, scale=1.0))

    def ref(self, n):
        return _both(ref_segsum, self.src, self.ptr, self.perm, n)[0]


def _gather_case(dev, n, nblk, gathered, pieces):
    _bounds_current()
    assert pre_tail_bwd_kernel(pieces, n) == BWD_TABLE[('pre', pieces, n)], (pieces, n)
    entry = 'pre_tail_bwd_gather ' + ('bf16x6' if pieces else 'images')
    s, g = _bwd_set(dev, n), _gen(dev, 91 + n + nblk)
    planes = {b: _Plane(g, dev, n, 2 * b, permuted) for b, permuted in gathered.items()}
    refs = {b: p.ref(n) for b, p in planes.items()}
    tag = 'rows %d nblk %d' % (n, nblk)
    # the planes as the launch sees them, for the references of everything downstream
    dP = ([refs[b][0] if b in planes else s.dP[b].double() for b in range(nblk)],
          [refs[b][1] if b in planes else s.dP[b] for b in range(nblk)])
    alone = {b: _Out(dev, n, D) for b in planes}
    order = sorted(planes)
    _call('pamnet_segment_sum_multi_f32', len(order), _parr([alone[b].p for b in order]), _parr([planes[b].src.data_ptr() for b in order]),
          _parr([planes[b].perm.data_ptr() if planes[b].perm is not None else None for b in order]),
          _parr([planes[b].ptr.data_ptr() for b in order]), n, D, _st(dev))
    gather = ([planes[b].src.data_ptr() if b in planes else None for b in range(nblk)],
              [planes[b].ptr.data_ptr() if b in planes else None for b in range(nblk)],
              [planes[b].perm.data_ptr() if b in planes and planes[b].perm is not None else None for b in range(nblk)])
    runs = []
    for in_place in (True, True, False):
        buf = _Out(dev, nblk, n, D)
        for b in range(nblk):
            if b not in planes:
                buf.v[b] = s.dP[b]
        o = _pre_tail_run(s, nblk, pieces, in_place, dP_ptr=buf.p, gather=gather)
        o['dP'] = buf
        runs.append(o)
    a = runs[0]
    other_bits = []
    for b in range(nblk):
        if b in planes:
            got, want = a['dP'].v[b], alone[b].v
            _check(entry, 'dP[%d] (gathered)' % b, got, refs[b], tag, BWD_FLOOR)
            short = (planes[b].ptr[1:] - planes[b].ptr[:-1]) <= GU
            assert _eq(got[short], want[short]), (tag, b)         # rows of up to four entries: the same additions
            rows = int((got != want).any(1).sum())
            print('node-chain gathered plane %d, %s: %d of %d rows (%d of them with more than %d entries) differ from the bits of '
                  'pamnet_segment_sum_multi_f32, by at most %.2e of the plane\'s scale'
                  % (b, tag, rows, n, int((~short).sum()), GU, float((got - want).abs().max() / want.abs().max())))
            if not _eq(got, want):
                other_bits.append(b)
        else:
            assert _eq(a['dP'].v[b], s.dP[b]), (tag, b)           # a plane that was read keeps its bits
    _chain_bwd_check(entry, a, s.ref_pre_tail(nblk, dP), 7, tag, BF16X6_EXTRA if pieces else 0.0)
    for r in runs[1:]:
        assert all(v.guards_intact() for v in r.values()) and _same_bits(a, r, PRE_TAIL_OUT + ('dP',)), tag
    _report(entry)
    assert not other_bits, (tag, 'gathered planes that are not the bits of pamnet_segment_sum_multi_f32', other_bits)


@pytest.mark.gpu
@pytest.mark.parametrize('pieces', [0, 1])
@pytest.mark.parametrize('nblk', [4, 1])
def test_gathered_planes(dev, nblk, pieces):
    """pamnet_node_pre_tail_bwd_gather_f32 at 37 rows: nblk = 4 with planes 0 (permuted) and 2 (not) formed in the launch, four
    source rows per step, and planes 1 and 3 read; nblk = 1 with its one plane gathered.  All outputs against fp64, the gathered
    planes written to dP also against the bits of pamnet_segment_sum_multi_f32, the read planes keep their bits."""
    _gather_case(dev, 37, nblk, {0: True, 2: False} if nblk == 4 else {0: True}, pieces)


@pytest.mark.gpu
def test_gathered_planes_4097(dev):
    """The same at 4 097 rows without pieces: the lean chain, which forms the planes with the segment-sum launch first."""
    _gather_case(dev, 4097, 4, {0: True, 2: False}, 0)


# ------------------------------------------------------------------------------------------ 11. argument errors
@pytest.mark.gpu
def test_argument_errors(dev):
    """Bad arguments are refused before any launch (PAMNET_EINVAL / PAMNET_ENULL as RuntimeError); zero rows are a no-op."""
    n = 17
    s, b, st = _fwd_set(dev, n), _bwd_set(dev, n), _st(dev)
    W1, Wx1, wp = s.wt.ptrs(1, 0)
    o = dict(Z=_Out(dev, 10, n, D), R=_Out(dev, 2, n, D), x_out=_Out(dev, n, D), out=_Out(dev, n), att=_Out(dev, n),
             Zx1=_Out(dev, n, D), x1=_Out(dev, n, D), P=_Out(dev, 4, n, D), m=_Out(dev, n, D))
    base = [s.rx.data_ptr(), n, _parr(W1), _parr([x.p for x in s.b]), s.w_out.p, s.b_out.p, s.w_att.p, o['Z'].p, o['R'].p, o['x_out'].p]
    nxt = lambda k: [Wx1, s.bx1.p, _parr(wp), 3 * D, k, o['Zx1'].p, o['x1'].p, o['P'].p]
    heads, deferred = [o['out'].p, o['att'].p], [None, None]
    x2 = s.x2.data_ptr()
    mlp = [s.x2.data_ptr(), n, 0, 1, _parr([W1[0], s.b[0].p, W1[1], s.b[1].p]), _parr([None, None, o['m'].p]), 1]
    no_rider = [None, 0, 0, 0, None, None, 0]
    with pytest.raises(RuntimeError, match='EINVAL'):         # next_nblk = 5
        _call('pamnet_node_tail_fwd_f32', x2, *base, *deferred, *nxt(5), 1, st)
    with pytest.raises(RuntimeError, match='EINVAL'):         # bf16x3 images with the heads in the chain
        _call('pamnet_node_tail_fwd_f32', x2, *base, *heads, *nxt(2), 2, st)
    with pytest.raises(RuntimeError, match='EINVAL'):         # a rider on row-major matrices
        _call('pamnet_node_tail_fwd_rider_f32', x2, *base, *nxt(2), *mlp, 0, st)
    with pytest.raises(RuntimeError, match='EINVAL'):         # a rider without a chain to ride on
        _call('pamnet_node_tail_fwd_rider_f32', x2, base[0], 0, *base[2:], *nxt(2), *mlp, 1, st)
    with pytest.raises(RuntimeError, match='ENULL'):          # agg = null
        _call('pamnet_node_tail_fwd_agg_f32', x2, *base, *nxt(2), *no_rider, 1, None, st)
    # an invalid rider request (row-major matrices) together with an aggregation: refused before the aggregation is launched
    lg, W0 = _LocalGraph(dev, n), s.wt.ptrs(0, 0)[0]
    o['x2'], o['m_t'] = _Out(dev, n, D), _Out(dev, lg.E, D)
    agg = _Agg(lg.m_ji.data_ptr(), lg.m_nb.data_ptr(), lg.s.data_ptr(), lg.q3.data_ptr(), lg.init.data_ptr(), lg.t_ptr.data_ptr(),
               lg.t_col.data_ptr(), lg.l_ptr.data_ptr(), o['m_t'].p)
    with pytest.raises(RuntimeError, match='EINVAL'):
        _call('pamnet_node_tail_fwd_agg_f32', o['x2'].p, base[0], n, _parr(W0), *base[3:], *nxt(2), *mlp, 0, ctypes.addressof(agg), st)
    holed = list(W1)
    holed[4] = None
    with pytest.raises(RuntimeError, match='ENULL'):          # a null entry among the ten weights
        _call('pamnet_node_tail_fwd_f32', x2, base[0], n, _parr(holed), *base[3:], *deferred, *nxt(2), 1, st)
    Wt, Wx1t, wpt = b.wt.ptrs(1, 1)
    bo = dict(dZ=_Out(dev, 10, n, D), dZx1=_Out(dev, n, D), d_x2=_Out(dev, n, D), d_resx=_Out(dev, n, D), dP=_Out(dev, 4, n, D))
    tail = lambda k: [b.dx1.data_ptr(), b.d_add.data_ptr(), n, Wx1t, _parr(wpt), k, b.Zx1.data_ptr(), bo['dZx1'].p,
                      b.g_head.data_ptr(), _parr(Wt[:7]), b.Z.data_ptr(), bo['dZ'].p, bo['d_x2'].p, bo['d_resx'].p, None, st]
    with pytest.raises(RuntimeError, match='ENULL'):          # gather_src = null
        _call('pamnet_node_pre_tail_bwd_gather_f32', bo['dP'].p, None, None, None, *tail(4))
    with pytest.raises(RuntimeError, match='EINVAL'):         # nblk = 0
        _call('pamnet_node_pre_tail_bwd_f32', b.dP.data_ptr(), *tail(0))
    with pytest.raises(RuntimeError, match='EINVAL'):         # ... and with the pieces flag
        _call('pamnet_node_pre_tail_bwd_f32', b.dP.data_ptr(), *tail(PIECES))
    # zero rows: OK, nothing launched, nothing written
    _call('pamnet_node_tail_fwd_f32', x2, base[0], 0, *base[2:], *heads, *nxt(2), 1, st)
    _call('pamnet_node_tail_fwd_rider_f32', x2, base[0], 0, *base[2:], *nxt(2), *no_rider, 1, st)
    t0 = tail(4)
    t0[2] = 0
    _call('pamnet_node_pre_tail_bwd_f32', b.dP.data_ptr(), *t0)
    _call('pamnet_node_tail_main_bwd_f32', None, b.g_head.data_ptr(), 0, _parr(Wt[:7]), b.Z.data_ptr(), bo['dZ'].p, bo['d_x2'].p,
          bo['d_resx'].p, 1, st)
    torch.cuda.synchronize()
    assert all(v.untouched() for v in list(o.values()) + list(bo.values()))


# ------------------------------------------------------------------------------------------ 12. the once-per-process switches
def _child(env, select):
    out = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-s', '-m', 'gpu', HERE, '-k', select],
                         capture_output=True, text=True, env=dict(os.environ, **env), timeout=600, cwd=REPO)
    last = {}
    for line in out.stdout.splitlines():
        if 'node-chain ' in line:
            line = line[line.index('node-chain '):]
            last[line.split(' worst')[0]] = line
    print('\n'.join(last[k] for k in sorted(last)))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-1000:]
    return out.stdout


@pytest.mark.gpu
def test_child_process_four_wave_chain():
    """The forward bf16x6 and aggregation cases of this file again in ONE child process with PAMNET_CHAIN_WAVES=4: the tables
    then name node_tail_fwd_bf16_kernel<., 4> (two 16-channel tiles per wave), asserted in the child."""
    assert WAVES == 8, 'the parent runs the default geometry'
    out = _child({'PAMNET_CHAIN_WAVES': '4'}, '(bf16x6 or forms_its_input) and not child_process')
    assert ' passed' in out and 'no tests ran' not in out


@pytest.mark.gpu
def test_child_process_parked_chains_beyond_256_tiles():
    """The 4 096- and 4 097-row cases again in ONE child process with PAMNET_CHAIN_LEAN=0: the parked kernels with more row tiles
    than CUs (the tables then name them for 4 097 rows, and the chain forms x2 itself there), asserted in the child."""
    assert LEAN == 2, 'the parent runs the default plan'
    out = _child({'PAMNET_CHAIN_LEAN': '0'}, '(4096 or 4097) and not child_process')
    assert ' passed' in out and 'no tests ran' not in out
