"""Nudged elastic band: the projection kernel pamnet_neb_force_f32 (csrc/neb.hip) and the driver pamnet_amd/neb.py.

The reference is tests/neb_ref.py neb_force_ref, the rule of include/pamnet_hip.h restated in numpy fp64, together with
tests/relax_ref.py fire_step_ref over the bands.  Inputs are made once on the CPU with fixed seeds and never modified.  Every
branch of the projection is decided by comparisons of fp32 energies widened to fp64 (exact in kernel and reference alike) or by
sums that are exactly zero in both, so the kernel batches need no margins.

Tolerances: KTOL = 1e-6 max-normalised per graph on dneb; 1e-12 relative on seg; 1e-12 of sqrt(sum |F|^2) on fpar; equality for
zeros, NaN placement and untouched rows."""
import copy
import warnings

import numpy as np
import pytest
import torch

from conftest import maxnorm_err
from neb_ref import band_of_graphs, climbing_image, neb_force_ref
from relax_ref import STATE, fire_step_ref

ENTRY = 'pamnet_neb_force_f32'
KTOL = 1e-6
DEFAULTS = dict(dt_max=1.0, max_step=0.2, n_min=5, f_inc=1.1, f_dec=0.5, a0=0.1, f_a=0.99)
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1025, 0]
LENGTHS = (3, 4, 9)
BAND_ROLES = ['climb', 'climb_off', 'status', 'nan_energy', 'inf_grad', 'all_fixed', 'identical', 'climb', 'climb_off', 'climb']
SHIFTS = (0, 3, 7)                                # the band of SIZES[i] atoms plays BAND_ROLES[(i + shift) % 10] at LENGTHS[(i + shift) % 3]
# energies along a band: 9 images hold rising, a maximum with E+ > E-, falling, E+ == E0, E- == E0, a maximum with E+ < E- that ties
# with the first one (the climbing image is the lower index), and a minimum
PROFILES = {3: [1.0, 2.0, 0.0], 4: [0.0, 1.0, 2.0, 0.5], 9: [0.0, 1.0, 2.5, 1.5, 0.5, 0.5, 2.5, 0.25, 1.2], 2: [0.5, 0.25], 1: [0.75]}
SENTINEL, SENTINEL64 = np.float32(123.25), -7.0
MODELS = [(32, 2), (128, 1)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs an MI355X'
    from pamnet_amd import lib
    lib.load()
    return torch.device('cuda:0')


class Case(object):
    pass


_MADE = {}


# ------------------------------------------------------------------------------------------------- kernel-test inputs
def _piece(rng, b, counts, role, shift):
    """One band: images of `counts` atoms.  Images of 63 atoms or more have a fifth of their atoms fixed (the same offsets in
    every image), and those rows hold NaN in pos and dE."""
    L, m = len(counts), counts[0]
    p = Case()
    p.counts, p.role = list(counts), role
    p.energy = (0.25 * b + 2.0 ** (b % 3) * np.asarray(PROFILES[L])).astype(np.float32)
    fix = np.zeros(m, dtype=bool)
    if role == 'all_fixed':
        fix[:] = True
    elif m >= 63:
        fix[rng.choice(m, m // 5, replace=False)] = True
    base, step = rng.uniform(-4.0, 4.0, (max(counts), 3)), 0.2 * rng.standard_normal((max(counts), 3))
    pos, dE, fixed = [], [], []
    for j, mj in enumerate(counts):
        r = base[:mj] + j * step[:mj] + 0.05 * rng.standard_normal((mj, 3))
        if role == 'identical' and j in (1, 2):
            r = pos[0].astype(np.float64).copy()
        g = rng.standard_normal((mj, 3))
        fj = fix[:mj] if role != 'mismatch' else np.zeros(mj, dtype=bool)
        r[fj], g[fj] = np.nan, np.nan
        pos.append(r.astype(np.float32)), dE.append(g.astype(np.float32)), fixed.append(fj)
    if role == 'nan_energy':
        p.energy[1] = np.nan
    if role == 'inf_grad' and m:
        a_free = int(np.nonzero(~fix)[0][m // 2 if m > 2 else 0])
        dE[1][a_free, 1] = (np.inf, -np.inf, np.nan)[SHIFTS.index(shift)]
    p.pos, p.dE, p.fixed = pos, dE, fixed
    p.k = float(rng.uniform(0.05, 2.0))
    p.status = 0 if role != 'status' else (2 if shift else 1)
    p.climb = role != 'climb_off'
    return p


def _assemble(pieces):
    """The batch of the bands `pieces`, in that order."""
    c = Case()
    c.pieces = pieces
    counts = [m for p in pieces for m in p.counts]
    c.gptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    c.band_ptr = np.concatenate([[0], np.cumsum([len(p.counts) for p in pieces])]).astype(np.int32)
    cat = lambda name, dtype, shape: (np.concatenate([a for p in pieces for a in getattr(p, name)]).astype(dtype)
                                      if pieces else np.zeros(shape, dtype))
    c.pos, c.dE, c.fixed = cat('pos', np.float32, (0, 3)), cat('dE', np.float32, (0, 3)), cat('fixed', bool, (0,))
    c.energy = np.concatenate([p.energy for p in pieces]).astype(np.float32)
    c.k = np.asarray([p.k for p in pieces], dtype=np.float64)
    c.status = np.asarray([p.status for p in pieces], dtype=np.int32)
    c.climb = np.asarray([p.climb for p in pieces], dtype=bool)
    c.band_of = band_of_graphs(c.band_ptr, len(counts))
    return c


def _kernel_case(shift):
    if shift in _MADE:
        return _MADE[shift]
    rng = np.random.RandomState(200 + shift)
    spec = [([s] * LENGTHS[(i + shift) % 3], BAND_ROLES[(i + shift) % 10]) for i, s in enumerate(SIZES)]
    spec.insert(4, ([7, 7], 'two'))
    spec.insert(8, ([3], 'one'))
    spec += [([5, 5, 6, 6], 'mismatch'), ([4, 4, 5], 'mismatch')]
    c = _assemble([_piece(rng, b, counts, role, shift) for b, (counts, role) in enumerate(spec)])
    n, G = c.pos.shape[0], len(c.gptr) - 1
    c.start = (np.full((n, 3), SENTINEL, np.float32), np.full(G, SENTINEL64), np.full(G, SENTINEL64))
    c.diag = {}
    c.ref = neb_force_ref(c.pos, c.dE, c.energy, c.gptr, c.band_ptr, c.k, c.fixed, c.status, c.climb, out=c.start, diag=c.diag)
    _MADE[shift] = c
    return c


def _assert_projection(got, want, c, diag, start, tag=''):
    """got / want / start: (dneb, seg, fpar); the checks of one launch against neb_force_ref.  Returns the worst errors."""
    (gd, gs, gf), (wd, ws, wf), (sd, ss, sf) = got, want, start
    worst = [0.0, 0.0, 0.0]
    for g in range(len(c.gptr) - 1):
        s = slice(int(c.gptr[g]), int(c.gptr[g + 1]))
        d = diag.get(g)
        if d is None:                             # a band that is not running: nothing of it was written
            assert np.array_equal(gd[s].view(np.int32), sd[s].view(np.int32)), (tag, g, 'untouched rows')
            assert gs[g] == ss[g] and gf[g] == sf[g], (tag, g)
            continue
        assert np.array_equal(np.isnan(gs[g]), np.isnan(ws[g])) and np.array_equal(np.isnan(gf[g]), np.isnan(wf[g])), (tag, g, d['role'])
        if not np.isnan(ws[g]):
            es = abs(gs[g] - ws[g]) / ws[g] if ws[g] else abs(gs[g])
            worst[1] = max(worst[1], es)
            assert es <= 1e-12, (tag, g, 'seg', gs[g], ws[g])
        if d['role'] != 'interior':               # endpoint: zeros; mismatched / nonfinite: NaN on free rows, 0 on fixed ones
            assert np.array_equal(gd[s], wd[s], equal_nan=True), (tag, g, d['role'])
            assert d['role'] != 'endpoint' or gf[g] == 0.0
            continue
        fx = c.fixed[s]
        assert np.array_equal(gd[s][fx], np.zeros((int(fx.sum()), 3), np.float32)), (tag, g, 'fixed rows')
        ef = abs(gf[g] - wf[g]) / max(np.sqrt(d['F2']), 1e-300)
        worst[2] = max(worst[2], ef)
        assert ef <= 1e-12, (tag, g, 'fpar', gf[g], wf[g])
        if fx.all():
            continue
        assert np.isfinite(gd[s][~fx]).all(), (tag, g)
        e = maxnorm_err(gd[s][~fx], wd[s][~fx])
        worst[0] = max(worst[0], e)
        assert e <= KTOL, (tag, g, d.get('branch'), e)
    return worst


# ------------------------------------------------------------------------------------------- the analytic potential
W_BANDS = [(5, 1), (8, 4), (7, 3), (11, 2)]       # (images, atoms)
W_H, W_KAPPA, W_S = (1.0, 1.5, 0.8, 2.0), (2.0, 3.0, 1.5, 2.5), (0.5, 0.6, 0.4, 0.7)
W_K, W_KT = (0.1, 0.2, 0.15, 0.3), (1.0, 1.5, 2.0, 1.2)
W_FMAX, W_CLIMB, W_NOISE, W_MAX, W_SEED, W_SLOTS = 0.01, 40, 0.02, 500, 31, 4


def _well(bands=(0, 1, 2, 3)):
    """The batch of the bands `bands` of W_BANDS.  Per graph, atom 0 sits in h (x^2 - 1)^2 + kappa (y - s (1 - x^2))^2 + kappa z^2
    and every other atom a is tethered to it by 1/2 k_t |r_a - r_0 - delta_a|^2: minima at x = -1 / +1 with E = 0, one first-order
    saddle at x = 0, y = s with E = h exactly, and a curved minimum-energy path.  Each band's numbers come from its own seed."""
    key = ('well',) + tuple(bands)
    if key in _MADE:
        return _MADE[key]
    w = Case()
    w.bands = tuple(bands)
    pos, delta, graph_par, counts = [], [], [], []
    for b in bands:
        L, m = W_BANDS[b]
        rng = np.random.RandomState(W_SEED + b)
        dl = np.concatenate([np.zeros((1, 3)), rng.uniform(-1.0, 1.0, (m - 1, 3))])
        for j in range(L):
            r0 = np.array([-1.0 + 2.0 * j / (L - 1), 0.0, 0.0])
            r = r0 + dl
            if 0 < j < L - 1:
                r = r + W_NOISE * rng.uniform(-1.0, 1.0, (m, 3))
            pos.append(r), delta.append(dl), counts.append(m)
            graph_par.append((W_H[b], W_KAPPA[b], W_S[b], W_KT[b]))
    w.pos0 = np.concatenate(pos).astype(np.float32)
    w.delta = np.concatenate(delta)
    w.par = np.asarray(graph_par, dtype=np.float64)               # [G, 4]: h, kappa, s, k_t
    w.gptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    w.band_ptr = np.concatenate([[0], np.cumsum([W_BANDS[b][0] for b in bands])]).astype(np.int32)
    w.batch = np.repeat(np.arange(len(counts)), counts)
    w.k = np.asarray([W_K[b] for b in bands], dtype=np.float64)
    w.aptr = w.gptr[w.band_ptr]
    ends = np.zeros(len(counts), dtype=bool)
    ends[w.band_ptr[:-1]] = ends[w.band_ptr[1:] - 1] = True
    w.move_fixed = ends[w.batch]
    _MADE[key] = w
    return w


def _well_eval(w, pos32):
    """(E fp32 [G], dE/dpos fp32 [N, 3]) of the analytic potential, formed in fp64 from the fp32 positions."""
    r = pos32.astype(np.float64)
    first = w.gptr[:-1][w.batch]
    h, kap, s, kt = (w.par[:, i] for i in range(4))
    x, y, z = (r[w.gptr[:-1], i] for i in range(3))
    q = y - s * (1.0 - x * x)
    E = h * (x * x - 1.0) ** 2 + kap * q * q + kap * z * z
    dE = np.zeros_like(r)
    dE[w.gptr[:-1]] = np.stack([4.0 * h * x * (x * x - 1.0) + 2.0 * kap * q * 2.0 * s * x, 2.0 * kap * q, 2.0 * kap * z], 1)
    u = r - r[first] - w.delta                                     # (zero rows for atom 0)
    E = E + np.bincount(w.batch, weights=0.5 * kt[w.batch] * (u * u).sum(1), minlength=len(h))
    g = kt[w.batch, None] * u
    dE += g
    np.subtract.at(dE, first, g)
    return E.astype(np.float32), dE.astype(np.float32)


def _well_reference(bands=(0, 1, 2, 3), climb_after=W_CLIMB):
    """The driver's loop restated on the CPU: _well_eval, neb_force_ref, fire_step_ref over the band ranges.  Returns a Case with
    the final pos, energy, state, iterations and barriers."""
    key = ('wellref', tuple(bands), climb_after)
    if key in _MADE:
        return _MADE[key]
    w = _well(bands)
    n, G, B = w.pos0.shape[0], len(w.gptr) - 1, len(w.band_ptr) - 1
    pos, vel = w.pos0.copy(), np.zeros((n, 3), np.float32)
    st = dict(dt=np.full(B, 0.1), a=np.full(B, 0.1), n_pos=np.zeros(B, np.int32), steps=np.zeros(B, np.int32),
              status=np.zeros(B, np.int32), fmax=np.zeros(B, np.float32))
    climb = np.full(B, climb_after == 0)
    out = None
    r = Case()
    for it in range(W_MAX):
        if climb_after and it == climb_after:
            climb[:] = True
            vel[:] = 0.0
            st['dt'][:], st['a'][:], st['n_pos'][:] = 0.1, 0.1, 0
            st['status'][st['status'] == 1] = 0
        E, dE = _well_eval(w, pos)
        out = neb_force_ref(pos, dE, E, w.gptr, w.band_ptr, w.k, None, st['status'], climb, out=out)
        pos, vel, st = fire_step_ref(pos, vel, out[0], w.aptr, st, W_FMAX, w.move_fixed, **DEFAULTS)
        if (climb_after is None or it >= climb_after) and not (st['status'] == 0).any():
            break
    r.iterations, r.pos, r.state = it + 1, pos, st
    r.energy, _ = _well_eval(w, pos)
    r.saddle = np.asarray([climbing_image(r.energy, int(w.band_ptr[b]), int(w.band_ptr[b + 1]) - 1) for b in range(B)])
    r.barrier_fwd = r.energy[r.saddle].astype(np.float64) - r.energy[w.band_ptr[:-1]]
    r.barrier_rev = r.energy[r.saddle].astype(np.float64) - r.energy[w.band_ptr[1:] - 1]
    _MADE[key] = r
    return r


def _well_bound(b):
    """n_free fmax^2 / (2 c_min) + 1e-6 h for band b of W_BANDS: c_min is the smallest absolute eigenvalue of the Hessian of one
    image at the saddle (atom 0 at (0, s, 0), the others at their tethers), by central differences of the fp64 gradient."""
    L, m = W_BANDS[b]
    h, kap, s, kt = W_H[b], W_KAPPA[b], W_S[b], W_KT[b]
    rng = np.random.RandomState(W_SEED + b)
    dl = np.concatenate([np.zeros((1, 3)), rng.uniform(-1.0, 1.0, (m - 1, 3))])

    def grad(r):
        x, y, z = r[0]
        q = y - s * (1.0 - x * x)
        g = np.zeros_like(r)
        g[0] = [4.0 * h * x * (x * x - 1.0) + 4.0 * kap * q * s * x, 2.0 * kap * q, 2.0 * kap * z]
        u = r - r[0] - dl
        g += kt * u
        g[0] -= kt * u.sum(0)
        return g.reshape(-1)

    r = np.array([0.0, s, 0.0]) + dl
    assert np.abs(grad(r)).max() < 1e-12                           # (a stationary point)
    eps, H = 1e-5, np.zeros((3 * m, 3 * m))
    for i in range(3 * m):
        e = np.zeros(3 * m)
        e[i] = eps
        H[i] = (grad(r + e.reshape(m, 3)) - grad(r - e.reshape(m, 3))) / (2.0 * eps)
    lam = np.linalg.eigvalsh(0.5 * (H + H.T))
    assert (lam < 0).sum() == 1, lam                               # (first order)
    return m * W_FMAX ** 2 / (2.0 * np.abs(lam).min()) + 1e-6 * h, float(np.abs(lam).min())


class Well(torch.nn.Module):
    """The analytic potential as a plain torch module, differentiable with respect to data.pos.  Every graph gathers its atoms
    into W_SLOTS slots (an unused slot points at atom 0 and weighs 0) and adds their terms in slot order: elementwise launches
    only, so a graph's energy and gradient are bitwise the same whatever else the batch holds."""

    def __init__(self, w):
        super().__init__()
        G = len(w.gptr) - 1
        idx, valid, delta = np.zeros((G, W_SLOTS), np.int64), np.zeros((G, W_SLOTS), np.float32), np.zeros((G, W_SLOTS, 3), np.float32)
        for g in range(G):
            lo, hi = int(w.gptr[g]), int(w.gptr[g + 1])
            idx[g] = lo
            idx[g, :hi - lo] = np.arange(lo, hi)
            valid[g, 1:hi - lo] = 1.0
            delta[g, :hi - lo] = w.delta[lo:hi]
        for name, v in (('idx', idx), ('valid', valid), ('delta', delta), ('par', w.par.astype(np.float32))):
            self.register_buffer(name, torch.from_numpy(v))

    def forward(self, data):
        r = data.pos[self.idx]                                     # [G, slots, 3]
        h, kap, s, kt = self.par.unbind(1)
        x, y, z = r[:, 0, 0], r[:, 0, 1], r[:, 0, 2]
        q = y - s * (1.0 - x * x)
        t = x * x - 1.0
        e = h * t * t + kap * q * q + kap * z * z
        for j in range(1, W_SLOTS):
            u = r[:, j] - r[:, 0] - self.delta[:, j]
            e = e + self.valid[:, j] * (0.5 * kt) * (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1] + u[:, 2] * u[:, 2])
        return e


def _well_data(w, dev):
    from pamnet_amd import synth
    return synth.Batch(pos=torch.from_numpy(w.pos0), batch=torch.from_numpy(w.batch), num_graphs=len(w.gptr) - 1,
                       band_ptr=torch.from_numpy(w.band_ptr)).to(dev)


# ---------------------------------------------------------------------------------------------------------- CPU tests
def test_header_declares_the_projection_at_abi_18():
    """(No GPU: the header and the built library.)"""
    import ctypes
    import re
    from pamnet_amd import build, lib
    decl = lib.declared_functions()
    assert ENTRY in decl
    P, D, I = ctypes.c_void_p, ctypes.c_double, ctypes.c_int64
    assert decl[ENTRY] == [P] * 5 + [I] * 2 + [P] * 2 + [I] + [P] * 3 + [D] + [P] * 4
    assert int(re.search(r'#define\s+PAMNET_ABI_VERSION\s+(\d+)', open(lib.HEADER).read()).group(1)) == 18
    h = ctypes.CDLL(build.build())
    assert h.pamnet_abi_version() == 18 and hasattr(h, ENTRY)


def test_neb_kernel_is_scratch_free(tmp_path):
    """(No GPU: hipcc cross-compiles.)  The compiler's report for csrc/neb.hip: no scratch, fewer than 64 registers, the six fp64
    partials of four wavefronts in LDS (DESIGN section 12 quotes the figures)."""
    import os
    import re
    import shutil
    import subprocess
    from pamnet_amd import build
    hipcc = '/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else shutil.which('hipcc')
    assert hipcc, 'hipcc not available'
    r = subprocess.run([hipcc] + build.FLAGS + ['-c', os.path.join(build.CSRC, 'neb.hip'), '-o', str(tmp_path / 'neb.o'),
                                                '-Rpass-analysis=kernel-resource-usage'], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = [b for b in re.split(r'remark: Function Name: ', r.stderr)[1:] if 'neb_force_kernel' in b.split()[0]]
    assert len(blocks) == 1
    num = lambda key: int(re.search(key + r': (\d+)', blocks[0]).group(1))
    assert num(r'ScratchSize \[bytes/lane\]') == 0
    assert num('VGPRs') + num('AGPRs') <= 64 and num(r'LDS Size \[bytes/block\]') <= 256


def test_the_reference_on_hand_made_bands():
    """(No GPU; a test of the reference.)  One atom, R- = (0, 0, 0), R0 = (1, 0, 0), R+ = (1, 2, 0): d- = (1, 0, 0), d+ = (0, 2, 0);
    F = (3, 4, 0), k = 0.5, so the spring term is 0.5 (2 - 1) t^.  The four tangent branches and the climbing inversion, with the
    answers written out."""
    pos = np.array([[0, 0, 0], [1, 0, 0], [1, 2, 0]], np.float32)
    dE = np.array([[9, 9, 9], [-3, -4, 0], [9, 9, 9]], np.float32)
    gptr, band_ptr = [0, 1, 2, 3], [0, 3]
    r10 = np.sqrt(10.0)
    cases = [  # energies, climb, t^, fpar, F_neb
        ([0, 1, 2], False, [0, 1, 0], 4.0, [3.0, 0.5, 0.0]),
        ([2, 1, 0], False, [1, 0, 0], 3.0, [0.5, 4.0, 0.0]),
        ([0, 3, 1], False, [1 / r10, 3 / r10, 0], 15 / r10, [3 - 1.5 + 0.5 / r10, 4 - 4.5 + 1.5 / r10, 0.0]),
        ([1, 3, 0], False, [0.6, 0.8, 0], 5.0, [0.3, 0.4, 0.0]),
        ([1, 3, 0], True, [0.6, 0.8, 0], 5.0, [-3.0, -4.0, 0.0]),
        ([0, 1, 2], True, [0, 1, 0], 4.0, [3.0, -4.0, 0.0]),
        ([1, 1, 1], False, [0, 0, 0], 0.0, [3.0, 4.0, 0.0]),
    ]
    branches = set()
    for E, climb, that, fp, fneb in cases:
        diag = {}
        dneb, seg, fpar = neb_force_ref(pos, dE, np.asarray(E, np.float32), gptr, band_ptr, 0.5, climb=[climb], diag=diag)
        assert np.allclose(diag[1]['that'][0], that, rtol=0, atol=1e-15), (E, diag[1]['that'])
        assert abs(fpar[1] - fp) < 1e-14 and fpar[0] == 0.0 and fpar[2] == 0.0
        assert np.allclose(-dneb[1].astype(np.float64), fneb, rtol=0, atol=1e-6), (E, climb, dneb[1])
        assert not dneb[0].any() and not dneb[2].any()
        assert seg.tolist() == [0.0, 1.0, 2.0]
        assert diag[1]['climbing'] == climb
        branches.add(diag[1]['branch'])
    assert branches == {'rising', 'falling', 'extremum+', 'extremum-'}
    # a tie goes to the lowest index, a NaN never climbs, endpoints never climb
    assert climbing_image(np.array([9, 1, 2, 2, 0], np.float32), 0, 4) == 2
    assert climbing_image(np.array([9, np.nan, 2, 1, 9], np.float32), 0, 4) == 2
    assert climbing_image(np.array([0, 1], np.float32), 0, 1) == -1


def test_the_kernel_batches_take_every_branch():
    """(No GPU.)  The three kernel-test batches: the image sizes and band lengths the test names, and together every role."""
    seen, sizes, lengths = set(), set(), set()
    for shift in SHIFTS:
        c = _kernel_case(shift)
        sizes.update(int(b - a) for a, b in zip(c.gptr[:-1], c.gptr[1:]))
        lengths.update(int(b - a) for a, b in zip(c.band_ptr[:-1], c.band_ptr[1:]))
        dneb, seg, fpar = c.ref
        for b, p in enumerate(c.pieces):
            first, last = int(c.band_ptr[b]), int(c.band_ptr[b + 1]) - 1
            for g in range(first, last + 1):
                s = slice(int(c.gptr[g]), int(c.gptr[g + 1]))
                d = c.diag.get(g)
                if p.role == 'status':
                    assert d is None and (dneb[s] == SENTINEL).all() and seg[g] == SENTINEL64
                    seen.add('status')
                    continue
                if d['role'] == 'endpoint':
                    assert not dneb[s].any() and fpar[g] == 0.0 and (g != first or seg[g] == 0.0)
                    seen.add('first' if g == first else 'last')
                    continue
                fx = c.fixed[s]
                assert not dneb[s][fx].any()
                if d['role'] in ('mismatched', 'nonfinite'):
                    assert np.isnan(dneb[s][~fx]).all() and np.isnan(fpar[g])
                    seen.add(d['role'] if p.role not in ('nan_energy', 'inf_grad') else p.role)
                    continue
                seen.add(d['branch'])
                E = c.energy[g - 1:g + 2]
                if E[2] == E[1] or E[0] == E[1]:
                    seen.add('E+ == E0' if E[2] == E[1] else 'E- == E0')
                if d['branch'].startswith('extremum') and E[1] < min(E[0], E[2]):
                    seen.add('minimum')
                if d['climbing']:
                    assert p.climb
                    seen.add('climbing')
                    if (c.energy[first + 1:last] == c.energy[g]).sum() > 1:
                        assert g == first + 1 + int(np.argmax(c.energy[first + 1:last] == c.energy[g]))
                        seen.add('climbing tie')
                if not p.climb:
                    seen.add('climb off')
                if d['t2'] == 0.0 and not fx.all():
                    assert np.array_equal(dneb[s][~fx], c.dE[s][~fx])
                    seen.add('zero tangent')
                if fx.all() and s.stop > s.start:
                    seen.add('all fixed')
                elif fx.any():
                    assert np.isnan(c.pos[s][fx]).all() and np.isnan(c.dE[s][fx]).all() and np.isfinite(dneb[s]).all()
                    seen.add('some fixed')
    assert sizes >= set(SIZES) and lengths == {1, 2, 3, 4, 9}, (sizes, lengths)
    want = {'first', 'last', 'rising', 'falling', 'extremum+', 'extremum-', 'minimum', 'E+ == E0', 'E- == E0', 'climbing',
            'climbing tie', 'climb off', 'status', 'nan_energy', 'inf_grad', 'all fixed', 'some fixed', 'zero tangent', 'mismatched'}
    assert seen == want, (seen ^ want)


def test_the_reference_finds_the_saddle_of_the_analytic_potential():
    """(No GPU.)  The preconditions of the end-to-end test, on the reference alone: every band converges, with its own number of
    steps; both barriers are within n_free fmax^2 / (2 c_min) + 1e-6 h of h; the straight interpolation is not the answer."""
    w, r = _well(), _well_reference()
    assert (r.state['status'] == 1).all(), r.state
    print('reference: iterations', r.iterations, 'steps', r.state['steps'], 'fmax', r.state['fmax'])
    for i, b in enumerate(w.bands):
        bound, c_min = _well_bound(b)
        print('band', b, 'h', W_H[b], 'barrier_fwd - h', r.barrier_fwd[i] - W_H[b], 'barrier_rev - h', r.barrier_rev[i] - W_H[b],
              'bound', bound, 'c_min', c_min)
        assert abs(r.barrier_fwd[i] - W_H[b]) <= bound and abs(r.barrier_rev[i] - W_H[b]) <= bound
        s = int(r.saddle[i])
        x, y = r.pos[w.gptr[s], 0], r.pos[w.gptr[s], 1]
        assert abs(x) < 0.02 and abs(y - W_S[b]) < 0.02, (x, y)    # the climbing image sits on the curved path's saddle
    assert len(set(r.state['steps'].tolist())) > 1


def test_without_the_climbing_image_the_barrier_is_underestimated():
    """(No GPU.)  The 8-image band alone, plain NEB on the reference: no image sits at x = 0, and the highest one reads more than
    5 % below h = 1.5 -- so a test of the barrier exercises the climbing branch."""
    r = _well_reference(bands=(1,), climb_after=None)
    assert (r.state['status'] == 1).all()
    print('plain NEB, 8 images: barrier', r.barrier_fwd[0], 'of h', W_H[1])
    assert r.barrier_fwd[0] < 0.95 * W_H[1]


def _interpolate_ref(pos_i, pos_f, batch, cell, pbc, images):
    """numpy fp64: the shortest image of final - initial over the lattice translations -2 .. 2 of the periodic axes, then the
    straight line; -> (pos fp32, band_ptr)."""
    out = []
    for b, L in enumerate(images):
        rows = np.nonzero(batch == b)[0]
        d = pos_f[rows].astype(np.float64) - pos_i[rows].astype(np.float64)
        if cell is not None:
            a = np.asarray(cell[b], dtype=np.float64) * np.asarray(pbc[b], dtype=np.float64)[:, None]
            n = np.array([(i, j, k) for i in range(-2, 3) for j in range(-2, 3) for k in range(-2, 3)], dtype=np.float64)
            cand = d[:, None, :] - (n @ a)[None]
            d = cand[np.arange(len(rows)), (cand * cand).sum(2).argmin(1)]
        for j in range(L):
            out.append((pos_i[rows].astype(np.float64) + j / (L - 1.0) * d).astype(np.float32))
    return np.concatenate(out), np.concatenate([[0], np.cumsum(images)])


def _pamnet_endpoints():
    """(initial, final, fixed of the initial batch, n_images): the batch of tests/test_relax.py _pamnet_batch -- a bond-free
    molecule, a triclinic cell, a slab whose bottom layer is fixed -- and a copy displaced by up to 0.3 A per coordinate (fixed
    atoms stay), in which atom 3 of the triclinic cell has moved on by 0.6 of the first cell vector: its shortest way back is
    -0.4 of it."""
    if 'pamnet' in _MADE:
        return _MADE['pamnet']
    from test_relax import _pamnet_batch
    from test_pbc_axes import TRI_A
    b, fixed = _pamnet_batch()
    rng = np.random.RandomState(17)
    d = rng.uniform(-0.3, 0.3, tuple(b.pos.shape))
    d[fixed.numpy()] = 0.0
    d[12 + 3] += 0.6 * np.asarray(TRI_A[0])
    final = copy.copy(b)
    final.pos = (b.pos.double() + torch.from_numpy(d)).float()
    _MADE['pamnet'] = (b, final, fixed, [3, 4, 3])
    return _MADE['pamnet']


def test_interpolate_against_a_numpy_restatement():
    """(No GPU: interpolate is plain torch.)  Positions of every image, the minimum-image branch (one atom's endpoints differ by
    more than half a cell vector; the molecule's open axes and the slab's open axis are not reduced), the replicated fields and
    band_ptr; an edge_index is offset per image."""
    from pamnet_amd import neb, synth
    initial, final, fixed, images = _pamnet_endpoints()
    band = neb.interpolate(initial, final, images)
    pbc = initial.pbc.numpy()
    want, band_ptr = _interpolate_ref(initial.pos.numpy(), final.pos.numpy(), initial.batch.numpy(), initial.cell.numpy(), pbc, images)
    assert band.band_ptr.dtype == torch.int32 and band.band_ptr.tolist() == band_ptr.tolist() and band.num_graphs == 10
    assert band.pos.dtype == torch.float32 and np.abs(band.pos.numpy().astype(np.float64) - want).max() <= 1e-6
    counts = np.bincount(initial.batch.numpy())
    graph_src = np.repeat(np.arange(3), images)
    assert band.batch.tolist() == np.repeat(np.arange(10), counts[graph_src]).tolist() and band.batch.dtype == initial.batch.dtype
    assert torch.equal(band.cell, initial.cell[torch.from_numpy(graph_src)]) and torch.equal(band.pbc, initial.pbc[torch.from_numpy(graph_src)])
    lo = 12 * 3                                                    # the first image of the triclinic band is `initial`, its last
    assert torch.equal(band.pos[lo:lo + 24], initial.pos[12:36])   # `final` up to the lattice step of the atom that went round
    last = band.pos[lo + 3 * 24:lo + 4 * 24].double() - final.pos[12:36].double()
    tri = initial.cell[1].double()
    assert float((last[3] + tri[0]).abs().max()) < 1e-5 and float(last[torch.arange(24) != 3].abs().max()) < 1e-6
    step = (band.pos[lo + 24:lo + 48] - band.pos[lo:lo + 24]).double().norm(dim=1)
    assert float(step.max()) < 0.5 * float(tri[0].norm()) / 3 + 0.3
    for t in (band.x,):
        assert torch.equal(t, torch.cat([initial.x[initial.batch == g] for g in graph_src]))
    # bonded molecules: edges follow their image
    a, b2 = synth.qm9_batch(0, 0, 2), synth.qm9_batch(0, 0, 2)
    b2.pos = a.pos + 0.1
    bonded = neb.interpolate(a, b2, [3, 4])
    n0, n1 = int((a.batch == 0).sum()), int((a.batch == 1).sum())
    e0, e1 = a.edge_index[:, a.batch[a.edge_index[0]] == 0], a.edge_index[:, a.batch[a.edge_index[0]] == 1]
    want_ei = torch.cat([e0 + j * n0 for j in range(3)] + [e1 - n0 + 3 * n0 + j * n1 for j in range(4)], 1)
    assert torch.equal(bonded.edge_index, want_ei) and not hasattr(bonded, 'cell')
    assert torch.allclose(bonded.pos[n0:2 * n0], a.pos[:n0] + 0.05, atol=1e-6)
    # refusals
    with pytest.raises(ValueError, match='at least 3 images'):
        neb.interpolate(initial, final, 2)
    with pytest.raises(ValueError, match='list of num_graphs = 3 ints'):
        neb.interpolate(initial, final, [3, 3])
    other = copy.copy(final)
    other.cell = final.cell * 1.01
    with pytest.raises(ValueError, match='share their cell'):
        neb.interpolate(initial, other, 3)
    other = copy.copy(final)
    other.x = final.x.flip(0)
    with pytest.raises(ValueError, match='atom types'):
        neb.interpolate(initial, other, 3)
    other = copy.copy(final)
    other.pos = final.pos[:-1]
    with pytest.raises(ValueError, match='same atoms'):
        neb.interpolate(initial, other, 3)


def test_neb_refusals():
    """(No GPU.)  A PAMNet that keeps its positions in x, a batch without band_ptr, an unknown FIRE parameter, and CPU tensors
    (RuntimeError: no CPU path) are refused before anything runs."""
    import models
    from pamnet_amd import neb, synth
    w = _well()
    model = Well(w)
    data = synth.Batch(pos=torch.from_numpy(w.pos0), batch=torch.from_numpy(w.batch), num_graphs=len(w.gptr) - 1,
                       band_ptr=torch.from_numpy(w.band_ptr))
    pdb = models.PAMNet(models.Config(dataset='PDBbind', dim=16, n_layer=1, cutoff_l=2.0, cutoff_g=6.0))
    with pytest.raises(ValueError, match=r'x\[:, :3\]'):
        neb.run(pdb, data)
    with pytest.raises(ValueError, match='no `band_ptr`'):
        neb.run(model, synth.Batch(pos=data.pos, batch=data.batch, num_graphs=data.num_graphs))
    with pytest.raises(TypeError, match='dt_min'):
        neb.run(model, data, dt_min=0.01)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        neb.run(model, data)
    assert torch.equal(data.pos, torch.from_numpy(w.pos0))


# ------------------------------------------------------------------------------------------------------- kernel tests
def _project_on_device(dev, c, k=None, with_start=True):
    """One launch on the batch `c` -> (dneb, seg, fpar) as numpy.  k: None = the per-band array of the case."""
    from pamnet_amd import neb
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n, G = c.pos.shape[0], len(c.gptr) - 1
    if with_start:
        dneb, seg, fpar = torch.full((n, 3), float(SENTINEL), device=dev), torch.full((G,), SENTINEL64, dtype=torch.float64, device=dev), \
            torch.full((G,), SENTINEL64, dtype=torch.float64, device=dev)
    else:
        dneb, seg, fpar = torch.zeros(n, 3, device=dev), torch.zeros(G, dtype=torch.float64, device=dev), torch.zeros(G, dtype=torch.float64, device=dev)
    neb.neb_force(t(c.pos), t(c.dE), t(c.energy), t(c.gptr), t(c.band_ptr), t(c.band_of), dneb, t(c.k) if k is None else k,
                  seg, fpar, t(c.fixed.astype(np.uint8)), t(c.status), t(c.climb.astype(np.uint8)))
    return dneb.cpu().numpy(), seg.cpu().numpy(), fpar.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('shift', SHIFTS)
def test_one_projection_of_a_batch_vs_the_reference(dev, shift):
    """Bands of 3, 4 and 9 images of 1, 2, 63, 64, 65, 255, 256, 257, 1025 and 0 atoms, a band of 2, a band of 1 and two bands
    whose atom counts change on the way (_kernel_case; the shift moves the roles over the sizes): dneb within KTOL per graph, seg
    to 1e-12, fpar to 1e-12 of sqrt(sum F^2); zeros, NaN placement and the sentinel rows of a band that is not running, equal."""
    c = _kernel_case(shift)
    got = _project_on_device(dev, c)
    worst = _assert_projection(got, c.ref, c, c.diag, c.start, tag=shift)
    print('shift', shift, 'worst dneb / seg / fpar error', worst)


@pytest.mark.gpu
def test_a_scalar_spring_constant_is_the_array_of_that_value(dev):
    c = copy.copy(_kernel_case(3))
    c.k = np.full(len(c.pieces), 0.37)
    a = _project_on_device(dev, c)
    b = _project_on_device(dev, c, k=0.37)
    assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b))
    assert np.isfinite(a[0]).sum() > 1000


@pytest.mark.gpu
def test_a_projection_is_repeatable_and_independent_of_the_batch(dev):
    """Two launches on the same inputs are equal bit for bit, and every band projected alone, and behind another band (another
    place in the batch), gives the rows of the batched call."""
    c = _kernel_case(7)
    one, two = _project_on_device(dev, c, with_start=False), _project_on_device(dev, c, with_start=False)
    assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(one, two))
    for b, p in enumerate(c.pieces):
        g0, g1 = int(c.band_ptr[b]), int(c.band_ptr[b + 1])
        a0, a1 = int(c.gptr[g0]), int(c.gptr[g1])
        alone = _project_on_device(dev, _assemble([p]), with_start=False)
        other = c.pieces[(b + 5) % len(c.pieces)]
        behind = _project_on_device(dev, _assemble([other, p]), with_start=False)
        sg, sa = len(other.counts), sum(other.counts)
        for got, (gs, as_) in ((alone, (0, 0)), (behind, (sg, sa))):
            assert np.array_equal(got[0][as_:], one[0][a0:a1], equal_nan=True), b
            assert np.array_equal(got[1][gs:], one[1][g0:g1], equal_nan=True) and np.array_equal(got[2][gs:], one[2][g0:g1], equal_nan=True), b


@pytest.mark.gpu
def test_the_entry_point_validates_its_arguments(dev):
    """A null required pointer is PAMNET_ENULL, a bad count or a scalar k that is negative or NaN PAMNET_EINVAL -- return codes
    only, nothing is launched; fixed, band_status, climb, k_b, seg and fpar may be null; no graphs: nothing is written."""
    from pamnet_amd import lib
    c = _kernel_case(0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ten = dict(pos=t(c.pos), dpos=t(c.dE), energy=t(c.energy), gptr=t(c.gptr), band_ptr=t(c.band_ptr), band_of=t(c.band_of),
               dneb=torch.full((c.pos.shape[0], 3), float(SENTINEL), device=dev))
    n, G, B = c.pos.shape[0], len(c.gptr) - 1, len(c.band_ptr) - 1

    def call(**kw):
        a = dict({name: lib.ptr(v) for name, v in ten.items()}, fixed=None, n=n, G=G, B=B, band_status=None, climb=None, k_b=None,
                 k=0.1, seg=None, fpar=None)
        a.update(kw)
        lib.call(ENTRY, a['pos'], a['dpos'], a['energy'], a['fixed'], a['gptr'], a['n'], a['G'], a['band_ptr'], a['band_of'], a['B'],
                 a['band_status'], a['climb'], a['k_b'], a['k'], a['dneb'], a['seg'], a['fpar'], lib.stream_of(ten['pos']))

    for name in ten:
        with pytest.raises(RuntimeError, match='PAMNET_ENULL'):
            call(**{name: None})
    for kw in (dict(n=-1), dict(G=-1), dict(B=-1), dict(G=2 ** 31), dict(B=2 ** 31), dict(k=-0.1), dict(k=float('nan'))):
        with pytest.raises(RuntimeError, match='PAMNET_EINVAL'):
            call(**kw)
    call(G=0)
    torch.cuda.synchronize()
    assert (ten['dneb'] == float(SENTINEL)).all()
    call()                                                         # every optional pointer null: all bands run, nothing climbs
    want = neb_force_ref(c.pos, c.dE, c.energy, c.gptr, c.band_ptr, 0.1, diag=None)
    got = ten['dneb'].cpu().numpy()
    rows = np.isfinite(want[0]).all(1) & np.isfinite(c.pos).all(1)
    assert np.array_equal(np.isnan(got), np.isnan(want[0])) and maxnorm_err(got[rows], want[0][rows]) <= KTOL


# ----------------------------------------------------------------------------------------------------- end to end
def _replay(res, gptr, band_ptr, aptr, k, fixed, move_fixed, fmax, tag):
    """Every step of a trace, launch by launch, against neb_force_ref and fire_step_ref on the step's own recorded inputs."""
    from test_relax import _assert_step_matches
    cpu = lambda t: t.cpu().numpy()
    c = Case()
    c.gptr, c.fixed = gptr, np.zeros(int(gptr[-1]), dtype=bool) if fixed is None else fixed
    worst = [0.0] * 5
    for i, r in enumerate(res.trace):
        status = cpu(r['state_before']['status'])
        start = (cpu(r['dneb_before']), cpu(r['seg_before']), cpu(r['fpar_before']))
        diag = {}
        want = neb_force_ref(cpu(r['pos']), cpu(r['dE']), cpu(r['energy']), gptr, band_ptr, k, fixed, status, cpu(r['climb']) != 0,
                             out=start, diag=diag)
        got = (cpu(r['dneb']), cpu(r['seg']), cpu(r['fpar']))
        w3 = _assert_projection(got, want, c, diag, start, tag=(tag, i))
        before = (cpu(r['pos']), cpu(r['v_before']), {name: cpu(v) for name, v in r['state_before'].items()})
        after = (cpu(r['pos_after']), cpu(r['v_after']), {name: cpu(v) for name, v in r['state_after'].items()})
        step = fire_step_ref(before[0], before[1], got[0], aptr, before[2], fmax, move_fixed, **DEFAULTS)
        w2 = _assert_step_matches(after, step, before, aptr, move_fixed, tag=(tag, i))
        worst = [max(a, b) for a, b in zip(worst, w3 + w2)]
        if i + 1 < len(res.trace):
            assert torch.equal(r['pos_after'], res.trace[i + 1]['pos'])
    return worst


@pytest.mark.gpu
def test_the_analytic_saddles_are_found(dev):
    """Four bands of different length, atom count, barrier, curvature and spring constant in one batch, climbing from step 40:
    every step replays against the references; all bands converge; both barriers are within n_free fmax^2 / (2 c_min) + 1e-6 h of
    h; the 8-image band without a climbing image reads more than 5 % low; each band run alone gives the same bits; and the loop
    synchronises only where the driver says it does."""
    from pamnet_amd import neb
    w = _well()
    model, data = Well(w).to(dev), _well_data(w, dev)
    k = torch.from_numpy(w.k).to(dev)
    pos0 = data.pos.clone()
    res = neb.run(model, data, fmax=W_FMAX, k=k, climb_after=W_CLIMB, max_steps=W_MAX, trace=True)
    assert torch.equal(data.pos, pos0) and res.converged.all() and not res.failed.any(), (res.converged, res.steps)
    worst = _replay(res, w.gptr, w.band_ptr, w.aptr, w.k, None, w.move_fixed, W_FMAX, 'well')
    print('analytic: iterations', len(res.trace), 'steps', res.steps.tolist(), 'worst dneb / seg / fpar / vel / displacement', worst)
    assert len(res.trace) > W_CLIMB and (res.fmax < W_FMAX).all()
    assert torch.equal(res.pos[torch.from_numpy(w.move_fixed).to(dev)], pos0[torch.from_numpy(w.move_fixed).to(dev)])
    for i, b in enumerate(w.bands):
        bound, _ = _well_bound(b)
        fwd, rev = float(res.barrier_fwd[i]), float(res.barrier_rev[i])
        print('band', b, 'barrier_fwd - h', fwd - W_H[b], 'barrier_rev - h', rev - W_H[b], 'bound', bound)
        assert abs(fwd - W_H[b]) <= bound and abs(rev - W_H[b]) <= bound
        first, last = int(w.band_ptr[i]), int(w.band_ptr[i + 1]) - 1
        assert first < int(res.saddle[i]) < last
        assert float(res.distance[first]) == 0.0 and (res.distance[first + 1:last + 1] > res.distance[first:last]).all()
        assert float(res.fpar[first]) == 0.0 and float(res.fpar[last]) == 0.0
    # the result belongs to the returned geometry
    d = copy.copy(data)
    d.pos = res.pos.clone().requires_grad_(True)
    e = model(d)
    de, = torch.autograd.grad(e.sum(), d.pos)
    assert torch.equal(res.energy, e.detach()) and torch.equal(res.forces, -de)
    E, dE = _well_eval(w, res.pos.cpu().numpy())
    assert maxnorm_err(res.energy.cpu().numpy(), E) <= 1e-5 and maxnorm_err(de.cpu().numpy(), dE) <= 1e-5
    # a band alone: the same bits
    for i, b in enumerate(w.bands):
        wb = _well((b,))
        rb = neb.run(Well(wb).to(dev), _well_data(wb, dev), fmax=W_FMAX, k=W_K[b], climb_after=W_CLIMB, max_steps=W_MAX)
        g0, g1 = int(w.band_ptr[i]), int(w.band_ptr[i + 1])
        a0, a1 = int(w.gptr[g0]), int(w.gptr[g1])
        for name in ('pos', 'forces', 'neb_forces'):
            assert torch.equal(getattr(rb, name), getattr(res, name)[a0:a1]), (b, name)
        for name in ('energy', 'distance', 'fpar'):
            assert torch.equal(getattr(rb, name), getattr(res, name)[g0:g1]), (b, name)
        for name in ('steps', 'fmax', 'converged', 'barrier_fwd', 'barrier_rev'):
            assert torch.equal(getattr(rb, name), getattr(res, name)[i:i + 1]), (b, name)
        assert int(rb.saddle[0]) == int(res.saddle[i]) - g0
    # plain NEB on the 8-image band: no image at the saddle
    wb = _well((1,))
    plain = neb.run(Well(wb).to(dev), _well_data(wb, dev), fmax=W_FMAX, k=W_K[1], climb_after=None, max_steps=W_MAX)
    print('plain NEB, 8 images: barrier', float(plain.barrier_fwd[0]))
    assert plain.converged.all() and float(plain.barrier_fwd[0]) < 0.95 * W_H[1]
    # synchronisation: one read at set-up, and the status vector every check_every steps
    try:
        torch.cuda.set_sync_debug_mode('warn')
    except Exception as e:                        # (a build without the debug mode: the rest of the test has run)
        print('set_sync_debug_mode is not available:', e)
        return
    try:
        counts = []
        for ce in (0, 5):
            with warnings.catch_warnings(record=True) as rec:
                warnings.simplefilter('always')
                r0 = neb.run(model, data, fmax=1e-9, k=k, climb_after=4, max_steps=10, check_every=ce)
            counts.append(sum('synchronizing' in str(x.message) for x in rec))
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert counts == [1, 3], counts
    assert r0.steps.tolist() == [10] * 4


@pytest.mark.gpu
def test_neb_refusals_on_the_device(dev):
    """Wrong dtypes and shapes, bands that are too short, unequal atom counts and values that are not finite raise ValueError."""
    from pamnet_amd import neb
    w = _well()
    model, data = Well(w).to(dev), _well_data(w, dev)
    B = len(w.band_ptr) - 1

    def variant(**kw):
        d = copy.copy(data)
        d.__dict__.update(kw)
        return d

    for d, kw, match in (
            (variant(band_ptr=data.band_ptr.float()), {}, '`data.band_ptr` is an int32'),
            (variant(band_ptr=data.band_ptr.cpu()), {}, '`data.band_ptr` is an int32'),
            (variant(band_ptr=data.band_ptr[:1]), {}, '`data.band_ptr` is an int32'),
            (variant(band_ptr=data.band_ptr[:-1]), {}, 'must be sorted, start at 0 and end at num_graphs'),
            (variant(band_ptr=data.band_ptr.flip(0)), {}, 'must be sorted'),
            (variant(band_ptr=torch.tensor([0, 2, 5, 13, 20, 31], dtype=torch.int32, device=dev)), {}, 'at least 3 images'),
            (variant(band_ptr=torch.tensor([0, 6, 13, 20, 31], dtype=torch.int32, device=dev)), {}, 'same number of atoms'),
            (data, dict(k=torch.full((B,), 0.1, device=dev)), 'a per-band `k`'),
            (data, dict(k=torch.full((B + 1,), 0.1, dtype=torch.float64, device=dev)), 'a per-band `k`'),
            (data, dict(k=torch.tensor([0.1, -0.1, 0.1, 0.1], dtype=torch.float64, device=dev)), '`k` must be finite'),
            (data, dict(k=-1.0), '`k` must be finite'),
            (data, dict(k='soft'), '`k`'),
            (data, dict(fmax=torch.full((B,), 0.1, dtype=torch.float64, device=dev)), 'a per-band `fmax`'),
            (data, dict(fmax=torch.tensor([0.1, float('nan'), 0.1, 0.1], device=dev)), '`fmax` must be finite'),
            (data, dict(climb_after=-1), '`climb_after`'),
            (data, dict(fixed=torch.zeros(3, dtype=torch.bool, device=dev)), '`fixed` is a torch.bool tensor')):
        with pytest.raises(ValueError, match=match):
            neb.run(model, d, max_steps=1, **kw)
    # per-band thresholds and a failing band: the others go on
    tol = torch.tensor([W_FMAX, 100.0, W_FMAX, W_FMAX], device=dev)
    bad = data.pos.clone()
    bad[int(w.gptr[int(w.band_ptr[2]) + 1]), 0] = float('nan')
    res = neb.run(model, variant(pos=bad), fmax=tol, k=0.1, climb_after=0, max_steps=30)
    assert res.failed.tolist() == [False, False, True, False] and res.steps[1] == 0 and res.converged[1] and res.steps[2] == 0
    assert int(res.steps[0]) > 0 and int(res.steps[3]) > 0


@pytest.mark.gpu
@pytest.mark.parametrize('dim,n_layer', MODELS)
def test_pamnet_bands_replayed_step_by_step(dev, dim, n_layer):
    """PAMNet on bands made by interpolate -- a bond-free molecule, a triclinic cell with an atom that goes the short way round,
    a slab with a fixed bottom layer -- 10 steps, the climbing image from step 5: interpolate's positions against the numpy
    restatement, every recorded step against the references, res.energy / res.forces bitwise a fresh evaluation at res.pos;
    endpoint images, fixed rows and the caller's positions as they were.  (Random weights: no barrier is asserted.)"""
    import models
    from pamnet_amd import neb
    from test_pbc_axes import CUT_G, CUT_L
    initial, final, fixed0, images = _pamnet_endpoints()
    band = neb.interpolate(initial.to(dev), final.to(dev), images)
    want, band_ptr = _interpolate_ref(initial.pos.numpy(), final.pos.numpy(), initial.batch.numpy(), initial.cell.numpy(),
                                      initial.pbc.numpy(), images)
    assert band.pos.is_cuda and np.abs(band.pos.cpu().numpy().astype(np.float64) - want).max() <= 1e-6
    counts = np.bincount(initial.batch.numpy())
    graph_src = np.repeat(np.arange(3), images)
    fixed_np = np.concatenate([fixed0.numpy()[initial.batch.numpy() == g] for g in graph_src])
    fixed = torch.from_numpy(fixed_np).to(dev)
    gptr = np.concatenate([[0], np.cumsum(counts[graph_src])]).astype(np.int32)
    aptr = gptr[band_ptr]
    ends = np.zeros(len(graph_src), dtype=bool)
    ends[band_ptr[:-1]] = ends[band_ptr[1:] - 1] = True
    move_fixed = ends[np.repeat(np.arange(len(graph_src)), counts[graph_src])] | fixed_np
    torch.manual_seed(0)
    model = models.PAMNet(models.Config(dataset='QM9', dim=dim, n_layer=n_layer, cutoff_l=CUT_L, cutoff_g=CUT_G)).to(dev)
    pos0 = band.pos.clone()
    kb = torch.tensor([0.1, 0.5, 0.2], dtype=torch.float64, device=dev)
    res = neb.run(model, band, fmax=1e-7, k=kb, climb_after=5, max_steps=10, fixed=fixed, trace=True)
    assert torch.equal(band.pos, pos0) and not band.pos.requires_grad
    assert len(res.trace) == 10 and res.steps.tolist() == [10, 10, 10] and not res.converged.any() and not res.failed.any()
    assert [int(r['climb'].sum()) for r in res.trace] == [0] * 5 + [3] * 5
    assert int(res.trace[5]['state_before']['n_pos'].abs().max()) == 0 and not res.trace[5]['v_before'].any()
    mf = torch.from_numpy(move_fixed).to(dev)
    assert torch.equal(res.pos[mf], pos0[mf]) and not torch.equal(res.pos[~mf], pos0[~mf])
    worst = _replay(res, gptr, band_ptr, aptr, kb.cpu().numpy(), fixed_np, move_fixed, 1e-7, (dim, n_layer))
    print('replay: worst dneb / seg / fpar / vel / displacement', worst)
    assert torch.equal(res.trace[-1]['pos_after'], res.pos)
    d = copy.copy(band)
    d.pos = res.pos.clone().requires_grad_(True)
    e = model(d)
    de, = torch.autograd.grad(e.sum(), d.pos)
    assert torch.equal(res.energy, e.detach()) and torch.equal(res.forces, -de) and torch.isfinite(res.neb_forces).all()
    assert not res.neb_forces[mf].any() and res.saddle.tolist() == [1, int(res.saddle[1]), 8] and int(res.saddle[1]) in (4, 5)
