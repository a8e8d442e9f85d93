"""Batched structure relaxation: the FIRE step kernel pamnet_fire_step_f32 (csrc/relax.hip) and the driver pamnet_amd/relax.py.

The reference is tests/relax_ref.py fire_step_ref, the rule of include/pamnet_hip.h restated in numpy fp64.  Inputs are made once
on the CPU with fixed seeds and never modified; the conditions under which kernel and reference take the same branch (both
compute in fp64 from the same fp32 inputs) are asserted by tests that need no GPU.

Tolerances: KTOL = 1e-6 max-normalised (tests/test_hip_forces.py) for fmax, the velocities and the displacement pos_new - pos_old
(not pos, whose magnitude would hide an error), per graph; 1e-12 relative for the fp64 state dt and a; equality for the integer
state and for everything that belongs to an atom or a graph that must not move."""
import copy

import numpy as np
import pytest
import torch

from conftest import maxnorm_err
from relax_ref import STATE, fire_step_ref

ENTRY = 'pamnet_fire_step_f32'
KTOL = 1e-6
FMAX_TOL = 0.05
DEFAULTS = dict(dt_max=1.0, max_step=0.2, n_min=5, f_inc=1.1, f_dec=0.5, a0=0.1, f_a=0.99)
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 300, 1025, 0]
ROLES = ['first', 'all_fixed', 'converged', 'up_few', 'up_many', 'up_clamp', 'down', 'converging', 'failed', 'nonfinite']
SHIFTS = (0, 5, 8)                                # graph i of the batch plays ROLES[(i + shift) % 10]; the empty graph is last
MODELS = [(32, 2), (128, 1)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs an MI355X'
    from pamnet_amd import lib
    lib.load()
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------- kernel-test inputs
class Case(object):
    pass


_MADE = {}


def _kernel_case(shift):
    """One batch of SIZES.  Forces are scaled to max |f| = 1 over a graph's free atoms (0.03 where the graph is to converge):
      first      v = 0, dt = 0.1                                      -> V2 == 0, dr = 0.01: cap inactive
      up_few     v = 0.3 f + noise, n_pos = 2, dt = 0.2               -> P > 0, n_pos <= n_min, dr ~ 0.1: cap inactive
      up_many    v = 0.8 f + noise, n_pos = 5, dt = 0.5, a = 0.08     -> P > 0 past n_min, dt = 0.55, cap active
      up_clamp   v = 0.8 f + noise, n_pos = 7, dt = 0.95, a = 0.07    -> dt 1.045 clamped to dt_max = 1, cap active
      down       v = -0.4 f + noise, n_pos = 3, dt = 0.4              -> P <= 0, dt = 0.2, dr = 0.04: cap inactive
      converging max |f| = 0.03 < 0.05;   converged / failed: status 1 / 2 with velocities and gradients that must not be read;
      all_fixed  every atom fixed;   nonfinite  one gradient entry NaN (shift 0, 8) or inf (shift 5).
    A moving graph of 63 atoms or more has a fifth of its atoms fixed, with velocities that must enter no sum."""
    if shift in _MADE:
        return _MADE[shift]
    rng = np.random.RandomState(100 + shift)
    n, G = sum(SIZES), len(SIZES)
    c = Case()
    c.gptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    c.roles = [ROLES[(i + shift) % 10] for i in range(G - 1)] + ['empty']
    c.pos = rng.uniform(-4.0, 4.0, (n, 3)).astype(np.float32)
    c.vel = np.zeros((n, 3), dtype=np.float32)
    c.dE = np.zeros((n, 3), dtype=np.float32)
    c.fixed = np.zeros(n, dtype=bool)
    c.state = dict(dt=np.full(G, 0.1), a=np.full(G, 0.1), n_pos=np.zeros(G, np.int32), steps=np.zeros(G, np.int32),
                   status=np.zeros(G, np.int32), fmax=np.full(G, -1.0, np.float32))
    moving = {'first': (0.0, 0, 0.1, 0.1), 'up_few': (0.3, 2, 0.2, 0.1), 'up_many': (0.8, 5, 0.5, 0.08),
              'up_clamp': (0.8, 7, 0.95, 0.07), 'down': (-0.4, 3, 0.4, 0.09), 'nonfinite': (0.3, 2, 0.2, 0.1)}
    for g, role in enumerate(c.roles):
        lo, hi = int(c.gptr[g]), int(c.gptr[g + 1])
        m = hi - lo
        if m == 0:
            continue
        f = rng.standard_normal((m, 3))
        noise = 0.1 * rng.standard_normal((m, 3))
        fix = np.zeros(m, dtype=bool)
        if role == 'all_fixed':
            fix[:] = True
        elif role in moving and m >= 63:
            fix[rng.choice(m, m // 5, replace=False)] = True
        free = ~fix
        if free.any():
            f /= np.sqrt((f[free] ** 2).sum(1).max())
        c.fixed[lo:hi] = fix
        c.state['steps'][g] = rng.randint(0, 40)
        if role in moving:
            coef, n_pos, dt, a = moving[role]
            v = coef * f + (noise if coef else 0.0)
            v[fix] = rng.standard_normal((int(fix.sum()), 3))
            c.state['n_pos'][g], c.state['dt'][g], c.state['a'][g] = n_pos, dt, a
        else:
            v = rng.standard_normal((m, 3))
            c.state['n_pos'][g], c.state['dt'][g], c.state['a'][g] = rng.randint(0, 9), rng.uniform(0.05, 1.0), rng.uniform(0.01, 0.1)
        if role == 'converging':
            f *= 0.03
        if role in ('converged', 'failed'):
            c.state['status'][g] = 1 if role == 'converged' else 2
            c.state['fmax'][g] = 0.04 if role == 'converged' else np.inf
        c.dE[lo:hi], c.vel[lo:hi] = (-f).astype(np.float32), v.astype(np.float32)
        if role == 'nonfinite':
            a_free = lo + int(np.nonzero(free)[0][m // 2 if m > 2 else 0])
            c.dE[a_free, 1] = np.inf if shift == 5 else np.nan
    diag = {}
    c.ref = fire_step_ref(c.pos, c.vel, c.dE, c.gptr, c.state, FMAX_TOL, c.fixed, diag=diag, **DEFAULTS)
    c.diag = diag
    _MADE[shift] = c
    return c


def _margins(d, tol, max_step=DEFAULTS['max_step'], n_min=DEFAULTS['n_min'], f_inc=DEFAULTS['f_inc'], dt_max=DEFAULTS['dt_max']):
    """The conditions of one graph's step record (relax_ref diag) under which fp64 arithmetic in another order takes the same
    branch.  A graph that was left alone (None) or failed has none."""
    if d is None or not np.isfinite(d['F2']):
        return
    assert abs(d['fm'] - tol) >= 0.01 * tol, d
    if 'P' not in d:
        return
    assert d['V2'] == 0.0 or abs(d['P']) > 1e-3 * np.sqrt(d['F2'] * d['V2']), d
    assert abs(d['max_dr'] - max_step) >= 0.01 * max_step, d
    if d['V2'] != 0.0 and d['P'] > 0.0 and d['n_pos_in'] + 1 > n_min:
        assert abs(d['dt_in'] * f_inc - dt_max) >= 0.01 * dt_max, d


# ------------------------------------------------------------------------------------------------------- harmonic wells
class Harmonic(torch.nn.Module):
    """E_g = 1/2 k_g sum_{a in g} |pos_a - x0_a|^2: a plain torch module, differentiable with respect to data.pos."""

    def __init__(self, k, x0):
        super().__init__()
        self.register_buffer('k', k)
        self.register_buffer('x0', x0)

    def forward(self, data):
        r2 = (data.pos - self.x0).pow(2).sum(1)
        return 0.5 * self.k * torch.zeros_like(self.k).index_add_(0, data.batch, r2)


H_SIZES, H_K, H_TOL, H_MAX, H_SEED = (4, 9, 70), (0.5, 2.0, 6.0), 0.01, 400, 6


def _harmonic():
    """(x0, pos0, batch, fixed, k) fp32 / bool numpy, and the reference trajectory: fire_step_ref iterated on the fp64 gradient
    k_g (pos - x0) rounded to fp32, until no graph is running.  Coordinates within [-2, 2]: an fp32 position carries 1e-7."""
    if 'h' in _MADE:
        return _MADE['h']
    rng = np.random.RandomState(H_SEED)
    n, G = sum(H_SIZES), len(H_SIZES)
    h = Case()
    h.batch = np.repeat(np.arange(G), H_SIZES)
    h.gptr = np.concatenate([[0], np.cumsum(H_SIZES)]).astype(np.int32)
    h.x0 = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    h.pos0 = (h.x0 + rng.uniform(-1.0, 1.0, (n, 3))).astype(np.float32)
    h.fixed = rng.uniform(size=n) < 0.2
    h.fixed[0] = False
    h.k = np.asarray(H_K, dtype=np.float32)
    pos, vel = h.pos0.copy(), np.zeros((n, 3), np.float32)
    st = dict(dt=np.full(G, 0.1), a=np.full(G, 0.1), n_pos=np.zeros(G, np.int32), steps=np.zeros(G, np.int32),
              status=np.zeros(G, np.int32), fmax=np.zeros(G, np.float32))
    h.diags = []
    for _ in range(H_MAX):
        dE = (h.k.astype(np.float64)[h.batch, None] * (pos.astype(np.float64) - h.x0)).astype(np.float32)
        diag = {}
        pos, vel, st = fire_step_ref(pos, vel, dE, h.gptr, st, H_TOL, h.fixed, diag=diag, **DEFAULTS)
        h.diags.append(diag)
        if not (st['status'] == 0).any():
            break
    h.pos, h.state = pos, st
    _MADE['h'] = h
    return h


# ------------------------------------------------------------------------------------------------------ descent inputs
def _descent_model(dim, n_layer):
    import models
    from oracle import pamnet_oracle as O
    cfg = models.Config(dataset='QM9', dim=dim, n_layer=n_layer, cutoff_l=5.0, cutoff_g=5.0)
    return cfg, O.init_state_dict(cfg, seed=7)


def _descent_batch():
    from pamnet_amd import synth
    return synth.qm9_batch(0, 0, 3)                                # open space, bonded (edge_index), three molecules


# ---------------------------------------------------------------------------------------------------------- CPU tests
def test_header_declares_the_fire_step_at_abi_18():
    """(No GPU: the header and the built library.)"""
    import ctypes
    import re
    from pamnet_amd import build, lib
    decl = lib.declared_functions()
    assert ENTRY in decl
    P, D = ctypes.c_void_p, ctypes.c_double
    assert decl[ENTRY] == [P] * 5 + [ctypes.c_int64] * 2 + [P] * 7 + [D] * 3 + [ctypes.c_int32] + [D] * 4 + [P]
    assert int(re.search(r'#define\s+PAMNET_ABI_VERSION\s+(\d+)', open(lib.HEADER).read()).group(1)) == 18
    h = ctypes.CDLL(build.build())
    assert h.pamnet_abi_version() == 18 and hasattr(h, ENTRY)


def test_fire_step_kernel_is_scratch_free(tmp_path):
    """(No GPU: hipcc cross-compiles.)  The compiler's report for csrc/relax.hip: no scratch, a few dozen registers, the five
    fp64 partials of four wavefronts in LDS (DESIGN section 10 quotes the figures)."""
    import os
    import re
    import shutil
    import subprocess
    from pamnet_amd import build
    hipcc = '/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else shutil.which('hipcc')
    assert hipcc, 'hipcc not available'
    r = subprocess.run([hipcc] + build.FLAGS + ['-c', os.path.join(build.CSRC, 'relax.hip'), '-o', str(tmp_path / 'relax.o'),
                                                '-Rpass-analysis=kernel-resource-usage'], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = [b for b in re.split(r'remark: Function Name: ', r.stderr)[1:] if 'fire_step_kernel' in b.split()[0]]
    assert len(blocks) == 1
    num = lambda key: int(re.search(key + r': (\d+)', blocks[0]).group(1))
    assert num(r'ScratchSize \[bytes/lane\]') == 0
    assert num('VGPRs') + num('AGPRs') <= 64 and num(r'LDS Size \[bytes/block\]') <= 256


def test_the_reference_relaxes_every_harmonic_well_at_its_own_pace():
    """(No GPU; a test of the reference.)  fire_step_ref iterated on three wells of different stiffness brings every graph below
    the threshold, each after its own number of steps -- the per-graph state doing its job -- and fixed atoms stay."""
    h = _harmonic()
    assert (h.state['status'] == 1).all(), h.state
    assert (h.state['fmax'] < H_TOL).all()
    f = h.k[h.batch, None] * (h.pos.astype(np.float64) - h.x0)
    f[h.fixed] = 0.0
    assert np.sqrt((f ** 2).sum(1)).max() < H_TOL
    assert len(set(h.state['steps'].tolist())) == len(H_SIZES), h.state['steps']
    assert h.fixed.any() and np.array_equal(h.pos[h.fixed], h.pos0[h.fixed])
    assert not np.array_equal(h.pos[~h.fixed], h.pos0[~h.fixed])
    print('harmonic wells: steps', h.state['steps'], 'iterations', len(h.diags))


def test_relax_inputs_meet_their_preconditions():
    """(No GPU.)  The kernel-test batches and the whole harmonic reference trajectory keep their distance from every branch point:
    |P| > 1e-3 sqrt(F2 V2) or V2 == 0 exactly; fm 1 % away from the threshold; max |dr| 1 % away from max_step; dt f_inc 1 % away
    from dt_max where the clamp is decided.  The kernel batches together take every branch."""
    seen = set()
    for shift in SHIFTS:
        c = _kernel_case(shift)
        assert [int(b - a) for a, b in zip(c.gptr[:-1], c.gptr[1:])] == SIZES
        _, _, st = c.ref
        for g, role in enumerate(c.roles):
            d = c.diag[g]
            _margins(d, FMAX_TOL)
            m, nfix = SIZES[g], int(c.fixed[c.gptr[g]:c.gptr[g + 1]].sum())
            if role in ('converged', 'failed'):
                assert d is None and st['status'][g] == c.state['status'][g] != 0
                seen.add(role)
                continue
            if role in ('all_fixed', 'empty', 'converging'):
                assert st['status'][g] == 1 and st['steps'][g] == c.state['steps'][g]
                assert (d['fm'] == 0.0 and nfix == m) if role != 'converging' else (0.0 < d['fm'] < FMAX_TOL and nfix < m)
                seen.add(role)
                continue
            if role == 'nonfinite':
                assert st['status'][g] == 2 and not np.isfinite(st['fmax'][g])
                assert np.isnan(st['fmax'][g]) == (shift != 5)
                seen.add('nonfinite')
                continue
            assert st['status'][g] == 0 and st['steps'][g] == c.state['steps'][g] + 1
            capped = d['max_dr'] > DEFAULTS['max_step']
            if role == 'first':
                assert d['V2'] == 0.0 and st['n_pos'][g] == 0 and not capped
            elif role == 'up_few':
                assert d['P'] > 0 and st['n_pos'][g] == 3 and st['dt'][g] == c.state['dt'][g] and not capped
            elif role == 'up_many':
                assert d['P'] > 0 and st['n_pos'][g] == 6 and st['dt'][g] == c.state['dt'][g] * 1.1 < 1.0 and capped
                assert st['a'][g] == c.state['a'][g] * 0.99
            elif role == 'up_clamp':
                assert d['P'] > 0 and st['n_pos'][g] == 8 and st['dt'][g] == 1.0 < c.state['dt'][g] * 1.1 and capped
            else:
                assert role == 'down' and d['P'] < 0 and st['n_pos'][g] == 0 and st['a'][g] == 0.1 and not capped
                assert st['dt'][g] == c.state['dt'][g] * 0.5
            seen.update([role, 'capped' if capped else 'free', 'some_fixed' if nfix else 'none_fixed'])
    assert seen == set(ROLES) | {'empty', 'capped', 'free', 'some_fixed', 'none_fixed'}, seen
    h = _harmonic()
    branches = set()
    for diag in h.diags:
        for g, d in diag.items():
            _margins(d, H_TOL)
            if d is not None and 'P' in d:
                branches.add('first' if d['V2'] == 0.0 else 'up' if d['P'] > 0 else 'down')
                branches.add('capped' if d['max_dr'] > DEFAULTS['max_step'] else 'free')
    assert branches == {'first', 'up', 'down', 'capped', 'free'}, branches


def test_relax_refusals():
    """(No GPU.)  A PAMNet that keeps its positions in x, a batch without pos or batch, an unknown FIRE parameter, and CPU tensors
    (RuntimeError: no CPU path) are refused before anything runs."""
    import models
    from pamnet_amd import synth
    from pamnet_amd.relax import relax
    h = _harmonic()
    model = Harmonic(torch.from_numpy(h.k), torch.from_numpy(h.x0))
    data = synth.Batch(pos=torch.from_numpy(h.pos0), batch=torch.from_numpy(h.batch), num_graphs=len(H_SIZES))
    pdb = models.PAMNet(models.Config(dataset='PDBbind', dim=16, n_layer=1, cutoff_l=2.0, cutoff_g=6.0))
    with pytest.raises(ValueError, match=r'x\[:, :3\]'):
        relax(pdb, data)
    with pytest.raises(ValueError, match='no `pos`'):
        relax(model, synth.Batch(batch=data.batch, num_graphs=3))
    with pytest.raises(ValueError, match='no `batch`'):
        relax(model, synth.Batch(pos=data.pos, num_graphs=3))
    with pytest.raises(TypeError, match='dt_min'):
        relax(model, data, dt_min=0.01)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        relax(model, data)
    assert torch.equal(data.pos, torch.from_numpy(h.pos0))


def _oracle_descent(dim, n_layer, steps=20):
    """fire_step_ref over the fp64 oracle's forces from _descent_batch(): (E_initial, E_final, closest pair on the way)."""
    from oracle import pamnet_oracle as O
    cfg, sd = _descent_model(dim, n_layer)
    p = O.as_params({k: v.detach().double() for k, v in sd.items()})
    b = _descent_batch()
    G = int(b.num_graphs)
    gptr = np.concatenate([[0], np.cumsum(np.bincount(b.batch.numpy(), minlength=G))])

    def evaluate(pos32):
        leaf = torch.from_numpy(pos32).double().requires_grad_(True)
        out = O.pamnet_forward(p, cfg, b.x, b.batch, leaf, b.edge_index, dtype=torch.float64)
        g, = torch.autograd.grad(out.sum(), leaf)
        return out.detach().numpy().reshape(-1), g.numpy().astype(np.float32)

    pos, vel = b.pos.numpy().copy(), np.zeros((b.pos.size(0), 3), np.float32)
    st = dict(dt=np.full(G, 0.1), a=np.full(G, 0.1), n_pos=np.zeros(G, np.int32), steps=np.zeros(G, np.int32),
              status=np.zeros(G, np.int32), fmax=np.zeros(G, np.float32))
    e0, dE = evaluate(pos)
    closest = np.inf
    for _ in range(steps):
        pos, vel, st = fire_step_ref(pos, vel, dE, gptr, st, 1e-9, **DEFAULTS)
        e, dE = evaluate(pos)
        for g in range(G):
            q = pos[gptr[g]:gptr[g + 1]].astype(np.float64)
            d = np.sqrt(((q[:, None] - q[None]) ** 2).sum(-1))
            closest = min(closest, float(d[~np.eye(len(q), dtype=bool)].min()))
    assert (st['steps'] == steps).all()
    return e0, e, closest


@pytest.mark.parametrize('dim,n_layer', MODELS)
def test_the_descent_batch_goes_downhill_under_the_oracle(dim, n_layer):
    """(No GPU.)  The batch of the GPU descent test, chosen here: 20 FIRE steps on the fp64 oracle's forces lower every graph's
    oracle energy by more than 100 x the 1e-5 parity tolerance of its magnitude, and no pair comes closer than 0.7 A."""
    e0, e, closest = _oracle_descent(dim, n_layer)
    print('oracle energies', e0, '->', e, 'relative drop', (e0 - e) / np.abs(e0), 'closest pair', closest)
    assert ((e0 - e) > 100 * 1e-5 * np.abs(e0)).all()
    assert closest >= 0.7


# ------------------------------------------------------------------------------------------------------- kernel tests
def _step_on_device(dev, c, lo=0, hi=None, graphs=None):
    """One launch on the atoms [lo, hi) / graphs `graphs` (a slice) of a case -> (pos, vel, state) as numpy."""
    from pamnet_amd import relax as R
    graphs = slice(0, len(c.gptr) - 1) if graphs is None else graphs
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pos, vel, dE, fixed = t(c.pos[lo:hi]), t(c.vel[lo:hi]), t(c.dE[lo:hi]), t(c.fixed[lo:hi].astype(np.uint8))
    gptr = t(c.gptr[graphs.start:graphs.stop + 1] - lo)
    state = {k: t(c.state[k][graphs]) for k in STATE}
    R.fire_step(pos, vel, dE, gptr, state, FMAX_TOL, fixed, **DEFAULTS)
    return pos.cpu().numpy(), vel.cpu().numpy(), {k: v.cpu().numpy() for k, v in state.items()}


def _assert_step_matches(got, want, before, gptr, fixed, tag=''):
    """got / want / before: (pos, vel, state); the checks of one step against fire_step_ref."""
    (gp, gv, gs), (wp, wv, ws), (bp, bv, bs) = got, want, before
    for k in ('status', 'n_pos', 'steps'):
        assert np.array_equal(gs[k], ws[k]), (tag, k, gs[k], ws[k])
    for k in ('dt', 'a'):
        assert np.all(np.abs(gs[k] - ws[k]) <= 1e-12 * np.abs(ws[k])), (tag, k, gs[k], ws[k])
    finite = np.isfinite(ws['fmax'])
    assert np.array_equal(np.isnan(gs['fmax']), np.isnan(ws['fmax'])) and np.array_equal(np.isinf(gs['fmax']), np.isinf(ws['fmax']))
    assert np.all(np.abs(gs['fmax'][finite].astype(np.float64) - ws['fmax'][finite]) <= KTOL * ws['fmax'][finite]), (tag, 'fmax')
    worst = [0.0, 0.0]
    for g in range(len(gptr) - 1):
        s = slice(int(gptr[g]), int(gptr[g + 1]))
        moved = bs['status'][g] == 0 and ws['status'][g] == 0
        if not moved:                             # finished before, or converged / failed in this step: nothing of g changed
            assert np.array_equal(gp[s], bp[s]) and np.array_equal(gv[s], bv[s]), (tag, g)
            for k in ('dt', 'a', 'n_pos', 'steps'):
                assert gs[k][g] == bs[k][g], (tag, g, k)
            if bs['status'][g] != 0:
                assert gs['fmax'][g] == bs['fmax'][g] or (np.isnan(gs['fmax'][g]) and np.isnan(bs['fmax'][g]))
            continue
        if s.stop == s.start:
            continue
        fx = fixed[s]
        assert np.array_equal(gp[s][fx], bp[s][fx]) and np.array_equal(gv[s][fx], bv[s][fx]), (tag, g, 'fixed rows')
        ev = maxnorm_err(gv[s], wv[s])
        ed = maxnorm_err(gp[s].astype(np.float64) - bp[s], wp[s].astype(np.float64) - bp[s])
        assert float(np.abs(wp[s].astype(np.float64) - bp[s]).max()) > 0
        worst = [max(worst[0], ev), max(worst[1], ed)]
        assert ev <= KTOL and ed <= KTOL, (tag, g, ev, ed)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize('shift', SHIFTS)
def test_one_step_on_a_batch_vs_the_reference(dev, shift):
    """Graphs of 1, 2, 63, 64, 65, 255, 256, 257, 300, 1025 and 0 atoms whose prepared states take every branch (_kernel_case; the
    shift moves the branches over the sizes): status, n_pos, steps equal; dt, a to 1e-12; fmax, vel and the displacement within
    KTOL per graph; rows of fixed atoms, of finished graphs and of the graph that fails torch.equal to the inputs."""
    c = _kernel_case(shift)
    got = _step_on_device(dev, c)
    worst = _assert_step_matches(got, c.ref, (c.pos, c.vel, c.state), c.gptr, c.fixed, tag=shift)
    print('shift', shift, 'worst vel / displacement error', worst)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()


@pytest.mark.gpu
def test_a_step_is_repeatable_and_independent_of_the_batch(dev):
    """Two runs on the same inputs are equal bit for bit, and every graph stepped alone -- its atoms and its state as a batch of
    one -- gives the rows and the state of the batched call."""
    c = _kernel_case(5)
    p1, v1, s1 = _step_on_device(dev, c)
    p2, v2, s2 = _step_on_device(dev, c)
    assert np.array_equal(p1, p2) and np.array_equal(v1, v2)
    assert all(np.array_equal(s1[k], s2[k], equal_nan=True) for k in STATE)
    for g in range(len(SIZES)):
        lo, hi = int(c.gptr[g]), int(c.gptr[g + 1])
        p, v, s = _step_on_device(dev, c, lo, hi, slice(g, g + 1))
        assert np.array_equal(p, p1[lo:hi]) and np.array_equal(v, v1[lo:hi]), g
        assert all(np.array_equal(s[k], s1[k][g:g + 1], equal_nan=True) for k in STATE), g


@pytest.mark.gpu
def test_the_entry_point_validates_its_arguments(dev):
    """A null required pointer is PAMNET_ENULL, a bad count or parameter PAMNET_EINVAL; `fixed` and the per-graph threshold
    may be null; a per-graph threshold replaces the scalar."""
    from pamnet_amd import lib, relax as R
    c = _kernel_case(0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pos, vel, dE, gptr = t(c.pos), t(c.vel), t(c.dE), t(c.gptr)
    st = {k: t(c.state[k]) for k in STATE}
    G, n = len(SIZES), pos.size(0)

    def call(**kw):
        a = dict(pos=lib.ptr(pos), vel=lib.ptr(vel), dpos=lib.ptr(dE), fixed=None, gptr=lib.ptr(gptr), n=n, G=G, fmax_tol_g=None,
                 fmax_tol=1e9, dt_max=1.0, max_step=0.2, n_min=5, f_inc=1.1, f_dec=0.5, a0=0.1, f_a=0.99)
        a.update({k: lib.ptr(st[k]) for k in STATE})
        a.update(kw)
        lib.call(ENTRY, a['pos'], a['vel'], a['dpos'], a['fixed'], a['gptr'], a['n'], a['G'], a['dt'], a['a'], a['n_pos'],
                 a['steps'], a['status'], a['fmax'], a['fmax_tol_g'], a['fmax_tol'], a['dt_max'], a['max_step'], a['n_min'],
                 a['f_inc'], a['f_dec'], a['a0'], a['f_a'], lib.stream_of(pos))

    for k in ('pos', 'vel', 'dpos', 'gptr') + STATE:
        with pytest.raises(RuntimeError, match='PAMNET_ENULL'):
            call(**{k: None})
    for kw in (dict(n=-1), dict(G=-1), dict(n_min=-1), dict(dt_max=0.0), dict(max_step=-0.2), dict(f_inc=float('inf')),
               dict(f_dec=float('nan')), dict(a0=0.0), dict(f_a=-1.0), dict(fmax_tol=float('nan'))):
        with pytest.raises(RuntimeError, match='PAMNET_EINVAL'):
            call(**kw)
    call(G=0)
    torch.cuda.synchronize()
    assert torch.equal(pos, t(c.pos)) and torch.equal(vel, t(c.vel)) and all(torch.equal(st[k], t(c.state[k])) or k == 'fmax'
                                                                              for k in STATE)
    # a threshold of 1e9 converges every running graph whose gradient is finite; per graph: only those it is handed to
    tol_g = torch.full((G,), 1e9, device=dev)
    tol_g[3] = 1e-9
    call(fmax_tol_g=lib.ptr(tol_g), fmax_tol=1e-9)
    status = st['status'].cpu().numpy()
    roles = np.array(c.roles)
    assert status[3] == 0 and roles[3] == 'up_few'
    assert (status[roles == 'failed'] == 2).all() and (status[roles == 'nonfinite'] == 2).all()
    assert (status[~np.isin(roles, ['failed', 'nonfinite']) & (np.arange(G) != 3)] == 1).all()


# ----------------------------------------------------------------------------------------------------- end to end
@pytest.mark.gpu
def test_harmonic_wells_relax_as_the_reference_does(dev):
    """A plain torch module, three wells, some atoms fixed: per-graph steps and converged equal the reference's (whose margins the
    CPU test asserts for the whole trajectory), the final positions agree to 1e-5 of the initial displacement, fixed atoms and
    the caller's positions stay; and, where torch can police synchronisation, check_every=0 enqueues without one."""
    from pamnet_amd import synth
    from pamnet_amd.relax import relax
    h = _harmonic()
    model = Harmonic(torch.from_numpy(h.k), torch.from_numpy(h.x0)).to(dev)
    data = synth.Batch(pos=torch.from_numpy(h.pos0), batch=torch.from_numpy(h.batch), num_graphs=len(H_SIZES)).to(dev)
    fixed = torch.from_numpy(h.fixed).to(dev)
    res = relax(model, data, fmax=H_TOL, max_steps=H_MAX, fixed=fixed, check_every=10)
    assert res.trace is None and res.pos is not data.pos and torch.equal(data.pos.cpu(), torch.from_numpy(h.pos0))
    assert np.array_equal(res.steps.cpu().numpy(), h.state['steps']), (res.steps, h.state['steps'])
    assert res.converged.dtype == torch.bool and res.converged.all() and not res.failed.any()
    assert np.array_equal(res.converged.cpu().numpy(), h.state['status'] == 1)
    scale = float(np.sqrt(((h.pos0.astype(np.float64) - h.x0) ** 2).sum(1)).max())
    err = float(np.abs(res.pos.cpu().numpy().astype(np.float64) - h.pos).max())
    print('harmonic wells: max |pos - reference|', err, 'initial displacement', scale)
    assert err <= 1e-5 * scale
    assert torch.equal(res.pos[fixed], data.pos[fixed])
    assert (res.fmax < H_TOL).all() and maxnorm_err(res.fmax.cpu().numpy(), h.state['fmax']) <= 1e-5
    with torch.no_grad():
        d = copy.copy(data)
        d.pos = res.pos
        assert torch.allclose(res.energy, model(d), rtol=1e-5, atol=0.0)       # (index_add_ adds in no fixed order)
    assert torch.equal(res.forces, -model.k[data.batch, None] * (res.pos - model.x0))
    # per-graph thresholds: a graph handed a looser one stops earlier, the others as before
    tol_g = torch.tensor([H_TOL, 10 * H_TOL, H_TOL], device=dev)
    res_g = relax(model, data, fmax=tol_g, max_steps=H_MAX, fixed=fixed)
    sg, s0 = res_g.steps.cpu().numpy(), h.state['steps']
    assert sg[0] == s0[0] and sg[2] == s0[2] and sg[1] < s0[1] and res_g.converged.all()
    for kw in (dict(fixed=h.fixed), dict(fixed=h.fixed.tolist()), dict(fixed=fixed.float()), dict(fixed=fixed[:-1]),
               dict(fixed=fixed.cpu()), dict(fmax=[H_TOL] * 3), dict(fmax=tol_g.double()), dict(fmax=tol_g[:2])):
        with pytest.raises(ValueError, match='`fixed` is a torch.bool tensor' if 'fixed' in kw else '`fmax`'):
            relax(model, data, **kw)
    try:
        torch.cuda.set_sync_debug_mode('error')
    except Exception as e:                        # (a build without the debug mode: the rest of the test has run)
        print('set_sync_debug_mode is not available:', e)
        return
    try:
        res0 = relax(model, data, fmax=H_TOL, max_steps=12, fixed=fixed, check_every=0)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert res0.pos.is_cuda and int(res0.steps.max()) == 12


def _pamnet_batch():
    """[a bond-free molecule in open space (zero cell, pbc all False), 24 atoms in the triclinic cell TRI_A, the slab slab_min of
    tests/test_pbc_axes.py with pbc = (True, True, False)], and the slab's bottom layer (the third of its atoms lowest along the
    open axis) as the fixed mask."""
    if 'pamnet' in _MADE:
        return _MADE['pamnet']
    from test_pbc_axes import TRI_A, Struct, _batch, _scatter, _structs
    rng = np.random.RandomState(5)
    zero, none = np.zeros((3, 3)), (False, False, False)
    span = {0: (0.0, 5.0), 1: (0.0, 5.0), 2: (0.0, 5.0)}
    mol = Struct(rng.randint(0, 5, 12).astype(np.float32), _scatter(rng, 12, zero, none, span, 0).astype(np.float32), zero, none, 0)
    tri = Struct(rng.randint(0, 5, 24).astype(np.float32), _scatter(rng, 24, TRI_A, (True, True, True), {}, 2).astype(np.float32),
                 TRI_A, (True, True, True), 2)
    slab = _structs()['slab_min']
    b = _batch([mol, tri, slab])
    z = slab.pos[:, 2]
    fixed = np.zeros(b.pos.size(0), dtype=bool)
    fixed[mol.n + tri.n:] = z <= np.sort(z)[slab.n // 3 - 1]
    assert b.pbc.tolist() == [[False] * 3, [True] * 3, [True, True, False]] and int(fixed.sum()) == slab.n // 3
    _MADE['pamnet'] = (b, torch.from_numpy(fixed))
    return _MADE['pamnet']


@pytest.mark.gpu
@pytest.mark.parametrize('dim,n_layer', MODELS)
def test_pamnet_relaxation_replayed_step_by_step(dev, dim, n_layer):
    """PAMNet on {bond-free molecule, triclinic cell, slab with a fixed bottom layer}, trace=True, 8 steps: every recorded step,
    replayed alone through fire_step_ref from its recorded inputs, matches as in the kernel test; a fresh model call at a recorded
    geometry reproduces the recorded gradient bitwise; res.energy / res.forces are bitwise a fresh evaluation at res.pos; fixed
    rows, the caller's positions and every parameter .grad are as they were."""
    import models
    from pamnet_amd.relax import relax
    from test_pbc_axes import CUT_G, CUT_L
    b, fixed_cpu = _pamnet_batch()
    torch.manual_seed(0)
    model = models.PAMNet(models.Config(dataset='QM9', dim=dim, n_layer=n_layer, cutoff_l=CUT_L, cutoff_g=CUT_G)).to(dev)
    data, fixed = b.to(dev), fixed_cpu.to(dev)
    model(data).sum().backward()                                   # parameter gradients to find untouched afterwards
    snap = [None if p.grad is None else p.grad.clone() for p in model.parameters()]
    assert sum(s is not None for s in snap) > 10
    pos0 = data.pos.clone()
    res = relax(model, data, fmax=1e-6, max_steps=8, fixed=fixed, trace=True)
    assert torch.equal(data.pos, pos0) and not data.pos.requires_grad
    for p, s in zip(model.parameters(), snap):
        assert (p.grad is None) if s is None else torch.equal(p.grad, s)
    assert len(res.trace) == 8 and res.steps.tolist() == [8, 8, 8] and not res.converged.any() and not res.failed.any()
    assert torch.equal(res.pos[fixed], pos0[fixed]) and not torch.equal(res.pos[~fixed], pos0[~fixed])
    gptr = np.concatenate([[0], np.cumsum(np.bincount(b.batch.numpy(), minlength=3))])
    cpu = lambda t: t.cpu().numpy()
    worst = [0.0, 0.0]
    for i, r in enumerate(res.trace):
        before = (cpu(r['pos']), cpu(r['v_before']), {k: cpu(v) for k, v in r['state_before'].items()})
        got = (cpu(r['pos_after']), cpu(r['v_after']), {k: cpu(v) for k, v in r['state_after'].items()})
        want = fire_step_ref(before[0], before[1], cpu(r['dE']), gptr, before[2], 1e-6, fixed_cpu.numpy(), **DEFAULTS)
        w = _assert_step_matches(got, want, before, gptr, fixed_cpu.numpy(), tag=i)
        worst = [max(worst[0], w[0]), max(worst[1], w[1])]
        if i + 1 < len(res.trace):
            assert torch.equal(r['pos_after'], res.trace[i + 1]['pos']) and torch.equal(r['v_after'], res.trace[i + 1]['v_before'])
    print('replay: worst vel / displacement error', worst)
    assert torch.equal(res.trace[-1]['pos_after'], res.pos)

    def fresh(pos):
        d = copy.copy(data)
        d.pos = pos.clone().requires_grad_(True)
        e = model(d)
        return e.detach(), torch.autograd.grad(e.sum(), d.pos)[0]

    assert torch.equal(fresh(res.trace[3]['pos'])[1], res.trace[3]['dE'])
    e, de = fresh(res.pos)
    assert torch.equal(res.energy, e) and torch.equal(res.forces, -de) and torch.isfinite(res.forces).all()


@pytest.mark.gpu
@pytest.mark.parametrize('dim,n_layer', MODELS)
def test_relaxation_lowers_the_energy_of_every_molecule(dev, dim, n_layer):
    """The bonded open-space batch the CPU test chose: after 20 steps every graph's energy is below its initial one."""
    import models
    from pamnet_amd.relax import relax
    cfg, sd = _descent_model(dim, n_layer)
    model = models.PAMNet(cfg)
    model.load_state_dict(sd, strict=True)
    model = model.to(dev)
    data = _descent_batch().to(dev)
    with torch.no_grad():
        e0 = model(data)
    res = relax(model, data, fmax=1e-9, max_steps=20)
    print('energies', e0.tolist(), '->', res.energy.tolist())
    assert res.steps.tolist() == [20, 20, 20]
    assert (res.energy < e0).all()


@pytest.mark.gpu
@pytest.mark.parametrize('dim,n_layer', MODELS)
def test_a_store_batch_is_relaxed_without_its_stale_sizes(dev, dim, n_layer):
    """A MoleculeStore batch carries `sizes`, the host-side edge counts of the STORED geometry, which the forward trusts without
    a read-back.  The driver evaluates its moved copies without them: after a relaxation in which atoms cross cutoff_g (asserted:
    the global edge count at res.pos is no longer the stored one) the model's deferred checks are clean and none is pending,
    res.energy / res.forces are bitwise a plain-tensor evaluation at res.pos, and the caller's batch keeps its sizes."""
    import models
    from pamnet_amd import graph as G, store as S, synth
    from pamnet_amd.relax import relax
    torch.manual_seed(0)
    model = models.PAMNet(models.Config(dataset='QM9', dim=dim, n_layer=n_layer, cutoff_l=5.0, cutoff_g=5.0)).to(dev)
    mols = [synth.qm9_molecule(3, i) for i in range(12)]
    st = S.MoleculeStore(mols, dev).prepare_for(model)
    idx = list(range(12))
    b = st.collate(idx)
    key = S.size_key(model)
    sizes = dict(b.sizes)
    assert b.sizes.get(key) is not None
    with torch.no_grad():
        model(b)                                                   # the stored geometry: its sizes are right
    model.verify()
    res = relax(model, b, fmax=1e-9, max_steps=15, dt0=0.5, dt_max=1.5)
    assert b.sizes == sizes and res.steps.tolist() == [15] * 12 and torch.isfinite(res.energy).all()
    model.verify()                                                 # nothing was flagged on the way ...
    assert not model._pending_checks                               # ... and nothing waits
    plain = synth.collate(mols).to(dev)
    assert torch.equal(plain.pos, b.pos)
    g = G.build_graph('QM9', 5.0, 5.0, 'source_to_target', plain.x, plain.batch, res.pos, plain.edge_index, num_graphs=12,
                      need_grad=False, n_types=5)
    print('global edges: stored geometry', b.sizes[key][0], 'relaxed geometry', g.glob.m)
    assert g.glob.m != b.sizes[key][0]                             # the stored counts no longer describe the geometry
    plain.pos = res.pos.clone().requires_grad_(True)
    e = model(plain)
    de, = torch.autograd.grad(e.sum(), plain.pos)
    assert torch.equal(res.energy, e.detach()) and torch.equal(res.forces, -de)
