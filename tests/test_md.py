"""Batched molecular dynamics: the kernels pamnet_md_step_f32 / pamnet_md_init_velocities_f32 (csrc/md.hip) and the driver
pamnet_amd/md.py.

The reference is tests/md_ref.py: the Philox4x32-10 generator, md_step_ref and init_velocities_ref, the rules of
include/pamnet_hip.h restated in numpy fp64.  Inputs are made once on the CPU with fixed seeds and never modified; what the
end-to-end tests presuppose of the reference is asserted by tests that need no GPU.

Tolerances: KTOL = 1e-6 max-normalised (tests/test_hip_forces.py) per graph for the velocities and the displacement
pos_new - pos_old (not pos, whose magnitude would hide an error); 1e-12 relative for the fp64 kinetic energy; equality for steps,
status and everything that belongs to an atom or a graph that must not move."""
import copy
import warnings

import numpy as np
import pytest
import torch

from conftest import maxnorm_err
from md_ref import STATE, init_velocities_ref, md_step_ref, normals, philox4x32

STEP, INIT = 'pamnet_md_step_f32', 'pamnet_md_init_velocities_f32'
KTOL = 1e-6
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 300, 1025, 0]          # (tests/test_relax.py SIZES)
ROLES = ['nve', 'langevin', 'strong', 'kt0', 'all_fixed', 'failed', 'nan', 'inf', 'vinf']
SHIFTS = (0, 4, 7)                                # graph i of the batch plays ROLES[(i + shift) % 9]; the empty graph is last
FLAGS = ((0, 1), (1, 1), (1, 0), (0, 0))          # (kick_in, advance)
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


def _gptr(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


# ------------------------------------------------------------------------------------------------- kernel-test inputs
def _kernel_case(shift):
    """One batch of SIZES with per-graph dt in [0.02, 0.1], masses in [1, 40], steps in [0, 40), seeds over all of int64:
      nve        gamma = 0 (kT = 0.7 must not matter)        langevin   gamma = 2, kT = 0.7
      strong     gamma dt = 20: c1 = 2e-9                    kt0        gamma = 2, kT = 0
      all_fixed  every atom fixed                            failed     status 2, with velocities and gradients not to be read
      nan / inf  one gradient entry of a free atom           vinf       one velocity entry of a free atom infinite
    A graph of 63 atoms or more has a fifth of its atoms fixed, with velocities that must enter no sum."""
    if shift in _MADE:
        return _MADE[shift]
    rng = np.random.RandomState(200 + shift)
    n, G = sum(SIZES), len(SIZES)
    c = Case()
    c.gptr = _gptr(SIZES)
    c.roles = [ROLES[(i + shift) % len(ROLES)] for i in range(G - 1)] + ['empty']
    c.pos = rng.uniform(-4.0, 4.0, (n, 3)).astype(np.float32)
    c.vel = rng.standard_normal((n, 3)).astype(np.float32)
    c.dE = rng.standard_normal((n, 3)).astype(np.float32)
    c.mass = rng.uniform(1.0, 40.0, n).astype(np.float32)
    c.fixed = np.zeros(n, dtype=bool)
    c.dt = rng.uniform(0.02, 0.1, G)
    c.kT, c.gamma = np.full(G, 0.7), np.full(G, 2.0)
    c.state = dict(seed=rng.randint(-2 ** 63, 2 ** 63 - 1, G, dtype=np.int64), steps=rng.randint(0, 40, G).astype(np.int32),
                   status=np.zeros(G, np.int32), ke=np.full(G, -1.0))
    for g, role in enumerate(c.roles):
        lo, hi = int(c.gptr[g]), int(c.gptr[g + 1])
        m = hi - lo
        if m == 0:
            continue
        if role == 'all_fixed':
            c.fixed[lo:hi] = True
        elif m >= 63:
            c.fixed[lo + rng.choice(m, m // 5, replace=False)] = True
        free = lo + np.nonzero(~c.fixed[lo:hi])[0]
        if role == 'nve':
            c.gamma[g] = 0.0
        elif role == 'strong':
            c.gamma[g] = 20.0 / c.dt[g]
        elif role == 'kt0':
            c.kT[g] = 0.0
        elif role == 'failed':
            c.state['status'][g] = 2
            c.vel[lo, 0], c.dE[hi - 1, 2] = np.nan, np.inf
        elif role in ('nan', 'inf'):
            c.dE[free[len(free) // 2], 1] = np.nan if role == 'nan' else np.inf
        elif role == 'vinf':
            c.vel[free[len(free) // 2], 2] = -np.inf
    _MADE[shift] = c
    return c


def _ref(c, kick_in, advance, mass=True):
    key = ('ref', id(c), kick_in, advance, mass)
    if key not in _MADE:
        _MADE[key] = md_step_ref(c.pos, c.vel, c.dE, c.gptr, c.state, c.dt, c.kT, c.gamma, c.mass if mass else None, c.fixed,
                                 kick_in, advance)
    return _MADE[key]


def _indep_graphs():
    """One Langevin graph per size of SIZES, each with its own atoms, seed, step counter, dt, kT and gamma: the pieces of the
    batches of the independence test."""
    if 'indep' in _MADE:
        return _MADE['indep']
    rng = np.random.RandomState(31)
    out = []
    for m in SIZES:
        fixed = np.zeros(m, dtype=bool)
        if m >= 63:
            fixed[rng.choice(m, m // 5, replace=False)] = True
        out.append(dict(pos=rng.uniform(-4.0, 4.0, (m, 3)).astype(np.float32), vel=rng.standard_normal((m, 3)).astype(np.float32),
                        dE=rng.standard_normal((m, 3)).astype(np.float32), mass=rng.uniform(1.0, 40.0, m).astype(np.float32),
                        fixed=fixed, dt=rng.uniform(0.02, 0.1), kT=rng.uniform(0.1, 1.0), gamma=rng.uniform(0.5, 4.0),
                        seed=int(rng.randint(-2 ** 63, 2 ** 63 - 1, dtype=np.int64)), steps=int(rng.randint(0, 40))))
    _MADE['indep'] = out
    return out


def _assemble(graphs):
    """A Case from a list of graph records (_indep_graphs), in the order given."""
    c = Case()
    c.gptr = _gptr([len(g['pos']) for g in graphs])
    cat = lambda k, shape, dt: np.concatenate([g[k] for g in graphs]).reshape(shape).astype(dt) if graphs else np.zeros(shape, dt)
    c.pos, c.vel, c.dE = cat('pos', (-1, 3), np.float32), cat('vel', (-1, 3), np.float32), cat('dE', (-1, 3), np.float32)
    c.mass, c.fixed = cat('mass', (-1,), np.float32), cat('fixed', (-1,), bool)
    c.dt, c.kT, c.gamma = (np.array([g[k] for g in graphs], dtype=np.float64) for k in ('dt', 'kT', 'gamma'))
    G = len(graphs)
    c.state = dict(seed=np.array([g['seed'] for g in graphs], dtype=np.int64),
                   steps=np.array([g['steps'] for g in graphs], dtype=np.int32), status=np.zeros(G, np.int32), ke=np.zeros(G))
    return c


# ------------------------------------------------------------------------------------------------------- harmonic wells
class Harmonic(torch.nn.Module):
    """E_g = 1/2 k_g sum_{a in g} |pos_a - x0_a|^2: a plain torch module, differentiable with respect to data.pos (as in
    tests/test_relax.py)."""

    def __init__(self, k, x0):
        super().__init__()
        self.register_buffer('k', k)
        self.register_buffer('x0', x0)

    def forward(self, data):
        r2 = (data.pos - self.x0).pow(2).sum(1)
        return 0.5 * self.k * torch.zeros_like(self.k).index_add_(0, data.batch, r2)


H_DT = 0.05
NVE = dict(sizes=(4, 9, 70), k=(0.5, 2.0, 6.0), steps=400, seed=6, kT=0.0, gamma=0.0, spread=1.0, fix=0.2)
LAN = dict(sizes=(512,), k=(2.0,), steps=300, seed=2, kT=0.7, gamma=2.0, spread=0.0, fix=0.0)


def _harmonic(name, spec):
    """(x0, pos0, batch, mass, fixed, k) and the reference trajectory from rest: md_step_ref iterated on the fp64 gradient
    k_g (pos - x0) rounded to fp32, launch by launch as the driver does -- (0, 1), then (1, 1), and a closing (1, 0) -- with the
    records epot / ekin [steps + 1, G] taken at the full steps."""
    if name in _MADE:
        return _MADE[name]
    rng = np.random.RandomState(spec['seed'])
    sizes = spec['sizes']
    n, G = sum(sizes), len(sizes)
    h = Case()
    h.batch, h.gptr = np.repeat(np.arange(G), sizes), _gptr(sizes)
    h.x0 = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    h.pos0 = (h.x0 + spec['spread'] * rng.uniform(-1.0, 1.0, (n, 3))).astype(np.float32)
    h.mass = rng.uniform(1.0, 40.0, n).astype(np.float32)
    h.fixed = rng.uniform(size=n) < spec['fix']
    h.fixed[0] = False
    h.k = np.asarray(spec['k'], dtype=np.float32)
    h.seeds = spec['seed'] + np.arange(G, dtype=np.int64)
    kk = h.k.astype(np.float64)[h.batch, None]
    pos, vel = h.pos0.copy(), np.zeros((n, 3), np.float32)
    st = dict(seed=h.seeds, steps=np.zeros(G, np.int32), status=np.zeros(G, np.int32), ke=np.zeros(G))
    h.epot, h.ekin = np.zeros((spec['steps'] + 1, G)), np.zeros((spec['steps'] + 1, G))
    for it in range(spec['steps'] + 1):
        d = pos.astype(np.float64) - h.x0
        h.epot[it] = np.bincount(h.batch, weights=0.5 * (kk * d * d).sum(1), minlength=G)
        pos, vel, st = md_step_ref(pos, vel, (kk * d).astype(np.float32), h.gptr, st, H_DT, spec['kT'], spec['gamma'], h.mass,
                                   h.fixed, 1 if it else 0, 1 if it < spec['steps'] else 0)
        h.ekin[it] = st['ke']
    h.pos, h.vel, h.state = pos, vel, st
    _MADE[name] = h
    return h


def _shadow_bound(h, e0):
    """E0 h / (1 - h) + 1e-4 E0 per graph, h = max over the free atoms (k_g / m_a) dt^2 / 4: velocity Verlet conserves a shadow
    energy of a harmonic well that differs from the energy by a factor within 1 +- h exactly; the second term covers 400 fp32
    roundings of pos at 6e-8 each with two orders of margin."""
    hh = np.array([((h.k[g] / h.mass[(h.batch == g) & ~h.fixed].astype(np.float64)) * H_DT ** 2 / 4).max() for g in range(len(h.k))])
    return e0 * hh / (1.0 - hh) + 1e-4 * e0


# ---------------------------------------------------------------------------------------------------------- CPU tests
def test_header_declares_the_md_entry_points_at_abi_18():
    """(No GPU: the header and the built library.)"""
    import ctypes
    import re
    from pamnet_amd import build, lib
    decl = lib.declared_functions()
    P, D, I64, I32 = ctypes.c_void_p, ctypes.c_double, ctypes.c_int64, ctypes.c_int32
    assert decl[STEP] == [P] * 6 + [I64] * 2 + [P] * 7 + [D] * 3 + [I32] * 2 + [P]
    assert decl[INIT] == [P] * 4 + [I64] * 2 + [P] * 2 + [D] + [I32] * 2 + [P] * 2
    assert int(re.search(r'#define\s+PAMNET_ABI_VERSION\s+(\d+)', open(lib.HEADER).read()).group(1)) == 18
    h = ctypes.CDLL(build.build())
    assert h.pamnet_abi_version() == 18 and hasattr(h, STEP) and hasattr(h, INIT)


def test_md_kernels_are_scratch_free(tmp_path):
    """(No GPU: hipcc cross-compiles.)  The compiler's report for csrc/md.hip: neither kernel uses scratch (DESIGN section 11
    quotes the figures)."""
    import os
    import re
    import shutil
    import subprocess
    from pamnet_amd import build
    hipcc = '/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else shutil.which('hipcc')
    assert hipcc, 'hipcc not available'
    r = subprocess.run([hipcc] + build.FLAGS + ['-c', os.path.join(build.CSRC, 'md.hip'), '-o', str(tmp_path / 'md.o'),
                                                '-Rpass-analysis=kernel-resource-usage'], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for kernel in ('md_step_kernel', 'md_init_velocities_kernel'):
        blocks = [b for b in re.split(r'remark: Function Name: ', r.stderr)[1:] if kernel in b.split()[0]]
        assert len(blocks) == 1, kernel
        num = lambda key: int(re.search(key + r': (\d+)', blocks[0]).group(1))
        assert num(r'ScratchSize \[bytes/lane\]') == 0, kernel
        assert num(r'LDS Size \[bytes/block\]') <= 256, kernel


def test_philox_known_answers():
    """(No GPU.)  Philox4x32-10 as (counter; key) -> output."""
    known = [((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
             ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1')]
    for counter, key, want in known:
        assert ' '.join('%08x' % int(x[0]) for x in philox4x32(counter, key)) == want
    both = philox4x32((np.array([0, 0xffffffff]), np.array([0, 0xffffffff]), np.array([0, 0xffffffff]), np.array([0, 0xffffffff])),
                      (0, 0))                                      # (vectorised over atoms: the first row is the first answer)
    assert ' '.join('%08x' % int(x[0]) for x in both) == known[0][2]


@pytest.mark.parametrize('seed', [2, 1, 12345])
def test_reference_normals_are_standard_normal(seed):
    """(No GPU.)  4096 atoms, stream 1: n = 12288 values; |mean| sqrt(n) < 5, |var - 1| < 5 sqrt(2 / n), and every
    cross-correlation of the three components below 5 / sqrt(4096)."""
    z = normals(seed, 4096, 0, 1)
    n = z.size
    mean, var = abs(z.mean()) * np.sqrt(n), abs(z.var() - 1.0) / np.sqrt(2.0 / n)
    cross = np.abs(np.corrcoef(z.T) - np.eye(3)).max() * np.sqrt(4096)
    print('seed', seed, 'standard errors: mean', mean, 'variance', var, 'cross-correlation', cross)
    assert mean < 5 and var < 5 and cross < 5


def test_md_inputs_meet_their_preconditions():
    """(No GPU.)  The kernel-test batches play every role at the sizes of SIZES and the reference takes the branch the role names
    under every pair of flags; the NVE wells of the reference stay within the shadow-energy bound; the Langevin well of the
    reference is within 2.5 % of kT over records 100..299."""
    seen = set()
    for shift in SHIFTS:
        c = _kernel_case(shift)
        assert [int(b - a) for a, b in zip(c.gptr[:-1], c.gptr[1:])] == SIZES
        for kick_in, advance in FLAGS:
            for mass in (True, False):
                pos, vel, st = _ref(c, kick_in, advance, mass)
                for g, role in enumerate(c.roles):
                    s = slice(int(c.gptr[g]), int(c.gptr[g + 1]))
                    moved = not np.array_equal(pos[s], c.pos[s])
                    if role in ('failed', 'nan', 'inf', 'vinf'):
                        assert st['status'][g] == 2 and st['steps'][g] == c.state['steps'][g] and not moved
                        assert np.array_equal(vel[s], c.vel[s], equal_nan=True)
                        assert (st['ke'][g] == -1.0) == (role == 'failed')
                        if role != 'failed':
                            assert np.isfinite(st['ke'][g]) == (role in ('nan', 'inf') and not kick_in)
                    else:
                        assert st['status'][g] == 0 and st['steps'][g] == c.state['steps'][g] + advance
                        assert moved == (bool(advance) and role not in ('all_fixed', 'empty')), (role, g)
                        assert np.isfinite(st['ke'][g]) and (st['ke'][g] > 0) == (role not in ('all_fixed', 'empty'))
                    seen.add((role, SIZES[g]))
        strong = [g for g, r in enumerate(c.roles) if r == 'strong']
        assert all(np.exp(-c.gamma[g] * c.dt[g]) < 3e-9 for g in strong)
    assert {r for r, _ in seen} == set(ROLES) | {'empty'}
    for role in ('nve', 'langevin'):                              # each at a size below, at and above one wavefront / workgroup
        assert len({m for r, m in seen if r == role}) >= 3
    h = _harmonic('nve', NVE)
    e = h.epot + h.ekin
    assert h.fixed.any() and (h.state['status'] == 0).all() and (h.state['steps'] == NVE['steps']).all()
    drift, bound = np.abs(e - e[0]).max(0), _shadow_bound(h, e[0])
    print('NVE reference: energy', e[0], 'largest deviation', drift, 'bound', bound)
    assert (drift <= bound).all() and (drift > 0).all()
    assert (h.ekin.max(0) > 0.1 * e[0]).all()                      # (the wells do swing: energy moves between the two forms)
    assert np.array_equal(h.pos[h.fixed], h.pos0[h.fixed])
    lan = _harmonic('lan', LAN)
    kT = (2.0 * lan.ekin[100:300, 0] / (3 * LAN['sizes'][0])).mean()
    print('Langevin reference: mean kT over records 100..299', kT, 'relative error', kT / LAN['kT'] - 1.0)
    assert abs(kT / LAN['kT'] - 1.0) < 0.025


def test_run_refusals():
    """(No GPU.)  What relax() refuses -- a PAMNet that keeps its positions in x, a batch without pos or batch, CPU tensors
    (RuntimeError: no CPU path) -- is refused before anything runs."""
    import models
    from pamnet_amd import synth
    from pamnet_amd.md import run, temperature
    h = _harmonic('nve', NVE)
    model = Harmonic(torch.from_numpy(h.k), torch.from_numpy(h.x0))
    data = synth.Batch(pos=torch.from_numpy(h.pos0), batch=torch.from_numpy(h.batch), num_graphs=3)
    pdb = models.PAMNet(models.Config(dataset='PDBbind', dim=16, n_layer=1, cutoff_l=2.0, cutoff_g=6.0))
    with pytest.raises(ValueError, match=r'x\[:, :3\]'):
        run(pdb, data, 10, 0.05)
    with pytest.raises(ValueError, match='no `pos`'):
        run(model, synth.Batch(batch=data.batch, num_graphs=3), 10, 0.05)
    with pytest.raises(ValueError, match='no `batch`'):
        run(model, synth.Batch(pos=data.pos, num_graphs=3), 10, 0.05)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        run(model, data, 10, 0.05)
    assert torch.equal(data.pos, torch.from_numpy(h.pos0))
    assert temperature(6.0, 5, remove_com=True) == 1.0 and temperature(6.0, 4, remove_com=False) == 1.0


# ------------------------------------------------------------------------------------------------------- kernel tests
def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _step_on_device(dev, c, kick_in, advance, mass=True, graphs=None, scalars=None, seed=True):
    """One launch on the graphs `graphs` (a slice) of a case -> (pos, vel, state) as numpy.  scalars: (dt, kT, gamma) floats in
    place of the per-graph arrays; seed=False: a NULL seed."""
    from pamnet_amd import md as M
    graphs = slice(0, len(c.gptr) - 1) if graphs is None else graphs
    lo, hi = int(c.gptr[graphs.start]), int(c.gptr[graphs.stop])
    pos, vel, dE = _t(dev, c.pos[lo:hi]), _t(dev, c.vel[lo:hi]), _t(dev, c.dE[lo:hi])
    state = {k: _t(dev, c.state[k][graphs]) for k in STATE}
    if not seed:
        state['seed'] = None
    dt, kT, gamma = scalars if scalars is not None else (_t(dev, c.dt[graphs]), _t(dev, c.kT[graphs]), _t(dev, c.gamma[graphs]))
    M.md_step(pos, vel, dE, _t(dev, c.gptr[graphs.start:graphs.stop + 1] - lo), state, dt, kT, gamma,
              _t(dev, c.mass[lo:hi]) if mass else None, _t(dev, c.fixed[lo:hi].astype(np.uint8)), kick_in, advance)
    return pos.cpu().numpy(), vel.cpu().numpy(), {k: (None if v is None else v.cpu().numpy()) for k, v in state.items()}


def _assert_step_matches(got, want, before, gptr, fixed, advance, tag=''):
    """got / want / before: (pos, vel, state); the checks of one launch against md_step_ref."""
    (gp, gv, gs), (wp, wv, ws), (bp, bv, bs) = got, want, before
    for k in ('status', 'steps', 'seed'):
        assert np.array_equal(gs[k], ws[k]), (tag, k, gs[k], ws[k])
    worst = [0.0, 0.0]
    for g in range(len(gptr) - 1):
        s = slice(int(gptr[g]), int(gptr[g + 1]))
        gk, wk = gs['ke'][g], ws['ke'][g]
        if bs['status'][g] != 0:
            assert gk == bs['ke'][g] or (np.isnan(gk) and np.isnan(bs['ke'][g])), (tag, g)
        elif np.isfinite(wk):
            assert abs(gk - wk) <= 1e-12 * abs(wk), (tag, g, gk, wk)
        else:
            assert np.isnan(gk) == np.isnan(wk) and np.isinf(gk) == np.isinf(wk), (tag, g, gk, wk)
        if bs['status'][g] != 0 or ws['status'][g] != 0:           # left alone, or failed in this launch: bit for bit the input
            assert np.array_equal(gp[s], bp[s], equal_nan=True) and np.array_equal(gv[s], bv[s], equal_nan=True), (tag, g)
            assert gs['steps'][g] == bs['steps'][g], (tag, g)
            continue
        if s.stop == s.start:
            continue
        fx = fixed[s]
        assert np.array_equal(gp[s][fx], bp[s][fx]) and np.array_equal(gv[s][fx], bv[s][fx]), (tag, g, 'fixed rows')
        if fx.all():
            continue
        ev = maxnorm_err(gv[s][~fx], wv[s][~fx])
        if advance:
            want_d = wp[s].astype(np.float64) - bp[s]
            assert float(np.abs(want_d).max()) > 0
            ed = maxnorm_err(gp[s].astype(np.float64) - bp[s], want_d)
        else:
            assert np.array_equal(gp[s], bp[s]), (tag, g, 'pos')
            ed = 0.0
        worst = [max(worst[0], ev), max(worst[1], ed)]
        assert ev <= KTOL and ed <= KTOL, (tag, g, ev, ed)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize('shift', SHIFTS)
def test_one_step_on_a_batch_vs_the_reference(dev, shift):
    """Graphs of 1 .. 1025 and 0 atoms in the roles of _kernel_case, per-graph dt / kT / gamma, under every (kick_in, advance),
    with masses and with NULL: steps and status equal, ke to 1e-12, vel and the displacement within KTOL per graph; rows of fixed
    atoms, of the graph that was failed and of the graphs that fail bit for bit the input.  Then every running graph once more
    with ITS dt, kT and gamma as the scalars of the launch: bitwise what the per-graph arrays gave it."""
    c = _kernel_case(shift)
    worst = [0.0, 0.0]
    for kick_in, advance in FLAGS:
        for mass in (True, False):
            got = _step_on_device(dev, c, kick_in, advance, mass)
            w = _assert_step_matches(got, _ref(c, kick_in, advance, mass), (c.pos, c.vel, c.state), c.gptr, c.fixed, advance,
                                     tag=(shift, kick_in, advance, mass))
            worst = [max(worst[0], w[0]), max(worst[1], w[1])]
    print('shift', shift, 'worst vel / displacement error', worst)
    arrays = _step_on_device(dev, c, 1, 1)
    for g, role in enumerate(c.roles):
        if role not in ('nve', 'langevin', 'strong', 'kt0'):
            continue
        s = slice(int(c.gptr[g]), int(c.gptr[g + 1]))
        p, v, st = _step_on_device(dev, c, 1, 1, scalars=(float(c.dt[g]), float(c.kT[g]), float(c.gamma[g])))
        assert np.array_equal(p[s], arrays[0][s]) and np.array_equal(v[s], arrays[1][s]), (role, g)
        assert st['ke'][g] == arrays[2]['ke'][g] and st['steps'][g] == c.state['steps'][g] + 1


@pytest.mark.gpu
@pytest.mark.parametrize('remove_com,rescale', [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_init_velocities_vs_the_reference(dev, remove_com, rescale):
    """SIZES, masses in [1, 40], a fifth of the atoms fixed in graphs of 63 atoms or more, per-graph kT: velocities within KTOL per
    graph, ke to 1e-12, rows of fixed atoms untouched; after remove_com the momentum is below 1e-6 of sum m |v|; after rescale
    ke == dof kT / 2 to 1e-12.  With unit masses (NULL), kT = 1 and no flag the velocities are the reference's normals: the
    generator's device test."""
    from pamnet_amd import md as M
    c = _kernel_case(0)
    fixed = c.fixed & (np.array(c.roles)[np.repeat(np.arange(len(SIZES)), SIZES)] != 'all_fixed')
    G, n = len(SIZES), len(c.pos)
    kT = np.random.RandomState(3).uniform(0.1, 2.0, G)
    vel0 = np.full((n, 3), 7.0, np.float32)
    want, want_ke = init_velocities_ref(vel0, c.gptr, c.state['seed'], kT, c.mass, fixed, remove_com, rescale)
    vel, ke = _t(dev, vel0), torch.full((G,), -1.0, dtype=torch.float64, device=dev)
    M.init_velocities(vel, _t(dev, c.gptr), _t(dev, c.state['seed']), _t(dev, kT), ke, _t(dev, c.mass),
                      _t(dev, fixed.astype(np.uint8)), remove_com, rescale)
    got, ke = vel.cpu().numpy(), ke.cpu().numpy()
    assert np.array_equal(got[fixed], vel0[fixed]) and fixed.any()
    for g in range(G):
        s = slice(int(c.gptr[g]), int(c.gptr[g + 1]))
        free = ~fixed[s]
        if not free.any():
            assert ke[g] == 0.0
            continue
        v, m = got[s][free].astype(np.float64), c.mass[s][free].astype(np.float64)[:, None]
        if free.sum() == 1 and remove_com:        # one atom without its centre-of-mass motion: v - (m v) / m, roundings of 0
            assert np.abs(v).max() <= 1e-12 and ke[g] <= 1e-24
            continue
        assert abs(ke[g] - want_ke[g]) <= 1e-12 * want_ke[g], (g, ke[g], want_ke[g])
        assert maxnorm_err(got[s][free], want[s][free]) <= KTOL, g
        if remove_com and free.sum() > 1:
            assert np.abs((m * v).sum(0)).max() <= 1e-6 * (m * np.abs(v)).sum(), g
        dof = 3 * int(free.sum()) - 3 * remove_com
        if rescale and dof > 0:
            assert abs(ke[g] - 0.5 * dof * kT[g]) <= 1e-12 * 0.5 * dof * kT[g], g
    if not remove_com and not rescale:
        vel = _t(dev, vel0)
        M.init_velocities(vel, _t(dev, c.gptr), _t(dev, c.state['seed']), 1.0, _t(dev, np.zeros(G)), None, None, False, False)
        got = vel.cpu().numpy()
        for g in range(G):
            s = slice(int(c.gptr[g]), int(c.gptr[g + 1]))
            if SIZES[g]:
                assert maxnorm_err(got[s], normals(c.state['seed'][g], SIZES[g], 0, 1)) <= KTOL, g


@pytest.mark.gpu
def test_noise_depends_on_seed_and_step_only(dev):
    """Four copies of one 65-atom graph at rest (f = 0, kT = 1, gamma = 2) that differ in (seed, step) only: the same pair gives the
    same velocities bit for bit, another seed or another step different ones.  And a gamma = 0 graph beside thermostatted ones is
    bitwise the result of a launch with gamma = 0 and seed = NULL."""
    m = 65
    rng = np.random.RandomState(9)
    one = dict(pos=rng.uniform(-1, 1, (m, 3)).astype(np.float32), vel=np.zeros((m, 3), np.float32), dE=np.zeros((m, 3), np.float32),
               mass=np.ones(m, np.float32), fixed=np.zeros(m, bool), dt=0.05, kT=1.0, gamma=2.0)
    c = _assemble([dict(one, seed=s, steps=k) for s, k in ((5, 3), (6, 3), (5, 4), (5, 3))])
    p, v, st = _step_on_device(dev, c, 0, 1)
    a, b, d, e = (v[i * m:(i + 1) * m] for i in range(4))
    assert np.array_equal(a, e) and np.array_equal(p[:m], p[3 * m:])
    assert not np.array_equal(a, b) and not np.array_equal(a, d) and not np.array_equal(b, d)
    assert abs(np.corrcoef(a.ravel(), b.ravel())[0, 1]) < 5 / np.sqrt(3 * m) and abs(np.corrcoef(a.ravel(), d.ravel())[0, 1]) < 5 / np.sqrt(3 * m)
    assert st['steps'].tolist() == [4, 4, 5, 4]
    k = _kernel_case(0)
    c2 = copy.copy(k)
    c2.gamma = np.where(np.arange(len(SIZES)) % 2 == 0, 0.0, k.gamma)
    mixed = _step_on_device(dev, c2, 1, 1)
    plain = _step_on_device(dev, c2, 1, 1, scalars=(_t(dev, k.dt), 0.0, 0.0), seed=False)
    checked = 0
    for g in range(0, len(SIZES), 2):
        s = slice(int(k.gptr[g]), int(k.gptr[g + 1]))
        assert np.array_equal(mixed[0][s], plain[0][s], equal_nan=True) and np.array_equal(mixed[1][s], plain[1][s], equal_nan=True)
        assert mixed[2]['ke'][g] == plain[2]['ke'][g] or np.isnan(plain[2]['ke'][g])
        checked += int(mixed[2]['status'][g] == 0 and SIZES[g] > 0)
    assert checked >= 3


@pytest.mark.gpu
def test_a_step_is_repeatable_and_independent_of_the_batch(dev):
    """Thermostat on.  Every graph of _indep_graphs stepped alone, inside the batch in each of three rotations of its order, and
    twice over: its rows of pos and vel, its ke and its steps are equal bit for bit in all of them."""
    graphs = _indep_graphs()
    alone = []
    for g in graphs:
        p, v, st = _step_on_device(dev, _assemble([g]), 1, 1)
        alone.append((p, v, st['ke'][0], st['steps'][0]))
        assert st['steps'][0] == g['steps'] + 1
    for rot in (0, 4, 7, 0):
        order = list(range(rot, len(graphs))) + list(range(rot))
        c = _assemble([graphs[i] for i in order])
        p, v, st = _step_on_device(dev, c, 1, 1)
        for j, i in enumerate(order):
            s = slice(int(c.gptr[j]), int(c.gptr[j + 1]))
            assert np.array_equal(p[s], alone[i][0]) and np.array_equal(v[s], alone[i][1]), (rot, i)
            assert st['ke'][j] == alone[i][2] and st['steps'][j] == alone[i][3], (rot, i)
    assert not np.array_equal(alone[4][1], graphs[4]['vel'])


@pytest.mark.gpu
def test_the_entry_points_validate_their_arguments(dev):
    """Both entry points: a null required pointer is PAMNET_ENULL; a negative count, a flag other than 0 / 1 and a bad scalar where
    its per-graph array is NULL are PAMNET_EINVAL; mass, fixed and the per-graph arrays may be NULL, the step's seed where there
    is no friction; a per-graph array replaces its scalar; n_graphs == 0 launches nothing."""
    from pamnet_amd import lib
    c = _kernel_case(0)
    G, n = len(SIZES), len(c.pos)
    pos, vel, dE, gptr, mass = _t(dev, c.pos), _t(dev, c.vel), _t(dev, c.dE), _t(dev, c.gptr), _t(dev, c.mass)
    st = {k: _t(dev, c.state[k]) for k in STATE}
    dt_g, zeros = _t(dev, c.dt), _t(dev, np.zeros(G))
    nan, inf = float('nan'), float('inf')

    def step(**kw):
        a = dict(pos=lib.ptr(pos), vel=lib.ptr(vel), dpos=lib.ptr(dE), mass=None, fixed=None, gptr=lib.ptr(gptr), n=n, G=G,
                 dt_g=None, kT_g=None, gamma_g=None, dt=0.05, kT=0.5, gamma=1.0, kick_in=1, advance=1)
        a.update({k: lib.ptr(st[k]) for k in STATE})
        a.update(kw)
        lib.call(STEP, a['pos'], a['vel'], a['dpos'], a['mass'], a['fixed'], a['gptr'], a['n'], a['G'], a['seed'], a['steps'],
                 a['status'], a['ke'], a['dt_g'], a['kT_g'], a['gamma_g'], a['dt'], a['kT'], a['gamma'], a['kick_in'], a['advance'],
                 lib.stream_of(pos))

    def init(**kw):
        a = dict(vel=lib.ptr(vel), mass=None, fixed=None, gptr=lib.ptr(gptr), n=n, G=G, seed=lib.ptr(st['seed']), kT_g=None, kT=0.5,
                 remove_com=1, rescale=1, ke=lib.ptr(st['ke']))
        a.update(kw)
        lib.call(INIT, a['vel'], a['mass'], a['fixed'], a['gptr'], a['n'], a['G'], a['seed'], a['kT_g'], a['kT'], a['remove_com'],
                 a['rescale'], a['ke'], lib.stream_of(vel))

    for k in ('pos', 'vel', 'dpos', 'gptr', 'seed', 'steps', 'status', 'ke'):
        with pytest.raises(RuntimeError, match='PAMNET_ENULL'):
            step(**{k: None})
    with pytest.raises(RuntimeError, match='PAMNET_ENULL'):
        step(seed=None, gamma=0.0, gamma_g=lib.ptr(zeros))          # (a per-graph friction may hold anything: the seed is needed)
    for kw in (dict(n=-1), dict(G=-1), dict(G=2 ** 31), dict(kick_in=2), dict(kick_in=-1), dict(advance=2), dict(dt=0.0),
               dict(dt=-0.1), dict(dt=nan), dict(dt=inf), dict(kT=-1.0), dict(kT=nan), dict(kT=inf), dict(gamma=-1.0),
               dict(gamma=nan), dict(gamma=inf)):
        with pytest.raises(RuntimeError, match='PAMNET_EINVAL'):
            step(**kw)
    for k in ('vel', 'gptr', 'seed', 'ke'):
        with pytest.raises(RuntimeError, match='PAMNET_ENULL'):
            init(**{k: None})
    for kw in (dict(n=-1), dict(G=-1), dict(G=2 ** 31), dict(remove_com=2), dict(rescale=-1), dict(kT=-1.0), dict(kT=nan),
               dict(kT=inf)):
        with pytest.raises(RuntimeError, match='PAMNET_EINVAL'):
            init(**kw)
    step(G=0)
    init(G=0)
    torch.cuda.synchronize()
    same = lambda: (torch.equal(pos, _t(dev, c.pos)) and torch.equal(vel.nan_to_num(1.0, 2.0, 3.0), _t(dev, c.vel).nan_to_num(1.0, 2.0, 3.0))
                    and all(torch.equal(st[k], _t(dev, c.state[k])) for k in STATE))
    assert same()
    # a per-graph array replaces its scalar, which is then not looked at; every graph already failed: nothing is touched
    st['status'].fill_(2)
    step(dt_g=lib.ptr(dt_g), dt=nan, kT_g=lib.ptr(zeros), kT=-1.0, gamma_g=lib.ptr(zeros), gamma=inf, mass=lib.ptr(mass))
    step(seed=None, gamma=0.0)
    torch.cuda.synchronize()
    st['status'].copy_(_t(dev, c.state['status']))
    assert same()
    init(kT_g=lib.ptr(zeros), kT=nan, mass=lib.ptr(mass))          # kT = 0 for every graph: velocities 0, ke 0
    torch.cuda.synchronize()
    assert not vel.any() and not st['ke'].any()


# ----------------------------------------------------------------------------------------------------- end to end
def _replay(res, gptr, dt, kT, gamma, mass, fixed, steps):
    """Every launch of a trace through md_step_ref from its recorded inputs; consecutive launches hand on what they stored."""
    cpu = lambda t: None if t is None else t.cpu().numpy()
    worst = [0.0, 0.0]
    assert len(res.trace) == steps + 1
    for i, r in enumerate(res.trace):
        assert (r['kick_in'], r['advance']) == (1 if i else 0, 1 if i < steps else 0)
        before = (cpu(r['pos']), cpu(r['v_before']), {k: cpu(v) for k, v in r['state_before'].items()})
        got = (cpu(r['pos_after']), cpu(r['v_after']), {k: cpu(v) for k, v in r['state_after'].items()})
        want = md_step_ref(before[0], before[1], cpu(r['dE']), gptr, before[2], dt, kT, gamma, mass, fixed, r['kick_in'], r['advance'])
        w = _assert_step_matches(got, want, before, gptr, np.zeros(len(before[0]), bool) if fixed is None else fixed,
                                 r['advance'], tag=i)
        worst = [max(worst[0], w[0]), max(worst[1], w[1])]
        if i + 1 < len(res.trace):
            assert torch.equal(r['pos_after'], res.trace[i + 1]['pos']) and torch.equal(r['v_after'], res.trace[i + 1]['v_before'])
    assert torch.equal(res.trace[-1]['pos_after'], res.pos) and torch.equal(res.trace[-1]['v_after'], res.vel)
    assert torch.equal(res.trace[-1]['state_after']['ke'], res.kinetic)
    return worst


def _well(dev, h):
    from pamnet_amd import synth
    model = Harmonic(torch.from_numpy(h.k), torch.from_numpy(h.x0)).to(dev)
    data = synth.Batch(pos=torch.from_numpy(h.pos0), batch=torch.from_numpy(h.batch), num_graphs=len(h.k)).to(dev)
    return model, data


@pytest.mark.gpu
def test_harmonic_wells_conserve_their_energy(dev):
    """NVE from rest, three wells of 4 / 9 / 70 atoms, k = (0.5, 2, 6), masses in [1, 40], some atoms fixed, dt = 0.05, 400 steps,
    check_every = 0: every launch of the trace replayed through md_step_ref within KTOL; epot + ekin of every record within
    E0 h / (1 - h) + 1e-4 E0 of the first (_shadow_bound; the CPU test asserts it of the reference trajectory); the records are
    the trace's; fixed atoms and the caller's tensors stay.  Under torch's synchronisation debug mode the run synchronises once --
    the set-up read that finds the masses positive -- and without masses not at all."""
    from pamnet_amd.md import run
    h = _harmonic('nve', NVE)
    model, data = _well(dev, h)
    mass, fixed = _t(dev, h.mass), _t(dev, h.fixed)
    steps = NVE['steps']
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        torch.cuda.set_sync_debug_mode('warn')
        try:
            res = run(model, data, steps, H_DT, masses=mass, fixed=fixed, record_every=1, check_every=0, trace=True)
        finally:
            torch.cuda.set_sync_debug_mode('default')
    syncs = [str(w.message) for w in caught if 'called a synchronizing' in str(w.message)]
    print('synchronisations of a 400-step run:', syncs)
    assert len(syncs) == 1
    torch.cuda.set_sync_debug_mode('error')
    try:
        res12 = run(model, data, 12, H_DT, fixed=fixed, record_every=5, check_every=0)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert res12.steps.tolist() == [12, 12, 12] and tuple(res12.frames.shape) == (3, len(h.pos0), 3) and res12.trace is None
    assert torch.equal(data.pos.cpu(), torch.from_numpy(h.pos0)) and res.pos is not data.pos
    assert res.steps.tolist() == [steps] * 3 and not res.failed.any() and res.failed.dtype == torch.bool
    worst = _replay(res, h.gptr, H_DT, 0.0, 0.0, h.mass, h.fixed, steps)
    print('NVE wells: worst vel / displacement error of the replay', worst)
    assert tuple(res.frames.shape) == (steps + 1, len(h.pos0), 3) and tuple(res.epot.shape) == tuple(res.ekin.shape) == (steps + 1, 3)
    for i in (0, 1, 200, steps):
        assert torch.equal(res.frames[i], res.trace[i]['pos']) and torch.equal(res.ekin[i], res.trace[i]['state_after']['ke'])
    assert torch.equal(res.frames[steps], res.pos) and torch.equal(res.ekin[steps], res.kinetic)
    assert torch.equal(res.epot[steps], res.energy.double()) and torch.equal(res.pos[fixed], data.pos[fixed])
    assert torch.equal(res.forces, -model.k[data.batch, None] * (res.pos - model.x0))
    e = (res.epot + res.ekin).cpu().numpy()
    drift, bound = np.abs(e - e[0]).max(0), _shadow_bound(h, e[0])
    print('NVE wells: energy', e[0], 'largest deviation', drift, 'bound', bound)
    assert (drift <= bound).all()
    assert maxnorm_err(e[0], (h.epot + h.ekin)[0]) <= 1e-6


@pytest.mark.gpu
def test_a_harmonic_well_reaches_its_temperature(dev):
    """Langevin from rest at the minimum: 512 atoms, k = 2, masses in [1, 40], kT = 0.7, gamma = 2, dt = 0.05, 300 steps, seed 2: the
    mean of 2 ekin / (3 N) over records 100..299 is within 5 % of kT (the reference: within 2.5 %, asserted by the CPU test), and
    every launch of the trace replayed through md_step_ref is within KTOL."""
    from pamnet_amd.md import run, temperature
    h = _harmonic('lan', LAN)
    model, data = _well(dev, h)
    steps, N = LAN['steps'], LAN['sizes'][0]
    res = run(model, data, steps, H_DT, masses=_t(dev, h.mass), kT=LAN['kT'], gamma=LAN['gamma'], seed=LAN['seed'],
              velocities=torch.zeros(N, 3, device=dev), record_every=1, trace=True)
    assert res.steps.tolist() == [steps] and not res.failed.any()
    assert np.array_equal(res.trace[0]['state_before']['seed'].cpu().numpy(), h.seeds)
    worst = _replay(res, h.gptr, H_DT, LAN['kT'], LAN['gamma'], h.mass, None, steps)
    kT = float(temperature(res.ekin[100:300, 0], N, remove_com=False).mean())
    print('Langevin well: mean kT over records 100..299', kT, 'relative error', kT / LAN['kT'] - 1.0, 'replay', worst)
    assert abs(kT / LAN['kT'] - 1.0) < 0.05


def _pamnet_batch():
    """[a bond-free molecule in open space (zero cell, pbc all False), 24 atoms in the triclinic cell TRI_A, the slab slab_min of
    tests/test_pbc_axes.py with pbc = (True, True, False)], and the slab's bottom layer (the third of its atoms lowest along the
    open axis) as the fixed mask (as tests/test_relax.py builds it)."""
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
    mass = rng.uniform(1.0, 20.0, b.pos.size(0)).astype(np.float32)
    _MADE['pamnet'] = (b, torch.from_numpy(fixed), torch.from_numpy(mass))
    return _MADE['pamnet']


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['nve', 'langevin'])
@pytest.mark.parametrize('dim,n_layer', MODELS)
def test_pamnet_dynamics_replayed_step_by_step(dev, dim, n_layer, mode):
    """PAMNet on {bond-free molecule, triclinic cell, slab with a fixed bottom layer}, 8 steps of NVE from rest and of Langevin
    (per-graph seeds, Maxwell-Boltzmann start), trace=True: every launch replayed through md_step_ref from its recorded inputs
    matches as in the kernel test; the fixed layer is torch.equal to its start; res.energy / res.forces are bitwise a fresh
    evaluation at res.pos; the caller's positions and every parameter .grad are as they were."""
    import models
    from pamnet_amd.md import run
    from test_pbc_axes import CUT_G, CUT_L
    b, fixed_cpu, mass_cpu = _pamnet_batch()
    torch.manual_seed(0)
    model = models.PAMNet(models.Config(dataset='QM9', dim=dim, n_layer=n_layer, cutoff_l=CUT_L, cutoff_g=CUT_G)).to(dev)
    data, fixed, mass = b.to(dev), fixed_cpu.to(dev), mass_cpu.to(dev)
    model(data).sum().backward()                                   # parameter gradients to find untouched afterwards
    snap = [None if p.grad is None else p.grad.clone() for p in model.parameters()]
    pos0 = data.pos.clone()
    seeds = torch.tensor([11, -5, 2 ** 40 + 3], dtype=torch.int64, device=dev)
    kw = dict(kT=0.05, gamma=1.0, seed=seeds) if mode == 'langevin' else {}
    res = run(model, data, 8, 0.05, masses=mass, fixed=fixed, trace=True, **kw)
    assert torch.equal(data.pos, pos0) and not data.pos.requires_grad
    for p, s in zip(model.parameters(), snap):
        assert (p.grad is None) if s is None else torch.equal(p.grad, s)
    assert res.steps.tolist() == [8, 8, 8] and not res.failed.any()
    assert torch.equal(res.pos[fixed], pos0[fixed]) and not torch.equal(res.pos[~fixed], pos0[~fixed])
    assert not res.vel[fixed].any()
    gptr = np.concatenate([[0], np.cumsum(np.bincount(b.batch.numpy(), minlength=3))])
    if mode == 'langevin':                                         # the start: init_velocities at kT, centre of mass removed
        want, _ = init_velocities_ref(np.zeros((len(pos0), 3), np.float32), gptr, seeds.cpu().numpy(), 0.05, mass_cpu.numpy(),
                                      fixed_cpu.numpy(), True, False)
        assert maxnorm_err(res.trace[0]['v_before'].cpu().numpy(), want) <= KTOL
    else:
        assert not res.trace[0]['v_before'].any()
    worst = _replay(res, gptr, 0.05, kw.get('kT', 0.0), kw.get('gamma', 0.0), mass_cpu.numpy(), fixed_cpu.numpy(), 8)
    print(mode, 'replay: worst vel / displacement error', worst)
    d = copy.copy(data)
    d.pos = res.pos.clone().requires_grad_(True)
    e = model(d)
    de, = torch.autograd.grad(e.sum(), d.pos)
    assert torch.equal(res.energy, e.detach()) and torch.equal(res.forces, -de) and torch.isfinite(res.forces).all()


@pytest.mark.gpu
@pytest.mark.parametrize('dim,n_layer', MODELS)
def test_a_store_batch_is_run_without_its_stale_sizes(dev, dim, n_layer):
    """A MoleculeStore batch carries `sizes`, the host-side edge counts of the STORED geometry.  The driver evaluates its moved
    copies without them (relax._at): after 15 steps in which atoms cross cutoff_g (asserted: the global edge count at res.pos is
    no longer the stored one) the model's deferred checks are clean and none is pending, res.energy / res.forces are bitwise a
    plain-tensor evaluation at res.pos, and the caller's batch keeps its sizes."""
    import models
    from pamnet_amd import graph as G, store as S, synth
    from pamnet_amd.md import run
    torch.manual_seed(0)
    model = models.PAMNet(models.Config(dataset='QM9', dim=dim, n_layer=n_layer, cutoff_l=5.0, cutoff_g=5.0)).to(dev)
    mols = [synth.qm9_molecule(3, i) for i in range(12)]
    st = S.MoleculeStore(mols, dev).prepare_for(model)
    b = st.collate(list(range(12)))
    key = S.size_key(model)
    sizes = dict(b.sizes)
    assert b.sizes.get(key) is not None
    with torch.no_grad():
        model(b)                                                   # the stored geometry: its sizes are right
    model.verify()
    v0 = torch.from_numpy(0.5 * np.random.RandomState(4).standard_normal((b.pos.size(0), 3)).astype(np.float32)).to(dev)
    res = run(model, b, 15, 0.1, velocities=v0)
    assert b.sizes == sizes and res.steps.tolist() == [15] * 12 and torch.isfinite(res.energy).all() and not res.failed.any()
    model.verify()                                                 # nothing was flagged on the way ...
    assert not model._pending_checks                               # ... and nothing waits
    plain = synth.collate(mols).to(dev)
    assert torch.equal(plain.pos, b.pos)
    g = G.build_graph('QM9', 5.0, 5.0, 'source_to_target', plain.x, plain.batch, res.pos, plain.edge_index, num_graphs=12,
                      need_grad=False, n_types=5)
    print('global edges: stored geometry', b.sizes[key][0], 'final geometry', g.glob.m)
    assert g.glob.m != b.sizes[key][0]                             # the stored counts no longer describe the geometry
    plain.pos = res.pos.clone().requires_grad_(True)
    e = model(plain)
    de, = torch.autograd.grad(e.sum(), plain.pos)
    assert torch.equal(res.energy, e.detach()) and torch.equal(res.forces, -de)


@pytest.mark.gpu
def test_run_refuses_bad_arguments_on_the_device(dev):
    """Wrong shapes, dtypes and devices of masses / fixed / seed / velocities / per-graph tensors, gamma > 0 without kT, values
    out of range (floats at once, tensors by the one read at set-up), non-positive masses."""
    from pamnet_amd.md import run
    h = _harmonic('nve', NVE)
    model, data = _well(dev, h)
    mass, fixed = _t(dev, h.mass), _t(dev, h.fixed)
    f64 = lambda *v: torch.tensor(v, dtype=torch.float64, device=dev)
    bad_mass = mass.clone()
    bad_mass[5] = 0.0
    cases = [(dict(masses=h.mass), '`masses` is a float32'), (dict(masses=mass.double()), '`masses` is a float32'),
             (dict(masses=mass[:-1]), '`masses` is a float32'), (dict(masses=mass.cpu()), '`masses` is a float32'),
             (dict(masses=bad_mass), '`masses` must be finite and positive'), (dict(masses=-mass), '`masses` must be'),
             (dict(fixed=fixed.float()), '`fixed` is a torch.bool tensor'), (dict(fixed=fixed[:-1]), '`fixed` is a torch.bool'),
             (dict(seed=torch.zeros(3, dtype=torch.int32, device=dev)), 'per-graph `seed`'),
             (dict(seed=torch.zeros(2, dtype=torch.int64, device=dev)), 'per-graph `seed`'),
             (dict(seed=torch.zeros(3, dtype=torch.int64)), 'per-graph `seed`'), (dict(seed='x'), '`seed` is an int'),
             (dict(velocities=torch.zeros(5, 3, device=dev)), '`velocities` is a float32'),
             (dict(velocities=torch.zeros(len(h.pos0), 3)), '`velocities` is a float32'),
             (dict(gamma=1.0), 'needs its temperature'), (dict(gamma=f64(0, 1, 0)), 'needs its temperature'),
             (dict(gamma=-1.0, kT=1.0), '`gamma` must be non-negative'), (dict(kT=float('nan')), '`kT` must be non-negative'),
             (dict(dt=0.0), '`dt` must be positive'), (dict(dt=float('inf')), '`dt` must be positive'),
             (dict(dt=[0.1] * 3), '`dt` is a float'), (dict(dt=f64(0.1, 0.1)), 'per-graph `dt`'),
             (dict(dt=f64(0.1, 0.1, 0.1).float()), 'per-graph `dt`'), (dict(dt=f64(0.1, 0.1, 0.1).cpu()), 'per-graph `dt`'),
             (dict(dt=f64(0.1, 0.0, 0.1)), '`dt` must be finite'), (dict(kT=f64(0.1, -1.0, 0.1)), '`kT` must be finite'),
             (dict(gamma=f64(0.1, float('nan'), 0.1), kT=1.0), '`gamma` must be finite'), (dict(steps=-1), 'non-negative')]
    for kw, match in cases:
        args = dict(steps=5, dt=H_DT)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            run(model, data, **args)
    res = run(model, data, 0, H_DT, masses=mass, fixed=fixed, kT=f64(0.5, 0.0, 1.0), gamma=f64(1.0, 0.0, 0.0),
              seed=torch.tensor([1, 2, 3], device=dev), record_every=4)
    assert res.steps.tolist() == [0, 0, 0] and tuple(res.frames.shape) == (1, len(h.pos0), 3) and torch.equal(res.pos, data.pos)
    assert torch.equal(res.ekin[0], res.kinetic) and float(res.kinetic[1]) == 0.0 and float(res.kinetic[0]) > 0.0
