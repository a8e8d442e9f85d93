"""Constrained molecular dynamics: the kernels pamnet_md_constrained_step_f32 / pamnet_md_project_constraints_f32
(csrc/md_constraints.hip) and the constraint layer of pamnet_amd/md.py (Constraints, bond_constraints, constrained_step,
project_constraints, run(constraints=...)).

The reference is tests/md_constraints_ref.py: the rules of include/pamnet_hip.h restated in numpy fp64 with the same colour and
sweep order, over md_ref's generator and unconstrained step.  Inputs are made once on the CPU with fixed seeds and never modified;
what the GPU tests presuppose of the reference is asserted by tests that need no GPU.

Tolerances: KTOL = 1e-6 max-normalised per graph for the velocities and the displacement (tests/test_md.py); 1e-12 relative for
the fp64 kinetic energy; 1e-6 relative for the constrained distances of stored fp32 positions (the rounding of a coordinate below
2 is at most 1.2e-7; a distance of 1 moves by at most sqrt(3) x 2.4e-7 = 4.2e-7); equality for steps, status, sweeps and
everything that must not move."""
import numpy as np
import pytest
import torch

from conftest import maxnorm_err
from md_constraints_ref import STATE, ConsRef, colour_ref, constrained_step_ref, project_ref
from md_ref import init_velocities_ref, md_step_ref
from pamnet_amd import md as M
from test_md import FLAGS, KTOL, MODELS, SIZES, Harmonic

Constraints, bond_constraints = M.Constraints, M.bond_constraints      # (the names this file is about)
STEP, PROJECT = 'pamnet_md_constrained_step_f32', 'pamnet_md_project_constraints_f32'
TOL = 1e-10                                       # the solves' bound in the kernel tests and the reference physics
MAX_SWEEPS = 500                                 # of the kernel tests: every converging graph takes at most half (CPU test)
ROLE_OF = {1: 'failed', 2: 'one_fixed', 63: 'water', 64: 'none', 65: 'star', 255: 'ring', 256: 'nan', 257: 'unconverged',
           300: 'chain', 1025: 'chain', 0: 'empty'}
GAMMA_OF = {1: 2.0, 2: 2.0, 63: 2.0, 64: 2.0, 65: 0.0, 255: 2.0, 256: 0.0, 257: 2.0, 300: 2.0, 1025: 0.0, 0: 0.0}
LENGTH_TOL = 1e-6


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


# ------------------------------------------------------------------------------------------------------------ geometries
def _rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    return q * np.sign(np.diag(r))


def _chain(rng, m, box=1.5, shuffle=False):
    """A walk of unit steps kept inside |coordinate| <= box, every bond constrained: (pos [m, 3], pairs [m - 1, 2], lengths)."""
    pos = [rng.uniform(-0.5, 0.5, 3)]
    while len(pos) < m:
        u = rng.standard_normal(3)
        p = pos[-1] + u / np.linalg.norm(u)
        if np.abs(p).max() <= box:
            pos.append(p)
    pairs = np.stack([np.arange(m - 1), np.arange(1, m)], axis=1)
    if shuffle:
        pairs = pairs[rng.permutation(m - 1)]
    return np.array(pos), pairs, np.ones(m - 1)


def _arc(m, radius=1.5, turn=300.0):
    """m atoms evenly on `turn` degrees of a circle: a chain whose neighbouring bonds are almost parallel, so that a sweep hands a
    correction on by about one bond: (pos, pairs, lengths)."""
    phi = np.radians(turn) * np.arange(m) / (m - 1)
    pos = radius * np.stack([np.cos(phi), np.sin(phi), np.zeros(m)], axis=1)
    pairs = np.stack([np.arange(m - 1), np.arange(1, m)], axis=1)
    return pos, pairs, np.sqrt(((pos[1:] - pos[:-1]) ** 2).sum(1))


WATER = (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [np.cos(np.radians(104.5)), np.sin(np.radians(104.5)), 0.0]]),
         np.array([[0, 1], [0, 2], [1, 2]]))
STAR = (1.09 * np.array([[0.0, 0.0, 0.0], [1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]) / np.array([1, 3, 3, 3, 3])[:, None] ** 0.5,
        np.array([[0, 1], [0, 2], [0, 3], [0, 4]]))
_R5 = 1.4 / (2.0 * np.sin(np.pi / 5))
RING = (np.array([[_R5 * np.cos(2 * np.pi * k / 5), _R5 * np.sin(2 * np.pi * k / 5), 0.0] for k in range(5)]),
        np.array([[0, 1], [1, 2], [2, 3], [3, 4], [4, 0]]))


def _molecules(rng, template, count, spread=0.6):
    """`count` rotated copies of a template (pos, pairs) with centres inside +- spread: (pos, pairs, lengths).  The lengths are
    the template's, exact in fp64."""
    tp, tq = template
    k = len(tp)
    d = np.sqrt(((tp[tq[:, 0]] - tp[tq[:, 1]]) ** 2).sum(1))
    pos = np.concatenate([(tp - tp.mean(0)) @ _rotation(rng) + rng.uniform(-spread, spread, 3) for _ in range(count)])
    pairs = np.concatenate([tq + k * c for c in range(count)])
    return pos, pairs, np.tile(d, count)


# ------------------------------------------------------------------------------------------------- kernel-test inputs
def _kernel_case():
    """One batch of SIZES, per-graph dt in [0.02, 0.1], masses in [1, 40], steps in [0, 40), seeds over all of int64, kT = 0.7
    and gamma = 2 or 0 (GAMMA_OF), velocities and gradients standard normal:
      chain        300 and 1025 atoms, every bond constrained (1025: its pairs in a random order): more constraints than threads
      water        21 triangles; the oxygens of the first three are fixed     star   13 centres with four arms
      ring         51 rings of five                                            none   64 atoms, a fifth fixed, no constraint
      one_fixed    two atoms, the first fixed                                  failed status 2, with a velocity not to be read
      nan          a chain of 256 with one NaN gradient entry                  empty  the last graph
      unconverged  a chain of 257 equal masses along an arc (_arc) at rest and without forces, lengths 0.9 of its start: only the
                   stretched start keeps it from converging -- its velocity solves find nothing to do, and the contraction of
                   the whole chain, handed on bond by bond, takes far more sweeps than MAX_SWEEPS
    The pairs are listed with the later graphs first: Constraints has to sort them.  Coordinates stay below 2."""
    if 'kernel' in _MADE:
        return _MADE['kernel']
    rng = np.random.RandomState(77)
    n, G = sum(SIZES), len(SIZES)
    c = Case()
    c.gptr = _gptr(SIZES)
    c.batch = np.repeat(np.arange(G), SIZES)
    c.roles = [ROLE_OF[m] for m in SIZES]
    c.pos = rng.uniform(-1.5, 1.5, (n, 3))
    c.vel = rng.standard_normal((n, 3)).astype(np.float32)
    c.dE = rng.standard_normal((n, 3)).astype(np.float32)
    c.mass = rng.uniform(1.0, 40.0, n).astype(np.float32)
    c.fixed = np.zeros(n, dtype=bool)
    c.dt = rng.uniform(0.02, 0.1, G)
    c.kT, c.gamma = np.full(G, 0.7), np.array([GAMMA_OF[m] for m in SIZES])
    c.state = dict(seed=rng.randint(-2 ** 63, 2 ** 63 - 1, G, dtype=np.int64), steps=rng.randint(0, 40, G).astype(np.int32),
                   status=np.zeros(G, np.int32), ke=np.full(G, -1.0), sweeps=np.full(G, -1, np.int32))
    pairs, lengths = [], []
    for g, (m, role) in enumerate(zip(SIZES, c.roles)):
        lo = int(c.gptr[g])
        made = None
        if role == 'chain':
            made = _chain(rng, m, shuffle=(m == 1025))
        elif role == 'nan':
            made = _chain(rng, m)
        elif role == 'unconverged':
            made = _arc(m)
            c.vel[lo:lo + m], c.dE[lo:lo + m], c.mass[lo:lo + m] = 0.0, 0.0, 12.0
        elif role == 'water':
            made = _molecules(rng, WATER, m // 3)
            c.fixed[lo + 3 * np.arange(3)] = True
        elif role == 'star':
            made = _molecules(rng, STAR, m // 5)
        elif role == 'ring':
            made = _molecules(rng, RING, m // 5)
        elif role == 'one_fixed':
            made = (np.array([[0.2, -0.1, 0.3], [0.2, -0.1, 1.3]]), np.array([[1, 0]]), np.ones(1))
            c.fixed[lo] = True
        elif role == 'none':
            c.fixed[lo + rng.choice(m, m // 5, replace=False)] = True
        elif role == 'failed':
            c.state['status'][g] = 2
            c.vel[lo, 0], c.dE[lo, 2] = np.nan, np.inf
        if made is not None:
            c.pos[lo:lo + m] = made[0]
            pairs.append(made[1] + lo)
            lengths.append(made[2] * (0.9 if role == 'unconverged' else 1.0))
        if role == 'nan':
            c.dE[lo + m // 2, 1] = np.nan
    c.pos = c.pos.astype(np.float32)
    c.pairs, c.lengths = np.concatenate(pairs[::-1]).astype(np.int64), np.concatenate(lengths[::-1])
    c.cons = ConsRef(c.pairs, c.lengths, c.batch, G)
    _MADE['kernel'] = c
    return c


def _subset(c, order):
    """The Case made of the graphs `order` of c, in that order (their constraints keep their relative order)."""
    c2 = Case()
    sizes = [int(c.gptr[g + 1] - c.gptr[g]) for g in order]
    rows = np.concatenate([np.arange(c.gptr[g], c.gptr[g + 1]) for g in order] + [np.zeros(0, np.int64)]).astype(np.int64)
    new_row = np.full(len(c.pos), -1, np.int64)
    new_row[rows] = np.arange(len(rows))
    c2.gptr, c2.batch, c2.roles = _gptr(sizes), np.repeat(np.arange(len(order)), sizes), [c.roles[g] for g in order]
    for k in ('pos', 'vel', 'dE', 'mass', 'fixed'):
        setattr(c2, k, getattr(c, k)[rows])
    for k in ('dt', 'kT', 'gamma'):
        setattr(c2, k, getattr(c, k)[list(order)])
    c2.state = {k: v[list(order)] for k, v in c.state.items()}
    keep = np.isin(c.batch[c.pairs[:, 0]], list(order))
    c2.pairs, c2.lengths = new_row[c.pairs[keep]], c.lengths[keep]
    c2.cons = ConsRef(c2.pairs, c2.lengths, c2.batch, len(order))
    return c2


def _ref(c, kick_in, advance, mass=True):
    """(pos, vel, state, diag) of constrained_step_ref on a case, made once."""
    made, key = c.__dict__.setdefault('refs', {}), (kick_in, advance, mass)
    if key not in made:
        diag = {}
        out = constrained_step_ref(c.pos, c.vel, c.dE, c.gptr, c.state, c.cons, c.dt, c.kT, c.gamma, c.mass if mass else None,
                                   c.fixed, kick_in, advance, TOL, MAX_SWEEPS, diag)
        made[key] = out + (diag,)
    return made[key]


def _project_case():
    """The kernel case for the projection: its positions scattered by 2 % of a bond (so that SHAKE has work), the failed graph
    and the graph that cannot converge as they are."""
    if 'project' not in _MADE:
        c = _kernel_case()
        p = Case()
        p.__dict__.update(c.__dict__)
        p.__dict__.pop('refs', None)
        off = np.random.RandomState(5).uniform(-0.02, 0.02, c.pos.shape)
        off[c.batch == c.roles.index('unconverged')] = 0.0
        p.pos = (c.pos + off).astype(np.float32)
        p.state = dict(status=c.state['status'].copy(), ke=np.full(len(SIZES), -1.0), sweeps=np.full(len(SIZES), -1, np.int32))
        _MADE['project'] = p
    return _MADE['project']


# ------------------------------------------------------------------------------------------- wells with constraints
P_DT, P_STEPS = 0.05, 400
NVE = dict(systems=('chain65', 'water', 'star', 'ring'), k=(1.0, 2.0, 4.0, 1.0), kT=0.0, gamma=0.0, seed=12, steps=P_STEPS)
LAN = dict(systems=('chain65',), k=(1.0,), kT=0.5, gamma=4.0, seed=3, steps=P_STEPS)
DRIFT_FACTOR = 2.5                                # (see _energy_bound)


def _wells(name, spec):
    """Harmonic wells E_g = 1/2 k_g sum |pos - x0|^2 (tests/test_md.py Harmonic) around centres up to 0.3 off a geometry that
    meets the constraints, masses in [1, 16]: the inputs, without a trajectory."""
    if ('wells', name) in _MADE:
        return _MADE[('wells', name)]
    rng = np.random.RandomState(spec['seed'])
    geo = {'chain65': lambda: _chain(rng, 65), 'water': lambda: _molecules(rng, WATER, 1), 'star': lambda: _molecules(rng, STAR, 1),
           'ring': lambda: _molecules(rng, RING, 1)}
    made = [geo[s]() for s in spec['systems']]
    sizes = [len(m[0]) for m in made]
    n, G = sum(sizes), len(sizes)
    h = Case()
    h.gptr, h.batch = _gptr(sizes), np.repeat(np.arange(G), sizes)
    h.pos0 = np.concatenate([m[0] for m in made]).astype(np.float32)
    h.pairs = np.concatenate([m[1] + int(h.gptr[g]) for g, m in enumerate(made)]).astype(np.int64)
    h.lengths = np.concatenate([m[2] for m in made])
    h.cons = ConsRef(h.pairs, h.lengths, h.batch, G)
    h.x0 = (h.pos0 + rng.uniform(-0.3, 0.3, (n, 3))).astype(np.float32)
    h.mass = rng.uniform(1.0, 16.0, n).astype(np.float32)
    h.k = np.asarray(spec['k'], dtype=np.float32)
    h.seeds = spec['seed'] + np.arange(G, dtype=np.int64)
    _MADE[('wells', name)] = h
    return h


def _physics(name, spec):
    """The reference trajectory of _wells from rest at the geometry (NVE: velocity Verlet under constraints; Langevin: from zero
    velocity into the thermostat), dt = 0.05, tol = 1e-10, launch by launch as md.run enqueues it -- the projection of the
    positions, then (0, 1), (1, 1) ..., and a closing (1, 0) -- with epot / ekin / sweeps [steps + 1, G] at the full steps and the
    largest fp64 constraint deviation of any step."""
    if name in _MADE:
        return _MADE[name]
    h = _wells(name, spec)
    n, G = len(h.pos0), len(h.k)
    kk = h.k.astype(np.float64)[h.batch, None]
    steps = spec['steps']
    st = dict(seed=h.seeds, steps=np.zeros(G, np.int32), status=np.zeros(G, np.int32), ke=np.zeros(G), sweeps=np.zeros(G, np.int32))
    pos, _, pst = project_ref(h.pos0, None, h.gptr, st, h.cons, None, h.mass, None, True, False, TOL, 500)
    st.update(pst)
    vel = np.zeros((n, 3), np.float32)
    h.start = pos.copy()
    h.epot, h.ekin, h.sweeps = np.zeros((steps + 1, G)), np.zeros((steps + 1, G)), np.zeros((steps + 1, G), np.int32)
    h.deviation = 0.0
    for it in range(steps + 1):
        d = pos.astype(np.float64) - h.x0
        h.epot[it] = np.bincount(h.batch, weights=0.5 * (kk * d * d).sum(1), minlength=G)
        diag = {}
        pos, vel, st = constrained_step_ref(pos, vel, (kk * d).astype(np.float32), h.gptr, st, h.cons, P_DT, spec['kT'],
                                            spec['gamma'], h.mass, None, 1 if it else 0, 1 if it < steps else 0, TOL, 500, diag)
        h.ekin[it], h.sweeps[it] = st['ke'], st['sweeps']
        h.deviation = max([h.deviation] + [v for k, v in diag.items() if isinstance(k, tuple)])
    h.pos, h.vel, h.state = pos, vel, st
    _MADE[name] = h
    return h


def _energy_bound(h, e0):
    """DRIFT_FACTOR E0 hh / (1 - hh) + 1e-4 E0 per graph, hh = max over the atoms (k_g / m_a) dt^2 / 4.  Without constraints velocity
    Verlet conserves a shadow energy of the well within a factor 1 +- hh exactly (test_md._shadow_bound).  RATTLE is the same
    symmetric second-order scheme on the constraint manifold, so the deviation stays of order dt^2 and bounded, but the
    constraint forces add the centripetal frequencies |v| / d of the rigid parts to the well's sqrt(k / m): the constant is no
    longer 1.  It is set from the reference's own run (the CPU test prints and asserts it: the largest deviation is at most
    0.25 hh E0 / (1 - hh) for every system, 5e-5 .. 2e-4 of E0) with one order of margin: 2.5.  The second term covers 400 fp32
    roundings of pos, as in test_md."""
    hh = np.array([((h.k[g] / h.mass[h.batch == g].astype(np.float64)) * P_DT ** 2 / 4).max() for g in range(len(h.k))])
    return DRIFT_FACTOR * e0 * hh / (1.0 - hh) + 1e-4 * e0


# ---------------------------------------------------------------------------------------------------------- CPU tests
def test_header_declares_the_constraint_entry_points_at_abi_18():
    """(No GPU: the header and the built library.)"""
    import ctypes
    import re
    from pamnet_amd import build, lib
    decl = lib.declared_functions()
    P, D, I64, I32 = ctypes.c_void_p, ctypes.c_double, ctypes.c_int64, ctypes.c_int32
    cons = [P] * 5 + [I64] + [P] * 2 + [D] + [I32]              # cons_i, cons_j, cons_d, gcol, colptr, n_cons, work, sweeps, tol, max
    assert decl[STEP] == [P] * 6 + [I64] * 2 + [P] * 7 + [D] * 3 + [I32] * 2 + cons + [P]
    assert decl[PROJECT] == [P] * 5 + [I64] * 2 + [P] * 3 + [D] + cons + [I32] * 2 + [P]
    assert int(re.search(r'#define\s+PAMNET_ABI_VERSION\s+(\d+)', open(lib.HEADER).read()).group(1)) == 18
    h = ctypes.CDLL(build.build())
    assert h.pamnet_abi_version() == 18 and hasattr(h, STEP) and hasattr(h, PROJECT)


def test_constraint_kernels_are_scratch_free(tmp_path):
    """(No GPU: hipcc cross-compiles.)  The compiler's report for csrc/md_constraints.hip: neither kernel uses scratch (DESIGN
    section 11b quotes the figures)."""
    import os
    import re
    import shutil
    import subprocess
    from pamnet_amd import build
    hipcc = '/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else shutil.which('hipcc')
    assert hipcc, 'hipcc not available'
    r = subprocess.run([hipcc] + build.FLAGS + ['-c', os.path.join(build.CSRC, 'md_constraints.hip'), '-o', str(tmp_path / 'c.o'),
                                                '-Rpass-analysis=kernel-resource-usage'], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for kernel in ('md_constrained_step_kernel', 'md_project_constraints_kernel'):
        blocks = [b for b in re.split(r'remark: Function Name: ', r.stderr)[1:] if kernel in b.split()[0]]
        assert len(blocks) == 1, kernel
        num = lambda key: int(re.search(key + r': (\d+)', blocks[0]).group(1))
        print(kernel, 'VGPRs', num('VGPRs'), 'AGPRs', num('AGPRs'), 'LDS', num(r'LDS Size \[bytes/block\]'))
        assert num(r'ScratchSize \[bytes/lane\]') == 0, kernel


def _cpu_constraints(pairs, batch, lengths=None, pos=None, num_graphs=None):
    from pamnet_amd import synth
    kw = dict(batch=torch.as_tensor(np.asarray(batch, dtype=np.int64)))
    if pos is not None:
        kw['pos'] = torch.as_tensor(np.asarray(pos, dtype=np.float32))
    if num_graphs is not None:
        kw['num_graphs'] = num_graphs
    return Constraints(synth.Batch(**kw), torch.as_tensor(np.asarray(pairs, dtype=np.int64)).reshape(-1, 2),
                       None if lengths is None else torch.as_tensor(np.asarray(lengths, dtype=np.float64)))


def test_colouring_and_refusals():
    """(No GPU.)  A chain takes 2 colours, a triangle and a ring of five 3, a star of four arms 4; no colour holds two constraints
    with a common atom; a graph's colours are the same alone and after other graphs; the arrays Constraints keeps are those of
    the reference for the kernel-test batch (whose pairs arrive with the later graphs first); bond_constraints gives the unique
    pairs that touch the mask; every refusal is a ValueError before anything runs."""
    chain = np.stack([np.arange(9), np.arange(1, 10)], axis=1)
    shapes = {'chain': (chain, 10, 2), 'triangle': (WATER[1], 3, 3), 'ring': (RING[1], 5, 3), 'star': (STAR[1], 5, 4),
              'ring7': (np.stack([np.arange(7), (np.arange(7) + 1) % 7], axis=1), 7, 3)}
    for name, (pairs, m, want) in shapes.items():
        c = _cpu_constraints(pairs, np.zeros(m), np.ones(len(pairs)))
        assert int(c.colour.max()) + 1 == want == int(c.gcol[1]), name
        assert c.n_per_graph.tolist() == [len(pairs)] and c.n == len(pairs)
        ref, _ = colour_ref(pairs, np.zeros(len(pairs), np.int64))
        assert np.array_equal(c.colour, ref[c.order]), name
    # three graphs at once: the star after the chain after the ring, the pairs given star first
    sizes, off = [5, 10, 5], [0, 5, 15]
    pairs = np.concatenate([STAR[1] + 15, chain + 5, RING[1]])
    c = _cpu_constraints(pairs, np.repeat(np.arange(3), sizes), np.ones(len(pairs)))
    assert np.diff(c.gcol.numpy()).tolist() == [3, 2, 4] and c.n_per_graph.tolist() == [5, 9, 4]
    assert np.array_equal(c.graph, np.sort(c.graph)) and c.colptr[-1] == len(pairs) == c.n
    for g, (name, o) in enumerate(zip(('ring', 'chain', 'star'), off)):
        alone = _cpu_constraints(shapes[name][0], np.zeros(shapes[name][1]), np.ones(len(shapes[name][0])))
        sel = c.graph == g
        assert np.array_equal(c.pairs[sel] - o, alone.pairs) and np.array_equal(c.colour[sel], alone.colour), name
    k = _kernel_case()
    c = _cpu_constraints(k.pairs, k.batch, k.lengths, num_graphs=len(SIZES))
    r = k.cons
    for name in ('i', 'j', 'd', 'gcol', 'colptr'):
        assert np.array_equal(getattr(c, name).numpy(), getattr(r, name)), name
    assert c.i.dtype == c.j.dtype == c.gcol.dtype == c.colptr.dtype == torch.int32 and c.d.dtype == torch.float64
    assert np.array_equal(c.order, r.order) and np.array_equal(c.n_per_graph.numpy(), r.n_per_graph)
    assert np.array_equal(k.pairs[c.order], c.pairs) and not np.array_equal(c.order, np.arange(c.n))
    for s in range(len(r.colptr) - 1):                              # inside a colour no atom occurs twice
        atoms = np.concatenate([r.i[r.colptr[s]:r.colptr[s + 1]], r.j[r.colptr[s]:r.colptr[s + 1]]])
        assert len(np.unique(atoms)) == len(atoms) > 0
    per_graph = dict(zip(SIZES, np.diff(r.gcol).tolist()))
    assert per_graph[300] == 2 and per_graph[63] == 3 and per_graph[65] == 4 and per_graph[255] == 3 and per_graph[2] == 1
    assert per_graph[64] == per_graph[1] == per_graph[0] == 0 and per_graph[1025] in (2, 3)
    # lengths=None: the current distances of pos
    pos = np.random.RandomState(0).uniform(-1, 1, (10, 3)).astype(np.float32)
    c = _cpu_constraints(chain, np.zeros(10), pos=pos)
    want = np.linalg.norm(pos[chain[:, 0]].astype(np.float64) - pos[chain[:, 1]], axis=1)[c.order]      # (c.d is sorted)
    assert np.allclose(c.d.numpy(), want, rtol=1e-15, atol=0.0)
    # bond_constraints: both directions of a bond once, only bonds that touch the mask
    ei = torch.tensor([[0, 1, 1, 2, 2, 3, 3, 0, 4, 4], [1, 0, 2, 1, 3, 2, 0, 3, 4, 2]])
    mask = torch.tensor([True, False, False, True, False])
    assert bond_constraints(ei, mask).tolist() == [[0, 1], [0, 3], [2, 3]]
    assert bond_constraints(ei, torch.zeros(5, dtype=torch.bool)).shape == (0, 2)
    assert M.temperature(6.0, 5, remove_com=True, n_constraints=6) == 2.0 and M.temperature(6.0, 5) == 1.0
    # refusals
    batch = np.repeat(np.arange(2), 5)
    bad = [(dict(pairs=[[0, 5]], lengths=[1.0]), 'joins two graphs'), (dict(pairs=[[3, 3]], lengths=[1.0]), 'to itself'),
           (dict(pairs=[[0, 1], [1, 0]], lengths=[1.0, 1.0]), 'twice'), (dict(pairs=[[0, 1], [0, 1]], lengths=[1.0, 1.0]), 'twice'),
           (dict(pairs=[[0, 1]], lengths=[0.0]), 'positive and finite'), (dict(pairs=[[0, 1]], lengths=[-1.0]), 'positive'),
           (dict(pairs=[[0, 1]], lengths=[float('nan')]), 'positive'), (dict(pairs=[[0, 1]], lengths=[float('inf')]), 'positive'),
           (dict(pairs=[[0, 10]], lengths=[1.0]), r'rows in \[0, N\)'), (dict(pairs=[[-1, 2]], lengths=[1.0]), r'rows in \[0, N\)'),
           (dict(pairs=[[0, 1]], lengths=[1.0, 2.0]), r'one per pair'), (dict(pairs=[[0, 1]]), 'need `data.pos`')]
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            _cpu_constraints(kw['pairs'], batch, kw.get('lengths'))
    with pytest.raises(ValueError, match=r'\[C, 2\]'):
        Constraints(torch.as_tensor(batch), torch.zeros(3, 3, dtype=torch.int64), torch.ones(3, dtype=torch.float64))
    with pytest.raises(ValueError, match=r'\[C, 2\]'):
        Constraints(torch.as_tensor(batch), torch.zeros(3, 2), torch.ones(3, dtype=torch.float64))
    with pytest.raises(ValueError, match='coincide'):
        _cpu_constraints([[0, 1]], batch, pos=np.zeros((10, 3)))
    empty = _cpu_constraints(np.zeros((0, 2)), batch, np.zeros(0))
    assert empty.n == 0 and empty.gcol.tolist() == [0, 0, 0] and empty.colptr.tolist() == [0]


def _margins(diag, g):
    """The solves of graph g in a diag: (most sweeps, solves whose verdict is not `converged`, the smallest |err / TOL - 1| of any
    sweep: how far the closest decision of the reference was from falling the other way)."""
    solves = diag.get(g, [])
    errs = np.array([e for _, _, rec in solves for e in rec if np.isfinite(e)] + [np.inf])
    return (max([len(rec) for _, _, rec in solves] + [0]), [(kind, v) for kind, v, _ in solves if v != 0],
            float(np.abs(errs / TOL - 1.0).min()))


def test_kernel_inputs_meet_their_preconditions():
    """(No GPU.)  The kernel-test batch plays every role; under every pair of flags, with masses and without, the reference takes
    the branch the role names; every converging graph takes at most MAX_SWEEPS / 2 sweeps in every solve; the graph meant not
    to converge fails by running out of sweeps (verdict `not yet`, never `broken`) wherever it drifts; no decision of the
    reference is closer than 1e-5 relative to the bound (an err near 1e-10 of quantities of order 1 carries roundings near 1e-16, 1e-6 of
    it: fp64 arithmetic in another order decides alike); the
    projection case likewise."""
    c = _kernel_case()
    assert [int(b - a) for a, b in zip(c.gptr[:-1], c.gptr[1:])] == SIZES and set(c.roles) == set(ROLE_OF.values())
    assert float(np.abs(c.pos).max()) < 1.9
    n_cons = dict(zip(SIZES, c.cons.n_per_graph.tolist()))
    assert n_cons[300] == 299 and n_cons[1025] == 1024 and n_cons[63] == 63 and n_cons[65] == 52 and n_cons[255] == 255
    assert n_cons[2] == 1 and n_cons[64] == n_cons[1] == n_cons[0] == 0
    assert c.fixed[c.cons.i].sum() + c.fixed[c.cons.j].sum() == 7 and not (c.fixed[c.cons.i] & c.fixed[c.cons.j]).any()
    most_seen = 0
    for kick_in, advance in FLAGS:
        for mass in (True, False):
            pos, vel, st, diag = _ref(c, kick_in, advance, mass)
            for g, role in enumerate(c.roles):
                s = slice(int(c.gptr[g]), int(c.gptr[g + 1]))
                most, not_ok, margin = _margins(diag, g)
                same = np.array_equal(pos[s], c.pos[s]) and np.array_equal(vel[s], c.vel[s], equal_nan=True)
                tag = (role, kick_in, advance, mass)
                if role == 'failed':
                    assert st['status'][g] == 2 and same and st['sweeps'][g] == -1 and st['ke'][g] == -1.0, tag
                elif role == 'nan':
                    assert st['status'][g] == 2 and same and st['sweeps'][g] == 0 and st['steps'][g] == c.state['steps'][g], tag
                elif role == 'unconverged' and advance:            # the velocity solves converge: the stretched drift does not
                    assert st['status'][g] == 3 and same and st['steps'][g] == c.state['steps'][g], tag
                    assert st['sweeps'][g] == MAX_SWEEPS and not_ok == [('shake', 1)], (tag, not_ok)
                else:
                    assert st['status'][g] == 0 and st['steps'][g] == c.state['steps'][g] + advance and not not_ok, tag
                    assert st['sweeps'][g] == most <= MAX_SWEEPS // 2, (tag, most)
                    assert (st['sweeps'][g] > 0) == (role not in ('none', 'empty') and bool(advance or kick_in)), tag
                    most_seen = max(most_seen, most)
                    assert same == (role in ('empty', 'unconverged') or not (advance or kick_in)), tag
                if role not in ('failed', 'nan', 'empty', 'none'):
                    assert margin >= 1e-5, (tag, margin)
    print('most sweeps of a converging graph', most_seen, 'of', MAX_SWEEPS)
    assert most_seen > 8
    p = _project_case()
    for do_pos, do_vel in ((1, 1), (1, 0), (0, 1)):
        diag = {}
        pos, vel, st = project_ref(p.pos, p.vel, p.gptr, p.state, p.cons, p.dt, p.mass, p.fixed, do_pos, do_vel, TOL, MAX_SWEEPS, diag)
        for g, role in enumerate(p.roles):
            most, not_ok, margin = _margins(diag, g)
            if role == 'failed':
                assert st['status'][g] == 2 and st['sweeps'][g] == -1
            elif role == 'unconverged' and do_pos:
                assert st['status'][g] == 3 and st['sweeps'][g] == MAX_SWEEPS and not_ok == [('shake', 1)]
            else:
                assert st['status'][g] == 0 and most <= MAX_SWEEPS // 2, (role, most)
            if role not in ('failed', 'empty', 'none'):
                assert margin >= 1e-5, (role, do_pos, do_vel, margin)


def test_reference_physics():
    """(No GPU; tests of the reference.)  Wells plus constraints, dt = 0.05, 400 steps, tol = 1e-10.  NVE from rest -- a chain of 65,
    a water triangle, a four-arm star, a ring of five: epot + ekin stays within _energy_bound of its start, the wells swing, and
    the fp64 constraint deviation at the end of every step is at most 10 tol.  Langevin, a chain of 65 at kT = 0.5: the mean of
    temperature(ekin, 65, remove_com=False, n_constraints=64) over records 100..400 is within 2.5 % of kT, and counted with 3 N
    it is more than 20 % low."""
    h = _physics('nve', NVE)
    e = h.epot + h.ekin
    assert (h.state['status'] == 0).all() and (h.state['steps'] == P_STEPS).all()
    drift, bound = np.abs(e - e[0]).max(0), _energy_bound(h, e[0])
    hh = (bound - 1e-4 * e[0]) / DRIFT_FACTOR
    print('NVE reference: energy', e[0], 'largest deviation', drift, 'over E0', drift / e[0], 'over hh E0 / (1 - hh)', drift / hh,
          'bound', bound, 'most sweeps', h.sweeps.max(0), 'constraint deviation', h.deviation)
    assert (drift <= bound).all() and (drift > 0).all() and (drift / hh < DRIFT_FACTOR / 10.0).all()
    assert (h.ekin.max(0) > 0.1 * e[0]).all()
    assert 0.0 < h.deviation <= 10 * TOL
    assert (h.sweeps[:-1] > 0).all() and h.sweeps.max() <= 250
    lan = _physics('lan', LAN)
    N, C = 65, 64
    ek = lan.ekin[100:, 0]
    kT = float(M.temperature(ek, N, remove_com=False, n_constraints=C).mean())
    kT3n = float(M.temperature(ek, N, remove_com=False).mean())
    print('Langevin reference: kT', kT, 'relative error', kT / LAN['kT'] - 1.0, 'counted with 3 N', kT3n, 'deviation', lan.deviation)
    assert (lan.state['status'] == 0).all() and lan.deviation <= 10 * TOL
    assert abs(kT / LAN['kT'] - 1.0) < 0.025
    assert kT3n / LAN['kT'] < 0.8


# ------------------------------------------------------------------------------------------------------- kernel tests
def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _device_cons(dev, c, lengths=True):
    """The Constraints of a case on the device (lengths=False: the current distances of its positions)."""
    from pamnet_amd import synth
    data = synth.Batch(batch=_t(dev, c.batch.astype(np.int64)), pos=_t(dev, c.pos), num_graphs=len(c.gptr) - 1)
    return Constraints(data, _t(dev, c.pairs.reshape(-1, 2)), _t(dev, c.lengths) if lengths else None)


def _step_on_device(dev, c, kick_in, advance, mass=True, cons=None, entry='constrained'):
    """One launch on a case -> (pos, vel, state) as numpy.  entry='plain': pamnet_md_step_f32 on the same inputs."""
    pos, vel, dE = _t(dev, c.pos), _t(dev, c.vel), _t(dev, c.dE)
    state = {k: _t(dev, c.state[k]) for k in STATE}
    args = (_t(dev, c.dt), _t(dev, c.kT), _t(dev, c.gamma), _t(dev, c.mass) if mass else None, _t(dev, c.fixed.astype(np.uint8)),
            kick_in, advance)
    if entry == 'plain':
        M.md_step(pos, vel, dE, _t(dev, c.gptr), state, *args)
    else:
        M.constrained_step(pos, vel, dE, _t(dev, c.gptr), state, cons if cons is not None else _device_cons(dev, c), *args,
                           tol=TOL, max_sweeps=MAX_SWEEPS)
    return pos.cpu().numpy(), vel.cpu().numpy(), {k: v.cpu().numpy() for k, v in state.items()}


def _lengths_err(pos, cons, g):
    """The largest relative deviation of the constrained distances of graph g in (fp32) positions."""
    sel = cons.graph == g
    if not sel.any():
        return 0.0
    p = pos.astype(np.float64)
    d = np.sqrt(((p[cons.i[sel]] - p[cons.j[sel]]) ** 2).sum(1))
    return float(np.abs(d / cons.d[sel] - 1.0).max())


def _assert_matches(got, want, before, gptr, fixed, cons, advance, tag=''):
    """got / want / before: (pos, vel, state); the checks of one launch against constrained_step_ref."""
    (gp, gv, gs), (wp, wv, ws), (bp, bv, bs) = got, want, before
    for k in ('status', 'steps', 'sweeps', 'seed'):
        assert np.array_equal(gs[k], ws[k]), (tag, k, gs[k], ws[k])
    worst = [0.0, 0.0, 0.0]
    for g in range(len(gptr) - 1):
        s = slice(int(gptr[g]), int(gptr[g + 1]))
        gk, wk = gs['ke'][g], ws['ke'][g]
        if np.isfinite(wk):
            assert abs(gk - wk) <= 1e-12 * abs(wk), (tag, g, gk, wk)
        else:
            assert np.isnan(gk) == np.isnan(wk) and np.isinf(gk) == np.isinf(wk), (tag, g, gk, wk)
        if bs['status'][g] != 0 or ws['status'][g] != 0:           # left alone, failed or unconverged: bit for bit the input
            assert np.array_equal(gp[s], bp[s], equal_nan=True) and np.array_equal(gv[s], bv[s], equal_nan=True), (tag, g)
            continue
        if s.stop == s.start:
            continue
        fx = fixed[s]
        assert np.array_equal(gp[s][fx], bp[s][fx]) and np.array_equal(gv[s][fx], bv[s][fx]), (tag, g, 'fixed rows')
        ev = maxnorm_err(gv[s][~fx], wv[s][~fx])
        if advance:
            want_d = wp[s].astype(np.float64) - bp[s]
            assert float(np.abs(want_d).max()) > 0
            ed = maxnorm_err(gp[s].astype(np.float64) - bp[s], want_d)
            el = _lengths_err(gp, cons, g)
        else:
            assert np.array_equal(gp[s], bp[s]), (tag, g, 'pos')
            ed = el = 0.0
        worst = [max(worst[0], ev), max(worst[1], ed), max(worst[2], el)]
        assert ev <= KTOL and ed <= KTOL and el <= LENGTH_TOL, (tag, g, ev, ed, el)
    return worst


@pytest.mark.gpu
def test_one_launch_on_a_batch_vs_the_reference(dev):
    """Graphs of 1 .. 1025 and 0 atoms in the roles of _kernel_case, per-graph dt / kT / gamma, under every (kick_in, advance), with
    masses and with NULL: status, steps and sweeps equal, ke to 1e-12, vel and the displacement within KTOL per graph, the
    constrained distances of the stored positions within 1e-6; rows of fixed atoms, of the failed graph, of the graph with a NaN
    force and of the graph that does not converge bit for bit the input."""
    c = _kernel_case()
    cons = _device_cons(dev, c)
    worst = [0.0, 0.0, 0.0]
    for kick_in, advance in FLAGS:
        for mass in (True, False):
            got = _step_on_device(dev, c, kick_in, advance, mass, cons)
            w = _assert_matches(got, _ref(c, kick_in, advance, mass)[:3], (c.pos, c.vel, c.state), c.gptr, c.fixed, c.cons, advance,
                                tag=(kick_in, advance, mass))
            worst = [max(a, b) for a, b in zip(worst, w)]
    print('worst vel / displacement / length error', worst)
    assert worst[2] > 0.0                                          # (fp32 positions do not meet a length exactly: it was measured)


@pytest.mark.gpu
def test_graphs_without_constraints_take_the_plain_step_bitwise(dev):
    """Under every pair of flags: the graphs of the batch that have no constraints equal a launch of pamnet_md_step_f32 on the same
    inputs bit for bit; and with an empty Constraints every graph does, the failing one included (sweeps 0 where a graph ran)."""
    c = _kernel_case()
    cons, empty = _device_cons(dev, c), _device_cons(dev, _subset(c, [c.roles.index('none')]))
    n, G = len(c.pos), len(SIZES)
    from pamnet_amd import synth
    none = Constraints(synth.Batch(batch=_t(dev, c.batch.astype(np.int64)), num_graphs=G),
                       torch.zeros(0, 2, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.float64, device=dev))
    assert empty.n == 0 and none.n == 0 and none.n_atoms == n
    checked = 0
    for kick_in, advance in FLAGS:
        plain = _step_on_device(dev, c, kick_in, advance, entry='plain')
        mixed = _step_on_device(dev, c, kick_in, advance, cons=cons)
        bare = _step_on_device(dev, c, kick_in, advance, cons=none)
        for g, role in enumerate(c.roles):
            s = slice(int(c.gptr[g]), int(c.gptr[g + 1]))
            for got in ((mixed,) if role in ('none', 'failed', 'empty') else ()) + (bare,):
                assert np.array_equal(got[0][s], plain[0][s]) and np.array_equal(got[1][s], plain[1][s], equal_nan=True), (role, g)
                for k in ('steps', 'status'):
                    assert got[2][k][g] == plain[2][k][g], (role, k)
                assert got[2]['ke'][g] == plain[2]['ke'][g] or np.isnan(plain[2]['ke'][g]), role
                assert got[2]['sweeps'][g] == (-1 if role == 'failed' else 0), role
            checked += int(role == 'none' and advance and not np.array_equal(plain[0][s], c.pos[s]))
    assert checked == 2


@pytest.mark.gpu
def test_a_launch_is_repeatable_and_independent_of_the_batch(dev):
    """Every graph of the kernel case stepped alone, inside the batch in three rotations of its order, and twice over: its rows
    of pos and vel, its ke, steps, status and sweeps are equal bit for bit in all of them."""
    c = _kernel_case()
    G = len(SIZES)
    alone = []
    for g in range(G):
        p, v, st = _step_on_device(dev, _subset(c, [g]), 1, 1)
        alone.append((p, v, {k: st[k][0] for k in ('ke', 'steps', 'status', 'sweeps')}))
    for rot in (0, 4, 7, 0):
        order = list(range(rot, G)) + list(range(rot))
        c2 = _subset(c, order)
        p, v, st = _step_on_device(dev, c2, 1, 1)
        for j, g in enumerate(order):
            s = slice(int(c2.gptr[j]), int(c2.gptr[j + 1]))
            assert np.array_equal(p[s], alone[g][0], equal_nan=True) and np.array_equal(v[s], alone[g][1], equal_nan=True), (rot, g)
            for k, want in alone[g][2].items():
                assert st[k][j] == want or (k == 'ke' and np.isnan(want) and np.isnan(st[k][j])), (rot, g, k)
    moved = [g for g in range(G) if alone[g][2]['status'] == 0 and SIZES[g] > 0]
    assert len(moved) == 7 and all(not np.array_equal(alone[g][0], c.pos[c.gptr[g]:c.gptr[g + 1]]) for g in moved)


def _project_on_device(dev, p, cons, do_pos, do_vel, vel=None, fixed=True, tol=TOL):
    pos, v = _t(dev, p.pos), _t(dev, p.vel if vel is None else vel)
    state = {k: _t(dev, p.state[k]) for k in ('status', 'ke', 'sweeps')}
    M.project_constraints(pos, v, _t(dev, p.gptr), state, cons, _t(dev, p.dt), _t(dev, p.mass),
                          _t(dev, p.fixed.astype(np.uint8)) if fixed else None, do_pos, do_vel, tol, MAX_SWEEPS)
    return pos.cpu().numpy(), v.cpu().numpy(), {k: x.cpu().numpy() for k, x in state.items()}


@pytest.mark.gpu
def test_the_projection_vs_the_reference(dev):
    """pamnet_md_project_constraints_f32 on the kernel case with its positions scattered, under (do_pos, do_vel) = (1, 1), (1, 0),
    (0, 1): status and sweeps equal, ke to 1e-12 (untouched without do_vel), the displacement and the velocities within KTOL
    per graph, the projected distances within 1e-6, what a flag leaves out and the rows of fixed atoms, of the failed graph and
    of the graph that does not converge bit for bit the input.  Then a state that meets its constraints -- the lengths taken
    from the positions themselves, one velocity per graph, nothing fixed: one sweep per solve, nothing moves by more than
    1e-12, ke = 1/2 sum m |v|^2."""
    p = _project_case()
    cons = _device_cons(dev, p)
    for do_pos, do_vel in ((1, 1), (1, 0), (0, 1)):
        gp, gv, gs = _project_on_device(dev, p, cons, do_pos, do_vel)
        wp, wv, ws = project_ref(p.pos, p.vel, p.gptr, p.state, p.cons, p.dt, p.mass, p.fixed, do_pos, do_vel, TOL, MAX_SWEEPS)
        assert np.array_equal(gs['status'], ws['status']) and np.array_equal(gs['sweeps'], ws['sweeps']), (do_pos, do_vel)
        if not do_pos:
            assert np.array_equal(gp, p.pos)
        if not do_vel:
            assert np.array_equal(gv, p.vel, equal_nan=True) and np.array_equal(gs['ke'], p.state['ke'])
        for g, role in enumerate(p.roles):
            s = slice(int(p.gptr[g]), int(p.gptr[g + 1]))
            tag = (role, do_pos, do_vel)
            if do_vel and ws['status'][g] == 0:
                assert abs(gs['ke'][g] - ws['ke'][g]) <= 1e-12 * abs(ws['ke'][g]), tag
            if ws['status'][g] != 0:
                assert np.array_equal(gp[s], p.pos[s]) and np.array_equal(gv[s], p.vel[s], equal_nan=True), tag
                assert gs['ke'][g] == -1.0, tag
                continue
            fx = p.fixed[s]
            assert np.array_equal(gp[s][fx], p.pos[s][fx]) and np.array_equal(gv[s][fx], p.vel[s][fx]), tag
            if role in ('none', 'empty'):
                assert np.array_equal(gp[s], p.pos[s]) and np.array_equal(gv[s], p.vel[s]) and gs['sweeps'][g] == 0, tag
                continue
            if do_pos:
                want_d = wp[s].astype(np.float64) - p.pos[s]
                assert float(np.abs(want_d).max()) > 0 and maxnorm_err(gp[s].astype(np.float64) - p.pos[s], want_d) <= KTOL, tag
                assert _lengths_err(gp, p.cons, g) <= LENGTH_TOL, tag
            if do_vel and role != 'unconverged':
                assert not np.array_equal(gv[s], p.vel[s]) and maxnorm_err(gv[s][~fx], wv[s][~fx]) <= KTOL, tag
    met = _device_cons(dev, p, lengths=False)
    u = np.random.RandomState(8).standard_normal((len(SIZES), 3)).astype(np.float32)[p.batch]
    gp, gv, gs = _project_on_device(dev, p, met, 1, 1, vel=u, fixed=False)
    m = p.mass.astype(np.float64)
    for g, role in enumerate(p.roles):
        s = slice(int(p.gptr[g]), int(p.gptr[g + 1]))
        if role == 'failed':
            assert gs['status'][g] == 2 and gs['sweeps'][g] == -1
            continue
        assert gs['status'][g] == 0 and gs['sweeps'][g] == (0 if role in ('none', 'empty') else 1), (role, gs['sweeps'][g])
        assert np.abs(gp[s].astype(np.float64) - p.pos[s]).max(initial=0.0) <= 1e-12, role
        assert np.abs(gv[s].astype(np.float64) - u[s]).max(initial=0.0) <= 1e-12, role
        want = 0.5 * float((m[s, None] * u[s].astype(np.float64) ** 2).sum())
        assert abs(gs['ke'][g] - want) <= 1e-12 * want, role


@pytest.mark.gpu
def test_the_entry_points_validate_their_arguments(dev):
    """Both entry points: what pamnet_md_step_f32 refuses; a null sweeps, and with n_cons > 0 a null cons_i / cons_j / cons_d /
    gcol / colptr / work, are PAMNET_ENULL; tol not positive and finite, max_sweeps < 1, n_cons < 0 and a flag other than 0 / 1
    are PAMNET_EINVAL; with n_cons == 0 the constraint arrays may be NULL; the projection needs vel, ke and dt only with do_vel.
    Every graph has failed already: no launch of this test touches anything."""
    from pamnet_amd import lib
    c = _kernel_case()
    G, n = len(SIZES), len(c.pos)
    cons = _device_cons(dev, c)
    pos, vel, dE, gptr, mass = _t(dev, c.pos), _t(dev, c.vel), _t(dev, c.dE), _t(dev, c.gptr), _t(dev, c.mass)
    st = {k: _t(dev, c.state[k]) for k in STATE}
    st['status'].fill_(2)
    dt_g, zeros = _t(dev, c.dt), _t(dev, np.zeros(G))
    nan, inf = float('nan'), float('inf')
    base = dict(pos=lib.ptr(pos), vel=lib.ptr(vel), dpos=lib.ptr(dE), mass=None, fixed=None, gptr=lib.ptr(gptr), n=n, G=G,
                dt_g=None, kT_g=None, gamma_g=None, dt=0.05, kT=0.5, gamma=1.0, kick_in=1, advance=1, cons_i=lib.ptr(cons.i),
                cons_j=lib.ptr(cons.j), cons_d=lib.ptr(cons.d), gcol=lib.ptr(cons.gcol), colptr=lib.ptr(cons.colptr),
                n_cons=cons.n, work=lib.ptr(cons.work()), tol=1e-8, max_sweeps=100, do_pos=1, do_vel=1)
    base.update({k: lib.ptr(st[k]) for k in STATE})

    def step(**kw):
        a = dict(base)
        a.update(kw)
        lib.call(STEP, a['pos'], a['vel'], a['dpos'], a['mass'], a['fixed'], a['gptr'], a['n'], a['G'], a['seed'], a['steps'],
                 a['status'], a['ke'], a['dt_g'], a['kT_g'], a['gamma_g'], a['dt'], a['kT'], a['gamma'], a['kick_in'], a['advance'],
                 a['cons_i'], a['cons_j'], a['cons_d'], a['gcol'], a['colptr'], a['n_cons'], a['work'], a['sweeps'], a['tol'],
                 a['max_sweeps'], lib.stream_of(pos))

    def project(**kw):
        a = dict(base)
        a.update(kw)
        lib.call(PROJECT, a['pos'], a['vel'], a['mass'], a['fixed'], a['gptr'], a['n'], a['G'], a['status'], a['ke'], a['dt_g'],
                 a['dt'], a['cons_i'], a['cons_j'], a['cons_d'], a['gcol'], a['colptr'], a['n_cons'], a['work'], a['sweeps'],
                 a['tol'], a['max_sweeps'], a['do_pos'], a['do_vel'], lib.stream_of(pos))

    solver_null = ('sweeps', 'cons_i', 'cons_j', 'cons_d', 'gcol', 'colptr', 'work')
    solver_inval = (dict(tol=0.0), dict(tol=-1e-8), dict(tol=nan), dict(tol=inf), dict(max_sweeps=0), dict(max_sweeps=-3),
                    dict(n_cons=-1), dict(n=-1), dict(G=-1), dict(G=2 ** 31), dict(dt=0.0), dict(dt=-0.1), dict(dt=nan), dict(dt=inf))
    for k in ('pos', 'vel', 'dpos', 'gptr', 'seed', 'steps', 'status', 'ke') + solver_null:
        with pytest.raises(RuntimeError, match='PAMNET_ENULL'):
            step(**{k: None})
    with pytest.raises(RuntimeError, match='PAMNET_ENULL'):
        step(seed=None, gamma=0.0, gamma_g=lib.ptr(zeros))
    for kw in solver_inval + (dict(kick_in=2), dict(kick_in=-1), dict(advance=2), dict(kT=-1.0), dict(kT=nan), dict(kT=inf),
                              dict(gamma=-1.0), dict(gamma=nan), dict(gamma=inf)):
        with pytest.raises(RuntimeError, match='PAMNET_EINVAL'):
            step(**kw)
    for k in ('pos', 'vel', 'gptr', 'status', 'ke') + solver_null:
        with pytest.raises(RuntimeError, match='PAMNET_ENULL'):
            project(**{k: None})
    for kw in solver_inval + (dict(do_pos=2), dict(do_vel=-1), dict(do_pos=-1), dict(do_vel=2)):
        with pytest.raises(RuntimeError, match='PAMNET_EINVAL'):
            project(**kw)
    none = dict(cons_i=None, cons_j=None, cons_d=None, gcol=None, colptr=None, work=None, n_cons=0)
    step(G=0)
    project(G=0)
    step()
    project()
    step(**none)                                                   # without constraints none of their arrays is needed
    project(**none)
    step(seed=None, gamma=0.0)
    step(dt_g=lib.ptr(dt_g), dt=nan, kT_g=lib.ptr(zeros), kT=-1.0, gamma_g=lib.ptr(zeros), gamma=inf, mass=lib.ptr(mass))
    project(do_vel=0, vel=None, ke=None, dt=nan)                   # the projection of the positions alone
    project(dt_g=lib.ptr(dt_g), dt=nan)
    torch.cuda.synchronize()
    assert torch.equal(pos, _t(dev, c.pos)) and torch.equal(vel.nan_to_num(1.0, 2.0, 3.0), _t(dev, c.vel).nan_to_num(1.0, 2.0, 3.0))
    assert all(torch.equal(st[k], _t(dev, c.state[k])) for k in ('seed', 'steps', 'ke', 'sweeps')) and (st['status'] == 2).all()


# ----------------------------------------------------------------------------------------------------- end to end
def _replay(res, gptr, cons, dt, kT, gamma, mass, fixed, steps, tol, max_sweeps):
    """Every launch of a trace through constrained_step_ref from its recorded inputs; consecutive launches hand on what they
    stored."""
    cpu = lambda t: None if t is None else t.cpu().numpy()
    worst = [0.0, 0.0, 0.0]
    assert len(res.trace) == steps + 1
    for i, r in enumerate(res.trace):
        assert (r['kick_in'], r['advance']) == (1 if i else 0, 1 if i < steps else 0)
        assert set(r['state_before']) == set(STATE) == set(r['state_after'])
        before = (cpu(r['pos']), cpu(r['v_before']), {k: cpu(v) for k, v in r['state_before'].items()})
        got = (cpu(r['pos_after']), cpu(r['v_after']), {k: cpu(v) for k, v in r['state_after'].items()})
        want = constrained_step_ref(before[0], before[1], cpu(r['dE']), gptr, before[2], cons, dt, kT, gamma, mass, fixed,
                                    r['kick_in'], r['advance'], tol, max_sweeps)
        w = _assert_matches(got, want, before, gptr, np.zeros(len(before[0]), bool) if fixed is None else fixed, cons,
                            r['advance'], tag=i)
        worst = [max(a, b) for a, b in zip(worst, w)]
        if i + 1 < len(res.trace):
            assert torch.equal(r['pos_after'], res.trace[i + 1]['pos']) and torch.equal(r['v_after'], res.trace[i + 1]['v_before'])
    assert torch.equal(res.trace[-1]['pos_after'], res.pos) and torch.equal(res.trace[-1]['v_after'], res.vel)
    assert torch.equal(res.trace[-1]['state_after']['ke'], res.kinetic)
    assert torch.equal(res.trace[-1]['state_after']['sweeps'], res.sweeps)
    return worst


def _well(dev, h):
    from pamnet_amd import synth
    model = Harmonic(torch.from_numpy(h.k), torch.from_numpy(h.x0)).to(dev)
    data = synth.Batch(pos=torch.from_numpy(h.pos0), batch=torch.from_numpy(h.batch), num_graphs=len(h.k)).to(dev)
    return model, data, Constraints(data, _t(dev, h.pairs), _t(dev, h.lengths))


REPLAYED = 40                                     # steps of the traced runs (the replay costs a reference step per launch)


@pytest.mark.gpu
def test_constrained_wells_conserve_their_energy(dev):
    """md.run with constraints on the NVE wells of the CPU test (a chain of 65, a water triangle, a star, a ring of five), from
    rest, dt = 0.05, tol = 1e-10: over 400 steps epot + ekin of every record stays within _energy_bound of the first, nothing is
    unconverged, the first record is the reference's projection of the start, and the constrained distances of res.pos are
    within 1e-6.  The same run over 40 steps with trace=True is replayed launch by launch through constrained_step_ref within
    KTOL, with equal sweeps; its records are the first 41 of the long run, bit for bit."""
    from pamnet_amd.md import run
    h = _wells('nve', NVE)
    model, data, cons = _well(dev, h)
    mass, steps = _t(dev, h.mass), NVE['steps']
    res = run(model, data, steps, P_DT, masses=mass, record_every=1, constraints=cons, constraint_tol=TOL)
    assert res.steps.tolist() == [steps] * 4 and not res.failed.any() and not res.unconverged.any()
    assert res.unconverged.dtype == torch.bool and res.sweeps.dtype == torch.int32 and (res.sweeps > 0).all()
    assert torch.equal(data.pos.cpu(), torch.from_numpy(h.pos0))
    st = dict(status=np.zeros(4, np.int32), ke=np.zeros(4), sweeps=np.zeros(4, np.int32))
    start, _, _ = project_ref(h.pos0, None, h.gptr, st, h.cons, None, h.mass, None, True, False, TOL, 500)
    assert maxnorm_err(res.frames[0].cpu().numpy(), start) <= KTOL
    e = (res.epot + res.ekin).cpu().numpy()
    drift, bound = np.abs(e - e[0]).max(0), _energy_bound(h, e[0])
    print('constrained NVE wells: energy', e[0], 'largest deviation', drift, 'bound', bound)
    assert (drift <= bound).all() and (drift > 0).all()
    final = res.pos.cpu().numpy()
    assert max(_lengths_err(final, h.cons, g) for g in range(4)) <= LENGTH_TOL
    short = run(model, data, REPLAYED, P_DT, masses=mass, record_every=1, constraints=cons, constraint_tol=TOL, trace=True)
    worst = _replay(short, h.gptr, h.cons, P_DT, 0.0, 0.0, h.mass, None, REPLAYED, TOL, 500)
    print('constrained NVE wells: worst vel / displacement / length error of the replay', worst)
    assert torch.equal(short.frames, res.frames[:REPLAYED + 1]) and torch.equal(short.epot, res.epot[:REPLAYED + 1])
    assert torch.equal(short.ekin[:REPLAYED], res.ekin[:REPLAYED])


@pytest.mark.gpu
def test_a_constrained_chain_in_the_thermostat_is_replayed(dev):
    """Langevin on the chain of 65 of the CPU test (kT = 0.5, gamma = 4), Maxwell-Boltzmann start: the starting velocities are
    init_velocities_ref's projected by project_ref, and every launch of 40 steps replayed through constrained_step_ref is
    within KTOL with equal sweeps; the velocity along every constraint of res.vel is gone."""
    from pamnet_amd.md import run
    h = _wells('lan', LAN)
    model, data, cons = _well(dev, h)
    res = run(model, data, REPLAYED, P_DT, masses=_t(dev, h.mass), kT=LAN['kT'], gamma=LAN['gamma'], seed=LAN['seed'],
              remove_com=False, constraints=cons, constraint_tol=TOL, trace=True)
    assert res.steps.tolist() == [REPLAYED] and not res.failed.any() and not res.unconverged.any()
    st = dict(status=np.zeros(1, np.int32), ke=np.zeros(1), sweeps=np.zeros(1, np.int32))
    start, _, _ = project_ref(h.pos0, None, h.gptr, st, h.cons, None, h.mass, None, True, False, TOL, 500)
    v0, _ = init_velocities_ref(np.zeros((65, 3), np.float32), h.gptr, h.seeds, LAN['kT'], h.mass, None, False, False)
    _, v0p, _ = project_ref(start, v0, h.gptr, st, h.cons, P_DT, h.mass, None, False, True, TOL, 500)
    assert maxnorm_err(res.trace[0]['v_before'].cpu().numpy(), v0p) <= KTOL and not np.array_equal(v0, v0p)
    worst = _replay(res, h.gptr, h.cons, P_DT, LAN['kT'], LAN['gamma'], h.mass, None, REPLAYED, TOL, 500)
    print('constrained Langevin chain: worst vel / displacement / length error of the replay', worst)
    p, v = res.pos.cpu().numpy().astype(np.float64), res.vel.cpu().numpy().astype(np.float64)
    r, u = p[h.cons.i] - p[h.cons.j], v[h.cons.i] - v[h.cons.j]
    assert np.abs((r * u).sum(1)).max() <= 1e-5 * np.abs(u).max()  # (fp32 velocities: 6e-8 relative per component)


_MASS_OF_TYPE = (1.008, 12.011, 14.007, 15.999, 18.998)            # H, C, N, O, F (the QM9 schema's type index)


def _qm9_case():
    """Four molecules of synth.qm9_molecule(3, .) -- the first four whose coordinates stay below 3.2, so that a stored fp32
    coordinate is rounded by at most 2.4e-7 and a constrained distance by less than 1e-6 -- with the X-H bonds as constraints."""
    if 'qm9' not in _MADE:
        from pamnet_amd import synth
        mols = [m for m in (synth.qm9_molecule(3, i) for i in range(60)) if np.abs(m['pos']).max() < 3.2][:4]
        assert len(mols) == 4
        b = synth.collate(mols)
        pairs = bond_constraints(b.edge_index, b.x == 0)
        _MADE['qm9'] = (b, pairs, torch.tensor(_MASS_OF_TYPE, dtype=torch.float32)[b.x.long()])
    return _MADE['qm9']


@pytest.mark.gpu
@pytest.mark.parametrize('dim,n_layer', MODELS)
def test_pamnet_dynamics_with_frozen_hydrogen_bonds(dev, dim, n_layer):
    """PAMNet on four QM9-schema molecules with every X-H bond constrained at its starting length (bond_constraints of the
    hydrogens), 5 Langevin steps from a Maxwell-Boltzmann start with per-graph seeds, trace=True: every launch replayed through
    constrained_step_ref from its recorded inputs matches as in the kernel test; the constrained distances of res.pos are within
    1e-6 of their lengths; res.energy / res.forces are bitwise a fresh evaluation at res.pos.  Without constraints the run is
    bitwise the run with an empty Constraints, whose graphs take the plain step."""
    import copy
    import models
    from pamnet_amd.md import run
    b, pairs, mass_cpu = _qm9_case()
    torch.manual_seed(0)
    model = models.PAMNet(models.Config(dataset='QM9', dim=dim, n_layer=n_layer, cutoff_l=5.0, cutoff_g=5.0)).to(dev)
    data, mass = b.to(dev), mass_cpu.to(dev)
    cons = Constraints(data, pairs.to(dev))
    n_h = int((b.x == 0).sum())
    assert cons.n == n_h > 20 and int(cons.n_per_graph.sum()) == n_h and (cons.n_per_graph > 0).all()
    pos0 = data.pos.clone()
    seeds = torch.tensor([11, -5, 2 ** 40 + 3, 7], dtype=torch.int64, device=dev)
    kw = dict(masses=mass, kT=0.05, gamma=1.0, seed=seeds)
    res = run(model, data, 5, 0.05, trace=True, constraints=cons, **kw)
    assert torch.equal(data.pos, pos0) and res.steps.tolist() == [5] * 4 and not res.failed.any() and not res.unconverged.any()
    gptr = np.concatenate([[0], np.cumsum(np.bincount(b.batch.numpy(), minlength=4))])
    pr, x = pairs.numpy(), b.pos.numpy().astype(np.float64)
    ref = ConsRef(pr, np.sqrt(((x[pr[:, 0]] - x[pr[:, 1]]) ** 2).sum(1)), b.batch.numpy(), 4)
    assert np.allclose(ref.d, cons.d.cpu().numpy(), rtol=1e-14, atol=0.0) and np.array_equal(ref.i, cons.i.cpu().numpy())
    worst = _replay(res, gptr, ref, 0.05, 0.05, 1.0, mass_cpu.numpy(), None, 5, 1e-8, 500)
    print('replay: worst vel / displacement / length error', worst, 'sweeps', res.sweeps.tolist())
    p = res.pos.cpu().numpy().astype(np.float64)
    d = np.sqrt(((p[ref.i] - p[ref.j]) ** 2).sum(1))
    assert np.abs(d - ref.d).max() <= 1e-6 and not torch.equal(res.pos, pos0)
    at = copy.copy(data)
    at.pos = res.pos.clone().requires_grad_(True)
    e = model(at)
    de, = torch.autograd.grad(e.sum(), at.pos)
    assert torch.equal(res.energy, e.detach()) and torch.equal(res.forces, -de) and torch.isfinite(res.forces).all()
    plain = run(model, data, 5, 0.05, **kw)
    empty = run(model, data, 5, 0.05, constraints=Constraints(data, torch.zeros(0, 2, dtype=torch.int64, device=dev)), **kw)
    assert not hasattr(plain, 'sweeps') and empty.sweeps.tolist() == [0] * 4 and not empty.unconverged.any()
    for k in ('pos', 'vel', 'kinetic', 'energy', 'forces', 'steps'):
        assert torch.equal(getattr(plain, k), getattr(empty, k)), k
    assert not torch.equal(plain.pos, res.pos)


@pytest.mark.gpu
def test_run_refuses_bad_constraints_on_the_device(dev):
    """A constraint whose two atoms are fixed, pairs across graphs, lengths that are not positive, a Constraints of another
    batch or on another device, something that is no Constraints, a bad bound or sweep count: ValueError, before anything moves."""
    from pamnet_amd.md import run
    h = _wells('nve', NVE)
    model, data, cons = _well(dev, h)
    n = len(h.pos0)
    fixed = torch.zeros(n, dtype=torch.bool, device=dev)
    fixed[[0, 1]] = True                                           # both ends of the chain's first bond
    with pytest.raises(ValueError, match='both `fixed`'):
        run(model, data, 3, P_DT, fixed=fixed, constraints=cons)
    fixed[1] = False
    res = run(model, data, 3, P_DT, fixed=fixed, constraints=cons)  # one fixed end is fine
    assert res.steps.tolist() == [3] * 4 and torch.equal(res.pos[0], data.pos[0])
    with pytest.raises(ValueError, match='joins two graphs'):
        Constraints(data, torch.tensor([[0, n - 1]], device=dev))
    for bad in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='positive and finite'):
            Constraints(data, torch.tensor([[0, 1]], device=dev), torch.tensor([bad], dtype=torch.float64, device=dev))
    other = Constraints(data.batch[:-1], torch.tensor([[0, 1]], device=dev), torch.ones(1, dtype=torch.float64, device=dev))
    on_cpu = Constraints(data.batch.cpu(), torch.tensor([[0, 1]]), torch.ones(1, dtype=torch.float64))
    for kw, match in ((dict(constraints=other), 'of this batch'), (dict(constraints=on_cpu), 'of this batch'),
                      (dict(constraints=[[0, 1]]), 'of this batch'), (dict(constraints=cons, constraint_tol=0.0), 'constraint_tol'),
                      (dict(constraints=cons, constraint_tol=float('inf')), 'constraint_tol'),
                      (dict(constraints=cons, constraint_sweeps=0), 'constraint_sweeps')):
        with pytest.raises(ValueError, match=match):
            run(model, data, 3, P_DT, **kw)


@pytest.mark.gpu
def test_a_workspace_of_the_callers_own_gives_the_same_bits(dev):
    """constrained_step and project_constraints with `work=` (an fp64 tensor [9 n] filled with NaN: every row a solve reads it has
    written before) give bit for bit what the workspace kept by the Constraints gives -- the single-colour tether and the
    projection of positions and velocities in one launch included; a workspace that is too small or of another dtype is refused."""
    c = _kernel_case()
    cons = _device_cons(dev, c)
    n = len(c.pos)
    own = torch.full((9 * n,), float('nan'), dtype=torch.float64, device=dev)
    kept = _step_on_device(dev, c, 1, 1, cons=cons)
    pos, vel, dE = _t(dev, c.pos), _t(dev, c.vel), _t(dev, c.dE)
    state = {k: _t(dev, c.state[k]) for k in STATE}
    M.constrained_step(pos, vel, dE, _t(dev, c.gptr), state, cons, _t(dev, c.dt), _t(dev, c.kT), _t(dev, c.gamma), _t(dev, c.mass),
                       _t(dev, c.fixed.astype(np.uint8)), 1, 1, tol=TOL, max_sweeps=MAX_SWEEPS, work=own)
    assert np.array_equal(pos.cpu().numpy(), kept[0], equal_nan=True) and np.array_equal(vel.cpu().numpy(), kept[1], equal_nan=True)
    assert all(np.array_equal(state[k].cpu().numpy(), kept[2][k], equal_nan=True) for k in STATE)
    p = _project_case()
    kept = _project_on_device(dev, p, cons, 1, 1)
    own.fill_(float('nan'))
    pos, vel = _t(dev, p.pos), _t(dev, p.vel)
    st = {k: _t(dev, p.state[k]) for k in ('status', 'ke', 'sweeps')}
    args = (_t(dev, p.gptr), st, cons, _t(dev, p.dt), _t(dev, p.mass), _t(dev, p.fixed.astype(np.uint8)), 1, 1, TOL, MAX_SWEEPS)
    M.project_constraints(pos, vel, *args, work=own)
    assert np.array_equal(pos.cpu().numpy(), kept[0]) and np.array_equal(vel.cpu().numpy(), kept[1], equal_nan=True)
    assert all(np.array_equal(st[k].cpu().numpy(), kept[2][k]) for k in st)
    for bad in (own[:-1], own.float(), own.cpu()):
        with pytest.raises(ValueError, match='`work` is a float64'):
            M.project_constraints(pos, vel, *args, work=bad)
