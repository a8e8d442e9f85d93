"""Cell relaxation: the variable-cell FIRE step kernel pamnet_fire_cell_step_f32 (csrc/relax_cell.hip) and the driver
pamnet_amd/relax.py relax_cell.

The reference is tests/relax_cell_ref.py fire_cell_step_ref, the rule of include/pamnet_hip.h restated in numpy fp64.  Inputs are made
once on the CPU with fixed seeds and never modified; the conditions under which kernel and reference take the same branch (both
compute in fp64 from the same fp32 inputs) are asserted by tests that need no GPU.

Tolerances are those of tests/test_relax.py: KTOL = 1e-6 max-normalised per graph for what is stored in fp32 (fmax, smax, the
velocities, the displacement pos_new - pos_old and cell_new - cell_old); 1e-12 relative for the fp64 state (dt, a, F_new - F_old,
vcell); equality for the integer state and for everything that must not move."""
import copy

import numpy as np
import pytest
import torch

from conftest import maxnorm_err
from relax_cell_ref import CELL_STATE, fire_cell_step_ref, generalised_gradient, stress_terms
from relax_ref import STATE
from test_relax import DEFAULTS, KTOL, MODELS, ROLES as FIXED_ROLES, SIZES, _margins

ENTRY, FIXED_ENTRY = 'pamnet_fire_cell_step_f32', 'pamnet_fire_step_f32'
FMAX_TOL, SMAX_TOL = 0.05, 0.002
ROLES = list(FIXED_ROLES) + ['f_conv', 's_conv', 'both_conv', 'cell_cap', 'pressure', 'fixed_cell', 'w_nonfinite', 'singular',
                             'inverting']
SHIFTS = (0, 7, 13)                               # graph i plays ROLES[(i + shift) % 19]: together every role; the empty graph is last
EPS32 = 2.0 ** -24                                # half the relative spacing of fp32


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs an MI355X'
    from pamnet_amd import lib
    lib.load()
    return torch.device('cuda:0')


class Case(object):
    pass


_MADE = {}
# (coefficient of v along g, n_pos, dt, a) of the roles that move, as in tests/test_relax.py
_MOVING = {'first': (0.0, 0, 0.1, 0.1), 'up_few': (0.3, 2, 0.2, 0.1), 'up_many': (0.8, 5, 0.5, 0.08), 'up_clamp': (0.8, 7, 0.95, 0.07),
           'down': (-0.4, 3, 0.4, 0.09), 'nonfinite': (0.3, 2, 0.2, 0.1), 'all_fixed': (0.3, 2, 0.2, 0.1), 'f_conv': (0.3, 2, 0.2, 0.1),
           's_conv': (-0.4, 3, 0.4, 0.09), 'cell_cap': (0.8, 5, 0.5, 0.08), 'pressure': (0.3, 2, 0.2, 0.1),
           'fixed_cell': (0.8, 5, 0.5, 0.08), 'w_nonfinite': (0.3, 2, 0.2, 0.1), 'singular': (0.3, 2, 0.2, 0.1),
           'inverting': (0.8, 2, 0.5, 0.1), 'empty': (0.3, 2, 0.2, 0.1)}
# the largest stress component sm the virial is scaled to (threshold 0.002), and the largest force (threshold 0.05)
_SM = {'converging': 0.001, 's_conv': 0.001, 'both_conv': 0.0005, 'cell_cap': 0.03}
_FM = {'converging': 0.03, 'f_conv': 0.03, 'both_conv': 0.01}


def _kernel_case(shift, hydrostatic, uniform_p=None):
    """One batch of SIZES.  Every graph that moves has a triclinic cell0 (about 8 A, volume about 500), F = I + 0.04 noise, a cell
    factor in [3, 9], forces scaled to max |f| = 1 over its free atoms, a virial with an antisymmetric part scaled to
    sm = max |S| / V = 0.004 = 2 smax_tol, and velocities coef g + noise for atoms and cell alike (g the generalised force), so
    that the sign of P is that of coef.  The ten roles of tests/test_relax.py keep their states; all_fixed and the empty graph
    move their cell alone.  Beyond them:
      f_conv     max |f| = 0.03 < 0.05, sm = 0.004: moves;      s_conv   max |f| = 1, sm = 0.001 < 0.002: moves
      both_conv  0.01 and 0.0005 -> converged (as `converging`: 0.03 and 0.001)
      cell_cap   sm = 0.03: a row of dt v_c is the longest;     pressure p = 0.007 (p V about 3, as large as the virial)
      fixed_cell cell_dof = 0: the fixed-cell rule, cell / F / vcell / smax untouched
      w_nonfinite  a diagonal entry of W NaN (inf at shift 7) -> failed
      singular   cell0 has a zero row (all zero at shift 13) -> V == 0 -> failed
      inverting  L = 0.05 and a compressive stress: det F_new < 0 -> failed.
    A moving graph of 63 atoms or more has a fifth of its atoms fixed.  uniform_p: that pressure for every graph instead."""
    key = (shift, bool(hydrostatic), uniform_p)
    if key in _MADE:
        return _MADE[key]
    rng = np.random.RandomState(300 + shift)
    n, G = sum(SIZES), len(SIZES)
    c = Case()
    c.hydrostatic = bool(hydrostatic)
    c.gptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    c.roles = [ROLES[(i + shift) % len(ROLES)] for i in range(G - 1)] + ['empty']
    c.pos = rng.uniform(-4.0, 4.0, (n, 3)).astype(np.float32)
    c.vel, c.dE = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    c.fixed = np.zeros(n, dtype=bool)
    c.W, c.cell0 = np.zeros((G, 3, 3), np.float32), np.zeros((G, 3, 3), np.float32)
    c.F, c.vcell = np.tile(np.eye(3), (G, 1, 1)), np.zeros((G, 3, 3))
    c.L, c.p = np.zeros(G), np.zeros(G)
    c.dof = np.ones(G, dtype=bool)
    c.state = dict(dt=np.full(G, 0.1), a=np.full(G, 0.1), n_pos=np.zeros(G, np.int32), steps=np.zeros(G, np.int32),
                   status=np.zeros(G, np.int32), fmax=np.full(G, -1.0, np.float32), smax=np.full(G, -1.0, np.float32))
    for g, role in enumerate(c.roles):
        lo, hi = int(c.gptr[g]), int(c.gptr[g + 1])
        m = hi - lo
        cell0 = (8.0 * np.eye(3) + rng.uniform(-1.5, 1.5, (3, 3))).astype(np.float32)
        F = np.eye(3) + 0.04 * rng.standard_normal((3, 3))
        L = 0.05 if role == 'inverting' else rng.uniform(3.0, 9.0)
        p = 0.007 if role == 'pressure' else 0.0
        if uniform_p is not None:
            p = uniform_p
        if role == 'singular':
            cell0[2 if shift != 13 else slice(None)] = 0.0
        r = rng.standard_normal((3, 3)) * (0.1 if role == 'inverting' else 1.0)   # (inverting: S positive definite)
        W = 0.5 * (r + r.T) + 1.5 * np.eye(3) * (1.0 if role == 'inverting' else rng.choice([-1.0, 1.0]))
        W += 0.3 * np.triu(rng.standard_normal((3, 3)), 1)                        # (not symmetric: the kernel symmetrises)
        ref_cell = cell0 if role != 'singular' else (8.0 * np.eye(3)).astype(np.float32)
        _, _, sm0, _ = stress_terms(W.astype(np.float32), ref_cell, F, L, 0.0, hydrostatic)
        W = (W * (_SM.get(role, 0.004) / sm0)).astype(np.float32)
        f = rng.standard_normal((m, 3))
        noise = 0.1 * rng.standard_normal((m, 3))
        fix = np.zeros(m, dtype=bool)
        if role == 'all_fixed':
            fix[:] = True
        elif role in _MOVING and m >= 63:
            fix[rng.choice(m, m // 5, replace=False)] = True
        free = ~fix
        if free.any():
            f /= np.sqrt((f[free] ** 2).sum(1).max())
        f *= _FM.get(role, 1.0)
        c.fixed[lo:hi] = fix
        c.state['steps'][g] = rng.randint(0, 40)
        _, _, _, g_c = stress_terms(W, cell0, F, L, p, hydrostatic)
        if role in _MOVING:
            coef, n_pos, dt, a = _MOVING[role]
            v = coef * (f @ F.T) + (noise if coef else 0.0)
            v[fix] = rng.standard_normal((int(fix.sum()), 3))
            g_fin = np.where(np.isfinite(g_c), g_c, 0.0)
            vc = coef * g_fin + (0.05 * np.abs(g_fin).max() * rng.standard_normal((3, 3)) if coef else 0.0)
            c.state['n_pos'][g], c.state['dt'][g], c.state['a'][g] = n_pos, dt, a
        else:
            v, vc = rng.standard_normal((m, 3)), rng.standard_normal((3, 3))
            c.state['n_pos'][g], c.state['dt'][g], c.state['a'][g] = rng.randint(0, 9), rng.uniform(0.05, 1.0), rng.uniform(0.01, 0.1)
        if role in ('converged', 'failed'):
            c.state['status'][g] = 1 if role == 'converged' else 2
            c.state['fmax'][g] = 0.04 if role == 'converged' else np.inf
            c.state['smax'][g] = 0.001 if role == 'converged' else np.inf
        if role == 'fixed_cell':
            c.dof[g] = False
        c.dE[lo:hi], c.vel[lo:hi] = (-f).astype(np.float32), v.astype(np.float32)
        if role == 'nonfinite' and m:
            a_free = lo + int(np.nonzero(free)[0][m // 2 if m > 2 else 0])
            c.dE[a_free, 1] = np.inf if shift == 7 else np.nan
        if role == 'w_nonfinite':
            W[1, 1] = np.inf if shift == 7 else np.nan
        c.W[g], c.cell0[g], c.F[g], c.vcell[g], c.L[g], c.p[g] = W, cell0, F, vc, L, p
    c.cell = np.einsum('gij,gjk->gik', c.cell0.astype(np.float64), c.F).astype(np.float32)
    diag = {}
    c.ref = fire_cell_step_ref(c.pos, c.vel, c.dE, c.W, c.gptr, c.cell0, c.cell, c.F, c.vcell, c.state, FMAX_TOL, SMAX_TOL, c.fixed,
                               c.dof, c.L, c.p, hydrostatic, diag=diag, **DEFAULTS)
    c.diag = diag
    _MADE[key] = c
    return c


def _cell_margins(d, tol, stol, rows=True):
    """_margins of tests/test_relax.py, and for a graph that relaxes its cell: sm 1 % away from its threshold, det F_new away from
    0 and, for the kernel cases (rows), the longest cell row 1 % away from the longest atom row.  Which row is the longest is not
    a branch -- the cap reads their maximum, which _margins keeps 1 % away from max_step -- so on a trajectory, where atoms and
    cell take turns, it is not asserted."""
    if d is None:
        return
    _margins(d, tol)
    if not d.get('cell') or not np.isfinite(d['F2']) or not np.isfinite(d['V']) or d['V'] == 0.0:
        return
    assert abs(d['sm'] - stol) >= 0.01 * stol, d
    if 'max_dr' in d:
        assert not rows or abs(d['max_dr_cell'] - d['max_dr_atoms']) >= 0.01 * d['max_dr'], d
        assert abs(d['det_new']) > 0.1, d


def _before(c):
    return c.pos, c.vel, c.cell, c.F, c.vcell, c.state


# ---------------------------------------------------------------------------------------------------------- elastic wells
class ElasticWell(torch.nn.Module):
    """E_g = 1/2 k_g |C_g - C*_g|^2 + 1/2 kappa_g sum_{a in g} |pos_a - s_a C_g|^2 with fixed fractional targets s_a: a plain torch
    module that applies (I + strain) to the positions and the cell itself, differentiable in data.pos and data.strain."""

    def __init__(self, k, kappa, cstar, s):
        super().__init__()
        for name, v in (('k', k), ('kappa', kappa), ('cstar', cstar), ('s', s)):
            self.register_buffer(name, v)

    def forward(self, data):
        eps = torch.eye(3, dtype=data.pos.dtype, device=data.pos.device) + data.strain
        C = torch.bmm(data.cell, eps)
        pos = torch.bmm(data.pos[:, None, :], eps[data.batch]).squeeze(1)
        d = pos - torch.bmm(self.s[:, None, :], C[data.batch]).squeeze(1)
        atoms = torch.zeros_like(self.k).index_add_(0, data.batch, (d * d).sum(1))
        return 0.5 * self.k * (C - self.cstar).pow(2).sum((1, 2)) + 0.5 * self.kappa * atoms


W_SIZES, W_K, W_KAPPA, W_FTOL, W_STOL, W_MAX, W_P = (4, 9, 70), (0.5, 2.0, 6.0), (1.0, 0.5, 2.0), 0.01, 1.25e-4, 600, 0.02
W_SEED, W_AMP = 17, 0.2375                        # (W_AMP: the initial displacement of the free atoms; with W_STOL chosen so that
#                                                   all three trajectories keep the branch margins, as H_SEED of tests/test_relax.py)
W_C0 = 4.0                                        # the reference cells are cubes of this edge: coordinates stay within [-1, 6]


def _well_gradients(w, pos, cell):
    """fp64 (d [n, 3], dE/dpos, W [G, 3, 3]) of ElasticWell at fp32 pos and cell: W = k C^T (C - C*) + kappa sum d_a^T d_a."""
    C = cell.astype(np.float64)
    d = pos.astype(np.float64) - np.einsum('ai,aij->aj', w.s, C[w.batch])
    W = np.stack([w.k[g] * C[g].T @ (C[g] - w.cstar[g]) + w.kappa[g] * d[w.batch == g].T @ d[w.batch == g]
                  for g in range(len(W_SIZES))])
    return d, w.kappa[w.batch, None] * d, W


def _wells(kind):
    """Three wells of 4, 9 and 70 atoms and their reference trajectory: fire_cell_step_ref iterated on the fp64 gradients rounded
    to fp32 until no graph is running.

    S is the SYMMETRISED virial, so a rotation between C and C* is not a degree of freedom the rule relaxes (a model's energy does
    not depend on it; this test energy does).  The wells are therefore chosen so that W stays symmetric on the whole trajectory
    (asserted): cell0 = 4 I, C* symmetric, and generalised displacements whose second moment sum e^T e is a multiple of I --
    every matrix of the trajectory is then a polynomial in C*.
      'aniso'  C* symmetric positive definite with off-diagonal entries up to 0.4; free atoms displaced by W_AMP along the axes in
               turn (a multiple of three of them), fixed atoms (from the third graph: every fifth) at their fractional targets,
               which they keep by following the cell;  'aniso_p': the same under the pressure W_P;
      'hydro'  hydrostatic=True with cubic C* = (4.3, 3.8, 4.1) I; the same atoms."""
    if ('wells', kind) in _MADE:
        return _MADE[('wells', kind)]
    rng = np.random.RandomState(W_SEED)
    n, G = sum(W_SIZES), len(W_SIZES)
    w = Case()
    w.hydrostatic, w.p = kind == 'hydro', (W_P if kind == 'aniso_p' else 0.0)
    w.batch = np.repeat(np.arange(G), W_SIZES)
    w.gptr = np.concatenate([[0], np.cumsum(W_SIZES)]).astype(np.int32)
    w.k, w.kappa = np.asarray(W_K), np.asarray(W_KAPPA)
    w.s = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32).astype(np.float64)
    w.cell0 = np.tile(W_C0 * np.eye(3), (G, 1, 1)).astype(np.float32)
    if w.hydrostatic:
        w.cstar = np.stack([c * np.eye(3) for c in (4.3, 3.8, 4.1)])
    else:
        sym = [rng.uniform(-0.4, 0.4, (3, 3)) for _ in range(G)]
        w.cstar = np.stack([4.3 * np.eye(3) + 0.5 * (a + a.T) for a in sym]).astype(np.float32).astype(np.float64)
    w.fixed = np.zeros(n, dtype=bool)
    w.fixed[w.gptr[2]:w.gptr[3]:5] = True
    e = np.zeros((n, 3))
    for g in range(G):
        free = np.nonzero(~w.fixed[w.gptr[g]:w.gptr[g + 1]])[0] + w.gptr[g]
        free = free[:len(free) // 3 * 3]                                       # the others start at their targets
        e[free, np.arange(len(free)) % 3] = W_AMP * np.where(np.arange(len(free)) % 2, -1.0, 1.0)
    w.pos0 = (w.s @ (W_C0 * np.eye(3)) + e).astype(np.float32)
    w.L = np.asarray(W_SIZES, dtype=np.float64)
    pos, vel, cell = w.pos0.copy(), np.zeros((n, 3), np.float32), w.cell0.copy()
    F, vc = np.tile(np.eye(3), (G, 1, 1)), np.zeros((G, 3, 3))
    st = dict(dt=np.full(G, 0.1), a=np.full(G, 0.1), n_pos=np.zeros(G, np.int32), steps=np.zeros(G, np.int32),
              status=np.zeros(G, np.int32), fmax=np.zeros(G, np.float32), smax=np.zeros(G, np.float32))
    w.diags, w.asym = [], 0.0
    for _ in range(W_MAX):
        _, dE, W = _well_gradients(w, pos, cell)
        scale = w.k * np.abs(cell.astype(np.float64)).max((1, 2)) ** 2          # (of the terms of W1, which cancel at the minimum)
        w.asym = max(w.asym, float((np.abs(W - W.transpose(0, 2, 1)).max((1, 2)) / scale).max()))
        diag = {}
        pos, vel, cell, F, vc, st = fire_cell_step_ref(pos, vel, dE.astype(np.float32), W.astype(np.float32), w.gptr, w.cell0, cell,
                                                       F, vc, st, W_FTOL, W_STOL, w.fixed, None, w.L, w.p, w.hydrostatic, diag=diag,
                                                       **DEFAULTS)
        w.diags.append(diag)
        if not (st['status'] == 0).any():
            break
    w.pos, w.cell, w.F, w.state = pos, cell, F, st
    _MADE[('wells', kind)] = w
    return w


def _well_bounds(w, pos, cell, slack=0.0):
    """How far a CONVERGED result may be from the known minimum (p = 0), per graph: (bound on |C - C*|_F, bound on |pos_a - s_a C*|).

    Converged means max |f| < ftol and max |S_ij| < stol V for the f and S the step saw; `slack` is the relative error of what
    it saw against the fp64 values at the fp32 coordinates (2^-24: the reference rounds them to fp32).  With W = W1 + W2,
    W1 = k C^T (C - C*), W2 = kappa sum d^T d, d_a = pos_a - s_a C = f_a / kappa, and A the antisymmetric part of W (what the
    symmetrised rule does not see; evaluated here):  C - C* = C^-T (S + A - W2) / k, hence
        |C - C*|_F <= (3 stol V + |A|_F + |W2|_F) / (k sigma_min(C))    (|W2|_F, about n_free ftol^2 / kappa, is evaluated too),
    (hydrostatic, cubic: 3 k c (c - c*) = tr S - kappa sum |d|^2, the same bound with |A| = 0), and for a free atom
        |pos_a - s_a C*| <= ftol / kappa + |s_a| |C - C*|_F.
    A fixed atom started on its target and is moved by pos <- fp32(pos D) only: it stays there but for one rounding of its
    coordinates per step, half a spacing 2^-24 |x| <= 2^-21 (|x| < 8) each, times the steps of the graph."""
    ftol, stol = W_FTOL * (1.0 + slack), W_STOL * (1.0 + slack)
    d, _, W = _well_gradients(w, pos, cell)
    in_g = lambda g: w.batch == g
    out = []
    for g in range(len(W_SIZES)):
        C = cell[g].astype(np.float64)
        V = abs(np.linalg.det(C))
        A = 0.0 if w.hydrostatic else float(np.linalg.norm(0.5 * (W[g] - W[g].T)))
        W2 = float(np.linalg.norm(w.kappa[g] * d[in_g(g)].T @ d[in_g(g)]))        # (<= n_free ftol^2 / kappa, and evaluated)
        bc = (3.0 * stol * V + A + W2) / (w.k[g] * np.linalg.svd(C, compute_uv=False).min())
        out.append((bc, ftol / w.kappa[g] + np.sqrt(3.0) * bc))
    return out


def _assert_at_the_minimum(w, pos, cell, steps, slack, tag):
    for g, (bc, bp) in enumerate(_well_bounds(w, pos, cell, slack)):
        s = slice(int(w.gptr[g]), int(w.gptr[g + 1]))
        ec = float(np.linalg.norm(cell[g].astype(np.float64) - w.cstar[g]))
        target = w.s[s] @ w.cstar[g]
        ep = np.sqrt(((pos[s].astype(np.float64) - target) ** 2).sum(1))
        fx = w.fixed[s]
        spacing = int(steps[g]) * 2.0 ** -21 * np.sqrt(3.0)
        print(tag, 'graph', g, '|C - C*|', ec, 'bound', bc, 'max |pos - s C*|', float(ep.max()), 'bound', bp, 'fixed rows',
              float(ep[fx].max()) if fx.any() else None, 'spacing', spacing)
        assert ec <= bc, (tag, g, ec, bc)
        assert (ep[~fx] <= bp).all(), (tag, g, float(ep[~fx].max()), bp)
        if fx.any():                              # a fixed atom sits on s_a C: off s_a C* by the cell's error and the roundings
            assert (ep[fx] <= np.sqrt(3.0) * bc + spacing).all(), (tag, g, float(ep[fx].max()))


# ---------------------------------------------------------------------------------------------------------- CPU tests
def test_header_declares_the_cell_step_at_abi_18():
    """(No GPU: the header and the built library.)"""
    import ctypes
    import re
    from pamnet_amd import build, lib
    decl = lib.declared_functions()
    assert ENTRY in decl
    P, D, I = ctypes.c_void_p, ctypes.c_double, ctypes.c_int32
    assert decl[ENTRY] == [P] * 6 + [ctypes.c_int64] * 2 + [P] * 16 + [D] * 3 + [I] + [D] * 2 + [I] + [D] * 4 + [P]
    assert int(re.search(r'#define\s+PAMNET_ABI_VERSION\s+(\d+)', open(lib.HEADER).read()).group(1)) == 18
    h = ctypes.CDLL(build.build())
    assert h.pamnet_abi_version() == 18 and hasattr(h, ENTRY) and hasattr(h, FIXED_ENTRY)


def test_cell_step_kernel_is_scratch_free(tmp_path):
    """(No GPU: hipcc cross-compiles.)  The compiler's report for csrc/relax_cell.hip: one kernel, no scratch, the five fp64
    partials of four wavefronts in LDS (DESIGN section 10a quotes the figures)."""
    import os
    import re
    import shutil
    import subprocess
    from pamnet_amd import build
    hipcc = '/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else shutil.which('hipcc')
    assert hipcc, 'hipcc not available'
    r = subprocess.run([hipcc] + build.FLAGS + ['-c', os.path.join(build.CSRC, 'relax_cell.hip'), '-o', str(tmp_path / 'relax_cell.o'),
                                                '-Rpass-analysis=kernel-resource-usage'], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = [b for b in re.split(r'remark: Function Name: ', r.stderr)[1:] if 'fire_cell_kernel' in b.split()[0]]
    assert len(blocks) == 1 and 'fire_step_kernel' not in r.stderr
    num = lambda key: int(re.search(key + r': (\d+)', blocks[0]).group(1))
    print('VGPRs', num('VGPRs'), 'AGPRs', num('AGPRs'), 'LDS', num(r'LDS Size \[bytes/block\]'))
    assert num(r'ScratchSize \[bytes/lane\]') == 0 and num('VGPRs Spill') == 0 and num('SGPRs Spill') == 0
    assert num(r'LDS Size \[bytes/block\]') <= 256


def test_the_reference_gradient_is_the_derivative_in_the_generalised_coordinates():
    """(No GPU; a test of the reference's convention.)  For a smooth fp64 energy of the Gram matrix of M = [pos; cell] (invariant
    under rotation, so that its virial is symmetric), the reference's (g_a, g_c L) at a non-identity F and p > 0 is minus the
    central difference of E(x~ F, cell0 F) + p |det(cell0 F)| with respect to x~ and F: this pins F^T, F^-T, 1 / L and p V.
    h = 1e-4 on coordinates of size 1 .. 6: truncation h^2 / 6 |E'''| and rounding 2^-52 |E| / h are both below 1e-7 of the largest
    gradient entry for this quartic (E about 1e3, third derivatives about E / len^3); the bound is 1e-6."""
    rng = np.random.RandomState(2)
    m, L, p, h = 5, 3.5, 0.7, 1e-4
    cell0 = (5.0 * np.eye(3) + rng.uniform(-1.0, 1.0, (3, 3))).astype(np.float32).astype(np.float64)
    F = np.eye(3) + 0.1 * rng.standard_normal((3, 3))
    xt = rng.uniform(0.0, 5.0, (m, 3))
    a, b = rng.standard_normal((m + 3, m + 3)), rng.standard_normal((m + 3, m + 3))
    a, b = 0.5 * (a + a.T), 0.005 * (b + b.T)

    def energy(x, Fm):
        M = np.concatenate([x @ Fm, cell0 @ Fm])
        gm = M @ M.T
        return float((a * gm).sum() + 0.5 * (b * gm * gm).sum()) + p * abs(np.linalg.det(cell0 @ Fm))

    M = np.concatenate([xt @ F, cell0 @ F])
    dM = 2.0 * (a + b * (M @ M.T)) @ M
    W = M.T @ dM                                                   # dE/d eps of pos -> pos (I + eps), cell -> cell (I + eps)
    assert np.abs(W - W.T).max() < 1e-9 * np.abs(W).max()
    g_a, g_cL = generalised_gradient(dM[:m], W, cell0, F, L, p)

    def central(x, Fm, which, idx):
        lo, hi = [np.array(v) for v in (x, Fm)], [np.array(v) for v in (x, Fm)]
        hi[which][idx] += h
        lo[which][idx] -= h
        return (energy(*hi) - energy(*lo)) / (2 * h)

    fd_a = np.array([[central(xt, F, 0, (i, j)) for j in range(3)] for i in range(m)])
    fd_c = np.array([[central(xt, F, 1, (i, j)) for j in range(3)] for i in range(3)])
    scale = max(np.abs(fd_a).max(), np.abs(fd_c).max())
    print('generalised gradient vs central differences: atoms', np.abs(g_a + fd_a).max() / scale, 'cell',
          np.abs(g_cL + fd_c).max() / scale)
    assert np.abs(g_a + fd_a).max() <= 1e-6 * scale and np.abs(g_cL + fd_c).max() <= 1e-6 * scale
    assert np.abs(fd_c).min() > 1e-3 * scale and abs(p * np.linalg.det(cell0 @ F)) > 0.01 * scale


def test_cell_inputs_meet_their_preconditions():
    """(No GPU.)  The kernel-test batches keep their distance from every branch point (_cell_margins) and every role does what its
    name says, with hydrostatic on and off; together they take every branch."""
    seen = set()
    for hydro in (False, True):
        for shift in SHIFTS:
            c = _kernel_case(shift, hydro)
            st = c.ref[5]
            for g, role in enumerate(c.roles):
                d = c.diag[g]
                _cell_margins(d, FMAX_TOL, SMAX_TOL)
                nfix = int(c.fixed[c.gptr[g]:c.gptr[g + 1]].sum())
                if role in ('converged', 'failed'):
                    assert d is None and st['status'][g] == c.state['status'][g] != 0
                elif role in ('converging', 'both_conv'):
                    assert st['status'][g] == 1 and 0 < d['fm'] < FMAX_TOL and d['sm'] < SMAX_TOL
                elif role in ('nonfinite', 'w_nonfinite'):
                    assert st['status'][g] == 2 and not np.isfinite(st['fmax'][g]) and np.isnan(st['fmax'][g]) == (shift != 7)
                    assert role == 'nonfinite' or np.isnan(st['smax'][g]) == (shift != 7)
                elif role == 'singular':
                    assert st['status'][g] == 2 and d['V'] == 0.0 and np.isfinite(st['fmax'][g]) and np.isinf(st['smax'][g])
                elif role == 'inverting':
                    assert st['status'][g] == 2 and d['det_new'] < -0.1 and st['steps'][g] == c.state['steps'][g]
                else:
                    assert st['status'][g] == 0 and st['steps'][g] == c.state['steps'][g] + 1, (role, d)
                    if role == 'fixed_cell':
                        assert not d.get('cell') and np.array_equal(c.ref[3][g], c.F[g])
                    else:
                        assert d['cell'] and not np.array_equal(c.ref[3][g], c.F[g])
                        by_cell = d['max_dr_cell'] > d['max_dr_atoms']
                        assert role not in ('cell_cap', 'all_fixed', 'empty') or by_cell
                        assert role != 'cell_cap' or d['max_dr'] > DEFAULTS['max_step']
                        assert role != 'f_conv' or (d['fm'] < FMAX_TOL and d['sm'] > SMAX_TOL)
                        assert role != 's_conv' or (d['fm'] > FMAX_TOL and d['sm'] < SMAX_TOL)
                        assert role != 'pressure' or c.p[g] * d['V'] > 1.0
                        seen.update(['cap_by_cell' if by_cell else 'cap_by_atoms',
                                     'capped' if d['max_dr'] > DEFAULTS['max_step'] else 'free', 'some_fixed' if nfix else 'none_fixed',
                                     'first' if d['V2'] == 0.0 else 'up' if d['P'] > 0 else 'down'])
                seen.add(role)
    assert seen == set(ROLES) | {'empty', 'cap_by_cell', 'cap_by_atoms', 'capped', 'free', 'some_fixed', 'none_fixed', 'first', 'up',
                                 'down'}, seen


@pytest.mark.parametrize('kind', ['aniso', 'hydro'])
def test_the_reference_relaxes_every_elastic_well_to_its_minimum(kind):
    """(No GPU; a test of the reference.)  fire_cell_step_ref iterated on three elastic wells brings every graph below both
    thresholds, each after its own number of steps, with C at C* and every atom at s_a C* within _well_bounds; the virial stays
    symmetric on the way (what the wells were chosen for); every step keeps the branch margins."""
    w = _wells(kind)
    assert (w.state['status'] == 1).all(), w.state
    assert (w.state['fmax'] < W_FTOL).all() and (w.state['smax'] < W_STOL).all()
    assert len(set(w.state['steps'].tolist())) == len(W_SIZES), w.state['steps']
    assert w.asym < 1e-5, w.asym                                  # (relative to k |C|^2; fp32 roundings of pos and cell: 1e-7)
    assert w.fixed.any() and not np.array_equal(w.pos[w.fixed], w.pos0[w.fixed])       # fixed atoms follow the cell
    print(kind, 'wells: steps', w.state['steps'], 'iterations', len(w.diags), 'asymmetry of W', w.asym)
    _assert_at_the_minimum(w, w.pos, w.cell, w.state['steps'], EPS32, kind)
    branches = set()
    for diag in w.diags:
        for g, d in diag.items():
            _cell_margins(d, W_FTOL, W_STOL, rows=False)
            if d is not None and 'P' in d:
                branches.add('first' if d['V2'] == 0.0 else 'up' if d['P'] > 0 else 'down')
    assert branches == {'first', 'up', 'down'}, branches


def test_under_pressure_the_reference_stops_where_forces_and_stress_are_below_the_thresholds():
    """(No GPU.)  With p = 0.02 the quantity minimised is E + p V.  At the converged result, evaluated again in fp64 from the fp32
    coordinates: max |f| < ftol and max |S_ij| / V < stol, each up to the rounding of what the step saw -- f and W were rounded to
    fp32, half a spacing 2^-24 relative each; S = sym W + p V I cancels, so the stress carries 2^-24 max |W| / V -- and the cells
    are smaller than without pressure."""
    w, w0 = _wells('aniso_p'), _wells('aniso')
    assert (w.state['status'] == 1).all() and len(set(w.state['steps'].tolist())) == len(W_SIZES)
    _, dE, W = _well_gradients(w, w.pos, w.cell)
    for g in range(len(W_SIZES)):
        s = slice(int(w.gptr[g]), int(w.gptr[g + 1]))
        f = dE[s][~w.fixed[s]]
        fm = float(np.sqrt((f * f).sum(1).max()))
        V, _, sm, _ = stress_terms(W[g], w.cell0[g], w.F[g], w.L[g], w.p, False)
        print('graph', g, 'fm', fm, 'sm', sm, 'V', V, 'V at p = 0', abs(np.linalg.det(w0.cell[g].astype(np.float64))))
        assert fm < W_FTOL * (1.0 + 2 * EPS32)
        assert sm < W_STOL + 2 * EPS32 * float(np.abs(W[g]).max()) / V
        assert V < abs(np.linalg.det(w0.cell[g].astype(np.float64))) - 1.0
    for diag in w.diags:
        for d in diag.values():
            _cell_margins(d, W_FTOL, W_STOL, rows=False)


# ------------------------------------------------------------------------------------------------------- kernel tests
def _t(dev):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _step_on_device(dev, c, lo=0, hi=None, graphs=None, dof='case', scalars=False, p=None):
    """One launch on the atoms [lo, hi) / graphs `graphs` (a slice) of a case -> (pos, vel, cell, F, vcell, state) as numpy.
    scalars: thresholds and the pressure `p` as floats, else as per-graph arrays."""
    from pamnet_amd import relax as R
    graphs = slice(0, len(c.gptr) - 1) if graphs is None else graphs
    t = _t(dev)
    ng = graphs.stop - graphs.start
    pos, vel, dE, fixed = t(c.pos[lo:hi]), t(c.vel[lo:hi]), t(c.dE[lo:hi]), t(c.fixed[lo:hi].astype(np.uint8))
    gptr = t(c.gptr[graphs.start:graphs.stop + 1] - lo)
    state = {k: t(c.state[k][graphs]) for k in CELL_STATE}
    state['F'], state['vcell'] = t(c.F[graphs]), t(c.vcell[graphs])
    cell0, cell, W, L = t(c.cell0[graphs]), t(c.cell[graphs]), t(c.W[graphs]), t(c.L[graphs])
    dof8 = None if dof is None else t((c.dof[graphs] if isinstance(dof, str) else dof[graphs]).astype(np.uint8))
    prs = c.p[graphs] if p is None else np.full(ng, p)
    if scalars:
        ftol, stol, prs = FMAX_TOL, SMAX_TOL, float(p)
    else:
        ftol, stol, prs = t(np.full(ng, FMAX_TOL, np.float32)), t(np.full(ng, SMAX_TOL, np.float32)), t(prs.astype(np.float64))
    R.fire_cell_step(pos, vel, dE, W, gptr, cell0, cell, state, ftol, stol, L, fixed, dof8, prs, c.hydrostatic, **DEFAULTS)
    n = lambda v: v.cpu().numpy()
    for given, kept in ((cell0, c.cell0[graphs]), (W, c.W[graphs]), (dE, c.dE[lo:hi])):     # read only
        assert np.array_equal(n(given), kept, equal_nan=True)
    return n(pos), n(vel), n(cell), n(state['F']), n(state['vcell']), {k: n(state[k]) for k in CELL_STATE}


def _same_class(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b))


def _assert_cell_step_matches(got, want, before, gptr, fixed, dof, tag=''):
    """got / want / before: (pos, vel, cell, F, vcell, state); the checks of one step against fire_cell_step_ref."""
    (gp, gv, gc, gF, gvc, gs), (wp, wv, wc, wF, wvc, ws), (bp, bv, bc, bF, bvc, bs) = got, want, before
    for k in ('status', 'n_pos', 'steps'):
        assert np.array_equal(gs[k], ws[k]), (tag, k, gs[k], ws[k])
    for k in ('dt', 'a'):
        assert np.all(np.abs(gs[k] - ws[k]) <= 1e-12 * np.abs(ws[k])), (tag, k, gs[k], ws[k])
    for k in ('fmax', 'smax'):
        finite = np.isfinite(ws[k])
        assert _same_class(gs[k], ws[k]), (tag, k, gs[k], ws[k])
        assert np.all(np.abs(gs[k][finite].astype(np.float64) - ws[k][finite]) <= KTOL * np.abs(ws[k][finite])), (tag, k)
    same = lambda a, b: np.array_equal(a, b, equal_nan=True)
    worst = [0.0] * 5
    for g in range(len(gptr) - 1):
        s = slice(int(gptr[g]), int(gptr[g + 1]))
        moved = bs['status'][g] == 0 and ws['status'][g] == 0
        if not dof[g]:                            # a graph that keeps its cell: what belongs to the cell is untouched
            assert same(gc[g], bc[g]) and same(gF[g], bF[g]) and same(gvc[g], bvc[g]) and same(gs['smax'][g], bs['smax'][g]), (tag, g)
        if not moved:                             # finished before, or converged / failed in this step: nothing of g changed
            assert same(gp[s], bp[s]) and same(gv[s], bv[s]), (tag, g)
            assert same(gc[g], bc[g]) and same(gF[g], bF[g]) and same(gvc[g], bvc[g]), (tag, g)
            for k in ('dt', 'a', 'n_pos', 'steps'):
                assert gs[k][g] == bs[k][g], (tag, g, k)
            if bs['status'][g] != 0:
                assert same(gs['fmax'][g], bs['fmax'][g]) and same(gs['smax'][g], bs['smax'][g]), (tag, g)
            continue
        if dof[g]:
            e = [maxnorm_err(gc[g].astype(np.float64) - bc[g], wc[g].astype(np.float64) - bc[g]),
                 maxnorm_err(gF[g] - bF[g], wF[g] - bF[g]), maxnorm_err(gvc[g], wvc[g])]
            assert float(np.abs(wF[g] - bF[g]).max()) > 0
            assert e[0] <= KTOL and e[1] <= 1e-12 and e[2] <= 1e-12, (tag, g, e)
            worst[2:] = [max(a, b) for a, b in zip(worst[2:], e)]
        if s.stop == s.start:
            continue
        fx = fixed[s]
        assert np.array_equal(gv[s][fx], bv[s][fx]), (tag, g, 'vel rows of fixed atoms')
        if not dof[g]:
            assert np.array_equal(gp[s][fx], bp[s][fx]), (tag, g, 'fixed rows')
        elif fx.any():                            # fixed atoms follow the cell
            assert not np.array_equal(gp[s][fx], bp[s][fx]), (tag, g)
        if (~fx).any():
            ev = maxnorm_err(gv[s][~fx], wv[s][~fx])
            worst[0] = max(worst[0], ev)
            assert ev <= KTOL, (tag, g, ev)
        ed = maxnorm_err(gp[s].astype(np.float64) - bp[s], wp[s].astype(np.float64) - bp[s])
        assert float(np.abs(wp[s].astype(np.float64) - bp[s]).max()) > 0
        worst[1] = max(worst[1], ed)
        assert ed <= KTOL, (tag, g, ed)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize('hydrostatic', [False, True])
@pytest.mark.parametrize('shift', SHIFTS)
def test_one_cell_step_on_a_batch_vs_the_reference(dev, shift, hydrostatic):
    """Graphs of 1 ... 1025 atoms and an empty one in the nineteen roles of _kernel_case, per-graph thresholds and pressures:
    integer state equal; dt, a, F_new - F_old, vcell to 1e-12; fmax, smax, vel, the displacement of every atom (fixed ones
    follow the cell) and cell_new - cell_old within KTOL per graph; everything of a graph that was finished, converges or fails,
    and the cell, F, vcell and smax of a graph with cell_dof = 0, equal to the inputs."""
    c = _kernel_case(shift, hydrostatic)
    got = _step_on_device(dev, c)
    worst = _assert_cell_step_matches(got, c.ref, _before(c), c.gptr, c.fixed, c.dof, tag=(shift, hydrostatic))
    print('shift', shift, 'hydrostatic', hydrostatic, 'worst vel / displacement / cell / F / vcell error', worst)
    ok = np.isin(np.array(c.roles), ['nonfinite', 'w_nonfinite', 'failed'], invert=True)
    assert np.isfinite(got[0]).all() and np.isfinite(got[2][ok]).all() and np.isfinite(got[3]).all()


@pytest.mark.gpu
@pytest.mark.parametrize('hydrostatic', [False, True])
def test_per_graph_arrays_and_scalars_give_the_same_bits(dev, hydrostatic):
    """The thresholds and a pressure of 0.003 handed over as per-graph arrays and as scalars (cell_dof as the case has it)."""
    c = _kernel_case(7, hydrostatic)
    a = _step_on_device(dev, c, p=0.003)
    b = _step_on_device(dev, c, p=0.003, scalars=True)
    for x, y in zip(a[:5], b[:5]):
        assert np.array_equal(x, y, equal_nan=True)
    assert all(np.array_equal(a[5][k], b[5][k], equal_nan=True) for k in CELL_STATE)
    plain = _step_on_device(dev, c)                               # (the pressure is read: the case's own gives other bits)
    assert not np.array_equal(a[3], plain[3])


@pytest.mark.gpu
def test_a_graph_that_keeps_its_cell_takes_the_fixed_cell_step_bit_for_bit(dev):
    """cell_dof = 0 for every graph, and for the one graph of the case that has it: pos, vel, dt, a, n_pos, steps, status and
    fmax torch.equal to pamnet_fire_step_f32 on the same inputs; cell, F, vcell and smax untouched."""
    from pamnet_amd import relax as R
    t = _t(dev)
    for shift in SHIFTS:
        c = _kernel_case(shift, False)
        pos, vel, dE, fixed, gptr = t(c.pos), t(c.vel), t(c.dE), t(c.fixed.astype(np.uint8)), t(c.gptr)
        state = {k: t(c.state[k]) for k in STATE}
        R.fire_step(pos, vel, dE, gptr, state, FMAX_TOL, fixed, **DEFAULTS)
        want_p, want_v, want_s = pos.cpu().numpy(), vel.cpu().numpy(), {k: v.cpu().numpy() for k, v in state.items()}
        for dof in (np.zeros(len(SIZES), dtype=bool), 'case'):
            gp, gv, gc, gF, gvc, gs = _step_on_device(dev, c, dof=dof)
            graphs = range(len(SIZES)) if not isinstance(dof, str) else np.nonzero(~c.dof)[0]
            assert len(graphs) == (len(SIZES) if not isinstance(dof, str) else c.roles.count('fixed_cell'))
            for g in graphs:
                s = slice(int(c.gptr[g]), int(c.gptr[g + 1]))
                assert np.array_equal(gp[s], want_p[s], equal_nan=True) and np.array_equal(gv[s], want_v[s], equal_nan=True), (shift, g)
                for k in STATE:
                    assert np.array_equal(gs[k][g], want_s[k][g], equal_nan=True), (shift, g, k)
                assert np.array_equal(gc[g], c.cell[g]) and np.array_equal(gF[g], c.F[g]) and np.array_equal(gvc[g], c.vcell[g])
                assert gs['smax'][g] == c.state['smax'][g]
        assert (want_s['steps'] > c.state['steps']).sum() >= 5     # (the comparison is of graphs that moved)
    assert sum(_kernel_case(shift, False).roles.count('fixed_cell') for shift in SHIFTS) >= 2


@pytest.mark.gpu
def test_a_cell_step_is_repeatable_and_independent_of_the_batch(dev):
    """Two runs on the same inputs are equal bit for bit, and every graph stepped alone -- its atoms, its cell and its state as a
    batch of one -- gives the rows and the state of the batched call."""
    for shift, hydro in ((7, False), (13, True)):
        c = _kernel_case(shift, hydro)
        one, two = _step_on_device(dev, c), _step_on_device(dev, c)
        for x, y in zip(one[:5], two[:5]):
            assert np.array_equal(x, y, equal_nan=True)
        assert all(np.array_equal(one[5][k], two[5][k], equal_nan=True) for k in CELL_STATE)
        for g in range(len(SIZES)):
            lo, hi = int(c.gptr[g]), int(c.gptr[g + 1])
            p, v, cl, F, vc, s = _step_on_device(dev, c, lo, hi, slice(g, g + 1))
            assert np.array_equal(p, one[0][lo:hi], equal_nan=True) and np.array_equal(v, one[1][lo:hi], equal_nan=True), g
            assert np.array_equal(cl[0], one[2][g], equal_nan=True), g
            assert np.array_equal(F[0], one[3][g]) and np.array_equal(vc[0], one[4][g]), g
            assert all(np.array_equal(s[k], one[5][k][g:g + 1], equal_nan=True) for k in CELL_STATE), g


@pytest.mark.gpu
def test_the_cell_entry_point_validates_its_arguments(dev):
    """A null required pointer is PAMNET_ENULL, a bad count, flag or parameter PAMNET_EINVAL; fixed, cell_dof and the per-graph
    thresholds and pressures may be null; n_graphs == 0 launches nothing."""
    from pamnet_amd import lib
    c = _kernel_case(0, False)
    t = _t(dev)
    bufs = dict(pos=t(c.pos), vel=t(c.vel), dpos=t(c.dE), dstrain=t(c.W), gptr=t(c.gptr), cell0=t(c.cell0), cell=t(c.cell), F=t(c.F),
                vcell=t(c.vcell), cell_factor=t(c.L))
    bufs.update({k: t(c.state[k]) for k in CELL_STATE})
    keep = {k: v.clone() for k, v in bufs.items()}
    G, n = len(SIZES), bufs['pos'].size(0)
    order = ('pos', 'vel', 'dpos', 'dstrain', 'fixed', 'gptr', 'n', 'G', 'cell0', 'cell', 'F', 'vcell', 'cell_dof', 'cell_factor', 'dt',
             'a', 'n_pos', 'steps', 'status', 'fmax', 'smax', 'fmax_tol_g', 'smax_tol_g', 'pressure_g', 'fmax_tol', 'smax_tol',
             'pressure', 'hydrostatic', 'dt_max', 'max_step', 'n_min', 'f_inc', 'f_dec', 'a0', 'f_a')

    def call(**kw):
        a = dict(fixed=None, cell_dof=None, n=n, G=G, fmax_tol_g=None, smax_tol_g=None, pressure_g=None, fmax_tol=1e9, smax_tol=1e9,
                 pressure=0.0, hydrostatic=0, dt_max=1.0, max_step=0.2, n_min=5, f_inc=1.1, f_dec=0.5, a0=0.1, f_a=0.99)
        a.update({k: lib.ptr(v) for k, v in bufs.items()})
        a.update(kw)
        lib.call(ENTRY, *[a[k] for k in order], lib.stream_of(bufs['pos']))

    for k in bufs:
        with pytest.raises(RuntimeError, match='PAMNET_ENULL'):
            call(**{k: None})
    for kw in (dict(n=-1), dict(G=-1), dict(n_min=-1), dict(dt_max=0.0), dict(max_step=-0.2), dict(f_inc=float('inf')),
               dict(f_dec=float('nan')), dict(a0=0.0), dict(f_a=-1.0), dict(fmax_tol=float('nan')), dict(smax_tol=float('nan')),
               dict(pressure=float('inf')), dict(pressure=float('nan')), dict(hydrostatic=2), dict(hydrostatic=-1)):
        with pytest.raises(RuntimeError, match='PAMNET_EINVAL'):
            call(**kw)
    call(G=0)
    torch.cuda.synchronize()
    assert all(np.array_equal(bufs[k].cpu().numpy(), keep[k].cpu().numpy(), equal_nan=True) for k in bufs)
    # thresholds of 1e9 converge every running graph whose inputs are finite and whose cell has a volume; per graph: only those
    # they are handed to
    ftol_g, stol_g = torch.full((G,), 1e9, device=dev), torch.full((G,), 1e9, device=dev)
    ftol_g[3], stol_g[4] = 1e-9, 1e-12
    call(fmax_tol_g=lib.ptr(ftol_g), smax_tol_g=lib.ptr(stol_g), fmax_tol=1e-9, smax_tol=1e-12)
    status, roles = bufs['status'].cpu().numpy(), np.array(c.roles)
    assert status[3] == 0 and status[4] == 0 and roles[3] == 'up_few' and roles[4] == 'up_many'
    assert (status[np.isin(roles, ['failed', 'nonfinite'])] == 2).all()
    assert (status[~np.isin(roles, ['failed', 'nonfinite']) & ~np.isin(np.arange(G), [3, 4])] == 1).all()


# ----------------------------------------------------------------------------------------------------- end to end
def _replay(trace, cell0, gptr, fixed, dof, L, ftol, stol, p, hydrostatic, tag):
    """Every traced launch through the reference from its own recorded inputs (cell0: the caller's cell, never written)."""
    cpu = lambda v: v.cpu().numpy()
    worst = [0.0] * 5
    for i, r in enumerate(trace):
        sb, sa = {k: cpu(v) for k, v in r['state_before'].items()}, {k: cpu(v) for k, v in r['state_after'].items()}
        before = (cpu(r['pos']), cpu(r['v_before']), cpu(r['cell']), cpu(r['F']), cpu(r['vcell']), sb)
        got = (cpu(r['pos_after']), cpu(r['v_after']), cpu(r['cell_after']), cpu(r['F_after']), cpu(r['vcell_after']), sa)
        want = fire_cell_step_ref(before[0], before[1], cpu(r['dE']), cpu(r['W']), gptr, cell0, before[2], before[3], before[4], sb,
                                  ftol, stol, fixed, dof, L, p, hydrostatic, **DEFAULTS)
        w = _assert_cell_step_matches(got, want, before, gptr, fixed, dof, tag=(tag, i))
        worst = [max(a, b) for a, b in zip(worst, w)]
        if i + 1 < len(trace):
            nxt = trace[i + 1]
            assert torch.equal(r['pos_after'], nxt['pos']) and torch.equal(r['v_after'], nxt['v_before'])
            assert torch.equal(r['cell_after'], nxt['cell']) and torch.equal(r['F_after'], nxt['F'])
            assert torch.equal(r['vcell_after'], nxt['vcell'])
    return worst


def _well_on_device(w, dev):
    from pamnet_amd import synth
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).to(dev)
    model = ElasticWell(f32(w.k), f32(w.kappa), f32(w.cstar), f32(w.s))
    data = synth.Batch(pos=torch.from_numpy(w.pos0), batch=torch.from_numpy(w.batch), cell=torch.from_numpy(w.cell0),
                       num_graphs=len(W_SIZES)).to(dev)
    return model, data, torch.from_numpy(w.fixed).to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['aniso', 'hydro', 'aniso_p'])
def test_elastic_wells_relax_to_their_minimum_without_a_synchronisation(dev, kind):
    """ElasticWell through relax_cell with check_every=0 under torch's synchronisation debug mode (where torch has it), traced:
    every launch replayed through the reference from its own recorded inputs; every graph converged, each after its own number of
    steps; the result at the known minimum within _well_bounds, the thresholds widened by 1e-3 for the model's fp32 arithmetic
    (the step saw f and W evaluated in fp32: a few spacings of 5e-7 on coordinates below 8 against d = ftol / kappa >= 5e-3, and
    a relative 70 x 2^-24 on the sums of W); the caller's positions and cell untouched."""
    from pamnet_amd.relax import relax_cell
    w = _wells(kind)
    model, data, fixed = _well_on_device(w, dev)
    steps = int(w.state['steps'].max()) + 20
    debug = True
    try:
        torch.cuda.set_sync_debug_mode('error')
    except Exception as e:                        # (a build without the debug mode: the rest of the test runs as it is)
        print('set_sync_debug_mode is not available:', e)
        debug = False
    try:
        res = relax_cell(model, data, fmax=W_FTOL, smax=W_STOL, pressure=w.p, hydrostatic=w.hydrostatic, fixed=fixed,
                         max_steps=steps, check_every=0, trace=True)
    finally:
        if debug:
            torch.cuda.set_sync_debug_mode('default')
    assert len(res.trace) == steps and res.pos.is_cuda and res.cell.is_cuda
    assert torch.equal(data.pos.cpu(), torch.from_numpy(w.pos0)) and torch.equal(data.cell.cpu(), torch.from_numpy(w.cell0))
    assert res.pos is not data.pos and res.cell is not data.cell
    worst = _replay(res.trace, w.cell0, w.gptr, w.fixed, np.ones(len(W_SIZES), dtype=bool), w.L, W_FTOL, W_STOL, w.p, w.hydrostatic,
                    kind)
    print(kind, 'replay: worst vel / displacement / cell / F / vcell error', worst, 'steps', res.steps.tolist(), 'reference',
          w.state['steps'])
    assert res.converged.all() and not res.failed.any()
    assert len(set(res.steps.tolist())) == len(W_SIZES)
    assert (res.fmax < W_FTOL).all() and (res.smax < W_STOL).all()
    pos, cell = res.pos.cpu().numpy(), res.cell.cpu().numpy()
    vol = np.abs(np.linalg.det(cell.astype(np.float64)))
    assert np.allclose(res.volume.cpu().numpy(), vol, rtol=1e-12) and torch.equal(res.cell, res.trace[-1]['cell_after'])
    assert np.allclose(res.stress.cpu().numpy(), res.virial.cpu().numpy() / vol[:, None, None], rtol=1e-6, atol=0)
    assert np.abs(np.einsum('gij,gjk->gik', w.cell0.astype(np.float64), res.F.cpu().numpy()) - cell).max() <= 1e-6
    if kind != 'aniso_p':
        _assert_at_the_minimum(w, pos, cell, res.steps.cpu().numpy(), 1e-3, kind)
    else:                                         # under pressure: the fp64 gradients at the result, as the CPU test has them
        _, dE, W = _well_gradients(w, pos, cell)
        for g in range(len(W_SIZES)):
            s = slice(int(w.gptr[g]), int(w.gptr[g + 1]))
            f = dE[s][~w.fixed[s]]
            _, _, sm, _ = stress_terms(W[g], w.cell0[g], res.F[g].cpu().numpy(), w.L[g], w.p, False)
            assert float(np.sqrt((f * f).sum(1).max())) < W_FTOL * 1.001
            assert sm < W_STOL * 1.001 + 70 * EPS32 * np.abs(W[g]).max() / vol[g]


def _height_bound(cell, pbc, n_atoms, steps, max_step=DEFAULTS['max_step']):
    """A lower bound on the periodic heights of cell0 F after `steps` steps.  One step adds to each row of F at most max_step / L
    (the cap), so |F - I|_2 <= |F - I|_F <= steps sqrt(3) max_step / L =: x; the height of axis k is 1 / |column k of C^-1| with
    C^-1 = F^-1 cell0^-1, hence at least height0 sigma_min(F) >= height0 (1 - x)."""
    from test_pbc_axes import _axis_heights
    x = steps * np.sqrt(3.0) * max_step / n_atoms
    return min(_axis_heights(cell, pbc)) * (1.0 - x)


P_STEPS, SMALL_CELL = 8, [[6.0, 0.0, 0.0], [0.5, 6.0, 0.0], [-0.25, 0.5, 6.25]]


def _pamnet_batch(mode):
    """'minimum': [48 atoms in the triclinic cell TRI_A, the slab slab_min of tests/test_pbc_axes.py with pbc = (True, True, False)];
    'all' (cell_images='all'): a 12-atom cell of about 6 A, below twice the global cutoff, between them.  And the slab's bottom
    layer (the third of its atoms lowest along the open axis) as the fixed mask."""
    if ('pamnet', mode) in _MADE:
        return _MADE[('pamnet', mode)]
    from test_pbc_axes import TRI_A, Struct, _batch, _scatter, _structs
    rng = np.random.RandomState(5)
    full = (True, True, True)
    tri = Struct(rng.randint(0, 5, 48).astype(np.float32), _scatter(rng, 48, TRI_A, full, {}, 2).astype(np.float32), TRI_A, full, 2)
    small = Struct(rng.randint(0, 5, 12).astype(np.float32), _scatter(rng, 12, SMALL_CELL, full, {}, 3).astype(np.float32),
                   SMALL_CELL, full, 3)
    slab = _structs()['slab_min']
    structs = [tri, small, slab] if mode == 'all' else [tri, slab]
    b = _batch(structs)
    if mode == 'all':
        b.cell_images = 'all'
    z = slab.pos[:, 2]
    fixed = np.zeros(b.pos.size(0), dtype=bool)
    fixed[-slab.n:] = z <= np.sort(z)[slab.n // 3 - 1]
    _MADE[('pamnet', mode)] = (b, torch.from_numpy(fixed), structs)
    return _MADE[('pamnet', mode)]


@pytest.mark.parametrize('mode', ['minimum', 'all'])
def test_eight_capped_steps_keep_the_height_conditions_of_the_pamnet_batch(mode):
    """(No GPU.)  With the default cell factor (the atoms of the graph) eight steps at the cap max_step / L cannot bring a periodic
    height of the cells that relax to the limit of the graph build: 2 max(cutoff_l, cutoff_g) = 10 for minimum images,
    2 cutoff_l = 4 (and cutoff_g / 4) with cell_images='all'.  The slab has an open axis: it relaxes at fixed cell."""
    from test_pbc_axes import CUT_G, CUT_L
    b, fixed, structs = _pamnet_batch(mode)
    limit = 2 * CUT_L if mode == 'all' else 2 * max(CUT_L, CUT_G)
    for st in structs:
        if all(st.pbc):
            low = _height_bound(st.cell, st.pbc, st.n, P_STEPS)
            print(mode, st.n, 'atoms: heights stay above', low, 'limit', limit)
            assert low > 1.02 * limit and low > CUT_G / 4
    assert [all(st.pbc) for st in structs] == [True] * (len(structs) - 1) + [False] and int(fixed.sum()) == structs[-1].n // 3


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['minimum', 'all'])
@pytest.mark.parametrize('dim,n_layer', MODELS)
def test_pamnet_cell_relaxation_replayed_step_by_step(dev, dim, n_layer, mode):
    """PAMNet on {triclinic cell, (a small cell with cell_images='all',) slab with a fixed bottom layer}, trace=True, 8 steps under
    a pressure: every recorded step, replayed alone through fire_cell_step_ref from its recorded inputs, matches as in the kernel
    test; the slab relaxes at fixed cell (its cell_dof comes from pbc); res.energy / res.forces / res.virial are bitwise a fresh
    plain evaluation at res.pos and res.cell; the caller's batch and every parameter .grad are as they were."""
    import models
    from pamnet_amd.relax import relax_cell
    from test_pbc_axes import CUT_G, CUT_L
    b, fixed_cpu, structs = _pamnet_batch(mode)
    G = len(structs)
    torch.manual_seed(0)
    model = models.PAMNet(models.Config(dataset='QM9', dim=dim, n_layer=n_layer, cutoff_l=CUT_L, cutoff_g=CUT_G)).to(dev)
    data, fixed = b.to(dev), fixed_cpu.to(dev)
    model(data).sum().backward()                                   # parameter gradients to find untouched afterwards
    snap = [None if p.grad is None else p.grad.clone() for p in model.parameters()]
    pos0, cell0 = data.pos.clone(), data.cell.clone()
    res = relax_cell(model, data, fmax=1e-6, smax=1e-9, pressure=0.01, max_steps=P_STEPS, fixed=fixed, trace=True)
    assert torch.equal(data.pos, pos0) and torch.equal(data.cell, cell0) and not data.pos.requires_grad
    assert getattr(data, 'strain', None) is None
    for p, s in zip(model.parameters(), snap):
        assert (p.grad is None) if s is None else torch.equal(p.grad, s)
    assert len(res.trace) == P_STEPS and res.steps.tolist() == [P_STEPS] * G and not res.converged.any() and not res.failed.any()
    dof = np.array([all(st.pbc) for st in structs])
    gptr = np.concatenate([[0], np.cumsum([st.n for st in structs])])
    L = np.array([float(st.n) for st in structs])
    worst = _replay(res.trace, b.cell.numpy(), gptr, fixed_cpu.numpy(), dof, L, 1e-6, 1e-9, 0.01, False, (dim, mode))
    print('replay: worst vel / displacement / cell / F / vcell error', worst)
    eye = torch.eye(3, dtype=torch.float64, device=dev)
    assert torch.equal(res.cell[-1], cell0[-1]) and torch.equal(res.F[-1], eye) and torch.equal(res.pos[fixed], pos0[fixed])
    assert all(not torch.equal(res.cell[g], cell0[g]) for g in range(G - 1))
    assert torch.equal(res.trace[-1]['pos_after'], res.pos) and torch.equal(res.trace[-1]['cell_after'], res.cell)

    def fresh(pos, cell):
        d = copy.copy(data)
        d.pos, d.cell = pos.clone().requires_grad_(True), cell.clone()
        d.strain = torch.zeros(G, 3, 3, device=dev, requires_grad=True)
        e = model(d)
        return (e.detach(),) + torch.autograd.grad(e.sum(), [d.pos, d.strain])

    _, de, w = fresh(res.trace[3]['pos'], res.trace[3]['cell'])
    assert torch.equal(de, res.trace[3]['dE']) and torch.equal(w, res.trace[3]['W'])
    e, de, w = fresh(res.pos, res.cell)
    assert torch.equal(res.energy, e) and torch.equal(res.forces, -de) and torch.equal(res.virial, w)
    assert torch.isfinite(res.forces).all() and torch.isfinite(res.virial).all() and float(res.virial[0].abs().max()) > 0
    assert torch.isfinite(res.stress[:-1]).all() and (res.volume[:-1] > 0).all()


@pytest.mark.gpu
def test_relax_cell_refusals(dev):
    """A batch without `cell`, wrong shapes, dtypes and devices, a cell factor that is not positive, and cell_dof set on a graph
    with an open axis are refused before anything moves."""
    from pamnet_amd.relax import relax_cell
    w = _wells('aniso')
    model, data, fixed = _well_on_device(w, dev)
    G = len(W_SIZES)
    ok = dict(fmax=W_FTOL, smax=W_STOL, max_steps=2)
    bare = copy.copy(data)
    bare.cell = None
    with pytest.raises(ValueError, match='no `cell`'):
        relax_cell(model, bare, **ok)
    for cell in (data.cell[:2], data.cell.double(), data.cell.cpu(), data.cell.reshape(G, 9)):
        d = copy.copy(data)
        d.cell = cell
        with pytest.raises(ValueError, match='`data.cell` is a float32 tensor'):
            relax_cell(model, d, **ok)
    f64 = lambda v: torch.tensor(v, dtype=torch.float64, device=dev)
    for kw, match in ((dict(cell_factor=0.0), '`cell_factor` must be positive'),
                      (dict(cell_factor=float('inf')), '`cell_factor` must be'),
                      (dict(cell_factor=f64([4.0, -1.0, 70.0])), '`cell_factor` must be finite'),
                      (dict(cell_factor=f64([4.0, 9.0, 70.0]).float()), 'per-graph `cell_factor`'),
                      (dict(cell_factor=f64([4.0, 9.0])), 'per-graph `cell_factor`'), (dict(cell_factor='n'), '`cell_factor`'),
                      (dict(pressure=f64([0.0, float('nan'), 0.0])), '`pressure` must be finite'),
                      (dict(pressure=float('inf')), '`pressure` must be finite'),
                      (dict(pressure=f64([0.0] * 3).cpu()), 'per-graph `pressure`'),
                      (dict(smax=f64([1e-4] * 3)), 'per-graph `smax`'), (dict(smax=[1e-4] * 3), '`smax`'),
                      (dict(cell_dof=[True] * 3), '`cell_dof` is a torch.bool tensor'),
                      (dict(cell_dof=torch.ones(3, device=dev)), '`cell_dof` is a torch.bool tensor'),
                      (dict(cell_dof=torch.ones(2, dtype=torch.bool, device=dev)), '`cell_dof` is a torch.bool tensor')):
        with pytest.raises(ValueError, match=match):
            relax_cell(model, data, **dict(ok, **kw))
    with pytest.raises(TypeError, match='dt_min'):
        relax_cell(model, data, dt_min=0.01, **ok)
    slab = copy.copy(data)
    slab.pbc = torch.tensor([[True] * 3, [True, True, False], [True] * 3], device=dev)
    yes = torch.ones(G, dtype=torch.bool, device=dev)
    with pytest.raises(ValueError, match='open axis'):
        relax_cell(model, slab, cell_dof=yes, **ok)
    slab.pbc = (True, False, True)
    with pytest.raises(ValueError, match='open axis'):
        relax_cell(model, slab, cell_dof=yes, **ok)
    # accepted: the default leaves the graph with the open axis at fixed cell, and a given mask may switch a periodic graph off
    slab.pbc = torch.tensor([[True] * 3, [True, True, False], [True] * 3], device=dev)
    res = relax_cell(model, slab, cell_factor=f64([4.0, 9.0, 70.0]), pressure=f64([0.0] * 3),
                     **dict(ok, smax=torch.full((G,), 1e-4, device=dev)))
    assert torch.equal(res.cell[1], data.cell[1]) and not torch.equal(res.cell[0], data.cell[0])
    res = relax_cell(model, data, cell_dof=torch.tensor([False, True, True], device=dev), **ok)
    assert torch.equal(res.cell[0], data.cell[0]) and not torch.equal(res.cell[1], data.cell[1])
    assert torch.equal(data.pos.cpu(), torch.from_numpy(w.pos0))


@pytest.mark.gpu
def test_a_periodic_store_batch_is_relaxed_with_its_cells(dev):
    """A periodic MoleculeStore batch (cells of 10.5 A and more, minimum images: heights above 10) through relax_cell, five steps
    with a cell factor of 50 -- the strain moves by at most 5 sqrt(3) 0.2 / 50 = 3.5 %, which keeps 10.5 x 0.965 = 10.13 above the
    limit: the model's deferred checks are clean and none is pending, and res.energy / res.forces / res.virial are bitwise a
    plain-tensor evaluation at res.pos and res.cell."""
    from pamnet_amd import store as S
    from pamnet_amd.relax import relax_cell
    from test_pbc import _heights
    from test_store_pbc import ORDER, _items, _model, _plain
    items, steps, factor = _items(), 5, 50.0
    assert min(min(_heights(d['cell'])) for d in items) * (1.0 - steps * np.sqrt(3.0) * DEFAULTS['max_step'] / factor) > 10.1
    model = _model(dev)
    st = S.MoleculeStore(items, dev).prepare_for(model)
    bt = st.collate(ORDER)
    assert bt.mol_local[S.size_key(model, False)] is True and bt.cell is not None
    cell0 = bt.cell.clone()
    res = relax_cell(model, bt, fmax=0.0, smax=0.0, cell_factor=factor, max_steps=steps)      # (thresholds of 0: nothing converges)
    assert res.steps.tolist() == [steps] * len(ORDER) and torch.isfinite(res.energy).all() and torch.equal(bt.cell, cell0)
    moved = [not torch.equal(res.cell[g], cell0[g]) for g in range(len(ORDER))]
    assert sum(moved) >= len(ORDER) - 1, moved                      # (the lone atom feels nothing: its cell stays)
    model.verify()                                                 # nothing was flagged on the way ...
    assert not model._pending_checks                               # ... and nothing waits
    plain = _plain(items, ORDER, dev)
    assert torch.equal(plain.pos, bt.pos)
    plain.pos, plain.cell = res.pos.clone().requires_grad_(True), res.cell.clone()
    plain.strain = torch.zeros(len(ORDER), 3, 3, device=dev, requires_grad=True)
    e = model(plain)
    de, w = torch.autograd.grad(e.sum(), [plain.pos, plain.strain])
    assert torch.equal(res.energy, e.detach()) and torch.equal(res.forces, -de) and torch.equal(res.virial, w)
