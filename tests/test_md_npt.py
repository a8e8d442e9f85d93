"""Constant-pressure molecular dynamics: the kernel pamnet_md_npt_step_f32 (csrc/md_npt.hip) and the driver pamnet_amd/md.py
run_npt.

The reference is tests/md_npt_ref.py: md_npt_step_ref, the rule of include/pamnet_hip.h restated in numpy fp64 over the generator
and the fixed-cell step of tests/md_ref.py.  Inputs are made once on the CPU with fixed seeds and never modified; what the
end-to-end tests presuppose of the reference is asserted by tests that need no GPU.

Tolerances: KTOL = 1e-6 max-normalised (tests/test_md.py) per graph for the velocities, the displacement pos_new - pos_old and
the change cell_new - cell_old (not pos or cell, whose magnitude would hide an error); 1e-12 relative for the fp64 ke, pint, vol
and eps, and for the change of eps beside the rounding of the sum; equality for steps, status and everything that must stay unwritten."""
import copy
import warnings

import numpy as np
import pytest
import torch

from conftest import maxnorm_err
from md_npt_ref import NPT_STATE, barostat_normal, det3, md_npt_step_ref, npt_batch_ref
from md_ref import STATE, md_step_ref, normals
from test_md import FLAGS, KTOL, MODELS, SIZES

ENTRY, FIXED_ENTRY = 'pamnet_md_npt_step_f32', 'pamnet_md_step_f32'
ROLES = ['langevin', 'kt0', 'nve', 'some_fixed', 'all_fixed', 'fixed_cell', 'failed', 'w_nan', 'f_inf', 'singular', 'rate_big',
         'd_nonfinite']
SHIFTS = (0, 4, 8)                                # graph i plays ROLES[(i + shift) % 12]: together every role; the empty graph is last
BARO_FAILS = ('w_nan', 'f_inf', 'singular', 'd_nonfinite')
EPS32 = 2.0 ** -24


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
    """One batch of SIZES.  Every graph: a triclinic cell0 (about 8 A, volume about 500), a starting eps in [-0.2, 0.2] with
    cell = fp32(cell0 exp(eps / 3)), a virial W with random entries, per-graph dt in [0.02, 0.1], masses in [1, 40], steps in [0, 40),
    seeds over all of int64, kT = 0.7, gamma = 2, a target pressure in [-1, 1], and a rate that makes the drift of eps
    rate |P0 - P_int| dt between 0.025 and 0.1 (P_int taken with the half kick).  The roles:
      langevin     as above                                     kt0        kT = 0: no noise, from thermostat or barostat
      nve          gamma = 0: the barostat's noise alone        some_fixed half of the atoms fixed (they follow the cell)
      all_fixed    every atom fixed: the cell moves alone       fixed_cell cell_dof = 0; its W, cell0, pressure and rate are NaN
      failed       status 2, with NaN / inf in vel, dE, W, eps  w_nan      a diagonal entry of W NaN (inf at shift 4)
      f_inf        one gradient entry of a free atom infinite   singular   cell0 has a zero row (all zero at shift 8): V == 0
      rate_big     the drift 60 times larger: |d| of 1.5 to 6   d_nonfinite rate = 1e308, P0 = 1000: d overflows
    A graph of 63 atoms or more has a fifth of its atoms fixed, with velocities that must enter no sum."""
    if shift in _MADE:
        return _MADE[shift]
    rng = np.random.RandomState(400 + shift)
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
    c.p0, c.rate = rng.uniform(-1.0, 1.0, G), np.ones(G)
    c.dof = np.ones(G, dtype=bool)
    c.cell0 = (8.0 * np.eye(3) + rng.uniform(-1.5, 1.5, (G, 3, 3))).astype(np.float32)
    c.W = (40.0 * rng.standard_normal((G, 3, 3))).astype(np.float32)
    eps = rng.uniform(-0.2, 0.2, G)
    c.state = dict(seed=rng.randint(-2 ** 63, 2 ** 63 - 1, G, dtype=np.int64), steps=rng.randint(0, 40, G).astype(np.int32),
                   status=np.zeros(G, np.int32), ke=np.full(G, -1.0), eps=eps, pint=np.full(G, -2.0), vol=np.full(G, -3.0))
    for g, role in enumerate(c.roles):
        lo, hi = int(c.gptr[g]), int(c.gptr[g + 1])
        m = hi - lo
        if role == 'all_fixed':
            c.fixed[lo:hi] = True
        elif role == 'some_fixed' and m >= 2:
            c.fixed[lo + rng.choice(m, m // 2, replace=False)] = True
        elif m >= 63:
            c.fixed[lo + rng.choice(m, m // 5, replace=False)] = True
        free = lo + np.nonzero(~c.fixed[lo:hi])[0]
        # the pressure of the graph with the half kick, to size the rate by
        v = c.vel[free].astype(np.float64) - 0.5 * c.dt[g] * c.dE[free].astype(np.float64) / c.mass[free].astype(np.float64)[:, None]
        ke = 0.5 * float((c.mass[free].astype(np.float64)[:, None] * v * v).sum())
        vol = abs(det3(c.cell0[g])) * np.exp(eps[g])
        pint = (2.0 * ke - float(np.trace(c.W[g].astype(np.float64)))) / (3.0 * vol)
        c.rate[g] = rng.uniform(0.025, 0.1) / (c.dt[g] * abs(c.p0[g] - pint))
        if role == 'singular':                                     # (sized before its row is zeroed: V is 0 afterwards)
            c.cell0[g, 2 if shift != 8 else slice(None)] = 0.0
        if role == 'nve':
            c.gamma[g] = 0.0
        elif role == 'kt0':
            c.kT[g] = 0.0
        elif role == 'fixed_cell':
            c.dof[g] = False
            c.W[g], c.cell0[g], c.p0[g], c.rate[g] = np.nan, np.nan, np.nan, np.nan
        elif role == 'failed':
            c.state['status'][g] = 2
            c.state['eps'][g] = np.nan
            c.W[g, 0, 0] = np.inf
            if m:
                c.vel[lo, 0], c.dE[hi - 1, 2] = np.nan, np.inf
        elif role == 'w_nan':
            c.W[g, 1, 1] = np.inf if shift == 4 else np.nan
        elif role == 'f_inf':
            c.dE[free[len(free) // 2], 1] = np.inf
        elif role == 'rate_big':
            c.rate[g] *= 60.0
        elif role == 'd_nonfinite':
            c.rate[g], c.p0[g] = 1e308, 1000.0
    with np.errstate(all='ignore'):
        c.cell = (c.cell0.astype(np.float64) * np.exp(eps / 3.0)[:, None, None]).astype(np.float32)
    _MADE[shift] = c
    return c


def _ref(c, kick_in, advance, mass=True):
    key = ('ref', id(c), kick_in, advance, mass)
    if key not in _MADE:
        _MADE[key] = md_npt_step_ref(c.pos, c.vel, c.dE, c.W, c.gptr, c.cell0, c.cell, c.state, c.dt, c.kT, c.gamma, c.p0, c.rate,
                                     c.mass if mass else None, c.fixed, c.dof, kick_in, advance)
    return _MADE[key]


def _indep_graphs():
    """One NPT Langevin graph per size of SIZES, each with its own atoms, cell, eps, virial, seed, step counter, dt, kT, gamma,
    pressure and rate: the pieces of the batches of the independence test."""
    if 'indep' in _MADE:
        return _MADE['indep']
    rng = np.random.RandomState(41)
    out = []
    for m in SIZES:
        fixed = np.zeros(m, dtype=bool)
        if m >= 63:
            fixed[rng.choice(m, m // 5, replace=False)] = True
        cell0 = (8.0 * np.eye(3) + rng.uniform(-1.5, 1.5, (3, 3))).astype(np.float32)
        eps = rng.uniform(-0.2, 0.2)
        out.append(dict(pos=rng.uniform(-4.0, 4.0, (m, 3)).astype(np.float32), vel=rng.standard_normal((m, 3)).astype(np.float32),
                        dE=rng.standard_normal((m, 3)).astype(np.float32), mass=rng.uniform(1.0, 40.0, m).astype(np.float32),
                        fixed=fixed, dt=rng.uniform(0.02, 0.1), kT=rng.uniform(0.1, 1.0), gamma=rng.uniform(0.5, 4.0),
                        p0=rng.uniform(-1.0, 1.0), rate=rng.uniform(1e-4, 1e-3), cell0=cell0, eps=eps,
                        cell=(cell0.astype(np.float64) * np.exp(eps / 3.0)).astype(np.float32),
                        W=(40.0 * rng.standard_normal((3, 3))).astype(np.float32),
                        seed=int(rng.randint(-2 ** 63, 2 ** 63 - 1, dtype=np.int64)), steps=int(rng.randint(0, 40))))
    _MADE['indep'] = out
    return out


def _assemble(graphs):
    """A Case from a list of graph records (_indep_graphs), in the order given."""
    c = Case()
    G = len(graphs)
    c.gptr = _gptr([len(g['pos']) for g in graphs])
    c.roles = ['langevin'] * G
    cat = lambda k, shape, dt: np.concatenate([g[k] for g in graphs]).reshape(shape).astype(dt)
    c.pos, c.vel, c.dE = cat('pos', (-1, 3), np.float32), cat('vel', (-1, 3), np.float32), cat('dE', (-1, 3), np.float32)
    c.mass, c.fixed = cat('mass', (-1,), np.float32), cat('fixed', (-1,), bool)
    c.dt, c.kT, c.gamma, c.p0, c.rate = (np.array([g[k] for g in graphs], dtype=np.float64) for k in ('dt', 'kT', 'gamma', 'p0', 'rate'))
    c.cell0, c.cell, c.W = (np.stack([g[k] for g in graphs]).astype(np.float32) for k in ('cell0', 'cell', 'W'))
    c.dof = np.ones(G, dtype=bool)
    c.state = dict(seed=np.array([g['seed'] for g in graphs], dtype=np.int64),
                   steps=np.array([g['steps'] for g in graphs], dtype=np.int32), status=np.zeros(G, np.int32), ke=np.zeros(G),
                   eps=np.array([g['eps'] for g in graphs], dtype=np.float64), pint=np.zeros(G), vol=np.zeros(G))
    return c


# ------------------------------------------------------------------------------------------- the models of the physics tests
def _eye_plus(strain):
    return torch.eye(3, dtype=torch.float64, device=strain.device) + strain.double()


class VolumeWell(torch.nn.Module):
    """E_g = 1/2 B_g (V_g - V0_g)^2 / V0_g with V_g = det(cell_g (I + strain_g)) in fp64: a plain torch module whose forces are
    zero and whose virial is B (V - V0) / V0 V I, so P_int = -B (V - V0) / V0 at rest and the volume at the pressure P0 is
    V0 (1 - P0 / B)."""

    def __init__(self, B, V0):
        super().__init__()
        self.register_buffer('B', B)
        self.register_buffer('V0', V0)

    def forward(self, data):
        from pamnet_amd.relax import _det3
        V = _det3(data.cell.double() @ _eye_plus(data.strain))
        still = torch.zeros_like(self.B).index_add_(0, data.batch, data.pos.double().sum(1))
        return 0.5 * self.B * (V - self.V0) ** 2 / self.V0 + 0.0 * still


class IdealGas(torch.nn.Module):
    """E_g = 0 sum (pos (I + strain_g)): no forces, no virial, and differentiable with respect to both."""

    def forward(self, data):
        x = torch.einsum('ni,nij->nj', data.pos.double(), _eye_plus(data.strain)[data.batch])
        return 0.0 * torch.zeros(data.strain.size(0), dtype=torch.float64, device=x.device).index_add_(0, data.batch, x.sum(1))


# deterministic relaxation: three graphs, kT = 0, at rest
R_DT, R_STEPS, R_RB = 0.05, 150, 0.2              # rate_g = R_RB / (B_g dt): rate B dt = 0.2
R_B = np.array([2.0, 10.0, 0.5])
R_P0 = np.array([0.3, -1.0, 0.02])
R_SIZES = (3, 1, 5)
R_CELL0 = np.array([[[6.0, 0.0, 0.0], [0.5, 6.0, 0.0], [-0.25, 0.5, 6.25]],
                    [[4.0, 0.5, 0.0], [0.0, 5.0, 0.25], [1.0, 0.0, 4.5]],
                    [[7.0, 0.0, 0.0], [0.0, 7.0, 0.0], [0.0, 0.0, 7.0]]], dtype=np.float32)
R_START = np.array([1.1, 0.92, 1.05])             # |det cell0| / V0


def _relaxation():
    """(the well's inputs, the reference trajectory of md_npt_step_ref from rest with the virial of VolumeWell formed in fp64 from
    the fp32 cell and rounded to fp32, as the module hands it over; the a-priori bound).
    The bound on |V / V* - 1|.  With x = eps - eps*, one step is x <- x (1 - r B V(xi) / V0), r = rate dt, xi between eps and
    eps* (mean value theorem on P_int(eps) = -B (V0' e^eps - V0) / V0).  With r B max(V) / V0 < 1 the factor lies in (0, q],
    q = 1 - r B min(V_start, V*) / V0, so |x_n| <= |x_0| q^n; and |V / V* - 1| <= e^|x| - 1.  On top of it the fp32 cell: the
    module's volume is the determinant of a cell whose nine entries each carry a relative rounding of 2^-24, three factors per
    term -- 3 x 2^-24, doubled for the cancellation in a triclinic determinant -- and its virial is rounded once more: 8 x 2^-24
    in all, which at 150 steps is all that is left (q^150 < 1e-12)."""
    if 'relax' in _MADE:
        return _MADE['relax']
    w = Case()
    G, n = len(R_B), sum(R_SIZES)
    w.gptr, w.batch = _gptr(R_SIZES), np.repeat(np.arange(G), R_SIZES)
    w.cell0 = R_CELL0
    vol0 = np.array([abs(det3(c)) for c in R_CELL0])
    w.V0 = vol0 / R_START
    w.vstar = w.V0 * (1.0 - R_P0 / R_B)
    w.rate = R_RB / (R_B * R_DT)
    rng = np.random.RandomState(12)
    w.pos0 = np.concatenate([rng.uniform(0, 1, (m, 3)) @ R_CELL0[g].astype(np.float64) for g, m in enumerate(R_SIZES)]).astype(np.float32)
    w.fixed = np.zeros(n, dtype=bool)
    w.fixed[0] = True
    x0 = np.abs(np.log(vol0 / w.vstar))
    q = 1.0 - R_RB * np.minimum(vol0, w.vstar) / w.V0
    assert (R_RB * np.maximum(vol0, w.vstar) / w.V0 < 1.0).all() and (q > 0).all()
    w.bound = np.expm1(x0 * q ** R_STEPS) + 8 * EPS32
    pos, vel, cell = w.pos0.copy(), np.zeros((n, 3), np.float32), w.cell0.copy()
    st = dict(seed=None, steps=np.zeros(G, np.int32), status=np.zeros(G, np.int32), ke=np.zeros(G), eps=np.zeros(G),
              pint=np.zeros(G), vol=np.zeros(G))
    w.vols = np.zeros((R_STEPS + 1, G))
    for it in range(R_STEPS + 1):
        V = np.array([det3(c) for c in cell])
        W = ((R_B * (V - w.V0) / w.V0 * V)[:, None, None] * np.eye(3)).astype(np.float32)
        pos, vel, cell, st = md_npt_step_ref(pos, vel, np.zeros((n, 3), np.float32), W, w.gptr, w.cell0, cell, st, R_DT, 0.0, 0.0,
                                             R_P0, w.rate, None, w.fixed, None, 1 if it else 0, 1 if it < R_STEPS else 0)
        w.vols[it] = st['vol']
    w.pos, w.cell, w.state = pos, cell, st
    _MADE['relax'] = w
    return w


# ideal gas: G graphs of N free atoms of unit mass
GAS = dict(G=256, N=4, kT=1.0, p0=1.0, dt=0.05, rate=0.4, gamma=2.0, burn=300, stride=120, steps=2100)
GAS_SIGMAS = 4.0
GAS_BIAS_MEAN, GAS_BIAS_VAR = 0.005, 0.01         # the rule's O(dt) bias at rate dt = 0.02, measured on the reference (below)
GAS_RHO = 0.2                                     # the largest correlation of successive samples the tolerance allows for


def _gas_tolerances():
    """(n_eff, tolerance on mean / ((N + 1) kT / P0) - 1, tolerance on var / ((N + 1) (kT / P0)^2) - 1).
    Samples: G graphs x F records, successive records of a graph correlated by at most GAS_RHO (asserted of the reference), so
    n_eff = n (1 - rho) / (1 + rho).  A Gamma(k) variable, k = N + 1, has relative standard deviation 1 / sqrt(k) and kurtosis
    3 + 6 / k: the mean of n_eff samples has the relative standard error 1 / sqrt(k n_eff), their variance sqrt((2 + 6 / k) / n_eff).
    GAS_SIGMAS standard errors plus the bias of the first-order rule: the reference run over 4096 graphs (16 times the test's)
    gave mean / 5 = 1.0030 and var / 5 = 1.0048 at these parameters, 1.0085 and 1.0158 at twice the rate, 1.0006 and 0.9979 at half
    of it (standard errors 0.002 and 0.008) -- linear in rate dt, as a first-order scheme's is; 0.005 and 0.01 cover it."""
    k = GAS['N'] + 1
    n = GAS['G'] * ((GAS['steps'] - GAS['burn'] - 1) // GAS['stride'] + 1)
    n_eff = n * (1.0 - GAS_RHO) / (1.0 + GAS_RHO)
    return n_eff, GAS_SIGMAS / np.sqrt(k * n_eff) + GAS_BIAS_MEAN, GAS_SIGMAS * np.sqrt((2.0 + 6.0 / k) / n_eff) + GAS_BIAS_VAR


def _gas_records():
    """The records run_npt takes with record_every = stride that lie past the burn-in."""
    return [i for i in range(GAS['steps'] // GAS['stride'] + 1) if i * GAS['stride'] >= GAS['burn']]


def _gas_reference():
    """npt_batch_ref iterated with numpy's normals (the statistics do not depend on the generator): volumes and kinetic
    energies [F, G]."""
    if 'gas' in _MADE:
        return _MADE['gas']
    rng = np.random.RandomState(7)
    G, N, kT = GAS['G'], GAS['N'], GAS['kT']
    pos, vel = rng.uniform(0, 1, (G, N, 3)), np.sqrt(kT) * rng.standard_normal((G, N, 3))
    f, eps, V0 = np.zeros((G, N, 3)), np.zeros(G), (N + 1) * kT / GAS['p0']
    vols, kes = [], []
    for it in range(GAS['steps'] + 1):
        pos, vel, eps, ke, _, vol = npt_batch_ref(pos, vel, f, 0.0, V0, eps, GAS['dt'], kT, GAS['gamma'], GAS['p0'], GAS['rate'],
                                                 rng.standard_normal((G, N, 3)), rng.standard_normal(G), 1 if it else 0)
        if it % GAS['stride'] == 0 and it >= GAS['burn']:
            vols.append(vol), kes.append(ke)
    _MADE['gas'] = (np.array(vols), np.array(kes))
    return _MADE['gas']


def _gas_moments(vols):
    k, unit = GAS['N'] + 1, GAS['kT'] / GAS['p0']
    rho = np.corrcoef(vols[:-1].ravel(), vols[1:].ravel())[0, 1]
    return vols.mean() / (k * unit) - 1.0, vols.var() / (k * unit * unit) - 1.0, rho


# ---------------------------------------------------------------------------------------------------------- CPU tests
def test_header_declares_the_npt_step_at_abi_18():
    """(No GPU: the header and the built library.)"""
    import ctypes
    import re
    from pamnet_amd import build, lib
    decl = lib.declared_functions()
    P, D, I64, I32 = ctypes.c_void_p, ctypes.c_double, ctypes.c_int64, ctypes.c_int32
    assert decl[ENTRY] == [P] * 7 + [I64] * 2 + [P] * 10 + [P] * 5 + [D] * 5 + [I32] * 2 + [P]
    assert int(re.search(r'#define\s+PAMNET_ABI_VERSION\s+(\d+)', open(lib.HEADER).read()).group(1)) == 18
    h = ctypes.CDLL(build.build())
    assert h.pamnet_abi_version() == 18 and hasattr(h, ENTRY) and hasattr(h, FIXED_ENTRY)


def test_npt_kernel_is_scratch_free(tmp_path):
    """(No GPU: hipcc cross-compiles.)  The compiler's report for csrc/md_npt.hip: no scratch, and the LDS of the four wavefront
    partials (DESIGN section 11a quotes the figures)."""
    import os
    import re
    import shutil
    import subprocess
    from pamnet_amd import build
    hipcc = '/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else shutil.which('hipcc')
    assert hipcc, 'hipcc not available'
    r = subprocess.run([hipcc] + build.FLAGS + ['-c', os.path.join(build.CSRC, 'md_npt.hip'), '-o', str(tmp_path / 'md_npt.o'),
                                                '-Rpass-analysis=kernel-resource-usage'], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = [b for b in re.split(r'remark: Function Name: ', r.stderr)[1:] if 'md_npt_step_kernel' in b.split()[0]]
    assert len(blocks) == 1
    num = lambda key: int(re.search(key + r': (\d+)', blocks[0]).group(1))
    assert num(r'ScratchSize \[bytes/lane\]') == 0
    assert num(r'LDS Size \[bytes/block\]') <= 256


def test_the_barostat_normal_is_the_first_of_stream_two():
    """(No GPU.)  xi_c of the reference is normals(seed, 1, step, 2)[0, 0]: atom offset 0, stream 2; it differs from the streams of
    the thermostat and of the initial velocities, changes with seed and step, and the reference's step uses exactly it."""
    for seed, step in ((0, 0), (-5, 7), (2 ** 40 + 3, 39), (-2 ** 63, 2 ** 31 - 1)):
        x = barostat_normal(seed, step)
        assert x == normals(seed, 1, step, 2)[0, 0] == normals(seed, 9, step, 2)[0, 0]
        assert x != normals(seed, 1, step, 0)[0, 0] and x != normals(seed, 1, step, 1)[0, 0]
        assert x != barostat_normal(seed + 1, step) and x != barostat_normal(seed, step + 1)
    # one step of an empty graph at rest: d = -rate (P0 - P_int) dt + sqrt(2 kT rate dt / V) xi_c, read back from eps
    cell0 = (2.0 * np.eye(3, dtype=np.float32))[None]
    st = dict(seed=np.array([77], np.int64), steps=np.array([5], np.int32), status=np.zeros(1, np.int32), ke=np.zeros(1),
              eps=np.zeros(1), pint=np.zeros(1), vol=np.zeros(1))
    z = np.zeros((0, 3), np.float32)
    _, _, cell, out = md_npt_step_ref(z, z, z, np.zeros((1, 3, 3), np.float32), [0, 0], cell0, cell0, st, 0.1, 0.5, 0.0, 0.25, 3.0)
    want = -3.0 * 0.25 * 0.1 + np.sqrt(2 * 0.5 * 3.0 * 0.1 / 8.0) * barostat_normal(77, 5)
    assert abs(out['eps'][0] - want) <= 1e-15 and out['vol'][0] == 8.0 and out['pint'][0] == 0.0 and out['steps'][0] == 6
    assert np.array_equal(cell, (cell0.astype(np.float64) * np.exp(out['eps'][0] / 3.0)).astype(np.float32))


def test_npt_inputs_take_their_intended_branches():
    """(No GPU.)  The kernel-test batches play every role and the reference takes the branch the role names under every pair of
    flags, with masses and without."""
    seen = set()
    for shift in SHIFTS:
        c = _kernel_case(shift)
        assert [int(b - a) for a, b in zip(c.gptr[:-1], c.gptr[1:])] == SIZES
        for kick_in, advance in FLAGS:
            for mass in (True, False):
                pos, vel, cell, st = _ref(c, kick_in, advance, mass)
                for g, role in enumerate(c.roles):
                    s = slice(int(c.gptr[g]), int(c.gptr[g + 1]))
                    moved = not np.array_equal(pos[s], c.pos[s])
                    same_cell = np.array_equal(cell[g], c.cell[g], equal_nan=True)
                    same_eps = st['eps'][g] == c.state['eps'][g] or np.isnan(c.state['eps'][g])
                    tag = (shift, kick_in, advance, mass, role, g)
                    if role == 'failed' or role in BARO_FAILS:
                        assert st['status'][g] == 2 and st['steps'][g] == c.state['steps'][g] and not moved and same_cell and same_eps, tag
                        assert np.array_equal(vel[s], c.vel[s], equal_nan=True), tag
                        assert (st['ke'][g] == -1.0 and st['pint'][g] == -2.0 and st['vol'][g] == -3.0) == (role == 'failed'), tag
                        if role == 'singular':
                            assert st['vol'][g] == 0.0 and not np.isfinite(st['pint'][g]), tag
                        if role == 'd_nonfinite':
                            assert np.isfinite(st['ke'][g]) and np.isfinite(st['pint'][g]) and st['vol'][g] > 0, tag
                        if role == 'w_nan':
                            assert not np.isfinite(st['pint'][g]) and np.isfinite(st['ke'][g]), tag
                    elif role == 'fixed_cell':
                        assert st['status'][g] == 0 and st['steps'][g] == c.state['steps'][g] + advance and moved == bool(advance), tag
                        assert same_cell and same_eps and st['pint'][g] == -2.0 and st['vol'][g] == -3.0 and st['ke'][g] > 0, tag
                    else:
                        assert st['status'][g] == 0 and st['steps'][g] == c.state['steps'][g] + advance, tag
                        assert moved == (bool(advance) and role != 'empty'), tag
                        assert same_cell == (not advance) and same_eps == (not advance), tag
                        assert np.isfinite(st['pint'][g]) and st['vol'][g] > 0, tag
                        assert (st['ke'][g] > 0) == (role not in ('all_fixed', 'empty')), tag
                        if advance:
                            drift = -c.rate[g] * (c.p0[g] - st['pint'][g]) * c.dt[g]
                            assert (st['eps'][g] == c.state['eps'][g] + drift) == (role == 'kt0'), tag   # (noise: there, or exactly absent)
                            if role == 'rate_big' and kick_in and mass:
                                assert 1.5 <= abs(drift) <= 6.0, tag
                            fx = c.fixed[s]
                            if fx.any():                                                    # fixed atoms follow the cell
                                assert not np.array_equal(pos[s][fx], c.pos[s][fx]) and np.array_equal(vel[s][fx], c.vel[s][fx]), tag
                    seen.add((role, SIZES[g]))
    assert {r for r, _ in seen} == set(ROLES) | {'empty'}
    for role in ('langevin', 'kt0', 'nve'):                       # each at more than one size
        assert len({m for r, m in seen if r == role}) >= 2
    assert any(r == 'some_fixed' and m >= 2 for r, m in seen)


def test_the_batched_reference_is_the_reference():
    """(No GPU.)  npt_batch_ref -- the rule for many graphs at once, which the ideal-gas statistics run -- against md_npt_step_ref
    with the generator's normals handed in: three steps of five graphs of four unit-mass atoms under forces, to 1e-12."""
    rng = np.random.RandomState(3)
    G, N = 5, 4
    pos, vel = rng.uniform(0, 2, (G, N, 3)).astype(np.float32), rng.standard_normal((G, N, 3)).astype(np.float32)
    cell0 = np.tile(2.0 * np.eye(3, dtype=np.float32), (G, 1, 1))
    seeds = rng.randint(-2 ** 63, 2 ** 63 - 1, G, dtype=np.int64)
    st = dict(seed=seeds, steps=np.zeros(G, np.int32), status=np.zeros(G, np.int32), ke=np.zeros(G), eps=np.zeros(G),
              pint=np.zeros(G), vol=np.zeros(G))
    p, v, cell, gptr = pos.reshape(-1, 3), vel.reshape(-1, 3), cell0.copy(), _gptr([N] * G)
    bp, bv, beps = pos.astype(np.float64), vel.astype(np.float64), np.zeros(G)
    for it in range(3):
        dE = rng.standard_normal((G, N, 3)).astype(np.float32)
        W = rng.standard_normal((G, 3, 3)).astype(np.float32)
        xi = np.stack([normals(s, N, it, 0) for s in seeds])
        xi_c = np.array([barostat_normal(s, it) for s in seeds])
        p, v, cell, st = md_npt_step_ref(p, v, dE.reshape(-1, 3), W, gptr, cell0, cell, st, 0.05, 0.8, 1.5, 0.3, 0.6, None, None, None,
                                         1 if it else 0, 1)
        trW = (W[:, 0, 0].astype(np.float64) + W[:, 1, 1]) + W[:, 2, 2]
        bp, bv, beps, ke, pint, vol = npt_batch_ref(bp, bv, -dE.astype(np.float64), trW, 8.0, beps, 0.05, 0.8, 1.5, 0.3, 0.6, xi, xi_c,
                                                     1 if it else 0, round32=True)
        assert np.allclose(st['ke'], ke, rtol=1e-12, atol=0) and np.allclose(st['pint'], pint, rtol=1e-12, atol=0)
        assert np.allclose(st['vol'], vol, rtol=1e-12, atol=0) and np.allclose(st['eps'], beps, rtol=1e-12, atol=1e-15)
        assert maxnorm_err(p, bp.reshape(-1, 3)) <= 1e-7 and maxnorm_err(v, bv.reshape(-1, 3)) <= 1e-7    # (one fp32 rounding apart at most)


def test_the_reference_relaxes_the_volume_to_the_target_pressure():
    """(No GPU.)  The precondition of the deterministic relaxation: the reference trajectory, 150 steps with rate B dt = 0.2 from
    volumes 10 % above, 8 % below and 5 % above V0, ends within the bound of _relaxation of V* = V0 (1 - P0 / B) in every graph,
    approaches it monotonically, and has moved by far more than the bound."""
    w = _relaxation()
    err = np.abs(w.vols[-1] / w.vstar - 1.0)
    print('relaxation reference: V*', w.vstar, 'final', w.vols[-1], 'relative error', err, 'bound', w.bound)
    assert (err <= w.bound).all() and (w.bound < 6e-7).all()
    assert (np.abs(w.vols[0] / w.vstar - 1.0) > 0.02).all()
    gap = np.abs(w.vols / w.vstar - 1.0)
    assert (gap[1:40] < gap[:39]).all()
    assert (w.state['status'] == 0).all() and (w.state['steps'] == R_STEPS).all()
    assert abs(abs(det3(w.cell[0])) / w.vstar[0] - 1.0) <= w.bound[0]


def test_the_reference_gas_has_the_gamma_law_within_the_tolerances():
    """(No GPU.)  The preconditions of the ideal-gas test: its total tolerance on the mean is below half of 1 / (N + 1) = 10 % (a
    rule with the Jacobian term wrong has the mean N or N + 2 times kT / P0 and fails), the tolerance on the variance below the
    20 % that separate (N + 1) from N and N + 2; successive samples of the reference are correlated by less than GAS_RHO; and the
    reference alone is within both tolerances."""
    n_eff, tol_mean, tol_var = _gas_tolerances()
    k = GAS['N'] + 1
    assert tol_mean < 0.5 / k and tol_var < 1.0 / k
    vols, kes = _gas_reference()
    assert vols.shape == (len(_gas_records()), GAS['G'])
    mean, var, rho = _gas_moments(vols)
    print('gas reference: n_eff', n_eff, 'mean error', mean, 'tolerance', tol_mean, 'variance error', var, 'tolerance', tol_var,
          'correlation of successive samples', rho)
    assert abs(rho) < GAS_RHO and abs(mean) <= tol_mean and abs(var) <= tol_var
    kin = kes.mean() / (1.5 * GAS['N'] * GAS['kT']) - 1.0          # (3 N degrees of freedom a graph: as spread as the volume)
    print('gas reference: kinetic energy error', kin)
    assert abs(kin) <= tol_mean


def test_run_npt_refusals_without_a_device():
    """(No GPU.)  What run() refuses is refused before anything runs, and CPU tensors are a RuntimeError (no CPU path)."""
    import models
    from pamnet_amd import synth
    from pamnet_amd.md import run_npt
    w = _relaxation()
    model = VolumeWell(torch.from_numpy(R_B), torch.from_numpy(w.V0))
    data = synth.Batch(pos=torch.from_numpy(w.pos0), batch=torch.from_numpy(w.batch), cell=torch.from_numpy(w.cell0), num_graphs=3)
    ok = dict(steps=2, dt=R_DT, kT=0.0, pressure=0.0, tau_p=1.0, compressibility=1.0)
    pdb = models.PAMNet(models.Config(dataset='PDBbind', dim=16, n_layer=1, cutoff_l=2.0, cutoff_g=6.0))
    with pytest.raises(ValueError, match=r'x\[:, :3\]'):
        run_npt(pdb, data, **ok)
    with pytest.raises(ValueError, match='no `pos`'):
        run_npt(model, synth.Batch(batch=data.batch, cell=data.cell, num_graphs=3), **ok)
    with pytest.raises(ValueError, match='no `batch`'):
        run_npt(model, synth.Batch(pos=data.pos, cell=data.cell, num_graphs=3), **ok)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        run_npt(model, data, **ok)
    assert torch.equal(data.pos, torch.from_numpy(w.pos0)) and torch.equal(data.cell, torch.from_numpy(w.cell0))


# ------------------------------------------------------------------------------------------------------- kernel tests
def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _step_on_device(dev, c, kick_in, advance, mass=True, graphs=None, scalars=None, dof='case', seed=True):
    """One launch on the graphs `graphs` (a slice) of a case -> (pos, vel, cell, state) as numpy.  scalars: (dt, kT, gamma,
    pressure, rate) floats in place of the per-graph arrays; dof: 'case' (the case's mask) or None (NULL); seed=False: NULL."""
    from pamnet_amd import md as M
    graphs = slice(0, len(c.gptr) - 1) if graphs is None else graphs
    lo, hi = int(c.gptr[graphs.start]), int(c.gptr[graphs.stop])
    pos, vel, dE = _t(dev, c.pos[lo:hi]), _t(dev, c.vel[lo:hi]), _t(dev, c.dE[lo:hi])
    W, cell0, cell = _t(dev, c.W[graphs]), _t(dev, c.cell0[graphs]), _t(dev, c.cell[graphs])
    state = {k: _t(dev, c.state[k][graphs]) for k in NPT_STATE}
    if not seed:
        state['seed'] = None
    per_graph = tuple(_t(dev, a[graphs]) for a in (c.dt, c.kT, c.gamma, c.p0, c.rate))
    dt, kT, gamma, p0, rate = scalars if scalars is not None else per_graph
    M.npt_step(pos, vel, dE, W, _t(dev, c.gptr[graphs.start:graphs.stop + 1] - lo), cell0, cell, state, dt, kT, p0, rate, gamma,
               _t(dev, c.mass[lo:hi]) if mass else None, _t(dev, c.fixed[lo:hi].astype(np.uint8)),
               _t(dev, c.dof[graphs].astype(np.uint8)) if dof == 'case' else None, kick_in, advance)
    return (pos.cpu().numpy(), vel.cpu().numpy(), cell.cpu().numpy(),
            {k: (None if v is None else v.cpu().numpy()) for k, v in state.items()})


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _close64(got, want, tag):
    """An fp64 output: 1e-12 relative where the reference is finite, the same class (NaN, +inf, -inf) elsewhere."""
    if np.isfinite(want):
        assert abs(got - want) <= 1e-12 * abs(want), (tag, got, want)
    else:
        assert np.isnan(got) == np.isnan(want) and (np.isnan(want) or got == want), (tag, got, want)


def _assert_npt_matches(got, want, before, gptr, fixed, dof, advance, tag='', must_move=True):
    """got / want / before: (pos, vel, cell, state); the checks of one launch against md_npt_step_ref.  must_move: an advancing
    launch displaces every graph that has atoms (False for a relaxation that comes to rest: there a displacement of zero is
    matched by zero alone)."""
    (gp, gv, gc, gs), (wp, wv, wc, ws), (bp, bv, bc, bs) = got, want, before
    for k in ('status', 'steps', 'seed'):
        assert np.array_equal(gs[k], ws[k]), (tag, k, gs[k], ws[k])
    worst = [0.0, 0.0, 0.0]
    for g in range(len(gptr) - 1):
        s = slice(int(gptr[g]), int(gptr[g + 1]))
        t = (tag, g)
        if bs['status'][g] != 0:                                   # left alone: bit for bit the input
            assert all(_same(gs[k][g], bs[k][g]) for k in NPT_STATE), t
            assert _same(gp[s], bp[s]) and _same(gv[s], bv[s]) and _same(gc[g], bc[g]), t
            continue
        _close64(gs['ke'][g], ws['ke'][g], t + ('ke',))
        if not dof[g]:                                             # no barostat: nothing of it is written
            assert _same(gc[g], bc[g]) and all(_same(gs[k][g], bs[k][g]) for k in ('eps', 'pint', 'vol')), t
        else:
            _close64(gs['pint'][g], ws['pint'][g], t + ('pint',))
            _close64(gs['vol'][g], ws['vol'][g], t + ('vol',))
        if ws['status'][g] != 0:                                   # failed in this launch: nothing else is written
            assert _same(gp[s], bp[s]) and _same(gv[s], bv[s]) and _same(gc[g], bc[g]) and _same(gs['eps'][g], bs['eps'][g]), t
            continue
        fx = fixed[s]
        assert _same(gv[s][fx], bv[s][fx]), t + ('fixed rows of vel',)
        if not advance:
            assert np.array_equal(gp[s], bp[s]) and _same(gc[g], bc[g]) and gs['eps'][g] == bs['eps'][g], t
        elif dof[g]:
            # eps to 1e-12 relative, and its change d to 1e-12 relative beside the one rounding of eps + d (2^-53 relative, in
            # the kernel and in the reference each), so that a large eps cannot hide an error in a small d
            e_got, e_want, e_old = gs['eps'][g], ws['eps'][g], bs['eps'][g]
            assert (e_want != e_old or not must_move) and abs(e_got - e_want) <= 1e-12 * abs(e_want), t + ('eps', e_got, e_want)
            assert abs(e_got - e_want) <= 1e-12 * abs(e_want - e_old) + 2.0 ** -52 * max(abs(e_want), abs(e_old)), t + ('d', e_got, e_want)
            ec = maxnorm_err(gc[g].astype(np.float64) - bc[g], wc[g].astype(np.float64) - bc[g])
            worst[2] = max(worst[2], ec)
            assert ec <= KTOL, t + ('cell', ec)
        else:
            assert np.array_equal(gp[s][fx], bp[s][fx]), t + ('fixed rows of pos',)
        moving = np.ones(s.stop - s.start, dtype=bool) if dof[g] else ~fx      # the rows of pos an advancing launch writes
        if advance and moving.any():
            want_d = wp[s][moving].astype(np.float64) - bp[s][moving]
            assert not must_move or float(np.abs(want_d).max()) > 0, t
            ed = maxnorm_err(gp[s][moving].astype(np.float64) - bp[s][moving], want_d)
            worst[1] = max(worst[1], ed)
            assert ed <= KTOL, t + ('displacement', ed)
        if (~fx).any():
            ev = maxnorm_err(gv[s][~fx], wv[s][~fx])
            worst[0] = max(worst[0], ev)
            assert ev <= KTOL, t + ('vel', ev)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize('shift', SHIFTS)
def test_one_npt_step_on_a_batch_vs_the_reference(dev, shift):
    """Graphs of 1 .. 1025 and 0 atoms in the roles of _kernel_case (triclinic cell0, a starting eps that is not 0), per-graph dt /
    kT / gamma / pressure / rate, under every (kick_in, advance), with masses and with NULL: steps and status equal; ke, pint, vol,
    eps and its change to 1e-12; vel, the displacement and the change of the cell within KTOL per graph; what must stay
    unwritten bit for bit the input.  Then every running graph once more with ITS five values as the scalars of the launch:
    bitwise what the per-graph arrays gave it.  And the graph without a barostat: torch.equal to what pamnet_md_step_f32 writes
    from the same inputs, under every pair of flags."""
    from pamnet_amd import md as M
    c = _kernel_case(shift)
    before = (c.pos, c.vel, c.cell, c.state)
    worst = [0.0, 0.0, 0.0]
    for kick_in, advance in FLAGS:
        for mass in (True, False):
            got = _step_on_device(dev, c, kick_in, advance, mass)
            w = _assert_npt_matches(got, _ref(c, kick_in, advance, mass), before, c.gptr, c.fixed, c.dof, advance,
                                    tag=(shift, kick_in, advance, mass))
            worst = [max(a, b) for a, b in zip(worst, w)]
    print('shift', shift, 'worst vel / displacement / cell error', worst)
    arrays = _step_on_device(dev, c, 1, 1)
    for g, role in enumerate(c.roles):
        if role in BARO_FAILS + ('failed', 'fixed_cell'):
            continue
        s = slice(int(c.gptr[g]), int(c.gptr[g + 1]))
        p, v, cell, st = _step_on_device(dev, c, 1, 1, scalars=tuple(float(a[g]) for a in (c.dt, c.kT, c.gamma, c.p0, c.rate)))
        assert np.array_equal(p[s], arrays[0][s]) and np.array_equal(v[s], arrays[1][s]) and np.array_equal(cell[g], arrays[2][g]), (role, g)
        assert all(st[k][g] == arrays[3][k][g] for k in ('ke', 'eps', 'pint', 'vol')) and st['steps'][g] == c.state['steps'][g] + 1
    g = c.roles.index('fixed_cell')                                # (every shift has one: at 255, 2 and 1025 atoms)
    gs = slice(g, g + 1)
    lo, hi = int(c.gptr[g]), int(c.gptr[g + 1])
    for kick_in, advance in FLAGS:
        npt = _step_on_device(dev, c, kick_in, advance)
        pos, vel, dE = _t(dev, c.pos[lo:hi]), _t(dev, c.vel[lo:hi]), _t(dev, c.dE[lo:hi])
        state = {k: _t(dev, c.state[k][gs]) for k in STATE}
        M.md_step(pos, vel, dE, _t(dev, c.gptr[g:g + 2] - lo), state, _t(dev, c.dt[gs]), _t(dev, c.kT[gs]), _t(dev, c.gamma[gs]),
                  _t(dev, c.mass[lo:hi]), _t(dev, c.fixed[lo:hi].astype(np.uint8)), kick_in, advance)
        assert torch.equal(pos, _t(dev, npt[0][lo:hi])) and torch.equal(vel, _t(dev, npt[1][lo:hi])), (kick_in, advance)
        assert all(torch.equal(state[k], _t(dev, npt[3][k][gs])) for k in STATE), (kick_in, advance)


@pytest.mark.gpu
def test_an_npt_step_is_repeatable_and_independent_of_the_batch(dev):
    """Thermostat and barostat noise on.  Every graph of _indep_graphs stepped alone, inside the batch in each of three rotations
    of its order, and twice over: its rows of pos and vel, its cell, eps, ke, pint, vol and steps are equal bit for bit in all of
    them.  Four copies of one graph that differ in (seed, step) only: the same pair gives the same eps bit for bit, another seed
    or another step a different one, while pint and vol (which no noise enters) stay."""
    graphs = _indep_graphs()
    alone = []
    for g in graphs:
        p, v, cell, st = _step_on_device(dev, _assemble([g]), 1, 1, dof=None)
        alone.append((p, v, cell[0], [st[k][0] for k in ('eps', 'ke', 'pint', 'vol', 'steps')]))
        assert st['steps'][0] == g['steps'] + 1 and st['eps'][0] != g['eps']
    for rot in (0, 4, 7, 0):
        order = list(range(rot, len(graphs))) + list(range(rot))
        c = _assemble([graphs[i] for i in order])
        p, v, cell, st = _step_on_device(dev, c, 1, 1)
        for j, i in enumerate(order):
            s = slice(int(c.gptr[j]), int(c.gptr[j + 1]))
            assert np.array_equal(p[s], alone[i][0]) and np.array_equal(v[s], alone[i][1]) and np.array_equal(cell[j], alone[i][2]), (rot, i)
            assert [st[k][j] for k in ('eps', 'ke', 'pint', 'vol', 'steps')] == alone[i][3], (rot, i)
    one = graphs[4]                                                 # 65 atoms
    c = _assemble([dict(one, seed=s, steps=k) for s, k in ((5, 3), (6, 3), (5, 4), (5, 3))])
    p, v, cell, st = _step_on_device(dev, c, 1, 1)
    e = st['eps']
    assert e[0] == e[3] and np.array_equal(cell[0], cell[3]) and np.array_equal(p[:65], p[3 * 65:])
    assert len({e[0], e[1], e[2]}) == 3
    assert len(set(st['pint'])) == 1 and len(set(st['vol'])) == 1 and len(set(st['ke'])) == 1
    for j, (seed, step) in enumerate(((5, 3), (6, 3), (5, 4))):    # and it is the reference's normal that makes the difference
        noise = np.sqrt(2.0 * one['kT'] * one['rate'] * one['dt'] / st['vol'][j]) * barostat_normal(seed, step)
        drift = -one['rate'] * (one['p0'] - st['pint'][j]) * one['dt']
        assert abs((e[j] - one['eps']) - (drift + noise)) <= 1e-12 * abs(drift + noise)


@pytest.mark.gpu
def test_the_npt_entry_point_validates_its_arguments(dev):
    """A null required pointer is PAMNET_ENULL; a negative count, a flag other than 0 / 1 and a bad scalar where its per-graph array
    is NULL are PAMNET_EINVAL; mass, fixed, cell_dof and the per-graph arrays may be NULL, the seed only where neither noise can
    occur; a per-graph array replaces its scalar; n_graphs == 0 launches nothing."""
    from pamnet_amd import lib
    c = _kernel_case(0)
    G, n = len(SIZES), len(c.pos)
    pos, vel, dE, gptr, mass = _t(dev, c.pos), _t(dev, c.vel), _t(dev, c.dE), _t(dev, c.gptr), _t(dev, c.mass)
    W, cell0, cell = _t(dev, c.W), _t(dev, c.cell0), _t(dev, c.cell)
    st = {k: _t(dev, c.state[k]) for k in NPT_STATE}
    dt_g, zeros, ones = _t(dev, c.dt), _t(dev, np.zeros(G)), _t(dev, np.ones(G))
    nan, inf = float('nan'), float('inf')

    def step(**kw):
        a = dict(pos=lib.ptr(pos), vel=lib.ptr(vel), dpos=lib.ptr(dE), dstrain=lib.ptr(W), mass=None, fixed=None, gptr=lib.ptr(gptr),
                 n=n, G=G, cell0=lib.ptr(cell0), cell=lib.ptr(cell), cell_dof=None, dt_g=None, kT_g=None, gamma_g=None, p_g=None,
                 rate_g=None, dt=0.05, kT=0.5, gamma=1.0, p=0.1, rate=0.01, kick_in=1, advance=1)
        a.update({k: lib.ptr(st[k]) for k in NPT_STATE})
        a.update(kw)
        lib.call(ENTRY, a['pos'], a['vel'], a['dpos'], a['dstrain'], a['mass'], a['fixed'], a['gptr'], a['n'], a['G'], a['cell0'],
                 a['cell'], a['eps'], a['cell_dof'], a['seed'], a['steps'], a['status'], a['ke'], a['pint'], a['vol'], a['dt_g'],
                 a['kT_g'], a['gamma_g'], a['p_g'], a['rate_g'], a['dt'], a['kT'], a['gamma'], a['p'], a['rate'], a['kick_in'],
                 a['advance'], lib.stream_of(pos))

    for k in ('pos', 'vel', 'dpos', 'dstrain', 'gptr', 'cell0', 'cell', 'eps', 'seed', 'steps', 'status', 'ke', 'pint', 'vol'):
        with pytest.raises(RuntimeError, match='PAMNET_ENULL'):
            step(**{k: None})
    for kw in (dict(gamma=0.0), dict(kT=0.0), dict(gamma=0.0, kT=0.0, gamma_g=lib.ptr(zeros)),
               dict(gamma=0.0, kT=0.0, kT_g=lib.ptr(zeros))):       # (a per-graph array may hold anything: the seed is needed)
        with pytest.raises(RuntimeError, match='PAMNET_ENULL'):
            step(seed=None, **kw)
    for kw in (dict(n=-1), dict(G=-1), dict(G=2 ** 31), dict(kick_in=2), dict(kick_in=-1), dict(advance=2), dict(dt=0.0),
               dict(dt=-0.1), dict(dt=nan), dict(dt=inf), dict(kT=-1.0), dict(kT=nan), dict(kT=inf), dict(gamma=-1.0),
               dict(gamma=nan), dict(gamma=inf), dict(p=nan), dict(p=inf), dict(p=-inf), dict(rate=0.0), dict(rate=-1.0),
               dict(rate=nan), dict(rate=inf)):
        with pytest.raises(RuntimeError, match='PAMNET_EINVAL'):
            step(**kw)
    step(G=0)
    torch.cuda.synchronize()
    clean = lambda t: t.nan_to_num(1.0, 2.0, 3.0)
    same = lambda: (torch.equal(pos, _t(dev, c.pos)) and torch.equal(clean(vel), clean(_t(dev, c.vel)))
                    and torch.equal(clean(cell), clean(_t(dev, c.cell)))
                    and all(torch.equal(clean(st[k].double()), clean(_t(dev, c.state[k]).double())) for k in NPT_STATE))
    assert same()
    # a per-graph array replaces its scalar, which is then not looked at; every graph already failed: nothing is touched
    st['status'].fill_(2)
    step(dt_g=lib.ptr(dt_g), dt=nan, kT_g=lib.ptr(zeros), kT=-1.0, gamma_g=lib.ptr(zeros), gamma=inf, p_g=lib.ptr(zeros), p=nan,
         rate_g=lib.ptr(ones), rate=-1.0, mass=lib.ptr(mass), cell_dof=lib.ptr(_t(dev, c.dof.astype(np.uint8))))
    step(seed=None, gamma=0.0, kT=0.0)
    torch.cuda.synchronize()
    st['status'].copy_(_t(dev, c.state['status']))
    assert same()


# ----------------------------------------------------------------------------------------------------- end to end
def _cpu(t):
    return None if t is None else t.cpu().numpy()


def _replay(res, gptr, cell0, dt, kT, gamma, p0, rate, mass, fixed, dof, steps, must_move=True):
    """Every launch of a trace through md_npt_step_ref from its recorded inputs; consecutive launches hand on what they stored."""
    worst = [0.0, 0.0, 0.0]
    assert len(res.trace) == steps + 1
    fx = np.zeros(len(_cpu(res.pos)), bool) if fixed is None else fixed
    dof = np.ones(len(gptr) - 1, dtype=bool) if dof is None else dof
    same = lambda a, b: torch.equal(a.nan_to_num(-7.0), b.nan_to_num(-7.0))   # (pint of a graph without a barostat stays NaN)
    for i, r in enumerate(res.trace):
        assert (r['kick_in'], r['advance']) == (1 if i else 0, 1 if i < steps else 0)
        before = (_cpu(r['pos']), _cpu(r['v_before']), _cpu(r['cell']), {k: _cpu(v) for k, v in r['state_before'].items()})
        got = (_cpu(r['pos_after']), _cpu(r['v_after']), _cpu(r['cell_after']), {k: _cpu(v) for k, v in r['state_after'].items()})
        want = md_npt_step_ref(before[0], before[1], _cpu(r['dE']), _cpu(r['W']), gptr, cell0, before[2], before[3], dt, kT, gamma, p0,
                               rate, mass, fixed, dof, r['kick_in'], r['advance'])
        w = _assert_npt_matches(got, want, before, gptr, fx, dof, r['advance'], tag=i, must_move=must_move)
        worst = [max(a, b) for a, b in zip(worst, w)]
        if i + 1 < len(res.trace):
            nxt = res.trace[i + 1]
            assert torch.equal(r['pos_after'], nxt['pos']) and torch.equal(r['v_after'], nxt['v_before'])
            assert torch.equal(r['cell_after'], nxt['cell'])
    last = res.trace[-1]
    assert torch.equal(last['pos_after'], res.pos) and torch.equal(last['v_after'], res.vel) and torch.equal(last['cell_after'], res.cell)
    assert torch.equal(last['state_after']['ke'], res.kinetic) and same(last['state_after']['pint'], res.pressure)
    assert torch.equal(last['state_after']['vol'], res.volume) and torch.equal(last['state_after']['eps'], res.eps)
    return worst


def _well_on_device(w, dev):
    from pamnet_amd import synth
    model = VolumeWell(torch.from_numpy(R_B), torch.from_numpy(w.V0)).to(dev)
    data = synth.Batch(pos=torch.from_numpy(w.pos0), batch=torch.from_numpy(w.batch), cell=torch.from_numpy(w.cell0),
                       num_graphs=len(R_B)).to(dev)
    return model, data


@pytest.mark.gpu
def test_the_volume_relaxes_to_the_target_pressure_without_a_synchronisation(dev):
    """kT = 0, at rest, the three wells of _relaxation (B = 2 / 10 / 0.5, P0 = 0.3 / -1 / 0.02, triclinic and cubic cells that start
    10 % above, 8 % below and 5 % above V0, one atom fixed), per-graph pressure and tau_p, 150 steps: res.volume and |det res.cell|
    are within the bound of _relaxation -- the contraction's residual (below 1e-12) plus 8 x 2^-24 for the fp32 cell -- of
    V* = V0 (1 - P0 / B); the CPU test asserts the same of the reference.  Every launch of the trace replays through the reference;
    the atoms, fixed one included, keep their fractional coordinates; res.pressure is the target.  Under torch's synchronisation
    debug mode the run synchronises once -- the set-up read of the per-graph values -- and with floats not at all."""
    from pamnet_amd.md import run_npt
    w = _relaxation()
    model, data = _well_on_device(w, dev)
    fixed = _t(dev, w.fixed)
    p0, tau = _t(dev, R_P0), _t(dev, 1.0 / w.rate)
    zeros = torch.zeros(len(w.pos0), 3, device=dev)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        torch.cuda.set_sync_debug_mode('warn')
        try:
            res = run_npt(model, data, R_STEPS, R_DT, 0.0, p0, tau, 1.0, fixed=fixed, velocities=zeros, record_every=1,
                          check_every=0, trace=True)
        finally:
            torch.cuda.set_sync_debug_mode('default')
    syncs = [str(m.message) for m in caught if 'called a synchronizing' in str(m.message)]
    print('synchronisations of a 150-step run:', syncs)
    assert len(syncs) == 1
    torch.cuda.set_sync_debug_mode('error')
    try:
        res7 = run_npt(model, data, 7, R_DT, 0.0, 0.1, 2.0, 0.5, velocities=zeros, record_every=3, check_every=0)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert res7.steps.tolist() == [7] * 3 and tuple(res7.cells.shape) == (3, 3, 3, 3) and res7.trace is None
    assert torch.equal(data.pos.cpu(), torch.from_numpy(w.pos0)) and torch.equal(data.cell.cpu(), torch.from_numpy(w.cell0))
    assert res.steps.tolist() == [R_STEPS] * 3 and not res.failed.any()
    worst = _replay(res, w.gptr, w.cell0, R_DT, 0.0, 0.0, R_P0, w.rate, None, w.fixed, None, R_STEPS, must_move=False)
    vol, cell = res.volume.cpu().numpy(), res.cell.cpu().numpy()
    err = np.abs(vol / w.vstar - 1.0)
    err_cell = np.abs(np.array([abs(det3(c)) for c in cell]) / w.vstar - 1.0)
    print('relaxation: V*', w.vstar, 'volume', vol, 'relative error', err, 'of |det cell|', err_cell, 'bound', w.bound, 'replay', worst)
    assert (err <= w.bound).all() and (err_cell <= w.bound).all()
    assert np.abs(res.pressure.cpu().numpy() - R_P0).max() <= 1e-6 * np.abs(R_B).max()
    assert tuple(res.volumes.shape) == tuple(res.pressures.shape) == (R_STEPS + 1, 3) and tuple(res.cells.shape) == (R_STEPS + 1, 3, 3, 3)
    assert torch.equal(res.volumes[-1], res.volume) and torch.equal(res.cells[-1], res.cell) and torch.equal(res.frames[-1], res.pos)
    assert torch.equal(res.cells[0].cpu(), torch.from_numpy(w.cell0)) and maxnorm_err(res.volumes.cpu().numpy(), w.vols) <= 1e-6
    frac0 = np.concatenate([w.pos0[w.batch == g].astype(np.float64) @ np.linalg.inv(w.cell0[g].astype(np.float64)) for g in range(3)])
    frac = np.concatenate([res.pos.cpu().numpy()[w.batch == g].astype(np.float64) @ np.linalg.inv(cell[g].astype(np.float64)) for g in range(3)])
    assert np.abs(frac - frac0).max() <= 2e-5 and not res.vel.any()      # (150 fp32 roundings of a coordinate: 150 x 2^-24 = 9e-6)


@pytest.mark.gpu
def test_an_ideal_gas_has_the_gamma_law_of_its_volume(dev):
    """256 graphs of 4 free unit-mass atoms without forces or virial, Langevin thermostat (gamma = 2), kT = P0 = 1, dt = 0.05,
    rate = 0.4, seeds 0 .. 255, remove_com=False, 2100 steps, the volume recorded every 120 steps after a burn-in of 300: the pooled
    volumes have the mean (N + 1) kT / P0 and the variance (N + 1) (kT / P0)^2 of the Gamma(N + 1) law, within the tolerances of
    _gas_tolerances -- four standard errors of the decorrelated samples plus the measured first-order bias: 4.0 % on the mean (under
    half of 1 / (N + 1): a rule with the Jacobian term wrong fails) and 15.1 % on the variance.  The CPU test asserts the same of
    the reference."""
    from pamnet_amd import synth
    from pamnet_amd.md import run_npt
    G, N = GAS['G'], GAS['N']
    rng = np.random.RandomState(8)
    side = ((N + 1) * GAS['kT'] / GAS['p0']) ** (1.0 / 3.0)
    data = synth.Batch(pos=torch.from_numpy(rng.uniform(0, side, (G * N, 3)).astype(np.float32)),
                       batch=torch.arange(G).repeat_interleave(N), num_graphs=G,
                       cell=(side * torch.eye(3)).repeat(G, 1, 1).contiguous()).to(dev)
    res = run_npt(IdealGas(), data, GAS['steps'], GAS['dt'], GAS['kT'], GAS['p0'], 1.0, GAS['rate'], gamma=GAS['gamma'], seed=0,
                  remove_com=False, record_every=GAS['stride'])
    assert res.steps.tolist() == [GAS['steps']] * G and not res.failed.any()
    vols = res.volumes[_gas_records()].cpu().numpy()
    _, tol_mean, tol_var = _gas_tolerances()
    mean, var, rho = _gas_moments(vols)
    kin = float(res.ekin[_gas_records()].mean()) / (1.5 * N * GAS['kT']) - 1.0
    print('ideal gas: mean error', mean, 'tolerance', tol_mean, 'variance error', var, 'tolerance', tol_var, 'correlation', rho,
          'kinetic energy error', kin)
    assert vols.shape == (len(_gas_records()), G) and abs(rho) < GAS_RHO
    assert abs(mean) <= tol_mean and abs(var) <= tol_var
    assert abs(kin) <= tol_mean                                     # (the thermostat holds kT beside the barostat: 12 degrees of freedom a graph)


P_STEPS, P_SCALE = 6, 1.15


def _pamnet_batch():
    """[24 atoms in the triclinic cell 1.15 TRI_A, 20 atoms in 1.15 TRI_B with one atom fixed, the slab slab_min of
    tests/test_pbc_axes.py with pbc = (True, True, False)] and the mask: that atom and the slab's bottom layer.  The bulk heights
    are 1.15 x 11.3 = 13 A and more, against the 10 A the minimum-image build needs."""
    if 'pamnet' in _MADE:
        return _MADE['pamnet']
    from test_pbc_axes import TRI_A, TRI_B, Struct, _batch, _scatter, _structs
    rng = np.random.RandomState(6)
    full = (True, True, True)
    ca, cb = P_SCALE * np.asarray(TRI_A), P_SCALE * np.asarray(TRI_B)
    a = Struct(rng.randint(0, 5, 24).astype(np.float32), _scatter(rng, 24, ca, full, {}, 2).astype(np.float32), ca, full, 2)
    b = Struct(rng.randint(0, 5, 20).astype(np.float32), _scatter(rng, 20, cb, full, {}, 2).astype(np.float32), cb, full, 2)
    slab = _structs()['slab_min']
    structs = [a, b, slab]
    bt = _batch(structs)
    z = slab.pos[:, 2]
    fixed = np.zeros(bt.pos.size(0), dtype=bool)
    fixed[a.n + 3] = True
    fixed[-slab.n:] = z <= np.sort(z)[slab.n // 3 - 1]
    mass = rng.uniform(1.0, 20.0, bt.pos.size(0)).astype(np.float32)
    _MADE['pamnet'] = (bt, torch.from_numpy(fixed), torch.from_numpy(mass), structs)
    return _MADE['pamnet']


@pytest.mark.gpu
@pytest.mark.parametrize('dim,n_layer', MODELS)
def test_pamnet_npt_replayed_step_by_step(dev, dim, n_layer):
    """PAMNet on {triclinic bulk cell, a second bulk cell with a fixed atom, slab with a fixed bottom layer and an open axis},
    per-graph pressure and tau_p, Langevin with per-graph seeds, 6 steps, trace=True: every launch replayed through
    md_npt_step_ref from its recorded inputs matches as in the kernel test; the slab has no barostat (its cell_dof comes from pbc)
    and keeps its cell and its fixed layer; the bulk cells change; res.pressure, res.volume, res.cell, res.virial and the recorded
    frames belong together; res.energy / res.forces / res.virial are bitwise a fresh evaluation at res.pos and res.cell; every
    recorded cell keeps its heights above the build's bound; the caller's batch and every parameter .grad are as they were."""
    import models
    from pamnet_amd.md import run_npt
    from test_pbc_axes import CUT_G, CUT_L, _axis_heights
    b, fixed_cpu, mass_cpu, structs = _pamnet_batch()
    G = len(structs)
    torch.manual_seed(0)
    model = models.PAMNet(models.Config(dataset='QM9', dim=dim, n_layer=n_layer, cutoff_l=CUT_L, cutoff_g=CUT_G)).to(dev)
    data, fixed, mass = b.to(dev), fixed_cpu.to(dev), mass_cpu.to(dev)
    model(data).sum().backward()                                   # parameter gradients to find untouched afterwards
    snap = [None if p.grad is None else p.grad.clone() for p in model.parameters()]
    pos0, cell0 = data.pos.clone(), data.cell.clone()
    seeds = torch.tensor([11, -5, 2 ** 40 + 3], dtype=torch.int64, device=dev)
    p0, tau, beta = np.array([0.01, -0.02, 0.0]), np.array([5.0, 2.5, 1.0]), 20.0
    res = run_npt(model, data, P_STEPS, 0.05, 0.05, _t(dev, p0), _t(dev, tau), beta, masses=mass, gamma=1.0, seed=seeds, fixed=fixed,
                  record_every=2, trace=True)
    assert torch.equal(data.pos, pos0) and torch.equal(data.cell, cell0) and not data.pos.requires_grad
    assert getattr(data, 'strain', None) is None
    for p, s in zip(model.parameters(), snap):
        assert (p.grad is None) if s is None else torch.equal(p.grad, s)
    assert res.steps.tolist() == [P_STEPS] * G and not res.failed.any()
    dof = np.array([all(st.pbc) for st in structs])
    assert dof.tolist() == [True, True, False]
    gptr = np.concatenate([[0], np.cumsum([st.n for st in structs])])
    worst = _replay(res, gptr, b.cell.numpy(), 0.05, 0.05, 1.0, p0, beta / tau, mass_cpu.numpy(), fixed_cpu.numpy(), dof, P_STEPS)
    print('replay: worst vel / displacement / cell error', worst)
    slab = slice(int(gptr[2]), int(gptr[3]))
    assert torch.equal(res.cell[2], cell0[2]) and float(res.eps[2]) == 0.0 and torch.isnan(res.pressure[2])
    assert torch.equal(res.pos[slab][fixed[slab]], pos0[slab][fixed[slab]])
    assert all(not torch.equal(res.cell[g], cell0[g]) for g in (0, 1))
    held = int(gptr[1]) + 3                                         # the fixed atom of the second cell follows its cell
    assert not torch.equal(res.pos[held], pos0[held]) and not res.vel[held].any()
    frac = lambda p, c: p.double() @ torch.linalg.inv(c.double())
    assert float((frac(res.pos[held], res.cell[1]) - frac(pos0[held], cell0[1])).abs().max()) <= 2e-6
    # what the result holds belongs together
    vol, cell = res.volume.cpu().numpy(), res.cell.cpu().numpy()
    for g in (0, 1):
        assert abs(abs(det3(cell[g])) / vol[g] - 1.0) <= 8 * EPS32
        want = (2.0 * float(res.kinetic[g]) - float(torch.diagonal(res.virial[g]).double().sum())) / (3.0 * vol[g])
        assert abs(float(res.pressure[g]) - want) <= 1e-12 * abs(want)
        assert abs(np.exp(float(res.eps[g])) * abs(det3(b.cell[g].numpy())) / vol[g] - 1.0) <= 1e-12
    assert maxnorm_err(res.stress[:2].cpu().numpy(), res.virial[:2].cpu().numpy() / vol[:2, None, None]) <= 1e-6
    F = P_STEPS // 2 + 1
    assert tuple(res.cells.shape) == (F, G, 3, 3) and tuple(res.volumes.shape) == tuple(res.pressures.shape) == (F, G)
    for i in range(F):
        r = res.trace[2 * i]
        assert torch.equal(res.frames[i], r['pos']) and torch.equal(res.cells[i], r['cell'])
        assert torch.equal(res.volumes[i], r['state_after']['vol']) and torch.equal(res.ekin[i], r['state_after']['ke'])
        assert torch.equal(res.pressures[i][:2], r['state_after']['pint'][:2])
    assert torch.equal(res.cells[-1], res.cell) and torch.equal(res.frames[-1], res.pos) and torch.equal(res.volumes[-1], res.volume)
    limit = 2 * max(CUT_L, CUT_G)
    for r in res.trace:
        for g in (0, 1):
            assert min(_axis_heights(r['cell_after'][g].cpu().numpy(), structs[g].pbc)) > 1.02 * limit
    d = copy.copy(data)
    d.pos, d.cell = res.pos.clone().requires_grad_(True), res.cell.clone()
    d.strain = torch.zeros(G, 3, 3, device=dev, requires_grad=True)
    e = model(d)
    de, w = torch.autograd.grad(e.sum(), [d.pos, d.strain])
    assert torch.equal(res.energy, e.detach()) and torch.equal(res.forces, -de) and torch.equal(res.virial, w)
    assert torch.isfinite(res.forces).all() and torch.isfinite(res.virial).all() and float(res.virial[0].abs().max()) > 0


@pytest.mark.gpu
def test_a_periodic_store_batch_runs_at_constant_pressure(dev):
    """A periodic MoleculeStore batch (cells of 10.5 A and more, minimum images: heights above 10) through run_npt, five steps under
    a tension (P0 = -5, far below any P_int of the model, asserted) with rate dt = 5e-4: every cell grows, by 0.25 % in volume a
    step, so the heights stay above the limit.  The model's deferred checks are clean and none is pending, res.energy /
    res.forces / res.virial are bitwise a plain-tensor evaluation at res.pos and res.cell, and the caller's batch keeps its cells."""
    from pamnet_amd import store as S
    from pamnet_amd.md import run_npt
    from test_store_pbc import ORDER, _items, _model, _plain
    items, steps = _items(), 5
    model = _model(dev)
    st = S.MoleculeStore(items, dev).prepare_for(model)
    bt = st.collate(ORDER)
    assert bt.mol_local[S.size_key(model, False)] is True and bt.cell is not None
    cell0 = bt.cell.clone()
    res = run_npt(model, bt, steps, 0.05, 0.0, -5.0, 100.0, 1.0, record_every=1)
    assert res.steps.tolist() == [steps] * len(ORDER) and torch.isfinite(res.energy).all() and torch.equal(bt.cell, cell0)
    assert not res.failed.any() and float(res.pressures.abs().max()) < 1.0
    growth = (res.volumes[1:] / res.volumes[:-1]).cpu().numpy()
    assert (growth > 1.002).all() and (growth < 1.003).all()
    model.verify()                                                 # nothing was flagged on the way ...
    assert not model._pending_checks                               # ... and nothing waits
    plain = _plain(items, ORDER, dev)
    assert torch.equal(plain.pos, bt.pos)
    plain.pos, plain.cell = res.pos.clone().requires_grad_(True), res.cell.clone()
    plain.strain = torch.zeros(len(ORDER), 3, 3, device=dev, requires_grad=True)
    e = model(plain)
    de, w = torch.autograd.grad(e.sum(), [plain.pos, plain.strain])
    assert torch.equal(res.energy, e.detach()) and torch.equal(res.forces, -de) and torch.equal(res.virial, w)


@pytest.mark.gpu
def test_run_npt_refusals(dev):
    """A batch without `cell`, kT = None, wrong shapes, dtypes and devices, values out of range (floats at once, tensors by the one
    read at set-up) and cell_dof set on a graph with an open axis are refused before anything moves."""
    from pamnet_amd.md import run_npt
    w = _relaxation()
    model, data = _well_on_device(w, dev)
    G = 3
    ok = dict(steps=2, dt=R_DT, kT=0.0, pressure=0.0, tau_p=1.0, compressibility=1.0)
    bare = copy.copy(data)
    bare.cell = None
    with pytest.raises(ValueError, match='no `cell`'):
        run_npt(model, bare, **ok)
    for cell in (data.cell[:2], data.cell.double(), data.cell.cpu(), data.cell.reshape(G, 9)):
        d = copy.copy(data)
        d.cell = cell
        with pytest.raises(ValueError, match='`data.cell` is a float32 tensor'):
            run_npt(model, d, **ok)
    f64 = lambda *v: torch.tensor(v, dtype=torch.float64, device=dev)
    nan, inf = float('nan'), float('inf')
    cases = [(dict(kT=None), 'needs its temperature'), (dict(kT=-1.0), '`kT` must be non-negative'),
             (dict(kT=f64(0.1, -1.0, 0.1)), '`kT` must be finite'),
             (dict(pressure=inf), '`pressure` must be finite'), (dict(pressure=nan), '`pressure` must be finite'),
             (dict(pressure=f64(0.0, nan, 0.0)), '`pressure` must be finite'), (dict(pressure=f64(0.0, -inf, 0.0)), '`pressure` must be'),
             (dict(pressure=f64(0.0, 0.0).float()), 'per-graph `pressure`'), (dict(pressure=f64(0.0, 0.0, 0.0).cpu()), 'per-graph `pressure`'),
             (dict(pressure=[0.0] * 3), '`pressure` is a float'),
             (dict(tau_p=0.0), '`tau_p` must be positive'), (dict(tau_p=-1.0), '`tau_p` must be positive'),
             (dict(tau_p=inf), '`tau_p` must be positive'), (dict(tau_p=f64(1.0, 0.0, 1.0)), '`tau_p` must be finite'),
             (dict(tau_p=f64(1.0, 1.0)), 'per-graph `tau_p`'),
             (dict(compressibility=0.0), '`compressibility` must be positive'), (dict(compressibility=nan), '`compressibility` must be'),
             (dict(compressibility=f64(1.0, inf, 1.0)), '`compressibility` must be finite'),
             (dict(compressibility=f64(1.0, 1.0, 1.0).float()), 'per-graph `compressibility`'),
             (dict(tau_p=1e-200, compressibility=1e200), '`compressibility` / `tau_p`'),
             (dict(dt=0.0), '`dt` must be positive'), (dict(gamma=-1.0), '`gamma` must be non-negative'),
             (dict(steps=-1), 'non-negative'), (dict(masses=torch.ones(5, device=dev)), '`masses` is a float32'),
             (dict(masses=torch.zeros(len(w.pos0), device=dev)), '`masses` must be finite'),
             (dict(fixed=torch.zeros(len(w.pos0), device=dev)), '`fixed` is a torch.bool'),
             (dict(velocities=torch.zeros(5, 3, device=dev)), '`velocities` is a float32'),
             (dict(seed=torch.zeros(2, dtype=torch.int64, device=dev)), 'per-graph `seed`'),
             (dict(cell_dof=[True] * 3), '`cell_dof` is a torch.bool tensor'),
             (dict(cell_dof=torch.ones(3, device=dev)), '`cell_dof` is a torch.bool tensor'),
             (dict(cell_dof=torch.ones(2, dtype=torch.bool, device=dev)), '`cell_dof` is a torch.bool tensor')]
    for kw, match in cases:
        with pytest.raises(ValueError, match=match):
            run_npt(model, data, **dict(ok, **kw))
    slab = copy.copy(data)
    slab.pbc = torch.tensor([[True] * 3, [True, True, False], [True] * 3], device=dev)
    yes = torch.ones(G, dtype=torch.bool, device=dev)
    with pytest.raises(ValueError, match='open axis'):
        run_npt(model, slab, cell_dof=yes, **ok)
    slab.pbc = (True, False, True)
    with pytest.raises(ValueError, match='open axis'):
        run_npt(model, slab, cell_dof=yes, **ok)
    # accepted: the default leaves the graph with the open axis without a barostat, and a given mask may switch one off
    slab.pbc = torch.tensor([[True] * 3, [True, True, False], [True] * 3], device=dev)
    res = run_npt(model, slab, **dict(ok, pressure=f64(0.1, 0.1, 0.1), tau_p=f64(1.0, 2.0, 3.0)))
    assert torch.equal(res.cell[1], data.cell[1]) and not torch.equal(res.cell[0], data.cell[0]) and res.steps.tolist() == [2] * 3
    res = run_npt(model, data, cell_dof=torch.tensor([False, True, True], device=dev), **dict(ok, pressure=0.1))
    assert torch.equal(res.cell[0], data.cell[0]) and not torch.equal(res.cell[1], data.cell[1])
    res = run_npt(model, data, **dict(ok, steps=0, record_every=4))
    assert res.steps.tolist() == [0] * 3 and torch.equal(res.pos, data.pos) and torch.equal(res.cell, data.cell)
    assert tuple(res.cells.shape) == (1, 3, 3, 3) and torch.equal(res.volumes[0], res.volume) and torch.equal(res.pressures[0], res.pressure)
    assert torch.equal(data.pos.cpu(), torch.from_numpy(w.pos0))
