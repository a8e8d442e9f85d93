"""Batched L-BFGS relaxation: the step kernel pamnet_lbfgs_step_f32 (csrc/lbfgs.hip) and the driver pamnet_amd.relax.relax_lbfgs.

The reference is tests/lbfgs_ref.py lbfgs_step_ref, the rule of include/pamnet_hip.h restated in numpy fp64.  Inputs are made once
on the CPU with fixed seeds and never modified; the conditions under which kernel and reference take the same branch (both
compute in fp64 from the same fp32 inputs) are asserted by tests that need no GPU.

Tolerances (tests/test_relax.py): KTOL = 1e-6 max-normalised, per graph, for fmax and the displacement pos_new - pos_old; 1e-12
relative for rho and gamma; equality for the integer state, for the stored s / y rows and prev_pos / prev_dpos (single correctly
rounded operations, or copies) and for everything that belongs to an atom or a graph that must not move."""
import copy

import numpy as np
import pytest
import torch

from conftest import maxnorm_err
from lbfgs_ref import ARRAYS, INT_STATE, STATE, lbfgs_step_ref, new_state_ref
from relax_ref import fire_step_ref

ENTRY = 'pamnet_lbfgs_step_f32'
KTOL = 1e-6
FMAX_TOL = 0.05
MEM = 4
# skip_tol = 0.1 in the kernel batches: a pair with y perpendicular to s has ys = 0 up to rounding, which only a threshold of this
# size separates from the branch point by the 1 % the preconditions ask for.  The memory-32 batch and the drivers run the default.
KPARAMS = dict(alpha=70.0, max_step=0.2, skip_tol=0.1)
DEFAULTS = dict(alpha=70.0, max_step=0.2, skip_tol=1e-8)
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 300, 1025, 0]
ROLES = ['first', 'first_pair', 'partial', 'full_wrap', 'skip_perp', 'skip_neg', 'reset', 'converging', 'converged', 'failed',
         'all_fixed', 'nonfinite']
SHIFTS = (0, 4, 8)                                # graph i of the batch plays ROLES[(i + shift) % 12]; the empty graph is last


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
#        role:      (has_prev, count, head, new pair, max |gr|)
PLAN = {'first': (0, 0, 0, None, 1.0), 'first_pair': (1, 0, 0, 'good', 1.0), 'partial': (1, 2, 2, 'good', 0.06),
        'full_wrap': (1, 4, 2, 'good', 1.0), 'skip_perp': (1, 1, 1, 'perp', 1.0), 'skip_neg': (1, 3, 3, 'neg', 1.0),
        'reset': (1, 1, 1, 'neg', 1.0), 'converging': (1, 2, 2, 'good', 0.03), 'nonfinite': (1, 2, 2, 'good', 1.0)}


def _fill_graph(rng, c, g, role, memory, plan=PLAN):
    """The rows and the state of graph g for its role.  A history pair is (s, y = H s) with a fixed positive diagonal H of the
    graph (entries 0.5 .. 4), s of size 0.05: curvature positive, rho = 1 / y.s.  The new pair enters through prev_pos = pos - s
    and prev_dpos = gr - y, rounded to fp32 (kernel and reference both recompute s and y from the fp32 rows):
      good  y = H s;   perp  y = H s minus its component along s over the free atoms (ys = 0 up to the rounding of the rows);   neg  y = -H s.
    reset: one pair with s along gr and y = -2 s, so rho < 0 and H_k = gamma P + rho s s^T (P the projector off s) gives
    D = gr.H_k gr < 0; its new pair has negative curvature too and is skipped, so the prepared history is what the recursion sees."""
    lo, hi = int(c.gptr[g]), int(c.gptr[g + 1])
    m = hi - lo
    if m == 0:
        return
    sl = slice(lo, hi)
    fix = np.zeros(m, dtype=bool)
    if role == 'all_fixed':
        fix[:] = True
    elif role in plan and m >= 63:
        fix[rng.choice(m, m // 5, replace=False)] = True
    free = ~fix
    c.fixed[sl] = fix
    gr = rng.standard_normal((m, 3))
    if free.any():
        gr /= np.sqrt((gr[free] ** 2).sum(1).max())
    st = c.state
    st['steps'][g], st['skipped'][g], st['resets'][g] = rng.randint(0, 40), rng.randint(0, 5), rng.randint(0, 5)
    st['fmax'][g] = -1.0
    if role in ('converged', 'failed', 'all_fixed'):
        # rows and state that must not be read (NaN would spread) nor written
        st['status'][g] = {'converged': 1, 'failed': 2, 'all_fixed': 0}[role]
        if role != 'all_fixed':
            st['fmax'][g] = 0.04 if role == 'converged' else np.inf
        st['head'][g], st['count'][g], st['has_prev'][g] = rng.randint(0, memory), rng.randint(0, memory + 1), 1
        st['rho'][g], st['gamma'][g] = rng.standard_normal(memory), rng.uniform(0.1, 1.0)
        for k in ARRAYS:
            st[k][..., sl, :] = np.nan
        c.dE[sl] = gr.astype(np.float32)
        if role == 'failed':
            c.dE[lo, 0] = np.nan
        return
    has_prev, count, head, new, scale = plan[role]
    gr *= scale
    H = rng.uniform(0.5, 4.0, (m, 3))
    st['has_prev'][g], st['count'][g], st['head'][g] = has_prev, count, head
    st['rho'][g] = rng.standard_normal(memory)                     # slots without a pair: values that must not be used
    st['gamma'][g] = rng.uniform(0.1, 1.0)
    slots = [(head - 1 - j) % memory for j in range(count)]
    for k in slots:
        s = 0.05 * rng.standard_normal((m, 3))
        y = H * s
        if role == 'reset':
            s = 0.05 * gr + 0.002 * rng.standard_normal((m, 3))
            y = -2.0 * s
            st['gamma'][g] = 0.5
        st['hist_s'][k, sl], st['hist_y'][k, sl] = s, y
        st['rho'][g, k] = 1.0 / float((s[free] * y[free]).sum())
    if count and role != 'reset':
        k = slots[0]
        st['gamma'][g] = 1.0 / (st['rho'][g, k] * float((st['hist_y'][k, sl][free] ** 2).sum()))
    c.dE[sl] = gr.astype(np.float32)
    if has_prev:
        s = 0.05 * rng.standard_normal((m, 3))
        y = H * s
        if new == 'perp':
            y[free] -= s[free] * ((s[free] * y[free]).sum() / (s[free] * s[free]).sum())
        elif new == 'neg':
            y = -y
        # (pos, gr) rounded first: s and y are what the fp32 rows give
        st['prev_pos'][sl] = (c.pos[sl].astype(np.float64) - s).astype(np.float32)
        st['prev_dpos'][sl] = (c.dE[sl].astype(np.float64) - y).astype(np.float32)
    # fixed atoms: garbage that must enter no sum, in rows that must be neither read nor written
    for k in ARRAYS:
        st[k][..., lo + np.nonzero(fix)[0], :] = np.nan
    c.dE[lo + np.nonzero(fix)[0]] = (5.0 * rng.standard_normal((int(fix.sum()), 3))).astype(np.float32)
    if role == 'nonfinite':
        a_free = lo + int(np.nonzero(free)[0][m // 2 if m > 2 else 0])
        c.dE[a_free, 1] = np.inf if c.inf else np.nan


def _make_case(key, sizes, roles, memory, params, seed, inf=False, plan=PLAN):
    if key in _MADE:
        return _MADE[key]
    rng = np.random.RandomState(seed)
    n, G = sum(sizes), len(sizes)
    c = Case()
    c.memory, c.params, c.roles, c.inf = memory, params, roles, inf
    c.gptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    c.pos = rng.uniform(-4.0, 4.0, (n, 3)).astype(np.float32)
    c.dE = np.zeros((n, 3), dtype=np.float32)
    c.fixed = np.zeros(n, dtype=bool)
    c.state = new_state_ref(n, G, memory)
    c.state['work'][:] = rng.standard_normal((n, 3))               # the workspace carries nothing from step to step
    for g, role in enumerate(roles):
        _fill_graph(rng, c, g, role, memory, plan)
    c.diag = {}
    c.ref = lbfgs_step_ref(c.pos, c.dE, c.gptr, c.state, FMAX_TOL, c.fixed, diag=c.diag, **params)
    _MADE[key] = c
    return c


def _kernel_case(shift):
    """One batch of SIZES at memory 4, graph i in role ROLES[(i + shift) % 12] (PLAN, _fill_graph):
      first       no previous step: z = gr / alpha, cap inactive
      first_pair  the first pair is stored, z = gamma (two-loop over one pair), cap active
      partial     two pairs held, the third stored; max |gr| = 0.06: cap inactive
      full_wrap   four pairs held, head = 2: the new pair overwrites the oldest and the loop runs 2, 1, 0, 3; cap active
      skip_perp / skip_neg   the new pair is refused (y perpendicular to s / negative curvature), the history stays
      reset       a prepared pair with rho < 0 makes D < 0: history cleared, z = gr / alpha
      converging  max |gr| = 0.03 < 0.05;   converged / failed: status 1 / 2 with NaN rows that must not be read;
      all_fixed   every atom fixed, NaN rows;   nonfinite  one gradient entry NaN (shift 0, 8) or inf (shift 4).
    A moving graph of 63 atoms or more has a fifth of its atoms fixed, with NaN in the rows that must not be touched."""
    roles = [ROLES[(i + shift) % 12] for i in range(len(SIZES) - 1)] + ['empty']
    return _make_case(('k', shift), SIZES, roles, MEM, KPARAMS, 200 + shift, inf=shift == 4)


def _wide_case():
    """Two graphs (65 and 300 atoms) at memory 32 with a full ring, head = 17, default parameters."""
    return _make_case(('wide',), [65, 300], ['full_wrap', 'full_wrap'], 32, DEFAULTS, 77,
                      plan=dict(PLAN, full_wrap=(1, 32, 17, 'good', 1.0)))


def _margins(d, tol, p):
    """The conditions of one graph's step record (lbfgs_ref diag) under which fp64 arithmetic in another order takes the same
    branch.  A graph that was left alone (None) or failed has none."""
    if d is None or not np.isfinite(d['F2']):
        return
    assert abs(d['fm'] - tol) >= 0.01 * tol, d
    if 'D' not in d:
        return
    if d['has_prev']:
        r = np.sqrt(d['ss'] * d['yy'])
        assert abs(d['ys'] - p['skip_tol'] * r) >= 0.01 * r, d
    assert abs(d['D']) > 1e-3 * d['znorm'] * d['grnorm'], d
    assert abs(d['L'] - p['max_step']) >= 0.01 * p['max_step'], d


# ---------------------------------------------------------------------------------------------- anisotropic wells
class Wells(torch.nn.Module):
    """E_g = 1/2 sum_{a in g} sum_c k_c (pos_ac - x0_ac)^2: a plain torch module, differentiable with respect to data.pos."""

    def __init__(self, k, x0, n_graphs):
        super().__init__()
        self.register_buffer('k', k)
        self.register_buffer('x0', x0)
        self.n_graphs = n_graphs

    def forward(self, data):
        e = 0.5 * (self.k * (data.pos - self.x0).pow(2)).sum(1)
        return torch.zeros(self.n_graphs, dtype=e.dtype, device=e.device).index_add_(0, data.batch, e)


W_SIZES, W_K, W_TOL, W_MAX, W_SEED, W_MEM = (4, 9, 70), (0.5, 2.0, 6.0), 0.01, 400, 6, 10


def _wells():
    """(x0, pos0, batch, fixed, k) and two reference trajectories from the same start, on the gradient k (pos - x0) in fp32 -- the
    two roundings of the module's backward, fl(k fl(pos - x0)), so that reference and driver step on the same numbers (a
    quasi-Newton step divides by differences of gradients: one ulp of fp32 in dE near the minimum moves the step by far more
    than KTOL): lbfgs_step_ref with the defaults (memory 10) and fire_step_ref with its defaults, until no graph is running."""
    if 'w' in _MADE:
        return _MADE['w']
    rng = np.random.RandomState(W_SEED)
    n, G = sum(W_SIZES), len(W_SIZES)
    w = Case()
    w.batch = np.repeat(np.arange(G), W_SIZES)
    w.gptr = np.concatenate([[0], np.cumsum(W_SIZES)]).astype(np.int32)
    w.x0 = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    w.pos0 = (w.x0 + rng.uniform(-1.0, 1.0, (n, 3))).astype(np.float32)
    w.fixed = rng.uniform(size=n) < 0.2
    w.fixed[0] = False
    w.k = np.asarray(W_K, dtype=np.float32)
    grad = lambda pos: w.k[None, :] * (pos - w.x0)                 # fp32, rounded as Wells' backward rounds it: the same bits
    pos, st = w.pos0.copy(), new_state_ref(n, G, W_MEM)
    w.diags = []
    for _ in range(W_MAX):
        diag = {}
        pos, st = lbfgs_step_ref(pos, grad(pos), w.gptr, st, W_TOL, w.fixed, diag=diag, **DEFAULTS)
        w.diags.append(diag)
        if not (st['status'] == 0).any():
            break
    w.pos, w.state = pos, st
    pos, vel = w.pos0.copy(), np.zeros((n, 3), np.float32)
    fs = dict(dt=np.full(G, 0.1), a=np.full(G, 0.1), n_pos=np.zeros(G, np.int32), steps=np.zeros(G, np.int32),
              status=np.zeros(G, np.int32), fmax=np.zeros(G, np.float32))
    for _ in range(W_MAX):
        pos, vel, fs = fire_step_ref(pos, vel, grad(pos), w.gptr, fs, W_TOL, w.fixed)
        if not (fs['status'] == 0).any():
            break
    w.fire_pos, w.fire_state = pos, fs
    _MADE['w'] = w
    return w


# ---------------------------------------------------------------------------------------------------------- CPU tests
def test_header_declares_the_lbfgs_step_at_abi_18():
    """(No GPU: the header and the built library.)"""
    import ctypes
    import re
    from pamnet_amd import build, lib
    decl = lib.declared_functions()
    assert ENTRY in decl
    P, D, I64, I32 = ctypes.c_void_p, ctypes.c_double, ctypes.c_int64, ctypes.c_int32
    # pos dpos fixed gptr | n n_graphs | prev_pos prev_dpos hist_s hist_y work + the ten per-graph arrays + fmax_tol_g | fmax_tol |
    # memory | alpha max_step skip_tol | stream
    assert decl[ENTRY] == [P] * 4 + [I64] * 2 + [P] * 16 + [D] + [I32] + [D] * 3 + [P]
    assert int(re.search(r'#define\s+PAMNET_ABI_VERSION\s+(\d+)', open(lib.HEADER).read()).group(1)) == 18
    h = ctypes.CDLL(build.build())
    assert h.pamnet_abi_version() == 18 and hasattr(h, ENTRY)


def test_lbfgs_step_kernel_is_scratch_free(tmp_path):
    """(No GPU: hipcc cross-compiles.)  The compiler's report for csrc/lbfgs.hip: no scratch (the a_j live in LDS, not in a
    per-thread array), registers within 128, and LDS = two sets of 4 x 5 fp64 partials + 32 fp64 a_j = 576 bytes (DESIGN section
    10b quotes the figures)."""
    import os
    import re
    import shutil
    import subprocess
    from pamnet_amd import build
    hipcc = '/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else shutil.which('hipcc')
    assert hipcc, 'hipcc not available'
    r = subprocess.run([hipcc] + build.FLAGS + ['-c', os.path.join(build.CSRC, 'lbfgs.hip'), '-o', str(tmp_path / 'lbfgs.o'),
                                                '-Rpass-analysis=kernel-resource-usage'], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = [b for b in re.split(r'remark: Function Name: ', r.stderr)[1:] if 'lbfgs_step_kernel' in b.split()[0]]
    assert len(blocks) == 1
    num = lambda key: int(re.search(key + r': (\d+)', blocks[0]).group(1))
    print('lbfgs_step_kernel: VGPRs', num('VGPRs'), 'AGPRs', num('AGPRs'), 'LDS', num(r'LDS Size \[bytes/block\]'))
    assert num(r'ScratchSize \[bytes/lane\]') == 0
    assert num('VGPRs') + num('AGPRs') <= 128
    assert num(r'LDS Size \[bytes/block\]') <= 2 * 4 * 5 * 8 + 32 * 8


def test_the_reference_relaxes_the_wells_in_half_of_fire_steps():
    """(No GPU; a test of the reference.)  lbfgs_step_ref iterated on the three anisotropic wells brings every graph below the
    threshold with its fixed atoms in place, each graph in at most half the steps fire_step_ref takes from the same start."""
    w = _wells()
    assert (w.state['status'] == 1).all(), w.state
    assert (w.fire_state['status'] == 1).all(), w.fire_state
    assert (w.state['fmax'] < W_TOL).all()
    f = w.k[None, :] * (w.pos.astype(np.float64) - w.x0)
    f[w.fixed] = 0.0
    assert np.sqrt((f ** 2).sum(1)).max() < W_TOL
    assert w.fixed.any() and np.array_equal(w.pos[w.fixed], w.pos0[w.fixed])
    assert not np.array_equal(w.pos[~w.fixed], w.pos0[~w.fixed])
    print('wells: L-BFGS steps', w.state['steps'], 'FIRE steps', w.fire_state['steps'], 'skipped', w.state['skipped'], 'resets',
          w.state['resets'])
    assert (2 * w.state['steps'] <= w.fire_state['steps']).all()


def test_lbfgs_inputs_meet_their_preconditions():
    """(No GPU.)  The kernel-test batches and the whole reference trajectory on the wells keep their distance from every branch
    point: fm 1 % away from the threshold; L 1 % away from max_step; |ys - skip_tol sqrt(ss yy)| at least 1 % of sqrt(ss yy);
    |D| > 1e-3 |z| |gr|.  The kernel batches together take every branch."""
    seen = set()
    for shift in SHIFTS:
        c = _kernel_case(shift)
        assert [int(b - a) for a, b in zip(c.gptr[:-1], c.gptr[1:])] == SIZES
        _, st = c.ref
        for g, role in enumerate(c.roles):
            d = c.diag[g]
            _margins(d, FMAX_TOL, c.params)
            b = {k: c.state[k][g] for k in INT_STATE}
            m, nfix = SIZES[g], int(c.fixed[c.gptr[g]:c.gptr[g + 1]].sum())
            if role in ('converged', 'failed'):
                assert d is None and st['status'][g] == b['status'] != 0
                seen.add(role)
                continue
            if role in ('all_fixed', 'empty', 'converging'):
                assert st['status'][g] == 1 and all(st[k][g] == b[k] for k in INT_STATE if k != 'status')
                assert (d['fm'] == 0.0 and nfix == m) if role != 'converging' else (0.0 < d['fm'] < FMAX_TOL and nfix < m)
                seen.add(role)
                continue
            if role == 'nonfinite':
                assert st['status'][g] == 2 and not np.isfinite(st['fmax'][g])
                assert np.isnan(st['fmax'][g]) == (shift != 4)
                assert all(st[k][g] == b[k] for k in INT_STATE if k != 'status')
                seen.add('nonfinite_inf' if shift == 4 else 'nonfinite_nan')
                continue
            assert st['status'][g] == 0 and st['steps'][g] == b['steps'] + 1 and st['has_prev'][g] == 1
            capped = d['L'] > c.params['max_step']
            stored, skipped, reset = d['stored'], st['skipped'][g] - b['skipped'], st['resets'][g] - b['resets']
            assert skipped == (1 if d['has_prev'] and not stored else 0) and reset == int(d['reset'])
            if role == 'first':
                assert not d['has_prev'] and d['count'] == 0 and not reset and not capped
                assert st['head'][g] == 0 and st['count'][g] == 0
            elif role == 'first_pair':
                assert stored and not reset and (st['head'][g], st['count'][g]) == (1, 1) and capped
            elif role == 'partial':
                assert stored and not reset and (st['head'][g], st['count'][g]) == (3, 3) and not capped
            elif role == 'full_wrap':
                assert stored and not reset and (b['head'], b['count']) == (2, MEM) and (st['head'][g], st['count'][g]) == (3, MEM)
                assert capped
            elif role == 'skip_perp':
                assert not stored and not reset and abs(d['ys']) < 1e-5 * np.sqrt(d['ss'] * d['yy'])   # (0 up to the fp32 rows)
                assert (st['head'][g], st['count'][g]) == (1, 1)
            elif role == 'skip_neg':
                assert not stored and not reset and d['ys'] < 0 and (st['head'][g], st['count'][g]) == (3, 3)
            else:
                assert role == 'reset' and not stored and reset and d['D'] < 0 and c.state['rho'][g, 0] < 0
                assert (st['head'][g], st['count'][g]) == (0, 0) and not capped
            seen.update([role, 'capped' if capped else 'free', 'some_fixed' if nfix else 'none_fixed'])
    assert seen == (set(ROLES) - {'nonfinite'}) | {'nonfinite_nan', 'nonfinite_inf', 'empty', 'capped', 'free', 'some_fixed',
                                                   'none_fixed'}, seen
    c = _wide_case()
    for g in range(2):
        d = c.diag[g]
        _margins(d, FMAX_TOL, c.params)
        assert d['stored'] and not d['reset'] and d['count'] == 32 and (c.state['head'][g], c.ref[1]['head'][g]) == (17, 18)
    w = _wells()
    branches = set()
    for diag in w.diags:
        for g, d in diag.items():
            _margins(d, W_TOL, DEFAULTS)
            if d is not None and 'D' in d:
                assert not d['reset']
                branches.add('stored' if d['stored'] else 'skipped' if d['has_prev'] else 'first')
                branches.add('capped' if d['L'] > DEFAULTS['max_step'] else 'free')
    assert branches == {'first', 'stored', 'capped', 'free'}, branches


def test_relax_lbfgs_refusals():
    """(No GPU.)  A PAMNet that keeps its positions in x, a batch without pos or batch, an unknown parameter, a memory of 0 or 33,
    and CPU tensors (RuntimeError: no CPU path) are refused before anything runs."""
    import models
    from pamnet_amd import synth
    from pamnet_amd.relax import new_lbfgs_state, relax_lbfgs
    w = _wells()
    model = Wells(torch.from_numpy(w.k), torch.from_numpy(w.x0), len(W_SIZES))
    data = synth.Batch(pos=torch.from_numpy(w.pos0), batch=torch.from_numpy(w.batch), num_graphs=len(W_SIZES))
    pdb = models.PAMNet(models.Config(dataset='PDBbind', dim=16, n_layer=1, cutoff_l=2.0, cutoff_g=6.0))
    with pytest.raises(ValueError, match=r'x\[:, :3\]'):
        relax_lbfgs(pdb, data)
    with pytest.raises(ValueError, match='no `pos`'):
        relax_lbfgs(model, synth.Batch(batch=data.batch, num_graphs=3))
    with pytest.raises(ValueError, match='no `batch`'):
        relax_lbfgs(model, synth.Batch(pos=data.pos, num_graphs=3))
    with pytest.raises(TypeError, match='dt_max'):
        relax_lbfgs(model, data, dt_max=1.0)
    for bad in (0, 33):
        with pytest.raises(ValueError, match='`memory`'):
            relax_lbfgs(model, data, memory=bad)
        with pytest.raises(ValueError, match='`memory`'):
            new_lbfgs_state(4, 1, torch.device('cpu'), bad)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        relax_lbfgs(model, data)
    assert torch.equal(data.pos, torch.from_numpy(w.pos0))


# ------------------------------------------------------------------------------------------------------- kernel tests
def _step_on_device(dev, c, lo=0, hi=None, graphs=None):
    """One launch on the atoms [lo, hi) / graphs `graphs` (a slice) of a case -> (pos, state) as numpy."""
    from pamnet_amd import relax as R
    graphs = slice(0, len(c.gptr) - 1) if graphs is None else graphs
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pos, dE, fixed = t(c.pos[lo:hi]), t(c.dE[lo:hi]), t(c.fixed[lo:hi].astype(np.uint8))
    gptr = t(c.gptr[graphs.start:graphs.stop + 1] - lo)
    state = {k: t(c.state[k][..., lo:hi, :]) for k in ARRAYS}
    state.update({k: t(c.state[k][graphs]) for k in STATE if k not in ARRAYS})
    R.lbfgs_step(pos, dE, gptr, state, FMAX_TOL, fixed, **c.params)
    return pos.cpu().numpy(), {k: v.cpu().numpy() for k, v in state.items()}


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _assert_step_matches(got, want, before, dE, gptr, fixed, diag, tag=''):
    """got / want / before: (pos, state); the checks of one step against lbfgs_step_ref (whose diag says what was stored)."""
    (gp, gs), (wp, ws), (bp, bs) = got, want, before
    for k in INT_STATE:
        assert np.array_equal(gs[k], ws[k]), (tag, k, gs[k], ws[k])
    for k in ('rho', 'gamma'):
        assert np.all(np.abs(gs[k] - ws[k]) <= 1e-12 * np.abs(ws[k])), (tag, k, gs[k], ws[k])
    finite = np.isfinite(ws['fmax'])
    assert np.array_equal(np.isnan(gs['fmax']), np.isnan(ws['fmax'])) and np.array_equal(np.isinf(gs['fmax']), np.isinf(ws['fmax']))
    assert np.all(np.abs(gs['fmax'][finite].astype(np.float64) - ws['fmax'][finite]) <= KTOL * np.abs(ws['fmax'][finite])), (tag, 'fmax')
    worst = 0.0
    for g in range(len(gptr) - 1):
        s = slice(int(gptr[g]), int(gptr[g + 1]))
        moved = bs['status'][g] == 0 and ws['status'][g] == 0
        if not moved:                             # finished before, or converged / failed in this step: nothing of g changed
            assert _same(gp[s], bp[s]), (tag, g)
            for k in ARRAYS:
                assert _same(gs[k][..., s, :], bs[k][..., s, :]), (tag, g, k)
            for k in STATE:
                if k not in ARRAYS and k not in ('status', 'fmax'):
                    assert _same(gs[k][g], bs[k][g]), (tag, g, k)
            if bs['status'][g] != 0:
                assert _same(gs['fmax'][g], bs['fmax'][g])
            continue
        if s.stop == s.start:
            continue
        fx = fixed[s]
        assert _same(gp[s][fx], bp[s][fx]), (tag, g, 'fixed rows')
        for k in ARRAYS:
            assert _same(gs[k][..., s, :][..., fx, :], bs[k][..., s, :][..., fx, :]), (tag, g, k, 'fixed rows')
        fr = ~fx
        assert np.array_equal(gs['prev_pos'][s][fr], bp[s][fr]) and np.array_equal(gs['prev_dpos'][s][fr], dE[s][fr]), (tag, g, 'prev')
        d = diag[g]
        for k in ('hist_s', 'hist_y'):            # the stored rows are single fp64 subtractions: equal; every other slot stays
            assert np.array_equal(gs[k][:, s][:, fr], ws[k][:, s][:, fr]), (tag, g, k)
            keep = [i for i in range(gs[k].shape[0]) if not (d['stored'] and i == d['head_in'])]
            assert np.array_equal(gs[k][keep][:, s][:, fr], bs[k][keep][:, s][:, fr]), (tag, g, k, 'other slots')
        keep = [i for i in range(gs['rho'].shape[1]) if not (d['stored'] and i == d['head_in'])]
        assert np.array_equal(gs['rho'][g, keep], bs['rho'][g, keep]), (tag, g, 'rho of the other slots')
        if not d['stored']:
            assert gs['gamma'][g] == bs['gamma'][g], (tag, g, 'gamma')
        ed = maxnorm_err(gp[s].astype(np.float64) - bp[s], wp[s].astype(np.float64) - bp[s])
        assert float(np.abs(wp[s].astype(np.float64) - bp[s]).max()) > 0
        worst = max(worst, ed)
        assert ed <= KTOL, (tag, g, ed)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize('shift', SHIFTS)
def test_one_step_on_a_batch_vs_the_reference(dev, shift):
    """Graphs of 1, 2, 63, 64, 65, 255, 256, 257, 300, 1025 and 0 atoms at memory 4 whose prepared states take every branch
    (_kernel_case; the shift moves the branches over the sizes): integer state equal; rho, gamma to 1e-12; fmax and the
    displacement within KTOL per graph; prev_pos / prev_dpos and the stored s / y rows equal; rows of fixed atoms, of finished
    graphs and of the graph that fails equal to the inputs, NaN for NaN."""
    c = _kernel_case(shift)
    got = _step_on_device(dev, c)
    worst = _assert_step_matches(got, c.ref, (c.pos, c.state), c.dE, c.gptr, c.fixed, c.diag, tag=shift)
    print('shift', shift, 'worst displacement error', worst)
    moving = np.concatenate([np.arange(c.gptr[g], c.gptr[g + 1]) for g in range(len(SIZES)) if c.ref[1]['status'][g] == 0])
    assert np.isfinite(got[0][moving]).all()


@pytest.mark.gpu
def test_one_step_at_memory_32_with_a_full_ring(dev):
    """Graphs of 65 and 300 atoms, 32 pairs held, head = 17, default parameters: 66 dependent reductions and every a_j in use."""
    c = _wide_case()
    got = _step_on_device(dev, c)
    worst = _assert_step_matches(got, c.ref, (c.pos, c.state), c.dE, c.gptr, c.fixed, c.diag, tag='wide')
    print('memory 32: worst displacement error', worst)


@pytest.mark.gpu
def test_a_step_is_repeatable_and_independent_of_the_batch(dev):
    """Two runs on the same inputs are equal bit for bit, and every graph stepped alone -- its atoms and its state as a batch of
    one -- gives the rows and the state of the batched call (`work` included: the same arithmetic in the same order)."""
    for shift in SHIFTS:
        c = _kernel_case(shift)
        p1, s1 = _step_on_device(dev, c)
        p2, s2 = _step_on_device(dev, c)
        assert _same(p1, p2) and all(_same(s1[k], s2[k]) for k in STATE)
        for g in range(len(SIZES)):
            lo, hi = int(c.gptr[g]), int(c.gptr[g + 1])
            p, s = _step_on_device(dev, c, lo, hi, slice(g, g + 1))
            assert _same(p, p1[lo:hi]), (shift, g)
            assert all(_same(s[k], s1[k][..., lo:hi, :]) for k in ARRAYS), (shift, g)
            assert all(_same(s[k], s1[k][g:g + 1]) for k in STATE if k not in ARRAYS), (shift, g)


@pytest.mark.gpu
def test_the_entry_point_validates_its_arguments(dev):
    """A null required pointer is PAMNET_ENULL, a bad count or parameter PAMNET_EINVAL (memory 0 and 33 among them); `fixed` and
    the per-graph threshold may be null; n_graphs == 0 launches nothing; a per-graph threshold replaces the scalar."""
    from pamnet_amd import lib
    c = _kernel_case(0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pos, dE, gptr = t(c.pos), t(c.dE), t(c.gptr)
    st = {k: t(c.state[k]) for k in STATE}
    G, n = len(SIZES), pos.size(0)
    order = ('prev_pos', 'prev_dpos', 'hist_s', 'hist_y', 'work', 'rho', 'gamma', 'head', 'count', 'has_prev', 'skipped', 'resets',
             'steps', 'status', 'fmax')

    def call(**kw):
        a = dict(pos=lib.ptr(pos), dpos=lib.ptr(dE), fixed=None, gptr=lib.ptr(gptr), n=n, G=G, fmax_tol_g=None, fmax_tol=1e9,
                 memory=MEM, alpha=70.0, max_step=0.2, skip_tol=0.1)
        a.update({k: lib.ptr(st[k]) for k in STATE})
        a.update(kw)
        lib.call(ENTRY, a['pos'], a['dpos'], a['fixed'], a['gptr'], a['n'], a['G'], *([a[k] for k in order] +
                 [a['fmax_tol_g'], a['fmax_tol'], a['memory'], a['alpha'], a['max_step'], a['skip_tol'], lib.stream_of(pos)]))

    for k in ('pos', 'dpos', 'gptr') + order:
        with pytest.raises(RuntimeError, match='PAMNET_ENULL'):
            call(**{k: None})
    for kw in (dict(n=-1), dict(G=-1), dict(G=2 ** 31), dict(memory=0), dict(memory=33), dict(memory=-1), dict(alpha=0.0),
               dict(alpha=float('inf')), dict(max_step=-0.2), dict(max_step=float('nan')), dict(skip_tol=-1e-8),
               dict(skip_tol=float('nan')), dict(fmax_tol=float('nan'))):
        with pytest.raises(RuntimeError, match='PAMNET_EINVAL'):
            call(**kw)
    call(G=0)
    torch.cuda.synchronize()
    same = lambda a, b: _same(a.cpu().numpy(), b)
    assert same(pos, c.pos) and all(same(st[k], c.state[k]) for k in STATE)
    # a threshold of 1e9 converges every running graph whose gradient is finite; per graph: only those it is handed to
    tol_g = torch.full((G,), 1e9, device=dev)
    tol_g[3] = 1e-9
    call(fmax_tol_g=lib.ptr(tol_g), fmax_tol=1e-9)
    status = st['status'].cpu().numpy()
    roles = np.array(c.roles)
    assert status[3] == 0 and roles[3] == 'full_wrap' and int(st['steps'][3]) == c.state['steps'][3] + 1
    assert (status[roles == 'failed'] == 2).all() and (status[roles == 'nonfinite'] == 2).all()
    assert (status[~np.isin(roles, ['failed', 'nonfinite']) & (np.arange(G) != 3)] == 1).all()


# ----------------------------------------------------------------------------------------------------- end to end
@pytest.mark.gpu
def test_the_wells_relax_as_the_reference_does(dev):
    """A plain torch module, the three anisotropic wells, some atoms fixed: per-graph steps, status, skipped and resets equal the
    reference's (whose margins the CPU test asserts for the whole trajectory, and which steps on the module's own gradient bits:
    _wells), the displacement from the start agrees within KTOL per graph, fixed atoms and the caller's positions stay; and, where torch can police synchronisation, check_every=0
    enqueues without one."""
    from pamnet_amd import synth
    from pamnet_amd.relax import relax_lbfgs
    w = _wells()
    G = len(W_SIZES)
    model = Wells(torch.from_numpy(w.k), torch.from_numpy(w.x0), G).to(dev)
    data = synth.Batch(pos=torch.from_numpy(w.pos0), batch=torch.from_numpy(w.batch), num_graphs=G).to(dev)
    fixed = torch.from_numpy(w.fixed).to(dev)
    res = relax_lbfgs(model, data, fmax=W_TOL, max_steps=W_MAX, fixed=fixed, check_every=5)
    assert res.trace is None and res.pos is not data.pos and torch.equal(data.pos.cpu(), torch.from_numpy(w.pos0))
    assert np.array_equal(res.steps.cpu().numpy(), w.state['steps']), (res.steps, w.state['steps'])
    assert res.converged.dtype == torch.bool and res.converged.all() and not res.failed.any()
    assert np.array_equal(res.converged.cpu().numpy(), w.state['status'] == 1)
    assert np.array_equal(res.skipped.cpu().numpy(), w.state['skipped']) and np.array_equal(res.resets.cpu().numpy(), w.state['resets'])
    got = res.pos.cpu().numpy().astype(np.float64)
    for g in range(G):
        s = slice(int(w.gptr[g]), int(w.gptr[g + 1]))
        err = maxnorm_err(got[s] - w.pos0[s], w.pos[s].astype(np.float64) - w.pos0[s])
        print('wells: graph', g, 'steps', int(res.steps[g]), 'displacement error', err)
        assert err <= KTOL, (g, err)
    assert torch.equal(res.pos[fixed], data.pos[fixed])
    assert (res.fmax < W_TOL).all() and maxnorm_err(res.fmax.cpu().numpy(), w.state['fmax']) <= 1e-5
    assert torch.equal(res.forces, -model.k * (res.pos - model.x0))
    try:
        torch.cuda.set_sync_debug_mode('error')
    except Exception as e:                        # (a build without the debug mode: the rest of the test has run)
        print('set_sync_debug_mode is not available:', e)
        return
    try:
        res0 = relax_lbfgs(model, data, fmax=1e-9, max_steps=6, fixed=fixed, check_every=0)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert res0.pos.is_cuda and res0.steps.tolist() == [6] * G


@pytest.mark.gpu
def test_pamnet_relaxation_replayed_step_by_step(dev):
    """PAMNet (d = 32, L = 2) on {bond-free molecule, triclinic cell, slab with a fixed bottom layer}, trace=True, 8 steps: every
    recorded step, replayed alone through lbfgs_step_ref from its recorded inputs, matches as in the kernel test; res.energy /
    res.forces are bitwise a fresh evaluation at res.pos; fixed rows, the caller's positions and every parameter .grad are as
    they were; and after the first step -- steepest descent of length at most fm / alpha -- every graph's energy is lower."""
    import models
    from pamnet_amd.relax import relax_lbfgs
    from test_pbc_axes import CUT_G, CUT_L
    from test_relax import _pamnet_batch
    b, fixed_cpu = _pamnet_batch()
    torch.manual_seed(0)
    model = models.PAMNet(models.Config(dataset='QM9', dim=32, n_layer=2, cutoff_l=CUT_L, cutoff_g=CUT_G)).to(dev)
    data, fixed = b.to(dev), fixed_cpu.to(dev)
    model(data).sum().backward()                                   # parameter gradients to find untouched afterwards
    snap = [None if p.grad is None else p.grad.clone() for p in model.parameters()]
    assert sum(s is not None for s in snap) > 10
    pos0 = data.pos.clone()
    res = relax_lbfgs(model, data, fmax=1e-6, max_steps=8, fixed=fixed, trace=True)
    assert torch.equal(data.pos, pos0) and not data.pos.requires_grad
    for p, s in zip(model.parameters(), snap):
        assert (p.grad is None) if s is None else torch.equal(p.grad, s)
    assert len(res.trace) == 8 and res.steps.tolist() == [8, 8, 8] and not res.converged.any() and not res.failed.any()
    assert torch.equal(res.pos[fixed], pos0[fixed]) and not torch.equal(res.pos[~fixed], pos0[~fixed])
    print('skipped', res.skipped.tolist(), 'resets', res.resets.tolist())
    gptr = np.concatenate([[0], np.cumsum(np.bincount(b.batch.numpy(), minlength=3))])
    cpu = lambda t: t.cpu().numpy()
    worst = 0.0
    for i, r in enumerate(res.trace):
        before = (cpu(r['pos']), {k: cpu(v) for k, v in r['state_before'].items()})
        got = (cpu(r['pos_after']), {k: cpu(v) for k, v in r['state_after'].items()})
        diag = {}
        want = lbfgs_step_ref(before[0], cpu(r['dE']), gptr, before[1], 1e-6, fixed_cpu.numpy(), diag=diag, **DEFAULTS)
        worst = max(worst, _assert_step_matches(got, want, before, cpu(r['dE']), gptr, fixed_cpu.numpy(), diag, tag=i))
        if i + 1 < len(res.trace):
            nxt = res.trace[i + 1]
            assert torch.equal(r['pos_after'], nxt['pos'])
            assert all(torch.equal(r['state_after'][k], nxt['state_before'][k]) for k in STATE)
    print('replay: worst displacement error', worst)
    assert torch.equal(res.trace[-1]['pos_after'], res.pos)

    def fresh(pos):
        d = copy.copy(data)
        d.pos = pos.clone().requires_grad_(True)
        e = model(d)
        return e.detach(), torch.autograd.grad(e.sum(), d.pos)[0]

    e, de = fresh(res.pos)
    assert torch.equal(res.energy, e) and torch.equal(res.forces, -de) and torch.isfinite(res.forces).all()
    e0, e1 = fresh(pos0)[0], fresh(res.trace[1]['pos'])[0]
    print('energies: start', e0.tolist(), 'after the first step', e1.tolist(), 'after 8 steps', e.tolist())
    assert (e1 < e0).all()
