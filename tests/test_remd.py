"""Replica-exchange molecular dynamics: the kernel pamnet_remd_exchange_f64 (csrc/remd.hip) and the driver pamnet_amd/remd.py.

The reference is tests/remd_ref.py: exchange_ref, the rule of include/pamnet_hip.h restated in numpy fp64 on the Philox4x32-10
generator of tests/md_ref.py, and remd_run_ref, the driver's launch sequence over md_step_ref.  Inputs are made once on the CPU
with fixed seeds and never modified; what the GPU tests presuppose of the reference is asserted by tests that need no GPU.

Tolerances: equality for every integer output and for kT_g (a copy of an input); 1e-14 relative for ke (one fp64 product, the
quotient formed the same way on both sides); one fp32 ulp for a scaled velocity (fp64 sqrt and product, one rounding: the
device's sqrt may differ from numpy's in its last bit, which can move the rounding by one ulp); bitwise for every row that must
not change.  The step launches of a trace are checked as tests/test_md.py checks them (KTOL)."""
import warnings

import numpy as np
import pytest
import torch

from md_ref import md_step_ref
from remd_ref import LADDER, exchange_many_ref, exchange_ref, new_ladder, remd_run_ref
from test_md import KTOL, MODELS, Harmonic, _assert_step_matches

ENTRY = 'pamnet_remd_exchange_f64'
MARGIN = 1e-9                                     # |u - exp(D)| above which an fp64 exp that differs in its last bits cannot flip a decision
KT4 = (0.4, 0.55, 0.75, 1.0)
D_WELL = 24                                       # degrees of freedom of the 8-atom well: <E> = 12 kT


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs an MI355X'
    from pamnet_amd import lib
    lib.load()
    return torch.device('cuda:0')


class Case(object):
    pass


_MADE = {}


def _ptr(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


# ------------------------------------------------------------------------------------------------- kernel-test inputs
RUNGS = (1, 2, 3, 5, 8)                           # the ladders of the kernel case ...
ATOMS = (4, 300, 70, 9, 1)                        # ... and the atoms of each of their graphs: below, above a wavefront and a workgroup
CASE_SEED = 4                                     # (the first seed tried: it has every outcome, test_kernel_inputs_meet_their_preconditions)


def _kernel_case(parity):
    """Ladders of 1, 2, 3, 5 and 8 rungs (19 graphs of 4 / 300 / 70 / 9 / 1 atoms), geometric temperatures 0.4 .. 1.0 per ladder,
    energies Gamma(12) kT of the rung, a fifth of the atoms of the graphs of 9 atoms or more fixed, ke and velocities random,
    seeds over all of int64, attempts = (2, 6, 0, 4, 10) + parity.  Graph 2 of the ladder of five has status 2 and NaN / inf in
    its velocities; graph 5 of the ladder of eight has a NaN energy.  The tables start at the identity: the second of two
    attempts in sequence starts from exchanged ones."""
    if ('case', parity) in _MADE:
        return _MADE[('case', parity)]
    rng = np.random.RandomState(CASE_SEED)
    c = Case()
    c.lptr = _ptr(RUNGS)
    sizes = np.repeat(ATOMS, RUNGS)
    G, n = len(sizes), int(sizes.sum())
    c.gptr = _ptr(sizes)
    c.kT = np.concatenate([np.array([0.7]) if R == 1 else 0.4 * (1.0 / 0.4) ** (np.arange(R) / (R - 1.0)) for R in RUNGS])
    c.energy = rng.gamma(12.0, size=G) * c.kT
    c.vel = rng.standard_normal((n, 3)).astype(np.float32)
    c.ke = rng.uniform(1.0, 20.0, G)
    c.status = np.zeros(G, np.int32)
    c.fixed = np.zeros(n, dtype=bool)
    for g in range(G):
        m = int(sizes[g])
        if m >= 9:
            c.fixed[int(c.gptr[g]) + rng.choice(m, m // 5, replace=False)] = True
    c.failed, c.nan = int(c.lptr[3]) + 2, int(c.lptr[4]) + 5
    c.status[c.failed] = 2
    c.vel[int(c.gptr[c.failed])] = (np.nan, np.inf, 1.0)
    c.energy[c.nan] = np.nan
    seeds = rng.randint(-2 ** 63, 2 ** 63 - 1, len(RUNGS), dtype=np.int64)
    c.ladder = new_ladder(c.kT, c.lptr, seeds)
    c.ladder['attempts'] = (np.array([2, 6, 0, 4, 10]) + parity).astype(np.int32)
    c.ladder['tried'], c.ladder['accepted'] = rng.randint(0, 9, G).astype(np.int32), rng.randint(0, 9, G).astype(np.int32)
    _MADE[('case', parity)] = c
    return c


def _two_attempts(c):
    """The reference's two attempts in sequence: [(vel, ladder, ke, info)] with the inputs of the second the outputs of the first."""
    key = ('ref', id(c))
    if key not in _MADE:
        out, vel, ladder, ke = [], c.vel, c.ladder, c.ke
        for _ in range(2):
            info = []
            vel, ladder, ke = exchange_ref(c.energy, vel, c.gptr, c.lptr, c.kT, ladder, c.status, ke, c.fixed, info)
            out.append((vel, ladder, ke, info))
        _MADE[key] = out
    return _MADE[key]


def _subset(c, ladders):
    """The ladders `ladders` (a slice) of a case as a case of their own: graphs, atoms and the entries of slot re-based."""
    s = Case()
    g0, g1 = int(c.lptr[ladders.start]), int(c.lptr[ladders.stop])
    a0, a1 = int(c.gptr[g0]), int(c.gptr[g1])
    s.lptr, s.gptr = (c.lptr[ladders.start:ladders.stop + 1] - g0).astype(np.int32), (c.gptr[g0:g1 + 1] - a0).astype(np.int32)
    s.kT, s.energy, s.ke, s.status = c.kT[g0:g1], c.energy[g0:g1], c.ke[g0:g1], c.status[g0:g1]
    s.vel, s.fixed = c.vel[a0:a1], c.fixed[a0:a1]
    s.ladder = {k: c.ladder[k][g0:g1] for k in ('kT_g', 'rung', 'tried', 'accepted')}
    s.ladder['slot'] = (c.ladder['slot'][g0:g1] - g0).astype(np.int32)
    s.ladder['attempts'], s.ladder['seed'] = c.ladder['attempts'][ladders], c.ladder['seed'][ladders]
    return s


def _many_pairs():
    """64 ladders of two one-atom graphs with the same two energies, D = -0.8 (acceptance exp(-0.8) = 0.45): the accepted
    ladders are a 64-bit print of the uniforms."""
    if 'pairs' not in _MADE:
        c = Case()
        L = 64
        c.lptr, c.gptr = _ptr([2] * L), _ptr([1] * (2 * L))
        c.kT = np.tile([0.5, 1.0], L)
        c.energy = np.tile([0.4, 1.2], L)                            # D = (2 - 1)(0.4 - 1.2) = -0.8
        c.vel = np.ones((2 * L, 3), np.float32)
        c.ke, c.status, c.fixed = np.full(2 * L, 1.5), np.zeros(2 * L, np.int32), np.zeros(2 * L, bool)
        c.ladder = new_ladder(c.kT, c.lptr, 1000 + np.arange(L, dtype=np.int64))
        _MADE['pairs'] = c
    return _MADE['pairs']


# ------------------------------------------------------------------------------------------------------- harmonic wells
H_DT, H_GAMMA, H_K, H_EVERY, H_STEPS, H_REC, H_TRACED = 0.05, 2.0, 2.0, 10, 8000, 10, 200
B_REF, B_GPU = 0.025, 0.05                        # the margins of check (b): see test_the_reference_ladders_sample_their_temperatures


def _wells():
    """Two ladders x 4 replicas of an 8-atom harmonic well (unit masses, k = 2, d = 24) that start at the minimum: x0, batch,
    gptr, lptr, kT, the per-graph seeds of the dynamics and the per-ladder seeds of the exchange."""
    if 'wells' not in _MADE:
        rng = np.random.RandomState(17)
        h = Case()
        G, m = 8, 8
        h.gptr, h.lptr, h.batch = _ptr([m] * G), _ptr([4, 4]), np.repeat(np.arange(G), m)
        h.x0 = np.tile(rng.uniform(-1.0, 1.0, (m, 3)), (G, 1)).astype(np.float32)
        h.k = np.full(G, H_K, np.float32)
        h.kT = np.tile(KT4, 2)
        h.seeds = np.array([101, 202, 303, 404, 505, 606, 707, 808], dtype=np.int64)
        h.xseeds = np.array([31, -77], dtype=np.int64)
        _MADE['wells'] = h
    return _MADE['wells']


def _wells_reference():
    """remd_run_ref on _wells: Maxwell-Boltzmann start (centre of mass kept: remove_com False), gamma = 2, dt = 0.05,
    exchange_every = 10, 8000 steps, a record every 10."""
    if 'wells_ref' not in _MADE:
        from md_ref import init_velocities_ref
        h = _wells()
        kk = h.k.astype(np.float64)[h.batch, None]

        def grad(pos):
            d = pos.astype(np.float64) - h.x0
            return np.bincount(h.batch, weights=0.5 * (kk * d * d).sum(1), minlength=8), (kk * d).astype(np.float32)

        vel, ke = init_velocities_ref(np.zeros((64, 3), np.float32), h.gptr, h.seeds, h.kT, None, None, False, False)
        st = dict(seed=h.seeds, steps=np.zeros(8, np.int32), status=np.zeros(8, np.int32), ke=ke)
        _MADE['wells_ref'] = remd_run_ref(grad, h.x0, vel, h.gptr, h.lptr, st, new_ladder(h.kT, h.lptr, h.xseeds), H_STEPS, H_DT,
                                          h.kT, H_GAMMA, H_EVERY, record_every=H_REC)
    return _MADE['wells_ref']


def _rung_means(epot, frame_rung):
    """The mean potential energy per rung over the second half of the records and over both ladders, relative to 12 kT_r."""
    F = len(epot)
    by = np.zeros_like(epot)
    first = np.repeat([0, 4], 4)
    by[np.arange(F)[:, None], first[None, :] + frame_rung] = epot
    half = by[F // 2:]
    return half.reshape(len(half), 2, 4).mean((0, 1)) / (0.5 * D_WELL * np.asarray(KT4)) - 1.0


# ---------------------------------------------------------------------------------------------------------- CPU tests
def test_header_declares_the_exchange_entry_point_at_abi_18():
    """(No GPU: the header and the built library.)"""
    import ctypes
    import re
    from pamnet_amd import build, lib
    decl = lib.declared_functions()
    P, I64 = ctypes.c_void_p, ctypes.c_int64
    assert decl[ENTRY] == [P] * 15 + [I64] * 3 + [P]
    assert int(re.search(r'#define\s+PAMNET_ABI_VERSION\s+(\d+)', open(lib.HEADER).read()).group(1)) == 18
    h = ctypes.CDLL(build.build())
    assert h.pamnet_abi_version() == 18 and hasattr(h, ENTRY)


def test_the_exchange_kernel_is_scratch_free(tmp_path):
    """(No GPU: hipcc cross-compiles.)  The compiler's report for csrc/remd.hip: no scratch, and LDS at or below the 3072 bytes of
    one fp64 scale and one int32 graph per rung of a ladder of 256."""
    import os
    import re
    import shutil
    import subprocess
    from pamnet_amd import build
    hipcc = '/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else shutil.which('hipcc')
    assert hipcc, 'hipcc not available'
    r = subprocess.run([hipcc] + build.FLAGS + ['-c', os.path.join(build.CSRC, 'remd.hip'), '-o', str(tmp_path / 'remd.o'),
                                                '-Rpass-analysis=kernel-resource-usage'], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = [b for b in re.split(r'remark: Function Name: ', r.stderr)[1:] if 'remd_exchange_kernel' in b.split()[0]]
    assert len(blocks) == 1
    num = lambda key: int(re.search(key + r': (\d+)', blocks[0]).group(1))
    assert num(r'ScratchSize \[bytes/lane\]') == 0
    assert num(r'LDS Size \[bytes/block\]') <= 256 * (8 + 4)


def test_the_rule_keeps_every_rungs_ensemble():
    """(No GPU.)  200 000 ladders with energies drawn i.i.d. from Gamma(d / 2) kT_r, d = 24, kT = (0.4, 0.55, 0.75, 1.0), numpy
    seed 5, per-ladder exchange seeds 0 .. 199 999: after one exchange of either parity with the Philox uniforms the mean energy on
    every rung is within 4 standard errors (sqrt(12) kT_r / sqrt(L)) of 12 kT_r and every pair's acceptance lies strictly inside
    (0.3, 0.6).  The vectorised exchange_many_ref that makes this quick is exchange_ref on the first 300 ladders, decision by
    decision; with the opposite sign of D the means move by hundreds of standard errors (asserted: more than 50)."""
    L, kT = 200000, np.asarray(KT4)
    rng = np.random.RandomState(5)
    energy = rng.gamma(D_WELL / 2.0, size=(L, 4)) * kT
    seeds = np.arange(L, dtype=np.int64)
    se = np.sqrt(D_WELL / 2.0) * kT / np.sqrt(L)
    for attempt in (0, 1):
        out, acc, rungs = exchange_many_ref(energy, kT, seeds, attempt)
        z = (out.mean(0) - 0.5 * D_WELL * kT) / se
        print('attempt', attempt, 'z of the mean energy per rung', z, 'acceptance of the pairs', rungs, acc.mean(0))
        assert rungs.tolist() == ([0, 2] if attempt == 0 else [1])
        assert (np.abs(z) <= 4.0).all()
        assert ((acc.mean(0) > 0.3) & (acc.mean(0) < 0.6)).all()
        m = 300
        ladder = new_ladder(np.tile(kT, m), _ptr([4] * m), seeds[:m])
        ladder['attempts'][:] = attempt
        _, st, _ = exchange_ref(energy[:m].ravel(), np.zeros((4 * m, 3), np.float32), _ptr([1] * (4 * m)), _ptr([4] * m), np.tile(kT, m),
                                ladder, np.zeros(4 * m, np.int32), np.zeros(4 * m))
        assert np.array_equal(st['accepted'].reshape(m, 4)[:, rungs].astype(bool), acc[:m])
        assert np.array_equal(energy[:m].ravel()[st['slot']].reshape(m, 4), out[:m])
        wrong, _, _ = exchange_many_ref(-energy, kT, seeds, attempt)                    # D with the opposite sign
        assert np.abs((-wrong.mean(0) - 0.5 * D_WELL * kT) / se).max() > 50.0


@pytest.mark.parametrize('parity', [0, 1])
def test_kernel_inputs_meet_their_preconditions(parity):
    """(No GPU.)  The kernel case under the reference, two attempts in sequence: every tried pair has |u - exp(D)| > 1e-9 (an fp64
    exp that differs in its last bits cannot flip a decision); the second attempt starts from tables that are not the identity;
    the pairs next to the failed graph and to the NaN energy are skipped; slot stays the inverse of rung.  Over both parities the
    case has an accepted pair with D < 0, one with D >= 0, a rejected and a skipped pair (CASE_SEED)."""
    c = _kernel_case(parity)
    assert [int(b - a) for a, b in zip(c.lptr[:-1], c.lptr[1:])] == list(RUNGS) and c.fixed.any()
    assert sorted(set(np.diff(c.gptr).tolist())) == [1, 4, 9, 70, 300]
    (v1, l1, k1, info1), (v2, l2, k2, info2) = _two_attempts(c)
    for info in (info1, info2):
        assert all(abs(u - e) > MARGIN for _, _, d, u, e, _ in info if d < 0.0)
    assert not np.array_equal(l1['rung'], c.ladder['rung']) and not np.array_equal(l2['rung'], l1['rung'])
    assert np.array_equal(l2['attempts'], c.ladder['attempts'] + 2)
    for st in (l1, l2):
        lo = np.repeat(c.lptr[:-1], np.diff(c.lptr))
        assert np.array_equal(st['slot'][lo + st['rung']], np.arange(len(lo)))
        assert st['rung'][c.failed] == 2 and st['kT_g'][c.failed] == c.kT[c.failed]
    assert np.array_equal(v2[int(c.gptr[c.failed])], c.vel[int(c.gptr[c.failed])], equal_nan=True)
    assert np.array_equal(v2[c.fixed], c.vel[c.fixed])
    kinds = set()
    for p in (0, 1):
        cc = _kernel_case(p)
        before = cc.ladder
        for vel, st, ke, info in _two_attempts(cc):
            kinds |= {('accepted', d < 0.0) for _, _, d, _, _, a in info if a} | {('rejected',) for *_, a in info if not a}
            pairs = sum(len(range(int(a) & 1, R - 1, 2)) for a, R in zip(before['attempts'], RUNGS))
            if len(info) < pairs:
                kinds.add(('skipped',))
            assert (st['tried'] - before['tried']).sum() == len(info)
            before = st
    print('outcomes of the kernel case:', sorted(kinds))
    assert kinds == {('accepted', True), ('accepted', False), ('rejected',), ('skipped',)}
    m = _many_pairs()
    info = []
    _, st, _ = exchange_ref(m.energy, m.vel, m.gptr, m.lptr, m.kT, m.ladder, m.status, m.ke, m.fixed, info)
    assert len(info) == 64 and all(abs(u - e) > MARGIN and abs(d + 0.8) < 1e-12 for _, _, d, u, e, _ in info)
    assert 16 < st['accepted'].sum() < 48


def test_the_reference_ladders_sample_their_temperatures():
    """(No GPU.)  remd_run_ref on the wells of the driver test (two ladders x 4 replicas of an 8-atom well, k = 2, unit masses,
    kT = (0.4, 0.55, 0.75, 1.0), gamma = 2, dt = 0.05, exchange_every = 10, 8000 steps, a record every 10): the potential
    energy in RUNG order, averaged over the second half of the records and over the two ladders (802 records per rung), is
    12 kT_r on every rung within b_ref = 2.5 %: the reference's measured worst relative deviation is 2.03 %, rounded up to the next
    0.5 %.  The device test asserts b_gpu = 2 b_ref = 5 % (the precedent of test_a_harmonic_well_reaches_its_temperature: 2.5 % and
    5 %).  The runs are 8000 steps long, not 2000: at 2000 steps the reference's own worst deviation is 5.36 % and at 4000 steps
    5.03 %, both above 5 %, so the reference and the device run were lengthened alike and the margin was not.  Every pair is tried
    at every attempt of its parity and accepts some; the rungs of a ladder stay a permutation."""
    r = _wells_reference()
    dev_ = _rung_means(r['epot'], r['frame_rung'])
    acc = r['ladder']['accepted'] / np.maximum(r['ladder']['tried'], 1)
    print('reference ladders: relative deviation of <epot> per rung', dev_, 'worst', np.abs(dev_).max(), 'acceptance', acc)
    assert np.abs(dev_).max() <= B_REF and B_GPU == 2 * B_REF and B_REF <= 0.05
    A = (H_STEPS - 1) // H_EVERY
    assert r['ladder']['attempts'].tolist() == [A, A] and r['rungs'].shape == (A + 1, 8)
    assert r['ladder']['tried'].tolist() == [(A + 1) // 2, A // 2, (A + 1) // 2, 0] * 2
    assert all(0 < r['ladder']['accepted'][i] < r['ladder']['tried'][i] for i in (0, 1, 2, 4, 5, 6))
    assert (np.sort(r['rungs'].reshape(-1, 2, 4), axis=2) == np.arange(4)).all()
    assert (r['state']['steps'] == H_STEPS).all() and (r['state']['status'] == 0).all()


def test_host_refusals_and_helpers():
    """(No GPU.)  What run() refuses before anything touches the device: a gamma that is not positive (the message says why), a
    `replicas` that does not divide num_graphs, a malformed ladder pointer, a ladder above 256 rungs, a kT that is not fp64 [G], a
    negative exchange_every; then the CPU batch itself (RuntimeError: no CPU path).  temperatures() is geometric; replicate()
    repeats atoms, types, edges (offset per copy) and per-graph fields and attaches ladder_ptr; new_ladder_state() starts every
    graph on the rung of its place."""
    from pamnet_amd import remd, synth
    h = _wells()
    model = Harmonic(torch.from_numpy(h.k), torch.from_numpy(h.x0))
    data = synth.Batch(pos=torch.from_numpy(h.x0), batch=torch.from_numpy(h.batch), num_graphs=8)
    kT = torch.from_numpy(h.kT)
    ok = dict(steps=5, dt=H_DT, kT=kT, replicas=4, exchange_every=2, gamma=H_GAMMA)
    big = synth.Batch(pos=torch.zeros(257, 3), batch=torch.arange(257), num_graphs=257)
    cases = [(dict(gamma=0.0), 'thermostat'), (dict(gamma=-1.0), 'thermostat'), (dict(gamma=None), 'canonical ensemble'),
             (dict(replicas=3), 'divide num_graphs'), (dict(replicas=0), 'divide num_graphs'),
             (dict(replicas=[0, 5, 3, 8]), 'does not decrease'), (dict(replicas=[1, 4, 8]), 'starts at 0'),
             (dict(replicas=[0, 4, 7]), 'ends at num_graphs'), (dict(replicas=torch.tensor([0, 4, 8])), 'int32'),
             (dict(replicas='x'), '`replicas` is an int'), (dict(replicas=None), 'ladder_ptr'),
             (dict(kT=kT.float()), '`kT` is a float64'), (dict(kT=kT[:-1]), '`kT` is a float64'), (dict(kT=0.5), '`kT` is a float64'),
             (dict(exchange_every=-1), 'non-negative'), (dict(steps=-1), 'non-negative')]
    for kw, match in cases:
        args = dict(ok)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            remd.run(model, data, **args)
    with pytest.raises(ValueError, match='at most 256 rungs'):
        remd.run(model, big, 5, H_DT, kT=torch.ones(257, dtype=torch.float64), replicas=257, exchange_every=2, gamma=1.0)
    with pytest.raises(ValueError, match='at most 256 rungs'):
        remd.run(model, big, 5, H_DT, kT=torch.ones(257, dtype=torch.float64), replicas=[0, 257], exchange_every=2, gamma=1.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        remd.run(model, data, **ok)
    assert remd.MAX_RUNGS == 256
    t = remd.temperatures(0.4, 1.0, 4)
    assert t.dtype == torch.float64 and float(t[0]) == 0.4 and float(t[-1]) == 1.0
    assert torch.allclose(t[1:] / t[:-1], torch.full((3,), 2.5 ** (1.0 / 3.0), dtype=torch.float64), rtol=1e-14, atol=0.0)
    assert remd.temperatures(0.3, 0.9, 1).tolist() == [0.3]
    for bad in ((0.0, 1.0, 3), (1.0, 0.5, 3), (0.5, 1.0, 0)):
        with pytest.raises(ValueError, match='a ladder has'):
            remd.temperatures(*bad)
    b = synth.qm9_batch(0, 0, 2)
    b.cell = torch.arange(18, dtype=torch.float32).reshape(2, 3, 3)
    rep = remd.replicate(b, [3, 2])
    n0, n1 = int((b.batch == 0).sum()), int((b.batch == 1).sum())
    assert rep.num_graphs == 5 and rep.ladder_ptr.tolist() == [0, 3, 5] and rep.ladder_ptr.dtype == torch.int32
    assert torch.bincount(rep.batch).tolist() == [n0] * 3 + [n1] * 2 and rep.batch.dtype == b.batch.dtype
    assert torch.equal(rep.pos, torch.cat([b.pos[:n0]] * 3 + [b.pos[n0:]] * 2)) and torch.equal(rep.x, torch.cat([b.x[:n0]] * 3 + [b.x[n0:]] * 2))
    assert torch.equal(rep.cell, b.cell[[0, 0, 0, 1, 1]]) and torch.equal(rep.y, b.y[[0, 0, 0, 1, 1]])
    e0 = b.edge_index[:, b.batch[b.edge_index[0]] == 0]
    e1 = b.edge_index[:, b.batch[b.edge_index[0]] == 1] - n0
    want = torch.cat([e0, e0 + n0, e0 + 2 * n0, e1 + 3 * n0, e1 + 3 * n0 + n1], dim=1)
    assert torch.equal(rep.edge_index, want)
    assert remd.replicate(b, 2).ladder_ptr.tolist() == [0, 2, 4]
    with pytest.raises(ValueError, match='at least once'):
        remd.replicate(b, 0)
    with pytest.raises(ValueError, match='list of num_graphs'):
        remd.replicate(b, [2])
    st = remd.new_ladder_state(kT, [0, 4, 8], 7)
    ref = new_ladder(h.kT, [0, 4, 8], [7, 8])
    for k in LADDER + ('seed',):
        assert np.array_equal(st[k].numpy(), ref[k]) and st[k].numpy().dtype == ref[k].dtype, k
    assert st['lptr'].tolist() == [0, 4, 8] and st['kT_ladder'].tolist() == h.kT.tolist() and st['kT_g'] is not st['kT_ladder']
    with pytest.raises(ValueError, match='per-ladder `exchange_seed`'):
        remd.new_ladder_state(kT, 4, torch.zeros(3, dtype=torch.int64))


# ------------------------------------------------------------------------------------------------------- kernel tests
def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _exchange_on_device(dev, c, vel=None, ladder=None, ke=None, fixed=True, n_ladders=None):
    """One launch on a case -> (vel, ladder, ke) as numpy; vel, ladder, ke: in place of the case's."""
    from pamnet_amd import remd
    ladder = c.ladder if ladder is None else ladder
    v, k = _t(dev, c.vel if vel is None else vel), _t(dev, c.ke if ke is None else ke)
    st = {key: _t(dev, ladder[key]) for key in LADDER + ('seed',)}
    st['lptr'], st['kT_ladder'] = _t(dev, c.lptr), _t(dev, c.kT)
    remd.exchange(_t(dev, c.energy), v, _t(dev, c.gptr), st, _t(dev, c.status), k, _t(dev, c.fixed.astype(np.uint8)) if fixed else None)
    return v.cpu().numpy(), {key: st[key].cpu().numpy() for key in LADDER + ('seed',)}, k.cpu().numpy()


def _assert_exchange_matches(got, want, before, c, tag=''):
    """got / want / before: (vel, ladder, ke); the checks of one launch against exchange_ref."""
    (gv, gl, gk), (wv, wl, wk), (bv, bl, bk) = got, want, before
    for key in ('rung', 'slot', 'attempts', 'tried', 'accepted', 'kT_g', 'seed'):
        assert np.array_equal(gl[key], wl[key]), (tag, key, gl[key], wl[key])
    lo = np.repeat(c.lptr[:-1], np.diff(c.lptr))
    assert np.array_equal(gl['slot'][lo + gl['rung']], np.arange(len(lo))), tag
    assert (np.abs(gk - wk) <= 1e-14 * np.abs(wk)).all(), (tag, gk, wk)
    moved = bl['rung'] != wl['rung']
    assert np.array_equal(gk[~moved], bk[~moved]), tag
    worst = 0.0
    for g in range(len(lo)):
        s = slice(int(c.gptr[g]), int(c.gptr[g + 1]))
        if not moved[g]:                          # a skipped or rejected pair, a graph that is not running, no pair: bit for bit
            assert np.array_equal(gv[s], bv[s], equal_nan=True), (tag, g)
            continue
        fx = c.fixed[s]
        assert np.array_equal(gv[s][fx], bv[s][fx]), (tag, g, 'fixed rows')
        ulps = np.abs(gv[s][~fx].astype(np.float64) - wv[s][~fx]) / np.spacing(np.abs(wv[s][~fx]))
        assert not np.array_equal(wv[s][~fx], bv[s][~fx]) and ulps.max() <= 1.0, (tag, g, ulps.max())
        worst = max(worst, float(ulps.max()))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize('parity', [0, 1])
def test_one_exchange_on_a_batch_vs_the_reference(dev, parity):
    """Ladders of 1, 2, 3, 5 and 8 rungs, graphs of 1 .. 300 atoms, some atoms fixed, a failed graph in the middle of a ladder, a
    NaN energy, attempts of the given parity, then a second attempt from the exchanged tables: rung, slot, attempts, tried,
    accepted and kT_g equal exchange_ref's, ke to 1e-14, the scaled velocities within one fp32 ulp, every row that must not change
    bit for bit, slot the inverse of rung.  fixed = NULL scales the rows the mask protected."""
    c = _kernel_case(parity)
    (v1, l1, k1, _), (v2, l2, k2, _) = _two_attempts(c)
    got1 = _exchange_on_device(dev, c)
    w1 = _assert_exchange_matches(got1, (v1, l1, k1), (c.vel, c.ladder, c.ke), c, tag=(parity, 1))
    got2 = _exchange_on_device(dev, c, *got1)
    w2 = _assert_exchange_matches(got2, (v2, l2, k2), got1, c, tag=(parity, 2))
    print('parity', parity, 'worst velocity error in ulps:', w1, w2, 'accepted', (l2['accepted'] - c.ladder['accepted']).sum())
    free = _exchange_on_device(dev, c, fixed=False)
    moved = (l1['rung'] != c.ladder['rung'])[np.repeat(np.arange(len(c.kT)), np.diff(c.gptr))]
    assert np.array_equal(free[0][~c.fixed], got1[0][~c.fixed], equal_nan=True)
    assert (free[0][c.fixed & moved] != c.vel[c.fixed & moved]).any() and np.array_equal(free[0][c.fixed & ~moved], c.vel[c.fixed & ~moved])


@pytest.mark.gpu
def test_the_cap_of_256_rungs(dev):
    """A ladder of 256 one-atom graphs runs and matches the reference under both parities; one of 257 returns PAMNET_EINVAL and
    writes nothing."""
    from pamnet_amd import lib
    for R in (256, 257):
        rng = np.random.RandomState(R)
        c = Case()
        c.lptr, c.gptr = _ptr([R]), _ptr([1] * R)
        c.kT = 0.4 * 2.5 ** (np.arange(R) / (R - 1.0))
        c.energy = rng.gamma(12.0, size=R) * c.kT
        c.vel, c.ke = rng.standard_normal((R, 3)).astype(np.float32), rng.uniform(1.0, 2.0, R)
        c.status, c.fixed = np.zeros(R, np.int32), np.zeros(R, bool)
        c.ladder = new_ladder(c.kT, c.lptr, [-3])
        if R == 256:
            before = (c.vel, c.ladder, c.ke)
            for attempt in range(2):
                info = []
                want = exchange_ref(c.energy, before[0], c.gptr, c.lptr, c.kT, before[1], c.status, before[2], c.fixed, info)
                assert all(abs(u - e) > MARGIN for _, _, d, u, e, _ in info if d < 0.0) and len(info) == 128 - attempt
                got = _exchange_on_device(dev, c, *before)
                _assert_exchange_matches(got, want, before, c, tag=(R, attempt))
                assert 0 < (want[1]['accepted'] - before[1]['accepted']).sum() <= len(info)
                before = got
        else:
            with pytest.raises(RuntimeError, match='PAMNET_EINVAL'):
                _exchange_on_device(dev, c)
            st = {k: _t(dev, c.ladder[k]) for k in LADDER + ('seed',)}
            vel, ke = _t(dev, c.vel), _t(dev, c.ke)
            args = [_t(dev, c.energy), vel, None, _t(dev, c.gptr), _t(dev, c.lptr), _t(dev, c.kT), st['kT_g'], st['rung'], st['slot'],
                    _t(dev, c.status), ke, st['seed'], st['attempts'], st['tried'], st['accepted']]
            with pytest.raises(RuntimeError, match='PAMNET_EINVAL'):
                lib.call(ENTRY, *[lib.ptr(a) for a in args], R, R, 1, lib.stream_of(vel))
            torch.cuda.synchronize()
            assert torch.equal(vel, _t(dev, c.vel)) and torch.equal(ke, _t(dev, c.ke))
            assert all(torch.equal(st[k], _t(dev, c.ladder[k])) for k in LADDER)


@pytest.mark.gpu
def test_an_exchange_is_repeatable_and_independent_of_the_batch(dev):
    """Every ladder of the kernel case alone, as the middle of three (the first and last: at the edge of two), and inside the whole
    batch, and each of these twice on fresh copies: its rows of vel, its ke and every table entry are equal bit for bit."""
    for parity in (0, 1):
        c = _kernel_case(parity)
        whole = _exchange_on_device(dev, c)
        again = _exchange_on_device(dev, c)
        assert np.array_equal(again[0], whole[0], equal_nan=True) and np.array_equal(again[2], whole[2])
        assert all(np.array_equal(again[1][k], whole[1][k]) for k in LADDER)
        for l in range(len(RUNGS)):
            g0, g1 = int(c.lptr[l]), int(c.lptr[l + 1])
            a0, a1 = int(c.gptr[g0]), int(c.gptr[g1])
            for around in (slice(l, l + 1), slice(max(l - 1, 0), min(l + 2, len(RUNGS)))):
                s = _subset(c, around)
                for _ in range(2):
                    v, st, ke = _exchange_on_device(dev, s)
                    o = int(c.lptr[around.start])
                    ao = int(c.gptr[o])
                    assert np.array_equal(v[a0 - ao:a1 - ao], whole[0][a0:a1], equal_nan=True), (parity, l, around)
                    assert np.array_equal(ke[g0 - o:g1 - o], whole[2][g0:g1])
                    for k in ('kT_g', 'rung', 'tried', 'accepted'):
                        assert np.array_equal(st[k][g0 - o:g1 - o], whole[1][k][g0:g1]), (parity, l, k)
                    assert np.array_equal(st['slot'][g0 - o:g1 - o] + o, whole[1]['slot'][g0:g1])
                    assert st['attempts'][l - around.start] == whole[1]['attempts'][l]


@pytest.mark.gpu
def test_the_decision_depends_on_seed_attempt_and_rung_only(dev):
    """64 ladders of two one-atom graphs with D = -0.8 for every pair: the accepted ladders are exchange_ref's, so the uniforms
    are those of (seed, attempt, rung) on stream 3; another seed for every ladder, or another (even) attempt count, gives the
    reference's other pattern; another seed for the odd ladders alone changes nothing of the even ones.  (The seeds of the
    dynamics are no argument of the entry point: they cannot feed the decision.)  An odd attempt count tries nothing in a ladder
    of two, and counts the attempt."""
    m = _many_pairs()

    def both(ladder):
        want = exchange_ref(m.energy, m.vel, m.gptr, m.lptr, m.kT, ladder, m.status, m.ke, m.fixed)
        got = _exchange_on_device(dev, m, ladder=ladder)
        _assert_exchange_matches(got, want, (m.vel, ladder, m.ke), m)
        return got[1]['accepted'].reshape(64, 2)[:, 0]

    base = both(m.ladder)
    reseeded = both(dict(m.ladder, seed=m.ladder['seed'] + 64))
    later = both(dict(m.ladder, attempts=np.full(64, 2, np.int32)))
    assert 16 < base.sum() < 48 and not np.array_equal(base, reseeded) and not np.array_equal(base, later)
    assert not np.array_equal(reseeded, later)
    odd = m.ladder['seed'].copy()
    odd[1::2] += 977
    mixed = both(dict(m.ladder, seed=odd))
    assert np.array_equal(mixed[0::2], base[0::2]) and not np.array_equal(mixed[1::2], base[1::2])
    idle = both(dict(m.ladder, attempts=np.full(64, 1, np.int32)))
    assert not idle.any()


@pytest.mark.gpu
def test_the_entry_point_validates_its_arguments(dev):
    """A null pointer is PAMNET_ENULL (only fixed may be NULL), a negative count PAMNET_EINVAL, before any launch; n_ladders == 0
    launches nothing: the arrays are as they were."""
    from pamnet_amd import lib
    c = _kernel_case(0)
    st = {k: _t(dev, c.ladder[k]) for k in LADDER + ('seed',)}
    t = dict(energy=_t(dev, c.energy), vel=_t(dev, c.vel), gptr=_t(dev, c.gptr), lptr=_t(dev, c.lptr), kT_ladder=_t(dev, c.kT),
             status=_t(dev, c.status), ke=_t(dev, c.ke), **st)
    order = ('energy', 'vel', 'fixed', 'gptr', 'lptr', 'kT_ladder', 'kT_g', 'rung', 'slot', 'status', 'ke', 'seed', 'attempts', 'tried',
             'accepted')

    def call(**kw):
        a = {k: lib.ptr(t[k]) if k in t else None for k in order}
        a.update(n=len(c.vel), G=len(c.kT), L=len(RUNGS))
        a.update(kw)
        lib.call(ENTRY, *[a[k] for k in order], a['n'], a['G'], a['L'], lib.stream_of(t['vel']))

    for k in order:
        if k != 'fixed':
            with pytest.raises(RuntimeError, match='PAMNET_ENULL'):
                call(**{k: None})
    for kw in (dict(n=-1), dict(G=-1), dict(L=-1), dict(G=2 ** 31), dict(L=2 ** 31), dict(G=256 * len(RUNGS) + 1)):
        with pytest.raises(RuntimeError, match='PAMNET_EINVAL'):
            call(**kw)
    call(L=0)
    call(L=0, G=0, n=0)
    torch.cuda.synchronize()
    assert torch.equal(t['vel'].nan_to_num(1.0, 2.0, 3.0), _t(dev, c.vel).nan_to_num(1.0, 2.0, 3.0)) and torch.equal(t['ke'], _t(dev, c.ke))
    assert all(torch.equal(st[k], _t(dev, c.ladder[k])) for k in LADDER)


# ----------------------------------------------------------------------------------------------------- end to end
def _replay(res, gptr, lptr, kT_ladder, dt, gamma, mass, fixed, steps, every, step_ref=None):
    """Every launch of a trace from its recorded inputs: the step launches through md_step_ref (step_ref: another reference of the
    same signature) as tests/test_md.py checks them, the exchange launches through exchange_ref with every decision more than
    MARGIN from its threshold (asserted); the flags are (1, 0) / exchange / (0, 1) on exchange steps and (1, 1) elsewhere, (0, 1)
    for the first and (1, 0) for the closing launch; consecutive launches hand on what they stored."""
    cpu = lambda t: None if t is None else t.cpu().numpy()
    want_kinds = []
    for it in range(steps + 1):
        if every and 0 < it < steps and it % every == 0:
            want_kinds += [('step', 1, 0), ('exchange',), ('step', 0, 1)]
        else:
            want_kinds.append(('step', 1 if it else 0, 1 if it < steps else 0))
    got_kinds = [(r['kind'], r['kick_in'], r['advance']) if r['kind'] == 'step' else ('exchange',) for r in res.trace]
    assert got_kinds == want_kinds
    fx = np.zeros(int(gptr[-1]), bool) if fixed is None else fixed
    worst, kT_now, decisions = [0.0, 0.0, 0.0], kT_ladder, 0
    c = Case()
    c.gptr, c.lptr, c.fixed = gptr, lptr, fx
    for i, r in enumerate(res.trace):
        if r['kind'] == 'step':
            assert np.array_equal(cpu(r['kT']), kT_now), i
            before = (cpu(r['pos']), cpu(r['v_before']), {k: cpu(v) for k, v in r['state_before'].items()})
            got = (cpu(r['pos_after']), cpu(r['v_after']), {k: cpu(v) for k, v in r['state_after'].items()})
            if step_ref is None:
                want = md_step_ref(before[0], before[1], cpu(r['dE']), gptr, before[2], dt, kT_now, gamma, mass, fixed, r['kick_in'],
                                   r['advance'])
                w = _assert_step_matches(got, want, before, gptr, fx, r['advance'], tag=i)
            else:
                w = step_ref(got, before, cpu(r['dE']), kT_now, r['kick_in'], r['advance'], i)
            worst[:2] = [max(worst[0], w[0]), max(worst[1], w[1])]
            v_out = r['v_after']
        else:
            before = (cpu(r['v_before']), dict({k: cpu(v) for k, v in r['ladder_before'].items()}, seed=cpu(res.exchange_seed)),
                      cpu(r['ke_before']))
            got = (cpu(r['v_after']), dict({k: cpu(v) for k, v in r['ladder_after'].items()}, seed=before[1]['seed']), cpu(r['ke_after']))
            info = []
            want = exchange_ref(cpu(r['energy']), before[0], gptr, lptr, kT_ladder, before[1], cpu(r['status']), before[2], fx, info)
            assert all(abs(u - e) > MARGIN for _, _, d, u, e, _ in info if d < 0.0), i
            decisions += len(info)
            worst[2] = max(worst[2], _assert_exchange_matches(got, want, before, c, tag=i))
            assert np.array_equal(cpu(r['energy']), cpu(res.trace[i - 1]['energy']).reshape(-1).astype(np.float64))
            assert torch.equal(r['ke_before'], res.trace[i - 1]['state_after']['ke'])
            assert torch.equal(r['ke_after'], res.trace[i + 1]['state_before']['ke'])
            assert torch.equal(res.trace[i - 1]['dE'], res.trace[i + 1]['dE'])                     # the same forces open the next step
            kT_now = got[1]['kT_g']
            v_out = r['v_after']
        if i + 1 < len(res.trace):
            assert torch.equal(v_out, res.trace[i + 1]['v_before']), i
    assert torch.equal(res.trace[-1]['pos_after'], res.pos) and torch.equal(res.trace[-1]['v_after'], res.vel)
    assert torch.equal(res.trace[-1]['state_after']['ke'], res.kinetic) and np.array_equal(cpu(res.kT), kT_now)
    return worst, decisions


def _well_on(dev, h, graphs=slice(0, 8)):
    from pamnet_amd import synth
    a = slice(int(h.gptr[graphs.start]), int(h.gptr[graphs.stop]))
    model = Harmonic(torch.from_numpy(h.k[graphs]), torch.from_numpy(h.x0[a])).to(dev)
    data = synth.Batch(pos=torch.from_numpy(h.x0[a]), batch=torch.from_numpy(h.batch[a] - graphs.start),
                       num_graphs=graphs.stop - graphs.start).to(dev)
    return model, data


@pytest.mark.gpu
def test_ladders_of_harmonic_wells(dev):
    """Two ladders x 4 replicas of an 8-atom well (d = 24, k = 2, unit masses), kT = (0.4, 0.55, 0.75, 1.0), gamma = 2, dt = 0.05,
    exchange_every = 10, 8000 steps (see the CPU test for why not 2000), a record every 10, per-graph and per-ladder seed tensors,
    started at the minimum with Maxwell-Boltzmann velocities (remove_com False, as the reference run):
    (a) the same run over 200 steps with trace=True, replayed launch by launch: step launches through md_step_ref within KTOL,
        exchange launches through exchange_ref with equal tables (every decision is more than 1e-9 from its threshold: asserted),
        the flags (1, 0) / exchange / (0, 1) on exchange steps and (1, 1) elsewhere; its records are the long run's first;
    (b) by_rung(epot) averaged over the second half of the records and the two ladders is 12 kT_r on every rung within b_gpu =
        5 % = 2 b_ref; the reference's own worst deviation is 2.03 %, asserted within b_ref = 2.5 % by
        test_the_reference_ladders_sample_their_temperatures;
    (c) tried of pair r is the number of attempts of its parity, 0 <= accepted <= tried, every row of rungs is a permutation per
        ladder, by_rung undoes frame_rung for per-graph and per-atom records;
    (d) ladder 0 run alone with its seeds is bitwise its part of the batch run in pos, vel, rungs, epot and ekin;
    (e) under torch's synchronisation debug mode the long run synchronises once: the set-up read."""
    from pamnet_amd import remd
    h = _wells()
    model, data = _well_on(dev, h)
    kT, seeds, xseeds = _t(dev, h.kT), _t(dev, h.seeds), _t(dev, h.xseeds)
    kw = dict(dt=H_DT, replicas=4, exchange_every=H_EVERY, gamma=H_GAMMA, remove_com=False)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        torch.cuda.set_sync_debug_mode('warn')
        try:
            res = remd.run(model, data, H_STEPS, kT=kT, seed=seeds, exchange_seed=xseeds, record_every=H_REC, **kw)
        finally:
            torch.cuda.set_sync_debug_mode('default')
    syncs = [str(w.message) for w in caught if 'called a synchronizing' in str(w.message)]
    print('synchronisations of the long run:', syncs)
    assert len(syncs) == 1                                                                            # (e)
    assert res.steps.tolist() == [H_STEPS] * 8 and not res.failed.any() and res.trace is None
    assert torch.equal(data.pos.cpu(), torch.from_numpy(h.x0))
    # (a)
    short = remd.run(model, data, H_TRACED, kT=kT, seed=seeds, exchange_seed=xseeds, record_every=H_REC, trace=True, **kw)
    worst, decisions = _replay(short, h.gptr, h.lptr, h.kT, H_DT, H_GAMMA, None, None, H_TRACED, H_EVERY)
    print('wells: worst vel / displacement error of the replay, worst exchange ulps', worst, 'decisions replayed', decisions)
    assert decisions == sum(2 if a % 2 == 0 else 1 for a in range((H_TRACED - 1) // H_EVERY)) * 2
    F = H_TRACED // H_REC
    for k in ('frames', 'epot', 'ekin', 'frame_rung'):
        assert torch.equal(getattr(short, k)[:F], getattr(res, k)[:F]), k
    assert torch.equal(short.rungs, res.rungs[:short.rungs.size(0)])
    # (b)
    epot, frame_rung = res.epot.cpu().numpy(), res.frame_rung.cpu().numpy()
    by = res.by_rung(res.epot)
    dev_ = _rung_means(epot, frame_rung)
    half = by[by.size(0) // 2:].cpu().numpy()
    assert np.allclose(half.reshape(len(half), 2, 4).mean((0, 1)) / (12.0 * np.asarray(KT4)) - 1.0, dev_, rtol=0, atol=1e-12)
    print('wells: relative deviation of <epot> per rung', dev_, 'acceptance', res.acceptance().tolist())
    assert np.abs(dev_).max() <= B_GPU
    # (c)
    A = (H_STEPS - 1) // H_EVERY
    assert res.attempts.tolist() == [A, A] and tuple(res.rungs.shape) == (A + 1, 8) and res.rungs.dtype == torch.int32
    assert res.tried.tolist() == [(A + 1) // 2, A // 2, (A + 1) // 2, 0] * 2
    assert ((res.accepted >= 0) & (res.accepted <= res.tried)).all() and int(res.accepted.sum()) > 0
    assert (np.sort(res.rungs.cpu().numpy().reshape(-1, 2, 4), axis=2) == np.arange(4)).all()
    assert torch.equal(res.rungs[-1], res.rung) and torch.equal(res.kT, kT[(res.lptr[:-1].long().repeat_interleave(4) + res.rung.long())])
    assert torch.equal(res.slot[(res.lptr[:-1].long().repeat_interleave(4) + res.rung.long())].cpu(), torch.arange(8, dtype=torch.int32))
    acc = res.acceptance()
    assert torch.isnan(acc[[3, 7]]).all() and torch.equal(acc[:3], res.accepted[:3].double() / res.tried[:3].double())
    first = np.repeat([0, 4], 4)
    f = int(np.nonzero((frame_rung != frame_rung[0]).sum(1) >= 4)[0][0])        # a record with both ladders out of order
    frames_by = res.by_rung(res.frames)
    for g in range(8):
        dest = first[g] + frame_rung[f, g]
        assert by[f, dest] == res.epot[f, g]
        assert torch.equal(frames_by[f, 8 * dest:8 * dest + 8], res.frames[f, 8 * g:8 * g + 8])
    # (d)
    m0, d0 = _well_on(dev, h, slice(0, 4))
    alone = remd.run(m0, d0, H_STEPS, kT=kT[:4].contiguous(), seed=seeds[:4].contiguous(), exchange_seed=xseeds[:1].contiguous(),
                     record_every=H_REC, **kw)
    assert torch.equal(alone.pos, res.pos[:32]) and torch.equal(alone.vel, res.vel[:32])
    assert torch.equal(alone.rungs, res.rungs[:, :4]) and torch.equal(alone.epot, res.epot[:, :4])
    assert torch.equal(alone.ekin, res.ekin[:, :4]) and torch.equal(alone.accepted, res.accepted[:4])


@pytest.mark.gpu
def test_without_exchanges_the_run_is_md_run(dev):
    """exchange_every = 0: pos, vel, kinetic and steps are md.run's bit for bit, with the same seeds and the per-graph kT; no
    exchange was launched."""
    from pamnet_amd import md, remd
    h = _wells()
    model, data = _well_on(dev, h)
    kT, seeds = _t(dev, h.kT), _t(dev, h.seeds)
    want = md.run(model, data, 60, H_DT, kT=kT, gamma=H_GAMMA, seed=seeds, record_every=20)
    got = remd.run(model, data, 60, H_DT, kT=kT, replicas=4, exchange_every=0, gamma=H_GAMMA, seed=seeds, record_every=20)
    for k in ('pos', 'vel', 'kinetic', 'steps', 'energy', 'forces', 'frames', 'epot', 'ekin'):
        assert torch.equal(getattr(want, k), getattr(got, k)), k
    assert got.attempts.tolist() == [0, 0] and tuple(got.rungs.shape) == (1, 8) and not got.tried.any()
    assert torch.equal(got.kT, kT) and got.kT is not kT


_MASS_OF_TYPE = (1.008, 12.011, 14.007, 15.999, 18.998)            # H, C, N, O, F (the QM9 schema's type index)


@pytest.mark.gpu
@pytest.mark.parametrize('dim,n_layer', MODELS)
def test_pamnet_ladders_replayed_launch_by_launch(dev, dim, n_layer):
    """PAMNet on remd.replicate of two QM9-schema molecules into ladders of 3 (kT = 0.03 .. 0.05), 12 steps, exchange_every = 4,
    trace=True, replicas from the batch's ladder_ptr: every launch replayed as in the wells test (two exchange launches, four
    pairs decided); the first evaluation gives the copies of a molecule the same energy (to 1e-5 relative: fp32 sums over the
    same atoms at other places of the batch); res.energy is a fresh evaluation at res.pos."""
    import copy
    import models
    from pamnet_amd import remd, synth
    b = synth.qm9_batch(0, 0, 2)
    rep = remd.replicate(b, 3)
    torch.manual_seed(0)
    model = models.PAMNet(models.Config(dataset='QM9', dim=dim, n_layer=n_layer, cutoff_l=5.0, cutoff_g=5.0)).to(dev)
    data = rep.to(dev)
    mass_cpu = torch.tensor(_MASS_OF_TYPE, dtype=torch.float32)[rep.x.long()]
    kT = remd.temperatures(0.03, 0.05, 3).repeat(2)
    seeds = torch.tensor([11, -5, 2 ** 40 + 3, 7, 8, 9], dtype=torch.int64, device=dev)
    xseeds = torch.tensor([3, -2 ** 50], dtype=torch.int64, device=dev)
    res = remd.run(model, data, 12, 0.05, kT=kT.to(dev), exchange_every=4, gamma=1.0, masses=mass_cpu.to(dev), seed=seeds,
                   exchange_seed=xseeds, trace=True)
    assert res.steps.tolist() == [12] * 6 and not res.failed.any() and res.attempts.tolist() == [2, 2]
    assert res.lptr.tolist() == [0, 3, 6] and tuple(res.rungs.shape) == (3, 6)
    gptr = np.concatenate([[0], np.cumsum(np.bincount(rep.batch.numpy(), minlength=6))])
    worst, decisions = _replay(res, gptr, np.array([0, 3, 6]), kT.numpy(), 0.05, 1.0, mass_cpu.numpy(), None, 12, 4)
    print('PAMNet ladders: replay', worst, 'decisions', decisions, 'accepted', res.accepted.tolist())
    assert decisions == 4 and res.tried.tolist() == [1, 1, 0, 1, 1, 0]
    e0 = res.trace[0]['energy'].reshape(2, 3).double()
    print('first evaluation:', e0.tolist())
    assert (e0 - e0[:, :1]).abs().max() <= 1e-5 * e0.abs().max()
    at = copy.copy(data)
    at.pos = res.pos.clone().requires_grad_(True)
    e = model(at)
    assert torch.equal(res.energy, e.detach())


def _ethane():
    """An ethane-like molecule, X-H bonds of 0.9 and an X-X bond of 1.5, every coordinate below 2 in magnitude: (pos [8, 3], types
    (0 = H), bonds)."""
    t = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]) / np.sqrt(3.0)
    axis = t[3]
    c1, c2 = np.zeros(3), 1.5 * axis
    pos = np.concatenate([[c1], c1 + 0.9 * t[:3], [c2], c2 - 0.9 * np.array([[1, 1, -1 / 3.0], [1, -1 / 3.0, 1], [-1 / 3.0, 1, 1]])
                          / np.sqrt(19.0 / 9.0)])
    bonds = [(0, 1), (0, 2), (0, 3), (0, 4), (4, 5), (4, 6), (4, 7)]
    return pos - pos.mean(0), np.array([1, 0, 0, 0, 1, 0, 0, 0], np.float32), bonds


CONS_TOL = 1e-5


@pytest.mark.gpu
def test_a_constrained_ladder_keeps_its_bonds(dev):
    """A ladder of 3 replicas of an ethane-like molecule in a harmonic well (k = 4) with its six X-H bonds constrained at 0.9,
    kT = (0.5, 0.55, 0.6), gamma = 2, dt = 0.05, 60 steps, exchange_every = 5, constraint_tol = 1e-5: at least one exchange is
    accepted, nothing is unconverged, every constrained length is within constraint_tol of 0.9 -- the solve's relative bound gives
    0.9e-5, the fp32 storage of coordinates below 4 (asserted) at most 8.3e-7 more -- and the velocity along every constraint is zero to the
    bound of tests/test_md_constraints.py (1e-5 of the largest relative velocity).  Replicas with unequal constraint counts are
    refused by the set-up read."""
    from pamnet_amd import md, remd, synth
    pos, types, bonds = _ethane()
    assert np.abs(pos).max() < 2.0
    ei = np.array(bonds + [(b, a) for a, b in bonds], dtype=np.int64).T
    one = synth.Batch(pos=torch.from_numpy(pos.astype(np.float32)), x=torch.from_numpy(types), batch=torch.zeros(8, dtype=torch.int64),
                      edge_index=torch.from_numpy(ei), num_graphs=1)
    data = remd.replicate(one, 3).to(dev)
    pairs = md.bond_constraints(data.edge_index, data.x == 0)
    cons = md.Constraints(data, pairs, torch.full((len(pairs),), 0.9, dtype=torch.float64, device=dev))
    assert cons.n == 18 and cons.n_per_graph.tolist() == [6, 6, 6]
    rng = np.random.RandomState(8)
    x0 = np.tile(pos + rng.uniform(-0.2, 0.2, pos.shape), (3, 1)).astype(np.float32)
    model = Harmonic(torch.full((3,), 4.0), torch.from_numpy(x0)).to(dev)
    mass = torch.tensor([1.008, 12.011])[data.x.long().cpu()].to(dev)
    kT = torch.tensor([0.5, 0.55, 0.6], dtype=torch.float64, device=dev)
    res = remd.run(model, data, 60, 0.05, kT=kT, exchange_every=5, gamma=2.0, masses=mass, seed=3, exchange_seed=5, constraints=cons,
                   constraint_tol=CONS_TOL)
    print('constrained ladder: tried', res.tried.tolist(), 'accepted', res.accepted.tolist(), 'sweeps', res.sweeps.tolist())
    assert res.steps.tolist() == [60] * 3 and not res.failed.any() and not res.unconverged.any()
    assert res.attempts.tolist() == [11] and int(res.accepted.sum()) >= 1
    p, v = res.pos.cpu().numpy().astype(np.float64), res.vel.cpu().numpy().astype(np.float64)
    i, j = cons.i.cpu().numpy(), cons.j.cpu().numpy()
    r, u = p[i] - p[j], v[i] - v[j]
    d = np.sqrt((r * r).sum(1))
    print('constrained ladder: largest |d - 0.9|', np.abs(d - 0.9).max(), 'largest r.u', np.abs((r * u).sum(1)).max(), 'of', np.abs(u).max())
    assert np.abs(d - 0.9).max() <= CONS_TOL and np.abs(p).max() < 4.0
    assert np.abs((r * u).sum(1)).max() <= 1e-5 * np.abs(u).max()
    fewer = md.Constraints(data, pairs[:-1], torch.full((len(pairs) - 1,), 0.9, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError, match='same number of constraints'):
        remd.run(model, data, 5, 0.05, kT=kT, exchange_every=5, gamma=2.0, masses=mass, constraints=fewer)


@pytest.mark.gpu
def test_run_refuses_bad_ladders_on_the_device(dev):
    """The set-up read refuses replicas of a ladder with other atom counts or other atom types, and a kT / gamma entry that is not
    positive; tensors on the wrong device or of the wrong shape are refused before it."""
    from pamnet_amd import remd, synth
    h = _wells()
    model, data = _well_on(dev, h)
    kT = _t(dev, h.kT)
    ok = dict(steps=3, dt=H_DT, kT=kT, replicas=4, exchange_every=2, gamma=H_GAMMA)
    data.x = torch.arange(8, device=dev).repeat(8).float()
    assert remd.run(model, data, **ok).steps.tolist() == [3] * 8
    other = synth.Batch(pos=data.pos, batch=data.batch, num_graphs=8, x=data.x.clone())
    other.x[13] = 9.0
    with pytest.raises(ValueError, match='must hold the same atoms'):
        remd.run(model, other, **ok)
    moved = data.batch.clone()
    moved[8] = 0                                                   # graphs of 9 and 7 atoms in ladder 0
    uneven = synth.Batch(pos=data.pos, batch=moved, num_graphs=8)
    with pytest.raises(ValueError, match='must hold the same atoms'):
        remd.run(Harmonic(model.k, model.x0), uneven, **ok)
    f64 = lambda *v: torch.tensor(v, dtype=torch.float64, device=dev)
    bad = kT.clone()
    bad[5] = 0.0
    cases = [(dict(kT=bad), '`kT` must be finite and positive'), (dict(kT=-kT), '`kT` must be'),
             (dict(gamma=f64(2, 2, 0, 2, 2, 2, 2, 2)), '`gamma` must be finite and positive'), (dict(kT=kT.cpu()), 'per-graph `kT`'),
             (dict(gamma=f64(1, 2)), 'per-graph `gamma`'),
             (dict(exchange_seed=torch.zeros(3, dtype=torch.int64, device=dev)), 'per-ladder `exchange_seed`'),
             (dict(exchange_seed=torch.zeros(2, dtype=torch.int32, device=dev)), 'per-ladder `exchange_seed`'),
             (dict(exchange_seed='x'), '`exchange_seed` is an int')]
    for kw, match in cases:
        args = dict(ok)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            remd.run(model, data, **args)
