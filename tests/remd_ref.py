"""The rule of pamnet_remd_exchange_f64 (include/pamnet_hip.h) restated in numpy, fp64 -- the reference of tests/test_remd.py --
and remd_run_ref, the driver's launch sequence over md_step_ref.

exchange_ref, per ladder l (lo = lptr[l], R rungs, a = attempts[l], p = a & 1):
  1. every r = p (mod 2) with r + 1 < R: i = slot[lo + r], j = slot[lo + r + 1]; status[i] or status[j] != 0, or a non-finite
     energy: the pair is skipped.
  2. D = (1 / kT_r - 1 / kT_{r+1}) (E_i - E_j); tried[lo + r] += 1; accept if D >= 0 or u < exp(D), u = (x0 + 0.5) 2^-32 of
     Philox4x32-10 keyed by the two halves of seed[l] on the counter (r, a, 3, 0).
  3. accepted: slot entries swapped, rung[i] = r + 1, rung[j] = r, kT_g[i] = kT_{r+1}, kT_g[j] = kT_r, accepted[lo + r] += 1,
     free velocities of i times sqrt(kT_{r+1} / kT_r), of j times sqrt(kT_r / kT_{r+1}) (fp64 on the fp32 value, one rounding),
     ke[i] *= kT_{r+1} / kT_r, ke[j] *= kT_r / kT_{r+1}.
  4. attempts[l] += 1."""
import numpy as np

from md_ref import md_step_ref, philox4x32

LADDER = ('kT_g', 'rung', 'slot', 'attempts', 'tried', 'accepted')
STREAM = 3
MAX_RUNGS = 256


def uniform(seed, rungs, attempt):
    """u of the pairs `rungs` (an int array) of a ladder with `seed` at its attempt `attempt`: float64, inside (0, 1)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x = philox4x32((np.asarray(rungs, dtype=np.uint64), int(attempt) & 0xFFFFFFFF, STREAM, 0), (seed & 0xFFFFFFFF, seed >> 32))
    return (x[0].astype(np.float64) + 0.5) * 2.0 ** -32


def new_ladder(kT, lptr, seed):
    """The ladder state at the start: every graph on the rung of its place.  seed: int64 [L]."""
    kT, lptr = np.asarray(kT, dtype=np.float64), np.asarray(lptr, dtype=np.int64)
    G, L = len(kT), len(lptr) - 1
    lo = np.repeat(lptr[:-1], np.diff(lptr))
    return dict(kT_g=kT.copy(), rung=(np.arange(G) - lo).astype(np.int32), slot=np.arange(G, dtype=np.int32),
                attempts=np.zeros(L, np.int32), tried=np.zeros(G, np.int32), accepted=np.zeros(G, np.int32),
                seed=np.asarray(seed, dtype=np.int64))


def exchange_ref(energy, vel, gptr, lptr, kT_ladder, ladder, status, ke, fixed=None, info=None):
    """energy: float64 [G]; vel: float32 [n, 3]; ladder: dict of kT_g (float64), rung, slot, tried, accepted (int32) [G], attempts
    (int32) and seed (int64) [L].  Returns new (vel, ladder, ke); the inputs are not modified.  info: a list that receives, per
    tried pair, (ladder, r, D, u, exp(D), accepted)."""
    energy, kT_ladder = np.asarray(energy, dtype=np.float64), np.asarray(kT_ladder, dtype=np.float64)
    vel, ke = np.array(vel, dtype=np.float32), np.array(ke, dtype=np.float64)
    st = {k: np.array(ladder[k]) for k in LADDER}
    st['seed'] = np.array(ladder['seed'], dtype=np.int64)
    assert st['kT_g'].dtype == np.float64 and all(st[k].dtype == np.int32 for k in LADDER[1:])
    n = len(vel)
    fixed = np.zeros(n, dtype=bool) if fixed is None else np.asarray(fixed).astype(bool)
    for l in range(len(lptr) - 1):
        lo, hi = int(lptr[l]), int(lptr[l + 1])
        R, a = hi - lo, int(st['attempts'][l])
        assert R <= MAX_RUNGS
        for r in range(a & 1, R - 1, 2):
            i, j = int(st['slot'][lo + r]), int(st['slot'][lo + r + 1])
            if status[i] != 0 or status[j] != 0 or not (np.isfinite(energy[i]) and np.isfinite(energy[j])):     # 1
                continue
            kr, kq = kT_ladder[lo + r], kT_ladder[lo + r + 1]
            delta = (1.0 / kr - 1.0 / kq) * (energy[i] - energy[j])                                          # 2
            st['tried'][lo + r] += 1
            u = float(uniform(st['seed'][l], [r], a)[0])
            with np.errstate(over='ignore'):
                accept = bool(delta >= 0.0 or u < np.exp(delta))
                if info is not None:
                    info.append((l, r, float(delta), u, float(np.exp(delta)), accept))
            if not accept:
                continue
            st['slot'][lo + r], st['slot'][lo + r + 1] = j, i                                                 # 3
            st['rung'][i], st['rung'][j] = r + 1, r
            st['kT_g'][i], st['kT_g'][j] = kq, kr
            st['accepted'][lo + r] += 1
            for g, s in ((i, np.sqrt(kq / kr)), (j, np.sqrt(kr / kq))):
                rows = np.arange(int(gptr[g]), int(gptr[g + 1]))
                rows = rows[~fixed[rows]]
                vel[rows] = (vel[rows].astype(np.float64) * s).astype(np.float32)
            ke[i] *= kq / kr
            ke[j] *= kr / kq
        st['attempts'][l] = a + 1                                                                             # 4
    return vel, st, ke


def exchange_many_ref(energy, kT, seeds, attempt):
    """The decisions of exchange_ref for L ladders that share the temperatures kT [R], every graph running and on the rung of its
    place, vectorised: energy float64 [L, R] by rung, seeds int64 [L], one attempt count for all.  Returns (the energies by rung
    after the exchange [L, R], accepted bool [L, P], the rungs r of the P pairs)."""
    energy, kT = np.asarray(energy, dtype=np.float64), np.asarray(kT, dtype=np.float64)
    L, R = energy.shape
    rungs = np.arange(int(attempt) & 1, R - 1, 2)
    s = np.asarray(seeds, dtype=np.int64).astype(np.uint64)
    out, accepted = energy.copy(), np.zeros((L, len(rungs)), dtype=bool)
    for k, r in enumerate(rungs):
        c = [np.full(L, r, np.uint64), np.full(L, int(attempt) & 0xFFFFFFFF, np.uint64), np.full(L, STREAM, np.uint64),
             np.zeros(L, np.uint64)]
        k0, k1 = s & np.uint64(0xFFFFFFFF), s >> np.uint64(32)
        m = np.uint64(0xFFFFFFFF)
        for _ in range(10):                        # (philox4x32 of md_ref.py takes one key; here every ladder has its own)
            p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
            c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m]
            k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m, (k1 + np.uint64(0xBB67AE85)) & m
        u = (c[0].astype(np.float64) + 0.5) * 2.0 ** -32
        delta = (1.0 / kT[r] - 1.0 / kT[r + 1]) * (energy[:, r] - energy[:, r + 1])
        with np.errstate(over='ignore'):
            acc = (delta >= 0.0) | (u < np.exp(delta))
        accepted[:, k] = acc
        out[acc, r], out[acc, r + 1] = energy[acc, r + 1], energy[acc, r]
    return out, accepted, rungs


def remd_run_ref(grad, pos, vel, gptr, lptr, state, ladder, steps, dt, kT_ladder, gamma, exchange_every, mass=None, fixed=None,
                 record_every=0):
    """The launch sequence of pamnet_amd.remd.run over md_step_ref and exchange_ref.  grad(pos) -> (energy float64 [G], dE float32
    [n, 3]).  Step `it` is an exchange step where exchange_every > 0, it > 0 and it % exchange_every == 0: (kick_in 1, advance
    0), the exchange, (kick_in 0, advance 1) on the same forces; every other step is one launch (kick_in = 0 for the first).  One
    more evaluation and a closing launch end the run.  Returns dict(pos, vel, state, ladder, epot, ekin, frame_rung, rungs): the
    records are taken as the driver takes them (positions and energies before the launches of the step, ke after the closing
    launch and before the exchange, the rungs before the exchange)."""
    pos, vel = np.array(pos, dtype=np.float32), np.array(vel, dtype=np.float32)
    epot, ekin, frame_rung, rungs = [], [], [], [ladder['rung'].copy()]
    for it in range(steps + 1):
        e, dE = grad(pos)
        last = it == steps
        swap = bool(exchange_every) and it > 0 and it % exchange_every == 0 and not last
        rec = record_every and it % record_every == 0
        if rec:
            epot.append(np.array(e, dtype=np.float64))
            frame_rung.append(ladder['rung'].copy())
        if swap:
            pos, vel, state = md_step_ref(pos, vel, dE, gptr, state, dt, ladder['kT_g'], gamma, mass, fixed, 1, 0)
            if rec:
                ekin.append(state['ke'].copy())
            vel, ladder, ke = exchange_ref(e, vel, gptr, lptr, kT_ladder, ladder, state['status'], state['ke'], fixed)
            state = dict(state, ke=ke)
            rungs.append(ladder['rung'].copy())
            pos, vel, state = md_step_ref(pos, vel, dE, gptr, state, dt, ladder['kT_g'], gamma, mass, fixed, 0, 1)
        else:
            pos, vel, state = md_step_ref(pos, vel, dE, gptr, state, dt, ladder['kT_g'], gamma, mass, fixed, 1 if it else 0,
                                          0 if last else 1)
            if rec:
                ekin.append(state['ke'].copy())
    return dict(pos=pos, vel=vel, state=state, ladder=ladder, epot=np.array(epot), ekin=np.array(ekin),
                frame_rung=np.array(frame_rung), rungs=np.array(rungs))
