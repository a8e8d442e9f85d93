"""fire_step_ref: the FIRE step of pamnet_fire_step_f32 (include/pamnet_hip.h) restated in numpy, fp64 -- the reference of
tests/test_relax.py.  Per graph g, every sum and maximum over the free atoms of g, f = -dE/dpos:

  1. status[g] != 0: g is left alone.
  2. F2 = sum |f|^2, fm = max |f| (numpy's maximum: a NaN propagates); fmax[g] = fm.  F2 not finite: status[g] = 2, nothing
     else changes.  Else fm < tolerance: status[g] = 1, nothing else changes (no free atoms: fm = 0).
  3. P = sum f.v, V2 = sum |v|^2.  V2 == 0: nothing.  Else P > 0: n_pos += 1; if n_pos > n_min: dt = min(dt f_inc, dt_max),
     a *= f_a; then v <- (1 - a) v + a sqrt(V2 / F2) f.  Else: v <- 0, a = a0, dt *= f_dec, n_pos = 0.
  4. v <- v + dt f.
  5. dr = dt v, s = min(1, max_step / max |dr|) (1 where the maximum is 0), pos <- pos + s dr; v is not scaled.
  6. steps[g] += 1.

THE ORDER (as the header states it): n_pos, dt and a are updated first, the mixing of step 3 uses the updated a, steps 4 and 5
the updated dt.  fp64 from the fp32 inputs, one rounding to fp32 where pos and vel are stored; fixed atoms are skipped."""
import numpy as np

STATE = ('dt', 'a', 'n_pos', 'steps', 'status', 'fmax')


def fire_step_ref(pos, vel, dE, gptr, state, fmax_tol, fixed=None, dt_max=1.0, max_step=0.2, n_min=5, f_inc=1.1, f_dec=0.5,
                  a0=0.1, f_a=0.99, diag=None):
    """pos, vel, dE: float32 [n, 3]; gptr: [G + 1]; state: dict of dt, a (float64), n_pos, steps, status (int32), fmax (float32),
    each [G]; fmax_tol: a float or [G]; fixed: bool [n] or None.  Returns new (pos, vel, state); the inputs are not modified.
    diag: a dict that receives, per graph, the quantities the branches compare (None for a graph that was left alone)."""
    pos, vel = np.array(pos, dtype=np.float32), np.array(vel, dtype=np.float32)
    dE = np.asarray(dE, dtype=np.float32)
    n, G = pos.shape[0], len(gptr) - 1
    st = {k: np.array(state[k]) for k in STATE}
    assert st['dt'].dtype == np.float64 and st['a'].dtype == np.float64 and st['fmax'].dtype == np.float32
    fixed = np.zeros(n, dtype=bool) if fixed is None else np.asarray(fixed).astype(bool)
    tol = np.broadcast_to(np.asarray(fmax_tol, dtype=np.float64), (G,))
    for g in range(G):
        rec = None
        if diag is not None:
            diag[g] = None
        if st['status'][g] != 0:                                               # 1
            continue
        lo, hi = max(int(gptr[g]), 0), min(int(gptr[g + 1]), n)
        free = np.arange(lo, max(hi, lo))
        free = free[~fixed[free]]
        f, v = -dE[free].astype(np.float64), vel[free].astype(np.float64)
        with np.errstate(all='ignore'):
            f2 = (f * f).sum(1)
            F2 = float(f2.sum())                                               # 2
            fm = float(np.sqrt(f2.max())) if free.size else 0.0
            st['fmax'][g] = np.float32(fm)
        if diag is not None:
            rec = diag[g] = dict(F2=F2, fm=fm, tol=float(tol[g]))
        if not np.isfinite(F2):
            st['status'][g] = 2
            continue
        if fm < tol[g]:
            st['status'][g] = 1
            continue
        P, V2 = float((f * v).sum()), float((v * v).sum())                     # 3
        dt, a, n_pos = float(st['dt'][g]), float(st['a'][g]), int(st['n_pos'][g])
        if rec is not None:
            rec.update(P=P, V2=V2, dt_in=dt, n_pos_in=n_pos)
        if V2 == 0.0:
            pass
        elif P > 0.0:
            n_pos += 1
            if n_pos > n_min:
                dt = min(dt * f_inc, dt_max)
                a *= f_a
            v = (1.0 - a) * v + a * np.sqrt(V2 / F2) * f
        else:
            v = np.zeros_like(v)
            a = a0
            dt *= f_dec
            n_pos = 0
        v = v + dt * f                                                         # 4
        dr = dt * v                                                            # 5
        m = float(np.sqrt((dr * dr).sum(1).max())) if free.size else 0.0
        s = 1.0 if m == 0.0 else min(1.0, max_step / m)
        if rec is not None:
            rec.update(max_dr=m)
        pos[free] = (pos[free].astype(np.float64) + s * dr).astype(np.float32)
        vel[free] = v.astype(np.float32)
        st['dt'][g], st['a'][g], st['n_pos'][g] = dt, a, n_pos
        st['steps'][g] += 1                                                    # 6
    return pos, vel, st
