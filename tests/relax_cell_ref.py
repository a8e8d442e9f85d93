"""fire_cell_step_ref: the variable-cell FIRE step of pamnet_fire_cell_step_f32 (include/pamnet_hip.h) restated in numpy, fp64 --
the reference of tests/test_relax_cell.py.  Row-vector convention: pos -> pos (I + eps), cell -> cell (I + eps).  Per graph g a
reference cell cell0, a deformation gradient F (the current cell is cell0 F), generalised atom coordinates x~ = pos F^-1 and the
generalised cell coordinate L F; vel holds the generalised atom velocities, vcell those of L F.  For a running graph with
cell_dof != 0, "free" = not fixed, f = -dE/dpos, W = dE/d eps:

  1. V = |det(cell0 F)|; S = (W + W^T) / 2 + p V I; hydrostatic: S <- (tr S / 3) I; sm = max |S_ij| / V.
  2. fm = max |f|; g_a = f_a F^T; g_c = -(F^-T S) / L.
  3. F2 = sum |g_a|^2 + sum g_c^2.  F2 or V not finite or V == 0: status = 2, fmax = sqrt(F2), smax = sm, nothing else.
     fm < fmax_tol and sm < smax_tol: status = 1, fmax = fm, smax = sm, nothing else.
  4. P = sum g_a . v~_a + sum g_c v_c, V2 likewise; the FIRE decision of relax_ref.fire_step_ref (n_pos, dt, a first).
  5. v~ <- (c_v v~ + c_f g) + dt g for atom rows and the three cell rows.
  6. s = min(1, max_step / m), m the largest norm among the rows dt v~_a (free atoms) and the three rows of dt v_c.
  7. F_new = F + s dt v_c / L; det F_new not positive and finite: status = 2, fmax = fm, smax = sm, nothing else.
  8. D = F^-1 F_new.
  9. pos_a <- pos_a D for every atom, + s dt v~_a F_new for a free one; vel <- v~ (free atoms only).
 10. cell = fp32(cell0 F_new), F = F_new, vcell = v_c, steps += 1; fmax = fm, smax = sm, dt, a, n_pos.

A graph with cell_dof == 0 is handed to fire_step_ref: the fixed-cell rule, its cell, F, vcell and smax untouched.
fp64 from the fp32 inputs, one rounding to fp32 where pos, vel, cell, fmax and smax are stored."""
import numpy as np

from relax_ref import STATE, fire_step_ref

CELL_STATE = STATE + ('smax',)


def stress_terms(W, cell0, F, L, p, hydrostatic):
    """(V, S, sm, g_c) of steps 1 and 2 for one graph, fp64."""
    W, cell0, F = np.asarray(W, np.float64).reshape(3, 3), np.asarray(cell0, np.float64).reshape(3, 3), np.asarray(F).reshape(3, 3)
    with np.errstate(all='ignore'):
        V = abs(float(np.linalg.det(cell0 @ F))) if np.isfinite(cell0).all() and np.isfinite(F).all() else np.nan
        S = 0.5 * (W + W.T) + p * V * np.eye(3)
        if hydrostatic:
            S = np.diag([(S[0, 0] + S[1, 1] + S[2, 2]) / 3.0] * 3)    # (zeros off the diagonal, whatever the trace is)
        sm = np.float64(np.abs(S).max()) / np.float64(V)          # (numpy's maximum: a NaN propagates)
        try:
            Fi = np.linalg.inv(F)
        except np.linalg.LinAlgError:
            Fi = np.full((3, 3), np.nan)
        g_c = -(Fi.T @ S) / L
    return V, S, float(sm), g_c


def fire_cell_step_ref(pos, vel, dE, W, gptr, cell0, cell, F, vcell, state, fmax_tol, smax_tol, fixed=None, cell_dof=None,
                       cell_factor=None, pressure=0.0, hydrostatic=False, dt_max=1.0, max_step=0.2, n_min=5, f_inc=1.1,
                       f_dec=0.5, a0=0.1, f_a=0.99, diag=None):
    """pos, vel, dE: float32 [n, 3]; W, cell0, cell: float32 [G, 3, 3]; F, vcell: float64 [G, 3, 3]; state: the dict of
    fire_step_ref plus smax (float32 [G]); fmax_tol, smax_tol, pressure: a float or [G]; cell_factor: float64 [G]; cell_dof:
    bool [G] or None (all).  Returns new (pos, vel, cell, F, vcell, state); the inputs are not modified.  diag: a dict that
    receives, per graph, the quantities the branches compare (None for a graph that was left alone)."""
    pos, vel = np.array(pos, dtype=np.float32), np.array(vel, dtype=np.float32)
    dE = np.asarray(dE, dtype=np.float32)
    n, G = pos.shape[0], len(gptr) - 1
    W, cell0 = np.asarray(W, dtype=np.float32).reshape(G, 3, 3), np.asarray(cell0, dtype=np.float32).reshape(G, 3, 3)
    cell = np.array(cell, dtype=np.float32).reshape(G, 3, 3)
    F, vcell = np.array(F, dtype=np.float64).reshape(G, 3, 3), np.array(vcell, dtype=np.float64).reshape(G, 3, 3)
    st = {k: np.array(state[k]) for k in CELL_STATE}
    assert st['dt'].dtype == np.float64 and st['a'].dtype == np.float64 and st['smax'].dtype == np.float32
    fixed = np.zeros(n, dtype=bool) if fixed is None else np.asarray(fixed).astype(bool)
    dof = np.ones(G, dtype=bool) if cell_dof is None else np.asarray(cell_dof).astype(bool)
    tol = np.broadcast_to(np.asarray(fmax_tol, dtype=np.float64), (G,))
    stol = np.broadcast_to(np.asarray(smax_tol, dtype=np.float64), (G,))
    prs = np.broadcast_to(np.asarray(pressure, dtype=np.float64), (G,))
    Lf = np.asarray(cell_factor, dtype=np.float64)
    rule = dict(dt_max=dt_max, max_step=max_step, n_min=n_min, f_inc=f_inc, f_dec=f_dec, a0=a0, f_a=f_a)
    if not dof.all():                                             # the graphs that keep their cell: the fixed-cell rule
        keep = {k: st[k].copy() for k in STATE}
        keep['status'][dof] = 3                                   # (left alone by fire_step_ref)
        d0 = {} if diag is not None else None
        p0, v0, s0 = fire_step_ref(pos, vel, dE, gptr, keep, tol, fixed, diag=d0, **rule)
        for g in np.nonzero(~dof)[0]:
            lo, hi = max(int(gptr[g]), 0), min(int(gptr[g + 1]), n)
            pos[lo:hi], vel[lo:hi] = p0[lo:hi], v0[lo:hi]
            for k in STATE:
                st[k][g] = s0[k][g]
            if diag is not None:
                diag[g] = d0[g]
    for g in np.nonzero(dof)[0]:
        if diag is not None:
            diag[g] = None
        if st['status'][g] != 0:                                               # 0
            continue
        lo, hi = max(int(gptr[g]), 0), min(int(gptr[g + 1]), n)
        atoms = np.arange(lo, max(hi, lo))
        free = atoms[~fixed[atoms]]
        L, p, Fg = float(Lf[g]), float(prs[g]), F[g]
        V, S, sm, g_c = stress_terms(W[g], cell0[g], Fg, L, p, hydrostatic)     # 1
        f, v = -dE[free].astype(np.float64), vel[free].astype(np.float64)
        v_c = vcell[g].copy()
        with np.errstate(all='ignore'):
            fm = float(np.sqrt((f * f).sum(1).max())) if free.size else 0.0     # 2
            g_a = f @ Fg.T
            F2 = float((g_a * g_a).sum()) + float((g_c * g_c).sum())            # 3
        rec = None
        if diag is not None:
            rec = diag[g] = dict(F2=F2, fm=fm, tol=float(tol[g]), sm=sm, stol=float(stol[g]), V=V, cell=True)
        if not np.isfinite(F2) or not np.isfinite(V) or V == 0.0:
            with np.errstate(all='ignore'):
                st['status'][g], st['fmax'][g], st['smax'][g] = 2, np.float32(np.sqrt(F2)), np.float32(sm)
            continue
        if fm < tol[g] and sm < stol[g]:
            st['status'][g], st['fmax'][g], st['smax'][g] = 1, np.float32(fm), np.float32(sm)
            continue
        P = float((g_a * v).sum()) + float((g_c * v_c).sum())                   # 4
        V2 = float((v * v).sum()) + float((v_c * v_c).sum())
        dt, a, n_pos = float(st['dt'][g]), float(st['a'][g]), int(st['n_pos'][g])
        if rec is not None:
            rec.update(P=P, V2=V2, dt_in=dt, n_pos_in=n_pos)
        c_v, c_f = 1.0, 0.0
        if V2 == 0.0:
            pass
        elif P > 0.0:
            n_pos += 1
            if n_pos > n_min:
                dt = min(dt * f_inc, dt_max)
                a *= f_a
            c_v, c_f = 1.0 - a, a * np.sqrt(V2 / F2)
        else:
            c_v, a, n_pos = 0.0, a0, 0
            dt *= f_dec
        v = (c_v * v + c_f * g_a) + dt * g_a                                    # 5
        v_c = (c_v * v_c + c_f * g_c) + dt * g_c
        m_a = float(np.sqrt(((dt * v) ** 2).sum(1).max())) if free.size else 0.0    # 6
        m_c = float(np.sqrt(((dt * v_c) ** 2).sum(1).max()))
        m = max(m_a, m_c)
        s = 1.0 if m == 0.0 else min(1.0, max_step / m)
        Fn = Fg + s * dt * v_c / L                                              # 7
        dn = float(np.linalg.det(Fn))
        if rec is not None:
            rec.update(max_dr=m, max_dr_atoms=m_a, max_dr_cell=m_c, det_new=dn)
        if not (dn > 0.0 and np.isfinite(dn)):
            st['status'][g], st['fmax'][g], st['smax'][g] = 2, np.float32(fm), np.float32(sm)
            continue
        D = np.linalg.inv(Fg) @ Fn                                              # 8
        new = pos[atoms].astype(np.float64) @ D                                 # 9
        new[~fixed[atoms]] += (s * dt * v) @ Fn
        pos[atoms] = new.astype(np.float32)
        vel[free] = v.astype(np.float32)
        cell[g] = (cell0[g].astype(np.float64) @ Fn).astype(np.float32)         # 10
        F[g], vcell[g] = Fn, v_c
        st['dt'][g], st['a'][g], st['n_pos'][g] = dt, a, n_pos
        st['fmax'][g], st['smax'][g] = np.float32(fm), np.float32(sm)
        st['steps'][g] += 1
    return pos, vel, cell, F, vcell, st


def generalised_gradient(dE, W, cell0, F, L, p, hydrostatic=False):
    """(g_a [m, 3], g_c L [3, 3]) of one graph with every atom free: minus the gradient of E + p V with respect to x~ and to F."""
    _, _, _, g_c = stress_terms(W, cell0, F, L, p, hydrostatic)
    return -np.asarray(dE, np.float64) @ np.asarray(F).T, g_c * L
