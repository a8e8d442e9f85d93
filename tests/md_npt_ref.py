"""The rule of pamnet_md_npt_step_f32 (include/pamnet_hip.h) restated in numpy, fp64 -- the reference of tests/test_md_npt.py.
The generator and the fixed-cell step are those of tests/md_ref.py (imported, not copied).

md_npt_step_ref, per graph g with cell_dof[g] != 0, sums over the free atoms, f = -dE/dpos, W = dE/dstrain:
  1. status[g] != 0: g is left alone.
  2. v_n = v + kick_in (dt / 2) f / m.
  3. F2 = sum |f|^2, KE = 1/2 sum m |v_n|^2, trW = (W00 + W11) + W22, V = |det cell0[g]| exp(eps[g]),
     P_int = (2 KE - trW) / (3 V); ke[g] = KE, pint[g] = P_int, vol[g] = V.  F2, KE, trW or V not finite, or V == 0: status[g] = 2,
     nothing else changes.
  4. d = -rate (P0 - P_int) dt + sqrt(2 kT rate dt / V) xi_c, xi_c = normals(seed[g], 1, steps[g], 2)[0, 0] (stream 2); where
     kT == 0 the noise term is exactly 0.  d not finite: status[g] = 2, nothing else changes.
     advance == 0: vel <- v_n, done.
  5. v1 = v_n + (dt / 2) f / m; gamma > 0: v2 = c1 v1 + c2 sqrt(kT / m) xi (stream 0); else v2 = v1.  s = exp(d / 3).
     Free atom: pos <- s (pos + (dt / 2)(v1 + v2)), vel <- v2 / s.  Fixed atom: pos <- s pos.
     eps[g] += d; cell[g] = cell0[g] exp(eps_new / 3).
  6. steps[g] += 1.
A graph with cell_dof[g] == 0 goes through md_step_ref; its eps, cell, pint and vol stay.
fp64 from the fp32 inputs, one rounding to fp32 where pos, vel and cell are stored.

npt_batch_ref is the same rule for G graphs of N free unit-mass atoms at once, with the normals handed in: the statistical
tests run it over many graphs and steps in seconds; test_md_npt.py checks it against md_npt_step_ref step by step."""
import numpy as np

from md_ref import STATE, _free, md_step_ref, normals

NPT_STATE = STATE + ('eps', 'pint', 'vol')


def barostat_normal(seed, step):
    """xi_c of a graph: the first normal of the generator at counter (0, step, 2, 0) under the graph's key."""
    return float(normals(seed, 1, step, 2)[0, 0])


def det3(c):
    c = np.asarray(c, dtype=np.float64).reshape(3, 3)
    return (c[0, 0] * (c[1, 1] * c[2, 2] - c[1, 2] * c[2, 1]) - c[0, 1] * (c[1, 0] * c[2, 2] - c[1, 2] * c[2, 0])
            + c[0, 2] * (c[1, 0] * c[2, 1] - c[1, 1] * c[2, 0]))


def md_npt_step_ref(pos, vel, dE, W, gptr, cell0, cell, state, dt, kT, gamma, pressure, rate, mass=None, fixed=None, cell_dof=None,
                    kick_in=1, advance=1):
    """pos, vel, dE: float32 [n, 3]; W, cell0, cell: float32 [G, 3, 3]; gptr: [G + 1]; state: dict of seed (int64, or None where no
    noise can occur), steps, status (int32), ke, eps, pint, vol (float64), each [G]; dt, kT, gamma, pressure, rate: a float or
    [G]; mass: float32 [n] or None; fixed: bool [n] or None; cell_dof: bool [G] or None (all True).
    Returns new (pos, vel, cell, state); the inputs are not modified."""
    n, G = len(pos), len(gptr) - 1
    dof = np.ones(G, dtype=bool) if cell_dof is None else np.asarray(cell_dof).astype(bool)
    st = {k: (None if state[k] is None else np.array(state[k])) for k in NPT_STATE}
    assert all(st[k].dtype == np.float64 for k in ('ke', 'eps', 'pint', 'vol')) and st['steps'].dtype == np.int32
    # the graphs without a barostat: md_step_ref, with the others masked out by a status that is not 0
    masked = {k: st[k] for k in STATE}
    masked['status'] = np.where(dof, 1, st['status']).astype(np.int32)
    pos, vel, plain = md_step_ref(pos, vel, dE, gptr, masked, dt, kT, gamma, mass, fixed, kick_in, advance)
    for k in ('steps', 'ke'):
        st[k] = np.where(dof, st[k], plain[k])
    st['status'] = np.where(dof, st['status'], plain['status']).astype(np.int32)
    st['steps'] = st['steps'].astype(np.int32)
    dE, W = np.asarray(dE, dtype=np.float32), np.asarray(W, dtype=np.float32).reshape(G, 3, 3)
    cell0 = np.asarray(cell0, dtype=np.float32).reshape(G, 3, 3)
    cell = np.array(cell, dtype=np.float32).reshape(G, 3, 3)
    fixed = np.zeros(n, dtype=bool) if fixed is None else np.asarray(fixed).astype(bool)
    m_all = np.ones(n) if mass is None else np.asarray(mass, dtype=np.float32).astype(np.float64)
    dt, kT, gamma, pressure, rate = (np.broadcast_to(np.asarray(x, dtype=np.float64), (G,)) for x in (dt, kT, gamma, pressure, rate))
    for g in range(G):
        if not dof[g] or st['status'][g] != 0:                                 # 1
            continue
        lo, hi, free = _free(gptr, g, n, fixed)
        held = np.arange(lo, hi)[fixed[lo:hi]]
        h = 0.5 * dt[g]
        with np.errstate(all='ignore'):
            f, v, m = -dE[free].astype(np.float64), vel[free].astype(np.float64), m_all[free][:, None]
            a = f / m
            if kick_in:
                v = v + h * a                                                  # 2
            F2, KE = float((f * f).sum()), 0.5 * float((m * v * v).sum())      # 3
            w = W[g].astype(np.float64)
            trW = (w[0, 0] + w[1, 1]) + w[2, 2]
            V = abs(det3(cell0[g])) * np.exp(st['eps'][g])
            pint = (2.0 * KE - trW) / (3.0 * V)
            st['ke'][g], st['pint'][g], st['vol'][g] = KE, pint, V
            if not (np.isfinite(F2) and np.isfinite(KE) and np.isfinite(trW) and np.isfinite(V)) or V == 0.0:
                st['status'][g] = 2
                continue
            d = -rate[g] * (pressure[g] - pint) * dt[g]                        # 4
            if kT[g] > 0.0:
                d = d + np.sqrt(2.0 * kT[g] * rate[g] * dt[g] / V) * barostat_normal(st['seed'][g], st['steps'][g])
            if not np.isfinite(d):
                st['status'][g] = 2
                continue
            if not advance:
                vel[free] = v.astype(np.float32)
                continue
            v1 = v + h * a                                                     # 5
            if gamma[g] > 0.0:
                c1 = np.exp(-gamma[g] * dt[g])
                c2 = np.sqrt(1.0 - c1 * c1)
                xi = normals(st['seed'][g], hi - lo, st['steps'][g], 0)[free - lo]
                v2 = c1 * v1 + c2 * np.sqrt(kT[g] / m) * xi
            else:
                v2 = v1
            s = np.exp(d / 3.0)
            pos[free] = (s * (pos[free].astype(np.float64) + h * (v1 + v2))).astype(np.float32)
            vel[free] = (v2 / s).astype(np.float32)
            pos[held] = (s * pos[held].astype(np.float64)).astype(np.float32)
            st['eps'][g] += d
            cell[g] = (cell0[g].astype(np.float64) * np.exp(st['eps'][g] / 3.0)).astype(np.float32)
        st['steps'][g] += 1                                                    # 6
    return pos, vel, cell, st


def npt_batch_ref(pos, vel, f, trW, V0, eps, dt, kT, gamma, pressure, rate, xi, xi_c, kick_in=1, round32=False):
    """One advancing step (advance = 1) of the rule for G graphs of N free atoms of unit mass at once, in fp64: pos, vel, f
    [G, N, 3] (f the forces); trW, V0, eps, pressure, rate [G] or floats; xi [G, N, 3] the thermostat's normals (ignored where
    gamma is 0), xi_c [G] the barostat's.  round32: pos and vel go through fp32 as the kernel stores them.
    Returns (pos, vel, eps, ke, pint, vol)."""
    h = 0.5 * dt
    v = vel + h * f if kick_in else vel
    KE = 0.5 * (v * v).sum((1, 2))
    V = V0 * np.exp(eps)
    pint = (2.0 * KE - trW) / (3.0 * V)
    d = -rate * (pressure - pint) * dt
    if kT > 0.0:
        d = d + np.sqrt(2.0 * kT * rate * dt / V) * xi_c
    v1 = v + h * f
    if gamma > 0.0:
        c1 = np.exp(-gamma * dt)
        v2 = c1 * v1 + np.sqrt(1.0 - c1 * c1) * np.sqrt(kT) * xi
    else:
        v2 = v1
    s = np.exp(d / 3.0)[:, None, None]
    pos, vel = s * (pos + h * (v1 + v2)), v2 / s
    if round32:
        pos, vel = pos.astype(np.float32).astype(np.float64), vel.astype(np.float32).astype(np.float64)
    return pos, vel, eps + d, KE, pint, V
