"""The rules of pamnet_md_constrained_step_f32 and pamnet_md_project_constraints_f32 (include/pamnet_hip.h) restated in numpy,
fp64 -- the reference of tests/test_md_constraints.py.  The generator and the unconstrained step are tests/md_ref.py's.

The colouring: constraint k, in the order given, takes the smallest colour no earlier constraint with one of its atoms took; the
constraints are then sorted by (graph, colour), stably.  A sweep visits the colours of a graph in order; inside a colour no two
constraints share an atom, so updating a colour's constraints at once is the Gauss-Seidel sweep in the order (colour, position).

With w = 0 for a fixed atom and 1 / m otherwise, and a fixed atom's velocity taken as 0:
  RATTLE_V  r = x_i - x_j, u = v_i - v_j, err = |r.u| dt / d^2, kappa = r.u / ((w_i + w_j) r.r), v_i -= w_i kappa r, v_j += w_j kappa r
  SHAKE     s = x_i - x_j, r0 = x0_i - x0_j, err = |s.s - d^2| / (2 d^2), g = (s.s - d^2) / (2 (w_i + w_j) s.r0), x_i -= w_i g r0,
            x_j += w_j g r0
A solve has converged after the first sweep in which every err -- measured as the sweep reaches the constraint -- is <= tol; it
is broken by an err that is not finite or by s.r0 <= 0, and has failed after max_sweeps sweeps.

constrained_step_ref, per graph with constraints, f = -dE, sums over the free atoms:
  1. status != 0: left alone.
  2. v = v + kick_in (dt / 2) f / m; F2 = sum |f|^2, KE = 1/2 sum m |v|^2; either not finite: ke = KE, status = 2, sweeps = 0.
  3. kick_in: RATTLE_V and KE again; ke = KE (not finite: status = 2).
  4. advance == 0: vel <- v if kick_in; done.
  5. v += (dt / 2) f / m, RATTLE_V; half drift (x0 = x, x += (dt / 2) v, SHAKE, v = (x - x0) / (dt / 2)), RATTLE_V; gamma > 0:
     v = c1 v + c2 sqrt(kT / m) xi (md_ref's normals: stream 0, the graph's step), RATTLE_V; half drift, RATTLE_V.
  6. pos <- fp32(x), vel <- fp32(v), steps += 1.
  A failed solve: status = 3, sweeps written, pos / vel / steps stay.  sweeps = the most sweeps a solve of the launch ran.
A graph without constraints is md_step_ref's (sweeps = 0 where it was running)."""
import numpy as np

from md_ref import md_step_ref, normals

STATE = ('seed', 'steps', 'status', 'ke', 'sweeps')


def colour_ref(pairs, graph):
    """(colour [C], order [C]) of the constraints `pairs` [C, 2] of the graphs `graph` [C]."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    colour, at = np.zeros(len(pairs), dtype=np.int64), {}
    for k, (i, j) in enumerate(pairs.tolist()):
        taken = at.setdefault(i, set()) | at.setdefault(j, set())
        c = 0
        while c in taken:
            c += 1
        colour[k] = c
        at[i].add(c), at[j].add(c)
    order = sorted(range(len(pairs)), key=lambda k: (int(graph[k]), int(colour[k]), k))
    return colour, np.asarray(order, dtype=np.int64)


class ConsRef(object):
    """The sorted constraints and their two-level CSR: i, j, d, graph, colour (sorted), order, gcol [G + 1], colptr [K + 1]."""

    def __init__(self, pairs, lengths, batch, n_graphs):
        pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        batch = np.asarray(batch, dtype=np.int64)
        graph = batch[pairs[:, 0]] if len(pairs) else np.zeros(0, np.int64)
        colour, order = colour_ref(pairs, graph)
        self.order, self.graph, self.colour = order, graph[order], colour[order]
        self.i, self.j = pairs[order, 0], pairs[order, 1]
        self.d = np.asarray(lengths, dtype=np.float64)[order]
        n_col = np.zeros(n_graphs, dtype=np.int64)
        for g, c in zip(self.graph, self.colour):
            n_col[g] = max(n_col[g], c + 1)
        self.gcol = np.concatenate([[0], np.cumsum(n_col)]).astype(np.int64)
        colptr = np.zeros(int(self.gcol[-1]) + 1, dtype=np.int64)
        for g, c in zip(self.graph, self.colour):
            colptr[self.gcol[g] + c + 1] += 1
        self.colptr = np.cumsum(colptr)
        self.n, self.n_graphs = len(pairs), n_graphs
        self.n_per_graph = np.bincount(self.graph, minlength=n_graphs)

    def colours(self, g):
        """[(i, j, d)] of the colours of graph g, in order."""
        out = []
        for k in range(int(self.gcol[g]), int(self.gcol[g + 1])):
            s = slice(int(self.colptr[k]), int(self.colptr[k + 1]))
            out.append((self.i[s], self.j[s], self.d[s]))
        return out


def _verdict(errs, ok, tol, rec):
    worst = max([float(e.max()) for e in errs if e.size] or [0.0])
    if worst != worst:                                             # (max of an array with a NaN is NaN)
        worst = np.inf
    if rec is not None:
        rec.append(worst)
    if not ok or worst == np.inf:
        return 2
    return 0 if worst <= tol else 1


def _prepared(cols, w):
    """Per colour what no sweep changes: (i, j, d^2, w_i, w_j, w_i + w_j, every w_i + w_j > 0)."""
    return [(i, j, d * d, w[i], w[j], w[i] + w[j], bool((w[i] + w[j] > 0.0).all())) for i, j, d in cols]


def _dot(a, b):
    return np.einsum('ij,ij->i', a, b)


def rattle_ref(x, v, w, cols, dt, tol, max_sweeps, diag=None):
    """In place on v.  Returns (converged, sweeps).  diag: a list that takes (kind, verdict, [the largest err of each sweep])."""
    rec = [] if diag is not None else None
    it, verdict, prep = 0, 1, _prepared(cols, w)
    with np.errstate(all='ignore'):
        while it < max_sweeps:
            errs, ok = [], True
            for i, j, d2, wi, wj, ws, free in prep:
                r, u = x[i] - x[j], v[i] - v[j]
                rv, rr = _dot(r, u), _dot(r, r)
                err = np.abs(rv) * dt / d2
                errs.append(err)
                fin = np.isfinite(err)
                act = fin & (ws > 0.0) & (rr > 0.0)
                if free and act.all():                             # (the common case, without the masks)
                    kappa = rv / (ws * rr)
                    v[i] -= (wi * kappa)[:, None] * r
                    v[j] += (wj * kappa)[:, None] * r
                    continue
                ok = ok and bool(fin.all())
                kappa = rv[act] / (ws[act] * rr[act])
                v[i[act]] -= (wi[act] * kappa)[:, None] * r[act]
                v[j[act]] += (wj[act] * kappa)[:, None] * r[act]
            verdict = _verdict(errs, ok, tol, rec)
            it += 1
            if verdict != 1:
                break
    if diag is not None:
        diag.append(('rattle', verdict, rec))
    return verdict == 0, it


def shake_ref(x0, x, w, cols, tol, max_sweeps, diag=None):
    """In place on x.  Returns (converged, sweeps)."""
    rec = [] if diag is not None else None
    it, verdict, prep = 0, 1, _prepared(cols, w)
    with np.errstate(all='ignore'):
        while it < max_sweeps:
            errs, ok = [], True
            for i, j, d2, wi, wj, ws, free in prep:
                s, r0 = x[i] - x[j], x0[i] - x0[j]
                diff, sr = _dot(s, s) - d2, _dot(s, r0)
                err = np.abs(diff) / (2.0 * d2)
                errs.append(err)
                good = np.isfinite(err) & (sr > 0.0)
                if free and good.all():
                    gk = diff / (2.0 * ws * sr)
                    x[i] -= (wi * gk)[:, None] * r0
                    x[j] += (wj * gk)[:, None] * r0
                    continue
                ok = ok and bool(good.all())
                act = good & (ws > 0.0)
                gk = diff[act] / (2.0 * ws[act] * sr[act])
                x[i[act]] -= (wi[act] * gk)[:, None] * r0[act]
                x[j[act]] += (wj[act] * gk)[:, None] * r0[act]
            verdict = _verdict(errs, ok, tol, rec)
            it += 1
            if verdict != 1:
                break
    if diag is not None:
        diag.append(('shake', verdict, rec))
    return verdict == 0, it


def _setup(pos, gptr, mass, fixed):
    n, G = pos.shape[0], len(gptr) - 1
    fixed = np.zeros(n, dtype=bool) if fixed is None else np.asarray(fixed).astype(bool)
    m_all = np.ones(n) if mass is None else np.asarray(mass, dtype=np.float32).astype(np.float64)
    w = np.where(fixed, 0.0, 1.0 / m_all)
    return n, G, fixed, m_all, w


def constrained_step_ref(pos, vel, dE, gptr, state, cons, dt, kT=0.0, gamma=0.0, mass=None, fixed=None, kick_in=1, advance=1,
                         tol=1e-8, max_sweeps=500, diag=None):
    """md_step_ref's arguments, cons (a ConsRef) and state['sweeps'] (int32 [G]).  Returns new (pos, vel, state).  diag: a dict
    that takes, per constrained graph that ran, the list of its solves as (kind, verdict, [largest err per sweep])."""
    pos, vel = np.array(pos, dtype=np.float32), np.array(vel, dtype=np.float32)
    dE = np.asarray(dE, dtype=np.float32)
    n, G, fixed, m_all, w = _setup(pos, gptr, mass, fixed)
    st = {k: (None if state[k] is None else np.array(state[k])) for k in STATE}
    has = np.diff(cons.gcol) > 0
    plain = {k: (None if st[k] is None else st[k].copy()) for k in ('seed', 'steps', 'status', 'ke')}
    plain['status'][has] = 1                                       # the graphs without constraints: md_step_ref, the others masked
    p2, v2, s2 = md_step_ref(pos, vel, dE, gptr, plain, dt, kT, gamma, mass, fixed, kick_in, advance)
    dt, kT, gamma = (np.broadcast_to(np.asarray(x, dtype=np.float64), (G,)) for x in (dt, kT, gamma))
    x0, x, v = np.zeros((n, 3)), pos.astype(np.float64), np.zeros((n, 3))
    for g in range(G):
        lo, hi = max(int(gptr[g]), 0), min(int(gptr[g + 1]), n)
        if st['status'][g] != 0:                                               # 1
            continue
        if not has[g]:
            pos[lo:hi], vel[lo:hi] = p2[lo:hi], v2[lo:hi]
            for k in ('steps', 'status', 'ke'):
                st[k][g] = s2[k][g]
            st['sweeps'][g] = 0
            continue
        idx = np.arange(lo, hi)
        free = idx[~fixed[idx]]
        cols, h, most = cons.colours(g), 0.5 * dt[g], 0
        rec = None
        if diag is not None:
            rec = diag.setdefault(g, [])
        with np.errstate(all='ignore'):
            f, m = -dE[free].astype(np.float64), m_all[free][:, None]
            a = f / m
            v[free] = vel[free].astype(np.float64) + (h * a if kick_in else 0.0)      # 2
            F2, KE = float((f * f).sum()), 0.5 * float((m * v[free] * v[free]).sum())
            if not (np.isfinite(F2) and np.isfinite(KE)):
                st['ke'][g], st['status'][g], st['sweeps'][g] = KE, 2, 0
                continue
            ok = True
            if kick_in:                                                        # 3
                ok, it = rattle_ref(x, v, w, cols, dt[g], tol, max_sweeps, rec)
                most = max(most, it)
                if ok:
                    KE = 0.5 * float((m * v[free] * v[free]).sum())
            if ok and not np.isfinite(KE):
                st['ke'][g], st['status'][g], st['sweeps'][g] = KE, 2, most
                continue
            if ok:
                st['ke'][g] = KE
            if ok and not advance:                                             # 4
                if kick_in:
                    vel[free] = v[free].astype(np.float32)
                st['sweeps'][g] = most
                continue

            def half_drift():
                x0[idx] = x[idx]
                x[free] = x[free] + h * v[free]
                good, it = shake_ref(x0, x, w, cols, tol, max_sweeps, rec)
                if good:
                    v[free] = (x[free] - x0[free]) / h
                return good, it

            if ok:                                                             # 5
                v[free] = v[free] + h * a
                ok, it = rattle_ref(x, v, w, cols, dt[g], tol, max_sweeps, rec)
                most = max(most, it)
            for part in ('drift', 'rattle', 'noise', 'drift', 'rattle'):
                if not ok:
                    break
                if part == 'drift':
                    ok, it = half_drift()
                elif part == 'rattle':
                    ok, it = rattle_ref(x, v, w, cols, dt[g], tol, max_sweeps, rec)
                elif gamma[g] > 0.0:
                    c1 = np.exp(-gamma[g] * dt[g])
                    c2 = np.sqrt(1.0 - c1 * c1)
                    xi = normals(st['seed'][g], hi - lo, st['steps'][g], 0)[free - lo]
                    v[free] = c1 * v[free] + c2 * np.sqrt(kT[g] / m) * xi
                    ok, it = rattle_ref(x, v, w, cols, dt[g], tol, max_sweeps, rec)
                else:
                    continue
                most = max(most, it)
            st['sweeps'][g] = most
            if not ok:
                st['status'][g] = 3
                continue
            pos[free], vel[free] = x[free].astype(np.float32), v[free].astype(np.float32)      # 6
            if diag is not None:                                   # the constraints in fp64, before that rounding
                dev = [np.abs(((x[i] - x[j]) ** 2).sum(1) - d * d) / (2.0 * d * d) for i, j, d in cols]
                diag[('deviation', g)] = max(float(e.max()) for e in dev)
        st['steps'][g] += 1
    return pos, vel, st


def project_ref(pos, vel, gptr, state, cons, dt=None, mass=None, fixed=None, do_pos=True, do_vel=True, tol=1e-8, max_sweeps=500,
                diag=None):
    """pos, vel: float32 [n, 3] (vel may be None where do_vel is False); state: dict of status, ke, sweeps.  Returns new
    (pos, vel, state)."""
    pos = np.array(pos, dtype=np.float32)
    vel = None if vel is None else np.array(vel, dtype=np.float32)
    n, G, fixed, m_all, w = _setup(pos, gptr, mass, fixed)
    st = {k: np.array(state[k]) for k in ('status', 'ke', 'sweeps')}
    dt = np.broadcast_to(np.asarray(0.0 if dt is None else dt, dtype=np.float64), (G,))
    x, v = pos.astype(np.float64), np.zeros((n, 3))
    for g in range(G):
        lo, hi = max(int(gptr[g]), 0), min(int(gptr[g + 1]), n)
        if st['status'][g] != 0:
            continue
        idx = np.arange(lo, hi)
        free = idx[~fixed[idx]]
        m = m_all[free][:, None]
        cols = cons.colours(g)
        rec = None if diag is None else diag.setdefault(g, [])
        if do_vel:
            v[free] = vel[free].astype(np.float64)
        if not cols:
            if do_vel:
                st['ke'][g] = 0.5 * float((m * v[free] * v[free]).sum())
            st['sweeps'][g] = 0
            continue
        ok, most = True, 0
        if do_pos:
            x0 = x.copy()
            ok, most = shake_ref(x0, x, w, cols, tol, max_sweeps, rec)
        if ok and do_vel:
            ok, it = rattle_ref(x, v, w, cols, dt[g], tol, max_sweeps, rec)
            most = max(most, it)
        st['sweeps'][g] = most
        if not ok:
            st['status'][g] = 3
            continue
        if do_pos:
            pos[free] = x[free].astype(np.float32)
        if do_vel:
            vel[free] = v[free].astype(np.float32)
            st['ke'][g] = 0.5 * float((m * v[free] * v[free]).sum())
    return pos, vel, st
