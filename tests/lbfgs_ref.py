"""lbfgs_step_ref: the L-BFGS step of pamnet_lbfgs_step_f32 (include/pamnet_hip.h) restated in numpy, fp64 -- the reference of
tests/test_relax_lbfgs.py.  Per graph g, every sum and maximum over the free atoms of g, gr = dE/dpos, m = memory, |.| of an
atom the norm of its three components:

  1. status[g] != 0: g is left alone.
  2. F2 = sum |gr|^2, fm = max |gr|; fmax[g] = fm.  F2 not finite: status[g] = 2, fmax[g] = sqrt(F2), nothing else changes.
     Else fm < tolerance: status[g] = 1, nothing else changes (no free atoms: fm = 0).
  3. If has_prev[g]: s = pos - prev_pos, y = gr - prev_dpos (fp64 from the fp32 operands); ss = sum s.s, yy = sum y.y,
     ys = sum s.y.  If ys > skip_tol sqrt(ss yy): s, y go to ring slot head[g] of hist_s / hist_y, rho[g][head] = 1 / ys,
     gamma[g] = ys / yy, head = (head + 1) mod m, count = min(count + 1, m).  Otherwise skipped[g] += 1.
  4. Two-loop recursion over the count pairs held, pair j in slot (head - 1 - j) mod m (newest first): q = gr; for j = 0 ..
     count - 1: a_j = rho_j (s_j . q), q -= a_j y_j;  z = h0 q, h0 = gamma[g] if count > 0 else 1 / alpha;  for j = count - 1 .. 0:
     b = rho_j (y_j . z), z += (a_j - b) s_j.
  5. D = sum z . gr.  If not D > 0: count = head = 0, z = gr / alpha, resets[g] += 1, and the largest |z| is fm / alpha.
  6. L = max |z|, c = max_step / L if L > max_step else 1;  prev_pos <- pos, prev_dpos <- gr, has_prev = 1;
     pos <- float32(pos - c z);  steps[g] += 1.

fp64 from the fp32 inputs, one rounding to fp32 where pos is stored; fixed atoms are skipped everywhere: their rows of pos,
prev_pos, prev_dpos, hist_s, hist_y and work are neither read nor written.  `work` is the kernel's workspace: the reference
returns it as it was (its contents after a step are unspecified)."""
import numpy as np

SCALARS = ('rho', 'gamma', 'head', 'count', 'has_prev', 'skipped', 'resets', 'steps', 'status', 'fmax')
ARRAYS = ('prev_pos', 'prev_dpos', 'hist_s', 'hist_y', 'work')
STATE = ARRAYS + SCALARS
INT_STATE = ('head', 'count', 'has_prev', 'skipped', 'resets', 'steps', 'status')
DEFAULTS = dict(memory=10, alpha=70.0, max_step=0.2, skip_tol=1e-8)


def new_state_ref(n, n_graphs, memory):
    """The all-zero state of pamnet_amd.relax.new_lbfgs_state, as numpy."""
    st = dict(prev_pos=np.zeros((n, 3), np.float32), prev_dpos=np.zeros((n, 3), np.float32), hist_s=np.zeros((memory, n, 3)),
              hist_y=np.zeros((memory, n, 3)), work=np.zeros((n, 3)), rho=np.zeros((n_graphs, memory)), gamma=np.zeros(n_graphs),
              fmax=np.zeros(n_graphs, np.float32))
    for k in INT_STATE:
        st[k] = np.zeros(n_graphs, np.int32)
    return st


def lbfgs_step_ref(pos, dE, gptr, state, fmax_tol, fixed=None, alpha=70.0, max_step=0.2, skip_tol=1e-8, diag=None):
    """pos, dE: float32 [n, 3]; gptr: [G + 1]; state: the dict of STATE (memory = the leading extent of hist_s); fmax_tol: a float
    or [G]; fixed: bool [n] or None.  Returns new (pos, state); the inputs are not modified.
    diag: a dict that receives, per graph, the quantities the branches compare (None for a graph that was left alone)."""
    pos = np.array(pos, dtype=np.float32)
    dE = np.asarray(dE, dtype=np.float32)
    n, G = pos.shape[0], len(gptr) - 1
    st = {k: np.array(state[k]) for k in STATE}
    m = st['hist_s'].shape[0]
    assert st['hist_s'].shape == st['hist_y'].shape == (m, n, 3) and st['rho'].shape == (G, m)
    assert all(st[k].dtype == np.float64 for k in ('hist_s', 'hist_y', 'work', 'rho', 'gamma'))
    assert all(st[k].dtype == np.float32 for k in ('prev_pos', 'prev_dpos', 'fmax')) and all(st[k].dtype == np.int32 for k in INT_STATE)
    fixed = np.zeros(n, dtype=bool) if fixed is None else np.asarray(fixed).astype(bool)
    tol = np.broadcast_to(np.asarray(fmax_tol, dtype=np.float64), (G,))
    for g in range(G):
        if diag is not None:
            diag[g] = None
        if st['status'][g] != 0:                                               # 1
            continue
        lo, hi = max(int(gptr[g]), 0), min(int(gptr[g + 1]), n)
        free = np.arange(lo, max(hi, lo))
        free = free[~fixed[free]]
        gr = dE[free].astype(np.float64)
        with np.errstate(all='ignore'):
            g2 = (gr * gr).sum(1)
            F2 = float(g2.sum())                                               # 2
            fm = float(np.sqrt(g2.max())) if free.size else 0.0
            if not np.isfinite(F2):
                fm = float(np.sqrt(F2))
            st['fmax'][g] = np.float32(fm)
        rec = dict(F2=F2, fm=fm, tol=float(tol[g]))
        if diag is not None:
            diag[g] = rec
        if not np.isfinite(F2):
            st['status'][g] = 2
            continue
        if fm < tol[g]:
            st['status'][g] = 1
            continue
        head, count = int(st['head'][g]) % m, min(max(int(st['count'][g]), 0), m)
        rec.update(has_prev=bool(st['has_prev'][g]), count_in=count, head_in=head, stored=False)
        if st['has_prev'][g]:                                                  # 3
            s = pos[free].astype(np.float64) - st['prev_pos'][free].astype(np.float64)
            y = gr - st['prev_dpos'][free].astype(np.float64)
            with np.errstate(all='ignore'):
                ss, yy, ys = float((s * s).sum()), float((y * y).sum()), float((s * y).sum())
                bar = skip_tol * np.sqrt(ss * yy)
            rec.update(ss=ss, yy=yy, ys=ys)
            if ys > bar:
                st['hist_s'][head, free], st['hist_y'][head, free] = s, y
                st['rho'][g, head] = 1.0 / ys
                st['gamma'][g] = ys / yy
                head, count = (head + 1) % m, min(count + 1, m)
                rec['stored'] = True
            else:
                st['skipped'][g] += 1
        q = gr.copy()                                                          # 4
        slots = [(head - 1 - j) % m for j in range(count)]
        a = []
        with np.errstate(all='ignore'):
            for k in slots:
                a.append(st['rho'][g, k] * float((st['hist_s'][k, free] * q).sum()))
                q = q - a[-1] * st['hist_y'][k, free]
            z = (st['gamma'][g] if count > 0 else 1.0 / alpha) * q
            for j in range(count - 1, -1, -1):
                k = slots[j]
                b = st['rho'][g, k] * float((st['hist_y'][k, free] * z).sum())
                z = z + (a[j] - b) * st['hist_s'][k, free]
            D = float((z * gr).sum())                                          # 5
            znorm, grnorm = float(np.sqrt((z * z).sum())), float(np.sqrt(F2))
        rec.update(count=count, D=D, znorm=znorm, grnorm=grnorm, reset=not D > 0.0)
        if not D > 0.0:
            head, count = 0, 0
            z = gr / alpha
            st['resets'][g] += 1
            L = fm / alpha
        else:
            L = float(np.sqrt((z * z).sum(1).max())) if free.size else 0.0
        c = max_step / L if L > max_step else 1.0                              # 6
        rec.update(L=L)
        st['prev_pos'][free], st['prev_dpos'][free] = pos[free], dE[free]
        st['has_prev'][g] = 1
        pos[free] = (pos[free].astype(np.float64) - c * z).astype(np.float32)
        st['head'][g], st['count'][g] = head, count
        st['steps'][g] += 1
    return pos, st
