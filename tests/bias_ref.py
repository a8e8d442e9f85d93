"""The rules of pamnet_bias_apply_f64 and pamnet_bias_grid_f64 (include/pamnet_hip.h) restated in numpy, fp64 -- the reference of
tests/test_bias.py.

cv_ref:    a collective variable and its gradient (distance, angle, dihedral) by the header's closed forms.
apply_ref: one launch.  The additions are made in the kernel's order: thread q of 256 adds the hills q, q + 256, ... in that
           order; the 64 lanes of a wavefront are added by the butterfly v += v[lane ^ o], o = 32 .. 1; the four wavefront sums
           are added in order; the restraint energies follow in the order of the variables; dpos takes c_k ds_k/dx per variable
           in order and per atom in order, with one rounding to fp32 per addition.
grid_ref:  the bias of one table at a set of points, the hills in order.
metad_run_ref: the launch sequence of md.run(bias=...) over apply_ref and md_step_ref of tests/md_ref.py (its Philox generator)."""
import numpy as np

from md_ref import md_step_ref

TWO_PI = 6.283185307179586476925286766559
DISTANCE, ANGLE, DIHEDRAL = 0, 1, 2
N_ATOMS = (2, 3, 4)
TABLE = ('hill_c', 'hill_w', 'n_hills', 'dropped')
MAX_CVS, MAX_WALKERS = 16, 256


def wrap(d, periodic):
    return d - TWO_PI * np.rint(d / TWO_PI) if periodic else d


def cv_ref(kind, x):
    """kind: 0 / 1 / 2; x: float64 [2 | 3 | 4, 3] -> (s, ds/dx of the same shape)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all='ignore'):
        if kind == DISTANCE:
            r = x[1] - x[0]
            d = np.sqrt(r @ r)
            return d, np.stack([-r / d, r / d])
        if kind == ANGLE:
            a, b = x[0] - x[1], x[2] - x[1]
            nn = np.cross(a, b)
            n1 = np.sqrt(nn @ nn)
            gi, gk = np.cross(a, nn) / ((a @ a) * n1), np.cross(nn, b) / ((b @ b) * n1)
            return np.arctan2(n1, a @ b), np.stack([gi, -(gi + gk), gk])
        b1, b2, b3 = x[1] - x[0], x[2] - x[1], x[3] - x[2]
        m, nn = np.cross(b1, b2), np.cross(b2, b3)
        l2, m2, n2 = np.sqrt(b2 @ b2), m @ m, nn @ nn
        p, q = (b1 @ b2) / (m2 * l2), (b3 @ b2) / (n2 * l2)
        grad = np.stack([-l2 / m2 * m, (l2 / m2 + p) * m + q * nn, -p * m - (q + l2 / n2) * nn, l2 / n2 * nn])
        return np.arctan2(l2 * (b1 @ nn), m @ nn), grad


def hill_sums(s, periodic, hc, hw, n0, sigma, nde):
    """(V, dV/ds_0, dV/ds_1) of the point s against the hills [0, n0), in the kernel's order of additions."""
    acc = np.zeros((256, 3))
    for start in range(0, n0 if nde else 0, 256):                  # pass j: thread q takes hill start + q
        h = np.arange(start, min(start + 256, n0))
        q = h - start
        u0 = wrap(s[0] - hc[h, 0], periodic[0]) / sigma[0]
        u1 = wrap(s[1] - hc[h, 1], periodic[1]) / sigma[1] if nde > 1 else np.zeros(len(h))
        e = hw[h] * np.exp(-0.5 * (u0 * u0 + u1 * u1))
        acc[q, 0] += e
        acc[q, 1] -= e * u0 / sigma[0]
        if nde > 1:
            acc[q, 2] -= e * u1 / sigma[1]
    a = acc.reshape(4, 64, 3)
    for o in (32, 16, 8, 4, 2, 1):                                 # wave_sum
        a = a + a[:, np.arange(64) ^ o]
    p = a[:, 0]
    return ((p[0] + p[1]) + p[2]) + p[3]


def apply_ref(pos, dpos, status, gptr, bptr, tab, deposit):
    """pos, dpos: float32 [n, 3]; status: int32 [G]; gptr [G + 1]; bptr [T + 1]; tab: dict of cvptr [G + 1], kind [K], atoms
    [K, 4], kappa, centre, halfwidth [K], ndim [T], sigma [T, 2], height0, inv_dT [T], hill_c [T, H, 2], hill_w [T, H], n_hills,
    dropped [T].  Returns new (dpos, status, cv [K], ebias [G], table) with table the dict of the four hill arrays; the inputs
    are not modified."""
    pos = np.asarray(pos, dtype=np.float32)
    dpos, status = np.array(dpos, dtype=np.float32), np.array(status, dtype=np.int32)
    out = {k: np.array(tab[k]) for k in TABLE}
    K, G, T = len(tab['kind']), len(gptr) - 1, len(bptr) - 1
    cv, ebias = np.full(K, np.nan), np.full(G, np.nan)
    H = out['hill_c'].shape[1]
    for t in range(T):
        lo, hi = max(int(bptr[t]), 0), min(int(bptr[t + 1]), G)
        if hi - lo > MAX_WALKERS:
            continue
        nd = min(max(int(tab['ndim'][t]), 0), 2)
        n0 = min(max(int(tab['n_hills'][t]), 0), H)
        hc, hw, sigma = np.asarray(tab['hill_c'][t]), np.asarray(tab['hill_w'][t]), tab['sigma'][t]
        walkers = []
        for g in range(lo, hi):
            k0, k1 = max(int(tab['cvptr'][g]), 0), min(int(tab['cvptr'][g + 1]), K)
            nk = max(k1 - k0, 0)
            if status[g] != 0 or nk > MAX_CVS:                     # 1
                continue
            alo, ahi = max(int(gptr[g]), 0), min(int(gptr[g + 1]), len(pos))
            s, grads, good = np.zeros(nk), [], True
            for k in range(nk):                                    # 2
                kind = int(tab['kind'][k0 + k])
                if kind not in (0, 1, 2):
                    good = False
                    break
                at = [int(a) for a in tab['atoms'][k0 + k][:N_ATOMS[kind]]]
                if any(a < alo or a >= ahi for a in at):
                    good = False
                    break
                s[k], gr = cv_ref(kind, pos[at].astype(np.float64))
                grads.append((at, gr))
                good = good and bool(np.isfinite(s[k]) and np.isfinite(gr).all())
            if not good:
                status[g] = 2
                continue
            nde = min(nd, nk)
            periodic = [k < nk and tab['kind'][k0 + k] == DIHEDRAL for k in (0, 1)]
            V, dV0, dV1 = hill_sums(s, periodic, hc, hw, n0, sigma, nde) if nde else (0.0, 0.0, 0.0)       # 3
            E = V
            for k in range(nk):
                c = 0.0 if k >= nde else (dV0, dV1)[k]
                kap = float(tab['kappa'][k0 + k])
                if kap != 0.0:                                     # 4
                    d = wrap(s[k] - tab['centre'][k0 + k], tab['kind'][k0 + k] == DIHEDRAL)
                    a = abs(d) - tab['halfwidth'][k0 + k]
                    if a > 0.0:
                        E += 0.5 * kap * a * a
                        c += -kap * a if d < 0.0 else kap * a
                if c == 0.0:
                    continue
                at, gr = grads[k]
                for i, a in enumerate(at):                         # 6
                    for x in range(3):
                        dpos[a, x] = np.float32(np.float64(dpos[a, x]) + c * gr[i, x])
            cv[k0:k1], ebias[g] = s, E                             # 5
            if nde:
                walkers.append((s[0], s[1] if nde > 1 else 0.0, V))
        if deposit and nd > 0:                                     # 7
            cnt = n0
            for s0, s1, V in walkers:
                if cnt >= H:
                    out['dropped'][t] += 1
                    continue
                out['hill_c'][t, cnt] = (s0, s1)
                out['hill_w'][t, cnt] = tab['height0'][t] * np.exp(-V * tab['inv_dT'][t])
                cnt += 1
            out['n_hills'][t] = cnt
    return dpos, status, cv, ebias, out


def grid_ref(tab, t, points, periodic):
    """V of table t at points [M, ndim], the hills in order."""
    points = np.asarray(points, dtype=np.float64)
    nd = points.shape[1]
    n0 = min(max(int(tab['n_hills'][t]), 0), tab['hill_c'].shape[1])
    v = np.zeros(len(points))
    for h in range(n0):
        u2 = np.zeros(len(points))
        for d in range(nd):
            u = wrap(points[:, d] - tab['hill_c'][t, h, d], periodic[d]) / tab['sigma'][t, d]
            u2 = u2 + u * u
        v = v + tab['hill_w'][t, h] * np.exp(-0.5 * u2)
    return v


def free_energy_ref(tab, t, points, periodic, bias_factor):
    """-gamma / (gamma - 1) V (well-tempered) or -V (bias_factor None), shifted to minimum 0."""
    v = grid_ref(tab, t, points, periodic)
    f = -v if bias_factor is None else -bias_factor / (bias_factor - 1.0) * v
    return f - f.min()


def metad_run_ref(grad, pos, vel, gptr, state, bptr, tab, steps, dt, kT=0.0, gamma=0.0, pace=0, mass=None, fixed=None,
                  record_every=0):
    """The launch sequence of md.run(bias=...): evaluate -- grad(pos) -> (energy [G], dE float32 [n, 3]) --, apply_ref with
    deposit = advance and it % pace == 0, then md_step_ref: (0, 1), then (1, 1), and a closing (1, 0).  tab: apply_ref's.
    Returns a dict of pos, vel, state, table (the tab with its final hills), and with record_every the records frames, epot,
    ekin, ebias [F, G] and cv [F, K]."""
    pos, vel = np.array(pos, dtype=np.float32), np.array(vel, dtype=np.float32)
    st = {k: (None if v is None else np.array(v)) for k, v in state.items()}
    tab = dict(tab)
    G, K = len(gptr) - 1, len(tab['kind'])
    rec = None
    if record_every:
        F = steps // record_every + 1
        rec = dict(frames=np.zeros((F,) + pos.shape, np.float32), epot=np.zeros((F, G)), ekin=np.zeros((F, G)),
                   ebias=np.zeros((F, G)), cv=np.zeros((F, K)))
    for it in range(steps + 1):
        advance = 1 if it < steps else 0
        e, dE = grad(pos)
        dE, status, cv, ebias, hills = apply_ref(pos, dE, st['status'], gptr, bptr, tab, 1 if advance and pace and it % pace == 0 else 0)
        tab.update(hills)
        st['status'] = status
        if rec is not None and it % record_every == 0:
            r = it // record_every
            rec['frames'][r], rec['epot'][r], rec['ebias'][r], rec['cv'][r] = pos, e, ebias, cv
        pos, vel, st = md_step_ref(pos, vel, dE, gptr, st, dt, kT, gamma, mass, fixed, 1 if it else 0, advance)
        if rec is not None and it % record_every == 0:
            rec['ekin'][it // record_every] = st['ke']
    out = dict(pos=pos, vel=vel, state=st, table=tab)
    if rec is not None:
        out.update(rec)
    return out
