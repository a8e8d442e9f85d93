"""The rules of pamnet_vib_displace_f32, pamnet_vib_rows_f64 and pamnet_sym_eig_f64 (include/pamnet_hip.h) restated in numpy,
fp64 -- the references of tests/test_vib.py.

Layout: graph g has F_g free atoms, free_idx[fptr[g] .. fptr[g + 1]) ascending; its matrix of dimension d_g = 3 F_g is row-major
at moff[g] in a packed array (moff the prefix sum of d_g^2, dptr of d_g); row 3 f + c is free atom f, component c.  An evaluation
holds `pairs` = r central-difference pairs per graph: 2 r copies of the batch, copy 2 c the + and 2 c + 1 the - displacement of
pair c; in evaluation t pair c of graph g has job j = t r + c, active where j < 3 F_g: component j % 3 of free atom j / 3.

jacobi_ref: A <- (A + A^T) / 2; sweeps of the round-robin rounds rho = 0 .. m - 2 (m = d rounded up to even), round rho the
disjoint pairs (m - 1, rho), ((rho + k) mod (m - 1), (rho - k) mod (m - 1)), k = 1 .. m / 2 - 1, ordered p < q, a bye where
q >= d; all rotations of a round from the matrix at its start (a_pq == 0: none; theta = (a_qq - a_pp) / (2 a_pq),
t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), sign(0) = +1, c = 1 / sqrt(t^2 + 1), s = t c); all column updates, then all row
updates, then a_pp - t a_pq, a_qq + t a_pq and the zeros exactly; V's rows like A's; stop after a sweep with
off <= tol |A0|_F, or after max_sweeps; ascending by a stable sort; the largest component of each eigenvector positive, the
lowest index on a tie.  (The two norms are plain numpy sums: their order enters the result through the stop alone.)"""
import numpy as np


def round_pairs(m, rho):
    """The m / 2 pairs (p < q) of round rho for an even m."""
    pairs = [(m - 1, rho)] + [((rho + k) % (m - 1), (rho - k) % (m - 1)) for k in range(1, m // 2)]
    return [(min(p, q), max(p, q)) for p, q in pairs]


def jacobi_ref(a, tol=1e-15, max_sweeps=30):
    """-> (w [d], v [d, d] with row k the eigenvector of w[k], sweeps, status)."""
    a = np.array(a, dtype=np.float64)
    d = a.shape[0]
    if not np.isfinite(a).all():
        return np.full(d, np.nan), np.full((d, d), np.nan), 0, 2
    a = (a + a.T) * 0.5
    v = np.eye(d)
    norm0 = np.sqrt((a * a).sum())
    m = d + (d & 1)
    schedule = []
    for rho in range(m - 1):
        pq = np.asarray([(p, q) for p, q in round_pairs(m, rho) if q < d], dtype=np.int64).reshape(-1, 2)
        schedule.append((pq[:, 0], pq[:, 1]))
    done, converged = 0, False
    while done < max_sweeps and not converged:
        for P, Q in schedule:
            apq = a[P, Q]
            on = apq != 0.0
            if not on.any():
                continue
            P, Q, apq = P[on], Q[on], apq[on]
            app, aqq = a[P, P], a[Q, Q]
            with np.errstate(over='ignore', divide='ignore', invalid='ignore'):
                theta = (aqq - app) / (2.0 * apq)
                t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
            c = 1.0 / np.sqrt(t * t + 1.0)
            s = t * c
            x, y = a[:, P].copy(), a[:, Q].copy()                  # columns
            a[:, P], a[:, Q] = c * x - s * y, s * x + c * y
            x, y = a[P, :].copy(), a[Q, :].copy()                  # rows
            a[P, :], a[Q, :] = c[:, None] * x - s[:, None] * y, s[:, None] * x + c[:, None] * y
            a[P, P], a[Q, Q], a[P, Q], a[Q, P] = app - t * apq, aqq + t * apq, 0.0, 0.0
            x, y = v[P, :].copy(), v[Q, :].copy()
            v[P, :], v[Q, :] = c[:, None] * x - s[:, None] * y, s[:, None] * x + c[:, None] * y
        off = np.sqrt(((a - np.diag(np.diag(a))) ** 2).sum())
        done += 1
        converged = bool(off <= tol * norm0)
    w = np.diag(a).copy()
    order = np.argsort(w, kind='stable')
    w, v = w[order], v[order]
    for k in range(d):
        if v[k, int(np.argmax(np.abs(v[k])))] < 0.0:
            v[k] = -v[k]
    return w, v, done, 0 if converged else 1


def job_of(fptr, free_idx, g, pairs, t, c):
    """(atom, component, row) of pair c of graph g in evaluation t, or None where the pair is idle."""
    nf = int(fptr[g + 1]) - int(fptr[g])
    j = t * pairs + c
    if j >= 3 * nf:
        return None
    return int(free_idx[int(fptr[g]) + j // 3]), j % 3, j


def displace_ref(pos0, gptr, fptr, free_idx, pairs, t, delta):
    """pos_out fp32 [2 pairs n, 3]."""
    pos0 = np.asarray(pos0, dtype=np.float32)
    n = pos0.shape[0]
    out = np.tile(pos0, (2 * pairs, 1))
    for g in range(len(gptr) - 1):
        for c in range(pairs):
            job = job_of(fptr, free_idx, g, pairs, t, c)
            if job is None:
                continue
            a, comp, _ = job
            x0 = np.float64(pos0[a, comp])
            out[2 * c * n + a, comp] = np.float32(x0 + delta)
            out[(2 * c + 1) * n + a, comp] = np.float32(x0 - delta)
    return out


def rows_ref(dpos, pos0, masses, fptr, free_idx, moff, pairs, t, delta, h):
    """Stores the rows of evaluation t into the packed fp64 `h` (in place) -> the list of (graph, row) written."""
    dpos, pos0 = np.asarray(dpos, dtype=np.float32), np.asarray(pos0, dtype=np.float32)
    n = pos0.shape[0]
    written = []
    for g in range(len(fptr) - 1):
        f0, f1 = int(fptr[g]), int(fptr[g + 1])
        d = 3 * (f1 - f0)
        atoms = np.asarray(free_idx[f0:f1], dtype=np.int64)
        for c in range(pairs):
            job = job_of(fptr, free_idx, g, pairs, t, c)
            if job is None:
                continue
            a, comp, row = job
            x0 = np.float64(pos0[a, comp])
            sep = np.float64(np.float32(x0 + delta)) - np.float64(np.float32(x0 - delta))
            plus = dpos[2 * c * n + atoms].astype(np.float64).reshape(-1)
            minus = dpos[(2 * c + 1) * n + atoms].astype(np.float64).reshape(-1)
            ma = np.float64(masses[a]) if masses is not None else 1.0
            mb = np.repeat(np.asarray(masses, dtype=np.float32)[atoms].astype(np.float64), 3) if masses is not None else np.ones(d)
            lo = int(moff[g]) + row * d
            h[lo:lo + d] = (plus - minus) / sep / np.sqrt(ma * mb)
            written.append((g, row))
    return written


def layout(counts_free):
    """(dptr, moff) int64 of graphs with the given numbers of free atoms."""
    d = 3 * np.asarray(counts_free, dtype=np.int64)
    return np.concatenate([[0], np.cumsum(d)]).astype(np.int64), np.concatenate([[0], np.cumsum(d * d)]).astype(np.int64)
