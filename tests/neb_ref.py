"""neb_force_ref: the projection of pamnet_neb_force_f32 (include/pamnet_hip.h) restated in numpy, fp64 -- the reference of
tests/test_neb.py.  Image i = graph g of band b, neighbours -/+ = graphs g - 1 / g + 1, atoms matched by offset, F = -dE/dpos,
every sum over the free atoms of g (the image's own rows of `fixed` decide; rows of fixed atoms are never read, here or in the
neighbours, and their rows of dneb are 0):

  1. The first and last image of a band: dneb = 0 (the last image still reports seg).
  2. An interior image whose atom count differs from a neighbour's: free rows NaN, fpar = seg = NaN; a last image whose count
     differs from the previous image's has seg NaN.
  3. d+ = R_{i+1} - R_i, d- = R_i - R_{i-1}; Spp, Smm, Spm, Fp = F.d+, Fm = F.d-, F2; seg = sqrt(Smm).
  4. An energy of the three or a sum not finite: free rows NaN, fpar NaN.
  5. t = cp d+ + cm d-: rising (1, 0), falling (0, 1), else hi / lo = max / min of |E+ - E0|, |E- - E0|: E+ > E-: (hi, lo), else
     (lo, hi).  |t|^2 = cp^2 Spp + 2 cp cm Spm + cm^2 Smm; > 0: t^ = t / |t|, fpar = (cp Fp + cm Fm) / |t|; else t^ = 0, fpar = 0.
  6. climb[b]: the interior image of largest energy, scanning upward with `>` from -inf, has F_neb = F - 2 fpar t^.
  7. Else F_neb = F - fpar t^ + k (sqrt(Spp) - sqrt(Smm)) t^.

dneb = -F_neb, rounded to fp32 once."""
import numpy as np


def band_of_graphs(band_ptr, n_graphs):
    out = np.full(n_graphs, -1, dtype=np.int32)
    for b in range(len(band_ptr) - 1):
        out[max(int(band_ptr[b]), 0):min(int(band_ptr[b + 1]), n_graphs)] = b
    return out


def climbing_image(energy, first, last):
    """The graph index of the climbing image of the band first .. last (inclusive), or -1."""
    best, at = -np.inf, -1
    for i in range(first + 1, last):
        if float(energy[i]) > best:
            best, at = float(energy[i]), i
    return at


def neb_force_ref(pos, dE, energy, gptr, band_ptr, k, fixed=None, band_status=None, climb=None, out=None, diag=None):
    """pos, dE: float32 [n, 3]; energy: float32 [G]; gptr: [G + 1]; band_ptr: [B + 1]; k: a float or [B]; fixed: bool [n] or None;
    band_status: int [B] or None; climb: bool [B] or None; out: (dneb, seg, fpar) to start from (what an untouched band keeps),
    default zeros.  Returns new (dneb float32 [n, 3], seg, fpar float64 [G]).  diag: a dict that receives per graph the role,
    (cp, cm), t2 and the sums."""
    pos, dE = np.asarray(pos, dtype=np.float32), np.asarray(dE, dtype=np.float32)
    energy = np.asarray(energy, dtype=np.float32)
    n, G, B = pos.shape[0], len(gptr) - 1, len(band_ptr) - 1
    fixed = np.zeros(n, dtype=bool) if fixed is None else np.asarray(fixed).astype(bool)
    kb = np.broadcast_to(np.asarray(k, dtype=np.float64), (B,))
    if out is None:
        dneb, seg, fpar = np.zeros((n, 3), np.float32), np.zeros(G), np.zeros(G)
    else:
        dneb, seg, fpar = (np.array(o) for o in out)
    rng = lambda g: (max(int(gptr[g]), 0), min(int(gptr[g + 1]), n))
    for b in range(B):
        if band_status is not None and band_status[b] != 0:
            continue
        first, last = max(int(band_ptr[b]), 0), min(int(band_ptr[b + 1]) - 1, G - 1)
        top = climbing_image(energy, first, last) if climb is not None and climb[b] else -1
        for g in range(first, last + 1):
            lo, hi = rng(g)
            m = hi - lo
            rows = np.arange(lo, max(hi, lo))
            free = rows[~fixed[rows]]
            off = free - lo
            has_prev, has_next = g > first, g < last
            interior = has_prev and has_next
            rec = dict(role='interior' if interior else 'endpoint')
            if diag is not None:
                diag[g] = rec
            differs_prev = has_prev and (rng(g - 1)[1] - rng(g - 1)[0]) != m
            mismatched = interior and (differs_prev or (rng(g + 1)[1] - rng(g + 1)[0]) != m)
            with np.errstate(all='ignore'):
                if has_prev and not differs_prev and not mismatched:
                    dm = pos[free].astype(np.float64) - pos[rng(g - 1)[0] + off].astype(np.float64)
                    seg[g] = np.sqrt((dm * dm).sum())
                else:
                    seg[g] = np.nan if has_prev else 0.0
                dneb[rows] = 0.0
                if not interior:
                    fpar[g] = 0.0
                    continue
                if mismatched:
                    dneb[free], fpar[g], rec['role'] = np.nan, np.nan, 'mismatched'
                    continue
                dp = pos[rng(g + 1)[0] + off].astype(np.float64) - pos[free].astype(np.float64)
                F = -dE[free].astype(np.float64)
                Spp, Smm, Spm = (dp * dp).sum(), (dm * dm).sum(), (dp * dm).sum()
                Fp, Fm, F2 = (F * dp).sum(), (F * dm).sum(), (F * F).sum()
                Em, E0, Ep = float(energy[g - 1]), float(energy[g]), float(energy[g + 1])
                rec.update(Spp=Spp, Smm=Smm, Spm=Spm, Fp=Fp, Fm=Fm, F2=F2)
                if not np.all(np.isfinite([Em, E0, Ep, Spp, Smm, Spm, Fp, Fm, F2])):
                    dneb[free], fpar[g], rec['role'] = np.nan, np.nan, 'nonfinite'
                    continue
                if Ep > E0 > Em:
                    cp, cm, branch = 1.0, 0.0, 'rising'
                elif Ep < E0 < Em:
                    cp, cm, branch = 0.0, 1.0, 'falling'
                else:
                    up, dn = abs(Ep - E0), abs(Em - E0)
                    big, small = max(up, dn), min(up, dn)
                    (cp, cm), branch = ((big, small), 'extremum+') if Ep > Em else ((small, big), 'extremum-')
                t2 = (cp * cp) * Spp + 2.0 * (cp * cm) * Spm + (cm * cm) * Smm
                if t2 > 0.0:
                    norm = np.sqrt(t2)
                    that = (cp / norm) * dp + (cm / norm) * dm
                    fp = (cp * Fp + cm * Fm) / norm
                else:
                    that, fp = np.zeros_like(dp), 0.0
                climbing = g == top
                c = -2.0 * fp if climbing else float(kb[b]) * (np.sqrt(Spp) - np.sqrt(Smm)) - fp
                fpar[g] = fp
                dneb[free] = (-(F + c * that)).astype(np.float32)
                rec.update(branch=branch, cp=cp, cm=cm, t2=t2, that=that, climbing=climbing, free=free)
    return dneb, seg, fpar
