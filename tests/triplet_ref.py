"""Host reference of the triplet / pair row list and its transpose (csrc/graph.hip: triplet_count_kernel, triplet_fill,
triplet_transpose_kernel; include/pamnet_hip.h "Triplet / pair enumeration + angles").  numpy and the standard library only:
no torch device, no project kernel.  tests/test_hip_triplets.py compares the kernels with it element for element.

Input everywhere: a directed bond list as the kernels take it -- lptr [n + 1], src / dst [E], bond e = (src[e] -> dst[e]), grouped
by dst ascending (lptr[i] .. lptr[i + 1] are the bonds arriving at atom i), in ANY order inside a row; a bond may be listed more
than once.  PRECONDITION: no self-bonds (src[e] != dst[e]).  The kernels do not check it (the header says "No self loops"; the
graph routes strip them first); every function here asserts it, through check_input.

Row order (the header and the comment above triplet_fill): the rows of bond e = (j -> i) are [tp_ptr[e], tp_ptr[e + 1]);
first every q in lptr[j] .. lptr[j + 1] ascending with src[q] != i (kind 0: the triplet src[q] -> j -> i), then every q in
lptr[i] .. lptr[i + 1] ascending (kind 1: the pair (j, src[q]) -> i, e itself included).  tp_idx = q, tp_edge = e."""
from fractions import Fraction                  # noqa: F401  (the tests use it through this module as well)

import numpy as np

CAP = 16                  # triplet_transpose_kernel: both bond lists of an atom in registers up to this many entries each
PBC_ROW = 18              # doubles per graph in the cell table: the cell (row k = lattice vector a_k), then its inverse


def check_input(lptr, src, dst):
    """The input contract above; returns (n, E)."""
    lptr, src, dst = np.asarray(lptr), np.asarray(src), np.asarray(dst)
    n, E = len(lptr) - 1, len(src)
    assert n >= 0 and len(dst) == E and int(lptr[0]) == 0 and int(lptr[-1]) == E
    assert (np.diff(lptr) >= 0).all()
    if E:
        assert src.min() >= 0 and src.max() < n and dst.min() >= 0 and dst.max() < n
        assert np.array_equal(dst, np.repeat(np.arange(n), np.diff(lptr))), 'bonds are not grouped by dst ascending'
        assert (src != dst).all(), 'self-bond: outside the contract of the triplet kernels'
    return n, E


def group_by_dst(n, pairs):
    """(lptr, src, dst) int32 of a list of (src, dst) pairs: a stable sort by dst, so a row keeps the order of the listing."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    o = np.argsort(pairs[:, 1], kind='stable')
    src, dst = pairs[o, 0].astype(np.int32), pairs[o, 1].astype(np.int32)
    lptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=n))]).astype(np.int32)
    check_input(lptr, src, dst)
    return lptr, src, dst


def bond_transpose(src, n):
    """(lt_ptr, lt_perm): the bonds by SOURCE atom, ascending bond id inside a row."""
    src = np.asarray(src, dtype=np.int64)
    lt_perm = np.argsort(src, kind='stable').astype(np.int32)
    lt_ptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))]).astype(np.int32)
    return lt_ptr, lt_perm


# ---- the row list -------------------------------------------------------------------------------------------------------------
def counts(lptr, src, dst, with_triplets):
    """(tcount, tpcount) [E]: the rule of triplet_count_kernel."""
    n, E = check_input(lptr, src, dst)
    tcount, tpcount = np.zeros(E, np.int32), np.zeros(E, np.int32)
    for e in range(E):
        j, i = int(src[e]), int(dst[e])
        t = sum(1 for q in range(lptr[j], lptr[j + 1]) if src[q] != i) if with_triplets else 0
        tcount[e], tpcount[e] = t, t + (lptr[i + 1] - lptr[i])
    return tcount, tpcount


def rows(lptr, src, dst, with_triplets):
    """(tp_ptr [E + 1], tp_idx, tp_edge, tp_kind [T + P]) in the documented order."""
    n, E = check_input(lptr, src, dst)
    idx, edge, kind, ptr = [], [], [], [0]
    for e in range(E):
        j, i = int(src[e]), int(dst[e])
        if with_triplets:
            for q in range(lptr[j], lptr[j + 1]):
                if src[q] != i:
                    idx.append(q), edge.append(e), kind.append(0)
        for q in range(lptr[i], lptr[i + 1]):
            idx.append(q), edge.append(e), kind.append(1)
        ptr.append(len(idx))
    return tuple(np.asarray(a, dtype=np.int32) for a in (ptr, idx, edge, kind))


def transpose(tp_idx, E):
    """(tt_ptr [E + 1], tt_perm): a stable counting sort of tp_idx -- the rows that gather source bond q, ascending."""
    tp_idx = np.asarray(tp_idx, dtype=np.int64)
    tt_perm = np.argsort(tp_idx, kind='stable').astype(np.int32)
    tt_ptr = np.concatenate([[0], np.cumsum(np.bincount(tp_idx, minlength=E))]).astype(np.int32)
    return tt_ptr, tt_perm


def transpose_count(lptr, src, dst, with_triplets):
    """Rows that gather every bond q = (k -> j), from the bond lists alone (the rule of triplet_transpose_kernel<false>): a pair
    row of every bond arriving at j, and a triplet row of every bond leaving j towards an atom other than k."""
    n, E = check_input(lptr, src, dst)
    leaving, towards = {}, {}
    for e in range(E):
        leaving[int(src[e])] = leaving.get(int(src[e]), 0) + 1
        towards[int(src[e]), int(dst[e])] = towards.get((int(src[e]), int(dst[e])), 0) + 1
    out = np.zeros(E, np.int32)
    for q in range(E):
        k, j = int(src[q]), int(dst[q])
        out[q] = (lptr[j + 1] - lptr[j]) + ((leaving.get(j, 0) - towards.get((j, k), 0)) if with_triplets else 0)
    return out


def branch_table(lptr, src, dst, lt_ptr, with_triplets=True):
    """The form of triplet_transpose_kernel<true> every bond q = (k -> j) takes.  na = bonds leaving j (0 without triplets: the
    kernel then reads none of them), nb = bonds arriving at j; register form when na <= CAP and nb <= CAP, with pad_a = CAP - na
    and pad_b = CAP - nb padded slots; otherwise the loop form, because of 'a' (only na exceeds CAP), 'b' or 'ab'.
    Returns a dict of arrays over the bonds: na, nb, loop (bool), pad_a, pad_b (-1 in the loop form), why ('', 'a', 'b', 'ab')."""
    n, E = check_input(lptr, src, dst)
    lptr, lt_ptr = np.asarray(lptr, dtype=np.int64), np.asarray(lt_ptr, dtype=np.int64)
    j = np.asarray(dst, dtype=np.int64)
    na = (lt_ptr[j + 1] - lt_ptr[j]) if with_triplets else np.zeros(E, np.int64)
    nb = lptr[j + 1] - lptr[j]
    loop = (na > CAP) | (nb > CAP)
    why = np.where(na > CAP, np.where(nb > CAP, 'ab', 'a'), np.where(nb > CAP, 'b', ''))
    return dict(na=na, nb=nb, loop=loop, pad_a=np.where(loop, -1, CAP - na), pad_b=np.where(loop, -1, CAP - nb), why=why)


# ---- the angles ---------------------------------------------------------------------------------------------------------------
def _operands(a, b):
    """(y, x) = (|a x b|, a . b) of vectors [m, 3] as angle3 (csrc/geom_core.h) states them: every product and sum rounded to
    the vectors' own type on its own, sums associated (xx + yy) + zz, the root correctly rounded."""
    f = a.dtype.type
    assert f in (np.float32, np.float64) and b.dtype == a.dtype
    ax, ay, az, bx, by, bz = a[:, 0], a[:, 1], a[:, 2], b[:, 0], b[:, 1], b[:, 2]
    x = f(f(f(ax * bx) + f(ay * by)) + f(az * bz))
    cx, cy, cz = f(f(ay * bz) - f(az * by)), f(f(az * bx) - f(ax * bz)), f(f(ax * by) - f(ay * bx))
    y = np.sqrt(f(f(f(cx * cx) + f(cy * cy)) + f(cz * cz)))
    assert x.dtype == a.dtype and y.dtype == a.dtype
    return y, x


def row_vectors(bond_vec, tp_idx, tp_edge, tp_kind):
    """(a, b) of every row from bond_vec [E, 3] = p_src - p_dst of every bond.  Row (e, q): kind 0 -- a = p_j - p_i = v[e],
    b = p_k - p_j = v[q]; kind 1 -- a = p_i - p_j = -v[e] (a negation is exact), b = p_j' - p_i = v[q]."""
    e, q, kind = (np.asarray(t, dtype=np.int64) for t in (tp_edge, tp_idx, tp_kind))
    return np.where((kind == 1)[:, None], -bond_vec[e], bond_vec[e]).astype(bond_vec.dtype), bond_vec[q]


def _angles(bond_vec, tp_idx, tp_edge, tp_kind):
    y, x = _operands(*row_vectors(bond_vec, tp_idx, tp_edge, tp_kind))
    return (y, x), np.arctan2(y.astype(np.float64), x.astype(np.float64))


def angles_open(pos32, src, dst, tp_idx, tp_edge, tp_kind, operand_type=np.float32):
    """((y, x) fp32, theta64 = atan2(float64(y), float64(x))) of every row: open space, the fp32 differences of the positions.
    operand_type = np.float64: the same statements on the exact differences with operands in fp64 -- not what the kernels
    compute, but what an fp64 evaluation of the model's formula gives (the anchor to the oracle's angle_between)."""
    pos32 = np.asarray(pos32)
    assert pos32.dtype == np.float32
    p = pos32.astype(operand_type)
    v = p[np.asarray(src, dtype=np.int64)] - p[np.asarray(dst, dtype=np.int64)]
    return _angles(v.astype(operand_type).reshape(-1, 3), tp_idx, tp_edge, tp_kind)


def round_f32(v):
    """(the fp32 nearest to the Fraction v, ties to even; the distance of v from the nearest rounding tie, relative to |v|).
    Normal range only."""
    if v == 0:
        return np.float32(0.0), float('inf')
    mag = abs(v)
    e = mag.numerator.bit_length() - mag.denominator.bit_length()
    if Fraction(2) ** e > mag:
        e -= 1
    assert Fraction(2) ** e <= mag < Fraction(2) ** (e + 1) and -120 < e < 120
    quantum = Fraction(2) ** (e - 23)
    m = mag / quantum
    lo = m.numerator // m.denominator
    rem = m - lo
    up = rem > Fraction(1, 2) or (rem == Fraction(1, 2) and lo % 2 == 1)
    r = np.float32(float((lo + (1 if up else 0)) * quantum))            # (24 bits: exact in a double, exact in the cast)
    return (r if v > 0 else -r), float(abs(rem - Fraction(1, 2)) * quantum / mag)


def min_image_exact(pa, pb, row):
    """Minimum-image displacement p_a - p_b in exact rational arithmetic: pa, pb fp32 [3]; row: a graph's row of the cell table
    (its first nine doubles the cell, the next nine the inverse).  The image n = the fractional components d @ inverse rounded
    to the nearest integer; the displacement d - n @ cell uses the nine cell doubles alone.
    Returns (n [3] ints, fractional components [3], displacement [3]), the last two as Fractions."""
    d = [Fraction(float(pa[c])) - Fraction(float(pb[c])) for c in range(3)]
    cell, inv = [Fraction(float(v)) for v in row[:9]], [Fraction(float(v)) for v in row[9:18]]
    frac = [sum(d[m] * inv[3 * m + k] for m in range(3)) for k in range(3)]
    n = [round(f) for f in frac]                                         # (ties to even, as rint; the tests keep away from them)
    return n, frac, [d[c] - sum(n[k] * cell[3 * k + c] for k in range(3)) for c in range(3)]


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))               # (int / int division rounds correctly: one rounding)


def min_image_chain(pa, pb, row):
    """The same displacement by the statements of min_image (csrc/geom_core.h), every fma and product rounded to fp64 once:
    what the kernels hold before they round to fp32.  Returns (n [3], displacement [3]) as floats."""
    d = [float(pa[c]) - float(pb[c]) for c in range(3)]                  # (exact in fp64)
    c, inv = [float(v) for v in row[:9]], [float(v) for v in row[9:18]]
    n = [float(round(_fma(d[2], inv[6 + k], _fma(d[1], inv[3 + k], _fma(d[0], inv[k], 0.0))))) for k in range(3)]
    return n, [_fma(-n[2], c[6 + k], _fma(-n[1], c[3 + k], _fma(-n[0], c[k], d[k]))) for k in range(3)]


def bond_vectors_pbc(pos32, cell64, node_graph, src, dst):
    """Per bond (src -> dst): the minimum-image displacement p_src - p_dst rounded once to fp32 [E, 3], its image [E, 3], the
    smallest distance of a fractional component from a half-integer, and the smallest relative distance of an exact
    displacement component from an fp32 rounding tie."""
    pos32, cell64 = np.asarray(pos32), np.asarray(cell64, dtype=np.float64).reshape(-1, PBC_ROW)
    assert pos32.dtype == np.float32
    E = len(src)
    v, img, half, tie = np.zeros((E, 3), np.float32), np.zeros((E, 3), np.int64), float('inf'), float('inf')
    for e in range(E):
        a, b = int(src[e]), int(dst[e])
        assert node_graph[a] == node_graph[b]
        n, frac, disp = min_image_exact(pos32[a], pos32[b], cell64[int(node_graph[a])])
        img[e] = n
        for c in range(3):
            v[e, c], t = round_f32(disp[c])
            tie = min(tie, t)
            half = min(half, float(abs(abs(frac[c] - n[c]) - Fraction(1, 2))))
    return v, img, half, tie


def angles_pbc(pos32, cell64, node_graph, src, dst, tp_idx, tp_edge, tp_kind, bond_vec=None):
    """angles_open with both vectors of every row by the image rule: a and b are the exact minimum-image displacements rounded
    once to fp32 (the displacement of a reversed bond is the exact negation: every step of the rule is odd).  bond_vec: the
    first value of bond_vectors_pbc, when the caller has it already."""
    if bond_vec is None:
        bond_vec = bond_vectors_pbc(pos32, cell64, node_graph, src, dst)[0]
    return _angles(bond_vec, tp_idx, tp_edge, tp_kind)
