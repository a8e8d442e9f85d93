"""The step-by-step triplet / pair kernels of csrc/graph.hip -- pamnet_triplet_count_i32, pamnet_triplet_fill_f32,
pamnet_triplet_fill_pbc_f32, pamnet_triplet_transpose_count/fill_i32, pamnet_triplet_transpose_aux_i32, pamnet_expand_rows_i32 --
against the host reference of tests/triplet_ref.py, element for element and in the documented order.  The other two builders of
these lists (the molecule-local builder, the graph engine) are pinned to these kernels bit for bit elsewhere; here the kernels
themselves are pinned to lists and angles the host computes from the bond list alone.

Inputs: small, built on the host from a fixed seed, one per branch the kernels have (INPUTS below says what each is for);
`test_inputs_reach_every_form_of_the_transpose_kernel` proves with a host model of the kernel's branch condition that they do.
`dup` is kept: build_graph hands a user's bond list to these kernels as it is, duplicates included (tests/test_graph_engine.py
relies on it), so a bond listed twice is a legal input.

Host tests (no GPU): the inputs, the reference against the oracle.  GPU tests: marked `gpu`."""
import functools
import types
import zlib

import numpy as np
import pytest
import torch

import triplet_ref as R

gpu = pytest.mark.gpu

PI32 = np.float32(np.pi)
# |tp_angle - theta64| on every row but the self-pairs: atan2f within 2 ulp and ulp(pi) = 2**-22 -> at most 2 * 2**-23; the root
# may be one ulp off (the HIP headers map __fsqrt_rn to the native root) and enters through x y / (x^2 + y^2) <= 1/2 -> at most
# 2**-24; the sum rounded up.
ANGLE_TOL = 4 * 2.0 ** -23
I_SENT = -7                                               # outputs are pre-filled: -7 (int32), NaN (fp32)


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def _scatter(rng, n, min_sep=0.8, density=0.08, origin=(0.0, 0.0, 0.0)):
    """n points uniform in a cube at `density`, pairwise at least min_sep apart (rejection), fp32."""
    side = max(2.5, (n / density) ** (1.0 / 3.0))
    pts = np.zeros((0, 3))
    while len(pts) < n:
        p = rng.random(3) * side
        if len(pts) == 0 or np.sqrt(((pts - p) ** 2).sum(1)).min() >= min_sep:
            pts = np.vstack([pts, p])
    return (pts + np.asarray(origin)).astype(np.float32)


def _mols(rng):
    """12 bonded molecules of 3 .. 9 atoms: a random tree plus ring closures, degrees 1 .. 4, both directions of every bond.
    Returns (pairs as listed, positions, first atom of every molecule)."""
    sizes = [3, 9] + [int(s) for s in rng.integers(3, 10, size=10)]
    pairs, pos, first = [], [], [0]
    for m in sizes:
        base, deg, und = first[-1], np.zeros(m, int), set()
        order = rng.permutation(m)
        for t in range(1, m):
            free = [int(order[u]) for u in range(t) if deg[order[u]] < 4]
            a, b = free[int(rng.integers(len(free)))], int(order[t])
            und.add((min(a, b), max(a, b)))
            deg[a] += 1
            deg[b] += 1
        for _ in range(m):
            a, b = (int(v) for v in rng.integers(m, size=2))
            if a != b and deg[a] < 4 and deg[b] < 4 and (min(a, b), max(a, b)) not in und:
                und.add((min(a, b), max(a, b)))
                deg[a] += 1
                deg[b] += 1
        for a, b in sorted(und):
            pairs += [(base + a, base + b), (base + b, base + a)]
        pos.append(_scatter(rng, m, min_sep=0.9, density=0.35, origin=rng.random(3) * 20))
        first.append(base + m)
    return pairs, np.concatenate(pos), first


def _hub(rng, N):
    """A star: atom 0 bonded both ways with atoms 1 .. N, a few bonds among the leaves."""
    pairs = [(0, l) for l in range(1, N + 1)] + [(l, 0) for l in range(1, N + 1)]
    pairs += [(1, 2), (2, 1), (3, 4), (4, 3), (5, 6)]
    return N + 1, pairs


def _fan(n_in, n_out):
    """Atom 0 with n_in bonds arriving and n_out leaving, all one-way unless a partner is on both sides; the smaller side
    shares two partners with the larger one (so k == i skips happen) and has one of its own."""
    big = max(n_in, n_out)
    many, few = list(range(1, big + 1)), [1, 2, big + 1]
    assert min(n_in, n_out) == 3
    arriving, leaving = (many, few) if n_in > n_out else (few, many)
    pairs = [(k, 0) for k in arriving] + [(0, i) for i in leaving] + [(2, 3), (3, 2), (big + 1, 4)]
    return big + 2, pairs


def _clique(N):
    return N, [(a, b) for a in range(N) for b in range(N) if a != b]


def _sparse(rng, n, p, reverse):
    """Every unordered pair kept with probability p in one (random) direction; `reverse`: the share that gets the other too."""
    pairs = []
    for a in range(n):
        for b in range(a + 1, n):
            if rng.random() < p:
                s, d = (a, b) if rng.random() < 0.5 else (b, a)
                pairs.append((s, d))
                if rng.random() < reverse:
                    pairs.append((d, s))
    return n, pairs


def _holes(rng):
    """`mols` with atoms inserted that no bond arrives at: three at the start, runs of two and four in the middle, four at the
    end.  One of each run sends a single one-way bond into a molecule (bonds leaving only); the others have no bond at all,
    but for one atom near the end that a one-way bond arrives at (nothing leaves it).  The last two atoms have no bond."""
    pairs, pos, first = _mols(rng)
    n0 = first[-1]
    runs = {0: 3, first[4]: 2, first[8]: 4, n0: 4}                   # old index the run is inserted in front of -> its length
    new_of, inserted, at = np.zeros(n0 + 1, int), [], 0
    for old in range(n0 + 1):
        if old in runs:
            inserted.append(list(range(at, at + runs[old])))
            at += runs[old]
        new_of[old] = at
        at += 1
    n = n0 + sum(runs.values())
    out = [(int(new_of[a]), int(new_of[b])) for a, b in pairs]
    for run, target in zip(inserted, (first[1], first[5] + 1, first[9], first[11])):
        out.append((run[0], int(new_of[target])))                     # leaving only
    out.append((int(new_of[first[2]]), inserted[3][1]))              # arriving only
    p = np.zeros((n, 3), np.float32)
    p[new_of[:n0]] = pos
    ins = np.concatenate(inserted)
    p[ins] = _scatter(rng, len(ins), origin=(30.0, 30.0, 30.0))
    return n, out, p, inserted


def _blocks(rng):
    """A chain of 513 atoms bonded both ways and one one-way bond: 1025 bonds = four full workgroups and one thread.  The first
    64 atoms stand on a line (|a x b| == 0 exactly: angle 0 -- and pi on the rows of the one-way bond 10 -> 12, the only rows
    other than self-pairs whose vectors oppose each other), the others are scattered."""
    n = 513
    pairs = [(a, a + 1) for a in range(n - 1)] + [(a + 1, a) for a in range(n - 1)] + [(10, 12)]
    pos = np.concatenate([np.stack([np.arange(64) * 1.25, np.full(64, 0.5), np.full(64, -2.0)], 1).astype(np.float32),
                          _scatter(rng, n - 64, origin=(100.0, 0.0, 0.0))])
    return n, pairs, pos


INPUTS = {
    'mols': 'the usual case: 12 bonded molecules of 3 .. 9 atoms, degrees 1 .. 4',
    'hub15': 'a star, both bond lists of the hub below CAP', 'hub16': 'at CAP', 'hub17': 'over CAP',
    'in17_out3': 'only the arriving list of an atom exceeds CAP', 'in3_out17': 'only the leaving list does',
    'clique16': 'register form, one padded slot', 'clique17': 'register form without padding', 'clique18': 'loop form, dense',
    'one_way': 'no reverse bond anywhere: k == i never skips', 'half_way': 'half of the bonds have their reverse',
    'holes': 'empty rows of lptr and lt_ptr at the start, in the middle and at the end',
    'blocks': '1025 bonds: five workgroups, the last holding one thread',
    'dup': 'mols with four bonds listed twice',
    'empty': '7 atoms, no bond: the early returns',
}
NAMES = tuple(INPUTS)
PBC_NAMES = ('mols', 'hub17', 'one_way')                # their atoms under periodic boundaries: see PbcHost
WT = (1, 0)


class Host(object):
    """What the host reference says about one bond list with positions; every array read-only, made once."""

    def __init__(self, n, lptr, src, dst, pos, seed):
        self.n, self.E, self.lptr, self.src, self.dst, self.pos = n, len(src), lptr, src, dst, np.ascontiguousarray(pos, np.float32)
        assert self.pos.shape == (n, 3)
        self.lt_ptr, self.lt_perm = R.bond_transpose(src, n)
        rng = np.random.default_rng([7, seed])
        self.lt_shuffled = self.lt_perm.copy()                       # every row in an order of its own (the kNN route's rows)
        for a in range(n):
            rng.shuffle(self.lt_shuffled[self.lt_ptr[a]:self.lt_ptr[a + 1]])
        self._refs = {}

    def ref(self, wt):
        if wt not in self._refs:
            r = types.SimpleNamespace()
            r.tcount, r.tpcount = R.counts(self.lptr, self.src, self.dst, wt)
            r.tp_ptr, r.tp_idx, r.tp_edge, r.tp_kind = R.rows(self.lptr, self.src, self.dst, wt)
            r.tot = int(r.tp_ptr[-1])
            r.tt_ptr, r.tt_perm = R.transpose(r.tp_idx, self.E)
            r.self_pair = (r.tp_kind == 1) & (r.tp_idx == r.tp_edge)
            for a in vars(r).values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self._refs[wt] = r
        return self._refs[wt]

    def angles(self, wt):
        r = self.ref(wt)
        if not hasattr(r, 'theta'):
            r.operands, r.theta = R.angles_open(self.pos, self.src, self.dst, r.tp_idx, r.tp_edge, r.tp_kind)
        return r.operands, r.theta


@functools.lru_cache(maxsize=None)
def _listing(name):
    """(n, bonds as listed, positions or None, extra) of an input before its bonds are grouped."""
    rng = np.random.default_rng([20240917, zlib.crc32(name.encode())])
    extra = None
    if name in ('mols', 'dup'):
        pairs, pos, extra = _mols(np.random.default_rng([20240917, zlib.crc32(b'mols')]))
        n = extra[-1]
        if name == 'dup':                                            # a bond and its reverse, and two more, listed twice
            a, b = pairs[0]
            twice = [(a, b), (b, a), pairs[len(pairs) // 2], pairs[-1]]
            assert len(set(twice)) == 4
            pairs = pairs + twice
    elif name[:3] == 'hub':
        (n, pairs), pos = _hub(rng, int(name[3:])), None
    elif name == 'in17_out3':
        (n, pairs), pos = _fan(17, 3), None
    elif name == 'in3_out17':
        (n, pairs), pos = _fan(3, 17), None
    elif name[:6] == 'clique':
        (n, pairs), pos = _clique(int(name[6:])), None
    elif name == 'one_way':
        (n, pairs), pos = _sparse(rng, 60, 0.1, 0.0), None
    elif name == 'half_way':
        (n, pairs), pos = _sparse(rng, 60, 0.1, 0.5), None
    elif name == 'holes':
        n, pairs, pos, extra = _holes(np.random.default_rng([20240917, zlib.crc32(b'mols')]))
    elif name == 'blocks':
        n, pairs, pos = _blocks(rng)
    else:
        assert name == 'empty'
        n, pairs, pos = 7, [], None
    if pos is None:
        pos = _scatter(rng, n)
    pairs = [pairs[int(p)] for p in rng.permutation(len(pairs))]     # listed in any order: so are the rows of lptr
    return n, pairs, pos, extra


@functools.lru_cache(maxsize=None)
def host(name):
    n, pairs, pos, _ = _listing(name)
    return Host(n, *R.group_by_dst(n, pairs), pos, zlib.crc32(name.encode()))


# periodic inputs: heights above 4.0 = 2 * the bond cutoff; off-diagonal components of both signs in the triclinic cell
CUBE = [[4.5, 0.0, 0.0], [0.0, 4.5, 0.0], [0.0, 0.0, 4.5]]
BOX = [[4.5, 0.0, 0.0], [0.0, 5.25, 0.0], [0.0, 0.0, 4.75]]
TRI = [[5.0, 0.0, 0.0], [1.0, 5.0, 0.0], [-0.75, 0.875, 5.0]]
CELLS = np.array([CUBE, BOX, TRI], dtype=np.float32)
PBC_CUT = 2.0


def _host_table(cells32):
    """The cell table as the host makes it: the fp32 cell as doubles, then numpy's fp64 inverse (frac = d @ inverse)."""
    c = np.asarray(cells32, dtype=np.float32).astype(np.float64).reshape(-1, 3, 3)
    return np.concatenate([c.reshape(-1, 9), np.linalg.inv(c).reshape(-1, 9)], 1)


def _heights(cell):
    c = np.asarray(cell, dtype=np.float64)
    return [abs(np.linalg.det(c)) / np.linalg.norm(np.cross(c[(k + 1) % 3], c[(k + 2) % 3])) for k in range(3)]


def _min_image64(pos32, cell64):
    """fp64 brute force: (vectors [m, m, 3] of p_a - p_b, images [m, m, 3], distances [m, m]) of one graph."""
    p = pos32.astype(np.float64)
    d = p[:, None, :] - p[None, :, :]
    n = np.rint(d @ np.linalg.inv(cell64))
    v = d - n @ cell64
    return v, n, np.sqrt((v ** 2).sum(-1))


def _radius_pairs(pos32, gptr, cut, cells64=None):
    """Bonds (b -> a) for every ordered pair of one graph within `cut` (minimum image in a cell), fp64 from the fp32 positions;
    also the smallest |distance - cut| over all pairs."""
    pairs, margin = [], np.inf
    for g in range(len(gptr) - 1):
        s, e = int(gptr[g]), int(gptr[g + 1])
        if cells64 is None:
            p = pos32[s:e].astype(np.float64)
            d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))
        else:
            d = _min_image64(pos32[s:e], cells64[g])[2]
        off = ~np.eye(e - s, dtype=bool)
        margin = min(margin, float(np.abs(d[off] - cut).min())) if off.any() else margin
        a, b = np.nonzero((d <= cut) & off)
        pairs += [(int(y) + s, int(x) + s) for x, y in zip(a, b)]
    return pairs, margin


class PbcHost(Host):
    """The atoms of an open input in three cells: positions scattered in a cube, a box and a triclinic cell (the last graph's
    atoms displaced by whole lattice vectors: unwrapped input), bonds = minimum-image distance <= 2.0.  `mols` and `one_way`
    spread their atoms over the three cells.  `hub17` puts its 18 atoms into EVERY cell: a hub near the cell's corner and the 17
    others within the cutoff of it, wrapped into the cell -- an atom with 17 bonds each way under periodic boundaries (the loop
    form of the transpose on a periodic bond list), its neighbours in all eight octants around the corner."""

    def __init__(self, name):
        n = host(name).n
        rng = np.random.default_rng([20240918, zlib.crc32(name.encode())])
        hub = name == 'hub17'
        self.gptr = np.array([0, n, 2 * n, 3 * n] if hub else [0, n // 3, 2 * (n // 3), n], np.int32)
        n = int(self.gptr[-1])
        self.node_graph = np.repeat(np.arange(3, dtype=np.int32), np.diff(self.gptr))
        self.cells = CELLS
        self.table = _host_table(CELLS)
        cells64 = CELLS.astype(np.float64)
        pos = []
        for g in range(3):
            m, pts = int(self.gptr[g + 1] - self.gptr[g]), np.zeros((0, 3), np.float32)
            while len(pts) < m:
                if not hub:
                    p = rng.random(3) @ cells64[g]
                elif len(pts) == 0:
                    p = (rng.random(3) * 0.1) @ cells64[g]
                else:                                                 # uniform in the ball of radius 1.95 around the hub
                    v = (rng.random(3) * 2.0 - 1.0) * 1.95
                    if (v * v).sum() > 1.95 * 1.95:
                        continue
                    p = pts[0].astype(np.float64) + v
                    f = p @ np.linalg.inv(cells64[g])
                    p = (f - np.floor(f)) @ cells64[g]
                if g == 2 and (len(pts) or not hub):                  # (the hub itself stays: the ball is drawn around pts[0])
                    p = p + rng.integers(-2, 3, size=3).astype(np.float64) @ cells64[g]
                q = np.vstack([pts, p.astype(np.float32)[None]])
                if len(q) > 1:
                    d = _min_image64(q, cells64[g])[2][-1, :-1]
                    near = np.flatnonzero(d <= PBC_CUT + 0.01)
                    # one in twenty exact displacement components of random fp32 positions IS a rounding tie (25 significant
                    # bits): a candidate with one towards an atom it would be bonded to is drawn again
                    if d.min() < 0.7 or R.bond_vectors_pbc(q, self.table[g], np.zeros(len(q), np.int32),
                                                           [len(q) - 1] * len(near), near)[3] < 2.0 ** -40:
                        continue
                pts = q
            pos.append(pts)
        pos = np.concatenate(pos)
        pairs, self.cut_margin = _radius_pairs(pos, self.gptr, PBC_CUT, cells64)
        Host.__init__(self, n, *R.group_by_dst(n, pairs), pos, zlib.crc32(name.encode()) + 1)
        self._vec = {}

    def bond_vectors(self, table):
        key = np.asarray(table, np.float64).tobytes()
        if key not in self._vec:
            self._vec[key] = R.bond_vectors_pbc(self.pos, table, self.node_graph, self.src, self.dst)
        return self._vec[key]

    def angles_with(self, wt, table):
        r = self.ref(wt)
        return R.angles_pbc(self.pos, table, self.node_graph, self.src, self.dst, r.tp_idx, r.tp_edge, r.tp_kind,
                            bond_vec=self.bond_vectors(table)[0])


@functools.lru_cache(maxsize=None)
def pbc_host(name):
    return PbcHost(name)


ALL_NAMES = NAMES + tuple('pbc:' + p for p in PBC_NAMES)


def any_host(name):
    return pbc_host(name[4:]) if name[:4] == 'pbc:' else host(name)


# ---- host tests: the inputs do what INPUTS claims --------------------------------------------------------------------------
def test_inputs_are_what_the_table_says():
    pairs, pos, first = _listing('mols')[1], _listing('mols')[2], _listing('mols')[3]
    sizes = np.diff(first)
    assert len(sizes) == 12 and sizes.min() == 3 and sizes.max() == 9
    h = host('mols')
    assert set(pairs) == {(b, a) for a, b in pairs} and len(set(pairs)) == len(pairs)                  # symmetric, simple
    assert set(np.diff(h.lptr).tolist()) == {1, 2, 3, 4}
    mol = np.repeat(np.arange(12), sizes)
    assert (mol[h.src] == mol[h.dst]).all()
    for N in (15, 16, 17):
        h = host('hub%d' % N)
        assert h.lptr[1] - h.lptr[0] == N and h.lt_ptr[1] - h.lt_ptr[0] == N and h.E > 2 * N
    h = host('in17_out3')
    assert (h.lptr[1], h.lt_ptr[1]) == (17, 3)
    h = host('in3_out17')
    assert (h.lptr[1], h.lt_ptr[1]) == (3, 17)
    for N in (16, 17, 18):
        assert host('clique%d' % N).E == N * (N - 1)
    h = host('one_way')
    fwd = set(zip(h.src.tolist(), h.dst.tolist()))
    assert h.n == 60 and h.E > 120 and not any((d, s) in fwd for s, d in fwd)
    h = host('half_way')
    fwd = set(zip(h.src.tolist(), h.dst.tolist()))
    share = sum((d, s) in fwd for s, d in fwd) / float(len(fwd))
    assert h.n == 60 and 0.4 < share < 0.9                           # (half of the pairs: two thirds of the bonds)
    h, inserted = host('holes'), _listing('holes')[3]
    arriving, leaving = np.diff(h.lptr), np.diff(h.lt_ptr)
    assert inserted[0][0] == 0 and inserted[-1][-1] == h.n - 1 and [len(r) for r in inserted] == [3, 2, 4, 4]
    assert all(0 < r[0] and r[-1] < h.n - 1 for r in inserted[1:3])
    for run in inserted:
        assert arriving[run[0]] == 0 and leaving[run[0]] == 1        # bonds leaving only
        assert all(arriving[a] == 0 and leaving[a] == 0 for a in run[2:])
    assert arriving[inserted[3][1]] == 1 and leaving[inserted[3][1]] == 0 and h.E == host('mols').E + 5
    h = host('blocks')
    assert h.n == 513 and h.E == 1025 and (h.E + 255) // 256 == 5 and h.E % 256 == 1
    h = host('dup')
    listed = list(zip(h.src.tolist(), h.dst.tolist()))
    assert len(listed) - len(set(listed)) == 4 and h.E == host('mols').E + 4
    assert host('empty').n == 7 and host('empty').E == 0 and host('empty').ref(1).tot == 0
    assert max(host(name).ref(1).tot for name in NAMES) == host('clique18').ref(1).tot == 18 * 17 * 33
    for name in ('mols', 'hub17', 'clique18', 'one_way'):            # the shuffled transposed bond list is another order
        assert not np.array_equal(host(name).lt_perm, host(name).lt_shuffled)


def test_inputs_reach_every_form_of_the_transpose_kernel():
    """branch_table over every input: the register form with no padded slot on either side, with 15 padded slots on either side,
    the loop form because of the leaving list alone, of the arriving list alone, and of both.  Prints the table."""
    seen = dict(full=0, pad15_a=0, pad15_b=0, a=0, b=0, ab=0)
    print()
    print('%-10s %6s %7s %9s %5s %5s %5s  %s'
          % ('input', 'bonds', 'rows', 'register', 'a', 'b', 'ab', 'padded slots (leaving, arriving)'))
    for name in ALL_NAMES:
        h = any_host(name)
        t = R.branch_table(h.lptr, h.src, h.dst, h.lt_ptr)
        reg = ~t['loop']
        why = {w: int((t['why'] == w).sum()) for w in ('a', 'b', 'ab')}
        pads = ('%d..%d, %d..%d' % (t['pad_a'][reg].min(), t['pad_a'][reg].max(), t['pad_b'][reg].min(), t['pad_b'][reg].max())
                if reg.any() else '-')
        print('%-10s %6d %7d %9d %5d %5d %5d  %s' % (name, h.E, h.ref(1).tot, int(reg.sum()), why['a'], why['b'], why['ab'], pads))
        assert int(reg.sum()) + sum(why.values()) == h.E
        if name[:4] == 'pbc:':
            continue
        seen['full'] += int((reg & (t['pad_a'] == 0) & (t['pad_b'] == 0)).sum())
        seen['pad15_a'] += int((reg & (t['pad_a'] == 15)).sum())
        seen['pad15_b'] += int((reg & (t['pad_b'] == 15)).sum())
        for w in why:
            seen[w] += why[w]
        none = R.branch_table(h.lptr, h.src, h.dst, h.lt_ptr, with_triplets=False)      # pairs only: the leaving list is not read
        assert (none['na'] == 0).all() and np.array_equal(none['loop'], t['nb'] > R.CAP)
    assert all(v > 0 for v in seen.values()), seen
    h = host('hub16')
    assert not R.branch_table(h.lptr, h.src, h.dst, h.lt_ptr)['loop'].any()
    for name, w in (('in17_out3', 'b'), ('in3_out17', 'a'), ('hub17', 'ab'), ('clique18', 'ab')):
        h = host(name)
        t = R.branch_table(h.lptr, h.src, h.dst, h.lt_ptr)
        assert set(t['why'][t['loop']].tolist()) == {w} and t['loop'].any() and (name == 'clique18' or (~t['loop']).any())


@pytest.mark.parametrize('wt', WT)
def test_transpose_count_equals_the_row_lengths_of_the_transpose(wt):
    for name in ALL_NAMES:
        h = any_host(name)
        r = h.ref(wt)
        assert np.array_equal(R.transpose_count(h.lptr, h.src, h.dst, wt), np.diff(r.tt_ptr)), name
        assert np.array_equal(r.tp_idx[r.tt_perm], np.repeat(np.arange(h.E), np.diff(r.tt_ptr)))
        assert np.array_equal(np.diff(r.tp_ptr), r.tpcount) and np.array_equal(r.tp_edge, np.repeat(np.arange(h.E), r.tpcount))
        assert int((r.tp_kind == 0).sum()) == int(r.tcount.sum())
        for q in range(h.E):                                         # rows ascending inside a source bond
            rows = r.tt_perm[r.tt_ptr[q]:r.tt_ptr[q + 1]]
            assert (np.diff(rows) > 0).all()


def test_reference_refuses_a_self_bond():
    with pytest.raises(AssertionError, match='self-bond'):
        R.counts(np.array([0, 1, 2]), np.array([1, 1]), np.array([0, 1]), 1)
    with pytest.raises(AssertionError, match='grouped'):
        R.rows(np.array([0, 1, 2]), np.array([0, 1]), np.array([1, 0]), 1)


# the fp32 operands of theta64 against an fp64 evaluation of the same vectors: x carries three products and two sums, each
# rounded within 2**-24 of |a| |b| at most -> 3 u |a| |b|; a component of the cross product likewise, so |a x b| 3 sqrt(3) u, and
# its squares, sums and root 3 u more; an error (dx, dy) of the operands turns the angle by at most |(dx, dy)| / (|a| |b|)
# = sqrt(3^2 + 8.2^2) u < 9 u, u = 2**-24.  The oracle side takes the exact fp64 differences of the positions, theta64 their
# fp32 roundings: |da| <= u |a| and |db| <= u |b| turn each vector by at most u, the angle between them by at most 2 u more.
OPERAND_TOL = 11 * 2.0 ** -24


def _all_hosts():
    return [(name, host(name)) for name in NAMES] + [('pbc:' + name, pbc_host(name)) for name in PBC_NAMES]


def test_reference_matches_the_oracle():
    """Without duplicate bonds: the (k, j, i) and (j, i, j') key sets and the counts of PAMNet.indices; the angles of the oracle's
    angle_between in fp64 on the same vectors -- the reference's statements evaluated in fp64 to 1e-12 (vectors, signs and
    formula are the model's), and theta64, whose operands are rounded to fp32 as the kernel's are, within OPERAND_TOL."""
    from oracle import pamnet_oracle as O
    checked = 0
    for name, h in _all_hosts():
        if name in ('dup', 'empty'):
            continue
        r = h.ref(1)
        ei = torch.from_numpy(np.stack([h.src, h.dst]).astype(np.int64))
        (idx_i, idx_j, idx_k, idx_kj, idx_ji, i_p, j1_p, j2_p, jj_p, ji_p) = O.indices(ei, h.n)
        assert int(idx_kj.numel()) == int(r.tcount.sum()) and int(jj_p.numel()) == int((r.tp_kind == 1).sum())
        assert int(jj_p.numel()) == h.ref(0).tot and np.array_equal(h.ref(0).tp_idx, r.tp_idx[r.tp_kind == 1])
        t, p = r.tp_kind == 0, r.tp_kind == 1
        mine_t = list(zip(h.src[r.tp_idx[t]].tolist(), h.src[r.tp_edge[t]].tolist(), h.dst[r.tp_edge[t]].tolist()))
        mine_p = list(zip(h.src[r.tp_edge[p]].tolist(), h.dst[r.tp_edge[p]].tolist(), h.src[r.tp_idx[p]].tolist()))
        ref_t = list(zip(idx_k.tolist(), idx_j.tolist(), idx_i.tolist()))
        ref_p = list(zip(i_p.tolist(), j1_p.tolist(), j2_p.tolist()))
        assert len(set(mine_t)) == len(mine_t) == len(ref_t) and set(mine_t) == set(ref_t), name
        assert len(set(mine_p)) == len(mine_p) == len(ref_p) and set(mine_p) == set(ref_p), name
        # the oracle's edge ids are ours: idx_kj / idx_ji and the pair columns name the same bonds
        assert set(zip(idx_kj.tolist(), idx_ji.tolist())) == set(zip(r.tp_idx[t].tolist(), r.tp_edge[t].tolist()))
        assert set(zip(jj_p.tolist(), ji_p.tolist())) == set(zip(r.tp_idx[p].tolist(), r.tp_edge[p].tolist()))
        if name[:4] == 'pbc:':
            continue                                                  # (the oracle has no cells: their angles are anchored below)
        pos = torch.from_numpy(h.pos).double()
        want = dict(zip(ref_t, O.angle_between(pos[idx_j] - pos[idx_i], pos[idx_k] - pos[idx_j]).tolist()))
        want_p = dict(zip(ref_p, O.angle_between(pos[j1_p] - pos[i_p], pos[j2_p] - pos[j1_p]).tolist()))
        _, th64 = R.angles_open(h.pos, h.src, h.dst, r.tp_idx, r.tp_edge, r.tp_kind, operand_type=np.float64)
        _, th = h.angles(1)
        o = np.zeros(r.tot)
        o[t], o[p] = [want[k] for k in mine_t], [want_p[k] for k in mine_p]
        assert np.abs(th64 - o).max() < 1e-12, (name, np.abs(th64 - o).max())
        assert np.abs(th - o).max() < OPERAND_TOL, (name, np.abs(th - o).max())
        checked += r.tot
    assert checked > 20000


def test_no_angle_is_undefined_and_the_edge_values_occur():
    """No operand pair is (0, 0); self-pairs have y == 0 exactly and x < 0; the collinear atoms of `blocks` give y == 0 with both
    signs of x on rows that are not self-pairs."""
    for name, h in _all_hosts():
        for wt in WT:
            r = h.ref(wt)
            if name[:4] == 'pbc:':
                (y, x), th = h.angles_with(wt, h.table)
            else:
                (y, x), th = h.angles(wt)
            assert not ((x == 0) & (y == 0)).any(), name
            assert (y[r.self_pair] == 0).all() and (x[r.self_pair] < 0).all() and (th[r.self_pair] == np.pi).all()
            assert int(r.self_pair.sum()) == h.E
    r = host('blocks').ref(1)
    (y, x), th = host('blocks').angles(1)
    flat = (y == 0) & ~r.self_pair
    assert (flat & (x > 0)).sum() > 50 and (flat & (x < 0)).sum() > 0 and (th[flat & (x > 0)] == 0).all()
    assert (th[flat & (x < 0)] == np.pi).all()


@pytest.mark.parametrize('name', PBC_NAMES)
def test_periodic_inputs_meet_their_preconditions(name):
    """Cells with heights above twice the bond cutoff; no pair within 1e-6 of the cutoff; bonds and triplets across a face in
    every input; every fractional component at least 1e-3 from a half-integer; every exact displacement component at least
    2**-40 of its magnitude from an fp32 rounding tie -- which makes the fp64 fma chain of min_image and the exact value round to
    the same fp32, shown here statement by statement as well; and some components do need the rounding."""
    h = pbc_host(name)
    # the inputs are fixed by their seeds: (bonds, rows with triplets) as the commit that added them records them
    assert (h.E, h.ref(1).tot) == {'mols': (590, 9262), 'hub17': (510, 9978), 'one_way': (318, 3402)}[name]
    if name == 'hub17':                                              # a hub in every cell: 17 bonds arrive, 17 leave
        assert h.n == 54 and all(h.lptr[a + 1] - h.lptr[a] == 17 == h.lt_ptr[a + 1] - h.lt_ptr[a] for a in (0, 18, 36))
        assert (R.branch_table(h.lptr, h.src, h.dst, h.lt_ptr)['why'] == 'ab').sum() == 51
    assert all(min(_heights(c)) > 2 * PBC_CUT for c in CELLS) and min(_heights(TRI)) < 5.0
    assert any(v > 0 for v in np.ravel(TRI)[[3, 6, 7]]) and any(v < 0 for v in np.ravel(TRI)[[3, 6, 7]])
    assert h.cut_margin > 1e-6 and h.E > 0
    assert set(zip(h.src.tolist(), h.dst.tolist())) == set(zip(h.dst.tolist(), h.src.tolist()))
    vec, img, half, tie = h.bond_vectors(h.table)
    assert half >= 1e-3 and tie >= 2.0 ** -40, (half, tie)
    crossing = (img != 0).any(1)
    r = h.ref(1)
    trip = r.tp_kind == 0
    assert crossing.any() and (trip & (crossing[r.tp_edge] | crossing[r.tp_idx])).any()
    assert np.abs(img).max() >= 2                                    # the unwrapped graph: images beyond the neighbouring cell
    for g in range(3):
        assert crossing[h.node_graph[h.dst] == g].any(), g
    assert (np.sqrt((vec.astype(np.float64) ** 2).sum(1)) <= PBC_CUT + 1e-6).all()
    inexact = 0
    rev = {(int(s), int(d)): e for e, (s, d) in enumerate(zip(h.src, h.dst))}
    for e in range(h.E):
        a, b = int(h.src[e]), int(h.dst[e])
        n, d = R.min_image_chain(h.pos[a], h.pos[b], h.table[h.node_graph[a]])
        assert [int(v) for v in n] == img[e].tolist()
        exact = R.min_image_exact(h.pos[a], h.pos[b], h.table[h.node_graph[a]])[2]
        inexact += sum(R.Fraction(float(vec[e, c])) != exact[c] for c in range(3))
        assert np.array_equal(np.array(d, dtype=np.float64).astype(np.float32).view(np.uint32), vec[e].view(np.uint32)), e
        assert np.array_equal(vec[rev[b, a]], -vec[e])               # the reversed bond: the exact negation
    assert inexact > 0
    v64 = np.concatenate([_min_image64(h.pos[s:e], CELLS[g].astype(np.float64))[0][h.src[h.node_graph[h.dst] == g] - s,
                                                                                  h.dst[h.node_graph[h.dst] == g] - s]
                          for g, (s, e) in enumerate(zip(h.gptr[:-1], h.gptr[1:]))])
    assert np.abs(v64 - vec).max() < 1e-6                            # the brute force that chose the bonds: the same vectors


def test_a_wide_cell_gives_the_open_vectors():
    """With every image 0 the exact displacement rounds to the fp32 difference of the positions: the host side of the header's
    promise that the periodic kernel then returns the open kernel's floats."""
    h = host('half_way')
    table = _host_table(np.eye(3, dtype=np.float32)[None] * np.float32(1e4))
    vec, img, half, _ = R.bond_vectors_pbc(h.pos, table, np.zeros(h.n, np.int32), h.src, h.dst)
    assert not img.any() and np.array_equal(vec.view(np.uint32), (h.pos[h.src] - h.pos[h.dst]).view(np.uint32))


# ---- GPU tests ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs an MI355X'
    from pamnet_amd import lib
    lib.load()                                    # fail loudly if the HIP library is missing
    return torch.device('cuda:0')


_ON = {}


def on(dev, h):
    """The input's arrays on the device (uploaded once, never written)."""
    if id(h) not in _ON:
        d = types.SimpleNamespace()
        for k in ('lptr', 'src', 'dst', 'pos', 'lt_ptr', 'lt_perm', 'lt_shuffled'):
            setattr(d, k, up(dev, getattr(h, k)))
        if hasattr(h, 'node_graph'):
            d.node_graph = up(dev, h.node_graph)
        _ON[id(h)] = d
    return _ON[id(h)]


def ref_on(dev, h, wt):
    """The host lists the kernels take as inputs, on the device -- uploaded once and KEPT: a tensor made inside a call's argument
    list is freed before the kernel runs, and the next one takes its memory."""
    d = on(dev, h)
    if not hasattr(d, 'refs'):
        d.refs = {}
    if wt not in d.refs:
        r, t = h.ref(wt), types.SimpleNamespace()
        for k in ('tp_ptr', 'tcount', 'tt_ptr', 'tt_perm', 'tp_edge'):
            setattr(t, k, up(dev, getattr(r, k)))
        d.refs[wt] = t
    return d.refs[wt]


def up(dev, a):
    return torch.from_numpy(np.array(a)).to(dev)         # (a copy: the host's arrays are read-only)


def ints(dev, m):
    return torch.full((m,), I_SENT, dtype=torch.int32, device=dev)


def nans(dev, m):
    return torch.full((m,), float('nan'), dtype=torch.float32, device=dev)


def same(got, want):
    got = got.cpu().numpy()
    return got.dtype == np.asarray(want).dtype and np.array_equal(got, want)


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _fill(dev, h, wt, cap=None, table=None, node_graph=None):
    """pamnet_triplet_fill_f32 (or the periodic form) with the host's tp_ptr into sentinel-filled arrays of the full size."""
    from pamnet_amd import lib
    P, d, r = lib.ptr, on(dev, h), h.ref(wt)
    out = (ints(dev, r.tot), ints(dev, r.tot), nans(dev, r.tot), ints(dev, r.tot))
    tail = (P(d.lptr), P(d.src), P(d.dst), h.E, wt, P(ref_on(dev, h, wt).tp_ptr), P(out[0]), P(out[1]), P(out[2]), P(out[3]),
            r.tot if cap is None else cap, lib.stream_of(d.pos))
    if table is None:
        lib.call('pamnet_triplet_fill_f32', P(d.pos), *tail)
    else:
        lib.call('pamnet_triplet_fill_pbc_f32', P(d.pos), P(table), P(node_graph), *tail)
    return out                                                       # tp_idx, tp_edge, tp_angle, tp_kind


_WORST = {}


def _assert_angles(tag, name, r, got, operands, theta):
    """Self-pair rows bitwise pi, every other row within ANGLE_TOL of theta64; keeps and prints the worst error seen."""
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and not np.isnan(got).any()
    assert (bits(got[r.self_pair]) == bits(PI32)).all(), (name, got[r.self_pair][:4])
    err = np.abs(got.astype(np.float64) - theta)
    err[r.self_pair] = 0.0
    worst = float(err.max()) if err.size else 0.0
    _WORST[tag] = max(_WORST.get(tag, 0.0), worst)
    print('\n%s %s: worst |tp_angle - theta64| = %.3e (%.2f * 2**-23); over the %s runs so far %.3e'
          % (tag, name, worst, worst * 2.0 ** 23, tag, _WORST[tag]))
    if worst > ANGLE_TOL:
        w = int(err.argmax())
        print('row %d: operands y = %r, x = %r, theta64 = %r, kernel %r' % (w, operands[0][w], operands[1][w], theta[w], got[w]))
    assert worst <= ANGLE_TOL, (name, worst)


@gpu
@pytest.mark.parametrize('wt', WT)
@pytest.mark.parametrize('name', ALL_NAMES)
def test_count(dev, name, wt):
    """1. pamnet_triplet_count_i32."""
    from pamnet_amd import lib
    h = any_host(name)
    P, d, r = lib.ptr, on(dev, h), h.ref(wt)
    tcount, tpcount = ints(dev, h.E), ints(dev, h.E)
    lib.call('pamnet_triplet_count_i32', P(d.lptr), P(d.src), P(d.dst), h.E, wt, P(tcount), P(tpcount), lib.stream_of(d.pos))
    assert same(tcount, r.tcount) and same(tpcount, r.tpcount)


@gpu
@pytest.mark.parametrize('wt', WT)
@pytest.mark.parametrize('name', NAMES)
def test_fill_open(dev, name, wt):
    """2. pamnet_triplet_fill_f32: the three index arrays element for element, the angles."""
    h = host(name)
    r = h.ref(wt)
    tp_idx, tp_edge, tp_angle, tp_kind = _fill(dev, h, wt)
    assert same(tp_idx, r.tp_idx) and same(tp_edge, r.tp_edge) and same(tp_kind, r.tp_kind)
    _assert_angles('open', name, r, tp_angle, *h.angles(wt))


def _device_table(dev, cells32, cutoff):
    """pamnet_cell_prepare_f64 on the device, read back: (table tensor, table on the host)."""
    from pamnet_amd import lib
    cells = up(dev, np.asarray(cells32, np.float32).reshape(-1, 9))
    ng = int(cells.size(0))
    tab = torch.full((ng * R.PBC_ROW,), float('nan'), dtype=torch.float64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    lib.call('pamnet_cell_prepare_f64', lib.ptr(cells), ng, cutoff, lib.ptr(tab), lib.ptr(flag), lib.stream_of(cells))
    assert int(flag) == 0
    host_tab = tab.cpu().numpy().reshape(ng, R.PBC_ROW)
    want = _host_table(cells32)
    assert np.array_equal(host_tab[:, :9], want[:, :9]) and np.abs(host_tab[:, 9:] - want[:, 9:]).max() < 1e-13
    return tab, host_tab


@gpu
@pytest.mark.parametrize('wt', WT)
@pytest.mark.parametrize('name', PBC_NAMES)
def test_fill_periodic(dev, name, wt):
    """3. pamnet_triplet_fill_pbc_f32 with the table pamnet_cell_prepare_f64 made, which is also the reference's."""
    h = pbc_host(name)
    r = h.ref(wt)
    tab, host_tab = _device_table(dev, CELLS, PBC_CUT)
    tp_idx, tp_edge, tp_angle, tp_kind = _fill(dev, h, wt, table=tab, node_graph=on(dev, h).node_graph)
    assert same(tp_idx, r.tp_idx) and same(tp_edge, r.tp_edge) and same(tp_kind, r.tp_kind)
    vec, img, half, tie = h.bond_vectors(host_tab)
    assert half >= 1e-3 and tie >= 2.0 ** -40 and np.array_equal(img, h.bond_vectors(h.table)[1])
    _assert_angles('periodic', name, r, tp_angle, *h.angles_with(wt, host_tab))


@gpu
@pytest.mark.parametrize('wt', WT)
@pytest.mark.parametrize('name', ALL_NAMES)
def test_fill_periodic_in_a_wide_cell_is_the_open_fill(dev, name, wt):
    """3. A cell of edge 1e4: every image is 0, and the periodic kernel returns the open kernel's tp_angle bit for bit (the bond
    lists of the periodic inputs are bond lists like any other here: their atoms where they stand, in open space)."""
    h = any_host(name)
    r = h.ref(wt)
    tab, _ = _device_table(dev, np.eye(3, dtype=np.float32)[None] * np.float32(1e4), PBC_CUT)
    node_graph = torch.zeros(h.n, dtype=torch.int32, device=dev)
    opened, wide = _fill(dev, h, wt), _fill(dev, h, wt, table=tab, node_graph=node_graph)
    for k in (0, 1, 3):
        assert torch.equal(opened[k], wide[k])
    assert same(wide[0], r.tp_idx) and same(wide[1], r.tp_edge) and same(wide[3], r.tp_kind)
    assert not bool(torch.isnan(wide[2]).any()) and np.array_equal(bits(opened[2]), bits(wide[2]))


def _transpose(dev, h, wt, lt_perm, cap=None):
    from pamnet_amd import lib
    P, d, r, t = lib.ptr, on(dev, h), h.ref(wt), ref_on(dev, h, wt)
    out = ints(dev, r.tot)
    lib.call('pamnet_triplet_transpose_fill_i32', P(d.lptr), P(d.src), P(d.dst), P(d.lt_ptr), P(lt_perm), h.E, wt,
             P(t.tp_ptr), P(t.tcount), P(t.tt_ptr), P(out), r.tot if cap is None else cap,
             lib.stream_of(d.pos))
    return out


@gpu
@pytest.mark.parametrize('wt', WT)
@pytest.mark.parametrize('name', ALL_NAMES)
def test_transpose(dev, name, wt):
    """4. pamnet_triplet_transpose_count/fill_i32 against the stable counting sort of the HOST's tp_idx, with the transposed bond
    list sorted inside its rows and with every row shuffled."""
    from pamnet_amd import lib
    h = any_host(name)
    P, d, r = lib.ptr, on(dev, h), h.ref(wt)
    for lt_perm in (d.lt_perm, d.lt_shuffled):
        count = ints(dev, h.E)
        lib.call('pamnet_triplet_transpose_count_i32', P(d.lptr), P(d.src), P(d.dst), P(d.lt_ptr), P(lt_perm), h.E, wt, P(count),
                 lib.stream_of(d.pos))
        assert same(count, np.diff(r.tt_ptr))
        assert same(_transpose(dev, h, wt, lt_perm), r.tt_perm)


@gpu
@pytest.mark.parametrize('wt', WT)
@pytest.mark.parametrize('name', ['hub17', 'clique18', 'mols', 'pbc:hub17'])
def test_caps(dev, name, wt):
    """5. cap in {tot, tot - 1, tot - 17, 1} with arrays of the full size: below the cap the full run's values (transpose: clamped
    to cap - 1), at and beyond it the sentinels -- the open fill, the periodic fill (on the periodic hubs, both forms of the
    transpose on one bond list) and the transpose.  No size here lets a kernel leave its arrays."""
    h = any_host(name)
    r = h.ref(wt)
    space = {}
    if name[:4] == 'pbc:':
        space = dict(table=_device_table(dev, CELLS, PBC_CUT)[0], node_graph=on(dev, h).node_graph)
    full = [t.cpu().numpy() for t in _fill(dev, h, wt, **space)]
    assert r.tot > 17
    for cap in (r.tot, r.tot - 1, r.tot - 17, 1):
        got = [t.cpu().numpy() for t in _fill(dev, h, wt, cap=cap, **space)]
        for g, f, want in zip(got, full, (r.tp_idx, r.tp_edge, None, r.tp_kind)):
            if want is None:
                assert np.array_equal(bits(g[:cap]), bits(f[:cap])) and np.isnan(g[cap:]).all() and not np.isnan(g[:cap]).any()
            else:
                assert np.array_equal(g[:cap], want[:cap]) and (g[cap:] == I_SENT).all()
        for lt_perm in (on(dev, h).lt_perm, on(dev, h).lt_shuffled):
            got = _transpose(dev, h, wt, lt_perm, cap=cap).cpu().numpy()
            assert np.array_equal(got[:cap], np.minimum(r.tt_perm[:cap], cap - 1)) and (got[cap:] == I_SENT).all()


@gpu
@pytest.mark.parametrize('wt', WT)
def test_nothing_to_do_writes_nothing(dev, wt):
    """5. cap = 0 and n_edges = 0 return PAMNET_OK (lib.call raises otherwise) and leave every sentinel."""
    from pamnet_amd import lib
    h = host('mols')
    P, d, r = lib.ptr, on(dev, h), h.ref(wt)
    tab, _ = _device_table(dev, np.eye(3, dtype=np.float32)[None] * np.float32(1e4), PBC_CUT)
    node_graph = torch.zeros(h.n, dtype=torch.int32, device=dev)
    t = ref_on(dev, h, wt)
    tp_ptr, tcount, tt_ptr = t.tp_ptr, t.tcount, t.tt_ptr
    for E, cap in ((h.E, 0), (0, r.tot), (0, 0)):
        a, b, c, ang, cnt, cnt2 = (ints(dev, r.tot), ints(dev, r.tot), ints(dev, r.tot), nans(dev, r.tot), ints(dev, h.E),
                                   ints(dev, h.E))
        st = lib.stream_of(d.pos)
        tail = (P(d.lptr), P(d.src), P(d.dst), E, wt, P(tp_ptr), P(a), P(b), P(ang), P(c), cap, st)
        lib.call('pamnet_triplet_fill_f32', P(d.pos), *tail)
        lib.call('pamnet_triplet_fill_pbc_f32', P(d.pos), P(tab), P(node_graph), *tail)
        tt = ints(dev, r.tot)
        lib.call('pamnet_triplet_transpose_fill_i32', P(d.lptr), P(d.src), P(d.dst), P(d.lt_ptr), P(d.lt_perm), E, wt, P(tp_ptr),
                 P(tcount), P(tt_ptr), P(tt), cap, st)
        rows = ints(dev, r.tot)
        lib.call('pamnet_expand_rows_i32', P(tp_ptr), E, P(rows), cap, st)
        if E == 0:
            lib.call('pamnet_triplet_count_i32', P(d.lptr), P(d.src), P(d.dst), 0, wt, P(cnt), P(cnt2), st)
            lib.call('pamnet_triplet_transpose_count_i32', P(d.lptr), P(d.src), P(d.dst), P(d.lt_ptr), P(d.lt_perm), 0, wt,
                     P(cnt), st)
            te, tn = ints(dev, r.tot), ints(dev, r.tot)
            lib.call('pamnet_triplet_transpose_aux_i32', P(tt), P(b), P(d.dst), 0, P(te), P(tn), st)
            assert bool((te == I_SENT).all()) and bool((tn == I_SENT).all())
        torch.cuda.synchronize()
        for out in (a, b, c, tt, rows, cnt, cnt2):
            assert bool((out == I_SENT).all()), (E, cap)
        assert bool(torch.isnan(ang).all())


@gpu
@pytest.mark.parametrize('wt', WT)
@pytest.mark.parametrize('name', ALL_NAMES)
def test_transpose_aux(dev, name, wt):
    """6. pamnet_triplet_transpose_aux_i32: te = t_row[perm], tn = l_row[te]."""
    from pamnet_amd import lib
    h = any_host(name)
    P, d, r, t = lib.ptr, on(dev, h), h.ref(wt), ref_on(dev, h, wt)
    te, tn = ints(dev, r.tot), ints(dev, r.tot)
    lib.call('pamnet_triplet_transpose_aux_i32', P(t.tt_perm), P(t.tp_edge), P(d.dst), r.tot, P(te), P(tn),
             lib.stream_of(d.pos))
    want = r.tp_edge[r.tt_perm]
    assert same(te, want) and same(tn, h.dst[want])


@gpu
@pytest.mark.parametrize('name', ['hub17', 'clique18', 'mols', 'holes', 'blocks'])
def test_expand_rows_below_the_total(dev, name):
    """7. pamnet_expand_rows_i32 with cap below the total: host values below it, sentinels from it on -- over the rows of the
    triplet / pair pointer and over the bond pointer (with its empty rows)."""
    from pamnet_amd import lib
    h = host(name)
    r = h.ref(1)
    for ptr, want in ((r.tp_ptr, r.tp_edge), (h.lptr, h.dst)):
        tot = int(ptr[-1])
        p = up(dev, ptr)
        for cap in (tot, tot - 1, tot - 17, 1):
            out = ints(dev, tot)
            lib.call('pamnet_expand_rows_i32', lib.ptr(p), len(ptr) - 1, lib.ptr(out), cap, lib.stream_of(p))
            got = out.cpu().numpy()
            assert np.array_equal(got[:cap], want[:cap]) and (got[cap:] == I_SENT).all(), (name, cap)


# ---- GPU test: the public route ----------------------------------------------------------------------------------------------
LOCAL_CUT = 1.7


def _route_inputs(route):
    """(positions, bonds as listed or None, cells or None, the bonds the route must report) of `mols` for the three routes."""
    n, pairs, pos, first = _listing('mols')
    gptr = np.asarray(first, np.int32)
    if route == 'bonds':
        return pos, pairs, None, sorted(pairs), gptr
    if route == 'bond_free':
        want, margin = _radius_pairs(pos, gptr, LOCAL_CUT)
        assert margin > 1e-5
        return pos, None, None, sorted(want), gptr
    cells = CELLS[np.arange(12) % 3]                                  # every molecule in a cell of its own, wrapped into it
    mol = np.repeat(np.arange(12), np.diff(gptr))
    c64 = cells.astype(np.float64)[mol]
    frac = np.einsum('ac,ack->ak', pos.astype(np.float64), np.linalg.inv(c64))
    wrapped = np.einsum('ak,akc->ac', frac - np.floor(frac), c64).astype(np.float32)
    want, margin = _radius_pairs(wrapped, gptr, LOCAL_CUT, cells.astype(np.float64))
    assert margin > 1e-5
    return wrapped, None, cells, sorted(want), gptr


def test_route_inputs_have_bonds_and_images():
    for route in ('bonds', 'bond_free', 'cell'):
        pos, pairs, cells, want, gptr = _route_inputs(route)
        assert len(want) > 60 and len(set(want)) == len(want)
    mol = np.repeat(np.arange(12), np.diff(gptr))
    src, dst = np.array(want).T
    table = _host_table(cells)
    vec, img, half, tie = R.bond_vectors_pbc(pos, table, mol.astype(np.int32), src, dst)
    assert (img != 0).any(1).sum() > 10                              # molecules split by the faces of their cells
    assert half >= 1e-3
    for e in range(len(src)):                                        # the kernel's fp64 statements round to the exact value's fp32
        n, d = R.min_image_chain(pos[src[e]], pos[dst[e]], table[mol[src[e]]])
        assert [int(v) for v in n] == img[e].tolist()
        assert np.array_equal(np.array(d).astype(np.float32).view(np.uint32), vec[e].view(np.uint32))


@gpu
@pytest.mark.parametrize('wt', WT)
@pytest.mark.parametrize('route', ['bonds', 'bond_free', 'cell'])
def test_build_graph_returns_the_host_lists(dev, route, wt):
    """8. G.build_graph(mol_local=False) on `mols` -- with its bonds, bond-free at cutoff_l = 1.7, bond-free in cells: the local
    bonds it reports are the expected set, and for THOSE bonds g.tp.*, g.tp_kind, g.tp_T.*, g.n_trip, g.n_pair are exactly the
    host lists and g.tp_angle the host angles."""
    from pamnet_amd import graph as G
    pos, pairs, cells, want, gptr = _route_inputs(route)
    n = int(gptr[-1])
    batch = torch.from_numpy(np.repeat(np.arange(12), np.diff(gptr))).to(dev)
    x = (torch.arange(n, device=dev) % 5).float()
    ei = None if pairs is None else torch.tensor(pairs, dtype=torch.long).t().contiguous().to(dev)
    g = G.build_graph('QM9', LOCAL_CUT, PBC_CUT, 'source_to_target', x, batch, up(dev, pos), ei, num_graphs=12, n_types=5,
                      with_triplets=bool(wt), mol_local=False, need_grad=True,
                      cell=None if cells is None else up(dev, cells))
    assert isinstance(g, G.Graph) and not isinstance(g, G.EngineGraph)
    lptr, src, dst = (t.cpu().numpy() for t in (g.loc.ptr, g.loc.col, g.loc.row_of))
    assert sorted(zip(src.tolist(), dst.tolist())) == want
    h = Host(n, lptr, src, dst, pos, 99)
    r = h.ref(wt)
    assert g.tp.m == r.tot and g.n_trip == int(r.tcount.sum()) and g.n_pair == int((r.tp_kind == 1).sum())
    assert same(g.tp.ptr, r.tp_ptr) and same(g.tp.col, r.tp_idx) and same(g.tp.row_of, r.tp_edge) and same(g.tp_kind, r.tp_kind)
    assert same(g.tp_T.ptr, r.tt_ptr) and same(g.tp_T.perm, r.tt_perm)
    if cells is None:
        operands, theta = h.angles(wt)
    else:
        tab = g.cell_tab.cpu().numpy().reshape(12, R.PBC_ROW)
        assert np.array_equal(tab[:, :9], _host_table(cells)[:, :9])
        operands, theta = R.angles_pbc(pos, tab, batch.cpu().numpy(), src, dst, r.tp_idx, r.tp_edge, r.tp_kind)
    _assert_angles('route', route, r, g.tp_angle, operands, theta)
