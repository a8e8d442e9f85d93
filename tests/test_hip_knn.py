"""The k-nearest-neighbour search of the RNA path (csrc/graph.hip: knn_select, knn_topk, knn_stream, knn_kernel) and the
kernels behind it (the cut counts, the pair scan, the cut fill, the triplet + pair total) against the host references of
tests/knn_ref.py.  Every comparison is exact (bit patterns of the distances included) and every expected value is computed
on the host; the inputs are chosen so that each exit of the selection is taken, which the host tests confirm with a model of
the selection's control flow (`test_inputs_reach_every_exit`), at every K that sits at a limit of the wavefront code.

Host tests (no GPU): the references against brute force and the oracle, and the guard.  GPU tests: marked `gpu`."""
import functools
import zlib

import numpy as np
import pytest
import torch

import knn_ref as R

gpu = pytest.mark.gpu

SQRT2 = float(np.sqrt(np.float32(2.0)))                   # the fp32 distance of two lattice points one diagonal apart


def below(v):
    return float(np.nextafter(np.float32(v), np.float32(0)))


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def _random_graph(rng, m):
    """Uniform points at an RNA-like density (0.05 atoms per cubic Angstrom), coordinates with three decimals as the
    dataset's files carry them."""
    side = (m / 0.05) ** (1.0 / 3.0)
    return np.round(rng.random((m, 3)) * side, 3).astype(np.float32)


def _lattice(rng, m, hi):
    return rng.integers(0, hi, size=(m, 3)).astype(np.float32)


def _coincident(rng, same, others, box=9.0):
    p = np.concatenate([np.tile(np.array([[4.5, 3.25, 5.0]], np.float32), (same, 1)),
                        (rng.random((others, 3)) * box).astype(np.float32)])
    return p[rng.permutation(same + others)]


def _full_lanes(rng):
    """4096 nodes, the full cache: lane l of a wave caches the candidates with index % 64 == l.  Lanes 0 .. 59 hold points of
    one small box, lanes 60 .. 63 points of a box 1000 units away: at a probe between the two scales a lane's count is 64 or
    0, so the count's top bit plane decides alone -- and a far query has exactly KNN_SURV = 256 candidates below the probe."""
    p = (rng.random((4096, 3)) * 3).astype(np.float32)
    p[(np.arange(4096) % 64) >= 60] += np.float32(1000.0)
    return p


SIZES = (1, 2, 3, 49, 50, 51, 63, 64, 65, 511, 512, 513, 1000, 4095, 4096)
# case -> (the K values it runs with, the graphs)
CASES = {
    'sizes': ((1, 2, 17, 50, 63, 64), lambda rng: [_random_graph(rng, m) for m in SIZES]),
    'stream_random': ((1, 50, 64), lambda rng: [_random_graph(rng, m) for m in (4097, 30, 4100)]),
    'stream_lattice': ((1, 50, 64), lambda rng: [_lattice(rng, m, 7) for m in (4097, 30, 4100)]),
    'ties': ((1, 17, 50, 64), lambda rng: [_lattice(rng, 3000, 2),             # 375 points per site
                                            _lattice(rng, 1500, 4),             # ~23 per site
                                            _lattice(rng, 4096, 4),             # ~64 per site, the full cache
                                            _coincident(rng, 80, 220),
                                            np.tile(np.array([[1.5, -2.25, 3.0]], np.float32), (300, 1)),   # interval [0, 0]
                                            _coincident(rng, 64, 64)]),         # zeros == 64: sorted from zero at K = 50, 64
    'full_lanes': ((50, 64), lambda rng: [_full_lanes(rng), _coincident(rng, 4000, 96)]),   # counts of 64 in a lane: both stages
    'coincident': ((17, 50, 64), lambda rng: [_coincident(rng, 80, 220)]),
}
TIES_GRAPHS = ('lattice2_3000', 'lattice4_1500', 'lattice4_4096', 'coincident80_220', 'identical300', 'coincident64_64')


class Case(object):
    """One batch on the host: positions, graph pointer, the reference ordering (built once, sliced per K, never written)."""

    def __init__(self, name):
        self.name, (self.Ks, make) = name, CASES[name]
        graphs = make(np.random.default_rng([20240611, zlib.crc32(name.encode())]))     # (a seed of its own per case)
        self.pos = np.ascontiguousarray(np.concatenate(graphs))
        self.gptr = np.concatenate([[0], np.cumsum([len(g) for g in graphs])]).astype(np.int32)
        self.n = int(self.gptr[-1])
        self._order = None
        self._tables = {}

    @property
    def order(self):
        if self._order is None:
            self._order = R.ordering(self.pos, self.gptr)
            for a in self._order:
                a.setflags(write=False)
        return self._order

    def table(self, K, cutoff=np.inf):
        key = (K, float(cutoff))
        if key not in self._tables:
            t = R.table(self.pos, self.gptr, K, cutoff, order=self.order)
            for a in t:
                a.setflags(write=False)
            self._tables[key] = t
        return self._tables[key]

    def on(self, dev):
        node_graph = np.repeat(np.arange(len(self.gptr) - 1, dtype=np.int32), np.diff(self.gptr))
        return (torch.from_numpy(self.pos).to(dev), torch.from_numpy(node_graph).to(dev), torch.from_numpy(self.gptr).to(dev))


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def bits(x):
    """Bit patterns of an fp32 array or tensor, on the host."""
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def same_ints(got, want):
    return np.array_equal(got.detach().cpu().numpy().reshape(-1), np.asarray(want).reshape(-1))


def same_bits(got, want):
    return np.array_equal(bits(got).reshape(-1), bits(want).reshape(-1))


# ---- host tests: the references themselves ---------------------------------------------------------------------------------
def test_table_equals_brute_force_ranking():
    """A tiny tie-free batch (two graphs, one smaller than K) ranked candidate by candidate in plain Python."""
    rng = np.random.default_rng(1)
    pos = (rng.random((11, 3)) * 4).astype(np.float32)
    gptr = np.array([0, 7, 11], np.int32)
    K, cutoff = 5, 2.0
    nbr, dist = R.table(pos, gptr, K, cutoff)
    f = np.float32
    for g in range(2):
        beg, end = int(gptr[g]), int(gptr[g + 1])
        for i in range(beg, end):
            d2 = []
            for j in range(beg, end):
                dx, dy, dz = (f(pos[i, c] - pos[j, c]) for c in range(3))
                d2.append((f(f(f(dx * dx) + f(dy * dy)) + f(dz * dz)), j))
            assert len({d for d, _ in d2}) == len(d2)                  # tie-free, as stated
            d2.sort()
            for s in range(K):
                if s < len(d2):
                    d = np.sqrt(d2[s][0])
                    keep = d2[s][1] != i and d <= f(cutoff)
                    assert nbr[i, s] == (d2[s][1] if keep else -1) and dist[i, s] == d
                else:
                    assert nbr[i, s] == -1 and dist[i, s] == np.inf
    assert (nbr[:, 0] == -1).all() and (dist[:, 0] == 0).all()          # the self entry keeps its slot
    assert ((nbr == -1) & (dist > f(cutoff)) & np.isfinite(dist)).any()  # the cutoff masks something here


def test_table_edge_set_equals_oracle():
    from oracle import pamnet_oracle as O
    rng = np.random.default_rng(2)
    sizes = (70, 30, 120)
    pos = np.concatenate([_random_graph(rng, m) for m in sizes])
    gptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    batch = torch.from_numpy(np.repeat(np.arange(3), sizes))
    K = 50
    idx, d2 = R.ordering(pos, gptr)
    for row in d2[:, :K]:                                               # tie-free inside every row: topk's order is then fixed
        fin = row[np.isfinite(row)]
        assert len(np.unique(fin)) == len(fin)
    nbr, _ = R.table(pos, gptr, K)
    ei, _ = O.get_edge_info(O.knn_graph(torch.from_numpy(pos), batch, K), torch.from_numpy(pos))
    q = np.broadcast_to(np.arange(len(pos))[:, None], nbr.shape)
    got = set(zip(q[nbr >= 0].tolist(), nbr[nbr >= 0].tolist()))
    assert got == set(zip(ei[0].tolist(), ei[1].tolist())) and len(got) == int(ei.size(1))


@pytest.mark.parametrize('with_triplets', [True, False])
def test_tp_total_equals_oracle_indices(with_triplets):
    """tp_total == idx_kj.numel() + idx_jj_pair.numel() (pairs only: the latter) of PAMNet.indices on the same edges."""
    from oracle import pamnet_oracle as O
    rng = np.random.default_rng(3)
    pos = np.concatenate([_random_graph(rng, 60), _lattice(rng, 40, 3)])
    gptr = np.array([0, 60, 100], np.int32)
    K = 7
    nbr, dist = R.table(pos, gptr, K)
    for cut in (1.0, 2.5, 50.0):
        lists = R.cut_lists(nbr, dist, K, cut)
        _, i, _, j = lists
        ei = torch.from_numpy(np.stack([j, i]).astype(np.int64))        # (j, i) = edge_index: query -> neighbour
        out = O.indices(ei, 100)
        want = int(out[8].numel()) + (int(out[3].numel()) if with_triplets else 0)
        assert R.tp_total(100, lists, with_triplets) == want and (want > 0 or cut < 1.5)


def test_cut_lists_keeps_the_cut_itself():
    nbr = np.array([[-1, 3, 2], [0, -1, 1]], np.int32)
    dist = np.array([[0.0, 1.0, SQRT2], [1.0, 0.0, 2.0]], np.float32)
    ptr, n, d, q = R.cut_lists(nbr, dist, 3, SQRT2)
    assert ptr.tolist() == [0, 2, 3] and n.tolist() == [3, 2, 0] and q.tolist() == [0, 0, 1]
    ptr, n, d, q = R.cut_lists(nbr, dist, 3, below(SQRT2))
    assert ptr.tolist() == [0, 1, 2] and n.tolist() == [3, 0]


# ---- host test: the guard ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _branch_counts(name):
    c = case(name)
    per_graph = []
    for g in range(len(c.gptr) - 1):
        per_graph.append(R.branch_counts(c.pos, c.gptr[g:g + 2], c.Ks))
    return per_graph


def test_constants_of_the_selection():
    """The inputs below are sized for these values; a change of either has to be followed here."""
    assert R.constants() == {'KNN_CACHE': 64, 'KNN_SURV': 256}


def test_inputs_reach_every_exit():
    """The host model of knn_select's control flow, over every query of every case: each case reaches the exits it is named
    for, every exit is reached by at least 32 queries at K = 50 and at K = 64, and the first-stage tie fallback also by a
    graph that fills the register cache (4096 nodes)."""
    reached = {50: dict.fromkeys(R.BRANCHES, 0), 64: dict.fromkeys(R.BRANCHES, 0)}
    print()
    print('%-15s %-17s %3s  %s' % ('case', 'graph', 'K', '  '.join('%14s' % b for b in R.BRANCHES)))
    got = {}
    for name in sorted(CASES):
        c = case(name)
        names = TIES_GRAPHS if name == 'ties' else ['n=%d' % m for m in np.diff(c.gptr)]
        for g, per_k in enumerate(_branch_counts(name)):
            for K in c.Ks:
                cnt = per_k[K]
                got[name, g, K] = cnt
                if not (name == 'sizes' and int(np.diff(c.gptr)[g]) < 511 and g not in (0, 7)):     # (print the telling rows)
                    print('%-15s %-17s %3d  %s' % (name, names[g], K, '  '.join('%14d' % cnt[b] for b in R.BRANCHES)))
                if K in reached:
                    for b in R.BRANCHES:
                        reached[K][b] += cnt[b]

    def only(cnt, *allowed):
        return all(v == 0 for b, v in cnt.items() if b not in allowed)
    for K in case('ties').Ks:
        m = {g: got['ties', g, K] for g in range(len(TIES_GRAPHS))}
        assert m[0]['ties_cache'] == 3000 and m[4]['ties_cache'] == 300           # every query
        if K >= 50:
            assert m[1]['ties_survivors'] == 1500
            assert m[5]['sort_from_zero'] == 64
        else:
            assert m[1]['sort_from_zero'] >= 1000                                 # ~23 points per site: zeros >= K mostly
        if K == 64:
            assert m[2]['ties_cache'] >= 32 and m[2]['ties_survivors'] >= 32      # the full cache takes the first fallback
        if K >= 17:
            assert m[3]['ties_survivors'] >= 32 and m[3]['sort'] >= 32 and only(m[3], 'ties_survivors', 'sort')
        else:
            assert m[3]['sort_from_zero'] >= 32 and m[3]['ties_survivors'] >= 32
            assert only(m[3], 'sort_from_zero', 'ties_survivors')
    for K in case('coincident').Ks:
        cnt = got['coincident', 0, K]
        assert cnt['ties_survivors'] >= 32 and cnt['sort'] >= 32 and only(cnt, 'ties_survivors', 'sort')
    for K in case('full_lanes').Ks:
        assert got['full_lanes', 0, K]['sort'] == 4096
        assert got['full_lanes', 1, K]['ties_cache'] >= 4000                      # knn_topk over 64 full slots
    c = case('sizes')
    for g, m in enumerate(np.diff(c.gptr)):
        for K in c.Ks:
            want = 'sort_from_zero' if (K == 1 or m == 1) else 'sort'             # (a one-node graph: its zero reaches kk = 1)
            assert got['sizes', g, K][want] == m, (m, K, got['sizes', g, K])
    for name in ('stream_random', 'stream_lattice'):
        for K in case(name).Ks:
            assert got[name, 0, K]['stream'] == 4097 and got[name, 2, K]['stream'] == 4100
            assert got[name, 1, K]['stream'] == 0 and sum(got[name, 1, K].values()) == 30
    for K in (50, 64):
        for b in R.BRANCHES:
            assert reached[K][b] >= 32, (K, b, reached[K])
    # the scalar form of the model agrees with the batched one
    c = case('ties')
    for i in (0, 2999, 3000, 4499, 4500, 8595, 8596, 8896, 9195):
        g = int(np.searchsorted(c.gptr, i, side='right')) - 1
        for K in (1, 64):
            b = R.branches(c.pos, int(c.gptr[g]), int(c.gptr[g + 1]), (K,))[K][i - int(c.gptr[g])]
            assert R.branch(c.pos, int(c.gptr[g]), int(c.gptr[g + 1]), i, K) == R.BRANCHES[int(b)]


# ---- GPU tests: the search -------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs an MI355X'
    from pamnet_amd import lib
    lib.load()                                    # fail loudly if the HIP library is missing
    return torch.device('cuda:0')


def _search_twice(dev, c, K, cutoff=float('inf')):
    from pamnet_amd import graph as G
    pos, node_graph, gptr = c.on(dev)
    kp, kn, kd = G.knn_table(pos, node_graph, gptr, K, cutoff)
    _, kn2, kd2 = G.knn_table(pos, node_graph, gptr, K, cutoff)
    assert torch.equal(kn, kn2) and torch.equal(kd.view(torch.int32), kd2.view(torch.int32))       # run to run, bitwise
    assert same_ints(kp, np.arange(c.n + 1, dtype=np.int64) * K)
    return kn, kd


def _assert_table(c, K, kn, kd, cutoff=np.inf):
    want_n, want_d = c.table(K, cutoff)
    got_n, got_d = kn.cpu().numpy().reshape(c.n, K), bits(kd).reshape(c.n, K)
    bad = np.flatnonzero((got_n != want_n).any(1) | (got_d != bits(want_d)).any(1))
    assert bad.size == 0, '%s K=%d: %d rows differ, first %d (graph %d): nbr %s want %s' % (
        c.name, K, bad.size, bad[0], int(np.searchsorted(c.gptr, bad[0], side='right')) - 1, got_n[bad[0]], want_n[bad[0]])


@gpu
@pytest.mark.parametrize('K', CASES['sizes'][0])
def test_knn_every_cache_fill(dev, K):
    """Graphs of 1 .. 4096 nodes in one launch: below, at and above K, one cache slot, one slot group, all eight groups, the
    full cache; graph boundaries inside workgroups; the padding of graphs smaller than K."""
    c = case('sizes')
    kn, kd = _search_twice(dev, c, K)
    _assert_table(c, K, kn, kd)


@gpu
def test_knn_cutoff_masks_half(dev):
    c = case('sizes')
    K = 50
    _, d = c.table(K)
    cutoff = float(np.median(d[np.isfinite(d)]))                    # a distance of the table: entries AT the cutoff are kept
    want_n, _ = c.table(K, cutoff)
    n_inf, _ = c.table(K)
    assert 0.3 < (want_n >= 0).sum() / float((n_inf >= 0).sum()) < 0.7
    kn, kd = _search_twice(dev, c, K, cutoff)
    _assert_table(c, K, kn, kd, cutoff)


@gpu
@pytest.mark.parametrize('K', CASES['stream_random'][0])
@pytest.mark.parametrize('name', ['stream_random', 'stream_lattice'])
def test_knn_streaming_beside_selection(dev, name, K):
    """4097 and 4100 nodes stream; the 30-node graph between them puts selecting and streaming waves in one workgroup.  The
    lattice gives the insertion exact ties."""
    c = case(name)
    kn, kd = _search_twice(dev, c, K)
    _assert_table(c, K, kn, kd)


@gpu
@pytest.mark.parametrize('K', CASES['ties'][0])
def test_knn_tie_exits(dev, K):
    """Both tie fallbacks, the interval that starts at zero and the interval [0, 0], several graphs in one launch."""
    c = case('ties')
    kn, kd = _search_twice(dev, c, K)
    _assert_table(c, K, kn, kd)


@gpu
@pytest.mark.parametrize('K', CASES['full_lanes'][0])
def test_knn_lane_counts_of_64(dev, K):
    """A full cache whose lanes count 64 candidates at a probe (the seventh bit plane of the wave's count), in the first-stage
    bisection and in the tie fallback over the whole cache; a query with exactly KNN_SURV survivors."""
    c = case('full_lanes')
    kn, kd = _search_twice(dev, c, K)
    _assert_table(c, K, kn, kd)


# ---- GPU tests: the kernels behind the search -------------------------------------------------------------------------------
def _cuts_of(name, c, K):
    """(pairs of cuts, [(pair, side) AT a distance of the table, (pair, side) one ulp below it])."""
    if name == 'sizes':                                             # random points: one pair of plain cuts, one pair AT distances
        d = c.table(K)[1]
        d = np.sort(d[np.isfinite(d) & (d > 0)])
        a, b = float(d[len(d) // 2]), float(d[len(d) // 8])
        return [(5.0, 2.6), (a, b), (below(a), below(b))], [((1, 0), (2, 0)), ((1, 1), (2, 1))]
    return ([(2.0, 1.0), (SQRT2, below(1.0)), (below(2.0), below(SQRT2))],
            [((0, 0), (2, 0)), ((1, 0), (2, 1)), ((0, 1), (1, 1))])


@gpu
@pytest.mark.parametrize('name,K', [('ties', 50), ('ties', 64), ('sizes', 50), ('sizes', 17)])
def test_cuts_and_fill_equal_host_lists(dev, name, K):
    """pamnet_knn_cut_i32 (table + per-query counts), pamnet_exclusive_scan_pair_i32, pamnet_knn_cut_fill_i32 at exact, too
    small and too large capacities, G.knn_cuts, G.csr_filter and G.csr_filter2: all equal to cut_lists of the host table.  A cut
    that equals a distance keeps it, one ulp below drops it."""
    from pamnet_amd import graph as G, lib
    c = case(name)
    n = c.n
    pos, node_graph, gptr = c.on(dev)
    want_n, want_d = c.table(K)
    st, P = lib.stream_of(pos), lib.ptr
    i32 = lambda m: torch.empty(m, dtype=torch.int32, device=dev)
    kept = []
    cuts, at_and_below = _cuts_of(name, c, K)
    for cut_a, cut_b in cuts:
        wa, wb = R.cut_lists(want_n, want_d, K, cut_a), R.cut_lists(want_n, want_d, K, cut_b)
        kept.append((int(wa[0][-1]), int(wb[0][-1])))
        kn, kd = i32(n * K), torch.empty(n * K, device=dev)
        ca, cb, ra, rb, tmp = i32(n), i32(n), i32(n + 1), i32(n + 1), i32(n // 4096 + 2)
        lib.call('pamnet_knn_cut_i32', P(pos), P(node_graph), P(gptr), n, K, cut_a, cut_b, P(kn), P(kd), P(ca), P(cb), st)
        assert same_ints(kn, want_n) and same_bits(kd, want_d)
        assert same_ints(ca, np.diff(wa[0])) and same_ints(cb, np.diff(wb[0]))
        lib.call('pamnet_exclusive_scan_pair_i32', P(ca), P(ra), P(cb), P(rb), n, P(tmp), st)
        assert same_ints(ra, wa[0]) and same_ints(rb, wb[0])
        ea, eb = int(wa[0][-1]), int(wb[0][-1])
        for cap_a, cap_b in ((ea, eb), (max(ea - 5, 1), eb + 7), (ea + 7, max(eb - 5, 1))):
            outs = [(i32(cap).fill_(-7), torch.full((cap,), -7.0, device=dev), i32(cap).fill_(-7), i32(n + 1))
                    for cap in (cap_a, cap_b)]
            lib.call('pamnet_knn_cut_fill_i32', P(kn), P(kd), n, K, cut_a, P(ra), cap_a, P(outs[0][0]), P(outs[0][1]),
                     P(outs[0][2]), P(outs[0][3]), cut_b, P(rb), cap_b, P(outs[1][0]), P(outs[1][1]), P(outs[1][2]),
                     P(outs[1][3]), st)
            for (nbr, dist, row, ptr), w, cap in zip(outs, (wa, wb), (cap_a, cap_b)):
                m = min(cap, int(w[0][-1]))
                assert same_ints(ptr, np.minimum(w[0], cap))
                assert same_ints(nbr[:m], w[1][:m]) and same_bits(dist[:m], w[2][:m]) and same_ints(row[:m], w[3][:m])
                # nothing is written beyond what the list holds
                assert bool((nbr[m:] == -7).all()) and bool((dist[m:] == -7.0).all()) and bool((row[m:] == -7).all())
        res = G.knn_cuts(pos, node_graph, gptr, K, cut_a, cut_b)
        kp = torch.arange(n + 1, device=dev, dtype=torch.int32) * K
        pair = G.csr_filter2(kp, kn, kd, cut_a, cut_b)
        for w, got, one, two in zip((wa, wb), res, (G.csr_filter(kp, kn, kd, cut_a), G.csr_filter(kp, kn, kd, cut_b)), pair):
            assert same_ints(got[0], w[0]) and same_ints(got[1], w[1]) and same_bits(got[2], w[2]) and same_ints(got[3], w[3])
            for f in (one, two):
                assert same_ints(f[0], w[0]) and same_ints(f[1], w[1]) and same_bits(f[2], w[2])
    at = []
    for (pa, sa), (pb, sb) in at_and_below:                         # the cut AT a distance keeps exactly the entries at it more
        at.append(int(((want_n >= 0) & (want_d == np.float32(cuts[pa][sa]))).sum()))
        assert kept[pa][sa] - kept[pb][sb] == at[-1]
    assert max(at) > 0                                              # ... and the table has such entries


@gpu
@pytest.mark.parametrize('with_triplets', [True, False])
@pytest.mark.parametrize('K', [17, 50, 64])
@pytest.mark.parametrize('name', ['ties', 'coincident', 'sizes'])
def test_tp_total_equals_host_count(dev, name, K, with_triplets):
    """pamnet_knn_tp_total_i64 on the host table == tp_total of the host lists == the row total pamnet_triplet_count_i32 gives on
    the transposed local graph."""
    from pamnet_amd import graph as G, lib
    c = case(name)
    n = c.n
    want_n, want_d = c.table(K)
    kn, kd = (torch.from_numpy(np.array(a)).to(dev).reshape(-1) for a in (want_n, want_d))      # (copies: the cached table is read-only)
    for cut in (2.6, 5.0) if name == 'sizes' else (1.0, SQRT2, below(SQRT2), 2.0):
        lists = R.cut_lists(want_n, want_d, K, cut)
        want = R.tp_total(n, lists, with_triplets)
        buf = torch.zeros((n + 1) // 2 + 1, dtype=torch.int64, device=dev)         # [n] int32 in-degrees, then the int64 total
        lib.call('pamnet_knn_tp_total_i64', lib.ptr(kn), lib.ptr(kd), n, K, cut, 1 if with_triplets else 0, lib.ptr(buf),
                 lib.ptr(buf[-1:]), lib.stream_of(kn))
        assert int(buf[-1]) == want, (name, K, cut, int(buf[-1]), want)
        assert same_ints(buf[:-1].view(torch.int32)[:n], np.bincount(lists[1], minlength=n))
        if cut in (2.6, SQRT2):                                      # (one cut per case: the graph route is the slow part)
            qp, qn, qd, qq = (torch.from_numpy(a).to(dev) for a in lists)
            lp, l_src, l_dist, _ = G._transpose_edges(qp, qn, qd, n, q=qq)
            l_dst = G.expand_rows(lp, int(l_src.numel()))
            tp_ptr, _ = G._triplet_ptr(lp, l_src, l_dst, with_triplets)
            assert int(tp_ptr[-1]) == want


# ---- GPU tests: the whole builder ------------------------------------------------------------------------------------------
def _edge_key(q, nbr, dist, n):
    """Edges as (query * n + neighbour, distance bits), sorted by the key (a kNN list holds a pair once)."""
    key = np.asarray(q, np.int64) * n + np.asarray(nbr, np.int64)
    o = np.argsort(key, kind='stable')
    return key[o], bits(dist)[o]


@gpu
@pytest.mark.parametrize('flow', ['source_to_target', 'target_to_source'])
@pytest.mark.parametrize('K,route', [(50, 'cuts'), (50, 'sizes_steps'), (50, 'engine'), (64, 'cuts'), (64, 'engine')])
def test_build_graph_on_ties(dev, K, route, flow):
    """build_graph with the RNA schema on the ties batch: the global and the local edge sets with their distances equal the host
    lists and g.tp.m the host total -- by the one-search route (no sizes), by the step-by-step route with the host's sizes, and
    through the graph engine.  (build_graph takes host sizes at the models' k = 50 only: at k = 64 the engine is entered by
    its own function, and the step-by-step route with sizes does not exist.)"""
    from pamnet_amd import graph as G
    c = case('ties')
    n, ng = c.n, len(c.gptr) - 1
    cutoff_g, cutoff_l = 2.0, SQRT2
    want_n, want_d = c.table(K)
    wg, wl = R.cut_lists(want_n, want_d, K, cutoff_g), R.cut_lists(want_n, want_d, K, cutoff_l)
    with_triplets = flow == 'source_to_target'                       # (the other flow: pairs only, PAMNet_s' rows)
    tp = R.tp_total(n, wl, with_triplets)
    sizes = (int(wg[0][-1]), int(wl[0][-1]), tp)
    pos, node_graph, _ = c.on(dev)
    x = torch.cat([pos, (torch.arange(n, device=dev) % 3).float()[:, None]], 1).contiguous()
    batch = node_graph.long()
    kw = dict(num_graphs=ng, need_grad=False, knn_k=K, with_triplets=with_triplets, n_types=3, default_basis=False)
    saved = G.ENGINE
    try:
        G.ENGINE = route == 'engine'
        if route == 'cuts':
            g = G.build_graph('rna_x', cutoff_l, cutoff_g, flow, x, batch, **kw)
        elif K == G.KNN_K:
            g = G.build_graph('rna_x', cutoff_l, cutoff_g, flow, x, batch, sizes=sizes, **kw)
        else:
            g = G._engine_graph('rna_x', cutoff_l, cutoff_g, flow, x, batch, None, None, ng, False, K, with_triplets, 3, sizes,
                                default_basis=False)
    finally:
        G.ENGINE = saved
    assert isinstance(g, G.EngineGraph) == (route == 'engine')
    if g.check is not None:                                          # the device's own counts equal the host sizes
        torch.cuda.synchronize()
        G.raise_for_flag(G.read_flags([g.check]))
    assert (g.glob.m, g.loc.m, g.tp.m) == sizes
    row, col = g.glob.row_of.cpu().numpy(), g.glob.col.cpu().numpy()
    q, nb = (row, col) if flow == 'target_to_source' else (col, row)       # rows = where the global layer aggregates
    got, want = _edge_key(q, nb, g.dist_g, n), _edge_key(wg[3], wg[1], wg[2], n)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    got = _edge_key(g.loc.col.cpu().numpy(), g.loc.row_of.cpu().numpy(), g.dist_l, n)    # local: rows = neighbour i, col = query j
    want = _edge_key(wl[3], wl[1], wl[2], n)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert int(g.tp.ptr[-1]) == tp


# ---- GPU test: the bounds of k -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('k', [0, 65])
def test_k_out_of_range_is_refused_before_any_launch(dev, k):
    from pamnet_amd import lib
    n = 8
    pos = torch.rand(n, 3, device=dev)
    node_graph = torch.zeros(n, dtype=torch.int32, device=dev)
    gptr = torch.tensor([0, n], dtype=torch.int32, device=dev)
    mk = lambda m: torch.full((m,), -7, dtype=torch.int32, device=dev)
    nbr, dist, ca, cb = mk(n * 65), torch.full((n * 65,), -7.0, device=dev), mk(n), mk(n)
    raw, ptr_a, ptr_b = torch.zeros(n + 1, dtype=torch.int32, device=dev), mk(n + 1), mk(n + 1)
    tot = torch.full((n,), -7, dtype=torch.int64, device=dev)
    st, P = lib.stream_of(pos), lib.ptr
    with pytest.raises(RuntimeError, match='pamnet_knn_i32 failed: PAMNET_EINVAL'):
        lib.call('pamnet_knn_i32', P(pos), P(node_graph), P(gptr), n, k, 10.0, P(nbr), P(dist), st)
    with pytest.raises(RuntimeError, match='pamnet_knn_cut_i32 failed: PAMNET_EINVAL'):
        lib.call('pamnet_knn_cut_i32', P(pos), P(node_graph), P(gptr), n, k, 10.0, 1.0, P(nbr), P(dist), P(ca), P(cb), st)
    with pytest.raises(RuntimeError, match='pamnet_knn_tp_total_i64 failed: PAMNET_EINVAL'):
        lib.call('pamnet_knn_tp_total_i64', P(nbr), P(dist), n, k, 10.0, 1, P(ca), P(tot), st)
    with pytest.raises(RuntimeError, match='pamnet_knn_cut_fill_i32 failed: PAMNET_EINVAL'):
        lib.call('pamnet_knn_cut_fill_i32', P(nbr), P(dist), n, k, 10.0, P(raw), n, P(ca), P(dist), P(cb), P(ptr_a), 1.0, P(raw),
                 n, P(ca), P(dist), P(cb), P(ptr_b), st)
    torch.cuda.synchronize()
    for t in (nbr, ca, cb, ptr_a, ptr_b, tot):                       # nothing was launched: nothing was written
        assert bool((t == -7).all())
    assert bool((dist == -7.0).all())
