"""The narrow-width (dim 16 / 32 / 64) layer-stack engine (csrc/narrow_engine.hip, csrc/narrow_chain.h) in each of its
launch regimes, driven as the product drives it (pamnet_amd.stack.layer_stack on ModuleLists of GlobalMP / LocalMP and a
graph from build_graph) against tests/torch_formulation.py in fp64 on the same inputs.

The batch sizes are derived from the launch constants (restated in tests/narrow_engine_cases.py, guarded by CPU tests that
read the sources):

    n = 5            one partly filled tile in one wave, seven idle waves; every reduction has nblk = 1
    n = 128, 129     a full first row group; a second chain workgroup with one live row
    n = 1100         chain grid 9: the reducer's tail loop only; three layer pairs (a middle pair); the pairs-only local layer
    n = 3105, 4100   chain grids 25 and 33: the reducer's four-load loop once, and once with b = 32 left for the tail loop
    n = 65536        chain grid at its cap, every workgroup one row group
    n = 65537        workgroup 0 walks to a second row group of one row and adds into its partial row (nblk = 512); the row
                     kernels over E_g, E_l, T + P at their backward caps (nblk = 256), reduced by the engine's reducer

Bound, per tensor: err <= max(1e-5, 2 * err32), err = max-normalised error of the engine against the fp64 formulation,
err32 = the same error of the fp32 formulation (both are fp32 evaluations of one formula; the factor 2 allows another order
of summation), 1e-5 = the bound of tests/test_hip_narrow.py.  Nothing is compared with the engine's own output, and no
tensor is left out: outs, atts, the node features after every layer, the gradients of the four inputs and of every parameter.
Every case prints its worst (err, err32) per tensor class (run with -s to collect them)."""
import time

import pytest
import torch

import narrow_engine_cases as C
import torch_formulation as T
from test_hip_narrow import dev                             # noqa: F401  (the module-scoped fixture of the narrow tests)
from test_hip_narrow_walk import BLOCKS, WIDTHS, _err, cap_bwd, cap_fwd

FLOOR = 1e-5

#            n, layer pairs, pairs-only local layer
CASES = [(5, 1, False), (128, 1, False), (129, 1, False), (129, 2, False), (1100, 3, False), (3105, 1, False),
         (4100, 1, False), (4100, 2, False), (65536, 1, False), (65537, 1, False), (65537, 2, False)]
PARAMS = [(n, L, small, d) for n, L, small in CASES for d in WIDTHS] + [(1100, 2, True, 32)]
EXTRA = [(n, d) for n in (129, 4100, 65537) for d in WIDTHS]          # direct gradients, inference forward, determinism
SIZES = sorted({n for n, _, _ in CASES})
CHAIN_GRIDS = {5: 1, 128: 1, 129: 2, 1100: 9, 3105: 25, 4100: 33, 65536: 512, 65537: 512}
BIG = 65537


# ---- CPU: the table against the sources ----------------------------------------------------------------------------------
def test_table_matches_the_sources():
    C.check_sources(C.sources())


def test_guards_notice_a_reshaped_cap():
    """The guard fails on a source whose cap, loop or stride differs (texts edited here, never compiled)."""
    for name, old, new in (
            ('narrow_chain.h', 'constexpr int CHAIN_CAP = 512;', 'constexpr int CHAIN_CAP = 1024;'),
            ('narrow_chain.h', 'constexpr int CHW = 8;', 'constexpr int CHW = 4;'),
            ('narrow_chain.h', 'constexpr int MAXSEG = 32;', 'constexpr int MAXSEG = 64;'),
            ('narrow_chain.h', 'for (; b + 24 < nblk; b += 32) {\n            s0 += src', 'for (; b + 8 < nblk; b += 16) {\n            s0 += src'),
            ('narrow_chain.h', 'return d <= 32; }', 'return d <= 16; }'),
            ('narrow_chain.h', '((m + 15) / 16 + CHW - 1) / CHW;', '((m + 15) / 16 + 2 * CHW - 1) / (2 * CHW);'),
            ('narrow_core.h', 'constexpr int NARROW_BLOCKS = 256;', 'constexpr int NARROW_BLOCKS = 512;'),
            ('narrow_engine.hip', 'TRY(R.take(grid, p.stride, 23, &p.partial));', 'TRY(R.take(grid, p.stride, 24, &p.partial));'),
            ('narrow_engine.hip', '2 * (erow + 64) + (qb + 64);', '(erow + 64) + (qb + 64);')):
        texts = C.sources()
        assert texts[name].count(old) == 1, (name, old)
        texts[name] = texts[name].replace(old, new)
        with pytest.raises(AssertionError):
            C.check_sources(texts)


def test_chain_grids_and_row_groups():
    assert [C.chain_grid(n) for n in SIZES] == [CHAIN_GRIDS[n] for n in SIZES] == [1, 1, 2, 9, 25, 33, 512, 512]
    assert C.GROUP_ROWS == 128 and C.CHAIN_CAP * C.GROUP_ROWS == 65536
    assert C.chain_walk(5) == (1, 1, 1, 5)                       # one partly filled tile: waves 1..7 have no row
    assert C.chain_walk(128) == (1, 1, 1, 128)
    assert C.chain_walk(129) == (2, 2, 1, 1)                     # the second workgroup: one live row
    assert C.chain_walk(65536) == (512, 512, 1, 128)             # the cap without a walk
    assert C.chain_walk(65537) == (512, 513, 2, 1)               # workgroup 0 owns group 512: exactly one row, added
    assert [C.tail_resident(d) for d in WIDTHS] == [True, True, False]


def test_reducer_walk_at_the_tested_block_counts():
    walk = {nblk: C.reducer_walk(nblk) for nblk in (1, 2, 8, 9, 24, 25, 32, 33, 256, 512)}
    four = lambda nblk: [f for f, _, _ in walk[nblk]]
    tail = lambda nblk: [t for _, t, _ in walk[nblk]]
    assert four(1) == [0] * 8 and tail(1) == [1] + [0] * 7                     # one row: seven thread rows add nothing
    assert four(9) == [0] * 8 and tail(9) == [2] + [1] * 7                     # tail loop only
    assert four(25) == [1] + [0] * 7 and tail(25) == [0] + [3] * 7             # the four-load loop once (y = 0), tails beside it
    assert four(33) == [1] * 8 and tail(33) == [1] + [0] * 7                   # ... in every row, b = 32 left over for y = 0
    assert four(256) == [8] * 8 and tail(256) == [0] * 8                       # row kernels at their cap
    assert four(512) == [16] * 8 and tail(512) == [0] * 8                      # chains at their cap
    assert four(24) == [0] * 8 and four(32) == [1] * 8 and tail(32) == [0] * 8


def _small_case_tp_walks(n, d):
    return d == 64 and n >= 3105


_HOST_SIZES = {}


def _estimated_sizes(n, small=False):
    """(E_g, E_l, T + P): counted on the host for the batches up to 4 100 atoms, from the per-atom ratios above that."""
    if n <= 4100:
        if (n, small) not in _HOST_SIZES:
            _HOST_SIZES[(n, small)] = C.host_sizes(C.qm9_batch_of(n), small)
        return _HOST_SIZES[(n, small)]
    eg, el, tp, pairs = C.per_atom_ratios()
    return int(eg * n), int(el * n), int((pairs if small else tp) * n)


def test_sizes_take_the_regimes_they_are_named_for():
    eg_n, el_n, tp_n, pairs_n = C.per_atom_ratios()
    print('ENGINE per atom: E_g %.3f  E_l %.3f  T+P %.3f  pairs %.3f' % (eg_n, el_n, tp_n, pairs_n))
    assert 2.5 < eg_n < 5.0 and 1.8 < el_n < 2.0 and tp_n > 2.0 * pairs_n - el_n - 1e-9 > 5.0
    assert [cap_bwd(d) for d in WIDTHS] == [65536, 32768, 16384] and [cap_fwd(d) for d in WIDTHS] == [131072, 65536, 32768]
    eg, el, tp = _estimated_sizes(BIG)
    for d in WIDTHS:
        r = C.regimes(BIG, eg, el, tp, d)
        assert r['chain_grid'] == C.CHAIN_CAP and r['chain_walks'] and r['last_group_rows'] == 1
        assert min(eg, el, tp) > 1.2 * cap_bwd(16)                              # every row kernel beyond its backward cap
        assert r['bwd_grid'] == dict(eg=BLOCKS, el=BLOCKS, tp=BLOCKS) and all(r['bwd_walks'].values())
    # which forward launches walk: the pre chain over n and the edge projection over E_l (= 2 (n - molecules), about 1.89 n)
    # stay below the d = 16 forward cap and are above the caps at d = 32 (n by one tile) and 64; E_g and T + P are above all three
    walks = {d: C.regimes(BIG, eg, el, tp, d)['fwd_walks'] for d in WIDTHS}
    assert walks[16] == dict(n=False, eg=True, el=False, tp=True)
    assert walks[32] == dict(n=True, eg=True, el=True, tp=True)
    assert walks[64] == dict(n=True, eg=True, el=True, tp=True)
    assert 1.05 * el < cap_fwd(16) and el > 1.2 * cap_fwd(32)
    # the element-wise kernels (one float4 per thread) stride beyond 4096 workgroups at d = 64 only
    assert [C.regimes(BIG, eg, el, tp, d)['ew_strides'] for d in WIDTHS] == [False, False, True]
    # 65 536: no chain walks, the row kernels already do
    r = C.regimes(65536, *_estimated_sizes(65536), 16)
    assert not r['chain_walks'] and r['chain_grid'] == 512 and all(r['bwd_walks'].values())
    # below: no chain and no forward kernel walks; of the backward row kernels only the triplet / pair MLP at d = 64 does, from
    # 3 105 atoms on (T + P is about 7.8 n against a cap of 16 384 rows: its rows reach the reducer with nblk = 256 there)
    for n in (5, 128, 129, 1100, 3105, 4100):
        for d in WIDTHS:
            r = C.regimes(n, *_estimated_sizes(n), d)
            assert not r['chain_walks'] and not any(r['fwd_walks'].values())
            assert r['bwd_walks'] == dict(eg=False, el=False, tp=_small_case_tp_walks(n, d)), (n, d)
    assert C.regimes(5, 20, 8, 32, 64)['bwd_grid'] == dict(eg=1, el=1, tp=1)   # the five-atom molecule: nblk = 1 everywhere


def test_small_molecule_and_exact_atom_counts():
    b = C.qm9_batch_of(5)
    assert C.host_sizes(b) == (20, 8, 32) and C.host_sizes(b, small=True) == (20, 8, 20)
    for n in (128, 129, 1100, 4100):
        b = C.qm9_batch_of(n)
        assert b.x.numel() == n == b.batch.numel() == b.pos.size(0) and int(b.batch[-1]) + 1 == b.num_graphs
        assert bool((b.batch[1:] >= b.batch[:-1]).all()) and int(b.edge_index.max()) < n
        assert bool((b.batch[b.edge_index[0]] == b.batch[b.edge_index[1]]).all())        # bonds stay inside their molecule
        key = b.edge_index[0] * n + b.edge_index[1]
        assert bool((key[1:] > key[:-1]).all())                                           # sorted, no duplicate
    assert C.qm9_batch_of(4100).num_graphs > C.UNIT_MOLS                                  # a tiled copy plus a remainder


def test_reducer_bookkeeping_of_a_layer_pair():
    """Reducer::take in the order of narrow_stack::bwd: the table of 32 destinations flushes twice inside a pair (before the
    projection blocks' take and before the global tail's), the arena never does, and no take can return PAMNET_EINVAL."""
    assert [C.SEGS[k] for k in C.LOCAL_TAKES] == [23, 4, 6, 6] and [C.SEGS[k] for k in C.GLOBAL_TAKES] == [23, 3, 4]
    for n, L, small in CASES + [(1100, 2, True)]:
        ests = [_estimated_sizes(n, small)]
        ests.append((20 * n, 4 * n, 30 * n))                                    # far denser graphs: the same bookkeeping
        for eg, el, tp in ests:
            for d in WIDTHS:
                ev = C.reducer_trace(n, eg, el, tp, d, pairs=L)                  # (raises on PAMNET_EINVAL)
                cap = C.partial_floats(n, d)
                per_pair = [('take', 'tail'), ('take', 'mlp2'), ('flush', 27, 'table'), ('take', 'qblocks'), ('take', 'pre4'),
                            ('flush', 12, 'table'), ('take', 'tail'), ('take', 'global'), ('take', 'pre2'), ('flush', 30, 'pair')]
                got = [e[:2] if e[0] == 'take' else e for e in ev]
                assert got == per_pair * L, (n, d, got)
                for name, nblk, stride, segs in C.pair_takes(n, eg, el, tp, d):
                    assert ((nblk * stride + 63) & ~63) <= cap and segs <= C.MAXSEG
                # the takes of a whole pair fit the arena together: only the table makes the reducer flush
                assert sum((nblk * stride + 63) & ~63 for _, nblk, stride, _ in C.pair_takes(n, eg, el, tp, d)) <= cap
                offs = [e[2] for e in ev if e[0] == 'take']
                assert offs[0] == 0 and offs[2] == 0 and offs[4] == 0 and offs[1] > 0 and offs[3] > 0 and offs[6] > offs[5] > 0


# ---- GPU -----------------------------------------------------------------------------------------------------------------
_GRAPHS = {}


@pytest.fixture(scope='module')
def graphs(dev):
    """n, pairs only -> (graph on the device, seconds it took to collate and build); built once, shared by every width."""
    from pamnet_amd import graph as G

    def get(n, small=False):
        if (n, small) not in _GRAPHS:
            t0 = time.perf_counter()
            b = C.qm9_batch_of(n).to(dev)
            g = G.build_graph('QM9', C.CUTOFF_L, C.CUTOFF_G, 'source_to_target', b.x, b.batch, b.pos, b.edge_index,
                              num_graphs=b.num_graphs, with_triplets=not small, aux_tables=False)
            torch.cuda.synchronize()
            assert g.n == n
            if n <= 4100:                              # the host's count of bonds and triplet / pair rows is the device's
                eg, el, tp = C.host_sizes(b.to('cpu'), small)
                assert (el, tp) == (g.loc.m, g.tp.m) and abs(eg - g.glob.m) <= (0 if n == 5 else 2), (n, eg, el, tp)
            _GRAPHS[(n, small)] = (g, time.perf_counter() - t0)
        return _GRAPHS[(n, small)]
    yield get
    _GRAPHS.clear()


def _layers(d, L, small, dev, seed):
    """The two ModuleLists with every bias, W and W_out moved off their initial values (zero biases would hide bias handling)."""
    from pamnet_amd import modules
    torch.manual_seed(seed)
    gl = torch.nn.ModuleList([modules.GlobalMP(d) for _ in range(L)]).to(dev)
    ll = torch.nn.ModuleList([modules.LocalMP(d, small=small) for _ in range(L)]).to(dev)
    with torch.no_grad():
        for name, p in list(gl.named_parameters()) + list(ll.named_parameters()):
            if p.dim() == 1 or name.endswith('.W') or 'W_out' in name:
                p.add_(0.05 * torch.randn_like(p))
                assert float(p.abs().min()) > 0.0, name
    return gl, ll


def _inputs(g, d, dev, seed):
    gen = torch.Generator().manual_seed(seed)
    mk = lambda rows: (0.5 * torch.randn(rows, d, generator=gen)).to(dev).requires_grad_()
    return [mk(g.n), mk(g.glob.m), mk(g.loc.m), mk(g.tp.m)]


def _head_weights(L, n, dev):
    gen = torch.Generator().manual_seed(7)
    return [torch.randn(2 * L, n, generator=gen, dtype=torch.float64).to(dev) for _ in range(2)]


def _params(gl, ll):
    return [('global_layer.' + k, p) for k, p in gl.named_parameters()] + [('local_layer.' + k, p) for k, p in ll.named_parameters()]


def _engine_run(gl, ll, ins, g, w, monkeypatch=None):
    """One forward and backward through stack.layer_stack -> (outs, atts, x after every layer, input gradients, parameter
    gradients by name); with `monkeypatch`, the names of the library calls made are checked."""
    from pamnet_amd import lib, narrow, stack
    x0, e_g, rbf_e, e_sbf = ins
    assert narrow.engine_supported(x0, g)
    calls = []
    if monkeypatch is not None:
        real = lib.call
        monkeypatch.setattr(lib, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    for t in ins:
        t.grad = None
    outs, atts, saved = stack.layer_stack(gl, ll, x0, e_g, rbf_e, e_sbf, g)
    xs = [x.detach().clone() for x in stack.stack_x_layers(saved, g, len(gl), x0.size(1))]
    ((outs * w[0].float()).sum() + (atts * w[1].float()).sum()).backward()
    torch.cuda.synchronize()
    if monkeypatch is not None:
        monkeypatch.undo()
        assert 'pamnet_stack_fwd_f32' in calls and 'pamnet_stack_bwd_f32' in calls, calls
        assert not [c for c in calls if c.startswith('pamnet_narrow_')], calls             # no per-operator entry point
    return (outs.detach().clone(), atts.detach().clone(), xs, [t.grad for t in ins],
            {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in _params(gl, ll)})


def _copies(gl, ll, dtype):
    """Fresh layers of the same kinds holding the same values in `dtype` (no gradient, no engine plan attached)."""
    from pamnet_amd import modules
    d, p0 = gl[0].dim, next(gl.parameters())
    cg = torch.nn.ModuleList([modules.GlobalMP(d) for _ in gl]).to(p0.device).to(dtype)
    cl = torch.nn.ModuleList([modules.LocalMP(d, small=l.small) for l in ll]).to(p0.device).to(dtype)
    cg.load_state_dict({k: v.detach().to(dtype) for k, v in gl.state_dict().items()})
    cl.load_state_dict({k: v.detach().to(dtype) for k, v in ll.state_dict().items()})
    return cg, cl


def _formulation_run(gl, ll, ins, g, w, dtype):
    """The same through tests/torch_formulation.py on copies of layers and inputs in `dtype`."""
    gl, ll = _copies(gl, ll, dtype)
    x0, e_g, rbf_e, e_sbf = leaves = [t.detach().to(dtype).requires_grad_() for t in ins]
    x, outs, atts, xs = x0, [], [], []
    for lay_g, lay_l in zip(gl, ll):
        x, o, a = T.global_forward(lay_g, x, e_g, g)
        outs.append(o), atts.append(a), xs.append(x)
        x, o, a = T.local_forward(lay_l, x, rbf_e, e_sbf, g)
        outs.append(o), atts.append(a), xs.append(x)
    outs, atts = torch.stack(outs), torch.stack(atts)
    ((outs * w[0].to(dtype)).sum() + (atts * w[1].to(dtype)).sum()).backward()
    return (outs.detach(), atts.detach(), [t.detach() for t in xs], [t.grad for t in leaves],
            {k: p.grad for k, p in _params(gl, ll)})


def _named(run, L):
    """name -> (tensor class, tensor or None) of everything a run returns."""
    outs, atts, xs, d_in, grads = run
    out = {'outs': ('outs', outs), 'atts': ('atts', atts)}
    assert len(xs) == 2 * L
    for k, x in enumerate(xs):
        out['x after %s layer %d' % ('local' if k % 2 else 'global', k // 2)] = ('x_layers', x)
    for name, t in zip(('d x0', 'd e_g', 'd rbf_e', 'd e_sbf'), d_in):
        out[name] = ('d_inputs', t)
    for name, t in grads.items():
        out['d ' + name] = ('d_params', t)
    return out


def _compare(label, eng, r32, r64, L):
    """Every tensor of the engine run against fp64 at max(FLOOR, 2 err32); returns (failures, compared, worst per class)."""
    e, a, b = _named(eng, L), _named(r32, L), _named(r64, L)
    assert list(e) == list(a) == list(b)
    failures, worst, compared = [], {}, 0
    for name, (cls, got) in e.items():
        want32, want64 = a[name][1], b[name][1]
        if want64 is None or got is None:
            if not (want64 is None and got is None):
                failures.append((name, 'a gradient is None on one side only'))
            compared += 1
            continue
        assert got.shape == want64.shape == want32.shape, name
        compared += 1
        if float(want64.abs().max()) == 0.0:
            if float(got.abs().max()) != 0.0:
                failures.append((name, 'reference identically zero, engine not'))
            continue
        err, err32 = _err(got, want64), _err(want32, want64)
        if not err <= max(FLOOR, 2 * err32):
            failures.append((name, err, err32))
        if cls not in worst or err > worst[cls][0]:
            worst[cls] = (err, err32, name)
    for cls in ('outs', 'atts', 'x_layers', 'd_inputs', 'd_params'):
        err, err32, name = worst[cls]
        print('ENGINE %-24s %-9s err=%9.3e err32=%9.3e bound=%9.3e  (%s)' % (label, cls, err, err32, max(FLOOR, 2 * err32), name))
    return failures, compared, len(e)


def _assert_regime(n, g, d):
    """The conditions of test_sizes_take_the_regimes_they_are_named_for on the sizes of the graph the device built."""
    eg, el, tp = g.glob.m, g.loc.m, g.tp.m
    r = C.regimes(n, eg, el, tp, d)
    assert r['chain_grid'] == CHAIN_GRIDS[n]
    if n == BIG:
        assert r['chain_walks'] and r['last_group_rows'] == 1
        assert r['bwd_grid'] == dict(eg=BLOCKS, el=BLOCKS, tp=BLOCKS) and all(r['bwd_walks'].values())
        assert r['fwd_walks'] == dict(n=d != 16, eg=True, el=d != 16, tp=True)
        assert r['ew_strides'] == (d == 64)
    else:
        assert not r['chain_walks']
    if n == 65536:
        assert all(r['bwd_walks'].values())
    if n <= 4100:
        assert not any(r['fwd_walks'].values()) and r['bwd_walks'] == dict(eg=False, el=False, tp=_small_case_tp_walks(n, d))
    if n == 5:
        assert (eg, el, tp) == (20, 8, 32) and r['bwd_grid'] == dict(eg=1, el=1, tp=1)
    return r


@pytest.mark.gpu
@pytest.mark.parametrize('n,L,small,d', PARAMS)
def test_engine_vs_fp64_formulation(dev, graphs, monkeypatch, n, L, small, d):
    g, t_graph = graphs(n, small)
    r = _assert_regime(n, g, d)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    gl, ll = _layers(d, L, small, dev, seed=100 * d + L)
    ins = _inputs(g, d, dev, seed=n + d)
    w = _head_weights(L, n, dev)
    eng = _engine_run(gl, ll, ins, g, w, monkeypatch)
    r64 = _formulation_run(gl, ll, ins, g, w, torch.float64)
    r32 = _formulation_run(gl, ll, ins, g, w, torch.float32)
    label = 'n=%d L=%d d=%d%s' % (n, L, d, ' pairs-only' if small else '')
    failures, compared, total = _compare(label, eng, r32, r64, L)
    torch.cuda.synchronize()
    print('ENGINE %-24s sizes n=%d E_g=%d E_l=%d T+P=%d  chain grid %d  bwd row grids %s  fwd row grids %s  forward walks %s  '
          'element-wise strides %s  case %.2f s (+ graph %.2f s, once per n)'
          % (label, n, g.glob.m, g.loc.m, g.tp.m, r['chain_grid'], r['bwd_grid'], r['fwd_grid'],
             sorted(k for k, v in r['fwd_walks'].items() if v), r['ew_strides'], time.perf_counter() - t0, t_graph))
    assert compared == total                                      # the share of tensors left out is 0
    assert not failures, (label, failures)


@pytest.mark.gpu
@pytest.mark.parametrize('n,d', EXTRA)
def test_direct_gradients_inference_and_determinism(dev, graphs, n, d):
    """Two layer pairs.  A second run returns the bits of the first; the forward under no_grad (no saves) returns the bits of
    the training forward; and with the parameters re-homed by train.FlatParams(direct=True) the backward writes every
    gradient -- the strided [d, 3d] column blocks included -- into the flat buffer with the same launches: the same bits."""
    from pamnet_amd import stack
    from pamnet_amd.train import FlatParams
    L = 2
    g, _ = graphs(n)
    _assert_regime(n, g, d)
    gl, ll = _layers(d, L, False, dev, seed=7 * d + n)
    ins = _inputs(g, d, dev, seed=n + 3 * d)
    w = _head_weights(L, n, dev)

    def clear():
        for _, p in _params(gl, ll):
            p.grad = None

    first = _engine_run(gl, ll, ins, g, w)
    clear()
    second = _engine_run(gl, ll, ins, g, w)
    clear()
    a, b = _named(first, L), _named(second, L)
    for name in a:
        assert a[name][1] is not None and torch.equal(a[name][1], b[name][1]), ('second run', name)
    with torch.no_grad():
        outs, atts, _ = stack.layer_stack(gl, ll, *[t.detach() for t in ins], g)
    assert torch.equal(outs, first[0]) and torch.equal(atts, first[1])
    holder = torch.nn.Module()
    holder.global_layer, holder.local_layer = gl, ll
    fp = FlatParams(holder, direct=True)
    fp.zero_grad()
    plan = stack.stack_plan(gl, ll)
    assert plan.direct()
    direct = _engine_run(gl, ll, ins, g, w)
    assert plan.direct() and all(p.grad.data_ptr() == v.data_ptr() for p, v in zip(fp.params, fp.grad_views))
    c = _named(direct, L)
    for name in a:
        assert c[name][1] is not None and torch.equal(a[name][1], c[name][1]), ('direct gradients', name)
    # the padding between the parameters' slices of the flat gradient buffer stays zero
    used = torch.zeros_like(fp.grad, dtype=torch.bool)
    for name, p in zip(fp.names, fp.params):
        used[fp.offsets[name]:fp.offsets[name] + p.numel()] = True
    assert float(fp.grad[~used].abs().max()) == 0.0 if bool((~used).any()) else True
