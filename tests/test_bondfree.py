"""Bond-free molecules: a QM9-schema batch without `edge_index` gets its local graph from cutoff_l (all ordered pairs
(j -> i), i != j, of one molecule with |pos_i - pos_j| <= cutoff_l) -- pamnet_amd/graph.py build_graph, the bond-free form
of the molecule-local builder (csrc/graph_mol.hip: pamnet_mol_graph_free_count/fill_i32), models.PAMNet(num_atom_types=),
store.MoleculeStore.

The reference forward (models.py:104-115) handed edge_index = radius(pos, pos, cutoff_l, batch, batch) computes the same
thing (get_edge_info strips the self loops): that is the oracle call every parity test here makes.  Every batch is checked
on the CPU in fp64 first: no intramolecular pair within 1e-4 of cutoff_l, so that fp32 and fp64 agree on the edge set.

Parity protocol and constants: tests/test_hip_forces.py (err(hip, oracle_fp64) <= max(1e-5, 2 * err(oracle_fp32, oracle_fp64));
GRAD_TOL, CANCEL_TOL for the scalar head bias)."""
import numpy as np
import pytest
import torch

CUTOFF_G = 5.0
NEW = ('pamnet_mol_graph_free_count_i32', 'pamnet_mol_graph_free_fill_i32')
SEARCHES = ('pamnet_radius_count_i32', 'pamnet_radius_fill_i32', 'pamnet_csr_filter_count_i32', 'pamnet_csr_filter_fill_i32',
            'pamnet_triplet_count_i32', 'pamnet_triplet_fill_f32', 'pamnet_reverse_edges_i32', 'pamnet_csr_from_keys_i32')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs an MI355X'
    from pamnet_amd import lib
    lib.load()
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------------------ inputs
def _free(b):
    """The batch without its bond list."""
    from pamnet_amd import synth
    return synth.Batch(**{k: v for k, v in b.__dict__.items() if k != 'edge_index'})


def _assert_margin(b, cutoff_l):
    """The condition on the inputs: no intramolecular pair within 1e-4 of the cutoff (fp64, on the CPU)."""
    from oracle import pamnet_oracle as O
    for s, e in O._graph_slices(b.batch):
        p = b.pos[s:e].double()
        d = (p[:, None] - p[None]).pow(2).sum(-1).sqrt()
        off = d[~torch.eye(e - s, dtype=torch.bool)]
        assert off.numel() == 0 or float((off - cutoff_l).abs().min()) > 1e-4, (s, e, cutoff_l)
        assert off.numel() == 0 or float(off.min()) > 0.0                   # (coincident atoms: unsupported)


_BATCHES = {}


def _batch(name):
    """(batch with bonds, as synth makes it): made once, never modified."""
    from pamnet_amd import synth
    if name not in _BATCHES:
        _BATCHES[name] = {'b4': lambda: synth.qm9_batch(0, 0, 4), 'b16': lambda: synth.qm9_batch(0, 0, 16),
                          'ragged': synth.ragged_qm9_batch}[name]()
    return _BATCHES[name]


_ORACLE_EI = {}


def _oracle_ei(name, cutoff_l):
    """edge_index = radius(pos, pos, cutoff_l, batch, batch) (self loops included, as torch_cluster returns them)."""
    from oracle import pamnet_oracle as O
    key = (name, float(cutoff_l))
    if key not in _ORACLE_EI:
        b = _batch(name)
        _assert_margin(b, cutoff_l)
        _ORACLE_EI[key] = O.radius_graph(b.pos, b.batch, cutoff_l)
    return _ORACLE_EI[key]


def _build(b, cutoff_l, dev, edge_index=None, **kw):
    from pamnet_amd import graph as G
    kw.setdefault('n_types', 5)
    return G.build_graph('QM9', cutoff_l, CUTOFF_G, 'source_to_target', b.x.to(dev), b.batch.to(dev), b.pos.to(dev),
                         None if edge_index is None else edge_index.to(dev), num_graphs=b.num_graphs, **kw)


def _arrays(g):
    """Every index / geometry array of a graph, by name."""
    out = {'dist_g': g.dist_g, 'dist_l': g.dist_l, 'tp_angle': g.tp_angle, 'tp_kind': g.tp_kind}
    for name in ('glob', 'loc', 'tp'):
        c = getattr(g, name)
        out.update({name + '.ptr': c.ptr, name + '.row_of': c.row_of, name + '.col': c.col})
    for name in ('glob_T', 'loc_T', 'tp_T'):
        t = getattr(g, name)
        if t.ptr is not None:
            out.update({name + '.ptr': t.ptr, name + '.perm': t.perm})
    for name in ('tT_edge', 'tT_node', 'types', 'gptr', 'node_graph'):
        if getattr(g, name, None) is not None:
            out[name] = getattr(g, name)
    if getattr(g, 'seg_cuts', None) is not None:
        # a [260] buffer of which the launch writes grid + 1 words (the grid of the fused edge kernels for this edge count):
        # the rest is whatever the allocation held
        import ctypes
        from pamnet_amd import lib
        grid = ctypes.c_int64(-1)
        tmp = torch.empty_like(g.seg_cuts)
        lib.call('pamnet_seg_cuts_i32', lib.ptr(g.glob.ptr), lib.ptr(g.glob.row_of), g.n, g.glob.m, lib.ptr(tmp),
                 ctypes.addressof(grid), lib.stream_of(tmp))
        assert 1 <= grid.value <= 256
        out['seg_cuts'] = g.seg_cuts[:grid.value + 1]
        assert torch.equal(out['seg_cuts'], tmp[:grid.value + 1])
    return out


def _assert_same_graph(a, b):
    xa, xb = _arrays(a), _arrays(b)
    assert xa.keys() == xb.keys(), (sorted(xa), sorted(xb))
    for k in xa:
        assert xa[k].dtype == xb[k].dtype and torch.equal(xa[k], xb[k]), k


def _record(monkeypatch):
    """Record the symbols passed to lib.call from here on."""
    from pamnet_amd import lib
    calls, real = [], lib.call

    def rec(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(lib, 'call', rec)
    return calls


def _check_lists(g, b, ei, with_triplets=True, expect=None):
    """Test 1's checks of a HIP graph against the oracle's get_edge_info + indices on `ei`."""
    from oracle import pamnet_oracle as O
    n = int(b.x.numel())
    ei_l, dist = O.get_edge_info(ei, b.pos)
    src, dst = g.loc.col.cpu().long(), g.loc.row_of.cpu().long()
    # local edges: the library's order is (target i, source j) -- the oracle's list sorted the same way, exactly
    order = (ei_l[1] * n + ei_l[0]).argsort()
    assert torch.equal(dst, ei_l[1][order]) and torch.equal(src, ei_l[0][order])
    assert g.loc.m == ei_l.size(1)
    ptr = g.loc.ptr.cpu().long()
    assert torch.equal(ptr[1:] - ptr[:-1], torch.bincount(ei_l[1], minlength=n))
    if g.loc.m:
        assert float(((g.dist_l.cpu() - dist[order]).abs() / dist[order]).max()) < 1.3e-7        # fp32, <= 1 ulp apart
    (idx_i, idx_j, idx_k, idx_kj, idx_ji, i_p, j1_p, j2_p, jj_p, ji_p) = O.indices(ei_l, n)
    a2 = O.angle_between(b.pos[idx_j] - b.pos[idx_i], b.pos[idx_k] - b.pos[idx_j])
    a1 = O.angle_between(b.pos[j1_p] - b.pos[i_p], b.pos[j2_p] - b.pos[j1_p])
    e, e2 = g.tp.row_of.cpu().long(), g.tp.col.cpu().long()
    kind, ang = g.tp_kind.cpu(), g.tp_angle.cpu()
    rows = list(zip(e.tolist(), e2.tolist(), kind.tolist(), ang.tolist()))
    mine_t = [((int(src[b_]), int(src[a_]), int(dst[a_])), x) for a_, b_, k_, x in rows if k_ == 0]
    mine_p = [((int(src[a_]), int(dst[a_]), int(src[b_])), x) for a_, b_, k_, x in rows if k_ == 1]
    ref_t = {(int(k), int(j), int(i)): float(x) for k, j, i, x in zip(idx_k, idx_j, idx_i, a2)}
    ref_p = {(int(i), int(j1), int(j2)): float(x) for i, j1, j2, x in zip(i_p, j1_p, j2_p, a1)}
    assert len(ref_t) == idx_kj.numel() and len(ref_p) == jj_p.numel()                      # (no repeated row: sets are multisets)
    if with_triplets:
        assert sorted(k for k, _ in mine_t) == sorted(ref_t)
        if ref_t:
            assert max(abs(x - ref_t[k]) for k, x in mine_t) < 2e-6
    else:
        assert not mine_t
    assert sorted(k for k, _ in mine_p) == sorted(ref_p)
    if ref_p:
        assert max(abs(x - ref_p[k]) for k, x in mine_p) < 2e-3           # self-pairs: atan2(~0, -1): pi up to sqrt noise
    assert torch.equal(e, torch.sort(e).values)                          # rows grouped by target edge
    if expect is not None:
        assert (g.loc.m, len(mine_t), len(mine_p)) == expect
    # the global graph is the radius graph at cutoff_g, as ever
    ei_g, _ = O.get_edge_info(O.radius_graph(b.pos, b.batch, CUTOFF_G), b.pos)
    assert set(zip(g.glob.row_of.tolist(), g.glob.col.tolist())) == set(zip(ei_g[0].tolist(), ei_g[1].tolist()))


# ------------------------------------------------------------------------------------------- 1. lists against the oracle
@pytest.mark.gpu
@pytest.mark.parametrize('mol_local', [None, False])
@pytest.mark.parametrize('name,cutoff_l,expect', [('b4', 1.3, None), ('b4', 1.7, (194, 400, 594)), ('b4', 2.6, None),
                                                  ('ragged', 1.7, None)])
def test_local_lists_match_the_oracle(dev, name, cutoff_l, expect, mol_local):
    """Local edges, triplet / pair rows, lengths and angles of the bond-free graph equal the oracle's get_edge_info + indices on
    radius(pos, pos, cutoff_l), through the molecule-local builder (default) and the step-by-step launches."""
    b, ei = _batch(name), _oracle_ei(name, cutoff_l)
    g = _build(_free(b), cutoff_l, dev, mol_local=mol_local)
    _check_lists(g, b, ei, expect=expect)


@pytest.mark.gpu
@pytest.mark.parametrize('mol_local', [None, False])
@pytest.mark.parametrize('name', ['b4', 'ragged'])
def test_pairs_only(dev, name, mol_local):
    """with_triplets=False (PAMNet_s): the pair rows alone."""
    b, ei = _batch(name), _oracle_ei(name, 1.7)
    g = _build(_free(b), 1.7, dev, mol_local=mol_local, with_triplets=False)
    _check_lists(g, b, ei, with_triplets=False, expect=(194, 0, 594) if name == 'b4' else None)


@pytest.mark.gpu
def test_local_cutoff_above_the_global_one(dev):
    """cutoff_l may lie above cutoff_g: the local search is its own (here cutoff_g = 1.7 would hide edges of cutoff_l = 2.6)."""
    from pamnet_amd import graph as G
    b, ei = _batch('b4'), _oracle_ei('b4', 2.6)
    _assert_margin(b, 1.7)
    f = _free(b)
    for ml in (None, False):
        g = G.build_graph('QM9', 2.6, 1.7, 'source_to_target', f.x.to(dev), f.batch.to(dev), f.pos.to(dev), None, num_graphs=4,
                          n_types=5, mol_local=ml)
        assert g.loc.m == 472 and g.glob.m == 194
        src, dst = g.loc.col.cpu().long(), g.loc.row_of.cpu().long()
        keep = ei[0] != ei[1]
        assert set(zip(dst.tolist(), src.tolist())) == set(zip(ei[1][keep].tolist(), ei[0][keep].tolist()))


# --------------------------------------------------------------------------------- 2. route 2 equals route 1, and is taken
@pytest.mark.gpu
@pytest.mark.parametrize('need_grad', [True, False])
@pytest.mark.parametrize('name,cutoff_l,with_triplets', [('b4', 1.7, True), ('b4', 2.6, True), ('b16', 1.7, True),
                                                         ('ragged', 1.7, True), ('b4', 1.7, False)])
def test_builder_equals_step_by_step_and_is_taken(dev, monkeypatch, name, cutoff_l, with_triplets, need_grad):
    """Every array of the molecule-local builder's graph is bit-identical to the step-by-step route's, and the default run
    really is the builder: its two entry points, none of the step-by-step searches."""
    _oracle_ei(name, cutoff_l)                                           # (asserts the condition on the inputs)
    f = _free(_batch(name))
    calls = _record(monkeypatch)
    fast = _build(f, cutoff_l, dev, need_grad=need_grad, with_triplets=with_triplets)
    fast_calls = list(calls)
    del calls[:]
    slow = _build(f, cutoff_l, dev, need_grad=need_grad, with_triplets=with_triplets, mol_local=False)
    slow_calls = list(calls)
    print(name, cutoff_l, 'default:', fast_calls)
    print(name, cutoff_l, 'mol_local=False:', slow_calls)
    assert [c for c in fast_calls if c in NEW] == list(NEW), fast_calls
    assert not [c for c in fast_calls if c in SEARCHES], fast_calls
    assert not [c for c in slow_calls if c in NEW], slow_calls
    assert slow_calls.count('pamnet_radius_fill_i32') == 2, slow_calls
    _assert_same_graph(fast, slow)
    assert (fast.loc_T.ptr is not None) == need_grad


# ---------------------------------------------------------------------------------------------------------- 3. fallback
@pytest.mark.gpu
def test_a_molecule_over_the_builders_limit_takes_the_step_by_step_route(dev, monkeypatch):
    """cutoff_l = 5.0: the largest molecule of the batch has 306 directed local edges (> 256).  The count launch reports it,
    the graph that comes back is the step-by-step one and passes the oracle checks; nothing raises."""
    from pamnet_amd import graph as G, lib
    b, ei = _batch('b4'), _oracle_ei('b4', 5.0)
    ei_l = ei[:, ei[0] != ei[1]]
    per_mol = torch.bincount(b.batch[ei_l[1]], minlength=4)
    assert int(per_mol.max()) == 306 and ei_l.size(1) == 1152
    f = _free(b)
    # the count launch itself
    ing = G.ingest(f.batch.to(dev), 4, f.x.to(dev), 5)
    pos = f.pos.to(dev)
    mol_tot = torch.empty(16, dtype=torch.int32, device=dev)
    lib.call('pamnet_mol_graph_free_count_i32', lib.ptr(pos), lib.ptr(ing[1]), 77, 4, 5.0, CUTOFF_G, 1, lib.ptr(mol_tot),
             lib.ptr(ing[7]), lib.stream_of(pos))
    mt, tot = mol_tot.view(4, 4).cpu(), ing[7].cpu()
    over = per_mol > 256
    assert int(tot[2]) == 2 and torch.equal(mt[:, 3] == 2, over) and torch.equal(mt[~over, 2].long(), per_mol[~over])
    assert int(tot[3]) == int(per_mol[~over].sum())
    # build_graph: tries the builder, falls back
    calls = _record(monkeypatch)
    g = _build(f, 5.0, dev)
    assert NEW[0] in calls and NEW[1] not in calls and calls.count('pamnet_radius_fill_i32') == 2, calls
    _check_lists(g, b, ei)
    _assert_same_graph(g, _build(f, 5.0, dev, mol_local=False))


# ------------------------------------------------------------------------------------------ 4. a bonded batch is untouched
@pytest.mark.gpu
@pytest.mark.parametrize('mol_local', [None, False])
def test_a_batch_with_bonds_takes_its_old_route(dev, monkeypatch, mol_local):
    b = _batch('b16')
    calls = _record(monkeypatch)
    g1 = _build(b, 5.0, dev, edge_index=b.edge_index, mol_local=mol_local)
    first = list(calls)
    g2 = _build(b, 5.0, dev, edge_index=b.edge_index, mol_local=mol_local)
    assert not [c for c in calls if c in NEW], calls
    assert ('pamnet_mol_graph_fill_i32' in first) == (mol_local is None)
    _assert_same_graph(g1, g2)
    assert g1.loc.m == b.edge_index.size(1)


# ---------------------------------------------------------------------------------------------------- 5. model parity
def _logical(model):
    """The model seen through its logical blocks (a padded width), for _check_gradients: tests/test_hip_model.py's wrapper."""
    class _Logical(object):
        def named_parameters(self_):
            for k, p in model.named_parameters():
                mask, shape = model.logical_mask(k), model._logical_shapes[k]
                q = p.detach()[mask].reshape(shape)
                q.grad = None if p.grad is None else p.grad[mask].reshape(shape)
                if p.grad is not None and not bool(mask.all()):
                    assert float(p.grad[~mask].abs().max()) == 0.0, ('padding gradient', k)
                yield k, q

        def parameters(self_):
            return [q for _, q in self_.named_parameters()]
    return _Logical()


@pytest.mark.gpu
@pytest.mark.parametrize('small,dim,n_layer,n_types', [(False, 128, 2, 5), (False, 32, 2, 8), (False, 48, 1, 5),
                                                       (True, 128, 2, 5)])
def test_model_parity_with_the_oracle_on_radius_edges(dev, small, dim, n_layer, n_types):
    """Forward output, forces and every parameter gradient (L1 loss, Trainer.forward_backward: the one-node tape) of a model fed
    NO edge_index against the oracle fed edge_index = radius(pos, pos, cutoff_l): d = 128, the narrow engine (32, with eight
    atom types: every row of the [8, dim] table gets a gradient), a padded width (48) and PAMNet_s."""
    import models
    from oracle import pamnet_oracle as O
    from pamnet_amd import synth, train
    from test_hip_forces import CANCEL_TOL, GRAD_TOL, TOL, _check_gradients, _ok          # the project's constants / protocol
    assert (TOL, GRAD_TOL, CANCEL_TOL) == (1e-5, 1e-5, 1e-4)
    b, ei = _batch('b16'), _oracle_ei('b16', 1.7)
    cfg = models.Config(dataset='QM9', dim=dim, n_layer=n_layer, cutoff_l=1.7, cutoff_g=CUTOFF_G)
    fwd = O.pamnet_s_forward if small else O.pamnet_forward
    sd = O.init_state_dict(cfg, seed=7, small=small)
    x = b.x
    if n_types != 5:
        gen = torch.Generator().manual_seed(11)
        x = torch.randint(0, n_types, b.x.shape, generator=gen).to(b.x.dtype)
        assert sorted(set(x.long().tolist())) == list(range(n_types))
        sd['embeddings'] = (torch.rand((n_types, dim), generator=gen) * 2 - 1) * (3 ** 0.5)
    ob = synth.Batch(x=x, batch=b.batch, pos=b.pos, edge_index=ei, y=b.y, num_graphs=b.num_graphs)     # what the oracle sees
    free = _free(ob)
    cls = models.PAMNet_s if small else models.PAMNet
    model = cls(cfg) if n_types == 5 else cls(cfg, num_atom_types=n_types)
    assert tuple(model.state_dict()['embeddings'].shape) == (n_types, dim)
    model.load_state_dict(sd, strict=True)
    model = model.to(dev)

    def oracle(dtype, forces):
        p = O.as_params({k: v.detach().to(dtype) for k, v in sd.items()})
        pos = ob.pos.to(dtype).clone().requires_grad_(forces)
        out = fwd(p, cfg, ob.x, ob.batch, pos, ei, dtype=dtype)
        if forces:
            out.sum().backward()
            return out.detach(), pos.grad
        torch.nn.functional.l1_loss(out, ob.y.to(dtype)).backward()
        return out.detach(), p

    # forward output + forces
    data = free.to(dev)
    data.pos.requires_grad_(True)
    out = model(data)
    assert getattr(data, 'edge_index', None) is None
    out.sum().backward()
    F = data.pos.grad
    assert torch.isfinite(F).all()
    ref32, F32 = oracle(torch.float32, True)
    ref64, F64 = oracle(torch.float64, True)
    ok, info = _ok(out.detach().cpu().numpy(), ref32.numpy(), ref64.numpy())
    print('out err / floor', info)
    assert ok, ('out', info)
    ok, info = _ok(F.cpu().numpy(), F32.numpy(), F64.numpy())
    print('force err / floor', info)
    assert ok, ('forces', info)
    # parameter gradients of the L1 loss through the trainer's one-node tape
    model.zero_grad(set_to_none=True)
    tr = train.Trainer(model, lr=1e-4)
    assert model._one_node()
    tr.forward_backward(free.to(dev))
    _, p32 = oracle(torch.float32, False)
    _, p64 = oracle(torch.float64, False)
    seen = model if model.dim == dim else _logical(model)
    worst = _check_gradients(seen, p64, fwd, sd, cfg, ob, p32=p32)
    print('parameter gradient worst', worst)
    if n_types != 5:
        ge = dict(seen.named_parameters())['embeddings'].grad.cpu()
        assert ge.shape == (n_types, dim) and bool((ge.abs().amax(1) > 0).all())       # all eight rows (matched above)
    tr.close()


# ------------------------------------------------------------------------------------------ 6. same lists as explicit bonds
@pytest.mark.gpu
@pytest.mark.parametrize('small', [False, True])
def test_same_lists_as_the_same_edges_given_as_bonds(dev, small):
    import models
    b, ei = _batch('b16'), _oracle_ei('b16', 1.7)
    torch.manual_seed(0)
    cfg = models.Config(dataset='QM9', dim=16, n_layer=1, cutoff_l=1.7, cutoff_g=CUTOFF_G)
    model = (models.PAMNet_s if small else models.PAMNet)(cfg).to(dev)
    bonded = _free(b)
    bonded.edge_index = ei[:, ei[0] != ei[1]]
    with torch.no_grad():
        o1 = model(bonded.to(dev))
        g1 = model._graph_cache
        o2 = model(_free(b).to(dev))
        g2 = model._graph_cache
    assert g1.loc.m == 746
    for name in ('loc.ptr', 'loc.row_of', 'loc.col', 'tp.ptr', 'tp.row_of', 'tp.col', 'tp_kind', 'glob.ptr', 'glob.col'):
        assert torch.equal(_arrays(g1)[name], _arrays(g2)[name]), name
    assert torch.isfinite(o2).all() and o1.shape == o2.shape


# ------------------------------------------------------------------------------------------------------------ 7. store
@pytest.fixture(scope='module')
def free_store(dev):
    import models
    from pamnet_amd import store as S, synth
    mols = [synth.qm9_molecule(0, i) for i in range(24)]
    _assert_margin(synth.collate(mols), 1.7)
    bare = [{k: v for k, v in m.items() if k != 'edge_index'} for m in mols]
    torch.manual_seed(0)
    model = models.PAMNet(models.Config(dataset='QM9', dim=128, n_layer=2, cutoff_l=1.7, cutoff_g=CUTOFF_G)).to(dev)
    st = S.MoleculeStore(bare, dev)
    st.prepare_for(model)
    return st, model, mols


@pytest.mark.gpu
def test_store_forward_without_host_sync(dev, free_store):
    from oracle import pamnet_oracle as O
    from pamnet_amd import store as S, synth
    st, model, mols = free_store
    assert not st.has_edges
    key = S.size_key(model, False)
    assert key != S.size_key(model) and list(st._counts) == [key]         # bonded and bond-free sizes do not share a key
    idx = list(range(24))
    ref_b = synth.collate(mols)
    ei = O.radius_graph(ref_b.pos, ref_b.batch, 1.7)
    eg, el, tp = st._counts[key]
    per_mol = torch.bincount(ref_b.batch[ei[1][ei[0] != ei[1]]], minlength=24)
    assert np.array_equal(el, per_mol.numpy())
    with torch.no_grad():
        plain = _free(ref_b).to(dev)
        ref = model(plain)                                           # plain tensors: sizes read back from the device
        model(st.collate(idx))                                       # warm every cache the first hinted call fills
        torch.cuda.synchronize()
        b = st.collate(idx)
        assert b.edge_index is None and b.sizes[key] == (int(eg.sum()), int(el.sum()), int(tp.sum()))
        torch.cuda.set_sync_debug_mode('error')                      # any synchronising torch call raises from here on
        try:
            out = model(b)
        finally:
            torch.cuda.set_sync_debug_mode('default')
    model.verify()
    assert torch.equal(out, ref)


@pytest.mark.gpu
@pytest.mark.parametrize('which,delta', [(0, -1), (0, +1), (1, -1), (1, +1), (2, -1), (2, +1)])
def test_store_wrong_sizes_are_caught(dev, free_store, which, delta):
    from pamnet_amd import store as S
    from pamnet_amd.graph import GraphCheckError
    st, model, _ = free_store
    key = S.size_key(model, False)
    b = st.collate(list(range(24)))
    sz = list(b.sizes[key])
    sz[which] += delta
    b.sizes = {key: tuple(sz)}
    with torch.no_grad():
        out = model(b)                                               # runs to completion, memory-safe, result invalid
    assert out.shape == (24,)
    with pytest.raises(GraphCheckError):
        model.verify()
    model.verify()                                                   # the pending list is cleared by the raise


# ------------------------------------------------------------------------------------------ 8. Trainer.step end to end
@pytest.mark.gpu
def test_trainer_steps_equal_the_run_on_explicit_bonds(dev):
    """Three Trainer.step calls with next_data= (graphs built on the side stream) on bond-free batches: finite losses, a
    clean close(), and parameters torch.equal to a run fed the same batches with edge_index = radius(pos, pos, cutoff_l)."""
    import models
    from oracle import pamnet_oracle as O
    from pamnet_amd import synth, train
    cfg = models.Config(dataset='QM9', dim=128, n_layer=2, cutoff_l=1.7, cutoff_g=CUTOFF_G)
    sd = O.init_state_dict(cfg, seed=3)
    batches = [synth.qm9_batch(0, 16 * k, 16) for k in range(3)]
    eis = []
    for b in batches:
        _assert_margin(b, 1.7)
        ei = O.radius_graph(b.pos, b.batch, 1.7)
        eis.append(ei[:, ei[0] != ei[1]])

    def run(bonded):
        model = models.PAMNet(cfg)
        model.load_state_dict(sd, strict=True)
        model = model.to(dev)
        tr = train.Trainer(model, lr=1e-3)
        data = []
        for b, ei in zip(batches, eis):
            f = _free(b)
            if bonded:
                f.edge_index = ei
            data.append(f.to(dev))
        losses = [tr.step(data[k], next_data=data[k + 1] if k + 1 < len(data) else None) for k in range(len(data))]
        tr.close()
        torch.cuda.synchronize()
        return [float(v) for v in losses], {k: v.detach().clone() for k, v in model.state_dict().items()}

    losses, free_sd = run(False)
    assert all(np.isfinite(losses)), losses
    losses_b, bonded_sd = run(True)
    print('losses', losses, losses_b)
    for k in free_sd:
        assert torch.equal(free_sd[k], bonded_sd[k]), k
    assert not torch.equal(free_sd['embeddings'].cpu(), sd['embeddings'])          # (the steps did update)


# ------------------------------------------------------------------------------------------------------------ 9. C ABI
@pytest.mark.gpu
def test_new_entry_points_validate_their_arguments(dev):
    import ctypes
    from pamnet_amd import lib
    assert lib.load().pamnet_abi_version() == 18
    pos = torch.zeros((4, 3), device=dev)
    gptr = torch.tensor([0, 4], dtype=torch.int32, device=dev)
    mol_tot = torch.full((4,), 7, dtype=torch.int32, device=dev)
    totals = torch.zeros(4, dtype=torch.int32, device=dev)
    st = lib.stream_of(pos)
    P = lib.ptr

    def count(pos_=pos, gptr_=gptr, n=4, ng=1, cl=1.0, cg=2.0, mt=mol_tot, tot=totals):
        lib.call('pamnet_mol_graph_free_count_i32', P(pos_), P(gptr_), n, ng, cl, cg, 1, P(mt), P(tot), st)

    for kw in (dict(n=-1), dict(ng=0), dict(ng=-3), dict(cl=0.0), dict(cl=-1.0), dict(cg=0.0), dict(cl=float('nan'))):
        with pytest.raises(RuntimeError, match='EINVAL'):
            count(**kw)
    for kw in (dict(pos_=None), dict(gptr_=None), dict(mt=None), dict(tot=None)):
        with pytest.raises(RuntimeError, match='ENULL'):
            count(**kw)
    o = lib.MolGraphOut()
    buf = torch.zeros(64, dtype=torch.int32, device=dev)
    for name, _ in lib.MolGraphOut._fields_:
        setattr(o, name, buf.data_ptr())

    def fill(pos_=pos, gptr_=gptr, n=4, ng=1, nl=0, cl=1.0, cg=2.0, mt=mol_tot, eg=0, tp=0, out=o):
        lib.call('pamnet_mol_graph_free_fill_i32', P(pos_), P(gptr_), n, ng, nl, cl, cg, 1, 1, P(mt), eg, tp,
                 None if out is None else ctypes.addressof(out), st)

    for kw in (dict(n=-1), dict(ng=0), dict(nl=-1), dict(cl=0.0), dict(cg=-2.0), dict(eg=-1), dict(tp=-1)):
        with pytest.raises(RuntimeError, match='EINVAL'):
            fill(**kw)
    missing = lib.MolGraphOut()
    for name, _ in lib.MolGraphOut._fields_:
        setattr(missing, name, buf.data_ptr())
    missing.l_ptr = None
    for kw in (dict(pos_=None), dict(gptr_=None), dict(mt=None), dict(out=None), dict(out=missing)):
        with pytest.raises(RuntimeError, match='ENULL'):
            fill(**kw)
    torch.cuda.synchronize()
    assert int(mol_tot.min()) == 7 and int(totals.abs().max()) == 0 and int(buf.abs().max()) == 0     # nothing was launched


def test_header_declares_the_new_entry_points_at_abi_18():
    """(No GPU: the header and the built library.)"""
    import re
    from pamnet_amd import build, lib
    decl = lib.declared_functions()
    assert all(n in decl for n in NEW)
    assert len(decl[NEW[0]]) == 10 and len(decl[NEW[1]]) == 14
    assert int(re.search(r'#define\s+PAMNET_ABI_VERSION\s+(\d+)', open(lib.HEADER).read()).group(1)) == 18
    import ctypes
    h = ctypes.CDLL(build.build())
    assert h.pamnet_abi_version() == 18 and all(hasattr(h, n) for n in NEW)


# ----------------------------------------------------------------------------------------------------------- 10. errors
def test_num_atom_types_is_checked():
    """(No GPU: constructor checks and the state_dict shape.)"""
    import models
    qm9 = models.Config(dataset='QM9', dim=16, n_layer=1, cutoff_l=1.7, cutoff_g=CUTOFF_G)
    for cls in (models.PAMNet, models.PAMNet_s):
        for bad in (0, 9, -1, 2.5, True):
            with pytest.raises(ValueError, match='num_atom_types'):
                cls(qm9, num_atom_types=bad)
        assert tuple(cls(qm9).embeddings.shape) == (5, 16)                         # the default: state_dict as ever
        assert tuple(cls(qm9, num_atom_types=8).state_dict()['embeddings'].shape) == (8, 16)
        assert tuple(cls(qm9, num_atom_types=1).embeddings.shape) == (1, 16)
        with pytest.raises(TypeError):
            cls(qm9, 7, 6, 5, True, 8)                                             # keyword only
    padded = models.PAMNet(models.Config(dataset='QM9', dim=12, n_layer=1, cutoff_l=1.7, cutoff_g=CUTOFF_G), num_atom_types=7)
    assert tuple(padded.state_dict()['embeddings'].shape) == (7, 12) and tuple(padded.embeddings.shape) == (7, 16)
    for ds in ('PDBbind', 'rna_native'):
        cfg = models.Config(dataset=ds, dim=16, n_layer=1, cutoff_l=2.0, cutoff_g=6.0)
        with pytest.raises(ValueError, match='QM9'):
            models.PAMNet(cfg, num_atom_types=8)
        models.PAMNet(cfg)                                                         # (the default stays accepted)
        with pytest.raises(ValueError, match='num_atom_types'):
            models.PAMNet(cfg, num_atom_types=0)


@pytest.mark.gpu
def test_a_type_index_beyond_the_table_raises_the_input_error(dev):
    import models
    b = _batch('b4')
    cfg = models.Config(dataset='QM9', dim=16, n_layer=1, cutoff_l=1.7, cutoff_g=CUTOFF_G)
    model = models.PAMNet(cfg, num_atom_types=3).to(dev)
    assert int(b.x.max()) >= 3
    with torch.no_grad():
        with pytest.raises(IndexError):                              # plain tensors: the flag comes back with the sizes
            model(_free(b).to(dev))
        ok = _free(b)
        ok.x = ok.x.clamp(max=2)
        assert torch.isfinite(model(ok.to(dev))).all()
