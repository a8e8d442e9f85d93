"""Element tables indexed by atomic number: models.PAMNet / PAMNet_s(config, max_atomic_number=Z) -- `embeddings` is
[Z + 1, dim], row z is the element z, `data.x` carries atomic numbers.  The constructor contract (no GPU needed)."""
import os
import re
import shutil
import subprocess

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'physics-aware-multiplex-gnn_amd', 'csrc')


def _cfg(dim=128, dataset='QM9', n_layer=1):
    import models
    return models.Config(dataset=dataset, dim=dim, n_layer=n_layer, cutoff_l=1.7, cutoff_g=5.0)


def _classes():
    import models
    return models.PAMNet, models.PAMNet_s


@pytest.mark.parametrize('small', [False, True])
def test_table_has_a_row_per_atomic_number(small):
    from pamnet_amd import ops
    cls = _classes()[small]
    assert ops.TYPE_MAX == 8 and ops.TYPE_ROWS_MAX == 128
    for z in (1, 8, 94, 127):
        m = cls(_cfg(16), max_atomic_number=z)
        assert m.max_atomic_number == z and m.num_atom_types == z + 1
        assert tuple(m.embeddings.shape) == (z + 1, 16)
        assert tuple(m.state_dict()['embeddings'].shape) == (z + 1, 16)
    m = cls(_cfg(16))
    assert m.max_atomic_number is None and m.num_atom_types == 5
    m = cls(_cfg(16), num_atom_types=8)
    assert m.max_atomic_number is None and m.num_atom_types == 8


@pytest.mark.parametrize('small', [False, True])
def test_rows_are_drawn_by_the_law_of_the_five_row_table(small):
    """uniform(-sqrt 3, sqrt 3), every row (row 0 included), and the first draw of the stream as for the 5-row table."""
    cls = _classes()[small]
    torch.manual_seed(3)
    e = cls(_cfg(16), max_atomic_number=94).embeddings.detach()
    assert float(e.abs().max()) <= 3 ** 0.5 and float(e.abs().max()) > 1.6
    assert abs(float(e.mean())) < 0.1 and abs(float(e.var()) - 1.0) < 0.1
    assert bool((e.abs().amax(1) > 0).all())
    torch.manual_seed(3)
    again = cls(_cfg(16), max_atomic_number=94).embeddings.detach()
    assert torch.equal(e, again)                                            # seeded like every other parameter


@pytest.mark.parametrize('small', [False, True])
@pytest.mark.parametrize('bad', [0, 128, -1, 1000, 94.0, '94', True, False, None.__class__])
def test_values_outside_the_range_are_refused(small, bad):
    cls = _classes()[small]
    with pytest.raises(ValueError, match='max_atomic_number'):
        cls(_cfg(16), max_atomic_number=bad)


@pytest.mark.parametrize('small', [False, True])
def test_the_keyword_is_keyword_only(small):
    cls = _classes()[small]
    with pytest.raises(TypeError):
        cls(_cfg(16), 7, 6, 5, True, 5, 94)
    with pytest.raises(TypeError):
        cls(_cfg(16), 7, 6, 5, True, 94)


@pytest.mark.parametrize('small', [False, True])
def test_both_ways_to_size_the_table_together_are_refused(small):
    cls = _classes()[small]
    for n in (1, 4, 8):
        with pytest.raises(ValueError, match='max_atomic_number'):
            cls(_cfg(16), num_atom_types=n, max_atomic_number=94)
    assert cls(_cfg(16), num_atom_types=5, max_atomic_number=94).num_atom_types == 95        # (5: the default, not a choice)
    with pytest.raises(ValueError, match='num_atom_types'):                                     # (unchanged)
        cls(_cfg(16), num_atom_types=9)


@pytest.mark.parametrize('dataset', ['PDBbind', 'rna_native'])
def test_other_schemas_are_refused(dataset):
    import models
    with pytest.raises(ValueError, match='max_atomic_number') as e:
        models.PAMNet(_cfg(16, dataset), max_atomic_number=94)
    assert 'QM9 schema' in str(e.value)
    with pytest.raises(ValueError, match='max_atomic_number') as e:
        models.PAMNet_s(_cfg(16, dataset), max_atomic_number=94)
    assert 'QM9 schema' in str(e.value)


@pytest.mark.parametrize('small', [False, True])
def test_padded_width_speaks_the_logical_shape(small):
    cls = _classes()[small]
    torch.manual_seed(0)
    m = cls(_cfg(12), max_atomic_number=94)
    assert m.dim == 16 and m.config_dim == 12 and m.max_atomic_number == 94
    assert tuple(m.state_dict()['embeddings'].shape) == (95, 12)
    assert tuple(m.embeddings.shape) == (95, 16)
    assert m._logical_shapes['embeddings'] == (95, 12)
    assert float(m.embeddings.detach()[:, 12:].abs().max()) == 0.0
    assert bool((m.embeddings.detach()[:, :12].abs().amax(1) > 0).all())
    torch.manual_seed(0)
    twin = cls(_cfg(12), _pad=False, max_atomic_number=94)                   # seed for seed the unpadded model's values
    assert torch.equal(m.state_dict()['embeddings'], twin.state_dict()['embeddings'])
    m48 = cls(_cfg(48), max_atomic_number=94)
    assert tuple(m48.state_dict()['embeddings'].shape) == (95, 48) and tuple(m48.embeddings.shape) == (95, 64)
    m160 = cls(_cfg(160), max_atomic_number=94)
    assert tuple(m160.state_dict()['embeddings'].shape) == (95, 160)


@pytest.mark.parametrize('small', [False, True])
@pytest.mark.parametrize('dim', [16, 12])
def test_checkpoints(small, dim):
    cls = _classes()[small]
    a, b = cls(_cfg(dim), max_atomic_number=94), cls(_cfg(dim), max_atomic_number=94)
    sd = {k: v.clone() for k, v in a.state_dict().items()}
    sd['embeddings'] = torch.randn(95, dim)
    b.load_state_dict(sd, strict=True)
    assert torch.equal(b.state_dict()['embeddings'], sd['embeddings'])
    five = cls(_cfg(dim)).state_dict()
    assert tuple(five['embeddings'].shape) == (5, dim)
    with pytest.raises(RuntimeError, match='size mismatch for embeddings'):
        b.load_state_dict(five, strict=True)
    with pytest.raises(RuntimeError, match='size mismatch for embeddings'):
        cls(_cfg(dim)).load_state_dict(sd, strict=True)


def test_the_abi_declares_the_scratch_query():
    from pamnet_amd import lib
    assert 'pamnet_type_rows_scratch_bytes' in lib.declared_functions()
    assert len(lib.declared_functions()['pamnet_type_rows_scratch_bytes']) == 3
    assert int(re.search(r'#define\s+PAMNET_ABI_VERSION\s+(\d+)', open(lib.HEADER).read()).group(1)) == 18


def test_input_stage_kernels_keep_their_resources(tmp_path):
    """The wide type-row bodies ride in embed_multi_bwd_kernel / embed_multi_reduce_kernel as one more branch: that is allowed
    only while those kernels keep what they had without it (DESIGN, "Element tables") -- no scratch, 240 / 46 registers, the
    same LDS, two workgroups per CU for the backward.  The wide kernels themselves must not spill."""
    hipcc = '/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else shutil.which('hipcc')
    if not hipcc:
        pytest.skip('hipcc not available')
    want = {'embed_multi_fwd_kernel': (149, 47360, 3), 'embed_multi_bwd_kernel': (240, 47616, 2),
            'embed_multi_reduce_kernel': (46, 1056, 8), 'type_rows_grad_kernel': (64, 4096, 8),
            'type_rows_finish_kernel': (44, 0, 8), 'type_rows_grad_wide_kernel': (128, 4112, 4),
            'type_rows_finish_wide_kernel': (64, 0, 8)}
    seen = set()
    for src in ('embed.hip', 'reduce.hip'):
        r = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-I' + os.path.join(REPO, 'include'),
                            '-I' + CSRC, '-ffp-contract=on', '-c', os.path.join(CSRC, src), '-o', str(tmp_path / (src + '.o')),
                            '-Rpass-analysis=kernel-resource-usage'], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        for b in re.split(r'remark: Function Name: ', r.stderr)[1:]:
            for name, (vmax, lds, occ) in want.items():
                if re.search(r'\d+%sE' % name, b.split()[0]):
                    seen.add(name)
                    assert int(re.search(r'ScratchSize \[bytes/lane\]: (\d+)', b).group(1)) == 0, name
                    regs = int(re.search(r'VGPRs: (\d+)', b).group(1)) + int(re.search(r'AGPRs: (\d+)', b).group(1))
                    assert regs <= vmax, (name, regs)
                    assert int(re.search(r'LDS Size \[bytes/block\]: (\d+)', b).group(1)) == lds, name
                    assert int(re.search(r'Occupancy \[waves/SIMD\]: (\d+)', b).group(1)) >= occ, name
    assert seen == set(want), sorted(set(want) - seen)


# ============================================================================================================ on the GPU
ZS = (1, 6, 8, 78)                                  # H, C, O, Pt: the elements of the relabelling tests
TEN = (1, 6, 7, 8, 9, 16, 17, 35, 78, 92)
CUT_L, CUT_G = 2.0, 5.0


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs an MI355X'
    from pamnet_amd import lib
    lib.load()
    return torch.device('cuda:0')


def _record(monkeypatch):
    from pamnet_amd import lib
    calls, real = [], lib.call

    def rec(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(lib, 'call', rec)
    return calls


# ---------------------------------------------------------------------------------------------- parity with the oracle
@pytest.mark.gpu
@pytest.mark.parametrize('small,dim,n_layer,bonded', [(False, 128, 2, False), (False, 32, 2, False), (False, 48, 1, False),
                                                      (False, 160, 1, False), (True, 128, 2, False), (False, 128, 1, True)])
def test_model_parity_with_the_oracle_on_a_table_of_95_rows(dev, monkeypatch, small, dim, n_layer, bonded):
    """tests/test_bondfree.py::test_model_parity_with_the_oracle_on_radius_edges -- its batch, protocol and constants -- with x
    re-drawn from ten atomic numbers and max_atomic_number=94: outputs, forces, every parameter gradient; the table's gradient
    is non-zero in exactly the ten rows."""
    import models
    from oracle import pamnet_oracle as O
    from pamnet_amd import synth, train
    from test_bondfree import CUTOFF_G, _batch, _free, _logical, _oracle_ei
    from test_hip_forces import CANCEL_TOL, GRAD_TOL, TOL, _check_gradients, _ok
    assert (TOL, GRAD_TOL, CANCEL_TOL) == (1e-5, 1e-5, 1e-4)
    b, ei = _batch('b16'), _oracle_ei('b16', 1.7)
    cfg = models.Config(dataset='QM9', dim=dim, n_layer=n_layer, cutoff_l=1.7, cutoff_g=CUTOFF_G)
    fwd = O.pamnet_s_forward if small else O.pamnet_forward
    sd = O.init_state_dict(cfg, seed=7, small=small)
    gen = torch.Generator().manual_seed(11)
    x = torch.tensor(TEN)[torch.randint(0, 10, b.x.shape, generator=gen)].to(b.x.dtype)
    assert sorted(set(x.long().tolist())) == list(TEN)
    sd['embeddings'] = (torch.rand((95, dim), generator=gen) * 2 - 1) * (3 ** 0.5)
    ob = synth.Batch(x=x, batch=b.batch, pos=b.pos, edge_index=ei, y=b.y, num_graphs=b.num_graphs)     # what the oracle sees
    given = _free(ob)
    if bonded:
        given.edge_index = ei[:, ei[0] != ei[1]]
    cls = models.PAMNet_s if small else models.PAMNet
    model = cls(cfg, max_atomic_number=94)
    assert tuple(model.state_dict()['embeddings'].shape) == (95, dim)
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

    data = given.to(dev)
    data.pos.requires_grad_(True)
    out = model(data)
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
    model.zero_grad(set_to_none=True)
    tr = train.Trainer(model, lr=1e-4)
    assert model._one_node() == (model.dim in (16, 32, 64, 128))
    calls = _record(monkeypatch)
    tr.forward_backward(given.to(dev))
    if dim == 128:                                               # the one-launch input stage, not its per-operator fallback
        assert calls.count('pamnet_embed_multi_fwd_f32') == 1 and calls.count('pamnet_embed_multi_bwd_f32') == 1
        assert 'pamnet_type_rows_grad_f32' not in calls and 'pamnet_embed_bwd_f32' not in calls
    _, p32 = oracle(torch.float32, False)
    _, p64 = oracle(torch.float64, False)
    seen = model if model.dim == dim else _logical(model)
    worst = _check_gradients(seen, p64, fwd, sd, cfg, ob, p32=p32)
    print('parameter gradient worst', worst)
    ge = dict(seen.named_parameters())['embeddings'].grad.cpu()
    assert ge.shape == (95, dim)
    assert (ge.abs().amax(1) > 0).nonzero().view(-1).tolist() == list(TEN)
    tr.close()


# -------------------------------------------------------------------------------------- a wide table is a relabelling
def _twins(dev, dim=128, small=False, n_layer=1, seed=5):
    """(model with max_atomic_number=94, model with num_atom_types=4 whose rows 0 .. 3 are the rows 1, 6, 8, 78 of the first);
    every other weight equal."""
    import models
    from oracle import pamnet_oracle as O
    cfg = models.Config(dataset='QM9', dim=dim, n_layer=n_layer, cutoff_l=CUT_L, cutoff_g=CUT_G)
    sd = O.init_state_dict(cfg, seed=seed, small=small)
    gen = torch.Generator().manual_seed(seed)
    table = (torch.rand((95, dim), generator=gen) * 2 - 1) * 3 ** 0.5
    cls = models.PAMNet_s if small else models.PAMNet
    wide, compact = cls(cfg, max_atomic_number=94), cls(cfg, num_atom_types=4)
    wide.load_state_dict(dict(sd, embeddings=table), strict=True)
    compact.load_state_dict(dict(sd, embeddings=table[list(ZS)].clone()), strict=True)
    return wide.to(dev), compact.to(dev), table


def _label(x, wide):
    """x (any non-negative type ids) as compact indices 0 .. 3, or as their atomic numbers."""
    c = torch.as_tensor(x).long() % 4
    return (torch.tensor(ZS)[c] if wide else c).to(torch.float32)


def _relabelled(b, wide, **attrs):
    from pamnet_amd import synth
    d = dict(b.__dict__)
    d['x'] = _label(b.x, wide)
    d.update(attrs)
    return synth.Batch(**d)


def _run(model, data, forces, strain=False):
    model.zero_grad(set_to_none=True)
    if forces:
        data.pos.requires_grad_(True)
    if strain:
        data.strain = torch.zeros(data.num_graphs, 3, 3, device=data.pos.device, requires_grad=True)
    out = model(data)
    out.sum().backward()
    res = {'out': out.detach().clone()}
    if forces:
        res['forces'] = data.pos.grad.clone()
    if strain:
        res['virial'] = data.strain.grad.clone()
    assert all(torch.isfinite(v).all() and float(v.abs().max()) > 0 for v in res.values())
    return res, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


def _same(wide_run, compact_run):
    (rw, gw), (rc, gc) = wide_run, compact_run
    assert rw.keys() == rc.keys() and gw.keys() == gc.keys() and 'embeddings' in gw
    for k in rw:
        assert torch.equal(rw[k], rc[k]), k
    for k in gw:
        if k != 'embeddings':
            assert torch.equal(gw[k], gc[k]), k
    e = gw['embeddings']
    assert torch.equal(e[list(ZS)], gc['embeddings']) and float(gc['embeddings'].abs().amin(1).max()) > 0
    rest = torch.ones(95, dtype=torch.bool)
    rest[list(ZS)] = False
    assert float(e[rest.to(e.device)].abs().max()) == 0.0


def _qm9(count=8, start=0):
    from pamnet_amd import synth
    b = synth.qm9_batch(0, start, count)
    assert int(torch.bincount(b.batch).max()) <= 24
    return b


def _free(b):
    from pamnet_amd import synth
    return synth.Batch(**{k: v for k, v in b.__dict__.items() if k != 'edge_index'})


def _slab_batch():
    """Four molecules split across the in-plane boundary of a slab cell, pbc = (True, True, False) (tests/test_pbc_axes.py)."""
    from test_pbc_axes import _lifted
    return _lifted()[0]


def _small_cells():
    """Cells below twice cutoff_g (4.5 A): a slab and a wire, twice each -- cell_images='all'."""
    from test_pbc_axes import _batch, _structs
    s = _structs()
    return _batch([s['slab_all'], s['wire_all'], s['slab_all'], s['wire_all']])


@pytest.mark.gpu
@pytest.mark.parametrize('route,dim', [('bonded', 128), ('free', 128), ('free', 32), ('slab', 128), ('images', 128),
                                       ('prepare', 128), ('small', 128)])
def test_a_wide_table_is_a_relabelling(dev, route, dim):
    """Atomic numbers from {1, 6, 8, 78} under max_atomic_number=94 against compact indices under num_atom_types=4 with the same
    four rows: outputs, forces, the virial and every shared parameter gradient bit for bit, through the forces route (unfused
    input stage, ops.type_rows) and the training route (one-launch input stage at d = 128); the four rows equal, the other 91
    zero."""
    wide, compact, _ = _twins(dev, dim, small=route == 'small')
    strain, attrs = False, {}
    if route in ('bonded', 'prepare'):
        base = _qm9()
    elif route in ('free', 'small'):
        base = _free(_qm9())
    elif route == 'slab':
        base, strain, attrs = _slab_batch(), True, dict(mol_local=True)
    else:
        base, strain, attrs = _small_cells(), True, dict(cell_images='all')
    assert 4 <= base.num_graphs <= 16 and sorted(set(_label(base.x, True).long().tolist())) == sorted(ZS)

    def both(forces):
        runs = []
        for model, is_wide in ((wide, True), (compact, False)):
            data = _relabelled(base, is_wide, **attrs).to(dev)
            if route == 'prepare':
                if forces:
                    data.pos.requires_grad_(True)
                model.prepare(data)
                assert data._pamnet_prepared is not None
            runs.append(_run(model, data, forces, strain and forces))
        _same(*runs)
    both(True)
    both(False)
    wide.verify(), compact.verify()


@pytest.mark.gpu
@pytest.mark.parametrize('periodic', [False, True])
def test_relabelling_through_a_store_and_predict(dev, monkeypatch, periodic):
    """MoleculeStore with prepare_for and collate -- bonded: the one-call graph engine, which takes the table's size in its
    descriptor; periodic: slabs with pbc -- and train.predict over its batches."""
    import numpy as np
    from pamnet_amd import store as S, synth, train
    wide, compact, _ = _twins(dev)
    if periodic:
        from test_pbc_axes import _lifted
        items = [dict(x=st.x, pos=st.pos, cell=st.cell, pbc=st.pbc, y=np.float32(k)) for k, st in enumerate(_lifted()[2])]
    else:
        items = [synth.qm9_molecule(0, i) for i in range(8)]
    orders = [[3, 0, 2, 1, 3], list(range(len(items)))]
    calls = _record(monkeypatch)
    runs, preds = [], []
    for model, is_wide in ((wide, True), (compact, False)):
        st = S.MoleculeStore([dict(d, x=_label(d['x'], is_wide).numpy()) for d in items], dev).prepare_for(model)
        del calls[:]
        runs.append([_run(model, st.collate(o), forces) for o in orders for forces in (True, False)])
        assert ('pamnet_graph_build_i32' in calls) == (not periodic)
        model.verify()
        preds.append([out.detach().clone() for _, out in train.predict(model, [st.collate(o) for o in orders])])
    for a, b in zip(*runs):
        _same(a, b)
    assert all(torch.equal(a, b) for a, b in zip(*preds)) and len(preds[0]) == 2
    assert all(torch.isfinite(p).all() and p.numel() == len(o) for p, o in zip(preds[0], orders))


@pytest.mark.gpu
def test_an_atomic_number_beyond_the_table_raises_the_input_error(dev):
    from pamnet_amd import store as S, synth
    wide, _, _ = _twins(dev)
    b = _relabelled(_free(_qm9(4)), True)
    bad = _relabelled(_free(_qm9(4)), True)
    bad.x[5] = 95.0
    with torch.no_grad():
        assert torch.isfinite(wide(b.to(dev))).all()
        with pytest.raises(IndexError):                              # plain tensors: the flag comes back with the sizes
            wide(bad.to(dev))
        edge = _relabelled(_free(_qm9(4)), True)
        edge.x[5] = 94.0                                             # the last row is a row
        assert torch.isfinite(wide(edge.to(dev))).all()
    # a store's batch runs without a host round trip: the flag word waits for verify() (tests/test_store.py)
    mols = [synth.qm9_molecule(0, i) for i in range(4)]
    st = S.MoleculeStore([dict(m, x=_label(m['x'], True).numpy()) for m in mols], dev).prepare_for(wide)
    with torch.no_grad():
        wide(st.collate([0, 2, 3]))
        wide.verify()
        bt = st.collate([0, 1, 2])
        bt.x = bt.x.clone()
        bt.x[3] = 95.0
        wide(bt)                                                     # (the one-launch input stage writes a zero row there)
    with pytest.raises(IndexError):
        wide.verify()
    wide.verify()
