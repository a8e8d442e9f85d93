"""Periodic datasets in store.MoleculeStore: items with `cell` stay on the device, a collated batch carries `bt.cell`, no `sizes`,
and the store's word that every cell fits the molecule-local builder -- such a batch is built by the cell table plus
pamnet_mol_graph_pbc_count/fill_i32.  The yardstick is the same molecules handed over as plain tensors, which take the unchanged
step-by-step periodic route (inputs and their preconditions: tests/test_pbc_builder.py)."""
import numpy as np
import pytest
import torch

from test_pbc import BOX, _record, _scatter
from test_pbc_builder import CUTOFF_G, CUTOFF_L, NEW, PREPARE, STEPS, _batch6, dev  # noqa: F401  (dev: the fixture)

ORDER = [4, 0, 5, 2, 1, 3, 0]                    # a permuted index list, one cell twice


def _items(extra65=False):
    """The six cells of test_pbc_builder._batch6 as store items (x, pos, cell, y); extra65: a seventh of 65 atoms."""
    x, batch, pos, cell = _batch6()
    gen = torch.Generator().manual_seed(5)
    y = torch.randn(7, generator=gen)
    items = [dict(x=x[batch == g].numpy(), pos=pos[batch == g].numpy(), cell=cell[g].numpy(), y=np.float32(y[g])) for g in range(6)]
    if extra65:
        items.append(dict(x=torch.randint(0, 5, (65,), generator=gen).float().numpy(), pos=_scatter(gen, 65, BOX, 0.8).float().numpy(),
                          cell=np.asarray(BOX, dtype=np.float32), y=np.float32(y[6])))
    return items


def _plain(items, order, dev):
    """The items `order` as one plain-tensor batch on the device (no sizes, no word about the builder)."""
    from pamnet_amd import synth
    pick = [items[k] for k in order]
    return synth.Batch(x=torch.cat([torch.as_tensor(d['x']) for d in pick]), pos=torch.cat([torch.as_tensor(d['pos']) for d in pick]),
                       batch=torch.cat([torch.full((len(d['x']),), g, dtype=torch.long) for g, d in enumerate(pick)]),
                       cell=torch.stack([torch.as_tensor(d['cell']) for d in pick]),
                       y=torch.tensor([float(d['y']) for d in pick]), num_graphs=len(pick)).to(dev)


def _model(dev, dim=128, seed=0):
    import models
    torch.manual_seed(seed)
    return models.PAMNet(models.Config(dataset='QM9', dim=dim, n_layer=2, cutoff_l=CUTOFF_L, cutoff_g=CUTOFF_G)).to(dev)


@pytest.mark.gpu
def test_collate_hands_out_the_cells_and_the_builders_word_but_no_sizes(dev, monkeypatch):
    from pamnet_amd import store as S
    items = _items()
    model = _model(dev)
    st = S.MoleculeStore(items, dev)
    assert st.has_cell and st.cell.dtype == torch.float32 and tuple(st.cell.shape) == (6, 3, 3) and st.cell.device.type == 'cuda'
    key = S.size_key(model, False)
    assert st.collate(ORDER).mol_local.get(key) is None                        # nothing counted yet: nothing vouched for
    calls = _record(monkeypatch)
    st.prepare_for(model)
    assert [c for c in calls if c in STEPS] and not [c for c in calls if c in NEW], calls    # counted on the step-by-step route
    del calls[:]
    bt = st.collate(ORDER)
    assert torch.equal(bt.cell.cpu(), torch.stack([torch.as_tensor(items[k]['cell']) for k in ORDER]))
    assert bt.cell.dtype == torch.float32 and bt.cell.is_contiguous()
    assert bt.sizes is None and bt.mol_local[key] is True and bt.edge_index is None and bt.num_graphs == len(ORDER)
    ref = _plain(items, ORDER, dev)
    assert torch.equal(bt.pos, ref.pos) and torch.equal(bt.x, ref.x) and torch.equal(bt.batch.long(), ref.batch)
    with torch.no_grad():
        del calls[:]
        out = model(bt)
        assert [c for c in calls if c in NEW or c in STEPS or c == PREPARE] == [PREPARE, NEW[0], NEW[1]], calls
        del calls[:]
        want = model(ref)
        assert not [c for c in calls if c in NEW] and [c for c in calls if c in STEPS], calls
    model.verify()
    assert torch.isfinite(want).all() and torch.equal(out, want)
    # forces and the virial through the store's batch (the user attaches the strain)
    def grads(data):
        data.pos.requires_grad_(True)
        data.strain = torch.zeros(len(ORDER), 3, 3, device=dev, requires_grad=True)
        return torch.autograd.grad(model(data).sum(), [data.pos, data.strain])
    f_b, w_b = grads(st.collate(ORDER))
    f_s, w_s = grads(_plain(items, ORDER, dev))
    assert float(f_s.abs().max()) > 0 and torch.equal(f_b, f_s) and torch.equal(w_b, w_s)


@pytest.mark.gpu
def test_a_store_with_a_cell_over_the_limit_does_not_vouch(dev, monkeypatch):
    from pamnet_amd import store as S
    items = _items(extra65=True)
    model = _model(dev)
    st = S.MoleculeStore(items, dev).prepare_for(model)
    order = [6, 1, 0, 3]
    bt = st.collate(order)
    assert bt.sizes is None and bt.mol_local[S.size_key(model, False)] is False
    calls = _record(monkeypatch)
    with torch.no_grad():
        out = model(bt)
        assert not [c for c in calls if c in NEW] and [c for c in calls if c in STEPS], calls
        want = model(_plain(items, order, dev))
    assert torch.equal(out, want)


def test_a_store_is_periodic_as_a_whole_and_bond_free():
    """(No GPU: refused before anything is moved to a device.)"""
    from pamnet_amd import store as S, synth
    items = _items()
    mixed = items[:3] + [{k: v for k, v in items[3].items() if k != 'cell'}] + items[4:]
    with pytest.raises(ValueError, match='every item carries `cell`'):
        S.MoleculeStore(mixed, 'cpu')
    with pytest.raises(ValueError, match='every item carries `cell`'):
        S.MoleculeStore(mixed[::-1], 'cpu')
    bonded = [dict(synth.qm9_molecule(0, i), cell=np.eye(3, dtype=np.float32) * 40) for i in range(3)]
    with pytest.raises(ValueError, match='periodic batches are bond-free'):
        S.MoleculeStore(bonded, 'cpu')
    rows = [dict(x=np.zeros((5, 4), dtype=np.float32), cell=np.eye(3, dtype=np.float32) * 40, y=np.float32(0)) for _ in range(2)]
    with pytest.raises(ValueError, match='QM9 schema'):
        S.MoleculeStore(rows, 'cpu')
    with pytest.raises(ValueError, match=r'\[3, 3\]'):
        S.MoleculeStore([dict(items[0], cell=np.zeros(9, dtype=np.float32))], 'cpu')


@pytest.mark.gpu
def test_trainer_steps_fed_from_the_store_leave_the_same_parameters(dev, monkeypatch):
    """Two Trainer.step calls with next_data= (graphs built on the side stream): parameters torch.equal to two steps on the same
    batches as plain tensors; evaluate and train.predict agree too."""
    import models
    from oracle import pamnet_oracle as O
    from pamnet_amd import store as S, train
    cfg = models.Config(dataset='QM9', dim=128, n_layer=2, cutoff_l=CUTOFF_L, cutoff_g=CUTOFF_G)
    sd = O.init_state_dict(cfg, seed=3)
    items = _items()
    orders = [[4, 0, 5], [2, 1, 3, 0]]
    calls = _record(monkeypatch)

    def run(from_store):
        model = models.PAMNet(cfg)
        model.load_state_dict(sd, strict=True)
        model = model.to(dev)
        if from_store:
            st = S.MoleculeStore(items, dev).prepare_for(model)
            data = [st.collate(o) for o in orders]
        else:
            data = [_plain(items, o, dev) for o in orders]
        tr = train.Trainer(model, lr=1e-3)
        del calls[:]
        losses = [tr.step(data[k], next_data=data[k + 1] if k + 1 < len(data) else None) for k in range(len(data))]
        used = [c for c in calls if c in NEW]
        mae = tr.evaluate(data)
        tr.close()
        pred = [out.detach().clone() for _, out in train.predict(model, data)]
        torch.cuda.synchronize()
        return ([float(v) for v in losses], {k: v.detach().clone() for k, v in model.state_dict().items()}, used, mae,
                pred)

    losses_b, sd_b, used_b, mae_b, pred_b = run(True)
    losses_s, sd_s, used_s, mae_s, pred_s = run(False)
    assert sorted(used_b) == sorted(NEW * 2) and not used_s, (used_b, used_s)         # (the second graph: on the worker)
    assert all(np.isfinite(losses_b)) and losses_b == losses_s, (losses_b, losses_s)
    for k in sd_b:
        assert torch.equal(sd_b[k], sd_s[k]), k
    assert not torch.equal(sd_b['embeddings'].cpu(), sd['embeddings'])                # (the steps did update)
    assert mae_b == mae_s and len(pred_b) == len(pred_s) and all(torch.equal(a, b) for a, b in zip(pred_b, pred_s))


@pytest.mark.gpu
def test_an_open_space_store_calls_neither_new_entry_point(dev, monkeypatch):
    from pamnet_amd import store as S, synth
    mols = [synth.qm9_molecule(0, i) for i in range(8)]
    bare = [{k: v for k, v in m.items() if k != 'edge_index'} for m in mols]
    model = _model(dev)
    calls = _record(monkeypatch)
    for data_list in (mols, bare):
        st = S.MoleculeStore(data_list, dev).prepare_for(model)
        assert not st.has_cell and st.cell is None
        bt = st.collate(list(range(8)))
        assert not hasattr(bt, 'cell') and bt.sizes
        with torch.no_grad():
            assert torch.isfinite(model(bt)).all()
    model.verify()
    assert not [c for c in calls if c in NEW or c == PREPARE], calls
