"""Per-axis periodicity in store.MoleculeStore: items with `cell` may all carry `pbc` (three bools), the flags stay on the device
(bool [M, 3]) and a collated batch gathers `bt.pbc` beside `bt.cell`.  The yardstick is the same items handed over as one
plain-tensor batch with a pbc tensor (inputs and their preconditions: tests/test_pbc_axes.py)."""
import numpy as np
import pytest
import torch

from test_pbc import _record
from test_pbc_axes import CUT_G, CUT_L, PREPARE, PREPARE_AXES, _mixed, _structs, dev  # noqa: F401  (dev: the fixture)

ORDER = [3, 0, 4, 2, 1, 3]                       # a permuted index list, the molecule twice
BUILDER = ('pamnet_mol_graph_pbc_count_i32', 'pamnet_mol_graph_pbc_fill_i32')


def _items(with_pbc=True):
    """[bulk cube, slab, isolated molecule with a zero cell, wire, slab with a zero third vector] as store items."""
    bulk, slab, mol = _mixed()
    s = _structs()
    rng = np.random.RandomState(5)
    items = []
    for st in (bulk, slab, mol, s['wire_min'], s['slab_z']):
        d = dict(x=st.x, pos=st.pos, cell=st.cell, y=np.float32(rng.randn()))
        if with_pbc:
            d['pbc'] = st.pbc
        items.append(d)
    return items


def _plain(items, order, dev):
    from pamnet_amd import synth
    pick = [items[k] for k in order]
    return synth.Batch(x=torch.cat([torch.as_tensor(d['x']) for d in pick]), pos=torch.cat([torch.as_tensor(d['pos']) for d in pick]),
                       batch=torch.cat([torch.full((len(d['x']),), g, dtype=torch.long) for g, d in enumerate(pick)]),
                       cell=torch.stack([torch.as_tensor(d['cell']) for d in pick]),
                       pbc=torch.tensor([d['pbc'] for d in pick], dtype=torch.bool),
                       y=torch.tensor([float(d['y']) for d in pick]), num_graphs=len(pick)).to(dev)


def _model(dev):
    import models
    torch.manual_seed(0)
    return models.PAMNet(models.Config(dataset='QM9', dim=128, n_layer=2, cutoff_l=CUT_L, cutoff_g=CUT_G)).to(dev)


def test_a_store_carries_pbc_as_a_whole():
    """(No GPU: refused before anything is moved to a device.)"""
    from pamnet_amd import store as S
    items = _items()
    some = items[:2] + [{k: v for k, v in items[2].items() if k != 'pbc'}] + items[3:]
    for data_list in (some, some[::-1]):
        with pytest.raises(ValueError, match='every item has its three bools or none does'):
            S.MoleculeStore(data_list, 'cpu')
    with pytest.raises(ValueError, match='`pbc` belongs to periodic items'):
        S.MoleculeStore([{k: v for k, v in d.items() if k != 'cell'} for d in items], 'cpu')
    for bad in ((True, True), (1, 1, 0), 'TTF'):
        with pytest.raises(ValueError, match='three bools'):
            S.MoleculeStore([dict(items[0], pbc=bad)] + items[1:], 'cpu')
    st = S.MoleculeStore(items, 'cpu')                            # accepted: tuples, lists, bool arrays
    assert st.has_pbc and st.pbc.dtype == torch.bool and st.pbc.tolist() == [list(d['pbc']) for d in items]
    st = S.MoleculeStore([dict(d, pbc=np.array(d['pbc'])) for d in items[:2]] + [dict(d, pbc=list(d['pbc'])) for d in items[2:]], 'cpu')
    assert st.pbc.tolist() == [list(d['pbc']) for d in items]


@pytest.mark.gpu
def test_collate_gathers_pbc_and_the_batches_give_the_plain_batchs_bits(dev, monkeypatch):
    from pamnet_amd import store as S
    items = _items()
    model = _model(dev)
    st = S.MoleculeStore(items, dev)
    assert st.has_cell and st.has_pbc and st.pbc.dtype == torch.bool and tuple(st.pbc.shape) == (5, 3) and st.pbc.device.type == 'cuda'
    calls = _record(monkeypatch)
    st.prepare_for(model)                                         # counted with the cells AND their flags: the zero cell passes
    assert PREPARE_AXES in calls and PREPARE not in calls
    bt = st.collate(ORDER)
    assert bt.pbc.dtype == torch.bool and bt.pbc.is_contiguous() and bt.pbc.device.type == 'cuda'
    assert bt.pbc.tolist() == [list(items[k]['pbc']) for k in ORDER] and bt.sizes is None
    assert torch.equal(bt.cell.cpu(), torch.stack([torch.as_tensor(items[k]['cell']) for k in ORDER]))
    assert bt.mol_local[S.size_key(model, False)] is True         # the store's word on the builder is what it was
    ref = _plain(items, ORDER, dev)
    assert torch.equal(bt.pos, ref.pos) and torch.equal(bt.pbc, ref.pbc)

    def run(data):
        del calls[:]
        data.pos.requires_grad_(True)
        out = model(data)
        f, = torch.autograd.grad(out.sum(), data.pos)
        return out.detach(), f, list(calls)

    out, f, used = run(bt)
    want, f_want, used_plain = run(ref)
    assert [c for c in used if c in BUILDER] == list(BUILDER) and not [c for c in used_plain if c in BUILDER]
    assert PREPARE_AXES in used and PREPARE_AXES in used_plain and PREPARE not in used + used_plain
    assert torch.isfinite(want).all() and float(f_want.abs().max()) > 0
    assert torch.equal(out, want) and torch.equal(f, f_want)
    model.verify()


@pytest.mark.gpu
def test_trainer_steps_fed_from_a_store_with_pbc(dev):
    """prepare_for(model) plus two Trainer.step calls with next_data= (the second graph is built on the side stream, which waits
    for `pbc` too): losses and parameters torch.equal to two steps on the same batches as plain tensors."""
    import models
    from oracle import pamnet_oracle as O
    from pamnet_amd import store as S, train
    cfg = models.Config(dataset='QM9', dim=128, n_layer=2, cutoff_l=CUT_L, cutoff_g=CUT_G)
    sd = O.init_state_dict(cfg, seed=3)
    items = _items()
    orders = [[3, 0, 4], [2, 1, 3, 0]]

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
        losses = [tr.step(data[k], next_data=data[k + 1] if k + 1 < len(data) else None) for k in range(len(data))]
        mae = tr.evaluate(data)
        tr.close()
        pred = [out.detach().clone() for _, out in train.predict(model, data)]
        torch.cuda.synchronize()
        return [float(v) for v in losses], {k: v.detach().clone() for k, v in model.state_dict().items()}, mae, pred

    losses_b, sd_b, mae_b, pred_b = run(True)
    losses_s, sd_s, mae_s, pred_s = run(False)
    assert all(np.isfinite(losses_b)) and losses_b == losses_s, (losses_b, losses_s)
    for k in sd_b:
        assert torch.equal(sd_b[k], sd_s[k]), k
    assert not torch.equal(sd_b['embeddings'].cpu(), sd['embeddings'])                # (the steps did update)
    assert mae_b == mae_s and len(pred_b) == len(pred_s) and all(torch.equal(a, b) for a, b in zip(pred_b, pred_s))
