"""Trainer(param_groups=..., decoupled_weight_decay=..., accumulate=...) on the CPU (`-m "not gpu"`): group resolution, the
torch path (native_optimizer=False: the cross-check of the fused kernel) against torch's own optimiser used the ordinary way on
a twin module with per-tensor parameters, frozen slices, gradient accumulation (one process and 2 gloo ranks), checkpoints, and
the argument refusals of the new C entry points (nothing here launches a kernel: every refused call returns before the library
touches its "device" addresses, which are made-up integers)."""
import copy
import ctypes
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

from standin import LayeredStandIn

F = torch.nn.functional
EMA = 0.999                                   # min(0.999, (1 + n) / (10 + n)) at n = 99 999 (utils/ema.py:14)

GROUPS = [
    {'params': ['embeddings', 'global_layer.0.*', 'local_layer.0.*'], 'frozen': True},
    {'params': ['*.bias', 'rbf_g.freq'], 'weight_decay': 0.0},
    {'params': ['*.W_out.*', '*.W'], 'lr_scale': 10.0, 'weight_decay': 1e-2},
]
WD = 1e-3                                     # the constructor's decay: the default group's, and group 1's (frozen: unused)


def _hand_table(n_layer=2):
    """The assignment GROUPS gives LayeredStandIn(n_layer=2)'s names, written out by hand (first match wins: a bias of layer 0
    is frozen, the bias of a W_out head takes the no-decay group, not the heads' group)."""
    assert n_layer == 2
    t = {'embeddings': 1, 'rbf_g.freq': 2, 'mlp_rbf_g.0.0.weight': 0, 'mlp_rbf_g.0.0.bias': 2}
    for side in ('global_layer', 'local_layer'):
        for leaf in ('mlp_x1.0.0.weight', 'mlp_x1.0.0.bias', 'W_out.weight', 'W_out.bias', 'W'):
            t['%s.0.%s' % (side, leaf)] = 1
        t['%s.1.mlp_x1.0.0.weight' % side] = 0
        t['%s.1.mlp_x1.0.0.bias' % side] = 2
        t['%s.1.W_out.weight' % side] = 3
        t['%s.1.W_out.bias' % side] = 2
        t['%s.1.W' % side] = 3
    return t


# ------------------------------------------------------------------------------------------------------ group resolution
def test_group_resolution_against_a_hand_written_table():
    from pamnet_amd.train import Trainer
    tr = Trainer(LayeredStandIn(n_layer=2), weight_decay=WD, param_groups=GROUPS, native_optimizer=False)
    assert tr.group_of == _hand_table()
    assert set(tr.group_of) == set(tr.fp.names)
    assert tr.groups == [{'lr_scale': 1.0, 'weight_decay': WD, 'frozen': False},
                         {'lr_scale': 1.0, 'weight_decay': WD, 'frozen': True},
                         {'lr_scale': 1.0, 'weight_decay': 0.0, 'frozen': False},
                         {'lr_scale': 10.0, 'weight_decay': 1e-2, 'frozen': False}]
    # no groups: everything in the default group, the constructor's values
    d = Trainer(LayeredStandIn(n_layer=2), weight_decay=WD, native_optimizer=False)
    assert set(d.group_of.values()) == {0} and d.groups == [{'lr_scale': 1.0, 'weight_decay': WD, 'frozen': False}]
    assert d.micro_step == 0 and d.accumulate == 1
    # the order of the groups decides: with the heads' group first, the head biases are its own
    swapped = Trainer(LayeredStandIn(n_layer=2), param_groups=[GROUPS[2], GROUPS[1]], native_optimizer=False)
    assert swapped.group_of['global_layer.1.W_out.bias'] == 1 and swapped.group_of['global_layer.1.mlp_x1.0.0.bias'] == 2
    assert swapped.group_of['embeddings'] == 0


@pytest.mark.parametrize('groups,word', [
    ([{'params': ['*.bias', 'no_such_layer.*']}], 'no_such_layer.*'),
    ([{'params': ['*.bias'], 'learning_rate': 0.1}], 'learning_rate'),
    ([{'params': ['*.bias'], 'lr_scale': -1.0}], 'lr_scale'),
    ([{'params': ['*.bias'], 'weight_decay': -1e-3}], 'weight_decay'),
    ([{'params': ['*.bias']}] * 16, '16'),
    ([{'lr_scale': 2.0}], 'params'),
])
def test_group_resolution_refusals_name_the_offender(groups, word):
    from pamnet_amd.train import Trainer
    with pytest.raises(ValueError, match=word.replace('*', r'\*').replace('.', r'\.')):
        Trainer(LayeredStandIn(n_layer=2), param_groups=groups, native_optimizer=False)


def test_fifteen_groups_are_accepted_and_accumulate_is_validated():
    from pamnet_amd.train import Trainer
    tr = Trainer(LayeredStandIn(n_layer=2), param_groups=[{'params': ['*.bias']}] * 15, native_optimizer=False)
    assert set(tr.group_of.values()) == {0, 1} and len(tr.groups) == 16
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError, match='accumulate'):
            Trainer(LayeredStandIn(n_layer=2), accumulate=bad, native_optimizer=False)


# ---------------------------------------------------------------------------------------- torch path against the twin
def _twin_run(model0, batches, lrs, decoupled, ema, max_norm):
    """torch's optimiser the ordinary way: a twin with per-tensor parameters, the groups of _hand_table() built by hand,
    clip_grad_norm_ over the trainable parameters, the reference-style EMA over the trainable parameters."""
    twin = LayeredStandIn(n_layer=2)
    twin.load_state_dict(model0)
    table = _hand_table()
    named = dict(twin.named_parameters())
    spec = {0: (1.0, WD), 2: (1.0, 0.0), 3: (10.0, 1e-2)}
    pgs = [{'params': [named[n] for n in sorted(named) if table[n] == g], 'weight_decay': wd, 'scale': sc}
           for g, (sc, wd) in spec.items()]
    trainable = [p for pg in pgs for p in pg['params']]
    assert len(trainable) == sum(1 for g in table.values() if g != 1)
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(pgs, lr=1.0, betas=(0.9, 0.999), eps=1e-8)
    shadow = {n: p.detach().clone() for n, p in named.items()}
    norms = []
    for b, lr in zip(batches, lrs):
        for pg in opt.param_groups:
            pg['lr'] = lr * pg['scale']
        twin.zero_grad()
        F.l1_loss(twin(b), b.y).backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(trainable, max_norm=max_norm, norm_type=2)))
        opt.step()
        if ema:
            for n, p in named.items():
                if table[n] != 1:
                    shadow[n] = (1.0 - EMA) * p.detach() + EMA * shadow[n]
    state = {n: opt.state.get(p, {}) for n, p in named.items()}
    return {n: p.detach() for n, p in named.items()}, shadow, norms, state


@pytest.mark.parametrize('decoupled,ema', [(False, True), (True, True), (False, False)], ids=['l2', 'adamw', 'l2-no-ema'])
def test_torch_path_matches_a_twin_with_hand_built_groups(decoupled, ema):
    """Three groups, one frozen, four steps with a changing rate and an active clip.  Bound: the "few ulp" of the existing
    native-vs-torch test (rtol = atol = 1e-6).  Frozen slices: bitwise their initial values in the parameters and the shadow,
    moments exactly zero."""
    from pamnet_amd import synth
    from pamnet_amd.train import Trainer
    torch.manual_seed(3)
    model = LayeredStandIn(n_layer=2)
    model0 = copy.deepcopy(model.state_dict())
    batches = [synth.qm9_batch(1, 9 * i, 9) for i in range(4)]
    lrs = [1e-2 * (i + 1) for i in range(4)]
    max_norm = 0.05
    tr = Trainer(model, lr=1e-2, weight_decay=WD, ema_decay=EMA if ema else None, max_grad_norm=max_norm,
                 native_optimizer=False, param_groups=GROUPS, decoupled_weight_decay=decoupled)
    init_flat = tr.fp.flat.clone()
    norms = []
    for b, lr in zip(batches, lrs):
        tr.step(b, lr=lr)
        norms.append(float(tr.last_grad_norm))
    ref_p, ref_s, ref_norms, ref_state = _twin_run(model0, batches, lrs, decoupled, ema, max_norm)
    assert min(ref_norms) > max_norm                                    # the clip was binding on every step
    assert torch.allclose(torch.tensor(norms), torch.tensor(ref_norms), rtol=1e-6, atol=0)
    m, v = tr.adam_moments()
    table = _hand_table()
    assert (tr.shadow is not None) == ema
    for n, p in zip(tr.fp.names, tr.fp.params):
        o, k = tr.fp.offsets[n], p.numel()
        got = tr.fp.flat[o:o + k].view_as(p)
        if table[n] == 1:                                                # frozen
            assert torch.equal(got, model0[n]) and torch.equal(tr.fp.flat[o:o + k], init_flat[o:o + k]), n
            assert torch.equal(ref_p[n], model0[n])
            if ema:
                assert torch.equal(tr.shadow[o:o + k], init_flat[o:o + k]), n
            assert float(m[o:o + k].abs().max()) == 0.0 and float(v[o:o + k].abs().max()) == 0.0, n
            continue
        assert not torch.equal(got, model0[n]), n
        assert torch.allclose(got, ref_p[n], rtol=1e-6, atol=1e-6), n
        assert torch.allclose(m[o:o + k].view_as(p), ref_state[n]['exp_avg'], rtol=1e-6, atol=1e-6), n
        if ema:
            assert torch.allclose(tr.shadow[o:o + k].view_as(p), ref_s[n], rtol=1e-6, atol=1e-6), n
    # the decay modes differ where there is decay, so the comparison above tells them apart
    if decoupled:
        other_p = _twin_run(model0, batches, lrs, False, ema, max_norm)[0]
        n = 'global_layer.1.W_out.weight'
        assert not torch.allclose(other_p[n], ref_p[n], rtol=1e-6, atol=1e-6)


def test_no_options_keeps_the_single_flat_parameter_of_the_torch_path():
    """Old torch-mode checkpoints hold ONE parameter's state: the default trainer must still build exactly that."""
    from pamnet_amd.train import Trainer
    tr = Trainer(LayeredStandIn(n_layer=2), native_optimizer=False, param_groups=None, decoupled_weight_decay=False,
                 accumulate=1)
    assert len(tr.opt.param_groups) == 1 and len(tr.opt.param_groups[0]['params']) == 1
    assert tr.opt.param_groups[0]['params'][0].data_ptr() == tr.fp.flat.data_ptr()
    assert type(tr.opt) is torch.optim.Adam and tr.acc is None


# -------------------------------------------------------------------------------------------------------- accumulation
class Tiny(nn.Module):
    """Per-graph scalar from node features: sum-pool of an MLP (graphs are independent units, like PAMNet)."""

    def __init__(self):
        super().__init__()
        self.a, self.b = nn.Linear(6, 16), nn.Linear(16, 1)

    def forward(self, data):
        h = self.b(torch.tanh(self.a(data.x))).view(-1)
        return torch.zeros(data.num_graphs, dtype=h.dtype).index_add_(0, data.batch, h)


class D(object):
    pass


def _batch(lo, hi, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    sizes = torch.randint(3, 9, (64,), generator=g)
    xs = [torch.randn(int(s), 6, generator=g) for s in sizes]
    ys = torch.randn(64, generator=g)
    d = D()
    d.x = torch.cat(xs[lo:hi]).to(dtype)
    d.batch = torch.repeat_interleave(torch.arange(hi - lo), sizes[lo:hi])
    d.y, d.num_graphs = ys[lo:hi].to(dtype), hi - lo
    return d


def _fp64_gradient(state, lo, hi, denom):
    """d/dparams of sum_{graphs lo..hi} |out - y| / denom from ONE fp64 autograd run."""
    twin = Tiny().double()
    twin.load_state_dict({k: v.double() for k, v in state.items()})
    b = _batch(lo, hi, dtype=torch.float64)
    ((twin(b) - b.y).abs().sum() / denom).backward()
    return {n: p.grad for n, p in twin.named_parameters()}


def _assert_fp32_close(tr, acc, ref):
    """fp32 rounding: every term of these sums (over at most ~130 nodes) carries 2**-24 = 6e-8 of relative error, so the sum is
    within ~1e-5 of the tensor's largest entry -- the project's parity metric max|a - b| / max|b| at its 1e-5."""
    for n, p in zip(tr.fp.names, tr.fp.params):
        o = tr.fp.offsets[n]
        got = acc[o:o + p.numel()].view_as(p).double()
        err = float((got - ref[n]).abs().max() / ref[n].abs().max())
        assert err <= 1e-5, (n, err)


MICRO = [(0, 3), (3, 8), (8, 10), (10, 16)]            # 3 + 5 + 2 + 6 graphs


def test_accumulated_gradient_is_the_union_batch_gradient():
    """Four micro-batches of unequal graph counts, global_graphs = 16: the sum the update will use is the gradient of the mean
    loss over the union batch (one fp64 autograd run)."""
    from pamnet_amd.train import Trainer
    torch.manual_seed(7)
    model = Tiny()
    state = copy.deepcopy(model.state_dict())
    # five calls per cycle: after the four micro-batches the whole sum is still there to be read
    tr = Trainer(model, lr=1e-2, native_optimizer=False, accumulate=5)
    for i, (lo, hi) in enumerate(MICRO):
        loss = tr.step(_batch(lo, hi), global_graphs=16)
        assert tr.micro_step == i + 1
        b = _batch(lo, hi)
        assert abs(float(loss.detach()) - float(F.l1_loss(Tiny_from(state)(b), b.y).detach())) < 1e-6        # the micro-batch's own mean loss
    assert not hasattr(tr, 'last_grad_norm')                             # no update yet
    assert torch.equal(tr.fp.flat, Trainer(Tiny_from(state), native_optimizer=False).fp.flat)
    _assert_fp32_close(tr, tr.accumulated_grad(), _fp64_gradient(state, 0, 16, 16.0))
    assert float(tr.fp.grad.abs().max()) == 0.0                           # each call's gradient moved into the sum


def Tiny_from(state):
    m = Tiny()
    m.load_state_dict(state)
    return m


def test_accumulation_cycle_updates_on_every_kth_call_with_that_calls_rate():
    from pamnet_amd.train import Trainer
    torch.manual_seed(7)
    model = Tiny()
    state = copy.deepcopy(model.state_dict())
    tr = Trainer(model, lr=1e-2, native_optimizer=False, accumulate=4, max_grad_norm=None)
    before = tr.fp.flat.clone()
    for i, (lo, hi) in enumerate(MICRO[:3]):
        tr.step(_batch(lo, hi), lr=123.0, global_graphs=16)              # a rate that must never be used
        assert tr.micro_step == i + 1 and torch.equal(tr.fp.flat, before) and torch.equal(tr.shadow, before)
    # the partial sum: the first three micro-batches' share of the union mean
    _assert_fp32_close(tr, tr.accumulated_grad(), _fp64_gradient(state, 0, 10, 16.0))
    with torch.no_grad():
        mae = tr.evaluate([_batch(0, 16)])                                # mid-cycle evaluation keeps the partial sum
    assert mae > 0
    _assert_fp32_close(tr, tr.accumulated_grad(), _fp64_gradient(state, 0, 10, 16.0))
    tr.step(_batch(*MICRO[3]), lr=1e-3, global_graphs=16)
    assert tr.micro_step == 0 and float(tr.accumulated_grad().abs().max()) == 0.0
    ref = _fp64_gradient(state, 0, 16, 16.0)
    gn = float(torch.sqrt(sum((g ** 2).sum() for g in ref.values())))
    assert abs(float(tr.last_grad_norm) / gn - 1) < 1e-5
    # Adam's first step moves every parameter with a non-zero gradient by the UPDATE call's rate
    moved = (tr.fp.flat - before).abs().max()
    assert 0.5e-3 < float(moved) <= 1.0001e-3
    norm = float(tr.last_grad_norm)
    tr.step(_batch(0, 3), global_graphs=16)
    assert float(tr.last_grad_norm) == norm and tr.micro_step == 1       # changes on update calls only


def test_the_pieces_refuse_to_update_from_a_sum_they_did_not_build():
    """forward_backward() + clip() / optimizer_step() one by one is what a default trainer allows; with accumulate > 1 only
    step() adds a gradient to the sum, so the pieces raise instead of updating without it."""
    from pamnet_amd.train import Trainer
    torch.manual_seed(7)
    tr = Trainer(Tiny(), lr=1e-2, native_optimizer=False, accumulate=2)
    before = tr.fp.flat.clone()
    tr.forward_backward(_batch(0, 8))
    with pytest.raises(RuntimeError, match='step\\(\\)'):
        tr.clip()
    assert torch.equal(tr.fp.flat, before)
    d = Trainer(Tiny(), lr=1e-2, native_optimizer=False)                  # the default trainer: the pieces work as before
    d.forward_backward(_batch(0, 8))
    d.clip(), d.optimizer_step(), d.ema_update()
    assert not torch.equal(d.fp.flat, before)


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    from pamnet_amd.train import Trainer, shard_range
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.manual_seed(rank)                      # different seeds: the trainer broadcasts rank 0's parameters
    tr = Trainer(LayeredStandIn(), lr=1e-2, world_size=world, accumulate=2)
    assert tr._buckets is None                   # one exchange per update, on the sum
    for upd in range(2):
        for j in range(2):
            lo, hi = shard_range(13, rank, world)
            base = 26 * upd + 13 * j
            before = tr.fp.flat.clone()
            tr.step(_batch(base + lo, base + hi), global_graphs=26)
            assert torch.equal(before, tr.fp.flat) == (j == 0)
    if rank == 0:
        torch.save({'flat': tr.fp.flat.clone(), 'shadow': tr.shadow.clone(), 'norm': float(tr.last_grad_norm)}, out)
    ref = tr.fp.flat.clone()
    dist.broadcast(ref, 0)
    assert torch.equal(ref, tr.fp.flat)
    dist.destroy_process_group()


def test_accumulate_two_on_two_ranks_matches_single_process_on_the_union(tmp_path):
    """2 ranks x 2 micro-batches of 7 + 6 graphs = one update over 26 graphs == the single-process step on those 26 graphs
    (the pattern and the bounds of test_dp_matches_single_process)."""
    from pamnet_amd.train import Trainer
    out = str(tmp_path / 'acc.pt')
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    got = torch.load(out)
    torch.manual_seed(0)
    tr = Trainer(LayeredStandIn(), lr=1e-2, world_size=1)
    for upd in range(2):
        tr.step(_batch(26 * upd, 26 * upd + 26))
    assert torch.allclose(got['flat'], tr.fp.flat, rtol=1e-5, atol=1e-6)
    assert torch.allclose(got['shadow'], tr.shadow, rtol=1e-5, atol=1e-6)
    assert abs(got['norm'] / float(tr.last_grad_norm) - 1) < 1e-5


# --------------------------------------------------------------------------------------------------------- checkpoints
def test_checkpoint_in_mid_cycle_resumes_bit_for_bit():
    from pamnet_amd import synth
    from pamnet_amd.train import Trainer
    kw = dict(lr=1e-2, weight_decay=WD, native_optimizer=False, param_groups=GROUPS, decoupled_weight_decay=True,
              accumulate=2)
    batches = [synth.qm9_batch(2, 5 * i, 5) for i in range(6)]
    torch.manual_seed(2)
    a = Trainer(LayeredStandIn(n_layer=2), **kw)
    for b in batches[:3]:
        a.step(b)
    assert a.micro_step == 1
    ck = a.state_dict()
    assert ck['micro_step'] == 1 and ck['accumulate'] == 2 and ck['decoupled_weight_decay'] is True
    assert torch.equal(ck['accumulated_grad'], a.accumulated_grad()) and float(ck['accumulated_grad'].abs().max()) > 0
    assert ck['param_groups']['group_of'] == _hand_table()
    torch.manual_seed(5)
    c = Trainer(LayeredStandIn(n_layer=2), **kw)
    c.load_state_dict(ck)
    assert c.micro_step == 1 and torch.equal(c.accumulated_grad(), a.accumulated_grad())
    for b in batches[3:]:
        a.step(b), c.step(b)
        assert torch.equal(c.fp.flat, a.fp.flat) and torch.equal(c.shadow, a.shadow)
        assert torch.equal(c.accumulated_grad(), a.accumulated_grad())
    assert not torch.equal(a.fp.flat, ck['shadow'])
    # a checkpoint taken on an update boundary carries no partial sum
    assert a.micro_step == 0 and 'accumulated_grad' not in a.state_dict()


def test_checkpoint_mismatches_raise_and_the_default_round_trip_is_unchanged():
    from pamnet_amd.train import Trainer
    b = _batch(0, 10)
    mk = lambda **kw: Trainer(Tiny(), lr=1e-2, native_optimizer=False, **kw)
    torch.manual_seed(1)
    base = mk(param_groups=[{'params': ['a.*'], 'lr_scale': 0.5}])
    base.step(b)
    ck = base.state_dict()
    mk(param_groups=[{'params': ['a.*'], 'lr_scale': 0.5}]).load_state_dict(ck)
    for other in (dict(), dict(param_groups=[{'params': ['b.*'], 'lr_scale': 0.5}]),            # another group map
                  dict(param_groups=[{'params': ['a.*'], 'lr_scale': 0.25}]),                   # same map, other values
                  dict(param_groups=[{'params': ['a.*'], 'lr_scale': 0.5}], decoupled_weight_decay=True),
                  dict(param_groups=[{'params': ['a.*'], 'lr_scale': 0.5}], accumulate=2)):
        with pytest.raises(ValueError):
            mk(**other).load_state_dict(ck)
    # the default recipe: a round trip is exact, with and without the new keys (a checkpoint from before they existed)
    torch.manual_seed(2)
    a = mk()
    for _ in range(3):
        a.step(b)
    ck = a.state_dict()
    old = {k: v for k, v in ck.items() if k in ('model', 'shadow', 'lr', 'optimizer')}
    for sd in (ck, old):
        torch.manual_seed(5)
        c = mk()
        c.load_state_dict(copy.deepcopy(sd))          # (torch's load keeps the checkpoint's own step tensor: one copy each)
        assert torch.equal(c.fp.flat, a.fp.flat) and torch.equal(c.shadow, a.shadow)
        a2 = mk()
        a2.load_state_dict(copy.deepcopy(ck))
        a2.step(b), c.step(b)
        assert torch.equal(c.fp.flat, a2.fp.flat) and torch.equal(c.shadow, a2.shadow)
    for other in (dict(param_groups=[{'params': ['a.*'], 'frozen': True}]), dict(decoupled_weight_decay=True),
                  dict(accumulate=3)):
        with pytest.raises(ValueError):
            mk(**other).load_state_dict(old)


# --------------------------------------------------------------------------------------------------------------- C ABI
OK, EINVAL, ENULL = 0, -1, -2
BASE = 1 << 30                                # a made-up, 256-byte aligned device address: never dereferenced
NEW_SYMBOLS = ('pamnet_adam_ema_groups_f32', 'pamnet_sumsq_partials_masked_f32', 'pamnet_grad_accumulate_f32',
               'pamnet_chunk_groups_check')


@pytest.fixture(scope='module')
def h():
    from pamnet_amd import build, lib
    build.build()
    return lib.load()


def test_new_symbols_are_declared_and_exported(h):
    from pamnet_amd import lib
    decl = lib.declared_functions()
    for name in NEW_SYMBOLS:
        assert name in decl and hasattr(h, name), name
    assert len(decl['pamnet_adam_ema_groups_f32']) == 23
    assert h.pamnet_abi_version() >= 17
    # the two entry points of the default path keep their signatures
    assert len(decl['pamnet_adam_ema_norm_f32']) == 18 and len(decl['pamnet_adam_ema_f32']) == 17
    assert len(decl['pamnet_sumsq_partials_f32']) == 4


def test_chunk_groups_check(h):
    f = h.pamnet_chunk_groups_check
    arr = (ctypes.c_uint8 * 8)(0, 1, 1, 2, 2, 2, 0, 3)
    a = ctypes.addressof(arr)
    assert f(a, 8, 4) == OK and f(a, 8, 16) == OK
    assert f(a, 8, 3) == EINVAL                                  # a group id >= the number of groups
    assert f(a, 7, 3) == OK                                      # (the offender is the last chunk)
    assert f(a, 8, 0) == EINVAL and f(a, 8, 17) == EINVAL and f(a, -1, 4) == EINVAL
    assert f(None, 8, 4) == ENULL and f(None, 0, 4) == OK


def _tables(n=3, scale=None, wd=None, frozen=None):
    sc = (ctypes.c_float * n)(*(scale or [1.0] * n))
    w = (ctypes.c_float * n)(*(wd or [0.0] * n))
    fr = (ctypes.c_int32 * n)(*(frozen or [0] * n))
    return sc, w, fr


def _update_args(n=1024, n_groups=3, tables=None, step=1, ptrs=None):
    sc, w, fr = tables or _tables(max(n_groups, 1))
    p = {'p': BASE, 'g': BASE + (1 << 20), 'm': BASE + (2 << 20), 'v': BASE + (3 << 20), 'shadow': BASE + (4 << 20),
         'map': BASE + (5 << 20), 'scale': ctypes.addressof(sc), 'wd': ctypes.addressof(w), 'frozen': ctypes.addressof(fr),
         'part': BASE + (6 << 20), 'norm': BASE + (7 << 20)}
    p.update(ptrs or {})
    args = [p['p'], p['g'], p['m'], p['v'], p['shadow'], n, p['map'], n_groups, p['scale'], p['wd'], p['frozen'], 1e-3, 0.9,
            0.999, 1e-8, 0, step, 0.999, p['part'], p['norm'], 1000.0, 1, None]
    return args, (sc, w, fr)


def test_grouped_update_refusals(h):
    f = h.pamnet_adam_ema_groups_f32
    call = lambda **kw: f(*_update_args(**kw)[0])
    for n in (-64, 1000, 1024 + 4, 63):                          # the chunked forms want whole 64-float chunks
        assert call(n=n) == EINVAL, n
    assert call(step=0) == EINVAL
    assert call(n_groups=0) == EINVAL and call(n_groups=17) == EINVAL and call(n_groups=-1) == EINVAL
    assert call(tables=_tables(scale=[1.0, -0.5, 1.0])) == EINVAL
    assert call(tables=_tables(wd=[0.0, 0.0, -1e-2])) == EINVAL
    assert call(tables=_tables(scale=[1.0, float('nan'), 1.0])) == EINVAL
    for k in ('scale', 'wd', 'frozen', 'p', 'g', 'm', 'v', 'map', 'part'):
        assert call(ptrs={k: None}) == ENULL, k
    assert call(n=0) == OK                                        # nothing to do
    assert call(n=0, n_groups=16, tables=_tables(16)) == OK


def test_masked_norm_and_accumulate_refusals(h):
    f = h.pamnet_sumsq_partials_masked_f32
    fr = (ctypes.c_int32 * 3)(0, 1, 0)
    a = ctypes.addressof(fr)
    good = [BASE, 1024, BASE + 4096, 3, a, BASE + 8192, None]
    for n in (-64, 100, 1028):
        assert f(*(good[:1] + [n] + good[2:])) == EINVAL, n
    for ng in (0, 17, -3):
        assert f(*(good[:3] + [ng] + good[4:])) == EINVAL, ng
    for k in (0, 2, 4, 5):                                       # g, the chunk map, the frozen flags, the partials
        bad = list(good)
        bad[k] = None
        assert f(*bad) == ENULL, k
    g = h.pamnet_grad_accumulate_f32
    assert g(BASE, BASE + 4096, 6, None) == EINVAL and g(BASE, BASE + 4096, -4, None) == EINVAL
    assert g(None, BASE, 64, None) == ENULL and g(BASE, None, 64, None) == ENULL
    assert g(BASE, BASE, 64, None) == EINVAL                     # the sum and the gradient must be two buffers
    assert g(BASE, BASE + 4096, 0, None) == OK
