"""The engines must compute with the parameters the model holds NOW.

The fastest paths keep host-side state derived from the parameters: the layer-stack plan (stack.StackPlan: the Parameter
objects of both stacks, raw-pointer tables of their data and of their gradients), the cached parameter walk of models.PAMNet,
the flat buffers of train.Trainer and of the PAMNET_FLAT_PARAMS=1 interface.  Every test here runs a model, EDITS it the way
fine-tuning, checkpoint loading and the reference's EMA (utils/ema.py) do, and runs it again.

Reference: `fresh_twin(model)` -- a newly constructed model of the same class and config that has never run, loaded with
`model.state_dict()` by plain copy.  The engines are deterministic, so the edited model's output and every parameter
gradient must equal the twin's BIT FOR BIT; every replacement draws fresh random values (every element differs from the one
it replaces), so a stale table cannot pass by luck.  Against "both wrong the same way", each model case is also held to the
fp64 oracle once, after its last edit, with test_hip_model's own bounds (TOL, _check_gradients): no tolerance is new here.
"""
import copy
import re

import pytest
import torch
import torch.nn as nn

from test_hip_model import _check_gradients, _ok

# case -> (class name, dataset, dim, n_layer, cutoff_l, cutoff_g, flow, batch maker, its arguments)
CASES = {
    'qm9_d128_l3': ('PAMNet', 'QM9', 128, 3, 5.0, 5.0, 'source_to_target', 'qm9_batch', (8, 0, 6), {}),
    'qm9_d32_l2': ('PAMNet', 'QM9', 32, 2, 5.0, 5.0, 'source_to_target', 'qm9_batch', (8, 0, 6), {}),
    'qm9s_d128_l2': ('PAMNet_s', 'QM9', 128, 2, 5.0, 5.0, 'source_to_target', 'qm9_batch', (8, 0, 6), {}),
    'pdbbind_d128_l2': ('PAMNet', 'PDBbind', 128, 2, 2.0, 6.0, 'source_to_target', 'pdbbind_batch', (3, 0, 2),
                        dict(n_pocket=60, n_ligand=12)),
    'rna_d16_l1': ('PAMNet', 'rna_x', 16, 1, 2.6, 20.0, 'target_to_source', 'rna_batch', (5, 0, 2), dict(n_nodes=150)),
    'qm9_d136_l1': ('PAMNet', 'QM9', 136, 1, 5.0, 5.0, 'source_to_target', 'qm9_batch', (8, 0, 6), {}),      # no engine
}
FULL = ('qm9_d128_l3', 'qm9_d32_l2')                     # every edit
SOME = ('qm9s_d128_l2', 'pdbbind_d128_l2', 'rna_d16_l1', 'qm9_d136_l1')      # edits a, d, f (the last one: the control)
_BATCHES = {}


def _config(case):
    import models
    cls, ds, dim, L, cl, cg, flow = CASES[case][:7]
    return getattr(models, cls), models.Config(dataset=ds, dim=dim, n_layer=L, cutoff_l=cl, cutoff_g=cg, flow=flow)


def _build(case, device=None, seed=3):
    cls, cfg = _config(case)
    torch.manual_seed(seed)
    model = cls(cfg)
    return model if device is None else model.to(device)


def _batch(case):
    from pamnet_amd import synth
    if case not in _BATCHES:
        maker, args, kw = CASES[case][7:]
        _BATCHES[case] = getattr(synth, maker)(*args, **kw)
    return _BATCHES[case]


def fresh_twin(model):
    """What the edited model must compute: a model of the same class and config, newly constructed, never run, holding
    `model.state_dict()` by plain (in place) copy."""
    config, ns, nr, ee = model._ctor
    twin = type(model)(config, ns, nr, ee, num_atom_types=model.num_atom_types)
    twin = twin.to(next(iter(model.state_dict().values())).device)
    twin.load_state_dict({k: v.detach().clone() for k, v in model.state_dict().items()}, strict=True)
    return twin


def _fresh_like(t):
    """Freshly drawn values on the scale of `t`: every element is t's times a factor from [0.5, 1.5) (never exactly 1 for a
    whole tensor; an element keeps its value with probability 2^-24)."""
    return (t.detach() * (0.5 + torch.rand_like(t))).clone()


def _run(model, data):
    """Forward + backward under autograd, then a forward under no_grad: (out, {name: grad or None}, out_no_grad)."""
    for p in model.parameters():
        p.grad = None
    out = model(data)
    torch.nn.functional.l1_loss(out, data.y).backward()
    grads = {n: None if p.grad is None else p.grad.detach().clone() for n, p in model.named_parameters()}
    with torch.no_grad():
        quiet = model(data).clone()
    return out.detach().clone(), grads, quiet


def _assert_same(got, want, what):
    out, grads, quiet = got
    w_out, w_grads, w_quiet = want
    assert torch.equal(out, w_out), (what, 'training forward', float((out - w_out).abs().max()))
    assert torch.equal(quiet, w_quiet), (what, 'no_grad forward', float((quiet - w_quiet).abs().max()))
    assert list(grads) == list(w_grads), (what, 'parameter names')
    for n, g in grads.items():
        w = w_grads[n]
        assert (g is None) == (w is None), (what, n, 'gradient present on one side only')
        assert g is None or torch.equal(g, w), (what, n, float((g - w).abs().max()))


def _assert_follows(model, data, what):
    _assert_same(_run(model, data), _run(fresh_twin(model), data), what)


# ------------------------------------------------------------------------------------------------------ the edits
# Each is a generator: it applies one edit, yields its label, and (edits b and c) goes on to the next tensor.
def _owners(model):
    return {id(p): (mod, leaf) for mod in model.modules() for leaf, p in mod._parameters.items() if p is not None}


def _six(model):
    """Six tensors of the two stacks: the first, middle and last entry of the plan's list (what the pointer tables were
    keyed by) and three that are none of these -- a bias, an mlp_sbf weight and lin_rbf_out.weight."""
    from pamnet_amd import stack
    flat = stack.stack_plan(model.global_layer, model.local_layer).flat
    picks = [flat[0], flat[len(flat) // 2], flat[-1], model.global_layer[-1].mlp_m[0][0].bias,
             model.local_layer[0].mlp_sbf[0][0].weight, model.local_layer[-1].lin_rbf_out.weight]
    assert len(set(id(p) for p in picks)) == 6 and all(any(p is q for q in flat) for p in picks)
    owners = _owners(model)
    return [owners[id(p)] for p in picks]


def _heads(model):
    """The layers whose head edit a replaces: one that is neither the first global nor the last local one; with one layer
    pair, both heads."""
    if model.n_layer == 1:
        return [('global_layer.0', model.global_layer[0]), ('local_layer.0', model.local_layer[0])]
    return [('global_layer.1', model.global_layer[1]), ('local_layer.0', model.local_layer[0])]


def edit_a(model, dev):
    for _, layer in _heads(model):
        layer.W_out = nn.Linear(model.dim, 1).to(dev)
    yield 'a: head module replaced'


def edit_b(model, dev):
    for mod, leaf in _six(model):
        setattr(mod, leaf, nn.Parameter(_fresh_like(mod._parameters[leaf])))
        yield 'b: Parameter assigned over %s.%s' % (type(mod).__name__, leaf)


def edit_c(model, dev):
    keep = []
    for mod, leaf in _six(model):
        p = mod._parameters[leaf]
        p.data = _fresh_like(p)                      # the old tensor has no owner left: its block goes back to the allocator
        keep.append(torch.full_like(p, float('nan')))    # ... and comes out again here: a stale pointer now reads NaN
        yield 'c: .data re-pointed on %s.%s' % (type(mod).__name__, leaf)


def _sd2(model, dev):
    return {k: _fresh_like(v).to(dev) for k, v in model.state_dict().items()}


def edit_d(model, dev):
    model.load_state_dict(_sd2(model, dev), strict=True, assign=True)
    yield 'd: load_state_dict(assign=True)'


def edit_e(model, dev):
    model.load_state_dict(_sd2(model, dev), strict=True)
    yield 'e: load_state_dict in place'


def _fresh_copy(layer):
    new = copy.deepcopy(layer)
    with torch.no_grad():
        for p in new.parameters():
            p.copy_(_fresh_like(p))
    return new


def edit_f(model, dev):
    k = model.n_layer - 1
    model.local_layer[k] = _fresh_copy(model.local_layer[0])
    model.global_layer[k] = _fresh_copy(model.global_layer[0])
    yield 'f: a whole layer replaced in each stack'


def edit_g(model, dev):
    model.cpu()
    model.to(dev)
    yield 'g: device round trip'


EDITS = {'a': edit_a, 'b': edit_b, 'c': edit_c, 'd': edit_d, 'e': edit_e, 'f': edit_f, 'g': edit_g}
EDIT_CASES = [(c, e) for c in FULL for e in 'abcdefg'] + [(c, e) for c in SOME for e in 'adf']


# ------------------------------------------------------------------------------------------------------ CPU (not gpu)
def _assert_plan_is_live(model, plan):
    from pamnet_amd import stack
    assert plan.L == len(model.global_layer) == len(model.local_layer)
    for k in range(plan.L):
        for listed, live in ((plan.gl[k], stack.global_params(model.global_layer[k])),
                             (plan.ll[k], stack.local_params(model.local_layer[k]))):
            assert len(listed) == len(live) and all(a is b for a, b in zip(listed, live)), k
    live = [p for l in model.global_layer for p in stack.global_params(l)] + \
           [p for l in model.local_layer for p in stack.local_params(l)]
    assert len(plan.flat) == len(live) and all(a is b for a, b in zip(plan.flat, live))
    assert all(a is b for a, b in zip(plan.gflat + plan.lflat, live))


@pytest.mark.parametrize('case', ['qm9_d128_l3', 'qm9s_d128_l2', 'rna_d16_l1'])
@pytest.mark.parametrize('edit', ['a', 'b', 'd', 'f'])
def test_stack_plan_lists_the_live_parameters(case, edit):
    """stack.stack_plan() after an edit that replaces Parameter OBJECTS lists exactly what the layers hold, slot by slot
    (`is`): the plan the engine reads its pointer tables from is not kept across such an edit."""
    from pamnet_amd import stack
    model = _build(case)
    _assert_plan_is_live(model, stack.stack_plan(model.global_layer, model.local_layer))
    for what in EDITS[edit](model, torch.device('cpu')):
        _assert_plan_is_live(model, stack.stack_plan(model.global_layer, model.local_layer))
    assert stack.stack_plan(model.global_layer, model.local_layer) is stack.stack_plan(model.global_layer, model.local_layer)


@pytest.mark.parametrize('edit', ['a', 'b', 'd', 'f'])
def test_the_forwards_live_tree_check_drops_the_plan(edit):
    """Inside a forward the engine takes its plan WITHOUT walking the stacks (checked=True): what makes that sound is the
    live-tree check the forward starts with (its dtype check), which drops the plan together with the cached walk."""
    from pamnet_amd import stack
    model = _build('qm9_d32_l2')
    model._check_dtype()
    old = stack.stack_plan(model.global_layer, model.local_layer, checked=True)
    for what in EDITS[edit](model, torch.device('cpu')):
        model._check_dtype()                              # (what forward() does first)
        plan = stack.stack_plan(model.global_layer, model.local_layer, checked=True)
        assert plan is not old, what
        _assert_plan_is_live(model, plan)
        old = plan
    model._check_dtype()
    assert stack.stack_plan(model.global_layer, model.local_layer, checked=True) is old      # no edit: the plan is kept


def test_pointer_tables_follow_every_tensor():
    """The raw-pointer tables are keyed by the address of every tensor, not by three of them: `p.data = t` on any one
    parameter, and a .grad dropped or replaced on any one parameter, are seen."""
    from pamnet_amd import stack
    model = _build('qm9_d32_l2')
    plan = stack.stack_plan(model.global_layer, model.local_layer)

    def table():
        g, l = plan.param_tables()
        return [int(v or 0) for v in list(g) + list(l)]
    assert table() == [p.data_ptr() for p in plan.flat]
    for i in (0, 1, len(plan.flat) // 2, len(plan.flat) - 2, len(plan.flat) - 1):
        plan.flat[i].data = _fresh_like(plan.flat[i])
        assert table() == [p.data_ptr() for p in plan.flat], i
    assert not plan.direct()                              # no gradients, no permission
    for p in plan.flat:
        p.grad, p._pamnet_direct = torch.zeros_like(p), True
    assert plan.direct()
    for i in (1, len(plan.flat) // 2 + 1, len(plan.flat) - 2):
        p = plan.flat[i]
        old, p.grad = p.grad, None
        assert not plan.direct(), i
        p.grad = old
        assert plan.direct()
        p.grad = torch.zeros_like(p)
        assert plan.direct()
        assert [int(v or 0) for v in list(plan._ggrad) + list(plan._lgrad)] == [q.grad.data_ptr() for q in plan.flat], i
        p.grad = torch.zeros(p.shape[::-1]).t() if p.dim() == 2 and p.size(0) > 1 and p.size(1) > 1 else None
        assert not plan.direct(), i                       # (not contiguous / gone)
        p.grad = old


@pytest.mark.parametrize('edit,name', [('a', 'global_layer.1.W_out.weight'), ('b', 'global_layer.0.mlp_x1.0.0.weight'),
                                       ('c', 'global_layer.0.mlp_x1.0.0.weight'), ('d', 'embeddings')])
def test_trainer_ownership_check_names_the_parameter(edit, name):
    """train.Trainer owns flat buffers the model's parameters are views of.  After an edit that takes a parameter out of
    them, the check every step makes raises and names the first such parameter (the model's own order)."""
    from pamnet_amd import train
    model = _build('qm9_d32_l2')
    tr = train.Trainer(model, lr=1e-3, ema_decay=None)
    model._check_dtype()
    tr._check_ownership()
    next(EDITS[edit](model, torch.device('cpu')))
    model._check_dtype()
    with pytest.raises(RuntimeError, match="parameter '%s'" % re.escape(name)):
        tr._check_ownership()


def test_trainer_ownership_check_covers_a_forward_that_skipped_the_engine():
    """The stack parameters are covered by the plan's pointer key, which the engine call of a forward refreshes.  A forward
    that did not go through the engine (a batch the narrow engine refuses) refreshes nothing: the check then refreshes the
    key itself, so `p.data = t` on a stack parameter is still seen."""
    from pamnet_amd import stack, train
    model = _build('qm9_d32_l2')
    tr = train.Trainer(model, lr=1e-3, ema_decay=None)
    model._check_dtype()
    plan = stack.stack_plan(model.global_layer, model.local_layer, checked=True)
    plan.param_tables()
    tr._before = (plan, plan.table_calls - 1)             # a forward whose engine call keyed the tables
    tr._check_ownership()
    p = model.local_layer[1].lin_rbf_out.weight
    p.data = _fresh_like(p)
    tr._before = (plan, plan.table_calls)                 # a forward that made no engine call
    with pytest.raises(RuntimeError, match=re.escape("parameter 'local_layer.1.lin_rbf_out.weight'")):
        tr._check_ownership()


# ------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs an MI355X'
    return torch.device('cuda:0')


@pytest.mark.gpu
@pytest.mark.parametrize('case,edit', EDIT_CASES)
def test_edited_model_equals_a_fresh_twin(dev, case, edit):
    """One full forward + backward, then the edit, then forward + backward under autograd and a forward under no_grad: output
    and every parameter gradient equal, bit for bit, those of a fresh twin holding the edited model's state_dict."""
    model = _build(case, dev)
    data = _batch(case).to(dev)
    _run(model, data)
    for what in EDITS[edit](model, dev):
        _assert_follows(model, data, what)


@pytest.mark.gpu
@pytest.mark.parametrize('case', list(CASES))
def test_edited_model_vs_oracle(dev, case):
    """Every edit of the case in sequence (the model runs between them), then the model as it stands against the fp64 oracle
    with the suite's own bounds: output within TOL (never tighter than the fp32 oracle's own error), every gradient by
    test_hip_model._check_gradients -- the twin and the model cannot be wrong the same way."""
    from oracle import pamnet_oracle as O
    cls, cfg = _config(case)
    model = _build(case, dev)
    b = _batch(case)
    data = b.to(dev)
    _run(model, data)
    for e in ('abcdefg' if case in FULL else 'adf'):
        for what in EDITS[e](model, dev):
            _run(model, data)
    out, _, quiet = _run(model, data)                      # (leaves every p.grad of the last backward in place)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    fwd = O.pamnet_s_forward if cls.__name__ == 'PAMNet_s' else O.pamnet_forward
    pos, ei = getattr(b, 'pos', None), getattr(b, 'edge_index', None)
    ref32 = fwd(sd, cfg, b.x, b.batch, pos, ei)
    p64 = O.as_params({k: v.double() for k, v in sd.items()})
    x64 = b.x if cfg.dataset == 'QM9' else b.x.double()
    inter = {}
    ref64 = fwd(p64, cfg, x64, b.batch, pos, ei, dtype=torch.float64, intermediates=inter)
    torch.nn.functional.l1_loss(ref64, b.y.double()).backward()
    scale = None
    if cfg.dataset == 'PDBbind':                           # (signed pooling: judged on the sum it cancels from, as the suite does)
        pin = inter['pool_in'].detach().abs()
        scale = max(float(pin[b.batch == g].sum()) for g in range(int(b.batch.max()) + 1))
    for o in (out, quiet):
        ok, info = _ok(o.cpu().numpy(), ref32.detach().numpy(), ref64.detach().numpy(), scale)
        assert ok, ('out', info)
    _check_gradients(model, p64, fwd, sd, cfg, b)


@pytest.mark.gpu
@pytest.mark.parametrize('case', FULL)
def test_edit_between_forward_and_backward_keeps_autograd_semantics(dev, case):
    """Edit a between a forward and ITS backward ("Editing a model after it has run"): the backward
    differentiates the forward that ran -- the gradient is that of the weights the forward used and lands on the Parameters
    the forward used, as with autograd's saved tensors.  The heads hung in meanwhile took no part: no gradient."""
    model = _build(case, dev)
    data = _batch(case).to(dev)
    want = _run(fresh_twin(model), data)[1]
    _run(model, data)
    for p in model.parameters():
        p.grad = None
    out = model(data)
    loss = torch.nn.functional.l1_loss(out, data.y)
    old = {name: layer.W_out for name, layer in _heads(model)}
    next(edit_a(model, dev))
    loss.backward()
    new = set('%s.W_out.%s' % (name, leaf) for name in old for leaf in ('weight', 'bias'))
    for n, p in model.named_parameters():
        if n in new:
            assert p.grad is None, n
        else:
            assert (p.grad is None) == (want[n] is None) and (p.grad is None or torch.equal(p.grad, want[n])), n
    for name, head in old.items():
        assert torch.equal(head.weight.grad, want[name + '.W_out.weight']), name
        assert torch.equal(head.bias.grad, want[name + '.W_out.bias']), name
    _assert_follows(model, data, 'the next forward uses the new heads')


@pytest.mark.gpu
@pytest.mark.parametrize('case', FULL)
def test_tensor_moved_between_forward_and_backward_is_refused(dev, case):
    """`p.data = t` on a stack parameter between a forward and its backward: the saved activations belong to the old
    weights, so the backward raises a RuntimeError before it launches anything instead of mixing the
    two; a new forward + backward then follows the edit."""
    model = _build(case, dev)
    data = _batch(case).to(dev)
    _run(model, data)
    loss = torch.nn.functional.l1_loss(model(data), data.y)
    p = model.local_layer[0].mlp_sbf[0][0].weight
    p.data = _fresh_like(p)
    with pytest.raises(RuntimeError, match='between this forward and its backward'):
        loss.backward()
    del loss
    _assert_follows(model, data, 'after the refused backward')


# ---- train.Trainer: the model's parameters are views of flat buffers the trainer owns, gradients are written in place
def _trainer(model):
    from pamnet_amd import train
    return train.Trainer(model, lr=1e-3, ema_decay=None, max_grad_norm=None)


@pytest.mark.gpu
@pytest.mark.parametrize('case', FULL)
def test_trainer_follows_an_in_place_load(dev, case):
    """Edit e under a Trainer: load_state_dict copies through the views, the next step trains the new weights -- loss and
    the whole flat buffer after the update equal, bit for bit, those of a trainer on a fresh twin."""
    model = _build(case, dev)
    data = _batch(case).to(dev)
    tr = _trainer(model)
    assert model._one_node()
    tr.forward_backward(data)
    next(edit_e(model, dev))
    tr2 = _trainer(fresh_twin(model))
    loss, loss2 = tr.step(data), tr2.step(data)
    assert torch.equal(loss, loss2) and tr.fp.names == tr2.fp.names
    assert torch.equal(tr.fp.flat, tr2.fp.flat)
    assert all(torch.equal(v, w) for v, w in zip(model.state_dict().values(), tr2.model.state_dict().values()))


@pytest.mark.gpu
@pytest.mark.parametrize('case', FULL)
@pytest.mark.parametrize('edit,name', [('a', 'global_layer.1.W_out.weight'), ('b', 'global_layer.0.mlp_x1.0.0.weight'),
                                       ('d', 'embeddings')])
def test_trainer_refuses_parameters_it_does_not_own(dev, case, edit, name):
    """After edits a, b and d the model's parameters are no longer the views the trainer owns: step() raises a RuntimeError
    naming the first of them instead of updating a buffer the model does not read; nothing is updated."""
    model = _build(case, dev)
    data = _batch(case).to(dev)
    tr = _trainer(model)
    tr.step(data)
    next(EDITS[edit](model, dev))
    flat = tr.fp.flat.clone()
    with pytest.raises(RuntimeError, match="parameter '%s'" % re.escape(name)):
        tr.step(data)
    assert torch.equal(tr.fp.flat, flat)
    # refused behind the forward, before the backward: nothing half done is left -- the flat gradient is zero and clean
    assert tr._grad_clean and float(tr.fp.grad.abs().max()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize('case', FULL)
def test_direct_gradient_tables_follow_every_grad(dev, case):
    """A single .grad set to None, or replaced, on a parameter that is not one of the three the tables were keyed by: direct()
    is False without it, and with the new one the table the kernels write through holds the new address."""
    from pamnet_amd import stack
    model = _build(case, dev)
    data = _batch(case).to(dev)
    tr = _trainer(model)
    tr.forward_backward(data)
    plan = stack.stack_plan(model.global_layer, model.local_layer)
    assert plan.direct()
    p = model.local_layer[0].lin_rbf_out.weight
    flat = plan.flat
    assert not any(p is q for q in (flat[0], flat[len(flat) // 2], flat[-1]))
    old, p.grad = p.grad, None
    assert not plan.direct() and not model._one_node()
    p.grad = torch.zeros_like(p)
    assert plan.direct()
    assert [int(v or 0) for v in list(plan._ggrad) + list(plan._lgrad)] == [q.grad.data_ptr() for q in flat]
    want = old.clone()
    tr.forward_backward(data)                             # the kernels write where the table says
    assert torch.equal(p.grad, want) and float(old.abs().max()) == 0.0


# ---- PAMNET_FLAT_PARAMS=1: ONE flat nn.Parameter for the caller's optimiser and EMA
class _DataSwapEMA(object):
    """Shadow weights swapped in and out by re-pointing `param.data`, the form the reference's utils/ema.py uses (assign:
    `param.data = shadow[name]`; resume: `param.data = original[name]`) -- not the in-place copy of pamnet_amd.train."""

    def __init__(self, model):
        self.shadow = {n: _fresh_like(p.data) for n, p in model.named_parameters() if p.requires_grad}
        self.original = {}

    def assign(self, model):
        for n, p in model.named_parameters():
            self.original[n] = p.data.clone()
            p.data = self.shadow[n]

    def resume(self, model):
        for n, p in model.named_parameters():
            p.data = self.original[n]


def _flat_model(monkeypatch, dev):
    import models
    monkeypatch.setenv('PAMNET_FLAT_PARAMS', '1')
    model = _build('qm9_d128_l3', dev)
    named = list(model.named_parameters())
    assert [n for n, _ in named] == [models.FLAT_NAME]
    return model, named[0][1], _batch('qm9_d128_l3').to(dev)


def _by_name(model, flat_values):
    fp = model._flat_view().fp
    return {n: flat_values[fp.offsets[n]:fp.offsets[n] + p.numel()].view_as(p).clone() for n, p in zip(fp.names, fp.params)}


@pytest.mark.gpu
def test_flat_view_ema_assign_evaluates_the_shadow(dev, monkeypatch):
    """After assign the forward runs on the shadow weights: it equals a fresh twin loaded with them (and state_dict() shows
    them); after resume it is the first forward again."""
    model, flat, data = _flat_model(monkeypatch, dev)
    _run(model, data)
    with torch.no_grad():
        before = model(data).clone()
    ema = _DataSwapEMA(model)
    shadow = _by_name(model, ema.shadow['flat_parameters'])
    ema.assign(model)
    with torch.no_grad():
        got = model(data).clone()
    assert all(torch.equal(v, shadow[k]) for k, v in model.state_dict().items())
    twin = fresh_twin(model)
    twin.load_state_dict(shadow, strict=True)
    with torch.no_grad():
        want = twin(data).clone()
    assert torch.equal(got, want) and not torch.equal(got, before)
    ema.resume(model)
    with torch.no_grad():
        assert torch.equal(model(data), before)


@pytest.mark.gpu
def test_flat_view_optimizer_updates_what_the_kernels_read_after_ema_resume(dev, monkeypatch):
    """assign, resume, then one optimizer.step(): the weights the kernels read are the weights the optimiser updated -- the
    next forward differs from the one before the step and equals a twin loaded from model.state_dict(), and the one
    Parameter still is the model's flat buffer."""
    model, flat, data = _flat_model(monkeypatch, dev)
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    ema = _DataSwapEMA(model)
    ema.assign(model)
    with torch.no_grad():
        model(data)
    ema.resume(model)
    opt.zero_grad()
    out = model(data)
    pre = out.detach().clone()
    torch.nn.functional.l1_loss(out, data.y).backward()
    assert list(model.parameters())[0] is flat and flat.grad is not None and float(flat.grad.abs().max()) > 0
    weights = flat.detach().clone()
    opt.step()
    assert not torch.equal(flat.detach(), weights)
    with torch.no_grad():
        post = model(data).clone()
    assert not torch.equal(post, pre)
    assert flat.data_ptr() == model._flat_view().fp.flat.data_ptr()
    with torch.no_grad():
        assert torch.equal(post, fresh_twin(model)(data))
    sd = model.state_dict()
    assert all(torch.equal(v, sd[k]) for k, v in _by_name(model, flat.detach()).items())
