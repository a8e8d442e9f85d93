"""Forces: d prediction / d atom positions through the MI355X path (graph.differentiable_geometry and the geometric
backward kernels pamnet_rbf_ddist_f32, pamnet_sbf_bwd_f32, pamnet_pos_bwd_f32), against the CPU oracle, whose geometry
is plain differentiable torch (as the reference's is).

Parity protocol: err(a, b) = max|a-b| / max|b|, and
    err(hip, oracle_fp64) <= max(1e-5, 2 * err(oracle_fp32, oracle_fp64))
for the forward output, the forces (pos.grad; x.grad with all its columns for PDBbind / RNA) and every parameter gradient
of the same backward (PDBbind parameter gradients keep their 3e-5 bound, tests/test_hip_model.py).
"""
import math

import numpy as np
import pytest
import torch

from conftest import maxnorm_err

TOL = 1e-5
GRAD_TOL = 1e-5
PDBBIND_GRAD_TOL = 3e-5
CANCEL_TOL = 1e-4


def grad_tol(dataset):
    return PDBBIND_GRAD_TOL if str(dataset) == 'PDBbind' else GRAD_TOL


def _ok(a, ref32, ref64, scale=None):
    if scale is not None:
        e = float(np.max(np.abs(np.asarray(a, np.float64) - ref64))) / scale
        floor = float(np.max(np.abs(ref32.astype(np.float64) - ref64))) / scale
    else:
        e, floor = maxnorm_err(a, ref64), maxnorm_err(ref32, ref64)
    return e <= max(TOL, 2 * floor), (e, floor)


def _check_gradients(model, p64, fwd, sd, cfg, b, report=None, head_bias_terms=None, p32=None):
    """tests/test_hip_model.py's protocol, copied: every parameter gradient against the oracle's fp64 autograd,
        err(hip, fp64) <= max(GRAD_TOL, 2 * err(oracle_fp32, fp64))."""
    if p32 is None:
        p32 = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
        pos, ei = getattr(b, 'pos', None), getattr(b, 'edge_index', None)
        torch.nn.functional.l1_loss(fwd(p32, cfg, b.x, b.batch, pos, ei), b.y).backward()
    gn = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in model.parameters() if p.grad is not None)))
    gn64 = float(torch.sqrt(sum((p.grad ** 2).sum() for p in p64.values() if p.grad is not None)))
    gn32 = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in p32.values() if p.grad is not None)))
    assert abs(gn / gn64 - 1) <= max(GRAD_TOL, 2 * abs(gn32 / gn64 - 1)), (gn, gn64, gn32)
    worst = (0.0, 0.0, None)
    for k, p in model.named_parameters():
        if p64[k].grad is None:
            continue
        e = maxnorm_err(p.grad.cpu().numpy(), p64[k].grad.numpy())
        floor = maxnorm_err(p32[k].grad.numpy(), p64[k].grad.numpy())
        tol = grad_tol(cfg.dataset)
        if p.numel() == 1 and k.endswith('W_out.bias'):
            tol = CANCEL_TOL
            wk = k[:-4] + 'weight'
            scale = max(abs(float(p64[k].grad)), float(p64[wk].grad.abs().max()))
            if head_bias_terms is not None:
                scale = max(scale, 1e-3 * head_bias_terms)
            e = abs(float(p.grad) - float(p64[k].grad)) / scale
            floor = abs(float(p32[k].grad) - float(p64[k].grad)) / scale
        assert e <= max(tol, 2 * floor), (k, e, floor)
        if e > worst[0]:
            worst = (e, floor, k)
    if report is not None:
        report['grad_worst'] = worst
        report['grad_norm_rel'] = abs(gn / gn64 - 1)
    return worst


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs an MI355X'
    return torch.device('cuda:0')


def _qm9(dim, n_layer):
    import models
    return models.Config(dataset='QM9', dim=dim, n_layer=n_layer, cutoff_l=5.0, cutoff_g=5.0)


def _case(name):
    """(cfg, small, batch) of one force parity case."""
    import models
    from pamnet_amd import synth
    if name == 'rna_d16_l1':
        cfg = models.Config(dataset='rna_native', dim=16, n_layer=1, cutoff_l=2.6, cutoff_g=20.0, flow='target_to_source')
        return cfg, False, synth.rna_batch(2, 0, 2)
    if name == 'pdbbind_d128_l1':
        cfg = models.Config(dataset='PDBbind', dim=128, n_layer=1, cutoff_l=2.0, cutoff_g=6.0)
        return cfg, False, synth.pdbbind_batch(9, 0, 2, n_pocket=90, n_ligand=16)
    small = name.startswith('qm9s')
    dim, n_layer = (int(v) for v in name.split('_d')[1].split('_l'))
    return _qm9(dim, n_layer), small, synth.qm9_batch(0, 0, 16)


def _leaf_of(cfg, data):
    """The tensor forces are taken with respect to: QM9 pos; PDBbind / RNA x (positions are x[:, :3])."""
    return data.pos if cfg.dataset == 'QM9' else data.x


def _oracle_forces(fwd, sd, cfg, b, dtype, intermediates=None):
    """(output, d output.sum() / d leaf, parameters with .grad) of the oracle in `dtype`."""
    from oracle import pamnet_oracle as O
    p = O.as_params({k: v.detach().to(dtype) for k, v in sd.items()})
    if cfg.dataset == 'QM9':
        leaf = b.pos.to(dtype).clone().requires_grad_(True)
        out = fwd(p, cfg, b.x, b.batch, leaf, b.edge_index, dtype=dtype, intermediates=intermediates)
    else:
        leaf = b.x.to(dtype).clone().requires_grad_(True)
        out = fwd(p, cfg, leaf, b.batch, None, None, dtype=dtype, intermediates=intermediates)
    out.sum().backward()
    return out.detach(), leaf.grad, p


def _model(cfg, small, sd, dev):
    import models
    model = (models.PAMNet_s if small else models.PAMNet)(cfg)
    model.load_state_dict(sd, strict=True)
    return model.to(dev)


def _forces(model, cfg, data, how='backward'):
    leaf = _leaf_of(cfg, data)
    leaf.requires_grad_(True)
    leaf.grad = None
    out = model(data)
    if how == 'backward':
        out.sum().backward()
        return out.detach(), leaf.grad.detach().clone()
    return out.detach(), torch.autograd.grad(out.sum(), leaf)[0]


# ------------------------------------------------------------------------------------------------------------ 1. oracle
@pytest.mark.gpu
@pytest.mark.parametrize('case', ['qm9_d128_l2', 'qm9_d128_l6', 'qm9s_d128_l2', 'qm9_d64_l2', 'qm9_d160_l2',
                                  'rna_d16_l1', 'pdbbind_d128_l1'])
def test_forces_vs_oracle(dev, case):
    """Forces, forward output and every parameter gradient of E.sum().backward() with positions that require grad, at
    the d = 128 engine, PAMNet_s, a narrow width (64), a width above 128 on csrc/dense.hip (160), RNA (d = 16) and
    PDBbind (x.grad: position and feature columns)."""
    from oracle import pamnet_oracle as O
    cfg, small, b = _case(case)
    sd = O.init_state_dict(cfg, seed=7, small=small)
    fwd = O.pamnet_s_forward if small else O.pamnet_forward
    model = _model(cfg, small, sd, dev)
    data = b.to(dev)
    out, F = _forces(model, cfg, data)
    assert torch.isfinite(F).all()
    inter = {}
    ref32, F32, p32 = _oracle_forces(fwd, sd, cfg, b, torch.float32)
    ref64, F64, p64 = _oracle_forces(fwd, sd, cfg, b, torch.float64, intermediates=inter)
    assert torch.isfinite(F32).all() and torch.isfinite(F64).all()
    scale = None
    if cfg.dataset == 'PDBbind':
        pin = inter['pool_in'].detach().abs()
        scale = max(float(pin[b.batch == g].sum()) for g in range(int(b.batch.max()) + 1))
    ok, info = _ok(out.cpu().numpy(), ref32.numpy(), ref64.numpy(), scale)
    print(case, 'out err / floor', info)
    assert ok, ('out', info)
    ok, info = _ok(F.cpu().numpy(), F32.numpy(), F64.numpy())
    print(case, 'force err / floor', info)
    assert ok, ('forces', info)
    worst = _check_gradients(model, p64, fwd, sd, cfg, b, p32=p32)
    print(case, 'parameter gradient worst', worst)


# ------------------------------------------------------------------------------------ 2. autograd.grad, direct gradients
@pytest.mark.gpu
def test_autograd_grad_gives_the_same_forces_and_leaves_parameter_grads(dev):
    """torch.autograd.grad(E.sum(), pos) gives the forces of E.sum().backward() and writes no parameter .grad."""
    from oracle import pamnet_oracle as O
    from pamnet_amd import synth
    cfg = _qm9(128, 2)
    model = _model(cfg, False, O.init_state_dict(cfg, seed=3), dev)
    data = synth.qm9_batch(0, 0, 16).to(dev)
    _, F_bwd = _forces(model, cfg, data)
    snap = [None if p.grad is None else p.grad.clone() for p in model.parameters()]   # (init_linear: unused by QM9)
    assert sum(s is not None for s in snap) > 100
    _, F_grad = _forces(model, cfg, data, how='grad')
    assert torch.equal(F_grad, F_bwd)
    for p, s in zip(model.parameters(), snap):
        assert (p.grad is None) if s is None else torch.equal(p.grad, s)


@pytest.mark.gpu
@pytest.mark.parametrize('dim', [128, 32])
def test_forces_on_a_trainer_bound_model_write_no_gradient_buffer(dev, dim):
    """A model bound to a Trainer (gradient buffers with _pamnet_direct: the kernels may write p.grad in place): after one
    Trainer.step, torch.autograd.grad(E.sum(), pos) leaves every gradient bit-identical to a snapshot, and its forces
    equal those of a plain model holding the same weights."""
    from oracle import pamnet_oracle as O
    from pamnet_amd import synth
    from pamnet_amd.train import Trainer
    cfg = _qm9(dim, 2)
    model = _model(cfg, False, O.init_state_dict(cfg, seed=5), dev)
    trainer = Trainer(model, lr=1e-4)
    data = synth.qm9_batch(0, 0, 16).to(dev)
    trainer.step(data)
    trainer.forward_backward(data)                       # gradients that are not zero, left in the buffers
    torch.cuda.synchronize()
    snap_flat = trainer.fp.grad.clone()
    snap = [p.grad.clone() for p in model.parameters()]
    assert float(snap_flat.abs().max()) > 0
    fdata = synth.qm9_batch(0, 0, 16).to(dev)
    _, F = _forces(model, cfg, fdata, how='grad')
    torch.cuda.synchronize()
    assert torch.equal(trainer.fp.grad, snap_flat)
    for p, s in zip(model.parameters(), snap):
        assert torch.equal(p.grad, s)
    plain = _model(cfg, False, {k: v.detach().cpu() for k, v in model.state_dict().items()}, dev)
    _, F_plain = _forces(plain, cfg, synth.qm9_batch(0, 0, 16).to(dev))
    assert torch.equal(F, F_plain)


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['qm9_d128_l2', 'qm9_d16_l2', 'qm9_d160_l2', 'pdbbind_d128_l1'])
def test_a_retained_graph_can_be_differentiated_again(dev, case):
    """Forces with retain_graph=True, then backward passes through the same graph (forces and an energy loss from one
    forward): every pass gives the forces of a single pass, bitwise, and the first full backward its parameter gradients."""
    from oracle import pamnet_oracle as O
    cfg, small, b = _case(case)
    model = _model(cfg, small, O.init_state_dict(cfg, seed=9, small=small), dev)
    model.zero_grad(set_to_none=True)
    _, F_ref = _forces(model, cfg, b.to(dev))
    g_ref = [None if p.grad is None else p.grad.clone() for p in model.parameters()]
    model.zero_grad(set_to_none=True)
    data = b.to(dev)
    leaf = _leaf_of(cfg, data)
    leaf.requires_grad_(True)
    out = model(data)
    F1, = torch.autograd.grad(out.sum(), leaf, retain_graph=True)
    out.sum().backward(retain_graph=True)
    F2 = leaf.grad.clone()
    for p, r in zip(model.parameters(), g_ref):
        assert (p.grad is None) if r is None else torch.equal(p.grad, r)
    out.sum().backward()
    assert torch.equal(F1, F_ref)
    assert torch.equal(F2, F_ref)
    assert torch.equal(leaf.grad, F_ref + F_ref)                # (accumulated: the second pass gave F_ref again)


@pytest.mark.gpu
def test_positions_changed_in_place_before_the_backward_raise(dev):
    """As with the reference: the positions are saved for the backward, so changing them in place in between is caught."""
    from oracle import pamnet_oracle as O
    from pamnet_amd import synth
    cfg = _qm9(128, 2)
    model = _model(cfg, False, O.init_state_dict(cfg, seed=3), dev)
    data = synth.qm9_batch(0, 0, 4).to(dev)
    data.pos.requires_grad_(True)
    out = model(data)
    with torch.no_grad():
        data.pos.add_(0.01)
    with pytest.raises(RuntimeError, match='modified by an inplace operation'):
        out.sum().backward()


@pytest.mark.gpu
@pytest.mark.parametrize('dim', [128, 16])
def test_inspection_hooks_hold_no_autograd_graph_after_a_forces_forward(dev, dim):
    """model._graph_cache / _x_layers (kept until the next forward) refer to plain tensors: an E that is dropped without a
    backward frees its autograd graph."""
    from oracle import pamnet_oracle as O
    from pamnet_amd import synth
    cfg = _qm9(dim, 2)
    model = _model(cfg, False, O.init_state_dict(cfg, seed=3), dev)
    data = synth.qm9_batch(0, 0, 4).to(dev)
    data.pos.requires_grad_(True)
    out = model(data)
    assert out.grad_fn is not None
    gc = model._graph_cache
    for name in ('dist_g', 'dist_l', 'tp_angle', 'sbf'):
        assert not getattr(gc, name).requires_grad, name
    assert not any(x.requires_grad for x in model._x_layers)


# ------------------------------------------------------------------------------------ 3. prepare, reproducibility
@pytest.mark.gpu
@pytest.mark.parametrize('case', ['qm9_d128_l2', 'qm9_d16_l2', 'rna_d16_l1', 'pdbbind_d128_l1'])
def test_prepared_graph_and_repeated_runs_give_bitwise_equal_forces(dev, case):
    from oracle import pamnet_oracle as O
    cfg, small, b = _case(case)
    model = _model(cfg, small, O.init_state_dict(cfg, seed=9, small=small), dev)
    _, F1 = _forces(model, cfg, b.to(dev))
    _, F2 = _forces(model, cfg, b.to(dev))
    data = b.to(dev)
    _leaf_of(cfg, data).requires_grad_(True)
    model.prepare(data)
    out = model(data)
    out.sum().backward()
    F3 = _leaf_of(cfg, data).grad
    assert torch.isfinite(F1).all()
    assert torch.equal(F1, F2)
    assert torch.equal(F1, F3)


# ------------------------------------------------------------------------------------ 4. limits
@pytest.mark.gpu
def test_second_derivatives_raise(dev):
    from oracle import pamnet_oracle as O
    from pamnet_amd import synth
    cfg = _qm9(128, 2)
    model = _model(cfg, False, O.init_state_dict(cfg, seed=3), dev)
    data = synth.qm9_batch(0, 0, 4).to(dev)
    data.pos.requires_grad_(True)
    out = model(data)
    with pytest.raises(RuntimeError, match='second derivatives'):
        torch.autograd.grad(out.sum(), data.pos, create_graph=True)


@pytest.mark.gpu
def test_non_default_basis_with_position_gradients_raises(dev):
    import models
    from pamnet_amd import synth
    model = models.PAMNet(_qm9(32, 2), 5, 4, 6).to(dev)
    data = synth.qm9_batch(0, 0, 4).to(dev)
    data.pos.requires_grad_(True)
    with pytest.raises(NotImplementedError, match='default basis'):
        model(data)
    with torch.no_grad():                                 # (inference does not differentiate: it runs)
        assert torch.isfinite(model(data)).all()


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['qm9_d128_l2', 'qm9_d64_l2', 'pdbbind_d128_l1'])
def test_no_grad_forward_ignores_requires_grad(dev, case):
    from oracle import pamnet_oracle as O
    cfg, small, b = _case(case)
    model = _model(cfg, small, O.init_state_dict(cfg, seed=9, small=small), dev)
    with torch.no_grad():
        plain = model(b.to(dev))
        data = b.to(dev)
        _leaf_of(cfg, data).requires_grad_(True)
        marked = model(data)
    assert torch.equal(plain, marked)


# ------------------------------------------------------------------------------------ 5. properties at the headline batch
def _net_force_ratio(F, batch):
    """max over molecules of |sum_i F_i| / sum_i |F_i|."""
    F, batch = F.double().cpu(), batch.cpu()
    worst = 0.0
    for g in range(int(batch.max()) + 1):
        f = F[batch == g]
        worst = max(worst, float(f.sum(0).norm()) / max(float(f.norm(dim=1).sum()), 1e-300))
    return worst


def _rotation():
    a, b, c = 0.7, -1.1, 2.3
    rz = torch.tensor([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]], dtype=torch.float64)
    ry = torch.tensor([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]], dtype=torch.float64)
    rx = torch.tensor([[1, 0, 0], [0, math.cos(c), -math.sin(c)], [0, math.sin(c), math.cos(c)]], dtype=torch.float64)
    return rz @ ry @ rx


def _rotated(b, R):
    from pamnet_amd.synth import Batch
    kw = dict(b.__dict__)
    kw['pos'] = (b.pos.double() @ R.t()).float()
    return Batch(**kw)


def _closest_to_cutoff(b, cutoff):
    pos, batch = b.pos.double(), b.batch
    gap = float('inf')
    for g in range(int(batch.max()) + 1):
        p = pos[batch == g]
        d = torch.cdist(p, p)
        off = ~torch.eye(p.size(0), dtype=torch.bool)
        gap = min(gap, float((d[off] - cutoff).abs().min()) if off.any() else float('inf'))
    return gap


@pytest.mark.gpu
def test_force_properties_at_the_headline_batch(dev):
    """QM9 B = 128, d = 128, L = 6 (the oracle is too slow for forces there): per molecule the net force vanishes, and the
    forces rotate with the molecule.  Bounds: max(1e-6, 2x) and max(1e-5, 2x) of the fp32 oracle's own value on the first
    16 molecules, same weights."""
    from oracle import pamnet_oracle as O
    from pamnet_amd import synth
    cfg = _qm9(128, 6)
    sd = O.init_state_dict(cfg, seed=0)
    model = _model(cfg, False, sd, dev)
    b = synth.qm9_batch(0, 0, 128)
    # precondition: no pair of atoms of a molecule within 1e-5 of the cutoff, so a rotation cannot change the graph
    assert _closest_to_cutoff(b, cfg.cutoff_g) > 1e-5
    R = _rotation()
    _, F = _forces(model, cfg, b.to(dev))
    _, FR = _forces(model, cfg, _rotated(b, R).to(dev))
    assert torch.isfinite(F).all() and torch.isfinite(FR).all()
    net = _net_force_ratio(F, b.batch)
    rot = maxnorm_err(FR.double().cpu().numpy(), (F.double().cpu() @ R.t()).numpy())
    # the fp32 oracle's own values on the first 16 molecules
    b16 = synth.qm9_batch(0, 0, 16)
    _, F32, _ = _oracle_forces(O.pamnet_forward, sd, cfg, b16, torch.float32)
    _, F32R, _ = _oracle_forces(O.pamnet_forward, sd, cfg, _rotated(b16, R), torch.float32)
    net32 = _net_force_ratio(F32, b16.batch)
    rot32 = maxnorm_err(F32R.double().numpy(), (F32.double() @ R.t()).numpy())
    print('net force', net, 'oracle fp32', net32, '| rotation', rot, 'oracle fp32', rot32)
    assert net <= max(1e-6, 2 * net32), (net, net32)
    assert rot <= max(1e-5, 2 * rot32), (rot, rot32)


# ------------------------------------------------------------------------------------ 6. kernels vs fp64 torch
# Each entry point evaluates in fp64 and rounds its output once to fp32; the fp64 torch references below take the same
# fp32 inputs (the forward's own x = fp32(d * fp32(1/c)), the fp32 angle), so the expected difference is the final rounding
# (2^-24 of the largest value) plus fp64 noise: judged at 1e-6 of the largest reference value.
KTOL = 1e-6


def _graph(dev, count=6, seed=0):
    from pamnet_amd import graph as G
    from pamnet_amd import synth
    b = synth.qm9_batch(seed, 0, count).to(dev)
    g = G.build_graph('QM9', 5.0, 5.0, 'source_to_target', b.x, b.batch, b.pos, b.edge_index, num_graphs=count,
                      need_grad=True, n_types=5)
    return b, g


@pytest.mark.gpu
def test_rbf_ddist_kernel_vs_fp64_torch(dev):
    from oracle import pamnet_oracle as O
    from pamnet_amd import lib
    torch.manual_seed(0)
    cutoff = 5.0
    m = 3000
    dist = (torch.rand(m, device=dev) * 6.0 + 0.3)          # ~1/6 of them beyond the cutoff
    dist[:7] = torch.tensor([5.0, 5.0001, 7.0, 4.9999, 0.3, 1.0, 2.5], device=dev)
    freq = (torch.arange(1, 17, dtype=torch.float32) * math.pi + torch.randn(16) * 0.01).to(dev)
    g = torch.randn(m, 16, device=dev)
    dd = torch.empty(m, device=dev)
    lib.call('pamnet_rbf_ddist_f32', lib.ptr(dist), lib.ptr(freq), cutoff, m, lib.ptr(g), lib.ptr(dd), lib.stream_of(dist))
    torch.cuda.synchronize()
    x = (dist.cpu() * torch.tensor(1.0 / cutoff, dtype=torch.float32)).double().requires_grad_(True)
    ref = (O.bessel_rbf(x, freq.cpu().double(), 1.0) * g.cpu().double()).sum()
    gx, = torch.autograd.grad(ref, x)
    ref_dd = gx / cutoff
    got = dd.cpu().double()
    assert torch.isfinite(got).all()
    beyond = x.detach() >= 1.0
    assert beyond.any() and bool((got[beyond] == 0).all()) and bool((ref_dd[beyond] == 0).all())
    e = maxnorm_err(got.numpy(), ref_dd.numpy())
    print('rbf ddist err', e)
    assert e <= KTOL, e


@pytest.mark.gpu
def test_sbf_bwd_kernel_vs_fp64_torch(dev):
    from oracle import pamnet_oracle as O
    from pamnet_amd import lib
    b, g = _graph(dev)
    cutoff = 5.0
    dist = g.dist_l.clone()
    dist[::5] = dist[::5] + 4.0                              # some local edges beyond the cutoff
    angle = g.tp_angle
    e_l, tot = g.loc.m, g.tp.m
    torch.manual_seed(1)
    gs = torch.randn(tot, 42, device=dev)
    rad = torch.empty(e_l * 42, device=dev)
    dangle, ddist = torch.empty(tot, device=dev), torch.empty(e_l, device=dev)
    lib.call('pamnet_sbf_bwd_f32', lib.ptr(gs), lib.ptr(dist), cutoff, e_l, lib.ptr(g.tp.col), lib.ptr(angle), tot,
             lib.ptr(g.tp_T.ptr), lib.ptr(g.tp_T.perm), lib.ptr(rad), lib.ptr(dangle), lib.ptr(ddist), lib.stream_of(gs))
    torch.cuda.synchronize()
    x = (dist.cpu() * torch.tensor(1.0 / cutoff, dtype=torch.float32)).double().requires_grad_(True)
    a = angle.cpu().double().requires_grad_(True)
    sbf = O.spherical_basis(x, a, g.tp.col.long().cpu(), 1.0)
    gx, ga = torch.autograd.grad((sbf * gs.cpu().double()).sum(), (x, a))
    ref_dd = gx / cutoff
    assert torch.isfinite(ddist).all() and torch.isfinite(dangle).all()
    beyond = x.detach() >= 1.0
    assert beyond.any() and bool((ddist.cpu()[beyond] == 0).all())
    e_d = maxnorm_err(ddist.cpu().double().numpy(), ref_dd.numpy())
    e_a = maxnorm_err(dangle.cpu().double().numpy(), ga.numpy())
    print('sbf ddist err', e_d, 'dangle err', e_a)
    assert e_d <= KTOL and e_a <= KTOL, (e_d, e_a)


def _pos_bwd(g, pos, ddg, ddl, dang):
    from pamnet_amd import lib
    work = torch.empty(3 * g.loc.m, dtype=torch.float64, device=pos.device)
    dpos = torch.empty(g.n, 3, device=pos.device)
    lib.call('pamnet_pos_bwd_f32', lib.ptr(pos), g.n, lib.ptr(g.glob.ptr), lib.ptr(g.glob.row_of), lib.ptr(g.glob.col),
             lib.ptr(g.glob_T.ptr), lib.ptr(g.glob_T.perm), lib.ptr(ddg), g.glob.m, lib.ptr(g.loc.ptr), lib.ptr(g.loc.row_of),
             lib.ptr(g.loc.col), lib.ptr(g.loc_T.ptr), lib.ptr(g.loc_T.perm), lib.ptr(ddl), g.loc.m, lib.ptr(g.tp.ptr),
             lib.ptr(g.tp.row_of), lib.ptr(g.tp.col), lib.ptr(g.tp_kind), lib.ptr(g.tp_T.ptr), lib.ptr(g.tp_T.perm),
             lib.ptr(dang), g.tp.m, lib.ptr(work), lib.ptr(dpos), lib.stream_of(pos))
    torch.cuda.synchronize()
    return dpos.cpu()


def _torch_geometry(g, pos):
    """fp64 torch statement of graph construction's geometry (oracle: get_edge_info, angle_between)."""
    from oracle import pamnet_oracle as O
    gi, gc = g.glob.row_of.long().cpu(), g.glob.col.long().cpu()
    li, lj = g.loc.row_of.long().cpu(), g.loc.col.long().cpu()
    e, q, kind = g.tp.row_of.long().cpu(), g.tp.col.long().cpu(), g.tp_kind.cpu()
    dg = (pos[gi] - pos[gc]).pow(2).sum(-1).sqrt()
    u = pos[lj] - pos[li]
    dl = u.pow(2).sum(-1).sqrt()
    a = torch.where((kind == 0).unsqueeze(1), u[e], -u[e])
    ang = O.angle_between(a, u[q])
    return dg, dl, ang


@pytest.mark.gpu
def test_pos_bwd_kernel_vs_fp64_torch(dev):
    b, g = _graph(dev)
    pos = b.pos.float().contiguous()
    torch.manual_seed(2)
    ddg, ddl, dang = torch.randn(g.glob.m, device=dev), torch.randn(g.loc.m, device=dev), torch.randn(g.tp.m, device=dev)
    got = _pos_bwd(g, pos, ddg, ddl, dang)
    p64 = pos.cpu().double().requires_grad_(True)
    dg, dl, ang = _torch_geometry(g, p64)
    # the forward's values: the same graph, the same geometry
    assert maxnorm_err(g.tp_angle.cpu().numpy(), ang.detach().numpy()) < 1e-6
    ref, = torch.autograd.grad((dg * ddg.cpu().double()).sum() + (dl * ddl.cpu().double()).sum()
                               + (ang * dang.cpu().double()).sum(), p64)
    assert torch.isfinite(got).all() and torch.isfinite(ref).all()
    e = maxnorm_err(got.double().numpy(), ref.numpy())
    print('pos bwd err', e)
    assert e <= KTOL, e


@pytest.mark.gpu
def test_pos_bwd_collinear_pair_rows_contribute_exactly_zero(dev):
    """Pair rows whose two bonds are the same edge (b = -a, theta = pi, |a x b| = 0): no NaN / Inf, and exactly the zero
    contribution of torch's norm backward."""
    b, g = _graph(dev)
    pos = b.pos.float().contiguous()
    same = (g.tp.col == g.tp.row_of) & (g.tp_kind == 1)
    assert int(same.sum()) == g.loc.m                        # one such row per local edge
    dang = torch.where(same, torch.full_like(g.tp_angle, 3.0), torch.zeros_like(g.tp_angle))
    zg, zl = torch.zeros(g.glob.m, device=dev), torch.zeros(g.loc.m, device=dev)
    got = _pos_bwd(g, pos, zg, zl, dang)
    assert bool((got == 0).all())
    # torch's fp64 statement gives the same zero up to its own rounding: its cross product of b = -a is not exactly 0 (the
    # products are contracted), and what survives is ~1e-16 -- where a term of the wrong branch would be of the order of
    # |d angle| / |u| ~ 2 (bonds of ~1.5 A)
    p64 = pos.cpu().double().requires_grad_(True)
    _, _, ang = _torch_geometry(g, p64)
    ref, = torch.autograd.grad((ang * dang.cpu().double()).sum(), p64)
    assert torch.isfinite(ref).all()
    assert float(ref.abs().max()) < 1e-12, float(ref.abs().max())
