"""Parameter groups, frozen layers, AdamW and gradient accumulation on the MI355X (`-m gpu`): the grouped update / masked norm /
accumulate kernels (csrc/optim.hip, csrc/reduce.hip) against a float64 numpy restatement of torch's formulas, the Trainer's
native path against its torch path on the real model, the default path bit for bit, and the accumulated gradient of the engine
against the oracle's fp64 autograd."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import maxnorm_err

pytestmark = pytest.mark.gpu

RTOL = ATOL = 1e-6                 # "a few ulp": the bound of test_native_optimizer_kernel_matches_torch_adam


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs an MI355X'
    from pamnet_amd import lib
    lib.load()
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------------------ kernels
N_CHUNKS = 5000
# group of every 64-float chunk: a boundary right after the FIRST chunk and right before the LAST one (both group 2), a frozen
# run in the middle (group 1), a group of exactly one chunk (group 3) -- everything else the default group
SPANS = [(0, 1, 2), (1, 2000, 0), (2000, 3000, 1), (3000, 3001, 3), (3001, 4999, 0), (4999, 5000, 2)]
TABLE = {'lr_scale': [1.0, 1.0, 10.0, 0.5], 'weight_decay': [1e-3, 5e-2, 1e-2, 0.0], 'frozen': [0, 1, 0, 0]}


def _chunk_map():
    cmap = np.zeros(N_CHUNKS, np.uint8)
    for lo, hi, g in SPANS:
        cmap[lo:hi] = g
    return cmap


def _tables(t=TABLE):
    n = len(t['frozen'])
    return ((ctypes.c_float * n)(*t['lr_scale']), (ctypes.c_float * n)(*t['weight_decay']),
            (ctypes.c_int32 * n)(*t['frozen']))


def _numpy_update(p, g, m, v, s, grp, t, lr, b1, b2, eps, step, ema, max_norm, decoupled):
    """torch.optim.Adam / AdamW (single-tensor form, amsgrad=False) + clip_grad_norm_ over the trainable elements + the EMA of
    utils/ema.py, restated in float64 element by element."""
    p, g, m, v = (a.astype(np.float64) for a in (p, g, m, v))
    s = None if s is None else s.astype(np.float64)
    fz = np.asarray(t['frozen'], bool)[grp]
    lr_e = lr * np.asarray(t['lr_scale'], np.float64)[grp]
    wd_e = np.asarray(t['weight_decay'], np.float64)[grp]
    norm = np.sqrt(np.sum(g[~fz] ** 2))
    clip = min(max_norm / (norm + 1e-6), 1.0)
    gr = g * clip
    if decoupled:
        p1 = p * (1.0 - lr_e * wd_e)
    else:
        p1, gr = p, gr + wd_e * p
    m1 = b1 * m + (1 - b1) * gr
    v1 = b2 * v + (1 - b2) * gr * gr
    denom = np.sqrt(v1) / np.sqrt(1 - b2 ** step) + eps
    p1 = p1 - lr_e / (1 - b1 ** step) * (m1 / denom)
    out = [np.where(fz, a, b) for a, b in ((p, p1), (m, m1), (v, v1))]
    if s is not None:
        out.append(np.where(fz, s, ema * s + (1 - ema) * p1))
    return out, norm, clip


@pytest.mark.parametrize('max_norm', [5.0, 1e9], ids=['clip-binds', 'clip-idle'])
@pytest.mark.parametrize('ema', [True, False], ids=['ema', 'no-ema'])
@pytest.mark.parametrize('decoupled', [0, 1], ids=['l2', 'adamw'])
def test_grouped_update_and_masked_norm_against_float64(dev, decoupled, ema, max_norm):
    from pamnet_amd import lib, ops
    n = 64 * N_CHUNKS
    rng = np.random.default_rng(17 + decoupled)
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 0.3).astype(np.float32)
    m = (rng.standard_normal(n) * 0.1).astype(np.float32)
    v = (rng.random(n) * 0.05).astype(np.float32)
    s = rng.standard_normal(n).astype(np.float32) if ema else None
    cmap = _chunk_map()
    grp = np.repeat(cmap, 64)
    lr, b1, b2, eps, step, decay = 2e-3, 0.9, 0.999, 1e-8, 3, 0.999
    (want, norm64, clip) = _numpy_update(p, g, m, v, s, grp, TABLE, lr, b1, b2, eps, step, decay, max_norm, bool(decoupled))
    assert (clip < 1.0) == (max_norm == 5.0)
    P, G, M, V = (torch.from_numpy(a).to(dev) for a in (p, g, m, v))
    S = torch.from_numpy(s).to(dev) if ema else None
    cm = torch.from_numpy(cmap).to(dev)
    sc, wd, fr = _tables()
    lib.call('pamnet_chunk_groups_check', cmap.ctypes.data, N_CHUNKS, 4)
    part = ops.sumsq_partials_masked(G, cm, 4, fr)
    assert torch.equal(part, ops.sumsq_partials_masked(G, cm, 4, fr))             # fixed order: bitwise repeatable
    assert abs(float(part.sum().sqrt()) / norm64 - 1) <= RTOL
    full = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    assert norm64 < 0.95 * full                                                    # the frozen run is really outside the norm
    nrm = torch.zeros(1, device=dev)
    lib.call('pamnet_adam_ema_groups_f32', lib.ptr(P), lib.ptr(G), lib.ptr(M), lib.ptr(V), lib.ptr(S), n, lib.ptr(cm), 4,
             ctypes.addressof(sc), ctypes.addressof(wd), ctypes.addressof(fr), lr, b1, b2, eps, decoupled, step, decay,
             lib.ptr(part), lib.ptr(nrm), max_norm, 1, lib.stream_of(P))
    torch.cuda.synchronize()
    assert abs(float(nrm) / norm64 - 1) <= RTOL
    assert float(G.abs().max()) == 0.0                                             # zeroed everywhere, frozen chunks included
    fz = torch.from_numpy(np.asarray(TABLE['frozen'], bool)[grp])
    got = [P.cpu(), M.cpu(), V.cpu()] + ([S.cpu()] if ema else [])
    start = [p, m, v] + ([s] if ema else [])
    for name, a, w, a0 in zip(('p', 'm', 'v', 'shadow'), got, want, start):
        assert torch.equal(a[fz], torch.from_numpy(a0)[fz]), name                  # frozen: bitwise untouched
        live, ref = a[~fz].double(), torch.from_numpy(w)[~fz]
        assert torch.allclose(live, ref, rtol=RTOL, atol=ATOL), (name, float((live - ref).abs().max()))
        assert not torch.equal(a[~fz], torch.from_numpy(a0)[~fz]), name
    # every group boundary took ITS group's values: the chunks on both sides of each boundary, separately
    for lo, hi, gidx in SPANS:
        for c in (lo, hi - 1):
            sl = slice(64 * c, 64 * c + 64)
            if TABLE['frozen'][gidx]:
                assert torch.equal(got[0][sl], torch.from_numpy(p[sl])), c
            else:
                assert torch.allclose(got[0][sl].double(), torch.from_numpy(want[0][sl]), rtol=RTOL, atol=ATOL), c


def test_one_default_group_is_the_plain_update_bit_for_bit(dev):
    """With one group {1, wd, trainable} and L2 decay the grouped entry points give the bits of pamnet_sumsq_partials_f32 /
    pamnet_adam_ema_norm_f32 (include/pamnet_hip.h says so)."""
    from pamnet_amd import lib, ops
    n = 64 * 3001
    torch.manual_seed(5)
    base = [torch.randn(n, device=dev), torch.randn(n, device=dev) * 0.2, torch.randn(n, device=dev) * 0.1,
            torch.rand(n, device=dev) * 0.05, torch.randn(n, device=dev)]
    cm = torch.zeros(n // 64, dtype=torch.uint8, device=dev)
    sc, wd, fr = _tables({'lr_scale': [1.0], 'weight_decay': [1e-2], 'frozen': [0]})
    a, b = [t.clone() for t in base], [t.clone() for t in base]
    pa, pb = ops.sumsq_partials(a[1]), ops.sumsq_partials_masked(b[1], cm, 1, fr)
    assert torch.equal(pa, pb)
    na, nb = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    lib.call('pamnet_adam_ema_norm_f32', *[lib.ptr(t) for t in a], n, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 2, 0.999, lib.ptr(pa),
             lib.ptr(na), 1.0, 1, lib.stream_of(a[0]))
    lib.call('pamnet_adam_ema_groups_f32', *[lib.ptr(t) for t in b], n, lib.ptr(cm), 1, ctypes.addressof(sc),
             ctypes.addressof(wd), ctypes.addressof(fr), 1e-3, 0.9, 0.999, 1e-8, 0, 2, 0.999, lib.ptr(pb), lib.ptr(nb), 1.0, 1,
             lib.stream_of(b[0]))
    assert torch.equal(na, nb)
    for x, y, t0 in zip(a, b, base):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], base[0])


@pytest.mark.parametrize('n', [4, 1000, 64 * 4097, 3581100 // 4 * 4])
def test_grad_accumulate_kernel(dev, n):
    from pamnet_amd import lib
    torch.manual_seed(n)
    acc, g = torch.randn(n, device=dev), torch.randn(n, device=dev)
    want = acc + g                                         # one fp32 addition per element: exact to compare
    lib.call('pamnet_grad_accumulate_f32', lib.ptr(acc), lib.ptr(g), n, lib.stream_of(acc))
    assert torch.equal(acc, want) and float(g.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------ trainer
GROUPS = [
    {'params': ['embeddings', 'global_layer.0.*', 'local_layer.0.*'], 'frozen': True},
    {'params': ['*.bias', 'rbf_g.freq', 'rbf_l.freq'], 'weight_decay': 0.0},
    # (the interface's documented 10x; the steps below keep every group's rate inside what the bound was set for --
    #  test_native_optimizer_kernel_matches_torch_adam steps with up to 4e-3, here 1e-4 * (i + 1) * 10 <= 4e-3)
    {'params': ['*.W_out.*', '*.W'], 'lr_scale': 10.0, 'weight_decay': 1e-2},
]


def _hand_trainable_mask(fp):
    """Elements of the flat layout that GROUPS leaves trainable, from the names alone (the first group freezes the embeddings
    and layer pair 0; alignment padding belongs to nobody)."""
    mask = torch.zeros(fp.flat.numel(), dtype=torch.bool)
    for n, p in zip(fp.names, fp.params):
        if not (n == 'embeddings' or n.startswith(('global_layer.0.', 'local_layer.0.'))):
            mask[fp.offsets[n]:fp.offsets[n] + p.numel()] = True
    return mask.to(fp.flat.device)


@pytest.mark.parametrize('decoupled', [False, True], ids=['l2', 'adamw'])
@pytest.mark.parametrize('dim', [128, 32])
def test_native_grouped_update_matches_the_torch_path_on_the_model(dev, dim, decoupled):
    """Three groups, one frozen, 4 steps with clipping active and changing learning rates: the fused path (masked norm + one
    grouped launch) against torch.optim.Adam / AdamW with real param_groups over per-tensor views + clip_grad_norm_ over the
    trainable views + the EMA of the trainable slices (the pattern of test_native_optimizer_kernel_matches_torch_adam)."""
    import models
    from pamnet_amd import synth
    from pamnet_amd.train import Trainer
    cfg = models.Config(dataset='QM9', dim=dim, n_layer=2, cutoff_l=5.0, cutoff_g=5.0)
    batches = [synth.qm9_batch(4, 8 * i, 8).to(dev) for i in range(4)]
    res = []
    for native in (True, False):
        torch.manual_seed(11)
        model = models.PAMNet(cfg).to(dev)
        tr = Trainer(model, lr=1e-3, max_grad_norm=2.0, weight_decay=1e-3, native_optimizer=native, overlap_comm=False,
                     param_groups=GROUPS, decoupled_weight_decay=decoupled)
        assert tr.native_opt == native
        assert tr.group_of['embeddings'] == 1 and tr.group_of['global_layer.1.W_out.bias'] == 2
        assert tr.group_of['global_layer.1.W'] == 3 and tr.group_of['global_layer.1.W_out.weight'] == 3
        init = tr.fp.flat.clone()
        norms = []
        for i, b in enumerate(batches):
            tr.step(b, lr=1e-4 * (i + 1))
            norms.append(float(tr.last_grad_norm))
        if native:
            assert float(tr.fp.grad.abs().sum()) == 0.0
        m, v = tr.adam_moments()
        frozen = ~_hand_trainable_mask(tr.fp)
        assert int(frozen.sum()) > 0
        for t in (tr.fp.flat, tr.shadow):
            assert torch.equal(t[frozen], init[frozen])                        # bit for bit
        assert float(m[frozen].abs().max()) == 0.0 and float(v[frozen].abs().max()) == 0.0
        assert not torch.equal(tr.fp.flat[~frozen], init[~frozen])
        res.append((tr.fp.flat.clone(), tr.shadow.clone(), norms))
    (p1, s1, n1), (p0, s0, n0) = res
    assert max(n1) > 2.0                                                       # the clip was active
    assert np.allclose(n1, n0, rtol=1e-5)
    assert torch.allclose(p1, p0, rtol=RTOL, atol=ATOL), float((p1 - p0).abs().max())
    assert torch.allclose(s1, s0, rtol=RTOL, atol=ATOL), float((s1 - s0).abs().max())


def test_frozen_gradients_stay_out_of_the_reported_norm(dev):
    """last_grad_norm of a trainer with frozen layers = the norm over the trainable parameters of the same gradient."""
    import models
    from pamnet_amd import synth
    from pamnet_amd.train import Trainer
    cfg = models.Config(dataset='QM9', dim=128, n_layer=2, cutoff_l=5.0, cutoff_g=5.0)
    b = synth.qm9_batch(4, 0, 8).to(dev)
    torch.manual_seed(3)
    tr = Trainer(models.PAMNet(cfg).to(dev), lr=1e-3, param_groups=GROUPS[:1])
    tr.forward_backward(b)
    g = tr.fp.grad.double().cpu()
    mask = _hand_trainable_mask(tr.fp).cpu()
    want, everything = float(g[mask].norm()), float(g.norm())
    assert want < 0.999 * everything
    tr.last_grad_norm = tr.native_update(1e-3)
    assert abs(float(tr.last_grad_norm) / want - 1) <= 1e-6


def test_default_arguments_are_the_default_path_bit_for_bit(dev):
    import models
    from pamnet_amd import lib, synth
    from pamnet_amd.train import Trainer
    cfg = models.Config(dataset='QM9', dim=128, n_layer=2, cutoff_l=5.0, cutoff_g=5.0)
    batches = [synth.qm9_batch(6, 16 * i, 16).to(dev) for i in range(3)]
    res, calls = [], []
    real = lib.call
    for kw in (dict(), dict(param_groups=None, decoupled_weight_decay=False, accumulate=1)):
        torch.manual_seed(21)
        tr = Trainer(models.PAMNet(cfg).to(dev), lr=1e-3, max_grad_norm=2.0, weight_decay=1e-3, **kw)
        seen = []
        lib.call = lambda name, *a: (seen.append(name), real(name, *a))[1]
        try:
            for i, b in enumerate(batches):
                tr.step(b, lr=1e-3 * (i + 1))
        finally:
            lib.call = real
        torch.cuda.synchronize()
        res.append((tr.fp.flat.clone(), tr.shadow.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone(), tr.last_grad_norm.clone()))
        calls.append([n for n in seen if 'adam' in n or 'sumsq' in n or 'accumulate' in n])
    for x, y in zip(*res):
        assert torch.equal(x, y)
    assert calls[0] == calls[1] == ['pamnet_sumsq_partials_f32', 'pamnet_adam_ema_norm_f32'] * 3


# ------------------------------------------------------------------------------------- accumulation on the engine
GRAD_TOL = 1e-5          # gradients within 1e-5 of the reference's fp64 autograd ...
CANCEL_TOL = 1e-4        # ... the head bias (a scalar that is almost pure cancellation) on its weight gradient's scale


def _check_gradients(grads, p64, p32):
    """tests/test_hip_model.py's protocol restated for a dict of gradients: per tensor
        err(hip, fp64) <= max(GRAD_TOL, 2 * err(oracle_fp32, fp64)),   err(a, b) = max|a - b| / max|b|,
    and the same for the norm of the whole gradient."""
    gn = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())))
    gn64 = float(torch.sqrt(sum((p.grad ** 2).sum() for p in p64.values() if p.grad is not None)))
    gn32 = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in p32.values() if p.grad is not None)))
    assert abs(gn / gn64 - 1) <= max(GRAD_TOL, 2 * abs(gn32 / gn64 - 1)), (gn, gn64, gn32)
    worst = (0.0, 0.0, None)
    for k, g in grads.items():
        if p64[k].grad is None:
            continue
        e = maxnorm_err(g.cpu().numpy(), p64[k].grad.numpy())
        floor = maxnorm_err(p32[k].grad.numpy(), p64[k].grad.numpy())
        tol = GRAD_TOL
        if g.numel() == 1 and k.endswith('W_out.bias'):
            tol = CANCEL_TOL
            scale = max(abs(float(p64[k].grad)), float(p64[k[:-4] + 'weight'].grad.abs().max()))
            e = abs(float(g) - float(p64[k].grad)) / scale
            floor = abs(float(p32[k].grad) - float(p64[k].grad)) / scale
        print('%-40s err %.2e  fp32 oracle %.2e' % (k, e, floor))
        assert e <= max(tol, 2 * floor), (k, e, floor)
        if e > worst[0]:
            worst = (e, floor, k)
    return worst


def test_accumulated_gradient_of_four_micro_batches_vs_oracle(dev):
    """4 x 32 QM9 molecules: the sum of the four micro-gradients (each scaled by 32 / 128) against the oracle's fp64 gradient of
    the L1 loss of the 128-molecule batch.  The trainer is given five calls per cycle so that the whole sum can still be read
    after the fourth (an update would consume it)."""
    import os
    import models
    from oracle import pamnet_oracle as O
    from pamnet_amd import synth
    from pamnet_amd.train import Trainer
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    cfg = models.Config(dataset='QM9', dim=128, n_layer=2, cutoff_l=5.0, cutoff_g=5.0)
    sd = O.init_state_dict(cfg, seed=0)
    model = models.PAMNet(cfg)
    model.load_state_dict(sd, strict=True)
    tr = Trainer(model.to(dev), lr=1e-3, accumulate=5)
    for i in range(4):
        tr.step(synth.qm9_batch(0, 32 * i, 32).to(dev), global_graphs=128)
        assert tr.micro_step == i + 1
    acc = tr.accumulated_grad()
    mae = tr.evaluate([synth.qm9_batch(0, 0, 32).to(dev)])                  # mid-cycle: the partial sum survives
    assert mae > 0 and torch.equal(acc, tr.accumulated_grad()) and tr.micro_step == 4
    assert float(tr.fp.grad.abs().max()) == 0.0
    b = synth.qm9_batch(0, 0, 128)
    p64 = O.as_params({k: v.double() for k, v in sd.items()})
    torch.nn.functional.l1_loss(O.pamnet_forward(p64, cfg, b.x, b.batch, b.pos, b.edge_index, dtype=torch.float64),
                                b.y.double()).backward()
    p32 = O.as_params(sd)
    torch.nn.functional.l1_loss(O.pamnet_forward(p32, cfg, b.x, b.batch, b.pos, b.edge_index), b.y).backward()
    grads = {n: acc[tr.fp.offsets[n]:tr.fp.offsets[n] + p.numel()].view_as(p) for n, p in zip(tr.fp.names, tr.fp.params)}
    worst = _check_gradients(grads, p64, p32)
    print('accumulated 4 x 32 vs oracle fp64 on 128: worst %.2e (fp32 oracle %.2e, %s)' % worst)


def test_accumulated_step_is_bitwise_repeatable(dev):
    """Two runs of the same accumulated step (4 micro-batches, three groups, AdamW): parameters, shadow, moments and the
    reported norm are bitwise equal; updates happen on every fourth call only."""
    import models
    from pamnet_amd import synth
    from pamnet_amd.train import Trainer
    cfg = models.Config(dataset='QM9', dim=128, n_layer=2, cutoff_l=5.0, cutoff_g=5.0)
    batches = [synth.qm9_batch(8, 32 * i, 32).to(dev) for i in range(8)]
    runs = []
    for _ in range(2):
        torch.manual_seed(31)
        tr = Trainer(models.PAMNet(cfg).to(dev), lr=1e-3, max_grad_norm=2.0, weight_decay=1e-3, param_groups=GROUPS,
                     decoupled_weight_decay=True, accumulate=4)
        init = tr.fp.flat.clone()
        for i, b in enumerate(batches):
            before = tr.fp.flat.clone()
            tr.step(b, lr=1e-3)
            assert tr.micro_step == (i + 1) % 4
            assert torch.equal(before, tr.fp.flat) == ((i + 1) % 4 != 0)
            if i == 2:
                assert not hasattr(tr, 'last_grad_norm')
        assert float(tr.accumulated_grad().abs().max()) == 0.0 and float(tr.fp.grad.abs().max()) == 0.0
        assert tr.step_count == 2
        runs.append((tr.fp.flat.clone(), tr.shadow.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone(),
                     tr.last_grad_norm.clone()))
        assert not torch.equal(runs[-1][0], init)
    for x, y in zip(*runs):
        assert torch.equal(x, y)
