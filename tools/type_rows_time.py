"""Element tables indexed by atomic number (max_atomic_number): what the wide type-row gradient costs, for
profiles/type_rows_wide.txt.  Two measurements, each with three tables on the same rows:
  (a) the 5-row table of the QM9 schema (the 8-row kernels: the yardstick, taken twice -- "a" and "a again" -- so that the
      difference of two runs of the SAME code is on the page beside the differences that mean something)
  (b) a 95-row table, the same five elements at their atomic numbers 1, 6, 7, 8, 9 (one pass of the same loop)
  (c) a 95-row table, 40 distinct elements drawn uniformly (five passes per workgroup)
  1. the backward of the one-launch input stage (pamnet_embed_multi_bwd_f32: both launches) of the bench batch
     (synth.qm9_batch(0, 0, 128): 2 286 atoms, d = 128, cutoffs 5.0) -- fused._InputStage.backward as the training step calls
     it, gradient buffers allocated inside the call
  2. pamnet_type_rows_grad_f32 alone (both launches), d = 128, n = 2 286 and n = 100 000
Host clock around a device synchronise, the variants interleaved call by call in one process, --calls each after --warmup;
median / p5 / p95.  Run on the GPU box: python tools/type_rows_time.py"""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--calls', type=int, default=400)
ap.add_argument('--warmup', type=int, default=40)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'physics-aware-multiplex-gnn_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import models  # noqa: E402
from pamnet_amd import fused, lib, ops, synth  # noqa: E402

dev = torch.device('cuda:0')
lib.load()
FIVE = torch.tensor([1, 6, 7, 8, 9])


def timed(variants):
    times = [[] for _ in variants]
    for k in range(args.warmup + args.calls):
        for r, (name, fn) in enumerate(variants):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if k >= args.warmup:
                times[r].append(1e6 * (time.perf_counter() - t0))
    med = []
    for (name, _), t in zip(variants, times):
        t = np.asarray(t)
        med.append(float(np.median(t)))
        print('  %-44s median  %7.1f us   p5  %7.1f   p95  %7.1f   (n = %d)' % (name, med[-1], np.percentile(t, 5),
                                                                                np.percentile(t, 95), t.size))
    return med


def verdict(med):
    a, a2, b, c = med
    spread = abs(a - a2) / a
    print('  (a again) / (a) = %.3f: two runs of the same code differ by %.1f %%' % (a2 / a, 100 * spread))
    print('  (b) / (a) = %.3f  -- %s that spread' % (b / a, 'within' if abs(b - a) / a <= spread else 'OUTSIDE'))
    print('  (c) / (a) = %.3f' % (c / a))


def forty(n, gen):
    z = (torch.randperm(94, generator=gen)[:40] + 1).sort().values
    x = z[torch.randint(0, 40, (n,), generator=gen)]
    assert x.unique().numel() == 40 or n < 400
    return x


# ---- 1. the input stage's backward on the bench batch
cfg = models.Config(dataset='QM9', dim=128, n_layer=1, cutoff_l=5.0, cutoff_g=5.0)
batch = synth.qm9_batch(0, 0, 128)
gen = torch.Generator().manual_seed(0)
xs = {'a': batch.x, 'b': FIVE[batch.x.long()].to(batch.x.dtype), 'c': forty(batch.x.numel(), gen).to(batch.x.dtype)}


def stage_backward(wide, x):
    """The backward of the input stage of PAMNet._input_stage for this table, as a callable."""
    torch.manual_seed(0)
    model = (models.PAMNet(cfg, max_atomic_number=94) if wide else models.PAMNet(cfg)).to(dev)
    data = synth.Batch(**dict(batch.__dict__, x=x)).to(dev)
    g = model._graph(data)
    lin_l, lin_g, lin_a, lin_b = model.mlp_rbf_l[0][0], model.mlp_rbf_g[0][0], model.mlp_sbf2[0][0], model.mlp_sbf1[0][0]
    layers = [(None, g.dist_l, model.cutoff_l, None, True, True), (None, g.dist_g, model.cutoff_g, None, True, True),
              (g.sbf, None, None, g.tp_kind, True, True)]
    params = [model.rbf_l.freq, lin_l.weight, lin_l.bias, model.rbf_g.freq, lin_g.weight, lin_g.bias, lin_a.weight, lin_a.bias,
              lin_b.weight, lin_b.bias, model.embeddings]
    types = g.types if getattr(g, 'types', None) is not None else data.x.to(torch.int32).contiguous()
    ctx = ops._TapeCtx((False, False) + (True,) * len(params))
    outs = fused._InputStage.forward(ctx, fused.InputSpec(layers, types), params, *params)
    gouts = [torch.randn(o.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) for o in outs]
    sizes = (g.dist_l.numel(), g.dist_g.numel(), g.sbf.size(0), types.numel())
    return (lambda: fused._InputStage.backward(ctx, *gouts)), sizes, types


fa, sizes, ta = stage_backward(False, xs['a'])
fb, _, tb = stage_backward(True, xs['b'])
fc, _, tc = stage_backward(True, xs['c'])
ga, gb = fa()[-1], fb()[-1]
assert torch.equal(gb[FIVE.tolist()], ga) and int((gb.abs().amax(1) > 0).sum()) == 5            # (b) is (a), relabelled
print('input-stage backward, bench batch: %d local / %d global edges, %d triplet + pair rows, %d atoms; d = 128' % sizes)
verdict(timed([('(a) 5-row table', fa), ('(a again)', fa), ('(b) 95 rows, the same five elements', fb),
               ('(c) 95 rows, 40 elements', fc)]))

# ---- 2. the gradient alone
for n in (2286, 100000):
    if n == batch.x.numel():
        ia = batch.x.long()
    else:
        ia = torch.randint(0, 5, (n,), generator=gen)
    idx = {'a': ia.to(torch.int32).to(dev), 'b': FIVE[ia].to(torch.int32).to(dev), 'c': forty(n, gen).to(torch.int32).to(dev)}
    grad = torch.randn(n, 128, device=dev)
    out5, out95 = torch.empty(5, 128, device=dev), torch.empty(95, 128, device=dev)

    def call(i, T, out):
        scratch = ops.reduce_scratch(dev, T, 128)
        return lambda: lib.call('pamnet_type_rows_grad_f32', lib.ptr(grad), lib.ptr(i), n, T, 128, lib.ptr(scratch), lib.ptr(out),
                                lib.stream_of(grad))
    call(idx['a'], 5, out5)(), call(idx['b'], 95, out95)()
    assert torch.equal(out95[FIVE.tolist()], out5)
    print('pamnet_type_rows_grad_f32, n = %d, d = 128:' % n)
    verdict(timed([('(a) 5-row table', call(idx['a'], 5, out5)), ('(a again)', call(idx['a'], 5, out5)),
                   ('(b) 95 rows, the same five elements', call(idx['b'], 95, out95)),
                   ('(c) 95 rows, 40 elements', call(idx['c'], 95, out95))]))
