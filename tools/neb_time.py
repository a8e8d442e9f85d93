"""What a nudged-elastic-band iteration costs (profiles/neb.txt).  One process, the variants alternating inside each round, device
events:
  (i)   the projection launch alone, pamnet_neb_force_f32 called directly on synthetic gradients and energies, at one band of 5
        images and at 16 bands of 8 images (128 graphs, a QM9-sized batch): us per call over `--calls` back-to-back calls;
  (ii)  ms per neb.run() iteration at the 128-graph batch, QM9 d = 128, L = 6: the difference of a 50-step and a 10-step run over
        40, so that set-up and the closing evaluation cancel; check_every = 0 and = 10, the climbing image from step 5;
  (iii) the same forward + torch.autograd.grad with respect to pos, 40 times, without projection and step.
Run on the GPU box: python tools/neb_time.py [--rounds N] [--calls N] [--launch-only]."""
import argparse
import copy
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=15)
ap.add_argument('--calls', type=int, default=200)
ap.add_argument('--launch-only', action='store_true', help='part (i) alone (for a kernel trace)')
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'physics-aware-multiplex-gnn_amd'))

import torch  # noqa: E402
import models  # noqa: E402
from pamnet_amd import graph as G, neb, synth  # noqa: E402

dev = torch.device('cuda:0')
torch.manual_seed(0)


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def report(name, times, unit, scale):
    v = [t * scale for t in times]
    print('  %-34s median_%s %8.3f  min_%s %8.3f  max_%s %8.3f' % (name, unit, statistics.median(v), unit, min(v), unit, max(v)),
          flush=True)


def bands(n_bands, n_images):
    """n_bands QM9-sized molecules, each stretched into a band towards a copy displaced by up to 0.3 A per coordinate."""
    a = synth.qm9_batch(0, 0, n_bands).to(dev)
    b = copy.copy(a)
    b.pos = a.pos + 0.6 * (torch.rand_like(a.pos) - 0.5)
    return neb.interpolate(a, b, n_images)


# ---- (i) the launch alone
def launch_case(n_bands, n_images):
    d = bands(n_bands, n_images)
    count = int(d.num_graphs)
    gptr, _ = G.csr_from_keys(d.batch.to(torch.int32).contiguous(), count)
    band_of = torch.arange(count, device=dev, dtype=torch.int32) // n_images
    n = d.pos.size(0)
    de, energy = 0.05 * torch.randn(n, 3, device=dev), torch.randn(count, device=dev)
    dneb = torch.zeros_like(de)
    seg, fpar = torch.zeros(count, dtype=torch.float64, device=dev), torch.zeros(count, dtype=torch.float64, device=dev)
    climb = torch.ones(n_bands, dtype=torch.uint8, device=dev)

    def run():
        for _ in range(args.calls):
            neb.neb_force(d.pos, de, energy, gptr, d.band_ptr, band_of, dneb, 0.1, seg, fpar, None, None, climb)
    return n, count, run, dneb


cases = {c: launch_case(*c) for c in ((1, 5), (16, 8))}
for n, count, run, dneb in cases.values():
    run()
times = {c: [] for c in cases}
for _ in range(args.rounds):
    for c, (n, count, run, dneb) in cases.items():
        times[c].append(timed(run))
print('(i) pamnet_neb_force_f32 alone, %d back-to-back calls, %d rounds' % (args.calls, args.rounds))
for c, (n, count, run, dneb) in cases.items():
    assert bool(torch.isfinite(dneb).all()) and bool(dneb.any())
    report('%d band(s) x %d images, %d atoms' % (c[0], c[1], n), times[c], 'us', 1000.0 / args.calls)

if args.launch_only:
    sys.exit(0)

# ---- (ii), (iii) at the 128-graph batch
cfg = models.Config(dataset='QM9', dim=128, n_layer=6, cutoff_l=5.0, cutoff_g=5.0)
model = models.PAMNet(cfg).to(dev)
data = bands(16, 8)


def evaluations(k):
    cur = data.pos.detach().clone()
    for _ in range(k):
        d = copy.copy(data)
        d.pos = cur.detach().requires_grad_(True)
        e = model(d)
        torch.autograd.grad(e.sum(), d.pos)


def neb_run(steps, ce):
    return lambda: neb.run(model, data, fmax=0.0, k=0.1, climb_after=5, max_steps=steps, check_every=ce)


variants = {'neb50 ce0': neb_run(50, 0), 'neb10 ce0': neb_run(10, 0), 'neb50 ce10': neb_run(50, 10), 'neb10 ce10': neb_run(10, 10),
            'eval40': lambda: evaluations(40)}
for fn in variants.values():
    fn()
t = {k: [] for k in variants}
for _ in range(args.rounds):
    for k, fn in variants.items():
        t[k].append(timed(fn))
print('(ii) / (iii) 16 bands x 8 images = 128 graphs (%d atoms), QM9 d = 128, L = 6, %d rounds' % (data.pos.size(0), args.rounds))
report('(ii) neb iteration, ce=0', [(a - b) / 40 for a, b in zip(t['neb50 ce0'], t['neb10 ce0'])], 'ms', 1.0)
report('(ii) neb iteration, ce=10', [(a - b) / 40 for a, b in zip(t['neb50 ce10'], t['neb10 ce10'])], 'ms', 1.0)
report('(iii) forward + grad', [a / 40 for a in t['eval40']], 'ms', 1.0)
report('(ii) - (iii), ce=0', [(a - b) / 40 - c / 40 for a, b, c in zip(t['neb50 ce0'], t['neb10 ce0'], t['eval40'])], 'ms', 1.0)
report('(ii) - (iii), ce=10', [(a - b) / 40 - c / 40 for a, b, c in zip(t['neb50 ce10'], t['neb10 ce10'], t['eval40'])], 'ms', 1.0)
