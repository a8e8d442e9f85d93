"""What a relaxation step costs (profiles/relax.txt).  One process, the variants alternating inside each round, device events:
  (i)   the step launch alone, pamnet_fire_step_f32 called directly on synthetic gradients, at 3 and at 128 graphs: us per call
        over `--calls` back-to-back calls (a threshold of 0 keeps every graph running);
  (ii)  ms per relax() iteration, QM9 B = 128, d = 128, L = 6 (the batch of profiles/forces_qm9_b128.txt): the difference of a
        50-step and a 10-step relax() over 40, so that the closing evaluation cancels; check_every = 0 and = 10;
  (iii) the same forward + torch.autograd.grad with respect to pos, 40 times, without the optimiser step.
Run on the GPU box: python tools/relax_time.py [--rounds N] [--calls N] [--launch-only]."""
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
from pamnet_amd import graph as G, relax as R, synth  # noqa: E402

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
    print('  %-28s median_%s %8.3f  min_%s %8.3f  max_%s %8.3f' % (name, unit, statistics.median(v), unit, min(v), unit, max(v)),
          flush=True)


# ---- (i) the launch alone
def launch_case(count):
    b = synth.qm9_batch(0, 0, count).to(dev)
    gptr, _ = G.csr_from_keys(b.batch.to(torch.int32).contiguous(), count)
    n = b.pos.size(0)
    pos, de = b.pos.clone(), 0.05 * torch.randn(n, 3, device=dev)
    vel, state = R.new_state(n, count, dev)

    def run():
        for _ in range(args.calls):
            R.fire_step(pos, vel, de, gptr, state, 0.0)
    return n, run, state


cases = {c: launch_case(c) for c in (3, 128)}
for c, (n, run, state) in cases.items():
    run()
times = {c: [] for c in cases}
for _ in range(args.rounds):
    for c, (n, run, state) in cases.items():
        times[c].append(timed(run))
print('(i) pamnet_fire_step_f32 alone, %d back-to-back calls, %d rounds' % (args.calls, args.rounds))
for c, (n, run, state) in cases.items():
    assert int(state['status'].abs().max()) == 0 and int(state['steps'].min()) == args.calls * (args.rounds + 1)
    report('%d graphs, %d atoms' % (c, n), times[c], 'us', 1000.0 / args.calls)

if args.launch_only:
    sys.exit(0)

# ---- (ii), (iii) at the headline batch
cfg = models.Config(dataset='QM9', dim=128, n_layer=6, cutoff_l=5.0, cutoff_g=5.0)
model = models.PAMNet(cfg).to(dev)
data = synth.qm9_batch(0, 0, 128).to(dev)


def evaluations(k):
    cur = data.pos.detach().clone()
    for _ in range(k):
        d = copy.copy(data)
        d.pos = cur.detach().requires_grad_(True)
        e = model(d)
        torch.autograd.grad(e.sum(), d.pos)


variants = {'relax50 ce0': lambda: R.relax(model, data, fmax=0.0, max_steps=50, check_every=0),
            'relax10 ce0': lambda: R.relax(model, data, fmax=0.0, max_steps=10, check_every=0),
            'relax50 ce10': lambda: R.relax(model, data, fmax=0.0, max_steps=50, check_every=10),
            'relax10 ce10': lambda: R.relax(model, data, fmax=0.0, max_steps=10, check_every=10),
            'eval40': lambda: evaluations(40)}
for fn in variants.values():
    fn()
t = {k: [] for k in variants}
for _ in range(args.rounds):
    for k, fn in variants.items():
        t[k].append(timed(fn))
print('(ii) / (iii) QM9 B = 128 (%d atoms), d = 128, L = 6, %d rounds' % (data.pos.size(0), args.rounds))
report('(ii) relax iteration, ce=0', [(a - b) / 40 for a, b in zip(t['relax50 ce0'], t['relax10 ce0'])], 'ms', 1.0)
report('(ii) relax iteration, ce=10', [(a - b) / 40 for a, b in zip(t['relax50 ce10'], t['relax10 ce10'])], 'ms', 1.0)
report('(iii) forward + grad', [a / 40 for a in t['eval40']], 'ms', 1.0)
report('(ii) - (iii), ce=0', [(a - b) / 40 - c / 40 for a, b, c in zip(t['relax50 ce0'], t['relax10 ce0'], t['eval40'])], 'ms', 1.0)
report('(ii) - (iii), ce=10', [(a - b) / 40 - c / 40 for a, b, c in zip(t['relax50 ce10'], t['relax10 ce10'], t['eval40'])], 'ms', 1.0)
