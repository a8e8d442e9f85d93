"""What a molecular-dynamics step costs (profiles/md.txt).  One process, the variants alternating inside each round, device events:
  (i)   the step launch alone, pamnet_md_step_f32 called directly on synthetic gradients, at 3 and at 128 graphs, NVE (gamma = 0)
        and Langevin (gamma = 1: the generator runs): us per call over `--calls` back-to-back calls; and one
        pamnet_md_init_velocities_f32 call the same way;
  (ii)  ms per run() iteration, QM9 B = 128, d = 128, L = 6 (the batch of profiles/forces_qm9_b128.txt): the difference of a
        50-step and a 10-step run() over 40, so that set-up and the closing evaluation cancel; NVE and Langevin;
  (iii) the same forward + torch.autograd.grad with respect to pos, 40 times, without the integrator.
Run on the GPU box: python tools/md_time.py [--rounds N] [--calls N] [--launch-only]."""
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
from pamnet_amd import graph as G, md as M, synth  # noqa: E402

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
    print('  %-30s median_%s %8.3f  min_%s %8.3f  max_%s %8.3f' % (name, unit, statistics.median(v), unit, min(v), unit, max(v)),
          flush=True)


# ---- (i) the launches alone
def launch_case(count, gamma, init=False):
    b = synth.qm9_batch(0, 0, count).to(dev)
    gptr, _ = G.csr_from_keys(b.batch.to(torch.int32).contiguous(), count)
    n = b.pos.size(0)
    pos, de = b.pos.clone(), 0.05 * torch.randn(n, 3, device=dev)
    mass = 1.0 + 15.0 * torch.rand(n, device=dev)
    vel, state = M.new_state(n, count, dev, seed=1)

    def run():
        for _ in range(args.calls):
            if init:
                M.init_velocities(vel, gptr, state['seed'], 0.05, state['ke'], mass)
            else:
                M.md_step(pos, vel, de, gptr, state, 0.01, 0.05, gamma, mass)
    return n, run, state


cases = {('step NVE', 3): launch_case(3, 0.0), ('step NVE', 128): launch_case(128, 0.0),
         ('step Langevin', 3): launch_case(3, 1.0), ('step Langevin', 128): launch_case(128, 1.0),
         ('init_velocities', 3): launch_case(3, 0.0, True), ('init_velocities', 128): launch_case(128, 0.0, True)}
for n, run, state in cases.values():
    run()
times = {k: [] for k in cases}
for _ in range(args.rounds):
    for k, (n, run, state) in cases.items():
        times[k].append(timed(run))
print('(i) the launches alone, %d back-to-back calls, %d rounds' % (args.calls, args.rounds))
for (name, c), (n, run, state) in cases.items():
    assert int(state['status'].abs().max()) == 0
    assert name == 'init_velocities' or int(state['steps'].min()) == args.calls * (args.rounds + 1)
    report('%s, %d graphs, %d atoms' % (name, c, n), times[(name, c)], 'us', 1000.0 / args.calls)

if args.launch_only:
    sys.exit(0)

# ---- (ii), (iii) at the headline batch
cfg = models.Config(dataset='QM9', dim=128, n_layer=6, cutoff_l=5.0, cutoff_g=5.0)
model = models.PAMNet(cfg).to(dev)
data = synth.qm9_batch(0, 0, 128).to(dev)
masses = 1.0 + 15.0 * torch.rand(data.pos.size(0), device=dev)
seeds = torch.arange(128, dtype=torch.int64, device=dev)
zero = torch.zeros_like(data.pos)


def evaluations(k):
    cur = data.pos.detach().clone()
    for _ in range(k):
        d = copy.copy(data)
        d.pos = cur.detach().requires_grad_(True)
        e = model(d)
        torch.autograd.grad(e.sum(), d.pos)


# dt = 1e-3: the atoms hardly move, so every iteration evaluates the graph of the benchmark batch
nve = dict(dt=1e-3, masses=masses, velocities=zero)
lan = dict(dt=1e-3, masses=masses, velocities=zero, kT=0.02, gamma=1.0, seed=seeds)
variants = {'nve50': lambda: M.run(model, data, 50, **nve), 'nve10': lambda: M.run(model, data, 10, **nve),
            'lan50': lambda: M.run(model, data, 50, **lan), 'lan10': lambda: M.run(model, data, 10, **lan),
            'eval40': lambda: evaluations(40)}
for fn in variants.values():
    fn()
t = {k: [] for k in variants}
for _ in range(args.rounds):
    for k, fn in variants.items():
        t[k].append(timed(fn))
print('(ii) / (iii) QM9 B = 128 (%d atoms), d = 128, L = 6, %d rounds' % (data.pos.size(0), args.rounds))
report('(ii) run iteration, NVE', [(a - b) / 40 for a, b in zip(t['nve50'], t['nve10'])], 'ms', 1.0)
report('(ii) run iteration, Langevin', [(a - b) / 40 for a, b in zip(t['lan50'], t['lan10'])], 'ms', 1.0)
report('(iii) forward + grad', [a / 40 for a in t['eval40']], 'ms', 1.0)
report('(ii) - (iii), NVE', [(a - b) / 40 - c / 40 for a, b, c in zip(t['nve50'], t['nve10'], t['eval40'])], 'ms', 1.0)
report('(ii) - (iii), Langevin', [(a - b) / 40 - c / 40 for a, b, c in zip(t['lan50'], t['lan10'], t['eval40'])], 'ms', 1.0)
