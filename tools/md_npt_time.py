"""What a constant-pressure molecular-dynamics step costs (profiles/md_npt.txt).  One process, the variants alternating inside each
round, device events:
  (i)   the step launch alone, back to back: pamnet_md_npt_step_f32 against pamnet_md_step_f32 from the same build, on the same
        synthetic gradients, Langevin (gamma = 1, kT = 0.05: both generators run), at 3 and at 128 graphs: us per call over
        `--calls` calls (a rate of 1e-9 keeps the cells where they are while every statement of the step runs);
  (ii)  ms per iteration of run_npt() on a periodic batch (128 cells of 18 atoms, 12 A, d = 128, L = 6): the difference of a 50-step
        and a 10-step run over 40, so that set-up and the closing evaluation cancel; check_every = 0, no records;
  (iii) the same shallow copy + forward + torch.autograd.grad with respect to [pos, strain], 40 times, without the step;
  (iv)  ms per iteration of run() (NVT, no strain attached) on the same batch, the same way: (ii) - (iv) is what attaching `strain`
        costs, the virial backward included.
Run on the GPU box: python tools/md_npt_time.py [--rounds N] [--calls N] [--launch-only]."""
import argparse
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
from pamnet_amd import graph as G, md as M, relax as R, synth  # noqa: E402

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
    print('  %-42s median_%s %8.3f  min_%s %8.3f  max_%s %8.3f' % (name, unit, statistics.median(v), unit, min(v), unit, max(v)),
          flush=True)


# ---- (i) the launches alone
def launch_case(count):
    b = synth.qm9_batch(0, 0, count).to(dev)
    gptr, _ = G.csr_from_keys(b.batch.to(torch.int32).contiguous(), count)
    n = b.pos.size(0)
    de = 0.05 * torch.randn(n, 3, device=dev)
    mass = 1.0 + 15.0 * torch.rand(n, device=dev)
    pos_f, pos_c = b.pos.clone(), b.pos.clone()
    cell0 = (12.0 * torch.eye(3, device=dev)).repeat(count, 1, 1).contiguous()
    cell, w = cell0.clone(), torch.zeros(count, 3, 3, device=dev)
    vel_f, st_f = M.new_state(n, count, dev, seed=1)
    vel_c, st_c = M.new_npt_state(n, count, dev, cell0, seed=1)

    def fixed_cell():
        for _ in range(args.calls):
            M.md_step(pos_f, vel_f, de, gptr, st_f, 0.01, 0.05, 1.0, mass)

    def barostat():
        for _ in range(args.calls):
            M.npt_step(pos_c, vel_c, de, w, gptr, cell0, cell, st_c, 0.01, 0.05, 0.0, 1e-9, 1.0, mass)
    return n, {'pamnet_md_step_f32': (fixed_cell, st_f), 'pamnet_md_npt_step_f32': (barostat, st_c)}


cases = {c: launch_case(c) for c in (3, 128)}
times = {(c, k): [] for c, (n, runs) in cases.items() for k in runs}
for c, (n, runs) in cases.items():
    for k, (run, st) in runs.items():
        run()
for _ in range(args.rounds):
    for c, (n, runs) in cases.items():
        for k, (run, st) in runs.items():
            times[(c, k)].append(timed(run))
print('(i) the step launches alone, Langevin, %d back-to-back calls, %d rounds' % (args.calls, args.rounds))
for c, (n, runs) in cases.items():
    for k, (run, st) in runs.items():
        assert int(st['status'].abs().max()) == 0 and int(st['steps'].min()) == args.calls * (args.rounds + 1)
        report('%s, %d graphs, %d atoms' % (k.replace('pamnet_', '').replace('_f32', ''), c, n), times[(c, k)], 'us',
               1000.0 / args.calls)

if args.launch_only:
    sys.exit(0)

# ---- (ii) - (iv) the drivers on one periodic batch (the batch of tools/relax_cell_time.py)
B, ATOMS, EDGE = 128, 18, 12.0
gen = torch.Generator().manual_seed(1)
grid = torch.stack(torch.meshgrid(*[torch.arange(3.0)] * 3, indexing='ij'), -1).reshape(-1, 3)[:ATOMS] * (EDGE / 3.0)
pos = torch.cat([grid + 1.0 + 0.5 * torch.rand(ATOMS, 3, generator=gen) for _ in range(B)])          # (pairs 3.5 A apart or more)
data = synth.Batch(x=torch.randint(0, 5, (B * ATOMS,), generator=gen).float(), pos=pos,
                   batch=torch.arange(B).repeat_interleave(ATOMS), cell=(EDGE * torch.eye(3)).repeat(B, 1, 1), num_graphs=B).to(dev)
cfg = models.Config(dataset='QM9', dim=128, n_layer=6, cutoff_l=5.0, cutoff_g=5.0)
model = models.PAMNet(cfg).to(dev)
masses = 1.0 + 15.0 * torch.rand(B * ATOMS, device=dev)
seeds = torch.arange(B, dtype=torch.int64, device=dev)
zero = torch.zeros_like(data.pos)


def evaluations(k):
    cur, cell = data.pos.detach().clone(), data.cell.detach().clone()
    for _ in range(k):
        R._evaluate_cell(model, data, cur, cell)


# dt = 1e-3 and rate = 1e-6: atoms and cells hardly move, so every iteration evaluates the same graph and every height stays at 12 A
common = dict(dt=1e-3, masses=masses, velocities=zero, kT=0.02, gamma=1.0, seed=seeds)
npt = dict(common, pressure=0.0, tau_p=1.0, compressibility=1e-6)
variants = {'npt50': lambda: M.run_npt(model, data, 50, **npt), 'npt10': lambda: M.run_npt(model, data, 10, **npt),
            'nvt50': lambda: M.run(model, data, 50, **common), 'nvt10': lambda: M.run(model, data, 10, **common),
            'eval40': lambda: evaluations(40)}
for fn in variants.values():
    fn()
t = {k: [] for k in variants}
for _ in range(args.rounds):
    for k, fn in variants.items():
        t[k].append(timed(fn))
print('(ii) - (iv) %d periodic cells of %d atoms (%d atoms), d = 128, L = 6, Langevin, check_every = 0, %d rounds'
      % (B, ATOMS, B * ATOMS, args.rounds))
npt_it = [(a - b) / 40 for a, b in zip(t['npt50'], t['npt10'])]
nvt_it = [(a - b) / 40 for a, b in zip(t['nvt50'], t['nvt10'])]
ev_it = [a / 40 for a in t['eval40']]
report('(ii) run_npt iteration', npt_it, 'ms', 1.0)
report('(iii) forward + grad([pos, strain])', ev_it, 'ms', 1.0)
report('(iv) run iteration (NVT, no strain)', nvt_it, 'ms', 1.0)
report('(ii) - (iii)', [a - b for a, b in zip(npt_it, ev_it)], 'ms', 1.0)
report('(ii) - (iv)', [a - b for a, b in zip(npt_it, nvt_it)], 'ms', 1.0)
