"""What a variable-cell relaxation step costs (profiles/relax_cell.txt).  One process, the variants alternating inside each round,
device events:
  (i)   the step launch alone, back to back: pamnet_fire_cell_step_f32 against pamnet_fire_step_f32 from the same build, on the
        same synthetic gradients, at 3 and at 128 graphs: us per call over `--calls` calls (thresholds of 0 keep every graph
        running; the virial is zero, so the cells stay where they are while every statement of the step runs);
  (ii)  ms per iteration of relax_cell() against relax() on the same periodic batch (128 cells of 18 atoms, 12 A, d = 128, L = 6):
        the difference of a 50-step and a 10-step run over 40, so that set-up and the closing evaluation cancel; check_every = 0.
        The difference between the two drivers is the virial backward plus the step.
Run on the GPU box: python tools/relax_cell_time.py [--rounds N] [--calls N] [--launch-only]."""
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
    print('  %-42s median_%s %8.3f  min_%s %8.3f  max_%s %8.3f' % (name, unit, statistics.median(v), unit, min(v), unit, max(v)),
          flush=True)


# ---- (i) the launches alone
def launch_case(count):
    b = synth.qm9_batch(0, 0, count).to(dev)
    gptr, _ = G.csr_from_keys(b.batch.to(torch.int32).contiguous(), count)
    n = b.pos.size(0)
    de = 0.05 * torch.randn(n, 3, device=dev)
    pos_f, pos_c = b.pos.clone(), b.pos.clone()
    vel_f, st_f = R.new_state(n, count, dev)
    vel_c, st_c = R.new_cell_state(n, count, dev)
    cell0 = (12.0 * torch.eye(3, device=dev)).repeat(count, 1, 1).contiguous()
    cell, w = cell0.clone(), torch.zeros(count, 3, 3, device=dev)
    factor = (gptr[1:] - gptr[:-1]).to(torch.float64).contiguous()

    def fixed_cell():
        for _ in range(args.calls):
            R.fire_step(pos_f, vel_f, de, gptr, st_f, 0.0)

    def variable_cell():
        for _ in range(args.calls):
            R.fire_cell_step(pos_c, vel_c, de, w, gptr, cell0, cell, st_c, 0.0, 0.0, factor)
    return n, {'pamnet_fire_step_f32': (fixed_cell, st_f), 'pamnet_fire_cell_step_f32': (variable_cell, st_c)}


cases = {c: launch_case(c) for c in (3, 128)}
times = {(c, k): [] for c, (n, runs) in cases.items() for k in runs}
for c, (n, runs) in cases.items():
    for k, (run, st) in runs.items():
        run()
for _ in range(args.rounds):
    for c, (n, runs) in cases.items():
        for k, (run, st) in runs.items():
            times[(c, k)].append(timed(run))
print('(i) the step launches alone, %d back-to-back calls, %d rounds' % (args.calls, args.rounds))
for c, (n, runs) in cases.items():
    for k, (run, st) in runs.items():
        assert int(st['status'].abs().max()) == 0 and int(st['steps'].min()) == args.calls * (args.rounds + 1)
        report('%s, %d graphs, %d atoms' % (k.replace('pamnet_', '').replace('_f32', ''), c, n), times[(c, k)], 'us',
               1000.0 / args.calls)

if args.launch_only:
    sys.exit(0)

# ---- (ii) the drivers on one periodic batch
B, ATOMS, EDGE = 128, 18, 12.0
gen = torch.Generator().manual_seed(1)
grid = torch.stack(torch.meshgrid(*[torch.arange(3.0)] * 3, indexing='ij'), -1).reshape(-1, 3)[:ATOMS] * (EDGE / 3.0)
pos = torch.cat([grid + 1.0 + 0.5 * torch.rand(ATOMS, 3, generator=gen) for _ in range(B)])          # (pairs 3.5 A apart or more)
data = synth.Batch(x=torch.randint(0, 5, (B * ATOMS,), generator=gen).float(), pos=pos,
                   batch=torch.arange(B).repeat_interleave(ATOMS), cell=(EDGE * torch.eye(3)).repeat(B, 1, 1), num_graphs=B).to(dev)
cfg = models.Config(dataset='QM9', dim=128, n_layer=6, cutoff_l=5.0, cutoff_g=5.0)
model = models.PAMNet(cfg).to(dev)
# a cell factor of 1e4 atoms keeps every height above twice the cutoff for the whole run: 60 steps move the strain by 1e-3
variants = {'relax_cell50': lambda: R.relax_cell(model, data, fmax=0.0, smax=0.0, cell_factor=1e4, max_steps=50, check_every=0),
            'relax_cell10': lambda: R.relax_cell(model, data, fmax=0.0, smax=0.0, cell_factor=1e4, max_steps=10, check_every=0),
            'relax50': lambda: R.relax(model, data, fmax=0.0, max_steps=50, check_every=0),
            'relax10': lambda: R.relax(model, data, fmax=0.0, max_steps=10, check_every=0)}
for fn in variants.values():
    fn()
t = {k: [] for k in variants}
for _ in range(args.rounds):
    for k, fn in variants.items():
        t[k].append(timed(fn))
print('(ii) %d periodic cells of %d atoms (%d atoms), d = 128, L = 6, check_every = 0, %d rounds' % (B, ATOMS, B * ATOMS, args.rounds))
cell_it = [(a - b) / 40 for a, b in zip(t['relax_cell50'], t['relax_cell10'])]
fixed_it = [(a - b) / 40 for a, b in zip(t['relax50'], t['relax10'])]
report('relax_cell iteration', cell_it, 'ms', 1.0)
report('relax iteration', fixed_it, 'ms', 1.0)
report('relax_cell - relax', [a - b for a, b in zip(cell_it, fixed_it)], 'ms', 1.0)
