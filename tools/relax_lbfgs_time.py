"""What an L-BFGS relaxation step costs, and what it saves (profiles/relax_lbfgs.txt).  One process, the variants alternating
inside each round, device events:
  (i)   the step launch alone, pamnet_lbfgs_step_f32 called directly on synthetic gradients, at 3 and at 128 graphs, with no pair
        held (count = 0: 2 workgroup reductions) and with a full history at the default memory (count = 10: 22 reductions), and
        pamnet_fire_step_f32 beside it: us per call over `--calls` back-to-back calls.  The gradient stays the same from call to
        call, so y = 0, every new pair is refused and the history stays as prepared (asserted); a threshold of 0 keeps every
        graph running;
  (ii)  ms per relax_lbfgs() and per relax() iteration, QM9 B = 128, d = 128, L = 6 (the batch of profiles/relax.txt): the
        difference of a 50-step and a 10-step run over 40, so that the closing evaluation cancels; check_every = 0;
  (iii) steps to fmax = 0.05 of both drivers on a PAMNet batch (QM9-size molecules, the model of (ii)): per graph, with the pairs
        L-BFGS refused and its resets.
Run on the GPU box: python tools/relax_lbfgs_time.py [--rounds N] [--calls N] [--launch-only] [--graphs N] [--max-steps N]."""
import argparse
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=15)
ap.add_argument('--calls', type=int, default=200)
ap.add_argument('--launch-only', action='store_true', help='part (i) alone (for a kernel trace)')
ap.add_argument('--graphs', type=int, default=32, help='molecules of part (iii)')
ap.add_argument('--max-steps', type=int, default=400, help='step limit of part (iii)')
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'physics-aware-multiplex-gnn_amd'))

import torch  # noqa: E402
import models  # noqa: E402
from pamnet_amd import graph as G, relax as R, synth  # noqa: E402

dev = torch.device('cuda:0')
torch.manual_seed(0)
MEMORY = R.LBFGS_DEFAULTS['memory']


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


# ---- (i) the launch alone
def launch_case(graphs, count):
    b = synth.qm9_batch(0, 0, graphs).to(dev)
    gptr, _ = G.csr_from_keys(b.batch.to(torch.int32).contiguous(), graphs)
    n = b.pos.size(0)
    pos, de = b.pos.clone(), 0.05 * torch.randn(n, 3, device=dev)
    if count is None:                             # FIRE
        vel, state = R.new_state(n, graphs, dev)

        def run():
            for _ in range(args.calls):
                R.fire_step(pos, vel, de, gptr, state, 0.0)
        return n, run, state
    state = R.new_lbfgs_state(n, graphs, dev, MEMORY)
    if count:
        # pairs (s, y = H s) of one positive diagonal H: every curvature positive, the direction a descent direction
        H = torch.rand(n, 3, dtype=torch.float64, device=dev) * 3.5 + 0.5
        s = 0.05 * torch.randn(count, n, 3, dtype=torch.float64, device=dev)
        state['hist_s'][:count], state['hist_y'][:count] = s, H * s
        ys = torch.zeros(count, graphs, dtype=torch.float64, device=dev).index_add_(1, b.batch, (s * H * s).sum(2))
        yy = torch.zeros(count, graphs, dtype=torch.float64, device=dev).index_add_(1, b.batch, (H * s).pow(2).sum(2))
        state['rho'][:, :count] = (1.0 / ys).t()
        state['gamma'][:] = (ys / yy)[count - 1]
        state['count'][:] = count
        state['head'][:] = count % MEMORY

    def run():
        for _ in range(args.calls):
            R.lbfgs_step(pos, de, gptr, state, 0.0)
    return n, run, state


cases = {(g, c): launch_case(g, c) for g in (3, 128) for c in (None, 0, MEMORY)}
for n, run, state in cases.values():
    run()
times = {k: [] for k in cases}
for _ in range(args.rounds):
    for k, (n, run, state) in cases.items():
        times[k].append(timed(run))
print('(i) the step launch alone, %d back-to-back calls, %d rounds' % (args.calls, args.rounds))
for (g, c), (n, run, state) in cases.items():
    assert int(state['status'].abs().max()) == 0 and int(state['steps'].min()) == args.calls * (args.rounds + 1)
    if c is not None:
        assert int(state['resets'].max()) == 0 and bool((state['count'] == c).all())
        assert int(state['skipped'].min()) == args.calls * (args.rounds + 1) - 1
    report('%s, %d graphs, %d atoms' % ('fire' if c is None else 'lbfgs count=%d' % c, g, n), times[(g, c)], 'us',
           1000.0 / args.calls)

if args.launch_only:
    sys.exit(0)

# ---- (ii) at the headline batch
cfg = models.Config(dataset='QM9', dim=128, n_layer=6, cutoff_l=5.0, cutoff_g=5.0)
model = models.PAMNet(cfg).to(dev)
data = synth.qm9_batch(0, 0, 128).to(dev)
variants = {'lbfgs50': lambda: R.relax_lbfgs(model, data, fmax=0.0, max_steps=50, check_every=0),
            'fire50': lambda: R.relax(model, data, fmax=0.0, max_steps=50, check_every=0),
            'lbfgs10': lambda: R.relax_lbfgs(model, data, fmax=0.0, max_steps=10, check_every=0),
            'fire10': lambda: R.relax(model, data, fmax=0.0, max_steps=10, check_every=0)}
for fn in variants.values():
    fn()
t = {k: [] for k in variants}
for _ in range(args.rounds):
    for k, fn in variants.items():
        t[k].append(timed(fn))
print('(ii) QM9 B = 128 (%d atoms), d = 128, L = 6, check_every = 0, %d rounds' % (data.pos.size(0), args.rounds))
report('relax_lbfgs iteration', [(a - b) / 40 for a, b in zip(t['lbfgs50'], t['lbfgs10'])], 'ms', 1.0)
report('relax iteration', [(a - b) / 40 for a, b in zip(t['fire50'], t['fire10'])], 'ms', 1.0)
report('relax_lbfgs - relax', [((a - b) - (c - d)) / 40 for a, b, c, d in zip(t['lbfgs50'], t['lbfgs10'], t['fire50'], t['fire10'])],
       'ms', 1.0)

# ---- (iii) steps to fmax = 0.05
batch = synth.qm9_batch(0, 0, args.graphs).to(dev)
lb = R.relax_lbfgs(model, batch, fmax=0.05, max_steps=args.max_steps)
fi = R.relax(model, batch, fmax=0.05, max_steps=args.max_steps)
with torch.no_grad():
    e0 = model(batch)
print('(iii) steps to fmax = 0.05, %d molecules (%d atoms), the model of (ii), at most %d steps' % (args.graphs, batch.pos.size(0),
                                                                                                 args.max_steps))
print('  graph atoms | lbfgs: steps status skipped resets  E - E0 | fire: steps status  E - E0')
sizes = torch.bincount(batch.batch, minlength=args.graphs).tolist()
status = lambda r: ['running', 'converged', 'failed'][int(r[0]) + 2 * int(r[1])]
for g in range(args.graphs):
    print('  %5d %5d | %12d %9s %7d %6d %+.4e | %11d %9s %+.4e'
          % (g, sizes[g], int(lb.steps[g]), status((lb.converged[g], lb.failed[g])), int(lb.skipped[g]), int(lb.resets[g]),
             float(lb.energy[g] - e0[g]), int(fi.steps[g]), status((fi.converged[g], fi.failed[g])), float(fi.energy[g] - e0[g])))
both = lb.converged & fi.converged
print('  converged: lbfgs %d, fire %d, both %d of %d; over those both converged: lbfgs %d steps, fire %d steps in total (ratio %.2f)'
      % (int(lb.converged.sum()), int(fi.converged.sum()), int(both.sum()), args.graphs, int(lb.steps[both].sum()),
         int(fi.steps[both].sum()), float(fi.steps[both].sum()) / max(int(lb.steps[both].sum()), 1)))
print('  evaluations enqueued (the slowest graph decides): lbfgs %d, fire %d' % (int(lb.steps.max()), int(fi.steps.max())))
