"""What a constrained molecular-dynamics step costs (profiles/md_constraints.txt).  One process, the variants alternating inside
each round, device events:
  (i)   the step launch alone on synthetic gradients, at 3 and at 128 QM9-schema graphs, Langevin (gamma = 1):
        pamnet_md_constrained_step_f32 with every X-H bond constrained against pamnet_md_step_f32 on the same batch, us per call
        over `--calls` back-to-back calls, and the sweeps the last constrained launch took;
  (ii)  ms per run() iteration, QM9 B = 128, d = 128, L = 6 (the batch of profiles/md.txt), with the X-H constraints and without:
        the difference of a 50-step and a 10-step run() over 40, so that set-up and the closing evaluation cancel; the sweeps of
        the last launch of the constrained run;
  (iii) the same forward + torch.autograd.grad with respect to pos, 40 times, without the integrator.
Run on the GPU box: python tools/md_constraints_time.py [--rounds N] [--calls N] [--launch-only]."""
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
MASS = torch.tensor([1.008, 12.011, 14.007, 15.999, 18.998], device=dev)     # H, C, N, O, F by the schema's type index
TOL, SWEEPS = 1e-8, 500                           # (the defaults of run())


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
    print('  %-44s median_%s %8.3f  min_%s %8.3f  max_%s %8.3f' % (name, unit, statistics.median(v), unit, min(v), unit, max(v)),
          flush=True)


def xh(b):
    return M.Constraints(b, M.bond_constraints(b.edge_index, b.x == 0))


# ---- (i) the launches alone
def launch_case(count, constrained):
    b = synth.qm9_batch(0, 0, count).to(dev)
    gptr, _ = G.csr_from_keys(b.batch.to(torch.int32).contiguous(), count)
    n = b.pos.size(0)
    pos, de, mass = b.pos.clone(), 0.05 * torch.randn(n, 3, device=dev), MASS[b.x.long()].contiguous()
    vel, state = M.new_state(n, count, dev, seed=1)
    state['sweeps'] = torch.zeros(count, dtype=torch.int32, device=dev)
    cons = xh(b)

    def run():
        for _ in range(args.calls):
            if constrained:
                M.constrained_step(pos, vel, de, gptr, state, cons, 0.01, 0.05, 1.0, mass, tol=TOL, max_sweeps=SWEEPS)
            else:
                M.md_step(pos, vel, de, gptr, state, 0.01, 0.05, 1.0, mass)
    return n, run, state, cons


cases = {(name, c): launch_case(c, name != 'md_step') for c in (3, 128) for name in ('md_step', 'md_constrained_step')}
for n, run, state, cons in cases.values():
    run()
times = {k: [] for k in cases}
for _ in range(args.rounds):
    for k, (n, run, state, cons) in cases.items():
        times[k].append(timed(run))
print('(i) the launches alone, %d back-to-back calls, %d rounds' % (args.calls, args.rounds))
for (name, c), (n, run, state, cons) in cases.items():
    assert int(state['status'].abs().max()) == 0 and int(state['steps'].min()) == args.calls * (args.rounds + 1)
    report('%s, %d graphs, %d atoms' % (name, c, n), times[(name, c)], 'us', 1000.0 / args.calls)
    if name != 'md_step':
        s = state['sweeps'].float()
        print('      %d constraints in %d colours at most; sweeps of the last launch: mean %.2f, most %d'
              % (cons.n, int((cons.gcol[1:] - cons.gcol[:-1]).max()), float(s.mean()), int(s.max())))

if args.launch_only:
    sys.exit(0)

# ---- (ii), (iii) at the headline batch
cfg = models.Config(dataset='QM9', dim=128, n_layer=6, cutoff_l=5.0, cutoff_g=5.0)
model = models.PAMNet(cfg).to(dev)
data = synth.qm9_batch(0, 0, 128).to(dev)
masses = MASS[data.x.long()].contiguous()
seeds = torch.arange(128, dtype=torch.int64, device=dev)
cons = xh(data)


def evaluations(k):
    cur = data.pos.detach().clone()
    for _ in range(k):
        d = copy.copy(data)
        d.pos = cur.detach().requires_grad_(True)
        e = model(d)
        torch.autograd.grad(e.sum(), d.pos)


# dt = 0.1 (about 1 fs with eV, Angstrom and amu) and its double, from a Maxwell-Boltzmann start at kT = 0.025
lan = dict(masses=masses, kT=0.025, gamma=0.1, seed=seeds)
variants = {'free50': lambda: M.run(model, data, 50, 0.1, **lan), 'free10': lambda: M.run(model, data, 10, 0.1, **lan),
            'cons50': lambda: M.run(model, data, 50, 0.1, constraints=cons, **lan),
            'cons10': lambda: M.run(model, data, 10, 0.1, constraints=cons, **lan),
            'dbl50': lambda: M.run(model, data, 50, 0.2, constraints=cons, **lan),
            'dbl10': lambda: M.run(model, data, 10, 0.2, constraints=cons, **lan),
            'eval40': lambda: evaluations(40)}
last = {}
for k, fn in variants.items():
    last[k] = fn()
t = {k: [] for k in variants}
for _ in range(args.rounds):
    for k, fn in variants.items():
        t[k].append(timed(fn))
print('(ii) / (iii) QM9 B = 128 (%d atoms, %d X-H constraints), d = 128, L = 6, %d rounds' % (data.pos.size(0), cons.n, args.rounds))
per = lambda a, b: [(x - y) / 40 for x, y in zip(t[a], t[b])]
report('(ii) run iteration, no constraints, dt 0.1', per('free50', 'free10'), 'ms', 1.0)
report('(ii) run iteration, X-H constrained, dt 0.1', per('cons50', 'cons10'), 'ms', 1.0)
report('(ii) run iteration, X-H constrained, dt 0.2', per('dbl50', 'dbl10'), 'ms', 1.0)
report('(iii) forward + grad', [a / 40 for a in t['eval40']], 'ms', 1.0)
report('(ii) constrained - free, dt 0.1', [a - b for a, b in zip(per('cons50', 'cons10'), per('free50', 'free10'))], 'ms', 1.0)
for k, dt in (('cons50', 0.1), ('dbl50', 0.2)):
    r = last[k]
    p = r.pos.double()
    d = (p[cons.i.long()] - p[cons.j.long()]).norm(dim=1)
    tr = M.run(model, data, 10, dt, constraints=cons, trace=True, **lan)       # the sweeps of the ten advancing launches
    s = torch.stack([x['state_after']['sweeps'] for x in tr.trace[:-1]]).float()
    print('  dt %.1f: 50 steps: steps %d..%d, failed %d, unconverged %d, largest |d - length| %.2e; sweeps per launch over 10 steps '
          '(the most of its seven solves, per graph): mean %.2f, most %d'
          % (dt, int(r.steps.min()), int(r.steps.max()), int(r.failed.sum()), int(r.unconverged.sum()),
             float((d - cons.d).abs().max()), float(s.mean()), int(s.max())))
