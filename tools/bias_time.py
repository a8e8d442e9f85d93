"""What a bias over collective variables costs on top of plain dynamics (profiles/bias.txt).  One process, the variants
alternating inside each round, device events:
  (i)   the bias launch alone, pamnet_bias_apply_f64 on 128 QM9-schema molecules, every graph a group of its own with a phi / psi
        pair of dihedrals (2-d hills) and a wall on a distance, with 0, 400 and 4096 hills per table, deposit 0, and one group of
        128 walkers on one table of 400 hills; us per call over `--calls` back-to-back calls;
  (ii)  ms per iteration of md.run with and without `bias` (2-d well-tempered metadynamics, pace 50, and the wall) at the QM9
        batch (B = 128, d = 128, L = 6) and on 128 harmonic wells of 20 atoms (a plain torch module): the difference of a 210-step
        and a 10-step run over 200, so that set-up and the closing evaluation cancel.
`--plain` measures md.run without a bias alone and imports nothing of the bias: it runs on a tree that has none.
Run on the GPU box: python tools/bias_time.py [--rounds N] [--calls N] [--plain] [--launch-only]."""
import argparse
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=15)
ap.add_argument('--calls', type=int, default=200)
ap.add_argument('--plain', action='store_true', help='md.run without a bias alone (for a tree without pamnet_amd.bias)')
ap.add_argument('--launch-only', action='store_true', help='part (i) alone (for a kernel trace)')
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'physics-aware-multiplex-gnn_amd'))

import torch  # noqa: E402
import models  # noqa: E402
from pamnet_amd import md as M, synth  # noqa: E402

dev = torch.device('cuda:0')
torch.manual_seed(0)
MASS = torch.tensor([1.008, 12.011, 14.007, 15.999, 18.998], device=dev)     # H, C, N, O, F by the schema's type index
B_GRAPHS, PACE = 128, 50


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
    print('  %-58s median_%s %8.3f  min_%s %8.3f  max_%s %8.3f' % (name, unit, statistics.median(v), unit, min(v), unit, max(v)),
          flush=True)


class Harmonic(torch.nn.Module):
    def __init__(self, k, x0):
        super().__init__()
        self.register_buffer('k', k)
        self.register_buffer('x0', x0)

    def forward(self, data):
        r2 = (data.pos - self.x0).pow(2).sum(1)
        return 0.5 * self.k * torch.zeros_like(self.k).index_add_(0, data.batch, r2)


data = synth.qm9_batch(0, 0, B_GRAPHS).to(dev)
first = torch.cat([torch.zeros(1, dtype=torch.long, device=dev), torch.bincount(data.batch.long()).cumsum(0)])[:-1].tolist()


def make_bias(walkers=None, capacity=None):
    from pamnet_amd import bias as B
    cvs, rs = [], {}
    for g, o in enumerate(first):
        cvs += [B.dihedral(o, o + 1, o + 2, o + 3), B.dihedral(o + 1, o + 2, o + 3, o + 4), B.distance(o, o + 5)]
        rs[3 * g + 2] = dict(kappa=0.5, centre=3.0, halfwidth=1.0)
    return B.Bias(data, cvs, restraints=rs, walkers=walkers, capacity=capacity,
                  metadynamics=dict(ndim=2, sigma=0.35, height=0.01, bias_factor=8.0, kT=0.025, pace=PACE))


# ---- (i) the launch alone
if not args.plain:
    def launch_case(hills, walkers=None):
        b = make_bias(walkers, capacity=max(hills, 1))
        T = b.n_groups
        b.tab['hill_c'][:, :hills] = (torch.rand(T, hills, 2, device=dev, dtype=torch.float64) * 2 - 1) * 3.14159
        b.tab['hill_w'][:, :hills] = 0.01
        b.tab['n_hills'].fill_(hills)
        de = 0.05 * torch.randn(data.pos.size(0), 3, device=dev)
        status = torch.zeros(B_GRAPHS, dtype=torch.int32, device=dev)

        def run():
            for _ in range(args.calls):
                b.apply(data.pos, de, status, 0)
        return run, status

    cases = {'128 groups of 1, %4d hills each' % h: launch_case(h) for h in (0, 400, 4096)}
    cases['1 group of 128 walkers, 400 hills'] = launch_case(400, walkers=128)
    for run, _ in cases.values():
        run()
    t_l = {k: [] for k in cases}
    for _ in range(args.rounds):
        for k, (run, _) in cases.items():
            t_l[k].append(timed(run))
    print('(i) the bias launch alone, %d atoms, %d back-to-back calls, %d rounds' % (data.pos.size(0), args.calls, args.rounds))
    for k, (_, status) in cases.items():
        assert int(status.abs().max()) == 0
        report('bias_apply, ' + k, t_l[k], 'us', 1000.0 / args.calls)
    if args.launch_only:
        sys.exit(0)

# ---- (ii) md.run with and without
cfg = models.Config(dataset='QM9', dim=128, n_layer=6, cutoff_l=5.0, cutoff_g=5.0)
pamnet = models.PAMNet(cfg).to(dev)
wells = Harmonic(torch.full((B_GRAPHS,), 2.0, device=dev), data.pos.clone())
masses = MASS[data.x.long()].contiguous()
seeds = torch.arange(B_GRAPHS, dtype=torch.int64, device=dev)
common = dict(masses=masses, kT=0.025, gamma=0.1, seed=seeds)
LONG, SHORT = 210, 10
variants = {}
for name, model in (('QM9 PAMNet', pamnet), ('harmonic wells', wells)):
    for steps in (LONG, SHORT):
        variants[(name, 'plain', steps)] = lambda model=model, steps=steps: M.run(model, data, steps, 0.1, **common)
        if not args.plain:
            variants[(name, 'bias', steps)] = lambda model=model, steps=steps: M.run(model, data, steps, 0.1, bias=make_bias(), **common)
last = {k: fn() for k, fn in variants.items()}
t = {k: [] for k in variants}
for _ in range(args.rounds):
    for k, fn in variants.items():
        t[k].append(timed(fn))
print('(ii) md.run, B = %d (%d atoms), %d rounds; ms per iteration = (a %d-step run - a %d-step run) / %d'
      % (B_GRAPHS, data.pos.size(0), args.rounds, LONG, SHORT, LONG - SHORT))
per = lambda name, kind: [(x - y) / (LONG - SHORT) for x, y in zip(t[(name, kind, LONG)], t[(name, kind, SHORT)])]
for name in ('QM9 PAMNet', 'harmonic wells'):
    report(name + ', md.run iteration', per(name, 'plain'), 'ms', 1.0)
    if not args.plain:
        report(name + ', md.run(bias=...) iteration', per(name, 'bias'), 'ms', 1.0)
        report('  minus md.run', [a - b for a, b in zip(per(name, 'bias'), per(name, 'plain'))], 'ms', 1.0)
        r = last[(name, 'bias', LONG)]
        print('      %d steps: failed %d' % (LONG, int(r.failed.sum())))
