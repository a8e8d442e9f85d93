"""What replica exchange costs on top of plain dynamics (profiles/remd.txt).  One process, the variants alternating inside each
round, device events:
  (i)   the exchange launch alone, pamnet_remd_exchange_f64 on synthetic energies: one ladder of 4 graphs, and 16 ladders of 8
        (16 QM9-schema molecules replicated 8 times: 128 graphs), us per call over `--calls` back-to-back calls, and the share of
        the tried pairs that were accepted;
  (ii)  the two split step launches of an exchange step -- pamnet_md_step_f32 with (kick_in 1, advance 0), then (0, 1) -- against
        the one fused launch (1, 1) they replace, on the same 128 graphs and synthetic gradients, us per call (per pair of calls);
  (iii) ms per iteration of remd.run(exchange_every = k), k = 10 and 100, against md.run on the same batch (QM9 B = 128 as 16
        ladders of 8, d = 128, L = 6, per-graph kT): the difference of a 210-step and a 10-step run over 200, so that set-up and
        the closing evaluation cancel; the 200 steps hold 20 exchange steps at k = 10 and 2 at k = 100.
md.run is the baseline: it is unchanged by the exchange.
Run on the GPU box: python tools/remd_time.py [--rounds N] [--calls N] [--launch-only]."""
import argparse
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=15)
ap.add_argument('--calls', type=int, default=200)
ap.add_argument('--launch-only', action='store_true', help='parts (i) and (ii) alone (for a kernel trace)')
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'physics-aware-multiplex-gnn_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import models  # noqa: E402
from pamnet_amd import graph as G, md as M, remd as R, synth  # noqa: E402

dev = torch.device('cuda:0')
torch.manual_seed(0)
MASS = torch.tensor([1.008, 12.011, 14.007, 15.999, 18.998], device=dev)     # H, C, N, O, F by the schema's type index
KT_LO, KT_HI = 0.025, 0.05


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
    print('  %-52s median_%s %8.3f  min_%s %8.3f  max_%s %8.3f' % (name, unit, statistics.median(v), unit, min(v), unit, max(v)),
          flush=True)


def ladders(molecules, replicas):
    b = R.replicate(synth.qm9_batch(0, 0, molecules), replicas).to(dev)
    kT = R.temperatures(KT_LO, KT_HI, replicas).repeat(molecules).to(dev)
    return b, kT


# ---- (i), (ii) the launches alone
def exchange_case(molecules, replicas):
    b, kT = ladders(molecules, replicas)
    count, n = b.num_graphs, b.pos.size(0)
    gptr, _ = G.csr_from_keys(b.batch.to(torch.int32).contiguous(), count)
    vel, state = M.new_state(n, count, dev, seed=1)
    M.init_velocities(vel, gptr, state['seed'], kT, state['ke'], MASS[b.x.long()].contiguous())
    ladder = R.new_ladder_state(kT, replicas, 7)
    energy = torch.from_numpy(np.random.RandomState(0).gamma(1.5 * n / count, size=count)).to(dev) * kT   # (about 3 N kT / 2 each)

    def run():
        for _ in range(args.calls):
            R.exchange(energy, vel, gptr, ladder, state['status'], state['ke'])
    return '%d ladder%s of %d, %d atoms' % (molecules, 's' if molecules > 1 else '', replicas, n), run, ladder


def step_case(split):
    b, kT = ladders(16, 8)
    count, n = b.num_graphs, b.pos.size(0)
    gptr, _ = G.csr_from_keys(b.batch.to(torch.int32).contiguous(), count)
    pos, de, mass = b.pos.clone(), 0.05 * torch.randn(n, 3, device=dev), MASS[b.x.long()].contiguous()
    vel, state = M.new_state(n, count, dev, seed=1)

    def run():
        for _ in range(args.calls):
            if split:
                M.md_step(pos, vel, de, gptr, state, 0.01, kT, 1.0, mass, None, 1, 0)
                M.md_step(pos, vel, de, gptr, state, 0.01, kT, 1.0, mass, None, 0, 1)
            else:
                M.md_step(pos, vel, de, gptr, state, 0.01, kT, 1.0, mass, None, 1, 1)
    return run, state


ex = [exchange_case(1, 4), exchange_case(16, 8)]
st = {'fused (1, 1)': step_case(False), 'split (1, 0) + (0, 1)': step_case(True)}
for _, run, _ in ex:
    run()
for run, _ in st.values():
    run()
t_ex, t_st = [[] for _ in ex], {k: [] for k in st}
for _ in range(args.rounds):
    for i, (_, run, _) in enumerate(ex):
        t_ex[i].append(timed(run))
    for k, (run, _) in st.items():
        t_st[k].append(timed(run))
print('(i) the exchange launch alone, %d back-to-back calls, %d rounds' % (args.calls, args.rounds))
for i, (name, _, ladder) in enumerate(ex):
    assert int(ladder['attempts'].min()) == args.calls * (args.rounds + 1)
    report('remd_exchange, ' + name, t_ex[i], 'us', 1000.0 / args.calls)
    print('      pairs tried %d, accepted %d' % (int(ladder['tried'].sum()), int(ladder['accepted'].sum())))
print('(ii) the step launches of an exchange step, 128 graphs, %d back-to-back calls, %d rounds' % (args.calls, args.rounds))
for k, (_, state) in st.items():
    assert int(state['status'].abs().max()) == 0 and int(state['steps'].min()) == args.calls * (args.rounds + 1)
    report('md_step ' + k, t_st[k], 'us', 1000.0 / args.calls)

if args.launch_only:
    sys.exit(0)

# ---- (iii) at the headline batch
cfg = models.Config(dataset='QM9', dim=128, n_layer=6, cutoff_l=5.0, cutoff_g=5.0)
model = models.PAMNet(cfg).to(dev)
data, kT = ladders(16, 8)
masses = MASS[data.x.long()].contiguous()
seeds = torch.arange(128, dtype=torch.int64, device=dev)
common = dict(masses=masses, gamma=0.1, seed=seeds)
LONG, SHORT = 210, 10
variants = {}
for steps in (LONG, SHORT):
    variants[('md', steps)] = lambda steps=steps: M.run(model, data, steps, 0.1, kT=kT, **common)
    for k in (10, 100):
        variants[(k, steps)] = lambda steps=steps, k=k: R.run(model, data, steps, 0.1, kT=kT, replicas=8, exchange_every=k, **common)
last = {}
for k, fn in variants.items():
    last[k] = fn()
t = {k: [] for k in variants}
for _ in range(args.rounds):
    for k, fn in variants.items():
        t[k].append(timed(fn))
print('(iii) QM9 B = 128 as 16 ladders of 8 (%d atoms), d = 128, L = 6, %d rounds' % (data.pos.size(0), args.rounds))
per = lambda a: [(x - y) / (LONG - SHORT) for x, y in zip(t[(a, LONG)], t[(a, SHORT)])]
report('md.run iteration', per('md'), 'ms', 1.0)
for k in (10, 100):
    report('remd.run iteration, exchange_every = %d' % k, per(k), 'ms', 1.0)
    report('  minus md.run', [a - b for a, b in zip(per(k), per('md'))], 'ms', 1.0)
    r = last[(k, LONG)]
    print('      %d steps: attempts %d, pairs tried %d, accepted %d, failed %d'
          % (LONG, int(r.attempts.max()), int(r.tried.sum()), int(r.accepted.sum()), int(r.failed.sum())))
