"""What vibrational analysis costs (profiles/vib.txt).  One process, the variants alternating inside each round, device events:
  (i)   the eigensolver launch alone, pamnet_sym_eig_f64 through vib.eigh on one random symmetric matrix of d = 9, 87 and 192 and
        on a batch of 128 matrices of d = 87: ms per call (the copy that restores the consumed input is timed beside it and
        subtracted), the sweeps taken, and us per round = (ms per call) / (sweeps x (m - 1));
  (ii)  the two bookkeeping launches at a QM9-sized batch of 128 graphs, pairs = 4: us per call over `--calls` back-to-back calls;
  (iii) vib.run on that batch, QM9 d = 128, L = 6, against the same number of bare evaluations (forward + torch.autograd.grad of
        the replicated batch), and the solver's share.
Run on the GPU box: python tools/vib_time.py [--rounds N] [--calls N] [--solver-only]."""
import argparse
import copy
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=9)
ap.add_argument('--calls', type=int, default=200)
ap.add_argument('--solver-only', action='store_true', help='part (i) alone (for a kernel trace)')
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'physics-aware-multiplex-gnn_amd'))

import torch  # noqa: E402
import models  # noqa: E402
from pamnet_amd import graph as G, synth, vib  # noqa: E402

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


def report(name, times, unit, scale, tail=''):
    v = [t * scale for t in times]
    print('  %-40s median_%s %9.3f  min_%s %9.3f  max_%s %9.3f%s' % (name, unit, statistics.median(v), unit, min(v), unit, max(v),
                                                                      tail), flush=True)


# ---- (i) the solver alone
def solver_case(d, count, reps):
    m = torch.randn(count, d, d, dtype=torch.float64, device=dev)
    master = (m + m.transpose(1, 2)).reshape(-1).contiguous()
    dims = torch.full((count,), d, dtype=torch.long, device=dev)
    zero = torch.zeros(1, dtype=torch.long, device=dev)
    dptr, moff = torch.cat([zero, dims.cumsum(0)]), torch.cat([zero, (dims * dims).cumsum(0)])
    a, v = master.clone(), torch.zeros_like(master)
    w = torch.zeros(count * d, dtype=torch.float64, device=dev)
    st, sw = torch.zeros(count, dtype=torch.int32, device=dev), torch.zeros(count, dtype=torch.int32, device=dev)

    def solve():
        for _ in range(reps):
            a.copy_(master)
            vib.eigh(a, moff, dptr, v=v, w=w, status=st, sweeps=sw)

    def restore():
        for _ in range(reps):
            a.copy_(master)
    return solve, restore, st, sw, reps


solver = {(9, 1): solver_case(9, 1, 20), (87, 1): solver_case(87, 1, 5), (192, 1): solver_case(192, 1, 3),
          (87, 128): solver_case(87, 128, 3)}
for solve, restore, st, sw, reps in solver.values():
    solve(), restore()
t_solve, t_copy = {c: [] for c in solver}, {c: [] for c in solver}
for _ in range(args.rounds):
    for c, (solve, restore, st, sw, reps) in solver.items():
        t_solve[c].append(timed(solve) / reps)
        t_copy[c].append(timed(restore) / reps)
print('(i) pamnet_sym_eig_f64 alone, tol 1e-15, %d rounds' % args.rounds)
for (d, count), (solve, restore, st, sw, reps) in solver.items():
    assert int(st.max()) == 0
    net = [a - b for a, b in zip(t_solve[(d, count)], t_copy[(d, count)])]
    sweeps = int(sw.max())
    rounds = sweeps * ((d + 1) // 2 * 2 - 1)
    report('%d x d = %d' % (count, d), net, 'ms', 1.0, '   sweeps %d (max), us per round %.2f' % (sweeps, 1000.0 * statistics.median(net) / rounds))
if args.solver_only:
    sys.exit(0)

# ---- (ii) the bookkeeping launches at a QM9-sized batch
PAIRS = 4
data = synth.qm9_batch(0, 0, 128).to(dev)
n, count = data.pos.size(0), int(data.num_graphs)
cfg = models.Config(dataset='QM9', dim=128, n_layer=6, cutoff_l=5.0, cutoff_g=5.0)
model = models.PAMNet(cfg).to(dev)
hs = vib.hessian(model, data, pairs=PAIRS)
gptr, _ = G.csr_from_keys(data.batch.to(torch.int32).contiguous(), count)
evaluations = (hs.d_max + PAIRS - 1) // PAIRS
pos0 = data.pos.detach().clone().contiguous()
pos_out = torch.empty(2 * PAIRS * n, 3, device=dev)
de = 0.05 * torch.randn(2 * PAIRS * n, 3, device=dev)
h = torch.zeros_like(hs.hessian)


def displace_calls():
    for i in range(args.calls):
        vib.displace(pos0, gptr, hs.fptr, hs.free_idx, PAIRS, i % evaluations, 0.01, pos_out)


def rows_calls():
    for i in range(args.calls):
        vib.hessian_rows(de, pos0, hs.fptr, hs.free_idx, hs.moff, PAIRS, i % evaluations, 0.01, h)


book = {'pamnet_vib_displace_f32': displace_calls, 'pamnet_vib_rows_f64': rows_calls}
for fn in book.values():
    fn()
tb = {k: [] for k in book}
for _ in range(args.rounds):
    for k, fn in book.items():
        tb[k].append(timed(fn))
print('(ii) the bookkeeping launches, %d graphs, %d atoms, pairs = %d (%d copies), largest d = %d; %d back-to-back calls'
      % (count, n, PAIRS, 2 * PAIRS, hs.d_max, args.calls))
for k in book:
    report(k, tb[k], 'us', 1000.0 / args.calls)

# ---- (iii) vib.run against the evaluations it wraps
rep = vib._replicated(data, data.batch, n, count, 2 * PAIRS, dev)
tiled = pos0.repeat(2 * PAIRS, 1)


def bare():
    for _ in range(evaluations):
        d = copy.copy(rep)
        d.pos = tiled.detach().requires_grad_(True)
        e = model(d)
        torch.autograd.grad(e.sum(), d.pos)


def solve_only():
    a = hs.hessian.clone()
    vib.eigh(a, hs.moff, hs.dptr, w=torch.zeros(int(hs.free_idx.numel()) * 3, dtype=torch.float64, device=dev))


variants = {'vib.run': lambda: vib.run(model, data, pairs=PAIRS), 'vib.hessian': lambda: vib.hessian(model, data, pairs=PAIRS),
            'bare evaluations': bare, 'solver': solve_only}
for fn in variants.values():
    fn()
tv = {k: [] for k in variants}
for _ in range(args.rounds):
    for k, fn in variants.items():
        tv[k].append(timed(fn))
print('(iii) %d graphs (%d atoms), QM9 d = 128, L = 6, pairs = %d: %d evaluations of %d graphs (%d atoms); ms per call, %d rounds'
      % (count, n, PAIRS, evaluations, 2 * PAIRS * count, 2 * PAIRS * n, args.rounds))
for k in variants:
    report(k, tv[k], 'ms', 1.0)
report('vib.run - bare evaluations', [a - b for a, b in zip(tv['vib.run'], tv['bare evaluations'])], 'ms', 1.0)
report('vib.hessian - bare evaluations', [a - b for a, b in zip(tv['vib.hessian'], tv['bare evaluations'])], 'ms', 1.0)
