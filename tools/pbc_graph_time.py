"""Host time of graph construction for a periodic batch, builder route against step-by-step route, at the case-4 batch of
profiles/pbc_graph_build.txt: synth.qm9_batch(0, 0, 16) without its bond list (16 molecules, 295 atoms) at cutoff_l 1.7, cutoff_g
5.0, every molecule in a 40 A cube (nothing wraps: the same edge sets with and without `cell`).  Three routes of
graph.build_graph(need_grad=True):
  cell, builder        mol_local=True:  cell table, pamnet_mol_graph_pbc_count/fill_i32, one host round trip
  cell, step-by-step   mol_local=None:  cell table, two searches, one host round trip, fills, angle fill, transposes
  no cell, default     mol_local=None:  pamnet_mol_graph_free_count/fill_i32
Host clock around a device synchronise; the routes interleaved call by call in one process, --calls each after --warmup; median /
p5 / p95 per route and the same-session ratio builder / step-by-step.  Run on the GPU box: python tools/pbc_graph_time.py"""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--calls', type=int, default=300)
ap.add_argument('--warmup', type=int, default=30)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'physics-aware-multiplex-gnn_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from pamnet_amd import graph as G, lib, synth  # noqa: E402

dev = torch.device('cuda:0')
lib.load()
b = synth.qm9_batch(0, 0, 16)
x, batch, pos = b.x.to(dev), b.batch.to(dev), b.pos.to(dev)
cell = (torch.eye(3) * 40.0).expand(16, 3, 3).contiguous().to(dev)


def build(cell_, mol_local):
    return G.build_graph('QM9', 1.7, 5.0, 'source_to_target', x, batch, pos, None, num_graphs=16, n_types=5, need_grad=True,
                         cell=cell_, mol_local=mol_local)


routes = [('cell, builder (mol_local=True)', lambda: build(cell, True)),
          ('cell (periodic, step-by-step)', lambda: build(cell, None)),
          ('no cell, default (mol-local)', lambda: build(None, None))]
calls, real = [], lib.call


def rec(name, *a):
    calls.append(name)
    return real(name, *a)


lib.call = rec                                                       # which route each variant really takes, once
took = []
for name, fn in routes:
    del calls[:]
    g = fn()
    took.append([c.replace('pamnet_', '') for c in calls if 'mol_graph' in c or 'radius' in c or 'cell_prepare' in c])
lib.call = real
assert took[0] == ['cell_prepare_f64', 'mol_graph_pbc_count_i32', 'mol_graph_pbc_fill_i32'], took[0]
assert 'radius_pbc_fill_i32' in took[1] and not [c for c in took[1] if 'mol_graph' in c], took[1]
assert took[2] == ['mol_graph_free_count_i32', 'mol_graph_free_fill_i32'], took[2]
print('case-4 batch: 16 molecules, %d atoms, global edges %d, local edges %d, triplet + pair rows %d' % (g.n, g.glob.m, g.loc.m, g.tp.m))

times = [[] for _ in routes]
for k in range(args.warmup + args.calls):
    for r, (name, fn) in enumerate(routes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= args.warmup:
            times[r].append(1e6 * (time.perf_counter() - t0))
med = []
for (name, _), t in zip(routes, times):
    t = np.asarray(t)
    med.append(float(np.median(t)))
    print('case-4 batch                 %-34s median  %7.1f us   p5  %7.1f   p95  %7.1f   (n = %d)'
          % (name, med[-1], np.percentile(t, 5), np.percentile(t, 95), t.size))
print('same session, interleaved: builder / step-by-step with cell = %.3f; builder with cell / builder without = %.3f'
      % (med[0] / med[1], med[0] / med[2]))
