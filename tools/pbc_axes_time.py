"""Per-axis periodicity (data.pbc), two measurements for profiles/pbc_axes.txt:
  1. pamnet_cell_prepare_axes_f64 beside pamnet_cell_prepare_f64 on the cells of the periodic test batch (tests/test_pbc.py inputs
     'a': a 10.5 cube and a 10.5 x 12 x 11 box) and on the same two cells repeated to 4096 graphs, with pbc all True (the twin's
     arithmetic) and pbc = (True, True, False).
  2. the all-image search, count + fill (pamnet_radius_img_count/fill_i32), on a batch of slabs handed over with pbc = (True, True,
     False) and a zero third vector, against the same slabs handed over fully periodic with a 32 A third vector: candidates per
     row, and time.  The lists of the two are compared first.
Host clock around a device synchronise, the variants interleaved call by call in one process, --calls each after --warmup; median /
p5 / p95.  Run on the GPU box: python tools/pbc_axes_time.py"""
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
from pamnet_amd import graph as G, lib  # noqa: E402

dev = torch.device('cuda:0')
lib.load()
CUT_L, CUT_G = 2.0, 5.0


def timed(variants):
    times = [[] for _ in variants]
    for k in range(args.warmup + args.calls):
        for r, (name, fn) in enumerate(variants):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if k >= args.warmup:
                times[r].append(1e6 * (time.perf_counter() - t0))
    med = []
    for (name, _), t in zip(variants, times):
        t = np.asarray(t)
        med.append(float(np.median(t)))
        print('  %-58s median  %7.1f us   p5  %7.1f   p95  %7.1f   (n = %d)' % (name, med[-1], np.percentile(t, 5),
                                                                                np.percentile(t, 95), t.size))
    return med


# ---- 1. the table
two = torch.tensor([[[10.5, 0, 0], [0, 10.5, 0], [0, 0, 10.5]], [[10.5, 0, 0], [0, 12.0, 0], [0, 0, 11.0]]], dtype=torch.float32)
for reps in (1, 2048):
    cell = two.repeat(reps, 1, 1).to(dev).view(-1, 9).contiguous()
    ng = cell.size(0)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    all_true = torch.ones(ng, 3, dtype=torch.bool, device=dev)
    slab = torch.tensor([[True, True, False]], device=dev).expand(ng, 3).contiguous()
    assert torch.equal(G.cell_table(cell, CUT_G, flag), G.cell_table(cell, CUT_G, flag, all_true)) and int(flag) == 0
    print('cell table, %d graphs (one launch each; the result tensor is allocated inside the call):' % ng)
    timed([('pamnet_cell_prepare_f64', lambda: G.cell_table(cell, CUT_G, flag)),
           ('pamnet_cell_prepare_axes_f64, pbc all True', lambda: G.cell_table(cell, CUT_G, flag, all_true)),
           ('pamnet_cell_prepare_axes_f64, pbc (True, True, False)', lambda: G.cell_table(cell, CUT_G, flag, slab))])

# ---- 2. the all-image search on slabs
N_GRAPHS, N_ATOMS = 16, 64
gen = torch.Generator().manual_seed(0)
frac = torch.rand(N_GRAPHS * N_ATOMS, 3, generator=gen, dtype=torch.float64)
in_plane = torch.tensor([[9.0, 0.0, 0.0], [1.5, 9.0, 0.0]], dtype=torch.float64)
pos = (frac[:, :2] @ in_plane)
pos = torch.cat([pos, 8.0 * frac[:, 2:]], dim=1).float().to(dev)                      # z-spread 8 A < 16 - cutoff_g
batch = torch.arange(N_GRAPHS).repeat_interleave(N_ATOMS)
node_graph = batch.to(torch.int32).to(dev)
gptr = torch.arange(0, N_GRAPHS * N_ATOMS + 1, N_ATOMS, dtype=torch.int32, device=dev)


def cells(third):
    c = torch.cat([in_plane, torch.tensor([third], dtype=torch.float64)]).float()
    return c.expand(N_GRAPHS, 3, 3).contiguous().to(dev).view(-1, 9)


def prepared(third, pbc):
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    tab = G.cell_table(cells(third), CUT_L, flag, pbc)
    box = G.cell_images(tab, CUT_G, flag, pbc)
    ptr = G.radius_img_count(pos, tab, box, node_graph, gptr, CUT_G, 0, flag)
    total = int(ptr[-1])
    assert int(flag) == 0
    return tab, box, flag, total


def search(state):
    tab, box, flag, total = state
    ptr = G.radius_img_count(pos, tab, box, node_graph, gptr, CUT_G, 0, flag)
    return G.radius_img_fill(pos, tab, box, node_graph, gptr, CUT_G, ptr, total)


open_z = prepared([0.0, 0.0, 0.0], (True, True, False))
tall = prepared([0.0, 0.0, 32.0], None)
la, lb = search(open_z), search(tall)
assert all(torch.equal(u, v) for u, v in zip(la, lb)) and open_z[3] == tall[3]
for name, st in (('pbc = (True, True, False), third vector zero', open_z), ('fully periodic, third vector (0, 0, 32)', tall)):
    n_box = st[1][0].tolist()
    print('%s: box %s, candidates per row %d' % (name, n_box, N_ATOMS * int(np.prod([2 * k + 1 for k in n_box]))))
print('all-image search, count + fill: %d slabs of %d atoms, %d global edges (equal lists):' % (N_GRAPHS, N_ATOMS, open_z[3]))
med = timed([('pbc = (True, True, False)', lambda: search(open_z)), ('fully periodic, 32 A third vector', lambda: search(tall))])
print('same session, interleaved: per-axis / fully periodic = %.3f' % (med[0] / med[1]))
