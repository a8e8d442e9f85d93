"""Device time of the periodic geometry backward with and without the virial, entry points called directly on built graphs:
  twin:   pamnet_pos_bwd_pbc_f32 (dpos) -- of this build and, with --parent-lib, of another build (the parent commit's)
  virial: pamnet_pos_bwd_pbc_virial_f32 (dpos + dstrain)
at two shapes: 'c' = 300 + 2 + 37 atoms in three cells (tests/test_pbc_virial.py's case c in kind), 'b128' = 128 cells of 32 atoms
(4096 atoms).  Every figure: device events around --reps back-to-back calls, the variants alternating inside each of --rounds
rounds; median / min / max of the per-call time over the rounds.  Run on the GPU box: python tools/pbc_virial_time.py
[--parent-lib libpamnet_hip.so of the parent commit]."""
import argparse
import ctypes
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--parent-lib', default=None)
ap.add_argument('--reps', type=int, default=200)
ap.add_argument('--rounds', type=int, default=9)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'physics-aware-multiplex-gnn_amd'))

import torch  # noqa: E402
from pamnet_amd import graph as G, lib  # noqa: E402

dev = torch.device('cuda:0')
TWIN, VIRIAL = 'pamnet_pos_bwd_pbc_f32', 'pamnet_pos_bwd_pbc_virial_f32'


def scatter(gen, n, cell, min_sep=0.8):
    cell = torch.tensor(cell, dtype=torch.float64)
    inv = torch.linalg.inv(cell)
    pts = torch.empty((0, 3), dtype=torch.float64)
    while pts.size(0) < n:
        p = torch.rand(3, generator=gen, dtype=torch.float64) @ cell
        if pts.size(0):
            d = p - pts
            d = d - torch.round(d @ inv) @ cell
            if float(d.pow(2).sum(-1).min()) < min_sep ** 2:
                continue
        pts = torch.cat([pts, p[None]])
    return pts


def shape(name):
    gen = torch.Generator().manual_seed(11)
    cube = [[10.5, 0.0, 0.0], [0.0, 10.5, 0.0], [0.0, 0.0, 10.5]]
    if name == 'c':
        cells = [[[11.5, 0.0, 0.0], [2.0, 11.5, 0.0], [-1.5, 1.75, 11.5]], cube,
                 [[10.5, 0.0, 0.0], [0.0, 12.0, 0.0], [0.0, 0.0, 11.0]]]
        counts = [300, 2, 37]
    else:
        cells, counts = [cube] * 128, [32] * 128
    pos = torch.cat([scatter(gen, n, c) for n, c in zip(counts, cells)]).float()
    batch = torch.cat([torch.full((n,), k, dtype=torch.long) for k, n in enumerate(counts)])
    x = torch.randint(0, 5, (batch.numel(),), generator=gen).float()
    return x, batch, pos, torch.tensor(cells, dtype=torch.float32)


parent = None
if args.parent_lib:
    lib.load()                                                   # (first: one HIP runtime per process, torch's)
    parent = getattr(ctypes.CDLL(args.parent_lib), TWIN)
    parent.argtypes, parent.restype = lib.declared_functions()[TWIN], ctypes.c_int

for name in ('c', 'b128'):
    x, batch, pos, cell = shape(name)
    g = G.build_graph('QM9', 2.0, 5.0, 'source_to_target', x.to(dev), batch.to(dev), pos.to(dev), None,
                      num_graphs=int(cell.size(0)), n_types=5, cell=cell.to(dev), need_grad=True)
    n, ng, eg, el, tp = g.n, g.n_graphs, g.glob.m, g.loc.m, g.tp.m
    torch.manual_seed(2)
    ddg, ddl, dang = torch.randn(eg, device=dev), torch.randn(el, device=dev), torch.randn(tp, device=dev)
    P, st = lib.ptr, lib.stream_of(g.pos)
    work = torch.empty(3 * max(el, 1), dtype=torch.float64, device=dev)
    dpos, dpos_v, dpos_p = (torch.empty((n, 3), device=dev) for _ in range(3))
    atom_work = torch.empty((n, 9), dtype=torch.float64, device=dev)
    dstrain = torch.empty((ng, 9), device=dev)
    head = [P(g.pos), P(g.cell_tab), P(g.node_graph), n,
            P(g.glob.ptr), P(g.glob.row_of), P(g.glob.col), P(g.glob_T.ptr), P(g.glob_T.perm), P(ddg), eg,
            P(g.loc.ptr), P(g.loc.row_of), P(g.loc.col), P(g.loc_T.ptr), P(g.loc_T.perm), P(ddl), el,
            P(g.tp.ptr), P(g.tp.row_of), P(g.tp.col), P(g.tp_kind), P(g.tp_T.ptr), P(g.tp_T.perm), P(dang), tp, P(work)]
    variants = {'twin': lambda: lib.call(TWIN, *head, P(dpos), st),
                'virial': lambda: lib.call(VIRIAL, *head, P(dpos_v), P(g.gptr), ng, P(atom_work), P(dstrain), st)}
    if parent is not None:
        def parent_twin():
            rc = parent(*head, P(dpos_p), st)
            assert rc == 0, rc
        variants['parent twin'] = parent_twin
    for fn in variants.values():                                  # warm-up: code objects loaded, every buffer touched
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    assert torch.equal(dpos, dpos_v) and (parent is None or torch.equal(dpos, dpos_p))
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.reps):
                fn()
            e.record()
            torch.cuda.synchronize()
            times[k].append(1e3 * s.elapsed_time(e) / args.reps)
    print('SHAPE %s: atoms %d graphs %d global edges %d local edges %d triplet/pair rows %d; dpos equal in every variant'
          % (name, n, ng, eg, el, tp), flush=True)
    for k, v in times.items():
        print('  %-12s median_us %8.2f  min_us %8.2f  max_us %8.2f  (%d rounds x %d calls)'
              % (k, statistics.median(v), min(v), max(v), len(v), args.reps), flush=True)
