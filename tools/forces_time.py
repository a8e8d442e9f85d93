"""Median CUDA-event times of the force paths at QM9 B = 128, d = 128, L = 6 (the headline batch), plain autograd:
  a: forward + E.sum().backward(), parameters only (positions without grad)
  b: the same step with pos.requires_grad (parameters and forces)
  c: forward + torch.autograd.grad(E.sum(), pos) (forces only)
  f: the forward of a alone (a - f: the backward)
Run on the GPU box: python tools/forces_time.py [--root TREE] [--modes abc] [--steps N].  --root: import the model from
another checkout (mode a of the parent commit)."""
import argparse
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--modes', default='abc')
ap.add_argument('--steps', type=int, default=100)
ap.add_argument('--warmup', type=int, default=10)
args = ap.parse_args()
sys.path.insert(0, args.root)
sys.path.insert(0, os.path.join(args.root, 'physics-aware-multiplex-gnn_amd'))

import torch  # noqa: E402
import models  # noqa: E402
from pamnet_amd import synth  # noqa: E402

dev = torch.device('cuda:0')
torch.manual_seed(0)
cfg = models.Config(dataset='QM9', dim=128, n_layer=6, cutoff_l=5.0, cutoff_g=5.0)
model = models.PAMNet(cfg).to(dev)
base = synth.qm9_batch(0, 0, 128).to(dev)


def step(mode):
    data = synth.Batch(**dict(base.__dict__))
    if mode in 'af':
        out = model(data)
        if mode == 'a':
            out.sum().backward()
        return
    data.pos = base.pos.detach().clone().requires_grad_(True)
    out = model(data)
    if mode == 'b':
        out.sum().backward()
    else:
        torch.autograd.grad(out.sum(), data.pos)


for mode in args.modes:
    for _ in range(args.warmup):
        model.zero_grad(set_to_none=True)
        step(mode)
    times = []
    for _ in range(args.steps):
        model.zero_grad(set_to_none=True)               # (as an optimiser loop does: autograd hands its gradients over)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        step(mode)
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    print('MODE %s median_ms %.3f min_ms %.3f max_ms %.3f steps %d' % (mode, statistics.median(times), min(times),
                                                                      max(times), len(times)), flush=True)
