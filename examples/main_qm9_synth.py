#!/usr/bin/env python
"""The reference's QM9 driver loop (main_qm9.py:79-132) on the MI355X path, with QM9-schema synthetic molecules standing
in for the dataset (QM9 itself needs the RDKit-based reader + download, out of scope):

    python examples/main_qm9_synth.py --epochs 2 --train 2048 --val 256 --batch_size 128
    python -m torch.distributed.run --nproc-per-node 8 examples/main_qm9_synth.py ...      # molecule-sharded DP

Same hyper-parameters and schedule as the reference: Adam(lr, wd=0), warm-up over the first epoch then
ExponentialLR(0.9961697) stepped per iteration with the fractional epoch, clip_grad_norm_(1000), EMA(0.999) evaluated
under assign/resume, best-validation checkpoint of `model.state_dict()` (keys identical to the reference's).
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'physics-aware-multiplex-gnn_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from models import PAMNet, PAMNet_s, Config  # noqa: E402   (the drop-in for the reference's `models`)
from pamnet_amd import synth  # noqa: E402
from pamnet_amd.train import Trainer, WarmupExpLR, shard_range  # noqa: E402


def run_target(args, cfg, target, dev, world, rank):
    """The body of main_qm9.py:84-132 for one target."""
    model = (PAMNet if args.model == 'PAMNet' else PAMNet_s)(cfg).to(dev)
    # --freeze N: the embeddings and the first N layer pairs keep their values (fine-tuning); --accumulate K: one update per K
    # batches, on the mean over all of them (both default to the reference's recipe)
    groups = [{'params': ['embeddings'] + ['%s.%d.*' % (s, k) for k in range(args.freeze) for s in ('global_layer', 'local_layer')],
               'frozen': True}] if args.freeze > 0 else None
    trainer = Trainer(model, lr=args.lr, weight_decay=args.wd, ema_decay=0.999, max_grad_norm=1000.0, world_size=world,
                      param_groups=groups, accumulate=args.accumulate)
    if rank == 0:
        print('Target %d. Number of model parameters: ' % target, sum(v.numel() for v in model.state_dict().values()))    # (the reference's shapes: a dim without a kernel family of its own is held zero-padded)
    gb = args.batch_size
    steps_per_epoch = args.train // gb
    sched = WarmupExpLR(args.lr, gamma=0.9961697, steps_per_epoch=args.train / gb)

    lo, hi = shard_range(gb, rank, world)
    if args.resident:
        # the dataset lives on the device (QM9 itself: 134 k molecules, ~60 MB); batches are collated there by one gather
        # launch and carry their data-dependent sizes, so a step issues no device->host read (pamnet_amd/store.py)
        import numpy as np
        from pamnet_amd.store import MoleculeStore
        col = target + 5 if target in (7, 8, 9, 10) else target      # main_qm9.py:60-66
        labels = synth.qm9_label_table(args.seed, 0, args.train)[:, col]
        mols = []
        for i in range(args.train):
            m = synth.qm9_molecule(args.seed, i)
            m['y'] = np.float32(labels[i])
            mols.append(m)
        store = MoleculeStore(mols, dev).prepare_for(model)
        order = {'epoch': -1, 'perm': None}

        def train_batch(step, epoch=0):                             # this rank's shard of global batch `step`
            if order['epoch'] != epoch:                             # DataLoader(shuffle=True): same permutation on every rank
                order['epoch'], order['perm'] = epoch, np.random.default_rng(args.seed + epoch).permutation(args.train)
            return store.collate(order['perm'][step * gb + lo:step * gb + hi])
    else:
        def train_batch(step, epoch=0):
            return synth.qm9_batch(args.seed, step * gb + lo, hi - lo, target=target).to(dev)

    vlo, vhi = shard_range(args.val, rank, world)
    val = [synth.qm9_batch(args.seed + 1, args.train + vlo + i, min(gb, vhi - vlo - i), target=target).to(dev)
           for i in range(0, vhi - vlo, gb)]

    best = None
    for epoch in range(args.epochs):
        model.train()
        loss_sum = torch.zeros((), device=dev)
        nxt = train_batch(0, epoch)
        for step in range(steps_per_epoch):
            data, nxt = nxt, (train_batch(step + 1, epoch) if step + 1 < steps_per_epoch else None)
            # the LR the reference's optimiser has AT this step (scheduler stepped after optimizer.step, main_qm9.py:112-114)
            loss = trainer.step(data, lr=sched.lr_for_step(epoch, step, steps_per_epoch), global_graphs=gb * args.accumulate,
                                next_data=nxt)
            loss_sum += loss.detach() * data.num_graphs
        if world > 1:
            dist.all_reduce(loss_sum)
        val_mae = trainer.evaluate(val)                            # under the EMA weights (main_qm9.py:29-37)
        if best is None or val_mae <= best:
            best = val_mae
            if args.save and rank == 0:
                torch.save(model.state_dict(), args.save if len(str(args.target)) < 3 else '%s.t%d' % (args.save, target))
        if rank == 0:
            print('Epoch: {:03d}, Train MAE: {:.7f}, Val MAE: {:.7f}'.format(epoch + 1, float(loss_sum) / args.train, val_mae))
    if rank == 0:
        print('Best Validation MAE:', best)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', default='PAMNet', choices=['PAMNet', 'PAMNet_s'])
    ap.add_argument('--epochs', type=int, default=2)
    ap.add_argument('--lr', type=float, default=1e-4)
    ap.add_argument('--wd', type=float, default=0.0)
    ap.add_argument('--n_layer', type=int, default=6)
    ap.add_argument('--dim', type=int, default=128)
    ap.add_argument('--batch_size', type=int, default=128, help='global batch (split over the ranks)')
    ap.add_argument('--cutoff_l', type=float, default=5.0)
    ap.add_argument('--cutoff_g', type=float, default=5.0)
    ap.add_argument('--train', type=int, default=2048, help='synthetic training molecules')
    ap.add_argument('--val', type=int, default=256)
    ap.add_argument('--seed', type=int, default=480)
    ap.add_argument('--target', default='7', help="index of the target (0-11; 7-10 read label columns 12-15 as in "
                    "main_qm9.py:60-66), or 'all': the 12 targets one after the other (BASELINE configs[2])")
    ap.add_argument('--save', default='')
    ap.add_argument('--freeze', type=int, default=0, help='freeze the embeddings and the first N layer pairs')
    ap.add_argument('--accumulate', type=int, default=1, help='batches per optimiser update (gradient accumulation); when the steps of an epoch are not a multiple of it, the '
                    'last partial sum carries over the evaluation into the next epoch\'s first update')
    ap.add_argument('--resident', action='store_true', help='keep the training set on the device and collate batches there '
                    '(pamnet_amd.store.MoleculeStore): no device->host read per step; shuffled every epoch')
    args = ap.parse_args()

    world, rank = int(os.environ.get('WORLD_SIZE', '1')), int(os.environ.get('RANK', '0'))
    dev = torch.device('cuda', int(os.environ.get('LOCAL_RANK', '0')))
    torch.cuda.set_device(dev)
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group('nccl', device_id=dev)
    cfg = Config(dataset='QM9', dim=args.dim, n_layer=args.n_layer, cutoff_l=args.cutoff_l, cutoff_g=args.cutoff_g)
    targets = list(range(12)) if args.target == 'all' else [int(args.target)]
    results = {}
    for target in targets:                                         # 12 independent scalar-output runs
        torch.manual_seed(args.seed)                               # identical initial weights on every rank
        results[target] = run_target(args, cfg, target, dev, world, rank)
    if rank == 0 and len(targets) > 1:
        print('Best Validation MAE per target:', {t: round(v, 6) for t, v in results.items()})
    if world > 1:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
