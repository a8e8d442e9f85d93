"""Loss and a hash of the whole flat gradient of one training step (d = 128), one line per launch plan of the layer-stack
engine, plus the hash of an inference forward: same-bits check between two builds of the library (PAMNET_HIP_LIB=<other .so>)
or two settings of a switch.  Run on the GPU box: python tools/hash_step.py"""
import sys, hashlib, torch, os
import numpy as np
repo=os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, repo); sys.path.insert(0, os.path.join(repo,'physics-aware-multiplex-gnn_amd'))
import models
from pamnet_amd import synth
from pamnet_amd.train import Trainer
dev=torch.device('cuda:0')
def qm9_nodes(n_nodes, seed=4):
    """A QM9-schema batch of exactly n_nodes atoms: whole molecules while the next one fits, single atoms between the first ones
    for the rest (as tests/test_hip_model.py _qm9_batch_of)."""
    mols, n = [], 0
    while n + synth.qm9_molecule(seed, len(mols))['x'].shape[0] <= n_nodes:
        mols.append(synth.qm9_molecule(seed, len(mols))); n += mols[-1]['x'].shape[0]
    graphs = []
    for i, m in enumerate(mols):
        if i < n_nodes - n:
            graphs.append(dict(x=np.array([i % 5], np.float32), pos=np.zeros((1, 3), np.float32),
                               edge_index=np.zeros((2, 0), np.int64), y=np.float32(0.25 * (i % 7) - 0.75)))
        graphs.append(m)
    b = synth.collate(graphs)
    assert b.x.numel() == n_nodes
    return b
qm9=lambda L: models.Config(dataset='QM9', dim=128, n_layer=L, cutoff_l=5.0, cutoff_g=5.0)
pdb=lambda L: models.Config(dataset='PDBbind', dim=128, n_layer=L, cutoff_l=2.0, cutoff_g=6.0)
CASES=[('QM9', models.PAMNet, qm9(3), lambda: synth.qm9_batch(24,0,7)),                                      # riders
       ('PDBbind', models.PAMNet, pdb(2), lambda: synth.pdbbind_batch(3,0,2,n_pocket=60,n_ligand=12)),
       ('qm9_n2817', models.PAMNet, qm9(3), lambda: qm9_nodes(2817)),                                        # bf16x6, no riders
       ('qm9_n4097', models.PAMNet, qm9(3), lambda: qm9_nodes(4097)),                                        # lean
       ('qm9_n4097_l1', models.PAMNet, qm9(1), lambda: qm9_nodes(4097)),                                     # single-pair backward
       ('qm9s_n4097', models.PAMNet_s, qm9(2), lambda: qm9_nodes(4097)),                                     # pairs only
       ('pdbbind_b12', models.PAMNet, pdb(2), lambda: synth.collate([synth.pdbbind_complex(1,i) for i in range(12)]))]   # E_g >= 131072
for name, cls, cfg, make in CASES:
    torch.manual_seed(3)
    b=make().to(dev)
    model=cls(cfg).to(dev)
    tr=Trainer(model, loss='l1', max_grad_norm=None, ema_decay=None, lr=1e-3)
    loss=tr.forward_backward(b); torch.cuda.synchronize()
    g=model._graph_cache
    print('HASH', name, hashlib.sha256(tr.fp.grad.cpu().numpy().tobytes()).hexdigest()[:16], float(loss), 'n=%d eg=%d' % (g.n, g.glob.m))
    if name in ('QM9', 'qm9_n4097'):
        with torch.no_grad():
            out=model(b)
        torch.cuda.synchronize()
        print('HASH', name+'_nograd', hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()[:16], float(out.abs().sum()))
    del tr, model, b
    torch.cuda.empty_cache()
