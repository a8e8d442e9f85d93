"""The small batches the graph-construction tests share (tests/test_graph_engine.py, tests/test_graph_routes.py): one per
schema, with the keywords build_graph takes for it."""
import numpy as np


def case(kind, dev):
    from pamnet_amd import synth
    if kind == 'qm9':
        b = synth.qm9_batch(41, 0, 24)
        return b.to(dev), dict(dataset='QM9', cutoff_l=5.0, cutoff_g=5.0, flow='source_to_target', n_types=5)
    if kind == 'qm9_ragged':
        b = synth.collate([synth.qm9_molecule(3, 0),
                           dict(x=np.array([1], np.float32), pos=np.zeros((1, 3), np.float32),
                                edge_index=np.zeros((2, 0), np.int64), y=np.float32(0.1)),
                           synth.qm9_molecule(3, 1),
                           dict(x=np.array([0, 2], np.float32), pos=np.array([[0, 0, 0], [1.1, 0, 0]], np.float32),
                                edge_index=np.array([[0, 1], [1, 0]], np.int64), y=np.float32(0.2))])
        return b.to(dev), dict(dataset='QM9', cutoff_l=5.0, cutoff_g=5.0, flow='source_to_target', n_types=5)
    if kind == 'pdbbind':
        b = synth.pdbbind_batch(9, 0, 3, n_pocket=90, n_ligand=16)
        return b.to(dev), dict(dataset='PDBbind', cutoff_l=2.0, cutoff_g=6.0, flow='source_to_target', n_types=None)
    flow = 'target_to_source' if kind == 'rna_t2s' else 'source_to_target'
    b = synth.collate([synth.rna_chain(5, i, n_nodes=180 + 70 * i) for i in range(3)])
    return b.to(dev), dict(dataset='rna_x', cutoff_l=2.6, cutoff_g=20.0, flow=flow, n_types=3)
