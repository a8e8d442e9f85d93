"""A hash of every output array of the geometry kernels (csrc/graph.hip radius searches, cell table, image box, triplet fill;
csrc/forces.hip position backward), one line per case: same-bits check between two builds of the library
(PAMNET_HIP_LIB=<other .so>).  The cases call the pamnet_amd.graph wrappers, so the step-by-step kernels run whatever route
build_graph would take; sizes are the smallest that reach each launch form.  Run on the GPU box: python tools/hash_geometry.py"""
import sys, hashlib, torch, os
repo=os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, repo); sys.path.insert(0, os.path.join(repo,'physics-aware-multiplex-gnn_amd'))
from pamnet_amd import graph as G, lib
dev=torch.device('cuda:0')
P=lib.ptr
CUT_L, CUT_G = 2.0, 5.0
def H(name, *arrays):
    """sha256 over the raw bytes of the arrays, in order"""
    h=hashlib.sha256()
    for a in arrays:
        h.update(a.detach().contiguous().cpu().numpy().tobytes())
    print('HASH', name, h.hexdigest()[:16], ' '.join(str(tuple(a.shape)) for a in arrays))
def atoms(counts, side, seed):
    """counts[g] points uniform in a cube of `side` per graph (fp32), the batch vector (long) and the graphs' ranges (int32)"""
    gen=torch.Generator().manual_seed(seed)
    pos=torch.cat([torch.rand(n, 3, generator=gen) * side for n in counts] + [torch.zeros(0, 3)]).float()
    batch=torch.cat([torch.full((n,), g, dtype=torch.long) for g, n in enumerate(counts)] + [torch.zeros(0, dtype=torch.long)])
    gptr=torch.tensor([0] + list(counts)).cumsum(0).to(torch.int32)
    return pos.to(dev), batch.to(dev), gptr.to(dev)
def boxes(*sides):
    """orthorhombic cells [G, 3, 3] from (a, b, c) triples"""
    return torch.stack([torch.diag(torch.tensor(s, dtype=torch.float32)) for s in sides]).to(dev)
def word():
    return torch.zeros(1, dtype=torch.int32, device=dev)

# ---- radius count + fill: thread form (n < 96 graphs), wave form, capped rows in both, open space and minimum image
def radius(name, counts, side, max_nb=0, cell=None):
    pos, batch, gptr=atoms(counts, side, seed=len(counts) + sum(counts))
    ng=batch.to(torch.int32).contiguous()
    flag=word()
    tab=None if cell is None else G.cell_table(cell, CUT_G, flag)
    ptr=G.radius_count(pos, ng, gptr, CUT_G, max_nb, flag, cell_tab=tab)
    rows=[]
    ptr, nbr, dist=G.radius_fill(pos, ng, gptr, CUT_G, ptr, int(ptr[-1]), rows_out=rows, max_neighbors=max_nb, cell_tab=tab)
    H(name, ptr, nbr, dist, rows[0], flag)
for tag, cell_of in (('open', lambda k: None), ('pbc', lambda k: boxes(*[(11.0, 12.0, 13.0)] * k))):
    radius('radius_thread_' + tag, (1, 2, 19), 9.0, cell=cell_of(3))
    radius('radius_wave_' + tag, (97, 130), 11.0, cell=cell_of(2))
    radius('radius_cap8_wave_' + tag, (130,), 11.0, max_nb=8, cell=cell_of(1))
    radius('radius_cap8_thread_' + tag, (130, 1), 11.0, max_nb=8, cell=cell_of(2))

# ---- all-image radius: boxes (1, 1, 0) and (2, 1, 1); a single atom that finds its own images only
def radius_img(name, max_nb=0):
    pos, batch, gptr=atoms((23, 17, 1), 4.0, seed=5)
    ng=batch.to(torch.int32).contiguous()
    cell=boxes((6.0, 6.0, 20.0), (4.0, 7.0, 8.0), (4.0, 4.5, 9.0))
    pbc=torch.tensor([[1, 1, 0], [1, 1, 1], [1, 1, 1]], dtype=torch.bool, device=dev)
    flag=word()
    tab=G.cell_table(cell, 1.5, flag, pbc)
    box=G.cell_images(tab, CUT_G, flag, pbc)
    ptr=G.radius_img_count(pos, tab, box, ng, gptr, CUT_G, max_nb, flag)
    ptr, nbr, dist, row_of, img=G.radius_img_fill(pos, tab, box, ng, gptr, CUT_G, ptr, int(ptr[-1]), max_neighbors=max_nb)
    H(name, box, ptr, nbr, dist, row_of, img, flag)
radius_img('radius_img')
radius_img('radius_img_cap8', max_nb=8)

# ---- cell table and image box: periodic (triclinic), slab, wire, all-open, singular, too small; pbc None / all true / mixed
CELLS=torch.tensor([[[12.0, 0.0, 0.0], [2.0, 13.0, 0.0], [1.0, -3.0, 14.0]],
                    [[11.0, 1.0, 0.0], [0.5, 12.0, 0.0], [3.0, 3.0, 1.0]],
                    [[0.0, 0.0, 0.0], [7.0, 7.0, 0.0], [0.3, 0.2, 15.0]],
                    [[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 0.0]],
                    [[10.0, 0.0, 0.0], [20.0, 0.0, 0.0], [0.0, 0.0, 12.0]],
                    [[3.0, 0.0, 0.0], [0.0, 3.0, 0.0], [0.0, 0.0, 3.0]]]).to(dev)
MIXED=torch.tensor([[1, 1, 1], [1, 1, 0], [0, 0, 1], [0, 0, 0], [1, 1, 1], [1, 1, 1]], dtype=torch.bool, device=dev)
for tag, pbc in (('none', None), ('all_true', torch.ones_like(MIXED)), ('mixed', MIXED), ('tuple_slab', (True, True, False))):
    flag_t, flag_b=word(), word()
    tab=G.cell_table(CELLS, CUT_G, flag_t, pbc)
    box=G.cell_images(tab, CUT_G, flag_b, pbc)
    H('cells_' + tag, tab, flag_t, box, flag_b)

# ---- triplet fill and position backward on graphs of the step-by-step route
def build(counts, side, cutoff_l=CUT_L, n_graphs=None, **kw):
    """bond-free QM9-schema graph; n_graphs > len(counts): the last graphs have no atoms"""
    pos, batch, _=atoms(counts, side, seed=7 + len(counts))
    x=(torch.arange(batch.numel(), device=dev) % 5).float()
    return pos, G.build_graph('QM9', cutoff_l, CUT_G, 'source_to_target', x, batch, pos, None,
                              num_graphs=n_graphs or len(counts), n_types=5, mol_local=False, need_grad=True, **kw)
def triplets(name, pos, g):
    for wt in (0, 1):
        loc=g.loc
        tp_ptr, _=G._triplet_ptr(loc.ptr, loc.col, loc.row_of, wt)
        tot=int(tp_ptr[-1])
        idx, edge, kind=(torch.full((tot,), -7, dtype=torch.int32, device=dev) for _ in range(3))
        angle=torch.full((tot,), -7.0, device=dev)
        tab=getattr(g, 'cell_tab', None)
        G._call_in_cell('pamnet_triplet_fill_f32', 'pamnet_triplet_fill_pbc_f32', pos, None if tab is None else (tab, g.node_graph),
                        P(loc.ptr), P(loc.col), P(loc.row_of), loc.m, wt, P(tp_ptr), P(idx), P(edge), P(angle), P(kind), tot,
                        lib.stream_of(pos))
        H('%s_wt%d' % (name, wt), tp_ptr, idx, edge, angle, kind)
def pos_bwd(name, pos, g, virial=False):
    """the entry point of g's space on seeded cotangents; work arrays start from a sentinel, so what a launch leaves alone hashes too"""
    n, glob, eg, loc, el, trip, tp=G._index_lists(g)
    gen=torch.Generator().manual_seed(13)
    d_dg, d_dl, d_ang=(torch.randn(m, generator=gen).to(dev) for m in (eg, el, tp))
    work=torch.full((3 * max(el, 1),), -7.0, dtype=torch.float64, device=dev)
    dpos=torch.full((n, 3), -7.0, device=dev)
    tab, img=getattr(g, 'cell_tab', None), getattr(g, 'img_g', None)
    space=() if tab is None else (tab, g.node_graph)
    if img is not None:
        glob=glob[:3] + (img,) + glob[3:]
    sym='pamnet_pos_bwd%s%s_f32' % ('' if tab is None else ('_pbc' if img is None else '_img'), '_virial' if virial else '')
    args=[P(pos), *map(P, space), n, *map(P, glob), P(d_dg), eg, *map(P, loc), P(d_dl), el, *map(P, trip), P(d_ang), tp, P(work), P(dpos)]
    out=[dpos, work]
    if virial:
        atom_work=torch.full((9 * max(n, 1),), -7.0, dtype=torch.float64, device=dev)
        dstrain=torch.full((g.n_graphs, 9), -7.0, device=dev)
        args+=[P(g.gptr), g.n_graphs, P(atom_work), P(dstrain)]
        out+=[dstrain, atom_work]
    lib.call(sym, *args, lib.stream_of(pos))
    H(name + ('_virial' if virial else ''), *out)
BIG=boxes(*[(10.5, 11.0, 11.5)] * 3)                   # heights above 2 * CUT_G: the minimum-image graphs
THIN=boxes(*[(6.0, 4.5, 7.0)] * 3)                    # heights above 2 * CUT_L only: the all-image graphs
# atoms scattered over a cube of `side`: past the cell's faces in the periodic cases, so bonds and edges cross them
for name, big, side, kw in (('open', 30, 6.0, {}), ('pbc', 120, 11.5, dict(cell=BIG)), ('img', 30, 5.0, dict(cell=THIN, cell_images='all'))):
    graphs={'': build((9, big, 5), side, **kw),                                         # (img: rows of more than 64 global edges)
            '_empty_graph': build((9, big // 2), side, n_graphs=3, **kw),               # graph 2 of 3 has no atoms
            '_el0': build((9, 14, 3), side, cutoff_l=0.05, **kw)}                       # no local edge, no triplet / pair row
    for tag, (pos, g) in graphs.items():
        if name != 'img' and tag != '_empty_graph':
            triplets('triplets_%s%s' % (name, tag), pos, g)
        pos_bwd('pos_bwd_%s%s' % (name, tag), pos, g)
        if name != 'open':
            pos_bwd('pos_bwd_%s%s' % (name, tag), pos, g, virial=True)
torch.cuda.synchronize()
