"""Helpers of tests/test_hip_narrow_engine.py (plain module, no fixtures): the launch constants of the narrow-width
layer-stack engine (csrc/narrow_chain.h, csrc/narrow_engine.hip) restated and read back from the sources, the regimes its
grids and its reducer are in at a given batch, and QM9-schema batches of an exact atom count.

Nothing here touches the device: the graph of a batch is built by the test (pamnet_amd.graph.build_graph)."""
import os
import re

import numpy as np

from test_hip_narrow_walk import BLOCKS, BWD_WAVES, EW_BLOCKS, FWD_PER_CU, FWD_WAVES, WIDTHS, cap_bwd, cap_fwd, check_table

# ---- csrc/narrow_chain.h and csrc/narrow_engine.hip, restated ----------------------------------------------------------
CHW = 8                      # waves (16-row tiles) per chain workgroup: a row group is 16 * CHW = 128 rows
CHAIN_CAP = 512              # chain workgroups at most; beyond it `grp += gridDim.x` and later groups add into the partial row
MAXSEG = 32                  # destinations of one narrow_reduce_multi_kernel launch
NPB = 4                      # projection blocks a pre chain holds at most
RED_Y = 8                    # narrow_reduce_multi_kernel: dim3(64, 8), thread row y starts at partial row b = y
RED_GUARD, RED_STEP4, RED_STEP = 24, 32, 8      # `for (; b + 24 < nblk; b += 32)` (four loads), then `for (; b < nblk; b += 8)`
RESIDENT_MAX = 32            # tail_resident(d) = d <= 32: wg_reduce with a slot per wave; d = 64 takes turns
GROUP_ROWS = 16 * CHW

# destinations (`segs` of Reducer::take) in the order narrow_stack::bwd takes them for one layer pair
LOCAL_TAKES = ('tail', 'mlp2', 'qblocks', 'pre4')
GLOBAL_TAKES = ('tail', 'global', 'pre2')
SEGS = {'tail': 23, 'mlp2': 4, 'qblocks': 6, 'pre4': 6, 'global': 3, 'pre2': 4}

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, '..', 'physics-aware-multiplex-gnn_amd', 'csrc')
SOURCES = ('narrow_chain.h', 'narrow_engine.hip', 'narrow_core.h')


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def sources():
    return {name: source(name) for name in SOURCES}


def _one(text, name, pattern, want=1):
    found = re.findall(pattern, text)
    assert len(found) == want, ('%s: expected %d match(es) of %r, found %d -- a cap, a loop or a stride was reshaped: restate it in '
                                'tests/narrow_engine_cases.py, so that the sizes of the engine tests move with it'
                                % (name, want, pattern, len(found)))
    return found[0]


def ceil_div(a, b):
    return -(-a // b)


def chain_grid(m):
    want = ceil_div(ceil_div(m, 16), CHW)
    return max(1, min(want, CHAIN_CAP))


def bwd_row_grid(m, d):
    return max(1, min(ceil_div(ceil_div(m, 16), BWD_WAVES[d]), BLOCKS))


def fwd_row_grid(m, d):
    return max(1, min(ceil_div(ceil_div(m, 16), FWD_WAVES), BLOCKS * FWD_PER_CU[d]))


def tail_resident(d):
    return d <= RESIDENT_MAX


# ---- partial-row strides (floats) ----------------------------------------------------------------------------------------
def tail_stride(d):
    lin, mlp = d * d + d, 2 * d * d + 2 * d
    floats = lin + 4 * mlp + lin + 2 * d + 1             # TailRow<D>: L0, B1..B4, L5, heads [2 D + 1]
    return (floats + 3) & ~3


def pre_stride(d, nb):
    return (nb + 1) * d * d + d


def mlp2_stride(d):
    return 2 * d * d + 2 * d


def global_stride(d):
    return 2 * d * d + d


def qblock4_stride(d):
    return 4 * (d * d + d)


def check_sources(texts):
    """The constants above against the three sources (a dict name -> text); raises when a definition has another value or
    no longer has the form read here."""
    ch, en, co = texts['narrow_chain.h'], texts['narrow_engine.hip'], texts['narrow_core.h']
    check_table(co)                                                              # NARROW_BLOCKS, bwd_waves, fwd_per_cu, ew_grid
    _one(co, 'narrow_core.h', r'const int64_t want = \(tiles \+ waves - 1\) / waves;')
    _one(co, 'narrow_core.h', r'return \(int\)\(want < cap \? \(want > 0 \? want : 1\) : cap\);')
    assert int(_one(ch, 'narrow_chain.h', r'constexpr int CHW = (\d+);')) == CHW
    assert int(_one(ch, 'narrow_chain.h', r'constexpr int CHAIN_CAP = (\d+);')) == CHAIN_CAP
    assert int(_one(ch, 'narrow_chain.h', r'constexpr int MAXSEG = (\d+);')) == MAXSEG
    assert int(_one(ch, 'narrow_chain.h', r'constexpr int NPB = (\d+);')) == NPB
    _one(ch, 'narrow_chain.h', r'const int64_t want = \(\(m \+ 15\) / 16 \+ CHW - 1\) / CHW;')
    _one(ch, 'narrow_chain.h', r'return \(int\)\(want < 1 \? 1 : \(want > CHAIN_CAP \? CHAIN_CAP : want\)\);')
    assert int(_one(ch, 'narrow_chain.h', r'constexpr bool tail_resident\(int d\) \{ return d <= (\d+); \}')) == RESIDENT_MAX
    # the walk of the three chain kernels that own partial rows or outputs per row group
    _one(ch, 'narrow_chain.h', r'for \(int64_t grp = blockIdx\.x; grp \* CHW < ntiles; grp \+= gridDim\.x\) \{', 3)
    _one(ch, 'narrow_chain.h', r'const bool add = grp != \(int64_t\)blockIdx\.x;', 2)
    _one(ch, 'narrow_chain.h', r'const int64_t row0 = \(grp \* CHW \+ wave\) \* 16;', 3)
    # the reducer
    loop = _one(ch, 'narrow_chain.h', r'int b = y;\s*for \(; b \+ (\d+) < nblk; b \+= (\d+)\) \{')
    assert (int(loop[0]), int(loop[1])) == (RED_GUARD, RED_STEP4), loop
    assert int(_one(ch, 'narrow_chain.h', r'for \(; b < nblk; b \+= (\d+)\) s0 \+= src\[\(size_t\)b \* stride \+ p\];')) == RED_STEP
    for k, off in enumerate((0, 8, 16, 24)):
        _one(ch, 'narrow_chain.h', r's%d \+= src\[\(size_t\)%s \* stride \+ p\];' % (k, 'b' if off == 0 else r'\(b \+ %d\)' % off),
             2 if off == 0 else 1)                                               # (s0 also takes the tail loop's rows)
    _one(ch, 'narrow_chain.h', r's = \(s0 \+ s1\) \+ \(s2 \+ s3\);')
    assert int(_one(ch, 'narrow_chain.h', r'hipLaunchKernelGGL\(narrow_reduce_multi_kernel, dim3\(gx, S\.n\), dim3\(64, (\d+)\), 0, st, S\);')) == RED_Y
    _one(ch, 'narrow_chain.h', r'for \(int u = 1; u < %d; \+\+u\) s \+= part\[u\]\[x\];' % RED_Y)
    # Reducer::take
    _one(ch, 'narrow_chain.h', r'const int64_t need = \(\(int64_t\)nblk \* stride \+ 63\) & ~\(int64_t\)63;')
    _one(ch, 'narrow_chain.h', r'if \(need > cap \|\| segs > MAXSEG\) return PAMNET_EINVAL;')
    _one(ch, 'narrow_chain.h', r'if \(T\.S\.n \+ segs > MAXSEG \|\| used \+ need > cap\) \{')
    # strides
    _one(ch, 'narrow_chain.h', r'static constexpr int LIN = D \* D \+ D, MLP = 2 \* D \* D \+ 2 \* D;')
    _one(ch, 'narrow_chain.h', r'static constexpr int L0 = 0, B1 = LIN, B2 = B1 \+ MLP, B3 = B2 \+ MLP, B4 = B3 \+ MLP, L5 = B4 \+ MLP, H = L5 \+ LIN;')
    _one(ch, 'narrow_chain.h', r'static constexpr int FLOATS = H \+ 2 \* D \+ 1;')
    _one(ch, 'narrow_chain.h', r'static constexpr int STRIDE = \(FLOATS \+ 3\) & ~3;')
    _one(ch, 'narrow_chain.h', r'constexpr int npre_bwd_stride\(int d, int nb\) \{ return \(nb \+ 1\) \* d \* d \+ d; \}')
    _one(co, 'narrow_core.h', r'constexpr int nglobal_bwd_stride\(int d\) \{ return 2 \* d \* d \+ d; \}')
    _one(co, 'narrow_core.h', r'constexpr int nmlp2_bwd_stride\(int d\) \{ return 2 \* d \* d \+ 2 \* d; \}')
    _one(co, 'narrow_core.h', r'constexpr int nlinear_bwd_stride\(int d\) \{ return d \* d \+ d; \}')
    _one(co, 'narrow_core.h', r'constexpr int nqblock4_bwd_stride\(int d\) \{ return 4 \* nlinear_bwd_stride\(d\); \}')
    # the takes of narrow_stack::bwd: grid, stride and destinations of each
    _one(en, 'narrow_engine.hip', r'TRY\(R\.take\(grid, p\.stride, %d, &p\.partial\)\);' % SEGS['tail'])
    _one(en, 'narrow_engine.hip', r'TRY\(R\.take\(grid, p\.stride, p\.nb \+ 2, &p\.partial\)\);')
    _one(en, 'narrow_engine.hip', r'TRY\(R\.take\(bwd_row_grid\(m, d\), nglobal_bwd_stride\(d\), %d, &partial\)\);' % SEGS['global'])
    _one(en, 'narrow_engine.hip', r'TRY\(R\.take\(bwd_row_grid\(m, d\), nmlp2_bwd_stride\(d\), %d, &partial\)\);' % SEGS['mlp2'])
    _one(en, 'narrow_engine.hip', r'TRY\(R\.take\(bwd_row_grid\(m, d\), stride, %d, &partial\)\);' % SEGS['qblocks'])
    _one(en, 'narrow_engine.hip', r'const int grid = chain_grid\(p\.m\);', 2)
    assert SEGS['pre4'] == 4 + 2 and SEGS['pre2'] == 2 + 2
    # the arena the takes share (make_layout)
    _one(en, 'narrow_engine.hip', r'const int64_t chain = \(int64_t\)chain_grid\(n\) \* tail_stride\(\(int\)d\);')
    _one(en, 'narrow_engine.hip', r'const int64_t pre = \(int64_t\)chain_grid\(n\) \* npre_bwd_stride\(\(int\)d, NPB\);')
    _one(en, 'narrow_engine.hip', r'const int64_t erow = \(int64_t\)NARROW_BLOCKS \* nmlp2_bwd_stride\(\(int\)d\);')
    _one(en, 'narrow_engine.hip', r'const int64_t qb = \(int64_t\)NARROW_BLOCKS \* nqblock4_bwd_stride\(\(int\)d\);')
    _one(en, 'narrow_engine.hip', r'const int64_t pf = 2 \* \(chain \+ 64\) \+ 2 \* \(pre \+ 64\) \+ 2 \* \(erow \+ 64\) \+ \(qb \+ 64\);')
    _one(en, 'narrow_engine.hip', r'TRY\(R\.flush\(\)\);')


def partial_floats(n, d):
    """make_layout's arena of partial rows (csrc/narrow_engine.hip)."""
    chain, pre = chain_grid(n) * tail_stride(d), chain_grid(n) * pre_stride(d, NPB)
    erow, qb = BLOCKS * mlp2_stride(d), BLOCKS * qblock4_stride(d)
    return 2 * (chain + 64) + 2 * (pre + 64) + 2 * (erow + 64) + (qb + 64)


def pair_takes(n, eg, el, tp, d):
    """(name, nblk, stride, segs) of every Reducer::take of one layer pair, in the order of narrow_stack::bwd."""
    grid = chain_grid(n)
    sizes = {'tail': (grid, tail_stride(d)), 'mlp2': (bwd_row_grid(tp, d), mlp2_stride(d)),
             'qblocks': (bwd_row_grid(el, d), qblock4_stride(d)), 'pre4': (grid, pre_stride(d, 4)),
             'global': (bwd_row_grid(eg, d), global_stride(d)), 'pre2': (grid, pre_stride(d, 2))}
    return [(k,) + sizes[k] + (SEGS[k],) for k in LOCAL_TAKES + GLOBAL_TAKES]


def reducer_trace(n, eg, el, tp, d, pairs=1):
    """Reducer::take / flush of `pairs` layer pairs, restated: a list of ('take', name, offset, nblk) and ('flush', entries)
    events.  Raises where take would return PAMNET_EINVAL."""
    cap, used, entries, events = partial_floats(n, d), 0, 0, []
    for _ in range(pairs):
        for name, nblk, stride, segs in pair_takes(n, eg, el, tp, d):
            need = (nblk * stride + 63) & ~63
            assert need <= cap and segs <= MAXSEG, ('PAMNET_EINVAL', name, need, cap, segs)
            if entries + segs > MAXSEG or used + need > cap:
                events.append(('flush', entries, 'table' if entries + segs > MAXSEG else 'arena'))
                used = entries = 0
            events.append(('take', name, used, nblk))
            used += need
            entries += segs
        events.append(('flush', entries, 'pair'))
        used = entries = 0
    return events


def reducer_walk(nblk):
    """Per thread row y of narrow_reduce_multi_kernel: (passes of the four-load loop, passes of the tail loop, partial rows
    it adds).  Together the eight rows must add every partial row exactly once."""
    out = []
    for y in range(RED_Y):
        b, four, tail, rows = y, 0, 0, []
        while b + RED_GUARD < nblk:
            rows += [b, b + 8, b + 16, b + 24]
            b += RED_STEP4
            four += 1
        while b < nblk:
            rows.append(b)
            b += RED_STEP
            tail += 1
        out.append((four, tail, rows))
    seen = sorted(r for _, _, rows in out for r in rows)
    assert seen == list(range(nblk)), nblk
    return out


def chain_walk(n):
    """(workgroups, row groups, most groups one workgroup owns, rows of the last group)."""
    grid, groups = chain_grid(n), ceil_div(ceil_div(n, 16), CHW)
    return grid, groups, ceil_div(groups, grid), n - (groups - 1) * GROUP_ROWS


def regimes(n, eg, el, tp, d):
    """What the launches of one layer pair do at these sizes."""
    grid, groups, per_wg, last_rows = chain_walk(n)
    rows = {'eg': eg, 'el': el, 'tp': tp}
    return dict(chain_grid=grid, chain_groups=groups, chain_walks=per_wg > 1, last_group_rows=last_rows,
                bwd_grid={k: bwd_row_grid(m, d) for k, m in rows.items()},
                bwd_walks={k: m > cap_bwd(d) for k, m in rows.items()},
                fwd_grid={'n': fwd_row_grid(n, d), 'eg': fwd_row_grid(eg, d), 'el': fwd_row_grid(el, d), 'tp': fwd_row_grid(tp, d)},
                fwd_walks={k: m > cap_fwd(d) for k, m in dict(rows, n=n).items()},
                ew_strides=el * (d // 4) > EW_BLOCKS * 256)


# ---- batches -------------------------------------------------------------------------------------------------------------
CUTOFF_L, CUTOFF_G = 5.0, 2.0           # the local graph is the bond list; at 2.0 A a molecule keeps ~3.5 global edges per atom
UNIT_MOLS = 192                          # molecules of the collated batch the large cases tile


def small_molecule():
    """Five atoms: a carbon with four hydrogens (tetrahedron, slightly bent).  8 directed bonds, 32 triplet + pair rows
    (20 with pairs only); every atom has the four others within CUTOFF_G (C-H 1.09 A, H-H ~1.78 A)."""
    t = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64) / np.sqrt(3.0)
    pos = np.concatenate([np.zeros((1, 3)), 1.09 * t + np.array([[0.02, 0, 0], [0, -0.03, 0], [0, 0, 0.01], [0.01, 0.02, 0]])])
    src = np.array([0, 0, 0, 0, 1, 2, 3, 4], np.int64)
    dst = np.array([1, 2, 3, 4, 0, 0, 0, 0], np.int64)
    return dict(x=np.array([1, 0, 0, 0, 0], np.float32), pos=pos.astype(np.float32), edge_index=np.stack([src, dst]),
                y=np.float32(0.5))


def _single(k):
    return dict(x=np.array([k % 5], np.float32), pos=np.zeros((1, 3), np.float32), edge_index=np.zeros((2, 0), np.int64),
                y=np.float32(0.25 * (k % 7) - 0.75))


_UNIT = {}


def _unit(seed):
    from pamnet_amd import synth
    if seed not in _UNIT:
        _UNIT[seed] = [synth.qm9_molecule(seed, i) for i in range(UNIT_MOLS)]
    return _UNIT[seed]


def _arrays(graphs):
    """(x, pos, edge_index, atoms per graph) of a list of molecules, concatenated with index offsets."""
    sizes = np.array([g['x'].shape[0] for g in graphs], np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    return (np.concatenate([g['x'] for g in graphs]), np.concatenate([g['pos'] for g in graphs]),
            np.concatenate([g['edge_index'] + o for g, o in zip(graphs, off)], axis=1), sizes)


def qm9_batch_of(n_atoms, seed=4):
    """A QM9-schema synth.Batch of exactly `n_atoms` atoms: copies of one collated batch of UNIT_MOLS molecules while a
    whole copy fits (index offsets, no molecule generated or collated twice), then whole molecules of that batch while the
    next fits, the rest single atoms (no bond, no edge of either kind) spread between those molecules.  Five atoms: the
    hand-made molecule."""
    import torch
    from pamnet_amd import synth
    if n_atoms == 5:
        return synth.collate([small_molecule()])
    unit = _unit(seed)
    ux, upos, uei, usizes = _arrays(unit)
    copies = n_atoms // ux.shape[0]
    rest, left = [], n_atoms - copies * ux.shape[0]
    for m in unit:
        if m['x'].shape[0] > left:
            break
        rest.append(m)
        left -= m['x'].shape[0]
    assert rest or copies, n_atoms
    mixed, every = [], max(len(rest) // max(left, 1), 1)
    for i, m in enumerate(rest):
        if left and i % every == 0 and i // every < left:
            mixed.append(_single(i // every))
        mixed.append(m)
    mixed += [_single(k) for k in range(sum(g['x'].shape[0] == 1 for g in mixed), left)]
    parts_x, parts_pos, parts_ei, parts_sz, off = [], [], [], [], 0
    if copies:
        parts_x, parts_pos = [np.tile(ux, copies)], [np.tile(upos, (copies, 1))]
        shift = (np.arange(copies, dtype=np.int64) * ux.shape[0])[:, None, None]
        parts_ei = [(uei[None] + shift).transpose(1, 0, 2).reshape(2, -1)]
        parts_sz, off = [np.tile(usizes, copies)], copies * ux.shape[0]
    if mixed:
        mx, mpos, mei, msz = _arrays(mixed)
        parts_x.append(mx), parts_pos.append(mpos), parts_ei.append(mei + off), parts_sz.append(msz)
    sizes = np.concatenate(parts_sz)
    x = np.concatenate(parts_x)
    assert x.shape[0] == n_atoms == int(sizes.sum())
    return synth.Batch(x=torch.from_numpy(x), pos=torch.from_numpy(np.concatenate(parts_pos)),
                       edge_index=torch.from_numpy(np.ascontiguousarray(np.concatenate(parts_ei, axis=1))),
                       batch=torch.from_numpy(np.repeat(np.arange(sizes.shape[0], dtype=np.int64), sizes)),
                       y=torch.zeros(sizes.shape[0]), num_graphs=int(sizes.shape[0]))


def host_sizes(b, small=False):
    """(E_g, E_l, T + P) of a batch by plain numpy, from the definitions: pairs of one graph within CUTOFF_G (self excluded),
    directed bonds, and per bond j -> i the bonds k -> j (k != i; not with pairs only) plus the bonds j' -> i (the bond itself
    among them: csrc/graph.hip triplet_count_kernel)."""
    pos, batch, ei = b.pos.numpy().astype(np.float64), b.batch.numpy(), b.edge_index.numpy()
    n = pos.shape[0]
    start = np.concatenate([[0], np.cumsum(np.bincount(batch))])
    eg = 0
    for g in range(start.shape[0] - 1):
        p = pos[start[g]:start[g + 1]]
        dist = np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1))
        eg += int((dist <= CUTOFF_G).sum()) - p.shape[0]
    deg = np.bincount(ei[1], minlength=n)
    el = ei.shape[1]
    pairs = int(deg[ei[1]].sum())
    trips = 0 if small else int((deg[ei[0]] - 1).sum())
    return eg, el, trips + pairs


_RATIOS = {}


def per_atom_ratios(seed=4, mols=24):
    """(E_g / n, E_l / n, (T + P) / n, pairs / n) over the first `mols` synthetic molecules."""
    if seed not in _RATIOS:
        from pamnet_amd import synth
        b = synth.collate(_unit(seed)[:mols] if seed in _UNIT else [synth.qm9_molecule(seed, i) for i in range(mols)])
        n = float(b.x.shape[0])
        eg, el, tp = host_sizes(b)
        _RATIOS[seed] = (eg / n, el / n, tp / n, host_sizes(b, small=True)[2] / n)
    return _RATIOS[seed]
