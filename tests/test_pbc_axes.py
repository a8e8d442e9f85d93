"""Per-axis periodicity: `data.pbc` (torch.bool [num_graphs, 3], or three bools for every graph) says along which lattice vectors
a graph of a periodic batch repeats -- slabs, wires, and isolated molecules beside bulk cells.  pamnet_amd/graph.py
build_graph(pbc=), and the two entry points pamnet_cell_prepare_axes_f64 / pamnet_cell_images_axes_i32 (csrc/graph.hip), which
complete the cell with unit vectors orthogonal to the periodic ones and zero the open axes' inverse entries; every kernel that
reads the table is the fully periodic one.

The fp64 references are brute-force numpy written here: every image n of every ordered pair with n_k in [-K, K] along the
periodic axes and n_k = 0 along the open ones, displacements p_a - p_b - n @ cell from the USER's periodic vectors alone (the
vector of an open axis never enters).  Inputs are made once on the CPU with fixed seeds and never modified; their preconditions
are asserted in fp64 by a test that needs no GPU.  cutoff_l = 2.0, cutoff_g = 5.0 throughout.

Tolerances: TOL, GRAD_TOL, KTOL and the protocol _ok of tests/test_hip_forces.py."""
import itertools

import numpy as np
import pytest
import torch

from conftest import maxnorm_err
from test_pbc import _arrays, _geometry64, _record

PREPARE, PREPARE_AXES = 'pamnet_cell_prepare_f64', 'pamnet_cell_prepare_axes_f64'
IMAGES, IMAGES_AXES = 'pamnet_cell_images_i32', 'pamnet_cell_images_axes_i32'
NEW = (PREPARE_AXES, IMAGES_AXES)
PBC_BIT = 128
CUT_L, CUT_G = 2.0, 5.0
SEP = 0.9                                        # minimum separation of the generated atoms, over all images (>= 0.8)
TRI_A = [[11.5, 0.0, 0.0], [2.0, 11.5, 0.0], [-1.5, 1.75, 11.5]]
TRI_B = [[12.0, 0.0, 0.0], [-2.5, 11.75, 0.0], [1.75, -2.25, 11.625]]
# what stands on an open axis in the table test: zero, short, skewed, and parallel to TRI_*'s first vector (a singular matrix)
OPEN_VECTORS = ([0.0, 0.0, 0.0], [0.25, 0.5, -0.75], [3.0, -2.0, 1.0], [23.0, 0.0, 0.0])


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs an MI355X'
    from pamnet_amd import lib
    lib.load()
    return torch.device('cuda:0')


# ---------------------------------------------------------------------------------------------- fp64 references (numpy, CPU)
def _complete(cell, pbc):
    """The completion rule, fp64: the user's periodic vectors, unit vectors orthogonal to them on the open axes."""
    a = np.array(cell, dtype=np.float64)
    p = [bool(v) for v in pbc]
    unit = lambda w: w / np.linalg.norm(w)
    if sum(p) == 3:
        return a
    if sum(p) == 0:
        return np.eye(3)
    if sum(p) == 2:
        k = p.index(False)
        a[k] = unit(np.cross(a[(k + 1) % 3], a[(k + 2) % 3]))
        return a
    i = p.index(True)
    e = np.zeros(3)
    e[int(np.argmin(np.abs(a[i])))] = 1.0                         # (argmin: the lowest index on ties)
    j, k = (i + 1) % 3, (i + 2) % 3
    a[j] = unit(np.cross(a[i], e))
    a[k] = unit(np.cross(a[i], a[j]))
    return a


def _axis_heights(cell, pbc):
    """Heights |det'| / |a_j' x a_k'| of the PERIODIC axes in the completed cell: the in-plane heights of a slab, the length of
    a wire's vector."""
    c = _complete(cell, pbc)
    det = abs(np.linalg.det(c))
    return [det / np.linalg.norm(np.cross(c[(k + 1) % 3], c[(k + 2) % 3])) for k in range(3) if pbc[k]]


def _triples(pbc, K):
    """Image triples, ascending (n0, n1, n2): n_k in [-K, K] along periodic axes, 0 along open ones."""
    return np.array(list(itertools.product(*[range(-K, K + 1) if f else (0,) for f in pbc])), dtype=np.float64)


def _image_dists(pos, cell, pbc, K):
    """(nn [M, 3], d [n, n, M]): d[a, b, m] = |p_a - p_b - nn[m] @ cell| with the open axes' rows of `cell` left out."""
    nn = _triples(pbc, K)
    lat = np.where(np.array(pbc, dtype=bool)[:, None], np.asarray(cell, dtype=np.float64), 0.0)
    p = np.asarray(pos, dtype=np.float64)
    v = p[:, None, None, :] - p[None, :, None, :] - (nn @ lat)[None, None]
    return nn, np.sqrt((v ** 2).sum(-1))


def _own(n, nn):
    """[n, n, M]: the entry is an atom's own zero image."""
    return np.eye(n, dtype=bool)[:, :, None] & (np.abs(nn).sum(-1) == 0)[None, None]


class Struct(object):
    """One graph: x, pos (fp32 numpy), cell (fp32 numpy [3, 3]), pbc (three bools), K (the brute force's image range)."""

    def __init__(self, x, pos, cell, pbc, K):
        self.x, self.pos, self.cell, self.pbc, self.K = x, pos, np.asarray(cell, dtype=np.float32), tuple(pbc), K
        self.n = int(pos.shape[0])

    def dists(self):
        if '_d' not in self.__dict__:
            self._d = _image_dists(self.pos, self.cell, self.pbc, self.K)
        return self._d


def _lists_all(structs, r):
    """(ptr, row_of, col, img, dist) of the all-image graph at r: rows by query, then ascending (j, n0, n1, n2)."""
    rows, cols, img, dist, s = [], [], [], [], 0
    for st in structs:
        nn, d = st.dists()
        keep = (d <= r) & ~_own(st.n, nn)
        q, j, m = np.nonzero(keep)                                # (C order: ascending (q, j, m); m ascends with the image)
        rows.append(q + s), cols.append(j + s), img.append(nn[m].astype(np.int64)), dist.append(d[q, j, m])
        s += st.n
    rows, cols, img, dist = np.concatenate(rows), np.concatenate(cols), np.concatenate(img), np.concatenate(dist)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=s))])
    return ptr, rows, cols, img, dist


def _lists_min(structs, r):
    """(ptr, row_of, col, dist) of the minimum-image graph at r: rows by query, ascending neighbour, self excluded."""
    rows, cols, dist, s = [], [], [], 0
    for st in structs:
        nn, d = st.dists()
        dmin = d.min(-1)
        keep = (dmin <= r) & ~np.eye(st.n, dtype=bool)
        q, j = np.nonzero(keep)
        rows.append(q + s), cols.append(j + s), dist.append(dmin[q, j])
        s += st.n
    rows, cols, dist = np.concatenate(rows), np.concatenate(cols), np.concatenate(dist)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=s))])
    return ptr, rows, cols, dist


def _assert_clear(st, cutoffs=(CUT_L, CUT_G), one_image=None):
    """No (pair, image) distance within 1e-4 of a cutoff, minimum separation >= 0.8; one_image: at most one image of a pair
    within that radius (what the minimum-image mode needs)."""
    nn, d = st.dists()
    off = d[~_own(st.n, nn)]
    for r in cutoffs:
        assert float(np.abs(off - r).min()) > 1e-4, (r, float(np.abs(off - r).min()))
    assert float(off.min()) >= 0.8, float(off.min())
    if one_image is not None:
        assert int((d <= one_image).sum(-1).max()) <= 1


# ------------------------------------------------------------------------------------------------------------- inputs
def _scatter(rng, n, cell, pbc, spans, K, sep=SEP, grid=None):
    """n points: fractional coordinates uniform in [0, 1) along the periodic axes of the completed cell, uniform in `spans[k]`
    (Angstrom: the completed vectors there are unit vectors) along the open ones; rounded to fp32 (or to multiples of `grid`).
    Rejected: a point with an image distance below `sep` to a point before it or to itself, or within 2e-4 of a cutoff."""
    c = _complete(cell, pbc)
    pts = []
    while len(pts) < n:
        f = np.array([rng.uniform(0.0, 1.0) if pbc[k] else rng.uniform(*spans[k]) for k in range(3)])
        p = f @ c
        p = np.round(p / grid) * grid if grid else p.astype(np.float32).astype(np.float64)
        nn, d = _image_dists(np.array(pts + [p]), cell, pbc, K)
        near = d[-1][~_own(len(pts) + 1, nn)[-1]]
        if near.size and (near.min() < sep or min(np.abs(near - r).min() for r in (CUT_L, CUT_G)) < 2e-4):
            continue
        pts.append(p)
    return np.array(pts)


_MADE = {}


def _structs():
    """The graphs of the list tests, made once.
    slab_min: 30 atoms, triclinic in-plane lattice (heights 11.3 / 11.5), third vector short and skewed, atoms from 4 A below to 5 A
              above the 3 A it spans;  wire_min: 25 atoms along a skewed 11.2 A vector (axis 0), the other two vectors zero and short.
    slab_all: 10 atoms, 4.5 x 4.5 in-plane (below cutoff_g: self-images), third vector zero;  wire_all: 6 atoms along a 4.5 A vector.
    slab_z / slab_z2: a, b in the xy-plane, third vector zero, z-spread 10.5 (the slab-equals-tall-cell test)."""
    if 'structs' in _MADE:
        return _MADE['structs']
    rng = np.random.RandomState(11)
    spec = {'slab_min': (30, [[11.5, 0.0, 0.0], [2.0, 11.5, 0.0], [0.5, 0.25, 3.0]], (True, True, False), {2: (-4.0, 8.0)}, 2),
            'wire_min': (25, [[1.0, 2.0, 11.0], [0.0, 0.0, 0.0], [0.25, 0.0, 0.0]], (True, False, False),
                         {1: (-3.0, 3.0), 2: (-3.0, 3.0)}, 2),
            'slab_all': (10, [[4.5, 0.0, 0.0], [0.0, 4.5, 0.0], [0.0, 0.0, 0.0]], (True, True, False), {2: (-2.0, 5.0)}, 3),
            'wire_all': (6, [[0.0, 2.75, 3.5], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]], (True, False, False),
                         {1: (-2.0, 2.0), 2: (-2.0, 2.0)}, 3),
            'slab_z': (32, [[11.5, 0.0, 0.0], [2.0, 11.5, 0.0], [0.0, 0.0, 0.0]], (True, True, False), {2: (0.0, 10.5)}, 2),
            'slab_z2': (20, [[12.0, 0.0, 0.0], [-2.5, 11.75, 0.0], [0.0, 0.0, 0.0]], (True, True, False), {2: (-5.0, 5.5)}, 2)}
    out = {}
    for name, (n, cell, pbc, spans, K) in spec.items():
        pos = _scatter(rng, n, cell, pbc, spans, K)
        out[name] = Struct(rng.randint(0, 5, n).astype(np.float32), pos.astype(np.float32), cell, pbc, K)
    _MADE['structs'] = out
    return out


def _batch(structs, pbc='tensor', **kw):
    """synth.Batch of the graphs (CPU): x, batch, pos, cell, num_graphs and pbc -- 'tensor': the bool tensor of the graphs' flags;
    None: no pbc; anything else: handed over as it is."""
    from pamnet_amd import synth
    b = synth.Batch(x=torch.from_numpy(np.concatenate([s.x for s in structs])),
                    batch=torch.cat([torch.full((s.n,), g, dtype=torch.long) for g, s in enumerate(structs)]),
                    pos=torch.from_numpy(np.concatenate([s.pos for s in structs])),
                    cell=torch.from_numpy(np.stack([s.cell for s in structs])), num_graphs=len(structs), **kw)
    if isinstance(pbc, str) and pbc == 'tensor':
        b.pbc = torch.tensor([s.pbc for s in structs], dtype=torch.bool)
    elif pbc is not None:
        b.pbc = pbc
    return b


def _build(b, dev, cutoff_l=CUT_L, **kw):
    from pamnet_amd import graph as G
    d = b.to(dev)
    return G.build_graph('QM9', cutoff_l, CUT_G, 'source_to_target', d.x, d.batch, d.pos, None, num_graphs=d.num_graphs, n_types=5,
                         cell=getattr(d, 'cell', None), pbc=getattr(d, 'pbc', None), **kw)


def _tall(st, height=32.0):
    """The slab with (0, 0, height) as its third vector, fully periodic."""
    cell = st.cell.copy()
    cell[2] = [0.0, 0.0, height]
    return Struct(st.x, st.pos, cell, (True, True, True), st.K)


# ---- the lifted, split molecules (test 4)
LIFT_CELL = [[16.0, 0.0, 0.0], [3.0, 16.0, 0.0], [0.0, 0.0, 6.0]]


def _lifted():
    """Four molecules of synth.qm9_batch(0, 0, 4) without bonds, each translated in the plane (fp32) and wrapped into the 16 A
    in-plane lattice of LIFT_CELL -- so that it lies split across the in-plane boundary -- and lifted to 36 A and more above the
    plane, 30 A past the 6 A of the third vector.  Returns (periodic batch with pbc = (True, True, False), oracle batch with the
    unwrapped coordinates rebuilt in fp64 from the wrapped fp32 ones plus integer in-plane lattice vectors, the structs of the
    wrapped input as slabs, the same with the third vector periodic)."""
    if 'lifted' in _MADE:
        return _MADE['lifted']
    from oracle import pamnet_oracle as O
    from pamnet_amd import synth
    b = synth.qm9_batch(0, 0, 4)
    cell64 = np.array(LIFT_CELL, dtype=np.float64)
    rng = np.random.RandomState(4)
    wrapped, unwrapped, slabs, bulk = [], [], [], []
    for g in range(4):
        sel = (b.batch == g).numpy()
        p32 = b.pos.numpy()[sel]
        zlo = float(p32[:, 2].min())
        t = (np.array([rng.uniform(0, 1), rng.uniform(0, 1), 0.0]) @ cell64 + [0.0, 0.0, 36.0 - zlo]).astype(np.float32)
        moved = (p32 + t).astype(np.float64)                                         # fp32 translation
        m = np.floor(moved @ np.linalg.inv(cell64))
        m[:, 2] = 0.0                                                                # wrapped in the plane only
        w32 = (moved - m @ cell64).astype(np.float32)                                # the input
        wrapped.append(w32)
        unwrapped.append(w32.astype(np.float64) + m @ cell64)                        # exact rebuild
        x = b.x.numpy()[sel].astype(np.float32)
        slabs.append(Struct(x, w32, LIFT_CELL, (True, True, False), 2))
        bulk.append(Struct(x, w32, LIFT_CELL, (True, True, True), 2))
    pos_u = torch.from_numpy(np.concatenate(unwrapped))
    periodic = synth.Batch(x=b.x, batch=b.batch, pos=torch.from_numpy(np.concatenate(wrapped)),
                           cell=torch.tensor([LIFT_CELL] * 4, dtype=torch.float32), pbc=(True, True, False), y=b.y, num_graphs=4)
    ei = O.radius_graph(pos_u, b.batch, CUT_L)
    ei = ei[:, ei[0] != ei[1]]
    ob = synth.Batch(x=b.x, batch=b.batch, pos=pos_u, edge_index=ei, y=b.y, num_graphs=4)
    _MADE['lifted'] = (periodic, ob, slabs, bulk)
    return _MADE['lifted']


# ---- the mixed batch (test 5)
def _mixed():
    """[bulk cell: 20 atoms in a 10.5 cube; slab: slab_min; molecule: 14 atoms in open space, pbc all False, a zero cell]."""
    if 'mixed' not in _MADE:
        rng = np.random.RandomState(23)
        cube = [[10.5, 0.0, 0.0], [0.0, 10.5, 0.0], [0.0, 0.0, 10.5]]
        bulk = Struct(rng.randint(0, 5, 20).astype(np.float32),
                      _scatter(rng, 20, cube, (True, True, True), {}, 2).astype(np.float32), cube, (True, True, True), 2)
        zero = np.zeros((3, 3))
        none = (False, False, False)
        mol = Struct(rng.randint(0, 5, 14).astype(np.float32),
                     _scatter(rng, 14, zero, none, {0: (20.0, 25.0), 1: (-3.0, 2.0), 2: (-41.0, -36.5)}, 0).astype(np.float32),
                     zero, none, 0)
        _MADE['mixed'] = [bulk, _structs()['slab_min'], mol]
    return _MADE['mixed']


# ---- the slab and its in-plane 2 x 1 supercell (test 6)
GRID = 2.0 ** -12


def _super_slab():
    """A: 24 atoms on a 2^-12 grid in a slab with a = (10.5, 0, 0), b = (2, 11.5, 0) and a short skewed third vector, open.
    B: its 2 x 1 supercell in the plane as one graph (the atoms, then their copies at + a), exact in fp32."""
    if 'super' not in _MADE:
        rng = np.random.RandomState(6)
        cell = np.array([[10.5, 0.0, 0.0], [2.0, 11.5, 0.0], [0.5, -0.25, 2.0]])
        pbc = (True, True, False)
        pos = _scatter(rng, 24, cell, pbc, {2: (-3.0, 3.0)}, 2, grid=GRID)
        x = rng.randint(0, 5, 24).astype(np.float32)
        a = Struct(x, pos.astype(np.float32), cell, pbc, 2)
        cell_b = np.array([2 * cell[0], cell[1], cell[2]])
        pos_b = np.concatenate([pos, pos + cell[0]])
        b = Struct(np.concatenate([x, x]), pos_b.astype(np.float32), cell_b, pbc, 2)
        assert np.array_equal(a.pos.astype(np.float64), pos) and np.array_equal(b.pos.astype(np.float64), pos_b)
        _MADE['super'] = (a, b)
    return _MADE['super']


# -------------------------------------------------------------------------------------------------- CPU: preconditions
def test_axes_inputs_meet_their_preconditions():
    """(No GPU.)  What the GPU tests state about their inputs, in fp64 numpy: no (pair, image) distance within 1e-4 of either
    cutoff, minimum separation >= 0.8, the periodic-axis heights meet the mode's condition, atoms lie outside the box along
    the open axes, and the 'all' structures have self-images."""
    s = _structs()
    for name in ('slab_min', 'wire_min', 'slab_z', 'slab_z2'):
        h = _axis_heights(s[name].cell, s[name].pbc)
        assert min(h) > 2 * max(CUT_L, CUT_G), (name, h)
        _assert_clear(s[name], one_image=CUT_G)
        assert s[name].n <= 40
    for name in ('slab_all', 'wire_all'):
        h = _axis_heights(s[name].cell, s[name].pbc)
        assert 2 * CUT_L < min(h) and max(h) < CUT_G and min(h) >= CUT_G / 4, (name, h)
        _assert_clear(s[name], one_image=CUT_L)
        nn, d = s[name].dists()
        keep = (d <= CUT_G) & ~_own(s[name].n, nn)
        assert int(keep[np.eye(s[name].n, dtype=bool)].sum(-1).min()) >= 2            # every atom sees images of itself
        assert int(np.abs(nn[np.nonzero(keep)[2]]).max()) < s[name].K               # the brute force's range is wide enough
    assert all(abs(h - 4.5) < 1e-12 for h in _axis_heights(s['slab_all'].cell, s['slab_all'].pbc))
    # along the open axes the atoms leave the box the user's vector spans by several Angstrom
    z = s['slab_min'].pos.astype(np.float64) @ _complete(s['slab_min'].cell, s['slab_min'].pbc)[2]
    assert z.min() < -2.0 and z.max() > 3.0 + 3.0
    # the minimum-image structures have pairs across the periodic boundary within each cutoff's reach
    for name in ('slab_min', 'wire_min'):
        nn, d = s[name].dists()
        m = d.argmin(-1)
        assert bool(((d.min(-1) <= CUT_G) & (np.abs(nn[m]).sum(-1) > 0)).any())
    # the slab that equals its tall cell: z-spread below 16 - cutoff_g, and the tall cell is a valid fully periodic cell
    for name in ('slab_z', 'slab_z2'):
        zs = s[name].pos[:, 2].astype(np.float64)
        assert zs.max() - zs.min() < 16.0 - CUT_G and not s[name].cell[2].any() and not s[name].cell[:2, 2].any()
        tall = _tall(s[name])
        assert min(_axis_heights(tall.cell, tall.pbc)) > 2 * CUT_G
        for r in (CUT_L, CUT_G):                                                      # the same lists either way
            assert all(np.array_equal(u, v) for u, v in zip(_lists_min([s[name]], r), _lists_min([tall], r)))
        assert len(_lists_min([s[name]], CUT_L)[1]) > 0
    # the lifted molecules: split in the plane, 30 A past the third vector, and wrapped wrongly if that vector were periodic
    periodic, ob, slabs, bulk = _lifted()
    split = 0
    for st, bk in zip(slabs, bulk):
        _assert_clear(st, one_image=CUT_G)
        assert min(_axis_heights(st.cell, st.pbc)) > 2 * CUT_G
        assert float(st.pos[:, 2].min()) >= 36.0 - 1e-3 and 36.0 - 6.0 >= 30.0
        nn, d = st.dists()
        split += int(bool((np.abs(nn[d.argmin(-1)]).sum(-1) > 0).any()))
    assert split >= 2, split
    lm, lb = _lists_min(slabs, CUT_G), _lists_min(bulk, CUT_G)
    assert len(lm[1]) != len(lb[1]) or not np.array_equal(lm[2], lb[2]) or float(np.abs(lm[3] - lb[3]).max()) > 1.0
    pu = ob.pos.numpy()
    s0 = 0
    for st in slabs:                                              # the slab's minimum-image distances are the molecule's own
        true_d = np.sqrt(((pu[s0:s0 + st.n, None] - pu[None, s0:s0 + st.n]) ** 2).sum(-1))
        dmin = st.dists()[1].min(-1)
        near = true_d <= CUT_G + 1e-3
        assert float(np.abs(dmin[near] - true_d[near]).max()) < 1e-9 and bool((dmin[~near] > CUT_G + 1e-3).all())
        s0 += st.n
    # the mixed batch and the supercell
    bulk_c, slab, mol = _mixed()
    _assert_clear(bulk_c, one_image=CUT_G), _assert_clear(mol)
    assert not mol.cell.any() and mol.pbc == (False, False, False) and len(_lists_min([mol], CUT_L)[1]) > 0
    a, b = _super_slab()
    for st in (a, b):
        _assert_clear(st, one_image=CUT_G)
        assert min(_axis_heights(st.cell, st.pbc)) > 2 * CUT_G
    for r in (CUT_L, CUT_G):
        assert len(_lists_min([b], r)[1]) == 2 * len(_lists_min([a], r)[1])


# ------------------------------------------------------------------------------------------------------------ 8. C ABI
def test_header_declares_the_axes_entry_points_at_abi_18():
    """(No GPU: the header and the built library.)  The twins' argument lists with pbc behind the first pointer."""
    import ctypes
    import re
    from pamnet_amd import build, lib
    decl = lib.declared_functions()
    assert [len(decl[n]) for n in NEW] == [7, 7]
    assert len(decl[PREPARE]) == 6 and len(decl[IMAGES]) == 6
    assert int(re.search(r'#define\s+PAMNET_ABI_VERSION\s+(\d+)', open(lib.HEADER).read()).group(1)) == 18
    h = ctypes.CDLL(build.build())
    assert h.pamnet_abi_version() == 18 and all(hasattr(h, n) for n in NEW)


def test_axes_kernels_are_scratch_free(tmp_path):
    """(No GPU: hipcc cross-compiles csrc/graph.hip for gfx950.)  Compiler's resource report of the cell-table and image-box kernels, by the
    protocol of tests/test_build_resources.py."""
    import os
    import re
    import shutil
    import subprocess
    from pamnet_amd import build
    hipcc = '/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else shutil.which('hipcc')
    if not hipcc:
        pytest.skip('hipcc not available')
    r = subprocess.run([hipcc] + build.FLAGS + ['-c', os.path.join(build.CSRC, 'graph.hip'), '-o', str(tmp_path / 'graph.o'),
                                                '-Rpass-analysis=kernel-resource-usage'], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = {b.split()[0]: b for b in re.split(r'remark: Function Name: ', r.stderr)[1:]}
    for kernel in ('cell_prepare_kernel', 'cell_images_kernel'):
        found = [b for name, b in blocks.items() if kernel in name]
        assert len(found) == 1, kernel
        assert int(re.search(r'ScratchSize \[bytes/lane\]: (\d+)', found[0]).group(1)) == 0, kernel
        assert int(re.search(r'LDS Size \[bytes/block\]: (\d+)', found[0]).group(1)) == 0, kernel


@pytest.mark.gpu
def test_axes_entry_points_validate_their_arguments(dev):
    """EINVAL / ENULL with nothing launched: the sentinel-filled outputs stay."""
    from pamnet_amd import lib
    P = lib.ptr
    cell = torch.eye(3, device=dev).view(1, 9).contiguous() * 20
    pbc = torch.tensor([[1, 1, 0]], dtype=torch.uint8, device=dev)
    tab = torch.full((1, 18), 7.0, dtype=torch.float64, device=dev)
    box = torch.full((1, 3), 7, dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    st = lib.stream_of(cell)

    def prepare(c=cell, p=pbc, n=1, r=5.0, t=tab, f=flag):
        lib.call(PREPARE_AXES, P(c), P(p), n, r, P(t), P(f), st)

    def images(t=tab, p=pbc, n=1, r=5.0, b=box, f=flag):
        lib.call(IMAGES_AXES, P(t), P(p), n, r, P(b), P(f), st)

    bad_sizes = [dict(n=-1), dict(r=0.0), dict(r=-1.0), dict(r=float('nan')), dict(r=float('inf'))]
    for fn, kws, what in ((prepare, bad_sizes, 'EINVAL'), (prepare, [dict(c=None), dict(p=None), dict(t=None), dict(f=None)], 'ENULL'),
                          (images, bad_sizes, 'EINVAL'), (images, [dict(t=None), dict(p=None), dict(b=None), dict(f=None)], 'ENULL')):
        for kw in kws:
            with pytest.raises(RuntimeError, match=what):
                fn(**kw)
    prepare(n=0), images(n=0)                                     # nothing to do: OK, nothing launched
    torch.cuda.synchronize()
    assert bool((tab == 7).all()) and bool((box == 7).all()) and int(flag) == 0


# ------------------------------------------------------------------------------------------------- 1. table vs fp64 numpy
def _table(cells, pbc, cutoff, dev, twin=False):
    """(table [G, 18] fp64, flag word) on the CPU, from the new entry point or (twin) pamnet_cell_prepare_f64."""
    from pamnet_amd import graph as G
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    c = torch.tensor(np.asarray(cells, dtype=np.float32)).to(dev).contiguous().view(-1, 9)
    tab = G.cell_table(c, cutoff, flag, None if twin else torch.tensor(np.asarray(pbc, dtype=bool)).to(dev))
    torch.cuda.synchronize()
    return tab.cpu().numpy(), int(flag)


def _table_rows():
    """All eight flag patterns on the two triclinic cells, the open axes' vectors replaced in turn by a zero, a short, a skewed
    vector and one parallel to the first lattice vector."""
    cells, flags, k = [], [], 0
    for pbc in itertools.product([True, False], repeat=3):
        for base in (TRI_A, TRI_B):
            c = np.array(base, dtype=np.float64)
            for axis in range(3):
                if not pbc[axis]:
                    c[axis] = OPEN_VECTORS[k % len(OPEN_VECTORS)]
                    k += 1
            cells.append(c), flags.append(pbc)
    return cells, flags


@pytest.mark.gpu
def test_table_of_every_flag_pattern_vs_fp64_numpy(dev, monkeypatch):
    calls = _record(monkeypatch)
    cells, flags = _table_rows()
    assert len(set(flags)) == 8 and any(np.linalg.matrix_rank(c) < 3 for c in cells)
    tab, flag = _table(cells, flags, CUT_G, dev)
    assert calls == [PREPARE_AXES] and flag == 0
    worst = dict(unit=0.0, ortho=0.0, delta=0.0, complete=0.0)
    for c, pbc, row in zip(cells, flags, tab):
        got, inv = row[:9].reshape(3, 3), row[9:].reshape(3, 3)   # fractional component k of d: sum_m d[m] inv[m, k]
        want = _complete(c.astype(np.float32), pbc)
        worst['complete'] = max(worst['complete'], float(np.abs(got - want).max()))
        for k in range(3):
            if pbc[k]:
                assert np.array_equal(got[k], c[k])              # the user's vector, as given
                continue
            assert np.array_equal(inv[:, k], np.zeros(3)) and not np.signbit(inv[:, k]).any()        # exactly +0.0
            worst['unit'] = max(worst['unit'], abs(float(np.linalg.norm(got[k])) - 1.0))
            for i in range(3):
                if pbc[i]:                                        # the cosine of the angle to a periodic vector
                    worst['ortho'] = max(worst['ortho'], abs(float(got[k] @ got[i])) / float(np.linalg.norm(got[i])))
                    worst['delta'] = max(worst['delta'], abs(float(inv[:, i] @ got[k])))             # b_i . a_k' = 0
        for i in range(3):
            for j in range(3):
                if pbc[i] and pbc[j]:                             # b_i . a_j = delta_ij
                    worst['delta'] = max(worst['delta'], abs(float(inv[:, i] @ got[j]) - float(i == j)))
    print('table:', worst)
    assert worst['unit'] <= 1e-14 and worst['ortho'] <= 1e-14 and worst['delta'] <= 1e-13 and worst['complete'] <= 1e-14, worst


@pytest.mark.gpu
def test_table_verdicts_look_at_periodic_axes_only(dev):
    """A height just above 2 * cutoff passes, one just below fails; an open axis of any length never fails; degenerate periodic
    vectors fail with a finite table."""
    slab = [[10.5, 0.0, 0.0], [3.0, 10.5, 0.0], [0.0, 0.0, 1.0]]                      # in-plane heights 10.096 and 10.5
    h = _axis_heights(slab, (True, True, False))
    assert abs(min(h) - 10.5 * 10.5 / np.hypot(3.0, 10.5)) < 1e-12 and abs(max(h) - 10.5) < 1e-12
    for r, want in ((5.04, 0), (5.05, PBC_BIT), (5.3, PBC_BIT)):
        assert (2 * r < min(h)) == (want == 0)
        assert _table([slab], [(True, True, False)], r, dev)[1] == want, r
    wire = [[0.0, 6.3, 8.4], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]                        # length 10.5
    for r, want in ((5.2, 0), (5.3, PBC_BIT)):
        assert _table([wire], [(True, False, False)], r, dev)[1] == want, r
    assert _table([wire], [(False, False, False)], 1000.0, dev)[1] == 0               # a molecule has no condition at all
    for third in ([0.0, 0.0, 0.0], [0.0, 0.0, 1e-3], [0.0, 0.0, 1e6], [10.5, 0.0, 0.0], [float('nan')] * 3, [float('inf'), 0.0, 0.0]):
        tab, flag = _table([[slab[0], slab[1], third]], [(True, True, False)], CUT_G, dev)
        assert flag == 0 and np.isfinite(tab).all(), third
    # the same short or singular third vector, periodic: refused
    for third in ([0.0, 0.0, 1.0], [10.5, 0.0, 0.0]):
        assert _table([[slab[0], slab[1], third]], [(True, True, True)], CUT_G, dev)[1] == PBC_BIT
    for cell, pbc in (([[10.5, 0.0, 0.0], [21.0, 0.0, 0.0], [0.0, 0.0, 30.0]], (True, True, False)),     # parallel in-plane vectors
                      ([[0.0, 0.0, 0.0], [0.0, 30.0, 0.0], [0.0, 0.0, 30.0]], (True, False, False)),    # a wire of zero length
                      ([[0.0, 0.0, 0.0], [0.0, 30.0, 0.0], [0.0, 0.0, 30.0]], (True, True, False))):
        tab, flag = _table([cell], [pbc], CUT_G, dev)
        assert flag == PBC_BIT and np.isfinite(tab).all(), (cell, pbc)
    pre = torch.tensor([1 | 64], dtype=torch.int32, device=dev)                       # ORed into the word, never zeroed
    from pamnet_amd import graph as G
    G.cell_table(torch.zeros(1, 9, device=dev), CUT_G, pre, (True, False, False))
    assert int(pre) == (1 | 64 | PBC_BIT)


@pytest.mark.gpu
def test_rows_of_three_set_flags_are_bitwise_the_twins(dev):
    """Valid, too small, singular and non-finite cells with pbc all True: 18 doubles and the verdict of pamnet_cell_prepare_f64."""
    rng = np.random.RandomState(2)
    cells = [TRI_A, TRI_B, [[9.0, 0, 0], [0, 30.0, 0], [0, 0, 30.0]], [[10.5, 0, 0], [21.0, 0, 0], [0, 0, 10.5]],
             [[float('nan'), 0, 0], [0, 20.0, 0], [0, 0, 20.0]]]
    cells += [(np.eye(3) * 12.0 + rng.uniform(-3.0, 3.0, (3, 3))).tolist() for _ in range(300)]       # over one block of 256
    all_true = [(True, True, True)] * len(cells)
    for group in ([0, 1] + list(range(5, len(cells))), list(range(len(cells)))):
        pick = [cells[k] for k in group]
        tab, flag = _table(pick, all_true[:len(pick)], CUT_G, dev)
        twin, twin_flag = _table(pick, None, CUT_G, dev, twin=True)
        assert flag == twin_flag and (flag == PBC_BIT or len(group) < len(cells))
        assert np.array_equal(tab.view(np.int64), twin.view(np.int64))
    # one graph at a time: the verdict of each
    for k in range(5):
        assert _table([cells[k]], [(True, True, True)], CUT_G, dev)[1] == _table([cells[k]], None, CUT_G, dev, twin=True)[1]


# --------------------------------------------------------------------------------------------- 2. lists vs brute force
def _rel(got, want):
    return float((np.abs(got.cpu().double().numpy() - want) / want).max())


@pytest.mark.gpu
def test_minimum_image_lists_of_a_slab_and_a_wire_match_brute_force(dev, monkeypatch):
    s = _structs()
    structs = [s['slab_min'], s['wire_min']]
    for st in structs:
        _assert_clear(st, one_image=CUT_G)
    calls = _record(monkeypatch)
    g = _build(_batch(structs), dev, need_grad=True)
    assert PREPARE_AXES in calls and PREPARE not in calls and IMAGES_AXES not in calls and g.img_g is None
    for csr, dist, r in ((g.glob, g.dist_g, CUT_G), (g.loc, g.dist_l, CUT_L)):
        ptr, rows, cols, d = _lists_min(structs, r)
        assert np.array_equal(csr.ptr.cpu().numpy(), ptr) and np.array_equal(csr.row_of.cpu().numpy(), rows)
        assert np.array_equal(csr.col.cpu().numpy(), cols) and len(rows) > 0
        rel = _rel(dist, d)
        print('r', r, 'edges', len(rows), 'length rel err', rel)
        assert rel <= 1e-6, rel


@pytest.mark.gpu
def test_all_image_lists_of_a_slab_and_a_wire_match_brute_force(dev, monkeypatch):
    """ptr / row_of / col / img_g in the stated order (j, n0, n1, n2) over periodic-axis images only; img_g is 0 along open axes;
    the local graph stays the minimum-image one."""
    s = _structs()
    structs = [s['slab_all'], s['wire_all']]
    for st in structs:
        _assert_clear(st, one_image=CUT_L)
    calls = _record(monkeypatch)
    g = _build(_batch(structs), dev, need_grad=True, cell_images='all')
    assert [c for c in calls if c in (PREPARE, PREPARE_AXES, IMAGES, IMAGES_AXES)] == [PREPARE_AXES, IMAGES_AXES], calls
    ptr, rows, cols, img, d = _lists_all(structs, CUT_G)
    assert np.array_equal(g.glob.ptr.cpu().numpy(), ptr) and np.array_equal(g.glob.row_of.cpu().numpy(), rows)
    assert np.array_equal(g.glob.col.cpu().numpy(), cols) and np.array_equal(g.img_g.cpu().numpy(), img)
    assert _rel(g.dist_g, d) <= 1e-6
    batch = np.repeat(np.arange(2), [st.n for st in structs])
    im = g.img_g.cpu().numpy()
    for gi, st in enumerate(structs):
        mine = im[batch[rows] == gi]
        for k in range(3):
            assert bool(np.abs(mine[:, k]).max() > 0) == st.pbc[k], (gi, k)           # images along periodic axes, none along open
    assert int((rows == cols).sum()) > 0                          # self-images
    lptr, lrows, lcols, ld = _lists_min(structs, CUT_L)
    assert np.array_equal(g.loc.ptr.cpu().numpy(), lptr) and np.array_equal(g.loc.col.cpu().numpy(), lcols) and len(lrows) > 0
    assert _rel(g.dist_l, ld) <= 1e-6


# --------------------------------------------------------------------------- 3. a slab equals the tall fully periodic cell
def _energies(model, b, dev, **attrs):
    """(prediction, forces, virial, the model's graph) of one run with positions and a zero strain that require grad."""
    data = b.to(dev)
    for k, v in attrs.items():
        setattr(data, k, v)
    data.pos.requires_grad_(True)
    data.strain = torch.zeros(data.num_graphs, 3, 3, device=dev, requires_grad=True)
    out = model(data)
    f, w = torch.autograd.grad(out.sum(), [data.pos, data.strain])
    return out.detach(), f, w, getattr(model, '_graph_cache', None)


@pytest.mark.gpu
@pytest.mark.parametrize('small,dim', [(False, 128), (True, 32)])
def test_a_slab_equals_the_tall_fully_periodic_cell_bit_for_bit(dev, monkeypatch, small, dim):
    """Run A: third vector zero, pbc = (True, True, False).  Run B: third vector (0, 0, 32), no pbc.  Every graph array, the
    energies, the forces and the virial are torch.equal -- on the step-by-step route, on the molecule-local builder and with
    cell_images='all'; A calls the new prepare, B the twin."""
    import models
    s = _structs()
    slabs = [s['slab_z'], s['slab_z2']]
    a = _batch(slabs, pbc=(True, True, False))
    b = _batch([_tall(st) for st in slabs], pbc=None)
    assert not a.cell[:, 2].any() and b.cell[:, 2].tolist() == [[0.0, 0.0, 32.0]] * 2 and torch.equal(a.pos, b.pos)
    calls = _record(monkeypatch)
    for kw in (dict(), dict(mol_local=True), dict(cell_images='all')):
        del calls[:]
        ga = _build(a, dev, need_grad=True, with_triplets=not small, **kw)
        used_a = [c for c in calls if c in (PREPARE, PREPARE_AXES, IMAGES, IMAGES_AXES) or 'mol_graph' in c]
        del calls[:]
        gb = _build(b, dev, need_grad=True, with_triplets=not small, **kw)
        used_b = [c for c in calls if c in (PREPARE, PREPARE_AXES, IMAGES, IMAGES_AXES) or 'mol_graph' in c]
        builder = ['pamnet_mol_graph_pbc_count_i32', 'pamnet_mol_graph_pbc_fill_i32'] if 'mol_local' in kw else []
        images = 'cell_images' in kw
        assert used_a == [PREPARE_AXES] + ([IMAGES_AXES] if images else []) + builder, (kw, used_a)
        assert used_b == [PREPARE] + ([IMAGES] if images else []) + builder, (kw, used_b)
        xa, xb = _arrays(ga), _arrays(gb)
        assert xa.keys() == xb.keys() and ga.glob.m > 0 and ga.loc.m > 0 and ga.tp.m > 0
        for k in xa:
            assert xa[k].dtype == xb[k].dtype and torch.equal(xa[k], xb[k]), (kw, k)
        if images:
            assert torch.equal(ga.img_g, gb.img_g) and int(ga.img_g[:, 2].abs().max()) == 0
    torch.manual_seed(0)
    cfg = models.Config(dataset='QM9', dim=dim, n_layer=2, cutoff_l=CUT_L, cutoff_g=CUT_G)
    model = (models.PAMNet_s if small else models.PAMNet)(cfg).to(dev)
    for attrs in (dict(), dict(mol_local=True), dict(cell_images='all')):
        del calls[:]
        e_a, f_a, w_a, _ = _energies(model, a, dev, **attrs)
        assert PREPARE_AXES in calls and PREPARE not in calls
        del calls[:]
        e_b, f_b, w_b, _ = _energies(model, b, dev, **attrs)
        assert PREPARE in calls and PREPARE_AXES not in calls
        assert torch.isfinite(e_a).all() and float(f_a.abs().max()) > 0 and float(w_a.abs().max()) > 0
        assert torch.equal(e_a, e_b) and torch.equal(f_a, f_b) and torch.equal(w_a, w_b), attrs


# ----------------------------------------------------------------------------------------------- 4. open axes are open
@pytest.mark.gpu
def test_a_molecule_lifted_past_the_third_vector_matches_the_oracle(dev):
    """Molecules split across the in-plane boundary of a slab and lifted 30 A past the third vector's length, against the oracle
    fed the unwrapped coordinates: the prediction within TOL = 1e-5 max-normalised of the fp64 oracle, the forces by the protocol
    of tests/test_hip_forces.py at grad_tol: err(hip, oracle_fp64) <= max(grad_tol, 2 * err(oracle_fp32, oracle_fp64)).  With the
    third vector periodic the brute-force lists differ (asserted), so the test tells the two apart."""
    import models
    from oracle import pamnet_oracle as O
    from test_hip_forces import TOL, grad_tol
    assert TOL == 1e-5 and grad_tol('QM9') == 1e-5
    periodic, ob, slabs, bulk = _lifted()
    lm, lb = _lists_min(slabs, CUT_G), _lists_min(bulk, CUT_G)
    assert len(lm[1]) != len(lb[1]) or not np.array_equal(lm[2], lb[2]) or float(np.abs(lm[3] - lb[3]).max()) > 1.0
    cfg = models.Config(dataset='QM9', dim=128, n_layer=2, cutoff_l=CUT_L, cutoff_g=CUT_G)
    sd = O.init_state_dict(cfg, seed=7)
    model = models.PAMNet(cfg)
    model.load_state_dict(sd, strict=True)
    model = model.to(dev)

    def oracle(dtype):
        p = O.as_params({k: v.detach().to(dtype) for k, v in sd.items()})
        pos = ob.pos.to(dtype).clone().requires_grad_(True)
        out = O.pamnet_forward(p, cfg, ob.x, ob.batch, pos, ob.edge_index, dtype=dtype)
        out.sum().backward()
        return out.detach().numpy(), pos.grad.numpy()

    data = periodic.to(dev)
    data.pos.requires_grad_(True)
    out = model(data)
    g = model._graph_cache
    F, = torch.autograd.grad(out.sum(), data.pos)
    assert g.loc.m == ob.edge_index.size(1) and g.glob.m == len(lm[1])
    ref32, F32 = oracle(torch.float32)
    ref64, F64 = oracle(torch.float64)
    e_out, e_f = maxnorm_err(out.detach().cpu().numpy(), ref64), maxnorm_err(F.cpu().numpy(), F64)
    floor_f = maxnorm_err(F32, F64)
    print('out err', e_out, '(oracle fp32:', maxnorm_err(ref32, ref64), ') force err', e_f, 'floor', floor_f)
    assert torch.isfinite(F).all() and float(np.abs(F64).max()) > 0
    assert e_out <= TOL, e_out
    assert e_f <= max(grad_tol('QM9'), 2 * floor_f), (e_f, floor_f)


# -------------------------------------------------------------------------------------------------------- 5. mixed batch
def _molecule_slices(g, s, e):
    """The arrays of the graph that belong to nodes [s, e), index values made relative to the molecule's first node / local
    edge / row."""
    gp, lp = g.glob.ptr.long(), g.loc.ptr.long()
    g0, g1, l0, l1 = int(gp[s]), int(gp[e]), int(lp[s]), int(lp[e])
    tp = g.tp.ptr.long()
    t0, t1 = int(tp[l0]), int(tp[l1])
    return {'glob.ptr': gp[s:e + 1] - g0, 'glob.row_of': g.glob.row_of[g0:g1] - s, 'glob.col': g.glob.col[g0:g1] - s,
            'dist_g': g.dist_g[g0:g1], 'loc.ptr': lp[s:e + 1] - l0, 'loc.row_of': g.loc.row_of[l0:l1] - s,
            'loc.col': g.loc.col[l0:l1] - s, 'dist_l': g.dist_l[l0:l1], 'tp.ptr': tp[l0:l1 + 1] - t0,
            'tp.row_of': g.tp.row_of[t0:t1] - l0, 'tp.col': g.tp.col[t0:t1] - l0, 'tp_angle': g.tp_angle[t0:t1],
            'tp_kind': g.tp_kind[t0:t1]}


@pytest.mark.gpu
@pytest.mark.parametrize('mode', [None, 'all'])
def test_a_molecule_in_a_mixed_batch_is_the_open_space_molecule(dev, mode):
    """{bulk cell, slab, molecule with pbc all False and a zero cell}: the molecule's slices of every index list, of dist and of
    the angles are torch.equal to its open-space build without `cell`; its energy within TOL = 1e-5 (relative) and its forces
    within grad_tol = 1e-5 (max-normalised) of its stand-alone open-space run.

    Its virial W = d E / d strain equals V = sum_a pos_a (x) dE/dpos_a to fp32 rounding.  The bound: the molecule's image
    integers are all zero (asserted on the fp64 geometry of test_pbc._geometry64), so every edge vector is the exact difference
    of two positions and the edge form sum_e v_e (x) dE/dv_e equals the atom form in exact arithmetic.  What differs is the
    rounding of each force component to fp32, a relative 2^-24, weighted by the position it is multiplied with --
    sum_a |pos_a|_inf |F_a|_inf -- and the rounding of W itself, 2^-24 max |W|; a factor 2 covers the different summation orders
    of the two fp64 accumulations.  (The positions lie 20 to 45 A from the origin: the bound is dominated by the first term.)"""
    import models
    from pamnet_amd import synth
    from test_hip_forces import KTOL, TOL, grad_tol
    structs = _mixed()
    mol = structs[2]
    s0 = structs[0].n + structs[1].n
    kw = dict(cell_images=mode) if mode else {}
    g = _build(_batch(structs, **kw), dev, need_grad=True, **kw)
    alone = synth.Batch(x=torch.from_numpy(mol.x), batch=torch.zeros(mol.n, dtype=torch.long), pos=torch.from_numpy(mol.pos),
                        num_graphs=1)
    g1 = _build(alone, dev, need_grad=True)
    assert g1.cell_tab is None and g.cell_tab is not None
    got, want = _molecule_slices(g, s0, s0 + mol.n), _molecule_slices(g1, 0, mol.n)
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
    assert want['dist_g'].numel() > 0 and want['dist_l'].numel() > 0 and want['tp_angle'].numel() > 0
    if mode:
        assert int(g.img_g[int(g.glob.ptr[s0]):].abs().max()) == 0
    # the fp64 geometry of the stand-alone molecule (a 1000 A cube: every image integer is zero)
    dg, dl, ang, (n_g, n_l) = _geometry64(g1, alone.pos.double(), alone.batch, torch.eye(3).view(1, 3, 3) * 1000.0)
    assert not n_g.any() and not n_l.any()
    assert maxnorm_err(want['dist_g'].cpu().numpy(), dg.numpy()) <= KTOL and maxnorm_err(want['tp_angle'].cpu().numpy(), ang.numpy()) <= KTOL
    torch.manual_seed(0)
    model = models.PAMNet(models.Config(dataset='QM9', dim=128, n_layer=2, cutoff_l=CUT_L, cutoff_g=CUT_G)).to(dev)
    e, f, w, _ = _energies(model, _batch(structs, **kw), dev)
    one = alone.to(dev)
    one.pos.requires_grad_(True)
    e1 = model(one)
    f1, = torch.autograd.grad(e1.sum(), one.pos)
    e1 = e1.detach()
    err_e = abs(float(e[2]) - float(e1[0])) / abs(float(e1[0]))
    err_f = maxnorm_err(f[s0:].cpu().numpy(), f1.cpu().numpy())
    print('molecule in the mixed batch: energy rel err', err_e, 'force err', err_f)
    assert err_e <= TOL and err_f <= grad_tol('QM9') and float(f1.abs().max()) > 0
    p64, f64 = torch.from_numpy(mol.pos).double(), f[s0:].cpu().double()
    V = (p64[:, :, None] * f64[:, None, :]).sum(0)
    W = w[2].cpu().double()
    bound = 2.0 * 2.0 ** -24 * (float((p64.abs().max(1)[0] * f64.abs().max(1)[0]).sum()) + float(W.abs().max()))
    print('virial: max |W - V|', float((W - V).abs().max()), 'bound', bound, 'max |W|', float(W.abs().max()))
    assert float(W.abs().max()) > 0 and float((W - V).abs().max()) <= bound


# --------------------------------------------------------------------------------------------- 6. an in-plane supercell
@pytest.mark.gpu
@pytest.mark.parametrize('dim,n_layer', [(128, 2), (16, 1)])
def test_an_in_plane_supercell_of_a_slab_has_twice_the_energy_and_the_same_forces(dev, dim, n_layer):
    """Max-normalised at 1e-5, the bound of test_pbc.test_a_supercell_has_twice_the_energy_and_the_same_forces."""
    import models
    torch.manual_seed(1)
    a, b = _super_slab()
    model = models.PAMNet(models.Config(dataset='QM9', dim=dim, n_layer=n_layer, cutoff_l=CUT_L, cutoff_g=CUT_G)).to(dev)

    def run(st):
        data = _batch([st]).to(dev)
        data.pos.requires_grad_(True)
        out = model(data)
        g = model._graph_cache
        f, = torch.autograd.grad(out.sum(), data.pos)
        return out.detach().cpu().double(), f.cpu().double(), g

    e_a, f_a, g_a = run(a)
    e_b, f_b, g_b = run(b)
    assert g_b.glob.m == 2 * g_a.glob.m and g_b.loc.m == 2 * g_a.loc.m and g_b.tp.m == 2 * g_a.tp.m and g_a.loc.m > 0
    assert torch.isfinite(e_a).all() and float(e_a.abs().max()) > 0 and float(f_a.abs().max()) > 0
    err_e = maxnorm_err(e_b.numpy(), (2 * e_a).numpy())
    err_f = maxnorm_err(f_b.view(2, a.n, 3).numpy(), f_a.view(1, a.n, 3).expand(2, a.n, 3).numpy())
    print('slab supercell: energy err', err_e, 'force err', err_f)
    assert err_e <= 1e-5 and err_f <= 1e-5, (err_e, err_f)


# ------------------------------------------------------------------------------------------------------- 7. refusals
@pytest.mark.gpu
def test_axes_refusals_say_what_to_do_instead(dev):
    import models
    from pamnet_amd import synth
    torch.manual_seed(0)
    model = models.PAMNet(models.Config(dataset='QM9', dim=16, n_layer=1, cutoff_l=CUT_L, cutoff_g=CUT_G)).to(dev)
    s = _structs()
    slab = s['slab_z']

    def with_cell(cell, pbc=(True, True, False), **kw):
        return _batch([Struct(slab.x, slab.pos, cell, (True, True, False), 2)], pbc=pbc, **kw).to(dev)

    good = with_cell(slab.cell)
    with torch.no_grad():
        assert torch.isfinite(model(good)).all()
        # a periodic axis whose lattice is too small or degenerate, on every route
        short = [[9.9, 0.0, 0.0], [0.0, 11.5, 0.0], [0.0, 0.0, 0.0]]
        flat = [[11.5, 0.0, 0.0], [23.0, 0.0, 0.0], [0.0, 0.0, 40.0]]
        for cell in (short, flat):
            for kw in (dict(), dict(mol_local=True)):
                with pytest.raises(ValueError, match='too small or singular') as info:
                    model(with_cell(cell, **kw))
                assert 'per axis' in str(info.value) and 'PERIODIC axes' in str(info.value)
            with pytest.raises(ValueError, match='too small or singular'):
                model.prepare(with_cell(cell), need_grad=False)
        for cell in ([[3.9, 0.0, 0.0], [0.0, 11.5, 0.0], [0.0, 0.0, 0.0]], [[11.5, 0.0, 0.0], [0.0, 1.2, 0.0], [0.0, 0.0, 0.0]]):
            with pytest.raises(ValueError, match='too small or singular') as info:     # <= 2 cutoff_l; below cutoff_g / 4
                model(with_cell(cell, cell_images='all'))
            assert 'per axis' in str(info.value) and "cell_images='all'" in str(info.value)
        # the same zero third vector without pbc: today's refusal, today's wording
        with pytest.raises(ValueError, match='singular') as info:
            model(with_cell(slab.cell, pbc=None))
        assert 'per axis' not in str(info.value)
        # pbc without cell
        b4 = synth.qm9_batch(0, 0, 2)
        free = synth.Batch(**{k: v for k, v in b4.__dict__.items() if k != 'edge_index'})
        for pbc in ((True, True, False), torch.ones(2, 3, dtype=torch.bool)):
            lone = free.to(dev)
            lone.pbc = pbc.to(dev) if isinstance(pbc, torch.Tensor) else pbc
            with pytest.raises(ValueError, match='`pbc` belongs to periodic batches'):
                model(lone)
        # dtype, shape, device, and sequences that are not three bools
        flags = torch.tensor([[True, True, False]], device=dev)
        for bad in (flags.to(torch.uint8), flags.float(), flags.view(3), flags.expand(2, 3).contiguous(), flags[:, :2].contiguous()):
            with pytest.raises(ValueError, match=r'torch.bool tensor of shape \[num_graphs, 3\]'):
                model(with_cell(slab.cell, pbc=bad))
        on_cpu = with_cell(slab.cell)
        on_cpu.pbc = flags.cpu()
        with pytest.raises(ValueError, match='device'):
            model(on_cpu)
        for bad in ((True, True), (True, True, False, False), (1, 1, 0), 'TTF', [True, None, False], np.array([True, True, False])):
            with pytest.raises(ValueError, match='three Python bools'):
                model(with_cell(slab.cell, pbc=bad))
        assert torch.equal(model(with_cell(slab.cell, pbc=[True, True, False])), model(good))    # a list is as good as a tuple


@pytest.mark.gpu
def test_without_pbc_and_with_three_true_neither_new_entry_point_is_called(dev, monkeypatch):
    """No pbc, pbc = None and the tuple (True, True, True): the twins' entry points and the same bits, in both modes."""
    import models
    s = _structs()
    tall = [_tall(s['slab_z']), _tall(s['slab_z2'])]
    torch.manual_seed(0)
    model = models.PAMNet(models.Config(dataset='QM9', dim=16, n_layer=1, cutoff_l=CUT_L, cutoff_g=CUT_G)).to(dev)
    calls = _record(monkeypatch)
    for mode in (None, 'all'):
        kw = dict(cell_images=mode) if mode else {}
        outs = []
        for pbc in (None, (True, True, True), [True, True, True]):
            data = _batch(tall, pbc=pbc, **kw).to(dev)
            data.pos.requires_grad_(True)
            out = model(data)
            f, = torch.autograd.grad(out.sum(), data.pos)
            outs.append((out.detach(), f))
        assert PREPARE in calls and (IMAGES in calls) == bool(mode) and not [c for c in calls if c in NEW], calls
        assert all(torch.equal(o, outs[0][0]) and torch.equal(f, outs[0][1]) for o, f in outs[1:])
        del calls[:]
        # the all-true TENSOR takes the new entry points and gives the same bits
        data = _batch(tall, pbc=torch.ones(2, 3, dtype=torch.bool), **kw).to(dev)
        data.pos.requires_grad_(True)
        out = model(data)
        f, = torch.autograd.grad(out.sum(), data.pos)
        assert PREPARE_AXES in calls and PREPARE not in calls and (IMAGES_AXES in calls) == bool(mode)
        assert torch.equal(out.detach(), outs[0][0]) and torch.equal(f, outs[0][1])
        del calls[:]
