"""Vibrational analysis on the device: mass-weighted Hessians by central differences of the model's forces, and their normal
modes by a batched symmetric eigensolver.

    from pamnet_amd import vib
    res = vib.run(model, data, delta=0.01, masses=m, fixed=bottom_layer)
    res.freq, res.modes, res.n_negative(1e-3), res.zero_point()          # per graph

The model has no second derivatives, so the displaced copies of a structure are graphs of one batch: one forward plus
torch.autograd.grad evaluates `pairs` central-difference pairs of every graph at once.  Each evaluation sits between two
launches of csrc/vib.hip -- pamnet_vib_displace_f32 builds the displaced batch, pamnet_vib_rows_f64 turns its dE/dpos into rows
of the packed Hessians -- and one launch of pamnet_sym_eig_f64 (csrc/eig.hip; one workgroup per matrix, cyclic Jacobi in fp64)
diagonalises them all.  include/pamnet_hip.h states the layout and the three rules.  The loop takes no decision on the host: the
only device -> host read is one at set-up.  Every element of a Hessian is stored once, from its own two gradients, and a
matrix is diagonalised by its own workgroup in a fixed order: for a model whose graphs do not interact a structure's
frequencies are bitwise the same alone or in any batch, for any `pairs`, and from run to run.  There is no CPU path.

Rigid translations and rotations are not projected out: their modes appear as the near-zero eigenvalues they are.
"""
import numpy as np
import torch

from . import graph as G
from . import lib
from .relax import _checked, _evaluate

MAX_FREE = 64                                     # free atoms per graph: d = 192 is the eigensolver's bound


class VibHessian(object):
    """hessian: the packed mass-weighted Hessians, fp64 [sum d_g^2] (graph g row-major at moff[g], d_g = 3 F_g; row and column
    3 f + c is free atom f, component c); moff, dptr: int64 [G + 1], the prefix sums of d_g^2 and d_g; fptr: int32 [G + 1] and
    free_idx: int32 [sum F_g], the free atoms of every graph, ascending; d_max: the largest d_g (a Python int); trace
    (trace=True: one dict of pos, dE and energy per evaluation, else None).  All tensors on the device."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class VibResult(VibHessian):
    """VibHessian (its `hessian` a clone taken before the solver consumes it) and: asym fp64 [G] (max |H - H^T| of the graph
    before symmetrisation: the gauge of finite-difference noise, reported, not judged); w fp64 [sum d_g] (the eigenvalues of
    graph g ascending at dptr[g]); modes (packed like the Hessian: row k of graph g is the unit eigenvector of w[k], mass-weighted
    coordinates); freq = sign(w) sqrt(|w|), in the caller's units (an imaginary frequency reads negative); status int32 [G] (0
    converged, 1 max_sweeps reached, 2 a non-finite Hessian); sweeps int32 [G]."""

    def _graph_of_row(self):
        n = self.w.numel()
        rows = torch.arange(n, device=self.w.device)
        return torch.searchsorted(self.dptr[1:].contiguous(), rows, right=True)

    def n_negative(self, threshold=0.0):
        """int64 [G]: the eigenvalues of every graph below -threshold (threshold >= 0, in the units of w)."""
        below = (self.w < -abs(float(threshold))).long()
        return torch.zeros(self.dptr.numel() - 1, dtype=torch.long, device=self.w.device).index_add_(0, self._graph_of_row(), below)

    def zero_point(self, hbar=1.0):
        """fp64 [G]: 1/2 hbar sum sqrt(w) over the eigenvalues w > 0 of every graph (summed row by row of a padded table)."""
        n_graphs, dev = self.dptr.numel() - 1, self.w.device
        if self.w.numel() == 0:
            return torch.zeros(n_graphs, dtype=torch.float64, device=dev)
        col = torch.arange(max(self.d_max, 1), device=dev)[None]
        at = (self.dptr[:-1, None] + col).clamp(max=self.w.numel() - 1)
        inside = col < (self.dptr[1:] - self.dptr[:-1])[:, None]
        wv = self.w[at]
        root = torch.where(inside & (wv > 0), wv.clamp(min=0.0).sqrt(), torch.zeros_like(wv))
        return 0.5 * float(hbar) * root.sum(1)


# ------------------------------------------------------------------------------------------------------ the launches
def displace(pos0, gptr, fptr, free_idx, pairs, t, delta, pos_out):
    """Evaluation t of the displaced batch (one launch, no synchronisation): writes pos_out fp32 [2 pairs n, 3], every copy pos0
    [n, 3] bit for bit but the displaced coordinate of each active pair.  gptr, fptr: int32 [G + 1]; free_idx: int32."""
    lib.call('pamnet_vib_displace_f32', lib.ptr(pos0), lib.ptr(gptr), lib.ptr(fptr), lib.ptr(free_idx), pos0.size(0),
             gptr.numel() - 1, int(pairs), int(t), float(delta), lib.ptr(pos_out), lib.stream_of(pos0))


def hessian_rows(dpos, pos0, fptr, free_idx, moff, pairs, t, delta, h, masses=None):
    """The rows of evaluation t (one launch, no synchronisation): from dpos fp32 [2 pairs n, 3], the dE/dpos of the batch
    displace() made, into the packed fp64 `h`.  moff: int64 [G + 1]; masses: fp32 [n] or None."""
    lib.call('pamnet_vib_rows_f64', lib.ptr(dpos), lib.ptr(pos0), lib.ptr(masses), lib.ptr(fptr), lib.ptr(free_idx), lib.ptr(moff),
             pos0.size(0), fptr.numel() - 1, int(pairs), int(t), float(delta), lib.ptr(h), lib.stream_of(pos0))


def eigh(a, moff, dptr, tol=1e-15, max_sweeps=30, v=None, w=None, status=None, sweeps=None):
    """Eigenvalues and eigenvectors of a packed batch of symmetric fp64 matrices (one launch, one workgroup per matrix, d <= 192)
    -> (w, v, status, sweeps).  a: fp64, matrix g row-major at moff[g], read as (A + A^T) / 2 and CONSUMED as workspace; moff,
    dptr: int64 [G + 1] on the device, the prefix sums of d_g^2 and d_g.  w[dptr[g] ..] ascending; row k of v at moff[g] the unit
    eigenvector of w[k], its largest component positive.  Outputs that are not given are allocated; allocating `w` reads
    dptr[-1] from the device (the only synchronisation)."""
    n_mat = dptr.numel() - 1
    dev = a.device
    if v is None:
        v = torch.zeros_like(a)
    if w is None:
        w = torch.zeros(int(dptr[-1]), dtype=torch.float64, device=dev)
    if status is None:
        status = torch.zeros(n_mat, dtype=torch.int32, device=dev)
    if sweeps is None:
        sweeps = torch.zeros(n_mat, dtype=torch.int32, device=dev)
    lib.call('pamnet_sym_eig_f64', lib.ptr(a), lib.ptr(v), lib.ptr(w), lib.ptr(status), lib.ptr(sweeps), lib.ptr(moff),
             lib.ptr(dptr), n_mat, float(tol), int(max_sweeps), lib.stream_of(a))
    return w, v, status, sweeps


# ---------------------------------------------------------------------------------------------------------- drivers
def _replicated(data, batch, n, n_graphs, copies, device):
    """The batch `copies` times over, copy-major (the fields neb.interpolate replicates): graph g of copy k is graph
    k n_graphs + g, its atoms follow those of copy k - 1.  `pos` is attached by every evaluation.  Index arithmetic on the
    device, no read."""
    from .synth import Batch
    k = torch.arange(copies, device=device)
    out = Batch(batch=(batch[None] + (k * n_graphs).to(batch.dtype)[:, None]).reshape(-1), num_graphs=copies * n_graphs)
    x, ei = getattr(data, 'x', None), getattr(data, 'edge_index', None)
    if x is not None:
        out.x = x.repeat((copies,) + (1,) * (x.dim() - 1))
    if ei is not None:
        out.edge_index = (ei[:, None, :] + (k * n).to(ei.dtype)[None, :, None]).reshape(2, -1)
    for name in ('cell', 'pbc', 'cell_images', 'mol_local'):
        v = getattr(data, name, None)
        if v is None:
            continue
        per_graph = isinstance(v, torch.Tensor) and v.dim() >= 1 and v.size(0) == n_graphs
        setattr(out, name, v.repeat((copies,) + (1,) * (v.dim() - 1)) if per_graph else v)
    return out


def hessian(model, data, delta=0.01, masses=None, fixed=None, pairs=4, trace=False):
    """The mass-weighted Hessian of every graph of `data` by central differences of dE/dpos -> VibHessian.

    model:  as for relax(): any callable with model(data) -> [G] that is differentiable with respect to `data.pos` (QM9 schema).
    data:   the batch; `data.pos` is never written.
    delta:  the displacement, finite and positive, in the caller's length unit.  The divisor of every difference is the
            displacement as it was realised in fp32.
    masses: fp32 [N] on the device, positive; None: unit masses (the plain Hessian).
    fixed:  bool [N] on the device (True: the atom is not displaced and has no rows or columns), or None.  A graph has at most
            64 free atoms.
    pairs:  the central-difference pairs of every graph in one evaluation: the evaluated batch is 2 pairs copies of `data`, and
            there are ceil(3 max F_g / pairs) evaluations.
    trace:  keep, per evaluation, clones of the displaced positions, dE/dpos and the energies.

    Set-up is plain torch with one device -> host read (the free atoms of every graph, and that the masses are positive and
    finite); the loop is displace launch, evaluation, rows launch, and reads nothing."""
    try:
        delta = float(delta)
    except (TypeError, ValueError):
        raise ValueError('`delta` is a float; got %r' % (type(delta),))
    if not (0.0 < delta < float('inf')):
        raise ValueError('`delta` must be finite and positive; got %r' % (delta,))
    if int(pairs) != pairs or pairs < 1 or pairs > 32767:
        raise ValueError('`pairs` is a count of central-difference pairs per evaluation, 1 .. 32767; got %r' % (pairs,))
    pairs = int(pairs)
    pos, batch, n_graphs, _, fixed8 = _checked(model, data, 0.0, fixed)
    device, n = pos.device, pos.size(0)
    if masses is not None:
        if (not isinstance(masses, torch.Tensor) or masses.dtype != torch.float32 or tuple(masses.shape) != (n,)
                or masses.device != device):
            raise ValueError('`masses` is a float32 tensor [N] = [%d] on the device of `pos`; got %s'
                             % (n, '%s %s on %s' % (masses.dtype, tuple(masses.shape), masses.device)
                                if isinstance(masses, torch.Tensor) else type(masses)))
        masses = masses.detach().contiguous()

    # ---- set-up: the free atoms of every graph, and one read
    pos0 = pos.detach().to(torch.float32).clone().contiguous()
    gptr, _ = G.csr_from_keys(batch.to(torch.int32).contiguous(), n_graphs)
    free = torch.ones(n, dtype=torch.bool, device=device) if fixed8 is None else fixed8 == 0
    running = torch.cat([torch.zeros(1, dtype=torch.long, device=device), free.long().cumsum(0)])
    fptr64 = running[gptr.long()]                                 # free atoms before each graph
    order = torch.sort((~free).to(torch.uint8), stable=True)[1]   # the free atoms first, ascending
    ok = (torch.isfinite(masses) & (masses > 0)).all() if masses is not None else torch.ones((), dtype=torch.bool, device=device)
    host = torch.cat([ok.long().view(1), fptr64]).tolist()        # the one read
    if not host[0]:
        raise ValueError('`masses` must be positive and finite in every entry')
    fptr_h = np.asarray(host[1:], dtype=np.int64)
    counts = fptr_h[1:] - fptr_h[:-1]
    if len(counts) and counts.max() > MAX_FREE:
        raise ValueError('a graph has at most %d free atoms (a matrix of dimension 192: the eigensolver works on it in one '
                         'workgroup); graph %d has %d -- fix the atoms that do not take part' % (MAX_FREE, int(counts.argmax()),
                                                                                                 int(counts.max())))
    f_max = int(counts.max()) if len(counts) else 0
    total = int((9 * counts * counts).sum())
    fptr = fptr64.to(torch.int32).contiguous()
    free_idx = order[:int(fptr_h[-1])].to(torch.int32).contiguous()
    dims = 3 * (fptr64[1:] - fptr64[:-1])
    zero = torch.zeros(1, dtype=torch.long, device=device)
    dptr, moff = torch.cat([zero, dims.cumsum(0)]), torch.cat([zero, (dims * dims).cumsum(0)])

    rep = _replicated(data, batch, n, n_graphs, 2 * pairs, device)
    pos_out = torch.empty(2 * pairs * n, 3, dtype=torch.float32, device=device)
    h = torch.zeros(total, dtype=torch.float64, device=device)
    log = [] if trace else None
    for t in range((3 * f_max + pairs - 1) // pairs):
        displace(pos0, gptr, fptr, free_idx, pairs, t, delta, pos_out)
        e, de = _evaluate(model, rep, pos_out)
        if trace:
            log.append(dict(pos=pos_out.clone(), dE=de.clone(), energy=e.clone()))
        hessian_rows(de, pos0, fptr, free_idx, moff, pairs, t, delta, h, masses)
    return VibHessian(hessian=h, moff=moff, dptr=dptr, fptr=fptr, free_idx=free_idx, d_max=3 * f_max, trace=log)


def _asymmetry(h, moff, dptr):
    """max |H - H^T| of every packed matrix, fp64 [G]: index arithmetic on the device, no read."""
    n_graphs = dptr.numel() - 1
    out = torch.zeros(n_graphs, dtype=torch.float64, device=h.device)
    if h.numel() == 0:
        return out
    e = torch.arange(h.numel(), device=h.device)
    g = torch.searchsorted(moff[1:].contiguous(), e, right=True)
    d = (dptr[1:] - dptr[:-1])[g]
    local = e - moff[g]
    p, q = torch.div(local, d, rounding_mode='floor'), local % d
    return out.scatter_reduce(0, g, (h - h[moff[g] + q * d + p]).abs(), 'amax')


def run(model, data, delta=0.01, masses=None, fixed=None, pairs=4, trace=False, tol=1e-15, max_sweeps=30):
    """hessian(), then one launch of the eigensolver -> VibResult, all on the device.  delta, masses, fixed, pairs, trace: as
    for hessian().  tol, max_sweeps: the solver stops when the off-diagonal norm is below tol |H|_F, or after max_sweeps sweeps
    (status 1).  A relaxed structure is a minimum where res.n_negative(threshold) is 0, a climbing image a transition state where
    it is 1, with `threshold` above the size of the rigid-body modes and of res.asym."""
    if not (float(tol) >= 0.0) or int(max_sweeps) != max_sweeps or max_sweeps < 1:
        raise ValueError('`tol` is not negative and `max_sweeps` a count >= 1; got %r and %r' % (tol, max_sweeps))
    hs = hessian(model, data, delta=delta, masses=masses, fixed=fixed, pairs=pairs, trace=trace)
    device, n_graphs = hs.hessian.device, hs.dptr.numel() - 1
    kept = hs.hessian.clone()
    asym = _asymmetry(kept, hs.moff, hs.dptr)
    n_rows = 3 * int(hs.free_idx.numel())
    w = torch.zeros(n_rows, dtype=torch.float64, device=device)
    w, modes, status, sweeps = eigh(hs.hessian, hs.moff, hs.dptr, tol, max_sweeps, w=w)
    return VibResult(hessian=kept, asym=asym, w=w, modes=modes, freq=torch.sign(w) * w.abs().sqrt(), status=status, sweeps=sweeps,
                     moff=hs.moff, dptr=hs.dptr, fptr=hs.fptr, free_idx=hs.free_idx, d_max=hs.d_max, trace=hs.trace)
