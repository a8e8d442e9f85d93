"""Batched minimum-energy paths on the device: the nudged elastic band with the improved tangent (Henkelman & Jonsson, J. Chem.
Phys. 113, 9978, 2000) and a climbing image (Henkelman, Uberuaga & Jonsson, J. Chem. Phys. 113, 9901, 2000) over the forces of a
model.

    from pamnet_amd import neb
    band = neb.interpolate(initial, final, n_images=9)          # two batches of B minima -> one batch of 9 B images
    res = neb.run(model, band, fmax=0.05, k=0.1, climb_after=40)
    res.barrier_fwd, res.barrier_rev, res.saddle                # per band

The images of a band are consecutive graphs of one batch (`data.band_ptr`), so one forward plus torch.autograd.grad evaluates
every image of every band at once.  Each iteration is that evaluation and two launches: pamnet_neb_force_f32 (csrc/neb.hip; one
workgroup per image; include/pamnet_hip.h states the rule) turns dE/dpos into the projected gradient, and
pamnet_fire_step_f32 (csrc/relax.hip) moves the bands, its "graphs" being the bands.  FIRE state, convergence and failure are
therefore per band, a band's trajectory does not depend on its batch-mates, and it is bitwise repeatable.  The loop takes no
decision on the host: the only device -> host reads are one at set-up and the status vector every `check_every` steps.  There is
no CPU path.
"""
import numpy as np
import torch

from . import graph as G
from . import lib
from .relax import CONVERGED, FAILED, RUNNING, STATE, _checked, _evaluate, _fire_params, fire_step, new_state


class NebResult(object):
    """pos [N, 3] fp32 (a new tensor); energy [G], forces [N, 3] (the true forces) and neb_forces [N, 3] (the projected ones) of
    one evaluation at `pos`; converged / failed bool [B]; steps int32 [B] (the FIRE steps a band moved); fmax [B] (the largest
    projected force of the band's last step); saddle int64 [B] (the graph index of the highest interior image); barrier_fwd /
    barrier_rev [B] (the saddle's energy minus the first / last image's); distance fp64 [G] (the path length from the band's
    first image, image to image); fpar fp64 [G] (F . t^, 0 on endpoints); trace (trace=True: one dict per step, else None).
    All on the device."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


# ------------------------------------------------------------------------------------------------------- the launch
def neb_force(pos, dpos, energy, gptr, band_ptr, band_of, dneb, k, seg=None, fpar=None, fixed=None, band_status=None, climb=None):
    """One projection of every image (one launch, no synchronisation): writes dneb = -F_neb (fp32 [n, 3]), seg and fpar (fp64
    [G], or None).  pos, dpos: fp32 [n, 3]; energy: fp32 [G]; gptr: int32 [G + 1]; band_ptr: int32 [B + 1]; band_of: int32 [G];
    k: a float, or fp64 [B]; fixed: uint8 / bool [n] or None; band_status: int32 [B] or None (nonzero: the band is left alone);
    climb: uint8 / bool [B] or None."""
    per_band = isinstance(k, torch.Tensor)
    lib.call('pamnet_neb_force_f32', lib.ptr(pos), lib.ptr(dpos), lib.ptr(energy), lib.ptr(fixed), lib.ptr(gptr), pos.size(0),
             gptr.numel() - 1, lib.ptr(band_ptr), lib.ptr(band_of), band_ptr.numel() - 1, lib.ptr(band_status), lib.ptr(climb),
             lib.ptr(k) if per_band else None, 0.0 if per_band else float(k), lib.ptr(dneb), lib.ptr(seg), lib.ptr(fpar),
             lib.stream_of(pos))


# ------------------------------------------------------------------------------------------------------ interpolate
def _inv3(m):
    """Inverse of [G, 3, 3] by the adjugate, written out (elementwise launches: no factorisation, no synchronisation)."""
    c = lambda i, j: (m[:, (i + 1) % 3, (j + 1) % 3] * m[:, (i + 2) % 3, (j + 2) % 3]
                      - m[:, (i + 1) % 3, (j + 2) % 3] * m[:, (i + 2) % 3, (j + 1) % 3])
    cof = torch.stack([torch.stack([c(i, j) for j in range(3)], 1) for i in range(3)], 1)       # cof[i][j], cyclic: signs included
    det = (m[:, 0, :] * cof[:, 0, :]).sum(1)
    return cof.transpose(1, 2) / det[:, None, None]


_SHIFTS = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]


def minimum_image(d, cell, periodic, batch):
    """The displacements d [N, 3] (fp64) of atoms of the graphs `batch` reduced to their shortest periodic image: the fractional
    coordinates along the periodic vectors (rows k of cell [G, 3, 3] with periodic [G, 3] True) are rounded to the nearest
    integer, and the 27 lattice translations around that are searched for the shortest (exact for a cell whose rounded image is
    within one lattice step of the shortest: any cell that is not pathologically skewed).  An open axis is not reduced."""
    a = cell.to(torch.float64) * periodic.to(torch.float64)[:, :, None]           # open rows zeroed
    gram = a @ a.transpose(1, 2) + torch.diag_embed((~periodic).to(torch.float64))
    a_n = a[batch]
    frac = torch.einsum('nj,nkj->nk', d, a_n)[:, None, :] @ _inv3(gram)[batch]     # [N, 1, 3]
    n0 = torch.round(frac[:, 0, :])
    shifts = n0[:, None, :] + torch.tensor(_SHIFTS, dtype=torch.float64, device=d.device)[None]       # [N, 27, 3]
    cand = d[:, None, :] - torch.einsum('nsk,nkj->nsj', shifts, a_n)
    best = (cand * cand).sum(2).argmin(1)
    return cand[torch.arange(d.size(0), device=d.device), best]


def _periodic_axes(data, n_graphs, device):
    """bool [G, 3] of the batch's periodic axes, or None where it has no cell (`cell` alone means fully periodic)."""
    if getattr(data, 'cell', None) is None:
        return None
    pbc = getattr(data, 'pbc', None)
    if pbc is None:
        return torch.ones(n_graphs, 3, dtype=torch.bool, device=device)
    if isinstance(pbc, torch.Tensor):
        if pbc.dtype != torch.bool or tuple(pbc.shape) != (n_graphs, 3):
            raise ValueError('`pbc` is a torch.bool tensor [num_graphs, 3] = [%d, 3], or a tuple of three bools; got %s %s'
                             % (n_graphs, pbc.dtype, tuple(pbc.shape)))
        return pbc.to(device)
    flags = [bool(v) for v in pbc]
    if len(flags) != 3:
        raise ValueError('`pbc` is a torch.bool tensor [num_graphs, 3] or a tuple of three bools; got %r' % (pbc,))
    return torch.tensor(flags, dtype=torch.bool).to(device)[None].expand(n_graphs, 3).contiguous()


def interpolate(initial, final, n_images):
    """One batch of bands between the B graphs of `initial` and the B graphs of `final` (the same atoms per graph in the same
    order): band b is `n_images[b]` consecutive graphs (an int: the same for every band; endpoints included, at least 3), image j
    at initial + j / (n_images - 1) (final - initial).  On periodic axes (`cell` with `pbc`, or `cell` alone: fully periodic) the
    displacement final - initial is reduced to its minimum image first, so the band is continuous in unwrapped coordinates and
    its last image is `final` up to a lattice translation per atom.

    x, batch, num_graphs, edge_index (offset per image), cell, pbc, cell_images and mol_local are replicated per image from
    `initial`; `band_ptr` (int32 [B + 1]) is attached.  Plain torch at set-up, one device -> host read (the endpoints' cells, atom
    types and graph ids must agree: ValueError)."""
    from .synth import Batch
    pos_i, pos_f, batch = getattr(initial, 'pos', None), getattr(final, 'pos', None), getattr(initial, 'batch', None)
    if pos_i is None or pos_f is None or batch is None or getattr(final, 'batch', None) is None:
        raise ValueError('interpolate needs `pos` and `batch` on both endpoint batches')
    if pos_i.dim() != 2 or pos_i.size(1) != 3 or tuple(pos_f.shape) != tuple(pos_i.shape) or batch.numel() != pos_i.size(0) \
            or final.batch.numel() != pos_i.size(0):
        raise ValueError('the endpoint batches must hold the same atoms: `pos` [N, 3] with one `batch` entry per row; got %s / %s '
                         'and %s / %s' % (tuple(pos_i.shape), tuple(batch.shape), tuple(pos_f.shape), tuple(final.batch.shape)))
    device = pos_i.device
    if pos_f.device != device:
        raise ValueError('the endpoint batches are on different devices: %s and %s' % (device, pos_f.device))
    ng = getattr(initial, 'num_graphs', None)
    B = int(ng) if ng is not None else (int(batch[-1]) + 1 if batch.numel() else 0)
    if isinstance(n_images, (list, tuple)):
        images = [int(v) for v in n_images]
        if len(images) != B:
            raise ValueError('`n_images` is an int or a list of num_graphs = %d ints; got %d entries' % (B, len(images)))
    else:
        images = [int(n_images)] * B
    if any(v < 3 for v in images):
        raise ValueError('a band has at least 3 images (the endpoints included); got n_images = %r' % (n_images,))
    cell, x, ei = getattr(initial, 'cell', None), getattr(initial, 'x', None), getattr(initial, 'edge_index', None)
    same = [(batch == final.batch).all()]
    for name, u, v in (('cell', cell, getattr(final, 'cell', None)), ('x', x, getattr(final, 'x', None))):
        if (u is None) != (v is None) or (u is not None and tuple(u.shape) != tuple(v.shape)):
            raise ValueError('the endpoints must share their %s: `%s` differs in presence or shape' % (
                'cell' if name == 'cell' else 'atom types', name))
        if u is not None:
            same.append((u == v).all())
    counts = torch.bincount(batch.long(), minlength=B)
    ecount = torch.bincount(batch.long()[ei[0].long()], minlength=B) if ei is not None else counts.new_zeros(0)
    host = torch.cat([torch.stack(same).all().long().view(1), counts, ecount]).tolist()               # the one read
    if not host[0]:
        raise ValueError('the endpoints of a band must share their cell, their atom types (`x`) and their graph ids (`batch`), '
                         'atom by atom: `initial` and `final` differ')
    counts_h, ecount_h = np.asarray(host[1:1 + B], dtype=np.int64), np.asarray(host[1 + B:], dtype=np.int64)
    aptr = np.concatenate([[0], np.cumsum(counts_h)])

    periodic = _periodic_axes(initial, B, device)
    d = pos_f.to(torch.float64) - pos_i.to(torch.float64)
    if periodic is not None:
        d = minimum_image(d, cell, periodic, batch.long())

    # host-side index arithmetic: new graph (b, j) copies graph b
    graph_src = np.repeat(np.arange(B), images)
    frac = np.concatenate([np.arange(m) / float(m - 1) for m in images]) if B else np.zeros(0)
    band_ptr = np.concatenate([[0], np.cumsum(images)]).astype(np.int32)
    new_counts = counts_h[graph_src]
    new_aptr = np.concatenate([[0], np.cumsum(new_counts)])
    atom_src = np.concatenate([np.arange(aptr[b], aptr[b + 1]) for b in graph_src]) if len(graph_src) else np.zeros(0, np.int64)
    atom_graph = np.repeat(np.arange(len(graph_src)), new_counts)
    up = lambda arr, dtype: torch.from_numpy(np.ascontiguousarray(arr)).to(dtype).to(device)
    src, t = up(atom_src, torch.long), up(frac[atom_graph], torch.float64)
    gsrc = up(graph_src, torch.long)
    out = Batch(pos=(pos_i.to(torch.float64)[src] + t[:, None] * d[src]).to(torch.float32),
                batch=up(atom_graph, batch.dtype), num_graphs=int(len(graph_src)), band_ptr=up(band_ptr, torch.int32))
    if x is not None:
        out.x = x[src]
    if ei is not None:
        order = torch.sort(batch.long()[ei[0].long()], stable=True)[1]                                # edges grouped by graph
        eptr = np.concatenate([[0], np.cumsum(ecount_h)])
        e_src = np.concatenate([np.arange(eptr[b], eptr[b + 1]) for b in graph_src]) if len(graph_src) else np.zeros(0, np.int64)
        e_off = np.repeat(new_aptr[:-1] - aptr[graph_src], ecount_h[graph_src])
        out.edge_index = ei[:, order][:, up(e_src, torch.long)] + up(e_off, ei.dtype)[None]
    for name in ('cell', 'pbc', 'cell_images', 'mol_local'):
        v = getattr(initial, name, None)
        if v is None:
            continue
        per_graph = isinstance(v, torch.Tensor) and v.dim() >= 1 and v.size(0) == B
        setattr(out, name, v[gsrc.to(v.device)] if per_graph else v)
    return out


# -------------------------------------------------------------------------------------------------------------- run
def _per_band(name, v, n_bands, device, dtype, what):
    """A float, or a tensor [B] of `dtype` on the device of pos (contiguous), in the style of relax._checked."""
    if isinstance(v, torch.Tensor):
        if v.dtype != dtype or tuple(v.shape) != (n_bands,) or v.device != device:
            raise ValueError('a per-band `%s` is a %s tensor [num_bands] = [%d] on the device of `pos`; got %s %s on %s'
                             % (name, str(dtype).replace('torch.', ''), n_bands, v.dtype, tuple(v.shape), v.device))
        return v.detach().contiguous()
    try:
        return float(v)
    except (TypeError, ValueError):
        raise ValueError('`%s` (%s) is a float, or a %s tensor [num_bands] on the device of `pos`; got %r'
                         % (name, what, str(dtype).replace('torch.', ''), type(v)))


def _energies(e, n_graphs):
    if e.numel() != n_graphs:
        raise ValueError('the model must return one energy per graph: got %s for %d graphs' % (tuple(e.shape), n_graphs))
    return e.reshape(-1).to(torch.float32).contiguous()


def run(model, data, fmax=0.05, k=0.1, climb_after=None, max_steps=500, fixed=None, check_every=10, trace=False, **fire_params):
    """Relax every band of `data` (interpolate() makes one) to its minimum-energy path, until the largest projected force on a
    free atom of the band's interior images is below `fmax`, or for `max_steps` steps.

    model:  as for relax(): any callable with model(data) -> [G] that is differentiable with respect to `data.pos`.
    data:   the batch of images, with `data.band_ptr` (int32 / int64 [B + 1] on the device: band b is the consecutive graphs
            band_ptr[b] .. band_ptr[b + 1] - 1, at least 3, with equal atom counts).  `data.pos` is never written.  The first and
            last image of a band do not move.  Positions are unwrapped: the projection takes no cell.
    fmax:   the convergence threshold on the projected force, a float or fp32 [B] on the device.
    k:      the spring constant, a float or fp64 [B] on the device; not negative.
    climb_after: None: plain NEB.  0: a climbing image from the first step.  m: at iteration m the climbing image is switched on,
            the bands' FIRE state starts afresh (vel = 0, dt = dt0, a = a0, n_pos = 0) and converged bands run again; failed
            bands stay failed.  Elementwise on the device, no read.
    fixed:  bool [N] on the device (True: the atom does not move and enters no sum of the projection), or None; expected to be
            the same on every image of a band.
    check_every: the status vector is read every so many steps, to stop when no band is running (and the climbing image, if
            asked for, is on); 0: never.
    trace:  keep, per step, clones of pos, dE, energy, climb, dneb, seg, fpar, vel and the state before and after, in res.trace.
    fire_params: dt0, dt_max, max_step, n_min, f_inc, f_dec, a0, f_a (relax.FIRE_DEFAULTS).

    One read at set-up checks that band_ptr is sorted and covers all graphs, that every band has at least 3 images of equal atom
    counts, and that per-band tensors are finite.  One more evaluation and projection at the end: everything returned belongs
    to res.pos."""
    p = _fire_params(fire_params)
    band_ptr = getattr(data, 'band_ptr', None)
    if band_ptr is None:
        raise ValueError('neb.run needs `data.band_ptr` (int32 [num_bands + 1]: band b is the consecutive graphs band_ptr[b] .. '
                         'band_ptr[b + 1] - 1); the batch has no `band_ptr` -- neb.interpolate() attaches one')
    pos, batch, n_graphs, _, fixed8 = _checked(model, data, 0.0, fixed)
    device = pos.device
    if (not isinstance(band_ptr, torch.Tensor) or band_ptr.dtype not in (torch.int32, torch.int64) or band_ptr.dim() != 1
            or band_ptr.numel() < 2 or band_ptr.device != device):
        raise ValueError('`data.band_ptr` is an int32 / int64 tensor [num_bands + 1] (at least one band) on the device of `pos`; '
                         'got %s' % ('%s %s on %s' % (band_ptr.dtype, tuple(band_ptr.shape), band_ptr.device)
                                     if isinstance(band_ptr, torch.Tensor) else type(band_ptr)))
    B = band_ptr.numel() - 1
    tol = _per_band('fmax', fmax, B, device, torch.float32, 'the threshold on the projected force')
    kb = _per_band('k', k, B, device, torch.float64, 'the spring constant')
    if climb_after is not None and (int(climb_after) != climb_after or climb_after < 0):
        raise ValueError('`climb_after` is None or a step count >= 0; got %r' % (climb_after,))
    if isinstance(tol, float) and tol != tol:
        raise ValueError('`fmax` must not be NaN')
    if isinstance(kb, float) and not (0.0 <= kb < float('inf')):
        raise ValueError('`k` must be finite and not negative; got %r' % (kb,))

    # ---- set-up: the band layout on the device, and one read for every check at once
    bp = band_ptr.to(torch.int32).contiguous()
    bp64 = bp.long()
    gptr, _ = G.csr_from_keys(batch.to(torch.int32).contiguous(), n_graphs)
    ar = torch.arange(n_graphs, device=device)
    band_of64 = torch.searchsorted(bp64[1:].contiguous(), ar, right=True).clamp(max=B - 1)
    first = bp64[band_of64].clamp(0, max(n_graphs - 1, 0))
    last = (bp64[band_of64 + 1] - 1).clamp(0, max(n_graphs - 1, 0))
    counts = gptr[1:] - gptr[:-1]
    checks = [(counts == counts[first]).all() if n_graphs else torch.ones((), dtype=torch.bool, device=device),
              (torch.isfinite(kb) & (kb >= 0)).all() if isinstance(kb, torch.Tensor) else torch.ones((), dtype=torch.bool, device=device),
              torch.isfinite(tol).all() if isinstance(tol, torch.Tensor) else torch.ones((), dtype=torch.bool, device=device)]
    host = torch.cat([torch.stack(checks).long(), bp64]).tolist()                                     # the one read
    bp_h = host[3:]
    if bp_h[0] != 0 or bp_h[-1] != n_graphs or any(b < a for a, b in zip(bp_h[:-1], bp_h[1:])):
        raise ValueError('`data.band_ptr` must be sorted, start at 0 and end at num_graphs = %d; got %r' % (n_graphs, bp_h))
    if any(b - a < 3 for a, b in zip(bp_h[:-1], bp_h[1:])):
        raise ValueError('every band needs at least 3 images (two endpoints and one that moves); band sizes are %r'
                         % ([b - a for a, b in zip(bp_h[:-1], bp_h[1:])],))
    if not host[0]:
        raise ValueError('the images of a band must have the same number of atoms (matched by their order)')
    if not host[1]:
        raise ValueError('`k` must be finite and not negative in every entry')
    if not host[2]:
        raise ValueError('`fmax` must be finite in every entry')
    longest = max(b - a for a, b in zip(bp_h[:-1], bp_h[1:]))

    band_of = band_of64.to(torch.int32).contiguous()
    aptr = gptr[bp64].contiguous()                                # the bands as the "graphs" of the FIRE step
    is_end = (ar == first) | (ar == last)
    move_fixed = is_end[batch.long()]
    if fixed8 is not None:
        move_fixed = move_fixed | (fixed8 != 0)
    move_fixed = move_fixed.to(torch.uint8).contiguous()          # the step's mask: the caller's, and the endpoint images
    kernel_params = {name: v for name, v in p.items() if name != 'dt0'}
    cur = pos.detach().to(torch.float32).clone().contiguous()
    vel, state = new_state(cur.size(0), B, device, p['dt0'], p['a0'])
    climb = torch.full((B,), 1 if climb_after == 0 else 0, dtype=torch.uint8, device=device)
    dneb = torch.zeros_like(cur)
    seg = torch.zeros(n_graphs, dtype=torch.float64, device=device)
    fpar = torch.zeros(n_graphs, dtype=torch.float64, device=device)
    steps_log = [] if trace else None
    for it in range(int(max_steps)):
        if climb_after and it == climb_after:     # the climbing image comes on: a fresh FIRE state, converged bands run again
            climb.fill_(1)
            vel.zero_()
            state['dt'].fill_(float(p['dt0']))
            state['a'].fill_(float(p['a0']))
            state['n_pos'].zero_()
            state['status'].masked_fill_(state['status'] == CONVERGED, RUNNING)
        e, de = _evaluate(model, data, cur)
        e = _energies(e, n_graphs)
        if trace:
            rec = dict(pos=cur.clone(), dE=de.clone(), energy=e.clone(), climb=climb.clone(), dneb_before=dneb.clone(),
                       seg_before=seg.clone(), fpar_before=fpar.clone(), v_before=vel.clone(),
                       state_before={name: state[name].clone() for name in STATE})
        neb_force(cur, de, e, gptr, bp, band_of, dneb, kb, seg, fpar, fixed8, state['status'], climb)
        if trace:
            rec.update(dneb=dneb.clone(), seg=seg.clone(), fpar=fpar.clone())
        fire_step(cur, vel, dneb, aptr, state, tol, move_fixed, **kernel_params)
        if trace:
            rec.update(pos_after=cur.clone(), v_after=vel.clone(), state_after={name: state[name].clone() for name in STATE})
            steps_log.append(rec)
        climbing_is_on = climb_after is None or it >= climb_after
        if check_every and (it + 1) % int(check_every) == 0 and climbing_is_on and not bool((state['status'] == RUNNING).any()):
            break

    # ---- one more evaluation and projection (of every band, finished or not): the result belongs to the returned geometry
    energy, de = _evaluate(model, data, cur)
    energy = _energies(energy, n_graphs)
    dneb = torch.zeros_like(cur)
    neb_force(cur, de, energy, gptr, bp, band_of, dneb, kb, seg, fpar, fixed8, None, climb)
    neg_inf = torch.full_like(energy, float('-inf'))
    e_in = torch.where(is_end, neg_inf, energy)
    top = torch.full((B,), float('-inf'), dtype=energy.dtype, device=device).scatter_reduce(0, band_of64, e_in, 'amax')
    cand = torch.where(~is_end & (e_in == top[band_of64]), ar, torch.full_like(ar, n_graphs))
    saddle = torch.full((B,), n_graphs, dtype=ar.dtype, device=device).scatter_reduce(0, band_of64, cand, 'amin')
    saddle = torch.where(saddle == n_graphs, bp64[:-1] + 1, saddle)               # (no finite interior energy: the first one)
    distance = torch.zeros_like(seg)
    offset = ar - first
    for j in range(1, longest):                   # image by image: the same additions whatever else the batch holds
        distance = torch.where(offset == j, torch.roll(distance, 1) + seg, distance)
    return NebResult(pos=cur, energy=energy, forces=-de, neb_forces=-dneb, converged=state['status'] == CONVERGED,
                     failed=state['status'] == FAILED, steps=state['steps'], fmax=state['fmax'], saddle=saddle,
                     barrier_fwd=energy[saddle] - energy[bp64[:-1]], barrier_rev=energy[saddle] - energy[bp64[1:] - 1],
                     distance=distance, fpar=fpar, trace=steps_log)
