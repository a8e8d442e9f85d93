"""Batched structure relaxation on the device: FIRE (Bitzek et al., Phys. Rev. Lett. 97, 170201, 2006) over the forces of a model.

    from pamnet_amd.relax import relax
    res = relax(model, data, fmax=0.05, max_steps=200, fixed=bottom_layer)

Every graph of the batch carries its own time step, mixing coefficient, downhill counter, convergence flag and displacement
cap (csrc/relax.hip pamnet_fire_step_f32, one launch per step; include/pamnet_hip.h states the rule), so a structure's
trajectory does not depend on its batch-mates, and it is bitwise repeatable.  The loop takes no decision on the host: the only
device -> host read of the driver is the status vector, every `check_every` steps.  There is no CPU path.
"""
import copy

import torch

from . import graph as G
from . import lib

FIRE_DEFAULTS = dict(dt0=0.1, dt_max=1.0, max_step=0.2, n_min=5, f_inc=1.1, f_dec=0.5, a0=0.1, f_a=0.99)
STATE = ('dt', 'a', 'n_pos', 'steps', 'status', 'fmax')
RUNNING, CONVERGED, FAILED = 0, 1, 2


class RelaxResult(object):
    """pos [N, 3] fp32 (a new tensor), energy [G] and forces [N, 3] of one evaluation at `pos`, converged / failed bool [G],
    steps int32 [G] (the steps a graph moved), fmax [G] (the largest force of the graph's last step: of `pos` for a converged
    graph), trace (trace=True: one dict per step, else None).  All on the device."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def new_state(n, n_graphs, device, dt0=FIRE_DEFAULTS['dt0'], a0=FIRE_DEFAULTS['a0']):
    """(vel [n, 3] fp32 zeros, state) for pamnet_fire_step_f32: state = dict of dt, a (fp64), n_pos, steps, status (int32), fmax
    (fp32), each [n_graphs]."""
    i32 = dict(dtype=torch.int32, device=device)
    state = dict(dt=torch.full((n_graphs,), float(dt0), dtype=torch.float64, device=device),
                 a=torch.full((n_graphs,), float(a0), dtype=torch.float64, device=device),
                 n_pos=torch.zeros(n_graphs, **i32), steps=torch.zeros(n_graphs, **i32), status=torch.zeros(n_graphs, **i32),
                 fmax=torch.zeros(n_graphs, dtype=torch.float32, device=device))
    return torch.zeros(n, 3, dtype=torch.float32, device=device), state


def _fire_params(given):
    """FIRE_DEFAULTS with the caller's values; a name the rule does not have is a TypeError."""
    unknown = sorted(set(given) - set(FIRE_DEFAULTS))
    if unknown:
        raise TypeError('unknown FIRE parameter(s) %s: the rule has %s' % (', '.join(unknown), ', '.join(sorted(FIRE_DEFAULTS))))
    p = dict(FIRE_DEFAULTS)
    p.update(given)
    return p


def fire_step(pos, vel, dpos, gptr, state, fmax_tol, fixed=None, **fire_params):
    """One FIRE step of every running graph, in place on pos, vel and state (one launch, no synchronisation).  pos, vel, dpos:
    fp32 [n, 3]; gptr: int32 [n_graphs + 1]; fixed: uint8 / bool [n] or None; fmax_tol: a float, or fp32 [n_graphs]."""
    stream = lib.stream_of(pos)
    p = _fire_params(fire_params)
    per_graph = isinstance(fmax_tol, torch.Tensor)
    lib.call('pamnet_fire_step_f32', lib.ptr(pos), lib.ptr(vel), lib.ptr(dpos), lib.ptr(fixed), lib.ptr(gptr), pos.size(0),
             gptr.numel() - 1, lib.ptr(state['dt']), lib.ptr(state['a']), lib.ptr(state['n_pos']), lib.ptr(state['steps']),
             lib.ptr(state['status']), lib.ptr(state['fmax']), lib.ptr(fmax_tol) if per_graph else None,
             0.0 if per_graph else float(fmax_tol), float(p['dt_max']), float(p['max_step']), int(p['n_min']),
             float(p['f_inc']), float(p['f_dec']), float(p['a0']), float(p['f_a']), stream)


def _checked(model, data, fmax, fixed):
    """The refusals, before anything runs: (pos, batch, n_graphs, fmax, fixed as uint8)."""
    pos, batch = getattr(data, 'pos', None), getattr(data, 'batch', None)
    dataset = getattr(model, 'dataset', None)
    if isinstance(dataset, str) and dataset != 'QM9':
        raise ValueError('relax moves `data.pos`: a PAMNet of dataset %r keeps its positions in x[:, :3] (the PDBbind / RNA schemas '
                         'are not relaxed); use a QM9-schema model' % (dataset,))
    if pos is None or batch is None:
        raise ValueError('relax needs `data.pos` (fp32 [N, 3]) and `data.batch` (the sorted graph id of every atom); the batch has '
                         'no `%s`' % ('pos' if pos is None else 'batch'))
    lib.stream_of(pos)                            # (a CPU tensor: RuntimeError, there is no CPU path)
    lib.stream_of(batch)
    if pos.dim() != 2 or pos.size(1) != 3 or batch.numel() != pos.size(0):
        raise ValueError('`data.pos` must be [N, 3] with one `data.batch` entry per row; got %s and %s'
                         % (tuple(pos.shape), tuple(batch.shape)))
    ng = getattr(data, 'num_graphs', None)
    n_graphs = int(ng) if ng is not None else (int(batch[-1]) + 1 if batch.numel() else 0)   # (as build_graph: one read at set-up)
    if isinstance(fmax, torch.Tensor):
        if fmax.dtype != torch.float32 or tuple(fmax.shape) != (n_graphs,) or fmax.device != pos.device:
            raise ValueError('a per-graph `fmax` is a float32 tensor [num_graphs] = [%d] on the device of `pos`; got %s %s on %s'
                             % (n_graphs, fmax.dtype, tuple(fmax.shape), fmax.device))
        fmax = fmax.contiguous()
    else:
        try:
            fmax = float(fmax)
        except (TypeError, ValueError):
            raise ValueError('`fmax` is a float, or a float32 tensor [num_graphs] on the device of `pos`; got %r' % (type(fmax),))
    if fixed is not None:
        if (not isinstance(fixed, torch.Tensor) or fixed.dtype != torch.bool or tuple(fixed.shape) != (pos.size(0),)
                or fixed.device != pos.device):
            raise ValueError('`fixed` is a torch.bool tensor [N] = [%d] on the device of `pos` (True: the atom does not move); got '
                             '%s' % (pos.size(0), '%s %s on %s' % (fixed.dtype, tuple(fixed.shape), fixed.device)
                                     if isinstance(fixed, torch.Tensor) else type(fixed)))
        fixed = fixed.to(torch.uint8).contiguous()
    return pos, batch, n_graphs, fmax, fixed


def _at(data, cur):
    """A shallow copy of the batch at the positions `cur`, as a leaf that requires grad.  Everything else the batch carries
    (edge_index, cell, pbc, cell_images, mol_local, ...) is shared, except what was made for the old positions: a graph
    prepared ahead, and the host-side `sizes` of a MoleculeStore batch."""
    d = copy.copy(data)
    d.pos = cur.detach().requires_grad_(True)
    if getattr(d, '_pamnet_prepared', None) is not None:
        d._pamnet_prepared = None
    if getattr(d, 'sizes', None) is not None:     # a store's host-side edge counts belong to the stored geometry: once an atom
        d.sizes = None                            # crosses a cutoff they are wrong, so the sizes are read from the device
    return d


def _evaluate(model, data, cur):
    d = _at(data, cur)
    e = model(d)
    de, = torch.autograd.grad(e.sum(), d.pos)
    return e.detach(), de.contiguous()


def relax(model, data, fmax=0.05, max_steps=200, fixed=None, check_every=10, trace=False, **fire_params):
    """Relax every graph of `data` until its largest force on a free atom is below `fmax`, or for `max_steps` steps.

    model:  any callable with model(data) -> [G] that is differentiable with respect to `data.pos`: PAMNet / PAMNet_s on the QM9
            schema (bonded, bond-free, periodic with `cell` / `pbc` / `cell_images` / `mol_local`), or a plain torch module.  The
            graph is rebuilt by every evaluation, so bonds defined by cutoff_l may form and break; `edge_index` stays as given.
    data:   the batch; `data.pos` is never written (the driver moves its own copy) and no parameter .grad is touched.  The
            host-side `sizes` of a MoleculeStore batch are not used: they count the edges of the stored geometry, so every
            evaluation reads its sizes from the device (one host round trip each, as for plain tensors).
    fmax:   the convergence threshold, a float or fp32 [G] on the device.
    fixed:  bool [N] on the device (True: the atom does not move), or None.
    check_every: the status vector is read every so many steps, to stop when no graph is running; 0: never -- `max_steps`
            steps are enqueued and device tensors returned without a synchronisation of the driver's own.
    trace:  for tests and debugging: keep, per step, clones of pos before and after the step, dE/dpos, vel before and after and
            the state (dt, a, n_pos, steps, status, fmax) before and after, in res.trace.
    fire_params: dt0, dt_max, max_step, n_min, f_inc, f_dec, a0, f_a (FIRE_DEFAULTS).

    Converged and failed graphs stop moving but are still evaluated.  The cell is not relaxed (`strain` is not attached here)."""
    p = _fire_params(fire_params)
    pos, batch, n_graphs, tol, fixed8 = _checked(model, data, fmax, fixed)
    kernel_params = {k: v for k, v in p.items() if k != 'dt0'}
    cur = pos.detach().to(torch.float32).clone().contiguous()
    gptr, _ = G.csr_from_keys(batch.to(torch.int32).contiguous(), n_graphs)
    vel, state = new_state(cur.size(0), n_graphs, cur.device, p['dt0'], p['a0'])
    steps_log = [] if trace else None
    for it in range(int(max_steps)):
        _, de = _evaluate(model, data, cur)
        if trace:
            rec = dict(pos=cur.clone(), dE=de.clone(), v_before=vel.clone(), state_before={k: state[k].clone() for k in STATE})
        fire_step(cur, vel, de, gptr, state, tol, fixed8, **kernel_params)
        if trace:
            rec.update(pos_after=cur.clone(), v_after=vel.clone(), state_after={k: state[k].clone() for k in STATE})
            steps_log.append(rec)
        if check_every and (it + 1) % int(check_every) == 0 and not bool((state['status'] == RUNNING).any()):
            break
    energy, de = _evaluate(model, data, cur)      # one more evaluation: energy and forces belong to the returned geometry
    return RelaxResult(pos=cur, energy=energy, forces=-de, converged=state['status'] == CONVERGED,
                       failed=state['status'] == FAILED, steps=state['steps'], fmax=state['fmax'], trace=steps_log)
