"""Batched structure relaxation on the device: FIRE (Bitzek et al., Phys. Rev. Lett. 97, 170201, 2006) over the forces of a model.

    from pamnet_amd.relax import relax
    res = relax(model, data, fmax=0.05, max_steps=200, fixed=bottom_layer)

Every graph of the batch carries its own time step, mixing coefficient, downhill counter, convergence flag and displacement
cap (csrc/relax.hip pamnet_fire_step_f32, one launch per step; include/pamnet_hip.h states the rule), so a structure's
trajectory does not depend on its batch-mates, and it is bitwise repeatable.  The loop takes no decision on the host: the only
device -> host read of the driver is the status vector, every `check_every` steps.  There is no CPU path.

    from pamnet_amd.relax import relax_lbfgs
    res = relax_lbfgs(model, data, fmax=0.05, max_steps=200, fixed=bottom_layer, memory=10)

is the same loop with limited-memory BFGS steps (csrc/lbfgs.hip pamnet_lbfgs_step_f32): fewer evaluations per relaxation, every
piece of optimiser state -- history, curvature test, scaling, descent check, cap -- per graph, under the same guarantees.

    from pamnet_amd.relax import relax_cell
    res = relax_cell(model, data, fmax=0.05, smax=0.005, pressure=0.0)

relaxes the cell with the atoms (csrc/relax_cell.hip pamnet_fire_cell_step_f32): FIRE over the forces and the virial in the
unit-cell-filter formulation, under the same guarantees.
"""
import copy

import torch

from . import graph as G
from . import lib

FIRE_DEFAULTS = dict(dt0=0.1, dt_max=1.0, max_step=0.2, n_min=5, f_inc=1.1, f_dec=0.5, a0=0.1, f_a=0.99)
STATE = ('dt', 'a', 'n_pos', 'steps', 'status', 'fmax')
CELL_STATE = STATE + ('smax',)                    # per-graph scalars of the variable-cell step (F and vcell travel beside them)
RUNNING, CONVERGED, FAILED = 0, 1, 2


class RelaxResult(object):
    """pos [N, 3] fp32 (a new tensor), energy [G] and forces [N, 3] of one evaluation at `pos`, converged / failed bool [G],
    steps int32 [G] (the steps a graph moved), fmax [G] (the largest force of the graph's last step: of `pos` for a converged
    graph), trace (trace=True: one dict per step, else None).  All on the device.
    relax_cell adds: cell [G, 3, 3] fp32 (a new tensor), F [G, 3, 3] fp64 (cell = cell0 F), virial [G, 3, 3] fp32 (W = dE/d strain)
    and stress = W / volume of the same evaluation at `pos` and `cell`, volume [G] fp64 (|det cell|; a graph whose cell is
    singular, such as an open molecule's zero cell, has volume 0 and a non-finite stress), smax [G] fp32 (the largest
    |S_ij| / volume of the graph's last step).
    relax_lbfgs adds: skipped, resets int32 [G] (the pairs a graph refused for their curvature; the times it fell back to
    steepest descent)."""

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

    Converged and failed graphs stop moving but are still evaluated.  The cell is not relaxed (`strain` is not attached here):
    relax_cell does that."""
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


# ------------------------------------------------------------------------------------------------------------- L-BFGS
LBFGS_DEFAULTS = dict(memory=10, alpha=70.0, max_step=0.2, skip_tol=1e-8)
MAX_MEMORY = 32
LBFGS_SCALARS = ('rho', 'gamma', 'head', 'count', 'has_prev', 'skipped', 'resets', 'steps', 'status', 'fmax')   # per graph
LBFGS_ARRAYS = ('prev_pos', 'prev_dpos', 'hist_s', 'hist_y', 'work')                                            # per atom
LBFGS_STATE = LBFGS_ARRAYS + LBFGS_SCALARS


def _lbfgs_params(given):
    """LBFGS_DEFAULTS with the caller's values; a name the rule does not have is a TypeError, a memory outside 1 .. 32 a
    ValueError."""
    unknown = sorted(set(given) - set(LBFGS_DEFAULTS))
    if unknown:
        raise TypeError('unknown L-BFGS parameter(s) %s: the rule has %s' % (', '.join(unknown), ', '.join(sorted(LBFGS_DEFAULTS))))
    p = dict(LBFGS_DEFAULTS)
    p.update(given)
    m = p['memory']
    if isinstance(m, bool) or int(m) != m or not 1 <= int(m) <= MAX_MEMORY:
        raise ValueError('`memory` (the pairs every graph keeps) is an integer from 1 to %d; got %r' % (MAX_MEMORY, m))
    p['memory'] = int(m)
    return p


def new_lbfgs_state(n, n_graphs, device, memory=LBFGS_DEFAULTS['memory']):
    """The state of pamnet_lbfgs_step_f32, all zeros: prev_pos, prev_dpos (fp32 [n, 3]), hist_s, hist_y (fp64 [memory, n, 3]),
    work (fp64 [n, 3]), rho (fp64 [n_graphs, memory]), gamma (fp64 [n_graphs]), head, count, has_prev, skipped, resets, steps,
    status (int32 [n_graphs]) and fmax (fp32 [n_graphs]).  The memory is part of the state: its arrays are shaped by it."""
    memory = _lbfgs_params(dict(memory=memory))['memory']
    f32, f64, i32 = (dict(dtype=t, device=device) for t in (torch.float32, torch.float64, torch.int32))
    state = dict(prev_pos=torch.zeros(n, 3, **f32), prev_dpos=torch.zeros(n, 3, **f32), hist_s=torch.zeros(memory, n, 3, **f64),
                 hist_y=torch.zeros(memory, n, 3, **f64), work=torch.zeros(n, 3, **f64), rho=torch.zeros(n_graphs, memory, **f64),
                 gamma=torch.zeros(n_graphs, **f64), fmax=torch.zeros(n_graphs, **f32))
    for k in ('head', 'count', 'has_prev', 'skipped', 'resets', 'steps', 'status'):
        state[k] = torch.zeros(n_graphs, **i32)
    return state


def lbfgs_step(pos, dpos, gptr, state, fmax_tol, fixed=None, **lbfgs_params):
    """One L-BFGS step of every running graph, in place on pos and state (one launch, no synchronisation).  pos, dpos: fp32
    [n, 3]; gptr: int32 [n_graphs + 1]; state: new_lbfgs_state's, whose history fixes the memory (a `memory` given here must be
    that one); fixed: uint8 / bool [n] or None; fmax_tol: a float, or fp32 [n_graphs]."""
    stream = lib.stream_of(pos)
    memory = int(state['hist_s'].size(0))
    if 'memory' in lbfgs_params and lbfgs_params['memory'] != memory:
        raise ValueError('the state was made for memory = %d; got memory = %r' % (memory, lbfgs_params['memory']))
    p = _lbfgs_params(dict(lbfgs_params, memory=memory))
    n, n_graphs = pos.size(0), gptr.numel() - 1
    if (tuple(state['hist_s'].shape) != (memory, n, 3) or tuple(state['hist_y'].shape) != (memory, n, 3)
            or tuple(state['rho'].shape) != (n_graphs, memory)):
        raise ValueError('the state does not belong to this batch: hist_s %s, hist_y %s, rho %s for n = %d, n_graphs = %d, '
                         'memory = %d' % (tuple(state['hist_s'].shape), tuple(state['hist_y'].shape), tuple(state['rho'].shape), n,
                                          n_graphs, memory))
    tol_g, tol = _split(fmax_tol)
    lib.call('pamnet_lbfgs_step_f32', lib.ptr(pos), lib.ptr(dpos), lib.ptr(fixed), lib.ptr(gptr), n, n_graphs,
             lib.ptr(state['prev_pos']), lib.ptr(state['prev_dpos']), lib.ptr(state['hist_s']), lib.ptr(state['hist_y']),
             lib.ptr(state['work']), lib.ptr(state['rho']), lib.ptr(state['gamma']), lib.ptr(state['head']),
             lib.ptr(state['count']), lib.ptr(state['has_prev']), lib.ptr(state['skipped']), lib.ptr(state['resets']),
             lib.ptr(state['steps']), lib.ptr(state['status']), lib.ptr(state['fmax']), tol_g, tol, memory, float(p['alpha']),
             float(p['max_step']), float(p['skip_tol']), stream)


def relax_lbfgs(model, data, fmax=0.05, max_steps=200, fixed=None, check_every=10, trace=False, **lbfgs_params):
    """relax() with limited-memory BFGS steps in place of FIRE's (csrc/lbfgs.hip pamnet_lbfgs_step_f32, one launch per step;
    include/pamnet_hip.h states the rule): the two-loop recursion over the last `memory` pairs (s, y) of every graph, the initial
    matrix scaled by y.s / y.y, a pair kept only where its curvature is positive, steepest descent scaled by 1 / alpha on the
    first step and wherever the direction is not a descent direction, and a cap on the largest displacement of an atom -- no
    line search.  Every piece of that state is per graph, so a structure's trajectory does not depend on its batch-mates and
    is bitwise repeatable; the price of a relaxation is its number of evaluations, which this lowers.

    model, data, fmax, max_steps, fixed, check_every: as for relax().
    trace:  keep, per step, clones of pos before and after the step, dE/dpos and the whole state (LBFGS_STATE, the history
            included) before and after, in res.trace.
    lbfgs_params: memory (1 .. 32), alpha, max_step, skip_tol (LBFGS_DEFAULTS).  alpha = 70 is ASE's value, a convention for eV
            and Angstrom as fmax = 0.05 is: the first step moves an atom by its force / alpha.

    Returns a RelaxResult with the fields of relax() and skipped / resets, int32 [G]: the pairs a graph refused for their
    curvature and the times it fell back to steepest descent.  Converged and failed graphs stop moving but are still evaluated;
    the only device -> host read is the status vector, every `check_every` steps (0: never).  One more evaluation at the end."""
    p = _lbfgs_params(lbfgs_params)
    pos, batch, n_graphs, tol, fixed8 = _checked(model, data, fmax, fixed)
    kernel_params = {k: v for k, v in p.items() if k != 'memory'}
    cur = pos.detach().to(torch.float32).clone().contiguous()
    gptr, _ = G.csr_from_keys(batch.to(torch.int32).contiguous(), n_graphs)
    state = new_lbfgs_state(cur.size(0), n_graphs, cur.device, p['memory'])
    snap = lambda: {k: state[k].clone() for k in LBFGS_STATE}
    steps_log = [] if trace else None
    for it in range(int(max_steps)):
        _, de = _evaluate(model, data, cur)
        if trace:
            rec = dict(pos=cur.clone(), dE=de.clone(), state_before=snap())
        lbfgs_step(cur, de, gptr, state, tol, fixed8, **kernel_params)
        if trace:
            rec.update(pos_after=cur.clone(), state_after=snap())
            steps_log.append(rec)
        if check_every and (it + 1) % int(check_every) == 0 and not bool((state['status'] == RUNNING).any()):
            break
    energy, de = _evaluate(model, data, cur)      # one more evaluation: energy and forces belong to the returned geometry
    return RelaxResult(pos=cur, energy=energy, forces=-de, converged=state['status'] == CONVERGED,
                       failed=state['status'] == FAILED, steps=state['steps'], fmax=state['fmax'], skipped=state['skipped'],
                       resets=state['resets'], trace=steps_log)


# ----------------------------------------------------------------------------------------------------- cell relaxation
def new_cell_state(n, n_graphs, device, dt0=FIRE_DEFAULTS['dt0'], a0=FIRE_DEFAULTS['a0']):
    """(vel [n, 3] fp32 zeros, state) for pamnet_fire_cell_step_f32: the state of new_state plus smax (fp32 [n_graphs]), F (fp64
    [n_graphs, 3, 3], the identity: the cell is cell0 F) and vcell (fp64 [n_graphs, 3, 3] zeros)."""
    vel, state = new_state(n, n_graphs, device, dt0, a0)
    state['smax'] = torch.zeros(n_graphs, dtype=torch.float32, device=device)
    state['F'] = torch.eye(3, dtype=torch.float64, device=device).repeat(n_graphs, 1, 1).contiguous()
    state['vcell'] = torch.zeros(n_graphs, 3, 3, dtype=torch.float64, device=device)
    return vel, state


def _split(v):
    """A per-graph tensor or a scalar -> (pointer or None, the scalar the entry point takes beside it)."""
    return (lib.ptr(v), 0.0) if isinstance(v, torch.Tensor) else (None, float(v))


def fire_cell_step(pos, vel, dpos, dstrain, gptr, cell0, cell, state, fmax_tol, smax_tol, cell_factor, fixed=None, cell_dof=None,
                   pressure=0.0, hydrostatic=False, **fire_params):
    """One variable-cell FIRE step of every running graph, in place on pos, vel, cell and state (one launch, no
    synchronisation).  pos, vel, dpos: fp32 [n, 3]; dstrain (the virial), cell0 (read only), cell: fp32 [n_graphs, 3, 3]; gptr:
    int32 [n_graphs + 1]; state: new_cell_state's; fmax_tol, smax_tol: a float, or fp32 [n_graphs]; pressure: a float, or fp64
    [n_graphs]; cell_factor: fp64 [n_graphs]; fixed: uint8 / bool [n] or None; cell_dof: uint8 / bool [n_graphs] or None (every
    graph relaxes its cell; a graph with 0 takes the step of fire_step)."""
    p = _fire_params(fire_params)
    (ftol_g, ftol), (stol_g, stol), (p_g, p_s) = _split(fmax_tol), _split(smax_tol), _split(pressure)
    lib.call('pamnet_fire_cell_step_f32', lib.ptr(pos), lib.ptr(vel), lib.ptr(dpos), lib.ptr(dstrain), lib.ptr(fixed),
             lib.ptr(gptr), pos.size(0), gptr.numel() - 1, lib.ptr(cell0), lib.ptr(cell), lib.ptr(state['F']),
             lib.ptr(state['vcell']), lib.ptr(cell_dof), lib.ptr(cell_factor), lib.ptr(state['dt']), lib.ptr(state['a']),
             lib.ptr(state['n_pos']), lib.ptr(state['steps']), lib.ptr(state['status']), lib.ptr(state['fmax']),
             lib.ptr(state['smax']), ftol_g, stol_g, p_g, ftol, stol, p_s, int(bool(hydrostatic)), float(p['dt_max']),
             float(p['max_step']), int(p['n_min']), float(p['f_inc']), float(p['f_dec']), float(p['a0']), float(p['f_a']),
             lib.stream_of(pos))


def _per_graph(name, v, n_graphs, device, dtype, what):
    """A float, or a tensor [num_graphs] of `dtype` on the device of pos (contiguous), in the style of _checked."""
    if isinstance(v, torch.Tensor):
        if v.dtype != dtype or tuple(v.shape) != (n_graphs,) or v.device != device:
            raise ValueError('a per-graph `%s` is a %s tensor [num_graphs] = [%d] on the device of `pos`; got %s %s on %s'
                             % (name, str(dtype).replace('torch.', ''), n_graphs, v.dtype, tuple(v.shape), v.device))
        return v.detach().contiguous()
    try:
        return float(v)
    except (TypeError, ValueError):
        raise ValueError('`%s` (%s) is a float, or a %s tensor [num_graphs] on the device of `pos`; got %r'
                         % (name, what, str(dtype).replace('torch.', ''), type(v)))


def _det3(m):
    """det of [G, 3, 3], written out (elementwise launches: no factorisation, no synchronisation)."""
    return (m[:, 0, 0] * (m[:, 1, 1] * m[:, 2, 2] - m[:, 1, 2] * m[:, 2, 1])
            - m[:, 0, 1] * (m[:, 1, 0] * m[:, 2, 2] - m[:, 1, 2] * m[:, 2, 0])
            + m[:, 0, 2] * (m[:, 1, 0] * m[:, 2, 1] - m[:, 1, 1] * m[:, 2, 0]))


def _evaluate_cell(model, data, cur, cell):
    """(E, dE/dpos, W = dE/dstrain) at the positions `cur` in the cell `cell`."""
    d = _at(data, cur)
    d.cell = cell
    d.strain = torch.zeros(cell.size(0), 3, 3, dtype=torch.float32, device=cell.device, requires_grad=True)
    e = model(d)
    de, w = torch.autograd.grad(e.sum(), [d.pos, d.strain])
    return e.detach(), de.contiguous(), w.contiguous()


def _cell_dof(data, cell_dof, n_graphs, device, checks, verb):
    """The per-graph cell switch of relax_cell and md.run_npt as uint8 [num_graphs], or None where every graph moves its cell.
    cell_dof None: a graph moves its cell where all three axes of `data.pbc` are periodic.  A given mask is checked against
    `data.pbc` on the device: its validity goes into checks['cell_dof'] for the caller's one read at set-up (False: True on a
    graph with an open axis, which the caller refuses).  verb: what the graph does with its cell, for the message."""
    pbc = getattr(data, 'pbc', None)
    if isinstance(pbc, torch.Tensor):
        if pbc.dtype != torch.bool or tuple(pbc.shape) != (n_graphs, 3) or pbc.device != device:
            raise ValueError('`data.pbc` is a torch.bool tensor [num_graphs, 3] = [%d, 3] on the device of `pos`, or a tuple of '
                             'three bools; got %s %s on %s' % (n_graphs, pbc.dtype, tuple(pbc.shape), pbc.device))
        periodic = pbc.all(1)
    elif pbc is None:
        periodic = None
    else:
        try:
            periodic = all(bool(v) for v in pbc) and len(pbc) == 3
        except TypeError:
            raise ValueError('`data.pbc` is a torch.bool tensor [num_graphs, 3] or a tuple of three bools; got %r' % (pbc,))
    if cell_dof is None:
        dof8 = None if periodic is None or periodic is True else (
            periodic.to(torch.uint8) if isinstance(periodic, torch.Tensor) else torch.zeros(n_graphs, dtype=torch.uint8, device=device))
    else:
        if (not isinstance(cell_dof, torch.Tensor) or cell_dof.dtype != torch.bool or tuple(cell_dof.shape) != (n_graphs,)
                or cell_dof.device != device):
            raise ValueError('`cell_dof` is a torch.bool tensor [num_graphs] = [%d] on the device of `pos` (True: the graph %s '
                             'its cell); got %s' % (n_graphs, verb, '%s %s on %s' % (cell_dof.dtype, tuple(cell_dof.shape), cell_dof.device)
                                                    if isinstance(cell_dof, torch.Tensor) else type(cell_dof)))
        if isinstance(periodic, torch.Tensor):
            checks['cell_dof'] = ~(cell_dof & ~periodic).any()
        elif periodic is False:
            checks['cell_dof'] = ~cell_dof.any()
        dof8 = cell_dof.to(torch.uint8).contiguous()
    return dof8


def relax_cell(model, data, fmax=0.05, smax=0.005, pressure=0.0, hydrostatic=False, cell_dof=None, cell_factor=None, fixed=None,
               max_steps=200, check_every=10, trace=False, **fire_params):
    """Relax the atoms and the cell of every graph of a periodic batch until its largest force on a free atom is below `fmax` and
    its largest stress component below `smax`, or for `max_steps` steps: FIRE over the forces and the virial in the
    unit-cell-filter formulation (Tadmor et al. 1999; include/pamnet_hip.h states the rule), one launch per step.

    model:  as for relax(), and differentiable with respect to `data.strain` as well: PAMNet / PAMNet_s on periodic batches
            (`cell`, with `pbc` / `cell_images` / `mol_local`, MoleculeStore batches), or a plain torch module that applies
            `(I + data.strain[g])` to the positions and the cell of graph g itself.  Every evaluation gets the driver's positions
            as the leaf `pos`, the driver's current cell as `cell` and fp32 zeros [G, 3, 3] that require grad as `strain`, and is
            differentiated by torch.autograd.grad(E.sum(), [pos, strain]).  The graph build's own conditions on the cell heights
            apply to every evaluation; the driver adds none.
    data:   the batch, with `data.cell` fp32 [G, 3, 3] (row k = lattice vector a_k); neither `data.pos` nor `data.cell` is written.
    fmax:   the force threshold, a float or fp32 [G] on the device.
    smax:   the stress threshold on max |S_ij| / V, S = (W + W^T) / 2 + p V I, a float or fp32 [G] on the device, in the caller's
            energy / length^3.  The default 0.005 is a convention for eV and Angstrom (about 0.8 GPa), as fmax = 0.05 eV / A is.
    pressure: p, a float or fp64 [G] on the device, in the same unit: what is minimised is E + p V.
    hydrostatic: only the volume changes, S <- (tr S / 3) I (for the whole batch).
    cell_dof: bool [G] on the device: False = the graph keeps its cell and takes exactly the step of relax().  None: a graph
            relaxes its cell where all three axes of `data.pbc` are periodic (everywhere where the batch has no `pbc`); a graph
            with an open axis relaxes at fixed cell.  True on a graph with an open axis is refused.
    cell_factor: L, a float or fp64 [G] on the device, positive: the cell enters the optimiser as L F, so one step changes the
            strain by at most max_step / L.  None: the atoms of each graph (1 for an empty graph).
    fixed:  bool [N] on the device, or None.  A fixed atom of a graph that relaxes its cell keeps its fractional coordinates: it
            follows the cell (ASE's behaviour under a cell filter).
    check_every, trace, fire_params: as for relax(); a trace record also holds cell, W, F, vcell and cell_after, F_after,
            vcell_after, and its states include smax.

    Per-graph values (cell_factor, pressure, a given cell_dof against `pbc`) are checked in one read at set-up; the loop reads
    nothing but the status vector, every `check_every` steps (0: never).  One more evaluation at the end: res.energy, res.forces,
    res.virial and res.stress belong to res.pos and res.cell."""
    p = _fire_params(fire_params)
    pos, batch, n_graphs, tol, fixed8 = _checked(model, data, fmax, fixed)
    device = pos.device
    cell_in = getattr(data, 'cell', None)
    if cell_in is None:
        raise ValueError('relax_cell needs `data.cell` (fp32 [num_graphs, 3, 3], row k = lattice vector a_k): the batch has no '
                         '`cell`; relax() relaxes the atoms of structures in open space')
    if (not isinstance(cell_in, torch.Tensor) or cell_in.dtype != torch.float32 or tuple(cell_in.shape) != (n_graphs, 3, 3)
            or cell_in.device != device):
        raise ValueError('`data.cell` is a float32 tensor [num_graphs, 3, 3] = [%d, 3, 3] on the device of `pos`; got %s'
                         % (n_graphs, '%s %s on %s' % (cell_in.dtype, tuple(cell_in.shape), cell_in.device)
                            if isinstance(cell_in, torch.Tensor) else type(cell_in)))
    stol = _per_graph('smax', smax, n_graphs, device, torch.float32, 'the stress threshold')
    prs = _per_graph('pressure', pressure, n_graphs, device, torch.float64, 'p of E + p V')
    checks = {}
    if isinstance(prs, torch.Tensor):
        checks['pressure'] = torch.isfinite(prs).all()
    elif prs != prs or prs in (float('inf'), float('-inf')):
        raise ValueError('`pressure` must be finite; got %r' % (prs,))
    if isinstance(stol, float) and stol != stol:
        raise ValueError('`smax` must not be NaN')
    gptr, _ = G.csr_from_keys(batch.to(torch.int32).contiguous(), n_graphs)
    if cell_factor is None:
        factor = (gptr[1:] - gptr[:-1]).clamp(min=1).to(torch.float64)
    else:
        factor = _per_graph('cell_factor', cell_factor, n_graphs, device, torch.float64, 'L of the cell coordinate L F')
        if isinstance(factor, torch.Tensor):
            checks['cell_factor'] = (torch.isfinite(factor) & (factor > 0)).all()
        elif not (factor > 0.0 and factor != float('inf')):
            raise ValueError('`cell_factor` must be positive and finite; got %r' % (factor,))
        else:
            factor = torch.full((n_graphs,), factor, dtype=torch.float64, device=device)
    factor = factor.contiguous()
    dof8 = _cell_dof(data, cell_dof, n_graphs, device, checks, 'relaxes')
    names = list(checks)
    if names:                                     # (as md.run: one read at set-up, for every tensor of values at once)
        ok = torch.stack([checks[k] for k in names]).tolist()
        bad = [k for k, good in zip(names, ok) if not good]
        if 'cell_dof' in bad:
            raise ValueError('`cell_dof` is True on a graph with an open axis (`data.pbc`): a cell with an open axis is not relaxed '
                             '(the vector of an open axis carries no energy); leave that graph False, or relax the structure as '
                             'fully periodic')
        if bad:
            raise ValueError('%s must be finite (cell_factor: and positive) in every entry' % ' and '.join('`%s`' % k for k in bad))
    kernel_params = {k: v for k, v in p.items() if k != 'dt0'}
    cur = pos.detach().to(torch.float32).clone().contiguous()
    cell0 = cell_in.detach().clone().contiguous()
    cell = cell0.clone()
    vel, state = new_cell_state(cur.size(0), n_graphs, device, p['dt0'], p['a0'])
    snap = lambda: {k: state[k].clone() for k in CELL_STATE}
    steps_log = [] if trace else None
    for it in range(int(max_steps)):
        _, de, w = _evaluate_cell(model, data, cur, cell)
        if trace:
            rec = dict(pos=cur.clone(), dE=de.clone(), W=w.clone(), cell=cell.clone(), F=state['F'].clone(),
                       vcell=state['vcell'].clone(), v_before=vel.clone(), state_before=snap())
        fire_cell_step(cur, vel, de, w, gptr, cell0, cell, state, tol, stol, factor, fixed8, dof8, prs, hydrostatic,
                       **kernel_params)
        if trace:
            rec.update(pos_after=cur.clone(), v_after=vel.clone(), cell_after=cell.clone(), F_after=state['F'].clone(),
                       vcell_after=state['vcell'].clone(), state_after=snap())
            steps_log.append(rec)
        if check_every and (it + 1) % int(check_every) == 0 and not bool((state['status'] == RUNNING).any()):
            break
    energy, de, w = _evaluate_cell(model, data, cur, cell)     # one more evaluation: everything belongs to the returned geometry
    volume = _det3(cell.to(torch.float64)).abs()
    return RelaxResult(pos=cur, cell=cell, F=state['F'], energy=energy, forces=-de, virial=w,
                       stress=(w.to(torch.float64) / volume[:, None, None]).to(torch.float32), volume=volume,
                       converged=state['status'] == CONVERGED, failed=state['status'] == FAILED, steps=state['steps'],
                       fmax=state['fmax'], smax=state['smax'], trace=steps_log)
