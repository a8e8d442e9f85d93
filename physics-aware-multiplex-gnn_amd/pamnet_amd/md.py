"""Batched molecular dynamics on the device: NVE (velocity Verlet) and Langevin (BAOAB, Leimkuhler & Matthews, J. Chem. Phys. 138,
174102, 2013) over the forces of a model.

    from pamnet_amd.md import run
    res = run(model, data, steps=1000, dt=0.1, masses=m, kT=0.025, gamma=0.1, seed=seeds, record_every=10)

Every graph of the batch carries its own step counter, status and seed (csrc/md.hip pamnet_md_step_f32, one launch per step;
include/pamnet_hip.h states the rule and the generator).  The noise is counter-based -- Philox4x32-10 keyed by the graph's seed,
counted by the atom's offset in its graph and the graph's step -- so a structure's trajectory does not depend on its batch-mates
and is bitwise repeatable.  The loop takes no decision on the host.  There is no CPU path.

    from pamnet_amd.md import run_npt
    res = run_npt(model, data, steps=1000, dt=0.1, kT=0.025, pressure=6.2415e-7, tau_p=50.0, compressibility=8.0, gamma=0.1)

is the same dynamics at constant pressure (isotropic NPT): the stochastic cell rescaling barostat (Bernetti & Bussi, J. Chem.
Phys. 153, 114107, 2020) fused into the step launch (csrc/md_npt.hip pamnet_md_npt_step_f32), under the same guarantees.

    from pamnet_amd import md
    cons = md.Constraints(data, md.bond_constraints(data.edge_index, data.x == 0))      # every X-H bond at its current length
    res = md.run(model, data, steps=1000, dt=0.2, masses=m, kT=0.025, gamma=0.1, seed=seeds, constraints=cons)

holds bond lengths fixed (g-BAOAB: SHAKE / RATTLE sweeps over constraints coloured once on the host, inside the step launch:
csrc/md_constraints.hip pamnet_md_constrained_step_f32), which lets dt be doubled where X-H vibrations capped it.

    from pamnet_amd import bias
    b = bias.Bias(data, [bias.dihedral(4, 6, 8, 14)], metadynamics=dict(ndim=1, sigma=0.35, height=0.012, bias_factor=8, kT=0.025, pace=50))
    res = md.run(model, data, steps=20000, dt=0.1, masses=m, kT=0.025, gamma=0.1, seed=seeds, bias=b)

biases the run along collective variables (restraints and well-tempered metadynamics: one more launch per step before the
step launch, csrc/bias.hip pamnet_bias_apply_f64; pamnet_amd/bias.py).

Units are the caller's: with energies in eV, lengths in Angstrom and masses in amu the time unit is 10.1805 fs (dt = 0.1 is about
1 fs), kT is in eV and a pressure in eV / A^3 (160.2177 GPa; 1 bar = 6.2415e-7)."""
import torch

from . import graph as G
from . import lib
from .relax import _cell_dof, _checked, _det3, _evaluate, _evaluate_cell

STATE = ('seed', 'steps', 'status', 'ke')
NPT_STATE = STATE + ('eps', 'pint', 'vol')         # per-graph scalars of the constant-pressure step (cell travels beside them)
CONSTRAINED_STATE = STATE + ('sweeps',)            # of the constrained step: the most sweeps a solve of the launch took
RUNNING, FAILED = 0, 2
UNCONVERGED = 3                                   # (a constraint solve of the graph did not converge)


class MDResult(object):
    """pos, vel [N, 3] fp32 (new tensors), energy [G] and forces [N, 3] of one evaluation at `pos`, kinetic [G] fp64 (of `vel`),
    steps int32 [G] (the steps a graph moved), failed bool [G], frames [F, N, 3] fp32 / epot, ekin [F, G] fp64 (record_every > 0,
    else None), trace (trace=True: one dict per launch, else None).  All on the device.
    run with constraints adds: unconverged bool [G] (a constraint solve of the graph failed: status 3), sweeps int32 [G].
    run with bias adds: cv [F, K] and ebias [F, G] fp64 (record_every > 0, else None); forces include the bias, energy does not.
    run_npt adds: cell [G, 3, 3] fp32 (a new tensor), eps [G] fp64 (ln of the volume over the starting volume), volume and pressure
    [G] fp64 (the kernel's V and P_int = (2 KE - tr W) / (3 V) of `pos`, `vel` and `cell`; a graph without a barostat keeps
    |det cell| and NaN), virial [G, 3, 3] fp32 (W = dE/d strain) and stress = W / volume of the same evaluation; with record_every
    cells [F, G, 3, 3] fp32 and volumes, pressures [F, G] fp64."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def new_state(n, n_graphs, device, seed=0):
    """(vel [n, 3] fp32 zeros, state) for pamnet_md_step_f32: state = dict of seed (int64), steps, status (int32), ke (fp64), each
    [n_graphs].  seed: an int -- graph g gets seed + g -- or an int64 tensor [n_graphs] on the device."""
    if isinstance(seed, torch.Tensor):
        if seed.dtype != torch.int64 or tuple(seed.shape) != (n_graphs,) or seed.device != torch.device(device):
            raise ValueError('a per-graph `seed` is an int64 tensor [num_graphs] = [%d] on the device of `pos`; got %s %s on %s'
                             % (n_graphs, seed.dtype, tuple(seed.shape), seed.device))
        seed = seed.contiguous()
    else:
        try:
            seed = int(seed) + torch.arange(n_graphs, dtype=torch.int64, device=device)
        except (TypeError, ValueError):
            raise ValueError('`seed` is an int, or an int64 tensor [num_graphs] on the device of `pos`; got %r' % (type(seed),))
    state = dict(seed=seed, steps=torch.zeros(n_graphs, dtype=torch.int32, device=device),
                 status=torch.zeros(n_graphs, dtype=torch.int32, device=device),
                 ke=torch.zeros(n_graphs, dtype=torch.float64, device=device))
    return torch.zeros(n, 3, dtype=torch.float32, device=device), state


def _split(v):
    """A per-graph tensor or a scalar -> (pointer or None, the scalar the entry point takes beside it)."""
    return (lib.ptr(v), 0.0) if isinstance(v, torch.Tensor) else (None, float(v))


def md_step(pos, vel, dpos, gptr, state, dt, kT=0.0, gamma=0.0, mass=None, fixed=None, kick_in=1, advance=1):
    """One launch of pamnet_md_step_f32, in place on pos, vel and state (no synchronisation).  pos, vel, dpos: fp32 [n, 3]; gptr:
    int32 [n_graphs + 1]; mass: fp32 [n] or None; fixed: uint8 / bool [n] or None; dt, kT, gamma: a float, or fp64 [n_graphs];
    state['seed'] may be None where gamma is the float 0."""
    (dt_g, dt), (kT_g, kT), (gamma_g, gamma) = _split(dt), _split(kT), _split(gamma)
    lib.call('pamnet_md_step_f32', lib.ptr(pos), lib.ptr(vel), lib.ptr(dpos), lib.ptr(mass), lib.ptr(fixed), lib.ptr(gptr),
             pos.size(0), gptr.numel() - 1, lib.ptr(state['seed']), lib.ptr(state['steps']), lib.ptr(state['status']),
             lib.ptr(state['ke']), dt_g, kT_g, gamma_g, dt, kT, gamma, int(kick_in), int(advance), lib.stream_of(pos))


def init_velocities(vel, gptr, seed, kT, ke, mass=None, fixed=None, remove_com=True, rescale=False):
    """One launch of pamnet_md_init_velocities_f32: Maxwell-Boltzmann velocities at kT (a float, or fp64 [n_graphs]) into the rows
    of the free atoms of vel (fp32 [n, 3]), the kinetic energies into ke (fp64 [n_graphs]).  seed: int64 [n_graphs]."""
    kT_g, kT = _split(kT)
    lib.call('pamnet_md_init_velocities_f32', lib.ptr(vel), lib.ptr(mass), lib.ptr(fixed), lib.ptr(gptr), vel.size(0),
             gptr.numel() - 1, lib.ptr(seed), kT_g, kT, int(bool(remove_com)), int(bool(rescale)), lib.ptr(ke), lib.stream_of(vel))


def new_npt_state(n, n_graphs, device, cell0, seed=0):
    """(vel, state) of new_state plus eps (fp64 zeros), pint (fp64 NaN) and vol (fp64 |det cell0|), each [n_graphs]: the state of
    pamnet_md_npt_step_f32.  cell0: fp32 [n_graphs, 3, 3]."""
    vel, state = new_state(n, n_graphs, device, seed)
    state['eps'] = torch.zeros(n_graphs, dtype=torch.float64, device=device)
    state['pint'] = torch.full((n_graphs,), float('nan'), dtype=torch.float64, device=device)
    state['vol'] = _det3(cell0.to(torch.float64)).abs().contiguous()
    return vel, state


def npt_step(pos, vel, dpos, dstrain, gptr, cell0, cell, state, dt, kT, pressure, rate, gamma=0.0, mass=None, fixed=None,
             cell_dof=None, kick_in=1, advance=1):
    """One launch of pamnet_md_npt_step_f32, in place on pos, vel, cell and state (no synchronisation).  Beyond md_step: dstrain
    (the virial), cell0 (read only), cell: fp32 [n_graphs, 3, 3]; state: new_npt_state's; pressure, rate: a float, or fp64
    [n_graphs]; cell_dof: uint8 / bool [n_graphs] or None (every graph has a barostat; a graph with 0 takes the step of md_step).
    state['seed'] may be None where gamma and kT are the float 0."""
    (dt_g, dt), (kT_g, kT), (gamma_g, gamma) = _split(dt), _split(kT), _split(gamma)
    (p_g, pressure), (rate_g, rate) = _split(pressure), _split(rate)
    lib.call('pamnet_md_npt_step_f32', lib.ptr(pos), lib.ptr(vel), lib.ptr(dpos), lib.ptr(dstrain), lib.ptr(mass), lib.ptr(fixed),
             lib.ptr(gptr), pos.size(0), gptr.numel() - 1, lib.ptr(cell0), lib.ptr(cell), lib.ptr(state['eps']), lib.ptr(cell_dof),
             lib.ptr(state['seed']), lib.ptr(state['steps']), lib.ptr(state['status']), lib.ptr(state['ke']),
             lib.ptr(state['pint']), lib.ptr(state['vol']), dt_g, kT_g, gamma_g, p_g, rate_g, dt, kT, gamma, pressure, rate,
             int(kick_in), int(advance), lib.stream_of(pos))


def temperature(ekin, n_free, remove_com=True, n_constraints=0):
    """kT = 2 KE / dof with dof = 3 n_free - 3 (remove_com) - n_constraints; floats, arrays or tensors, per graph."""
    return 2.0 * ekin / (3 * n_free - (3 if remove_com else 0) - n_constraints)


def colour_constraints(pairs, graph):
    """Greedy colouring on the host, in the order given: constraint k takes the smallest colour that no earlier constraint with
    one of its atoms took, so a graph's colours depend on its own list only.  pairs: int [C, 2], graph: int [C] (numpy).
    Returns (colour [C], order [C]): `order` sorts the constraints by (graph, colour), stably."""
    import numpy as np
    pairs, graph = np.asarray(pairs, dtype=np.int64).reshape(-1, 2), np.asarray(graph, dtype=np.int64).reshape(-1)
    colour, used = np.zeros(len(pairs), dtype=np.int64), {}
    for k, (i, j) in enumerate(pairs.tolist()):
        taken = used.get(i, 0) | used.get(j, 0)   # (bit c set: colour c is taken at one of the two atoms)
        c = (~taken & (taken + 1)).bit_length() - 1
        colour[k] = c
        used[i], used[j] = used.get(i, 0) | (1 << c), used.get(j, 0) | (1 << c)
    return colour, np.lexsort((colour, graph))


class Constraints(object):
    """Distance constraints |x_i - x_j| = d of a batch, checked, coloured and sorted once (one read of the host at set-up), for
    constrained_step / project_constraints / run(constraints=...).

    data_or_batch: the batch (`batch`, `pos`, and `num_graphs` if it has it), or its `batch` tensor [N] alone.
    pairs:   int64 [C, 2], atom rows; both atoms of a pair in one graph, i != j, no pair twice (in either order).
    lengths: fp64 [C], positive and finite; None: the current distances of `data.pos`.
    Holds, on the device of the batch and sorted by (graph, colour): i, j (int32 [C]), d (fp64 [C]), gcol (int32 [G + 1]: the
    colours of a graph), colptr (int32 [K + 1]: the constraints of a colour); n_per_graph (int64 [G]); and on the host pairs,
    colour and graph of the sorted constraints and `order`, their places in the caller's list."""

    def __init__(self, data_or_batch, pairs, lengths=None):
        import numpy as np
        batch = data_or_batch if isinstance(data_or_batch, torch.Tensor) else getattr(data_or_batch, 'batch', None)
        pos = None if isinstance(data_or_batch, torch.Tensor) else getattr(data_or_batch, 'pos', None)
        if not isinstance(batch, torch.Tensor) or batch.dim() != 1:
            raise ValueError('Constraints needs the batch, or its `batch` tensor [N] (the sorted graph id of every atom)')
        device, n = batch.device, batch.numel()
        b = batch.detach().cpu().numpy().astype(np.int64)
        ng = None if isinstance(data_or_batch, torch.Tensor) else getattr(data_or_batch, 'num_graphs', None)
        n_graphs = int(ng) if ng is not None else (int(b[-1]) + 1 if n else 0)
        try:
            p = (pairs.detach().cpu().numpy() if isinstance(pairs, torch.Tensor) else np.asarray(pairs))
        except (TypeError, ValueError):
            raise ValueError('`pairs` is an int64 tensor [C, 2] of atom rows; got %r' % (type(pairs),)) from None
        if p.dtype.kind not in 'iu' or p.ndim != 2 or p.shape[1] != 2:
            if not (p.size == 0 and p.ndim <= 2):
                raise ValueError('`pairs` is an int64 tensor [C, 2] of atom rows; got %s %s' % (p.dtype, tuple(p.shape)))
        p = p.astype(np.int64).reshape(-1, 2)
        C = len(p)
        if C and (p.min() < 0 or p.max() >= n):
            raise ValueError('`pairs` holds atom rows in [0, N) = [0, %d); got %d .. %d' % (n, p.min(), p.max()))
        if (p[:, 0] == p[:, 1]).any():
            raise ValueError('a constraint joins two different atoms; `pairs`[%d] joins an atom to itself'
                             % int(np.nonzero(p[:, 0] == p[:, 1])[0][0]))
        graph = b[p[:, 0]] if C else np.zeros(0, np.int64)
        if C and (graph != b[p[:, 1]]).any():
            raise ValueError('both atoms of a constraint are in one graph; `pairs`[%d] joins two graphs'
                             % int(np.nonzero(graph != b[p[:, 1]])[0][0]))
        if C and (graph.min() < 0 or graph.max() >= n_graphs):
            raise ValueError('`batch` holds graph ids outside [0, num_graphs) = [0, %d)' % n_graphs)
        key = np.sort(p, axis=1)
        if len(np.unique(key[:, 0] * max(n, 1) + key[:, 1])) != C:
            raise ValueError('`pairs` holds a pair twice (the order of its two atoms does not matter)')
        if lengths is None:
            if pos is None:
                raise ValueError('`lengths` is None: the current distances need `data.pos`, and only a `batch` tensor was given')
            x = pos.detach().cpu().numpy().astype(np.float64)
            d = np.sqrt(((x[p[:, 0]] - x[p[:, 1]]) ** 2).sum(1)) if C else np.zeros(0)
        else:
            try:
                d = (lengths.detach().cpu().numpy() if isinstance(lengths, torch.Tensor) else np.asarray(lengths)).astype(np.float64)
            except (TypeError, ValueError):
                raise ValueError('`lengths` is a float64 tensor [C]; got %r' % (type(lengths),)) from None
            if d.shape != (C,):
                raise ValueError('`lengths` is a float64 tensor [C] = [%d], one per pair; got %s' % (C, tuple(d.shape)))
        if not (np.isfinite(d) & (d > 0)).all():
            raise ValueError('the lengths of the constraints must be positive and finite%s'
                             % (' (two constrained atoms of `data.pos` coincide)' if lengths is None else ''))
        colour, order = colour_constraints(p, graph)
        self.order = order
        self.pairs, self.colour, self.graph, self.lengths = p[order], colour[order], graph[order], d[order]
        n_col = np.zeros(n_graphs, dtype=np.int64)                 # colours of a graph: its largest colour + 1
        if C:
            np.maximum.at(n_col, self.graph, self.colour + 1)
        gcol = np.concatenate([[0], np.cumsum(n_col)])
        slot = gcol[self.graph] + self.colour if C else np.zeros(0, np.int64)   # (ascending: the constraints are sorted by it)
        colptr = np.concatenate([[0], np.cumsum(np.bincount(slot, minlength=int(gcol[-1])))])
        if max(C, int(gcol[-1]), n) > 0x7fffffff:
            raise ValueError('the constraint arrays are int32: N, C and the number of colours stay below 2^31')
        to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(device)
        self.n, self.n_atoms, self.n_graphs, self.device = C, n, n_graphs, device
        self.i, self.j, self.d = to(self.pairs[:, 0], np.int32), to(self.pairs[:, 1], np.int32), to(self.lengths, np.float64)
        self.gcol, self.colptr = to(gcol, np.int32), to(colptr, np.int32)
        self.n_per_graph = to(np.bincount(self.graph, minlength=n_graphs), np.int64)
        self._work = None

    def work(self):
        """The fp64 workspace [9 N] (x0, x, v) that constrained_step / project_constraints use where none is passed, made once.
        Launches that share it must follow one another on one stream: concurrent launches (other streams) each need a `work` of
        their own.  run() allocates one per run."""
        if self._work is None:
            self._work = torch.zeros(9 * self.n_atoms, dtype=torch.float64, device=self.device)
        return self._work


def bond_constraints(edge_index, mask):
    """The unique pairs (i < j) of `edge_index` (int [2, E]; both directions of a bond count once) with at least one atom in
    `mask` (bool [N]), e.g. data.z == 1 for the X-H bonds: int64 [C, 2] on the device of `edge_index`, sorted."""
    a, b = edge_index[0].to(torch.int64), edge_index[1].to(torch.int64)
    keep = (a != b) & (mask[a] | mask[b])
    lo, hi = torch.minimum(a, b)[keep], torch.maximum(a, b)[keep]
    n = mask.numel()
    key = torch.unique(lo * n + hi)
    return torch.stack([key // n, key % n], dim=1)


def _cons_args(cons, work):
    if cons.n and work is None:
        work = cons.work()
    elif cons.n and (work.dtype != torch.float64 or work.numel() < 9 * cons.n_atoms or work.device != cons.device):
        raise ValueError('`work` is a float64 tensor of at least 9 N = %d entries on the device of the constraints; got %s [%d] on %s'
                         % (9 * cons.n_atoms, work.dtype, work.numel(), work.device))
    return (lib.ptr(cons.i), lib.ptr(cons.j), lib.ptr(cons.d), lib.ptr(cons.gcol), lib.ptr(cons.colptr), cons.n,
            lib.ptr(work) if cons.n else None)


def constrained_step(pos, vel, dpos, gptr, state, cons, dt, kT=0.0, gamma=0.0, mass=None, fixed=None, kick_in=1, advance=1,
                     tol=1e-8, max_sweeps=500, work=None):
    """One launch of pamnet_md_constrained_step_f32, in place on pos, vel and state (no synchronisation): md_step's arguments,
    `cons` (a Constraints of this batch), and state['sweeps'] (int32 [n_graphs]) beside md_step's state.  work: fp64 [9 n]
    workspace; None: the one `cons` keeps, which launches on one stream may share (Constraints.work)."""
    (dt_g, dt), (kT_g, kT), (gamma_g, gamma) = _split(dt), _split(kT), _split(gamma)
    lib.call('pamnet_md_constrained_step_f32', lib.ptr(pos), lib.ptr(vel), lib.ptr(dpos), lib.ptr(mass), lib.ptr(fixed),
             lib.ptr(gptr), pos.size(0), gptr.numel() - 1, lib.ptr(state['seed']), lib.ptr(state['steps']),
             lib.ptr(state['status']), lib.ptr(state['ke']), dt_g, kT_g, gamma_g, dt, kT, gamma, int(kick_in), int(advance),
             *_cons_args(cons, work), lib.ptr(state['sweeps']), float(tol), int(max_sweeps), lib.stream_of(pos))


def project_constraints(pos, vel, gptr, state, cons, dt=None, mass=None, fixed=None, do_pos=True, do_vel=True, tol=1e-8,
                        max_sweeps=500, work=None):
    """One launch of pamnet_md_project_constraints_f32, in place (no synchronisation): do_pos moves pos onto the lengths (SHAKE
    along the current differences), do_vel removes the velocity along every constraint (RATTLE; needs dt, which scales its
    convergence bound) and writes state['ke'].  vel may be None where do_vel is False.  state: status, ke, sweeps.  work: as for
    constrained_step."""
    dt_g, dt = _split(0.0 if dt is None else dt)
    lib.call('pamnet_md_project_constraints_f32', lib.ptr(pos), lib.ptr(vel), lib.ptr(mass), lib.ptr(fixed), lib.ptr(gptr),
             pos.size(0), gptr.numel() - 1, lib.ptr(state['status']), lib.ptr(state['ke']), dt_g, dt, *_cons_args(cons, work),
             lib.ptr(state['sweeps']), float(tol), int(max_sweeps), int(bool(do_pos)), int(bool(do_vel)), lib.stream_of(pos))


def _per_graph(name, v, n_graphs, device, positive):
    """A float, or an fp64 tensor [num_graphs] on the device of pos -> (the value to hand on, its validity as a 0-dim device bool
    or None).  A float is checked here.  positive: True (> 0), False (>= 0) or None (any finite value)."""
    if isinstance(v, torch.Tensor):
        if v.dtype != torch.float64 or tuple(v.shape) != (n_graphs,) or v.device != device:
            raise ValueError('a per-graph `%s` is a float64 tensor [num_graphs] = [%d] on the device of `pos`; got %s %s on %s'
                             % (name, n_graphs, v.dtype, tuple(v.shape), v.device))
        v = v.contiguous()
        if positive is None:
            return v, torch.isfinite(v).all()
        return v, (torch.isfinite(v) & ((v > 0) if positive else (v >= 0))).all()
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise ValueError('`%s` is a float, or a float64 tensor [num_graphs] on the device of `pos`; got %r' % (name, type(v)))
    if positive is None:
        if v != v or v in (float('inf'), float('-inf')):
            raise ValueError('`%s` must be finite; got %r' % (name, v))
        return v, None
    if not ((v > 0.0 if positive else v >= 0.0) and v != float('inf')):
        raise ValueError('`%s` must be %s and finite; got %r' % (name, 'positive' if positive else 'non-negative', v))
    return v, None


def run(model, data, steps, dt, masses=None, kT=None, gamma=0.0, seed=0, fixed=None, velocities=None, remove_com=True,
        record_every=0, check_every=0, trace=False, constraints=None, constraint_tol=1e-8, constraint_sweeps=500, bias=None):
    """Move every graph of `data` for `steps` steps of length `dt`: velocity Verlet where gamma is 0, Langevin dynamics (BAOAB) at
    temperature kT and friction gamma elsewhere.  One model evaluation and one launch of the integrator per step.

    model:  any callable with model(data) -> [G] that is differentiable with respect to `data.pos`, as for relax(): PAMNet /
            PAMNet_s on the QM9 schema (bonded, bond-free, periodic with `cell` / `pbc` / `cell_images` / `mol_local`, MoleculeStore
            batches), or a plain torch module.  The graph is rebuilt by every evaluation; positions are never wrapped.
    data:   the batch; `data.pos` is never written and no parameter .grad is touched (see relax()).
    dt, kT, gamma: a float, or an fp64 tensor [G] on the device (one value per graph).  gamma > 0 needs kT.  Units are the
            caller's: with eV, Angstrom and amu the time unit is 10.1805 fs.
    masses: fp32 [N] on the device, positive; None: unit masses.
    seed:   an int: graph g gets seed + g, so its noise depends on its place in the batch.  Only an int64 tensor [G] on the device
            -- one seed per structure, chosen by the caller -- makes a graph's noise, and with it its trajectory, independent of
            where in which batch it runs.
    fixed:  bool [N] on the device (True: the atom does not move), or None.
    velocities: fp32 [N, 3] on the device (not written); None: Maxwell-Boltzmann velocities at kT (the centre-of-mass motion
            removed if `remove_com`, not rescaled), or zeros where kT is None.
    record_every: k > 0: the steps 0, k, 2k, ... <= steps are recorded at the full step (x_n and the velocities v_n that belong to
            it) into res.frames [F, N, 3], res.epot and res.ekin [F, G] with F = steps // k + 1, by device-side copies.  Records
            that an early stop (check_every) did not reach stay zero.
    check_every: k > 0: the status vector is read every k steps, to stop once every graph has failed (a non-finite force or
            velocity).  0 (default): never -- everything is enqueued without a synchronisation of the driver's own.
    trace:  for tests and debugging: one dict per launch with clones of pos, dE/dpos, vel and the state before and after it.
    constraints: a Constraints of this batch, or None.  With constraints the rule is g-BAOAB (Leimkuhler & Matthews 2016, one
            geodesic sub-step per half drift; csrc/md_constraints.hip pamnet_md_constrained_step_f32 replaces the step launch):
            the bond lengths are held by SHAKE / RATTLE, which lets `dt` be doubled where X-H vibrations capped it.  At set-up
            the positions are projected onto the lengths and the starting velocities (Maxwell-Boltzmann or given) onto the
            constraints.  A constraint between two fixed atoms is refused.  Positions are never wrapped, so a constrained pair
            must sit in one image.  res.sweeps (int32 [G]) holds the most sweeps a solve of the last launch took,
            res.unconverged (bool [G]) the graphs a solve failed for (status 3): they stop as a failed graph does.  The state of
            a trace record gains `sweeps`.  A temperature counts dof = 3 N - 3 - C: temperature(..., n_constraints=C).
    constraint_tol, constraint_sweeps: the relative bound of both solves and the sweeps one may take.
    bias:   a bias.Bias of this batch, or None: restraints and well-tempered metadynamics over collective variables (CVs).  After
            every evaluation one more launch (csrc/bias.hip pamnet_bias_apply_f64) adds the gradient of the bias to dE/dpos,
            before the step launch -- plain or constrained, unchanged -- reads it; on the steps `it` with it % pace == 0 it also
            deposits one hill per walker (never in the closing launch).  That depends on the loop index only: no decision on the
            host.  Where the Bias was given no `capacity`, its tables grow here by what the run can deposit.  res.forces INCLUDE
            the bias, res.energy and res.epot do NOT (the model alone).  With record_every, res.cv [F, K] (the CVs, in the sorted
            order of the Bias) and res.ebias [F, G] (the bias energies), fp64, are recorded beside epot; without, both are None
            (bias.cv and bias.ebias hold those of res.pos).  NaN marks a graph that was not running.  A graph whose CV or CV
            gradient is not finite fails (status 2) like one with a non-finite force.  A trace record gains dE_model (dE before the bias; dE is what the step launch read), status_before_bias, cv,
            ebias, deposit and n_hills_before / n_hills_after; hills_before / hills_after (centres, heights) where it deposits.
            With None the launches are exactly those without this argument.  run_npt and remd.run take no bias: the virial
            of a bias and its part in the exchange energy are not implemented.

    The first launch opens step 0 (kick_in = 0), every later one closes the step before and opens the next, and one more
    evaluation and a closing launch (advance = 0) end the run: res.vel, res.kinetic, res.energy and res.forces all belong to
    res.pos.  A failed graph stops moving but is still evaluated."""
    if bias is not None:                          # (a refusal that needs no device comes first)
        from .bias import Bias
        p = getattr(data, 'pos', None)
        if not isinstance(bias, Bias) or (isinstance(p, torch.Tensor) and (bias.n_atoms, bias.device) != (p.size(0), p.device)):
            raise ValueError('`bias` is a bias.Bias of this batch (N atoms, on the device of `pos`); got %s'
                             % ('%d atoms on %s' % (bias.n_atoms, bias.device) if isinstance(bias, Bias) else type(bias)))
    try:
        pos, batch, n_graphs, _, fixed8 = _checked(model, data, 0.0, fixed)
    except ValueError as e:
        raise ValueError('md.run takes what relax() takes: %s' % (e,)) from None
    device, n = pos.device, pos.size(0)
    steps, record_every, check_every = int(steps), int(record_every), int(check_every)
    if steps < 0 or record_every < 0 or check_every < 0:
        raise ValueError('`steps`, `record_every` and `check_every` are non-negative; got %d, %d, %d'
                         % (steps, record_every, check_every))
    thermostat = isinstance(gamma, torch.Tensor) or (isinstance(gamma, (int, float)) and gamma > 0)
    if thermostat and kT is None:
        raise ValueError('a thermostat (`gamma` > 0, or per graph) needs its temperature: pass `kT`')
    checks = {}
    dt, checks['dt'] = _per_graph('dt', dt, n_graphs, device, True)
    gamma, checks['gamma'] = _per_graph('gamma', gamma, n_graphs, device, False)
    kT_k, checks['kT'] = _per_graph('kT', 0.0 if kT is None else kT, n_graphs, device, False)
    if masses is not None:
        if (not isinstance(masses, torch.Tensor) or masses.dtype != torch.float32 or tuple(masses.shape) != (n,)
                or masses.device != device):
            raise ValueError('`masses` is a float32 tensor [N] = [%d] on the device of `pos`; got %s'
                             % (n, '%s %s on %s' % (masses.dtype, tuple(masses.shape), masses.device)
                                if isinstance(masses, torch.Tensor) else type(masses)))
        masses = masses.contiguous()
        checks['masses'] = (torch.isfinite(masses) & (masses > 0)).all()
    if velocities is not None and (not isinstance(velocities, torch.Tensor) or velocities.dtype != torch.float32
                                   or tuple(velocities.shape) != (n, 3) or velocities.device != device):
        raise ValueError('`velocities` is a float32 tensor [N, 3] = [%d, 3] on the device of `pos`; got %s'
                         % (n, '%s %s on %s' % (velocities.dtype, tuple(velocities.shape), velocities.device)
                            if isinstance(velocities, torch.Tensor) else type(velocities)))
    cons = constraints
    if cons is not None:
        if not isinstance(cons, Constraints) or (cons.n_atoms, cons.n_graphs, cons.device) != (n, n_graphs, device):
            raise ValueError('`constraints` is a md.Constraints of this batch (N = %d, num_graphs = %d, on %s); got %s'
                             % (n, n_graphs, device, '%d atoms, %d graphs on %s' % (cons.n_atoms, cons.n_graphs, cons.device)
                                if isinstance(cons, Constraints) else type(cons)))
        constraint_tol, constraint_sweeps = float(constraint_tol), int(constraint_sweeps)
        if not (constraint_tol > 0.0 and constraint_tol != float('inf')) or constraint_sweeps < 1:
            raise ValueError('`constraint_tol` is positive and finite and `constraint_sweeps` at least 1; got %r, %r'
                             % (constraint_tol, constraint_sweeps))
        if fixed8 is not None and cons.n:
            checks['constraints'] = ~(fixed8[cons.i.long()] & fixed8[cons.j.long()]).bool().any()
    if bias is not None:
        if (bias.n_atoms, bias.n_graphs, bias.device) != (n, n_graphs, device):
            raise ValueError('`bias` is a bias.Bias of this batch (N = %d, num_graphs = %d, on %s); got %d atoms, %d graphs on %s'
                             % (n, n_graphs, device, bias.n_atoms, bias.n_graphs, bias.device))
        bias.reserve(steps)
    vel, state = new_state(n, n_graphs, device, seed)
    names = [k for k, v in checks.items() if v is not None]
    if names:                                     # (as num_graphs: one read at set-up, for every tensor of values at once)
        ok = torch.stack([checks[k] for k in names]).tolist()
        bad = [k for k, good in zip(names, ok) if not good]
        if 'constraints' in bad:
            raise ValueError('`constraints` holds a pair whose two atoms are both `fixed`: its length cannot change, so there is '
                             'nothing to constrain; drop the pair')
        if bad:
            raise ValueError('%s must be finite and positive (kT, gamma: non-negative) in every entry'
                             % ' and '.join('`%s`' % k for k in bad))
    cur = pos.detach().to(torch.float32).clone().contiguous()
    gptr, _ = G.csr_from_keys(batch.to(torch.int32).contiguous(), n_graphs)
    if cons is not None:                          # the positions onto the lengths, before anything is evaluated
        state['sweeps'] = torch.zeros(n_graphs, dtype=torch.int32, device=device)
        solver = dict(tol=constraint_tol, max_sweeps=constraint_sweeps,     # (a workspace of this run's own: runs of one
                      work=torch.empty(9 * n, dtype=torch.float64, device=device))   # Constraints on other streams share nothing)
        project_constraints(cur, None, gptr, state, cons, None, masses, fixed8, do_pos=True, do_vel=False, **solver)
    if velocities is not None:
        vel = velocities.detach().clone().contiguous()
    elif kT is not None:
        init_velocities(vel, gptr, state['seed'], kT_k, state['ke'], masses, fixed8, remove_com=remove_com)
    if cons is not None and (velocities is not None or kT is not None):
        project_constraints(cur, vel, gptr, state, cons, dt, masses, fixed8, do_pos=False, do_vel=True, **solver)
    keys = STATE if cons is None else CONSTRAINED_STATE
    frames = epot = ekin = cvs = ebiases = None
    if record_every:
        n_rec = steps // record_every + 1
        frames = torch.zeros(n_rec, n, 3, dtype=torch.float32, device=device)
        epot = torch.zeros(n_rec, n_graphs, dtype=torch.float64, device=device)
        ekin = torch.zeros(n_rec, n_graphs, dtype=torch.float64, device=device)
        if bias is not None:
            cvs = torch.zeros(n_rec, bias.n_cvs, dtype=torch.float64, device=device)
            ebiases = torch.zeros(n_rec, n_graphs, dtype=torch.float64, device=device)
    log = [] if trace else None

    def launch(it, kick_in, advance):
        """Evaluate at cur, then the bias launch if there is one, then one launch; step `it` is recorded at its full step: cur
        before the launch, ke after it."""
        e, de = _evaluate(model, data, cur)
        rec = record_every and it % record_every == 0
        if rec:
            frames[it // record_every].copy_(cur)
            epot[it // record_every].copy_(e.reshape(-1))
        if bias is not None:
            deposit = 1 if advance and bias.pace and it % bias.pace == 0 else 0
            if trace:
                tb = dict(dE_model=de.clone(), status_before_bias=state['status'].clone(), deposit=deposit,
                          n_hills_before=bias.tab['n_hills'].clone())
                if deposit:
                    tb['hills_before'] = (bias.tab['hill_c'].clone(), bias.tab['hill_w'].clone())
            bias.apply(cur, de, state['status'], deposit)
            if rec:
                cvs[it // record_every].copy_(bias.cv)
                ebiases[it // record_every].copy_(bias.ebias)
            if trace:
                tb.update(cv=bias.cv.clone(), ebias=bias.ebias.clone(), n_hills_after=bias.tab['n_hills'].clone())
                if deposit:
                    tb['hills_after'] = (bias.tab['hill_c'].clone(), bias.tab['hill_w'].clone())
        if trace:
            t = dict(pos=cur.clone(), dE=de.clone(), v_before=vel.clone(), kick_in=kick_in, advance=advance,
                     state_before={k: state[k].clone() for k in keys})
        if cons is None:
            md_step(cur, vel, de, gptr, state, dt, kT_k, gamma, masses, fixed8, kick_in, advance)
        else:
            constrained_step(cur, vel, de, gptr, state, cons, dt, kT_k, gamma, masses, fixed8, kick_in, advance, **solver)
        if rec:
            ekin[it // record_every].copy_(state['ke'])
        if trace:
            t.update(pos_after=cur.clone(), v_after=vel.clone(), state_after={k: state[k].clone() for k in keys})
            if bias is not None:
                t.update(tb)
            log.append(t)
        return e, de

    done = 0
    for it in range(steps):
        launch(it, 1 if it else 0, 1)
        done = it + 1
        if check_every and done % check_every == 0 and not bool((state['status'] == RUNNING).any()):
            break
    energy, de = launch(done, 1 if done else 0, 0)  # one more evaluation: energy, forces, vel and ke belong to the final geometry
    res = MDResult(pos=cur, vel=vel, energy=energy, kinetic=state['ke'], forces=-de, steps=state['steps'],
                   failed=state['status'] == FAILED, frames=frames, epot=epot, ekin=ekin, trace=log)
    if cons is not None:
        res.unconverged, res.sweeps = state['status'] == UNCONVERGED, state['sweeps']
    if bias is not None:
        res.cv, res.ebias = cvs, ebiases
    return res


def run_npt(model, data, steps, dt, kT, pressure, tau_p, compressibility, masses=None, gamma=0.0, seed=0, fixed=None,
            velocities=None, remove_com=True, cell_dof=None, record_every=0, check_every=0, trace=False):
    """Move every graph of a periodic batch for `steps` steps of length `dt` at the temperature kT and the pressure `pressure`:
    the BAOAB step of run() with the isotropic stochastic cell rescaling barostat (Bernetti & Bussi 2020) in the same launch
    (include/pamnet_hip.h states the rule).  One model evaluation -- with `strain` attached, for the virial -- and one launch per
    step; no decision on the host.

    model:  as for run(), and differentiable with respect to `data.strain` as well, as for relax_cell(): PAMNet / PAMNet_s on
            periodic batches, or a plain torch module that applies (I + data.strain[g]) to the positions and the cell of graph g.
            The graph build's own conditions on the cell heights apply to every evaluation; the driver adds none.
    data:   the batch, with `data.cell` fp32 [G, 3, 3] (row k = lattice vector a_k); neither `data.pos` nor `data.cell` is written.
    dt, kT, gamma, masses, seed, fixed, velocities, remove_com, record_every, check_every: as for run().  kT is required: it
            sets the barostat's noise.  kT = 0 gives a deterministic relaxation of the volume towards `pressure`.  A fixed atom
            of a graph with a barostat keeps its fractional coordinates: it follows the cell.
    pressure: P0, a float or fp64 [G] on the device, finite, in the caller's energy / length^3 (with eV and Angstrom:
            160.2177 GPa; 1 bar = 6.2415e-7).
    tau_p, compressibility: the coupling time and the isothermal compressibility beta_T (1 / pressure), floats or fp64 [G] on the
            device, positive.  Only rate = compressibility / tau_p enters the rule; the explicit update wants
            rate x bulk modulus x dt well below 1.
    cell_dof: bool [G] on the device: False = the graph has no barostat and takes exactly the step of run().  None: a graph has
            one where all three axes of `data.pbc` are periodic (everywhere where the batch has no `pbc`).  True on a graph with
            an open axis is refused.
    trace:  as for run(); a record also holds W and cell, and the states hold eps, pint and vol; cell_after beside pos_after.

    The launch sequence and the records are those of run(): res.vel, res.kinetic, res.pressure, res.volume, res.energy,
    res.forces, res.virial and res.stress all belong to res.pos and res.cell.  With record_every, res.cells, res.volumes and
    res.pressures are recorded beside frames, epot and ekin."""
    try:
        pos, batch, n_graphs, _, fixed8 = _checked(model, data, 0.0, fixed)
    except ValueError as e:
        raise ValueError('md.run_npt takes what relax() takes: %s' % (e,)) from None
    device, n = pos.device, pos.size(0)
    cell_in = getattr(data, 'cell', None)
    if cell_in is None:
        raise ValueError('run_npt needs `data.cell` (fp32 [num_graphs, 3, 3], row k = lattice vector a_k): the batch has no `cell`, '
                         'and a structure in open space has no volume to couple to a pressure; run() moves it at fixed shape')
    if (not isinstance(cell_in, torch.Tensor) or cell_in.dtype != torch.float32 or tuple(cell_in.shape) != (n_graphs, 3, 3)
            or cell_in.device != device):
        raise ValueError('`data.cell` is a float32 tensor [num_graphs, 3, 3] = [%d, 3, 3] on the device of `pos`; got %s'
                         % (n_graphs, '%s %s on %s' % (cell_in.dtype, tuple(cell_in.shape), cell_in.device)
                            if isinstance(cell_in, torch.Tensor) else type(cell_in)))
    steps, record_every, check_every = int(steps), int(record_every), int(check_every)
    if steps < 0 or record_every < 0 or check_every < 0:
        raise ValueError('`steps`, `record_every` and `check_every` are non-negative; got %d, %d, %d'
                         % (steps, record_every, check_every))
    if kT is None:
        raise ValueError('constant-pressure dynamics needs its temperature: pass `kT` (it sets the noise of the barostat; kT = 0 '
                         'relaxes the volume without noise)')
    checks = {}
    dt, checks['dt'] = _per_graph('dt', dt, n_graphs, device, True)
    gamma, checks['gamma'] = _per_graph('gamma', gamma, n_graphs, device, False)
    kT, checks['kT'] = _per_graph('kT', kT, n_graphs, device, False)
    pressure, checks['pressure'] = _per_graph('pressure', pressure, n_graphs, device, None)
    tau_p, checks['tau_p'] = _per_graph('tau_p', tau_p, n_graphs, device, True)
    compressibility, checks['compressibility'] = _per_graph('compressibility', compressibility, n_graphs, device, True)
    rate = compressibility / tau_p                # (a float, or fp64 [G] on the device)
    if isinstance(rate, torch.Tensor):
        rate = rate.contiguous()
    elif not (rate > 0.0 and rate != float('inf')):
        raise ValueError('`compressibility` / `tau_p` must be positive and finite; got %r' % (rate,))
    if masses is not None:
        if (not isinstance(masses, torch.Tensor) or masses.dtype != torch.float32 or tuple(masses.shape) != (n,)
                or masses.device != device):
            raise ValueError('`masses` is a float32 tensor [N] = [%d] on the device of `pos`; got %s'
                             % (n, '%s %s on %s' % (masses.dtype, tuple(masses.shape), masses.device)
                                if isinstance(masses, torch.Tensor) else type(masses)))
        masses = masses.contiguous()
        checks['masses'] = (torch.isfinite(masses) & (masses > 0)).all()
    if velocities is not None and (not isinstance(velocities, torch.Tensor) or velocities.dtype != torch.float32
                                   or tuple(velocities.shape) != (n, 3) or velocities.device != device):
        raise ValueError('`velocities` is a float32 tensor [N, 3] = [%d, 3] on the device of `pos`; got %s'
                         % (n, '%s %s on %s' % (velocities.dtype, tuple(velocities.shape), velocities.device)
                            if isinstance(velocities, torch.Tensor) else type(velocities)))
    dof8 = _cell_dof(data, cell_dof, n_graphs, device, checks, 'has a barostat on')
    cell0 = cell_in.detach().clone().contiguous()
    cell = cell0.clone()
    vel, state = new_npt_state(n, n_graphs, device, cell0, seed)
    names = [k for k, v in checks.items() if v is not None]
    if names:                                     # (as run: one read at set-up, for every tensor of values at once)
        ok = torch.stack([checks[k] for k in names]).tolist()
        bad = [k for k, good in zip(names, ok) if not good]
        if 'cell_dof' in bad:
            raise ValueError('`cell_dof` is True on a graph with an open axis (`data.pbc`): a cell with an open axis has no volume '
                             'to couple to a pressure; leave that graph False, or run the structure as fully periodic')
        if bad:
            raise ValueError('%s must be finite and positive (kT, gamma: non-negative; pressure: any sign) in every entry'
                             % ' and '.join('`%s`' % k for k in bad))
    cur = pos.detach().to(torch.float32).clone().contiguous()
    gptr, _ = G.csr_from_keys(batch.to(torch.int32).contiguous(), n_graphs)
    if velocities is not None:
        vel = velocities.detach().clone().contiguous()
    else:
        init_velocities(vel, gptr, state['seed'], kT, state['ke'], masses, fixed8, remove_com=remove_com)
    frames = epot = ekin = cells = volumes = pressures = None
    if record_every:
        n_rec = steps // record_every + 1
        f64 = dict(dtype=torch.float64, device=device)
        frames = torch.zeros(n_rec, n, 3, dtype=torch.float32, device=device)
        cells = torch.zeros(n_rec, n_graphs, 3, 3, dtype=torch.float32, device=device)
        epot, ekin = torch.zeros(n_rec, n_graphs, **f64), torch.zeros(n_rec, n_graphs, **f64)
        volumes, pressures = torch.zeros(n_rec, n_graphs, **f64), torch.zeros(n_rec, n_graphs, **f64)
    log = [] if trace else None
    snap = lambda: {k: state[k].clone() for k in NPT_STATE}

    def launch(it, kick_in, advance):
        """Evaluate at cur and cell, then one launch; step `it` is recorded at its full step: cur and cell before the launch, ke,
        pint and vol (which the launch forms for that geometry) after it."""
        e, de, w = _evaluate_cell(model, data, cur, cell)
        rec = record_every and it % record_every == 0
        if rec:
            frames[it // record_every].copy_(cur)
            cells[it // record_every].copy_(cell)
            epot[it // record_every].copy_(e.reshape(-1))
        if trace:
            t = dict(pos=cur.clone(), dE=de.clone(), W=w.clone(), cell=cell.clone(), v_before=vel.clone(), kick_in=kick_in,
                     advance=advance, state_before=snap())
        npt_step(cur, vel, de, w, gptr, cell0, cell, state, dt, kT, pressure, rate, gamma, masses, fixed8, dof8, kick_in, advance)
        if rec:
            ekin[it // record_every].copy_(state['ke'])
            volumes[it // record_every].copy_(state['vol'])
            pressures[it // record_every].copy_(state['pint'])
        if trace:
            t.update(pos_after=cur.clone(), v_after=vel.clone(), cell_after=cell.clone(), state_after=snap())
            log.append(t)
        return e, de, w

    done = 0
    for it in range(steps):
        launch(it, 1 if it else 0, 1)
        done = it + 1
        if check_every and done % check_every == 0 and not bool((state['status'] == RUNNING).any()):
            break
    energy, de, w = launch(done, 1 if done else 0, 0)   # one more evaluation: everything belongs to the final geometry
    volume = state['vol']
    return MDResult(pos=cur, vel=vel, cell=cell, eps=state['eps'], energy=energy, kinetic=state['ke'], forces=-de, virial=w,
                    stress=(w.to(torch.float64) / volume[:, None, None]).to(torch.float32), volume=volume, pressure=state['pint'],
                    steps=state['steps'], failed=state['status'] == FAILED, frames=frames, epot=epot, ekin=ekin, cells=cells,
                    volumes=volumes, pressures=pressures, trace=log)
