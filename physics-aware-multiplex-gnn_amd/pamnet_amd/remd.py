"""Replica-exchange molecular dynamics (parallel tempering; Sugita & Okamoto, Chem. Phys. Lett. 314, 141, 1999) on the device:
temperature ladders as graphs of one batch.

    from pamnet_amd import remd
    rep = remd.replicate(data, 8)                                     # every structure 8 times, consecutively: one ladder each
    kT = remd.temperatures(0.025, 0.08, 8).repeat(data.num_graphs).to(device)
    res = remd.run(model, rep, steps=10000, dt=0.1, kT=kT, replicas=8, exchange_every=100, gamma=0.1, masses=m, record_every=100)
    res.acceptance()                                                  # accepted / tried of every neighbouring pair
    res.by_rung(res.epot)                                             # the records in rung order: column lo + r is rung r

A ladder of R temperatures is R consecutive graphs of the batch, so its dynamics is md.run's: one model evaluation and one launch
of pamnet_md_step_f32 per step, with the temperature per graph that launch already takes.  Every `exchange_every` steps one more
launch -- pamnet_remd_exchange_f64 (csrc/remd.hip; include/pamnet_hip.h states the rule) -- takes the Metropolis decision for every
neighbouring pair of every ladder on the device and swaps TEMPERATURES, not configurations: no position, graph or neighbour
structure moves, only kT per graph, the rung tables and a scale of the velocities.  Its noise is counter-based (Philox4x32-10
keyed by the ladder's seed, counted by the rung and the ladder's attempt), so a ladder's trajectory is bitwise the same alone or in
any batch, and from run to run.  The loop takes no decision on the host.  There is no CPU path."""
import numpy as np
import torch

from . import graph as G
from . import lib
from .md import (CONSTRAINED_STATE, FAILED, RUNNING, STATE, UNCONVERGED, Constraints, MDResult, _per_graph, constrained_step,
                 init_velocities, md_step, new_state, project_constraints)
from .relax import _checked, _evaluate

MAX_RUNGS = 256                                   # the rungs of one ladder at most (csrc/remd.hip REMD_MAX_RUNGS)
LADDER = ('kT_g', 'rung', 'slot', 'attempts', 'tried', 'accepted')


class REMDResult(MDResult):
    """MDResult's fields (pos, vel, energy, forces, kinetic, steps, failed, frames, epot, ekin, trace; unconverged and sweeps with
    constraints), in WALKER order -- graph g is the configuration that started on rung g - lo of its ladder, whatever
    temperature it holds now -- plus: kT fp64 [G] (the temperatures held at the end), rung, slot int32 [G], attempts int32 [L],
    tried, accepted int32 [G] (entry lo + r: the pair (r, r + 1); the last entry of a ladder stays 0), rungs int32 [A + 1, G] (the
    rung of every graph after each of the A exchange launches; row 0: the start), frame_rung int32 [F, G] (the rung a graph held
    during a recorded step; None without record_every), lptr int32 [L + 1], exchange_seed int64 [L].  All on the device."""

    def acceptance(self):
        """accepted / tried per pair, fp64 [G]; NaN where nothing was tried."""
        return self.accepted.to(torch.float64) / self.tried.to(torch.float64)

    def by_rung(self, values, atoms=None):
        """A record in walker order -> rung order, with frame_rung: values [F, G, ...] (epot, ekin): column lo + r of the result is
        the graph that held rung r of its ladder during the step; values [F, N, ...] (frames): the atoms of that graph, through
        gptr (the graphs of a ladder hold the same atoms).  atoms: True / False says which; None: per atom where values.size(1) is
        N and not G.  Post-processing in plain torch."""
        if self.frame_rung is None:
            raise ValueError('by_rung reorders recorded steps: run with `record_every` > 0')
        n_graphs, n = self.frame_rung.size(1), self.pos.size(0)
        if atoms is None:
            atoms = values.dim() >= 2 and values.size(1) == n and n != n_graphs
        if values.dim() < 2 or values.size(0) != self.frame_rung.size(0) or values.size(1) != (n if atoms else n_graphs):
            raise ValueError('`values` is [F, G, ...] = [%d, %d, ...] (or [F, N, ...] = [%d, %d, ...], per atom); got %s'
                             % (self.frame_rung.size(0), n_graphs, self.frame_rung.size(0), n, tuple(values.shape)))
        dest = self._first[None, :] + self.frame_rung.long()               # [F, G]: where graph g of a record goes
        if atoms:
            gptr, batch = self._gptr.long(), self._batch.long()
            dest = gptr[dest[:, batch]] + (torch.arange(n, device=dest.device) - gptr[batch])[None, :]
        out = torch.empty_like(values)
        out[torch.arange(values.size(0), device=dest.device)[:, None], dest] = values
        return out


def temperatures(kT_min, kT_max, n, device=None):
    """A geometric ladder of n temperatures from kT_min to kT_max (both positive, kT_min <= kT_max): fp64 [n]."""
    kT_min, kT_max, n = float(kT_min), float(kT_max), int(n)
    if not (0.0 < kT_min <= kT_max < float('inf')) or n < 1:
        raise ValueError('a ladder has n >= 1 temperatures with 0 < kT_min <= kT_max; got %r, %r, %r' % (kT_min, kT_max, n))
    if n == 1:
        return torch.tensor([kT_min], dtype=torch.float64, device=device)
    t = torch.arange(n, dtype=torch.float64) / (n - 1)
    out = kT_min * (kT_max / kT_min) ** t
    out[-1] = kT_max
    return out.to(device) if device is not None else out


def _upload(a, dtype, device):
    """A host array on `device` without a synchronisation: through pinned memory, as an asynchronous copy on the current stream."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype))
    return t.pin_memory().to(device, non_blocking=True) if torch.device(device).type == 'cuda' else t.to(device)


def _ladder_ptr(replicas, n_graphs):
    """`replicas` -> lptr as a host list, checked: an int R (num_graphs % R == 0), or an int list / int32 tensor [L + 1] that starts
    at 0, does not decrease and ends at num_graphs; no ladder above MAX_RUNGS."""
    if isinstance(replicas, torch.Tensor):
        if replicas.dtype != torch.int32 or replicas.dim() != 1:
            raise ValueError('a `replicas` tensor is the ladder pointer `lptr`: int32 [L + 1]; got %s %s'
                             % (replicas.dtype, tuple(replicas.shape)))
        lptr = replicas.tolist()                  # (a pointer on the device: one read at set-up; an int or a list costs none)
    elif isinstance(replicas, (list, tuple)):
        try:
            lptr = [int(v) for v in replicas]
        except (TypeError, ValueError):
            raise ValueError('a `replicas` list is the ladder pointer `lptr` of L + 1 ints; got %r' % (replicas,)) from None
    else:
        try:
            R = int(replicas)
        except (TypeError, ValueError):
            raise ValueError('`replicas` is an int R, or the ladder pointer `lptr` as an int list or an int32 tensor [L + 1]; '
                             'got %r' % (type(replicas),)) from None
        if R < 1 or n_graphs % R:
            raise ValueError('`replicas` = %d must be positive and divide num_graphs = %d: ladder l is the graphs [l R, (l + 1) R)'
                             % (R, n_graphs))
        lptr = list(range(0, n_graphs + 1, R))
    if not lptr or lptr[0] != 0 or lptr[-1] != n_graphs or any(b < a for a, b in zip(lptr[:-1], lptr[1:])):
        raise ValueError('the ladder pointer `lptr` starts at 0, does not decrease and ends at num_graphs = %d; got %r'
                         % (n_graphs, lptr if len(lptr) <= 12 else lptr[:6] + ['...'] + lptr[-3:]))
    most = max([b - a for a, b in zip(lptr[:-1], lptr[1:])] or [0])
    if most > MAX_RUNGS:
        raise ValueError('a ladder has at most %d rungs (one workgroup decides a ladder); the longest of `replicas` has %d'
                         % (MAX_RUNGS, most))
    return lptr


def new_ladder_state(kT, lptr, exchange_seed=0):
    """The state of pamnet_remd_exchange_f64 at the start, every graph on the rung of its place: dict of lptr (int32 [L + 1]),
    kT_ladder (fp64 [G]: kT itself), kT_g (a copy: what the step launch reads), rung, slot (int32 [G]), seed (int64 [L]), attempts
    (int32 [L]), tried, accepted (int32 [G]), on the device of kT.  kT: fp64 [G]; lptr: what run() takes as `replicas`;
    exchange_seed: an int -- ladder l gets exchange_seed + l -- or an int64 tensor [L] on the device of kT."""
    if not isinstance(kT, torch.Tensor) or kT.dtype != torch.float64 or kT.dim() != 1:
        raise ValueError('`kT` is a float64 tensor [num_graphs], the temperature of the rung every graph starts on; got %s'
                         % ('%s %s' % (kT.dtype, tuple(kT.shape)) if isinstance(kT, torch.Tensor) else type(kT)))
    device, n_graphs = kT.device, kT.numel()
    host = _ladder_ptr(lptr, n_graphs)
    n_ladders = len(host) - 1
    if isinstance(exchange_seed, torch.Tensor):
        if exchange_seed.dtype != torch.int64 or tuple(exchange_seed.shape) != (n_ladders,) or exchange_seed.device != device:
            raise ValueError('a per-ladder `exchange_seed` is an int64 tensor [num_ladders] = [%d] on the device of `kT`; got %s %s '
                             'on %s' % (n_ladders, exchange_seed.dtype, tuple(exchange_seed.shape), exchange_seed.device))
        seed = exchange_seed.contiguous()
    else:
        try:
            seed = int(exchange_seed) + torch.arange(n_ladders, dtype=torch.int64, device=device)
        except (TypeError, ValueError):
            raise ValueError('`exchange_seed` is an int, or an int64 tensor [num_ladders] on the device of `kT`; got %r'
                             % (type(exchange_seed),)) from None
    first = np.repeat(np.asarray(host[:-1], dtype=np.int64), np.diff(np.asarray(host, dtype=np.int64)))
    i32 = lambda a: _upload(a, np.int32, device)
    zeros = lambda m: torch.zeros(m, dtype=torch.int32, device=device)
    return dict(lptr=i32(host), kT_ladder=kT.detach().contiguous(), kT_g=kT.detach().clone().contiguous(),
                rung=i32(np.arange(n_graphs) - first), slot=i32(np.arange(n_graphs)), seed=seed, attempts=zeros(n_ladders),
                tried=zeros(n_graphs), accepted=zeros(n_graphs))


def exchange(energy, vel, gptr, ladder, status, ke, fixed=None):
    """One launch of pamnet_remd_exchange_f64, in place on vel, ke and ladder (new_ladder_state's; no synchronisation).  energy:
    fp64 [n_graphs], the potential energies at the current positions; vel: fp32 [n, 3], the velocities that belong to them (after
    a closing step launch); gptr: int32 [n_graphs + 1]; status: int32 [n_graphs], ke: fp64 [n_graphs] (the step's state); fixed:
    uint8 / bool [n] or None."""
    lib.call('pamnet_remd_exchange_f64', lib.ptr(energy), lib.ptr(vel), lib.ptr(fixed), lib.ptr(gptr), lib.ptr(ladder['lptr']),
             lib.ptr(ladder['kT_ladder']), lib.ptr(ladder['kT_g']), lib.ptr(ladder['rung']), lib.ptr(ladder['slot']),
             lib.ptr(status), lib.ptr(ke), lib.ptr(ladder['seed']), lib.ptr(ladder['attempts']), lib.ptr(ladder['tried']),
             lib.ptr(ladder['accepted']), vel.size(0), gptr.numel() - 1, ladder['lptr'].numel() - 1, lib.stream_of(vel))


def replicate(data, n):
    """Every graph of `data` repeated n times consecutively (n: an int, or a list of one int per graph, each at least 1): the
    batch of the ladders.  pos, x, batch, num_graphs and edge_index (offset per copy) are replicated; y, cell, pbc, cell_images
    and mol_local per graph, as neb.interpolate does; `ladder_ptr` (int32 [B + 1], on the host) is attached, which
    run(replicas=None) uses.  Plain torch at set-up, one device -> host read (the atom and edge counts of the graphs)."""
    from .synth import Batch
    pos, batch = getattr(data, 'pos', None), getattr(data, 'batch', None)
    if pos is None or batch is None:
        raise ValueError('replicate needs `data.pos` and `data.batch`; the batch has no `%s`' % ('pos' if pos is None else 'batch'))
    if pos.dim() != 2 or batch.numel() != pos.size(0):
        raise ValueError('`data.pos` must be [N, 3] with one `data.batch` entry per row; got %s and %s'
                         % (tuple(pos.shape), tuple(batch.shape)))
    device = pos.device
    ng = getattr(data, 'num_graphs', None)
    B = int(ng) if ng is not None else (int(batch[-1]) + 1 if batch.numel() else 0)
    if isinstance(n, (list, tuple)):
        copies = [int(v) for v in n]
        if len(copies) != B:
            raise ValueError('`n` is an int or a list of num_graphs = %d ints; got %d entries' % (B, len(copies)))
    else:
        copies = [int(n)] * B
    if any(v < 1 for v in copies):
        raise ValueError('every graph is repeated at least once; got n = %r' % (n,))
    x, ei = getattr(data, 'x', None), getattr(data, 'edge_index', None)
    counts = torch.bincount(batch.long(), minlength=B)
    ecount = torch.bincount(batch.long()[ei[0].long()], minlength=B) if ei is not None else counts.new_zeros(0)
    host = torch.cat([counts, ecount]).tolist()                                                       # the one read
    counts_h, ecount_h = np.asarray(host[:B], dtype=np.int64), np.asarray(host[B:], dtype=np.int64)
    aptr = np.concatenate([[0], np.cumsum(counts_h)])
    graph_src = np.repeat(np.arange(B), copies)                    # new graph (b, c) copies graph b
    new_counts = counts_h[graph_src]
    new_aptr = np.concatenate([[0], np.cumsum(new_counts)])
    atom_src = np.concatenate([np.arange(aptr[b], aptr[b + 1]) for b in graph_src]) if len(graph_src) else np.zeros(0, np.int64)
    atom_graph = np.repeat(np.arange(len(graph_src)), new_counts)
    up = lambda arr, dtype: torch.from_numpy(np.ascontiguousarray(arr)).to(dtype).to(device)
    src, gsrc = up(atom_src, torch.long), up(graph_src, torch.long)
    out = Batch(pos=pos[src], batch=up(atom_graph, batch.dtype), num_graphs=int(len(graph_src)),
                ladder_ptr=torch.from_numpy(np.concatenate([[0], np.cumsum(copies)]).astype(np.int32)))
    if x is not None:
        out.x = x[src]
    if ei is not None:
        order = torch.sort(batch.long()[ei[0].long()], stable=True)[1]                                # edges grouped by graph
        eptr = np.concatenate([[0], np.cumsum(ecount_h)])
        e_src = np.concatenate([np.arange(eptr[b], eptr[b + 1]) for b in graph_src]) if len(graph_src) else np.zeros(0, np.int64)
        e_off = np.repeat(new_aptr[:-1] - aptr[graph_src], ecount_h[graph_src])
        out.edge_index = ei[:, order][:, up(e_src, torch.long)] + up(e_off, ei.dtype)[None]
    for name in ('y', 'cell', 'pbc', 'cell_images', 'mol_local'):
        v = getattr(data, name, None)
        if v is None:
            continue
        per_graph = isinstance(v, torch.Tensor) and v.dim() >= 1 and v.size(0) == B
        setattr(out, name, v[gsrc.to(v.device)] if per_graph else v)
    return out


def run(model, data, steps, dt, kT, replicas=None, exchange_every=0, gamma=None, masses=None, seed=0, exchange_seed=0, fixed=None,
        velocities=None, remove_com=True, record_every=0, check_every=0, trace=False, constraints=None, constraint_tol=1e-8,
        constraint_sweeps=500):
    """Langevin dynamics (md.run's BAOAB step) of temperature ladders with exchange attempts between neighbouring rungs.

    model, data, steps, dt, masses, seed, fixed, velocities, remove_com, record_every, check_every, constraints, constraint_tol,
            constraint_sweeps: as for md.run.  The graphs of one ladder must hold the same atoms (equal atom counts, equal
            `data.x` where present) and, with `constraints`, the same number of constraints: remd.replicate builds such a batch.
    kT:     fp64 [G] on the device, positive: entry g is the temperature of the rung graph g starts on -- ascending inside a
            ladder by convention (remd.temperatures); only neighbouring entries exchange.
    replicas: an int R -- num_graphs % R == 0 and ladder l is the graphs [l R, (l + 1) R) --, or the ladder pointer `lptr` as an
            int list or int32 tensor [L + 1] (a tensor on the device costs one read at set-up).  None: `data.ladder_ptr`
            (remd.replicate attaches it).  A ladder has at most 256 rungs; one of a single graph never exchanges.
    exchange_every: k > 0: step `it` is an exchange step where it > 0 and it % k == 0.  0: never; the launches are md.run's.
    gamma:  a float or fp64 [G], positive everywhere: the exchange rule assumes that every rung samples the canonical ensemble
            at its temperature, which dynamics without a thermostat does not.
    exchange_seed: an int -- ladder l gets exchange_seed + l -- or an int64 tensor [L] on the device: with per-graph `seed`
            tensors too, a ladder's trajectory does not depend on where in which batch it runs.
    trace:  as for md.run; a record gains kind = 'step', the evaluation's energy and kT (the temperatures the launch read), and
            every exchange launch adds one of kind = 'exchange' with clones of energy (fp64), status, and of vel, ke, kT_g, rung,
            slot, attempts, tried and accepted before and after.

    On an exchange step the evaluation at the current positions is followed by three launches: the step launch with (kick_in 1,
    advance 0), which leaves the velocities and `ke` belonging to the positions; the exchange with that evaluation's energies; and
    the step launch with (kick_in 0, advance 1) on the same forces, which opens the next step at the exchanged temperatures.  A
    recorded frame of an exchange step is taken before the exchange: it belongs to the rung res.frame_rung names.  The closing
    launch of the run is never followed by an exchange.  Beyond the one read at set-up that md.run makes for its value checks --
    the ladder checks are folded into it -- nothing synchronises.  Returns a REMDResult."""
    pos, batch = getattr(data, 'pos', None), getattr(data, 'batch', None)
    ng = getattr(data, 'num_graphs', None)
    if pos is not None and batch is not None:     # the refusals that need no device come first
        n_graphs = int(ng) if ng is not None else (int(batch.reshape(-1)[-1]) + 1 if batch.numel() else 0)
        steps, record_every, check_every, exchange_every = int(steps), int(record_every), int(check_every), int(exchange_every)
        if steps < 0 or record_every < 0 or check_every < 0 or exchange_every < 0:
            raise ValueError('`steps`, `record_every`, `check_every` and `exchange_every` are non-negative; got %d, %d, %d, %d'
                             % (steps, record_every, check_every, exchange_every))
        if gamma is None or (not isinstance(gamma, torch.Tensor) and not (isinstance(gamma, (int, float)) and gamma > 0)):
            raise ValueError('replica exchange needs a thermostat on every graph: `gamma` must be positive (a float, or fp64 '
                             '[num_graphs]); got %r.  The exchange rule assumes that each rung samples the canonical ensemble at '
                             'its temperature, which dynamics without a thermostat does not' % (gamma,))
        if not isinstance(kT, torch.Tensor) or kT.dtype != torch.float64 or tuple(kT.shape) != (n_graphs,):
            raise ValueError('`kT` is a float64 tensor [num_graphs] = [%d] on the device of `pos`, the temperature of the rung '
                             'every graph starts on; got %s' % (n_graphs, '%s %s' % (kT.dtype, tuple(kT.shape))
                                                                if isinstance(kT, torch.Tensor) else type(kT)))
        if replicas is None:
            replicas = getattr(data, 'ladder_ptr', None)
            if replicas is None:
                raise ValueError('`replicas` is None and the batch has no `ladder_ptr` (remd.replicate attaches one): pass the '
                                 'replicas per ladder, or the ladder pointer')
        lptr_h = _ladder_ptr(replicas, n_graphs)
    try:
        pos, batch, n_graphs, _, fixed8 = _checked(model, data, 0.0, fixed)
    except ValueError as e:
        raise ValueError('remd.run takes what relax() takes: %s' % (e,)) from None
    device, n = pos.device, pos.size(0)
    checks = {}
    dt, checks['dt'] = _per_graph('dt', dt, n_graphs, device, True)
    gamma, checks['gamma'] = _per_graph('gamma', gamma, n_graphs, device, True)
    kT_k, checks['kT'] = _per_graph('kT', kT, n_graphs, device, True)
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
    vel, state = new_state(n, n_graphs, device, seed)
    ladder = new_ladder_state(kT_k, lptr_h, exchange_seed)
    gptr, _ = G.csr_from_keys(batch.to(torch.int32).contiguous(), n_graphs)
    # the graphs of a ladder hold the same atoms: every graph against the first of its ladder, on the device
    first_h = np.repeat(np.asarray(lptr_h[:-1], dtype=np.int64), np.diff(np.asarray(lptr_h, dtype=np.int64)))
    first = _upload(first_h, np.int64, device)
    if n_graphs:
        glong = gptr.long()
        counts = glong[1:] - glong[:-1]
        same = (counts == counts[first]).all()
        x = getattr(data, 'x', None)
        if isinstance(x, torch.Tensor) and x.size(0) == n and n:
            b = batch.long()
            twin = (glong[first[b]] + (torch.arange(n, device=device) - glong[b])).clamp_(0, n - 1)   # the atom's twin there
            same = same & (x == x[twin]).all()
        checks['ladder atoms'] = same
        if cons is not None:
            checks['ladder constraints'] = (cons.n_per_graph == cons.n_per_graph[first]).all()
    names = [k for k, v in checks.items() if v is not None]
    if names:                                     # (as md.run: one read at set-up, for every tensor of values at once)
        ok = torch.stack([checks[k] for k in names]).tolist()
        bad = [k for k, good in zip(names, ok) if not good]
        if 'ladder atoms' in bad:
            raise ValueError('the graphs of one ladder must hold the same atoms -- equal atom counts, and equal `data.x` atom by '
                             'atom --: they are replicas of one structure at different temperatures (remd.replicate builds them)')
        if 'ladder constraints' in bad:
            raise ValueError('with `constraints`, every graph of a ladder must have the same number of constraints '
                             '(`constraints.n_per_graph`): an exchange hands a graph the temperature of another with the same '
                             'degrees of freedom')
        if 'constraints' in bad:
            raise ValueError('`constraints` holds a pair whose two atoms are both `fixed`: its length cannot change, so there is '
                             'nothing to constrain; drop the pair')
        if bad:
            raise ValueError('%s must be finite and positive in every entry' % ' and '.join('`%s`' % k for k in bad))
    kT_g = ladder['kT_g']                         # what the step launch reads: the exchange rewrites it in place
    cur = pos.detach().to(torch.float32).clone().contiguous()
    if cons is not None:                          # the positions onto the lengths, before anything is evaluated
        state['sweeps'] = torch.zeros(n_graphs, dtype=torch.int32, device=device)
        solver = dict(tol=constraint_tol, max_sweeps=constraint_sweeps,
                      work=torch.empty(9 * n, dtype=torch.float64, device=device))
        project_constraints(cur, None, gptr, state, cons, None, masses, fixed8, do_pos=True, do_vel=False, **solver)
    if velocities is not None:
        vel = velocities.detach().clone().contiguous()
    else:
        init_velocities(vel, gptr, state['seed'], kT_g, state['ke'], masses, fixed8, remove_com=remove_com)
    if cons is not None:
        project_constraints(cur, vel, gptr, state, cons, dt, masses, fixed8, do_pos=False, do_vel=True, **solver)
    keys = STATE if cons is None else CONSTRAINED_STATE
    frames = epot = ekin = frame_rung = None
    if record_every:
        n_rec = steps // record_every + 1
        frames = torch.zeros(n_rec, n, 3, dtype=torch.float32, device=device)
        epot = torch.zeros(n_rec, n_graphs, dtype=torch.float64, device=device)
        ekin = torch.zeros(n_rec, n_graphs, dtype=torch.float64, device=device)
        frame_rung = torch.zeros(n_rec, n_graphs, dtype=torch.int32, device=device)
    n_swaps = (steps - 1) // exchange_every if exchange_every and steps else 0
    rungs = torch.zeros(n_swaps + 1, n_graphs, dtype=torch.int32, device=device)
    rungs[0].copy_(ladder['rung'])
    log = [] if trace else None
    snap = lambda: {k: state[k].clone() for k in keys}

    def step(e, de, kick_in, advance):
        if trace:
            t = dict(kind='step', pos=cur.clone(), energy=e.clone(), dE=de.clone(), v_before=vel.clone(), kick_in=kick_in,
                     advance=advance, kT=kT_g.clone(), state_before=snap())
        if cons is None:
            md_step(cur, vel, de, gptr, state, dt, kT_g, gamma, masses, fixed8, kick_in, advance)
        else:
            constrained_step(cur, vel, de, gptr, state, cons, dt, kT_g, gamma, masses, fixed8, kick_in, advance, **solver)
        if trace:
            t.update(pos_after=cur.clone(), v_after=vel.clone(), state_after=snap())
            log.append(t)

    def launch(it, kick_in, advance, swap):
        """Evaluate at cur, then one launch -- or, on an exchange step, the closing launch, the exchange and the opening launch;
        step `it` is recorded at its full step: cur and the rungs before the launches, ke after the first of them."""
        e, de = _evaluate(model, data, cur)
        rec = record_every and it % record_every == 0
        if rec:
            frames[it // record_every].copy_(cur)
            epot[it // record_every].copy_(e.reshape(-1))
            frame_rung[it // record_every].copy_(ladder['rung'])
        step(e, de, kick_in, 0 if swap else advance)
        if rec:
            ekin[it // record_every].copy_(state['ke'])
        if swap:
            e64 = e.detach().reshape(-1).to(torch.float64).contiguous()
            if trace:
                t = dict(kind='exchange', energy=e64.clone(), v_before=vel.clone(), ke_before=state['ke'].clone(),
                         status=state['status'].clone(), ladder_before={k: ladder[k].clone() for k in LADDER})
            exchange(e64, vel, gptr, ladder, state['status'], state['ke'], fixed8)
            rungs[it // exchange_every].copy_(ladder['rung'])
            if trace:
                t.update(v_after=vel.clone(), ke_after=state['ke'].clone(), ladder_after={k: ladder[k].clone() for k in LADDER})
                log.append(t)
            step(e, de, 0, 1)
        return e, de

    done = 0
    for it in range(steps):
        launch(it, 1 if it else 0, 1, bool(exchange_every) and it > 0 and it % exchange_every == 0)
        done = it + 1
        if check_every and done % check_every == 0 and not bool((state['status'] == RUNNING).any()):
            break
    energy, de = launch(done, 1 if done else 0, 0, False)   # one more evaluation: energy, forces, vel and ke belong to res.pos
    res = REMDResult(pos=cur, vel=vel, energy=energy, kinetic=state['ke'], forces=-de, steps=state['steps'],
                     failed=state['status'] == FAILED, frames=frames, epot=epot, ekin=ekin, trace=log, kT=kT_g, rung=ladder['rung'],
                     slot=ladder['slot'], attempts=ladder['attempts'], tried=ladder['tried'], accepted=ladder['accepted'],
                     rungs=rungs, frame_rung=frame_rung, lptr=ladder['lptr'], exchange_seed=ladder['seed'], _first=first, _gptr=gptr, _batch=batch)
    if cons is not None:
        res.unconverged, res.sweeps = state['status'] == UNCONVERGED, state['sweeps']
    return res
