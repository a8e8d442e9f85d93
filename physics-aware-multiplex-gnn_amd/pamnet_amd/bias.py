"""Biased dynamics over collective variables on the device: harmonic restraints (umbrella windows, walls) and well-tempered
metadynamics (Barducci, Bussi & Parrinello, Phys. Rev. Lett. 100, 020603, 2008) with multiple walkers (Raiteri et al., J. Phys.
Chem. B 110, 3533, 2006), for md.run(bias=...).

    from pamnet_amd import bias, md
    b = bias.Bias(data, [bias.dihedral(4, 6, 8, 14), bias.dihedral(6, 8, 14, 16)],
                  metadynamics=dict(ndim=2, sigma=0.35, height=0.012, bias_factor=8.0, kT=0.0259, pace=50))
    res = md.run(model, data, steps=20000, dt=0.1, masses=m, kT=0.0259, gamma=0.1, seed=seeds, bias=b, record_every=10)
    res.cv, res.ebias                                 # the recorded variables [F, K] and bias energies [F, G]
    b.free_energy(grid)                               # -gamma / (gamma - 1) V on a grid of points, minimum 0

    w = bias.Bias(data, [bias.distance(0, 5)], restraints={0: dict(kappa=40.0, centre=2.5)})            # an umbrella window
    rep = remd.replicate(data, 4)                     # four walkers per structure on one hill table each
    b4 = bias.Bias(rep, cvs_of_every_copy, metadynamics=dict(...), walkers=4)

The bias is per-graph state on the device: one launch of pamnet_bias_apply_f64 per step (csrc/bias.hip; include/pamnet_hip.h states
the rule) between the model evaluation and the step launch forms every collective variable (CV) in fp64, adds the gradient of
the bias to dE/dpos and, every `pace` steps, appends one hill per walker.  Its sums run in a fixed order and it uses no atomics,
so a structure's trajectory is bitwise the same alone or in any batch, and from run to run.  There is no CPU path."""
import numpy as np
import torch

from . import lib

MAX_CVS = 16                                      # the CVs of one graph at most (csrc/bias.hip BIAS_MAX_CVS)
MAX_WALKERS = 256                                 # the graphs of one group at most (BIAS_MAX_WALKERS)
KINDS = ('distance', 'angle', 'dihedral')
N_ATOMS = (2, 3, 4)
CVS = ('cvptr', 'kind', 'atoms', 'kappa', 'centre', 'halfwidth')
GROUPS = ('bptr', 'ndim', 'sigma', 'height0', 'inv_dT')
TABLE = ('hill_c', 'hill_w', 'n_hills', 'dropped')
_METAD = ('ndim', 'sigma', 'height', 'bias_factor', 'kT', 'pace')


def distance(i, j):
    """The CV |x_j - x_i| of two atom rows."""
    return ('distance', (int(i), int(j)))


def angle(i, j, k):
    """The CV angle at atom j between the atoms i and k, in radians, in [0, pi]."""
    return ('angle', (int(i), int(j), int(k)))


def dihedral(i, j, k, l):
    """The CV dihedral angle of four atom rows about the bond j - k, in radians, in (-pi, pi] (IUPAC sign); periodic."""
    return ('dihedral', (int(i), int(j), int(k), int(l)))


def apply_launch(pos, dpos, status, gptr, tab, deposit, cv, ebias):
    """One launch of pamnet_bias_apply_f64 on plain tensors, in place on dpos, status and the hill table (no synchronisation).
    tab: a dict of the tensors named in CVS, GROUPS and TABLE, as include/pamnet_hip.h lays them out."""
    p = lib.ptr
    lib.call('pamnet_bias_apply_f64', p(pos), p(dpos), p(status), p(gptr), p(tab['bptr']), p(tab['cvptr']), p(tab['kind']),
             p(tab['atoms']), p(tab['kappa']), p(tab['centre']), p(tab['halfwidth']), p(tab['ndim']), p(tab['sigma']),
             p(tab['height0']), p(tab['inv_dT']), p(tab['hill_c']), p(tab['hill_w']), p(tab['n_hills']), p(tab['dropped']), p(cv),
             p(ebias), pos.size(0), gptr.numel() - 1, tab['bptr'].numel() - 1, tab['kind'].numel(), tab['hill_w'].size(1),
             int(deposit), lib.stream_of(pos))


def grid_launch(tab, periodic, table, points, out):
    """One launch of pamnet_bias_grid_f64: out[i] = V of table `table` at points[i] (fp64 [M, ndim])."""
    p = lib.ptr
    lib.call('pamnet_bias_grid_f64', p(tab['hill_c']), p(tab['hill_w']), p(tab['n_hills']), p(tab['sigma']), p(periodic), p(points),
             p(out), int(table), tab['hill_w'].size(0), tab['hill_w'].size(1), points.size(0), points.size(1), lib.stream_of(points))


def _group_ptr(walkers, n_graphs):
    """`walkers` -> the group pointer as a host list, checked: None (every graph alone), an int W (num_graphs % W == 0), or an
    int list / int32 tensor [T + 1] that starts at 0, does not decrease and ends at num_graphs; no group above MAX_WALKERS."""
    if walkers is None:
        return list(range(n_graphs + 1))
    if isinstance(walkers, torch.Tensor):
        if walkers.dtype != torch.int32 or walkers.dim() != 1:
            raise ValueError('a `walkers` tensor is the group pointer: int32 [T + 1]; got %s %s' % (walkers.dtype, tuple(walkers.shape)))
        ptr = walkers.tolist()
    elif isinstance(walkers, (list, tuple)):
        try:
            ptr = [int(v) for v in walkers]
        except (TypeError, ValueError):
            raise ValueError('a `walkers` list is the group pointer of T + 1 ints; got %r' % (walkers,)) from None
    else:
        try:
            W = int(walkers)
        except (TypeError, ValueError):
            raise ValueError('`walkers` is None, an int W, or the group pointer as an int list or an int32 tensor [T + 1]; got %r'
                             % (type(walkers),)) from None
        if W < 1 or n_graphs % W:
            raise ValueError('`walkers` = %d must be positive and divide num_graphs = %d: group t is the graphs [t W, (t + 1) W)'
                             % (W, n_graphs))
        ptr = list(range(0, n_graphs + 1, W))
    if not ptr or ptr[0] != 0 or ptr[-1] != n_graphs or any(b < a for a, b in zip(ptr[:-1], ptr[1:])):
        raise ValueError('the group pointer starts at 0, does not decrease and ends at num_graphs = %d; got %r'
                         % (n_graphs, ptr if len(ptr) <= 12 else ptr[:6] + ['...'] + ptr[-3:]))
    most = max([b - a for a, b in zip(ptr[:-1], ptr[1:])] or [0])
    if most > MAX_WALKERS:
        raise ValueError('a group has at most %d walkers (one workgroup takes a group); the largest of `walkers` has %d'
                         % (MAX_WALKERS, most))
    return ptr


class Bias(object):
    """The collective variables, restraints and hill tables of a batch, checked and sorted once (one read of the host at
    set-up, as md.Constraints), for md.run(bias=...).

    data_or_batch: the batch (`batch`, and `num_graphs` if it has it), or its `batch` tensor [N] alone.
    cvs:     a list of distance(i, j) / angle(i, j, k) / dihedral(i, j, k, l) over atom rows; the atoms of a CV are distinct and
             in one graph; at most 16 per graph.  They are sorted by graph, stably: `order` holds the caller's index of every
             sorted CV, and res.cv of md.run is in the sorted order (the caller's, where the list goes graph by graph).
    restraints: {index into `cvs`: dict(kappa=, centre=, halfwidth=0.0)}: E = 1/2 kappa max(0, |s - centre| - halfwidth)^2.
             halfwidth 0 is an umbrella window, halfwidth > 0 a pair of walls at centre -+ halfwidth.  A dihedral's difference is
             periodic.
    metadynamics: dict(ndim=1 | 2, sigma=a float or one per dimension, height=, bias_factor=gamma > 1 or None (plain
             metadynamics), kT= (needed with a bias factor), pace=steps between two hills): the FIRST ndim CVs of every graph
             carry the hills.  A group whose graphs have no CV at all takes no hills; any other needs ndim CVs in every graph.
    walkers: None: every graph has a hill table of its own.  An int W: the graphs [t W, (t + 1) W) are W walkers on table t
             (remd.replicate(data, W) builds such a batch).  Or the group pointer, an int list or int32 tensor [T + 1].  The
             walkers of a group must list the same CVs (kinds and atoms, relative to the first atom of the graph).
    capacity: the hills a table can hold.  None: md.run sizes the table for its run, W (steps // pace + 1) more than it holds.
             Where a table is full, hills are dropped and `dropped` counts them.

    Holds, on the device of the batch: cvptr, kind, atoms, kappa, centre, halfwidth (sorted), bptr, ndim, sigma, height0, inv_dT,
    periodic, gptr, and after the tables exist hill_c [T, capacity, 2], hill_w [T, capacity], n_hills, dropped [T]."""

    def __init__(self, data_or_batch, cvs, restraints=None, metadynamics=None, walkers=None, capacity=None):
        batch = data_or_batch if isinstance(data_or_batch, torch.Tensor) else getattr(data_or_batch, 'batch', None)
        if not isinstance(batch, torch.Tensor) or batch.dim() != 1:
            raise ValueError('Bias needs the batch, or its `batch` tensor [N] (the sorted graph id of every atom)')
        device, n = batch.device, batch.numel()
        b = batch.detach().cpu().numpy().astype(np.int64)          # the one read
        ng = None if isinstance(data_or_batch, torch.Tensor) else getattr(data_or_batch, 'num_graphs', None)
        n_graphs = int(ng) if ng is not None else (int(b[-1]) + 1 if n else 0)
        if n and (b.min() < 0 or b.max() >= n_graphs or (np.diff(b) < 0).any()):
            raise ValueError('`batch` holds the sorted graph id of every atom, in [0, num_graphs) = [0, %d)' % n_graphs)
        gptr = np.concatenate([[0], np.cumsum(np.bincount(b, minlength=n_graphs))]).astype(np.int64)
        # ---- the CVs
        kinds, atoms = [], []
        for c, spec in enumerate(cvs):
            try:
                name, at = spec
                at = tuple(int(a) for a in at)
            except (TypeError, ValueError):
                raise ValueError('`cvs`[%d] is not a CV: build them with distance(), angle() and dihedral(); got %r' % (c, spec)) from None
            if name not in KINDS or len(at) != N_ATOMS[KINDS.index(name)]:
                raise ValueError('`cvs`[%d]: a %r CV over %d atoms is unknown: distance (2 atoms), angle (3) or dihedral (4)'
                                 % (c, name, len(at)))
            if min(at) < 0 or max(at) >= n:
                raise ValueError('`cvs`[%d] holds atom rows in [0, N) = [0, %d); got %r' % (c, n, at))
            if len(set(at)) != len(at):
                raise ValueError('the atoms of a CV are distinct; `cvs`[%d] = %s%r repeats an atom' % (c, name, at))
            if len(set(b[list(at)].tolist())) != 1:
                raise ValueError('the atoms of a CV are in one graph; `cvs`[%d] = %s%r joins two graphs' % (c, name, at))
            kinds.append(KINDS.index(name))
            atoms.append(at + (at[0],) * (4 - len(at)))
        K = len(kinds)
        kinds, atoms = np.asarray(kinds, dtype=np.int64).reshape(K), np.asarray(atoms, dtype=np.int64).reshape(K, 4)
        graph = b[atoms[:, 0]] if K else np.zeros(0, np.int64)
        per_graph = np.bincount(graph, minlength=n_graphs)
        if K and per_graph.max() > MAX_CVS:
            raise ValueError('a graph has at most %d CVs (one thread forms each); graph %d has %d'
                             % (MAX_CVS, int(per_graph.argmax()), int(per_graph.max())))
        order = np.argsort(graph, kind='stable')
        self.order = order
        self.cv_kind, self.cv_atoms, self.cv_graph = kinds[order], atoms[order], graph[order]
        cvptr = np.concatenate([[0], np.cumsum(per_graph)]).astype(np.int64)
        # ---- the restraints
        kappa, centre, halfwidth = np.zeros(K), np.zeros(K), np.zeros(K)
        place = np.empty(K, dtype=np.int64)
        place[order] = np.arange(K)                                # the caller's CV c is the sorted CV place[c]
        for c, r in (restraints or {}).items():
            if not isinstance(c, (int, np.integer)) or not 0 <= c < K:
                raise ValueError('`restraints` maps an index into `cvs` (0 .. %d) to dict(kappa=, centre=, halfwidth=0.0); got the key %r'
                                 % (K - 1, c))
            if not isinstance(r, dict) or set(r) - {'kappa', 'centre', 'halfwidth'} or not {'kappa', 'centre'} <= set(r):
                raise ValueError('`restraints`[%d] is dict(kappa=, centre=, halfwidth=0.0); got %r' % (c, r))
            k_, c_, h_ = float(r['kappa']), float(r['centre']), float(r.get('halfwidth', 0.0))
            if not (np.isfinite([k_, c_, h_]).all() and k_ >= 0.0 and h_ >= 0.0):
                raise ValueError('`restraints`[%d]: kappa and halfwidth are non-negative and finite, centre is finite; got %r' % (c, r))
            kappa[place[c]], centre[place[c]], halfwidth[place[c]] = k_, c_, h_
        # ---- the groups
        bptr = np.asarray(_group_ptr(walkers, n_graphs), dtype=np.int64)
        T = len(bptr) - 1
        rel = self.cv_atoms - gptr[self.cv_graph][:, None] if K else self.cv_atoms
        for t in range(T):
            g0 = int(bptr[t])
            first = (self.cv_kind[cvptr[g0]:cvptr[g0 + 1]], rel[cvptr[g0]:cvptr[g0 + 1]]) if bptr[t + 1] > g0 else None
            for g in range(g0 + 1, int(bptr[t + 1])):
                s = slice(cvptr[g], cvptr[g + 1])
                if not (np.array_equal(self.cv_kind[s], first[0]) and np.array_equal(rel[s], first[1])):
                    raise ValueError('the walkers of a group list the same CVs -- kinds and atoms, counted from the first atom of '
                                     'the graph --: graph %d differs from graph %d, the first of its group' % (g, g0))
        # ---- metadynamics
        ndim, sigma, height0, inv_dT = np.zeros(T, np.int64), np.ones((T, 2)), np.zeros(T), np.zeros(T)
        self.pace, self.bias_factor = 0, None
        if metadynamics is not None:
            if not isinstance(metadynamics, dict) or set(metadynamics) - set(_METAD) or not {'ndim', 'sigma', 'height', 'pace'} <= set(metadynamics):
                raise ValueError('`metadynamics` is dict(ndim, sigma, height, pace, bias_factor=None, kT=None); got %r' % (metadynamics,))
            nd = metadynamics['ndim']
            if nd not in (1, 2):
                raise ValueError('`metadynamics`: ndim is 1 or 2 (the first ndim CVs of every graph carry the hills); got %r' % (nd,))
            sg = np.atleast_1d(np.asarray(metadynamics['sigma'], dtype=np.float64))
            sg = np.repeat(sg, nd) if sg.shape == (1,) else sg
            if sg.shape != (nd,) or not (np.isfinite(sg) & (sg > 0)).all():
                raise ValueError('`metadynamics`: sigma is positive and finite, a float or one per dimension; got %r'
                                 % (metadynamics['sigma'],))
            h0, pace = float(metadynamics['height']), metadynamics['pace']
            if not (h0 > 0.0 and np.isfinite(h0)):
                raise ValueError('`metadynamics`: height is positive and finite; got %r' % (metadynamics['height'],))
            if not isinstance(pace, (int, np.integer)) or pace < 1:
                raise ValueError('`metadynamics`: pace is a positive int, the steps between two hills; got %r' % (pace,))
            bf, kT = metadynamics.get('bias_factor'), metadynamics.get('kT')
            idt = 0.0
            if bf is not None:
                if not (float(bf) > 1.0 and np.isfinite(float(bf))):
                    raise ValueError('`metadynamics`: bias_factor is above 1 (None: plain metadynamics, the limit of a large one); '
                                     'got %r' % (bf,))
                if kT is None or not (float(kT) > 0.0 and np.isfinite(float(kT))):
                    raise ValueError('`metadynamics`: a bias_factor needs the temperature: kT positive and finite; got %r' % (kT,))
                idt = 1.0 / (float(kT) * (float(bf) - 1.0))
                self.bias_factor = float(bf)
            for t in range(T):
                counts = per_graph[bptr[t]:bptr[t + 1]]
                if len(counts) == 0 or not counts.any():
                    continue                                       # a group without CVs takes no hills
                if counts.min() < nd:
                    raise ValueError('`metadynamics`: the first ndim = %d CVs of every graph carry the hills; graph %d has %d'
                                     % (nd, int(bptr[t]) + int(counts.argmin()), int(counts.min())))
                ndim[t], height0[t], inv_dT[t] = nd, h0, idt
                sigma[t, :nd] = sg
            self.pace = int(pace)
        periodic = np.zeros((T, 2), dtype=np.int64)
        for t in range(T):
            if ndim[t]:
                k0 = cvptr[bptr[t]]
                periodic[t, :ndim[t]] = self.cv_kind[k0:k0 + ndim[t]] == KINDS.index('dihedral')
        if capacity is not None and (not isinstance(capacity, (int, np.integer)) or capacity < 0):
            raise ValueError('`capacity` is a non-negative int, the hills one table can hold, or None; got %r' % (capacity,))
        if max(K, n, n_graphs) > 0x7fffffff:
            raise ValueError('the bias arrays are int32: N, num_graphs and the number of CVs stay below 2^31')
        to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(device)
        self.n_cvs, self.n_atoms, self.n_graphs, self.n_groups, self.device = K, n, n_graphs, T, device
        self.group_ptr, self.group_ndim, self.group_periodic = bptr, ndim, periodic
        self.max_walkers = int(np.diff(bptr).max()) if T else 0
        self.gptr = to(gptr, np.int32)
        self.tab = dict(cvptr=to(cvptr, np.int32), kind=to(self.cv_kind, np.int32), atoms=to(self.cv_atoms, np.int32),
                        kappa=to(kappa, np.float64), centre=to(centre, np.float64), halfwidth=to(halfwidth, np.float64),
                        bptr=to(bptr, np.int32), ndim=to(ndim, np.int32), sigma=to(sigma, np.float64),
                        height0=to(height0, np.float64), inv_dT=to(inv_dT, np.float64))
        self.periodic = to(periodic, np.int32)
        self.cv = torch.full((K,), float('nan'), dtype=torch.float64, device=device)
        self.ebias = torch.full((n_graphs,), float('nan'), dtype=torch.float64, device=device)
        self._fixed_capacity = capacity is not None
        self.capacity = None
        if capacity is not None or not self.pace:
            self._allocate(int(capacity or 0))

    # the tables ---------------------------------------------------------------------------------------------------------
    def _allocate(self, capacity):
        """Tables of `capacity` hills; the hills held so far are copied over (device-side, no synchronisation)."""
        T, dev = self.n_groups, self.device
        hill_c = torch.zeros(T, capacity, 2, dtype=torch.float64, device=dev)
        hill_w = torch.zeros(T, capacity, dtype=torch.float64, device=dev)
        if self.capacity:
            hill_c[:, :self.capacity].copy_(self.tab['hill_c'])
            hill_w[:, :self.capacity].copy_(self.tab['hill_w'])
        else:
            self.tab['n_hills'] = torch.zeros(T, dtype=torch.int32, device=dev)
            self.tab['dropped'] = torch.zeros(T, dtype=torch.int32, device=dev)
        self.tab['hill_c'], self.tab['hill_w'], self.capacity = hill_c, hill_w, capacity

    def reserve(self, steps):
        """Room for a run of `steps` steps: where `capacity` was left None, the tables grow by W (steps // pace + 1) hills --
        the most the run can deposit.  md.run calls it; a given `capacity` stays."""
        if self.pace and not self._fixed_capacity:
            self._allocate((self.capacity or 0) + self.max_walkers * (int(steps) // self.pace + 1))

    # the launches -------------------------------------------------------------------------------------------------------
    def apply(self, pos, dpos, status, deposit):
        """One launch of pamnet_bias_apply_f64, in place on dpos (fp32 [N, 3]: the bias gradient is added), status (int32 [G])
        and, where deposit is 1, the hill tables; self.cv (fp64 [K]) and self.ebias (fp64 [G]) are written.  No synchronisation."""
        if self.capacity is None:
            raise ValueError('the hill tables have no size yet: pass `capacity` to Bias, or call reserve(steps) as md.run does')
        apply_launch(pos, dpos, status, self.gptr, self.tab, deposit, self.cv, self.ebias)

    def _points(self, points, group):
        group = int(group)
        if not 0 <= group < self.n_groups or not self.group_ndim[group]:
            raise ValueError('`group` names a group with hills, in [0, %d); got %r' % (self.n_groups, group))
        if self.capacity is None:
            raise ValueError('the hill tables have no size yet: nothing was deposited')
        nd = int(self.group_ndim[group])
        p = torch.as_tensor(points, dtype=torch.float64).to(self.device)
        p = p.reshape(-1, 1) if p.dim() == 1 and nd == 1 else p
        if p.dim() != 2 or p.size(1) != nd:
            raise ValueError('`points` is [M, ndim] = [M, %d] (or [M] where ndim is 1); got %s' % (nd, tuple(p.shape)))
        return p.contiguous(), group

    def potential(self, points, group=0):
        """V of the hill table of `group` at `points` ([M, ndim], or [M] where ndim is 1): fp64 [M] on the device, one launch of
        pamnet_bias_grid_f64."""
        p, group = self._points(points, group)
        out = torch.empty(p.size(0), dtype=torch.float64, device=self.device)
        grid_launch(self.tab, self.periodic, group, p, out)
        return out

    def free_energy(self, points, group=0):
        """The free-energy estimate on `points`: -gamma / (gamma - 1) V with the bias factor gamma (well-tempered), -V for
        plain metadynamics; shifted so that its minimum over the points is 0.  fp64 [M] on the device."""
        v = self.potential(points, group)
        f = -v if self.bias_factor is None else -(self.bias_factor / (self.bias_factor - 1.0)) * v
        return f - f.min() if f.numel() else f

    def hills(self, group=0):
        """(centres [n_hills, ndim], heights [n_hills]) of the table of `group`: views of the tables (one read of n_hills)."""
        group = int(group)
        if not 0 <= group < self.n_groups:
            raise ValueError('`group` is in [0, %d); got %r' % (self.n_groups, group))
        if self.capacity is None:
            raise ValueError('the hill tables have no size yet: nothing was deposited')
        m = int(self.tab['n_hills'][group])
        return self.tab['hill_c'][group, :m, :int(self.group_ndim[group])], self.tab['hill_w'][group, :m]
