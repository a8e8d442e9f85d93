"""Vibrational analysis: the bookkeeping launches pamnet_vib_displace_f32 / pamnet_vib_rows_f64 (csrc/vib.hip), the batched
symmetric eigensolver pamnet_sym_eig_f64 (csrc/eig.hip) and the drivers of pamnet_amd/vib.py.

The references are tests/vib_ref.py: displace_ref and rows_ref (the two bookkeeping rules) and jacobi_ref (the solver's rule), all
numpy fp64, and numpy.linalg.eigvalsh.  Inputs are made once on the CPU with fixed seeds and never modified.

Tolerances, with eps = 2^-52 and |A| the Frobenius norm of the symmetrised input:
  solver:  max |w - w_eigvalsh| and max |V A - diag(w) V| <= 8 d eps |A|, max |V V^T - I| <= 8 d eps, sweeps <= 20.  jacobi_ref
           itself stays below 0.65 / 1.97 / 1.67 of d eps (|A|) and 16 sweeps on the matrices here (the 1.97 is the residual of the
           noisy kind, 0.33 elsewhere); the factor of four to five covers fused multiply-adds and the kernel's summation order.
  rows:    4 eps relative (three correctly rounded fp64 operations after an exact widening).  displace: equality.
  Hessian of the analytic potential: the element bound _Wells.bound derives from the truncation term, the fp32 rounding of the two
           gradients and the midpoint offset; eigenvalues: d times the largest element bound (Weyl)."""
import copy
import warnings

import numpy as np
import pytest
import torch

from vib_ref import displace_ref, jacobi_ref, job_of, layout, round_pairs, rows_ref

ENTRIES = ('pamnet_vib_displace_f32', 'pamnet_vib_rows_f64', 'pamnet_sym_eig_f64')
EPS = 2.0 ** -52
KINDS = ('random', 'degenerate', 'zero6', 'graded', 'noisy')
GPU_KINDS = KINDS + ('diagonal', 'zero', 'nan', 'inf')
CPU_DIMS = (1, 2, 3, 5, 6, 9, 63, 64, 65, 87, 96, 192)
GPU_DIMS = (0, 1, 2, 3, 5, 6, 9, 63, 64, 65, 87, 96, 97, 192)   # (96 | 97: A staged in LDS | worked on in global memory)
SENTINEL = -7.25
MODELS = [(32, 2), (128, 1)]
_MADE = {}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs an MI355X'
    from pamnet_amd import lib
    lib.load()
    return torch.device('cuda:0')


class Case(object):
    pass


# ------------------------------------------------------------------------------------------------------- matrices
def _orthogonal(rng, d):
    q, r = np.linalg.qr(rng.standard_normal((d, d)))
    return q * np.sign(np.diag(r))


def _matrix(kind, d):
    """The test matrix of a kind and a dimension (not symmetric where the kind says so: symmetrisation is part of the rule)."""
    key = ('matrix', kind, d)
    if key in _MADE:
        return _MADE[key]
    rng = np.random.RandomState(1000 + 7 * d + GPU_KINDS.index(kind))
    if kind == 'random':
        a = rng.standard_normal((d, d))
    elif kind == 'degenerate':                    # every eigenvalue three times (the last group shorter)
        lam = np.repeat(rng.uniform(-2.0, 2.0, (d + 2) // 3), 3)[:d]
        q = _orthogonal(rng, d)
        a = (q * lam) @ q.T
    elif kind in ('zero6', 'noisy'):              # B B^T with six zero modes; `noisy` adds 1e-5 of asymmetric noise
        b = rng.standard_normal((d, max(d - 6, 1)))
        a = b @ b.T
        if kind == 'noisy':
            a = a + 1e-5 * rng.standard_normal((d, d))
    elif kind == 'graded':                        # 1e-6 .. 1e2, both signs
        lam = np.logspace(-6.0, 2.0, d) * np.where(np.arange(d) % 2 == 0, 1.0, -1.0)
        q = _orthogonal(rng, d)
        a = (q * lam) @ q.T
    elif kind == 'diagonal':
        a = np.diag(rng.uniform(-3.0, 3.0, d))
    elif kind == 'zero':
        a = np.zeros((d, d))
    else:                                         # one NaN / one Inf in an otherwise random matrix
        a = rng.standard_normal((d, d))
        a[d // 2, d // 3] = np.nan if kind == 'nan' else np.inf
    _MADE[key] = np.ascontiguousarray(a, dtype=np.float64)
    return _MADE[key]


def _reference(kind, d, tol=1e-15):
    key = ('jacobi', kind, d, tol)
    if key not in _MADE:
        _MADE[key] = jacobi_ref(_matrix(kind, d), tol, 30)
    return _MADE[key]


def _assert_solution(a, w, v, sweeps, tag):
    """The conditions of the solver on one finite matrix -> the three errors in units of d eps (|A|)."""
    d = a.shape[0]
    s = (a + a.T) * 0.5
    norm = np.sqrt((s * s).sum())
    ew = np.abs(w - np.linalg.eigvalsh(s)).max()
    er = np.abs(v @ s - w[:, None] * v).max()
    eo = np.abs(v @ v.T - np.eye(d)).max()
    assert ew <= 8 * d * EPS * norm and er <= 8 * d * EPS * norm and eo <= 8 * d * EPS, (tag, ew, er, eo, norm)
    assert (np.diff(w) >= 0).all() and sweeps <= 20, (tag, sweeps)
    top = np.abs(v).argmax(1)
    assert (v[np.arange(d), top] > 0).all(), (tag, 'sign convention')
    scale = d * EPS * norm if norm else 1.0
    return ew / scale, er / scale, eo / (d * EPS)


# ------------------------------------------------------------------------------------------- the analytic potential
W_SLOTS = 22
# atoms, where atom 0 sits, (h, kappa, s, k_t), fixed offsets inside the graph
W_GRAPHS = [(1, 'min', (1.0, 2.0, 0.5, 1.0), ()), (2, 'saddle', (1.5, 3.0, 0.75, 1.5), ()),
            (4, 'general', (0.8, 1.5, 0.625, 2.0), ()), (22, 'min', (2.0, 2.5, 0.5, 1.2), ()),
            (4, 'saddle', (1.5, 2.0, 0.5, 1.0), (2,)), (1, 'general', (1.0, 3.0, 0.75, 1.0), ()),
            (22, 'saddle', (1.0, 2.0, 0.625, 0.8), (5, 6)), (2, 'min', (0.8, 1.5, 0.75, 2.0), ())]
W_DELTA, W_PAIRS = 0.01, 3


class _Wells(object):
    """Per graph, atom 0 sits in h (x^2 - 1)^2 + kappa (y - s (1 - x^2))^2 + kappa z^2 and every other atom a is tethered to it by
    1/2 k_t |r_a - r_0 - delta_a|^2: minima at x = -1 / +1, one first-order saddle at (0, s, 0).  The Hessian is known in closed
    form: H_xx = 4 h (3 x^2 - 1) + 4 kappa s q + 8 kappa s^2 x^2 with q = y - s (1 - x^2), H_xy = 4 kappa s x, H_yy = H_zz =
    2 kappa on atom 0; + k_t I on both diagonal blocks and - k_t I between atom 0 and a tethered atom.  The only derivatives
    beyond the second are E_xxx = 24 (h + kappa s^2) x, E_xxy = 4 kappa s and E_xxxx = 24 h + 24 kappa s^2, all on atom 0."""

    def __init__(self, graphs=tuple(range(len(W_GRAPHS)))):
        self.graphs = tuple(graphs)
        pos, delta, par, counts, fixed, kinds = [], [], [], [], [], []
        for g in graphs:
            m, kind, p, fx = W_GRAPHS[g]
            rng = np.random.RandomState(400 + g)
            dl = np.concatenate([np.zeros((1, 3)), rng.uniform(-1.0, 1.0, (m - 1, 3))])
            r0 = {'min': [1.0 if g % 2 else -1.0, 0.0, 0.0], 'saddle': [0.0, p[2], 0.0], 'general': [0.37, 0.61, -0.19]}[kind]
            r = np.asarray(r0) + dl
            if kind == 'general':
                r[1:] += 0.05 * rng.uniform(-1.0, 1.0, (m - 1, 3))
            f = np.zeros(m, dtype=bool)
            f[list(fx)] = True
            pos.append(r), delta.append(dl), par.append(p), counts.append(m), fixed.append(f), kinds.append(kind)
        self.kinds = kinds
        self.pos0 = np.concatenate(pos).astype(np.float32)
        self.delta, self.par = np.concatenate(delta), np.asarray(par, dtype=np.float64)
        self.gptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        self.batch = np.repeat(np.arange(len(counts)), counts)
        self.fixed = np.concatenate(fixed)
        self.n = int(self.gptr[-1])
        self.masses = np.concatenate([np.random.RandomState(900 + g).uniform(1.0, 16.0, W_GRAPHS[g][0]) for g in graphs]).astype(np.float32)
        free = ~self.fixed
        self.fptr = np.concatenate([[0], np.cumsum([free[a:b].sum() for a, b in zip(self.gptr[:-1], self.gptr[1:])])]).astype(np.int32)
        self.free_idx = np.nonzero(free)[0].astype(np.int32)
        self.dptr, self.moff = layout(self.fptr[1:] - self.fptr[:-1])

    def grad32(self, pos32):
        """dE/dpos fp32 of any number of copies of the batch, formed in fp64 from the fp32 positions, one rounding."""
        r = pos32.astype(np.float64).reshape(-1, self.n, 3)
        first = self.gptr[:-1][self.batch]
        h, kap, s, kt = (self.par[:, i] for i in range(4))
        x, y, z = (r[:, self.gptr[:-1], i] for i in range(3))
        q = y - s * (1.0 - x * x)
        dE = np.zeros_like(r)
        dE[:, self.gptr[:-1]] = np.stack([4.0 * h * x * (x * x - 1.0) + 4.0 * kap * q * s * x, 2.0 * kap * q, 2.0 * kap * z], -1)
        g = kt[self.batch][None, :, None] * (r - r[:, first] - self.delta[None])
        dE += g
        for k in range(r.shape[0]):
            np.subtract.at(dE[k], first, g[k])
        return dE.reshape(-1, 3).astype(np.float32)

    def hessian(self, i, weighted=True):
        """The closed form for graph i at pos0, restricted to the free atoms, divided by sqrt(m m') where `weighted`."""
        lo, hi = int(self.gptr[i]), int(self.gptr[i + 1])
        m = hi - lo
        h, kap, s, kt = self.par[i]
        x, y, z = self.pos0[lo].astype(np.float64)
        q = y - s * (1.0 - x * x)
        H = np.zeros((3 * m, 3 * m))
        H[0, 0] = 4.0 * h * (3.0 * x * x - 1.0) + 4.0 * kap * s * q + 8.0 * kap * s * s * x * x
        H[0, 1] = H[1, 0] = 4.0 * kap * s * x
        H[1, 1] = H[2, 2] = 2.0 * kap
        for a in range(1, m):
            for c in range(3):
                H[3 * a + c, 3 * a + c] += kt
                H[c, c] += kt
                H[3 * a + c, c] -= kt
                H[c, 3 * a + c] -= kt
        keep = np.repeat(~self.fixed[lo:hi], 3)
        H = H[keep][:, keep]
        if weighted:
            mw = np.repeat(self.masses[lo:hi][~self.fixed[lo:hi]].astype(np.float64), 3)
            H = H / np.sqrt(mw[:, None] * mw[None, :])
        return H

    def finite_differences(self, pairs=W_PAIRS, delta=W_DELTA):
        """(the packed Hessian by displace_ref, grad32 and rows_ref; the packed element bound).  The bound of element (u, v), row u
        the displaced coordinate, with D the realised separation of the two displaced positions, all over sqrt(m m'):
          1. truncation: the central difference of a cubic gradient is exact but for D^2 / 24 E_xxxx on the xx element of atom 0
             (the force is cubic in x and at most linear in everything else, so there are no higher terms and no others);
          2. rounding: each fp32 gradient is within 2^-24 relative of its value, so the difference carries at most
             (|dE+| + |dE-|) 2^-24 / D;
          3. midpoint: the two displaced positions are rounded to fp32, which moves their midpoint off x0 by at most ulp(x0) / 2,
             and the element by that times |dH_uv / du|: |E_xxx| on xx and |E_xxy| on xy of atom 0's row x, zero elsewhere."""
        key = ('fd', pairs, delta)
        if key in self.__dict__:
            return self.__dict__[key]
        total = int(self.moff[-1])
        H, R = np.full(total, np.nan), np.full(total, np.nan)
        f_max = int((self.fptr[1:] - self.fptr[:-1]).max())
        n = self.n
        for t in range((3 * f_max + pairs - 1) // pairs):
            pos = displace_ref(self.pos0, self.gptr, self.fptr, self.free_idx, pairs, t, delta)
            dE = self.grad32(pos)
            rows_ref(dE, self.pos0, self.masses, self.fptr, self.free_idx, self.moff, pairs, t, delta, H)
            mag = np.abs(dE).reshape(2 * pairs, n, 3)
            mag[1::2] *= -1.0                                      # (|dE+|) - (-|dE-|)
            rows_ref(mag.reshape(-1, 3), self.pos0, self.masses, self.fptr, self.free_idx, self.moff, pairs, t, delta, R)
        assert not np.isnan(H).any() and not np.isnan(R).any()
        B = R * 2.0 ** -24
        for i in range(len(self.gptr) - 1):
            a0 = int(self.gptr[i])
            assert not self.fixed[a0] and int(self.free_idx[self.fptr[i]]) == a0
            h, kap, s, _ = self.par[i]
            x0 = np.float64(self.pos0[a0, 0])
            D = np.float64(np.float32(x0 + delta)) - np.float64(np.float32(x0 - delta))
            half_ulp = 0.5 * np.float64(np.spacing(np.float32(abs(x0))))
            m0 = np.float64(self.masses[a0])
            lo = int(self.moff[i])
            B[lo] += (D * D / 24.0 * (24.0 * h + 24.0 * kap * s * s) + half_ulp * abs(24.0 * (h + kap * s * s) * x0)) / m0
            B[lo + 1] += half_ulp * abs(4.0 * kap * s) / m0
        self.__dict__[key] = (H, B)
        return H, B

    def torch_model(self):
        return _WellsModule(self)

    def data(self, dev):
        from pamnet_amd import synth
        return synth.Batch(pos=torch.from_numpy(self.pos0), batch=torch.from_numpy(self.batch), num_graphs=len(self.gptr) - 1).to(dev)


class _WellsModule(torch.nn.Module):
    """The analytic potential as a torch module over any number of copies of its batch (copy-major), in fp64 from the fp32
    positions, so that dE/dpos is the fp64 gradient rounded once.  Every graph gathers its atoms into W_SLOTS slots (an unused
    slot points at atom 0 and weighs 0) and adds their terms in slot order: elementwise launches only, so a graph's gradient is
    bitwise the same whatever else the batch holds."""

    def __init__(self, w):
        super().__init__()
        G = len(w.gptr) - 1
        idx, valid, delta = np.zeros((G, W_SLOTS), np.int64), np.zeros((G, W_SLOTS)), np.zeros((G, W_SLOTS, 3))
        for g in range(G):
            lo, hi = int(w.gptr[g]), int(w.gptr[g + 1])
            idx[g] = lo
            idx[g, :hi - lo] = np.arange(lo, hi)
            valid[g, 1:hi - lo] = 1.0
            delta[g, :hi - lo] = w.delta[lo:hi]
        self.n0, self.used = w.n, int(max(w.gptr[1:] - w.gptr[:-1]))
        for name, v in (('idx', idx), ('valid', valid), ('delta', delta), ('par', w.par)):
            self.register_buffer(name, torch.from_numpy(v))

    def forward(self, data):
        pos = data.pos.double()
        copies = pos.size(0) // self.n0
        shift = torch.arange(copies, device=pos.device) * self.n0
        r = pos[(self.idx[None] + shift[:, None, None]).reshape(-1, W_SLOTS)]
        h, kap, s, kt = self.par.repeat(copies, 1).unbind(1)
        valid, delta = self.valid.repeat(copies, 1), self.delta.repeat(copies, 1, 1)
        x, y, z = r[:, 0, 0], r[:, 0, 1], r[:, 0, 2]
        q = y - s * (1.0 - x * x)
        t = x * x - 1.0
        e = h * t * t + kap * q * q + kap * z * z
        for j in range(1, self.used):
            u = r[:, j] - r[:, 0] - delta[:, j]
            e = e + valid[:, j] * (0.5 * kt) * (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1] + u[:, 2] * u[:, 2])
        return e


def _wells(graphs=tuple(range(len(W_GRAPHS)))):
    key = ('wells',) + tuple(graphs)
    if key not in _MADE:
        _MADE[key] = _Wells(graphs)
    return _MADE[key]


# ------------------------------------------------------------------------------------------------- bookkeeping inputs
def _book():
    """Graphs of 0, 1, 2, 63, 64, 65, 2 and 64 atoms: a fifth of the atoms of the 63, the 65 and the second 64 fixed, the second graph
    of 2 all fixed; positions that include coordinates whose +- delta does not round symmetrically; masses in [1, 16]."""
    if 'book' in _MADE:
        return _MADE['book']
    c = Case()
    rng = np.random.RandomState(77)
    sizes = [0, 1, 2, 63, 64, 65, 2, 64]
    c.gptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    c.n = int(c.gptr[-1])
    c.pos0 = rng.uniform(-6.0, 6.0, (c.n, 3)).astype(np.float32)
    fixed = np.zeros(c.n, dtype=bool)
    for g in (3, 5, 7):
        lo, m = int(c.gptr[g]), sizes[g]
        fixed[lo + rng.choice(m, m // 5, replace=False)] = True
    fixed[c.gptr[6]:c.gptr[7]] = True
    c.fixed = fixed
    free = ~fixed
    c.fptr = np.concatenate([[0], np.cumsum([free[a:b].sum() for a, b in zip(c.gptr[:-1], c.gptr[1:])])]).astype(np.int32)
    c.free_idx = np.nonzero(free)[0].astype(np.int32)
    c.dptr, c.moff = layout(c.fptr[1:] - c.fptr[:-1])
    c.masses = rng.uniform(1.0, 16.0, c.n).astype(np.float32)
    c.delta = 0.01
    c.f_max = int((c.fptr[1:] - c.fptr[:-1]).max())
    _MADE['book'] = c
    return c


def _book_ts(c, pairs):
    last = (3 * c.f_max + pairs - 1) // pairs - 1
    return sorted({0, (3 + pairs - 1) // pairs, last // 2, last})     # first, past the end of the 1-atom graph, middle, last


# ---------------------------------------------------------------------------------------------------------- CPU tests
def test_header_declares_the_three_entry_points_at_abi_18():
    """(No GPU: the header and the built library.)"""
    import ctypes
    import re
    from pamnet_amd import build, lib
    decl = lib.declared_functions()
    P, D, I, I32 = ctypes.c_void_p, ctypes.c_double, ctypes.c_int64, ctypes.c_int32
    assert decl[ENTRIES[0]] == [P] * 4 + [I] * 4 + [D] + [P] * 2
    assert decl[ENTRIES[1]] == [P] * 6 + [I] * 4 + [D] + [P] * 2
    assert decl[ENTRIES[2]] == [P] * 7 + [I, D, I32, P]
    assert int(re.search(r'#define\s+PAMNET_ABI_VERSION\s+(\d+)', open(lib.HEADER).read()).group(1)) == 18
    h = ctypes.CDLL(build.build())
    assert h.pamnet_abi_version() == 18 and all(hasattr(h, name) for name in ENTRIES)


def test_vib_kernels_are_scratch_free(tmp_path):
    """(No GPU: hipcc cross-compiles.)  The compiler's report for csrc/vib.hip and csrc/eig.hip: no scratch in any kernel; the
    bookkeeping kernels use no LDS and fewer than 64 registers, the solver fewer than 128 and 8 KiB of LDS (DESIGN section 13
    quotes the figures)."""
    import os
    import re
    import shutil
    import subprocess
    from pamnet_amd import build
    hipcc = '/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else shutil.which('hipcc')
    assert hipcc, 'hipcc not available'
    limits = {'vib_displace_kernel': (64, 0), 'vib_rows_kernel': (64, 0), 'sym_eig_kernel': (128, 8192)}
    seen = set()
    for name in ('vib', 'eig'):
        r = subprocess.run([hipcc] + build.FLAGS + ['-c', os.path.join(build.CSRC, name + '.hip'), '-o', str(tmp_path / (name + '.o')),
                                                    '-Rpass-analysis=kernel-resource-usage'], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        for block in re.split(r'remark: Function Name: ', r.stderr)[1:]:
            kernel = [k for k in limits if k in block.split()[0]]
            assert len(kernel) == 1, block.split()[0]
            num = lambda key: int(re.search(key + r': (\d+)', block).group(1))
            assert num(r'ScratchSize \[bytes/lane\]') == 0, kernel
            regs, lds = limits[kernel[0]]
            assert num('VGPRs') + num('AGPRs') <= regs and num(r'LDS Size \[bytes/block\]') <= lds, (kernel, block)
            seen.add(kernel[0])
    assert seen == set(limits)


def test_the_schedule_covers_every_pair_once_per_sweep():
    """(No GPU.)  d = 1 .. 13, 63, 64, 65 and 192: the rounds of a sweep hold disjoint pairs and together every p < q < m once."""
    for d in list(range(1, 14)) + [63, 64, 65, 192]:
        m = d + (d & 1)
        seen = set()
        for rho in range(m - 1):
            pairs = round_pairs(m, rho)
            flat = [i for pq in pairs for i in pq]
            assert len(pairs) == m // 2 and sorted(flat) == list(range(m)), (d, rho)
            assert all(p < q for p, q in pairs)
            seen.update(pairs)
        assert seen == {(p, q) for p in range(m) for q in range(p + 1, m)}, d


@pytest.mark.parametrize('kind', KINDS)
def test_the_reference_solver_vs_eigvalsh(kind):
    """(No GPU; a test of the reference.)  jacobi_ref at tol = 1e-15 and 1e-14 on every dimension: the conditions the GPU test uses."""
    worst = [0.0, 0.0, 0.0, 0]
    for d in CPU_DIMS:
        for tol in (1e-15, 1e-14):
            w, v, sweeps, status = _reference(kind, d, tol)
            assert status == 0, (kind, d, tol, sweeps)
            e = _assert_solution(_matrix(kind, d), w, v, sweeps, (kind, d, tol))
            worst = [max(a, b) for a, b in zip(worst, e + (sweeps,))]
    print(kind, 'worst w / residual / orthogonality in d eps (|A|), sweeps:', worst)


def test_the_reference_solver_on_special_inputs():
    """(No GPU.)  A diagonal and a zero matrix take one sweep without a rotation; a non-finite entry is status 2; one sweep of a
    random matrix is status 1 with finite results; ties keep their diagonal order and the sign convention holds."""
    w, v, sweeps, status = jacobi_ref(np.diag([3.0, -1.0, 3.0, 0.5]))
    assert (sweeps, status) == (1, 0) and w.tolist() == [-1.0, 0.5, 3.0, 3.0]
    assert np.array_equal(v, np.eye(4)[[1, 3, 0, 2]])
    w, v, sweeps, status = jacobi_ref(np.zeros((5, 5)))
    assert (sweeps, status) == (1, 0) and not w.any() and np.array_equal(v, np.eye(5))
    assert jacobi_ref(_matrix('nan', 9))[3] == 2 and jacobi_ref(_matrix('inf', 9))[3] == 2
    w, v, sweeps, status = jacobi_ref(_matrix('random', 9), 1e-15, 1)
    assert (sweeps, status) == (1, 1) and np.isfinite(w).all() and np.isfinite(v).all()
    w, v, _, _ = jacobi_ref(np.array([[2.0, -1.0], [-1.0, 2.0]]))
    assert np.allclose(w, [1.0, 3.0], atol=1e-15) and np.allclose(v, np.array([[1.0, 1.0], [1.0, -1.0]]) / np.sqrt(2.0), atol=1e-15)


def test_the_bookkeeping_references_on_a_hand_made_case():
    """(No GPU; a test of the references.)  One graph of two free atoms, pairs = 2, delta = 0.01.  Atom 0 sits at x = 1: fl(1.01) - fl(0.99) in fp32 is not 0.02, and the divisor is that realised separation.  Job 0 displaces x of atom
    0, job 1 its y; evaluation 1 holds jobs 2 and 3 (z of atom 0, x of atom 1); evaluation 3 holds job 6, which does not exist."""
    pos0 = np.array([[1.0, 0.5, -2.0], [3.0, 0.25, 0.0]], np.float32)
    gptr, fptr, free_idx = [0, 2], [0, 2], [0, 1]
    _, moff = layout([2])
    out = displace_ref(pos0, gptr, fptr, free_idx, 2, 0, 0.01)
    want = np.tile(pos0, (4, 1))
    want[0, 0], want[2, 0] = np.float32(1.01), np.float32(0.99)
    want[4, 1], want[6, 1] = np.float32(0.51), np.float32(0.49)
    assert out.dtype == np.float32 and np.array_equal(out, want)
    out = displace_ref(pos0, gptr, fptr, free_idx, 2, 1, 0.01)
    want = np.tile(pos0, (4, 1))
    want[0, 2], want[2, 2] = np.float32(-1.99), np.float32(-2.01)
    want[5, 0], want[7, 0] = np.float32(3.01), np.float32(2.99)
    assert np.array_equal(out, want)
    assert np.array_equal(displace_ref(pos0, gptr, fptr, free_idx, 2, 3, 0.01), np.tile(pos0, (4, 1)))
    sep = float(np.float32(1.01)) - float(np.float32(0.99))
    assert sep != 0.02 and abs(sep - 0.02) < 1e-7
    assert job_of(fptr, free_idx, 0, 2, 1, 1) == (1, 0, 3) and job_of(fptr, free_idx, 0, 2, 3, 0) is None
    # dE of the four copies: only the rows the formula reads matter
    dpos = np.zeros((8, 3), np.float32)
    dpos[0], dpos[1] = [2.0, 4.0, 6.0], [8.0, 10.0, 12.0]          # copy 0 = + of pair 0
    dpos[2], dpos[3] = [1.0, 1.0, 1.0], [2.0, 2.0, 2.0]            # copy 1 = - of pair 0
    dpos[4], dpos[5] = [0.5, 0.0, 0.0], [0.0, 0.0, 3.0]            # copy 2 = + of pair 1
    dpos[6], dpos[7] = [0.0, 0.5, 0.0], [0.0, 0.0, 1.0]            # copy 3 = - of pair 1
    masses = np.array([4.0, 9.0], np.float32)
    h = np.full(36, SENTINEL)
    written = rows_ref(dpos, pos0, masses, fptr, free_idx, moff, 2, 0, 0.01, h)
    assert written == [(0, 0), (0, 1)]
    row0 = np.array([1.0, 3.0, 5.0, 6.0, 8.0, 10.0]) / sep / np.array([4.0, 4.0, 4.0, 6.0, 6.0, 6.0])
    sep_y = float(np.float32(0.51)) - float(np.float32(0.49))
    row1 = np.array([0.5, -0.5, 0.0, 0.0, 0.0, 2.0]) / sep_y / np.array([4.0, 4.0, 4.0, 6.0, 6.0, 6.0])
    assert np.allclose(h[:6], row0, rtol=4 * EPS, atol=0) and np.allclose(h[6:12], row1, rtol=4 * EPS, atol=0)
    assert (h[12:] == SENTINEL).all()
    h2 = np.full(36, SENTINEL)
    assert rows_ref(dpos, pos0, None, fptr, free_idx, moff, 2, 3, 0.01, h2) == [] and (h2 == SENTINEL).all()
    rows_ref(dpos, pos0, None, fptr, free_idx, moff, 2, 0, 0.01, h2)
    assert np.allclose(h2[:6], np.array([1.0, 3.0, 5.0, 6.0, 8.0, 10.0]) / sep, rtol=4 * EPS, atol=0)


def test_the_references_stay_inside_the_bound_on_the_analytic_potential():
    """(No GPU.)  The end-to-end bound on the references alone: displace_ref, the potential's fp32 gradient and rows_ref give every
    element of every mass-weighted Hessian within the bound of _Wells.finite_differences of the closed form -- at minima, at
    saddles and at general points; the closed form has no negative eigenvalue at a minimum and exactly one at a saddle, all of
    them further from zero than twice the Frobenius norm of the bound, so the count survives the finite differences."""
    w = _wells()
    assert sorted(set(int(b - a) for a, b in zip(w.gptr[:-1], w.gptr[1:]))) == [1, 2, 4, 22] and w.fixed.any()
    assert int((w.fptr[1:] - w.fptr[:-1]).max()) == 22 and set(w.kinds) == {'min', 'saddle', 'general'}
    H, B = w.finite_differences()
    for i in range(len(w.gptr) - 1):
        lo, hi = int(w.moff[i]), int(w.moff[i + 1])
        want = w.hessian(i).reshape(-1)
        err = np.abs(H[lo:hi] - want)
        print('graph', i, w.kinds[i], 'd', int(w.dptr[i + 1] - w.dptr[i]), 'worst error / bound', float((err / np.maximum(B[lo:hi], 1e-300)).max()),
              'largest bound', float(B[lo:hi].max()))
        assert (err <= B[lo:hi]).all(), (i, float((err / B[lo:hi]).max()))
        lam = np.linalg.eigvalsh(w.hessian(i))
        assert np.abs(lam).min() > 2 * np.sqrt((B[lo:hi] ** 2).sum()), (i, lam)     # (|E|_2 <= |E|_F <= |B|_F)
        if w.kinds[i] != 'general':
            assert int((lam < 0).sum()) == (1 if w.kinds[i] == 'saddle' else 0), (i, lam)
    # the truncation term is what the bound says, where it is the leading one
    i = 3
    lo = int(w.moff[i])
    h, kap, s, _ = w.par[i]
    trunc = W_DELTA ** 2 * 4.0 / 24.0 * (24.0 * h + 24.0 * kap * s * s) / float(w.masses[w.gptr[i]])
    assert abs((H[lo] - w.hessian(i)[0, 0]) - trunc) < 0.05 * trunc


def test_vib_refusals():
    """(No GPU.)  A PAMNet that keeps its positions in x, a delta that is not positive and finite, pairs < 1 and CPU tensors
    (RuntimeError: no CPU path) are refused before anything runs."""
    import models
    from pamnet_amd import synth, vib
    w = _wells((0, 1))
    model = w.torch_model()
    data = synth.Batch(pos=torch.from_numpy(w.pos0), batch=torch.from_numpy(w.batch), num_graphs=2)
    pdb = models.PAMNet(models.Config(dataset='PDBbind', dim=16, n_layer=1, cutoff_l=2.0, cutoff_g=6.0))
    with pytest.raises(ValueError, match=r'x\[:, :3\]'):
        vib.run(pdb, data)
    for bad in (0.0, -0.01, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='`delta` must be finite and positive'):
            vib.hessian(model, data, delta=bad)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match='`pairs`'):
            vib.hessian(model, data, pairs=bad)
    with pytest.raises(ValueError, match='`max_sweeps`'):
        vib.run(model, data, max_sweeps=0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        vib.run(model, data)
    assert torch.equal(data.pos, torch.from_numpy(w.pos0))


# ------------------------------------------------------------------------------------------------ bookkeeping launches
def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize('pairs', (1, 2, 5))
def test_displace_launch_is_the_reference_bit_for_bit(dev, pairs):
    """Graphs of 0, 1, 2, 63, 64 and 65 atoms, some with a fifth of their atoms fixed, one all fixed; the first, a middle and the
    last evaluation and the first one past the end of the 1-atom graph: pos_out equals displace_ref bit for bit, so idle copies,
    fixed rows and undisplaced coordinates are pos0."""
    from pamnet_amd import vib
    c = _book()
    pos0, gptr, fptr, free_idx = _t(c.pos0, dev), _t(c.gptr, dev), _t(c.fptr, dev), _t(c.free_idx, dev)
    for t in _book_ts(c, pairs):
        out = torch.full((2 * pairs * c.n, 3), SENTINEL, device=dev)
        vib.displace(pos0, gptr, fptr, free_idx, pairs, t, c.delta, out)
        want = displace_ref(c.pos0, c.gptr, c.fptr, c.free_idx, pairs, t, c.delta)
        got = out.cpu().numpy()
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (pairs, t)
        changed = (want != np.tile(c.pos0, (2 * pairs, 1))).sum()
        active = sum(job_of(c.fptr, c.free_idx, g, pairs, t, k) is not None for g in range(len(c.gptr) - 1) for k in range(pairs))
        assert changed == 2 * active and (t > 0 or active > 0), (pairs, t, changed, active)


@pytest.mark.gpu
@pytest.mark.parametrize('pairs', (1, 2, 5))
def test_rows_launch_vs_the_reference(dev, pairs):
    """The same batch with random fp32 dE/dpos, with and without masses: every stored element within 4 * 2^-52 relative of
    rows_ref; rows of idle pairs, other rows and a border around the matrices keep their sentinel."""
    from pamnet_amd import vib
    c = _book()
    rng = np.random.RandomState(5 + pairs)
    dpos = rng.standard_normal((2 * pairs * c.n, 3)).astype(np.float32)
    pad = 16
    moff = c.moff + pad
    pos0, fptr, free_idx, moff_d, dpos_d = _t(c.pos0, dev), _t(c.fptr, dev), _t(c.free_idx, dev), _t(moff, dev), _t(dpos, dev)
    worst = 0.0
    for masses in (None, c.masses):
        for t in _book_ts(c, pairs):
            h = torch.full((int(moff[-1]) + pad,), SENTINEL, dtype=torch.float64, device=dev)
            vib.hessian_rows(dpos_d, pos0, fptr, free_idx, moff_d, pairs, t, c.delta, h, None if masses is None else _t(masses, dev))
            want = np.full(int(moff[-1]) + pad, SENTINEL)
            written = rows_ref(dpos, c.pos0, masses, c.fptr, c.free_idx, moff, pairs, t, c.delta, want)
            got = h.cpu().numpy()
            stored = want != SENTINEL
            assert np.array_equal(got == SENTINEL, ~stored), (pairs, t)
            rel = np.abs(got[stored] - want[stored]) / np.abs(want[stored])
            worst = max(worst, float(rel.max()) if rel.size else 0.0)
            assert (rel <= 4 * EPS).all(), (pairs, t, float(rel.max()))
            assert t > 0 or len(written) > 0
    print('pairs', pairs, 'worst relative error in eps', worst / EPS)


@pytest.mark.gpu
def test_a_full_sweep_stores_every_element_once(dev):
    """pairs = 5 over all evaluations into a NaN-filled array: none left, and the whole array is rows_ref's."""
    from pamnet_amd import vib
    c = _book()
    pairs = 5
    rng = np.random.RandomState(3)
    dpos = rng.standard_normal((2 * pairs * c.n, 3)).astype(np.float32)
    pos0, fptr, free_idx, moff_d, dpos_d, masses = (_t(v, dev) for v in (c.pos0, c.fptr, c.free_idx, c.moff, dpos, c.masses))
    h = torch.full((int(c.moff[-1]),), float('nan'), dtype=torch.float64, device=dev)
    want = np.full(int(c.moff[-1]), np.nan)
    count = 0
    for t in range((3 * c.f_max + pairs - 1) // pairs):
        vib.hessian_rows(dpos_d, pos0, fptr, free_idx, moff_d, pairs, t, c.delta, h, masses)
        count += len(rows_ref(dpos, c.pos0, c.masses, c.fptr, c.free_idx, c.moff, pairs, t, c.delta, want))
    got = h.cpu().numpy()
    assert count == int(c.dptr[-1]) and not np.isnan(want).any() and not np.isnan(got).any()
    assert (np.abs(got - want) <= 4 * EPS * np.abs(want)).all()


# ------------------------------------------------------------------------------------------------------- eigensolver
def _pack(mats, pad=0):
    """(a packed with a sentinel border of `pad` elements, moff, dptr, the same for w) of a list of square matrices."""
    d = np.asarray([m.shape[0] for m in mats], dtype=np.int64)
    dptr = np.concatenate([[0], np.cumsum(d)]) + pad
    moff = np.concatenate([[0], np.cumsum(d * d)]) + pad
    a = np.full(int(moff[-1]) + pad, SENTINEL)
    for m, lo in zip(mats, moff[:-1]):
        a[lo:lo + m.size] = m.reshape(-1)
    return a, moff.astype(np.int64), dptr.astype(np.int64)


def _solve(dev, mats, pad=0, tol=1e-15, max_sweeps=30):
    """One launch -> per matrix (w, v, status, sweeps) as numpy, and the borders (a, v, w) for the sentinel checks."""
    from pamnet_amd import vib
    a, moff, dptr = _pack(mats, pad)
    a_d = _t(a, dev)
    v_d = torch.full_like(a_d, SENTINEL)
    w_d = torch.full((int(dptr[-1]) + pad,), SENTINEL, dtype=torch.float64, device=dev)
    st = torch.full((len(mats),), -9, dtype=torch.int32, device=dev)
    sw = torch.full((len(mats),), -9, dtype=torch.int32, device=dev)
    vib.eigh(a_d, _t(moff, dev), _t(dptr, dev), tol, max_sweeps, v=v_d, w=w_d, status=st, sweeps=sw)
    a_h, v_h, w_h, st, sw = a_d.cpu().numpy(), v_d.cpu().numpy(), w_d.cpu().numpy(), st.cpu().numpy(), sw.cpu().numpy()
    out = []
    for i, m in enumerate(mats):
        d = m.shape[0]
        out.append((w_h[dptr[i]:dptr[i] + d].copy(), v_h[moff[i]:moff[i] + d * d].reshape(d, d).copy(), int(st[i]), int(sw[i])))
    if pad:
        for arr, ends in ((a_h, moff), (v_h, moff), (w_h, dptr)):
            assert (arr[:pad] == SENTINEL).all() and (arr[ends[-1]:] == SENTINEL).all(), 'border'
    return out


def _same(x, y):
    return (np.array_equal(x[0], y[0], equal_nan=True) and np.array_equal(x[1], y[1], equal_nan=True) and x[2:] == y[2:])


@pytest.mark.gpu
def test_the_solver_on_one_batch_of_every_dimension_and_kind(dev):
    """d = 0, 1, 2, 3, 5, 6, 9, 63, 64, 65, 87, 96, 97 and 192 in one batch, rotating over the nine kinds (twice, shifted, so that
    every large dimension meets a finite kind): against eigvalsh and the symmetrised input -- the three conditions, w ascending,
    sweeps <= 20, the sign convention -- and against jacobi_ref on w; a zero and a diagonal matrix take one sweep; a NaN or an Inf
    is status 2 with NaN in w and v of that matrix only; a second launch, the reversed batch and every matrix alone give the
    same bits; a sentinel border around a, v and w is untouched."""
    for shift in (0, 4):
        kinds = [GPU_KINDS[(i + shift) % len(GPU_KINDS)] for i in range(len(GPU_DIMS))]
        mats = [_matrix(k, d) for k, d in zip(kinds, GPU_DIMS)]
        res = _solve(dev, mats, pad=32)
        worst = [0.0, 0.0, 0.0, 0.0, 0]
        for (w, v, status, sweeps), m, kind, d in zip(res, mats, kinds, GPU_DIMS):
            if d == 0:
                assert (status, sweeps) == (-9, -9)                # nothing is written
                continue
            if kind in ('nan', 'inf'):
                assert status == 2 and sweeps == 0 and np.isnan(w).all() and np.isnan(v).all(), (kind, d)
                continue
            assert status == 0 and np.isfinite(w).all() and np.isfinite(v).all(), (kind, d, status, sweeps)
            e = _assert_solution(m, w, v, sweeps, (kind, d))
            if kind in ('zero', 'diagonal'):
                assert sweeps == 1 and np.array_equal(w, np.sort(np.diag(m))), (kind, d)
            w_ref = _reference(kind, d)[0]
            s = (m + m.T) * 0.5
            norm = np.sqrt((s * s).sum())
            ej = np.abs(w - w_ref).max()
            assert ej <= 8 * d * EPS * norm, (kind, d, ej)
            worst = [max(a, b) for a, b in zip(worst, e + (ej / (d * EPS * norm) if norm else 0.0, sweeps))]
        print('shift', shift, 'worst w / residual / orthogonality / w vs jacobi_ref in d eps (|A|), sweeps:', worst)
        again = _solve(dev, mats, pad=32)
        assert all(_same(x, y) for x, y in zip(res, again)), 'a second launch'
        back = _solve(dev, mats[::-1])[::-1]
        assert all(_same(x, y) for x, y in zip(res, back)), 'the reversed batch'
        if shift == 0:
            for i, m in enumerate(mats):
                if m.shape[0]:
                    assert _same(_solve(dev, [m])[0], res[i]), ('alone', i)


@pytest.mark.gpu
def test_one_sweep_is_status_1_and_too_large_a_matrix_status_3(dev):
    """max_sweeps = 1 on random matrices: status 1, one sweep, finite results that are already ordered and orthonormal to rounding.
    A matrix of d = 193 between two others: status 3, its w and v keep their sentinels, its neighbours are solved as alone."""
    mats = [_matrix('random', 9), _matrix('random', 65)]
    for (w, v, status, sweeps), m in zip(_solve(dev, mats, pad=8, max_sweeps=1), mats):
        d = m.shape[0]
        assert (status, sweeps) == (1, 1) and np.isfinite(w).all() and np.isfinite(v).all() and (np.diff(w) >= 0).all()
        assert np.abs(v @ v.T - np.eye(d)).max() <= 8 * d * EPS
    big = np.random.RandomState(1).standard_normal((193, 193))
    mats = [_matrix('random', 9), big, _matrix('graded', 5)]
    res = _solve(dev, mats, pad=8)
    assert res[1][2] == 3 and (res[1][0] == SENTINEL).all() and (res[1][1] == SENTINEL).all()
    for i in (0, 2):
        assert res[i][2] == 0 and _same(res[i], _solve(dev, [mats[i]])[0])
        _assert_solution(mats[i], res[i][0], res[i][1], res[i][3], i)


@pytest.mark.gpu
def test_the_entry_points_validate_their_arguments(dev):
    """A null required pointer is PAMNET_ENULL, a bad count, delta, tol or max_sweeps PAMNET_EINVAL -- return codes only, nothing is
    launched; masses may be null; no graphs or matrices: nothing is written."""
    from pamnet_amd import lib
    c = _book()
    pairs = 2
    ten = dict(pos0=_t(c.pos0, dev), gptr=_t(c.gptr, dev), fptr=_t(c.fptr, dev), free_idx=_t(c.free_idx, dev), moff=_t(c.moff, dev),
               pos_out=torch.full((2 * pairs * c.n, 3), SENTINEL, device=dev), dpos=torch.zeros(2 * pairs * c.n, 3, device=dev),
               h=torch.full((int(c.moff[-1]),), SENTINEL, dtype=torch.float64, device=dev))
    stream = lib.stream_of(ten['pos0'])
    G = len(c.gptr) - 1

    def displace(**kw):
        a = dict({k: lib.ptr(v) for k, v in ten.items()}, n=c.n, G=G, pairs=pairs, t=0, delta=0.01)
        a.update(kw)
        lib.call(ENTRIES[0], a['pos0'], a['gptr'], a['fptr'], a['free_idx'], a['n'], a['G'], a['pairs'], a['t'], a['delta'],
                 a['pos_out'], stream)

    def rows(**kw):
        a = dict({k: lib.ptr(v) for k, v in ten.items()}, masses=None, n=c.n, G=G, pairs=pairs, t=0, delta=0.01)
        a.update(kw)
        lib.call(ENTRIES[1], a['dpos'], a['pos0'], a['masses'], a['fptr'], a['free_idx'], a['moff'], a['n'], a['G'], a['pairs'], a['t'],
                 a['delta'], a['h'], stream)

    bad = (dict(n=-1), dict(G=-1), dict(G=2 ** 31), dict(pairs=0), dict(pairs=32768), dict(t=-1), dict(delta=0.0), dict(delta=-1.0),
           dict(delta=float('nan')), dict(delta=float('inf')))
    for fn, names in ((displace, ('pos0', 'gptr', 'fptr', 'free_idx', 'pos_out')), (rows, ('dpos', 'pos0', 'fptr', 'free_idx', 'moff', 'h'))):
        for name in names:
            with pytest.raises(RuntimeError, match='PAMNET_ENULL'):
                fn(**{name: None})
        for kw in bad:
            with pytest.raises(RuntimeError, match='PAMNET_EINVAL'):
                fn(**kw)
        fn(G=0)
    torch.cuda.synchronize()
    assert (ten['pos_out'] == SENTINEL).all() and (ten['h'] == SENTINEL).all()

    a, moff, dptr = _pack([_matrix('random', 5)])
    e = dict(a=_t(a, dev), v=torch.full((25,), SENTINEL, dtype=torch.float64, device=dev),
             w=torch.full((5,), SENTINEL, dtype=torch.float64, device=dev), status=torch.zeros(1, dtype=torch.int32, device=dev),
             sweeps=torch.zeros(1, dtype=torch.int32, device=dev), moff=_t(moff, dev), dptr=_t(dptr, dev))

    def eig(**kw):
        p = dict({k: lib.ptr(v) for k, v in e.items()}, n_mat=1, tol=1e-15, max_sweeps=30)
        p.update(kw)
        lib.call(ENTRIES[2], p['a'], p['v'], p['w'], p['status'], p['sweeps'], p['moff'], p['dptr'], p['n_mat'], p['tol'],
                 p['max_sweeps'], stream)

    for name in e:
        with pytest.raises(RuntimeError, match='PAMNET_ENULL'):
            eig(**{name: None})
    for kw in (dict(n_mat=-1), dict(n_mat=2 ** 31), dict(tol=-1e-15), dict(tol=float('nan')), dict(max_sweeps=0), dict(max_sweeps=-3)):
        with pytest.raises(RuntimeError, match='PAMNET_EINVAL'):
            eig(**kw)
    eig(n_mat=0)
    torch.cuda.synchronize()
    assert (e['w'] == SENTINEL).all() and (e['v'] == SENTINEL).all()
    eig()
    assert int(e['status'][0]) == 0 and (e['w'] != SENTINEL).all()


# ----------------------------------------------------------------------------------------------------- end to end
@pytest.mark.gpu
def test_vib_run_on_the_analytic_potential(dev):
    """Graphs of 1, 2, 4 and 22 atoms at minima, saddles and general points in one batch, two of them with fixed atoms, masses in
    [1, 16], pairs = 3: every element of every Hessian inside the bound of _Wells.finite_differences; w within d times the largest
    element bound of eigvalsh of the closed form; n_negative 0 at the minima and 1 at the saddles; zero_point by its definition;
    asym, freq and the kept Hessian what they say; each graph alone, pairs = 1 and pairs = 7 give the same bits; and under the
    synchronisation debug mode the run warns once."""
    from pamnet_amd import vib
    w = _wells()
    model, data = w.torch_model().to(dev), w.data(dev)
    masses, fixed = _t(w.masses, dev), _t(w.fixed, dev)
    pos0 = data.pos.clone()
    res = vib.run(model, data, delta=W_DELTA, masses=masses, fixed=fixed, pairs=W_PAIRS)
    assert torch.equal(data.pos, pos0) and not data.pos.requires_grad
    assert res.fptr.tolist() == w.fptr.tolist() and res.free_idx.tolist() == w.free_idx.tolist()
    assert res.moff.tolist() == w.moff.tolist() and res.dptr.tolist() == w.dptr.tolist() and res.d_max == 66
    assert res.status.tolist() == [0] * len(w.graphs) and int(res.sweeps.max()) <= 20
    H, wv, modes = res.hessian.cpu().numpy(), res.w.cpu().numpy(), res.modes.cpu().numpy()
    _, B = w.finite_differences()
    neg, zp, asym = res.n_negative(0.0).tolist(), res.zero_point(hbar=2.0).cpu().numpy(), res.asym.cpu().numpy()
    for i in range(len(w.graphs)):
        lo, hi, d = int(w.moff[i]), int(w.moff[i + 1]), int(w.dptr[i + 1] - w.dptr[i])
        want = w.hessian(i)
        err = np.abs(H[lo:hi] - want.reshape(-1))
        print('graph', i, w.kinds[i], 'd', d, 'worst error / bound', float((err / np.maximum(B[lo:hi], 1e-300)).max()), 'asym', asym[i])
        assert (err <= B[lo:hi]).all(), (i, float((err / B[lo:hi]).max()))
        wi = wv[int(w.dptr[i]):int(w.dptr[i + 1])]
        assert np.abs(wi - np.linalg.eigvalsh(want)).max() <= d * B[lo:hi].max(), i
        Hi = H[lo:hi].reshape(d, d)
        _assert_solution(Hi, wi, modes[lo:hi].reshape(d, d), int(res.sweeps[i]), ('run', i))
        assert asym[i] == np.abs(Hi - Hi.T).max()
        if w.kinds[i] != 'general':
            assert neg[i] == (1 if w.kinds[i] == 'saddle' else 0), (i, wi[:3])
        assert neg[i] == int((wi < 0).sum())
        assert abs(zp[i] - 0.5 * 2.0 * np.sqrt(wi[wi > 0]).sum()) <= 1e-13 * max(zp[i], 1.0)
    assert np.array_equal(res.freq.cpu().numpy(), np.sign(wv) * np.sqrt(np.abs(wv)))
    assert res.n_negative(1e9).tolist() == [0] * len(w.graphs)
    # each graph alone: the same bits
    for i, g in enumerate(w.graphs):
        wg = _wells((g,))
        a0, a1 = int(w.gptr[i]), int(w.gptr[i + 1])
        rg = vib.run(wg.torch_model().to(dev), wg.data(dev), delta=W_DELTA, masses=masses[a0:a1].contiguous(),
                     fixed=fixed[a0:a1].contiguous(), pairs=W_PAIRS)
        lo, hi = int(w.moff[i]), int(w.moff[i + 1])
        assert torch.equal(rg.hessian, res.hessian[lo:hi]) and torch.equal(rg.modes, res.modes[lo:hi]), g
        assert torch.equal(rg.w, res.w[int(w.dptr[i]):int(w.dptr[i + 1])]) and torch.equal(rg.sweeps, res.sweeps[i:i + 1]), g
    # the grouping of jobs into evaluations does not matter
    for pairs in (1, 7):
        other = vib.hessian(model, data, delta=W_DELTA, masses=masses, fixed=fixed, pairs=pairs)
        assert torch.equal(other.hessian, res.hessian), pairs
    # synchronisation: one read at set-up, none in the loop, none for the solver
    try:
        torch.cuda.set_sync_debug_mode('warn')
    except Exception as e:                        # (a build without the debug mode: the rest of the test has run)
        print('set_sync_debug_mode is not available:', e)
        return
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter('always')
            vib.run(model, data, delta=W_DELTA, masses=masses, fixed=fixed, pairs=W_PAIRS)
        count = sum('synchronizing' in str(x.message) for x in rec)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert count == 1, count


def _pamnet_batch():
    """[a bond-free molecule of 5 atoms in open space (zero cell, pbc all False), 4 atoms in a triclinic cell below twice the global
    cutoff, the 10-atom slab slab_all of tests/test_pbc_axes.py with pbc = (True, True, False)] under cell_images='all', and the
    slab's bottom layer (the third of its atoms lowest along the open axis) as the fixed mask."""
    if 'pamnet' in _MADE:
        return _MADE['pamnet']
    from test_pbc_axes import Struct, _batch, _scatter, _structs
    rng = np.random.RandomState(9)
    zero, none = np.zeros((3, 3)), (False, False, False)
    tri_cell = [[4.75, 0.0, 0.0], [0.75, 4.5, 0.0], [-0.5, 0.625, 4.625]]
    mol = Struct(rng.randint(0, 5, 5).astype(np.float32),
                 _scatter(rng, 5, zero, none, {0: (0.0, 3.0), 1: (0.0, 3.0), 2: (0.0, 3.0)}, 0).astype(np.float32), zero, none, 0)
    tri = Struct(rng.randint(0, 5, 4).astype(np.float32), _scatter(rng, 4, tri_cell, (True, True, True), {}, 3).astype(np.float32),
                 tri_cell, (True, True, True), 3)
    slab = _structs()['slab_all']
    b = _batch([mol, tri, slab], cell_images='all')
    z = slab.pos[:, 2]
    fixed = np.zeros(b.pos.size(0), dtype=bool)
    fixed[mol.n + tri.n:] = z <= np.sort(z)[slab.n // 3 - 1]
    assert int(fixed.sum()) == slab.n // 3
    _MADE['pamnet'] = (b, torch.from_numpy(fixed))
    return _MADE['pamnet']


@pytest.mark.gpu
@pytest.mark.parametrize('dim,n_layer', MODELS)
def test_pamnet_hessian_replays_from_its_trace(dev, dim, n_layer):
    """PAMNet on {bond-free molecule, small triclinic cell, slab with a fixed bottom layer} under cell_images='all', pairs = 2,
    trace=True: the recorded positions of every evaluation equal displace_ref bit for bit; every row of the result replays from
    the recorded dE/dpos through rows_ref within 4 * 2^-52; asym is finite; data.pos is as it was.  (Random weights: neither the
    symmetry nor the curvature of the model is asserted.)"""
    import models
    from pamnet_amd import vib
    from test_pbc_axes import CUT_G, CUT_L
    b, fixed = _pamnet_batch()
    data = b.to(dev)
    torch.manual_seed(0)
    model = models.PAMNet(models.Config(dataset='QM9', dim=dim, n_layer=n_layer, cutoff_l=CUT_L, cutoff_g=CUT_G)).to(dev)
    masses = torch.from_numpy(np.random.RandomState(2).uniform(1.0, 16.0, b.pos.size(0)).astype(np.float32))
    pos0 = data.pos.clone()
    res = vib.run(model, data, delta=0.01, masses=masses.to(dev), fixed=fixed.to(dev), pairs=2, trace=True)
    assert torch.equal(data.pos, pos0) and not data.pos.requires_grad
    batch, fx = b.batch.numpy(), fixed.numpy()
    gptr = np.concatenate([[0], np.cumsum(np.bincount(batch, minlength=3))]).astype(np.int32)
    free = ~fx
    fptr = np.concatenate([[0], np.cumsum([free[a:c].sum() for a, c in zip(gptr[:-1], gptr[1:])])]).astype(np.int32)
    free_idx = np.nonzero(free)[0].astype(np.int32)
    dptr, moff = layout(fptr[1:] - fptr[:-1])
    assert res.fptr.tolist() == fptr.tolist() and res.free_idx.tolist() == free_idx.tolist() and res.moff.tolist() == moff.tolist()
    f_max = int((fptr[1:] - fptr[:-1]).max())
    assert len(res.trace) == (3 * f_max + 1) // 2
    want = np.full(int(moff[-1]), np.nan)
    for t, rec in enumerate(res.trace):
        pos = displace_ref(b.pos.numpy(), gptr, fptr, free_idx, 2, t, 0.01)
        assert np.array_equal(rec['pos'].cpu().numpy().view(np.int32), pos.view(np.int32)), t
        assert rec['energy'].numel() == 4 * 3
        rows_ref(rec['dE'].cpu().numpy(), b.pos.numpy(), masses.numpy(), fptr, free_idx, moff, 2, t, 0.01, want)
    got = res.hessian.cpu().numpy()
    assert not np.isnan(want).any() and np.isfinite(got).all() and np.abs(got).max() > 0
    assert (np.abs(got - want) <= 4 * EPS * np.abs(want)).all()
    assert torch.isfinite(res.asym).all() and res.status.tolist() == [0, 0, 0] and torch.isfinite(res.w).all()
    print('PAMNet', dim, n_layer, 'asym', res.asym.tolist(), 'lowest w', [float(res.w[int(dptr[i])]) for i in range(3)])


@pytest.mark.gpu
def test_vib_refusals_on_the_device(dev):
    """A non-QM9 schema, more than 64 free atoms, wrong dtype, shape or device of masses and fixed, masses that are not positive, a
    delta that is not positive and pairs < 1 raise ValueError before anything is evaluated."""
    import models
    from pamnet_amd import synth, vib
    w = _wells((0, 1, 2))
    model, data = w.torch_model().to(dev), w.data(dev)
    n = w.n
    pdb = models.PAMNet(models.Config(dataset='PDBbind', dim=16, n_layer=1, cutoff_l=2.0, cutoff_g=6.0)).to(dev)
    with pytest.raises(ValueError, match=r'x\[:, :3\]'):
        vib.run(pdb, data)
    crowd = synth.Batch(pos=torch.randn(70, 3, device=dev), batch=torch.cat([torch.zeros(65), torch.ones(5)]).long().to(dev), num_graphs=2)

    def never(d):
        raise AssertionError('the model must not be evaluated')

    with pytest.raises(ValueError, match='at most 64 free atoms'):
        vib.hessian(never, crowd)
    some = torch.zeros(70, dtype=torch.bool, device=dev)
    some[:2] = True
    with pytest.raises(AssertionError, match='the model must not be evaluated'):   # 63 free atoms: accepted, the loop starts
        vib.hessian(never, crowd, fixed=some)
    ok_m = torch.ones(n, device=dev)
    for kw, match in ((dict(masses=ok_m.double()), '`masses` is a float32'), (dict(masses=ok_m[:-1]), '`masses` is a float32'),
                      (dict(masses=ok_m.cpu()), '`masses` is a float32'), (dict(masses=[1.0] * n), '`masses` is a float32'),
                      (dict(masses=ok_m * 0), '`masses` must be positive'), (dict(masses=-ok_m), '`masses` must be positive'),
                      (dict(masses=ok_m * float('nan')), '`masses` must be positive'),
                      (dict(fixed=torch.zeros(n, dtype=torch.uint8, device=dev)), '`fixed` is a torch.bool'),
                      (dict(fixed=torch.zeros(n + 1, dtype=torch.bool, device=dev)), '`fixed` is a torch.bool'),
                      (dict(fixed=torch.zeros(n, dtype=torch.bool)), '`fixed` is a torch.bool'),
                      (dict(delta=0.0), '`delta` must be finite'), (dict(delta=-0.01), '`delta` must be finite'),
                      (dict(pairs=0), '`pairs`')):
        with pytest.raises(ValueError, match=match):
            vib.run(never, data, **kw)
    with pytest.raises(ValueError, match='`tol`'):
        vib.run(never, data, tol=-1.0)
