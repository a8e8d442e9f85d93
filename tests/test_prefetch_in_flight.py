"""The chunked edge kernels hold the NEXT chunk's rows in registers across a barrier and a GEMM phase (csrc/edge_agg.hip:
global_edge_agg_fwd_kernel, global_edge_agg_bwd_kernel; csrc/edge_chain.hip: global_edge_fwd_kernel).  The requests clamp
the address of a row behind the range; the backward's leave the value alone (gemm_core.h ldg4c / ldg4cl) and the zero for
such a row is made where the row is used, the others zero it at the request.  What can go wrong is a use site without that
zero, or a chunk that takes over rows requested for another one, so the shapes here are the smallest at which a workgroup of
a saturated grid (256 workgroups) walks

  * several chunks and ends in a partial one        (E_g = 256 * 119 + 5: 48 + 48 + 23 rows backward, 112 + 7 forward),
  * several chunks and ends ON a chunk boundary     (uniform degrees: 2 x 48 rows backward, 2 x 112 rows forward),
  * one chunk with a ragged last tile               (E_g = 37),

about 14 edges per node, each against the fp64 torch formulation at the tolerances of test_hip_edge_agg.py (forward 2e-6,
backward 3e-6, max-normalised) and of test_hip_edge_chain.py (row kernel: max(2e-6, twice torch's own fp32 error)).
Poison: every row operand once more with a chunk of NaN rows behind the valid ones -- finite outputs, the bits of the
unpadded run.  The two forward forms (PAMNET_AGG_PP = 0 / 1) bit for bit; the backward overwriting and accumulating."""
import numpy as np
import pytest
import torch

from conftest import maxnorm_err

pytestmark = pytest.mark.gpu
D = 128
PAD = 112          # rows of poison behind every row operand: the longest chunk of the chunked kernels


def _near14(m, seed):
    """Degrees 8 .. 20 (about 14 per node) that sum to m."""
    rng = np.random.default_rng(seed)
    n = m // 14
    deg = 14 + rng.integers(-5, 6, size=n)
    d = m - int(deg.sum())
    deg[:abs(d)] += 1 if d > 0 else -1
    assert int(deg.sum()) == m and deg.min() >= 8 and deg.max() <= 20
    return deg


GRAPHS = {
    'partial_last_chunk': lambda: _near14(256 * 119 + 5, 1),
    'chunk_boundary_bwd': lambda: np.full(2048, 12),          # 96 rows per workgroup: two full 48-row chunks
    'chunk_boundary_fwd': lambda: np.full(4096, 14),          # 224 rows per workgroup: two full 112-row chunks
    'one_ragged_chunk': lambda: np.array([5, 0, 9, 3, 7, 13]),   # 37 rows on three workgroups
}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _padded(t):
    """The rows of t with PAD rows of NaN behind them (one allocation): the valid prefix."""
    buf = torch.full((t.size(0) + PAD, D), float('nan'), device=t.device)
    buf[:t.size(0)] = t
    return buf[:t.size(0)], buf


class _Case:
    """One graph: inputs, the fp64 results, and the kernels' results on exact-size operands (computed once, never modified)."""

    def __init__(self, dev, name):
        from pamnet_amd import lib
        self.lib, self.dev = lib, dev
        deg = np.asarray(GRAPHS[name](), dtype=np.int64)
        self.n, self.m = len(deg), int(deg.sum())
        rng = np.random.default_rng(5)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.int32).to(dev)
        self.ptr = t(np.concatenate([[0], np.cumsum(deg)]))
        self.row_of = t(np.repeat(np.arange(self.n), deg))
        self.col = t(rng.integers(0, self.n, size=self.m))
        gen = torch.Generator().manual_seed(11)
        mk = lambda *s: (0.5 * torch.randn(*s, generator=gen)).to(dev)
        self.e, self.z_in, self.ea_in, self.de0 = (mk(self.m, D) for _ in range(4))
        self.Pi, self.Pj, self.init, self.d_agg = (mk(self.n, D) for _ in range(4))
        self.Wm, self.bm, self.Wea = mk(D, 3 * D) / 4, mk(D) / 4, mk(D, D) / 4
        self.cuts = torch.full((257,), -1, dtype=torch.int32, device=dev)
        self.st = lib.stream_of(self.Pi)
        lib.call('pamnet_seg_cuts_i32', lib.ptr(self.ptr), lib.ptr(self.row_of), self.n, self.m, lib.ptr(self.cuts), None, self.st)
        dd = lambda x: x.double()
        ro, co = self.row_of.long(), self.col.long()
        We = self.Wm[:, 2 * D:]
        # forward, fp64
        z = dd(self.e) @ dd(We).t() + dd(self.bm) + dd(self.Pi)[ro] + dd(self.Pj)[co]
        ea = dd(self.e) @ dd(self.Wea).t()
        out = dd(self.init).clone().index_add_(0, ro, torch.nn.functional.silu(z) * ea)
        self.fwd64 = (out, z, ea)
        # backward on its own saves (z_in, ea_in), fp64
        dm = dd(self.d_agg)[ro]
        sg = torch.sigmoid(dd(self.z_in))
        dz = dm * dd(self.ea_in) * (sg * (1 + dd(self.z_in) * (1 - sg)))
        dea = dm * torch.nn.functional.silu(dd(self.z_in))
        d_e = dz @ dd(We) + dea @ dd(self.Wea)
        dPi = torch.zeros(self.n, D, dtype=torch.float64, device=dev).index_add_(0, ro, dz)
        self.bwd64 = {0: (dz, dea, d_e, dPi), 1: (dz, dea, d_e + dd(self.de0), dPi)}
        self.fwd = {pp: self.run_fwd(self.e, pp) for pp in ('0', '1')}
        self.bwd = {acc: self.run_bwd(self.z_in, self.ea_in, self.de0.clone(), acc) for acc in (0, 1)}

    def run_fwd(self, e, pp, cuts=True, entry='pamnet_global_edge_agg_fwd_f32'):
        import os
        lib, m, n = self.lib, self.m, self.n
        z, zbuf = _padded(torch.zeros(m, D, device=self.dev))
        ea, eabuf = _padded(torch.zeros(m, D, device=self.dev))
        z.fill_(float('nan')), ea.fill_(float('nan'))
        out = torch.full((n, D), float('nan'), device=self.dev)
        old = os.environ.get('PAMNET_AGG_PP')
        os.environ['PAMNET_AGG_PP'] = pp
        try:
            lib.call(entry, lib.ptr(e), m, n, self.Wm.data_ptr() + 8 * D, 3 * D, lib.ptr(self.bm), lib.ptr(self.Wea), D,
                     lib.ptr(self.Pi), lib.ptr(self.Pj), lib.ptr(self.ptr), lib.ptr(self.row_of), lib.ptr(self.col),
                     lib.ptr(self.cuts) if cuts else None, lib.ptr(self.init), lib.ptr(z), lib.ptr(ea), lib.ptr(out), self.st)
            torch.cuda.synchronize()
        finally:
            if old is None:
                del os.environ['PAMNET_AGG_PP']
            else:
                os.environ['PAMNET_AGG_PP'] = old
        assert torch.isnan(zbuf[m:]).all() and torch.isnan(eabuf[m:]).all()        # nothing written behind the rows
        return out, z, ea

    def run_bwd(self, z, ea, d_e, acc, cuts=True):
        """d_e: the tensor the kernel writes (acc = 0) or adds to (acc = 1); returned with the others."""
        lib, m, n = self.lib, self.m, self.n
        dz, dzbuf = _padded(torch.zeros(m, D, device=self.dev))
        dea, deabuf = _padded(torch.zeros(m, D, device=self.dev))
        dz.fill_(float('nan')), dea.fill_(float('nan'))
        if not acc:
            d_e.fill_(float('nan'))
        dPi = torch.full((n, D), float('nan'), device=self.dev)
        lib.call('pamnet_global_edge_agg_bwd_f32', lib.ptr(self.d_agg), m, n, lib.ptr(self.ptr), lib.ptr(self.row_of),
                 lib.ptr(self.cuts) if cuts else None, lib.ptr(z), lib.ptr(ea), self.Wm.data_ptr() + 8 * D, 3 * D, lib.ptr(self.Wea),
                 D, lib.ptr(dz), lib.ptr(dea), lib.ptr(d_e), acc, lib.ptr(dPi), self.st)
        torch.cuda.synchronize()
        assert torch.isnan(dzbuf[m:]).all() and torch.isnan(deabuf[m:]).all()
        return dz, dea, d_e, dPi


_CASES = {}


@pytest.fixture
def case(dev, request):
    name = request.param
    if name not in _CASES:
        _CASES[name] = _Case(dev, name)
    return _CASES[name]


ALL = pytest.mark.parametrize('case', sorted(GRAPHS), indirect=True)


@ALL
def test_chunked_forward_against_fp64(case):
    for got, want, what in zip(case.fwd['0'], case.fwd64, ('out', 'z', 'ea')):
        assert torch.isfinite(got).all(), what
        err = maxnorm_err(got.cpu(), want.cpu())
        print('forward %s: %.2e' % (what, err))
        assert err < 2e-6, (what, err)


@ALL
def test_forward_forms_agree_bit_for_bit(case):
    """PAMNET_AGG_PP = 1 (ping-pong stream) and = 0 (chunked) behind the same entry point, and the ping-pong entry point itself."""
    for a, b, what in zip(case.fwd['0'], case.fwd['1'], ('out', 'z', 'ea')):
        assert torch.equal(a, b), what
    for a, b, what in zip(case.fwd['0'], case.run_fwd(case.e, '0', entry='pamnet_global_edge_agg_fwd_pp_f32'), ('out', 'z', 'ea')):
        assert torch.equal(a, b), what


@ALL
@pytest.mark.parametrize('pp', ['0', '1'])
def test_forward_ignores_poison_behind_the_rows(case, pp):
    e, ebuf = _padded(case.e)
    for cuts in (True, False):              # the precomputed work split / the one every workgroup derives
        got = case.run_fwd(e, pp, cuts)
        for a, b, what in zip(got, case.fwd[pp], ('out', 'z', 'ea')):
            assert torch.isfinite(a).all(), what
            assert torch.equal(a, b), what


@ALL
@pytest.mark.parametrize('acc', [0, 1])
def test_backward_against_fp64(case, acc):
    for got, want, what in zip(case.bwd[acc], case.bwd64[acc], ('dz', 'dea', 'd_e', 'dPi')):
        assert torch.isfinite(got).all(), what
        err = maxnorm_err(got.cpu(), want.cpu())
        print('backward acc=%d %s: %.2e' % (acc, what, err))
        assert err < 3e-6, (what, err)


@ALL
@pytest.mark.parametrize('acc', [0, 1])
def test_backward_ignores_poison_behind_the_rows(case, acc):
    z, zbuf = _padded(case.z_in)
    ea, eabuf = _padded(case.ea_in)
    for cuts in (True, False):
        d_e, debuf = _padded(case.de0)
        got = case.run_bwd(z, ea, d_e, acc, cuts)
        assert torch.isnan(debuf[case.m:]).all()
        for a, b, what in zip(got, case.bwd[acc], ('dz', 'dea', 'd_e', 'dPi')):
            assert torch.isfinite(a).all(), what
            assert torch.equal(a, b), what


# ---- the row kernel on edge_chain.hip's plan: 256 workgroups, chunks of <= 8 tiles of 16 rows
ROW_CASES = {
    'two_chunks': 256 * 16 * 8 + 53,      # 9 tiles per workgroup, walked as 5 + 4; the last workgroup ends in a ragged tile
    'one_full_chunk': 256 * 16 * 8 - 11,  # 8 tiles per workgroup, one chunk
    'tiny': 37,
}


@pytest.mark.parametrize('name', sorted(ROW_CASES))
def test_row_kernel_forward(dev, name):
    from pamnet_amd import lib
    rows = ROW_CASES[name]
    n = max(rows // 14, 4)
    gen = torch.Generator().manual_seed(29)
    mk = lambda *s: (0.5 * torch.randn(*s, generator=gen)).to(dev)
    e, Pi, Pj = mk(rows, D), mk(n, D), mk(n, D)
    Wm, bm, Wea = mk(D, 3 * D) / 4, mk(D) / 4, mk(D, D) / 4
    row_of = torch.sort(torch.randint(0, n, (rows,), generator=gen))[0].to(torch.int32).to(dev)
    col = torch.randint(0, n, (rows,), generator=gen).to(torch.int32).to(dev)
    st = lib.stream_of(e)

    def f(e, We, bm, Wea, Pi, Pj):
        z = e @ We.t() + bm + Pi[row_of.long()] + Pj[col.long()]
        ea = e @ Wea.t()
        return z, ea, torch.nn.functional.silu(z) * ea

    args = (e, Wm[:, 2 * D:], bm, Wea, Pi, Pj)
    r64, r32 = f(*[a.double() for a in args]), f(*args)

    def run(e):
        outs = [_padded(torch.zeros(rows, D, device=dev)) for _ in range(3)]
        for o, _ in outs:
            o.fill_(float('nan'))
        lib.call('pamnet_global_edge_fwd_f32', lib.ptr(e), rows, Wm.data_ptr() + 8 * D, 3 * D, lib.ptr(bm), lib.ptr(Wea), D,
                 lib.ptr(Pi), lib.ptr(Pj), lib.ptr(row_of), lib.ptr(col), *[lib.ptr(o) for o, _ in outs], st)
        torch.cuda.synchronize()
        assert all(torch.isnan(b[rows:]).all() for _, b in outs)
        return [o for o, _ in outs]

    plain = run(e)
    for got, w64, w32, what in zip(plain, r64, r32, ('z', 'ea', 'msg')):
        assert torch.isfinite(got).all(), what
        err, floor = maxnorm_err(got.cpu(), w64.cpu()), maxnorm_err(w32.cpu(), w64.cpu())
        print('row kernel %s %s: %.2e (torch fp32: %.2e)' % (name, what, err, floor))
        assert err <= max(2e-6, 2 * floor), (what, err, floor)
    for a, b, what in zip(run(_padded(e)[0]), plain, ('z', 'ea', 'msg')):
        assert torch.isfinite(a).all() and torch.equal(a, b), what
