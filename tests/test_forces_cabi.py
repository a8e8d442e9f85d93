"""CPU-side checks of the geometric backward entry points (forces): every one refuses a null pointer or a negative count
with PAMNET_EINVAL before it touches a device (no GPU in the build container)."""
import ctypes

import pytest

from pamnet_amd import build, lib

EINVAL = -1
_MEM = ctypes.create_string_buffer(64)     # a non-null address; never dereferenced (every call is refused first)


@pytest.fixture(scope='module')
def h():
    build.build()
    return lib.load()


def test_rbf_ddist_refuses_bad_arguments(h):
    b = ctypes.addressof(_MEM)
    f = h.pamnet_rbf_ddist_f32
    assert f(b, b, 5.0, -1, b, b, None) == EINVAL                      # negative count
    assert f(b, b, 0.0, 4, b, b, None) == EINVAL                       # cutoff
    for k in range(4):                                                 # each pointer in turn
        args = [b, b, b, b]
        args[k] = None
        assert f(args[0], args[1], 5.0, 4, args[2], args[3], None) == EINVAL, k


def test_sbf_bwd_refuses_bad_arguments(h):
    b = ctypes.addressof(_MEM)
    f = h.pamnet_sbf_bwd_f32
    ptrs = [b] * 9                       # gsbf, dist, idx, angle, tt_ptr, tt_perm, rad, dangle, ddist

    def call(p, n_edges=4, n_rows=6, cutoff=5.0):
        return f(p[0], p[1], cutoff, n_edges, p[2], p[3], n_rows, p[4], p[5], p[6], p[7], p[8], None)
    assert call(ptrs, n_edges=-1) == EINVAL
    assert call(ptrs, n_rows=-1) == EINVAL
    assert call(ptrs, cutoff=-1.0) == EINVAL
    assert call(ptrs, n_edges=0, n_rows=6) == EINVAL                  # rows gather edges: rows without edges
    for k in range(9):
        p = list(ptrs)
        p[k] = None
        assert call(p) == EINVAL, k


def test_pos_bwd_refuses_bad_arguments(h):
    b = ctypes.addressof(_MEM)
    f = h.pamnet_pos_bwd_f32
    # pos, g_ptr, g_row, g_col, gt_ptr, gt_perm, ddist_g | l_ptr, l_row, l_col, lt_ptr, lt_perm, ddist_l |
    # t_ptr, t_row, t_col, t_kind, tt_ptr, tt_perm, dangle | bond_work, dpos
    ptrs = [b] * 22

    def call(p, n=3, eg=4, el=2, tp=2):
        return f(p[0], n, p[1], p[2], p[3], p[4], p[5], p[6], eg, p[7], p[8], p[9], p[10], p[11], p[12], el,
                 p[13], p[14], p[15], p[16], p[17], p[18], p[19], tp, p[20], p[21], None)
    for bad in ({'n': -1}, {'eg': -1}, {'el': -1}, {'tp': -1}):
        assert call(ptrs, **bad) == EINVAL, bad
    for k in range(22):
        p = list(ptrs)
        p[k] = None
        assert call(p) == EINVAL, k
