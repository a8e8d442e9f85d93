"""CPU-side checks of the layer-stack engine's size queries (csrc/engine.hip, csrc/narrow_engine.hip): pamnet_stack_workspace,
pamnet_stack_layout and pamnet_stack_pack_floats.  Nothing here launches a kernel: the calls take sizes and write host
integers.  The figures pin the arena layout: both arenas of a step are carved by the walk that reports these sizes, and a
caller allocates exactly what is reported."""
import ctypes
import os
import subprocess
import sys

import pytest

from pamnet_amd import build, lib

OK, EINVAL, ENULL = 0, -1, -2
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def h():
    build.build()
    return lib.load()


def _workspace(h, n, eg, el, tp, n_layer, d=128):
    out = (ctypes.c_int64 * 2)(-7, -7)
    rc = h.pamnet_stack_workspace(n, eg, el, tp, n_layer, d, ctypes.addressof(out), ctypes.addressof(out) + 8)
    return rc, [int(out[0]), int(out[1])]


def _layout(h, n, eg, el, tp, d=128):
    out = (ctypes.c_int64 * 3)(-7, -7, -7)
    rc = h.pamnet_stack_layout(n, eg, el, tp, d, ctypes.addressof(out))
    return rc, [int(v) for v in out]


# (n, eg, el, tp, n_layer) -> workspace [saved, temp], layout [pair, global x_out, local x_out]; d = 128, default environment.
# The sizes lie on both sides of every bound of the launch plans: 2816 / 2817 nodes (riders), 4096 / 4097 (parked / lean
# chains), 131071 / 131072 global edges (the edge backward that forms its own weight gradients reserves its partial tiles).
D128 = [
    ((0, 0, 0, 0, 1), [0, 1597760], [0, 0, 0]),
    ((1, 0, 0, 0, 1), [5504, 1602432], [5504, 1792, 4544]),
    ((16, 30, 30, 90, 1), [143744, 1740672], [143744, 36352, 133184]),
    ((2816, 60000, 60000, 180000, 3), [433042560, 252003840], [144347520, 20406272, 142500032]),
    ((2817, 60000, 60000, 180000, 3), [433058688, 253339648], [144352896, 20408064, 142504512]),
    ((4096, 90000, 90000, 260000, 3), [636163584, 338362944], [212054528, 30380032, 209367296]),
    ((4097, 90000, 90000, 260000, 3), [636180096, 339698816], [212060032, 30381824, 209371840]),
    ((5176, 131071, 60000, 200000, 3), [545330688, 319581504], [181776896, 42829568, 178380928]),
    ((5176, 131072, 60000, 200000, 3), [545331456, 328103616], [181777152, 42829824, 178381184]),
    ((5176, 197750, 60000, 200000, 3), [596540160, 353707968], [198846720, 59899392, 195450752]),
    ((2304, 46000, 46000, 140000, 6), [672868608, 211828224], [112144768, 15904768, 110633152]),
]
NARROW = [
    (64, (2816, 60000, 60000, 180000, 3), [127094784, 63408512], [42364928, 1261568, 3424256]),
    (16, (2816, 60000, 60000, 180000, 3), [31773696, 13625408], [10591232, 315392, 856064]),
]


def _check_properties(sizes, d, ws, lay):
    n, n_layer = sizes[0], sizes[4]
    assert ws[0] == n_layer * lay[0]
    assert 0 <= lay[1] and lay[1] + n * d <= lay[2] and lay[2] + n * d <= lay[0]      # both node outputs lie inside a pair


@pytest.mark.parametrize('sizes,ws,lay', D128, ids=['-'.join(str(v) for v in c[0]) for c in D128])
def test_workspace_and_layout_d128(h, sizes, ws, lay):
    assert _workspace(h, *sizes) == (OK, ws)
    assert _layout(h, *sizes[:4]) == (OK, lay)
    _check_properties(sizes, 128, ws, lay)


@pytest.mark.parametrize('d,sizes,ws,lay', NARROW, ids=['d%d' % c[0] for c in NARROW])
def test_workspace_and_layout_narrow(h, d, sizes, ws, lay):
    assert _workspace(h, *sizes, d=d) == (OK, ws)
    assert _layout(h, *sizes[:4], d=d) == (OK, lay)
    _check_properties(sizes, d, ws, lay)


def test_pack_floats(h):
    for n_layer in (1, 3, 6):
        out = ctypes.c_int64(-7)
        assert h.pamnet_stack_pack_floats(n_layer, 128, ctypes.addressof(out)) == OK
        assert out.value == 884736 * n_layer
        assert h.pamnet_stack_pack_floats(n_layer, 64, ctypes.addressof(out)) == OK and out.value == 0   # packed inside `temp`


BIG = (5176, 197750, 60000, 200000, 3)
TINY = (16, 30, 30, 90, 1)
# environment -> sizes, workspace, layout (None: not pinned)
SWITCHED = [
    ({'PAMNET_EDGE_RECOMPUTE': '1'}, BIG, [448643328, 354370496], [149547776, 10600448, 146151808]),
    ({'PAMNET_EDGE_WGRAD': '0'}, BIG, [596540160, 345186240], None),
    ({'PAMNET_EDGE_WGRAD': '1'}, TINY, [143744, 1809280], None),
    ({'PAMNET_EDGE_WGRAD': '1', 'PAMNET_EDGE_RECOMPUTE': '1'}, TINY, [140160, 1811328], [140160, 32768, 129600]),
]
_CHILD = (
    "import sys, ctypes\n"
    "sys.path.insert(0, %r)\n"
    "from pamnet_amd import lib\n"
    "h = lib.load()\n"
    "s = [int(v) for v in sys.argv[1:]]\n"
    "w = (ctypes.c_int64 * 2)(); l = (ctypes.c_int64 * 3)()\n"
    "rw = h.pamnet_stack_workspace(*s, 128, ctypes.addressof(w), ctypes.addressof(w) + 8)\n"
    "rl = h.pamnet_stack_layout(*s[:4], 128, ctypes.addressof(l))\n"
    "print('SIZES', rw, rl, *w, *l)\n"
) % os.path.join(REPO, 'physics-aware-multiplex-gnn_amd')


@pytest.mark.parametrize('env,sizes,ws,lay', SWITCHED, ids=['+'.join('%s=%s' % (k[7:], v) for k, v in c[0].items()) for c in SWITCHED])
def test_switches_that_change_the_layout(h, env, sizes, ws, lay):
    """PAMNET_EDGE_WGRAD and PAMNET_EDGE_RECOMPUTE move slabs between the arenas.  Each setting in a process of its own:
    the switches are read once."""
    r = subprocess.run([sys.executable, '-c', _CHILD] + [str(v) for v in sizes], capture_output=True, text=True,
                       env=dict(os.environ, **env), timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [int(v) for v in [l for l in r.stdout.splitlines() if l.startswith('SIZES')][0].split()[1:]]
    assert got[:2] == [OK, OK]
    assert got[2:4] == ws
    if lay is not None:
        assert got[4:] == lay
    _check_properties(sizes, 128, got[2:4], got[4:])


def test_refusals(h):
    good = (16, 30, 30, 90, 1)
    for k in range(5):
        bad = list(good)
        bad[k] = -1
        for d in (128, 64):
            assert _workspace(h, *bad, d=d) == (EINVAL, [-7, -7]), (k, d)
        if k < 4:
            assert _layout(h, *bad[:4]) == (EINVAL, [-7, -7, -7]), k
    for d in (128, 64):
        assert _workspace(h, 16, 30, 30, 90, 0, d=d) == (EINVAL, [-7, -7])
    for d in (48, 0, 256):                                             # a width no engine is built for
        assert _workspace(h, *good, d=d) == (EINVAL, [-7, -7])
        assert _layout(h, *good[:4], d=d) == (EINVAL, [-7, -7, -7])
        assert h.pamnet_stack_pack_floats(1, d, ctypes.addressof(ctypes.c_int64())) == EINVAL
    # a null output: the d = 128 engine calls it a bad argument, the narrow one a missing pointer
    one = ctypes.c_int64(-7)
    a = ctypes.addressof(one)
    assert h.pamnet_stack_workspace(*good, 128, None, a) == EINVAL and h.pamnet_stack_workspace(*good, 128, a, None) == EINVAL
    assert h.pamnet_stack_workspace(*good, 64, None, a) == ENULL and h.pamnet_stack_workspace(*good, 64, a, None) == ENULL
    assert h.pamnet_stack_layout(*good[:4], 128, None) == EINVAL
    assert h.pamnet_stack_layout(*good[:4], 64, None) == ENULL
    assert h.pamnet_stack_pack_floats(1, 128, None) == EINVAL and h.pamnet_stack_pack_floats(1, 64, None) == EINVAL
    assert h.pamnet_stack_pack_floats(0, 128, a) == EINVAL and h.pamnet_stack_pack_floats(0, 64, a) == EINVAL
    assert one.value == -7
