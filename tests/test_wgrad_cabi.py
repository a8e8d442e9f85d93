"""CPU-side checks of the weight-gradient entry points (csrc/wgrad.hip): the host-side slot planning and every refusal.
Nothing here launches a kernel: the planning calls only fill caller-owned host memory, and every other call is refused
before the library builds a batch, so the "device" addresses are made-up integers that are never dereferenced."""
import ctypes

import pytest

from pamnet_amd import build, lib

OK, EINVAL, ENULL = 0, -1, -2
MAXJ, MAXJ_S = 24, 16                      # jobs per stand-alone batch / per rider plan (csrc/wgrad_core.h)
SLOT_FLOATS = 128 * 128 + 2 * 128          # one partial tile with its two bias parts
BASE = 1 << 30                             # a made-up, 16-byte aligned device address


@pytest.fixture(scope='module')
def h():
    build.build()
    return lib.load()


def _nbytes(h, name):
    n = ctypes.c_int64(0)
    assert getattr(h, name)(ctypes.addressof(n)) == OK
    return int(n.value)


def _ctx(h):
    return (ctypes.c_char * _nbytes(h, 'pamnet_wgrad_ctx_bytes'))()        # zeroed


def _rider_mem(h):
    return (ctypes.c_char * _nbytes(h, 'pamnet_wgrad_rider_bytes'))()


def _job_arrays(rows):
    """The ten leading arguments of the batched / deferred / rider-plan entries for jobs of `rows` rows each."""
    n = len(rows)
    P, I64, I32 = ctypes.c_void_p * max(n, 1), ctypes.c_int64 * max(n, 1), ctypes.c_int32 * max(n, 1)
    fill = lambda v: [v] * n + [0] * (max(n, 1) - n)
    return [n, P(*fill(BASE)), I64(*fill(128)), P(*fill(BASE + 64)), I64(*fill(128)), I32(*fill(0)),
            I64(*(list(rows) + [0] * (max(n, 1) - n))), P(*fill(BASE + 128)), I64(*fill(128)), P(*fill(BASE + 192))]


def _plan(h, rows, max_slots, partial=BASE + 4096, rider=None, args=None):
    """pamnet_wgrad_rider_plan_f32 -> (rc, *slots_out (-7: not written), rider memory)."""
    rider = _rider_mem(h) if rider is None else rider
    out = ctypes.c_int64(-7)
    a = _job_arrays(rows) if args is None else args
    rc = h.pamnet_wgrad_rider_plan_f32(*a, partial, max_slots, ctypes.addressof(rider), ctypes.addressof(out))
    return rc, int(out.value), rider


def _documented_slots(rows, max_slots):
    """The rule of include/pamnet_hip.h, restated: 256 rows per slot, growing by 64 until the batch fits; every job takes at
    least one slot and at most 256."""
    chunk = 256
    while True:
        slots = sum(min(max(-(-r // chunk), 1), 256) for r in rows)
        if slots <= max_slots:
            return slots
        chunk += 64


RIDER_PLANS = [
    ([200000], 4),                 # the three plans that overran max_slots while the chunk stopped growing at 16 384 rows
    ([20000] * 10, 10),
    ([49152], 2),
    ([2816] * 10, 80),             # the engine's largest rider batch: fits at 256 + 64 k rows with room to spare
    ([2816] * 10, 10),
    ([0, 5], 2),
    ([300] * 16, 16),
    ([10 ** 7], 1),
    ([1], 1), ([256, 257], 3), ([256, 257], 2), ([100000], 256), ([100000], 300), ([16384 * 3 + 1] * 2, 7),
]


@pytest.mark.parametrize('rows,max_slots', RIDER_PLANS, ids=['%dx%d-%d' % (len(r), max(r), s) for r, s in RIDER_PLANS])
def test_rider_plan_stays_within_max_slots(h, rows, max_slots):
    rc, slots, _ = _plan(h, rows, max_slots)
    if rc != OK:
        assert rc == EINVAL and slots == -7
        pytest.fail('a plan with max_slots >= njobs exists (one slot per job) and was refused')
    assert len(rows) <= slots <= max_slots, (slots, max_slots)
    assert slots == _documented_slots(rows, max_slots)


def test_rider_plan_refusals(h):
    rc, slots, _ = _plan(h, [300] * (MAXJ_S + 1), 100)
    assert (rc, slots) == (EINVAL, -7)
    rc, slots, _ = _plan(h, [300] * MAXJ_S, 100)
    assert rc == OK and slots == 2 * MAXJ_S
    assert _plan(h, [], 4)[:2] == (EINVAL, -7)
    assert _plan(h, [5, 5, 5], 2)[:2] == (EINVAL, -7)              # max_slots < njobs
    for k in range(1, 10):                                         # each host array in turn
        a = _job_arrays([300, 40])
        a[k] = None
        assert _plan(h, [300, 40], 8, args=a)[:2] == (ENULL, -7), k
    for k in (1, 3, 7):                                            # a job without dZ / A / dW
        a = _job_arrays([300, 40])
        a[k][1] = None
        assert _plan(h, [300, 40], 8, args=a)[:2] == (ENULL, -7), k
    assert _plan(h, [300], 8, partial=None)[:2] == (ENULL, -7)
    a = _job_arrays([300])
    assert h.pamnet_wgrad_rider_plan_f32(*a, BASE, 8, None, None) == ENULL
    assert h.pamnet_wgrad_rider_plan_f32(*a, BASE, 8, ctypes.addressof(_rider_mem(h)), None) == OK     # slots_out is optional
    assert h.pamnet_wgrad_rider_bytes(None) == ENULL and h.pamnet_wgrad_ctx_bytes(None) == ENULL


def _tail(head=None, outs=(BASE, BASE, BASE), blocks=3):
    return [head, blocks, outs[0], outs[1], outs[2]]


def test_batched_and_deferred_refusals(h):
    ctx = _ctx(h)
    cx = ctypes.addressof(ctx)
    batched = lambda a, partial=BASE + 4096, tail=None: h.pamnet_wgrad_batched_f32(*a, partial, *(tail or _tail()), None)
    deferred = lambda a, partial=BASE + 4096, tail=None, tail2=None, c=cx: h.pamnet_wgrad_deferred_f32(
        *a, partial, *(tail or _tail()), *(tail2 or [None, None, None, None]), c, None)
    assert batched(_job_arrays([300] * (MAXJ + 1))) == EINVAL
    assert deferred(_job_arrays([300] * (MAXJ + 1))) == EINVAL
    assert deferred(_job_arrays([])) == EINVAL
    assert batched(_job_arrays([]), tail=_tail(head=BASE)) == EINVAL          # head vectors need a batch to ride with
    assert batched(_job_arrays([])) == OK                                     # nothing to do
    a = _job_arrays([300])
    a[0] = -1
    assert batched(a) == EINVAL and deferred(a) == EINVAL
    # a head partial with a null output, or a negative block count
    for k in range(3):
        outs = [BASE] * 3
        outs[k] = None
        assert batched(_job_arrays([300]), tail=_tail(BASE, outs)) == ENULL, k
        assert deferred(_job_arrays([300]), tail=_tail(BASE, outs)) == ENULL, k
        assert deferred(_job_arrays([300]), tail2=[BASE] + outs) == ENULL, k
    assert batched(_job_arrays([300]), tail=_tail(BASE, blocks=-1)) == ENULL
    assert deferred(_job_arrays([300]), tail=_tail(BASE, blocks=-1)) == ENULL
    # each required pointer in turn
    for k in range(1, 10):
        a = _job_arrays([300, 40])
        a[k] = None
        assert batched(a) == ENULL and deferred(a) == ENULL, k
    for k in (1, 3, 7):
        a = _job_arrays([300, 40])
        a[k][1] = None
        assert batched(a) == ENULL and deferred(a) == ENULL, k
    assert batched(_job_arrays([300]), partial=None) == ENULL
    assert deferred(_job_arrays([300]), partial=None) == ENULL
    assert deferred(_job_arrays([300]), c=None) == ENULL
    assert h.pamnet_wgrad_flush_f32(None, None) == ENULL
    assert bytes(ctx) == bytes(len(ctx))                                      # no refused call left anything pending


def test_deferred_refuses_the_scratch_of_a_pending_rider_batch(h):
    ctx = _ctx(h)
    part = BASE + (1 << 20)
    rc, slots, rider = _plan(h, [300, 40], 8, partial=part)
    assert rc == OK and slots == 3
    assert h.pamnet_wgrad_rider_enqueue_f32(ctypes.addressof(ctx), ctypes.addressof(rider)) == OK
    a = _job_arrays([300])
    rc = h.pamnet_wgrad_deferred_f32(*a, part, None, 0, None, None, None, None, None, None, None, ctypes.addressof(ctx), None)
    assert rc == EINVAL                                             # its slots are still waiting for their reduction


def test_rider_enqueue_refusals(h):
    ctx = _ctx(h)
    cx = ctypes.addressof(ctx)
    part = BASE + (1 << 20)
    _, s1, first = _plan(h, [300, 40, 1000], 80, partial=part)
    assert s1 == 2 + 1 + 4
    assert h.pamnet_wgrad_rider_enqueue_f32(None, ctypes.addressof(first)) == ENULL
    assert h.pamnet_wgrad_rider_enqueue_f32(cx, None) == ENULL
    assert h.pamnet_wgrad_rider_enqueue_f32(cx, ctypes.addressof(first)) == OK
    behind = part + 4 * s1 * SLOT_FLOATS
    for wrong in (part, behind + 4 * SLOT_FLOATS, behind - 4 * SLOT_FLOATS, behind + 4):
        _, _, second = _plan(h, [500], 80, partial=wrong)
        assert h.pamnet_wgrad_rider_enqueue_f32(cx, ctypes.addressof(second)) == EINVAL, wrong - part
    _, _, many = _plan(h, [10] * (MAXJ - 3 + 1), 80, partial=behind)          # 3 + 22 jobs > 24
    assert h.pamnet_wgrad_rider_enqueue_f32(cx, ctypes.addressof(many)) == EINVAL
    _, s2, second = _plan(h, [10] * (MAXJ_S - 1) + [700], 80, partial=behind)     # 3 + 16 jobs: appended
    assert h.pamnet_wgrad_rider_enqueue_f32(cx, ctypes.addressof(second)) == OK
    # the appended batch moved the end of the pending slots: a third rider must start behind BOTH
    _, _, third = _plan(h, [10] * 5, 80, partial=behind)
    assert h.pamnet_wgrad_rider_enqueue_f32(cx, ctypes.addressof(third)) == EINVAL
    _, _, third = _plan(h, [10] * 5, 80, partial=behind + 4 * s2 * SLOT_FLOATS)
    assert h.pamnet_wgrad_rider_enqueue_f32(cx, ctypes.addressof(third)) == OK    # 3 + 16 + 5 = 24 jobs
    _, _, fourth = _plan(h, [10], 80, partial=behind + 4 * (s2 + 5) * SLOT_FLOATS)
    assert h.pamnet_wgrad_rider_enqueue_f32(cx, ctypes.addressof(fourth)) == EINVAL


def test_edge_enqueue_refusals(h):
    ctx = _ctx(h)
    cx = ctypes.addressof(ctx)
    f = h.pamnet_wgrad_edge_enqueue_f32
    good = [cx, 9, BASE, 384, BASE + 64, BASE + 128, 128, BASE + 4096]
    for k in (0, 2, 5, 7):                                         # ctx, dW_e, dW_ea, partial (db may be null)
        a = list(good)
        a[k] = None
        assert f(*a) == ENULL, k
    for slots in (0, -1, 257):
        a = list(good)
        a[1] = slots
        assert f(*a) == EINVAL, slots
    assert bytes(ctx) == bytes(len(ctx))
    a = list(good)
    a[4] = None
    assert f(*a) == OK
    assert f(*good) == EINVAL                                      # one at a time: the next launch consumes it
    a = list(good)
    a[1] = 256
    assert f(*[ctypes.addressof(_ctx(h))] + a[1:]) == OK


@pytest.mark.parametrize('rows', [[0], [1], [128], [129], [10 ** 6], [300] * 24, [0, 1, 128, 129, 10 ** 6]],
                         ids=lambda v: 'x'.join(str(r) for r in sorted(set(v))) + '_%d' % len(v))
def test_scratch_floats(h, rows):
    """sum_j clamp(ceil(rows_j / 128), 1, 256) slots: the bound for any plan (no chunk is below 128 rows)."""
    n = ctypes.c_int64(-7)
    arr = (ctypes.c_int64 * len(rows))(*rows)
    assert h.pamnet_wgrad_scratch_floats(len(rows), arr, ctypes.addressof(n)) == OK
    assert n.value == sum(min(max(-(-r // 128), 1), 256) for r in rows) * (128 * 128 + 256)


def test_scratch_floats_refusals(h):
    n = ctypes.c_int64(-7)
    arr = (ctypes.c_int64 * 25)(*([5] * 25))
    f = h.pamnet_wgrad_scratch_floats
    assert f(25, arr, ctypes.addressof(n)) == EINVAL and f(-1, arr, ctypes.addressof(n)) == EINVAL
    assert f(3, None, ctypes.addressof(n)) == EINVAL and f(3, arr, None) == EINVAL
    assert n.value == -7
    assert f(0, None, ctypes.addressof(n)) == OK and n.value == 0
