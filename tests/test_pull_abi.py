"""CPU tests of the stream-ordered barrier / broadcast / fcollect interface:
the entry points and hooks reject bad arguments before touching HIP, the host
plan switches schedule exactly at the two-phase limit and at P == 2 and
`fused` exactly at the fused two-shot limit, the limit's setter, and the
counters before any call.  No GPU calls here: every call below returns from
its argument checks (a call that got past them would try to initialise a
device this suite does not have)."""
import ctypes

import pytest

EINVAL = 1
A, B = 1 << 20, 2 << 20     # two fake, well separated addresses: never dereferenced


def test_on_stream_calls_reject_bad_arguments_before_hip(shm):
    L = shm.lib()
    bar = L.shmemx_barrier_on_stream
    bad_sets = ((-1, 0, 2), (0, -1, 2), (0, 31, 2), (0, 0, 0), (0, 0, -3))
    for st in bad_sets:
        assert bar(*st, None) == EINVAL, st
        assert shm.last_error() == EINVAL
        for bits in (32, 64):
            bc = getattr(L, f"shmemx_broadcast{bits}_on_stream")
            fc = getattr(L, f"shmemx_fcollect{bits}_on_stream")
            assert bc(A, B, 8, 0, *st, None) == EINVAL, st
            assert fc(A, B, 8, *st, None) == EINVAL, st
            assert bc(A, B, 0, 0, *st, None) == EINVAL, st      # also with nothing to move
            assert fc(A, B, 0, *st, None) == EINVAL, st
    for bits in (32, 64):
        bc = getattr(L, f"shmemx_broadcast{bits}_on_stream")
        fc = getattr(L, f"shmemx_fcollect{bits}_on_stream")
        esize = bits // 8
        for root in (-1, 3, 16):
            assert bc(A, B, 8, root, 0, 0, 3, None) == EINVAL          # root outside 0..PE_size-1
            assert bc(A, B, 0, root, 0, 0, 3, None) == EINVAL
        assert bc(None, B, 8, 0, 0, 0, 3, None) == EINVAL              # NULL operands with elements
        assert bc(A, None, 8, 0, 0, 0, 3, None) == EINVAL
        assert fc(None, B, 8, 0, 0, 3, None) == EINVAL
        assert fc(A, None, 8, 0, 0, 3, None) == EINVAL
        # a partial overlap of target and source (in place is a legal broadcast)
        assert bc(A, A + esize, 8, 0, 0, 0, 3, None) == EINVAL
        assert bc(A + 7 * esize, A, 8, 0, 0, 0, 3, None) == EINVAL
        # fcollect: any overlap of [target, target + P nbytes) with the source
        assert fc(A, A, 8, 0, 0, 3, None) == EINVAL
        assert fc(A, A + 23 * esize, 8, 0, 0, 3, None) == EINVAL       # the last element of the target
        assert fc(A + 7 * esize, A, 8, 0, 0, 3, None) == EINVAL
        assert fc(A, B, 2 ** 62, 0, 0, 3, None) == EINVAL               # nelems * size wraps
        assert bc(A, B, 2 ** 62, 0, 0, 0, 3, None) == EINVAL
        assert shm.last_error() == EINVAL
    with pytest.raises(shm.ShmemError) as e:
        shm.barrier_on_stream(0, 0, 0)
    assert e.value.code == EINVAL
    with pytest.raises(shm.ShmemError) as e:
        shm.broadcast_on_stream(64, A, B, 8, 5, 0, 0, 3)
    assert e.value.code == EINVAL
    with pytest.raises(shm.ShmemError) as e:
        shm.fcollect_on_stream(32, A, A, 8, 0, 0, 3)
    assert e.value.code == EINVAL


def test_pull_loopback_argument_errors_without_a_device(shm):
    """shmemx_pull_loopback: EINVAL for a schedule outside 0..2, P outside
    1..16, m outside 0..P-1, a broadcast's root outside 0..P-1, an element
    size other than 4 or 8, and NULL arrays or a NULL entry when there are
    elements; nothing to do for zero elements."""
    fn = shm.lib().shmemx_pull_loopback
    good = (ctypes.c_void_p * 16)(*([64] * 16))
    hole = (ctypes.c_void_p * 16)(*([64] * 5 + [None] + [64] * 10))
    err = ctypes.c_uint(7)
    for schedule in (-1, 3):
        assert fn(schedule, 3, 0, 0, 8, good, good, 16, err, None) == EINVAL
    for schedule in (0, 1, 2):
        for P in (0, -1, 17):
            assert fn(schedule, P, 0, 0, 8, good, good, 16, err, None) == EINVAL
        for P, m in ((3, -1), (3, 3), (16, 16), (1, 1)):
            assert fn(schedule, P, m, 0, 8, good, good, 16, err, None) == EINVAL
        for esize in (0, 2, 16):
            assert fn(schedule, 3, 0, 0, esize, good, good, 16, err, None) == EINVAL
        assert fn(schedule, 3, 0, 0, 8, None, good, 16, err, None) == EINVAL
        assert fn(schedule, 3, 0, 0, 8, good, None, 16, err, None) == EINVAL
        assert fn(schedule, 6, 0, 0, 8, hole, good, 16, err, None) == EINVAL
        assert fn(schedule, 6, 2, 0, 4, good, hole, 16, err, None) == EINVAL
        assert shm.last_error() == EINVAL
        # zero elements: nothing to do, whatever the arrays
        assert fn(schedule, 3, 2, 0, 8, good, good, 0, err, None) == 0
        assert fn(schedule, 6, 0, 5, 4, hole, None, 0, None, None) == 0
        assert shm.last_error() == 0
    for schedule in (1, 2):
        for P, root in ((3, -1), (3, 3), (1, 1)):
            assert fn(schedule, P, 0, root, 8, good, good, 16, err, None) == EINVAL
    assert fn(0, 3, 0, 99, 8, good, good, 0, err, None) == 0     # an fcollect has no root
    assert err.value == 7        # never written before a launch
    with pytest.raises(shm.ShmemError) as e:
        shm.pull_loopback(2, [64, 64], [64, 0], 8, 8, m=1)
    assert e.value.code == EINVAL
    with pytest.raises(ValueError):
        shm.pull_loopback(0, [64, 64], [64], 8, 8)
    assert shm.pull_loopback(1, [64, 64], [64, 64], 0, 4) == 0


def test_pull_plan_argument_errors(shm):
    fn = shm.lib().shmemx_pull_plan
    p = shm.PullPlan()
    ok = (1, 8, 100, 4, 1, 0)
    assert fn(*ok, ctypes.byref(p)) == 0
    assert fn(*ok, None) == EINVAL
    for bad in ((-1, 8, 100, 4, 1, 0), (2, 8, 100, 4, 1, 0), (1, 2, 100, 4, 1, 0), (1, 16, 100, 4, 1, 0),
                (1, 8, 100, 0, 0, 0), (1, 8, 100, 17, 0, 0), (1, 8, 100, 4, -1, 0), (1, 8, 100, 4, 4, 0),
                (1, 8, 100, 4, 1, -1), (1, 8, 100, 4, 1, 4), (0, 8, 2 ** 62, 4, 1, 0)):
        assert fn(*bad, ctypes.byref(p)) == EINVAL, bad
    assert fn(0, 8, 100, 4, 1, 99, ctypes.byref(p)) == 0         # an fcollect has no root


@pytest.fixture
def limits(shm):
    """Known limits for the plan tests; the process's own put back after."""
    prev_two, prev_fused = shm.set_bcast_twophase_kb(64), shm.set_fused_twoshot_kb(1024)
    yield 64 << 10, 1024 << 10
    shm.set_bcast_twophase_kb(prev_two)
    shm.set_fused_twoshot_kb(prev_fused)


@pytest.mark.parametrize("esize", [4, 8])
def test_pull_plan_switches_schedule_at_the_threshold_and_at_two_members(shm, limits, esize):
    two, _ = limits
    at = two // esize                       # the largest one-phase array, in elements
    for P in (3, 4, 8, 16):
        for m in range(P):
            for root in (0, P - 1):
                assert shm.pull_plan("broadcast", esize, at, P, m, root).schedule == 1
                assert shm.pull_plan("broadcast", esize, at + 1, P, m, root).schedule == 2
    for n in (1, at, at + 1, 100 * at):
        for m in (0, 1):
            assert shm.pull_plan("broadcast", esize, n, 2, m, 0).schedule == 1     # P == 2: one link either way
    # nothing to launch: no elements, or one member
    assert shm.pull_plan("broadcast", esize, 0, 8, 3, 0).schedule == 0
    assert shm.pull_plan("broadcast", esize, at + 1, 1, 0, 0).schedule == 0
    assert shm.pull_plan("fcollect", esize, 0, 8, 3).schedule == 0
    assert shm.pull_plan("fcollect", esize, 100, 1, 0).schedule == 0
    # an fcollect has one phase at every size
    assert shm.pull_plan("fcollect", esize, 100 * at, 8, 3).schedule == 1
    # the limit at 0: two phases whenever there are three members
    prev = shm.set_bcast_twophase_kb(0)
    try:
        assert shm.pull_plan("broadcast", esize, 1, 3, 1, 0).schedule == 2
        assert shm.pull_plan("broadcast", esize, 1, 2, 1, 0).schedule == 1
    finally:
        shm.set_bcast_twophase_kb(prev)


@pytest.mark.parametrize("esize", [4, 8])
def test_pull_plan_switches_fused_at_the_fused_twoshot_limit(shm, limits, esize):
    _, fused = limits
    at = fused // esize
    for P in (2, 3, 8):
        assert shm.pull_plan("broadcast", esize, at, P, 1, 0).fused
        assert not shm.pull_plan("broadcast", esize, at + 1, P, 1, 0).fused
        # the root runs the same launches as the others
        assert shm.pull_plan("broadcast", esize, at, P, 0, 0).fused
        assert not shm.pull_plan("broadcast", esize, at + 1, P, 0, 0).fused
        # fcollect: the P-fold target counts
        assert shm.pull_plan("fcollect", esize, at // P, P, 1).fused
        assert not shm.pull_plan("fcollect", esize, at // P + 1, P, 1).fused
    prev = shm.set_fused_twoshot_kb(0)
    try:
        assert not shm.pull_plan("broadcast", esize, 1, 3, 1, 0).fused
        assert not shm.pull_plan("fcollect", esize, 1, 3, 1).fused
    finally:
        shm.set_fused_twoshot_kb(prev)


def test_pull_plan_segments_and_slices(shm, limits):
    """The plan's segment counts and slice: the slices of
    Slices(nelems, P - 1, esize) over the non-roots in set order."""
    two, _ = limits
    n, P, esize = two // 8 + 1001, 8, 8
    g = 2                                           # elements per 16-byte granule
    slice_ = -(-(-(-n // (P - 1))) // g) * g
    for root in (0, 3, 7):
        edge = 0
        for m in range(P):
            p = shm.pull_plan("broadcast", esize, n, P, m, root)
            assert p.schedule == 2
            if m == root:
                assert (p.nseg_a, p.nseg_b, p.lo, p.hi) == (0, 0, 0, 0)
                continue
            assert (p.nseg_a, p.nseg_b) == (1, P - 2)
            assert p.lo == edge and p.hi == min(n, edge + slice_)
            edge = p.hi
        assert edge == n
    # fewer elements than non-roots: empty slices pull nothing and are not gathered
    prev = shm.set_bcast_twophase_kb(0)
    try:
        plans = [shm.pull_plan("broadcast", 4, 5, 8, m, 7) for m in range(8)]
        assert [(p.lo, p.hi) for p in plans[:3]] == [(0, 4), (4, 5), (5, 5)]
        assert [p.nseg_a for p in plans] == [1, 1, 0, 0, 0, 0, 0, 0]
        assert [p.nseg_b for p in plans] == [1, 1, 2, 2, 2, 2, 2, 0]
    finally:
        shm.set_bcast_twophase_kb(prev)
    p = shm.pull_plan("broadcast", 8, 100, 8, 2, 5)
    assert (p.schedule, p.nseg_a, p.nseg_b, p.lo, p.hi) == (1, 1, 0, 0, 0)
    p = shm.pull_plan("fcollect", 4, 100, 8, 2)
    assert (p.schedule, p.nseg_a, p.nseg_b) == (1, 8, 0)


def test_bcast_twophase_limit_setter(shm):
    """shmemx_set_bcast_twophase_kb returns the previous limit (the derived
    2 MiB default unless $SHMEMX_BCAST_TWOPHASE_KB says otherwise) and refuses
    a negative one with -1 and EINVAL."""
    import os
    default = int(os.environ.get("SHMEMX_BCAST_TWOPHASE_KB", "2048"))
    prev = shm.set_bcast_twophase_kb(0)
    assert prev == default
    assert shm.set_bcast_twophase_kb(16384) == 0
    assert shm.lib().shmemx_set_bcast_twophase_kb(-1) == -1
    assert shm.last_error() == EINVAL
    with pytest.raises(shm.ShmemError):
        shm.set_bcast_twophase_kb(-5)
    assert shm.set_bcast_twophase_kb(prev) == 16384


def test_pull_stats_are_zero_before_any_call(shm):
    stats = shm.pull_stats()
    assert list(stats) == ["barriers", "broadcasts", "fcollects", "fused_calls", "twophase_broadcasts"]
    assert all(v == 0 for v in stats.values()), stats
    buf = (ctypes.c_ulonglong * 8)(*([9] * 8))
    assert shm.lib().shmemx_pull_stats(buf, 8, 0) == 5
    assert list(buf) == [0] * 5 + [9] * 3
    assert shm.lib().shmemx_pull_stats(buf, 2, 1) == 2
    assert shm.lib().shmemx_pull_stats(None, 5, 0) == 0
