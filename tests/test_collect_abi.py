"""CPU tests of the stream-ordered collect's interface: the new symbols are
exported and declared, every EINVAL path returns before any HIP call (a call
that got past its argument checks would try to initialise a device this suite
does not have), shmemx_collect_route switches exactly at the fused two-shot
limit, and the older counters keep their shape."""
import ctypes
import os
import re
import subprocess

import pytest

EINVAL = 1
A, B = 1 << 20, 2 << 20     # two fake, well separated addresses: never dereferenced
W = 3 << 20                 # a fake 8-byte aligned word
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
HEADER = os.path.join(REPO, "include", "shmem_reduce_mi355x.h")

SYMBOLS = ("shmemx_collect32_on_stream", "shmemx_collect64_on_stream", "shmemx_collect32_counted_on_stream",
           "shmemx_collect64_counted_on_stream", "shmemx_collect_stats", "shmemx_collect_route",
           "shmemx_collect_loopback")


def test_collect_symbols_are_exported_and_declared(shm):
    out = subprocess.run(["nm", "-D", "--defined-only", shm.LIB_PATH], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines() if line.strip()}
    header = open(HEADER).read()
    for name in SYMBOLS:
        assert name in exported, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert "has no stream-ordered form" not in header


def test_collect_on_stream_rejects_bad_arguments_before_hip(shm):
    L = shm.lib()
    bad_sets = ((-1, 0, 2), (0, -1, 2), (0, 31, 2), (0, 0, 0), (0, 0, -3))
    for bits in (32, 64):
        esize = bits // 8
        co = getattr(L, f"shmemx_collect{bits}_on_stream")
        cc = getattr(L, f"shmemx_collect{bits}_counted_on_stream")
        for st in bad_sets:
            assert co(A, B, 8, 64, *st, None) == EINVAL, st
            assert co(A, B, 0, 0, *st, None) == EINVAL, st          # also with nothing to move
            assert cc(A, B, W, None, 64, *st, None) == EINVAL, st
            assert cc(A, B, W, W + 16, 0, *st, None) == EINVAL, st
        # esize * capacity * 16 wraps
        assert co(A, B, 8, 2 ** 62, 0, 0, 3, None) == EINVAL
        assert co(A, B, 8, 2 ** 64 // (16 * esize) + 1, 0, 0, 3, None) == EINVAL
        assert cc(A, B, W, None, 2 ** 62, 0, 0, 3, None) == EINVAL
        # NULL operands with capacity > 0
        assert co(None, B, 8, 64, 0, 0, 3, None) == EINVAL
        assert co(A, None, 8, 64, 0, 0, 3, None) == EINVAL
        assert cc(None, B, W, None, 64, 0, 0, 3, None) == EINVAL
        assert cc(A, None, W, None, 64, 0, 0, 3, None) == EINVAL
        # the counted form with a NULL count, also with capacity 0; misaligned words
        assert cc(A, B, None, None, 64, 0, 0, 3, None) == EINVAL
        assert cc(A, B, None, W, 0, 0, 0, 3, None) == EINVAL
        assert cc(A, B, W + 4, None, 64, 0, 0, 3, None) == EINVAL
        assert cc(A, B, W, W + 20, 64, 0, 0, 3, None) == EINVAL
        # operands that are not whole elements
        assert co(A + 2, B, 8, 64, 0, 0, 3, None) == EINVAL
        assert co(A, B + esize // 2, 8, 64, 0, 0, 3, None) == EINVAL
        # a source that STARTS inside [target, target + capacity * esize)
        assert co(A, A, 8, 64, 0, 0, 3, None) == EINVAL
        assert co(A, A + 63 * esize, 1, 64, 0, 0, 3, None) == EINVAL      # the target's last element
        assert cc(A, A + esize, W, None, 64, 0, 0, 3, None) == EINVAL
        assert shm.last_error() == EINVAL
    with pytest.raises(shm.ShmemError) as e:
        shm.collect_on_stream(64, A, A + 8, 8, 64, 0, 0, 3)
    assert e.value.code == EINVAL
    with pytest.raises(shm.ShmemError) as e:
        shm.collect_counted_on_stream(32, A, B, None, None, 64, 0, 0, 3)
    assert e.value.code == EINVAL


def test_collect_loopback_argument_errors_without_a_device(shm):
    fn = shm.lib().shmemx_collect_loopback
    good = (ctypes.c_void_p * 16)(*([B] * 16))
    hole = (ctypes.c_void_p * 16)(*([B] * 5 + [None] + [B] * 10))
    odd = (ctypes.c_void_p * 16)(*([B] * 5 + [B + 2] + [B] * 10))
    inside = (ctypes.c_void_p * 16)(*([B] * 2 + [A + 8] + [B] * 13))
    counts = (ctypes.c_ulonglong * 16)(*([4] * 16))
    where = (ctypes.c_ulonglong * 2)(7, 7)
    over, err = ctypes.c_uint(7), ctypes.c_uint(7)
    tail = (where, over, err, None)
    for fused in (0, 1):
        for counted in (0, 1):
            for P in (0, -1, 17):
                assert fn(P, 0, 8, A, good, counts, 64, fused, counted, *tail) == EINVAL
            for P, m in ((3, -1), (3, 3), (16, 16), (1, 1)):
                assert fn(P, m, 8, A, good, counts, 64, fused, counted, *tail) == EINVAL
            for esize in (0, 2, 16):
                assert fn(3, 0, esize, A, good, counts, 64, fused, counted, *tail) == EINVAL
            assert fn(3, 0, 8, A, good, None, 64, fused, counted, *tail) == EINVAL
            assert fn(3, 0, 8, A, good, None, 0, fused, counted, *tail) == EINVAL
            assert fn(3, 0, 8, A, good, counts, 2 ** 62, fused, counted, *tail) == EINVAL
            assert fn(3, 0, 8, None, good, counts, 64, fused, counted, *tail) == EINVAL
            assert fn(3, 0, 8, A, None, counts, 64, fused, counted, *tail) == EINVAL
            assert fn(6, 0, 8, A, hole, counts, 64, fused, counted, *tail) == EINVAL
            assert fn(6, 0, 4, A, odd, counts, 64, fused, counted, *tail) == EINVAL
            assert fn(3, 0, 4, A + 2, good, counts, 64, fused, counted, *tail) == EINVAL
            assert fn(3, 2, 8, A, inside, counts, 64, fused, counted, *tail) == EINVAL   # srcs[m] inside the target
            assert shm.last_error() == EINVAL
            # no capacity: nothing to do, whatever the arrays
            assert fn(3, 2, 8, A, good, counts, 0, fused, counted, *tail) == 0
            assert fn(6, 0, 4, None, None, counts, 0, fused, counted, None, None, None, None) == 0
            assert shm.last_error() == 0
    assert (where[0], where[1], over.value, err.value) == (7, 7, 7, 7)      # never written before a launch
    with pytest.raises(shm.ShmemError) as e:
        shm.collect_loopback(A, [B, B], [4, 4], 64, 8, m=2)
    assert e.value.code == EINVAL
    with pytest.raises(ValueError):
        shm.collect_loopback(A, [B, B], [4], 64, 8)
    assert shm.collect_loopback(A, [B, B], [4, 4], 0, 4) == (0, 0, 0, 0)


def test_collect_route_switches_at_the_fused_twoshot_limit(shm):
    fn = shm.lib().shmemx_collect_route
    fused = ctypes.c_int(9)
    for bad in ((0, 64, 3), (2, 64, 3), (16, 64, 3), (8, 64, 0), (8, 64, 17), (8, 2 ** 62, 3)):
        assert fn(*bad, ctypes.byref(fused)) == EINVAL, bad
    assert fn(8, 64, 3, None) == EINVAL
    assert fused.value == 9
    prev = shm.set_fused_twoshot_kb(1024)
    try:
        limit = 1024 << 10
        for esize in (4, 8):
            at = limit // esize                 # the largest fused capacity, in elements
            for P in (1, 2, 3, 8, 16):          # the members' number does not move the limit
                assert shm.collect_route(esize, at - 1, P)          # one element (at least one byte) below
                assert shm.collect_route(esize, at, P)              # at the limit
                assert not shm.collect_route(esize, at + 1, P)      # above
                assert not shm.collect_route(esize, 0, P)           # nothing is launched
                assert shm.collect_route(esize, 1, P)
        assert shm.set_fused_twoshot_kb(64) == 1024
        assert shm.collect_route(8, 8192, 3) and not shm.collect_route(8, 8193, 3)
        assert shm.collect_route(4, 16384, 3) and not shm.collect_route(4, 16385, 3)
        shm.set_fused_twoshot_kb(0)
        assert not shm.collect_route(4, 1, 3)
    finally:
        shm.set_fused_twoshot_kb(prev)


def test_collect_stats_before_any_call_and_pull_stats_keep_their_keys(shm):
    stats = shm.collect_stats()
    assert list(stats) == ["collects", "fused_calls", "overflows"]
    assert all(v == 0 for v in stats.values()), stats
    buf = (ctypes.c_ulonglong * 6)(*([9] * 6))
    assert shm.lib().shmemx_collect_stats(buf, 6, 0) == 3
    assert list(buf) == [0] * 3 + [9] * 3
    assert shm.lib().shmemx_collect_stats(buf, 2, 1) == 2
    assert shm.lib().shmemx_collect_stats(None, 3, 0) == 0
    assert list(shm.pull_stats()) == ["barriers", "broadcasts", "fcollects", "fused_calls", "twophase_broadcasts"]
    buf = (ctypes.c_ulonglong * 8)(*([9] * 8))
    assert shm.lib().shmemx_pull_stats(buf, 8, 0) == 5
