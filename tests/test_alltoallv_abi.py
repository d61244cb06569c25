"""CPU tests of the stream-ordered alltoall / alltoallv interface: the new
symbols are exported and declared, every EINVAL path returns before any HIP
call (a call that got past its argument checks would try to initialise a
device this suite does not have), shmemx_alltoallv_route switches exactly at
the fused two-shot limit, and the older counters keep their shape."""
import ctypes
import os
import re
import subprocess

import pytest

EINVAL = 1
T, S = 1 << 20, 2 << 20       # fake, well separated addresses: never dereferenced
C, O, W = 3 << 20, 4 << 20, 5 << 20   # fake 8-byte aligned tables and where words
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
HEADER = os.path.join(REPO, "include", "shmem_reduce_mi355x.h")

SYMBOLS = ("shmemx_alltoall32_on_stream", "shmemx_alltoall64_on_stream", "shmemx_alltoallv32_on_stream",
           "shmemx_alltoallv64_on_stream", "shmemx_alltoall_stats", "shmemx_alltoallv_route",
           "shmemx_alltoallv_loopback")
BAD_SETS = ((-1, 0, 2), (0, -1, 2), (0, 31, 2), (0, 0, 0), (0, 0, -3))


def test_alltoall_symbols_are_exported_and_declared(shm):
    out = subprocess.run(["nm", "-D", "--defined-only", shm.LIB_PATH], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines() if line.strip()}
    header = open(HEADER).read()
    for name in SYMBOLS:
        assert name in exported, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    # no blocking names: the reference's sample_sort.c defines its own shmem_alltoall32
    assert not any(re.match(r"shmem_alltoall", n) for n in exported)
    assert not re.search(r"\b(int|void)\s+shmem_alltoall", header)
    for fn in ("alltoall_on_stream", "alltoallv_on_stream", "alltoall_stats", "alltoallv_route", "alltoallv_loopback"):
        assert callable(getattr(shm, fn)), fn


def test_alltoall_on_stream_rejects_bad_arguments_before_hip(shm):
    L = shm.lib()
    for bits in (32, 64):
        esize = bits // 8
        a2a = getattr(L, f"shmemx_alltoall{bits}_on_stream")
        for st in BAD_SETS:
            assert a2a(T, S, 8, *st, None) == EINVAL, st
            assert a2a(T, S, 0, *st, None) == EINVAL, st            # also with nothing to move
        # PE_size * nelems * esize * 16 wraps
        assert a2a(T, S, 2 ** 62, 0, 0, 3, None) == EINVAL
        assert a2a(T, S, 2 ** 64 // (16 * esize * 3) + 1, 0, 0, 3, None) == EINVAL
        # NULL or not element-aligned operands
        assert a2a(None, S, 8, 0, 0, 3, None) == EINVAL
        assert a2a(T, None, 8, 0, 0, 3, None) == EINVAL
        assert a2a(T + 2, S, 8, 0, 0, 3, None) == EINVAL
        assert a2a(T, S + esize // 2, 8, 0, 0, 3, None) == EINVAL
        # any overlap of target and source, each 3 * 8 elements
        assert a2a(T, T, 8, 0, 0, 3, None) == EINVAL
        assert a2a(T, T + 23 * esize, 8, 0, 0, 3, None) == EINVAL      # the target's last element
        assert a2a(T + 23 * esize, T, 8, 0, 0, 3, None) == EINVAL      # the source's last element
        assert shm.last_error() == EINVAL
    with pytest.raises(shm.ShmemError) as e:
        shm.alltoall_on_stream(64, T, T + 8, 8, 0, 0, 3)
    assert e.value.code == EINVAL


def test_alltoallv_on_stream_rejects_bad_arguments_before_hip(shm):
    L = shm.lib()
    P, cap, scap = 3, 64, 48
    tb = P * 8
    for bits in (32, 64):
        esize = bits // 8
        v = getattr(L, f"shmemx_alltoallv{bits}_on_stream")
        for st in BAD_SETS:
            assert v(T, S, C, O, W, cap, scap, *st, None) == EINVAL, st
            assert v(T, S, C, O, None, 0, 0, *st, None) == EINVAL, st
        # capacity or src_capacity times esize * 16 wraps
        assert v(T, S, C, O, None, 2 ** 62, scap, 0, 0, P, None) == EINVAL
        assert v(T, S, C, O, None, cap, 2 ** 62, 0, 0, P, None) == EINVAL
        assert v(T, S, C, O, None, 2 ** 64 // (16 * esize) + 1, scap, 0, 0, P, None) == EINVAL
        assert v(T, S, C, O, None, cap, 2 ** 64 // (16 * esize) + 1, 0, 0, P, None) == EINVAL
        # NULL operands; the tables also with nothing to move
        assert v(None, S, C, O, None, cap, scap, 0, 0, P, None) == EINVAL
        assert v(T, None, C, O, None, cap, scap, 0, 0, P, None) == EINVAL
        assert v(T, S, None, O, None, cap, scap, 0, 0, P, None) == EINVAL
        assert v(T, S, C, None, None, cap, scap, 0, 0, P, None) == EINVAL
        assert v(T, S, None, None, None, 0, 0, 0, 0, P, None) == EINVAL
        # misaligned: whole elements, 8-byte tables and where words
        assert v(T + 2, S, C, O, None, cap, scap, 0, 0, P, None) == EINVAL
        assert v(T, S + esize // 2, C, O, None, cap, scap, 0, 0, P, None) == EINVAL
        assert v(T, S, C + 4, O, None, cap, scap, 0, 0, P, None) == EINVAL
        assert v(T, S, C, O + 4, None, cap, scap, 0, 0, P, None) == EINVAL
        assert v(T, S, C, O, W + 4, cap, scap, 0, 0, P, None) == EINVAL
        # target, source and the two tables pairwise disjoint: the six pairs, at their first and last bytes
        tend, send = T + cap * esize, T + scap * esize
        assert v(T, T + (cap - 1) * esize, C, O, None, cap, scap, 0, 0, P, None) == EINVAL      # target / source
        assert v(T + (scap - 1) * esize, T, C, O, None, cap, scap, 0, 0, P, None) == EINVAL
        assert v(T, S, tend - 8, O, None, cap, scap, 0, 0, P, None) == EINVAL                    # target / counts
        assert v(T, S, T - tb + 8, O, None, cap, scap, 0, 0, P, None) == EINVAL
        assert v(T, S, C, tend - 8, None, cap, scap, 0, 0, P, None) == EINVAL                    # target / offsets
        assert v(S, T, send - 8, O, None, cap, scap, 0, 0, P, None) == EINVAL                    # source / counts
        assert v(S, T, C, T - tb + 8, None, cap, scap, 0, 0, P, None) == EINVAL                  # source / offsets
        assert v(T, S, C, C, None, cap, scap, 0, 0, P, None) == EINVAL                           # counts / offsets
        assert v(T, S, C, C + tb - 8, None, cap, scap, 0, 0, P, None) == EINVAL
        assert v(T, S, C + tb - 8, C, None, cap, scap, 0, 0, P, None) == EINVAL
        assert shm.last_error() == EINVAL
    with pytest.raises(shm.ShmemError) as e:
        shm.alltoallv_on_stream(32, T, S, C, C, None, cap, scap, 0, 0, P)
    assert e.value.code == EINVAL


def test_alltoallv_loopback_argument_errors_without_a_device(shm):
    fn = shm.lib().shmemx_alltoallv_loopback
    good = (ctypes.c_void_p * 16)(*([S] * 16))
    hole = (ctypes.c_void_p * 16)(*([S] * 5 + [None] + [S] * 10))
    odd = (ctypes.c_void_p * 16)(*([S] * 5 + [S + 2] + [S] * 10))
    inside = (ctypes.c_void_p * 16)(*([S] * 2 + [T + 8] + [S] * 13))
    below = (ctypes.c_void_p * 16)(*([S] * 2 + [T - 8] + [S] * 13))     # its last element is the target's first
    counts = (ctypes.c_ulonglong * 256)(*([4] * 256))
    offs = (ctypes.c_ulonglong * 256)(*([0] * 256))
    where = (ctypes.c_ulonglong * 17)(*([7] * 17))
    over, err = ctypes.c_uint(7), ctypes.c_uint(7)
    tail = (where, over, err, None)
    for fused in (0, 1):
        for P in (0, -1, 17):
            assert fn(P, 0, 8, T, good, counts, offs, 64, 64, fused, *tail) == EINVAL
        for P, m in ((3, -1), (3, 3), (16, 16), (1, 1)):
            assert fn(P, m, 8, T, good, counts, offs, 64, 64, fused, *tail) == EINVAL
        for esize in (0, 2, 16):
            assert fn(3, 0, esize, T, good, counts, offs, 64, 64, fused, *tail) == EINVAL
        assert fn(3, 0, 8, T, good, counts, None, 64, 64, fused, *tail) == EINVAL       # counts without offsets
        assert fn(3, 0, 8, T, good, None, offs, 63, 63, fused, *tail) == EINVAL         # offsets without counts
        assert fn(3, 0, 8, T, good, None, None, 64, 64, fused, *tail) == EINVAL         # fixed: 64 is not 3 * nelems
        assert fn(3, 0, 8, T, good, counts, offs, 2 ** 62, 64, fused, *tail) == EINVAL
        assert fn(3, 0, 8, T, good, counts, offs, 64, 2 ** 62, fused, *tail) == EINVAL
        assert fn(3, 0, 8, None, good, counts, offs, 64, 64, fused, *tail) == EINVAL
        assert fn(3, 0, 8, T, None, counts, offs, 64, 64, fused, *tail) == EINVAL
        assert fn(6, 0, 8, T, hole, counts, offs, 64, 64, fused, *tail) == EINVAL
        assert fn(6, 0, 4, T, odd, counts, offs, 64, 64, fused, *tail) == EINVAL
        assert fn(3, 0, 4, T + 2, good, counts, offs, 64, 64, fused, *tail) == EINVAL
        assert fn(3, 0, 8, T, inside, counts, offs, 64, 64, fused, *tail) == EINVAL     # a peer's source in the target
        assert fn(3, 0, 8, T, below, counts, offs, 64, 2, fused, *tail) == EINVAL
        assert fn(3, 0, 8, T, inside, None, None, 63, 0, fused, *tail) == EINVAL
        assert shm.last_error() == EINVAL
        # nothing to move: nothing to do, whatever the arrays
        assert fn(3, 2, 8, T, good, counts, offs, 0, 64, fused, *tail) == 0
        assert fn(3, 2, 8, T, good, counts, offs, 64, 0, fused, *tail) == 0
        assert fn(6, 0, 4, None, None, None, None, 0, 0, fused, None, None, None, None) == 0
        assert shm.last_error() == 0
    assert list(where) == [7] * 17 and (over.value, err.value) == (7, 7)      # never written before a launch
    with pytest.raises(shm.ShmemError) as e:
        shm.alltoallv_loopback(T, [S, S], [[4, 4], [4, 4]], [[0, 4], [0, 4]], 64, 64, 8, m=2)
    assert e.value.code == EINVAL
    with pytest.raises(ValueError):
        shm.alltoallv_loopback(T, [S, S], [[4, 4]], [[0, 4], [0, 4]], 64, 64, 8)
    with pytest.raises(ValueError):
        shm.alltoallv_loopback(T, [S, S], [[4, 4], [4, 4]], None, 64, 64, 8)
    assert shm.alltoallv_loopback(T, [S, S], None, None, 0, 0, 4) == ([0, 0, 0], 0, 0)


def test_alltoallv_route_switches_at_the_fused_twoshot_limit(shm):
    fn = shm.lib().shmemx_alltoallv_route
    fused = ctypes.c_int(9)
    for bad in ((0, 64, 3), (2, 64, 3), (16, 64, 3), (8, 64, 0), (8, 64, 17), (8, 2 ** 62, 3)):
        assert fn(*bad, ctypes.byref(fused)) == EINVAL, bad
    assert fn(8, 64, 3, None) == EINVAL
    assert fused.value == 9
    prev = shm.set_fused_twoshot_kb(64)
    try:
        limit = 64 << 10
        for esize in (4, 8):
            at = limit // esize                 # the largest fused capacity, in elements
            for P in (1, 2, 3, 8, 16):          # the members' number does not move the limit
                assert shm.alltoallv_route(esize, at - 1, P)          # one element below
                assert shm.alltoallv_route(esize, at, P)              # at the limit
                assert not shm.alltoallv_route(esize, at + 1, P)      # one element above
                assert not shm.alltoallv_route(esize, 0, P)           # nothing is launched
                assert shm.alltoallv_route(esize, 1, P)
                assert shm.alltoallv_route(esize, at, P) == shm.collect_route(esize, at, P)
                assert shm.alltoallv_route(esize, at + 1, P) == shm.collect_route(esize, at + 1, P)
        assert shm.set_fused_twoshot_kb(1) == 64
        assert shm.alltoallv_route(8, 128, 3) and not shm.alltoallv_route(8, 129, 3)
        assert shm.alltoallv_route(4, 256, 3) and not shm.alltoallv_route(4, 257, 3)
        shm.set_fused_twoshot_kb(0)
        assert not shm.alltoallv_route(4, 1, 3)
    finally:
        shm.set_fused_twoshot_kb(prev)


def test_alltoall_stats_before_any_call_and_older_stats_keep_their_keys(shm):
    stats = shm.alltoall_stats()
    assert list(stats) == ["alltoalls", "alltoallvs", "fused_calls", "overflows"]
    assert all(v == 0 for v in stats.values()), stats
    buf = (ctypes.c_ulonglong * 6)(*([9] * 6))
    assert shm.lib().shmemx_alltoall_stats(buf, 6, 0) == 4
    assert list(buf) == [0] * 4 + [9] * 2
    assert shm.lib().shmemx_alltoall_stats(buf, 2, 1) == 2
    assert shm.lib().shmemx_alltoall_stats(None, 4, 0) == 0
    assert list(shm.collect_stats()) == ["collects", "fused_calls", "overflows"]
    assert list(shm.pull_stats()) == ["barriers", "broadcasts", "fcollects", "fused_calls", "twophase_broadcasts"]
