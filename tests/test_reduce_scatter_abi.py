"""CPU tests of the stream-ordered reduce-scatter's interface: the new symbols
are exported and declared, every EINVAL path returns before any HIP call (a
call that got past its argument checks would try to initialise a device this
suite does not have), shmemx_reduce_scatter_route switches exactly at the
fused two-shot limit on the SOURCE's bytes, and the older counters keep their
shape."""
import ctypes
import os
import re
import subprocess

import pytest

EINVAL = 1
A, B = 1 << 20, 2 << 20     # two fake, well separated addresses: never dereferenced
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
HEADER = os.path.join(REPO, "include", "shmem_reduce_mi355x.h")

SYMBOLS = ("shmemx_reduce_scatter_on_stream", "shmemx_reduce_scatter_route", "shmemx_reduce_scatter_stats",
           "shmemx_reduce_scatter_loopback")
ELEM_SIZE = {"short": 2, "int": 4, "long": 8, "longlong": 8, "float": 4, "double": 8,
             "longdouble": 16, "complexd": 16, "complexf": 8}


def test_reduce_scatter_symbols_are_exported_and_declared(shm):
    out = subprocess.run(["nm", "-D", "--defined-only", shm.LIB_PATH], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines() if line.strip()}
    header = open(HEADER).read()
    for name in SYMBOLS:
        assert name in exported, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    # the header says why there is no own-order answer
    assert "the\n * reference has no reduce-scatter" in header
    for name in ("reduce_scatter_on_stream", "reduce_scatter_route", "reduce_scatter_stats",
                 "reduce_scatter_loopback"):
        assert callable(getattr(shm, name))


def test_reduce_scatter_on_stream_rejects_bad_arguments_before_hip(shm):
    fn = shm.lib().shmemx_reduce_scatter_on_stream
    T, O = shm.TYPES, shm.OPS
    dsum = (T["double"], O["sum"])
    for st in ((-1, 0, 2), (0, -1, 2), (0, 31, 2), (0, 0, 0), (0, 0, -3)):
        assert fn(*dsum, A, B, 8, *st, None) == EINVAL, st
        assert fn(*dsum, A, B, 0, *st, None) == EINVAL, st              # also with nothing to move
    # pairs the reference lacks, unknown types and ops
    for t, o in (("float", "and"), ("double", "xor"), ("complexd", "min"), ("complexf", "max"), ("longdouble", "or")):
        assert not shm.lib().shmemx_op_valid(T[t], O[o])
        assert fn(T[t], O[o], A, B, 8, 0, 0, 3, None) == EINVAL, (t, o)
        assert fn(T[t], O[o], A, B, 0, 0, 0, 3, None) == EINVAL, (t, o)
    for t, o in ((-1, 0), (9, 0), (1, -1), (1, 7)):
        assert fn(t, o, A, B, 8, 0, 0, 3, None) == EINVAL, (t, o)
    for name, sz in ELEM_SIZE.items():
        pair = (T[name], O["sum"])
        # P * nelems * size * 16 wraps: the first nelems that does, and far past it
        edge = 2 ** 64 // (16 * sz * 3)
        assert fn(*pair, A, B, edge + 1, 0, 0, 3, None) == EINVAL, name
        assert fn(*pair, A, B, 2 ** 62, 0, 0, 3, None) == EINVAL, name
        assert fn(*pair, A, B, 2 ** 64 - 1, 0, 0, 1, None) == EINVAL, name
        # NULL operands with nelems > 0
        assert fn(*pair, None, B, 8, 0, 0, 3, None) == EINVAL, name
        assert fn(*pair, A, None, 8, 0, 0, 3, None) == EINVAL, name
        # operands that are not element-aligned
        assert fn(*pair, A + 1, B, 8, 0, 0, 3, None) == EINVAL, name
        assert fn(*pair, A, B + 1, 8, 0, 0, 3, None) == EINVAL, name
        if sz > 2:
            assert fn(*pair, A + min(sz, 8) // 2, B, 8, 0, 0, 3, None) == EINVAL, name
            assert fn(*pair, A, B + min(sz, 8) // 2, 8, 0, 0, 3, None) == EINVAL, name
        # any overlap of the target's nelems with the source's P * nelems
        # elements, at both ends of the source; there is no in-place form
        n, P = 8, 3
        S = P * n * sz
        assert fn(*pair, B, B, n, 0, 0, P, None) == EINVAL, name                    # the first block, in place
        assert fn(*pair, B + sz, B, n, 0, 0, P, None) == EINVAL, name
        assert fn(*pair, B - n * sz + sz, B, n, 0, 0, P, None) == EINVAL, name      # the target's last element
        assert fn(*pair, B + S - sz, B, n, 0, 0, P, None) == EINVAL, name           # the source's last element
        assert fn(*pair, B + 2 * n * sz, B, n, 0, 0, P, None) == EINVAL, name       # the last block, in place
        assert fn(*pair, B + n * sz, B, n, 0, 0, P, None) == EINVAL, name           # my own block (m = 1)
        assert shm.last_error() == EINVAL
    with pytest.raises(shm.ShmemError) as e:
        shm.reduce_scatter_on_stream("double", "sum", A, A + 8, 8, 0, 0, 3)
    assert e.value.code == EINVAL
    with pytest.raises(shm.ShmemError) as e:
        shm.reduce_scatter_on_stream("int", "max", A, B, 8, 0, 0, 0)
    assert e.value.code == EINVAL


def test_reduce_scatter_loopback_argument_errors_without_a_device(shm):
    fn = shm.lib().shmemx_reduce_scatter_loopback
    T, O = shm.TYPES, shm.OPS
    d, s = T["double"], O["sum"]
    good = (ctypes.c_void_p * 16)(*([B + k * (1 << 16) for k in range(16)]))
    hole = (ctypes.c_void_p * 16)(*([B] * 5 + [None] + [B] * 10))
    odd = (ctypes.c_void_p * 16)(*([B] * 5 + [B + 4] + [B] * 10))
    meets = (ctypes.c_void_p * 16)(*([B] * 2 + [A - 3 * 64 * 8 + 8] + [B] * 13))    # its last element is tgt's first
    err = ctypes.c_uint(7)
    for fused in (0, 1):
        for P in (0, -1, 17):
            assert fn(d, s, P, 0, A, good, 64, fused, err, None) == EINVAL
        for P, m in ((3, -1), (3, 3), (16, 16), (1, 1)):
            assert fn(d, s, P, m, A, good, 64, fused, err, None) == EINVAL
        assert fn(T["float"], O["xor"], 3, 0, A, good, 64, fused, err, None) == EINVAL
        assert fn(T["complexd"], O["max"], 3, 0, A, good, 0, fused, err, None) == EINVAL
        assert fn(d, s, 3, 0, A, good, 2 ** 62, fused, err, None) == EINVAL
        assert fn(d, s, 3, 0, None, good, 64, fused, err, None) == EINVAL
        assert fn(d, s, 3, 0, A, None, 64, fused, err, None) == EINVAL
        assert fn(d, s, 6, 0, A, hole, 64, fused, err, None) == EINVAL
        assert fn(d, s, 6, 0, A, odd, 64, fused, err, None) == EINVAL
        assert fn(d, s, 3, 0, A + 4, good, 64, fused, err, None) == EINVAL
        assert fn(d, s, 3, 0, A, meets, 64, fused, err, None) == EINVAL
        assert shm.last_error() == EINVAL
        # nothing to fold: nothing to do, whatever the arrays
        assert fn(d, s, 3, 2, A, good, 0, fused, err, None) == 0
        assert fn(d, s, 6, 0, None, None, 0, fused, None, None) == 0
        assert shm.last_error() == 0
    assert err.value == 7      # never written before a launch
    with pytest.raises(shm.ShmemError) as e:
        shm.reduce_scatter_loopback("double", "sum", A, [B, B], 64, m=2)
    assert e.value.code == EINVAL
    assert shm.reduce_scatter_loopback("double", "sum", A, [B, B], 0) == 0


def test_reduce_scatter_route_switches_at_the_fused_twoshot_limit(shm):
    fn = shm.lib().shmemx_reduce_scatter_route
    T = shm.TYPES
    fused = ctypes.c_int(9)
    for bad in ((-1, 64, 3), (9, 64, 3), (T["double"], 64, 0), (T["double"], 64, 17), (T["double"], 64, -1),
                (T["double"], 2 ** 62, 3), (T["short"], 2 ** 64 // (16 * 2 * 16) + 1, 16)):
        assert fn(*bad, ctypes.byref(fused)) == EINVAL, bad
    assert fn(T["double"], 64, 3, None) == EINVAL
    assert fused.value == 9
    prev = shm.set_fused_twoshot_kb(64)
    try:
        limit = 64 << 10                        # the SOURCE's bytes: P * nelems * size
        for name, sz in ELEM_SIZE.items():
            for P in (2, 4, 8, 16):             # 16: the most members a call takes
                at = limit // (P * sz)          # the largest fused nelems (P * sz divides the limit)
                assert at * P * sz == limit
                assert shm.reduce_scatter_route(name, at - 1, P), (name, P)         # one element below
                assert shm.reduce_scatter_route(name, at, P), (name, P)             # at the limit
                assert not shm.reduce_scatter_route(name, at + 1, P), (name, P)     # above
                assert not shm.reduce_scatter_route(name, 0, P)                     # nothing is launched
                assert shm.reduce_scatter_route(name, 1, P)
            # 3 members: 3 * sz does not divide the limit
            at = limit // (3 * sz)
            assert shm.reduce_scatter_route(name, at, 3) and not shm.reduce_scatter_route(name, at + 1, 3)
            # one member: a copy, no fused launch at any size
            for n in (0, 1, limit // sz, limit // sz + 1):
                assert not shm.reduce_scatter_route(name, n, 1)
        assert shm.reduce_scatter_route("double", 512, 16) and not shm.reduce_scatter_route("double", 513, 16)
        shm.set_fused_twoshot_kb(0)
        assert not shm.reduce_scatter_route("int", 1, 3)
    finally:
        shm.set_fused_twoshot_kb(prev)


def test_reduce_scatter_stats_before_any_call_and_the_older_stats_keep_their_keys(shm):
    stats = shm.reduce_scatter_stats()
    assert list(stats) == ["calls", "fused_calls"]
    assert all(v == 0 for v in stats.values()), stats
    buf = (ctypes.c_ulonglong * 5)(*([9] * 5))
    assert shm.lib().shmemx_reduce_scatter_stats(buf, 5, 0) == 2
    assert list(buf) == [0] * 2 + [9] * 3
    assert shm.lib().shmemx_reduce_scatter_stats(buf, 1, 1) == 1
    assert shm.lib().shmemx_reduce_scatter_stats(None, 2, 0) == 0
    assert shm.lib().shmemx_reduce_scatter_stats(buf, -1, 0) == 0
    assert list(shm.pull_stats()) == ["barriers", "broadcasts", "fcollects", "fused_calls", "twophase_broadcasts"]
    assert list(shm.collect_stats()) == ["collects", "fused_calls", "overflows"]
    assert list(shm.alltoall_stats()) == ["alltoalls", "alltoallvs", "fused_calls", "overflows"]
