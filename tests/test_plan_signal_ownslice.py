"""CPU tests of SIGNAL's own slice: the switch, the plan it changes, the
slot-size query and the argument checks of its loopback hook.  Host-side
logic only, no device.

With the switch on, `signal` plans the six own-order pairs (float, double and
long double min / max) above the one-shot limit as OWNSLICE plans them: a
slice per member and P - 1 result slots of one slice each.  Everything else,
and everything with the switch off, plans as before."""
import ctypes
import os

import pytest

OWN_PAIRS = [(t, o) for t in ("float", "double", "longdouble") for o in ("min", "max")]
LIMIT = int(os.environ.get("SHMEMX_DIRECT_ONESHOT_KB", "256")) << 10


def slice_of(n, P, sz):
    """set_geom.h Slices: ceil(n / P) rounded up to the 16-byte granule."""
    g = 1 if sz >= 16 else 16 // sz
    return -(-(-(-n // P)) // g) * g


@pytest.fixture
def switched_on(shm):
    prev = shm.set_signal_ownslice(True)
    yield
    shm.set_signal_ownslice(prev)


def test_setter_round_trip(shm):
    L = shm.lib()
    start = L.shmemx_set_signal_ownslice(1)
    assert start in (0, 1)
    assert L.shmemx_set_signal_ownslice(0) == 1
    assert L.shmemx_set_signal_ownslice(7) == 0          # any positive value is "on"
    assert L.shmemx_set_signal_ownslice(0) == 1
    # a negative value is refused: -1, EINVAL, the setting unchanged
    assert L.shmemx_set_signal_ownslice(-1) == -1 and shm.last_error() == 1
    assert L.shmemx_set_signal_ownslice(start) == 0
    assert shm.set_signal_ownslice(bool(start)) == bool(start)
    if "SHMEMX_SIGNAL_OWNSLICE" not in os.environ:
        assert start == 0                                # off by default
    assert len(shm.ALGOS) == 8 and "signal" in shm.ALGOS


def _cases():
    """(P, n in elements of `sz` bytes) above the one-shot limit, odd sizes."""
    for P in (2, 3, 8, 16):
        yield P, lambda sz: LIMIT // sz + 1
        yield P, lambda sz: 4 * (LIMIT // sz) + 70001


def test_signal_plans_a_slice_and_p_minus_1_slots(shm):
    plans_off = {}
    for t, o in OWN_PAIRS:
        sz = shm.type_size(t)
        for P, n_of in _cases():
            n = n_of(sz)
            for pe in sorted({0, P // 2, P - 1}):
                plans_off[t, o, P, n, pe] = shm.plan(t, o, n, 0, 0, P, pe, P, "signal")
    prev = shm.set_signal_ownslice(True)
    try:
        for (t, o, P, n, pe), off in plans_off.items():
            sz = shm.type_size(t)
            assert n * sz > LIMIT
            p = shm.plan(t, o, n, 0, 0, P, pe, P, "signal")
            assert p.algo == "signal" and p.member == pe and p.nmembers == P and p.elem_size == sz
            assert p.chunk == slice_of(n, P, sz)
            assert p.ws_bytes == (P - 1) * p.chunk * sz == shm.order_slots_bytes(t, P, n)
            assert (p.main, p.tail) == (off.main, off.tail)
            # today's plan: the whole array on every member, no workspace
            assert off.chunk == n and off.ws_bytes == 0
            # as OWNSLICE plans the same call
            q = shm.plan(t, o, n, 0, 0, P, pe, P, "ownslice")
            assert (q.chunk, q.ws_bytes) == (p.chunk, p.ws_bytes)
    finally:
        shm.set_signal_ownslice(prev)


def test_signal_plan_on_a_strided_set(shm, switched_on):
    for t, o in OWN_PAIRS:
        sz = shm.type_size(t)
        n = LIMIT // sz + 1
        p = shm.plan(t, o, n, 1, 1, 3, 3, 8, "signal")
        assert p.member == 1 and p.chunk == slice_of(n, 3, sz) and p.ws_bytes == 2 * p.chunk * sz


_EMPTY_SLICES = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import shmem_mi355x as shm
out = []
for t in ("float", "double", "longdouble"):
    for P in (2, 3, 8, 16):
        for n in (1, P - 1, 3 * P + 1):
            p = shm.plan(t, "min", n, 0, 0, P, P - 1, P, "signal")
            out.append([t, P, n, p.algo, p.chunk, p.ws_bytes])
print(json.dumps(out))
"""


def test_signal_plan_with_empty_slices(shm):
    """A one-shot limit of 0 and both variables from the environment, in a
    process of its own (the library reads them once): arrays of fewer
    elements than members, whose last slices are empty, plan a slice of one
    granule and P - 1 slots of it."""
    import json
    import subprocess
    import sys
    env = dict(os.environ, SHMEMX_DIRECT_ONESHOT_KB="0", SHMEMX_SIGNAL_OWNSLICE="1")
    out = subprocess.run([sys.executable, "-c", _EMPTY_SLICES, os.path.dirname(os.path.dirname(shm.__file__))],
                         env=env, check=True, capture_output=True, text=True).stdout
    rows = json.loads(out.strip().splitlines()[-1])
    assert len(rows) == 3 * 4 * 3
    empty = 0
    for t, P, n, algo, chunk, ws in rows:
        sz = shm.type_size(t)
        assert algo == "signal" and chunk == slice_of(n, P, sz) and ws == (P - 1) * chunk * sz, (t, P, n)
        empty += (P - 1) * chunk >= n                    # the last member owns nothing
    assert empty >= 3 * 4


def test_everything_else_plans_as_before(shm):
    calls = []
    for t, o in OWN_PAIRS:
        sz = shm.type_size(t)
        for n in (1, 1013, LIMIT // sz):                 # at or below the one-shot limit
            if n * sz <= LIMIT and n > 0:
                calls.append((t, o, n, 0, 0, 8, 3, 8, "signal"))
        calls.append((t, o, 4 * (LIMIT // sz) + 5, 2, 0, 1, 2, 8, "signal"))    # P = 1
        for algo in ("direct", "gather", "ownslice", "auto"):                    # other algorithms
            calls.append((t, o, 4 * (LIMIT // sz) + 5, 0, 0, 8, 3, 8, algo))
    for t, o in (("long", "xor"), ("float", "sum"), ("double", "prod"), ("int", "max"), ("complexd", "sum")):
        for n in (1013, 1 << 22):                        # other pairs
            calls.append((t, o, n, 0, 0, 8, 2, 8, "signal"))
    before = [shm.plan(*c) for c in calls]
    prev = shm.set_signal_ownslice(True)
    try:
        on = [shm.plan(*c) for c in calls]
    finally:
        shm.set_signal_ownslice(prev)
    assert on == before
    # and with the switch off again, the six pairs above the limit too
    big = [(t, o, 4 * (LIMIT // shm.type_size(t)) + 5, 0, 0, 8, 3, 8, "signal") for t, o in OWN_PAIRS]
    prev = shm.set_signal_ownslice(False)
    try:
        for c in big:
            p = shm.plan(*c)
            assert p.algo == "signal" and p.chunk == c[2] and p.ws_bytes == 0
    finally:
        shm.set_signal_ownslice(prev)


def test_order_slots_bytes_is_the_geometry_formula(shm):
    for t in ("float", "double", "longdouble", "short", "complexf"):
        sz = shm.type_size(t)
        for P in (1, 2, 3, 5, 8, 9, 16):
            for n in (0, 1, 2, P - 1, P, P + 1, 1013, 70001, 1 << 24):
                assert shm.order_slots_bytes(t, P, n) == (P - 1) * slice_of(n, P, sz) * sz, (t, P, n)
    L = shm.lib()
    assert L.shmemx_order_slots_bytes(99, 4, 100) == 0
    assert L.shmemx_order_slots_bytes(shm.TYPES["double"], 0, 100) == 0
    assert L.shmemx_order_slots_bytes(shm.TYPES["double"], 17, 100) == 0


def test_new_counters_are_appended(shm):
    st = shm.direct_stats(reset=False)
    assert st["signal_ownslice_calls"] == 0 and st["signal_ownslice_fused_calls"] == 0
    assert shm.DIRECT_STAT_INDEX["ownslice_calls"] == 13
    assert shm.DIRECT_STAT_INDEX["signal_ownslice_calls"] == 14
    assert shm.DIRECT_STAT_INDEX["signal_ownslice_fused_calls"] == 15
    buf = (ctypes.c_double * 14)(*([-1.0] * 14))
    assert shm.lib().shmemx_direct_stats(buf, 14, 0) == 14     # a caller with the old length still works


def test_orders_loopback_argument_errors_without_a_device(shm):
    """shmemx_fused_orders_loopback rejects bad arguments before any HIP call."""
    fn = shm.lib().shmemx_fused_orders_loopback
    T, O = shm.TYPES, shm.OPS
    D, MAX = T["double"], O["max"]
    A = 1 << 20                                                  # addresses never dereferenced
    good = (ctypes.c_void_p * 17)(*[A + 4096 * k for k in range(17)])
    hole = (ctypes.c_void_p * 3)(A, None, A + 8192)
    n = 64
    assert fn(D, MAX, 0, 0, good, good, good, n, None, None) == 1         # P < 1
    assert fn(D, MAX, 17, 0, good, good, good, n, None, None) == 1        # P > 16
    assert fn(D, MAX, 3, -1, good, good, good, n, None, None) == 1        # m outside 0..P-1
    assert fn(D, MAX, 3, 3, good, good, good, n, None, None) == 1
    assert fn(D, O["xor"], 3, 0, good, good, good, n, None, None) == 1    # not a reference pair
    assert fn(99, MAX, 3, 0, good, good, good, n, None, None) == 1
    assert fn(D, MAX, 3, 0, None, good, good, n, None, None) == 1         # NULL arrays
    assert fn(D, MAX, 3, 0, good, None, good, n, None, None) == 1
    assert fn(D, MAX, 3, 0, good, good, None, n, None, None) == 1
    assert fn(D, MAX, 3, 0, hole, good, good, n, None, None) == 1         # NULL entries
    assert fn(D, MAX, 3, 0, good, hole, good, n, None, None) == 1
    assert fn(D, MAX, 3, 0, good, good, hole, n, None, None) == 1
    assert shm.last_error() == 1
    assert fn(D, O["sum"], 3, 0, good, good, good, n, None, None) == 3    # ENOTSUP: not one of the six
    assert fn(T["int"], MAX, 3, 0, good, good, good, n, None, None) == 3
    assert fn(D, MAX, 3, 0, None, None, None, 0, None, None) == 0         # nothing to do
    assert shm.last_error() == 0
    with pytest.raises(ValueError):
        shm.fused_orders_loopback("double", "max", [A, A + 4096], [A], [A, A + 4096], 8)
    # the pinned errors of the existing hook are as they were
    old = shm.lib().shmemx_fused_loopback
    assert old(D, MAX, 3, 3, 0, 0, good, good, n, None, None) == 1
    assert old(D, MAX, 1, 3, 0, 1, good, good, n, None, None) == 1
