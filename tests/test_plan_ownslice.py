"""CPU tests of SHMEMX_ALGO_OWNSLICE's plan and of the P-order fold's
argument checks: host-side logic only, no device.

OWNSLICE is the two-shot schedule of the six own-order pairs (float, double
and long double min / max): a slice per member and P - 1 result slots of one
slice each above the one-shot limit, DIRECT's own-order one shot up to it,
and plain DIRECT for every other pair."""
import ctypes
import os

import pytest

OWN_PAIRS = [(t, o) for t in ("float", "double", "longdouble") for o in ("min", "max")]


def slice_of(n, P, sz):
    """set_geom.h Slices: ceil(n / P) rounded up to the 16-byte granule."""
    g = 1 if sz >= 16 else 16 // sz
    return -(-(-(-n // P)) // g) * g


def test_ownslice_plans_a_slice_and_p_minus_1_slots(shm):
    n, P = 1 << 20, 8
    limit = int(os.environ.get("SHMEMX_DIRECT_ONESHOT_KB", "256")) << 10
    assert n * 8 > limit
    for pe in range(P):
        p = shm.plan("double", "max", n, 0, 0, P, pe, P, "ownslice")
        assert p.algo == "ownslice" and p.member == pe and p.nmembers == P and p.elem_size == 8
        assert p.chunk == slice_of(n, P, 8) == n // P
        assert p.ws_bytes == 7 * p.chunk * 8 <= n * 8
    # against GATHER's n * P * sz in one piece
    assert shm.plan("double", "max", n, 0, 0, P, 0, P, "gather").ws_bytes == n * P * 8
    # an odd size: the slice is rounded up to whole 16-byte granules
    for t, o in OWN_PAIRS:
        sz = shm.type_size(t)
        m = 70001 * (16 // sz) * 4
        p = shm.plan(t, o, m, 1, 1, 3, 3, 8, "ownslice")
        assert p.algo == "ownslice" and p.member == 1
        assert p.chunk == slice_of(m, 3, sz) and p.ws_bytes == 2 * p.chunk * sz <= m * sz


def test_ownslice_small_arrays_take_the_one_shot(shm):
    p = shm.plan("double", "max", 1013, 0, 0, 8, 3, 8, "ownslice")
    assert p.algo == "ownslice" and p.chunk == 1013 and p.ws_bytes == 0


@pytest.mark.parametrize("t,op", [("long", "xor"), ("float", "sum")])
def test_ownslice_on_other_pairs_is_direct(shm, t, op):
    for n in (1013, 1 << 20):
        want = shm.plan(t, op, n, 0, 0, 8, 2, 8, "direct")
        assert want.algo == "direct"
        assert shm.plan(t, op, n, 0, 0, 8, 2, 8, "ownslice") == want
    # a one-member set too, own-order pair or not
    assert shm.plan("double", "max", 1 << 20, 2, 0, 1, 2, 8, "ownslice") == \
        shm.plan("double", "max", 1 << 20, 2, 0, 1, 2, 8, "direct")


def test_ownslice_limits(shm):
    with pytest.raises(shm.ShmemError) as e:
        shm.plan("double", "max", 1 << 20, 0, 0, 17, 0, 17, "ownslice")
    assert e.value.code == 3                                    # ENOTSUP: P > 16
    with pytest.raises(shm.ShmemError) as e:
        shm.plan("double", "max", 1 << 20, 0, 1, 4, 1, 8, "ownslice")
    assert e.value.code == 2                                    # ENOTMEMBER
    assert shm.plan("double", "max", 1 << 20, 0, 0, 16, 15, 16, "ownslice").algo == "ownslice"


def test_auto_does_not_choose_ownslice(shm):
    """auto keeps planning the six pairs as it did: GATHER."""
    for t, o in OWN_PAIRS:
        for n in (1013, 1 << 20):
            a = shm.plan(t, o, n, 0, 0, 8, 1, 8, "auto")
            assert a.algo == shm.plan(t, o, n, 0, 0, 8, 1, 8, "gather").algo == "gather"
    assert shm.ALGOS["ownslice"] == 7 and len(set(shm.ALGOS.values())) == len(shm.ALGOS) == 8
    assert shm.DIRECT_COUNTS[-1] == "ownslice_calls"
    st = shm.direct_stats(reset=False)
    assert st["ownslice_calls"] == 0


def test_fold_orders_argument_errors_without_a_device(shm):
    """shmemx_fold_orders_on_stream rejects bad arguments before touching
    HIP: EINVAL for nins outside 1..16, a NULL entry, a pair the reference
    lacks or an output overlapping anything but its own input exactly;
    ENOTSUP for a reference pair outside the six; nothing to do for zero
    elements."""
    fn = shm.lib().shmemx_fold_orders_on_stream
    T, O = shm.TYPES, shm.OPS
    D, MAX = T["double"], O["max"]
    A = 1 << 20                                                  # addresses never dereferenced
    good_in = (ctypes.c_void_p * 17)(*[A + 4096 * k for k in range(17)])
    good_out = (ctypes.c_void_p * 17)(*[16 * A + 4096 * k for k in range(17)])
    n = 16
    assert fn(D, MAX, good_out, good_in, 0, n, None) == 1        # nins < 1
    assert fn(D, MAX, good_out, good_in, 17, n, None) == 1       # nins > 16
    assert fn(D, MAX, good_out, good_in, -1, n, None) == 1
    hole = (ctypes.c_void_p * 3)(A, None, A + 8192)
    assert fn(D, MAX, good_out, hole, 3, n, None) == 1           # NULL input
    assert fn(D, MAX, hole, good_in, 3, n, None) == 1            # NULL output
    assert fn(D, MAX, None, good_in, 3, n, None) == 1            # NULL arrays
    assert fn(D, MAX, good_out, None, 3, n, None) == 1
    assert fn(D, O["xor"], good_out, good_in, 3, n, None) == 1   # not a reference pair
    assert fn(T["complexd"], MAX, good_out, good_in, 3, n, None) == 1
    assert fn(99, MAX, good_out, good_in, 3, n, None) == 1
    assert fn(T["int"], O["sum"], good_out, good_in, 3, n, None) == 3     # ENOTSUP
    assert fn(T["short"], O["min"], good_out, good_in, 3, n, None) == 3
    assert fn(D, O["sum"], good_out, good_in, 3, n, None) == 3
    # overlaps: outs[0] on ins[1]; on ins[1]'s last element; outs[0] == outs[2];
    # outs[1] shifted by one element from its own input
    for outs in ([A + 4096, 16 * A + 4096, 16 * A + 8192],
                 [A + 4096 + 8 * (n - 1), 16 * A + 4096, 16 * A + 8192],
                 [16 * A, 16 * A + 4096, 16 * A],
                 [16 * A, A + 4096 + 8, 16 * A + 8192]):
        assert fn(D, MAX, (ctypes.c_void_p * 3)(*outs), good_in, 3, n, None) == 1, outs
    assert shm.last_error() == 1
    # zero elements: nothing to do, whatever the arrays; in place is legal
    # (checked up to the launch on the GPU: tests/test_gpu_fold_orders.py)
    assert fn(D, MAX, None, None, 3, 0, None) == 0
    assert fn(D, MAX, hole, hole, 3, 0, None) == 0
    assert shm.last_error() == 0
    with pytest.raises(ValueError):
        shm.fold_orders_on_stream("double", "max", [A], [A, A + 4096], 8)
    with pytest.raises(shm.ShmemError) as e:
        shm.fold_orders_on_stream("int", "sum", [16 * A], [A], 8)
    assert e.value.code == 3
