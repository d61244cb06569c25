"""GPU parity of the P-order fold (shmemx_fold_orders_on_stream, OWNSLICE's
first phase): outs[k] = ins[k] folded with the other inputs ascending, for
every k in one launch.  Bit for bit against the existing fold kernel run once
per order, and against the oracle's PE k (reduce-op.c:219-248), on the six
pairs whose answer depends on the order, over NaNs of both signs, signed
zeros, infinities and the smallest normal."""
import ctypes

import numpy as np
import pytest
from gpu_util import from_dev, same_bits, to_dev

pytestmark = pytest.mark.gpu

PAIRS = [(t, o) for t in ("float", "double", "longdouble") for o in ("min", "max")]
PS = (1, 2, 3, 8, 9, 16)                 # 9 crosses into the 16-input instantiation
SHIFT = 3                                # spare elements in front of every array


def unrolled_chunk(t, P):
    """Elements of one full chunk of the kernel, which is also its block of
    vectors: 256 lanes x one 16-byte vector per input (kUnrollOrders = 1)."""
    E = 1 if t == "longdouble" else 4 if t == "float" else 2
    return 256 * E, 256 * E


def sizes(t, P):
    chunk, block = unrolled_chunk(t, P)
    return [0, 1, 5, 1013, 70001, chunk, chunk + block + 3]


_CACHE = {}


def case(oracle, t, op, P, n):
    """Sources (with SHIFT + 1 spare elements) and every member's expected
    result, computed once."""
    key = (t, op, P, n)
    if key not in _CACHE:
        srcs = oracle.special_sources(t, P, n + SHIFT + 1, seed=0x0D0E5 + 131 * P + n)
        _CACHE[key] = srcs
    return _CACHE[key]


def expected(oracle, t, op, view):
    P = view.shape[0]
    return [oracle.reduce_one(t, op, view, 0, 0, P, k) for k in range(P)]


def test_inputs_discriminate(oracle):
    """On the oracle alone: for every P >= 2 some member's answer differs
    from member 0's, so a kernel that handed every member one order fails."""
    for t, op in PAIRS:
        for P in PS[1:]:
            view = np.ascontiguousarray(case(oracle, t, op, P, 1013)[:, :1013])
            want = expected(oracle, t, op, view)
            assert any(not same_bits(want[k], want[0]) for k in range(1, P)), (t, op, P)


def dev_view(torch, t, buf, start, n):
    """Elements [start, start + n) of a device buffer (long double: raw 16-byte slots)."""
    w = 16 if t == "longdouble" else 1
    return buf[start * w:(start + n) * w]


def run(torch, shm, oracle, t, op, P, n, in_off, out_off, in_place=None):
    srcs = case(oracle, t, op, P, n)
    view = np.ascontiguousarray(np.stack([srcs[p][in_off[p]:in_off[p] + n] for p in range(P)]))
    ibuf = [to_dev(torch, srcs[p]) for p in range(P)]
    obuf = [torch.zeros_like(ibuf[p]) for p in range(P)]
    ins = [dev_view(torch, t, ibuf[p], in_off[p], n) for p in range(P)]
    outs = [dev_view(torch, t, obuf[p], out_off[p], n) for p in range(P)]
    if in_place is not None:
        outs[in_place] = ins[in_place]
    # the yardstick first (it reads the inputs the in-place launch overwrites)
    yard = []
    for k in range(P):
        y = torch.zeros_like(ins[k])
        shm.fold_n(t, op, y, [ins[k]] + [ins[j] for j in range(P) if j != k], n)
        yard.append(y)
    # zero-length tensors have no address to speak of: any non-NULL one does
    ptr = (lambda x: x.data_ptr() or 16) if n == 0 else (lambda x: x.data_ptr())
    shm.fold_orders_on_stream(t, op, [ptr(x) for x in outs], [ptr(x) for x in ins], n)
    torch.cuda.synchronize()
    want = expected(oracle, t, op, view) if n else [view[k] for k in range(P)]
    what = f"{t} {op} P={P} n={n} in_off={in_off} out_off={out_off} in_place={in_place}"
    for k in range(P):
        got = from_dev(outs[k], srcs.dtype)
        assert same_bits(got, from_dev(yard[k], srcs.dtype)), f"{what}: order {k} differs from fold_n"
        assert same_bits(got, want[k]), f"{what}: order {k} differs from the oracle"
        if in_place != k:        # nothing written outside [out_off, out_off + n)
            whole = from_dev(obuf[k], srcs.dtype).view(np.uint8).reshape(len(srcs[k]), -1)
            assert not whole[:out_off[k]].any() and not whole[out_off[k] + n:].any(), f"{what}: wrote outside"
    for p in range(P):           # inputs unchanged
        if in_place != p:
            assert same_bits(from_dev(ibuf[p], srcs.dtype), srcs[p]), f"{what}: input {p} changed"


@pytest.mark.parametrize("t,op", PAIRS)
def test_fold_orders_every_order_aligned(cuda, shm, oracle, t, op):
    import torch
    for P in PS:
        for n in sizes(t, P):
            run(torch, shm, oracle, t, op, P, n, [0] * P, [0] * P)


@pytest.mark.parametrize("t,op", PAIRS)
def test_fold_orders_head_and_scalar_paths(cuda, shm, oracle, t, op):
    """All arrays shifted alike by one element (a non-zero head where an
    element is smaller than 16 bytes), and one input shifted alone (no common
    alignment: the scalar path)."""
    import torch
    for P in (2, 8, 9):
        chunk, block = unrolled_chunk(t, P)
        for n in (5, 1013, chunk + block + 3):
            run(torch, shm, oracle, t, op, P, n, [1] * P, [1] * P)
            alone = [0] * P
            alone[P // 2] = 1
            run(torch, shm, oracle, t, op, P, n, alone, [0] * P)
            run(torch, shm, oracle, t, op, P, n, [0] * P, [0] * (P - 1) + [SHIFT])


@pytest.mark.parametrize("t,op", PAIRS)
def test_fold_orders_last_output_in_place(cuda, shm, oracle, t, op):
    """outs[P-1] is ins[P-1]: the owner's own target slice over its source."""
    import torch
    for P in (1, 3, 8, 16):
        chunk, block = unrolled_chunk(t, P)
        for n in (1013, chunk + block + 3):
            run(torch, shm, oracle, t, op, P, n, [0] * P, [0] * P, in_place=P - 1)
            run(torch, shm, oracle, t, op, P, n, [1] * P, [1] * P, in_place=P - 1)


def test_fold_orders_kernel_clock_kind(cuda, shm, oracle):
    """One launch, reported as a kind of its own (4, "orders_fold")."""
    import torch
    P, n = 3, 1013
    srcs = case(oracle, "double", "max", P, n)
    ins = [to_dev(torch, srcs[p][:n]) for p in range(P)]
    outs = [torch.empty_like(x) for x in ins]
    shm.kernel_timing(True)
    try:
        shm.fold_orders_on_stream("double", "max", outs, ins, n)
        kt, dropped = shm.kernel_times()
        us, kinds = (ctypes.c_double * 4)(), (ctypes.c_int * 4)()
        shm.fold_orders_on_stream("double", "max", outs, ins, n)
        got = shm.lib().shmemx_kernel_times(us, kinds, 4, None)
    finally:
        shm.kernel_timing(False)
    assert dropped == 0 and len(kt) == 1 and kt[0][0] == "orders_fold" and kt[0][1] > 0, kt
    assert got == 1 and kinds[0] == 4 and us[0] > 0
