"""The stream-ordered reduce-scatter's kernel (signal_kernels.hip
signal_reduce_scatter_kernel) and its unfused route (the device barriers around
the peers fold) in one process, through shmemx_reduce_scatter_loopback /
shm.reduce_scatter_loopback: member m's launches of a P-member set whose arrays
all live on this GPU, the handshakes looped back.  The grid barrier, the
fences, the XCD-coverage check and the fold run for real.

Every launch works on one device buffer that holds the target and the P whole
sources of P * nelems elements, each array between at least 64 canary bytes
(0xA5).  Block m of every source holds oracle.fill's (or, for the floating
types, also oracle.special_sources') values; the rest of a source, which the
call must never read, a constant byte.  Before the launch the target holds a
byte pattern.  After it

  target     = oracle.reduce_one(type, op, blocks, 0, 0, P, pe=0) on the [P,
               nelems] array of the members' block m, bit for bit (PE 0's
               order is set order; long double: the 10 x87 bytes of a slot);
  the rest   of the buffer, the canaries around the target and every source
               included, byte for byte as before;
  error word 0.

A 64-block grid of 256 lanes folds U = 4 / 2 / 1 vectors per lane per step for
up to 4 / 8 / 16 inputs, so the grid's step is 64 * 256 * U vectors.  The
vector body runs only when the target and all P block starts are 16-byte
aligned; block m starts m * nelems * size bytes into its source.
"""
import numpy as np
import pytest
from gpu_util import same_bits

pytestmark = pytest.mark.gpu

CANARY, GUARD = 0xA5, 64
KBLOCK, GRID, MAX_IN = 256, 64, 16
ELEM_SIZE = {"short": 2, "int": 4, "long": 8, "longlong": 8, "float": 4, "double": 8,
             "longdouble": 16, "complexd": 16, "complexf": 8}
TYPES = tuple(ELEM_SIZE)
PAIRS = [(t, o) for t in TYPES for o in ("sum", "prod")] + \
        [(t, o) for t in ("short", "int", "long", "longlong") for o in ("and", "or", "xor")] + \
        [(t, o) for t in ("short", "int", "long", "longlong", "float", "double", "longdouble")
         for o in ("min", "max")]
SPECIAL = 2     # oracle.special_sources instead of oracle.fill


def test_the_pairs_are_the_reference_pairs(shm):
    assert len(PAIRS) == 44 and sorted(PAIRS) == sorted(shm.REFERENCE_PAIRS)


def pattern(seed, nbytes):
    idx = np.arange(nbytes, dtype=np.uint32)
    return ((idx * np.uint32(2654435761) + np.uint32((seed * 0x9E3779B1 + 12345) & 0xFFFFFFFF)) >> np.uint32(13)) \
        .astype(np.uint8)


def blocks_of(oracle, t, kind, P, nelems, seed):
    """[P, nelems]: what block m of the members' sources holds."""
    if kind == SPECIAL:
        return oracle.special_sources(t, P, nelems, seed)
    return np.stack([oracle.fill(t, kind, seed + k, nelems) for k in range(P)])


def run_case(shm, oracle, cuda, t, op, P, m, nelems, fused=True, kind=1, tlead=0, slead=0, seed=0x5CA77E4):
    import torch
    sz = ELEM_SIZE[t]
    blocks = np.ascontiguousarray(blocks_of(oracle, t, kind, P, nelems, seed), dtype=oracle.NP_DTYPE[t])
    want = oracle.reduce_one(t, op, blocks, 0, 0, P, 0)
    size = 0

    def place(nbytes, lead):
        nonlocal size
        start = (size + 255) // 256 * 256 + GUARD + lead
        size = start + nbytes + GUARD
        return start

    tgt = place(nelems * sz, tlead)
    src = [place(P * nelems * sz, slead) for _ in range(P)]
    image = np.full(size + 256, CANARY, np.uint8)
    image[tgt:tgt + nelems * sz] = pattern(1, nelems * sz)
    for k in range(P):
        image[src[k]:src[k] + P * nelems * sz] = 0x30 + k
        at = src[k] + m * nelems * sz
        image[at:at + nelems * sz] = blocks[k].view(np.uint8)
    buf = torch.empty(image.size, dtype=torch.uint8, device=cuda)
    assert buf.data_ptr() % 256 == 0
    buf.copy_(torch.from_numpy(image))
    torch.cuda.synchronize()
    base = buf.data_ptr()
    err = shm.reduce_scatter_loopback(t, op, base + tgt, [base + s for s in src], nelems, m=m, fused=fused)
    got = buf.cpu().numpy()
    tag = f"{t} {op} P={P} m={m} nelems={nelems} fused={fused} kind={kind} tlead={tlead} slead={slead}"
    assert err == 0, f"{tag}: signal error word {err}"
    end = tgt + nelems * sz
    assert np.array_equal(got[:tgt], image[:tgt]), f"{tag}: bytes before the target changed"
    if not np.array_equal(got[end:], image[end:]):
        bad = np.flatnonzero(got[end:] != image[end:])
        raise AssertionError(f"{tag}: {bad.size} bytes after the target changed (a source or a canary), "
                             f"first at target end{bad[0]:+d}")
    res = got[tgt:end].copy().view(oracle.NP_DTYPE[t])
    if not same_bits(res, want):
        a, b = res.view(np.uint8).reshape(nelems, sz), want.view(np.uint8).reshape(nelems, sz)
        width = 10 if t == "longdouble" else sz
        bad = np.flatnonzero((a[:, :width] != b[:, :width]).any(axis=1))
        raise AssertionError(f"{tag}: {bad.size} of {nelems} elements differ, first {bad[0]}: "
                             f"got {res[bad[0]]!r} want {want[bad[0]]!r}")


@pytest.mark.parametrize("t,op", PAIRS, ids=[f"{t}-{o}" for t, o in PAIRS])
def test_all_pairs(shm, oracle, cuda, t, op):
    # 1027 elements: block 1 starts off a 16-byte boundary for the 2- and
    # 4-byte types (the element loop), on one for the others (vectors + tail)
    for kind in (0, 1) + ((SPECIAL,) if t in ("float", "double", "longdouble") else ()):
        run_case(shm, oracle, cuda, t, op, 3, 1, 1027, kind=kind)


@pytest.mark.parametrize("P", [1, 2, 4, 5, 8, 9, 16])
def test_member_counts(shm, oracle, cuda, P):
    # both sides of every fold_vecs instantiation (4 / 5, 8 / 9, 16 inputs)
    for m in (range(P) if P == 5 else sorted({0, P - 1})):
        run_case(shm, oracle, cuda, "int", "sum", P, m, 1028)        # vectors
        run_case(shm, oracle, cuda, "int", "sum", P, m, 1027)        # m odd: the element loop


@pytest.mark.parametrize("nelems", [1, 4, 1024, 1025])
def test_sizes(shm, oracle, cuda, nelems):
    for t, op in (("int", "sum"), ("double", "max"), ("short", "xor")):
        for m in (0, 2):
            run_case(shm, oracle, cuda, t, op, 3, m, nelems)
            run_case(shm, oracle, cuda, t, op, 3, m, nelems, fused=False)


@pytest.mark.parametrize("P", [3, 8, 16])
def test_partial_steps(shm, oracle, cuda, P):
    """One case per MAXIN: 16-byte aligned blocks (m even) of two full grid
    steps plus a partial step of 3 * kBlock + 5 vectors, and 1 trailing
    element."""
    U = MAX_IN // (4 if P <= 4 else 8 if P <= 8 else 16)
    nvec = 2 * GRID * KBLOCK * U + 3 * KBLOCK + 5
    run_case(shm, oracle, cuda, "double", "sum", P, 2, 2 * nvec + 1)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("t,op", [("longdouble", "sum"), ("complexd", "prod")])
def test_heavy_ops(shm, oracle, cuda, t, op, fused):
    for m in range(3):
        run_case(shm, oracle, cuda, t, op, 3, m, 257, fused=fused)
    if t == "longdouble":
        run_case(shm, oracle, cuda, t, op, 3, 1, 257, fused=fused, kind=SPECIAL)


def test_unfused_route(shm, oracle, cuda):
    run_case(shm, oracle, cuda, "int", "sum", 3, 1, 7, fused=False)                # small: elements
    run_case(shm, oracle, cuda, "double", "sum", 5, 2, 40962, fused=False)         # vectors, several blocks
    run_case(shm, oracle, cuda, "float", "min", 9, 3, 4099, fused=False, kind=SPECIAL)


def test_operands_off_a_16_byte_boundary(shm, oracle, cuda):
    """The target alone, the sources alone, and both off a 16-byte boundary:
    the element loop takes the whole block."""
    for tlead, slead in ((8, 0), (0, 8), (8, 8)):
        run_case(shm, oracle, cuda, "double", "sum", 3, 2, 1030, tlead=tlead, slead=slead)
        run_case(shm, oracle, cuda, "short", "max", 5, 4, 1032, tlead=tlead // 4, slead=slead // 4)
