"""The fused pull kernel (signal_kernels.hip signal_pull_kernel) in one
process, through shmemx_pull_loopback / shm.pull_loopback: member m's launch
of a P-member stream-ordered fcollect (schedule 0), one-phase broadcast (1) or
two-phase broadcast (2) whose members' arrays all live on this GPU, with the
peer handshakes looped back onto the launch's own counters.  The grid barrier,
the fences, the XCD-coverage check and both gathers run for real.

Every launch works on one device buffer that holds the P sources and the P
targets, each array with its own position-dependent pattern and at least 64
canary bytes (0xA5) on both sides.  After member m's launch the WHOLE buffer
is compared, byte for byte, with what numpy says it must hold:

  fcollect    tgts[m] = srcs[0] | srcs[1] | ... | srcs[P-1];
  one phase   tgts[m] = srcs[root]                       (m != root);
  two phase   tgts[m][lo(m):hi(m)] = srcs[root] there, and
              tgts[m][lo(i):hi(i)] = what tgts[i] held there before the launch,
              for every other non-root i                 (m != root);
  all         every other byte as before: the canaries, the sources, the other
              members' targets, and for m == root its own target too.

The slices lo/hi are restated here (slices_of), independent of set_geom.h:
ceil(n / (P - 1)) elements rounded up to whole 16-byte granules, over the
non-roots in set order.

A 64-block grid of 256 lanes copies U = 4 / 2 / 1 vectors per lane per step
for a list of up to 4 / 8 / 16 segments, so a step is 64 * 256 * U * 16 bytes
per segment: 1 MiB up to 4 segments, 512 KiB up to 8, 256 KiB up to 16.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANARY, GUARD = 0xA5, 64
GRID, KBLOCK = 64, 256
FCOLLECT, ONE_PHASE, TWO_PHASE = 0, 1, 2


def step_bytes(nseg):
    """Bytes of one segment that one pass of the grid copies, for a list of
    nseg segments."""
    u = 4 if nseg <= 4 else 2 if nseg <= 8 else 1
    return GRID * KBLOCK * u * 16


def slices_of(n, P, root, esize):
    """{non-root i: (lo, hi)} in elements."""
    g = 16 // esize
    per = -(-n // (P - 1))
    sl = -(-per // g) * g
    out, k = {}, 0
    for i in range(P):
        if i == root:
            continue
        out[i] = (min(n, k * sl), min(n, (k + 1) * sl))
        k += 1
    return out


def pattern(seed, nbytes):
    """nbytes bytes that depend on the array (seed) and the position."""
    idx = np.arange(nbytes, dtype=np.uint32)
    return ((idx * np.uint32(2654435761) + np.uint32((seed * 0x9E3779B1 + 12345) & 0xFFFFFFFF)) >> np.uint32(13)) \
        .astype(np.uint8)


class Layout:
    """Arrays in one buffer: each starts 16-byte aligned plus its lead, with
    at least GUARD canary bytes before and after it."""

    def __init__(self):
        self.size = 0
        self.arrays = []

    def add(self, nbytes, lead=0):
        start = (self.size + 255) // 256 * 256 + GUARD + lead
        self.size = start + nbytes + GUARD
        self.arrays.append((start, nbytes))
        return start


def run_case(shm, cuda, schedule, P, m, root, esize, n, mode="aligned", lean=False):
    """One launch.  mode: "aligned" every array on a 16-byte boundary; "src4"
    every source 4 bytes past one (the byte path); "inplace" tgts[i] is
    srcs[i] (broadcasts).  lean: the arrays the launch never touches are 64
    bytes long (the big cases)."""
    import torch
    nb = n * esize
    tlen = P * nb if schedule == FCOLLECT else nb
    lay = Layout()
    src_used = [schedule == FCOLLECT or i == root for i in range(P)]
    tgt_used = [i == m or (schedule == TWO_PHASE and i != root) for i in range(P)]
    tgt = [lay.add(tlen if tgt_used[i] or not lean else 64) for i in range(P)]
    if mode == "inplace":
        assert schedule != FCOLLECT and not lean
        src = list(tgt)
    else:
        src = [lay.add(nb if src_used[i] or not lean else 64, 4 if mode == "src4" else 0) for i in range(P)]
    image = np.full(lay.size + 256, CANARY, np.uint8)
    for k, (start, length) in enumerate(lay.arrays):
        image[start:start + length] = pattern(k + 1, length)
    want = image.copy()
    if schedule == FCOLLECT:
        for i in range(P):
            want[tgt[m] + i * nb:tgt[m] + (i + 1) * nb] = image[src[i]:src[i] + nb]
    elif m != root and schedule == ONE_PHASE:
        want[tgt[m]:tgt[m] + nb] = image[src[root]:src[root] + nb]
    elif m != root:
        for i, (lo, hi) in slices_of(n, P, root, esize).items():
            frm = src[root] if i == m else tgt[i]
            want[tgt[m] + lo * esize:tgt[m] + hi * esize] = image[frm + lo * esize:frm + hi * esize]
    buf = torch.empty(image.size, dtype=torch.uint8, device=cuda)
    assert buf.data_ptr() % 256 == 0
    buf.copy_(torch.from_numpy(image))
    torch.cuda.synchronize()
    base = buf.data_ptr()
    err = shm.pull_loopback(schedule, [base + t for t in tgt], [base + s for s in src], n, esize, m=m, root=root)
    got = buf.cpu().numpy()
    tag = f"schedule={schedule} P={P} m={m} root={root} esize={esize} n={n} mode={mode}"
    assert err == 0, f"{tag}: signal error word {err}"
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        where = [f"tgt[{i}]+{bad[0] - t}" for i, t in enumerate(tgt) if t - GUARD <= bad[0] < t + tlen + GUARD]
        raise AssertionError(f"{tag}: {bad.size} bytes differ, first at {bad[0]} ({where}), "
                             f"got {got[bad[0]]:#x} want {want[bad[0]]:#x}")
    if m == root and schedule != FCOLLECT:      # the root's target is never written
        assert np.array_equal(got[tgt[m]:tgt[m] + nb], image[tgt[m]:tgt[m] + nb]), tag


def roots_of(P):
    return sorted({0, P // 2, P - 1})


def members_of(P, root):
    """The root itself, its right neighbour and the member furthest from it."""
    return sorted({root, (root + 1) % P, (root + P // 2) % P})


@pytest.mark.parametrize("P", [1, 2, 3, 8, 16])
def test_pull_loopback_small_shapes(shm, cuda, P):
    """1 element; 3 elements, fewer than the non-roots at 8 and 16 members, so
    most slices are empty; 1013 elements: a vector body plus a byte tail.
    Both element sizes, every alignment mode, roots 0 / middle / P - 1, m the
    root and other members."""
    ncases = 0
    for esize in (4, 8):
        for n in (1, 3, 1013):
            for mode in ("aligned", "src4", "inplace"):
                for root in roots_of(P):
                    for m in members_of(P, root):
                        for schedule in (FCOLLECT, ONE_PHASE, TWO_PHASE):
                            if schedule == FCOLLECT and (mode == "inplace" or root != roots_of(P)[0]):
                                continue        # an fcollect has no root and is never in place
                            run_case(shm, cuda, schedule, P, m, root, esize, n, mode)
                            ncases += 1
    print(f"P={P}: {ncases} launches")
    assert ncases >= 3 * 2 * 3 * 2      # even at P == 1


def big_elems(nseg, esize):
    """Elements of one segment: two full grid steps, a partial step and a
    byte tail, for a list of nseg segments."""
    nb = 2 * step_bytes(nseg) + 40 * KBLOCK * 16 + 3 * 16 + 8
    assert nb % 16 == 8 and nb % esize == 0
    return nb // esize


@pytest.mark.parametrize("P", [3, 8, 16])
def test_pull_loopback_past_two_grid_steps(shm, cuda, P):
    """Every list's vector loop runs two full passes of the grid, a partial
    one and a byte tail: the fcollect's P segments, the one-phase broadcast's
    one, and the two-phase broadcast's P - 2 segments of list B (whose slices
    are that long).  16-byte aligned; and once on the byte path."""
    esize = 4 if P == 8 else 8
    root, m = P // 2, P - 1
    run_case(shm, cuda, FCOLLECT, P, m, root, esize, big_elems(P, esize), lean=True)
    run_case(shm, cuda, ONE_PHASE, P, m, root, esize, big_elems(1, esize), lean=True)
    # P - 1 slices of big_elems each, less a few elements: a short last slice
    n = (P - 1) * big_elems(max(1, P - 2), esize) - 5
    sl = slices_of(n, P, root, esize)
    assert all((hi - lo) * esize > 2 * step_bytes(P - 2) for lo, hi in sl.values())
    run_case(shm, cuda, TWO_PHASE, P, m, root, esize, n, lean=True)
    if P == 3:
        run_case(shm, cuda, TWO_PHASE, P, 0, root, esize, n, mode="src4", lean=True)
        run_case(shm, cuda, TWO_PHASE, P, root, root, esize, n, lean=True)     # the root: handshakes only
