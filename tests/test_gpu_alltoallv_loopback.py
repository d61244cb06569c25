"""The stream-ordered alltoall / alltoallv kernels (signal_kernels.hip:
signal_alltoallv_kernel and the unfused plan / copy kernels) in one process,
through shmemx_alltoallv_loopback / shm.alltoallv_loopback: receiver m's
launches of a P-member exchange whose arrays all live on this GPU, the count
and offset tables in private device memory, the handshakes looped back.  The
2 P table loads, the plan, the per-segment copy and both barriers run for real.

Every launch works on one device buffer that holds the target and the P
sources, each array with its own position-dependent pattern and at least 64
canary bytes (0xA5) on both sides.  After the launch the WHOLE buffer is
compared, byte for byte, with what numpy says it must hold:

  healthy    target[off_i : off_i + n_i] = srcs[i][from_i : from_i + n_i] with
             n_i = counts[i][m], from_i = offsets[i][m], off_i = n_0 + ... +
             n_(i-1); where = (off_0 .. off_(P-1), total); no overflow;
  overflow   (a bad pair, or total > capacity) the buffer as before the
             launch; where = P + 1 times all ones; one overflow counted;
  both       the device barriers' error word 0, and every other byte as
             before: the canaries, the sources, the target past the total.

A source starts 16-byte aligned plus its lead; a segment whose source block
and target block agree mod 16 takes the vector path (with a head and a tail
of elements when it does not start on a boundary), any other the element-wide
path.

A 64-block grid of 256 lanes copies U = 4 / 2 / 1 units per lane per step for
up to 4 / 8 / 16 segments: 70 001 x 8 bytes are past two steps (of 256 KiB) at
more than 8 segments.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANARY, GUARD = 0xA5, 64
ONES = (1 << 64) - 1


def pattern(seed, nbytes):
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


def rows_of(counts, gap=lambda i, j: (i + 2 * j) % 3, unit=1):
    """Offsets for a count matrix: sender i lays its blocks out in DESCENDING
    receiver order, rotated by i, with gaps between them: non-monotonic and
    non-contiguous in j.  Returns (offsets, the elements the longest row
    needs).  unit: every offset a multiple of it."""
    P = len(counts)
    offsets, need = [[0] * P for _ in range(P)], 0
    for i in range(P):
        at = 0
        for r in range(P):
            j = (i - r) % P
            at += gap(i, j) * unit
            offsets[i][j] = at
            at += (counts[i][j] + unit - 1) // unit * unit
        need = max(need, at)
    return offsets, need


def is_vector(src_addr, dst_addr):
    return (src_addr ^ dst_addr) & 15 == 0


def run_case(shm, cuda, P, m, esize, counts, offsets, capacity, src_capacity, fused, leads=None, tgt_lead=0,
             overflow=False, want_kinds=None):
    """One call of receiver m.  counts / offsets None: the fixed alltoall of
    capacity // P elements per pair.  leads[i]: bytes source i starts past a
    16-byte boundary.  want_kinds: the set of copy paths the non-empty
    segments must take, {"vector"}, {"element"} or both."""
    import torch
    leads = leads or [0] * P
    fixed = counts is None
    if fixed:
        nelems = capacity // P
        n = [nelems] * P
        frm = [m * nelems] * P
        src_capacity = capacity
    else:
        n = [counts[i][m] for i in range(P)]
        frm = [offsets[i][m] for i in range(P)]
    lay = Layout()
    tgt = lay.add(capacity * esize, tgt_lead)
    src = [lay.add(src_capacity * esize, leads[i]) for i in range(P)]
    image = np.full(lay.size + 256, CANARY, np.uint8)
    for k, (start, length) in enumerate(lay.arrays):
        image[start:start + length] = pattern(k + 1, length)
    want = image.copy()
    total = sum(n)
    off = [sum(n[:i]) for i in range(P)]
    if not overflow:
        assert total <= capacity and all(frm[i] + n[i] <= src_capacity for i in range(P))
        for i in range(P):
            want[tgt + off[i] * esize:tgt + (off[i] + n[i]) * esize] = \
                image[src[i] + frm[i] * esize:src[i] + (frm[i] + n[i]) * esize]
    buf = torch.empty(image.size, dtype=torch.uint8, device=cuda)
    assert buf.data_ptr() % 256 == 0
    if want_kinds is not None and not overflow:
        kinds = {"vector" if is_vector(src[i] + frm[i] * esize, tgt + off[i] * esize) else "element"
                 for i in range(P) if n[i]}
        assert kinds == want_kinds, (kinds, want_kinds)
    buf.copy_(torch.from_numpy(image))
    torch.cuda.synchronize()
    base = buf.data_ptr()
    where, over, err = shm.alltoallv_loopback(base + tgt, [base + s for s in src], counts, offsets, capacity,
                                              src_capacity, esize, m=m, fused=fused)
    got = buf.cpu().numpy()
    tag = (f"P={P} m={m} esize={esize} n={n} from={frm} capacity={capacity} src_capacity={src_capacity} "
           f"fused={fused} fixed={fixed} leads={leads} tgt_lead={tgt_lead}")
    assert err == 0, f"{tag}: signal error word {err}"
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{tag}: {bad.size} bytes differ, first at target{bad[0] - tgt:+d}, "
                             f"got {got[bad[0]]:#x} want {want[bad[0]]:#x}")
    if overflow:
        assert (where, over) == ([ONES] * (P + 1), 1), f"{tag}: where {where} overflows {over}"
    else:
        assert (where, over) == (off + [total], 0), f"{tag}: where {where} overflows {over}"


def members_of(P):
    return sorted({0, P // 2, P - 1})


def mixed_leads(P, m, esize, counts, offsets, tgt_lead):
    """Leads that make the even senders' segments agree with their target
    blocks mod 16 (vectors, with a head and a tail where the block does not
    start on a boundary) and the odd senders' differ by one element
    (element-wide words)."""
    off = 0
    leads = []
    for i in range(P):
        want = tgt_lead + off * esize + (0 if i % 2 == 0 else esize)
        leads.append((want - offsets[i][m] * esize) % 16)
        off += counts[i][m]
    return leads


@pytest.mark.parametrize("P", [2, 3, 8, 16])
def test_alltoallv_loopback_small_shapes(shm, cuda, P):
    """Both element widths, both routes, m first / middle / last: all-aligned
    blocks (vectors only), odd counts with mixed leads (element-wide and
    head/tail segments in one call), rows with zeros, all from non-monotonic,
    non-contiguous source offsets; totals equal to the capacity and below it."""
    ncases = 0
    for esize in (4, 8):
        g = 16 // esize
        aligned = [[g * (1 + (7 * i + 3 * j) % 5) for j in range(P)] for i in range(P)]
        odd = [[(1, 3, 5, 7, 1013)[(i + 2 * j) % 5] for j in range(P)] for i in range(P)]
        zeros = [[0 if (i + j) % 3 == 0 else 3 + i + 2 * j for j in range(P)] for i in range(P)]
        none = [[0] * P for _ in range(P)]
        for fused in (True, False):
            for m in members_of(P):
                k = ncases
                # vectors only: counts, offsets, leads and gaps all whole 16-byte granules
                offsets, need = rows_of(aligned, unit=g)
                total = sum(aligned[i][m] for i in range(P))
                run_case(shm, cuda, P, m, esize, aligned, offsets, total + (0 if k % 2 else g), need, fused,
                         want_kinds={"vector"})
                # odd counts: element-wide and head/tail vector segments in one call
                offsets, need = rows_of(odd)
                total = sum(odd[i][m] for i in range(P))
                tgt_lead = 8 if k % 2 else 0
                run_case(shm, cuda, P, m, esize, odd, offsets, total + (5 if k % 2 else 0), need + k % 3, fused,
                         leads=mixed_leads(P, m, esize, odd, offsets, tgt_lead), tgt_lead=tgt_lead,
                         want_kinds={"vector", "element"})
                # rows with zeros (member m's own block among them for some m), and nothing at all
                offsets, need = rows_of(zeros)
                total = sum(zeros[i][m] for i in range(P))
                run_case(shm, cuda, P, m, esize, zeros, offsets, max(1, total), need, fused)
                offsets, need = rows_of(none)       # an empty block's offset must lie inside the source too
                run_case(shm, cuda, P, m, esize, none, offsets, 4, need, fused)
                ncases += 4
    print(f"P={P}: {ncases} launches")


@pytest.mark.parametrize("P", [9, 16])
def test_alltoallv_loopback_long_block_at_nine_senders(shm, cuda, P):
    """Nine senders hold a block for member m, one of them 70 001 x 8 bytes
    (8-byte elements; the same bytes as 140 002 4-byte ones), the others short
    odd counts: more than 8 segments, so a lane copies one unit per step and
    the long block runs past two steps of the fused grid while the short ones
    are done; once aligned (vectors with a tail) and once 8 bytes off
    (element-wide)."""
    for esize, long_count in ((8, 70001), (4, 140002)):
        for m in members_of(P):
            long_at = (0, 8, 4)[m % 3]              # the first, the last and a middle one of the nine
            counts = [[0] * P for _ in range(P)]
            for i in range(9):
                counts[i][m] = 3 + 2 * i
                counts[i][(m + 1) % P] = 5          # a neighbour column the call must not read
            counts[long_at][m] = long_count
            offsets, need = rows_of(counts, unit=16 // esize)
            total = sum(counts[i][m] for i in range(P))
            assert sum(1 for i in range(P) if counts[i][m]) == 9 and long_count * esize > 2 * 64 * 256 * 16
            for lead in (0, 8):
                leads = [0] * P
                leads[long_at] = lead
                for fused in (True, False):
                    run_case(shm, cuda, P, m, esize, counts, offsets, total, need, fused, leads=leads)


@pytest.mark.parametrize("P", [2, 3, 8, 16])
def test_alltoall_loopback_fixed_blocks(shm, cuda, P):
    """The fixed alltoall through the same kernels with immediates: nelems 1,
    3, 4 and 1013, so blocks of 4 to 8104 bytes that are and are not multiples
    of 16; block i of the target is block m of source i."""
    for esize in (4, 8):
        for nelems in (1, 3, 4, 1013):
            for m in members_of(P):
                for fused in (True, False):
                    run_case(shm, cuda, P, m, esize, None, None, P * nelems, P * nelems, fused)
                    run_case(shm, cuda, P, m, esize, None, None, P * nelems, P * nelems, fused,
                             leads=[(i * esize) % 16 for i in range(P)], tgt_lead=8 if m else 0)


@pytest.mark.parametrize("P", [2, 3, 8, 16])
def test_alltoallv_loopback_overflow_is_an_answer_not_a_fault(shm, cuda, P):
    """total == capacity + 1, and a peer's pair whose offset + count is one
    element past src_capacity (also a count above it, and offset 2^64 - 1):
    the buffer is unchanged, the canaries past that peer's source included,
    so nothing was read into the target; where is all ones, one overflow is
    counted and the device barriers' error word stays 0.  The healthy call
    that follows each is exact."""
    for esize in (4, 8):
        counts = [[5 + 3 * i + j for j in range(P)] for i in range(P)]
        offsets, need = rows_of(counts)
        for fused in (True, False):
            for m in members_of(P):
                total = sum(counts[i][m] for i in range(P))
                run_case(shm, cuda, P, m, esize, counts, offsets, total - 1, need, fused, overflow=True)
                run_case(shm, cuda, P, m, esize, counts, offsets, total, need, fused)
                peer = (m + 1) % P
                for bad_count, bad_offset in ((counts[peer][m], need - counts[peer][m] + 1),
                                              (need + 1, 0), (counts[peer][m], ONES), (ONES, 1)):
                    c = [list(r) for r in counts]
                    o = [list(r) for r in offsets]
                    c[peer][m], o[peer][m] = bad_count, bad_offset
                    run_case(shm, cuda, P, m, esize, c, o, 4 * total + need, need, fused, overflow=True)
                    # the same garbage in a column this receiver does not read is harmless
                    c = [list(r) for r in counts]
                    o = [list(r) for r in offsets]
                    c[peer][(m + 1) % P], o[peer][(m + 1) % P] = bad_count, bad_offset
                    run_case(shm, cuda, P, m, esize, c, o, 4 * total + need, need, fused)
                # flush with the source's end: the last element that may be read
                o = [list(r) for r in offsets]
                o[peer][m] = need - counts[peer][m]
                run_case(shm, cuda, P, m, esize, counts, o, total, need, fused)
