"""The stream-ordered collect's kernels (signal_kernels.hip: signal_collect_kernel
and the unfused publish / plan / copy kernels) in one process, through
shmemx_collect_loopback / shm.collect_loopback: member m's launches of a
P-member collect whose arrays all live on this GPU, the peers' counts given,
the handshakes looped back.  The publish, the exchange of the count words, the
plan, the per-segment copy and both barriers run for real.

Every launch works on one device buffer that holds the target and the P
sources, each array with its own position-dependent pattern and at least 64
canary bytes (0xA5) on both sides.  After the launch the WHOLE buffer is
compared, byte for byte, with what numpy says it must hold:

  healthy    target[off_i : off_i + n_i] = srcs[i][:n_i], off_i = n_0 + ... +
             n_(i-1), for every member i; where = (off_m, total); no overflow;
  overflow   (a poison count, or total > capacity) the buffer as before the
             launch; where = (all ones, all ones); one overflow counted;
  both       the device barriers' error word 0, and every other byte as
             before: the canaries, the sources, the target past the total.

A source starts 16-byte aligned plus its lead; a segment whose source and
target agree mod 16 takes the vector path (with a head and a tail of elements
when the lead is not 0), any other the element-wide path.

A 64-block grid of 256 lanes copies U = 4 / 2 / 1 units per lane per step for
up to 4 / 8 / 16 segments: 70 001 x 8 bytes are past two steps (of 256 KiB) at
more than 8 segments, and past one at more than 4.
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


def run_case(shm, cuda, P, m, esize, counts, capacity, fused, counted, leads=None, tgt_lead=0, overflow=False,
             tight=False):
    """One call of member m.  counts: what the members publish (ONES: a
    poison peer).  leads[i]: bytes source i starts past a 16-byte boundary.
    tight: source m lies just below the target, with less room than its
    count, so member m publishes poison itself."""
    import torch
    leads = leads or [0] * P
    real = [0 if c == ONES else c for c in counts]
    lay = Layout()
    src = [None] * P
    if tight:
        src[m] = lay.add(16, leads[m])                  # its room ends at the target: a few hundred bytes
    tgt = lay.add(capacity * esize, tgt_lead)
    for i in range(P):
        if src[i] is None:
            src[i] = lay.add(max(real[i] * esize, 16), leads[i])
    image = np.full(lay.size + 256, CANARY, np.uint8)
    for k, (start, length) in enumerate(lay.arrays):
        image[start:start + length] = pattern(k + 1, length)
    want = image.copy()
    total = sum(real)
    off = [sum(real[:i]) for i in range(P)]
    if not overflow:
        assert total <= capacity and ONES not in counts and not tight
        for i in range(P):
            want[tgt + off[i] * esize:tgt + (off[i] + real[i]) * esize] = image[src[i]:src[i] + real[i] * esize]
    if tight:
        assert (tgt - src[m]) // esize < counts[m] <= capacity
    buf = torch.empty(image.size, dtype=torch.uint8, device=cuda)
    assert buf.data_ptr() % 256 == 0
    buf.copy_(torch.from_numpy(image))
    torch.cuda.synchronize()
    base = buf.data_ptr()
    w0, w1, over, err = shm.collect_loopback(base + tgt, [base + s for s in src], counts, capacity, esize, m=m,
                                             fused=fused, counted=counted)
    got = buf.cpu().numpy()
    tag = (f"P={P} m={m} esize={esize} counts={counts} capacity={capacity} fused={fused} counted={counted} "
           f"leads={leads} tgt_lead={tgt_lead}")
    assert err == 0, f"{tag}: signal error word {err}"
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{tag}: {bad.size} bytes differ, first at target{bad[0] - tgt:+d}, "
                             f"got {got[bad[0]]:#x} want {want[bad[0]]:#x}")
    if overflow:
        assert (w0, w1, over) == (ONES, ONES, 1), f"{tag}: where ({w0:#x}, {w1:#x}) overflows {over}"
    else:
        assert (w0, w1, over) == (off[m], total, 0), f"{tag}: where ({w0}, {w1}) overflows {over}"


def members_of(P):
    return sorted({0, P // 2, P - 1})


def count_sets(P, esize):
    """[(counts, leads, tgt_lead)]"""
    g = 16 // esize
    sets = []
    # every count a whole number of 16-byte granules, everything aligned: vectors only
    sets.append(([g * (1 + (7 * i) % 5) for i in range(P)], [0] * P, 0))
    # odd counts: the offsets leave most segments off their sources' alignment (element-wide words); the
    # even members' sources start where their target segment does mod 16 (vectors with a head and a tail)
    odd = [(1, 3, 5, 7, 1013)[i % 5] for i in range(P)]
    off = [sum(odd[:i]) for i in range(P)]
    sets.append((odd, [(off[i] * esize) % 16 if i % 2 == 0 else 0 for i in range(P)], 0))
    # the same with the target 8 bytes off
    sets.append((odd, [(off[i] * esize + 8) % 16 if i % 2 == 0 else 0 for i in range(P)], 8))
    # zeros in the middle
    zeros = [0 if P // 3 <= i < max(P // 3 + 1, 2 * P // 3) and P > 1 else 3 + i for i in range(P)]
    sets.append((zeros, [0] * P, 0))
    sets.append(([0] * P, [0] * P, 0))
    return sets


@pytest.mark.parametrize("P", [1, 2, 3, 8, 16])
def test_collect_loopback_small_shapes(shm, cuda, P):
    """Both element widths, both routes, the count immediate and read from
    device memory, m first / middle / last; totals equal to the capacity and
    below it."""
    ncases = 0
    for esize in (4, 8):
        for k, (counts, leads, tgt_lead) in enumerate(count_sets(P, esize)):
            for m in members_of(P):
                for fused in (True, False):
                    for counted in (False, True):
                        slack = 0 if (k + m + fused + counted) % 2 == 0 else 5
                        capacity = max(1, sum(counts) + slack)
                        run_case(shm, cuda, P, m, esize, counts, capacity, fused, counted, leads, tgt_lead)
                        ncases += 1
    print(f"P={P}: {ncases} launches")
    assert ncases >= 2 * 5 * 2 * 2


@pytest.mark.parametrize("P", [3, 8, 16])
def test_collect_loopback_long_segment(shm, cuda, P):
    """One member holds 70 001 x 8 bytes (8-byte elements; the same bytes as
    140 002 4-byte ones), the others short odd counts and a zero: the long
    segment runs several passes of the grid while the short ones are done;
    once aligned (vectors with a tail) and once 8 bytes off (element-wide)."""
    for esize, long_count in ((8, 70001), (4, 140002)):
        for long_at in (0, P - 1):
            counts = [3 + 2 * i for i in range(P)]
            counts[P // 2] = 0
            counts[long_at] = long_count
            for lead in (0, 8):
                leads = [0] * P
                leads[long_at] = lead
                for fused in (True, False):
                    m = (long_at + 1) % P
                    run_case(shm, cuda, P, m, esize, counts, sum(counts), fused, lead == 8, leads)


@pytest.mark.parametrize("P", [1, 2, 3, 8, 16])
def test_collect_loopback_overflow_is_an_answer_not_a_fault(shm, cuda, P):
    """total == capacity + 1, a poison peer, and a member whose own source
    has too little room (it publishes poison itself): the target is unchanged,
    where is all ones, one overflow is counted and the device barriers' error
    word stays 0; the healthy call that follows each is exact."""
    for esize in (4, 8):
        for fused in (True, False):
            for counted in (False, True):
                for m in members_of(P):
                    counts = [5 + 3 * i for i in range(P)]
                    total = sum(counts)
                    run_case(shm, cuda, P, m, esize, counts, total - 1, fused, counted, overflow=True)
                    run_case(shm, cuda, P, m, esize, counts, total, fused, counted)
                    if P > 1:
                        poisoned = list(counts)
                        poisoned[(m + 1) % P] = ONES
                        run_case(shm, cuda, P, m, esize, poisoned, 4 * total, fused, counted, overflow=True)
                        run_case(shm, cuda, P, m, esize, counts, 4 * total, fused, counted)
                    # my own count fits the capacity, not my source's room below the target
                    mine = list(counts)
                    mine[m] = 1013
                    run_case(shm, cuda, P, m, esize, mine, sum(mine) + 7, fused, counted, overflow=True, tight=True)
                    run_case(shm, cuda, P, m, esize, mine, sum(mine) + 7, fused, counted)
                    # my own count above the capacity
                    run_case(shm, cuda, P, m, esize, mine, 1012, fused, counted, overflow=True)
