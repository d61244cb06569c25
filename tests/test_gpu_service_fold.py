"""The service workgroup's fold of the small-call exchange (service.hip
fold_slots, member_at, unpack_cfg) in one process, through
shmemx_service_fold_loopback / shm.service_fold_loopback: the hook fills a
private image of the exchange's 64 slots with 0xA5, copies every member's
source into its slot and posts the real fold request as PE `me` of the set.

Sources are rows of one read-only [64, SLOT // size] array per (type, kind):
row q is PE q's source, so the rows outside a set hold other seeds and a read
of a wrong slot shows.  The reference of every case is
oracle.reduce_sim(t, op, rows, PE_start, logPE_stride, PE_size): row `me` with
own_order, row PE_start without.  The fold is element-wise, so one reduce_sim
per (type, kind, op, set) over the whole rows, sliced, serves every n (special
values: per n, they are no prefix of each other).

Comparison is bit for bit (gpu_util.same_bits: a long double's 10 value
bytes), except float / double sum and prod on special values: NaN exactly
where the oracle has NaN, the same bits elsewhere.  No tolerance anywhere.

Every target sits in a 0xA5-filled buffer of its own, dst in one and dst2 in
another; after each call every byte outside [dst, dst + n * size) must still
be 0xA5, the same for dst2, and dst2 must hold dst's bytes (or, when absent,
its buffer is untouched).  Every request must count in shmemx_service_stats as
served and as a fold.  Only results are asserted; nothing is timed.

SLOT is node::kXchgSlotBytes; test_slot_constant_matches_the_library (no GPU)
keeps the two together, and the 767 / 768 / 769 / 1537-word cases (the copy
threads' second trip over a slot) join the size group by themselves once SLOT
is large enough to hold them.

cases() builds every case without torch or a GPU; test_service_fold_case_lists
(no GPU) checks that the list holds what the GPU tests claim.
"""
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest
from gpu_util import same_bits, value_bytes
from test_gpu_fold import DEVICE_PAIRS

gpu = pytest.mark.gpu

SLOT = 4096                   # node::kXchgSlotBytes
NPES = 64                     # node::kMaxPes: the slots of the exchange
CANARY = 0xA5
COPY_THREADS = 768            # kCopyThreads: copy thread t folds words t, t + 768, ...
SECOND_TRIP_WORDS = (767, 768, 769, 1537)
ELEM_SIZE = {"short": 2, "int": 4, "long": 8, "longlong": 8, "float": 4, "double": 8,
             "longdouble": 16, "complexd": 16, "complexf": 8}
BATCH_PAIRS = [("double", "sum"), ("short", "max"), ("longdouble", "sum"), ("complexf", "prod")]
BATCH_P = (1, 2, 7, 8, 9, 15, 16, 17, 24, 33, 63, 64)
SETS = [(3, 0, 17), (1, 1, 31), (0, 2, 16), (5, 3, 8), (63, 0, 1)]
OWN_ORDER_TYPES = ["float", "double", "longdouble"]
OWN_SETS = [(0, 0, 2), (0, 0, 5), (0, 0, 9), (0, 0, 17), (0, 0, 64), (1, 1, 9)]
ALIGN_PAIRS = [("short", "max"), ("int", "xor"), ("double", "sum"), ("complexd", "prod")]
SPECIAL = 2                   # kind: oracle.special_sources instead of oracle.sources
LEAD = 32                     # canary bytes before a 16-byte boundary the target is placed from
REGION = LEAD + 32 + SLOT + 48   # a target's buffer (a multiple of 16)

# set (start, log, P); mes: the members the caller plays; own: own_order;
# kind: 0 / 1 of oracle.sources or SPECIAL; tlead: bytes dst sits past a
# 16-byte boundary; t2lead: the same for dst2, None without one; pinned:
# "dst" / "dst2" in page-locked host memory, None: both on the device
Case = namedtuple("Case", "group t op start log P mes n own kind tlead t2lead pinned")


def vec_elems(t):
    return max(1, 16 // ELEM_SIZE[t])


def members(start, log, P):
    return [start + (i << log) for i in range(P)]


def _first_middle_last(start, log, P):
    m = members(start, log, P)
    return tuple(sorted({m[0], m[P // 2], m[-1]}))


def cases():
    out = []

    def add(group, t, op, s, mes, n, own=False, kind=1, tlead=0, t2lead=None, pinned=None):
        out.append(Case(group, t, op, s[0], s[1], s[2], tuple(mes), n, own, kind, tlead, t2lead, pinned))

    # the member loop's batches of 8: one batch short of full, full, one over;
    # two, three, five and eight batches
    for t, op in BATCH_PAIRS:
        for P in BATCH_P:
            for n in (vec_elems(t) + 1, SLOT // ELEM_SIZE[t]):
                add("batches", t, op, (0, 0, P), _first_middle_last(0, 0, P), n)
    # PE_start > 0, strides 1, 2, 4 and 8, the last PE alone
    for t, op in (("double", "sum"), ("int", "xor")):
        for s in SETS:
            add("sets", t, op, s, members(*s), 2 * vec_elems(t) + 1)
    # a partial last word, whole words, a whole slot; the copy threads' second
    # trip (word 768 on) where a slot holds it
    for t, op in (("double", "sum"), ("short", "sum")):
        E, full = vec_elems(t), SLOT // ELEM_SIZE[t]
        ns = {1, E - 1, E, E + 1, 2 * E + 1, full - 1, full}
        ns |= {w * E for w in SECOND_TRIP_WORDS if w * 16 <= SLOT}
        for s in ((0, 0, 3), (0, 0, 9)):
            for n in sorted(k for k in ns if k >= 1):
                add("sizes", t, op, s, (s[0] + 1,), n)
    for t, op in DEVICE_PAIRS:
        for s in ((0, 0, 3), (2, 1, 9)):
            for n in (2 * vec_elems(t) + 1, SLOT // ELEM_SIZE[t]):
                for kind in (0, 1):
                    add("instances", t, op, s, (members(*s)[s[2] // 2],), n, kind=kind)
    # every member in its own order, and every member in PE_start's
    for t in OWN_ORDER_TYPES:
        for op in ("min", "max"):
            for s in OWN_SETS:
                for own in (True, False):
                    add("own", t, op, s, members(*s), 64, own=own, kind=SPECIAL)
    for t in ("float", "double"):
        for op in ("sum", "prod"):
            for P in (3, 9):
                for n in (2 * vec_elems(t) + 1, 64):
                    add("special", t, op, (0, 0, P), (P // 2,), n, kind=SPECIAL)
    # dst 0, 1 and 3 elements past a 16-byte boundary (complexd: 8 bytes past
    # one); dst2 absent, at dst's offset, at another
    for t, op in ALIGN_PAIRS:
        sz = ELEM_SIZE[t]
        for tlead in ((8,) if t == "complexd" else (0, sz, 3 * sz)):
            for t2lead in (None, tlead, tlead + min(sz, 8)):
                for P in (3, 9):
                    for n in (2 * vec_elems(t) + 1, SLOT // sz - 1):
                        add("align", t, op, (0, 0, P), (P - 1,), n, tlead=tlead, t2lead=t2lead)
    # dst page-locked (a host-operand call's bounce buffer); dst on the device
    # and dst2 page-locked (the mirrored heap's settle alias)
    for t, op, own in (("int", "sum", False), ("double", "max", True)):
        for n in (2 * vec_elems(t) + 1, SLOT // ELEM_SIZE[t]):
            add("pinned", t, op, (0, 0, 3), (1,), n, own=own, pinned="dst")
            add("pinned", t, op, (0, 0, 3), (2,), n, own=own, t2lead=0, pinned="dst2")
    return out


def _pick(group, **where):
    return [c for c in cases() if c.group == group and all(getattr(c, k) == v for k, v in where.items())]


# ------------------------------------------------------------ the case lists
def test_service_fold_case_lists(shm):
    """What the GPU tests below claim about their cases, without a GPU."""
    assert all(shm.type_size(t) == sz for t, sz in ELEM_SIZE.items())
    assert REGION % 16 == 0 and NPES * SLOT == 64 * SLOT
    all_cases = cases()
    for c in all_cases:
        sz, m = ELEM_SIZE[c.t], members(c.start, c.log, c.P)
        assert 1 <= c.P <= NPES and c.start >= 0 and 0 <= c.log <= 7 and m[-1] < NPES, c
        assert c.mes and all(me in m for me in c.mes), c
        assert 1 <= c.n and c.n * sz <= SLOT, c
        assert (c.t, c.op) in DEVICE_PAIRS, c
        assert c.tlead % sz in (0, 8) and LEAD + c.tlead + c.n * sz + 48 <= REGION, c
        if c.t2lead is not None:
            assert c.t2lead % min(sz, 8) == 0 and LEAD + c.t2lead + c.n * sz + 48 <= REGION, c
    # member batches: 8k - 1, 8k, 8k + 1 for k = 1, 2, and 64; first, middle, last member
    for t, op in BATCH_PAIRS:
        mine = [c for c in all_cases if c.group == "batches" and (c.t, c.op) == (t, op)]
        Ps = {c.P for c in mine}
        assert Ps == set(BATCH_P)
        assert Ps >= {8 * k + d for k in (1, 2) for d in (-1, 0, 1)} | {64}
        assert {c.n for c in mine} == {vec_elems(t) + 1, SLOT // ELEM_SIZE[t]}
        for c in mine:
            assert (c.start, c.log) == (0, 0) and set(c.mes) == {0, c.P // 2, c.P - 1}
        assert any(me >= 8 for c in mine for me in c.mes)
    sets = [c for c in all_cases if c.group == "sets"]
    assert {(c.t, c.op) for c in sets} == {("double", "sum"), ("int", "xor")}
    for t in ("double", "int"):
        assert {(c.start, c.log, c.P) for c in sets if c.t == t} == set(SETS)
    assert all(list(c.mes) == members(c.start, c.log, c.P) and c.n == 2 * vec_elems(c.t) + 1 for c in sets)
    # sizes: the second-trip words are there exactly when a slot holds them
    for t in ("double", "short"):
        E, full = vec_elems(t), SLOT // ELEM_SIZE[t]
        for s in ((0, 0, 3), (0, 0, 9)):
            ns = {c.n for c in all_cases if c.group == "sizes" and c.t == t and (c.start, c.log, c.P) == s}
            assert ns >= {1, E - 1, E, E + 1, 2 * E + 1, full - 1, full} - {0}
            for w in SECOND_TRIP_WORDS:
                assert (w * E in ns) == (w * 16 <= SLOT), (t, w)
            # nothing reaches copy thread 0's second word before the slot grows
            assert (max(ns) * ELEM_SIZE[t] > COPY_THREADS * 16) == (SLOT > COPY_THREADS * 16)
    assert not any(w * 16 <= 4096 for w in SECOND_TRIP_WORDS)   # none at the 4 KiB slot
    inst = [c for c in all_cases if c.group == "instances"]
    assert {(c.t, c.op) for c in inst} == set(DEVICE_PAIRS)
    for t, op in DEVICE_PAIRS:
        mine = [c for c in inst if (c.t, c.op) == (t, op)]
        assert {(c.start, c.log, c.P, c.n, c.kind) for c in mine} == {
            (s[0], s[1], s[2], n, k) for s in ((0, 0, 3), (2, 1, 9))
            for n in (2 * vec_elems(t) + 1, SLOT // ELEM_SIZE[t]) for k in (0, 1)}
    own = [c for c in all_cases if c.group == "own"]
    assert {(c.t, c.op) for c in own} == {(t, op) for t in OWN_ORDER_TYPES for op in ("min", "max")}
    for t in OWN_ORDER_TYPES:
        for op in ("min", "max"):
            for flag in (True, False):
                mine = [c for c in own if (c.t, c.op, c.own) == (t, op, flag)]
                assert {(c.start, c.log, c.P) for c in mine} == set(OWN_SETS)
    assert {s[2] for s in OWN_SETS if s[:2] == (0, 0)} == {2, 5, 9, 17, 64} and (1, 1, 9) in OWN_SETS
    assert all(list(c.mes) == members(c.start, c.log, c.P) and c.n == 64 and c.kind == SPECIAL for c in own)
    spec = [c for c in all_cases if c.group == "special"]
    assert {(c.t, c.op, c.P) for c in spec} == {(t, op, P) for t in ("float", "double")
                                                 for op in ("sum", "prod") for P in (3, 9)}
    align = [c for c in all_cases if c.group == "align"]
    for t in ("short", "int", "double"):
        sz = ELEM_SIZE[t]
        mine = [c for c in align if c.t == t]
        assert {c.tlead for c in mine} == {0, sz, 3 * sz}
        for tlead in (0, sz, 3 * sz):
            for P in (3, 9):
                for n in (2 * vec_elems(t) + 1, SLOT // sz - 1):
                    t2 = [c.t2lead for c in mine if (c.tlead, c.P, c.n) == (tlead, P, n)]
                    assert len(t2) == 3 and t2[0] is None and t2[1] == tlead and t2[2] % 16 != tlead % 16
    cd = [c for c in align if c.t == "complexd"]
    assert cd and all(c.tlead == 8 for c in cd) and {c.t2lead for c in cd} == {None, 8, 16}
    assert {(c.P, c.n) for c in cd} == {(P, n) for P in (3, 9) for n in (3, SLOT // 16 - 1)}
    pin = [c for c in all_cases if c.group == "pinned"]
    assert {(c.t, c.op, c.pinned, c.t2lead is None) for c in pin} == {
        (t, op, p, p == "dst") for t, op in (("int", "sum"), ("double", "max")) for p in ("dst", "dst2")}
    assert all(c.P == 3 for c in pin)
    assert all(c.pinned is None for c in all_cases if c.group != "pinned")


_LIMIT_CHILD = r"""
import ctypes, sys
L = ctypes.CDLL(sys.argv[1])
slot = int(sys.argv[2])
i, vp, sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
fn = L.shmemx_service_fold_loopback
fn.argtypes = [i, i, i, i, i, i, i, vp, vp, ctypes.POINTER(vp), sz]
fn.restype = i
L.shmemx_type_size.argtypes = [i]
L.shmemx_type_size.restype = sz
srcs = (vp * 3)(64, 64, 64)
for t in range(9):
    esz = L.shmemx_type_size(t)
    print(t, esz, fn(t, 0, 0, 0, 0, 3, 1, 64, None, srcs, slot // esz),
          fn(t, 0, 0, 0, 0, 3, 1, 64, None, srcs, slot // esz + 1),
          fn(t, 0, 0, 0, 0, 3, 1, 64, 64, srcs, 1))
"""


def test_slot_constant_matches_the_library(shm):
    """SLOT is node::kXchgSlotBytes: for every type the hook accepts
    SLOT // size elements and rejects one more with EINVAL.  The accepted
    calls must not run (their addresses are fake), so they are made in a
    process that never called shmem_init and has the service switched off:
    past the argument checks, and before any HIP call, they end in ENOTSUP."""
    r = subprocess.run([sys.executable, "-c", _LIMIT_CHILD, shm.LIB_PATH, str(SLOT)],
                       env=dict(os.environ, SHMEMX_SERVICE="0"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [tuple(int(x) for x in ln.split()) for ln in r.stdout.splitlines()]
    assert len(rows) == len(ELEM_SIZE)
    EINVAL, ENOTSUP = 1, 3
    for name, code in shm.TYPES.items():
        t, esz, at_limit, past_limit, one = rows[code]
        assert (t, esz) == (code, ELEM_SIZE[name])
        assert at_limit == ENOTSUP, (name, "a whole slot of elements was refused", at_limit)
        assert past_limit == EINVAL, (name, "more than a slot of elements was accepted", past_limit)
        assert one == ENOTSUP


# ---------------------------------------------------- references, computed once
_SRC, _WANT = {}, {}


def _rows(oracle, c):
    """The [64, >= n] sources of a case's type and kind: PE q's source is row q."""
    if c.kind == SPECIAL:
        key = (c.t, c.kind, c.n)
        if key not in _SRC:
            _SRC[key] = oracle.special_sources(c.t, NPES, c.n, seed=0x5E7F01D + c.n)
            _SRC[key].flags.writeable = False
        return _SRC[key]
    key = (c.t, c.kind)
    if key not in _SRC:
        _SRC[key] = oracle.sources(c.t, c.kind, NPES, SLOT // ELEM_SIZE[c.t], base_seed=0x5E7F0000)
        _SRC[key].flags.writeable = False
        assert _SRC[key].nbytes == NPES * SLOT
    return _SRC[key]


def _want(oracle, c, me):
    """The oracle's result of PE me (own order) or of PE_start."""
    rows = _rows(oracle, c)
    key = (c.t, c.kind, c.n if c.kind == SPECIAL else 0, c.op, c.start, c.log, c.P)
    if key not in _WANT:
        _WANT[key] = oracle.reduce_sim(c.t, c.op, rows, c.start, c.log, c.P)
        _WANT[key].flags.writeable = False
    return _WANT[key][me if c.own else c.start][:c.n]


def _assert_fold(c, got, want, what):
    if c.kind == SPECIAL and c.op in ("sum", "prod"):
        # the NaN payload an add or a multiply produces is not specified
        nan_w, nan_g = np.isnan(want), np.isnan(got)
        assert np.array_equal(nan_w, nan_g), what
        assert same_bits(got[~nan_g], want[~nan_w]), what
    else:
        assert same_bits(got, want), what


class _Targets:
    """The two target buffers, dst's and dst2's, each on the device or
    page-locked on the host, refilled with 0xA5 before every request."""

    def __init__(self, torch, pinned=None):
        self.torch = torch
        self.a = self._buffer(pinned == "dst")
        self.b = self._buffer(pinned == "dst2")

    def _buffer(self, pinned):
        torch = self.torch
        buf = (torch.empty(REGION, dtype=torch.uint8, pin_memory=True) if pinned
               else torch.empty(REGION, dtype=torch.uint8, device="cuda"))
        assert buf.data_ptr() % 16 == 0
        return buf

    def refill(self):
        self.a.fill_(CANARY)
        self.b.fill_(CANARY)

    def dst(self, tlead):
        return self.a.data_ptr() + LEAD + tlead

    def dst2(self, t2lead):
        return None if t2lead is None else self.b.data_ptr() + LEAD + t2lead

    def images(self):
        return self.a.cpu().numpy().copy(), self.b.cpu().numpy().copy()

    def check(self, what, nbytes, tlead, t2lead):
        """Nothing outside the targets was written, and dst2 (if any) holds
        dst's bytes; returns dst's."""
        a, b = self.images()
        lo = LEAD + tlead
        got = a[lo:lo + nbytes]
        outside = a.copy()
        outside[lo:lo + nbytes] = CANARY
        bad = np.flatnonzero(outside != CANARY)
        assert bad.size == 0, (what, "bytes outside dst were written, first at offsets", bad[:4] - lo)
        if t2lead is None:
            assert (b == CANARY).all(), (what, "a request without dst2 wrote the dst2 buffer")
        else:
            lo2 = LEAD + t2lead
            assert (b[:lo2] == CANARY).all() and (b[lo2 + nbytes:] == CANARY).all(), \
                (what, "bytes outside dst2 were written")
            assert b[lo2:lo2 + nbytes].tobytes() == got.tobytes(), (what, "dst2 differs from dst")
        return got.copy()


def _fold(shm, oracle, tg, c, me):
    """One request of case c as PE me, checked."""
    rows = _rows(oracle, c)
    srcs = [rows[q, :c.n] for q in members(c.start, c.log, c.P)]
    tg.refill()
    shm.service_fold_loopback(c.t, c.op, tg.dst(c.tlead), srcs, c.n, PE_start=c.start, logPE_stride=c.log,
                              me=me, own_order=c.own, dst2=tg.dst2(c.t2lead))
    what = (c._replace(mes=()), me)
    got = tg.check(what, c.n * ELEM_SIZE[c.t], c.tlead, c.t2lead).view(rows.dtype)
    _assert_fold(c, got, _want(oracle, c, me), what)


def _run(torch, shm, oracle, picked):
    """Every member asked for of every case; every request served as a fold."""
    assert picked
    shm.init()
    targets = {}
    before = shm.service_stats()
    requests = 0
    for c in picked:
        tg = targets.get(c.pinned) or targets.setdefault(c.pinned, _Targets(torch, c.pinned))
        for me in c.mes:
            _fold(shm, oracle, tg, c, me)
            requests += 1
    after = shm.service_stats()
    assert after["served"] - before["served"] == requests
    assert after["folds"] - before["folds"] == requests


@gpu
@pytest.mark.parametrize("t,op", BATCH_PAIRS)
def test_fold_member_batches(cuda, shm, oracle, t, op):
    """Sets of 1, 2, 7, 8, 9, 15, 16, 17, 24, 33, 63 and 64 members: the
    member loop's batches of 8 (one short of a batch, a full one, one over, up
    to eight batches), as the first, the middle and the last member, at E + 1
    elements and at a whole slot."""
    import torch
    _run(torch, shm, oracle, _pick("batches", t=t, op=op))


@gpu
def test_fold_strided_and_offset_sets(cuda, shm, oracle):
    """(3,0,17), (1,1,31), (0,2,16), (5,3,8) and (63,0,1) as every member:
    member_at's start and stride, against rows of other seeds all around."""
    import torch
    _run(torch, shm, oracle, _pick("sets"))


@gpu
def test_fold_size_edges(cuda, shm, oracle):
    """1, E - 1, E, E + 1, 2E + 1 elements, one short of a slot and a whole
    slot, of 3 and of 9 members; and 767, 768, 769 and 1537 words once a slot
    holds them."""
    import torch
    _run(torch, shm, oracle, _pick("sizes"))


@gpu
@pytest.mark.parametrize("t", sorted({t for t, _ in DEVICE_PAIRS}))
def test_fold_every_kernel_instance(cuda, shm, oracle, t):
    """Every (type, op) pair over (0,0,3) and (2,1,9) at 2E + 1 elements and a
    whole slot, both kinds of oracle.sources."""
    import torch
    _run(torch, shm, oracle, _pick("instances", t=t))


@gpu
@pytest.mark.parametrize("t", OWN_ORDER_TYPES)
def test_fold_own_order_every_member(cuda, shm, oracle, t):
    """min / max over NaN, +-0 and +-inf at P = 2, 5, 9, 17, 64 and (1,1,9):
    with own_order every member gets its own answer (itself first, then the
    others ascending: reduce_sim(...)[me]), without it PE_start's, whoever
    asks.  The inputs make at least two members' answers differ, so an
    order-blind kernel fails."""
    import torch
    picked = _pick("own", t=t)
    for c in picked:
        if c.own:
            want = {value_bytes(_want(oracle, c, me)) for me in c.mes}
            assert len(want) >= 2, c._replace(mes=())
    _run(torch, shm, oracle, picked)


@gpu
def test_fold_special_values_sum_prod(cuda, shm, oracle):
    """float / double sum and prod over NaN, +-0, +-inf at P = 3 and 9: NaN
    where the oracle has NaN, the same bits elsewhere."""
    import torch
    _run(torch, shm, oracle, _pick("special"))


@gpu
@pytest.mark.parametrize("t,op", ALIGN_PAIRS)
def test_fold_target_alignment(cuda, shm, oracle, t, op):
    """dst at 0, 1 and 3 elements past a 16-byte boundary (complexd: 8 bytes
    past one); dst2 absent, at dst's offset, and at a different one."""
    import torch
    _run(torch, shm, oracle, _pick("align", t=t, op=op))


@gpu
def test_fold_page_locked_targets(cuda, shm, oracle):
    """dst in page-locked host memory (what a host-operand call's bounce
    buffer is), and dst on the device with dst2 page-locked (the mirrored
    heap's settle alias)."""
    import torch
    _run(torch, shm, oracle, _pick("pinned"))


@gpu
def test_300_mixed_requests_on_one_resident_workgroup(cuda, shm, oracle):
    """A one-member copy, a fold of 3 members, a fold of 17 members in own
    order into dst and dst2, a copy again, 300 requests in turn: every result
    right, served up by 300 and folds by exactly the folds, and no request
    carries the one before's cfg (a copy after a fold copies) or dst2 (the
    dst2 buffer stays untouched by the requests without one)."""
    import torch
    shm.init()
    f3 = Case("mixed", "int", "xor", 2, 1, 3, (), 2 * vec_elems("int") + 1, False, 1, 4, None, None)
    f17 = Case("mixed", "double", "max", 3, 0, 17, (), 64, True, SPECIAL, 8, 8, None)
    assert len({value_bytes(_want(oracle, f17, me)) for me in members(3, 0, 17)}) >= 2
    rows = _rows(oracle, Case("mixed", "double", "sum", 0, 0, 1, (), 1, False, 1, 0, None, None))
    dev_rows = torch.from_numpy(rows.copy()).cuda()
    ncopy, tlead = 37, 8
    tg = _Targets(torch)
    torch.cuda.synchronize()
    before = shm.service_stats()
    folds = 0
    for k in range(300):
        kind = k % 4
        if kind == 1:
            _fold(shm, oracle, tg, f3, members(2, 1, 3)[(k // 4) % 3])
            folds += 1
        elif kind == 2:
            _fold(shm, oracle, tg, f17, members(3, 0, 17)[(k // 4) % 17])
            folds += 1
        else:
            q = k % NPES
            tg.refill()
            shm.to_all("double", "sum", tg.dst(tlead), dev_rows[q].data_ptr(), ncopy, 0, 0, 1)
            assert shm.last_error() == 0
            got = tg.check(("copy", k), ncopy * 8, tlead, None).view(np.float64)
            assert same_bits(got, rows[q, :ncopy]), ("copy", k)
    after = shm.service_stats()
    assert after["served"] - before["served"] == 300
    assert after["folds"] - before["folds"] == folds == 150
