"""SIGNAL's fused own-slice kernel (signal_kernels.hip signal_orders2_kernel)
in one process, through shmemx_fused_orders_loopback /
shm.fused_orders_loopback: member m's launch of a P-member set whose sources,
targets and slot areas all live on this GPU, with the peer handshakes looped
back onto the launch's own counters.  The grid barrier, the fences, the
XCD-coverage check, the P-order fold and the gather run for real.

Every launch works on three device buffers: the P sources, the P targets and
the P slot areas (shm.order_slots_bytes each), each array between canary
bytes (0xA5).  Before a launch every target and every slot area holds its own
seeded random bytes.  With [lo(i), hi(i)) the two-shot slices, after member
m's launch all three buffers are compared, whole, with what they must hold:

  tgts[m][lo(m):hi(m)]   the oracle's result of member m there;
  slot k of slots[m]     (k != m, at byte (k < m ? k : k - 1) * slice * size)
                         the oracle's result of member k over [lo(m), hi(m)),
                         and its bytes beyond count(m) elements as before;
  tgts[m][lo(i):hi(i)]   (i != m) the bytes slots[i] held in m's slot;
  every other byte       as before: the other targets, the other slot areas,
                         the canaries, and the sources.

In place (tgts[i] is srcs[i]) there is no target buffer and the source buffer
takes its part.  The sources are oracle.special_sources (NaNs, signed zeros,
infinities), one reduce_sim per (type, op, P, n), sliced; the seed of a case
is the first of its sequence for which the oracle gives at least two members
different results over every launched member's slice, so an order-blind
kernel fails every case (the choice looks at the oracle alone).

The slices and the slot offsets are restated here (slice_bounds, slot_off),
independent of set_geom.h.  The fold moves ONE 16-byte vector per input per
lane, so a block's step is 256 vectors and the 64-block grid's 64 * 256; up to
8 inputs take the MAXIN 8 body, 9 and more the MAXIN 16 one.

orders_cases() builds every case without torch or a GPU;
test_fused_orders_case_lists (no GPU) checks that it holds what the GPU tests
claim.
"""
from collections import namedtuple

import numpy as np
import pytest
from gpu_util import same_bits, value_bytes
from test_gpu_fold import _dev_bytes
from test_gpu_fused import (CANARY, ELEM_SIZE, GRID, KBLOCK, MEM_CAP, _Arrays as _FusedArrays, _Counters,
                            _pick as _pick_fused, _prime as _prime_fused, oneshot_cases, slice_bounds,
                            twoshot_cases, vec_elems)

gpu = pytest.mark.gpu

OWN_PAIRS = [(t, o) for t in ("float", "double", "longdouble") for o in ("min", "max")]
THREE_PAIRS = [("float", "min"), ("double", "max"), ("longdouble", "max")]
PS = (2, 3, 5, 8, 9, 16)
STEP = KBLOCK                  # vectors a block folds per step (one per lane)

# ms: the members launched; tlead / slead: bytes every target / every source
# and slot area sits past a 16-byte boundary; inplace: tgts[i] is srcs[i]
Case = namedtuple("Case", "group t op P n ms tlead slead inplace")


def slice_elems(n, P, sz):
    """Elements of a whole slice: ceil(n / P) rounded up to 16 bytes."""
    g = max(1, 16 // sz)
    return -(-(-(-n // P)) // g) * g


def slot_off(slice_len, sz, owner, k):
    """Byte offset of member k's slot in owner's area: slots of one whole
    slice each, in member order with the owner left out."""
    return (k if k < owner else k - 1) * slice_len * sz


def _some_members(P):
    return tuple(sorted({0, P // 2, P - 1}))


def orders_cases():
    out = []

    def add(group, t, op, P, n, ms, tlead=0, slead=0, inplace=False):
        out.append(Case(group, t, op, P, n, tuple(ms), tlead, slead, inplace))

    # every instance at every member count: slices of exactly s vectors around
    # a block's step; 8 | 9 is the MAXIN split
    for t, op in OWN_PAIRS:
        E = vec_elems(t)
        for P in PS:
            for s in (1, STEP - 1, STEP, STEP + 1):
                add("steps", t, op, P, P * s * E, _some_members(P))
    # the grid's step and a second pass of the vector loop
    for t, op in [(t, o) for t in ("float", "double") for o in ("min", "max")] + [("longdouble", "min")]:
        E = vec_elems(t)
        for P in ((2,) if t == "longdouble" else (2, 9)):
            for s in (GRID * STEP - 1, GRID * STEP, GRID * STEP + 1, GRID * STEP + STEP + 1):
                if t == "longdouble" and s != GRID * STEP + 1:
                    continue
                add("grid", t, op, P, P * s * E, _some_members(P))
    # a scalar tail, a short last slice, a whole slice (and one more element) less
    for t, op in THREE_PAIRS:
        E = vec_elems(t)
        s = STEP + 1
        for P in (3, 9):
            for r in sorted({1, E, E + 1, s * E, s * E + 1}):
                add("short", t, op, P, P * s * E - r, range(P))
    # most members own nothing
    for t, op in THREE_PAIRS:
        for P in (3, 8, 16):
            for n in sorted({1, P - 1, vec_elems(t) * (P - 2) + 1}):
                add("empty", t, op, P, n, range(P))
    # all aligned; sources, slots and targets one element off (the scalar fold,
    # the byte gather); only the targets one element off
    for t, op in (("float", "max"), ("double", "min")):
        sz = ELEM_SIZE[t]
        for P in (3, 16):
            for tlead, slead in ((0, 0), (sz, sz), (sz, 0)):
                add("align", t, op, P, P * (STEP + 1) * vec_elems(t) - 1, _some_members(P), tlead, slead)
    # in place: single launches (a serial replay of members cannot compose in
    # place: member 0's gather overwrites slices later members' folds read)
    for t, op in THREE_PAIRS:
        for P in (3, 9):
            add("inplace", t, op, P, P * (STEP + 1) * vec_elems(t) - 1, range(P), inplace=True)
    # every member once, then every member again: the whole collective
    for t, op in (("float", "max"), ("longdouble", "min")):
        for P in (5, 16):
            add("composed", t, op, P, P * (STEP + 1) * vec_elems(t) - 3, range(P))
    return out


def layout(c):
    """Where a case's arrays sit in its device buffers: array i of the targets
    at byte i * t_stride + t_off (sources and slot areas alike), at least 32
    canary bytes before it and 48 after; and the device bytes the case
    allocates (the buffers, and the staging copy of one while it is uploaded)."""
    sz = ELEM_SIZE[c.t]
    nb = c.n * sz
    lb = (c.P - 1) * slice_elems(c.n, c.P, sz) * sz
    t_stride = -(-(32 + c.tlead + nb + 48) // 16) * 16
    s_stride = -(-(32 + c.slead + nb + 48) // 16) * 16
    l_stride = -(-(32 + c.slead + lb + 48) // 16) * 16
    strides = [s_stride, l_stride] + ([] if c.inplace else [t_stride])
    return {"nbytes": nb, "lbytes": lb, "t_stride": t_stride, "t_off": 32 + c.tlead, "s_stride": s_stride,
            "s_off": 32 + c.slead, "l_stride": l_stride, "l_off": 32 + c.slead,
            "device_bytes": c.P * (sum(strides) + max(strides))}


# ------------------------------------------------------------ the case list
def test_fused_orders_case_lists(shm):
    """What the GPU tests below claim about their cases, without a GPU."""
    cases = orders_cases()
    assert {(c.t, c.op) for c in cases if c.group == "steps"} == set(OWN_PAIRS)
    for t, op in OWN_PAIRS:
        E, sz = vec_elems(t), ELEM_SIZE[t]
        for P in PS:
            got = set()
            for c in [c for c in cases if (c.group, c.t, c.op, c.P) == ("steps", t, op, P)]:
                sl = slice_bounds(c.n, P, sz)
                assert all(hi - lo == sl[0][1] for lo, hi in sl) and sl[0][1] % E == 0
                got.add(sl[0][1] // E)
                assert set(c.ms) == {0, P // 2, P - 1}
            assert got == {1, 255, 256, 257}, (t, op, P, got)
    # both MAXIN bodies
    assert {c.P <= 8 for c in cases} == {True, False} and {8, 9} <= {c.P for c in cases}
    grid = [c for c in cases if c.group == "grid"]
    for t in ("float", "double"):
        for P in (2, 9):
            got = {slice_bounds(c.n, P, ELEM_SIZE[t])[0][1] // vec_elems(t) for c in grid if (c.t, c.P) == (t, P)}
            assert got == {64 * 256 - 1, 64 * 256, 64 * 256 + 1, 64 * 256 + 257}, (t, P, got)
    assert [(c.t, c.P) for c in grid if c.t == "longdouble"] == [("longdouble", 2)]
    assert {c.P for c in grid} == {2, 9}
    empty_own = short_last = tail = 0
    for c in cases:
        sz, E = ELEM_SIZE[c.t], vec_elems(c.t)
        assert shm.type_size(c.t) == sz and (c.t, c.op) in OWN_PAIRS
        assert 2 <= c.P <= 16 and c.n >= 1 and all(0 <= m < c.P for m in c.ms)
        L = layout(c)
        assert L["device_bytes"] <= MEM_CAP, c
        assert L["lbytes"] == shm.order_slots_bytes(c.t, c.P, c.n)
        assert c.tlead % sz == 0 and c.slead % sz == 0
        sl = slice_bounds(c.n, c.P, sz)
        assert sl[0][0] == 0 and sl[-1][1] == c.n and sl[0][1] == min(c.n, slice_elems(c.n, c.P, sz))
        assert all(sl[i][1] == sl[i + 1][0] for i in range(c.P - 1))
        assert all(lo <= hi and (lo == hi or lo % E == 0) for lo, hi in sl)
        counts = [hi - lo for lo, hi in sl]
        nonempty = [k for k in counts if k]
        empty_own += any(counts[m] == 0 for m in c.ms)
        short_last += len(nonempty) > 1 and nonempty[-1] < nonempty[0]
        tail += any(counts[m] % E for m in c.ms)
    assert empty_own and short_last and tail, (empty_own, short_last, tail)
    assert all(set(c.ms) == set(range(c.P)) for c in cases if c.group in ("short", "empty", "inplace", "composed"))
    assert {c.P for c in cases if c.group == "empty"} == {3, 8, 16}
    align = [c for c in cases if c.group == "align"]
    assert {(c.tlead != 0, c.slead != 0) for c in align} == {(False, False), (True, True), (True, False)}
    assert {c.P for c in align} == {3, 16} and {c.t for c in align} == {"float", "double"}
    assert all(c.inplace == (c.group == "inplace") for c in cases)
    assert {c.P for c in cases if c.inplace} == {3, 9}
    assert {(c.t, c.P) for c in cases if c.group == "composed"} == {(t, P) for t in ("float", "longdouble")
                                                                     for P in (5, 16)}


# ---------------------------------------------------- references, computed once
_REF = {}


def _differs(c, want):
    """At least two members' results differ over the slice of every launched
    member that owns one (and over the whole array)."""
    sl = slice_bounds(c.n, c.P, ELEM_SIZE[c.t])
    for lo, hi in [(0, c.n)] + [sl[m] for m in c.ms if sl[m][1] > sl[m][0]]:
        if len({value_bytes(want[k][lo:hi]) for k in range(c.P)}) < 2:
            return False
    return True


def _ref(oracle, c):
    """The case's [P, n] sources and every member's result, [P, n]."""
    key = (c.t, c.op, c.P, c.n)
    if key not in _REF:
        seed0 = 0x0D0E5 + 131 * c.P + 7 * c.n
        for seed in range(seed0, seed0 + 4096):
            srcs = oracle.special_sources(c.t, c.P, c.n, seed=seed)
            want = oracle.reduce_sim(c.t, c.op, srcs, 0, 0, c.P)
            if _differs(c, want):
                break
        else:
            raise AssertionError(f"{c}: no seed makes two members' results differ")
        srcs.flags.writeable = False
        want.flags.writeable = False
        _REF[key] = (srcs, want)
    return _REF[key]


class _Arrays:
    """A case's sources, targets and slot areas on the device, and their host
    images (name -> bytes: "S", "L" and, unless in place, "T")."""

    def __init__(self, torch, oracle, c):
        self.torch, self.c = torch, c
        L = self.L = layout(c)
        self.sz = ELEM_SIZE[c.t]
        self.sl = slice_bounds(c.n, c.P, self.sz)
        self.slice = slice_elems(c.n, c.P, self.sz)
        srcs, self.want = _ref(oracle, c)
        assert _differs(c, self.want), c
        self.dtype = srcs.dtype
        self.tname = "S" if c.inplace else "T"
        self.pre = {"S": np.full(c.P * L["s_stride"], CANARY, np.uint8),
                    "L": np.full(c.P * L["l_stride"], CANARY, np.uint8)}
        if not c.inplace:
            self.pre["T"] = np.full(c.P * L["t_stride"], CANARY, np.uint8)
        for i in range(c.P):
            self.arr(self.pre, "S", i)[:] = np.ascontiguousarray(srcs[i]).view(np.uint8)
            rng = np.random.default_rng(0x0DE75 + 1009 * i + c.n)
            self.arr(self.pre, "L", i)[:] = rng.integers(0, 256, L["lbytes"], dtype=np.uint8)
            if not c.inplace:
                self.arr(self.pre, "T", i)[:] = rng.integers(0, 256, L["nbytes"], dtype=np.uint8)
        self.dev = {k: _dev_bytes(torch, v) for k, v in self.pre.items()}
        self.sptr = [self.dev["S"].data_ptr() + i * L["s_stride"] + L["s_off"] for i in range(c.P)]
        self.lptr = [self.dev["L"].data_ptr() + i * L["l_stride"] + L["l_off"] for i in range(c.P)]
        self.tptr = self.sptr if c.inplace else [self.dev["T"].data_ptr() + i * L["t_stride"] + L["t_off"]
                                                 for i in range(c.P)]
        assert all(p % 16 == c.slead % 16 for p in self.sptr + self.lptr)
        assert all(p % 16 == (c.slead if c.inplace else c.tlead) % 16 for p in self.tptr)
        self.before = {k: v.copy() for k, v in self.pre.items()}   # what the buffers hold now

    def arr(self, images, name, i):
        key = {"S": "s", "T": "t", "L": "l"}[name]
        a = i * self.L[key + "_stride"] + self.L[key + "_off"]
        return images[name][a:a + (self.L["lbytes"] if name == "L" else self.L["nbytes"])]

    def launch(self, shm, m, stream=0):
        c = self.c
        assert shm.fused_orders_loopback(c.t, c.op, self.tptr, self.sptr, self.lptr, c.n, m=m, stream=stream) == 0

    def _folded(self, got_bytes, exp_bytes, want, what):
        """got holds `want`'s values (long double: its 10 value bytes); then
        exp takes got's bytes, so the whole-buffer compare covers the rest."""
        got = got_bytes.copy().view(self.dtype)
        if not same_bits(got, want):
            w = 10 if self.c.t == "longdouble" else self.sz
            bad = np.flatnonzero((got.view(np.uint8).reshape(len(want), -1)[:, :w] !=
                                  np.ascontiguousarray(want).view(np.uint8).reshape(len(want), -1)[:, :w]).any(axis=1))
            raise AssertionError(f"{what}: {bad.size} elements differ from the oracle, first at {bad[:4].tolist()}")
        exp_bytes[:] = got_bytes

    def check(self, m):
        """After member m's launch on buffers that held self.before."""
        c, sz, sl = self.c, self.sz, self.sl
        got = {k: v.cpu().numpy() for k, v in self.dev.items()}
        exp = {k: v.copy() for k, v in self.before.items()}
        lo, hi = sl[m]
        mine = self.arr(exp, self.tname, m)
        # the other owners' slots for m, as they were
        for i, (a, b) in enumerate(sl):
            if i != m and b > a:
                off = slot_off(self.slice, sz, i, m)
                mine[a * sz:b * sz] = self.arr(self.before, "L", i)[off:off + (b - a) * sz]
        # m's own order into its target, the other orders into its slots
        self._folded(self.arr(got, self.tname, m)[lo * sz:hi * sz], mine[lo * sz:hi * sz],
                     self.want[m][lo:hi], (c, m, "target"))
        for k in range(c.P):
            if k != m:
                off = slot_off(self.slice, sz, m, k)
                self._folded(self.arr(got, "L", m)[off:off + (hi - lo) * sz],
                             self.arr(exp, "L", m)[off:off + (hi - lo) * sz], self.want[k][lo:hi],
                             (c, m, f"slot of member {k}"))
        for name in got:
            if not np.array_equal(got[name], exp[name]):
                key = {"S": "s", "T": "t", "L": "l"}[name]
                bad = np.flatnonzero(got[name] != exp[name])
                where = [(int(b) // self.L[key + "_stride"], int(b) % self.L[key + "_stride"] - self.L[key + "_off"])
                         for b in bad[:4]]
                raise AssertionError(f"{(c, m)}: {bad.size} bytes of buffer {name} differ, first at "
                                     f"(array, byte offset) {where}")
        self.before = got

    def refill(self, m):
        """Target m and slot area m back to their seeded bytes (in place: the
        source m, which is the target); the others are unchanged."""
        for name in (self.tname, "L"):
            key = {"S": "s", "T": "t", "L": "l"}[name]
            a = m * self.L[key + "_stride"] + self.L[key + "_off"]
            fresh = self.arr(self.pre, name, m)
            self.dev[name][a:a + fresh.size] = self.torch.from_numpy(fresh.copy()).cuda()
            self.arr(self.before, name, m)[:] = fresh


def _run(torch, shm, oracle, cases):
    """Every member of every case, each launch on freshly filled arrays."""
    assert cases
    counters = _Counters(shm)
    for c in cases:
        arr = _Arrays(torch, oracle, c)
        for m in c.ms:
            arr.launch(shm, m)
            counters.launches += 1
            arr.check(m)
            arr.refill(m)
        del arr
    counters.check()


def _pick(group, **where):
    return [c for c in orders_cases() if c.group == group and all(getattr(c, k) == v for k, v in where.items())]


# ------------------------------------------------------------------ the tests
@gpu
@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("t", ["float", "double", "longdouble"])
def test_orders_every_instance_and_member_count(cuda, shm, oracle, t, P):
    """min and max at slices of 1, 255, 256 and 257 vectors (a block's step at
    one vector per lane), members 0, P // 2 and P - 1; P = 8 | 9 is the MAXIN
    split."""
    import torch
    _run(torch, shm, oracle, _pick("steps", t=t, P=P))


@gpu
@pytest.mark.parametrize("t,P", [("float", 2), ("float", 9), ("double", 2), ("double", 9), ("longdouble", 2)])
def test_orders_grid_step_and_second_pass(cuda, shm, oracle, t, P):
    """Slices of 64 * 256 - 1, 64 * 256, 64 * 256 + 1 and 64 * 256 + 257
    vectors: the grid's step and a second pass of the vector loop (long
    double: the one slice of 64 * 256 + 1)."""
    import torch
    _run(torch, shm, oracle, _pick("grid", t=t, P=P))


@gpu
@pytest.mark.parametrize("P", [3, 9])
def test_orders_short_slices(cuda, shm, oracle, P):
    """n short of P slices of 257 vectors by 1 element (a scalar tail in the
    last slice and a byte tail in its gather), a vector, a vector and an
    element, a whole slice, and a slice and an element; every member."""
    import torch
    _run(torch, shm, oracle, _pick("short", P=P))


@gpu
def test_orders_mostly_empty_slices(cuda, shm, oracle):
    """1, P - 1 and E (P - 2) + 1 elements over 3, 8 and 16 members: most own
    nothing, and every member is launched, those with an empty slice too."""
    import torch
    _run(torch, shm, oracle, _pick("empty"))


@gpu
@pytest.mark.parametrize("P", [3, 16])
def test_orders_alignment(cuda, shm, oracle, P):
    """Every array 16-byte aligned; sources, slots and targets one element
    off (the scalar fold, the byte gather); only the targets one element off."""
    import torch
    _run(torch, shm, oracle, _pick("align", P=P))


@gpu
@pytest.mark.parametrize("P", [3, 9])
def test_orders_in_place_single_launches(cuda, shm, oracle, P):
    """tgts[i] is srcs[i]: output m of the fold aliases input m exactly; every
    member alone, on fresh sources."""
    import torch
    _run(torch, shm, oracle, _pick("inplace", P=P))


@gpu
@pytest.mark.parametrize("P", [5, 16])
def test_orders_composed_collective(cuda, shm, oracle, P):
    """Members 0..P-1 once each (every owner's slots are then final), then all
    of them again: every target holds its own member's whole oracle result."""
    import torch
    cases = _pick("composed", P=P)
    assert cases
    counters = _Counters(shm)
    for c in cases:
        arr = _Arrays(torch, oracle, c)
        for _ in range(2):
            for m in c.ms:
                arr.launch(shm, m)
                counters.launches += 1
                arr.check(m)     # against what the buffers held before this launch
        got = {"T": arr.dev["T"].cpu().numpy()}
        for k in range(c.P):
            assert same_bits(arr.arr(got, "T", k).copy().view(arr.dtype), arr.want[k]), (c, k)
    counters.check()


@gpu
def test_200_mixed_launches_on_one_stream(cuda, shm, oracle):
    """This kernel in turn with the existing fused one shot and two shot
    (shmemx_fused_loopback) on one stream, 200 launches: the shared grid
    barrier's self-resetting counter and its generation hold, and every result
    is right."""
    import torch
    one, two = oneshot_cases(), twoshot_cases()
    fused = [_pick_fused(one, "counts", t="double", P=5, n=700)[0],
             _pick_fused(two, "short", t="double", P=5)[0],
             _pick_fused(one, "own", t="float", n=1500)[0],
             _pick_fused(two, "steps", t="short", P=9)[3]]
    _prime_fused(oracle, fused)
    mine = [_pick("short", t="float", P=9)[0], _pick("steps", t="longdouble", P=3)[3],
            _pick("inplace", t="double", P=3)[0], _pick("empty", t="double", P=8)[1]]
    arrs = []
    for a, b in zip(mine, fused):
        arrs += [_Arrays(torch, oracle, a), _FusedArrays(torch, oracle, b)]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    counters = _Counters(shm)
    for k in range(200):
        arr = arrs[k % len(arrs)]
        m = (k // len(arrs)) % arr.c.P
        arr.launch(shm, m, stream=stream.cuda_stream)
        counters.launches += 1
        arr.check(m)
        arr.refill(m)
        torch.cuda.synchronize()
    counters.check()
