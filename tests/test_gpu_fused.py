"""The fused one-shot and two-shot kernels (signal_kernels.hip
signal_fold_kernel / signal_fold2_kernel) and the unfused device barrier, in
one process, through shmemx_fused_loopback / shm.fused_loopback: member m's
launch of a P-member set whose members' arrays all live on this GPU, with the
peer handshakes looped back onto the launch's own counters.  The grid barrier,
the fences, the XCD-coverage check, the fold and the gather run for real.

Every launch works on two device buffers: one holds the P sources, one the P
targets, each array between canary bytes (0xA5).  Before a launch every target
holds its own seeded random bytes.  After member m's launch the whole target
buffer is compared with what it must hold:

  one shot   tgts[m] = the oracle's fold of every whole source (set order:
             reduce_sim(...)[0]; own order: reduce_sim(...)[m]);
  two shot   tgts[m][lo(m):hi(m)] = the oracle's fold over that range, and
             tgts[m][lo(i):hi(i)] = the bytes tgts[i] held there, for i != m;
  both       every other byte (the other members' targets, the canaries) as
             before, and the source buffer unchanged.

The fold is element-wise and oracle.sources(..., n)[p] is a prefix of
oracle.sources(..., n')[p] for n' > n, so one reduce_sim per (type, op, P,
kind) over the longest array, sliced, is the reference of every case.

The slices lo/hi are restated here (slice_bounds), independent of set_geom.h.
A 64-block grid of 256 lanes folds U = 4 / 2 / 1 vectors per lane per step
for up to 4 / 8 / 16 inputs, so a block's step is 256 U vectors and the
grid's 64 * 256 U.

oneshot_cases() and twoshot_cases() build every case without torch or a GPU;
test_fused_case_lists (no GPU) checks that they hold what the GPU tests claim.
"""
from collections import namedtuple

import numpy as np
import pytest
from gpu_util import same_bits, value_bytes
from test_gpu_fold import DEVICE_PAIRS, _dev_bytes

gpu = pytest.mark.gpu

CANARY = 0xA5
KBLOCK = 256                  # lanes per block
GRID = 64                     # blocks of a fused launch
TINY = 4 * KBLOCK             # kFusedTinyElems: one block folds alone up to here
MAX_IN = 16                   # kMaxFoldInputs
MEM_CAP = 256 << 20           # device bytes one case may allocate
ELEM_SIZE = {"short": 2, "int": 4, "long": 8, "longlong": 8, "float": 4, "double": 8,
             "longdouble": 16, "complexd": 16, "complexf": 8}
TWOSHOT_PU = [(2, 4), (3, 4), (4, 4), (5, 2), (6, 2), (8, 2), (9, 1), (12, 1), (16, 1)]
LIGHT_PAIRS = [("double", "sum"), ("short", "max")]
HEAVY_PAIRS = [("longdouble", "sum"), ("complexd", "prod"), ("complexf", "prod")]
OWN_ORDER_TYPES = ["float", "double", "longdouble"]
SPECIAL = 2                   # kind: oracle.special_sources instead of oracle.sources

# schedule 0 one shot / 1 two shot; ms: the members launched; own: own order;
# kind: 0 / 1 of oracle.sources or SPECIAL; tlead / slead: bytes every target /
# source sits past a 16-byte boundary
Case = namedtuple("Case", "group schedule t op P n ms own kind tlead slead")


def vec_elems(t):
    return max(1, 16 // ELEM_SIZE[t])


def unroll(P):
    return 4 if P <= 4 else 2 if P <= 8 else 1


def slice_bounds(n, P, sz):
    """[lo(i), hi(i)) of the two-shot slices: ceil(n / P) elements rounded up
    to whole 16-byte granules each."""
    g = max(1, 16 // sz)
    per = -(-n // P)
    sl = -(-per // g) * g
    return [(min(n, i * sl), min(n, (i + 1) * sl)) for i in range(P)]


def _some_members(P):
    return tuple(sorted({0, P // 2, P - 1}))


def oneshot_cases():
    out = []

    def add(group, t, op, P, n, ms=(0,), own=False, kind=1, tlead=0, slead=0):
        out.append(Case(group, 0, t, op, P, n, tuple(ms), own, kind, tlead, slead))

    # the tiny path, its boundary, one and two wraps of the 64 x 256-lane grid
    for n in (1, 2, 255, 256, 257, 1023, 1024, 1025, 16383, 16384, 16385, 32769):
        add("sizes", "double", "sum", 3, n, ms=(1,))
    # every input count: the register-array path of fold_elem, and the loop
    for n in (700, 1500):
        for t, op in LIGHT_PAIRS:
            for nins in range(1, MAX_IN + 1):
                add("counts", t, op, nins, n, ms=(nins // 2,))
        for t, op in (("longdouble", "sum"), ("complexd", "prod")):
            for nins in (1, 2, 9, 16):
                add("counts", t, op, nins, n, ms=(nins // 2,))
    for t, op in DEVICE_PAIRS:
        for n in (700, 16385):
            for kind in (0, 1):
                add("instances", t, op, 3, n, ms=(2,), kind=kind)
    for t in OWN_ORDER_TYPES:
        for op in ("min", "max"):
            for n in (700, 1500):
                add("own", t, op, 5, n, ms=range(5), own=True, kind=SPECIAL)
    for t in ("float", "double"):
        for op in ("sum", "prod"):
            for n in (700, 1500):
                add("special", t, op, 3, n, ms=(0,), kind=SPECIAL)
    for t, op in (("short", "sum"), ("int", "sum"), ("double", "sum")):
        for n in (700, 1500):
            add("align", t, op, 3, n, ms=(1,), tlead=3 * ELEM_SIZE[t], slead=ELEM_SIZE[t])
    return out


def twoshot_cases():
    out = []

    def add(group, t, op, P, n, ms, tlead=0, slead=0):
        out.append(Case(group, 1, t, op, P, n, tuple(ms), False, 1, tlead, slead))

    for P, U in TWOSHOT_PU:
        step = KBLOCK * U
        for t, op in LIGHT_PAIRS:
            E = vec_elems(t)
            # slices of exactly s vectors around fold_vecs' block step ...
            svals = [1, step - 1, step, step + 1, 2 * step + 1]
            if P in (2, 5, 16):   # ... the grid's step, and a second pass of the main loop
                svals += [GRID * step - 1, GRID * step, GRID * step + 1, GRID * step + step + 1]
            for s in svals:
                add("steps", t, op, P, P * s * E, _some_members(P))
            # a scalar tail, a short last slice, a whole slice (and one more element) less
            s = step + 1
            for r in (1, E, E + 1, s * E, s * E + 1):
                add("short", t, op, P, P * s * E - r, range(P))
    # most members own nothing
    for P in (3, 8, 16):
        for t, op in LIGHT_PAIRS:
            for n in sorted({1, P - 1, vec_elems(t) * (P - 2) + 1}):
                add("empty", t, op, P, n, range(P))
    # the v += nthr loop of the heavy ops
    for t, op in HEAVY_PAIRS:
        for P in (3, 9):
            for s in (1, 255, 256, 257, GRID * KBLOCK + 1):
                add("heavy", t, op, P, P * s * vec_elems(t), _some_members(P))
    # all aligned; all one element off (fold_span's scalar path, gather_span's
    # byte path); sources aligned and targets one element off
    for P in (3, 16):
        s = KBLOCK * unroll(P) + 1
        for t, op in (("short", "max"), ("int", "xor"), ("double", "sum")):
            sz = ELEM_SIZE[t]
            for tlead, slead in ((0, 0), (sz, sz), (sz, 0)):
                add("align", t, op, P, P * s * vec_elems(t) - 1, _some_members(P), tlead, slead)
    # every member once, then every member again: the whole collective
    for P in (5, 16):
        for t, op in (("double", "sum"), ("int", "xor")):
            add("composed", t, op, P, P * (KBLOCK * unroll(P) + 1) * vec_elems(t) - 3, range(P))
    return out


def layout(c):
    """Where a case's arrays sit in its two device buffers: array i of the
    targets at byte i * t_stride + t_off (sources alike), at least 32 canary
    bytes before it and 48 after; and the device bytes the case allocates
    (both buffers, and the staging copy of one while it is uploaded)."""
    nb = c.n * ELEM_SIZE[c.t]
    t_stride = -(-(32 + c.tlead + nb + 48) // 16) * 16
    s_stride = -(-(32 + c.slead + nb + 48) // 16) * 16
    return {"nbytes": nb, "t_stride": t_stride, "t_off": 32 + c.tlead, "s_stride": s_stride,
            "s_off": 32 + c.slead,
            "device_bytes": c.P * (t_stride + s_stride) + c.P * max(t_stride, s_stride)}


# ------------------------------------------------------------ the case lists
def test_fused_case_lists(shm):
    """What the GPU tests below claim about their cases, without a GPU."""
    assert all(shm.type_size(t) == sz for t, sz in ELEM_SIZE.items())
    one, two = oneshot_cases(), twoshot_cases()
    for t, op in LIGHT_PAIRS:
        assert {c.P for c in one if c.group == "counts" and (c.t, c.op) == (t, op)} == set(range(1, 17))
    assert {c.n for c in one if c.group == "sizes"} >= {1024, 1025, 16383, 16384, 16385, 32769}
    assert {(c.t, c.op) for c in one if c.group == "instances"} == set(DEVICE_PAIRS)
    assert all(set(c.ms) == set(range(c.P)) for c in one if c.group == "own")
    empty = short_last = tail = 0
    for P, U in TWOSHOT_PU:
        assert unroll(P) == U
        for t, op in LIGHT_PAIRS:
            E = vec_elems(t)
            mine = [c for c in two if (c.t, c.op, c.P) == (t, op, P) and c.group == "steps"]
            got = set()
            for c in mine:
                sl = slice_bounds(c.n, P, ELEM_SIZE[t])
                assert all(hi - lo == sl[0][1] for lo, hi in sl) and sl[0][1] % E == 0
                got.add(sl[0][1] // E)
            assert got >= {256 * U - 1, 256 * U, 256 * U + 1}, (P, t, got)
            if P in (2, 5, 16):
                assert got >= {64 * 256 * U - 1, 64 * 256 * U, 64 * 256 * U + 1}
    for c in one + two:
        assert c.P >= 1 and c.P <= MAX_IN and c.n >= 1 and all(0 <= m < c.P for m in c.ms)
        assert layout(c)["device_bytes"] <= MEM_CAP, c
        assert c.tlead % ELEM_SIZE[c.t] == 0 and c.slead % ELEM_SIZE[c.t] == 0
    for c in two:
        sz, E = ELEM_SIZE[c.t], vec_elems(c.t)
        sl = slice_bounds(c.n, c.P, sz)
        # disjoint, in order, covering [0, n); every non-empty slice starts on
        # a 16-byte granule of the array
        assert sl[0][0] == 0 and sl[-1][1] == c.n
        assert all(sl[i][1] == sl[i + 1][0] for i in range(c.P - 1))
        assert all(lo <= hi and (lo == hi or lo % E == 0) for lo, hi in sl)
        counts = [hi - lo for lo, hi in sl]
        nonempty = [k for k in counts if k]
        empty += 0 in counts
        short_last += len(nonempty) > 1 and nonempty[-1] < nonempty[0]
        tail += any(k % E for k in counts)
    assert empty and short_last and tail, (empty, short_last, tail)
    # an empty own slice is launched too
    assert any(slice_bounds(c.n, c.P, ELEM_SIZE[c.t])[m][0] == slice_bounds(c.n, c.P, ELEM_SIZE[c.t])[m][1]
               for c in two for m in c.ms)


# ---------------------------------------------------- references, computed once
_SRC, _WANT = {}, {}


def _sources(oracle, c):
    """The case's [P, n] sources: rows of one shared, read-only array per
    (type, kind) (special values: per shape, they are no prefix of each other)."""
    if c.kind == SPECIAL:
        key = (c.t, c.kind, c.P, c.n)
        if key not in _SRC:
            _SRC[key] = oracle.special_sources(c.t, c.P, c.n, seed=0xF05ED + 131 * c.P + c.n)
            _SRC[key].flags.writeable = False
        return _SRC[key]
    key = (c.t, c.kind)
    have = _SRC.get(key)
    if have is None or have.shape[1] < c.n:
        have = oracle.sources(c.t, c.kind, MAX_IN, c.n, base_seed=0xF05ED000)
        have.flags.writeable = False
        _SRC[key] = have
        for k in [k for k in _WANT if k[:2] == key]:
            del _WANT[k]
    return have[:c.P, :c.n]


def _want(oracle, c, m):
    """The oracle's result of member m (own order) or PE_start (set order)."""
    srcs = _sources(oracle, c)
    if c.kind == SPECIAL:
        key = (c.t, c.kind, c.op, c.P, c.n)
        if key not in _WANT:
            _WANT[key] = oracle.reduce_sim(c.t, c.op, srcs, 0, 0, c.P)
        return _WANT[key][m if c.own else 0]
    key = (c.t, c.kind, c.op, c.P)
    have = _WANT.get(key)
    if have is None or have.shape[1] < c.n:
        full = _SRC[(c.t, c.kind)]
        have = _WANT[key] = oracle.reduce_sim(c.t, c.op, full[:c.P], 0, 0, c.P)
    return have[m if c.own else 0][:c.n]


def _prime(oracle, cases):
    """Sources and references at the longest n of each key first, so that the
    shared arrays are computed once."""
    for c in sorted(cases, key=lambda c: -c.n):
        _want(oracle, c, 0)


def _assert_fold(c, got, want, what):
    if c.kind == SPECIAL and c.op in ("sum", "prod"):
        # the NaN payload an add or a multiply produces is not specified
        nan_w, nan_g = np.isnan(want), np.isnan(got)
        assert np.array_equal(nan_w, nan_g), what
        assert same_bits(got[~nan_g], want[~nan_w]), what
    else:
        assert same_bits(got, want), what


class _Counters:
    """One XCD-coverage check per launch, none incomplete (direct_stats)."""

    def __init__(self, shm):
        self.shm, self.launches = shm, 0
        self.before = shm.direct_stats(reset=False)

    def check(self):
        after = self.shm.direct_stats(reset=False)
        assert after["fences_device"] - self.before["fences_device"] == self.launches
        assert after["fences_device_incomplete"] - self.before["fences_device_incomplete"] == 0


class _Arrays:
    """A case's sources and targets on the device, and their host images."""

    def __init__(self, torch, oracle, c):
        self.torch, self.oracle, self.c = torch, oracle, c
        L = self.L = layout(c)
        self.dtype = _sources(oracle, c).dtype
        srcs = _sources(oracle, c)
        self.s_host = np.full(c.P * L["s_stride"], CANARY, np.uint8)
        self.t_pre = np.full(c.P * L["t_stride"], CANARY, np.uint8)
        for i in range(c.P):
            self._src(self.s_host, i)[:] = np.ascontiguousarray(srcs[i]).view(np.uint8)
            rng = np.random.default_rng(0x7A56E7 + 1009 * i + c.n)
            self._tgt(self.t_pre, i)[:] = rng.integers(0, 256, L["nbytes"], dtype=np.uint8)
        self.S = _dev_bytes(torch, self.s_host)
        self.T = _dev_bytes(torch, self.t_pre)
        self.sptr = [self.S.data_ptr() + i * L["s_stride"] + L["s_off"] for i in range(c.P)]
        self.tptr = [self.T.data_ptr() + i * L["t_stride"] + L["t_off"] for i in range(c.P)]
        assert all(p % 16 == c.slead % 16 for p in self.sptr)
        assert all(p % 16 == c.tlead % 16 for p in self.tptr)
        self.before = self.t_pre.copy()   # what the target buffer holds now

    def _src(self, image, i):
        a = i * self.L["s_stride"] + self.L["s_off"]
        return image[a:a + self.L["nbytes"]]

    def _tgt(self, image, i):
        a = i * self.L["t_stride"] + self.L["t_off"]
        return image[a:a + self.L["nbytes"]]

    def launch(self, shm, m, stream=0):
        c = self.c
        err = shm.fused_loopback(c.t, c.op, c.schedule, self.tptr, self.sptr, c.n, m=m,
                                 own_order=c.own, stream=stream)
        assert err == 0

    def check(self, m):
        """After member m's launch on a target buffer that held self.before."""
        c, sz = self.c, ELEM_SIZE[self.c.t]
        what = (c, m)
        got = self.T.cpu().numpy()
        exp = self.before.copy()
        mine = self._tgt(exp, m)
        lo, hi = 0, c.n
        if c.schedule == 1:
            sl = slice_bounds(c.n, c.P, sz)
            lo, hi = sl[m]
            for i, (a, b) in enumerate(sl):
                if i != m:
                    mine[a * sz:b * sz] = self._tgt(self.before, i)[a * sz:b * sz]
        folded = self._tgt(got, m)[lo * sz:hi * sz].copy().view(self.dtype)
        _assert_fold(c, folded, _want(self.oracle, c, m)[lo:hi], what)
        mine[lo * sz:hi * sz] = self._tgt(got, m)[lo * sz:hi * sz]
        if not np.array_equal(got, exp):
            bad = np.flatnonzero(got != exp)
            where = [(int(b) // self.L["t_stride"], int(b) % self.L["t_stride"] - self.L["t_off"])
                     for b in bad[:4]]
            raise AssertionError(f"{what}: {bad.size} target-buffer bytes differ, first at "
                                 f"(array, byte offset) {where}")
        assert np.array_equal(self.S.cpu().numpy(), self.s_host), (what, "a source changed")
        self.before = got

    def refill(self, m):
        """Target m back to its seeded bytes (the others are unchanged)."""
        a = m * self.L["t_stride"] + self.L["t_off"]
        self.T[a:a + self.L["nbytes"]] = self.torch.from_numpy(self._tgt(self.t_pre, m).copy()).cuda()
        self._tgt(self.before, m)[:] = self._tgt(self.t_pre, m)


def _run(torch, shm, oracle, cases):
    """Every member of every case, each launch on freshly filled targets."""
    assert cases
    _prime(oracle, cases)
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


def _pick(cases, group, **where):
    return [c for c in cases if c.group == group and all(getattr(c, k) == v for k, v in where.items())]


# ------------------------------------------------------------------ one shot
@gpu
def test_oneshot_size_edges(cuda, shm, oracle):
    """double sum of 3 inputs at 1, 2, 255..257, 1023..1025 (the last size one
    block folds alone, and the first the grid folds), 16383..16385 (the
    64 x 256-lane grid wraps once) and 32769 (twice).  Up to 1024 elements the
    kernel stores the host signal itself, and the hook fails without it."""
    import torch
    _run(torch, shm, oracle, _pick(oneshot_cases(), "sizes"))


@gpu
@pytest.mark.parametrize("t,op", LIGHT_PAIRS + [("longdouble", "sum"), ("complexd", "prod")])
def test_oneshot_every_input_count(cuda, shm, oracle, t, op):
    """1..16 inputs (fold_elem's register array and its k < nins predicates),
    and 1, 2, 9 and 16 for the heavy ops' loop; 700 (tiny) and 1500 elements."""
    import torch
    _run(torch, shm, oracle, _pick(oneshot_cases(), "counts", t=t, op=op))


@gpu
@pytest.mark.parametrize("t", sorted({t for t, _ in DEVICE_PAIRS}))
def test_oneshot_every_kernel_instance(cuda, shm, oracle, t):
    """Every (type, op) pair with 3 inputs at 700 and 16385 elements, both
    kinds of oracle.sources."""
    import torch
    _run(torch, shm, oracle, _pick(oneshot_cases(), "instances", t=t))


@gpu
@pytest.mark.parametrize("t", OWN_ORDER_TYPES)
def test_oneshot_own_order_every_member(cuda, shm, oracle, t):
    """min / max over NaN, +-0 and +-inf, each member in its own order (m
    first, then the others ascending) against reduce_sim(...)[m]; the inputs
    make at least two members' results differ, so an order-blind kernel fails."""
    import torch
    cases = _pick(oneshot_cases(), "own", t=t)
    for c in cases:
        want = [value_bytes(_want(oracle, c, m)) for m in range(c.P)]
        assert len(set(want)) >= 2, c
    _run(torch, shm, oracle, cases)


@gpu
def test_oneshot_special_values_sum_prod(cuda, shm, oracle):
    """float / double sum and prod over NaN, +-0, +-inf: NaN where the oracle
    has NaN, the same bits elsewhere."""
    import torch
    _run(torch, shm, oracle, _pick(oneshot_cases(), "special"))


@gpu
def test_oneshot_element_alignment(cuda, shm, oracle):
    """Targets 3 elements and sources 1 element past a 16-byte boundary."""
    import torch
    _run(torch, shm, oracle, _pick(oneshot_cases(), "align"))


# ------------------------------------------------------------------ two shot
@gpu
@pytest.mark.parametrize("P,U", TWOSHOT_PU)
def test_twoshot_step_edges(cuda, shm, oracle, P, U):
    """Slices of 1, 256U - 1, 256U, 256U + 1 and 2 * 256U + 1 vectors (a
    block's step of fold_vecs<.., 4 / 8 / 16> and gather_vecs<4 / 8 / 16>: the
    full-step loop against the last partial step), and at P = 2, 5, 16 of
    64 * 256U - 1, 64 * 256U, 64 * 256U + 1 and 64 * 256U + 256U + 1 (the
    grid's step, a second pass), for members 0, P // 2 and P - 1."""
    import torch
    _run(torch, shm, oracle, _pick(twoshot_cases(), "steps", P=P))


@gpu
@pytest.mark.parametrize("P,U", TWOSHOT_PU)
def test_twoshot_short_slices(cuda, shm, oracle, P, U):
    """n short of P slices of 256U + 1 vectors by 1 element (a scalar tail in
    the last slice and a byte tail in its gather), a vector, a vector and an
    element, a whole slice, and a slice and an element; every member."""
    import torch
    _run(torch, shm, oracle, _pick(twoshot_cases(), "short", P=P))


@gpu
def test_twoshot_mostly_empty_slices(cuda, shm, oracle):
    """1, P - 1 and E (P - 2) + 1 elements over 3, 8 and 16 members: most own
    nothing, and every member is launched, those with an empty slice too."""
    import torch
    _run(torch, shm, oracle, _pick(twoshot_cases(), "empty"))


@gpu
@pytest.mark.parametrize("t,op", HEAVY_PAIRS)
def test_twoshot_heavy_ops(cuda, shm, oracle, t, op):
    """The one-vector-at-a-time loop of the soft x87 and the complex products:
    slices of 1, 255, 256, 257 and 64 * 256 + 1 vectors at P = 3 and 9."""
    import torch
    _run(torch, shm, oracle, _pick(twoshot_cases(), "heavy", t=t, op=op))


@gpu
@pytest.mark.parametrize("P", [3, 16])
def test_twoshot_alignment(cuda, shm, oracle, P):
    """Every array 16-byte aligned; every array one element off (fold_span's
    scalar path, gather_span's byte path); only the targets one element off."""
    import torch
    _run(torch, shm, oracle, _pick(twoshot_cases(), "align", P=P))


@gpu
@pytest.mark.parametrize("P", [5, 16])
def test_twoshot_composed_collective(cuda, shm, oracle, P):
    """Members 0..P-1 once each (every slice is then final in its owner), then
    all of them again: every target holds the oracle's whole result."""
    import torch
    cases = _pick(twoshot_cases(), "composed", P=P)
    assert cases
    counters = _Counters(shm)
    for c in cases:
        arr = _Arrays(torch, oracle, c)
        for _ in range(2):
            for m in c.ms:
                arr.launch(shm, m)
                counters.launches += 1
                arr.check(m)     # against what the buffer held before this launch
        got = arr.T.cpu().numpy()
        want = _want(oracle, c, 0)
        for i in range(c.P):
            assert same_bits(arr._tgt(got, i).copy().view(arr.dtype), want), (c, i)
    counters.check()


# ------------------------------------------- the barrier, the coverage check
@gpu
@pytest.mark.parametrize("P", [1, 2, 16])
def test_unfused_barrier_alone(cuda, shm, P):
    """launch_sys_fence + launch_signal ten times: OK, error word 0, ten
    coverage checks, none incomplete."""
    counters = _Counters(shm)
    for _ in range(10):
        assert shm.fused_loopback("double", "sum", 2, [0] * P, [0] * P, 0) == 0
        counters.launches += 1
    counters.check()


@gpu
def test_300_mixed_launches_on_one_stream(cuda, shm, oracle):
    """Tiny and grid one shots and two shots in turn on one stream, 300
    launches: the grid barrier's self-resetting counter and its generation
    hold, and every result is right."""
    import torch
    cases = [_pick(oneshot_cases(), "counts", t="double", P=5, n=700)[0],
             _pick(twoshot_cases(), "short", t="double", P=5)[0],
             _pick(oneshot_cases(), "counts", t="short", P=12, n=1500)[0],
             _pick(twoshot_cases(), "steps", t="short", P=9)[3],
             _pick(oneshot_cases(), "own", t="float", n=1500)[0],
             _pick(twoshot_cases(), "heavy", t="complexf", P=3)[3]]
    _prime(oracle, cases)
    arrs = [_Arrays(torch, oracle, c) for c in cases]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    counters = _Counters(shm)
    for k in range(300):
        arr = arrs[k % len(arrs)]
        m = (k // len(arrs)) % arr.c.P
        arr.launch(shm, m, stream=stream.cuda_stream)
        counters.launches += 1
        arr.check(m)
        arr.refill(m)
        torch.cuda.synchronize()
    counters.check()
