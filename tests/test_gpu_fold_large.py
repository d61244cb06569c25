"""The fold family (csrc/fold_kernels.hip) at production sizes: every
non-temporal instance, and the all-scalar path past one trip of its grid.

A call that moves 32 MiB or more runs the NT = 3 twin of its kernel (span16.h
nt_policy), and a call whose arrays differ mod 16 runs all scalar on at most
2048 workgroups, so from 2048 x 256 + 1 elements its grid-stride loop takes a
second trip.  The other fold tests stay below both.

large_cases() lays every launch out without torch or a GPU: route, type, op,
P, n and every array's address mod 16.  test_large_case_list_reaches_every_instance
(no GPU) asks the library which instance and grid each case launches
(shmemx_fold_launch_shape: the launch's own choice, from the addresses mod 16)
and compares the union with the dispatch table restated here: all 183 reachable
NT = 3 instances, every vector case with head, tail, whole chunks and a partial
one, the twins one element below the cut, two and three scalar trips.  So a
case that stops reaching its instance (somebody moves the cut, or a route's
choice) fails there, on any machine.

The GPU tests run the same cases: inputs oracle.sources(kind = 1), so a
misplaced vector shows, with every 97th element of each floating or complex
input (a different phase per input) overwritten with NaNs of both signs, signed
zeros, infinities and the smallest normal, or Annex G's operands; the target in
a canary-filled buffer; the result bit for bit against the oracle (PE_start's
order; every member's own order for the P-order fold) by the rules of
test_gpu_fold.py; the canary intact; every input unchanged.  Before it launches,
a case asks the library again with its real addresses and requires the answer
of the census.
"""
from dataclasses import dataclass

import numpy as np
import pytest
from gpu_util import same_bits
from x87_cases import annex_g_operands, assert_annex_g

CUT = 32 << 20                # bytes moved from which a call is non-temporal
LANES = 256                   # one workgroup
B = 2048 * LANES              # elements one trip of the all-scalar grid covers
CANARY = 0xA5
LO, HI = 32, 48               # canary bytes in front of (before the lead) and behind every array

SIZE = {"short": 2, "int": 4, "long": 8, "longlong": 8, "float": 4, "double": 8,
        "longdouble": 16, "complexd": 16, "complexf": 8}
DTYPE = {"short": np.int16, "int": np.int32, "long": np.int64, "longlong": np.int64, "float": np.float32,
         "double": np.float64, "longdouble": np.longdouble, "complexd": np.complex128, "complexf": np.complex64}
INT_OPS = ("sum", "prod", "and", "or", "xor", "min", "max")
REAL_OPS = ("sum", "prod", "min", "max")
OPS = {"short": INT_OPS, "int": INT_OPS, "long": INT_OPS, "longlong": INT_OPS, "float": REAL_OPS,
       "double": REAL_OPS, "longdouble": REAL_OPS, "complexd": ("sum", "prod"), "complexf": ("sum", "prod")}
CPP_TYPES = ("short", "int", "long", "float", "double", "longdouble", "complexd", "complexf")
CPP_TYPE = {t: "long" if t == "longlong" else t for t in SIZE}      # the C++ type that runs it
HEAVY = {("longdouble", o) for o in REAL_OPS} | {("complexd", "prod"), ("complexf", "prod")}
OWN_ORDER = {(t, o) for t in ("float", "double", "longdouble") for o in ("min", "max")}

# group -> (route, P for the i-th C++ type); the peers groups cover their
# kernel's whole range of input counts, one of them as long long
GROUPS = {
    "fold2": ("fold", lambda i: 2),
    "fold_n3": ("fold_n", lambda i: 3),
    "peers4": ("peers", lambda i: 3 + i % 2),
    "peers8": ("peers", lambda i: 5 + i % 4),
    "peers16": ("peers", lambda i: 9 + i),
}
ORDERS_P = {"orders8": {"float": 8, "double": 3, "longdouble": 6},
            "orders16": {"float": 9, "double": 16, "longdouble": 12}}
COPY_TYPES = ("short", "float", "double", "longdouble")     # one per element size
# one pair per kernel family (and MAXIN) runs again one element below the cut
TWINS = {"fold2": ("double", "sum"), "fold_n3": ("int", "xor"), "peers4": ("float", "sum"),
         "peers8": ("short", "max"), "peers16": ("complexf", "sum"), "orders8": ("double", "min"),
         "orders16": ("float", "max"), "copy": ("short", "sum")}
IN_PLACE = ("orders16", "double", "max")     # this case again with outs[P-1] = ins[P-1]


@dataclass(frozen=True)
class Case:
    name: str
    group: str          # the pytest item is (group, type)
    kind: str           # "nt": at the cut; "below": one element below it; "scalar"
    route: str          # fold (shm.fold, in place), fold_n, peers, copy, orders
    t: str
    op: str
    P: int              # inputs
    n: int
    leads: tuple        # address mod 16 of every array: the target(s), then the inputs
    in_place: int = -1  # orders: outs[in_place] is ins[in_place]

    @property
    def item(self):
        return f"{self.group}-{self.t}"


def arrays_moved(route, P):
    """The array count of the policy rule: (nins + 1), 2, 2 nins."""
    return 2 if route == "copy" else 2 * P if route == "orders" else P + 1


def cut_elems(route, P, sz):
    """The smallest n whose arrays hold 32 MiB."""
    return -(-CUT // (arrays_moved(route, P) * sz))


def vector_n(route, P, sz):
    """The first n past the cut that, with every array one element past a
    16-byte boundary, has a scalar head and tail (elements below 16 bytes) and
    an odd number of vectors, so the last chunk is partial whatever the
    kernel's vectors per lane."""
    E = 16 // sz
    n = cut_elems(route, P, sz) + 1
    while True:
        head = E - 1 if E > 1 else 0
        nvec, tail = divmod(n - head, E)
        if nvec % 2 and (tail or E == 1):
            return n
        n += 1


def narrays(route, P):
    return 2 if route in ("fold", "copy") else 2 * P if route == "orders" else P + 1


def nt_cases():
    out = []

    def add(group, route, t, op, P):
        sz = SIZE[t]
        lead = sz % 16                                   # one element; a 16-byte type stays aligned
        leads = (lead,) * narrays(route, P)
        out.append(Case(f"{group}-{t}-{op}-P{P}", group, "nt", route, t, op, P, vector_n(route, P, sz), leads))
        if TWINS[group] == (t, op):
            out.append(Case(f"{group}-{t}-{op}-P{P}-below", group, "below", route, t, op, P,
                            cut_elems(route, P, sz) - 1, leads))
        if IN_PLACE == (group, t, op):
            out.append(Case(f"{group}-{t}-{op}-P{P}-in-place", group, "nt", route, t, op, P,
                            vector_n(route, P, sz), leads, in_place=P - 1))

    for group, (route, P_of) in GROUPS.items():
        for i, t in enumerate(CPP_TYPES):
            if group == "peers8" and t == "long":
                t = "longlong"
            for op in OPS[t]:
                add(group, route, t, op, P_of(i))
    for group, P_of in ORDERS_P.items():
        for t, P in P_of.items():
            for op in ("min", "max"):
                add(group, "orders", t, op, P)
    for t in COPY_TYPES:
        add("copy", "copy", t, "sum", 1)
    return out


# (name, route, type, op, P, leads): arrays at different addresses mod 16
SCALAR_KINDS = (
    ("copy-2-byte", "copy", "short", "sum", 1, (0, 2)),
    ("copy-16-byte", "copy", "complexd", "sum", 1, (0, 8)),            # source at 8 mod 16, target at 0
    ("two-inputs", "fold_n", "short", "sum", 2, (0, 2, 4)),
    ("three-inputs", "fold_n", "int", "xor", 3, (4, 0, 8, 12)),
    ("peers", "peers", "double", "sum", 5, (0, 0, 8, 0, 8, 8)),
    ("orders", "orders", "float", "max", 3, (0, 0, 0, 0, 4, 0)),       # one input shifted alone
    ("target-alone", "fold_n", "complexd", "prod", 3, (8, 0, 0, 0)),   # only the target at 8 mod 16
)
SCALAR_NS = (B + 1, 2 * B + 257)      # one element on the second trip; three trips, the last partial


def scalar_cases():
    return [Case(f"scalar-{name}-n{n}", f"scalar-{name}", "scalar", route, t, op, P, n, leads)
            for name, route, t, op, P, leads in SCALAR_KINDS for n in SCALAR_NS]


def large_cases():
    return nt_cases() + scalar_cases()


def items():
    seen = []
    for c in large_cases():
        if c.item not in seen:
            seen.append(c.item)
    return seen


def launch_shape(shm, c, addrs):
    """shmemx_fold_launch_shape for case c with its arrays at addrs (targets
    first, as c.leads)."""
    if c.route == "fold":
        return shm.fold_launch_shape(c.t, c.op, "plain", addrs[0], [addrs[0], addrs[1]], c.n)
    if c.route == "orders":
        return shm.fold_launch_shape(c.t, c.op, "orders", list(addrs[:c.P]), list(addrs[c.P:]), c.n)
    return shm.fold_launch_shape(c.t, c.op, "peers" if c.route == "peers" else "plain", addrs[0],
                                 list(addrs[1:]), c.n)


def made_up_addresses(c):
    a = [0x7F0000000000 + (k << 32) + LO + lead for k, lead in enumerate(c.leads)]
    if c.in_place >= 0:
        a[c.in_place] = a[c.P + c.in_place]
    return a


def instance(c, s):
    """The kernel instance behind a launch shape, as the dispatch table names
    it: the copy runs on the element size alone."""
    if s.family == "copy":
        return ("copy", 0, SIZE[c.t], None, s.nt)
    return (s.family, s.maxin, CPP_TYPE[c.t], c.op, s.nt)


def expected_nt3_instances():
    """The dispatch table of fold_kernels.hip, restated: 37 C++ pairs (long and
    long long are one), the six heavy ones kept off the peers kernels, the six
    own-order pairs, one copy per element size."""
    pairs = [(t, o) for t in CPP_TYPES for o in OPS[t]]
    assert len(pairs) == 37 and len(HEAVY) == 6 and len(OWN_ORDER) == 6
    want = {("fold2", 0, t, o, 3) for t, o in pairs} | {("fold_n", 0, t, o, 3) for t, o in pairs}
    want |= {("peers", m, t, o, 3) for m in (4, 8, 16) for t, o in pairs if (t, o) not in HEAVY}
    want |= {("orders", m, t, o, 3) for m in (8, 16) for t, o in OWN_ORDER}
    want |= {("copy", 0, sz, None, 3) for sz in (2, 4, 8, 16)}
    assert len(want) == 37 + 37 + 93 + 12 + 4 == 183
    return want


def test_large_case_list_reaches_every_instance(shm):
    cases = large_cases()
    assert len({c.name for c in cases}) == len(cases)
    shapes = {c.name: launch_shape(shm, c, made_up_addresses(c)) for c in cases}
    nt = [c for c in cases if c.kind == "nt"]
    below = [c for c in cases if c.kind == "below"]
    scalar = [c for c in cases if c.kind == "scalar"]

    # every reachable NT = 3 instance, each by exactly one case (so none can go
    # unnoticed), the in-place launch apart
    reached = [instance(c, shapes[c.name]) for c in nt if c.in_place < 0]
    assert set(reached) == expected_nt3_instances()
    heavy_on_peers = [c for c in nt if c.route == "peers" and (CPP_TYPE[c.t], c.op) in HEAVY]
    assert len(reached) - len(heavy_on_peers) == len(set(reached)) == 183
    # the peers route takes all 37 pairs in each of its three ranges of P, the
    # heavy ones through the runtime-nins kernel
    for group, (lo, hi, maxin) in {"peers4": (3, 4, 4), "peers8": (5, 8, 8), "peers16": (9, 16, 16)}.items():
        mine = [c for c in nt if c.group == group]
        assert sorted((CPP_TYPE[c.t], c.op) for c in mine) == sorted((t, o) for t in CPP_TYPES for o in OPS[t])
        assert {c.P for c in mine} == set(range(lo, hi + 1)), group
        for c in mine:
            s = shapes[c.name]
            want = ("fold_n", 0) if (CPP_TYPE[c.t], c.op) in HEAVY else ("peers", maxin)
            assert (s.family, s.maxin) == want, c.name
    assert len(heavy_on_peers) == 18
    assert any(c.t == "longlong" for c in nt) and any(c.t == "long" for c in nt)
    assert {c.P for c in nt if c.group == "fold2"} == {2} and {c.P for c in nt if c.group == "fold_n3"} == {3}
    orders_P = {c.P for c in nt if c.route == "orders"}
    assert any(P <= 8 for P in orders_P) and any(P >= 9 for P in orders_P)
    assert [(c.group, c.t, c.op, c.in_place) for c in nt if c.in_place >= 0] == [IN_PLACE + (15,)]
    assert all(shapes[c.name].nt == 3 for c in nt)

    for c in nt:
        s, sz = shapes[c.name], SIZE[c.t]
        E = 16 // sz
        chunk = LANES * s.vectors_per_lane
        assert s.head + s.nvec * E + s.tail == c.n, c.name
        # the smallest n at the cut, plus the few elements that make the edges
        assert 0 < c.n - cut_elems(c.route, c.P, sz) <= 4 * E, c.name
        if E > 1:
            assert s.head > 0 and s.tail > 0, c.name
        assert s.nvec // chunk >= 2 and s.nvec % chunk, c.name
        assert s.scalar_trips == (1 if E > 1 else 0), c.name
        assert s.blocks == -(-s.nvec // chunk), c.name
        assert arrays_moved(c.route, c.P) * c.n * sz <= 41 << 20, c.name          # device memory of a case
        pipelined = c.t == "longdouble" and s.family == "fold_n" and c.P >= 3
        assert s.ld80_pipelined == pipelined, c.name
    assert sum(shapes[c.name].ld80_pipelined for c in nt) == 4 * 4       # fold_n3 and the three peers ranges

    # one element below the cut: the same family, the default cache policy
    assert {c.group: (c.t, c.op) for c in below} == TWINS
    for c in below:
        full = [d for d in nt if (d.group, d.t, d.op, d.in_place) == (c.group, c.t, c.op, -1)]
        assert len(full) == 1 and full[0].P == c.P and full[0].leads == c.leads, c.name
        s, f = shapes[c.name], shapes[full[0].name]
        sz = SIZE[c.t]
        assert arrays_moved(c.route, c.P) * c.n * sz < CUT <= arrays_moved(c.route, c.P) * (c.n + 1) * sz
        assert (s.nt, s.family, s.maxin, s.vectors_per_lane) == (0, f.family, f.maxin, f.vectors_per_lane), c.name
        assert s.nvec > 0, c.name

    # the all-scalar path: no body, two and three trips of 2048 workgroups
    assert sorted((c.group, c.n) for c in scalar) == sorted((f"scalar-{k[0]}", n) for k in SCALAR_KINDS
                                                            for n in SCALAR_NS)
    for c in scalar:
        s = shapes[c.name]
        assert (s.nvec, s.head, s.tail, s.blocks) == (0, c.n, 0, 2048), c.name
        assert s.scalar_trips == {B + 1: 2, 2 * B + 257: 3}[c.n], c.name
        assert len(set(c.leads)) > 1 and all(lead % min(SIZE[c.t], 8) == 0 for lead in c.leads), c.name
    fam = {c.group: shapes[c.name].family for c in scalar}
    assert fam == {"scalar-copy-2-byte": "copy", "scalar-copy-16-byte": "copy", "scalar-two-inputs": "fold2",
                   "scalar-three-inputs": "fold_n", "scalar-peers": "peers", "scalar-orders": "orders",
                   "scalar-target-alone": "fold_n"}
    orders = [c for c in scalar if c.route == "orders"][0]
    assert sorted(orders.leads[orders.P:]) == [0, 0, 4] and set(orders.leads[:orders.P]) == {0}
    alone = [c for c in scalar if c.group == "scalar-target-alone"][0]
    assert alone.leads[0] == 8 and set(alone.leads[1:]) == {0}

    # every case of an item shares its inputs: one type, one P, one placement
    for item in items():
        mine = [c for c in cases if c.item == item]
        assert len({(c.t, c.P, c.leads, c.route) for c in mine}) == 1, item
    assert len(items()) == 5 * 8 + 6 + 4 + len(SCALAR_KINDS)


# ------------------------------------------------------------------ inputs
def make_inputs(oracle, t, P, n, seed):
    """[P, n] sources of kind 1 (mixed signs, full range); in every floating
    and complex input every 97th element, from a phase of its own, is a NaN of
    either sign, a signed zero, an infinity, +-1, 2 or the smallest normal
    (oracle.special_sources' pool), or one of Annex G's 64 operands."""
    srcs = oracle.sources(t, 1, P, n, base_seed=seed)
    for p in range(P):
        idx = np.arange((11 * p + 5) % 97, n, 97)
        if t in ("float", "double", "longdouble"):
            srcs[p, idx] = oracle.special_sources(t, 1, len(idx), seed=seed + 1000 + p)[0]
        elif t in ("complexd", "complexf"):
            zs = annex_g_operands(t)[1][:64]
            srcs[p, idx] = zs[(oracle.splitmix64(seed + 2000 + p, len(idx)) % np.uint64(64)).astype(np.int64)]
    return srcs


def item_seed(item):
    return 0x1A26E0000 + 7919 * sum(item.encode())


def expected(oracle, c, srcs):
    """The oracle's answer over all of srcs: PE_start's order, or for the
    P-order fold every member's own."""
    if c.route == "orders":
        return [oracle.reduce_one(c.t, c.op, srcs, 0, 0, c.P, k) for k in range(c.P)]
    return oracle.reduce_one(c.t, c.op, srcs, 0, 0, c.P, 0)


def test_large_orders_inputs_discriminate(oracle):
    """On the oracle alone, over the leading 8192 elements of each P-order
    item's inputs: some member's answer differs from member 0's, so a kernel
    that handed every member one order fails.  (The GPU test asserts the same
    over the whole arrays.)"""
    for c in large_cases():
        if c.route == "orders" and c.in_place < 0 and c.kind != "below":
            srcs = make_inputs(oracle, c.t, c.P, 8192, item_seed(c.item))
            want = expected(oracle, c, srcs)
            assert any(not same_bits(want[k], want[0]) for k in range(1, c.P)), c.name


# --------------------------------------------------------------- GPU side
def assert_result(c, got, want, what):
    """test_gpu_fold.py's rules: bit for bit; a floating sum or product may
    differ in a NaN's payload (IEEE 754 does not specify it), so NaN where the
    oracle has NaN and exact bits elsewhere; long double value bytes exact."""
    if c.route == "copy":
        assert same_bits(got, want), what
    elif c.t in ("complexd", "complexf"):
        assert_annex_g(got, want, what)
    elif c.t in ("float", "double") and c.op in ("sum", "prod"):
        nan_w, nan_g = np.isnan(want), np.isnan(got)
        assert np.array_equal(nan_w, nan_g), what
        assert same_bits(got[~nan_g], want[~nan_w]), what
    else:
        assert same_bits(got, want), what


class Guarded:
    """`data`'s bytes (or nbytes of canary) on the device at address
    lead mod 16, with LO canary bytes in front of the lead and HI behind."""

    def __init__(self, torch, lead, data=None, nbytes=0):
        raw = None if data is None else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        self.nbytes = nbytes if raw is None else raw.size
        self.lo = LO + lead
        self.host = np.full(self.lo + self.nbytes + HI, CANARY, dtype=np.uint8)
        if raw is not None:
            self.host[self.lo:self.lo + self.nbytes] = raw
        self.dev = torch.from_numpy(self.host).cuda()
        assert self.dev.data_ptr() % 16 == 0
        self.ptr = self.dev.data_ptr() + self.lo

    def read(self, dtype, n, what):
        """The first n elements, after checking the canary around the n."""
        got = self.dev.cpu().numpy()
        end = self.lo + n * np.dtype(dtype).itemsize
        assert end == self.lo + self.nbytes
        assert (got[:self.lo] == CANARY).all() and (got[end:] == CANARY).all(), f"{what}: wrote outside the target"
        return got[self.lo:end].view(dtype)

    def unchanged(self):
        return bool((self.dev.cpu().numpy() == self.host).all())


def run_item(torch, shm, oracle, item):
    cases = [c for c in large_cases() if c.item == item]
    first = cases[0]
    t, P, route, leads = first.t, first.P, first.route, first.leads
    dt, sz = DTYPE[t], SIZE[t]
    nmax = max(c.n for c in cases)
    srcs = make_inputs(oracle, t, P, nmax, item_seed(item))
    in_leads = leads[-P:] if route != "fold" else leads
    # (the two-input fold runs in place: its first input is uploaded per case)
    inputs = [None if route == "fold" and p == 0 else Guarded(torch, in_leads[p], data=srcs[p]) for p in range(P)]
    wants = {}
    for c in cases:
        what = c.name
        if c.op not in wants:
            wants[c.op] = expected(oracle, c, srcs)
            if route == "orders":
                assert any(not same_bits(w, wants[c.op][0]) for w in wants[c.op][1:]), f"{what}: one shared answer"
        want = wants[c.op]
        ins = [g.ptr if g else None for g in inputs]
        if route == "fold":                    # acc = op(acc, in): the accumulator is target and input 0
            outs = [Guarded(torch, leads[0], data=srcs[0][:c.n])]
            ins[0] = outs[0].ptr
        elif route == "orders":
            outs = [Guarded(torch, leads[k], nbytes=c.n * sz) for k in range(P)]
            if c.in_place >= 0:
                outs[c.in_place] = Guarded(torch, leads[c.in_place], data=srcs[c.in_place][:c.n])
                ins[c.in_place] = outs[c.in_place].ptr
        else:
            outs = [Guarded(torch, leads[0], nbytes=c.n * sz)]
        addrs = [g.ptr for g in outs] + (ins if route != "fold" else ins[1:])
        assert [a % 16 for a in addrs] == list(leads), what
        # the instance and grid the census saw for this case
        assert launch_shape(shm, c, addrs) == launch_shape(shm, c, made_up_addresses(c)), what
        if route == "fold":
            shm.fold(t, c.op, outs[0].ptr, ins[1], c.n)
        elif route == "orders":
            shm.fold_orders_on_stream(t, c.op, [g.ptr for g in outs], ins, c.n)
        else:
            shm.fold_n(t, c.op, outs[0].ptr, ins, c.n, peers=route == "peers")
        torch.cuda.synchronize()
        assert shm.last_error() == 0, what
        for k, g in enumerate(outs):
            w = want[k] if route == "orders" else want
            got = g.read(dt, c.n, what)
            assert_result(c, got, w[:c.n], f"{what}: output {k}")
            if route == "copy":      # a copy moves bits: long double's padding bytes too, which no oracle defines
                assert got.tobytes() == srcs[0][:c.n].tobytes(), f"{what}: not the source's bytes"
        del outs
    for p, g in enumerate(inputs):
        assert g is None or g.unchanged(), f"{item}: input {p} changed"


@pytest.mark.gpu
@pytest.mark.parametrize("item", items())
def test_fold_large(cuda, shm, oracle, item):
    """Every case of one (route, type): the non-temporal instances at the
    cut, the twin one element below it, or the all-scalar path at two and
    three trips."""
    import torch
    run_item(torch, shm, oracle, item)
