"""The software x87 (ld80.h) and the Annex G complex product (cmul) as hipcc
compiles them for the GPU, on directed operands (x87_cases.py), through every
route that instantiates them:

  fold2      shm.fold_n, two inputs (fold_kernel<ld80, OP, 2>), both orders
  fold_n3    shm.fold_n, three inputs: the runtime-count kernel's pipelined
             long double branch, and the same under peers (a heavy op keeps
             the runtime kernel there)
  orders     shm.fold_orders_on_stream, min / max, P = 3 and 9 (the 8- and
             16-input instances, ROLLED loop), every member's own answer
  oneshot    shm.fused_loopback schedule 0: a size one block folds alone
             (at most 1024 elements) and one the grid folds
  twoshot    shm.fused_loopback schedule 1, every member's slice
  service    shm.service_fold_loopback, requests of at most 256 elements,
             with and without own_order

Long double results are compared bit for bit on the 10 value bytes, NaN
payloads included, with the oracle (the host's x87: test_x87_cases.py shows
the oracle, numpy and the census's integer arithmetic agree on every pair).
The three-input routes fold (a, b, c) with c = x87_cases.third(op, a, b).
Complex products follow test_complex_prod_annex_g's rule: NaN exactly where
the oracle has NaN, identical bytes elsewhere.  Every target lies between
0xA5 canary bytes.  No tolerance anywhere, nothing is timed.

A failure names route, op, group and pair index, and prints the operands; the
same pair can then be given to tests/native/test_ld80 --pairs, which
test_x87_cases.py shows to be right on the whole list on the host.

What each route runs, in pairs (a op b, then r op c for the three-input
routes), by census class: test_routes_hold_their_classes prints the table.
"""
import numpy as np
import pytest
import x87_cases as X
from gpu_util import from_dev
from test_gpu_fold import _dev_bytes, _fold_into_guarded
from test_gpu_fused import slice_bounds
from test_gpu_service_fold import _Targets

gpu = pytest.mark.gpu

OPS = ("sum", "prod", "min", "max")
CANARY = 0xA5
TINY = 1024                   # kFusedTinyElems: one block folds alone up to here
REQUEST = 256                 # long doubles (and double complexes) in one exchange slot
_CACHE = {}


class _Listed:
    """The list, its census, the per-op third operands and the references,
    each computed once and read-only."""

    def __init__(self, oracle):
        self.oracle = oracle
        self.a, self.b, self.groups = X.pairs()
        self.cen = X.census(self.a, self.b)
        self.all = np.arange(len(self.a))
        self.sub = np.array(X.cover(self.cen, self.groups))
        self.cmp = X.select(self.groups, "compare/", "special/")
        self._c, self._want = {}, {}

    def c(self, op):
        if op not in self._c:
            self._c[op] = X.third(op, self.a, self.b)
            self._c[op].flags.writeable = False
        return self._c[op]

    def want2(self, op, swapped=False):
        key = (op, 2, swapped)
        if key not in self._want:
            srcs = np.stack([self.b, self.a] if swapped else [self.a, self.b])
            self._want[key] = self.oracle.reduce_sim("longdouble", op, srcs, 0, 0, 2)[0]
        return self._want[key]

    def want3(self, op):
        """Every member's own-order answer of (a, b, c); [0] is the set order's."""
        key = (op, 3)
        if key not in self._want:
            self._want[key] = self.oracle.reduce_sim("longdouble", op, np.stack([self.a, self.b, self.c(op)]),
                                                     0, 0, 3)
        return self._want[key]


@pytest.fixture(scope="module")
def listed(oracle):
    if "L" not in _CACHE:
        _CACHE["L"] = _Listed(oracle)
    return _CACHE["L"]


def _hex(x, i):
    sig, se = X.from_slots(x[i:i + 1])[0]
    return "%04x:%016x" % (se, sig)


def _same(route, op, got, want, idx, L, operands):
    """got == want on the 10 value bytes; idx[k] is element k's pair index."""
    g = np.ascontiguousarray(got).view(np.uint8).reshape(-1, 16)[:, :10]
    w = np.ascontiguousarray(want).view(np.uint8).reshape(-1, 16)[:, :10]
    assert g.shape == w.shape, (route, op, g.shape, w.shape)
    bad = np.flatnonzero((g != w).any(axis=1))
    if bad.size:
        k = int(bad[0])
        i = int(idx[k])
        raise AssertionError("%s %s: %d of %d elements differ; first at element %d, group %s, pair %d: "
                             "operands %s got %s want %s" % (
                                 route, op, bad.size, len(g), k, L.groups[i], i,
                                 " ".join(_hex(x, k) for x in operands), _hex(got, k), _hex(want, k)))


# -------------------------------------------------- what every route runs (no GPU)
def test_routes_hold_their_classes(listed):
    """Every route's list holds every census class of the whole list (the
    orders route: every compare and specials group), the one-block fused
    size and every service request fit, and the table of what each route
    runs is printed (pytest -s)."""
    L = listed
    every = set(X.counts(L.cen))
    assert len(L.all) > TINY and len(L.sub) <= TINY
    assert set(X.counts(L.cen, L.sub)) == every
    assert {L.groups[i] for i in L.sub} == set(L.groups)
    assert {L.groups[i] for i in L.cmp} == {g for g in L.groups if g.startswith(("compare/", "special/"))}
    rows = {"fold2 (x2 orders), fold_n3, fold_n3 peers, oneshot grid, twoshot": L.all,
            "oneshot one block, service": L.sub, "orders (P = 3, 9)": L.cmp}
    for name, idx in rows.items():
        print("\n%s: %d pairs, a op b: %s" % (name, len(idx), X.broad(L.cen, idx)))
    for op in ("sum", "prod"):
        r = X.host_op(op, L.a, L.b)
        for name, idx in list(rows.items())[:2]:
            step2 = X.census(r[idx], L.c(op)[idx])
            print("\n%s: (a %s b) then c: %s" % (name, op, X.broad(step2)))


# --------------------------------------------------------------- fold_n routes
@gpu
@pytest.mark.parametrize("op", OPS)
def test_two_input_fold(cuda, shm, listed, op):
    import torch
    L = listed
    da, db = _dev_bytes(torch, L.a), _dev_bytes(torch, L.b)
    for swapped in (False, True):
        x, y = (db, da) if swapped else (da, db)
        got = _fold_into_guarded(torch, shm, "longdouble", op, [x.data_ptr(), y.data_ptr()], len(L.a), 16, 0,
                                 False, np.longdouble)
        _same("fold2 %s" % ("b,a" if swapped else "a,b"), op, got, L.want2(op, swapped), L.all, L,
              (L.b, L.a) if swapped else (L.a, L.b))


@gpu
@pytest.mark.parametrize("peers", [False, True])
@pytest.mark.parametrize("op", OPS)
def test_runtime_count_fold(cuda, shm, listed, op, peers):
    import torch
    L = listed
    srcs = (L.a, L.b, L.c(op))
    dev = [_dev_bytes(torch, s) for s in srcs]
    got = _fold_into_guarded(torch, shm, "longdouble", op, [d.data_ptr() for d in dev], len(L.a), 16, 0, peers,
                             np.longdouble)
    _same("fold_n3%s" % (" peers" if peers else ""), op, got, L.want3(op)[0], L.all, L, srcs)


@gpu
@pytest.mark.parametrize("P", [3, 9])
@pytest.mark.parametrize("op", ["min", "max"])
def test_p_order_fold(cuda, shm, oracle, listed, op, P):
    """Inputs 0..2 are a, b, c of the compare and specials groups; the
    further ones the same three rotated by 37 pairs each, so every member
    meets other classes.  Member k's answer against oracle.reduce_one."""
    import torch
    L = listed
    idx = L.cmp
    n, nb = len(idx), len(idx) * 16
    base = (L.a[idx], L.b[idx], L.c(op)[idx])
    srcs = np.stack([np.roll(base[k % 3], 37 * (k // 3)) for k in range(P)])
    dev = [_dev_bytes(torch, srcs[k]) for k in range(P)]
    stride = 32 + nb + 48
    out = torch.full((P * stride,), CANARY, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 16 == 0 and stride % 16 == 0
    shm.fold_orders_on_stream("longdouble", op, [out.data_ptr() + k * stride + 32 for k in range(P)],
                              [d.data_ptr() for d in dev], n)
    torch.cuda.synchronize()
    image = out.cpu().numpy().reshape(P, stride)
    assert (image[:, :32] == CANARY).all() and (image[:, 32 + nb:] == CANARY).all(), "orders: wrote outside"
    for k in range(P):
        want = oracle.reduce_one("longdouble", op, srcs, 0, 0, P, k)
        got = image[k, 32:32 + nb].copy().view(np.longdouble)
        _same("orders P=%d member %d" % (P, k), op, got, want, idx, L, tuple(srcs))
    for k in range(P):
        assert from_dev(dev[k], np.longdouble).tobytes() == srcs[k].tobytes(), "orders: an input changed"


# ---------------------------------------------------------------- fused routes
def _fused(torch, shm, t, op, schedule, srcs, m, compare):
    """Member m's fused launch over srcs [P, n]: compare(got, lo, hi) sees
    the elements the launch must have folded; every other byte of the target
    buffer (the gathered slices of a two shot aside, which must hold what
    their owners' targets held) and the sources must be as before."""
    P, n = srcs.shape
    sz = srcs.itemsize
    nb = n * sz
    stride = -(-(32 + nb + 48) // 16) * 16
    s_host = np.full(P * stride, CANARY, np.uint8)
    t_pre = np.full(P * stride, CANARY, np.uint8)
    for i in range(P):
        s_host[i * stride + 32:i * stride + 32 + nb] = np.ascontiguousarray(srcs[i]).view(np.uint8)
        rng = np.random.default_rng(0x87E7 + 1009 * i + n)
        t_pre[i * stride + 32:i * stride + 32 + nb] = rng.integers(0, 256, nb, dtype=np.uint8)
    S, T = _dev_bytes(torch, s_host), _dev_bytes(torch, t_pre)
    err = shm.fused_loopback(t, op, schedule, [T.data_ptr() + i * stride + 32 for i in range(P)],
                             [S.data_ptr() + i * stride + 32 for i in range(P)], n, m=m)
    assert err == 0
    got, exp = T.cpu().numpy(), t_pre.copy()
    mine = exp[m * stride + 32:m * stride + 32 + nb]
    lo, hi = 0, n
    if schedule == 1:
        sl = slice_bounds(n, P, sz)
        lo, hi = sl[m]
        for i, (x, y) in enumerate(sl):
            if i != m:
                mine[x * sz:y * sz] = t_pre[i * stride + 32 + x * sz:i * stride + 32 + y * sz]
    folded = got[m * stride + 32 + lo * sz:m * stride + 32 + hi * sz]
    compare(folded.copy().view(srcs.dtype), lo, hi)
    mine[lo * sz:hi * sz] = folded
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, ("fused schedule %d %s %s m=%d: target-buffer bytes outside the fold differ, first at"
                           % (schedule, t, op, m), bad[:4])
    assert np.array_equal(S.cpu().numpy(), s_host), "a source changed"


def _fused_ld(torch, shm, L, op, schedule, idx, m, route):
    srcs = np.stack([L.a[idx], L.b[idx], L.c(op)[idx]])
    want = L.want3(op)[0][idx]
    _fused(torch, shm, "longdouble", op, schedule, srcs, m,
           lambda got, lo, hi: _same("%s m=%d" % (route, m), op, got, want[lo:hi], idx[lo:hi], L,
                                     tuple(s[lo:hi] for s in srcs)))


@gpu
@pytest.mark.parametrize("op", OPS)
def test_fused_one_shot(cuda, shm, listed, op):
    import torch
    L = listed
    assert len(L.sub) <= TINY < len(L.all)
    _fused_ld(torch, shm, L, op, 0, L.sub, 1, "oneshot one block")
    _fused_ld(torch, shm, L, op, 0, L.all, 2, "oneshot grid")


@gpu
@pytest.mark.parametrize("op", OPS)
def test_fused_two_shot(cuda, shm, listed, op):
    import torch
    L = listed
    for m in range(3):
        _fused_ld(torch, shm, L, op, 1, L.all, m, "twoshot")


# ------------------------------------------------------------ the service fold
def _service(torch, shm, t, op, own, srcs, want_of, compare):
    """srcs [3, n] in requests of at most REQUEST elements as PE 0, 1, 2 with
    own_order (each its own answer) or as PE 1 without (PE_start's)."""
    shm.init()
    tg = _Targets(torch)
    before = shm.service_stats()
    requests = 0
    n, sz = srcs.shape[1], srcs.itemsize
    for lo in range(0, n, REQUEST):
        hi = min(n, lo + REQUEST)
        rows = [np.ascontiguousarray(srcs[p, lo:hi]) for p in range(3)]
        for me in ((0, 1, 2) if own else (1,)):
            tg.refill()
            shm.service_fold_loopback(t, op, tg.dst(0), rows, hi - lo, me=me, own_order=own)
            got = tg.check(("service", t, op, own, lo, me), (hi - lo) * sz, 0, None).view(srcs.dtype)
            compare(got, want_of(me if own else 0)[lo:hi], lo, hi, me)
            requests += 1
    after = shm.service_stats()
    assert after["served"] - before["served"] == requests and after["folds"] - before["folds"] == requests


@gpu
@pytest.mark.parametrize("own", [False, True])
@pytest.mark.parametrize("op", OPS)
def test_service_fold(cuda, shm, listed, op, own):
    import torch
    L = listed
    idx = L.sub
    srcs = np.stack([L.a[idx], L.b[idx], L.c(op)[idx]])
    want = L.want3(op)
    _service(torch, shm, "longdouble", op, own, srcs, lambda me: want[me][idx],
             lambda got, w, lo, hi, me: _same("service own=%s me=%d" % (own, me), op, got, w, idx[lo:hi], L,
                                              tuple(s[lo:hi] for s in srcs)))


# ----------------------------------------------------------- the complex product
def _annex_g(oracle, t):
    """(srcs [3, 4096], every member's answer): every pair of the Annex G
    operands, and as third input the second in reverse."""
    key = ("annex", t)
    if key not in _CACHE:
        a, b = X.annex_g_operands(t)
        srcs = np.stack([a, b, b[::-1]])
        srcs.flags.writeable = False
        _CACHE[key] = (srcs, oracle.reduce_sim(t, "prod", srcs, 0, 0, 3))
    return _CACHE[key]


@gpu
@pytest.mark.parametrize("t", ["complexd", "complexf"])
def test_complex_prod_annex_g_runtime_fold(cuda, shm, oracle, t):
    import torch
    srcs, want = _annex_g(oracle, t)
    dev = [_dev_bytes(torch, s) for s in srcs]
    for peers in (False, True):
        got = _fold_into_guarded(torch, shm, t, "prod", [d.data_ptr() for d in dev], srcs.shape[1],
                                 srcs.itemsize, 0, peers, srcs.dtype)
        X.assert_annex_g(got, want[0], ("fold_n3", t, "peers" if peers else "plain"))


@gpu
@pytest.mark.parametrize("t", ["complexd", "complexf"])
def test_complex_prod_annex_g_fused(cuda, shm, oracle, t):
    """One shot in launches of 1024 (one block folds alone) and of all 4096
    (the grid), two shot as every member."""
    import torch
    srcs, want = _annex_g(oracle, t)
    n = srcs.shape[1]
    for lo in range(0, n, TINY):
        part = np.ascontiguousarray(srcs[:, lo:lo + TINY])
        _fused(torch, shm, t, "prod", 0, part, 1,
               lambda got, x, y: X.assert_annex_g(got, want[0][lo + x:lo + y], ("oneshot one block", t, lo)))
    _fused(torch, shm, t, "prod", 0, srcs, 2,
           lambda got, x, y: X.assert_annex_g(got, want[0][x:y], ("oneshot grid", t)))
    for m in range(3):
        _fused(torch, shm, t, "prod", 1, srcs, m,
               lambda got, x, y: X.assert_annex_g(got, want[0][x:y], ("twoshot", t, m)))


@gpu
@pytest.mark.parametrize("t", ["complexd", "complexf"])
def test_complex_prod_annex_g_service_fold(cuda, shm, oracle, t):
    import torch
    srcs, want = _annex_g(oracle, t)
    for own in (False, True):
        _service(torch, shm, t, "prod", own, srcs, lambda me: want[me],
                 lambda got, w, lo, hi, me: X.assert_annex_g(got, w, ("service", t, own, lo, me)))
