"""The directed x87 operands (x87_cases.py) without a GPU: the list holds every
class the GPU tests rely on, its references agree with each other on every
pair, and the host build of ld80.h is right on all of it.

Three references meet here: numpy's long double (the host's x87 unit), the
oracle (the reference's fold, compiled C), and the census's own arithmetic in
Python integers.  They agree on every pair of the list, unsupported encodings
included, so the oracle alone carries the GPU comparison in
test_gpu_x87_edges.py.
"""
import os
import subprocess

import numpy as np
import pytest
import x87_cases as X
from gpu_util import same_bits, value_bytes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ("sum", "prod", "min", "max")


@pytest.fixture(scope="module")
def listed():
    a, b, groups = X.pairs()
    return a, b, groups, X.census(a, b)


def _differing(got, want):
    g = np.ascontiguousarray(got).view(np.uint8).reshape(-1, 16)[:, :10]
    w = np.ascontiguousarray(want).view(np.uint8).reshape(-1, 16)[:, :10]
    return np.flatnonzero((g != w).any(axis=1))


def _assert_same(got, want, a, b, groups, what):
    bad = _differing(got, want)
    if bad.size:
        i = int(bad[0])
        show = [X.from_slots(x[i:i + 1])[0] for x in (a, b, got, want)]
        raise AssertionError("%s: %d pairs differ, first %d (%s): a=%s b=%s got=%s want=%s" % (
            what, bad.size, i, groups[i], *["%04x:%016x" % (se, sig) for sig, se in show]))


def test_list_fits(listed):
    a, b, groups, cen = listed
    assert len(a) == len(b) == len(groups) == len(cen) <= X.MAX_PAIRS
    assert a.dtype == b.dtype == np.longdouble and a.itemsize == 16
    a2, b2, g2 = X.pairs()
    assert value_bytes(a) == value_bytes(a2) and value_bytes(b) == value_bytes(b2) and groups == g2
    pad = np.ascontiguousarray(a).view(np.uint8).reshape(-1, 16)[:, 10:]
    assert not pad.any()


def test_census_minimums(listed):
    """Conditions, not measurements: every (d, signs) of the fast add at
    least 5 times; ties of both parities, rounding carries, overflow and
    cancellation into the denormal range for add, ties of both parities and
    rounding carries for mul, every product exponent -66..+2 and
    0x7FFD..0x8000 at least 8 times; every result class; every specials and
    compare group in both operand orders."""
    a, b, groups, cen = listed
    assert X.shortfalls(groups, cen) == []


@pytest.mark.parametrize("drop,missing", [
    (("mul/tie",), "mul:tie:even"), (("mul/round-carry",), "mul:round-carry"),
    (("add/cancel-into-denormal", "add/normal/low"), "add:cancel-into-denormal"),
    (("add/normal/top",), "add:overflow"),
    (("special/nan-equal-significands",), "group special/nan-equal-significands/ab"),
    (("compare/zeros",), "group compare/zeros/ba")])
def test_census_notices_an_emptied_class(drop, missing):
    """The same list without a class's groups falls short of exactly that class."""
    a, b, groups = X.pairs(drop=drop)
    short = X.shortfalls(groups, X.census(a, b))
    assert any(s.startswith(missing) for s in short), short


def test_cover_keeps_every_class(listed):
    a, b, groups, cen = listed
    sub = X.cover(cen, groups)
    assert len(sub) < len(a) // 8 and sub == sorted(set(sub))
    assert set(X.counts(cen, sub)) == set(X.counts(cen))
    assert {groups[i] for i in sub} == set(groups)
    assert X.shortfalls([groups[i] for i in sub], [cen[i] for i in sub]) != []   # minimums need the whole list


def test_census_arithmetic_is_the_hosts(listed):
    """The census's sums, products and comparisons, from Python integers, are
    the host x87's on every pair: its classes describe what really happens."""
    a, b, groups, cen = listed
    _assert_same(X.to_slots([c[1] for c in cen]), X.host_op("sum", a, b), a, b, groups, "census add")
    _assert_same(X.to_slots([c[2] for c in cen]), X.host_op("prod", a, b), a, b, groups, "census mul")
    with np.errstate(all="ignore"):
        assert np.array_equal(np.array([c[3] for c in cen]), a < b)
        assert np.array_equal(np.array([c[4] for c in cen]), a > b)


@pytest.mark.parametrize("op", OPS)
def test_oracle_is_the_hosts_x87(oracle, listed, op):
    """oracle.reduce_sim equals numpy's own a op b on the 10 value bytes of
    every pair, both orders, and on the three-input chains."""
    a, b, groups, _ = listed
    for x, y in ((a, b), (b, a)):
        want = X.host_op(op, x, y)
        _assert_same(oracle.reduce_sim("longdouble", op, np.stack([x, y]), 0, 0, 2)[0], want, x, y, groups,
                     "oracle " + op)
    c = X.third(op, a, b)
    got = oracle.reduce_sim("longdouble", op, np.stack([a, b, c]), 0, 0, 3)[0]
    _assert_same(got, X.host_op(op, X.host_op(op, a, b), c), a, b, groups, "oracle chain " + op)


def test_chains_reach_their_classes(listed):
    """The third operands do what they are for: after a + b, exact
    cancellation, ties and sticky-only roundings; after a * b, products on
    the denormal range and the overflow boundary."""
    a, b, _, _ = listed
    c = X.third("sum", a, b)
    got = X.counts(X.census(X.host_op("sum", a, b), c))
    for lab in ("add:cancel", "add:tie:even", "add:tie:odd", "add:inexact"):
        assert got[lab] >= 8, (lab, got[lab])
    assert sum(k for lab, k in got.items() if lab.startswith("add:d=64:")) >= 8
    assert sum(k for lab, k in got.items() if lab.startswith("add:d=65:")) >= 8
    c = X.third("prod", a, b)
    got = X.counts(X.census(X.host_op("prod", a, b), c))
    assert sum(k for lab, k in got.items() if lab.startswith("mul:e=-")) >= 8
    assert sum(k for lab, k in got.items() if lab.startswith("mul:e=32")) >= 8


def test_host_build_of_ld80_on_the_directed_list(tmp_path, oracle, listed):
    """ld80.h as g++ compiles it, on the whole list in both orders, against
    the oracle: a GPU mismatch on a pair that passes here is the device
    compiler's (or undefined behaviour), one that fails here is the logic's."""
    a, b, groups, _ = listed
    exe = tmp_path / "test_ld80"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(REPO, "openshmem-async_amd", "csrc"),
                    os.path.join(REPO, "tests", "native", "test_ld80.cpp"), "-o", str(exe)], check=True)
    for x, y, order in ((a, b, "ab"), (b, a, "ba")):
        inp, outp = tmp_path / ("pairs_" + order), tmp_path / ("results_" + order)
        np.stack([x, y], axis=1).tofile(inp)
        r = subprocess.run([str(exe), "--pairs", str(inp), str(outp)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout == "pairs %d\n" % len(x), r.stdout + r.stderr
        got = np.fromfile(outp, dtype=np.longdouble).reshape(len(x), 4)
        for k, op in enumerate(OPS):
            want = oracle.reduce_sim("longdouble", op, np.stack([x, y]), 0, 0, 2)[0]
            _assert_same(np.ascontiguousarray(got[:, k]), want, x, y, groups, "host ld80 %s %s" % (op, order))


@pytest.mark.parametrize("t", ["complexd", "complexf"])
def test_annex_g_operands(oracle, t):
    """64 x 64 pairs; the oracle's product recovers infinities (a NaN-free
    infinite result exists) and has NaNs, so both sides of the rule are hit."""
    a, b = X.annex_g_operands(t)
    assert len(a) == len(b) == 4096 and len(np.unique(a.view(np.uint8).reshape(4096, -1), axis=0)) == 64
    want = oracle.reduce_sim(t, "prod", np.stack([a, b]), 0, 0, 2)[0]
    assert np.isnan(want.real).any() and np.isinf(want.real[~np.isnan(want.real)]).any()
    recovered = (np.isnan(a.real) | np.isnan(a.imag) | np.isnan(b.real) | np.isnan(b.imag)) & np.isinf(want.real)
    assert recovered.any()
    X.assert_annex_g(want, want, t)
    assert same_bits(want, want)
