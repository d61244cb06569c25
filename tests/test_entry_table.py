"""CPU tests of the two tables of csrc/entry.cpp that forward a name to a
(type, op): the 44 typed stream-ordered forms and the 37 Fortran forwarders
(tests/entry_table.py restates them).  The list itself, the header, the
aliases in the built library, every prototype (compile only), and the census
that makes the bitwise multi-PE check of tests/test_gpu_entry_points.py
discriminating: on its inputs no other reduction of the same element size
gives the promised bytes.  No GPU calls here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import entry_table as et
from test_abi import HEADER, LIB, exported

PRE = None


def preprocessed():
    global PRE
    if PRE is None:
        PRE = subprocess.run(["gcc", "-E", "-P", "-x", "c", HEADER], check=True,
                             capture_output=True, text=True).stdout
    return PRE


def test_entry_counts(shm):
    assert len(et.STREAM_ENTRIES) == 44 and len(et.FORTRAN_ENTRIES) == 37
    assert len({e.symbol for e in et.ENTRIES}) == 81
    assert len(et.all_symbols()) == 44 + 2 * 37
    assert [(e.type, e.op) for e in et.STREAM_ENTRIES] == list(shm.REFERENCE_PAIRS)
    for e in et.ENTRIES:
        assert (e.type, e.op) in shm.REFERENCE_PAIRS, e
    # 6 real and integer kinds x 4 ops, 3 integer kinds x 3 ops, 2 complex kinds x 2 ops
    by_op = {}
    for e in et.FORTRAN_ENTRIES:
        by_op.setdefault(e.op, set()).add(e.type)
    assert {op: len(ts) for op, ts in by_op.items()} == {"sum": 8, "prod": 8, "max": 6, "min": 6,
                                                           "and": 3, "or": 3, "xor": 3}


def test_every_name_is_declared_in_the_header():
    import re
    declared = set(re.findall(r"\b(p?shmemx?_[A-Za-z0-9_]+)\s*\(", preprocessed()))
    missing = [s for s in et.all_symbols() if s not in declared]
    assert not missing, missing
    # and the header declares no Fortran forwarder or typed stream form the list lacks
    extra = [d for d in declared if (d.endswith("_to_all_") or d.endswith("_to_all_on_stream"))
             and d not in et.all_symbols()]
    assert not extra, extra


def test_shmem_and_pshmem_names_are_one_function(shm):
    """shmem_X and pshmem_X resolve to the same address for the 44 blocking
    and the 37 Fortran names; nm -D shows pshmem_ strong and shmem_ weak."""
    L = ctypes.CDLL(LIB)
    syms = exported()
    names = [f"shmem_{t}_{o}_to_all" for t, o in shm.REFERENCE_PAIRS] + [e.symbol for e in et.FORTRAN_ENTRIES]
    assert len(names) == 44 + 37
    seen = {}
    for name in names:
        a = ctypes.cast(getattr(L, name), ctypes.c_void_p).value
        b = ctypes.cast(getattr(L, "p" + name), ctypes.c_void_p).value
        assert a and a == b, name
        assert syms["p" + name][1] == "T" and syms[name][1] == "W", name
        assert syms[name][0] == syms["p" + name][0], name
        seen.setdefault(a, []).append(name)
    # 81 functions: no two names share a body (an alias naming another entry)
    shared = [v for v in seen.values() if len(v) > 1]
    assert not shared, shared
    stream = {ctypes.cast(getattr(L, e.symbol), ctypes.c_void_p).value for e in et.STREAM_ENTRIES}
    assert len(stream) == 44 and not stream & set(seen)


@pytest.mark.parametrize("compiler", ["gcc", "g++"])
def test_every_prototype_is_the_promised_one(tmp_path, compiler):
    """A function pointer of exactly the promised type initialised from every
    typed stream form and every Fortran forwarder in both spellings: a wrong
    element type, a missing const, int for int * or another return type is an
    error (C: -Werror -Wincompatible-pointer-types; C++: always)."""
    lines = ['#include "shmem_reduce_mi355x.h"']
    k = 0
    for e in et.ENTRIES:
        for name in et.spellings(e):
            lines.append(et.c_prototype(e, name, f"(*p{k})"))
            k += 1
    assert k == 44 + 2 * 37
    lines.append("int main(void) { return 0; }")
    ext, flags = ((".c", ["-std=c99", "-Werror", "-Wincompatible-pointer-types"]) if compiler == "gcc"
                  else (".cpp", ["-std=c++17", "-Werror"]))
    src = tmp_path / ("prototypes" + ext)
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([compiler, *flags, "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)], check=True)
    # the check bites: one wrong element type is refused
    bad = tmp_path / ("bad" + ext)
    wrong = et.c_prototype(et.Entry("x", "stream", "double", "max"), "shmemx_float_max_to_all_on_stream", "(*q)")
    bad.write_text(lines[0] + "\n" + wrong + "\nint main(void) { return 0; }\n")
    out = subprocess.run([compiler, *flags, "-fsyntax-only", "-I", os.path.dirname(HEADER), str(bad)],
                         capture_output=True, text=True)
    assert out.returncode != 0


def test_directed_sources_are_exact_inputs(shm, oracle):
    """Non-zero, finite, small; columns that are all negative, all positive
    and mixed; the same call gives the same bytes (the PE processes each
    regenerate all P sources)."""
    for t, op in shm.REFERENCE_PAIRS:
        s = et.directed_sources(t, op, et.NPES, et.NELEMS)
        assert s.shape == (et.NPES, et.NELEMS) and s.dtype == oracle.NP_DTYPE[t]
        assert s.tobytes() == et.directed_sources(t, op, et.NPES, et.NELEMS).tobytes()
        parts = [s.real, s.imag] if s.dtype.kind == "c" else [s]
        for x in parts:
            x = x.astype(np.float64)
            assert np.all(np.isfinite(x)) and np.all(x != 0) and np.all(np.abs(x) <= 9)
            assert np.all(x * 4 == np.round(x * 4))
            neg, pos = (x < 0).all(axis=0), (x > 0).all(axis=0)
            assert neg.sum() >= et.NELEMS // 3 and pos.sum() >= et.NELEMS // 3
            assert (~neg & ~pos).sum() >= et.NELEMS // 3 - 1


def test_discrimination_census(shm, oracle):
    """Every entry on every set: the oracle's result for the promised
    (type, op) against its result for every other pair of the same element
    size on the same source bytes.  At least 4 of the 67 elements differ on
    the promised type's value bytes, on every member, so a row wired to any
    other pair fails the bitwise GPU check; and every member of a set has the
    same reference bytes (order independence, which that check relies on).
    Only long against long long with the same op is exempt: one operation."""
    assert ("longlong", "sum") not in et.confusable("long", "sum")
    assert ("longlong", "prod") in et.confusable("long", "sum")
    assert ("long", "max") in et.confusable("double", "max") and ("complexf", "sum") in et.confusable("double", "max")
    assert sorted(et.confusable("complexd", "sum")) == sorted(
        [("complexd", "prod")] + [("longdouble", o) for o in ("sum", "prod", "min", "max")])
    worst, compared = None, 0
    for t, op in sorted({(e.type, e.op) for e in et.ENTRIES}):
        rows, order_free = et.census(t, op)
        assert order_free, f"{t} {op}: the members of a set differ in their reference bytes"
        assert len(rows) == len(et.SETS) * len(et.confusable(t, op)) and rows
        for st, other, d in rows:
            compared += 1
            if worst is None or d < worst[0]:
                worst = (d, (t, op), other, st)
    print(f"census: {compared} comparisons, minimum {worst[0]} of {et.NELEMS} elements differ "
          f"({worst[1]} against {worst[2]} on set {worst[3]})")
    assert worst[0] >= 4, worst
