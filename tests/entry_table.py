"""The typed stream-ordered forms and the Fortran forwarders of
openshmem-async_amd/csrc/entry.cpp, restated: which exported symbol promises
which (type, op).  Shared by tests/test_entry_table.py (CPU: counts, header,
aliases, prototypes and the discrimination census) and the PE processes of
tests/test_gpu_entry_points.py (tests/gpu_entry_child.py).  Needs no GPU and
does not read entry.cpp: a wrong row there must disagree with this list.

directed_sources() gives inputs on which the promised reduction is exact and
independent of the fold order, so every member of a set has the same
reference bits on every algorithm and the GPU comparison is bitwise, and on
which every other reduction of the same element size gives other bytes
(confusable(), differing(): the census)."""
import zlib
from collections import namedtuple

import numpy as np

import oracle
import shmem_mi355x as shm

Entry = namedtuple("Entry", "symbol kind type op")   # kind: "stream" or "fortran"

# Fortran kind -> the C type its forwarder promises (fortran.c:1003-1054)
FORTRAN_KINDS = {"int2": "short", "int4": "int", "int8": "long", "real4": "float", "real8": "double",
                 "real16": "longdouble", "comp4": "complexf", "comp8": "complexd"}
FORTRAN_REAL = ("int2", "int4", "int8", "real4", "real8", "real16")
FORTRAN_INT = ("int2", "int4", "int8")
FORTRAN_COMPLEX = ("comp4", "comp8")

STREAM_ENTRIES = [Entry(f"shmemx_{t}_{op}_to_all_on_stream", "stream", t, op) for t, op in shm.REFERENCE_PAIRS]
FORTRAN_ENTRIES = (
    [Entry(f"shmem_{f}_{op}_to_all_", "fortran", FORTRAN_KINDS[f], op)
     for op in ("sum", "prod", "max", "min") for f in FORTRAN_REAL] +
    [Entry(f"shmem_{f}_{op}_to_all_", "fortran", FORTRAN_KINDS[f], op)
     for op in ("and", "or", "xor") for f in FORTRAN_INT] +
    [Entry(f"shmem_{f}_{op}_to_all_", "fortran", FORTRAN_KINDS[f], op)
     for op in ("sum", "prod") for f in FORTRAN_COMPLEX])
ENTRIES = STREAM_ENTRIES + FORTRAN_ENTRIES

# The shape and the active sets of the multi-PE run: 67 elements (a scalar
# head and tail around a vector body) on 3 PEs; the whole job, PEs {0, 2} and
# PEs {1, 2}.  The last two are each other's image under a swap of PE_start
# and logPE_stride.
NPES, NELEMS = 3, 67
SETS = ((0, 0, 3), (0, 1, 2), (1, 0, 2))

C_TYPE = {"short": "short", "int": "int", "long": "long", "longlong": "long long", "float": "float",
          "double": "double", "longdouble": "long double", "complexd": "SHMEMX_COMPLEX(double)",
          "complexf": "SHMEMX_COMPLEX(float)"}


def spellings(e):
    """The exported names of an entry: a Fortran forwarder has a pshmem_
    strong name and a weak shmem_ alias, a typed stream form one name."""
    return (e.symbol, "p" + e.symbol) if e.kind == "fortran" else (e.symbol,)


def all_symbols():
    return sorted(s for e in ENTRIES for s in spellings(e))


def members(st):
    start, log, size = st
    return [start + (i << log) for i in range(size)]


def c_prototype(e, name, declarator):
    """`declarator` (a function-pointer declarator such as "(*p0)") with the
    type the header promises for entry e."""
    T = C_TYPE[e.type]
    if e.kind == "stream":
        return f"int {declarator}({T} *, const {T} *, int, int, int, int, void *) = {name};"
    return f"void {declarator}({T} *, {T} *, int *, int *, int *, int *, {T} *, int *) = {name};"


def value_width(t):
    """The bytes of an element that hold its value: 10 of a long double's 16."""
    return 10 if t == "longdouble" else np.dtype(oracle.NP_DTYPE[t]).itemsize


def _signed_small(rng, P, n, bound):
    """[P, n] non-zero integers of magnitude 1..bound.  Column i: every PE
    negative (i % 3 == 0), every PE positive (i % 3 == 1), mixed signs
    otherwise; the magnitudes of a column are distinct while bound allows, and
    the PE that holds the largest varies from column to column."""
    k = np.empty((P, n), np.int64)
    for i in range(n):
        mag = rng.permutation(bound)[:P] + 1 if bound >= P else rng.integers(1, bound + 1, P)
        if i % 3 == 0:
            sign = -np.ones(P, np.int64)
        elif i % 3 == 1:
            sign = np.ones(P, np.int64)
        else:
            sign = np.where(rng.integers(0, 2, P) == 1, 1, -1)
            if abs(sign.sum()) == P:          # all alike: flip one
                sign[rng.integers(0, P)] *= -1
        k[:, i] = sign * mag
    return k


def directed_sources(t, op, P, n):
    """[P, n] sources of type t for op: small non-zero integers, k/4 for the
    floating types, a/2 + i b/2 for the complex ones.  Sums, products (at most
    bound^P <= 32767: no overflow in a short, exact in a float), minima, maxima
    and the bitwise ops of them are exact, so the result does not depend on the
    fold order; no NaN, no zero.  A long double's 6 padding bytes are zero."""
    assert 1 <= P <= 8 and (t, op) in shm.REFERENCE_PAIRS
    rng = np.random.default_rng(zlib.crc32(f"{t}/{op}/{P}/{n}".encode()))
    bound = 9 if op != "prod" else max(2, min(9, int(32767 ** (1.0 / P))))
    dt = np.dtype(oracle.NP_DTYPE[t])
    a = _signed_small(rng, P, n, bound)
    if t in ("complexd", "complexf"):
        b = _signed_small(rng, P, n, bound)
        out = np.empty((P, n), dt)
        out.real, out.imag = a / 2.0, b / 2.0
    elif dt.kind == "f":
        out = (a.astype(dt) / dt.type(4)).astype(dt)
    else:
        out = a.astype(dt)
    if t == "longdouble":
        out.view(np.uint8).reshape(P, n, dt.itemsize)[:, :, 10:] = 0
    return np.ascontiguousarray(out)


def confusable(t, op):
    """Every other pair of REFERENCE_PAIRS an entry promising (t, op) could be
    wired to unnoticed by the element size: the same size, another type or op.
    long and long long with the same op are the same operation."""
    size = np.dtype(oracle.NP_DTYPE[t]).itemsize
    same = {"long": "longlong", "longlong": "long"}
    return [(t2, op2) for t2, op2 in shm.REFERENCE_PAIRS
            if np.dtype(oracle.NP_DTYPE[t2]).itemsize == size and (t2, op2) != (t, op)
            and not (op2 == op and same.get(t) == t2)]


def reference(t, op, srcs, st):
    """[npes, n]: every PE's target after the reduction on set st (members'
    rows hold the result, the others zeros)."""
    return oracle.reduce_sim(t, op, srcs, *st)


def differing(t, a, b):
    """How many elements of a and b (same bytes per element) differ on the
    value bytes of type t."""
    w, size = value_width(t), np.dtype(oracle.NP_DTYPE[t]).itemsize
    a8 = np.ascontiguousarray(a).view(np.uint8).reshape(-1, size)[:, :w]
    b8 = np.ascontiguousarray(b).view(np.uint8).reshape(-1, size)[:, :w]
    return int((a8 != b8).any(axis=1).sum())


def census(t, op, P=NPES, n=NELEMS, sets=SETS):
    """For (t, op) on directed_sources: [(set, other pair, elements of the n
    where the other pair's result on the same source bytes differs from the
    promised one on the promised type's value bytes: the fewest over the
    set's members, each holding its own result of the other pair)], and
    whether every member of every set has the same reference bytes."""
    srcs = directed_sources(t, op, P, n)
    rows, order_free = [], True
    for st in sets:
        m = members(st)
        ref = reference(t, op, srcs, st)
        order_free &= all(differing(t, ref[m[0]], ref[q]) == 0 for q in m)
        for t2, op2 in confusable(t, op):
            alt = reference(t2, op2, srcs.view(oracle.NP_DTYPE[t2]), st)
            rows.append((st, (t2, op2), min(differing(t, ref[q], alt[q]) for q in m)))
    return rows, order_free
