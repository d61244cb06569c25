"""One PE of test_gpu_reduce_scatter.py: P of these processes share the one GPU
and run the stream-ordered reduce-scatter for real across processes (block m
of every member's source folded over IPC mappings, under the device barriers).

    SHMEM_PE=p SHMEM_NPES=P SHMEM_BOOTSTRAP_FILE=f python gpu_reduce_scatter_child.py OUT.json SCENARIO

Every call is checked, on every member, bit for bit against
oracle.reduce_one(type, op, blocks, 0, 0, P, pe=0) on the [P, nelems] array of
the members' block m (PE 0's order is set order); the guard bytes around the
target and the whole source must be as before the call.  Writes a JSON report
to OUT.json.
"""
import ctypes
import faulthandler
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "openshmem-async_amd"))
sys.path.insert(0, os.path.join(REPO, "oracle"))
import oracle  # noqa: E402
import shmem_mi355x as shm  # noqa: E402
from gpu_util import same_bits  # noqa: E402

out_path, scenario = sys.argv[1], sys.argv[2]
faulthandler.dump_traceback_later(90, repeat=True)
pe, npes = int(os.environ["SHMEM_PE"]), int(os.environ["SHMEM_NPES"])
torch.cuda.set_device(0)
shm.init()
assert shm.my_pe() == pe and shm.n_pes() == npes

ENOTSUP = 3
SPECIAL = 2
GUARD, PAD = 0xAB, 64
CAP = 1 << 20
ARENA = [shm.malloc(CAP) for _ in range(4)]     # source, target / slices, gathered, SIGNAL's answer
assert all(ARENA), "shmem_malloc failed"
A, B, C, D = (p + PAD for p in ARENA)
FUSED_BYTES = int(os.environ.get("SHMEMX_FUSED_TWOSHOT_KB", "4096")) << 10
fails, ncases = [], 0
expect = {"calls": 0, "fused_calls": 0}


def members(st):
    start, log, size = st
    return [start + i * (1 << log) for i in range(size)]


def read(ptr, dtype, n):
    a = np.empty(n, dtype)
    shm.memcpy(a, ptr, a.nbytes)
    return a


def sources_of(t, kind, P, n, seed):
    """[P, P * n]: the whole source of every member of the set, in set order."""
    if kind == SPECIAL:
        return oracle.special_sources(t, P, P * n, seed)
    return np.stack([oracle.fill(t, kind, seed + k, P * n) for k in range(P)])


def want_of(t, op, srcs, m, n):
    P = len(srcs)
    blocks = np.ascontiguousarray(srcs[:, m * n:(m + 1) * n])
    return oracle.reduce_one(t, op, blocks, 0, 0, P, 0)


def count(P, n, sz):
    expect["calls"] += 1
    expect["fused_calls"] += P > 1 and P * n * sz <= FUSED_BYTES


def case(t, op, n, st, seed, kind=1, off=0):
    """One call of the set st; off: bytes both operands lie past 16-byte
    alignment.  A PE outside the set makes no call and keeps its heap."""
    global ncases
    dt = np.dtype(oracle.NP_DTYPE[t])
    sz, mem = dt.itemsize, members(st)
    P = len(mem)
    srcs = np.ascontiguousarray(sources_of(t, kind, P, n, seed), dtype=dt)
    tag = f"{t} {op} n={n} set={st} kind={kind} off={off}"
    regions = [(ARENA[0], P * n * sz + 2 * PAD + off), (ARENA[1], n * sz + 2 * PAD + off)]
    for p, nbytes in regions:
        shm.memcpy(p, np.full(nbytes, GUARD, np.uint8), nbytes)
    torch.cuda.synchronize()
    ncases += 1
    if pe not in mem:
        return regions
    print(tag, flush=True)
    m = mem.index(pe)
    src, tgt = A + off, B + off
    shm.memcpy(src, srcs[m], srcs[m].nbytes)
    before = [read(p, np.uint8, nbytes) for p, nbytes in regions]
    count(P, n, sz)
    try:
        shm.reduce_scatter_on_stream(t, op, tgt, src, n, *st)
    except shm.ShmemError as e:
        fails.append(f"{tag}: error {e.code}")
        return regions
    torch.cuda.synchronize()
    if shm.last_error():
        fails.append(f"{tag}: last_error {shm.last_error()}")
    got, want = read(tgt, dt, n), want_of(t, op, srcs, m, n)
    if not same_bits(got, want):
        fails.append(f"{tag}: member {m}'s target differs from the oracle")
    for (p, nbytes), b in zip(regions, before):
        a = read(p, np.uint8, nbytes)
        keep = np.ones(nbytes, bool)
        if p == ARENA[1]:
            keep[tgt - p:tgt - p + n * sz] = False
        if not np.array_equal(a[keep], b[keep]):
            bad = np.flatnonzero((a != b) & keep)
            fails.append(f"{tag}: {len(bad)} bytes outside the target changed, first at region offset "
                         f"{bad[:4].tolist()}")
    return regions


def host_barrier():
    torch.cuda.synchronize()
    shm.barrier_all()


seed = 0x5CA7
host_barrier()

if scenario == "routes":
    # $SHMEMX_FUSED_TWOSHOT_KB=64 keeps both routes small: below the limit on
    # the source's bytes one launch, above it five
    assert FUSED_BYTES == 64 << 10
    st = (0, 0, npes)
    for t in ("int", "double", "longdouble"):
        sz = np.dtype(oracle.NP_DTYPE[t]).itemsize
        at = FUSED_BYTES // (npes * sz)
        for op in ("sum", "min"):
            kind = SPECIAL if op == "min" and t != "int" else 1
            # fused: 16-byte aligned blocks, and an odd count (odd blocks off a boundary for int, a tail for all);
            # unfused: the same above the limit
            for n in (min(1024, at), min(1024, at) - 5, at + 16, at + 13):
                seed += 16
                case(t, op, n, st, seed, kind=kind)
    seed += 16
    case("double", "sum", 1024, st, seed, off=8)          # both operands 8 bytes off: the element loop
    # every PE's own one-member set: one copy, in the heap and outside it
    seed += 16
    case("double", "sum", 1013, (pe, 0, 1), seed + pe)
    t_src = torch.arange(100, dtype=torch.int64, device="cuda") + pe
    t_tgt = torch.full((100,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    shm.reduce_scatter_on_stream("long", "xor", t_tgt, t_src, 100, pe, 0, 1)
    torch.cuda.synchronize()
    count(1, 100, 8)
    ncases += 1
    if not torch.equal(t_tgt, t_src) or shm.last_error():
        fails.append(f"one-member reduce-scatter outside the heap: last_error {shm.last_error()}")
    # nothing to fold: nothing launched, nothing counted
    shm.reduce_scatter_on_stream("int", "sum", B, A, 0, *st)
elif scenario == "partial":
    # a set that leaves one PE out: it makes no call and its heap keeps its bytes
    st = (1, 0, 2) if npes == 3 else (0, 1, 2)
    outsider = pe not in members(st)
    regions = []
    for t, op, n in (("int", "sum", 1027), ("double", "min", 1024), ("longdouble", "sum", 300),
                     ("double", "sum", FUSED_BYTES // 16 + 8)):
        seed += 16
        regions = case(t, op, n, st, seed, kind=SPECIAL if op == "min" else 1)
        host_barrier()
        if outsider:
            for p, nbytes in regions:
                if not bool((read(p, np.uint8, nbytes) == GUARD).all()):
                    fails.append(f"{t} {op} n={n}: the non-member's heap changed")
elif scenario == "identity":
    # reduce_scatter into the slice buffer, then fcollect64 of the slices ==
    # SIGNAL's allreduce of the same sources, bit for bit.  The slice buffer
    # is a symmetric object of its own (the same offset on every member), as
    # fcollect's source must be: member m's slice is slice m of the gathered
    # array, not of a buffer that holds them all.
    st, n = (0, 0, npes), 1536
    for op in ("sum", "xor"):
        for nn in (n, n + 1):
            seed += 16
            srcs = sources_of("long", 1, npes, nn, seed)
            shm.memcpy(A, np.ascontiguousarray(srcs[pe]), srcs[pe].nbytes)
            for p in (B, C, D):
                shm.memcpy(p, np.full(npes * nn * 8, GUARD, np.uint8), npes * nn * 8)
            torch.cuda.synchronize()
            count(npes, nn, 8)
            shm.reduce_scatter_on_stream("long", op, B, A, nn, *st)
            shm.fcollect_on_stream(64, C, B, nn, *st)
            shm.reduce_on_stream("long", op, D, A, npes * nn, *st, algo="signal")
            torch.cuda.synchronize()
            ncases += 1
            two, one = read(C, np.int64, npes * nn), read(D, np.int64, npes * nn)
            want = oracle.reduce_one("long", op, srcs, 0, 0, npes, 0)
            if shm.last_error() or two.tobytes() != one.tobytes() or one.tobytes() != want.tobytes():
                fails.append(f"identity long {op} n={nn}: last_error {shm.last_error()}, reduce_scatter + fcollect64 "
                             f"{'==' if two.tobytes() == one.tobytes() else '!='} SIGNAL, SIGNAL "
                             f"{'==' if one.tobytes() == want.tobytes() else '!='} the oracle")
elif scenario == "graph":
    # after a warm call: {reduce_scatter, a fold of a bias into the slice (the
    # caller's own kernel between the halves), fcollect64, barrier} captured
    # on one stream, a linear chain, and replayed on fresh sources
    stream = torch.cuda.Stream()
    sid = stream.cuda_stream
    st, n = (0, 0, npes), 2050
    mine = B                          # the slice: a symmetric object, as fcollect's source must be
    bias_dev = torch.zeros(n, dtype=torch.float64, device="cuda")

    def step():
        shm.reduce_scatter_on_stream("double", "sum", mine, A, n, *st, sid)
        shm.fold("double", "sum", mine, bias_dev, n, sid)
        shm.fcollect_on_stream(64, C, mine, n, *st, sid)
        shm.barrier_on_stream(*st, sid)

    shm.memcpy(A, np.zeros(npes * n), npes * n * 8)
    host_barrier()
    with torch.cuda.stream(stream):
        step()                                                        # warm: maps the peers
    torch.cuda.synchronize()
    shm.reduce_scatter_stats(reset=True)
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph, stream=stream):
            step()
    except shm.ShmemError as e:
        fails.append(f"graph: the capture was refused, error {e.code}")
        graph = None
    count(npes, n, 8)                                                 # the call made while capturing
    for rep in range(4 if graph else 0):
        seed += 32
        srcs = sources_of("double", 1, npes, n, seed)
        bias = np.stack([oracle.fill("double", 1, seed + 16 + k, n) for k in range(npes)])
        want = np.concatenate([
            oracle.reduce_one("double", "sum", np.stack([want_of("double", "sum", srcs, k, n), bias[k]]), 0, 0, 2, 0)
            for k in range(npes)])
        shm.memcpy(A, np.ascontiguousarray(srcs[pe]), srcs[pe].nbytes)
        shm.memcpy(C, np.full(npes * n * 8, GUARD, np.uint8), npes * n * 8)
        bias_dev.copy_(torch.from_numpy(bias[pe]))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        ncases += 1
        got = read(C, np.float64, npes * n)
        if shm.last_error() or got.tobytes() != want.tobytes():
            bad = np.flatnonzero(got.view(np.int64) != want.view(np.int64))
            fails.append(f"graph replay {rep}: last_error {shm.last_error()}, {len(bad)} elements differ, first at "
                         f"{bad[:4].tolist()}")
    del graph
elif scenario == "mirrored":
    # $SHMEMX_HEAP_MEMORY=mirrored (the library's default): shmem_malloc
    # returns host-view addresses.  Host code writes the source with plain
    # stores, the call runs on the HBM twins, and host code reads the target
    # back (the load waits for the call's stream).
    assert os.environ.get("SHMEMX_HEAP_MEMORY") == "mirrored"

    def host_view(ptr, dtype, n):
        buf = (ctypes.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr)
        return np.frombuffer(buf, dtype=dtype, count=n)

    st = (0, 0, npes)
    for rnd, n in enumerate((30001, 1024, 30001, 7)):
        seed += 16
        sv, tv = host_view(A, np.float64, npes * n), host_view(B, np.float64, n)
        srcs = sources_of("double", 1, npes, n, seed)
        sv[:] = srcs[pe]
        tv.view(np.uint8)[:] = GUARD
        count(npes, n, 8)
        shm.reduce_scatter_on_stream("double", "sum", B, A, n, *st)
        got = tv.copy()
        ncases += 1
        if shm.last_error() or got.tobytes() != want_of("double", "sum", srcs, pe, n).tobytes():
            fails.append(f"mirrored round {rnd}: last_error {shm.last_error()}, the target differs from the oracle")
        if sv.tobytes() != srcs[pe].tobytes():
            fails.append(f"mirrored round {rnd}: the source changed")
        shm.barrier_on_stream(*st)
        torch.cuda.synchronize()
elif scenario == "refusal":
    # every member passes an operand outside the heap: ENOTSUP on every
    # member, nothing launched, nothing counted, and a healthy call follows
    st, n = (0, 0, npes), 1013
    private = torch.zeros(npes * n, dtype=torch.int64, device="cuda")
    attempts = (("source", lambda: shm.reduce_scatter_on_stream("long", "sum", B, private, n, *st)),
                ("target", lambda: shm.reduce_scatter_on_stream("long", "sum", private, A, n, *st)))
    for what, attempt in attempts:
        ncases += 1
        try:
            attempt()
            fails.append(f"{what} outside the heap: the call was accepted")
        except shm.ShmemError as e:
            if e.code != ENOTSUP or shm.last_error() != ENOTSUP:
                fails.append(f"{what} outside the heap: error {e.code}, last_error {shm.last_error()}")
    host_barrier()
    case("long", "sum", n, st, seed + 16)
    case("double", "max", 1024, st, seed + 32, kind=SPECIAL)
else:
    raise SystemExit(f"unknown scenario {scenario}")

torch.cuda.synchronize()
stats = shm.reduce_scatter_stats()
pull = shm.pull_stats()
shm.barrier_all()
shm.finalize()
with open(out_path, "w") as f:
    json.dump({"pe": pe, "fails": fails, "ncases": ncases, "expect": {k: int(v) for k, v in expect.items()},
               "stats": {k: int(v) for k, v in stats.items()}, "pull_keys": list(pull)}, f)
print(f"PE {pe}: {ncases} cases, {len(fails)} failures", *fails[:10], sep="\n", flush=True)
sys.exit(1 if fails else 0)
