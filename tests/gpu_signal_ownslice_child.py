"""One PE of test_gpu_signal_ownslice.py: P of these processes share the one
GPU and run SIGNAL's own slice for real across processes (the owner of a slice
folds it in every member's order inside the fused launch, or with the
P-order fold kernel between device barriers; the members pull their results
from the owners' IPC scratch), stream-ordered.

    SHMEM_PE=p SHMEM_NPES=P SHMEM_BOOTSTRAP_FILE=f python gpu_signal_ownslice_child.py OUT.json SCENARIO

Every call is checked, on every member, against the oracle's answer for that
PE and against the bits of the same call under `gather`; the bytes around the
target (guard words, and the source where it is not the target) must be as
before the call.  Writes a JSON report to OUT.json.
"""
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

PAIRS = [(t, o) for t in ("float", "double", "longdouble") for o in ("min", "max")]
MODES = ("heap", "inplace", "heap8")
GUARD, PAD = 0xAB, 64
CAP = 4 << 20
ARENA_A, ARENA_B = shm.malloc(CAP), shm.malloc(CAP)
ARENA_C, ARENA_D = shm.malloc(CAP), shm.malloc(CAP)     # the interleaved scenario's second call
assert ARENA_A and ARENA_B and ARENA_C and ARENA_D, "shmem_malloc failed"
fails, ncases, expected, differs = [], 0, 0, 0


def member(start, log, size):
    step = 1 << log
    return pe >= start and (pe - start) % step == 0 and (pe - start) // step < size


def place(mode, t, nb, arenas=(ARENA_A, ARENA_B)):
    """(source address, target address, [(region address, bytes)]) of one
    call's operands, all in the heap, each region PAD bytes wider than its
    array on both sides."""
    a, b = arenas
    if mode == "heap":
        return a + PAD, b + PAD, [(a, nb + 2 * PAD), (b, nb + 2 * PAD)]
    if mode == "heap8":      # off 16-byte alignment by 8 (long double: by one element)
        off = 16 if t == "longdouble" else 8
        return a + PAD + off, b + PAD + off, [(a, nb + 2 * PAD + off), (b, nb + 2 * PAD + off)]
    return a + PAD, a + PAD, [(a, nb + 2 * PAD)]            # inplace


def image(regions):
    out = []
    for p, nbytes in regions:
        a = np.empty(nbytes, np.uint8)
        shm.memcpy(a, p, nbytes)
        out.append(a)
    return out


def fill(regions, src, mine):
    for p, nbytes in regions:
        shm.memcpy(p, np.full(nbytes, GUARD, np.uint8), nbytes)
    shm.memcpy(src, mine, mine.nbytes)


def call(t, op, n, st, algo, mode, mine, stream=0):
    """One collective call from freshly filled regions: (the target's
    elements, the regions before, the regions after, tgt, regions, error)."""
    nb = n * mine.itemsize
    src, tgt, regions = place(mode, t, nb)
    fill(regions, src, mine)
    before = image(regions)
    err = 0
    try:
        shm.reduce_on_stream(t, op, tgt, src, n, *st, algo, stream)
    except shm.ShmemError as e:
        err = e.code
    torch.cuda.synchronize()
    after = image(regions)
    got = np.empty(n, mine.dtype)
    shm.memcpy(got, tgt, nb)
    return got, before, after, tgt, regions, err


def judge(tag, t, n, got, want, ref, before, after, tgt, regions, err):
    if err or shm.last_error():
        fails.append(f"{tag}: error {err} / last_error {shm.last_error()}")
        return
    if not same_bits(got, want):
        w = 10 if t == "longdouble" else got.itemsize
        bad = np.flatnonzero((got.view(np.uint8).reshape(n, -1)[:, :w] !=
                              want.view(np.uint8).reshape(n, -1)[:, :w]).any(axis=1))
        fails.append(f"{tag}: {len(bad)} elements differ from the oracle, first at {bad[:4].tolist()}")
    if ref is not None and not same_bits(got, ref):
        fails.append(f"{tag}: differs from the same call under gather")
    # everything outside the target as before the call: the guard bytes
    # around it, and the source where it is not the target
    nb = n * got.itemsize
    for (p, nbytes), b, a in zip(regions, before, after):
        keep = np.ones(nbytes, bool)
        if p <= tgt < p + nbytes:
            keep[tgt - p:tgt - p + nb] = False
        if not np.array_equal(a[keep], b[keep]):
            where = np.flatnonzero((a != b) & keep)
            fails.append(f"{tag}: {len(where)} bytes outside the target changed, first at region offset "
                         f"{where[:4].tolist()} (target at {tgt - p})")


def run_case(t, op, n, st, mode, seed, own_slice=True, stream=0):
    global ncases, expected, differs
    srcs = oracle.special_sources(t, npes, n, seed)
    if not member(*st):
        return
    ncases += 1
    tag = f"{t} {op} n={n} set={st} mode={mode}"
    print(tag, flush=True)
    mine = np.ascontiguousarray(srcs[pe])
    want = oracle.reduce_one(t, op, srcs, *st, pe)
    if st[0] == 0 and st[1] == 0:
        first = oracle.reduce_one(t, op, srcs, *st, st[0])
        w = 10 if t == "longdouble" else mine.itemsize
        differs += int((want.view(np.uint8).reshape(n, -1)[:, :w] !=
                        first.view(np.uint8).reshape(n, -1)[:, :w]).any(axis=1).sum())
    ref = call(t, op, n, st, "gather", mode, mine)[0]
    got, before, after, tgt, regions, err = call(t, op, n, st, "signal", mode, mine, stream)
    expected += own_slice
    judge(tag, t, n, got, want, ref, before, after, tgt, regions, err)


def sets():
    s = [(0, 0, npes)]
    if npes >= 8:
        s += [(0, 1, 4), (2, 0, 4)]      # strided: PEs 0, 2, 4, 6; an offset run: PEs 2..5
    return s


def rotate(seq, k, count):
    return [seq[(k + i) % len(seq)] for i in range(count)]


def sizes(t):
    return (1, 3, 1013, 20001 if t == "longdouble" else 70001)


seed = 0x51C5
if scenario in ("forced", "off"):
    # $SHMEMX_DIRECT_ONESHOT_KB=0: every size is above the one-shot limit.
    # 1 and 3 elements leave members without a slice.  The whole job sees
    # every operand placement with every pair and size; the partial sets of
    # the 8-PE run two placements per (pair, size), in rotation.  "off": the
    # same calls with the switch off take today's own-order route.
    assert os.environ.get("SHMEMX_DIRECT_ONESHOT_KB") == "0"
    assert (os.environ.get("SHMEMX_SIGNAL_OWNSLICE") == "1") == (scenario == "forced")
    k = 0
    for st in sets():
        for t, op in PAIRS:
            for n in sizes(t):
                for mode in (MODES if st[2] == npes else rotate(MODES, k, 2)):
                    seed += 1
                    run_case(t, op, n, st, mode, seed, scenario == "forced")
                k += 1
elif scenario == "unfused":
    # $SHMEMX_FUSED_TWOSHOT_KB=64: 70001 doubles take the five-launch schedule
    assert os.environ.get("SHMEMX_FUSED_TWOSHOT_KB") == "64"
    for op in ("min", "max"):
        for mode in MODES:
            seed += 1
            run_case("double", op, 70001, (0, 0, npes), mode, seed)
elif scenario == "chunks":
    # $SHMEMX_DIRECT_SCRATCH_MB=1: half a MiB of result slots, so 300 007
    # floats and 150 001 doubles (1.2 MB; slots of 0.8 MB) take several chunks
    assert os.environ.get("SHMEMX_DIRECT_SCRATCH_MB") == "1"
    assert os.environ.get("SHMEMX_FUSED_TWOSHOT_KB") == "0"
    for t, op in PAIRS[:4]:
        n = 300007 if t == "float" else 150001
        for mode in ("heap", "inplace"):
            seed += 1
            run_case(t, op, n, (0, 0, npes), mode, seed)
elif scenario == "graph":
    # a single-stream capture after a warm call (which allocates, publishes,
    # maps and votes on the scratch regions); every replay reduces fresh
    # special sources; the in-place capture needs no temporary
    stream = torch.cuda.Stream()
    n, st = 50000, (0, 0, npes)
    for mode in ("heap", "inplace"):
        src, tgt, regions = place(mode, "double", n * 8)
        torch.cuda.synchronize()
        shm.barrier_all()
        fill(regions, src, np.zeros(n, np.float64))
        shm.reduce_on_stream("double", "max", tgt, src, n, *st, "signal", stream.cuda_stream)   # warm
        torch.cuda.synchronize()
        expected += 1
        graph = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(graph, stream=stream):
                shm.reduce_on_stream("double", "max", tgt, src, n, *st, "signal", stream.cuda_stream)
        except shm.ShmemError as e:
            fails.append(f"graph {mode}: the capture was refused, error {e.code}")
            continue
        expected += 1
        for rep_i in range(5):
            seed += 1
            srcs = oracle.special_sources("double", npes, n, seed)
            mine = np.ascontiguousarray(srcs[pe])
            want = oracle.reduce_one("double", "max", srcs, *st, pe)
            differs += int((want.view(np.uint64) != oracle.reduce_one("double", "max", srcs, *st, 0)
                            .view(np.uint64)).sum())
            fill(regions, src, mine)
            before = image(regions)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            ncases += 1
            got = np.empty(n, np.float64)
            shm.memcpy(got, tgt, n * 8)
            judge(f"graph {mode} replay {rep_i}", "double", n, got, want, None, before, image(regions), tgt,
                  regions, 0)
        del graph
elif scenario == "interleaved":
    # a blocking OWNSLICE call (the library's stream, host barriers) right
    # behind a stream-ordered call of this route on another stream, which is
    # still running: both use the slot area, 20 rounds
    stream = torch.cuda.Stream()
    n, st = 70001, (0, 0, npes)
    for rnd in range(20):
        seed += 2
        s1 = oracle.special_sources("double", npes, n, seed)
        s2 = oracle.special_sources("double", npes, n, seed + 1)
        src1, tgt1, reg1 = place("heap" if rnd % 2 else "inplace", "double", n * 8)
        src2, tgt2, reg2 = place("heap", "double", n * 8, (ARENA_C, ARENA_D))
        fill(reg1, src1, np.ascontiguousarray(s1[pe]))
        fill(reg2, src2, np.ascontiguousarray(s2[pe]))
        b1, b2 = image(reg1), image(reg2)
        torch.cuda.synchronize()
        shm.barrier_all()
        err = 0
        try:
            shm.reduce_on_stream("double", "max", tgt1, src1, n, *st, "signal", stream.cuda_stream)
            shm.reduce_on_stream("double", "min", tgt2, src2, n, *st, "ownslice")
        except shm.ShmemError as e:
            err = e.code
        torch.cuda.synchronize()
        expected += 1
        ncases += 2
        for tag, op, srcs, tgt, reg, b in (("signal", "max", s1, tgt1, reg1, b1), ("ownslice", "min", s2, tgt2, reg2, b2)):
            got = np.empty(n, np.float64)
            shm.memcpy(got, tgt, n * 8)
            want = oracle.reduce_one("double", op, srcs, *st, pe)
            differs += int((want.view(np.uint64) != oracle.reduce_one("double", op, srcs, *st, 0).view(np.uint64)).sum())
            judge(f"interleaved round {rnd} {tag}", "double", n, got, want, None, b, image(reg), tgt, reg, err)
else:
    raise SystemExit(f"unknown scenario {scenario}")

stats = shm.direct_stats(reset=False)
shm.barrier_all()
shm.finalize()
with open(out_path, "w") as f:
    json.dump({"pe": pe, "fails": fails, "ncases": ncases, "expected": expected, "differs": differs,
               "signal_ownslice_calls": stats["signal_ownslice_calls"],
               "signal_ownslice_fused_calls": stats["signal_ownslice_fused_calls"],
               "ownslice_calls": stats["ownslice_calls"]}, f)
print(f"PE {pe}: {ncases} cases, {len(fails)} failures", flush=True)
sys.exit(1 if fails else 0)
