"""One PE of test_gpu_pull.py: P of these processes share the one GPU and run
the stream-ordered barrier, broadcast and fcollect for real across processes
(pulls from the peers' heaps over IPC mappings under the device barriers).

    SHMEM_PE=p SHMEM_NPES=P SHMEM_BOOTSTRAP_FILE=f python gpu_pull_child.py OUT.json SCENARIO

Every call is checked, on every member, against oracle.broadcast_sim /
oracle.collect_sim; the bytes around the target (guard bytes, and the source
where it is not the target) must be as before the call, and so must the root's
target.  Writes a JSON report to OUT.json.
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

out_path, scenario = sys.argv[1], sys.argv[2]
faulthandler.dump_traceback_later(90, repeat=True)
pe, npes = int(os.environ["SHMEM_PE"]), int(os.environ["SHMEM_NPES"])
torch.cuda.set_device(0)
shm.init()
assert shm.my_pe() == pe and shm.n_pes() == npes

ENOTMEMBER, ENOTSUP, EINVAL = 2, 3, 1
TYPE_OF = {32: "int", 64: "long"}
MODES = ("heap", "heap8", "inplace")
GUARD, PAD = 0xAB, 64
CAP = 6 << 20                                   # 8 x 70001 x 8 bytes of fcollect target fit
ARENA_A, ARENA_B = shm.malloc(CAP), shm.malloc(CAP)
assert ARENA_A and ARENA_B, "shmem_malloc failed"
FUSED_BYTES = int(os.environ.get("SHMEMX_FUSED_TWOSHOT_KB", "4096")) << 10
twophase_bytes = int(os.environ.get("SHMEMX_BCAST_TWOPHASE_KB", "2048")) << 10
fails, ncases = [], 0
expect = {"barriers": 0, "broadcasts": 0, "fcollects": 0, "fused_calls": 0, "twophase_broadcasts": 0}


def members(st):
    start, log, size = st
    return [start + i * (1 << log) for i in range(size)]


def place(mode, src_bytes, tgt_bytes):
    """(source address, target address, [(region address, bytes)]): all in
    the heap, each region PAD bytes wider than its array on both sides."""
    off = 8 if mode == "heap8" else 0               # 8 bytes off 16-byte alignment
    if mode == "inplace":
        return ARENA_A + PAD, ARENA_A + PAD, [(ARENA_A, tgt_bytes + 2 * PAD)]
    return (ARENA_A + PAD + off, ARENA_B + PAD + off,
            [(ARENA_A, src_bytes + 2 * PAD + off), (ARENA_B, tgt_bytes + 2 * PAD + off)])


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


def judge(tag, got, want, before, after, tgt, regions):
    if shm.last_error():
        fails.append(f"{tag}: last_error {shm.last_error()}")
        return
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got != want)
        fails.append(f"{tag}: {len(bad)} elements differ from the oracle, first at {bad[:4].tolist()}")
    # everything outside the target as before the call: the guard bytes
    # around it, and the source where it is not the target
    for (p, nbytes), b, a in zip(regions, before, after):
        keep = np.ones(nbytes, bool)
        if p <= tgt < p + nbytes:
            keep[tgt - p:tgt - p + got.nbytes] = False
        if not np.array_equal(a[keep], b[keep]):
            where = np.flatnonzero((a != b) & keep)
            fails.append(f"{tag}: {len(where)} bytes outside the target changed, first at region offset "
                         f"{where[:4].tolist()} (target at {tgt - p})")


def run_call(tag, issue, src, tgt, regions, mine, tgt_elems, want):
    """Fill, call, wait, compare.  issue(): the stream-ordered call."""
    global ncases
    ncases += 1
    print(tag, flush=True)
    fill(regions, src, mine)
    before = image(regions)
    try:
        issue()
    except shm.ShmemError as e:
        fails.append(f"{tag}: error {e.code}")
        return
    torch.cuda.synchronize()
    got = np.empty(tgt_elems, mine.dtype)
    shm.memcpy(got, tgt, got.nbytes)
    judge(tag, got, want, before, image(regions), tgt, regions)


def broadcast_case(bits, n, root, st, mode, seed, stream=0):
    t = TYPE_OF[bits]
    srcs = oracle.sources(t, 1, npes, n, seed)
    if pe not in members(st):
        return
    nb = n * (bits // 8)
    src, tgt, regions = place(mode, nb, nb)
    # what every PE's target holds before the call: guard bytes, or its source
    before_t = srcs.copy()
    if mode != "inplace":
        before_t.view(np.uint8)[:] = GUARD
    want = oracle.broadcast_sim(srcs, before_t, root, *st)[pe]
    if pe == members(st)[root]:
        assert want.tobytes() == before_t[pe].tobytes()     # the root's target is never written
    P = st[2]
    expect["broadcasts"] += 1
    expect["fused_calls"] += nb <= FUSED_BYTES
    expect["twophase_broadcasts"] += P > 2 and nb > twophase_bytes
    run_call(f"broadcast{bits} n={n} root={root} set={st} mode={mode}",
             lambda: shm.broadcast_on_stream(bits, tgt, src, n, root, *st, stream),
             src, tgt, regions, np.ascontiguousarray(srcs[pe]), n, want)


def fcollect_case(bits, n, st, mode, seed, stream=0):
    t = TYPE_OF[bits]
    srcs = oracle.sources(t, 1, npes, n, seed)
    if pe not in members(st):
        return
    P, nb = st[2], n * (bits // 8)
    src, tgt, regions = place(mode, nb, P * nb)
    before_t = np.full((npes, P * n), 0, srcs.dtype)
    before_t.view(np.uint8)[:] = GUARD
    want = oracle.collect_sim(srcs, [n] * npes, before_t, *st)[pe]
    expect["fcollects"] += 1
    expect["fused_calls"] += P * nb <= FUSED_BYTES
    run_call(f"fcollect{bits} n={n} set={st} mode={mode}",
             lambda: shm.fcollect_on_stream(bits, tgt, src, n, *st, stream),
             src, tgt, regions, np.ascontiguousarray(srcs[pe]), P * n, want)


def sets():
    s = [(0, 0, npes)]
    if npes >= 8:
        s += [(0, 1, 4), (2, 0, 3)]      # strided: PEs 0, 2, 4, 6; an offset run: PEs 2, 3, 4
    return s


SIZES = (1, 3, 1013, 70001)
seed = 0xB0CA

if scenario == "route":
    # every size, both widths, roots 0 and P - 1, every operand placement on
    # the whole job; the partial sets of the 8-PE run two placements per
    # (width, size), in rotation
    k = 0
    for st in sets():
        for bits in (32, 64):
            for n in SIZES:
                modes = MODES if st[2] == npes else [MODES[(k + j) % 3] for j in range(2)]
                k += 1
                for mode in modes:
                    for root in (0, st[2] - 1):
                        seed += 1
                        broadcast_case(bits, n, root, st, mode, seed)
                    if mode != "inplace":
                        seed += 1
                        fcollect_case(bits, n, st, mode, seed)
elif scenario == "unfused":
    # $SHMEMX_FUSED_TWOSHOT_KB=64: 70001 x 8 bytes take the unfused launches,
    # one phase (the default limit) and, with the limit at 0, two phases
    assert os.environ.get("SHMEMX_FUSED_TWOSHOT_KB") == "64"
    st = (0, 0, npes)
    for limit_kb in (twophase_bytes >> 10, 0):
        shm.set_bcast_twophase_kb(limit_kb)
        twophase_bytes = limit_kb << 10
        for mode in MODES:
            for root in (0, npes - 1):
                seed += 1
                broadcast_case(64, 70001, root, st, mode, seed)
            if mode != "inplace":
                seed += 1
                fcollect_case(64, 70001, st, mode, seed)
elif scenario == "graph":
    # after a warm call of each: fcollect -> SIGNAL long sum -> broadcast ->
    # barrier captured on one stream, replayed on fresh sources
    stream = torch.cuda.Stream()
    sid = stream.cuda_stream
    n, st, P, root = 5000, (0, 0, npes), npes, npes - 1
    S, F = ARENA_A + PAD, ARENA_A + (1 << 20)                   # source; fcollect target (P n longs)
    R, B = ARENA_B + PAD, ARENA_B + (1 << 20)                   # the sum; the broadcast's target
    zeros = np.zeros(P * n, np.int64)

    def step():
        shm.fcollect_on_stream(64, F, S, n, *st, sid)
        shm.reduce_on_stream("long", "sum", R, F, P * n, *st, "signal", sid)
        shm.broadcast_on_stream(64, B, R, P * n, root, *st, sid)
        shm.barrier_on_stream(*st, sid)

    for a in (S, F, R, B):
        shm.memcpy(a, zeros, zeros.nbytes if a != S else n * 8)
    torch.cuda.synchronize()
    shm.barrier_all()
    step()                                                        # warm: maps the peers
    torch.cuda.synchronize()
    shm.pull_stats(reset=True)
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph, stream=stream):
            step()
    except shm.ShmemError as e:
        fails.append(f"graph: the capture was refused, error {e.code}")
        graph = None
    expect.update(barriers=1, broadcasts=1, fcollects=1, fused_calls=2)   # the calls made while capturing
    for rep in range(5 if graph else 0):
        seed += 1
        srcs = oracle.sources("long", 1, npes, n, seed)
        guard = np.full((npes, P * n), 0, np.int64)
        guard.view(np.uint8)[:] = GUARD
        want_f = oracle.collect_sim(srcs, [n] * npes, guard, *st)
        want_r = oracle.reduce_sim("long", "sum", want_f, *st)
        want_b = oracle.broadcast_sim(want_r, guard, root, *st)
        shm.memcpy(S, np.ascontiguousarray(srcs[pe]), n * 8)
        for a in (F, R, B):
            shm.memcpy(a, guard[pe], P * n * 8)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        ncases += 1
        for name, a, want in (("fcollect", F, want_f), ("sum", R, want_r), ("broadcast", B, want_b)):
            got = np.empty(P * n, np.int64)
            shm.memcpy(got, a, got.nbytes)
            if got.tobytes() != want[pe].tobytes():
                bad = np.flatnonzero(got != want[pe])
                fails.append(f"graph replay {rep}: {name}: {len(bad)} elements differ, first at {bad[:4].tolist()}")
        if shm.last_error():
            fails.append(f"graph replay {rep}: last_error {shm.last_error()}")
    del graph
elif scenario == "barrier":
    # PE k writes a word into its heap block with a stream copy and calls the
    # barrier; its neighbour copies the word out of k's heap on its own
    # stream.  No host synchronisation between the write and the barrier; a
    # second barrier keeps round r + 1's write behind round r's read.
    hip = ctypes.CDLL("libamdhip64.so.7")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
                                   ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    ROUNDS, st = 20, (0, 0, npes)
    stream = torch.cuda.Stream()
    sid = stream.cuda_stream
    word = ARENA_A + PAD
    nb = (pe + 1) % npes
    theirs = shm.heap_ptr(word, nb)
    assert theirs, "the neighbour's heap is not mapped"

    def value(p, r):
        return (p + 1) * 1000003 + r * 7919

    vals = torch.tensor([value(pe, r) for r in range(ROUNDS)], dtype=torch.int64).pin_memory()
    outs = torch.zeros(ROUNDS, dtype=torch.int64).pin_memory()
    torch.cuda.synchronize()
    shm.barrier_all()
    for r in range(ROUNDS):
        rc = hip.hipMemcpyAsync(word, vals.data_ptr() + 8 * r, 8, 4, sid)
        shm.barrier_on_stream(*st, sid)
        rc |= hip.hipMemcpyAsync(outs.data_ptr() + 8 * r, theirs, 8, 4, sid)
        shm.barrier_on_stream(*st, sid)
        expect["barriers"] += 2
        if rc:
            fails.append(f"round {r}: hipMemcpyAsync failed ({rc})")
    torch.cuda.synchronize()
    ncases = ROUNDS
    for r in range(ROUNDS):
        if int(outs[r]) != value(nb, r):
            fails.append(f"round {r}: read {int(outs[r])} from PE {nb}'s heap, it wrote {value(nb, r)}")
elif scenario == "refusal":
    # every member passes an operand outside the heap: ENOTSUP on every
    # member, nothing launched, and the next blocking calls are healthy
    st = (0, 0, npes)
    n = 1013
    private = torch.zeros(npes * n, dtype=torch.int64, device="cuda")
    heap_a, heap_b = ARENA_A + PAD, ARENA_B + PAD
    torch.cuda.synchronize()
    shm.barrier_all()
    attempts = (("broadcast target", lambda: shm.broadcast_on_stream(64, private, heap_a, n, 0, *st)),
                ("broadcast source", lambda: shm.broadcast_on_stream(64, heap_b, private, n, 0, *st)),
                ("fcollect target", lambda: shm.fcollect_on_stream(64, private, heap_a, n, *st)),
                ("fcollect source", lambda: shm.fcollect_on_stream(32, heap_b, private, n, *st)))
    for what, attempt in attempts:
        ncases += 1
        try:
            attempt()
            fails.append(f"{what} outside the heap: the call was accepted")
        except shm.ShmemError as e:
            if e.code != ENOTSUP or shm.last_error() != ENOTSUP:
                fails.append(f"{what} outside the heap: error {e.code}, last_error {shm.last_error()}")
    # a set that reaches past the job; a caller outside the set
    try:
        shm.barrier_on_stream(0, 0, npes + 1)
        fails.append("a set past the job was accepted")
    except shm.ShmemError as e:
        if e.code != EINVAL:
            fails.append(f"a set past the job: error {e.code}")
    part = (0, 0, npes - 1)
    try:
        shm.barrier_on_stream(*part)
        if pe == npes - 1:
            fails.append("a caller outside the set was accepted")
        else:
            expect["barriers"] += npes - 1 > 1
    except shm.ShmemError as e:
        if pe != npes - 1 or e.code != ENOTMEMBER:
            fails.append(f"barrier on {part}: error {e.code}")
    torch.cuda.synchronize()
    # the next blocking calls are healthy
    srcs = oracle.sources("long", 1, npes, n, seed)
    guard = np.full((npes, n), 0, np.int64)
    guard.view(np.uint8)[:] = GUARD
    shm.memcpy(heap_a, np.ascontiguousarray(srcs[pe]), n * 8)
    shm.memcpy(heap_b, guard[pe], n * 8)
    shm.barrier_all()
    shm.broadcast(64, heap_b, heap_a, n, 1, *st)
    got = np.empty(n, np.int64)
    shm.memcpy(got, heap_b, n * 8)
    ncases += 1
    if shm.last_error() or got.tobytes() != oracle.broadcast_sim(srcs, guard, 1, *st)[pe].tobytes():
        fails.append(f"the blocking broadcast after the refusals: last_error {shm.last_error()}")
elif scenario == "mirrored":
    # $SHMEMX_HEAP_MEMORY=mirrored (the library's default): shmem_malloc
    # returns host-view addresses.  Host code writes the sources and the
    # guard bytes with plain stores, the calls run on the HBM twins, and host
    # code reads the targets back (the load waits for the call's stream).
    assert os.environ.get("SHMEMX_HEAP_MEMORY") == "mirrored"

    def host_view(ptr, dtype, n):
        buf = (ctypes.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr)
        return np.frombuffer(buf, dtype=dtype, count=n)

    st, n = (0, 0, npes), 70001
    sv = host_view(ARENA_A + PAD, np.int64, n)
    tv = host_view(ARENA_B + PAD, np.int64, npes * n)
    guard = np.empty((npes, npes * n), np.int64)
    guard.view(np.uint8)[:] = GUARD
    for rnd in range(3):
        seed += 1
        root, two = rnd % npes, rnd % 2 == 1
        shm.set_bcast_twophase_kb(0 if two else 2048)
        srcs = oracle.sources("long", 1, npes, n, seed)
        for what in ("broadcast", "fcollect"):
            sv[:] = srcs[pe]
            tv[:] = guard[pe]
            if what == "broadcast":
                want = oracle.broadcast_sim(srcs, guard[:, :n], root, *st)[pe]
                shm.broadcast_on_stream(64, ARENA_B + PAD, ARENA_A + PAD, n, root, *st)
                expect["broadcasts"] += 1
                expect["twophase_broadcasts"] += two and npes > 2
            else:
                want = oracle.collect_sim(srcs, [n] * npes, guard, *st)[pe]
                shm.fcollect_on_stream(64, ARENA_B + PAD, ARENA_A + PAD, n, *st)
                expect["fcollects"] += 1
            expect["fused_calls"] += 1
            got = tv[:len(want)].copy()
            ncases += 1
            if shm.last_error() or got.tobytes() != want.tobytes():
                bad = np.flatnonzero(got != want)
                fails.append(f"mirrored {what} round {rnd}: last_error {shm.last_error()}, {len(bad)} elements "
                             f"differ, first at {bad[:4].tolist()}")
            if sv.tobytes() != srcs[pe].tobytes():
                fails.append(f"mirrored {what} round {rnd}: the source changed")
            shm.barrier_on_stream(*st)
            expect["barriers"] += 1
            torch.cuda.synchronize()
else:
    raise SystemExit(f"unknown scenario {scenario}")

stats = shm.pull_stats()
torch.cuda.synchronize()
shm.barrier_all()
shm.finalize()
with open(out_path, "w") as f:
    json.dump({"pe": pe, "fails": fails, "ncases": ncases, "expect": {k: int(v) for k, v in expect.items()},
               "stats": {k: int(v) for k, v in stats.items()}}, f)
print(f"PE {pe}: {ncases} cases, {len(fails)} failures", flush=True)
sys.exit(1 if fails else 0)
