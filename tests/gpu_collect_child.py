"""One PE of test_gpu_collect.py: P of these processes share the one GPU and
run the stream-ordered collect for real across processes (the counts exchanged
through the members' heaps, the segments pulled over IPC mappings, under the
device barriers).

    SHMEM_PE=p SHMEM_NPES=P SHMEM_BOOTSTRAP_FILE=f python gpu_collect_child.py OUT.json SCENARIO

Every call is checked, on every member, against oracle.collect_sim with the
members' real counts; the whole target up to its capacity, the guard bytes
around it and the source must be as the oracle and the fill say.  Writes a
JSON report to OUT.json.
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

ENOTSUP = 3
ONES = (1 << 64) - 1
TYPE_OF = {32: "int", 64: "long"}
GUARD, PAD = 0xAB, 64
CAP = 1 << 20                                   # 70001 x 8 bytes and 8 short segments fit
ARENA_A, ARENA_B = shm.malloc(CAP), shm.malloc(CAP)
assert ARENA_A and ARENA_B, "shmem_malloc failed"
FUSED_BYTES = int(os.environ.get("SHMEMX_FUSED_TWOSHOT_KB", "4096")) << 10
fails, ncases = [], 0
expect = {"collects": 0, "fused_calls": 0, "overflows": 0}
# the counted form's operands: plain device memory outside the heap
count_dev = torch.zeros(1, dtype=torch.int64, device="cuda")
where_dev = torch.zeros(2, dtype=torch.int64, device="cuda")


def members(st):
    start, log, size = st
    return [start + i * (1 << log) for i in range(size)]


def image(regions):
    out = []
    for p, nbytes in regions:
        a = np.empty(nbytes, np.uint8)
        shm.memcpy(a, p, nbytes)
        out.append(a)
    return out


def collect_case(bits, counts, capacity, st, off, seed, counted, overflow=False):
    """counts[p]: PE p's count (every PE of the job has one; only the set's
    count).  off: bytes the operands lie past 16-byte alignment."""
    global ncases
    t, esz = TYPE_OF[bits], bits // 8
    maxn = max(1, max(counts))
    srcs = oracle.sources(t, 1, npes, maxn, seed)
    if pe not in members(st):
        return
    ncases += 1
    tag = f"collect{bits} counts={counts} capacity={capacity} set={st} off={off} counted={counted}"
    print(tag, flush=True)
    src, tgt = ARENA_A + PAD + off, ARENA_B + PAD + off
    regions = [(ARENA_A, maxn * esz + 2 * PAD + off), (ARENA_B, capacity * esz + 2 * PAD + off)]
    for p, nbytes in regions:
        shm.memcpy(p, np.full(nbytes, GUARD, np.uint8), nbytes)
    mine = np.ascontiguousarray(srcs[pe])
    shm.memcpy(src, mine, mine.nbytes)
    before = image(regions)
    guard = np.empty((npes, capacity), srcs.dtype)
    guard.view(np.uint8)[:] = GUARD
    mem = members(st)
    total = sum(counts[p] for p in mem)
    offset = sum(counts[p] for p in mem[:mem.index(pe)])
    want = guard[pe] if overflow else oracle.collect_sim(srcs, counts, guard, *st)[pe]
    expect["collects"] += 1
    expect["fused_calls"] += capacity * esz <= FUSED_BYTES
    expect["overflows"] += overflow
    try:
        if counted:
            count_dev.fill_(counts[pe])
            where_dev.fill_(0x77)
            torch.cuda.synchronize()
            shm.collect_counted_on_stream(bits, tgt, src, count_dev, where_dev, capacity, *st)
        else:
            shm.collect_on_stream(bits, tgt, src, counts[pe], capacity, *st)
    except shm.ShmemError as e:
        fails.append(f"{tag}: error {e.code}")
        return
    torch.cuda.synchronize()
    if shm.last_error():
        fails.append(f"{tag}: last_error {shm.last_error()}")
    got = np.empty(capacity, srcs.dtype)
    shm.memcpy(got, tgt, got.nbytes)
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got != want)
        fails.append(f"{tag}: {len(bad)} elements differ from the oracle, first at {bad[:4].tolist()}")
    if counted:
        where = [int(v) & ONES for v in where_dev.cpu().tolist()]
        if where != ([ONES, ONES] if overflow else [offset, total]):
            fails.append(f"{tag}: where {where}, offset {offset} total {total}")
    # everything outside the target as before the call: the guard bytes and the source
    for (p, nbytes), b, a in zip(regions, before, image(regions)):
        keep = np.ones(nbytes, bool)
        if p == ARENA_B:
            keep[tgt - p:tgt - p + got.nbytes] = False
        if not np.array_equal(a[keep], b[keep]):
            where_bad = np.flatnonzero((a != b) & keep)
            fails.append(f"{tag}: {len(where_bad)} bytes outside the target changed, first at region offset "
                         f"{where_bad[:4].tolist()}")


def sets():
    s = [(0, 0, npes)]
    if npes >= 8:
        s += [(0, 1, 4), (2, 0, 3)]      # strided: PEs 0, 2, 4, 6; an offset run: PEs 2, 3, 4
    return s


def count_patterns(st):
    """Counts per PE of the job: 17 pe + 1; the same with one member at zero;
    all zero; the same with one member at 70001."""
    mem = members(st)
    base = [17 * p + 1 for p in range(npes)]
    zero = list(base)
    zero[mem[len(mem) // 2]] = 0
    big = list(base)
    big[mem[1]] = 70001
    return [base, zero, [0] * npes, big]


def healthy_blocking_calls(seed):
    """The blocking calls after the scenario's last collect: shmem_int_sum_to_all
    and shmem_collect64 on the whole job."""
    global ncases
    n, st = 1013, (0, 0, npes)
    srcs = oracle.sources("int", 1, npes, n, seed)
    shm.memcpy(ARENA_A + PAD, np.ascontiguousarray(srcs[pe]), n * 4)
    shm.barrier_all()
    shm.to_all("int", "sum", ARENA_B + PAD, ARENA_A + PAD, n, *st)
    got = np.empty(n, np.int32)
    shm.memcpy(got, ARENA_B + PAD, n * 4)
    ncases += 1
    if shm.last_error() or got.tobytes() != oracle.reduce_sim("int", "sum", srcs, *st)[pe].tobytes():
        fails.append(f"the blocking int sum after the scenario: last_error {shm.last_error()}")
    shm.barrier_all()
    counts = [5 * p + 2 for p in range(npes)]
    lsrcs = oracle.sources("long", 1, npes, max(counts), seed + 1)
    guard = np.empty((npes, sum(counts)), np.int64)
    guard.view(np.uint8)[:] = GUARD
    shm.memcpy(ARENA_A + PAD, np.ascontiguousarray(lsrcs[pe]), lsrcs[pe].nbytes)
    shm.barrier_all()
    shm.collect(64, ARENA_B + PAD, ARENA_A + PAD, counts[pe], *st)
    got = np.empty(sum(counts), np.int64)
    shm.memcpy(got, ARENA_B + PAD, got.nbytes)
    ncases += 1
    if shm.last_error() or got.tobytes() != oracle.collect_sim(lsrcs, counts, guard, *st)[pe].tobytes():
        fails.append(f"the blocking collect64 after the scenario: last_error {shm.last_error()}")


seed = 0xC011
torch.cuda.synchronize()
shm.barrier_all()

if scenario == "route":
    k = 0
    for st in sets():
        for bits in (32, 64):
            for counts in count_patterns(st):
                for off in (0, 8):
                    seed += 1
                    k += 1
                    total = sum(counts[p] for p in members(st))
                    # the total fills the capacity exactly, or leaves room
                    capacity = max(4, total + (0 if k % 3 else 5))
                    collect_case(bits, counts, capacity, st, off, seed, counted=k % 2 == 0)
    # a one-member set (every PE its own): a copy of the member's own count through the same kernels, with no
    # peer; in the heap, and on plain device memory outside it
    for bits, counted in ((32, False), (64, True)):
        seed += 1
        counts = [1013 + p for p in range(npes)]
        collect_case(bits, counts, counts[pe] + 3, (pe, 0, 1), 8, seed, counted)
    t_src = torch.arange(100, dtype=torch.int64, device="cuda") + pe
    t_tgt = torch.full((128,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    shm.collect_on_stream(64, t_tgt, t_src, 100, 128, pe, 0, 1)
    torch.cuda.synchronize()
    expect["collects"] += 1
    expect["fused_calls"] += 1
    ncases += 1
    if not (torch.equal(t_tgt[:100], t_src) and bool((t_tgt[100:] == -1).all())) or shm.last_error():
        fails.append(f"one-member collect outside the heap: last_error {shm.last_error()}")
elif scenario == "unfused":
    # $SHMEMX_FUSED_TWOSHOT_KB=64 and capacities above it: publish, barrier,
    # plan, copy, barrier
    assert os.environ.get("SHMEMX_FUSED_TWOSHOT_KB") == "64"
    st = (0, 0, npes)
    for bits in (32, 64):
        for counts in count_patterns(st):
            for off in (0, 8):
                seed += 1
                capacity = max(sum(counts), (64 << 10) // (bits // 8) + 1)
                assert capacity * (bits // 8) > FUSED_BYTES
                collect_case(bits, counts, capacity, st, off, seed, counted=off == 8)
elif scenario == "graph":
    # after a warm call: {copy of the count from a pinned host word into
    # nelems_dev, collect64_counted, barrier} captured on one stream and
    # replayed with other counts and sources; the replay reads the count anew
    hip = ctypes.CDLL("libamdhip64.so.7")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    stream = torch.cuda.Stream()
    sid = stream.cuda_stream
    st, capacity, maxn = (0, 0, npes), 4000 * npes, 4000
    S, T = ARENA_A + PAD, ARENA_B + PAD
    host_count = torch.zeros(1, dtype=torch.int64).pin_memory()

    def step():
        rc = hip.hipMemcpyAsync(count_dev.data_ptr(), host_count.data_ptr(), 8, 1, sid)
        assert rc == 0, rc
        shm.collect_counted_on_stream(64, T, S, count_dev, where_dev, capacity, *st, sid)
        shm.barrier_on_stream(*st, sid)

    host_count[0] = 1
    shm.memcpy(S, np.zeros(maxn, np.int64), maxn * 8)
    shm.memcpy(T, np.zeros(capacity, np.int64), capacity * 8)
    torch.cuda.synchronize()
    shm.barrier_all()
    step()                                                        # warm: maps the peers
    torch.cuda.synchronize()
    shm.collect_stats(reset=True)
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph, stream=stream):
            step()
    except shm.ShmemError as e:
        fails.append(f"graph: the capture was refused, error {e.code}")
        graph = None
    expect.update(collects=1, fused_calls=1)                      # the call made while capturing
    guard = np.empty((npes, capacity), np.int64)
    guard.view(np.uint8)[:] = GUARD
    for rep in range(5 if graph else 0):
        seed += 1
        counts = [(1009 * (rep + 1) + 977 * p) % maxn if (rep + p) % 4 else 0 for p in range(npes)]
        srcs = oracle.sources("long", 1, npes, maxn, seed)
        want = oracle.collect_sim(srcs, counts, guard, *st)[pe]
        shm.memcpy(S, np.ascontiguousarray(srcs[pe]), maxn * 8)
        shm.memcpy(T, guard[pe], capacity * 8)
        where_dev.fill_(0x77)
        host_count[0] = counts[pe]
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        ncases += 1
        got = np.empty(capacity, np.int64)
        shm.memcpy(got, T, got.nbytes)
        if got.tobytes() != want.tobytes():
            bad = np.flatnonzero(got != want)
            fails.append(f"graph replay {rep}: counts {counts}: {len(bad)} elements differ, first at {bad[:4].tolist()}")
        where = where_dev.cpu().tolist()
        if where != [sum(counts[:pe]), sum(counts)]:
            fails.append(f"graph replay {rep}: counts {counts}: where {where}")
        if shm.last_error():
            fails.append(f"graph replay {rep}: last_error {shm.last_error()}")
    del graph
elif scenario == "overflow":
    # one PE's count pushes the total past the capacity; then one PE's count
    # alone is above it (that member publishes poison): every PE reads the
    # same overflow, an untouched target, an all-ones where; the next collect
    # and the blocking calls are healthy (a device-barrier error would abort
    # the first blocking call)
    st, capacity = (0, 0, npes), 1000
    over = [300] * npes
    over[npes - 1] = capacity - 300 * (npes - 1) + 1
    lone = [10] * npes
    lone[1] = capacity + 1
    fits = [300] * npes
    fits[npes - 1] = capacity - 300 * (npes - 1)
    for bits in (32, 64):
        for counted in (False, True):
            for counts, bad in ((over, True), (fits, False), (lone, True), (fits, False)):
                seed += 1
                collect_case(bits, counts, capacity, st, 0, seed, counted, overflow=bad)
    healthy_blocking_calls(seed + 100)
elif scenario == "mirrored":
    # $SHMEMX_HEAP_MEMORY=mirrored (the library's default): shmem_malloc
    # returns host-view addresses.  Host code writes the sources and the
    # guard bytes with plain stores, the call runs on the HBM twins, and host
    # code reads the target back (the load waits for the call's stream).
    assert os.environ.get("SHMEMX_HEAP_MEMORY") == "mirrored"

    def host_view(ptr, dtype, n):
        buf = (ctypes.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr)
        return np.frombuffer(buf, dtype=dtype, count=n)

    st, maxn = (0, 0, npes), 30001
    capacity = npes * maxn
    sv = host_view(ARENA_A + PAD, np.int64, maxn)
    tv = host_view(ARENA_B + PAD, np.int64, capacity)
    guard = np.empty((npes, capacity), np.int64)
    guard.view(np.uint8)[:] = GUARD
    for rnd in range(4):
        seed += 1
        counts = [maxn - 1000 * ((p + rnd) % npes) - rnd for p in range(npes)]
        srcs = oracle.sources("long", 1, npes, maxn, seed)
        want = oracle.collect_sim(srcs, counts, guard, *st)[pe]
        sv[:] = srcs[pe]
        tv[:] = guard[pe]
        if rnd % 2:
            count_dev.fill_(counts[pe])
            torch.cuda.synchronize()
            shm.collect_counted_on_stream(64, ARENA_B + PAD, ARENA_A + PAD, count_dev, None, capacity, *st)
        else:
            shm.collect_on_stream(64, ARENA_B + PAD, ARENA_A + PAD, counts[pe], capacity, *st)
        expect["collects"] += 1
        expect["fused_calls"] += 1
        got = tv.copy()
        ncases += 1
        if shm.last_error() or got.tobytes() != want.tobytes():
            bad = np.flatnonzero(got != want)
            fails.append(f"mirrored round {rnd}: last_error {shm.last_error()}, {len(bad)} elements differ, first at "
                         f"{bad[:4].tolist()}")
        if sv.tobytes() != srcs[pe].tobytes():
            fails.append(f"mirrored round {rnd}: the source changed")
        shm.barrier_on_stream(*st)
        torch.cuda.synchronize()
elif scenario == "refusal":
    # every member passes an operand outside the heap: ENOTSUP on every
    # member, nothing launched, and the next blocking calls are healthy
    st, n = (0, 0, npes), 1013
    private = torch.zeros(npes * n, dtype=torch.int64, device="cuda")
    heap_a, heap_b = ARENA_A + PAD, ARENA_B + PAD
    attempts = (("target", lambda: shm.collect_on_stream(64, private, heap_a, n, npes * n, *st)),
                ("source", lambda: shm.collect_on_stream(32, heap_b, private, n, npes * n, *st)),
                ("counted target", lambda: shm.collect_counted_on_stream(64, private, heap_a, count_dev, where_dev,
                                                                         npes * n, *st)),
                ("target's end", lambda: shm.collect_on_stream(64, ARENA_B + CAP - 64, heap_a, 4, 1 << 30, *st)))
    for what, attempt in attempts:
        ncases += 1
        try:
            attempt()
            fails.append(f"{what} outside the heap: the call was accepted")
        except shm.ShmemError as e:
            if e.code != ENOTSUP or shm.last_error() != ENOTSUP:
                fails.append(f"{what} outside the heap: error {e.code}, last_error {shm.last_error()}")
    torch.cuda.synchronize()
    healthy_blocking_calls(seed + 100)
else:
    raise SystemExit(f"unknown scenario {scenario}")

torch.cuda.synchronize()
stats = shm.collect_stats()
pull = shm.pull_stats()
shm.barrier_all()
shm.finalize()
with open(out_path, "w") as f:
    json.dump({"pe": pe, "fails": fails, "ncases": ncases, "expect": {k: int(v) for k, v in expect.items()},
               "stats": {k: int(v) for k, v in stats.items()}, "pull_keys": list(pull)}, f)
print(f"PE {pe}: {ncases} cases, {len(fails)} failures", flush=True)
sys.exit(1 if fails else 0)
