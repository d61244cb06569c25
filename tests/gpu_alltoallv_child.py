"""One PE of test_gpu_alltoallv.py: P of these processes share the one GPU and
run the stream-ordered alltoall / alltoallv for real across processes (the
count and offset tables read from the members' heaps, the blocks pulled over
IPC mappings, under the device barriers).

    SHMEM_PE=p SHMEM_NPES=P SHMEM_BOOTSTRAP_FILE=f python gpu_alltoallv_child.py OUT.json SCENARIO[,SCENARIO...]

Every call is checked, on every member, against a numpy model below: every PE
derives every member's source and tables from the case's seed, so it knows
what it must receive.  The whole target up to its capacity, the guard bytes
around it, the source and where_dev must be as the model says.  Writes a JSON
report to OUT.json.
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
import shmem_mi355x as shm  # noqa: E402

out_path, scenarios = sys.argv[1], sys.argv[2].split(",")
faulthandler.dump_traceback_later(90, repeat=True)
pe, npes = int(os.environ["SHMEM_PE"]), int(os.environ["SHMEM_NPES"])
torch.cuda.set_device(0)
shm.init()
assert shm.my_pe() == pe and shm.n_pes() == npes

ENOTSUP = 3
ONES = (1 << 64) - 1
DTYPE = {32: np.uint32, 64: np.uint64}
GUARD, PAD = 0xAB, 64
CAP = 2 << 20                                   # 70001 x 8 bytes and 15 short blocks fit a source
ARENA_S, ARENA_T, TAB = shm.malloc(CAP), shm.malloc(CAP), shm.malloc(4096)
assert ARENA_S and ARENA_T and TAB, "shmem_malloc failed"
COUNTS, OFFSETS, WHERE, SUM_OUT = TAB, TAB + 512, TAB + 1024, TAB + 2048      # 8-byte words in the heap
DEFAULT_KB = shm.set_fused_twoshot_kb(4096)
shm.set_fused_twoshot_kb(DEFAULT_KB)
fused_bytes = DEFAULT_KB << 10
fails, ncases = [], 0
expect = {"alltoalls": 0, "alltoallvs": 0, "fused_calls": 0, "overflows": 0}
where_private = torch.zeros(17, dtype=torch.int64, device="cuda")     # where_dev outside the heap


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


def source_of(bits, i, n, seed):
    """Member i's source of case `seed`: the same on every PE."""
    rng = np.random.default_rng([seed, i, bits])
    return rng.integers(0, np.iinfo(DTYPE[bits]).max, n, dtype=DTYPE[bits], endpoint=True)


def rows_of(counts, unit=1):
    """Offsets for a P x P count matrix: sender i lays its blocks out in
    descending receiver order, rotated by i, with gaps: non-monotonic and
    non-contiguous.  Returns (offsets, the elements the longest row needs)."""
    P = len(counts)
    offsets, need = [[0] * P for _ in range(P)], 1
    for i in range(P):
        at = 0
        for r in range(P):
            j = (i - r) % P
            at += ((i + 2 * j) % 3) * unit
            offsets[i][j] = at
            at += (counts[i][j] + unit - 1) // unit * unit
        need = max(need, at)
    return offsets, need


def model(bits, counts, offsets, capacity, src_capacity, m, seed):
    """(what receiver m's target holds, where, overflow): a guard-filled
    target with sender i's block at the prefix sum of the blocks before it."""
    P = len(counts)
    want = np.empty(capacity, DTYPE[bits])
    want.view(np.uint8)[:] = GUARD
    n = [counts[i][m] for i in range(P)]
    frm = [offsets[i][m] for i in range(P)]
    bad = any(n[i] > src_capacity or frm[i] > src_capacity - n[i] for i in range(P)) or sum(n) > capacity
    if bad:
        return want, [ONES] * (P + 1), True
    where, at = [], 0
    for i in range(P):
        where.append(at)
        want[at:at + n[i]] = source_of(bits, i, src_capacity, seed)[frm[i]:frm[i] + n[i]]
        at += n[i]
    return want, where + [at], False


def check_target(tag, bits, tgt, capacity, want, regions, before):
    got = np.empty(capacity, DTYPE[bits])
    shm.memcpy(got, tgt, got.nbytes)
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got != want)
        fails.append(f"{tag}: {len(bad)} elements differ from the model, first at {bad[:4].tolist()}")
    # everything outside the target as before the call: the guard bytes and the source
    for (p, nbytes), b, a in zip(regions, before, image(regions)):
        keep = np.ones(nbytes, bool)
        if p == ARENA_T:
            keep[tgt - p:tgt - p + got.nbytes] = False
        if not np.array_equal(a[keep], b[keep]):
            where_bad = np.flatnonzero((a != b) & keep)
            fails.append(f"{tag}: {len(where_bad)} bytes outside the target changed, first at region offset "
                         f"{where_bad[:4].tolist()}")


def prepare(bits, st, src_capacity, capacity, off, seed):
    """Guard-fill both arenas, write my source; returns (src, tgt, regions, before)."""
    esz = bits // 8
    m = members(st).index(pe)
    src, tgt = ARENA_S + PAD + off, ARENA_T + PAD + off
    regions = [(ARENA_S, src_capacity * esz + 2 * PAD + off), (ARENA_T, capacity * esz + 2 * PAD + off)]
    assert max(r[1] for r in regions) <= CAP
    for p, nbytes in regions:
        shm.memcpy(p, np.full(nbytes, GUARD, np.uint8), nbytes)
    mine = source_of(bits, m, src_capacity, seed)
    shm.memcpy(src, mine, mine.nbytes)
    return src, tgt, regions, image(regions)


def alltoallv_case(bits, counts, offsets, capacity, src_capacity, st, off, seed, where_in_heap=True):
    """counts / offsets: P x P over the set's members, row i what member i sends."""
    global ncases
    if pe not in members(st):
        return None
    P, m, esz = st[2], members(st).index(pe), bits // 8
    ncases += 1
    tag = f"alltoallv{bits} set={st} m={m} capacity={capacity} src_capacity={src_capacity} off={off} seed={seed:#x}"
    print(tag, flush=True)
    want, want_where, overflow = model(bits, counts, offsets, capacity, src_capacity, m, seed)
    src, tgt, regions, before = prepare(bits, st, src_capacity, capacity, off, seed)
    shm.memcpy(COUNTS, np.array(counts[m], np.uint64), P * 8)
    shm.memcpy(OFFSETS, np.array(offsets[m], np.uint64), P * 8)
    where = WHERE if where_in_heap else where_private
    stale = np.full(P + 1, 0x77, np.uint64)
    if where_in_heap:
        shm.memcpy(WHERE, stale, stale.nbytes)
    else:
        where_private.fill_(0x77)
    torch.cuda.synchronize()
    expect["alltoallvs"] += 1
    expect["fused_calls"] += capacity * esz <= fused_bytes
    expect["overflows"] += overflow
    try:
        shm.alltoallv_on_stream(bits, tgt, src, COUNTS, OFFSETS, where, capacity, src_capacity, *st)
    except shm.ShmemError as e:
        fails.append(f"{tag}: error {e.code}")
        return None
    torch.cuda.synchronize()
    if shm.last_error():
        fails.append(f"{tag}: last_error {shm.last_error()}")
    check_target(tag, bits, tgt, capacity, want, regions, before)
    if where_in_heap:
        got_where = np.empty(P + 1, np.uint64)
        shm.memcpy(got_where, WHERE, got_where.nbytes)
        got_where = [int(v) for v in got_where]
    else:
        got_where = [int(v) & ONES for v in where_private[:P + 1].cpu().tolist()]
    if got_where != want_where:
        fails.append(f"{tag}: where {got_where}, model {want_where}")
    return overflow


def alltoall_case(bits, nelems, st, off, seed):
    global ncases
    if pe not in members(st):
        return
    P, m, esz = st[2], members(st).index(pe), bits // 8
    ncases += 1
    tag = f"alltoall{bits} nelems={nelems} set={st} m={m} off={off} seed={seed:#x}"
    print(tag, flush=True)
    n = P * nelems
    counts = [[nelems] * P for _ in range(P)]
    offsets = [[j * nelems for j in range(P)] for _ in range(P)]
    want, _, overflow = model(bits, counts, offsets, n, n, m, seed)
    assert not overflow
    src, tgt, regions, before = prepare(bits, st, n, n, off, seed)
    torch.cuda.synchronize()
    expect["alltoalls"] += 1
    expect["fused_calls"] += n * esz <= fused_bytes
    try:
        shm.alltoall_on_stream(bits, tgt, src, nelems, *st)
    except shm.ShmemError as e:
        fails.append(f"{tag}: error {e.code}")
        return
    torch.cuda.synchronize()
    if shm.last_error():
        fails.append(f"{tag}: last_error {shm.last_error()}")
    check_target(tag, bits, tgt, n, want, regions, before)


def sets():
    s = [(0, 0, npes)]
    if npes >= 8:
        s += [(0, 1, 4), (2, 0, 3)]      # strided: PEs 0, 2, 4, 6; an offset run: PEs 2, 3, 4
    return s


def count_patterns(P):
    """P x P count matrices: odd counts; the same with zeros (a diagonal of
    own blocks among them); one 70001-element block; nothing at all."""
    odd = [[(1, 3, 5, 7, 1013)[(i + 2 * j) % 5] for j in range(P)] for i in range(P)]
    zeros = [[0 if (i + j) % 3 == 0 else 3 + i + 2 * j for j in range(P)] for i in range(P)]
    big = [list(r) for r in zeros]
    big[P - 1][0] = 70001
    return [odd, zeros, big, [[0] * P for _ in range(P)]]


def set_limit(kb):
    """Collective in effect: every PE of the job calls it at the same point."""
    global fused_bytes
    shm.set_fused_twoshot_kb(kb)
    fused_bytes = kb << 10


def blocking_sum_is_healthy(seed):
    """shmem_longlong_sum_to_all on the whole job after the scenario's last
    call: a device-barrier error would abort it."""
    global ncases
    n, st = 1013, (0, 0, npes)
    vals = [source_of(64, p, n, seed).astype(np.int64) for p in range(npes)]
    shm.memcpy(ARENA_S + PAD, vals[pe], n * 8)
    shm.barrier_all()
    shm.to_all("longlong", "sum", ARENA_T + PAD, ARENA_S + PAD, n, *st)
    got = np.empty(n, np.int64)
    shm.memcpy(got, ARENA_T + PAD, n * 8)
    ncases += 1
    with np.errstate(over="ignore"):
        want = np.sum(np.stack(vals), axis=0, dtype=np.int64)
    if shm.last_error() or got.tobytes() != want.tobytes():
        fails.append(f"the blocking longlong sum after the scenario: last_error {shm.last_error()}")
    shm.barrier_all()


def isx_model(P, keys_per_pe, seed):
    """ISx's key exchange: every PE draws keys_per_pe uniform 32-bit keys
    below 2^27 and buckets them by key range; the ranges are uneven (one is
    2048 keys wide), as after a sample sort's splitters.  Returns (bounds,
    per-PE sources grouped by destination, counts, offsets)."""
    top = 1 << 27
    weights = [j + 1 for j in range(P)]
    narrow = P // 2
    weights[narrow] = 0
    scale = (top - 2048) // sum(weights)
    bounds = [0]
    for j in range(P):
        bounds.append(bounds[-1] + (2048 if j == narrow else weights[j] * scale))
    bounds[-1] = top
    srcs, counts, offsets = [], [], []
    for i in range(P):
        keys = np.random.default_rng([seed, i]).integers(0, top, keys_per_pe, dtype=np.uint32)
        dest = np.searchsorted(np.array(bounds[1:], np.int64), keys.astype(np.int64), side="right")
        order = np.argsort(dest, kind="stable")
        srcs.append(keys[order])
        c = np.bincount(dest, minlength=P).tolist()
        counts.append(c)
        offsets.append([sum(c[:j]) for j in range(P)])
    return bounds, srcs, counts, offsets


seed = 0xA2A
# chosen so that, at 8 PEs, the model alone shows an empty block and pairwise different totals
ISX_SEED = 0x15C
torch.cuda.synchronize()
shm.barrier_all()

for scenario in scenarios:
    if scenario == "route":
        # both routes on whole and strided sets: the default limit (fused),
        # then 1 KiB with capacities above it (barrier, plan, copy, barrier)
        for limit_kb in (DEFAULT_KB, 1):
            set_limit(limit_kb)
            k = 0
            for st in sets():
                P = st[2]
                for bits in (32, 64):
                    for counts in count_patterns(P):
                        k += 1
                        seed += 1
                        offsets, need = rows_of(counts)
                        most = max(sum(counts[i][j] for i in range(P)) for j in range(P))
                        # the fullest target is filled exactly, or has room left
                        capacity = max(most + (0 if k % 3 else 5), 1024 // (bits // 8) + 1)
                        alltoallv_case(bits, counts, offsets, capacity, need + k % 2, st, 8 * (k % 2), seed,
                                       where_in_heap=k % 4 < 2)
                    for nelems in (3, 1013):
                        seed += 1
                        alltoall_case(bits, nelems, st, 8 * (nelems % 2), seed)
        set_limit(DEFAULT_KB)
        # a one-member set (every PE its own): no heap needed, no handshake
        seed += 1
        alltoallv_case(64, [[1013]], [[7]], 1013 + 3, 1013 + 7, (pe, 0, 1), 8, seed)
        t_src = torch.arange(100, dtype=torch.int64, device="cuda") + pe
        t_tgt = torch.full((128,), -1, dtype=torch.int64, device="cuda")
        t_tab = torch.tensor([60, 40], dtype=torch.int64, device="cuda")          # count, offset
        torch.cuda.synchronize()
        shm.alltoallv_on_stream(64, t_tgt, t_src, t_tab[0:], t_tab[1:], None, 128, 100, pe, 0, 1)
        torch.cuda.synchronize()
        expect["alltoallvs"] += 1
        expect["fused_calls"] += 1
        ncases += 1
        if not (torch.equal(t_tgt[:60], t_src[40:]) and bool((t_tgt[60:] == -1).all())) or shm.last_error():
            fails.append(f"one-member alltoallv outside the heap: last_error {shm.last_error()}")
    elif scenario == "isx":
        # one ISx iteration's exchange: count (on the host here), exchange,
        # and the sum of the bucket sizes the SIGNAL longlong sum gives
        KEYS = 4096
        st, P = (0, 0, npes), npes
        bounds, srcs, counts, offsets = isx_model(P, KEYS, ISX_SEED)
        totals = [sum(counts[i][j] for i in range(P)) for j in range(P)]
        if P == 8:      # on the model alone, before any GPU call
            assert any(counts[i][j] == 0 for i in range(P) for j in range(P)), "no empty block"
            assert len(set(totals)) == P, f"totals {totals} are not pairwise different"
        capacity = 2 * KEYS * 2
        assert max(totals) <= capacity and sum(totals) == P * KEYS
        S, T = ARENA_S + PAD, ARENA_T + PAD
        shm.memcpy(S, srcs[pe], KEYS * 4)
        shm.memcpy(T, np.full(capacity * 4, GUARD, np.uint8), capacity * 4)
        shm.memcpy(COUNTS, np.array(counts[pe], np.uint64), P * 8)
        shm.memcpy(OFFSETS, np.array(offsets[pe], np.uint64), P * 8)
        shm.memcpy(SUM_OUT, np.zeros(1, np.int64), 8)
        torch.cuda.synchronize()
        shm.alltoallv_on_stream(32, T, S, COUNTS, OFFSETS, WHERE, capacity, KEYS, *st)
        shm.reduce_on_stream("longlong", "sum", SUM_OUT, WHERE + P * 8, 1, *st, "signal")
        torch.cuda.synchronize()
        expect["alltoallvs"] += 1
        expect["fused_calls"] += 1
        ncases += 1
        got_where = np.empty(P + 1, np.uint64)
        shm.memcpy(got_where, WHERE, got_where.nbytes)
        want_where = [sum(counts[i][pe] for i in range(k)) for k in range(P)] + [totals[pe]]
        if [int(v) for v in got_where] != want_where:
            fails.append(f"isx: where {got_where.tolist()}, model {want_where}")
        got = np.empty(capacity, np.uint32)
        shm.memcpy(got, T, got.nbytes)
        want = np.concatenate([srcs[i][offsets[i][pe]:offsets[i][pe] + counts[i][pe]] for i in range(P)])
        bucket = got[:totals[pe]]
        if not np.array_equal(np.sort(bucket), np.sort(want)):
            fails.append("isx: my bucket is not the multiset the model gives")
        if bucket.size and not (int(bucket.min()) >= bounds[pe] and int(bucket.max()) < bounds[pe + 1]):
            fails.append(f"isx: keys outside my range [{bounds[pe]}, {bounds[pe + 1]})")
        if not np.all(got[totals[pe]:].view(np.uint8) == GUARD):
            fails.append("isx: the target past my bucket changed")
        total_keys = np.empty(1, np.int64)
        shm.memcpy(total_keys, SUM_OUT, 8)
        if int(total_keys[0]) != P * KEYS or shm.last_error():
            fails.append(f"isx: the sum of the bucket sizes is {int(total_keys[0])}, not {P * KEYS}; last_error "
                         f"{shm.last_error()}")
    elif scenario == "graph":
        # after a warm call: {copy of new tables from pinned host memory into
        # the heap, alltoallv64, the SIGNAL longlong sum of where[P], barrier}
        # captured on one stream and replayed with other tables and sources
        hip = ctypes.CDLL("libamdhip64.so.7")
        hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
                                       ctypes.c_void_p]
        hip.hipMemcpyAsync.restype = ctypes.c_int
        stream = torch.cuda.Stream()
        sid = stream.cuda_stream
        st, P, maxn = (0, 0, npes), npes, 1500
        src_capacity = P * (maxn + 2) + 8
        capacity = P * maxn
        S, T = ARENA_S + PAD, ARENA_T + PAD
        host_tab = torch.zeros(2 * 64, dtype=torch.int64).pin_memory()      # counts at 0, offsets at 64 words

        def step():
            rc = hip.hipMemcpyAsync(COUNTS, host_tab.data_ptr(), P * 8, 1, sid)
            assert rc == 0, rc
            rc = hip.hipMemcpyAsync(OFFSETS, host_tab.data_ptr() + 512, P * 8, 1, sid)
            assert rc == 0, rc
            shm.alltoallv_on_stream(64, T, S, COUNTS, OFFSETS, WHERE, capacity, src_capacity, *st, sid)
            shm.reduce_on_stream("longlong", "sum", SUM_OUT, WHERE + P * 8, 1, *st, "signal", sid)
            shm.barrier_on_stream(*st, sid)

        shm.memcpy(S, np.zeros(src_capacity, np.uint64), src_capacity * 8)
        shm.memcpy(T, np.zeros(capacity, np.uint64), capacity * 8)
        host_tab[:] = 0
        host_tab[:P] = 1
        torch.cuda.synchronize()
        shm.barrier_all()
        step()                                                        # warm: maps the peers, makes the state
        torch.cuda.synchronize()
        shm.alltoall_stats(reset=True)
        for key in expect:
            expect[key] = 0
        graph = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(graph, stream=stream):
                step()
        except shm.ShmemError as e:
            fails.append(f"graph: the capture was refused, error {e.code}")
            graph = None
        expect.update(alltoallvs=1, fused_calls=1)                    # the call made while capturing
        for rep in range(3 if graph else 0):
            seed += 1
            counts = [[(1009 * (rep + 1) + 977 * i + 313 * j) % maxn if (rep + i + j) % 4 else 0 for j in range(P)]
                      for i in range(P)]
            offsets, need = rows_of(counts)
            assert need <= src_capacity
            want, want_where, overflow = model(64, counts, offsets, capacity, src_capacity, pe, seed)
            assert not overflow
            shm.memcpy(S, source_of(64, pe, src_capacity, seed), src_capacity * 8)
            shm.memcpy(T, np.full(capacity * 8, GUARD, np.uint8), capacity * 8)
            shm.memcpy(WHERE, np.full(P + 1, 0x77, np.uint64), (P + 1) * 8)
            host_tab[:P] = torch.tensor(counts[pe], dtype=torch.int64)
            host_tab[64:64 + P] = torch.tensor(offsets[pe], dtype=torch.int64)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            ncases += 1
            got = np.empty(capacity, np.uint64)
            shm.memcpy(got, T, got.nbytes)
            if got.tobytes() != want.tobytes():
                bad = np.flatnonzero(got != want)
                fails.append(f"graph replay {rep}: {len(bad)} elements differ, first at {bad[:4].tolist()}")
            got_where = np.empty(P + 1, np.uint64)
            shm.memcpy(got_where, WHERE, got_where.nbytes)
            if [int(v) for v in got_where] != want_where:
                fails.append(f"graph replay {rep}: where {got_where.tolist()}, model {want_where}")
            total = np.empty(1, np.int64)
            shm.memcpy(total, SUM_OUT, 8)
            everything = sum(counts[i][j] for i in range(P) for j in range(P))
            if int(total[0]) != everything:
                fails.append(f"graph replay {rep}: the sum of the totals is {int(total[0])}, model {everything}")
            if shm.last_error():
                fails.append(f"graph replay {rep}: last_error {shm.last_error()}")
        del graph
    elif scenario == "overflow":
        # one member's total is over the capacity: that member keeps its
        # target and reads all ones, every other member's result is exact;
        # then a peer's pair points one element past its source, for one
        # receiver only; the healthy calls in between and the blocking
        # reduction after them succeed
        st, P = (0, 0, npes), npes
        for bits in (32, 64):
            base = [[100 + 10 * i + j for j in range(P)] for i in range(P)]
            offsets, need = rows_of(base)
            capacity = max(sum(base[i][j] for i in range(P)) for j in range(P))
            over = [list(r) for r in base]
            over[0][1] += capacity                     # receiver 1 overflows by its total, the others do not
            offsets_over, need_over = rows_of(over)
            past = [list(r) for r in offsets]
            past[P - 1][0] = need - base[P - 1][0] + 1         # receiver 0: one element past member P - 1's source
            for counts, offs, room, bad_at in ((over, offsets_over, need_over, 1), (base, offsets, need, None),
                                               (base, past, need, 0), (base, offsets, need, None)):
                for limit_kb in (DEFAULT_KB, 1):
                    set_limit(limit_kb)
                    seed += 1
                    overflow = alltoallv_case(bits, counts, offs, capacity, room, st, 0, seed)
                    if overflow != (pe == bad_at):
                        fails.append(f"overflow: PE {pe} saw overflow={overflow}, the bad receiver is {bad_at}")
        set_limit(DEFAULT_KB)
        blocking_sum_is_healthy(seed + 100)
    elif scenario == "mirrored":
        # $SHMEMX_HEAP_MEMORY=mirrored (the library's default): shmem_malloc
        # returns host-view addresses.  Host code writes the sources, the
        # tables and the guard bytes with plain stores, the call runs on the
        # HBM twins, and host code reads the target and where back (the load
        # waits for the call's stream).
        assert os.environ.get("SHMEMX_HEAP_MEMORY") == "mirrored"

        def host_view(ptr, dtype, n):
            buf = (ctypes.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr)
            return np.frombuffer(buf, dtype=dtype, count=n)

        st, P, maxn = (0, 0, npes), npes, 9001
        src_capacity, capacity = P * (maxn + 2) + 8, P * maxn
        sv = host_view(ARENA_S + PAD, np.uint64, src_capacity)
        tv = host_view(ARENA_T + PAD, np.uint64, capacity)
        cv, ov, wv = (host_view(a, np.uint64, P + 1) for a in (COUNTS, OFFSETS, WHERE))
        for rnd in range(4):
            seed += 1
            if rnd == 3:
                nelems = maxn
                counts = [[nelems] * P for _ in range(P)]
                offsets = [[j * nelems for j in range(P)] for _ in range(P)]
                room = cap = P * nelems
            else:
                counts = [[maxn - 1000 * ((i + j + rnd) % P) - rnd for j in range(P)] for i in range(P)]
                offsets, need = rows_of(counts)
                room, cap = src_capacity, capacity
                assert need <= room
            want, want_where, overflow = model(64, counts, offsets, cap, room, pe, seed)
            assert not overflow
            sv[:room] = source_of(64, pe, room, seed)
            tv.view(np.uint8)[:] = GUARD
            cv[:P], ov[:P], wv[:] = counts[pe], offsets[pe], 0x77
            if rnd == 3:
                shm.alltoall_on_stream(64, ARENA_T + PAD, ARENA_S + PAD, nelems, *st)
                expect["alltoalls"] += 1
            else:
                shm.alltoallv_on_stream(64, ARENA_T + PAD, ARENA_S + PAD, COUNTS, OFFSETS, WHERE, cap, room, *st)
                expect["alltoallvs"] += 1
            expect["fused_calls"] += 1
            got = tv[:cap].copy()
            ncases += 1
            if shm.last_error() or got.tobytes() != want.tobytes():
                bad = np.flatnonzero(got != want)
                fails.append(f"mirrored round {rnd}: last_error {shm.last_error()}, {len(bad)} elements differ, "
                             f"first at {bad[:4].tolist()}")
            if rnd != 3 and [int(v) for v in wv.copy()] != want_where:
                fails.append(f"mirrored round {rnd}: where {wv.tolist()}, model {want_where}")
            if sv[:room].tobytes() != source_of(64, pe, room, seed).tobytes():
                fails.append(f"mirrored round {rnd}: the source changed")
            shm.barrier_on_stream(*st)
            torch.cuda.synchronize()
    elif scenario == "refusal":
        # every member passes an operand outside the heap: ENOTSUP on every
        # member and nothing launched: the counters do not move
        st, n = (0, 0, npes), 1013
        private = torch.zeros(npes * n, dtype=torch.int64, device="cuda")
        ptab = torch.zeros(64, dtype=torch.int64, device="cuda")
        S, T = ARENA_S + PAD, ARENA_T + PAD
        torch.cuda.synchronize()
        stats0 = shm.alltoall_stats()
        attempts = (("source", lambda: shm.alltoallv_on_stream(64, T, private, COUNTS, OFFSETS, WHERE, n, n, *st)),
                    ("target", lambda: shm.alltoallv_on_stream(32, private, S, COUNTS, OFFSETS, None, n, n, *st)),
                    ("counts", lambda: shm.alltoallv_on_stream(64, T, S, ptab, OFFSETS, None, n, n, *st)),
                    ("offsets", lambda: shm.alltoallv_on_stream(64, T, S, COUNTS, ptab, None, n, n, *st)),
                    ("alltoall source", lambda: shm.alltoall_on_stream(64, T, private, n, *st)),
                    ("alltoall target", lambda: shm.alltoall_on_stream(32, private, S, n, *st)))
        for what, attempt in attempts:
            ncases += 1
            try:
                attempt()
                fails.append(f"{what} outside the heap: the call was accepted")
            except shm.ShmemError as e:
                if e.code != ENOTSUP or shm.last_error() != ENOTSUP:
                    fails.append(f"{what} outside the heap: error {e.code}, last_error {shm.last_error()}")
        torch.cuda.synchronize()
        if shm.alltoall_stats() != stats0:
            fails.append(f"refusal: the counters moved from {stats0} to {shm.alltoall_stats()}")
        blocking_sum_is_healthy(seed + 200)
    else:
        raise SystemExit(f"unknown scenario {scenario}")

torch.cuda.synchronize()
stats = shm.alltoall_stats()
collect_keys, pull_keys = list(shm.collect_stats()), list(shm.pull_stats())
shm.barrier_all()
shm.finalize()
with open(out_path, "w") as f:
    json.dump({"pe": pe, "fails": fails, "ncases": ncases, "expect": {k: int(v) for k, v in expect.items()},
               "stats": {k: int(v) for k, v in stats.items()}, "collect_keys": collect_keys, "pull_keys": pull_keys},
              f)
print(f"PE {pe}: {ncases} cases, {len(fails)} failures", flush=True)
sys.exit(1 if fails else 0)
