"""One PE of test_gpu_ownslice.py: P of these processes share the one GPU and
run SHMEMX_ALGO_OWNSLICE for real across processes (the owner of a slice
folds it in every member's order, the members pull their results from the
owners' IPC scratch).

    SHMEM_PE=p SHMEM_NPES=P SHMEM_BOOTSTRAP_FILE=f python gpu_ownslice_child.py OUT.json SCENARIO

Every call is checked, on every member, against the oracle's answer for that
PE and against the bits of the same call under `gather`; the bytes around the
target (guard words, and the source where it is not the target) must be as
before the call.  Writes a JSON report to OUT.json.
"""
import faulthandler
import json
import os
import sys
import time

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
if os.environ.get("FAKE_RCCL"):
    import ctypes
    ctypes.CDLL(os.environ["FAKE_RCCL"], mode=ctypes.RTLD_GLOBAL)
torch.cuda.set_device(0)
shm.init()
assert shm.my_pe() == pe and shm.n_pes() == npes
# shmem_init refuses a job whose PEs were started with different limits, so a
# PE that is to disagree sets its own after it: the library reads
# $SHMEMX_DIRECT_ONESHOT_KB at the first reduction
if os.environ.get("OWNSLICE_LATE_ONESHOT_KB"):
    os.environ["SHMEMX_DIRECT_ONESHOT_KB"] = os.environ["OWNSLICE_LATE_ONESHOT_KB"]

PAIRS = [(t, o) for t in ("float", "double", "longdouble") for o in ("min", "max")]
MODES = ("heap", "inplace", "heap8", "device", "overlap_fwd", "overlap_rev")
GUARD, PAD = 0xAB, 64
CAP = 4 << 20
ARENA_A, ARENA_B = shm.malloc(CAP), shm.malloc(CAP)
assert ARENA_A and ARENA_B, "shmem_malloc failed"
fails, ncases, two_phase, differs, fused = [], 0, 0, 0, 0


def member(start, log, size):
    step = 1 << log
    return pe >= start and (pe - start) % step == 0 and (pe - start) // step < size


def place(mode, t, nb, sz):
    """(source address, target address, [(region address, bytes)], keep-alive)
    of one call's operands, each region PAD bytes wider than its array on
    both sides."""
    if mode == "device":     # outside the heap: the source is staged
        a = torch.empty(nb + 2 * PAD, dtype=torch.uint8, device="cuda")
        b = torch.empty(nb + 2 * PAD, dtype=torch.uint8, device="cuda")
        return (a.data_ptr() + PAD, b.data_ptr() + PAD,
                [(a.data_ptr(), nb + 2 * PAD), (b.data_ptr(), nb + 2 * PAD)], (a, b))
    shift = 3 * sz
    if mode == "heap":
        return ARENA_A + PAD, ARENA_B + PAD, [(ARENA_A, nb + 2 * PAD), (ARENA_B, nb + 2 * PAD)], None
    if mode == "heap8":      # off 16-byte alignment by 8 (long double: by one element)
        off = 16 if t == "longdouble" else 8
        return (ARENA_A + PAD + off, ARENA_B + PAD + off,
                [(ARENA_A, nb + 2 * PAD + off), (ARENA_B, nb + 2 * PAD + off)], None)
    if mode == "inplace":
        return ARENA_A + PAD, ARENA_A + PAD, [(ARENA_A, nb + 2 * PAD)], None
    if mode == "overlap_fwd":   # the target starts inside the source: chunks walk backwards
        return ARENA_A + PAD, ARENA_A + PAD + shift, [(ARENA_A, nb + shift + 2 * PAD)], None
    return ARENA_A + PAD + shift, ARENA_A + PAD, [(ARENA_A, nb + shift + 2 * PAD)], None   # overlap_rev


def image(regions):
    out = []
    for p, nbytes in regions:
        a = np.empty(nbytes, np.uint8)
        shm.memcpy(a, p, nbytes)
        out.append(a)
    return out


def call(t, op, n, st, algo, mode, mine):
    """One collective call from freshly filled regions: (the target's elements,
    the regions before, the regions after, src, tgt, regions, error code)."""
    sz = mine.itemsize
    nb = n * sz
    src, tgt, regions, keep = place(mode, t, nb, sz)
    for p, nbytes in regions:
        shm.memcpy(p, np.full(nbytes, GUARD, np.uint8), nbytes)
    shm.memcpy(src, mine, nb)
    before = image(regions)
    global fused
    err = 0
    fused0 = shm.direct_stats(reset=False)["fused_calls"]
    try:
        shm.reduce_on_stream(t, op, tgt, src, n, *st, algo)
    except shm.ShmemError as e:
        err = e.code
    torch.cuda.synchronize()
    if algo == "ownslice":
        fused += shm.direct_stats(reset=False)["fused_calls"] - fused0
    after = image(regions)
    got = np.empty(n, mine.dtype)
    shm.memcpy(got, tgt, nb)
    del keep
    return got, before, after, src, tgt, regions, err


def run_case(t, op, n, st, mode, seed, expect_two_phase):
    global ncases, two_phase, differs
    srcs = oracle.special_sources(t, npes, n, seed)
    if not member(*st):
        return
    ncases += 1
    tag = f"{t} {op} n={n} set={st} mode={mode}"
    print(tag, flush=True)
    mine = np.ascontiguousarray(srcs[pe])
    want = oracle.reduce_one(t, op, srcs, *st, pe)
    if st[2] > 1 and st[0] == 0 and st[1] == 0:
        first = oracle.reduce_one(t, op, srcs, *st, st[0])
        differs += 0 if same_bits(want, first) else int(
            (want.view(np.uint8).reshape(n, -1)[:, :10] != first.view(np.uint8).reshape(n, -1)[:, :10]).any(axis=1).sum())
    ref = call(t, op, n, st, "gather", mode, mine)[0]
    got, before, after, src, tgt, regions, err = call(t, op, n, st, "ownslice", mode, mine)
    if st[2] > 1 and expect_two_phase:
        two_phase += 1
    if err or shm.last_error():
        fails.append(f"{tag}: error {err} / last_error {shm.last_error()}")
        return
    if not same_bits(got, want):
        w = 10 if t == "longdouble" else mine.itemsize
        bad = np.flatnonzero((got.view(np.uint8).reshape(n, -1)[:, :w] !=
                              want.view(np.uint8).reshape(n, -1)[:, :w]).any(axis=1))
        fails.append(f"{tag}: {len(bad)} elements differ from the oracle, first at {bad[:4].tolist()}")
    if not same_bits(got, ref):
        fails.append(f"{tag}: differs from the same call under gather")
    # everything outside the target as before the call: the guard bytes
    # around it, and the source where the target does not cover it
    nb = n * mine.itemsize
    for (p, nbytes), b, a in zip(regions, before, after):
        keep = np.ones(nbytes, bool)
        if p <= tgt < p + nbytes:
            keep[tgt - p:tgt - p + nb] = False
        if not np.array_equal(a[keep], b[keep]):
            where = np.flatnonzero((a != b) & keep)
            fails.append(f"{tag}: {len(where)} bytes outside the target changed, first at region offset "
                         f"{where[:4].tolist()} (target at {tgt - p})")


def sets():
    s = [(0, 0, npes)]
    if npes >= 8:
        s += [(0, 1, 4), (2, 0, 4)]      # strided: PEs 0, 2, 4, 6; an offset run: PEs 2..5
    return s


def rotate(seq, k, count):
    return [seq[(k + i) % len(seq)] for i in range(count)]


seed = 0x0515
if scenario == "forced":
    # $SHMEMX_DIRECT_ONESHOT_KB=0: every size takes the two-phase schedule.
    # 1 and 3 elements leave members without a slice at 8 PEs.  The whole job
    # sees every operand placement with every pair and size; the partial
    # sets of the 8-PE run two placements per (pair, size), in rotation.
    assert os.environ.get("SHMEMX_DIRECT_ONESHOT_KB") == "0"
    k = 0
    for st in sets():
        for t, op in PAIRS:
            for n in (1, 3, 1013, 70001):
                for mode in (MODES if st[2] == npes else rotate(MODES, k, 2)):
                    seed += 1
                    run_case(t, op, n, st, mode, seed, True)
                k += 1
    # the blocking entry points with the algorithm set job-wide, on pageable
    # host arrays (staged): the six pairs run the two phases, any other pair
    # runs as DIRECT
    shm.set_algo("ownslice")
    for t, op in PAIRS + [("long", "xor"), ("double", "sum")]:
        seed += 1
        n = 1013
        own = (t, op) in PAIRS
        srcs = oracle.special_sources(t, npes, n, seed) if own else oracle.sources(t, 1, npes, n, base_seed=seed)
        mine = np.ascontiguousarray(srcs[pe])
        tgt = np.zeros_like(mine)
        tag = f"blocking {t} {op} n={n}"
        print(tag, flush=True)
        shm.to_all(t, op, tgt, mine.copy(), n, 0, 0, npes)
        ncases += 1
        two_phase += own
        if shm.last_error() or not same_bits(tgt, oracle.reduce_one(t, op, srcs, 0, 0, npes, pe if own else 0)):
            fails.append(f"{tag}: last_error {shm.last_error()} or differs from the oracle")
    shm.set_algo("auto")
elif scenario == "chunks":
    # $SHMEMX_DIRECT_SCRATCH_MB=1: half a MiB of staging, so 300 007 floats and
    # 150 001 doubles (1.2 MB) take three chunks whenever a member stages or
    # the array is larger than a chunk; the overlapping case walks backwards
    assert os.environ.get("SHMEMX_DIRECT_SCRATCH_MB") == "1"
    for t, op in PAIRS[:4]:
        n = 300007 if t == "float" else 150001
        for mode in ("heap", "device", "overlap_fwd"):
            seed += 1
            run_case(t, op, n, (0, 0, npes), mode, seed, True)
elif scenario == "default":
    # the default one-shot limit: 1013 elements take the fused own-order one
    # shot, not the two phases
    for t, op in PAIRS:
        seed += 1
        run_case(t, op, 1013, (0, 0, npes), "heap", seed, False)
elif scenario == "mismatch":
    # members whose $SHMEMX_DIRECT_ONESHOT_KB differ (PE 1's set after
    # shmem_init, which would refuse the job otherwise): ENOTSUP on every member,
    # at once, target untouched; at 8 KB the limits even pick different
    # schedules (one shot on PE 1, two phases elsewhere)
    for n in (70001, 1013):
        srcs = oracle.special_sources("double", npes, n, seed + n)
        t0 = time.time()
        got, before, after, src, tgt, regions, err = call("double", "max", n, (0, 0, npes), "ownslice", "heap",
                                                          np.ascontiguousarray(srcs[pe]))
        ncases += 1
        if err != 3 or time.time() - t0 > 30 or any(not np.array_equal(a, b) for a, b in zip(after, before)):
            fails.append(f"mismatch n={n}: error {err} after {time.time() - t0:.1f} s, want ENOTSUP, target untouched")
else:
    raise SystemExit(f"unknown scenario {scenario}")

stats = shm.direct_stats(reset=False)
shm.barrier_all()
shm.finalize()
with open(out_path, "w") as f:
    json.dump({"pe": pe, "fails": fails, "ncases": ncases, "two_phase_expected": two_phase,
               "ownslice_calls": stats["ownslice_calls"], "fused_calls": fused,
               "differs": differs}, f)
print(f"PE {pe}: {ncases} cases, {len(fails)} failures", flush=True)
sys.exit(1 if fails else 0)
