#!/usr/bin/env python3
"""Benchmark: GiB/s of device-resident shmem_double_sum_to_all, nreduce = 32 Mi.

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...

A plain run does what the headline needs and nothing else: it sets up the
operands, runs W warm-up steps, times K steps, writes the timed path's outputs
if --dump-outputs is given, and prints the one JSON line (`correct`,
`cpu_baseline` and `guard` are null, `extras` empty).  --full adds everything
else the line can carry, after the timed steps: the correctness guard on what
was timed, the kernel-clock cross-check and the measured ceiling of the
roofline, the CPU baseline and its table, and the extras (other algorithms,
sizes, precisions and API forms).

A "step" is one pass of the hot path over one batch of synthetic input
(BASELINE.json metric; DESIGN.md "Measurement"):

* N = 1 (BASELINE.json configs[1], "1 PE = 1 MI355X, local reduce only"): the
  local element-wise reduction of the reference, write_to[i] =
  op(write_to[i], pWrk[i]) (reduce-op.c:231-235), as the HIP fold kernel over
  the whole 32 Mi-element array, called through the C ABI
  (shmemx_fold_on_stream).  value = nreduce*8 B / step time.
* N > 1 (configs[2]): the full collective shmemx_double_sum_to_all on all N
  PEs (one per GPU, RCCL over xGMI), stream-ordered.  value = algbw =
  nreduce*8 B / step time, SURVEY.md §8(d) config 3's definition (every PE
  reduces its own 32 Mi array into one 32 Mi result; weak scaling: the array
  per PE stays 32 Mi as N grows); aggregate_GiBps = N x that (input bytes of
  the whole job per second) and roofline.busbw_GBps = algbw x 2(N-1)/N.

Timing: W untimed warm-up steps, then K steps bracketed by a barrier and a
device synchronize on both sides; the max over ranks is reported.  The
kernel's average launch duration comes from HIP events recorded on the stream
the kernel runs on.  The CPU baseline (--full; rank 0) times the oracle
restatement of the reference's src/reduce on the host cores.

--dump-outputs DIR: right after the timed steps, rank 0 writes what the timed
path left in its output array (N = 1: the fold's accumulator, `acc`; N > 1:
the collective's target, `target`) as DIR/<name>.npy in float64.  An array
over 64 MB is written as a fixed sample (DUMP_SAMPLE elements at seeded
indices, the same in every run).  The operands come from seeded generators,
so the same arguments give the same inputs, and two builds can be compared
output for output.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import threading
import time

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "openshmem-async_amd"))
# The bench's operands are shmem_malloc'd blocks handed to the fold kernel and
# RCCL directly: the HBM heap's device addresses (the library's default is the
# mirrored heap, whose host view is for reference-style host code).
os.environ.setdefault("SHMEMX_HEAP_MEMORY", "device")
import shmem_mi355x as shm  # noqa: E402

GiB = float(1 << 30)
HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec (MI355X_MICROARCH.md)
XGMI_LINK_GBS = 153.0          # per link per direction, 7 links per GPU
XGMI_PEAK_BASIS = (
    "peak = (N-1) x 153 GB/s: each GPU's N-1 direct xGMI links (one per peer, full mesh of 8) at "
    "153 GB/s per link in EACH direction, the figure of the task statement ('7 links x ~153 GB/s "
    "per GPU') and SURVEY.md section 8(d) config 3; achieved = the bytes each GPU sends (= the bytes "
    "it receives) in reduce-scatter + all-gather, 2(N-1)/N x 256 MiB, over the time per call. "
    "measured_link_ceiling_GBps (extras.xgmi_links.pull_all, same run) is the links' measured rate")


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--nreduce", type=int, default=32 * 1024 * 1024)
    ap.add_argument("--algo", default="auto", choices=list(shm.ALGOS))
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the timed path's output array after the last timed step as "
                         "DIR/<name>.npy (float64; a fixed seeded sample if it is over 64 MB)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run the correctness guard, the roofline's "
                         "cross-checks, the CPU baseline and the extras (the options below)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-reps", type=int, default=20,
                    help="warm calls the N = 1 CPU baseline times (the median is reported)")
    ap.add_argument("--cpu-reps-multi", type=int, default=7,
                    help="warm calls the N > 1 CPU baseline (N PE processes) times")
    ap.add_argument("--cpu-table", type=int, default=1,
                    help="also time every BASELINE.json config on the host (cpu_baseline.table)")
    ap.add_argument("--extras", type=int, default=1, help="also time the other algorithms / API forms")
    ap.add_argument("--extras-timeout", type=float, default=300.0,
                    help="seconds the extras may take before the line is printed without the rest")
    ap.add_argument("--extras-only", default="",
                    help="comma-separated names of the extras to run (default: all)")
    ap.add_argument("--corrupt-guard-test", action="store_true",
                    help="tests only: corrupt one element of rank 0's target before the N > 1 "
                         "correctness guard, which must then report correct false")
    ap.add_argument("--extras-max-nreduce", type=int, default=256 * 1024 * 1024,
                    help="cap on the extras' array sizes (elements; the tests' short N > 1 runs "
                         "lower it; the driver's runs keep the full BASELINE.json sizes)")
    return ap.parse_args()


def pmc_traffic(kernel_key: str, pdir: str | None = None, code_sha: str | None = None):
    """(HBM bytes per launch, note) from the newest committed rocprofv3 PMC
    summary (profiles/r*_pmc.json, written by tools/summarize_prof.py), but
    only if it was measured on the device code this run loaded (its
    library.device_code_sha256 = the sha256 of the loaded library's
    .hip_fatbin): a kernel change without a fresh counter pass reports
    traffic None and says why."""
    pdir = pdir or os.path.join(REPO, "profiles")
    code_sha = code_sha or shm.device_code_sha256()
    if not os.path.isdir(pdir):
        return None, "no profiles/ directory"
    for name in sorted(os.listdir(pdir), reverse=True):
        if not (name.startswith("r") and name.endswith("_pmc.json")):
            continue
        try:
            with open(os.path.join(pdir, name)) as f:
                d = json.load(f)
        except (OSError, ValueError):
            continue
        v = d.get(kernel_key, {}).get("hbm_bytes_per_launch")
        if not v:
            continue
        measured = (d.get("library") or {}).get("device_code_sha256")
        if not measured or measured != code_sha:
            return None, (f"profiles/{name} was measured on other device code (sha256 {str(measured)[:16]}, "
                          f"loaded {str(code_sha)[:16]}): rerun the pmc step (tools/gpu_steps.sh pmc)")
        return float(v), f"profiles/{name}: FETCH_SIZE / WRITE_SIZE passes on this device code"
    return None, "no PMC summary with this kernel under profiles/"


def cpu_model() -> str:
    try:
        with open("/proc/cpuinfo") as f:
            return next(ln.split(":", 1)[1].strip() for ln in f if ln.startswith("model name"))
    except (OSError, StopIteration):
        return "unknown CPU"


def pin_base(P: int) -> int:
    """First of the LAST P consecutive CPUs this process may run on (the box
    gives a job a CPU share, not the whole host), or -1 to leave the PEs
    unpinned.  The last ones, not the first: CPU 0 of a share also serves
    interrupts and, usually, the runtimes' own threads."""
    allowed = sorted(os.sched_getaffinity(0))
    for i in range(len(allowed) - P, -1, -1):
        if allowed[i + P - 1] - allowed[i] == P - 1:
            return allowed[i]
    return -1


def spread_ms(times):
    """min / median / max of per-call seconds, in ms."""
    return {"min_ms": round(min(times) * 1e3, 3), "median_ms": round(statistics.median(times) * 1e3, 3),
            "max_ms": round(max(times) * 1e3, 3), "calls": len(times)}


def cpu_baseline(n: int, reps: int, world: int = 1):
    """The same workload as the GPU step, on the host cores, in the oracle
    restatement of the reference's src/reduce (reduce-op.c, gcc -O2: faster
    than the reference's own default build, -std=c99 with no -O,
    configure:524-539, so a conservative baseline).

    * world == 1: the local reduction write_to = op(write_to, pWrk) over n
      doubles (reduce-op.c:224-245, 64-element pWrk staging, an indirect call
      per element), one process pinned to one core; n*8/t like the GPU value.
    * world > 1: the whole shmem_double_sum_to_all of the line's config on
      `world` PEs = `world` forked processes over shared memory (the GASNet
      smp model, oshrun.in:97-98), pinned to `world` consecutive cores, the
      reference's peer loop (reduce-op.c:213-250); value = algbw n*8/t like
      the GPU value (aggregate_GiBps = world x that), t = PE 0's time per call.
    Median of `reps` warm calls, with min / max and the wall time."""
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import oracle  # cpu_baseline leg only
    base = pin_base(world)
    t0 = time.perf_counter()
    if world == 1:
        times = oracle.fold_time("double", "sum", n, reps=reps, pin=base)
        what = (f"the local reduce of shmem_double_sum_to_all, write_to = write_to + pWrk over nreduce={n} "
                f"(64-element pWrk staging, indirect call per element, :224-245), the N = 1 GPU step's "
                f"workload, one process")
    else:
        times, _ = oracle.reduce_fork("double", "sum", world, 0, 0, world, n, kind=0, reps=reps,
                                      pin_base=base)
        what = (f"the whole shmem_double_sum_to_all over nreduce={n} on {world} PEs (the line's config): "
                f"{world} forked PE processes over shared memory, the reference's copy + barrier + peer "
                f"loop (reduce-op.c:213-250), PE 0's time per call")
    wall = time.perf_counter() - t0
    med = statistics.median(times)
    cpus = (str(base) if world == 1 else f"{base}-{base + world - 1}") if base >= 0 else "unpinned"
    return {"value": round(n * 8 / med / GiB, 4), "unit": "GiB/s", "cores": world,
            "aggregate_GiBps": round(world * n * 8 / med / GiB, 4),
            "kind": "port",
            "sample": f"oracle restatement of reduce-op.c (gcc -O2, faster than the reference's default "
                      f"-std=c99 without -O): {what}, pinned to CPU {cpus} (the last of the job's "
                      f"{len(os.sched_getaffinity(0))} usable CPUs); median of {len(times)} warm calls "
                      f"({med * 1e3:.1f} ms/call, {wall:.1f} s wall); host: {cpu_model()}, "
                      f"{os.cpu_count()} logical CPUs",
            "cpus": cpus, "spread": spread_ms(times), "wall_s": round(wall, 2),
            # SURVEY §8(d) timing method: per-PE algbw, the host, the cores used
            "per_pe_GiBps": round(n * 8 / med / GiB, 4), "cpu_model": cpu_model(),
            "host_cpus": os.cpu_count(), "usable_cpus": len(os.sched_getaffinity(0))}


def cpu_baseline_table(reps: int = 3):
    """BASELINE.md's CPU-baseline plan, every BASELINE.json config on the
    host: the oracle restatement of reduce-op.c (gcc -O2) as P forked PE
    processes pinned to P consecutive CPUs over shared memory (the GASNet
    smp model, oshrun.in:97-98); one warm-up call, then the median of `reps`
    calls of PE 0; per-PE algbw = nreduce*sizeof(T)/t.  The float sweep is
    capped at 16 Mi elements and the median is of 3 calls (BASELINE.md says
    5), so the table costs about a minute of wall time: 256 Mi floats at 8 PEs
    alone would hold 8 GiB of host memory for ~30 s."""
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import oracle  # cpu_baseline leg only
    Mi = 1024 * 1024
    rows = [("int", "sum", 2, 1024, "configs[0]"), ("int", "sum", 2, 1, "configs[0] at n = 1"),
            ("int", "sum", 2, 4096, "configs[0] at n = 4096"), ("longlong", "sum", 1, 1, "ISx's call, 1 PE")]
    rows += [("double", "sum", P, 32 * Mi, "configs[1]" if P == 1 else "configs[2]") for P in (1, 2, 4, 8)]
    rows += [("long", op, 4, 64 * Mi, "configs[3]") for op in ("and", "or", "xor")]
    n = 4 * 1024
    while n <= 16 * Mi:
        rows.append(("float", "sum", 8, n, "configs[4]"))
        n *= 4
    size = {"int": 4, "double": 8, "long": 8, "float": 4, "longlong": 8}
    out = []
    t0 = time.perf_counter()
    base = pin_base(1)
    ft = oracle.fold_time("double", "sum", 32 * Mi, reps=reps, pin=base)
    fold = statistics.median(ft)
    out.append({"config": "configs[1]", "call": "local reduce of shmem_double_sum_to_all "
                "(write_to = write_to + pWrk, the N = 1 GPU step)", "nreduce": 32 * Mi, "PEs": 1,
                "cores": 1, "cpus": str(base), "ms_per_call": round(fold * 1e3, 4),
                "spread": spread_ms(ft), "per_pe_GiBps": round(32 * Mi * 8 / fold / GiB, 4)})
    for t, op, P, n, cfg in rows:
        base = pin_base(P)
        times, _ = oracle.reduce_fork(t, op, P, 0, 0, P, n, kind=0,
                                      reps=reps if n * size[t] >= 1 << 20 else 4 * reps, pin_base=base)
        med = statistics.median(times)
        out.append({"config": cfg, "call": f"shmem_{t}_{op}_to_all", "nreduce": n, "PEs": P,
                    "cores": P, "cpus": f"{base}-{base + P - 1}" if base >= 0 else "unpinned",
                    "ms_per_call": round(med * 1e3, 4), "spread": spread_ms(times),
                    "per_pe_GiBps": round(n * size[t] / med / GiB, 4)})
    return {"host": f"{cpu_model()}, {os.cpu_count()} logical CPUs, "
                    f"{len(os.sched_getaffinity(0))} usable by this job",
            "method": "oracle restatement of reduce-op.c (gcc -O2), fork-per-PE over shared memory, "
                      f"PE 0 per-call time, median of {reps} warm calls (x4 below 1 MiB)",
            "wall_s": round(time.perf_counter() - t0, 1), "rows": out}


def host_e2e(n: int):
    """The north-star end-to-end rate: source/target in HOST memory (the
    reference's symmetric heap), blocking shmem_double_sum_to_all at
    PE_size = 1 = H2D + device path + D2H.  Pageable (numpy), the same numpy
    arrays page-locked once with shmemx_host_register, and torch pinned."""
    import numpy as np
    res = {}
    psync = np.full(128, -1, dtype=np.int64)
    for kind in ("pageable", "registered", "pinned"):
        if kind in ("pageable", "registered"):
            src = np.random.default_rng(1).random(n) + 1.0
            tgt = np.zeros(n)
            if kind == "registered":   # shmemx_host_register, once, as on the heap segment
                shm.host_register(src, src.nbytes)
                shm.host_register(tgt, tgt.nbytes)
        else:
            src = torch.rand(n, dtype=torch.float64).pin_memory()
            tgt = torch.zeros(n, dtype=torch.float64).pin_memory()
        shm.to_all("double", "sum", tgt, src, n, 0, 0, 1, None, psync)   # warm-up
        ts = []
        for _ in range(7):
            t0 = time.perf_counter()
            shm.to_all("double", "sum", tgt, src, n, 0, 0, 1, None, psync)
            ts.append(time.perf_counter() - t0)
        t = statistics.median(ts)
        ok = bool((np.asarray(tgt) == np.asarray(src)).all())
        if kind == "registered":
            shm.host_unregister(src)
            shm.host_unregister(tgt)
        res[kind] = {"GiBps": round(n * 8 / t / GiB, 2), "ms_per_call": round(t * 1e3, 2),
                     "GiBps_min_max": [round(n * 8 / max(ts) / GiB, 2), round(n * 8 / min(ts) / GiB, 2)],
                     "correct": ok}
    return res


def host_e2e_multi(world: int, rank: int, n: int, barrier, max_over_ranks):
    """SURVEY §8(d) "host-resident e2e" for configs[2]: every PE's source and
    target in HOST memory (the reference's heap is host memory), the blocking
    shmem_double_sum_to_all over all N PEs = per PE H2D + the collective + D2H:
    page-locked arrays (the pinned pipeline) and, under
    "pageable", numpy arrays (the page-locked ring and its copy gangs, every
    PE's copies sharing the host's memory).  t = the slowest PE's call (median
    of 3 warm calls); GiBps = N * n * 8 B / t (every PE's input bytes, the
    extras' aggregate unit), algbw_GiBps = n * 8 B / t.  Sources are
    integer-valued doubles, PE r's = (r + 1) * base, so every rounding order
    gives the exact sum and the check is bit-exact: base * N (N + 1) / 2."""
    import numpy as np
    psync = np.full(128, -1, dtype=np.int64)
    base = torch.randint(0, 1 << 20, (n,), dtype=torch.int64,
                         generator=torch.Generator().manual_seed(7)).to(torch.float64)
    want = base * (world * (world + 1) // 2)

    def run(src, tgt, read):
        shm.to_all("double", "sum", tgt, src, n, 0, 0, world, None, psync)   # warm-up
        err = shm.last_error()
        ts = []
        for _ in range(3):
            barrier()
            t0 = time.perf_counter()
            shm.to_all("double", "sum", tgt, src, n, 0, 0, world, None, psync)
            ts.append(max_over_ranks(time.perf_counter() - t0))
            err = err or shm.last_error()
        t = statistics.median(ts)
        ok = err == 0 and bool(torch.equal(read(), want))
        ok = max_over_ranks(0.0 if ok else 1.0) == 0.0
        return {"GiBps": round(world * n * 8 / t / GiB, 2), "algbw_GiBps": round(n * 8 / t / GiB, 2),
                "ms_per_call": round(t * 1e3, 2), "correct": ok, "last_error": err}

    src = (base * (rank + 1)).pin_memory()
    tgt = torch.full((n,), float("nan"), dtype=torch.float64).pin_memory()
    out = run(src, tgt, lambda: tgt)
    out.update(nreduce=n, buffers_note="page-locked host memory (torch pin_memory) on every PE")
    del src, tgt
    psrc = (base * (rank + 1)).numpy().copy()
    ptgt = np.full(n, np.nan)
    out["pageable"] = run(psrc, ptgt, lambda: torch.from_numpy(ptgt))
    out["pageable_note"] = "numpy (pageable) arrays on every PE: the page-locked ring and its two copy gangs"
    return out


def config_extras(world, stream, barrier, max_over_ranks, cap=256 * 1024 * 1024):
    """BASELINE.json configs[3] and [4] as extra lines (not `value`):
    long and/or/xor over 64 Mi elements, and the float sum GiB/s-vs-size curve
    for nreduce 4 Ki .. 256 Mi (both capped at `cap` elements).  At N = 1 the
    step is the local fold (2 inputs), at N > 1 the full collective."""
    sp = stream.cuda_stream
    g = torch.Generator(device="cuda")
    g.manual_seed(0xC0F + int(os.environ.get("RANK", "0")))
    out = {}

    # Working sets under the 256 MiB Infinity Cache (MALL) stay on-die across
    # back-to-back steps, so a warm rate there is not HBM bandwidth (DESIGN.md
    # §4.2).  The "cold" rate reads a 1 GiB scratch before every step (a
    # read-only sweep: it evicts the step's arrays and leaves no dirty line)
    # and times the steps alone with HIP events on the stream: every step
    # starts from HBM.  Round 2 rewrote the scratch instead; the dirty lines
    # that left in the MALL were then written back inside the timed step
    # (profiles/r03_cold_midsize.txt) — that variant is kept, labelled, as
    # the rate right after a producer's writes.
    scratch = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    scratch64 = scratch.view(torch.float64)

    detail = {}

    def rate(type_name, op, n, elem, steps, cold=None):
        x = (torch.randint(-2**62, 2**62, (n,), dtype=torch.int64, device="cuda", generator=g)
             if elem == 8 and type_name == "long" else
             torch.rand(n, dtype=torch.float32, device="cuda", generator=g))
        y = torch.empty_like(x)
        torch.cuda.synchronize()
        if world == 1:
            fn = lambda: shm.fold(type_name, op, y, x, n, sp)          # noqa: E731
        else:
            fn = lambda: shm.reduce_on_stream(type_name, op, y, x, n, 0, 0, world, "auto", sp)  # noqa: E731
        for _ in range(2):
            fn()
        if cold:
            def cold_pass(clock):
                """`steps` flushed steps; marker-event seconds, and with the
                kernel clock on each fold's own duration (us list)"""
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                      for _ in range(steps)]
                barrier()
                torch.cuda.synchronize()
                if clock:
                    shm.kernel_timing(True)
                with torch.cuda.stream(stream):
                    for k, (e0, e1) in enumerate(ev):
                        if cold == "dirty":
                            scratch.fill_(k & 0xFF)
                        else:
                            scratch64.sum()
                        e0.record(stream)
                        fn()
                        e1.record(stream)
                torch.cuda.synchronize()
                kern = None
                if clock:
                    kt, _ = shm.kernel_times()
                    shm.kernel_timing(False)
                    kern = [us for kind, us in kt if kind == "fold"]
                return sum(e0.elapsed_time(e1) for e0, e1 in ev) * 1e-3, kern
            w_ev, _ = cold_pass(False)
            w = w_ev
            if world == 1:
                # N = 1: each fold's own duration from the library's kernel
                # clock (its dispatch's events), in a pass of its own; the
                # marker events of the pass above add the launch boundary and
                # their own latency, which a step of a few us cannot amortise
                _, kern = cold_pass(True)
                if kern and len(kern) == steps:
                    w = sum(kern) * 1e-6
                    detail.setdefault(cold, {})[str(n)] = {
                        "kernel_us": round(statistics.median(kern), 2),
                        "marker_event_us": round(w_ev / steps * 1e6, 2)}
        else:
            w, _ = time_region(fn, steps, stream, barrier)
        w = max_over_ranks(w)
        return round(world * n * elem * steps / w / GiB, 2)

    nlong = min(64 * 1024 * 1024, cap)
    for op in ("and", "or", "xor"):
        key = "64Mi" if nlong == 64 * 1024 * 1024 else str(nlong)
        out[f"long_{op}_{key}_GiBps"] = rate("long", op, nlong, 8, 10)
    cold, dirty, warm = {}, {}, {}
    n = 4 * 1024
    while n <= min(256 * 1024 * 1024, cap):
        steps = 20 if n >= 1 << 24 else 50
        cold[str(n)] = rate("float", "sum", n, 4, steps, cold="clean")
        dirty[str(n)] = rate("float", "sum", n, 4, steps, cold="dirty")
        warm[str(n)] = rate("float", "sum", n, 4, steps)
        n *= 4
    out["float_sum_GiBps_vs_nreduce"] = cold
    out["float_sum_GiBps_vs_nreduce_note"] = (
        "cold: a 1 GiB scratch is read (read-only sweep: evicts, leaves nothing dirty) before every "
        "step and only the steps are timed, so every step reads and writes HBM; GiB/s = PEs x "
        "nreduce x 4 B / step.  N = 1: the step is the fold kernel's own duration (the library's "
        "kernel clock, shmemx_kernel_times: start/stop events of the dispatch itself); "
        "float_sum_us_vs_nreduce gives it beside the marker-event time around each launch (a separate "
        "pass), whose difference is the launch boundary plus the markers' latency, not kernel work.  N > 1: "
        "marker events around the whole collective")
    if detail.get("clean"):
        out["float_sum_us_vs_nreduce"] = detail["clean"]
    if world > 1:
        # algbw = S / t per PE and busbw = algbw x
        # 2(P-1)/P (the bytes each GPU moves over xGMI in RS + AG), GB/s,
        # from the same cold timings (t = max over ranks per step)
        algbw, busbw = {}, {}
        for k, v in cold.items():
            t = world * int(k) * 4 / (v * GiB)          # seconds per step
            algbw[k] = round(int(k) * 4 / t / 1e9, 2)
            busbw[k] = round(algbw[k] * 2 * (world - 1) / world, 2)
        out["float_sum_algbw_GBps_vs_nreduce"] = algbw
        out["float_sum_busbw_GBps_vs_nreduce"] = busbw
    out["float_sum_GiBps_vs_nreduce_after_write_flush"] = dirty
    out["float_sum_GiBps_vs_nreduce_after_write_flush_note"] = (
        "the same, but the scratch is REWRITTEN before every step (round 2's flush): up to 256 MiB "
        "of its dirty lines sit in the Infinity Cache and are written back inside the timed step, "
        "as after a producer kernel's writes")
    out["float_sum_GiBps_vs_nreduce_warm_mall_resident"] = warm
    out["float_sum_GiBps_vs_nreduce_warm_note"] = (
        "back to back, no flush: working sets (3 x nreduce x 4 B at N = 1) under 256 MiB are served "
        "from the Infinity Cache; not HBM bandwidth")
    del scratch
    return out


_CALL_TIMER = None


def call_times_us(type_name, op, target, source, n, start, logstride, size, psync, warm, reps):
    """Per-call microseconds of the blocking shmem_<type>_<op>_to_all, each
    call timed from C (tools/libcalltimer.so: no Python between calls), or
    None if the helper is not built."""
    import ctypes
    global _CALL_TIMER
    if _CALL_TIMER is None:
        path = os.path.join(REPO, "tools", "libcalltimer.so")
        if not os.path.exists(path):
            return None
        L = ctypes.CDLL(path)
        vp, i = ctypes.c_void_p, ctypes.c_int
        L.call_timer_to_all.argtypes = [vp, vp, vp, i, i, i, i, vp, vp, i, i, ctypes.POINTER(ctypes.c_double)]
        L.call_timer_to_all.restype = i
        _CALL_TIMER = L
    fn = ctypes.cast(getattr(shm.lib(), f"shmem_{type_name}_{op}_to_all"), ctypes.c_void_p)
    out = (ctypes.c_double * max(1, reps))()
    rc = _CALL_TIMER.call_timer_to_all(fn, shm.addr(target), shm.addr(source), n, start, logstride, size,
                                       None, shm.addr(psync), warm, reps, out)
    return list(out)[:reps] if rc == 0 else None


def latency_extras(world, barrier, max_over_ranks):
    """Small-message latency of the blocking drop-in call (the ISx use:
    shmem_longlong_sum_to_all with nreduce = 1, isx.c:617), host- and
    device-resident, microseconds per call (max over ranks)."""
    import numpy as np
    out = {}
    psync = np.full(128, -1, dtype=np.int64)
    if hasattr(shm, "service_stats"):
        shm.service_stats(reset=True)
    for n in (1, 64, 4096):
        for where in ("host", "device"):
            if where == "host":
                src = np.arange(n, dtype=np.int64)
                tgt = np.zeros(n, dtype=np.int64)
            else:
                src = torch.arange(n, dtype=torch.int64, device="cuda")
                tgt = torch.zeros(n, dtype=torch.int64, device="cuda")
            for _ in range(5):
                shm.to_all("longlong", "sum", tgt, src, n, 0, 0, world, None, psync)
            barrier()
            reps = 200
            t0 = time.perf_counter()
            for _ in range(reps):
                shm.to_all("longlong", "sum", tgt, src, n, 0, 0, world, None, psync)
            t = max_over_ranks((time.perf_counter() - t0) / reps)
            out[f"longlong_sum_n{n}_{where}_us"] = round(t * 1e6, 1)
            # the same call from C, each call timed alone (median, min)
            barrier()
            ct = call_times_us("longlong", "sum", tgt, src, n, 0, 0, world, psync, 5, reps)
            if ct:
                out[f"longlong_sum_n{n}_{where}_from_c_us"] = {
                    "median": round(max_over_ranks(statistics.median(ct)), 2),
                    "min": round(max_over_ranks(min(ct)), 2)}
    # BASELINE configs[0]'s call, shmem_int_sum_to_all, at n = 1 / 1024 / 4096:
    # against the reference CPU's 3.0 / 3.9 / 8.8 us (cpu_baseline.table);
    # at PE_size 1 up to 32 KiB it is the resident service workgroup's
    # (csrc/service.hip), which these counters show
    if hasattr(shm, "service_stats"):
        out["service_stats_longlong"] = shm.service_stats(reset=True)
    for n in (1, 1024, 4096):
        for where in ("host", "device"):
            if where == "host":
                src = np.arange(n, dtype=np.int32)
                tgt = np.zeros(n, dtype=np.int32)
            else:
                src = torch.arange(n, dtype=torch.int32, device="cuda")
                tgt = torch.zeros(n, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
            barrier()
            ct = call_times_us("int", "sum", tgt, src, n, 0, 0, world, psync, 5, 500)
            if ct:
                out[f"int_sum_n{n}_{where}_from_c_us"] = {
                    "median": round(max_over_ranks(statistics.median(ct)), 2),
                    "p10": round(max_over_ranks(sorted(ct)[len(ct) // 10]), 2),
                    "min": round(max_over_ranks(min(ct)), 2)}
            want = np.arange(n, dtype=np.int32) * (world if world > 1 else 1)
            got = tgt if where == "host" else tgt.cpu().numpy()
            if world == 1 and not np.array_equal(got, want):
                out[f"int_sum_n{n}_{where}_error"] = "wrong result"
    if hasattr(shm, "service_stats"):
        out["service_stats_int"] = shm.service_stats(reset=True)
    out["from_c_note"] = ("*_from_c_us: the same blocking call timed call by call from C "
                          "(tools/call_timer.c), without the Python caller's overhead")
    return out


def config0_extra(world, rank, barrier, max_over_ranks, reps=300):
    """BASELINE.json configs[0] through the product: shmem_int_sum_to_all on
    2 PEs (PE_start 0, the first two GPUs; the other ranks skip the calls, as
    OpenSHMEM's non-members do), nreduce 1, 1024 (the config) and 4096,
    blocking calls from symmetric-heap operands (HBM, what `auto` runs
    device-resident) and from host arrays (the reference's heap is host
    memory), microseconds per call: median and min over `reps` calls timed one
    by one from C (tools/call_timer.c; the slower member's), beside the
    reference's CPU time for the same
    call (cpu_baseline.table at N = 1, 4.0-4.6 us at n = 1024).  Every target
    is checked exactly (integer sums)."""
    import numpy as np
    if world < 2:
        return "needs N >= 2"
    member = rank < 2
    psync = np.full(128, -1, dtype=np.int64)
    out = {}
    hs, ht = malloc_pair(4096 * 4)
    try:
        if not (hs and ht):
            return "shmem_malloc failed"
        for n in (1, 1024, 4096):
            base = np.arange(n, dtype=np.int32) % 977
            want = base * 2 + 1                        # PE 0: base, PE 1: base + 1
            mine = base + rank
            for where in ("heap", "host"):
                if where == "heap":
                    shm.memcpy(hs, mine, n * 4)
                    src, tgt = hs, ht
                else:
                    src, tgt = mine.copy(), np.zeros(n, dtype=np.int32)
                ts, ok = [], True
                barrier()
                if member:
                    ct = call_times_us("int", "sum", tgt, src, n, 0, 0, 2, psync, 5, reps)
                    if ct is not None:
                        ts = [t * 1e-6 for t in ct]
                    else:
                        for k in range(reps + 5):
                            t0 = time.perf_counter()
                            shm.to_all("int", "sum", tgt, src, n, 0, 0, 2, None, psync)
                            if k >= 5:
                                ts.append(time.perf_counter() - t0)
                    ok = shm.last_error() == 0
                if member:
                    got = np.empty(n, dtype=np.int32)
                    if where == "heap":
                        shm.memcpy(got, ht, n * 4)
                    else:
                        got = tgt
                    ok = ok and bool(np.array_equal(got, want))
                med = max_over_ranks(statistics.median(ts) if ts else 0.0)
                lo = max_over_ranks(min(ts) if ts else 0.0)
                out[f"n{n}_{where}"] = {"median_us": round(med * 1e6, 1), "min_us": round(lo * 1e6, 1),
                                        "calls": reps,
                                        "correct": max_over_ranks(0.0 if (ok or not member) else 1.0) == 0.0}
        algo = shm.plan("int", "sum", 1024, 0, 0, 2, min(rank, 1), world, "auto").algo
        out["plan_note"] = f"auto's plan for the 2-PE set at n = 1024: {algo}"
        out["method_note"] = ("shmem_int_sum_to_all on PEs 0-1 (BASELINE configs[0]), blocking, each call timed "
                              "alone; the reference's CPU time for the same call is cpu_baseline.table's "
                              "configs[0] rows (N = 1 line)")
        return out
    finally:
        if ht:
            shm.free(ht)
        if hs:
            shm.free(hs)


def heap_latency_extras(world, barrier, max_over_ranks):
    """Small-message latency with symmetric-heap operands (N > 1): DIRECT
    (host barriers) and SIGNAL (device barriers), each call waited for, as a
    blocking call would be; microseconds per call (max over ranks)."""
    out = {}
    hs, ht = malloc_pair(4096 * 8)
    try:
        if not (hs and ht):
            return "shmem_malloc failed"
        for algo in ("direct", "signal"):
            for n in (1, 64, 4096):
                def call():
                    shm.reduce_on_stream("longlong", "sum", ht, hs, n, 0, 0, world, algo)
                    torch.cuda.synchronize()
                for _ in range(5):
                    call()
                barrier()
                reps = 200
                t0 = time.perf_counter()
                for _ in range(reps):
                    call()
                t = max_over_ranks((time.perf_counter() - t0) / reps)
                out[f"longlong_sum_n{n}_heap_{algo}_us"] = round(t * 1e6, 1)
    except shm.ShmemError as e:
        out["error"] = str(e)
    finally:
        if ht:
            shm.free(ht)
        if hs:
            shm.free(hs)
    return out


def malloc_pair(nbytes):
    """Two symmetric-heap blocks (collective), zeroed."""
    hs, ht = shm.malloc(nbytes), shm.malloc(nbytes)
    for h in (hs, ht):
        if h:
            shm.memcpy(h, torch.zeros(nbytes, dtype=torch.uint8), nbytes)
    return hs, ht


def direct_extra(world, n, src, sp, stream, barrier, max_over_ranks, steps, algo="direct"):
    """SHMEMX_ALGO_DIRECT (host barriers) or SHMEMX_ALGO_SIGNAL (device
    barriers, stream-ordered) with source and target in the symmetric heap
    (HBM, IPC-mapped): each PE's kernels read its peers' arrays over xGMI in
    place (reduce-scatter then all-gather, both pulls).  Checked against the
    same ULP bound as the main line and for cross-PE consistency."""
    nbytes = n * 8
    hs = ht = 0
    try:
        hs, ht = shm.malloc(nbytes), shm.malloc(nbytes)
        if not hs or not ht:
            return "shmem_malloc failed"
        shm.memcpy(hs, src, nbytes)

        def step():
            shm.reduce_on_stream("double", "sum", ht, hs, n, 0, 0, world, algo, sp)
        for _ in range(2):
            step()
        shm.direct_stats(reset=True)
        w, _ = time_region(step, steps, stream, barrier)
        w = max_over_ranks(w)
        st = shm.direct_stats(reset=True)
        calls = st.pop("calls")
        phases = {k: round(max_over_ranks(st[k] / calls), 1) for k in shm.DIRECT_PHASES} if calls else {}
        # every fence that handed data between GPUs reached every XCD
        fences = {k: int(max_over_ranks(st.get(k, 0.0))) for k in shm.FENCE_STATS}
        remote = (world - 1) / world * nbytes          # bytes each PE pulls per phase
        for k in ("fold", "gather"):
            if phases.get(f"{k}_us"):
                phases[f"{k}_xgmi_read_GBps"] = round(remote / (phases[f"{k}_us"] * 1e-6) / 1e9, 1)
        got = torch.empty(n, dtype=torch.float64, device="cuda")
        shm.memcpy(got, ht, nbytes)
        sample = torch.arange(0, n, max(1, n // 4096), device="cuda")
        mine = src[sample].cpu()
        import torch.distributed as dist
        allv = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(allv, mine)
        ref = sum(allv[1:], allv[0].clone())
        tol = 2 * (world - 1) * 2.0 ** -53 * sum((v.abs() for v in allv[1:]), allv[0].abs())
        ok = bool(((got[sample].cpu() - ref).abs() <= tol).all())
        ok = shm.verify("double", ht, n, 0, 0, world) and ok
        ok = max_over_ranks(0.0 if ok else 1.0) == 0.0
        out = {"GiBps": round(world * nbytes * steps / w / GiB, 2),
               "ms_per_call": round(w / steps * 1e3, 3), "correct": ok}
        if phases:
            out["phases_per_call_max_over_ranks"] = phases
        out["fences_max_over_ranks"] = fences
        return out
    except shm.ShmemError as e:
        return str(e)
    finally:
        if ht:
            shm.free(ht)
        if hs:
            shm.free(hs)


def xgmi_extra(world, rank, sp, stream, barrier, max_over_ranks, nbytes=64 << 20):
    """Raw link rates between this GPU and its peers, measured with the
    library's gather (copy) kernel on IPC-mapped symmetric-heap blocks:
    pull = loads from the peers' HBM into my HBM (what DIRECT and SIGNAL do),
    push = stores from my HBM into the peers' HBM (what they never do: the
    data for deciding whether a store-based exchange would beat the pulls);
    from one peer (PE me+1) and from / to all peers at once.  GB/s per GPU,
    the slowest rank's; plus whether pushed bytes were visible to the peer
    after shmem_barrier_all (system fences on every XCD)."""
    if world < 2:
        return "needs N >= 2"
    blk = shm.malloc(nbytes)
    if not blk:
        return "shmem_malloc failed"
    try:
        peers = [q for q in range(world) if q != rank]
        paddr = {q: shm.heap_ptr(blk, q) for q in peers}
        # collective: every rank takes the same path
        if max_over_ranks(0.0 if all(paddr.values()) else 1.0) != 0.0:
            return "no IPC mapping of the peers' heap (node block down) on some rank"
        loc = torch.full((nbytes,), (rank + 1) & 0xFF, dtype=torch.uint8, device="cuda")
        nxt = (rank + 1) % world
        seg = (nbytes // len(peers)) // 16 * 16
        slot = (nbytes // world) // 16 * 16
        base = loc.data_ptr()
        cases = {
            "pull_one": ([paddr[nxt]], [base], [nbytes]),
            "pull_all": ([paddr[q] for q in peers], [base + i * seg for i in range(len(peers))],
                         [seg] * len(peers)),
            "push_one": ([base], [paddr[nxt]], [nbytes]),
            "push_all": ([base] * len(peers), [paddr[q] + rank * slot for q in peers], [slot] * len(peers)),
        }
        out = {"bytes_per_gpu": {}, "GBps_per_gpu": {}}
        for name, (src, dst, lens) in cases.items():
            if name.startswith("push"):
                # the pulls overwrote my buffer with the peers' bytes: my own
                # pattern again before anything is pushed from it
                loc.fill_((rank + 1) & 0xFF)
                torch.cuda.synchronize()

            def step(src=src, dst=dst, lens=lens):
                shm.gather(src, dst, lens, sp)
            for _ in range(2):
                step()
            k = 10
            w, _ = time_region(step, k, stream, barrier)
            w = max_over_ranks(w)
            out["bytes_per_gpu"][name] = sum(lens)
            out["GBps_per_gpu"][name] = round(sum(lens) * k / w / 1e9, 1)
        # visibility of stores into a peer's HBM: PE me - 1 writes its
        # pattern over my whole block once more, and after the library's
        # barrier (system fences on every XCD) my copy must read it
        src, dst, lens = cases["push_one"]
        shm.gather(src, dst, lens, sp)
        torch.cuda.synchronize()
        shm.barrier_all()
        got = torch.empty(4096, dtype=torch.uint8, device="cuda")
        shm.memcpy(got, blk + nbytes - 4096, 4096)
        writer = (rank - 1) % world
        ok = bool((got == ((writer + 1) & 0xFF)).all())
        out["push_visible_after_barrier"] = max_over_ranks(0.0 if ok else 1.0) == 0.0
        out["method_note"] = ("gather kernel (csrc/fold_kernels.hip) on IPC-mapped heap blocks: pull = peers' HBM -> "
                       "mine, push = mine -> peers' HBM; GB/s = bytes this GPU moved / time, max over ranks")
        return out
    finally:
        torch.cuda.synchronize()
        barrier()
        shm.free(blk)


def push_extra(world, rank, n, sp, stream, barrier, max_over_ranks, steps):
    """A store-based all-reduce composed from the library's public pieces (a
    measurement for the next algorithm, not a library path): every PE
    stores slice q of its source into PE q's receive block over the IPC
    mapping (one gather launch), shmem_barrier_all (system fences on every
    XCD), folds its slice from the P copies in its own HBM in set order
    (shmemx_fold_n), barrier, stores its result slice into every peer's
    target, barrier.  The same bytes cross the links as in DIRECT, as stores
    instead of loads, and the fold reads local HBM.  Sources are small
    integers, so every element of the target is checked exactly."""
    P = world
    if P < 2:
        return "needs N >= 2"
    sl = ((n + P - 1) // P + 1) // 2 * 2          # elements per slice, 16-B multiple

    def lo(i):
        return min(n, i * sl)

    def hi(i):
        return min(n, (i + 1) * sl)
    hs, ht = malloc_pair(n * 8)
    recv = shm.malloc(P * sl * 8)
    try:
        if not (hs and ht and recv):
            return "shmem_malloc failed"
        peers = [q for q in range(P) if q != rank]
        ps = {q: shm.heap_ptr(recv, q) for q in peers}
        pt = {q: shm.heap_ptr(ht, q) for q in peers}
        if max_over_ranks(0.0 if all(ps.values()) and all(pt.values()) else 1.0) != 0.0:
            return "no IPC mapping of the peers' heap (node block down) on some rank"
        base = exact_source(hs, n, rank)
        mlo, mhi = lo(rank), hi(rank)
        qs = [q for q in peers if hi(q) > lo(q)]
        p1 = ([hs + lo(q) * 8 for q in qs], [ps[q] + rank * sl * 8 for q in qs],
              [(hi(q) - lo(q)) * 8 for q in qs])
        ins = [hs + mlo * 8 if i == rank else recv + i * sl * 8 for i in range(P)]
        p3 = ([ht + mlo * 8] * len(peers), [pt[q] + mlo * 8 for q in peers], [(mhi - mlo) * 8] * len(peers))

        def call():
            if qs:
                shm.gather(*p1, sp)
            torch.cuda.synchronize()
            shm.barrier_all()
            if mhi > mlo:
                shm.fold_n("double", "sum", ht + mlo * 8, ins, mhi - mlo, sp)
            torch.cuda.synchronize()
            shm.barrier_all()
            if mhi > mlo:
                shm.gather(*p3, sp)
            torch.cuda.synchronize()
            shm.barrier_all()
        for _ in range(2):
            call()
        w, _ = time_region(call, steps, stream, barrier)
        w = max_over_ranks(w)
        ok = exact_target_ok(ht, base, n, range(P))
        return {"GiBps": round(P * n * 8 * steps / w / GiB, 2), "ms_per_call": round(w / steps * 1e3, 3),
                "correct": max_over_ranks(0.0 if ok else 1.0) == 0.0,
                "method_note": "push slices (gather kernel, stores over IPC) -> barrier_all -> local fold "
                               "(shmemx_fold_n) -> barrier_all -> push result slice -> barrier_all; "
                               "compare direct_heap (the same exchange as loads)"}
    finally:
        torch.cuda.synchronize()
        barrier()
        for h in (recv, ht, hs):
            if h:
                shm.free(h)


def coherence_extra(world, rank, sp, max_over_ranks, iters=20):
    """Cross-GPU coherence check of the IPC pulls (N > 1): DIRECT and SIGNAL
    on heap operands whose contents change on every call, at a fused one-shot
    (1 KiB), a fused two-shot (1 MiB) and a multi-launch two-shot (16 MiB)
    size.  Source values are small integers, (i mod 1024) + 7 * rank + 3 * it,
    so every PE's sum is exact in any order and the whole target is compared
    with it.  A stale line of a peer's previous source or target (an L2 that
    was not written back or invalidated on some XCD) shows up as mismatched
    elements.  Reports calls and the mismatches summed over elements, max
    over ranks."""
    sizes = [128, 1 << 17, 1 << 21]
    hs, ht = malloc_pair(sizes[-1] * 8)
    out = {}
    try:
        if not (hs and ht):
            return "shmem_malloc failed"
        for algo in ("direct", "signal"):
            bad = calls = 0
            err = None
            for it in range(iters):
                for n in sizes:
                    base = torch.arange(n, device="cuda", dtype=torch.float64).remainder_(1024)
                    shm.memcpy(hs, base + (7 * rank + 3 * it), n * 8)
                    try:
                        shm.reduce_on_stream("double", "sum", ht, hs, n, 0, 0, world, algo, sp)
                    except shm.ShmemError as e:
                        err = str(e)
                        break
                    torch.cuda.synchronize()
                    got = torch.empty(n, device="cuda", dtype=torch.float64)
                    shm.memcpy(got, ht, n * 8)
                    want = base * world + (7 * world * (world - 1) // 2 + 3 * it * world)
                    bad += int((got != want).sum().item())
                    calls += 1
                if err:
                    break
            out[algo] = err if err else {"calls": calls, "mismatched_elements": int(max_over_ranks(bad))}
    finally:
        if ht:
            shm.free(ht)
        if hs:
            shm.free(hs)
    return out


def exact_source(hs, n, rank):
    """Fill heap block hs with (i mod 1024) + rank: small integers, so any
    summation order gives the exact sum, and the target can be checked whole."""
    base = torch.arange(n, device="cuda", dtype=torch.float64).remainder_(1024)
    shm.memcpy(hs, base + rank, n * 8)
    return base


def exact_target_ok(ht, base, n, members):
    """Is the target [0, n) at hs's exact sum over `members` (ranks)?"""
    got = torch.empty(n, device="cuda", dtype=torch.float64)
    shm.memcpy(got, ht, n * 8)
    return bool(torch.equal(got, base * len(members) + float(sum(members))))


# The size buckets and set shapes `auto` chooses among (bytes per PE), and
# the algorithms the library's table ($SHMEMX_AUTO_FULL / _PARTIAL) may name:
# SIGNAL is timed but never a table choice (it needs heap operands on every
# PE; DIRECT takes any operand and runs the same fused launches on heap ones).
AUTO_BUCKETS = {"8B": 1, "4KiB": 1 << 9, "512KiB": 1 << 16, "4MiB": 1 << 19, "128MiB": 1 << 24}
AUTO_TABLE_ALGOS = {"full": ("allreduce", "rccl", "a2a", "direct", "gather"),
                    "partial": ("allreduce", "rccl", "a2a", "direct", "gather")}


def crossover_extra(world, rank, sp, stream, barrier, max_over_ranks, cap=1 << 24, out=None):
    """double sum over the full set, per algorithm and size, with source and
    target in the symmetric heap (so DIRECT and SIGNAL can run too): GiB/s of
    the whole job (N * n * 8 B / max-over-ranks time), microseconds per call,
    and whether every element of every PE's target was exact after the timed
    calls.  The data `auto`'s per-size choice (auto_recommendation) is set
    from.  `out` (if given) is filled cell by cell, so a watchdog that prints
    the line part-way still carries the cells measured so far."""
    sizes = sorted(set([1, 1 << 9, 1 << 12, 1 << 16, 1 << 18, 1 << 19, 1 << 20, 1 << 24]))
    sizes = [n for n in sizes if n <= cap] or [1]
    nbytes = sizes[-1] * 8
    hs, ht = malloc_pair(nbytes)
    out = {} if out is None else out
    out.update({"GiBps": {}, "us_per_call": {}, "correct": {}})
    try:
        if not (hs and ht):
            return "shmem_malloc failed"
        base = exact_source(hs, sizes[-1], rank)
        torch.cuda.synchronize()
        for algo in ("rccl", "allreduce", "a2a", "direct", "signal", "gather"):
            row, row_us, row_ok = {}, {}, {}
            out["GiBps"][algo] = row
            out["us_per_call"][algo] = row_us
            out["correct"][algo] = row_ok
            for n in sizes:
                def step(n=n, algo=algo):
                    shm.reduce_on_stream("double", "sum", ht, hs, n, 0, 0, world, algo, sp)
                try:
                    for _ in range(3):
                        step()
                    k = 20 if n <= 1 << 20 else 10
                    w, _ = time_region(step, k, stream, barrier)
                    w = max_over_ranks(w)
                    row[str(n)] = round(world * n * 8 * k / w / GiB, 4)
                    row_us[str(n)] = round(w / k * 1e6, 1)
                    ok = exact_target_ok(ht, base[:n], n, range(world))
                    row_ok[str(n)] = max_over_ranks(0.0 if ok else 1.0) == 0.0
                except shm.ShmemError as e:
                    row[str(n)] = row_us[str(n)] = row_ok[str(n)] = str(e)
        # the fused two-shot launch against the multi-launch two shot at the
        # same sizes (512 KiB, 2 MiB, 8 MiB per PE), to set
        # $SHMEMX_FUSED_TWOSHOT_KB's default from (every rank sets the same
        # limit before its calls)
        prev = shm.set_fused_twoshot_kb(0)
        try:
            cmp = {}
            for algo in ("direct", "signal"):
                cmp[algo] = {}
                for n in [m for m in (1 << 16, 1 << 18, 1 << 20) if m <= cap]:
                    cell = {}
                    for label, kb in (("fused", 16384), ("unfused", 0)):
                        shm.set_fused_twoshot_kb(kb)

                        def step(n=n, algo=algo):
                            shm.reduce_on_stream("double", "sum", ht, hs, n, 0, 0, world, algo, sp)
                        try:
                            for _ in range(3):
                                step()
                            w, _ = time_region(step, 10, stream, barrier)
                            cell[label] = round(max_over_ranks(w) / 10 * 1e6, 1)
                        except shm.ShmemError as e:
                            cell[label] = str(e)
                    cmp[algo][str(n)] = cell
            out["twoshot_fused_vs_unfused_us"] = cmp
        finally:
            shm.set_fused_twoshot_kb(prev)
    finally:
        if ht:
            shm.free(ht)
        if hs:
            shm.free(hs)
    return out


def subset_extra(world, rank, sp, stream, barrier, max_over_ranks, cap=1 << 24, out=None):
    """double sum on partial active sets (N >= 4): the first half of the PEs
    (PE_start 0, stride 1) and every other PE (PE_start 0, logPE_stride 1),
    heap operands, per algorithm, microseconds per call (max over ranks;
    non-members skip the call, as OpenSHMEM's do) and whether every member's
    target was exact.  `auto` sends the RCCL-native pairs on these sets
    through RCCL on the set's members-only communicator (set_comm.cpp; the
    first call builds it, so the warm-up calls absorb that); the table is the
    data to revisit it (auto_recommendation).
    `out` (if given) is filled cell by cell, as in crossover_extra."""
    if world < 4:
        return "needs N >= 4"
    sizes = [n for n in AUTO_BUCKETS.values() if n <= cap] or [1]
    hs, ht = malloc_pair(sizes[-1] * 8)
    out = {} if out is None else out
    try:
        if not (hs and ht):
            return "shmem_malloc failed"
        base = exact_source(hs, sizes[-1], rank)
        torch.cuda.synchronize()
        for name, (start, logstride, size) in (("first_half", (0, 0, world // 2)),
                                               ("every_other", (0, 1, world // 2))):
            members = [start + (i << logstride) for i in range(size)]
            member = rank in members
            table, table_ok = {}, {}
            out[f"{name}_us_per_call"] = table
            out[f"{name}_correct"] = table_ok
            for algo in ("rccl", "allreduce", "a2a", "direct", "signal", "gather"):
                row, row_ok = {}, {}
                table[algo] = row
                table_ok[algo] = row_ok
                for n in sizes:
                    failed = []

                    def step(n=n, algo=algo):
                        # never raises: a member's error must not leave the
                        # others waiting in time_region's barrier
                        if member and not failed:
                            try:
                                shm.reduce_on_stream("double", "sum", ht, hs, n, start, logstride, size,
                                                     algo, sp)
                            except shm.ShmemError as e:
                                failed.append(str(e))
                    for _ in range(3):
                        step()
                    k = 20 if n <= 1 << 16 else 10
                    w, _ = time_region(step, k, stream, barrier)
                    w = max_over_ranks(w)
                    if max_over_ranks(1.0 if failed else 0.0):
                        row[str(n)] = row_ok[str(n)] = failed[0] if failed else "error on another member"
                    else:
                        row[str(n)] = round(w / k * 1e6, 1)
                        ok = exact_target_ok(ht, base[:n], n, members) if member else True
                        row_ok[str(n)] = max_over_ranks(0.0 if ok else 1.0) == 0.0
    finally:
        if ht:
            shm.free(ht)
        if hs:
            shm.free(hs)
    return out


def auto_recommendation(crossover, partial):
    """The fastest correct algorithm per size bucket and set shape, from the
    crossover (full set) and partial_sets tables, as one compact object, plus
    the $SHMEMX_AUTO_FULL / $SHMEMX_AUTO_PARTIAL values that make the
    library's `auto` take it (runtime.cpp make_plan; "bytes:algo" cut
    points, ascending; a cut between two buckets sits at their geometric
    mean).  "fastest" names the fastest correct algorithm of all (SIGNAL
    included); "table" the fastest the table may name."""
    def best(us_row, ok_row, algos):
        cands = [(us_row[a], a) for a in algos
                 if isinstance(us_row.get(a), (int, float)) and ok_row.get(a) is True]
        return min(cands)[1] if cands else None

    shapes = {}
    if isinstance(crossover, dict):
        shapes["full"] = (crossover.get("us_per_call", {}), crossover.get("correct", {}))
    if isinstance(partial, dict):
        shapes["half"] = (partial.get("first_half_us_per_call", {}), partial.get("first_half_correct", {}))
        shapes["strided"] = (partial.get("every_other_us_per_call", {}), partial.get("every_other_correct", {}))
    out = {}
    for shape, (us, ok) in shapes.items():
        row = {}
        for label, n in AUTO_BUCKETS.items():
            us_n = {a: r.get(str(n)) for a, r in us.items()}
            ok_n = {a: r.get(str(n)) for a, r in ok.items()}
            kind = "full" if shape == "full" else "partial"
            row[label] = {"fastest": best(us_n, ok_n, list(us_n)),
                          "table": best(us_n, ok_n, AUTO_TABLE_ALGOS[kind]),
                          "us": {a: v for a, v in us_n.items() if isinstance(v, (int, float))}}
        out[shape] = row

    def env_value(rows):
        cuts, prev_n, prev_algo = [], None, None
        for label, n in AUTO_BUCKETS.items():
            algo = rows.get(label, {}).get("table")
            if algo is None:
                continue
            if algo != prev_algo:
                cut = 0 if prev_n is None else int(((prev_n * 8) * (n * 8)) ** 0.5)
                cuts.append(f"{cut}:{algo}")
                prev_algo = algo
            prev_n = n
        return ",".join(cuts)
    env = {}
    if "full" in out and env_value(out["full"]):
        env["SHMEMX_AUTO_FULL"] = env_value(out["full"])
    # one partial table for both partial shapes: the strided set's choice
    # (every other PE crosses the most links), else the half set's
    for shape in ("strided", "half"):
        if shape in out and env_value(out[shape]):
            env["SHMEMX_AUTO_PARTIAL"] = env_value(out[shape])
            break
    # $SHMEMX_FUSED_TWOSHOT_KB: the array size up to which DIRECT's and
    # SIGNAL's two shot runs as one fused launch, from the fused-vs-unfused
    # cells (512 KiB, 2 MiB, 8 MiB per PE): up to the last size where the
    # fused launch won for both, cut at the geometric mean with the first size
    # where it lost (256 KiB, the one shot's own limit, if it lost at once)
    kb = fused_twoshot_kb(crossover.get("twoshot_fused_vs_unfused_us")
                          if isinstance(crossover, dict) else None)
    if kb is not None:
        env["SHMEMX_FUSED_TWOSHOT_KB"] = str(kb)
    out["env"] = env
    return out


def fused_twoshot_kb(cells):
    """$SHMEMX_FUSED_TWOSHOT_KB from {algo: {str(n doubles): {"fused": us,
    "unfused": us}}}, or None without a usable cell."""
    if not isinstance(cells, dict):
        return None
    sizes = sorted({int(n) for row in cells.values() if isinstance(row, dict) for n in row})
    wins = []
    for n in sizes:
        verdicts = []
        for row in cells.values():
            c = row.get(str(n)) if isinstance(row, dict) else None
            if isinstance(c, dict) and all(isinstance(c.get(k), (int, float)) for k in ("fused", "unfused")):
                verdicts.append(c["fused"] <= c["unfused"])
        if not verdicts:
            break
        wins.append(all(verdicts))
    if not wins:
        return None
    lead = 0
    while lead < len(wins) and wins[lead]:
        lead += 1
    kib = [n * 8 // 1024 for n in sizes[:len(wins)]]
    if lead == 0:
        return 256
    if lead == len(wins):
        return kib[-1]
    return int((kib[lead - 1] * kib[lead]) ** 0.5)


def measured_ceiling(ptrs, nbytes, stream_ptr, reps=20):
    """The device's measured HBM streaming ceiling beside the spec peak
    (SURVEY §8d): tools/libceiling.so reads the given arrays (nbytes each)
    with 16-B non-temporal loads and nothing else, each launch timed by its
    own dispatch events; the median rate in GB/s.  A read-only stream is the
    fastest thing HBM does here (6.8-7.1 TB/s; a copy's honest rate is
    6.1-6.4, profiles/r04_stream_lab_*.txt), so no kernel that also writes
    can beat it.  None if the helper is not built."""
    import ctypes
    path = os.path.join(REPO, "tools", "libceiling.so")
    if not os.path.exists(path):
        return None
    L = ctypes.CDLL(path)
    dp = ctypes.POINTER(ctypes.c_double)
    L.ceiling_read.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_size_t,
                               ctypes.c_void_p, ctypes.c_int, dp, dp]
    L.ceiling_read.restype = ctypes.c_int
    arr = (ctypes.c_void_p * len(ptrs))(*ptrs)
    med, lo = ctypes.c_double(), ctypes.c_double()
    if L.ceiling_read(arr, len(ptrs), nbytes, stream_ptr, reps, ctypes.byref(med), ctypes.byref(lo)):
        return None
    total = len(ptrs) * nbytes
    return {"kernel": f"read-only stream of {len(ptrs)} x {nbytes >> 20} MiB (the bench's own arrays), "
                      f"16-B non-temporal loads, 256 lanes x 4 vectors per array (tools/ceiling.hip)",
            "bytes_per_launch": total, "median_us": round(med.value, 2), "min_us": round(lo.value, 2),
            "GBps": round(total / med.value / 1e3, 1), "launches": reps}


DUMP_LIMIT_BYTES = 64 * 1000 * 1000   # --dump-outputs writes at most this much
DUMP_SAMPLE = 1 << 20                 # elements written of an array over the limit
DUMP_SEED = 0xD0D0


def dump_indices(n: int):
    """The elements --dump-outputs writes of an n-element float64 array: all
    of them (None) if they fit DUMP_LIMIT_BYTES, else DUMP_SAMPLE sorted
    indices drawn once from a seeded generator (the same for every run and
    build, whatever the array holds)."""
    import numpy as np
    if n * 8 <= DUMP_LIMIT_BYTES:
        return None
    return np.sort(np.random.default_rng(DUMP_SEED).integers(0, n, size=DUMP_SAMPLE, dtype=np.int64))


def dump_output(dirname: str, name: str, values, n: int):
    """Write `values` (a float64 CUDA tensor of n elements: the timed path's
    output array) or its fixed sample as dirname/name.npy; returns what was
    written, for the line."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    idx = dump_indices(n)
    if idx is None:
        out = values.cpu().numpy()
    else:
        out = values[torch.from_numpy(idx).to(values.device)].cpu().numpy()
    out = np.ascontiguousarray(out, dtype=np.float64)
    path = os.path.join(dirname, name + ".npy")
    np.save(path, out)
    return {"file": name + ".npy", "dtype": "float64", "elements": int(out.size), "of": n,
            "sample": None if idx is None else f"numpy default_rng({DUMP_SEED:#x}).integers(0, {n}, "
                                               f"{DUMP_SAMPLE}), sorted"}


def time_region(fn, steps, stream, barrier):
    """Run fn() `steps` times on `stream`; returns (wall_s, event_s)."""
    barrier()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    start.record(stream)
    for _ in range(steps):
        fn()
    stop.record(stream)
    torch.cuda.synchronize()
    barrier()
    t1 = time.perf_counter()
    return t1 - t0, start.elapsed_time(stop) * 1e-3


def stage(rank, what):
    """Progress on stderr (the JSON line stays alone on stdout): where a run
    that never prints its line stopped."""
    print(f"[bench rank {rank} {time.strftime('%H:%M:%S')}] {what}", file=sys.stderr, flush=True)


def main():
    a = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # a run stuck anywhere (RCCL bootstrap, a collective) leaves every
    # thread's Python stack on stderr after 10 minutes
    import faulthandler
    faulthandler.dump_traceback_later(600, exit=False)
    stage(rank, f"start: {world} rank(s), steps {a.steps}, warm-up {a.warmup}")
    if a.gpus != world:
        if world == 1 and a.gpus > 1:
            sys.exit("bench.py --gpus N>1 must be launched with torch.distributed.run")
        print(f"warning: --gpus {a.gpus} but WORLD_SIZE={world}; using {world}", file=sys.stderr)
    # SHMEMX_SHARE_GPU=1: every rank on device 0 (a rehearsal of the N > 1
    # path on a one-GPU box, IPC transport only; never a reported number)
    share = os.environ.get("SHMEMX_SHARE_GPU") == "1"
    # $FAKE_RCCL: the RCCL test double (tests/native/fake_rccl.cpp) in place
    # of librccl, so the RCCL transport can be rehearsed with every rank on
    # one GPU; its numbers are a host-memory shim's, never reported
    fake_rccl = os.environ.get("FAKE_RCCL")
    if fake_rccl:
        import ctypes
        ctypes.CDLL(fake_rccl, mode=ctypes.RTLD_GLOBAL)
    if share and os.environ.get("SHMEMX_TRANSPORT") != "ipc" and not fake_rccl:
        sys.exit("SHMEMX_SHARE_GPU=1 needs SHMEMX_TRANSPORT=ipc or $FAKE_RCCL "
                 "(RCCL refuses two ranks on one GPU)")
    local = 0 if share else local
    torch.cuda.set_device(local)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")
        shm.init_from_torch_distributed(device=local)
    else:
        shm.init_attr(0, 1, local, None)

    def barrier():
        if dist is not None:
            dist.barrier()

    def max_over_ranks(x: float) -> float:
        if dist is None:
            return x
        t = torch.tensor([x], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    n = a.nreduce
    nbytes = n * 8
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    g = torch.Generator(device="cuda")
    g.manual_seed(0x5EED0000 + rank)
    src = torch.rand(n, dtype=torch.float64, device="cuda", generator=g) + 1.0   # [1, 2)
    tgt = torch.empty_like(src)
    torch.cuda.synchronize()

    extras = {}
    # The operands live in the symmetric heap (shmem_malloc, one HBM segment
    # per PE), as the reference's source/target are symmetric objects carved
    # from its heap (memory/symmem.c:168-227).  Heap blocks also give the
    # fold a steady 122 us, where separately allocated torch tensors land on
    # a slow physical pairing now and then (129 us; profiles/archive/r01_placement_*).
    heap_blocks = [shm.malloc(nbytes) for _ in range(2)]
    use_heap = max_over_ranks(0.0 if all(heap_blocks) else 1.0) == 0.0

    def arr(t, k):
        """Address of the k-th operand, holding t's values."""
        if not use_heap:
            return t
        torch.cuda.synchronize()
        shm.memcpy(heap_blocks[k], t, nbytes)
        return heap_blocks[k]

    if world == 1:
        workload = "local reduce (fold acc = acc + in) of shmem_double_sum_to_all, 1 PE"
        inp_t = torch.rand(n, dtype=torch.float64, device="cuda", generator=g) + 1.0
        acc = arr(src.clone(), 0)
        inp = arr(inp_t, 1)

        def step():
            shm.fold("double", "sum", acc, inp, n, sp)
        alg_bytes = 3 * nbytes                 # read acc, read in, write acc
        algo_used = "fold"
    else:
        if fake_rccl:
            over = "RCCL TEST DOUBLE through host memory, all ranks on one GPU (rehearsal)"
        elif share:
            over = "IPC transport, all ranks on one GPU (rehearsal)"
        else:
            over = "RCCL over xGMI"
        workload = f"shmem_double_sum_to_all on {world} PEs (one per GPU), {over}"
        algo_used = a.algo
        src_a = arr(src, 0)
        tgt_a = heap_blocks[1] if use_heap else tgt

        def step():
            shm.reduce_on_stream("double", "sum", tgt_a, src_a, n, 0, 0, world, algo_used, sp)
        alg_bytes = None

    stage(rank, f"operands ready ({workload}); warm-up")
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    stage(rank, "timed region")
    wall, ev = time_region(step, a.steps, stream, barrier)
    stage(rank, "timed region done")
    dumped = None
    if a.dump_outputs and rank == 0:
        # what the last timed step left in the timed path's output array,
        # before anything below runs another step on it
        out_a, out_name = (acc, "acc") if world == 1 else (tgt_a, "target")
        if isinstance(out_a, int):
            blk, out_a = out_a, torch.empty_like(src)
            shm.memcpy(out_a, blk, nbytes)
        torch.cuda.synchronize()
        dumped = dump_output(a.dump_outputs, out_name, out_a, n)
        del out_a
        stage(rank, f"outputs written to {a.dump_outputs}")
    wall = max_over_ranks(wall)
    ev = max_over_ranks(ev)
    ms_per_step = wall / a.steps * 1e3
    # algbw: one PE's array per call time, at every N
    value = nbytes * a.steps / wall / GiB
    aggregate = world * value
    guard = None

    # correctness guard on what was timed (--full)
    if not a.full:
        ok = None
    elif world == 1:
        # one more step on the very arrays that were timed, from a known acc
        chk = arr(src.clone(), 0)
        torch.cuda.synchronize()
        shm.fold("double", "sum", chk, inp, n, sp)
        torch.cuda.synchronize()
        got = torch.empty_like(src)
        shm.memcpy(got, chk, nbytes)
        ok = torch.equal(got, src + inp_t)
    else:
        def sum_guard(record=None):
            """The timed target against the reference's result on EVERY
            element: each PE regenerates all N sources on its own GPU from
            their seeds (0x5EED0000 + rank, the generator is deterministic on
            one device type), folds them left to right in PE_start order in
            fp64 (reduce-op.c:219-248; the oracle's order) and holds the target
            to the stated bound |d| <= 2 gamma(N-1) sum_p |x_p|; NaN anywhere
            fails.  And identical on every PE (checksum of the whole target,
            compared across the set).  record: filled with what was checked."""
            if use_heap:
                shm.memcpy(tgt, tgt_a, nbytes)
            torch.cuda.synchronize()
            if a.corrupt_guard_test and rank == 0:
                # the guard's negative control (tests only): one element off
                # by far more than the bound
                tgt[n // 2] += 1e-6
            gen = torch.Generator(device="cuda")
            ref = abs_sum = None
            for p in range(world):
                gen.manual_seed(0x5EED0000 + p)
                x = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) + 1.0
                if ref is None:
                    ref, abs_sum = x.clone(), x.abs()
                else:
                    ref.add_(x)
                    abs_sum.add_(x.abs())
                del x
            u = 2.0 ** -53
            k = world - 1
            bound = abs_sum.mul_(2 * k * u / (1 - k * u) * (1 + 2 * world * u))
            err = (tgt - ref).abs_()
            bad = int((~(err <= bound)).sum().item())            # NaN counts as bad
            inexact = int((tgt.view(torch.int64) != ref.view(torch.int64)).sum().item())
            worst = float((err / bound.clamp_min(1e-300)).max().item())
            same = shm.verify("double", tgt, n, 0, 0, world)
            del ref, bound, err
            good = bad == 0 and same
            if record is not None:
                record.update({"elements_checked": n, "elements_out_of_bound": int(max_over_ranks(bad)),
                               "elements_not_bit_equal_to_pe_order": int(max_over_ranks(inexact)),
                               "max_err_over_bound": round(max_over_ranks(worst), 4),
                               "same_on_every_pe": max_over_ranks(0.0 if same else 1.0) == 0.0,
                               "reference": "fp64 left fold of every PE's regenerated source in PE_start "
                                            "order (reduce-op.c:219-248), bound 2 gamma(N-1) sum|x|"})
            return max_over_ranks(0.0 if good else 1.0) == 0.0
        guard = {}
        ok = sum_guard(guard)

    if world == 1:
        t_launch = ev / a.steps
        achieved = alg_bytes / t_launch / 1e9
        traffic, traffic_note = pmc_traffic("fold_double_sum")
        roofline = {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS,
                    "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
                    "traffic": traffic, "traffic_note": traffic_note,
                    "device_code_sha256": shm.device_code_sha256(), "alg_bytes_per_launch": alg_bytes,
                    "avg_launch_us": round(t_launch * 1e6, 2),
                    "kernel": "fold_kernel<double,SUM,2 inputs>"}
        if a.full:
            # cross-check of avg_launch_us (HIP events over the timed region): K
            # more launches of the same step, each timed by its own dispatch
            # events (the library's kernel clock), after the timed region
            try:
                torch.cuda.synchronize()
                shm.kernel_timing(True)
                for _ in range(a.steps):
                    step()
                torch.cuda.synchronize()
                kt, _ = shm.kernel_times()
                shm.kernel_timing(False)
                kus = [us for kind, us in kt if kind == "fold"]
                if kus:
                    roofline["kernel_clock_us"] = {"mean": round(statistics.mean(kus), 2),
                                                   "median": round(statistics.median(kus), 2),
                                                   "min": round(min(kus), 2), "launches": len(kus)}
            except Exception as e:   # noqa: BLE001 — a cross-check, never the headline
                roofline["kernel_clock_us"] = f"error: {type(e).__name__}: {e}"
            # the measured streaming ceiling beside the spec peak:
            # a read-only stream over the bench's own three 256 MiB arrays
            try:
                ptr = lambda x: x if isinstance(x, int) else x.data_ptr()   # noqa: E731
                mc = measured_ceiling([ptr(acc), ptr(inp), tgt.data_ptr()], nbytes, sp)
                if mc:
                    roofline["measured_ceiling_GBps"] = mc["GBps"]
                    roofline["frac_of_measured_ceiling"] = round(achieved / mc["GBps"], 4)
                    roofline["measured_ceiling"] = mc
            except Exception as e:   # noqa: BLE001
                roofline["measured_ceiling"] = f"error: {type(e).__name__}: {e}"
    else:
        t_call = ev / a.steps
        xgmi_bytes = 2 * (world - 1) / world * nbytes        # per GPU, RS + AG
        achieved = xgmi_bytes / t_call / 1e9
        peak = (world - 1) * XGMI_LINK_GBS
        roofline = {"bound": "xgmi", "achieved": round(achieved, 1), "peak": peak,
                    "unit": "GB/s", "frac": round(achieved / peak, 4), "traffic": None,
                    "alg_bytes_per_launch": int(xgmi_bytes),
                    "avg_launch_us": round(t_call * 1e6, 2),
                    "busbw_GBps": round(achieved, 1),
                    "peak_basis": XGMI_PEAK_BASIS,
                    "algbw_GiBps": round(nbytes / t_call / GiB, 2),
                    "algbw_note": "algbw here from HIP events on the stream; value from the wall clock "
                                  "around the timed steps (max over ranks)"}

    cpu = None
    if a.full and rank == 0 and not a.no_cpu_baseline:
        # the reference's CPU src/reduce on this host, in the same run
        # (north_star): at N > 1 the line's own config on N PE processes
        stage(rank, "cpu baseline")
        try:
            cpu = cpu_baseline(n, a.cpu_reps if world == 1 else a.cpu_reps_multi, world)
        except Exception as e:   # noqa: BLE001 — a reported baseline, never the headline
            cpu = {"value": None, "error": f"{type(e).__name__}: {e}", "cores": world}
        if world == 1 and a.cpu_table:
            # every BASELINE.json config on the host cores (BASELINE.md's plan);
            # the P = 1 double-sum row sits beside this N = 1 GPU value
            try:
                cpu["table"] = cpu_baseline_table()
            except Exception as e:   # noqa: BLE001 — a reported baseline, never the headline
                cpu["table"] = f"error: {type(e).__name__}: {e}"

    barrier()     # the other ranks wait here while rank 0 times the CPU leg

    line = {
        "metric": "GiB/s device-resident shmem_double_sum_to_all, nreduce=32Mi, 1/2/4/8 GPUs",
        "value": round(value, 2), "unit": "GiB/s", "n_gpus": world, "steps": a.steps,
        "warmup": a.warmup, "ms_per_step": round(ms_per_step, 4), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": workload, "nreduce": n, "type": "double", "op": "sum",
                   "PE_size": world,
                   "algo": algo_used if world == 1 else
                   shm.plan("double", "sum", n, 0, 0, world, rank, world, algo_used).algo,
                   "parallelism": f"one PE per GPU x{world}",
                   "transport": os.environ.get("SHMEMX_TRANSPORT", "rccl") if world > 1 else
                   "none (one PE: the step is the local fold, no exchange)",
                   "arrays": "symmetric heap (shmem_malloc, HBM)" if use_heap else "hipMalloc (torch)"},
        "roofline": roofline, "cpu_baseline": cpu, "correct": ok, "extras": extras,
        "full": a.full, "outputs": dumped,
    }
    if world > 1:
        line["aggregate_GiBps"] = round(aggregate, 2)
        line["value_definition"] = (
            "value = algbw = nreduce x 8 B / time per call (SURVEY.md 8(d) config 3), the rate of one PE's "
            "array; aggregate_GiBps = N x value (every PE's input bytes per second); roofline.busbw_GBps "
            "= algbw x 2(N-1)/N in GB/s; cpu_baseline.value is algbw the same way.  extras' *_GiBps "
            "fields at N > 1 are aggregate (N x nreduce x size / t) unless named algbw")
        line["guard"] = guard
    emitted = threading.Lock()
    exit_code = 1 if ok is False else 0      # a plain run checks nothing: ok is None

    def emit(note=None):
        """Print the one JSON line (rank 0), at most once."""
        if not emitted.acquire(blocking=False):
            return
        shm.set_fatal_note(None)       # the line is printed here, not by the handler
        if note:
            line["extras"] = dict(extras, note=note)
            # cut short by the watchdog: the recommendation from the cells
            # the crossover / partial-set tables hold so far
            if world > 1 and "auto_recommendation" not in extras:
                try:
                    line["extras"]["auto_recommendation"] = dict(
                        auto_recommendation(extras.get("algo_crossover"), extras.get("partial_sets")),
                        note="from the cells measured before the extras were cut short")
                except Exception as e:   # noqa: BLE001
                    line["extras"]["auto_recommendation"] = f"error: {type(e).__name__}: {e}"
        if rank == 0:
            print(json.dumps(line), flush=True)

    def arm_fatal_note(running):
        """If this process dies on a fatal signal while `running` (a FATAL
        abort in an RCCL/HIP call, a GPU fault, the launcher's SIGTERM after
        another rank died), rank 0 still prints the measured line, with the
        extras finished so far."""
        text = ""
        if rank == 0:
            text = json.dumps(dict(line, extras=dict(
                extras, note=f"extras stopped by a fatal signal during {running}"))) + "\n"
        shm.set_fatal_note(text, exit_code)

    # The headline is measured and checked by now.  The extras below exercise
    # other algorithms and API forms; a hang among them must not cost the
    # line: after --extras-timeout seconds every rank prints what it has
    # (rank 0) and leaves.
    def watchdog():
        emit(f"extras stopped after {a.extras_timeout} s (timeout)")
        if rank != 0:
            # every rank's timer fires within milliseconds of the others';
            # the others leave a moment after rank 0 has printed, so rank 0
            # does not first see a peer vanish from a collective and take
            # the extra's error path instead
            time.sleep(2.0)
        os._exit(exit_code)
    timer = threading.Timer(a.extras_timeout, watchdog)
    timer.daemon = True
    if a.full:
        timer.start()

    only = {x for x in a.extras_only.split(",") if x}

    def guarded(name, fn):
        if only and name not in only:
            return
        arm_fatal_note(name)
        stage(rank, f"extra {name}")
        try:
            extras[name] = fn()
        except Exception as e:   # noqa: BLE001 — an extra never costs the headline
            extras[name] = f"error: {type(e).__name__}: {e}"

    if not a.full:
        pass      # a plain run: the line as it stands
    elif world == 1:
        if a.extras:
            # the drop-in call itself at PE_size = 1 (copy semantics, reduce-op.c:213-216)
            def api_pe_size_1():
                def api_step():
                    shm.reduce_on_stream("double", "sum", tgt, src, n, 0, 0, 1, "auto", sp)
                for _ in range(3):
                    api_step()
                k2 = max(5, a.steps // 2)
                w2, e2 = time_region(api_step, k2, stream, barrier)
                # and each call's copy kernel by its own dispatch events
                shm.kernel_timing(True)
                for _ in range(k2):
                    api_step()
                torch.cuda.synchronize()
                kt, _ = shm.kernel_times()
                shm.kernel_timing(False)
                kus = [us for kind, us in kt if kind == "copy"]
                t_ev = e2 / k2
                out = {"clock_events": {"us_per_call": round(t_ev * 1e6, 2),
                                        "GiBps": round(nbytes / t_ev / GiB, 1),
                                        "hbm_GBps": round(2 * nbytes / t_ev / 1e9, 1)},
                       "clock_wall": {"us_per_call": round(w2 / k2 * 1e6, 2),
                                      "GiBps": round(nbytes / (w2 / k2) / GiB, 1)},
                       "note": "each block's fields come from one clock: HIP events over the timed "
                               "calls, the host's wall clock, the copy kernel's own dispatch events"}
                if kus:
                    ku = statistics.median(kus)
                    out["clock_kernel"] = {"kernel": "fold_kernel<T,SUM,1 input,1 vector,nt> (the copy)",
                                           "us": round(ku, 2), "hbm_GBps": round(2 * nbytes / ku / 1e3, 1)}
                return out
            guarded("api_pe_size_1", api_pe_size_1)
            guarded("host_resident_e2e", lambda: host_e2e(n))
            guarded("configs", lambda: config_extras(world, stream, barrier, max_over_ranks,
                                                     a.extras_max_nreduce))
            guarded("latency", lambda: latency_extras(world, barrier, max_over_ranks))

            def isx_mirrored_round():
                """ISx's nreduce = 1 round (a host store, shmem_longlong_sum_to_all,
                a host load: examples/ISx/SHMEM/isx.c:615-624) on the library's
                default mirrored heap, timed in a child process (the heap mode
                is per process; this one hands out HBM addresses)."""
                import subprocess
                env = dict(os.environ)
                env.pop("SHMEMX_HEAP_MEMORY", None)   # the library's default: mirrored
                r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "isx_mirror_latency.py"), "2000"],
                                   capture_output=True, text=True, timeout=120, env=env)
                found = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
                if r.returncode != 0 or not found:
                    return f"error: exit {r.returncode}: {r.stderr[-300:]}"
                d = json.loads(found[-1])
                return {k: d[k] for k in ("round_us", "call_us", "host_load_us", "rounds",
                                          "mirror_stats_per_round")} | {"tool": "tools/isx_mirror_latency.py"}
            guarded("isx_mirrored_round", isx_mirrored_round)
    elif a.extras:
        for alt in ("rccl", "allreduce", "a2a", "gather"):
            if alt == algo_used:
                continue

            def alt_rate(alt=alt):
                def alt_step():
                    shm.reduce_on_stream("double", "sum", tgt, src, n, 0, 0, world, alt, sp)
                try:
                    for _ in range(2):
                        alt_step()
                    k3 = max(3, a.steps // 4)
                    w3, _ = time_region(alt_step, k3, stream, barrier)
                    w3 = max_over_ranks(w3)
                    return round(world * nbytes * k3 / w3 / GiB, 2)
                except shm.ShmemError as e:
                    return str(e)
            guarded(f"algo_{alt}_GiBps", alt_rate)
        if use_heap and os.environ.get("SHMEMX_TRANSPORT", "rccl") != "ipc":
            # the RCCL algorithms again with the heap segment registered with
            # RCCL (shmemx_rccl_register_heap): whether RCCL then moves the
            # heap operands in place, faster, before it is made a default
            def rccl_registered():
                res = {}
                shm.rccl_register_heap(True)
                try:
                    for alt in ("rccl", "allreduce"):
                        def reg_step(alt=alt):
                            shm.reduce_on_stream("double", "sum", tgt_a, src_a, n, 0, 0, world, alt, sp)
                        for _ in range(2):
                            reg_step()
                        k3 = max(3, a.steps // 4)
                        w3, _ = time_region(reg_step, k3, stream, barrier)
                        res[f"algo_{alt}_GiBps"] = round(world * nbytes * k3 / max_over_ranks(w3) / GiB, 2)
                        res[f"algo_{alt}_correct"] = sum_guard()
                finally:
                    shm.rccl_register_heap(False)
                res["headline_unregistered_GiBps"] = round(value, 2)
                # adopt it (an environment change) only where it is correct and
                # at least 3 % faster than the unregistered headline
                best = max(res["algo_rccl_GiBps"] if res["algo_rccl_correct"] else 0.0,
                           res["algo_allreduce_GiBps"] if res["algo_allreduce_correct"] else 0.0)
                res["recommend_env"] = {"SHMEMX_RCCL_REGISTER": "1"} if best > 1.03 * value else {}
                return res
            guarded("rccl_registered", rccl_registered)
        guarded("configs", lambda: config_extras(world, stream, barrier, max_over_ranks,
                                                     a.extras_max_nreduce))
        guarded("latency", lambda: latency_extras(world, barrier, max_over_ranks))
        guarded("config0", lambda: config0_extra(world, rank, barrier, max_over_ranks))
        guarded("host_resident_e2e", lambda: host_e2e_multi(world, rank, min(n, a.extras_max_nreduce),
                                                            barrier, max_over_ranks))
        # last: the kernels that load from the peers' HBM through IPC mappings
        guarded("direct_heap", lambda: direct_extra(world, n, src, sp, stream, barrier,
                                                    max_over_ranks, max(3, a.steps // 4)))
        guarded("signal_heap", lambda: direct_extra(world, n, src, sp, stream, barrier,
                                                    max_over_ranks, max(3, a.steps // 4), "signal"))
        guarded("coherence", lambda: coherence_extra(world, rank, sp, max_over_ranks))
        guarded("heap_latency", lambda: heap_latency_extras(world, barrier, max_over_ranks))
        # these two fill their tables cell by cell in place (extras[name] is
        # the table from the start), so a watchdog cut keeps what they measured
        if not only or "algo_crossover" in only:
            extras["algo_crossover"] = {}
        guarded("algo_crossover", lambda: crossover_extra(world, rank, sp, stream, barrier,
                                                          max_over_ranks, a.extras_max_nreduce,
                                                          out=extras.get("algo_crossover")))
        if not only or "partial_sets" in only:
            extras["partial_sets"] = {}
        guarded("partial_sets", lambda: subset_extra(world, rank, sp, stream, barrier, max_over_ranks,
                                                     a.extras_max_nreduce, out=extras.get("partial_sets")))
        guarded("auto_recommendation", lambda: auto_recommendation(extras.get("algo_crossover"),
                                                                   extras.get("partial_sets")))
        # the very last: the first stores into the peers' HBM over xGMI any
        # run makes (the library itself only loads from the peers), after
        # everything the next round's settings are read from
        guarded("xgmi_links", lambda: xgmi_extra(world, rank, sp, stream, barrier, max_over_ranks))
        xl = extras.get("xgmi_links")
        if isinstance(xl, dict) and (xl.get("GBps_per_gpu") or {}).get("pull_all"):
            # the links' measured rate beside the spec peak: a copy kernel
            # pulling from every peer at once (the all-gather's pattern)
            meas = xl["GBps_per_gpu"]["pull_all"]
            line["roofline"]["measured_link_ceiling_GBps"] = meas
            line["roofline"]["frac_of_measured_links"] = round(achieved / meas, 4)
        guarded("push_allreduce", lambda: push_extra(world, rank, n, sp, stream, barrier, max_over_ranks,
                                                     max(3, a.steps // 4)))

    timer.cancel()
    faulthandler.cancel_dump_traceback_later()
    emit()
    stage(rank, "line printed")
    for blk in heap_blocks:
        if blk:
            shm.free(blk)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    # N = 1 leaves normally (shmem_finalize, then the interpreter's own exit),
    # so whatever observes the process at exit (exit handlers, library
    # destructors, a profiler's tool) runs, as for any program that loads the
    # library.  N > 1 leaves without the interpreter's and the runtimes'
    # exit-time teardown (RCCL communicator, HIP): the line is out, and
    # nothing the driver reads depends on it (the node block's /dev/shm name
    # went at init); except under rocprofv3 (it sets ROCPROF* variables),
    # whose tool writes the traces and counters at exit.
    sys.stdout.flush()
    sys.stderr.flush()
    if world == 1 or any(k.startswith("ROCPROF") for k in os.environ):
        shm.finalize()
        sys.exit(exit_code)
    os._exit(exit_code)


if __name__ == "__main__":
    main()
