"""Every typed stream-ordered form and every Fortran forwarder of
csrc/entry.cpp, called by its exported name across 3 PE processes on one GPU
(tests/gpu_entry_child.py) and held bit for bit to the oracle's result for
the (type, op) its name promises (tests/entry_table.py).

At PE_size = 1 every reduction is a copy, so a row of those tables wired to
another op or to another type of the same size passes; here it cannot
(test_entry_table.py::test_discrimination_census).  The sets (0,1,2) = PEs
{0, 2} and (1,0,2) = PEs {1, 2} are each other's image under a swap of
PE_start and logPE_stride, so a forwarder that dereferences them in the wrong
order turns a member into a non-member.

The PE processes are started as tests/test_gpu_pull.py starts its own: IPC
transport, device heap, a 10 s device-barrier timeout."""
import json
import os
import signal
import subprocess
import sys

import pytest

import entry_table as et

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "gpu_entry_child.py")

pytestmark = pytest.mark.gpu


def run_pes(tmp_path, npes, timeout=300):
    boot = str(tmp_path / "uid")
    procs = []
    for pe in range(npes):
        env = dict(os.environ, SHMEM_PE=str(pe), SHMEM_NPES=str(npes), LOCAL_RANK="0",
                   SHMEM_BOOTSTRAP_FILE=boot, SHMEMX_TRANSPORT="ipc", SHMEMX_BARRIER_TIMEOUT="120",
                   SHMEMX_HEAP_MEMORY="device", SHMEMX_SIGNAL_TIMEOUT="10")
        for k in ("RANK", "WORLD_SIZE", "SHMEM_REDUCE_ALGO", "SHMEMX_DEBUG"):   # the defaults
            env.pop(k, None)
        out = str(tmp_path / f"pe{pe}.json")
        log = open(tmp_path / f"pe{pe}.log", "w")
        procs.append((subprocess.Popen([sys.executable, CHILD, out], env=env, stdout=log,
                                       stderr=subprocess.STDOUT, start_new_session=True), out, log))
    try:
        rcs = [p.wait(timeout=timeout) for p, _, _ in procs]
    finally:
        for p, _, _ in procs:
            if p.poll() is None:
                os.killpg(p.pid, signal.SIGKILL)
                p.wait()
    logs = []
    for _, _, log in procs:
        log.close()
        logs.append(open(log.name).read())
    if any(rcs):
        raise AssertionError("\n".join(f"--- PE {pe} exit {rc}:\n" + text[-1500:]
                                       for pe, (rc, text) in enumerate(zip(rcs, logs))))
    reports = []
    for _, out, _ in procs:
        with open(out) as f:
            reports.append(json.load(f))
    return reports


def test_every_typed_stream_form_and_fortran_forwarder_across_three_pes(tmp_path):
    """One 3-PE run.  The 44 typed stream forms on the sets (0,0,3), (0,1,2)
    and (1,0,2): heap operands on the NULL stream; four pairs on a torch
    stream; one pair per element size on torch tensors outside the heap;
    ENOTMEMBER through a typed name with an untouched target.  The 37 Fortran
    forwarders on the same sets, by-reference integers, a NULL pWrk and an
    INTEGER pSync that stays -1: heap operands and host arrays, shmem_ and
    pshmem_ spellings alternating; nreduce = 0 and nreduce = -1 through one
    forwarder of each element size.  No failure on any PE, and the names the
    PEs executed are exactly the 44 + 2 x 37 of entry_table.ENTRIES."""
    reports = run_pes(tmp_path, et.NPES)
    assert sorted(r["pe"] for r in reports) == list(range(et.NPES))
    for r in reports:
        assert not r["fails"], f"PE {r['pe']}: {len(r['fails'])} failures: {r['fails'][:10]}"
    called = set()
    for r in reports:
        called |= set(r["called"])
    assert sorted(called) == et.all_symbols()
    # PE 2 is in every set: 3 sets x (44 + 4 + 4 stream, 2 x 37 Fortran), 1 + 15 more
    nsets = {0: 2, 1: 2, 2: 3}
    for r in reports:
        assert r["ncases"] == nsets[r["pe"]] * (44 + 4 + 4 + 2 * 37) + 1 + 15, r["ncases"]
