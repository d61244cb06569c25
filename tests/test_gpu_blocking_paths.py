"""Every path of the blocking entry points' body (openshmem-async_amd/csrc/
staging.cpp) at one PE, where a call is a copy (reduce-op.c:213-216): target
and source in device, pageable and page-locked host memory, at the sizes where
the path changes (one element; 4 KiB; 32 KiB, the service workgroup's limit,
and one element past it; 256 KiB, the bounce buffers' limit, and one element
past it, the first step onto the chunked pipeline), separate, in place and
partially overlapping.  Every result is the source's bytes, the 64 bytes on
either side of the target are untouched and no call leaves an error.  The same
matrix runs in fresh child processes without the service workgroup, through
the one-rank RCCL schedules, and on a mirrored heap through its host view.
(Multi-chunk pipelines, the multi-PE exchange and the mirrored heap's block
accounting have tests of their own in test_gpu_api.py and test_gpu_ipc.py.)"""
import os
import subprocess
import sys

import pytest

import gpu_blocking_paths_child as paths

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("t,op", paths.PAIRS)
def test_blocking_paths_one_pe(cuda, shm, oracle, t, op):
    """In this process, the service workgroup on: it serves exactly the calls
    of at most 32 KiB that are plain copies (overlapping device arrays go
    through the engine's temporary)."""
    import torch
    shm.init()
    torch.cuda.synchronize()
    shm.service_stats(reset=True)
    calls, served = paths.run_matrix(shm, oracle, torch, [(t, op)])
    st = shm.service_stats(reset=True)
    assert calls == 6 * (9 + 6)
    assert st["served"] == served, (st, served)


@pytest.mark.parametrize("name,mode,env", [
    ("service_off", "matrix", {"SHMEMX_SERVICE": "0"}),
    ("one_rank_rccl", "matrix", {"SHMEMX_FORCE_COLLECTIVE": "1"}),
    ("mirrored_heap", "mirrored", {"SHMEMX_HEAP_MEMORY": "mirrored"}),
])
def test_blocking_paths_one_pe_settings(name, mode, env):
    """The launched copies in place of the service workgroup; the collective
    paths (small host arrays through the stage buffers around a one-rank RCCL
    call); shmem_malloc'd operands of a mirrored heap, written and read by the
    host through the view (8 B, 4 KiB, 256 KiB, 256 KiB + 8: the light path,
    the settled result, the plain path)."""
    r = subprocess.run(["timeout", "-k", "10", "150", sys.executable,
                        os.path.join(HERE, "gpu_blocking_paths_child.py"), mode],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=200)
    last = r.stdout.strip().splitlines()[-1:]     # (RCCL prints its banner first)
    assert r.returncode == 0 and last and last[0].startswith("ok "), (name, r.stdout[-1000:], r.stderr[-3000:])
