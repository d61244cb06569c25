"""The matrices of test_gpu_blocking_paths.py, importable (the in-process
test) and runnable as a child process (`matrix` under the settings the parent
puts in the environment, `mirrored` on a $SHMEMX_HEAP_MEMORY=mirrored heap).

One PE: a blocking shmem_<T>_<op>_to_all with PE_size 1 is a copy
(reduce-op.c:213-216), so every result is the source's bytes; each case
compares the whole target buffer, 64 canary bytes on either side included.
Prints "ok ..." or raises."""
import ctypes
import os
import sys

import numpy as np

KIB = 1024
SERVICE_MAX = 32 * KIB     # kServiceMaxBytes: up to here the resident workgroup copies
BOUNCE_MAX = 256 * KIB     # kSmallHostBytes: up to here host arrays bounce, past it the pipeline
CANARY = 64
PAIRS = (("int", "sum"), ("double", "max"))
KINDS = ("device", "pageable", "pinned")


def sizes(esz):
    return (esz, 4096, SERVICE_MAX, SERVICE_MAX + esz, BOUNCE_MAX, BOUNCE_MAX + esz)


class Buf:
    """A byte buffer of one kind with a 64-byte aligned start."""

    def __init__(self, torch, kind, nbytes):
        self.kind = kind
        if kind == "device":
            self.t = torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda")
            base = self.t.data_ptr()
        elif kind == "pinned":
            self.t = torch.zeros(nbytes + 64, dtype=torch.uint8).pin_memory()
            base = self.t.data_ptr()
        else:
            self.a = np.zeros(nbytes + 64, np.uint8)
            base = self.a.ctypes.data
        self.lead = (-base) % 64
        self.ptr = base + self.lead

    def write(self, torch, image: bytes):
        src = np.frombuffer(image, np.uint8)
        lo, hi = self.lead, self.lead + src.size
        if self.kind == "device":
            self.t[lo:hi].copy_(torch.from_numpy(src.copy()))
            torch.cuda.synchronize()
        elif self.kind == "pinned":
            self.t.numpy()[lo:hi] = src
        else:
            self.a[lo:hi] = src

    def read(self, nbytes) -> bytes:
        lo, hi = self.lead, self.lead + nbytes
        if self.kind == "device":
            return self.t[lo:hi].cpu().numpy().tobytes()
        if self.kind == "pinned":
            return self.t.numpy()[lo:hi].tobytes()
        return self.a[lo:hi].tobytes()


def run_matrix(shm, oracle, torch, pairs=PAIRS):
    """target x source over the three kinds, separate; in place and partially
    overlapping (target = source + n/2 elements) for device-device and
    host-host.  Returns (calls, calls the service workgroup must have served
    when it is on and the call is not collective)."""
    cap = CANARY + BOUNCE_MAX + 8 + BOUNCE_MAX // 2 + 8 + CANARY
    src_buf = {k: Buf(torch, k, cap) for k in KINDS}
    tgt_buf = {k: Buf(torch, k, cap) for k in KINDS}
    can = b"\xa5" * CANARY
    calls = served = 0
    for t, op in pairs:
        esz = np.dtype(oracle.NP_DTYPE[t]).itemsize
        for nbytes in sizes(esz):
            n = nbytes // esz
            h = (n // 2) * esz
            small = nbytes <= SERVICE_MAX
            for tk in KINDS:
                for sk in KINDS:
                    calls += 1
                    data = oracle.fill(t, 1, 7000 + calls, n).tobytes()
                    S, T = src_buf[sk], tgt_buf[tk]
                    S.write(torch, can + data + can)
                    T.write(torch, can + b"\xa5" * nbytes + can)
                    shm.to_all(t, op, T.ptr + CANARY, S.ptr + CANARY, n, 0, 0, 1)
                    assert shm.last_error() == 0, (t, nbytes, tk, sk, shm.last_error())
                    assert T.read(nbytes + 2 * CANARY) == can + data + can, (t, nbytes, tk, sk, "separate")
                    assert S.read(nbytes + 2 * CANARY) == can + data + can, (t, nbytes, tk, sk, "source changed")
                    served += small
            for k in KINDS:
                B = src_buf[k]
                calls += 1
                data = oracle.fill(t, 1, 7000 + calls, n).tobytes()
                B.write(torch, can + data + can)
                shm.to_all(t, op, B.ptr + CANARY, B.ptr + CANARY, n, 0, 0, 1)
                assert shm.last_error() == 0, (t, nbytes, k, "in place", shm.last_error())
                assert B.read(nbytes + 2 * CANARY) == can + data + can, (t, nbytes, k, "in place")
                served += small
                calls += 1
                data = oracle.fill(t, 1, 7000 + calls, n).tobytes()
                B.write(torch, can + data + b"\xa5" * h + can)
                shm.to_all(t, op, B.ptr + CANARY + h, B.ptr + CANARY, n, 0, 0, 1)
                assert shm.last_error() == 0, (t, nbytes, k, "overlap", shm.last_error())
                assert B.read(nbytes + h + 2 * CANARY) == can + data[:h] + data + can, (t, nbytes, k, "overlap")
                # overlapping device arrays go through the engine's temporary
                served += small and (k != "device" or h == 0)
    return calls, served


def host_view(ptr, nbytes):
    return np.frombuffer((ctypes.c_char * nbytes).from_address(ptr), np.uint8)


def run_mirrored(shm, oracle):
    """shmem_malloc'd operands of a mirrored heap, filled and read back
    through the host view: 8 B (the light path), 4 KiB and 256 KiB (the result
    settled into the view by the call) and 256 KiB + 8 (the plain path: the
    target's blocks are fetched when the host reads them); separate and in
    place, three rounds of fresh data each."""
    can = np.full(CANARY, 0xA5, np.uint8)
    calls = 0
    for t, op in PAIRS:
        esz = np.dtype(oracle.NP_DTYPE[t]).itemsize
        for nbytes in (8, 4 * KIB, BOUNCE_MAX, BOUNCE_MAX + 8):
            n = nbytes // esz
            span = nbytes + 2 * CANARY
            sp, tp = shm.malloc(span), shm.malloc(span)
            assert sp and tp
            sv, tv = host_view(sp, span), host_view(tp, span)
            for rnd in range(3):
                calls += 1
                data = np.frombuffer(oracle.fill(t, 1, 9000 + calls, n).tobytes(), np.uint8)
                sv[:] = np.concatenate([can, data, can])
                tv[:] = 0xA5
                shm.mirror_stats(reset=True)
                shm.to_all(t, op, tp + CANARY, sp + CANARY, n, 0, 0, 1)
                assert shm.last_error() == 0, (t, nbytes, rnd, shm.last_error())
                got = tv.copy()
                st = shm.mirror_stats(reset=True)
                assert got.tobytes() == np.concatenate([can, data, can]).tobytes(), (t, nbytes, rnd, "separate")
                assert sv.tobytes() == np.concatenate([can, data, can]).tobytes(), (t, nbytes, rnd, "source")
                # up to 256 KiB the call leaves the result in the view; past
                # it the host's read fetches the target's blocks
                assert (st["blocks_fetched"] == 0) == (nbytes <= BOUNCE_MAX), (t, nbytes, rnd, st)
                calls += 1
                data = np.frombuffer(oracle.fill(t, 1, 9000 + calls, n).tobytes(), np.uint8)
                sv[:] = np.concatenate([can, data, can])
                shm.to_all(t, op, sp + CANARY, sp + CANARY, n, 0, 0, 1)
                assert shm.last_error() == 0, (t, nbytes, rnd, "in place", shm.last_error())
                assert sv.tobytes() == np.concatenate([can, data, can]).tobytes(), (t, nbytes, rnd, "in place")
            del sv, tv
            shm.free(tp)
            shm.free(sp)
    return calls


if __name__ == "__main__":
    import torch

    REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(REPO, "openshmem-async_amd"))
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import oracle
    import shmem_mi355x as shm

    torch.cuda.set_device(0)
    if os.environ.get("SHMEMX_FORCE_COLLECTIVE") == "1":
        shm.init_attr(0, 1, 0, None)     # a one-rank RCCL communicator
    else:
        shm.init()
    if sys.argv[1] == "mirrored":
        assert os.environ.get("SHMEMX_HEAP_MEMORY") == "mirrored"
        print("ok", run_mirrored(shm, oracle), "calls", flush=True)
    else:
        shm.service_stats(reset=True)
        calls, _ = run_matrix(shm, oracle, torch)
        st = shm.service_stats(reset=True)
        # neither setting leaves a call to the service workgroup
        assert st["served"] == 0, st
        print("ok", calls, "calls", flush=True)
