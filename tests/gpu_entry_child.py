"""One PE of test_gpu_entry_points.py: 3 of these processes share the one GPU
on the IPC transport and call every typed stream-ordered form
(shmemx_<T>_<op>_to_all_on_stream) and every Fortran forwarder
(shmem_<F>_<op>_to_all_, in both spellings) of csrc/entry.cpp by its exported
name, through ctypes prototypes set here, on three active sets.

    SHMEM_PE=p SHMEM_NPES=3 SHMEM_BOOTSTRAP_FILE=f python gpu_entry_child.py OUT.json

Every result is compared bit for bit, on the value bytes, with the oracle's
result for the (type, op) the NAME promises (tests/entry_table.py), on inputs
where any other pair of the same element size gives other bytes
(test_entry_table.py::test_discrimination_census) and the fold order does not
matter.  The 16 bytes after the target must keep their 0xAB.  Writes
{"pe", "fails", "ncases", "called"} to OUT.json.
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
import entry_table as et  # noqa: E402
import shmem_mi355x as shm  # noqa: E402

out_path = sys.argv[1]
faulthandler.dump_traceback_later(90, repeat=True)
pe, npes = int(os.environ["SHMEM_PE"]), int(os.environ["SHMEM_NPES"])
assert npes == et.NPES
torch.cuda.set_device(0)
shm.init()
assert shm.my_pe() == pe and shm.n_pes() == npes

EINVAL, ENOTMEMBER = 1, 2
GUARD, TAIL = 0xAB, 16
N = et.NELEMS
L = shm.lib()
vp, ci = ctypes.c_void_p, ctypes.c_int
cip = ctypes.POINTER(ci)
for e in et.ENTRIES:
    for name in et.spellings(e):
        f = getattr(L, name)
        if e.kind == "stream":
            f.argtypes, f.restype = [vp, vp, ci, ci, ci, ci, vp], ci
        else:
            f.argtypes, f.restype = [vp, vp, cip, cip, cip, cip, vp, vp], None

HEAP_SRC, HEAP_TGT = shm.malloc(4096), shm.malloc(4096)
assert HEAP_SRC and HEAP_TGT, "shmem_malloc failed"
fails, called = [], set()
ncases = 0
_sources, _wants = {}, {}


def sources(t, op):
    if (t, op) not in _sources:
        _sources[t, op] = et.directed_sources(t, op, npes, N)
    return _sources[t, op]


def want_of(t, op, st):
    if (t, op, st) not in _wants:
        _wants[t, op, st] = et.reference(t, op, sources(t, op), st)[pe]
    return _wants[t, op, st]


class Operands:
    """This PE's source and a target of the array's bytes + TAIL, all 0xAB,
    in the heap, in torch device tensors outside it, or in host arrays."""

    def __init__(self, where, mine):
        self.where, self.nb = where, mine.nbytes
        fill = np.full(self.nb + TAIL, GUARD, np.uint8)
        if where == "heap":
            shm.memcpy(HEAP_SRC, mine, self.nb)
            shm.memcpy(HEAP_TGT, fill, fill.nbytes)
            self.src, self.tgt = HEAP_SRC, HEAP_TGT
        elif where == "device":
            self.s = torch.from_numpy(mine.view(np.uint8).copy()).cuda()
            self.d = torch.from_numpy(fill).cuda()
            torch.cuda.synchronize()
            self.src, self.tgt = self.s.data_ptr(), self.d.data_ptr()
        else:
            self.s, self.d = mine.copy(), fill
            self.src, self.tgt = self.s.ctypes.data, self.d.ctypes.data

    def target_bytes(self):
        torch.cuda.synchronize()
        if self.where == "heap":
            got = np.empty(self.nb + TAIL, np.uint8)
            shm.memcpy(got, HEAP_TGT, got.nbytes)
            return got
        return self.d.cpu().numpy() if self.where == "device" else self.d


def judge(tag, t, got, want):
    """got: the target's bytes + TAIL after the call; want: the oracle's
    elements, or None for a call that must leave the target untouched."""
    if want is None:
        if not (got == GUARD).all():
            fails.append(f"{tag}: {int((got != GUARD).sum())} bytes of the target changed")
        return
    bad = et.differing(t, got[:want.nbytes], want)
    if bad:
        fails.append(f"{tag}: {bad} of {len(want)} elements differ from the oracle's {t} result")
    if not (got[want.nbytes:] == GUARD).all():
        fails.append(f"{tag}: the {TAIL} bytes after the target changed")


def stream_case(e, st, where, stream=0, n=N, want_rc=0):
    """One call of a typed stream form by name.  want_rc != 0, or n <= 0: the
    target must stay untouched."""
    global ncases
    if want_rc == 0 and pe not in et.members(st):
        return
    ncases += 1
    called.add(e.symbol)
    tag = f"{e.symbol} set={st} {where}{' torch stream' if stream else ''} n={n}"
    print(tag, flush=True)
    ops = Operands(where, np.ascontiguousarray(sources(e.type, e.op)[pe]))
    rc = getattr(L, e.symbol)(ops.tgt, ops.src, n, *st, stream or None)
    err = shm.last_error()
    if rc != want_rc or err != want_rc:
        fails.append(f"{tag}: returned {rc}, last_error {err}, want {want_rc}")
    judge(tag, e.type, ops.target_bytes(), want_of(e.type, e.op, st) if want_rc == 0 and n > 0 else None)


def fortran_case(e, name, st, where, n=N, want_err=0):
    """One call of a Fortran forwarder by name: every integer by reference,
    pWrk NULL, pSync 128 INTEGERs of -1 that must stay so."""
    global ncases
    if pe not in et.members(st):
        return
    ncases += 1
    called.add(name)
    tag = f"{name} set={st} {where} n={n}"
    print(tag, flush=True)
    ops = Operands(where, np.ascontiguousarray(sources(e.type, e.op)[pe]))
    psync = np.full(128, -1, np.int32)
    getattr(L, name)(ops.tgt, ops.src, ctypes.byref(ci(n)), ctypes.byref(ci(st[0])), ctypes.byref(ci(st[1])),
                     ctypes.byref(ci(st[2])), None, psync.ctypes.data)
    err = shm.last_error()
    if err != want_err:
        fails.append(f"{tag}: last_error {err}, want {want_err}")
    judge(tag, e.type, ops.target_bytes(), want_of(e.type, e.op, st) if want_err == 0 and n > 0 else None)
    if not (psync == -1).all():
        fails.append(f"{tag}: pSync changed")


by_name = {e.symbol: e for e in et.ENTRIES}

# every typed stream form on every set: heap operands, the NULL stream
for e in et.STREAM_ENTRIES:
    for st in et.SETS:
        stream_case(e, st, "heap")
# a few on a torch stream
torch_stream = torch.cuda.Stream()
for t, op in (("double", "sum"), ("int", "xor"), ("float", "max"), ("longdouble", "prod")):
    for st in et.SETS:
        stream_case(by_name[f"shmemx_{t}_{op}_to_all_on_stream"], st, "heap", torch_stream.cuda_stream)
# one pair per element size on torch device tensors outside the heap
for t, op in (("short", "max"), ("float", "sum"), ("long", "and"), ("complexd", "prod")):
    for st in et.SETS:
        stream_case(by_name[f"shmemx_{t}_{op}_to_all_on_stream"], st, "device")
# a caller outside the set, through a typed name: PE 0 on PEs {1, 2} gets
# ENOTMEMBER and an untouched target; the members make their matching call
int_sum = by_name["shmemx_int_sum_to_all_on_stream"]
if pe == 0:
    stream_case(int_sum, (1, 0, 2), "heap", want_rc=ENOTMEMBER)
else:
    stream_case(int_sum, (1, 0, 2), "heap")

# every Fortran forwarder on every set, heap operands and host arrays; the
# spelling alternates from entry to entry and between the two placements, so
# both names of every forwarder run
for k, e in enumerate(et.FORTRAN_ENTRIES):
    for where, flip in (("heap", 0), ("host", 1)):
        for st in et.SETS:
            fortran_case(e, et.spellings(e)[(k + flip) % 2], st, where)
# nreduce = 0 (nothing to do) and nreduce = -1 (EINVAL) through one forwarder
# of each element size: the target untouched
world = et.SETS[0]
for name in ("shmem_int2_max_to_all_", "pshmem_real4_sum_to_all_", "shmem_int8_xor_to_all_",
             "pshmem_real16_min_to_all_", "shmem_comp8_prod_to_all_"):
    e = by_name[name[1:] if name.startswith("p") else name]
    fortran_case(e, name, world, "heap", n=0)
    fortran_case(e, name, world, "heap", n=-1, want_err=EINVAL)
    fortran_case(e, name, world, "host", n=-1, want_err=EINVAL)

torch.cuda.synchronize()
shm.barrier_all()
shm.finalize()
with open(out_path, "w") as f:
    json.dump({"pe": pe, "fails": fails, "ncases": ncases, "called": sorted(called)}, f)
for line in fails:
    print("FAIL", line, flush=True)
print(f"PE {pe}: {ncases} cases, {len(fails)} failures", flush=True)
# (exit 0 with the report written: the parent judges the failures it lists)
