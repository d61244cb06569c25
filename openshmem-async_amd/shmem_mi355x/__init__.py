"""Python view of libshmem_reduce_mi355x.so (ctypes, no torch types in the ABI).

The product is the C ABI in ``include/shmem_reduce_mi355x.h``; this module is
the thin host-side mirror used by the tests and ``bench.py``.  It keeps the
reference's names and argument meaning: ``to_all("double", "sum", target,
source, nreduce, PE_start, logPE_stride, PE_size, pWrk, pSync)`` calls the C
entry point ``shmem_double_sum_to_all`` (reference src/reduce/reduce-op.c:
372-431, prototype src/shmem.h:1412-1648) with raw pointers.

Array arguments may be torch tensors (device or host), numpy arrays, or plain
integer addresses.  Loading fails loudly when the shared library has not been
built: there is no Python or CPU fallback for any reduction.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "libshmem_reduce_mi355x.so")

# SHMEMX_TYPE_* / SHMEMX_OP_* / SHMEMX_ALGO_* of the header.
TYPES = {"short": 0, "int": 1, "long": 2, "longlong": 3, "float": 4,
         "double": 5, "longdouble": 6, "complexd": 7, "complexf": 8}
OPS = {"sum": 0, "prod": 1, "and": 2, "or": 3, "xor": 4, "min": 5, "max": 6}
ALGOS = {"auto": 0, "rccl": 1, "a2a": 2, "gather": 3, "allreduce": 4, "direct": 5,
         "signal": 6, "ownslice": 7}
ERRORS = {0: "OK", 1: "EINVAL", 2: "ENOTMEMBER", 3: "ENOTSUP", 4: "ENOINIT",
          5: "ENOMEM", 6: "EDEVICE"}

# Which (type, op) pairs the reference exports (reduce-op.c:388-431).
REFERENCE_PAIRS = [(t, o) for t in TYPES for o in ("sum", "prod")] + \
    [(t, o) for t in ("short", "int", "long", "longlong") for o in ("and", "or", "xor")] + \
    [(t, o) for t in ("short", "int", "long", "longlong", "float", "double", "longdouble")
     for o in ("max", "min")]


class ShmemError(RuntimeError):
    """A shmemx_* call returned an error code."""

    def __init__(self, code: int, what: str):
        super().__init__(f"{what}: {ERRORS.get(code, code)}")
        self.code = code


class Plan(ctypes.Structure):
    _fields_ = [("algo", ctypes.c_int), ("member", ctypes.c_int),
                ("nmembers", ctypes.c_int), ("elem_size", ctypes.c_int),
                ("chunk", ctypes.c_longlong), ("main", ctypes.c_longlong),
                ("tail", ctypes.c_longlong), ("ws_bytes", ctypes.c_longlong)]


class PullPlan(ctypes.Structure):
    _fields_ = [("schedule", ctypes.c_int), ("fused", ctypes.c_int),
                ("nseg_a", ctypes.c_int), ("nseg_b", ctypes.c_int),
                ("lo", ctypes.c_longlong), ("hi", ctypes.c_longlong)]


class LaunchShape(ctypes.Structure):
    _fields_ = [("family", ctypes.c_int), ("maxin", ctypes.c_int),
                ("vectors_per_lane", ctypes.c_int), ("nt", ctypes.c_int),
                ("ld80_pipelined", ctypes.c_int), ("blocks", ctypes.c_longlong),
                ("head", ctypes.c_longlong), ("nvec", ctypes.c_longlong),
                ("tail", ctypes.c_longlong), ("scalar_trips", ctypes.c_longlong)]


_lib = None


def device_code_sha256(path: str = LIB_PATH) -> str | None:
    """sha256 of the library's gfx950 device code (its ELF .hip_fatbin
    section): what a rocprofv3 counter pass over the kernels measured.  Host
    code changes leave it alone; any kernel change moves it.  None if the
    file or the section is missing."""
    import hashlib
    import struct
    try:
        with open(path, "rb") as f:
            elf = f.read()
    except OSError:
        return None
    if elf[:4] != b"\x7fELF" or elf[4] != 2:          # ELF64 only
        return None
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)

    def sect(i):
        name, _, _, _, off, size = struct.unpack_from("<IIQQQQ", elf, shoff + i * shentsize)
        return name, off, size
    _, stroff, _ = sect(shstrndx)
    for i in range(shnum):
        name, off, size = sect(i)
        end = elf.index(b"\0", stroff + name)
        if elf[stroff + name:end] == b".hip_fatbin":
            return hashlib.sha256(elf[off:off + size]).hexdigest()
    return None


def lib() -> ctypes.CDLL:
    """Load the shared library (once).  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is not built; run `make -C openshmem-async_amd` "
            "(or __graft_entry__.build()) — there is no fallback path")
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so.7
    # and loads it by path.  Import torch first (when present) so that the
    # library's DT_NEEDED libamdhip64.so.7 / librccl.so.1 bind to the copies
    # already loaded; loading ours first would put two HIP runtimes in the
    # process and the second sees no device.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    L.shmemx_reduce_on_stream.argtypes = [i, i, vp, vp, i, i, i, i, i, vp]
    L.shmemx_reduce_on_stream.restype = i
    L.shmemx_fold_on_stream.argtypes = [i, i, vp, vp, sz, vp]
    L.shmemx_fold_on_stream.restype = i
    L.shmemx_fold_n_on_stream.argtypes = [i, i, vp, ctypes.POINTER(vp), i, sz, vp]
    L.shmemx_fold_n_on_stream.restype = i
    L.shmemx_fold_n_peers_on_stream.argtypes = [i, i, vp, ctypes.POINTER(vp), i, sz, vp]
    L.shmemx_fold_n_peers_on_stream.restype = i
    L.shmemx_fold_orders_on_stream.argtypes = [i, i, ctypes.POINTER(vp), ctypes.POINTER(vp), i, sz, vp]
    L.shmemx_fold_orders_on_stream.restype = i
    L.shmemx_gather_on_stream.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(vp),
                                          ctypes.POINTER(sz), i, vp]
    L.shmemx_gather_on_stream.restype = i
    L.shmemx_fused_loopback.argtypes = [i, i, i, i, i, i, ctypes.POINTER(vp), ctypes.POINTER(vp), sz,
                                        ctypes.POINTER(ctypes.c_uint), vp]
    L.shmemx_fused_loopback.restype = i
    L.shmemx_fused_orders_loopback.argtypes = [i, i, i, i, ctypes.POINTER(vp), ctypes.POINTER(vp),
                                               ctypes.POINTER(vp), sz, ctypes.POINTER(ctypes.c_uint), vp]
    L.shmemx_fused_orders_loopback.restype = i
    L.shmemx_order_slots_bytes.argtypes = [i, i, sz]
    L.shmemx_order_slots_bytes.restype = sz
    L.shmemx_barrier_on_stream.argtypes = [i, i, i, vp]
    L.shmemx_barrier_on_stream.restype = i
    for bits in (32, 64):
        getattr(L, f"shmemx_broadcast{bits}_on_stream").argtypes = [vp, vp, sz, i, i, i, i, vp]
        getattr(L, f"shmemx_broadcast{bits}_on_stream").restype = i
        getattr(L, f"shmemx_fcollect{bits}_on_stream").argtypes = [vp, vp, sz, i, i, i, vp]
        getattr(L, f"shmemx_fcollect{bits}_on_stream").restype = i
    ullp = ctypes.POINTER(ctypes.c_ulonglong)
    for bits in (32, 64):
        getattr(L, f"shmemx_collect{bits}_on_stream").argtypes = [vp, vp, sz, sz, i, i, i, vp]
        getattr(L, f"shmemx_collect{bits}_on_stream").restype = i
        getattr(L, f"shmemx_collect{bits}_counted_on_stream").argtypes = [vp, vp, vp, vp, sz, i, i, i, vp]
        getattr(L, f"shmemx_collect{bits}_counted_on_stream").restype = i
    L.shmemx_collect_stats.argtypes = [ullp, i, i]
    L.shmemx_collect_stats.restype = i
    L.shmemx_collect_route.argtypes = [sz, sz, i, ctypes.POINTER(i)]
    L.shmemx_collect_route.restype = i
    L.shmemx_collect_loopback.argtypes = [i, i, sz, vp, ctypes.POINTER(vp), ullp, sz, i, i, ullp,
                                          ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint), vp]
    L.shmemx_collect_loopback.restype = i
    for bits in (32, 64):
        getattr(L, f"shmemx_alltoall{bits}_on_stream").argtypes = [vp, vp, sz, i, i, i, vp]
        getattr(L, f"shmemx_alltoall{bits}_on_stream").restype = i
        getattr(L, f"shmemx_alltoallv{bits}_on_stream").argtypes = [vp, vp, vp, vp, vp, sz, sz, i, i, i, vp]
        getattr(L, f"shmemx_alltoallv{bits}_on_stream").restype = i
    L.shmemx_alltoall_stats.argtypes = [ullp, i, i]
    L.shmemx_alltoall_stats.restype = i
    L.shmemx_alltoallv_route.argtypes = [sz, sz, i, ctypes.POINTER(i)]
    L.shmemx_alltoallv_route.restype = i
    L.shmemx_alltoallv_loopback.argtypes = [i, i, sz, vp, ctypes.POINTER(vp), ullp, ullp, sz, sz, i, ullp,
                                            ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint), vp]
    L.shmemx_alltoallv_loopback.restype = i
    L.shmemx_reduce_scatter_on_stream.argtypes = [i, i, vp, vp, sz, i, i, i, vp]
    L.shmemx_reduce_scatter_on_stream.restype = i
    L.shmemx_reduce_scatter_route.argtypes = [i, sz, i, ctypes.POINTER(i)]
    L.shmemx_reduce_scatter_route.restype = i
    L.shmemx_reduce_scatter_stats.argtypes = [ullp, i, i]
    L.shmemx_reduce_scatter_stats.restype = i
    L.shmemx_reduce_scatter_loopback.argtypes = [i, i, i, i, vp, ctypes.POINTER(vp), sz, i,
                                                 ctypes.POINTER(ctypes.c_uint), vp]
    L.shmemx_reduce_scatter_loopback.restype = i
    L.shmemx_set_bcast_twophase_kb.argtypes = [ctypes.c_long]
    L.shmemx_set_bcast_twophase_kb.restype = ctypes.c_long
    L.shmemx_pull_stats.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), i, i]
    L.shmemx_pull_stats.restype = i
    L.shmemx_pull_plan.argtypes = [i, sz, sz, i, i, i, ctypes.POINTER(PullPlan)]
    L.shmemx_pull_plan.restype = i
    L.shmemx_pull_loopback.argtypes = [i, i, i, i, sz, ctypes.POINTER(vp), ctypes.POINTER(vp), sz,
                                       ctypes.POINTER(ctypes.c_uint), vp]
    L.shmemx_pull_loopback.restype = i
    L.shmemx_set_signal_ownslice.argtypes = [ctypes.c_long]
    L.shmemx_set_signal_ownslice.restype = ctypes.c_long
    L.shmemx_reduce_plan.argtypes = [i, i, i, i, i, i, i, i, i, ctypes.POINTER(Plan)]
    L.shmemx_reduce_plan.restype = i
    L.shmemx_fold_launch_shape.argtypes = [i, i, i, i, sz, ctypes.POINTER(vp), ctypes.POINTER(vp),
                                           ctypes.POINTER(LaunchShape)]
    L.shmemx_fold_launch_shape.restype = i
    L.shmemx_get_uniqueid.argtypes = [vp]
    L.shmemx_get_uniqueid.restype = i
    L.shmemx_uniqueid_size.restype = i
    L.shmemx_init_attr.argtypes = [i, i, i, vp]
    L.shmemx_init_attr.restype = i
    L.shmemx_get_stream.restype = vp
    L.shmemx_set_algo.argtypes = [i]
    L.shmemx_set_algo.restype = i
    L.shmemx_rccl_register_heap.argtypes = [i]
    L.shmemx_rccl_register_heap.restype = i
    L.shmemx_set_comms.restype = i
    L.shmemx_kernel_timing.argtypes = [i]
    L.shmemx_kernel_timing.restype = i
    L.shmemx_kernel_times.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), i,
                                      ctypes.POINTER(ctypes.c_ulonglong)]
    L.shmemx_kernel_times.restype = i
    L.shmemx_set_fused_twoshot_kb.argtypes = [ctypes.c_long]
    L.shmemx_set_fused_twoshot_kb.restype = ctypes.c_long
    L.shmemx_type_size.argtypes = [i]
    L.shmemx_type_size.restype = sz
    L.shmemx_op_valid.argtypes = [i, i]
    L.shmemx_op_on_device.argtypes = [i, i]
    L.shmemx_reduce_last_error.restype = i
    L.shmemx_reduce_error_string.argtypes = [i]
    L.shmemx_reduce_error_string.restype = ctypes.c_char_p
    for bits in (32, 64):
        for name in (f"shmem_broadcast{bits}", f"pshmem_broadcast{bits}"):
            getattr(L, name).argtypes = [vp, vp, sz, i, i, i, i, vp]
            getattr(L, name).restype = None
        for kind in ("fcollect", "collect"):
            for name in (f"shmem_{kind}{bits}", f"pshmem_{kind}{bits}"):
                getattr(L, name).argtypes = [vp, vp, sz, i, i, i, vp]
                getattr(L, name).restype = None
    L.shmemx_checksum.argtypes = [i, vp, sz, ctypes.POINTER(ctypes.c_ulonglong)]
    L.shmemx_checksum.restype = i
    L.shmemx_verify.argtypes = [i, vp, i, i, i, i, ctypes.POINTER(i)]
    L.shmemx_verify.restype = i
    L.shmem_barrier.argtypes = [i, i, i, vp]
    L.shmem_barrier.restype = None
    L.shmem_barrier_all.restype = None
    L.shmem_malloc.argtypes = [sz]
    L.shmem_malloc.restype = vp
    L.shmemx_heap_ptr.argtypes = [vp, i]
    L.shmemx_heap_ptr.restype = vp
    L.shmem_align.argtypes = [sz, sz]
    L.shmem_align.restype = vp
    L.shmem_realloc.argtypes = [vp, sz]
    L.shmem_realloc.restype = vp
    L.shmem_free.argtypes = [vp]
    L.shmem_free.restype = None
    L.shmemx_mirror_stats.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), i, i]
    L.shmemx_mirror_stats.restype = i
    L.shmemx_mirror_device_ptr.argtypes = [vp]
    L.shmemx_mirror_device_ptr.restype = vp
    L.shmemx_mirror_sync.argtypes = [vp, sz]
    L.shmemx_mirror_sync.restype = i
    L.shmemx_mirror_invalidate.argtypes = [vp, sz]
    L.shmemx_mirror_invalidate.restype = i
    L.shmemx_mirror_acquire.argtypes = [vp, sz, i]
    L.shmemx_mirror_acquire.restype = i
    L.shmemx_direct_stats.argtypes = [ctypes.POINTER(ctypes.c_double), i, i]
    L.shmemx_direct_stats.restype = i
    L.shmemx_service_stats.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), i, i]
    L.shmemx_service_stats.restype = i
    L.shmemx_service_fold_loopback.argtypes = [i, i, i, i, i, i, i, vp, vp, ctypes.POINTER(vp), sz]
    L.shmemx_service_fold_loopback.restype = i
    L.shmemx_host_register.argtypes = [vp, sz]
    L.shmemx_host_register.restype = i
    L.shmemx_host_unregister.argtypes = [vp]
    L.shmemx_host_unregister.restype = i
    L.shmemx_set_fatal_note.argtypes = [ctypes.c_char_p, i]
    L.shmemx_set_fatal_note.restype = i
    for t, o in REFERENCE_PAIRS:
        for prefix in ("shmem", "pshmem"):
            f = getattr(L, f"{prefix}_{t}_{o}_to_all")
            f.argtypes = [vp, vp, i, i, i, i, vp, vp]
            f.restype = None
    _lib = L
    return L


def addr(x) -> int | None:
    """Raw address of a torch tensor, numpy array, ctypes object or int."""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    if hasattr(x, "ctypes"):
        return x.ctypes.data
    return ctypes.addressof(x)


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise ShmemError(rc, what)


# ------------------------------------------------------------------ runtime
def init_attr(pe: int, npes: int, device: int = -1, uid: bytes | None = None) -> None:
    buf = None
    if uid is not None:
        buf = ctypes.create_string_buffer(bytes(uid), len(uid))
    _check(lib().shmemx_init_attr(pe, npes, device, buf), "shmemx_init_attr")


def get_uniqueid() -> bytes:
    n = lib().shmemx_uniqueid_size()
    buf = ctypes.create_string_buffer(n)
    _check(lib().shmemx_get_uniqueid(buf), "shmemx_get_uniqueid")
    return buf.raw


def init_from_torch_distributed(device: int = -1) -> None:
    """Bootstrap every rank of an initialised torch.distributed group (gloo is
    enough: it only carries the 128-byte RCCL id)."""
    import torch
    import torch.distributed as dist
    rank, world = dist.get_rank(), dist.get_world_size()
    if world == 1:
        init_attr(0, 1, device, None)
        return
    n = lib().shmemx_uniqueid_size()
    t = torch.zeros(n, dtype=torch.uint8)
    if rank == 0:
        t.copy_(torch.frombuffer(bytearray(get_uniqueid()), dtype=torch.uint8))
    dist.broadcast(t, src=0)
    init_attr(rank, world, device, bytes(t.numpy().tobytes()))


def init() -> None:
    lib().shmem_init()


def finalize() -> None:
    lib().shmem_finalize()


def my_pe() -> int:
    return lib().shmem_my_pe()


def n_pes() -> int:
    return lib().shmem_n_pes()


def get_stream() -> int:
    return lib().shmemx_get_stream() or 0


def set_fused_twoshot_kb(kb: int) -> int:
    """shmemx_set_fused_twoshot_kb: the largest DIRECT/SIGNAL two-shot call
    (KiB) run as one fused launch; returns the previous limit.  Collective in
    effect: every member must set the same value."""
    prev = lib().shmemx_set_fused_twoshot_kb(kb)
    if prev < 0:
        raise ShmemError(1, "shmemx_set_fused_twoshot_kb")
    return prev


def set_signal_ownslice(on: bool) -> bool:
    """shmemx_set_signal_ownslice: SIGNAL takes the six own-order pairs above
    the one-shot limit through OWNSLICE's schedule under its device barriers
    (default $SHMEMX_SIGNAL_OWNSLICE, else off); returns the previous setting.
    Collective in effect: every member must set the same value."""
    prev = lib().shmemx_set_signal_ownslice(1 if on else 0)
    if prev < 0:
        raise ShmemError(1, "shmemx_set_signal_ownslice")
    return bool(prev)


def set_algo(name: str) -> str:
    prev = lib().shmemx_set_algo(ALGOS[name])
    return {v: k for k, v in ALGOS.items()}[prev]


def last_error() -> int:
    return lib().shmemx_reduce_last_error()


# --------------------------------------------------------------- reductions
def to_all(type_name: str, op: str, target, source, nreduce: int, PE_start: int,
           logPE_stride: int, PE_size: int, pWrk=None, pSync=None) -> None:
    """shmem_<type>_<op>_to_all, blocking (reference reduce-op.c:372-386)."""
    f = getattr(lib(), f"shmem_{type_name}_{op}_to_all")
    f(addr(target), addr(source), nreduce, PE_start, logPE_stride, PE_size,
      addr(pWrk), addr(pSync))


def reduce_on_stream(type_name: str, op: str, target, source, nreduce: int,
                     PE_start: int = 0, logPE_stride: int = 0, PE_size: int = 1,
                     algo: str = "auto", stream: int = 0) -> None:
    rc = lib().shmemx_reduce_on_stream(TYPES[type_name], OPS[op], addr(target), addr(source),
                                       nreduce, PE_start, logPE_stride, PE_size,
                                       ALGOS[algo], stream or None)
    _check(rc, f"shmemx_reduce_on_stream({type_name},{op})")


def fold(type_name: str, op: str, acc, inp, nelems: int, stream: int = 0) -> None:
    """acc[i] = op(acc[i], inp[i]) on the GPU (reduce-op.c:231-235)."""
    rc = lib().shmemx_fold_on_stream(TYPES[type_name], OPS[op], addr(acc), addr(inp),
                                     nelems, stream or None)
    _check(rc, f"shmemx_fold_on_stream({type_name},{op})")


def fold_n(type_name: str, op: str, out, ins, nelems: int, stream: int = 0, peers: bool = False) -> None:
    """shmemx_fold_n_on_stream, or with peers=True shmemx_fold_n_peers_on_stream
    (every input's loads in flight before any op: the peers' HBM over xGMI)."""
    arr = (ctypes.c_void_p * len(ins))(*[addr(x) for x in ins])
    fn = lib().shmemx_fold_n_peers_on_stream if peers else lib().shmemx_fold_n_on_stream
    rc = fn(TYPES[type_name], OPS[op], addr(out), arr, len(ins), nelems, stream or None)
    _check(rc, f"shmemx_fold_n{'_peers' if peers else ''}_on_stream({type_name},{op})")


def fold_orders_on_stream(type_name: str, op: str, outs, ins, nelems: int, stream: int = 0) -> None:
    """shmemx_fold_orders_on_stream: outs[k] = ins[k] folded with the other
    inputs ascending, for every k in one launch (each member's own reference
    order; float / double / longdouble min and max).  outs[k] may be ins[k]."""
    if len(outs) != len(ins):
        raise ValueError("one output per input")
    a = (ctypes.c_void_p * len(outs))(*[addr(x) for x in outs])
    b = (ctypes.c_void_p * len(ins))(*[addr(x) for x in ins])
    rc = lib().shmemx_fold_orders_on_stream(TYPES[type_name], OPS[op], a, b, len(ins), nelems, stream or None)
    _check(rc, f"shmemx_fold_orders_on_stream({type_name},{op})")


def gather(srcs, dsts, nbytes, stream: int = 0) -> None:
    """shmemx_gather_on_stream: copy byte ranges srcs[i] -> dsts[i] in one
    launch (DIRECT's all-gather kernel)."""
    k = len(srcs)
    a = (ctypes.c_void_p * k)(*[addr(x) for x in srcs])
    b = (ctypes.c_void_p * k)(*[addr(x) for x in dsts])
    c = (ctypes.c_size_t * k)(*nbytes)
    _check(lib().shmemx_gather_on_stream(a, b, c, k, stream or None), "shmemx_gather_on_stream")


def fused_loopback(type_name: str, op: str, schedule: int, tgts, srcs, nelems: int, m: int = 0,
                   own_order: bool = False, stream: int = 0) -> int:
    """shmemx_fused_loopback: member m's fused one-shot (schedule 0) or
    two-shot (1) launch, or the unfused device barrier (2), of a
    len(tgts)-member set whose arrays are all this process's, with the peer
    handshakes looped back.  Blocking.  Returns the device barriers' error
    word (0 when the call returned OK)."""
    P = len(tgts)
    a = (ctypes.c_void_p * P)(*[addr(x) for x in tgts])
    b = (ctypes.c_void_p * len(srcs))(*[addr(x) for x in srcs])
    if len(srcs) != P:
        raise ValueError("one source per target")
    err = ctypes.c_uint(0)
    rc = lib().shmemx_fused_loopback(TYPES[type_name], OPS[op], schedule, P, m, 1 if own_order else 0,
                                     a, b, nelems, ctypes.byref(err), stream or None)
    _check(rc, f"shmemx_fused_loopback({type_name},{op},schedule={schedule},P={P},m={m}): "
               f"error word {err.value}")
    return err.value


def fused_orders_loopback(type_name: str, op: str, tgts, srcs, slots, nelems: int, m: int = 0,
                          stream: int = 0) -> int:
    """shmemx_fused_orders_loopback: member m's fused own-slice launch
    (SIGNAL's own slice: the P-order fold of slice m, the mid handshake, the
    gather of m's slot from every other owner) of a len(tgts)-member set whose
    sources, targets and slot areas (order_slots_bytes each) are all this
    process's, with the peer handshakes looped back.  Blocking.  Returns the
    device barriers' error word (0 when the call returned OK)."""
    P = len(tgts)
    if len(srcs) != P or len(slots) != P:
        raise ValueError("one source and one slot area per target")
    a = (ctypes.c_void_p * P)(*[addr(x) for x in tgts])
    b = (ctypes.c_void_p * P)(*[addr(x) for x in srcs])
    c = (ctypes.c_void_p * P)(*[addr(x) for x in slots])
    err = ctypes.c_uint(0)
    rc = lib().shmemx_fused_orders_loopback(TYPES[type_name], OPS[op], P, m, a, b, c, nelems,
                                            ctypes.byref(err), stream or None)
    _check(rc, f"shmemx_fused_orders_loopback({type_name},{op},P={P},m={m}): error word {err.value}")
    return err.value


def order_slots_bytes(type_name: str, P: int, nelems: int) -> int:
    """shmemx_order_slots_bytes: bytes of one member's P - 1 result slots for
    nelems elements over P members.  Host logic only."""
    return lib().shmemx_order_slots_bytes(TYPES[type_name], P, nelems)


@dataclass
class PlanInfo:
    algo: str
    member: int
    nmembers: int
    elem_size: int
    chunk: int
    main: int
    tail: int
    ws_bytes: int


def plan(type_name: str, op: str, nreduce: int, PE_start: int, logPE_stride: int,
         PE_size: int, pe: int, npes: int, algo: str = "auto") -> PlanInfo:
    p = Plan()
    rc = lib().shmemx_reduce_plan(TYPES[type_name], OPS[op], nreduce, PE_start, logPE_stride,
                                  PE_size, pe, npes, ALGOS[algo], ctypes.byref(p))
    _check(rc, "shmemx_reduce_plan")
    inv = {v: k for k, v in ALGOS.items()}
    return PlanInfo(inv[p.algo], p.member, p.nmembers, p.elem_size, p.chunk, p.main,
                    p.tail, p.ws_bytes)


FOLD_ROUTES = {"plain": 0, "peers": 1, "orders": 2}
FOLD_FAMILIES = {-1: None, 0: "fold2", 1: "fold_n", 2: "peers", 3: "orders", 4: "copy"}


@dataclass
class LaunchShapeInfo:
    family: str | None      # None: nothing is launched (nelems == 0)
    maxin: int
    vectors_per_lane: int
    nt: int
    blocks: int
    head: int
    nvec: int
    tail: int
    scalar_trips: int
    ld80_pipelined: bool


def fold_launch_shape(type_name: str, op: str, route: str, outs, ins, nelems: int) -> LaunchShapeInfo:
    """shmemx_fold_launch_shape: the kernel instance and grid that
    fold / fold_n (route "plain"; one input: the copy), fold_n(peers=True)
    ("peers") or fold_orders_on_stream ("orders") would launch for these
    arrays, which may be plain integer addresses: only their values mod 16
    are looked at.  outs: the output, or the list of "orders" outputs.
    Host logic only; no GPU needed."""
    if not isinstance(outs, (list, tuple)):
        outs = [outs]
    a = (ctypes.c_void_p * max(len(outs), 1))(*[addr(x) for x in outs])
    b = (ctypes.c_void_p * max(len(ins), 1))(*[addr(x) for x in ins])
    s = LaunchShape()
    rc = lib().shmemx_fold_launch_shape(TYPES[type_name], OPS[op], FOLD_ROUTES[route], len(ins), nelems,
                                        a, b, ctypes.byref(s))
    _check(rc, f"shmemx_fold_launch_shape({type_name},{op},{route},nins={len(ins)})")
    return LaunchShapeInfo(FOLD_FAMILIES[s.family], s.maxin, s.vectors_per_lane, s.nt, s.blocks, s.head,
                           s.nvec, s.tail, s.scalar_trips, bool(s.ld80_pipelined))


def rccl_register_heap(on: bool) -> None:
    """shmemx_rccl_register_heap: the heap segment (de)registered with RCCL."""
    _check(lib().shmemx_rccl_register_heap(1 if on else 0), "shmemx_rccl_register_heap")


def set_comms() -> int:
    """shmemx_set_comms: members-only RCCL communicators held for partial sets."""
    return lib().shmemx_set_comms()


KERNEL_KINDS = ("fold", "copy", "peers_fold", "gather", "orders_fold")


def kernel_timing(on: bool) -> None:
    """shmemx_kernel_timing: time every fold-family launch from here on
    (start/stop events of the dispatch itself, kernel time only)."""
    lib().shmemx_kernel_timing(1 if on else 0)


def kernel_times(max_launches: int = 4096):
    """shmemx_kernel_times: [(kind, microseconds)] of the launches timed since
    the last read, in launch order (waits for them), and the untimed count."""
    us = (ctypes.c_double * max_launches)()
    kind = (ctypes.c_int * max_launches)()
    dropped = ctypes.c_ulonglong(0)
    n = lib().shmemx_kernel_times(us, kind, max_launches, ctypes.byref(dropped))
    return [(KERNEL_KINDS[kind[i]], us[i]) for i in range(n)], dropped.value


def type_size(type_name: str) -> int:
    return lib().shmemx_type_size(TYPES[type_name])


def op_on_device(type_name: str, op: str) -> bool:
    return bool(lib().shmemx_op_on_device(TYPES[type_name], OPS[op]))


# ------------------------------------------- neighbouring collectives, heap
def barrier(PE_start: int, logPE_stride: int, PE_size: int, pSync=None) -> None:
    lib().shmem_barrier(PE_start, logPE_stride, PE_size, addr(pSync))


def barrier_all() -> None:
    lib().shmem_barrier_all()


def broadcast(bits: int, target, source, nelems: int, PE_root: int, PE_start: int,
              logPE_stride: int, PE_size: int, pSync=None) -> None:
    """shmem_broadcast{32,64} (reference broadcast/broadcast.c)."""
    getattr(lib(), f"shmem_broadcast{bits}")(addr(target), addr(source), nelems, PE_root,
                                             PE_start, logPE_stride, PE_size, addr(pSync))


def fcollect(bits: int, target, source, nelems: int, PE_start: int, logPE_stride: int,
             PE_size: int, pSync=None) -> None:
    getattr(lib(), f"shmem_fcollect{bits}")(addr(target), addr(source), nelems, PE_start,
                                            logPE_stride, PE_size, addr(pSync))


def collect(bits: int, target, source, nelems: int, PE_start: int, logPE_stride: int,
            PE_size: int, pSync=None) -> None:
    getattr(lib(), f"shmem_collect{bits}")(addr(target), addr(source), nelems, PE_start,
                                           logPE_stride, PE_size, addr(pSync))


def barrier_on_stream(PE_start: int, logPE_stride: int, PE_size: int, stream: int = 0) -> None:
    """shmemx_barrier_on_stream: the set's barrier as stream work (a system
    fence and the device barrier), capturable."""
    _check(lib().shmemx_barrier_on_stream(PE_start, logPE_stride, PE_size, stream or None),
           "shmemx_barrier_on_stream")


def broadcast_on_stream(bits: int, target, source, nelems: int, PE_root: int, PE_start: int,
                        logPE_stride: int, PE_size: int, stream: int = 0) -> None:
    """shmemx_broadcast{32,64}_on_stream: heap operands only; the root's
    target is never written."""
    rc = getattr(lib(), f"shmemx_broadcast{bits}_on_stream")(addr(target), addr(source), nelems, PE_root,
                                                             PE_start, logPE_stride, PE_size, stream or None)
    _check(rc, f"shmemx_broadcast{bits}_on_stream")


def fcollect_on_stream(bits: int, target, source, nelems: int, PE_start: int, logPE_stride: int,
                       PE_size: int, stream: int = 0) -> None:
    """shmemx_fcollect{32,64}_on_stream: heap operands only."""
    rc = getattr(lib(), f"shmemx_fcollect{bits}_on_stream")(addr(target), addr(source), nelems, PE_start,
                                                            logPE_stride, PE_size, stream or None)
    _check(rc, f"shmemx_fcollect{bits}_on_stream")


def set_bcast_twophase_kb(kb: int) -> int:
    """shmemx_set_bcast_twophase_kb: the largest stream-ordered broadcast
    (KiB) that stays one phase; returns the previous limit.  Collective in
    effect: every member must set the same value."""
    prev = lib().shmemx_set_bcast_twophase_kb(kb)
    if prev < 0:
        raise ShmemError(1, "shmemx_set_bcast_twophase_kb")
    return prev


PULL_STATS = ("barriers", "broadcasts", "fcollects", "fused_calls", "twophase_broadcasts")


def pull_stats(reset: bool = False) -> dict:
    """shmemx_pull_stats: the stream-ordered barriers, broadcasts and
    fcollects since the last reset, those of the latter two that ran as one
    fused launch, and the two-phase broadcasts."""
    buf = (ctypes.c_ulonglong * len(PULL_STATS))()
    k = lib().shmemx_pull_stats(buf, len(buf), 1 if reset else 0)
    return {name: buf[i] for i, name in enumerate(PULL_STATS[:max(0, k)])}


def collect_on_stream(bits: int, target, source, nelems: int, capacity: int, PE_start: int, logPE_stride: int,
                      PE_size: int, stream: int = 0) -> None:
    """shmemx_collect{32,64}_on_stream: heap operands only; capacity is the
    elements the target holds, the same on every member."""
    rc = getattr(lib(), f"shmemx_collect{bits}_on_stream")(addr(target), addr(source), nelems, capacity, PE_start,
                                                           logPE_stride, PE_size, stream or None)
    _check(rc, f"shmemx_collect{bits}_on_stream")


def collect_counted_on_stream(bits: int, target, source, nelems_dev, where_dev, capacity: int, PE_start: int,
                              logPE_stride: int, PE_size: int, stream: int = 0) -> None:
    """shmemx_collect{32,64}_counted_on_stream: the count is the 8-byte word
    at nelems_dev when the call executes; where_dev (or None) receives this
    member's offset and the total."""
    rc = getattr(lib(), f"shmemx_collect{bits}_counted_on_stream")(
        addr(target), addr(source), addr(nelems_dev), addr(where_dev), capacity, PE_start, logPE_stride, PE_size,
        stream or None)
    _check(rc, f"shmemx_collect{bits}_counted_on_stream")


COLLECT_STATS = ("collects", "fused_calls", "overflows")
ALL_ONES = (1 << 64) - 1


def collect_stats(reset: bool = False) -> dict:
    """shmemx_collect_stats: the stream-ordered collects since the last
    reset, those that ran as one fused launch, and the overflows the device
    saw (synchronise the stream first)."""
    buf = (ctypes.c_ulonglong * len(COLLECT_STATS))()
    k = lib().shmemx_collect_stats(buf, len(buf), 1 if reset else 0)
    return {name: buf[i] for i, name in enumerate(COLLECT_STATS[:max(0, k)])}


def collect_route(esize: int, capacity: int, P: int) -> bool:
    """shmemx_collect_route: would a collect of this capacity run as one
    fused launch under the current limit?  Host logic only."""
    fused = ctypes.c_int(-1)
    _check(lib().shmemx_collect_route(esize, capacity, P, ctypes.byref(fused)),
           f"shmemx_collect_route(esize={esize},capacity={capacity},P={P})")
    return bool(fused.value)


def collect_loopback(tgt, srcs, counts, capacity: int, esize: int, m: int = 0, fused: bool = True,
                     counted: bool = False, stream: int = 0):
    """shmemx_collect_loopback: member m's collect launches of a
    len(srcs)-member set whose arrays are all this process's, the peers'
    counts given, the handshakes looped back.  Blocking.  Returns (where[0],
    where[1], overflows counted, the device barriers' error word)."""
    P = len(srcs)
    if len(counts) != P:
        raise ValueError("one count per source")
    a = (ctypes.c_void_p * P)(*[addr(x) for x in srcs])
    c = (ctypes.c_ulonglong * P)(*counts)
    where = (ctypes.c_ulonglong * 2)(0, 0)
    over, err = ctypes.c_uint(0), ctypes.c_uint(0)
    rc = lib().shmemx_collect_loopback(P, m, esize, addr(tgt), a, c, capacity, 1 if fused else 0,
                                       1 if counted else 0, where, ctypes.byref(over), ctypes.byref(err),
                                       stream or None)
    _check(rc, f"shmemx_collect_loopback(P={P},m={m},fused={fused},counted={counted}): error word {err.value}")
    return where[0], where[1], over.value, err.value


def alltoall_on_stream(bits: int, target, source, nelems: int, PE_start: int, logPE_stride: int, PE_size: int,
                       stream: int = 0) -> None:
    """shmemx_alltoall{32,64}_on_stream: heap operands only, PE_size * nelems
    elements each; my block j goes to member j's block of my index."""
    rc = getattr(lib(), f"shmemx_alltoall{bits}_on_stream")(addr(target), addr(source), nelems, PE_start,
                                                            logPE_stride, PE_size, stream or None)
    _check(rc, f"shmemx_alltoall{bits}_on_stream")


def alltoallv_on_stream(bits: int, target, source, send_counts, send_offsets, where_dev, capacity: int,
                        src_capacity: int, PE_start: int, logPE_stride: int, PE_size: int, stream: int = 0) -> None:
    """shmemx_alltoallv{32,64}_on_stream: send_counts / send_offsets are
    8-byte-word heap tables the peers read when the call executes; where_dev
    (or None) receives the PE_size block offsets and the total received."""
    rc = getattr(lib(), f"shmemx_alltoallv{bits}_on_stream")(
        addr(target), addr(source), addr(send_counts), addr(send_offsets), addr(where_dev), capacity, src_capacity,
        PE_start, logPE_stride, PE_size, stream or None)
    _check(rc, f"shmemx_alltoallv{bits}_on_stream")


ALLTOALL_STATS = ("alltoalls", "alltoallvs", "fused_calls", "overflows")


def alltoall_stats(reset: bool = False) -> dict:
    """shmemx_alltoall_stats: the stream-ordered alltoalls and alltoallvs
    since the last reset, those of them that ran as one fused launch, and the
    overflows the device saw (synchronise the stream first)."""
    buf = (ctypes.c_ulonglong * len(ALLTOALL_STATS))()
    k = lib().shmemx_alltoall_stats(buf, len(buf), 1 if reset else 0)
    return {name: buf[i] for i, name in enumerate(ALLTOALL_STATS[:max(0, k)])}


def alltoallv_route(esize: int, capacity: int, P: int) -> bool:
    """shmemx_alltoallv_route: would an alltoallv of this capacity run as one
    fused launch under the current limit?  Host logic only."""
    fused = ctypes.c_int(-1)
    _check(lib().shmemx_alltoallv_route(esize, capacity, P, ctypes.byref(fused)),
           f"shmemx_alltoallv_route(esize={esize},capacity={capacity},P={P})")
    return bool(fused.value)


def alltoallv_loopback(tgt, srcs, counts, offsets, capacity: int, src_capacity: int, esize: int, m: int = 0,
                       fused: bool = True, stream: int = 0):
    """shmemx_alltoallv_loopback: member m's alltoallv launches of a
    len(srcs)-member set whose arrays are all this process's.  counts and
    offsets are P x P nested lists, row i what member i sends; both None runs
    the fixed alltoall of capacity // P elements per pair.  Blocking.  Returns
    (the P + 1 where words, overflows counted, the device barriers' error
    word)."""
    P = len(srcs)
    a = (ctypes.c_void_p * P)(*[addr(x) for x in srcs])
    c = o = None
    if counts is not None or offsets is not None:
        if counts is None or offsets is None or len(counts) != P or len(offsets) != P or \
                any(len(r) != P for r in counts) or any(len(r) != P for r in offsets):
            raise ValueError("counts and offsets are P x P")
        c = (ctypes.c_ulonglong * (P * P))(*[v for r in counts for v in r])
        o = (ctypes.c_ulonglong * (P * P))(*[v for r in offsets for v in r])
    where = (ctypes.c_ulonglong * (P + 1))(*([0] * (P + 1)))
    over, err = ctypes.c_uint(0), ctypes.c_uint(0)
    rc = lib().shmemx_alltoallv_loopback(P, m, esize, addr(tgt), a, c, o, capacity, src_capacity,
                                         1 if fused else 0, where, ctypes.byref(over), ctypes.byref(err),
                                         stream or None)
    _check(rc, f"shmemx_alltoallv_loopback(P={P},m={m},fused={fused}): error word {err.value}")
    return list(where), over.value, err.value


def reduce_scatter_on_stream(type_name: str, op: str, target, source, nelems: int, PE_start: int,
                             logPE_stride: int, PE_size: int, stream: int = 0) -> None:
    """shmemx_reduce_scatter_on_stream: heap operands only; the source holds
    PE_size * nelems elements, the target nelems: the set-order fold of this
    member's block of every member's source."""
    rc = lib().shmemx_reduce_scatter_on_stream(TYPES[type_name], OPS[op], addr(target), addr(source), nelems,
                                               PE_start, logPE_stride, PE_size, stream or None)
    _check(rc, f"shmemx_reduce_scatter_on_stream({type_name},{op})")


def reduce_scatter_route(type_name: str, nelems: int, P: int) -> bool:
    """shmemx_reduce_scatter_route: would a reduce-scatter of nelems elements
    per member run as one fused launch under the current limit?  Host logic
    only."""
    fused = ctypes.c_int(-1)
    _check(lib().shmemx_reduce_scatter_route(TYPES[type_name], nelems, P, ctypes.byref(fused)),
           f"shmemx_reduce_scatter_route({type_name},nelems={nelems},P={P})")
    return bool(fused.value)


REDUCE_SCATTER_STATS = ("calls", "fused_calls")


def reduce_scatter_stats(reset: bool = False) -> dict:
    """shmemx_reduce_scatter_stats: the stream-ordered reduce-scatters since
    the last reset and those that ran as one fused launch."""
    buf = (ctypes.c_ulonglong * len(REDUCE_SCATTER_STATS))()
    k = lib().shmemx_reduce_scatter_stats(buf, len(buf), 1 if reset else 0)
    return {name: buf[i] for i, name in enumerate(REDUCE_SCATTER_STATS[:max(0, k)])}


def reduce_scatter_loopback(type_name: str, op: str, tgt, srcs, nelems: int, m: int = 0, fused: bool = True,
                            stream: int = 0) -> int:
    """shmemx_reduce_scatter_loopback: member m's reduce-scatter launches of a
    len(srcs)-member set whose arrays (each source len(srcs) * nelems
    elements) are all this process's, the handshakes looped back.  Blocking.
    Returns the device barriers' error word (0 when the call returned OK)."""
    P = len(srcs)
    a = (ctypes.c_void_p * P)(*[addr(x) for x in srcs])
    err = ctypes.c_uint(0)
    rc = lib().shmemx_reduce_scatter_loopback(TYPES[type_name], OPS[op], P, m, addr(tgt), a, nelems,
                                              1 if fused else 0, ctypes.byref(err), stream or None)
    _check(rc, f"shmemx_reduce_scatter_loopback({type_name},{op},P={P},m={m},fused={fused}): "
               f"error word {err.value}")
    return err.value


PULL_KINDS ={"fcollect": 0, "broadcast": 1}


@dataclass
class PullPlanInfo:
    schedule: int       # 0 nothing launched, 1 one phase, 2 two phases
    fused: bool
    nseg_a: int
    nseg_b: int
    lo: int
    hi: int


def pull_plan(kind: str, esize: int, nelems: int, P: int, m: int, root: int = 0) -> PullPlanInfo:
    """shmemx_pull_plan: how member m's stream-ordered fcollect / broadcast
    would run under the current limits.  Host logic only."""
    p = PullPlan()
    _check(lib().shmemx_pull_plan(PULL_KINDS[kind], esize, nelems, P, m, root, ctypes.byref(p)),
           f"shmemx_pull_plan({kind},esize={esize},P={P},m={m},root={root})")
    return PullPlanInfo(p.schedule, bool(p.fused), p.nseg_a, p.nseg_b, p.lo, p.hi)


def pull_loopback(schedule: int, tgts, srcs, nelems: int, esize: int, m: int = 0, root: int = 0,
                  stream: int = 0) -> int:
    """shmemx_pull_loopback: member m's fused pull launch (schedule 0
    fcollect, 1 one-phase broadcast, 2 two-phase broadcast) of a
    len(tgts)-member set whose arrays are all this process's, with the peer
    handshakes looped back.  Blocking.  Returns the device barriers' error
    word (0 when the call returned OK)."""
    P = len(tgts)
    if len(srcs) != P:
        raise ValueError("one source per target")
    a = (ctypes.c_void_p * P)(*[addr(x) for x in tgts])
    b = (ctypes.c_void_p * P)(*[addr(x) for x in srcs])
    err = ctypes.c_uint(0)
    rc = lib().shmemx_pull_loopback(schedule, P, m, root, esize, a, b, nelems, ctypes.byref(err), stream or None)
    _check(rc, f"shmemx_pull_loopback(schedule={schedule},P={P},m={m},root={root}): error word {err.value}")
    return err.value


def heap_ptr(address: int, pe: int) -> int:
    """shmemx_heap_ptr: PE `pe`'s copy of a symmetric-heap address, as mapped
    on this PE (0 if not mapped)."""
    return lib().shmemx_heap_ptr(address, pe) or 0


DIRECT_PHASES = ("entry_wait_us", "entry_barrier_us", "fold_us", "fold_barrier_us",
                 "gather_us", "exit_barrier_us")


FENCE_STATS = ("fences_host", "fence_refills_host", "fences_device", "fences_device_incomplete")
# by kind, not by index: the two SIGNAL own-slice counters were appended to
# shmemx_direct_stats after OWNSLICE's (DIRECT_STAT_INDEX below)
DIRECT_COUNTS = ("fused_calls", "fused_twoshot_calls", "signal_ownslice_calls",
                 "signal_ownslice_fused_calls", "ownslice_calls")
_STATS_IN_ORDER = DIRECT_PHASES + FENCE_STATS + ("fused_calls", "fused_twoshot_calls", "ownslice_calls",
                                                 "signal_ownslice_calls", "signal_ownslice_fused_calls")
# name -> index in shmemx_direct_stats' out[]
DIRECT_STAT_INDEX = {"calls": 0, **{name: k + 1 for k, name in enumerate(_STATS_IN_ORDER)}}


def direct_stats(reset: bool = True) -> dict:
    """shmemx_direct_stats: DIRECT calls since the last reset, the host-side
    microseconds summed over them per phase, and the system-fence coverage
    counters (fences checked on the host / refilled because a fence missed an
    XCD; fences checked by the SIGNAL barrier / found incomplete), and the
    one-shot / two-shot calls that ran as one fused launch, the calls that
    ran OWNSLICE's two-phase schedule, and the SIGNAL calls that ran its own
    slice / ran it with every chunk as one fused launch."""
    buf = (ctypes.c_double * len(DIRECT_STAT_INDEX))()
    k = lib().shmemx_direct_stats(buf, len(buf), 1 if reset else 0)
    return {name: buf[i] for name, i in DIRECT_STAT_INDEX.items() if i < k}


SERVICE_STATS = ("served", "launches", "null_stream_busy", "library_stream_busy", "ns_before_post",
                 "ns_round_trip", "folds")


def service_stats(reset: bool = False) -> dict:
    """shmemx_service_stats: small one-member blocking calls the resident
    service workgroup served, its launches, and the calls that found the
    legacy default stream / the library's stream busy and waited for it
    first."""
    buf = (ctypes.c_ulonglong * len(SERVICE_STATS))()
    k = lib().shmemx_service_stats(buf, len(buf), 1 if reset else 0)
    return {name: buf[i] for i, name in enumerate(SERVICE_STATS[:max(0, k)])}


def service_fold_loopback(type_name: str, op: str, dst, srcs, nelems: int, PE_start: int = 0,
                          logPE_stride: int = 0, me: int | None = None, own_order: bool = False,
                          dst2=None) -> None:
    """shmemx_service_fold_loopback: one fold request of the small-call
    exchange served by the resident workgroup in this process.  srcs: one host
    array (numpy, or an address) per member of (PE_start, logPE_stride,
    len(srcs)); me: the member the caller plays (default PE_start); dst, dst2:
    device-accessible targets.  Blocking."""
    P = len(srcs)
    keep = [s for s in srcs]   # the arrays stay alive over the call
    a = (ctypes.c_void_p * max(P, 1))(*[addr(x) for x in keep])
    rc = lib().shmemx_service_fold_loopback(TYPES[type_name], OPS[op], 1 if own_order else 0, PE_start,
                                            logPE_stride, P, PE_start if me is None else me,
                                            addr(dst), addr(dst2), a, nelems)
    _check(rc, f"shmemx_service_fold_loopback({type_name},{op},set=({PE_start},{logPE_stride},{P}),me={me})")


MIRROR_STATS = ("write_faults", "read_faults", "blocks_flushed", "blocks_fetched",
                "blocks_device_newer", "fault_waits", "blocks_settled")


def mirror_stats(reset: bool = False) -> dict:
    """shmemx_mirror_stats: the mirrored heap's fault and block counters."""
    buf = (ctypes.c_ulonglong * len(MIRROR_STATS))()
    k = lib().shmemx_mirror_stats(buf, len(buf), 1 if reset else 0)
    return {name: buf[i] for i, name in enumerate(MIRROR_STATS[:k])}


def mirror_device_ptr(address: int) -> int:
    return lib().shmemx_mirror_device_ptr(address) or 0


def mirror_sync(address: int, nbytes: int) -> None:
    _check(lib().shmemx_mirror_sync(address, nbytes), "shmemx_mirror_sync")


def mirror_invalidate(address: int, nbytes: int) -> None:
    _check(lib().shmemx_mirror_invalidate(address, nbytes), "shmemx_mirror_invalidate")


def mirror_acquire(address: int, nbytes: int, for_write: bool = False) -> None:
    """shmemx_mirror_acquire: open [address, address + nbytes) of the view to
    code that cannot take the page fault (system calls)."""
    _check(lib().shmemx_mirror_acquire(address, nbytes, 1 if for_write else 0),
           "shmemx_mirror_acquire")


def host_register(buf, nbytes: int) -> None:
    """shmemx_host_register: page-lock a host range (the reference's heap
    segment) so host operands inside it take the pinned pipeline."""
    _check(lib().shmemx_host_register(addr(buf), nbytes), "shmemx_host_register")


def host_unregister(buf) -> None:
    _check(lib().shmemx_host_unregister(addr(buf)), "shmemx_host_unregister")


def set_fatal_note(text: str | None, exit_code: int = 1) -> None:
    """shmemx_set_fatal_note: text written to stdout if the process dies on
    SIGABRT/SIGSEGV/SIGBUS/SIGFPE/SIGILL/SIGTERM, then _exit(exit_code) for
    SIGTERM and _exit(128 + signal) for the others; None uninstalls."""
    raw = None if text is None else text.encode()
    _check(lib().shmemx_set_fatal_note(raw, exit_code), "shmemx_set_fatal_note")


_hip = None


def memcpy(dst, src, nbytes: int) -> None:
    """hipMemcpy(kind = default) between any host/device addresses (heap
    pointers are plain device addresses, not tensors), complete on return.
    A device-to-device hipMemcpy returns before the copy has run (it is only
    ordered on the legacy default stream), so a reduction enqueued right
    after it on a non-blocking stream (torch.cuda.Stream, the stream-ordered
    API) could read the old bytes: the device is synchronised here."""
    global _hip
    if _hip is None:
        lib()   # torch's HIP runtime first
        _hip = ctypes.CDLL("libamdhip64.so.7")
        _hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        _hip.hipMemcpy.restype = ctypes.c_int
        _hip.hipDeviceSynchronize.restype = ctypes.c_int
    rc = _hip.hipMemcpy(addr(dst), addr(src), nbytes, 4)   # hipMemcpyDefault
    if rc == 0:
        rc = _hip.hipDeviceSynchronize()
    if rc != 0:
        raise ShmemError(6, f"hipMemcpy failed ({rc})")


def malloc(nbytes: int) -> int:
    """shmem_malloc: symmetric HBM allocation (device address, 0 on failure)."""
    return lib().shmem_malloc(nbytes) or 0


def align(alignment: int, nbytes: int) -> int:
    return lib().shmem_align(alignment, nbytes) or 0


def realloc(ptr: int, nbytes: int) -> int:
    return lib().shmem_realloc(ptr or None, nbytes) or 0


def free(ptr: int) -> None:
    lib().shmem_free(ptr or None)


def checksum(type_name: str, ptr, nelems: int) -> int:
    """shmemx_checksum: position-aware 64-bit checksum (gfx950 kernel)."""
    out = ctypes.c_ulonglong(0)
    _check(lib().shmemx_checksum(TYPES[type_name], addr(ptr), nelems, ctypes.byref(out)),
           "shmemx_checksum")
    return out.value


def verify(type_name: str, target, nreduce: int, PE_start: int, logPE_stride: int,
           PE_size: int) -> bool:
    """shmemx_verify: do all members of the set hold the same target?"""
    eq = ctypes.c_int(0)
    _check(lib().shmemx_verify(TYPES[type_name], addr(target), nreduce, PE_start, logPE_stride,
                               PE_size, ctypes.byref(eq)), "shmemx_verify")
    return bool(eq.value)
