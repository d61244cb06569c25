"""CPU tests of the C ABI library: it loads, exports every symbol the header
declares (pshmem_* strong, shmem_* weak aliases, reduce-op.c:275-364), the
header compiles and links from C, and the host-side planning logic (which
algorithm, which shards) is right.  No GPU calls here."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "shmem_reduce_mi355x.h")
LIBDIR = os.path.join(REPO, "openshmem-async_amd")
LIB = os.path.join(LIBDIR, "libshmem_reduce_mi355x.so")


def declared_functions():
    pre = subprocess.run(["gcc", "-E", "-P", "-x", "c", HEADER], check=True,
                         capture_output=True, text=True).stdout
    return sorted(set(re.findall(r"\b(p?shmemx?_[A-Za-z0-9_]+)\s*\(", pre)))


def exported():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True,
                         capture_output=True, text=True).stdout
    syms = {}
    for line in out.splitlines():
        parts = line.split()
        if len(parts) == 3:
            syms[parts[2]] = (parts[0], parts[1])
    return syms


def test_library_loads(shm):
    assert shm.lib() is not None


def test_every_declared_symbol_is_exported():
    decl = declared_functions()
    assert len(decl) >= 88 + 8
    syms = exported()
    missing = [d for d in decl if d not in syms]
    assert not missing, missing


def test_pshmem_strong_shmem_weak_same_address(shm):
    syms = exported()
    pairs = [f"{t}_{o}_to_all" for t, o in shm.REFERENCE_PAIRS] + ["init", "finalize", "my_pe", "n_pes"]
    assert len(shm.REFERENCE_PAIRS) == 44
    for p in pairs:
        addr_s, kind_s = syms["shmem_" + p]
        addr_p, kind_p = syms["pshmem_" + p]
        assert kind_p == "T" and kind_s == "W", p
        assert addr_s == addr_p, p


def test_reference_pair_set_matches_reduce_op_c(shm, oracle):
    """The 44 (type, op) pairs are exactly those reduce-op.c:388-431 defines."""
    for t in shm.TYPES:
        for o in shm.OPS:
            assert ((t, o) in shm.REFERENCE_PAIRS) == oracle.op_valid(t, o), (t, o)
            assert bool(shm.lib().shmemx_op_valid(shm.TYPES[t], shm.OPS[o])) == oracle.op_valid(t, o)


def test_enum_numbering_matches_oracle(shm, oracle):
    assert shm.TYPES == oracle.TYPES and shm.OPS == oracle.OPS
    for t in shm.TYPES:
        assert shm.type_size(t) == oracle.lib().oracle_type_size(oracle.TYPES[t])


def test_header_compiles_and_links_from_c(tmp_path):
    """A C99 caller written like the reference's users (ISx, isx.c:617)."""
    src = tmp_path / "caller.c"
    src.write_text(r'''
#include <complex.h>
#include "shmem_reduce_mi355x.h"
static long pSync[SHMEM_REDUCE_SYNC_SIZE];
static long long llWrk[SHMEM_REDUCE_MIN_WRKDATA_SIZE];
int main(void) {
    static long long total, mine = 3;
    double complex z = 1.0, w;
    for (int i = 0; i < SHMEM_REDUCE_SYNC_SIZE; i++) pSync[i] = SHMEM_SYNC_VALUE;
    shmem_init();
    shmem_longlong_sum_to_all(&total, &mine, 1, 0, 0, shmem_n_pes(), llWrk, pSync);
    shmem_complexd_prod_to_all(&w, &z, 1, 0, 0, 1, NULL, pSync);
    pshmem_double_max_to_all(NULL, NULL, 0, 0, 0, 1, NULL, pSync);
    shmem_finalize();
    return (int)(total != 3 * shmem_n_pes());
}
''')
    exe = tmp_path / "caller"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src),
                    "-L", LIBDIR, "-lshmem_reduce_mi355x", f"-Wl,-rpath,{LIBDIR}", "-o", str(exe)],
                   check=True)
    assert exe.exists()


REF_API = os.path.join(REPO, "oracle", "_ref")


def test_reference_header_and_ours_agree(tmp_path):
    """The drop-in boundary against the reference's OWN public headers
    (src/shmem.h, src/pshmem.h; they build standalone), as the precompiled
    headers build() makes of them where the reference is present
    (oracle/build_ref.sh -> oracle/_ref/shmem.h.gch and ref_api.h.gch =
    oracle/ref_api.h, both headers; gcc takes <name>.gch for #include <name>
    when it is the first include and the flags match, -Winvalid-pch says why
    if not):
      * one translation unit includes the reference's shmem.h and pshmem.h and
        then ours: C allows a function to be redeclared only with a compatible
        type, so any of our prototypes that differs from the reference's (the
        44 reductions at shmem.h:1412-1648, their pshmem names, and the
        runtime/collective entry points both headers declare) is a compile
        error under -Werror;
      * the reduction constants our header gives a program (shmem.h:1400-1410)
        equal the reference header's values;
      * a program compiled against the reference's shmem.h alone (no header
        of ours: a reference user's source as it stands) links against
        libshmem_reduce_mi355x.so with every symbol resolved."""
    if not (os.path.exists(os.path.join(REF_API, "shmem.h.gch"))
            and os.path.exists(os.path.join(REF_API, "ref_api.h.gch"))):
        pytest.skip("oracle/_ref holds no reference headers (the reference is not on this host)")
    both = tmp_path / "both.c"
    both.write_text('#include <ref_api.h>\n'
                    '#include "shmem_reduce_mi355x.h"\nint main(void){return 0;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-Winvalid-pch", "-I", REF_API,
                    "-I", os.path.dirname(HEADER), "-c", str(both), "-o", str(tmp_path / "both.o")],
                   check=True)
    names = ["SHMEM_REDUCE_SYNC_SIZE", "SHMEM_REDUCE_MIN_WRKDATA_SIZE", "SHMEM_SYNC_VALUE",
             "_SHMEM_REDUCE_SYNC_SIZE", "_SHMEM_REDUCE_MIN_WRKDATA_SIZE", "_SHMEM_SYNC_VALUE"]
    prog = ("#include HDR\n#include <stdio.h>\nint main(void){\n" +
            "".join(f'#ifdef {n}\n printf("{n} %ld\\n", (long)({n}));\n#endif\n' for n in names) +
            "return 0;}\n")
    src = tmp_path / "consts.c"
    src.write_text(prog)
    vals = {}
    for tag, hdr, inc in (("ref", "<shmem.h>", REF_API),
                          ("ours", '"shmem_reduce_mi355x.h"', os.path.dirname(HEADER))):
        exe = tmp_path / f"consts_{tag}"
        subprocess.run(["gcc", "-std=c99", "-Winvalid-pch", f"-DHDR={hdr}", "-I", inc, str(src),
                        "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
        vals[tag] = dict(line.split() for line in out.splitlines())
    for n in ("SHMEM_REDUCE_SYNC_SIZE", "SHMEM_REDUCE_MIN_WRKDATA_SIZE", "SHMEM_SYNC_VALUE"):
        assert vals["ours"][n] == vals["ref"][n], n
    user = tmp_path / "user.c"
    user.write_text(r'''#include <shmem.h>
static long pSync[_SHMEM_REDUCE_SYNC_SIZE];
static double dWrk[_SHMEM_REDUCE_MIN_WRKDATA_SIZE];
static long long llWrk[_SHMEM_REDUCE_MIN_WRKDATA_SIZE];
int main(void) {
    static double t[4], s[4];
    static long long total, mine = 1;
    for (int i = 0; i < _SHMEM_REDUCE_SYNC_SIZE; i++) pSync[i] = _SHMEM_SYNC_VALUE;
    shmem_init();
    shmem_double_sum_to_all(t, s, 4, 0, 0, shmem_n_pes(), dWrk, pSync);
    shmem_longlong_sum_to_all(&total, &mine, 1, 0, 0, shmem_n_pes(), llWrk, pSync);
    shmem_barrier_all();
    shmem_finalize();
    return 0;
}
''')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-Winvalid-pch", "-I", REF_API, str(user),
                    "-L", LIBDIR, "-lshmem_reduce_mi355x", f"-Wl,-rpath,{LIBDIR}",
                    "-Wl,--no-undefined", "-o", str(tmp_path / "user")], check=True)


def test_header_compiles_as_cpp(tmp_path):
    src = tmp_path / "caller.cpp"
    src.write_text('#include "shmem_reduce_mi355x.h"\n'
                   'int main(){ std::complex<double> a, b; '
                   'shmem_complexd_sum_to_all(&a, &b, 1, 0, 0, 1, nullptr, nullptr); return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)],
                   check=True)


# ------------------------------------------------------------------- plans
def test_plan_algorithm_selection(shm):
    P = shm.plan
    # full set, RCCL-native pairs -> RCCL reduce-scatter + all-gather; up to
    # 4 MiB ($SHMEMX_ALLREDUCE_MAX_KB) one RCCL all-reduce
    assert P("double", "sum", 1 << 25, 0, 0, 8, 3, 8).algo == "rccl"
    assert P("double", "sum", (4 << 20) // 8 + 1, 0, 0, 8, 3, 8).algo == "rccl"
    assert P("double", "sum", (4 << 20) // 8, 0, 0, 8, 3, 8).algo == "allreduce"
    assert P("long", "max", 1000, 0, 0, 4, 0, 4).algo == "allreduce"
    assert P("int", "prod", 1000, 0, 0, 2, 1, 2).algo == "allreduce"
    # bitwise (no RCCL op), short (no RCCL type), complex -> A2A
    for t, o in [("long", "xor"), ("int", "and"), ("short", "sum"), ("complexd", "prod")]:
        assert P(t, o, 1000, 0, 0, 4, 2, 4).algo == "a2a", (t, o)
    # float / double / long double min and max: each PE's own fold order
    # (a<b?a:b under NaN and +-0), so GATHER under auto and for an explicit
    # a2a; DIRECT and SIGNAL plan the whole array on every member
    for t in ("float", "double", "longdouble"):
        for o in ("min", "max"):
            assert P(t, o, 1000, 0, 0, 4, 2, 4).algo == "gather", (t, o)
            assert P(t, o, 1000, 0, 0, 4, 2, 4, "a2a").algo == "gather", (t, o)
            for a in ("direct", "signal"):
                q = P(t, o, 1000, 0, 0, 4, 2, 4, a)
                assert q.algo == a and q.chunk == 1000, (t, o, a)
    assert P("double", "min", 1000, 0, 0, 4, 2, 4, "direct").chunk == 1000
    assert P("double", "sum", 1000, 0, 0, 4, 2, 4, "direct").chunk == 250
    # strided or partial sets: A2A under the built-in rule (PE_start bits, no
    # communicator set-up); the set's members-only RCCL communicator
    # (set_comm.cpp) when asked for by name
    assert P("double", "sum", 1000, 0, 1, 4, 2, 8).algo == "a2a"
    assert P("double", "sum", 1000, 1, 0, 3, 2, 8).algo == "a2a"
    assert P("double", "sum", 1 << 20, 1, 0, 3, 2, 8).algo == "a2a"
    assert P("double", "sum", 1000, 1, 0, 3, 2, 8, "rccl").algo == "rccl"
    assert P("double", "sum", 1000, 1, 0, 3, 2, 8, "allreduce").algo == "allreduce"
    assert P("long", "xor", 1000, 1, 0, 3, 2, 8).algo == "a2a"
    assert P("float", "min", 1000, 0, 1, 4, 2, 8).algo == "gather"
    # explicit choices
    assert P("double", "sum", 1000, 0, 0, 4, 2, 4, "gather").algo == "gather"
    assert P("double", "sum", 1000, 0, 0, 4, 2, 4, "a2a").algo == "a2a"
    with pytest.raises(shm.ShmemError) as e:
        P("long", "xor", 1000, 0, 0, 4, 2, 4, "rccl")
    assert e.value.code == 3


def test_plan_errors(shm):
    P = shm.plan
    cases = [((100, 0, 0, 4, 5, 8), 2),      # PE 5 not in {0..3}
             ((100, 1, 1, 3, 2, 8), 2),      # PE 2 not in {1,3,5}
             ((100, 0, 0, 9, 0, 8), 1),      # set beyond npes
             ((-1, 0, 0, 2, 0, 2), 1),       # nreduce < 0
             ((100, 0, -1, 2, 0, 2), 1),     # negative stride
             ((100, 0, 0, 0, 0, 2), 1)]      # empty set
    for args, code in cases:
        with pytest.raises(shm.ShmemError) as e:
            P("double", "sum", *args)
        assert e.value.code == code, args
    assert P("longdouble", "sum", 10, 0, 0, 1, 0, 1).algo in ("a2a", "rccl")
    assert P("longdouble", "max", 10, 0, 0, 4, 1, 4).algo == "gather"   # own order
    assert P("longdouble", "sum", 10, 0, 0, 4, 1, 4).algo == "a2a"   # no RCCL type
    with pytest.raises(shm.ShmemError) as e:
        P("double", "xor", 10, 0, 0, 1, 0, 1)
    assert e.value.code == 1


@pytest.mark.parametrize("t", ["short", "int", "double", "complexd", "complexf"])
@pytest.mark.parametrize("P_", [2, 3, 5, 8])
@pytest.mark.parametrize("n", [0, 1, 7, 64, 1000, 4103, (1 << 25) + 3])
def test_plan_shards_cover_and_align(shm, t, P_, n):
    """A2A shards tile [0, n) exactly, every shard starts on a 16-byte
    boundary of the array; RCCL main+tail == n with 16-byte shards."""
    sz = shm.type_size(t)
    g = max(1, 16 // sz)
    p = shm.plan(t, "sum", n, 0, 0, P_, 0, P_, "a2a")
    assert p.chunk % g == 0 and p.chunk * P_ >= n
    counts = [max(0, min(p.chunk, n - i * p.chunk)) for i in range(P_)]
    assert sum(counts) == n
    assert p.ws_bytes == p.chunk * P_ * sz
    if t in ("int", "double"):
        r = shm.plan(t, "sum", n, 0, 0, P_, 0, P_, "rccl")
        assert r.main == r.chunk * P_ and r.main + r.tail == n
        assert r.chunk % g == 0 and r.tail < P_ * g
    q = shm.plan(t, "sum", n, 0, 0, P_, 0, P_, "gather")
    assert q.ws_bytes == n * P_ * sz


def test_direct_stats_without_calls(shm):
    """shmemx_direct_stats is host-only bookkeeping: no DIRECT call yet means
    zero calls, zero time in every phase and no fences checked, and it never
    needs a device."""
    st = shm.direct_stats(reset=True)
    assert st["calls"] == 0
    assert set(st) == {"calls", *shm.DIRECT_PHASES, *shm.FENCE_STATS, *shm.DIRECT_COUNTS}
    assert all(v == 0 for v in st.values())


def test_typed_stream_forms_for_all_44(shm):
    """shmemx_<T>_<op>_to_all_on_stream exists for every reference pair and
    the header declares it returning int."""
    syms = exported()
    missing = [f"shmemx_{t}_{o}_to_all_on_stream" for t, o in shm.REFERENCE_PAIRS
               if f"shmemx_{t}_{o}_to_all_on_stream" not in syms]
    assert not missing, missing
    pre = subprocess.run(["gcc", "-E", "-P", "-x", "c", HEADER], check=True,
                         capture_output=True, text=True).stdout
    decls = re.findall(r"(\w+)\s+shmemx_\w+_to_all_on_stream\s*\(", pre)
    assert len(decls) == 44 and set(decls) == {"int"}


def test_fortran_constants_match_the_c_header():
    """include/shmem_reduce_mi355x.fh holds the reference's Fortran values
    (src/shmem.fh:63-82): default INTEGER words, twice the C header's long
    counts on LP64; SHMEM_SYNC_VALUE is the same -1."""
    inc = os.path.join(REPO, "include")
    c = dict(re.findall(r"#define\s+(SHMEM_\w+)\s+\(?(-?\d+)L\)?", open(os.path.join(inc, "shmem_reduce_mi355x.h")).read()))
    f = dict(re.findall(r"parameter\s*\(\s*(SHMEM_\w+)\s*=\s*(-?\d+)\s*\)", open(os.path.join(inc, "shmem_reduce_mi355x.fh")).read()))
    assert set(f) == {"SHMEM_REDUCE_SYNC_SIZE", "SHMEM_REDUCE_MIN_WRKDATA_SIZE", "SHMEM_BCAST_SYNC_SIZE",
                      "SHMEM_BARRIER_SYNC_SIZE", "SHMEM_COLLECT_SYNC_SIZE", "SHMEM_SYNC_VALUE"}
    for name, v in f.items():
        want = int(c[name]) if name == "SHMEM_SYNC_VALUE" else 2 * int(c[name])
        assert int(v) == want, (name, v, c[name])


@pytest.mark.parametrize("peers", [False, True])
def test_fold_n_argument_errors_without_a_device(shm, peers):
    """shmemx_fold_n_on_stream / shmemx_fold_n_peers_on_stream reject bad
    arguments before touching HIP: EINVAL for no inputs, a NULL input or a
    pair the reference lacks; nothing to do for zero elements."""
    import ctypes
    fn = shm.lib().shmemx_fold_n_peers_on_stream if peers else shm.lib().shmemx_fold_n_on_stream
    T, O = shm.TYPES, shm.OPS
    ins = (ctypes.c_void_p * 2)(8, None)
    assert fn(T["double"], O["sum"], 8, ins, 0, 16, None) == 1            # nins < 1
    assert fn(T["double"], O["sum"], 8, ins, 2, 16, None) == 1            # NULL input
    assert fn(T["double"], O["xor"], 8, ins, 1, 16, None) == 1            # not a reference pair
    assert fn(T["double"], O["sum"], 8, ins, 2, 0, None) == 0             # zero elements


def test_fold_launch_shape_is_declared_exported_and_host_only(shm):
    """shmemx_fold_launch_shape: the header declares it, nm -D shows it as a
    defined function, and it answers from the addresses mod 16 alone (made-up
    addresses, no device): family, MAXIN, vectors per lane, NT bits, grid,
    split, scalar trips.  EINVAL exactly where the launch refuses."""
    import ctypes
    assert "shmemx_fold_launch_shape" in declared_functions()
    assert exported()["shmemx_fold_launch_shape"][1] == "T"
    q = shm.fold_launch_shape
    A = [0x7F0000000000 + (k << 32) for k in range(17)]
    n2 = (32 << 20) // 24                                  # 3 arrays of n doubles reach 32 MiB one past this
    s = q("double", "sum", "plain", A[0], [A[0], A[1]], n2 + 1)
    assert (s.family, s.maxin, s.vectors_per_lane, s.nt) == ("fold2", 0, 4, 3)
    assert (s.head, s.nvec, s.tail, s.scalar_trips) == (0, (n2 + 1) // 2, (n2 + 1) % 2, (n2 + 1) % 2)
    assert s.blocks == -(-s.nvec // 1024) and not s.ld80_pipelined
    assert q("double", "sum", "plain", A[0], [A[0], A[1]], n2).nt == 0
    s = q("short", "max", "peers", A[0] + 2, [a + 2 for a in A[1:6]], 1000)
    assert (s.family, s.maxin, s.vectors_per_lane, s.nt, s.blocks) == ("peers", 8, 4, 0, 1)
    assert (s.head, s.nvec, s.tail, s.scalar_trips) == (7, 124, 1, 1)
    s = q("short", "max", "peers", A[0], [a + 2 for a in A[1:6]], 2048 * 256 + 1)   # the target apart
    assert (s.family, s.head, s.nvec, s.tail, s.blocks, s.scalar_trips) == ("peers", 2048 * 256 + 1, 0, 0, 2048, 2)
    assert q("int", "xor", "peers", A[0], A[1:13], 4096).maxin == 16
    assert q("int", "xor", "peers", A[0], A[1:13], 4096).vectors_per_lane == 2
    assert q("int", "xor", "peers", A[0], A[1:3], 4096).family == "fold2"
    assert q("int", "xor", "plain", A[0], A[1:13], 4096).family == "fold_n"
    s = q("longdouble", "prod", "peers", A[0], A[1:4], 4096)         # heavy: the runtime-nins kernel
    assert (s.family, s.maxin, s.ld80_pipelined) == ("fold_n", 0, True)
    assert not q("longdouble", "prod", "plain", A[0], A[1:4], 1023).ld80_pipelined   # no whole chunk
    assert q("complexf", "prod", "peers", A[0], A[1:4], 64).family == "fold_n"
    assert q("complexf", "sum", "peers", A[0], A[1:4], 64).family == "peers"
    s = q("float", "min", "orders", A[:9], A[8:17], 1000)             # outs[8] is ins[0]: addresses only
    assert (s.family, s.maxin, s.vectors_per_lane, s.nvec) == ("orders", 16, 1, 250)
    assert q("float", "min", "orders", A[:8], A[8:16], 1000).maxin == 8
    s = q("complexd", "sum", "plain", A[0], [A[1] + 8], 300)          # the copy, source at 8 mod 16
    assert (s.family, s.vectors_per_lane, s.nvec, s.blocks, s.scalar_trips) == ("copy", 8, 0, 2, 1)
    assert q("int", "sum", "plain", A[0], [A[1]], 2048 * 4).vectors_per_lane == 8
    assert q("int", "sum", "plain", A[0], [A[1]], 2048 * 4 + 4).vectors_per_lane == 1
    s = q("int", "sum", "plain", A[0], [A[1]], 0)                     # nothing to launch
    assert s.family is None and s.blocks == 0

    fn = shm.lib().shmemx_fold_launch_shape
    T, O = shm.TYPES, shm.OPS
    out = shm.LaunchShape()
    good = (ctypes.c_void_p * 17)(*A)
    hole = (ctypes.c_void_p * 17)(*(A[:3] + [None] + A[4:]))
    null_out = (ctypes.c_void_p * 1)(None)

    def call(t="double", op="sum", route=0, nins=3, n=64, outs=good, ins=good, shape=out):
        return fn(T[t], O[op], route, nins, n, outs, ins, ctypes.byref(shape) if shape is not None else None)

    assert call() == 0
    assert call(op="xor") == 1                        # not a reference pair
    assert fn(99, 0, 0, 3, 64, good, good, ctypes.byref(out)) == 1
    for route in (-1, 3):
        assert call(route=route) == 1
    for route in (0, 1, 2):
        op = "max" if route == 2 else "sum"
        assert call(op=op, route=route, nins=0) == 1 and call(op=op, route=route, nins=17) == 1
        assert call(op=op, route=route, nins=16) == 0
        assert call(op=op, route=route, nins=5, ins=hole) == 1     # a NULL input
        assert call(op=op, route=route, outs=None) == 1
        assert call(op=op, route=route, ins=None) == 1
        assert call(op=op, route=route, shape=None) == 1
    assert call(outs=null_out) == 1 and call(route=1, outs=null_out) == 1
    assert call(route=2, op="max", nins=5, outs=hole) == 1          # a NULL output of the P-order fold
    assert call(route=2, op="sum") == 1 and call(route=2, t="int", op="max") == 1   # not an own-order pair
    assert call(n=0, ins=None) == 0 and out.family == -1            # zero elements: the inputs are not looked at


def test_fused_loopback_argument_errors_without_a_device(shm):
    """shmemx_fused_loopback rejects bad arguments before touching HIP: EINVAL
    for a pair the reference lacks, a schedule outside 0..2, P outside 1..16,
    m outside 0..P-1, own order with the two shot, and NULL arrays or a NULL
    entry when there are elements; nothing to do for zero elements."""
    import ctypes
    fn = shm.lib().shmemx_fused_loopback
    D, I = shm.TYPES["double"], shm.TYPES["int"]
    SUM, XOR, MIN = shm.OPS["sum"], shm.OPS["xor"], shm.OPS["min"]
    good = (ctypes.c_void_p * 16)(*([64] * 16))
    hole = (ctypes.c_void_p * 16)(*([64] * 5 + [None] + [64] * 10))
    err = ctypes.c_uint(7)
    for schedule in (0, 1, 2):
        assert fn(D, XOR, schedule, 3, 0, 0, good, good, 16, err, None) == 1       # not a reference pair
        assert fn(shm.TYPES["complexd"], MIN, schedule, 3, 0, 0, good, good, 16, err, None) == 1
        assert fn(99, SUM, schedule, 3, 0, 0, good, good, 16, err, None) == 1
        for P in (0, -1, 17):
            assert fn(D, SUM, schedule, P, 0, 0, good, good, 16, err, None) == 1   # P outside 1..16
        for P, m in ((3, -1), (3, 3), (16, 16), (1, 1)):
            assert fn(D, SUM, schedule, P, m, 0, good, good, 16, err, None) == 1   # m outside 0..P-1
    for schedule in (-1, 3):
        assert fn(D, SUM, schedule, 3, 0, 0, good, good, 16, err, None) == 1
    assert fn(D, MIN, 1, 3, 0, 1, good, good, 16, err, None) == 1                  # own order, two shot
    assert fn(D, MIN, 1, 3, 0, 1, good, good, 0, err, None) == 1
    for schedule in (0, 1):
        assert fn(D, SUM, schedule, 3, 0, 0, None, good, 16, err, None) == 1       # NULL arrays
        assert fn(D, SUM, schedule, 3, 0, 0, good, None, 16, err, None) == 1
        assert fn(D, SUM, schedule, 6, 0, 0, hole, good, 16, err, None) == 1       # a NULL entry
        assert fn(I, XOR, schedule, 6, 2, 0, good, hole, 16, err, None) == 1
        # zero elements: nothing to do, whatever the arrays
        assert fn(D, SUM, schedule, 3, 2, 0, good, good, 0, err, None) == 0
        assert fn(D, SUM, schedule, 6, 0, 0, hole, None, 0, None, None) == 0
    assert fn(D, MIN, 0, 16, 15, 1, good, good, 0, err, None) == 0                 # own order, one shot
    assert shm.last_error() == 0
    assert err.value == 7        # never written before a launch
    with pytest.raises(shm.ShmemError) as e:
        shm.fused_loopback("double", "sum", 1, [64, 64], [64, 0], 8, m=1)
    assert e.value.code == 1
    with pytest.raises(ValueError):
        shm.fused_loopback("double", "sum", 0, [64, 64], [64], 8)
    assert shm.fused_loopback("double", "sum", 0, [64, 64], [64, 64], 0) == 0


def test_service_fold_loopback_argument_errors_without_a_device(shm):
    """shmemx_service_fold_loopback rejects bad arguments before touching HIP:
    EINVAL for a pair the reference lacks, PE_size outside 1..64, a negative
    PE_start, logPE_stride outside 0..7, a last member at 64 or above, a
    caller outside the set, more elements than one slot holds, a NULL target,
    and NULL sources or a NULL entry when there are elements; nothing to do
    for zero elements.  (No call here passes those checks with elements to
    fold: the fake addresses are never used.)"""
    import ctypes
    fn = shm.lib().shmemx_service_fold_loopback
    D, I = shm.TYPES["double"], shm.TYPES["int"]
    SUM, XOR, MIN = shm.OPS["sum"], shm.OPS["xor"], shm.OPS["min"]
    good = (ctypes.c_void_p * 64)(*([64] * 64))
    hole = (ctypes.c_void_p * 64)(*([64] * 5 + [None] + [64] * 58))
    EINVAL = 1

    def call(t=D, op=SUM, own=0, start=0, log=0, size=3, me=0, dst=64, dst2=None, srcs=good, n=4):
        return fn(t, op, own, start, log, size, me, dst, dst2, srcs, n)

    assert call(op=XOR) == EINVAL                                   # not a reference pair
    assert call(t=shm.TYPES["complexd"], op=MIN) == EINVAL
    assert call(t=99) == EINVAL
    for size in (0, -1, 65):
        assert call(size=size) == EINVAL                            # PE_size outside 1..64
    assert call(start=-1, me=-1) == EINVAL                          # PE_start < 0
    assert call(start=-1, me=0) == EINVAL
    for log in (-1, 8, 31):
        assert call(log=log, size=1) == EINVAL                      # logPE_stride outside 0..7
    for start, log, size in ((62, 0, 3), (64, 0, 1), (0, 0, 65), (1, 6, 2), (0, 7, 2), (4, 2, 16), (0, 1, 33)):
        assert call(start=start, log=log, size=size, me=start) == EINVAL   # a member at 64 or above
    for start, log, size, me in ((0, 0, 3, 3), (0, 0, 3, -1), (2, 0, 3, 1), (0, 1, 3, 1), (0, 1, 3, 6),
                                 (4, 2, 3, 6), (0, 0, 64, 64)):
        assert call(start=start, log=log, size=size, me=me) == EINVAL      # me is no member
    for name, t in shm.TYPES.items():
        op = SUM
        assert call(t=t, op=op, n=4096 // shm.type_size(name) + 1) == EINVAL   # more than a slot
    assert call(n=2 ** 61) == EINVAL                                # (nelems * size wraps)
    assert call(dst=None) == EINVAL                                 # NULL target
    assert call(srcs=None) == EINVAL                                # NULL sources
    assert call(size=6, srcs=hole) == EINVAL                        # a NULL entry
    assert call(t=I, op=XOR, size=6, me=5, srcs=hole) == EINVAL
    assert shm.last_error() == EINVAL
    # zero elements: nothing to do, whatever the sources
    assert call(n=0) == 0
    assert call(n=0, srcs=None) == 0
    assert call(n=0, size=6, srcs=hole, dst2=64) == 0
    assert call(n=0, start=63, size=1, me=63, own=1, op=MIN) == 0
    assert call(n=0, start=1, log=1, size=32, me=63) == 0           # the last member is PE 63
    assert shm.last_error() == 0
    # ... but the other checks still hold
    assert call(n=0, dst=None) == EINVAL
    assert call(n=0, me=3) == EINVAL
    with pytest.raises(shm.ShmemError) as e:
        shm.service_fold_loopback("double", "sum", 64, [64, 64, 0], 4)
    assert e.value.code == EINVAL
    shm.service_fold_loopback("double", "sum", 64, [64, 64], 0, PE_start=3, me=4)


def test_fused_twoshot_limit_setter(shm):
    """shmemx_set_fused_twoshot_kb returns the previous limit (the 4 MiB
    default unless $SHMEMX_FUSED_TWOSHOT_KB says otherwise) and refuses a
    negative one."""
    import os
    default = int(os.environ.get("SHMEMX_FUSED_TWOSHOT_KB", "4096"))
    prev = shm.set_fused_twoshot_kb(0)
    assert prev == default
    assert shm.set_fused_twoshot_kb(16384) == 0
    with pytest.raises(shm.ShmemError):
        shm.set_fused_twoshot_kb(-1)
    assert shm.set_fused_twoshot_kb(prev) == 16384


def test_plan_without_set_comms():
    """$SHMEMX_SET_COMMS=0 (read once per process, so in a child): partial
    sets plan A2A for the RCCL-native pairs and refuse an explicit rccl, as
    before set communicators existed; the whole job is unchanged."""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import shmem_mi355x as shm\n"
            "assert shm.plan('double', 'sum', 1000, 1, 0, 3, 2, 8).algo == 'a2a'\n"
            "assert shm.plan('double', 'sum', 1000, 0, 0, 8, 2, 8).algo == 'allreduce'\n"
            "try:\n    shm.plan('double', 'sum', 1000, 1, 0, 3, 2, 8, 'rccl')\n    raise SystemExit('rccl planned')\n"
            "except shm.ShmemError as e:\n    assert e.code == 3\n"
            "print('ok')\n") % os.path.join(os.path.dirname(HEADER), "..", "openshmem-async_amd")
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SHMEMX_SET_COMMS="0"),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
