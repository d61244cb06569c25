"""alltoallv_plan (set_geom.h), the layout a receiver of a stream-ordered
alltoallv derives from the (count, offset) pairs its peers hold for it, as a
stand-alone host program under AddressSanitizer and UndefinedBehaviorSanitizer
(gcc) against a brute-force model: target offsets are prefix sums in sender
order, `from` is carried through, empty blocks are left out, every bad pair is
rejected in every position, a total above the capacity overflows, sums near
2^64 saturate instead of wrapping, and the fixed alltoall's immediates are
exact (tests/native/test_alltoallv_geom.cpp)."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "openshmem-async_amd", "csrc")
SRC = os.path.join(REPO, "tests", "native", "test_alltoallv_geom.cpp")


def test_alltoallv_plan_under_asan_ubsan(tmp_path):
    exe = tmp_path / "alltoallv_geom_san"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-I", CSRC, SRC, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
                                  UBSAN_OPTIONS="print_stacktrace=1"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.startswith("ok "), out.stdout[-2000:]
    assert "runtime error" not in out.stderr, out.stderr[-4000:]
