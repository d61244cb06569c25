"""CPU check of the small-call exchange's slot protocol
(openshmem-async_amd/csrc/node.cpp xchg_claim / xchg_finish: the per-pair done
counts that stand in for the reference's exit barrier), with real forked
processes, random overlapping active sets and readers that sleep while the
writers run ahead (tests/native/test_xchg.cpp).  No GPU: the block is mapped
without page-locking it, node::xchg_attach(false).

The negative control (--write-before-claim: the slot is filled before
xchg_claim's wait instead of after it, 2 PEs, every reader sleeps 50-300 us on
every call) must be seen to fail, by exit status 1 and a message that names
the slot, not by a hang or an abort.

No ThreadSanitizer run of this program: its PEs are processes, and the tool
does not follow shared memory across fork().  AddressSanitizer and
UndefinedBehaviorSanitizer run it in test_sanitize_host.py."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "openshmem-async_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("xchg") / "test_xchg"
    subprocess.run(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", CSRC,
                    "-I", os.path.join(REPO, "include"), "-I", "/opt/rocm/include",
                    os.path.join(REPO, "tests", "native", "test_xchg.cpp"),
                    os.path.join(CSRC, "node.cpp"), "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath,/opt/rocm/lib", "-o", str(out)], check=True)
    return str(out)


def _run(exe, *args):
    env = dict(os.environ, SHMEMX_BARRIER_TIMEOUT="60")
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, env=env)


@pytest.mark.parametrize("npes", [2, 5, 8])
def test_xchg_slots_random_overlapping_sets(exe, npes):
    out = _run(exe, str(npes), "3000")
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok 3000 calls"), out.stdout


def test_xchg_control_write_before_claim_is_caught(exe):
    out = _run(exe, "--write-before-claim", "2", "3000")
    assert out.returncode == 1, (out.returncode, out.stdout + out.stderr)
    assert out.stdout.startswith("FAIL call ") and "slot" in out.stdout, out.stdout + out.stderr
    assert "FATAL" not in out.stderr, out.stderr
