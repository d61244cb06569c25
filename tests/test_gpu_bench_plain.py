"""bench.py's plain N = 1 run (`bench.py --gpus 1 --steps K --warmup W`, the
command every change is measured with) and --dump-outputs: the line carries
the headline alone, the dumped array is what the timed steps left in the
fold's accumulator, the same from run to run, and --steps sets the number of
timed steps.  Small arrays (64 Ki doubles): the numbers are not reported.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
N = 1 << 16


@functools.lru_cache(maxsize=None)
def plain_run(out_dir, steps, warmup):
    """One plain bench process; (line, dumped accumulator)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps),
           "--warmup", str(warmup), "--nreduce", str(N), "--dump-outputs", out_dir]
    p = subprocess.run(cmd, env=env, cwd=REPO, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-3000:]}"
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0]), np.load(os.path.join(out_dir, "acc.npy"))


@pytest.fixture(scope="module")
def dump_root(tmp_path_factory):
    return tmp_path_factory.mktemp("bench_plain")


@pytest.mark.gpu
def test_plain_line_is_the_headline_alone_and_dump_repeats(dump_root):
    line, acc = plain_run(str(dump_root / "k2"), 2, 0)
    assert line["steps"] == 2 and line["warmup"] == 0 and line["n_gpus"] == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["unit"] == "GiB/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f64"
    # value = nreduce x 8 B per step time, in GiB/s; the line rounds value to
    # 0.01 and ms_per_step to 0.0001
    ms = line["ms_per_step"]
    want = N * 8 / (ms * 1e-3) / 2 ** 30
    assert abs(line["value"] - want) <= 0.005 + want * 0.00005 / ms + 1e-9, (line["value"], ms)
    # nothing but the headline: no guard, no CPU baseline, no extras
    assert line["full"] is False and line["correct"] is None
    assert line["cpu_baseline"] is None and line["extras"] == {}
    assert "kernel_clock_us" not in line["roofline"] and "measured_ceiling" not in line["roofline"]
    assert line["outputs"] == {"file": "acc.npy", "dtype": "float64", "elements": N, "of": N, "sample": None}
    assert acc.dtype == np.float64 and acc.shape == (N,)
    line_b, acc_b = plain_run(str(dump_root / "again"), 2, 0)
    assert acc.tobytes() == acc_b.tobytes()


@pytest.mark.gpu
def test_steps_sets_the_number_of_timed_steps(dump_root):
    """acc starts as src and every step adds in (both in [1, 2)): after 0
    warm-up and K steps acc = src + K x in, rounded once per step.  From the
    dumps of K = 1, 2 and 3: in = acc2 - acc1 (exact or one rounding off),
    and acc3 must be acc2 + in again, not acc2 or acc2 + 2 in."""
    acc1 = plain_run(str(dump_root / "k1"), 1, 0)[1]
    acc2 = plain_run(str(dump_root / "k2"), 2, 0)[1]
    acc3 = plain_run(str(dump_root / "k3"), 3, 0)[1]
    inp = acc2 - acc1
    u = 2.0 ** -53
    assert (acc1 >= 2.0).all() and (acc1 < 4.0).all()
    assert (inp >= 1.0 - 8 * u).all() and (inp < 2.0 + 8 * u).all()
    # one rounding of a value below 8 per step: |error| <= 8 u each, 3 in all
    assert (np.abs(acc3 - (acc2 + inp)) <= 3 * 8 * u).all()
