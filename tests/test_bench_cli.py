"""GPU: bench.py's command line.  A plain run times the headline's steps and nothing else;
--dump-outputs writes the timed launch's last-step outputs, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOARDS, STEPS, WARMUP = 8192, 20, 5
# the other legs' keys in the --full line
FULL_KEYS = ("launched_step", "api_step", "perft_startpos", "single_env", "variants", "perft", "concurrent")
DUMPED = {"action": (BOARDS,), "reward": (BOARDS,), "done": (BOARDS,), "reason": (BOARDS,),
          "boards": (BOARDS, 64), "meta": (BOARDS, 8), "nsteps": (BOARDS,)}


def run_bench(out_dir):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "GC_BENCH_DEVICES"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                          "--warmup", str(WARMUP), "--settle", "300", "--boards", str(BOARDS),
                          "--dump-outputs", str(out_dir)], capture_output=True, text=True, env=env, timeout=120,
                         check=True)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0]), {k: np.load(os.path.join(out_dir, k + ".npy")) for k in DUMPED}


@pytest.fixture(scope="module")
def first_run(tmp_path_factory):
    return run_bench(tmp_path_factory.mktemp("dump_a"))


@pytest.mark.gpu
def test_plain_line_is_the_headline_alone(first_run):
    line, _ = first_run
    assert line["unit"] == "env_steps/s" and line["higher_is_better"] is True and line["dtype"] == "u64"
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["n_gpus"] == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["ms_per_step"] * STEPS - line["timed_region_ms"]) <= 1e-9 * line["timed_region_ms"]
    # value = the timed steps of every board / the region: at most one step per board per ply
    assert line["value"] * line["timed_region_ms"] / 1e3 <= BOARDS * STEPS * (1 + 1e-9)
    assert line["cpu_baseline"] is None and not [k for k in FULL_KEYS if k in line]


@pytest.mark.gpu
def test_dumped_outputs(first_run, tmp_path):
    _, a = first_run
    for k, shape in DUMPED.items():
        assert a[k].dtype == np.float32 and a[k].shape == shape, k
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    # one step's outputs in their ranges: an action of the 4101 (-1: the driver's no-move reset),
    # a done flag, a reason code, piece ids, and boards that have all stepped
    assert ((a["action"] >= -1) & (a["action"] < 4101)).all() and np.isin(a["done"], (0, 1)).all()
    assert ((a["reason"] >= 0) & (a["reason"] <= 10)).all() and (np.abs(a["boards"]) <= 6).all()
    assert (a["nsteps"] > 0).all() and (a["nsteps"] <= 300 + WARMUP + STEPS).all()
    _, b = run_bench(tmp_path)  # the same arguments: the same inputs, the same outputs
    for k in DUMPED:
        assert np.array_equal(a[k], b[k]), k
