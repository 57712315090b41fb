"""bench.py end to end on the GPU at a small size: a plain run prints the headline line only,
--steps sets the number of timed steps, and --dump-outputs writes the per-tape results of the last
timed step, which equal an independent run of the same seeded workload on the interpreter."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from mythril_amd import native, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAPES, ROWS = 48, 4096 + 77  # more than one workgroup, a partial last block


def _bench(args):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--tapes", str(TAPES), "--rows-per-gpu", str(ROWS)] + args, env=env,
                       capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0]), p.stderr


def test_plain_run_dumps_the_last_steps_results(gpu_ctx, tmp_path):
    out = str(tmp_path / "dump")
    line, err = _bench(["--steps", "3", "--warmup", "2", "--dump-outputs", out])
    assert line["metric"] == "constraint-evals/sec" and line["unit"] == "evals/s"
    assert line["higher_is_better"] is True and line["dtype"] == "u32"
    assert line["steps"] == 3 and line["warmup"] == 2
    assert err.count("] step ") == 3 and err.count("] warmup ") == 2
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(TAPES * ROWS / (line["ms_per_step"] / 1e3))
    # a plain run measures nothing beside the headline
    assert line["full"] is False
    assert not {"roofline", "full_eval", "cpu_baseline"} & set(line)
    assert sorted(os.listdir(out)) == ["first_hit.npy", "hit_count.npy"]
    fh = np.load(os.path.join(out, "first_hit.npy"))
    hc = np.load(os.path.join(out, "hit_count.npy"))
    assert fh.dtype == np.float64 and hc.dtype == np.float64
    assert fh.shape == (TAPES,) and hc.shape == (TAPES,)
    assert int((hc > 0).sum()) == line["tapes_with_witness"]
    # the same seeded workload through the interpreter in this process
    ts = synth.generate(TAPES)
    a = gpu_ctx.assignments(ts.n_vars, ROWS)
    a.generate(synth.load_spec()["assignment_seed"], 0)
    fh0, hc0 = native.run(gpu_ctx, gpu_ctx.compile(ts), a, mode=native.MODE_COUNT_ALL)
    assert np.array_equal(hc, hc0.astype(np.float64))
    assert np.array_equal(fh, fh0.view(np.int64).astype(np.float64))
    assert (fh[hc == 0] == -1).all() and (fh[hc > 0] >= 0).all()


def test_full_run_adds_the_other_figures():
    line, _ = _bench(["--steps", "1", "--warmup", "0", "--full", "--cpu-seconds", "0.2"])
    assert line["full"] is True and line["steps"] == 1
    assert line["full_eval"]["results_identical"] is True
    assert line["roofline"]["peak_measured_add_chain"] > 0
    assert line["cpu_baseline"]["value"] > 0
