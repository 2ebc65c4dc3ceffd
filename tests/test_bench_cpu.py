"""bench.py driver contract on the CPU path (tiny GPT): the result line,
--steps, --full and --dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(*extra):
    env = dict(os.environ)
    # tiny CPU config even on a GPU machine: this checks the driver
    # contract, not throughput
    env["CUDA_VISIBLE_DEVICES"] = ""
    env["HIP_VISIBLE_DEVICES"] = ""
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
         "--steps", "3", "--warmup", "1", *extra],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_dump_outputs_reproducible(tmp_path):
    d1, d2 = tmp_path / "a", tmp_path / "b"
    res = _run_bench("--dump-outputs", str(d1))
    res_full = _run_bench("--full", "--dump-outputs", str(d2))
    for r in (res, res_full):
        assert r["metric"] == "model_tflops_aggregate"
        assert r["unit"] == "TFLOPS" and r["higher_is_better"] is True
        assert r["steps"] == 3 and r["warmup"] == 1
        assert r["ms_per_step"] > 0 and r["value"] >= 0
        assert "dtype" in r
    names = sorted(os.listdir(d1))
    assert names == ["loss.npy", "params_sample.npy"]
    assert sorted(os.listdir(d2)) == names
    total = 0
    for n in names:
        a, b = np.load(d1 / n), np.load(d2 / n)
        assert a.dtype == np.float32 and a.size > 0
        assert np.isfinite(a).all()
        # seeded weights + inputs: the CPU path is bit-reproducible
        np.testing.assert_array_equal(a, b)
        total += a.nbytes
    assert total <= 64 * 2**20
    loss = np.load(d1 / "loss.npy")
    assert loss.shape == (1,)
    assert abs(float(loss[0]) - res["config"]["loss"]) < 1e-6
