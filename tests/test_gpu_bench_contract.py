"""The driver-facing contract of bench.py: ONE JSON line on stdout, with the fields the round instructions name - run here on a
small batch (the default run is the BASELINE configuration at B = 128) through the same code path: child-process hipGraph
capture, reference-loop timing (H2D + sync per iteration), GEMM replay for `roofline`, the bounded CPU baseline."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_prints_one_json_line_with_the_contract_fields():
    cp = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "16",
                         "--full", "--no-modes", "--cpu-iters", "1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                        timeout=1200, cwd=ROOT)
    assert cp.returncode == 0, cp.stderr[-2000:]
    lines = [ln for ln in cp.stdout.splitlines() if ln.strip()]
    assert lines and lines[-1].startswith("{"), cp.stdout[-500:]
    assert sum(1 for ln in lines if ln.startswith("{") and '"metric"' in ln) == 1
    j = json.loads(lines[-1])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in j, key
    assert j["n_gpus"] == 1 and j["steps"] == 3 and j["warmup"] == 1 and j["higher_is_better"] is True
    assert j["scaling"] == "weak" and j["vs_baseline"] is None and j["dtype"] == "bf16" and j["data"] == "synthetic"
    assert "workload" in j["config"] and "model" not in j["config"]
    assert j["value"] > 0 and abs(j["value"] - 16 * 3 / (j["ms_per_step"] * 3e-3)) / j["value"] < 0.02      # value = B / s per step
    r = j["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in r, key
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and r["peak"] == 2500.0
    assert 0.0 < r["frac"] < 1.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert r["traffic"] is None                 # (the PMC figure belongs to the B = 128 configuration only)
    ev = j["eval"]                              # forward-only throughput of do_inference's call (VERDICT r3 missing #5)
    assert ev["value"] > j["value"] and ev["features_finite"] is True and "eager" in ev
    hk = r["hbm_kernels"]
    assert len(hk) >= 5 and all(k["sets"] >= 3 and 0.0 < k["frac"] < 1.0 for k in hk)      # rotating operand sets: HBM, not Infinity Cache
    c = j["cpu_baseline"]
    for key in ("value", "unit", "cores", "kind", "sample"):
        assert key in c, key
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0


def test_bench_starts_its_own_ranks():
    """`python bench.py --gpus N` must work unaided (VERDICT r3 missing #1): N > 1 re-execs through torch.distributed.run; the
    same launcher is exercised here with one rank (`--spawn`): a real 1-rank RCCL group, bucket all-reduces issued from inside
    the backward, rank 0's JSON line relayed as the only line of stdout."""
    cp = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--spawn", "--steps", "3", "--warmup", "1",
                         "--batch", "16", "--full"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=1200, cwd=ROOT)
    assert cp.returncode == 0, cp.stderr[-3000:]
    lines = [ln for ln in cp.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), cp.stdout[-800:]
    j = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "rccl_ranks", "rank_ms_per_step"):
        assert key in j, key
    assert j["n_gpus"] == 1 and j["rccl_ranks"] == 1 and j["config"]["parallelism"] == "dp1" and j["config"]["global_batch"] == 16
    assert "RCCL" in j["config"]["launch"]
    import math
    assert math.isfinite(j["config"]["loss"]) and j["config"]["loss"] > 0
    assert j["value"] > 0 and abs(j["value"] - 16 * 3 / (j["ms_per_step"] * 3e-3)) / j["value"] < 0.02
    assert len(j["rank_ms_per_step"]["all"]) == 1 and j["rank_ms_per_step"]["max"] <= j["ms_per_step"] * 1.001
    assert j["config"]["grad_buckets"]


def test_plain_bench_times_the_steps_and_dumps_the_last_ones_outputs(tmp_path):
    """The plain line (no --full): the headline fields only; --steps K really runs K timed iterations (EDITOR_BENCH_ITER_TIMES=1: one
    wall time per timed iteration on stderr); --dump-outputs writes what the last timed step computed - the loss, the forward outputs
    and a parameter / gradient sample - as float32 / float64 .npy files, 64 MB at most, and a second run with the same arguments
    (same seeded inputs) writes the same values."""
    import numpy as np
    env = dict(os.environ, EDITOR_BENCH_ITER_TIMES="1")
    runs = []
    for name in ("dump_a", "dump_b"):
        cp = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch",
                             "16", "--dump-outputs", name], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600,
                            cwd=str(tmp_path), env=env)       # (a relative directory: the timing child must write it there too)
        assert cp.returncode == 0, cp.stderr[-2000:]
        lines = [ln for ln in cp.stdout.splitlines() if ln.strip()]
        assert lines and lines[-1].startswith("{"), cp.stdout[-500:]
        j = json.loads(lines[-1])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in j, key
        for key in ("roofline", "eval", "replay_only", "modes", "other_configs", "cpu_baseline", "torch_gpu_yardstick"):
            assert key not in j, key                     # --full only
        assert j["steps"] == 3 and j["warmup"] == 1 and j["dtype"] == "bf16" and j["higher_is_better"] is True
        iters = [ln for ln in cp.stderr.splitlines() if ln.startswith("iteration ms:")]
        assert iters, cp.stderr[-2000:]
        it_ms = [float(v) for v in iters[-1].split(":", 1)[1].split()]
        assert len(it_ms) == 3                           # the timed region ran exactly --steps iterations
        assert abs(sum(it_ms) / 3 - j["ms_per_step"]) <= 0.05 * j["ms_per_step"] + 0.2
        out_dir = tmp_path / name
        files = sorted(p.name for p in out_dir.iterdir())
        assert files == sorted(n + ".npy" for n in j["outputs_dumped"]["arrays"])
        assert {"loss.npy", "output_0.npy", "output_1.npy", "params_sample.npy", "grads_sample.npy"} <= set(files)
        arrays = {f: np.load(out_dir / f) for f in files}
        assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
        assert all(a.dtype in (np.float32, np.float64) and a.size > 0 and np.isfinite(a).all() for a in arrays.values())
        assert arrays["loss.npy"].dtype == np.float64 and arrays["params_sample.npy"].size == arrays["grads_sample.npy"].size
        assert arrays["output_0.npy"].size == 16 * 171 and arrays["output_1.npy"].size == 16 * 2304      # score, cls4t (RGBNT201)
        assert np.abs(arrays["grads_sample.npy"]).max() > 0
        runs.append(arrays)
    for f in runs[0]:
        assert np.array_equal(runs[0][f], runs[1][f]), f


def test_bench_refuses_more_ranks_than_gpus_loudly():
    import torch
    n = torch.cuda.device_count() + 1
    cp = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "1", "--warmup", "0"],
                        stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, cwd=ROOT)
    assert cp.returncode != 0 and "GPU(s)" in cp.stderr and not cp.stdout.strip()
