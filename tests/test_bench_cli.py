"""bench.py command line: the result line's contract, --dump-outputs and
--full, on the tiny dataset in a single process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# several steps and a warm-up step, so that the dumping run's return to the
# seeded initial weights before its last timed step is exercised
STEPS, WARMUP = 3, 1


def _bench(tmp_path, device, dump, extra=()):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(REPO, "bench.py"),
           "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
           "--dataset", "tiny", "--device", device,
           "--partition-dir", str(tmp_path / "parts"),
           "--dump-outputs", str(tmp_path / dump)] + list(extra)
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600,
                         env=env, cwd=REPO)
    assert out.returncode == 0, f"stdout:\n{out.stdout}\nstderr:\n{out.stderr}"
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    arrays = {f[:-4]: np.load(tmp_path / dump / f)
              for f in sorted(os.listdir(tmp_path / dump))}
    return json.loads(lines[0]), arrays


def _check(tmp_path, device):
    res, a = _bench(tmp_path, device, "a")
    res_full, b = _bench(tmp_path, device, "b", extra=["--full"])
    for r in (res, res_full):
        for key in ("metric", "value", "unit", "higher_is_better", "dtype",
                    "ms_per_step"):
            assert key in r, key
        assert r["steps"] == STEPS and r["warmup"] == WARMUP
        assert r["unit"] == "edges/s" and r["higher_is_better"] is True
        assert r["ms_per_step"] > 0
        # value is edges / (seconds per timed step)
        assert r["value"] == pytest.approx(
            r["config"]["n_edges"] / (r["ms_per_step"] * 1e-3), rel=1e-9)
    assert set(a) == set(b) and "logits" in a and "loss" in a
    assert any(k.startswith("grad.") for k in a)
    assert sum(v.nbytes for v in a.values()) <= 64 * 10**6
    for k in a:
        assert a[k].dtype == np.float32, (k, a[k].dtype)
        assert a[k].shape == b[k].shape and a[k].size > 0, k
        assert np.isfinite(a[k]).all(), k
        # the last step starts from the seeded weights, so the two runs
        # differ by fp32 summation order at most: every element is a sum
        # of at most a few thousand terms no larger than the array's
        # largest, which bounds the difference by ~1000 eps of that scale
        scale = np.abs(a[k]).max()
        assert np.abs(a[k] - b[k]).max() <= 1e-4 * scale, k
    assert a["logits"].ndim == 2 and a["loss"].shape == (1,)


def test_bench_dump_outputs_and_full_cpu(tmp_path):
    _check(tmp_path, "cpu")


@pytest.mark.gpu
def test_bench_dump_outputs_and_full_gpu(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    _check(tmp_path, "cuda:0")


def test_bench_runs_from_read_only_directory(tmp_path):
    """Started from a directory it cannot write to, with the default
    --partition-dir, the benchmark keeps its partition store under the
    temporary directory instead of failing."""
    ro = tmp_path / "ro"
    ro.mkdir()
    scratch = tmp_path / "tmp"
    scratch.mkdir()
    ro.chmod(0o555)
    privileged = os.access(ro, os.W_OK)     # such a user writes anywhere
    env = dict(os.environ, TMPDIR=str(scratch))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    try:
        out = subprocess.run(
            [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
             "--steps", "1", "--warmup", "0", "--dataset", "tiny",
             "--device", "cpu"],
            capture_output=True, text=True, timeout=600, env=env, cwd=ro)
    finally:
        ro.chmod(0o755)
    assert out.returncode == 0, f"stdout:\n{out.stdout}\nstderr:\n{out.stderr}"
    res = json.loads([l for l in out.stdout.splitlines()
                      if l.startswith("{")][-1])
    assert res["steps"] == 1 and res["ms_per_step"] > 0
    if privileged:
        assert (ro / "bench_partition").is_dir()
    else:
        assert os.listdir(scratch) and not os.listdir(ro)
