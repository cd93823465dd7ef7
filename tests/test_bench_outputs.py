"""bench.py's plain / --full split and --dump-outputs, on the CPU (tiny model, in-process engine path)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parse(argv, monkeypatch):
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_measures_the_headline_phase_only(monkeypatch):
    plain = _parse(["--gpus", "1", "--steps", "7", "--warmup", "3"], monkeypatch)
    assert plain.phases == "reference" and not plain.full and plain.dump_outputs is None
    assert plain.steps == 7 and plain.warmup == 3
    full = _parse(["--gpus", "1", "--steps", "7", "--warmup", "3", "--full"], monkeypatch)
    assert full.phases == "reference,greedy" and full.full
    # an explicit list is kept either way
    assert _parse(["--phases", "greedy"], monkeypatch).phases == "greedy"
    assert _parse(["--phases", "greedy,reference", "--full"], monkeypatch).phases == "greedy,reference"


def _run(tmp_path, out_dir):
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="2")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--path", "engine", "--steps", "3",
           "--warmup", "1", "--concurrency", "4", "--prompt-len", "32", "--gen-len", "6", "--step-group", "2",
           "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_dump_outputs_cpu(tmp_path):
    """The dump is one float32 array, a row per probe request, the same in a second run with the same arguments;
    the result line is the plain one (its steps, ms_per_step from the window, no second phase)."""
    out = _run(tmp_path, tmp_path / "a")
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["config"]["window_engine_steps"] == 3 * 2 and "other_phases" not in out["config"]
    # ms_per_step is the window's time per step: value (tokens/s) x window seconds = the window's tokens
    tokens = out["config"]["window_output_tokens"]
    assert abs(out["ms_per_step"] * 3 / 1e3 * out["value"] - tokens) <= 0.01 * tokens + 1
    assert sorted(os.listdir(tmp_path / "a")) == ["logits.npy"]
    a = np.load(tmp_path / "a" / "logits.npy")
    assert a.dtype == np.float32 and a.ndim == 2 and a.shape[0] == 4 and 0 < a.shape[1] <= 8192
    assert a.nbytes <= 64 << 20 and np.isfinite(a).all()
    assert (np.abs(a).sum(axis=1) > 0).all()  # every probe request's row was recorded
    assert len({r.tobytes() for r in a}) == 4  # from its own prompt
    _run(tmp_path, tmp_path / "b")
    assert np.array_equal(a, np.load(tmp_path / "b" / "logits.npy"))
