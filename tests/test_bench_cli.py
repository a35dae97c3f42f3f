"""bench.py command-line contract: --steps really sets the timed steps, the
result line carries ms_per_step, a plain run has no extras, and
--dump-outputs writes the last step's result reproducibly."""
import json
import os
import subprocess
import sys

import pytest

np = pytest.importorskip("numpy")
pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, timeout=180):
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1"] + args,
        capture_output=True, text=True, timeout=timeout, cwd=REPO,
    )
    assert r.returncode == 0, f"bench failed:\n{r.stdout}\n{r.stderr}"
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_tiny_run_dumps_last_step(tmp_path):
    outs = []
    for name in ("a", "b"):
        d = tmp_path / name
        j = _bench(["--steps", "7", "--warmup", "2", "--dump-outputs", str(d)])
        assert j["steps"] == 7 and j["warmup"] == 2
        assert j["metric"] == "cross_party_objects_per_sec"
        assert j["ms_per_step"] > 0
        # value = 2 transfers per step / seconds per step
        assert j["value"] == pytest.approx(2000.0 / j["ms_per_step"], rel=1e-2)
        assert "extras" not in j["config"]
        assert sorted(os.listdir(d)) == ["last_step_result.npy"]
        outs.append(np.load(d / "last_step_result.npy"))
    assert outs[0].dtype == np.float64
    # Two parties each contribute 1; the aggregate is what fed.get returns.
    assert outs[0].tolist() == [2.0]
    assert outs[1].tolist() == outs[0].tolist()


def test_data_mode_honours_explicit_steps(tmp_path):
    """An explicit --steps above 50 used to be clamped to 10 in push mode."""
    j = _bench(["--mode", "push", "--push-gib", "0.001", "--steps", "60",
                "--warmup", "1", "--dump-outputs", str(tmp_path)])
    assert j["steps"] == 60
    nbytes = (int(0.001 * (1 << 30)) // 2) * 2
    assert j["value"] == pytest.approx(
        nbytes / (j["ms_per_step"] * 1e-3) / 1e9, rel=1e-2
    )
    out = np.load(tmp_path / "last_step_result.npy")
    assert out.tolist() == [float(nbytes)]
