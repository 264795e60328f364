"""bench.py as every change is measured: a plain run times one block of exactly --steps steps and prints the headline line only, and
--dump-outputs writes what the last timed step computed — the same files from run to run, since the inputs and the model are seeded."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"bench.py exited with {r.returncode}\n{r.stderr[-4000:]}"
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_plain_run_times_the_steps_asked_for_and_dumps_the_last_step(tmp_path):
    args = ["--gpus", "1", "--steps", "7", "--warmup", "2", "--batch", "32"]
    runs = [_bench(args + ["--dump-outputs", str(tmp_path / tag)]) for tag in ("a", "b")]
    for d in runs:
        assert d["steps"] == 7 and d["blocks"]["n"] == 1 and d["graph_capture_error"] is None and "HIP-graph" in d["config"]["execution"]
        assert d["metric"].startswith("molecules/s") and d["unit"] == "molecules/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        assert abs(d["value"] - 32 * 1e3 / d["ms_per_step"]) <= 1e-3 * d["value"]
        assert not {"eager", "roofline", "kernel_share", "forward_only", "with_input_pipeline", "cpu_baseline"} & d.keys()
    names = {"y_pred", "loss", "grad_flat", "params"}
    assert {f[:-4] for f in os.listdir(tmp_path / "a")} == names
    for n in names:
        x, y = np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy")
        assert x.dtype == np.float32 and x.shape == y.shape and x.size > 0 and np.isfinite(x).all(), n
        np.testing.assert_allclose(x, y, rtol=1e-4, atol=1e-5, err_msg=n)
    assert np.load(tmp_path / "a" / "y_pred.npy").shape == (32, 1)
    assert float(np.load(tmp_path / "a" / "loss.npy")[0]) == pytest.approx(runs[0]["loss"]["last"], rel=1e-6)
    # the gradient is the step's own, clipped to global norm 1 (Trainer(gradient_clip_val=1.0)) ...
    assert 0.0 < float(np.linalg.norm(np.load(tmp_path / "a" / "grad_flat.npy").astype(np.float64))) <= 1.0 + 1e-5
    # ... and the parameters are those after the last timed step: one step fewer leaves them one Adam step (lr 1e-4) behind
    _bench(["--gpus", "1", "--steps", "6", "--warmup", "2", "--batch", "32", "--dump-outputs", str(tmp_path / "c")])
    p7, p6 = np.load(tmp_path / "a" / "params.npy"), np.load(tmp_path / "c" / "params.npy")
    assert p7.shape == p6.shape and 0.0 < float(np.abs(p7 - p6).max()) < 1e-2
    assert not np.array_equal(np.load(tmp_path / "a" / "grad_flat.npy"), np.load(tmp_path / "c" / "grad_flat.npy"))
