"""The RCCL path of the training step, exercised on ONE GPU (the boxes of this pool have one): a fresh child process started through
torch.distributed.run — exactly how the driver starts the ranks of `bench.py --gpus N` — builds a 1-rank "nccl" (= RCCL) group and
runs the world > 1 step, graph A -> all_reduce of the flat gradient buffer -> graph B, because of --force-collective.
Reference: Lightning DDP of the training harness (conan_fgw/src/trainer.py:315-319; sampler data/datamodules.py:40-41)."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _run_child(cmd, env, tag):
    """Run a child to completion keeping EVERYTHING it and its ranks wrote: stdout / stderr go to files under gpurun_out/ (merged
    back from the GPU box) and are printed whole when the child fails — the abort message of a rank is in the middle of the stream,
    not in its last 2000 characters (round 3)."""
    logdir = os.path.join(ROOT, "gpurun_out", "rccl_tests")
    os.makedirs(logdir, exist_ok=True)
    fo, fe = os.path.join(logdir, tag + ".out"), os.path.join(logdir, tag + ".err")
    env = dict(env, TORCH_SHOW_CPP_STACKTRACES="1", NCCL_DEBUG="WARN", PYTHONFAULTHANDLER="1")
    with open(fo, "w") as o, open(fe, "w") as e:
        rc = subprocess.run(cmd, env=env, cwd=ROOT, stdout=o, stderr=e, timeout=900).returncode
    out, err = open(fo).read(), open(fe).read()
    assert rc == 0, f"child exited with {rc}\n---- stderr ({fe}) ----\n{err}\n---- stdout ({fo}) ----\n{out}"
    return out


def _bench(args, distributed, tag, nproc=1):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.pop("HSA_ENABLE_IPC_MODE_LEGACY", None)                  # bench.py must set it by itself before its first GPU call
    cmd = [sys.executable]
    if distributed:
        cmd += ["-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1", "--master-port", str(_free_port())]
    cmd += [os.path.join(ROOT, "bench.py"), "--full"] + args            # the collective's cost and the per-rank checks are --full figures
    out = _run_child(cmd, env, tag)
    line = [l for l in out.splitlines() if l.startswith("{")][-1]
    return json.loads(line)


def test_one_rank_rccl_step_runs_the_collective_and_matches_the_plain_step():
    common = ["--gpus", "1", "--steps", "5", "--warmup", "3", "--blocks", "3", "--no-cpu-baseline"]
    d = _bench(common + ["--force-collective"], distributed=True, tag="rccl1")
    assert d["rccl_ranks"] == 1 and d["n_gpus"] == 1
    assert d["allreduce_us"] is not None and d["allreduce_us"] > 0
    assert d["allreduce"]["in_timed_step"] and d["allreduce"]["calls_per_step"] == 1 and d["allreduce"]["forced"]
    assert d["graph_capture_error"] is None and "HIP-graph" in d["config"]["execution"]
    p = _bench(common, distributed=False, tag="plain")
    assert p["rccl_ranks"] == 0 and not p["allreduce"]["in_timed_step"]
    # same model, same batch, same seed: the loss after the same number of optimiser steps agrees (a 1-rank sum is the identity) ...
    assert abs(d["loss"]["last"] - p["loss"]["last"]) <= 1e-4 * abs(p["loss"]["last"]) + 1e-6
    # ... and one more call per step costs a few tens of microseconds, not a different step (boxes of this pool differ by ~4 %)
    assert d["ms_per_step"] <= 1.10 * p["ms_per_step"] + 0.05, (d["ms_per_step"], p["ms_per_step"])
    assert d["value"] >= 0.90 * p["value"] - 1.0


def test_one_rank_rccl_step_survives_slow_capture():
    """The round-3 abort: ProcessGroupNCCL's watchdog polls the end event of a collective that ran on the stream a HIP-graph capture
    then starts on (hipErrorCapturedEvent -> std::terminate).  TORCH_SHOW_CPP_STACKTRACES makes every C++ exception on the way cost about a
    second, which is what made the window certain on the driver's box; the child runs with it (see _run_child) and three times in a row."""
    for i in range(3):
        d = _bench(["--gpus", "1", "--steps", "3", "--warmup", "2", "--blocks", "1", "--no-cpu-baseline", "--force-collective"], distributed=True, tag=f"rccl1_rep{i}")
        assert d["graph_capture_error"] is None and d["allreduce"]["in_timed_step"]


def test_two_rank_step_end_to_end_on_one_gpu():
    """bench.py's world > 1 branch as the driver starts it (torch.distributed.run, 2 ranks), on the ONE GPU of this box: --backend gloo
    moves the flat gradient buffer through host memory, everything else is the real thing — per-rank shards (seed + 1000 * rank), graph A ->
    all-reduce -> graph B, barrier + MAX-over-ranks timing, rank-0-only JSON.  (datamodules.py:40-41, trainer.py:315-319.)"""
    d = _bench(["--gpus", "2", "--steps", "4", "--warmup", "2", "--blocks", "2", "--no-cpu-baseline", "--backend", "gloo", "--batch", "64"],
               distributed=True, tag="gloo2", nproc=2)
    assert d["n_gpus"] == 2 and d["dist"]["ranks"] == 2 and d["dist"]["backend"].startswith("gloo") and d["rccl_ranks"] == 0
    assert d["allreduce"]["in_timed_step"] and d["allreduce"]["calls_per_step"] == 1 and not d["allreduce"]["forced"]
    assert d["graph_capture_error"] is None and "HIP-graph" in d["config"]["execution"]
    assert d["config"]["parallelism"] == "dp2" and d["scaling"] == "weak"
    pr = d["dist"]["per_rank"]
    assert len(pr["loss"]) == 2 and pr["loss"][0] != pr["loss"][1]                       # different shards ...
    assert pr["parameter_checksum"][0] == pr["parameter_checksum"][1]                   # ... the same model after the same averaged updates
    assert d["value"] > 0 and abs(d["value"] - 2 * 64 * d["steps"] / (d["ms_per_step"] * 1e-3 * d["steps"])) <= 1e-3 * d["value"]


def test_eight_rank_dry_run_of_cfg3_on_one_gpu():
    """BASELINE.json configs[2] (Lipophilicity + SchNet, K=5, sharded over 8 ranks) as the driver would start it — `--config cfg3`, 8 ranks of
    torch.distributed.run — with the ranks sharing this box's one GPU over gloo and 16 molecules each instead of 128 (eight processes' worth of
    workspaces on one device): every rank captures and replays its own shard (N_max per rank, datamodules.py:40-41), one collective per step,
    identical parameters on all eight ranks afterwards, per-rank step times in the line.  A functional run of the 8-rank code path, not a rate."""
    d = _bench(["--gpus", "8", "--config", "cfg3", "--batch", "16", "--steps", "3", "--warmup", "2", "--blocks", "1", "--no-cpu-baseline", "--backend", "gloo"],
               distributed=True, tag="gloo8_cfg3", nproc=8)
    assert d["n_gpus"] == 8 and d["dist"]["ranks"] == 8 and d["config"]["parallelism"] == "dp8"
    assert "LIPO" in d["config"]["workload"] and d["config"]["molecules_per_gpu"] == 16 and d["config"]["max_nodes"] > 64      # the large-N FGW kernels
    assert d["allreduce"]["in_timed_step"] and d["allreduce"]["calls_per_step"] == 1
    assert d["graph_capture_error"] is None
    pr = d["dist"]["per_rank"]
    assert len(pr["loss"]) == 8 and len(set(pr["loss"])) == 8                            # eight different shards
    assert len(set(pr["parameter_checksum"])) == 1                                        # one model
    assert len(pr["ms_per_step"]) == 8 and pr["ms_per_step_min"] > 0 and d["allreduce_exposed_us"] is not None


def test_overlapped_buckets_with_deferred_weight_gradients():
    """2 ranks (gloo, both on cuda:0): FlatGradients.backward() with deferred weight gradients AND the overlapped early bucket.  The
    early-bucket hook must not mistake not-yet-accumulated siblings of a multi-output autograd node for copied gradients."""
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "_rank_probe_gpu.py")]
    out = _run_child(cmd, env, "probe2")
    d = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    assert d["error"] is None, d["error"]
    assert d["n_ranks"] == 2 and 0 < d["early"] < d["total"]
    assert all(n == 2 for n in d["launches"]), d["launches"]            # the early bucket really travelled on its own
