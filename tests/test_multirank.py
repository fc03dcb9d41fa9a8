"""Multi-rank (world 4 / 8) correctness over gloo, CPU-only.

Proves the properties the round-end 8-GPU SCALE run depends on, without any
GPU: (1) every rank finishes with a bit-identical state_dict (the reference's
implicit invariant — it collects all ranks' states and takes [0],
reference distributed.py:255-261); (2) the distributed result agrees with a
single-process run on the concatenated data (grad-averaging semantics);
(3) bucket all-reduce launch order is deterministic and identical across
ranks and steps; (4) the torchrun/bench.py contract works at world>1 over
gloo (the exact launch shape the driver uses for SCALE).
"""

from __future__ import annotations

import json
import os
import socket
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(REPO, "tests", "multirank_worker.py")


def _free_port() -> int:
    s = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_world(world: int, outdir: str, steps: int = 5, timeout: float = 420.0) -> None:
    port = _free_port()
    procs = [
        subprocess.Popen(
            [sys.executable, WORKER, "--rank", str(r), "--world", str(world),
             "--port", str(port), "--outdir", outdir, "--steps", str(steps)],
            cwd=REPO,
        )
        for r in range(world)
    ]
    codes = [p.wait(timeout=timeout) for p in procs]
    assert codes == [0] * world, "worker exit codes: %r" % codes


@pytest.mark.parametrize("world", [4, 8])
def test_world_n_states_bitwise_identical(world, tmp_path):
    outdir = str(tmp_path)
    _run_world(world, outdir)

    states = [torch.load(os.path.join(outdir, "state_%d.pt" % r)) for r in range(world)]
    ref = states[0]
    for r in range(1, world):
        assert set(states[r]) == set(ref)
        for k in ref:
            assert torch.equal(states[r][k], ref[k]), (
                "rank %d state %r differs from rank 0" % (r, k)
            )

    # launch order: identical across ranks, identical across steps
    orders = [json.load(open(os.path.join(outdir, "order_%d.json" % r))) for r in range(world)]
    n_buckets = orders[0]["n_buckets"]
    assert n_buckets >= 3, "test wants a multi-bucket model, got %d" % n_buckets
    seq0 = orders[0]["order"]
    per_step = len(seq0) // 5
    assert per_step == n_buckets, "every bucket should launch exactly once per step"
    assert seq0[:per_step] * 5 == seq0, "launch order must not vary across steps"
    for r in range(1, world):
        assert orders[r]["order"] == seq0, "rank %d launch order differs" % r

    # losses agree across ranks only AFTER the first sync (same model, own
    # shard -> per-rank loss values differ; just sanity-check they are finite)
    for r in range(world):
        losses = json.load(open(os.path.join(outdir, "losses_%d.json" % r)))
        assert all(l == l and abs(l) < 1e6 for l in losses)


def test_world4_agrees_with_single_process(tmp_path):
    """Distributed grad averaging == single-process full-batch on the
    concatenated shards (equal shard sizes -> mean of shard-means = global
    mean)."""
    import torch.nn as nn

    from sparktorch_amd.parallel.sync import SyncTrainer
    from tests.multirank_worker import build_model, shard

    world = 4
    outdir = str(tmp_path)
    _run_world(world, outdir)
    dist_state = torch.load(os.path.join(outdir, "state_0.pt"))

    model = build_model()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    trainer = SyncTrainer(model, nn.MSELoss(), opt, device="cpu", world_size=1)
    xs, ys = zip(*(shard(r) for r in range(world)))
    x = torch.cat(xs)
    y = torch.cat(ys)
    for _ in range(5):
        trainer.train_step(x, y)
    single_state = trainer.state_dict_cpu()

    assert set(single_state) == set(dist_state)
    for k in single_state:
        assert torch.allclose(single_state[k], dist_state[k], atol=2e-5, rtol=1e-4), (
            "param %r: max diff %g"
            % (k, (single_state[k] - dist_state[k]).abs().max().item())
        )


@pytest.mark.parametrize("world", [2, 4, 8])
def test_bench_torchrun_contract_gloo(world, tmp_path):
    """The exact launch the driver uses for SCALE_rNN.json, on CPU/gloo:
    torch.distributed.run -> bench.py --gpus N; rank 0 must print one valid
    JSON line with the whole-job aggregate."""
    port = _free_port()
    proc = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run",
         "--nnodes=1", "--nproc-per-node", str(world),
         "--master-addr", "127.0.0.1", "--master-port", str(port),
         os.path.join(REPO, "bench.py"),
         "--gpus", str(world), "--steps", "3", "--warmup", "1", "--batch", "512",
         "--device", "cpu"],  # gloo also where a GPU is visible (one card, N ranks)
        capture_output=True,
        text=True,
        timeout=420,
        cwd=REPO,
    )
    assert proc.returncode == 0, proc.stdout + "\n" + proc.stderr
    line = next(l for l in proc.stdout.splitlines() if l.startswith("{"))
    out = json.loads(line)
    assert out["n_gpus"] == world
    assert out["steps"] == 3
    assert out["config"]["parallelism"] == "dp%d" % world
    assert out["config"]["global_batch"] == 512 * world
    assert out["value"] > 0


def test_bench_time_to_loss_world2_no_deadlock(tmp_path):
    """time_to_loss at world>1: ranks see different data, so the stop
    decision must be collective — a rank breaking on its local loss would
    leave the others deadlocked in the next all-reduce.  Runs the real
    torchrun launch on gloo."""
    port = _free_port()
    proc = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run",
         "--nnodes=1", "--nproc-per-node", "2",
         "--master-addr", "127.0.0.1", "--master-port", str(port),
         os.path.join(REPO, "bench.py"),
         "--mode", "time_to_loss", "--batch", "1024",
         "--max-steps", "30", "--target-loss", "2.1",
         "--device", "cpu"],  # gloo also where a GPU is visible (one card, 2 ranks)
        capture_output=True,
        text=True,
        timeout=420,
        cwd=REPO,
    )
    assert proc.returncode == 0, proc.stdout + "\n" + proc.stderr
    line = next(l for l in proc.stdout.splitlines() if l.startswith("{"))
    out = json.loads(line)
    assert out["metric"] == "time_to_loss_s"
    assert out["n_gpus"] == 2
    assert out["config"]["parallelism"] == "dp2"
