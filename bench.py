#!/usr/bin/env python3
"""Flagship benchmark: MNIST-784 3-layer MLP (784-256-256-10) synchronous
data-parallel training — the BASELINE.json headline metric
(samples/sec/node, weak scaling over 1/2/4/8 MI355X).

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N>1
launched via torch.distributed.run with one rank per GPU over RCCL.  W
untimed warmup steps, then exactly K timed steps bracketed by barrier +
synchronize on both sides; elapsed is MAX over ranks; rank 0 prints ONE JSON
line.  A plain run does only that: set up, warm up, time the K steps, print.
Every other measurement is chosen explicitly (``--mode``, ``--model``,
``--hipgraph``); ``--full`` is the switch for secondary measurements that ride
along with the headline run (none exist today, so it changes nothing yet).

``--dump-outputs DIR`` writes, after the timed steps, ``DIR/<name>.npy``
(float32, or float64 for integer buffers and the scalar losses).  Training
modes: ``loss``, what the last timed step returned, and ``ref.*``: loss,
gradients and weights of one more, untimed step that the same trainer takes
on the same batch after being rewound to its seeded initial state (see
``timed_path_outputs`` for why not the weights after the timed steps).
``--mode infer``: the logits of the last timed step.  Seeds are fixed, so the
inputs are identical from run to run with the same arguments.

The timed step is the full training step: zero -> fwd (fused MFMA linear+
relu) -> fused CE (loss+dlogits one kernel) -> bwd (MFMA dgrad/wgrad,
bucketed RCCL all-reduce overlapped with backward) -> fused Adam.  Synthetic
data (randn features, uniform labels), random-init weights, bf16 activations
with fp32 master weights & fp32 MFMA accumulation.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch
import torch.distributed as dist
import torch.nn as nn


DUMP_BUDGET_BYTES = 64 * 1000 * 1000  # cap on everything --dump-outputs writes


def initial_state(trainer) -> dict:
    """Copy of the trainer's weights and buffers, taken before the first step."""
    return {k: v.detach().clone() for k, v in trainer.model.state_dict().items()}


def timed_path_outputs(trainer, init_state, last_loss, x, y) -> dict:
    """What ``--dump-outputs`` writes for the training modes.

    ``loss``: the value the last timed ``train_step`` returned.

    ``ref.*``: the timed trainer itself — same object, buckets, optimizer,
    captured graph — is rewound in place to ``init_state`` with zeroed Adam
    moments and step counter, and takes one more, untimed ``train_step`` on the
    same batch; its loss, the gradients it leaves and the weights after it are
    written.  Anything the timed steps left behind in the trainer that a step
    should not depend on (stale buffers, missed zeroing, caches) shows here.

    The weights the timed steps end in are not written, because they do not
    repeat from run to run: the split-K wgrad, bias-grad and loss kernels
    accumulate with fp32 atomics, so one step repeats only to rounding (~3e-7
    on the weights), and Adam on this batch (random labels; the gradients are
    cancellation noise) multiplies that by orders of magnitude per step.  Two
    identical runs on one MI355X differ by 8% of the largest weight after 25
    steps; the loss still agrees to 2e-6 there and to 6e-4 after 200 steps.
    Collective when world > 1: every rank must call it."""
    opt = trainer.optimizer
    if opt is None or not hasattr(opt, "exp_avg"):
        raise RuntimeError("--dump-outputs rewinds the fused Adam state; no fused Adam on this trainer")
    with torch.no_grad():
        trainer.model.load_state_dict(init_state)
        opt.step_count = 0
        for t in list(opt.exp_avg) + list(opt.exp_avg_sq):
            t.zero_()
        if opt.step_dev is not None:
            opt.step_dev.zero_()
    ref_loss = trainer.train_step(x, y)
    outs = {"loss": torch.tensor([last_loss], dtype=torch.float64),
            "ref.loss": torch.tensor([ref_loss], dtype=torch.float64)}
    for k, p in trainer.model.named_parameters():
        if p.grad is not None:
            outs["ref.grad." + k] = p.grad
    for k, v in trainer.model.state_dict().items():
        outs["ref.state." + k] = v
    return outs


def dump_outputs(dirname: str, tensors: dict) -> None:
    """Write each tensor as ``dirname/<name>.npy``: float32 for floating
    tensors, float64 for float64/integer ones.  If the total would exceed
    DUMP_BUDGET_BYTES every array is cut to the same fraction of its elements,
    picked by a fixed-seed sample of the flattened array (sorted indices), so
    two runs dump the same positions."""
    import numpy as np

    os.makedirs(dirname, exist_ok=True)
    arrays = {}
    for name, t in tensors.items():
        t = t.detach()
        wide = t.dtype == torch.float64 or not t.dtype.is_floating_point
        arrays[name] = t.to("cpu", torch.float64 if wide else torch.float32).numpy()
    # .npy headers are ~128 bytes each; leave room for them
    budget = DUMP_BUDGET_BYTES - 256 * len(arrays)
    total = sum(a.nbytes for a in arrays.values())
    frac = min(1.0, budget / max(1, total))
    for i, (name, a) in enumerate(sorted(arrays.items())):
        if frac < 1.0 and a.size > 1:
            keep = max(1, int(a.size * frac))
            idx = np.sort(np.random.default_rng(i).choice(a.size, keep, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(dirname, name + ".npy"), np.ascontiguousarray(a))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=0,
                    help="per-GPU batch (weak scaling); 0 = per-model default "
                         "(mlp 2097152, cnn 131072, resnet18 2048 — measured sweet spots)")
    ap.add_argument("--device", type=str, default=None)
    ap.add_argument("--hipgraph", action="store_true", help="capture the train step in a HIP graph")
    ap.add_argument("--model", type=str, default="mnist_mlp",
                    choices=["mnist_mlp", "mnist_cnn", "resnet18"],
                    help="mnist_mlp = BASELINE flagship; mnist_cnn = examples/simple_cnn config; "
                         "resnet18 = BASELINE config 4 (synthetic 3x224x224)")
    ap.add_argument("--mode", type=str, default="train",
                    choices=["train", "infer", "time_to_loss", "fit"],
                    help="infer = saved-pipeline batch inference (HIP-graph forward); "
                         "time_to_loss = seconds of training until --target-loss on a "
                         "fixed synthetic batch (the BASELINE.json companion metric); "
                         "fit = estimator-path cost: the timed region starts from raw "
                         "per-row fp64 Vector rows (pinned staging + device cast ingest "
                         "included), then runs the training iterations")
    ap.add_argument("--target-loss", type=float, default=1.0)
    ap.add_argument("--max-steps", type=int, default=2000)
    ap.add_argument("--full", action="store_true",
                    help="also run the secondary measurements that accompany the "
                         "headline figure (none today: a plain run is already only "
                         "setup, warmup, the timed steps and the result line)")
    ap.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                    help="after the timed steps write DIR/<name>.npy: the last timed "
                         "step's loss, plus loss, gradients and weights of one more "
                         "untimed step of the same trainer rewound to its seeded "
                         "initial state (training modes); the last step's logits "
                         "(--mode infer)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")

    if args.mode == "fit" and args.batch == 0 and args.model == "mnist_mlp":
        # fit mode materializes per-row fp64 Vector objects; 131072 rows is
        # the BASELINE config-2 partition size (the 2M sweet-spot batch would
        # spend minutes just building python row objects)
        args.batch = 131072

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))

    on_gpu = torch.cuda.is_available() if args.device is None else args.device.startswith("cuda")
    if on_gpu:
        torch.cuda.set_device(local_rank % max(1, torch.cuda.device_count()))
        device = "cuda:%d" % (local_rank % max(1, torch.cuda.device_count()))
    else:
        device = "cpu"

    if world > 1:
        dist.init_process_group("nccl" if on_gpu else "gloo")

    from sparktorch_amd.parallel.sync import SyncTrainer

    torch.manual_seed(1234)  # identical initial weights on every rank
    if args.model == "mnist_cnn":
        if args.batch == 0:
            args.batch = 131072
        if on_gpu:
            from sparktorch_amd.ops.modules import MnistCNNFused

            model = MnistCNNFused()
        else:
            from sparktorch_amd.models.mnist import MnistCNN

            model = MnistCNN()
    elif args.model == "resnet18":
        if args.batch == 0:
            args.batch = 2048
        if on_gpu:
            from sparktorch_amd.ops.modules import ResNet18Fused

            model = ResNet18Fused()
        else:
            from sparktorch_amd.models.resnet import ResNet18

            model = ResNet18()
    elif on_gpu:
        if args.batch == 0:
            args.batch = 2097152
        from sparktorch_amd.ops.modules import MnistMLPFused

        model = MnistMLPFused()
    else:
        if args.batch == 0:
            args.batch = 8192  # CPU-sized
        from sparktorch_amd.models.mnist import MnistMLP

        model = MnistMLP()

    if args.mode == "infer":
        return run_infer(args, model, device, on_gpu)
    if args.mode == "time_to_loss":
        return run_time_to_loss(args, model, device, on_gpu, world, rank)
    if args.mode == "fit":
        return run_fit(args, model, device, on_gpu, world, rank)

    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    trainer = SyncTrainer(
        model,
        nn.CrossEntropyLoss(),
        opt,
        device=device,
        world_size=world,
        compile_mode="hipgraph" if (args.hipgraph and world == 1 and on_gpu) else None,
    )

    in_dim = 3 * 224 * 224 if args.model == "resnet18" else 784
    n_classes = 1000 if args.model == "resnet18" else 10
    torch.manual_seed(1234 + rank)  # rank-local data shard
    x = torch.randn(args.batch, in_dim, device=device)
    if on_gpu:
        x = x.to(torch.bfloat16)
    y = torch.randint(0, n_classes, (args.batch,), device=device)

    def barrier_sync():
        if world > 1:
            dist.barrier()
        if on_gpu:
            torch.cuda.synchronize()

    init_state = initial_state(trainer) if args.dump_outputs else None
    for _ in range(args.warmup):
        trainer.train_step(x, y)

    barrier_sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = trainer.train_step(x, y)
    barrier_sync()
    elapsed = time.perf_counter() - t0

    if args.dump_outputs:
        outs = timed_path_outputs(trainer, init_state, loss, x, y)
        if rank == 0:
            dump_outputs(args.dump_outputs, outs)

    # max over ranks
    if world > 1:
        et = torch.tensor([elapsed], device=device if on_gpu else "cpu")
        dist.all_reduce(et, op=dist.ReduceOp.MAX)
        elapsed = float(et)

    n_gpus = world if world > 1 else (args.gpus if on_gpu else 1)
    total_samples = args.batch * n_gpus * args.steps
    samples_per_sec = total_samples / elapsed
    ms_per_step = elapsed / args.steps * 1000.0

    if rank == 0:
        out = {
            "metric": "samples_per_sec",
            "value": samples_per_sec,
            "unit": "samples/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,  # reference publishes no numbers
            "dtype": "bf16" if on_gpu else "fp32",
            "data": "synthetic",
            "config": {
                "model": {"mnist_mlp": "mnist_mlp_784x256x256x10",
                          "mnist_cnn": "mnist_cnn_conv16x5_conv32x3_fc3872x10",
                          "resnet18": "resnet18_3x224x224_1000cls"}[args.model],
                "global_batch": args.batch * n_gpus,
                "seq_len": None,
                "parallelism": "dp%d" % n_gpus,
                "optimizer": "fused_adam",
                "loss": "cross_entropy_fused",
                "hipgraph": bool(args.hipgraph),
            },
        }
        print(json.dumps(out), flush=True)

    if world > 1:
        dist.destroy_process_group()
    return 0


def run_fit(args, model, device, on_gpu, world, rank) -> int:
    """Estimator-path cost (BASELINE config 2 as fit() sees it): the timed
    region covers what a barrier task pays after receiving its partition —
    per-row fp64 Vector ingest (np.stack gather -> pinned staging ->
    hipMemcpyAsync -> on-device cast, utils.data.handle_features_device) plus
    ``--steps`` training iterations.  Shows the pack is not the bottleneck."""
    import numpy as np

    from sparktorch_amd.parallel.sync import SyncTrainer
    from sparktorch_amd.utils.data import handle_features, handle_features_device
    from sparktorch_amd.utils.serialize import DataObj

    in_dim = 3 * 224 * 224 if args.model == "resnet18" else 784
    n_classes = 1000 if args.model == "resnet18" else 10
    rng = np.random.default_rng(1234 + rank)
    # Spark-shaped partition: one fp64 vector per row (DenseVector.toArray)
    feat_mat = rng.standard_normal((args.batch, in_dim))  # fp64
    labels = rng.integers(0, n_classes, args.batch)
    rows = [DataObj(feat_mat[i], float(labels[i]), None, None) for i in range(args.batch)]

    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    trainer = SyncTrainer(model, nn.CrossEntropyLoss(), opt, device=device, world_size=world)
    init_state = initial_state(trainer) if args.dump_outputs else None

    def ingest():
        if on_gpu:
            return handle_features_device(rows, 0.0, device=device)
        return handle_features(rows, 0.0)

    # warmup: full ingest + warmup steps (allocator, kernels, autograd graphs)
    d = ingest()
    x, y = d.x_train, d.y_train
    if not on_gpu:
        x, y = x.to(device), y.to(device)
    for _ in range(args.warmup):
        trainer.train_step(x, y)

    if world > 1:
        dist.barrier()
    if on_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    d = ingest()
    x, y = d.x_train, d.y_train
    if not on_gpu:
        x, y = x.to(device), y.to(device)
    if on_gpu:
        torch.cuda.synchronize()
    t_ingest = time.perf_counter() - t0
    for _ in range(args.steps):
        loss = trainer.train_step(x, y)
    if world > 1:
        dist.barrier()
    if on_gpu:
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0

    if args.dump_outputs:
        outs = timed_path_outputs(trainer, init_state, loss, x, y)
        if rank == 0:
            dump_outputs(args.dump_outputs, outs)

    if world > 1:
        et = torch.tensor([elapsed], device=device if on_gpu else "cpu")
        dist.all_reduce(et, op=dist.ReduceOp.MAX)
        elapsed = float(et)

    n_gpus = world if world > 1 else (args.gpus if on_gpu else 1)
    if rank == 0:
        print(json.dumps({
            "metric": "fit_samples_per_sec",
            "value": args.batch * n_gpus * args.steps / elapsed,
            "unit": "samples/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1000.0,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16" if on_gpu else "fp32",
            "data": "synthetic",
            "config": {"model": args.model, "global_batch": args.batch * n_gpus,
                       "seq_len": None, "parallelism": "dp%d" % n_gpus,
                       "ingest_ms": t_ingest * 1000.0,
                       "ingest_included_in_timed_region": True},
        }), flush=True)
    if world > 1:
        dist.destroy_process_group()
    return 0


def run_time_to_loss(args, model, device, on_gpu, world, rank) -> int:
    """Train on one fixed synthetic batch until loss < target; report wall
    seconds (strong-scaling companion to the throughput metric)."""
    from sparktorch_amd.parallel.sync import SyncTrainer

    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    trainer = SyncTrainer(model, nn.CrossEntropyLoss(), opt, device=device, world_size=world)
    init_state = initial_state(trainer) if args.dump_outputs else None
    in_dim = 3 * 224 * 224 if args.model == "resnet18" else 784
    n_classes = 1000 if args.model == "resnet18" else 10
    torch.manual_seed(1234 + rank)
    x = torch.randn(args.batch, in_dim, device=device)
    if on_gpu:
        x = x.to(torch.bfloat16)
    y = torch.randint(0, n_classes, (args.batch,), device=device)

    trainer.train_step(x, y)  # warmup/compile outside the clock
    if on_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    steps = 0
    loss = float("inf")
    while steps < args.max_steps:
        loss = trainer.train_step(x, y)
        steps += 1
        if world > 1:
            # collective stop: every rank must take the same branch or the
            # next step's all-reduce deadlocks (rank-seeded data -> local
            # losses differ); stop only when the WORST rank hits target
            lt = torch.tensor([loss], device=device if on_gpu else "cpu")
            dist.all_reduce(lt, op=dist.ReduceOp.MAX)
            loss = float(lt)
        if loss < args.target_loss:
            break
    if on_gpu:
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs:
        outs = timed_path_outputs(trainer, init_state, loss, x, y)
        if rank == 0:
            dump_outputs(args.dump_outputs, outs)
    if rank == 0:
        print(json.dumps({
            "metric": "time_to_loss_s",
            "value": elapsed,
            "unit": "s",
            "n_gpus": world if world > 1 else 1,
            "steps": steps,
            "warmup": 1,
            "ms_per_step": elapsed / max(1, steps) * 1000.0,
            "higher_is_better": False,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "bf16" if on_gpu else "fp32",
            "data": "synthetic",
            "config": {"model": args.model, "global_batch": args.batch,
                       "target_loss": args.target_loss, "reached": loss < args.target_loss,
                       "final_loss": loss, "seq_len": None,
                       "parallelism": "dp%d" % (world if world > 1 else 1)},
        }), flush=True)
    if world > 1:
        dist.destroy_process_group()
    return 0


def run_infer(args, model, device, on_gpu) -> int:
    """Saved-pipeline batch inference benchmark (BASELINE config 5): batched
    mapPartitions forward, HIP-graph captured and replayed per batch."""
    import json as _json

    model = model.to(device).eval()
    bs = args.batch
    in_dim = 3 * 224 * 224 if args.model == "resnet18" else 784
    x = torch.randn(bs, in_dim, device=device)
    if on_gpu:
        from sparktorch_amd.ops.graph import GraphedForward

        runner = GraphedForward(model, device=device, batch_size=bs)
        x = x.to(torch.bfloat16)

        def step():
            return runner.replay_device(x)
        step()  # capture
    else:
        def step():
            with torch.no_grad():
                return model(x)

    for _ in range(args.warmup):
        step()
    if on_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        logits = step()
    if on_gpu:
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"logits": logits})
    out = {
        "metric": "inference_samples_per_sec",
        "value": bs * args.steps / elapsed,
        "unit": "samples/s",
        "n_gpus": 1,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1000.0,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "bf16" if on_gpu else "fp32",
        "data": "synthetic",
        "config": {"model": args.model, "global_batch": bs, "seq_len": None,
                   "parallelism": "dp1", "hipgraph": bool(on_gpu)},
    }
    print(_json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
