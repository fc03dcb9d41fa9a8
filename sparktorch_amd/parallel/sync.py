"""Synchronous data-parallel training engine.

Re-design of the reference's sync engine (distributed.py:66-261) for MI355X:

* one worker process = one rank = one GPU; RCCL (``"nccl"`` on ROCm) over
  xGMI instead of gloo whenever the device is a GPU;
* gradients live in flat ~25 MB buckets whose all-reduce launches the moment
  the bucket's grads are complete, overlapping with the rest of backward
  (:mod:`sparktorch_amd.parallel.buckets`) — vs one blocking per-parameter
  all-reduce in the reference (distributed.py:179-181);
* the optimizer is a fused flat-bucket HIP kernel when on GPU
  (:mod:`sparktorch_amd.ops.optim`), folding the 1/world grad averaging into
  the update instead of a separate divide pass;
* ``compileMode`` is honored (the reference's torch.compile call is broken —
  distributed.py:117-118 tests the *builtin* ``compile``); mode
  ``"hipgraph"`` captures the whole train step in a HIP graph and replays it.

Reference behaviors preserved: long-label retry for classification criteria
(distributed.py:152-157), autoencoder mode when no labels (distributed.py:136),
minibatch sampling (distributed.py:145-148), early-stop consensus — one loss
all-reduce per iteration; every rank derives the same stop decision from the
identical reduced value (vs two collectives at distributed.py:184-196) —
identical final states on every rank.
"""

from __future__ import annotations

import random
from typing import Any, Iterable, List, Optional

import numpy as np
import torch
import torch.distributed as dist

from sparktorch_amd.compat.barrier import get_barrier_context
from sparktorch_amd.parallel.buckets import FlatBuckets
from sparktorch_amd.parallel.rendezvous import (
    cleanup_stale_process_group,
    init_process_group_from_barrier,
    pick_device,
)
from sparktorch_amd.utils.data import handle_features, handle_features_device
from sparktorch_amd.utils.early_stopper import EarlyStopping
from sparktorch_amd.utils.sampling import DeviceMinibatchSampler
from sparktorch_amd.utils.trace import StepMetrics, trace_range
from sparktorch_amd.utils.serialize import (
    load_base_torch,
    load_torch_model,
    serialize_torch_obj,
)


def compute_loss(criterion, pred: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """Criterion with the reference's long-label retry (distributed.py:152-157):
    classification losses want int64 class targets."""
    cname = type(criterion).__name__
    if cname in ("HipCrossEntropy", "HipMSE"):
        return criterion(pred, y)  # fused losses handle their own casts
    if cname in ("CrossEntropyLoss", "NLLLoss") or isinstance(
        criterion, (torch.nn.CrossEntropyLoss, torch.nn.NLLLoss)
    ):
        return criterion(pred, y.flatten().long())
    try:
        return criterion(pred, y.float() if y.dtype != pred.dtype else y)
    except RuntimeError:
        return criterion(pred, y.flatten().long())


class SyncTrainer:
    """One rank's training state: model + flat buckets + (fused) optimizer.

    Usable both from barrier workers (``handle_model``) and directly from
    torchrun-launched benchmark ranks.
    """

    def __init__(
        self,
        model: torch.nn.Module,
        criterion,
        torch_optimizer: torch.optim.Optimizer,
        device: str = "cpu",
        world_size: Optional[int] = None,
        bucket_cap_mb: float = 25.0,
        compile_mode: Optional[str] = None,
    ):
        self.device = device
        self.model = model.to(device)
        self.criterion = criterion
        self.native = device.startswith("cuda")
        if self.native:
            # GPU: the hand-written MFMA/fused-kernel path is mandatory —
            # fail loudly rather than silently running eager torch.
            from sparktorch_amd import ops as _ops

            _ops.ext()
            from sparktorch_amd.ops.modules import (
                convert_criterion_for_mi355x,
                convert_model_for_mi355x,
            )

            self.model = convert_model_for_mi355x(self.model)
            self.criterion = convert_criterion_for_mi355x(self.criterion)
        self.world_size = (
            world_size
            if world_size is not None
            else (dist.get_world_size() if dist.is_initialized() else 1)
        )

        self.buckets = FlatBuckets(
            list(self.model.parameters()), bucket_cap_mb=bucket_cap_mb, world_size=self.world_size
        )
        self.buckets.register_hooks()

        from sparktorch_amd.ops.optim import fused_optimizer_for

        self.optimizer = fused_optimizer_for(torch_optimizer, self.buckets)
        self._torch_opt = None
        if self.optimizer is None:
            # No fused mapping: rebuild the torch optimizer on the re-bound
            # (flattened) parameters; averaging happens in finalize().
            # Param groups (and settings edited in them after construction)
            # carry over when the model still holds the optimizer's very
            # parameters; a conversion that replaced them leaves only the
            # constructor defaults to go by.
            live = {id(p) for p in self.model.parameters()}
            groups = torch_optimizer.param_groups
            if groups and all(id(p) in live for g in groups for p in g["params"]) and sum(
                len(g["params"]) for g in groups
            ) == len(live):
                self._torch_opt = type(torch_optimizer)(
                    [dict(g) for g in groups], **torch_optimizer.defaults
                )
            else:
                self._torch_opt = type(torch_optimizer)(
                    self.model.parameters(), **torch_optimizer.defaults
                )

        self._graph = None
        self._graph_inputs = None
        self._sampled_graph = None  # (sampler, graph, static loss)
        self.compile_mode = compile_mode
        if compile_mode and compile_mode not in ("hipgraph",):
            # Correct implementation of the reference's broken torch.compile
            # hook (distributed.py:117-118).
            self.model = torch.compile(self.model, mode=compile_mode)

    # ------------------------------------------------------------------
    def _forward_backward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        # A model that offers the explicit forward + cross-entropy + backward
        # step (MnistMLPFused.ce_step) takes it when the loss is the fused
        # cross-entropy and every gradient goes straight into its bucket view:
        # the head's forward, the loss and the head's backward are one kernel.
        if (
            self.native
            and type(self.criterion).__name__ == "HipCrossEntropy"
            and (not self.compile_mode or self.compile_mode == "hipgraph")
            and y is not None
            and hasattr(self.model, "ce_step_supported")
            and self.model.ce_step_supported(x)
        ):
            return self.model.ce_step(x, y)
        pred = self.model(x)
        loss = compute_loss(self.criterion, pred, y)
        loss.backward()
        return loss

    def train_step(self, x: torch.Tensor, y: torch.Tensor) -> float:
        """zero -> fwd -> bwd (all-reduce overlapped) -> finalize -> step."""
        if self.compile_mode == "hipgraph" and x.is_cuda:
            return self._train_step_graphed(x, y)
        self.buckets.zero_grad()
        loss = self._forward_backward(x, y)
        if self.optimizer is not None:
            self.buckets.finalize(average=False)  # scale fused into the update
            self.optimizer.step(grad_scale=1.0 / self.world_size)
        else:
            self.buckets.finalize(average=True)
            self._torch_opt.step()
        return float(loss.detach())

    # ------------------------------------------------------------------
    def _train_step_graphed(self, x: torch.Tensor, y: torch.Tensor) -> float:
        """Whole-step HIP-graph capture and replay (compileMode='hipgraph').

        The step (zero + fwd + bwd + fused step) is captured once per input
        shape and replayed thereafter — removes every launch gap in
        launch-bound small-model training.  Collectives are NOT captured;
        graph mode therefore requires world_size == 1 or external averaging.
        """
        key = (tuple(x.shape), tuple(y.shape) if y is not None else None)
        if self._graph is None or self._graph_inputs[0] != key:
            if self.world_size > 1:
                raise RuntimeError(
                    "compileMode='hipgraph' currently supports world_size==1 "
                    "(collectives are not graph-captured)"
                )
            static_x = x.clone()
            static_y = y.clone() if y is not None else None
            # Warmup steps REALLY execute (capture itself records without
            # executing) — snapshot the training state so the first replay
            # starts exactly where eager would.
            snap_params = [b.flat_param.clone() for b in self.buckets.buckets]
            # module buffers mutate during the 2 real warmup steps too
            # (BatchNorm running stats / num_batches_tracked)
            snap_buffers = {k: v.clone() for k, v in self.model.named_buffers()}
            snap_opt = None
            if self.optimizer is not None:
                sd = getattr(self.optimizer, "step_dev", None)
                snap_opt = (
                    self.optimizer.step_count,
                    [t.clone() for t in getattr(self.optimizer, "exp_avg", [])],
                    [t.clone() for t in getattr(self.optimizer, "exp_avg_sq", [])],
                    [t.clone() if t is not None else None
                     for t in getattr(self.optimizer, "momentum_buf", [])],
                    sd.clone() if sd is not None else None,
                )
            # warmup on a side stream (required before capture)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(2):
                    self.buckets.zero_grad()
                    loss = self._forward_backward(static_x, static_y)
                    if self.optimizer is not None:
                        self.optimizer.step(grad_scale=1.0)
                    else:
                        self._torch_opt.step()
            torch.cuda.current_stream().wait_stream(s)
            g = torch.cuda.CUDAGraph()
            static_loss = torch.zeros((), device=x.device)
            with torch.cuda.graph(g):
                self.buckets.zero_grad()
                loss = self._forward_backward(static_x, static_y)
                static_loss.copy_(loss.detach())
                if self.optimizer is not None:
                    self.optimizer.step(grad_scale=1.0)
                else:
                    self._torch_opt.step()
            # restore pre-warmup state (the capture pass records, it does
            # not execute — only the 2 warmup steps mutated anything)
            for b, p0 in zip(self.buckets.buckets, snap_params):
                b.flat_param.copy_(p0)
            for k, v in self.model.named_buffers():
                v.copy_(snap_buffers[k])
            if snap_opt is not None:
                self.optimizer.step_count = snap_opt[0]
                for t, t0 in zip(getattr(self.optimizer, "exp_avg", []), snap_opt[1]):
                    t.copy_(t0)
                for t, t0 in zip(getattr(self.optimizer, "exp_avg_sq", []), snap_opt[2]):
                    t.copy_(t0)
                for t, t0 in zip(getattr(self.optimizer, "momentum_buf", []), snap_opt[3]):
                    if t is not None and t0 is not None:
                        t.copy_(t0)
                sd = getattr(self.optimizer, "step_dev", None)
                if sd is not None and snap_opt[4] is not None:
                    sd.copy_(snap_opt[4])
            self._graph = g
            self._graph_inputs = (key, static_x, static_y, static_loss)
        _, static_x, static_y, static_loss = self._graph_inputs
        static_x.copy_(x)
        if static_y is not None:
            static_y.copy_(y)
        self._graph.replay()
        return float(static_loss)

    # ------------------------------------------------------------------
    def _step_body(self, x: torch.Tensor, y: torch.Tensor, grad_scale: float) -> torch.Tensor:
        self.buckets.zero_grad()
        loss = self._forward_backward(x, y)
        if self.optimizer is not None:
            self.buckets.finalize(average=False)  # scale fused into the update
            self.optimizer.step(grad_scale=grad_scale)
        else:
            self.buckets.finalize(average=True)
            self._torch_opt.step()
        return loss

    def train_step_sampled(self, sampler) -> float:
        """One step on the next minibatch of a
        :class:`~sparktorch_amd.utils.sampling.DeviceMinibatchSampler`.

        Eager: draw + gather, then the body of :meth:`train_step`.  With
        ``compile_mode='hipgraph'`` on a GPU the draw, the gather and the
        sampler's counter increment are captured together with zero + fwd +
        bwd + fused step, so an iteration is one graph replay plus the loss
        read and the host chooses nothing."""
        if self.compile_mode == "hipgraph" and sampler.native:
            return self._train_step_sampled_graphed(sampler)
        xb, yb = sampler.next()
        return float(self._step_body(xb, yb, 1.0 / self.world_size).detach())

    def _train_step_sampled_graphed(self, sampler) -> float:
        if self._sampled_graph is None or self._sampled_graph[0] is not sampler:
            if self.world_size > 1:
                raise RuntimeError(
                    "compileMode='hipgraph' currently supports world_size==1 "
                    "(collectives are not graph-captured)"
                )
            # As in _train_step_graphed: the two warmup steps really execute,
            # so everything they mutate is put back before the first replay —
            # here also the sampler's counter, or they would consume draws.
            snap = [(t, t.clone()) for t in self._mutable_state()]
            snap.append((sampler.step_dev, sampler.step_dev.clone()))
            step_count = self.optimizer.step_count if self.optimizer is not None else None

            def whole_step():
                xb, yb = sampler.next()
                return self._step_body(xb, yb, 1.0)

            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(2):
                    whole_step()
            torch.cuda.current_stream().wait_stream(s)
            g = torch.cuda.CUDAGraph()
            static_loss = torch.zeros((), device=sampler.step_dev.device)
            with torch.cuda.graph(g):
                static_loss.copy_(whole_step().detach())
            for t, t0 in snap:
                t.copy_(t0)
            if step_count is not None:
                self.optimizer.step_count = step_count
            self._sampled_graph = (sampler, g, static_loss)
        _, g, static_loss = self._sampled_graph
        g.replay()
        if self.optimizer is not None:
            self.optimizer.step_count += 1  # host mirror of the device counter
        return float(static_loss)

    def _mutable_state(self) -> List[torch.Tensor]:
        """Every tensor a train step writes and the next one reads."""
        state = [b.flat_param for b in self.buckets.buckets]
        state += [v for _, v in self.model.named_buffers()]
        if self.optimizer is not None:
            for name in ("exp_avg", "exp_avg_sq", "momentum_buf"):
                state += [t for t in getattr(self.optimizer, name, []) if t is not None]
            sd = getattr(self.optimizer, "step_dev", None)
            if sd is not None:
                state.append(sd)
        else:
            for st in self._torch_opt.state.values():
                state += [t for t in st.values() if torch.is_tensor(t)]
        return state

    # ------------------------------------------------------------------
    @torch.no_grad()
    def validation_loss(self, x_val: torch.Tensor, y_val: torch.Tensor) -> float:
        self.model.eval()
        loss = compute_loss(self.criterion, self.model(x_val), y_val)
        self.model.train()
        return float(loss)

    def state_dict_cpu(self) -> dict:
        return {k: v.detach().cpu() for k, v in self.model.state_dict().items()}


# ----------------------------------------------------------------------------
# Barrier-worker entry (reference handle_model, distributed.py:66-205)
# ----------------------------------------------------------------------------


def handle_model(
    index: int,
    iterator: Iterable,
    torch_obj_str: str,
    iters: int = 10,
    verbose: int = 0,
    mini_batch: int = -1,
    validation_pct: float = 0.0,
    device: str = "cpu",
    early_stop_patience: int = -1,
    backend: Optional[str] = None,
    compile_mode: Optional[str] = None,
    bucket_cap_mb: float = 25.0,
) -> List[dict]:
    if index < 0:
        raise RuntimeError("invalid partition index")

    ctx = get_barrier_context()
    cleanup_stale_process_group()
    rank = index
    dev = pick_device(device, rank)
    world_size = init_process_group_from_barrier(ctx, rank, dev, backend)

    try:
        loaded = load_torch_model(torch_obj_str, device=dev)
        if dev.startswith("cuda"):
            # device ingest: pinned fp64 staging + hipMemcpyAsync + on-device
            # cast to bf16 (utils.data.handle_features_device)
            data = handle_features_device(iterator, validation_pct, device=dev)
        else:
            data = handle_features(iterator, validation_pct)
        if data.x_train is None:
            raise RuntimeError(
                "rank %d received an empty partition; repartition so every "
                "barrier task has data" % rank
            )

        x_train = data.x_train.to(dev) if not data.x_train.is_cuda else data.x_train
        # autoencoder mode: no labels -> y = x (reference distributed.py:136)
        y_train = (
            (data.y_train.to(dev) if not data.y_train.is_cuda else data.y_train)
            if data.y_train is not None
            else x_train
        )
        x_val = data.x_val.to(dev) if data.x_val is not None and not data.x_val.is_cuda else data.x_val
        y_val = (
            (data.y_val.to(dev) if not data.y_val.is_cuda else data.y_val)
            if data.y_val is not None
            else (x_val if x_val is not None else None)
        )

        trainer = SyncTrainer(
            loaded.model,
            loaded.criterion,
            loaded.optimizer,
            device=dev,
            world_size=world_size,
            compile_mode=compile_mode,
            bucket_cap_mb=bucket_cap_mb,
        )

        es = EarlyStopping(patience=early_stop_patience) if early_stop_patience > 0 else None
        n = x_train.shape[0]
        # collectives must live on the comm device (RCCL wants GPU tensors)
        comm_dev = dev if dev.startswith("cuda") else "cpu"
        metrics = StepMetrics()

        # GPU minibatches are drawn and gathered on the device (one seed from
        # np.random here, nothing per iteration); the CPU path keeps the
        # reference's per-iteration np.random.choice
        sampler = None
        if dev.startswith("cuda") and 0 < mini_batch < n:
            sampler = DeviceMinibatchSampler(
                x_train, y_train if data.y_train is not None else None, mini_batch
            )

        for i in range(iters):
            if sampler is not None:
                metrics.start()
                with trace_range("train_step"):
                    loss = trainer.train_step_sampled(sampler)
                metrics.stop(loss)
            else:
                if 0 < mini_batch < n:
                    idx = torch.from_numpy(np.random.choice(n, mini_batch, replace=False))
                    xb = x_train[idx]
                    yb = y_train[idx]
                else:
                    xb, yb = x_train, y_train

                metrics.start()
                with trace_range("train_step"):
                    loss = trainer.train_step(xb, yb)
                metrics.stop(loss)

            if es is not None:
                loss_for_es = (
                    trainer.validation_loss(x_val, y_val) if x_val is not None else loss
                )
                # ONE collective per early-stop iteration (vs the reference's
                # two, distributed.py:188,194): all-reduce guarantees every
                # rank receives the identical summed loss, and EarlyStopping
                # is deterministic in its input history, so every rank reaches
                # the same stop decision locally — the consensus flag needs no
                # second collective.
                lt = torch.tensor([loss_for_es], device=comm_dev)
                dist.all_reduce(lt)
                if es.step(float(lt) / world_size):
                    break

            if verbose:
                print("rank %d iter %d loss %.6f" % (rank, i, loss), flush=True)

        if verbose:
            print("rank %d metrics %r" % (rank, metrics), flush=True)

        # ranks end in identical states (grads synced; same init) —
        # reference collects all and takes [0] (distributed.py:255-261)
        return [trainer.state_dict_cpu()]
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


# ----------------------------------------------------------------------------
# Driver entry (reference train_distributed, distributed.py:208-261)
# ----------------------------------------------------------------------------


def train_distributed(
    rdd,
    torch_obj: str,
    iters: int = 10,
    partition_shuffles: int = 1,
    verbose: int = 0,
    mini_batch: int = -1,
    validation_pct: float = 0.0,
    device: str = "cpu",
    early_stop_patience: int = -1,
    backend: Optional[str] = None,
    compile_mode: Optional[str] = None,
    bucket_cap_mb: float = 25.0,
) -> dict:
    """Run sync data-parallel training over a (barrier) RDD; returns the
    trained state_dict."""
    torch_obj_str, _shapes = load_base_torch(torch_obj)

    state = None
    for shuffle_round in range(max(1, partition_shuffles)):
        obj_str = torch_obj_str
        if state is not None:
            # carry trained weights into the next shuffle round
            loaded = load_torch_model(torch_obj_str)
            loaded.model.load_state_dict(state)
            obj_str, _ = load_base_torch(
                serialize_torch_obj(
                    loaded.model,
                    loaded.criterion,
                    type(loaded.optimizer),
                    **loaded.optimizer.defaults,
                )
            )

        def worker(index, iterator, _obj=obj_str):
            return handle_model(
                index,
                iterator,
                _obj,
                iters=iters,
                verbose=verbose,
                mini_batch=mini_batch,
                validation_pct=validation_pct,
                device=device,
                early_stop_patience=early_stop_patience,
                backend=backend,
                compile_mode=compile_mode,
                bucket_cap_mb=bucket_cap_mb,
            )

        # barrier scheduling is mandatory for sync mode: every rank must be
        # alive simultaneously for the allGather rendezvous (reference builds
        # PipelinedRDD(isFromBarrier=True), distributed.py:53-63).  Applied
        # per round so repartition below still sees the plain RDD (pyspark's
        # RDDBarrier exposes only mapPartitions*).
        brdd = rdd.barrier() if hasattr(rdd, "barrier") else rdd
        states = brdd.mapPartitionsWithIndex(worker).collect()
        state = states[0]

        if shuffle_round + 1 < partition_shuffles:
            rdd = rdd.repartition(rdd.getNumPartitions())

    return state
