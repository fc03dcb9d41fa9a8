"""HIP-graph-captured batched inference.

Replaces the reference's per-row batch-1 Python UDF forward
(torch_distributed.py:106-128) with: pack rows -> fixed-size batches -> one
graph-captured forward replayed per batch (pad-and-mask for the ragged last
batch).  Removes every per-launch gap in small-model serving, which is the
entire cost at batch-1 in the reference design.
"""

from __future__ import annotations

from typing import Callable, Optional

import torch


def class_id_call(model) -> Optional[Callable[[torch.Tensor], torch.Tensor]]:
    """``model.predict_classes`` where the model offers it for a multi-output
    net (one int32 class id per row, the argmax of its logits), else None.
    Callers that only want the argmax capture it in place of ``model(x)`` and
    copy back 4 bytes a row."""
    fn = getattr(model, "predict_classes", None)
    if not callable(fn) or int(getattr(model, "num_classes", 2)) < 2:
        return None
    return fn


class GraphedForward:
    """Capture ``model(x)`` for a fixed batch shape once; replay thereafter.

    Inputs shorter than ``batch_size`` are padded (rows beyond the real count
    are sliced off the output), so ONE graph serves every batch including the
    ragged tail.  ``call``, when given, is captured in place of ``model(x)``:
    any callable of the device batch that returns one tensor with a leading
    batch dimension (e.g. ``model.predict_classes``).
    """

    def __init__(self, model: torch.nn.Module, device: str = "cuda:0", batch_size: int = 8192,
                 call: Optional[Callable[[torch.Tensor], torch.Tensor]] = None):
        self.model = model.to(device).eval()
        self._call = call if call is not None else self.model
        self.device = device
        self.batch_size = batch_size
        self._graph: Optional[torch.cuda.CUDAGraph] = None
        self._static_in: Optional[torch.Tensor] = None
        self._static_out: Optional[torch.Tensor] = None
        self._feat_shape = None

    def _capture(self, feat_shape) -> None:
        x = torch.zeros((self.batch_size, *feat_shape), device=self.device)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.no_grad():
            for _ in range(2):
                out = self._call(x)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g), torch.no_grad():
            out = self._call(x)
        self._graph = g
        self._static_in = x
        self._static_out = out
        self._feat_shape = tuple(feat_shape)

    @torch.no_grad()
    def replay_device(self, x_dev: torch.Tensor) -> torch.Tensor:
        """Replay on a device-resident full batch (the serving hot loop: no
        host copy, no ragged handling)."""
        feat_shape = tuple(x_dev.shape[1:])
        if self._graph is None or self._feat_shape != feat_shape:
            self._capture(feat_shape)
        self._static_in.copy_(x_dev)
        self._graph.replay()
        return self._static_out

    @torch.no_grad()
    def __call__(self, x_cpu: torch.Tensor) -> torch.Tensor:
        feat_shape = tuple(x_cpu.shape[1:])
        n = x_cpu.shape[0]
        if n > self.batch_size:
            raise ValueError("batch larger than captured size")
        if self._graph is None or self._feat_shape != feat_shape:
            self._capture(feat_shape)
        self._static_in[:n].copy_(x_cpu.to(self.device, non_blocking=True))
        if n < self.batch_size:
            self._static_in[n:].zero_()
        self._graph.replay()
        # NB: a view of the static output buffer — consume (copy/cpu()) before
        # the next replay overwrites it; both call sites do so immediately
        return self._static_out[:n]
