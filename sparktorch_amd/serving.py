"""Model serving for trained SparkTorch models.

The reference's deployment story ends at ``SparkTorchModel.transform`` over
a DataFrame (batch scoring inside Spark).  For production serving on an
MI355X node this module exposes the same trained artifact over HTTP:

* loads either a saved pipeline stage (``PysparkReaderWriter`` carrier
  format), a dill/base64 ``modStr``, or an in-memory ``nn.Module``;
* requests are scored in fixed-size batches through the SAME inference
  engine as ``SparkTorchModel._transform`` — on GPU that is the
  hipGraph-captured forward (:class:`sparktorch_amd.ops.graph.GraphedForward`,
  one replay per batch, 305 M rows/s on the MNIST MLP), on CPU plain eager;
* output semantics match the transformer exactly: argmax for multi-output
  nets, raw scalar otherwise, or the full vector with ``vector_out``.

Usage:

    from sparktorch_amd.serving import InferenceServer
    srv = InferenceServer(model)              # nn.Module / modStr / stage
    app = srv.app()                           # FastAPI app (uvicorn-ready)

    # or: python -m sparktorch_amd.serving --stage saved_stage_dir --port 8000

Endpoints: ``GET /health``, ``GET /info``, ``POST /predict`` with
``{"instances": [[...], ...], "vector_out": false}``.
"""

from __future__ import annotations

import argparse
import threading
from typing import Any, List, Optional

import numpy as np
import torch

from sparktorch_amd.utils.codec import b64_to_obj


class InferenceServer:
    def __init__(
        self,
        model,
        device: Optional[str] = None,
        batch_size: int = 8192,
        vector_out: bool = False,
    ):
        if isinstance(model, str):
            model = b64_to_obj(model)  # modStr payload
        if hasattr(model, "getPytorchModel"):  # SparkTorchModel stage
            model = model.getPytorchModel()
        if not isinstance(model, torch.nn.Module):
            raise TypeError("model must be an nn.Module, a modStr, or a SparkTorchModel")
        self.device = device or ("cuda:0" if torch.cuda.is_available() else "cpu")
        self.batch_size = int(batch_size)
        self.vector_out = bool(vector_out)
        self.model = model.to(self.device).eval()
        self._runner = None
        # class ids only (argmax requests of a model with predict_classes):
        # its own captured graph, 4 bytes a row copied back instead of logits
        self._id_runner = None
        if self.device.startswith("cuda"):
            from sparktorch_amd.ops.graph import GraphedForward, class_id_call

            self._runner = GraphedForward(self.model, device=self.device,
                                          batch_size=self.batch_size)
            call = class_id_call(self.model)
            if call is not None:
                self._id_runner = GraphedForward(self.model, device=self.device,
                                                 batch_size=self.batch_size, call=call)
        self._n_served = 0
        # FastAPI dispatches sync endpoints on a threadpool; the hipGraph
        # replay reuses static input/output buffers, so scoring must be
        # serialized (throughput comes from batching, not request threads)
        self._lock = threading.Lock()

    # ------------------------------------------------------------------
    @torch.no_grad()
    def predict(self, instances: List[List[float]], vector_out: Optional[bool] = None) -> List[Any]:
        """Score a list of feature rows with SparkTorchModel semantics."""
        use_vec = self.vector_out if vector_out is None else bool(vector_out)
        feats = np.asarray(instances, dtype=np.float32)
        if feats.ndim == 1:
            feats = feats.reshape(1, -1)
        out: List[Any] = []
        with self._lock:
            return self._predict_locked(feats, use_vec, out)

    def _predict_locked(self, feats, use_vec, out):
        for s in range(0, len(feats), self.batch_size):
            xb = torch.from_numpy(feats[s : s + self.batch_size])
            if not use_vec and self._id_runner is not None:
                out.extend(float(v) for v in self._id_runner(xb).cpu().numpy())
                continue
            if self._runner is not None:
                pred = self._runner(xb)
            else:
                pred = self.model(xb.to(self.device))
            pred = pred.float().cpu().numpy()
            if use_vec:
                out.extend(row.tolist() for row in pred)
            elif pred.ndim > 1 and pred.shape[1] > 1:
                out.extend(float(v) for v in np.argmax(pred, axis=1))
            else:
                out.extend(float(v) for v in pred.reshape(-1))
        self._n_served += len(feats)
        return out

    # ------------------------------------------------------------------
    def app(self):
        """Build the FastAPI app (import deferred so the core package does
        not require fastapi)."""
        from fastapi import Body, FastAPI, HTTPException

        api = FastAPI(title="sparktorch_amd inference", version="0.1.0")
        srv = self

        @api.get("/health")
        def health():
            return {"status": "ok", "device": srv.device}

        @api.get("/info")
        def info():
            n_params = sum(p.numel() for p in srv.model.parameters())
            return {
                "device": srv.device,
                "batch_size": srv.batch_size,
                "hipgraph": srv._runner is not None,
                "n_parameters": n_params,
                "n_served": srv._n_served,
            }

        @api.post("/predict")
        def predict(payload: dict = Body(...)):
            instances = payload.get("instances")
            if not instances:
                raise HTTPException(status_code=400, detail="instances is empty")
            try:
                return {"predictions": srv.predict(instances, payload.get("vector_out"))}
            except Exception as e:  # shape/dtype errors surface as 400s
                raise HTTPException(status_code=400, detail=str(e))

        return api


def load_stage(path: str):
    """Load a saved SparkTorch stage (carrier format) from disk."""
    from sparktorch_amd.torch_distributed import SparkTorchModel

    return SparkTorchModel.load(path)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description="Serve a trained SparkTorch model over HTTP")
    ap.add_argument("--stage", type=str, help="saved SparkTorchModel directory")
    ap.add_argument("--host", type=str, default="0.0.0.0")
    ap.add_argument("--port", type=int, default=8000)
    ap.add_argument("--batch-size", type=int, default=8192)
    ap.add_argument("--device", type=str, default=None)
    args = ap.parse_args(argv)
    if not args.stage:
        ap.error("--stage is required")

    import uvicorn

    srv = InferenceServer(load_stage(args.stage), device=args.device,
                          batch_size=args.batch_size)
    uvicorn.run(srv.app(), host=args.host, port=args.port)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
