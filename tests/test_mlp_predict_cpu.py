"""hip_mlp_predict off the GPU (the F.linear / F.relu chain plus argmax) and
the transformer on a model whose forward returns bf16."""

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from sparktorch_amd.compat.local import LocalDataFrame
from sparktorch_amd.inference import create_spark_torch_model
from sparktorch_amd.ops import functional as Fn
from sparktorch_amd.ops.modules import MnistMLPFused


def _layers(seed, dims, tie=False):
    g = torch.Generator().manual_seed(seed)
    layers = []
    for i in range(len(dims) - 1):
        w = torch.randn(dims[i + 1], dims[i], generator=g) / dims[i] ** 0.5
        b = torch.randn(dims[i + 1], generator=g) if i % 2 == 0 else None
        layers.append([w, b, i < len(dims) - 2])
    if tie:  # classes 1 and 3 tie exactly on every row
        w, _, relu = layers[-1]
        w[3] = w[1]
        b = torch.randn(dims[-1], generator=g)
        b[3] = b[1]
        layers[-1] = [w, b, relu]
    return [tuple(l) for l in layers]


def _reference(x, layers):
    h = x
    for w, b, relu in layers:
        h = F.linear(h, w, b)
        if relu:
            h = F.relu(h)
    return h


def test_cpu_chain_and_argmax():
    layers = _layers(1, (24, 64, 192, 10))
    x = torch.randn(37, 24, generator=torch.Generator().manual_seed(2))
    ref = _reference(x, layers)
    classes, logits = Fn.hip_mlp_predict(x, layers, want_logits=True)
    assert classes.dtype == torch.int32 and classes.shape == (37,)
    assert torch.equal(logits, ref)
    assert np.array_equal(classes.numpy(), np.argmax(ref.numpy(), axis=1))
    classes2, none = Fn.hip_mlp_predict(x, layers)
    assert none is None
    assert torch.equal(classes2, classes)


def test_cpu_ties_take_the_lower_index():
    layers = _layers(3, (16, 64, 6), tie=True)
    w, b, _ = layers[-1]
    # make the tied pair the row maximum everywhere: lift both biases alike
    b = b.clone()
    b[1] += 100.0
    b[3] += 100.0
    layers[-1] = (w, b, False)
    x = torch.randn(50, 16, generator=torch.Generator().manual_seed(4))
    ref = _reference(x, layers).numpy()
    assert (ref[:, 1] == ref[:, 3]).all() and (ref.argmax(1) == 1).all()
    classes, none = Fn.hip_mlp_predict(x, layers, want_logits=False)
    assert none is None
    assert (classes.numpy() == 1).all()


def test_cpu_module_predict_classes():
    torch.manual_seed(5)
    model = MnistMLPFused(40, 64, 10).eval()
    x = torch.randn(33, 40)
    with torch.no_grad():
        ref = model(x)
    ids = model.predict_classes(x)
    assert ids.dtype == torch.int32
    assert np.array_equal(ids.numpy(), np.argmax(ref.numpy(), axis=1))


class Bf16Net(nn.Module):
    """A net whose forward returns bf16, as every Hip* model does on the GPU."""

    def __init__(self):
        super().__init__()
        self.fc = nn.Linear(12, 5)

    def forward(self, x):
        return self.fc(x).to(torch.bfloat16)


def _bf16_case():
    torch.manual_seed(6)
    net = Bf16Net()
    feats = np.random.RandomState(7).randn(70, 12).astype(np.float32)
    df = LocalDataFrame.from_arrays(feats, [0.0] * 70, num_partitions=1)
    with torch.no_grad():
        logits = net(torch.from_numpy(feats)).float().numpy()
    return net, df, logits


def test_transformer_bf16_output_argmax():
    """Raised TypeError (numpy has no bf16) before the transformer widened
    sub-fp32 outputs.  batchSize 32 over 70 rows: a ragged last batch."""
    net, df, logits = _bf16_case()
    stage = create_spark_torch_model(net, "features", "p")
    stage.setParams(batchSize=32, device="cpu")
    preds = [r["p"] for r in stage.transform(df).collect()]
    assert len(preds) == 70
    assert all(isinstance(p, float) for p in preds)
    assert np.array_equal(np.asarray(preds), np.argmax(logits, axis=1).astype(np.float64))


def test_transformer_bf16_output_vector():
    net, df, logits = _bf16_case()
    stage = create_spark_torch_model(net, "features", "p", useVectorOut=True)
    stage.setParams(batchSize=32, device="cpu")
    preds = [np.asarray(r["p"]) for r in stage.transform(df).collect()]
    assert len(preds) == 70
    assert np.array_equal(np.stack(preds), logits.astype(np.float64))
