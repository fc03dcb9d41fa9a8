"""One-launch MLP inference (mlp_predict.hip: hidden layers, head and argmax
with the activations kept in LDS) against the per-layer linear_fwd chain it
replaces, and the routes built on it: hip_mlp_predict, MnistMLPFused,
GraphedForward(call=), the transformer and the inference server."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped off-GPU
    pytest.skip("needs MI355X", allow_module_level=True)

from sparktorch_amd import ops
from sparktorch_amd.compat.local import LocalDataFrame
from sparktorch_amd.inference import create_spark_torch_model
from sparktorch_amd.ops import functional as Fn
from sparktorch_amd.ops.graph import GraphedForward
from sparktorch_amd.ops.modules import MnistMLPFused
from sparktorch_amd.serving import InferenceServer

DEV = "cuda:0"
TOL = 0.02  # max|a - ref| / max|ref| against fp32 torch

MS = (1, 127, 128, 129, 255, 257, 1000)
K0S = (8, 24, 40, 200, 784)
CHAINS = ((64,), (256,), (192, 64), (256, 256), (128, 256, 64, 192))
CS = (2, 10, 16)


def bf(x):
    return x.to(torch.bfloat16)


def bits(t):
    return t.view(torch.int16)


def make_chain(K0, widths, C, bias_rule, seed):
    """bf16 weights and fp32-or-absent biases of hidden layers `widths` and a
    C-class head; bias_rule(l) says whether layer l (head = len(widths)) has one."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    ws, bs = [], []
    k = K0
    for l, n in enumerate(tuple(widths) + (C,)):
        ws.append(bf(torch.randn(n, k, device=DEV, generator=g) / k ** 0.5).contiguous())
        bs.append(torch.randn(n, device=DEV, generator=g) * 0.5 if bias_rule(l) else None)
        k = n
    return ws, bs


def make_x(M, K0, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return bf(torch.randn(M, K0, device=DEV, generator=g)).contiguous()


def oracle(x, ws, bs):
    """The route being replaced: one linear_fwd per layer, pinned to gemm.hip."""
    ext = ops.ext()
    h = x
    for l, (w, b) in enumerate(zip(ws, bs)):
        h = ext.linear_fwd(h, w, b, l < len(ws) - 1, False)
    return h


def np_argmax(logits):
    return np.argmax(logits.float().cpu().numpy(), axis=1)


def check(x, ws, bs, max_blocks=0, tag=""):
    ref = oracle(x, ws, bs)
    classes, logits = ops.ext().mlp_predict(x, ws, bs, True, max_blocks)
    torch.cuda.synchronize()
    assert classes.dtype == torch.int32 and classes.shape == (x.shape[0],), tag
    assert logits.dtype == torch.bfloat16 and logits.shape == ref.shape, tag
    assert torch.equal(bits(logits), bits(ref)), tag
    assert np.array_equal(classes.cpu().numpy(), np_argmax(ref)), tag
    return classes, logits, ref


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("widths", CHAINS, ids=lambda w: "x".join(map(str, w)))
def test_edges_match_per_layer_chain(widths, C):
    assert ops.ext().mlp_predict_supported(784, list(widths), C)
    # C = 10: every layer biased; C = 2: the even layers; C = 16: the odd ones
    rule = {10: lambda l: True, 2: lambda l: l % 2 == 0, 16: lambda l: l % 2 == 1}[C]
    for K0 in K0S:
        ws, bs = make_chain(K0, widths, C, rule, seed=100 + K0)
        x_all = make_x(max(MS), K0, seed=7 + K0)  # smaller M are row prefixes
        for M in MS:
            check(x_all[:M], ws, bs, tag="M=%d K0=%d widths=%s C=%d" % (M, K0, widths, C))


def test_sanity_against_fp32_torch():
    K0, widths, C = 784, (256, 256), 10
    ws, bs = make_chain(K0, widths, C, lambda l: True, seed=11)
    x = make_x(1000, K0, seed=12)
    _, logits, _ = check(x, ws, bs)
    h = x.float()
    for l, (w, b) in enumerate(zip(ws, bs)):
        h = h @ w.float().t() + b
        if l < len(ws) - 1:
            h = bf(torch.relu(h)).float()
    err = ((logits.float() - h).abs().max() / h.abs().max()).item()
    print("fp32 torch rel err %.3e" % err)
    assert err <= TOL


def test_ties_take_the_lower_index():
    K0, widths, C = 40, (64,), 10
    ws, bs = make_chain(K0, widths, C, lambda l: True, seed=21)
    ws[-1][7] = ws[-1][2]
    bs[-1][7] = bs[-1][2]
    # lift the tied pair to the top of every row
    bs[-1][2] += 100.0
    bs[-1][7] += 100.0
    x = make_x(300, K0, seed=22)
    classes, logits, _ = check(x, ws, bs)
    assert torch.equal(bits(logits[:, 2]), bits(logits[:, 7]))
    assert (classes == 2).all()


def test_non_finite_rows():
    K0, widths, C = 40, (64, 64), 10
    ws, bs = make_chain(K0, widths, C, lambda l: True, seed=31)
    x = make_x(300, K0, seed=32)
    bad = [3, 64, 130, 131, 299]
    x[3, 5] = float("inf")
    x[64, 0] = float("nan")
    x[130, 39] = float("inf")
    x[131, 7] = float("nan")
    x[299, 20] = float("inf")
    ref = oracle(x, ws, bs)
    classes, logits = ops.ext().mlp_predict(x, ws, bs, True, 0)
    good = torch.ones(300, dtype=torch.bool, device=DEV)
    good[bad] = False
    assert torch.isfinite(ref[good].float()).all()
    assert torch.equal(bits(logits[good]), bits(ref[good]))
    assert np.array_equal(classes[good].cpu().numpy(), np_argmax(ref[good]))
    assert torch.equal(torch.isnan(logits[~good]), torch.isnan(ref[~good]))
    assert np.array_equal(classes[~good].cpu().numpy(), np_argmax(logits[~good]))


def test_argmax_of_nan_and_inf_logits():
    """Head biases of NaN / +-inf put those values into chosen logit columns of
    every row: the first NaN wins, then +inf, as np.argmax."""
    K0, widths, C = 24, (64,), 10
    ws, bs = make_chain(K0, widths, C, lambda l: True, seed=41)
    x = make_x(200, K0, seed=42)
    for vals in ({4: float("inf")}, {6: float("nan"), 8: float("nan"), 1: float("inf")},
                 {0: float("-inf"), 9: float("inf"), 5: float("inf")}):
        b = [t.clone() for t in bs]
        for c, v in vals.items():
            b[-1][c] = v
        classes, logits = ops.ext().mlp_predict(x, ws, b, True, 0)
        ref = oracle(x, ws, b)
        assert torch.equal(torch.isnan(logits), torch.isnan(ref))
        assert np.array_equal(classes.cpu().numpy(), np_argmax(logits))
        want = 6 if 6 in vals else (4 if 4 in vals else 5)
        assert (classes == want).all()


@pytest.mark.parametrize("max_blocks", [1, 3])
def test_several_tiles_per_block(max_blocks):
    """40 000 rows on one or three persistent blocks: each walks a hundred or
    more tiles and the last one is partial."""
    K0, widths, C = 40, (64,), 10
    ws, bs = make_chain(K0, widths, C, lambda l: True, seed=51)
    x = make_x(40000, K0, seed=52)
    check(x, ws, bs, max_blocks=max_blocks)


def test_several_tiles_per_block_deep_chain():
    """The flagship widths on two blocks: the next tile's x slabs are in
    flight under the hidden layers of this one."""
    K0, widths, C = 200, (256, 256), 10
    ws, bs = make_chain(K0, widths, C, lambda l: l != 1, seed=53)
    x = make_x(1500, K0, seed=54)
    check(x, ws, bs, max_blocks=2)


def test_no_logits_requested():
    K0, widths, C = 200, (192, 64), 16
    ws, bs = make_chain(K0, widths, C, lambda l: True, seed=61)
    x = make_x(257, K0, seed=62)
    classes, _, _ = check(x, ws, bs)
    classes2, none = ops.ext().mlp_predict(x, ws, bs, False, 0)
    assert none is None
    assert torch.equal(classes2, classes)


def test_unsupported_shapes_raise():
    ext = ops.ext()
    x = make_x(16, 40, seed=71)

    def run(K0, widths, C, cast=None):
        ws, bs = make_chain(K0, widths, C, lambda l: True, seed=72)
        if cast is not None:
            ws = [w.to(cast) for w in ws]
        return ext.mlp_predict(make_x(16, K0, seed=73), ws, bs, True, 0)

    run(40, (64,), 10)  # the baseline is fine
    assert not ext.mlp_predict_supported(40, [96], 10)
    assert not ext.mlp_predict_supported(40, [64], 17)
    assert not ext.mlp_predict_supported(40, [64], 1)
    assert not ext.mlp_predict_supported(12, [64], 10)
    assert not ext.mlp_predict_supported(40, [64] * 5, 10)
    for K0, widths, C in ((40, (96,), 10), (40, (64,), 17), (12, (64,), 10),
                          (40, (64, 64, 64, 64, 64), 10)):
        with pytest.raises(RuntimeError):
            run(K0, widths, C)
    with pytest.raises(RuntimeError):
        run(40, (64,), 10, cast=torch.float32)
    ws, bs = make_chain(40, (64,), 10, lambda l: True, seed=74)
    with pytest.raises(RuntimeError):  # the chain does not fit x
        ext.mlp_predict(make_x(16, 48, seed=75), ws, bs, True, 0)
    del x


class _ExtProxy:
    """The extension with mlp_predict replaced by a tripwire."""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        if name == "mlp_predict":
            raise AssertionError("fused kernel reached")
        return getattr(self._real, name)


def _fp32_layers(K0, widths, C, seed):
    ws, bs = make_chain(K0, widths, C, lambda l: True, seed)
    n = len(ws)
    return [(w.float(), b, l < n - 1) for l, (w, b) in enumerate(zip(ws, bs))]


def test_functional_route_and_fallback_flag(monkeypatch):
    layers = _fp32_layers(40, (64, 128), 10, seed=81)
    x = make_x(300, 40, seed=82)
    calls = []
    real = ops.ext()

    class Counting(_ExtProxy):
        def __getattr__(self, name):
            if name == "mlp_predict":
                calls.append(1)
            return getattr(self._real, name)

    monkeypatch.setattr(Fn.ops, "ext", lambda: Counting(real))
    c1, l1 = Fn.hip_mlp_predict(x, layers, want_logits=True)
    assert len(calls) == 1  # the kernel ran
    c1b, none = Fn.hip_mlp_predict(x.float(), layers)  # fp32 x is cast first
    assert none is None and torch.equal(c1b, c1)

    monkeypatch.setattr(Fn, "_PREDICT_FUSION", False)
    monkeypatch.setattr(Fn.ops, "ext", lambda: _ExtProxy(real))
    c0, l0 = Fn.hip_mlp_predict(x, layers, want_logits=True)
    assert c0.dtype == torch.int32
    assert torch.equal(bits(l1), bits(l0))
    assert torch.equal(c1, c0)


def test_functional_falls_back_on_unsupported_chain(monkeypatch):
    real = ops.ext()
    monkeypatch.setattr(Fn.ops, "ext", lambda: _ExtProxy(real))
    x = make_x(100, 40, seed=91)
    for widths, C in (((96,), 10), ((64,), 17)):
        layers = _fp32_layers(40, widths, C, seed=92)
        classes, logits = Fn.hip_mlp_predict(x, layers, want_logits=True)
        assert np.array_equal(classes.cpu().numpy(), np_argmax(logits))
    layers = _fp32_layers(40, (64,), 10, seed=93)
    layers[0] = (layers[0][0], layers[0][1], False)  # a hidden layer without ReLU
    classes, logits = Fn.hip_mlp_predict(x, layers, want_logits=True)
    assert np.array_equal(classes.cpu().numpy(), np_argmax(logits))


def _count_kernel(monkeypatch):
    calls = []
    real = ops.ext()

    class Counting(_ExtProxy):
        def __getattr__(self, name):
            if name == "mlp_predict":
                calls.append(1)
            return getattr(self._real, name)

    monkeypatch.setattr(Fn.ops, "ext", lambda: Counting(real))
    return calls


def test_module_route(monkeypatch):
    torch.manual_seed(101)
    model = MnistMLPFused(40, 64, 10).to(DEV).eval()
    x = make_x(300, 40, seed=102)
    calls = _count_kernel(monkeypatch)
    with torch.no_grad():
        below = model(x)  # under the measured row threshold: per-layer route
    assert len(calls) == 0
    monkeypatch.setattr(Fn, "mlp_predict_min_rows", lambda: 1)
    with torch.no_grad():
        fused = model(x)
    assert len(calls) == 1
    assert torch.equal(bits(fused), bits(below))
    monkeypatch.setattr(Fn, "_PREDICT_FUSION", False)
    with torch.no_grad():
        off = model(x)
    assert len(calls) == 1
    assert torch.equal(bits(fused), bits(off))
    monkeypatch.setattr(Fn, "_PREDICT_FUSION", True)
    ids = model.predict_classes(x)
    assert len(calls) == 2
    assert np.array_equal(ids.cpu().numpy(), np_argmax(off))
    # grad enabled, or train mode: the autograd chain, never the kernel
    y = model(x)
    assert y.requires_grad and len(calls) == 2
    model.train()
    with torch.no_grad():
        model(x)
    assert len(calls) == 2


def test_graphed_class_ids():
    torch.manual_seed(111)
    model = MnistMLPFused(40, 64, 10).to(DEV).eval()
    runner = GraphedForward(model, device=DEV, call=model.predict_classes, batch_size=128)
    rng = np.random.RandomState(112)
    for n in (128, 77):
        xb = torch.from_numpy(rng.randn(n, 40).astype(np.float32))
        got = runner(xb).cpu().numpy()
        assert got.dtype == np.int32 and got.shape == (n,)
        want = model.predict_classes(xb.to(DEV)).cpu().numpy()
        assert np.array_equal(got, want)
        with torch.no_grad():
            assert np.array_equal(got, np_argmax(model(xb.to(DEV))))


def _served_case():
    torch.manual_seed(121)
    model = MnistMLPFused(40, 64, 10)
    feats = np.random.RandomState(122).randn(300, 40).astype(np.float32)
    with torch.no_grad():
        logits = model.to(DEV).eval()(torch.from_numpy(feats).to(DEV)).float().cpu().numpy()
    return model.cpu(), feats, logits


def test_transformer_on_gpu():
    model, feats, logits = _served_case()
    df = LocalDataFrame.from_arrays(feats, [0.0] * len(feats), num_partitions=1)
    stage = create_spark_torch_model(model, "features", "p")
    stage.setParams(batchSize=128, device=DEV)
    preds = [r["p"] for r in stage.transform(df).collect()]
    assert all(isinstance(p, float) for p in preds)
    assert np.array_equal(np.asarray(preds), np.argmax(logits, axis=1).astype(np.float64))

    vec = create_spark_torch_model(model, "features", "p", useVectorOut=True)
    vec.setParams(batchSize=128, device=DEV)
    rows = np.stack([np.asarray(r["p"]) for r in vec.transform(df).collect()])
    assert np.array_equal(rows, logits.astype(np.float64))


def test_inference_server_on_gpu():
    model, feats, logits = _served_case()
    srv = InferenceServer(model, device=DEV, batch_size=128)
    preds = srv.predict(feats.tolist())
    assert all(isinstance(p, float) for p in preds)
    assert np.array_equal(np.asarray(preds), np.argmax(logits, axis=1).astype(np.float64))
    rows = np.asarray(srv.predict(feats.tolist(), vector_out=True))
    assert np.array_equal(rows, logits.astype(np.float64))
