"""fp32 rows in the one-launch MLP inference kernel (mlp_predict_kernel<true>):
bit-identical to casting x with torch and running the bf16 kernel."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped off-GPU
    pytest.skip("needs MI355X", allow_module_level=True)

from sparktorch_amd import ops
from sparktorch_amd.ops import functional as Fn
from sparktorch_amd.ops.modules import MnistMLPFused

DEV = "cuda:0"
TOL = 0.02  # max|a - ref| / max|ref|, as tests/test_gpu_mlp_predict.py


def make_chain(K0, widths, C, bias_rule, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    ws, bs, k = [], [], K0
    for l, n in enumerate(tuple(widths) + (C,)):
        ws.append((torch.randn(n, k, device=DEV, generator=g) / k ** 0.5).to(torch.bfloat16))
        bs.append(torch.randn(n, device=DEV, generator=g) * 0.5 if bias_rule(l) else None)
        k = n
    return ws, bs


def make_x(M, K0, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(M, K0, device=DEV, generator=g)


def both(x, ws, bs, max_blocks=0):
    """(classes, logits as int16 bits) of the fp32 route and of the cast route."""
    ext = ops.ext()
    c1, l1 = ext.mlp_predict(x, ws, bs, True, max_blocks)
    c0, l0 = ext.mlp_predict(x.to(torch.bfloat16), ws, bs, True, max_blocks)
    assert l1.dtype == torch.bfloat16 and c1.dtype == torch.int32
    return c1, l1, c0, l0


def same(x, ws, bs, max_blocks=0, tag=""):
    c1, l1, c0, l0 = both(x, ws, bs, max_blocks)
    assert torch.equal(l1.view(torch.int16), l0.view(torch.int16)), tag
    assert torch.equal(c1, c0), tag
    return l1


@pytest.mark.parametrize("C", (2, 10, 16))
@pytest.mark.parametrize("widths", ((64,), (256, 256), (128, 256, 64, 192)),
                         ids=lambda w: "x".join(map(str, w)))
def test_edges_bit_identical_to_cast_route(widths, C):
    rule = {10: lambda l: True, 2: lambda l: l % 2 == 0, 16: lambda l: l % 2 == 1}[C]
    for K0 in (8, 24, 40, 200, 784):
        ws, bs = make_chain(K0, widths, C, rule, seed=100 + K0)
        x_all = make_x(1000, K0, seed=7 + K0)
        for M in (1, 127, 128, 129, 257, 1000):
            logits = same(x_all[:M], ws, bs, tag="M=%d K0=%d" % (M, K0))
        if (K0, widths, C) == (784, (256, 256), 10):
            h = x_all.to(torch.bfloat16).double()
            for l, (w, b) in enumerate(zip(ws, bs)):
                h = h @ w.double().t() + b.double()
                if l < len(ws) - 1:
                    h = torch.relu(h).to(torch.bfloat16).double()
            err = ((logits.double() - h).abs().max() / h.abs().max()).item()
            print("fp64 rel err %.3e" % err)
            assert err <= TOL


def test_rounding_is_nearest_even_and_overflows_to_inf():
    K0, M = 40, 300
    ws, bs = make_chain(K0, (64,), 10, lambda l: True, seed=21)
    base = make_x(M, K0, seed=22).to(torch.bfloat16).float().view(torch.int32)
    # bf16 value + half an ulp (odd and even mantissas both occur), then that
    # +- one fp32 ulp, cycling over the columns
    col = torch.arange(K0, device=DEV) % 4
    delta = torch.tensor([0x8000, 0x8001, 0x7FFF, 0], device=DEV, dtype=torch.int32)[col]
    x = (base + delta).view(torch.float32).contiguous()
    x[5, 3] = 3.4e38
    x[200, 39] = -3.4e38
    assert torch.isinf(x.to(torch.bfloat16)[5, 3])
    same(x, ws, bs)


def test_non_finite_rows():
    K0, M = 40, 300
    ws, bs = make_chain(K0, (64, 64), 10, lambda l: True, seed=31)
    x = make_x(M, K0, seed=32)
    xi = x.view(torch.int32)
    x[3, 5] = float("inf")
    x[64, 0] = float("-inf")
    xi[130, 39] = 0x7F800001  # low-payload NaN in the last column of the K tail slab
    xi[131, 7] = 0x7FC00000
    xi[299, 32] = -0x7FFFFF  # 0xFF800001
    bad = [3, 64, 130, 131, 299]
    c1, l1, c0, l0 = both(x, ws, bs)
    good = torch.ones(M, dtype=torch.bool, device=DEV)
    good[bad] = False
    assert torch.isfinite(l0[good].float()).all()
    assert torch.equal(l1[good].view(torch.int16), l0[good].view(torch.int16))
    assert torch.equal(c1[good], c0[good])
    assert torch.equal(torch.isnan(l1[~good]), torch.isnan(l0[~good]))
    assert np.array_equal(c1.cpu().numpy(), np.argmax(l1.float().cpu().numpy(), axis=1))


@pytest.mark.parametrize("max_blocks", (1, 2))
@pytest.mark.parametrize("K0,widths,M", ((40, (64,), 40000), (200, (256, 256), 1500)))
def test_persistent_walk(K0, widths, M, max_blocks):
    ws, bs = make_chain(K0, widths, 10, lambda l: l != 1, seed=51)
    same(make_x(M, K0, seed=52), ws, bs, max_blocks=max_blocks)


def test_routes(monkeypatch):
    K0, M = 40, 300
    ws, bs = make_chain(K0, (64, 128), 10, lambda l: True, seed=81)
    layers = [(w.float(), b, l < 2) for l, (w, b) in enumerate(zip(ws, bs))]
    x = make_x(M, K0, seed=82)
    seen = []
    real = ops.ext()

    class Recording:
        def __getattr__(self, name):
            if name == "mlp_predict":
                return lambda xx, *a: (seen.append(xx.dtype), real.mlp_predict(xx, *a))[1]
            return getattr(real, name)

    monkeypatch.setattr(Fn.ops, "ext", lambda: Recording())
    c1, l1 = Fn.hip_mlp_predict(x, layers, want_logits=True)
    buf = torch.zeros(M * K0 + 4, device=DEV)
    view = buf.flatten()[1:1 + M * K0].view(M, K0)
    view.copy_(x)
    assert view.data_ptr() % 16 != 0
    c2, l2 = Fn.hip_mlp_predict(view, layers, want_logits=True)
    monkeypatch.setattr(Fn, "_PREDICT_F32", False)
    c0, l0 = Fn.hip_mlp_predict(x, layers, want_logits=True)
    assert seen == [torch.float32, torch.bfloat16, torch.bfloat16]
    for c, l in ((c1, l1), (c2, l2)):
        assert torch.equal(l.view(torch.int16), l0.view(torch.int16)) and torch.equal(c, c0)

    monkeypatch.setattr(Fn, "_PREDICT_F32", True)
    torch.manual_seed(101)
    model = MnistMLPFused(40, 64, 10).to(DEV).eval()
    ids = model.predict_classes(x)
    assert seen[-1] == torch.float32
    monkeypatch.setattr(Fn, "_PREDICT_FUSION", False)
    with torch.no_grad():
        off = model(x)
    assert np.array_equal(ids.cpu().numpy(), np.argmax(off.float().cpu().numpy(), axis=1))
