"""What the fused bindings refuse.  For each of them one valid call at the
smallest served shape (64 rows, 64 inputs where the kernel serves that width,
10 classes), then the same call with one operand spoiled at a time: a wrong
dtype, a non-contiguous view, one wrong dimension, an optional fp32 vector of
the wrong length, an activation that starts 8 bytes into a 16-byte line.
Every spoiled call raises RuntimeError before anything is launched: no
operand, dw / db / out among them, has a bit changed."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped off-GPU
    pytest.skip("needs MI355X", allow_module_level=True)

from sparktorch_amd import ops

DEV = "cuda:0"
B, K, C = 64, 64, 10
BF, F32, I64 = torch.bfloat16, torch.float32, torch.int64
WRONG_DTYPE = {BF: torch.float16, F32: torch.float64, I64: torch.int32}


def _rand(gen, *shape, dtype=BF):
    return torch.randn(*shape, device=DEV, generator=gen).to(dtype).contiguous()


def _operands(gen, spec):
    """spec: name -> (dtype, shape); int64 operands are class ids."""
    t = {}
    for name, (dtype, shape) in spec.items():
        if dtype == I64:
            t[name] = torch.randint(0, C, shape, device=DEV, generator=gen)
        else:
            t[name] = _rand(gen, *shape, dtype=dtype)
    return t


# name -> (operand spec, the call, optional fp32 vectors, activations whose
# alignment the binding checks).  H = 128 and No = 128 are the narrowest
# widths linear_hidden_head_ce and linear_hidden_bwd serve, N = 32 the
# narrowest linear_mse does.
CASES = {
    "linear_head_bwd": (
        {"dz_out": (BF, (B, C)), "w": (BF, (C, K)), "y_in": (BF, (B, K)), "dw": (F32, (C, K)),
         "db": (F32, (C,))},
        lambda e, t: e.linear_head_bwd(t["dz_out"], t["w"], t["y_in"], t["dw"], t["db"], 0),
        ("db",), ("y_in",)),
    "linear_head_ce": (
        {"y_in": (BF, (B, K)), "w": (BF, (C, K)), "bias": (F32, (C,)), "target": (I64, (B,)),
         "dw": (F32, (C, K)), "db": (F32, (C,))},
        lambda e, t: e.linear_head_ce(t["y_in"], t["w"], t["bias"], t["target"], t["dw"], t["db"],
                                      True, 0),
        ("bias", "db"), ("y_in",)),
    "linear_head_mse": (
        {"y_in": (BF, (B, K)), "w": (BF, (C, K)), "bias": (F32, (C,)), "target": (BF, (B, C)),
         "dw": (F32, (C, K)), "db": (F32, (C,))},
        lambda e, t: e.linear_head_mse(t["y_in"], t["w"], t["bias"], t["target"], t["dw"], t["db"],
                                       True, 0),
        ("bias", "db"), ("y_in",)),
    "linear_hidden_head_ce": (
        {"x": (BF, (B, K)), "w2": (BF, (128, K)), "b2": (F32, (128,)), "w3": (BF, (C, 128)),
         "b3": (F32, (C,)), "target": (I64, (B,)), "dw3": (F32, (C, 128)), "db3": (F32, (C,))},
        lambda e, t: e.linear_hidden_head_ce(t["x"], t["w2"], t["b2"], t["w3"], t["b3"],
                                             t["target"], t["dw3"], t["db3"], True, True, 0),
        ("b2", "b3", "db3"), ("x",)),
    "linear_mse": (
        {"y_in": (BF, (B, K)), "w": (BF, (32, K)), "bias": (F32, (32,)), "target": (BF, (B, 32))},
        lambda e, t: e.linear_mse(t["y_in"], t["w"], t["bias"], t["target"], True, 0),
        ("bias",), ("y_in", "target")),
    "linear_wgrad_stream": (
        {"dz": (BF, (B, 64)), "x": (BF, (B, K)), "dw": (F32, (64, K)), "db": (F32, (64,))},
        lambda e, t: e.linear_wgrad_stream(t["dz"], t["x"], t["dw"], t["db"], 0),
        ("db",), ("dz", "x")),
    "linear_wgrad_wide": (
        {"dz": (BF, (B, 64)), "x": (BF, (B, K)), "dw": (F32, (64, K)), "db": (F32, (64,))},
        lambda e, t: e.linear_wgrad_wide(t["dz"], t["x"], t["dw"], t["db"], 0),
        ("db",), ("dz", "x")),
    "linear_hidden_bwd": (
        {"dz": (BF, (B, 128)), "w": (BF, (128, K)), "x_in": (BF, (B, K)), "dw": (F32, (128, K)),
         "db": (F32, (128,)), "out": (BF, (B, K))},
        lambda e, t: e.linear_hidden_bwd(t["dz"], t["w"], t["x_in"], t["dw"], t["db"], 0, t["out"]),
        ("db",), ("dz", "x_in", "out")),
    "mlp_predict": (
        {"x": (BF, (B, K)), "w0": (BF, (64, K)), "b0": (F32, (64,)), "w1": (BF, (C, 64)),
         "b1": (F32, (C,))},
        lambda e, t: e.mlp_predict(t["x"], [t["w0"], t["w1"]], [t["b0"], t["b1"]], True, 0),
        ("b0", "b1"), ("x",)),
}


def _wrong_dtype(t):
    return t.to(WRONG_DTYPE[t.dtype])


def _non_contiguous(t):
    # the same values behind a stride of two in the last dimension
    wide = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], device=DEV, dtype=t.dtype)
    v = wide[..., ::2]
    v.copy_(t)
    assert not v.is_contiguous()
    return v


def _wrong_dim(t):
    # 8 more columns (one more element of a vector): rows stay 16-byte multiples
    extra = 8 if t.dim() == 2 else 1
    return torch.cat([t, t[..., :extra]], dim=-1).contiguous()


def _offset8(t):
    # a contiguous view that starts 4 bf16 elements into a larger buffer
    buf = torch.zeros(4 + t.numel(), device=DEV, dtype=t.dtype)
    v = buf[4:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 8
    return v


def _spoilings(spec, vectors, activations):
    for name, (_, shape) in spec.items():
        yield name, "dtype", _wrong_dtype
        yield name, "non-contiguous", _non_contiguous
        if name in vectors:
            yield name, "length", _wrong_dim
        else:
            yield name, "dimension", _wrong_dim
    for name in activations:
        yield name, "8-byte offset", _offset8


@pytest.mark.parametrize("binding", sorted(CASES))
def test_binding_refuses_spoiled_operands(binding):
    ext = ops.ext()
    spec, call, vectors, activations = CASES[binding]
    good = _operands(torch.Generator(device=DEV).manual_seed(7), spec)
    for t in good.values():
        assert t.data_ptr() % 16 == 0
    # the valid call runs (on copies: it accumulates into dw / db)
    call(ext, {k: v.clone() for k, v in good.items()})
    torch.cuda.synchronize()
    n = 0
    for name, what, spoil in _spoilings(spec, vectors, activations):
        args = dict(good)
        args[name] = spoil(good[name])
        before = {k: v.clone() for k, v in args.items()}
        with pytest.raises(RuntimeError):
            call(ext, args)
            pytest.fail("%s accepted %s with a wrong %s" % (binding, name, what))
        torch.cuda.synchronize()
        for k, v in args.items():
            assert torch.equal(v, before[k]), "%s: %s changed after a refused call (%s %s)" % (
                binding, k, name, what)
        n += 1
    assert n >= 3 * len(spec)
