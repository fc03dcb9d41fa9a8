"""linear_mse (linear_mse.hip) against the two launches it replaces
(linear_fwd -> mse_fused) and fp64, the autoencoder train step built on it
(mlp_chain_mse_step with a wide head) and the trainer route.  Bounds are
test_gpu_head_mse.py's: TOL against fp64, ATOMIC for fp32 atomic-order
differences of dW / db, and for the loss twice the two-step route's own error
against the fp64 mean over the bf16 values, floor LOSS_REL."""

import itertools

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped off-GPU
    pytest.skip("needs MI355X", allow_module_level=True)

from sparktorch_amd import ops
from sparktorch_amd.ops import functional as Fn
from sparktorch_amd.ops.modules import MLPAutoEncoderFused
from sparktorch_amd.parallel import sync
from sparktorch_amd.parallel.buckets import FlatBuckets

DEV = "cuda:0"
TOL = 0.02  # max|a - ref| / max|ref| against fp64
ATOMIC = 1e-5  # of max|ref|: fp32 atomic-order differences of dw / db
LOSS_REL = 2e-6  # atomic-order noise of the fp32 loss sum


@pytest.fixture(autouse=True)
def _any_batch(monkeypatch):
    """the measured row threshold would keep these small batches off the kernel"""
    monkeypatch.setattr(Fn, "_LINEAR_MSE_MIN_ROWS", 1)


def _count_kernel_calls(monkeypatch):
    calls, real = [], ops.ext().linear_mse
    monkeypatch.setattr(ops.ext(), "linear_mse", lambda *a, **k: calls.append(1) or real(*a, **k))
    return calls


def bf(x):
    return x.to(torch.bfloat16)


def bits(t):
    return t.view(torch.int16)


def _loss_ok(fused, old, ref):
    e1, e0 = abs(fused - ref), abs(old - ref)
    print("loss err fused %.3e two-step %.3e of %.7g (rel %.2e)" % (e1, e0, ref, e1 / abs(ref)))
    return e1 <= max(2 * e0, LOSS_REL * abs(ref))


def _check(B, N, H, with_bias, max_blocks=0, seed=90):
    """fused against linear_fwd -> mse_fused and fp64 at one case"""
    tag = "B=%d N=%d H=%d bias=%d mb=%d" % (B, N, H, with_bias, max_blocks)
    torch.manual_seed(seed)
    y = bf(torch.relu(torch.randn(B, H, device=DEV))).contiguous()
    w = bf(torch.randn(N, H, device=DEV) * 0.1).contiguous()
    bias = torch.randn(N, device=DEV) if with_bias else None
    t = bf(torch.randn(B, N, device=DEV)).contiguous()
    ext = ops.ext()
    pred0 = ext.linear_fwd(y, w, bias, False)
    loss0, dpred0 = ext.mse_fused(pred0, t)
    d = pred0.double() - t.double()  # fp64 from the bf16-rounded pred
    ref_loss, ref_dp = (d * d).mean().item(), 2 * d / d.numel()

    loss, dpred, pred = Fn.linear_mse(y, w, bias, t, True, max_blocks)
    assert pred.shape == (B, N) and torch.equal(bits(pred), bits(pred0)), tag
    assert dpred.shape == (B, N) and torch.equal(bits(dpred), bits(dpred0)), tag
    assert ((dpred.double() - ref_dp).abs().max() / ref_dp.abs().max()).item() < TOL, tag
    assert loss.shape == () and loss.dtype == torch.float32, tag
    assert _loss_ok(loss.item(), loss0.item(), ref_loss), tag
    loss2, dpred2, none = Fn.linear_mse(y, w, bias, t, False, max_blocks)  # loss is defined
    assert none is None and torch.equal(bits(dpred2), bits(dpred0)), tag
    assert abs(loss2.item() - loss.item()) <= LOSS_REL * abs(ref_loss), tag


@pytest.mark.parametrize("H", [64, 128, 256])
@pytest.mark.parametrize("N", [32, 48, 784, "chunk+16"])
def test_linear_mse_matches_two_steps(monkeypatch, N, H):
    if N == "chunk+16":  # one full column chunk and a one-fragment tail
        N = ops.ext().linear_mse_chunk_cols(H) + 16
    assert ops.ext().linear_mse_supported(N, H)
    calls = _count_kernel_calls(monkeypatch)
    for B, with_bias in itertools.product((1, 127, 128, 129, 1000), (True, False)):
        _check(B, N, H, with_bias)
    assert len(calls) == 20  # the kernel ran, with and without pred


@pytest.mark.parametrize("H", [64, 128, 256])
@pytest.mark.parametrize("N", [48, 784])
def test_linear_mse_several_tiles_per_block(monkeypatch, N, H):
    """each block walks four tiles (the flat (tile, chunk) walk), the last partial"""
    calls = _count_kernel_calls(monkeypatch)
    _check(1000, N, H, True, max_blocks=2)
    assert len(calls) == 2


@pytest.mark.parametrize("N,H,flag", [(24, 96, True), (48, 64, False)])
def test_linear_mse_fallback_route(monkeypatch, N, H, flag):
    """an unserved shape or the flag off: two-step results, no fused binding"""
    monkeypatch.setattr(Fn, "_LINEAR_MSE_FUSION", flag)
    monkeypatch.setattr(ops.ext(), "linear_mse", None)  # calling it raises
    for B in (1, 129):
        _check(B, N, H, True)
    monkeypatch.setattr(Fn, "_LINEAR_MSE_FUSION", True)
    monkeypatch.setattr(Fn, "_LINEAR_MSE_MIN_ROWS", None)  # and below the measured threshold
    _check(Fn.linear_mse_min_rows() - 1, 48, 64, True)


def _chain_step(dims, x, state=None):
    torch.manual_seed(91)
    model = MLPAutoEncoderFused(dims[0], dims[1:]).to(DEV)
    if state is not None:
        model.load_state_dict(state)
    fb = FlatBuckets(list(model.parameters()), world_size=1)
    fb.register_hooks()
    fb.zero_grad()
    loss = Fn.mlp_chain_mse_step(x, model._layers(), x)
    fb.finalize(average=False)
    return model, loss.item(), [p.grad.clone() for p in model.parameters()]


@pytest.mark.parametrize("dims", [(32, 64), (48, 128, 64)])
def test_chain_step_wide_head_vs_unfused(monkeypatch, dims):
    """the autoencoder step, its target the input tensor itself"""
    torch.manual_seed(92)
    x = bf(torch.randn(300, dims[0], device=DEV)).contiguous()
    calls = _count_kernel_calls(monkeypatch)
    model, loss, grads = _chain_step(dims, x)
    assert Fn.mlp_chain_mse_supported(x, model._layers(), x) and len(calls) == 1
    monkeypatch.setattr(Fn, "_LINEAR_MSE_FUSION", False)
    assert not Fn.mlp_chain_mse_supported(x, model._layers(), x)
    _, loss0, grads0 = _chain_step(dims, x, model.state_dict())
    assert len(calls) == 1
    with torch.no_grad():
        ref = ((model(x).double() - x.double()) ** 2).mean().item()
    assert _loss_ok(loss, loss0, ref)
    for (k, _), g, g0 in zip(model.named_parameters(), grads, grads0):
        assert g0.abs().max() > 0 and (g - g0).abs().max() <= ATOMIC * g0.abs().max(), k


def _trainer(state=None, compile_mode=None):
    torch.manual_seed(93)
    model = MLPAutoEncoderFused(32, (64,)).to(DEV)
    if state is not None:
        model.load_state_dict(state)
    return sync.SyncTrainer(model, nn.MSELoss(), torch.optim.SGD(model.parameters(), lr=0.05),
                            device=DEV, world_size=1, compile_mode=compile_mode)


def test_trainer_autoencoder_fused_vs_unfused_vs_graph(monkeypatch):
    torch.manual_seed(94)
    x = bf(torch.randn(200, 32, device=DEV))
    ta = _trainer()
    state = {k: v.clone() for k, v in ta.model.state_dict().items()}
    tg = _trainer(state, compile_mode="hipgraph")
    calls = _count_kernel_calls(monkeypatch)
    la = [ta.train_step(x, x)]
    after_one = [p.detach().clone() for p in ta.model.parameters()]
    la += [ta.train_step(x, x) for _ in range(2)]
    assert len(calls) == 3  # the new route ran
    lg = [tg.train_step(x, x) for _ in range(3)]
    assert len(calls) > 3
    n = len(calls)
    monkeypatch.setattr(Fn, "_LINEAR_MSE_FUSION", False)
    tb = _trainer(state)
    lb = tb.train_step(x, x)
    assert len(calls) == n  # and the flag turns it off
    with torch.no_grad():
        pred = _trainer(state).model(x)
    ref = ((pred.double() - x.double()) ** 2).mean().item()
    assert _loss_ok(la[0], lb, ref)
    assert la[-1] < la[0]
    for a, g in zip(la, lg):  # the chain's graph test's bound
        assert abs(a - g) <= 1e-3 * abs(a)
    for p, (k, q) in zip(after_one, tb.model.named_parameters()):  # one step each
        assert (p - q).abs().max() <= ATOMIC * q.abs().max(), k
