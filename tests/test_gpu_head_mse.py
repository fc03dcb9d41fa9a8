"""linear_head_mse (head_bwd.hip's head_mse_kernel) against the three launches
it replaces (linear_fwd -> mse_fused -> linear_head_bwd) and fp64, and the
trainer route built on it.  Loss bound: against the fp64 mean of
(pred - target)^2 over the bf16 values, twice the three-step route's own error
at the same case, floor LOSS_REL."""

import itertools

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped off-GPU
    pytest.skip("needs MI355X", allow_module_level=True)

from sparktorch_amd import ops
from sparktorch_amd.ops import functional as Fn
from sparktorch_amd.ops.modules import MnistMLPFused
from sparktorch_amd.parallel import sync

DEV = "cuda:0"
TOL = 0.02  # max|a - ref| / max|ref| against fp64
ATOMIC = 1e-5  # of max|ref|: fp32 atomic-order differences of dw / db
LOSS_REL = 2e-6  # atomic-order noise of the fp32 loss sum


def bf(x):
    return x.to(torch.bfloat16)


def bits(t):
    return t.view(torch.int16)


def rel_err(a, ref):
    return ((a.double() - ref).abs().max() / (ref.abs().max() + 1e-300)).item()


def _case(B, C, H, with_bias, seed):
    """y: a 'saved ReLU output' holding 0.0, -0.0, negative and positive entries"""
    torch.manual_seed(seed)
    w = bf(torch.randn(C, H, device=DEV) * 0.1).contiguous()
    bias = torch.randn(C, device=DEV) if with_bias else None
    t = bf(torch.randn(B, C, device=DEV)).contiguous()
    y = torch.randn(B, H, device=DEV)
    flat = y.view(-1)
    flat[0::5], flat[1::5], flat[2], flat[3] = 0.0, -0.0, -1.5, 2.0
    y = bf(y).contiguous()
    assert (bits(y) == 0).any() and (bits(y) == -32768).any() and (y < 0).any() and (y > 0).any()
    return y, w, bias, t


def _three_steps(y, w, bias, t, with_db, max_blocks=0):
    ext = ops.ext()
    pred = ext.linear_fwd(y, w, bias, False)
    loss, dpred = ext.mse_fused(pred, t)
    dw = torch.zeros_like(w, dtype=torch.float32)
    db = torch.zeros(w.shape[0], device=DEV) if with_db else None
    dz = Fn.linear_head_bwd(dpred, w, y, dw, db, max_blocks)
    return pred, loss, dz, dw, db


def _loss_ok(fused, old, ref):
    e1, e0 = abs(fused - ref), abs(old - ref)
    print("loss err fused %.3e three-step %.3e of %.7g" % (e1, e0, ref))
    return e1 <= max(2 * e0, LOSS_REL * abs(ref))


def _check(B, C, H, with_bias, with_db, max_blocks=0, seed=70):
    tag = "B=%d C=%d H=%d bias=%d db=%d mb=%d" % (B, C, H, with_bias, with_db, max_blocks)
    y, w, bias, t = _case(B, C, H, with_bias, seed)
    pred0, loss0, dz0, dw0, db0 = _three_steps(y, w, bias, t, with_db, max_blocks)
    # fp64 from the bf16-rounded pred and dpred
    d = pred0.double() - t.double()
    ref_loss = (d * d).mean().item()
    dp = bf((2 * d / d.numel()).float()).double()
    ref_dw, ref_db = dp.t() @ y.double(), dp.sum(0)

    dw = torch.zeros_like(dw0)
    db = torch.zeros_like(db0) if with_db else None
    loss, dz, pred = Fn.linear_head_mse(y, w, bias, t, dw, db, True, max_blocks)
    print(tag, "dw %.2e / fp64 %.2e" % ((dw - dw0).abs().max().item(), rel_err(dw, ref_dw)))
    assert pred.shape == (B, C) and torch.equal(bits(pred), bits(pred0)), tag
    assert dz.shape == (B, H) and torch.equal(bits(dz), bits(dz0)), tag
    assert (bits(dz) == 0)[~(y > 0)].all(), tag
    assert loss.shape == () and loss.dtype == torch.float32, tag
    assert _loss_ok(loss.item(), loss0.item(), ref_loss), tag
    assert (dw - dw0).abs().max() <= ATOMIC * dw0.abs().max() + 1e-30, tag
    assert rel_err(dw, ref_dw) < TOL, tag
    if with_db:
        assert (db - db0).abs().max() <= ATOMIC * db0.abs().max() + 1e-30, tag
        assert rel_err(db, ref_db) < TOL, tag
    return (y, w, bias, t), (loss, dz, dw, db)


@pytest.mark.parametrize("H", [64, 128, 256, 512])
@pytest.mark.parametrize("C", [1, 3, 16])
def test_head_mse_matches_three_steps(C, H):
    assert ops.ext().head_bwd_supported(C, H)
    for B, with_bias, with_db in itertools.product((1, 63, 64, 65, 129, 1000), (True, False),
                                                   (True, False)):
        _check(B, C, H, with_bias, with_db)


@pytest.mark.parametrize("H", [64, 128, 256, 512])
def test_head_mse_several_tiles_per_block(H):
    """each block walks many tiles (target prefetch, lane loss sums), the last partial"""
    _check(1000, 3, H, True, True, max_blocks=2)


@pytest.mark.parametrize("H", [64, 512])
def test_head_mse_accumulates_grads_defines_loss(H):
    (y, w, bias, t), (loss, dz1, dw, db) = _check(1000, 3, H, True, True, seed=71)
    dw1, db1, l1 = dw.clone(), db.clone(), loss.item()
    loss2, dz2, pred = Fn.linear_head_mse(y, w, bias, t, dw, db)
    assert pred is None  # want_pred=False
    assert torch.equal(bits(dz2), bits(dz1))
    assert (dw - 2 * dw1).abs().max() <= ATOMIC * dw1.abs().max()
    assert (db - 2 * db1).abs().max() <= ATOMIC * db1.abs().max()
    assert abs(loss2.item() - l1) <= LOSS_REL * abs(l1)


@pytest.mark.parametrize("C,H,flag", [(17, 64, True), (3, 96, True), (3, 64, False)])
def test_head_mse_fallback_route(monkeypatch, C, H, flag):
    """an unserved shape or the flag off: three-step results, no fused binding"""
    monkeypatch.setattr(Fn, "_HEAD_MSE_FUSION", flag)
    monkeypatch.setattr(ops.ext(), "linear_head_mse", None)  # calling it raises
    for B in (1, 129):
        _check(B, C, H, True, True)


def _trainer(classes, state=None, compile_mode=None, criterion=None):
    torch.manual_seed(80)
    model = MnistMLPFused(32, 64, classes).to(DEV)
    if state is not None:
        model.load_state_dict(state)
    return sync.SyncTrainer(model, criterion or nn.MSELoss(),
                            torch.optim.SGD(model.parameters(), lr=0.05), device=DEV,
                            world_size=1, compile_mode=compile_mode)


def _batch(classes):
    torch.manual_seed(81)
    return bf(torch.randn(200, 32, device=DEV)), torch.randn(200, classes, device=DEV)


def _count_calls(monkeypatch):
    calls, real = [], Fn.linear_head_mse
    monkeypatch.setattr(Fn, "linear_head_mse", lambda *a, **k: calls.append(1) or real(*a, **k))
    return calls


@pytest.mark.parametrize("classes", [1, 3])
def test_trainer_step_fused_vs_unfused_vs_graph(monkeypatch, classes):
    x, y = _batch(classes)
    ta = _trainer(classes)
    state = {k: v.clone() for k, v in ta.model.state_dict().items()}
    tg = _trainer(classes, state, compile_mode="hipgraph")
    calls = _count_calls(monkeypatch)
    la = [ta.train_step(x, y)]
    after_one = [p.detach().clone() for p in ta.model.parameters()]
    la += [ta.train_step(x, y) for _ in range(2)]
    assert len(calls) == 3  # the new route ran
    lg = [tg.train_step(x, y) for _ in range(3)]
    assert len(calls) == 6  # two warmup steps and the capture
    monkeypatch.setattr(Fn, "_HEAD_MSE_FUSION", False)
    tb = _trainer(classes, state)
    lb = tb.train_step(x, y)
    assert len(calls) == 6  # and the flag turns it off
    # fp64 loss of the first step from the old route's own bf16 predictions
    with torch.no_grad():
        pred = _trainer(classes, state).model(x)
    ref = ((pred.double() - bf(y).double()) ** 2).mean().item()
    assert _loss_ok(la[0], lb, ref)
    assert la[-1] < la[0]
    for a, g in zip(la, lg):  # the chain's graph test's bound
        assert abs(a - g) <= 1e-3 * abs(a)
    for p, (k, q) in zip(after_one, tb.model.named_parameters()):  # one step each
        assert (p - q).abs().max() <= ATOMIC * q.abs().max(), k


def test_trainer_keeps_autograd_route(monkeypatch):
    """No labels (autoencoder mode hands y=None down) and any criterion but
    HipMSE go through compute_loss, never through linear_head_mse."""
    x, y = _batch(3)
    seen = []
    real = sync.compute_loss
    monkeypatch.setattr(sync, "compute_loss",
                        lambda c, p, t: seen.append(1) or real(c, p, t if t is not None else y))
    calls = _count_calls(monkeypatch)
    _trainer(3).train_step(x, None)
    _trainer(3, criterion=nn.L1Loss()).train_step(x, y)
    assert len(seen) == 2 and not calls
