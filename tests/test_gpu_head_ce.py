"""One-pass head forward + cross-entropy + head backward (linear_head_ce,
head_bwd.hip's head_ce_kernel) against the three launches it replaces
(linear_fwd -> ce_fused -> linear_head_bwd) and fp32 references, and the
trainer route built on it (mlp_chain_ce_step)."""

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped off-GPU
    pytest.skip("needs MI355X", allow_module_level=True)

from sparktorch_amd import ops
from sparktorch_amd.ops import functional as Fn
from sparktorch_amd.ops.modules import MnistMLPFused

DEV = "cuda:0"
TOL = 0.02  # max|a - ref| / max|ref| against fp32 torch
ATOMIC = 1e-5  # of max|ref|: fp32 atomic-order differences of dw / db
LOSS_REL = 2e-6  # atomic-order noise of the fp32 loss sum


def bf(x):
    return x.to(torch.bfloat16)


def bits(t):
    return t.view(torch.int16)


def rel_err(a, ref):
    return ((a.float() - ref).abs().max() / (ref.abs().max() + 1e-12)).item()


def relu_like(shape, seed):
    """bf16 'saved ReLU output' holding 0.0, -0.0, negative and positive entries."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    y = torch.randn(shape, device=DEV, generator=g)
    flat = y.view(-1)
    flat[0::5] = 0.0
    flat[1::5] = -0.0
    flat[2] = -1.5
    flat[3] = 2.0
    y = bf(y).contiguous()
    b = bits(y).view(-1)
    assert (b == 0).any() and (b == -32768).any()  # +0 and -0 present
    assert (y < 0).any() and (y > 0).any()
    return y


def _case(B, C, H, with_bias, seed, w_scale=0.1):
    torch.manual_seed(seed)
    w = bf(torch.randn(C, H, device=DEV) * w_scale).contiguous()
    bias = torch.randn(C, device=DEV) if with_bias else None
    y = relu_like((B, H), seed + 1)
    t = torch.randint(0, C, (B,), device=DEV)
    return y, w, bias, t


def _three_steps(y, w, bias, t, with_db, max_blocks=0):
    """The launches the kernel replaces, through the raw bindings."""
    ext = ops.ext()
    C, H = w.shape
    logits = ext.linear_fwd(y, w, bias, False)
    loss, dlogits = ext.ce_fused(logits, t)
    dw = torch.zeros(C, H, device=DEV)
    db = torch.zeros(C, device=DEV) if with_db else None
    dz = Fn.linear_head_bwd(dlogits, w, y, dw, db, max_blocks)
    return logits, loss, dz, dw, db


def _fp32_reference(y, w, bias, t):
    """dw / db in fp32 torch from the bf16-rounded logits and dlogits."""
    B, C = y.shape[0], w.shape[0]
    z = y.float() @ w.float().t()
    if bias is not None:
        z = z + bias
    z = bf(z).float()
    p = torch.softmax(z, dim=1)
    p[torch.arange(B, device=DEV), t] -= 1.0
    dl = bf(p / B).float()
    return dl.t() @ y.float(), dl.sum(0)


def _check(B, C, H, with_bias, with_db, max_blocks=0, seed=50, w_scale=0.1):
    tag = "B=%d C=%d H=%d bias=%d db=%d mb=%d" % (B, C, H, with_bias, with_db, max_blocks)
    y, w, bias, t = _case(B, C, H, with_bias, seed, w_scale)
    logits0, loss0, dz0, dw0, db0 = _three_steps(y, w, bias, t, with_db, max_blocks)
    ref_dw, ref_db = _fp32_reference(y, w, bias, t)

    dw = torch.zeros(C, H, device=DEV)
    db = torch.zeros(C, device=DEV) if with_db else None
    loss, dz, logits = Fn.linear_head_ce(y, w, bias, t, dw, db, True, max_blocks)
    l0, l1 = loss0.item(), loss.item()
    print(tag, "loss %.7g vs %.7g  dw %.2e / fp32 %.2e" % (
        l1, l0, (dw - dw0).abs().max().item(), rel_err(dw, ref_dw)))

    assert logits.shape == (B, C) and logits.dtype == torch.bfloat16, tag
    assert torch.equal(logits, logits0), tag
    assert dz.shape == (B, H) and dz.dtype == torch.bfloat16, tag
    assert torch.equal(bits(dz), bits(dz0)), tag
    assert (bits(dz) == 0)[~(y > 0)].all(), tag
    assert loss.shape == () and loss.dtype == torch.float32 and torch.isfinite(loss), tag
    assert abs(l1 - l0) <= LOSS_REL * abs(l0), (tag, l1, l0)
    assert (dw - dw0).abs().max() <= ATOMIC * dw0.abs().max() + 1e-30, tag
    assert rel_err(dw, ref_dw) < TOL, tag
    if with_db:
        assert (db - db0).abs().max() <= ATOMIC * db0.abs().max() + 1e-30, tag
        assert rel_err(db, ref_db) < TOL, tag
    return (y, w, bias, t), (loss, dz, dw, db)


@pytest.mark.parametrize("H", [64, 128, 256, 512])
@pytest.mark.parametrize("C", [1, 3, 10, 16])
def test_head_ce_matches_three_steps(C, H):
    assert ops.ext().head_bwd_supported(C, H)
    for B in (1, 63, 64, 65, 129, 1000):
        for with_bias in (True, False):
            for with_db in (True, False):
                _check(B, C, H, with_bias, with_db)


@pytest.mark.parametrize("H", [64, 128, 256, 512])
def test_head_ce_several_tiles_per_block(H):
    """max_blocks=2: each block walks many tiles and ends on a partial one."""
    _check(1000, 10, H, True, True, max_blocks=2)


@pytest.mark.parametrize("C,H", [(3, 64), (10, 256), (16, 512)])
def test_head_ce_across_ce_kernel_threshold(C, H):
    """Above batch 2048 ce_fused sums a row's exponentials class by class
    instead of by lane butterfly; the fused kernel follows it bit for bit."""
    for B in (2048, 2049, 4100):
        _check(B, C, H, True, True, seed=55)


def test_head_ce_no_logits_requested():
    y, w, bias, t = _case(129, 10, 256, True, 51)
    dw = torch.zeros(10, 256, device=DEV)
    loss, dz, logits = Fn.linear_head_ce(y, w, bias, t, dw, None)
    assert logits is None
    _, loss0, dz0, dw0, _ = _three_steps(y, w, bias, t, False)
    assert torch.equal(bits(dz), bits(dz0))
    assert abs(loss.item() - loss0.item()) <= LOSS_REL * abs(loss0.item())
    assert (dw - dw0).abs().max() <= ATOMIC * dw0.abs().max()


@pytest.mark.parametrize("H", [64, 256, 512])
def test_head_ce_accumulates_grads_defines_loss(H):
    (y, w, bias, t), (loss1, dz1, dw, db) = _check(1000, 10, H, True, True, seed=52)
    dw1, db1 = dw.clone(), db.clone()
    loss2, dz2, _ = Fn.linear_head_ce(y, w, bias, t, dw, db)
    assert torch.equal(bits(dz2), bits(dz1))
    assert (dw - 2 * dw1).abs().max() <= ATOMIC * dw1.abs().max()
    assert (db - 2 * db1).abs().max() <= ATOMIC * db1.abs().max()
    assert abs(loss2.item() - loss1.item()) <= LOSS_REL * abs(loss1.item())


@pytest.mark.parametrize("B", [65, 1000])
def test_head_ce_large_logits(B):
    """w scaled so the logits reach about +-80: exponentials underflow, the
    loss is tens of units; everything stays finite and on the old route's bits."""
    (y, w, bias, t), (loss, dz, dw, db) = _check(B, 10, 256, True, True, seed=53, w_scale=1.6)
    z = ops.ext().linear_fwd(y, w, bias, False).float()
    assert z.abs().max() > 60, z.abs().max()
    assert torch.isfinite(loss) and torch.isfinite(dz.float()).all()
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()


@pytest.mark.parametrize("C,H", [(17, 64), (10, 96)])
def test_head_ce_fallback_route(C, H):
    assert not ops.ext().head_bwd_supported(C, H)
    for B in (1, 129, 1000):
        _check(B, C, H, True, True)
    y, w, bias, t = _case(8, C, H, True, 54)
    with pytest.raises(RuntimeError):
        ops.ext().linear_head_ce(y, w, bias, t, torch.zeros(C, H, device=DEV), None)


def test_head_ce_flag_off_takes_three_steps(monkeypatch):
    monkeypatch.setattr(Fn, "_HEAD_CE_FUSION", False)
    real = ops.ext()
    monkeypatch.setattr(Fn.ops, "ext", lambda: _ExtProxy(real))
    _check(129, 10, 64, True, True)


class _ExtProxy:
    """The extension with linear_head_ce replaced by a tripwire."""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        if name == "linear_head_ce":
            raise AssertionError("fused kernel reached")
        return getattr(self._real, name)


# ---------------------------------------------------------------------------
# trainer route
# ---------------------------------------------------------------------------

DIMS = (40, 64, 10)
BATCH = 300


def _model_and_batch():
    torch.manual_seed(60)
    model = MnistMLPFused(*DIMS).to(DEV)
    x = bf(torch.randn(BATCH, DIMS[0], device=DEV))
    t = torch.randint(0, DIMS[2], (BATCH,), device=DEV)
    return model, x, t


def _twin(model):
    twin = MnistMLPFused(*DIMS).to(DEV)
    twin.load_state_dict(model.state_dict())
    return twin


def _trainer(model, compile_mode=None, criterion=None):
    from sparktorch_amd.parallel.sync import SyncTrainer

    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    return SyncTrainer(model, criterion or nn.CrossEntropyLoss(), opt, device=DEV,
                       world_size=1, compile_mode=compile_mode)


def _count_calls(monkeypatch):
    calls = []
    real = Fn.linear_head_ce

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(Fn, "linear_head_ce", counted)
    return calls


def _tripwire(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("linear_head_ce reached on a route that must not take it")

    monkeypatch.setattr(Fn, "linear_head_ce", boom)


def test_trainer_step_fused_vs_unfused(monkeypatch):
    model, x, t = _model_and_batch()
    twin = _twin(model)
    calls = _count_calls(monkeypatch)
    ta = _trainer(model)
    la = ta.train_step(x, t)
    assert len(calls) == 1  # the new route ran
    monkeypatch.setattr(Fn, "_HEAD_CE_FUSION", False)
    tb = _trainer(twin)
    lb = tb.train_step(x, t)
    assert len(calls) == 1  # and the flag turns it off
    print("loss fused %.7g unfused %.7g" % (la, lb))
    assert abs(la - lb) <= LOSS_REL * abs(lb), (la, lb)
    for (k, p), (_, q) in zip(ta.model.named_parameters(), tb.model.named_parameters()):
        assert p.grad is not None and q.grad is not None, k
        assert (p.grad - q.grad).abs().max() <= ATOMIC * q.grad.abs().max(), k


def test_trainer_hipgraph_vs_eager(monkeypatch):
    """Three graphed steps track three eager steps, both on the new route, to
    the 1e-3 of the loss the chain's graph test uses."""
    model, x, t = _model_and_batch()
    twin = _twin(model)
    calls = _count_calls(monkeypatch)
    te, tg = _trainer(model), _trainer(twin, compile_mode="hipgraph")
    le = [te.train_step(x, t) for _ in range(3)]
    assert len(calls) == 3
    lg = [tg.train_step(x, t) for _ in range(3)]
    assert len(calls) == 6  # two warmup steps and the capture
    print("eager", le, "graph", lg)
    assert le[-1] < le[0]
    for a, b in zip(le, lg):
        assert abs(a - b) <= 1e-3 * abs(a)


def test_trainer_keeps_old_route_without_direct_grads(monkeypatch):
    model, x, t = _model_and_batch()
    tr = _trainer(model)
    tr.buckets.remove_hooks()  # no parameter is bucket-direct any more
    _tripwire(monkeypatch)
    l0 = tr.train_step(x, t)
    l1 = tr.train_step(x, t)
    assert l0 == l0 and l1 < l0


def test_trainer_keeps_old_route_with_frozen_parameter(monkeypatch):
    model, x, t = _model_and_batch()
    model.fc1.bias.requires_grad_(False)
    tr = _trainer(model)
    _tripwire(monkeypatch)
    l0 = tr.train_step(x, t)
    assert l0 == l0


def test_trainer_keeps_old_route_for_other_criterion(monkeypatch):
    model, x, t = _model_and_batch()
    tr = _trainer(model, criterion=nn.MSELoss())
    _tripwire(monkeypatch)
    onehot = bf(torch.nn.functional.one_hot(t, DIMS[2]).float())
    l0 = tr.train_step(x, onehot)
    assert l0 == l0


def test_model_call_and_validation_untouched(monkeypatch):
    model, x, t = _model_and_batch()
    tr = _trainer(model)
    _tripwire(monkeypatch)
    with torch.no_grad():
        z = tr.model(x)
    assert z.shape == (BATCH, DIMS[2])
    assert tr.validation_loss(x, t) > 0
