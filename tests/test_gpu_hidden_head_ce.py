"""The last hidden layer's forward fused into the head's loss pass
(linear_hidden_head_ce, hidden_head_ce.hip) against the two launches it
replaces (linear_fwd -> linear_head_ce) on the same tensors, and the trainer
route built on it (mlp_chain_ce_step).

h2, the logits and dz2 must match bit for bit; the loss, dw3 and db3 differ by
the order of fp32 atomics only and keep test_gpu_head_ce.py's tolerances."""

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
# tests/test_gpu_head_ce.py's tolerances for the same quantities
ATOMIC = 1e-5  # of max|ref|: fp32 atomic-order differences of dw / db
LOSS_REL = 2e-6  # atomic-order noise of the fp32 loss sum

PAIRS = [(k, h) for h in (128, 256) for k in range(32, 257, 32)]  # every served (K_in, H)


def bf(x):
    return x.to(torch.bfloat16)


def bits(t):
    return t.view(torch.int16)


def _case(B, K, H, C, bias2, bias3, seed, w3_scale=0.1, b2_value=None):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = bf(torch.randn(B, K, device=DEV, generator=g)).contiguous()
    w2 = bf(torch.randn(H, K, device=DEV, generator=g) * 0.1).contiguous()
    w3 = bf(torch.randn(C, H, device=DEV, generator=g) * w3_scale).contiguous()
    b2 = torch.randn(H, device=DEV, generator=g) if bias2 else None
    if b2_value is not None:
        b2 = torch.full((H,), float(b2_value), device=DEV)
    b3 = torch.randn(C, device=DEV, generator=g) if bias3 else None
    t = torch.randint(0, C, (B,), device=DEV, generator=g)
    return x, w2, b2, w3, b3, t


def _pair(x, w2, b2, w3, b3, t, with_db, max_blocks=0):
    """The two launches the kernel replaces."""
    C, H = w3.shape
    h2 = ops.ext().linear_fwd(x, w2, b2, True)
    dw = torch.zeros(C, H, device=DEV)
    db = torch.zeros(C, device=DEV) if with_db else None
    loss, dz, logits = Fn.linear_head_ce(h2, w3, b3, t, dw, db, True, max_blocks)
    return h2, logits, loss, dz, dw, db


def _fused(x, w2, b2, w3, b3, t, with_db, max_blocks=0, dw=None, db=None):
    """The kernel through the raw binding: no threshold, no fallback."""
    C, H = w3.shape
    if dw is None:
        dw = torch.zeros(C, H, device=DEV)
        db = torch.zeros(C, device=DEV) if with_db else None
    loss, dz, logits, h2 = ops.ext().linear_hidden_head_ce(x, w2, b2, w3, b3, t, dw, db, True,
                                                           True, max_blocks)
    return h2, logits, loss, dz, dw, db


def _compare(got, want, tag):
    h2, logits, loss, dz, dw, db = got
    h2_0, logits0, loss0, dz0, dw0, db0 = want
    l1, l0 = loss.item(), loss0.item()
    print(tag, "loss %.7g vs %.7g  dw %.2e of %.2e" % (
        l1, l0, (dw - dw0).abs().max().item(), dw0.abs().max().item()))
    assert h2.shape == h2_0.shape and h2.dtype == torch.bfloat16, tag
    assert torch.equal(bits(h2), bits(h2_0)), tag
    assert torch.equal(bits(logits), bits(logits0)), tag
    assert dz.shape == dz0.shape and dz.dtype == torch.bfloat16, tag
    assert torch.equal(bits(dz), bits(dz0)), tag
    assert loss.shape == () and loss.dtype == torch.float32 and torch.isfinite(loss), tag
    assert abs(l1 - l0) <= LOSS_REL * abs(l0), (tag, l1, l0)
    assert (dw - dw0).abs().max() <= ATOMIC * dw0.abs().max() + 1e-30, tag
    if db0 is not None:
        assert (db - db0).abs().max() <= ATOMIC * db0.abs().max() + 1e-30, tag


def _check(B, K, H, C, bias2=True, bias3=True, with_db=True, max_blocks=0, seed=70, **kw):
    tag = "B=%d K=%d H=%d C=%d b2=%d b3=%d db=%d mb=%d" % (B, K, H, C, bias2, bias3, with_db,
                                                           max_blocks)
    case = _case(B, K, H, C, bias2, bias3, seed, **kw)
    want = _pair(*case, with_db, max_blocks)
    got = _fused(*case, with_db, max_blocks)
    _compare(got, want, tag)
    return case, got, want


@pytest.mark.parametrize("K,H", [(256, 256), (64, 128)])
def test_row_counts(K, H):
    """A partial tile, exactly one tile, a tile plus one row, and both sides of
    the batch at which ce_fused's summation order switches."""
    assert ops.ext().hidden_head_ce_supported(K, H, 10)
    for B in (1, 127, 128, 129, 257, 1000, 2047, 2048, 2049):
        _check(B, K, H, 10)


@pytest.mark.parametrize("K,H", [(256, 256), (96, 128)])
def test_several_tiles_per_block(K, H):
    """max_blocks=2: each block walks several tiles and ends on a partial one."""
    _check(1000, K, H, 10, max_blocks=2)


@pytest.mark.parametrize("K,H", PAIRS)
def test_every_served_pair(K, H):
    for C in (1, 10, 16):
        assert ops.ext().hidden_head_ce_supported(K, H, C)
        for bias2, bias3, with_db in ((True, True, True), (False, True, False),
                                      (True, False, True), (False, False, False)):
            _check(257, K, H, C, bias2, bias3, with_db, seed=71)


@pytest.mark.parametrize("K,H", [(256, 256), (128, 128)])
def test_dead_relu_rows(K, H):
    """b2 = -100: every h2 is 0, so dz2 and dw3 vanish, db3 does not, and the
    loss is that of the bias-only logits."""
    B, C = 300, 10
    case, got, _ = _check(B, K, H, C, seed=72, b2_value=-100.0)
    b3, t = case[4], case[5]
    h2, logits, loss, dz, dw, db = got
    assert (bits(h2) == 0).all()
    assert (bits(dz) == 0).all()
    assert (dw == 0).all()
    assert (db != 0).any()
    ref = nn.functional.cross_entropy(bf(b3).float().expand(B, C), t)
    # fp32 exp / log of the fast-math kind: a few ulp per row, averaged
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item()), (loss.item(), ref.item())


@pytest.mark.parametrize("B", [129, 1000])
def test_large_logits(B):
    """w3 scaled so the logits reach about +-80: exponentials underflow, the
    loss is tens of units; everything stays finite and on the pair's bits."""
    _, got, want = _check(B, 256, 256, 10, seed=73, w3_scale=1.6)
    h2, logits, loss, dz, dw, db = got
    assert want[1].float().abs().max() > 60, want[1].float().abs().max()
    assert torch.isfinite(loss) and torch.isfinite(dz.float()).all()
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()


@pytest.mark.parametrize("K,H", [(256, 256), (32, 128)])
def test_accumulates_grads_defines_loss(K, H):
    case, (h2, logits, loss1, dz1, dw, db), _ = _check(1000, K, H, 10, seed=74)
    dw1, db1 = dw.clone(), db.clone()
    _, _, loss2, dz2, _, _ = _fused(*case, True, dw=dw, db=db)
    assert torch.equal(bits(dz2), bits(dz1))
    assert (dw - 2 * dw1).abs().max() <= ATOMIC * dw1.abs().max()
    assert (db - 2 * db1).abs().max() <= ATOMIC * db1.abs().max()
    assert abs(loss2.item() - loss1.item()) <= LOSS_REL * abs(loss1.item())


def test_nothing_extra_requested():
    case = _case(129, 256, 256, 10, True, True, 75)
    dw = torch.zeros(10, 256, device=DEV)
    loss, dz, logits, h2 = ops.ext().linear_hidden_head_ce(*case, dw, None)
    assert logits.numel() == 0 and h2.numel() == 0
    _, _, loss0, dz0, dw0, _ = _pair(*case, False)
    assert torch.equal(bits(dz), bits(dz0))
    assert abs(loss.item() - loss0.item()) <= LOSS_REL * abs(loss0.item())
    assert (dw - dw0).abs().max() <= ATOMIC * dw0.abs().max()


class _ExtProxy:
    """The extension with linear_hidden_head_ce replaced by a tripwire."""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        if name == "linear_hidden_head_ce":
            raise AssertionError("fused kernel reached")
        return getattr(self._real, name)


def _wrapper(case, with_db=True):
    x, w2, b2, w3, b3, t = case
    C, H = w3.shape
    dw = torch.zeros(C, H, device=DEV)
    db = torch.zeros(C, device=DEV) if with_db else None
    loss, dz, logits, h2 = Fn.linear_hidden_head_ce(x, w2, b2, w3, b3, t, dw, db, True, True)
    return h2, logits, loss, dz, dw, db


@pytest.mark.parametrize("K,H,C", [(784, 256, 10), (256, 512, 10), (256, 256, 17)])
def test_fallback_unsupported_shape(monkeypatch, K, H, C):
    assert not ops.ext().hidden_head_ce_supported(K, H, C)
    monkeypatch.setattr(Fn, "_HIDDEN_HEAD_CE_MIN_ROWS", 1)
    real = ops.ext()
    monkeypatch.setattr(Fn.ops, "ext", lambda: _ExtProxy(real))
    case = _case(300, K, H, C, True, True, 76)
    _compare(_wrapper(case), _pair(*case, True), "fallback K=%d H=%d C=%d" % (K, H, C))
    with pytest.raises(RuntimeError):
        real.linear_hidden_head_ce(*case, torch.zeros(C, H, device=DEV), None)


def test_wrapper_takes_kernel_above_threshold_only(monkeypatch):
    case = _case(300, 256, 256, 10, True, True, 77)
    want = _pair(*case, True)
    calls = []
    real = ops.ext()

    class Counting(_ExtProxy):
        def __getattr__(self, name):
            if name == "linear_hidden_head_ce":
                calls.append(1)
            return getattr(self._real, name)

    monkeypatch.setattr(Fn.ops, "ext", lambda: Counting(real))
    assert Fn.hidden_head_ce_min_rows() == real.hidden_head_ce_min_rows() > 300
    _compare(_wrapper(case), want, "below threshold")
    assert not calls
    monkeypatch.setattr(Fn, "_HIDDEN_HEAD_CE_MIN_ROWS", 1)
    _compare(_wrapper(case), want, "threshold overridden")
    assert len(calls) == 1
    monkeypatch.setattr(Fn, "_HIDDEN_HEAD_CE_FUSION", False)
    _compare(_wrapper(case), want, "flag off")
    assert len(calls) == 1


# ---------------------------------------------------------------------------
# trainer route
# ---------------------------------------------------------------------------

DIMS = (64, 128, 10)
BATCH = 1000


def _model_and_batches(n=1):
    torch.manual_seed(80)
    model = MnistMLPFused(*DIMS).to(DEV)
    xs = [bf(torch.randn(BATCH, DIMS[0], device=DEV)) for _ in range(n)]
    ts = [torch.randint(0, DIMS[2], (BATCH,), device=DEV) for _ in range(n)]
    return model, xs, ts


def _twin(model):
    twin = MnistMLPFused(*DIMS).to(DEV)
    twin.load_state_dict(model.state_dict())
    return twin


def _trainer(model, compile_mode=None):
    from sparktorch_amd.parallel.sync import SyncTrainer

    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    return SyncTrainer(model, nn.CrossEntropyLoss(), opt, device=DEV, world_size=1,
                       compile_mode=compile_mode)


def _count_calls(monkeypatch):
    calls = []
    real = Fn.linear_hidden_head_ce

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(Fn, "linear_hidden_head_ce", counted)
    return calls


def test_trainer_step_fused_vs_unfused(monkeypatch):
    monkeypatch.setattr(Fn, "_HIDDEN_HEAD_CE_MIN_ROWS", 1)
    model, (x,), (t,) = _model_and_batches()
    twin = _twin(model)
    calls = _count_calls(monkeypatch)
    ta = _trainer(model)
    la = ta.train_step(x, t)
    assert len(calls) == 1  # the new route ran
    monkeypatch.setattr(Fn, "_HIDDEN_HEAD_CE_FUSION", False)
    tb = _trainer(twin)
    lb = tb.train_step(x, t)
    assert len(calls) == 1  # and the flag turns it off
    print("loss fused %.7g unfused %.7g" % (la, lb))
    assert abs(la - lb) <= LOSS_REL * abs(lb), (la, lb)
    for (k, p), (_, q) in zip(ta.model.named_parameters(), tb.model.named_parameters()):
        assert p.grad is not None and q.grad is not None, k
        if k.startswith("fc3"):
            assert (p.grad - q.grad).abs().max() <= ATOMIC * q.grad.abs().max(), k
        else:
            assert torch.equal(p.grad, q.grad), k


def test_trainer_hipgraph_vs_eager(monkeypatch):
    """Three graphed steps track three eager steps, both on the new route, to
    the 1e-3 of the loss the chain's graph test uses."""
    monkeypatch.setattr(Fn, "_HIDDEN_HEAD_CE_MIN_ROWS", 1)
    model, (x,), (t,) = _model_and_batches()
    twin = _twin(model)
    calls = _count_calls(monkeypatch)
    te, tg = _trainer(model), _trainer(twin, compile_mode="hipgraph")
    le = [te.train_step(x, t) for _ in range(3)]
    assert len(calls) == 3
    lg = [tg.train_step(x, t) for _ in range(3)]
    assert len(calls) > 3  # warmup steps and the capture went the same way
    print("eager", le, "graph", lg)
    assert le[-1] < le[0]
    for a, b in zip(le, lg):
        assert abs(a - b) <= 1e-3 * abs(a)


def test_trainer_three_batches_fused_vs_unfused(monkeypatch):
    """Different batches step after step: anything stale in the aliased LDS
    image or the loss scalar shows against the two-launch route."""
    monkeypatch.setattr(Fn, "_HIDDEN_HEAD_CE_MIN_ROWS", 1)
    model, xs, ts = _model_and_batches(3)
    twin = _twin(model)
    calls = _count_calls(monkeypatch)
    ta = _trainer(model)
    la = [ta.train_step(x, t) for x, t in zip(xs, ts)]
    assert len(calls) == 3
    monkeypatch.setattr(Fn, "_HIDDEN_HEAD_CE_FUSION", False)
    tb = _trainer(twin)
    lb = [tb.train_step(x, t) for x, t in zip(xs, ts)]
    assert len(calls) == 3
    print("fused", la, "unfused", lb)
    # step 1 starts from equal weights: the loss differs by atomic order only.
    # Later steps start from weights that already differ by that much, which
    # Adam's normalised update carries into the loss: the chain's 1e-3.
    assert abs(la[0] - lb[0]) <= LOSS_REL * abs(lb[0])
    for a, b in zip(la[1:], lb[1:]):
        assert abs(a - b) <= 1e-3 * abs(b)
    assert len(set(la)) == 3
