"""Fused MLP backward: the ReLU mask folded into the dgrad epilogue
(linear_dgrad_relu), the one-pass classifier-head backward (linear_head_bwd)
and the chain autograd node that wires both into MnistMLPFused — each against
the unfused per-layer kernels / fp32 references on bf16-quantized inputs."""

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped off-GPU
    pytest.skip("needs MI355X", allow_module_level=True)

from sparktorch_amd import ops
from sparktorch_amd.ops import functional as Fn
from sparktorch_amd.ops.modules import HipLinear, MnistMLPFused

DEV = "cuda:0"
TOL = 0.02  # max|a - ref| / max|ref|


def bf(x):
    return x.to(torch.bfloat16)


def ref_of(x):
    """fp32 value of the bf16-quantized tensor (what the kernel actually sees)."""
    return bf(x).float()


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
    bits = y.view(torch.int16).view(-1)
    assert (bits == 0).any() and (bits == -32768).any()  # +0 and -0 present
    assert (y < 0).any() and (y > 0).any()
    return y


def is_pos_zero(t):
    return t.view(torch.int16) == 0


# ---------------------------------------------------------------------------
# linear_dgrad_relu
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("M,N_out,K_in", [(1, 16, 8), (127, 96, 200), (257, 256, 256),
                                          (130, 10, 64), (129, 64, 100)])
def test_dgrad_relu_bit_identical(M, N_out, K_in):
    ext = ops.ext()
    torch.manual_seed(10)
    dz = bf(torch.randn(M, N_out, device=DEV)).contiguous()
    w = bf(torch.randn(N_out, K_in, device=DEV) * 0.1).contiguous()
    y = relu_like((M, K_in), 11)
    want = ext.relu_bwd(ext.linear_dgrad(dz, w), y)
    got = ext.linear_dgrad_relu(dz, w, y)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert is_pos_zero(got)[~(y > 0)].all()
    # fp32 master weights take the same epilogue
    w32 = w.float().contiguous()
    assert torch.equal(ext.linear_dgrad_relu(dz, w32, y).view(torch.int16),
                       ext.relu_bwd(ext.linear_dgrad(dz, w32), y).view(torch.int16))


# ---------------------------------------------------------------------------
# linear_head_bwd
# ---------------------------------------------------------------------------

def _head_case(B, C, H, seed):
    torch.manual_seed(seed)
    dz = bf(torch.randn(B, C, device=DEV)).contiguous()
    w = bf(torch.randn(C, H, device=DEV) * 0.1).contiguous()
    y = relu_like((B, H), seed + 1)
    ref_dx = (dz.float() @ w.float()) * (y > 0)
    ref_dw = dz.float().t() @ y.float()
    ref_db = dz.float().sum(0)
    return dz, w, y, ref_dx, ref_dw, ref_db


def _check_head(B, C, H, max_blocks=0, seed=20):
    dz, w, y, ref_dx, ref_dw, ref_db = _head_case(B, C, H, seed)
    dw = torch.zeros(C, H, device=DEV)
    db = torch.zeros(C, device=DEV)
    dx = Fn.linear_head_bwd(dz, w, y, dw, db, max_blocks)
    tag = "B=%d C=%d H=%d mb=%d" % (B, C, H, max_blocks)
    e = (rel_err(dx, ref_dx), rel_err(dw, ref_dw), rel_err(db, ref_db))
    print(tag, "dx %.2e dw %.2e db %.2e" % e)
    assert dx.shape == (B, H) and dx.dtype == torch.bfloat16
    assert is_pos_zero(dx)[~(y > 0)].all(), tag
    assert max(e) < TOL, (tag, e)
    # accumulate semantics: a second call doubles dw / db (fp32 atomics, so to
    # rounding: a few ulp of the largest partial sum)
    dw1, db1 = dw.clone(), db.clone()
    dx2 = Fn.linear_head_bwd(dz, w, y, dw, db, max_blocks)
    assert torch.equal(dx2.view(torch.int16), dx.view(torch.int16)), tag
    assert (dw - 2 * dw1).abs().max() <= 1e-5 * ref_dw.abs().max() + 1e-30, tag
    assert (db - 2 * db1).abs().max() <= 1e-5 * ref_db.abs().max() + 1e-30, tag
    # db=None
    dwn = torch.zeros(C, H, device=DEV)
    dxn = Fn.linear_head_bwd(dz, w, y, dwn, None, max_blocks)
    assert torch.equal(dxn.view(torch.int16), dx.view(torch.int16)), tag
    assert rel_err(dwn, ref_dw) < TOL, tag


@pytest.mark.parametrize("H", [64, 256, 512])
@pytest.mark.parametrize("C", [1, 3, 10, 16])
def test_head_bwd_matches_unfused(C, H):
    assert ops.ext().head_bwd_supported(C, H)
    for B in (1, 127, 128, 129, 1000):
        _check_head(B, C, H)


@pytest.mark.parametrize("H", [64, 128, 256, 512])
def test_head_bwd_several_tiles_per_block(H):
    """max_blocks=2: each block walks many tiles and ends on a partial one."""
    _check_head(1000, 10, H, max_blocks=2)


@pytest.mark.parametrize("C,H", [(17, 64), (10, 96)])
def test_head_bwd_fallback_route(C, H):
    assert not ops.ext().head_bwd_supported(C, H)
    for B in (1, 129, 1000):
        _check_head(B, C, H)


def test_head_bwd_binding_rejects_unsupported():
    dz, w, y, *_ = _head_case(8, 17, 64, 30)
    with pytest.raises(RuntimeError):
        ops.ext().linear_head_bwd(dz, w, y, torch.zeros(17, 64, device=DEV), None)


# ---------------------------------------------------------------------------
# chain vs per-layer path
# ---------------------------------------------------------------------------

class _PerLayerMLP(nn.Module):
    """Three chained HipLinears — the path MnistMLPFused took before the chain."""

    def __init__(self, in_dim, hidden, classes):
        super().__init__()
        self.fc1 = HipLinear(in_dim, hidden, activation="relu")
        self.fc2 = HipLinear(hidden, hidden, activation="relu")
        self.fc3 = HipLinear(hidden, classes, activation=None)

    def forward(self, x):
        if x.is_cuda and x.dtype != torch.bfloat16:
            x = x.to(torch.bfloat16)
        return self.fc3(self.fc2(self.fc1(x)))


DIMS = (40, 64, 10)
BATCH = 300


def _pair():
    torch.manual_seed(40)
    chain = MnistMLPFused(*DIMS).to(DEV)
    layered = _PerLayerMLP(*DIMS).to(DEV)
    layered.load_state_dict(chain.state_dict())
    x = bf(torch.randn(BATCH, DIMS[0], device=DEV))
    t = torch.randint(0, DIMS[2], (BATCH,), device=DEV)
    return chain, layered, x, t


def _fwd_bwd(model, x, t):
    logits = model(x)
    loss = Fn.hip_cross_entropy(logits, t)
    loss.backward()
    return loss.item(), logits.detach()


def _same_loss(a, b):
    """The fused CE kernel sums its per-row terms with fp32 atomicAdd, so two
    runs on identical logits repeat only to rounding (bench.py's docstring
    gives 2e-6 for that)."""
    return abs(a - b) <= 2e-6 * abs(b)


@pytest.mark.parametrize("fused_head", [True, False])
def test_chain_matches_per_layer_autograd(fused_head, monkeypatch):
    monkeypatch.setattr(Fn, "_HEAD_FUSION", fused_head)
    chain, layered, x, t = _pair()
    assert list(chain.state_dict()) == list(layered.state_dict())
    (la, za), (lb, zb) = _fwd_bwd(chain, x, t), _fwd_bwd(layered, x, t)
    assert torch.equal(za, zb)  # the forward is the same kernels on the same bits
    assert _same_loss(la, lb), (la, lb)
    grads = {}
    for (k, p), (_, q) in zip(chain.named_parameters(), layered.named_parameters()):
        assert rel_err(p.grad, q.grad.float()) < TOL, k
        if not fused_head:
            assert torch.equal(p.grad, q.grad), k
        grads[k] = p.grad.clone()
    # plain autograd accumulation: a second backward doubles .grad
    _fwd_bwd(chain, x, t)
    for k, p in chain.named_parameters():
        assert (p.grad - 2 * grads[k]).abs().max() <= 1e-5 * grads[k].abs().max(), k


def test_chain_input_gradient():
    chain, layered, x, t = _pair()
    xa = x.clone().requires_grad_(True)
    xb = x.clone().requires_grad_(True)
    _fwd_bwd(chain, xa, t)
    _fwd_bwd(layered, xb, t)
    assert rel_err(xa.grad, xb.grad.float()) < TOL


def _trainer(model, compile_mode=None):
    from sparktorch_amd.parallel.sync import SyncTrainer

    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    return SyncTrainer(model, nn.CrossEntropyLoss(), opt, device=DEV, world_size=1,
                       compile_mode=compile_mode)


def test_chain_sync_trainer_direct_grads():
    """Direct-grad / bucket path: one SyncTrainer step on each model."""
    chain, layered, x, t = _pair()
    ta, tb = _trainer(chain), _trainer(layered)
    la, lb = ta.train_step(x, t), tb.train_step(x, t)
    assert _same_loss(la, lb), (la, lb)
    for (k, p), (_, q) in zip(ta.model.named_parameters(), tb.model.named_parameters()):
        assert p.grad is not None and rel_err(p.grad, q.grad.float()) < TOL, k


def test_chain_sync_trainer_hipgraph_vs_eager():
    """Three graphed steps track three eager steps.  The two runs differ only
    by the order of the head kernel's fp32 atomics (~1e-7 relative on dW3/db3);
    Adam can turn that into a bf16 rounding flip of a few logits, each worth at
    most 2^-8 relative on one of 3000 logits — far below 1e-3 of the loss."""
    chain, _, x, t = _pair()
    twin = MnistMLPFused(*DIMS).to(DEV)
    twin.load_state_dict(chain.state_dict())
    te, tg = _trainer(chain), _trainer(twin, compile_mode="hipgraph")
    le = [te.train_step(x, t) for _ in range(3)]
    lg = [tg.train_step(x, t) for _ in range(3)]
    print("eager", le, "graph", lg)
    assert le[-1] < le[0]
    for a, b in zip(le, lg):
        assert abs(a - b) <= 1e-3 * abs(a)
