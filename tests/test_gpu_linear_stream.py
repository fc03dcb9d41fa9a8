"""Full-N streaming Linear forward / dgrad (linear_stream.hip): forced through
the *_stream bindings at every partial-tile edge, against float64 with a
derived elementwise bound, bit for bit against gemm.hip's route, and wired
into one MnistMLPFused train step."""

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
TOL = 0.02  # max|a - ref| / max|ref|, as in test_gpu_mlp_fusion.py

# every partial-tile edge of a 128-row tile (and of a 256-row one)
MS = (1, 127, 128, 129, 255, 256, 257, 1000, 4099)
NS = (192, 256)
# one partial slab, whole slabs, whole slabs plus a tail (slab depth 32 or 64)
KS = (8, 24, 64, 200, 256, 784)
M_MAX = max(MS)


def bf(x):
    return x.to(torch.bfloat16)


def bits(t):
    return t.view(torch.int16)


def rel_err(a, ref):
    return ((a.float() - ref).abs().max() / (ref.abs().max() + 1e-12)).item()


def relu_like(shape, seed):
    """bf16 'saved ReLU output' with +0, -0, negative and positive entries."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    y = torch.randn(shape, device=DEV, generator=g)
    flat = y.view(-1)
    flat[0::5] = 0.0
    flat[1::5] = -0.0
    flat[2::7] = -1.5
    y = bf(y).contiguous()
    b = bits(y).view(-1)
    assert (b == 0).any() and (b == -32768).any()
    assert (y < 0).any() and (y > 0).any()
    return y


_CASES = {}


def case(N, K):
    """Operands for (N, K) at the largest M, made once; smaller M are row
    prefixes.  Nothing here is modified by a test."""
    if (N, K) not in _CASES:
        g = torch.Generator(device=DEV).manual_seed(1000 * N + K)
        a = bf(torch.randn(M_MAX, K, device=DEV, generator=g)).contiguous()
        w_fwd = bf(torch.randn(N, K, device=DEV, generator=g) * 0.1).contiguous()  # W[N][K]
        w_bwd = bf(torch.randn(K, N, device=DEV, generator=g) * 0.1).contiguous()  # W[N_out=K][K_in=N]
        bias = torch.randn(N, device=DEV, generator=g)
        ad, aa = a.double(), a.double().abs()
        _CASES[(N, K)] = dict(
            a=a, w_fwd=w_fwd, w_bwd=w_bwd, bias=bias,
            ref_fwd=ad @ w_fwd.double().t(), s_fwd=aa @ w_fwd.double().abs().t(),
            ref_bwd=ad @ w_bwd.double(), s_bwd=aa @ w_bwd.double().abs(),
            mask=relu_like((M_MAX, N), 7 * N + K))
    return _CASES[(N, K)]


def within_bound(out, ref, S, K):
    """|out - ref| <= 2^-8 |ref| + K 2^-23 S + 1e-30 on every element: one bf16
    rounding of the result plus the standard bound of an fp32 sum of K terms."""
    err = (out.double() - ref).abs()
    lim = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * S + 1e-30
    return bool((err <= lim).all()), (err - lim).max().item()


EPIS = [(False, False), (True, False), (True, True), (False, True)]  # (bias, relu)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
def test_forward_float64_bound_and_bits(N, K):
    ext = ops.ext()
    c = case(N, K)
    assert ext.linear_fwd_stream_supported(N, K, M_MAX)
    for M in MS:
        a = c["a"][:M]
        for has_bias, relu in EPIS:
            b = c["bias"] if has_bias else None
            ref = c["ref_fwd"][:M] + (c["bias"].double() if has_bias else 0.0)
            if relu:
                ref = ref.clamp_min(0.0)
            new = ext.linear_fwd_stream(a, c["w_fwd"], b, relu)
            old = ext.linear_fwd(a, c["w_fwd"], b, relu, False)
            tag = "M=%d N=%d K=%d bias=%s relu=%s" % (M, N, K, has_bias, relu)
            assert new.shape == (M, N) and new.dtype == torch.bfloat16
            ok_new, over_new = within_bound(new, ref, c["s_fwd"][:M], K)
            ok_old, over_old = within_bound(old, ref, c["s_fwd"][:M], K)
            assert ok_old, ("the bound is wrong, not the kernel", tag, over_old)
            assert ok_new, (tag, over_new)
            assert torch.equal(bits(new), bits(old)), tag


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
def test_dgrad_float64_bound_bits_and_mask(N, K):
    """dX[M, N] = dZ[M, K] W[K, N]: K is the layer's N_out, N its K_in."""
    ext = ops.ext()
    c = case(N, K)
    w = c["w_bwd"]
    for M in MS:
        dz, y = c["a"][:M], c["mask"][:M]
        ref, S = c["ref_bwd"][:M], c["s_bwd"][:M]
        tag = "M=%d N=%d K=%d" % (M, N, K)
        new = ext.linear_dgrad_stream(dz, w, None)
        old = ext.linear_dgrad(dz, w, False)
        assert new.shape == (M, N) and new.dtype == torch.bfloat16
        ok_old, over_old = within_bound(old, ref, S, K)
        assert ok_old, ("the bound is wrong, not the kernel", tag, over_old)
        ok_new, over_new = within_bound(new, ref, S, K)
        assert ok_new, (tag, over_new)
        assert torch.equal(bits(new), bits(old)), tag
        # mask: bit +0 exactly where (y > 0) is false, untouched elsewhere
        newm = ext.linear_dgrad_stream(dz, w, y)
        oldm = ext.linear_dgrad_relu(dz, w, y, False)
        keep = y > 0
        assert (bits(newm)[~keep] == 0).all(), tag
        assert torch.equal(bits(newm)[keep], bits(new)[keep]), tag
        assert torch.equal(bits(newm), bits(oldm)), tag
        okm, overm = within_bound(newm, ref * keep, S, K)
        assert okm, (tag, overm)


def test_supported_gate():
    ext = ops.ext()
    ok = ext.linear_fwd_stream_supported
    assert ok(256, 784, 1) and ok(192, 8, 4099) and ok(256, 256, 2097152)
    for N in (64, 128, 320, 512):      # at or under one old tile; over the block
        assert not ok(N, 256, 1000)
    for N in (136, 200, 250):          # not a multiple of 64
        assert not ok(N, 256, 1000)
    for K in (0, 4, 12, 783):          # rows must be 16 B
        assert not ok(256, K, 1000)
    assert not ok(256, 256, 0)


@pytest.mark.parametrize("N,K", [(64, 64), (200, 64), (256, 12), (320, 64)])
def test_forced_bindings_reject_unsupported(N, K):
    ext = ops.ext()
    x = bf(torch.randn(10, K, device=DEV)).contiguous()
    w = bf(torch.randn(N, K, device=DEV)).contiguous()
    with pytest.raises(RuntimeError):
        ext.linear_fwd_stream(x, w, None, False)
    dz = bf(torch.randn(10, K, device=DEV)).contiguous()
    wt = bf(torch.randn(K, N, device=DEV)).contiguous()
    with pytest.raises(RuntimeError):
        ext.linear_dgrad_stream(dz, wt, None)
    with pytest.raises(RuntimeError):  # fp32 master weights stay on gemm.hip
        ext.linear_fwd_stream(bf(torch.randn(10, 64, device=DEV)).contiguous(),
                              torch.randn(256, 64, device=DEV), None, False)


def test_public_bindings_route_by_rows():
    """Below the threshold the public bindings give what gemm.hip gives (it IS
    that route); from it on they give what the forced bindings give.  fp32
    master weights and allow_stream=False stay on gemm.hip at any M."""
    ext = ops.ext()
    thr = ext.linear_fwd_stream_min_rows()
    assert thr > 257
    N, K = 256, 64
    g = torch.Generator(device=DEV).manual_seed(5)
    x = bf(torch.randn(thr, K, device=DEV, generator=g)).contiguous()
    w = bf(torch.randn(N, K, device=DEV, generator=g) * 0.1).contiguous()
    wt = bf(torch.randn(K, N, device=DEV, generator=g) * 0.1).contiguous()
    b = torch.randn(N, device=DEV, generator=g)
    y = relu_like((thr, N), 6)
    for M in (257, thr - 1, thr):
        xs, ys = x[:M], y[:M]
        assert torch.equal(bits(ext.linear_fwd(xs, w, b, True)),
                           bits(ext.linear_fwd(xs, w, b, True, False)))
        assert torch.equal(bits(ext.linear_dgrad(xs, wt)), bits(ext.linear_dgrad(xs, wt, False)))
        assert torch.equal(bits(ext.linear_dgrad_relu(xs, wt, ys)),
                           bits(ext.linear_dgrad_relu(xs, wt, ys, False)))
    assert torch.equal(bits(ext.linear_fwd(x, w, b, True)), bits(ext.linear_fwd_stream(x, w, b, True)))
    assert torch.equal(bits(ext.linear_dgrad_relu(x, wt, y)), bits(ext.linear_dgrad_stream(x, wt, y)))
    w32 = w.float().contiguous()
    assert torch.equal(bits(ext.linear_fwd(x, w32, b, True)), bits(ext.linear_fwd(x, w, b, True)))


# ---------------------------------------------------------------------------
# one train step of the flagship model shape through the new route
# ---------------------------------------------------------------------------

DIMS = (784, 256, 10)
BATCH = 4099


@pytest.fixture
def stream_from_row_one():
    """Route every supported shape to the streaming kernel whatever its M."""
    ext = ops.ext()
    old = ext.set_linear_stream_min_rows(1)
    yield
    ext.set_linear_stream_min_rows(old)


def _trainer(model, compile_mode=None):
    from sparktorch_amd.parallel.sync import SyncTrainer

    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    return SyncTrainer(model, nn.CrossEntropyLoss(), opt, device=DEV, world_size=1,
                       compile_mode=compile_mode)


def _models(n):
    torch.manual_seed(50)
    first = MnistMLPFused(*DIMS).to(DEV)
    out = [first]
    for _ in range(n - 1):
        m = MnistMLPFused(*DIMS).to(DEV)
        m.load_state_dict(first.state_dict())
        out.append(m)
    x = bf(torch.rand(BATCH, DIMS[0], device=DEV))
    t = torch.randint(0, DIMS[2], (BATCH,), device=DEV)
    return out, x, t


def test_train_step_matches_old_route(stream_from_row_one, monkeypatch):
    (new, old), x, t = _models(2)
    tn, to = _trainer(new), _trainer(old)
    ln = tn.train_step(x, t)
    monkeypatch.setattr(Fn, "_LINEAR_STREAM", False)
    lo = to.train_step(x, t)
    print("loss new %.8f old %.8f" % (ln, lo))
    assert abs(ln - lo) <= 2e-6 * abs(lo), (ln, lo)
    for (k, p), (_, q) in zip(tn.model.named_parameters(), to.model.named_parameters()):
        assert p.grad is not None and rel_err(p.grad, q.grad.float()) < TOL, k


def test_train_step_hipgraph_vs_eager(stream_from_row_one):
    """Three graphed steps through the streaming kernels track three eager ones
    (test_gpu_mlp_fusion.py, test_chain_sync_trainer_hipgraph_vs_eager, says
    why 1e-3 of the loss)."""
    (eager, graphed), x, t = _models(2)
    te, tg = _trainer(eager), _trainer(graphed, compile_mode="hipgraph")
    le = [te.train_step(x, t) for _ in range(3)]
    lg = [tg.train_step(x, t) for _ in range(3)]
    print("eager", le, "graph", lg)
    assert le[-1] < le[0]
    for a, b in zip(le, lg):
        assert abs(a - b) <= 1e-3 * abs(a)
