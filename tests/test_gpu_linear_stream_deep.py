"""Deep-K forward of the streaming Linear kernels (linear_stream.hip,
linear_stream_deep_kernel: 256-row tiles, K > 256), forced through
linear_fwd_stream(..., path=2) so that small M reaches it: bit for bit against
gemm.hip's route and against the 128-row streaming kernel, inside the float64
bound of test_gpu_linear_stream.py, rejected where it does not apply, and
routed by rows in one MnistMLPFused train step."""

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped off-GPU
    pytest.skip("needs MI355X", allow_module_level=True)

from sparktorch_amd import ops
from sparktorch_amd.ops.modules import MnistMLPFused

DEV = "cuda:0"
TILE128, DEEP = 1, 2  # linear_fwd_stream's path argument

# a single partial 256-row tile, a full one, one row past it, several tiles
# with a ragged last one
MS = (1, 255, 256, 257, 777)
NS = (192, 256)
# smallest K of the path (8 slabs + an 8-wide tail), exactly nine slabs, the
# flagship's 24 slabs + 16 (nearly five trips round the ring of five), a
# multiple of 32 past it
KS = (264, 288, 784, 800)
M_MAX = max(MS)
EPIS = [(False, False), (True, False), (True, True), (False, True)]  # (bias, relu)


def bf(x):
    return x.to(torch.bfloat16)


def bits(t):
    return t.view(torch.int16)


_CASES = {}


def case(N, K):
    """Operands and float64 references for (N, K) at the largest M, made
    once; smaller M are row prefixes.  Nothing here is modified by a test."""
    if (N, K) not in _CASES:
        g = torch.Generator(device=DEV).manual_seed(1000 * N + K)
        a = bf(torch.randn(M_MAX, K, device=DEV, generator=g)).contiguous()
        w = bf(torch.randn(N, K, device=DEV, generator=g) * 0.1).contiguous()
        bias = torch.randn(N, device=DEV, generator=g)
        _CASES[(N, K)] = dict(a=a, w=w, bias=bias, ref=a.double() @ w.double().t(),
                              S=a.double().abs() @ w.double().abs().t())
    return _CASES[(N, K)]


def within_bound(out, ref, S, K):
    """|out - ref| <= 2^-8 |ref| + K 2^-23 S + 1e-30 on every element: the
    bound of test_gpu_linear_stream.py (one bf16 rounding of the result plus
    the standard bound of an fp32 sum of K terms)."""
    err = (out.double() - ref).abs()
    lim = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * S + 1e-30
    return bool((err <= lim).all()), (err - lim).max().item()


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
def test_deep_forward_bits_and_float64_bound(N, K):
    ext = ops.ext()
    c = case(N, K)
    assert ext.linear_fwd_stream_deep_supported(N, K, M_MAX)
    for M in MS:
        a = c["a"][:M]
        for has_bias, relu in EPIS:
            b = c["bias"] if has_bias else None
            ref = c["ref"][:M] + (c["bias"].double() if has_bias else 0.0)
            if relu:
                ref = ref.clamp_min(0.0)
            new = ext.linear_fwd_stream(a, c["w"], b, relu, DEEP)
            cur = ext.linear_fwd_stream(a, c["w"], b, relu, TILE128)
            old = ext.linear_fwd(a, c["w"], b, relu, False)
            tag = "M=%d N=%d K=%d bias=%s relu=%s" % (M, N, K, has_bias, relu)
            assert new.shape == (M, N) and new.dtype == torch.bfloat16
            ok, over = within_bound(new, ref, c["S"][:M], K)
            assert ok, (tag, over)
            assert torch.equal(bits(new), bits(old)), tag
            assert torch.equal(bits(new), bits(cur)), tag


def test_deep_rejects():
    """K <= 256, N <= 128 and misaligned pointers raise and launch nothing."""
    ext = ops.ext()
    ok = ext.linear_fwd_stream_deep_supported
    assert ok(256, 784, 1) and ok(192, 264, 777) and ok(256, 800, 2097152)
    assert not ok(256, 256, 1000) and not ok(256, 64, 1000)
    assert not ok(128, 784, 1000) and not ok(64, 784, 1000)
    assert not ok(320, 784, 1000) and not ok(200, 784, 1000)
    assert not ok(256, 780, 1000) and not ok(256, 784, 0)
    for N, K in [(256, 256), (256, 64), (128, 784), (64, 784)]:
        x = bf(torch.randn(300, K, device=DEV)).contiguous()
        w = bf(torch.randn(N, K, device=DEV)).contiguous()
        with pytest.raises(RuntimeError):
            ext.linear_fwd_stream(x, w, None, False, DEEP)
    # 16-byte alignment: views that start 8 elements + 1 into a buffer
    K, N = 784, 256
    xbuf = bf(torch.randn(300 * K + 8, device=DEV))
    wbuf = bf(torch.randn(N * K + 8, device=DEV))
    x_ok, w_ok = xbuf[:300 * K].view(300, K), wbuf[:N * K].view(N, K)
    x_off, w_off = xbuf[1:300 * K + 1].view(300, K), wbuf[1:N * K + 1].view(N, K)
    assert ext.linear_fwd_stream(x_ok, w_ok, None, False, DEEP).shape == (300, N)
    with pytest.raises(RuntimeError):
        ext.linear_fwd_stream(x_off, w_ok, None, False, DEEP)
    with pytest.raises(RuntimeError):
        ext.linear_fwd_stream(x_ok, w_off, None, False, DEEP)
    with pytest.raises(RuntimeError):  # no such path
        ext.linear_fwd_stream(x_ok, w_ok, None, False, 3)


# ---------------------------------------------------------------------------
# routing
# ---------------------------------------------------------------------------

BATCH = 1000


@pytest.fixture
def stream_from_row_one():
    """Route every supported shape to the streaming kernels whatever its M."""
    ext = ops.ext()
    old = ext.set_linear_stream_min_rows(1)
    yield
    ext.set_linear_stream_min_rows(old)


def _trainer(model):
    from sparktorch_amd.parallel.sync import SyncTrainer

    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    return SyncTrainer(model, nn.CrossEntropyLoss(), opt, device=DEV, world_size=1)


def test_train_step_deep_route_matches_current(stream_from_row_one):
    """One SyncTrainer step of MnistMLPFused at batch 1000 with fc1's forward
    on the deep kernel and one with it on the 128-row kernel: the forwards are
    bit-identical, so the loss and the fc1 / fc2 gradients are too (fc1's
    wgrad, fc2's fused backward and the head take identical inputs; what is
    left is the order of their fp32 atomics, which the loss bound and the
    1e-6 on the head's gradients allow for)."""
    ext = ops.ext()
    torch.manual_seed(50)
    first = MnistMLPFused().to(DEV)
    second = MnistMLPFused().to(DEV)
    second.load_state_dict(first.state_dict())
    x = bf(torch.rand(BATCH, 784, device=DEV))
    t = torch.randint(0, 10, (BATCH,), device=DEV)
    assert BATCH < ext.linear_fwd_stream_deep_min_rows()
    t_deep, t_cur = _trainer(first), _trainer(second)
    old = ext.set_linear_stream_deep_min_rows(1)
    try:
        assert ext.linear_fwd_stream_deep_min_rows() == 1
        l_deep = t_deep.train_step(x, t)
    finally:
        ext.set_linear_stream_deep_min_rows(old)
    l_cur = t_cur.train_step(x, t)
    print("loss deep %.8f current %.8f" % (l_deep, l_cur))
    assert abs(l_deep - l_cur) <= 2e-6 * abs(l_cur), (l_deep, l_cur)
    grads = {k: (p.grad, q.grad) for (k, p), (_, q) in
             zip(t_deep.model.named_parameters(), t_cur.model.named_parameters())}
    assert all(g is not None for pair in grads.values() for g in pair)
    names = list(grads)
    fc12 = [k for k in names if k.startswith(("fc1", "fc2"))]
    assert len(fc12) == 4, names
    for k in fc12:
        p, q = grads[k]
        print(k, "max |diff|", (p.float() - q.float()).abs().max().item())
        assert torch.equal(p, q), k


def test_small_batch_keeps_todays_route():
    """Nothing overridden: below the stream threshold linear_fwd is gemm.hip's
    route, and the deep threshold lies at or above the stream threshold, so a
    small K > 256 forward never reaches the deep kernel by itself."""
    ext = ops.ext()
    thr, deep_thr = ext.linear_fwd_stream_min_rows(), ext.linear_fwd_stream_deep_min_rows()
    assert 257 < thr <= deep_thr
    c = case(256, 784)
    x = c["a"][:777]
    assert torch.equal(bits(ext.linear_fwd(x, c["w"], c["bias"], True)),
                       bits(ext.linear_fwd(x, c["w"], c["bias"], True, False)))
    # the automatic path of the forced binding is the 128-row kernel down here
    assert torch.equal(bits(ext.linear_fwd_stream(x, c["w"], c["bias"], True)),
                       bits(ext.linear_fwd_stream(x, c["w"], c["bias"], True, TILE128)))
