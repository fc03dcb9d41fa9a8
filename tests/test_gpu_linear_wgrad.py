"""Batch-streaming Linear wgrad+db (linear_wgrad.hip): the launcher against a
float64 reference and against the split-K gemm_kernel route on the same
bf16-quantized inputs, its accumulate contract, bounds, the routing rule in
functional.linear_wgrad_into and one MnistMLPFused train step on each route."""

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
TOL = 0.02  # max|a - ref| / max|ref|
BATCHES = (1, 31, 32, 33, 63, 65, 127, 1000, 4099)


def bf(x):
    return x.to(torch.bfloat16)


def err64(a, ref64):
    return ((a.double() - ref64).abs().max() / (ref64.abs().max() + 1e-300)).item()


def _case(B, No, Ki, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    dz = bf(torch.randn(B, No, device=DEV, generator=g)).contiguous()
    x = bf(torch.randn(B, Ki, device=DEV, generator=g).relu_()).contiguous()
    return dz, x


def _refs(dz, x):
    return dz.double().t() @ x.double(), dz.double().sum(0)


def _old_route(dz, x, with_db=True):
    ext = ops.ext()
    No, Ki = dz.shape[1], x.shape[1]
    sk = Fn._choose_splitk(dz.shape[0], No, Ki)
    dw = torch.zeros(No, Ki, device=DEV)
    db = torch.zeros(No, device=DEV)
    if with_db:
        ext.linear_wgrad_bias_into(dz, x, dw, db, sk)
    else:
        ext.linear_wgrad_into(dz, x, dw, sk)
    return dw, db


def _stream(dz, x, max_blocks=0, with_db=True):
    dw = torch.zeros(dz.shape[1], x.shape[1], device=DEV)
    db = torch.zeros(dz.shape[1], device=DEV) if with_db else None
    ops.ext().linear_wgrad_stream(dz, x, dw, db, max_blocks)
    return dw, db


def _check(dz, x, max_blocks=0, tag=""):
    """New kernel's error against float64 <= 4x the split-K route's on the same
    input (both multiply exactly and accumulate in fp32; 4x covers the other
    summation order) and under TOL."""
    ref_dw, ref_db = _refs(dz, x)
    old_dw, old_db = _old_route(dz, x)
    dw, db = _stream(dz, x, max_blocks)
    e_new = (err64(dw, ref_dw), err64(db, ref_db))
    e_old = (err64(old_dw, ref_dw), err64(old_db, ref_db))
    print("%s B=%d No=%d Ki=%d mb=%d: dw new %.2e old %.2e | db new %.2e old %.2e"
          % (tag, dz.shape[0], dz.shape[1], x.shape[1], max_blocks, e_new[0], e_old[0],
             e_new[1], e_old[1]))
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()
    for n, o in zip(e_new, e_old):
        assert n <= 4 * o and n < TOL, (tag, e_new, e_old)
    return dw, db, ref_dw, ref_db


@pytest.mark.parametrize("Ki", [8, 16, 64, 200, 256, 784])
@pytest.mark.parametrize("No", [64, 128, 256])
def test_stream_matches_reference(No, Ki):
    assert ops.ext().linear_wgrad_stream_can_run(No, Ki, 1)
    for B in BATCHES:
        dz, x = _case(B, No, Ki, 100 + B)
        _check(dz, x)


@pytest.mark.parametrize("max_blocks", [1, 2])
@pytest.mark.parametrize("No,Ki", [(256, 784), (128, 256), (64, 200)])
def test_stream_many_tiles_per_block(No, Ki, max_blocks):
    """Each block walks many tiles (both LDS buffer pairs in turn) and the
    owner of the last one ends on a partial tile.

    max_blocks = 1 at B = 4099 is the longest single walk here (128 full
    tiles): it takes the kernel's half-way flush, without which one fp32
    chain over all 4099 rows measured 4.6x - 6.1x the split-K route's error
    (that route cuts them into 8 slices); with it 2.2x - 2.5x."""
    for B in (1000, 4099):
        dz, x = _case(B, No, Ki, 200 + B)
        _check(dz, x, max_blocks)


@pytest.mark.parametrize("No,Ki,B", [(256, 784, 1000), (64, 16, 33), (128, 200, 4099)])
def test_stream_accumulates(No, Ki, B):
    dz, x = _case(B, No, Ki, 300)
    ref_dw, ref_db = _refs(dz, x)
    dw, db = _stream(dz, x)
    dw1, db1 = dw.clone(), db.clone()
    ops.ext().linear_wgrad_stream(dz, x, dw, db, 0)
    # fp32 atomics: doubled to a few ulp of the largest partial sum
    assert (dw - 2 * dw1).abs().max() <= 1e-5 * ref_dw.abs().max() + 1e-30
    assert (db - 2 * db1).abs().max() <= 1e-5 * ref_db.abs().max() + 1e-30
    dwn, _ = _stream(dz, x, with_db=False)
    assert (dwn - dw1).abs().max() <= 1e-5 * ref_dw.abs().max() + 1e-30


@pytest.mark.parametrize("No,Ki,B", [(256, 784, 33), (64, 200, 127), (128, 8, 1000),
                                     (256, 256, 64)])
def test_stream_bounds(No, Ki, B):
    """Operands that end exactly where their allocation ends, and operands
    with NaN on both sides: a row- or column-tail over-read shows up as a
    non-finite or wrong result."""
    dz0, x0 = _case(B, No, Ki, 400)
    # views ending at the end of their allocations (16-byte aligned start)
    zb = torch.empty(24 + B * No, device=DEV, dtype=torch.bfloat16)
    xb = torch.empty(40 + B * Ki, device=DEV, dtype=torch.bfloat16)
    dz = zb[24:].view(B, No).copy_(dz0)
    x = xb[40:].view(B, Ki).copy_(x0)
    _check(dz, x, tag="end-of-alloc")
    # NaN guards before and after both operands in one larger tensor
    guard = 4096
    big = torch.full((3 * guard + B * (No + Ki),), float("nan"), device=DEV,
                     dtype=torch.bfloat16)
    dz = big[guard:guard + B * No].view(B, No).copy_(dz0)
    x = big[2 * guard + B * No:2 * guard + B * (No + Ki)].view(B, Ki).copy_(x0)
    assert dz.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0
    _check(dz, x, tag="nan-guard")
    _check(dz, x, max_blocks=1, tag="nan-guard")


class _Spy:
    """ops.ext() stand-in that records which bindings were called."""

    def __init__(self, ext):
        self._ext, self.calls = ext, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self._ext, name)


def _route(monkeypatch, dz, x, with_db=True):
    spy = _Spy(ops.ext())
    monkeypatch.setattr(Fn.ops, "ext", lambda: spy)
    dw = torch.zeros(dz.shape[1], x.shape[1], device=DEV)
    db = torch.zeros(dz.shape[1], device=DEV) if with_db else None
    Fn.linear_wgrad_into(dz, x, dw, db)
    monkeypatch.undo()
    return dw, db, spy.calls


# B = 300 keeps split-K at one slice, so the old route repeats bit for bit
@pytest.mark.parametrize("No,Ki,B", [(10, 64, 300), (96, 64, 300), (64, 100, 300),
                                     (256, 784, 300)])
@pytest.mark.parametrize("with_db", [True, False])
def test_rejected_shapes_keep_old_route(No, Ki, B, with_db, monkeypatch):
    assert not ops.ext().linear_wgrad_stream_supported(No, Ki, B)
    assert Fn._choose_splitk(B, No, Ki) == 1
    dz, x = _case(B, No, Ki, 500)
    dw, db, calls = _route(monkeypatch, dz, x, with_db)
    assert "linear_wgrad_stream" not in calls
    want_dw, want_db = _old_route(dz, x, with_db)
    assert torch.equal(dw, want_dw)
    if with_db:
        assert torch.equal(db, want_db)


def test_unaligned_operands_keep_old_route(monkeypatch):
    B, No, Ki = 300, 64, 64
    monkeypatch.setattr(Fn, "_WGRAD_STREAM_MIN_BATCH", 1)
    dz0, x0 = _case(B, No, Ki, 510)
    xb = torch.empty(4 + B * Ki, device=DEV, dtype=torch.bfloat16)
    x = xb[4:].view(B, Ki).copy_(x0)  # 8-byte aligned only
    assert x.data_ptr() % 16 == 8
    dw, db, calls = _route(monkeypatch, dz0, x)
    assert "linear_wgrad_stream" not in calls
    want_dw, want_db = _old_route(dz0, x)
    assert torch.equal(dw, want_dw) and torch.equal(db, want_db)


def test_switch_and_threshold(monkeypatch):
    ext = ops.ext()
    No, Ki = 64, 64
    B = 1 << 13
    while not ext.linear_wgrad_stream_supported(No, Ki, B):  # find the threshold
        B *= 2
        assert B <= 1 << 22
    assert not ext.linear_wgrad_stream_supported(No, Ki, 300)
    dz, x = _case(B, No, Ki, 520)
    ref_dw, ref_db = _refs(dz, x)
    dw, db, calls = _route(monkeypatch, dz, x)
    assert "linear_wgrad_stream" in calls
    assert err64(dw, ref_dw) < TOL and err64(db, ref_db) < TOL
    monkeypatch.setattr(Fn, "_WGRAD_STREAM", False)
    dw, db, calls = _route(monkeypatch, dz, x)
    assert "linear_wgrad_stream" not in calls and "linear_wgrad_bias_into" in calls
    assert err64(dw, ref_dw) < TOL and err64(db, ref_db) < TOL


def test_binding_rejects_unsupported():
    dz, x = _case(40, 96, 64, 530)
    with pytest.raises(RuntimeError):
        ops.ext().linear_wgrad_stream(dz, x, torch.zeros(96, 64, device=DEV), None, 0)
    dz, x = _case(40, 64, 100, 531)
    with pytest.raises(RuntimeError):
        ops.ext().linear_wgrad_stream(dz, x, torch.zeros(64, 100, device=DEV), None, 0)


def _train_once(stream, compile_mode, state, x, t, monkeypatch):
    from sparktorch_amd.parallel.sync import SyncTrainer

    monkeypatch.setattr(Fn, "_WGRAD_STREAM", stream)
    monkeypatch.setattr(Fn, "_WGRAD_STREAM_MIN_BATCH", 1)
    spy = _Spy(ops.ext())
    monkeypatch.setattr(Fn.ops, "ext", lambda: spy)
    model = MnistMLPFused().to(DEV)
    model.load_state_dict(state)
    tr = SyncTrainer(model, nn.CrossEntropyLoss(), torch.optim.Adam(model.parameters(), lr=1e-3),
                     device=DEV, world_size=1, compile_mode=compile_mode)
    loss = tr.train_step(x, t)
    torch.cuda.synchronize()
    grads = {k: p.grad.clone() for k, p in tr.model.named_parameters()}
    monkeypatch.undo()
    return loss, grads, spy.calls


@pytest.mark.parametrize("compile_mode", [None, "hipgraph"])
def test_train_step_on_both_routes(compile_mode, monkeypatch):
    """One MnistMLPFused (784-256-256-10) step at B = 1000 with fc1 / fc2's
    dW+db on the streaming kernel and on the split-K route."""
    torch.manual_seed(60)
    state = {k: v.clone() for k, v in MnistMLPFused().to(DEV).state_dict().items()}
    x = bf(torch.randn(1000, 784, device=DEV))
    t = torch.randint(0, 10, (1000,), device=DEV)
    l_new, g_new, c_new = _train_once(True, compile_mode, state, x, t, monkeypatch)
    l_old, g_old, c_old = _train_once(False, compile_mode, state, x, t, monkeypatch)
    assert "linear_wgrad_stream" in c_new and "linear_wgrad_stream" not in c_old
    print(compile_mode, "loss", l_new, l_old)
    # the forward is the same kernels; CE sums its rows with fp32 atomics
    assert abs(l_new - l_old) <= 2e-6 * abs(l_old)
    for k in g_old:
        e = ((g_new[k] - g_old[k]).abs().max() / (g_old[k].abs().max() + 1e-30)).item()
        print(k, "%.2e" % e)
        assert torch.isfinite(g_new[k]).all() and e < TOL, (k, e)
