"""Wide-layer streaming Linear wgrad+db (linear_wgrad_wide.hip): the launcher
against a float64 reference and against the split-K gemm_kernel route on the
same bf16 inputs, its accumulate contract, bounds, the routing rule in
functional.linear_wgrad_into and one MLPAutoEncoderFused step on each route."""

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped off-GPU
    pytest.skip("needs MI355X", allow_module_level=True)

from sparktorch_amd import ops
from sparktorch_amd.ops import functional as Fn
from sparktorch_amd.ops.modules import MLPAutoEncoderFused

DEV = "cuda:0"
TOL = 0.02  # max|a - ref| / max|ref|


def err64(a, ref64):
    return ((a.double() - ref64).abs().max() / (ref64.abs().max() + 1e-300)).item()


def _case(B, No, Ki, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    dz = torch.randn(B, No, device=DEV, generator=g).to(torch.bfloat16).contiguous()
    x = torch.randn(B, Ki, device=DEV, generator=g).relu_().to(torch.bfloat16).contiguous()
    return dz, x


def _old_route(dz, x):
    dw = torch.zeros(dz.shape[1], x.shape[1], device=DEV)
    db = torch.zeros(dz.shape[1], device=DEV)
    sk = Fn._choose_splitk(dz.shape[0], dz.shape[1], x.shape[1])
    ops.ext().linear_wgrad_bias_into(dz, x, dw, db, sk)
    return dw, db


def _wide(dz, x, max_blocks=0, with_db=True):
    dw = torch.zeros(dz.shape[1], x.shape[1], device=DEV)
    db = torch.zeros(dz.shape[1], device=DEV) if with_db else None
    ops.ext().linear_wgrad_wide(dz, x, dw, db, max_blocks)
    return dw, db


def _check(dz, x, max_blocks=0, tag=""):
    """New kernel's error against float64 <= 4x the split-K route's on the same
    input (both multiply exactly and accumulate in fp32; 4x covers the other
    summation order) and under TOL, for dW and for db."""
    refs = (dz.double().t() @ x.double(), dz.double().sum(0))
    new, old = _wide(dz, x, max_blocks), _old_route(dz, x)
    e_new = [err64(a, r) for a, r in zip(new, refs)]
    e_old = [err64(a, r) for a, r in zip(old, refs)]
    print("%s B=%d No=%d Ki=%d mb=%d: dw new %.2e old %.2e | db new %.2e old %.2e"
          % (tag, dz.shape[0], dz.shape[1], x.shape[1], max_blocks, e_new[0], e_old[0],
             e_new[1], e_old[1]))
    assert all(torch.isfinite(a).all() for a in new)
    for n, o in zip(e_new, e_old):
        assert n <= 4 * o and n < TOL, (tag, e_new, e_old)


@pytest.mark.parametrize("Ki", [64, 128, 256])
@pytest.mark.parametrize("No", [264, 784, 1000])
def test_wide_matches_reference(No, Ki):
    assert ops.ext().linear_wgrad_wide_can_run(No, Ki, 1)
    for B in (1, 31, 33, 65, 1000, 4099):
        _check(*_case(B, No, Ki, 100 + B))


@pytest.mark.parametrize("max_blocks", [1, 2])
@pytest.mark.parametrize("No,Ki", [(784, 256), (264, 64)])
def test_wide_many_tiles_per_block(No, Ki, max_blocks):
    """Each block walks many tiles (both buffer sets in turn), the owner of the
    last one ends on a partial tile, and max_blocks = 1 at B = 4099 (128 full
    tiles in one walk) takes the half-way flush."""
    for B in (1000, 4099):
        _check(*_case(B, No, Ki, 200 + B), max_blocks=max_blocks)


@pytest.mark.parametrize("No,Ki,B", [(784, 256, 1000), (264, 64, 33), (1000, 128, 4099)])
def test_wide_accumulates(No, Ki, B):
    dz, x = _case(B, No, Ki, 300)
    m_dw = (dz.double().t() @ x.double()).abs().max()
    m_db = dz.double().sum(0).abs().max()
    dw, db = _wide(dz, x)
    dw1, db1 = dw.clone(), db.clone()
    ops.ext().linear_wgrad_wide(dz, x, dw, db, 0)
    # fp32 atomics: doubled to a few ulp of the largest partial sum
    assert (dw - 2 * dw1).abs().max() <= 1e-5 * m_dw + 1e-30
    assert (db - 2 * db1).abs().max() <= 1e-5 * m_db + 1e-30
    dwn, _ = _wide(dz, x, with_db=False)
    assert (dwn - dw1).abs().max() <= 1e-5 * m_dw + 1e-30


@pytest.mark.parametrize("No,Ki,B", [(784, 256, 33), (1000, 128, 127), (264, 64, 64)])
def test_wide_bounds(No, Ki, B):
    """Operands that end exactly where their allocation ends, and operands
    with NaN on both sides: a row- or column-tail over-read shows up as a
    non-finite or wrong result."""
    dz0, x0 = _case(B, No, Ki, 400)
    zb = torch.empty(24 + B * No, device=DEV, dtype=torch.bfloat16)
    xb = torch.empty(40 + B * Ki, device=DEV, dtype=torch.bfloat16)
    _check(zb[24:].view(B, No).copy_(dz0), xb[40:].view(B, Ki).copy_(x0), tag="end-of-alloc")
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


def _route(monkeypatch, dz, x, with_db=True, **flags):
    """Fn.linear_wgrad_into under the given module flags: its error against
    float64 (dW, db) and the bindings it called."""
    for k, v in flags.items():
        monkeypatch.setattr(Fn, k, v)
    spy = _Spy(ops.ext())
    monkeypatch.setattr(Fn.ops, "ext", lambda: spy)
    dw = torch.zeros(dz.shape[1], x.shape[1], device=DEV)
    db = torch.zeros(dz.shape[1], device=DEV) if with_db else None
    Fn.linear_wgrad_into(dz, x, dw, db)
    monkeypatch.undo()
    assert err64(dw, dz.double().t() @ x.double()) < TOL
    assert db is None or err64(db, dz.double().sum(0)) < TOL
    return spy.calls


def test_routing(monkeypatch):
    ext = ops.ext()
    No, Ki, B = 784, 256, 1 << 10
    while not ext.linear_wgrad_wide_supported(No, Ki, B):  # find the threshold
        B *= 2
        assert B <= 1 << 21
    dz, x = _case(B, No, Ki, 500)
    assert "linear_wgrad_wide" in _route(monkeypatch, dz, x)
    assert "linear_wgrad_wide" in _route(monkeypatch, dz, x, with_db=False)
    for flag in ("_WGRAD_WIDE", "_WGRAD_STREAM"):
        calls = _route(monkeypatch, dz, x, **{flag: False})
        assert "linear_wgrad_wide" not in calls and "linear_wgrad_bias_into" in calls
    calls = _route(monkeypatch, dz, x, with_db=False, _WGRAD_WIDE=False)
    assert "linear_wgrad_wide" not in calls and "linear_wgrad_into" in calls
    # below the measured threshold: split-K
    assert not ext.linear_wgrad_wide_supported(No, Ki, B // 2)
    calls = _route(monkeypatch, dz[:B // 2], x[:B // 2])
    assert "linear_wgrad_wide" not in calls and "linear_wgrad_bias_into" in calls
    # an operand aligned to 8 B only keeps the split-K route
    xb = torch.empty(4 + 300 * Ki, device=DEV, dtype=torch.bfloat16)
    x8 = xb[4:].view(300, Ki).copy_(x[:300])
    assert x8.data_ptr() % 16 == 8
    calls = _route(monkeypatch, dz[:300], x8, _WGRAD_WIDE_MIN_BATCH=1)
    assert "linear_wgrad_wide" not in calls and "linear_wgrad_bias_into" in calls
    assert "linear_wgrad_wide" in _route(monkeypatch, dz[:300], x[:300], _WGRAD_WIDE_MIN_BATCH=1)
    # the mirrored shape stays with linear_wgrad_stream
    calls = _route(monkeypatch, *_case(300, 256, 784, 510), _WGRAD_WIDE_MIN_BATCH=1,
                   _WGRAD_STREAM_MIN_BATCH=1)
    assert "linear_wgrad_stream" in calls and "linear_wgrad_wide" not in calls


@pytest.mark.parametrize("No,Ki", [(784, 100), (260, 64)])
def test_binding_rejects_unsupported(No, Ki):
    assert not ops.ext().linear_wgrad_wide_can_run(No, Ki, 40)
    dz, x = _case(40, No, Ki, 530)
    with pytest.raises(RuntimeError):
        ops.ext().linear_wgrad_wide(dz, x, torch.zeros(No, Ki, device=DEV), None, 0)


def _train_once(wide, compile_mode, state, x, monkeypatch):
    from sparktorch_amd.parallel.sync import SyncTrainer

    monkeypatch.setattr(Fn, "_WGRAD_WIDE", wide)
    monkeypatch.setattr(Fn, "_WGRAD_WIDE_MIN_BATCH", 1)
    spy = _Spy(ops.ext())
    monkeypatch.setattr(Fn.ops, "ext", lambda: spy)
    model = MLPAutoEncoderFused().to(DEV)
    model.load_state_dict(state)
    tr = SyncTrainer(model, nn.MSELoss(), torch.optim.SGD(model.parameters(), lr=1e-2),
                     device=DEV, world_size=1, compile_mode=compile_mode)
    loss = tr.train_step(x, x)
    torch.cuda.synchronize()
    grads = {k: p.grad.clone() for k, p in tr.model.named_parameters()}
    monkeypatch.undo()
    return loss, grads, spy.calls


@pytest.mark.parametrize("compile_mode", [None, "hipgraph"])
def test_train_step_on_both_routes(compile_mode, monkeypatch):
    """One MLPAutoEncoderFused (784-256-64-256-784) MSE step at B = 1000 with
    the output layer's dW+db on the wide kernel and on the split-K route;
    under hipgraph this is also the check that the launch is capturable."""
    torch.manual_seed(60)
    state = {k: v.clone() for k, v in MLPAutoEncoderFused().to(DEV).state_dict().items()}
    x = torch.randn(1000, 784, device=DEV).to(torch.bfloat16)
    l_new, g_new, c_new = _train_once(True, compile_mode, state, x, monkeypatch)
    l_old, g_old, c_old = _train_once(False, compile_mode, state, x, monkeypatch)
    assert "linear_wgrad_wide" in c_new and "linear_wgrad_wide" not in c_old
    print(compile_mode, "loss", l_new, l_old)
    assert abs(l_new - l_old) <= 2e-6 * abs(l_old)  # the forward is the same kernels
    for k in g_old:
        e = ((g_new[k] - g_old[k]).abs().max() / (g_old[k].abs().max() + 1e-30)).item()
        print(k, "%.2e" % e)
        assert torch.isfinite(g_new[k]).all() and e < TOL, (k, e)
