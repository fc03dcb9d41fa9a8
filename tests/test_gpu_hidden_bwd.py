"""One-pass hidden-layer backward (hidden_bwd.hip): dz_in bit for bit against
linear_dgrad_relu on both of its routes, dW / db against float64 under
test_gpu_linear_wgrad's rule, the accumulate contract, bounds, the routing in
functional.py and MnistMLPFused train steps with the fusion on and off."""

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
# edges of the 32-row tile, and at 1000 / 4099 (with max_blocks) enough tiles
# to turn the ring of three several times
BATCHES = (1, 31, 32, 33, 63, 65, 127, 1000, 4099)
# (No, Ki): the flagship, the narrower No, Ki of one column tile, Ki = 200
# (two 112-column tiles, the second partial) and Ki = 784 (seven of them)
SHAPES = [(256, 256), (128, 256), (256, 128), (128, 200), (256, 200), (128, 784), (256, 8)]


def bf(x):
    return x.to(torch.bfloat16)


def err64(a, ref64):
    return ((a.double() - ref64).abs().max() / (ref64.abs().max() + 1e-300)).item()


def _case(B, No, Ki, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    dz = bf(torch.randn(B, No, device=DEV, generator=g)).contiguous()
    x = bf(torch.randn(B, Ki, device=DEV, generator=g).relu_()).contiguous()
    w = bf(torch.randn(No, Ki, device=DEV, generator=g) / No ** 0.5).contiguous()
    return dz, x, w


def _refs(dz, x):
    return dz.double().t() @ x.double(), dz.double().sum(0)


def _old_wgrad(dz, x, with_db=True):
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


def _fused(dz, x, w, max_blocks=0, with_db=True, out=None):
    dw = torch.zeros(dz.shape[1], x.shape[1], device=DEV)
    db = torch.zeros(dz.shape[1], device=DEV) if with_db else None
    dzin = ops.ext().linear_hidden_bwd(dz, w, x, dw, db, max_blocks, out)
    return dzin, dw, db


def _check(dz, x, w, max_blocks=0, tag="", out=None):
    """dz_in equal to linear_dgrad_relu's on both routes; dW / db error against
    float64 <= 4x the split-K route's on the same input and under TOL (the
    rule and both numbers are test_gpu_linear_wgrad._check's)."""
    ext = ops.ext()
    dzin, dw, db = _fused(dz, x, w, max_blocks, out=out)
    assert torch.equal(dzin, ext.linear_dgrad_relu(dz, w, x, True)), tag
    assert torch.equal(dzin, ext.linear_dgrad_relu(dz, w, x, False)), tag
    ref_dw, ref_db = _refs(dz, x)
    old_dw, old_db = _old_wgrad(dz, x)
    e_new = (err64(dw, ref_dw), err64(db, ref_db))
    e_old = (err64(old_dw, ref_dw), err64(old_db, ref_db))
    print("%s B=%d No=%d Ki=%d mb=%d: dw new %.2e old %.2e | db new %.2e old %.2e"
          % (tag, dz.shape[0], dz.shape[1], x.shape[1], max_blocks, e_new[0], e_old[0],
             e_new[1], e_old[1]))
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()
    for n, o in zip(e_new, e_old):
        assert n <= 4 * o and n < TOL, (tag, e_new, e_old)
    return dzin, dw, db


@pytest.mark.parametrize("No,Ki", SHAPES)
def test_matches_references(No, Ki):
    assert ops.ext().linear_hidden_bwd_can_run(No, Ki, 1)
    for B in BATCHES:
        _check(*_case(B, No, Ki, 100 + B))


@pytest.mark.parametrize("max_blocks", [1, 2])
@pytest.mark.parametrize("No,Ki", [(256, 256), (128, 200), (256, 784)])
def test_many_tiles_per_block(No, Ki, max_blocks):
    """Each block walks many tiles (every image set of the ring in turn, the
    half-way flush at B = 4099 with one block) and the owner of the last one
    ends on a partial tile."""
    for B in (1000, 4099):
        _check(*_case(B, No, Ki, 200 + B), max_blocks=max_blocks)


@pytest.mark.parametrize("No,Ki,B", [(256, 256, 1000), (128, 200, 33), (256, 784, 4099)])
def test_accumulates(No, Ki, B):
    dz, x, w = _case(B, No, Ki, 300)
    ref_dw, ref_db = _refs(dz, x)
    _, dw, db = _fused(dz, x, w)
    dw1, db1 = dw.clone(), db.clone()
    ops.ext().linear_hidden_bwd(dz, w, x, dw, db, 0)
    # fp32 atomics: doubled to a few ulp of the largest partial sum
    assert (dw - 2 * dw1).abs().max() <= 1e-5 * ref_dw.abs().max() + 1e-30
    assert (db - 2 * db1).abs().max() <= 1e-5 * ref_db.abs().max() + 1e-30
    _, dwn, _ = _fused(dz, x, w, with_db=False)
    assert (dwn - dw1).abs().max() <= 1e-5 * ref_dw.abs().max() + 1e-30


@pytest.mark.parametrize("No,Ki,B", [(256, 256, 33), (128, 200, 127), (256, 8, 1000),
                                     (256, 256, 64), (128, 784, 65)])
def test_bounds(No, Ki, B):
    """Operands that end exactly where their allocation ends, operands with
    NaN on both sides, and dz_in inside a NaN-filled buffer whose guards (the
    rows at and past B among them) must stay untouched."""
    dz0, x0, w = _case(B, No, Ki, 400)
    zb = torch.empty(24 + B * No, device=DEV, dtype=torch.bfloat16)
    xb = torch.empty(40 + B * Ki, device=DEV, dtype=torch.bfloat16)
    wb = torch.empty(8 + No * Ki, device=DEV, dtype=torch.bfloat16)
    dz = zb[24:].view(B, No).copy_(dz0)
    x = xb[40:].view(B, Ki).copy_(x0)
    _check(dz, x, wb[8:].view(No, Ki).copy_(w), tag="end-of-alloc")
    guard = 4096
    big = torch.full((3 * guard + B * (No + Ki),), float("nan"), device=DEV,
                     dtype=torch.bfloat16)
    dz = big[guard:guard + B * No].view(B, No).copy_(dz0)
    x = big[2 * guard + B * No:2 * guard + B * (No + Ki)].view(B, Ki).copy_(x0)
    wg = torch.full((2 * guard + No * Ki,), float("nan"), device=DEV, dtype=torch.bfloat16)
    wv = wg[guard:guard + No * Ki].view(No, Ki).copy_(w)
    assert dz.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0
    for mb in (0, 1):
        # guard rows after the output: two tiles' worth, so a store of the
        # partial tile's rows past B would land in them
        rows = 64
        obuf = torch.full((guard + (B + rows) * Ki,), float("nan"), device=DEV,
                          dtype=torch.bfloat16)
        out = obuf[guard:guard + B * Ki].view(B, Ki)
        dzin, _, _ = _check(dz, x, wv, max_blocks=mb, tag="nan-guard", out=out)
        assert dzin.data_ptr() == out.data_ptr()
        assert torch.isnan(obuf[:guard]).all() and torch.isnan(obuf[guard + B * Ki:]).all()
        assert torch.isfinite(out).all()


def test_binding_rejects_unsupported():
    ext = ops.ext()
    for No, Ki in [(64, 64), (96, 64), (256, 100), (512, 256)]:
        assert not ext.linear_hidden_bwd_can_run(No, Ki, 40)
        dz, x, w = _case(40, No, Ki, 530)
        with pytest.raises(RuntimeError):
            ext.linear_hidden_bwd(dz, w, x, torch.zeros(No, Ki, device=DEV), None, 0)
    dz, x, w = _case(40, 128, 64, 531)
    xb = torch.empty(4 + 40 * 64, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):  # 8-byte aligned only
        ext.linear_hidden_bwd(dz, w, xb[4:].view(40, 64).copy_(x),
                              torch.zeros(128, 64, device=DEV), None, 0)


class _Spy:
    """ops.ext() stand-in that records which bindings were called."""

    def __init__(self, ext):
        self._ext, self.calls = ext, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self._ext, name)


def _route(monkeypatch, dz, x, w32, b32):
    """mlp_chain_ce_step's per-layer body for one masked hidden layer with
    direct gradients; returns (dz_in, dw, db, calls)."""
    spy = _Spy(ops.ext())
    monkeypatch.setattr(Fn.ops, "ext", lambda: spy)  # undone below: set nothing else here
    notes = []
    w = torch.nn.Parameter(w32.clone())
    b = torch.nn.Parameter(b32.clone())
    w.grad, b.grad = torch.zeros_like(w), torch.zeros_like(b)
    w._bucket_notify = lambda: notes.append("w")
    b._bucket_notify = lambda: notes.append("b")
    wb = ops.ext().cast_f32_bf16(w.detach())
    if Fn._hidden_bwd_ok(spy, dz, x, wb):
        dzin, _, _ = Fn._hidden_bwd(spy, dz, x, w, wb, b, True)
    else:
        dzin = spy.linear_dgrad_relu(dz, wb, x, Fn._LINEAR_STREAM)
        Fn._linear_param_grads(spy, dz, x, w, b, True, True)
    monkeypatch.setattr(Fn.ops, "ext", lambda: spy._ext)
    assert notes == ["w", "b"]
    return dzin, w.grad, b.grad, spy.calls


def _pair(dz, x, w32):
    """The two-launch route at a batch where split-K has one slice."""
    ext = ops.ext()
    wb = ext.cast_f32_bf16(w32)
    dw, db = _old_wgrad(dz, x)
    return ext.linear_dgrad_relu(dz, wb, x, True), dw, db


def test_routing(monkeypatch):
    B = 300  # split-K has one slice: the old route repeats bit for bit
    monkeypatch.setattr(Fn, "_WGRAD_STREAM_MIN_BATCH", 1)
    dz, x, w = _case(B, 256, 256, 500)
    w32, b32 = w.float(), torch.zeros(256, device=DEV)
    assert Fn._choose_splitk(B, 256, 256) == 1

    dzin, dw, db, calls = _route(monkeypatch, dz, x, w32, b32)
    assert "linear_hidden_bwd" in calls and "linear_dgrad_relu" not in calls
    assert "linear_wgrad_stream" not in calls
    want = _pair(dz, x, w32)
    assert torch.equal(dzin, want[0])
    ref_dw, ref_db = _refs(dz, x)
    assert err64(dw, ref_dw) < TOL and err64(db, ref_db) < TOL
    # one row group at this batch: every dW element gets a single atomicAdd
    # onto zero, so the streaming wgrad repeats bit for bit as well
    sdw, sdb = torch.zeros_like(want[1]), torch.zeros_like(want[2])
    ops.ext().linear_wgrad_stream(dz, x, sdw, sdb, 0)

    def old(calls):
        return "linear_hidden_bwd" not in calls and "linear_dgrad_relu" in calls

    # each switch off: the pair, bit for bit (dW / db: split-K, one slice)
    for name in ("_HIDDEN_BWD_FUSION", "_WGRAD_STREAM", "_LINEAR_STREAM"):
        monkeypatch.setattr(Fn, name, False)
        dzin, dw, db, calls = _route(monkeypatch, dz, x, w32, b32)
        monkeypatch.setattr(Fn, name, True)
        assert old(calls), name
        assert torch.equal(dzin, want[0]), name
        if name == "_WGRAD_STREAM":
            assert torch.equal(dw, want[1]) and torch.equal(db, want[2])
        else:
            assert "linear_wgrad_stream" in calls
            assert torch.equal(dw, sdw) and torch.equal(db, sdb)
    # below the batch threshold
    monkeypatch.setattr(Fn, "_WGRAD_STREAM_MIN_BATCH", None)
    assert not ops.ext().linear_hidden_bwd_supported(256, 256, B)
    dzin, dw, db, calls = _route(monkeypatch, dz, x, w32, b32)
    assert old(calls) and torch.equal(dzin, want[0])
    assert torch.equal(dw, want[1]) and torch.equal(db, want[2])
    monkeypatch.setattr(Fn, "_WGRAD_STREAM_MIN_BATCH", 1)
    # unsupported shape (No = 64)
    dz2, x2, w2 = _case(B, 64, 256, 501)
    dzin, dw, db, calls = _route(monkeypatch, dz2, x2, w2.float(), torch.zeros(64, device=DEV))
    assert old(calls) and "linear_wgrad_stream" in calls
    assert torch.equal(dzin, ops.ext().linear_dgrad_relu(dz2, w2, x2, True))
    # unaligned x_in
    xb = torch.empty(4 + B * 256, device=DEV, dtype=torch.bfloat16)
    xu = xb[4:].view(B, 256).copy_(x)
    assert xu.data_ptr() % 16 == 8
    dzin, dw, db, calls = _route(monkeypatch, dz, xu, w32, b32)
    assert old(calls) and "linear_wgrad_stream" not in calls
    assert torch.equal(dzin, want[0])
    assert torch.equal(dw, want[1]) and torch.equal(db, want[2])


def test_threshold_routes_big_batches():
    ext = ops.ext()
    B = 1 << 12
    while not ext.linear_hidden_bwd_supported(256, 256, B):
        B *= 2
        assert B <= 1 << 22
    assert ext.linear_wgrad_stream_supported(256, 256, B)
    assert not ext.linear_hidden_bwd_supported(64, 256, 1 << 22)


def _train_once(fused, compile_mode, criterion, state, x, t, monkeypatch):
    from sparktorch_amd.parallel.sync import SyncTrainer

    monkeypatch.setattr(Fn, "_HIDDEN_BWD_FUSION", fused)
    monkeypatch.setattr(Fn, "_WGRAD_STREAM_MIN_BATCH", 1)
    spy = _Spy(ops.ext())
    monkeypatch.setattr(Fn.ops, "ext", lambda: spy)
    model = MnistMLPFused().to(DEV)
    model.load_state_dict(state)
    tr = SyncTrainer(model, criterion, torch.optim.Adam(model.parameters(), lr=1e-3),
                     device=DEV, world_size=1, compile_mode=compile_mode)
    out = []
    for _ in range(2):
        n0 = len(spy.calls)
        loss = tr.train_step(x, t)
        torch.cuda.synchronize()
        grads = {k: p.grad.clone() for k, p in tr.model.named_parameters()}
        out.append((loss, grads, spy.calls[n0:]))
    monkeypatch.undo()
    return out


def _compare_steps(new, old, compile_mode):
    for step, ((l_new, g_new, c_new), (l_old, g_old, c_old)) in enumerate(zip(new, old)):
        if compile_mode is None:
            assert c_new.count("linear_hidden_bwd") == 1, c_new  # fc2
            assert c_new.count("linear_wgrad_stream") == 1  # fc1
        elif step == 0:
            # warm-up passes and the capture: once in each
            passes = c_new.count("linear_head_ce")
            assert passes >= 1 and c_new.count("linear_hidden_bwd") == passes, c_new
            assert c_new.count("linear_wgrad_stream") == passes
        else:
            assert "linear_hidden_bwd" not in c_new  # a replay calls no binding
        assert "linear_hidden_bwd" not in c_old
        print(compile_mode, "step", step, "loss", l_new, l_old)
        assert abs(l_new - l_old) <= 2e-6 * abs(l_old)
        for k in g_old:
            e = ((g_new[k] - g_old[k]).abs().max() / (g_old[k].abs().max() + 1e-30)).item()
            print(k, "%.2e" % e)
            assert torch.isfinite(g_new[k]).all() and e < TOL, (k, e)


@pytest.mark.parametrize("compile_mode", [None, "hipgraph"])
def test_train_step_fused_against_pair(compile_mode, monkeypatch):
    """Two MnistMLPFused (784-256-256-10) steps at B = 1000 under
    cross-entropy (mlp_chain_ce_step) with fc2's backward fused and not."""
    torch.manual_seed(60)
    state = {k: v.clone() for k, v in MnistMLPFused().to(DEV).state_dict().items()}
    x = bf(torch.randn(1000, 784, device=DEV))
    t = torch.randint(0, 10, (1000,), device=DEV)
    new = _train_once(True, compile_mode, nn.CrossEntropyLoss(), state, x, t, monkeypatch)
    old = _train_once(False, compile_mode, nn.CrossEntropyLoss(), state, x, t, monkeypatch)
    _compare_steps(new, old, compile_mode)


def test_autograd_path(monkeypatch):
    """The same under a criterion the explicit cross-entropy step does not
    serve, so the backward is _MLPChainFn's."""
    torch.manual_seed(61)
    state = {k: v.clone() for k, v in MnistMLPFused().to(DEV).state_dict().items()}
    x = bf(torch.randn(1000, 784, device=DEV))
    t = torch.nn.functional.one_hot(torch.randint(0, 10, (1000,), device=DEV), 10).float()
    new = _train_once(True, None, nn.MSELoss(), state, x, t, monkeypatch)
    old = _train_once(False, None, nn.MSELoss(), state, x, t, monkeypatch)
    assert "linear_head_ce" not in new[0][2]
    _compare_steps(new, old, None)


def test_autograd_returns_fresh_gradients(monkeypatch):
    """Plain leaf parameters (no bucket views): the fused call's dW / db are
    handed back to autograd and match the pair's."""
    monkeypatch.setattr(Fn, "_WGRAD_STREAM_MIN_BATCH", 1)
    g = torch.Generator(device=DEV).manual_seed(62)
    x = bf(torch.randn(300, 64, device=DEV, generator=g))
    shapes = [(256, 64), (256, 256), (10, 256)]

    def run(fused):
        monkeypatch.setattr(Fn, "_HIDDEN_BWD_FUSION", fused)
        gg = torch.Generator(device=DEV).manual_seed(63)
        ps = []
        for no, ki in shapes:
            ps.append((torch.randn(no, ki, device=DEV, generator=gg).div_(ki ** 0.5)
                       .requires_grad_(), torch.zeros(no, device=DEV).requires_grad_()))
        spy = _Spy(ops.ext())
        monkeypatch.setattr(Fn.ops, "ext", lambda: spy)
        y = Fn.hip_mlp_chain(x, [(ps[0][0], ps[0][1], True), (ps[1][0], ps[1][1], True),
                                 (ps[2][0], ps[2][1], False)])
        y.float().square().mean().backward()
        monkeypatch.setattr(Fn.ops, "ext", lambda: spy._ext)
        return [p.grad for pair in ps for p in pair], spy.calls

    g_new, c_new = run(True)
    g_old, c_old = run(False)
    assert c_new.count("linear_hidden_bwd") == 1 and "linear_hidden_bwd" not in c_old
    for a, b in zip(g_new, g_old):
        assert a is not None and torch.isfinite(a).all()
        assert ((a - b).abs().max() / (b.abs().max() + 1e-30)).item() < TOL
