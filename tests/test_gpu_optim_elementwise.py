"""The optimizer, bias-gradient and cast kernels of elementwise.hip against
float64 references.

* fused_adam against an fp64 recurrence written here; the bias corrections
  come either from the host (step_dev=None) or from the device step counter
  (what FusedAdam.step always uses on a GPU), where the host values passed
  along are deliberately wrong to prove the kernel ignores them.
* fused_sgd against torch.optim.SGD run in fp64.
* Cap for p, m, v and the momentum buffer: 1e-5 absolute at lr 0.01 (Adam) /
  0.05 (SGD), the project's existing cap; __powf's error in 1 - 0.999^t moves
  an Adam step by about lr * 1e-4 = 1e-6.
* bias_grad against the fp64 column sum, cap 1e-5 * sum|dz| per column (the
  fp32 chain bound with a wide margin).
* the casts bit-equal to torch's conversions on crafted patterns, NaN staying
  NaN with any payload.

Sizes n in {1, 3, 4, 5, 1027, 2 097 159}: below, at and above the 4-wide
vector body, and one past the 2048 x 256 x 4 grid cap so that the stride loop
iterates and a tail remains.  The big size repeats a 1027-long pattern, so
its reference is the pattern's (no tensor here exceeds 16 MB).
"""

import math

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped off-GPU
    pytest.skip("needs MI355X", allow_module_level=True)

from sparktorch_amd import ops
from sparktorch_amd.models.simple_net import Net
from sparktorch_amd.ops.optim import FusedAdam, FusedSGD, fused_optimizer_for
from sparktorch_amd.parallel.buckets import FlatBuckets

DEV = "cuda:0"
SIZES = [1, 3, 4, 5, 1027, 2_097_159]
PATTERN = 1027
CAP = 1e-5


def bf(x):
    return x.to(torch.bfloat16)


def tiled(pattern, n):
    """fp32 device tensor of n elements repeating the (<= 1027-long) pattern."""
    reps = -(-n // pattern.numel())
    return pattern.float().repeat(reps)[:n].contiguous().to(DEV)


def worst_err(got, ref_pattern):
    """max |got[i] - ref_pattern[i % L]| in fp64, in chunks of 2^19."""
    L = ref_pattern.numel()
    ref_pattern = ref_pattern.to(got.device)
    worst = 0.0
    for s in range(0, got.numel(), 1 << 19):
        e = min(got.numel(), s + (1 << 19))
        idx = torch.arange(s, e, device=got.device) % L
        worst = max(worst, (got[s:e].double() - ref_pattern[idx]).abs().max().item())
    return worst


# ---------------------------------- fused_adam ----------------------------------

def adam_ref_step(p, g, m, v, t, lr, b1, b2, eps, wd, gscale, adamw):
    """One Adam / AdamW step in fp64 (torch.optim semantics)."""
    g = g * gscale
    if wd != 0.0:
        if adamw:
            p = p * (1.0 - lr * wd)
        else:
            g = g + wd * p
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1 = 1.0 - b1 ** t
    bc2 = 1.0 - b2 ** t
    p = p - (lr / bc1) * (m / (torch.sqrt(v / bc2) + eps))
    return p, m, v


def run_adam(n, t0, on_device, lr=0.01, betas=(0.9, 0.999), eps=1e-8, wd=0.0, gscale=1.0,
             adamw=False, steps=3):
    L = min(n, PATTERN)
    b1, b2 = betas
    p_ref = torch.randn(L).float().double()
    m_ref = torch.zeros(L, dtype=torch.float64)
    v_ref = torch.zeros(L, dtype=torch.float64)
    p = tiled(p_ref, n)
    m = torch.zeros_like(p)
    v = torch.zeros_like(p)
    step_dev = torch.tensor([t0 - 1], dtype=torch.int32, device=DEV) if on_device else None
    for k in range(steps):
        t = t0 + k
        g_pat = torch.randn(L).float().double()
        g = tiled(g_pat, n)
        if on_device:
            ops.ext().increment_i32(step_dev)
            bc1, bc2 = 0.5, 0.25  # wrong on purpose: the kernel must use step_dev
        else:
            bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        ops.ext().fused_adam(p, g, m, v, lr, b1, b2, eps, wd, bc1, bc2, gscale, adamw, step_dev)
        p_ref, m_ref, v_ref = adam_ref_step(p_ref, g_pat, m_ref, v_ref, t, lr, b1, b2, eps, wd,
                                            gscale, adamw)
    torch.cuda.synchronize()
    if on_device:
        assert step_dev.item() == t0 + steps - 1
    errs = (worst_err(p, p_ref), worst_err(m, m_ref), worst_err(v, v_ref))
    print("ADAM n=%d t0=%d dev=%d wd=%g adamw=%d gscale=%g betas=%s eps=%g: p %.3e m %.3e v %.3e"
          % ((n, t0, on_device, wd, adamw, gscale, betas, eps) + errs))
    assert max(errs) <= CAP, errs


@pytest.mark.parametrize("on_device", [False, True], ids=["host_bc", "step_dev"])
@pytest.mark.parametrize("n", SIZES)
def test_fused_adam_sizes(n, on_device):
    torch.manual_seed(n)
    run_adam(n, 1, on_device)


@pytest.mark.parametrize("t0", [1, 2, 1000])
def test_fused_adam_step_dev_bias_correction(t0):
    """Bias corrections computed in the kernel from the device step counter
    holding t0, t0 + 1, t0 + 2."""
    torch.manual_seed(7)
    run_adam(1027, t0, True)


ADAM_OPTIONS = {
    "wd_adam": dict(wd=0.01, adamw=False),
    "wd_adamw": dict(wd=0.01, adamw=True),
    "gscale": dict(gscale=0.25),
    "betas": dict(betas=(0.8, 0.99)),
    "eps": dict(eps=1e-6),
}


@pytest.mark.parametrize("on_device", [False, True], ids=["host_bc", "step_dev"])
@pytest.mark.parametrize("case", sorted(ADAM_OPTIONS))
def test_fused_adam_options(case, on_device):
    torch.manual_seed(8)
    run_adam(1027, 1, on_device, **ADAM_OPTIONS[case])


# ---------------------------------- fused_sgd ----------------------------------

SGD_CASES = {
    "plain": dict(),
    "momentum": dict(momentum=0.9),
    "dampening": dict(momentum=0.9, dampening=0.1),
    "nesterov": dict(momentum=0.9, nesterov=True),
    "wd": dict(momentum=0.9, weight_decay=1e-4),
    "gscale": dict(momentum=0.9, gscale=0.5),
    "no_momentum_buf": dict(weight_decay=1e-4),
}


def run_sgd(n, momentum=0.0, dampening=0.0, nesterov=False, weight_decay=0.0, gscale=1.0,
            lr=0.05, steps=4):
    """steps of the kernel against torch.optim.SGD on an fp64 parameter; the
    first step takes the kernel's `first` branch, the others the later one."""
    L = min(n, PATTERN)
    p_ref = nn.Parameter(torch.randn(L).float().double())
    opt = torch.optim.SGD([p_ref], lr=lr, momentum=momentum, dampening=dampening,
                          nesterov=nesterov, weight_decay=weight_decay)
    p = tiled(p_ref.detach(), n)
    has_momentum = momentum != 0.0
    buf = torch.zeros_like(p) if has_momentum else None
    for k in range(steps):
        g_pat = torch.randn(L).float().double()
        g = tiled(g_pat, n)
        ops.ext().fused_sgd(p, g, buf if has_momentum else g, lr, momentum, weight_decay,
                            dampening, gscale, nesterov, k == 0, has_momentum)
        p_ref.grad = g_pat * gscale
        opt.step()
    torch.cuda.synchronize()
    errs = [worst_err(p, p_ref.detach())]
    if has_momentum:
        errs.append(worst_err(buf, opt.state[p_ref]["momentum_buffer"]))
    print("SGD n=%d momentum=%g dampening=%g nesterov=%d wd=%g gscale=%g: %s"
          % (n, momentum, dampening, nesterov, weight_decay, gscale,
             " ".join("%.3e" % e for e in errs)))
    assert max(errs) <= CAP, errs


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case", ["plain", "momentum"])
def test_fused_sgd_sizes(case, n):
    torch.manual_seed(n + 1)
    run_sgd(n, **SGD_CASES[case])


@pytest.mark.parametrize("case", sorted(set(SGD_CASES) - {"plain", "momentum"}))
def test_fused_sgd_options(case):
    torch.manual_seed(9)
    run_sgd(1027, **SGD_CASES[case])


# ------------------------- FlatBuckets + fused_optimizer_for -------------------------

@pytest.mark.parametrize("name", ["adamw", "sgd_nesterov"])
def test_fused_optimizer_wrapper_matches_torch_gpu(name):
    """A small Net on the GPU: FlatBuckets + fused_optimizer_for against the
    torch optimizer it was mapped from, 5 steps."""
    make = {
        "adamw": (FusedAdam, lambda ps: torch.optim.AdamW(ps, lr=0.01, weight_decay=0.01)),
        "sgd_nesterov": (FusedSGD, lambda ps: torch.optim.SGD(ps, lr=0.05, momentum=0.9,
                                                              nesterov=True)),
    }[name]
    torch.manual_seed(11)
    ref = Net().to(DEV)
    fused_model = Net().to(DEV)
    fused_model.load_state_dict(ref.state_dict())
    ref_opt = make[1](ref.parameters())
    fb = FlatBuckets(list(fused_model.parameters()), world_size=1)
    fused_opt = fused_optimizer_for(make[1](fused_model.parameters()), fb)
    assert isinstance(fused_opt, make[0])
    assert fb.flat_pairs()[0][0].is_cuda

    crit = nn.MSELoss()
    x = torch.randn(32, 10).to(DEV)
    y = torch.randn(32, 1).to(DEV)
    for _ in range(5):
        ref_opt.zero_grad()
        crit(ref(x), y).backward()
        ref_opt.step()

        fb.zero_grad()
        crit(fused_model(x), y).backward()
        fb.finalize(average=False)
        fused_opt.step(grad_scale=1.0)
    torch.cuda.synchronize()
    worst = max((pa - pb).abs().max().item()
                for pa, pb in zip(ref.parameters(), fused_model.parameters()))
    print("WRAPPER %s worst |p - p_torch| = %.3e" % (name, worst))
    assert worst <= CAP


# ---------------------------------- bias_grad ----------------------------------

BIAS_SHAPES = [(4096, 8), (4097, 64), (4096, 2048), (4096, 40), (5000, 37), (1, 16), (63, 520)]


@pytest.mark.parametrize("M,N", BIAS_SHAPES)
def test_bias_grad_and_into(M, N):
    """The first three shapes take the scratch path (N % 8 == 0,
    256 % (N / 8) == 0, M >= 4096), the others the atomics path."""
    torch.manual_seed(M + N)
    # drawn and summed in row chunks of <= 1M elements: the largest shape is a
    # 16 MB bf16 tensor, its fp64 copy would be 64 MB
    rows = max(1, (1 << 20) // N)
    dz = torch.cat([bf(torch.randn(min(rows, M - r), N) + 0.25) for r in range(0, M, rows)])
    dz = dz.to(DEV)
    ref = torch.zeros(N, dtype=torch.float64, device=DEV)
    cap = torch.zeros(N, dtype=torch.float64, device=DEV)
    for r in range(0, M, rows):
        part = dz[r:r + rows].double()
        ref += part.sum(0)
        cap += 1e-5 * part.abs().sum(0)

    db = ops.ext().bias_grad(dz)
    over = ((db.double() - ref).abs() - cap).max().item()

    pattern = (torch.arange(N, dtype=torch.float32) * 0.125 - 3.3).to(DEV)
    acc = pattern.clone()
    ops.ext().bias_grad_into(dz, acc)
    # the pre-filled value is one more term of the chain
    over_into = ((acc.double() - (pattern.double() + ref)).abs()
                 - (cap + 1e-5 * pattern.double().abs())).max().item()
    print("BIAS M=%d N=%d (err - cap): bias_grad %.3e into %.3e, smallest cap %.3e"
          % (M, N, over, over_into, cap.min().item()))
    assert over <= 0.0
    assert over_into <= 0.0


# ------------------------------------ casts ------------------------------------

def _f32_bits(bits):
    return torch.tensor(bits, dtype=torch.int64).to(torch.int32).view(torch.float32)


def _s32(x):
    return x - (1 << 32) if x >= (1 << 31) else x


NAN_BITS = [0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0xFFFFFFFF]

F32_PATTERNS = [
    0x3F808000,  # 1 + 2^-8: tie, rounds down to even
    0x3F818000,  # tie, rounds up to even
    0xBF808000, 0xBF818000,  # the same ties, negative
    0x3F808001, 0x3F807FFF,  # just above / below a tie
    0x7F7FFFFF, 0xFF7FFFFF,  # largest finite fp32: rounds up to Inf
    0x7F7F7FFF, 0x7F7F8000,  # below / at the tie under the largest finite bf16
    0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x80000001,  # subnormals
    0x00800000,  # smallest normal
    0x00000000, 0x80000000,  # +-0
    0x7F800000, 0xFF800000,  # +-Inf
]

F64_PATTERNS = [
    1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8),  # bf16 ties (exact in fp32)
    1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24,  # fp32 ties, both ways
    1.0 + 2.0 ** -8 + 2.0 ** -40,  # above a bf16 tie only in fp64
    3.4028234663852886e38,  # largest finite fp32
    3.4028235677973366e38,  # halfway to 2^128: rounds to Inf in fp32
    3.3e38, 1e39, -1e39, 1e300,
    1e-40, -1e-40, 1e-45, 7e-46, 1e-46, 1e-320,  # fp32 subnormals, underflow, fp64 subnormal
    0.0, -0.0, math.inf, -math.inf,
]

F64_NAN_BITS = [0x7FF8000000000000, 0x7FF0000000000001, 0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF,
                0x7FF0000020000000]


def _padded(patterns, n):
    """n-long vector: the patterns first, then a ramp of ordinary values."""
    k = min(n, patterns.numel())
    out = (torch.arange(n, dtype=torch.float64) * 0.37 - 1234.5).to(patterns.dtype)
    out[:k] = patterns[:k]
    return out


def _assert_bits_equal(tag, got, want, nan_mask):
    got, want = got.cpu(), want.cpu()
    int_t = {2: torch.int16, 4: torch.int32}[got.element_size()]
    same = got.view(int_t) == want.view(int_t)
    ok = torch.where(nan_mask, torch.isnan(got.float()), same)
    bad = (~ok).nonzero().flatten().tolist()
    mask = (1 << (8 * got.element_size())) - 1
    bits = lambda t: [hex(v & mask) for v in t.view(int_t)[bad[:8]].tolist()]
    print("CAST %s: %d mismatches%s" % (tag, len(bad), "" if not bad else
          " at %s got %s want %s" % (bad[:8], bits(got), bits(want))))
    assert not bad, (tag, bad[:8])


@pytest.mark.parametrize("n", [1, 7, 10_001])
def test_cast_f32_bf16_bits(n):
    """With the rounding add applied to NaN bit patterns too (f32_to_bf16 of
    common.h, which the cast kernels used before), 0x7F800001 came out as
    0x7F80 = +Inf, 0x7FFFFFFF as 0x8000 = -0.0 and 0xFFFFFFFF as 0x0000 = +0.0
    (measured on the MI355X); 0x7FC00000 survived."""
    pats = _f32_bits([_s32(b) for b in F32_PATTERNS])
    nans = _f32_bits([_s32(b) for b in NAN_BITS])
    for tag, head in (("patterns", pats), ("nans", nans), ("mixed", torch.cat([nans, pats]))):
        # a 1-long run takes each value in turn, so every pattern meets the scalar tail
        starts = range(head.numel()) if n == 1 else [0]
        for s in starts:
            src = _padded(head[s:], n)
            got = ops.ext().cast_f32_bf16(src.to(DEV))
            _assert_bits_equal("f32->bf16 n=%d %s[%d]" % (n, tag, s), got, src.bfloat16(),
                               torch.isnan(src))


@pytest.mark.parametrize("n", [1, 7, 10_001])
def test_cast_f64_bits(n):
    pats = torch.tensor(F64_PATTERNS, dtype=torch.float64)
    nans = torch.tensor([b - (1 << 64) if b >= (1 << 63) else b for b in F64_NAN_BITS],
                        dtype=torch.int64).view(torch.float64)
    for tag, head in (("patterns", pats), ("nans", nans), ("mixed", torch.cat([nans, pats]))):
        starts = range(head.numel()) if n == 1 else [0]
        for s in starts:
            src = _padded(head[s:], n)
            dev = src.to(DEV)
            nan = torch.isnan(src)
            _assert_bits_equal("f64->f32 n=%d %s[%d]" % (n, tag, s), ops.ext().cast_f64_f32(dev),
                               src.float(), nan)
            _assert_bits_equal("f64->bf16 n=%d %s[%d]" % (n, tag, s),
                               ops.ext().cast_f64_bf16(dev), src.float().bfloat16(), nan)
