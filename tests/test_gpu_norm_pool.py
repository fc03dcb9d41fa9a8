"""BatchNorm, max-pool and global-average-pool kernels against float64
references computed from the bf16-quantized inputs, with the operation written
out in plain torch (biased variance for normalisation, unbiased for
running_var).

Tolerances are derived, not tuned:

* a bf16 output is one rounding of an fp32 value:
  |got - ref| <= 2^-8 |ref| + a, where a = 1e-5 * max|ref| + 1e-6 carries the
  relative invstd error the statistics are allowed (1e-5);
* invstd within 1e-5 relative, mean within 1e-6 * max(|mean|, std);
* running stats within 1e-5 relative (running_mean plus the allowed mean
  error times the momentum);
* dgamma / dbeta within the fp32 summation bound n * 2^-24 * sum|terms| of the
  channel, computed from the fp64 terms.  With a fused ReLU the mask of an
  element whose fp64 pre-activation lies within a of zero is undetermined, so
  its term is added to its channel's cap (and, divided by n, to that
  channel's dx tolerance);
* dx leaves out elements whose pre-activation lies within 1e-3 of zero; their
  share is asserted to stay <= 0.5 %;
* max-pool forward is bit-equal (a max of bf16 values is exact), backward is
  the fp64 scatter-sum rounded once to bf16, one bf16 ulp allowed.

Which test launches which kernel (NHWC routing by channel count C):

  norm.hip
    bn_stats_partial_kernel, bn_stats_finalize_kernel (NCHW)
        test_bn_stats_conditioning[nchw-16], test_bn_stats_small_extents_nchw,
        test_bn_running_stats[nchw-7], test_bn_fwd_bwd[nchw-*]
    bn_stats_partial_nhwc_kernel + bn_stats_finalize_kernel (C = 3, 24)
        test_bn_stats_conditioning[nhwc-24], test_bn_stats_small_extents_nhwc,
        test_bn_running_stats[nhwc-24], test_bn_fwd_bwd[nhwc-3 / nhwc-24]
    bn_stats_partial_nhwc_vec_kernel + bn_stats_finalize2_kernel
    (C = 8, 16, 64, 1024, 2048)
        test_bn_stats_conditioning[nhwc-16], test_bn_stats_small_extents_nhwc,
        test_bn_running_stats[nhwc-16], test_bn_fwd_bwd[nhwc-8 / 64 / 1024]
    bn_apply_kernel, bn_bwd_reduce_kernel, bn_bwd_dx_kernel (NCHW)
        test_bn_fwd_bwd[nchw-*], test_bn_apply_residual[nchw-16],
        test_bn_bwd_reduce_accumulates[nchw-7]
    bn_apply_nhwc_kernel (C = 3, 24) / bn_apply_nhwc_vec_kernel (8, 16, 64, 1024)
        test_bn_fwd_bwd[nhwc-*], test_bn_apply_residual[nhwc-24 / nhwc-16]
    bn_bwd_reduce_nhwc_kernel (C = 3, 24, atomics)
        test_bn_fwd_bwd[nhwc-3 / 24], test_bn_bwd_reduce_accumulates[nhwc-24]
    bn_bwd_reduce_nhwc_vec_kernel + bn_bwd_reduce_finalize_kernel (8, 16, 64, 1024)
        test_bn_fwd_bwd[nhwc-8 / 64 / 1024], test_bn_bwd_reduce_accumulates[nhwc-16]
    bn_bwd_dx_nhwc_kernel (C = 3, 24 and the mixed routing C = 1024, where the
    vec reduce recomputes the ReLU mask from x and the scalar dx reads the
    saved output) / bn_bwd_dx_nhwc_vec_kernel (8, 64)
        test_bn_fwd_bwd[nhwc-*]
    maxpool_gen_fwd_kernel, maxpool_gen_bwd_kernel
        test_maxpool_nchw (every geometry; (2,2,0) also through the disjoint
        maxpool_fwd / maxpool_bwd kernels of conv.hip, which the wrapper routes
        it to)
    gap_fwd_kernel, gap_bwd_kernel
        test_global_avg_pool_nchw
  conv_nhwc.hip
    maxpool_nhwc_fwd_kernel, maxpool_nhwc_bwd_kernel (C = 3, 12)
    maxpool_nhwc_fwd_vec_kernel, maxpool_nhwc_bwd_vec_kernel (C = 8)
        test_maxpool_nhwc
    gap_nhwc_fwd_kernel, gap_nhwc_bwd_kernel
        test_global_avg_pool_nhwc
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped off-GPU
    pytest.skip("needs MI355X", allow_module_level=True)

from sparktorch_amd import ops
from sparktorch_amd.ops.functional import (
    _MaxPool2dGenFn,
    hip_batch_norm2d,
    hip_batch_norm2d_nhwc,
    hip_global_avg_pool,
    hip_global_avg_pool_nhwc,
    hip_max_pool2d,
    hip_max_pool2d_nhwc,
)

DEV = "cuda:0"
BF16_REL = 2.0 ** -8   # one bf16 rounding of an fp32 value, with margin for the fp32 error
F32_EPS = 2.0 ** -24
INVSTD_REL = 1e-5      # allowed relative error of invstd
MEAN_REL = 1e-6        # allowed error of mean, relative to max(|mean|, std)


def bf(x):
    return x.to(torch.bfloat16)


def shape4(layout, B, C, H, W):
    return (B, C, H, W) if layout == "nchw" else (B, H, W, C)


def to_mc(t, layout):
    """[M, C] float64 matrix of a 4-d activation tensor (rows = B*H*W)."""
    t = t.detach().double()
    if layout == "nchw":
        t = t.permute(0, 2, 3, 1)
    return t.reshape(-1, t.shape[-1])


def chan_data(layout, B, C, H, W, mean, std):
    """bf16 activations, channel c ~ mean[c] + std[c] * N(0, 1); drawn on the
    CPU generator so a seed fixes them."""
    m = torch.as_tensor(mean, dtype=torch.float32).expand(C)
    s = torch.as_tensor(std, dtype=torch.float32).expand(C)
    x = torch.randn(B * H * W, C) * s + m
    x = x.reshape(B, H, W, C)
    if layout == "nchw":
        x = x.permute(0, 3, 1, 2)
    return bf(x.contiguous()).to(DEV)


# ----------------------------- ext call adapters -----------------------------

def ext_stats(layout, x, rm, rv, momentum, eps):
    e = ops.ext()
    return (e.bn_stats if layout == "nchw" else e.bn_stats_nhwc)(x, rm, rv, momentum, eps)


def ext_apply(layout, x, res, mean, invstd, gamma, beta, relu):
    e = ops.ext()
    return (e.bn_apply if layout == "nchw" else e.bn_apply_nhwc)(x, res, mean, invstd, gamma,
                                                                 beta, relu)


def ext_reduce(layout, dy, yrelu, x, mean, invstd, gamma, beta, dbeta, dgamma):
    e = ops.ext()
    if layout == "nchw":
        e.bn_bwd_reduce(dy, yrelu, x, mean, invstd, dbeta, dgamma)
    else:
        e.bn_bwd_reduce_nhwc(dy, yrelu, x, mean, invstd, gamma, beta, dbeta, dgamma)


# ------------------------------ fp64 references ------------------------------

def ref_stats(X, eps):
    """mean, biased var, invstd of the [M, C] fp64 matrix X."""
    mean = X.mean(0)
    var = ((X - mean) ** 2).mean(0)
    return mean, var, 1.0 / torch.sqrt(var + eps)


def check_stats(tag, mean, invstd, X, eps):
    rmean, rvar, rinv = ref_stats(X, eps)
    inv_rel = ((invstd.double() - rinv).abs() / rinv).max().item()
    scale = torch.maximum(rmean.abs(), rvar.sqrt())
    mean_rel = ((mean.double() - rmean).abs() / scale.clamp_min(1e-30)).max().item()
    print("BNSTATS %s invstd_rel=%.3e mean_err_over_scale=%.3e" % (tag, inv_rel, mean_rel))
    assert inv_rel <= INVSTD_REL, (tag, inv_rel)
    assert mean_rel <= MEAN_REL, (tag, mean_rel)


def bf16_close(tag, got, ref, extra=0.0, keep=None):
    """|got - ref| <= 2^-8 |ref| + 1e-5 max|ref| + 1e-6 (+ extra), on `keep`."""
    got = got.double()
    a = INVSTD_REL * ref.abs().max().item() + 1e-6
    tol = BF16_REL * ref.abs() + a + extra
    over = (got - ref).abs() - tol
    if keep is not None:
        over = torch.where(keep, over, torch.full_like(over, -1.0))
    worst = over.max().item()
    print("BF16OUT %s worst (err - tol)=%.3e, a=%.3e" % (tag, worst, a))
    assert worst <= 0.0, (tag, worst)


def bn_reference(X, G, gamma, beta, mean, invstd, relu, train, R=None):
    """Everything BN computes, in fp64 on [M, C] matrices, with the caps of
    the fp32 reductions."""
    n = X.shape[0]
    xhat = (X - mean) * invstd
    pre = xhat * gamma + beta
    if R is not None:
        pre = pre + R
    y = pre.clamp_min(0.0) if relu else pre
    out = {"y": y, "pre": pre}
    if G is None:
        return out
    live = (pre > 0).double() if relu else torch.ones_like(pre)
    tb = G * live
    tg = tb * xhat
    out["dbeta"], out["dgamma"] = tb.sum(0), tg.sum(0)
    cap_b = n * F32_EPS * tb.abs().sum(0)
    cap_g = n * F32_EPS * tg.abs().sum(0)
    if relu:
        a = INVSTD_REL * y.abs().max().item() + 1e-6
        unsure = (pre.abs() <= a).double()
        cap_b = cap_b + (G.abs() * unsure).sum(0)
        cap_g = cap_g + ((G * xhat).abs() * unsure).sum(0)
    out["cap_b"], out["cap_g"] = cap_b, cap_g
    if train:
        out["dx"] = gamma * invstd * (tb - out["dbeta"] / n - xhat * out["dgamma"] / n)
        # what the allowed dbeta / dgamma error may move dx by
        out["dx_extra"] = (gamma * invstd).abs() * (cap_b + xhat.abs() * cap_g) / n
    else:
        out["dx"] = gamma * invstd * tb
        out["dx_extra"] = torch.zeros_like(pre)
    return out


def check_sums(tag, got, ref, cap):
    over = ((got.double() - ref).abs() - cap).max().item()
    print("BNSUM %s worst (err - cap)=%.3e, smallest cap=%.3e" % (tag, over, cap.min().item()))
    assert over <= 0.0, (tag, over)


# ------------------------------- BN statistics -------------------------------

SWEEP = [(0.0, 1.0), (32.0, 1.0), (100.0, 0.5), (200.0, 1.0), (1000.0, 4.0), (3.0, 0.02),
         (-200.0, 1.0)]


@pytest.mark.parametrize("mu,sd", SWEEP)
@pytest.mark.parametrize("layout,C", [("nchw", 16), ("nhwc", 16), ("nhwc", 24)])
def test_bn_stats_conditioning(layout, C, mu, sd):
    """2048 values per channel at growing mean/std: one-pass E[x^2] - E[x]^2 in
    fp32 missed the invstd cap from mean/std = 32 upward (measured on the
    MI355X: 5e-5 to 2e-4 at 32/1, up to 1.5e-2 at -200/1 in the NHWC scalar
    kernel); sums shifted by a per-channel pivot meet it with 8.5e-7 at worst
    (profiles/bn_stats_shift.md)."""
    torch.manual_seed(100 + C)
    eps = 1e-5
    x = chan_data(layout, 8, C, 16, 16, mu, sd)
    mean, invstd = ext_stats(layout, x, None, None, 0.1, eps)
    check_stats("sweep %s C=%d mean=%g std=%g" % (layout, C, mu, sd), mean, invstd,
                to_mc(x, layout), eps)


def _chan_params(C):
    m = torch.linspace(-2.0, 2.0, C)
    s = torch.linspace(0.5, 1.5, C).flip(0)
    return m, s


@pytest.mark.parametrize("shape", [(3, 7, 5, 9), (2, 5, 1, 1), (1, 300, 2, 3)])
def test_bn_stats_small_extents_nchw(shape):
    torch.manual_seed(3)
    B, C, H, W = shape
    eps = 1e-5
    x = chan_data("nchw", B, C, H, W, *_chan_params(C))
    mean, invstd = ext_stats("nchw", x, None, None, 0.1, eps)
    check_stats("nchw %s" % (shape,), mean, invstd, to_mc(x, "nchw"), eps)


@pytest.mark.parametrize("C", [3, 8, 24, 64, 1024, 2048])
def test_bn_stats_small_extents_nhwc(C):
    """30 rows: fewer than the 64 scratch slices / the row splits, so most
    blocks own an empty range."""
    torch.manual_seed(4)
    eps = 1e-5
    x = chan_data("nhwc", 1, C, 5, 6, *_chan_params(C))
    mean, invstd = ext_stats("nhwc", x, None, None, 0.1, eps)
    check_stats("nhwc M=30 C=%d" % C, mean, invstd, to_mc(x, "nhwc"), eps)


@pytest.mark.parametrize("layout,C", [("nchw", 7), ("nhwc", 16), ("nhwc", 24)])
def test_bn_running_stats(layout, C):
    """30 values per channel (biased and unbiased variance 3 % apart),
    momentum 0.3, eps 1e-3, non-trivial initial running stats."""
    torch.manual_seed(5)
    momentum, eps = 0.3, 1e-3
    x = chan_data(layout, 2, C, 3, 5, *_chan_params(C))
    X = to_mc(x, layout)
    n = X.shape[0]
    assert n == 30
    rm0 = (torch.randn(C) * 0.7 + 0.3).to(DEV)
    rv0 = (torch.rand(C) + 0.5).to(DEV)
    rm, rv = rm0.clone(), rv0.clone()
    mean, invstd = ext_stats(layout, x, rm, rv, momentum, eps)
    check_stats("running %s C=%d" % (layout, C), mean, invstd, X, eps)

    rmean, rvar, _ = ref_stats(X, eps)
    ref_rm = (1 - momentum) * rm0.double() + momentum * rmean
    ref_rv = (1 - momentum) * rv0.double() + momentum * rvar * n / (n - 1)
    cap_rm = 1e-5 * ref_rm.abs() + momentum * MEAN_REL * torch.maximum(rmean.abs(), rvar.sqrt())
    err_rm = ((rm.double() - ref_rm).abs() - cap_rm).max().item()
    err_rv = ((rv.double() - ref_rv).abs() / ref_rv).max().item()
    print("BNRUN %s C=%d running_mean (err - cap)=%.3e running_var rel=%.3e"
          % (layout, C, err_rm, err_rv))
    assert err_rm <= 0.0
    assert err_rv <= 1e-5

    # without running stats: same mean / invstd, and nothing of the earlier
    # buffers is written
    rm_keep, rv_keep = rm.clone(), rv.clone()
    mean2, invstd2 = ext_stats(layout, x, None, None, momentum, eps)
    check_stats("running=None %s C=%d" % (layout, C), mean2, invstd2, X, eps)
    assert torch.equal(rm, rm_keep) and torch.equal(rv, rv_keep)


# --------------------------- BN apply / reduce / dx ---------------------------

def _bn_case(layout, C, rows):
    B, H, W = rows
    x = chan_data(layout, B, C, H, W, *_chan_params(C))
    gamma = (torch.rand(C) + 0.5) * torch.where(torch.arange(C) % 3 == 2, -1.0, 1.0)
    beta = torch.randn(C) * 0.5
    g = bf(torch.randn(shape4(layout, B, C, H, W))).to(DEV)
    return x, gamma.to(DEV), beta.to(DEV), g


BN_SHAPES = [
    ("nchw", 7, (3, 5, 9)),
    ("nchw", 16, (4, 6, 6)),
    ("nhwc", 3, (4, 9, 11)),
    ("nhwc", 8, (4, 9, 11)),
    ("nhwc", 24, (4, 9, 11)),
    ("nhwc", 64, (2, 6, 11)),
    ("nhwc", 1024, (2, 6, 11)),
]


@pytest.mark.parametrize("relu", [False, True], ids=["lin", "relu"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("layout,C,rows", BN_SHAPES, ids=["%s-%d" % (l, c) for l, c, _ in BN_SHAPES])
def test_bn_fwd_bwd(layout, C, rows, train, relu):
    """The autograd wrappers (bn_stats*, bn_apply*, bn_bwd_reduce*, bn_bwd_dx*
    underneath) in training and eval mode, with and without the fused ReLU."""
    torch.manual_seed(20 + C)
    momentum, eps = 0.2, 1e-4
    x, gamma, beta, g = _bn_case(layout, C, rows)
    rm0 = (torch.randn(C) * 0.5).to(DEV)
    rv0 = (torch.rand(C) + 0.5).to(DEV)
    rm, rv = rm0.clone(), rv0.clone()

    xr = x.clone().requires_grad_(True)
    gr = gamma.clone().requires_grad_(True)
    br = beta.clone().requires_grad_(True)
    fn = hip_batch_norm2d if layout == "nchw" else hip_batch_norm2d_nhwc
    y = fn(xr, gr, br, rm, rv, training=train, momentum=momentum, eps=eps, relu=relu)
    y.backward(g)

    X, G = to_mc(x, layout), to_mc(g, layout)
    n = X.shape[0]
    if train:
        mean, var, invstd = ref_stats(X, eps)
    else:
        mean, invstd = rm0.double(), 1.0 / torch.sqrt(rv0.double() + eps)
    ref = bn_reference(X, G, gamma.double(), beta.double(), mean, invstd, relu, train)
    tag = "%s C=%d %s %s" % (layout, C, "train" if train else "eval", "relu" if relu else "lin")

    bf16_close("y " + tag, to_mc(y, layout), ref["y"])
    check_sums("dbeta " + tag, br.grad, ref["dbeta"], ref["cap_b"])
    check_sums("dgamma " + tag, gr.grad, ref["dgamma"], ref["cap_g"])

    keep = None
    if relu:
        keep = ref["pre"].abs() >= 1e-3
        share = 1.0 - keep.double().mean().item()
        print("BNEDGE %s excluded share=%.4f" % (tag, share))
        assert share <= 0.005, share
    bf16_close("dx " + tag, to_mc(xr.grad, layout), ref["dx"], extra=ref["dx_extra"], keep=keep)

    if train:
        ref_rm = (1 - momentum) * rm0.double() + momentum * mean
        ref_rv = (1 - momentum) * rv0.double() + momentum * var * n / (n - 1)
        cap_rm = 1e-5 * ref_rm.abs() + momentum * MEAN_REL * torch.maximum(mean.abs(), var.sqrt())
        assert ((rm.double() - ref_rm).abs() <= cap_rm).all()
        assert ((rv.double() - ref_rv).abs() <= 1e-5 * ref_rv).all()
    else:
        # eval leaves the running stats alone, to the bit
        assert torch.equal(rm, rm0) and torch.equal(rv, rv0)


@pytest.mark.parametrize("relu", [False, True], ids=["lin", "relu"])
@pytest.mark.parametrize("layout,C", [("nchw", 16), ("nhwc", 16), ("nhwc", 24)])
def test_bn_apply_residual(layout, C, relu):
    """y = bn(x) + res (+ relu): C=16 takes the NHWC vec kernel, C=24 the
    scalar one."""
    torch.manual_seed(30 + C)
    eps = 1e-5
    B, H, W = 3, 5, 7
    x, gamma, beta, _ = _bn_case(layout, C, (B, H, W))
    res = bf(torch.randn(shape4(layout, B, C, H, W)) * 1.5).to(DEV)
    X = to_mc(x, layout)
    mean, _, invstd = ref_stats(X, eps)
    y = ext_apply(layout, x, res, mean.float(), invstd.float(), gamma, beta, relu)
    ref = bn_reference(X, None, gamma.double(), beta.double(), mean, invstd, relu, True,
                       R=to_mc(res, layout))
    bf16_close("residual %s C=%d relu=%d" % (layout, C, relu), to_mc(y, layout), ref["y"])
    # and the residual really is used
    y0 = ext_apply(layout, x, None, mean.float(), invstd.float(), gamma, beta, relu)
    assert not torch.equal(y0, y)


@pytest.mark.parametrize("layout,C", [("nchw", 7), ("nhwc", 16), ("nhwc", 24)])
def test_bn_bwd_reduce_accumulates(layout, C):
    """dbeta / dgamma are added into what the buffers hold: atomics (NCHW,
    NHWC C=24) and the scratch finalize's += (NHWC C=16)."""
    torch.manual_seed(40 + C)
    eps = 1e-5
    x, gamma, beta, g = _bn_case(layout, C, (3, 5, 9))
    X, G = to_mc(x, layout), to_mc(g, layout)
    n = X.shape[0]
    mean, _, invstd = ref_stats(X, eps)
    ref = bn_reference(X, G, gamma.double(), beta.double(), mean, invstd, False, True)
    pat_b = (torch.arange(C, dtype=torch.float32) * 0.25 - 1.37).to(DEV)
    pat_g = (torch.arange(C, dtype=torch.float32) * -0.5 + 2.21).to(DEV)
    dbeta, dgamma = pat_b.clone(), pat_g.clone()
    ext_reduce(layout, g, None, x, mean.float(), invstd.float(), gamma, beta, dbeta, dgamma)
    # the pattern is one more term of the fp32 chain
    check_sums("acc dbeta %s C=%d" % (layout, C), dbeta, pat_b.double() + ref["dbeta"],
               ref["cap_b"] + n * F32_EPS * pat_b.double().abs())
    check_sums("acc dgamma %s C=%d" % (layout, C), dgamma, pat_g.double() + ref["dgamma"],
               ref["cap_g"] + n * F32_EPS * pat_g.double().abs())


# ---------------------------------- max-pool ----------------------------------

POOL_GEOMS = [(3, 2, 1), (2, 2, 0), (3, 1, 1), (2, 3, 0), (5, 2, 2)]
POOL_H, POOL_W = 7, 10


def _tie_free(n):
    # integers mod 251 scaled by 1/128 are exact in bf16; two cells of a window
    # are < 251 scan positions apart in NCHW, and in NHWC their distance
    # (dh * W + dw) * C is no multiple of the prime 251, so a window has no ties
    return (((torch.arange(n) * 97) % 251).float() - 125.0) / 128.0


def _bf16_ordinal(t):
    """bf16 values as integers that count ulps across zero."""
    b = t.contiguous().view(torch.int16).int()
    return torch.where(b >= 0, b, -(b & 0x7FFF))


def _pool_reference(x_nchw, g_nchw, ks, s, p):
    """fp64 max_pool2d and its scatter-sum gradient on the CPU."""
    x2 = x_nchw.detach().double().cpu().requires_grad_(True)
    y2 = F.max_pool2d(x2, ks, stride=s, padding=p)
    y2.backward(g_nchw.detach().double().cpu())
    return y2.detach(), x2.grad


def _check_pool(tag, y, dx, x_nchw, g_nchw, ks, s, p):
    """y, dx given as NCHW views of the kernel results."""
    y_ref, dx_ref = _pool_reference(x_nchw, g_nchw, ks, s, p)
    assert torch.equal(y.cpu().view(torch.int16), bf(y_ref).view(torch.int16)), tag
    ulps = (_bf16_ordinal(dx.cpu()) - _bf16_ordinal(bf(dx_ref))).abs().max().item()
    print("POOL %s dx worst ulp distance=%d" % (tag, ulps))
    assert ulps <= 1, (tag, ulps)
    if s > ks:
        H, W = x_nchw.shape[2:]
        HO, WO = (H + 2 * p - ks) // s + 1, (W + 2 * p - ks) // s + 1
        cov_h = torch.zeros(H, dtype=torch.bool)
        cov_w = torch.zeros(W, dtype=torch.bool)
        for o in range(HO):
            cov_h[max(o * s - p, 0):o * s - p + ks] = True
        for o in range(WO):
            cov_w[max(o * s - p, 0):o * s - p + ks] = True
        uncovered = ~(cov_h[:, None] & cov_w[None, :])
        assert uncovered.any()
        assert (dx.cpu().float()[:, :, uncovered] == 0).all(), tag


@pytest.mark.parametrize("ks,s,p", POOL_GEOMS)
@pytest.mark.parametrize("C", [3, 8, 12])
def test_maxpool_nchw(C, ks, s, p):
    torch.manual_seed(50)
    B, H, W = 2, POOL_H, POOL_W
    x = bf(_tie_free(B * C * H * W).reshape(B, C, H, W)).to(DEV)
    HO, WO = (H + 2 * p - ks) // s + 1, (W + 2 * p - ks) // s + 1
    g = bf(torch.randn(B, C, HO, WO)).to(DEV)
    paths = [("wrapper", lambda t: hip_max_pool2d(t, ks, stride=s, padding=p))]
    if s == ks and p == 0:  # the wrapper took the disjoint kernels: run the general ones too
        paths.append(("general", lambda t: _MaxPool2dGenFn.apply(t, ks, s, p)))
    for name, fn in paths:
        xr = x.clone().requires_grad_(True)
        y = fn(xr)
        y.backward(g)
        _check_pool("nchw %s C=%d %s" % (name, C, (ks, s, p)), y.detach(), xr.grad, x, g, ks, s, p)


@pytest.mark.parametrize("ks,s,p", POOL_GEOMS)
@pytest.mark.parametrize("C", [3, 8, 12])
def test_maxpool_nhwc(C, ks, s, p):
    """C = 3, 12 take the scalar kernels, C = 8 the 8-channel vector ones."""
    torch.manual_seed(51)
    B, H, W = 2, POOL_H, POOL_W
    x = bf(_tie_free(B * C * H * W).reshape(B, H, W, C)).to(DEV)
    HO, WO = (H + 2 * p - ks) // s + 1, (W + 2 * p - ks) // s + 1
    g = bf(torch.randn(B, HO, WO, C)).to(DEV)
    xr = x.clone().requires_grad_(True)
    y = hip_max_pool2d_nhwc(xr, ks, stride=s, padding=p)
    y.backward(g)
    nchw = lambda t: t.detach().permute(0, 3, 1, 2).contiguous()
    _check_pool("nhwc C=%d %s" % (C, (ks, s, p)), nchw(y), nchw(xr.grad), nchw(x), nchw(g),
                ks, s, p)


# ----------------------------- global average pool -----------------------------

def _check_gap(tag, y, dx, X3, G2):
    """X3: [B, HW, C] fp64 inputs, G2: [B, C] fp64 output gradients; y [B, C]
    and dx [B, HW, C] are the kernel results."""
    hw = X3.shape[1]
    y_ref = X3.mean(1)
    # fp32 sum of HW values: HW * 2^-24 * sum|x|, then / HW
    tol = BF16_REL * y_ref.abs() + F32_EPS * X3.abs().sum(1) + 1e-30
    over = ((y.double() - y_ref).abs() - tol).max().item()
    dx_ref = (G2 / hw)[:, None, :].expand_as(X3)
    over_dx = ((dx.double() - dx_ref).abs() - BF16_REL * dx_ref.abs()).max().item()
    print("GAP %s y (err - tol)=%.3e dx (err - tol)=%.3e" % (tag, over, over_dx))
    assert over <= 0.0 and over_dx <= 0.0, (tag, over, over_dx)


@pytest.mark.parametrize("H,W", [(1, 1), (7, 7), (15, 20)])
@pytest.mark.parametrize("C", [3, 70])
def test_global_avg_pool_nchw(C, H, W):
    torch.manual_seed(60)
    B = 3
    x = bf(torch.randn(B, C, H, W) + 0.5).to(DEV)
    g = bf(torch.randn(B, C)).to(DEV)
    xr = x.clone().requires_grad_(True)
    y = hip_global_avg_pool(xr)
    assert y.shape == (B, C)
    y.backward(g)
    flat = lambda t: t.detach().double().reshape(B, C, H * W).permute(0, 2, 1)
    _check_gap("nchw C=%d HW=%d" % (C, H * W), y.detach(), flat(xr.grad), flat(x), g.double())


@pytest.mark.parametrize("H,W", [(1, 1), (7, 7), (15, 20)])
@pytest.mark.parametrize("C", [3, 70, 300])
def test_global_avg_pool_nhwc(C, H, W):
    torch.manual_seed(61)
    B = 3
    x = bf(torch.randn(B, H, W, C) + 0.5).to(DEV)
    g = bf(torch.randn(B, C)).to(DEV)
    xr = x.clone().requires_grad_(True)
    y = hip_global_avg_pool_nhwc(xr)
    assert y.shape == (B, C)
    y.backward(g)
    flat = lambda t: t.detach().double().reshape(B, H * W, C)
    _check_gap("nhwc C=%d HW=%d" % (C, H * W), y.detach(), flat(xr.grad), flat(x), g.double())
