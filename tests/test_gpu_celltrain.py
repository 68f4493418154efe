"""GPU (-m gpu): training the cell head on the HIP library -- the training-mode BatchNorm kernels alone through the C ABI (clsconv with ldiff_conv_args.bn_stats,
ldiff_op_bn_finalize, ldiff_op_bn_apply, ldiff_op_cls_head_feat), ldiff_resnet_forward_train against the float64 restatement (tests/resnet_train_ref.py), and
Segmentor.train_cell_model end to end.

Error model of the statistics (derived, not tuned).  Row i of the conv has the fp32 accumulator a_i = y_i (1 + ...) with |a_i - y_i| <= e_i = (K + 2) 2^-24 sum |x w|
(the conv tests' accumulation term).  A partial is a sum of at most L = 8 chained fp32 additions (the kernel's comment states L; `chain_length()` reads it there), the
partials are added in double.  Per channel:
    |S_lib  - S |  <=  sum e_i + L 2^-24 sum |y_i|
    |S2_lib - S2|  <=  sum (2 |y_i| e_i + e_i^2) + (L + 1) 2^-24 sum y_i^2        (one more rounding: the square's fma)"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kernel_routing
import resnet_ref
import resnet_train_ref as tref
from ldiffusion_amd import _lib, cellhead
from ldiffusion_amd.models import ResNetClassifier
from test_gpu_cellhead import conv_reference, nhwc16, reached, stream, synthetic_label_map

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
U16 = 2.0 ** -11
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def chain_length():
    """L, the longest chain of fp32 additions into one partial, as the kernel's comment states it."""
    src = open(os.path.join(ROOT, "ldiffusion_amd", "csrc", "kernels_cls.hip")).read()
    return int(re.search(r"LONGEST CHAIN of fp32 additions into one partial: L = MT \+ 4 <= (\d+)", src).group(1))


# ---- 1. clsconv with the batch-statistics epilogue ---------------------------------------------------------------------------------------------------
def bn_conv_args(x, w, stride):
    """ldiff_conv_args of a raw classifier conv with bn_stats (no bias, residual or ReLU; cls_conv = 1); returns (args, y, partials [N, R, 2], keep-alive list)."""
    B, Cin, H, W = x.shape
    Cout, _, ks, _ = w.shape
    cpad = (Cin + 7) // 8 * 8
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    xd = nhwc16(x, cpad)
    wm = torch.zeros((Cout, ks, ks, cpad), dtype=torch.float16)
    wm[..., :Cin] = w.permute(0, 2, 3, 1).to(torch.float16)
    wd = wm.reshape(Cout, -1).contiguous().to(DEV)
    y = torch.full((B, Ho, Wo, Cout), float("nan"), dtype=torch.float16, device=DEV)
    a = _lib.ConvArgs()
    a.x, a.C1, a.B, a.Hin, a.Win, a.Hout, a.Wout = xd.data_ptr(), cpad, B, H, W, Ho, Wo
    a.ks, a.stride, a.pad_t, a.pad_l = ks, stride, ks // 2, ks // 2
    a.w, a.N, a.Nrows, a.n_real = wd.data_ptr(), Cout, Cout, Cout
    a.y, a.ldy, a.cls_conv = y.data_ptr(), Cout, 1
    R = _lib.load().ldiff_op_conv_bn_stats_blocks(C.byref(a))
    assert R > 0, _lib.load().ldiff_last_error()
    part = torch.full((Cout, R, 2), float("nan"), dtype=torch.float32, device=DEV)
    a.bn_stats = part.data_ptr()
    return a, y, part, [xd, wd]


def run_bn_conv(lib, x, w, stride):
    """(y [M, N] float64, partials [N, R, 2] float64, rows per partial from the kernel's name, kernel names)."""
    a, y, part, keep = bn_conv_args(x, w, stride)
    with reached(lib) as names:
        _lib.check(lib.ldiff_op_conv(C.byref(a), stream()))
    torch.cuda.synchronize()
    bn = [n for n in names if n.endswith(",bn>")]
    assert len(bn) == 1 and len(names) == 1, names
    rows = int(re.match(r"clsconv<\dx\d,\d+x(\d+),bn>", bn[0]).group(1))
    M = y.shape[0] * y.shape[1] * y.shape[2]
    assert part.shape[1] == 4 * ((M + 4 * rows - 1) // (4 * rows))
    return y.reshape(M, -1).double().cpu(), part.double().cpu(), rows, bn[0]


# (ks, Cin, Cout, stride, H, W, B, kernel): M = 33635 on the <4,4> tile with a ragged last workgroup; <1,1> with M = 27 < 64; M = 5, one partly filled wave; the
# stem; 64 -> 16 channels on a 64 x 64 map at B = 8 (M = 32768: 512 workgroups of the <1,1> tile -- the plan gives 16 output channels the 64-pixel wave tile only from
# 512 workgroups of 256 rows on); <1,4>: 32 channels at B = 16, 512 such workgroups
BN_CONV_CASES = [(1, 64, 256, 1, 31, 31, 35, "clsconv<1x1,64x64,bn>"), (3, 16, 16, 2, 5, 5, 3, "clsconv<3x3,16x16,bn>"), (1, 32, 64, 1, 1, 1, 5, "clsconv<1x1,64x16,bn>"),
                 (7, 8, 16, 2, 32, 32, 2, "clsconv<7x7,16x16,bn>"), (3, 64, 16, 1, 64, 64, 8, "clsconv<3x3,16x16,bn>"), (3, 64, 32, 1, 64, 64, 16, "clsconv<3x3,16x64,bn>")]


def block_sums(v, rows, R):
    """v [M, N] float64 -> [N, R] sums over the rows of each partial's row block (blocks past M: zero)."""
    M, N = v.shape
    pad = torch.zeros((R * rows, N), dtype=torch.float64)
    pad[:M] = v
    return pad.view(R, rows, N).sum(1).t()


@pytest.mark.parametrize("ks,cin,cout,stride,H,W,B,kernel", BN_CONV_CASES)
def test_bn_conv_exact_on_integers(lib, ks, cin, cout, stride, H, W, B, kernel):
    """Small integers: every product, every sum and every square's sum stays an integer below 2^24, so the raw output, each partial's sum and sum of squares are
    exact, the partials of row blocks past M are zero, and two launches give identical bytes."""
    g = torch.Generator().manual_seed(ks * 100 + cout)
    x = torch.randint(-2, 3, (B, cin, H, W), generator=g).float()
    w = torch.randint(-1, 2, (cout, cin, ks, ks), generator=g).float()
    y, part, rows, name = run_bn_conv(lib, x, w, stride)
    assert name == kernel
    want = F.conv2d(x.double(), w.double(), None, stride=stride, padding=ks // 2).permute(0, 2, 3, 1).reshape(y.shape)
    R = part.shape[1]
    s, q = block_sums(want, rows, R), block_sums(want * want, rows, R)
    assert want.abs().max().item() < 2048 and q.max().item() < 2 ** 24, "the case is not exact in fp32 / fp16"
    assert torch.equal(y, want)
    assert torch.equal(part[..., 0], s) and torch.equal(part[..., 1], q)
    first_empty = (y.shape[0] + rows - 1) // rows
    assert first_empty == R or not part[:, first_empty:].any()
    assert torch.equal(part[..., 0].sum(1), want.sum(0)) and torch.equal(part[..., 1].sum(1), (want * want).sum(0))
    y2, part2, _, _ = run_bn_conv(lib, x, w, stride)
    assert torch.equal(y2, y) and torch.equal(part2, part)


def stats_bound(x, w, stride, L):
    """(y [M, N] float64, per-element bound of the raw output, per-channel bounds of S and S2) of the module docstring."""
    ks = w.shape[2]
    y, tol = conv_reference(x, w, torch.zeros(w.shape[0]), stride, None, False)
    K = ks * ks * x.shape[1]
    e = (K + 2) * U * F.conv2d(x.double().abs(), w.double().abs(), None, stride=stride, padding=ks // 2)
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
    y, tol, e = flat(y), flat(tol), flat(e)
    tol_s = e.sum(0) + L * U * y.abs().sum(0)
    tol_q = (2 * y.abs() * e + e * e).sum(0) + (L + 1) * U * (y * y).sum(0)
    return y, tol, tol_s, tol_q


@pytest.mark.parametrize("ks,cin,cout,stride,H,W,B,kernel", BN_CONV_CASES + [(1, 32, 64, 1, 9, 9, 3, "clsconv<1x1,64x16,bn>")])
def test_bn_conv_against_float64(lib, ks, cin, cout, stride, H, W, B, kernel):
    """Random fp16 operands: the raw output inside clsconv's per-element bound, the channel totals of the partials inside the docstring's bounds, which reject the
    sums of a shifted tap.  The last case has channel means of at least 8 standard deviations (the cancellation case of var = E[y^2] - mean^2)."""
    L = chain_length()
    assert L == 8
    g = torch.Generator().manual_seed(ks * 1000 + cout * 10 + H)
    offset_case = (H, W) == (9, 9)
    if offset_case:
        x = (torch.randn((B, cin, H, W), generator=g) * 0.1 + 1.0).to(torch.float16).float()
        w = (torch.randn((cout, cin, ks, ks), generator=g).abs() * 0.2 + 0.05).to(torch.float16).float()
    else:
        x = (torch.randn((B, cin, H, W), generator=g) * 1.2 + 0.2).to(torch.float16).float()
        w = (torch.randn((cout, cin, ks, ks), generator=g) * (2.0 / (ks * ks * cin)) ** 0.5).to(torch.float16).float()
    got, part, rows, name = run_bn_conv(lib, x, w, stride)
    assert name == kernel
    y, tol, tol_s, tol_q = stats_bound(x, w, stride, L)
    if offset_case:
        assert (y.mean(0).abs() / y.std(0)).min().item() >= 8.0
    assert ((got - y).abs() <= tol).all()
    s, q = part[..., 0].sum(1), part[..., 1].sum(1)
    rs, rq = ((s - y.sum(0)).abs() / tol_s).max().item(), ((q - (y * y).sum(0)).abs() / tol_q).max().item()
    print(f"[bn conv] {name} M={y.shape[0]}: sum {rs:.3f}, sum of squares {rq:.3f} of the bound")
    assert rs <= 1.0 and rq <= 1.0
    shifted = torch.roll(w, 1, 3) if ks > 1 else torch.roll(w, 1, 1)
    wrong = stats_bound(x, shifted, stride, L)[0]
    assert ((s - wrong.sum(0)).abs() > tol_s).float().mean().item() > 0.5 and ((q - (wrong * wrong).sum(0)).abs() > tol_q).float().mean().item() > 0.5


def test_bn_conv_refusals(lib):
    """bn_stats is the classifier family's raw form on request or it is refused; the per-image `stats` field keeps its meaning beside cls_conv = 1."""
    g = torch.Generator().manual_seed(3)
    x, w = torch.randn((2, 64, 8, 8), generator=g), torch.randn((64, 64, 3, 3), generator=g) * 0.1
    bias = torch.zeros(64, device=DEV)
    res = torch.zeros((2, 8, 8, 64), dtype=torch.float16, device=DEV)
    for field, value in (("bias", bias.data_ptr()), ("res", res.data_ptr()), ("relu_out", 1), ("cls_conv", 0), ("cls_conv", -1), ("pad_t", 0)):
        a, y, part, keep = bn_conv_args(x, w, 1)
        setattr(a, field, value)
        if field == "res":
            a.ld_res = 64
        with pytest.raises(ValueError, match="bn_stats"):
            _lib.check(lib.ldiff_op_conv(C.byref(a), stream()))
        torch.cuda.synchronize()
        assert torch.isnan(part).all()            # nothing was launched
    a, y, part, keep = bn_conv_args(x, w, 1)         # cls_conv = 1 with `stats` set: the route of before (never this family), bn_stats beside it refused
    st = torch.zeros(2 * 64 * 64 * 2, dtype=torch.float32, device=DEV)
    a.stats = st.data_ptr()
    with pytest.raises(ValueError, match="bn_stats"):
        _lib.check(lib.ldiff_op_conv(C.byref(a), stream()))
    a.bn_stats = None
    with reached(lib) as names:
        _lib.check(lib.ldiff_op_conv(C.byref(a), stream()))
    assert names and not any(n.startswith("clsconv<") for n in names), names


# ---- 2. bn_finalize -----------------------------------------------------------------------------------------------------------------------------------
def ulps(got, want):
    """|got - want| in units of float32's spacing at |want| (float64 tensors)."""
    sp = torch.from_numpy(np.spacing(np.abs(want.numpy()).astype(np.float32)).astype(np.float64))
    return ((got - want).abs() / sp).max().item()


def run_finalize(lib, part, n, gamma, beta, offset=0, T=None):
    N, R, _ = part.shape
    T = T if T is not None else N
    pd, gd, bd = part.float().contiguous().to(DEV), gamma.float().to(DEV), beta.float().to(DEV)
    scale, shift = (torch.full((N,), float("nan"), dtype=torch.float32, device=DEV) for _ in range(2))
    stats = torch.full((2, T), float("nan"), dtype=torch.float32, device=DEV)
    rc = lib.ldiff_op_bn_finalize(_lib.ptr(pd), R, N, n, _lib.ptr(gd), _lib.ptr(bd), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(stats), offset, T, stream())
    torch.cuda.synchronize()
    return rc, scale.double().cpu(), shift.double().cpu(), stats.double().cpu()


def finalize_reference(part, n, gamma, beta):
    s, q = part.float().double()[..., 0].sum(1), part.float().double()[..., 1].sum(1)
    mean = s / n
    var = (q / n - mean * mean).clamp_min(0.0)
    scale = gamma.float().double() / torch.sqrt(var + 1e-5)
    return mean, var * n / (n - 1), scale, beta.float().double() - mean * scale


@pytest.mark.parametrize("N,R,rows", [(64, 7, 64), (16, 1, 16), (200, 37, 16)])
def test_bn_finalize_against_double(lib, N, R, rows):
    """On given partials (R not a multiple of the loop's unroll, one partial, N not a multiple of the block): mean, unbiased variance and scale within 1 float32
    ulp of the double computation, shift within 2; written at the caller's offset of the flat [2][T] buffer, nothing else touched."""
    g = torch.Generator().manual_seed(N + R)
    n = R * rows - 3
    v = torch.randn((R * rows, N), generator=g, dtype=torch.float64) * (0.5 + torch.rand(N, generator=g, dtype=torch.float64)) + torch.randn(N, generator=g, dtype=torch.float64)
    v[n:] = 0
    part = torch.stack([v.view(R, rows, N).sum(1).t(), (v * v).view(R, rows, N).sum(1).t()], 2)
    gamma, beta = 1.0 + 0.1 * torch.randn(N, generator=g), 0.1 * torch.randn(N, generator=g)
    rc, scale, shift, stats = run_finalize(lib, part, n, gamma, beta, offset=24, T=N + 40)
    assert rc == 0, lib.ldiff_last_error()
    mean, uvar, sc, sh = finalize_reference(part, n, gamma, beta)
    figs = dict(mean=ulps(stats[0, 24:24 + N], mean), var=ulps(stats[1, 24:24 + N], uvar), scale=ulps(scale, sc), shift=ulps(shift, sh))
    print(f"[bn_finalize] N={N} R={R}: ulps {figs}")
    assert figs["mean"] <= 1 and figs["var"] <= 1 and figs["scale"] <= 1 and figs["shift"] <= 2
    assert torch.isnan(stats[:, :24]).all() and torch.isnan(stats[:, 24 + N:]).all()
    assert ulps(stats[1, 24:24 + N], uvar * (n - 1) / n) > 1                         # (the biased variance would miss)


def test_bn_finalize_constant_clamped_and_refused(lib):
    R, rows = 5, 16
    n = R * rows
    part = torch.zeros((16, R, 2), dtype=torch.float64)
    part[0, :, 0], part[0, :, 1] = 1.5 * rows, 2.25 * rows                       # a constant channel: variance exactly 0
    c = float(np.float32(1.1))
    part[1, :, 0] = c * rows                                                      # sumsq rounded to float32 and pushed 8 ulps down: sumsq / n - mean^2 < 0
    q32 = np.float32(c * c * rows)
    part[1, :, 1] = float(q32 - 8 * np.spacing(q32))
    assert (part[1, :, 1].float().double().sum() / n - (part[1, :, 0].float().double().sum() / n) ** 2).item() < 0
    gamma, beta = torch.full((16,), 0.75), torch.full((16,), 0.25)
    rc, scale, shift, stats = run_finalize(lib, part, n, gamma, beta)
    assert rc == 0
    assert stats[1, 0].item() == 0.0 and stats[1, 1].item() == 0.0 and stats[0, 0].item() == 1.5
    want = torch.tensor([0.75 / np.sqrt(1e-5)] * 2, dtype=torch.float64)
    assert ulps(scale[:2], want) <= 1 and torch.isfinite(scale).all() and torch.isfinite(shift).all() and torch.isfinite(stats).all()
    rc, scale, shift, stats = run_finalize(lib, part[:, :1], 1, gamma, beta)      # n = 1: refused on the host, nothing launched
    assert rc == -1 and b"more than 1 value per channel" in lib.ldiff_last_error()
    assert torch.isnan(scale).all() and torch.isnan(stats).all()


# ---- 3. bn_apply --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [16, 2048])
@pytest.mark.parametrize("mode", ["none", "plain", "bn"])
def test_bn_apply_against_float64(lib, N, mode):
    """The three identity forms, with and without the ReLU, M = 37 (at N = 16 the 74 threads fill no 256-thread block; at N = 2048 a row is one block): every element within
    2^-11 |y| + 4 2^-24 (|x s| + |t| + |r s2| + |t2|); the same bound rejects a dropped identity and a dropped ReLU."""
    M = 37
    g = torch.Generator().manual_seed(N + len(mode))
    x = (torch.randn((M, N), generator=g) * 3).to(torch.float16)
    r = (torch.randn((M, N), generator=g) * 2).to(torch.float16)
    s, t, s2, t2 = (torch.randn(N, generator=g) for _ in range(4))
    xd, rd, sd_, td, s2d, t2d = (v.to(DEV) for v in (x, r, s, t, s2, t2))
    for relu in (0, 1):
        y = torch.full((M, N), float("nan"), dtype=torch.float16, device=DEV)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        idp = _lib.ptr(rd) if mode != "none" else None
        _lib.check(lib.ldiff_op_bn_apply(_lib.ptr(xd), M, N, _lib.ptr(sd_), _lib.ptr(td), idp, _lib.ptr(s2d) if mode == "bn" else None, _lib.ptr(t2d) if mode == "bn" else None,
                                         relu, _lib.ptr(y), _lib.ptr(flag), stream()))
        torch.cuda.synchronize()
        main = x.double() * s.double() + t.double()
        mag = (x.double() * s.double()).abs() + t.double().abs()
        idv = torch.zeros_like(main)
        if mode == "plain":
            idv, mag = r.double(), mag + r.double().abs()
        elif mode == "bn":
            idv, mag = r.double() * s2.double() + t2.double(), mag + (r.double() * s2.double()).abs() + t2.double().abs()
        pre = main + idv
        want = F.relu(pre) if relu else pre
        tol = U16 * want.abs() + 4 * U * mag
        got = y.double().cpu()
        assert ((got - want).abs() <= tol).all(), f"N={N} {mode} relu={relu}: worst {((got - want).abs() / tol).max().item():.3f} of the bound"
        assert int(flag.item()) == 0
        if mode != "none":
            assert ((got - (F.relu(main) if relu else main)).abs() > tol).float().mean().item() > 0.3
        if relu:
            assert ((got - pre).abs() > tol).float().mean().item() > 0.3


def test_bn_apply_flags_an_overflow_the_relu_would_hide(lib):
    M, N = 5, 16
    x = torch.ones((M, N), dtype=torch.float16)
    x[3, 9] = -60000.0
    s, t = torch.full((N,), 2.0), torch.zeros(N)       # -120000: beyond fp16's range, in front of a ReLU that turns it into 0
    xd, sd_, td = x.to(DEV), s.to(DEV), t.to(DEV)
    y = torch.empty((M, N), dtype=torch.float16, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.check(lib.ldiff_op_bn_apply(_lib.ptr(xd), M, N, _lib.ptr(sd_), _lib.ptr(td), None, None, None, 1, _lib.ptr(y), _lib.ptr(flag), stream()))
    torch.cuda.synchronize()
    assert int(flag.item()) == 1 and y[3, 9].item() == 0.0 and torch.isfinite(y).all()
    with pytest.raises(ValueError, match="multiple of 8"):
        _lib.check(lib.ldiff_op_bn_apply(_lib.ptr(xd), M, 12, _lib.ptr(sd_), _lib.ptr(td), None, None, None, 1, _lib.ptr(y), None, stream()))


def test_cls_head_feat_keeps_the_heads_bits(lib):
    B, HW, A, NCLS = 5, 4, 256, 6
    g = torch.Generator().manual_seed(9)
    x = torch.randn((B, HW, A), generator=g).to(torch.float16).to(DEV)
    w, bias = (torch.randn((NCLS, A), generator=g) / 16).to(DEV), (torch.randn(NCLS, generator=g) * 0.2).to(DEV)
    lo = [torch.full((B, NCLS), float("nan"), dtype=torch.float32, device=DEV) for _ in range(2)]
    la = [torch.full((B,), -1, dtype=torch.int32, device=DEV) for _ in range(2)]
    feat = torch.full((B, A), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(lib.ldiff_op_cls_head(_lib.ptr(x), B, HW, A, A, _lib.ptr(w), _lib.ptr(bias), NCLS, _lib.ptr(lo[0]), _lib.ptr(la[0]), stream()))
    _lib.check(lib.ldiff_op_cls_head_feat(_lib.ptr(x), B, HW, A, A, _lib.ptr(w), _lib.ptr(bias), NCLS, _lib.ptr(lo[1]), _lib.ptr(la[1]), _lib.ptr(feat), stream()))
    torch.cuda.synchronize()
    assert torch.equal(lo[0], lo[1]) and torch.equal(la[0], la[1])
    want = x.double().mean(1)
    assert ((feat.double() - want).abs() <= 8 * U * x.double().abs().mean(1)).all()      # HW = 4 fp32 additions and the division
    feat2 = torch.empty_like(feat)
    _lib.check(lib.ldiff_op_cls_head_feat(_lib.ptr(x), B, HW, A, A, _lib.ptr(w), _lib.ptr(bias), NCLS, None, None, _lib.ptr(feat2), stream()))   # logits / labels may be NULL
    assert torch.equal(feat2, feat)


# ---- 4. the network in training mode ------------------------------------------------------------------------------------------------------------------
REDUCED = dict(layers=(1, 1, 2, 1), width=16, adapter=32, S=64)       # layer 4's map is 2 x 2 at S = 64: B = 1 is legal
FULL = dict(layers=(3, 8, 36, 3), width=64, adapter=256, S=64)        # ResNet152
NC = 4
TRAIN_CASES = [("reduced", 1, 31), ("reduced", 6, 32), ("full", 12, 33)]
# Measured on the MI355X, per case: max |lib - f64| / max |fp16-storage model - f64| of (the features, the batch means, the unbiased batch variances); the statistics'
# errors are taken per BatchNorm relative to the layer's largest float64 value, then the worst layer.  The asserted factor is twice the measured one.  As in
# test_gpu_cellhead.py: a measured ratio above 2 would be a lost fp32 sum to be found, not a number to record.
MEASURED = {("reduced", 1, 31): (0.893, 1.135, 1.041), ("reduced", 6, 32): (0.948, 0.926, 0.876), ("full", 12, 33): (0.973, 1.068, 1.064)}


def spec_of(name):
    return REDUCED if name == "reduced" else FULL


def layer_error(got, ref, layout):
    return max(((got[o:o + c] - ref[o:o + c]).abs().max() / ref[o:o + c].abs().max()).item() for _, o, c in layout)


@functools.lru_cache(maxsize=None)
def train_case(name, B, seed):
    spec = spec_of(name)
    sd = resnet_ref.synthetic_state_dict(spec["layers"], spec["width"], NC, seed, 0.25, spec["adapter"])
    x = torch.randn((B, 3, spec["S"], spec["S"]), generator=torch.Generator().manual_seed(seed + 100)).to(torch.float16).float()
    ref = tref.forward_train(sd, spec["layers"], x, torch.float64)
    model = tref.forward_train(sd, spec["layers"], x, torch.float64, store=resnet_ref.fp16_storage)
    net = ResNetClassifier(NC, sd, DEV, spec["layers"], spec["width"], spec["adapter"], train=True)
    crops = resnet_ref.to_nhwc8(x).to(DEV)
    feats, mean, var, logits, labels = net.forward_train(crops, want_logits=True)
    net.check_finite()
    return dict(sd=sd, x=x, crops=crops, ref=ref, model=model, net=net, feats=feats.double().cpu(), mean=mean.double().cpu(), var=var.double().cpu(), logits=logits.double().cpu(),
                labels=labels.long().cpu(), raw=(feats, mean, var))


@pytest.mark.parametrize("name,B,seed", TRAIN_CASES)
def test_forward_train_against_float64(name, B, seed):
    """Features and every BatchNorm's batch mean / unbiased variance against the float64 restatement.  Yardstick: the same restatement with the weights and every
    stored tensor rounded to fp16.  The library rounds twice per conv (the raw and the applied tensor) and takes the statistics from the fp32 accumulators; the model
    rounds at least as often and takes them from the rounded tensor."""
    c = train_case(name, B, seed)
    spec = spec_of(name)
    layout, T = tref.bn_layout(spec["layers"], spec["width"])
    assert c["net"].bn_layout == layout and c["net"].bn_channels == T and c["mean"].shape == (T,)
    assert torch.isfinite(c["feats"]).all() and torch.isfinite(c["mean"]).all() and torch.isfinite(c["var"]).all() and (c["var"] >= 0).all()
    ref, model = c["ref"], c["model"]
    e_lib = ((c["feats"] - ref["features"]).abs().max().item(), layer_error(c["mean"], ref["mean"], layout), layer_error(c["var"], ref["var"], layout))
    e_model = ((model["features"] - ref["features"]).abs().max().item(), layer_error(model["mean"], ref["mean"], layout), layer_error(model["var"], ref["var"], layout))
    ratios = tuple(a / b for a, b in zip(e_lib, e_model))
    print(f"[forward_train] {name} B={B}: lib {tuple(f'{v:.3e}' for v in e_lib)}, fp16-storage model {tuple(f'{v:.3e}' for v in e_model)}, ratios {tuple(f'{v:.3f}' for v in ratios)}")
    assert (c["logits"] - (c["feats"] @ c["sd"]["classifier.weight"].double().t() + c["sd"]["classifier.bias"].double())).abs().max().item() <= 1e-4
    assert MEASURED[(name, B, seed)] is not None, "no measured ratio recorded for this case"
    for what, r, m in zip(("features", "batch mean", "batch variance"), ratios, MEASURED[(name, B, seed)]):
        assert r <= 2.0 * m, f"{name} B={B}: the {what}' error is {r:.3f} x the fp16-storage model's (asserted: twice the recorded {m:.3f})"


def test_forward_train_is_reproducible_and_eval_is_unchanged():
    """forward_train twice: bit-equal outputs.  A train-enabled handle's eval-mode logits: bit-equal to a plain handle's."""
    c = train_case("reduced", 6, 32)
    feats, mean, var = c["net"].forward_train(c["crops"])
    assert torch.equal(feats, c["raw"][0]) and torch.equal(mean, c["raw"][1]) and torch.equal(var, c["raw"][2])
    plain = ResNetClassifier(NC, c["sd"], DEV, REDUCED["layers"], REDUCED["width"], REDUCED["adapter"])
    for _ in range(3):   # eager, captured, replayed
        lo_t, la_t = c["net"](c["crops"])
        lo_p, la_p = plain(c["crops"])
        assert torch.equal(lo_t, lo_p) and torch.equal(la_t, la_p)
    plain.check_finite()
    c["net"].check_finite()


def test_forward_train_refusals():
    c = train_case("reduced", 6, 32)
    small = torch.zeros((1, 32, 32, 8), dtype=torch.float16, device=DEV)
    with pytest.raises(ValueError, match=r"more than 1 value per channel.*encoder\.7\.0\.bn2"):      # S = 32, B = 1: layer 4's map is 1 x 1
        c["net"].forward_train(small)
    c["net"].forward_train(torch.zeros((2, 32, 32, 8), dtype=torch.float16, device=DEV))            # B = 2 is legal there
    plain = ResNetClassifier(NC, c["sd"], DEV, REDUCED["layers"], REDUCED["width"], REDUCED["adapter"])
    assert plain.bn_layout == c["net"].bn_layout
    with pytest.raises(RuntimeError, match="set_train"):
        plain.forward_train(c["crops"])
    with pytest.raises(RuntimeError, match="before the load"):
        plain.set_train(True)


# ---- 5. end to end: Segmentor.train_cell_model ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    from ldiffusion_amd import configs, weights
    from ldiffusion_amd.models import AutoencoderKL, UNet2DConditionModel
    ucfg, vcfg = configs.TINY_UNET, configs.TINY_VAE
    usd = weights.synthetic_state_dict(weights.unet_param_shapes(ucfg), 42, fp16_values=True)
    vsd = weights.synthetic_state_dict(weights.vae_param_shapes(vcfg), 43, fp16_values=True)
    return dict(unet=UNet2DConditionModel(ucfg, usd, DEV), vae=AutoencoderKL(vcfg, vsd, DEV))


E2E_SEED = 51     # the classifier's seed, chosen on the CPU so that the float64 restatement's own loop (resnet_train_ref.train_loop, lr 1e-2) falls by more than 0.02 per epoch
# Measured on the MI355X for the end-to-end case: max |lib - f64| over the logits of the first image's instances in front of any update.  The run's own error is asserted
# against twice this figure, and so is the first cross-entropy against the restatement's (a logit error e moves a cross-entropy by at most 2 e).
E2E_MEASURED_LOGIT_ERROR = 1.777e-03


@pytest.fixture(scope="module")
def e2e(tiny, tmp_path_factory):
    """Folders of the tiny UNet / VAE, the loaders (2 training images, the second with an EMPTY label map, 1 validation image), the label maps and class masks."""
    tmp = tmp_path_factory.mktemp("celltrain")
    sd_dir, w_dir = tmp / "sd", tmp / "train_save" / "unet" / "25_01_01"
    tiny["unet"].save_pretrained(str(sd_dir / "unet"))
    tiny["vae"].save_pretrained(str(sd_dir / "vae"))
    tiny["unet"].save_pretrained(str(w_dir))
    labels = synthetic_label_map()
    ids = np.unique(labels)
    rng = np.random.default_rng(7)
    paint = np.zeros(int(labels.max()) + 1, np.int64)
    paint[ids[ids != 0]] = rng.integers(1, NC, size=int((ids != 0).sum()))
    mask = torch.from_numpy(paint[labels])
    g = torch.Generator().manual_seed(8)
    imgs = [torch.rand((1, 3, 64, 64), generator=g) for _ in range(3)]
    train = [(imgs[0], mask[None], 0), (imgs[1], mask[None], 0)]
    val = [(imgs[2], mask[None], 0)]
    ctx = (torch.randn((1, 6, 64), generator=torch.Generator().manual_seed(2)) * 0.5).to(DEV)
    seen = []

    def instances(image):
        """The first training image and the validation image carry the synthetic label map, the other training image none: told apart by the image itself."""
        assert image.dtype == np.float32 and image.shape == (1024, 1024, 3) and 0.0 <= image.min() and image.max() <= 1.0
        key = image.tobytes()[:4096]
        if key not in [k for k, _ in seen]:
            seen.append((key, image))
        return labels if [k for k, _ in seen].index(key) != 1 else np.zeros_like(labels)

    sd = resnet_ref.synthetic_state_dict(REDUCED["layers"], REDUCED["width"], NC, E2E_SEED, 0.25, REDUCED["adapter"])
    return dict(tmp=tmp, sd_dir=str(sd_dir), w_dir=str(w_dir), train=train, val=val, ctx=ctx, instances=instances, labels=labels, mask=mask, sd=sd, seen=seen)


def run_trainer(e2e, save_root, **kw):
    from ldiffusion_amd.segmentor import Segmentor
    seg = Segmentor(e2e["train"], e2e["val"], "cell", NC)
    folder = seg.train_cell_model(kw.pop("epochs"), e2e["w_dir"], e2e["sd_dir"], cell_weights=e2e["sd"], instances=e2e["instances"], save_root=str(save_root), seed=0,
                                  text_embeddings=e2e["ctx"], **kw)
    return seg, folder


def reference_inputs(e2e):
    """After a trainer run: the crops the library cuts from the image the label-map callable saw first (fp16-exact, as float64), the instances' targets, and the float64
    restatement / fp16-storage model of one training-mode forward over them."""
    if "ref_inputs" not in e2e:
        image = e2e["seen"][0][1]
        rgb = torch.from_numpy(np.rint(image.astype(np.float64) * 255.0).astype(np.uint8)).to(DEV)
        head = cellhead.CellSegClassifier(NC, e2e["sd"], DEV, input_norm=False, train=True)
        ids, boxes = cellhead.instance_boxes(torch.from_numpy(e2e["labels"]).to(DEV))
        assert 25 <= ids.numel() <= 40
        lib_crops = head.crops(rgb, boxes)
        crops = lib_crops[..., :3].permute(0, 3, 1, 2).double().cpu()
        lib_logits = head.net.forward_train(lib_crops, want_logits=True)[3].double().cpu()
        e2e["ref_inputs"] = dict(crops=crops, targets=cellhead.instance_targets(torch.from_numpy(e2e["labels"]), e2e["mask"], NC), lib_logits=lib_logits,
                                 ref=tref.forward_train(e2e["sd"], REDUCED["layers"], crops, torch.float64),
                                 model=tref.forward_train(e2e["sd"], REDUCED["layers"], crops, torch.float64, store=resnet_ref.fp16_storage))
    return e2e["ref_inputs"]


def test_train_cell_model_without_fit_changes_only_the_running_statistics(e2e):
    """fit_classifier=False, 2 epochs -- exactly what the reference's loop changes: every tensor but running_mean / running_var / num_batches_tracked is bit-equal
    to cell_weights, num_batches_tracked = 2 (the image with the empty label map is not counted), and the running statistics agree with the float64 restatement's
    EMA over the same crops under the network test's recorded ratio."""
    seg, folder = run_trainer(e2e, e2e["tmp"] / "nofit", epochs=2, fit_classifier=False)
    assert folder is not None and os.path.isfile(os.path.join(folder, "cellclassifier.pth"))
    out = cellhead.read_cellclassifier(folder)
    assert cellhead.check_state_dict(out, NC, REDUCED["layers"], REDUCED["width"], REDUCED["adapter"])
    layout, T = tref.bn_layout(REDUCED["layers"], REDUCED["width"])
    for k, v in e2e["sd"].items():
        if not k.endswith(("running_mean", "running_var")):
            assert out[k].dtype == torch.float32 and torch.equal(out[k], v), k
    for p, _, _ in layout:
        assert out[p + ".num_batches_tracked"].dtype == torch.int64 and int(out[p + ".num_batches_tracked"]) == 2
    assert seg.cell_training_log["loss"] == [0.0, 0.0]
    # the float64 restatement on the crops the library cuts from the image the callable saw
    r = reference_inputs(e2e)
    want, _, _ = tref.train_loop(e2e["sd"], REDUCED["layers"], [(r["crops"], r["targets"]), (None, None)], False, 2, 1e-2)
    m = MEASURED[("reduced", 6, 32)]
    assert m is not None, "no measured ratio recorded"
    for name, key, factor in (("running_mean", "mean", m[1]), ("running_var", "var", m[2])):
        # two steps with the same batch statistics b: running = 0.81 r0 + 0.19 b.  The b the written statistics imply is compared as the network test compares the
        # batch statistics (worst layer, relative to the layer's largest value), plus the float32 roundings of the two updates carried back through 1 / 0.19
        worst_run, worst_model = 0.0, 0.0
        for p, o, c in layout:
            r0, ref_b = e2e["sd"][f"{p}.{name}"].double(), r["ref"][key][o:o + c]
            implied = (out[f"{p}.{name}"].double() - 0.81 * r0) / 0.19
            slack = 4 * U / 0.19 * max(r0.abs().max().item(), ref_b.abs().max().item())
            worst_run = max(worst_run, (((implied - ref_b).abs().max().item() - slack) / ref_b.abs().max().item()))
            worst_model = max(worst_model, ((r["model"][key][o:o + c] - ref_b).abs().max() / ref_b.abs().max()).item())
            assert (out[f"{p}.{name}"].double() - want[f"{p}.{name}"].double()).abs().max().item() <= 1e-2 * max(1.0, want[f"{p}.{name}"].abs().max().item()), (p, name)
        print(f"[train_cell_model] {name}: implied batch statistics {worst_run:.3e} against the fp16-storage model's {worst_model:.3e}")
        assert worst_run <= 2.0 * factor * worst_model, (name, worst_run, worst_model, factor)


def test_train_cell_model_fits_the_classifier(e2e):
    """fit_classifier=True, lr 1e-2, 3 epochs: the epoch-mean cross-entropy falls in every epoch (as the float64 restatement's own loop does, by a clear margin: the
    seed was chosen for that on the CPU); the first image's cross-entropy in front of any update equals the restatement's; cache_features on and off write
    bit-identical tensors; the folder serves inference_cell_model."""
    from PIL import Image
    seg, folder = run_trainer(e2e, e2e["tmp"] / "fit", epochs=3, fit_classifier=True, lr=1e-2)
    seg2, folder2 = run_trainer(e2e, e2e["tmp"] / "fit_nocache", epochs=3, fit_classifier=True, lr=1e-2, cache_features=False)
    assert folder is not None and folder2 is not None and folder != folder2
    a, b = cellhead.read_cellclassifier(folder), cellhead.read_cellclassifier(folder2)
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a)
    assert seg.cell_training_log["loss"] == seg2.cell_training_log["loss"]
    loss = seg.cell_training_log["loss"]
    print(f"[train_cell_model] epoch losses {loss}, validation dice {seg.cell_training_log['dice']}")
    assert loss[0] > loss[1] > loss[2] > 0
    r = reference_inputs(e2e)
    _, ref_means, ref_first = tref.train_loop(e2e["sd"], REDUCED["layers"], [(r["crops"], r["targets"]), (None, None)], True, 3, 1e-2)
    assert ref_means[1] < ref_means[0] - 0.02 and ref_means[2] < ref_means[1] - 0.02, ref_means      # the clear margin: several times the cross-entropy error 2 e below
    e_run = (r["lib_logits"] - r["ref"]["logits"]).abs().max().item()
    print(f"[train_cell_model] first image: max |lib - f64| over the logits {e_run:.3e}; cross-entropy {seg.cell_training_log['first_loss']:.6f} against float64's {ref_first:.6f}; "
          f"float64 epoch means {ref_means}")
    assert E2E_MEASURED_LOGIT_ERROR is not None, "no measured logit error recorded"
    assert e_run <= 2 * E2E_MEASURED_LOGIT_ERROR
    assert abs(seg.cell_training_log["first_loss"] - ref_first) <= 2 * E2E_MEASURED_LOGIT_ERROR
    # the folder is what inference_cell_model takes
    img = (np.random.default_rng(5).random((96, 80, 3)) * 255).astype(np.uint8)
    path = e2e["tmp"] / "roi.png"
    Image.fromarray(img).save(path)
    decoded, mask = seg.inference_cell_model(str(path), e2e["sd_dir"], e2e["w_dir"], folder, text_embeddings=e2e["ctx"], instances=lambda image: e2e["labels"])
    assert mask.shape == (96, 80) and mask.dtype == np.uint8 and (mask > 0).any() and int(mask.max()) < NC


def test_train_cell_model_returns_none_when_validation_never_beats_zero(e2e, monkeypatch):
    from ldiffusion_amd.segmentor import Segmentor
    monkeypatch.setattr(Segmentor, "micro_dice", lambda self, predicted_labels, true_labels, num_classes=7: (torch.zeros(num_classes), torch.tensor(0.0)))
    root = e2e["tmp"] / "never"
    seg, folder = run_trainer(e2e, root, epochs=1, fit_classifier=False)
    assert folder is None and not os.path.exists(root)
