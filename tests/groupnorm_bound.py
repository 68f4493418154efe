"""Float64 references, derived error bounds, wrong references and fp32 emulations for the inference-time GroupNorm path
(csrc/kernels_norm.hip: gn_small_kernel, gn_partial_kernel + gn_finalize_kernel, gn_finalize2_kernel, fold_gn_weights_kernel; the statistics
the conv / GEMM epilogues emit; the per-image weights of gemm_dma).  Imports without a GPU; tests/test_cpu_groupnorm_bound.py judges every
bound here on the CPU, tests/test_gpu_groupnorm.py applies them to the kernels.

u = 2^-24, gamma(n) = 2 n u (as in test_gpu_backward.py).

1. Statistics -> scale / shift.  Both forms sum x and x^2 in fp32 chains, combine the chains in float64 and finalize in float64:
       mean = S1 / n,  var = max(S2 / n - mean^2, 0),  rstd = fp32(1 / sqrt(var + eps)),  scale = gamma rstd,  shift = beta - fp32(mean) scale.
   An error of k u in S2 (relative) is k u E[x^2] in var, i.e. k u amp relative to var + eps with amp = E[x^2] / (var + eps) >= 1, and half
   of that in rstd; an error of k u sum|x| in S1 is at most k u rms in mean (rms = sqrt(E[x^2]) >= E|x|).  So
       tol_scale = |scale| (4 u + c u amp)
       tol_shift = tol_scale |mean| + |scale| c u rms + 4 u (|shift| + |beta|)
   (the form of test_gpu_nnunet.py's InstanceNorm finalize test, plus the term for the error of the mean, which that test's float64-made
   partial sums do not have).  4 u: the roundings of rstd, gamma rstd, fp32(mean), the product and the subtraction.
   The worst-case gamma(L) over the longest chain (L = 1,408 in gn_small_kernel at HW = 4096, Cg = 80) is ~10^4 times the error such a chain
   really has and rejects nothing, so c is MEASURED: emulate_small / emulate_partial repeat each kernel's own summation order in fp32
   (per-thread sequential chains, the four-pixel unroll, the LDS combine, then float64), and
       C_STATS = 4 x the worst (error - the 4 u terms) / (u amp |scale|) resp. / (u |scale| (amp |mean| + rms)) of the emulation over 20 seeds
                 of every case of STATS_CASES (stats_c_ratio), at least the project's existing 2.
   The factor 4 is for what the emulation cannot copy from the compiler: FMA contraction and the association inside the unrolled loops.
   Measured (python tests/groupnorm_bound.py, 20 seeds): worst ratio 5.72, C_STATS = 23 (see the constant below).

2. Fused statistics.  Level 1, per (image, channel): the R partials added in float64 against the float64 sum / sum of squares of the fp16
   output the kernel stored: |d sum| <= gamma(L_b) sum|y|, |d sumsq| <= (gamma(L_b) + 2u) sum y^2, L_b = the number of values one partial
   accumulates in fp32 (uniform per kernel, so the per-block bounds add up to one expression over the image).  Level 2: section 1's bound
   behind ldiff_op_gn_finalize.

3. GroupNorm folded into a 1x1 conv: y = (W diag(s_b)) x + (bias + W t_b), the folded weights rounded to fp16.  Per output element
       tol = sum_c (2^-11 |W s| + 2^-25) |x|                   fp16 rounding of the folded weight, and its subnormal floor
           + 2u sum_c |W s x|                                   the fp32 product in the fold (before the fp16 rounding)
           + gamma(K) sum_c |W s x|                             the GEMM's fp32 accumulation
           + gamma(K / 64 + 6) sum_c |W t| + u |bias|           the folded bias: 64 lanes of sequential chains of K / 64 terms (8 per trip of the
                                                                channel loop, ceil(K / 512) trips), then six shuffle steps
           + 2^-11 |ref| + 2^-24                                the output's own rounding.
   The unfolded route (igemm<...,gn>) rounds the normalised operand a = fp16(x s + t) instead:
       tol = sum_c ((2^-11 + 2u) |a| + 2^-25) |W| + gamma(K) sum_c |a W| + u |bias| + 2^-11 |ref| + 2^-24.
"""
import math
from collections import namedtuple

import torch

U = 2.0 ** -24
H16 = 2.0 ** -11

# 4 x the emulation's worst stats_c_ratio over 20 seeds of every STATS_CASES entry, rounded up.  Measured (python tests/groupnorm_bound.py):
# worst 5.719, in small_c2560_hw4096 (the 1,408-term chains); next small_ratio30 0.688, small_ratio8 0.589, two_ratio30 0.499, two_ratio8 0.339,
# small_hw1 0.190; every other case <= 0.05 (the 4 u terms cover it).  4 x 5.719 = 22.9.
C_STATS = 23.0
C_STATS_WORST_EMULATION = 5.719


def gamma(n):
    return 2.0 * n * U


def f32eps(eps):
    """The eps the kernels see: a C float, widened to double in the finalize."""
    return float(torch.tensor(eps, dtype=torch.float32).double())


# ======================================================================================================================
# 1. statistics
# ======================================================================================================================
StatsCase = namedtuple("StatsCase", "form B C1 C2 HW groups eps ratio split pitch special affine", defaults=(1e-5, 0.2, False, 0, None, False))
ONE, TWO = "gn_stats<1>", "gn_stats<2>"
STATS_CASES = {
    # one-launch form (gn_small_kernel)
    "small_c640_cg20_hw1024": StatsCase(ONE, 4, 640, 0, 1024, 32),                 # Cg = 20 cuts 16-byte chunks
    "small_concat_1280_640_hw256": StatsCase(ONE, 8, 1280, 640, 256, 32),          # Cg = 60: a group straddles the concat
    "small_c2560_hw4096": StatsCase(ONE, 1, 1280, 1280, 4096, 32),                 # the longest chain (1,408 terms), through the small-batch clause
    "small_hw1": StatsCase(ONE, 2, 64, 0, 1, 32),
    "small_c32_cg1": StatsCase(ONE, 2, 32, 0, 1024, 32),
    "small_split": StatsCase(ONE, 4, 640, 0, 1024, 32, split=True),
    "small_pitched": StatsCase(ONE, 4, 640, 0, 1024, 32, pitch=704),
    "small_eps6_affine": StatsCase(ONE, 4, 640, 0, 1024, 32, eps=1e-6, affine=True),
    "small_ratio8": StatsCase(ONE, 4, 640, 0, 1024, 32, ratio=8.0),
    # |mean| / std = 30 (amp ~ 900): the bound still rejects a lost pixel only where a pixel is 1 / 64 of the group.  At HW = 1024 / 2048 (either form)
    # it accepts that wrong reference (0.48 / 0.72 of the bound), so neither form has a ratio-30 case on its base shape
    "small_ratio30_hw64": StatsCase(ONE, 4, 640, 0, 64, 32, ratio=30.0),
    "small_const_group": StatsCase(ONE, 4, 640, 0, 1024, 32, special="const"),
    "small_var_eps": StatsCase(ONE, 4, 640, 0, 1024, 32, special="vareps"),
    # two-launch form (gn_partial_kernel + gn_finalize_kernel)
    "two_c128_hw2048": StatsCase(TWO, 8, 128, 0, 2048, 32),
    "two_c320_hw4160": StatsCase(TWO, 2, 320, 0, 4160, 32),                        # R = 6 pixel rows over 32-pixel chunks: one unrolled trip + the scalar tail
    "two_c320_hw4150_ragged": StatsCase(TWO, 2, 320, 0, 4150, 32),                 # the last chunk holds 22 pixels
    "two_concat_128_64_hw2048": StatsCase(TWO, 8, 128, 64, 2048, 32),              # two sources (blockIdx.z), Cg = 6 straddles
    "two_c64_hw33000_pix64": StatsCase(TWO, 1, 64, 0, 33000, 32),                  # HW / 32 > 1024: gn_chunks doubles pix to 64; ragged last chunk
    "two_split": StatsCase(TWO, 8, 128, 0, 2048, 32, split=True),
    "two_pitched": StatsCase(TWO, 8, 128, 0, 2048, 32, pitch=160),
    "two_eps6_affine": StatsCase(TWO, 8, 128, 0, 2048, 32, eps=1e-6, affine=True),
    "two_ratio8": StatsCase(TWO, 8, 128, 0, 2048, 32, ratio=8.0),
    "two_const_group": StatsCase(TWO, 8, 128, 0, 2048, 32, special="const"),
    "two_var_eps": StatsCase(TWO, 8, 128, 0, 2048, 32, special="vareps"),
}
CONST_VALUE = 1.5   # every fp32 partial sum of 1.5 and of 2.25 is exact, so a constant group has var = 0 exactly


def expected_form(case):
    """The predicate of launch_gn_stats (csrc/kernels_norm.hip), restated: which form the library takes for the case's shape."""
    return ONE if (case.HW <= 1024 and case.B * case.groups >= 64) or (case.B * case.groups < 256 and case.HW <= 4096) else TWO


def make_stats_input(case, seed):
    """-> dict(hi, lo [B, HW, C] fp16 (lo None unless split), gamma, beta [C] fp32, v [B, HW, C] float64 = the values the kernel sees).
    Channel means are spread by half a standard deviation, so that a group boundary off by one channel moves the statistics."""
    g = torch.Generator().manual_seed(seed)
    C = case.C1 + case.C2
    std = math.sqrt(case.eps) if case.special == "vareps" else 1.7
    off = case.ratio + (torch.rand((1, 1, C), generator=g, dtype=torch.float64) - 0.5)
    x = std * (torch.randn((case.B, case.HW, C), generator=g, dtype=torch.float32).double() + off)
    if case.special == "const":
        x[:, :, :C // case.groups] = CONST_VALUE
    hi = x.to(torch.float16)
    lo = (x - hi.double()).to(torch.float16) if case.split else None
    if case.affine:
        gam, bet = 1 + 0.3 * torch.randn(C, generator=g), 0.5 * torch.randn(C, generator=g)
    else:
        gam, bet = torch.ones(C), torch.zeros(C)
    v = hi.double() + (lo.double() if lo is not None else 0.0)
    return dict(hi=hi, lo=lo, gamma=gam, beta=bet, v=v)


StatsRef = namedtuple("StatsRef", "scale shift mean var ex2 beta eps")


def stats_reference(v, groups, eps, gam, bet, shift_channels=0, drop_last=False):
    """float64 scale / shift [B, C] of v [B, HW, C].  shift_channels = 1: every group takes the channels one further (the wrong reference
    'group boundary off by one'); drop_last: the last pixel left out."""
    B, HW, C = v.shape
    if shift_channels:
        v = torch.roll(v, -shift_channels, dims=2)
    if drop_last:
        v = v[:, :-1]
    Cg = C // groups
    vg = v.reshape(B, v.shape[1], groups, Cg)
    mean = vg.mean((1, 3))
    ex2 = (vg * vg).mean((1, 3))
    var = ((vg - mean[:, None, :, None]) ** 2).mean((1, 3))
    e = f32eps(eps)
    ex = lambda t: t.repeat_interleave(Cg, dim=1)
    sc = gam.double()[None] * ex(1.0 / torch.sqrt(var + e))
    sh = bet.double()[None] - ex(mean) * sc
    return StatsRef(sc, sh, ex(mean), ex(var), ex(ex2), bet.double()[None], e)


def stats_tol(ref, c=None):
    c = C_STATS if c is None else c
    amp = (ref.ex2 / (ref.var + ref.eps)).clamp_min(1.0)
    tol_sc = ref.scale.abs() * (4 * U + c * U * amp)
    tol_sh = tol_sc * ref.mean.abs() + ref.scale.abs() * c * U * ref.ex2.sqrt() + 4 * U * (ref.shift.abs() + ref.beta.abs())
    return tol_sc, tol_sh


def stats_ratio(scale, shift, ref, c=None):
    """max over every (image, channel) of |error| / bound, scale and shift together (<= 1: accepted)."""
    tol_sc, tol_sh = stats_tol(ref, c)
    tiny = 1e-300
    return max(((scale.double() - ref.scale).abs() / (tol_sc + tiny)).max().item(), ((shift.double() - ref.shift).abs() / (tol_sh + tiny)).max().item())


def stats_c_ratio(scale, shift, ref):
    """The quantity C_STATS is 4 x the maximum of: what the error exceeds the bound's 4 u terms by, over the quantity c multiplies --
    (|d scale| - 4 u |scale|) / (u amp |scale|) and (|d shift| - 4 u (|shift| + |beta|)) / (u |scale| (amp |mean| + rms)).  (Without the
    subtraction a channel whose gamma is near zero divides the rounding of beta by nothing.)"""
    amp = (ref.ex2 / (ref.var + ref.eps)).clamp_min(1.0)
    d_sc = ((scale.double() - ref.scale).abs() - 4 * U * ref.scale.abs()).clamp_min(0.0) / (U * amp * ref.scale.abs() + 1e-300)
    d_sh = ((shift.double() - ref.shift).abs() - 4 * U * (ref.shift.abs() + ref.beta.abs())).clamp_min(0.0)
    d_sh = d_sh / (U * ref.scale.abs() * (amp * ref.mean.abs() + ref.ex2.sqrt()) + 1e-300)
    return max(d_sc.max().item(), d_sh.max().item())


def stats_wrong_references(inp, case):
    """[(name, StatsRef)] the case's bound must reject: group boundary off by one channel, last pixel left out (where there is more than one
    pixel), and float64 at 2 eps where some group's variance is within 10 x of eps."""
    right = stats_reference(inp["v"], case.groups, case.eps, inp["gamma"], inp["beta"])
    out = [("group off by one channel", stats_reference(inp["v"], case.groups, case.eps, inp["gamma"], inp["beta"], shift_channels=1))]
    if case.HW > 1:
        out.append(("last pixel left out", stats_reference(inp["v"], case.groups, case.eps, inp["gamma"], inp["beta"], drop_last=True)))
    if (right.var <= 10 * right.eps).any():
        out.append(("eps doubled", stats_reference(inp["v"], case.groups, 2 * case.eps, inp["gamma"], inp["beta"])))
    return out


def _seen32(inp, case):
    """The fp32 values load8 produces: fp32(hi) + fp32(lo)."""
    x = inp["hi"].float()
    return x + inp["lo"].float() if inp["lo"] is not None else x


def emulate_small(x, C1, groups):
    """gn_small_kernel's sums in its own order: thread t of 256 takes the items t, t + 256, ... (item = (pixel, 16-byte chunk overlapping the
    group)), eight channels each in sequence (channels outside the group add 0), one fp32 chain per thread; threads combine in float64.
    x [B, HW, C] fp32 -> (S1, S2) float64 [B, groups].  (C1 % 8 == 0: a chunk never straddles the sources, so the concat is one channel space.)"""
    B, HW, C = x.shape
    Cg = C // groups
    S1, S2 = torch.zeros((B, groups), dtype=torch.float64), torch.zeros((B, groups), dtype=torch.float64)
    for grp in range(groups):
        c0, c1 = grp * Cg, grp * Cg + Cg
        k0, k1 = c0 >> 3, (c1 + 7) >> 3
        sub = x[:, :, k0 * 8:k1 * 8].clone()
        ch = torch.arange(k0 * 8, k1 * 8)
        sub[:, :, (ch < c0) | (ch >= c1)] = 0.0
        items = sub.reshape(B, HW * (k1 - k0), 8)
        T = (items.shape[1] + 255) // 256
        pad = torch.zeros((B, T * 256, 8), dtype=torch.float32)
        pad[:, :items.shape[1]] = items
        seq = pad.reshape(B, T, 256, 8).permute(1, 3, 0, 2).reshape(T * 8, B, 256).contiguous()
        a, q = torch.zeros((B, 256)), torch.zeros((B, 256))
        for s in range(T * 8):
            v = seq[s]
            a = a + v
            q = q + v * v
        S1[:, grp], S2[:, grp] = a.double().sum(1), q.double().sum(1)
    return S1, S2


def gn_chunks(HW):
    pix = 32
    while HW // pix > 1024:
        pix *= 2
    return (HW + pix - 1) // pix


def _partial_chunks(X, R):
    """X [B, n, P, C] fp32 (n chunks of P pixels) -> fp32 (s, ss) [B, n, C]: rows r = 0..R-1 take pixels r, r + R, ..., four at a time as
    (f0 + f1) + (f2 + f3) while four are left, then one by one; the rows are added in sequence (the LDS combine)."""
    a = q = None
    for r in range(R):
        seq = X[:, :, r::R, :]
        L = seq.shape[2]
        s = torch.zeros_like(X[:, :, 0, :])
        ss = torch.zeros_like(s)
        i = 0
        while i + 3 < L:
            f0, f1, f2, f3 = seq[:, :, i], seq[:, :, i + 1], seq[:, :, i + 2], seq[:, :, i + 3]
            s = s + ((f0 + f1) + (f2 + f3))
            ss = ss + ((f0 * f0 + f1 * f1) + (f2 * f2 + f3 * f3))
            i += 4
        while i < L:
            f = seq[:, :, i]
            s = s + f
            ss = ss + f * f
            i += 1
        a = s if a is None else a + s
        q = ss if q is None else q + ss
    return (torch.zeros_like(X[:, :, 0, :]) + a), (torch.zeros_like(X[:, :, 0, :]) + q)


def emulate_partial(x, C1, groups):
    """gn_partial_kernel + gn_finalize_kernel's sums: per source, per chunk of pixels, fp32 partials per channel (_partial_chunks); chunks and
    the group's channels combine in float64.  x [B, HW, C] fp32 -> (S1, S2) float64 [B, groups]."""
    B, HW, C = x.shape
    nchunk = gn_chunks(HW)
    pix = (HW + nchunk - 1) // nchunk
    S1c, S2c = [], []
    for lo_c, hi_c in ((0, C1), (C1, C)):
        if hi_c == lo_c:
            continue
        xs = x[:, :, lo_c:hi_c]
        Cs = hi_c - lo_c
        R = 256 // (Cs // 8)
        nfull = HW // pix
        s, ss = _partial_chunks(xs[:, :nfull * pix].reshape(B, nfull, pix, Cs), R)
        s1, s2 = s.double().sum(1), ss.double().sum(1)
        if nfull * pix < HW:
            s, ss = _partial_chunks(xs[:, nfull * pix:].reshape(B, 1, HW - nfull * pix, Cs), R)
            s1, s2 = s1 + s.double().sum(1), s2 + ss.double().sum(1)
        S1c.append(s1)
        S2c.append(s2)
    S1c, S2c = torch.cat(S1c, 1), torch.cat(S2c, 1)
    Cg = C // groups
    return S1c.reshape(B, groups, Cg).sum(2), S2c.reshape(B, groups, Cg).sum(2)


def finalize_emulation(S1, S2, n, eps, gam, bet):
    """The finalize every form shares: float64 mean / var from the sums, rstd, gamma rstd, beta - fp32(mean) gamma rstd in fp32."""
    mean = S1 / n
    var = (S2 / n - mean * mean).clamp_min(0.0)
    rstd = (1.0 / torch.sqrt(var + f32eps(eps))).float()
    Cg = gam.numel() // S1.shape[1]
    gsc = gam.float()[None] * rstd.repeat_interleave(Cg, dim=1)
    return gsc, bet.float()[None] - mean.float().repeat_interleave(Cg, dim=1) * gsc


def stats_emulation(inp, case):
    x = _seen32(inp, case)
    S1, S2 = (emulate_small if case.form == ONE else emulate_partial)(x, case.C1, case.groups)
    return finalize_emulation(S1, S2, float(case.HW * ((case.C1 + case.C2) // case.groups)), case.eps, inp["gamma"], inp["beta"])


# ======================================================================================================================
# 2. fused statistics
# ======================================================================================================================
def sums_reference(y):
    """y [B, HW, N] (the fp16 output, or hi + lo in float64) -> float64 (sum, sum of squares, sum|y|) [B, N]."""
    y = y.double()
    return y.sum(1), (y * y).sum(1), y.abs().sum(1)


def sums_ratio(stats, y, L_b, extra_u=0):
    """stats [B, N, R, 2] fp32 partials, y [B, HW, N]: worst |error| / bound of the two sums (level 1).  One partial is an fp32 chain of L_b
    terms of the block: gamma(L_b) sum|y| for the sum; the squares carry one more rounding each, (gamma(L_b) + 2u) sum y^2.  extra_u: further
    relative error of each summed value in units of u (4 for a split output, whose statistics are of the fp32 value, within 2^-22 of hi + lo)."""
    s, q, sa = sums_reference(y)
    got = stats.double().sum(2)
    rs = ((got[..., 0] - s).abs() / ((gamma(L_b) + extra_u * U) * sa + 1e-300)).max().item()
    rq = ((got[..., 1] - q).abs() / ((gamma(L_b) + (2 + 2 * extra_u) * U) * q + 1e-300)).max().item()
    return rs, rq


def emulate_blocks(y, block_rows):
    """fp32 partials of consecutive blocks of block_rows rows, each one sequential chain: y [B, HW, N] -> [B, N, R, 2] fp32."""
    B, HW, N = y.shape
    R = HW // block_rows
    yb = y.float().reshape(B, R, block_rows, N)
    a, q = torch.zeros((B, R, N)), torch.zeros((B, R, N))
    for i in range(block_rows):
        v = yb[:, :, i]
        a = a + v
        q = q + v * v
    return torch.stack((a, q), -1).permute(0, 2, 1, 3).contiguous()


# ======================================================================================================================
# 3. GroupNorm folded into a 1x1 conv
# ======================================================================================================================
def fold_reference(x, W, s, t, bias):
    """x [B, HW, C] fp16, W [N, C] fp16, s / t [B, C] fp32, bias [N] fp32 or None -> float64 [B, HW, N] = (x s_b + t_b) W^T + bias."""
    a = x.double() * s.double()[:, None, :] + t.double()[:, None, :]
    y = a @ W.double().t()
    return y + bias.double() if bias is not None else y


def fold_tol(x, W, s, t, bias, ref):
    K = x.shape[-1]
    xd, Wd, sd, td = x.double(), W.double(), s.double(), t.double()
    wsx = (xd.abs() * sd.abs()[:, None, :]) @ Wd.abs().t()                                  # sum_c |W s x|
    floor = 2.0 ** -25 * xd.abs().sum(-1, keepdim=True)
    wt = (td.abs() @ Wd.abs().t())[:, None, :]                                               # sum_c |W t|
    tol = (H16 + 2 * U + gamma(K)) * wsx + floor + gamma(K / 64 + 6) * wt + H16 * ref.abs() + U
    return tol + U * bias.double().abs() if bias is not None else tol


def unfolded_tol(x, W, s, t, bias, ref):
    K = x.shape[-1]
    a = (x.double() * s.double()[:, None, :] + t.double()[:, None, :]).abs()
    aw = a @ W.double().abs().t()
    tol = (H16 + 2 * U + gamma(K)) * aw + 2.0 ** -25 * W.double().abs().sum(1) + H16 * ref.abs() + U
    return tol + U * bias.double().abs() if bias is not None else tol


def ratio(got, ref, tol):
    return ((got.double() - ref).abs() / tol).max().item()


def rel_err(got, ref):
    return ((got.double() - ref).abs().max() / ref.abs().max()).item()


def fold_wrong_references(x, W, s, t, bias):
    """[(name, float64 reference)] the fold's bound must reject."""
    B = x.shape[0]
    out = []
    if B > 1:
        nxt = [(b + 1) % B for b in range(B)]
        out.append(("scale / shift of the next image", fold_reference(x, W, s[nxt], t[nxt], bias)))
    keep = torch.ones(x.shape[-1], dtype=torch.float16)
    keep[-64:] = 0
    out.append(("last K block of 64 left out", fold_reference(x, W * keep, s, t, bias)))
    out.append(("shift left out of the bias", fold_reference(x, W, s, torch.zeros_like(t), bias)))
    return out


def folded_weights_emulation(W, s, t, bias):
    """fold_gn_weights_kernel: W_b = fp16(fp32(W) s_b) and bias_b = bias + sum_c W t_b in the kernel's order (lane l of 64 takes channels
    8 l .. 8 l + 7 of every 512, one sequential fp32 chain; six xor-shuffle steps) -> fp16 [B, N, C], fp32 [B, N]."""
    N, K = W.shape
    B = s.shape[0]
    Wf = (W.float()[None] * s.float()[:, None, :]).to(torch.float16)
    trips = (K + 511) // 512
    prod = torch.zeros((B, N, trips * 512))
    prod[:, :, :K] = W.float()[None] * t.float()[:, None, :]
    seq = prod.reshape(B, N, trips, 64, 8).permute(2, 4, 0, 1, 3).reshape(trips * 8, B, N, 64)
    acc = torch.zeros((B, N, 64))
    for i in range(trips * 8):
        acc = acc + seq[i]
    lanes = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, :, lanes ^ off]
    bb = acc[:, :, 0] + (bias.float()[None] if bias is not None else 0.0)
    return Wf, bb


def folded_emulation(x, W, s, t, bias):
    """The folded route on the CPU: the fold kernel's weights and biases, an fp32 GEMM, one rounding to fp16."""
    Wf, bb = folded_weights_emulation(W, s, t, bias)
    return (torch.bmm(x.float(), Wf.float().transpose(1, 2)) + bb[:, None, :]).to(torch.float16)


def unfolded_emulation(x, W, s, t, bias):
    """The GroupNorm prologue route: a = fp16(x s + t), an fp32 GEMM, one rounding."""
    a = (x.float() * s.float()[:, None, :] + t.float()[:, None, :]).to(torch.float16)
    y = a.float() @ W.float().t()
    return (y + bias.float() if bias is not None else y).to(torch.float16)


FoldCase = namedtuple("FoldCase", "B HW C N Nrows bias folds kernel ratio std", defaults=(0.3, 1.0))
FOLD_CASES = {
    # name: B, HW, C, N, Nrows, bias?, the plan folds?, the GEMM kernel the case is meant for
    "vae_qkv_smallest_map": FoldCase(2, 64, 512, 1536, 1536, True, True, "gemm_dma<64,64>"),
    "hw192_three_images": FoldCase(3, 192, 320, 320, 320, True, True, "gemm_dma<64,64>"),
    # M = 1536 rows x 2048 columns would take 128-row tiles (12 x 32 = 384 of them); HW = 192 is no multiple of 128, so the tile rule keeps 64 x 64
    "hw192_tile_rule": FoldCase(8, 192, 320, 2048, 2048, True, True, "gemm_dma<64,64>"),
    "c1280_second_trip": FoldCase(1, 64, 1280, 1280, 1280, True, True, "gemm_dma<64,64>"),
    "nrows_322": FoldCase(2, 64, 320, 320, 322, True, True, "gemm_dma<64,64>"),
    "null_bias": FoldCase(2, 64, 320, 320, 320, False, True, "gemm_dma<64,64>"),
    "hw128_tiles_128": FoldCase(4, 1024, 320, 1536, 1536, True, True, "gemm_dma<128,128>"),   # 128-row tiles where they divide an image
    "hw48_declined": FoldCase(2, 48, 320, 320, 320, True, False, "igemm<64,64,fast,gn>"),
}
# operand regimes on the first shape: (|group mean| / std, std)
FOLD_REGIMES = {"mean0.3": (0.3, 1.0), "mean3": (3.0, 1.0), "mean10": (10.0, 1.0), "std1": (0.0, 1.0), "std1024": (0.0, 1024.0), "std4096": (0.0, 4096.0)}


def make_fold_input(case, seed, ratio_=None, std=None):
    """x fp16 [B, HW, C], W fp16 [Nrows, C] (rows >= N zero), s / t fp32 [B, C], bias fp32 [Nrows] or None.  s and t normalise 32 groups of x
    (float64 statistics), with per-channel gamma / beta, and are then scaled per image by 1, 2.7, 0.4, ... so that image b's weights are wrong
    for every other image."""
    r = case.ratio if ratio_ is None else ratio_
    sd = case.std if std is None else std
    g = torch.Generator().manual_seed(seed)
    B, HW, C = case.B, case.HW, case.C
    groups = 32
    Cg = C // groups
    gmean = r * sd * (1 + 0.2 * (torch.rand((B, 1, groups), generator=g) - 0.5)) * (torch.randint(0, 2, (B, 1, groups), generator=g) * 2 - 1)
    x = (sd * torch.randn((B, HW, C), generator=g) + gmean.repeat_interleave(Cg, dim=2)).to(torch.float16)
    xg = x.double().reshape(B, HW, groups, Cg)
    mean, var = xg.mean((1, 3)), xg.var((1, 3), unbiased=False)
    rstd = (1.0 / torch.sqrt(var + 1e-5)).repeat_interleave(Cg, dim=1)
    gam, bet = 1 + 0.2 * torch.randn(C, generator=g).double(), 0.3 * torch.randn(C, generator=g).double()
    f = torch.tensor([1.0, 2.7, 0.4, 1.9, 0.6, 3.3, 0.8, 1.4])[:B].double()[:, None]
    s = (gam[None] * rstd * f).float()
    t = ((bet[None] - mean.repeat_interleave(Cg, dim=1) * gam[None] * rstd) * f).float()
    W = torch.zeros((case.Nrows, C), dtype=torch.float16)
    W[:case.N] = (torch.randn((case.N, C), generator=g) / math.sqrt(C)).to(torch.float16)
    bias = None
    if case.bias:
        bias = torch.zeros(case.Nrows)
        bias[:case.N] = 0.5 * torch.randn(case.N, generator=g)
    return dict(x=x, W=W, s=s, t=t, bias=bias)


def _measure_c(seeds=20):
    worst = {}
    for name, case in STATS_CASES.items():
        w = 0.0
        for seed in range(seeds):
            inp = make_stats_input(case, 1000 + seed)
            ref = stats_reference(inp["v"], case.groups, case.eps, inp["gamma"], inp["beta"])
            sc, sh = stats_emulation(inp, case)
            w = max(w, stats_c_ratio(sc, sh, ref))
        worst[name] = w
        print(f"[gn-c] {name}: worst emulation error / (u amp) over {seeds} seeds = {w:.3f}", flush=True)
    m = max(worst.values())
    print(f"[gn-c] worst {m:.3f} ({max(worst, key=worst.get)}): c = max(2, 4 x worst) = {max(2.0, 4 * m):.3f}")
    return worst


if __name__ == "__main__":
    _measure_c()
