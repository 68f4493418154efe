"""Float64 references, derived error bounds, wrong references and fp32 emulations for the LayerNorm / linear / GEGLU chain of the transformer
block's forward path (csrc/kernels_norm.hip: layernorm_kernel; csrc/kernels_gemm_ast.hip: lngemm<320>, lngemm<320,geglu>; csrc/kernels_elem.hip:
geglu_kernel; the GEGLU epilogues of gemm_dma / gemm_df and act_out 1 | 2 of gemm_dma; csrc/common.h: erf_as, gelu_erf).  Imports without a
GPU; tests/test_cpu_transformer_bound.py judges every bound here on the CPU, tests/test_gpu_transformer_block.py applies them to the kernels.

u = 2^-24, H16 = 2^-11, gamma(n) = 2 n u (tests/groupnorm_bound.py, whose helpers are used here).

a. LayerNorm.  y = f16(a), a = (x - m) r g + b, m / var over the C channels, r = 1 / sqrt(var + eps); x = what the kernel sees (the fp32 sum
   fp32(hi) + fp32(lo) of a split row, one IEEE addition that the reference repeats: it is not always exact, 1000 + 2^-12 needs 22 bits).  The kernel's order:
     sum     each lane adds its channels in sequence, L = 8 ceil(C / 512) terms in layernorm_kernel (8 channels per 16-byte chunk, one chunk per
             lane and trip, at most 5 trips: L <= 40), then 6 xor-shuffle steps; the lngemm prologue keeps a row in 4 lanes: L = 80 (10 k-steps of 8
             channels), then 2 shuffle steps.  |d sum| <= gamma(L + S) sum|x|.
     mean    sum / C (layernorm_kernel: one rounding) or sum * fp32(1 / C) (lngemm: two).  So dm <= c u mean|x| with the WORST-CASE
             c = gamma(L + S) / u + 2 = 2 (L + S) + 2   (94 for layernorm_kernel at C > 2048, 166 for lngemm).
             The worst case is enough: with it every rejection condition of tests/test_cpu_transformer_bound.py holds, so c is not measured.
     var     two-pass, around the COMPUTED mean: sum (x - m^)^2 / C = var + dm^2 exactly, so dm enters var only squared.  Each square carries the
             rounding of the difference and of the product (3u), the chain gamma(L + S), the division by C 2u and the addition of eps u:
             relative error gamma(L + S) + 6u of var + eps, half of that in r.
     rsqrtf  a hardware approximation: 1 ulp = 2u (the allowance kernels_igemm.hip states for the hardware transcendentals).
             E_r = gamma(L + S) / 2 + 3u + 2u + dm^2 / (2 (var + eps))      relative error of r
     affine  (x - m^) one rounding, * r, * g one each, + b one on the result (or one fewer, contracted to an FMA), in fp32:
             tol_pre = |g| r (dm + |x - m| (E_r + 3u) + u dm) + u |a|        the value before the fp16 rounding
     output  tol = tol_pre + H16 |a| + 2^-24.
   The term that matters is |g| r dm = |g| c u mean|x| / std: the amplification |mean| / std.  At |mean| / std = 1000 (split rows) it is 5.6e-3 |g|
   for layernorm_kernel and accepts the unbiased variance at C >= 640; the benign rows of the same launch reject it (ACCEPTED_AT_HIGH_RATIO).

b. LayerNorm into a GEMM.  ref = sum_c W16_c r16(a_c) + bias with a the float64 LayerNorm (the fused kernel never stores its operand).  The
   kernel's operand is r16(a^) with |a^ - a| <= t = tol_pre: it equals r16(a) unless a lies within t of an fp16 rounding boundary ("flip"), and
   then differs by at most floor(t / ulp) + 1 ulps (one ulp while t < ulp, the usual case).
       tol = sum_{c in flip} |W_c| (floor(t_c / ulp16(a_c)) + 1) ulp16(a_c) + gamma(K) sum_c |r16(a_c) W_c| + u |bias| + H16 |ref| + 2^-24
   and 2u |ref| more for the columns multiplied by qscale in fp32 before the one rounding.  tol_pre is taken with lngemm's chain (the longer
   one), so the two-launch form is judged by the same bound against the same reference.  With the GEGLU epilogue the value and the gate carry this
   bound without its output rounding (T_x, T_g) and
       tol = T_x |gelu(P_g)| + |P_x| (|gelu'(P_g)| + 0.8 T_g) T_g + section c's bound at (h, g) = (P_x, P_g)          (|gelu''| <= 0.8).

c. GELU / GEGLU.  ref = h 0.5 g erfc(-g / sqrt 2) in float64 (never 1 + erf: it cancels in the negative tail).  gelu_erf(g) = 0.5f g (1 + erf_as(g c)),
   c = fp32(1 / sqrt 2): 0.5 g is exact, the product with (1 + erf) rounds once, the product with h once more:
       tol = |h| (0.5 |g| E_ERF + 3u |gelu(g)|) + H16 |ref| + 2^-24
   E_ERF = the absolute error of the fp32 value 1 + erf_as(fp32(g c)) against erfc(-g / sqrt 2).  It is MEASURED: emulate_erf_as repeats common.h's
   sequence in float32 (every FMA as one rounding, exact reciprocal and exp2) and E_ERF = 2 x its worst error over every finite fp16 gate and the
   fp32 gates of the fused-epilogue cases (epilogue_gates); the 2 is for the 1 ulp each of v_rcp_f32 and v_exp_f32.  See the constants below.
   The Abramowitz & Stegun 7.1.26 formula itself is within 1.5e-7 of erf in exact arithmetic; the fp32 evaluation is 3-4 times that, worst near
   g = 0.06, where 1 - poly t e cancels to ~0.05 and keeps the rounding of a value near 1.  In the negative tail 1 + erf_as is a multiple of 2^-24: for
   g < -5.547 gelu_erf returns -0 where the true value is -8e-8 and smaller -- inside 0.5 |g| E_ERF, but a relative error of 100 %.
   A split output (act_out behind the text encoder's FC1: hi + lo) replaces H16 |ref| by 2^-21 |ref| + 2^-24: only that case can tell the sixth digit of a
   coefficient, everywhere else the fp16 rounding of the output is 50 times larger than such a change.
   quick_gelu (act_out 1, kernels_gemm.hip act_out4): v rcp(1 + exp2(v k)), k = fp32(-fp32(1.702) fp32(log2 e)), a constant folded in fp32.  Roundings
   found, as relative errors of s = sigmoid(z), z = fp32(1.702) v: the constant k (fp32(log2 e) and the folded product: 2u of the exponent, i.e.
   2 |z| (1 - s) u of s), the product v k (|z| (1 - s) u), v_exp_f32 (2u of e: (1 - s) 2u), 1 + e (u), v_rcp_f32 (2u), and v * s (u):
       tol = |v s| (6 + 3 |z| (1 - s)) u + the output rounding
   -- not the flat 4u: the roundings of the exponent alone pass it for z < -1.4.
"""
import math
from collections import namedtuple

import numpy as np
import torch

from groupnorm_bound import H16, U, f32eps, gamma

SQRT1_2 = 0.7071067811865476
LOG2E = 1.4426950408889634
F16_MAX_ROUND = 65520.0        # |value| >= this rounds to infinity

# ---- measured constants (python tests/transformer_bound.py prints them) ----------------------------------------------------------------------
# emulate_erf_as, worst |1 + erf_as(fp32(g c)) - erfc(-g / sqrt 2)|: 5.128e-7 over the 63,488 finite fp16 gates (at g = 0.0596), 4.772e-7 over the
# fp32 gates of epilogue_gates (every gelu-form fused-epilogue case; at g = 0.0426).  E_ERF = 2 x 5.128e-7, rounded up.  (With a5 changed in its
# sixth digit the same measurement gives 1.04e-5.)
E_ERF_WORST_EMULATION = 5.128e-7
E_ERF = 1.03e-6
# ... and of gelu itself, |0.5 g (1 + erf_as) - gelu(g)|: 4.54e-7 absolute (g = 3.033); gelu_erf returns -0 for every gate below -5.547, where the
# true value is -8.1e-8 and smaller: a relative error of 100 %, inside 0.5 |g| E_ERF.
GELU_WORST_EMULATION = 4.544e-7


# ======================================================================================================================
# a. LayerNorm
# ======================================================================================================================
LN_KERNEL, LNGEMM_KERNEL = "layernorm", "lngemm"


def chain_terms(C, kernel=LN_KERNEL):
    """(L, S): the terms one lane adds in sequence and the shuffle steps behind them."""
    return (80, 2) if kernel == LNGEMM_KERNEL else (8 * ((C + 511) // 512), 6)


def c_mean(C, kernel=LN_KERNEL):
    """dm <= c u mean|x|, worst case."""
    L, S = chain_terms(C, kernel)
    return 2.0 * (L + S) + 2.0


LnRef = namedtuple("LnRef", "a xc r var absmean gamma eps")


def ln_reference(x, gam, bet, eps, unbiased=False, stat_channels=None, divisor=None, onepass32=False):
    """float64 LayerNorm of x [rows, C] (float64: the values the kernel sees).  The keyword arguments make the wrong references: unbiased (var / (C - 1)),
    stat_channels (statistics over the first so many channels only, still divided by C), divisor (mean and variance divided by it instead of C),
    onepass32 (var = E[x^2] - E[x]^2 accumulated in fp32)."""
    x = x.double()
    C = x.shape[1]
    n = float(divisor if divisor else C)
    xs = x[:, :stat_channels] if stat_channels else x
    if onepass32:
        x32 = xs.float()
        m32 = x32.sum(1, keepdim=True) / n
        var = ((x32 * x32).sum(1, keepdim=True) / n - m32 * m32).clamp_min(0.0).double()
        m = m32.double()
    else:
        m = xs.sum(1, keepdim=True) / n
        var = ((xs - m) ** 2).sum(1, keepdim=True) / (n - 1.0 if unbiased else n)
    e = f32eps(eps)
    r = 1.0 / torch.sqrt(var + e)
    a = (x - m) * r * gam.double()[None] + bet.double()[None]
    return LnRef(a, x - m, r, var, x.abs().mean(1, keepdim=True), gam.double()[None], e)


def ln_tol_pre(ref, C, kernel=LN_KERNEL):
    L, S = chain_terms(C, kernel)
    dm = c_mean(C, kernel) * U * ref.absmean
    e_r = gamma(L + S) / 2 + 5 * U + dm * dm / (2 * (ref.var + ref.eps))
    return ref.gamma.abs() * ref.r * (dm * (1 + U) + ref.xc.abs() * (e_r + 3 * U)) + U * ref.a.abs()


def ln_tol(ref, C, kernel=LN_KERNEL):
    return ln_tol_pre(ref, C, kernel) + H16 * ref.a.abs() + 2.0 ** -24


def row_ratio(got, ref, tol):
    """[rows]: each row's worst |error| / bound."""
    return torch.nan_to_num((got.double() - ref).abs() / tol, nan=float("inf")).amax(1)


FAMILIES = ("benign", "ratio30", "ratio1000", "const", "vareps", "outlier_first", "outlier_last", "zero")
CONST_VALUES = (1.5, -3.0, 0.25, 96.0)     # every fp32 partial sum of C <= 2560 of them is exact, and so is sum / C

LnCase = namedtuple("LnCase", "C rows layout eps first", defaults=(1e-5, 0))
LN_CASES = {
    # name: C, rows, layout, eps, the family of row 0 (row i is of family (first + i) % 8; "ratio1000" is "ratio30" unless the rows are split)
    "c8_one_lane": LnCase(8, 513, "plain"),
    "c64": LnCase(64, 513, "split"),
    "c320": LnCase(320, 513, "plain"),
    "c320_split": LnCase(320, 513, "split"),
    "c320_pitched_eps6": LnCase(320, 513, "pitched", 1e-6),
    "c512_one_full_trip": LnCase(512, 5, "plain", first=0),
    "c520_lane0_second_trip": LnCase(520, 513, "split"),
    "c640": LnCase(640, 513, "plain"),
    "c640_split_eps6": LnCase(640, 513, "split", 1e-6),
    "c1280": LnCase(1280, 513, "plain"),
    "c1280_split": LnCase(1280, 513, "split"),
    "c1280_pitched_rows3": LnCase(1280, 3, "pitched", first=4),
    "c2048_four_full_trips": LnCase(2048, 4, "plain", first=1),
    "c2056_lane0_fifth_trip": LnCase(2056, 513, "split"),
    "c2560": LnCase(2560, 513, "plain"),
    "c2560_split_row1": LnCase(2560, 1, "split", first=2),
    "c2560_pitched_rows5_eps6": LnCase(2560, 5, "pitched", 1e-6, first=3),
    "c640_rows1_vareps": LnCase(640, 1, "plain", first=4),
    "c320_rows4_split": LnCase(320, 4, "split", first=4),
}
PITCH_EXTRA = 24      # a pitched view's rows are C + 24 apart (a multiple of 8 that is no multiple of 64)
# Wrong references the bound of a |mean| / std = 1000 row accepts (its allowance for the mean, c u mean|x| / std = 94 u 1000 = 5.6e-3 |g| at C > 2048, is
# larger than they are), and the family of the SAME launch and width that rejects each: the unbiased variance at C >= 640 (1 / 2C <= 7.8e-4), eps = 0 /
# 1e-6 / 1e-3 (the row's variance is 1), both rejected by the benign resp. the variance-near-eps rows.  Constant and all-zero rows normalise to beta
# whatever the statistics are: they judge nothing but eps = 0 (0 x inf) and the affine step, and are compared with f16(beta) exactly.
ACCEPTED_AT_HIGH_RATIO = {"variance / (C - 1)": "benign", "eps = 0": "vareps", "eps = 1e-06": "vareps", "eps = 1e-05": "vareps", "eps = 0.001": "vareps"}
# the family whose rows must reject each wrong reference wherever a launch has such rows (tests/test_cpu_transformer_bound.py, tests/test_gpu_transformer_block.py)
KILLED_BY = {"variance / (C - 1)": "benign", "eps = 0": "vareps", "eps = 1e-06": "vareps", "eps = 1e-05": "vareps", "eps = 0.001": "vareps",
             "one-pass variance in fp32": "ratio1000", "statistics without the last trip": "benign", "statistics without the lo half": "benign",
             "gamma / beta of the next chunk": "benign", "mean over the pitch": "benign"}


def by_family(per_row, fam):
    """{family: worst of its rows}."""
    out = {}
    for v, f in zip(per_row.tolist(), fam):
        out[f] = max(out.get(f, 0.0), v)
    return out


def out_rounding(ref, split_out=False):
    """The part of every bound that is the output's own rounding (a split output: of its lo half)."""
    return (2.0 ** -21 if split_out else H16) * ref.abs() + 2.0 ** -24


def margin(got, ref, tol, split_out=False, mask=None):
    """What the error exceeds the output's own rounding by, as a fraction of the rest of the bound: the output rounding alone takes an element to
    0.99 of `tol` by its nature, this is the share of the DERIVED part that is used."""
    out = out_rounding(ref, split_out)
    r = ((got.double() - ref).abs() - out * (1 + 1e-9)).clamp_min(0.0) / (tol - out + 1e-300)
    if mask is not None:
        r = torch.where(mask, r, torch.zeros_like(r))
    return torch.nan_to_num(r, nan=float("inf")).max().item()


def families_of(case):
    fam = [FAMILIES[(case.first + i) % len(FAMILIES)] for i in range(case.rows)]
    return [("ratio30" if f == "ratio1000" and case.layout != "split" else f) for f in fam]


def make_ln_input(case, seed, C=None, rows=None):
    """-> dict(hi, lo [rows, C] fp16 (lo None unless split), x [rows, C] float64 = hi + lo, gamma, beta [C] fp32 (gamma with zeros and negative
    entries), fam [rows] family names)."""
    C = case.C if C is None else C
    rows = case.rows if rows is None else rows
    g = torch.Generator().manual_seed(seed)
    fam = families_of(case._replace(rows=rows))
    z = torch.randn((rows, C), generator=g, dtype=torch.float64)
    sd = 10.0 ** (-3.0 + torch.rand((rows, 1), generator=g, dtype=torch.float64))          # 1e-3 .. 1e-2
    x = torch.empty((rows, C), dtype=torch.float64)
    for i, f in enumerate(fam):
        if f == "benign":
            x[i] = 2.0 * z[i] + 0.5
        elif f == "ratio30":
            x[i] = 30.0 + z[i]
        elif f == "ratio1000":
            x[i] = 1000.0 + z[i]
        elif f == "const":
            x[i] = CONST_VALUES[(i // len(FAMILIES)) % len(CONST_VALUES)]
        elif f == "vareps":
            x[i] = sd[i] * z[i]
        elif f in ("outlier_first", "outlier_last"):
            x[i] = z[i]
            x[i, 0 if f == "outlier_first" else C - 1] = 1.0e4
        else:
            x[i] = 0.0
    hi = x.to(torch.float16)
    lo = (x - hi.double()).to(torch.float16) if case.layout == "split" else None
    v = (hi.float() + lo.float()).double() if lo is not None else hi.double()      # the kernel's own fp32 addition (load8)
    gam = 1.0 + 0.3 * torch.randn(C, generator=g)
    gam[::7] = 0.0
    gam[3::5] = -gam[3::5]
    bet = 0.5 * torch.randn(C, generator=g)
    return dict(hi=hi, lo=lo, x=v, gamma=gam, beta=bet, fam=fam)


def ln_wrong_references(inp, case, eps=None):
    """[(name, float64 reference)] of the LayerNorm of the case."""
    eps = case.eps if eps is None else eps
    x, gam, bet = inp["x"], inp["gamma"], inp["beta"]
    C = x.shape[1]
    out = [("variance / (C - 1)", ln_reference(x, gam, bet, eps, unbiased=True).a)]
    for e in (0.0, 1e-6, 1e-5, 1e-3):
        if e != eps:
            out.append((f"eps = {e:g}", ln_reference(x, gam, bet, e).a))
    out.append(("one-pass variance in fp32", ln_reference(x, gam, bet, eps, onepass32=True).a))
    if C > 512:
        out.append(("statistics without the last trip", ln_reference(x, gam, bet, eps, stat_channels=((C - 1) // 512) * 512).a))
    if inp["lo"] is not None:
        rh = ln_reference(inp["hi"].double(), gam, bet, eps)
        out.append(("statistics without the lo half", (x - (inp["hi"].double() - rh.xc)) * rh.r * gam.double()[None] + bet.double()[None]))
    if C > 8:
        out.append(("gamma / beta of the next chunk", ln_reference(x, torch.roll(gam, -8), torch.roll(bet, -8), eps).a))
    if case.layout == "pitched":
        out.append(("mean over the pitch", ln_reference(x, gam, bet, eps, divisor=C + PITCH_EXTRA).a))
    return out


def _lane_sums(t, shuffles):
    """t [rows, terms, lanes] fp32 -> [rows]: every lane adds its terms in sequence, then xor-shuffle steps over the lanes."""
    acc = torch.zeros((t.shape[0], t.shape[2]), dtype=torch.float32)
    for s in range(t.shape[1]):
        acc = acc + t[:, s]
    lanes = torch.arange(t.shape[2])
    for off in shuffles:
        acc = acc + acc[:, lanes ^ off]
    return acc[:, 0]


def _lanes(v, kernel):
    """v [rows, C] fp32 -> ([rows, terms, lanes] in the kernel's order, mask of the channels that exist, shuffle offsets)."""
    rows, C = v.shape
    if kernel == LNGEMM_KERNEL:                     # lane g of 4 holds channels ks * 32 + g * 8 + j, added ks-major
        return v.reshape(rows, C // 32, 4, 8).permute(0, 1, 3, 2).reshape(rows, C // 4, 4), None, (1, 2)
    trips = (C + 511) // 512
    pad = torch.zeros((rows, trips * 512), dtype=torch.float32)
    pad[:, :C] = v
    mask = torch.zeros(trips * 512, dtype=torch.bool)
    mask[:C] = True
    to = lambda t: t.reshape(-1, trips, 64, 8).permute(0, 1, 3, 2).reshape(-1, trips * 8, 64)
    return to(pad), to(mask[None].expand(1, -1))[0], (32, 16, 8, 4, 2, 1)


def emulate_layernorm(inp, eps, kernel=LN_KERNEL, unbiased=False):
    """The kernel's LayerNorm in fp32, in its own order (module docstring a.) -> fp32 [rows, C], the value BEFORE the fp16 rounding.  rsqrtf is the
    correctly rounded value.  unbiased: the deliberate defect of the mutation check (variance / (C - 1))."""
    v = inp["hi"].float()
    if inp["lo"] is not None:
        v = v + inp["lo"].float()
    rows, C = v.shape
    t, mask, sh = _lanes(v, kernel)
    s = _lane_sums(t, sh)
    if kernel == LNGEMM_KERNEL:
        mean = s * torch.tensor(1.0 / C, dtype=torch.float32)
    else:
        mean = s / torch.tensor(float(C), dtype=torch.float32)
    d = t - mean[:, None, None]
    if mask is not None:
        d = torch.where(mask[None], d, torch.zeros((), dtype=torch.float32))
    q = _lane_sums(d * d, sh)
    n = torch.tensor(float(C - 1 if unbiased else C), dtype=torch.float32)
    arg = (q * (torch.tensor(1.0, dtype=torch.float32) / n) if kernel == LNGEMM_KERNEL else q / n) + torch.tensor(eps, dtype=torch.float32)
    rstd = (1.0 / torch.sqrt(arg.double())).float()
    return (v - mean[:, None]) * rstd[:, None] * inp["gamma"].float()[None] + inp["beta"].float()[None]


# ======================================================================================================================
# b. LayerNorm into a GEMM
# ======================================================================================================================
def r16(t):
    return t.to(torch.float16).double()


def ulp16(a):
    """The spacing of fp16 at |a| (float64 tensor)."""
    _, ex = torch.frexp(a.abs().clamp_min(2.0 ** -24))
    return torch.ldexp(torch.ones_like(a), (ex - 1).clamp_min(-14) - 10)


def flip_allowance(a, t):
    """[..] the most r16(a^) can differ from r16(a) for |a^ - a| <= t: 0 where a is farther than t from every fp16 rounding boundary, else
    (floor(t / ulp) + 1) ulp, ulp taken at |a| + t."""
    ulp = ulp16(a.abs())
    frac = a.abs() / ulp
    dist = ((frac - torch.floor(frac)) - 0.5).abs() * ulp
    ulp_hi = ulp16(a.abs() + t)
    return torch.where(dist <= t, (torch.floor(t / ulp_hi) + 1.0) * ulp_hi, torch.zeros_like(a))


LinRef = namedtuple("LinRef", "ref tol pre tol_pre")


def ln_linear_reference(lnref, W, bias, C, qcols=0, qscale=1.0, a=None):
    """-> LinRef(ref, tol [M, N] float64 of the plain epilogue; pre, tol_pre: the same without the output's rounding, for the GEGLU epilogue).
    lnref: ln_reference of the rows; W [N, C] fp16; bias [N] fp32 or None; a: another float64 operand in place of lnref.a (the wrong references)."""
    Wd = W.double()
    a16 = r16(lnref.a if a is None else a)
    pre = a16 @ Wd.t()
    e = flip_allowance(lnref.a, ln_tol_pre(lnref, C, LNGEMM_KERNEL))
    tol = e @ Wd.abs().t() + gamma(C) * (a16.abs() @ Wd.abs().t())
    if bias is not None:
        pre = pre + bias.double()[None]
        tol = tol + U * bias.double().abs()[None]
    tol_pre = tol + U * pre.abs()
    ref, tol = pre.clone(), tol.clone()
    if qcols:
        ref[:, :qcols] = ref[:, :qcols] * float(torch.tensor(qscale, dtype=torch.float32))
        tol[:, :qcols] = tol[:, :qcols] * abs(qscale) + 2 * U * ref[:, :qcols].abs()
    return LinRef(ref, tol + H16 * ref.abs() + 2.0 ** -24, pre, tol_pre)


def gelu64(g):
    g = g.double()
    return 0.5 * g * torch.special.erfc(-g * SQRT1_2)


def gelu_prime64(g):
    g = g.double()
    return 0.5 * torch.special.erfc(-g * SQRT1_2) + g * torch.exp(-0.5 * g * g) / math.sqrt(2 * math.pi)


def ln_geglu_reference(lin, inner):
    """The GEGLU epilogue behind ln_linear_reference (columns [value | gate], each `inner` wide) -> (ref, tol) [M, inner]."""
    px, pg, tx, tg = lin.pre[:, :inner], lin.pre[:, inner:], lin.tol_pre[:, :inner], lin.tol_pre[:, inner:]
    ref = px * gelu64(pg)
    tol = tx * gelu64(pg).abs() + px.abs() * (gelu_prime64(pg).abs() + 0.8 * tg) * tg + geglu_tol(px, pg, ref)
    return ref, tol


LinCase = namedtuple("LinCase", "M N split bias qcols geglu first", defaults=(0,))
QSCALE = LOG2E / math.sqrt(40.0)
LIN_CASES = {
    # M around the 32-row wave and the 128-row workgroup; N = one panel, two, an odd count, the q/k/v shape
    "m1_n64": LinCase(1, 64, False, True, 0, False, 0),
    "m31_n128_split_q64": LinCase(31, 128, True, False, 64, False),
    "m32_n192": LinCase(32, 192, False, True, 0, False),
    "m33_n960_split_q320": LinCase(33, 960, True, True, 320, False),
    "m127_n64_split_q64": LinCase(127, 64, True, True, 64, False),
    "m128_n128_geglu": LinCase(128, 128, False, False, 0, True),
    "m129_n192_split_q64": LinCase(129, 192, True, True, 64, False),
    "m300_n960_split_q320": LinCase(300, 960, True, True, 320, False),
    "m300_n960_plain": LinCase(300, 960, False, False, 0, False),
    "m300_n128_split_geglu": LinCase(300, 128, True, True, 0, True),
    "m33_n128_geglu": LinCase(33, 128, False, True, 0, True, 5),
}


def geglu_perm(inner):
    """Row r of the [value | gate] weight matrix -> its row in the x / gate-interleaved-by-16 layout the kernels read."""
    perm = torch.empty(2 * inner, dtype=torch.long)
    for r in range(2 * inner):
        q = r if r < inner else r - inner
        perm[(q // 16) * 32 + (0 if r < inner else 16) + q % 16] = r
    return perm


def make_lin_input(case, seed):
    C = 320
    inp = make_ln_input(LnCase(C, case.M, "split" if case.split else "plain", 1e-5, case.first), seed)
    g = torch.Generator().manual_seed(seed + 1)
    inp["W"] = (torch.randn((case.N, C), generator=g) / math.sqrt(C)).to(torch.float16)
    inp["bias"] = 0.3 * torch.randn(case.N, generator=g) if case.bias else None
    return inp


def emulate_ln_linear(inp, case, eps=1e-5, kernel=LNGEMM_KERNEL, unbiased=False):
    """fp32 emulation of the fused launch (or, kernel = LN_KERNEL, of the two-launch form): the LayerNorm emulation rounded once to fp16, an fp32
    GEMM, the epilogue in fp32, one rounding."""
    a16 = emulate_layernorm(inp, eps, kernel, unbiased).to(torch.float16)
    p = a16.float() @ inp["W"].float().t()
    if inp["bias"] is not None:
        p = p + inp["bias"].float()[None]
    if case.geglu:
        inner = case.N // 2
        return (p[:, :inner] * emulate_gelu(p[:, inner:])).to(torch.float16)
    if case.qcols and kernel == LNGEMM_KERNEL:
        p[:, :case.qcols] = p[:, :case.qcols] * torch.tensor(QSCALE, dtype=torch.float32)
    return p.to(torch.float16)


def lin_reference(inp, case, eps=1e-5, qscaled=True, a=None, lnref=None):
    """(ref, tol) of the case's output; a: a wrong LayerNorm in place of the right one."""
    lnref = ln_reference(inp["x"], inp["gamma"], inp["beta"], eps) if lnref is None else lnref
    lin = ln_linear_reference(lnref, inp["W"], inp["bias"], 320, case.qcols if qscaled else 0, QSCALE, a=a)
    return ln_geglu_reference(lin, case.N // 2) if case.geglu else (lin.ref, lin.tol)


# ======================================================================================================================
# c. GELU / GEGLU
# ======================================================================================================================
A_S = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)      # Abramowitz & Stegun 7.1.26, a1 .. a5
A5_SIXTH_DIGIT = 1.061415429                                                      # the wrong reference / mutation: a5 changed in its sixth digit


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def _fma(a, b, c):
    """One rounding: the product of two fp32 values is exact in float64."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate_erf_as(x, a5=A_S[4]):
    """common.h's erf_as in float32 (numpy), operation by operation, every FMA one rounding, exact reciprocal and exp2.  x: float32 array."""
    x = np.asarray(x, dtype=np.float32)
    k = lambda v: np.float32(v)
    ax = np.abs(x)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        t = (1.0 / _fma(np.full_like(ax, k(0.3275911)), ax, np.full_like(ax, k(1.0))).astype(np.float64)).astype(np.float32)
        poly = _fma(np.full_like(t, k(a5)), t, np.full_like(t, k(A_S[3])))
        poly = _fma(poly, t, np.full_like(t, k(A_S[2])))
        poly = _fma(poly, t, np.full_like(t, k(A_S[1])))
        poly = _fma(poly, t, np.full_like(t, k(A_S[0])))
        arg = (ax * ax) * k(-LOG2E)                                  # two fp32 roundings
        e = np.exp2(arg.astype(np.float64)).astype(np.float32)
        y = _fma(-(poly * t), e, np.full_like(t, k(1.0)))
    return np.copysign(y, x)


def emulate_one_plus_erf(g, a5=A_S[4]):
    """fp32 1 + erf_as(fp32(g c)), c = fp32(1 / sqrt 2): the factor of gelu_erf that E_ERF bounds.  g: float32 array."""
    g = np.asarray(g, dtype=np.float32)
    return np.float32(1.0) + emulate_erf_as(g * np.float32(SQRT1_2), a5)


def emulate_gelu(g, a5=A_S[4]):
    """gelu_erf in fp32 -> a torch fp32 tensor of g's shape (g: torch fp32)."""
    gn = g.detach().cpu().numpy().astype(np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        out = (np.float32(0.5) * gn) * emulate_one_plus_erf(gn, a5)
    return torch.from_numpy(out.astype(np.float32)).reshape(g.shape)


def one_plus_erf64(g):
    return torch.special.erfc(-torch.as_tensor(g, dtype=torch.float64) * SQRT1_2)


def erf_error(g, a5=A_S[4]):
    """Worst |emulate_one_plus_erf - erfc(-g / sqrt 2)| over the float32 array g, and the g it is at."""
    g = np.asarray(g, dtype=np.float32).ravel()
    err = (torch.from_numpy(emulate_one_plus_erf(g, a5).astype(np.float64)) - one_plus_erf64(g.astype(np.float64))).abs()
    i = int(err.argmax())
    return float(err[i]), float(g[i])


def geglu_reference(h, g):
    return h.double() * gelu64(g)


def geglu_tol(h, g, ref, split_out=False):
    h, g = h.double(), g.double()
    out = (2.0 ** -21 if split_out else H16) * ref.abs() + 2.0 ** -24
    return h.abs() * (0.5 * g.abs() * E_ERF + 3 * U * gelu64(g).abs()) + out


K_QUICK = float(torch.tensor(1.702, dtype=torch.float32))      # the constant the kernel (and fp32 torch) uses


def quick_gelu_reference(v):
    v = v.double()
    return v * torch.sigmoid(K_QUICK * v)


def quick_gelu_tol(v, ref, split_out=False):
    v = v.double()
    z = K_QUICK * v
    s = torch.sigmoid(z)
    return ref.abs() * (6.0 + 3.0 * z.abs() * (1.0 - s)) * U + (2.0 ** -21 if split_out else H16) * ref.abs() + 2.0 ** -24


def emulate_quick_gelu(v):
    """act_out4's quick_gelu in fp32, operation by operation (exact reciprocal and exp2) -> torch fp32."""
    vn = v.detach().cpu().numpy().astype(np.float32)
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        k = np.float32(-1.702) * np.float32(LOG2E)                       # the kernel's constant: folded in fp32
        e = np.exp2((vn * k).astype(np.float64)).astype(np.float32)
        out = vn * (1.0 / (np.float32(1.0) + e).astype(np.float64)).astype(np.float32)
    return torch.from_numpy(out).reshape(v.shape)


def gelu_tanh64(g):
    g = g.double()
    return 0.5 * g * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (g + 0.044715 * g ** 3)))


def gelu_as64(g, a5):
    """0.5 g (1 + erf) with the A&S formula in float64 and another a5: the wrong reference 'a5 changed in its sixth digit' is this at A5_SIXTH_DIGIT
    minus this at the right a5, added to the right gelu (so that the formula's own 1.5e-7 does not count against it)."""
    g = g.double()
    x = g * SQRT1_2
    t = 1.0 / (1.0 + 0.3275911 * x.abs())
    poly = (((a5 * t + A_S[3]) * t + A_S[2]) * t + A_S[1]) * t + A_S[0]
    return 0.5 * g * (1.0 + torch.sign(x) * (1.0 - poly * t * torch.exp(-x * x)))


def gelu_wrong_references(g):
    """[(name, float64 gelu(g))] wrong forms of the exact GELU (the value is multiplied by h outside)."""
    return [("tanh-form GELU", gelu_tanh64(g)),
            ("quick_gelu in place of gelu", quick_gelu_reference(g)),
            ("erf with a5 changed in its sixth digit", gelu64(g) + gelu_as64(g, A5_SIXTH_DIGIT) - gelu_as64(g, A_S[4]))]


# ---- the gates of the tests ---------------------------------------------------------------------------------------
GEGLU_H = (1.0, -1.0, 1.0 / 3.0, 100.0, 2.0 ** -14, 6.0e4)


def all_fp16():
    """Every finite fp16 value (63,488 of them: +-0 and the subnormals included), as an fp16 tensor in bit order."""
    bits = torch.arange(0, 65536, dtype=torch.int32)
    bits = bits[(bits & 0x7C00) != 0x7C00]
    return bits.to(torch.int16).view(torch.float16)


def geglu_sweep_input():
    """The one launch of the geglu_kernel sweep: rows = the six h of GEGLU_H, C4 = 63,488: [6, 2 C4] fp16 = [h | every finite fp16 gate]."""
    gts = all_fp16()
    x = torch.empty((len(GEGLU_H), 2 * gts.numel()), dtype=torch.float16)
    for i, h in enumerate(GEGLU_H):
        x[i, :gts.numel()] = h
    x[:, gts.numel():] = gts[None]
    return x


EpiCase = namedtuple("EpiCase", "kernel mode M K N split_out", defaults=(False,))
# The fused epilogues, exact by construction: weight row n is one-hot, so column n's fp32 sum is ONE fp16 element of the row (every other product is
# an exact zero), and the fp32 bias moves it off the fp16 grid.  M, N straddle one tile: 64 x 64 of gemm_dma<64,64> (M = 130: two tiles and two
# rows; N = 96 / 72: a tile and a half / a tile and a 16-byte group); the 128 columns (64 outputs) of an lngemm<320,geglu> panel and its 32-row wave;
# gemm_df<geglu> only at the smallest shape plan_conv sends there (M >= 4096 rows, K >= 512; N = 256 is two of its 128-column units).
EPI_CASES = {
    "gemm_dma_geglu": EpiCase("gemm_dma<64,64>", "geglu", 130, 64, 96),
    "gemm_dma_act_gelu": EpiCase("gemm_dma<64,64>", "gelu", 130, 64, 72),
    "gemm_dma_act_gelu_split_out": EpiCase("gemm_dma<64,64>", "gelu", 130, 64, 72, True),
    "gemm_dma_act_quick_gelu": EpiCase("gemm_dma<64,64>", "quick_gelu", 130, 64, 72),
    "gemm_dma_act_quick_gelu_split_out": EpiCase("gemm_dma<64,64>", "quick_gelu", 130, 64, 72, True),     # the text encoder's FC1 as it runs: hi | lo
    "gemm_df_geglu": EpiCase("gemm_df<geglu>", "geglu", 4096, 512, 256),
    "lngemm_geglu": EpiCase("lngemm<320,geglu>", "geglu", 33, 320, 2560),
}


def sweep_values(n, seed):
    """n gate values: dense over [-12, 12] (4/5 of them, evenly spaced and jittered), the rest log-spaced tails to +-6e4 and +-0."""
    g = torch.Generator().manual_seed(seed)
    nd = (4 * n) // 5
    dense = torch.linspace(-12.0, 12.0, nd, dtype=torch.float64) + (torch.rand(nd, generator=g, dtype=torch.float64) - 0.5) * (24.0 / nd)
    nt = n - nd
    mag = 12.0 * (6.0e4 / 12.0) ** torch.linspace(0.0, 1.0, nt, dtype=torch.float64)
    tails = mag * (1.0 - 2.0 * (torch.arange(nt) % 2).double())
    tails[:2] = torch.tensor([0.0, -0.0], dtype=torch.float64)
    v = torch.cat([dense, tails])
    return v[torch.randperm(n, generator=g)]


def make_epilogue_input(name):
    """-> dict(x [M, K] fp16, W [N, K] fp16 one-hot rows ([value | gate] order for geglu), bias [N] fp32, h32 / g32 [M, Nout] fp32: the value and the
    gate (act_out: the pre-activation) each output sees, exactly.  lngemm: x is a dummy row set, gamma = 0 and beta holds the operand, so that the
    normalised operand is f16(beta) exactly for every row."""
    case = EPI_CASES[name]
    seed = sum(map(ord, name))
    g = torch.Generator().manual_seed(seed)
    M, K, N = case.M, case.K, case.N
    geglu = case.mode == "geglu"
    Nout = N // 2 if geglu else N
    out = {}
    if case.kernel.startswith("lngemm"):
        op = torch.empty((1, K), dtype=torch.float64)
        op[0, :K // 2] = sweep_values(K // 2, seed)                      # gate channels
        op[0, K // 2:] = torch.tensor(GEGLU_H, dtype=torch.float64).repeat(K)[:K - K // 2]
        op16 = op.to(torch.float16).expand(M, K).contiguous()
        out["beta"], out["gamma"] = op16[0].float(), torch.zeros(K)
        x = (torch.randn((M, K), generator=g) * 2 + 0.5).to(torch.float16)
        gate_ch = torch.arange(Nout) % (K // 2)
        val_ch = K // 2 + torch.arange(Nout) % (K - K // 2)
    else:
        ng = K - len(GEGLU_H) if geglu else K
        vals = sweep_values(M * ng, seed).reshape(M, ng)
        x = torch.empty((M, K), dtype=torch.float16)
        x[:, :ng] = vals.to(torch.float16)
        if geglu:
            x[:, ng:] = torch.tensor(GEGLU_H, dtype=torch.float16)[None]
        op16 = x
        gate_ch = torch.arange(Nout) % ng
        val_ch = ng + torch.arange(Nout) % len(GEGLU_H) if geglu else None
    W = torch.zeros((N, K), dtype=torch.float16)
    if geglu:
        W[torch.arange(Nout), val_ch] = 1.0
        W[Nout + torch.arange(Nout), gate_ch] = 1.0
    else:
        W[torch.arange(N), gate_ch] = 1.0
    bias = (torch.rand(N, generator=g) - 0.5) * 0.25
    bias[::5] = 0.0                                                       # some gates stay on the fp16 grid
    if geglu:
        bias[:Nout] = bias[:Nout] * (torch.arange(Nout) % 2)              # ... and every other value
    if case.kernel.startswith("lngemm"):                                  # one row of operands only: the bias carries the sweep of the gates
        bias[Nout:] = (sweep_values(Nout, seed + 1) - op16[0, gate_ch].double()).float()
    p32 = op16.float() @ W.float().t() + bias[None]                       # exact: one nonzero product per sum, then ONE fp32 addition
    assert torch.equal((op16.double() @ W.double().t() + bias.double()[None]).float(), p32)
    out.update(x=x, W=W, bias=bias, h32=p32[:, :Nout] if geglu else None, g32=p32[:, Nout:] if geglu else p32)
    return out


def epilogue_reference(name, inp):
    """(ref, tol, [(wrong name, wrong ref)]) of the case's output [M, Nout]."""
    case = EPI_CASES[name]
    gt = inp["g32"]
    if case.mode == "quick_gelu":
        ref = quick_gelu_reference(gt)
        return ref, quick_gelu_tol(gt, ref, case.split_out), [("gelu in place of quick_gelu", gelu64(gt))]
    h = inp["h32"] if case.mode == "geglu" else torch.ones_like(gt)
    ref = geglu_reference(h, gt)
    wrong = [(n, h.double() * w) for n, w in gelu_wrong_references(gt)]
    if case.mode == "geglu":
        wrong.append(("value and gate halves swapped", geglu_reference(gt, h)))
    return ref, geglu_tol(h, gt, ref, case.split_out), wrong


def emulate_epilogue(name, inp):
    """The epilogue in fp32 -> the fp16 output (a split output: hi + lo as float64)."""
    case = EPI_CASES[name]
    v = emulate_quick_gelu(inp["g32"]) if case.mode == "quick_gelu" else emulate_gelu(inp["g32"])
    if case.mode == "geglu":
        v = inp["h32"] * v
    hi = v.to(torch.float16)
    if case.split_out:
        return hi.double() + (v - hi.float()).to(torch.float16).double()
    return hi


def epilogue_gates():
    """Every fp32 gate of the gelu-form fused-epilogue cases (E_ERF is measured over them), one float32 array."""
    return np.concatenate([make_epilogue_input(n)["g32"].numpy().ravel() for n, c in EPI_CASES.items() if c.mode != "quick_gelu"])


def overflow_split(ref, tol):
    """(compare, must_be_inf): elements whose reference stays below fp16's overflow threshold with the bound to spare / passes it with the bound to
    spare; the few in between may be either."""
    return ref.abs() + tol < F16_MAX_ROUND, ref.abs() - tol >= F16_MAX_ROUND


def ratio(got, ref, tol, mask=None):
    r = (got.double() - ref).abs() / tol
    if mask is not None:
        r = torch.where(mask, r, torch.zeros_like(r))
    return torch.nan_to_num(r, nan=float("inf")).max().item()


def _measure():
    w16, at16 = erf_error(all_fp16().float().numpy())
    w32, at32 = erf_error(epilogue_gates())
    print(f"[erf] worst |1 + erf_as - erfc| of the emulation: {w16:.3e} over the fp16 gates (g = {at16:.4f}), {w32:.3e} over the fp32 gates (g = {at32:.4f}); "
          f"E_ERF = 2 x {max(w16, w32):.3e} = {2 * max(w16, w32):.3e}")
    g = all_fp16().float()
    ge = (emulate_gelu(g).double() - gelu64(g)).abs()
    i = int(ge.argmax())
    print(f"[erf] worst |gelu_erf - gelu| of the emulation: {ge[i].item():.3e} at g = {g[i].item():.4f}")
    neg = g[(g < 0) & (emulate_gelu(g) == 0) & (g > -1e4)]
    print(f"[erf] gelu_erf returns -0 for every gate below {neg.max().item():.3f} (true value {gelu64(neg.max()).item():.2e})")
    wa, _ = erf_error(all_fp16().float().numpy(), A5_SIXTH_DIGIT)
    print(f"[erf] with a5 changed in its sixth digit: {wa:.3e}")


if __name__ == "__main__":
    _measure()
