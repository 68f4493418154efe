"""Bit-exact forward cases for the diffusion path's contraction kernels (ldiff_op_conv): case table, operand builders, the epilogue rule emulator.
No GPU import: tests/test_cpu_conv_exact.py checks the builders' conditions, tests/test_gpu_conv_exact.py launches the cases.

Regime E (exact).  The MFMA operands are small integers in fp16 (behind a GroupNorm prologue: x, scale = 2^j and an integer shift chosen so that the
normalised operand is an integer; with SiLU an alphabet on which fp16(silu(a)) is 0 or a itself, far from a rounding boundary); bias, time embedding and
residual hi / lo are multiples of 2^-6 (integers where statistics are fused).  Sum + bias + temb, its product with 2^-out_shift and the sums with the residual
are then representable in fp32 in ANY order, so the float64 value v is what every kernel's fp32 pipeline holds, and the stored bits follow:
    fp32 output: v        plain fp16 output: rne16(v)        split output: hi = rne16(v), lo = rne16(v - hi)
with one declared exception, conv3x3<16x16d> with a residual: rne16(rne16(v) + res), its packed-fp16 add (kernels_conv3x3d.hip, store_unit).

Regime R (rounding order).  Integer MFMA operands (so the accumulator is exact), bias / temb / residual with random mantissas, and a numpy float32 emulation
of the kernel's own order of additions, read from its source:
    halo  conv3x3<8x8|8x16,...> (kernels_conv3x3.hip):        ((acc + (bias + temb)) * 2^-k + res_hi) + res_lo
    gemm  gemm_dma (kernels_gemm.hip), gemm_df (..._df.hip):   ((acc + bias) * 2^-k + res_hi) + res_lo                  (no time embedding)
    igemm igemm (kernels_igemm.hip, epilogue.h):               ((((acc + bias) + temb) * 2^-k) + res_hi) + res_lo
    reduce splitk_reduce[_stats] (kernels_conv3x3.hip):        as igemm, acc = the (exact) sum of the partials
Multiplying by 2^-k is exact, so a contraction of `* 2^-k + res` into an fma cannot change a bit.  conv3x3p / conv3x3d / conv3x3n / conv3x3nt are regime E
only: p and d start their accumulators at bias + temb (and p adds the residual in the middle of the MFMA chain), so the rounding of an inexact C + sum is
the matrix unit's; n / nt add the bias behind sums that the tap fold re-associates in fp32.
"""
import functools
import types
import zlib

import numpy as np
import torch
import torch.nn.functional as F

SENTINEL16 = 0x5A5A          # bit pattern the outputs are pre-filled with (fp16 210.25; fp32 0x5A5A5A5A)
CANARY_ROWS = 4              # rows behind M that must stay untouched
PAD_COLS = 8                 # columns behind the stored ones (ldy = stored + 8) that must stay untouched

_DEFAULTS = dict(C2=0, ks=3, stride=1, asym=False, ups=0, c3d_ups=0, gn=None, opsplit=False, pitch=False, temb=False, res=None, out="f16", stats=False,
                 splitk=0, short_runs=0, out_shift=0, sc=0, sc_pitch=0, gemm_df=0, n_real=0, regimes="E", r_out=None, r_shift=0, epi=None)

# name: kernel the launch must reach, B, C1, H, W, N (stored columns) and the options.  n_real: the layer's output channels where N rounds them up (the weight
# rows and the bias behind them are zero: those columns hold the other addends alone).  gn: None | "affine" (silu_in = 0) | "silu"; res: None | "plain" | "split";
# out: "f16" | "split" | "f32"; opsplit: split operand (hi | lo, both read, weights through ldiff_op_dup_weights); pitch: plain operand read through
# ld = 2 C (the unread lo half holds large integers); epi: whose order of additions regime R emulates (halo | gemm | igemm | reduce); r_out / r_shift:
# the output form and range shift of the regime-R launch (fp32 where the kernel has it: an fp16 store hides the last fp32 bit; an explicit split count
# needs an fp16 output, and gemm_df has no fp32 one: split there).
# A 3x3 launch of two or more slabs without statistics, fp32 output or parity folding is split by the planner at these sizes (conv3x3_splitk_plan): its
# epilogue is then the reduce kernel's.  The halo kernels' own fp16 epilogue is pinned by the one-slab, the parity and the statistics cases and by two
# cases whose grids are large enough (256 workgroups) to stay unsplit.
CASES = {
    # ---- halo-tile kernels, 8x16 tiles (maps at least 16 wide) ----
    "w32_ragged_12x27_cout18_of_20": dict(kernel="conv3x3<8x16,32>", B=1, C1=64, H=12, W=27, N=20, n_real=18, temb=True, res="plain", regimes="ER", epi="halo", r_out="f32", r_shift=4),
    "w32_gn_affine_stats_split": dict(kernel="conv3x3<8x16,32,gn>", B=2, C1=128, H=16, W=20, N=32, gn="affine", res="split", out="split", stats=True),
    "w64_upsample_odd_9x19": dict(kernel="conv3x3<8x16,64>", B=2, C1=128, H=9, W=19, N=64, ups=1, temb=True),
    "w64_gn_silu_concat_128_64_pitch_stats": dict(kernel="conv3x3<8x16,64,gn>", B=1, C1=128, C2=64, H=16, W=16, N=64, gn="silu", pitch=True, stats=True),
    "w128_split_operand_ragged_20x27_shift4": dict(kernel="conv3x3<8x16,128>", B=2, C1=64, H=20, W=27, N=128, opsplit=True, res="split", out="split", out_shift=4),
    "w128_gn_silu_5slabs_splitk3_stats": dict(kernel="conv3x3<8x16,128,gn>", B=1, C1=320, H=16, W=16, N=96, gn="silu", temb=True, res="split", out="split", stats=True,
                                              splitk=3),
    # 2 x 8 x 8 tiles x 2 channel tiles = 256 workgroups: the planner leaves the two slabs unsplit, so this is the kernel's own fp16 hi | lo store
    "w128_two_slabs_unsplit_ragged_60x124": dict(kernel="conv3x3<8x16,128>", B=2, C1=128, H=60, W=124, N=256, temb=True, res="split", out="split", regimes="ER", epi="halo",
                                                 r_out="split", r_shift=4),
    "w160_ragged_17x33_f32": dict(kernel="conv3x3<8x16,160>", B=1, C1=128, H=17, W=33, N=160, res="plain", temb=True, out="f32", regimes="ER", epi="halo", r_out="f32"),
    "w160_gn_affine_320_stats": dict(kernel="conv3x3<8x16,160,gn>", B=2, C1=128, H=8, W=16, N=320, gn="affine", stats=True),
    # ---- halo-tile kernels, 8x8 tiles (maps narrower than 16) ----
    "s32_1x1_spatial": dict(kernel="conv3x3<8x8,32>", B=3, C1=64, H=1, W=1, N=32, temb=True, res="plain", regimes="ER", epi="halo", r_out="f32", r_shift=4),
    "s32_gn_silu_ragged_12x12_cout22_of_24_stats": dict(kernel="conv3x3<8x8,32,gn>", B=2, C1=64, H=12, W=12, N=24, n_real=22, gn="silu", stats=True),
    "s64_upsample_odd_5x7": dict(kernel="conv3x3<8x8,64>", B=2, C1=128, H=5, W=7, N=64, ups=1, res="plain"),
    "s64_gn_affine_ragged_10x14_f32": dict(kernel="conv3x3<8x8,64,gn>", B=1, C1=128, H=10, W=14, N=64, gn="affine", res="plain", out="f32"),
    "s128_16slabs_splitk16": dict(kernel="conv3x3<8x8,128>", B=1, C1=1024, H=8, W=8, N=128, temb=True, res="plain", splitk=16, regimes="ER", epi="reduce", r_out="split"),
    "s128_two_slabs_unsplit_ragged_12x12": dict(kernel="conv3x3<8x8,128>", B=16, C1=128, H=12, W=12, N=512, res="plain"),      # 16 x 4 tiles x 4 channel tiles: unsplit
    "s128_gn_silu_pitch_split_stats": dict(kernel="conv3x3<8x8,128,gn>", B=2, C1=128, H=8, W=12, N=128, gn="silu", pitch=True, res="split", out="split", stats=True),
    "s160_one_slab_shift4": dict(kernel="conv3x3<8x8,160>", B=2, C1=64, H=8, W=8, N=160, res="plain", out_shift=4),
    "s160_gn_silu_320_ragged_12x10_stats": dict(kernel="conv3x3<8x8,160,gn>", B=1, C1=128, H=12, W=10, N=320, gn="silu", out="split", stats=True),
    # ---- narrow-output kernels (4 stored columns) ----
    "n4_concat_128_64_ragged_24x40_f32": dict(kernel="conv3x3<8x16,n4>", B=2, C1=128, C2=64, H=24, W=40, N=4, n_real=4, out="f32"),
    # (fp16 output: 4 x 8 x 8 = 256 tiles, so that the planner leaves the three slabs unsplit -- a split launch is not the narrow kernel's)
    "n4_gn_silu_192_ragged_60x124_f16": dict(kernel="conv3x3<8x16,n4,gn>", B=4, C1=192, H=60, W=124, N=4, n_real=4, gn="silu"),
    "n3fold_ragged_20x27_f32": dict(kernel="conv3x3<8x16,n3fold>", B=2, C1=128, H=20, W=27, N=4, n_real=3, out="f32"),
    "n3fold_gn_silu_cout2_f32": dict(kernel="conv3x3<8x16,n3fold,gn>", B=1, C1=128, H=8, W=16, N=4, n_real=2, gn="silu", out="f32"),
    # ---- dataflow kernel (the grid has to fill the chip: 256 units) ----
    "d_gn_256x256_temb_res": dict(kernel="conv3x3<16x16d,128,gn>", B=1, C1=64, H=256, W=256, N=128, gn="silu", temb=True, res="plain"),
    "d_gn_two_units_per_workgroup_shift4_temb_res": dict(kernel="conv3x3<16x16d,128,gn>", B=2, C1=64, H=256, W=256, N=128, gn="silu", temb=True, res="plain", out_shift=4),
    "d_gn_two_slabs_shortcut_pitch_stats_short_runs": dict(kernel="conv3x3<16x16d,128,gn>", B=1, C1=128, H=256, W=256, N=128, gn="silu", sc=64, sc_pitch=128, stats=True,
                                                           short_runs=1),
    "d_ups_128x128_stats": dict(kernel="conv3x3<16x16d,128,ups>", B=1, C1=64, H=128, W=128, N=128, ups=1, c3d_ups=1, stats=True),
    # ---- 16x16 ping-pong kernel (tile lists that fill the chip: 8 x 5 x 6 = 240 tiles of the ragged 72 x 88 map) ----
    "p64_concat_ragged_72x88_two_tiles_per_workgroup_res_stats": dict(kernel="conv3x3<16x16,64>", B=16, C1=64, C2=64, H=72, W=88, N=64, res="plain", stats=True),
    "p128_split_operand_ragged_72x88_shift4_short_runs": dict(kernel="conv3x3<16x16,128>", B=8, C1=32, H=72, W=88, N=128, opsplit=True, temb=True, res="split", out="split",
                                                              out_shift=4, short_runs=1),
    "p128_two_slabs_ragged_72x88_split_stats": dict(kernel="conv3x3<16x16,128>", B=8, C1=128, H=72, W=88, N=128, res="split", out="split", stats=True),
    "p128_upsample_ragged_56x72": dict(kernel="conv3x3<16x16,128>", B=3, C1=64, H=56, W=72, N=128, ups=1),
    # ---- LDS-DMA GEMM ----
    "g64_concat_128_64_pitch_tail_rows": dict(kernel="gemm_dma<64,64>", ks=1, B=1, C1=128, C2=64, H=1, W=300, N=320, pitch=True, res="split", out="split", regimes="ER",
                                              epi="gemm", r_out="f32", r_shift=4),
    "g64_10steps_splitk3_stats": dict(kernel="gemm_dma<64,64>", ks=1, B=2, C1=640, H=16, W=16, N=256, res="plain", stats=True, splitk=3, regimes="ER", epi="reduce", r_out="split", r_shift=4),
    "g64_40steps_splitk7": dict(kernel="gemm_dma<64,64>", ks=1, B=2, C1=1280, C2=1280, H=8, W=8, N=128, out="split", splitk=7, regimes="ER", epi="reduce", r_out="split", r_shift=4),
    "g128x64_stats": dict(kernel="gemm_dma<128,64>", ks=1, B=3, C1=64, H=32, W=32, N=1024, stats=True),
    "g128x128_split_operand": dict(kernel="gemm_dma<128,128>", ks=1, B=1, C1=64, H=1, W=3072, N=2048, opsplit=True, res="plain", out="split"),
    # ---- dataflow GEMM, plain epilogues (forced unit shapes: 16 mt + ntw) ----
    "df_mt4_concat_tail_rows_tail_columns": dict(kernel="gemm_df", ks=1, B=1, C1=128, C2=64, H=1, W=1000, N=200, res="split", out="split", gemm_df=16 * 4 + 2, regimes="ER",
                                                 epi="gemm", r_out="split", r_shift=4),
    "df_mt8_stats_res": dict(kernel="gemm_df", ks=1, B=2, C1=64, H=32, W=32, N=320, res="plain", stats=True, gemm_df=16 * 8 + 5),
    "df_mt8_shift4": dict(kernel="gemm_df", ks=1, B=1, C1=128, H=1, W=2048, N=320, res="plain", out_shift=4, gemm_df=16 * 8 + 5),
    # ---- register-staged implicit GEMM ----
    "i128x128_gen_c32_split": dict(kernel="igemm<128,128,gen>", ks=1, B=1, C1=32, H=96, W=256, N=256, temb=True, res="split", out="split"),
    "i128x128_gen_gn_affine_c96_stats": dict(kernel="igemm<128,128,gen,gn>", ks=1, B=1, C1=96, H=96, W=256, N=256, gn="affine", stats=True),
    "i128x128_fast_temb_res_shift4": dict(kernel="igemm<128,128,fast>", ks=1, B=1, C1=64, H=96, W=256, N=256, temb=True, res="plain", out_shift=4, regimes="ER", epi="igemm",
                                          r_out="f32", r_shift=4),
    "i128x128_fast_gn_silu_c128": dict(kernel="igemm<128,128,fast,gn>", ks=1, B=1, C1=128, H=96, W=256, N=256, gn="silu", temb=True),
    "i128x64_gen_c40_f32": dict(kernel="igemm<128,64,gen>", ks=1, B=1, C1=40, H=192, W=256, N=64, temb=True, out="f32"),
    "i128x64_gen_gn_silu_c96": dict(kernel="igemm<128,64,gen,gn>", ks=1, B=1, C1=96, H=192, W=256, N=64, gn="silu", res="plain"),
    "i128x64_fast_concat_temb_stats": dict(kernel="igemm<128,64,fast>", ks=1, B=2, C1=64, C2=64, H=96, W=256, N=64, temb=True, stats=True),
    "i128x64_fast_gn_affine_split": dict(kernel="igemm<128,64,fast,gn>", ks=1, B=1, C1=64, H=192, W=256, N=64, gn="affine", res="split", out="split"),
    "i64_gen_c8_3x3_ragged_12x10": dict(kernel="igemm<64,64,gen>", B=2, C1=8, H=12, W=10, N=40, temb=True, res="plain", regimes="ER", epi="igemm", r_out="f32"),
    "i64_gen_gn_affine_stride2_asym_vae": dict(kernel="igemm<64,64,gen,gn>", B=2, C1=32, H=16, W=16, N=32, stride=2, asym=True, gn="affine", res="plain"),
    "i64_fast_stride2_split_operand_splitk5": dict(kernel="igemm<64,64,fast>", B=2, C1=64, H=16, W=16, N=64, stride=2, opsplit=True, temb=True, res="split", out="split",
                                                   splitk=5),
    "i64_fast_gn_silu_stride2_odd_15x15_stats": dict(kernel="igemm<64,64,fast,gn>", B=2, C1=128, H=15, W=15, N=64, stride=2, gn="silu", stats=True),
}

# what is left out of this table, and who owns it
EXCLUDED = {
    "gemm_df<geglu>": "GEGLU and act_out epilogues are not exact arithmetic: tests/transformer_bound.py",
    "lngemm<320>": "LayerNorm prologue: tests/transformer_bound.py",
    "lngemm<320,geglu>": "LayerNorm prologue, GEGLU: tests/transformer_bound.py",
}
EXACT_LAUNCHERS = ("launch_conv3x3n", "launch_conv3x3d", "launch_conv3x3p", "launch_conv3x3", "launch_gemm_dma", "launch_gemm_df", "launch_igemm")

SILU_POS = np.array([16, 20, 24, 28, 32, 40, 48], dtype=np.float64)
SILU_NEG = np.array([-32, -40, -48, -64], dtype=np.float64)


def case(name):
    c = types.SimpleNamespace(**{**_DEFAULTS, **CASES[name]}, name=name)
    c.Cin = c.C1 + c.C2
    He, We = c.H << c.ups, c.W << c.ups
    p = c.ks // 2
    c.pads = (0, 1, 0, 1) if c.asym else (p, p, p, p)          # top, bottom, left, right
    c.Ho = (He + c.pads[0] + c.pads[1] - c.ks) // c.stride + 1
    c.Wo = (We + c.pads[2] + c.pads[3] - c.ks) // c.stride + 1
    c.M = c.B * c.Ho * c.Wo
    c.K = c.ks * c.ks * c.Cin + c.sc
    c.K_seen = min(c.ks, He) * min(c.ks, We) * c.Cin + c.sc      # terms of a sum that are not padding, at most (the amplitudes follow it)
    assert not (c.opsplit and (c.gn or c.pitch)) and not (c.stats and c.out_shift) and not (c.stats and c.out == "f32")
    return c


def regime_case(name, regime):
    """The launch of `regime`: E as the table says; R with the table's r_out / r_shift (statistics stay on, so that the same kernel instantiation runs)."""
    c = case(name)
    assert regime in c.regimes
    if regime == "R":
        c.out, c.out_shift = c.r_out, c.r_shift
    return c


def silu64(a):
    return a / (1.0 + np.exp(-a))


def rne16(v):
    return np.asarray(v).astype(np.float16)


def rtz16(v):
    """float -> fp16 rounded toward zero (what v_cvt_pkrtz does): the wrong rule the inputs must be able to show"""
    v = np.asarray(v, dtype=np.float64)
    h = v.astype(np.float16)
    over = np.abs(h.astype(np.float64)) > np.abs(v)
    return np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float16)


def _amplitude(K, rms_a, target, at_most):
    """weight alphabet [-a, a]: the smallest a whose predicted output deviation sqrt(K) rms_a sigma_w reaches `target`, or (statistics) the largest below it"""
    best = 1
    for a in range(1, 513):
        s = np.sqrt(K) * rms_a * np.sqrt(a * (a + 1) / 3.0)
        if at_most:
            if s <= target:
                best = a
        elif s >= target:
            return a
    return best if at_most else 512


@functools.lru_cache(maxsize=2)
def integer_part(name):
    """The operands of the MFMAs and their exact contraction, shared by both regimes: numpy arrays (NHWC) on a namespace."""
    c = case(name)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    o = types.SimpleNamespace()
    shape = (c.B, c.H, c.W, c.Cin)
    target = 60.0 if c.stats else 4000.0 * 2.0 ** c.out_shift
    if c.gn == "silu":
        p_pos, p_neg = (0.04, 0.10) if c.stats else (0.5, 0.2)
        u = rng.random(shape)
        a = np.where(u < p_pos, rng.choice(SILU_POS, shape), np.where(u < p_pos + p_neg, rng.choice(SILU_NEG, shape), 0.0))
        rms_a = float(np.sqrt(p_pos * np.mean(SILU_POS ** 2)))
        aw = _amplitude(c.K_seen, rms_a, target, c.stats)
    else:
        ax = 1 if c.stats else _amplitude(c.K_seen, 1.0, np.sqrt(target * np.sqrt(c.K_seen)), False)   # both factors from [-a, a]: sigma_x sigma_w sqrt(K) ~ target
        rms_a = np.sqrt(ax * (ax + 1) / 3.0)
        aw = _amplitude(c.K_seen, rms_a, target, c.stats)
        a = rng.integers(-ax, ax + 1, shape).astype(np.float64)
    o.x_lo = None
    if c.gn:
        j = rng.integers(-1, 2, (c.B, c.Cin))
        o.scale = (2.0 ** j).astype(np.float32)
        o.shift = (rng.integers(-3, 4, (c.B, c.Cin)) * 2).astype(np.float32)
        if c.gn == "affine":   # an integer x with x * 2^j + shift = a: a even where x would be a half
            a = a - np.where(j[:, None, None, :] == 1, np.mod(a, 2), 0.0)
        x = (a - o.shift[:, None, None, :]) / o.scale[:, None, None, :].astype(np.float64)
        pre = x * o.scale[:, None, None, :].astype(np.float64) + o.shift[:, None, None, :]
        assert np.array_equal(pre, a) and np.array_equal(x.astype(np.float16).astype(np.float64), x)
        if c.gn == "silu":
            s = silu64(a)
            a_eff = rne16(s).astype(np.float64)
            # fp16(silu(a)) is 0 or a, and silu(a) sits within 1e-3 of half an fp16 spacing of it: a 1-ulp v_exp / v_rcp cannot move the rounding
            half = np.where(a_eff == 0, 2.0 ** -25, np.spacing(np.abs(a_eff).astype(np.float16)).astype(np.float64) / 2)
            assert np.all((a_eff == 0) | (a_eff == a)) and np.all(np.abs(s - a_eff) <= 1e-3 * half)
        else:
            a_eff = a
        o.x_hi = x
    elif c.opsplit:   # hi and lo drawn independently (to_split of an integer has lo = 0 and tests nothing)
        ax = max(1, int(np.abs(a).max()))
        o.x_hi = a
        o.x_lo = rng.integers(-(ax // 2 + 1), ax // 2 + 2, shape).astype(np.float64)
        a_eff = o.x_hi + o.x_lo
    else:
        o.x_hi, a_eff = a, a
    if c.pitch:   # the half of each row that must NOT be read: large, so that a stray read is seen
        o.x_lo = rng.integers(500, 2000, shape).astype(np.float64) * rng.choice([-1.0, 1.0], shape)
    o.w = rng.integers(-aw, aw + 1, (c.N, c.ks, c.ks, c.Cin)).astype(np.float64)
    if c.stats:   # a long K beside fused statistics: sparse weights keep sum y^2 of a partial below 2^24 where [-1, 1] alone does not
        full = np.sqrt(c.K_seen) * rms_a * np.sqrt(aw * (aw + 1) / 3.0)
        if full > target:
            o.w *= rng.random(o.w.shape) < (target / full) ** 2
    if c.n_real:
        o.w[c.n_real:] = 0.0
    up = a_eff.repeat(2, 1).repeat(2, 2) if c.ups else a_eff
    t, b, l, r = c.pads
    o.a_pad = np.pad(up, ((0, 0), (t, b), (l, r), (0, 0)))
    o.a_eff = a_eff
    with torch.no_grad():
        acc = F.conv2d(torch.from_numpy(o.a_pad).permute(0, 3, 1, 2), torch.from_numpy(o.w).permute(0, 3, 1, 2), stride=c.stride)
    o.acc = acc.permute(0, 2, 3, 1).contiguous().numpy()
    assert o.acc.shape == (c.B, c.Ho, c.Wo, c.N)
    bound = c.ks * c.ks * c.Cin * np.abs(a_eff).max() * np.abs(o.w).max()
    if c.ups:   # parity folding pre-sums up to four taps: the sums must be fp16 integers
        assert 4 * aw <= 2048
    if c.sc:
        o.sc_x = rng.integers(-1, 2, (c.B, c.H, c.W, c.sc_pitch or c.sc)).astype(np.float64)
        o.sc_x[..., c.sc:] = rng.integers(500, 2000, o.sc_x[..., c.sc:].shape)      # (behind the pitch: unread)
        o.sc_w = rng.integers(-aw, aw + 1, (c.N, c.sc)).astype(np.float64)
        o.acc = o.acc + o.sc_x[..., :c.sc] @ o.sc_w.T
        bound += c.sc * np.abs(o.sc_w).max()
    assert bound < 2 ** 24, f"{name}: a partial sum can reach {bound:.0f} >= 2^24"      # |sum| < 2^24 at EVERY partial sum, whatever the order
    o.aw = aw
    return o


def build(name, regime):
    """Operands of one launch.  Returns (case, o): o has x_hi, x_lo, w, acc, scale, shift, bias, sc_bias, temb, res_hi, res_lo (None where absent)."""
    c = regime_case(name, regime)
    ip = integer_part(name)
    o = types.SimpleNamespace(**vars(ip))
    rng = np.random.default_rng(zlib.crc32((name + regime).encode()))
    shp = (c.B, c.Ho, c.Wo, c.N)
    o.sc_bias = o.temb = o.res_hi = o.res_lo = None
    if regime == "E":
        q = 1.0 if c.stats else 64.0        # integers beside fused statistics (y^2 must be exact), else multiples of 2^-6
        qa = q / 2.0 ** c.out_shift if not c.stats else q      # the addends in front of the range shift: multiples of 2^(k - 6), of 2^-6 behind it
        o.bias = (rng.integers(-8 * q, 8 * q + 1, c.N) / qa).astype(np.float32)
        if c.sc:
            o.sc_bias = (rng.integers(-8 * q, 8 * q + 1, c.N) / qa).astype(np.float32)
        if c.temb:
            o.temb = (rng.integers(-8 * q, 8 * q + 1, (c.B, c.N)) / qa).astype(np.float32)
        if c.res:
            o.res_hi = ((rng.integers(-64, 65, shp) if c.stats else rng.integers(-2047, 2048, shp)) / q).astype(np.float16)
            if c.res == "split":
                o.res_lo = ((rng.integers(-4, 5, shp) if c.stats else rng.integers(-31, 32, shp)) / q).astype(np.float16)
    else:
        o.bias = (rng.standard_normal(c.N) * 8).astype(np.float32)
        if c.temb:
            o.temb = (rng.standard_normal((c.B, c.N)) * 8).astype(np.float32)
        if c.res:
            o.res_hi = (rng.standard_normal(shp) * 300).astype(np.float16)
            if c.res == "split":
                o.res_lo = (rng.standard_normal(shp) * 0.1).astype(np.float16)
    if c.n_real:
        o.bias[c.n_real:] = 0.0
    return c, o


def _f(dt, a):
    return None if a is None else np.asarray(a).astype(dt)


def value(c, o, regime, rule=None, acc=None):
    """v, the fp32 value in front of the store, [B, Ho, Wo, N]: float64 in regime E (any order gives it), float32 in the kernel's order in regime R.
    rule: None = the kernel's, or one of the WRONG rules the inputs must discriminate (test_cpu_conv_exact.py)."""
    dt = np.float64 if regime == "E" else np.float32
    acc = _f(dt, o.acc if acc is None else acc)
    bias = _f(dt, o.bias)
    if o.sc_bias is not None:
        bias = bias + _f(dt, o.sc_bias)
    temb = None if o.temb is None else _f(dt, o.temb)[:, None, None, :]
    order = c.epi or "igemm"
    if rule == "addend_order_swapped":
        order = {"halo": "igemm", "igemm": "halo", "reduce": "halo"}[order]
    if temb is None:
        s = acc + bias
    elif order == "halo":
        s = acc + (bias + temb)
    else:
        s = (acc + bias) + temb
    osc = dt(2.0 ** -c.out_shift)
    rh, rl = _f(dt, o.res_hi), _f(dt, o.res_lo)
    if rule == "lo_dropped":
        rl = None
    if rule == "res_before_shift":
        if rh is not None:
            s = s + rh
        if rl is not None:
            s = s + rl
        return s * osc
    v = s * osc
    if rule == "round_before_res" or (rule is None and c.kernel.startswith("conv3x3<16x16d") and rh is not None):
        v = _f(dt, rne16(v))
    if rh is not None:
        v = v + rh
    if rl is not None:
        v = v + rl
    return v


def expected(c, o, regime, rule=None, acc=None):
    """The bits the launch must store: dict(f32= | hi=, lo=) and, with fused statistics in regime E, stats [B, N, 2] float64 totals."""
    v = value(c, o, regime, rule, acc)
    cvt = rtz16 if rule == "rtz" else rne16
    out = {}
    if c.out == "f32":
        out["f32"] = v.astype(np.float32)
        return out
    hi = cvt(v)
    out["hi"] = hi
    if c.out == "split":
        lo = cvt(v.astype(np.float32) - hi.astype(np.float32))
        out["lo"] = np.zeros_like(lo) if rule == "lo_dropped" else lo
    if c.stats and regime == "E":
        op = v if c.out == "split" else hi.astype(np.float64)
        tot = np.stack([op.sum((1, 2)), (op * op).sum((1, 2))], -1)            # [B, N, 2]
        if rule == "stats_extra_pixel":
            b = o.bias.astype(np.float64) + (0 if o.sc_bias is None else o.sc_bias.astype(np.float64))
            tot = tot + np.stack([b, b * b], -1)[None]
        out["stats"] = tot
        out["stat_operand"] = op
    return out


def check_exact_conditions(c, o):
    """Regime E: the conditions under which float64 is what every fp32 pipeline holds, and under which the case exercises the roundings."""
    v = value(c, o, "E")
    for t in (o.acc, o.acc + o.bias.astype(np.float64), v * 2.0 ** c.out_shift, v):
        assert np.array_equal(t.astype(np.float32).astype(np.float64), t), f"{c.name}: a value of the pipeline is not an fp32"
    if o.temb is not None:
        t = o.acc + o.temb.astype(np.float64)[:, None, None, :]
        assert np.array_equal(t.astype(np.float32).astype(np.float64), t)
    real = v[..., :c.n_real] if c.n_real else v
    assert np.abs(v).max() < 60000, f"{c.name}: |v| reaches {np.abs(v).max():.0f}"
    if not c.stats:
        big = float((np.abs(real) > 2048).mean())
        assert big >= 0.10, f"{c.name}: only {big:.3f} of the outputs are above 2048"
    else:
        e = expected(c, o, "E")
        op = e["stat_operand"]
        assert np.abs(op).max() <= 2048 and np.array_equal(op, np.round(op))
        sq = np.sort((op * op).reshape(c.B, -1, c.N), axis=1)[:, -256:, :].sum(1)      # any partial of at most 256 pixels
        assert sq.max() < 2 ** 24, f"{c.name}: a statistics partial can reach {sq.max():.0f}"
        assert np.abs(e["stats"]).max() < 2 ** 53


def element_count(c):
    n = c.M * (c.n_real or c.N)
    return n * (2 if c.out == "split" else 1)


# ---- wrong rules that change the operands (test_cpu_conv_exact.py) ----
def acc_with_one_weight_zeroed(c, o):
    """(acc', n0): one (tap, channel) element of output channel n0's weights zeroed"""
    n0 = (c.n_real or c.N) // 2
    nz = np.argwhere(o.w[n0] != 0)
    ky, kx, c0 = nz[len(nz) // 2]
    acc = o.acc.copy()
    s = c.stride
    acc[..., n0] -= o.w[n0, ky, kx, c0] * o.a_pad[:, ky:ky + (c.Ho - 1) * s + 1:s, kx:kx + (c.Wo - 1) * s + 1:s, c0]
    return acc, n0


def acc_with_neighbour_halo(c, o):
    """(acc', (oy, ox)) with the out-of-image taps of ONE border pixel of image 0 read from the nearest pixel inside instead of zero; None without such a tap"""
    t, b, l, r = c.pads
    Hp, Wp = o.a_pad.shape[1:3]
    for oy, ox in ((0, 0), (c.Ho - 1, c.Wo - 1)):
        delta = np.zeros(c.N)
        hit = False
        for ky in range(c.ks):
            for kx in range(c.ks):
                iy, ix = oy * c.stride + ky, ox * c.stride + kx
                cy, cx = min(max(iy, t), Hp - b - 1), min(max(ix, l), Wp - r - 1)
                if (cy, cx) != (iy, ix):
                    hit = True
                    delta += o.w[:, ky, kx, :] @ o.a_pad[0, cy, cx, :]
        if hit:
            acc = o.acc.copy()
            acc[0, oy, ox, :] += delta
            return acc, (oy, ox)
    return None
