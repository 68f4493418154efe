"""-m gpu: the inference-time GroupNorm path against float64 with the derived bounds of tests/groupnorm_bound.py (judged on the CPU by
tests/test_cpu_groupnorm_bound.py): the separate statistics pass in both of its forms, the statistics the conv / GEMM epilogues emit (the
sums, and scale / shift behind ldiff_op_gn_finalize), and GroupNorm folded into a 1x1 conv's per-image weights (ldiff_conv_args.fold_gn).
Every case states the kernel it is meant for and fails if the library routes it elsewhere (profiler rows: gn_stats<1> / gn_stats<2>,
fold_gn_weights, the conv / GEMM names of tests/kernel_routing.py), and every case's bound also rejects that case's wrong references.

MEASURED (MI355X)
    Section 1, error / bound (error over u amp, the quantity C_STATS = 23 is four times the emulation's worst 5.72 of):
        small_c640_cg20_hw1024 0.052 (0.000), small_concat_1280_640_hw256 0.051 (0.000), small_c2560_hw4096 0.348 (5.524), small_hw1 0.027 (0.148),
        small_c32_cg1 0.033 (0.000), small_split 0.037 (0.000), small_pitched 0.052 (0.000), small_eps6_affine 0.079 (0.000), small_ratio8 0.026
        (0.531), small_ratio30_hw64 0.006 (0.143), small_const_group 0.052 (0.000), small_var_eps 0.031 (0.000), two_c128_hw2048 0.038 (0.000),
        two_c320_hw4160 0.035 (0.000), two_c320_hw4150_ragged 0.035 (0.000), two_concat_128_64_hw2048 0.044 (0.000), two_c64_hw33000_pix64 0.028
        (0.000), two_split 0.035 (0.019), two_pitched 0.038 (0.000), two_eps6_affine 0.061 (0.000), two_ratio8 0.016 (0.291), two_const_group 0.038
        (0.000), two_var_eps 0.024 (0.000)
    Section 2, sum / sum of squares / scale-shift, each as a fraction of its bound:
        halo_8x16 0.0000 / 0.0036 / 0.010, halo_8x8 0.0000 / 0.0282 / 0.019, pingpong_256x256 0.0000 / 0.0015 / 0.008, pingpong_lo8 0.0009 / 0.0011
        / 0.005, dataflow_gn 0.0000 / 0.0061 / 0.026, dataflow_ups 0.0000 / 0.0055 / 0.020, gemm_dma 0.0000 / 0.0181 / 0.009, gemm_df 0.0000 /
        0.0081 / 0.008, igemm_stride2 0.0000 / 0.0146 / 0.015, halo_parity_upsample 0.0000 / 0.0030 / 0.012, splitk4_3x3 0.0000 / 0.0413 / 0.029,
        splitk3_1x1 0.0000 / 0.0286 / 0.017, splitk2_igemm 0.0000 / 0.0240 / 0.024, halo_8x16_split_out 0.0030 / 0.0029 / 0.012, halo_8x16_n64
        0.0000 / 0.0040 / 0.014, gemm_dma_var_eps 0.0000 / 0.0105 / 0.006, two sources 128 + 64: scale / shift 0.012 of the bound
    Section 3, error / bound (max error / max|ref|):
        vae_qkv_smallest_map 0.195 (4.21e-04), hw192_three_images 0.291 (4.45e-04), hw192_tile_rule 0.325 (4.62e-04), c1280_second_trip 0.133
        (4.38e-04), nrows_322 0.218 (3.49e-04), null_bias 0.244 (3.84e-04), hw128_tiles_128 0.335 (3.90e-04), hw48_declined 0.227 (3.94e-04)
    Section 3, operand regimes on the VAE q/k/v shape, max error / max|ref| (the table of DESIGN.md section 4):
        mean0.3 unfolded 4.57e-04 folded 4.21e-04 emulated 4.21e-04 | of the bounds 0.213 / 0.195
        mean3 unfolded 4.33e-04 folded 6.84e-04 emulated 6.84e-04 | of the bounds 0.198 / 0.103
        mean10 unfolded 4.49e-04 folded 1.80e-03 emulated 1.80e-03 | of the bounds 0.208 / 0.086
        std1 unfolded 4.15e-04 folded 3.94e-04 emulated 3.94e-04 | of the bounds 0.213 / 0.205
        std1024 unfolded 4.12e-04 folded 4.18e-04 emulated 4.18e-04 | of the bounds 0.212 / 0.138
        std4096 unfolded 4.12e-04 folded 6.25e-04 emulated 6.25e-04 | of the bounds 0.212 / 0.117
    The kernels' figures equal those of the CPU emulations (tests/test_cpu_groupnorm_bound.py, same seeds) to the digits shown.

Deliberate defects, each built into the library once and reverted (old = the statistics / fold coverage the suite had before this file):
    the last 32-row block's statistics store skipped in gemm_dma's epilogue: old tests fail too (their NaN-filled buffers, and the bit-for-bit
        comparison with gemm_df); here test_fused_statistics_against_float64[gemm_dma, gemm_dma_var_eps];
    image 0's folded weights for every tile (kernels_gemm.hip, img = 0): old tests fail only at model level (VAE encode / decode and sampler parity,
        the shifted decoders); here every folded case and regime with B > 1 (12 tests);
    the scalar tail loop of gn_partial_kernel dropped: ONE old case fails (test_group_norm_stats[c128_hw16384_eps6]; the model tests and the other
        ten statistics cases stay green, most of them never reach the two-launch form); here all eleven two-launch cases;
    the predicate of launch_gn_stats retuned (one-launch form only for HW <= 64): every old test stays green; here the ten one-launch cases and the
        range-shift identity on that form fail on their route check.
"""
import contextlib
import ctypes as C
import math

import pytest
import torch

import groupnorm_bound as gb
from kernel_routing import matrix_kernels
from ldiffusion_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"


def sp():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@contextlib.contextmanager
def profiled(lib):
    """with profiled(lib) as names: <launches> -> every profiler row name of the launches (kernel_routing.reached keeps the matrix kernels only)."""
    names = set()
    torch.cuda.synchronize()
    lib.ldiff_prof_set_filter(None)
    _lib.prof_collect()
    lib.ldiff_prof_enable(1)
    try:
        yield names
    finally:
        try:
            torch.cuda.synchronize()
            names.update(r["name"] for r in _lib.prof_collect())
        finally:
            lib.ldiff_prof_enable(0)


# ======================================================================================================================
# 1. the separate statistics pass (ldiff_op_gn_stats)
# ======================================================================================================================
def _source(hi, lo, pitch):
    """One source as the kernel reads it: [B, HW, ld] fp16 with the lo half (split) behind the hi half; columns the kernel must not read are NaN."""
    B, HW, Cs = hi.shape
    ld = pitch if pitch else (2 * Cs if lo is not None else Cs)
    buf = torch.full((B, HW, ld), float("nan"), dtype=torch.float16)
    buf[..., :Cs] = hi
    if lo is not None:
        buf[..., Cs:2 * Cs] = lo
    return buf.to(DEV), ld if (pitch or lo is not None) else 0, Cs if lo is not None else 0


def run_gn_stats(lib, case, inp, eps=None):
    C1, C2, Cc = case.C1, case.C2, case.C1 + case.C2
    lo = inp["lo"]
    x1, ld1, lo1 = _source(inp["hi"][..., :C1], lo[..., :C1] if lo is not None else None, case.pitch)
    x2, ld2, lo2 = (None, 0, 0)
    if C2:
        x2, ld2, lo2 = _source(inp["hi"][..., C1:], lo[..., C1:] if lo is not None else None, 0)
    scale = torch.full((case.B, Cc), float("nan"), device=DEV)
    shift = torch.full((case.B, Cc), float("nan"), device=DEV)
    gd, bd = inp["gamma"].to(DEV), inp["beta"].to(DEV)
    with profiled(lib) as names:
        _lib.check(lib.ldiff_op_gn_stats(x1.data_ptr(), C1, ld1, lo1, x2.data_ptr() if C2 else None, C2, ld2, lo2, case.B, case.HW, case.groups,
                                         case.eps if eps is None else eps, gd.data_ptr(), bd.data_ptr(), scale.data_ptr(), shift.data_ptr(), sp()))
    return scale.cpu(), shift.cpu(), {n for n in names if n.startswith("gn_stats")}


@pytest.mark.parametrize("name", list(gb.STATS_CASES))
def test_gn_stats_against_float64(lib, name):
    """scale / shift of ldiff_op_gn_stats against the float64 statistics of the values the kernel sees (hi + lo for a split source), within
    groupnorm_bound.stats_tol; the case reaches the form it names; the same bound rejects the group boundary off by one channel, the last pixel
    left out and, where a variance is within 10 x of eps, eps doubled.  A constant group (var = 0 exactly) gives scale = gamma / sqrt(eps) bit for bit."""
    case = gb.STATS_CASES[name]
    inp = gb.make_stats_input(case, 7)
    scale, shift, forms = run_gn_stats(lib, case, inp)
    assert forms == {case.form}, f"{name}: reached {sorted(forms)}, the case is meant for {case.form}"
    assert torch.isfinite(scale).all() and torch.isfinite(shift).all()
    ref = gb.stats_reference(inp["v"], case.groups, case.eps, inp["gamma"], inp["beta"])
    r = gb.stats_ratio(scale, shift, ref)
    print(f"[gn-err] {name} ({case.form}): error / bound = {r:.3f}, error / (u amp) = {gb.stats_c_ratio(scale, shift, ref):.3f} (c = {gb.C_STATS})")
    assert r <= 1.0, f"{name}: scale / shift at {r:.3f} of the bound"
    for what, wrong in gb.stats_wrong_references(inp, case):
        rw = gb.stats_ratio(scale, shift, wrong)
        assert rw > 1.0, f"{name}: the bound accepts the wrong reference '{what}' ({rw:.3f})"
    if case.special == "const":
        Cg = (case.C1 + case.C2) // case.groups
        rstd = torch.tensor(1.0 / math.sqrt(gb.f32eps(case.eps)), dtype=torch.float64).float()
        assert (scale[:, :Cg] == rstd).all(), "a constant group must give gamma / sqrt(eps) exactly"
        assert (shift[:, :Cg] == -(torch.tensor(gb.CONST_VALUE) * rstd)).all()


@pytest.mark.parametrize("name", ["small_c640_cg20_hw1024", "two_c128_hw2048"])
@pytest.mark.parametrize("k", [4, 8])
def test_gn_stats_range_shift_identity(lib, name, k):
    """x 2^-k at eps 4^-k: scale = 2^k x the unshifted scale and shift unchanged, bit for bit (a power of two is exact through the fp32 sums
    and the float64 finalize).  The inputs are multiples of 2^-10, so that x 2^-k is exact in fp16 down into the subnormals."""
    case = gb.STATS_CASES[name]._replace(affine=True)
    inp = gb.make_stats_input(case, 11)
    inp["hi"] = (torch.round(inp["hi"].float() * 1024) / 1024).to(torch.float16)
    small = dict(inp, hi=(inp["hi"].float() * 2.0 ** -k).to(torch.float16))
    assert torch.equal(small["hi"].float() * 2.0 ** k, inp["hi"].float())
    sc0, sh0, _ = run_gn_stats(lib, case, inp)
    sck, shk, forms = run_gn_stats(lib, case, small, eps=case.eps * 4.0 ** -k)
    assert forms == {case.form}
    assert torch.equal(sck, sc0 * 2.0 ** k) and torch.equal(shk, sh0)


# ======================================================================================================================
# 2. statistics fused into the producers (ldiff_conv_args.stats + ldiff_op_gn_finalize)
# ======================================================================================================================
# name: (B, Cin, H, W, N, ks, stride, gn prologue, operand "plain" | "lo8", split output, splitk, gemm_df, ups, c3d_ups, kernel, L_b)
#   L_b = the values one partial accumulates in fp32: an 8 x 16 pixel tile (128: the wide halo kernel, one wave group of the 16 x 16 kernels, one
#   parity of a folded upsample), half an 8 x 8 tile (32), 32 rows (the GEMM / implicit-GEMM epilogues and the split-K reduce)
FUSED_CASES = {
    "halo_8x16": (2, 64, 32, 32, 128, 3, 1, False, "plain", False, 0, 0, 0, 0, "conv3x3<8x16,128>", 128),
    "halo_8x8": (3, 128, 8, 8, 128, 3, 1, False, "plain", False, 0, 0, 0, 0, "conv3x3<8x8,128>", 32),
    "pingpong_256x256": (1, 64, 256, 256, 128, 3, 1, False, "plain", False, 0, 0, 0, 0, "conv3x3<16x16,128>", 128),   # the largest map of the section
    "pingpong_lo8": (4, 128, 128, 128, 128, 3, 1, False, "lo8", True, 0, 0, 0, 0, "conv3x3<16x16,128>", 128),
    "dataflow_gn": (1, 64, 256, 256, 128, 3, 1, True, "plain", False, 0, 0, 0, 0, "conv3x3<16x16d,128,gn>", 128),     # one unit per workgroup, one slab
    "dataflow_ups": (2, 64, 128, 128, 128, 3, 1, False, "plain", False, 0, 0, 1, 1, "conv3x3<16x16d,128,ups>", 128),
    "gemm_dma": (2, 128, 16, 16, 256, 1, 1, False, "plain", False, 0, -1, 0, 0, "gemm_dma<64,64>", 32),
    "gemm_df": (2, 256, 32, 64, 256, 1, 1, False, "plain", False, 0, 1, 0, 0, "gemm_df", 32),
    "igemm_stride2": (2, 64, 32, 32, 64, 3, 2, False, "plain", False, 0, 0, 0, 0, "igemm<64,64,fast>", 32),
    "halo_parity_upsample": (1, 64, 16, 16, 64, 3, 1, False, "plain", False, 0, 0, 1, 0, "conv3x3<8x16,64>", 128),
    "splitk4_3x3": (3, 256, 8, 8, 128, 3, 1, False, "plain", False, 4, 0, 0, 0, "conv3x3<8x8,128>", 32),
    "splitk3_1x1": (2, 512, 16, 16, 256, 1, 1, False, "plain", False, 3, -1, 0, 0, "gemm_dma<64,64>", 32),
    "splitk2_igemm": (2, 64, 32, 32, 64, 3, 2, False, "plain", False, 2, 0, 0, 0, "igemm<64,64,fast>", 32),
    "halo_8x16_split_out": (2, 64, 32, 32, 128, 3, 1, False, "plain", True, 0, 0, 0, 0, "conv3x3<8x16,128>", 128),
    # a second producer on halo_8x16's map: its 64 channels behind the other's 128 make a group (Cg = 6) straddle C1 in the two-source finalize
    "halo_8x16_n64": (2, 64, 32, 32, 64, 3, 1, False, "plain", False, 0, 0, 0, 0, "conv3x3<8x16,64>", 128),
    # output std 3e-3 around 0.025: the groups' variances are ~ eps
    "gemm_dma_var_eps": (2, 128, 16, 16, 256, 1, 1, False, "plain", False, 0, -1, 0, 0, "gemm_dma<64,64>", 32),
}


def run_producer(lib, name):
    """One ldiff_op_conv launch with fused statistics -> (v [B, HW, N] float64: the stored output, hi + lo for a split one; stats [B, N, R, 2] cpu;
    the matrix kernels reached).  The bias puts the output's mean at ~8 of its standard deviations."""
    B, Cin, H, W, N, ks, stride, gn, operand, split_out, splitk, gdf, ups, c3d_ups, kernel, L_b = FUSED_CASES[name]
    g = torch.Generator().manual_seed(len(name) * 131 + N)
    K = ks * ks * Cin
    wscale, bmean = (3e-3, 0.025) if name.endswith("var_eps") else (1.0, 8.0)
    x = torch.randn((B, H, W, Cin), generator=g)
    w = (torch.randn((N, ks, ks, Cin), generator=g) * (wscale / math.sqrt(K))).to(torch.float16)
    bias = bmean * (1 + (0.0 if wscale != 1.0 else 0.06) * torch.randn(N, generator=g))
    a = _lib.ConvArgs()
    keep = []
    if operand == "lo8":
        x32 = torch.cat([x.to(torch.float16), (x - x.to(torch.float16).float()).to(torch.float16)], -1).contiguous().to(DEV)
        ones, zeros = torch.ones((B, Cin), device=DEV), torch.zeros((B, Cin), device=DEV)
        xq = torch.empty((B, H, W, 3 * Cin), dtype=torch.uint8, device=DEV)
        _lib.check(lib.ldiff_op_norm_apply_lo8(x32.data_ptr(), Cin, 2 * Cin, Cin, B, H * W, ones.data_ptr(), zeros.data_ptr(), 0, xq.data_ptr(), sp()))
        wd = w.reshape(N, -1).contiguous().to(DEV)
        wq = torch.empty((N, 9, 3 * Cin), dtype=torch.uint8, device=DEV)
        wsc = torch.zeros(4, dtype=torch.int32, device=DEV)
        _lib.check(lib.ldiff_op_lo8_weights(wd.data_ptr(), wq.data_ptr(), wsc.data_ptr(), N, 9, Cin, sp()))
        keep += [x32, xq, wd, wq, wsc]
        a.x, a.C1, a.w = xq.data_ptr(), Cin + Cin // 2, wq.data_ptr()
        a.lo8_slab0, a.lo8_scale = Cin // 64, wsc.data_ptr()
    else:
        xd, wd = x.to(torch.float16).to(DEV), w.reshape(N, -1).contiguous().to(DEV)
        keep += [xd, wd]
        a.x, a.C1, a.w = xd.data_ptr(), Cin, wd.data_ptr()
    He, We = H << ups, W << ups
    Ho, Wo = (He + 2 * (ks // 2) - ks) // stride + 1, (We + 2 * (ks // 2) - ks) // stride + 1
    a.B, a.Hin, a.Win, a.Hout, a.Wout = B, H, W, Ho, Wo
    a.ks, a.stride, a.pad_t, a.pad_l, a.ups, a.c3d_ups = ks, stride, ks // 2, ks // 2, ups, c3d_ups
    a.N, a.Nrows = N, N
    bd = bias.to(DEV)
    a.bias = bd.data_ptr()
    if gn:
        sc, sh = (1.0 + 0.2 * torch.randn((B, Cin), generator=g)).to(DEV), (0.2 * torch.randn((B, Cin), generator=g)).to(DEV)
        keep += [sc, sh]
        a.gn_scale, a.gn_shift, a.silu_in = sc.data_ptr(), sh.data_ptr(), 1
    ldy = 2 * N if split_out else N
    y = torch.full((B, Ho * Wo, ldy), float("nan"), dtype=torch.float16, device=DEV)
    a.y, a.ldy, a.y_lo, a.splitk, a.gemm_df = y.data_ptr(), ldy, N if split_out else 0, splitk, gdf
    R = lib.ldiff_op_conv_stats_blocks(C.byref(a))
    assert R > 0, f"{name}: no fused statistics for this shape"
    st = torch.full((B, N, R, 2), float("nan"), device=DEV)   # NaN first: every entry must be written
    a.stats = st.data_ptr()
    with profiled(lib) as names:
        _lib.check(lib.ldiff_op_conv(C.byref(a), sp()))
    yc = y.cpu().double()
    v = yc[..., :N] + yc[..., N:] if split_out else yc
    assert torch.isfinite(v).all()
    return v, st.cpu(), matrix_kernels(names)


def finalize(lib, st, HW, eps=1e-5, st2=None, gam=None, bet=None):
    B, N1, R1, _ = st.shape
    N2, R2 = (st2.shape[1], st2.shape[2]) if st2 is not None else (0, 0)
    Cc = N1 + N2
    gam = torch.ones(Cc) if gam is None else gam
    bet = torch.zeros(Cc) if bet is None else bet
    s1, gd, bd = st.contiguous().to(DEV), gam.to(DEV), bet.to(DEV)
    s2 = st2.contiguous().to(DEV) if st2 is not None else None
    scale, shift = torch.full((B, Cc), float("nan"), device=DEV), torch.full((B, Cc), float("nan"), device=DEV)
    _lib.check(lib.ldiff_op_gn_finalize(s1.data_ptr(), R1, N1, s2.data_ptr() if st2 is not None else None, R2, N2, B, HW, 32, eps, gd.data_ptr(), bd.data_ptr(),
                                        scale.data_ptr(), shift.data_ptr(), sp()))
    torch.cuda.synchronize()
    return scale.cpu(), shift.cpu()


_PRODUCED = {}


def produced(lib, name):
    """Each producer runs once; the two-source finalize test reuses two of the outputs (never modified)."""
    if name not in _PRODUCED:
        _PRODUCED[name] = run_producer(lib, name)
    return _PRODUCED[name]


@pytest.mark.parametrize("name", list(FUSED_CASES))
def test_fused_statistics_against_float64(lib, name):
    """Level 1: the R partials of every (image, channel), added in float64, against the float64 sum and sum of squares of the output the kernel
    stored, within gamma(L_b) sum|y| and (gamma(L_b) + 2u) sum y^2 (a split output's statistics are of the fp32 value, within 2^-22 of hi + lo:
    4u more).  Level 2: scale / shift behind ldiff_op_gn_finalize within section 1's bound.  Both levels reject the statistics with one row
    block's contribution removed; where the variances are ~ eps the finalize level rejects eps doubled."""
    split_out, kernel, L_b = FUSED_CASES[name][9], FUSED_CASES[name][14], FUSED_CASES[name][15]
    v, st, kernels = produced(lib, name)
    assert kernels == {kernel}, f"{name}: reached {sorted(kernels)}, the case is meant for {kernel}"
    assert torch.isfinite(st).all(), "statistics not written everywhere"
    extra = 4 if split_out else 0
    rs, rq = gb.sums_ratio(st, v, L_b, extra)
    HW = v.shape[1]
    scale, shift = finalize(lib, st, HW)
    ref = gb.stats_reference(v, 32, 1e-5, torch.ones(v.shape[2]), torch.zeros(v.shape[2]))
    r2 = gb.stats_ratio(scale, shift, ref)
    print(f"[gn-fused] {name} ({kernel}, R = {st.shape[2]}, L_b = {L_b}): sum {rs:.4f}, sum of squares {rq:.4f}, scale / shift {r2:.3f} of the bound")
    assert rs <= 1.0 and rq <= 1.0, f"{name}: partial sums at {rs:.3f} / {rq:.3f} of the bound"
    assert r2 <= 1.0, f"{name}: scale / shift at {r2:.3f} of the bound"
    cut = st.clone()
    cut[0, :, -1, :] = 0.0                                    # one row block's contribution removed
    ws, wq = gb.sums_ratio(cut, v, L_b, extra)
    assert ws > 1.0 and wq > 1.0, f"{name}: the sums' bound accepts a lost row block ({ws:.3f}, {wq:.3f})"
    assert gb.stats_ratio(*finalize(lib, cut, HW), ref) > 1.0, f"{name}: the finalize bound accepts a lost row block"
    if (ref.var <= 10 * ref.eps).any():
        assert name.endswith("var_eps")
        assert gb.stats_ratio(scale, shift, gb.stats_reference(v, 32, 2e-5, torch.ones(v.shape[2]), torch.zeros(v.shape[2]))) > 1.0
    else:
        assert not name.endswith("var_eps")


def test_fused_statistics_two_sources(lib):
    """ldiff_op_gn_finalize over two producers' partials (part2: the second concat source): 128 + 64 channels in 32 groups of 6, one of which
    straddles C1; per-channel gamma / beta."""
    v1, st1, _ = produced(lib, "halo_8x16")
    v2, st2, _ = produced(lib, "halo_8x16_n64")
    g = torch.Generator().manual_seed(5)
    gam, bet = 1 + 0.3 * torch.randn(192, generator=g), 0.5 * torch.randn(192, generator=g)
    v = torch.cat([v1, v2], -1)
    scale, shift = finalize(lib, st1, v.shape[1], st2=st2, gam=gam, bet=bet)
    ref = gb.stats_reference(v, 32, 1e-5, gam, bet)
    r = gb.stats_ratio(scale, shift, ref)
    print(f"[gn-fused] two sources 128 + 64: scale / shift {r:.3f} of the bound")
    assert r <= 1.0
    assert gb.stats_ratio(scale, shift, gb.stats_reference(v, 32, 1e-5, gam, bet, shift_channels=1)) > 1.0
    cut = st2.clone()
    cut[0, :, -1, :] = 0.0
    assert gb.stats_ratio(*finalize(lib, st1, v.shape[1], st2=cut, gam=gam, bet=bet), ref) > 1.0


# ======================================================================================================================
# 3. GroupNorm folded into the 1x1 conv (ldiff_conv_args.fold_gn)
# ======================================================================================================================
def run_fold(lib, case, inp, fold):
    """The launch(es) of a GroupNorm -> 1x1 conv: fold = 1 plans it as the executors do (fold_gn_weights + gemm_dma on per-image weights where
    the plan folds), fold = 0 is the GroupNorm-prologue route.  -> (y [B, HW, N] fp16 cpu, every profiler row name)."""
    B, HW, Cc, N = case.B, case.HW, case.C, case.N
    xd, wd, sd, td = inp["x"].to(DEV), inp["W"].to(DEV), inp["s"].to(DEV), inp["t"].to(DEV)
    bd = inp["bias"].to(DEV) if inp["bias"] is not None else None
    y = torch.full((B, HW, N), float("nan"), dtype=torch.float16, device=DEV)
    a = _lib.ConvArgs()
    a.x, a.C1, a.B, a.Hin, a.Win, a.Hout, a.Wout, a.ks, a.stride = xd.data_ptr(), Cc, B, 1, HW, 1, HW, 1, 1
    a.w, a.N, a.Nrows, a.y, a.ldy = wd.data_ptr(), N, case.Nrows, y.data_ptr(), N
    a.gn_scale, a.gn_shift, a.fold_gn = sd.data_ptr(), td.data_ptr(), fold
    if bd is not None:
        a.bias = bd.data_ptr()
    with profiled(lib) as names:
        _lib.check(lib.ldiff_op_conv(C.byref(a), sp()))
    return y.cpu(), names


def check_fold_route(names, case, fold, what):
    kernels = matrix_kernels(names)
    if fold and case.folds:
        assert kernels == {case.kernel} and "fold_gn_weights" in names, f"{what}: reached {sorted(names)}, the case is meant for fold_gn_weights + {case.kernel}"
    else:
        assert "fold_gn_weights" not in names and len(kernels) == 1 and all(k.startswith("igemm<") and k.endswith(",gn>") for k in kernels), \
            f"{what}: reached {sorted(names)}, the case is meant for the GroupNorm prologue of igemm<...,gn>"
        if not case.folds:
            assert kernels == {case.kernel}


@pytest.mark.parametrize("name", list(gb.FOLD_CASES))
def test_fold_gn_against_float64(lib, name):
    """fold_gn_weights + gemm_dma on per-image weights against (x s_b + t_b) W^T + bias in float64, within groupnorm_bound.fold_tol per element; the
    bound rejects image b computed with image b + 1's scale / shift, the last K block left out and the shift left out of the bias.  The HW = 48
    case must be declined by the plan and stay within the unfolded model."""
    case = gb.FOLD_CASES[name]
    inp = gb.make_fold_input(case, 3)
    x, W, s, t, bias = inp["x"], inp["W"][:case.N], inp["s"], inp["t"], (inp["bias"][:case.N] if inp["bias"] is not None else None)
    y, names = run_fold(lib, case, inp, 1)
    check_fold_route(names, case, 1, name)
    ref = gb.fold_reference(x, W, s, t, bias)
    tol = gb.fold_tol(x, W, s, t, bias, ref) if case.folds else gb.unfolded_tol(x, W, s, t, bias, ref)
    r = gb.ratio(y, ref, tol)
    print(f"[gn-fold] {name} ({'folded' if case.folds else 'declined'}, {case.kernel}): error / bound = {r:.3f}, max error / max|ref| = {gb.rel_err(y, ref):.2e}")
    assert torch.isfinite(y.float()).all() and r <= 1.0, f"{name}: {r:.3f} of the bound"
    for what, wrong in gb.fold_wrong_references(x, W, s, t, bias):
        rw = gb.ratio(y, wrong, tol)
        assert rw > 1.0, f"{name}: the bound accepts the wrong reference '{what}' ({rw:.3f})"


@pytest.mark.parametrize("regime", list(gb.FOLD_REGIMES))
def test_fold_gn_operand_regimes(lib, regime):
    """The VAE q/k/v shape at |group mean| / std 0.3, 3, 10 and at std 1, 1024, 4096 (folded weights in fp16's subnormals): the folded launch within
    its bound and within 2 x the CPU emulation's error for the same inputs (the emulation describes the kernel); the unfolded launch within its own
    bound.  Both routes' errors are printed: the table of DESIGN.md."""
    case = gb.FOLD_CASES["vae_qkv_smallest_map"]
    mr, sd = gb.FOLD_REGIMES[regime]
    inp = gb.make_fold_input(case, 3, mr, sd)
    x, W, s, t, bias = inp["x"], inp["W"], inp["s"], inp["t"], inp["bias"]
    ref = gb.fold_reference(x, W, s, t, bias)
    yf, names = run_fold(lib, case, inp, 1)
    check_fold_route(names, case, 1, regime)
    yu, names = run_fold(lib, case, inp, 0)
    check_fold_route(names, case, 0, regime)
    rf, ru = gb.ratio(yf, ref, gb.fold_tol(x, W, s, t, bias, ref)), gb.ratio(yu, ref, gb.unfolded_tol(x, W, s, t, bias, ref))
    ef, eu, ee = gb.rel_err(yf, ref), gb.rel_err(yu, ref), gb.rel_err(gb.folded_emulation(x, W, s, t, bias), ref)
    print(f"[gn-fold] regime {regime}: max error / max|ref| unfolded {eu:.2e}, folded {ef:.2e} (CPU emulation of the fold {ee:.2e}); "
          f"error / bound unfolded {ru:.3f}, folded {rf:.3f}")
    assert rf <= 1.0, f"{regime}: folded launch at {rf:.3f} of its bound"
    assert ru <= 1.0, f"{regime}: unfolded launch at {ru:.3f} of its bound"
    assert ef <= 2.0 * ee, f"{regime}: folded error {ef:.3e} is more than twice the emulation's {ee:.3e}"


def test_fold_gn_overflow_is_visible(lib):
    """A scale so large that |W s| passes 65504 (a shifted decoder at large k can produce one): the folded weights hold fp16 infinities.
    Found: the launch's output is non-finite (inf - inf = NaN in the sums), torch.isfinite shows it, and a following ldiff_op_gn_stats on that
    output returns non-finite scale / shift (its sums are NaN); the single-kernel entry points expose no sticky flag, the executors' handles do
    (the same sums set it: flag_nonfinite)."""
    case = gb.FOLD_CASES["vae_qkv_smallest_map"]
    inp = gb.make_fold_input(case, 3)
    inp["s"] = inp["s"] * 1.0e7
    assert ((inp["W"].float().abs().max() * inp["s"].abs().max()) > 65504).item()
    y, names = run_fold(lib, case, inp, 1)
    check_fold_route(names, case, 1, "overflow")
    assert not torch.isfinite(y.float()).all()
    st_case = gb.StatsCase(gb.ONE, case.B, case.N, 0, case.HW, 32)
    assert gb.expected_form(st_case) == gb.ONE
    scale, shift, _ = run_gn_stats(lib, st_case, dict(hi=y, lo=None, gamma=torch.ones(case.N), beta=torch.zeros(case.N)))
    assert not torch.isfinite(scale).all() and not torch.isfinite(shift).all()
