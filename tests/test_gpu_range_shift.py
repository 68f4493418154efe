"""-m gpu: the VAE decoder's range shift (include/ldiff.h ldiff_vae_set_range_shift, ldiff_conv_args.out_shift; DESIGN.md section 3 "Range").

A launch with out_shift = k computes (sum + bias) * 2^-k, then adds a residual that was supplied shifted.  A power of two is exact, so:
  * kernel level: every output element (hi and lo) that stays at or above 2^-14 after the shift equals the k = 0 output times 2^-k bit for bit,
    and the fused statistics equal sum * 2^-k and sumsq * 4^-k bit for bit (inputs are built so that no stored value becomes an fp16 subnormal);
  * a split output whose hi half rounds to inf must reach the GroupNorm finalize as a non-finite value (the detector gap of split epilogues);
  * model level: decoders whose fp16 activations overflow decode at the k fit_range_shift picks, within the healthy bounds of
    test_gpu_models.py (sample / image <= 4e-3 of range, rgb within one grey level), and the UNet / encoder are untouched by k."""
import ctypes as C
import math
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ldiffusion_amd import _lib, configs, weights
from ldiffusion_amd.models import AutoencoderKL, UNet2DConditionModel
from ldiffusion_amd.pipeline import LaplaceSampler, StableDiffusionImg2ImgPipeline
from oracle import noise_post, pipeline as op
from oracle.unet import _conv, _gn, resnet_block
from oracle.vae import VAE_EPS, _mid, vae_decode
from kernel_routing import matrix_kernels, reached

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP16_MIN_NORMAL = 2.0 ** -14


def sp():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------------------------------------------------------------------------
# name: (B, Cin, H, W, N, ks, stride, gn, operand, res, out, splitk, gemm_df, kernel prefix)
#   operand: "plain" fp16 x | "lo8" split operand with an fp8 lo half; res / out: "none" | "plain" | "split"
KCASES = {
    "halo_8x16_gn_split": (2, 64, 16, 32, 128, 3, 1, True, "plain", "split", "split", 0, 0, "conv3x3<8x16,128,gn>"),
    "halo_8x16_gn_plain": (2, 64, 16, 32, 128, 3, 1, True, "plain", "plain", "plain", 0, 0, "conv3x3<8x16,128,gn>"),
    "halo_8x8_gn_split": (2, 128, 8, 8, 128, 3, 1, True, "plain", "split", "split", 0, 0, "conv3x3<8x8,128,gn>"),
    "halo_splitk4_stats_split": (2, 512, 8, 8, 128, 3, 1, True, "plain", "split", "split", 4, 0, "conv3x3<8x8,128,gn>"),
    "halo_splitk4_stats_plain": (2, 512, 8, 8, 128, 3, 1, True, "plain", "plain", "plain", 4, 0, "conv3x3<8x8,128,gn>"),
    "pingpong_split": (1, 64, 256, 256, 128, 3, 1, False, "plain", "split", "split", 0, 0, "conv3x3<16x16,128>"),
    "pingpong_plain": (1, 64, 256, 256, 128, 3, 1, False, "plain", "plain", "plain", 0, 0, "conv3x3<16x16,128>"),
    "pingpong_lo8_split": (4, 128, 128, 128, 128, 3, 1, False, "lo8", "split", "split", 0, 0, "conv3x3<16x16,128>"),
    "pingpong_lo8_nores": (4, 128, 128, 128, 128, 3, 1, False, "lo8", "none", "split", 0, 0, "conv3x3<16x16,128>"),
    "dataflow_gn_res": (1, 128, 256, 256, 128, 3, 1, True, "plain", "plain", "plain", 0, 0, "conv3x3<16x16d,128,gn>"),
    "gemm_dma_split": (2, 128, 16, 16, 128, 1, 1, False, "plain", "split", "split", 0, -1, "gemm_dma<"),
    "gemm_dma_plain": (2, 128, 16, 16, 128, 1, 1, False, "plain", "plain", "plain", 0, -1, "gemm_dma<"),
    "gemm_df_split": (2, 256, 32, 64, 256, 1, 1, False, "plain", "split", "split", 0, 1, "gemm_df"),
    "gemm_df_plain": (2, 256, 32, 64, 256, 1, 1, False, "plain", "plain", "plain", 0, 1, "gemm_df"),
    "igemm_gn1x1_split": (2, 128, 16, 16, 128, 1, 1, True, "plain", "split", "split", 0, 0, "igemm<"),
    "igemm_stride2_split": (2, 128, 32, 32, 128, 3, 2, False, "plain", "split", "split", 0, 0, "igemm<"),
}


def _signed(g, shape, lo, hi, sign):
    """values of magnitude in [lo, hi) with the given sign (broadcast over channels): the sums stay clear of zero and of fp16's subnormals"""
    return sign * (lo + (hi - lo) * torch.rand(shape, generator=g))


class KCase:
    """One ldiff_op_conv launch of KCASES, runnable at any out_shift with the residual given shifted by the same k."""

    def __init__(self, lib, name):
        self.lib, self.name = lib, name
        (B, Cin, H, W, N, ks, stride, gn, operand, res, out, splitk, gdf, self.kernel) = KCASES[name]
        self.B, self.N, self.res, self.out = B, N, res, out
        g = torch.Generator().manual_seed(zlib.crc32(name.encode()) % 10000)
        Ho, Wo = (H + 2 * (ks // 2) - ks) // stride + 1, (W + 2 * (ks // 2) - ks) // stride + 1
        self.Ho, self.Wo = Ho, Wo
        K = ks * ks * Cin
        x = torch.randn((B, H, W, Cin), generator=g)
        w = (torch.randn((N, ks, ks, Cin), generator=g) * (0.25 / math.sqrt(K))).to(torch.float16)
        sign = torch.where(torch.rand(N, generator=g) < 0.5, -1.0, 1.0)
        self.sign = sign
        bias = _signed(g, (N,), 8.0, 16.0, sign)
        a = self.a = _lib.ConvArgs()
        self.keep = []
        if operand == "lo8":
            x32 = torch.cat([x.to(torch.float16), (x - x.to(torch.float16).float()).to(torch.float16)], -1).contiguous().to(DEV)
            ones, zeros = torch.ones((B, Cin), device=DEV), torch.zeros((B, Cin), device=DEV)
            xq = torch.empty((B, H, W, 3 * Cin), dtype=torch.uint8, device=DEV)
            _lib.check(lib.ldiff_op_norm_apply_lo8(x32.data_ptr(), Cin, 2 * Cin, Cin, B, H * W, ones.data_ptr(), zeros.data_ptr(), 0, xq.data_ptr(), sp()))
            wd = w.reshape(N, -1).contiguous().to(DEV)
            wq = torch.empty((N, 9, 3 * Cin), dtype=torch.uint8, device=DEV)
            wsc = torch.zeros(4, dtype=torch.int32, device=DEV)
            _lib.check(lib.ldiff_op_lo8_weights(wd.data_ptr(), wq.data_ptr(), wsc.data_ptr(), N, 9, Cin, sp()))
            self.keep += [x32, xq, wd, wq, wsc]
            a.x, a.C1, a.w, a.Nrows = xq.data_ptr(), Cin + Cin // 2, wq.data_ptr(), N
            a.lo8_slab0, a.lo8_scale = Cin // 64, wsc.data_ptr()
        else:
            xd = x.to(torch.float16).to(DEV)
            wd = w.reshape(N, -1).contiguous().to(DEV)
            self.keep += [xd, wd]
            a.x, a.C1, a.w, a.Nrows = xd.data_ptr(), Cin, wd.data_ptr(), N
        a.B, a.Hin, a.Win, a.Hout, a.Wout = B, H, W, Ho, Wo
        a.ks, a.stride, a.pad_t, a.pad_l = ks, stride, ks // 2, ks // 2
        a.N = N
        bd = bias.to(DEV)
        self.keep.append(bd)
        a.bias = bd.data_ptr()
        if gn:
            sc, sh = (1.0 + 0.2 * torch.randn((B, Cin), generator=g)).to(DEV), (0.2 * torch.randn((B, Cin), generator=g)).to(DEV)
            self.keep += [sc, sh]
            a.gn_scale, a.gn_shift, a.silu_in = sc.data_ptr(), sh.data_ptr(), 0 if ks == 1 else 1
        # residual: hi of magnitude [1, 8), lo of magnitude [0.25, 0.5), both with the bias's sign (no cancellation), exactly shiftable by <= 2^-12
        self.rhi = _signed(g, (B, Ho, Wo, N), 1.0, 8.0, sign).to(torch.float16)
        self.rlo = _signed(g, (B, Ho, Wo, N), 0.25, 0.5, sign).to(torch.float16)
        self.ldy = 2 * N if out == "split" else N
        a.ldy, a.y_lo = self.ldy, (N if out == "split" else 0)
        a.splitk, a.gemm_df = splitk, gdf
        self.y = torch.empty((B, Ho, Wo, self.ldy), dtype=torch.float16, device=DEV)
        a.y = self.y.data_ptr()
        self._set_res(self.rhi, self.rlo, 0)   # (the layout of the launch, as the plan sees it, before its statistics row blocks are asked for)
        self.R = lib.ldiff_op_conv_stats_blocks(C.byref(a))
        assert self.R > 0, f"{name}: no fused statistics for this shape"

    def _set_res(self, rhi, rlo, k):
        a, N, s = self.a, self.N, 2.0 ** -k
        self.rd = None
        if self.res == "split":
            self.rd = torch.cat([(rhi.float() * s).to(torch.float16), (rlo.float() * s).to(torch.float16)], -1).contiguous().to(DEV)
            a.res, a.ld_res, a.res_lo = self.rd.data_ptr(), 2 * N, N
        elif self.res == "plain":
            self.rd = (rhi.float() * s).to(torch.float16).contiguous().to(DEV)
            a.res, a.ld_res, a.res_lo = self.rd.data_ptr(), N, 0
        else:
            a.res, a.ld_res, a.res_lo = None, 0, 0

    def run(self, k, poke=None):
        """-> (y [B, Ho, Wo, ldy] fp16 cpu, stats [B, N, R, 2] f32 cpu, reached kernel names).  poke: (index, hi, lo) written into the residual first."""
        a, B, N = self.a, self.B, self.N
        rhi, rlo = self.rhi.clone(), self.rlo.clone()
        if poke is not None:
            rhi[poke[0]], rlo[poke[0]] = poke[1], poke[2]
        self._set_res(rhi, rlo, k)
        y = self.y
        y.fill_(float("nan"))
        st = torch.full((B, N, self.R, 2), float("nan"), device=DEV)
        a.y, a.stats, a.out_shift = y.data_ptr(), st.data_ptr(), k
        with reached(self.lib) as names:
            _lib.check(self.lib.ldiff_op_conv(C.byref(a), sp()))
            torch.cuda.synchronize()
        return y.cpu(), st.cpu(), set(names)


def _finalize(lib, st, B, N, HW):
    R = st.shape[2]
    std = st.contiguous().to(DEV)
    gd, bd = torch.ones(N, device=DEV), torch.zeros(N, device=DEV)
    scale, shift = torch.empty((B, N), device=DEV), torch.empty((B, N), device=DEV)
    _lib.check(lib.ldiff_op_gn_finalize(std.data_ptr(), R, N, None, 0, 0, B, HW, 32, 1e-6, gd.data_ptr(), bd.data_ptr(), scale.data_ptr(), shift.data_ptr(), sp()))
    torch.cuda.synchronize()
    return scale.cpu(), shift.cpu()


@pytest.mark.parametrize("name", list(KCASES))
def test_out_shift_is_exact_in_every_kernel(lib, name):
    case = KCase(lib, name)
    y0, st0, n0 = case.run(0)
    assert n0 and all(n.startswith(case.kernel) for n in n0), f"{name}: reached {sorted(n0)}, meant for {case.kernel}"
    assert torch.isfinite(y0.float()).all() and torch.isfinite(st0).all()
    for k in (1, 4, 12):
        yk, stk, nk = case.run(k)
        assert nk == n0, f"{name} k={k}: reached {sorted(nk)}, k = 0 reached {sorted(n0)}"
        ref = y0.float() * 2.0 ** -k                                        # exact in fp32
        keep = (ref.abs() >= FP16_MIN_NORMAL) | (ref == 0)
        bad = (yk.float() != ref) & keep
        print(f"{name} k={k}: {int(keep.sum())} of {ref.numel()} stored halves compared, {int(bad.sum())} differ")
        assert not bad.any(), f"{name} k={k}: {int(bad.sum())} stored values are not the k = 0 values times 2^-k"
        if case.out == "plain":   # (nothing of a plain output left out: its statistics are of the stored values)
            assert keep.all()
        assert torch.equal(stk[..., 0], st0[..., 0] * 2.0 ** -k), f"{name} k={k}: sums"
        assert torch.equal(stk[..., 1], st0[..., 1] * 4.0 ** -k), f"{name} k={k}: sums of squares"


@pytest.mark.parametrize("name", [n for n, c in KCASES.items() if c[10] == "split"])
def test_split_output_overflow_reaches_the_statistics(lib, name):
    """A split output element past 65520: its hi half is inf while the fp32 value the statistics sum is finite.  The finalize must see it."""
    case = KCase(lib, name)
    n = int(torch.nonzero(case.sign > 0)[0])
    idx = (case.B - 1, case.Ho // 2, case.Wo // 3, n)
    if case.res == "split":
        y, st, _ = case.run(0, poke=(idx, 65504.0, 64.0))
    else:   # no residual operand (the fp8-lo kernel without one): push the bias past the limit instead
        b = _signed(torch.Generator().manual_seed(1), (case.N,), 8.0, 16.0, case.sign)
        b[n] = 65600.0
        bd = b.to(DEV)
        case.keep.append(bd)
        case.a.bias = bd.data_ptr()
        y, st, _ = case.run(0)
    hi = y[idx].float()
    assert torch.isinf(hi), f"{name}: the poked element did not overflow its hi half ({hi.item()})"
    scale, shift = _finalize(lib, st, case.B, case.N, case.Ho * case.Wo)
    flagged = not (torch.isfinite(scale[idx[0], n]) and torch.isfinite(shift[idx[0], n]))
    assert flagged, f"{name}: an inf hi half left the GroupNorm scale / shift finite (the detector would stay silent)"


def test_out_shift_declines_and_rejects(lib):
    a = _lib.ConvArgs()
    x = torch.zeros((1, 16, 16, 64), dtype=torch.float16, device=DEV)
    w = torch.zeros((64, 9 * 64), dtype=torch.float16, device=DEV)
    y = torch.zeros((1, 16, 16, 64), dtype=torch.float16, device=DEV)
    a.x, a.C1, a.B, a.Hin, a.Win, a.Hout, a.Wout = x.data_ptr(), 64, 1, 16, 16, 16, 16
    a.ks, a.stride, a.pad_t, a.pad_l = 3, 1, 1, 1
    a.w, a.N, a.Nrows, a.y, a.ldy = w.data_ptr(), 64, 64, y.data_ptr(), 64
    for k in (-1, 17):
        a.out_shift = k
        assert lib.ldiff_op_conv(C.byref(a), sp()) == -1, f"out_shift {k} must be refused"
    # the folded shortcut of the dataflow kernel declines a shifted launch: refused by this entry point (the executor runs the two launches)
    B, Cin, Hs, Cout, Cs = 1, 128, 256, 128, 64
    xs = torch.zeros((B, Hs, Hs, Cin), dtype=torch.float16, device=DEV)
    scx = torch.zeros((B, Hs, Hs, Cs), dtype=torch.float16, device=DEV)
    w3 = torch.zeros((Cout, 9 * Cin), dtype=torch.float16, device=DEV)
    wsc = torch.zeros((Cout, Cs), dtype=torch.float16, device=DEV)
    ys = torch.zeros((B, Hs, Hs, Cout), dtype=torch.float16, device=DEV)
    ones, zeros = torch.ones((B, Cin), device=DEV), torch.zeros((B, Cin), device=DEV)
    b = _lib.ConvArgs()
    b.x, b.C1, b.B, b.Hin, b.Win, b.Hout, b.Wout = xs.data_ptr(), Cin, B, Hs, Hs, Hs, Hs
    b.ks, b.stride, b.pad_t, b.pad_l = 3, 1, 1, 1
    b.w, b.N, b.Nrows, b.y, b.ldy = w3.data_ptr(), Cout, Cout, ys.data_ptr(), Cout
    b.gn_scale, b.gn_shift, b.silu_in = ones.data_ptr(), zeros.data_ptr(), 1
    b.sc_x, b.sc_C, b.sc_w = scx.data_ptr(), Cs, wsc.data_ptr()
    _lib.check(lib.ldiff_op_conv(C.byref(b), sp()))   # k = 0: folded
    b.out_shift = 4
    assert lib.ldiff_op_conv(C.byref(b), sp()) == -1
    # the narrow-output kernels (the VAE's conv_out) are never asked to shift: a shifted launch of that shape goes elsewhere
    xn = torch.zeros((1, 64, 64, 128), dtype=torch.float16, device=DEV)
    wn = torch.zeros((32, 9 * 128), dtype=torch.float16, device=DEV)   # (rows past Nrows = 16 allocated: a 32-column tile may read them)
    yn = torch.zeros((1, 64, 64, 4), dtype=torch.float32, device=DEV)
    c = _lib.ConvArgs()
    c.x, c.C1, c.B, c.Hin, c.Win, c.Hout, c.Wout = xn.data_ptr(), 128, 1, 64, 64, 64, 64
    c.ks, c.stride, c.pad_t, c.pad_l = 3, 1, 1, 1
    c.w, c.N, c.Nrows, c.n_real, c.y, c.ldy, c.out_f32 = wn.data_ptr(), 4, 16, 3, yn.data_ptr(), 4, 1
    got = {}
    for k in (0, 1):
        c.out_shift = k
        with reached(lib) as names:
            _lib.check(lib.ldiff_op_conv(C.byref(c), sp()))
            torch.cuda.synchronize()
        got[k] = set(names)
    assert any(",n" in n for n in got[0]) and not any(",n" in n for n in got[1]), got
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    ucfg, vcfg = configs.TINY_UNET, configs.TINY_VAE
    usd = weights.synthetic_state_dict(weights.unet_param_shapes(ucfg), 42, fp16_values=True)
    vsd = weights.synthetic_state_dict(weights.vae_param_shapes(vcfg), 43, fp16_values=True)
    return dict(ucfg=ucfg, vcfg=vcfg, usd=usd, vsd=vsd, unet=UNet2DConditionModel(ucfg, usd, DEV))


def rel_err(got, ref):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert torch.isfinite(got).all(), "non-finite output"
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-6)).item()


def _scaled(sd, key, s):
    bad = dict(sd)
    bad[key + ".weight"], bad[key + ".bias"] = sd[key + ".weight"] * s, sd[key + ".bias"] * s
    assert bad[key + ".weight"].abs().max() < 65504
    return bad


def _stream_absmax(sd, cfg, zs):
    """max |x| over the decoder's residual stream (conv_in output, every block output) of the fp32 oracle"""
    groups, boc, lpb = cfg["norm_num_groups"], cfg["block_out_channels"], cfg["layers_per_block"]
    h = _conv(sd, "decoder.conv_in", _conv(sd, "post_quant_conv", zs, padding=0))
    m = h.abs().max().item()
    h = _mid(sd, "decoder.mid_block", h, groups)
    m = max(m, h.abs().max().item())
    for i in range(len(boc)):
        for j in range(lpb + 1):
            h = resnet_block(sd, f"decoder.up_blocks.{i}.resnets.{j}", h, None, groups, VAE_EPS)
            m = max(m, h.abs().max().item())
        if i != len(boc) - 1:
            h = _conv(sd, f"decoder.up_blocks.{i}.upsamplers.0.conv", F.interpolate(h, scale_factor=2.0, mode="nearest"))
            m = max(m, h.abs().max().item())
    return m


def _overflowing(case, sd, cfg, zs):
    """(a) mid_block.resnets.0.conv1 (feeds only norm2), (b) decoder.conv_in (the whole stream), (c) the last up-block resnet's conv2 (the final
    stream): scaled by the smallest power of two that takes the fp32 activation past 2 x 65504."""
    groups = cfg["norm_num_groups"]
    if case == "a":
        key = "decoder.mid_block.resnets.0.conv1"
        a = F.silu(_gn(sd, "decoder.mid_block.resnets.0.norm1", _conv(sd, "decoder.conv_in", _conv(sd, "post_quant_conv", zs, padding=0)), groups, VAE_EPS))
        measure = lambda s: _conv(sd, key, a).abs().max().item() * s
    elif case == "b":
        key = "decoder.conv_in"
        m = _conv(sd, key, _conv(sd, "post_quant_conv", zs, padding=0)).abs().max().item()
        measure = lambda s: m * s
    else:
        nb = len(cfg["block_out_channels"])
        key = f"decoder.up_blocks.{nb - 1}.resnets.{cfg['layers_per_block']}.conv2"
        measure = lambda s: _stream_absmax(_scaled(sd, key, s), cfg, zs)
    s = 1.0
    while measure(s) <= 2 * 65504:
        s *= 2.0
    return _scaled(sd, key, s), key, s


def _check_decode(vae, bad, vcfg, z, what):
    zs = 1 / 0.18215
    osample = vae_decode(bad, vcfg, z / 0.18215)
    assert torch.isfinite(osample).all(), "the fp32 graph itself must stay finite"
    sample, _, _ = vae._decode(z.to(DEV), zs, want_sample=True)
    _, image, rgb = vae._decode(z.to(DEV), zs, want_image=True, want_rgb=True)
    vae.check_finite()
    oimg = (osample / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1)
    pipe_img = StableDiffusionImg2ImgPipeline(vae, None).decode_latents(z.to(DEV))
    e_s = rel_err(sample, osample)
    e_i = float(np.abs(pipe_img - oimg.numpy()).max())
    rd = np.abs(rgb.cpu().numpy().astype(int) - noise_post.to_uint8(oimg.numpy()).astype(int)).max()
    # decode_latents: the healthy bound is 4e-3 in image units (test_decode_latents_uint8_and_luma), where the healthy decoder's sample stays within
    # +-2.  A scaled checkpoint's sample reaches further (case (c): max|sample| ~ 4, measured image error 4.1e-3 at a sample error of 2.0e-3 of its
    # range): the image is held to the sample's own 4e-3 of range, in image units (x / 2), wherever that is the looser of the two
    smax = osample.abs().max().item()
    i_bound = 4e-3 * max(1.0, smax / 2)
    print(f"{what}: k = {vae.range_shift}: sample rel err {e_s:.3e} (max|sample| {smax:.2f}), decode_latents max err {e_i:.3e} (bound {i_bound:.2e}), "
          f"rgb max diff {rd}")
    assert e_s <= 4e-3 and e_i <= i_bound and rd <= 1
    assert torch.allclose(image.cpu(), torch.from_numpy(pipe_img))


def test_split_output_overflow_is_detected_in_the_decoder(tiny):
    """Case (c): the final stream passes 65504 in the last up-block's conv2 + residual.  In modes 1 / 2 that output is split and its statistics
    were taken of the finite fp32 value: the flag must fire anyway (and, unshifted, it does in mode 0 too)."""
    from ldiffusion_amd._lib import NonFiniteError
    vcfg, vsd = tiny["vcfg"], tiny["vsd"]
    z = torch.randn((2, 4, 8, 8), generator=torch.Generator().manual_seed(21)) * 0.3
    bad, key, s = _overflowing("c", vsd, vcfg, z / 0.18215)
    assert torch.isfinite(vae_decode(bad, vcfg, z / 0.18215)).all()
    vae = AutoencoderKL(vcfg, bad, DEV)
    for mode in (0, 1, 2):
        vae.set_precision(2, mode)
        vae._decode(z.to(DEV), 1 / 0.18215, want_image=True)
        with pytest.raises(NonFiniteError, match="range_shift"):
            vae.check_finite()


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_overflowing_decoders_decode_with_a_range_shift(tiny, case):
    vcfg, vsd = tiny["vcfg"], tiny["vsd"]
    z = torch.randn((2, 4, 8, 8), generator=torch.Generator().manual_seed(11)) * 0.3
    bad, key, s = _overflowing(case, vsd, vcfg, z / 0.18215)
    print(f"case ({case}): {key} x {s:g}")
    vae = AutoencoderKL(vcfg, bad, DEV)
    for mode in (0, 1, 2):
        vae.set_precision(2, mode)
        vae.set_range_shift(0)
        k = vae.fit_range_shift(z.to(DEV), 1 / 0.18215)
        assert k > 0 and vae.range_shift == k
        _check_decode(vae, bad, vcfg, z, f"case ({case}) mode {mode}")


def test_overflowing_decoder_at_sd15_width():
    vcfg = configs.SD15_VAE
    vsd = weights.synthetic_state_dict(weights.vae_param_shapes(vcfg), 43, fp16_values=True)
    z = torch.randn((1, 4, 32, 32), generator=torch.Generator().manual_seed(5)) * 0.3
    bad, key, s = _overflowing("b", vsd, vcfg, z / 0.18215)
    vae = AutoencoderKL(vcfg, bad, DEV)
    k = vae.fit_range_shift(z.to(DEV), 1 / 0.18215)
    print(f"SD-1.5 width, 256^2, {key} x {s:g}: fitted k = {k}")
    _check_decode(vae, bad, vcfg, z, "SD-1.5 width case (b)")


def test_sampler_with_a_shifted_decoder(tiny):
    from ldiffusion_amd._lib import NonFiniteError
    ucfg, vcfg, usd, vsd = tiny["ucfg"], tiny["vcfg"], tiny["usd"], tiny["vsd"]
    g = torch.Generator().manual_seed(1234)
    x = torch.rand((2, 3, 64, 64), generator=g)
    ctx = torch.randn((1, 6, ucfg["cross_attention_dim"]), generator=g) * 0.5
    z = torch.randn((2, 4, 8, 8), generator=torch.Generator().manual_seed(11)) * 0.3
    bad, key, s = _overflowing("b", vsd, vcfg, z / 0.18215)
    vae = AutoencoderKL(vcfg, bad, DEV)
    sampler = LaplaceSampler(StableDiffusionImg2ImgPipeline(vae, tiny["unet"]))
    out0 = sampler.sample(x.to(DEV), ctx.to(DEV), 5)
    lat0 = out0["latents"].clone()
    with pytest.raises(NonFiniteError):
        sampler.check_finite()
    # the sampler decodes the latents of every pass: fit k on the oracle's, one step of margin for the device's (which differ by rounding)
    ref = op.sample_v6(op.OraclePipeline(op.OracleUNet(usd, ucfg), op.OracleVAE(bad, vcfg)), x, ctx, 5)
    k = min(16, vae.fit_range_shift(torch.cat(list(ref["latents"])).to(DEV), 1 / 0.18215) + 2)
    vae.set_range_shift(k)
    out = sampler.sample(x.to(DEV), ctx.to(DEV), 5)
    sampler.check_finite()
    assert torch.equal(out["latents"], lat0), "the UNet and the encoder do not depend on the decoder's range shift"
    fd = np.abs(out["features"].cpu().numpy().astype(int) - ref["features"].astype(int))
    rd = np.abs(out["rgb"].cpu().numpy().astype(int) - ref["rgb_u8"][:, -1].astype(int))
    print(f"sampler, case (b), k = {k}: luma max diff {fd.max()} ({(fd > 0).mean():.4f} of the pixels), rgb max diff {rd.max()}")
    assert fd.max() <= 1 and rd.max() <= 1


def test_healthy_weights_at_the_bench_shape_are_unchanged_by_a_shift():
    """SD-1.5 width, B = 8, 512^2, 5 passes, deferred join (the benchmark's configuration) on healthy synthetic weights."""
    ucfg, vcfg = configs.SD15_UNET, configs.SD15_VAE
    usd = weights.synthetic_state_dict(weights.unet_param_shapes(ucfg), 42, fp16_values=True)
    vsd = weights.synthetic_state_dict(weights.vae_param_shapes(vcfg), 43, fp16_values=True)
    vae = AutoencoderKL(vcfg, vsd, DEV)
    sampler = LaplaceSampler(StableDiffusionImg2ImgPipeline(vae, UNet2DConditionModel(ucfg, usd, DEV)))
    g = torch.Generator().manual_seed(1234)
    x = torch.rand((8, 3, 512, 512), generator=g).to(DEV)
    ctx = (torch.randn((1, 6, 768), generator=g) * 0.5).to(DEV)
    sampler.set_overlap(2)

    def run(k):
        vae.set_range_shift(k)
        with reached(vae._lib) as names:
            out = sampler.sample(x, ctx, 5)
            sampler.join()
        sampler.check_finite()
        enc = vae.encode(x[:2]).latent_dist.mean.clone()
        return {n: t.clone() for n, t in out.items()}, matrix_kernels(names), enc

    o0, n0, e0 = run(0)
    o4, n4, e4 = run(4)
    o0b, _, e0b = run(0)
    sampler.set_overlap(1)
    assert torch.equal(o4["latents"], o0["latents"])
    fd = (o4["features"].int() - o0["features"].int()).abs()
    rd = (o4["rgb"].int() - o0["rgb"].int()).abs()
    print(f"bench shape, k = 4 vs 0: {int((fd > 0).sum())} of {fd.numel()} luma values and {int((rd > 0).sum())} of {rd.numel()} rgb values differ "
          f"(max {fd.max().item()} / {rd.max().item()}); kernels only at k = 4: {sorted(n4 - n0)}")
    assert fd.max() <= 1 and rd.max() <= 1
    assert n0 <= n4, f"kernels reached at k = 0 but not at k = 4: {sorted(n0 - n4)}"
    for n in ("latents", "features", "rgb"):
        assert torch.equal(o0b[n], o0[n]), f"back at k = 0: {n} differs from the first run"
    assert torch.equal(e0, e4) and torch.equal(e0, e0b), "the encoder must not depend on the decoder's range shift"


def test_range_shift_api(tiny):
    from ldiffusion_amd._lib import NonFiniteError
    vcfg, vsd = tiny["vcfg"], tiny["vsd"]
    vae = AutoencoderKL(vcfg, vsd, DEV, range_shift=3)
    assert vae.range_shift == 3
    assert vae.set_range_shift(0) is vae and vae.range_shift == 0
    for k in (-1, 17):
        with pytest.raises(ValueError):
            vae.set_range_shift(k)
    assert vae.range_shift == 0
    assert vae._lib.ldiff_vae_set_range_shift(vae._h, 17) == -1
    z = torch.randn((2, 4, 8, 8), generator=torch.Generator().manual_seed(11)) * 0.3
    assert vae.fit_range_shift(z.to(DEV), 1 / 0.18215) == 0          # healthy: no shift needed
    bad, _, _ = _overflowing("b", vsd, vcfg, z / 0.18215)
    badvae = AutoencoderKL(vcfg, bad, DEV)
    with pytest.raises(NonFiniteError):
        badvae.fit_range_shift(z.to(DEV), 1 / 0.18215, k_max=0)
    assert badvae.range_shift == 0
    badvae.check_finite()


def test_shifted_bias_follows_k(tiny):
    """The pre-scaled bias copies (shortcut and upsampler convs of a shifted decoder) are kept per layer and keyed on k: decodes at k = 0, 4, 2 on one
    handle, and the last equals, bit for bit, the first decode of a fresh handle set to k = 2."""
    vcfg, vsd = tiny["vcfg"], tiny["vsd"]
    z = (torch.randn((2, 4, 8, 8), generator=torch.Generator().manual_seed(12)) * 0.3).to(DEV)
    vae = AutoencoderKL(vcfg, vsd, DEV)
    got = {}
    for k in (0, 4, 2):
        got[k] = vae.set_range_shift(k)._decode(z, 1 / 0.18215, want_sample=True)[0].clone()
    vae.check_finite()
    fresh = AutoencoderKL(vcfg, vsd, DEV, range_shift=2)
    ref = fresh._decode(z, 1 / 0.18215, want_sample=True)[0].clone()
    fresh.check_finite()
    assert torch.equal(got[2], ref), "k = 2 after k = 4 differs from a fresh handle at k = 2: a bias copy scaled for another k was reused"
