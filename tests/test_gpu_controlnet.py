"""GPU (-m gpu): the ControlNet of the multimodal sampler (V7) on the HIP library -- the conditioning-embedding conv kernel alone, the stand-alone
forward, the forward attached to the UNet (eager and graph replay), SD-v1.5 width, V7 end to end, and the non-finite detector.

References: tests/controlnet_ref.py (plain-torch restatement assembled from oracle.unet's blocks) in float32 for parity, float64 for the kernel.
Synthetic weights come from weights.synthetic_state_dict(..., fp16_values=True), whose zero convs are NOT zero: a zero-initialised ControlNet
would pass every parity test with a dead trunk."""
import contextlib
import ctypes as C
import types

import pytest
import torch
import torch.nn.functional as F

import kernel_routing
from controlnet_ref import controlnet_forward, skip_shapes
from kernel_routing import check_route
from ldiffusion_amd import _lib, configs, weights
from ldiffusion_amd.models import AutoencoderKL, ControlNetModel, UNet2DConditionModel
from ldiffusion_amd.pipeline import StableDiffusionImg2ImgPipeline
from oracle import noise_post, pipeline as op
from oracle.unet import unet_forward

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ZERO_CONVS = ("controlnet_down_blocks.", "controlnet_mid_block.")


@contextlib.contextmanager
def reached(lib):
    """kernel_routing.reached with the new kernel's profiler stem counted in (its inventory lists the kernels that existed before this one)."""
    old = kernel_routing.ROUTED_PREFIXES
    kernel_routing.ROUTED_PREFIXES = old + ("condconv<",)
    try:
        with kernel_routing.reached(lib) as names:
            yield names
    finally:
        kernel_routing.ROUTED_PREFIXES = old


def rel_err(got, ref):
    """max|got - ref| / max|ref|: the project's error relative to the range of the compared tensor (tests/test_gpu_models.py)."""
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), "non-finite output"
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-6)).item()


@pytest.fixture(scope="module")
def tiny():
    ucfg, vcfg, ccfg = configs.TINY_UNET, configs.TINY_VAE, configs.TINY_CONTROLNET
    usd = weights.synthetic_state_dict(weights.unet_param_shapes(ucfg), 42, fp16_values=True)
    vsd = weights.synthetic_state_dict(weights.vae_param_shapes(vcfg), 43, fp16_values=True)
    csd = weights.synthetic_state_dict(weights.controlnet_param_shapes(ccfg), 44, fp16_values=True)
    return dict(ucfg=ucfg, vcfg=vcfg, ccfg=ccfg, usd=usd, vsd=vsd, csd=csd, unet=UNet2DConditionModel(ucfg, usd, DEV), vae=AutoencoderKL(vcfg, vsd, DEV),
                cn=ControlNetModel(ccfg, csd, DEV))


# ---- 4. the conditioning-embedding conv kernel alone ---------------------------------------------------------------------------------------
EMB_LAYERS = [(8, 16, 1), (16, 16, 1), (16, 32, 2), (32, 32, 1), (32, 96, 2), (96, 96, 1), (96, 256, 2)]   # (stored Cin, Cout, stride); 3 real inputs are stored as 8
SIZES = [(1, 37, 45), (3, 16, 64), (1, 9, 131), (3, 21, 19)]   # (B, H, W): odd sizes (stride 2 on odd maps, partial tiles both ways), one whole tile row, a wide strip


def run_cond_conv(lib, x, w, bias, stride, silu, cond_conv):
    """x [B, Cin, H, W], w [Cout, Cin, 3, 3] (values already fp16-representable), bias fp32 -> ([B, Cout, Ho, Wo] as stored, kernel names reached)."""
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    xd = x.permute(0, 2, 3, 1).contiguous().to(torch.float16).to(DEV)
    wd = w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).contiguous().to(torch.float16).to(DEV)
    bd = bias.float().to(DEV)
    y = torch.full((B, Ho, Wo, Cout), float("nan"), dtype=torch.float16, device=DEV)
    a = _lib.ConvArgs()
    a.x, a.C1, a.B, a.Hin, a.Win, a.Hout, a.Wout = xd.data_ptr(), Cin, B, H, W, Ho, Wo
    a.ks, a.stride, a.pad_t, a.pad_l = 3, stride, 1, 1
    a.w, a.N, a.Nrows, a.n_real, a.bias = wd.data_ptr(), Cout, Cout, Cout, bd.data_ptr()
    a.y, a.ldy = y.data_ptr(), Cout
    a.silu_out, a.cond_conv = int(silu), cond_conv
    with reached(lib) as names:
        _lib.check(lib.ldiff_op_conv(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return y.permute(0, 3, 1, 2).cpu(), names


@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("cin,cout,stride", EMB_LAYERS)
def test_cond_conv_kernel_against_float64(lib, cin, cout, stride, silu):
    """Every layer shape of the embedding on the new kernel, through ldiff_op_conv.  Reference: float64 conv (+ SiLU) on the fp16-rounded operands
    the kernel sees.  Bound, per element (the error model tests/test_gpu_kernels.py assert_conv_close derives for this project's conv kernels):
    2^-11 |ref| for the output's fp16 rounding + 1e-5 max|ref| for the fp32 accumulation order; SiLU's slope is at most 1.1, so behind it the
    second term is 1.1e-5 max|ref|.  Every element of every case is compared."""
    name = f"condconv<{cin}x{cout},s{stride}" + (",silu>" if silu else ">")
    for B, H, W in SIZES:
        g = torch.Generator().manual_seed(cin * 1000 + cout * 10 + stride + H)
        x = torch.randn((B, cin, H, W), generator=g).to(torch.float16).float()
        w = (torch.randn((cout, cin, 3, 3), generator=g) * (1.0 / (9 * cin)) ** 0.5).to(torch.float16).float()
        bias = torch.randn(cout, generator=g) * 0.1
        got, names = run_cond_conv(lib, x, w, bias, stride, silu, 1)   # (cond_conv = 1: the kernel itself, whatever the routing rule says about layer and size)
        check_route(names, name, f"cond conv {cin}->{cout} s{stride} B={B} {H}x{W} silu={silu}")
        ref = F.conv2d(x.double(), w.double(), bias.double(), stride=stride, padding=1)
        if silu:
            ref = F.silu(ref)
        assert got.shape == ref.shape
        assert torch.isfinite(got).all()
        m = ref.abs().max().item()
        err = (got.double() - ref).abs()
        tol = 2.0 ** -11 * ref.abs() + (1.1e-5 if silu else 1e-5) * m
        print(f"[cond-conv] {name} B={B} {H}x{W}: max err {err.max().item() / m:.2e} of max|ref|, {(err / tol).max().item():.2f} of the bound")
        bad = err > tol
        assert not bad.any(), f"{name} B={B} {H}x{W}: {int(bad.sum())}/{bad.numel()} out of tolerance, max err {err.max().item():.3e} (max|ref| {m:.3f})"


@pytest.mark.parametrize("cin,cout,stride", [(16, 16, 1), (16, 32, 2), (8, 16, 1)])
def test_cond_conv_kernel_exact_on_integers(lib, cin, cout, stride):
    """Fragment maps: small integers (every product and sum exact in fp16 / fp32), asymmetric in both operands -- a transposed or permuted
    fragment cannot cancel out.  The result must be the integer convolution exactly."""
    g = torch.Generator().manual_seed(cin + cout + stride)
    x = torch.randint(-3, 4, (2, cin, 19, 35), generator=g).float()
    w = torch.randint(-2, 3, (cout, cin, 3, 3), generator=g).float()
    bias = torch.randint(-5, 6, (cout,), generator=g).float()
    got, names = run_cond_conv(lib, x, w, bias, stride, False, 1)
    check_route(names, f"condconv<{cin}x{cout},s{stride}>", "integer case")
    assert torch.equal(got.double(), F.conv2d(x.double(), w.double(), bias.double(), stride=stride, padding=1))


def test_cond_conv_routing_rules(lib):
    """The executors' choice (cond_conv = 0): a plain launch of an embedding shape keeps the route it had before the kernel existed; a launch that asks
    for the SiLU epilogue reaches the kernel where it was measured faster (64 workgroups up, never 96 -> 256), and is refused wherever the kernel does
    not take it (no silent other path)."""
    g = torch.Generator().manual_seed(1)
    x, w, bias = torch.randn((2, 16, 64, 128), generator=g), torch.randn((16, 16, 3, 3), generator=g) * 0.1, torch.zeros(16)
    _, names = run_cond_conv(lib, x, w, bias, 1, False, 0)
    assert names and not any(n.startswith("condconv<") for n in names), names
    _, names = run_cond_conv(lib, x, w, bias, 1, True, 0)            # 2 x 8 x 4 = 64 workgroups
    check_route(names, "condconv<16x16,s1,silu>", "executors' choice, 64 workgroups")
    with pytest.raises(ValueError, match="silu_out"):
        run_cond_conv(lib, x[:1], w, bias, 1, True, 0)                # 32 workgroups: the executors route this layer elsewhere and run the SiLU themselves
    with pytest.raises(ValueError, match="silu_out"):
        run_cond_conv(lib, torch.randn((8, 96, 64, 64), generator=g), torch.randn((256, 96, 3, 3), generator=g) * 0.03, torch.zeros(256), 2, True, 0)
    with pytest.raises(ValueError, match="silu_out"):
        run_cond_conv(lib, x, w, bias, 1, True, -1)
    with pytest.raises(ValueError, match="silu_out"):   # 64 -> 64 is not an embedding shape
        run_cond_conv(lib, torch.randn((1, 64, 8, 8), generator=g), torch.randn((64, 64, 3, 3), generator=g) * 0.1, torch.zeros(64), 1, True, 0)


# ---- 5. stand-alone forward --------------------------------------------------------------------------------------------------------------
def _inputs(B, h, w, L, dim, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((B, 4, h, w), generator=g), torch.randn((1, L, dim), generator=g) * 0.5, torch.rand((B, 3, 8 * h, 8 * w), generator=g))


@pytest.mark.parametrize("t", [751, 1])
def test_controlnet_forward_tiny(tiny, t):
    """B = 2, 16 x 16 latents, 128 x 128 conditioning image: each of the 13 tensors against the fp32 restatement, error over the tensor's range.
    Bound 1.2e-3: what the tiny UNet tests hold at the default precision for these same blocks."""
    x, ctx, cond = _inputs(2, 16, 16, 6, 64, 80 + t)
    cn = tiny["cn"]
    out = cn(x.to(DEV), torch.tensor(t), ctx.to(DEV), cond.to(DEV))
    with torch.no_grad():
        rd, rm = controlnet_forward(tiny["csd"], tiny["ccfg"], x, t, ctx, cond)
        rd64, rm64 = controlnet_forward(tiny["csd"], tiny["ccfg"], x, t, ctx, cond, dtype=torch.float64)
    assert len(out.down_block_res_samples) == 12 and [tuple(v.shape) for v in out.down_block_res_samples] == skip_shapes(tiny["ccfg"], 2, 16, 16)
    errs = [rel_err(g_, r_) for g_, r_ in zip(out.down_block_res_samples + [out.mid_block_res_sample], rd + [rm])]
    own = [rel_err(r_, r64) for r_, r64 in zip(rd + [rm], rd64 + [rm64])]
    print(f"controlnet tiny t={t}: rel err of the 13 tensors " + " ".join(f"{e:.2e}" for e in errs))
    print(f"   the fp32 restatement against its float64 form      " + " ".join(f"{e:.2e}" for e in own))
    assert max(errs) <= 1.2e-3
    pair = cn(sample=x.to(DEV), timestep=t, encoder_hidden_states=ctx.to(DEV), controlnet_cond=cond.to(DEV), return_dict=False)   # the reference's call (segmentor.py:357-363)
    assert isinstance(pair, tuple) and all(torch.equal(a, b) for a, b in zip(pair[0] + [pair[1]], out.down_block_res_samples + [out.mid_block_res_sample]))
    half = cn(x.to(DEV), t, ctx.to(DEV), cond.to(DEV), conditioning_scale=0.5)
    eh = [rel_err(g_, 0.5 * r_) for g_, r_ in zip(half.down_block_res_samples + [half.mid_block_res_sample], rd + [rm])]
    print(f"   conditioning_scale = 0.5                           " + " ".join(f"{e:.2e}" for e in eh))
    assert max(eh) <= 1.2e-3
    with pytest.raises(ValueError, match="guess_mode"):
        cn(x.to(DEV), t, ctx.to(DEV), cond.to(DEV), guess_mode=True)
    with pytest.raises(ValueError):
        cn(x.to(DEV), t, ctx.to(DEV), cond[:, :, :64].to(DEV))   # conditioning image that is not 8 x the latents


def test_controlnet_zeroed_zero_convs_give_exact_zeros(tiny):
    sd = {k: (torch.zeros_like(v) if k.startswith(ZERO_CONVS) else v) for k, v in tiny["csd"].items()}
    cn = ControlNetModel(tiny["ccfg"], sd, DEV)
    x, ctx, cond = _inputs(2, 16, 16, 6, 64, 90)
    down, mid = cn(x.to(DEV), 501, ctx.to(DEV), cond.to(DEV), return_dict=False)
    assert all(not v.any() for v in down + [mid])


# ---- 6. attached forward -----------------------------------------------------------------------------------------------------------------
def test_attached_forward_against_oracle(tiny):
    """unet(x, t, ctx, controlnet_cond=c) with the ControlNet attached against the oracle UNet fed with the restatement's residuals; the detached
    two-call path (stand-alone forward + thirteen tensors) on the same inputs meets the same bound.  1.2e-3: test_unet_controlnet_additional_residuals."""
    unet, cn = tiny["unet"], tiny["cn"]
    for t, scale in ((501, 1.0), (1, 0.5)):
        x, ctx, cond = _inputs(2, 16, 16, 6, 64, 100 + t)
        before = unet(x.to(DEV), t, ctx.to(DEV)).sample.clone()
        with torch.no_grad():
            rd, rm = controlnet_forward(tiny["csd"], tiny["ccfg"], x, t, ctx, cond, conditioning_scale=scale)
            ref = unet_forward(tiny["usd"], tiny["ucfg"], x, t, ctx, down_block_additional_residuals=rd, mid_block_additional_residual=rm).sample
        unet.attach_controlnet(cn, conditioning_scale=scale)
        try:
            got = unet(x.to(DEV), t, ctx.to(DEV), controlnet_cond=cond.to(DEV)).sample.clone()
            with pytest.raises(ValueError, match="controlnet_cond"):
                unet(x.to(DEV), t, ctx.to(DEV))
        finally:
            unet.detach_controlnet()
        down, mid = cn(x.to(DEV), t, ctx.to(DEV), cond.to(DEV), conditioning_scale=scale, return_dict=False)
        two = unet(x.to(DEV), t, ctx.to(DEV), down_block_additional_residuals=down, mid_block_additional_residual=mid).sample
        ea, ed = rel_err(got, ref), rel_err(two, ref)
        print(f"attached t={t} scale={scale}: rel err {ea:.3e}; detached two-call path {ed:.3e}; the ControlNet moves the output by {rel_err(before, ref):.3e}")
        assert ea <= 1.2e-3 and ed <= 1.2e-3
        assert not torch.equal(got, before)
        assert torch.equal(unet(x.to(DEV), t, ctx.to(DEV)).sample, before)   # detached: what it was before attaching
        with pytest.raises(ValueError, match="attached"):
            unet(x.to(DEV), t, ctx.to(DEV), controlnet_cond=cond.to(DEV))


def test_attach_refuses_a_mismatched_controlnet(tiny):
    ccfg = dict(tiny["ccfg"], block_out_channels=[64, 128, 128, 128])
    other = ControlNetModel(ccfg, weights.synthetic_state_dict(weights.controlnet_param_shapes(ccfg), 5, fp16_values=True), DEV)
    with pytest.raises(ValueError, match=r"64,128,256,256.*64,128,128,128"):
        tiny["unet"].attach_controlnet(other)
    with pytest.raises(TypeError):
        tiny["unet"].attach_controlnet(object())


# ---- 7. graph ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
def test_attached_graph_replay_equals_eager(tiny):
    """With set_graph(True) the attached forward (the ControlNet's launches included) is captured on its second use: replays equal the eager launches
    bit for bit over samples and timesteps, and a new conditioning image, a new scale and a detach must not replay stale state."""
    unet, cn = tiny["unet"], tiny["cn"]
    g = torch.Generator().manual_seed(150)
    xs = [torch.randn((2, 4, 16, 16), generator=g).to(DEV) for _ in range(3)]
    ctx = (torch.randn((1, 6, 64), generator=g) * 0.5).to(DEV)
    conds = [torch.rand((2, 3, 128, 128), generator=g).to(DEV) for _ in range(2)]
    plain = unet(xs[0], 751, ctx).sample.clone()
    try:
        unet.set_graph(False)
        ref = {}
        for scale in (1.0, 0.5):
            unet.attach_controlnet(cn, conditioning_scale=scale)
            for c in range(2):
                for i in range(3):
                    for t in (751, 1):
                        ref[(scale, c, i, t)] = unet(xs[i], t, ctx, controlnet_cond=conds[c]).sample.clone()
        assert not torch.equal(ref[(1.0, 0, 0, 751)], ref[(1.0, 1, 0, 751)]) and not torch.equal(ref[(1.0, 0, 0, 751)], ref[(0.5, 0, 0, 751)])
        unet.set_graph(True)
        r0 = unet.graph_replays
        for rep in range(2):
            for scale in (1.0, 0.5):
                unet.attach_controlnet(cn, conditioning_scale=scale)
                for c in range(2):
                    for i in range(3):
                        for t in (751, 1):
                            assert torch.equal(unet(xs[i], t, ctx, controlnet_cond=conds[c]).sample, ref[(scale, c, i, t)]), (rep, scale, c, i, t)
        assert unet.graph_replays - r0 >= 24, unet.graph_replays - r0
        nodes_attached = unet.graph_nodes
        unet.detach_controlnet()
        for _ in range(3):
            assert torch.equal(unet(xs[0], 751, ctx).sample, plain)
        assert 0 < unet.graph_nodes < nodes_attached
        unet.attach_controlnet(cn, conditioning_scale=1.0)
        for _ in range(3):
            assert torch.equal(unet(xs[2], 1, ctx, controlnet_cond=conds[1]).sample, ref[(1.0, 1, 2, 1)])
    finally:
        unet.detach_controlnet()
        unet.set_graph(True)


# ---- 8. SD-v1.5 width --------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(1500)
def test_sd15_width_controlnet_against_oracle():
    """SD-v1.5 widths (361.3 M + 859.5 M parameters, synthetic weights), B = 1, 32 x 32 latents, 256 x 256 conditioning image (V7's own size).
    1e-3: the bound of test_sd15_width_unet_and_vae_against_oracle."""
    ucfg, ccfg = configs.SD15_UNET, configs.SD15_CONTROLNET
    usd = weights.synthetic_state_dict(weights.unet_param_shapes(ucfg), 42, fp16_values=True)
    csd = weights.synthetic_state_dict(weights.controlnet_param_shapes(ccfg), 44, fp16_values=True)
    x, ctx, cond = _inputs(1, 32, 32, 6, 768, 2)
    unet, cn = UNet2DConditionModel(ucfg, usd, DEV), ControlNetModel(ccfg, csd, DEV)
    down, mid = cn(x.to(DEV), 501, ctx.to(DEV), cond.to(DEV), return_dict=False)
    unet.attach_controlnet(cn)
    got = unet(x.to(DEV), 501, ctx.to(DEV), controlnet_cond=cond.to(DEV)).sample
    unet.check_finite()
    with torch.no_grad():
        rd, rm = controlnet_forward(csd, ccfg, x, 501, ctx, cond)
        ref = unet_forward(usd, ucfg, x, 501, ctx, down_block_additional_residuals=rd, mid_block_additional_residual=rm).sample
    errs = [rel_err(g_, r_) for g_, r_ in zip(down + [mid], rd + [rm])]
    e_u = rel_err(got, ref)
    print("SD15 width: rel err of the 13 tensors " + " ".join(f"{e:.2e}" for e in errs) + f"; attached UNet output {e_u:.3e}")
    assert max(errs) <= 1e-3 and e_u <= 1e-3


# ---- 9. V7 end to end --------------------------------------------------------------------------------------------------------------------
class _Tok:
    def __call__(self, prompts, **kw):
        ids = [[49406, 320, 24857, 5471, 49407] for _ in prompts]
        return {"input_ids": torch.tensor(ids) if kw.get("return_tensors") == "pt" else ids}


class _Enc:
    def __init__(self, hidden):
        self.config = types.SimpleNamespace(hidden_size=hidden)
        self.table = torch.randn((49408, hidden), generator=torch.Generator().manual_seed(99)) * 0.5

    def __call__(self, ids):
        return {"last_hidden_state": self.table.to(ids.device)[ids]}

    def to(self, *a, **k):
        return self

    def eval(self):
        return self


@pytest.mark.timeout(900)
def test_multimodal_augment_v7_with_the_hip_controlnet(tiny, monkeypatch):
    """Segmentor.ldiffusion_augment_for_multimodal (V7: RGB + depth) with models.ControlNetModel as its `controlnet`, against the same chain on the
    oracle's graphs and the restatement, with the same random draws.  4e-3: the bound of the existing V7 mirror test for a decoded image."""
    from ldiffusion_amd import models as M
    from ldiffusion_amd.segmentor import Segmentor
    g = torch.Generator().manual_seed(170)
    B = 2
    rgb, dtm = torch.rand((B, 3, 200, 180), generator=g), torch.rand((B, 1, 200, 180), generator=g)
    eps32 = torch.finfo(torch.float32).eps
    u = torch.rand((B, 4, 32, 32), generator=g) * (2 - eps32) + (eps32 - 1)
    post = torch.randn((B, 4, 32, 32), generator=g)
    calls = {"i": 0}

    def fake_sample(self, generator=None):
        i = calls["i"]; calls["i"] += 1
        return self.mean + self.std * post[i:i + 1].to(self.mean.device)
    monkeypatch.setattr(M._LatentDist, "sample", fake_sample)
    unet, vae, cn = tiny["unet"], tiny["vae"], tiny["cn"]
    pipe = StableDiffusionImg2ImgPipeline(vae, unet, tokenizer=_Tok(), text_encoder=_Enc(48))
    seg = Segmentor(None, None, "cell", 3)
    torch.manual_seed(2)
    got = seg.ldiffusion_augment_for_multimodal(rgb, dtm, pipe, unet, vae, cn, B, DEV, u=u)
    assert unet._controlnet is None   # attached for the call only
    proj = seg.ldiffusion_proj
    ovae, F_ = op.OracleVAE(tiny["vsd"], tiny["vcfg"]), torch.nn.functional
    rgb2, dtm2 = F_.interpolate(rgb, size=(256, 256), mode="bilinear", align_corners=False), F_.interpolate(dtm, size=(256, 256), mode="bilinear", align_corners=False)
    emb = _Enc(48).table[torch.tensor([[49406, 320, 24857, 5471, 49407]])]
    ctx = F_.linear(emb, proj.weight.detach().cpu(), proj.bias.detach().cpu())
    worst = 0.0
    with torch.no_grad():
        for i in range(B):
            mom = ovae.encode(rgb2[i:i + 1]).latent_dist
            lat = (mom.mean + torch.exp(0.5 * torch.clamp(mom.logvar, -30.0, 20.0)) * post[i:i + 1]) * 0.18215
            depth = F_.interpolate(dtm2[i:i + 1], size=(32, 32), mode="bilinear", align_corners=False).repeat(1, 4, 1, 1)
            noisy = lat + noise_post.laplace_from_uniform(u[i:i + 1], 0.0, 1.0) * depth
            down, mid = controlnet_forward(tiny["csd"], tiny["ccfg"], noisy, 1, ctx, dtm2[i:i + 1].repeat(1, 3, 1, 1))
            eps = unet_forward(tiny["usd"], tiny["ucfg"], noisy, 1, ctx, down_block_additional_residuals=down, mid_block_additional_residual=mid).sample
            ref = ovae.decode((noisy - eps * depth) / 0.18215).sample[0].permute(1, 2, 0)
            assert got[i].shape == (256, 256, 3)
            worst = max(worst, rel_err(torch.from_numpy(got[i]), ref))
    print(f"V7 with the HIP ControlNet: reconstruction rel err vs the oracle chain {worst:.3e}")
    assert worst <= 4e-3


# ---- 10. non-finite detector -------------------------------------------------------------------------------------------------------------
def test_check_finite_reports_an_overflowing_embedding(tiny):
    """The embedding's last two weights scaled by 2^8 and 2^17 (each still an fp16 value): the embedding's output leaves fp16's range (a numerical
    overflow, as tests/test_gpu_range_shift.py makes them), the sum with conv_in carries it into the trunk's first GroupNorm, whose statistics set the flag."""
    sd = dict(tiny["csd"])
    sd["controlnet_cond_embedding.blocks.5.weight"] = sd["controlnet_cond_embedding.blocks.5.weight"] * 2.0 ** 8
    sd["controlnet_cond_embedding.conv_out.weight"] = sd["controlnet_cond_embedding.conv_out.weight"] * 2.0 ** 17
    assert all(torch.isfinite(v.to(torch.float16)).all() for v in sd.values())
    bad = ControlNetModel(tiny["ccfg"], sd, DEV)
    x, ctx, cond = _inputs(2, 16, 16, 6, 64, 200)
    tiny["cn"](x.to(DEV), 501, ctx.to(DEV), cond.to(DEV))
    tiny["cn"].check_finite()                                   # the healthy network reports nothing
    bad(x.to(DEV), 501, ctx.to(DEV), cond.to(DEV))
    with pytest.raises(_lib.NonFiniteError):
        bad.check_finite()
    bad.check_finite()                                          # reported once, then cleared
    unet = tiny["unet"]
    unet.attach_controlnet(bad)
    try:
        unet(x.to(DEV), 501, ctx.to(DEV), controlnet_cond=cond.to(DEV))
        with pytest.raises(_lib.NonFiniteError):
            unet.check_finite()
    finally:
        unet.detach_controlnet()
    bad.check_finite()
    out = unet(x.to(DEV), 501, ctx.to(DEV)).sample
    unet.check_finite()
    assert torch.isfinite(out).all()
