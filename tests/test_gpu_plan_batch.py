"""-m gpu: the plan batch (ldiff_*_set_plan_batch, DESIGN.md "Batch invariance").  With n >= 1 every batch-dependent choice of a launch -- kernel, tile,
split-K count, unit shape, GroupNorm form -- is made as if the batch were n, so an image submitted in ANY batch B <= n gets the same bits.

Every comparison here is torch.equal: no tolerances.  The handles are built once per module; each test puts the plan batch back to 0."""
import ctypes as C

import pytest
import torch

from kernel_routing import reached
from ldiffusion_amd import _lib, configs, parallel, tiling, weights
from ldiffusion_amd.models import AutoencoderKL, ControlNetModel, UNet2DConditionModel
from ldiffusion_amd.pipeline import LaplaceSampler, StableDiffusionImg2ImgPipeline, probe_argmax_mask

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def sp():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def apart(a, b):
    """max |a - b| / max |b| (printed figures only; nothing is asserted with it)"""
    return ((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-6)).item()


# ---- the handles ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    """The `tiny` configuration of tests/test_gpu_models.py (same seeds), plus the ControlNet of tests/test_gpu_controlnet.py."""
    ucfg, vcfg, ccfg = configs.TINY_UNET, configs.TINY_VAE, configs.TINY_CONTROLNET
    usd = weights.synthetic_state_dict(weights.unet_param_shapes(ucfg), 42, fp16_values=True)
    vsd = weights.synthetic_state_dict(weights.vae_param_shapes(vcfg), 43, fp16_values=True)
    csd = weights.synthetic_state_dict(weights.controlnet_param_shapes(ccfg), 44, fp16_values=True)
    unet, vae = UNet2DConditionModel(ucfg, usd, DEV), AutoencoderKL(vcfg, vsd, DEV)
    pipe = StableDiffusionImg2ImgPipeline(vae, unet)
    return dict(unet=unet, vae=vae, pipe=pipe, sampler=LaplaceSampler(pipe), cn=ControlNetModel(ccfg, csd, DEV))


@pytest.fixture(scope="module")
def sd_unet():
    """SD-v1.5 widths and head dims, one layer per block (half the load time): the row counts at which the fill-the-chip thresholds flip between B = 1 and 8."""
    cfg = dict(configs.SD15_UNET, layers_per_block=1)
    return UNet2DConditionModel(cfg, weights.synthetic_state_dict(weights.unet_param_shapes(cfg), 42, fp16_values=True), DEV)


@pytest.fixture(scope="module")
def sd_unet_case(sd_unet):
    """The inputs of the SD-width pass and its B = 8 output under n = 8, shared by the tests that need it."""
    g = torch.Generator().manual_seed(21)
    x = torch.randn((8, 4, 64, 64), generator=g).to(DEV)
    ctx = (torch.randn((1, 77, 768), generator=g) * 0.5).to(DEV)
    sd_unet.set_plan_batch(8)
    try:
        full = sd_unet(x, 501, ctx).sample.clone()
    finally:
        sd_unet.set_plan_batch(0)
    assert torch.isfinite(full).all()
    return dict(x=x, ctx=ctx, full=full)


def tiles_and_probe():
    g = torch.Generator().manual_seed(6)   # the ROI of test_tiles_are_independent_units
    roi = torch.rand((3, 128, 128), generator=g).to(DEV)
    ctx = (torch.randn((1, 6, 64), generator=g) * 0.5).to(DEV)
    tiles, _ = tiling.split_tiles(roi, (64, 64), 1.0)
    assert tiles.shape[0] == 4
    W = (torch.randn((3, 5), generator=g) * 0.05).to(DEV)
    b = (torch.randn(3, generator=g) * 0.1).to(DEV)
    return tiles, ctx, W, b


def sample(tiny, tiles, ctx, W, b):
    o = tiny["sampler"].sample(tiles.contiguous(), ctx, 5)
    out = {k: o[k].clone() for k in ("latents", "features", "rgb")}
    assert out["features"].shape[1] == W.shape[1]   # one luma plane per pass
    out["mask"] = probe_argmax_mask(out["features"], W, b).clone()
    return out


def assert_same(got, want, lo, hi, what):
    for k in ("latents", "features", "rgb", "mask"):
        assert torch.equal(got[k], want[k][lo:hi]), f"{what}: {k} of tiles {lo}:{hi} differ from the batch of {want[k].shape[0]}"


# ---- 1. tiny config, whole sampler --------------------------------------------------------------------------------------------------------------------
def test_tiny_sampler_is_batch_invariant(tiny):
    """128 x 128 ROI cut into four 64 x 64 tiles, 5 passes, n = 4: every tile alone and the shards (0:1, 1:4) and (0:3, 3:4) give the B = 4 run's latents,
    features, rgb and probe masks bit for bit.  Then n = 1 with batches of 1: they agree with each other (repeated, in another order).
    On the parent commit the same comparison in default mode ends 3.2e-4 of the latents' range apart (printed below for this tree)."""
    tiles, ctx, W, b = tiles_and_probe()
    pipe = tiny["pipe"]
    try:
        full0 = sample(tiny, tiles, ctx, W, b)
        one0 = sample(tiny, tiles[0:1], ctx, W, b)
        fd = (one0["features"].int() - full0["features"][0:1].int()).abs()
        print(f"default mode (n = 0), tile 0 alone vs inside the batch of 4: latents {apart(one0['latents'], full0['latents'][0:1]):.2e} of range apart, "
              f"luma != on {(fd > 0).float().mean().item():.4f} of the values")
        pipe.set_plan_batch(4)
        full = sample(tiny, tiles, ctx, W, b)
        assert torch.isfinite(full["latents"]).all()
        for i in range(4):
            assert_same(sample(tiny, tiles[i:i + 1], ctx, W, b), full, i, i + 1, "n = 4, tile alone")
        for lo, hi in [(0, 1), (1, 4), (0, 3), (3, 4)]:
            assert_same(sample(tiny, tiles[lo:hi], ctx, W, b), full, lo, hi, "n = 4, shard")
        for r in range(2):   # and the shards parallel.shard_range hands two ranks
            lo, hi = parallel.shard_range(4, r, 2)
            assert_same(sample(tiny, tiles[lo:hi], ctx, W, b), full, lo, hi, "n = 4, rank shard")
        pipe.set_plan_batch(1)
        first = [sample(tiny, tiles[i:i + 1], ctx, W, b) for i in range(4)]
        for i in reversed(range(4)):
            assert_same(sample(tiny, tiles[i:i + 1], ctx, W, b), first[i], 0, 1, "n = 1, tile alone again")
    finally:
        pipe.set_plan_batch(0)


# ---- 2. n = B keeps the default plans ------------------------------------------------------------------------------------------------------------------
def test_plan_batch_equal_to_the_batch_keeps_the_default_plans_tiny(tiny):
    tiles, ctx, W, b = tiles_and_probe()
    default = sample(tiny, tiles, ctx, W, b)
    try:
        tiny["pipe"].set_plan_batch(4)
        assert_same(sample(tiny, tiles, ctx, W, b), default, 0, 4, "n = B = 4 against n = 0")
    finally:
        tiny["pipe"].set_plan_batch(0)


def test_plan_batch_equal_to_the_batch_keeps_the_default_plans_sd_width(sd_unet, sd_unet_case):
    c = sd_unet_case
    assert sd_unet.plan_batch == 0
    default = sd_unet(c["x"], 501, c["ctx"]).sample
    assert torch.equal(default, c["full"]), "SD-width UNet pass at B = 8: n = 8 differs from the default mode (n = 0)"


# ---- 3. SD-v1.5 widths, one UNet pass -----------------------------------------------------------------------------------------------------------------
def test_sd_width_unet_pass_is_batch_invariant(lib, sd_unet, sd_unet_case):
    """Widths 320/640/1280/1280, 64 x 64 latents, L = 77, precision 1, n = 8: image 0 alone, image 7 alone and images 2:5 as B = 3 equal the B = 8 run per
    image, and the B = 1 and B = 8 runs launch the same set of conv / GEMM / attention kernels."""
    c = sd_unet_case
    x, ctx, full = c["x"], c["ctx"], c["full"]
    try:
        d1 = sd_unet(x[0:1].contiguous(), 501, ctx).sample
        print(f"default mode (n = 0), SD-width UNet pass, image 0 at B = 1 vs inside B = 8: {apart(d1, full[0:1]):.2e} of the output's range apart "
              f"({(d1 != full[0:1]).float().mean().item():.3f} of the values differ)")
        sd_unet.set_plan_batch(8)
        for lo, hi in [(0, 1), (7, 8), (2, 5)]:
            got = sd_unet(x[lo:hi].contiguous(), 501, ctx).sample
            assert torch.equal(got, full[lo:hi]), f"n = 8: images {lo}:{hi} as B = {hi - lo} differ from the B = 8 run ({apart(got, full[lo:hi]):.2e} of range)"
        with reached(lib) as names1:
            y1 = sd_unet(x[0:1].contiguous(), 501, ctx).sample
        with reached(lib) as names8:
            y8 = sd_unet(x, 501, ctx).sample
        assert names1 == names8, f"n = 8: kernels only at B = 1 {sorted(names1 - names8)}, only at B = 8 {sorted(names8 - names1)}"
        assert torch.equal(y8, full) and torch.equal(y1, full[0:1])   # (profiled = eager launches: the graph replays nothing else)
    finally:
        sd_unet.set_plan_batch(0)


# ---- 4. VAE at full width ---------------------------------------------------------------------------------------------------------------------------
def test_sd_width_vae_is_batch_invariant():
    """512 x 512 images, n = 4, default precisions (encoder 2, decoder 0): moments, decoder sample and the uint8 image of B = 4 against image 0 alone and
    images 1:4; one decode under range shift 4."""
    vcfg = configs.SD15_VAE
    vae = AutoencoderKL(vcfg, weights.synthetic_state_dict(weights.vae_param_shapes(vcfg), 43, fp16_values=True), DEV)
    g = torch.Generator().manual_seed(31)
    img = torch.rand((4, 3, 512, 512), generator=g).to(DEV)
    vae.set_plan_batch(4)

    def enc(x):
        d = vae.encode(x.contiguous()).latent_dist
        return d.mean.clone(), d.logvar.clone()

    def dec(z):
        s, _, rgb = vae._decode(z.contiguous(), 1.0, want_sample=True, want_rgb=True)
        return s.clone(), rgb.clone()

    mean, logvar = enc(img)
    assert torch.isfinite(mean).all()
    z = mean
    s4, rgb4 = dec(z)
    assert torch.isfinite(s4).all()
    for lo, hi in [(0, 1), (1, 4)]:
        m, lv = enc(img[lo:hi])
        assert torch.equal(m, mean[lo:hi]) and torch.equal(lv, logvar[lo:hi]), f"encode: images {lo}:{hi} differ from the batch of 4"
        s, rgb = dec(z[lo:hi])
        assert torch.equal(s, s4[lo:hi]), f"decode: sample of images {lo}:{hi} differs from the batch of 4 ({apart(s, s4[lo:hi]):.2e} of range)"
        assert torch.equal(rgb, rgb4[lo:hi]), f"decode: uint8 image of images {lo}:{hi} differs from the batch of 4"
    vae.set_range_shift(4)
    s4k, rgb4k = dec(z)
    s, rgb = dec(z[0:1])
    assert torch.equal(s, s4k[0:1]) and torch.equal(rgb, rgb4k[0:1]), "decode under range shift 4: image 0 alone differs from the batch of 4"
    vae.check_finite()
    with pytest.raises(ValueError, match=r"batch 5 exceeds the plan batch 4"):
        vae.encode(torch.zeros((5, 3, 64, 64), device=DEV))


# ---- 5. ControlNet attached -----------------------------------------------------------------------------------------------------------------------------
def test_attached_controlnet_is_batch_invariant(tiny):
    unet, cn = tiny["unet"], tiny["cn"]
    g = torch.Generator().manual_seed(41)
    x = torch.randn((4, 4, 16, 16), generator=g).to(DEV)
    ctx = (torch.randn((1, 6, 64), generator=g) * 0.5).to(DEV)
    cond = torch.rand((4, 3, 128, 128), generator=g).to(DEV)
    try:
        unet.set_plan_batch(4)
        cn.set_plan_batch(4)
        unet.attach_controlnet(cn, conditioning_scale=0.7)
        full = unet(x, 501, ctx, controlnet_cond=cond).sample.clone()
        assert torch.isfinite(full).all()
        for i in (0, 2):
            got = unet(x[i:i + 1].contiguous(), 501, ctx, controlnet_cond=cond[i:i + 1].contiguous()).sample
            assert torch.equal(got, full[i:i + 1]), f"attached ControlNet, n = 4: image {i} alone differs from the batch of 4"
        cn.set_plan_batch(2)   # the two handles must agree at forward time
        with pytest.raises(ValueError, match=r"plan batch is 2, the UNet's 4"):
            unet(x[0:2].contiguous(), 501, ctx, controlnet_cond=cond[0:2].contiguous())
        cn.set_plan_batch(4)
        unet.detach_controlnet()
        down4, mid4 = cn(x, 501, ctx, cond, 0.7, return_dict=False)   # the diffusers surface: thirteen tensors
        down1, mid1 = cn(x[3:4].contiguous(), 501, ctx, cond[3:4].contiguous(), 0.7, return_dict=False)
        for a, b4 in zip(down1 + [mid1], down4 + [mid4]):
            assert torch.equal(a, b4[3:4]), "ControlNet forward, n = 4: image 3 alone differs from the batch of 4"
    finally:
        unet.detach_controlnet()
        unet.set_plan_batch(0)
        cn.set_plan_batch(0)


# ---- 6. refusals and graph hygiene ---------------------------------------------------------------------------------------------------------------------
def test_refusals_and_graph_hygiene(lib, tiny):
    unet = tiny["unet"]
    g = torch.Generator().manual_seed(51)
    x = torch.randn((3, 4, 16, 16), generator=g).to(DEV)
    ctx = (torch.randn((1, 6, 64), generator=g) * 0.5).to(DEV)
    try:
        for h in (unet, tiny["vae"], tiny["cn"]):
            with pytest.raises(ValueError, match=r"n = -1 must be >= 0"):
                h.set_plan_batch(-1)
        unet.set_plan_batch(2)
        with pytest.raises(ValueError, match=r"batch 3 exceeds the plan batch 2"):
            unet(x, 501, ctx)
        with pytest.raises(ValueError, match=r"batch 3 exceeds the plan batch 2"):
            unet(x, 501, ctx.expand(3, -1, -1).contiguous())   # (refused at set_context already)
        # C ABI: a context projected under another plan batch is a state error until set_context is called again
        e = ctx.float().contiguous()
        _lib.check(lib.ldiff_unet_set_context(unet._h, _lib.ptr(e), 1, 6, sp()))
        _lib.check(lib.ldiff_unet_set_plan_batch(unet._h, 3))
        out = torch.empty_like(x)
        rc = lib.ldiff_unet_forward(unet._h, _lib.ptr(x), 3, 16, 16, 501.0, _lib.ptr(out), sp())
        assert rc == -3 and b"call set_context again" in lib.ldiff_last_error()
        # a change of n: the next forwards run eagerly, capture and replay again, with the new plans
        unet.set_plan_batch(3)
        a = [unet(x, 501, ctx).sample.clone() for _ in range(3)]
        assert unet.graph_nodes > 0
        replays = unet.graph_replays
        unet.set_plan_batch(1)
        assert unet.plan_batch == 1
        b = [unet(x[1:2].contiguous(), 501, ctx).sample.clone() for _ in range(3)]   # eager, captured + replayed, replayed
        assert unet.graph_nodes > 0 and unet.graph_replays == replays + 2
        unet.set_graph(False)
        ref = unet(x[1:2].contiguous(), 501, ctx).sample.clone()   # n = 1, launched eagerly
        unet.set_graph(True)
        assert all(torch.equal(t, ref) for t in b), "after a change of n the replayed graph does not compute the new n's results"
        assert torch.equal(a[0], a[1]) and torch.equal(a[1], a[2])
        unet.set_plan_batch(3)
        assert torch.equal(unet(x, 501, ctx).sample, a[0])
    finally:
        unet.set_graph(True)
        unet.set_plan_batch(0)


# ---- 7. op level: one case per family whose choice moves --------------------------------------------------------------------------------------------------
def op_conv(lib, x, w, bias, ks, plan_batch):
    """x [B, H, W, Cin] f16, w [N, ks ks Cin] f16 (device) -> y [B, H, W, N] f16, kernel names"""
    B, H, W, Cin = x.shape
    N = w.shape[0]
    y = torch.full((B, H, W, N), float("nan"), dtype=torch.float16, device=DEV)
    a = _lib.ConvArgs()
    a.x, a.C1, a.B, a.Hin, a.Win, a.Hout, a.Wout = x.data_ptr(), Cin, B, H, W, H, W
    a.ks, a.stride, a.pad_t, a.pad_l = ks, 1, ks // 2, ks // 2
    a.w, a.N, a.Nrows, a.n_real, a.bias = w.data_ptr(), N, N, N, bias.data_ptr()
    a.y, a.ldy = y.data_ptr(), N
    with reached(lib) as names:
        _lib.check(lib.ldiff_op_conv_pb(C.byref(a), plan_batch, sp()))
    torch.cuda.synchronize()
    return y, names


@pytest.mark.parametrize("name,H,W,Cin,N,ks", [
    ("conv3x3_8x8_level_splitk", 8, 8, 1280, 1280, 3),        # 3 x 3 at the 8 x 8 level: the split-K count follows the workgroup count
    ("conv1x1_k2560_m64_per_image", 8, 8, 2560, 1280, 1),     # 1 x 1 over the concat input, M = 64 B: LDS-DMA GEMM tile and split
    ("linear_level0_m4096_per_image", 64, 64, 320, 320, 1),   # level-0 linear, M = 4096 B: dataflow GEMM vs LDS-DMA GEMM, and the dataflow unit shape
])
def test_op_conv_rows_of_an_image_do_not_depend_on_the_batch(lib, name, H, W, Cin, N, ks):
    g = torch.Generator().manual_seed(H + Cin + ks)
    x = torch.randn((8, H, W, Cin), generator=g).to(torch.float16).to(DEV)
    w = (torch.randn((N, ks * ks * Cin), generator=g) * (1.0 / (ks * ks * Cin)) ** 0.5).to(torch.float16).to(DEV)
    bias = (torch.randn(N, generator=g) * 0.1).to(DEV)
    y8, n8 = op_conv(lib, x, w, bias, ks, 8)
    y1, n1 = op_conv(lib, x[3:4].contiguous(), w, bias, ks, 8)
    d8, _ = op_conv(lib, x, w, bias, ks, 0)
    d1, m1 = op_conv(lib, x[3:4].contiguous(), w, bias, ks, 0)
    print(f"[{name}] plan_batch = 8: B = 8 {sorted(n8)}, B = 1 {sorted(n1)}; default B = 1 {sorted(m1)}, image 3 differs from the default B = 8 run on "
          f"{(d1 != d8[3:4]).float().mean().item():.4f} of the values")
    assert torch.isfinite(y8.float()).all()
    assert n1 == n8, f"{name}: plan_batch = 8 reaches {sorted(n1)} at B = 1 and {sorted(n8)} at B = 8"
    assert torch.equal(y1, y8[3:4]), f"{name}: image 3 at B = 1 differs from its rows in the B = 8 launch"
    assert torch.equal(d8, y8), f"{name}: plan_batch = B differs from the default plans"
    with pytest.raises(ValueError, match=r"batch 8 .* plan batch of 4"):
        op_conv(lib, x, w, bias, ks, 4)


def test_op_gn_stats_form_does_not_depend_on_the_batch(lib):
    """C = 320, H W = 4096, 32 groups: B groups = 32 at B = 1 (one launch) and 256 at B = 8 (partial + finalize)."""
    g = torch.Generator().manual_seed(61)
    Cc, HW, G = 320, 4096, 32
    x = torch.randn((8, HW, Cc), generator=g).to(torch.float16).to(DEV)
    gamma, beta = (torch.rand(Cc, generator=g) + 0.5).to(DEV), (torch.randn(Cc, generator=g) * 0.1).to(DEV)

    def run(xs, pb):
        B = xs.shape[0]
        scale, shift = torch.empty((B, Cc), device=DEV), torch.empty((B, Cc), device=DEV)
        lib.ldiff_prof_set_filter(None)
        _lib.prof_collect()
        lib.ldiff_prof_enable(1)
        try:
            _lib.check(lib.ldiff_op_gn_stats_pb(_lib.ptr(xs), Cc, Cc, 0, None, 0, 0, 0, B, HW, G, 1e-5, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(scale), _lib.ptr(shift), pb, sp()))
            torch.cuda.synchronize()
            form = {r["name"] for r in _lib.prof_collect() if r["name"].startswith("gn_stats")}
        finally:
            lib.ldiff_prof_enable(0)
        return scale, shift, form

    s8, t8, f8 = run(x, 8)
    s1, t1, f1 = run(x[3:4].contiguous(), 8)
    _, _, d1 = run(x[3:4].contiguous(), 0)
    assert f8 == f1 == {"gn_stats<2>"} and d1 == {"gn_stats<1>"}, (f8, f1, d1)
    assert torch.equal(s1, s8[3:4]) and torch.equal(t1, t8[3:4])
    with pytest.raises(ValueError, match=r"batch 8 under a plan batch of 2"):
        run(x, 2)


@pytest.mark.parametrize("Lk", [77, 16])   # the prompt's length, and a short one: the short-K/V kernel is chosen by B x query blocks
def test_op_cross_attention_does_not_depend_on_the_batch(lib, Lk):
    g = torch.Generator().manual_seed(70 + Lk)
    B, heads, d, Lq = 8, 8, 40, 4096
    Cc = heads * d
    q = torch.randn((B, Lq, Cc), generator=g).to(torch.float16).to(DEV)
    kv = (torch.randn((1, Lk, 2 * Cc), generator=g) * 0.5).to(torch.float16).to(DEV)   # one prompt for the batch

    def run(qs, pb):
        n = qs.shape[0]
        o = torch.full((n, Lq, Cc), float("nan"), dtype=torch.float16, device=DEV)
        with reached(lib) as names:
            _lib.check(lib.ldiff_op_attention_pb(_lib.ptr(qs), Cc, _lib.ptr(kv), 2 * Cc, C.c_void_p(kv.data_ptr() + 2 * Cc), 2 * Cc, _lib.ptr(o), Cc, n, heads, Lq, Lk, d,
                                                 Lq * Cc, 0, Lq * Cc, d ** -0.5, pb, sp()))
        torch.cuda.synchronize()
        return o, names

    o8, n8 = run(q, 8)
    o1, n1 = run(q[3:4].contiguous(), 8)
    _, m1 = run(q[3:4].contiguous(), 0)
    print(f"[cross-attention Lk = {Lk}] plan_batch = 8: B = 8 {sorted(n8)}, B = 1 {sorted(n1)}; default B = 1 {sorted(m1)}")
    assert torch.isfinite(o8.float()).all()
    assert n1 == n8 and torch.equal(o1, o8[3:4])
    with pytest.raises(ValueError, match=r"batch 8 under a plan batch of 2"):
        run(q, 2)
