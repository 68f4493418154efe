"""CPU (-m "not gpu"): the oracle against the committed golden fixtures.

third_party fixtures (tests/golden/{laplace_torch,luma_pil,round_numpy}.npz, reference_*.{json,npz}) PIN the oracle:
they were produced by installed torch / Pillow / numpy and by the reference's own python (scripts/gen_golden*.py).
restatement fixtures (pndm.npz, tiny_graph.npz) freeze the restated diffusers semantics (diffusers itself is absent:
parity for those functions is unpinned, see oracle/__init__.py).
Fixtures compared bit for bit against the oracle's own float arithmetic are taken and checked under oracle/pinned_cpu.py.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ldiffusion_amd import configs, weights
from oracle import metrics, noise_post, pipeline as op, schedule, unet as ounet
from oracle.pinned_cpu import PINNED_CPU_ENV

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def gold(name):
    return np.load(os.path.join(GOLD, name), allow_pickle=False)


def pinned_cpu_numerics(test):
    """Runs `test` in a fresh pytest process under PINNED_CPU_ENV (the environment its fixture was generated in): torch's CPU
    kernels round differently per CPU vendor, instruction set and thread count, and the environment must precede torch's load."""
    @functools.wraps(test)
    def run():
        if all(os.environ.get(k) == v for k, v in PINNED_CPU_ENV.items()):
            return test()
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
            "-m", "pytest", "-q", "-p", "no:cacheprovider", f"{os.path.abspath(__file__)}::{test.__name__}"]
        r = subprocess.run(cmd, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), env=dict(os.environ, **PINNED_CPU_ENV), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, f"{test.__name__} under {PINNED_CPU_ENV}:\n{r.stdout[-6000:]}\n{r.stderr[-2000:]}"
    return run


# ---------------------------------------------------------------- pinned against third-party code
def test_laplace_matches_torch_distributions_bit_exact():
    z = gold("laplace_torch.npz")
    assert str(z["provenance"]).startswith("third_party")
    for scale, u, sample in zip(z["scale"], z["u"], z["sample"]):
        got = noise_post.laplace_from_uniform(torch.from_numpy(u), 0.0, torch.tensor(float(scale)))
        assert np.array_equal(got.numpy(), sample)
    # and live against the installed torch (same global-generator draw)
    torch.manual_seed(11)
    ref = torch.distributions.Laplace(0, torch.tensor(0.5)).sample((64,))
    torch.manual_seed(11)
    u = torch.empty(64).uniform_(torch.finfo(torch.float32).eps - 1, 1)
    assert torch.equal(noise_post.laplace_from_uniform(u, 0.0, torch.tensor(0.5)), ref)


def test_laplace_forward_noise_scale_and_edges():
    abar = schedule.alphas_cumprod()
    for t, s in [(1, 0.0413), (251, 0.573), (501, 0.851), (751, 0.972)]:   # SURVEY R7 spot values
        assert abs(float(torch.sqrt(1 - abar[t])) - s) < 5e-4
    z0 = torch.zeros(4)
    u = torch.tensor([0.0, 0.5, -0.5, torch.finfo(torch.float32).eps - 1])
    x = noise_post.laplace_forward_noise(z0, abar[501], u)
    assert x[0] == 0 and x[1] > 0 and x[2] == -x[1] and torch.isfinite(x).all() and x[3] < -10


def test_luma_matches_pillow_bit_exact():
    z = gold("luma_pil.npz")
    assert np.array_equal(noise_post.luma_u8(z["rgb"]), z["luma"])
    from PIL import Image
    rgb = np.random.default_rng(5).integers(0, 256, size=(33, 17, 3), dtype=np.uint8)
    assert np.array_equal(noise_post.luma_u8(rgb), np.array(Image.fromarray(rgb).convert("L")))


def test_uint8_rounding_matches_numpy_half_even():
    z = gold("round_numpy.npz")
    assert np.array_equal(noise_post.to_uint8(z["x"]), z["u8"])
    assert noise_post.to_uint8(np.array([0.5 / 255, 1.5 / 255, 2.5 / 255], np.float32)).tolist() == [0, 2, 2]


def test_metrics_and_luts_match_reference_python():
    with open(os.path.join(GOLD, "reference_metrics.json")) as f:
        fx = json.load(f)
    for c in fx["metrics"]:
        B, Cc, H, W = c["shape"]
        g = torch.Generator().manual_seed(c["seed"])
        logits = torch.randn((B, Cc, H, W), generator=g)
        target = torch.randint(0, Cc, (B, H, W), generator=g)
        if c["force_class0"]:
            target[:] = 0
            logits[:, 0] += 100
        per, avg = metrics.micro_dice(logits, target, Cc)
        assert per.tolist() == pytest.approx(c["dice_per_class"], abs=1e-7) and float(avg) == pytest.approx(c["dice"], abs=1e-7)
        miou, iou = metrics.mean_iou_and_per_class(logits, target, Cc)
        assert miou == pytest.approx(c["miou"], abs=1e-12) and {str(k): v for k, v in iou.items()} == c["iou_per_class"]
        assert metrics.pixel_accuracy(logits, target, Cc)[0] == pytest.approx(c["pixel_accuracy"], abs=1e-12)
        assert metrics.frequency_weighted_iou(logits, target, Cc) == pytest.approx(c["fw_iou"], abs=1e-7)
    assert {str(k): v for k, v in metrics.PIXEL_TO_LABEL.items()} == fx["luts"]["pixel_to_label"]
    assert {str(k): v for k, v in metrics.PIXEL_TO_LABEL_CELL.items()} == fx["luts"]["pixel_to_label_cell"]
    assert metrics.map_mask(np.array(fx["luts"]["map_mask_in"], np.uint8)).tolist() == fx["luts"]["map_mask_out"]


@pinned_cpu_numerics
def test_one_pass_sampler_restatement_equals_reference_loop():
    """Segmentor.ldiffusion_augment (reference code, segmentor.py:86-112) was run on the oracle's objects to make the fixture;
    the oracle's own restatement of that loop must reproduce it: same UNet timesteps, same decoded images."""
    from PIL import Image
    z = gold("reference_augment_v3.npz")
    ucfg, vcfg = configs.TINY_UNET, configs.TINY_VAE
    usd = weights.synthetic_state_dict(weights.unet_param_shapes(ucfg), 42)
    vsd = weights.synthetic_state_dict(weights.vae_param_shapes(vcfg), 43)
    pipe = op.OraclePipeline(op.OracleUNet(usd, ucfg), op.OracleVAE(vsd, vcfg))
    g = torch.Generator().manual_seed(int(z["inputs_seed"]))
    inputs = torch.rand((2, 3, 64, 64), generator=g)
    table = torch.randn((49408, int(z["hidden"])), generator=torch.Generator().manual_seed(99)) * 0.5
    emb = table[torch.tensor([z["ids"].tolist()])]                                  # text_encoder(ids)["last_hidden_state"]
    ctx = torch.nn.functional.linear(emb, torch.from_numpy(z["proj_weight"]), torch.from_numpy(z["proj_bias"]))  # segmentor.py:60
    outs = []
    for i in range(2):                                                              # the reference loops one image at a time
        r = op.sample_one_pass(pipe, inputs[i:i + 1], ctx)
        im = Image.fromarray(r["rgb_u8"][0]).resize((1024, 1024), Image.BILINEAR)   # Resize((1024,1024)) + ToTensor (segmentor.py:87-90,108)
        outs.append(torch.from_numpy(np.asarray(im, np.float32) / 255.0).permute(2, 0, 1))
    out = torch.stack(outs)
    assert pipe.unet.calls == z["unet_calls"].tolist() == [1, 1]                    # set_timesteps(1) -> one pass at t = 1 per image
    assert list(out.shape) == z["out_shape"].tolist()
    assert np.array_equal(torch.nn.functional.avg_pool2d(out, 64).numpy(), z["pooled"])


@pinned_cpu_numerics
def test_v4_restatement_equals_reference_copy_or_convert_image():
    """utils.copy_or_convert_image (reference code, utils.py:176-208; sampler variant V4) was run on the oracle's objects to make the
    fixture (scripts/gen_golden_v4.py), with the text-alignment wrapper of its call site around the UNet.  Pinned: the wrapper is handed
    embeddings of width 1280 (the function's own nn.Linear(768, 1280)), falls back to its cached embeddings (F12), ONE UNet pass at t = 1 on
    a 128 x 128 latent of the image resized to 1024 x 1024 and ImageNet-normalised, and the PNG holds decode_latents -> numpy_to_pil of the
    stepped latents.  The oracle's restatement of that loop must reproduce the PNG bit for bit."""
    from PIL import Image
    z = gold("reference_v4.npz")
    assert z["calls_t"].tolist() == [1] and z["calls_fallback"].tolist() == [True] and z["calls_given_dim"].tolist() == [1280]
    assert z["calls_sample_shape"].tolist() == [[1, 4, 128, 128]] and z["base_unet_calls"].tolist() == [1] and bool(z["plain_copy"])
    ucfg, vcfg = configs.TINY_UNET, configs.TINY_VAE
    usd = weights.synthetic_state_dict(weights.unet_param_shapes(ucfg), 42)
    vsd = weights.synthetic_state_dict(weights.vae_param_shapes(vcfg), 43)
    pipe = op.OraclePipeline(op.OracleUNet(usd, ucfg), op.OracleVAE(vsd, vcfg))
    h, w = z["image_hw"].tolist()
    img = Image.fromarray((torch.rand((h, w, 3), generator=torch.Generator().manual_seed(int(z["image_seed"]))) * 255).to(torch.uint8).numpy(), "RGB")
    cached = torch.randn((1, 5, ucfg["cross_attention_dim"]), generator=torch.Generator().manual_seed(int(z["cached_seed"]))) * 0.5
    x = torch.from_numpy(np.asarray(img.resize((1024, 1024), Image.BILINEAR), np.float32) / 255.0).permute(2, 0, 1)[None]
    x = (x - torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)) / torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    out = op.sample_one_pass(pipe, x, cached)["rgb_u8"][0]
    assert list(out.shape) == z["out_shape"].tolist() and pipe.unet.calls == [1]
    assert np.array_equal(out[480:544, 480:544], z["crop"])
    assert np.array_equal(torch.nn.functional.avg_pool2d(torch.from_numpy(out.copy()).permute(2, 0, 1).float()[None], 64)[0].numpy(), z["pooled"])


# ---------------------------------------------------------------- restated diffusers semantics (regression fixtures)
@pinned_cpu_numerics
def test_pndm_schedule_and_trajectory():
    z = gold("pndm.npz")
    sch = schedule.PNDMOracle()
    assert np.array_equal(sch.alphas_cumprod.numpy(), z["alphas_cumprod"])
    a = sch.alphas_cumprod
    for t, v in [(0, 0.999150), (1, 0.998296), (251, 0.672151), (501, 0.274999), (751, 0.055719)]:   # SURVEY R6 spot values
        assert abs(float(a[t]) - v) < 2e-6
    for n in (1, 2, 4, 5, 10, 19, 20):
        assert np.array_equal(schedule.plms_timesteps(n), z[f"timesteps_{n}"])
    assert schedule.plms_timesteps(1).tolist() == [1]
    assert schedule.plms_timesteps(4).tolist() == [751, 501, 501, 251, 1]
    assert schedule.plms_timesteps(5).tolist() == [801, 601, 601, 401, 201, 1]
    assert len(schedule.plms_timesteps(20)) == 21
    sch.set_timesteps(4)
    x = torch.from_numpy(z["traj_x"][0])
    for i, t in enumerate(sch.timesteps):
        x = sch.step(torch.from_numpy(z["traj_eps"][i]), t, x).prev_sample
        assert np.allclose(x.numpy(), z["traj_x"][i + 1], rtol=0, atol=1e-6)
    with pytest.raises(ZeroDivisionError):
        schedule.plms_timesteps(0)


def test_plms_second_call_reuses_first_sample():
    """counter==1 branch: timestep is rewound and the update restarts from the sample of the first call."""
    sch = schedule.PNDMOracle()
    sch.set_timesteps(4)
    x0 = torch.ones(3)
    e0, e1 = torch.full((3,), 0.5), torch.full((3,), -0.25)
    x1 = sch.step(e0, 751, x0).prev_sample
    x2 = sch.step(e1, 501, x1).prev_sample
    sc, ce, _, _ = sch.prev_sample_coeffs(751, 501)
    assert torch.allclose(x2, sc * x0 - ce * (e0 + e1) / 2, atol=1e-6)


def test_timestep_embedding_layout():
    e = ounet.timestep_embedding(torch.tensor([0, 7]), 320, True, 0)
    assert e.shape == (2, 320)
    assert torch.all(e[0, :160] == 1) and torch.all(e[0, 160:] == 0)         # flip_sin_to_cos: [cos | sin]
    assert abs(float(e[1, 0]) - float(torch.cos(torch.tensor(7.0)))) < 1e-6  # freq_0 = 1


def test_param_counts_match_sd15():
    u = weights.param_count(weights.unet_param_shapes(configs.SD15_UNET))
    v = weights.vae_param_shapes(configs.SD15_VAE)
    enc = weights.param_count({k: s for k, s in v.items() if k.startswith(("encoder", "quant"))})
    dec = weights.param_count({k: s for k, s in v.items() if k.startswith(("decoder", "post"))})
    assert (u, enc, dec) == (859_520_964, 34_163_664, 49_490_199)           # published SD-v1.5 sizes


def test_tiny_graph_regression():
    z = gold("tiny_graph.npz")
    ucfg, vcfg = configs.TINY_UNET, configs.TINY_VAE
    usd = weights.synthetic_state_dict(weights.unet_param_shapes(ucfg), 42)
    vsd = weights.synthetic_state_dict(weights.vae_param_shapes(vcfg), 43)
    pipe = op.OraclePipeline(op.OracleUNet(usd, ucfg), op.OracleVAE(vsd, vcfg))
    x, ctx, lat = (torch.from_numpy(z[k]) for k in ("images", "ctx", "lat_in"))
    close = lambda a, b: np.abs(a - b).max() <= 2e-5 * max(1.0, np.abs(b).max())   # thread-count dependent fp32 summation order
    assert close(pipe.unet(lat, 501, ctx).sample.numpy(), z["unet_eps_t501"])
    d = pipe.vae.encode(x).latent_dist
    assert close(torch.cat([d.mean, d.logvar], 1).numpy(), z["vae_moments"])
    assert close(pipe.vae.decode(lat).sample.numpy(), z["vae_decode"])
    s5 = op.sample_v6(pipe, x, ctx, 5)
    assert pipe.unet.calls[-5:] == z["v6_unet_calls"].tolist() == [751, 501, 501, 251, 1]
    assert close(s5["latents"][-1].numpy(), z["v6_latents"][-1])
    assert (np.abs(s5["features"].astype(int) - z["v6_features"].astype(int)) > 1).mean() < 1e-3


def test_sampler_edge_cases():
    ucfg, vcfg = configs.TINY_UNET, configs.TINY_VAE
    usd = weights.synthetic_state_dict(weights.unet_param_shapes(ucfg), 42)
    vsd = weights.synthetic_state_dict(weights.vae_param_shapes(vcfg), 43)
    pipe = op.OraclePipeline(op.OracleUNet(usd, ucfg), op.OracleVAE(vsd, vcfg))
    x = torch.rand((1, 3, 64, 64))                    # smallest patch the 4-level UNet accepts (8x8 latents)
    ctx = torch.randn((1, 1, 64))                     # shortest possible context
    r = op.sample_v6(pipe, x, ctx, 3)
    assert r["features"].shape == (1, 3, 64, 64) and r["features"].dtype == np.uint8
    with pytest.raises(ZeroDivisionError):            # N=1 -> set_timesteps(0), as the reference would (pixel_latent_vector.py:74)
        op.sample_v6(pipe, x, ctx, 1)
    lat = pipe.vae.encode(x).latent_dist
    assert torch.equal(lat.sample(noise=torch.zeros_like(lat.mean)), lat.mean)
    g = torch.Generator().manual_seed(3)
    u = [noise_post.laplace_uniform_draw((1, 4, 8, 8), g) for _ in range(2)]
    f = op.laplace_features_v5(pipe, x, ctx, 1, u, out_hw=16)   # ldiffusion.py:198: N=5 -> set_timesteps(1) -> one pass
    assert f["gray"].shape == (1, 1, 16, 16)


def test_weights_layout_roundtrip(tmp_path):
    cfg = configs.TINY_VAE
    sd = weights.synthetic_state_dict(weights.vae_param_shapes(cfg), 1)
    weights.save_model_dir(str(tmp_path / "vae"), cfg, sd)
    cfg2, sd2 = weights.load_model_dir(str(tmp_path / "vae"))
    assert cfg2["block_out_channels"] == cfg["block_out_channels"] and all(torch.equal(sd[k], sd2[k]) for k in sd)
    old = {k.replace(".to_q.", ".query.").replace(".to_k.", ".key.").replace(".to_v.", ".value.").replace(".to_out.0.", ".proj_attn."): v
           for k, v in sd.items()}
    assert set(weights.normalize_vae_keys(old)) == set(sd)
    with pytest.raises(FileNotFoundError):
        os.remove(tmp_path / "vae" / weights.WEIGHTS_NAME)
        weights.load_model_dir(str(tmp_path / "vae"))
    with pytest.raises(ValueError):
        configs.validate_unet_config(dict(configs.SD15_UNET, block_out_channels=[100, 200, 400, 400]))


def test_tiling_matches_reference_helpers():
    """oracle/tiling.py and the product's host-side tiling against the outputs of the reference's own nnU-Net helpers
    (tests/golden/reference_tiling.json, scripts/gen_golden_tiling.py)."""
    import json
    from ldiffusion_amd import tiling as ptiling
    from oracle import tiling as otiling
    with open(os.path.join(GOLD, "reference_tiling.json")) as f:
        d = json.load(f)
    for c in d["steps"]:
        assert otiling.steps_for_sliding_window(c["image_size"], c["tile_size"], c["tile_step_size"]) == c["steps"]
        assert ptiling.compute_steps_for_sliding_window(c["image_size"], c["tile_size"], c["tile_step_size"]) == c["steps"]
    assert otiling.tile_origins((1024, 1024), (512, 512), 1.0) == [(0, 0), (0, 512), (512, 0), (512, 512)]   # BASELINE configs[3]
    g = np.array(d["gaussian"]["values"])
    assert np.abs(otiling.gaussian_importance((64, 48), 0.125, 10) - g).max() < 2e-6
    assert np.abs(ptiling.compute_gaussian((64, 48), 0.125, 10, torch.float64).numpy() - g).max() < 2e-6
    # merge: product (torch) == oracle (numpy) on random overlapping tiles; edge cases
    rng = np.random.default_rng(0)
    origins = otiling.tile_origins((96, 80), (64, 48), 0.5)
    tiles = rng.standard_normal((len(origins), 3, 64, 48)).astype(np.float32)
    a = otiling.merge_logits(tiles, origins, (96, 80))
    b = ptiling.merge_tile_logits(torch.from_numpy(tiles), origins, (96, 80)).numpy()
    assert np.abs(a - b).max() < 1e-5
    with pytest.raises(ValueError):
        ptiling.compute_steps_for_sliding_window((100, 100), (128, 128), 0.5)
    with pytest.raises(ValueError):
        ptiling.compute_steps_for_sliding_window((256, 256), (128, 128), 0.0)
    with pytest.raises(RuntimeError):
        ptiling.merge_tile_logits(torch.zeros((1, 2, 8, 8)), [(0, 0)], (16, 16))
    t, o = ptiling.split_tiles(torch.arange(3 * 16 * 16, dtype=torch.float32).reshape(3, 16, 16), (8, 8), 1.0)
    assert t.shape == (4, 3, 8, 8) and o == [(0, 0), (0, 8), (8, 0), (8, 8)] and torch.equal(t[3], torch.arange(3 * 256.).reshape(3, 16, 16)[:, 8:, 8:])


def _sw_network(W):
    def network(x):   # the stand-in head of scripts/gen_golden_sliding_window.py: integer weights (exact on any device) + a column ramp
        ramp = torch.arange(x.shape[-1], dtype=torch.float32, device=x.device) * 0.125
        return torch.einsum("oc,bchw->bohw", W.to(x.device), x.float()) + ramp[None, None, None, :]
    return network


def test_sliding_window_predictor_matches_reference_code_bit_for_bit():
    """ldiffusion_amd.tiling.predict_sliding_window_return_logits against the outputs of the REFERENCE's own
    nnUNetPredictor._internal_predict_sliding_window_return_logits / _internal_maybe_mirror_and_predict / compute_gaussian
    (predict_from_raw_data.py:505-589, run in the build container by scripts/gen_golden_sliding_window.py): tile order, mirroring
    TTA, the float16 importance map (zeros lifted after the cast) and the float16 accumulation must agree bit for bit."""
    from ldiffusion_amd import tiling
    z = np.load(os.path.join(GOLD, "reference_sliding_window.npz"))
    g16 = tiling.compute_gaussian((32, 32), 1.0 / 8, 10)            # default dtype = the reference's float16
    assert g16.dtype == torch.float16 and torch.equal(g16, torch.from_numpy(z["gaussian_f16_32x32"]))
    assert float(g16.min()) > 0
    net = _sw_network(torch.from_numpy(z["head_weight"]))
    for tag in "abc":
        th, tw, step, mm = z[tag + "_cfg"]
        mirror = None if mm < 0 else tuple(i for i in range(2) if (int(mm) >> i) & 1)
        got = tiling.predict_sliding_window_return_logits(torch.from_numpy(z[tag + "_image"]), net, 4, (int(th), int(tw)), float(step), True, mirror)
        assert got.dtype == torch.float16 and torch.equal(got, torch.from_numpy(z[tag + "_logits_f16"])), tag
        assert len(tiling.tile_origins(tuple(z[tag + "_image"].shape[1:]), (int(th), int(tw)), float(step))) == int(z[tag + "_n_slicers"]) or tag == "c"
    # an image smaller than the tile is zero padded around its centre and the padding is cut off again
    small = torch.from_numpy(z["a_image"])[:, :20, :27]
    out = tiling.predict_sliding_window_return_logits(small, net, 4, (32, 32), 0.5, True, (0, 1))
    assert out.shape == (4, 20, 27) and torch.isfinite(out.float()).all()
    with pytest.raises(RuntimeError, match="inf"):
        tiling.predict_sliding_window_return_logits(torch.full((3, 32, 32), 6e4), lambda x: x[:, :1] * 10.0, 1, (32, 32), 1.0, True, None)


def test_oracle_against_real_diffusers_when_pinned():
    """tests/golden/diffusers_tiny.npz is written by scripts/gen_golden_diffusers.py where real diffusers is importable (it is not in
    this environment: the oracle's UNet / VAE / PNDM arithmetic is PARITY UNPINNED until that file exists).  When present, the
    oracle must reproduce real diffusers on the same weights and inputs to fp32 round-off."""
    path = os.path.join(GOLD, "diffusers_tiny.npz")
    if not os.path.exists(path):
        pytest.skip("parity unpinned: no diffusers_tiny.npz (run scripts/gen_golden_diffusers.py where diffusers==0.34.0 is importable)")
    from ldiffusion_amd import configs, weights
    from oracle import noise_post, schedule, unet as ounet, vae as ovae
    z = np.load(path)
    usd = weights.synthetic_state_dict(weights.unet_param_shapes(configs.TINY_UNET), 42)
    vsd = weights.synthetic_state_dict(weights.vae_param_shapes(configs.TINY_VAE), 43)
    close = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() <= 2e-5 * max(1.0, np.abs(np.asarray(b)).max())
    with torch.no_grad():
        for t in (1, 501, 751):
            assert close(ounet.unet_forward(usd, configs.TINY_UNET, torch.from_numpy(z["unet_x"]), t, torch.from_numpy(z["unet_ctx"])).sample, z[f"unet_t{t}"]), t
        mom = ovae.vae_encode_moments(vsd, configs.TINY_VAE, torch.from_numpy(z["vae_img"]))
        d = ovae.LatentDist(mom)
        assert close(d.mean, z["vae_mean"]) and close(d.logvar, z["vae_logvar"])
        assert close(ovae.vae_decode(vsd, configs.TINY_VAE, torch.from_numpy(z["vae_z"])), z["vae_dec"])
    assert np.array_equal(schedule.alphas_cumprod().numpy(), z["alphas_cumprod"])
    for n in (1, 4, 9, 19):
        sch = schedule.PNDMOracle()
        sch.set_timesteps(n)
        assert sch.timesteps.tolist() == z[f"timesteps_{n}"].tolist()
        x = torch.from_numpy(z[f"plms_{n}_x"][0])
        for i, t in enumerate(sch.timesteps):
            x = sch.step(torch.from_numpy(z[f"plms_{n}_eps"][i]), t, x).prev_sample
            assert close(x, z[f"plms_{n}_x"][i + 1]), (n, i)
    if "decode_latents" in z:
        img = noise_post.decode_post(ovae.vae_decode(vsd, configs.TINY_VAE, torch.from_numpy(z["vae_z"]) / 0.18215))
        assert close(img, z["decode_latents"]) and np.abs(noise_post.to_uint8(z["decode_latents"]).astype(int) - z["numpy_to_pil_u8"].astype(int)).max() == 0


def test_infonce_mirror_matches_reference_code():
    """ldiffusion_amd.loss.InfoNceLoss.compute_contrastive_loss against the REFERENCE's own function (model/loss.py:44-109, run in the build
    container by scripts/gen_golden_loss.py): with the same torch seed the mirror must draw the same (anchor, positive, negatives) triples
    -- same loss value, and the random stream left in the same state."""
    from ldiffusion_amd.loss import InfoNceLoss
    z = np.load(os.path.join(GOLD, "reference_infonce.npz"))
    for tag in "abc":
        torch.manual_seed(int(z[tag + "_seed"]))
        loss = InfoNceLoss().compute_contrastive_loss(torch.from_numpy(z[tag + "_features"]), torch.from_numpy(z[tag + "_labels"]))
        assert abs(float(loss) - float(z[tag + "_loss"])) <= 1e-6 * abs(float(z[tag + "_loss"])), tag
        assert torch.rand(1).item() == float(z[tag + "_next_rand"]), tag
    with pytest.raises(RuntimeError, match="VGG19"):
        InfoNceLoss().compute_loss(torch.zeros((1, 3, 8, 8)), torch.zeros((1, 3, 8, 8)), torch.zeros((1, 2, 8, 8)), torch.zeros((1, 1, 8, 8)))
    vgg = lambda x: x.mean((2, 3))                                      # an injected feature extractor enables the content term
    l2 = InfoNceLoss(vgg_features=vgg).compute_content_loss(torch.ones((1, 3, 8, 8)), torch.zeros((1, 3, 8, 8)))
    assert abs(float(l2) - 1.0) < 1e-6
