"""CPU (-m "not gpu"): the ControlNet's configuration, checkpoint layout and the plain-torch restatement the GPU tests compare against."""
import copy

import pytest
import torch

from controlnet_ref import cond_embedding, controlnet_forward, skip_shapes
from ldiffusion_amd import configs, weights
from oracle.unet import _conv, unet_forward


def _tiny(seed=7):
    cfg = configs.TINY_CONTROLNET
    return cfg, weights.synthetic_state_dict(weights.controlnet_param_shapes(cfg), seed, fp16_values=True)


def _inputs(B=2, h=8, w=8, L=5, seed=3):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((B, 4, h, w), generator=g), torch.randn((1, L, configs.TINY_CONTROLNET["cross_attention_dim"]), generator=g) * 0.5,
            torch.rand((B, 3, 8 * h, 8 * w), generator=g))


def test_sd15_controlnet_parameter_layout():
    cfg, ucfg = configs.SD15_CONTROLNET, configs.SD15_UNET
    shapes, ushapes = weights.controlnet_param_shapes(cfg), weights.unet_param_shapes(ucfg)
    shared = {k: v for k, v in ushapes.items() if k.split(".")[0] in ("conv_in", "time_embedding", "down_blocks", "mid_block")}
    assert weights.param_count(shared) == 348_712_960
    for k, v in shared.items():
        assert shapes[k] == v, k
    emb = {k: v for k, v in shapes.items() if k.startswith("controlnet_cond_embedding.")}
    zero = {k: v for k, v in shapes.items() if k.startswith(("controlnet_down_blocks.", "controlnet_mid_block."))}
    assert weights.param_count(emb) == 1_086_480 and weights.param_count(zero) == 11_479_680
    assert weights.param_count(shapes) == 361_279_120 == weights.param_count(shared) + weights.param_count(emb) + weights.param_count(zero)
    assert set(shapes) == set(shared) | set(emb) | set(zero)
    sk = skip_shapes(ucfg, 1, 64, 64)
    assert len(sk) == 12
    for i, s in enumerate(sk):
        assert shapes[f"controlnet_down_blocks.{i}.weight"] == (s[1], s[1], 1, 1) and shapes[f"controlnet_down_blocks.{i}.bias"] == (s[1],)
    assert f"controlnet_down_blocks.{len(sk)}.weight" not in shapes
    assert shapes["controlnet_mid_block.weight"] == (sk[-1][1], sk[-1][1], 1, 1)
    assert [shapes[f"controlnet_cond_embedding.{n}.weight"][:2] for n in ("conv_in", "blocks.0", "blocks.1", "blocks.2", "blocks.3", "blocks.4", "blocks.5", "conv_out")] == \
        [(16, 3), (16, 16), (32, 16), (32, 32), (96, 32), (96, 96), (256, 96), (320, 256)]
    assert configs.TINY_CONTROLNET["conditioning_embedding_out_channels"] == [16, 32, 96, 256]
    assert configs.TINY_CONTROLNET["block_out_channels"] == configs.TINY_UNET["block_out_channels"]
    assert cfg["_class_name"] == "ControlNetModel" and cfg["conditioning_channels"] == 3


def test_restatement_wiring():
    cfg, sd = _tiny()
    ucfg = configs.TINY_UNET
    usd = weights.synthetic_state_dict(weights.unet_param_shapes(ucfg), 42, fp16_values=True)
    x, ctx, cond = _inputs()
    B, h, w = x.shape[0], x.shape[2], x.shape[3]
    with torch.no_grad():
        assert tuple(cond_embedding(sd, cfg, cond).shape) == (B, cfg["block_out_channels"][0], h, w)
        down, mid = controlnet_forward(sd, cfg, x, 501, ctx, cond)
        shapes = skip_shapes(cfg, B, h, w)
        assert len(down) == 12 and [tuple(t.shape) for t in down] == shapes and tuple(mid.shape) == shapes[-1]
        assert all(t.abs().max() > 1e-3 for t in down + [mid]), "synthetic zero convs must not be zero: a dead trunk would pass every parity test"
        # linear in conditioning_scale
        d2, m2 = controlnet_forward(sd, cfg, x, 501, ctx, cond, conditioning_scale=0.5)
        for a, b in zip(down + [mid], d2 + [m2]):
            assert torch.allclose(b, 0.5 * a, rtol=0, atol=1e-6 * a.abs().max().item())
        # zeroed zero convs: exact zeros, and the UNet fed with them is the plain UNet
        z = {k: (torch.zeros_like(v) if k.startswith(("controlnet_down_blocks.", "controlnet_mid_block.")) else v) for k, v in sd.items()}
        d0, m0 = controlnet_forward(z, cfg, x, 501, ctx, cond)
        assert all(not t.any() for t in d0 + [m0])
        assert torch.equal(unet_forward(usd, ucfg, x, 501, ctx, down_block_additional_residuals=d0, mid_block_additional_residual=m0).sample,
                           unet_forward(usd, ucfg, x, 501, ctx).sample)
        # conv_out of the embedding zeroed + identity zero convs: residual 0 is conv_in(sample)
        e = dict(sd)
        e["controlnet_cond_embedding.conv_out.weight"] = torch.zeros_like(sd["controlnet_cond_embedding.conv_out.weight"])
        e["controlnet_cond_embedding.conv_out.bias"] = torch.zeros_like(sd["controlnet_cond_embedding.conv_out.bias"])
        c0 = cfg["block_out_channels"][0]
        e["controlnet_down_blocks.0.weight"] = torch.eye(c0).reshape(c0, c0, 1, 1)
        e["controlnet_down_blocks.0.bias"] = torch.zeros(c0)
        di, _ = controlnet_forward(e, cfg, x, 501, ctx, cond)
        assert torch.equal(di[0], _conv(sd, "conv_in", x))
        # the float64 form agrees with the float32 one to float32 round-off
        d64, m64 = controlnet_forward(sd, cfg, x, 501, ctx, cond, dtype=torch.float64)
        assert d64[0].dtype == torch.float64
        for a, b in zip(down + [mid], d64 + [m64]):
            assert (a.double() - b).abs().max() <= 1e-4 * b.abs().max()


def test_validate_controlnet_config_refuses_by_name_and_directory_round_trip(tmp_path):
    cfg, sd = _tiny()
    configs.validate_controlnet_config(configs.with_defaults(cfg, configs.CONTROLNET_DEFAULTS))
    configs.validate_controlnet_config(configs.with_defaults(configs.SD15_CONTROLNET, configs.CONTROLNET_DEFAULTS))
    for field, value in (("global_pool_conditions", True), ("class_embed_type", "timestep"), ("addition_embed_type", "text"), ("num_class_embeds", 10),
                         ("controlnet_conditioning_channel_order", "bgr"), ("use_linear_projection", True), ("act_fn", "gelu")):
        bad = dict(copy.deepcopy(cfg), **{field: value})
        with pytest.raises(ValueError, match=field.replace("act_fn", "SiLU")):
            configs.validate_controlnet_config(configs.with_defaults(bad, configs.CONTROLNET_DEFAULTS))
    bad = dict(copy.deepcopy(cfg), down_block_types=["AttnDownBlock2D"] + cfg["down_block_types"][1:])
    with pytest.raises(ValueError, match="AttnDownBlock2D"):
        configs.validate_controlnet_config(configs.with_defaults(bad, configs.CONTROLNET_DEFAULTS))
    weights.save_model_dir(str(tmp_path / "cn"), cfg, sd)
    cfg2, sd2 = weights.load_model_dir(str(tmp_path / "cn"))
    assert cfg2 == cfg and list(sd2) and set(sd2) == set(sd)
    for k in sd:
        assert torch.equal(sd2[k], sd[k]), k
