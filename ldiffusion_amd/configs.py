"""Model configs in the diffusers `config.json` vocabulary.

SD15_UNET / SD15_VAE reproduce the public SD-v1.5 `unet/config.json` and
`vae/config.json` fields the sampling path depends on:
the reference loads exactly these through `from_pretrained`
(/root/reference/segmentor.py:77-80, ldiffusion.py:66-70).
TINY_* are reduced-width graphs with the same topology, used by the parity
tests so the CPU oracle finishes in seconds.
"""
from __future__ import annotations

import copy

SD15_UNET = {
    "_class_name": "UNet2DConditionModel",
    "sample_size": 64,
    "in_channels": 4,
    "out_channels": 4,
    "down_block_types": ["CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"],
    "up_block_types": ["UpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D"],
    "block_out_channels": [320, 640, 1280, 1280],
    "layers_per_block": 2,
    "attention_head_dim": 8,  # SD-v1.5 quirk: number of heads
    "cross_attention_dim": 768,
    "norm_num_groups": 32,
    "norm_eps": 1e-5,
    "act_fn": "silu",
    "flip_sin_to_cos": True,
    "freq_shift": 0,
    "downsample_padding": 1,
    "center_input_sample": False,
    "use_linear_projection": False,
}

SD15_VAE = {
    "_class_name": "AutoencoderKL",
    "in_channels": 3,
    "out_channels": 3,
    "latent_channels": 4,
    "block_out_channels": [128, 256, 512, 512],
    "down_block_types": ["DownEncoderBlock2D"] * 4,
    "up_block_types": ["UpDecoderBlock2D"] * 4,
    "layers_per_block": 2,
    "norm_num_groups": 32,
    "act_fn": "silu",
    "sample_size": 512,
    "scaling_factor": 0.18215,
}

# Same topology, 1/5 width (head dims 8/16/32/32), cross-attention dim 64.
TINY_UNET = dict(copy.deepcopy(SD15_UNET), block_out_channels=[64, 128, 256, 256], cross_attention_dim=64)
# Same topology, 1/4 width.
TINY_VAE = dict(copy.deepcopy(SD15_VAE), block_out_channels=[32, 64, 128, 128])

# ControlNetModel (the network `Segmentor.ldiffusion_augment_for_multimodal` takes its thirteen residual tensors from,
# /root/reference/segmentor.py:301-386): the UNet's conv_in, time embedding, down blocks and mid block, a conditioning embedding in
# front and one 1x1 "zero conv" behind every skip tensor.  The fields are those of the public SD-v1.5 ControlNet config.json files.
_CONTROLNET_FIELDS = {
    "_class_name": "ControlNetModel",
    "conditioning_channels": 3,
    "conditioning_embedding_out_channels": [16, 32, 96, 256],
    "controlnet_conditioning_channel_order": "rgb",
    "global_pool_conditions": False,
}
_UNET_ONLY_FIELDS = ("up_block_types", "out_channels", "sample_size", "center_input_sample")
SD15_CONTROLNET = dict({k: v for k, v in copy.deepcopy(SD15_UNET).items() if k not in _UNET_ONLY_FIELDS}, **copy.deepcopy(_CONTROLNET_FIELDS))
# TINY_UNET's widths behind the embedding's REAL channel list: the conditioning-embedding kernel is tested at the channel counts it will see
TINY_CONTROLNET = dict(copy.deepcopy(SD15_CONTROLNET), block_out_channels=[64, 128, 256, 256], cross_attention_dim=64)


# diffusers' constructor defaults for the fields the sampling path reads: a config.json written by an older diffusers (or a
# hand-trimmed one) may omit any of them, and `from_pretrained` then fills these in (UNet2DConditionModel.__init__ /
# AutoencoderKL.__init__ signatures of diffusers 0.34.0 [mem]).
UNET_DEFAULTS = {
    "sample_size": None, "in_channels": 4, "out_channels": 4, "center_input_sample": False, "flip_sin_to_cos": True, "freq_shift": 0,
    "down_block_types": ["CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"],
    "up_block_types": ["UpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D"],
    "block_out_channels": [320, 640, 1280, 1280], "layers_per_block": 2, "downsample_padding": 1, "act_fn": "silu",
    "norm_num_groups": 32, "norm_eps": 1e-5, "cross_attention_dim": 1280, "attention_head_dim": 8, "use_linear_projection": False,
}
CONTROLNET_DEFAULTS = {
    "in_channels": 4, "conditioning_channels": 3, "flip_sin_to_cos": True, "freq_shift": 0,
    "down_block_types": ["CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"],
    "block_out_channels": [320, 640, 1280, 1280], "layers_per_block": 2, "downsample_padding": 1, "act_fn": "silu",
    "norm_num_groups": 32, "norm_eps": 1e-5, "cross_attention_dim": 1280, "attention_head_dim": 8, "use_linear_projection": False,
    "conditioning_embedding_out_channels": [16, 32, 96, 256], "controlnet_conditioning_channel_order": "rgb",
    "global_pool_conditions": False, "class_embed_type": None, "addition_embed_type": None, "num_class_embeds": None,
    "mid_block_type": "UNetMidBlock2DCrossAttn",
}
VAE_DEFAULTS = {
    "in_channels": 3, "out_channels": 3, "down_block_types": ["DownEncoderBlock2D"], "up_block_types": ["UpDecoderBlock2D"],
    "block_out_channels": [64], "layers_per_block": 1, "act_fn": "silu", "latent_channels": 4, "norm_num_groups": 32, "sample_size": 32,
    "scaling_factor": 0.18215,
}


def with_defaults(cfg: dict, defaults: dict) -> dict:
    out = dict(defaults)
    out.update(cfg)
    return out


def validate_unet_config(cfg: dict) -> None:
    """Reject configs outside what the HIP executor implements (fail loudly, no fallback)."""
    boc = cfg["block_out_channels"]
    n = len(boc)
    if len(cfg["down_block_types"]) != n or len(cfg["up_block_types"]) != n:
        raise ValueError("down/up block lists must match block_out_channels")
    for t in cfg["down_block_types"]:
        if t not in ("CrossAttnDownBlock2D", "DownBlock2D"):
            raise ValueError(f"unsupported down block type {t}")
    for t in cfg["up_block_types"]:
        if t not in ("CrossAttnUpBlock2D", "UpBlock2D"):
            raise ValueError(f"unsupported up block type {t}")
    heads = cfg["attention_head_dim"]
    if not isinstance(heads, int):
        raise ValueError("per-block attention_head_dim lists are not supported")
    for c in boc:
        if c % cfg["norm_num_groups"] or c % 8:
            raise ValueError(f"channel count {c} must be divisible by norm_num_groups and by 8")
        if (c // heads) % 8 or c % heads:
            raise ValueError(f"head dim {c}/{heads} must be a multiple of 8")
    if cfg["cross_attention_dim"] % 8:
        raise ValueError("cross_attention_dim must be a multiple of 8")
    if cfg.get("use_linear_projection", False):
        raise ValueError("use_linear_projection=True is not supported")
    if cfg.get("act_fn", "silu") != "silu":
        raise ValueError("only SiLU is supported")


def controlnet_trunk_config(cfg: dict) -> dict:
    """The UNet-shaped view of a ControlNet config: what `validate_unet_config` and the UNet-side helpers read.  The up path does not
    exist in a ControlNet; the mirrored block list stands in so that the shared code sees a well-formed UNet config."""
    up = ["CrossAttnUpBlock2D" if t == "CrossAttnDownBlock2D" else "UpBlock2D" for t in reversed(cfg["down_block_types"])]
    return dict(cfg, up_block_types=up, out_channels=cfg["in_channels"])


def validate_controlnet_config(cfg: dict) -> None:
    """Reject ControlNet configs outside what the HIP executor implements (fail loudly, no fallback): everything
    `validate_unet_config` refuses, plus the ControlNet-only switches."""
    if cfg.get("global_pool_conditions", False):
        raise ValueError("global_pool_conditions=True is not supported")
    for k in ("class_embed_type", "addition_embed_type", "num_class_embeds"):
        if cfg.get(k) is not None:
            raise ValueError(f"{k}={cfg[k]!r} is not supported (class / addition embeddings are not built)")
    if cfg.get("controlnet_conditioning_channel_order", "rgb") != "rgb":
        raise ValueError(f"controlnet_conditioning_channel_order={cfg['controlnet_conditioning_channel_order']!r} is not supported (only 'rgb')")
    if cfg.get("mid_block_type", "UNetMidBlock2DCrossAttn") != "UNetMidBlock2DCrossAttn":
        raise ValueError(f"mid_block_type={cfg['mid_block_type']!r} is not supported")
    if cfg.get("conditioning_channels", 3) > 8 or cfg.get("conditioning_channels", 3) < 1:
        raise ValueError("conditioning_channels must be between 1 and 8")
    emb = list(cfg.get("conditioning_embedding_out_channels", ()))
    if not 1 <= len(emb) <= 8 or any(c % 8 for c in emb):
        raise ValueError("conditioning_embedding_out_channels must hold 1..8 channel counts, each a multiple of 8")
    if len(cfg["down_block_types"]) != len(cfg["block_out_channels"]):
        raise ValueError("down block list must match block_out_channels")
    validate_unet_config(controlnet_trunk_config(cfg))


def validate_vae_config(cfg: dict) -> None:
    for c in cfg["block_out_channels"]:
        if c % cfg["norm_num_groups"] or c % 8:
            raise ValueError(f"channel count {c} must be divisible by norm_num_groups and by 8")
    if cfg["latent_channels"] > 8 or cfg["in_channels"] > 8 or cfg["out_channels"] > 8:
        raise ValueError("in/out/latent channels above 8 are not supported")
