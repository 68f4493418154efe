"""ControlNetModel forward restated in plain torch (helper of the ControlNet tests; TEST INFRASTRUCTURE ONLY).

Follows the public algorithm of diffusers 0.34 `ControlNetModel` for SD-v1.5-style configs.  Like the rest of the oracle it CANNOT be pinned
against diffusers here (the package is absent: see oracle/__init__), so it is an independent restatement, not a recording.  The blocks are
`oracle.unet`'s own (`timestep_embedding`, `resnet_block`, `transformer2d`, `_conv`): the ones the UNet parity already rests on.  Only the
conditioning embedding, the zero convs and the wiring are new text:

    emb  = conv_out(SiLU(... SiLU(conv_in(cond)) ...))      per channel pair (c_i, c_i+1): conv3x3 c_i -> c_i, SiLU, conv3x3 c_i -> c_i+1 stride 2, SiLU
    h    = conv_in(sample) + emb
    skips, mid = the UNet's down path and mid block on h (same time embedding, same context)
    residual_i = conditioning_scale * controlnet_down_blocks[i](skip_i);   mid residual = conditioning_scale * controlnet_mid_block(mid)

`dtype` is the arithmetic of the whole forward: float32 for parity with the library, float64 for references of single kernels and for
judging the float32 form's own round-off."""
import torch
import torch.nn.functional as F

from oracle.unet import _conv, _lin, resnet_block, timestep_embedding, transformer2d

EMB = "controlnet_cond_embedding"


def cond_embedding(sd, cfg, cond):
    """[B, conditioning_channels, 8h, 8w] -> [B, block_out_channels[0], h, w] (for the four-entry channel list)."""
    h = F.silu(_conv(sd, EMB + ".conv_in", cond))
    for i in range(len(cfg["conditioning_embedding_out_channels"]) - 1):
        h = F.silu(_conv(sd, f"{EMB}.blocks.{2 * i}", h))
        h = F.silu(_conv(sd, f"{EMB}.blocks.{2 * i + 1}", h, stride=2, padding=1))
    return _conv(sd, EMB + ".conv_out", h)


def controlnet_forward(sd, cfg, sample, timestep, ctx, cond, conditioning_scale=1.0, dtype=torch.float32):
    """Returns (list of the skip-stack residuals, mid residual), each `dtype`."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    sample, ctx, cond = sample.to(dtype), ctx.to(dtype), cond.to(dtype)
    B = sample.shape[0]
    if ctx.shape[0] != B:
        ctx = ctx.expand(B, -1, -1)
    if cond.shape[0] != B:
        cond = cond.expand(B, -1, -1, -1)
    boc = cfg["block_out_channels"]
    groups, eps, heads, lpb = cfg["norm_num_groups"], cfg["norm_eps"], cfg["attention_head_dim"], cfg["layers_per_block"]
    t = torch.as_tensor(timestep)
    if t.dim() == 0:
        t = t[None]
    temb = timestep_embedding(t.expand(B), boc[0], cfg["flip_sin_to_cos"], cfg["freq_shift"]).to(dtype)
    temb = _lin(sd, "time_embedding.linear_2", F.silu(_lin(sd, "time_embedding.linear_1", temb)))

    h = _conv(sd, "conv_in", sample) + cond_embedding(sd, cfg, cond)
    skips = [h]
    for i, btype in enumerate(cfg["down_block_types"]):
        for j in range(lpb):
            h = resnet_block(sd, f"down_blocks.{i}.resnets.{j}", h, temb, groups, eps)
            if btype == "CrossAttnDownBlock2D":
                h = transformer2d(sd, f"down_blocks.{i}.attentions.{j}", h, ctx, heads, groups)
            skips.append(h)
        if i != len(boc) - 1:
            h = _conv(sd, f"down_blocks.{i}.downsamplers.0.conv", h, stride=2, padding=1)
            skips.append(h)
    h = resnet_block(sd, "mid_block.resnets.0", h, temb, groups, eps)
    h = transformer2d(sd, "mid_block.attentions.0", h, ctx, heads, groups)
    h = resnet_block(sd, "mid_block.resnets.1", h, temb, groups, eps)
    down = [_conv(sd, f"controlnet_down_blocks.{i}", s, padding=0) * conditioning_scale for i, s in enumerate(skips)]
    mid = _conv(sd, "controlnet_mid_block", h, padding=0) * conditioning_scale
    return down, mid


def skip_shapes(cfg, B, h, w):
    """Shapes of the UNet's skip tensors in stack order (what `UNet2DConditionModel._skip_shapes` describes), from the config alone."""
    boc, lpb = cfg["block_out_channels"], cfg["layers_per_block"]
    shapes = [(B, boc[0], h, w)]
    for i, c in enumerate(boc):
        shapes += [(B, c, h, w)] * lpb
        if i != len(boc) - 1:
            h, w = h // 2, w // 2
            shapes.append((B, c, h, w))
    return shapes
