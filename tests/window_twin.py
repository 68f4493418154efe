"""Host twin of the batched sliding window (ldiff_op_window_gather / _accumulate_batch / _finish, include/ldiff.h) in plain torch on CPU tensors: the
arithmetic statement the kernels implement, pinned to the reference's recorded output by tests/test_cpu_window_plan.py and compared with the device by
tests/test_gpu_window_batched.py.  Not part of the package.

Per pixel the order is: the chunk's valid tiles in slicer order; per tile the mirror average in the PREDICTION's dtype (adds in variant order, then one
division by the variant count), the product with the importance map in the promoted type of (prediction, map), the sum rounded to the accumulators' dtype,
and, at the end, one correctly rounded division.  A tile's pixels are independent, so each step below is one tensor op over the tile: every element still
sees exactly that sequence of individually rounded operations (CPU torch rounds each half-precision op once, from an exact float32 result)."""
import torch

from ldiffusion_amd import tiling


def sw_network(W):
    """The stand-in head of the sliding-window fixture (tests/test_cpu_oracle.py `_sw_network`): integer weights + a column ramp, float32 out."""
    def network(x):
        ramp = torch.arange(x.shape[-1], dtype=torch.float32, device=x.device) * 0.125
        return torch.einsum("oc,bchw->bohw", W.to(x.device), x.float()) + ramp[None, None, None, :]
    return network


def flip_dims(mask, first_axis):
    return tuple(first_axis + a for a in range(2) if (mask >> a) & 1)


def gather(image, plan, origins):
    """[len(origins) * M, C, th, tw]: the padded image's tiles under every variant, tile-major then variant."""
    padded, _ = tiling.pad_to_tile(image, plan.tile_hw)
    th, tw = plan.tile_hw
    out = []
    for y, x in origins:
        tile = padded[:, y:y + th, x:x + tw]
        out += [torch.flip(tile, flip_dims(m, 1)) if m else tile for m in plan.variants]
    return torch.stack(out).contiguous()


def accumulate_chunk(acc, cnt, pred, g, origins, n_valid, variants):
    """The first n_valid tiles of one chunk, in order, into acc / cnt (in place)."""
    M = len(variants)
    th, tw = pred.shape[-2:]
    for k in range(n_valid):
        y, x = origins[k]
        p = pred[k * M].clone()
        for v in range(1, M):
            p = p + torch.flip(pred[k * M + v], flip_dims(variants[v], 1))      # rounded to the prediction's dtype
        if M > 1:
            p = p / M                                                           # likewise
        if acc.dtype == torch.float32:
            p = p.float()                                                       # a float16 prediction is widened AFTER its average
        prod = p * g if g is not None else p                                    # promoted type of (prediction, map)
        acc[:, y:y + th, x:x + tw] = (acc[:, y:y + th, x:x + tw] + prod).to(acc.dtype)
        cnt[y:y + th, x:x + tw] = (cnt[y:y + th, x:x + tw] + (g if g is not None else 1)).to(cnt.dtype)


def accumulate_image(image, network, num_heads, tile_hw, tile_step_size=0.5, use_gaussian=True, mirror_axes=None, acc_dtype=torch.float16, batch_tiles=1):
    """-> (acc, cnt, plan) over the padded extent, before the division; `network` sees the same batches as on the device (filler tiles included)."""
    plan = tiling.window_plan(tuple(image.shape[1:]), tile_hw, tile_step_size, mirror_axes, batch_tiles)
    acc = torch.zeros((num_heads,) + plan.padded_hw, dtype=acc_dtype)
    cnt = torch.zeros(plan.padded_hw, dtype=acc_dtype)
    g = tiling.compute_gaussian(plan.tile_hw, 1.0 / 8, 10, acc_dtype) if use_gaussian else None
    for origins, n_valid in plan.chunks:
        accumulate_chunk(acc, cnt, network(gather(image.float(), plan, origins)), g, origins, n_valid, plan.variants)
    return acc, cnt, plan


def finish(acc, cnt, plan):
    """logits [heads, H, W] = acc / cnt inside the revert slices, one correctly rounded division; RuntimeError on +-inf there."""
    logits = (acc / cnt)[(slice(None),) + plan.revert]
    if bool(torch.isinf(logits).any()):
        raise RuntimeError("Encountered inf in predicted array")
    return logits


def argmax_rule(logits):
    """uint8 [H, W]: the first maximal class; a pixel with any NaN or +inf logit is class 0 (argmax(softmax(.)), ldiff_argmax_u8's rule)."""
    l = logits.float()
    bad = (torch.isnan(l) | (l == float("inf"))).any(0)
    l = torch.where(torch.isnan(l), torch.full_like(l, float("-inf")), l)
    m = l.argmax(0)   # CPU torch.argmax returns the first maximal index
    m[bad] = 0
    return m.to(torch.uint8)
