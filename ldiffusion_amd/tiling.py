"""ROI tiling for BASELINE.json configs[3]: a 1024x1024 ROI is cut into 512x512 patches, every patch goes through the
sampler (independent units: they shard over batch entries and over ranks exactly like whole patches), and the per-patch
class logits are merged back into the ROI before the arg-max.

Mirrors the vendored nnU-Net helpers the reference's tissue path runs
(/root/reference/model/nnunetv2/inference/sliding_window_prediction.py:32-56 `compute_steps_for_sliding_window`,
:10-29 `compute_gaussian`; /root/reference/model/nnunetv2/inference/predict_from_raw_data.py:505-524 slicer order,
:530-545 mirroring test-time augmentation, :547-589 Gaussian-weighted accumulation in float16, :591-635 padding of images smaller
than a tile) with the same names and argument meaning; tensors stay on the device.  `predict_sliding_window_return_logits` is
pinned bit for bit to the reference's own code (tests/golden/reference_sliding_window.npz, scripts/gen_golden_sliding_window.py).
"""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import numpy as np
import torch


def compute_steps_for_sliding_window(image_size: Sequence[int], tile_size: Sequence[int], tile_step_size: float) -> List[List[int]]:
    if any(i < t for i, t in zip(image_size, tile_size)):
        raise ValueError("image size must be as large or larger than patch_size")
    if not 0 < tile_step_size <= 1:
        raise ValueError("step_size must be larger than 0 and smaller or equal to 1")
    steps = []
    for I, T in zip(image_size, tile_size):
        n = int(math.ceil((I - T) / (T * tile_step_size))) + 1
        actual = (I - T) / (n - 1) if n > 1 else 0.0
        steps.append([int(np.round(actual * k)) for k in range(n)])
    return steps


def tile_origins(image_hw: Tuple[int, int], tile_hw: Tuple[int, int], tile_step_size: float = 1.0) -> List[Tuple[int, int]]:
    sy, sx = compute_steps_for_sliding_window(image_hw, tile_hw, tile_step_size)
    return [(y, x) for y in sy for x in sx]


def split_tiles(image: torch.Tensor, tile_hw: Tuple[int, int], tile_step_size: float = 1.0):
    """[C, H, W] or [1, C, H, W] -> ([n, C, th, tw] contiguous on the same device, origins)."""
    if image.dim() == 4:
        if image.shape[0] != 1:
            raise ValueError("split_tiles takes one ROI")
        image = image[0]
    if image.dim() != 3:
        raise ValueError("ROI must be [C, H, W]")
    th, tw = tile_hw
    origins = tile_origins(tuple(image.shape[1:]), tile_hw, tile_step_size)
    return torch.stack([image[:, y:y + th, x:x + tw] for y, x in origins], 0).contiguous(), origins


def compute_gaussian(tile_size: Sequence[int], sigma_scale: float = 1.0 / 8, value_scaling_factor: float = 1.0,
                     dtype=torch.float16, device="cpu") -> torch.Tensor:
    """Separable Gaussian of an impulse at the tile centre (truncated at 4 sigma, zero padded), peak = value_scaling_factor, cast
    to `dtype` (the reference's default is float16) and THEN zeros lifted to the smallest non-zero value, in that order
    (sliding_window_prediction.py:22-27: the float16 tail underflows to zero before the lift).  Built from the 1-D kernels
    directly (no scipy at run time)."""
    axes = []
    for n in tile_size:
        sigma = n * sigma_scale
        radius = int(4.0 * sigma + 0.5)
        k = np.exp(-0.5 * (np.arange(-radius, radius + 1) / sigma) ** 2)
        k /= k.sum()
        line = np.zeros(n)
        c = n // 2
        for d in range(-radius, radius + 1):   # correlate the impulse with the (symmetric) kernel
            if 0 <= c + d < n:
                line[c + d] = k[d + radius]
        axes.append(line)
    g = axes[0]
    for a in axes[1:]:
        g = np.multiply.outer(g, a)
    g = torch.from_numpy(g / g.max() * value_scaling_factor).to(dtype).to(device)
    g[g == 0] = g[g != 0].min()
    return g


def _window_accumulate(acc: torch.Tensor, cnt: torch.Tensor, pred: torch.Tensor, g, y: int, x: int) -> None:
    """acc[:, y:y+th, x:x+tw] += pred * g;  cnt[y:y+th, x:x+tw] += g  (g None: weight 1).  Device tensors: ONE launch of
    ldiff_window_accumulate (the same two roundings per element as the tensor formulation below, which serves host tensors: the CPU tests
    pin it to the reference's predictor)."""
    th, tw = pred.shape[-2:]
    if tuple(pred.shape) != (acc.shape[0], th, tw):   # the kernel indexes pred with acc's class count: a head with fewer channels would be read out of bounds
        raise ValueError(f"window accumulate: prediction {tuple(pred.shape)} does not match the accumulator's {acc.shape[0]} classes")
    if g is not None and tuple(g.shape) != (th, tw):
        raise ValueError(f"window accumulate: importance map {tuple(g.shape)} does not match the tile {(th, tw)}")
    if y < 0 or x < 0 or y + th > acc.shape[1] or x + tw > acc.shape[2]:
        raise ValueError(f"window accumulate: tile {(th, tw)} at {(y, x)} leaves the {tuple(acc.shape[1:])} accumulator")
    if acc.is_cuda:
        from . import _lib
        if acc.dtype == torch.float32 and pred.dtype in (torch.float16, torch.bfloat16):
            pred = pred.float()   # a half-precision head (autocast) into float32 accumulators: identical to the tensor formulation's type promotion
        kinds = {(torch.float32, torch.float32): 0, (torch.float16, torch.float16): 1, (torch.float16, torch.float32): 3}
        if acc.dtype != cnt.dtype or (acc.dtype, pred.dtype) not in kinds or not (acc.is_contiguous() and cnt.is_contiguous()):
            raise ValueError("window accumulate: contiguous float32 accumulators with a float32 prediction, or float16 ones with a float16 / float32 prediction")
        pred = pred.contiguous()
        gg = None if g is None else g.to(acc.dtype).contiguous()
        _lib.check(_lib.load().ldiff_window_accumulate(_lib.ptr(acc), _lib.ptr(cnt), _lib.ptr(pred), _lib.ptr(gg), acc.shape[0], acc.shape[1], acc.shape[2],
                                                       th, tw, int(y), int(x), kinds[(acc.dtype, pred.dtype)], _lib.stream_ptr()))
        return
    acc[:, y:y + th, x:x + tw] += pred * g if g is not None else pred
    cnt[y:y + th, x:x + tw] += g if g is not None else 1


def merge_tile_logits(tiles: torch.Tensor, origins: Sequence[Tuple[int, int]], image_hw: Tuple[int, int], use_gaussian: bool = True,
                      dtype=torch.float32) -> torch.Tensor:
    """[n, C, th, tw] logits -> [C, H, W]: `logits[sl] += pred * g; n[sl] += g; logits /= n` on the tiles' device.
    dtype=torch.float16 reproduces the reference's accumulators and importance map (predict_from_raw_data.py:563-570); the default
    float32 is a deliberate deviation for the sampler's own tile merge (BASELINE configs[3]): it avoids the fp16 underflow of the
    map's tail and the 11-bit accumulation, and is what the oracle's float64 merge is compared with."""
    if tiles.dim() != 4 or len(origins) != tiles.shape[0]:
        raise ValueError("tiles must be [n, C, th, tw] with one origin per tile")
    n, C, th, tw = tiles.shape
    g = compute_gaussian((th, tw), 1.0 / 8, 10.0, dtype, tiles.device) if use_gaussian else torch.ones((th, tw), dtype=dtype, device=tiles.device)
    acc = torch.zeros((C,) + tuple(image_hw), dtype=dtype, device=tiles.device)
    cnt = torch.zeros(tuple(image_hw), dtype=dtype, device=tiles.device)
    for t, (y, x) in zip(tiles, origins):
        _window_accumulate(acc, cnt, t if (dtype == torch.float16 and t.dtype == torch.float32) else t.to(dtype), g, y, x)
    if not bool((cnt > 0).all()):
        raise RuntimeError("tiles do not cover the ROI")
    return acc / cnt


def maybe_mirror_and_predict(network, x: torch.Tensor, mirror_axes=None) -> torch.Tensor:
    """predict_from_raw_data.py:530-545: the network on x and on every non-empty combination of flips over `mirror_axes`
    (0 = rows, 1 = columns of a [1, C, h, w] tile), each prediction flipped back, averaged."""
    import itertools
    prediction = network(x)
    if mirror_axes is not None:
        if max(mirror_axes) > x.dim() - 3:
            raise ValueError("mirror_axes does not match the dimension of the input!")
        combos = [c for i in range(len(mirror_axes)) for c in itertools.combinations([m + 2 for m in mirror_axes], i + 1)]
        for axes in combos:
            prediction += torch.flip(network(torch.flip(x, (*axes,))), (*axes,))
        prediction /= (len(combos) + 1)
    return prediction


def pad_to_tile(image: torch.Tensor, tile_hw: Tuple[int, int]):
    """acvl_utils `pad_nd_image(image, new_shape=tile, 'constant', value 0, return_slicer=True)` for [C, H, W]: images smaller than
    the tile are zero padded, the excess split evenly (the odd element goes to the far side).  Returns (padded, (sy, sx))."""
    C, H, W = image.shape
    ph, pw = max(tile_hw[0] - H, 0), max(tile_hw[1] - W, 0)
    t, l = ph // 2, pw // 2
    if ph or pw:
        image = torch.nn.functional.pad(image, (l, pw - l, t, ph - t), mode="constant", value=0)
    return image, (slice(t, t + H), slice(l, l + W))


@torch.no_grad()
def predict_sliding_window_return_logits(image: torch.Tensor, network, num_heads: int, tile_hw: Tuple[int, int], tile_step_size: float = 0.5,
                                         use_gaussian: bool = True, mirror_axes=None, acc_dtype=torch.float16) -> torch.Tensor:
    """nnUNetPredictor.predict_sliding_window_return_logits (predict_from_raw_data.py:547-635) for one 2-D image [C, H, W] that
    is already on the device: tiles in the reference's slicer order (rows outer), mirroring TTA per tile, Gaussian-weighted
    accumulation `logits[sl] += pred * g; n[sl] += g` in `acc_dtype` (float16 in the reference), `logits /= n`, the inf check,
    padding reverted.  `network([1, C, th, tw]) -> [1, num_heads, th, tw]` is the injected tissue head.  Returns
    [num_heads, H, W] in `acc_dtype` on the image's device."""
    if image.dim() != 3:
        raise ValueError("input_image must be [C, H, W]")
    data, revert = pad_to_tile(image, tile_hw)
    th, tw = tile_hw
    logits = torch.zeros((num_heads,) + tuple(data.shape[1:]), dtype=acc_dtype, device=data.device)
    n_pred = torch.zeros(tuple(data.shape[1:]), dtype=acc_dtype, device=data.device)
    g = compute_gaussian((th, tw), sigma_scale=1.0 / 8, value_scaling_factor=10, dtype=acc_dtype, device=data.device) if use_gaussian else None
    for y, x in tile_origins(tuple(data.shape[1:]), tile_hw, tile_step_size):
        pred = maybe_mirror_and_predict(network, data[None, :, y:y + th, x:x + tw], mirror_axes)[0]
        _window_accumulate(logits, n_pred, pred, g if use_gaussian else None, y, x)
    logits /= n_pred
    if bool(torch.isinf(logits).any()):
        raise RuntimeError("Encountered inf in predicted array. Aborting... If this problem persists, reduce value_scaling_factor in "
                           "compute_gaussian or increase the dtype of predicted_logits to fp32")
    return logits[(slice(None),) + revert]


def merge_tile_masks(masks: torch.Tensor, origins: Sequence[Tuple[int, int]], image_hw: Tuple[int, int]) -> torch.Tensor:
    """Non-overlapping tiles (tile_step_size 1.0 on a multiple of the tile): [n, th, tw] uint8 -> [H, W] by plain copies."""
    n, th, tw = masks.shape
    out = torch.zeros(tuple(image_hw), dtype=masks.dtype, device=masks.device)
    seen = torch.zeros(tuple(image_hw), dtype=torch.bool, device=masks.device)
    for m, (y, x) in zip(masks, origins):
        if bool(seen[y:y + th, x:x + tw].any()):
            raise ValueError("merge_tile_masks needs non-overlapping tiles; merge logits instead")
        out[y:y + th, x:x + tw] = m
        seen[y:y + th, x:x + tw] = True
    if not bool(seen.all()):
        raise RuntimeError("tiles do not cover the ROI")
    return out


# ---- the sliding window in batches: a few launches per image instead of one network call per tile and mirror variant ---------------------
WINDOW_MAX_TILES = 64   # LDIFF_WINDOW_MAX_TILES: tiles of one launch (they travel by value in the kernels' arguments)


def mirror_variants(mirror_axes) -> List[int]:
    """The evaluations of `maybe_mirror_and_predict`, in its order, as 2-bit flip masks (bit 0: axis 0 = rows, bit 1: axis 1 = columns): the
    identity, then every non-empty combination of `mirror_axes` as itertools.combinations yields them.  1, 2 or 4 variants in 2-D."""
    import itertools
    masks = [0]
    if mirror_axes is not None:
        axes = [int(a) for a in mirror_axes]
        if not axes or min(axes) < 0 or max(axes) > 1:
            raise ValueError("mirror_axes does not match the dimension of the input!")
        if len(set(axes)) != len(axes):
            raise ValueError(f"mirror_axes {tuple(axes)} names an axis twice")
        for i in range(len(axes)):
            for combo in itertools.combinations(axes, i + 1):
                masks.append(sum(1 << a for a in combo))
    return masks


class WindowPlan:
    """Host plan of one image's batched sliding window (`window_plan`):
    image_hw, tile_hw; padded_hw, pad = (top, left) and revert = (slice, slice) by `pad_to_tile`'s rule; origins in the reference's slicer order;
    variants (flip masks, `mirror_variants`); batch_tiles; chunks = [(origins of exactly batch_tiles tiles, n_valid)]: consecutive runs of the
    origins, a short last run filled by repeating its last tile so that every network call of the image has the batch batch_tiles * len(variants)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def batch(self) -> int:
        return self.batch_tiles * len(self.variants)


def window_plan(image_hw, tile_hw, tile_step_size: float = 0.5, mirror_axes=None, batch_tiles: int = 1) -> WindowPlan:
    H, W = (int(v) for v in image_hw)
    th, tw = (int(v) for v in tile_hw)
    batch_tiles = int(batch_tiles)
    if H < 1 or W < 1 or th < 1 or tw < 1:
        raise ValueError(f"window_plan: image_hw {(H, W)} and tile_hw {(th, tw)} must be positive")
    if not 1 <= batch_tiles <= WINDOW_MAX_TILES:
        raise ValueError(f"window_plan: batch_tiles {batch_tiles} out of range [1, {WINDOW_MAX_TILES}] (tiles of one launch)")
    ph, pw = max(th - H, 0), max(tw - W, 0)
    top, left = ph // 2, pw // 2
    padded = (H + ph, W + pw)
    origins = tile_origins(padded, (th, tw), tile_step_size)
    chunks = []
    for i in range(0, len(origins), batch_tiles):
        run = origins[i:i + batch_tiles]
        chunks.append((run + [run[-1]] * (batch_tiles - len(run)), len(run)))
    return WindowPlan(image_hw=(H, W), tile_hw=(th, tw), padded_hw=padded, pad=(top, left), revert=(slice(top, top + H), slice(left, left + W)),
                      origins=origins, variants=mirror_variants(mirror_axes), batch_tiles=batch_tiles, chunks=chunks)


def _window_tiles(origins, n_valid: int, variants):
    """ldiff_window_tiles of one chunk (a host struct: the launchers copy it into the kernels' arguments)."""
    from . import _lib
    if len(origins) > WINDOW_MAX_TILES:
        raise ValueError(f"window tiles: n_tiles {len(origins)} exceeds the {WINDOW_MAX_TILES} tiles of one launch")
    t = _lib.WindowTiles()
    t.n_tiles, t.n_valid, t.n_variants = len(origins), int(n_valid), len(variants)
    for i, v in enumerate(variants):
        t.variants[i] = int(v)
    for k, (y, x) in enumerate(origins):
        t.y0[k], t.x0[k] = int(y), int(x)
    return t


_WINDOW_KINDS = {(torch.float32, torch.float32): 0, (torch.float16, torch.float16): 1, (torch.float32, torch.float16): 2, (torch.float16, torch.float32): 3}
_INF_MESSAGE = ("Encountered inf in predicted array. Aborting... If this problem persists, reduce value_scaling_factor in "
                "compute_gaussian or increase the dtype of predicted_logits to fp32")


def window_gather(image: torch.Tensor, plan: WindowPlan, origins, out: torch.Tensor = None) -> torch.Tensor:
    """One launch of ldiff_op_window_gather: `origins` (at most WINDOW_MAX_TILES tiles of the padded extent) x plan.variants out of the float32 device image
    [C, h, w] (unit stride along x; any row and plane stride) -> [len(origins) * M, C, th, tw] float32, tile-major then variant; exactly 0 in the pad."""
    from . import _lib
    if not (isinstance(image, torch.Tensor) and image.is_cuda and image.dim() == 3 and image.dtype == torch.float32 and image.stride(2) == 1):
        raise ValueError("window gather: `image` must be a float32 device tensor [C, h, w] with unit stride along x")
    if tuple(image.shape[1:]) != tuple(plan.image_hw):
        raise ValueError(f"window gather: image {tuple(image.shape[1:])} does not match the plan's {tuple(plan.image_hw)}")
    (th, tw), C = plan.tile_hw, image.shape[0]
    t = _window_tiles(origins, len(origins), plan.variants)
    shape = (len(origins) * len(plan.variants), C, th, tw)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=image.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != image.device:
        raise ValueError(f"window gather: `out` must be a contiguous float32 {shape} on the image's device")
    _lib.check(_lib.load().ldiff_op_window_gather(_lib.ptr(image), C, image.shape[1], image.shape[2], image.stride(1), image.stride(0), plan.pad[0], plan.pad[1],
                                                  plan.padded_hw[0], plan.padded_hw[1], t, th, tw, _lib.ptr(out), _lib.stream_ptr()))
    return out


def window_accumulate_batch(acc: torch.Tensor, cnt: torch.Tensor, pred: torch.Tensor, g, origins, n_valid: int, variants) -> None:
    """One launch of ldiff_op_window_accumulate_batch: pred [len(origins) * M, heads, th, tw] (float32 or float16, tile-major then variant) un-flipped,
    averaged over the variants in the prediction's dtype, weighted by g [th, tw] (None: 1) and added into acc [heads, Hp, Wp] / cnt [Hp, Wp] for the first
    `n_valid` tiles in order -- bit for bit what `maybe_mirror_and_predict` + `_window_accumulate` leave per tile."""
    from . import _lib
    if not (acc.is_cuda and cnt.is_cuda and pred.is_cuda):
        raise ValueError("window accumulate batch: device tensors only")
    if acc.dim() != 3 or acc.dtype != cnt.dtype or tuple(cnt.shape) != tuple(acc.shape[1:]) or not (acc.is_contiguous() and cnt.is_contiguous()):
        raise ValueError("window accumulate batch: contiguous accumulators acc [heads, Hp, Wp] and cnt [Hp, Wp] of one dtype")
    if (acc.dtype, pred.dtype) not in _WINDOW_KINDS:
        raise ValueError(f"window accumulate batch: float32 / float16 accumulators with a float32 / float16 prediction, not {acc.dtype} with {pred.dtype}")
    heads = acc.shape[0]
    if pred.dim() != 4 or pred.shape[0] != len(origins) * len(variants) or pred.shape[1] != heads:
        raise ValueError(f"window accumulate batch: prediction {tuple(pred.shape)} is not [{len(origins)} tiles * {len(variants)} variants, {heads} heads, th, tw]")
    th, tw = pred.shape[-2:]
    if g is not None and tuple(g.shape) != (th, tw):
        raise ValueError(f"window accumulate batch: importance map {tuple(g.shape)} does not match the tile {(th, tw)}")
    gg = None if g is None else g.to(acc.dtype).contiguous()
    pred = pred.contiguous()
    t = _window_tiles(origins, n_valid, variants)
    _lib.check(_lib.load().ldiff_op_window_accumulate_batch(_lib.ptr(acc), _lib.ptr(cnt), _lib.ptr(pred), _lib.ptr(gg), heads, acc.shape[1], acc.shape[2], th, tw, t,
                                                            _WINDOW_KINDS[(acc.dtype, pred.dtype)], _lib.stream_ptr()))


def window_finish(acc: torch.Tensor, cnt: torch.Tensor, box, inf_flag: torch.Tensor, logits: torch.Tensor = None, mask: torch.Tensor = None, mask_origin=(0, 0)) -> None:
    """One launch of ldiff_op_window_finish over box = (y0, x0, h, w) of the padded extent: logits [heads, h, w] (the accumulators' dtype) = acc / cnt, correctly
    rounded; inf_flag (device int32 [1], zeroed by the caller) set when any logit is +-inf; the uint8 arg-max (`segmentor.argmax_mask`'s rule) into
    mask [H0, W0] at mask_origin.  Either output may be None."""
    from . import _lib
    y0, x0, h, w = (int(v) for v in box)
    if acc.dtype not in (torch.float32, torch.float16) or acc.dtype != cnt.dtype or not (acc.is_cuda and acc.is_contiguous() and cnt.is_contiguous()):
        raise ValueError("window finish: contiguous float32 or float16 device accumulators of one dtype")
    if inf_flag.dtype != torch.int32 or not inf_flag.is_cuda or inf_flag.numel() < 1:
        raise ValueError("window finish: `inf_flag` must be a device int32 tensor")
    if logits is not None and (tuple(logits.shape) != (acc.shape[0], h, w) or logits.dtype != acc.dtype or not logits.is_contiguous() or not logits.is_cuda):
        raise ValueError(f"window finish: `logits` must be a contiguous {acc.dtype} device tensor {(acc.shape[0], h, w)}")
    mh = mw = 0
    if mask is not None:
        if mask.dim() != 2 or mask.dtype != torch.uint8 or not mask.is_contiguous() or not mask.is_cuda:
            raise ValueError("window finish: `mask` must be a contiguous uint8 device tensor [H0, W0]")
        mh, mw = mask.shape
    _lib.check(_lib.load().ldiff_op_window_finish(_lib.ptr(acc), _lib.ptr(cnt), acc.shape[0], acc.shape[1], acc.shape[2], y0, x0, h, w, int(acc.dtype == torch.float16),
                                                  _lib.ptr(logits), _lib.ptr(mask), mh, mw, int(mask_origin[0]), int(mask_origin[1]), _lib.ptr(inf_flag), _lib.stream_ptr()))


@torch.no_grad()
def window_accumulate_image(image: torch.Tensor, network, num_heads: int, tile_hw, tile_step_size: float = 0.5, use_gaussian: bool = True, mirror_axes=None,
                            acc_dtype=torch.float16, batch_tiles: int = 1):
    """The chunk loop of `predict_sliding_window_batched`: gather, ONE network call, accumulate, per chunk of the image's plan.  Returns (acc [num_heads, Hp, Wp],
    cnt [Hp, Wp], plan): the accumulators BEFORE the division, over the padded extent."""
    accs, cnt, plan = _window_accumulate_folds(image, [network], num_heads, tile_hw, tile_step_size, use_gaussian, mirror_axes, acc_dtype, batch_tiles)
    return accs[0], cnt, plan


def _window_accumulate_folds(image: torch.Tensor, networks, num_heads: int, tile_hw, tile_step_size, use_gaussian, mirror_axes, acc_dtype, batch_tiles):
    """`window_accumulate_image` for a list of networks: one plan, one gather per chunk, then per network in order one call and one accumulate launch into that
    network's own accumulators.  The count plane does not depend on the prediction: the first network's is returned, the others add into one scratch plane.
    Returns (accs, cnt, plan)."""
    if not isinstance(image, torch.Tensor) or not image.is_cuda:
        raise ValueError("predict_sliding_window_batched: `image` must be a tensor on the device (a host tensor goes through predict_sliding_window_return_logits)")
    if image.dim() != 3:
        raise ValueError("input_image must be [C, H, W]")
    if acc_dtype not in (torch.float32, torch.float16):
        raise ValueError(f"predict_sliding_window_batched: acc_dtype {acc_dtype} is not float32 or float16")
    num_heads = int(num_heads)
    if not 1 <= num_heads <= 32:
        raise ValueError(f"predict_sliding_window_batched: num_heads {num_heads} out of range [1, 32]")
    if image.dtype != torch.float32:
        image = image.float()
    if image.stride(2) != 1 or image.stride(1) < image.shape[2] or image.stride(0) < (image.shape[1] - 1) * image.stride(1) + image.shape[2]:
        image = image.contiguous()
    plan = window_plan(tuple(image.shape[1:]), tile_hw, tile_step_size, mirror_axes, batch_tiles)
    (th, tw), (Hp, Wp), dev = plan.tile_hw, plan.padded_hw, image.device
    want = (plan.batch, num_heads, th, tw)
    accs = [torch.zeros((num_heads, Hp, Wp), dtype=acc_dtype, device=dev) for _ in networks]
    cnt = torch.zeros((Hp, Wp), dtype=acc_dtype, device=dev)
    scratch = torch.zeros((Hp, Wp), dtype=acc_dtype, device=dev) if len(networks) > 1 else None
    g = compute_gaussian((th, tw), sigma_scale=1.0 / 8, value_scaling_factor=10, dtype=acc_dtype, device=dev) if use_gaussian else None
    x = torch.empty((plan.batch, image.shape[0], th, tw), dtype=torch.float32, device=dev)
    for origins, n_valid in plan.chunks:
        window_gather(image, plan, origins, out=x)
        for k, network in enumerate(networks):
            pred = network(x)
            if not isinstance(pred, torch.Tensor) or not pred.is_cuda:
                raise ValueError(f"predict_sliding_window_batched: the network must return a device tensor {want}")
            if tuple(pred.shape) != want:
                raise ValueError(f"predict_sliding_window_batched: the network returned {tuple(pred.shape)} for a batch of {plan.batch} "
                                 f"({plan.batch_tiles} tiles x {len(plan.variants)} mirror variants); expected {want}")
            if pred.dtype not in (torch.float32, torch.float16):
                raise ValueError(f"predict_sliding_window_batched: the network returned {pred.dtype}; expected float32 or float16")
            window_accumulate_batch(accs[k], cnt if k == 0 else scratch, pred, g, origins, n_valid, plan.variants)
    return accs, cnt, plan


@torch.no_grad()
def predict_sliding_window_batched(image: torch.Tensor, network, num_heads: int, tile_hw: Tuple[int, int], tile_step_size: float = 0.5, use_gaussian: bool = True,
                                   mirror_axes=None, acc_dtype=torch.float16, batch_tiles: int = 1, return_mask: bool = False, mask_out: torch.Tensor = None,
                                   mask_origin=(0, 0)):
    """`predict_sliding_window_return_logits` in a few launches per image.  Per chunk of `batch_tiles` tiles (`window_plan`): ldiff_op_window_gather builds
    x [batch_tiles * M, C, th, tw] float32 (tile-major, then the M mirror variants in `maybe_mirror_and_predict`'s order, already flipped), `network(x)` is called ONCE
    and must return [batch_tiles * M, num_heads, th, tw] in float32 or float16 on the device, ldiff_op_window_accumulate_batch un-flips, averages (every add and the
    division rounded to the prediction's dtype) and accumulates `logits[sl] += pred * g; n[sl] += g` in `acc_dtype`, tiles in slicer order; ldiff_op_window_finish
    divides (correctly rounded), flags inf, and writes the logits or the arg-max.  Every call of one image has the same batch: a short last chunk repeats its
    last tile and the repeats are not accumulated (the network must treat batch entries independently, as the library's head does bit for bit).
    acc and cnt before the division equal the per-tile path's bit for bit, for any `batch_tiles`; the logits are those of a correctly rounded division (the host's),
    where the per-tile path's device division of float16 accumulators may differ by one ulp.
    Device tensors only.  Returns [num_heads, H, W] in `acc_dtype`; with return_mask=True the uint8 arg-max instead, written into `mask_out` [H0, W0] (zeroed by the
    caller; default: a new [H, W] mask) at `mask_origin` -- `nnunet.uncrop_mask` without a copy.  The one host synchronisation is the read of the inf flag."""
    acc, cnt, plan = window_accumulate_image(image, network, num_heads, tile_hw, tile_step_size, use_gaussian, mirror_axes, acc_dtype, batch_tiles)
    (H, W), dev = plan.image_hw, acc.device
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    box = (plan.pad[0], plan.pad[1], H, W)
    if return_mask:
        out = mask_out if mask_out is not None else torch.zeros((H, W), dtype=torch.uint8, device=dev)
        window_finish(acc, cnt, box, flag, mask=out, mask_origin=mask_origin)
    else:
        out = torch.empty((acc.shape[0], H, W), dtype=acc_dtype, device=dev)
        window_finish(acc, cnt, box, flag, logits=out)
    if int(flag.item()):
        raise RuntimeError(_INF_MESSAGE)
    return out


# ---- several heads of one image: the folds of a cross-validation, averaged as nnUNetPredictor averages them -------------------------------
ENSEMBLE_MAX_FOLDS = 8   # LDIFF_ENSEMBLE_MAX_FOLDS: accumulators of one finish launch (their pointers travel by value in the kernel's arguments)


def window_finish_ensemble(accs, cnt, box, inf_flag: torch.Tensor, logits: torch.Tensor = None, mask: torch.Tensor = None, mask_origin=(0, 0)) -> None:
    """One launch of ldiff_op_window_finish_ensemble over box = (y0, x0, h, w): per fold `l_k = acc_k / cnt` as `window_finish` rounds it (cnt None: the entries of
    `accs` are logits already), inf_flag set when any l_k is +-inf, then `s = l_0; s += l_k` in order and `s /= len(accs)`, every step rounded to the accumulators'
    dtype (predict_from_raw_data.py:459-494); logits [heads, h, w] receives s, mask its arg-max at mask_origin.  Either output may be None."""
    import ctypes
    from . import _lib
    accs = list(accs)
    y0, x0, h, w = (int(v) for v in box)
    if not 1 <= len(accs) <= ENSEMBLE_MAX_FOLDS:
        raise ValueError(f"window finish ensemble: n_folds {len(accs)} out of range [1, {ENSEMBLE_MAX_FOLDS}]")
    first = accs[0]
    for k, acc in enumerate(accs):
        if not isinstance(acc, torch.Tensor) or acc.dtype not in (torch.float32, torch.float16) or acc.dim() != 3 or not (acc.is_cuda and acc.is_contiguous()):
            raise ValueError(f"window finish ensemble: accumulator {k} is no contiguous float32 or float16 device tensor [heads, Hp, Wp]")
        if acc.dtype != first.dtype or tuple(acc.shape) != tuple(first.shape) or acc.device != first.device:
            raise ValueError(f"window finish ensemble: accumulator {k} ({acc.dtype} {tuple(acc.shape)} on {acc.device}) does not match accumulator 0 "
                             f"({first.dtype} {tuple(first.shape)} on {first.device})")
    if cnt is not None and (cnt.dtype != first.dtype or tuple(cnt.shape) != tuple(first.shape[1:]) or not (cnt.is_cuda and cnt.is_contiguous())):
        raise ValueError(f"window finish ensemble: `cnt` must be a contiguous {first.dtype} device tensor {tuple(first.shape[1:])}")
    if inf_flag.dtype != torch.int32 or not inf_flag.is_cuda or inf_flag.numel() < 1:
        raise ValueError("window finish ensemble: `inf_flag` must be a device int32 tensor")
    if logits is not None and (tuple(logits.shape) != (first.shape[0], h, w) or logits.dtype != first.dtype or not logits.is_contiguous() or not logits.is_cuda):
        raise ValueError(f"window finish ensemble: `logits` must be a contiguous {first.dtype} device tensor {(first.shape[0], h, w)}")
    mh = mw = 0
    if mask is not None:
        if mask.dim() != 2 or mask.dtype != torch.uint8 or not mask.is_contiguous() or not mask.is_cuda:
            raise ValueError("window finish ensemble: `mask` must be a contiguous uint8 device tensor [H0, W0]")
        mh, mw = mask.shape
    table = (ctypes.c_void_p * len(accs))(*[acc.data_ptr() for acc in accs])
    _lib.check(_lib.load().ldiff_op_window_finish_ensemble(table, len(accs), _lib.ptr(cnt), first.shape[0], first.shape[1], first.shape[2], y0, x0, h, w,
                                                           int(first.dtype == torch.float16), _lib.ptr(logits), _lib.ptr(mask), mh, mw, int(mask_origin[0]),
                                                           int(mask_origin[1]), _lib.ptr(inf_flag), _lib.stream_ptr()))


@torch.no_grad()
def predict_sliding_window_ensemble(image: torch.Tensor, networks, num_heads: int, tile_hw: Tuple[int, int], tile_step_size: float = 0.5, use_gaussian: bool = True,
                                    mirror_axes=None, acc_dtype=torch.float16, batch_tiles=1, return_mask: bool = False, mask_out: torch.Tensor = None,
                                    mask_origin=(0, 0)):
    """nnUNetPredictor.predict_logits_from_preprocessed_data for several parameter sets (predict_from_raw_data.py:459-494): every network's sliding window over the
    image, the logits summed in the networks' order and divided by their number, each step rounded to `acc_dtype`.
    batch_tiles an integer: `predict_sliding_window_batched`'s launches with ONE plan and one gather per chunk; every network is called once per chunk on the same
    batch and accumulated into its own accumulators; ONE ldiff_op_window_finish_ensemble divides every fold by the count plane (the same for every fold: the first
    one's is used), flags inf per fold, averages and writes the logits or the arg-max; one read of the inf flag.  With one network the result is
    `predict_sliding_window_batched`'s bit for bit.
    batch_tiles None: each network's `predict_sliding_window_return_logits` (which raises on inf itself), then the same kernel without a count plane.
    Returns and `return_mask`, `mask_out`, `mask_origin` as `predict_sliding_window_batched`."""
    networks = list(networks)
    if not 1 <= len(networks) <= ENSEMBLE_MAX_FOLDS:
        raise ValueError(f"predict_sliding_window_ensemble: {len(networks)} networks; one launch averages 1 to {ENSEMBLE_MAX_FOLDS}")
    if batch_tiles is None:
        if not isinstance(image, torch.Tensor) or not image.is_cuda:
            raise ValueError("predict_sliding_window_ensemble: `image` must be a tensor on the device")
        accs = [predict_sliding_window_return_logits(image, net, num_heads, tile_hw, tile_step_size, use_gaussian, mirror_axes, acc_dtype).contiguous() for net in networks]
        cnt, (H, W), box, dev = None, tuple(accs[0].shape[1:]), (0, 0) + tuple(accs[0].shape[1:]), accs[0].device
    else:
        accs, cnt, plan = _window_accumulate_folds(image, networks, num_heads, tile_hw, tile_step_size, use_gaussian, mirror_axes, acc_dtype, batch_tiles)
        (H, W), dev = plan.image_hw, accs[0].device
        box = (plan.pad[0], plan.pad[1], H, W)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    if return_mask:
        out = mask_out if mask_out is not None else torch.zeros((H, W), dtype=torch.uint8, device=dev)
        window_finish_ensemble(accs, cnt, box, flag, mask=out, mask_origin=mask_origin)
    else:
        out = torch.empty((accs[0].shape[0], H, W), dtype=acc_dtype, device=dev)
        window_finish_ensemble(accs, cnt, box, flag, logits=out)
    if int(flag.item()):
        raise RuntimeError(_INF_MESSAGE)
    return out
