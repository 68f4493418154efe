"""The nnU-Net v2 tissue head: what `nnUNetPredictor.initialize_from_trained_model_folder(segmentor_weight, use_folds=(0,),
checkpoint_name='checkpoint_best.pth')` (/root/reference/segmentor.py:463-468) reads, resolved for the one architecture the HIP library runs.

Covered: `PlainConvUNet`, 2-D, one fold, as model/nnunetv2/utilities/get_network_from_plans.py builds it (conv bias, InstanceNorm2d(eps=1e-5, affine),
LeakyReLU(0.01), stride-in-conv downsampling, transposed-conv upsampling with kernel = stride, deep supervision off), 3x3 kernels, strides 1 (first
stage) and 2 (every later stage) in both axes.  Everything else a plans file can ask for is refused with a ValueError that names the field.

The state-dict key layout belongs to the package `dynamic_network_architectures`, which the test-suite cannot import: it is restated here from
knowledge of that package and is UNPINNED; scripts/gen_golden_nnunet.py pins names and one forward pass where it is installed.

Nothing in this module touches the GPU except `load_trained_model_folder` (which builds `models.PlainConvUNet`) and the tensors callers hand in.
"""
from __future__ import annotations

import json
import os
import re
from copy import deepcopy
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

NORMALIZATIONS = ("ZScoreNormalization", "RGBTo01Normalization", "RescaleTo01Normalization", "NoNormalization")
# map_channel_name_to_normalization.py: channel names that are not in the mapping (the reference's own datasets name theirs R / G / B,
# /root/reference/utils.py:277-281) fall back to z-score
CHANNEL_NAME_TO_NORMALIZATION = {"noNorm": "NoNormalization", "zscore": "ZScoreNormalization", "rescale_to_0_1": "RescaleTo01Normalization",
                                 "rgb_to_0_1": "RGBTo01Normalization", "CT": "CTNormalization"}


def _refuse(field: str, why: str):
    raise ValueError(f"nnU-Net plans: `{field}` {why}; the HIP tissue head covers PlainConvUNet, 2-D, 3x3 kernels, strides 1 / 2, one fold")


def resolve_configuration(plans: dict, name: str) -> dict:
    """PlansManager._internal_resolve_configuration_inheritance (plans_handler.py:197-219): `inherits_from` chains, child keys win."""
    visited: Tuple[str, ...] = ()
    chain = []
    cur = name
    while True:
        if cur not in plans.get("configurations", {}):
            raise ValueError(f"The configuration {cur} does not exist in the plans. Valid configuration names are {list(plans.get('configurations', {}))}.")
        if cur in visited:
            raise RuntimeError(f"Circular dependency detected while solving `inherits_from`: {visited + (cur,)}")
        visited += (cur,)
        cfg = plans["configurations"][cur]
        chain.append(cfg)
        if "inherits_from" not in cfg:
            break
        cur = cfg["inherits_from"]
    out: dict = {}
    for cfg in reversed(chain):
        out.update(deepcopy(cfg))
    return out


def label_spec(labels: dict) -> Tuple[int, Optional[int]]:
    """(n_heads, ignore_label) of a dataset.json `labels` mapping, by LabelManager's rules (label_handling.py:35-45, 101-106): the optional entry
    `"ignore"` must be an integer and the highest value, max(all other labels) + 1 -- with consecutive labels their number, so it is the first value
    the network has no head for; `n_heads` leaves it out.  Regions (they go through `region_spec`), and an ignore entry that breaks the rule, are refused
    naming the field."""
    if any(isinstance(v, (list, tuple)) for v in labels.values()):
        _refuse("labels", "defines regions")
    if "ignore" not in labels:
        return len(labels), None
    k, n_heads = labels["ignore"], len(labels) - 1
    if isinstance(k, bool) or not isinstance(k, int):
        _refuse("labels", f"has an ignore label that is not an integer: {k!r}")
    if k != n_heads:
        _refuse("labels", f"has the ignore label {k}, which is not the highest value, the number of other labels {n_heads}")
    return n_heads, k


# `sigmoid(logit) > 0.5` is a step function of the logit; the step depends on the dtype the sigmoid is taken in.  Each constant is the LARGEST logit that
# still compares false, so the rule is `logit > threshold` (tests/test_cpu_nnunet_regions.py finds both again with torch on the CPU):
#   inference thresholds sigmoid(l.float()) (label_handling.py:136-141, 171): float32; torch's 1 / (1 + exp(-x)) gives 0.5 up to x = 1.5 * 2^-24, where
#   1 + exp(-x) still rounds to 2 (bisection over float32, and every float32 of [2^-27, 2^-21) enumerated: one step);
#   validation thresholds torch.sigmoid(output) on the network's float16 output (nnUNetTrainer.py:960): the float32 value rounds to the float16 0.5 up
#   to x = 2^-10, a tie that goes to even (all finite float16 values enumerated).
REGION_THRESHOLD_F32 = 1.5 * 2.0 ** -24
REGION_THRESHOLD_F16 = 2.0 ** -10
REGION_IGNORE_BIT, REGION_BAD_BIT, REGION_MAX = 1 << 31, 1 << 30, 24


def has_regions(labels: dict) -> bool:
    """LabelManager's rule (label_handling.py:32-33): an entry that lists more than one value."""
    return any(isinstance(v, (list, tuple)) and len(v) > 1 for v in labels.values())


def region_spec(labels: dict, regions_class_order) -> dict:
    """LabelManager (label_handling.py:22-100, 204-234) for a dataset.json `labels` mapping with list-valued entries:
    `all_labels` (sorted, the ignore label left out), `foreground_regions` (dictionary order, as tuples or single integers; entries that are only
    background dropped, a region that holds 0 among other labels kept), `n_heads` = their number, `ignore_label` (None, or the integer max(all_labels) + 1),
    `regions_class_order` (required, one entry per region, each 0 .. 255: the value `ldiff_op_region_mask_u8` writes) and `table`: uint32 [256] indexed by
    label value -- bit r: the value belongs to foreground region r; bit 31: the ignore label; bit 30: neither a label nor the ignore label.
    Refusals name the field."""
    if "background" not in labels or isinstance(labels["background"], (list, tuple)) or int(labels["background"]) != 0:
        _refuse("labels", "must declare `background` as the label 0")
    ignore = labels.get("ignore")
    if ignore is not None and (isinstance(ignore, bool) or not isinstance(ignore, int)):
        _refuse("labels", f"has an ignore label that is not an integer: {ignore!r}")
    if not has_regions(labels):   # LabelManager reads such a mapping as plain classes (softmax heads), single-valued lists included
        _refuse("labels", "defines no region of more than one value, so nnU-Net reads it as plain labels")
    all_labels, regions = set(), []
    for name, r in labels.items():
        if name == "ignore":
            continue
        values = [int(v) for v in r] if isinstance(r, (list, tuple)) else [int(r)]
        all_labels.update(values)
        if set(values) == {0}:   # a region that is only background
            continue
        regions.append(tuple(values) if isinstance(r, (list, tuple)) else int(r))
    all_labels = sorted(all_labels)
    if all_labels[0] < 0 or all_labels[-1] > 254:
        _refuse("labels", f"holds values outside 0 .. 254: {all_labels[0]} .. {all_labels[-1]} (label maps are bytes, and 255 stands for every value beyond them)")
    if ignore is not None and ignore != all_labels[-1] + 1:
        _refuse("labels", f"has the ignore label {ignore}, which is not the highest value, max(all labels) + 1 = {all_labels[-1] + 1}")
    if len(regions) < 1:
        _refuse("labels", "defines no foreground region")
    if len(regions) > REGION_MAX:
        _refuse("labels", f"defines {len(regions)} regions; the membership table has {REGION_MAX} region bits")
    if regions_class_order is None:
        _refuse("regions_class_order", "is missing, and region labels need it")
    order = list(regions_class_order)
    if len(order) != len(regions):
        _refuse("regions_class_order", f"has {len(order)} entries for {len(regions)} regions")
    if any(isinstance(c, bool) or int(c) != c or not 0 <= int(c) <= 255 for c in order):
        _refuse("regions_class_order", f"holds an entry that is no integer in 0 .. 255: {order}")
    table = [REGION_BAD_BIT] * 256
    for v in all_labels:
        table[v] = 0
    for i, r in enumerate(regions):
        for v in (r if isinstance(r, tuple) else (r,)):
            table[v] |= 1 << i
    if ignore is not None:
        table[ignore] = REGION_IGNORE_BIT
    return dict(all_labels=all_labels, foreground_regions=regions, n_heads=len(regions), ignore_label=ignore, regions_class_order=[int(c) for c in order],
                table=np.array(table, dtype=np.uint32))


def region_table_tensor(table, device=None) -> torch.Tensor:
    """The membership table as the kernels take it: the uint32 [256] bit patterns in an int32 tensor (torch has no arithmetic on uint32), on `device`."""
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(table, dtype=np.uint32)).view(np.int32).copy())
    return t if device is None else t.to(device)


def network_spec(plans: dict, configuration_name: str, dataset_json: dict, accept_ignore: bool = False, accept_regions: bool = False) -> dict:
    """The layer list of the network `get_network_from_plans` would build, plus what the sliding window and the preprocessing need.
    Refuses, naming the field, whatever the HIP head does not cover.  `accept_ignore`: a dataset with an ignore label (`label_spec`) is taken and
    adds `ignore_label` to the spec; `n_heads` never counts it, so no head can predict it.  Off, the default, such a dataset is refused as it always
    was: a caller that has not asked for the label would train on it as a class of its own.
    `accept_regions`: a dataset whose labels define regions is taken through `region_spec`: `n_heads` is the number of foreground regions (one sigmoid head
    each) and the spec gains `regions`, `regions_class_order`, `region_table` and, where one is declared, `ignore_label`.  Off, it is refused as before."""
    cfg = resolve_configuration(plans, configuration_name)
    if cfg.get("UNet_class_name") != "PlainConvUNet":
        _refuse("UNet_class_name", f"is {cfg.get('UNet_class_name')!r}")
    if cfg.get("previous_stage") is not None:
        _refuse("previous_stage", "names a cascade")
    ks = cfg["conv_kernel_sizes"]
    pool = cfg["pool_op_kernel_sizes"]
    n_stages = len(ks)
    if any(len(k) != 2 for k in ks):
        _refuse("conv_kernel_sizes", f"is {len(ks[0])}-dimensional")
    if any(list(k) != [3, 3] for k in ks):
        _refuse("conv_kernel_sizes", f"holds a kernel other than [3, 3]: {ks}")
    if len(pool) != n_stages or any(len(p) != 2 or p[0] != p[1] for p in pool):
        _refuse("pool_op_kernel_sizes", f"is anisotropic or does not match the stages: {pool}")
    strides = [int(p[0]) for p in pool]
    if n_stages < 2 or strides[0] != 1 or any(s != 2 for s in strides[1:]):
        _refuse("pool_op_kernel_sizes", f"must be [1, 1] for the first stage and [2, 2] for every later one: {pool}")
    if any(bool(m) for m in cfg.get("use_mask_for_norm", [])):
        _refuse("use_mask_for_norm", "is true for a channel")
    tf = list(plans.get("transpose_forward", [0, 1, 2]))
    if tf != sorted(tf):
        _refuse("transpose_forward", f"is not the identity: {tf}")
    schemes = list(cfg["normalization_schemes"])
    for s in schemes:
        if s not in NORMALIZATIONS:
            _refuse("normalization_schemes", f"names {s!r}")
    regions = None
    if accept_regions and has_regions(dataset_json["labels"]):
        regions = region_spec(dataset_json["labels"], dataset_json.get("regions_class_order"))
        n_heads, ignore_label = regions["n_heads"], regions["ignore_label"]
    else:
        n_heads, ignore_label = label_spec(dataset_json["labels"])
    if ignore_label is not None and regions is None and not accept_ignore:
        _refuse("labels", "defines an ignore label (network_spec(accept_ignore=True) takes it)")
    channels = dataset_json["channel_names"] if "channel_names" in dataset_json else dataset_json["modality"]
    in_channels = len(channels)
    if len(schemes) != in_channels:
        _refuse("normalization_schemes", f"has {len(schemes)} entries for {in_channels} channels")
    base, cap = int(cfg["UNet_base_num_features"]), int(cfg["unet_max_num_features"])
    features = [min(base * 2 ** i, cap) for i in range(n_stages)]
    if any(f % 16 for f in features):
        _refuse("UNet_base_num_features", f"gives stage widths that are not multiples of 16: {features}")
    nce, ncd = [int(v) for v in cfg["n_conv_per_stage_encoder"]], [int(v) for v in cfg["n_conv_per_stage_decoder"]]
    if len(nce) != n_stages or len(ncd) != n_stages - 1:
        _refuse("n_conv_per_stage_encoder", f"/ n_conv_per_stage_decoder do not match {n_stages} stages: {nce} / {ncd}")
    patch = [int(v) for v in cfg["patch_size"]]
    div = 1
    for s in strides:
        div *= s
    if len(patch) != 2 or any(p % div for p in patch):
        _refuse("patch_size", f"{patch} is not divisible by the product of the strides, {div}")
    spec = dict(in_channels=in_channels, n_stages=n_stages, features=features, strides=strides, n_conv_encoder=nce, n_conv_decoder=ncd,
                n_heads=n_heads, patch_size=tuple(patch), normalization_schemes=schemes)
    if ignore_label is not None:
        spec["ignore_label"] = ignore_label
    if regions is not None:
        spec.update(regions=regions["foreground_regions"], regions_class_order=regions["regions_class_order"], region_table=regions["table"])
    return spec


def param_shapes(spec: dict, deep_supervision: bool = False) -> Dict[str, Tuple[int, ...]]:
    """name -> shape of every tensor the handle expects (the canonical names of a PlainConvUNet state dict; see the module docstring: unpinned).
    deep_supervision: also the heads of the lower decoder stages, `decoder.seg_layers.0 .. n_stages - 3` (stage j ends at width features[n - 2 - j]):
    what the network holds while it trains (nnunet_train) and what a checkpoint's `network_weights` lists."""
    out: Dict[str, Tuple[int, ...]] = {}
    f, n = spec["features"], spec["n_stages"]

    def block(prefix, cin, cout):
        out[prefix + ".conv.weight"] = (cout, cin, 3, 3)
        out[prefix + ".conv.bias"] = (cout,)
        out[prefix + ".norm.weight"] = (cout,)
        out[prefix + ".norm.bias"] = (cout,)

    for s in range(n):
        cin = spec["in_channels"] if s == 0 else f[s - 1]
        for i in range(spec["n_conv_encoder"][s]):
            block(f"encoder.stages.{s}.0.convs.{i}", cin, f[s])
            cin = f[s]
    for j in range(n - 1):
        below, skip = f[n - 1 - j], f[n - 2 - j]
        out[f"decoder.transpconvs.{j}.weight"] = (below, skip, 2, 2)
        out[f"decoder.transpconvs.{j}.bias"] = (skip,)
        cin = 2 * skip
        for i in range(spec["n_conv_decoder"][j]):
            block(f"decoder.stages.{j}.convs.{i}", cin, skip)
            cin = skip
    for j in (range(n - 1) if deep_supervision else (n - 2,)):
        out[f"decoder.seg_layers.{j}.weight"] = (spec["n_heads"], f[n - 2 - j], 1, 1)
        out[f"decoder.seg_layers.{j}.bias"] = (spec["n_heads"],)
    return out


_SEG = re.compile(r"^decoder\.seg_layers\.(\d+)\.")


def clean_state_dict(sd: dict, spec: dict) -> dict:
    """Drop what a checkpoint holds beside the canonical names: the `_orig_mod.` prefix of a compiled network, the `....all_modules.{k}.*`
    views of conv / norm, the decoder's reference to the encoder (`decoder.encoder.*`) and the deep-supervision heads that do not run."""
    used = spec["n_stages"] - 2
    out = {}
    for k, v in sd.items():
        if k.startswith("_orig_mod."):
            k = k[len("_orig_mod."):]
        if ".all_modules." in k or k.startswith("decoder.encoder."):
            continue
        m = _SEG.match(k)
        if m and int(m.group(1)) != used:
            continue
        out[k] = v
    return out


def check_state_dict(sd: dict, spec: dict) -> None:
    """Names and shapes against `param_shapes`: an unexpected name, a missing tensor (by name) or a wrong shape raises."""
    want = param_shapes(spec)
    unexpected = [k for k in sd if k not in want]
    if unexpected:
        raise ValueError(f"unexpected tensors in checkpoint: {unexpected[:5]}{' ...' if len(unexpected) > 5 else ''}")
    missing = [k for k in want if k not in sd]
    if missing:
        raise RuntimeError(f"{len(missing)} nnU-Net tensors missing from the checkpoint, e.g. {missing[:5]}")
    for k, shape in want.items():
        if tuple(sd[k].shape) != tuple(shape):
            raise ValueError(f"load({k}): shape {list(sd[k].shape)} does not match expected {list(shape)}")


# ---- preprocessing: DefaultPreprocessor.run_case_npy for a PNG (default_preprocessor.py:40-113), on the tensor's device ----
def nonzero_bbox(data: torch.Tensor) -> Tuple[int, int, int, int]:
    """crop_to_nonzero's box for [C, H, W]: rows / columns where any channel is non-zero, as (y0, y1, x0, x1), end exclusive (filling holes of the
    mask, as create_nonzero_mask does, never moves its bounding box).  An all-zero image keeps its full extent."""
    nz = (data != 0).any(0)
    rows, cols = nz.any(1).nonzero().flatten(), nz.any(0).nonzero().flatten()
    if rows.numel() == 0:
        return 0, int(data.shape[1]), 0, int(data.shape[2])
    return int(rows[0]), int(rows[-1]) + 1, int(cols[0]), int(cols[-1]) + 1


def normalize(data: torch.Tensor, schemes: Sequence[str]) -> torch.Tensor:
    """default_normalization_schemes.py, per channel of a float32 [C, H, W] (use_mask_for_norm false): ZScoreNormalization (x - mean) / max(std, 1e-8)
    with the population std; RGBTo01Normalization x / 255; RescaleTo01Normalization (x - min) / max(max - min, 1e-8); NoNormalization."""
    out = torch.empty_like(data, dtype=torch.float32)
    for c, scheme in enumerate(schemes):
        x = data[c].to(torch.float32)
        if scheme == "ZScoreNormalization":
            out[c] = (x - x.mean()) / max(float(x.std(unbiased=False)), 1e-8)
        elif scheme == "RGBTo01Normalization":
            if float(x.min()) < 0 or float(x.max()) > 255:
                raise ValueError("RGBTo01Normalization: pixel values outside 0..255")
            out[c] = x / 255.0
        elif scheme == "RescaleTo01Normalization":
            x = x - x.min()
            out[c] = x / max(float(x.max()), 1e-8)
        elif scheme == "NoNormalization":
            out[c] = x
        else:
            _refuse("normalization_schemes", f"names {scheme!r}")
    return out


def preprocess(data: torch.Tensor, schemes: Sequence[str]):
    """[C, H, W] in the PNG's 0..255 scale -> (cropped + normalised float32 [C, h, w], (y0, y1, x0, x1)); no resampling (a PNG has spacing 1)."""
    box = nonzero_bbox(data)
    return normalize(data[:, box[0]:box[1], box[2]:box[3]].to(torch.float32), schemes), box


def uncrop_mask(mask: torch.Tensor, box, full_hw) -> torch.Tensor:
    """Pixels outside the crop box are label 0 (export_prediction.py: insert_crop_into_image on a zero array)."""
    out = torch.zeros(tuple(full_hw), dtype=mask.dtype, device=mask.device)
    out[box[0]:box[1], box[2]:box[3]] = mask
    return out


def region_mask_u8(logits: torch.Tensor, regions_class_order, threshold: float = REGION_THRESHOLD_F32, out: torch.Tensor = None, origin=(0, 0)) -> torch.Tensor:
    """ldiff_op_region_mask_u8: LabelManager.convert_probabilities_to_segmentation's region branch on device logits [R, H, W] (float16 or float32) --
    0, then regions_class_order[i] where logit i > threshold, in order.  Written into `out` (uint8 [H0, W0] on the device) at `origin`, or a new [H, W] mask."""
    import ctypes
    from . import _lib
    if logits.dim() != 3 or not logits.is_cuda or logits.dtype not in (torch.float16, torch.float32):
        raise ValueError("region_mask_u8: `logits` must be a float16 or float32 device tensor [R, H, W]")
    logits = logits.contiguous()
    R, H, W = logits.shape
    order = [int(c) for c in regions_class_order]
    if len(order) != R:
        raise ValueError(f"region_mask_u8: regions_class_order has {len(order)} entries for {R} regions")
    if out is None:
        out = torch.empty((H, W), dtype=torch.uint8, device=logits.device)
    elif out.dim() != 2 or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != logits.device:
        raise ValueError("region_mask_u8: `out` must be a contiguous uint8 tensor [H0, W0] on the logits' device")
    _lib.check(_lib.load().ldiff_op_region_mask_u8(_lib.ptr(logits), int(logits.dtype == torch.float32), R, H, W, (ctypes.c_int * R)(*order), float(threshold),
                                                   _lib.ptr(out), out.shape[0], out.shape[1], int(origin[0]), int(origin[1]), _lib.stream_ptr()))
    return out


class TrainedModel:
    """What the predictor keeps after initialize_from_trained_model_folder: `.network` (callable [B, C, h, w] -> [B, heads, h, w]), `.patch_size`,
    `.mirror_axes` (the checkpoint's inference_allowed_mirroring_axes), `.normalization_schemes`, `.num_heads`, `.spec`."""

    def __init__(self, network, spec: dict, mirror_axes):
        self.network = network
        self.spec = spec
        self.patch_size = tuple(spec["patch_size"])
        self.mirror_axes = None if mirror_axes is None else tuple(int(a) for a in mirror_axes)
        self.normalization_schemes = list(spec["normalization_schemes"])
        self.num_heads = int(spec["n_heads"])

    def __call__(self, x):
        return self.network(x)

    @torch.no_grad()
    def predict_mask(self, data: torch.Tensor, tile_size=None, tile_step_size: float = 0.5, mirror_axes="checkpoint", network=None,
                     batch_tiles=None, postprocess=None) -> torch.Tensor:
        """[C, H, W] in 0..255 scale on the device -> uint8 mask [H, W]: crop to non-zero, normalise, nnU-Net's sliding window, arg-max, un-crop.
        The tile is the plans' patch size (or `tile_size`), NOT clamped to the image: an image smaller than the patch is zero padded to it
        (predict_from_raw_data.py:614, tiling.pad_to_tile), as the reference does -- InstanceNorm statistics and Gaussian weights are then those of a full patch.
        `network` replaces the head (tests: a float64 restatement under the same preprocessing).
        batch_tiles: None = one network call per tile and mirror variant; an integer = `tiling.predict_sliding_window_batched`: that many tiles times the mirror
        variants per network call, the mask written at the crop box's place by the finish kernel.  The same mask bit for bit (the head is batch invariant).
        postprocess: None = the mask as predicted; `(fns, kwargs)` or the path of a `postprocessing.json` (`nnunet_post.determine_postprocessing*`) = nnU-Net's
        fitted postprocessing applied to the finished, un-cropped mask on the device (`nnunet_post.apply_postprocessing`)."""
        return _predict_mask(self, [network if network is not None else self.network], False, data, tile_size, tile_step_size, mirror_axes, batch_tiles, postprocess)


def _predict_mask(head, networks, ensemble: bool, data: torch.Tensor, tile_size, tile_step_size, mirror_axes, batch_tiles, postprocess) -> torch.Tensor:
    """`TrainedModel.predict_mask` and `FoldEnsemble.predict_mask`: preprocessing, tile check, crop box, the sliding window of `networks` (one head: `tiling`'s
    single-head entries as ever; `ensemble`: `tiling.predict_sliding_window_ensemble`), region rule or arg-max, un-crop, postprocessing.  `head` gives spec, patch
    size, mirror axes, normalisation and head count."""
    if postprocess is not None:
        from . import nnunet_post
        fns, kwargs = nnunet_post.load_postprocessing(postprocess) if isinstance(postprocess, (str, os.PathLike)) else postprocess
        mask = _predict_mask(head, networks, ensemble, data, tile_size, tile_step_size, mirror_axes, batch_tiles, None)
        return nnunet_post.apply_postprocessing(mask.contiguous(), fns, kwargs)
    from . import tiling
    from .segmentor import argmax_mask
    x, box = preprocess(data, head.normalization_schemes)
    tile = tuple(int(t) for t in tile_size) if tile_size is not None else head.patch_size
    div = 1
    for st in head.spec["strides"]:
        div *= st
    if len(tile) != 2 or any(t < div or t % div for t in tile):
        raise ValueError(f"tile_size {tile} must be a multiple of the product of the network's strides, {div}, in both axes")
    axes = head.mirror_axes if mirror_axes == "checkpoint" else mirror_axes
    bt = None if batch_tiles is None else int(batch_tiles)
    if "regions" in head.spec:   # one sigmoid head per region: the region rule in place of the arg-max; outside the crop box 0 (revert_cropping_on_probabilities)
        if ensemble:
            logits = tiling.predict_sliding_window_ensemble(x, networks, head.num_heads, tile, tile_step_size, True, axes, batch_tiles=bt)
        elif bt is not None:
            logits = tiling.predict_sliding_window_batched(x, networks[0], head.num_heads, tile, tile_step_size, True, axes, batch_tiles=bt)
        else:
            logits = tiling.predict_sliding_window_return_logits(x, networks[0], head.num_heads, tile, tile_step_size, True, axes)
        out = torch.zeros(tuple(data.shape[1:]), dtype=torch.uint8, device=x.device)
        return region_mask_u8(logits, head.spec["regions_class_order"], REGION_THRESHOLD_F32, out=out, origin=(box[0], box[2]))
    if ensemble or bt is not None:
        out = torch.zeros(tuple(data.shape[1:]), dtype=torch.uint8, device=x.device)   # pixels outside the crop box are label 0 (uncrop_mask)
        if ensemble:
            return tiling.predict_sliding_window_ensemble(x, networks, head.num_heads, tile, tile_step_size, True, axes, batch_tiles=bt, return_mask=True, mask_out=out,
                                                          mask_origin=(box[0], box[2]))
        return tiling.predict_sliding_window_batched(x, networks[0], head.num_heads, tile, tile_step_size, True, axes, batch_tiles=bt, return_mask=True, mask_out=out,
                                                     mask_origin=(box[0], box[2]))
    logits = tiling.predict_sliding_window_return_logits(x, networks[0], head.num_heads, tile, tile_step_size, True, axes)
    return uncrop_mask(argmax_mask(logits[None].float())[0], box, data.shape[1:])


class FoldEnsemble:
    """The folds of one trained-model folder behind one `predict_mask`: what nnUNetPredictor holds after `initialize_from_trained_model_folder(..., use_folds=(0, 1, ...))`
    -- `.models` (one `TrainedModel` per fold, in the given order), and `.spec`, `.patch_size`, `.mirror_axes`, `.normalization_schemes`, `.num_heads` of the FIRST
    fold (predict_from_raw_data.py:95-105 keeps the first checkpoint's trainer name, configuration and mirroring axes)."""

    def __init__(self, models, folds=None):
        self.models = list(models)
        if not self.models:
            raise ValueError("FoldEnsemble: no folds")
        self.folds = tuple(folds) if folds is not None else tuple(range(len(self.models)))
        first = self.models[0]
        self.spec, self.patch_size, self.mirror_axes = first.spec, first.patch_size, first.mirror_axes
        self.normalization_schemes, self.num_heads = first.normalization_schemes, first.num_heads

    @torch.no_grad()
    def predict_mask(self, data: torch.Tensor, tile_size=None, tile_step_size: float = 0.5, mirror_axes="checkpoint", network=None,
                     batch_tiles=None, postprocess=None) -> torch.Tensor:
        """`TrainedModel.predict_mask` with the folds' logits averaged before the arg-max (or the region rule), on the device, with the reference's roundings
        (`tiling.predict_sliding_window_ensemble`).  `network`: a sequence of callables that replaces the folds' heads, one per fold."""
        networks = [m.network for m in self.models] if network is None else list(network)
        return _predict_mask(self, networks, True, data, tile_size, tile_step_size, mirror_axes, batch_tiles, postprocess)


def read_trained_model_folder(model_dir: str, fold=0, checkpoint_name: str = "checkpoint_best.pth"):
    """predict_from_raw_data.py:78-121 without the network: (spec, cleaned state dict, inference_allowed_mirroring_axes)."""
    if isinstance(fold, (list, tuple)):
        if len(fold) != 1:
            _refuse("use_folds", f"names {len(fold)} folds")
        fold = fold[0]
    plans, dataset_json = _read_model_jsons(model_dir)
    ckpt = _load_fold_checkpoint(model_dir, fold, checkpoint_name)
    spec = _checkpoint_spec(ckpt, plans, dataset_json)
    return spec, _checked_state_dict(ckpt, spec), ckpt.get("inference_allowed_mirroring_axes")


# one reading of a trained-model folder's files, for `read_trained_model_folder` and `read_fold_ensemble`
def _read_model_jsons(model_dir: str):
    with open(os.path.join(model_dir, "dataset.json")) as f:
        dataset_json = json.load(f)
    with open(os.path.join(model_dir, "plans.json")) as f:
        plans = json.load(f)
    return plans, dataset_json


def _load_fold_checkpoint(model_dir: str, fold, checkpoint_name: str) -> dict:
    return torch.load(os.path.join(model_dir, f"fold_{fold}", checkpoint_name), map_location="cpu", weights_only=False)


def _checkpoint_spec(ckpt: dict, plans: dict, dataset_json: dict) -> dict:
    # the network has no head for an ignore label: inference is the same.  A trained folder with region labels was made on purpose: no opt-in to load it
    return network_spec(plans, ckpt["init_args"]["configuration"], dataset_json, accept_ignore=True, accept_regions=True)


def _checked_state_dict(ckpt: dict, spec: dict) -> dict:
    sd = clean_state_dict(ckpt["network_weights"], spec)
    check_state_dict(sd, spec)
    return sd


def write_trained_model_folder(path: str, plans: dict, dataset_json: dict) -> str:
    """The two JSON files nnU-Net keeps beside `fold_0/` in a trained-model folder (nnUNetTrainer.__init__ / run_training: plans.json, dataset.json);
    the checkpoints themselves are written by nnunet_train.Trainer.save_checkpoint.  Returns `path`."""
    os.makedirs(os.path.join(path, "fold_0"), exist_ok=True)
    with open(os.path.join(path, "dataset.json"), "w") as f:
        json.dump(dataset_json, f, indent=4)
    with open(os.path.join(path, "plans.json"), "w") as f:
        json.dump(plans, f, indent=4)
    return path


def load_trained_model_folder(model_dir: str, fold=0, checkpoint_name: str = "checkpoint_best.pth", device=None) -> TrainedModel:
    from .models import PlainConvUNet
    spec, sd, axes = read_trained_model_folder(model_dir, fold, checkpoint_name)
    return TrainedModel(PlainConvUNet(spec, sd, device=device), spec, axes)


def available_folds(model_dir: str, checkpoint_name: str = "checkpoint_best.pth") -> List[int]:
    """nnUNetPredictor.auto_detect_available_folds (predict_from_raw_data.py:123-131): the `fold_<int>` folders of `model_dir` that hold `checkpoint_name`, sorted;
    `fold_all` is never among them."""
    folds = []
    for name in os.listdir(model_dir):
        m = re.fullmatch(r"fold_(\d+)", name)
        if m and os.path.isfile(os.path.join(model_dir, name, checkpoint_name)):
            folds.append(int(m.group(1)))
    return sorted(folds)


def check_folds(folds, what: str = "use_folds") -> Tuple[int, ...]:
    """A sequence of distinct fold numbers as a tuple of ints; `all` and anything that is no integer are refused by name."""
    if isinstance(folds, (str, bytes)) or not isinstance(folds, (list, tuple)):
        raise ValueError(f"`{what}` must be a sequence of fold numbers, not {folds!r}" + (" (fold \"all\" is not covered)" if folds == "all" else ""))
    out = []
    for f in folds:
        if f == "all":
            raise ValueError(f"`{what}` names the fold \"all\" (training on every case), which is not covered")
        if isinstance(f, bool) or not isinstance(f, (int, np.integer)) or f < 0:
            raise ValueError(f"`{what}` holds {f!r}, which is no fold number")
        out.append(int(f))
    if not out:
        raise ValueError(f"`{what}` names no fold")
    if len(set(out)) != len(out):
        raise ValueError(f"`{what}` names a fold twice: {tuple(out)}")
    return tuple(out)


def read_fold_ensemble(model_dir: str, folds=None, checkpoint_name: str = "checkpoint_best.pth"):
    """`load_fold_ensemble` without the networks: (folds, spec, [cleaned state dict per fold], mirror axes).  Nothing here touches the device."""
    if folds is None:
        folds = available_folds(model_dir, checkpoint_name)
        if not folds:
            raise ValueError(f"no fold_<n>/{checkpoint_name} in {model_dir}")
    folds = check_folds(folds)
    from .tiling import ENSEMBLE_MAX_FOLDS
    if len(folds) > ENSEMBLE_MAX_FOLDS:
        raise ValueError(f"`use_folds` names {len(folds)} folds; one ensemble averages at most {ENSEMBLE_MAX_FOLDS}")
    plans, dataset_json = _read_model_jsons(model_dir)
    spec = axes = configuration = None
    sds = []
    for i, fold in enumerate(folds):
        path = os.path.join(model_dir, f"fold_{fold}", checkpoint_name)
        if not os.path.isfile(path):
            raise FileNotFoundError(f"fold {fold}: {path} does not exist")
        ckpt = _load_fold_checkpoint(model_dir, fold, checkpoint_name)
        name = ckpt["init_args"]["configuration"]
        if i == 0:   # the first fold decides configuration and mirroring (predict_from_raw_data.py:95-105)
            configuration, axes = name, ckpt.get("inference_allowed_mirroring_axes")
            spec = _checkpoint_spec(ckpt, plans, dataset_json)
        elif name != configuration:
            raise ValueError(f"fold {fold}: the checkpoint names the configuration {name!r}, fold {folds[0]} names {configuration!r}; one ensemble has one configuration")
        try:
            sds.append(_checked_state_dict(ckpt, spec))
        except (ValueError, RuntimeError) as e:
            raise type(e)(f"fold {fold}: {e}") from e
    return folds, spec, sds, axes


def load_fold_ensemble(model_dir: str, folds=None, checkpoint_name: str = "checkpoint_best.pth", device=None) -> FoldEnsemble:
    """initialize_from_trained_model_folder for several folds (predict_from_raw_data.py:78-121): `folds` None = every fold `available_folds` finds; one fold is
    allowed.  Every checkpoint is read and checked before the first network is built."""
    from .models import PlainConvUNet
    folds, spec, sds, axes = read_fold_ensemble(model_dir, folds, checkpoint_name)
    return FoldEnsemble([TrainedModel(PlainConvUNet(spec, sd, device=device), spec, axes) for sd in sds], folds)
