"""nnU-Net's plan-and-preprocess entry point for the tissue head's 2-D PNG datasets: what `plan_and_preprocess_entry()` (/root/reference/segmentor.py:207-215)
decides before `nnUNetTrainer` starts -- the dataset fingerprint, the plans and the cross-validation split -- as host logic over what the case kernels of
kernels_segprep.hip return.

    extract_fingerprint   DatasetFingerprintExtractor.analyze_case / run (fingerprint_extractor.py:41-194) for NaturalImage2DIO cases
    get_pool_and_conv_props, plan_experiment   network_topology.py:30-105, default_experiment_planner.py:156-500, the 2-D configuration
    crossval_splits       nnUNetTrainer.do_split (:537-546)
    conv_feature_map_size the one piece that lives in another package (see its docstring: unpinned)

Everything but `extract_fingerprint` on device tensors is plain numpy.  tests/test_cpu_nnunet_plan.py pins each function to the reference's own code through
fixtures that scripts/gen_golden_planner.py records.
"""
from __future__ import annotations

from copy import deepcopy
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import nnunet

SPACING_2D = (999.0, 1.0, 1.0)           # NaturalImage2DIO.read_images: a PNG is one slice, [C, 1, H, W]
ANISO_THRESHOLD = 3                      # nnunetv2/configuration.py
NUM_FOREGROUND_VOXELS = 10e7             # DatasetFingerprintExtractor.num_foreground_voxels_for_intensitystats
# ExperimentPlanner.__init__ (:50-66)
UNET_BASE_NUM_FEATURES = 32
UNET_REFERENCE_VAL_2D = 85000000
UNET_REFERENCE_VAL_CORRESP_GB = 8
UNET_REFERENCE_VAL_CORRESP_BS_2D = 12
UNET_FEATUREMAP_MIN_EDGE_LENGTH = 4
UNET_BLOCKS_PER_STAGE = 2
UNET_MIN_BATCH_SIZE = 2
UNET_MAX_FEATURES_2D = 512
# default_normalization_schemes.py: leaves_pixels_outside_mask_at_zero_if_use_mask_for_norm_is_true
LEAVES_OUTSIDE_AT_ZERO = {"ZScoreNormalization": True, "CTNormalization": False, "NoNormalization": False, "RescaleTo01Normalization": False,
                          "RGBTo01Normalization": False}


# ---- fingerprint ------------------------------------------------------------------------------------------------------------------------------
def foreground_ranks(num_fg: int, n_channels: int, num_samples: int, seed: int = 1234) -> List[np.ndarray]:
    """The draws of collect_foreground_intensities (:53-69) as ranks into the case's foreground pixels in row-major order: ONE RandomState(seed) walked
    through the channels; `rs.choice(foreground_pixels, n, replace=True)` consumes the stream as `rs.randint(0, num_fg, n)` does and returns
    foreground_pixels[those].  A case without foreground draws nothing (its lists stay empty)."""
    rs = np.random.RandomState(seed)
    if num_fg <= 0:
        return [np.zeros(0, np.int64) for _ in range(n_channels)]
    return [rs.randint(0, num_fg, num_samples).astype(np.int64) for _ in range(n_channels)]


def _case_on_host(img: torch.Tensor, seg: torch.Tensor, num_samples: int):
    """analyze_case for a case in host memory: numpy indexing where the device path launches kernels."""
    box = nnunet.nonzero_bbox(img)
    data = np.asarray(img[:, box[0]:box[1], box[2]:box[3]])
    fg = np.asarray(seg[box[0]:box[1], box[2]:box[3]]) > 0
    ranks = foreground_ranks(int(fg.sum()), data.shape[0], num_samples)
    return box, [data[c][fg][ranks[c]] for c in range(data.shape[0])]


def _case_on_device(img: torch.Tensor, seg: torch.Tensor, num_samples: int):
    from . import nnunet_data as nd
    box = nd.case_bbox(img)
    _, prefix, totals = nd.case_counts(seg, box, 32)      # only `label > 0` matters here: every label below 32 is a class of its own
    num_fg = int(totals[32])
    ranks = foreground_ranks(num_fg, int(img.shape[0]), num_samples)
    out = []
    for c in range(int(img.shape[0])):
        if ranks[c].size == 0:
            out.append(np.zeros(0, np.asarray(torch.empty(0, dtype=img.dtype)).dtype))
            continue
        _, values = nd.case_rank_to_coord(seg, box, -1, prefix[32], torch.from_numpy(ranks[c]).to(img.device), image=img)
        out.append(values[:, c].cpu().numpy())
    return box, out


def extract_fingerprint(cases, dataset_json: dict, num_foreground_voxels: float = NUM_FOREGROUND_VOXELS) -> dict:
    """DatasetFingerprintExtractor.run for 2-D natural images.  `cases`: pairs (image [C, H, W] uint8 or float32, label map [H, W] uint8), on the
    device (the box, the foreground count and the sampled intensities then come from the case kernels) or on the host.  Per case: crop to non-zero,
    `shapes_after_crop` [1, h, w], `spacings` (999, 1, 1), the relative size after cropping, and per channel `int(num_foreground_voxels // n_cases)`
    foreground intensities drawn as `foreground_ranks` states.  The seven statistics per channel are numpy's over the concatenated samples (:168-177).
    Returns the dictionary `dataset_fingerprint.json` holds."""
    cases = list(cases)
    if not cases:
        raise ValueError("extract_fingerprint: no cases")
    channels = dataset_json["channel_names"] if "channel_names" in dataset_json else dataset_json["modality"]
    num_samples = int(num_foreground_voxels // len(cases))
    shapes, spacings, rel, samples = [], [], [], [[] for _ in channels]
    for i, (img, seg) in enumerate(cases):
        img, seg = torch.as_tensor(img), torch.as_tensor(seg)
        if img.dim() != 3 or img.shape[0] != len(channels) or tuple(seg.shape) != tuple(img.shape[1:]):
            raise ValueError(f"extract_fingerprint: case {i}: image {tuple(img.shape)} / labels {tuple(seg.shape)} do not fit {len(channels)} channels")
        box, per_channel = (_case_on_device if img.is_cuda else _case_on_host)(img, seg, num_samples)
        h, w = box[1] - box[0], box[3] - box[2]
        shapes.append([1, h, w])
        spacings.append(list(SPACING_2D))
        rel.append(float(np.prod((1, h, w)) / np.prod((1, int(img.shape[1]), int(img.shape[2])))))
        for c, v in enumerate(per_channel):
            samples[c].append(np.asarray(v, dtype=np.float32))   # NaturalImage2DIO hands float32 on
    props = {}
    for c in range(len(channels)):
        v = np.concatenate(samples[c])
        if v.size == 0:
            raise ValueError("extract_fingerprint: no case has a foreground pixel (the reference's np.min of an empty array raises here too)")
        props[str(c)] = {"mean": float(np.mean(v)), "median": float(np.median(v)), "std": float(np.std(v)), "min": float(np.min(v)), "max": float(np.max(v)),
                         "percentile_99_5": float(np.percentile(v, 99.5)), "percentile_00_5": float(np.percentile(v, 0.5))}
    return {"spacings": spacings, "shapes_after_crop": shapes, "foreground_intensity_properties_per_channel": props,
            "median_relative_size_after_cropping": float(np.median(rel, 0))}


# ---- topology ---------------------------------------------------------------------------------------------------------------------------------
def get_pool_and_conv_props(spacing: Sequence[float], patch_size: Sequence[int], min_feature_map_size: int, max_numpool: int):
    """network_topology.get_pool_and_conv_props (:30-105): pool every axis that is still at least 2 * min_feature_map_size long, within a factor 2 of
    the finest remaining spacing and below max_numpool, until none is left (a single remaining axis needs 3 * min_feature_map_size); an axis' conv
    kernel turns 3 once its spacing is within a factor 2 of the finest and stays 3; the patch is padded up to a multiple of 2^pools per axis.
    Returns (num_pool_per_axis, pool_op_kernel_sizes, conv_kernel_sizes, patch_size, must_be_divisible_by)."""
    dim = len(spacing)
    cur_spacing, cur_size = [float(s) for s in spacing], list(patch_size)
    pools, convs = [[1] * dim], []
    num_pool, kernel = [0] * dim, [1] * dim
    while True:
        valid = [i for i in range(dim) if cur_size[i] >= 2 * min_feature_map_size]
        if not valid:
            break
        finest = min(cur_spacing[i] for i in valid)
        valid = [i for i in valid if cur_spacing[i] / finest < 2 and num_pool[i] < max_numpool]
        if not valid or (len(valid) == 1 and cur_size[valid[0]] < 3 * min_feature_map_size):
            break
        for d in range(dim):
            if kernel[d] != 3 and cur_spacing[d] / min(cur_spacing) < 2:
                kernel[d] = 3
        step = [1] * dim
        for v in valid:
            step[v] = 2
            num_pool[v] += 1
            cur_spacing[v] *= 2
            cur_size[v] = np.ceil(cur_size[v] / 2)
        pools.append(step)
        convs.append(list(kernel))
    div = 2 ** np.array(num_pool)
    padded = np.array([int(p) if p % d == 0 else int(p + d - p % d) for p, d in zip(patch_size, div)]).astype(int)
    convs.append([3] * dim)
    return num_pool, pools, convs, padded, div


def conv_feature_map_size(patch_size: Sequence[int], n_stages: int, strides: Sequence[Sequence[int]], num_input_channels: int,
                          features_per_stage: Sequence[int], blocks_per_stage_encoder: Sequence[int], blocks_per_stage_decoder: Sequence[int],
                          num_labels: int) -> int:
    """`PlainConvUNet(...).compute_conv_feature_map_size(patch_size)` -- the figure ExperimentPlanner.static_estimate_VRAM_usage (:86-112) compares
    with its reference value.  The method belongs to the package `dynamic_network_architectures`, which the test-suite cannot import: it is restated
    here from knowledge of that package and is UNPINNED; everything around it is pinned with this function in its place.
    As restated: the number of conv output elements of one forward pass without deep supervision -- per encoder stage its convs' outputs at the
    stage's resolution (the stride sits in the first conv); per decoder stage the transposed conv's output and the stage's convs at the skip's
    resolution; the segmentation head at full resolution.  The input channels do not enter."""
    size = [int(p) for p in patch_size]
    skip_sizes, total = [], 0
    for s in range(n_stages):
        size = [a // int(b) for a, b in zip(size, strides[s])]
        skip_sizes.append(size)
        total += int(blocks_per_stage_encoder[s]) * int(features_per_stage[s]) * int(np.prod(size, dtype=np.int64))
    for j in range(n_stages - 1):                      # decoder stage j works at the resolution of encoder stage n - 2 - j
        s = n_stages - 2 - j
        px = int(np.prod(skip_sizes[s], dtype=np.int64))
        total += int(blocks_per_stage_decoder[j]) * int(features_per_stage[s]) * px    # the stage's convs
        total += int(features_per_stage[s]) * px                                       # the transposed conv
        if j == n_stages - 2:
            total += int(num_labels) * px                                              # the one head that is on
    return int(total)


# ---- planner ----------------------------------------------------------------------------------------------------------------------------------
def _normalization(dataset_json: dict, fingerprint: dict) -> Tuple[List[str], List[bool]]:
    """determine_normalization_scheme_and_whether_mask_is_used_for_norm (:199-214)."""
    channels = dataset_json["channel_names"] if "channel_names" in dataset_json else dataset_json["modality"]
    schemes = [nnunet.CHANNEL_NAME_TO_NORMALIZATION.get(m, "ZScoreNormalization") for m in channels.values()]
    if fingerprint["median_relative_size_after_cropping"] < (3 / 4.0):
        return schemes, [LEAVES_OUTSIDE_AT_ZERO[s] for s in schemes]
    return schemes, [False] * len(schemes)


def fullres_target_spacing(fingerprint: dict) -> np.ndarray:
    """determine_fullres_target_spacing (:156-197): the median spacing; where one axis is both much coarser (factor 3) and much shorter than the
    others, its 10th percentile instead, kept above the others' spacing."""
    spacings, sizes = np.vstack(fingerprint["spacings"]), np.vstack(fingerprint["shapes_after_crop"])
    target, target_size = np.percentile(spacings, 50, 0), np.percentile(sizes, 50, 0)
    worst = int(np.argmax(target))
    others = [i for i in range(len(target)) if i != worst]
    if target[worst] > ANISO_THRESHOLD * max(target[i] for i in others) and target_size[worst] * ANISO_THRESHOLD < min(target_size[i] for i in others):
        t = np.percentile(spacings[:, worst], 10)
        if t < max(target[i] for i in others):
            t = max(max(target[i] for i in others), t) + 1e-5
        target[worst] = t
    return target


def plan_2d(spacing, median_shape, n_cases_voxels: float, dataset_json: dict, fingerprint: dict, gpu_memory_target_in_gb: float = 8) -> dict:
    """get_plans_for_configuration (:229-369) for two axes: the initial patch (the aspect of 1 / spacing at 2048^2 pixels, clipped to the median shape),
    the reduction loop (shave the axis that is largest relative to the median shape by its divisibility step until the estimate fits), the batch size
    (the headroom against 12 patches, at most 5 % of the dataset's pixels, at least 2)."""
    spacing = np.asarray(spacing, dtype=np.float64)
    median_shape = np.asarray(median_shape)
    if len(spacing) != 2:
        raise ValueError(f"plan_2d: two axes, got spacing {spacing}")
    if not all(s > 0 for s in spacing):
        raise ValueError(f"Spacing must be > 0! Spacing: {spacing}")
    channels = dataset_json["channel_names"] if "channel_names" in dataset_json else dataset_json["modality"]
    n_in, n_labels = len(channels), len(dataset_json["labels"])
    aspect = 1 / spacing
    initial = [round(i) for i in aspect * (2048 ** 2 / np.prod(aspect)) ** (1 / 2)]
    initial = np.array([min(i, j) for i, j in zip(initial, median_shape[:2])])

    def topology(patch):
        num_pool, pools, convs, patch, div = get_pool_and_conv_props(spacing, patch, UNET_FEATUREMAP_MIN_EDGE_LENGTH, 999999)
        n = len(pools)
        est = conv_feature_map_size(tuple(patch), n, tuple(tuple(p) for p in pools), n_in,
                                    tuple(min(UNET_MAX_FEATURES_2D, UNET_BASE_NUM_FEATURES * 2 ** i) for i in range(n)), (UNET_BLOCKS_PER_STAGE,) * n,
                                    (UNET_BLOCKS_PER_STAGE,) * (n - 1), n_labels)
        return num_pool, pools, convs, patch, div, est

    num_pool, pools, convs, patch, div, estimate = topology(initial)
    reference = UNET_REFERENCE_VAL_2D * (gpu_memory_target_in_gb / UNET_REFERENCE_VAL_CORRESP_GB)
    while estimate > reference:
        axis = np.argsort(patch / median_shape[:2])[-1]
        tmp = deepcopy(patch)
        tmp[axis] -= div[axis]
        div = get_pool_and_conv_props(spacing, tmp, UNET_FEATUREMAP_MIN_EDGE_LENGTH, 999999)[4]   # the step once the axis is shorter (:292-304)
        patch[axis] -= div[axis]
        num_pool, pools, convs, patch, div, estimate = topology(patch)
    batch_size = round((reference / estimate) * UNET_REFERENCE_VAL_CORRESP_BS_2D)
    cap = round(n_cases_voxels * 0.05 / np.prod(patch, dtype=np.float64))
    batch_size = max(min(batch_size, cap), UNET_MIN_BATCH_SIZE)
    schemes, use_mask = _normalization(dataset_json, fingerprint)
    n = len(pools)
    resampling = {"order_z": 0, "force_separate_z": None}
    return {
        "data_identifier": "nnUNetPlans_2d",
        "preprocessor_name": "DefaultPreprocessor",
        "batch_size": int(batch_size),
        "patch_size": [int(v) for v in patch],
        "median_image_size_in_voxels": [float(v) for v in median_shape],
        "spacing": [float(v) for v in spacing],
        "normalization_schemes": schemes,
        "use_mask_for_norm": use_mask,
        "UNet_class_name": "PlainConvUNet",
        "UNet_base_num_features": UNET_BASE_NUM_FEATURES,
        "n_conv_per_stage_encoder": [UNET_BLOCKS_PER_STAGE] * n,
        "n_conv_per_stage_decoder": [UNET_BLOCKS_PER_STAGE] * (n - 1),
        "num_pool_per_axis": [int(v) for v in num_pool],
        "pool_op_kernel_sizes": [[int(v) for v in p] for p in pools],
        "conv_kernel_sizes": [[int(v) for v in k] for k in convs],
        "unet_max_num_features": UNET_MAX_FEATURES_2D,
        "resampling_fn_data": "resample_data_or_seg_to_shape",
        "resampling_fn_seg": "resample_data_or_seg_to_shape",
        "resampling_fn_data_kwargs": {"is_seg": False, "order": 3, **resampling},
        "resampling_fn_seg_kwargs": {"is_seg": True, "order": 1, **resampling},
        "resampling_fn_probabilities": "resample_data_or_seg_to_shape",
        "resampling_fn_probabilities_kwargs": {"is_seg": False, "order": 1, **resampling},
    }


def plan_experiment(fingerprint: dict, dataset_json: dict, dataset_name: str, gpu_memory_target_in_gb: float = 8) -> dict:
    """ExperimentPlanner.plan_experiment (:371-500) for a dataset of 2-D images: the `nnUNetPlans.json` dictionary with the reference's keys in the
    reference's order, values as `recursive_fix_for_json_export` leaves them (what a `json.load` of the reference's file returns, tuples aside).  A
    dataset whose median shape has more than one slice is refused: the 3-D configurations are not planned."""
    target = fullres_target_spacing(fingerprint)
    forward = [int(np.argmax(target))] + [i for i in range(3) if i != int(np.argmax(target))]
    backward = [int(np.argwhere(np.array(forward) == i)[0][0]) for i in range(3)]
    new_shapes = [[int(round(i / j * k)) for i, j, k in zip(sp, target, sh)] for sp, sh in zip(fingerprint["spacings"], fingerprint["shapes_after_crop"])]
    median_shape = np.median(new_shapes, 0)[forward]
    if median_shape[0] != 1:
        nnunet._refuse("shapes_after_crop", f"has a median of {median_shape[0]:g} slices: a 3-D dataset")
    n_voxels = float(np.prod(median_shape, dtype=np.float64) * dataset_json["numTraining"])
    plan = plan_2d(target[forward][1:], median_shape[1:], n_voxels, dataset_json, fingerprint, gpu_memory_target_in_gb)
    plan["batch_dice"] = True
    props = fingerprint["foreground_intensity_properties_per_channel"]
    return {
        "dataset_name": dataset_name,
        "plans_name": "nnUNetPlans",
        "original_median_spacing_after_transp": [float(i) for i in np.median(fingerprint["spacings"], 0)[forward]],
        "original_median_shape_after_transp": [int(round(i)) for i in np.median(fingerprint["shapes_after_crop"], 0)[forward]],
        "image_reader_writer": "NaturalImage2DIO",
        "transpose_forward": forward,
        "transpose_backward": backward,
        "configurations": {"2d": plan},
        "experiment_planner_used": "ExperimentPlanner",
        "label_manager": "LabelManager",
        "foreground_intensity_properties_per_channel": {str(k): dict(v) for k, v in props.items()},
    }


# ---- split ------------------------------------------------------------------------------------------------------------------------------------
def crossval_splits(keys: Sequence[str], n_splits: int = 5, seed: int = 12345) -> List[Dict[str, List[str]]]:
    """nnUNetTrainer.do_split (:537-546): `KFold(5, shuffle=True, random_state=12345)` over the sorted keys, restated without sklearn: the validation
    folds are contiguous chunks of `RandomState(seed).shuffle(arange(n))`, each sorted, n // 5 long with one more for the first n % 5; the training
    keys are the others, in order.  Fewer keys than folds: KFold's ValueError."""
    keys = np.sort(list(keys))
    n = len(keys)
    if n_splits > n:
        raise ValueError(f"Cannot have number of splits n_splits={n_splits} greater than the number of samples: n_samples={n}.")
    order = np.arange(n)
    np.random.RandomState(seed).shuffle(order)
    sizes = np.full(n_splits, n // n_splits, dtype=int)
    sizes[:n % n_splits] += 1
    splits, start = [], 0
    for size in sizes:
        val = np.zeros(n, bool)
        val[order[start:start + size]] = True
        splits.append({"train": [str(k) for k in keys[~val]], "val": [str(k) for k in keys[val]]})
        start += size
    return splits
