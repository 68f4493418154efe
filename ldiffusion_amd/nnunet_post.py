"""What nnU-Net v2 does after the last epoch of a fold: the final validation (`nnUNetTrainer.perform_actual_validation`, nnUNetTrainer.py:1119-1246), its
scores (evaluation/evaluate_predictions.py) and the largest-component postprocessing fitted on them (postprocessing/remove_connected_components.py).

On the device: the prediction (`TrainedModel.predict_mask`), the confusion counts (`metrics.confusion_matrix`) and the connected components
(`ldiff_op_keep_largest_component`, csrc/kernels_segpost.hip).  On the host: a few integers per case and the JSON files.

Pinned by tests/golden/reference_eval_metrics.json (scripts/gen_golden_eval_metrics.py runs the reference's `compute_metrics`): `case_metrics`.
RESTATED, because the reference's own code cannot run in the test-suite: `summarize` (`compute_metrics_on_folder` needs a spawn pool), the greedy rule of
`determine_postprocessing` (a spawn pool, and `acvl_utils`, which is not installed), and the component rule itself -- `acvl_utils`'
`remove_all_but_largest_component` restated as `skimage.measure.label(mask, connectivity=None)` followed by the arg-max of the sizes, with ties going
to the component whose first pixel in raster order comes first (UNPINNED).

The record of a fitted postprocessing is `postprocessing.json` in the reference's layout (input_folder, postprocessed, postprocessing_fns,
postprocessing_kwargs).  `postprocessing.pkl` is NOT written: it pickles a function of the package `nnunetv2`, which is not installed here, so
nothing could load it; `load_postprocessing` reads the JSON instead.

    python -m ldiffusion_amd.nnunet_post determine -i PRED_DIR -ref LABEL_DIR -m MODEL_DIR
    python -m ldiffusion_amd.nnunet_post apply -i IN_DIR -o OUT_DIR -pp_json PRED_DIR/postprocessing.json
    python -m ldiffusion_amd.nnunet_post accumulate -m MODEL_DIR -f 0 1 2 3 4 -ref LABEL_DIR
"""
from __future__ import annotations

import json
import os
import warnings
from copy import deepcopy
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib

LabelOrRegion = Union[int, Tuple[int, ...]]
KEEP_LARGEST = "remove_all_but_largest_component_from_segmentation"   # the one function the reference fits (remove_connected_components.py:22)
METRIC_NAMES = ("Dice", "IoU", "FP", "TP", "FN", "TN", "n_pred", "n_ref")   # compute_metrics' insertion order (evaluate_predictions.py:108-119)
FILE_ENDING = ".png"
_OTHER_MAX = 31   # metrics.MAX_CLASSES - 1: the distinct label values one call scores, plus one class for every other value


# ---- labels and regions -------------------------------------------------------------------------------------------------------------------------------
def _values(label_or_region) -> Tuple[int, ...]:
    """region_or_label_to_mask's reading (evaluate_predictions.py:67-74): a scalar is one value, anything else a collection of values."""
    if isinstance(label_or_region, (int, np.integer)) and not isinstance(label_or_region, bool):
        return (int(label_or_region),)
    if isinstance(label_or_region, (tuple, list)):
        return tuple(int(v) for v in label_or_region)
    raise ValueError(f"a label is an integer and a region a tuple of integers, got {label_or_region!r}")


def _as_list(labels_or_regions) -> list:
    """remove_all_but_largest_component_from_segmentation's reading (:27-28): anything but a list is ONE label or region."""
    return list(labels_or_regions) if isinstance(labels_or_regions, list) else [labels_or_regions]


def _key(label_or_region):
    return tuple(label_or_region) if isinstance(label_or_region, (tuple, list)) else int(label_or_region)


def membership_table(labels_or_regions) -> torch.Tensor:
    """The 256-byte table of `ldiff_op_keep_largest_component` (host tensor): byte v = 1 when v is in the label, the list of labels or the region."""
    table = torch.zeros(256, dtype=torch.uint8)
    for entry in _as_list(labels_or_regions):
        for v in _values(entry):
            if not 0 <= v <= 255:
                raise ValueError(f"labels_or_regions: the value {v} does not fit a uint8 label map")
            table[v] = 1
    return table


def label_lists(dataset_json: dict):
    """(labels_or_regions, foreground_labels, ignore_label) as determine_postprocessing and perform_actual_validation take them from the LabelManager
    (remove_connected_components.py:93-94, nnUNetTrainer.py:1232-1235): the foreground regions in dataset.json order where the labels define regions,
    else the foreground labels; the foreground labels are all label values but 0, sorted, the ignore label left out."""
    from . import nnunet
    labels = dataset_json["labels"]
    if nnunet.has_regions(labels):
        spec = nnunet.region_spec(labels, dataset_json.get("regions_class_order"))
        foreground = [v for v in spec["all_labels"] if v != 0]
        return list(spec["foreground_regions"]), foreground, spec["ignore_label"]
    _, ignore = nnunet.label_spec(labels)
    values = sorted({int(v[0]) if isinstance(v, (list, tuple)) else int(v) for name, v in labels.items() if name != "ignore"})
    foreground = [v for v in values if v != 0]
    return list(foreground), foreground, ignore


# ---- the kernel's two entries -------------------------------------------------------------------------------------------------------------------------
def _seg3(seg: torch.Tensor, what: str) -> torch.Tensor:
    _lib.require_gpu()
    if not isinstance(seg, torch.Tensor) or not seg.is_cuda or seg.dtype != torch.uint8 or seg.dim() not in (2, 3):
        raise ValueError(f"{what}: `seg` must be a uint8 device tensor [H, W] or [N, H, W]")
    return (seg[None] if seg.dim() == 2 else seg).contiguous()


def _workspace(N, H, W, device):
    nbytes = _lib.load().ldiff_op_keep_largest_component_ws_bytes(N, H, W)
    return torch.empty(max(nbytes, 8), dtype=torch.uint8, device=device), nbytes


def keep_largest_component(seg: torch.Tensor, labels_or_regions, background_label: int = 0, out: torch.Tensor = None) -> torch.Tensor:
    """remove_all_but_largest_component_from_segmentation (remove_connected_components.py:22-34) on uint8 device label maps [H, W] or [N, H, W], each
    image on its own: the pixels of `labels_or_regions` (an int, a tuple = one region, or a list of either) form one mask; of its 8-connected components
    the largest stays (ties: the module docstring), every other member pixel becomes `background_label`.  Returns a new tensor (or `out`, which must
    not be `seg`: the input is never modified)."""
    s = _seg3(seg, "keep_largest_component")
    N, H, W = s.shape
    if out is None:
        o = torch.empty_like(s)
    else:
        if out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or out.numel() != s.numel() or out.device != s.device:
            raise ValueError("keep_largest_component: `out` must be a contiguous uint8 tensor of seg's shape on seg's device")
        o = out
    table = membership_table(labels_or_regions).to(s.device)
    with torch.cuda.device(s.device):
        ws, nbytes = _workspace(N, H, W, s.device)
        _lib.check(_lib.load().ldiff_op_keep_largest_component(_lib.ptr(s), _lib.ptr(o), N, H, W, _lib.ptr(table), int(background_label), _lib.ptr(ws), nbytes,
                                                               _lib.stream_ptr()))
    return o if out is not None else o.view(seg.shape)


def cc_label(seg: torch.Tensor, labels_or_regions):
    """ldiff_op_cc_label: (labels, sizes), both int32 of seg's shape -- a member pixel's label is 1 + the smallest linear index y W + x of its 8-connected
    component, 0 outside the mask; `sizes` holds a component's pixel count at that smallest pixel and 0 everywhere else."""
    s = _seg3(seg, "cc_label")
    N, H, W = s.shape
    labels = torch.empty(s.shape, dtype=torch.int32, device=s.device)
    sizes = torch.empty(s.shape, dtype=torch.int32, device=s.device)
    table = membership_table(labels_or_regions).to(s.device)
    with torch.cuda.device(s.device):
        ws, nbytes = _workspace(N, H, W, s.device)
        _lib.check(_lib.load().ldiff_op_cc_label(_lib.ptr(s), N, H, W, _lib.ptr(table), _lib.ptr(labels), _lib.ptr(sizes), _lib.ptr(ws), nbytes, _lib.stream_ptr()))
    return labels.view(seg.shape), sizes.view(seg.shape)


def apply_postprocessing(seg: torch.Tensor, fns: Sequence[str], kwargs: Sequence[dict]) -> torch.Tensor:
    """remove_connected_components.apply_postprocessing (:37-40) with the functions by name, as postprocessing.json records them."""
    if len(fns) != len(kwargs):
        raise ValueError(f"apply_postprocessing: {len(fns)} functions for {len(kwargs)} keyword sets")
    for fn, kw in zip(fns, kwargs):
        if fn != KEEP_LARGEST:
            raise ValueError(f"apply_postprocessing: unknown postprocessing function {fn!r} (known: {KEEP_LARGEST})")
        seg = keep_largest_component(seg, **kw)
    return seg


# ---- scores -------------------------------------------------------------------------------------------------------------------------------------------
def metrics_from_confusion(conf: np.ndarray, index_of: Dict[int, int], labels_or_regions) -> dict:
    """compute_metrics' numbers (evaluate_predictions.py:103-119) from one confusion matrix (rows = reference, columns = prediction) whose class i stands
    for the label value v with index_of[v] = i; the last class collects every other value.  Region counts are sums of cells; TN is what is left of the
    counted pixels.  Python ints and floats."""
    conf = np.asarray(conf, dtype=np.int64)
    total = int(conf.sum())
    out = {}
    for r in labels_or_regions:
        idx = sorted({index_of[v] for v in _values(r)})
        row, col = int(conf[idx, :].sum()), int(conf[:, idx].sum())
        tp = int(conf[np.ix_(idx, idx)].sum())
        fp, fn = col - tp, row - tp
        m = {}
        if tp + fp + fn == 0:
            m["Dice"], m["IoU"] = float("nan"), float("nan")
        else:
            m["Dice"], m["IoU"] = 2 * tp / (2 * tp + fp + fn), tp / (tp + fp + fn)
        m.update(FP=fp, TP=tp, FN=fn, TN=total - tp - fp - fn, n_pred=fp + tp, n_ref=fn + tp)
        out[_key(r)] = m
    return out


def _luts(labels_or_regions, ignore_label):
    values = sorted({v for r in labels_or_regions for v in _values(r)})
    if len(values) > _OTHER_MAX:
        raise ValueError(f"case_metrics: {len(values)} distinct label values; one call scores at most {_OTHER_MAX}")
    if any(not 0 <= v <= 255 for v in values):
        raise ValueError(f"case_metrics: label values outside 0 .. 255: {values}")
    index_of = {v: i for i, v in enumerate(values)}
    pred = torch.full((256,), len(values), dtype=torch.uint8)
    for v, i in index_of.items():
        pred[v] = i
    ref = pred.clone()
    if ignore_label is not None:
        if not 0 <= int(ignore_label) <= 255:
            raise ValueError(f"case_metrics: ignore_label = {ignore_label} does not fit a uint8 label map")
        ref[int(ignore_label)] = 255   # no class: the confusion kernel drops the pixel
    return index_of, pred, ref, len(values) + 1


def case_metrics(ref: torch.Tensor, pred: torch.Tensor, labels_or_regions, ignore_label: Optional[int] = None) -> dict:
    """evaluate_predictions.compute_metrics (:89-120) for one case on uint8 device masks [H, W]: {label or region: {Dice, IoU, FP, TP, FN, TN, n_pred,
    n_ref}}.  One `metrics.confusion_matrix` launch over the values the labels and regions name plus one class for every other value; a reference pixel
    that carries `ignore_label` enters no cell.  Dice and IoU are nan where tp + fp + fn == 0."""
    from . import metrics
    labels_or_regions = list(labels_or_regions)
    index_of, pl, rl, n = _luts(labels_or_regions, ignore_label)
    if ref.shape != pred.shape or ref.dim() != 2:
        raise ValueError(f"case_metrics: reference {tuple(ref.shape)} and prediction {tuple(pred.shape)} must be two [H, W] masks of one size")
    conf = metrics.confusion_matrix(pred, ref.to(pred.device), n, pred_lut=pl, target_lut=rl)
    return metrics_from_confusion(conf[0].cpu().numpy(), index_of, labels_or_regions)


def summarize(per_case: List[dict]) -> dict:
    """compute_metrics_on_folder's aggregation (evaluate_predictions.py:151-172), RESTATED (the function itself needs a spawn pool): `mean` = np.nanmean over
    the cases per label or region and metric, the counts included; `foreground_mean` = the plain mean of those means over every key but 0 (so one
    all-nan class makes it nan).  `per_case`: [{"metrics": {...}, ...}] as `case_metrics` gives them, optionally with reference_file / prediction_file."""
    if not per_case:
        raise ValueError("summarize: no cases")
    keys = list(per_case[0]["metrics"].keys())
    names = list(per_case[0]["metrics"][keys[0]].keys())
    means = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # "Mean of empty slice": a class absent from every case is nan, as in the reference
        for k in keys:
            means[k] = {m: float(np.nanmean([c["metrics"][k][m] for c in per_case])) for m in names}
        foreground = {m: float(np.mean([means[k][m] for k in keys if k != 0 and k != "0"])) for m in names}
    return {"metric_per_case": deepcopy(per_case), "mean": means, "foreground_mean": foreground}


def label_or_region_to_key(label_or_region) -> str:
    return str(label_or_region)


def key_to_label_or_region(key: str):
    """evaluate_predictions.key_to_label_or_region (:24-31)."""
    try:
        return int(key)
    except ValueError:
        return tuple(int(i) for i in key.replace("(", "").replace(")", "").split(",") if len(i.strip()) > 0)


def save_summary_json(results: dict, output_file: str) -> None:
    """evaluate_predictions.save_summary_json (:34-48): keys are str(label_or_region), sort_keys=True, indent 4 (batchgenerators' save_json)."""
    out = deepcopy(results)
    out["mean"] = {label_or_region_to_key(k): v for k, v in results["mean"].items()}
    for i, case in enumerate(results["metric_per_case"]):
        out["metric_per_case"][i]["metrics"] = {label_or_region_to_key(k): v for k, v in case["metrics"].items()}
    with open(output_file, "w") as f:
        json.dump(out, f, sort_keys=True, indent=4)


def load_summary_json(filename: str) -> dict:
    """evaluate_predictions.load_summary_json (:51-60)."""
    with open(filename) as f:
        results = json.load(f)
    results["mean"] = {key_to_label_or_region(k): v for k, v in results["mean"].items()}
    for case in results["metric_per_case"]:
        case["metrics"] = {key_to_label_or_region(k): v for k, v in case["metrics"].items()}
    return results


def _summary_of(preds, refs, labels_or_regions, ignore_label, names=None) -> dict:
    cases = []
    for i, (p, r) in enumerate(zip(preds, refs)):
        case = {"metrics": case_metrics(r, p, labels_or_regions, ignore_label)}
        if names is not None:
            case.update(reference_file=names[i][0], prediction_file=names[i][1])
        cases.append(case)
    return summarize(cases)


# ---- the greedy rule ----------------------------------------------------------------------------------------------------------------------------------
def greedy_decisions(baseline: dict, labels_or_regions, foreground_labels, trial):
    """determine_postprocessing's decisions (remove_connected_components.py:114-220), RESTATED (the function needs a spawn pool and acvl_utils), on
    whatever `trial(kwargs) -> summary` scores -- `trial` applies remove-all-but-largest with `kwargs` ON TOP of everything accepted so far, and
    `accept()` on the returned object makes that state the new source.
      1. the whole foreground (`labels_or_regions=foreground_labels`, a list: one mask) is kept only if foreground_mean Dice rises AND no entry's mean
         Dice falls;
      2. with more than one entry, each label or region in order, on top of what is kept: kept where THAT entry's mean Dice rises.
    Comparisons are the reference's `>` / `<` on floats, so a nan never wins and never vetoes.  Returns (fns, kwargs, final summary)."""
    fns, kwargs, current = [], [], baseline
    kw = {"labels_or_regions": list(foreground_labels)}
    cand, accept = trial(kw)
    do_this = cand["foreground_mean"]["Dice"] > current["foreground_mean"]["Dice"]
    if do_this:
        for k in cand["mean"]:
            if cand["mean"][k]["Dice"] < current["mean"][k]["Dice"]:
                do_this = False
                break
    if do_this:
        accept()
        fns.append(KEEP_LARGEST)
        kwargs.append(kw)
        current = cand
    if len(labels_or_regions) > 1:
        for r in labels_or_regions:
            kw = {"labels_or_regions": r}
            cand, accept = trial(kw)
            if cand["mean"][_key(r)]["Dice"] > current["mean"][_key(r)]["Dice"]:
                accept()
                fns.append(KEEP_LARGEST)
                kwargs.append(kw)
                current = cand
    return fns, kwargs, current


def determine_postprocessing(preds: Sequence[torch.Tensor], refs: Sequence[torch.Tensor], labels_or_regions, foreground_labels, ignore_label=None, names=None):
    """The reference's greedy fit (`greedy_decisions`) on device-resident masks: `preds`, `refs` = uint8 [H, W] tensors per case.  Every trial is one
    `keep_largest_component` launch sequence and one confusion launch per case; nothing is written.
    Returns ((fns, kwargs), baseline summary, postprocessed summary, postprocessed masks)."""
    labels_or_regions = [_key(r) for r in labels_or_regions]
    state = {"masks": list(preds)}
    baseline = _summary_of(state["masks"], refs, labels_or_regions, ignore_label, names)

    def trial(kw):
        masks = [keep_largest_component(m, **kw) for m in state["masks"]]
        return _summary_of(masks, refs, labels_or_regions, ignore_label, names), lambda: state.update(masks=masks)

    fns, kwargs, final = greedy_decisions(baseline, labels_or_regions, foreground_labels, trial)
    return (fns, kwargs), baseline, final, state["masks"]


def _jsonable(obj):
    """recursive_fix_for_json_export's effect on what this module builds: tuples become lists, numpy scalars python ones."""
    if isinstance(obj, dict):
        return {k: _jsonable(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [_jsonable(v) for v in obj]
    if isinstance(obj, np.generic):
        return obj.item()
    return obj


def save_postprocessing_json(path: str, fns, kwargs, baseline: dict, final: dict) -> None:
    """postprocessing.json as remove_connected_components.py:226-239 writes it (save_json's default: sort_keys=True, indent 4)."""
    record = {"input_folder": {"foreground_mean": baseline["foreground_mean"], "mean": {label_or_region_to_key(k): v for k, v in baseline["mean"].items()}},
              "postprocessed": {"foreground_mean": final["foreground_mean"], "mean": {label_or_region_to_key(k): v for k, v in final["mean"].items()}},
              "postprocessing_fns": list(fns), "postprocessing_kwargs": _jsonable(list(kwargs))}
    with open(path, "w") as f:
        json.dump(record, f, sort_keys=True, indent=4)


def _region_from_json(entry):
    return tuple(int(v) for v in entry) if isinstance(entry, list) else int(entry)


def load_postprocessing(path: str):
    """(fns, kwargs) of a postprocessing.json.  JSON has no tuples, so a region comes back as a flat list of integers -- which the filter reads as a
    list of labels: the same mask, the union of the values, either way.  Lists inside a list become tuples again."""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"no postprocessing record at {path} (train with postprocessing=True, or run `python -m ldiffusion_amd.nnunet_post determine`)")
    with open(path) as f:
        record = json.load(f)
    fns, kwargs = list(record["postprocessing_fns"]), []
    for kw in record["postprocessing_kwargs"]:
        lr = kw["labels_or_regions"]
        if isinstance(lr, list):
            lr = [_region_from_json(v) for v in lr]
        kwargs.append(dict(kw, labels_or_regions=lr))
    return fns, kwargs


# ---- folders ------------------------------------------------------------------------------------------------------------------------------------------
def _read_mask(path: str, device) -> torch.Tensor:
    from PIL import Image
    with Image.open(path) as im:
        return torch.from_numpy(np.array(im.convert("L"), np.uint8)).to(device)


def _write_masks(masks: Dict[str, torch.Tensor], folder: str, io_workers: int = 4) -> None:
    """<key>.png per mask through `utils.copy_or_convert_images`' writer threads' task (`utils._save_rgb`); a worker's exception is re-raised here."""
    from concurrent.futures import ThreadPoolExecutor
    from . import utils
    os.makedirs(folder, exist_ok=True)
    if isinstance(io_workers, bool) or not isinstance(io_workers, (int, np.integer)) or not 0 <= io_workers <= utils.MAX_IO_WORKERS:
        raise ValueError(f"io_workers = {io_workers!r}: an integer in 0 .. {utils.MAX_IO_WORKERS}")
    pool = ThreadPoolExecutor(max_workers=int(io_workers), thread_name_prefix="ldiff-imgio") if io_workers else None
    try:
        pending = []
        for key, m in masks.items():
            host, dst = m.cpu().numpy(), os.path.join(folder, key + FILE_ENDING)
            pending.append(pool.submit(utils._save_rgb, host, dst) if pool is not None else utils._Inline(utils._save_rgb(host, dst)))
        for f in pending:
            f.result()
    finally:
        if pool is not None:
            pool.shutdown(wait=True, cancel_futures=True)


def determine_postprocessing_folder(pred_dir: str, ref_dir: str, model_dir: str, device="cuda:0", io_workers: int = 4):
    """remove_connected_components.determine_postprocessing on folders: every `*.png` of `pred_dir` against the file of the same name in `ref_dir`,
    labels and regions from `<model_dir>/dataset.json`.  Writes `pred_dir/summary.json` where it is missing, `pred_dir/postprocessed/` (the masks and
    their summary.json) and `pred_dir/postprocessing.json`; returns (fns, kwargs)."""
    with open(os.path.join(model_dir, "dataset.json")) as f:
        labels_or_regions, foreground, ignore = label_lists(json.load(f))
    files = sorted(n for n in os.listdir(pred_dir) if n.endswith(FILE_ENDING))
    if not files:
        raise ValueError(f"determine_postprocessing_folder: no {FILE_ENDING} files in {pred_dir}")
    preds = [_read_mask(os.path.join(pred_dir, n), device) for n in files]
    refs = [_read_mask(os.path.join(ref_dir, n), device) for n in files]
    names = [(os.path.join(ref_dir, n), os.path.join(pred_dir, n)) for n in files]
    (fns, kwargs), baseline, final, masks = determine_postprocessing(preds, refs, labels_or_regions, foreground, ignore, names)
    if not os.path.isfile(os.path.join(pred_dir, "summary.json")):
        save_summary_json(baseline, os.path.join(pred_dir, "summary.json"))
    out_dir = os.path.join(pred_dir, "postprocessed")
    _write_masks({n[:-len(FILE_ENDING)]: m for n, m in zip(files, masks)}, out_dir, io_workers)
    for case, n in zip(final["metric_per_case"], files):
        case["prediction_file"] = os.path.join(out_dir, n)
    save_summary_json(final, os.path.join(out_dir, "summary.json"))
    save_postprocessing_json(os.path.join(pred_dir, "postprocessing.json"), fns, kwargs, baseline, final)
    return fns, kwargs


def apply_postprocessing_to_folder(in_dir: str, out_dir: str, postprocessing_json: str, device="cuda:0", io_workers: int = 4) -> None:
    """remove_connected_components.apply_postprocessing_to_folder with the record read from `postprocessing_json`."""
    fns, kwargs = load_postprocessing(postprocessing_json)
    files = sorted(n for n in os.listdir(in_dir) if n.endswith(FILE_ENDING))
    _write_masks({n[:-len(FILE_ENDING)]: apply_postprocessing(_read_mask(os.path.join(in_dir, n), device), fns, kwargs) for n in files}, out_dir, io_workers)


# ---- the final validation of a fold -------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def validate_fold(model_dir: str, cases: dict, val_keys: Sequence[str], *, checkpoint_name: str = "checkpoint_final.pth", batch_tiles=None, io_workers: int = 4,
                  device=None, fold: int = 0) -> dict:
    """nnUNetTrainer.perform_actual_validation (nnUNetTrainer.py:1119-1246) for one fold (`fold`, default 0) of a trained-model folder: every key of `val_keys` is predicted
    in full from its raw device image -- `cases[key]` = (uint8 [C, H, W], uint8 label map [H, W]), as the tissue stage holds them -- with
    `TrainedModel.predict_mask`: step 0.5, Gaussian weighting, the checkpoint's mirror axes, the predictor that function builds.  Writes
    `fold_<fold>/validation/<key>.png` and `fold_<fold>/validation/summary.json` (foreground regions for a region model, else foreground labels; the ignore label
    left out of every count) and returns the summary.  Under a process group of several ranks rank 0 validates and the others wait at a barrier (they
    return None)."""
    import torch.distributed as dist
    from . import nnunet
    world = dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1
    summary = None
    if world == 1 or dist.get_rank() == 0:
        with open(os.path.join(model_dir, "dataset.json")) as f:
            labels_or_regions, _, ignore = label_lists(json.load(f))
        if device is None:
            device = cases[val_keys[0]][0].device
        head = nnunet.load_trained_model_folder(model_dir, fold, checkpoint_name, device=device)
        out_dir = os.path.join(model_dir, f"fold_{fold}", "validation")
        masks = {}
        for key in val_keys:
            img = cases[key][0]
            masks[key] = head.predict_mask(img.to(device).float(), batch_tiles=batch_tiles)
        head.network.check_finite()   # before any file is written
        _write_masks(masks, out_dir, io_workers)
        per_case = [{"metrics": case_metrics(cases[k][1].to(device), masks[k], labels_or_regions, ignore), "reference_file": k + FILE_ENDING,
                     "prediction_file": os.path.join(out_dir, k + FILE_ENDING)} for k in val_keys]
        summary = summarize(per_case)
        save_summary_json(summary, os.path.join(out_dir, "summary.json"))
    if world > 1:
        dist.barrier()
    return summary


# ---- the folds of a cross-validation, scored together --------------------------------------------------------------------------------------------------
def crossval_folder(model_dir: str, folds) -> str:
    """`<model_dir>/crossval_results_folds_<f0>_<f1>...`: where find_best_configuration keeps the merged validation of `folds` (find_best_configuration.py,
    `folds_tuple_to_string`: the fold numbers in the given order, joined by `_`)."""
    return os.path.join(model_dir, "crossval_results_folds_" + "_".join(str(f) for f in folds))


def accumulate_cv_results(model_dir: str, folds, gt_dir: str, device="cuda:0", io_workers: int = 4) -> dict:
    """evaluation/accumulate_cv_results.py with overwrite=True: `crossval_folder(model_dir, folds)` is made anew and receives dataset.json, plans.json and every
    `fold_<f>/validation/*.png`; the merged folder is then scored again against the files of the same names in `gt_dir` (`case_metrics`, `summarize`: no fold's own
    summary.json is read) into its `summary.json`.  RuntimeError, in the reference's words, for a fold without `validation/` and for a case that more than one
    fold predicted.  `io_workers` stands where the reference has num_processes; the copies are made in line.  Returns the summary."""
    import shutil
    merged = crossval_folder(model_dir, folds)
    if os.path.isdir(merged):
        shutil.rmtree(merged)
    os.makedirs(merged)
    with open(os.path.join(model_dir, "dataset.json")) as f:
        labels_or_regions, _, ignore = label_lists(json.load(f))
    for name in ("dataset.json", "plans.json"):
        shutil.copy(os.path.join(model_dir, name), os.path.join(merged, name))
    for f in folds:
        val_dir = os.path.join(model_dir, f"fold_{f}", "validation")
        if not os.path.isdir(val_dir):
            raise RuntimeError(f"fold {f} of model {model_dir} is missing. Please train it!")
        for pf in sorted(n for n in os.listdir(val_dir) if n.endswith(FILE_ENDING) and os.path.isfile(os.path.join(val_dir, n))):
            if os.path.isfile(os.path.join(merged, pf)):
                raise RuntimeError(f"More than one of your folds has a prediction for case {pf}")
            shutil.copy(os.path.join(val_dir, pf), os.path.join(merged, pf))
    files = sorted(n for n in os.listdir(merged) if n.endswith(FILE_ENDING))
    if not files:
        raise ValueError(f"accumulate_cv_results: the folds {tuple(folds)} of {model_dir} hold no {FILE_ENDING} predictions")
    per_case = [{"metrics": case_metrics(_read_mask(os.path.join(gt_dir, n), device), _read_mask(os.path.join(merged, n), device), labels_or_regions, ignore),
                 "reference_file": os.path.join(gt_dir, n), "prediction_file": os.path.join(merged, n)} for n in files]
    summary = summarize(per_case)
    save_summary_json(summary, os.path.join(merged, "summary.json"))
    return summary


def main(argv=None):
    """The reference's two entry points (remove_connected_components.py:298-333), with the JSON record in the pickle's place, and accumulate_cv_results."""
    import argparse
    parser = argparse.ArgumentParser(prog="python -m ldiffusion_amd.nnunet_post")
    sub = parser.add_subparsers(dest="command", required=True)
    d = sub.add_parser("determine", help="writes postprocessing.json and postprocessed/ in the input folder")
    d.add_argument("-i", required=True, help="folder with predicted masks")
    d.add_argument("-ref", required=True, help="folder with ground-truth label maps")
    d.add_argument("-m", required=True, help="trained-model folder (its dataset.json names the labels)")
    a = sub.add_parser("apply", help="applies a postprocessing.json to a folder of masks")
    a.add_argument("-i", required=True, help="input folder")
    a.add_argument("-o", required=True, help="output folder")
    a.add_argument("-pp_json", required=True, help="postprocessing.json")
    c = sub.add_parser("accumulate", help="merges the folds' validation folders into crossval_results_folds_... and scores them again")
    c.add_argument("-m", required=True, help="trained-model folder")
    c.add_argument("-f", type=int, nargs="+", default=[0, 1, 2, 3, 4], help="folds")
    c.add_argument("-ref", required=True, help="folder with ground-truth label maps")
    for p in (d, a, c):
        p.add_argument("-np", type=int, default=4, help="writer threads")
        p.add_argument("--device", default="cuda:0")
    args = parser.parse_args(argv)
    if args.command == "accumulate":
        return accumulate_cv_results(args.m, tuple(args.f), args.ref, device=args.device, io_workers=args.np)
    if args.command == "determine":
        return determine_postprocessing_folder(args.i, args.ref, args.m, device=args.device, io_workers=args.np)
    return apply_postprocessing_to_folder(args.i, args.o, args.pp_json, device=args.device, io_workers=args.np)


if __name__ == "__main__":
    main()
