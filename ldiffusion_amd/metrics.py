"""Mask scoring on the device (include/ldiff.h "Metrics").

The reference scores masks with per-class masked sums and an `.item()` each (utils.py:55-104, evaluate.py:11-45, segmentor.py:114-142): C^2 host
synchronisations per image for the frequency-weighted IoU alone.  All four metrics are functions of one integer matrix, so here ONE launch
(`ldiff_confusion`) counts it where the masks or logits already are, one copy brings C^2 integers to the host, and `ldiff_seg_metrics` -- the same host
routine a C caller uses -- applies the reference's rules and arithmetic.  Matrices add: over batches (`out=`), images, and ranks
(`parallel.reduce_confusion`).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib

MAX_CLASSES = 32
# dataset.py:10-32
PIXEL_TO_LABEL = {0: 0, 100: 1, 150: 2, 50: 3, 200: 4, 250: 5, 255: 6}
PIXEL_TO_LABEL_CELL = {0: 0, 25: 1, 50: 2, 75: 3, 100: 4, 125: 5, 150: 6, 175: 7, 200: 8, 225: 9, 250: 10}


def label_lut(level: str) -> torch.Tensor:
    """The grey level -> class id table of `convert_labels` (dataset.py:48-63) as 256 uint8 entries; unlisted grey levels map to 0, as the
    reference's zero-initialised `label_img` leaves them.  Pass it (moved to the device once) as `target_lut` / `pred_lut`."""
    if level == "tissue":
        table = PIXEL_TO_LABEL
    elif level == "cell":
        table = PIXEL_TO_LABEL_CELL
    else:
        raise ValueError("Unsupported level. Use 'tissue' or 'cell'.")   # dataset.py:63
    lut = torch.zeros(256, dtype=torch.uint8)
    for grey, label in table.items():
        lut[grey] = label
    return lut


def _lut_on(lut, device) -> Optional[torch.Tensor]:
    if lut is None:
        return None
    lut = torch.as_tensor(lut)
    if lut.dtype != torch.uint8 or lut.numel() != 256:
        raise ValueError(f"a LUT is 256 uint8 entries, got {lut.numel()} of {lut.dtype}")
    return lut.to(device).contiguous()


def confusion_matrix(pred: torch.Tensor, target: torch.Tensor, num_classes: int, pred_lut=None, target_lut=None, out: torch.Tensor = None,
                     dropped: torch.Tensor = None) -> torch.Tensor:
    """Per-image confusion matrices int64 [B, C, C] on the device (rows = targets, columns = predictions), ADDED to `out` when given.

    pred: uint8 mask [B, H, W], or logits [B, C, H, W] float32 / float16 (`pred.dim() == 4`; arg-max in the kernel, `argmax_mask`'s rule).
    target: uint8 or integer labels [B, H, W] (int64 is read as it is; other integer types are widened first).
    dropped: int64 [B], += the pixels whose target or prediction is no class in [0, num_classes).  Nothing is synchronised."""
    _lib.require_gpu()
    if pred.dim() == 2:
        pred = pred[None]
    if target.dim() == 2:
        target = target[None]
    logits = pred.dim() == 4
    if pred.dim() not in (3, 4) or target.dim() != 3:
        raise ValueError(f"pred must be [B,H,W] or [B,C,H,W] and target [B,H,W], got {tuple(pred.shape)} and {tuple(target.shape)}")
    if not pred.is_cuda:
        raise ValueError("confusion_matrix takes device tensors")
    pred = pred.detach()
    if logits and pred.shape[1] != num_classes:
        # the reference's arg-max runs over whatever channels there are; classes beyond num_classes then match nothing
        from .pipeline import argmax_mask
        pred, logits = argmax_mask(pred), False
    if logits:
        if pred.dtype not in (torch.float32, torch.float16):
            raise ValueError(f"logits must be float32 or float16, got {pred.dtype}")
        kind = 1 if pred.dtype == torch.float32 else 2
    else:
        if pred.dtype != torch.uint8:
            raise ValueError(f"a mask prediction is uint8 (argmax_mask's output), got {pred.dtype}")
        kind = 0
    B, H, W = pred.shape[0], pred.shape[-2], pred.shape[-1]
    if tuple(target.shape) != (B, H, W):
        raise ValueError(f"target {tuple(target.shape)} does not match prediction {tuple(pred.shape)}")
    target = target.detach().to(pred.device)
    if target.dtype != torch.uint8:
        if target.is_floating_point() or target.dtype == torch.bool:
            raise ValueError(f"target must hold integer labels, got {target.dtype}")
        target = target.to(torch.int64)
    pred, target = pred.contiguous(), target.contiguous()
    pl, tl = _lut_on(pred_lut, pred.device), _lut_on(target_lut, pred.device)
    shape = (B, num_classes, num_classes)
    if out is None:
        out = torch.zeros(shape, dtype=torch.int64, device=pred.device) if 1 <= num_classes <= MAX_CLASSES else torch.zeros(0, dtype=torch.int64, device=pred.device)
    elif out.dtype != torch.int64 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != pred.device:
        raise ValueError(f"out must be a contiguous int64 {shape} tensor on {pred.device}")
    if dropped is not None and (dropped.dtype != torch.int64 or tuple(dropped.shape) != (B,) or not dropped.is_contiguous() or dropped.device != pred.device):
        raise ValueError(f"dropped must be a contiguous int64 [{B}] tensor on {pred.device}")
    with torch.cuda.device(pred.device):
        _lib.check(_lib.load().ldiff_confusion(_lib.ptr(pred), kind, _lib.ptr(target), 0 if target.dtype == torch.uint8 else 1, _lib.ptr(pl), _lib.ptr(tl),
                                               B, num_classes, H, W, _lib.ptr(out), _lib.ptr(dropped), _lib.stream_ptr()))
    return out


@dataclass
class SegMetrics:
    """The reference's four metrics of one confusion matrix, in the reference's number formats."""
    num_classes: int
    dice_per_class: np.ndarray               # float32 [C] (utils.py:55-82)
    dice: float                              # float32 mean over C
    iou_per_class: Dict[int, Optional[float]]  # None: empty union (utils.py:96-98)
    miou: float
    pa_per_class: List[float]                # evaluate.py:11-27
    pixel_accuracy: float
    fw_iou: float                            # evaluate.py:29-45
    fw_iou_fg: float                         # ignore_background=True


def from_confusion(conf) -> SegMetrics:
    """Metrics of ONE [C, C] matrix (tensor on any device, or array) through `ldiff_seg_metrics`.  A [B, C, C] stack is summed first: the
    reference flattens the whole batch together."""
    if isinstance(conf, torch.Tensor):
        conf = conf.detach().cpu().numpy()   # the one copy: C^2 (or B C^2) integers
    conf = np.asarray(conf)
    if conf.ndim == 3:
        conf = conf.sum(0)
    if conf.ndim != 2 or conf.shape[0] != conf.shape[1] or conf.dtype.kind not in "iu":
        raise ValueError(f"a confusion matrix is a square integer matrix, got {conf.shape} of {conf.dtype}")
    conf = np.ascontiguousarray(conf, dtype=np.int64)
    n = conf.shape[0]
    rec = _lib.SegMetricsOut()
    _lib.check(_lib.load().ldiff_seg_metrics(conf.ctypes.data_as(C.POINTER(C.c_int64)), n, C.byref(rec)))
    return SegMetrics(
        num_classes=n,
        dice_per_class=np.array(rec.dice[:n], np.float32),
        dice=float(rec.dice_mean),
        iou_per_class={c: (None if rec.iou_skipped[c] else float(rec.iou[c])) for c in range(n)},
        miou=float(rec.iou_mean),
        pa_per_class=[float(v) for v in rec.pa[:n]],
        pixel_accuracy=float(rec.pa_mean),
        fw_iou=float(rec.fw_iou),
        fw_iou_fg=float(rec.fw_iou_fg))


def score(pred: torch.Tensor, target: torch.Tensor, num_classes: int) -> SegMetrics:
    """One launch, one copy of C^2 integers per image, the whole batch scored together: what every reference-named wrapper calls."""
    if pred.dim() == 3 and target.dim() == 3 and pred.is_contiguous() and target.is_contiguous():
        pred, target = pred.view(1, -1, pred.shape[-1]), target.view(1, -1, target.shape[-1])   # masks of a batch are one tall image: one matrix comes back
    return from_confusion(confusion_matrix(pred, target, num_classes))
