"""Mirror of the reference's evaluate.py: `pixel_accuracy` (:11-27), `frequency_weighted_iou` (:29-45), `evaluate` (:48-126) and its command line
(:129-139).  Same names, arguments, errors, report lines and formats; the counting runs on the device (ldiffusion_amd/metrics.py): the PNG pairs are
uploaded in batches of equal shape and each batch is ONE `ldiff_confusion` launch into per-image matrices, instead of ~5 C + C^2 masked sums with a host
synchronisation each per image.

    python -m ldiffusion_amd.evaluate --image-dir PRED --label-dir GT --num-classes 7 [--save-dir DIR]
"""
from __future__ import annotations

import datetime
import glob
import os
import warnings

import numpy as np
import torch

from . import metrics

BATCH = 32   # images of one shape per launch


def pixel_accuracy(pred, target, num_classes):
    """evaluate.py:11-27: logits [B, C, H, W], labels [B, H, W] -> (mean over classes of TP / |target == c|, the per-class list); 1.0 for an absent class."""
    m = metrics.score(pred, target, num_classes)
    return m.pixel_accuracy, m.pa_per_class


def frequency_weighted_iou(pred, target, num_classes, ignore_background=False):
    """evaluate.py:29-45: float32 arithmetic with + 1e-10 in the denominator; `ignore_background` leaves class 0 out without renormalising the
    frequencies, as there."""
    m = metrics.score(pred, target, num_classes)
    return m.fw_iou_fg if ignore_background else m.fw_iou


def _read_pairs(image_files, label_files, num_classes):
    pairs = []
    for img_path, lbl_path in zip(image_files, label_files):
        from PIL import Image
        pred, gt = np.array(Image.open(img_path)), np.array(Image.open(lbl_path))
        if pred.shape != gt.shape:
            raise ValueError(f"尺寸不一致: {img_path} vs {lbl_path}")   # :64-65
        if pred.ndim != 2:
            raise ValueError(f"{img_path}: a class-index image has one channel, got shape {pred.shape}")
        if pred.size and (int(pred.max()) >= num_classes or int(pred.min()) < 0):
            raise ValueError(f"{img_path}: class values must be smaller than num_classes = {num_classes}")   # one_hot (:70) refuses them
        pairs.append((pred.astype(np.uint8), gt if gt.dtype == np.uint8 else gt.astype(np.int64)))
    return pairs


def per_image_confusion(pairs, num_classes, device=None) -> np.ndarray:
    """(prediction, label) arrays -> (int64 [N, C, C], dropped int64 [N]) on the host: batches of equal shape and label type, one launch each, one
    copy at the end."""
    device = device or torch.device("cuda", torch.cuda.current_device())
    groups = {}
    for i, (p, g) in enumerate(pairs):
        groups.setdefault((p.shape, g.dtype.str), []).append(i)
    order, parts = [], []
    for idx in groups.values():
        for k in range(0, len(idx), BATCH):
            sel = idx[k:k + BATCH]
            pred = torch.from_numpy(np.stack([pairs[i][0] for i in sel])).to(device)
            gt = torch.from_numpy(np.stack([pairs[i][1] for i in sel])).to(device)
            dropped = torch.zeros(len(sel), dtype=torch.int64, device=device)
            conf = metrics.confusion_matrix(pred, gt, num_classes, dropped=dropped)
            parts.append(torch.cat([conf.view(len(sel), -1), dropped[:, None]], 1))
            order += sel
    out = np.zeros((len(pairs), num_classes * num_classes + 1), np.int64)
    if parts:
        out[order] = torch.cat(parts).cpu().numpy()
    return out[:, :-1].reshape(len(pairs), num_classes, num_classes), out[:, -1]


def evaluate(image_dir, label_dir, num_classes, save_dir="./eval_results"):
    """evaluate.py:48-126.  Returns {"dice", "iou", "pa", "fwiou"}: the four means of the report (the reference returns nothing)."""
    os.makedirs(save_dir, exist_ok=True)
    image_files = sorted(glob.glob(os.path.join(image_dir, "*.png")))
    label_files = sorted(glob.glob(os.path.join(label_dir, "*.png")))
    if len(image_files) != len(label_files):
        raise ValueError(f"The number of images: {len(image_files)}, The number of labels: {len(label_files)}, they must be equal.")

    conf, dropped = per_image_confusion(_read_pairs(image_files, label_files, num_classes), num_classes)
    if dropped.sum():
        # the one place where the reference is no function of the matrix: its Dice and IoU count a prediction on such a pixel as a false positive
        warnings.warn(f"{int(dropped.sum())} pixels in {int((dropped > 0).sum())} label images are outside [0, {num_classes}) and are left out of all four metrics")
    all_dice, all_iou, all_pa, all_fwiou = [], [], [], []
    per_class_dice, per_class_iou, per_class_pa = [], [], []
    for c in conf:                                                        # foreground means per image, :72-93
        m = metrics.from_confusion(c)
        fg_dice = torch.from_numpy(m.dice_per_class[1:].copy())
        all_dice.append(torch.mean(fg_dice).item())
        per_class_dice.append(fg_dice.numpy())
        iou_vals = [m.iou_per_class[k] for k in range(1, num_classes) if m.iou_per_class[k] is not None]
        all_iou.append(sum(iou_vals) / len(iou_vals) if iou_vals else 1.0)
        per_class_iou.append([m.iou_per_class[k] if m.iou_per_class[k] is not None else 1.0 for k in range(1, num_classes)])
        all_pa.append(np.mean(m.pa_per_class[1:]))
        per_class_pa.append(m.pa_per_class[1:])
        all_fwiou.append(m.fw_iou_fg)

    mean_dice, mean_iou, mean_pa, mean_fwiou = np.mean(all_dice), np.mean(all_iou), np.mean(all_pa), np.mean(all_fwiou)
    per_class_dice = np.mean(per_class_dice, axis=0)
    per_class_iou = np.mean(per_class_iou, axis=0)
    per_class_pa = np.mean(per_class_pa, axis=0)

    timestamp = datetime.datetime.now().strftime("%Y%m%d_%H%M%S")
    save_path = os.path.join(save_dir, f"metrics_{timestamp}.txt")
    with open(save_path, "w") as f:
        f.write("=== Segmentation Evaluation Results ===\n")
        f.write(f"Image dir: {image_dir}\n")
        f.write(f"Label dir: {label_dir}\n")
        f.write(f"Classes: {num_classes}\n\n")
        f.write(f"The number of images: {len(image_files)}\n\n")
        f.write(f"Mean Dice:  {mean_dice:.4f}\n")
        f.write(f"Mean IoU:   {mean_iou:.4f}\n")
        f.write(f"Mean PA:    {mean_pa:.4f}\n")
        f.write(f"Mean FWIoU: {mean_fwiou:.4f}\n\n")
        f.write("Per-class metrics:\n")
        for c in range(1, num_classes):
            idx = c - 1
            f.write(f"Class {c}: Dice={per_class_dice[idx]:.4f}, IoU={per_class_iou[idx]:.4f}, PA={per_class_pa[idx]:.4f}\n")
    print(f"Evaluation complete! Results saved to {save_path}")
    return {"dice": float(mean_dice), "iou": float(mean_iou), "pa": float(mean_pa), "fwiou": float(mean_fwiou)}


if __name__ == "__main__":
    import argparse

    parser = argparse.ArgumentParser(description="Evaluate segmentation results.")
    parser.add_argument("--image-dir", type=str, required=True, help="predicted images folder")
    parser.add_argument("--label-dir", type=str, required=True, help="labels folder")
    parser.add_argument("--num-classes", type=int, required=True, help="num-classes")
    parser.add_argument("--save-dir", type=str, default="./LDiffusion/eval/eval_report", help="results save folder")
    args = parser.parse_args()
    evaluate(args.image_dir, args.label_dir, args.num_classes, args.save_dir)
