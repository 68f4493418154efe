"""Generate tests/golden/reference_dc_focal_loss.npz by running the REFERENCE's own modules on the CPU, in float64: the region losses
nnUNetTrainer._build_loss builds for a dataset with regions (nnUNetTrainer.py:349-355) -- DC_and_Focal_loss({}, {'batch_dice': .., 'do_bg': True,
'smooth': 1e-5, 'ddp': False}, use_ignore_label=.., dice_class=MemoryEfficientSoftDiceLoss) -- and upstream's DC_and_BCE_loss with the same arguments,
and LabelManager's region rules (label_handling.py).  Loaded as scripts/gen_golden_dc_ce_loss_ignore.py loads them.
usage: python scripts/gen_golden_dc_focal_loss.py <the reference's model/nnunetv2 folder>

As shipped, the reference's compound_losses.py never imports the name `F` that its FocalLoss calls (`F.binary_cross_entropy_with_logits`), so its own
region path raises NameError.  This script gives the module the one meaning the name can have, torch.nn.functional, and says so in `provenance`.

B = 2, R = 3, 6 x 5.  One label map with values 0 .. 3 and a second with about 30 % of the pixels set to the ignore label 4; the one-hot region target the
losses take is formed here from the label map (one channel per region, and last the ignore channel), which is what the reference's
ConvertSegmentationToRegionsTransform hands them.  Logits are fp16-exact and stored as fp16, losses and gradients as float64.  Only inputs and outputs
are committed; the reference is never read at test time."""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1]

for pkg in ["nnunetv2", "nnunetv2.utilities", "nnunetv2.training", "nnunetv2.training.loss", "nnunetv2.utilities.label_handling", "acvl_utils",
            "acvl_utils.cropping_and_padding", "batchgenerators", "batchgenerators.utilities"]:
    m = types.ModuleType(pkg)
    m.__path__ = []
    sys.modules[pkg] = m
# what label_handling.py imports and the paths exercised here never call
for name, attr in [("acvl_utils.cropping_and_padding.bounding_boxes", "bounding_box_to_slice"), ("batchgenerators.utilities.file_and_folder_operations", "join"),
                   ("nnunetv2.utilities.find_class_by_name", "recursive_find_python_class")]:
    m = types.ModuleType(name)
    setattr(m, attr, None)
    sys.modules[name] = m


def _load(modname, rel):
    spec = importlib.util.spec_from_file_location(modname, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[modname] = mod
    spec.loader.exec_module(mod)
    return mod


_load("nnunetv2.utilities.ddp_allgather", "utilities/ddp_allgather.py")
_load("nnunetv2.utilities.helpers", "utilities/helpers.py")
dice = _load("nnunetv2.training.loss.dice", "training/loss/dice.py")
_load("nnunetv2.training.loss.robust_ce_loss", "training/loss/robust_ce_loss.py")
compound = _load("nnunetv2.training.loss.compound_losses", "training/loss/compound_losses.py")
lh = _load("nnunetv2.utilities.label_handling.label_handling", "utilities/label_handling/label_handling.py")

PROVENANCE = ("reference model/nnunetv2: training/loss/compound_losses.py DC_and_Focal_loss / DC_and_BCE_loss, training/loss/dice.py "
              "MemoryEfficientSoftDiceLoss, utilities/label_handling/label_handling.py LabelManager; float64 on the CPU.  ")
if not hasattr(compound, "F"):
    compound.F = torch.nn.functional
    PROVENANCE += ("compound_losses.py does not import the name F that FocalLoss uses (NameError as shipped); the generator set "
                   "compound_losses.F = torch.nn.functional, the one meaning the name can have.")

B, R, H, W = 2, 3, 6, 5
LABELS = {"background": 0, "whole": [1, 2, 3], "core": [2, 3], "enhancing": 3}
LABELS_IGNORE = dict(LABELS, ignore=4)
ORDER = [1, 2, 3]

g = torch.Generator().manual_seed(731)
logits16 = (2.0 * torch.randn((B, R, H, W), generator=g)).to(torch.float16)
seg = torch.randint(0, 4, (B, H, W), generator=g)
seg_ign = seg.clone()
while (seg_ign == 4).double().mean() < 0.3:
    b, y, x = (int(torch.randint(0, hi, (1,), generator=g)) for hi in (B, H, W))
    seg_ign[b, y:y + 2, x:x + 2] = 4

out = {"provenance": np.array(PROVENANCE), "logits": logits16.numpy(), "labels": np.array(json.dumps(LABELS)), "labels_ignore": np.array(json.dumps(LABELS_IGNORE)),
       "regions_class_order": np.array(ORDER, dtype=np.int64), "seg": seg.numpy().astype(np.uint8), "seg_ignore": seg_ign.numpy().astype(np.uint8)}


def onehot_regions(s, regions, ignore):
    planes = [torch.isin(s, torch.tensor(r if isinstance(r, tuple) else (r,))) for r in regions]
    if ignore is not None:
        planes.append(s == ignore)
    return torch.stack(planes, 1).double()


cases = []
for use_ignore in (False, True):
    lm = lh.LabelManager(LABELS_IGNORE if use_ignore else LABELS, ORDER)
    target = onehot_regions(seg_ign if use_ignore else seg, lm.foreground_regions, lm.ignore_label)
    for batch_dice in (True, False):
        for form in ("focal", "bce"):
            dkw = {"batch_dice": batch_dice, "do_bg": True, "smooth": 1e-5, "ddp": False}
            if form == "focal":
                fn = compound.DC_and_Focal_loss({}, dkw, use_ignore_label=use_ignore, dice_class=dice.MemoryEfficientSoftDiceLoss)
            else:
                fn = compound.DC_and_BCE_loss({}, dkw, use_ignore_label=use_ignore, dice_class=dice.MemoryEfficientSoftDiceLoss)
            z = logits16.double().requires_grad_(True)
            value = fn(z, target)
            value.backward()
            name = f"{form}_{'ignore' if use_ignore else 'plain'}_{'batch' if batch_dice else 'sample'}"
            cases.append(name)
            out[f"{name}.loss"] = np.float64(value.item())
            out[f"{name}.grad"] = z.grad.numpy()
            print(name, value.item())
out["cases"] = np.array(cases)

# LabelManager: three dictionaries -- plain regions, a region that contains 0 among other labels, a permuted regions_class_order with an ignore label
g = torch.Generator().manual_seed(732)
lm_logits = (1.5 * torch.randn((R, H, W), generator=g)).float()
out["lm.logits"] = lm_logits.numpy()
LM = [("plain", LABELS, ORDER), ("with_zero", {"background": 0, "a": [0, 1], "b": [1, 2], "c": 2}, [1, 2, 3]), ("permuted", LABELS_IGNORE, [3, 1, 2])]
out["lm.names"] = np.array([n for n, _, _ in LM])
for name, labels, order in LM:
    lm = lh.LabelManager(labels, order)
    out[f"lm.{name}.labels"] = np.array(json.dumps(labels))
    out[f"lm.{name}.order"] = np.array(order, dtype=np.int64)
    out[f"lm.{name}.foreground_regions"] = np.array(json.dumps([list(r) if isinstance(r, tuple) else r for r in lm.foreground_regions]))
    out[f"lm.{name}.all_labels"] = np.array([int(v) for v in lm.all_labels], dtype=np.int64)
    out[f"lm.{name}.num_segmentation_heads"] = np.int64(lm.num_segmentation_heads)
    out[f"lm.{name}.ignore_label"] = np.int64(-1 if lm.ignore_label is None else lm.ignore_label)
    out[f"lm.{name}.segmentation"] = lm.convert_logits_to_segmentation(lm_logits).numpy().astype(np.int16)
    print(name, lm.foreground_regions, lm.num_segmentation_heads)

path = os.path.join(ROOT, "tests", "golden", "reference_dc_focal_loss.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
