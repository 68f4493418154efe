"""Generate tests/golden/reference_dc_ce_loss.npz by running the REFERENCE's own loss modules on the CPU:
DeepSupervisionWrapper(DC_and_CE_loss({'batch_dice': .., 'smooth': 1e-5, 'do_bg': False, 'ddp': False}, {}, weight_ce=1, weight_dice=1, ignore_label=None,
dice_class=MemoryEfficientSoftDiceLoss), weights) as nnUNetTrainer._build_loss builds it (/root/reference/model/nnunetv2/training/nnUNetTrainer/
nnUNetTrainer.py:352-374), with the `nnunetv2` package names stubbed as empty packages and the six files loaded by path.  Only inputs (logits, targets,
weights) and outputs (loss, logit gradients) are committed; /root/reference is never read at test time."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/model/nnunetv2"

for pkg in ["nnunetv2", "nnunetv2.utilities", "nnunetv2.training", "nnunetv2.training.loss"]:
    m = types.ModuleType(pkg)
    m.__path__ = []
    sys.modules[pkg] = m


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
ds = _load("nnunetv2.training.loss.deep_supervision", "training/loss/deep_supervision.py")

SCALES, B = (32, 16, 8, 4), 2
# (name, n_heads, batch_dice, a foreground class absent from the lowest graded scale's target)
CASES = [("n4_batch", 4, True, False), ("n4_sample", 4, False, False), ("n7_batch", 7, True, False), ("n7_sample_absent", 7, False, True)]


def weights(n):   # nnUNetTrainer.py:364-372
    w = np.array([1 / (2 ** i) for i in range(n)])
    w[-1] = 0
    return w / w.sum()


out = {"cases": np.array([c[0] for c in CASES])}
for ci, (name, n, batch_dice, absent) in enumerate(CASES):
    g = torch.Generator().manual_seed(100 + ci)
    w = weights(len(SCALES))
    logits = [(2.0 * torch.randn((B, n, s, s), generator=g)).to(torch.float16).float().requires_grad_(True) for s in SCALES]
    targets = [torch.randint(0, n, (B, 1, s, s), generator=g).float() for s in SCALES]
    if absent:
        for t in targets[1:]:
            t[t == n - 1] = 0          # class n - 1 absent from every scale but the first
        targets[2][1][targets[2][1] == 2] = 1   # and class 2 absent from one SAMPLE of the third scale (per-sample Dice sees sum_gt = 0 there)
    loss_fn = ds.DeepSupervisionWrapper(compound.DC_and_CE_loss({"batch_dice": batch_dice, "smooth": 1e-5, "do_bg": False, "ddp": False}, {}, weight_ce=1,
                                                                weight_dice=1, ignore_label=None, dice_class=dice.MemoryEfficientSoftDiceLoss), w)
    value = loss_fn(logits, targets)
    value.backward()
    out[f"{name}.n_heads"] = np.int64(n)
    out[f"{name}.batch_dice"] = np.int64(batch_dice)
    out[f"{name}.weights"] = w.astype(np.float64)
    out[f"{name}.loss"] = np.float32(value.item())
    for i, s in enumerate(SCALES):
        out[f"{name}.logits{i}"] = logits[i].detach().numpy().astype(np.float16)      # exact: the values were rounded to fp16 above
        out[f"{name}.target{i}"] = targets[i][:, 0].numpy().astype(np.uint8)
        out[f"{name}.grad{i}"] = (logits[i].grad if logits[i].grad is not None else torch.zeros_like(logits[i])).numpy().astype(np.float32)
    print(name, "loss", value.item())

path = os.path.join(ROOT, "tests", "golden", "reference_dc_ce_loss.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
