"""Generate tests/golden/reference_dc_ce_loss_ignore.npz by running the REFERENCE's own loss modules on the CPU, in float64:
DeepSupervisionWrapper(DC_and_CE_loss({'batch_dice': .., 'smooth': 1e-5, 'do_bg': False, 'ddp': False}, {}, weight_ce=1, weight_dice=1, ignore_label=k,
dice_class=MemoryEfficientSoftDiceLoss), weights) as nnUNetTrainer._build_loss builds it for a dataset with an ignore label (nnUNetTrainer.py:352-374),
loaded as scripts/gen_golden_dc_ce_loss.py loads them.  usage: python scripts/gen_golden_dc_ce_loss_ignore.py <the reference's model/nnunetv2 folder>

B = 2, 24 x 20 and 12 x 10 (two scales, BOTH graded: weights 2/3 and 1/3 -- the trainer's own rule would zero the second of two), k = n.  Targets: `blobs`
(about 30 % of the pixels ignored, in rectangles), `image` (the second image ignored entirely), `all` (the whole batch ignored), `none` (no pixel ignored).
The full product n x batch_dice x targets does not fit the 100 KiB a fixture may take (one n = 9 gradient is 43 KB in float32), so the file holds the cases
below: every n, both batch_dice settings and every target kind occur, and each n meets both a partly ignored and a degenerate target.  The logits are
fp16-exact and stored as fp16, the loss as float64, the gradients -- computed in float64 -- rounded once to float32.  Only inputs and outputs are
committed; the reference is never read at test time."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1]

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

SCALES, B = ((24, 20), (12, 10)), 2
WEIGHTS = np.array([2 / 3, 1 / 3])
# (n_heads, batch_dice, target kind)
CASES = [(3, True, "blobs"), (3, True, "image"), (3, True, "all"), (3, True, "none"), (3, False, "blobs"),
         (9, True, "image"), (9, False, "all")]


def make_targets(n, kind, g):
    """One label map per scale (the lower one drawn on its own: the loss does not care), classes 0 .. n - 1, the ignored pixels n."""
    out = []
    for h, w in SCALES:
        t = torch.randint(0, n, (B, 1, h, w), generator=g)
        if kind == "blobs":   # rectangles until about 30 % of the pixels are covered
            while (t == n).double().mean() < 0.3:
                b = int(torch.randint(0, B, (1,), generator=g))
                y, x = int(torch.randint(0, h, (1,), generator=g)), int(torch.randint(0, w, (1,), generator=g))
                t[b, 0, y:y + max(2, h // 4), x:x + max(2, w // 4)] = n
        elif kind == "image":
            t[1] = n
        elif kind == "all":
            t[:] = n
        out.append(t.double())
    return out


out = {"cases": np.array([f"n{n}_{'batch' if bd else 'sample'}_{kind}" for n, bd, kind in CASES]), "weights": WEIGHTS}
logits_of = {}
for ci, (n, batch_dice, kind) in enumerate(CASES):
    name = str(out["cases"][ci])
    if n not in logits_of:   # one set of logits per n, shared by its cases
        g = torch.Generator().manual_seed(500 + n)
        logits_of[n] = [(2.0 * torch.randn((B, n, h, w), generator=g)).to(torch.float16) for h, w in SCALES]
        for i, z in enumerate(logits_of[n]):
            out[f"n{n}.logits{i}"] = z.numpy()
    logits = [z.double().requires_grad_(True) for z in logits_of[n]]
    targets = make_targets(n, kind, torch.Generator().manual_seed(600 + ci))
    loss_fn = ds.DeepSupervisionWrapper(compound.DC_and_CE_loss({"batch_dice": batch_dice, "smooth": 1e-5, "do_bg": False, "ddp": False}, {}, weight_ce=1,
                                                                weight_dice=1, ignore_label=n, dice_class=dice.MemoryEfficientSoftDiceLoss), WEIGHTS)
    value = loss_fn(logits, targets)
    value.backward()
    out[f"{name}.n_heads"] = np.int64(n)
    out[f"{name}.batch_dice"] = np.int64(batch_dice)
    out[f"{name}.loss"] = np.float64(value.item())
    for i in range(len(SCALES)):
        out[f"{name}.target{i}"] = targets[i][:, 0].numpy().astype(np.uint8)
        out[f"{name}.grad{i}"] = (logits[i].grad if logits[i].grad is not None else torch.zeros_like(logits[i])).numpy().astype(np.float32)
    print(name, "loss", value.item(), "ignored", float((targets[0] == n).double().mean()))

path = os.path.join(ROOT, "tests", "golden", "reference_dc_ce_loss_ignore.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
