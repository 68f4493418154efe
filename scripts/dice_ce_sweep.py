"""Bit-level sweep of the tissue head's Dice + cross-entropy entries (csrc/kernels_segtrain.hip), plain and with nnU-Net's ignore label, one line per case:

    <form> n=<n_heads> <H>x<W> batch_dice=<0|1> <u8|i64> | dice_ce <sha256 of loss and dlogits> | stats <sha256 of the rows> | from_sums <sha256 of loss and dlogits>

over n_heads 3 / 9 / 17 / 32 (row pitch 8 / 16 / 24 / 32: every instantiation of the streaming kernels), 15 x 13, 48 x 40 and 72 x 64 pixels at B = 2 (fewer
pixels than a workgroup has threads, one ragged chunk, a full chunk plus a ragged one), batch_dice on and off, uint8 and int64 labels, and the forms

    plain        no ignore label
    none         the ignore form, no pixel ignored
    blobs        about 30 % of the pixels ignored (tests/nnunet_ignore_ref.ignore_blobs)
    image        one whole image ignored
    all          the whole batch ignored
    bad          blobs, and one label that is neither a class nor the ignore label: NaN in the loss and in that pixel's row, compared as bytes like the rest

then the tiny trainer of tests/test_gpu_nnunet_ignore.py after three steps, plain and with an ignore label.  from_sums is the split entry at world 1 on
the rows of stats.  Only the Python surface of ldiffusion_amd.autograd and nnunet_train is used, so the same file runs against any build:

    python scripts/dice_ce_sweep.py [--tree PATH]     # PATH: a checkout with a built libldiff_hip.so (default: this one)

Two builds compute the same loss if and only if their outputs are identical line for line (profiles/dice_ce_unified_hashes.txt)."""
import argparse
import hashlib
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
opt = ap.parse_args()
sys.path.insert(0, os.path.join(opt.tree, "tests"))
sys.path.insert(0, opt.tree)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import nnunet_ignore_ref as iref  # noqa: E402
import nnunet_train_ref as ref  # noqa: E402
from ldiffusion_amd import autograd as ag, nnunet, nnunet_train  # noqa: E402

DEV = "cuda:0"
WEIGHT, SCALE = 4 / 7, 1024.0


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def case(form, n, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.zeros((2, H, W, (n + 7) // 8 * 8), dtype=torch.float16)
    logits[..., :n] = (2.0 * torch.randn((2, H, W, n), generator=g)).to(torch.float16)
    logits[..., n:] = 7.0
    target = torch.randint(0, n, (2, H, W), generator=g)
    if form in ("blobs", "bad"):
        target = iref.ignore_blobs(target, n, 0.3, seed + 1)
    if form == "bad":
        spot = tuple(int(v) for v in (target != n).nonzero()[0])
        target[spot] = 200
    if form == "image":
        target[1] = n
    if form == "all":
        target[:] = n
    return logits, target


def losses():
    seed = 0
    for form in ("plain", "none", "blobs", "image", "all", "bad"):
        for n in (3, 9, 17, 32):
            for H, W in ((15, 13), (48, 40), (72, 64)):
                seed += 1
                logits, target = case(form, n, H, W, 5000 + seed)
                kw = {} if form == "plain" else {"ignore_label": n}
                for bd in (True, False):
                    for i64 in (False, True):
                        z, t = logits.to(DEV), (target if i64 else target.to(torch.uint8)).to(DEV)
                        one = ag.dice_ce(z, t, n, bd, WEIGHT, SCALE, **kw)
                        sums = ag.dice_ce_stats(z, t, n, bd, **kw)
                        split = ag.dice_ce_from_sums(z, t, n, bd, sums, sums, 1, WEIGHT, SCALE, **kw)
                        torch.cuda.synchronize()
                        print(f"{form} n={n} {H}x{W} batch_dice={int(bd)} {'i64' if i64 else 'u8'} | dice_ce {sha(*one)} | stats {sha(sums)} | from_sums {sha(*split)}")


def trainers():
    golden = os.path.join(opt.tree, "tests", "golden")
    with open(os.path.join(golden, "nnunet_plans_2d.json")) as f:
        plans = json.load(f)
    with open(os.path.join(golden, "nnunet_dataset.json")) as f:
        ds = json.load(f)
    spec = nnunet.network_spec(plans, "2d_reduced", ds)
    batch_dice, k = bool(plans["configurations"]["2d"]["batch_dice"]), spec["n_heads"]
    g = torch.Generator().manual_seed(9)
    x = F.avg_pool2d(torch.randn((2, 3, 36, 36), generator=g), 5, 1) * 2.2
    targets = ref.label_maps(2, k, 32, spec["n_stages"] - 1, 10)
    sd = nnunet_train.initial_state_dict(spec, 7)
    for name, kw, tg in (("plain", {}, targets), ("ignore_label", {"ignore_label": k}, [iref.ignore_blobs(t, k, 0.3, 40 + i) for i, t in enumerate(targets)])):
        tr = nnunet_train.Trainer(spec, sd, batch_dice, 10, device=DEV, configuration="2d_reduced", **kw)
        steps = [float(tr.train_step(x, tg)).hex() for _ in range(3)]
        torch.cuda.synchronize()
        bufs = tr.state["sgd"]["momentum_buffer"]
        print(f"trainer {name} | params {sha(*tr.params)} | buffers {sha(*(bufs[i] for i in sorted(bufs)))} | losses {steps}")


if __name__ == "__main__":
    losses()
    trainers()
