"""Confusion matrices on the HIP library (ldiff_confusion, ldiffusion_amd.metrics) against what a user had before it existed, on the same GPU:

  reference   the reference's own formulation: evaluate.py:29-45 (C^2 masked sums with an .item() each), and for the mask form's "all four metrics"
              row also utils.py:55-104 + evaluate.py:11-27 (their 2C - 3C more), on device tensors
  bincount    torch.bincount(t * C + p, minlength=C * C) per image (the arg-max by torch.argmax first in logit form), then one copy

Shapes: B = 8 of 512 x 512 and B = 2 of 1024 x 1024, C = 7; mask form (uint8 prediction and target) and logit form (float32 and float16 logits, int64
target as the reference holds it).  Inputs are segmentation-like: constant blocks of 32 x 32 pixels with 5 % of the pixels relabelled at random, and a
uniform-random variant (the worst case for the kernel's uniform-wave path, the best for LDS atomics).

Every side is timed after a warm-up as --reps rounds of --inner calls, sides alternating, host clock around work that ends in a device synchronise;
the library's side ends in the copy of the matrix to the host, like the others, so the figures are call times including launch and copy overhead.  The
kernel's own time is from HIP events around the launch (ldiff_prof_*), with the bytes the algorithm needs (2 B per pixel in mask form, C x element + 8 B in
logit form with int64 labels) over that time as achieved bytes/s.  Before timing, the three sides' matrices are compared (exact).

usage: python scripts/bench_metrics.py [--reps 10] [--inner 10] [--out profiles/metrics_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ldiffusion_amd import _lib, metrics  # noqa: E402

SHAPES = ((8, 512, 512), (2, 1024, 1024))
C = 7


def labels(B, H, W, seed, noise):
    g = torch.Generator().manual_seed(seed)
    if noise >= 1.0:
        return torch.randint(0, C, (B, H, W), generator=g, dtype=torch.uint8)
    blocks = torch.randint(0, C, (B, H // 32, W // 32), generator=g, dtype=torch.uint8)
    x = blocks.repeat_interleave(32, 1).repeat_interleave(32, 2)
    flip = torch.rand((B, H, W), generator=g) < noise
    return torch.where(flip, torch.randint(0, C, (B, H, W), generator=g, dtype=torch.uint8), x)


def reference_fwiou_hist(pred_labels, target):
    """evaluate.py:32-35 on device tensors: C^2 masked sums, an .item() each."""
    hist = torch.zeros((C, C), dtype=torch.float)
    for i in range(C):
        for j in range(C):
            hist[i, j] = ((target == i) & (pred_labels == j)).sum().item()
    return hist


def reference_other_three(pred_labels, target):
    """utils.py:55-104 and evaluate.py:11-27 on device tensors, given the arg-max: the masked sums and host synchronisations they make."""
    t, p = target.view(-1), pred_labels.view(-1)
    out = []
    for c in range(C):
        tc, pc = (t == c).float(), (p == c).float()
        if torch.sum(tc) == 0 and torch.sum(pc) == 0:
            continue
        tp, fp, fn = torch.sum(tc * pc), torch.sum((1 - tc) * pc), torch.sum(tc * (1 - pc))
        out.append(0 if tp + fp + fn == 0 else (2 * tp / (2 * tp + fp + fn)).item())
    for c in range(C):
        pi, ti = pred_labels == c, target == c
        out.append(((pi & ti).sum().item(), (pi | ti).sum().item()))
    for c in range(C):
        pi, ti = pred_labels == c, target == c
        out.append(((pi & ti).sum().item(), ti.sum().item()))
    return out


def bincount_conf(pred_labels, target):
    B = target.shape[0]
    idx = target.reshape(B, -1).long() * C + pred_labels.reshape(B, -1).long()
    return torch.stack([torch.bincount(idx[b], minlength=C * C) for b in range(B)]).view(B, C, C)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics needs a GPU: a CPU run gives no time")
    dev = "cuda:0"
    lib = _lib.load()
    lines = [f"confusion matrices, C = {C}; {args.reps} rounds x {args.inner} calls per side, sides alternating; ms per call incl. the copy of the result to the host: median (min .. max)",
             f"device: {torch.cuda.get_device_name(0)}; kernel = HIP-event time of the one launch, GB/s = algorithmic bytes over it"]
    for B, H, W in SHAPES:
        for noise, what in ((0.05, "32 x 32 constant blocks, 5 % noise"), (1.0, "uniform random labels")):
            t8 = labels(B, H, W, 1, noise).to(dev)
            p8 = labels(B, H, W, 2, noise).to(dev)
            p8 = torch.where(torch.rand((B, H, W), device=dev) < 0.8, t8, p8)            # a prediction that is mostly right
            t64 = t8.long()
            x32 = torch.randn((B, C, H, W), device=dev)
            x32.scatter_add_(1, p8.long()[:, None], torch.full((B, 1, H, W), 6.0, device=dev))   # logits whose arg-max is mostly p8
            x16 = x32.half()
            forms = {
                "mask u8 / u8": (p8, t8, lambda: p8, 2.0),
                "logits f32 / i64": (x32, t64, lambda: torch.argmax(x32, 1), 4.0 * C + 8),
                "logits f16 / i64": (x16, t64, lambda: torch.argmax(x16, 1), 2.0 * C + 8),
            }
            lines.append(f"B = {B}, {H} x {W}, {what}")
            for form, (pred, tgt, to_labels, bytes_per_pixel) in forms.items():
                sides = {
                    "ldiff_confusion": lambda: metrics.confusion_matrix(pred, tgt, C).cpu(),
                    "torch bincount": lambda: bincount_conf(to_labels(), tgt).cpu(),
                    "reference (C^2 .item())": lambda: reference_fwiou_hist(to_labels(), tgt),
                }
                if form.startswith("mask"):
                    sides["reference, all four metrics"] = lambda: (reference_fwiou_hist(to_labels(), tgt), reference_other_three(to_labels(), tgt))
                ours = sides["ldiff_confusion"]()
                assert torch.equal(ours, sides["torch bincount"]()), "library and bincount disagree"
                assert torch.equal(ours.sum(0).float(), sides["reference (C^2 .item())"]()), "library and the reference's hist disagree"
                times = {name: [] for name in sides}
                for name, fn in sides.items():
                    for _ in range(3):
                        fn()
                for _ in range(args.reps):
                    for name, fn in sides.items():
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(args.inner):
                            fn()
                        torch.cuda.synchronize()
                        times[name].append((time.perf_counter() - t0) * 1e3 / args.inner)
                _lib.prof_collect()
                lib.ldiff_prof_enable(1)
                try:
                    for _ in range(20):
                        metrics.confusion_matrix(pred, tgt, C)
                    torch.cuda.synchronize()
                finally:
                    lib.ldiff_prof_enable(0)
                row = [r for r in _lib.prof_collect() if r["name"] == "confusion"][0]
                k_ms = row["ms"] / row["launches"]
                assert row["bytes"] / row["launches"] == bytes_per_pixel * B * H * W
                lines.append(f"  {form:17s} kernel {k_ms * 1e3:7.1f} us = {row['bytes'] / row['launches'] / k_ms * 1e-6:7.1f} GB/s")
                for name in sides:
                    t = times[name]
                    lines.append(f"      {name:28s} {statistics.median(t):9.3f} ms ({min(t):.3f} .. {max(t):.3f})   x{statistics.median(t) / statistics.median(times['ldiff_confusion']):.1f}")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
