"""Whole-image prediction of the nnU-Net tissue head: the per-tile sliding window (`TrainedModel.predict_mask(batch_tiles=None)`: one head call per tile and
mirror variant, torch.flip / add / divide and one ldiff_window_accumulate per tile) against the batched one (`batch_tiles=b`: ldiff_op_window_gather, ONE head call
of batch b * M, ldiff_op_window_accumulate_batch per chunk, then ldiff_op_window_finish).

Case: the planner's default width (tests/golden/nnunet_plans_2d.json "2d", 512^2 patches), a 1024^2 image, step 0.5, both mirror axes: 9 tiles x 4 variants =
36 evaluations.  batch_tiles 1, 2, 3, 9 are batches of 4, 8, 12, 36.  Synthetic weights, a smooth synthetic image.

Every side has a model handle of its own (a handle keeps one captured graph; sides of different batch would evict each other's).  After two warm-up calls per
side (eager, then capture) the sides alternate inside one process; each call is timed with a host clock around work that ends in a device synchronise
(preprocessing, window, arg-max, un-crop).  Median, min .. max over the passes; the per-tile path of the same run is the yardstick, no threshold is
asserted.  The masks of all sides are compared (they must be equal bit for bit).  Peak bytes of the batch x and of the prediction per batch_tiles are computed
from the shapes.

usage: python scripts/bench_tissue_window.py [--passes 7] [--size 1024] [--batch-tiles 1,2,3,9] [--config 2d] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import nnunet_ref  # noqa: E402  (tests/: synthetic weights)
from ldiffusion_amd import nnunet, tiling  # noqa: E402
from ldiffusion_amd.models import PlainConvUNet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batch-tiles", default="1,2,3,9")
    ap.add_argument("--config", default="2d")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tissue_window.py measures on the GPU; there is none")
    dev = "cuda:0"
    with open(os.path.join(ROOT, "tests", "golden", "nnunet_plans_2d.json")) as f:
        plans = json.load(f)
    with open(os.path.join(ROOT, "tests", "golden", "nnunet_dataset.json")) as f:
        ds = json.load(f)
    spec = nnunet.network_spec(plans, args.config, ds)
    sd = nnunet_ref.synthetic_state_dict(spec, 27)
    tile, axes, step = tuple(spec["patch_size"]), (0, 1), 0.5
    g = torch.Generator().manual_seed(5)
    image = (torch.nn.functional.avg_pool2d(torch.rand((1, 3, args.size + 8, args.size + 8), generator=g), 9, 1)[0] * 254 + 1).to(dev)
    plan = tiling.window_plan((args.size, args.size), tile, step, axes, 1)
    n_tiles, M = len(plan.origins), len(plan.variants)
    sides = [None] + [int(b) for b in args.batch_tiles.split(",")]
    models = {b: nnunet.TrainedModel(PlainConvUNet(spec, sd, dev), spec, axes) for b in sides}
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def call(b):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mask = models[b].predict_mask(image, tile, step, axes, batch_tiles=b)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, mask

    say(f"tissue window: config {args.config} (features {spec['features']}), image {args.size}^2, tile {tile}, step {step}, mirror axes {axes}: "
        f"{n_tiles} tiles x {M} variants = {n_tiles * M} evaluations; device {torch.cuda.get_device_name(0)}; {args.passes} alternating passes after 2 warm-ups per side")
    masks = {}
    for b in sides:
        for _ in range(2):
            _, masks[b] = call(b)
        models[b].network.check_finite()
    for b in sides[1:]:
        differ = int((masks[b] != masks[None]).sum())
        say(f"  mask of batch_tiles {b} vs the per-tile path: {differ} of {masks[None].numel()} pixels differ")
    times = {b: [] for b in sides}
    for _ in range(args.passes):
        for b in sides:
            times[b].append(call(b)[0])
    base = statistics.median(times[None])
    say()
    say("| path | head calls x batch | median ms | min .. max ms | per-tile / this | x bytes | pred bytes |")
    say("|---|---|---|---|---|---|---|")
    heads = spec["n_heads"]
    for b in sides:
        t = times[b]
        if b is None:
            calls, B, name = n_tiles * M, 1, "per tile (batch_tiles=None)"
        else:
            calls, B, name = -(-n_tiles // b), b * M, f"batch_tiles={b}"
        xb, pb = B * spec["in_channels"] * tile[0] * tile[1] * 4, B * heads * tile[0] * tile[1] * 4
        say(f"| {name} | {calls} x {B} | {statistics.median(t):.2f} | {min(t):.2f} .. {max(t):.2f} | {base / statistics.median(t):.3f} | {xb / 2**20:.1f} MiB | {pb / 2**20:.1f} MiB |")
    say()
    say("raw ms per pass: " + json.dumps({str(b): [round(v, 3) for v in t] for b, t in times.items()}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
