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

With --folds K1,K2,... (e.g. 1,3,5) the fold ensemble is measured instead (DESIGN.md section 7 "Tissue head, folds and ensemble"): max(K) handles stay resident; per K,
`FoldEnsemble.predict_mask(batch_tiles=b)` (one gather per chunk, K head calls, ONE ldiff_op_window_finish_ensemble) against K single-fold `TrainedModel.predict_mask(batch_tiles=b)`
calls on the same handles, b = the first entry of --batch-tiles, the sides alternating after two warm-up calls of every handle and of the ensemble.  The yardstick is K x the single-fold
time of the same run.  Also: the device time (events) of the ensemble finish launch beside ldiff_op_window_finish's on accumulators of the image's size, and the device memory in use
with all handles resident (free memory before and after, so the library's own allocations count).

usage: python scripts/bench_tissue_window.py [--passes 7] [--size 1024] [--batch-tiles 1,2,3,9] [--config 2d] [--folds 1,3,5] [--out FILE]
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
    ap.add_argument("--folds", default=None, help="fold counts of the ensemble measurement, e.g. 1,3,5")
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
    tile, axes, step = tuple(spec["patch_size"]), (0, 1), 0.5
    g = torch.Generator().manual_seed(5)
    image = (torch.nn.functional.avg_pool2d(torch.rand((1, 3, args.size + 8, args.size + 8), generator=g), 9, 1)[0] * 254 + 1).to(dev)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def finish():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    if args.folds:
        bench_folds(args, spec, image, tile, step, axes, dev, say)
        return finish()
    sd = nnunet_ref.synthetic_state_dict(spec, 27)
    plan = tiling.window_plan((args.size, args.size), tile, step, axes, 1)
    n_tiles, M = len(plan.origins), len(plan.variants)
    sides = [None] + [int(b) for b in args.batch_tiles.split(",")]
    models = {b: nnunet.TrainedModel(PlainConvUNet(spec, sd, dev), spec, axes) for b in sides}

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
    finish()


def bench_folds(args, spec, image, tile, step, axes, dev, say):
    counts = [int(k) for k in args.folds.split(",")]
    b = int(args.batch_tiles.split(",")[0])
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    models = [nnunet.TrainedModel(PlainConvUNet(spec, nnunet_ref.synthetic_state_dict(spec, 27 + k), dev), spec, axes) for k in range(max(counts))]
    torch.cuda.synchronize()
    created = free0 - torch.cuda.mem_get_info()[0]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    say(f"tissue fold ensemble: config {args.config} (features {spec['features']}), image {args.size}^2, tile {tile}, step {step}, mirror axes {axes}, batch_tiles {b}; "
        f"device {torch.cuda.get_device_name(0)}; {args.passes} alternating passes after 2 warm-ups of every handle and every ensemble")
    for m in models:
        for _ in range(2):
            m.predict_mask(image, tile, step, axes, batch_tiles=b)
        m.network.check_finite()
    ensembles = {K: nnunet.FoldEnsemble(models[:K]) for K in counts}
    for e in ensembles.values():
        for _ in range(2):
            e.predict_mask(image, tile, step, axes, batch_tiles=b)
    torch.cuda.synchronize()
    resident = free0 - torch.cuda.mem_get_info()[0]
    torch.cuda.reset_peak_memory_stats()          # from here on: the timed calls only
    held = torch.cuda.memory_allocated()
    say()
    say("| folds K | ensemble median ms | min .. max ms | K single-fold calls median ms | min .. max ms | K singles / ensemble |")
    say("|---|---|---|---|---|---|")
    raw = {}
    for K in counts:
        te, ts = [], []
        for _ in range(args.passes):
            te.append(timed(lambda: ensembles[K].predict_mask(image, tile, step, axes, batch_tiles=b))[0])
            ts.append(timed(lambda: [m.predict_mask(image, tile, step, axes, batch_tiles=b) for m in models[:K]])[0])
        raw[K] = {"ensemble": [round(v, 3) for v in te], "singles": [round(v, 3) for v in ts]}
        say(f"| {K} | {statistics.median(te):.2f} | {min(te):.2f} .. {max(te):.2f} | {statistics.median(ts):.2f} | {min(ts):.2f} .. {max(ts):.2f} | "
            f"{statistics.median(ts) / statistics.median(te):.3f} |")
    peak_timed = torch.cuda.max_memory_allocated()
    # the finish launches alone, on accumulators of the image's size (float16, the predictor's)
    heads, n = spec["n_heads"], args.size
    accs = [torch.randn((heads, n, n), device=dev).half() for _ in range(max(counts))]
    cnt = (torch.rand((n, n), device=dev) * 30 + 1).half()
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    mask = torch.zeros((n, n), dtype=torch.uint8, device=dev)

    def device_us(fn, reps=20):
        fn()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(reps):
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            ts.append(start.elapsed_time(stop) * 1e3)
        return statistics.median(ts), min(ts), max(ts)

    say()
    say("| finish launch (mask out, float16, %d heads, %d^2) | median us | min .. max us |" % (heads, n))
    say("|---|---|---|")
    m_, lo, hi = device_us(lambda: tiling.window_finish(accs[0], cnt, (0, 0, n, n), flag, mask=mask))
    say(f"| ldiff_op_window_finish | {m_:.1f} | {lo:.1f} .. {hi:.1f} |")
    for K in counts:
        m_, lo, hi = device_us(lambda: tiling.window_finish_ensemble(accs[:K], cnt, (0, 0, n, n), flag, mask=mask))
        say(f"| ldiff_op_window_finish_ensemble, K = {K} | {m_:.1f} | {lo:.1f} .. {hi:.1f} |")
    say()
    K, (Hn, Wn) = max(counts), image.shape[1:]
    window = (K * heads + 2) * Hn * Wn * 2 + b * 4 * spec["in_channels"] * tile[0] * tile[1] * 4
    say(f"device memory, free before - free after (the library's own allocations count): {created / 2**20:.0f} MiB with {len(models)} handles created (weights), "
        f"{resident / 2**20:.0f} MiB after every handle's and every ensemble's warm-up at batch {b * 4} ({resident / 2**20 / len(models):.0f} MiB per handle: workspace, captured graph, "
        f"and torch's cached blocks)")
    say(f"torch's allocator during the timed calls (peak statistics reset after the warm-up): {held / 2**20:.0f} MiB held at their start (image, handles' tensors), peak "
        f"{peak_timed / 2**20:.0f} MiB; the ensemble window of K = {K} itself holds {window / 2**20:.0f} MiB (K accumulators of {heads} heads, count and scratch planes in float16, the gathered batch)")
    say("raw ms per pass: " + json.dumps(raw))


if __name__ == "__main__":
    main()
