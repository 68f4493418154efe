"""Time per training batch of the tissue head's data path (ldiffusion_amd.nnunet_data) at the planner's shape: B = 12, 3 x 512^2, 7 deep-supervision scales,
cases of 1024^2.  Device time by events around the two launches (ldiff_op_seg_sample, ldiff_op_seg_intensity), after warm-up:
    worst     every transform on for every sample and channel (rotation + scale, noise, blur, brightness, contrast, both gammas)
    expected  the tables draw_batch produces (nnU-Net's probabilities)
    host      wall time of a whole PatchLoader batch (draws, table upload, launches) without waiting for the device
and, for scale, the same pipeline in numpy / scipy on 16 threads, one sample per task (what nnU-Net's worker pool does).
--lowres adds, from the same process, the two device rows with the low-resolution simulation (ldiff_op_seg_intensity_lr):
    worst_lowres     the worst case above with every plane's step on, zooms spread over 0.5 ... 1
    expected_lowres  the tables draw_batch(lowres=True) produces (25 % of the samples, half of their channels)
and the loader rows with PatchLoader(lowres=True).  The numpy pipeline does not run the step.

    python scripts/bench_nnunet_data.py [--batches 20] [--warmup 3] [--no-numpy] [--lowres]
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ldiffusion_amd import _lib  # noqa: E402
from ldiffusion_amd import nnunet_data as nd  # noqa: E402

B, C, PATCH, SCALES, CASE, N_HEADS, N_CASES = 12, 3, (512, 512), 7, 1024, 7, 8


def make_store(device):
    g = torch.Generator().manual_seed(0)
    cases = []
    for i in range(N_CASES):
        img = (torch.nn.functional.avg_pool2d(torch.rand((1, C, CASE + 4, CASE + 4), generator=g), 5, 1)[0] * 255).to(torch.uint8)
        f = torch.nn.functional.avg_pool2d(torch.randn((1, 1, CASE + 32, CASE + 32), generator=g), 33, 1)[0, 0]
        seg = torch.bucketize(f / f.std(), torch.linspace(-1.2, 1.2, N_HEADS - 1)).to(torch.uint8)
        cases.append((img, seg.numpy()))
    return nd.CaseStore(cases, ["ZScoreNormalization"] * C, N_HEADS, device)


def worst_tables(rng, store, lowres=False):
    s, ch = nd.draw_batch(rng, store, B, PATCH)
    if lowres:
        ch["lowres_zoom"] = np.linspace(0.5, 0.99, B * C, dtype=np.float32).reshape(B, C)
    loader_patch = nd.initial_patch_size(PATCH)
    for b in range(B):
        s[b]["m"], s[b]["copy"] = nd.spatial_matrix(PATCH, loader_patch, (200, 180), 0.3 + 0.2 * b, 0.7 + 0.05 * b, (b % 2 == 0, b % 3 == 0), True)
    s["noise_sigma"] = 0.05
    ch["blur_sigma"], ch["brightness"], ch["contrast"], ch["gamma_inverted"], ch["gamma"] = 1.0, 1.1, 1.2, 0.8, 1.4
    return s, ch


def device_ms(store, tables, warmup, lowres=False):
    ws = None
    times = []
    for i, (s, ch) in enumerate(tables):
        s_dev, c_dev = nd.upload_tables(s, ch, store.arena.device)
        torch.cuda.synchronize()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        data, _ = nd.sample_patches(store, s_dev, B, PATCH, SCALES)
        e[1].record()
        if ws is None:
            need = int(_lib.load().ldiff_op_seg_intensity_lr_ws_bytes(B, C, *PATCH)) if lowres else data.numel() * 4
            ws = torch.empty(need, dtype=torch.uint8, device=data.device)
        nd.augment_intensity_(data, s_dev, c_dev, 0, workspace=ws, lowres=lowres)
        e[2].record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append((e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])))
    return {"sample_ms": statistics.median(t[0] for t in times), "intensity_ms": statistics.median(t[1] for t in times),
            "total_ms": statistics.median(t[0] + t[1] for t in times), "total_max_ms": max(t[0] + t[1] for t in times)}


def numpy_sample(args):
    """One sample the way the CPU pipeline runs it: scipy's map_coordinates / gaussian_filter, numpy for the rest, float32."""
    import scipy.ndimage as ndi
    raw, seg, s, ch, seed = args
    h, w = PATCH
    rng = np.random.default_rng(seed)
    m = s["m"].astype(np.float64)
    i, j = np.mgrid[:h, :w].astype(np.float32)
    y, x = m[0] * i + m[1] * j + m[2], m[3] * i + m[4] * j + m[5]
    if s["copy"]:
        yi, xi = y.astype(np.int64), x.astype(np.int64)
        ok = (yi >= 0) & (yi < raw.shape[1]) & (xi >= 0) & (xi < raw.shape[2])
        data = np.where(ok, raw[:, yi.clip(0, raw.shape[1] - 1), xi.clip(0, raw.shape[2] - 1)], 0).astype(np.float32)
        lab = np.where(ok, seg[yi.clip(0, seg.shape[0] - 1), xi.clip(0, seg.shape[1] - 1)], 0)
    else:
        data = np.stack([ndi.map_coordinates(raw[c], [y, x], order=3, mode="constant", cval=0.0) for c in range(C)]).astype(np.float32)
        lab = np.zeros((h, w), np.uint8)
        for c in range(1, N_HEADS):
            lab[ndi.map_coordinates((seg == c).astype(np.float32), [y, x], order=1, mode="constant", cval=0.0) >= 0.5] = c
    if s["noise_sigma"] > 0:
        data += rng.normal(0, s["noise_sigma"], data.shape).astype(np.float32)
    for c in range(C):
        p, r = data[c], ch[c]
        if r["blur_sigma"] > 0:
            p = ndi.gaussian_filter(p, float(r["blur_sigma"]))
        if r["brightness"] != 1:
            p = p * r["brightness"]
        if r["contrast"] > 0:
            mn, lo, hi = p.mean(), p.min(), p.max()
            p = np.clip((p - mn) * r["contrast"] + mn, lo, hi)
        for g, inv in ((r["gamma_inverted"], True), (r["gamma"], False)):
            if g > 0:
                p = -p if inv else p
                mn, sd, lo = p.mean(), p.std(), p.min()
                rnge = p.max() - lo
                p = np.power((p - lo) / (rnge + 1e-7), g) * rnge + lo
                p = p - p.mean()
                p = p / (p.std() + 1e-8) * sd + mn
                p = -p if inv else p
        data[c] = p
    targets = [lab[(1 << k) >> 1::1 << k, (1 << k) >> 1::1 << k] for k in range(SCALES)]
    return data, targets


def numpy_ms(store, tables, threads=16):
    raws = [store.raw(i).cpu().numpy() for i in range(len(store))]
    segs = [store.labels(i).cpu().numpy() for i in range(len(store))]
    times = []
    with ThreadPoolExecutor(threads) as ex:
        for s, ch in tables:
            t0 = time.perf_counter()
            list(ex.map(numpy_sample, [(raws[int(s[b]["case_index"])], segs[int(s[b]["case_index"])], s[b], ch[b], b) for b in range(B)]))
            times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--lowres", action="store_true", help="also time the chain with the low-resolution simulation")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    t0 = time.perf_counter()
    store = make_store("cuda:0")
    out = {"shape": {"B": B, "C": C, "patch": PATCH, "scales": SCALES, "case": CASE, "cases": N_CASES}, "store_build_s": round(time.perf_counter() - t0, 2),
           "arena_MB": round(store.arena.numel() / 2 ** 20, 1)}
    rng = np.random.default_rng(1)
    n = args.batches + args.warmup
    worst = [worst_tables(rng, store) for _ in range(n)]
    expected = [nd.draw_batch(rng, store, B, PATCH) for _ in range(n)]
    out["worst"] = device_ms(store, worst, args.warmup)
    out["expected"] = device_ms(store, expected, args.warmup)
    if args.lowres:
        out["worst_lowres"] = device_ms(store, [worst_tables(rng, store, True) for _ in range(n)], args.warmup, True)
        out["expected_lowres"] = device_ms(store, [nd.draw_batch(rng, store, B, PATCH, lowres=True) for _ in range(n)], args.warmup, True)
    loader = nd.PatchLoader(store, PATCH, B, SCALES, seed=2, lowres=args.lowres)
    for _ in range(args.warmup):
        next(loader)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.batches):
        next(loader)
    out["host_ms_per_batch"] = round((time.perf_counter() - t0) * 1e3 / args.batches, 3)
    torch.cuda.synchronize()
    out["loader_ms_per_batch_with_device"] = round((time.perf_counter() - t0) * 1e3 / args.batches, 3)
    if not args.no_numpy:
        try:
            out["numpy_16_threads_ms"] = {"worst": round(numpy_ms(store, worst[:3]), 1), "expected": round(numpy_ms(store, expected[:6]), 1)}
        except ImportError as e:
            out["numpy_16_threads_ms"] = f"skipped: {e}"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
