"""Weight + bias gradient of one 3 x 3 conv (32 -> 32 channels by default) on the two routes of autograd.Conv2dFn, "staged" (transpose + im2col_t + GEMM over
K = M, colsum) and "direct" (ldiff_op_conv_wgrad, ldiff_op_colsum_slabs), over a range of M = B H W: the crossover behind autograd.WGRAD_DIRECT_MIN_ROWS.
The two routes alternate; device time per backward by HIP events, median of --passes.  Nothing is asserted.

usage: python scripts/bench_wgrad_routes.py [--channels 32] [--passes 20] [--sizes 32,64,96,128,192,256,512]
       python scripts/bench_wgrad_routes.py --wide [--passes 20]     "staged" against "wide" (ldiff_op_conv_wgrad_wide) on the trainer's wide layers, at the
                                                                     trainer's M and at M = 12288, 3072, 768: the table behind autograd.WGRAD_WIDE_MIN_ROWS
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ldiffusion_amd import autograd as ag  # noqa: E402


# The layers of the tissue-head trainer at the planner's width (7 stages, 512^2, B = 12) with M >= 16384 that ldiff_op_conv_wgrad refuses:
# (name, Cin, Cout, k, stride, output edge at the trainer's size; 0 = a linear over M rows)
WIDE_LAYERS = [("enc 64->128 s2", 64, 128, 3, 2, 128), ("enc/dec 128->128", 128, 128, 3, 1, 128), ("enc 128->256 s2", 128, 256, 3, 2, 64), ("enc/dec 256->256", 256, 256, 3, 1, 64),
               ("dec 256->128", 256, 128, 3, 1, 128), ("dec 512->256", 512, 256, 3, 1, 64), ("tconv 128->4*64", 128, 256, 1, 1, 0), ("tconv 256->4*128", 256, 512, 1, 1, 0),
               ("head 256->8", 256, 8, 1, 1, 64)]
WIDE_TRAINER_M = {"tconv 128->4*64": 196608, "tconv 256->4*128": 49152}
ROUTES3 = ("staged", "direct", "wide")
WIDE_EDGES = (32, 16, 8)   # B = 12: M = 12288, 3072, 768 -- the 512-channel stages' maps, where the staged GEMM's K is short


def bench_wide(a):
    """staged against wide per layer of WIDE_LAYERS, at the trainer's M and at M = 12288, 3072, 768: the table behind autograd.WGRAD_WIDE_MIN_ROWS.  "direct" runs
    beside them: for these layers it is the staged weight gradient with the slab column sum, what "auto" gives them from WGRAD_DIRECT_MIN_ROWS on, so the
    weight gradient's share of the gain is wide against direct."""
    dev, B = "cuda:0", 12
    g = torch.Generator().manual_seed(0)
    print(f"weight + bias gradient, B = {B}, device time per backward in us: median [min .. max] of {a.passes}, the routes alternating; "
          f"wide wins = the smaller median of staged and direct - wide median > the largest (max - min) of the three")
    for name, Cin, Cout, k, stride, edge in WIDE_LAYERS:
        w = (0.05 * torch.randn((Cout, Cin, k, k), generator=g)).to(dev).requires_grad_(True)
        b = torch.zeros(Cout, device=dev).requires_grad_(True)
        for e in (edge,) + WIDE_EDGES:
            if e == 0:
                M = WIDE_TRAINER_M[name]
                shape_x = (1, 1, M, Cin)
            elif name.startswith("tconv"):
                M = B * e * e
                shape_x = (1, 1, M, Cin)
            else:
                shape_x = (B, e * stride, e * stride, Cin)
            x = torch.randn(shape_x, generator=g).to(torch.float16).to(dev)
            nodes = {}
            for route in ROUTES3:
                with ag.wgrad_route(route):
                    nodes[route] = ag.Conv2dFn.apply(x, w, b, stride, 0)
            dy = (0.1 * torch.randn(tuple(nodes["wide"].shape), generator=g)).to(torch.float16).to(dev)
            M = dy.numel() // dy.shape[-1]
            times = {r: [] for r in ROUTES3}
            for i in range(a.passes + 2):
                for route in ROUTES3:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    torch.autograd.grad(nodes[route], (w, b), dy, retain_graph=True)
                    e1.record()
                    e1.synchronize()
                    if i >= 2:
                        times[route].append(e0.elapsed_time(e1) * 1e3)
            med = {r: statistics.median(t) for r, t in times.items()}
            spread = max(max(t) - min(t) for t in times.values())
            verdict = "wide" if min(med["staged"], med["direct"]) - med["wide"] > spread else "staged"
            print(f"  {name:<18} k={k} s={stride} M = {M:>7}: " + "   ".join(f"{r} {med[r]:9.1f} [{min(t):9.1f} .. {max(t):9.1f}]" for r, t in times.items())
                  + f"   staged / wide = {med['staged'] / med['wide']:6.2f}   direct / wide = {med['direct'] / med['wide']:6.2f}   -> {verdict}", flush=True)
            del nodes, x, dy
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--sizes", default="32,64,96,128,192,256,512")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--wide", action="store_true", help="the wide layers of the tissue-head trainer: staged against wide (autograd.WGRAD_WIDE_MIN_ROWS)")
    a = ap.parse_args()
    if a.wide:
        return bench_wide(a)
    dev, Cc, B = "cuda:0", a.channels, a.batch
    g = torch.Generator().manual_seed(0)
    w = (0.05 * torch.randn((Cc, Cc, 3, 3), generator=g)).to(dev).requires_grad_(True)
    b = torch.zeros(Cc, device=dev).requires_grad_(True)
    print(f"3 x 3 conv {Cc} -> {Cc}, B = {B}: weight + bias gradient, device time per backward (median [min .. max] of {a.passes}, the routes alternating)")
    for size in (int(s) for s in a.sizes.split(",")):
        x = torch.randn((B, size, size, Cc), generator=g).to(torch.float16).to(dev)
        dy = (0.1 * torch.randn((B, size, size, Cc), generator=g)).to(torch.float16).to(dev)
        nodes = {}
        for route in ("staged", "direct"):
            with ag.wgrad_route(route):
                nodes[route] = ag.Conv2dFn.apply(x, w, b, 1, 0)
        times = {"staged": [], "direct": []}
        for i in range(a.passes + 3):
            for route in ("staged", "direct"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                torch.autograd.grad(nodes[route], (w, b), dy, retain_graph=True)
                e1.record()
                e1.synchronize()
                if i >= 3:
                    times[route].append(e0.elapsed_time(e1) * 1e3)
        s, d = statistics.median(times["staged"]), statistics.median(times["direct"])
        band = {r: f"[{min(t):9.1f} .. {max(t):9.1f}]" for r, t in times.items()}
        print(f"  M = {B * size * size:>8} ({B} x {size}^2): staged {s:10.1f} {band['staged']} us   direct {d:10.1f} {band['direct']} us   staged / direct = {s / d:6.2f}", flush=True)


if __name__ == "__main__":
    main()
