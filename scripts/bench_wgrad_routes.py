"""Weight + bias gradient of one 3 x 3 conv (32 -> 32 channels by default) on the two routes of autograd.Conv2dFn, "staged" (transpose + im2col_t + GEMM over
K = M, colsum) and "direct" (ldiff_op_conv_wgrad, ldiff_op_colsum_slabs), over a range of M = B H W: the crossover behind autograd.WGRAD_DIRECT_MIN_ROWS.
The two routes alternate; device time per backward by HIP events, median of --passes.  Nothing is asserted.

usage: python scripts/bench_wgrad_routes.py [--channels 32] [--passes 20] [--sizes 32,64,96,128,192,256,512]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ldiffusion_amd import autograd as ag  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--sizes", default="32,64,96,128,192,256,512")
    ap.add_argument("--batch", type=int, default=1)
    a = ap.parse_args()
    dev, Cc, B = "cuda:0", a.channels, a.batch
    g = torch.Generator().manual_seed(0)
    w = (0.05 * torch.randn((Cc, Cc, 3, 3), generator=g)).to(dev).requires_grad_(True)
    b = torch.zeros(Cc, device=dev).requires_grad_(True)
    print(f"3 x 3 conv {Cc} -> {Cc}, B = {B}: weight + bias gradient, device time per backward (median of {a.passes}, the routes alternating)")
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
        print(f"  M = {B * size * size:>8} ({B} x {size}^2): staged {s:10.1f} us   direct {d:10.1f} us   staged / direct = {s / d:6.2f}")


if __name__ == "__main__":
    main()
