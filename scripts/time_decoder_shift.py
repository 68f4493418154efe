"""Decoder time at the benchmark's shape (SD-1.5 width, B = 8, 512 x 512, decoder mode 0) with range shift k = 0 against k = K, alternating on one box.

    python scripts/time_decoder_shift.py [--k 4] [--rounds 5] [--iters 10]

Prints per round the median decode time of each k and, at the end, the median ratio.  Healthy synthetic weights: both decode the same image."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ldiffusion_amd import configs, weights  # noqa: E402
from ldiffusion_amd.models import AutoencoderKL  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    args = ap.parse_args()
    vcfg = configs.SD15_VAE
    vae = AutoencoderKL(vcfg, weights.synthetic_state_dict(weights.vae_param_shapes(vcfg), 43, fp16_values=True), "cuda:0")
    vae.set_precision(2, 0)
    z = (torch.randn((args.batch, 4, 64, 64), generator=torch.Generator().manual_seed(0)) * 0.3).cuda()
    luma = torch.empty((args.batch, 1, 512, 512), dtype=torch.uint8, device="cuda")

    def timed(k):
        vae.set_range_shift(k)
        for _ in range(2):
            vae._decode(z, 1 / 0.18215, want_rgb=True, luma=luma)
        ts = []
        for _ in range(args.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            vae._decode(z, 1 / 0.18215, want_rgb=True, luma=luma)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        vae.check_finite()
        return statistics.median(ts)

    ratios = []
    for r in range(args.rounds):
        a, b = (timed(0), timed(args.k)) if r % 2 == 0 else tuple(reversed((timed(args.k), timed(0))))
        ratios.append(b / a)
        print(f"round {r}: k=0 {a:.3f} ms, k={args.k} {b:.3f} ms, ratio {b / a:.4f}", flush=True)
    print(f"median ratio k={args.k} / k=0: {statistics.median(ratios):.4f} (min {min(ratios):.4f}, max {max(ratios):.4f})")


if __name__ == "__main__":
    main()
