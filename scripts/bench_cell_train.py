"""A training-mode pass of the cell head's instance classifier (ldiff_resnet_forward_train, ResNetClassifier.forward_train: ResNet152 with batch statistics,
three launches per conv -- clsconv<...,bn>, bn_finalize, bn_apply) against what a user had before it existed: the same network as torch.nn modules in
`.train()` under torch.autocast(fp16), channels-last, no_grad (the reference's loop reaches no parameter with a gradient), on the same GPU.
B = 16, 256 and 1024 crops of 64^2.

The two sides alternate inside one call after a warm-up, --passes timed passes each (device-synchronised wall time per pass; median, min, max); then one
profiled pass prints the per-launch table (ldiff_prof_*).

usage: python scripts/bench_cell_train.py [--passes 20] [--batches 16,256,1024]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402

from bench_cell_head import ADAPTER, LAYERS, NC, WIDTH, TorchClassifier, fmt, timed_pass  # noqa: E402
from ldiffusion_amd import _lib  # noqa: E402
from ldiffusion_amd.models import ResNetClassifier  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--batches", default="16,256,1024")
    a = ap.parse_args()
    import resnet_ref
    dev = "cuda:0"
    sd = resnet_ref.synthetic_state_dict(LAYERS, WIDTH, NC, 13)
    net = ResNetClassifier(NC, sd, dev, LAYERS, WIDTH, ADAPTER, train=True)
    tnet = TorchClassifier()
    tnet.load_state_dict(sd, strict=False)
    tnet = tnet.to(dev).train().to(memory_format=torch.channels_last)
    lib = _lib.load()
    for B in [int(b) for b in a.batches.split(",")]:
        x = torch.randn((B, 3, 64, 64), generator=torch.Generator().manual_seed(1))
        xl = resnet_ref.to_nhwc8(x).to(dev)
        xt = x.to(dev).contiguous(memory_format=torch.channels_last)

        def run_lib():
            net.forward_train(xl)

        def run_torch():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                tnet(xt)

        for _ in range(3):
            run_lib(); run_torch()
        tl, tt = [], []
        for _ in range(a.passes):
            tl.append(timed_pass(run_lib))
            tt.append(timed_pass(run_torch))
        net.check_finite()
        print(f"B={B} crops of 64^2, {a.passes} alternating passes: library forward_train {fmt(tl)} | torch.nn .train() under autocast(fp16), channels-last {fmt(tt)} | "
              f"library / torch = {statistics.median(tl) / statistics.median(tt):.3f}", flush=True)
        lib.ldiff_prof_set_filter(None)
        _lib.prof_collect()
        lib.ldiff_prof_enable(1)
        run_lib()
        torch.cuda.synchronize()
        lib.ldiff_prof_enable(0)
        prof = sorted(_lib.prof_collect(), key=lambda r: -r["ms"])
        tot = sum(r["ms"] for r in prof)
        print(f"  per-launch table of one pass under the profiler (sum {tot:.3f} ms, {sum(r['launches'] for r in prof)} profiled launches):")
        for r in prof:
            print(f"    {r['name']:<30} x{r['launches']:<4} {r['ms']:8.3f} ms  {r['flops'] / max(r['ms'], 1e-9) / 1e9:8.1f} TFLOP/s  {r['bytes'] / 1e6:9.1f} MB", flush=True)


if __name__ == "__main__":
    main()
