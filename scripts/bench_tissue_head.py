"""The nnU-Net tissue head (ldiff_segnet, models.PlainConvUNet) against what a user had before it existed: the same network as torch.nn modules under
torch.autocast(fp16), handed to Segmentor.inference_tissue_model_nnUNetv2 as `predictor=`.  Planner-default width (7 stages, 32 .. 512 features, two
convs per stage, tests/golden/nnunet_plans_2d.json "2d"), at 512^2 and the largest patch the fixture plans name, B = 1 and 4, graphs on.

The two sides alternate inside one call after a warm-up, --passes timed passes each (device-synchronised wall time per pass; median, min, max); then one
profiled pass prints the per-launch list (ldiff_prof_*), and for the head's own kernels bytes / time against the 8 TB/s bench.py uses.

usage: python scripts/bench_tissue_head.py [--passes 50] [--sizes 512] [--batches 1,4]
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
from torch import nn  # noqa: E402

from ldiffusion_amd import _lib, nnunet  # noqa: E402
from ldiffusion_amd.models import PlainConvUNet  # noqa: E402

HBM = 8.0e12


def shapes_account(spec, size):
    """MACs and activation bytes of one pass at B = 1 from the shapes alone: (total GMAC, rows of (layer, Cin, Cout, H_out, MAC, bytes read + written))."""
    f, n = spec["features"], spec["n_stages"]
    rows, h = [], size
    for s in range(n):
        cin = spec["in_channels"] if s == 0 else f[s - 1]
        for i in range(spec["n_conv_encoder"][s]):
            hin = h
            if i == 0:
                h //= spec["strides"][s]
            rows.append((f"enc{s}.{i}", cin, f[s], h, 9 * cin * f[s] * h * h, 2 * (max(cin, 8) * hin * hin + f[s] * h * h)))
            cin = f[s]
    for j in range(n - 1):
        below, skip = f[n - 1 - j], f[n - 2 - j]
        rows.append((f"up{j}", below, skip, 2 * h, below * skip * 4 * h * h, 2 * (below * h * h + skip * 4 * h * h)))
        h *= 2
        cin = 2 * skip
        for i in range(spec["n_conv_decoder"][j]):
            rows.append((f"dec{j}.{i}", cin, skip, h, 9 * cin * skip * h * h, 2 * (cin + skip) * h * h))
            cin = skip
    rows.append(("head", f[0], spec["n_heads"], h, f[0] * spec["n_heads"] * h * h, 2 * f[0] * h * h + 4 * spec["n_heads"] * h * h))
    return sum(r[4] for r in rows) / 1e9, rows


class Block(nn.Sequential):
    def __init__(self, cin, cout, stride):
        super().__init__(nn.Conv2d(cin, cout, 3, stride, 1), nn.InstanceNorm2d(cout, eps=1e-5, affine=True), nn.LeakyReLU(0.01, inplace=True))


class TorchPlainConvUNet(nn.Module):
    """The restatement a user would write (tests/test_cpu_nnunet.py checks the same wiring against tests/nnunet_ref.py)."""

    def __init__(self, spec):
        super().__init__()
        f, n = spec["features"], spec["n_stages"]
        self.enc = nn.ModuleList([nn.Sequential(*[Block((spec["in_channels"] if s == 0 else f[s - 1]) if i == 0 else f[s], f[s], spec["strides"][s] if i == 0 else 1)
                                                  for i in range(spec["n_conv_encoder"][s])]) for s in range(n)])
        self.up = nn.ModuleList([nn.ConvTranspose2d(f[n - 1 - j], f[n - 2 - j], 2, 2) for j in range(n - 1)])
        self.dec = nn.ModuleList([nn.Sequential(*[Block(2 * f[n - 2 - j] if i == 0 else f[n - 2 - j], f[n - 2 - j], 1) for i in range(spec["n_conv_decoder"][j])])
                                  for j in range(n - 1)])
        self.head = nn.Conv2d(f[0], spec["n_heads"], 1)

    def forward(self, x):
        skips = []
        for st in self.enc:
            x = st(x)
            skips.append(x)
        for j, (up, st) in enumerate(zip(self.up, self.dec)):
            x = st(torch.cat((up(x), skips[-(j + 2)]), 1))
        return self.head(x)


def timed_pass(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=50)
    ap.add_argument("--sizes", default="")
    ap.add_argument("--batches", default="1,4")
    a = ap.parse_args()
    import nnunet_ref
    with open(os.path.join(ROOT, "tests", "golden", "nnunet_plans_2d.json")) as f:
        plans = json.load(f)
    with open(os.path.join(ROOT, "tests", "golden", "nnunet_dataset.json")) as f:
        ds = json.load(f)
    spec = nnunet.network_spec(plans, "2d", ds)
    largest = max(max(c["patch_size"]) for c in plans["configurations"].values() if "patch_size" in c)
    sizes = [int(s) for s in a.sizes.split(",") if s] or sorted({512, largest})
    sd = nnunet_ref.synthetic_state_dict(spec, 27)
    dev = "cuda:0"
    net = PlainConvUNet(spec, sd, dev)
    tnet = TorchPlainConvUNet(spec).to(dev).eval()
    lib = _lib.load()
    for size in sizes:
        gmac, rows = shapes_account(spec, size)
        print(f"== {size}^2: {gmac:.1f} GMAC per tile from the shapes; 32 -> 32 at full resolution: {rows[1][4] * 2 / 1e9:.2f} GFLOP against {rows[1][5] / 1e6:.1f} MB; "
              f"a 1024^2 ROI at step 0.5 with both mirror axes = 9 tiles x 4 = {36 * shapes_account(spec, 512)[0] / 1e3:.2f} TMAC at 512^2 tiles")
        for B in [int(b) for b in a.batches.split(",")]:
            x = torch.randn((B, 3, size, size), generator=torch.Generator().manual_seed(1)).to(dev)

            def run_lib():
                net(x)

            def run_torch():
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                    tnet(x)

            for _ in range(5):
                run_lib(); run_torch()
            tl, tt = [], []
            for _ in range(a.passes):
                tl.append(timed_pass(run_lib))
                tt.append(timed_pass(run_torch))
            net.check_finite()
            f = lambda v: f"median {statistics.median(v):.3f} ms (min {min(v):.3f}, max {max(v):.3f})"
            print(f"B={B} {size}^2, {a.passes} alternating passes: library {f(tl)} | torch.nn under autocast(fp16) {f(tt)} | "
                  f"library / torch = {statistics.median(tl) / statistics.median(tt):.3f} (graph replays so far: {net.graph_replays})")
            lib.ldiff_prof_set_filter(None)
            _lib.prof_collect()
            lib.ldiff_prof_enable(1)
            run_lib()
            torch.cuda.synchronize()
            lib.ldiff_prof_enable(0)
            prof = sorted(_lib.prof_collect(), key=lambda r: -r["ms"])
            tot = sum(r["ms"] for r in prof)
            print(f"  per-launch list of one eager pass under the profiler (sum {tot:.3f} ms, {sum(r['launches'] for r in prof)} profiled launches):")
            for r in prof:
                line = f"    {r['name']:<28} x{r['launches']:<3} {r['ms']:8.3f} ms  {r['flops'] / max(r['ms'], 1e-9) / 1e9:8.1f} TFLOP/s"
                if r["name"].startswith(("segconv<", "tconv2x2<")) and r["ms"] > 0:
                    t_mem, t_mfma = r["bytes"] / HBM * 1e3, r["flops"] / 2.5e15 * 1e3
                    line += f"  {r['bytes'] / 1e6:8.1f} MB = {t_mem / r['ms'] * 100:5.1f} % of 8 TB/s ({'memory' if t_mem > t_mfma else 'matrix'} bound applies)"
                print(line)


if __name__ == "__main__":
    main()
