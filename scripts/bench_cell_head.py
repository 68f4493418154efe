"""The cell head's instance classifier (ldiff_resnet, models.ResNetClassifier: ResNet152 trunk + adapter + linear head) against what a user had before it
existed: the same network as torch.nn modules under torch.autocast(fp16), channels-last, on the same GPU.  B = 16, 256 and 1024 crops of 64^2, graphs on;
then `CellSegClassifier.predict_mask` on a 1024^2 image with about 400 instances (boxes, crops, classifier in chunks of 256, painting).

The two sides alternate inside one call after a warm-up, --passes timed passes each (device-synchronised wall time per pass; median, min, max); then one
profiled pass prints the per-launch table (ldiff_prof_*).

usage: python scripts/bench_cell_head.py [--passes 20] [--batches 16,256,1024]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch import nn  # noqa: E402

from ldiffusion_amd import _lib, cellhead  # noqa: E402
from ldiffusion_amd.models import ResNetClassifier  # noqa: E402

LAYERS, WIDTH, ADAPTER, NC = cellhead.RESNET152_LAYERS, 64, 256, 5


class Bottleneck(nn.Module):
    def __init__(self, inplanes, planes, stride, down):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(inplanes, planes, 1, bias=False), nn.BatchNorm2d(planes)
        self.conv2, self.bn2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False), nn.BatchNorm2d(planes)
        self.conv3, self.bn3 = nn.Conv2d(planes, 4 * planes, 1, bias=False), nn.BatchNorm2d(4 * planes)
        self.downsample = nn.Sequential(nn.Conv2d(inplanes, 4 * planes, 1, stride, bias=False), nn.BatchNorm2d(4 * planes)) if down else None

    def forward(self, x):
        out = F.relu(self.bn1(self.conv1(x)))
        out = F.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return F.relu(out + (x if self.downsample is None else self.downsample(x)))


class TorchClassifier(nn.Module):
    """The restatement a user would write (tests/test_cpu_cellhead.py checks the same wiring against tests/resnet_ref.py)."""

    def __init__(self):
        super().__init__()
        mods = [nn.Conv2d(3, WIDTH, 7, 2, 3, bias=False), nn.BatchNorm2d(WIDTH), nn.ReLU(), nn.MaxPool2d(3, 2, 1)]
        inplanes = WIDTH
        for li, n in enumerate(LAYERS):
            blocks = []
            for b in range(n):
                blocks.append(Bottleneck(inplanes, WIDTH << li, 2 if (b == 0 and li > 0) else 1, b == 0))
                inplanes = 4 * (WIDTH << li)
            mods.append(nn.Sequential(*blocks))
        self.encoder = nn.Sequential(*mods)
        self.adapter = nn.Conv2d(inplanes, ADAPTER, 3, padding=1)
        self.classifier = nn.Linear(ADAPTER, NC)

    def forward(self, x):
        return self.classifier(F.adaptive_avg_pool2d(self.adapter(self.encoder(x)), (1, 1)).flatten(1))


def timed_pass(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def fmt(v):
    return f"median {statistics.median(v):.3f} ms (min {min(v):.3f}, max {max(v):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--batches", default="16,256,1024")
    a = ap.parse_args()
    import resnet_ref
    dev = "cuda:0"
    sd = resnet_ref.synthetic_state_dict(LAYERS, WIDTH, NC, 13)
    net = ResNetClassifier(NC, sd, dev)
    tnet = TorchClassifier()
    tnet.load_state_dict(sd, strict=False)
    tnet = tnet.to(dev).eval().to(memory_format=torch.channels_last)
    lib = _lib.load()
    gmac = 0.0
    for B in [int(b) for b in a.batches.split(",")]:
        x = torch.randn((B, 3, 64, 64), generator=torch.Generator().manual_seed(1))
        xl = resnet_ref.to_nhwc8(x).to(dev)
        xt = x.to(dev).contiguous(memory_format=torch.channels_last)

        def run_lib():
            net(xl)

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
        print(f"B={B} crops of 64^2, {a.passes} alternating passes: library {fmt(tl)} | torch.nn under autocast(fp16), channels-last {fmt(tt)} | "
              f"library / torch = {statistics.median(tl) / statistics.median(tt):.3f} (graph replays so far: {net.graph_replays})", flush=True)
        lib.ldiff_prof_set_filter(None)
        _lib.prof_collect()
        lib.ldiff_prof_enable(1)
        run_lib()
        torch.cuda.synchronize()
        lib.ldiff_prof_enable(0)
        prof = sorted(_lib.prof_collect(), key=lambda r: -r["ms"])
        tot = sum(r["ms"] for r in prof)
        gmac = sum(r["flops"] for r in prof) / 2e9 / B
        print(f"  per-launch table of one eager pass under the profiler (sum {tot:.3f} ms, {sum(r['launches'] for r in prof)} profiled launches, {gmac:.3f} GMAC per crop):")
        for r in prof:
            print(f"    {r['name']:<30} x{r['launches']:<4} {r['ms']:8.3f} ms  {r['flops'] / max(r['ms'], 1e-9) / 1e9:8.1f} TFLOP/s  {r['bytes'] / 1e6:9.1f} MB", flush=True)

    # predict_mask: a 1024^2 image with about 400 instances on a 20 x 20 grid (discs and rectangles of 12 .. 44 pixels)
    rng = np.random.default_rng(2)
    labels = np.zeros((1024, 1024), np.int64)
    yy, xx = np.mgrid[:1024, :1024]
    k = 1
    for gy in range(20):
        for gx in range(20):
            cy, cx, r = 26 + gy * 51, 26 + gx * 51, int(rng.integers(6, 23))
            if (gy + gx) % 2:
                labels[cy - r:cy + r, cx - r:cx + r] = k
            else:
                labels[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = k
            k += 1
    head = cellhead.CellSegClassifier(NC, sd, dev, instances=lambda image: labels)
    rgb = torch.from_numpy(rng.integers(0, 256, (1024, 1024, 3), dtype=np.uint8)).to(dev)
    lab = torch.from_numpy(labels).to(dev)
    for _ in range(3):
        head.predict_mask(rgb, lab)
    tp = [timed_pass(lambda: head.predict_mask(rgb, lab)) for _ in range(a.passes)]
    tb = [timed_pass(lambda: cellhead.instance_boxes(lab)) for _ in range(a.passes)]
    ids, boxes = cellhead.instance_boxes(lab)
    tc = [timed_pass(lambda: head.crops(rgb, boxes)) for _ in range(a.passes)]
    head.net.check_finite()
    print(f"predict_mask, 1024^2 image, {ids.numel()} instances (label map on the device): {fmt(tp)}; of it instance_boxes {fmt(tb)}, crop_resize_norm {fmt(tc)}")


if __name__ == "__main__":
    main()
