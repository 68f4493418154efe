"""Wall time to build a `nnunet_data.CaseStore` of N synthetic 1024^2 RGB cases (uint8 images with a black frame, 7 classes), on one box, from the same
process: the host build (normalise on the CPU, np.argwhere per class; the path every earlier commit has) against `build="device"` (the ldiff_op_case_*
kernels), each with the spline prefilter on the host and on the device.  The cases start in host memory, as a PNG reader leaves them; every row ends with a
device synchronisation.  The first device build of a process also pays the library's load and is reported apart (`warm-up`).

    python scripts/bench_nnunet_prep.py [--cases 8] [--repeats 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ldiffusion_amd import nnunet_data as nd  # noqa: E402

C, CASE, N_HEADS = 3, 1024, 7


def make_cases(n):
    g = torch.Generator().manual_seed(0)
    cases = []
    for _ in range(n):
        img = (torch.nn.functional.avg_pool2d(torch.rand((1, C, CASE + 4, CASE + 4), generator=g), 5, 1)[0] * 254 + 1).to(torch.uint8)
        img[:, :8], img[:, :, -5:] = 0, 0          # a frame the device build crops away
        f = torch.nn.functional.avg_pool2d(torch.randn((1, 1, CASE + 32, CASE + 32), generator=g), 33, 1)[0, 0]
        seg = torch.bucketize(f / f.std(), torch.linspace(-1.2, 1.2, N_HEADS - 1)).to(torch.uint8)
        cases.append((img, seg))
    return cases


def timed(fn, repeats):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        store = fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
        del store
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    cases = make_cases(args.cases)
    schemes = ["ZScoreNormalization"] * C
    t0 = time.perf_counter()
    nd.CaseStore(cases[:1], schemes, N_HEADS, "cuda:0", build="device", prefilter="device")
    torch.cuda.synchronize()
    rows = {"warm-up (one case, device build, first call of the process)": [time.perf_counter() - t0]}
    for name, kw in (("host build, host prefilter (the default)", dict(build="host", prefilter="host")),
                     ("host build + crop, device prefilter", dict(build="host", crop=True, prefilter="device")),
                     ("device build, host prefilter", dict(build="device", prefilter="host")),
                     ("device build, device prefilter", dict(build="device", prefilter="device"))):
        rows[name] = timed(lambda kw=kw: nd.CaseStore(cases, schemes, N_HEADS, "cuda:0", **kw), args.repeats)
    for name, t in rows.items():
        print(f"{name:70s} median {statistics.median(t) * 1e3:10.1f} ms   min {min(t) * 1e3:10.1f} ms   ({len(t)} runs, {args.cases} cases)")
    print(json.dumps({"cases": args.cases, "case": [C, CASE, CASE], "seconds": {k: v for k, v in rows.items()}}))


if __name__ == "__main__":
    main()
