"""What the ControlNet costs and what the fused hand-off saves, at SD-v1.5 width (synthetic weights), measured on the GPU:
  (a) each conditioning-embedding layer on the conditioning-embedding kernel (condconv<...>, SiLU in its epilogue) against the same layer as
      plan_conv routed it before that kernel existed (ldiff_conv_args.cond_conv = -1: the register-staged implicit GEMM) plus the separate
      ldiff_op_silu launch that route needs;
  (b) ControlNetModel.set_cond as a whole;
  (c) the UNet forward plain, attached (the ControlNet inside the forward, zero convs writing into the skip stack) and detached
      (stand-alone ControlNet forward + thirteen fp32 residual tensors through the UNet call).
HIP events around synchronised work, every shape warmed, the two sides of a comparison alternating inside one repeat, median and
min .. max over the repeats printed (the spread a difference has to beat).
usage: python scripts/bench_controlnet.py [--config b8|v7|both] [--repeats N] [--iters N] [--skip-unet]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from ldiffusion_amd import _lib, configs, weights
from ldiffusion_amd.models import ControlNetModel, UNet2DConditionModel

DEV = "cuda:0"
CONFIGS = {"b8": (8, 64, 64), "v7": (1, 32, 32)}   # (B, latent h, latent w); the conditioning image is 8 x that per side
LAYERS = [("conv_in", 8, 16, 1, 1), ("blocks.0", 16, 16, 1, 1), ("blocks.1", 16, 32, 2, 1), ("blocks.2", 32, 32, 1, 2), ("blocks.3", 32, 96, 2, 2),
          ("blocks.4", 96, 96, 1, 4), ("blocks.5", 96, 256, 2, 4)]   # (name, stored Cin, Cout, stride, input map = image / this)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def ab(sides, repeats, iters):
    """sides: {name: fn}.  Warm every side, then `repeats` rounds with the sides alternating inside a round -> {name: (median, min, max)} in ms."""
    for fn in sides.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in sides}
    for _ in range(repeats):
        for k, fn in sides.items():
            t[k].append(timed(fn, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def fmt(r):
    return f"{r[0] * 1e3:9.1f} us ({r[1] * 1e3:.1f} .. {r[2] * 1e3:.1f})"


def bench_layers(lib, B, H, W, repeats, iters):
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    print(f"(a) embedding layers, B = {B}, {H} x {W} conditioning image: new kernel (SiLU fused) | previous route (igemm + ldiff_op_silu) | ratio previous / new")
    g = torch.Generator().manual_seed(0)
    for name, cin, cout, stride, div in LAYERS:
        h, w = H // div, W // div
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        x = torch.randn((B, h, w, cin), generator=g).to(torch.float16).to(DEV)
        wt = (torch.randn((cout, 9 * cin), generator=g) * (1.0 / (9 * cin)) ** 0.5).to(torch.float16).to(DEV)
        bias = (torch.randn(cout, generator=g) * 0.1).to(DEV)
        y = torch.empty((B, ho, wo, cout), dtype=torch.float16, device=DEV)
        y2 = torch.empty_like(y)

        def args(silu, cond):
            a = _lib.ConvArgs()
            a.x, a.C1, a.B, a.Hin, a.Win, a.Hout, a.Wout = x.data_ptr(), cin, B, h, w, ho, wo
            a.ks, a.stride, a.pad_t, a.pad_l = 3, stride, 1, 1
            a.w, a.N, a.Nrows, a.n_real, a.bias = wt.data_ptr(), cout, cout, cout, bias.data_ptr()
            a.y, a.ldy, a.silu_out, a.cond_conv = y.data_ptr(), cout, silu, cond
            return a
        a_new, a_old = args(1, 1), args(0, -1)   # (1: the new kernel whatever the routing rule says about this layer)

        def new():
            _lib.check(lib.ldiff_op_conv(C.byref(a_new), sp))

        def old():
            _lib.check(lib.ldiff_op_conv(C.byref(a_old), sp))
            _lib.check(lib.ldiff_op_silu(C.c_void_p(y.data_ptr()), C.c_void_p(y2.data_ptr()), y.numel(), sp))
        lib.ldiff_prof_enable(1)
        new(); old()
        torch.cuda.synchronize()
        kern = sorted(r["name"] for r in _lib.prof_collect())
        lib.ldiff_prof_enable(0)
        r = ab({"new": new, "old": old}, repeats, iters)
        gf = 2.0 * B * ho * wo * cout * 9 * cin / 1e9
        print(f"  {name:9s} {cin:3d} -> {cout:3d} s{stride} {h:4d}x{w:<4d} {fmt(r['new'])} | {fmt(r['old'])} | {r['old'][0] / r['new'][0]:5.2f}x   "
              f"({gf / r['new'][0]:.0f} GFLOP/ms new; kernels {kern})")


def bench_models(unet, cn, B, h, w, repeats, iters, skip_unet):
    g = torch.Generator().manual_seed(1)
    x = torch.randn((B, 4, h, w), generator=g).to(DEV)
    ctx = (torch.randn((1, 77, 768), generator=g) * 0.5).to(DEV)
    conds = [torch.rand((B, 3, 8 * h, 8 * w), generator=g).to(DEV) for _ in range(2)]
    k = [0]

    def set_cond():   # a new image each time: the cache key changes, the embedding runs
        k[0] ^= 1
        conds[k[0]].add_(0)
        cn.set_cond(conds[k[0]])
    cn.set_context(ctx)
    r = ab({"set_cond": set_cond}, repeats, iters)
    print(f"(b) set_cond, B = {B}, {8 * h} x {8 * w}: {fmt(r['set_cond'])}")
    if skip_unet:
        return
    cond = conds[0]

    def plain():
        unet(x, 501, ctx)

    def attached():
        unet(x, 501, ctx, controlnet_cond=cond)

    def detached():
        down, mid = cn(x, 501, ctx, cond, return_dict=False)
        unet(x, 501, ctx, down_block_additional_residuals=down, mid_block_additional_residual=mid)
    # the graph cache holds one configuration: alternating attached / plain inside a round would re-capture every time, so each mode gets its own rounds
    res = {}
    for name, fn, att in (("plain", plain, False), ("attached", attached, True), ("detached", detached, False), ("plain again", plain, False), ("attached again", attached, True)):
        if att:
            unet.attach_controlnet(cn)
        else:
            unet.detach_controlnet()
        res[name] = ab({name: fn}, repeats, iters)[name]
    unet.detach_controlnet()
    print(f"(c) UNet forward, B = {B}, {h} x {w} latents (graph replay where the path allows it; the detached path runs eagerly):")
    for name, v in res.items():
        print(f"  {name:15s} {v[0]:8.3f} ms ({v[1]:.3f} .. {v[2]:.3f})")
    p, a, d = res["plain"][0], res["attached"][0], res["detached"][0]
    print(f"  attached / plain = {a / p:.2f} (two plain passes = 2.00); detached / attached = {d / a:.2f}; graph nodes of the attached forward {unet.graph_nodes}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="both", choices=["b8", "v7", "both"])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--skip-unet", action="store_true")
    a = ap.parse_args()
    _lib.require_gpu()
    lib = _lib.load()
    print(f"device: {torch.cuda.get_device_name(0)}; library version {lib.ldiff_version()}")
    names = ["b8", "v7"] if a.config == "both" else [a.config]
    for n in names:
        B, h, w = CONFIGS[n]
        bench_layers(lib, B, 8 * h, 8 * w, a.repeats, a.iters)
    ucfg, ccfg = configs.SD15_UNET, configs.SD15_CONTROLNET
    cn = ControlNetModel(ccfg, weights.synthetic_state_dict(weights.controlnet_param_shapes(ccfg), 44, fp16_values=True), DEV)
    unet = None if a.skip_unet else UNet2DConditionModel(ucfg, weights.synthetic_state_dict(weights.unet_param_shapes(ucfg), 42, fp16_values=True), DEV)
    for n in names:
        B, h, w = CONFIGS[n]
        bench_models(unet, cn, B, h, w, a.repeats, max(3, a.iters // 4), a.skip_unet)


if __name__ == "__main__":
    main()
