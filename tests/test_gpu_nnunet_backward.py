"""-m gpu: the backward pass of the tissue-head trainer (ldiffusion_amd/nnunet_train.py) layer by layer -- every autograd.Conv2dFn signature of one
TrainableSegNet step, the transposed-conv path, and the staged weight gradient at a long K -- each output per element against float64 on exactly the
operands the kernels see.  tests/test_gpu_nnunet_train.py grades the same step as a whole, by one figure per parameter tensor; this file is what sees a
wrong element.

Error model: that of tests/test_gpu_backward.py (u = 2^-24, gamma(K) = 2 K u, an fp16 output's own 2^-11), whose conv_reference, check_bound and gamma are
imported, not restated.  Where "auto" sent a case to the direct weight gradient / the slab column sum (M = B Ho Wo >= ag.WGRAD_DIRECT_MIN_ROWS), dw / db
are held to tests/wgrad_bound.py's (chain + partials + 2) u sum |dy x| with the plan ag.wgrad_plan / ag.colsum_slabs_plan states for the launch.  The
transposed conv's terms are derived in tests/nnunet_step_sigs.py.  Nothing here is fitted to what the kernels return.

  a. NNUNET_CASES: one case per signature of `2d_reduced` at 2 x 64 x 64 (the whole-step test's shape) and of `2d` at 2 x 128 x 128 (the smallest square at
     which all seven stages, the 512-wide ones included, have a 2 x 2 map; its top level has M = 32768 and takes the direct route, the rest the staged
     one, as in the real step), plus the shapes the route census asked for.  y, dx, dw, db; the wrong references of conv_reference (last live K block, two
     taps swapped) must break the bound; pad columns zero; the kernel of each role is stated.
  b. TrainableSegNet.tconv itself on a one-layer parameter dict for every decoder.transpconvs.* shape of both specs on 2 x (4 x 4), 2 x (16 x 16) and
     1 x (5 x 7) maps: y, dx, weight.grad [ci, co, di, dj] and bias.grad; di / dj exchanged and a one-sub-pixel bias gradient must break the bound.
  c. LONGK_CASES under wgrad_route("staged"): integer data in [-3, 3] must give dw and db bit for bit (twice), random data (tests/wgrad_bound.py random_case:
     same-sign terms, so that a missing row range shows against the magnitude sum) must stay within gamma(Mpad); the wrong reference leaves out the last 64
     rows where the bound sees that, else the last K / 16 rows.  The staged GEMM writes fp32 and plan_conv plans no split-K for an fp32 output
     (csrc/conv_route.hip: `ask.splitk == 0 && !q.out_f32`), so at every K here it is ONE K loop of gemm_dma<64,64> over all the rows: what these cases
     guard is that loop's and im2col_t's row range, not a split's placement.
  d. One eager Trainer step per spec with Conv2dFn.apply / InstanceNormLReLUFn.apply wrapped: every signature seen is one nnunet_step_sigs lists and has a
     case.  And the route census: every signature of the real configuration (`2d`, B = 12, 512 x 512) runs once per role on device-made random data; the
     kernel each role reaches must be one a case of (a) - (c) pins in that role.

Measured on an MI355X: see MEASURED below and DESIGN.md section 7 "Tissue head, backward per layer".  With the zero insertion's stride removed from
Conv2dFn.backward the eleven stride-2 cases of (a) fail (dx); with permute(3, 2, 1, 0) in tconv all fifteen cases of (b) fail; with a split-K reduce that drops its
last split 22 cases of (a) and the six 512-wide cases of (b) fail, through y and dx of the split forward / dgrad launches.
"""
import json
import math
import os
import time

import numpy as np
import pytest
import torch

import nnunet_step_sigs as ns
import nnunet_train_ref as tref
import test_gpu_backward as tb
import wgrad_bound as wb
from kernel_routing import check_route, reached
from ldiffusion_amd import autograd as ag, nnunet, nnunet_train, train
from test_gpu_backward import check_bound, conv_reference, gamma

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U, H16 = tb.U, tb.H16
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
PARITY_SHAPES = {"2d_reduced": (2, 64, 64), "2d": (2, 128, 128)}
REAL_SHAPE = ("2d", (12, 512, 512))

# Worst error / bound per group as teardown_module prints them, measured on an MI355X (DESIGN.md section 7 has the date, the commit and the census table); a record, not
# asserted: the assertions are the bounds themselves.  Ratios near 1 are fp16 outputs, whose own 2^-11 rounding is the bound.
MEASURED = {"conv y": 0.974, "conv dx": 0.996, "conv dx (stride 2)": 0.961, "conv dw": 0.197, "conv dw (direct)": 0.000, "conv db": 0.037, "conv db (slabs)": 0.000,
            "tconv y": 0.958, "tconv dx": 0.899, "tconv dw": 0.027, "tconv db": 0.005, "long-K dw": 0.004, "long-K db": 0.000}
# Narrowest rejection of a wrong reference (its error / its bound): y 20.7 (last live K block, 1024 -> 512 at 2 x 4 x 4), dx 69.5 (512 -> 512 stride 2 at 2 x 4 x 4),
# dw 2.97 (64-row block at K = 12288), 1.47 (K / 16 rows at K = 49152), 6.87 (two taps swapped), db 1.21 (64-row block at K = 8192), 2.04 (K / 16 rows at K = 12288);
# tconv di / dj exchanged 4130 (y), 549 (dx), 6040 (dW), one sub-pixel 1010 (db); long-K dw 8.25 and db 8.1 (64 rows at K = 65536, same-sign data).
# The longest census case took 0.08 s (three passes of 3(8) -> 32 at 12 x 512 x 512, the first case to run); the longest parity case 2.0 s, nearly all of it the float64
# reference of a 256 x 256 map on the host.


def spec_of(config):
    with open(os.path.join(GOLDEN, "nnunet_plans_2d.json")) as f:
        plans = json.load(f)
    with open(os.path.join(GOLDEN, "nnunet_dataset.json")) as f:
        ds = json.load(f)
    return nnunet.network_spec(plans, config, ds), plans


def out_hw(sig):
    B, H, W, Cx, Cout, Cin, k, stride, ups = sig[:9]
    p = k // 2
    return ((H << ups) + 2 * p - k) // stride + 1, ((W << ups) + 2 * p - k) // stride + 1


def sig_name(sig):
    B, H, W, Cx, Cout, Cin, k, stride, ups, has_bias, trainable = sig
    rows = f"rows{W}" if tb._linear_like(sig) else f"B{B}_{H}x{W}"
    return f"{rows}_{Cx}" + (f"({Cin})" if Cin != Cx else "") + f"-{Cout}_k{k}" + ("_s2" if stride == 2 else "")


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# running one Conv2dFn signature role by role
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def run_roles(lib, mp, xd, wd, bd, dyd, stride, ups, route, roles=("forward", "dgrad", "wgrad")):
    """Conv2dFn on device operands under ag.wgrad_route(route), one pass per role so that each role's kernels are told apart: the forward; a backward in
    which only x takes a gradient; one in which only weight and bias do.  ag.conv_wgrad_direct and ag.colsum_slabs are wrapped (mp: a MonkeyPatch): where
    they ran, `dw_plan` / `db_plan` hold the plan of that launch."""
    out = dict(f_names=set(), d_names=set(), w_names=set(), dw_plan=None, db_plan=None)
    direct_w, direct_c = ag.conv_wgrad_direct, ag.colsum_slabs

    def spy_w(x, dy, Cout, Cin, k, st, wgs=0):
        out["dw_plan"] = ag.wgrad_plan(dy.shape[0], dy.shape[1], dy.shape[2], x.shape[3], dy.shape[3], k, wgs)
        return direct_w(x, dy, Cout, Cin, k, st, wgs)

    def spy_c(dy, N=None):
        out["db_plan"] = ag.colsum_slabs_plan(dy.numel() // dy.shape[-1], dy.shape[-1] if N is None else N)
        return direct_c(dy, N)

    mp.setattr(ag, "conv_wgrad_direct", spy_w)
    mp.setattr(ag, "colsum_slabs", spy_c)
    try:
        with ag.wgrad_route(route):
            if "forward" in roles:
                with reached(lib) as out["f_names"]:
                    out["y"] = ag.Conv2dFn.apply(xd, wd, bd, stride, ups)
                torch.cuda.synchronize()
            if "dgrad" in roles:
                x1 = xd.clone().requires_grad_(True)
                y1 = ag.Conv2dFn.apply(x1, wd, bd, stride, ups)
                with reached(lib) as out["d_names"]:
                    y1.backward(dyd)
                torch.cuda.synchronize()
                out["dx"] = x1.grad
                assert out["dw_plan"] is None and out["db_plan"] is None, "a backward that wants dx alone formed a weight or bias gradient"
            if "wgrad" in roles:
                w2 = wd.clone().requires_grad_(True)
                b2 = bd.clone().requires_grad_(True) if bd is not None else None
                y2 = ag.Conv2dFn.apply(xd, w2, b2, stride, ups)
                with reached(lib) as out["w_names"]:
                    y2.backward(dyd)
                torch.cuda.synchronize()
                out["dw"], out["db"] = w2.grad, (b2.grad if b2 is not None else None)
    finally:
        mp.setattr(ag, "conv_wgrad_direct", direct_w)
        mp.setattr(ag, "colsum_slabs", direct_c)
    out["routes"] = (_one(out["f_names"]), _one(out["d_names"]), "direct" if out["dw_plan"] is not None else _one(out["w_names"]))
    return out


def _one(names):
    names = sorted(names)
    return names[0] if len(names) == 1 else tuple(names)


def check_roles(run, want, name):
    check_route(run["f_names"], want[0], f"{name} forward")
    check_route(run["d_names"], want[1], f"{name} dgrad")
    if want[2] is None:
        return
    if want[2] == "direct":
        assert run["dw_plan"] is not None and not run["w_names"], f"{name} wgrad: the case is meant for the direct route, reached {sorted(run['w_names'])}"
    else:
        assert run["dw_plan"] is None, f"{name} wgrad: took the direct route, the case is meant for {want[2]}"
        check_route(run["w_names"], want[2], f"{name} wgrad")


def host_case(sig):
    """test_conv_backward_at_the_step_shapes' operands: unit-scale x and dy, He-scaled weights, biases around 0.1, all fp16-representable, NCHW on the host."""
    B, H, W, Cx, Cout, Cin, k, stride, ups, has_bias, trainable = sig
    g = torch.Generator().manual_seed(sum(sig[:8]) * 31 + k)
    x = tb.r16(torch.randn((B, Cin, H, W), generator=g))
    w = tb.r16(torch.randn((Cout, Cin, k, k), generator=g) / math.sqrt(Cin * k * k))
    b = tb.r16(torch.randn(Cout, generator=g) * 0.1) if has_bias else None
    Ho, Wo = out_hw(sig)
    dy = tb.r16(torch.randn((B, Cout, Ho, Wo), generator=g))
    return x, w, b, dy


def to_device(sig, x, w, b, dy):
    """NHWC float16 with zero pad channels; the weight as the step holds it (float32, [out, in] for a linear)."""
    B, H, W, Cx, Cout, Cin, k = sig[:7]
    Ho, Wo = out_hw(sig)
    Cy = tb._r(Cout, 8)
    xd = torch.zeros((B, H, W, Cx), dtype=torch.float16)
    xd[..., :Cin] = x.permute(0, 2, 3, 1)
    dyd = torch.zeros((B, Ho, Wo, Cy), dtype=torch.float16)
    dyd[..., :Cout] = dy.permute(0, 2, 3, 1)
    wd = (w.view(Cout, Cin) if tb._linear_like(sig) else w).contiguous().to(DEV)
    return xd.to(DEV), wd, (b.to(DEV) if b is not None else None), dyd.to(DEV)


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# a. per-layer parity.  signature -> (forward, dgrad, wgrad) kernel, "direct" = ldiff_op_conv_wgrad; read from the first run on an MI355X
# ------------------------------------------------------------------------------------------------------------------------------------------------------
NNUNET_CASES = {
    # 2d_reduced at 2 x 64 x 64
    (2, 64, 64, 8, 32, 3, 3, 1, 0, True, True): ("igemm<64,64,gen>", "igemm<64,64,gen>", "gemm_dma<64,64>"),
    (2, 64, 64, 32, 32, 32, 3, 1, 0, True, True): ("igemm<64,64,gen>", "igemm<64,64,gen>", "gemm_dma<64,64>"),
    (2, 64, 64, 32, 64, 32, 3, 2, 0, True, True): ("igemm<64,64,gen>", "conv3x3<8x16,32>", "gemm_dma<64,64>"),
    (2, 32, 32, 64, 64, 64, 3, 1, 0, True, True): ("conv3x3<8x16,64>", "conv3x3<8x16,64>", "gemm_dma<64,64>"),
    (2, 32, 32, 64, 128, 64, 3, 2, 0, True, True): ("igemm<64,64,fast>", "conv3x3<8x16,64>", "gemm_dma<64,64>"),
    (2, 16, 16, 128, 128, 128, 3, 1, 0, True, True): ("conv3x3<8x16,128>", "conv3x3<8x16,128>", "gemm_dma<64,64>"),
    (2, 16, 16, 128, 256, 128, 3, 2, 0, True, True): ("igemm<64,64,fast>", "conv3x3<8x16,128>", "gemm_dma<64,64>"),
    (2, 8, 8, 256, 256, 256, 3, 1, 0, True, True): ("conv3x3<8x8,128>", "conv3x3<8x8,128>", "gemm_dma<64,64>"),
    (1, 1, 128, 256, 512, 256, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "gemm_dma<64,64>"),
    (2, 16, 16, 256, 128, 256, 3, 1, 0, True, True): ("conv3x3<8x16,128>", "conv3x3<8x16,128>", "gemm_dma<64,64>"),
    (2, 16, 16, 128, 4, 128, 1, 1, 0, True, True): ("gemm_dma<64,64>", "igemm<64,64,gen>", "gemm_dma<64,64>"),
    (1, 1, 512, 128, 256, 128, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "gemm_dma<64,64>"),
    (2, 32, 32, 128, 64, 128, 3, 1, 0, True, True): ("conv3x3<8x16,64>", "conv3x3<8x16,128>", "gemm_dma<64,64>"),
    (2, 32, 32, 64, 4, 64, 1, 1, 0, True, True): ("gemm_dma<64,64>", "igemm<64,64,gen>", "gemm_dma<64,64>"),
    (1, 1, 2048, 64, 128, 64, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "gemm_dma<64,64>"),
    (2, 64, 64, 64, 32, 64, 3, 1, 0, True, True): ("conv3x3<8x16,32>", "igemm<64,64,gen>", "gemm_dma<64,64>"),
    (2, 64, 64, 32, 4, 32, 1, 1, 0, True, True): ("igemm<64,64,gen>", "igemm<64,64,gen>", "gemm_dma<64,64>"),
    # 2d at 2 x 128 x 128: the top level (M = 32768) on the direct route
    (2, 128, 128, 8, 32, 3, 3, 1, 0, True, True): ("igemm<64,64,gen>", "igemm<64,64,gen>", "direct"),
    (2, 128, 128, 32, 32, 32, 3, 1, 0, True, True): ("igemm<64,64,gen>", "igemm<64,64,gen>", "direct"),
    (2, 128, 128, 32, 64, 32, 3, 2, 0, True, True): ("igemm<64,64,gen>", "conv3x3<8x16,32>", "gemm_dma<64,64>"),
    (2, 64, 64, 64, 64, 64, 3, 1, 0, True, True): ("conv3x3<8x16,64>", "conv3x3<8x16,64>", "gemm_dma<64,64>"),
    (2, 64, 64, 64, 128, 64, 3, 2, 0, True, True): ("igemm<64,64,fast>", "conv3x3<8x16,64>", "gemm_dma<64,64>"),
    (2, 32, 32, 128, 128, 128, 3, 1, 0, True, True): ("conv3x3<8x16,128>", "conv3x3<8x16,128>", "gemm_dma<64,64>"),
    (2, 32, 32, 128, 256, 128, 3, 2, 0, True, True): ("igemm<64,64,fast>", "conv3x3<8x16,128>", "gemm_dma<64,64>"),
    (2, 16, 16, 256, 256, 256, 3, 1, 0, True, True): ("conv3x3<8x16,128>", "conv3x3<8x16,128>", "gemm_dma<64,64>"),
    (2, 16, 16, 256, 512, 256, 3, 2, 0, True, True): ("igemm<64,64,fast>", "conv3x3<8x16,128>", "gemm_dma<64,64>"),
    (2, 8, 8, 512, 512, 512, 3, 1, 0, True, True): ("conv3x3<8x8,128>", "conv3x3<8x8,128>", "gemm_dma<64,64>"),
    (2, 8, 8, 512, 512, 512, 3, 2, 0, True, True): ("igemm<64,64,fast>", "conv3x3<8x8,128>", "igemm<64,64,gen>"),
    (2, 4, 4, 512, 512, 512, 3, 1, 0, True, True): ("conv3x3<8x8,128>", "conv3x3<8x8,128>", "igemm<64,64,gen>"),
    (2, 4, 4, 512, 512, 512, 3, 2, 0, True, True): ("igemm<64,64,fast>", "conv3x3<8x8,128>", "igemm<64,64,gen>"),
    (2, 2, 2, 512, 512, 512, 3, 1, 0, True, True): ("conv3x3<8x8,128>", "conv3x3<8x8,128>", "igemm<64,64,gen>"),
    (1, 1, 8, 512, 2048, 512, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "igemm<64,64,gen>"),
    (2, 4, 4, 1024, 512, 1024, 3, 1, 0, True, True): ("conv3x3<8x8,128>", "conv3x3<8x8,128>", "igemm<128,64,gen>"),
    (2, 4, 4, 512, 4, 512, 1, 1, 0, True, True): ("gemm_dma<64,64>", "igemm<64,64,gen>", "igemm<64,64,gen>"),
    (1, 1, 32, 512, 2048, 512, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "igemm<64,64,gen>"),
    (2, 8, 8, 1024, 512, 1024, 3, 1, 0, True, True): ("conv3x3<8x8,128>", "conv3x3<8x8,128>", "gemm_dma<128,64>"),
    (2, 8, 8, 512, 4, 512, 1, 1, 0, True, True): ("gemm_dma<64,64>", "igemm<64,64,gen>", "gemm_dma<64,64>"),
    (1, 1, 128, 512, 1024, 512, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "gemm_dma<64,64>"),
    (2, 16, 16, 512, 256, 512, 3, 1, 0, True, True): ("conv3x3<8x16,128>", "conv3x3<8x16,128>", "gemm_dma<64,64>"),
    (2, 16, 16, 256, 4, 256, 1, 1, 0, True, True): ("gemm_dma<64,64>", "igemm<64,64,gen>", "gemm_dma<64,64>"),
    (1, 1, 512, 256, 512, 256, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "gemm_dma<64,64>"),
    (2, 32, 32, 256, 128, 256, 3, 1, 0, True, True): ("conv3x3<8x16,128>", "conv3x3<8x16,128>", "gemm_dma<64,64>"),
    (2, 32, 32, 128, 4, 128, 1, 1, 0, True, True): ("gemm_dma<64,64>", "igemm<64,64,gen>", "gemm_dma<64,64>"),
    (1, 1, 2048, 128, 256, 128, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "gemm_dma<64,64>"),
    (2, 64, 64, 128, 64, 128, 3, 1, 0, True, True): ("conv3x3<8x16,64>", "conv3x3<8x16,128>", "gemm_dma<64,64>"),
    (2, 64, 64, 64, 4, 64, 1, 1, 0, True, True): ("gemm_dma<64,64>", "igemm<64,64,gen>", "gemm_dma<64,64>"),
    (1, 1, 8192, 64, 128, 64, 1, 1, 0, True, True): ("gemm_df", "gemm_df", "gemm_dma<64,64>"),
    (2, 128, 128, 64, 32, 64, 3, 1, 0, True, True): ("conv3x3<8x16,32>", "igemm<64,64,gen>", "direct"),
    (2, 128, 128, 32, 4, 32, 1, 1, 0, True, True): ("igemm<64,64,gen>", "igemm<64,64,gen>", "direct"),
    # what the route census asked for: the smallest shapes at the trainer's widths that reach the kernels the real configuration (B = 12, 512 x 512) reaches and
    # none of the cases above does.  The 16 x 16 ping-pong conv wants >= 226 tiles of 16 x 16 pixels (conv3x3p_selected: 88 % of the 256 CUs): one 256 x 256 map;
    # the 128-row GEMM tiles want 384 workgroups (gemm_dma_tile, igemm_tile).
    (1, 256, 256, 32, 32, 32, 3, 1, 0, True, True): ("igemm<128,64,gen>", "igemm<128,64,gen>", "direct"),
    (1, 256, 256, 64, 4, 64, 1, 1, 0, True, True): ("gemm_dma<128,64>", "igemm<128,64,gen>", "direct"),
    # forward on the 128-column ping-pong kernel: Cout > 64, so the weight gradient is staged at K = 65536, where gamma(K) sum |terms| of zero-mean data holds
    # no wrong reference to account; the case is forward and dgrad only (trainable False, as the frozen layers of test_gpu_backward.py) and LONGK_CASES has its dw
    (1, 256, 256, 64, 128, 64, 3, 1, 0, True, False): ("conv3x3<16x16,128>", "conv3x3<16x16,64>", None),
    (1, 256, 256, 128, 64, 128, 3, 1, 0, True, True): ("conv3x3<16x16,64>", "conv3x3<16x16,128>", "direct"),
    (3, 256, 256, 64, 128, 64, 3, 2, 0, True, True): ("igemm<128,128,fast>", "conv3x3<16x16,64>", "gemm_dma<64,64>"),
    (6, 128, 128, 64, 128, 64, 3, 2, 0, True, True): ("igemm<128,64,fast>", "conv3x3<8x16,64>", "gemm_dma<64,64>"),
    (1, 1, 3072, 512, 2048, 512, 1, 1, 0, True, True): ("gemm_dma<128,128>", "gemm_dma<128,64>", "gemm_dma<64,64>"),
    (12, 32, 32, 512, 4, 512, 1, 1, 0, True, True): ("gemm_dma<64,64>", "igemm<128,128,gen>", "gemm_dma<64,64>"),
}


# Past this many rows a staged weight / bias gradient's worst-case bound gamma(K) sum |terms| grows faster than a 64-row block of zero-mean data (about
# sqrt(64) terms of 2 K^2 u): the wrong reference conv_reference builds is then inside the bound for ANY kernel, so the block left out grows to K / 16 rows,
# the most one split of the GEMM covers (section c states the same rule).  Up to LONG_K rows, and on the direct route at any K, the 64-row block must be seen.
LONG_K = 8192


def _sees(got, wrong, tol):
    return ((got.double().cpu() - wrong.double().cpu()).abs() > tol.double().cpu()).any().item()


def _wider_block(ref, dy):
    """(n, keep): n = K / 16 rows and the mask over dy [B, C, Ho, Wo] that drops the last n rows m = (b, oy, ox)."""
    B, _, Ho, Wo = dy.shape
    n = ref["Mpad"] // 16
    return n, (torch.arange(ref["M"]) < ref["M"] - n).to(torch.float64).view(B, 1, Ho, Wo)


@pytest.mark.parametrize("sig", list(NNUNET_CASES), ids=sig_name)
def test_conv_backward_at_the_trainer_shapes(lib, monkeypatch, sig):
    """Section (a) of the module docstring: Conv2dFn under wgrad_route("auto") as test_gpu_backward.test_conv_backward_at_the_step_shapes runs it."""
    B, H, W, Cx, Cout, Cin, k, stride, ups, has_bias, trainable = sig
    name = sig_name(sig)
    Ho, Wo = out_hw(sig)
    Cy = tb._r(Cout, 8)
    x, w, b, dy = host_case(sig)
    ref = conv_reference(x.double(), w.double(), None if b is None else b.double(), dy.double(), k, stride, ups, Cx, Cy)
    run = run_roles(lib, monkeypatch, *to_device(sig, x, w, b, dy), stride, ups, "auto", roles=("forward", "dgrad", "wgrad") if trainable else ("forward", "dgrad"))
    print(f"[bwd-route] {name}: forward {run['routes'][0]} dgrad {run['routes'][1]} wgrad {run['routes'][2]}")
    y, dx = run["y"], run["dx"]
    want = NNUNET_CASES[sig]
    assert y.shape == (B, Ho, Wo, Cy) and y.dtype == torch.float16 and (y[..., Cout:] == 0).all(), "pad columns of y"
    assert dx.shape == (B, H, W, Cx) and dx.dtype == torch.float16 and (dx[..., Cin:] == 0).all(), "pad columns of dx"

    f16 = lambda r, e: H16 * r.abs() + e * (1 + H16) + U
    check_bound(y[..., :Cout].permute(0, 3, 1, 2), ref["y"], f16(ref["y"], ref["ey"]), f"{name} y (K <= {int(ref['Ky'].max())})", "nnunet conv y",
                [(ref["y_wrong_name"], ref["y_wrong"], f16(ref["y_wrong"], ref["ey"]))])
    check_bound(dx[..., :Cin].permute(0, 3, 1, 2), ref["dx"], f16(ref["dx"], ref["edx"]), f"{name} dx (K <= {ref['Kdx_max']})",
                "nnunet conv dx" + (" (stride 2)" if stride == 2 else ""), [(ref["dx_wrong_name"], ref["dx_wrong"], f16(ref["dx_wrong"], ref["edx"]))])
    if not trainable:
        assert want[2] is None and not run["w_names"]
        check_roles(run, want, name)
        return
    dw, db = run["dw"], run["db"]
    M = B * Ho * Wo
    want_direct = M >= ag.WGRAD_DIRECT_MIN_ROWS and ag.wgrad_direct_eligible(k, stride, ups, Cx, Cy, Cout, Cin)
    assert (run["dw_plan"] is not None) == want_direct, f"{name}: M = {M}; 'auto' took the {'direct' if run['dw_plan'] else 'staged'} weight gradient"
    assert (run["db_plan"] is not None) == (M >= ag.WGRAD_DIRECT_MIN_ROWS)
    assert dw.dtype == torch.float32 and db.dtype == torch.float32 and db.shape == (Cout,)
    if run["dw_plan"] is not None:
        edw, kw = wb.bound(ref["edw"] / gamma(ref["Mpad"]), run["dw_plan"]), f"direct, chain {run['dw_plan']['chain']} + partials {run['dw_plan']['partials']}"
    else:
        edw, kw = ref["edw"], f"K = Mpad = {ref['Mpad']}"
    got_dw = dw.view(Cout, Cin, k, k)
    wrong = [("all of K" if ref["Mpad"] <= 64 else "last K block", ref["dw_wrong"], edw)]
    if run["dw_plan"] is None and ref["Mpad"] > LONG_K and not _sees(got_dw, ref["dw_wrong"], edw):
        n, keep = _wider_block(ref, dy)
        wrong = [(f"last {n} rows (K / 16)", torch.nn.grad.conv2d_weight(x.double(), w.shape, dy.double() * keep, stride=stride, padding=k // 2), edw)]
    live = ref["dw_live_taps"]
    if len(live) >= 2:
        (a0, a1), (c0, c1) = (live[0] // k, live[0] % k), (live[1] // k, live[1] % k)
        sw = ref["dw"].clone()
        sw[:, :, a0, a1], sw[:, :, c0, c1] = ref["dw"][:, :, c0, c1], ref["dw"][:, :, a0, a1]
        wrong.append((f"taps {live[0]} and {live[1]} swapped", sw, edw))
    check_bound(got_dw, ref["dw"], edw, f"{name} dw ({kw})", "nnunet conv dw" + (" (direct)" if run["dw_plan"] else ""), wrong)
    if run["db_plan"] is not None:
        edb, kb = wb.bound(ref["edb"] / gamma(ref["M"]), run["db_plan"]), f"slabs, chain {run['db_plan']['chain']} + partials {run['db_plan']['partials']}"
    else:
        edb, kb = ref["edb"], f"K = {ref['M']}"
    wrong = [("all of K" if ref["M"] <= 64 else "last K block", ref["db_wrong"], edb)]
    if run["db_plan"] is None and ref["M"] > LONG_K and not _sees(db, ref["db_wrong"], edb):
        n, keep = _wider_block(ref, dy)
        wrong = [(f"last {n} rows (K / 16)", (dy.double() * keep).sum((0, 2, 3)), edb)]
    check_bound(db, ref["db"], edb, f"{name} db ({kb})", "nnunet conv db" + (" (slabs)" if run["db_plan"] else ""), wrong)
    check_roles(run, want, name)


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# b. the transposed conv, through TrainableSegNet.tconv itself
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def transpconv_shapes():
    out = []
    for config in PARITY_SHAPES:
        for s in ns.transpconv_shapes(spec_of(config)[0]):
            if s not in out:
                out.append(s)
    return out


@pytest.mark.parametrize("B,h,w", ns.TCONV_MAPS)
@pytest.mark.parametrize("cin,cout", transpconv_shapes())
def test_tconv_backward_against_float64(lib, monkeypatch, cin, cout, B, h, w):
    """Section (b): TrainableSegNet.tconv on a one-layer parameter dict against nnunet_step_sigs.tconv_reference."""
    x, W, b, dy = ns.tconv_case(cin, cout, B, h, w)
    net = object.__new__(nnunet_train.TrainableSegNet)
    train._Graph.__init__(net, {"t.weight": W, "t.bias": b}, DEV, True)
    xd = x.permute(0, 2, 3, 1).contiguous().to(torch.float16).to(DEV).requires_grad_(True)
    dyd = dy.permute(0, 2, 3, 1).contiguous().to(torch.float16).to(DEV)
    plans = {}
    direct_w, direct_c = ag.conv_wgrad_direct, ag.colsum_slabs
    monkeypatch.setattr(ag, "conv_wgrad_direct", lambda x_, dy_, Co, Ci, k, st, wgs=0: (
        plans.__setitem__("dw", ag.wgrad_plan(dy_.shape[0], dy_.shape[1], dy_.shape[2], x_.shape[3], dy_.shape[3], k, wgs)), direct_w(x_, dy_, Co, Ci, k, st, wgs))[1])
    monkeypatch.setattr(ag, "colsum_slabs", lambda dy_, N=None: (
        plans.__setitem__("db", ag.colsum_slabs_plan(dy_.numel() // dy_.shape[-1], dy_.shape[-1] if N is None else N)), direct_c(dy_, N))[1])
    with ag.wgrad_route("auto"):     # as TrainableSegNet.__call__ runs it
        with reached(lib) as f_names:
            y = net.tconv("t", xd)
        with reached(lib) as b_names:
            y.backward(dyd)
    torch.cuda.synchronize()
    name = f"tconv {cin}->{cout} B{B} {h}x{w}"
    print(f"[bwd-route] {name}: forward {sorted(f_names)} backward {sorted(b_names)}" + (" direct" if plans else ""))
    ref = ns.tconv_reference(x.double(), W.double(), b.double(), dy.double(), plans.get("dw"), plans.get("db"))
    assert y.shape == (B, 2 * h, 2 * w, cout) and y.dtype == torch.float16 and xd.grad.shape == xd.shape
    wg, bg = net.p["t.weight"].grad, net.p["t.bias"].grad
    assert wg.shape == (cin, cout, 2, 2) and wg.dtype == torch.float32 and bg.shape == (cout,) and bg.dtype == torch.float32
    f16 = ns.f16_bound
    check_bound(y.detach().permute(0, 3, 1, 2), ref["y"], f16(ref["y"], ref["ey"]), f"{name} y (K = {cin + 1})", "nnunet tconv y",
                [("di / dj exchanged", ref["y_swapped"], f16(ref["y_swapped"], ref["ey"]))])
    check_bound(xd.grad.permute(0, 3, 1, 2), ref["dx"], f16(ref["dx"], ref["edx"]), f"{name} dx (K = {4 * cout})", "nnunet tconv dx",
                [("di / dj exchanged", ref["dx_swapped"], f16(ref["dx_swapped"], ref["edx"]))])
    check_bound(wg, ref["dw"], ref["edw"], f"{name} dw (K = {ref['Kdw']})", "nnunet tconv dw", [("di / dj exchanged", ref["dw_swapped"], ref["edw"])])
    check_bound(bg, ref["db"], ref["edb"], f"{name} db (K = {ref['M']} + 3)", "nnunet tconv db", [("one sub-pixel", ref["db_one_subpixel"], ref["edb"])])


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# c. the staged weight gradient at a long K.  signature -> the wgrad GEMM's kernel
# ------------------------------------------------------------------------------------------------------------------------------------------------------
LONGK_CASES = {
    (1, 64, 128, 128, 128, 128, 3, 1, 0, True, True): "gemm_dma<64,64>",
    (1, 64, 128, 256, 256, 256, 3, 1, 0, True, True): "gemm_dma<64,64>",
    (1, 64, 128, 256, 128, 256, 3, 1, 0, True, True): "gemm_dma<64,64>",
    (1, 128, 128, 512, 512, 512, 3, 2, 0, True, True): "gemm_dma<64,64>",
    (1, 1, 8192, 128, 256, 128, 1, 1, 0, True, True): "gemm_dma<64,64>",
    (1, 256, 256, 64, 128, 64, 3, 1, 0, True, True): "gemm_dma<64,64>",       # K = 65536: the weight gradient of the forward-only case of NNUNET_CASES
}


def _staged_reference(x, dy, sig, drops=(), mags=True):
    """float64 dw [Cout, Cin, k, k] and db from NHWC arrays (wgrad_bound.im2col's columns, one GEMM over the rows m = (b, oy, ox)); with `mags` the magnitude
    sums sum |dy x| and sum |dy|; per n of `drops` the same sums with the last n rows left out, under ("dw", n) / ("db", n)."""
    B, H, W, Cx, Cout, Cin, k, stride = sig[:8]
    Ho, Wo = dy.shape[1:3]
    M = B * Ho * Wo
    xc = torch.from_numpy(wb.im2col(x[..., :Cin].astype(np.float64), k, stride, Ho, Wo).reshape(M, k * k * Cin))
    d = torch.from_numpy(dy[..., :Cout].astype(np.float64).reshape(M, Cout))
    unpack = lambda t: t.view(Cout, k, k, Cin).permute(0, 3, 1, 2).contiguous()
    out = {"dw": unpack(d.T @ xc), "db": d.sum(0)}
    if mags:
        out["mag"], out["magb"] = unpack(d.abs().T @ xc.abs()), d.abs().sum(0)
    for n in drops:
        out[("dw", n)], out[("db", n)] = out["dw"] - unpack(d[-n:].T @ xc[-n:]), out["db"] - d[-n:].sum(0)
    return out


@pytest.mark.parametrize("sig", list(LONGK_CASES), ids=sig_name)
def test_staged_wgrad_at_a_long_k(lib, monkeypatch, sig):
    """Section (c): dw and db of the staged route, exact on integers (9 * 3 * 3 * K < 2^24) and within gamma(Mpad) / gamma(M) on random data."""
    B, H, W, Cx, Cout, Cin, k, stride, ups, has_bias, trainable = sig
    name = sig_name(sig)
    Ho, Wo = out_hw(sig)
    Cy = tb._r(Cout, 8)
    M = B * Ho * Wo
    Mpad = tb._r(M, 8)
    g = torch.Generator().manual_seed(M + Cx)
    wshape = (Cout, Cin) if tb._linear_like(sig) else (Cout, Cin, k, k)
    wd = (torch.randn(wshape, generator=g) / math.sqrt(Cin * k * k)).to(DEV)
    bd = torch.zeros(Cout).to(DEV)

    def run(xn, dyn):
        r = run_roles(lib, monkeypatch, torch.from_numpy(xn).to(DEV), wd, bd, torch.from_numpy(dyn).to(DEV), stride, ups, "staged", roles=("wgrad",))
        assert r["dw_plan"] is None and r["db_plan"] is None
        return r

    # integers: exact, and the same bits twice
    xi, dyi = wb.int_case(B, H, W, Cx, Cy, k, stride, 11 + Cx + Cout)
    assert 9 * 3 * 3 * M < 2 ** 24
    ints = _staged_reference(xi, dyi, sig, mags=False)
    r1, r2 = run(xi, dyi), run(xi, dyi)
    got_w, got_b = r1["dw"].double().cpu().view(Cout, Cin, k, k), r1["db"].double().cpu()
    off_w, off_b = (got_w - ints["dw"]).abs(), (got_b - ints["db"]).abs()
    print(f"[bwd-err] {name} integers, K = {M}: dw off by at most {off_w.max():.0f} ({int((off_w > 0).sum())} elements), db by {off_b.max():.0f}; wgrad {r1['routes'][2]}")
    assert off_w.max() == 0 and off_b.max() == 0, f"{name}: the integer weight / bias gradient is not exact"
    assert torch.equal(r1["dw"], r2["dw"]) and torch.equal(r1["db"], r2["db"]), f"{name}: a second call differs"

    # random data within gamma(Mpad)
    xr, dyr = wb.random_case(B, H, W, Cx, Cy, k, stride, 13 + Cx + Cout)
    ref = _staged_reference(xr, dyr, sig, drops=(64, Mpad // 16))
    rr = run(xr, dyr)
    got_w, got_b = rr["dw"].double().cpu().view(Cout, Cin, k, k), rr["db"].double().cpu()
    tol_w, tol_b = gamma(Mpad) * ref["mag"], gamma(M) * ref["magb"]
    sees = lambda got, wr, tol: ((got - wr).abs() > tol).any().item()
    dropw = 64 if sees(got_w, ref[("dw", 64)], tol_w) else Mpad // 16
    dropb = 64 if sees(got_b, ref[("db", 64)], tol_b) else Mpad // 16
    check_bound(got_w, ref["dw"], tol_w, f"{name} dw (staged, K = Mpad = {Mpad})", "nnunet long-K dw", [(f"last {dropw} rows", ref[("dw", dropw)], tol_w)])
    check_bound(got_b, ref["db"], tol_b, f"{name} db (K = {M})", "nnunet long-K db", [(f"last {dropb} rows", ref[("db", dropb)], tol_b)])
    want = LONGK_CASES[sig]
    check_route(rr["w_names"], want, f"{name} wgrad")
    check_route(r1["w_names"], want, f"{name} wgrad (integers)")


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# d. completeness, and the routes at the real configuration
# ------------------------------------------------------------------------------------------------------------------------------------------------------
def trainer_signatures(monkeypatch, config, B, H, W, seed=5):
    """One eager forward + loss + backward of the Trainer with the two autograd functions' `apply` wrapped, as test_gpu_backward.step_signatures wraps them."""
    seen = {"conv": [], "norm": []}
    conv_apply, norm_apply = ag.Conv2dFn.apply, ag.InstanceNormLReLUFn.apply

    def conv(x, w, b, stride=1, ups=0):
        Bx, Hx, Wx, Cx = x.shape
        seen["conv"].append((Bx, Hx, Wx, Cx, w.shape[0], w.shape[1], w.shape[2] if w.dim() == 4 else 1, stride, ups, b is not None, w.requires_grad))
        return conv_apply(x, w, b, stride, ups)

    def norm(x, *a):
        seen["norm"].append((x.shape[0], x.shape[3], x.shape[1], x.shape[2]))
        return norm_apply(x, *a)

    monkeypatch.setattr(ag.Conv2dFn, "apply", conv)
    monkeypatch.setattr(ag.InstanceNormLReLUFn, "apply", norm)
    spec, plans = spec_of(config)
    tr = nnunet_train.Trainer(spec, tref.synthetic_state_dict(spec, seed), bool(plans["configurations"]["2d"]["batch_dice"]), 10, device=DEV)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn((B, spec["in_channels"], H, W), generator=g)
    assert H == W
    targets = tref.label_maps(B, spec["n_heads"], H, spec["n_stages"] - 1, seed + 2)
    total = tr.loss(tr.network(x), [t.to(DEV) for t in targets], 1024.0)
    total.backward()
    torch.cuda.synchronize()
    assert math.isfinite(float(total))
    graded = [k for k, p in tr.network.p.items() if not k.startswith("decoder.seg_layers.0.")]
    assert all(tr.network.p[k].grad is not None and torch.isfinite(tr.network.p[k].grad).all() for k in graded)
    return spec, seen


@pytest.mark.parametrize("config", list(PARITY_SHAPES))
def test_every_signature_of_the_trainer_step_has_a_case(lib, monkeypatch, config):
    """Section (d): the calls of one eager step are exactly nnunet_step_sigs' lists, in order, and every conv signature is a key of NNUNET_CASES."""
    B, H, W = PARITY_SHAPES[config]
    spec, seen = trainer_signatures(monkeypatch, config, B, H, W)
    stated, stated_n = ns.conv_signatures(spec, B, H, W), ns.norm_signatures(spec, B, H, W)
    print(f"[step-sigs] {config} {B}x{H}x{W}: {len(seen['conv'])} Conv2dFn calls ({len(set(seen['conv']))} signatures), {len(seen['norm'])} InstanceNormLReLUFn calls")
    assert seen["conv"] == stated, f"conv_signatures differs from the step: {sorted(set(seen['conv']) ^ set(stated))}"
    assert seen["norm"] == stated_n, f"norm_signatures differs from the step: {sorted(set(seen['norm']) ^ set(stated_n))}"
    missing = sorted(set(seen["conv"]) - set(NNUNET_CASES))
    assert not missing, f"layer signatures of the {config} step no case covers: {missing}"


def pinned_by_role():
    """role -> the kernels the cases of (a) and (c) state for it ("direct" included)."""
    roles = {"forward": set(), "dgrad": set(), "wgrad": set()}
    for want in NNUNET_CASES.values():
        for role, names in zip(roles, want):
            if names:
                roles[role] |= {names} if isinstance(names, str) else set(names)
    for names in LONGK_CASES.values():
        if names:
            roles["wgrad"] |= {names} if isinstance(names, str) else set(names)
    return roles


def device_case(sig, seed=0):
    """Random operands made on the device (the census shapes are too large to fill from the host in a test's time): unit-scale x and dy, zero pad channels."""
    B, H, W, Cx, Cout, Cin, k, stride, ups, has_bias, trainable = sig
    Ho, Wo = out_hw(sig)
    Cy = tb._r(Cout, 8)
    g = torch.Generator(device=DEV).manual_seed(seed + sum(sig[:8]))
    xd = torch.randn((B, H, W, Cx), generator=g, device=DEV, dtype=torch.float16)
    dyd = torch.randn((B, Ho, Wo, Cy), generator=g, device=DEV, dtype=torch.float16)
    xd[..., Cin:] = 0
    dyd[..., Cout:] = 0
    wshape = (Cout, Cin) if tb._linear_like(sig) else (Cout, Cin, k, k)
    wd = torch.randn(wshape, generator=g, device=DEV) / math.sqrt(Cin * k * k)
    bd = torch.randn(Cout, generator=g, device=DEV) * 0.1
    return xd, wd, bd, dyd


def census_routes(lib, mp, sig):
    """(forward, dgrad, wgrad) kernels of one signature under "auto" on device-made data, and the wall time of the three passes; outputs finite, pad columns zero."""
    t0 = time.perf_counter()
    xd, wd, bd, dyd = device_case(sig)
    run = run_roles(lib, mp, xd, wd, bd, dyd, sig[7], sig[8], "auto")
    ok = all(torch.isfinite(run[n]).all().item() for n in ("y", "dx", "dw", "db"))
    ok = ok and (run["y"][..., sig[4]:] == 0).all().item() and (run["dx"][..., sig[5]:] == 0).all().item()
    return run["routes"], ok, time.perf_counter() - t0


def real_signatures():
    spec, _ = spec_of(REAL_SHAPE[0])
    out = []
    for s in ns.conv_signatures(spec, *REAL_SHAPE[1]):
        if s not in out:
            out.append(s)
    return out


CENSUS = {}


@pytest.mark.parametrize("sig", real_signatures(), ids=sig_name)
def test_route_census_at_the_real_configuration(lib, monkeypatch, sig):
    """`2d` at B = 12, 512 x 512, what scripts/bench_nnunet_train.py runs, one layer at a time: no reference, the outputs finite; the kernel of each role must be
    one a parity case pins in that role -- else that kernel runs in the real step with no per-element test behind it."""
    routes, ok, dt = census_routes(lib, monkeypatch, sig)
    CENSUS[sig] = (routes, dt)
    print(f"[census] {sig_name(sig)}: forward {routes[0]} dgrad {routes[1]} wgrad {routes[2]} ({dt:.2f} s)")
    assert ok, f"{sig_name(sig)}: a non-finite output or a non-zero pad column"
    pinned = pinned_by_role()
    for role, names in zip(pinned, routes):
        names = {names} if isinstance(names, str) else set(names)
        assert names and names <= pinned[role], f"{sig_name(sig)} {role}: reaches {sorted(names)}, which no parity case pins in that role (pinned: {sorted(pinned[role])})"


def teardown_module(module):
    mine = {k: v for k, v in tb.WORST.items() if k.startswith("nnunet ")}
    if mine:
        print("\n[bwd-err] worst measured error / bound per group: " + ", ".join(f"{k[7:]} {v:.3f}" for k, v in sorted(mine.items())))
    if CENSUS:
        slow = max(CENSUS, key=lambda s: CENSUS[s][1])
        print(f"[census] {len(CENSUS)} signatures; the longest case, {sig_name(slow)}, took {CENSUS[slow][1]:.2f} s")
        print("[census] | signature | forward | dgrad | wgrad |")
        for s, (r, _) in CENSUS.items():
            print(f"[census] | {sig_name(s)} | {r[0]} | {r[1]} | {r[2]} |")
