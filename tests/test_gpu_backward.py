"""-m gpu: the backward pass of the fine-tuning step (ldiffusion_amd/autograd.py, csrc/kernels_bwd.hip) at the layer shapes the SD-1.5-width
step really runs (BASELINE.json configs[4]: B = 2, 8 x 8 latents, the frozen VAE decoder up to 64 x 64), each output against a float64
reference on exactly the operands the kernels see, with a per-element error model.

Error model.  u = 2^-24 (fp32 unit roundoff), gamma(K) = 2 K u: the worst-case bound of a K-term fp32 summation in any order, doubled for
MFMA accumulation that does not round to nearest.  fp16 x fp16 products are exact in fp32, so for a contraction whose exact terms have
absolute sum S the fp32 result is within gamma(K) S.  An fp16 output adds its own rounding, 2^-11 |ref| (and 2^-24 where it is
subnormal).
  * conv / linear y and dx (fp16):  2^-11 |ref| + gamma(K) S + 2^-24;  K = (live taps) * Cx (+1 for the bias) for y, (live taps) * Cy for
    dx, per element: a tap on the zero padding adds exact zeros (conv_reference).
    Nearest-2x upsample: dgrad runs on the up-sampled grid, rounds those values to fp16 and sums each 2 x 2 block in torch; the reference is
    the exact float64 sum, and the bound adds 2^-11 * sum |pre-sum values| (each pre-sum value's own fp16 rounding) to the gamma terms
    of the four pre-sum values.
  * conv / linear dw and db (fp32):  gamma(K) S only, K = Mpad = roundup(B*Ho*Wo, 8) for dw (the wgrad GEMM's K), B*Ho*Wo for db.
Each conv case also checks that the bound can fail: the same check must reject a reference that leaves out the last K block of 64 terms
(one K step of the kernels; all of K if K <= 64) and, for a 3x3 dw, one with two live taps' columns swapped.
  * attention backward: see attn_error_bound (derived from attn_bwd_kernel: fp32 scalar FMAs, a recomputed softmax, one fp16 rounding).
  * GroupNorm / LayerNorm / GEGLU / SiLU backward: see the docstrings of their bound functions.
Each group prints the measured worst ratio of error to bound ([bwd-err] lines).  Measured on an MI355X (no bound needed loosening): conv y
0.96, dx 0.97, dx after an upsample 0.13, dw 0.21, db 0.04; attention staged 0.82, direct 0.77; GroupNorm(+SiLU) y 0.98, dx 0.94, dgamma /
dbeta <= 0.07; LayerNorm y 0.82, dx 0.80; GEGLU 0.996; SiLU 0.985 (the fp16 rounding term dominates where the ratio is near 1).  Every wrong
reference broke its bound; the narrowest margins, 2.7x to 3.9x, are dx at K = 9 * 1280 after an upsample and at K = 10240.

Routing.  Each conv case states the kernel its forward, its dgrad and its wgrad launch reach (CONV_CASES), each attention case the
backward path (attn_bwd<staged> / attn_bwd<direct>); test_every_signature_of_the_step_has_a_case fails on a layer shape of the step that no
case covers, so the kernels every backward role of the step reaches are pinned here.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from ldiffusion_amd import _lib, autograd as ag
from kernel_routing import check_route, reached

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
H16 = 2.0 ** -11


def gamma(K):
    return 2.0 * K * U


def r16(x):
    return x.to(torch.float16).to(torch.float32)


def _r(x, m):
    return (x + m - 1) // m * m


WORST = {}   # group -> worst measured error / bound


def _note(group, ratio):
    WORST[group] = max(WORST.get(group, 0.0), ratio)


def _ratio(err, tol):   # err / tol; where the bound is 0 (an element with no live term) the error must be exactly 0
    return torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))


def check_bound(got, ref, tol, what, group=None, wrong=()):
    """every |got - ref| <= tol (float64, same shapes); each (name, wrong_ref, wrong_tol) of `wrong` must break its bound somewhere."""
    got, ref, tol = got.double().cpu(), ref.double().cpu(), tol.double().cpu()
    assert got.shape == ref.shape == tol.shape, f"{what}: shapes {tuple(got.shape)} {tuple(ref.shape)} {tuple(tol.shape)}"
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - ref).abs()
    ratio = _ratio(err, tol).max().item() if err.numel() else 0.0
    rej = []
    for name, wref, wtol in wrong:
        r = _ratio((got - wref.double().cpu()).abs(), wtol.double().cpu()).max().item()
        rej.append(f"{name} {r:.3g}x")
        assert r > 1.0, f"{what}: the bound does not reject the wrong reference '{name}' (worst {r:.3f} of its bound): too loose to see it"
    print(f"[bwd-err] {what}: {ratio:.3f} of the bound" + (f"; wrong refs at {', '.join(rej)} of theirs" if rej else ""))
    if group:
        _note(group, ratio)
    bad = err > tol
    assert not bad.any(), (f"{what}: {int(bad.sum())}/{bad.numel()} out of the bound, worst {ratio:.3f}x "
                           f"at {tuple(int(i) for i in torch.nonzero(_ratio(err, tol) == ratio)[0])}")


# ------------------------------------------------------------------------------------------------------------------------------------------
# 1. conv / linear backward at every Conv2dFn signature of the step
# signature (B, H, W, Cx, Cout, Cin, k, stride, ups, has_bias, trainable) -> (forward, dgrad, wgrad) kernel (wgrad None: frozen weights)
# ------------------------------------------------------------------------------------------------------------------------------------------
_CTX_LENGTHS = (1, 6, 7, 77)   # prompt lengths without padding (CLIP's limit is 77); the step's reference fixture uses 6

CONV_CASES = {
    # text projection: [Lk, 768] rows (batch 1) -> 768
    **{(1, 1, L, 768, 768, 768, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "igemm<64,64,gen>") for L in _CTX_LENGTHS},
    # time embedding MLP (B = 2 rows)
    (1, 1, 2, 320, 1280, 320, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "igemm<64,64,gen>"),
    (1, 1, 2, 1280, 1280, 1280, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "igemm<64,64,gen>"),
    # ResnetBlock2D.time_emb_proj
    (1, 1, 2, 1280, 320, 1280, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "igemm<64,64,gen>"),
    (1, 1, 2, 1280, 640, 1280, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "igemm<64,64,gen>"),
    # attn2.to_k / to_v on the expanded context [2 * Lk, 768]
    **{(1, 1, 2 * L, 768, C, 768, 1, 1, 0, False, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "igemm<64,64,gen>") for L in _CTX_LENGTHS for C in (320, 640, 1280)},
    # UNet, 8 x 8 level (320)
    (2, 8, 8, 8, 320, 4, 3, 1, 0, True, True): ("igemm<64,64,gen>", "conv3x3<8x8,32>", "gemm_dma<64,64>"),
    (2, 8, 8, 320, 320, 320, 3, 1, 0, True, True): ("conv3x3<8x8,160>", "conv3x3<8x8,160>", "gemm_dma<64,64>"),
    (2, 8, 8, 320, 320, 320, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "gemm_dma<64,64>"),
    (1, 1, 128, 320, 320, 320, 1, 1, 0, False, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "gemm_dma<64,64>"),
    (1, 1, 128, 320, 320, 320, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "gemm_dma<64,64>"),
    (1, 1, 128, 320, 2560, 320, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "gemm_dma<64,64>"),
    (1, 1, 128, 1280, 320, 1280, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "gemm_dma<64,64>"),
    (2, 8, 8, 320, 320, 320, 3, 2, 0, True, True): ("igemm<64,64,fast>", "conv3x3<8x8,160>", "igemm<64,64,gen>"),
    (2, 8, 8, 960, 320, 960, 3, 1, 0, True, True): ("conv3x3<8x8,160>", "conv3x3<8x8,160>", "gemm_dma<128,64>"),
    (2, 8, 8, 960, 320, 960, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "gemm_dma<64,64>"),
    (2, 8, 8, 640, 320, 640, 3, 1, 0, True, True): ("conv3x3<8x8,160>", "conv3x3<8x8,128>", "gemm_dma<64,64>"),
    (2, 8, 8, 640, 320, 640, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "gemm_dma<64,64>"),
    (2, 8, 8, 320, 4, 320, 3, 1, 0, True, True): ("conv3x3<8x8,32>", "igemm<64,64,gen>", "gemm_dma<64,64>"),
    # 4 x 4 level (640)
    (2, 4, 4, 320, 640, 320, 3, 1, 0, True, True): ("conv3x3<8x8,128>", "conv3x3<8x8,160>", "igemm<64,64,gen>"),
    (2, 4, 4, 640, 640, 640, 3, 1, 0, True, True): ("conv3x3<8x8,128>", "conv3x3<8x8,128>", "igemm<128,64,gen>"),
    (2, 4, 4, 320, 640, 320, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "igemm<64,64,gen>"),
    (2, 4, 4, 640, 640, 640, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "igemm<64,64,gen>"),
    (1, 1, 32, 640, 640, 640, 1, 1, 0, False, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "igemm<64,64,gen>"),
    (1, 1, 32, 640, 640, 640, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "igemm<64,64,gen>"),
    (1, 1, 32, 640, 5120, 640, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "igemm<128,64,gen>"),
    (1, 1, 32, 2560, 640, 2560, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "igemm<64,64,gen>"),
    (2, 4, 4, 640, 640, 640, 3, 2, 0, True, True): ("igemm<64,64,fast>", "conv3x3<8x8,128>", "igemm<128,64,gen>"),
    (2, 4, 4, 1920, 640, 1920, 3, 1, 0, True, True): ("conv3x3<8x8,128>", "conv3x3<8x8,128>", "igemm<128,128,gen>"),
    (2, 4, 4, 1920, 640, 1920, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "igemm<64,64,gen>"),
    (2, 4, 4, 1280, 640, 1280, 3, 1, 0, True, True): ("conv3x3<8x8,128>", "conv3x3<8x8,128>", "igemm<128,128,gen>"),
    (2, 4, 4, 1280, 640, 1280, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "igemm<64,64,gen>"),
    (2, 4, 4, 960, 640, 960, 3, 1, 0, True, True): ("conv3x3<8x8,128>", "conv3x3<8x8,160>", "igemm<128,64,gen>"),
    (2, 4, 4, 960, 640, 960, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "igemm<64,64,gen>"),
    (2, 4, 4, 640, 640, 640, 3, 1, 1, True, True): ("conv3x3<8x8,128>", "conv3x3<8x8,128>", "gemm_dma<128,64>"),
    # 2 x 2 level (1280)
    (2, 2, 2, 640, 1280, 640, 3, 1, 0, True, True): ("conv3x3<8x8,128>", "conv3x3<8x8,128>", "igemm<128,128,gen>"),
    (2, 2, 2, 1280, 1280, 1280, 3, 1, 0, True, True): ("conv3x3<8x8,128>", "conv3x3<8x8,128>", "igemm<128,128,gen>"),
    (2, 2, 2, 640, 1280, 640, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "igemm<64,64,gen>"),
    (2, 2, 2, 1280, 1280, 1280, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "igemm<64,64,gen>"),
    (1, 1, 8, 1280, 1280, 1280, 1, 1, 0, False, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "igemm<64,64,gen>"),
    (1, 1, 8, 1280, 1280, 1280, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "igemm<64,64,gen>"),
    (1, 1, 8, 1280, 10240, 1280, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "igemm<128,128,gen>"),
    (1, 1, 8, 5120, 1280, 5120, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<128,64>", "igemm<128,128,gen>"),
    (2, 2, 2, 1280, 1280, 1280, 3, 2, 0, True, True): ("igemm<64,64,fast>", "conv3x3<8x8,128>", "igemm<128,128,gen>"),
    (2, 2, 2, 2560, 1280, 2560, 3, 1, 0, True, True): ("conv3x3<8x8,128>", "conv3x3<8x8,128>", "igemm<128,128,gen>"),
    (2, 2, 2, 2560, 1280, 2560, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "igemm<128,64,gen>"),
    (2, 2, 2, 1920, 1280, 1920, 3, 1, 0, True, True): ("conv3x3<8x8,128>", "conv3x3<8x8,128>", "igemm<128,128,gen>"),
    (2, 2, 2, 1920, 1280, 1920, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "igemm<64,64,gen>"),
    (2, 2, 2, 1280, 1280, 1280, 3, 1, 1, True, True): ("conv3x3<8x8,128>", "conv3x3<8x8,128>", "igemm<128,128,gen>"),
    # 1 x 1 level (1280) and the mid block
    (2, 1, 1, 1280, 1280, 1280, 3, 1, 0, True, True): ("conv3x3<8x8,128>", "conv3x3<8x8,128>", "igemm<128,128,gen>"),
    (2, 1, 1, 1280, 1280, 1280, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "igemm<64,64,gen>"),
    (1, 1, 2, 1280, 1280, 1280, 1, 1, 0, False, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "igemm<64,64,gen>"),
    (1, 1, 2, 1280, 10240, 1280, 1, 1, 0, True, True): ("gemm_dma<128,64>", "gemm_dma<64,64>", "igemm<128,128,gen>"),
    (1, 1, 2, 5120, 1280, 5120, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<128,64>", "igemm<128,128,gen>"),
    (2, 1, 1, 2560, 1280, 2560, 3, 1, 0, True, True): ("conv3x3<8x8,128>", "conv3x3<8x8,128>", "igemm<128,128,gen>"),
    (2, 1, 1, 2560, 1280, 2560, 1, 1, 0, True, True): ("gemm_dma<64,64>", "gemm_dma<64,64>", "igemm<128,64,gen>"),
    (2, 1, 1, 1280, 1280, 1280, 3, 1, 1, True, True): ("conv3x3<8x8,128>", "conv3x3<8x8,128>", "igemm<128,128,gen>"),
    # frozen VAE decoder (forward and dgrad only)
    (2, 8, 8, 8, 4, 4, 1, 1, 0, True, False): ("igemm<64,64,gen>", "igemm<64,64,gen>", None),
    (2, 8, 8, 8, 512, 4, 3, 1, 0, True, False): ("igemm<64,64,gen>", "conv3x3<8x8,32>", None),
    (2, 8, 8, 512, 512, 512, 3, 1, 0, True, False): ("conv3x3<8x8,128>", "conv3x3<8x8,128>", None),
    (1, 1, 128, 512, 512, 512, 1, 1, 0, True, False): ("gemm_dma<64,64>", "gemm_dma<64,64>", None),
    (2, 8, 8, 512, 512, 512, 3, 1, 1, True, False): ("conv3x3<8x8,128>", "conv3x3<8x16,128>", None),
    (2, 16, 16, 512, 512, 512, 3, 1, 0, True, False): ("conv3x3<8x16,128>", "conv3x3<8x16,128>", None),
    (2, 16, 16, 512, 512, 512, 3, 1, 1, True, False): ("conv3x3<8x16,128>", "conv3x3<8x16,128>", None),
    (2, 32, 32, 512, 256, 512, 3, 1, 0, True, False): ("conv3x3<8x16,128>", "conv3x3<8x16,128>", None),
    (2, 32, 32, 256, 256, 256, 3, 1, 0, True, False): ("conv3x3<8x16,128>", "conv3x3<8x16,128>", None),
    (2, 32, 32, 512, 256, 512, 1, 1, 0, True, False): ("gemm_dma<64,64>", "gemm_dma<64,64>", None),
    (2, 32, 32, 256, 256, 256, 3, 1, 1, True, False): ("conv3x3<8x16,128>", "conv3x3<8x16,128>", None),
    (2, 64, 64, 256, 128, 256, 3, 1, 0, True, False): ("conv3x3<8x16,128>", "conv3x3<8x16,128>", None),
    (2, 64, 64, 128, 128, 128, 3, 1, 0, True, False): ("conv3x3<8x16,128>", "conv3x3<8x16,128>", None),
    (2, 64, 64, 256, 128, 256, 1, 1, 0, True, False): ("gemm_df", "gemm_df", None),
    (2, 64, 64, 128, 3, 128, 3, 1, 0, True, False): ("conv3x3<8x16,32>", "igemm<64,64,gen>", None),
}


def conv_name(sig):
    B, H, W, Cx, Cout, Cin, k, stride, ups, has_bias, trainable = sig
    s = f"{'unet' if trainable else 'vae'}_B{B}_{H}x{W}_{Cx}" + (f"({Cin})" if Cin != Cx else "") + f"-{Cout}_k{k}"
    return s + ("_s2" if stride == 2 else "") + ("_up" if ups else "") + ("" if has_bias else "_nobias")


def _fold2(t):   # [B, C, 2H, 2W] -> sum of every 2 x 2 block
    B, Cc, H2, W2 = t.shape
    return t.view(B, Cc, H2 // 2, 2, W2 // 2, 2).sum((3, 5))


def conv_reference(x, w, b, dy, k, stride, ups, Cx, Cy):
    """float64 y, dx, dw, db of conv2d(nearest_up(x, 2**ups), w, b, stride, k // 2) for the cotangent dy; their gamma terms gamma(K) S per
    element; and the references the bound must reject.  x [B,Cin,H,W], w [Cout,Cin,k,k], dy [B,Cout,Ho,Wo].

    K per element counts the terms that are not structurally zero: taps that fall on the zero padding (or, in dgrad after a stride-2
    forward, on the inserted zeros) add exact zeros, which round nothing.  At a 1 x 1 map a 3 x 3 conv has one live tap, so K = Cx there, not
    9 Cx.  The K block the wrong references leave out is the last 64 of the kernel's K order (tap * Cx + c for y, flipped tap * Cy + n for
    dx, the rows m for dw / db) among the live taps."""
    pad = k // 2
    xu = F.interpolate(x, scale_factor=2.0, mode="nearest") if ups else x
    B, Cin, He, We = xu.shape
    Cout = w.shape[0]
    Ho, Wo = dy.shape[2:]
    kk = k * k
    one = torch.ones((1, 1, k, k), dtype=x.dtype)
    onehot = torch.eye(kk, dtype=x.dtype).view(kk, 1, k, k)
    out = {}
    # ---- y: K order tap * Cx + c
    out["y"] = F.conv2d(xu, w, b, stride=stride, padding=pad)
    Sy = F.conv2d(xu.abs(), w.abs(), None if b is None else b.abs(), stride=stride, padding=pad)
    taps_y = F.conv2d(torch.ones((1, 1, He, We), dtype=x.dtype), one, stride=stride, padding=pad)     # live taps per output pixel
    out["Ky"] = taps_y * Cx + (0 if b is None else 1)
    out["ey"] = gamma(out["Ky"]) * Sy
    live_y = F.conv2d(torch.ones((1, 1, He, We), dtype=x.dtype), onehot, stride=stride, padding=pad)[0].flatten(1).amax(1) > 0
    order = [(tap, c) for tap in range(kk) if live_y[tap] for c in range(Cx)][-64:]
    my = torch.zeros((Cin, kk), dtype=x.dtype)
    for tap, c in order:
        if c < Cin:
            my[c, tap] = 1
    c0 = min(c for _, c in order)
    if c0 < Cin:
        out["y_wrong"] = out["y"] - F.conv2d(xu[:, c0:], (w * my.view(1, Cin, k, k))[:, c0:], None, stride=stride, padding=pad)
    else:
        out["y_wrong"] = out["y"]
    out["y_wrong_name"] = "all of K" if len(order) == sum(int(t) for t in live_y) * Cx else "last live K block"
    # ---- dx on the (up-sampled) grid: K order flipped tap * Cy + n over dy channels
    dxu = torch.nn.grad.conv2d_input(xu.shape, w, dy, stride=stride, padding=pad)
    Sdxu = torch.nn.grad.conv2d_input(xu.shape, w.abs(), dy.abs(), stride=stride, padding=pad)
    ones_dy = torch.ones((1, 1, Ho, Wo), dtype=x.dtype)
    taps_dx = torch.nn.grad.conv2d_input((1, 1, He, We), one, ones_dy, stride=stride, padding=pad)
    edxu = gamma(taps_dx * Cy) * Sdxu
    live_d = torch.stack([torch.nn.grad.conv2d_input((1, 1, He, We), onehot[t:t + 1], ones_dy, stride=stride, padding=pad).amax() > 0 for t in range(kk)])
    orderd = [(kk - 1 - tp, n) for tp in range(kk) if live_d[kk - 1 - tp] for n in range(Cy)][-64:]
    md = torch.zeros((Cout, kk), dtype=x.dtype)
    for tap, n in orderd:
        if n < Cout:
            md[n, tap] = 1
    n0 = min(n for _, n in orderd)
    if n0 < Cout:
        dxu_wrong = dxu - torch.nn.grad.conv2d_input(xu.shape, (w * md.view(Cout, 1, k, k))[n0:], dy[:, n0:], stride=stride, padding=pad)
    else:
        dxu_wrong = dxu
    out["dx_wrong_name"] = "all of K" if len(orderd) == sum(int(t) for t in live_d) * Cy else "last live K block"
    if ups:
        out["dx"], out["edx"], out["dx_wrong"] = _fold2(dxu), _fold2(edxu) + H16 * _fold2(dxu.abs()), _fold2(dxu_wrong)
    else:
        out["dx"], out["edx"], out["dx_wrong"] = dxu, edxu, dxu_wrong
    out["Kdx_max"] = int(taps_dx.max()) * Cy
    # ---- dw over K = Mpad rows m = (b, oy, ox); db over the M rows
    M = B * Ho * Wo
    Mpad = _r(M, 8)
    out["dw"] = torch.nn.grad.conv2d_weight(xu, w.shape, dy, stride=stride, padding=pad)
    out["edw"] = gamma(Mpad) * torch.nn.grad.conv2d_weight(xu.abs(), w.shape, dy.abs(), stride=stride, padding=pad)
    keep = (torch.arange(M) < max(0, Mpad - 64)).to(dy.dtype).view(B, 1, Ho, Wo)
    out["dw_wrong"] = torch.nn.grad.conv2d_weight(xu, w.shape, dy * keep, stride=stride, padding=pad)
    out["dw_live_taps"] = [t for t in range(kk) if live_y[t]]
    out["db"] = dy.sum((0, 2, 3))
    out["edb"] = gamma(M) * dy.abs().sum((0, 2, 3))
    out["db_wrong"] = (dy * keep).sum((0, 2, 3))
    out["M"], out["Mpad"] = M, Mpad
    return out


def _linear_like(sig):
    B, H, W, Cx, Cout, Cin, k = sig[:7]
    return B == 1 and H == 1 and k == 1   # rows through ag.linear: the step's weights are [out, in]


@pytest.mark.parametrize("sig", list(CONV_CASES), ids=conv_name)
def test_conv_backward_at_the_step_shapes(lib, sig):
    B, H, W, Cx, Cout, Cin, k, stride, ups, has_bias, trainable = sig
    name = conv_name(sig)
    g = torch.Generator().manual_seed(sum(sig[:8]) * 31 + k)
    x = r16(torch.randn((B, Cin, H, W), generator=g))
    w = r16(torch.randn((Cout, Cin, k, k), generator=g) / math.sqrt(Cin * k * k))
    b = r16(torch.randn(Cout, generator=g) * 0.1) if has_bias else None
    Ho = ((H << ups) + 2 * (k // 2) - k) // stride + 1
    Wo = ((W << ups) + 2 * (k // 2) - k) // stride + 1
    Cy = _r(Cout, 8)
    dy = r16(torch.randn((B, Cout, Ho, Wo), generator=g))
    ref = conv_reference(x.double(), w.double(), None if b is None else b.double(), dy.double(), k, stride, ups, Cx, Cy)

    xd = torch.zeros((B, H, W, Cx), dtype=torch.float16)
    xd[..., :Cin] = x.permute(0, 2, 3, 1)
    xd = xd.to(DEV)
    wd = (w.view(Cout, Cin) if _linear_like(sig) else w).contiguous().to(DEV)
    bd = b.to(DEV) if has_bias else None
    dyd = torch.zeros((B, Ho, Wo, Cy), dtype=torch.float16)
    dyd[..., :Cout] = dy.permute(0, 2, 3, 1)
    dyd = dyd.to(DEV)
    want = CONV_CASES[sig]

    # forward
    with reached(lib) as f_names:
        y = ag.Conv2dFn.apply(xd, wd, bd, stride, ups)
    torch.cuda.synchronize()
    # dgrad: only x requires grad
    x1 = xd.clone().requires_grad_(True)
    y1 = ag.Conv2dFn.apply(x1, wd, bd, stride, ups)
    with reached(lib) as d_names:
        y1.backward(dyd)
    torch.cuda.synchronize()
    # wgrad + bias column sums: only w and b require grad
    w_names, w2, b2 = set(), None, None
    if trainable:
        w2 = wd.clone().requires_grad_(True)
        b2 = bd.clone().requires_grad_(True) if has_bias else None
        y2 = ag.Conv2dFn.apply(xd, w2, b2, stride, ups)
        with reached(lib) as w_names:
            y2.backward(dyd)
        torch.cuda.synchronize()
        assert y2.grad_fn is not None
    routes = (sorted(f_names), sorted(d_names), sorted(w_names))
    print(f"[bwd-route] {name}: forward {routes[0]} dgrad {routes[1]} wgrad {routes[2]}")

    # pad columns zero, dtypes
    assert y.shape == (B, Ho, Wo, Cy) and y.dtype == torch.float16 and (y[..., Cout:] == 0).all()
    assert x1.grad.shape == xd.shape and x1.grad.dtype == torch.float16 and (x1.grad[..., Cin:] == 0).all()
    if trainable:
        assert w2.grad.dtype == torch.float32 and w2.grad.shape == wd.shape

    f16 = lambda r, e: H16 * r.abs() + e * (1 + H16) + U
    got_y = y[..., :Cout].permute(0, 3, 1, 2)
    check_bound(got_y, ref["y"], f16(ref["y"], ref["ey"]), f"{name} y (K <= {int(ref['Ky'].max())})", "conv y",
                [(ref["y_wrong_name"], ref["y_wrong"], f16(ref["y_wrong"], ref["ey"]))])
    got_dx = x1.grad[..., :Cin].permute(0, 3, 1, 2)
    check_bound(got_dx, ref["dx"], f16(ref["dx"], ref["edx"]), f"{name} dx (K <= {ref['Kdx_max']})", "conv dx" + (" (ups)" if ups else ""),
                [(ref["dx_wrong_name"], ref["dx_wrong"], f16(ref["dx_wrong"], ref["edx"]))])
    if trainable:
        Kw = ref["Mpad"]
        got_dw = w2.grad.view(Cout, Cin, k, k)
        wrong = [("all of K" if Kw <= 64 else "last K block", ref["dw_wrong"], ref["edw"])]
        live = ref["dw_live_taps"]
        if len(live) >= 2:   # two live taps' columns swapped
            t0, t1 = (live[0] // k, live[0] % k), (live[1] // k, live[1] % k)
            sw = ref["dw"].clone()
            sw[:, :, t0[0], t0[1]], sw[:, :, t1[0], t1[1]] = ref["dw"][:, :, t1[0], t1[1]], ref["dw"][:, :, t0[0], t0[1]]
            wrong.append((f"taps {live[0]} and {live[1]} swapped", sw, ref["edw"]))
        check_bound(got_dw, ref["dw"], ref["edw"], f"{name} dw (K = Mpad = {Kw})", "conv dw", wrong)
        if has_bias:
            check_bound(b2.grad, ref["db"], ref["edb"], f"{name} db", "conv db",
                        [("all of K" if ref["M"] <= 64 else "last K block", ref["db_wrong"], ref["edb"])])
    # the kernels each role reached (after the numbers: a case whose route moved still reports its errors)
    assert want is not None, f"{name}: CONV_CASES states no kernels for this signature (reached {routes})"
    check_route(f_names, want[0], f"{name} forward")
    check_route(d_names, want[1], f"{name} dgrad")
    if trainable:
        check_route(w_names, want[2], f"{name} wgrad")
    else:
        assert want[2] is None and not w_names


# ------------------------------------------------------------------------------------------------------------------------------------------
# 2. attention backward
# ------------------------------------------------------------------------------------------------------------------------------------------
def attn_error_bound(q, k, v, dO, scale):
    """float64 reference (dq, dk, dv) of softmax(scale q k^T) v for the cotangent dO and a per-element bound for attn_bwd_kernel.
    q [.., Lq, d], k / v [.., Lk, d], dO [.., Lq, d].  First-order propagation of the kernel's fp32 arithmetic, g(n) = gamma(n):
      scores  S = scale q.k over d fp32 FMAs:                        eS  = g(d) scale sum|q||k|   (+ u |S| for the scale)
      P       softmax of S, recomputed (max, __expf, one sum, one divide):
              eP_ij = P_ij (eS_ij + max_l eS_il + u (2 Lk + 8 + 2 |S_ij - max_l S_il|))
      dP      dO.v over d:                                           edP = g(d) sum|dO||v|
      dot_i   sum_j dP_ij P_ij over Lk:                              edot = sum_j (|dP| eP + P edP) + g(Lk) sum_j |dP P|
      dS      P (dP - dot):                                          edS = eP |dP - dot| + P (edP + edot) + 3u |P (dP - dot)|
      dV      sum_j P_jk dO_jc:        sum_j eP |dO| + g(Lq) sum_j P |dO|
      dQ, dK  scale sum dS k / dS^T q: scale (sum edS |k| + g(Lk or Lq) sum |dS| |k|)
    plus one fp16 rounding of each output, 2^-11 |ref| + 2^-24."""
    Lk, Lq, d = k.shape[-2], q.shape[-2], q.shape[-1]
    S = scale * q @ k.transpose(-1, -2)
    eS = gamma(d) * scale * (q.abs() @ k.abs().transpose(-1, -2)) + U * S.abs()
    P = torch.softmax(S, -1)
    mx = S.max(-1, keepdim=True).values
    eP = P * (eS + eS.max(-1, keepdim=True).values + U * (2 * Lk + 8 + 2 * (S - mx).abs()))
    dP = dO @ v.transpose(-1, -2)
    edP = gamma(d) * (dO.abs() @ v.abs().transpose(-1, -2))
    dot = (dP * P).sum(-1, keepdim=True)
    edot = (dP.abs() * eP + P * edP).sum(-1, keepdim=True) + gamma(Lk) * (dP * P).abs().sum(-1, keepdim=True)
    dS = P * (dP - dot)
    edS = eP * (dP - dot).abs() + P * (edP + edot) + 3 * U * dS.abs()
    dv = P.transpose(-1, -2) @ dO
    edv = eP.transpose(-1, -2) @ dO.abs() + gamma(Lq) * (P.transpose(-1, -2) @ dO.abs())
    dq = scale * dS @ k
    edq = scale * (edS @ k.abs() + gamma(Lk) * (dS.abs() @ k.abs()))
    dk = scale * dS.transpose(-1, -2) @ q
    edk = scale * (edS.transpose(-1, -2) @ q.abs() + gamma(Lq) * (dS.abs().transpose(-1, -2) @ q.abs()))
    out = {}
    for n, r, e in (("dq", dq, edq), ("dk", dk, edk), ("dv", dv, edv)):
        out[n] = (r, H16 * r.abs() + e * (1 + H16) + U)
    return out


def _heads(t, B, L, heads, d):   # [B, L, heads*d] -> [B, heads, L, d]
    return t.view(B, L, heads, d).transpose(1, 2)


def _unheads(t):
    B, h, L, d = t.shape
    return t.transpose(1, 2).reshape(B, L, h * d)


# (B, heads, Lq, Lk, d) -> the backward path
ATTN_CASES = {
    **{(2, 8, L, L, d): "attn_bwd<staged>" for L, d in ((64, 40), (16, 80), (4, 160), (1, 160))},               # self-attention
    **{(2, 8, L, Lk, d): "attn_bwd<staged>" for L, d in ((64, 40), (16, 80), (4, 160), (1, 160)) for Lk in _CTX_LENGTHS},   # cross
    (2, 1, 64, 64, 512): "attn_bwd<staged>",        # VAE mid block: one head of 512
    (2, 8, 64, 128, 40): "attn_bwd<staged>",        # Lq * Lk = 8192: every register slot of the staged path
    (1, 2, 8192, 1, 40): "attn_bwd<direct>",        # Lq * Lk = 8192 with one key: the staging (2 (Lq + Lk) rows) does not fit
    (1, 1, 4096, 2, 64): "attn_bwd<direct>",
    (3, 8, 16, 7, 80): "attn_bwd<staged>",          # three batch entries, K and V per entry
}


def attn_name(key):
    B, heads, Lq, Lk, d = key
    return f"B{B}_h{heads}_{Lq}x{Lk}_d{d}"


@pytest.mark.parametrize("key", list(ATTN_CASES), ids=attn_name)
def test_attention_backward_at_the_step_shapes(lib, key):
    B, heads, Lq, Lk, d = key
    Cc = heads * d
    g = torch.Generator().manual_seed(Lq * 7 + Lk * 3 + d + B)
    q, k, v, dO = (r16(torch.randn((B, L, Cc), generator=g) * s) for L, s in ((Lq, 1.0), (Lk, 1.0), (Lk, 1.0), (Lq, 1.0)))
    qd, kd, vd = (t.to(torch.float16).to(DEV).requires_grad_(True) for t in (q, k, v))
    o = ag.AttentionFn.apply(qd, kd, vd, heads)
    with reached(lib) as names:
        o.backward(dO.to(torch.float16).to(DEV))
    torch.cuda.synchronize()
    name = attn_name(key)
    check_route(names, ATTN_CASES[key], name)
    sh = lambda t, L: _heads(t, B, L, heads, d)
    ref = attn_error_bound(sh(q, Lq).double(), sh(k, Lk).double(), sh(v, Lk).double(), sh(dO, Lq).double(), 1.0 / math.sqrt(d))
    for n, got in (("dq", qd.grad), ("dk", kd.grad), ("dv", vd.grad)):
        r, tol = ref[n]
        assert got.dtype == torch.float16
        check_bound(got.float(), _unheads(r), _unheads(tol), f"attn {name} {n}", f"attention ({ATTN_CASES[key][9:-1]})")


def test_attention_backward_odd_row_pitch_takes_the_direct_path(lib):
    """Rows of 41 halves (an odd pitch; the staged path reads 32-bit words): ldiff_op_attention_bwd directly, one head of 40 of each row,
    B = 2 with per-entry K / V.  The column outside the head is not written."""
    B, Lq, Lk, d, ld = 2, 16, 7, 40, 41
    g = torch.Generator().manual_seed(41)
    q, k, v, dO = (r16(torch.randn((B, L, ld), generator=g)) for L in (Lq, Lk, Lk, Lq))
    dev = [t.to(torch.float16).to(DEV) for t in (q, k, v, dO)]
    outs = [torch.full((B, L, ld), 7.0, dtype=torch.float16, device=DEV) for L in (Lq, Lk, Lk)]
    scale = 1.0 / math.sqrt(d)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    with reached(lib) as names:
        _lib.check(lib.ldiff_op_attention_bwd(dev[0].data_ptr(), ld, dev[1].data_ptr(), ld, dev[2].data_ptr(), ld, dev[3].data_ptr(), ld, outs[0].data_ptr(),
                                              outs[1].data_ptr(), outs[2].data_ptr(), B, 1, Lq, Lk, d, Lq * ld, Lk * ld, Lq * ld, scale, s))
    torch.cuda.synchronize()
    check_route(names, "attn_bwd<direct>", "odd pitch")
    ref = attn_error_bound(*(t[..., :d].double() for t in (q, k, v, dO)), scale)
    for n, got in zip(("dq", "dk", "dv"), outs):
        r, tol = ref[n]
        check_bound(got[..., :d].float(), r, tol, f"odd pitch {n}", "attention (direct)")
        assert (got[..., d:] == 7.0).all(), f"{n}: a column outside the head was written"


def test_attention_backward_rejections(lib):
    """The two documented refusals of launch_attn_bwd: broadcast K / V (kv_bstride = 0) with B > 1, and Lq * Lk > 8192."""
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    t = torch.zeros((2, 128, 64), dtype=torch.float16, device=DEV)
    o = [torch.empty_like(t) for _ in range(3)]
    args = lambda B, Lq, Lk, kvb: (t.data_ptr(), 64, t.data_ptr(), 64, t.data_ptr(), 64, t.data_ptr(), 64, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                   B, 1, Lq, Lk, 64, Lq * 64, kvb, Lq * 64, 0.125, s)
    with pytest.raises(ValueError, match="broadcast"):
        _lib.check(lib.ldiff_op_attention_bwd(*args(2, 16, 16, 0)))
    with pytest.raises(ValueError, match="8192"):
        _lib.check(lib.ldiff_op_attention_bwd(*args(1, 128, 65, 65 * 64)))
    _lib.check(lib.ldiff_op_attention_bwd(*args(1, 128, 64, 0)))   # at the limit, one batch entry with kv_bstride 0: accepted
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------------------------
# 3. GroupNorm(+SiLU), LayerNorm, GEGLU, SiLU backward at the training widths
# ------------------------------------------------------------------------------------------------------------------------------------------
def _dsilu(a):
    s = torch.sigmoid(a)
    return s * (1 + a * (1 - s))


def _d2silu(a):
    s = torch.sigmoid(a)
    return s * (1 - s) * (2 + a * (1 - 2 * s))


def norm_backward_bound(x, dy, gamma_, beta_, eps, silu, reduce_dims, param_dims, n, nsum):
    """float64 reference of y = act(xhat gamma + beta) (act = SiLU or identity; xhat over `reduce_dims`, n elements per group) and of its
    backward (dgamma, dbeta summed over `param_dims`, nsum terms each), with a first-order per-element bound of the kernels' fp32 arithmetic
    (gn_train_fwd/bwd_kernel, ldiff_op_layernorm + ln_bwd_kernel).  g = gamma(.) of the module docstring:
      mean:   e_mu = g(n) mean|x|                rstd: rel e_r = g(n) mean(x^2) / var + 2 e_mu mean|x - mu| / var + 4u   (one- or two-pass
                                                       variance, rsqrtf)
      xhat:   e_xh = r e_mu + |xh| (e_r + 2u)    a = xh gamma + beta:  e_a = |gamma| e_xh + 2u (|xh gamma| + |beta|)
      SiLU:   the sigmoid (__expf, a division) to d = (8 + |a|) u relative, so act'(a) = s (1 + a (1 - s)) is within
              e_act' = (1 + 3|a|) s d + 3u s (1 + |a|) (absolute: act' passes through 0) and y = a s within |a| s d + u |y|
      da = dy act'(a):  e_da = |dy| (|act''(a)| e_a + e_act')          (zero without SiLU: da = dy)
      m1, m2 = the group means of da gamma and da gamma xh: the propagated errors + g(n) mean|terms|
      dx = r (da gamma - m1 - xh m2):  e_dx = |dx| e_r + r (|gamma| e_da + e_m1 + e_xh |m2| + |xh| e_m2 + 4u (|da gamma| + |m1| + |xh m2|))
      dgamma = sum da xh, dbeta = sum da (fp32 atomics, any order): the propagated errors + g(nsum) sum|terms|
    fp16 outputs add 2^-11 |ref| + 2^-24."""
    mean = lambda t: t.mean(reduce_dims, keepdim=True)
    mu = mean(x)
    xc = x - mu
    var = mean(xc * xc)
    r = 1.0 / torch.sqrt(var + eps)
    xh = xc * r
    a = xh * gamma_ + beta_
    if silu:
        sg = torch.sigmoid(a)
        act1, act2 = _dsilu(a), _d2silu(a).abs()
        dsg = (8 + a.abs()) * U
        e_act1 = (1 + 3 * a.abs()) * sg * dsg + 3 * U * sg * (1 + a.abs())
        y = a * sg
    else:
        act1, act2, e_act1, y = torch.ones_like(a), torch.zeros_like(a), torch.zeros_like(a), a
    da = dy * act1
    m1 = mean(da * gamma_)
    m2 = mean(da * gamma_ * xh)
    dx = r * (da * gamma_ - m1 - xh * m2)
    e_mu = gamma(n) * mean(x.abs())
    e_r = gamma(n) * mean(x * x) / (var + eps) + 2 * e_mu * mean(xc.abs()) / (var + eps) + 4 * U
    e_xh = r * e_mu + xh.abs() * (e_r + 2 * U)
    e_a = gamma_.abs() * e_xh + 2 * U * ((xh * gamma_).abs() + beta_.abs())
    e_da = dy.abs() * (act2 * e_a + e_act1)
    e_m1 = mean(gamma_.abs() * e_da) + gamma(n) * mean((da * gamma_).abs())
    e_m2 = mean(gamma_.abs() * (e_da * xh.abs() + da.abs() * e_xh)) + gamma(n) * mean((da * gamma_ * xh).abs())
    e_dx = dx.abs() * e_r + r * (gamma_.abs() * e_da + e_m1 + e_xh * m2.abs() + xh.abs() * e_m2
                                 + 4 * U * ((da * gamma_).abs() + m1.abs() + (xh * m2).abs()))
    e_y = (act1.abs() * e_a + a.abs() * sg * dsg + U * y.abs()) if silu else e_a
    dg = (da * xh).sum(param_dims)
    db = da.sum(param_dims)
    e_dg = (da.abs() * e_xh + xh.abs() * e_da).sum(param_dims) + gamma(nsum) * (da * xh).abs().sum(param_dims)
    e_db = e_da.sum(param_dims) + gamma(nsum) * da.abs().sum(param_dims)
    f16 = lambda ref, e: H16 * ref.abs() + e * (1 + H16) + U
    return {"y": (y, f16(y, e_y)), "dx": (dx, f16(dx, e_dx)), "dgamma": (dg, e_dg), "dbeta": (db, e_db)}


def _norm_inputs(shape, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = r16(torch.randn(shape, generator=g) * 1.5 + 0.3)
    dy = r16(torch.randn(shape, generator=g))
    gm, bt = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    return x, dy, gm, bt


UNET_WIDTHS = (320, 640, 960, 1280, 1920, 2560)
GN_CASES = [(2, hw, C, 32, 1e-5 if silu else 1e-6, silu) for hw in (64, 16, 4, 1) for C in UNET_WIDTHS for silu in (1, 0)] + \
           [(2, hw, C, 32, 1e-6, silu) for hw in (64, 256, 1024, 4096) for C in (128, 256, 512) for silu in (1, 0)]


@pytest.mark.parametrize("B,HW,C,groups,eps,silu", GN_CASES)
def test_group_norm_backward_at_the_step_widths(B, HW, C, groups, eps, silu):
    """GroupNormFn (ldiff_op_gn_train_fwd / _bwd) on NHWC [B, HW, C] (square maps) against norm_backward_bound."""
    x, dy, gm, bt = _norm_inputs((B, HW, C), C, HW * 7 + C + silu)
    Cg = C // groups
    xd = x.to(torch.float16).to(DEV).view(B, int(math.isqrt(HW)), -1, C).requires_grad_(True)
    gd, bd = gm.to(DEV).requires_grad_(True), bt.to(DEV).requires_grad_(True)
    y = ag.GroupNormFn.apply(xd, gd, bd, groups, eps, silu)
    y.backward(dy.to(torch.float16).to(DEV).view_as(y))
    grp = lambda t: t.double().view(B, HW, groups, Cg)
    ref = norm_backward_bound(grp(x), grp(dy), gm.double().view(groups, Cg), bt.double().view(groups, Cg), eps, silu, (1, 3), (0, 1), HW * Cg, B * HW)
    name = f"group norm B={B} HW={HW} C={C} silu={silu}"
    what = "group norm" + (" + silu" if silu else "")
    check_bound(y.float().cpu().view(B, HW, groups, Cg), *ref["y"], f"{name} y", what + " y")
    check_bound(xd.grad.float().cpu().view(B, HW, groups, Cg), *ref["dx"], f"{name} dx", what + " dx")
    rg, tg = ref["dgamma"]
    rb, tb = ref["dbeta"]
    check_bound(gd.grad.view(groups, Cg), rg, tg, f"{name} dgamma", what + " dgamma")
    check_bound(bd.grad.view(groups, Cg), rb, tb, f"{name} dbeta", what + " dbeta")


LN_CASES = [(B * L, C) for B in (2,) for L, C in ((64, 320), (16, 640), (4, 1280), (1, 1280))] + \
           [(rows, C) for rows in (128, 32, 8, 2) for C in (320, 640, 1280) if (rows, C) not in ((128, 320), (32, 640), (8, 1280), (2, 1280))]


@pytest.mark.parametrize("rows,C", LN_CASES)
def test_layer_norm_backward_at_the_step_widths(rows, C):
    """LayerNormFn (ldiff_op_layernorm / ldiff_op_ln_bwd) over rows = B * L against norm_backward_bound (eps 1e-5)."""
    x, dy, gm, bt = _norm_inputs((rows, C), C, rows * 13 + C)
    xd = x.to(torch.float16).to(DEV).requires_grad_(True)
    gd, bd = gm.to(DEV).requires_grad_(True), bt.to(DEV).requires_grad_(True)
    y = ag.LayerNormFn.apply(xd, gd, bd, 1e-5)
    y.backward(dy.to(torch.float16).to(DEV))
    ref = norm_backward_bound(x.double(), dy.double(), gm.double(), bt.double(), 1e-5, 0, (1,), (0,), C, rows)
    name = f"layer norm {rows}x{C}"
    for n, got in (("y", y), ("dx", xd.grad), ("dgamma", gd.grad), ("dbeta", bd.grad)):
        check_bound(got.float().cpu(), *ref[n], f"{name} {n}", f"layer norm {n}")


GEGLU_CASES = [(M, C4) for M in (128, 32, 8, 2) for C4 in (1280, 2560, 5120)]


@pytest.mark.parametrize("M,C4", GEGLU_CASES)
def test_geglu_backward_at_the_step_widths(M, C4):
    """GegluFn backward (geglu_bwd_kernel): dh = dy gelu(g), dg = dy h (Phi(g) + g phi(g)) in float64.  Bound per element: the products and
    sums of three or four fp32 values (6u relative each), erff to 4u absolute and __expf to 4u relative (on Phi and phi, which enter
    multiplied by |dy| and |dy h| (|g| phi); __expf(-g^2 / 2) to (4 + g^2) u relative), then the fp16 rounding."""
    g = torch.Generator().manual_seed(M + C4)
    x = r16(torch.randn((M, 2 * C4), generator=g) * 1.5)
    dy = r16(torch.randn((M, C4), generator=g))
    xd = x.to(torch.float16).to(DEV).requires_grad_(True)
    ag.GegluFn.apply(xd).backward(dy.to(torch.float16).to(DEV))
    h, gt, d = x[:, :C4].double(), x[:, C4:].double(), dy.double()
    cdf = 0.5 * (1 + torch.erf(gt / math.sqrt(2)))
    pdf = torch.exp(-0.5 * gt * gt) / math.sqrt(2 * math.pi)
    dh = d * gt * cdf
    dg = d * h * (cdf + gt * pdf)
    e_dh = 6 * U * dh.abs() + (d * gt).abs() * 4 * U
    e_dg = 6 * U * (d * h).abs() * (cdf + (gt * pdf).abs()) + (d * h).abs() * (4 * U + (gt * pdf).abs() * (4 + gt * gt) * U)
    ref = torch.cat([dh, dg], 1)
    tol = H16 * ref.abs() + torch.cat([e_dh, e_dg], 1) * (1 + H16) + U
    check_bound(xd.grad.float().cpu(), ref, tol, f"geglu {M}x{C4} dx", "geglu dx")


def test_silu_backward_at_the_time_embedding_width():
    """SiluFn on [2, 1280] (the time-embedding MLP): y and dx against float64.  The sigmoid (expf, a division) to d = (8 + |x|) u relative;
    d/dx x s(x) = s (1 + x (1 - s)) passes through 0, so its bound is absolute, (1 + 3|x|) s d + 3u s (1 + |x|); then the fp16 rounding."""
    g = torch.Generator().manual_seed(1280)
    x = r16(torch.randn((2, 1280), generator=g) * 3.0)
    dy = r16(torch.randn((2, 1280), generator=g))
    xd = x.to(torch.float16).to(DEV).requires_grad_(True)
    y = ag.silu(xd)
    y.backward(dy.to(torch.float16).to(DEV))
    xx, dd = x.double(), dy.double()
    yr = xx * torch.sigmoid(xx)
    dxr = dd * _dsilu(xx)
    sg, dsg = torch.sigmoid(xx), (8 + xx.abs()) * U
    e_dx = dd.abs() * ((1 + 3 * xx.abs()) * sg * dsg + 3 * U * sg * (1 + xx.abs())) + 2 * U * dxr.abs()
    check_bound(y.float().cpu(), yr, H16 * yr.abs() + xx.abs() * sg * dsg + U * yr.abs() + U, "silu y", "silu")
    check_bound(xd.grad.float().cpu(), dxr, H16 * dxr.abs() + e_dx + U, "silu dx", "silu")


# ------------------------------------------------------------------------------------------------------------------------------------------
# 4. every signature of the SD-1.5-width step has a case
# ------------------------------------------------------------------------------------------------------------------------------------------
def step_signatures(monkeypatch, Lk=6):
    """One eager forward + backward of the SD-1.5-width training step (synthetic weights, B = 2, 8 x 8 latents, one V5 pass) with the
    autograd functions' `apply` wrapped: {kind: set of signatures}."""
    from ldiffusion_amd import configs, train, weights
    from oracle import schedule
    sigs = {"conv": set(), "attn": set(), "gn": set(), "ln": set(), "geglu": set()}

    def wrap(cls, kind, sig_of):
        orig = cls.apply

        def apply(*a):
            sigs[kind].add(sig_of(*a))
            return orig(*a)
        monkeypatch.setattr(cls, "apply", apply)

    def conv_sig(x, w, b, stride=1, ups=0):
        B, H, W, Cx = x.shape
        return (B, H, W, Cx, w.shape[0], w.shape[1], w.shape[2] if w.dim() == 4 else 1, stride, ups, b is not None, w.requires_grad)
    wrap(ag.Conv2dFn, "conv", conv_sig)
    wrap(ag.AttentionFn, "attn", lambda q, k, v, heads: (q.shape[0], heads, q.shape[1], k.shape[1], q.shape[2] // heads))
    wrap(ag.GroupNormFn, "gn", lambda x, g, b, groups, eps, silu: (x.shape[0], x.shape[1] * x.shape[2], x.shape[3], groups, eps, int(silu)))
    wrap(ag.LayerNormFn, "ln", lambda x, g, b, eps: (x.numel() // x.shape[-1], x.shape[-1]))
    wrap(ag.GegluFn, "geglu", lambda x: (x.numel() // x.shape[-1], x.shape[-1] // 2))

    ucfg, vcfg = configs.SD15_UNET, configs.SD15_VAE
    unet = train.TrainableUNet(ucfg, weights.synthetic_state_dict(weights.unet_param_shapes(ucfg), 42, fp16_values=True), DEV)
    dec = train.FrozenVAEDecoder(vcfg, weights.synthetic_state_dict(weights.vae_param_shapes(vcfg), 43, fp16_values=True), DEV)
    g = torch.Generator().manual_seed(77)
    pw = (torch.randn((768, 768), generator=g) / 768 ** 0.5).to(DEV).requires_grad_(True)
    pb = (torch.randn(768, generator=g) * 0.05).to(DEV).requires_grad_(True)
    sch = schedule.PNDMOracle()
    sch.set_timesteps(1)
    ts = [int(t) for t in sch.timesteps]
    z0 = (torch.randn((2, 4, 8, 8), generator=g) * 0.8).to(DEV)
    u_list = [(torch.rand((2, 4, 8, 8), generator=g) * 1.98 - 0.99).to(DEV) for _ in ts]
    pairs = [[(int(torch.randint(0, 4096, (1,), generator=g)), int(torch.randint(0, 4096, (1,), generator=g)),
               torch.randint(0, 4096, (64,), generator=g).tolist()) for _ in range(6)] for _ in range(2)]
    ctx = train.text_projection((torch.randn((1, Lk, 768), generator=g) * 0.5).to(DEV), pw, pb)
    feats, _ = train.v5_features(unet, dec, z0, ctx, ts, sch.alphas_cumprod, u_list)
    loss = train.contrastive_loss(feats, pairs)
    (loss * train.LOSS_SCALE).backward()
    torch.cuda.synchronize()
    assert math.isfinite(loss.item())
    assert all(p.grad is not None for p in unet.p.values()) and pw.grad is not None
    return sigs


def covered():
    return {"conv": set(CONV_CASES), "attn": set(ATTN_CASES), "gn": set(GN_CASES), "ln": set(LN_CASES), "geglu": set(GEGLU_CASES)}


@pytest.mark.timeout(900)
def test_every_signature_of_the_step_has_a_case(lib, monkeypatch):
    """The SD-1.5-width step's Conv2dFn / AttentionFn / GroupNormFn / LayerNormFn / GegluFn signatures (one eager forward + backward, no
    CPU oracle) must all be cases of this file: routing is a function of shape, so the per-role kernels below are all pinned here."""
    sigs = step_signatures(monkeypatch)
    cov = covered()
    missing = {kind: sorted(s - cov[kind]) for kind, s in sigs.items() if s - cov[kind]}
    for kind, s in sigs.items():
        print(f"[step-sigs] {kind}: {len(s)} signatures")
    roles = {"forward": set(), "dgrad": set(), "wgrad": set()}
    for sig in sigs["conv"]:
        want = CONV_CASES.get(sig)
        if want:
            for role, names in zip(roles, want):
                if names:
                    roles[role] |= {names} if isinstance(names, str) else set(names)
    for role, names in roles.items():
        print(f"[step-kernels] {role}: {sorted(names)}")
    print(f"[step-kernels] attention backward: {sorted({ATTN_CASES[s] for s in sigs['attn'] if s in ATTN_CASES})}")
    assert not missing, "layer signatures of the step no case covers: " + "; ".join(f"{k}: {v}" for k, v in missing.items())


def pinned_kernels():
    """Every kernel a case of this file states it reaches (test_gpu_kernels.pinned_kernels takes these in)."""
    out = set(ATTN_CASES.values())
    for want in CONV_CASES.values():
        for names in want or ():
            if names:
                out |= {names} if isinstance(names, str) else set(names)
    return out


def teardown_module(module):
    if WORST:
        print("\n[bwd-err] worst measured error / bound per group: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))
