"""What one step of the tissue-head trainer (ldiffusion_amd/nnunet_train.py TrainableSegNet) asks of autograd.Conv2dFn and autograd.InstanceNormLReLUFn, stated
from the spec alone (no GPU), and a float64 reference of its transposed-conv path with the error model of tests/test_gpu_backward.py.

conv_signatures / norm_signatures are kept against the network itself by tests/test_gpu_nnunet_backward.py (one eager step with the two `apply`s wrapped) and
against a hand-written list by tests/test_cpu_nnunet_step_sigs.py.

The transposed conv.  TrainableSegNet.tconv runs ConvTranspose2d(kernel = stride = 2) as ag.linear on the weight viewed as [(di, dj, co), ci], bias.repeat(4),
then a depth-to-space permute; dW [ci, co, di, dj] and db reach the parameters through torch's view / repeat backward.  With u = 2^-24 and gamma(K) = 2 K u
(test_gpu_backward.py's: a K-term fp32 sum in any order, doubled for MFMA accumulation), per element:
    y  (fp16)  2^-11 |y| + gamma(cin + 1) (sum |x| |W| + |b|) + 2^-24           the linear's K is the cin inputs and the bias
    dx (fp16)  2^-11 |dx| + gamma(4 cout) sum |dy| |W| + 2^-24                    the dgrad GEMM runs over the 4 cout columns of the linear's output
    dW (fp32)  gamma(roundup(B h w, 8)) sum |x| |dy|                              the staged wgrad GEMM's K is the padded row count; on the direct route
               (chain + partials + 2) u sum |x| |dy| with the plan of ag.wgrad_plan (tests/wgrad_bound.py)
    db (fp32)  (gamma(B h w) + 3u) sum |dy|                                       the column sum over the rows gives 4 cout values (the direct route: its plan's
               chain + partials + 2 in place of 2 B h w); torch's backward of bias.repeat(4) then adds the four sub-pixels' values in fp32: three more roundings
The sub-pixel order is what the path can get wrong without the loss curve showing it, so the wrong references are the same function with di and dj exchanged
(y, dx and dW) and the bias gradient of the sub-pixel (0, 0) alone (db)."""
import torch

U = 2.0 ** -24
H16 = 2.0 ** -11


def gamma(K):
    return 2.0 * K * U


def _r(x, m):
    return (x + m - 1) // m * m


def level_sizes(spec, H, W):
    """(h, w) of the feature map of every stage for an H x W input."""
    out, h, w = [], H, W
    for st in spec["strides"]:
        h, w = (h - 1) // st + 1, (w - 1) // st + 1   # 3 x 3, padding 1
        out.append((h, w))
    return out


def conv_signatures(spec, B, H, W):
    """Every Conv2dFn.apply of one TrainableSegNet forward on a [B, in_channels, H, W] batch with all heads, in call order (a signature that several layers
    share appears once per layer): (B, H, W, Cx, Cout, Cin, k, stride, ups, has_bias, trainable) with H, W the conv's INPUT map, as tests/test_gpu_backward.py
    writes them.  The transposed convs are the linear layers they run as: rows [1, 1, B h w, cin] -> 4 cout columns."""
    f, n = spec["features"], spec["n_stages"]
    hw = level_sizes(spec, H, W)
    sigs = []
    h, w, cin = H, W, spec["in_channels"]
    for s in range(n):
        for i in range(spec["n_conv_encoder"][s]):
            st = spec["strides"][s] if i == 0 else 1
            sigs.append((B, h, w, _r(cin, 8), f[s], cin, 3, st, 0, True, True))
            h, w = hw[s]
            cin = f[s]
    for j in range(n - 1):
        below, skip = f[n - 1 - j], f[n - 2 - j]
        h, w = hw[n - 1 - j]
        sigs.append((1, 1, B * h * w, below, 4 * skip, below, 1, 1, 0, True, True))
        h, w = hw[n - 2 - j]
        cin = 2 * skip
        for i in range(spec["n_conv_decoder"][j]):
            sigs.append((B, h, w, cin, skip, cin, 3, 1, 0, True, True))
            cin = skip
        sigs.append((B, h, w, skip, spec["n_heads"], skip, 1, 1, 0, True, True))
    return sigs


def norm_signatures(spec, B, H, W):
    """(B, C, h, w) of every InstanceNormLReLUFn.apply of the same forward, in call order: one behind each 3 x 3 conv."""
    f, n = spec["features"], spec["n_stages"]
    hw = level_sizes(spec, H, W)
    out = []
    for s in range(n):
        out += [(B, f[s]) + hw[s]] * spec["n_conv_encoder"][s]
    for j in range(n - 1):
        out += [(B, f[n - 2 - j]) + hw[n - 2 - j]] * spec["n_conv_decoder"][j]
    return out


def transpconv_shapes(spec):
    """(cin, cout) of decoder.transpconvs.0 .. n_stages - 2."""
    f, n = spec["features"], spec["n_stages"]
    return [(f[n - 1 - j], f[n - 2 - j]) for j in range(n - 1)]


# ---- the transposed conv in float64 -----------------------------------------------------------------------------------------------------------------
def _sub(t):   # [B, C, 2h, 2w] -> [B, C, h, di, w, dj]
    B, C, H2, W2 = t.shape
    return t.view(B, C, H2 // 2, 2, W2 // 2, 2)


def _tconv(x, W, b, dy):
    y = torch.einsum("bcij,cokl->boikjl", x, W).reshape(dy.shape) + b.view(1, -1, 1, 1)
    dys = _sub(dy)
    dx = torch.einsum("boikjl,cokl->bcij", dys, W)
    dW = torch.einsum("bcij,boikjl->cokl", x, dys)
    return y, dx, dW, dys.sum((0, 2, 4))   # the last: the bias gradient per sub-pixel [co, di, dj]


def tconv_reference(x, W, b, dy, dw_plan=None, db_plan=None):
    """float64 y, dx, dW [ci, co, 2, 2], db of F.conv_transpose2d(x, W, b, stride=2) for the cotangent dy, their gamma terms (module docstring; e*) and the two
    wrong references.  x [B, ci, h, w], W [ci, co, 2, 2], b [co], dy [B, co, 2h, 2w], all float64.  dw_plan / db_plan: the plans of ag.wgrad_plan /
    ag.colsum_slabs_plan where the direct route formed dW / the column sums."""
    B, ci, h, w = x.shape
    co = W.shape[1]
    M = B * h * w
    y, dx, dW, dbs = _tconv(x, W, b, dy)
    Sy, Sdx, SdW, Sdbs = _tconv(x.abs(), W.abs(), b.abs(), dy.abs())
    out = dict(y=y, dx=dx, dw=dW, db=dbs.sum((1, 2)), M=M, Mpad=_r(M, 8))
    out["ey"] = gamma(ci + 1) * Sy
    out["edx"] = gamma(4 * co) * Sdx
    out["Kdw"] = _r(M, 8) if dw_plan is None else dw_plan["chain"] + dw_plan["partials"] + 2
    out["edw"] = (gamma(_r(M, 8)) if dw_plan is None else out["Kdw"] * U) * SdW
    cs = gamma(M) if db_plan is None else (db_plan["chain"] + db_plan["partials"] + 2) * U
    out["edb"] = (cs + 3 * U * (1 + cs)) * Sdbs.sum((1, 2))
    # di and dj exchanged: the function a weight view permute(3, 2, 1, 0) computes
    Wt = W.transpose(2, 3).contiguous()
    yw, dxw, dWw, _ = _tconv(x, Wt, b, dy)
    out["y_swapped"], out["dx_swapped"] = yw, dxw
    out["dw_swapped"] = dW.transpose(2, 3).contiguous()
    # the bias gradient of one sub-pixel only: what a backward that drops bias.repeat's sum returns
    out["db_one_subpixel"] = dbs[:, 0, 0].contiguous()
    return out


def f16_bound(ref, e):
    """an fp16 output: its own rounding on top of the fp32 error e (test_gpu_backward.py's f16)."""
    return H16 * ref.abs() + e * (1 + H16) + U


def tconv_case(cin, cout, B, h, w):
    """The inputs the GPU test feeds TrainableSegNet.tconv (fp16-representable values; the bias is not zero so that db's wrong reference differs)."""
    g = torch.Generator().manual_seed(cin * 7 + cout * 3 + B * 1000 + h * 31 + w)
    r16 = lambda t: t.to(torch.float16).to(torch.float32)
    x = r16(torch.randn((B, cin, h, w), generator=g))
    W = r16(torch.randn((cin, cout, 2, 2), generator=g) / cin ** 0.5)
    b = r16(torch.randn(cout, generator=g) * 0.1)
    dy = r16(torch.randn((B, cout, 2 * h, 2 * w), generator=g))
    return x, W, b, dy


TCONV_MAPS = [(2, 4, 4), (2, 16, 16), (1, 5, 7)]   # (B, h, w) of the input map
