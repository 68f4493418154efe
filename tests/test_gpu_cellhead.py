"""GPU (-m gpu): the cell head on the HIP library (include/ldiff.h ldiff_resnet_*, ldiffusion_amd/cellhead.py) -- its kernels alone through the C ABI
(clsconv through ldiff_op_conv, maxpool3x3s2, crop_resize_norm, cls_head), the whole classifier against the float64 restatement
(tests/resnet_ref.py), labels, batch invariance / graph replay / overflow detection, and Segmentor.inference_cell_model with `segmentor_weight` a
folder that holds cellclassifier.pth.

Error model of the conv cases (per element, on fp16-exact x, w, res and fp32 bias; derived, not tuned):
    |lib - f64| <= 2^-11 |f64| + (K + 2) 2^-24 (sum |x w| + |bias| + |res|)
the output's one fp16 rounding plus fp32 accumulation of the K products, the bias and the residual in any order."""
import contextlib
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kernel_routing
import resnet_ref
from ldiffusion_amd import _lib, cellhead
from ldiffusion_amd.models import ResNetClassifier

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
U16 = 2.0 ** -11


@contextlib.contextmanager
def reached(lib):
    """with reached(lib) as names: <launches>  ->  the conv / GEMM kernels the launches ran, the classifier's `clsconv<...>` among them, from the library's
    per-launch profiler (a block of its own: kernel_routing's inventory lists the kernels that existed before this family)."""
    names = set()
    torch.cuda.synchronize()
    lib.ldiff_prof_set_filter(None)
    _lib.prof_collect()                  # drop rows nobody collected
    lib.ldiff_prof_enable(1)
    try:
        yield names
    finally:
        try:
            torch.cuda.synchronize()
            names.update(r["name"] for r in _lib.prof_collect() if r["name"].startswith(kernel_routing.ROUTED_PREFIXES + ("clsconv<",)))
        finally:
            lib.ldiff_prof_enable(0)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def nhwc16(t, cpad=None):
    """[B, C, H, W] -> [B, H, W, cpad] float16 on the device, the channels past C zero."""
    B, Cc, H, W = t.shape
    cpad = cpad or Cc
    out = torch.zeros((B, H, W, cpad), dtype=torch.float16)
    out[..., :Cc] = t.permute(0, 2, 3, 1).to(torch.float16)
    return out.to(DEV)


# ---- 1. clsconv against float64 -------------------------------------------------------------------------------------------------------------------
def conv_args(x, w, bias, stride, res, relu, cls_conv, N=None):
    """ldiff_conv_args of a classifier conv; returns (args, y tensor, keep-alive list).  The input channels are stored padded to a multiple of 8."""
    B, Cin, H, W = x.shape
    Cout, _, ks, _ = w.shape
    cpad = (Cin + 7) // 8 * 8
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    xd = nhwc16(x, cpad)
    wm = torch.zeros((Cout, ks, ks, cpad), dtype=torch.float16)
    wm[..., :Cin] = w.permute(0, 2, 3, 1).to(torch.float16)
    wd, bd = wm.reshape(Cout, -1).contiguous().to(DEV), bias.float().contiguous().to(DEV)
    N = N or Cout
    y = torch.full((B, Ho, Wo, N), float("nan"), dtype=torch.float16, device=DEV)
    a = _lib.ConvArgs()
    a.x, a.C1, a.B, a.Hin, a.Win, a.Hout, a.Wout = xd.data_ptr(), cpad, B, H, W, Ho, Wo
    a.ks, a.stride, a.pad_t, a.pad_l = ks, stride, ks // 2, ks // 2
    a.w, a.N, a.Nrows, a.n_real, a.bias = wd.data_ptr(), N, Cout, N, bd.data_ptr()
    a.y, a.ldy = y.data_ptr(), N
    keep = [xd, wd, bd]
    if res is not None:
        rd = nhwc16(res)
        keep.append(rd)
        a.res, a.ld_res = rd.data_ptr(), res.shape[1]
    a.relu_out, a.cls_conv = int(relu), cls_conv
    return a, y, keep


def run_clsconv(lib, x, w, bias, stride, res, relu, cls_conv):
    a, y, keep = conv_args(x, w, bias, stride, res, relu, cls_conv)
    with reached(lib) as names:
        _lib.check(lib.ldiff_op_conv(C.byref(a), stream()))
    torch.cuda.synchronize()
    return y.permute(0, 3, 1, 2).double().cpu(), names


def conv_reference(x, w, bias, stride, res, relu):
    """(y float64, per-element bound of the module docstring)."""
    ks = w.shape[2]
    v = F.conv2d(x.double(), w.double(), bias.double(), stride=stride, padding=ks // 2)
    S = F.conv2d(x.double().abs(), w.double().abs(), bias.double().abs(), stride=stride, padding=ks // 2)
    if res is not None:
        v, S = v + res.double(), S + res.double().abs()
    y = F.relu(v) if relu else v
    K = ks * ks * x.shape[1]
    return y, U16 * y.abs() + (K + 2) * U * S


def assert_rejects_wrong(got, refs, tol, what):
    """The bound bites: each wrong reference leaves elements outside it."""
    for name, wrong in refs.items():
        bad = ((got - wrong).abs() > tol).float().mean().item()
        assert bad > 0.05, f"{what}: the bound accepts the wrong reference '{name}' ({bad:.3f} of the elements outside)"


# (ks, stride, Cin, Cout, H, W, B): 1x1 on a 4x4 map with M = 48 (no tile multiple); 1x1 stride 2; 3x3 on 2x2 and 1x1 maps (taps out of bounds);
# 3x3 stride 2 on an even and an odd map; the 7x7 stem with 3 channels stored as 8.  Cout 16 (one channel tile per workgroup), 64 and 256 (four).
CONV_CASES = [(1, 1, 64, 256, 4, 4, 3), (1, 2, 64, 16, 4, 4, 2), (3, 1, 32, 64, 2, 2, 2), (3, 1, 32, 16, 1, 1, 3), (3, 2, 16, 64, 8, 8, 2), (3, 2, 16, 16, 5, 5, 1),
              (7, 2, 3, 64, 16, 16, 2)]


def conv_operands(ks, stride, cin, cout, H, W, B, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn((B, cin, H, W), generator=g) * 1.2 + 0.2).to(torch.float16).float()
    w = (torch.randn((cout, cin, ks, ks), generator=g) * (2.0 / (ks * ks * cin)) ** 0.5).to(torch.float16).float()
    bias = torch.randn(cout, generator=g) * 0.3
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    res = (torch.randn((B, cout, Ho, Wo), generator=g) * 1.5).to(torch.float16).float()
    return x, w, bias, res


@pytest.mark.parametrize("ks,stride,cin,cout,H,W,B", CONV_CASES)
def test_clsconv_against_float64(lib, ks, stride, cin, cout, H, W, B):
    """Every case with and without the residual, with and without the ReLU: inside the derived bound, and the same bound rejects a shifted tap, a
    dropped ReLU and a dropped residual.  A launch with relu_out reaches the family by the executors' choice (cls_conv = 0), one without on request."""
    x, w, bias, res = conv_operands(ks, stride, cin, cout, H, W, B, ks * 1000 + cout * 10 + stride + H)
    stem = f"clsconv<{ks}x{ks},{64 if cout % 64 == 0 else 16}x16"
    for use_res in (False, True):
        for relu in (False, True):
            r = res if use_res else None
            got, names = run_clsconv(lib, x, w, bias, stride, r, relu, 0 if relu else 1)
            what = f"clsconv {ks}x{ks} s{stride} {cin}->{cout} {H}x{W} B={B} res={use_res} relu={relu}"
            kernel_routing.check_route(names, stem + (",relu>" if relu else ">"), what)
            y, tol = conv_reference(x, w, bias, stride, r, relu)
            assert got.shape == y.shape and torch.isfinite(got).all()
            ratio = ((got - y).abs() / tol).max().item()
            print(f"[clsconv] {what}: max err {(got - y).abs().max().item():.2e}, {ratio:.3f} of the bound")
            assert ratio <= 1.0, f"{what}: {int(((got - y).abs() > tol).sum())}/{y.numel()} elements outside the bound (worst {ratio:.2f})"
            shifted = torch.roll(w, 1, 3) if ks > 1 else torch.roll(w, 1, 1)   # (a 1x1 conv has one tap: its channels shifted instead)
            wrong = {"tap shifted": conv_reference(x, shifted, bias, stride, r, relu)[0]}
            if relu:
                wrong["ReLU dropped"] = conv_reference(x, w, bias, stride, r, False)[0]
            if use_res:
                wrong["residual dropped"] = conv_reference(x, w, bias, stride, None, relu)[0]
            assert_rejects_wrong(got, wrong, tol, what)


def test_clsconv_exact_on_integers(lib):
    """Small integers: every product and sum is exact in fp32 and the result in fp16, so the fragment maps are checked to the bit."""
    g = torch.Generator().manual_seed(7)
    for ks, stride, cin, cout, H, W, B in [(3, 2, 16, 64, 7, 6, 3), (1, 1, 24, 16, 3, 5, 2), (7, 2, 3, 16, 9, 10, 1), (3, 1, 8, 256, 4, 4, 5)]:
        x = torch.randint(-3, 4, (B, cin, H, W), generator=g).float()
        w = torch.randint(-2, 3, (cout, cin, ks, ks), generator=g).float()
        bias = torch.randint(-4, 5, (cout,), generator=g).float()
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        res = torch.randint(-5, 6, (B, cout, Ho, Wo), generator=g).float()
        for relu in (False, True):
            got, _ = run_clsconv(lib, x, w, bias, stride, res, relu, 1)
            want = F.conv2d(x.double(), w.double(), bias.double(), stride=stride, padding=ks // 2) + res.double()
            want = F.relu(want) if relu else want
            assert want.abs().max().item() < 2048 and torch.equal(got, want), f"{ks}x{ks} s{stride} {cin}->{cout} relu={relu}"


def test_clsconv_sum_does_not_depend_on_batch_or_tile(lib):
    """A batch large enough for the 64-pixel wave tile (M = 32768) equals its images run alone (16-pixel wave tile) bit for bit."""
    g = torch.Generator().manual_seed(8)
    x = torch.randn((32, 64, 32, 32), generator=g).to(torch.float16).float()
    w = (torch.randn((256, 64, 1, 1), generator=g) * 0.18).to(torch.float16).float()
    bias = torch.randn(256, generator=g) * 0.3
    big, names = run_clsconv(lib, x, w, bias, 1, None, True, 0)
    kernel_routing.check_route(names, "clsconv<1x1,64x64,relu>", "B = 32")
    for i in (0, 17, 31):
        one, names = run_clsconv(lib, x[i:i + 1], w, bias, 1, None, True, 0)
        kernel_routing.check_route(names, "clsconv<1x1,64x16,relu>", "B = 1")
        assert torch.equal(one[0], big[i])


def test_clsconv_routing(lib):
    """relu_out is never routed elsewhere: an ineligible shape or cls_conv = -1 is LDIFF_ERR_INVALID; a plain launch of an eligible shape keeps the route
    it always had (cls_conv = 0) and reaches the family only on request."""
    x, w, bias, _ = conv_operands(3, 1, 32, 64, 4, 4, 2, 9)
    a, y, keep = conv_args(x, w, bias, 1, None, True, -1)
    with pytest.raises(ValueError, match="relu_out"):
        _lib.check(lib.ldiff_op_conv(C.byref(a), stream()))
    x2, w2, bias2, _ = conv_operands(3, 1, 32, 24, 4, 4, 2, 10)      # 24 output channels: not a multiple of 16
    a, y, keep = conv_args(x2, w2, bias2, 1, None, True, 0)
    with pytest.raises(ValueError, match="relu_out"):
        _lib.check(lib.ldiff_op_conv(C.byref(a), stream()))
    a, y, keep = conv_args(x, w, bias, 1, None, True, 0)
    a.pad_t = 0                                                         # padding other than ks / 2
    with pytest.raises(ValueError, match="relu_out"):
        _lib.check(lib.ldiff_op_conv(C.byref(a), stream()))
    for field, value in (("silu_out", 1), ("cond_conv", 1), ("seg_conv", 1), ("lrelu_in", 1), ("tconv", 1)):   # another family's selector beside relu_out: refused, not taken there
        a, y, keep = conv_args(x, w, bias, 1, None, True, 0)
        setattr(a, field, value)
        with pytest.raises(ValueError, match="relu_out"):
            _lib.check(lib.ldiff_op_conv(C.byref(a), stream()))
    xs, ws, bs, _ = conv_operands(3, 1, 8, 16, 8, 8, 1, 11)            # a shape of the conditioning-embedding kernel AND of this family: relu_out + silu_out is refused
    a, y, keep = conv_args(xs, ws, bs, 1, None, True, 0)
    a.silu_out = 1
    with pytest.raises(ValueError, match="relu_out"):
        _lib.check(lib.ldiff_op_conv(C.byref(a), stream()))
    a, y, keep = conv_args(x, w, bias, 1, None, True, 0)               # a folded shortcut beside relu_out: refused, never dropped
    a.sc_x, a.sc_C, a.sc_w = keep[0].data_ptr(), 32, keep[1].data_ptr()
    with pytest.raises(ValueError, match="relu_out"):
        _lib.check(lib.ldiff_op_conv(C.byref(a), stream()))
    a, y, keep = conv_args(x, w, bias, 1, None, False, 0)              # plain: the route such a launch had before the family existed
    with reached(lib) as names:
        _lib.check(lib.ldiff_op_conv(C.byref(a), stream()))
    assert names and not any(n.startswith("clsconv<") for n in names), names
    torch.cuda.synchronize()
    ref, tol = conv_reference(x, w, bias, 1, None, False)
    assert ((y.permute(0, 3, 1, 2).double().cpu() - ref).abs() <= tol).all()


# ---- 2. maxpool3x3s2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(6, 6), (7, 5)])
def test_maxpool_exact(lib, H, W):
    x = torch.randn((3, 16, H, W), generator=torch.Generator().manual_seed(H * 10 + W)).to(torch.float16)
    want = F.max_pool2d(x.float(), 3, 2, 1)
    Ho, Wo = want.shape[2:]
    y = torch.full((3, Ho, Wo, 16), float("nan"), dtype=torch.float16, device=DEV)
    xd = nhwc16(x.float())
    _lib.check(lib.ldiff_op_maxpool3x3s2(_lib.ptr(xd), _lib.ptr(y), 3, H, W, 16, stream()))
    assert torch.equal(y.permute(0, 3, 1, 2).float().cpu(), want)
    with pytest.raises(ValueError, match="multiple of 8"):
        _lib.check(lib.ldiff_op_maxpool3x3s2(_lib.ptr(xd), _lib.ptr(y), 3, H, W, 12, stream()))


# ---- 3. crop_resize_norm --------------------------------------------------------------------------------------------------------------------------
def reference_crops(rgb, boxes, S=64, antialias=True):
    """The reference's chain in float64: normalise in float32 (what the head is handed), numpy's own wrapping cast, / 255, anti-aliased bilinear
    resize, normalise.  [n, 3, S, S] float64."""
    mean32, std32 = np.asarray(cellhead.IMAGENET_MEAN, np.float32), np.asarray(cellhead.IMAGENET_STD, np.float32)
    image = (rgb.astype(np.float32) / np.float32(255.0) - mean32) / std32
    mean, std = torch.tensor(cellhead.IMAGENET_MEAN, dtype=torch.float64).view(1, 3, 1, 1), torch.tensor(cellhead.IMAGENET_STD, dtype=torch.float64).view(1, 3, 1, 1)
    out = []
    for x1, y1, x2, y2 in boxes:
        with np.errstate(invalid="ignore"):
            patch = (image[y1:y2 + 1, x1:x2 + 1] * 255).astype(np.uint8)
        t = torch.from_numpy(patch).permute(2, 0, 1)[None].double() / 255.0
        t = F.interpolate(t, size=(S, S), mode="bilinear", antialias=antialias, align_corners=False)
        out.append((t - mean) / std)
    return torch.cat(out)


def fp16_ulp(v):
    """Spacing of fp16 at |v| (float64 tensor), subnormal spacing below 2^-14."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 10)


def lib_crops(lib, rgb, boxes, S=64):
    rgb_d = torch.from_numpy(rgb).to(DEV)
    boxes_d = torch.tensor(boxes, dtype=torch.int32, device=DEV)
    lut = torch.from_numpy(cellhead.build_lut()).to(DEV)
    out = torch.full((len(boxes), S, S, 8), float("nan"), dtype=torch.float16, device=DEV)
    mean, std = (C.c_double * 3)(*cellhead.IMAGENET_MEAN), (C.c_double * 3)(*cellhead.IMAGENET_STD)
    _lib.check(lib.ldiff_op_crop_resize_norm(_lib.ptr(rgb_d), rgb.shape[0], rgb.shape[1], _lib.ptr(boxes_d), len(boxes), _lib.ptr(lut), S, mean, std, _lib.ptr(out), stream()))
    torch.cuda.synchronize()
    return out.cpu()


def test_crop_resize_norm_against_float64(lib):
    """Boxes of 5 x 5 (upsampled: plain bilinear), 64 x 64 (identity), 65 x 90 and 200 x 37 (anti-aliased, one axis or both), two of them on the image
    border.  Every output within one fp16 ulp of the float64 value (half an ulp is the rounding's)."""
    rgb = np.random.default_rng(3).integers(0, 256, (128, 256, 3), dtype=np.uint8)
    boxes = [(3, 4, 7, 8), (10, 10, 73, 73), (100, 38, 164, 127), (56, 0, 255, 36)]
    got = lib_crops(lib, rgb, boxes)
    want = reference_crops(rgb, boxes)
    assert (got[..., 3:] == 0).all()
    g = got[..., :3].permute(0, 3, 1, 2).double()
    ratio = ((g - want).abs() / fp16_ulp(want)).amax((1, 2, 3))
    print(f"[crops] worst error in fp16 ulps per box: {[round(r, 3) for r in ratio.tolist()]}")
    assert (ratio <= 1.0).all()
    assert torch.equal(g[1], want[1].to(torch.float16).double())        # 64 x 64 -> 64 x 64: one tap of weight 1
    # the bound bites: the same crops without anti-aliasing, and the crop shifted by one pixel
    for name, wrong in {"no antialias": reference_crops(rgb, [boxes[3]], antialias=False), "shifted": reference_crops(rgb, [(57, 0, 255, 36)])}.items():
        assert ((g[3:4] - wrong).abs() > fp16_ulp(want[3:4])).float().mean().item() > 0.5, name
    zero = lib_crops(lib, rgb, [(250, 10, 260, 20)])                     # leaves the image: a zero crop, nothing read outside
    assert (zero == 0).all()


# ---- 4. cls_head ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,HW,A,NC", [(5, 4, 256, 6), (3, 1, 32, 2), (2, 9, 80, 4)])
def test_cls_head_against_float64(lib, B, HW, A, NC):
    g = torch.Generator().manual_seed(B * 100 + HW)
    x = torch.randn((B, HW, A), generator=g).to(torch.float16)
    w, bias = torch.randn((NC, A), generator=g) / A ** 0.5, torch.randn(NC, generator=g) * 0.2
    logits = torch.full((B, NC), float("nan"), dtype=torch.float32, device=DEV)
    labels = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
    _lib.check(lib.ldiff_op_cls_head(_lib.ptr(xd), B, HW, A, A, _lib.ptr(wd), _lib.ptr(bd), NC, _lib.ptr(logits), _lib.ptr(labels), stream()))
    torch.cuda.synchronize()
    feat = x.double().mean(1)
    want = feat @ w.double().T + bias.double()
    tol = 256 * U * (feat.abs() @ w.double().abs().T)
    err = (logits.double().cpu() - want).abs()
    print(f"[cls_head] B={B} HW={HW} A={A}: worst {(err / tol).max().item():.4f} of the bound")
    assert (err <= tol).all()
    top = want[:, 1:].topk(min(2, NC - 1), 1).values
    clear = torch.ones(B, dtype=torch.bool) if NC == 2 else (top[:, 0] - top[:, 1]) > 2 * tol.amax(1)
    assert clear.any() and torch.equal(labels.cpu().long()[clear], (want[:, 1:].argmax(1) + 1)[clear])
    wrong = feat @ torch.roll(w.double(), 1, 1).T + bias.double()
    assert ((logits.double().cpu() - wrong).abs() > tol).float().mean().item() > 0.5
    logits2 = torch.empty_like(logits)
    _lib.check(lib.ldiff_op_cls_head(_lib.ptr(xd), B, HW, A, A, _lib.ptr(wd), _lib.ptr(bd), NC, _lib.ptr(logits2), None, stream()))   # labels may be NULL
    assert torch.equal(logits2, logits)


# ---- 5. the whole classifier against float64 -----------------------------------------------------------------------------------------------------
REDUCED = dict(layers=(1, 1, 2, 1), width=16, adapter=64, S=32)
FULL = dict(layers=(3, 8, 36, 3), width=64, adapter=256, S=64)        # ResNet152
NC = 4
# (name, B, seed).  The full-size seed was chosen on the CPU so that the float64 reference alone has no crop inside twice the fp16-storage model's error.
NETWORK_CASES = [("reduced", 1, 21), ("reduced", 5, 22), ("full", 12, 13)]
# Measured on the MI355X, per case: (max |lib - f64| / max |fp16-storage model - f64| over the logits, max |lib - f64| in logit units).  The asserted factor of a
# case is twice its measured ratio; the labels' tie margin is twice its measured error.
MEASURED = {("reduced", 1, 21): (0.817, 4.221e-03), ("reduced", 5, 22): (1.339, 5.112e-03), ("full", 12, 13): (0.796, 3.588e-02)}


def spec_of(name):
    return REDUCED if name == "reduced" else FULL


def build_case(spec, B, seed, bn3_gain=0.25):
    """Weights, crops, the classifier fitted on the float64 features of these crops, float64 logits and the fp16-storage model's."""
    sd = resnet_ref.synthetic_state_dict(spec["layers"], spec["width"], NC, seed, bn3_gain, spec["adapter"])
    n_fit = max(B, 8)   # the classifier is fitted on at least 8 crops (one crop has no spread); the case uses the first B
    x = torch.randn((n_fit, 3, spec["S"], spec["S"]), generator=torch.Generator().manual_seed(seed + 100)).to(torch.float16).float()
    feat = resnet_ref.forward(sd, spec["layers"], x, torch.float64, return_features=True)
    sd = resnet_ref.fit_classifier(sd, feat, seed + 1)
    x, feat = x[:B], feat[:B]
    w, b = sd["classifier.weight"].double(), sd["classifier.bias"].double()
    model_feat = resnet_ref.forward(sd, spec["layers"], x, torch.float64, store=resnet_ref.fp16_storage, return_features=True)
    return dict(sd=sd, x=x, ref=F.linear(feat, w, b), model=F.linear(model_feat, w, b))


@functools.lru_cache(maxsize=None)
def network_case(name, B, seed):
    spec = spec_of(name)
    c = build_case(spec, B, seed)
    net = ResNetClassifier(NC, c["sd"], DEV, spec["layers"], spec["width"], spec["adapter"])
    logits, labels = net(resnet_ref.to_nhwc8(c["x"]).to(DEV))
    net.check_finite()
    c.update(net=net, got=logits.double().cpu(), labels=labels.long().cpu())
    return c


@pytest.mark.parametrize("name,B,seed", NETWORK_CASES)
def test_network_logits_against_float64(name, B, seed):
    """Logits of the whole classifier against the float64 restatement (un-folded BatchNorm).  Yardstick: the same restatement with the weights and every
    stored tensor rounded to fp16.  The library rounds once per fused conv + BatchNorm (+ add) + ReLU and keeps the pooling and the head in fp32, so it
    should sit at or under the model; a ratio above 2 would mean fp32 sums are being lost.  Asserted: twice the measured ratio."""
    c = network_case(name, B, seed)
    e_lib, e_model = (c["got"] - c["ref"]).abs().max().item(), (c["model"] - c["ref"]).abs().max().item()
    spread = c["ref"].std().item()
    print(f"[network] {name} B={B}: lib {e_lib:.3e}, fp16-storage model {e_model:.3e} (logit spread {spread:.2f}), ratio {e_lib / e_model:.3f}")
    assert c["got"].shape == c["ref"].shape == (B, NC)
    m = 2.0 * MEASURED[(name, B, seed)][0]
    assert e_lib <= m * e_model, f"{name} B={B}: lib error {e_lib:.3e} is {e_lib / e_model:.2f} x the fp16-storage model's {e_model:.3e} (asserted: {m:.2f} x)"


@pytest.mark.parametrize("name,B,seed", NETWORK_CASES)
def test_network_labels_against_float64(name, B, seed):
    """A crop's class may differ from float64's only where the float64 gap between its two best classes among 1 .. C - 1 is at most twice the logit error
    recorded for the case (MEASURED: a recorded figure, not this run's); at most 2 of the 12 full-size crops may sit inside that margin."""
    c = network_case(name, B, seed)
    e_lib = MEASURED[(name, B, seed)][1]
    top = c["ref"][:, 1:].topk(2, 1).values
    inside = (top[:, 0] - top[:, 1]) <= 2 * e_lib
    want = resnet_ref.labels_of(c["ref"])
    differ = c["labels"] != want
    print(f"[labels] {name} B={B}: lib {c['labels'].tolist()}, float64 {want.tolist()}, {int(inside.sum())} inside the margin, {int(differ.sum())} differ")
    assert torch.equal(c["labels"], resnet_ref.labels_of(c["got"])), "the kernel's label is not the arg-max of its own logits"
    assert not (differ & ~inside).any()
    if name == "full":
        assert int(inside.sum()) <= 2 and len(set(want.tolist())) >= 2


# ---- 6. batch invariance, graph replay, overflow, load errors -------------------------------------------------------------------------------------
def test_batch_invariance_and_graph_replay():
    c = network_case("reduced", 5, 22)
    spec = REDUCED
    x = resnet_ref.to_nhwc8(c["x"]).to(DEV)
    eager = ResNetClassifier(NC, c["sd"], DEV, spec["layers"], spec["width"], spec["adapter"]).set_graph(False)
    ref_logits, ref_labels = eager(x)
    assert eager.graph_replays == 0
    net = ResNetClassifier(NC, c["sd"], DEV, spec["layers"], spec["width"], spec["adapter"])
    outs = [net(x) for _ in range(4)]        # eager, capture + replay, replay, replay
    assert net.graph_replays == 3
    for lo, la in outs:
        assert torch.equal(lo, ref_logits) and torch.equal(la, ref_labels)
    ones = [net(x[i:i + 1]) for i in range(5)]
    assert torch.equal(torch.cat([o[0] for o in ones]), ref_logits), "B = 5 differs from five B = 1 calls"
    assert torch.equal(torch.cat([o[1] for o in ones]), ref_labels)
    net.check_finite()
    with pytest.raises(ValueError, match="S = 48"):
        net(torch.zeros((1, 48, 48, 8), dtype=torch.float16, device=DEV))


def test_graph_cache_lifecycle():
    """The replay cache through its states on one handle: eager, capture, replays; off and on again; another batch in between; a reloaded checkpoint
    (whole: a folded group is reloaded whole).  Every output equals an eager twin's bit for bit, and the replay counter moves exactly when a graph was launched."""
    spec = REDUCED
    make = lambda sd: ResNetClassifier(NC, sd, DEV, spec["layers"], spec["width"], spec["adapter"])
    sd = network_case("reduced", 5, 22)["sd"]
    sd2 = resnet_ref.synthetic_state_dict(spec["layers"], spec["width"], NC, 23, 0.25, spec["adapter"])
    x = resnet_ref.to_nhwc8(torch.randn((2, 3, spec["S"], spec["S"]), generator=torch.Generator().manual_seed(24))).to(DEV)
    same = lambda got, ref: torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    ref = make(sd).set_graph(False)(x)
    net = make(sd)
    outs = [net(x) for _ in range(4)]        # eager, capture + replay, replay, replay
    assert net.graph_replays == 3
    assert all(same(o, ref) for o in outs)
    net.set_graph(False)
    assert same(net(x), ref) and net.graph_replays == 3
    net.set_graph(True)
    outs = [net(x) for _ in range(3)]        # the graph went with set_graph(False): eager, capture + replay, replay
    assert net.graph_replays == 5
    assert all(same(o, ref) for o in outs)
    assert same(net(x[:1]), (ref[0][:1], ref[1][:1]))   # another batch in between drops the cached graph
    for _ in range(2):
        assert same(net(x), ref)
    net.load_state_dict(sd2)
    ref2 = make(sd2).set_graph(False)(x)
    assert not torch.equal(ref2[0], ref[0])
    for _ in range(3):
        assert same(net(x), ref2), "a replay of the graph captured with the first checkpoint"
    net.check_finite()


def test_batch_invariance_at_full_size():
    c = network_case("full", 12, 13)
    x = resnet_ref.to_nhwc8(c["x"]).to(DEV)
    got = c["net"](x)[0]
    one = torch.cat([c["net"](x[i:i + 1])[0] for i in (0, 5, 11)])
    assert torch.equal(one, got[[0, 5, 11]])


def test_overflow_trips_check_finite():
    """bn3 gamma ~ 1: every block adds a full-size branch to the stream, which passes fp16's range in layer 3 of the 50-block network."""
    spec = FULL
    sd = resnet_ref.synthetic_state_dict(spec["layers"], spec["width"], NC, 31, 1.0, spec["adapter"])
    net = ResNetClassifier(NC, sd, DEV, spec["layers"], spec["width"], spec["adapter"])
    net(resnet_ref.to_nhwc8(torch.randn((1, 3, 64, 64), generator=torch.Generator().manual_seed(1))).to(DEV))
    with pytest.raises(_lib.NonFiniteError):
        net.check_finite()
    net.check_finite()   # the flag is cleared once reported


def test_load_errors():
    spec = REDUCED
    sd = resnet_ref.synthetic_state_dict(spec["layers"], spec["width"], NC, 32, 0.25, spec["adapter"])
    with pytest.raises(RuntimeError, match="missing"):
        ResNetClassifier(NC, {k: v for k, v in sd.items() if k != "encoder.6.1.bn2.running_mean"}, DEV, spec["layers"], spec["width"], spec["adapter"])
    with pytest.raises(ValueError, match="does not match"):
        ResNetClassifier(NC, dict(sd, **{"adapter.weight": torch.zeros((spec["adapter"], 512, 1, 1))}), DEV, spec["layers"], spec["width"], spec["adapter"])
    with pytest.raises(ValueError, match="width"):
        ResNetClassifier(NC, sd, DEV, spec["layers"], 24, spec["adapter"])
    ResNetClassifier(NC, dict(sd, **{"encoder.1.num_batches_tracked": torch.tensor(7)}), DEV, spec["layers"], spec["width"], spec["adapter"])   # accepted and dropped


def test_partial_reload_of_a_folded_group():
    """A conv is folded with its BatchNorm at the first forward, so one tensor of the group alone cannot be reloaded: the next forward refuses it and names
    the rule.  The group's five tensors loaded together are taken, and the output is a fresh handle's built from the same values, bit for bit."""
    spec = REDUCED
    make = lambda sd: ResNetClassifier(NC, sd, DEV, spec["layers"], spec["width"], spec["adapter"])
    sd = network_case("reduced", 5, 22)["sd"]
    x = resnet_ref.to_nhwc8(torch.randn((2, 3, spec["S"], spec["S"]), generator=torch.Generator().manual_seed(25))).to(DEV)
    group = ["encoder.4.0.conv1.weight"] + ["encoder.4.0.bn1." + v for v in ("weight", "bias", "running_mean", "running_var")]
    gamma = sd["encoder.4.0.bn1.weight"] * 1.5 + 0.25
    net = make(sd)
    before = net(x)
    net.load_state_dict({"encoder.4.0.bn1.weight": gamma})
    with pytest.raises(RuntimeError, match="was folded"):
        net(x)
    sd2 = dict(sd, **{"encoder.4.0.bn1.weight": gamma})
    net.load_state_dict({k: sd2[k] for k in group})
    got, ref = net(x), make(sd2).set_graph(False)(x)
    assert not torch.equal(ref[0], before[0]), "the reloaded gamma must change the logits"
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    net.check_finite()


# ---- 7. end to end --------------------------------------------------------------------------------------------------------------------------------
# Measured on the MI355X for the end-to-end case below: max |lib - f64| over the logits of its 31 instances.  The tie margin is twice this figure, and the run's own
# error is asserted against twice it.
E2E_MEASURED_LOGIT_ERROR = 5.962e-03


def synthetic_label_map(H=1024, W=1024, seed=4):
    """About 30 discs and rectangles, two of them below the size rule (4 pixels high / wide)."""
    rng = np.random.default_rng(seed)
    m = np.zeros((H, W), np.int64)
    yy, xx = np.mgrid[:H, :W]
    k = 1
    for gy in range(5):
        for gx in range(6):
            cy, cx = 100 + gy * 190 + int(rng.integers(-20, 21)), 90 + gx * 165 + int(rng.integers(-20, 21))
            if (gy + gx) % 2 == 0:
                r = int(rng.integers(6, 60))
                m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = k
            else:
                h, w = int(rng.integers(5, 75)), int(rng.integers(5, 75))
                m[cy - h:cy + h, cx - w:cx + w] = k
            k += 3
    m[10:14, 500:530] = 200     # 4 rows: skipped
    m[900:960, 1000:1004] = 201  # 4 columns: skipped
    m[1000:1024, 0:30] = 202    # on the border
    return m


@pytest.fixture(scope="module")
def tiny():
    from ldiffusion_amd import configs, weights
    from ldiffusion_amd.models import AutoencoderKL, UNet2DConditionModel
    ucfg, vcfg = configs.TINY_UNET, configs.TINY_VAE
    usd = weights.synthetic_state_dict(weights.unet_param_shapes(ucfg), 42, fp16_values=True)
    vsd = weights.synthetic_state_dict(weights.vae_param_shapes(vcfg), 43, fp16_values=True)
    return dict(unet=UNet2DConditionModel(ucfg, usd, DEV), vae=AutoencoderKL(vcfg, vsd, DEV))


def test_segmentor_inference_cell_model_from_a_checkpoint_folder(tiny, tmp_path):
    """segmentor.py:490-545 with `segmentor_weight` = a folder holding cellclassifier.pth and the label map injected as `instances=`: the mask equals the
    float64 head's classes painted over the same label map of the same decoded image (instances inside the tie margin excepted), skipped instances and
    the background are 0, and the result is NEAREST-resized to the input size."""
    from PIL import Image
    from ldiffusion_amd.segmentor import Segmentor
    sd_dir, w_dir, seg_dir = tmp_path / "sd", tmp_path / "train_save" / "unet" / "25_01_01", tmp_path / "segmentor"
    tiny["unet"].save_pretrained(str(sd_dir / "unet"))
    tiny["vae"].save_pretrained(str(sd_dir / "vae"))
    tiny["unet"].save_pretrained(str(w_dir))
    os.makedirs(seg_dir)
    img = (np.random.default_rng(5).random((96, 80, 3)) * 255).astype(np.uint8)
    path = tmp_path / "roi.png"
    Image.fromarray(img).save(path)
    ctx = (torch.randn((1, 6, 64), generator=torch.Generator().manual_seed(2)) * 0.5).to(DEV)
    labels = synthetic_label_map()
    seen = {}

    def instances(image):
        seen["image"] = np.array(image)
        return labels

    spec = REDUCED
    sd = resnet_ref.synthetic_state_dict(spec["layers"], spec["width"], NC, 41, 0.25, spec["adapter"])
    seg = Segmentor(None, None, "cell", NC)
    # first pass with any classifier: what the decoded image is (the label map's callable sees it), so that the classifier can be fitted on its crops
    torch.save(sd, seg_dir / "cellclassifier.pth")
    seg.inference_cell_model(str(path), str(sd_dir), str(w_dir), str(seg_dir), text_embeddings=ctx, instances=instances)
    image = seen["image"]
    assert image.shape == (1024, 1024, 3) and image.dtype == np.float32
    mean, std = np.asarray(cellhead.IMAGENET_MEAN, np.float32), np.asarray(cellhead.IMAGENET_STD, np.float32)
    rgb = np.clip(np.rint((image.astype(np.float64) * std + mean) * 255.0), 0, 255).astype(np.uint8)
    assert np.allclose((rgb.astype(np.float32) / np.float32(255.0) - mean) / std, image, rtol=1e-6, atol=1e-6), "the head is not handed the normalised decoded image"
    ids, boxes = cellhead.instance_boxes(torch.from_numpy(labels))
    assert 25 <= ids.numel() <= 40 and 200 not in ids.tolist() and 201 not in ids.tolist() and 202 in ids.tolist()
    crops = reference_crops(rgb, boxes.tolist(), 64)     # (the head's crop size is the reference's 64, whatever the network's depth)
    feat = resnet_ref.forward(sd, spec["layers"], crops, torch.float64, return_features=True)
    sd = resnet_ref.fit_classifier(sd, feat, 42)
    ref = F.linear(feat, sd["classifier.weight"].double(), sd["classifier.bias"].double())
    want = resnet_ref.labels_of(ref)
    assert len(set(want.tolist())) >= 2
    torch.save(sd, seg_dir / "cellclassifier.pth")
    os.utime(seg_dir / "cellclassifier.pth", (1, 1))     # (a new mtime: the cached head is rebuilt)
    decoded, mask = seg.inference_cell_model(str(path), str(sd_dir), str(w_dir), str(seg_dir), text_embeddings=ctx, instances=instances)
    assert decoded.size == (80, 96) and mask.shape == (96, 80) and mask.dtype == np.uint8
    top = ref[:, 1:].topk(2, 1).values
    tie = (top[:, 0] - top[:, 1]) <= 2 * E2E_MEASURED_LOGIT_ERROR
    lib_logits, _ = seg._cell_head(str(seg_dir)).classify(torch.from_numpy(rgb).to(DEV), boxes.to(DEV))
    e_run = (lib_logits.double().cpu() - ref).abs().max().item()
    print(f"[e2e] {ids.numel()} instances, classes {sorted(set(want.tolist()))}, {int(tie.sum())} inside the tie margin; max |lib - f64| over the logits {e_run:.3e}")
    assert e_run <= 2 * E2E_MEASURED_LOGIT_ERROR, f"logit error {e_run:.3e} against the recorded {E2E_MEASURED_LOGIT_ERROR:.3e}"
    assert int(tie.sum()) <= 2, "too many instances inside the tie margin: change the classifier's seed (none were at the recorded figure)"
    paint = np.zeros(int(labels.max()) + 1, np.uint8)
    paint[ids.numpy()] = want.numpy().astype(np.uint8)
    ambiguous = np.zeros(int(labels.max()) + 1, np.uint8)
    ambiguous[ids.numpy()[tie.numpy()]] = 1
    nearest = lambda a: np.array(Image.fromarray(a).resize((80, 96), resample=Image.NEAREST))
    want_mask, amb = nearest(paint[labels]), nearest(ambiguous[labels]).astype(bool)
    assert (want_mask > 0).any() and np.array_equal(mask[~amb], want_mask[~amb])
    skipped = nearest(np.isin(labels, (0, 200, 201)).astype(np.uint8)).astype(bool)
    assert (mask[skipped] == 0).all()
    # the head= protocol still works, and the built head fits it: one-hot [1, C, H, W]
    head = seg._cell_head(str(seg_dir))
    x = torch.from_numpy(image).permute(2, 0, 1)[None].to(DEV)
    onehot = head(x, instances=instances)
    assert tuple(onehot.shape) == (1, NC, 1024, 1024) and torch.equal(onehot.sum(1), torch.ones((1, 1024, 1024), device=DEV))
    assert np.array_equal(nearest(onehot.argmax(1)[0].cpu().numpy().astype(np.uint8)), mask)
    # `instances=` holds for one call: the cached head keeps no callable, and without one (and without cellpose) the next call says so
    assert head._instances is None
    try:
        import cellpose  # noqa: F401
    except Exception:
        with pytest.raises(RuntimeError, match="instances="):
            seg.inference_cell_model(str(path), str(sd_dir), str(w_dir), str(seg_dir), text_embeddings=ctx)
