"""torch.autograd.Function wrappers over the forward / backward HIP kernels: the tape is torch's, every contraction, normalisation,
activation and attention FLOP of both passes runs in libldiff_hip.so (include/ldiff.h, "Backward-pass primitives").

This is the arithmetic layer of the reference's fine-tuning step (/root/reference/ldiffusion.py:227-255: V5 loop, `engine.backward`,
`engine.step`): UNet2DConditionModel + the 768->768 text projection are trained on 64 x 64 images = 8 x 8 latents, where a step is bound
by the weights it reads and writes.  Conventions: activations and their gradients are NHWC float16 CUDA tensors, parameters are float32
masters in the torch / diffusers layouts ([Cout, Cin, k, k], [out, in]) and receive float32 gradients.
  * dgrad = the forward conv kernel on the weights rearranged to [Cin][k][k][Cout] with the taps flipped (a layout cast in torch),
  * wgrad = the forward GEMM kernel over K = M on dy^T (ldiff_op_transpose) and im2col(x)^T (ldiff_op_im2col_t): the "staged" route, the default;
    under `wgrad_route("direct")` / `("auto")` the narrow convs over many pixels take ldiff_op_conv_wgrad (an MFMA contraction over the pixel index straight
    from the NHWC tensors) and the bias gradients ldiff_op_colsum_slabs instead (csrc/kernels_wgrad.hip; the tissue-head trainer runs under "auto");
    under `wgrad_route("wide")` / `("auto-wide")` the wide convs that entry refuses take ldiff_op_conv_wgrad_wide as well (the same kernel, Cy in blocks of 64),
  * GroupNorm(+SiLU), LayerNorm, GEGLU, attention: dedicated backward kernels (csrc/kernels_bwd.hip).
There is no CPU or torch-op fallback for those; reshapes / layout casts / the residual `+` are torch tensor plumbing.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .optim import ADAMW_CHUNK, SUMSQ_CHAIN, adamw_step, bucket_pack, sgd_nesterov_step, sumsq, sumsq_plan  # noqa: F401  (the step tail: optim.py)

_sp = _lib.stream_ptr


def _r(x, m):
    return (x + m - 1) // m * m


def _check_act(x, what):
    if not (x.is_cuda and x.dtype == torch.float16 and x.is_contiguous()):
        raise ValueError(f"{what} must be a contiguous float16 CUDA tensor")


_PACK_CACHE: dict | None = None   # (weight data_ptr, dgrad) -> packed tensor, while a PackPlan is active (train.GraphedStep)


def _pack_dims(Cout, Cin, dgrad, cols=None):
    if dgrad:
        return _r(_r(Cin, 8), 16), (cols if cols is not None else _r(Cout, 8))
    return _r(Cout, 16), _r(Cin, 8)


def pack_weight(w: torch.Tensor, dgrad: bool = False, cols: int | None = None) -> torch.Tensor:
    """[Cout, Cin, k, k] (or [out, in]) float32 -> the kernel layout, float16, one launch (ldiff_op_pack_weight):
    forward  [roundup(Cout,16)][k*k*roundup(Cin,8)]        rows >= Cout zero;
    dgrad    [roundup(cols_x,16)][k*k*cols]  = the weights rearranged to [Cin][k][k][Cout] with the taps flipped (`cols` = channels of dy).
    While a PackPlan is active, the layouts it has already produced for this storage are returned instead."""
    lib = _lib.load()
    w = w.detach()
    if w.dim() == 2:
        w = w[:, :, None, None]
    if _PACK_CACHE is not None:
        hit = _PACK_CACHE.get((w.data_ptr(), bool(dgrad)))
        if hit is not None and (not dgrad or cols is None or hit.shape[1] == w.shape[2] * w.shape[3] * cols):
            return hit
    if not (w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()):
        w = w.float().contiguous()
    Cout, Cin, k, _ = w.shape
    rows, cp = _pack_dims(Cout, Cin, dgrad, cols)
    out = torch.empty((rows, k * k * cp), dtype=torch.float16, device=w.device)
    _lib.check(lib.ldiff_op_pack_weight(w.data_ptr(), out.data_ptr(), Cout, Cin, k, rows, cp, int(dgrad), _sp()))
    return out


class PackPlan:
    """Forward and dgrad layouts of MANY conv / linear weights ([Cout, Cin, k, k] or [out, in], contiguous float32 CUDA) in ONE launch
    (ldiff_op_pack_weight_multi) into persistent float16 buffers; `run()` refreshes them from the current master values, `cache()` is the
    (data_ptr, dgrad) -> packed tensor map `pack_weight` consults while the plan is active (`with plan:`)."""

    def __init__(self, weights):
        import numpy as np
        ws = [w for w in weights if w.dim() in (2, 4)]
        if not ws:
            raise ValueError("PackPlan: no weights")
        dev = ws[0].device
        metas, total = [], 0
        for w in ws:
            if not (w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()):
                raise ValueError("PackPlan: weights must be contiguous float32 CUDA tensors")
            Cout, Cin = w.shape[0], w.shape[1]
            k = w.shape[2] if w.dim() == 4 else 1
            if k not in (1, 3):
                raise ValueError("PackPlan: kernel size 1 or 3")
            for dgrad in (False, True):
                rows, cp = _pack_dims(Cout, Cin, dgrad)
                metas.append((w, dgrad, Cout, Cin, k * k, rows, cp, total))
                total += rows * k * k * cp
        self.flat = torch.empty(total, dtype=torch.float16, device=dev)
        self._cache, rec, prefix, tiles = {}, [], [0], 0
        for w, dgrad, Cout, Cin, kk, rows, cp, off in metas:
            view = self.flat[off:off + rows * kk * cp].view(rows, kk * cp)
            self._cache[(w.data_ptr(), dgrad)] = view
            if dgrad:
                tx, ty = -(-cp // 64), -(-rows // (64 if kk == 1 else 16))
            else:
                tx, ty = -(-cp // 256), (-(-rows // 8) if kk == 1 else rows)
            rec.append((w.data_ptr(), view.data_ptr(), Cout, Cin, kk, rows, cp, int(dgrad), tx, 0))
            tiles += tx * ty
            prefix.append(tiles)
        arr = np.zeros(len(rec), dtype=np.dtype([("w", "<u8"), ("dst", "<u8"), ("i", "<i4", (8,))]))
        for j, r in enumerate(rec):
            arr[j] = (r[0], r[1], r[2:])
        self.entries = torch.from_numpy(arr.view(np.uint8).reshape(-1).copy()).to(dev)
        self.prefix = torch.tensor(prefix, dtype=torch.int32).to(dev)
        self.n_entries, self.n_tiles = len(rec), tiles
        self._keep = ws

    def run(self):
        _lib.check(_lib.load().ldiff_op_pack_weight_multi(self.entries.data_ptr(), self.prefix.data_ptr(), self.n_entries, self.n_tiles, _sp()))

    def cache(self):
        return self._cache


class packed_weights:
    """`with packed_weights(plan_a, plan_b, ...):` -- pack_weight returns the plans' layouts for the storages they cover."""

    def __init__(self, *plans):
        self.map = {}
        for p in plans:
            self.map.update(p.cache())

    def __enter__(self):
        global _PACK_CACHE
        self.prev, _PACK_CACHE = _PACK_CACHE, self.map
        return self

    def __exit__(self, *exc):
        global _PACK_CACHE
        _PACK_CACHE = self.prev
        return False


def _conv_call(x, w16, Cout, k, stride, ups, bias=None, Ho=None, Wo=None, out_f32=False, pad=None):
    """ldiff_op_conv on NHWC x [B,H,W,C] with packed weights; returns [B,Ho,Wo,roundup(Cout,8)] f16 (or f32 [.., roundup(Cout,4)])."""
    lib = _lib.load()
    B, H, W, Cin = x.shape
    pad = k // 2 if pad is None else pad
    He, We = H << ups, W << ups
    Ho = (He + 2 * pad - k) // stride + 1 if Ho is None else Ho
    Wo = (We + 2 * pad - k) // stride + 1 if Wo is None else Wo
    a = _lib.ConvArgs()
    a.x, a.C1, a.B, a.Hin, a.Win, a.Hout, a.Wout = x.data_ptr(), Cin, B, H, W, Ho, Wo
    a.ks, a.stride, a.pad_t, a.pad_l, a.ups = k, stride, pad, pad, ups
    a.w, a.N, a.Nrows = w16.data_ptr(), _r(Cout, 4), w16.shape[0]
    keep = []
    if bias is not None:
        b = bias.detach()
        if not (b.dtype == torch.float32 and b.is_contiguous() and b.numel() == w16.shape[0]):   # the kernel reads Nrows floats
            bp = torch.zeros(w16.shape[0], dtype=torch.float32, device=x.device)
            bp[:Cout] = b.float()
            b = bp
        a.bias = b.data_ptr()
        keep.append(b)
    ld = _r(Cout, 4) if out_f32 else _r(Cout, 8)
    alloc = torch.empty if ld == _r(Cout, 4) else torch.zeros   # the kernel writes roundup(Cout, 4) columns; pad columns beyond must be zero
    y = alloc((B, Ho, Wo, ld), dtype=torch.float32 if out_f32 else torch.float16, device=x.device)
    a.y, a.ldy, a.out_f32 = y.data_ptr(), ld, int(out_f32)
    _lib.check(lib.ldiff_op_conv(C.byref(a), _sp()))
    return y


# ---- which kernels form a conv's weight and bias gradient ----
# "staged": transpose + im2col_t + GEMM over K = M, and ldiff_op_colsum: what the fine-tuning step was built on (M a few hundred rows, N hundreds of columns).
# "direct": ldiff_op_conv_wgrad wherever the shape is eligible (else staged) and ldiff_op_colsum_slabs for every bias gradient.
# "auto":   "direct" for the launches with M = B Ho Wo >= WGRAD_DIRECT_MIN_ROWS, "staged" below.
# "wide":   every weight gradient on a direct kernel wherever one takes the shape: ldiff_op_conv_wgrad where it is eligible (the bits of "direct"), else
#           ldiff_op_conv_wgrad_wide (both channel counts blocked: the same kernel of csrc/kernels_wgrad.hip), else staged; ldiff_op_colsum_slabs for every bias gradient it takes.
# "auto-wide": the launches ldiff_op_conv_wgrad takes follow "auto" (and keep its bits); those only the wide entry takes go to it at
#           M >= WGRAD_WIDE_MIN_ROWS; every bias gradient ldiff_op_colsum_slabs takes goes through it, whatever M.
# The route is read when the FORWARD runs and kept with the node, so a backward() called outside the `with` follows the forward's route.
WGRAD_ROUTES = ("staged", "direct", "auto", "wide", "auto-wide")
# Crossover of the two routes at 32 -> 32 channels, 3 x 3, B = 1 (scripts/bench_wgrad_routes.py on an MI355X, weight + bias gradient, device time per backward,
# median of 20, the routes alternating; DESIGN.md section 7 "Direct weight and bias gradients"):
#     M        1024    4096    9216    16384    36864    65536    262144
#     staged    178     231     346     1044     2480     4389     17397  us
#     direct    161     163      70       71      104      109       176  us
# The direct route is the faster one from the smallest M measured on: the crossover lies BELOW 16384, and the constant never goes below 16384 -- the trainer's
# tests reach M = 2 * 64^2 = 8192 and keep the staged route bit for bit -- so the floor is the value.
WGRAD_DIRECT_MIN_ROWS = 16384
# Crossover into the wide entry per layer class of the tissue-head trainer (scripts/bench_wgrad_routes.py --wide on an MI355X, B = 12, weight + bias gradient, device
# time per backward in us, median of 10, staged / direct / wide alternating; "direct" is the staged weight gradient with the slab column sum, what "auto" gives
# these layers from WGRAD_DIRECT_MIN_ROWS on; DESIGN.md section 7 "Wide weight gradients" has min and max):
#     layer              at the trainer's M: staged / direct / wide      M = 12288                M = 3072             M = 768
#     3x3  64->128 s2    196608:  22647 / 2817 / 282                    1012 / 221 / 161         264 / 186 / 163      187 / 190 / 166
#     3x3 128->128       196608:  24446 / 4654 / 287                    1017 / 250 / 162         289 / 180 / 160      190 / 195 / 169
#     3x3 128->256 s2     49152:   3835 /  720 / 208                    1021 / 254 / 163         313 / 186 / 162      184 / 194 / 170
#     3x3 256->256        49152:   5759 / 1142 / 266                    1074 / 311 / 164         337 / 181 / 165      179 / 185 / 165
#     3x3 256->128       196608:  24158 / 4391 / 387                    1096 / 306 / 162         334 / 186 / 166      186 / 194 / 169
#     3x3 512->256        49152:   6444 / 1671 / 375                    1180 / 418 / 175         371 / 192 / 165      179 / 185 / 163
#     1x1 128->256       196608:  18526 / 2321 / 301                     965 / 205 / 165         194 / 175 / 161      169 / 176 / 162
#     1x1 256->512        49152:   3493 /  545 / 219                     939 / 217 / 164         256 / 174 / 160      169 / 175 / 160
#     1x1 256->8          49152:   2279 /  525 / 164                     433 / 222 / 164         180 / 173 / 162      169 / 173 / 159
# At its trainer's M every class is 2.5 -- 16 x faster on the wide entry than on "direct", far beyond the largest spread (max - min) of the three.  At M = 12288 eight of nine still
# win by more than the spread (1x1 128->256: 40 us ahead under a spread of 61 us: staged by the rule); at 3072 and 768 the launches bound all three routes (160 us) and
# the gap is within the spread for most.  So the crossover lies BELOW 16384 for every class, and, as with WGRAD_DIRECT_MIN_ROWS, the constant never goes below 16384.
WGRAD_WIDE_MIN_ROWS = 16384
_WGRAD_ROUTE = "staged"
_WGRAD_ROUTE_STATED = False   # a caller has set the route (nnunet_train.TrainableSegNet runs under "auto" unless one has)


def _check_route(mode):
    if mode not in WGRAD_ROUTES:
        raise ValueError(f"wgrad route {mode!r}: one of {WGRAD_ROUTES}")


def set_wgrad_route(mode: str) -> str:
    """Set the module-wide route of weight / bias gradients (one of WGRAD_ROUTES); returns the previous one."""
    global _WGRAD_ROUTE, _WGRAD_ROUTE_STATED
    _check_route(mode)
    prev, _WGRAD_ROUTE, _WGRAD_ROUTE_STATED = _WGRAD_ROUTE, mode, True
    return prev


def stated_wgrad_route(default: str) -> str:
    """The route a caller has set (set_wgrad_route, or an enclosing wgrad_route), else `default`."""
    return _WGRAD_ROUTE if _WGRAD_ROUTE_STATED else default


class wgrad_route:
    """`with wgrad_route("direct"):` -- the Conv2dFn nodes whose forward runs inside take that route in their backward."""

    def __init__(self, mode: str):
        _check_route(mode)
        self.mode = mode

    def __enter__(self):
        global _WGRAD_ROUTE, _WGRAD_ROUTE_STATED
        self.prev = (_WGRAD_ROUTE, _WGRAD_ROUTE_STATED)
        _WGRAD_ROUTE, _WGRAD_ROUTE_STATED = self.mode, True
        return self

    def __exit__(self, *exc):
        global _WGRAD_ROUTE, _WGRAD_ROUTE_STATED
        _WGRAD_ROUTE, _WGRAD_ROUTE_STATED = self.prev
        return False


_NARROW_LIMITS = (128, 64, 128)     # Cx, Cy at k = 3, Cy at k = 1: what ldiff_op_conv_wgrad takes (include/ldiff.h)
_WIDE_LIMITS = (1024, 512, 2048)    # the same of ldiff_op_conv_wgrad_wide


def _wgrad_eligible(limits, k, stride, ups, Cx, Cy, Cout, Cin) -> bool:
    cx_max, cy_max3, cy_max1 = limits
    return (ups == 0 and ((k == 3 and stride in (1, 2)) or (k == 1 and stride == 1)) and Cx % 8 == 0 and 8 <= Cx <= cx_max and Cy % 8 == 0
            and 8 <= Cy <= (cy_max3 if k == 3 else cy_max1) and 1 <= Cout <= Cy and 1 <= Cin <= Cx)


def wgrad_direct_eligible(k, stride, ups, Cx, Cy, Cout, Cin) -> bool:
    """The shapes ldiff_op_conv_wgrad takes (include/ldiff.h)."""
    return _wgrad_eligible(_NARROW_LIMITS, k, stride, ups, Cx, Cy, Cout, Cin)


def wgrad_wide_eligible(k, stride, ups, Cx, Cy, Cout, Cin) -> bool:
    """The shapes ldiff_op_conv_wgrad_wide takes (include/ldiff.h)."""
    return _wgrad_eligible(_WIDE_LIMITS, k, stride, ups, Cx, Cy, Cout, Cin)


def _wgrad_plan(nb, yslabs, B, Ho, Wo, Cx, k, wgs) -> dict:
    """The plan of csrc/kernels_wgrad.hip wgrad_plan for workgroups of `nb` output channels over `yslabs` slabs of Cy: tiles of TH x 32 output pixels (k = 1:
    TH * 32 consecutive pixels), `wgs` tile-walking workgroups per nb x 32 block of (Cy, Cx), `slabs` = the blocks, `chain` = the most terms one accumulator adds
    (an MFMA's inner sum counted as 32) and `partials` = the partial sums the finalize adds per element."""
    TH = 8 if k == 1 else 4
    xslabs = -(-Cx // 32)
    tiles = -(-(B * Ho * Wo) // (TH * 32)) if k == 1 else B * (-(-Ho // TH)) * (-(-Wo // 32))
    n = wgs if wgs > 0 else min(tiles, max(1, 1024 // (xslabs * yslabs)))
    return dict(TH=TH, tiles=tiles, wgs=n, slabs=xslabs * yslabs, chain=-(-tiles // n) * TH * 32, partials=n, ws_bytes=n * nb * yslabs * k * k * xslabs * 32 * 4)


def wgrad_plan(B, Ho, Wo, Cx, Cy, k, wgs=0) -> dict:
    """The plan ldiff_op_conv_wgrad makes for a launch, for the error bounds of the tests: the whole of Cy (padded to 32 / 64 / 128) in one workgroup."""
    return _wgrad_plan(32 if Cy <= 32 else 64 if Cy <= 64 else 128, 1, B, Ho, Wo, Cx, k, wgs)


def wgrad_wide_plan(B, Ho, Wo, Cx, Cy, k, wgs=0) -> dict:
    """The plan ldiff_op_conv_wgrad_wide makes for a launch, with the keys of wgrad_plan: Cy in slabs of 64."""
    return _wgrad_plan(64, -(-Cy // 64), B, Ho, Wo, Cx, k, wgs)


def wgrad_entry(route, M, k, stride, ups, Cx, Cy, Cout, Cin):
    """(entry, slab_bias) of a conv's backward under `route` at M = B Ho Wo rows, by the comment at the head of this section: entry = "narrow"
    (ldiff_op_conv_wgrad), "wide" (ldiff_op_conv_wgrad_wide) or "staged"; slab_bias = the route asks for ldiff_op_colsum_slabs (its own limits on Cy are the launch's)."""
    direct = route in ("direct", "wide") or (route in ("auto", "auto-wide") and M >= WGRAD_DIRECT_MIN_ROWS)
    wide = route == "wide" or (route == "auto-wide" and M >= WGRAD_WIDE_MIN_ROWS)
    narrow_ok = wgrad_direct_eligible(k, stride, ups, Cx, Cy, Cout, Cin)
    if direct and narrow_ok:
        entry = "narrow"
    elif wide and not narrow_ok and wgrad_wide_eligible(k, stride, ups, Cx, Cy, Cout, Cin):
        entry = "wide"
    else:
        entry = "staged"
    return entry, direct or route == "auto-wide"


def colsum_slabs_plan(M, N) -> dict:
    """The plan of ldiff_op_colsum_slabs (csrc/kernels_wgrad.hip colsum_plan): `chain` = rows one thread adds plus the row lanes one LDS pass adds."""
    rp = 256 // (N // 8)
    slabs = min(max(-(-M // 256), 1), 1024)
    rows = -(-M // slabs)
    slabs = -(-M // rows)
    return dict(slabs=slabs, rows=rows, row_lanes=rp, chain=-(-rows // rp) + rp, partials=slabs, ws_bytes=slabs * N * 4)


def _conv_wgrad(entry, x, dy, Cout, Cin, k, stride, wgs):
    _check_act(x, "x")
    _check_act(dy, "dy")
    lib = _lib.load()
    B, H, W, Cx = x.shape
    _, Ho, Wo, Cy = dy.shape
    dw = torch.empty((Cout, Cin, k, k), dtype=torch.float32, device=x.device)
    nb = getattr(lib, entry + "_ws_bytes")(B, Ho, Wo, Cx, Cy, k, int(wgs))
    ws = _workspace(nb, x.device)
    _lib.check(getattr(lib, entry)(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), B, H, W, Cx, Ho, Wo, Cy, Cout, Cin, k, stride, int(wgs), ws.data_ptr(), nb, _sp()))
    return dw


def conv_wgrad_direct(x, dy, Cout, Cin, k, stride, wgs=0):
    """ldiff_op_conv_wgrad: x [B,H,W,Cx], dy [B,Ho,Wo,Cy] NHWC float16 -> dw float32 [Cout, Cin, k, k]."""
    return _conv_wgrad("ldiff_op_conv_wgrad", x, dy, Cout, Cin, k, stride, wgs)


def conv_wgrad_wide(x, dy, Cout, Cin, k, stride, wgs=0):
    """ldiff_op_conv_wgrad_wide: x [B,H,W,Cx], dy [B,Ho,Wo,Cy] NHWC float16 -> dw float32 [Cout, Cin, k, k]."""
    return _conv_wgrad("ldiff_op_conv_wgrad_wide", x, dy, Cout, Cin, k, stride, wgs)


def colsum_slabs(dy, N=None):
    """ldiff_op_colsum_slabs over the rows of float16 dy [..., ld]: float32 [N] (N = ld unless given)."""
    _check_act(dy, "dy")
    lib = _lib.load()
    ld = dy.shape[-1]
    N = ld if N is None else N
    M = dy.numel() // ld
    db = torch.empty(N, dtype=torch.float32, device=dy.device)
    nb = lib.ldiff_op_colsum_slabs_ws_bytes(M, N)
    ws = _workspace(nb, dy.device)
    _lib.check(lib.ldiff_op_colsum_slabs(dy.data_ptr(), db.data_ptr(), M, N, ld, ws.data_ptr(), nb, _sp()))
    return db


class Conv2dFn(torch.autograd.Function):
    """y = conv2d(nearest_up(x, 2**ups), weight, bias, stride, padding=k//2) on NHWC float16 activations (k in {1, 3}).
    Channel counts of x must be multiples of 8 (pad the 4-channel latents); y has roundup(Cout, 8) channels, the pad columns zero."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride=1, ups=0):
        _check_act(x, "x")
        Cout, Cin, k = weight.shape[0], weight.shape[1], (weight.shape[2] if weight.dim() == 4 else 1)
        if x.shape[-1] != _r(Cin, 8):
            raise ValueError(f"x has {x.shape[-1]} channels, the weight expects {Cin} (padded to {_r(Cin, 8)})")
        y = _conv_call(x, pack_weight(weight), Cout, k, stride, ups, bias)
        ctx.save_for_backward(x, weight)
        ctx.meta = (stride, ups, bias is not None, k, Cout, Cin)
        ctx.wgrad_route = _WGRAD_ROUTE
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, weight = ctx.saved_tensors
        stride, ups, has_bias, k, Cout, Cin = ctx.meta
        dy = dy.contiguous()
        B, H, W, Cx = x.shape
        _, Ho, Wo, Cy = dy.shape
        w4 = weight if weight.dim() == 4 else weight[:, :, None, None]
        dx = dw = db = None
        entry, slab_bias = wgrad_entry(ctx.wgrad_route, B * Ho * Wo, k, stride, ups, Cx, Cy, Cout, Cin)
        if ctx.needs_input_grad[0]:
            # dgrad: conv (stride 1) of dy -- zero-inserted for a stride-2 forward -- with the weights [Cin][k][k][Cout], taps flipped
            wd = pack_weight(w4, dgrad=True, cols=Cy)
            g = dy
            He, We = H << ups, W << ups
            if stride == 2:
                g = torch.zeros((B, He, We, Cy), dtype=torch.float16, device=x.device)
                g[:, ::2, ::2] = dy
            dxu = _conv_call(g, wd, Cx, k, 1, 0)
            dx = dxu if ups == 0 else dxu.view(B, H, 2, W, 2, Cx).float().sum((2, 4)).to(torch.float16)
        if ctx.needs_input_grad[1] and entry != "staged":
            dw = (conv_wgrad_direct if entry == "narrow" else conv_wgrad_wide)(x, dy, Cout, Cin, k, stride).view(weight.shape)
        elif ctx.needs_input_grad[1]:
            # wgrad: dW[n][tap*Cx + c] = sum_m dy[m, n] * xcol[m, tap*Cx + c]  as a GEMM over K = M
            M = B * Ho * Wo
            Mpad = _r(M, 8)
            Kc = k * k * Cx
            dyT = torch.empty((Cy, Mpad), dtype=torch.float16, device=x.device)
            _lib.check(lib.ldiff_op_transpose(dy.data_ptr(), dyT.data_ptr(), M, Cy, Cy, Mpad, _sp()))
            xcolT = torch.empty((_r(Kc, 16), Mpad), dtype=torch.float16, device=x.device)   # im2col_t writes rows < Kc (columns >= M zero)
            if xcolT.shape[0] > Kc:
                xcolT[Kc:].zero_()
            _lib.check(lib.ldiff_op_im2col_t(x.data_ptr(), xcolT.data_ptr(), B, H, W, Cx, k, stride, k // 2, ups, Ho, Wo, Mpad, _sp()))
            g = _conv_call(dyT.view(1, 1, Cy, Mpad), xcolT, Kc, 1, 1, 0, out_f32=True)        # [1,1,Cy,Kc] f32
            if k == 1 and Cx == Cin and Cy == Cout and g.shape[-1] == Cin:
                dw = g.view(weight.shape)   # 1 x 1 / linear with unpadded channel counts: the GEMM's [Cout][Cin] output IS the weight gradient (no unpack launch)
            else:
                dw = torch.empty(weight.shape, dtype=torch.float32, device=x.device)
                _lib.check(lib.ldiff_op_unpack_wgrad(g.data_ptr(), dw.data_ptr(), Cout, Cin, k, Cx, g.shape[-1], _sp()))
        if has_bias and ctx.needs_input_grad[2]:
            if slab_bias and Cy % 8 == 0 and Cy <= 2048:
                db = colsum_slabs(dy)
            else:
                db = torch.empty(Cy, dtype=torch.float32, device=x.device)
                _lib.check(lib.ldiff_op_colsum(dy.data_ptr(), db.data_ptr(), B * Ho * Wo, Cy, Cy, _sp()))
            db = db[:Cout]
        return dx, dw, db, None, None


def linear(x, weight, bias=None):
    """F.linear on float16 rows [..., Cin] through the conv kernels (k = 1)."""
    shp = x.shape
    y = Conv2dFn.apply(x.reshape(1, 1, -1, shp[-1]).contiguous(), weight, bias, 1, 0)
    y = y.reshape(*shp[:-1], y.shape[-1])
    return y if y.shape[-1] == weight.shape[0] else y[..., :weight.shape[0]]


class GroupNormFn(torch.autograd.Function):
    """y = act(group_norm(x, groups, gamma, beta, eps)) on NHWC float16 [B, H, W, C]; act = SiLU when `silu`."""

    @staticmethod
    def forward(ctx, x, gamma, beta, groups, eps, silu):
        _check_act(x, "x")
        lib = _lib.load()
        B, H, W, Cc = x.shape
        y = torch.empty_like(x)
        mean = torch.empty((B, groups), dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        g32, b32 = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        _lib.check(lib.ldiff_op_gn_train_fwd(x.data_ptr(), y.data_ptr(), g32.data_ptr(), b32.data_ptr(), mean.data_ptr(), rstd.data_ptr(), B, H * W, Cc,
                                             groups, float(eps), int(silu), _sp()))
        ctx.save_for_backward(x, g32, b32, mean, rstd)
        ctx.meta = (groups, int(silu))
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, g32, b32, mean, rstd = ctx.saved_tensors
        groups, silu = ctx.meta
        B, H, W, Cc = x.shape
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        dg, db = torch.zeros(Cc, dtype=torch.float32, device=x.device), torch.zeros(Cc, dtype=torch.float32, device=x.device)
        _lib.check(lib.ldiff_op_gn_train_bwd(x.data_ptr(), dy.data_ptr(), g32.data_ptr(), b32.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
                                             dg.data_ptr(), db.data_ptr(), B, H * W, Cc, groups, silu, _sp()))
        return dx, dg, db, None, None, None


class LayerNormFn(torch.autograd.Function):
    """F.layer_norm over the last dim of float16 rows [..., C]."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        _check_act(x, "x")
        lib = _lib.load()
        Cc = x.shape[-1]
        rows = x.numel() // Cc
        y = torch.empty_like(x)
        g32, b32 = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        _lib.check(lib.ldiff_op_layernorm(x.data_ptr(), 0, 0, y.data_ptr(), rows, Cc, g32.data_ptr(), b32.data_ptr(), float(eps), _sp()))
        ctx.save_for_backward(x, g32)
        ctx.eps = float(eps)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, g32 = ctx.saved_tensors
        Cc = x.shape[-1]
        rows = x.numel() // Cc
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        dg, db = torch.zeros(Cc, dtype=torch.float32, device=x.device), torch.zeros(Cc, dtype=torch.float32, device=x.device)
        _lib.check(lib.ldiff_op_ln_bwd(x.data_ptr(), dy.data_ptr(), g32.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), rows, Cc, ctx.eps, _sp()))
        return dx, dg, db, None


class GegluFn(torch.autograd.Function):
    """[M, 2*C4] = [h | gate] -> h * gelu_erf(gate)   (diffusers GEGLU)."""

    @staticmethod
    def forward(ctx, x):
        _check_act(x, "x")
        lib = _lib.load()
        C4 = x.shape[-1] // 2
        M = x.numel() // x.shape[-1]
        y = torch.empty(x.shape[:-1] + (C4,), dtype=torch.float16, device=x.device)
        _lib.check(lib.ldiff_op_geglu(x.data_ptr(), y.data_ptr(), M, C4, _sp()))
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        (x,) = ctx.saved_tensors
        C4 = x.shape[-1] // 2
        M = x.numel() // x.shape[-1]
        dx = torch.empty_like(x)
        _lib.check(lib.ldiff_op_geglu_bwd(x.data_ptr(), dy.contiguous().data_ptr(), dx.data_ptr(), M, C4, _sp()))
        return dx


class SiluFn(torch.autograd.Function):
    """y = x * sigmoid(x) on float16 tensors of any shape (ldiff_op_silu / ldiff_op_silu_bwd): the two activations of the time-embedding MLP,
    the last elementwise ops of the step that used to run through ATen."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        _check_act(x, "silu input")
        y = torch.empty_like(x)
        _lib.check(_lib.load().ldiff_op_silu(x.data_ptr(), y.data_ptr(), x.numel(), _sp()))
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        _lib.check(_lib.load().ldiff_op_silu_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), _sp()))
        return dx


def silu(x):
    return SiluFn.apply(x)


class AttentionFn(torch.autograd.Function):
    """softmax(q k^T / sqrt(d)) v per head on float16 [B, L, heads*d] tensors (K/V given per batch entry, not broadcast)."""

    @staticmethod
    def forward(ctx, q, k, v, heads):
        for t, n in ((q, "q"), (k, "k"), (v, "v")):
            _check_act(t, n)
        lib = _lib.load()
        B, Lq, Cc = q.shape
        Lk = k.shape[1]
        d = Cc // heads
        o = torch.empty_like(q)
        scale = 1.0 / d ** 0.5
        _lib.check(lib.ldiff_op_attention(q.data_ptr(), Cc, k.data_ptr(), Cc, v.data_ptr(), Cc, o.data_ptr(), Cc, B, heads, Lq, Lk, d, Lq * Cc, Lk * Cc, Lq * Cc,
                                          scale, _sp()))
        ctx.save_for_backward(q, k, v)
        ctx.meta = (heads, scale)
        return o

    @staticmethod
    def backward(ctx, do):
        lib = _lib.load()
        q, k, v = ctx.saved_tensors
        heads, scale = ctx.meta
        B, Lq, Cc = q.shape
        Lk = k.shape[1]
        do = do.contiguous()
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        _lib.check(lib.ldiff_op_attention_bwd(q.data_ptr(), Cc, k.data_ptr(), Cc, v.data_ptr(), Cc, do.data_ptr(), Cc, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
                                              B, heads, Lq, Lk, Cc // heads, Lq * Cc, Lk * Cc, Lq * Cc, scale, _sp()))
        return dq, dk, dv, None


class InfoNceFn(torch.autograd.Function):
    """Contrastive feature loss for given sample triples (/root/reference/model/loss.py:89-109): forward value and d loss / d features from
    ONE launch of ldiff_op_infonce; backward only scales the stored gradient.  features f32 [B, n, H, W]; bi/ai/pi int32 [T], ni int32 [T, K]."""

    @staticmethod
    def forward(ctx, features, bi, ai, pi, ni, temperature, count=None):
        """count: optional device int32 scalar = the number of valid triples (the index tensors are then capacity-sized: shape-stable launch)."""
        if not (features.is_cuda and features.dtype == torch.float32):
            raise ValueError("InfoNceFn: features must be a float32 CUDA tensor")
        f = features.contiguous()
        B, n, H, W = f.shape
        T, K = ni.shape
        if count is None and T > 0:
            # eager use: the indices address global reads and atomic scatters; the torch gather this replaces raised on a bad index
            # (triples sampled at another resolution than the feature map).  The capacity-sized graph path validates on the host
            # before the upload (train.GraphedStep.set_batch): no device read-back inside a replayed step.
            # ONE device reduction and ONE read-back for the four bounds (was eight host syncs per step)
            px = torch.cat([ai.reshape(-1), pi.reshape(-1), ni.reshape(-1)]).long()
            lo, hi, blo, bhi = torch.stack([px.min(), px.max(), bi.min().long(), bi.max().long()]).tolist()
            if lo < 0 or hi >= H * W or blo < 0 or bhi >= B:
                raise IndexError(f"InfoNceFn: sample indices out of range for features [B={B}, {H}x{W}] (pixel {lo}..{hi}, image {blo}..{bhi})")
        loss = torch.empty(1, dtype=torch.float32, device=f.device)
        df = torch.empty_like(f)
        _lib.check(_lib.load().ldiff_op_infonce(f.data_ptr(), B, n, H * W, bi.data_ptr(), ai.data_ptr(), pi.data_ptr(), ni.data_ptr(), T,
                                                None if count is None else count.data_ptr(), K, float(temperature), loss.data_ptr(), df.data_ptr(), _sp()))
        ctx.save_for_backward(df)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (df,) = ctx.saved_tensors
        return g * df, None, None, None, None, None, None


# ---- training form of the nnU-Net tissue head (csrc/kernels_segtrain.hip; ldiffusion_amd/nnunet_train.py) ----
def _workspace(nbytes, device):
    return torch.empty(max(int(nbytes), 16) // 8 + 1, dtype=torch.float64, device=device)   # 8-byte elements: the loss kernels keep double sums in it


class InstanceNormLReLUFn(torch.autograd.Function):
    """y = leaky_relu(instance_norm(x, gamma, beta, eps), slope) on NHWC float16 [B, H, W, C], C % 8 == 0 (ldiff_op_in_train_fwd / _bwd): the norm +
    nonlinearity of every conv block of nnU-Net's PlainConvUNet.  mean / rstd [B, C] float32 are kept; the backward recomputes the mask from x."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps=1e-5, slope=0.01):
        _check_act(x, "x")
        lib = _lib.load()
        B, H, W, Cc = x.shape
        y = torch.empty_like(x)
        mean = torch.empty((B, Cc), dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        g32, b32 = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        nb = lib.ldiff_op_in_train_ws_bytes(B, H * W, Cc)
        ws = _workspace(nb, x.device)
        _lib.check(lib.ldiff_op_in_train_fwd(x.data_ptr(), y.data_ptr(), g32.data_ptr(), b32.data_ptr(), mean.data_ptr(), rstd.data_ptr(), B, H * W, Cc,
                                             float(eps), float(slope), ws.data_ptr(), nb, _sp()))
        ctx.save_for_backward(x, g32, b32, mean, rstd)
        ctx.slope = float(slope)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, g32, b32, mean, rstd = ctx.saved_tensors
        B, H, W, Cc = x.shape
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        dg, db = torch.empty(Cc, dtype=torch.float32, device=x.device), torch.empty(Cc, dtype=torch.float32, device=x.device)
        nb = lib.ldiff_op_in_train_ws_bytes(B, H * W, Cc)
        ws = _workspace(nb, x.device)
        _lib.check(lib.ldiff_op_in_train_bwd(x.data_ptr(), dy.data_ptr(), g32.data_ptr(), b32.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
                                             dg.data_ptr(), db.data_ptr(), B, H * W, Cc, ctx.slope, ws.data_ptr(), nb, _sp()))
        return dx, dg, db, None, None


def _dice_ce_args(logits, target, what):
    _check_act(logits, "logits")
    if target.dim() == 4 and target.shape[1] == 1:
        target = target[:, 0]
    B, H, W, ld = logits.shape
    if tuple(target.shape) != (B, H, W):
        raise ValueError(f"{what}: target {tuple(target.shape)} does not match logits {tuple(logits.shape)}")
    if target.dtype not in (torch.uint8, torch.int64):   # the nnU-Net loader hands float label maps (RobustCrossEntropyLoss casts them with .long())
        target = target.long() if target.is_floating_point() else target.to(torch.int64)
    return target.to(logits.device).contiguous(), B, H, W, ld


def _dice_ce_ws(lib, B, HW, n_heads, device, ignore_label=None):
    """(workspace, its byte count) of the three Dice + CE entries, or of their ignore form"""
    nb = (lib.ldiff_op_dice_ce_ws_bytes if ignore_label is None else lib.ldiff_op_dice_ce_ignore_ws_bytes)(B, HW, int(n_heads))
    return _workspace(nb, device), nb


def _ignore_label(ignore_label, n_heads, what):
    """None, or the label as the C entries take it: an integer that is no class (nnU-Net's own rule, nnunet.label_spec, makes it n_heads)."""
    if ignore_label is None:
        return None
    if isinstance(ignore_label, bool) or int(ignore_label) != ignore_label or not int(n_heads) <= int(ignore_label) <= 254:
        raise ValueError(f"{what}: ignore_label {ignore_label!r} must be an integer in [n_heads = {int(n_heads)}, 254]")
    return int(ignore_label)


def dice_ce(logits, target, n_heads, batch_dice, weight=1.0, grad_scale=1.0, smooth=1e-5, ignore_label=None):
    """ldiff_op_dice_ce on float16 logits [B, H, W, roundup(n_heads, 8)] and uint8 / int64 labels [B, H, W] (or [B, 1, H, W]):
    (loss float32 0-dim, dlogits float16 = grad_scale * weight * d loss / d logits in the logits' layout).  `ignore_label`: nnU-Net's ignore label
    (ldiff_op_dice_ce_ignore): pixels carrying it add nothing to the loss and get a zero gradient; None is the plain entry.  Region labels go through
    `dice_focal` (nnunet.network_spec(accept_regions=True))."""
    target, B, H, W, ld = _dice_ce_args(logits, target, "dice_ce")
    ignore_label = _ignore_label(ignore_label, n_heads, "dice_ce")
    lib = _lib.load()
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits)
    ws, nb = _dice_ce_ws(lib, B, H * W, n_heads, logits.device, ignore_label)
    if ignore_label is not None:
        _lib.check(lib.ldiff_op_dice_ce_ignore(logits.data_ptr(), ld, int(n_heads), ignore_label, target.data_ptr(), int(target.dtype == torch.int64), B, H * W,
                                               int(bool(batch_dice)), float(smooth), float(weight), float(grad_scale), loss.data_ptr(), dlogits.data_ptr(),
                                               ws.data_ptr(), nb, _sp()))
        return loss[0], dlogits
    _lib.check(lib.ldiff_op_dice_ce(logits.data_ptr(), ld, int(n_heads), target.data_ptr(), int(target.dtype == torch.int64), B, H * W, int(bool(batch_dice)),
                                    float(smooth), float(weight), float(grad_scale), loss.data_ptr(), dlogits.data_ptr(), ws.data_ptr(), nb, _sp()))
    return loss[0], dlogits


class DiceCeFn(torch.autograd.Function):
    """nnU-Net's DC_and_CE_loss of one deep-supervision scale as a term of the step's loss.  forward returns `weight` * loss of the scale in float32
    (`weight` = the scale's deep-supervision weight; the value is NOT multiplied by the loss scale).  The gradient was formed by the same call in float32
    and stored as float16 = `grad_scale` * d(weight * loss) / d logits, because most of it lies below float16's range unscaled; backward hands out that
    tensor times the incoming gradient (1 when the caller backpropagates the sum of the terms: the product is then the stored tensor bit for bit), so
    `grad_scale` acts as the loss scale of this term and the caller unscales the parameter gradients by 1 / grad_scale (nnunet_train.Trainer.train_step)."""

    @staticmethod
    def forward(ctx, logits, target, n_heads, batch_dice, weight, grad_scale, smooth=1e-5, ignore_label=None):
        loss, dlogits = dice_ce(logits, target, n_heads, batch_dice, weight, grad_scale, smooth, ignore_label)
        ctx.save_for_backward(dlogits)
        return loss * float(weight)

    @staticmethod
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        return (dlogits.float() * g).to(dlogits.dtype), None, None, None, None, None, None, None


def dice_ce_nacc(n_heads, ignore_label=None):
    """Doubles per row of the loss statistics: sum_pred, intersect, sum_gt per padded class, the cross-entropy sum, the count of labels outside [0, n_heads)
    (ignored pixels excepted) and, in the ignore form (ldiff_op_dice_ce_ignore_nacc), the count of annotated pixels.
    The one definition is csrc/kernels_segtrain.hip's NACC = 3 NC + 2 + IGN (NC = 8 NV columns of a padded row); this mirrors it, to spare the step a
    library call per scale."""
    return 3 * 8 * ((int(n_heads) + 7) // 8) + (2 if ignore_label is None else 3)


def dice_ce_stats(logits, target, n_heads, batch_dice, out=None, ignore_label=None):
    """ldiff_op_dice_ce_stats: the sums `dice_ce` forms before its coefficients, float64 [1 or B, dice_ce_nacc(n_heads)] on the device (one row with
    `batch_dice`), added in dice_ce's order.  `out`: a contiguous float64 device tensor of that many elements to write into (a row of a caller's table).
    `ignore_label`: the ignore form (ldiff_op_dice_ce_ignore_stats), rows of dice_ce_nacc(n_heads, ignore_label)."""
    lib = _lib.load()
    target, B, H, W, ld = _dice_ce_args(logits, target, "dice_ce_stats")
    ignore_label = _ignore_label(ignore_label, n_heads, "dice_ce_stats")
    rows, nacc = (1 if batch_dice else B), dice_ce_nacc(n_heads, ignore_label)
    if out is None:
        out = torch.empty((rows, nacc), dtype=torch.float64, device=logits.device)
    elif not (out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() == rows * nacc):
        raise ValueError(f"dice_ce_stats: out must be a contiguous float64 CUDA tensor of {rows * nacc} elements")
    ws, nb = _dice_ce_ws(lib, B, H * W, n_heads, logits.device, ignore_label)
    if ignore_label is not None:
        _lib.check(lib.ldiff_op_dice_ce_ignore_stats(logits.data_ptr(), ld, int(n_heads), ignore_label, target.data_ptr(), int(target.dtype == torch.int64), B, H * W,
                                                     int(bool(batch_dice)), out.data_ptr(), ws.data_ptr(), nb, _sp()))
        return out
    _lib.check(lib.ldiff_op_dice_ce_stats(logits.data_ptr(), ld, int(n_heads), target.data_ptr(), int(target.dtype == torch.int64), B, H * W,
                                          int(bool(batch_dice)), out.data_ptr(), ws.data_ptr(), nb, _sp()))
    return out


def dice_ce_from_sums(logits, target, n_heads, batch_dice, dice_sums, local_sums, world=1, weight=1.0, grad_scale=1.0, smooth=1e-5, ignore_label=None):
    """ldiff_op_dice_ce_from_sums: (loss, dlogits) as `dice_ce` returns them, the Dice term from `dice_sums` (with `batch_dice` possibly the sum of `world`
    processes' statistics; its gradient then carries the factor `world`), the cross-entropy from `local_sums` over this process's B H W pixels.
    `ignore_label`: the ignore form (ldiff_op_dice_ce_ignore_from_sums) on `dice_ce_stats(..., ignore_label=)`'s rows: the cross-entropy over this
    process's annotated pixels.  It is built for one process: world = 1 and `dice_sums` is `local_sums`, anything else raises NotImplementedError."""
    lib = _lib.load()
    target, B, H, W, ld = _dice_ce_args(logits, target, "dice_ce_from_sums")
    ignore_label = _ignore_label(ignore_label, n_heads, "dice_ce_from_sums")
    rows, nacc = (1 if batch_dice else B), dice_ce_nacc(n_heads, ignore_label)
    for name, t in (("dice_sums", dice_sums), ("local_sums", local_sums)):
        if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() == rows * nacc):
            raise ValueError(f"dice_ce_from_sums: {name} must be a contiguous float64 CUDA tensor of {rows * nacc} elements")
    if not batch_dice and (int(world) != 1 or dice_sums.data_ptr() != local_sums.data_ptr()):
        raise ValueError("dice_ce_from_sums: without batch_dice the Dice term is per sample and stays local (world = 1, dice_sums is local_sums)")
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits)
    ws, nb = _dice_ce_ws(lib, B, H * W, n_heads, logits.device, ignore_label)
    if ignore_label is not None:
        if int(world) != 1 or dice_sums.data_ptr() != local_sums.data_ptr():
            raise NotImplementedError(f"dice_ce_from_sums(ignore_label={ignore_label}) with the statistics of world = {int(world)} processes: the data-parallel "
                                      "exchange of the ignore form is not built")
        _lib.check(lib.ldiff_op_dice_ce_ignore_from_sums(logits.data_ptr(), ld, int(n_heads), ignore_label, target.data_ptr(), int(target.dtype == torch.int64), B,
                                                         H * W, int(bool(batch_dice)), float(smooth), float(weight), float(grad_scale), local_sums.data_ptr(),
                                                         loss.data_ptr(), dlogits.data_ptr(), ws.data_ptr(), nb, _sp()))
        return loss[0], dlogits
    _lib.check(lib.ldiff_op_dice_ce_from_sums(logits.data_ptr(), ld, int(n_heads), target.data_ptr(), int(target.dtype == torch.int64), B, H * W,
                                              int(bool(batch_dice)), float(smooth), float(weight), float(grad_scale), dice_sums.data_ptr(), local_sums.data_ptr(),
                                              int(world), loss.data_ptr(), dlogits.data_ptr(), ws.data_ptr(), nb, _sp()))
    return loss[0], dlogits


class DiceCeSumsFn(torch.autograd.Function):
    """DiceCeFn with the statistics supplied: the term of a data-parallel rank.  `dice_sums` / `local_sums` / `world` as dice_ce_from_sums takes them;
    value, stored gradient and backward as DiceCeFn's.  At world = 1 on `dice_ce_stats`' own sums it is DiceCeFn bit for bit."""

    @staticmethod
    def forward(ctx, logits, target, n_heads, batch_dice, dice_sums, local_sums, world, weight, grad_scale, smooth=1e-5, ignore_label=None):
        loss, dlogits = dice_ce_from_sums(logits, target, n_heads, batch_dice, dice_sums, local_sums, world, weight, grad_scale, smooth, ignore_label)
        ctx.save_for_backward(dlogits)
        return loss * float(weight)

    @staticmethod
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        return (dlogits.float() * g).to(dlogits.dtype), None, None, None, None, None, None, None, None, None, None


# ---- region labels: Dice + focal / BCE on the label map through the membership table (csrc/kernels_segregion.hip) ----
def _region_args(logits, target, table, n_regions, what):
    target, B, H, W, ld = _dice_ce_args(logits, target, what)
    n_regions = int(n_regions)
    if not 1 <= n_regions <= 24:
        raise ValueError(f"{what}: {n_regions} regions (1 .. 24)")
    if not (isinstance(table, torch.Tensor) and table.is_cuda and table.dtype == torch.int32 and table.is_contiguous() and table.numel() == 256):
        raise ValueError(f"{what}: `table` must be the membership table as nnunet.region_table_tensor(table, device) gives it: int32 [256] on the device")
    return target, B, H, W, ld, n_regions


def _region_form(region_loss, what):
    if region_loss not in ("focal", "bce"):
        raise ValueError(f"{what}: region_loss {region_loss!r} is neither 'focal' nor 'bce'")
    return int(region_loss == "bce")


def dice_focal_nacc(n_regions):
    """Doubles per row of the region loss's statistics (ldiff_op_dice_focal_nacc): sum_pred, intersect, sum_gt per padded region, the focal / BCE sum, the count
    of bad labels, the count of annotated pixels."""
    return 3 * 8 * ((int(n_regions) + 7) // 8) + 3


def dice_focal(logits, target, table, n_regions, batch_dice, weight=1.0, grad_scale=1.0, smooth=1e-5, use_ignore=False, region_loss="focal"):
    """ldiff_op_dice_focal on float16 logits [B, H, W, roundup(n_regions, 8)] and the uint8 / int64 LABEL MAP [B, H, W] (or [B, 1, H, W]): the reference's
    DC_and_Focal_loss (`region_loss="bce"`: nnU-Net's DC_and_BCE_loss) of one scale -> (loss float32 0-dim, dlogits float16 = grad_scale * weight * d loss /
    d logits).  `table`: the membership table on the device; `use_ignore`: pixels whose label carries the table's ignore bit take no part."""
    what = "dice_focal"
    target, B, H, W, ld, n = _region_args(logits, target, table, n_regions, what)
    bce = _region_form(region_loss, what)
    lib = _lib.load()
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits)
    nb = lib.ldiff_op_dice_focal_ws_bytes(B, H * W, n)
    ws = _workspace(nb, logits.device)
    _lib.check(lib.ldiff_op_dice_focal(logits.data_ptr(), ld, n, table.data_ptr(), target.data_ptr(), int(target.dtype == torch.int64), int(bool(use_ignore)), bce, B,
                                       H * W, int(bool(batch_dice)), float(smooth), float(weight), float(grad_scale), loss.data_ptr(), dlogits.data_ptr(),
                                       ws.data_ptr(), nb, _sp()))
    return loss[0], dlogits


def dice_focal_stats(logits, target, table, n_regions, batch_dice, out=None, use_ignore=False, region_loss="focal"):
    """ldiff_op_dice_focal_stats: the sums `dice_focal` forms before its coefficients, float64 [1 or B, dice_focal_nacc(n_regions)] on the device, added in
    dice_focal's order.  `out` as dice_ce_stats'."""
    what = "dice_focal_stats"
    target, B, H, W, ld, n = _region_args(logits, target, table, n_regions, what)
    bce = _region_form(region_loss, what)
    lib = _lib.load()
    rows, nacc = (1 if batch_dice else B), dice_focal_nacc(n)
    if out is None:
        out = torch.empty((rows, nacc), dtype=torch.float64, device=logits.device)
    elif not (out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() == rows * nacc):
        raise ValueError(f"{what}: out must be a contiguous float64 CUDA tensor of {rows * nacc} elements")
    nb = lib.ldiff_op_dice_focal_ws_bytes(B, H * W, n)
    ws = _workspace(nb, logits.device)
    _lib.check(lib.ldiff_op_dice_focal_stats(logits.data_ptr(), ld, n, table.data_ptr(), target.data_ptr(), int(target.dtype == torch.int64), int(bool(use_ignore)),
                                             bce, B, H * W, int(bool(batch_dice)), out.data_ptr(), ws.data_ptr(), nb, _sp()))
    return out


def dice_focal_from_sums(logits, target, table, n_regions, batch_dice, dice_sums, local_sums, world=1, weight=1.0, grad_scale=1.0, smooth=1e-5, use_ignore=False,
                         region_loss="focal"):
    """ldiff_op_dice_focal_from_sums: (loss, dlogits) as `dice_focal` returns them, the Dice term from `dice_sums` (with `batch_dice` possibly the sum of `world`
    processes' statistics; its gradient then carries the factor `world`), the focal / BCE term from `local_sums`.  With `use_ignore` it is built for one
    process: world = 1 and `dice_sums` is `local_sums`, anything else raises NotImplementedError."""
    what = "dice_focal_from_sums"
    target, B, H, W, ld, n = _region_args(logits, target, table, n_regions, what)
    bce = _region_form(region_loss, what)
    lib = _lib.load()
    rows, nacc = (1 if batch_dice else B), dice_focal_nacc(n)
    for name, t in (("dice_sums", dice_sums), ("local_sums", local_sums)):
        if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() == rows * nacc):
            raise ValueError(f"{what}: {name} must be a contiguous float64 CUDA tensor of {rows * nacc} elements")
    local = int(world) == 1 and dice_sums.data_ptr() == local_sums.data_ptr()
    if not batch_dice and not local:
        raise ValueError(f"{what}: without batch_dice the Dice term is per sample and stays local (world = 1, dice_sums is local_sums)")
    if use_ignore and not local:
        raise NotImplementedError(f"{what}(use_ignore=True) with the statistics of world = {int(world)} processes: the data-parallel exchange with an ignore "
                                  "label is not built")
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits)
    nb = lib.ldiff_op_dice_focal_ws_bytes(B, H * W, n)
    ws = _workspace(nb, logits.device)
    _lib.check(lib.ldiff_op_dice_focal_from_sums(logits.data_ptr(), ld, n, table.data_ptr(), target.data_ptr(), int(target.dtype == torch.int64),
                                                 int(bool(use_ignore)), bce, B, H * W, int(bool(batch_dice)), float(smooth), float(weight), float(grad_scale),
                                                 dice_sums.data_ptr(), local_sums.data_ptr(), int(world), loss.data_ptr(), dlogits.data_ptr(), ws.data_ptr(), nb, _sp()))
    return loss[0], dlogits


class DiceFocalFn(torch.autograd.Function):
    """DiceCeFn for region labels: `weight` * the region loss of one deep-supervision scale; value, stored gradient and backward as DiceCeFn's."""

    @staticmethod
    def forward(ctx, logits, target, table, n_regions, batch_dice, weight, grad_scale, smooth=1e-5, use_ignore=False, region_loss="focal"):
        loss, dlogits = dice_focal(logits, target, table, n_regions, batch_dice, weight, grad_scale, smooth, use_ignore, region_loss)
        ctx.save_for_backward(dlogits)
        return loss * float(weight)

    @staticmethod
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        return (dlogits.float() * g).to(dlogits.dtype), None, None, None, None, None, None, None, None, None


class DiceFocalSumsFn(torch.autograd.Function):
    """DiceFocalFn with the statistics supplied: the term of a data-parallel rank, as DiceCeSumsFn is DiceCeFn's."""

    @staticmethod
    def forward(ctx, logits, target, table, n_regions, batch_dice, dice_sums, local_sums, world, weight, grad_scale, smooth=1e-5, use_ignore=False, region_loss="focal"):
        loss, dlogits = dice_focal_from_sums(logits, target, table, n_regions, batch_dice, dice_sums, local_sums, world, weight, grad_scale, smooth, use_ignore,
                                             region_loss)
        ctx.save_for_backward(dlogits)
        return loss * float(weight)

    @staticmethod
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        return (dlogits.float() * g).to(dlogits.dtype), None, None, None, None, None, None, None, None, None, None, None, None


def region_counts(logits, target, table, n_regions, threshold):
    """ldiff_op_region_counts: int64 [3, n_regions] on the device = tp, fp, fn of `logit > threshold` against the table's region bits, over the pixels whose
    label does not carry the ignore bit; exact."""
    what = "region_counts"
    target, B, H, W, ld, n = _region_args(logits, target, table, n_regions, what)
    lib = _lib.load()
    out = torch.empty((3, n), dtype=torch.int64, device=logits.device)
    nb = lib.ldiff_op_region_counts_ws_bytes(B, H * W, n)
    ws = _workspace(nb, logits.device)
    _lib.check(lib.ldiff_op_region_counts(logits.data_ptr(), ld, n, table.data_ptr(), target.data_ptr(), int(target.dtype == torch.int64), B, H * W, float(threshold),
                                          out.data_ptr(), ws.data_ptr(), nb, _sp()))
    return out
