"""The device image front end: `PIL.Image.resize(size, Image.BILINEAR)` of 8-bit images, bit for bit, on the HIP library (include/ldiff.h
ldiff_op_resize_u8, csrc/kernels_imgio.hip), optionally with ToTensor + Normalize behind it as a table -- the sampler's input in one step.

Pillow's rule for 8-bit data (src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc) is
integer arithmetic, so agreement is exact:
  * the horizontal pass runs first, then the vertical one; a pass is skipped when its side does not change; the intermediate image is uint8;
  * per output index xx:  scale = in / out, fs = max(scale, 1), support = fs, center = (xx + 0.5) * scale,
    xmin = max(int(center - support + 0.5), 0), xmax = min(int(center + support + 0.5), in) - xmin;
  * w[x] = tri((x + xmin - center + 0.5) * (1 / fs)) with tri(a) = max(1 - |a|, 0), summed in index order and divided, all in double;
  * k = int(0.5 + w * 2**22);  out = clip((2**21 + sum k[x] * src[xmin + x]) >> 22, 0, 255).
The tables are made here, on the host, in double, once per (in, out) pair, and uploaded once per device; the kernels only apply them.
`resize_u8_host` is the same two passes in numpy from the same tables: the rule can be tested without a GPU.

`size` is Pillow's: (width, height).  Out of scope: BICUBIC / LANCZOS / NEAREST, reducing_gap, box arguments, 16-bit and float modes."""
from __future__ import annotations

import functools
import math

import numpy as np

PRECISION_BITS = 22
ROUND = 1 << (PRECISION_BITS - 1)
MAX_TAPS = 128   # LDIFF_RESIZE_MAX_TAPS: the longest coefficient row the kernel takes = reductions up to 63x (16x has 33 taps)


def _side(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
        raise ValueError(f"{name} = {v!r}: a side must be an integer >= 1")
    return int(v)


@functools.lru_cache(maxsize=64)
def _window_weights(in_size: int, out_size: int):
    """The double stage of one pass in_size -> out_size: (xmin int64 [out], xmax int64 [out] = window length, w float64 [out, taps]), the normalised
    triangle weights in index order, zeros behind a row's window."""
    in_size, out_size = _side("in_size", in_size), _side("out_size", out_size)
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    taps = int(math.ceil(support)) * 2 + 1
    if taps > MAX_TAPS:
        raise ValueError(f"size: {in_size} -> {out_size} needs a window of {taps} taps, the kernel takes {MAX_TAPS} (reductions up to {(MAX_TAPS - 1) // 2}x)")
    ss = 1.0 / fs
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)           # C's (int): truncation, and numpy's astype truncates too
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    w = np.zeros((out_size, taps), np.float64)
    ww = np.zeros(out_size, np.float64)
    for x in range(taps):                                                      # index order, as the C loop sums it
        a = np.abs(((x + xmin).astype(np.float64) - center + 0.5) * ss)
        col = np.where(x < xmax, np.where(a < 1.0, 1.0 - a, 0.0), 0.0)
        w[:, x] = col
        ww += col
    nz = ww != 0.0
    w[nz] /= ww[nz, None]
    for a in (xmin, xmax, w):
        a.setflags(write=False)
    return xmin, xmax, w


def weights(in_size: int, out_size: int):
    """(bounds int32 [out, 2] = (first source index, window length), w float64 [out, taps]) of one pass in_size -> out_size: the window rule above before
    it turns into integers.  These are the antialiased triangle weights of `F.interpolate(..., mode="bilinear", antialias=True, align_corners=False)`
    (the same window and the same normalisation), which the warm-up kernel applies in float32 (dataset.py, ldiff_op_warmup_images).  Read-only arrays."""
    xmin, xmax, w = _window_weights(in_size, out_size)
    bounds = np.stack([xmin, xmax], 1).astype(np.int32)
    bounds.setflags(write=False)
    return bounds, w


@functools.lru_cache(maxsize=64)
def coefficients(in_size: int, out_size: int):
    """(bounds int32 [out, 2] = (first source index, window length), coef int32 [out, taps]) of one pass in_size -> out_size; taps =
    ceil(max(in / out, 1)) * 2 + 1 as Pillow allocates it, zeros behind a row's window.  Cached; the arrays are read-only."""
    xmin, xmax, w = _window_weights(in_size, out_size)
    taps = w.shape[1]
    coef = np.where(w < 0, -0.5 + w * (1 << PRECISION_BITS), 0.5 + w * (1 << PRECISION_BITS)).astype(np.int32)
    coef[np.arange(taps)[None, :] >= xmax[:, None]] = 0
    bounds = np.stack([xmin, xmax], 1).astype(np.int32)
    bounds.setflags(write=False)
    coef.setflags(write=False)
    return bounds, coef


def resample_pass_host(src: np.ndarray, axis: int, out_size: int, round_const: int = ROUND) -> np.ndarray:
    """One pass of the rule along `axis` of a uint8 array, in numpy int64 (the sum fits int32; the kernels use that)."""
    bounds, coef = coefficients(src.shape[axis], out_size)
    s = np.moveaxis(src, axis, 0).astype(np.int64)
    n_in = s.shape[0]
    acc = np.full((out_size,) + s.shape[1:], round_const, np.int64)
    tail = (1,) * (s.ndim - 1)
    for j in range(coef.shape[1]):
        idx = np.minimum(bounds[:, 0].astype(np.int64) + j, n_in - 1)           # behind the window the coefficient is 0
        acc += coef[:, j].astype(np.int64).reshape((-1,) + tail) * s[idx]
    return np.moveaxis(np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8), 0, axis)


def _check_host(x):
    if not isinstance(x, np.ndarray) or x.dtype != np.uint8 or x.ndim not in (2, 3, 4):
        raise ValueError("x: a uint8 array [H, W], [H, W, C] or [B, H, W, C]")
    if x.ndim >= 3 and x.shape[-1] not in (1, 3):
        raise ValueError(f"x: {x.shape[-1]} channels: 1 or 3")
    if 0 in x.shape:
        raise ValueError(f"x: a side of 0 in shape {tuple(x.shape)}")


def _check_size(size):
    try:
        ow, oh = size
    except (TypeError, ValueError):
        raise ValueError(f"size = {size!r}: (width, height)") from None
    return _side("size[0]", ow), _side("size[1]", oh)


def resize_u8_host(x: np.ndarray, size) -> np.ndarray:
    """The numpy restatement: `Image.fromarray(x).resize(size, Image.BILINEAR)` for uint8 [H, W], [H, W, C] or [B, H, W, C], C = 1 or 3."""
    _check_host(x)
    ow, oh = _check_size(size)
    ay = 1 if x.ndim == 4 else 0
    h, w = x.shape[ay], x.shape[ay + 1]
    coefficients(w, ow), coefficients(h, oh)   # refusals before any work
    out = x
    if ow != w:
        out = resample_pass_host(out, ay + 1, ow)
    if oh != h:
        out = resample_pass_host(out, ay, oh)
    return out.copy() if out is x else out


# ---- the device side ---------------------------------------------------------------------------------------------------------------------------------
_device_tables: dict = {}
_norm_tables: dict = {}


def _tables(in_size, out_size, device):
    import torch
    key = (in_size, out_size, str(device))
    t = _device_tables.get(key)
    if t is None:
        bounds, coef = coefficients(in_size, out_size)
        t = _device_tables[key] = (torch.from_numpy(bounds.copy()).to(device), torch.from_numpy(coef.copy()).to(device), coef.shape[1])
    return t


def normalize_table(mean, std, device):
    """float32 [3, 256] on `device`: ToTensor + Normalize of the 256 grey levels, by the per-image path's own expression (utils.copy_or_convert_image):
    `np.float32 / 255.0` on the host, then `(x - mean) / std` in torch ON THE DEVICE it will run on -- so the table path and the per-image path agree
    bit for bit by construction, whatever the rounding of torch's division there.  Cached per (mean, std, device)."""
    import torch
    device = torch.device(device)
    key = (tuple(float(m) for m in mean), tuple(float(s) for s in std), str(device))
    if len(key[0]) != 3 or len(key[1]) != 3:
        raise ValueError("mean / std: three values each")
    t = _norm_tables.get(key)
    if t is None:
        grey = torch.from_numpy(np.arange(256, dtype=np.uint8).reshape(1, 256, 1).astype(np.float32) / 255.0).expand(1, 256, 3).permute(2, 0, 1)[None].to(device)
        m = torch.tensor(key[0], device=device).view(1, 3, 1, 1)
        s = torch.tensor(key[1], device=device).view(1, 3, 1, 1)
        t = _norm_tables[key] = ((grey - m) / s).reshape(3, 256).contiguous()
    return t


def unit_table(device):
    """float32 [3, 256] on `device`: ToTensor alone, `np.float32 / 255.0` as numpy divides on the host (torch's division by a scalar need not round as numpy's)."""
    import torch
    key = ("unit", str(torch.device(device)))
    t = _norm_tables.get(key)
    if t is None:
        t = _norm_tables[key] = torch.from_numpy(np.tile(np.arange(256, dtype=np.uint8).astype(np.float32) / 255.0, (3, 1))).to(device)
    return t


def _resize(x, size, lut):
    import ctypes as C

    import torch

    from . import _lib
    if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or x.dim() != 4:
        raise ValueError("x: a uint8 tensor [B, Hs, Ws, C]")
    B, Hs, Ws, Cc = x.shape
    if Cc not in (1, 3):
        raise ValueError(f"x: {Cc} channels: 1 or 3")
    if lut is not None and Cc != 3:
        raise ValueError(f"x: {Cc} channels: resize_normalize takes 3")
    if 0 in x.shape:
        raise ValueError(f"x: a side of 0 in shape {tuple(x.shape)}")
    ow, oh = _check_size(size)
    coefficients(Ws, ow), coefficients(Hs, oh)   # a window longer than MAX_TAPS raises here, naming `size`
    if not x.is_cuda:
        raise ValueError("x: a tensor on the GPU (there is no CPU fallback; resize_u8_host is the numpy restatement)")
    _lib.require_gpu()
    x = x.contiguous()
    lib = _lib.load()
    null = (None, None, 0)
    with torch.cuda.device(x.device):
        hb, hc, ht = _tables(Ws, ow, x.device) if ow != Ws else null
        vb, vc, vt = _tables(Hs, oh, x.device) if oh != Hs else null
        out = torch.empty((B, 3, oh, ow), device=x.device, dtype=torch.float32) if lut is not None else torch.empty((B, oh, ow, Cc), device=x.device, dtype=torch.uint8)
        nws = lib.ldiff_op_resize_u8_ws_bytes(B, Hs, Ws, Cc, oh, ow, int(lut is not None))
        ws = torch.empty((max(nws, 0),), device=x.device, dtype=torch.uint8) if nws > 0 else None
        _lib.check(lib.ldiff_op_resize_u8(_lib.ptr(x), B, Hs, Ws, Cc, oh, ow, _lib.ptr(hb), _lib.ptr(hc), ht, _lib.ptr(vb), _lib.ptr(vc), vt, _lib.ptr(lut), _lib.ptr(out),
                                          _lib.ptr(ws), C.c_int64(max(nws, 0)), _lib.stream_ptr()))
    return out


def resize_u8(x, size):
    """uint8 [B, Hs, Ws, C] on the GPU (C = 1 or 3, interleaved) -> uint8 [B, Ho, Wo, C] = `Image.resize(size, Image.BILINEAR)` of every image, bit for bit;
    size = (Wo, Ho).  Raises ValueError naming the argument for other channel counts, a side of 0 and a window above MAX_TAPS."""
    return _resize(x, size, None)


def resize_normalize(x, size, mean, std):
    """uint8 [B, Hs, Ws, 3] on the GPU -> float32 [B, 3, Ho, Wo]: Resize + ToTensor + Normalize(mean, std) as the per-image path computes them
    (`normalize_table`), in one library call: the sampler's input."""
    import torch
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError("x: a uint8 tensor [B, Hs, Ws, 3] on the GPU")
    lut = normalize_table(mean, std, x.device)
    return _resize(x, size, lut)


def resize_to_tensor(x, size):
    """uint8 [B, Hs, Ws, 3] on the GPU -> float32 [B, 3, Ho, Wo] in [0, 1]: Resize + ToTensor (`np.float32 / 255.0` of the resized bytes, `unit_table`)."""
    import torch
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError("x: a uint8 tensor [B, Hs, Ws, 3] on the GPU")
    return _resize(x, size, unit_table(x.device))
