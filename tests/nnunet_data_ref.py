"""Float64 numpy restatements of the training-data rules of ldiffusion_amd.nnunet_data / kernels_segaug.hip (spatial transform, cubic data sampling,
label vote, noise, blur, brightness, contrast, gamma, mirror, deep-supervision targets), each with the error bound of the float32 kernel against it.
The restatements take the float32 table values the kernels take.  tests/test_cpu_nnunet_data.py pins them to scipy; the GPU tests use them without it.

Bounds.  u = 2^-24 (float32 unit roundoff).  They are first-order in u with the stated constants rounded up, per element unless noted.

  reduction   a plane's sum is formed as: per thread a sequential sum over its strided walk (at most T(n) = max(4 ceil(n / 4096), ceil(n / 1024)) terms:
              1024 threads, float4 or scalar loads), a 6-level butterfly, then the 16 wave partials in sequence: every input passes through at most
              K(n) = T(n) + 6 + 15 additions, so |sum^ - sum| <= K(n) u sum|x|.  min / max are exact.
  power       powf is documented within 2 ulp of the true value in HIP's device math: relative 4 u.
"""
import math

import numpy as np

U = 2.0 ** -24
POW_REL = 4 * U
THREADS = 1024


def K(n: int) -> int:
    return max(4 * math.ceil(n / (4 * THREADS)), math.ceil(n / THREADS)) + 6 + 15


def sum_err(x) -> float:
    return 1.01 * K(x.size) * U * float(np.abs(x).sum())


# ---- spatial ---------------------------------------------------------------------------------------------------------------------------------
def coordinates(m, h, w):
    """Patch index -> case coordinate by the float32 matrix, in float64, and the bound of the kernel's float32 evaluation fma(m0, i, fma(m1, j, m2)):
    two roundings, each of a partial sum no larger than |m0 i| + |m1 j| + |m2|."""
    m = np.asarray(m, np.float32).astype(np.float64)
    i, j = np.mgrid[:h, :w].astype(np.float64)
    y = m[0] * i + m[1] * j + m[2]
    x = m[3] * i + m[4] * j + m[5]
    ey = 2 * U * (np.abs(m[0] * i) + np.abs(m[1] * j) + abs(m[2]))
    ex = 2 * U * (np.abs(m[3] * i) + np.abs(m[4] * j) + abs(m[5]))
    return y, x, ey, ex


def spatial_coordinates(patch, loader_patch, bbox_lbs, angle, zoom, flip):
    """Rules 1 and 10 without a matrix: SpatialTransform(random_crop=False, no elastic deformation) followed by MirrorTransform, as the case coordinate
    (y, x) of every patch pixel.  The centred grid g = (i - (h-1)/2, j - (w-1)/2); rotated by batchgenerators' rotate_coords_2d,
    (r, c) -> (r cos a + c sin a, -r sin a + c cos a); times the scale; plus the centre of the loader's crop, bbox_lbs + (loader_patch - 1) / 2.
    Mirroring an axis of the OUTPUT reverses the coordinate arrays along that axis (np.flip): every step between the two transforms is pointwise or
    symmetric."""
    h, w = patch
    i, j = np.mgrid[:h, :w].astype(np.float64)
    g0, g1 = i - (h - 1) / 2.0, j - (w - 1) / 2.0
    r0 = g0 * math.cos(angle) + g1 * math.sin(angle)
    r1 = -g0 * math.sin(angle) + g1 * math.cos(angle)
    y = r0 * zoom + bbox_lbs[0] + (loader_patch[0] - 1) / 2.0
    x = r1 * zoom + bbox_lbs[1] + (loader_patch[1] - 1) / 2.0
    for axis in (0, 1):
        if flip[axis]:
            y, x = np.flip(y, axis), np.flip(x, axis)
    return y, x


def centre_crop_coordinates(patch, loader_patch, bbox_lbs, flip):
    """Without rotation and scale batchgenerators takes the integer centre crop of the loader's crop: first index bbox_lbs + (loader_patch - patch) // 2;
    then the mirror as above."""
    h, w = patch
    i, j = np.mgrid[:h, :w]
    y = i + int(bbox_lbs[0]) + (int(loader_patch[0]) - h) // 2
    x = j + int(bbox_lbs[1]) + (int(loader_patch[1]) - w) // 2
    for axis in (0, 1):
        if flip[axis]:
            y, x = np.flip(y, axis), np.flip(x, axis)
    return y, x


def _bspline3(t):
    s = 1.0 - t
    return np.stack([s ** 3 / 6, (4 - 6 * t ** 2 + 3 * t ** 3) / 6, (4 - 6 * s ** 2 + 3 * s ** 3) / 6, t ** 3 / 6])


def _bspline3_d(t):
    s = 1.0 - t
    return np.stack([-s ** 2 / 2, (-4 * t + 3 * t ** 2) / 2, (4 * s - 3 * s ** 2) / 2, t ** 2 / 2])


def _mirror(i, n):
    i = np.abs(i)
    i = np.where(i > n - 1, 2 * (n - 1) - i, i)
    return np.clip(i, 0, n - 1)


def cubic_sample(coef, y, x, ey=0.0, ex=0.0):
    """scipy.ndimage.map_coordinates(order=3, mode='constant', cval=0, prefilter=False) on coefficients [C, H, W] at (y, x): 4 x 4 B-spline taps
    mirrored at whole samples, 0 where a coordinate leaves [0, n - 1].  Returns (values [C, ...], bound [C, ...], edge): `edge` marks the points whose
    coordinate is within its own rounding of the border of validity, where kernel and restatement may differ by the whole value.
    bound = u (8 sum|wy wx c| + 16 sum (wy + wx)|c|)       the 16-term fma sum (4 + 4 fmas per element) and the weights' own rounding (each weight a
                                                            cubic in t by at most 6 operations on terms <= 4: absolute error <= 16 u)
          + ey |df/dy| + ex |df/dx| + u max|c|             the coordinate rounding through the spline's derivative; the second-order rest is far below u"""
    coef = np.asarray(coef, np.float64)
    Cc, H, W = coef.shape
    inside = (y >= 0) & (y <= H - 1) & (x >= 0) & (x <= W - 1)
    edge = (np.abs(y) <= ey) | (np.abs(y - (H - 1)) <= ey) | (np.abs(x) <= ex) | (np.abs(x - (W - 1)) <= ex)
    fy, fx = np.floor(y), np.floor(x)
    wy, wx, dy, dx = _bspline3(y - fy), _bspline3(x - fx), _bspline3_d(y - fy), _bspline3_d(x - fx)
    val = np.zeros((Cc,) + y.shape)
    mag, wmag, gy, gx = np.zeros_like(val), np.zeros_like(val), np.zeros_like(val), np.zeros_like(val)
    for a in range(4):
        iy = _mirror(fy.astype(np.int64) - 1 + a, H)
        for b in range(4):
            ix = _mirror(fx.astype(np.int64) - 1 + b, W)
            c = coef[:, iy, ix]
            val += wy[a] * wx[b] * c
            mag += wy[a] * wx[b] * np.abs(c)
            wmag += (wy[a] + wx[b]) * np.abs(c)
            gy += dy[a] * wx[b] * c
            gx += wy[a] * dx[b] * c
    bound = U * (8 * mag + 16 * wmag) + ey * np.abs(gy) + ex * np.abs(gx) + U * np.abs(coef).max()
    return np.where(inside, val, 0.0), np.where(inside, bound, 0.0), edge


def vote_labels(seg, y, x, n_heads):
    """interpolate_img(is_seg=True, order=1, cval=-1) + RemoveLabelTransform(-1, 0): per label the bilinear weight on it, the highest label whose weight
    reaches 0.5, else 0; 0 outside the image.  Returns (labels uint8, near): `near` marks the points where some label's weight lies within 1e-3 of 0.5."""
    seg = np.asarray(seg)
    H, W = seg.shape
    inside = (y >= 0) & (y <= H - 1) & (x >= 0) & (x <= W - 1)
    yc, xc = np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)
    fy, fx = np.floor(yc), np.floor(xc)
    ty, tx = yc - fy, xc - fx
    y0, x0 = fy.astype(np.int64), fx.astype(np.int64)
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
    out = np.zeros(y.shape, np.uint8)
    near = np.zeros(y.shape, bool)
    for c in range(n_heads):
        ind = (seg == c).astype(np.float64)
        wsum = (1 - ty) * (1 - tx) * ind[y0, x0] + (1 - ty) * tx * ind[y0, x1] + ty * (1 - tx) * ind[y1, x0] + ty * tx * ind[y1, x1]
        out[wsum >= 0.5] = c
        near |= np.abs(wsum - 0.5) <= 1e-3
    return np.where(inside, out, 0).astype(np.uint8), near & inside


def copy_crop(raw, seg, m, h, w):
    """A copy-mode sample: y = m0 i + m2, x = m4 j + m5 with integer values; zero / background outside."""
    m = np.asarray(m, np.float64)
    i, j = np.mgrid[:h, :w]
    y, x = (int(m[0]) * i + int(m[2])), (int(m[4]) * j + int(m[5]))
    H, W = seg.shape
    inside = (y >= 0) & (y < H) & (x >= 0) & (x < W)
    yc, xc = np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)
    return np.where(inside, raw[:, yc, xc], 0).astype(raw.dtype), np.where(inside, seg[yc, xc], 0).astype(np.uint8)


def ds_indices(k: int, n: int):
    """DownsampleSegForDSTransform2 (order 0) at scale 2^-k: the full-resolution index behind output index i (k = 0: the identity)."""
    return np.arange(n >> k) * (1 << k) + ((1 << k) >> 1)


# ---- intensity -------------------------------------------------------------------------------------------------------------------------------
def _arr(e, like):
    return np.broadcast_to(np.asarray(e, np.float64), like.shape)


def noise(x, sigma, z, e_in=0.0):
    """GaussianNoiseTransform given the draw: x + sigma z.  One fma."""
    y = x + float(sigma) * z
    return y, _arr(e_in, x) + U * np.abs(y)


def _reflect(i, n):
    i = np.asarray(i)
    while ((i < 0) | (i >= n)).any():
        i = np.where(i < 0, -i - 1, i)
        i = np.where(i >= n, 2 * n - 1 - i, i)
    return i


def _blur_axis(x, sigma, axis):
    radius = int(4.0 * float(sigma) + 0.5)
    k = np.arange(-radius, radius + 1)
    wgt = np.exp(-0.5 * (k / float(sigma)) ** 2)
    wgt /= wgt.sum()
    n = x.shape[axis]
    out = np.zeros_like(x)
    for kk, wk in zip(k, wgt):
        out += wk * np.take(x, _reflect(np.arange(n) + kk, n), axis=axis)
    return out


def blur(x, sigma, e_in=0.0):
    """scipy.ndimage.gaussian_filter(x, sigma) on [h, w]: axis 0 then axis 1, radius int(4 sigma + 0.5), normalised taps, 'reflect' borders.
    A normalised tap carries relative error <= 64 u (expf within 2 ulp of an argument of magnitude <= 11 known to 2 u, the 9-term sum, the reciprocal
    and the product), a pass is a chain of <= 9 fmas: each pass errs by <= 73 u blur(|input|); asserted with 80 u."""
    sigma = float(np.float32(sigma))
    v = _blur_axis(x, sigma, 0)
    y = _blur_axis(v, sigma, 1)
    e = _blur_axis(_blur_axis(_arr(e_in, x), sigma, 0), sigma, 1)
    e = e + 80 * U * (_blur_axis(_blur_axis(np.abs(x), sigma, 0), sigma, 1) + _blur_axis(np.abs(v), sigma, 1))
    return y, e


def brightness(x, mult, e_in=0.0):
    y = x * float(mult)
    return y, abs(float(mult)) * _arr(e_in, x) + U * np.abs(y)


def _mean_err(x, e_in):
    return sum_err(x) / x.size + U * abs(float(x.mean())) + float(np.mean(e_in))


def contrast(x, f, e_in=0.0):
    """ContrastAugmentationTransform: clip((x - mean) f + mean, min, max).  d = x - mean^ (one rounding), fma(d, f, mean^) (one); clip is 1-Lipschitz
    in the value and in its two bounds, whose error is that of the input."""
    f, e_in = float(f), _arr(e_in, x)
    m, lo, hi = x.mean(), x.min(), x.max()
    e_m = _mean_err(x, e_in)
    pre = (x - m) * f + m
    e_pre = f * (e_in + e_m + U * np.abs(x - m)) + e_m + U * np.abs(pre)
    return np.clip(pre, lo, hi), np.maximum(e_pre, e_in.max())


def gamma(x, g, invert, e_in=0.0):
    """GammaTransform(retain_stats=True) with the issue's seven steps.  The bound follows the kernel's operations one by one; the power's input error
    goes through the exact increments of t -> t^g over [b - e_b, b + e_b] (no derivative: it is unbounded at 0 for g < 1)."""
    g, e_in = float(g), _arr(e_in, x)
    if invert:
        x = -x
    n = x.size
    m, s, lo, hi = x.mean(), x.std(), x.min(), x.max()
    r = hi - lo
    e_max = float(e_in.max())
    e_m = _mean_err(x, e_in)
    # the std is 1-Lipschitz in the rms norm of the data; a centre off by e_m adds at most e_m; squares, sum, division, root: (K + 8) u relative
    e_s = math.sqrt(float(np.mean(e_in ** 2))) + e_m + (K(n) + 8) * U * s
    e_r = 2 * e_max + U * r
    den = r + 1e-7
    e_den = e_r + U * den
    den_lo = max(den - e_den, 1e-7 * (1 - 2 * U))   # the computed range is >= 0
    b = (x - lo) / den
    e_b = (e_in + e_max + U * np.abs(x - lo)) / den_lo + (x - lo) * e_den / (den * den_lo) + U * b
    p = b ** g
    e_p = np.maximum((b + e_b) ** g - p, p - np.maximum(b - e_b, 0.0) ** g) + POW_REL * (b + e_b) ** g
    q = p * r + lo
    e_q = e_p * (r + e_r) + p * e_r + e_max + U * np.abs(q)
    m2 = q.mean()
    e_m2 = _mean_err(q, e_q)
    c = q - m2
    e_c = e_q + e_m2 + U * np.abs(c)
    s2 = q.std()
    e_s2 = math.sqrt(float(np.mean(e_q ** 2))) + e_m2 + (K(n) + 8) * U * s2
    D = s2 + 1e-8
    e_D = e_s2 + U * D
    D_lo = max(D - e_D, 1e-8 * (1 - 2 * U))
    ratio = c / D
    e_ratio = e_c / D_lo + np.abs(c) * e_D / (D * D_lo) + U * np.abs(ratio)
    # |c_i| <= sqrt(n) std(c) holds for the computed values too (the kernel's std is formed from the very differences it divides)
    ratio_max = np.minimum(np.abs(ratio) + e_ratio, 1.001 * math.sqrt(n))
    e_ratio = np.minimum(e_ratio, np.abs(ratio) + ratio_max)
    y = ratio * s + m
    e_y = e_ratio * s + ratio_max * e_s + e_m + U * np.abs(y)
    return (-y if invert else y), e_y


def chain(x, sigma_noise, z, ch, e_in=0.0):
    """Steps 4-7 and 9 in the kernel's order on one plane; `ch`: a CHAN_DTYPE row (0 = off, brightness 1 = off)."""
    e = _arr(e_in, x)
    if sigma_noise > 0:
        x, e = noise(x, np.float32(sigma_noise), z, e)
    if ch["blur_sigma"] > 0:
        x, e = blur(x, ch["blur_sigma"], e)
    if ch["brightness"] != 1:
        x, e = brightness(x, ch["brightness"], e)
    if ch["contrast"] > 0:
        x, e = contrast(x, ch["contrast"], e)
    if ch["gamma_inverted"] > 0:
        x, e = gamma(x, ch["gamma_inverted"], True, e)
    if ch["gamma"] > 0:
        x, e = gamma(x, ch["gamma"], False, e)
    return x, e
