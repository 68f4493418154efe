"""Float64 numpy restatement of the low-resolution simulation of ldiffusion_amd.nnunet_data / kernels_segaug.hip (SimulateLowResolutionTransform:
order-0 resize down, order-3 resize up, clip), of the device's cubic B-spline prefilter, and the error bounds of the float32 kernels against them.
tests/test_cpu_nnunet_lowres.py pins the restatement to scipy.ndimage.zoom; the GPU tests use it without scipy.  The skimage half of the rule
(resize(order, mode='edge', anti_aliasing=False) = zoom(mode='nearest', grid_mode=True) and a clip to the input's range, skimage >= 0.19) is restated
from the public package and not pinned: scikit-image is not a test dependency.

Bounds.  u = 2^-24; first-order in u, constants rounded up, per element (as tests/nnunet_data_ref.py).

  prefilter   One axis is  c+[0] = 6 s sum_k wgt(k) x[k];  c+[k] = 6 x[k] + z c+[k-1];  c[n-1] = L (c+[n-1] + z c+[n-2]);  c[k] = z (c[k+1] - c+[k]),
              z = sqrt(3) - 2.  Every output is a sum over paths input j -> causal distance d1 -> anti-causal distance d2 of weight
              6 |z|^(d1 + d2) (times |L| or |z|).  Roundings on a path of total distance d = d1 + d2, in the kernel's operation order:
                axis 0 (one thread walks the line)   causal step: 6 x, the fma, the rounded pole: 2 d1 + 2;  end value 4;  anti-causal step: subtract,
                                                     multiply, pole: 3 d2                                                     <= 6 + 3 d
                axis 1 (one wave scans the line)     per 64-sample chunk <= 6 shuffle levels and the carry, an fma and a rounded power each: 14 per
                                                     chunk crossed, <= 14 (d1 / 64 + 1) + 14 (d2 / 64 + 1);  6 x and -z c+: 2      <= 30 + d
              (30 + 3 d) |z|^d <= 30 Q^d with Q = 0.3 (|z| / Q = 0.893, and (1 + d / 10) 0.893^d < 1 for d >= 1), so these roundings are at most
              30 u M_Q(|input|), where M_q is the SAME recursion run on magnitudes with the pole q: every product positive, every constant at least
              the true one (q / (1 - q^2) >= |L|, 1 / (1 - q^(2n-2)) >= 1 / (1 - z^(2n-2)) for q >= |z|).
              The start sum has roundings of its own: axis 0 adds its <= 64 terms in sequence (64 fmas, a weight from two rounded table entries 3 u,
              scale and division 3 u), axis 1 by a product and six butterfly levels: <= 70 u sum_k |wgt(k) x[k]| on c+[0] alone, which then walks the
              line like an input at sample 0: the term 70 u S, S = sum_k wgt_Q(k) |x[k]|, is added to the source at sample 0.
              An input error e passes through the exact filter, whose path magnitudes are M_|z|'s: M_|z|(e).  The amplification 1 / (1 - |pole|) of
              each of the two recursive passes and the gain 6 enter through M (M_|z| has gain 6 x 1.366 x 0.366 = 3.0 per axis, M_Q 3.7).
                  e0 = M_Q,axis0(30 u |x| + 70 u S at 0) + M_|z|,axis0(e_in),   e1 = M_Q,axis1(30 u (|c0| + e0) + 70 u S at 0) + M_|z|,axis1(e0)
  taps        the 16-term fma sum (4 + 4 fmas per coefficient: 8 u of |wy wx c|), the weights (a cubic in t by at most 6 operations on terms <= 4 and
              t = rem / (2 n) itself one rounding: 17 u absolute each), and the coefficients' own error through the positive weights, which sum to 1:
                  u (8 sum |wy wx c| + 17 sum (wy + wx) |c|) + sum wy wx e1
  clip        1-Lipschitz in the value and in its two bounds; min d and max d are exact copies of inputs, so they err by the input's error only.
"""
import math

import numpy as np

import nnunet_data_ref as ref
from ldiffusion_amd.nnunet_data import spline_coefficients

U = ref.U
PAD = 12
Q = 0.3
Z = 2.0 - math.sqrt(3.0)   # |pole|
ROUNDINGS, START_ROUNDINGS = 30, 70


def lowres_shape(h, w, zoom):
    """np.round(shape * zoom) with the float32 product, half to even."""
    z = np.float32(zoom)
    return int(np.round(np.float32(h) * z)), int(np.round(np.float32(w) * z))


def is_on(h, w, zoom):
    z = np.float32(zoom)
    if not (z > 0 and z <= 1):   # NaN fails both
        return False
    m0, m1 = lowres_shape(h, w, z)
    return m0 >= 1 and m1 >= 1 and (m0, m1) != (h, w)


def down_index(n, m):
    """Order 0, grid_mode: the source index of target index i, floor((i + 1/2) n / m) in integers."""
    i = np.arange(m, dtype=np.int64)
    return ((2 * i + 1) * n) // (2 * m)


def up_coordinate(n, m):
    """Order 3, grid_mode: target index i of n reads source coordinate (i + 1/2) m / n - 1/2 = num / (2 n): (floor, fraction) from integers."""
    i = np.arange(n, dtype=np.int64)
    num = (2 * i + 1) * m - n
    return num // (2 * n), (num % (2 * n)) / (2.0 * n)


def _axis0(x):
    """spline_coefficients along axis 0 alone."""
    return spline_coefficients(x.T[:, None, :])[:, 0, :].T


def _magnitude_axis(a, axis, q=Q):
    """M of the module docstring along one axis: the recursion of spline_coefficients on magnitudes, every term positive, pole q."""
    c = np.moveaxis(np.array(a, dtype=np.float64), axis, 0)
    n = c.shape[0]
    if n == 1:
        return np.moveaxis(c, 0, axis)
    c = c * 6.0
    if n > 64:
        acc = sum((q ** k) * c[k] for k in range(64))
    else:
        acc = c[0] + (q ** (n - 1)) * c[n - 1]
        for k in range(1, n - 1):
            acc = acc + (q ** k + q ** (2 * n - 2 - k)) * c[k]
        acc = acc / (1.0 - q ** (2 * n - 2))
    c[0] = acc
    for k in range(1, n):
        c[k] += q * c[k - 1]
    c[n - 1] = (q / (1.0 - q * q)) * (c[n - 1] + q * c[n - 2])
    for k in range(n - 2, -1, -1):
        c[k] = q * (c[k + 1] + c[k])
    return np.moveaxis(c, 0, axis)


def _axis_bound(mag, e_in, axis):
    """One axis of the prefilter's bound: `mag` bounds the magnitude of the axis's input as the kernel sees it, `e_in` its error."""
    n = mag.shape[axis]
    if n == 1:
        return e_in
    m = np.moveaxis(mag, axis, 0)
    hz = min(n, 64)
    wgt = [Q ** k if (n > 64 or k in (0, n - 1)) else Q ** k + Q ** (2 * n - 2 - k) for k in range(hz)]
    src = np.moveaxis(ROUNDINGS * U * mag, axis, 0).copy()
    src[0] += START_ROUNDINGS * U * sum(wk * m[k] for k, wk in enumerate(wgt))
    return _magnitude_axis(np.moveaxis(src, 0, axis), axis, Q) + _magnitude_axis(e_in, axis, Z)


def prefilter(x, e_in=0.0):
    """spline_coefficients of one [H, W] plane and the bound of the device's float32 prefilter against it."""
    x = np.asarray(x, np.float64)
    e_in = np.broadcast_to(np.asarray(e_in, np.float64), x.shape)
    e0 = _axis_bound(np.abs(x), e_in, 0)
    e1 = _axis_bound(np.abs(_axis0(x)) + e0, e0, 1)
    return spline_coefficients(x), e1


def _bspline1(t):
    return np.stack([np.zeros_like(t), 1.0 - t, t, np.zeros_like(t)])


def lowres(x, zoom, e_in=0.0, up_order=3, pad_mode="edge", grid=True, clip=True):
    """The rule of include/ldiff.h (ldiff_op_seg_intensity_lr) on one [h, w] plane in float64 with the float32 table value `zoom`: (result, bound).  An off row returns (x, e_in).
    The keywords state the WRONG variants the tests must tell apart: order-1 up-sampling, a mirror for the edge pad, sample centres without
    grid_mode (index i of n at i (m - 1) / (n - 1)), no clip."""
    x = np.asarray(x, np.float64)
    h, w = x.shape
    e_in = np.broadcast_to(np.asarray(e_in, np.float64), x.shape)
    if not is_on(h, w, zoom):
        return x, e_in
    m = lowres_shape(h, w, zoom)
    if grid:
        iy, ix = down_index(h, m[0]), down_index(w, m[1])
        (fy, ty), (fx, tx) = up_coordinate(h, m[0]), up_coordinate(w, m[1])
    else:
        src = [np.arange(m[a]) * ((n - 1) / max(m[a] - 1, 1)) for a, n in enumerate((h, w))]
        iy, ix = (np.floor(s + 0.5).astype(np.int64) for s in src)
        dst = [np.arange(n) * ((m[a] - 1) / max(n - 1, 1)) for a, n in enumerate((h, w))]
        (fy, ty), (fx, tx) = ((np.floor(s).astype(np.int64), s - np.floor(s)) for s in dst)
    d = x[np.ix_(iy, ix)]
    e_d = e_in[np.ix_(iy, ix)]
    padded = np.pad(d, PAD, "edge" if pad_mode == "edge" else "reflect")   # numpy's 'reflect' mirrors at whole samples
    coef, e_c = prefilter(padded, np.pad(e_d, PAD, "edge"))
    if up_order == 1:
        coef, e_c = padded, np.pad(e_d, PAD, "edge")
    weights = ref._bspline3 if up_order == 3 else _bspline1
    wy, wx = weights(ty), weights(tx)
    val, mag, wmag, err = (np.zeros((h, w)) for _ in range(4))
    Hp, Wp = coef.shape
    for a in range(4):
        ry = np.clip(fy - 1 + a + PAD, 0, Hp - 1)
        for b in range(4):
            rx = np.clip(fx - 1 + b + PAD, 0, Wp - 1)
            c = coef[np.ix_(ry, rx)]
            wgt = wy[a][:, None] * wx[b][None, :]
            val += wgt * c
            mag += wgt * np.abs(c)
            wmag += (wy[a][:, None] + wx[b][None, :]) * np.abs(c)
            err += wgt * e_c[np.ix_(ry, rx)]
    bound = U * (8 * mag + 17 * wmag) + err
    if clip:
        val = np.clip(val, d.min(), d.max())
        bound = np.maximum(bound, float(e_in.max()))
    return val, bound


def chain(x, sigma_noise, z, ch, e_in=0.0, lowres_after_gammas=False, **variant):
    """tests/nnunet_data_ref.chain with the low-resolution simulation between contrast and the gammas, the kernel's (and nnU-Net's) order;
    `lowres_after_gammas` states the wrong order."""
    e = ref._arr(e_in, x)
    if sigma_noise > 0:
        x, e = ref.noise(x, np.float32(sigma_noise), z, e)
    if ch["blur_sigma"] > 0:
        x, e = ref.blur(x, ch["blur_sigma"], e)
    if ch["brightness"] != 1:
        x, e = ref.brightness(x, ch["brightness"], e)
    if ch["contrast"] > 0:
        x, e = ref.contrast(x, ch["contrast"], e)
    if not lowres_after_gammas:
        x, e = lowres(x, ch["lowres_zoom"], e, **variant)
    if ch["gamma_inverted"] > 0:
        x, e = ref.gamma(x, ch["gamma_inverted"], True, e)
    if ch["gamma"] > 0:
        x, e = ref.gamma(x, ch["gamma"], False, e)
    if lowres_after_gammas:
        x, e = lowres(x, ch["lowres_zoom"], e, **variant)
    return x, e


def step_plane(h, w, seed):
    """A smooth random plane with a step in it: what separates the wrong variants."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((h + 2, w + 2))
    x = (x[:-2, :-2] + x[1:-1, 1:-1] + x[2:, 2:] + x[:-2, 2:] + x[2:, :-2]) * 0.5 + 0.3
    x[h // 3:, w // 2:] += 2.0
    return x.astype(np.float32)


def block_plane(h, w):
    """A block at the plane's maximum beside one at its minimum on a smooth ramp: the cubic overshoots at the blocks' edges, so the clip bites."""
    i, j = np.mgrid[:h, :w]
    x = 0.02 * i + 0.01 * j
    x[h // 4:h // 2, w // 4:w // 2] = 3.0
    x[h // 4:h // 2, w // 2:3 * w // 4] = -2.0
    return x.astype(np.float32)


# chain rows on which the order of the step and the gammas shows beyond ten times the chain's bound: contrast, the step and one gamma
ORDER_ROWS = [dict(contrast=1.2, lowres_zoom=0.5, gamma=1.5), dict(contrast=1.2, lowres_zoom=0.53, gamma_inverted=1.5), dict(contrast=0.8, lowres_zoom=0.77, gamma=0.7)]


def chan_row(**values):
    """One CHAN_DTYPE row: everything off but `values`."""
    from ldiffusion_amd.nnunet_data import CHAN_DTYPE
    ch = np.zeros((), CHAN_DTYPE)
    ch["brightness"] = 1.0
    for key, v in values.items():
        ch[key] = v
    return ch
