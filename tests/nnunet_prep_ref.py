"""float64 restatement of nnU-Net's per-case normalisation (`nnunet.normalize`, default_normalization_schemes.py) and the per-element bound on what
ldiff_op_case_apply may differ from it by, derived from the roundings the kernel makes.  No constant here is fitted to a measurement.

The kernel forms, per channel,   q = fl32( fl32(x - s32) / d32 )   with s32 = fl32(s'), d32 = fl32(d'), where s', d' are the host's float64 subtrahend and
divisor: (mean, max(std, 1e-8)) for ZScoreNormalization, (min, max(fl32(max - min), 1e-8)) for RescaleTo01Normalization, (0, 255) for RGBTo01Normalization and
(0, 1) for NoNormalization.  The restatement is t = (x - s) / d with s, d exact to float64.

With u = 2^-24 (float32 unit roundoff), a = fl32(x - s32) = (x - s32)(1 + e1), q = (a / d32)(1 + e2), |e1|, |e2| <= u, |s32 - s'| <= u |s'|, |d32 - d'| <= u d':
    q - t = (a / d32) e2 + [ (x - s32) e1 + (s - s32) + (x - s)(1 - d32 / d) ] / d32
    |q - t| <= u |a / d32| + [ u |x - s32| + |s - s32| + |x - s| |1 - d32 / d| ] / d32
|s - s32| <= u |s'| + |s' - s| and |1 - d32 / d| <= u (1 + r) + r with r = |d' - d| / d: what the host's float64 evaluation of s', d' is off by.  For a uint8 image
the sums are exact integers, mean and variance correctly rounded quotients of them: |s' - s| <= 2^-53 |s|, r <= 2^-51 (a quotient and a square root).  For a
float32 image the kernel's float64 partial sums of n terms carry at most n 2^-53 sum|x| (any order), so |s' - s| <= n 2^-53 mean|x| and the variance
S2 / n - mean^2 is off by at most 2 n 2^-53 (mean(x^2) + mean|x|^2) =: e_var, r <= e_var / (2 d^2) + 2^-51 (first order in the square root, doubled below for
the higher orders).  One float32 subnormal spacing (2^-149) covers a quotient that underflows; the bound itself is evaluated in float64 and widened by
2^-30 for that."""
import numpy as np

U = 2.0 ** -24


def _host_slack(x64: np.ndarray, is_u8: bool, s: float, d: float, scheme: str):
    """(|s' - s|, r): what the host's float64 subtrahend / divisor may be off by (module docstring)."""
    if scheme != "ZScoreNormalization":
        return 0.0, 0.0              # min, max and their float32 difference are exact data values / one float32 rounding (counted in u)
    if is_u8:
        return 2.0 ** -53 * abs(s), 2.0 ** -51
    n = x64.size
    e_sum = n * 2.0 ** -53
    e_var = 2 * e_sum * (float(np.mean(x64 * x64)) + float(np.mean(np.abs(x64))) ** 2)
    return e_sum * float(np.mean(np.abs(x64))), 2 * (e_var / (2 * d * d)) + 2.0 ** -51


def exact_scalars(x64: np.ndarray, scheme: str):
    """(s, d) of t = (x - s) / d in float64."""
    if scheme == "ZScoreNormalization":
        return float(np.mean(x64)), max(float(np.std(x64)), 1e-8)
    if scheme == "RGBTo01Normalization":
        return 0.0, 255.0
    if scheme == "RescaleTo01Normalization":
        return float(x64.min()), max(float(x64.max() - x64.min()), 1e-8)
    if scheme == "NoNormalization":
        return 0.0, 1.0
    raise ValueError(scheme)


def normalize_with_bound(x: np.ndarray, schemes, sub32: np.ndarray, div32: np.ndarray):
    """x [C, h, w] uint8 or float32; sub32 / div32: the float32 scalars the kernel was given.  Returns (t [C, h, w] float64, bound [C, h, w] float64)."""
    is_u8 = x.dtype == np.uint8
    t, bound = np.empty(x.shape, np.float64), np.empty(x.shape, np.float64)
    for c, scheme in enumerate(schemes):
        x64 = x[c].astype(np.float64)
        s, d = exact_scalars(x64, scheme)
        t[c] = (x64 - s) / d
        s32, d32 = float(np.float32(sub32[c])), float(np.float32(div32[c]))
        ds, r = _host_slack(x64, is_u8, s, d, scheme)
        a = (x[c].astype(np.float32) - np.float32(s32)).astype(np.float64)       # fl32(x - s32), as the kernel forms it
        e_s = abs(s32 - s) if scheme != "ZScoreNormalization" else U * (abs(s) + ds) + ds
        e_d = abs(1.0 - d32 / d) if scheme != "ZScoreNormalization" else U * (1 + r) + r
        bound[c] = (U * np.abs(a / d32) + (U * np.abs(x64 - s32) + e_s + np.abs(x64 - s) * e_d) / d32 + 2.0 ** -149) * (1 + 2.0 ** -30)
    return t, bound


def torch_reduction_bound(x: np.ndarray, schemes, sub32: np.ndarray, div32: np.ndarray):
    """What `nnunet.normalize` on the host (torch float32 reductions for mean and std) may differ from t by: the same formula with the subtrahend and the
    divisor known only to the worst case of a float32 summation of n terms in ANY order, (n - 1) u sum|x| (Higham, Accuracy and Stability, eq. 4.4):
    |mean32 - mean| <= n u mean|x|, and for the standard deviation sqrt(var) with var off by at most 2 n u (mean(x^2) + mean|x|^2)."""
    t, bound = np.empty(x.shape, np.float64), np.empty(x.shape, np.float64)
    for c, scheme in enumerate(schemes):
        x64 = x[c].astype(np.float64)
        s, d = exact_scalars(x64, scheme)
        t[c] = (x64 - s) / d
        if scheme != "ZScoreNormalization":      # the host forms the same float32 operations as the kernel
            bound[c] = normalize_with_bound(x[c:c + 1], [scheme], sub32[c:c + 1], div32[c:c + 1])[1][0]
            continue
        n = x64.size
        e_s = n * U * float(np.mean(np.abs(x64))) + U * abs(s)
        e_var = 2 * n * U * (float(np.mean(x64 * x64)) + float(np.mean(np.abs(x64))) ** 2)
        e_d = 2 * e_var / (2 * d * d) + 2 * U
        bound[c] = (U * np.abs(t[c]) * (1 + e_d) + (U * (np.abs(x64 - s) + e_s) + e_s + np.abs(x64 - s) * e_d) / (d * (1 - e_d)) + 2.0 ** -149) * (1 + 2.0 ** -30)
    return t, bound
