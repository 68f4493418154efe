"""Float64 restatement of the region losses of nnU-Net's tissue head (TEST INFRASTRUCTURE ONLY) and the error bound of the library's region entries
(ldiff_op_dice_focal / _stats / _from_sums, csrc/kernels_segregion.hip).

The loss follows the public algorithm of the reference's DC_and_Focal_loss (FocalLoss: alpha 0.25, gamma 2) and of nnunetv2's DC_and_BCE_loss over
MemoryEfficientSoftDiceLoss(apply_nonlin=sigmoid, do_bg=True, smooth=1e-5) with a loss mask: the one-hot region target is the table lookup of the label
map; with an ignore label the Dice sums run over annotated pixels and the focal / BCE term is its sum over annotated elements divided by the number of
annotated PIXELS (not times R), without one it is the mean over all B R H W elements.  tests/test_cpu_nnunet_regions.py pins it to values recorded from
those modules (tests/golden/reference_dc_focal_loss.npz)."""
import numpy as np
import torch
import torch.nn.functional as F

import nnunet_train_ref as ref

U = ref.U
IGNORE_BIT, BAD_BIT = 1 << 31, 1 << 30
DICE_CHAIN = 16 + 6 + 2      # csrc/kernels_segregion.hip: 16 pixels per thread (DFL_PIX = 4096 over 256 threads), a 64-lane butterfly, four waves; then double
# expf and log1pf: the HIP math API's accuracy table (ROCm documentation, "HIP math API", single-precision device functions) gives a maximum error of 1 ulp
# for each.  One ulp of a float32 result r is at most 2^-23 |r| = 2 u |r|; the bound doubles the documented figure, as its stated margin: 2 ulp = 4 u.
E_EXP = 4 * U


def membership(target, table, R):
    """(y [B, R, H, W] float64, ignored [B, H, W] bool) of an integer label map through the uint32 [256] table."""
    m = torch.from_numpy(np.asarray(table, dtype=np.uint32).astype(np.int64))[target.long()]
    assert not (m & BAD_BIT).any(), "a label that is in no region, no label of the dataset and not the ignore label"
    y = torch.stack([(m >> r) & 1 for r in range(R)], 1).double()
    return y, (m & IGNORE_BIT) != 0


def dc_focal_loss(logits, target, table, batch_dice, use_ignore, form="focal", smooth=1e-5, wrong=None):
    """logits [B, R, H, W] (float64, differentiable), target integer [B, H, W] -> focal (or BCE) term - mean dc.
    `wrong`: a plausible WRONG loss the bounds must reject -- "norm": the ignore form's normaliser with the factor R (and the plain one without it);
    "M": the Dice mean over Bd (R - 1) terms; "dice_all": the Dice sums over all pixels instead of the annotated ones."""
    B, R = logits.shape[:2]
    y, ignored = membership(target, table, R)
    assert use_ignore or not ignored.any()
    m = (~ignored).double()[:, None]
    dm = torch.ones_like(m) if wrong == "dice_all" else m
    p = torch.sigmoid(logits)
    intersect, sum_pred, sum_gt = (p * y * dm).sum((2, 3)), (p * dm).sum((2, 3)), (y * dm).sum((2, 3))
    if batch_dice:
        intersect, sum_pred, sum_gt = intersect.sum(0), sum_pred.sum(0), sum_gt.sum(0)
    dc = (2 * intersect + smooth) / torch.clip(sum_gt + sum_pred + smooth, 1e-8)
    dice = dc.sum() / ((1 if batch_dice else B) * (R - 1)) if wrong == "M" else dc.mean()
    bce = F.binary_cross_entropy_with_logits(logits, y, reduction="none")
    if form == "focal":
        p_t = y * p + (1 - y) * (1 - p)
        term = 0.25 * (1 - p_t) ** 2 * bce
    else:
        term = bce
    if use_ignore:
        norm = max(float(m.sum()), 1e-8) * (R if wrong == "norm" else 1)
        term = (term * m).sum() / norm
    else:
        term = term.mean() * (R if wrong == "norm" else 1)
    return term - dice


def loss_reference(logits, target, table, R, batch_dice, use_ignore, form, weight, grad_scale, wrong=None, world=1):
    """float64 value and grad_scale * weight * d loss / d logits [B, H, W, R] of logits [B, H, W, ld] (the library's layout)."""
    z = logits[..., :R].double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    loss = dc_focal_loss(z, target, table, batch_dice, use_ignore, form, wrong=wrong)
    (grad,) = torch.autograd.grad(loss, z)
    return float(loss.detach()), (grad * (weight * grad_scale)).permute(0, 2, 3, 1)


def loss_bounds(logits, target, table, R, batch_dice, use_ignore, form, weight, grad_scale, dice_logits=None, dice_target=None, world=1):
    """Bounds on |kernel - float64|: (tol_value, e, mag) with the gradient entry off by at most e * mag before its one rounding to fp16 (the caller adds
    2^-11 |d| (1 + e) + 2^-25, the fp16 rounding of dlogits at the chosen grad_scale).  u = 2^-24; every term is formed in fp32:
      e    = exp(-|x|), within E_EXP;  r = 1 / (1 + e): an add and a division, 2 u;  p and 1 - p are r or e r: e_p = E_EXP + 3 u + E_EXP (e's own error
             reaches r damped by e / (1 + e) <= 1): 11 u, no cancellation (1 - p is never formed by subtraction);
      bce  = [max(x, 0) - x y] + log1p(e): the bracket is exact (0, x or -x), log1p within E_EXP of log1p of its argument, whose error E_EXP it passes
             on damped by (e / (1 + e)) / log1p(e) <= 1; a sum of two non-negative terms, one rounding: e_b = 2 E_EXP + u;
      f    = 0.25 q^2 bce (three roundings, the factor 0.25 exact): e_f = 2 e_p + e_b + 3 u;  BCE: e_f = e_b;
      df   = 0.25 q^2 (2 p_t bce + q): the bracket adds non-negative terms, e_p + e_b + 2 u; the product 2 e_p + 3 u more;  BCE: df = p or -(1 - p), e_p;
      sums : non-negative terms through a chain of DICE_CHAIN fp32 adds for the Dice sums (gamma(DICE_CHAIN) + e_p = e_s) and of 16 R + 8 adds for the focal
             sum, into which a thread adds its R regions of 16 pixels (gamma(16 R + 8) + e_f = e_fs); the partials are added in double;
      coefficients (double, one rounding to fp32): coef0 = 2 / (D M) within e_s + u, coef1 = N / (D^2 M) within 3 e_s + u;
      1 / normaliser: one rounding.
    d = gsw (df inv + p (1 - p) (coef1 - y coef0)): |error| <= e mag, mag = gsw (|df| inv + p (1 - p) (coef1 + y coef0)),
    e = (e_df + 2 u) + (2 e_p + 2 u + 3 e_s + 2 u) + 2 u -- the sum of the two terms' relative errors, which bounds either.
    value = focal sum / normaliser - mean dc: e_fs |term| + (2 e_s + 2 u) |mean dc| + u (|term| + |mean dc|) for the rounding of the result.
    `dice_logits` / `dice_target` / `world`: the data-parallel form -- the Dice sums over all ranks' pixels, the gradient's Dice part times `world`."""
    B, H, W, _ = logits.shape
    z = logits[..., :R].double()
    y, ignored = membership(target, table, R)
    y = y.permute(0, 2, 3, 1)
    m = (~ignored).double()[..., None]
    p = torch.sigmoid(z)
    e_p = 2 * E_EXP + 3 * U
    e_b = 2 * E_EXP + U
    e_f = 2 * e_p + e_b + 3 * U if form == "focal" else e_b
    e_df = 3 * e_p + e_b + 5 * U if form == "focal" else e_p
    e_s = ref.gamma(DICE_CHAIN) + e_p
    e_fs = ref.gamma(16 * R + 8) + e_f
    if dice_logits is None:
        dz, dy, dmask = z, y, m
    else:
        dz = dice_logits[..., :R].double()
        dy, dign = membership(dice_target, table, R)
        dy, dmask = dy.permute(0, 2, 3, 1), (~dign).double()[..., None]
    dp = torch.sigmoid(dz)
    dims = (0, 1, 2) if batch_dice else (1, 2)
    I, P, G = (dp * dy * dmask).sum(dims, keepdim=True), (dp * dmask).sum(dims, keepdim=True), (dy * dmask).sum(dims, keepdim=True)
    D = (G + P + 1e-5).clamp_min(1e-8)
    N = 2 * I + 1e-5
    M = (1 if batch_dice else dz.shape[0]) * R
    g_abs = world * (N / (D * D * M) + y * 2 / (D * M))
    bce = F.binary_cross_entropy_with_logits(z, y, reduction="none")
    q = y * (1 - p) + (1 - y) * p
    if form == "focal":
        term = 0.25 * q * q * bce
        df = 0.25 * q * q * (2 * (1 - q) * bce + q)
    else:
        term, df = bce, q
    A = float(m.sum())
    inv = (1.0 / A if A else 0.0) if use_ignore else 1.0 / (B * R * H * W)
    gsw = weight * grad_scale
    mag = m * gsw * (df * inv + p * (1 - p) * g_abs)
    e = (e_df + 2 * U) + (2 * e_p + 3 * e_s + 4 * U) + 2 * U
    term_mean = float((term * m).sum()) * inv
    dc = float((N / D).sum() / M)
    tol_value = e_fs * abs(term_mean) + (2 * e_s + 2 * U) * abs(dc) + U * (abs(term_mean) + abs(dc))
    return tol_value, e, mag


def step_gradients(sd, spec, x, targets, weights, table, batch_dice, slope, form="focal", storage16=False, loss_scale=1.0):
    """nnunet_train_ref.step_gradients with the region loss (no ignore label): (loss, {name: d loss / d parameter}) in float64 through the float64 tape of
    the network, or through its fp16-storage model (every stored tensor, forward and backward, rounded to fp16 at `loss_scale`)."""
    leaves = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()}
    outs = ref.forward_deep_supervision(leaves, spec, x.double(), slope, storage16)
    loss = sum(w * dc_focal_loss(o, t, table, batch_dice, False, form) for o, t, w in zip(outs, targets, weights) if w != 0.0)
    names = list(leaves)
    grads = torch.autograd.grad(loss * loss_scale, [leaves[k] for k in names], allow_unused=True)
    return float(loss.detach()), {k: (None if g is None else g / loss_scale) for k, g in zip(names, grads)}


def ignore_blobs(target, ignore, fraction, seed):
    """`target` [B, H, W] with rectangles set to `ignore` until at least `fraction` of the pixels carry it."""
    g = torch.Generator().manual_seed(seed)
    t = target.clone()
    B, H, W = t.shape
    while (t == ignore).double().mean() < fraction:
        b, yy, xx = (int(torch.randint(0, hi, (1,), generator=g)) for hi in (B, H, W))
        t[b, yy:yy + max(2, H // 4), xx:xx + max(2, W // 4)] = ignore
    return t


def region_segmentation(logits, order, threshold):
    """convert_probabilities_to_segmentation's region branch on logits [R, H, W] with the step of sigmoid(.) > 0.5 at `logit > threshold`."""
    seg = torch.zeros(logits.shape[1:], dtype=torch.int16)
    for i, c in enumerate(order):
        seg[logits[i] > threshold] = int(c)
    return seg


def step_of_sigmoid_f16():
    """The largest float16 x with torch.sigmoid(x) > 0.5 false, by enumeration of all finite float16 values (sigmoid taken in float16, as validation does)."""
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16)
    x = bits.view(torch.float16)
    x = x[torch.isfinite(x)]
    x = x[torch.argsort(x.float(), stable=True)]
    above = torch.sigmoid(x) > 0.5
    k = int(above.nonzero()[0])
    assert above[k:].all() and not above[:k].any(), "not a step function"
    return float(x[k - 1])


def step_of_sigmoid_f32():
    """The largest float32 x with torch.sigmoid(x) > 0.5 false, by bisection over the float32 bit patterns of [0, 1] (sigmoid is monotone there)."""
    def above(b):
        return bool(torch.sigmoid(torch.tensor([b], dtype=torch.int32).view(torch.float32)) > 0.5)
    lo, hi = 0, int(torch.tensor([1.0]).view(torch.int32))   # bit patterns of non-negative floats order as the floats do
    assert not above(lo) and above(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if above(mid):
            hi = mid
        else:
            lo = mid
    return float(torch.tensor([lo], dtype=torch.int32).view(torch.float32))
