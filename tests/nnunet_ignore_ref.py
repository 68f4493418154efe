"""Float64 restatement of nnU-Net's Dice + cross-entropy loss with an ignore label (TEST INFRASTRUCTURE ONLY), and the error bound of the library's
ignore form (ldiff_op_dice_ce_ignore), extended from tests/test_gpu_nnunet_train.py's bound of the plain form.

The loss follows the public algorithm of nnunetv2's DC_and_CE_loss(ignore_label=k) (compound_losses.py:31-56) over MemoryEfficientSoftDiceLoss with a
loss mask (dice.py:72-119) and torch's cross_entropy(ignore_index=k): mask = target != k; the three Dice sums run over masked pixels; the cross-entropy
is the sum over masked pixels over their number, and 0 when there is none.  tests/test_cpu_nnunet_ignore.py pins it to values recorded from those
modules (tests/golden/reference_dc_ce_loss_ignore.npz)."""
import torch
import torch.nn.functional as F

import nnunet_train_ref as ref

U = ref.U
DCE_CHAIN = 16 + 6 + 2   # as tests/test_gpu_nnunet_train.py: 16 pixels per thread, a 64-lane butterfly, four waves; the rest is added in double


def dc_ce_loss_ignore(logits, target, batch_dice, ignore, do_bg=False, smooth=1e-5):
    """logits [B, n, H, W] (any float dtype, differentiable), target integer [B, H, W] with values in [0, n) or `ignore` -> CE - mean_c dc_c."""
    B, n = logits.shape[:2]
    target = target.long()
    mask = (target != ignore)
    m = mask.to(logits.dtype)[:, None]
    p = torch.softmax(logits, 1)
    onehot = F.one_hot(torch.where(mask, target, torch.zeros_like(target)), n).permute(0, 3, 1, 2).to(logits.dtype)
    first = 0 if do_bg else 1
    p, onehot = p[:, first:], onehot[:, first:]
    intersect, sum_pred, sum_gt = (p * onehot * m).sum((2, 3)), (p * m).sum((2, 3)), (onehot * m).sum((2, 3))
    if batch_dice:
        intersect, sum_pred, sum_gt = intersect.sum(0), sum_pred.sum(0), sum_gt.sum(0)
    dc = (2 * intersect + smooth) / torch.clip(sum_gt + sum_pred + smooth, 1e-8)
    count = int(mask.sum())
    if count == 0:
        return -dc.mean()
    logp = torch.log_softmax(logits, 1)
    picked = logp.gather(1, torch.where(mask, target, torch.zeros_like(target))[:, None])[:, 0]
    ce = -(picked * mask.to(logits.dtype)).sum() / count
    return ce - dc.mean()


def deep_supervision_loss_ignore(outputs, targets, weights, batch_dice, ignore, **kw):
    return sum(w * dc_ce_loss_ignore(o, t, batch_dice, ignore, **kw) for o, t, w in zip(outputs, targets, weights) if w != 0.0)


def ignore_blobs(target, ignore, fraction, seed):
    """`target` [B, H, W] with rectangles set to `ignore` until at least `fraction` of the pixels carry it."""
    g = torch.Generator().manual_seed(seed)
    t = target.clone()
    B, H, W = t.shape
    while (t == ignore).double().mean() < fraction:
        b, y, x = (int(torch.randint(0, hi, (1,), generator=g)) for hi in (B, H, W))
        t[b, y:y + max(2, H // 4), x:x + max(2, W // 4)] = ignore
    return t


def loss_reference(logits, target, n, batch_dice, ignore, weight, grad_scale, **kw):
    """float64 value and grad_scale * weight * d loss / d logits [B, H, W, n] of logits [B, H, W, ld] (the library's layout)."""
    z = logits[..., :n].double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    loss = dc_ce_loss_ignore(z, target, batch_dice, ignore, **kw)
    (grad,) = torch.autograd.grad(loss, z, allow_unused=True)
    grad = torch.zeros_like(z) if grad is None else grad
    return float(loss.detach()), (grad * (weight * grad_scale)).permute(0, 2, 3, 1)


def loss_bounds(logits, target, n, batch_dice, ignore, weight, grad_scale):
    """Bounds on |kernel - float64| for the value and per gradient entry: test_gpu_nnunet_train.loss_bounds with the mask carried through.
    What the ignore label changes in the derivation, term by term (u = 2^-24, e_p = (2 n + 8) u the error of a softmax value, e_s = gamma(DCE_CHAIN) + e_p
    that of a sum):
      * every sum runs over annotated pixels only: a sum of FEWER non-negative terms through the same chain, so e_s stands, with I, P, G (and so D, N,
        the coefficients and their errors 2 e_s + 2u, e_s + u, 3 e_s + u) formed from the masked sums;
      * B H W becomes the annotated count A, an integer counted exactly (fp32 partial counts of at most 4096, added in double); 1 / A is rounded once
        to fp32 where the plain form rounds 1 / (B H W) once: the same single rounding, already inside gamma(n + 4);
      * an ignored pixel's gradient row is exactly zero: its bound is 0 (mag = 0 there) -- the test asserts equality there, not a tolerance;
      * A = 0: the cross-entropy term is absent, the value is -mean dc alone, whose bound is the Dice part of the plain bound.
    mag = gsw ((p_k + [t = k]) / A + p_k (|g_k| + sum_j p_j |g_j|)) at annotated pixels; the entry is off by at most e mag, e = 3 e_s + 2 e_p + gamma(n + 4),
    then rounded to fp16 once (the caller adds 2^-11 |d| (1 + e) + 2^-25)."""
    B, H, W, _ = logits.shape
    z = logits[..., :n].double()
    p = torch.softmax(z, -1)
    mask = (target != ignore)
    m = mask.double()[..., None]
    onehot = F.one_hot(torch.where(mask, target, torch.zeros_like(target)), n).double() * m
    e_p = (2 * n + 8) * U
    e_s = ref.gamma(DCE_CHAIN) + e_p
    dims = (0, 1, 2) if batch_dice else (1, 2)
    I, P, G = (p * onehot).sum(dims, keepdim=True), (p * m).sum(dims, keepdim=True), onehot.sum(dims, keepdim=True)
    D = (G + P + 1e-5).clamp_min(1e-8)
    N = 2 * I + 1e-5
    M = (1 if batch_dice else B) * (n - 1)
    fg = torch.ones(n, dtype=torch.float64)
    fg[0] = 0
    g_abs = fg * (N / (D * D * M) + onehot * 2 / (D * M))
    gsw = weight * grad_scale
    A = int(mask.sum())
    inv = 1.0 / A if A else 0.0
    mag = m * gsw * ((p + onehot) * inv + p * (g_abs + (p * g_abs).sum(-1, keepdim=True)))
    e = 3 * e_s + 2 * e_p + ref.gamma(n + 4)
    ce = -(torch.log(p) * onehot).sum(-1)
    ce_mean = ce.sum().item() * inv
    dc = (fg * N / D).sum() / M
    tol_value = e_s * abs(ce_mean) + (2 * e_s + 2 * U) * abs(dc.item()) + U * (abs(ce_mean) + abs(dc.item()))
    return tol_value, e, mag
