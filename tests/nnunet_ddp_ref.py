"""Float64 restatement of the data-parallel tissue-head loss (TEST INFRASTRUCTURE ONLY): what rank r of W holds after nnU-Net's
DC_and_CE_loss(ddp=True) under DeepSupervisionWrapper and its backward, BEFORE DistributedDataParallel averages anything.

Rank r, local batch B_r, scale i with weight w_i, batch_dice on:
    value     l_r = sum_i w_i [ CE_sum_r,i / (B_r H W) - mean_c dc_c(S_i) ],   S_i = sum over the ranks (in rank order) of their {intersect, sum_pred, sum_gt}
    gradient  d l_r / d logits_r = w_i [ (p - 1_t) / (B_r H W) + W d(-mean dc(S_i)) / d logits_r ]
The factor W is AllGatherGrad.backward: it all-reduces W identical gradient rows and keeps this rank's.  With batch_dice off nothing is gathered.
tests/test_cpu_nnunet_ddp.py pins this to values recorded from the reference's modules under a two-rank group (tests/golden/reference_dc_ce_loss_ddp.npz);
`variant` states the neighbours the bounds must reject."""
import torch
import torch.nn.functional as F

from nnunet_train_ref import U, U16, SUB16, gamma

VARIANTS = ("rule", "global_mean_ce", "no_world_factor", "local_sums")


def _stats(z, target, n):
    p = torch.softmax(z, 1)
    onehot = F.one_hot(target.long(), n).permute(0, 3, 1, 2).to(z.dtype)
    return (p[:, 1:] * onehot[:, 1:]).sum((2, 3)), p[:, 1:].sum((2, 3)), onehot[:, 1:].sum((2, 3))


def _dice(intersect, sum_pred, sum_gt, smooth):
    return ((2 * intersect + smooth) / torch.clip(sum_gt + sum_pred + smooth, 1e-8)).mean()


def rank_loss(parts_logits, parts_targets, rank, batch_dice, variant="rule", smooth=1e-5):
    """One scale.  parts_logits[q] [B_q, n, H, W] float64, parts_targets[q] integer [B_q, H, W] for every rank q.  Returns (value, gradient with respect to
    parts_logits[rank]) of rank `rank`, unweighted.  variant: "rule" (above); "global_mean_ce": the cross-entropy as the mean over the GLOBAL batch (what one
    process on the concatenated batch has; after the gradient average it weighs every sample alike, the rule weighs every RANK alike);
    "no_world_factor": the Dice gradient without the factor W; "local_sums": the Dice term from this rank's statistics alone."""
    assert variant in VARIANTS
    world = len(parts_logits)
    n = parts_logits[0].shape[1]
    z = parts_logits[rank].detach().clone().requires_grad_(True)
    t = parts_targets[rank]
    Br, _, H, W = z.shape
    G = sum(q.shape[0] for q in parts_logits)
    ce_sum = F.cross_entropy(z, t.long(), reduction="sum")
    if variant == "global_mean_ce":
        with torch.no_grad():
            others = sum(F.cross_entropy(parts_logits[q], parts_targets[q].long(), reduction="sum") for q in range(world) if q != rank)
        ce = (ce_sum + others) / (G * H * W)
        ce_grad_factor = float(world)      # the average over the ranks that follows divides by W
    else:
        ce = ce_sum / (Br * H * W)
        ce_grad_factor = 1.0
    mine = _stats(z, t, n)
    if batch_dice:
        if variant == "local_sums":
            total, factor = [s.sum(0) for s in mine], 1.0
        else:
            total = None
            for q in range(world):   # rank order
                if q == rank:
                    s = [v.sum(0) for v in mine]
                else:
                    with torch.no_grad():
                        s = [v.sum(0) for v in _stats(parts_logits[q], parts_targets[q], n)]
                total = s if total is None else [a + b for a, b in zip(total, s)]
            factor = 1.0 if variant == "no_world_factor" else float(world)
        dice = _dice(*total, smooth)
    else:
        dice, factor = _dice(*mine, smooth), 1.0
    (g_ce,) = torch.autograd.grad(ce, z, retain_graph=True)
    (g_dc,) = torch.autograd.grad(-dice, z)
    return float((ce - dice).detach()), ce_grad_factor * g_ce + factor * g_dc


def rank_deep_supervision(parts_logits, parts_targets, rank, weights, batch_dice, variant="rule"):
    """parts_logits[q][i]: rank q, scale i.  Returns (value, [gradient per scale, None where the weight is 0]) of rank `rank`."""
    value, grads = 0.0, []
    for i, w in enumerate(weights):
        if w == 0.0:
            grads.append(None)
            continue
        v, g = rank_loss([pl[i] for pl in parts_logits], [pt[i] for pt in parts_targets], rank, batch_dice, variant)
        value += w * v
        grads.append(w * g)
    return value, grads


def fixture_bounds(value, g_ref, w, Br, H, W, world):
    """The existing fixture test's bound (tests/test_cpu_nnunet_train.py) with the Dice factor carried: the reference ran in fp32."""
    return 16 * U * max(1.0, abs(value)), 32 * U * world * w / (Br * H * W) + 2.0 ** -20 * g_ref.abs()


def kernel_bounds(parts_logits, parts_targets, rank, n, weight, grad_scale):
    """Bounds on |ldiff_op_dice_ce_stats + _from_sums - float64| for rank `rank`'s value and per entry of its dlogits, batch_dice on, derived as
    test_gpu_nnunet_train.loss_bounds derives the one-call loss's (the same kernels in the same summation orders): every rank's fp32 partial sums carry
    e_s = gamma(DCE_CHAIN) + e_p of themselves, they are sums of non-negative terms and are added in double, so the global sums carry e_s too; the
    coefficients are formed in double from them (x W is exact there); the gradient kernel is unchanged.  What changes against loss_bounds: the sums run
    over all ranks, the Dice magnitude carries the factor W, the cross-entropy count is B_r.
    parts_logits[q] [B_q, H, W, ld] float16 (the kernel's layout), parts_targets[q] [B_q, H, W]."""
    from test_gpu_nnunet_train import DCE_CHAIN
    world = len(parts_logits)
    Br, H, W, _ = parts_logits[rank].shape
    e_p = (2 * n + 8) * U
    e_s = gamma(DCE_CHAIN) + e_p
    I = P = G = 0.0
    for q in range(world):
        pq = torch.softmax(parts_logits[q][..., :n].double(), -1)
        oq = F.one_hot(parts_targets[q].long(), n).double()
        I, P, G = I + (pq * oq).sum((0, 1, 2)), P + pq.sum((0, 1, 2)), G + oq.sum((0, 1, 2))
        if q == rank:
            p, onehot = pq, oq
    D = (G + P + 1e-5).clamp_min(1e-8)
    N = 2 * I + 1e-5
    M = n - 1
    fg = torch.ones(n, dtype=torch.float64)
    fg[0] = 0
    g_abs = fg * (N / (D * D * M) + onehot * 2 / (D * M))
    gsw = weight * grad_scale
    mag = gsw * ((p + onehot) / (Br * H * W) + world * p * (g_abs + (p * g_abs).sum(-1, keepdim=True)))
    e = 3 * e_s + 2 * e_p + gamma(n + 4)
    ce = -(torch.log(p) * onehot).sum(-1)
    dc = (fg * N / D).sum() / M
    tol_value = e_s * ce.abs().mean().item() + (2 * e_s + 2 * U) * abs(dc.item()) + U * (ce.mean().item() + abs(dc.item()))

    def tol_of(gref):
        return e * mag + U16 * gref.abs() * (1 + e) + SUB16

    return tol_value, tol_of
