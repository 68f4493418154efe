"""GPU (-m gpu): the training step of the nnU-Net tissue head on the HIP library (ldiffusion_amd/nnunet_train.py; csrc/kernels_segtrain.hip) -- its three
kernels alone against float64 with derived bounds (tests/nnunet_train_ref.py states them), the whole backward pass against the float64 tape with the
fp16-storage model as the yardstick, a short training run, and the round trip through a trained-model folder.

u = 2^-24, gamma(n) = 2 n u as in tests/test_gpu_nnunet.py.

Where the kernels' loops wrap (IN_LANE_SHAPES, IN_WRAP_SHAPES, LOSS_WRAP_NB; tests/test_cpu_nnunet_train.py pins the thresholds), measured on an MI355X as the worst
error / bound over the group's cases: IN_LANE_SHAPES y 0.983, dx 0.975, dgamma 0.006, dbeta 0.016; IN_WRAP_SHAPES y 0.987, dx 0.982, dgamma 0.001, dbeta 0.002, saved
mean 0.012, saved rstd 0.013 (the existing IN_SHAPES in the same run: 0.985, 0.973, 0.008, 0.018); LOSS_WRAP_NB value 0.012, gradient 0.966 (the fp16 rounding
of the stored gradient alone takes 0.96 of that bound).  With both finalizes cut to their first pass over the partials exactly the wrap cases fail."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nnunet_train_ref as ref
from ldiffusion_amd import _lib, autograd as ag, nnunet, nnunet_train, train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
U, U16, SUB16 = ref.U, ref.U16, ref.SUB16


def fixtures():
    with open(os.path.join(GOLDEN, "nnunet_plans_2d.json")) as f:
        plans = json.load(f)
    with open(os.path.join(GOLDEN, "nnunet_dataset.json")) as f:
        ds = json.load(f)
    return plans, ds


def sp():
    return _lib.stream_ptr()


# ---- 1. InstanceNorm + LeakyReLU -------------------------------------------------------------------------------------------------------------------
def run_in_train(lib, x, dy, gm, bt, eps, slope):
    """x, dy [B, HW, C] fp16 on the host -> (y, mean, rstd, dx, dgamma, dbeta) float64 on the host, straight through the C entry points."""
    B, HW, C = x.shape
    xd, dyd, gd, bd = x.to(DEV), dy.to(DEV), gm.float().to(DEV), bt.float().to(DEV)
    y, dx = torch.full_like(xd, float("nan")), torch.full_like(xd, float("nan"))
    mean, rstd = torch.full((B, C), float("nan"), device=DEV), torch.full((B, C), float("nan"), device=DEV)
    dg, db = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
    nb = lib.ldiff_op_in_train_ws_bytes(B, HW, C)
    assert nb > 0
    ws = torch.empty(nb // 4 + 4, dtype=torch.float32, device=DEV)
    _lib.check(lib.ldiff_op_in_train_fwd(_lib.ptr(xd), _lib.ptr(y), _lib.ptr(gd), _lib.ptr(bd), _lib.ptr(mean), _lib.ptr(rstd), B, HW, C, eps, slope, _lib.ptr(ws), nb, sp()))
    _lib.check(lib.ldiff_op_in_train_bwd(_lib.ptr(xd), _lib.ptr(dyd), _lib.ptr(gd), _lib.ptr(bd), _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(dx), _lib.ptr(dg), _lib.ptr(db),
                                         B, HW, C, slope, _lib.ptr(ws), nb, sp()))
    torch.cuda.synchronize()
    return tuple(t.double().cpu() for t in (y, mean, rstd, dx, dg, db))


IN_SHAPES = [(2, 32, 4, 4), (1, 16, 24, 40), (2, 64, 64, 64), (3, 256, 8, 8), (2, 512, 2, 2), (2, 512, 8, 8)]   # the last two: the bottleneck norms of the `2d` plan


# Thread layouts no shape above reaches (ref.in_layout): C / 8 = 3, 5, 12 does not divide 256, so 256 - nrl G = 1, 1, 4 threads of a workgroup idle and a
# row lane's first thread is no multiple of a wave's width -- with 63 rows (fewer than the 85 row lanes), with two slabs an image, with 51 and with 21 row
# lanes; C / 8 = 257 takes a second pass over the channel vectors with a single live thread.
IN_LANE_SHAPES = [(2, 24, 7, 9), (2, 24, 40, 70), (3, 40, 33, 50), (2, 96, 30, 30), (2, 2056, 9, 9)]
# More than 64 slabs an image, where the finalize kernels' `r += 64` loops take a second and a third pass: R = 72; R = 72 with a last slab of 127 rows; R = 131.
# R > 64 needs HW C > 64 * 65536 elements an image whatever C is, so these are the smallest such shapes.  One slope: the float64 side takes seconds.
IN_WRAP_SHAPES = [(1, 512, 96, 96), (2, 512, 97, 95), (1, 512, 129, 129)]
IN_CASES = [s + (slope,) for slope in (0.01, 1.0) for s in IN_SHAPES + IN_LANE_SHAPES] + [s + (0.01,) for s in IN_WRAP_SHAPES]


@pytest.mark.parametrize("B,C,H,W,slope", IN_CASES)
def test_instance_norm_lrelu_against_float64(lib, B, C, H, W, slope):
    """Forward and backward on the same fp16 inputs against float64, per element, with nnunet_train_ref.in_lrelu_bounds (derived there from the kernel's
    summation order).  Inputs of unit scale with a per-channel offset, as a conv's output is.  Elements whose float64 pre-activation is smaller than
    the fp32 evaluation error of that value may take either branch (at most 0.5 % of them).  The same bounds must reject a reference with slope 0 and
    one whose statistics run over the batch (where the batch has more than one image: with one they are the same function) and, where an image has
    more than 64 slabs, one whose sums stop after the first 64 (nnunet_train_ref.in_lrelu_first_pass_reference: mean, rstd, dgamma, dbeta)."""
    HW = H * W
    g = torch.Generator().manual_seed(B * 1000 + C + HW)
    x = (torch.randn((B, HW, C), generator=g) * (0.5 + torch.rand((1, 1, C), generator=g)) + 0.5 * torch.randn((B, 1, C), generator=g)).to(torch.float16)
    dy = (torch.randn((B, HW, C), generator=g) * 0.1).to(torch.float16)
    gm, bt = (1.0 + 0.2 * torch.randn(C, generator=g)).float(), (0.3 * torch.randn(C, generator=g)).float()
    eps = 1e-5
    y, mean, rstd, dx, dg, db = run_in_train(lib, x, dy, gm, bt, eps, slope)
    x64, dy64, gm64, bt64 = x.double(), dy.double(), gm.double(), bt.double()
    want, tol = ref.in_lrelu_bounds(x64, dy64, gm64, bt64, eps, slope)
    amb = tol["ambiguous"]
    share = amb.double().mean().item()
    # saved statistics
    gs, gq = ref.gamma(ref.IN_ROWS + 2), ref.gamma(ref.IN_ROWS + 3)
    mu, var = want["mu"][:, 0], want["var"][:, 0]
    assert ((mean - mu).abs() <= gs * x64.abs().mean(1) + U * mu.abs()).all()
    e_r = 1.5 * gq * (x64 * x64).mean(1) / (var + eps) + U
    assert ((rstd * torch.sqrt(var + eps) - 1).abs() <= e_r).all()

    def errors(w):
        """element errors of y and dx against reference `w`; an ambiguous element is measured against the nearer branch"""
        a, xh, r = w["a"], w["xh"], w["r"]
        s_alt = torch.where(a > 0, torch.full_like(a, slope), torch.ones_like(a))
        y_alt = a * s_alt
        dx_alt = r * gm64 * (dy64 * s_alt - w["m1"] - xh * w["m2"])
        ey = torch.where(amb, torch.minimum((y - w["y"]).abs(), (y - y_alt).abs()), (y - w["y"]).abs())
        edx = torch.where(amb, torch.minimum((dx - w["dx"]).abs(), (dx - dx_alt).abs()), (dx - w["dx"]).abs())
        return ey, edx

    ey, edx = errors(want)
    print(f"[in_train] B={B} C={C} {H}x{W} slope={slope}: y {(ey / tol['y']).max():.3f} dx {(edx / tol['dx']).max():.3f} dgamma {((dg - want['dgamma']).abs() / tol['dgamma']).max():.3f} "
          f"dbeta {((db - want['dbeta']).abs() / tol['dbeta']).max():.3f} of the bound; {share:.2e} of the elements may take either branch")
    assert share <= 0.005
    assert (ey <= tol["y"]).all() and (edx <= tol["dx"]).all()
    assert ((dg - want["dgamma"]).abs() <= tol["dgamma"]).all() and ((db - want["dbeta"]).abs() <= tol["dbeta"]).all()
    wrong = [("slope 0", ref.in_lrelu_reference(x64, dy64, gm64, bt64, eps, 0.0))]
    if B > 1:
        wrong.append(("batch statistics", ref.in_lrelu_reference(x64, dy64, gm64, bt64, eps, slope, batch_stats=True)))
    for what, w in wrong:
        wy, wdx = errors(w)
        assert (wy > tol["y"]).double().mean() > 0.2, f"the forward bound accepts {what}"
        assert (wdx > tol["dx"]).double().mean() > 0.2, f"the backward bound accepts {what}"
        assert ((dg - w["dgamma"]).abs() > tol["dgamma"]).double().mean() > 0.2, f"the dgamma bound accepts {what}"
        if not (slope == 1.0 and what == "batch statistics"):   # at slope 1 dbeta = sum dy whatever the statistics are: the same function, nothing to reject
            assert ((db - w["dbeta"]).abs() > tol["dbeta"]).double().mean() > 0.2, f"the dbeta bound accepts {what}"
    lay = ref.in_layout(HW, C)
    if lay["R"] > 64:   # a finalize that stopped after its first pass over the slabs: the sums of the first 64 S pixels of an image
        w = ref.in_lrelu_first_pass_reference(x64, dy64, gm64, bt64, eps, slope, 64 * lay["S"])
        what = f"sums over the first 64 of {lay['R']} slabs"
        print(f"[in_train] B={B} C={C} {H}x{W}: {lay['R']} slabs an image: mean {((mean - mu).abs() / (gs * x64.abs().mean(1) + U * mu.abs())).max():.3f} "
              f"rstd {((rstd * torch.sqrt(var + eps) - 1).abs() / e_r).max():.3f} of the bound")
        assert ((mean - w["mu"][:, 0]).abs() > gs * x64.abs().mean(1) + U * mu.abs()).double().mean() > 0.2, f"the bound on the saved mean accepts {what}"
        assert ((rstd * torch.sqrt(w["var"][:, 0] + eps) - 1).abs() > e_r).double().mean() > 0.2, f"the bound on the saved rstd accepts {what}"
        assert ((dg - w["dgamma"]).abs() > tol["dgamma"]).double().mean() > 0.2, f"the dgamma bound accepts {what}"
        assert ((db - w["dbeta"]).abs() > tol["dbeta"]).double().mean() > 0.2, f"the dbeta bound accepts {what}"


def test_instance_norm_lrelu_function_and_refusals(lib):
    """The autograd.Function hands the same numbers to torch's tape, and the entry points refuse what they do not cover."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn((2, 6, 10, 24), generator=g).to(torch.float16).to(DEV).requires_grad_(True)
    gm, bt = torch.nn.Parameter((1 + 0.1 * torch.randn(24, generator=g)).to(DEV)), torch.nn.Parameter((0.1 * torch.randn(24, generator=g)).to(DEV))
    dy = torch.randn((2, 6, 10, 24), generator=g).to(torch.float16).to(DEV)
    y = ag.InstanceNormLReLUFn.apply(x, gm, bt, 1e-5, 0.01)
    y.backward(dy)
    got = run_in_train(lib, x.detach().cpu().reshape(2, 60, 24), dy.cpu().reshape(2, 60, 24), gm.detach().cpu(), bt.detach().cpu(), 1e-5, 0.01)
    assert torch.equal(y.detach().double().cpu().reshape(2, 60, 24), got[0]) and torch.equal(x.grad.double().cpu().reshape(2, 60, 24), got[3])
    assert torch.equal(gm.grad.double().cpu(), got[4]) and torch.equal(bt.grad.double().cpu(), got[5])
    assert lib.ldiff_op_in_train_ws_bytes(1, 16, 12) == 0
    ws = torch.empty(64, device=DEV)
    t = torch.zeros(16 * 12, dtype=torch.float16, device=DEV)
    f = torch.zeros(16, device=DEV)
    with pytest.raises(ValueError, match="multiple of 8"):
        _lib.check(lib.ldiff_op_in_train_fwd(_lib.ptr(t), _lib.ptr(t), _lib.ptr(f), _lib.ptr(f), _lib.ptr(f), _lib.ptr(f), 1, 16, 12, 1e-5, 0.01, _lib.ptr(ws), 256, sp()))
    with pytest.raises(ValueError, match="workspace"):
        _lib.check(lib.ldiff_op_in_train_fwd(_lib.ptr(t), _lib.ptr(t), _lib.ptr(f), _lib.ptr(f), _lib.ptr(f), _lib.ptr(f), 1, 16, 8, 1e-5, 0.01, _lib.ptr(ws), 8, sp()))


# ---- 2. the loss -----------------------------------------------------------------------------------------------------------------------------------
DCE_CHAIN = 16 + 6 + 2   # csrc/kernels_segtrain.hip: 4096 pixels per workgroup = 16 per thread, a 64-lane butterfly, four waves; the rest is added in double


def loss_case(n, B, H, W, absent, seed):
    g = torch.Generator().manual_seed(seed)
    ld = (n + 7) // 8 * 8
    logits = torch.zeros((B, H, W, ld), dtype=torch.float16)
    logits[..., :n] = (2.0 * torch.randn((B, H, W, n), generator=g)).to(torch.float16)
    logits[..., n:] = 7.0     # the pad columns take no part, whatever they hold
    target = torch.randint(0, n, (B, H, W), generator=g)
    if absent:
        target[target == n - 1] = 0
    return logits, target


def run_dice_ce(logits, target, n, batch_dice, weight, grad_scale):
    loss, dl = ag.dice_ce(logits.to(DEV), target.to(DEV), n, batch_dice, weight, grad_scale)
    torch.cuda.synchronize()
    return loss.cpu(), dl.cpu()


def loss_reference(logits, target, n, batch_dice, weight, grad_scale, **kw):
    """float64 value and grad_scale * weight * d loss / d logits [B, H, W, n], with the magnitude sums the bound uses."""
    z = logits[..., :n].double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    loss = ref.dc_ce_loss(z, target, batch_dice, **kw)
    (grad,) = torch.autograd.grad(loss, z)
    return float(loss.detach()), (grad * (weight * grad_scale)).permute(0, 2, 3, 1)


def loss_bounds(logits, target, n, batch_dice, weight, grad_scale):
    """Bounds on |kernel - float64| for the value and per gradient entry.
    fp32 evaluation: softmax values carry e_p = (2 n + 8) u (exp to 1 ulp, a sum of n terms, a reciprocal and a product); each of the three sums per
    class carries e_s = gamma(DCE_CHAIN) + e_p of itself (they are sums of non-negative terms); dc = N / D carries 2 e_s + 2u, the gradient factors
    2 / (D M) and N / (D^2 M) carry e_s + u and 3 e_s + u.  With g_k = coef1_k - coef0_k [t = k] and mag = gsw ((p_k + [t = k]) / (B H W) + p_k (|g_k| + sum_j p_j |g_j|))
    the entry is off by at most e mag, e = 3 e_s + 2 e_p + gamma(n + 4), in fp32, then rounded to fp16 once: 2^-11 |d| (1 + e) + 2^-25 (the subnormal floor).
    Value: the cross-entropy mean carries e_s of mean |ce|, the Dice mean 2 e_s + 2u of mean dc, the difference one rounding."""
    B, H, W, _ = logits.shape
    z = logits[..., :n].double()
    p = torch.softmax(z, -1)
    onehot = F.one_hot(target, n).double()
    e_p = (2 * n + 8) * U
    e_s = ref.gamma(DCE_CHAIN) + e_p
    dims = (0, 1, 2) if batch_dice else (1, 2)
    I, P, G = (p * onehot).sum(dims, keepdim=True), p.sum(dims, keepdim=True), onehot.sum(dims, keepdim=True)
    D = (G + P + 1e-5).clamp_min(1e-8)
    N = 2 * I + 1e-5
    M = (1 if batch_dice else B) * (n - 1)
    fg = torch.ones(n, dtype=torch.float64)
    fg[0] = 0
    g_abs = fg * (N / (D * D * M) + onehot * 2 / (D * M))
    gsw = weight * grad_scale
    mag = gsw * ((p + onehot) / (B * H * W) + p * (g_abs + (p * g_abs).sum(-1, keepdim=True)))
    e = 3 * e_s + 2 * e_p + ref.gamma(n + 4)
    ce = -(torch.log(p) * onehot).sum(-1)
    dc = (fg * N / D).sum() / M
    tol_value = e_s * ce.abs().mean().item() + (2 * e_s + 2 * U) * abs(dc.item()) + U * (ce.mean().item() + abs(dc.item()))
    return tol_value, e, mag


LOSS_CASES = [(n, shape, bd, i64, gs, absent) for n in (4, 7, 11) for shape in ((2, 4, 4), (1, 24, 40), (2, 64, 64)) for bd in (True, False)
              for i64 in (False, True) for gs in (1.0, 65536.0) for absent in (False, True)]
# row pitches 24 and 32, the kernels' NV = 3 and NV = 4 instantiations: one full chunk of DCE_PIX pixels plus a ragged one, and fewer pixels than a
# workgroup has threads; at the loss scale that keeps the gradient's entries in fp16's normal range, where the bound is a relative one
LOSS_CASES += [(n, (2,) + hw, bd, True, 65536.0, False) for n in (17, 32) for hw in ((72, 64), (15, 13)) for bd in (True, False)]
# Batches at which the one-workgroup finalize covers its tables in several passes of 256 threads once batch_dice is off: B NACC = 286 / 814 / 882 slots
# of sums (dce_reduce_sums), B NC = 88 / 264 / 288 coefficients (dce_coef_loss): the first wraps the sums alone, the others both.  batch_dice on has one
# row whatever B is: the control.  tests/test_cpu_nnunet_train.py pins the two thresholds to these cases.
LOSS_WRAP_NB = [(4, 11), (17, 11), (32, 9)]
LOSS_CASES += [(n, (B,) + hw, bd, True, 65536.0, False) for n, B in LOSS_WRAP_NB for hw in ((15, 13), (72, 64)) for bd in (False, True)]


def first_pass_reference(logits, target, n, batch_dice, weight, grad_scale, keep):
    """loss_reference for ref.first_pass_dice_loss: the Dice term of samples < keep alone (WRONG: the bounds must reject it)."""
    z = logits[..., :n].double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    loss = ref.first_pass_dice_loss(z, target, keep, lambda a, t: ref.dc_ce_loss(a, t, batch_dice), F.cross_entropy)
    (grad,) = torch.autograd.grad(loss, z)
    return float(loss.detach()), (grad * (weight * grad_scale)).permute(0, 2, 3, 1)


@pytest.mark.parametrize("i,n,shape,batch_dice,i64,grad_scale,absent", [(i,) + c for i, c in enumerate(LOSS_CASES)])
def test_dice_ce_against_float64(lib, i, n, shape, batch_dice, i64, grad_scale, absent):
    """Value and dlogits of ldiff_op_dice_ce against the float64 restatement (pinned to the reference's modules by tests/test_cpu_nnunet_train.py), over the
    full product of: n_heads 4 / 7 / 11 (row pitch 8 / 8 / 16); fewer pixels than a workgroup's share, an odd size, two workgroups per image; batch_dice
    on / off; uint8 / int64 labels; loss scale 1 / 65536; every class present / a foreground class absent from the target; and n_heads 17 / 32 (row pitch
    24 / 32) at two sizes with both batch_dice values.  Pad columns exactly zero; two
    launches bit-identical; the bound rejects do_bg = True, smooth = 1 and, for a batch of more than one image, the flipped batch_dice (by the value or by
    an entry of the gradient).  LOSS_WRAP_NB: n_heads 4 / 17 / 32 at batches of 11 / 11 / 9 and two sizes, where the finalize's loops over [sample][slot]
    wrap with batch_dice off; there the bounds also reject, by the value and by the gradient, a Dice term that leaves out the samples of the later passes."""
    B, H, W = shape
    weight = 4 / 7
    logits, target = loss_case(n, B, H, W, absent, 300 + i)
    tgt = target if i64 else target.to(torch.uint8)
    loss, dl = run_dice_ce(logits, tgt, n, batch_dice, weight, grad_scale)
    loss2, dl2 = run_dice_ce(logits, tgt, n, batch_dice, weight, grad_scale)
    assert torch.equal(loss, loss2) and torch.equal(dl, dl2), "two launches on the same inputs differ"
    assert dl.dtype == torch.float16 and dl.shape == logits.shape and not dl[..., n:].any(), "pad columns must be exactly zero"
    want, gwant = loss_reference(logits, target, n, batch_dice, weight, grad_scale)
    tol_value, e, mag = loss_bounds(logits, target, n, batch_dice, weight, grad_scale)
    got = dl[..., :n].double()

    def tol_of(gref):
        return e * mag + U16 * gref.abs() * (1 + e) + SUB16

    err = (got - gwant).abs()
    print(f"[dice_ce] n={n} {shape} batch_dice={batch_dice} scale={grad_scale:g}: value off by {abs(float(loss) - want):.2e} (bound {tol_value:.2e}), gradient at "
          f"{(err / tol_of(gwant)).max():.3f} of its bound, |g| up to {gwant.abs().max():.2e}")
    assert abs(float(loss) - want) <= tol_value
    assert (err <= tol_of(gwant)).all()
    wrong = [("do_bg", dict(do_bg=True), batch_dice), ("smooth = 1", dict(smooth=1.0), batch_dice)] + ([("flipped batch_dice", {}, not batch_dice)] if B > 1 else [])
    for what, kw, bd in wrong:
        w, gw = loss_reference(logits, target, n, bd, weight, grad_scale, **kw)
        assert abs(float(loss) - w) > tol_value or ((got - gw).abs() > tol_of(gw)).any(), f"the bounds accept {what}"
    keep = 256 // ag.dice_ce_nacc(n)   # the samples whose every slot of the sums table lies in the finalize's first pass
    if keep < B:
        w, gw = first_pass_reference(logits, target, n, batch_dice, weight, grad_scale, keep)
        assert abs(float(loss) - w) > tol_value, f"the value's bound accepts a Dice term of the first {keep} samples of {B}"
        assert ((got - gw).abs() > tol_of(gw)).any(), f"the gradient's bound accepts a Dice term of the first {keep} samples of {B}"


@pytest.mark.parametrize("n,B,ignore", [(32, 9, None), (17, 11, 17)], ids=["plain", "ignore"])
def test_dice_ce_stays_inside_its_workspace(lib, n, B, ignore):
    """One case per form straight through the C entry with batch_dice off, where `sums`, `dcs` and `coef` scale with B: a workspace of exactly ws_bytes with
    64 NaN floats behind it.  The canaries stay NaN, and loss and dlogits are the wrapper's bits (whose workspace is the same size, sized by the same call)."""
    H, W = 72, 64
    logits, target = loss_case(n, B, H, W, False, 40 + n)
    if ignore is not None:
        target[:, 10:30, 5:40] = ignore
    weight, scale = 4 / 7, 65536.0
    want_loss, want_dl = ag.dice_ce(logits.to(DEV), target.to(DEV), n, False, weight, scale, ignore_label=ignore)
    ld, td = logits.to(DEV), target.to(DEV)
    nb = (lib.ldiff_op_dice_ce_ws_bytes if ignore is None else lib.ldiff_op_dice_ce_ignore_ws_bytes)(B, H * W, n)
    assert nb > 0 and nb % 4 == 0
    ws = torch.full((nb // 4 + 64,), float("nan"), dtype=torch.float32, device=DEV)
    loss, dl = torch.full((1,), float("nan"), device=DEV), torch.full_like(ld, float("nan"))
    head = (_lib.ptr(ld), ld.shape[-1], n) + (() if ignore is None else (ignore,))
    entry = lib.ldiff_op_dice_ce if ignore is None else lib.ldiff_op_dice_ce_ignore
    _lib.check(entry(*head, _lib.ptr(td), 1, B, H * W, 0, 1e-5, weight, scale, _lib.ptr(loss), _lib.ptr(dl), _lib.ptr(ws), nb, sp()))
    torch.cuda.synchronize()
    assert ws[nb // 4:].isnan().all(), "the entry wrote behind ws_bytes"
    assert torch.equal(loss[0], want_loss) and torch.equal(dl, want_dl) and math.isfinite(float(loss))


def test_dice_ce_refusals_and_bad_labels(lib):
    logits, target = loss_case(4, 1, 4, 4, False, 1)
    with pytest.raises(ValueError, match="heads"):
        ag.dice_ce(logits.to(DEV), target.to(DEV), 1, True)
    with pytest.raises(ValueError, match="pitch"):
        ag.dice_ce(logits.to(DEV), target.to(DEV), 11, True)
    target[0, 0, 0] = 9
    loss, dl = ag.dice_ce(logits.to(DEV), target.to(DEV), 4, True)
    assert math.isnan(float(loss)), "a label outside [0, n_heads) must not pass silently"
    assert dl[0, 0, 0, :4].isnan().all() and not dl[0, 0, 0, 4:].any(), "and its gradient is poisoned, so that the step's overflow test skips the update"


def test_dice_ce_function_scales_with_the_incoming_gradient(lib):
    """DiceCeFn returns the weighted term and its backward multiplies the stored (weighted, scaled) gradient by the incoming one: loss.backward() hands out the
    stored tensor bit for bit, (0.5 * loss).backward() half of it."""
    logits, target = loss_case(7, 2, 24, 40, False, 3)
    w, gs = 4 / 7, 1024.0
    plain, stored = ag.dice_ce(logits.to(DEV), target.to(DEV), 7, True, w, gs)
    for factor in (1.0, 0.5):
        z = logits.to(DEV).requires_grad_(True)
        term = ag.DiceCeFn.apply(z, target.to(DEV), 7, True, w, gs, 1e-5)
        assert torch.equal(term, plain * w)
        (factor * term).backward()
        assert z.grad.dtype == torch.float16 and torch.equal(z.grad, (stored.float() * factor).to(torch.float16))


# ---- 3. SGD ----------------------------------------------------------------------------------------------------------------------------------------
def test_sgd_nesterov_against_torch_float64(lib):
    """Three steps of ag.sgd_nesterov_step against torch.optim.SGD(momentum 0.99, nesterov, weight decay) in float64 from the same fp32 start: tensors of 1, 7
    and 4099 elements and one of a chunk and five (two workgroups), a tensor without gradient (untouched, as in torch), inv_scale and clip_coef device scalars.
    Bound, per element and step, from the update rule's operations (each rounds once, u = 2^-24; a contraction to fma only removes roundings):
    lr, wd and m themselves are rounded to fp32 when they are passed):
        g = sc grad + wd p:        |dg| <= 4u (|sc grad| + |wd p|) + wd |dp'|           (sc = inv_scale clip_coef: one rounding, then the product; wd, wd p; the sum)
        buf = m buf' + g:          |dbuf| <= m |dbuf'| + |dg| + 3u (|m buf'| + |g|)      (m, m buf', the sum; the first step sets buf = g)
        p -= lr (g + m buf):       |dp| <= |dp'| + lr (|dg| + m |dbuf|) + 5u lr (|g| + |m buf|) + u |p|   (m, m buf, the sum, lr, the product; the difference)"""
    lr, wd, mom = 1e-2, 3e-5, 0.99
    inv_scale, clip = torch.tensor([1.0 / 1000.0], dtype=torch.float32), torch.tensor([0.37], dtype=torch.float32)
    sc = float(inv_scale.double() * clip.double())
    g = torch.Generator().manual_seed(11)
    sizes = [1, 7, 4099, ag.ADAMW_CHUNK + 5, 9]
    start = [torch.randn(n, generator=g) for n in sizes]
    params = [t.clone().to(DEV) for t in start]
    ref_p = [torch.nn.Parameter(t.double().clone()) for t in start]
    opt = torch.optim.SGD(ref_p, lr, momentum=mom, nesterov=True, weight_decay=wd)
    state = {}
    dp = [torch.zeros(n, dtype=torch.float64) for n in sizes]
    dbuf = [torch.zeros(n, dtype=torch.float64) for n in sizes]
    inv_d, clip_d = inv_scale.to(DEV), clip.to(DEV)
    for step in range(3):
        grads = [torch.randn(n, generator=g) * 1000.0 for n in sizes]
        grads[-1] = None
        prev = [p.detach().clone() for p in ref_p]
        prev_buf = [opt.state[p]["momentum_buffer"].clone() if step and "momentum_buffer" in opt.state[p] else torch.zeros_like(p) for p in ref_p]
        for p, gr in zip(ref_p, grads):
            p.grad = None if gr is None else gr.double() * sc
        opt.step()
        ag.sgd_nesterov_step(params, [None if gr is None else gr.to(DEV) for gr in grads], state, lr, wd, mom, inv_d, clip_d)
        torch.cuda.synchronize()
        for k, (p, gr) in enumerate(zip(ref_p, grads)):
            got = params[k].double().cpu()
            if gr is None:
                assert torch.equal(got, start[k].double()), "a tensor without gradient must stay untouched"
                continue
            g64 = gr.double() * sc + wd * prev[k]
            buf = opt.state[p]["momentum_buffer"]
            mb = mom * prev_buf[k] if step else torch.zeros_like(g64)
            dg = 4 * U * ((gr.double() * sc).abs() + (wd * prev[k]).abs()) + wd * dp[k]
            dbuf[k] = (mom * dbuf[k] + 3 * U * (mb.abs() + g64.abs()) if step else 0) + dg
            dp[k] = dp[k] + lr * (dg + mom * dbuf[k]) + 5 * U * lr * (g64.abs() + (mom * buf).abs()) + U * p.detach().abs()
            err = (got - p.detach()).abs()
            assert (err <= dp[k]).all(), f"step {step}, tensor of {sizes[k]}: {(err / dp[k]).max():.2f} of the bound"
            gbuf = state["momentum_buffer"][k].double().cpu()
            assert ((gbuf - buf).abs() <= dbuf[k]).all()
            assert ((got - p.detach()).abs().max() < 1e-3 * (prev[k] - p.detach()).abs().max()), "the bound is far below the size of a step"
    # the bound tells the rule from its neighbours: plain momentum (no Nesterov look-ahead) lands elsewhere
    plain = [torch.nn.Parameter(t.double().clone()) for t in start]
    o2 = torch.optim.SGD(plain, lr, momentum=mom, nesterov=False, weight_decay=wd)
    g = torch.Generator().manual_seed(11)
    [torch.randn(n, generator=g) for n in sizes]
    for step in range(3):
        grads = [torch.randn(n, generator=g) * 1000.0 for n in sizes]
        for p, gr in zip(plain[:-1], grads):
            p.grad = gr.double() * sc
        o2.step()
    assert ((params[2].double().cpu() - plain[2].detach()).abs() > dp[2]).double().mean() > 0.5


# ---- 4. the whole step against the float64 tape ---------------------------------------------------------------------------------------------------
M_CAP = 2.0
LOSS_SCALE = 1024.0
STEP_CASES = [("2d_reduced", 2, 64, 41), ("2d_reduced", 2, 32, 42)]
# Measured on the MI355X (see DESIGN.md section 7 for the date and commit), per case and slope: (worst ratio over the graded parameter tensors of the library's
# figure to the fp16-storage model's, worst ratio of the absolute errors over the conv.bias tensors).  Slope 1.0: figure = max |g - g64| / max |g64|;
# slope 0.01: figure = ||g - g64|| / ||g64||.  Asserted factor: twice the measured ratio, at most M_CAP.
MEASURED_ROUND_TRIP = 0.710   # |inference head - Trainer.eval_logits| / (fp16-storage model's error of the float64 logits): 1.335e-2 / 1.880e-2, same run
MEASURED = {("2d_reduced", 2, 64, 41, 1.0): (1.654, 1.393), ("2d_reduced", 2, 32, 42, 1.0): (1.948, 1.256),
            ("2d_reduced", 2, 64, 41, 0.01): (1.434, 1.684), ("2d_reduced", 2, 32, 42, 0.01): (1.407, 1.550)}
_steps = {}


def step_case(config, B, size, seed, slope):
    key = (config, B, size, seed, slope)
    if key not in _steps:
        plans, ds = fixtures()
        spec = nnunet.network_spec(plans, config, ds)
        sd = ref.synthetic_state_dict(spec, seed)
        g = torch.Generator().manual_seed(seed + 100)
        x = F.avg_pool2d(torch.randn((B, 3, size + 4, size + 4), generator=g), 5, 1) * 2.2    # as test_gpu_nnunet.network_case builds its input
        n_out = spec["n_stages"] - 1
        targets = ref.label_maps(B, spec["n_heads"], size, n_out, seed + 200)
        assert all(len(t.unique()) == spec["n_heads"] for t in targets[:-1])
        weights = nnunet_train.deep_supervision_weights(n_out)
        batch_dice = bool(plans["configurations"]["2d"]["batch_dice"])
        tr = nnunet_train.Trainer(spec, sd, batch_dice, 10, device=DEV, slope=slope)
        outs = tr.network(x)
        total = tr.loss(outs, [t.to(DEV) for t in targets], LOSS_SCALE)
        total.backward()
        torch.cuda.synchronize()
        lib_g = {k: (None if p.grad is None else p.grad.double().cpu() / LOSS_SCALE) for k, p in tr.network.p.items()}
        l64, g64 = ref.step_gradients(sd, spec, x, targets, weights, batch_dice, slope)
        lm, gmod = ref.step_gradients(sd, spec, x, targets, weights, batch_dice, slope, storage16=True, loss_scale=LOSS_SCALE)
        _steps.clear()
        _steps[key] = dict(spec=spec, lib=lib_g, f64=g64, model=gmod, loss=(float(total), l64, lm))
    return _steps[key]


def _step_figures(c, l2):
    rows, bias_rows = [], []
    for k, g64 in c["f64"].items():
        if g64 is None:
            continue
        gl, gm_ = c["lib"][k], c["model"][k]
        if k.endswith(".conv.bias"):
            bias_rows.append((k, (gl - g64).abs().max().item(), (gm_ - g64).abs().max().item()))
        elif l2:
            rows.append((k, ((gl - g64).norm() / g64.norm()).item(), ((gm_ - g64).norm() / g64.norm()).item()))
        else:
            rows.append((k, ((gl - g64).abs().max() / g64.abs().max()).item(), ((gm_ - g64).abs().max() / g64.abs().max()).item()))
    return rows, bias_rows


def _check_step(config, B, size, seed, slope, l2):
    c = step_case(config, B, size, seed, slope)
    # the ungraded head: no gradient at all, in the library as in torch
    assert c["f64"]["decoder.seg_layers.0.weight"] is None and c["lib"]["decoder.seg_layers.0.weight"] is None and c["lib"]["decoder.seg_layers.0.bias"] is None
    assert all((c["lib"][k] is None) == (g is None) for k, g in c["f64"].items())
    lt, l64, lm = c["loss"]
    rows, bias_rows = _step_figures(c, l2)
    worst = max(rows, key=lambda r: r[1] / r[2])
    worst_b = max(bias_rows, key=lambda r: r[1] / r[2])
    print(f"[step] {config} B={B} {size}^2 slope={slope}: loss lib {lt:.6f} f64 {l64:.6f} model {lm:.6f}; worst tensor {worst[0]}: lib {worst[1]:.3e} model {worst[2]:.3e} "
          f"ratio {worst[1] / worst[2]:.3f}; largest lib figure {max(r[1] for r in rows):.3e}, model {max(r[2] for r in rows):.3e}; conv.bias worst {worst_b[0]}: "
          f"lib {worst_b[1]:.3e} model {worst_b[2]:.3e} ratio {worst_b[1] / worst_b[2]:.3f}")
    m, mb = (min(M_CAP, 2.0 * v) for v in MEASURED[(config, B, size, seed, slope)])
    for k, e_lib, e_model in rows:
        assert e_lib <= m * e_model, f"{k}: library {e_lib:.3e}, fp16-storage model {e_model:.3e}: {e_lib / e_model:.2f} x (asserted {m:.2f} x)"
    for k, e_lib, e_model in bias_rows:
        assert e_lib <= mb * e_model, f"{k}: library {e_lib:.3e} absolute, fp16-storage model {e_model:.3e}: {e_lib / e_model:.2f} x (asserted {mb:.2f} x)"


@pytest.mark.parametrize("config,B,size,seed", STEP_CASES)
def test_whole_step_gradients_slope_one(config, B, size, seed):
    """Every parameter gradient of one step at LeakyReLU slope 1.0, where the gradient is a well-conditioned function of the forward's rounding: per tensor
    max |g - g_f64| / max |g_f64| of the library against the same figure of the fp16-storage model (the float64 tape with every stored tensor, forward and
    backward, rounded to fp16 at the step's loss scale).  The conv biases in front of an InstanceNorm have a mathematically zero gradient: they are compared
    in absolute terms with the model's own values; the ungraded lowest head has no gradient at all."""
    _check_step(config, B, size, seed, 1.0, False)


@pytest.mark.parametrize("config,B,size,seed", STEP_CASES)
def test_whole_step_gradients_slope_001(config, B, size, seed):
    """The same at nnU-Net's slope 0.01, per tensor in relative L2 terms against the fp16-storage model's: a few activations change side of the kink under
    fp16 storage (in the model as in the library), so this catches a wrong mask or a dropped path -- errors of order 1 -- and claims no more."""
    _check_step(config, B, size, seed, 0.01, True)


# ---- 5. training, and the round trip through a trained-model folder -------------------------------------------------------------------------------
def _trainer(seed=7, size=64, B=2, **kw):
    plans, ds = fixtures()
    spec = nnunet.network_spec(plans, "2d_reduced", ds)
    g = torch.Generator().manual_seed(seed)
    x = F.avg_pool2d(torch.randn((B, 3, size + 4, size + 4), generator=g), 5, 1) * 2.2
    targets = ref.label_maps(B, spec["n_heads"], size, spec["n_stages"] - 1, seed + 1)
    tr = nnunet_train.Trainer(spec, nnunet_train.initial_state_dict(spec, seed), bool(plans["configurations"]["2d"]["batch_dice"]), device=DEV, configuration="2d_reduced", **kw)
    return tr, x, targets, plans, ds


def test_training_lowers_the_loss_and_overflow_skips_the_update():
    tr, x, targets, _, _ = _trainer(num_epochs=10)
    before = {k: p.detach().clone() for k, p in tr.network.p.items()}
    losses = [tr.train_step(x, targets) for _ in range(20)]
    print(f"[train] loss {losses[0]:.4f} -> {losses[-1]:.4f}, loss scale {tr.state['loss_scale']:g}, skipped {tr.state.get('skipped_steps', 0)}")
    assert all(math.isfinite(v) for v in losses)
    assert losses[-1] < losses[0]
    for k, p in tr.network.p.items():
        if k.startswith("decoder.seg_layers.0."):
            assert p.grad is None and torch.equal(p.detach(), before[k]), f"{k} is not graded: it must stay bit-unchanged (no weight decay either)"
        else:
            assert not torch.equal(p.detach(), before[k]), f"{k} did not move"
    # a forced overflow: a loss scale of 2^40 sends the float16 gradients to inf
    snap = {k: p.detach().clone() for k, p in tr.network.p.items()}
    bufs = {i: b.clone() for i, b in tr.state["sgd"]["momentum_buffer"].items()}
    tr.state["loss_scale"] = 2.0 ** 40
    skipped = tr.state.get("skipped_steps", 0)
    v = tr.train_step(x, targets)
    assert math.isfinite(v)
    assert tr.state["skipped_steps"] == skipped + 1 and tr.state["loss_scale"] == 2.0 ** 39
    assert all(torch.equal(p.detach(), snap[k]) for k, p in tr.network.p.items()), "an overflowing step must leave the parameters bit-unchanged"
    assert all(torch.equal(b, bufs[i]) for i, b in tr.state["sgd"]["momentum_buffer"].items())
    # a label outside [0, n_heads) at a scale that does not overflow: the loss kernel poisons loss and gradient, the update is skipped, train_step raises
    tr.state["loss_scale"] = 1024.0
    bad = [t.clone() for t in targets]
    bad[0][0, 0, 0] = 200
    with pytest.raises(ValueError, match="label outside"):
        tr.train_step(x, bad)
    assert tr.state["skipped_steps"] == skipped + 2
    assert all(torch.equal(p.detach(), snap[k]) for k, p in tr.network.p.items()), "a step with a bad label must leave the parameters bit-unchanged"


def test_run_training_round_trip(tmp_path):
    """Two epochs of two iterations into a trained-model folder; nnunet.load_trained_model_folder reads it back, and the inference head's logits agree with the
    trainer's own within the bound test_gpu_nnunet.test_network_logits_against_float64 uses for the configuration: min(2, twice the measured ratio) times the
    fp16-storage model's error of the float64 logits (the two run the same weights through the same forward kernels; they differ in the statistics'
    summation order and in where the norm is fused).  Each of the two is also within that rule's cap of the float64 logits."""
    import nnunet_ref
    tr, x, targets, plans, ds = _trainer(seed=9, num_epochs=2)
    folder = nnunet.write_trained_model_folder(str(tmp_path / "tissue_model"), plans, ds)
    vx, vt, _, _ = _trainer(seed=10, num_epochs=1)[1:]
    seen = []
    step = tr.validation_step

    def recording(data, tg):
        out = step(data, tg)
        seen.append(out)
        return out

    tr.validation_step = recording
    log = tr.run_training([{"data": x, "target": targets}], [(vx, vt)], os.path.join(folder, "fold_0"), iterations_per_epoch=2, val_iterations=1)
    assert len(log["train_losses"]) == 2 and tr.current_epoch == 2 and len(seen) == 2
    for name in ("checkpoint_best.pth", "checkpoint_final.pth"):
        assert os.path.exists(os.path.join(folder, "fold_0", name))
    ema, best = None, None
    for o in seen:
        tp, fp, fn = (o[k].astype(np.float64) for k in ("tp_hard", "fp_hard", "fn_hard"))
        assert len(tp) == tr.n_heads - 1 and (tp + fn).sum() == (vt[0] != 0).sum().item()
        with np.errstate(invalid="ignore", divide="ignore"):
            dice = float(np.nanmean(2 * tp / (2 * tp + fp + fn)))
        ema = dice if ema is None else 0.9 * ema + 0.1 * dice
        best = ema if best is None or ema > best else best
    assert tr._best_ema == best
    final = torch.load(os.path.join(folder, "fold_0", "checkpoint_final.pth"), map_location="cpu", weights_only=False)
    assert set(final) >= {"network_weights", "optimizer_state", "grad_scaler_state", "_best_ema", "current_epoch", "init_args", "trainer_name", "inference_allowed_mirroring_axes"}
    assert final["current_epoch"] == 2 and final["_best_ema"] == best and final["trainer_name"] == "nnUNetTrainer"
    assert set(final["network_weights"]) == set(nnunet.param_shapes(tr.spec, deep_supervision=True))
    assert all(torch.equal(final["network_weights"][k], p.detach().cpu()) for k, p in tr.network.p.items())
    model = nnunet.load_trained_model_folder(folder, checkpoint_name="checkpoint_final.pth", device=DEV)
    nnunet.load_trained_model_folder(folder, device=DEV)   # checkpoint_best.pth, the predictor's default
    assert model.mirror_axes == (0, 1) and model.spec == tr.spec
    got, own = model(vx.to(DEV)).double().cpu(), tr.eval_logits(vx).double().cpu()
    sd = {k: v for k, v in final["network_weights"].items() if k in nnunet.param_shapes(tr.spec)}
    f64 = nnunet_ref.forward(sd, tr.spec, vx, torch.float64)
    e_model = (nnunet_ref.forward(sd, tr.spec, vx, torch.float64, store=nnunet_ref.fp16_storage) - f64).abs().max().item()
    print(f"[round trip] inference head against the trainer's logits: {(got - own).abs().max():.3e}; fp16-storage model against float64: {e_model:.3e}; "
          f"ratio {(got - own).abs().max().item() / e_model:.3f}; against float64: head {(got - f64).abs().max():.3e}, trainer {(own - f64).abs().max():.3e}")
    assert got.shape == own.shape == (2, tr.n_heads, 64, 64)
    assert (got - own).abs().max().item() <= min(M_CAP, 2.0 * MEASURED_ROUND_TRIP) * e_model
    assert (got - f64).abs().max().item() <= M_CAP * e_model and (own - f64).abs().max().item() <= M_CAP * e_model
