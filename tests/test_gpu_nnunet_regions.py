"""GPU (-m gpu): region labels for the tissue head on the HIP library (csrc/kernels_segregion.hip) -- the Dice + focal / BCE entries
(ldiff_op_dice_focal / _stats / _from_sums) against the float64 restatement with the derived bound of tests/nnunet_region_ref.py, their exact
properties, the validation counts and the mask rule against torch, the trainer on a region spec, the trained folder's prediction, and the
data-parallel phases driven by hand in one process.

u = 2^-24, gamma(n) = 2 n u as in tests/test_gpu_nnunet_train.py."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nnunet_region_ref as rref
import nnunet_train_ref as ref
from ldiffusion_amd import autograd as ag, nnunet, nnunet_train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
U, U16, SUB16 = ref.U, ref.U16, ref.SUB16
WEIGHT, SCALE = 4 / 7, 1024.0
LABELS3 = {"background": 0, "whole": [1, 2, 3], "core": [2, 3], "enhancing": 3, "ignore": 4}
LABELS9 = dict({"background": 0}, **{f"r{i}": list(range(i + 1, 10)) for i in range(9)}, ignore=10)   # nine nested regions over the labels 1 .. 9


def spec_of(R):
    return nnunet.region_spec(LABELS3 if R == 3 else LABELS9, list(range(1, R + 1)))


def table_dev(rs):
    return nnunet.region_table_tensor(rs["table"], DEV)


def loss_case(R, B, H, W, seed, fraction=0.3):
    """fp16 logits [B, H, W, ld] with junk in the pad columns, int64 label maps with every label and about `fraction` of the pixels ignored."""
    rs = spec_of(R)
    g = torch.Generator().manual_seed(seed)
    ld = (R + 7) // 8 * 8
    logits = torch.zeros((B, H, W, ld), dtype=torch.float16)
    logits[..., :R] = (2.0 * torch.randn((B, H, W, R), generator=g)).to(torch.float16)
    logits[..., R:] = 7.0
    target = torch.randint(0, rs["ignore_label"], (B, H, W), generator=g)
    return rs, logits, (rref.ignore_blobs(target, rs["ignore_label"], fraction, seed + 1) if fraction else target)


def run(rs, logits, target, batch_dice, use_ignore, form="focal", weight=WEIGHT, grad_scale=SCALE):
    loss, dl = ag.dice_focal(logits.to(DEV), target.to(DEV), table_dev(rs), rs["n_heads"], batch_dice, weight, grad_scale, use_ignore=use_ignore, region_loss=form)
    torch.cuda.synchronize()
    return loss.cpu(), dl.cpu()


def tol_of(e, mag, gref):
    return e * mag + U16 * gref.abs() * (1 + e) + SUB16


# ---- 1. the loss against float64 ---------------------------------------------------------------------------------------------------------------------
# 72 x 72 = 5184 pixels: two chunks of 4096 per image, the second ragged and no multiple of 256.  B = 2 with batch_dice, B = 3 without.
LOSS_CASES = [(R, bd, i64, ign, "focal") for R in (3, 9) for bd in (True, False) for i64 in (False, True) for ign in (True, False)] + [(3, True, False, True, "bce")]


@pytest.mark.parametrize("i,R,batch_dice,i64,ignored,form", [(i,) + c for i, c in enumerate(LOSS_CASES)])
def test_dice_focal_against_float64(lib, i, R, batch_dice, i64, ignored, form):
    """Value and dlogits within nnunet_region_ref.loss_bounds of the float64 restatement (pinned to the reference's modules by
    tests/test_cpu_nnunet_regions.py); ignored rows and pad columns exactly +0; two launches bit-identical; the bounds reject the normaliser with the
    factor R, M = Bd (R - 1), the Dice over all pixels (where some are ignored) and the other form."""
    _against_float64(300 + i, R, 2 if batch_dice else 3, 72, 72, batch_dice, i64, ignored, form)


def test_dice_focal_where_the_finalize_loops_wrap(lib):
    """B = 20, R = 9, 8 x 8, per-sample Dice: Bd NC = 320 coefficients and Bd NACC = 1020 slots of sums, more than the finalize's 256 threads cover in a pass."""
    assert 20 * 16 > 256 and 20 * ag.dice_focal_nacc(9) > 256
    _against_float64(390, 9, 20, 8, 8, False, True, True, "focal")


def _against_float64(seed, R, B, H, W, batch_dice, i64, ignored, form):
    rs, logits, target = loss_case(R, B, H, W, seed, 0.3 if ignored else 0.0)
    tgt = target if i64 else target.to(torch.uint8)
    loss, dl = run(rs, logits, tgt, batch_dice, ignored, form)
    loss2, dl2 = run(rs, logits, tgt, batch_dice, ignored, form)
    assert torch.equal(loss, loss2) and torch.equal(dl.view(torch.int16), dl2.view(torch.int16)), "two launches on the same inputs differ"
    assert dl.dtype == torch.float16 and dl.shape == logits.shape
    assert not dl[..., R:].view(torch.int16).any(), "pad columns must be +0"
    ign = target == rs["ignore_label"]
    if ignored:
        assert 0.3 <= ign.double().mean() < 0.5 and not dl[ign].view(torch.int16).any(), "an ignored pixel's dlogits row must be +0"
    else:
        assert not ign.any()
    table = rs["table"]
    want, gwant = rref.loss_reference(logits, target, table, R, batch_dice, ignored, form, WEIGHT, SCALE)
    tol_value, e, mag = rref.loss_bounds(logits, target, table, R, batch_dice, ignored, form, WEIGHT, SCALE)
    got = dl[..., :R].double()
    err, keep = (got - gwant).abs(), ~ign
    print(f"[dice_focal] R={R} B={B} {H}x{W} batch_dice={batch_dice} i64={i64} ignored={ignored} {form}: value off by {abs(float(loss) - want):.2e} "
          f"(bound {tol_value:.2e}), gradient at {(err[keep] / tol_of(e, mag, gwant)[keep]).max():.3f} of its bound, |g| up to {gwant.abs().max():.2e}")
    assert abs(float(loss) - want) <= tol_value
    assert (err[keep] <= tol_of(e, mag, gwant)[keep]).all()
    wrong = [("the normaliser with the factor R", dict(form=form, wrong="norm")), ("M = Bd (R - 1)", dict(form=form, wrong="M")),
             ("focal swapped with BCE", dict(form="bce" if form == "focal" else "focal"))]
    if ignored:
        wrong.append(("the Dice over all pixels", dict(form=form, wrong="dice_all")))
    for what, kw in wrong:
        w, gw = rref.loss_reference(logits, target, table, R, batch_dice, ignored, kw.pop("form"), WEIGHT, SCALE, **kw)
        assert abs(float(loss) - w) > tol_value or ((got - gw).abs() > tol_of(e, mag, gw))[keep].any(), f"the bounds accept {what}"


# ---- 2. exact properties -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,batch_dice", [(3, True), (9, False)])
def test_ignored_logits_reach_no_output(lib, R, batch_dice):
    rs, logits, target = loss_case(R, 2, 72, 72, 410 + R)
    ign = target == rs["ignore_label"]
    loss, dl = run(rs, logits, target, batch_dice, True)
    assert not dl[ign].view(torch.int16).any() and dl[~ign][:, :R].any()
    for fill in (float("nan"), 65504.0):
        poked = logits.clone()
        poked[ign] = fill
        loss_p, dl_p = run(rs, poked, target, batch_dice, True)
        assert torch.equal(loss, loss_p) and torch.equal(dl.view(torch.int16), dl_p.view(torch.int16)) and math.isfinite(float(loss)), fill


@pytest.mark.parametrize("R,batch_dice,form", [(3, True, "focal"), (9, False, "focal"), (3, False, "bce")])
def test_whole_batch_ignored(lib, R, batch_dice, form):
    """No annotated pixel: the focal term is 0 / max(0, 1e-8) = 0, every dc is smooth / smooth = 1, so the loss is -1 (float64 in the kernel, one fp32
    rounding: 2 u asserted) and the gradient is +0 everywhere."""
    rs, logits, _ = loss_case(R, 2, 37, 53, 420)
    target = torch.full((2, 37, 53), rs["ignore_label"], dtype=torch.int64)
    loss, dl = run(rs, logits, target, batch_dice, True, form)
    assert abs(float(loss) + 1.0) <= 2 * U and not dl.view(torch.int16).any()


def test_bad_labels_and_refusals(lib):
    rs, logits, target = loss_case(3, 2, 15, 13, 430)
    spot = tuple(int(v) for v in (target != 4).nonzero()[0])
    for value, tgt_of in ((200, lambda t: t), (200, lambda t: t.to(torch.uint8)), (-1, lambda t: t), (5, lambda t: t)):
        bad = target.clone()
        bad[spot] = value                                               # neither a label nor the ignore label (bit 30 of the table)
        loss, dl = run(rs, logits, tgt_of(bad), True, True)
        assert math.isnan(float(loss)) and dl[spot][:3].isnan().all() and not dl[spot][3:].view(torch.int16).any()
        keep = torch.ones_like(target, dtype=torch.bool)
        keep[spot] = False
        assert not dl[keep].isnan().any()
    assert math.isnan(float(run(rs, logits, target, True, False)[0])), "without use_ignore a pixel with the ignore bit is a bad label"
    ld, td, tab = logits.to(DEV), target.to(DEV), table_dev(rs)
    with pytest.raises(ValueError, match="region_loss"):
        ag.dice_focal(ld, td, tab, 3, True, region_loss="dice")
    with pytest.raises(ValueError, match="table"):
        ag.dice_focal(ld, td, tab.cpu(), 3, True)
    with pytest.raises(ValueError, match="regions"):
        ag.dice_focal(ld, td, tab, 25, True)
    with pytest.raises(ValueError, match="row pitch"):
        ag.dice_focal(ld, td, tab, 9, True)
    z = ld.clone().requires_grad_(True)
    value, stored = ag.dice_focal(ld, td, tab, 3, True, WEIGHT, SCALE, use_ignore=True)
    term = ag.DiceFocalFn.apply(z, td, tab, 3, True, WEIGHT, SCALE, 1e-5, True, "focal")
    assert torch.equal(term, value * WEIGHT)
    term.backward()
    assert torch.equal(z.grad, stored)


@pytest.mark.parametrize("R,B,hw,batch_dice,ignored", [(3, 2, (72, 72), True, True), (9, 3, (72, 72), False, False), (9, 20, (8, 8), False, True),
                                                       (3, 2, (15, 13), True, False)])
def test_split_at_world_one_equals_the_one_call_entry(lib, R, B, hw, batch_dice, ignored):
    """stats then from_sums at world 1 give the one-call entry's bits (the wrapping shape included); the rows carry the exact region histograms and the
    annotated count."""
    rs, logits, target = loss_case(R, B, hw[0], hw[1], 440 + R, 0.3 if ignored else 0.0)
    NC = logits.shape[-1]
    one = run(rs, logits, target, batch_dice, ignored)
    ld, td, tab = logits.to(DEV), target.to(DEV), table_dev(rs)
    sums = ag.dice_focal_stats(ld, td, tab, R, batch_dice, use_ignore=ignored)
    assert sums.shape == (1 if batch_dice else B, ag.dice_focal_nacc(R)) and sums.dtype == torch.float64
    y, ign = rref.membership(target, rs["table"], R)
    hist = (y * (~ign)[:, None]).sum((2, 3))
    hist = hist.sum(0, keepdim=True) if batch_dice else hist
    count = (~ign).reshape(B, -1).sum(1).double()
    count = count.sum(0, keepdim=True) if batch_dice else count
    assert torch.equal(sums[:, 2 * NC:2 * NC + R].cpu(), hist) and torch.equal(sums[:, -1].cpu(), count) and float(sums[:, -2].sum()) == 0.0
    loss, dl = ag.dice_focal_from_sums(ld, td, tab, R, batch_dice, sums, sums, 1, WEIGHT, SCALE, use_ignore=ignored)
    assert torch.equal(loss.cpu(), one[0]) and torch.equal(dl.cpu().view(torch.int16), one[1].view(torch.int16))
    if ignored and batch_dice:
        with pytest.raises(NotImplementedError, match="ignore"):
            ag.dice_focal_from_sums(ld, td, tab, R, True, sums * 2, sums, 2, WEIGHT, SCALE, use_ignore=True)
    if not batch_dice:
        with pytest.raises(ValueError, match="per sample"):
            ag.dice_focal_from_sums(ld, td, tab, R, False, sums.clone(), sums, 1, WEIGHT, SCALE, use_ignore=ignored)


@pytest.mark.parametrize("R", [3, 9])
def test_the_two_normalisers_differ_by_the_factor_R(lib, R):
    """use_ignore = 1 on a target with nothing ignored: the same Dice term, the focal term R times the plain one (compound_losses.py:202 against :204).
    With weight = 1: loss_ignore - loss_plain = (R - 1) focal_mean, each value within its derived bound."""
    rs, logits, target = loss_case(R, 2, 37, 53, 450 + R, fraction=0.0)
    plain, on = run(rs, logits, target, True, False, weight=1.0)[0], run(rs, logits, target, True, True, weight=1.0)[0]
    y, _ = rref.membership(target, rs["table"], R)
    z = logits[..., :R].double().permute(0, 3, 1, 2)
    bce = F.binary_cross_entropy_with_logits(z, y, reduction="none")
    focal_mean = float((0.25 * (1 - torch.exp(-bce)) ** 2 * bce).mean())
    tol = sum(rref.loss_bounds(logits, target, rs["table"], R, True, ui, "focal", 1.0, 1.0)[0] for ui in (False, True))
    assert abs((float(on) - float(plain)) - (R - 1) * focal_mean) <= tol and (R - 1) * focal_mean > 100 * tol


# ---- 3. the data-parallel split, by hand -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,form", [(3, "focal"), (9, "focal"), (3, "bce")])
def test_exchanged_statistics_against_float64(lib, R, form):
    """One batch of 4 in two parts of 2 (no ignore label): each part's statistics, added in part order, then from_sums per part with world = 2.  The rule is
    dce_coef_loss's: rank r's value is its own focal mean minus the Dice of the summed statistics, its dlogits the gradient of focal_r - world * dice(all).
    Within the derived bound; the bound rejects a missing factor world and local instead of global sums."""
    rs, logits, target = loss_case(R, 4, 37, 53, 460 + R, fraction=0.0)
    tab = table_dev(rs)
    pl, pt = [logits[:2].contiguous(), logits[2:].contiguous()], [target[:2].contiguous(), target[2:].contiguous()]
    stats = [ag.dice_focal_stats(pl[q].to(DEV), pt[q].to(DEV), tab, R, True, region_loss=form) for q in range(2)]
    total = stats[0] + stats[1]
    whole = ag.dice_focal_stats(logits.to(DEV), target.to(DEV), tab, R, True, region_loss=form)
    NC = logits.shape[-1]
    assert torch.equal(total[:, 2 * NC:2 * NC + R], whole[:, 2 * NC:2 * NC + R]) and torch.equal(total[:, -1], whole[:, -1])
    assert ((total - whole).abs() <= 1e-12 * whole.abs()).all()
    zs = [p[..., :R].double().permute(0, 3, 1, 2).clone().requires_grad_(True) for p in pl]
    for r in range(2):
        loss, dl = ag.dice_focal_from_sums(pl[r].to(DEV), pt[r].to(DEV), tab, R, True, total, stats[r], 2, WEIGHT, SCALE, region_loss=form)
        got = dl[..., :R].double().cpu()

        def parts(z, t):
            """(the focal / BCE mean, -mean dc) of a batch: the restatement is their sum, and with wrong="norm" R times the first plus the second"""
            both = rref.dc_focal_loss(z, t, rs["table"], True, False, form)
            term = (rref.dc_focal_loss(z, t, rs["table"], True, False, form, wrong="norm") - both) / (R - 1)
            return term, both - term

        def rule(world_factor, global_sums):
            term_r = parts(zs[r], pt[r])[0]
            neg_dice = parts(torch.cat(zs, 0), torch.cat(pt, 0))[1] if global_sums else parts(zs[r], pt[r])[1]
            (g,) = torch.autograd.grad(term_r + world_factor * neg_dice, zs[r])
            return float((term_r + neg_dice).detach()), (g * (WEIGHT * SCALE)).permute(0, 2, 3, 1)

        want, gwant = rule(2.0, True)
        tol_value, e, mag = rref.loss_bounds(pl[r], pt[r], rs["table"], R, True, False, form, WEIGHT, SCALE, dice_logits=logits, dice_target=target, world=2)
        err = (got - gwant).abs()
        print(f"[ddp region loss] R={R} {form} rank {r}: value off by {abs(float(loss) - want):.2e} (bound {tol_value:.2e}), gradient at "
              f"{(err / tol_of(e, mag, gwant)).max():.3f} of its bound")
        assert abs(float(loss) - want) <= tol_value and (err <= tol_of(e, mag, gwant)).all()
        for what, args in (("a missing factor world", (1.0, True)), ("local sums", (2.0, False))):
            w, gw = rule(*args)
            assert abs(float(loss) - w) > tol_value or ((got - gw).abs() > tol_of(e, mag, gw)).any(), f"the bounds accept {what}"


# ---- 4. the validation counts and the mask ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,hw,i64", [(3, (37, 53), True), (9, (72, 72), False), (3, (72, 72), False), (9, (37, 53), True)])
def test_region_counts_equal_torch(lib, R, hw, i64):
    rs, logits, target = loss_case(R, 2, hw[0], hw[1], 470 + R)
    thr = nnunet.REGION_THRESHOLD_F16
    edge = torch.tensor([thr, thr * (1 + 2.0 ** -10), -thr, 0.0, float("inf"), -float("inf"), float("nan")], dtype=torch.float16)
    logits[0, 0, :7, 0] = edge                                        # the threshold's neighbours, +-inf and NaN among the logits
    logits[1, 1, :7, R - 1] = edge
    tgt = target if i64 else target.to(torch.uint8)
    got = ag.region_counts(logits.to(DEV), tgt.to(DEV), table_dev(rs), R, thr).cpu()
    y, ign = rref.membership(target, rs["table"], R)
    y, keep = y.bool(), (~ign)[:, None]
    pred = (torch.sigmoid(logits[..., :R]) > 0.5).permute(0, 3, 1, 2)   # the reference's expression, on the float16 output
    assert torch.equal(pred, (logits[..., :R] > thr).permute(0, 3, 1, 2))
    want = torch.stack([(pred & y & keep).sum((0, 2, 3)), (pred & ~y & keep).sum((0, 2, 3)), (~pred & y & keep).sum((0, 2, 3))])
    assert got.dtype == torch.int64 and got.shape == (3, R) and torch.equal(got, want) and int(want.sum()) > 0


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_region_mask_equals_the_reference_rule(lib, dtype):
    """Overlapping regions under a permuted regions_class_order: the later entry wins.  The two neighbours of each threshold, +-inf and NaN among the
    logits; float16 and float32 input; placement into a larger mask that keeps its other pixels."""
    R, H, W = 3, 37, 53
    order = [3, 1, 2]
    g = torch.Generator().manual_seed(480)
    logits = (1.5 * torch.randn((R, H, W), generator=g)).to(dtype)
    t32, t16 = nnunet.REGION_THRESHOLD_F32, nnunet.REGION_THRESHOLD_F16
    nxt32 = float((torch.tensor([t32]).view(torch.int32) + 1).view(torch.float32))
    edge = [t32, nxt32, t16, t16 * (1 + 2.0 ** -10), -t32, 0.0, float("inf"), -float("inf"), float("nan")]
    for r in range(R):
        logits[r, r, :len(edge)] = torch.tensor(edge).to(dtype)
        logits[(r + 1) % R, r, :len(edge)] = -1.0
        logits[(r + 2) % R, r, :len(edge)] = -1.0
    for thr in (t32, t16):
        want = rref.region_segmentation(logits.float(), order, thr)
        if thr == t32:   # the reference's own expression at inference
            seg = torch.zeros((H, W), dtype=torch.int16)
            for i, c in enumerate(order):
                seg[torch.sigmoid(logits.float())[i] > 0.5] = c
            assert torch.equal(seg, want)
        got = nnunet.region_mask_u8(logits.to(DEV), order, thr).cpu()
        assert got.dtype == torch.uint8 and torch.equal(got.to(torch.int16), want) and set(got.unique().tolist()) == {0, 1, 2, 3}
        big = torch.full((H + 9, W + 6), 77, dtype=torch.uint8, device=DEV)
        nnunet.region_mask_u8(logits.to(DEV), order, thr, out=big, origin=(4, 5))
        inside = big[4:4 + H, 5:5 + W].cpu()
        big[4:4 + H, 5:5 + W] = 77
        assert torch.equal(inside, got) and bool((big == 77).all())
    with pytest.raises(ValueError, match="does not lie inside"):
        nnunet.region_mask_u8(logits.to(DEV), order, t32, out=torch.zeros((H, W), dtype=torch.uint8, device=DEV), origin=(1, 0))
    with pytest.raises(ValueError, match="entries"):
        nnunet.region_mask_u8(logits.to(DEV), [1, 2], t32)


# ---- 5. the trainer ------------------------------------------------------------------------------------------------------------------------------------
def region_fixture(ignore=False, order=(1, 2, 3)):
    with open(os.path.join(GOLDEN, "nnunet_plans_2d.json")) as f:
        plans = json.load(f)
    with open(os.path.join(GOLDEN, "nnunet_dataset.json")) as f:
        ds = json.load(f)
    ds["labels"] = {k: v for k, v in LABELS3.items() if ignore or k != "ignore"}
    ds["regions_class_order"] = list(order)
    return plans, ds, nnunet.network_spec(plans, "2d_reduced", ds, accept_regions=True)


def _trainer_inputs(spec, seed=7, size=32, B=2, ignore=False):
    g = torch.Generator().manual_seed(seed)
    x = F.avg_pool2d(torch.randn((B, 3, size + 4, size + 4), generator=g), 5, 1) * 2.2
    targets = ref.label_maps(B, 4, size, spec["n_stages"] - 1, seed + 1)   # label values 0 .. 3
    if ignore:
        targets = [rref.ignore_blobs(t, 4, 0.3, 40 + i) for i, t in enumerate(targets)]
    return x, targets


@pytest.mark.parametrize("ignore,region_loss", [(False, "focal"), (True, "focal"), (False, "bce")])
def test_trainer_on_a_region_spec(ignore, region_loss):
    """One train_step: the loss on the trainer's OWN logits is the weighted sum of the restatement within the summed derived bounds (as
    test_trainer_with_ignored_pixels forms it), and misses the other form by far; parameters move.  validation_step's R-long counts equal torch's."""
    plans, ds, spec = region_fixture(ignore)
    batch_dice = bool(plans["configurations"]["2d"]["batch_dice"])
    x, targets = _trainer_inputs(spec, 9, ignore=ignore)
    sd = ref.synthetic_state_dict(spec, 9)
    tr = nnunet_train.Trainer(spec, sd, batch_dice, 10, device=DEV, configuration="2d_reduced", region_loss=region_loss)
    assert tr.regions and tr.n_heads == 3 and tr.ignore_label == (4 if ignore else None)
    outs = tr.network(x)
    lib_loss = float(tr.loss(outs, [t.to(DEV) for t in targets]))
    table = spec["region_table"]
    graded = [(o.detach().cpu(), t, w) for o, t, w in zip(outs, targets, tr.weights) if w != 0.0]
    want = sum(w * rref.loss_reference(o, t, table, 3, batch_dice, ignore, region_loss, 1.0, 1.0)[0] for o, t, w in graded)
    tol = sum(w * rref.loss_bounds(o, t, table, 3, batch_dice, ignore, region_loss, 1.0, 1.0)[0] for o, t, w in graded) + 2 * len(graded) * U * abs(want)
    other = sum(w * rref.loss_reference(o, t, table, 3, batch_dice, ignore, "bce" if region_loss == "focal" else "focal", 1.0, 1.0)[0] for o, t, w in graded)
    print(f"[trainer regions] ignore={ignore} {region_loss}: on its own logits off by {abs(lib_loss - want):.3e}, bound {tol:.3e}; the other form is {abs(other - want):.3e} away")
    assert abs(lib_loss - want) <= tol < abs(other - want)
    v = tr.validation_step(x, [t.to(DEV) for t in targets])
    top = outs[0].detach().cpu()[..., :3]
    y, ign = rref.membership(targets[0], table, 3)
    y, keep, pred = y.bool(), (~ign)[:, None], (torch.sigmoid(top) > 0.5).permute(0, 3, 1, 2)
    for key, m in (("tp_hard", pred & y & keep), ("fp_hard", pred & ~y & keep), ("fn_hard", ~pred & y & keep)):
        assert v[key].shape == (3,) and np.array_equal(v[key], m.sum((0, 2, 3)).numpy()), key
    assert math.isfinite(v["loss"])
    before = [p.detach().clone() for p in tr.params]
    first = tr.train_step(x, targets)
    assert math.isfinite(first) and abs(first - lib_loss) < 1e-6 and tr.state.get("skipped_steps", 0) == 0
    assert any(not torch.equal(p, q) for p, q in zip(tr.params, before))
    with pytest.raises(ValueError, match="region_loss"):
        nnunet_train.Trainer(spec, sd, batch_dice, 10, device=DEV, region_loss="ce")


def test_two_epochs_write_a_folder_that_predicts_region_masks(tmp_path):
    """Two epochs of two iterations write checkpoint_best.pth and checkpoint_final.pth; the folder loads without an opt-in; predict_mask returns only
    values of regions_class_order and 0, the same mask bit for bit per tile and with batch_tiles = 2, and 0 outside the crop box."""
    plans, ds, spec = region_fixture(order=(3, 1, 2))
    batch_dice = bool(plans["configurations"]["2d"]["batch_dice"])
    x, targets = _trainer_inputs(spec, 11)
    folder = nnunet.write_trained_model_folder(str(tmp_path / "model"), plans, ds)
    tr = nnunet_train.Trainer(spec, nnunet_train.initial_state_dict(spec, 7), batch_dice, 2, device=DEV, configuration="2d_reduced",
                              init_args={"configuration": "2d_reduced", "fold": 0})
    batches = [(x, targets)]
    log = tr.run_training(batches, batches, os.path.join(folder, "fold_0"), iterations_per_epoch=2, val_iterations=1)
    assert len(log["train_losses"]) == 2 and np.isfinite(log["train_losses"]).all() and len(log["dice_per_class_or_region"][0]) == 3
    assert all(os.path.exists(os.path.join(folder, "fold_0", n)) for n in ("checkpoint_best.pth", "checkpoint_final.pth"))
    head = nnunet.load_trained_model_folder(folder, device=DEV)
    assert head.num_heads == 3 and head.spec["regions_class_order"] == [3, 1, 2] and head.spec["regions"] == [(1, 2, 3), (2, 3), 3]
    g = torch.Generator().manual_seed(3)
    img = (torch.rand((3, 80, 72), generator=g) * 254 + 1).floor()
    img[:, :6] = 0                                                    # rows outside the crop box
    img[:, :, :4] = 0
    data = img.to(DEV)
    per_tile = head.predict_mask(data, tile_size=(32, 32))
    batched = head.predict_mask(data, tile_size=(32, 32), batch_tiles=2)
    assert per_tile.dtype == torch.uint8 and per_tile.shape == (80, 72) and torch.equal(per_tile, batched)
    assert set(per_tile.unique().tolist()) <= {0, 1, 2, 3} and not per_tile[:6].any() and not per_tile[:, :4].any()
    logits = head.network(nnunet.preprocess(data, head.normalization_schemes)[0][None, :, :32, :32])[0]
    assert torch.equal(nnunet.region_mask_u8(logits.float(), [3, 1, 2]).cpu().to(torch.int16), rref.region_segmentation(logits.float().cpu(), [3, 1, 2], nnunet.REGION_THRESHOLD_F32))


def test_two_trainers_at_world_two_by_hand():
    """The three phases with the two collectives done in this process, no process spawned, on the halves of a batch of 4 at 64 x 64 (LeakyReLU slope 1.0,
    where the gradient is a well-conditioned function of the forward's rounding: tests/test_gpu_nnunet_train.py).
    * The summed statistics of the two trainers equal one trainer's on the whole batch: counts exactly, sums to float64 rounding where the two runs'
      logits agree and else within the Lipschitz bound of the logits' difference.
    * Values: rank r's value is sum_i w_i (focal_r - dice(all)) of its own logits.  Each run's value lies within ITS OWN bound of its float64 restatement:
      sum_i w_i loss_bounds_i (the rank's bound takes the Dice sums of all ranks' logits) plus 2 u per graded term for the weighting and adding in fp32.
      The mean of the ranks' values (a halving: exact) is therefore within the mean of their two bounds of the mean of their restatements.
    * The averaged bucket, (bucket_0 + bucket_1) / (world * loss scale), per live tensor against the float64 tape of the whole batch's step (equal parts make
      (1 / W) sum_r focal_r - dice(all) the whole batch's loss): the library's figure (max |g - g64| / max |g64|) within
      M_CAP = 2 times the fp16-storage model's (the float64 tape with every stored tensor rounded to fp16 at the loss scale: the project's yardstick for a
      step, tests/test_gpu_nnunet_train.py), and so is the single trainer's gradient on the whole batch; hence the two agree within twice that.  The bound
      rejects the bucket without the factor 1 / world in every tensor.  The conv biases in front of an InstanceNorm are left out of this assertion and only
      printed: their gradient is mathematically zero, so the library's value and the model's are two realisations of rounding noise (about 1e-7 absolute
      here) whose ratio no number format bounds.  Measured on an MI355X: averaged bucket 2.14 x the model's, the single trainer on the whole batch 3.13 x
      (decoder.stages.1.convs.1.conv.bias, 9.9e-8 against 4.6e-8); the other tensors 1.48 x and 1.47 x.
    * The update runs on both ranks and leaves them with the same parameters."""
    import test_gpu_nnunet_train as T
    plans, ds, spec = region_fixture()
    batch_dice = bool(plans["configurations"]["2d"]["batch_dice"])
    assert batch_dice
    slope, R, table = 1.0, 3, spec["region_table"]
    x, targets = _trainer_inputs(spec, 13, size=64, B=4)
    halves = [(x[:2], [t[:2] for t in targets]), (x[2:], [t[2:] for t in targets])]
    sd = nnunet_train.initial_state_dict(spec, 7)
    kw = dict(device=DEV, configuration="2d_reduced", ddp=True, slope=slope, loss_scale=T.LOSS_SCALE)
    trainers = [nnunet_train.Trainer(spec, sd, batch_dice, 10, **kw) for _ in range(2)]
    for tr in trainers:
        tr.world = 2
    whole = nnunet_train.Trainer(spec, sd, batch_dice, 10, **kw)
    graded_idx = [i for i, w in enumerate(whole.weights) if w != 0.0]
    with torch.no_grad():
        own = [[o.detach().cpu() for o in tr.network(h[0])] for tr, h in zip(trainers, halves)]
        own_whole = [o.detach().cpu() for o in whole.network(x)]
    tables = [tr.step_forward(*h) for tr, h in zip(trainers, halves)]
    sums = tables[0] + tables[1]
    one = whole.step_forward(x, targets)
    NC = 8
    assert sums.shape == one.shape == (len(graded_idx), ag.dice_focal_nacc(R))
    assert torch.equal(sums[:, 2 * NC:2 * NC + R], one[:, 2 * NC:2 * NC + R]) and torch.equal(sums[:, -1], one[:, -1]) and float(sums[:, -2].sum()) == 0.0
    # The sums of p and of the focal term follow the logits, and the head's fp16 logits of a batch of 2 need not be those of the batch of 4 bit for bit
    # (another launch plan).  sigmoid is 1/4-Lipschitz and the focal term 1/2-Lipschitz (|df/dx| = 0.25 q^2 (2 p_t bce + q) <= 0.25 (2 / e + 1), as
    # p_t (-ln p_t) <= 1 / e), so a slot moves by at most that times the summed logit difference of its scale; where the logits agree, float64 rounding.
    for row, i in enumerate(graded_idx):
        delta = float((torch.cat((own[0][i], own[1][i]), 0)[..., :R].double() - own_whole[i][..., :R].double()).abs().sum())
        lip = torch.zeros(ag.dice_focal_nacc(R), dtype=torch.float64)
        lip[:2 * NC], lip[3 * NC] = 0.25, 0.5
        off = (sums[row] - one[row]).abs().cpu()
        print(f"[ddp regions] scale {i}: summed logit difference {delta:.3e}, statistics off by up to {off.max():.3e}")
        assert (off <= lip * delta + 1e-12 * one[row].abs().cpu()).all(), i
    outs = [tr.step_backward(sums) for tr in trainers]
    total_whole, bucket_whole = whole.step_backward(one)

    # values: every run against its own restatement within its own bound
    def parts(z, t):
        both = rref.dc_focal_loss(z, t, table, True, False, "focal")
        term = (rref.dc_focal_loss(z, t, table, True, False, "focal", wrong="norm") - both) / (R - 1)
        return float(term), float(both - term)

    def nchw(o):
        return o[..., :R].double().permute(0, 3, 1, 2)

    wants, tols = [], []
    for r in range(2):
        want = tol = 0.0
        for i in graded_idx:
            o_all, t_all = torch.cat((own[0][i], own[1][i]), 0), targets[i]
            want += whole.weights[i] * (parts(nchw(own[r][i]), halves[r][1][i])[0] + parts(nchw(o_all), t_all)[1])
            tol += whole.weights[i] * rref.loss_bounds(own[r][i], halves[r][1][i], table, R, True, False, "focal", 1.0, 1.0, dice_logits=o_all, dice_target=t_all, world=2)[0]
        wants.append(want)
        tols.append(tol + 2 * len(graded_idx) * U * abs(want))
        assert abs(float(outs[r][0]) - want) <= tols[r], r
    want_w = sum(whole.weights[i] * sum(parts(nchw(own_whole[i]), targets[i])) for i in graded_idx)
    tol_w = sum(whole.weights[i] * rref.loss_bounds(own_whole[i], targets[i], table, R, True, False, "focal", 1.0, 1.0)[0] for i in graded_idx) + \
        2 * len(graded_idx) * U * abs(want_w)
    mean_value = (float(outs[0][0]) + float(outs[1][0])) / 2
    print(f"[ddp regions] mean of the ranks' values {mean_value:.6f} (restated {sum(wants) / 2:.6f}, bound {sum(tols) / 2:.2e}); the whole batch "
          f"{float(total_whole):.6f} (restated {want_w:.6f}, bound {tol_w:.2e})")
    assert abs(mean_value - sum(wants) / 2) <= sum(tols) / 2 and abs(float(total_whole) - want_w) <= tol_w

    # the averaged bucket against the float64 tape of the whole batch
    def per_tensor(tr, flat):
        g = {k: None for k in tr.names}
        for j, i in enumerate(tr._live):
            g[tr.names[i]] = flat[tr._offsets[j]:tr._offsets[j + 1]].view_as(tr.params[i])
        return g

    summed = (outs[0][1] + outs[1][1]).double().cpu()
    assert summed.shape == bucket_whole.shape
    ddp_g = per_tensor(trainers[0], summed / (2 * T.LOSS_SCALE))
    no_world = per_tensor(trainers[0], summed / T.LOSS_SCALE)
    whole_g = per_tensor(whole, bucket_whole.double().cpu() / T.LOSS_SCALE)
    weights = nnunet_train.deep_supervision_weights(spec["n_stages"] - 1)
    _, g64 = rref.step_gradients(sd, spec, x, targets, weights, table, True, slope)
    _, gmod = rref.step_gradients(sd, spec, x, targets, weights, table, True, slope, storage16=True, loss_scale=T.LOSS_SCALE)
    assert all((ddp_g[k] is None) == (g is None) for k, g in g64.items()) and ddp_g["decoder.seg_layers.0.weight"] is None
    figures = {name: T._step_figures(dict(f64=g64, lib=lib_g, model=gmod), False) for name, lib_g in (("ddp", ddp_g), ("whole", whole_g), ("no 1 / world", no_world))}
    for name in ("ddp", "whole"):
        rows, bias_rows = figures[name]
        print(f"[ddp regions] {name}: worst ratio to the fp16-storage model {max(r[1] / r[2] for r in rows):.3f}, conv.bias {max(r[1] / r[2] for r in bias_rows):.3f}")
    for name in ("ddp", "whole"):
        for k, e_lib, e_model in figures[name][0]:
            assert e_lib <= T.M_CAP * e_model, f"{name} {k}: library {e_lib:.3e}, fp16-storage model {e_model:.3e}: {e_lib / e_model:.2f} x (asserted {T.M_CAP} x)"
    for k, _, e_model in figures["ddp"][0]:   # each within M_CAP e_model of the tape, so within twice that of each other
        assert ((ddp_g[k] - whole_g[k]).abs().max() / g64[k].abs().max()).item() <= 2 * T.M_CAP * e_model, k
    for k, e_lib, e_model in figures["no 1 / world"][0]:
        assert e_lib > T.M_CAP * e_model, f"the bound accepts {k} without the factor 1 / world"

    ran = [tr.step_update((outs[0][1] + outs[1][1]).clone()) for tr in trainers]
    assert ran == [True, True] and all(torch.equal(p, q) for p, q in zip(trainers[0].params, trainers[1].params))
    assert any(not torch.equal(p.detach().cpu(), sd[n]) for n, p in zip(trainers[0].names, trainers[0].params))
    ign = nnunet_train.Trainer(region_fixture(ignore=True)[2], sd, batch_dice, 10, device=DEV, configuration="2d_reduced", ddp=True)
    ign.world = 2                                                     # regions with an ignore label above world size 1 stay refused
    with pytest.raises(NotImplementedError, match="ignore_label"):
        ign.step_forward(*halves[0])


# ---- 6. the store ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ignore", [False, True])
def test_device_build_of_a_region_store_equals_the_host_build(ignore):
    """Per region the membership plane (a gather through the table) goes through ldiff_op_case_counts / ldiff_op_case_rank_to_coord with two heads and
    selector 1: the same class_locations as the host's np.isin walk, entry by entry, and the same batches from both stores."""
    from ldiffusion_amd import nnunet_data as nd
    rs = nnunet.region_spec({k: v for k, v in LABELS3.items() if ignore or k != "ignore"}, [1, 2, 3])
    rng = np.random.default_rng(21)
    top = 5 if ignore else 4
    cases = [(torch.from_numpy(rng.integers(1, 256, (3, 40, 36)).astype(np.uint8)),
              torch.from_numpy(np.kron(rng.integers(0, top, (10, 9)), np.ones((4, 4), np.int64)).astype(np.uint8))) for _ in range(2)]
    schemes = ["ZScoreNormalization"] * 3
    host = nd.CaseStore(cases, schemes, 3, device=DEV, regions=rs, build="host", crop=True)
    dev = nd.CaseStore([(i.to(DEV), s.to(DEV)) for i, s in cases], schemes, 3, device=DEV, regions=rs, build="device")
    keys = [(1, 2, 3), (2, 3), 3] + ([(0, 1, 2, 3)] if ignore else [])
    for i in range(2):
        assert torch.equal(host.labels(i), dev.labels(i)) and list(host.class_locations[i]) == list(dev.class_locations[i]) == keys
        for k in keys:
            hl, dl = np.asarray(host.class_locations[i][k]), np.asarray(dev.class_locations[i][k])
            assert len(hl) > 0 and hl.shape == dl.shape and np.array_equal(hl, dl), (i, k)
            assert np.array_equal(dl[np.lexsort((dl[:, 1], dl[:, 0]))], np.argwhere(np.isin(cases[i][1].numpy(), k)))
    a, b = next(nd.PatchLoader(host, (16, 16), 4, 2, seed=5, train=True)), next(nd.PatchLoader(dev, (16, 16), 4, 2, seed=5, train=True))
    assert all(torch.equal(p, q) for p, q in zip(a["target"], b["target"])) and int(a["target"][0].max()) <= top - 1


# ---- 7. the stage ----------------------------------------------------------------------------------------------------------------------------------
def test_stage_with_region_labels(tmp_path, monkeypatch):
    """Six 64 x 64 images (tests/test_gpu_nnunet_ignore.py's stage setting) through Segmentor.train_tissue_model_nnUNetv2(regions=..., as grey levels):
    dataset.json carries the region labels as class indices and regions_class_order, the label PNGs keep class indices, the stores are keyed by region,
    the trainer reports three regions, and the written folder loads and predicts only values of regions_class_order and 0."""
    from PIL import Image
    from ldiffusion_amd import metrics, utils
    from ldiffusion_amd.segmentor import Segmentor
    rng = np.random.RandomState(33)
    levels = np.array(sorted(metrics.PIXEL_TO_LABEL), np.uint8)
    src = tmp_path / "src"
    src.mkdir()
    images, labels = [], []
    for i in range(6):
        Image.fromarray(rng.randint(1, 256, (64, 64, 3)).astype(np.uint8)).save(src / f"im{i}.png")
        Image.fromarray(levels[np.kron(rng.randint(0, 7, (8, 8)), np.ones((8, 8), np.int64))]).save(src / f"lb{i}.png")
        images.append(str(src / f"im{i}.png"))
        labels.append(str(src / f"lb{i}.png"))
    for name in ("nnUNet_raw", "nnUNet_preprocessed", "nnUNet_results"):
        (tmp_path / name).mkdir()
        monkeypatch.setenv(name, str(tmp_path / name))
    monkeypatch.setattr(Segmentor, "load_ldiffusion", lambda self, w, p, **kw: (None, None, None))
    monkeypatch.setattr(utils, "check_images_same_size", lambda paths: False)      # plain copies: no sampler runs
    regions = {"any": [100, 150, 50, 200, 250, 255], "high": [200, 250, 255], "top": [255]}   # grey levels of metrics.PIXEL_TO_LABEL
    seg = Segmentor(None, None, "tissue", 7)
    with pytest.raises(ValueError, match="`regions_class_order` is missing"):
        seg.train_tissue_model_nnUNetv2(1, "weights", "sd", images, labels, images[:2], labels[:2], regions=regions)
    with pytest.raises(ValueError, match=r"classes \[1, 2, 3\] lie in no region"):
        seg.train_tissue_model_nnUNetv2(1, "weights", "sd", images, labels, images[:2], labels[:2], regions={"high": [4, 5, 6]}, regions_class_order=[4])
    assert not os.listdir(tmp_path / "nnUNet_raw"), "a refused call writes nothing"
    folder = seg.train_tissue_model_nnUNetv2(1, "weights", "sd", images, labels, images[:2], labels[:2], iterations_per_epoch=2, val_iterations=1,
                                             num_foreground_voxels=6e4, regions=regions, regions_class_order=[1, 4, 6])
    monkeypatch.undo()
    raw = tmp_path / "nnUNet_raw" / "Dataset001_Custom"
    want_labels = {"background": 0, "any": [1, 2, 3, 4, 5, 6], "high": [4, 5, 6], "top": [6]}
    for path in (raw / "dataset.json", os.path.join(folder, "dataset.json")):
        ds = json.loads(open(path).read())
        assert ds["labels"] == want_labels and ds["regions_class_order"] == [1, 4, 6]
    assert np.array(Image.open(raw / "labelsTr" / "case_000.png")).max() <= 6
    log = seg.training_log
    assert len(log["train_losses"]) == 1 and np.isfinite(log["train_losses"]).all() and np.isfinite(log["val_losses"]).all()
    assert len(log["dice_per_class_or_region"][0]) == 3
    assert all(list(cl) == [(1, 2, 3, 4, 5, 6), (4, 5, 6), (6,)] for cl in seg.tissue_loaders[0].store.class_locations)
    head = nnunet.load_trained_model_folder(folder, device=DEV)
    assert head.num_heads == 3 and head.spec["regions_class_order"] == [1, 4, 6]
    data = torch.from_numpy(rng.randint(1, 256, (3, 64, 48)).astype(np.float32)).to(DEV)
    mask = head.predict_mask(data)
    assert mask.shape == (64, 48) and set(mask.unique().tolist()) <= {0, 1, 4, 6} and torch.equal(mask, head.predict_mask(data, batch_tiles=2))
