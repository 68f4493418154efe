"""GPU (-m gpu): nnU-Net's ignore label for the tissue head on the HIP library -- the ignore form of the Dice + cross-entropy entries
(ldiff_op_dice_ce_ignore / _stats / _from_sums; csrc/kernels_segtrain.hip) against the float64 restatement with the derived bound of
tests/nnunet_ignore_ref.py, its exact properties (zero rows, isolation from ignored logits, the plain entry's bits where nothing is ignored), the trainer,
the device build of a store with an ignore label, and the stage from label PNGs with an ignored grey level to a folder the inference head reads.

u = 2^-24, gamma(n) = 2 n u as in tests/test_gpu_nnunet_train.py.

WRAP_CASES (batches at which the finalize covers its tables in several passes), measured on an MI355X as the worst error / bound over the cases: value 0.008,
gradient 0.998 (the float64 gradient rounded to fp16 sits at 0.998 of that bound on the same inputs: at this loss scale the bound is the rounding of the store)."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nnunet_ignore_ref as iref
import nnunet_train_ref as ref
import test_gpu_nnunet_train as T
from ldiffusion_amd import autograd as ag, metrics, nnunet, nnunet_data as nd, nnunet_train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
U, U16, SUB16 = ref.U, ref.U16, ref.SUB16
M_CAP = 2.0          # tests/test_gpu_nnunet_train.py's cap on the library's error in units of the fp16-storage model's
WEIGHT, SCALE = 4 / 7, 1024.0


def fixtures():
    with open(os.path.join(GOLDEN, "nnunet_plans_2d.json")) as f:
        plans = json.load(f)
    with open(os.path.join(GOLDEN, "nnunet_dataset.json")) as f:
        ds = json.load(f)
    return plans, ds


# ---- 1. the kernels --------------------------------------------------------------------------------------------------------------------------------
def loss_case(n, B, H, W, seed, fraction=0.3):
    """fp16 logits [B, H, W, ld] with junk in the pad columns, int64 targets with every class and about `fraction` of the pixels ignored (label n)."""
    g = torch.Generator().manual_seed(seed)
    ld = (n + 7) // 8 * 8
    logits = torch.zeros((B, H, W, ld), dtype=torch.float16)
    logits[..., :n] = (2.0 * torch.randn((B, H, W, n), generator=g)).to(torch.float16)
    logits[..., n:] = 7.0
    target = torch.randint(0, n, (B, H, W), generator=g)
    return logits, (iref.ignore_blobs(target, n, fraction, seed + 1) if fraction else target)


def run(logits, target, n, batch_dice, ignore, weight=WEIGHT, grad_scale=SCALE):
    loss, dl = ag.dice_ce(logits.to(DEV), target.to(DEV), n, batch_dice, weight, grad_scale, ignore_label=ignore)
    torch.cuda.synchronize()
    return loss.cpu(), dl.cpu()


SHAPES = [(15, 13), (48, 40), (72, 64)]   # fewer pixels than a workgroup has threads; one ragged chunk of DCE_PIX = 4096; one full chunk plus 512 pixels
KERNEL_CASES = [(n, hw, bd, i64) for n in (3, 9) for hw in SHAPES for bd in (True, False) for i64 in (False, True)]
# row pitches 24 and 32, the kernels' NV = 3 and NV = 4 instantiations.  The leading number is the case's seed offset, picked on the CPU so that
# ignore_blobs ends within the fraction asserted below and every class keeps an annotated pixel in each image
WIDE_CASES = [(24, 17, (72, 64), True, True), (25, 17, (72, 64), False, True), (26, 17, (15, 13), True, True), (27, 17, (15, 13), False, True),
              (28, 32, (72, 64), True, True), (29, 32, (72, 64), False, True), (31, 32, (15, 13), True, True), (33, 32, (15, 13), False, True)]


# tests/test_gpu_nnunet_train.py's LOSS_WRAP_NB in the ignore form, whose rows are one slot longer: B NACC = 297 / 825 / 891 slots of sums, B NC = 88 / 264 /
# 288 coefficients, so that the finalize's loops wrap with batch_dice off.  (seed offset, n, B, map, batch_dice)
WRAP_CASES = [(40 + 4 * k + 2 * j + int(bd), n, B, hw, bd) for k, (n, B) in enumerate(T.LOSS_WRAP_NB) for j, hw in enumerate(((15, 13), (72, 64))) for bd in (False, True)]


@pytest.mark.parametrize("i,n,hw,batch_dice,i64", [(i,) + c for i, c in enumerate(KERNEL_CASES)] + WIDE_CASES)
def test_dice_ce_ignore_against_float64(lib, i, n, hw, batch_dice, i64):
    """Value and dlogits of the ignore form against the float64 restatement (pinned to the reference's modules by tests/test_cpu_nnunet_ignore.py) within
    nnunet_ignore_ref.loss_bounds; every ignored pixel's row exactly zero, pad columns exactly zero, two launches bit-identical; the bound rejects the
    plain loss with the ignored pixels read as background, and the flipped batch_dice."""
    _ignore_against_float64(i, n, 2, hw, batch_dice, i64)


@pytest.mark.parametrize("i,n,B,hw,batch_dice", WRAP_CASES)
def test_dice_ce_ignore_against_float64_where_the_finalize_wraps(lib, i, n, B, hw, batch_dice):
    """The same statements at WRAP_CASES (int64 labels); there the bounds also reject, by the value and by the gradient, a Dice term that leaves out the
    samples whose slots of the sums table the finalize reaches in a later pass."""
    _ignore_against_float64(i, n, B, hw, batch_dice, True)


def _ignore_against_float64(i, n, B, hw, batch_dice, i64):
    H, W = hw
    logits, target = loss_case(n, B, H, W, 700 + i)
    tgt = target if i64 else target.to(torch.uint8)
    loss, dl = run(logits, tgt, n, batch_dice, n)
    loss2, dl2 = run(logits, tgt, n, batch_dice, n)
    assert torch.equal(loss, loss2) and torch.equal(dl, dl2), "two launches on the same inputs differ"
    assert dl.dtype == torch.float16 and dl.shape == logits.shape and not dl[..., n:].any(), "pad columns must be exactly zero"
    ignored = target == n
    assert 0.3 <= ignored.double().mean() < 0.5
    assert torch.equal(dl[ignored], torch.zeros_like(dl[ignored])), "an ignored pixel's dlogits must be exactly zero"
    want, gwant = iref.loss_reference(logits, target, n, batch_dice, n, WEIGHT, SCALE)
    tol_value, e, mag = iref.loss_bounds(logits, target, n, batch_dice, n, WEIGHT, SCALE)
    got = dl[..., :n].double()

    def tol_of(gref):
        return e * mag + U16 * gref.abs() * (1 + e) + SUB16

    err = (got - gwant).abs()
    keep = ~ignored
    print(f"[dice_ce ignore] n={n} {hw} batch_dice={batch_dice} i64={i64}: value off by {abs(float(loss) - want):.2e} (bound {tol_value:.2e}), gradient at "
          f"{(err[keep] / tol_of(gwant)[keep]).max():.3f} of its bound, |g| up to {gwant.abs().max():.2e}, {float(ignored.double().mean()):.2f} ignored")
    assert abs(float(loss) - want) <= tol_value
    assert (err[keep] <= tol_of(gwant)[keep]).all()
    as_background = torch.where(ignored, torch.zeros_like(target), target)
    wrong = [("ignored pixels read as background", iref.loss_reference(logits, as_background, n, batch_dice, n + 1, WEIGHT, SCALE)),
             ("flipped batch_dice", iref.loss_reference(logits, target, n, not batch_dice, n, WEIGHT, SCALE))]
    for what, (w, gw) in wrong:
        assert abs(float(loss) - w) > tol_value or ((got - gw).abs() > tol_of(gw) + 0.0)[keep].any(), f"the bounds accept {what}"
    first = 256 // ag.dice_ce_nacc(n, n)   # the samples whose every slot of the sums table lies in the finalize's first pass
    if first < B:
        z = logits[..., :n].double().permute(0, 3, 1, 2).clone().requires_grad_(True)
        w = ref.first_pass_dice_loss(z, target, first, lambda a, t: iref.dc_ce_loss_ignore(a, t, batch_dice, n), lambda a, t: F.cross_entropy(a, t, ignore_index=n))
        gw = torch.autograd.grad(w, z)[0].permute(0, 2, 3, 1) * (WEIGHT * SCALE)
        assert abs(float(loss) - float(w)) > tol_value, f"the value's bound accepts a Dice term of the first {first} samples of {B}"
        assert ((got - gw).abs() > tol_of(gw))[keep].any(), f"the gradient's bound accepts a Dice term of the first {first} samples of {B}"


@pytest.mark.parametrize("n,hw,batch_dice", [(3, (48, 40), True), (9, (72, 64), False), (9, (15, 13), True)])
def test_ignored_logits_reach_no_output(lib, n, hw, batch_dice):
    """Isolation: +-65504 (and NaN) in the logits of ignored pixels leaves the loss and every other dlogits element bit-identical, the ignored rows zero."""
    logits, target = loss_case(n, 2, hw[0], hw[1], 810 + n)
    ignored = target == n
    loss, dl = run(logits, target, n, batch_dice, n)
    for fill in (65504.0, -65504.0, float("nan")):
        poked = logits.clone()
        poked[ignored] = fill
        loss_p, dl_p = run(poked, target, n, batch_dice, n)
        assert torch.equal(loss, loss_p) and torch.equal(dl, dl_p), fill
    alt = logits.clone()
    alt[ignored] = torch.where(torch.arange(alt.shape[-1]) % 2 == 0, 65504.0, -65504.0).to(torch.float16)
    loss_p, dl_p = run(alt, target, n, batch_dice, n)
    assert torch.equal(loss, loss_p) and torch.equal(dl, dl_p) and math.isfinite(float(loss))


@pytest.mark.parametrize("n", [3, 9])
@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("batch_dice", [True, False])
def test_no_ignored_pixel_gives_the_plain_entry_bits(lib, n, hw, batch_dice):
    logits, target = loss_case(n, 2, hw[0], hw[1], 900 + n, fraction=0.0)
    for tgt in (target, target.to(torch.uint8)):
        plain = run(logits, tgt, n, batch_dice, None)
        ign = run(logits, tgt, n, batch_dice, n)
        assert torch.equal(plain[0], ign[0]) and torch.equal(plain[1], ign[1])
        assert plain[1][..., :n].any()


@pytest.mark.parametrize("n,batch_dice", [(3, True), (3, False), (9, True), (9, False)])
def test_whole_batch_ignored(lib, n, batch_dice):
    """No annotated pixel: the cross-entropy term is 0 and every dc is smooth / smooth, so the loss is -1 up to the rounding of that quotient and of the
    mean (float64 in the kernel, one fp32 rounding at the end: 2 u asserted), and the gradient is zero everywhere."""
    logits, _ = loss_case(n, 2, 48, 40, 950)
    target = torch.full((2, 48, 40), n, dtype=torch.int64)
    loss, dl = run(logits, target, n, batch_dice, n)
    assert abs(float(loss) + 1.0) <= 2 * U and torch.equal(dl, torch.zeros_like(dl))
    one = target.clone()
    one[0] = torch.randint(0, n, (48, 40), generator=torch.Generator().manual_seed(1))   # one image ignored entirely: finite, and its rows zero
    loss, dl = run(logits, one, n, batch_dice, n)
    want, gwant = iref.loss_reference(logits, one, n, batch_dice, n, WEIGHT, SCALE)
    tol_value, e, mag = iref.loss_bounds(logits, one, n, batch_dice, n, WEIGHT, SCALE)
    assert abs(float(loss) - want) <= tol_value and not dl[1].any() and dl[0, ..., :n].any()
    assert ((dl[..., :n].double() - gwant).abs() <= e * mag + U16 * gwant.abs() * (1 + e) + SUB16)[0].all()


def test_bad_labels_and_refusals(lib):
    logits, target = loss_case(3, 2, 15, 13, 960)
    bad = target.clone()
    spot = tuple(int(v) for v in (target != 3).nonzero()[0])
    bad[spot] = 200                                                     # neither a class nor the ignore label
    for tgt in (bad, bad.to(torch.uint8)):
        loss, dl = run(logits, tgt, 3, True, 3)
        assert math.isnan(float(loss)) and dl[spot][:3].isnan().all() and not dl[spot][3:].any()
        assert torch.equal(dl[target == 3], torch.zeros_like(dl[target == 3]))
    neg = target.clone()
    neg[spot] = -1                                                      # an int64 label outside a byte's range is no class either
    assert math.isnan(float(run(logits, neg, 3, False, 3)[0]))
    assert math.isnan(float(run(logits, target, 3, True, None)[0])), "without the keyword the label 3 keeps today's meaning"
    for k in (2, 255, 3.5, True):
        with pytest.raises(ValueError, match="ignore_label"):
            ag.dice_ce(logits.to(DEV), target.to(DEV), 3, True, ignore_label=k)
    z = logits.to(DEV).requires_grad_(True)
    plain, stored = ag.dice_ce(logits.to(DEV), target.to(DEV), 3, True, WEIGHT, SCALE, ignore_label=3)
    term = ag.DiceCeFn.apply(z, target.to(DEV), 3, True, WEIGHT, SCALE, 1e-5, 3)
    assert torch.equal(term, plain * WEIGHT)
    term.backward()
    assert torch.equal(z.grad, stored)


@pytest.mark.parametrize("n,hw,batch_dice", [(3, (15, 13), True), (3, (72, 64), False), (9, (48, 40), True), (9, (72, 64), False)])
def test_split_at_world_one_equals_the_one_call_entry(lib, n, hw, batch_dice):
    _split_at_world_one(n, 2, hw, batch_dice)


@pytest.mark.parametrize("batch_dice", [False, True])
@pytest.mark.parametrize("n,B,hw", [(4, 11, (15, 13)), (17, 11, (72, 64)), (32, 9, (15, 13))])
def test_split_at_world_one_where_the_finalize_wraps(lib, n, B, hw, batch_dice):
    """WRAP_CASES' batches through the split entries: every row of the sums table carries its sample's exact label histogram over annotated pixels and its
    annotated count (the reduce kernel's later passes write rows like the first), and from_sums on that table gives the one-call entry's bits."""
    _split_at_world_one(n, B, hw, batch_dice)


def _split_at_world_one(n, B, hw, batch_dice):
    logits, target = loss_case(n, B, hw[0], hw[1], 980 + n)
    NC = logits.shape[-1]
    rows = target.reshape(1 if batch_dice else B, -1)
    hist = torch.stack([(rows == c).sum(1) for c in range(n)], -1).double()
    for tgt in (target, target.to(torch.uint8)):
        one = run(logits, tgt, n, batch_dice, n)
        ld, td = logits.to(DEV), tgt.to(DEV)
        sums = ag.dice_ce_stats(ld, td, n, batch_dice, ignore_label=n)
        assert sums.shape == (1 if batch_dice else B, ag.dice_ce_nacc(n, n)) and sums.dtype == torch.float64
        assert float(sums[:, -1].sum()) == float((target != n).sum()) and float(sums[:, -2].sum()) == 0.0      # the annotated count, exactly; no bad label
        assert torch.equal(sums[:, 2 * NC:2 * NC + n].cpu(), hist) and torch.equal(sums[:, -1].cpu(), (rows != n).sum(1).double())   # row by row
        loss, dl = ag.dice_ce_from_sums(ld, td, n, batch_dice, sums, sums, 1, WEIGHT, SCALE, ignore_label=n)
        assert torch.equal(loss.cpu(), one[0]) and torch.equal(dl.cpu(), one[1])
        plain_rows = ag.dice_ce_stats(ld, torch.where(td == n, torch.zeros_like(td), td), n, batch_dice)
        assert plain_rows.shape[1] == sums.shape[1] - 1                                                       # the plain row keeps its width
    for kw in (dict(dice_sums=sums * 2, local_sums=sums, world=2), dict(dice_sums=sums.clone(), local_sums=sums, world=1)):   # the exchange is not built
        if batch_dice:
            with pytest.raises(NotImplementedError, match="ignore"):
                ag.dice_ce_from_sums(ld, td, n, batch_dice, weight=WEIGHT, grad_scale=SCALE, ignore_label=n, **kw)


# ---- 2. the trainer --------------------------------------------------------------------------------------------------------------------------------
def _trainer_inputs(seed=7, size=32, B=2):
    plans, ds = fixtures()
    spec = nnunet.network_spec(plans, "2d_reduced", ds)
    g = torch.Generator().manual_seed(seed)
    x = F.avg_pool2d(torch.randn((B, 3, size + 4, size + 4), generator=g), 5, 1) * 2.2
    targets = ref.label_maps(B, spec["n_heads"], size, spec["n_stages"] - 1, seed + 1)
    return spec, bool(plans["configurations"]["2d"]["batch_dice"]), x, targets


def test_trainer_without_ignored_pixels_equals_the_plain_trainer():
    spec, batch_dice, x, targets = _trainer_inputs()
    k = spec["n_heads"]
    sd = nnunet_train.initial_state_dict(spec, 7)
    a = nnunet_train.Trainer(spec, sd, batch_dice, 10, device=DEV, configuration="2d_reduced")
    b = nnunet_train.Trainer(spec, sd, batch_dice, 10, device=DEV, configuration="2d_reduced", ignore_label=k)
    d = nnunet_train.Trainer(spec, sd, batch_dice, 10, device=DEV, configuration="2d_reduced", ddp=True)                    # the three-phase step at world 1 ...
    c = nnunet_train.Trainer(spec, sd, batch_dice, 10, device=DEV, configuration="2d_reduced", ignore_label=k, ddp=True)   # ... and its ignore form
    for _ in range(2):
        la, lb, ld, lc = (t.train_step(x, targets) for t in (a, b, d, c))
        assert la == lb and ld == lc
    for one, other in ((a, b), (d, c)):
        assert all(torch.equal(p, q) for p, q in zip(one.params, other.params))
        bufs_a, bufs_o = one.state["sgd"]["momentum_buffer"], other.state["sgd"]["momentum_buffer"]
        assert set(bufs_a) == set(bufs_o) and all(torch.equal(bufs_a[i], bufs_o[i]) for i in bufs_a)
    assert any(not torch.equal(p.detach().cpu(), sd[name]) for name, p in zip(a.names, a.params))
    with pytest.raises(ValueError, match="ignore_label"):
        nnunet_train.Trainer(spec, sd, batch_dice, 10, device=DEV, ignore_label=k + 1)
    c.world = 2                                                                        # collectives done by hand for two trainers: not built with an ignore label
    with pytest.raises(NotImplementedError, match="ignore_label"):
        c.step_forward(x, targets)


def test_trainer_with_ignored_pixels():
    """About 30 % ignored.  The loss against the float64 restatement on the float64 network, within the whole-step yardstick (the fp16-storage model,
    factor M_CAP): the library's logits of a graded scale lie within d_i = M_CAP * max |fp16-storage model's logits - float64 logits| of the float64 ones
    (tests/test_gpu_nnunet_train.py's round-trip rule); per pixel the cross-entropy moves by at most 2 d (log-sum-exp and the picked logit by d each), a
    softmax value by the factor e^(2 d), so intersect and sum_pred by 2 d relative and dc = N / D <= 1 by 4 d to first order: |loss_i - loss64_i| <= 6 d_i
    (first order; d is about 1e-2, the second-order term is below 10 % of it and is covered by asserting 6.6 d).  validation_step's tp / fp / fn: a host
    count over annotated pixels of the trainer's own arg-max, exactly."""
    spec, batch_dice, x, targets = _trainer_inputs(seed=9)
    k = spec["n_heads"]
    targets = [iref.ignore_blobs(t, k, 0.3, 40 + i) for i, t in enumerate(targets)]
    sd = ref.synthetic_state_dict(spec, 9)
    tr = nnunet_train.Trainer(spec, sd, batch_dice, 10, device=DEV, configuration="2d_reduced", ignore_label=k)
    outs = tr.network(x)
    lib_loss = float(tr.loss(outs, [t.to(DEV) for t in targets]))
    torch.cuda.synchronize()
    leaves = {name: v.double() for name, v in sd.items()}
    with torch.no_grad():
        o64 = ref.forward_deep_supervision(leaves, spec, x.double(), 0.01, False)
        o16 = ref.forward_deep_supervision(leaves, spec, x.double(), 0.01, True)
    l64 = float(iref.deep_supervision_loss_ignore(o64, targets, tr.weights, batch_dice, k))
    bound = sum(w * 6.6 * M_CAP * (a - b).abs().max().item() for a, b, w in zip(o16, o64, tr.weights) if w != 0.0)
    print(f"[trainer ignore] loss lib {lib_loss:.6f} f64 {l64:.6f}: off by {abs(lib_loss - l64):.3e}, bound {bound:.3e}")
    assert abs(lib_loss - l64) <= bound
    # that yardstick is wide (the network's fp16 storage); the sharp statement is on the trainer's OWN logits: the weighted sum of the restatement over
    # them, within the kernels' derived value bounds -- which the plain loss with the ignored pixels read as background misses by far
    own = [o.detach().cpu() for o in outs]
    graded = [(o, t, w) for o, t, w in zip(own, targets, tr.weights) if w != 0.0]
    want = sum(w * iref.loss_reference(o, t, k, batch_dice, k, 1.0, 1.0)[0] for o, t, w in graded)
    tol = sum(w * iref.loss_bounds(o, t, k, batch_dice, k, 1.0, 1.0)[0] for o, t, w in graded) + 2 * len(graded) * U * abs(want)   # the terms are weighted and added in fp32
    plain = sum(w * iref.loss_reference(o, torch.where(t == k, torch.zeros_like(t), t), k, batch_dice, k + 1, 1.0, 1.0)[0] for o, t, w in graded)
    print(f"[trainer ignore] on its own logits: off by {abs(lib_loss - want):.3e}, bound {tol:.3e}; the plain loss is {abs(plain - want):.3e} away")
    assert abs(lib_loss - want) <= tol < abs(plain - want)
    v = tr.validation_step(x, [t.to(DEV) for t in targets])
    pred = tr.eval_logits(x).argmax(1).cpu()
    top, keep = targets[0], targets[0] != k
    for c in range(1, k):
        tp = int(((pred == c) & (top == c) & keep).sum())
        fp = int(((pred == c) & (top != c) & keep).sum())
        fn = int(((pred != c) & (top == c) & keep).sum())
        assert (int(v["tp_hard"][c - 1]), int(v["fp_hard"][c - 1]), int(v["fn_hard"][c - 1])) == (tp, fp, fn), c
    assert int((v["tp_hard"] + v["fn_hard"]).sum()) == int(((top != 0) & keep).sum()) and math.isfinite(v["loss"])
    first = tr.train_step(x, targets)
    assert math.isfinite(first) and abs(first - lib_loss) < 1e-6 and tr.state.get("skipped_steps", 0) == 0
    with pytest.raises(ValueError, match="label outside"):
        nnunet_train.Trainer(spec, sd, batch_dice, 10, device=DEV, configuration="2d_reduced").train_step(x, targets)   # without the keyword: today's meaning


# ---- 3. the store ----------------------------------------------------------------------------------------------------------------------------------
def test_device_build_with_an_ignore_label_equals_the_host_build():
    g = np.load(os.path.join(GOLDEN, "nnunet_class_locations_ignore.npz"))
    n = int(g["n_heads"])
    labels = {"background": 0, "a": 1, "b": 2, "ignore": n}
    rng = np.random.default_rng(12)
    cases = [(torch.from_numpy(rng.integers(1, 256, (3, 40, 36)).astype(np.uint8)), torch.from_numpy(g[f"{name}.seg"])) for name in ("a", "b")]
    schemes = ["ZScoreNormalization"] * 3
    host = nd.CaseStore(cases, schemes, n, device=DEV, labels=labels, build="host", crop=True)
    dev = nd.CaseStore([(i.to(DEV), s.to(DEV)) for i, s in cases], schemes, n, device=DEV, labels=labels, build="device")
    key = nd.annotated_key(n)
    assert host.boxes == dev.boxes == [(0, 40, 0, 36)] * 2 and host.ignore_label == dev.ignore_label == n
    for i, name in enumerate(("a", "b")):
        assert torch.equal(host.labels(i), dev.labels(i))
        assert list(host.class_locations[i]) == list(dev.class_locations[i]) == [1, 2, key]
        for c in (1, 2, key):
            hl, dl = host.class_locations[i][c], dev.class_locations[i][c]
            want = g[f"{name}.locations_{'annotated' if c == key else c}"][:, 2:]
            assert len(hl) == len(dl) == len(want) and (len(want) == 0 or (dl.dtype == hl.dtype and np.array_equal(hl, dl) and np.array_equal(dl, want))), (i, c)
    assert len(dev.class_locations[0][key]) == int((g["a.seg"] < n).sum()) > 0 and len(dev.class_locations[1][key]) == 0
    a, b = next(nd.PatchLoader(host, (16, 16), 4, 2, seed=5, train=True)), next(nd.PatchLoader(dev, (16, 16), 4, 2, seed=5, train=True))
    assert all(torch.equal(p, q) for p, q in zip(a["target"], b["target"])) and int(a["target"][0].max()) <= n
    bad = cases[0][1].clone()
    bad[0, 0] = n + 1
    with pytest.raises(ValueError, match=rf"labels \[{n + 1}\] outside"):
        nd.CaseStore([(cases[0][0].to(DEV), bad.to(DEV))], schemes, n, device=DEV, labels=labels, build="device")
    # the new selector through the public wrappers: `label < n` is selector -1 - n, its prefix the sum of the classes' rows
    seg = cases[0][1].to(DEV)
    _, prefix, totals = nd.case_counts(seg, (0, 40, 0, 36), n)
    classes = prefix[:n].sum(0, dtype=torch.int32).contiguous()
    ranks = torch.arange(int(classes[-1]), device=DEV)
    coords, _ = nd.case_rank_to_coord(seg, (0, 40, 0, 36), -1 - n, classes, ranks)
    assert np.array_equal(coords.cpu().numpy(), np.argwhere(g["a.seg"] < n)) and int(totals[:n].sum()) == int(classes[-1])


# ---- 4. the stage ----------------------------------------------------------------------------------------------------------------------------------
def test_stage_with_an_ignored_grey_level(tmp_path, monkeypatch):
    """Six 64 x 64 images (nnU-Net's five-fold split refuses fewer than five cases; six is tests/test_gpu_nnunet_prep.py's count) whose labels leave a
    band unlabelled (grey level 25) through Segmentor.train_tissue_model_nnUNetv2(ignore_pixel=25), one epoch of two iterations (that test's setting);
    the written folder loads and inference_tissue_model_nnUNetv2 returns a mask without 7."""
    from PIL import Image
    import test_gpu_models as tgm
    from ldiffusion_amd import configs, utils, weights
    from ldiffusion_amd.segmentor import Segmentor
    rng = np.random.RandomState(31)
    levels = np.array(sorted(metrics.PIXEL_TO_LABEL), np.uint8)
    assert 25 not in metrics.PIXEL_TO_LABEL
    src = tmp_path / "src"
    src.mkdir()
    images, labels = [], []
    for i in range(6):
        Image.fromarray(rng.randint(1, 256, (64, 64, 3)).astype(np.uint8)).save(src / f"im{i}.png")
        lab = levels[np.kron(rng.randint(0, 7, (8, 8)), np.ones((8, 8), np.int64))]
        lab[:, 20 + 3 * i:44] = 25
        Image.fromarray(lab).save(src / f"lb{i}.png")
        images.append(str(src / f"im{i}.png"))
        labels.append(str(src / f"lb{i}.png"))
    for name in ("nnUNet_raw", "nnUNet_preprocessed", "nnUNet_results"):
        (tmp_path / name).mkdir()
        monkeypatch.setenv(name, str(tmp_path / name))
    monkeypatch.setattr(Segmentor, "load_ldiffusion", lambda self, w, p, **kw: (None, None, None))
    monkeypatch.setattr(utils, "check_images_same_size", lambda paths: False)      # plain copies: no sampler runs (the existing stage tests use mixed sizes for this)
    seg = Segmentor(None, None, "tissue", 7)
    folder = seg.train_tissue_model_nnUNetv2(1, "weights", "sd", images, labels, images[:2], labels[:2], iterations_per_epoch=2, val_iterations=1,
                                             num_foreground_voxels=6e4, ignore_pixel=25)
    monkeypatch.undo()
    raw = tmp_path / "nnUNet_raw" / "Dataset001_Custom"
    assert json.loads((raw / "dataset.json").read_text())["labels"]["ignore"] == 7
    written = np.array(Image.open(raw / "labelsTr" / "case_000.png"))
    assert (written[:, 20:44] == 7).all() and written.max() == 7
    assert json.loads(open(os.path.join(folder, "dataset.json")).read())["labels"]["ignore"] == 7
    ckpt = torch.load(os.path.join(folder, "fold_0", "checkpoint_final.pth"), map_location="cpu", weights_only=False)
    assert ckpt["init_args"]["configuration"] == "2d" and ckpt["init_args"]["dataset_json"]["labels"]["ignore"] == 7
    log = seg.training_log
    assert len(log["train_losses"]) == 1 and np.isfinite(log["train_losses"]).all() and np.isfinite(log["val_losses"]).all()
    assert all(nd.annotated_key(7) in cl for cl in seg.tissue_loaders[0].store.class_locations)
    head = nnunet.load_trained_model_folder(folder, device=DEV)
    assert head.num_heads == 7 and head.spec["ignore_label"] == 7
    tiny = dict(ucfg=configs.TINY_UNET, vcfg=configs.TINY_VAE, usd=weights.synthetic_state_dict(weights.unet_param_shapes(configs.TINY_UNET), 42, fp16_values=True),
                vsd=weights.synthetic_state_dict(weights.vae_param_shapes(configs.TINY_VAE), 43, fp16_values=True))
    sd_dir, w_dir, _ = tgm._write_sd_dirs(tmp_path, tiny, torch.float32, torch.float32)
    rect = tmp_path / "rect.png"                                                     # not square: the image goes to the head as it is
    Image.fromarray(rng.randint(1, 256, (64, 48, 3)).astype(np.uint8)).save(rect)
    _, mask = Segmentor(None, None, "tissue", 7).inference_tissue_model_nnUNetv2(str(rect), str(sd_dir), str(w_dir), folder)
    assert mask.shape == (64, 48) and mask.dtype == np.uint8 and int(mask.max()) < 7
