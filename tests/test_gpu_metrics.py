"""-m gpu: mask scoring on the device -- `ldiff_confusion` through the C ABI and through ldiffusion_amd.metrics / utils / evaluate / Segmentor.

The result is an integer matrix, so every comparison of counts is EXACT equality against a numpy `bincount` of the same inputs.  The metrics derived
from it are compared with the reference's recorded values (tests/golden/reference_metrics.json) and with oracle/metrics.py at the tolerances
tests/test_cpu_oracle.py uses against the same file: 1e-7 where the reference computes in float32 (Dice, frequency-weighted IoU), 1e-12 where it
computes in double (mean IoU, pixel accuracy).

Which counting path a pattern takes (kernels_metrics.hip): a constant image keeps every wave on the uniform path (one lane adds the lane count), a
left / right split at an odd column mixes uniform and divergent waves, a checkerboard makes every 16-pixel run of a lane non-flat while whole pixel
slots stay uniform across a row, and uniform random labels leave only the LDS atomic path."""
import os

import numpy as np
import pytest
import torch

from ldiffusion_amd import _lib, evaluate as lev, metrics, utils as lutils
from ldiffusion_amd.pipeline import argmax_mask
from ldiffusion_amd.segmentor import Segmentor
from oracle import metrics as om
from metrics_ref import check_against_fixture, fixture_cases, numpy_confusion

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def expected(pred, target, n):
    """(conf [B, n, n], dropped [B]) of label arrays [B, H, W] (any integer type) by numpy."""
    pred, target = np.asarray(pred), np.asarray(target)
    conf = np.stack([numpy_confusion(p, t, n) for p, t in zip(pred, target)])
    return conf, np.array([p.size for p in pred], np.int64) - conf.sum((1, 2))


def c_confusion(lib, pred, target, n, pred_lut=None, target_lut=None, conf=None, dropped=None):
    """One `ldiff_confusion` call on device tensors, straight through the C ABI; returns (conf, dropped) as numpy."""
    B, H, W = pred.shape[0], pred.shape[-2], pred.shape[-1]
    kind = 0 if pred.dtype == torch.uint8 else 1 if pred.dtype == torch.float32 else 2
    conf = torch.zeros((B, n, n), dtype=torch.int64, device=pred.device) if conf is None else conf
    dropped = torch.zeros(B, dtype=torch.int64, device=pred.device) if dropped is None else dropped
    _lib.check(lib.ldiff_confusion(_lib.ptr(pred), kind, _lib.ptr(target), 0 if target.dtype == torch.uint8 else 1, _lib.ptr(pred_lut), _lib.ptr(target_lut),
                                   B, n, H, W, _lib.ptr(conf), _lib.ptr(dropped), _lib.stream_ptr()))
    return conf.cpu().numpy(), dropped.cpu().numpy()


# ---------------------------------------------------------------- the reference's recorded cases, in logit form
def test_fixture_cases_on_the_device_match_the_reference(lib):
    seg = Segmentor(None, None, "tissue", 7)
    for c, logits, target in fixture_cases():
        n = c["shape"][1]
        x, t = logits.to(DEV), target.to(DEV)
        conf = metrics.confusion_matrix(x, t, n).cpu().numpy()
        want, _ = expected(torch.argmax(logits, 1).numpy(), target.numpy(), n)
        assert np.array_equal(conf, want), c["shape"]
        check_against_fixture(c, metrics.from_confusion(conf))
        # the reference-named entry points against the recorded values, and against the oracle's restatement of the same functions
        o_per, o_avg = om.micro_dice(logits, target, n)
        o_miou, o_iou = om.mean_iou_and_per_class(logits, target, n)
        o_pa, o_pal = om.pixel_accuracy(logits, target, n)
        o_fw = om.frequency_weighted_iou(logits, target, n)
        for fn in (lutils.micro_dice, seg.micro_dice):
            per, avg = fn(x, t, num_classes=n)
            assert per.dtype == torch.float32 and tuple(per.shape) == (n,) and avg.dim() == 0
            assert per.tolist() == pytest.approx(c["dice_per_class"], abs=1e-7) and float(avg) == pytest.approx(c["dice"], abs=1e-7)
            assert per.tolist() == pytest.approx(o_per.tolist(), abs=1e-7) and float(avg) == pytest.approx(float(o_avg), abs=1e-7)
        miou, iou = lutils.mean_iou_and_per_class(x, t, n)
        assert isinstance(miou, float) and miou == pytest.approx(c["miou"], abs=1e-12) and miou == pytest.approx(o_miou, abs=1e-12)
        assert {str(k): v for k, v in iou.items() if v is None} == {k: v for k, v in c["iou_per_class"].items() if v is None}
        assert {k for k, v in iou.items() if v is None} == {k for k, v in o_iou.items() if v is None}
        for k, v in o_iou.items():
            assert v is None or (iou[k] == pytest.approx(v, abs=1e-12) and iou[k] == pytest.approx(c["iou_per_class"][str(k)], abs=1e-12))
        pa, pal = lev.pixel_accuracy(x, t, n)
        assert pa == pytest.approx(c["pixel_accuracy"], abs=1e-12) and pa == pytest.approx(o_pa, abs=1e-12) and pal == pytest.approx(o_pal, abs=1e-12)
        fw = lev.frequency_weighted_iou(x, t, n)
        assert fw == pytest.approx(c["fw_iou"], abs=1e-7) and fw == pytest.approx(o_fw, abs=1e-7)
        assert lev.frequency_weighted_iou(x, t, n, ignore_background=True) == pytest.approx(metrics.from_confusion(conf).fw_iou_fg, abs=0)


# ---------------------------------------------------------------- shapes x class counts x patterns, mask form, through the C ABI
SHAPES = [(1, 4, 4), (3, 5, 5), (2, 17, 23), (1, 64, 64), (2, 512, 512)]   # the last: several workgroups flush into one matrix
PATTERNS = ["constant", "split", "checkerboard", "random"]


def pattern(name, B, H, W, n, seed):
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    if name == "constant":
        p, t = np.full((B, H, W), n - 1), np.full((B, H, W), (n - 1) // 2)
    elif name == "split":
        col = (W // 2) | 1                                  # an odd column: no 16-pixel run lines up with it
        p = np.broadcast_to(np.where(xx < col, 0, n - 1), (B, H, W))
        t = np.broadcast_to(np.where(xx < col, (n - 1) // 2, 0), (B, H, W))
    elif name == "checkerboard":
        p = np.broadcast_to(((xx + yy) & 1) * (n - 1), (B, H, W))
        t = np.broadcast_to(((xx + yy + 1) & 1) * min(1, n - 1), (B, H, W))
    else:
        rng = np.random.default_rng(seed)
        p, t = rng.integers(0, n + 1, (B, H, W)), rng.integers(0, n + 1, (B, H, W))   # n itself is no class: those pixels are dropped
    return np.ascontiguousarray(p, dtype=np.uint8), np.ascontiguousarray(t, dtype=np.uint8)


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("n", [1, 2, 7, 11, 32])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mask_form_shape_and_pattern_grid(lib, shape, n, name):
    B, H, W = shape
    p, t = pattern(name, B, H, W, n, seed=B * H * W + n)
    want_conf, want_drop = expected(p, t, n)
    conf, drop = c_confusion(lib, torch.from_numpy(p).to(DEV), torch.from_numpy(t).to(DEV), n)
    assert np.array_equal(conf, want_conf) and np.array_equal(drop, want_drop)
    assert conf.sum() + drop.sum() == B * H * W
    if name != "random":
        assert drop.sum() == 0


# ---------------------------------------------------------------- views that start off every boundary
@pytest.mark.parametrize("shape", [(2, 17, 23), (1, 64, 64), (2, 96, 100)], ids=lambda s: "x".join(map(str, s)))
def test_misaligned_views_give_identical_matrices(lib, shape):
    B, H, W = shape
    n, N = 7, B * H * W
    rng = np.random.default_rng(7)
    p = rng.integers(0, n + 1, N).astype(np.uint8)
    p[: N // 3] = 2                                                    # a constant stretch: the flat path sees misaligned heads too
    t = rng.integers(0, n, N).astype(np.uint8)
    want = expected(p.reshape(shape), t.reshape(shape), n)
    for po, to in [(0, 0), (1, 1), (3, 3), (1, 3), (3, 0)]:            # equal phase: 16-byte body; unequal: the scalar walk
        pb, tb = torch.zeros(N + 3, dtype=torch.uint8, device=DEV), torch.zeros(N + 3, dtype=torch.uint8, device=DEV)
        pb[po:po + N] = torch.from_numpy(p).to(DEV)
        tb[to:to + N] = torch.from_numpy(t).to(DEV)
        pv, tv = pb[po:po + N].view(shape), tb[to:to + N].view(shape)
        assert pv.data_ptr() % 16 == po and tv.data_ptr() % 16 == to and pv.is_contiguous()
        got = c_confusion(lib, pv, tv, n)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (po, to)
        assert np.array_equal(metrics.confusion_matrix(pv, tv, n).cpu().numpy(), want[0]), (po, to)
    # logits that start 1 and 3 elements into their buffer (4 / 12 bytes for float32, 2 / 6 for float16), labels as int64
    g = torch.Generator().manual_seed(3)
    x = torch.randn((B, n, H, W), generator=g)
    t64 = torch.from_numpy(t.reshape(shape).astype(np.int64)).to(DEV)
    for dtype in (torch.float32, torch.float16):
        xd = x.to(dtype)
        want_x = expected(torch.argmax(xd.float(), 1).numpy(), t.reshape(shape), n)[0]
        for off in (0, 1, 3):
            buf = torch.zeros(xd.numel() + 3, dtype=dtype, device=DEV)
            buf[off:off + xd.numel()] = xd.reshape(-1).to(DEV)
            got = metrics.confusion_matrix(buf[off:off + xd.numel()].view(xd.shape), t64, n).cpu().numpy()
            assert np.array_equal(got, want_x), (dtype, off)


# ---------------------------------------------------------------- logit form == mask form of the library's own arg-max
def special_logits(B, n, H, W, seed, class0_only):
    """Random logits with ties, NaN, +inf and -inf pixels.  class0_only: NaN and +inf sit in class 0 only, where `torch.argmax` (first NaN, first
    maximum) and the library's rule (any NaN or +inf logit -> class 0) name the same class."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, n, H, W), generator=g)
    x = (x * 4).round() / 4                                            # quarter steps: exact in float16, ties among the maxima are common
    flat = x.permute(0, 2, 3, 1).reshape(-1, n)                        # [pixels, n]
    pix = torch.randperm(flat.shape[0], generator=g)
    k = max(4, flat.shape[0] // 16)
    for j, val in enumerate((float("nan"), float("inf"), float("-inf"))):
        rows = pix[j * k:(j + 1) * k]
        cols = torch.randint(0, n, (k,), generator=g)
        if class0_only and val != float("-inf"):
            cols = torch.zeros(k, dtype=torch.long)
        flat[rows, cols] = val
    rows = pix[3 * k:4 * k]
    flat[rows, 1:] = flat[rows, :1]                                    # every class ties: the first one wins
    flat[pix[4 * k:5 * k]] = float("-inf")                             # all -inf: class 0
    return flat.reshape(B, H, W, n).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("shape", [(2, 7, 32, 40), (2, 7, 17, 23), (1, 11, 50, 50), (3, 2, 9, 8), (1, 32, 24, 24)], ids=lambda s: "x".join(map(str, s)))
def test_logit_form_equals_mask_form_of_ldiff_argmax_u8(lib, shape):
    B, n, H, W = shape                                                 # H W a multiple of 8 / of 4 only / of neither: 16-byte and one-pixel plane loads
    rng = np.random.default_rng(11)
    t = torch.from_numpy(rng.integers(0, n, (B, H, W)).astype(np.uint8)).to(DEV)
    x = special_logits(B, n, H, W, seed=5, class0_only=False)
    assert torch.isnan(x).any() and torch.isinf(x).any()
    xd = x.to(DEV)
    mask = argmax_mask(xd)                                             # ldiff_argmax_u8
    want = c_confusion(lib, mask, t, n)
    assert np.array_equal(want[0], expected(mask.cpu().numpy(), t.cpu().numpy(), n)[0]) and want[1].sum() == 0
    got = c_confusion(lib, xd, t, n)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # float16 logits follow the same rule (widened to float32 first) ...
    got16 = c_confusion(lib, xd.half(), t, n)
    mask16 = argmax_mask(xd.half().float())
    assert np.array_equal(got16[0], c_confusion(lib, mask16, t, n)[0]) and got16[1].sum() == 0
    # ... and equal torch.argmax(x.float(), 1) on inputs where the two rules name the same class
    y = special_logits(B, n, H, W, seed=6, class0_only=True).half()
    assert torch.isnan(y).any() and torch.isinf(y).any()
    ref = torch.argmax(y.float(), 1).numpy()
    assert np.array_equal(c_confusion(lib, y.to(DEV), t, n)[0], expected(ref, t.cpu().numpy(), n)[0])
    assert np.array_equal(c_confusion(lib, y.float().to(DEV), t, n)[0], expected(ref, t.cpu().numpy(), n)[0])


# ---------------------------------------------------------------- targets
def test_uint8_and_int64_targets_and_what_is_dropped(lib):
    B, H, W, n = 2, 37, 41, 7
    rng = np.random.default_rng(21)
    p = rng.integers(0, n, (B, H, W)).astype(np.uint8)
    t = rng.integers(0, n, (B, H, W)).astype(np.uint8)
    pd = torch.from_numpy(p).to(DEV)
    a = c_confusion(lib, pd, torch.from_numpy(t).to(DEV), n)
    b = c_confusion(lib, pd, torch.from_numpy(t.astype(np.int64)).to(DEV), n)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], expected(p, t, n)[0]) and a[1].sum() == 0 and b[1].sum() == 0
    # int64 labels that are no class: -1, C, 255, 2^40 -- each lands in `dropped`, exactly, and nowhere else
    t64 = t.astype(np.int64)
    bad = {(0, 0, 0): -1, (0, 5, 7): n, (0, 36, 40): 255, (1, 0, 1): 1 << 40, (1, 20, 20): -(1 << 40), (1, 36, 40): n}
    for pos, v in bad.items():
        t64[pos] = v
    conf, drop = c_confusion(lib, pd, torch.from_numpy(t64).to(DEV), n)
    want_conf, want_drop = expected(p, t64, n)
    assert want_drop.tolist() == [3, 3]
    assert np.array_equal(conf, want_conf) and np.array_equal(drop, want_drop)
    # ... in logit form too
    x = torch.randn((B, n, H, W), generator=torch.Generator().manual_seed(2))
    conf, drop = c_confusion(lib, x.to(DEV), torch.from_numpy(t64).to(DEV), n)
    assert np.array_equal(conf, expected(torch.argmax(x, 1).numpy(), t64, n)[0]) and drop.tolist() == [3, 3]
    # uint8 target 255 (the usual "ignore" label) at C = 7, and mask predictions >= C
    t8, p8 = t.copy(), p.copy()
    t8[0, :3] = 255
    p8[1, 10:12] = n
    p8[1, 30, 3] = 200
    p8[0, 0, 0] = 9                                                    # a pixel where both are no class is dropped once
    conf, drop = c_confusion(lib, torch.from_numpy(p8).to(DEV), torch.from_numpy(t8).to(DEV), n)
    want_conf, want_drop = expected(p8, t8, n)
    assert want_drop.tolist() == [3 * W, 2 * W + 1]
    assert np.array_equal(conf, want_conf) and np.array_equal(drop, want_drop)
    # the python surface: dropped is optional, an int32 target is widened, a LUT with an int64 target is refused
    assert np.array_equal(metrics.confusion_matrix(torch.from_numpy(p8).to(DEV), torch.from_numpy(t8.astype(np.int32)).to(DEV), n).cpu().numpy(), want_conf)
    lut = metrics.label_lut("tissue").to(DEV)
    with pytest.raises(ValueError):
        metrics.confusion_matrix(pd, torch.from_numpy(t64).to(DEV), n, target_lut=lut)
    with pytest.raises(ValueError):
        metrics.confusion_matrix(pd, torch.from_numpy(t64).to(DEV), n, pred_lut=lut)
    with pytest.raises(ValueError):
        metrics.confusion_matrix(x.to(DEV), torch.from_numpy(t).to(DEV), n, pred_lut=lut)   # a prediction LUT needs the mask form
    for bad_n in (0, 33):
        with pytest.raises(ValueError):
            metrics.confusion_matrix(pd, torch.from_numpy(t).to(DEV), bad_n)


# ---------------------------------------------------------------- LUTs
@pytest.mark.parametrize("level,n", [("tissue", 7), ("cell", 11), ("tissue", 4)])
def test_grey_level_images_through_the_label_luts(lib, level, n):
    B, H, W = 2, 45, 31
    lut = metrics.label_lut(level)
    levels = np.array([g for g in range(256) if lut[g] != 0] + [0, 0, 0, 7, 33, 99, 254], np.uint8)   # the table's levels, and some outside it
    rng = np.random.default_rng(31)
    tg, pg = rng.choice(levels, (B, H, W)), rng.choice(levels, (B, H, W))
    tg[0, :10] = levels[1]                                             # a constant region through the LUT
    pg[0, :10] = levels[2]
    l = lut.numpy()
    want_conf, want_drop = expected(l[pg], l[tg], n)                   # the host-mapped labels; tissue at C = 4: labels 4..6 are dropped
    assert (want_drop.sum() > 0) == (n == 4)
    ld = lut.to(DEV)
    conf, drop = c_confusion(lib, torch.from_numpy(pg).to(DEV), torch.from_numpy(tg).to(DEV), n, pred_lut=ld, target_lut=ld)
    assert np.array_equal(conf, want_conf) and np.array_equal(drop, want_drop)
    # one LUT only: the other operand already holds class ids
    conf, drop = c_confusion(lib, torch.from_numpy(l[pg]).to(DEV), torch.from_numpy(tg).to(DEV), n, target_lut=ld)
    assert np.array_equal(conf, want_conf) and np.array_equal(drop, want_drop)
    conf = metrics.confusion_matrix(torch.from_numpy(pg).to(DEV), torch.from_numpy(l[tg]).to(DEV), n, pred_lut=lut).cpu().numpy()   # a host LUT is uploaded
    assert np.array_equal(conf, want_conf)
    # a target LUT beside logits
    x = torch.randn((B, n, H, W), generator=torch.Generator().manual_seed(4))
    conf, drop = c_confusion(lib, x.to(DEV), torch.from_numpy(tg).to(DEV), n, target_lut=ld)
    assert np.array_equal(conf, expected(torch.argmax(x, 1).numpy(), l[tg], n)[0])


# ---------------------------------------------------------------- the call adds
def test_accumulation_and_reproducibility(lib):
    B, H, W, n = 2, 130, 129, 7
    rng = np.random.default_rng(41)
    p1, t1, p2, t2 = (torch.from_numpy(rng.integers(0, n + 1, (B, H, W)).astype(np.uint8)).to(DEV) for _ in range(4))
    w1, w2 = expected(p1.cpu().numpy(), t1.cpu().numpy(), n), expected(p2.cpu().numpy(), t2.cpu().numpy(), n)
    init = torch.arange(B * n * n, dtype=torch.int64, device=DEV).view(B, n, n) * 1000 + (1 << 33)    # beyond 32 bits: the adds are 64-bit
    conf, drop = init.clone(), torch.full((B,), 5, dtype=torch.int64, device=DEV)
    metrics.confusion_matrix(p1, t1, n, out=conf, dropped=drop)
    got = metrics.confusion_matrix(p2, t2, n, out=conf, dropped=drop)
    assert got is conf
    assert np.array_equal(conf.cpu().numpy(), init.cpu().numpy() + w1[0] + w2[0]) and np.array_equal(drop.cpu().numpy(), 5 + w1[1] + w2[1])
    a = metrics.confusion_matrix(p1, t1, n)
    b = metrics.confusion_matrix(p1, t1, n)
    assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), w1[0])                              # the same launch again: bitwise identical
    # an empty batch enqueues nothing and leaves the matrix alone
    e = metrics.confusion_matrix(torch.zeros((2, 0, 5), dtype=torch.uint8, device=DEV), torch.zeros((2, 0, 5), dtype=torch.uint8, device=DEV), n, out=conf)
    assert np.array_equal(e.cpu().numpy(), init.cpu().numpy() + w1[0] + w2[0])


# ---------------------------------------------------------------- evaluate()
def reference_fg_means(pred, gt, n):
    """evaluate.py:67-93 for one pair with the oracle's restatements: the foreground means of the four metrics and the per-class rows."""
    onehot = torch.nn.functional.one_hot(torch.from_numpy(pred).long()[None], num_classes=n).permute(0, 3, 1, 2).float()
    g = torch.from_numpy(gt).long()[None]
    per, _ = om.micro_dice(onehot, g, n)
    _, iou = om.mean_iou_and_per_class(onehot, g, n)
    vals = [iou[c] for c in range(1, n) if iou[c] is not None]
    _, pal = om.pixel_accuracy(onehot, g, n)
    hist = torch.from_numpy(numpy_confusion(pred, gt, n)).float()       # evaluate.py:32-45 with ignore_background=True
    freq = hist.sum(1) / hist.sum()
    iu = torch.diag(hist) / (hist.sum(1) + hist.sum(0) - torch.diag(hist) + 1e-10)
    return (torch.mean(per[1:]).item(), sum(vals) / len(vals) if vals else 1.0, float(np.mean(pal[1:])), (freq[1:] * iu[1:]).sum().item(),
            per[1:].numpy(), [iou[c] if iou[c] is not None else 1.0 for c in range(1, n)], pal[1:])


def test_evaluate_scores_png_pairs_like_the_reference(lib, tmp_path):
    from PIL import Image
    n = 5
    rng = np.random.default_rng(51)
    img_dir, lbl_dir, out_dir = tmp_path / "pred", tmp_path / "gt", tmp_path / "report"
    img_dir.mkdir(), lbl_dir.mkdir()
    pairs = []
    for i, (H, W) in enumerate([(40, 56), (33, 47), (40, 56)]):        # two sizes: two batches
        gt = rng.integers(0, n, (H, W)).astype(np.uint8)
        pred = np.where(rng.random((H, W)) < 0.7, gt, rng.integers(0, n, (H, W))).astype(np.uint8)
        if i == 1:
            gt[gt == 4] = 0
            pred[pred == 4] = 0                                        # class 4 absent from this pair: Dice 1, IoU None -> 1.0 in the per-class row
        Image.fromarray(pred).save(img_dir / f"im{i}.png")
        Image.fromarray(gt).save(lbl_dir / f"im{i}.png")
        pairs.append((pred, gt))
    got = lev.evaluate(str(img_dir), str(lbl_dir), n, str(out_dir))
    ref = [reference_fg_means(p, g, n) for p, g in pairs]
    assert set(got) == {"dice", "iou", "pa", "fwiou"}
    assert got["dice"] == pytest.approx(np.mean([r[0] for r in ref]), abs=1e-7) and got["fwiou"] == pytest.approx(np.mean([r[3] for r in ref]), abs=1e-7)
    assert got["iou"] == pytest.approx(np.mean([r[1] for r in ref]), abs=1e-12) and got["pa"] == pytest.approx(np.mean([r[2] for r in ref]), abs=1e-12)
    reports = sorted(os.listdir(out_dir))
    assert len(reports) == 1 and reports[0].startswith("metrics_") and reports[0].endswith(".txt")
    lines = open(out_dir / reports[0]).read().split("\n")
    pc = [np.mean([r[k] for r in ref], axis=0) for k in (4, 5, 6)]
    assert lines == ["=== Segmentation Evaluation Results ===", f"Image dir: {img_dir}", f"Label dir: {lbl_dir}", f"Classes: {n}", "", "The number of images: 3", "",
                     f"Mean Dice:  {got['dice']:.4f}", f"Mean IoU:   {got['iou']:.4f}", f"Mean PA:    {got['pa']:.4f}", f"Mean FWIoU: {got['fwiou']:.4f}", "",
                     "Per-class metrics:"] + [f"Class {c}: Dice={pc[0][c - 1]:.4f}, IoU={pc[1][c - 1]:.4f}, PA={pc[2][c - 1]:.4f}" for c in range(1, n)] + [""]
    # labels outside [0, n) are in no cell of the matrix: evaluate says so instead of hiding them
    ign_img, ign_lbl = tmp_path / "pred_ign", tmp_path / "gt_ign"
    ign_img.mkdir(), ign_lbl.mkdir()
    gt = pairs[0][1].copy()
    gt[:2] = 255
    Image.fromarray(pairs[0][0]).save(ign_img / "a.png")
    Image.fromarray(gt).save(ign_lbl / "a.png")
    with pytest.warns(UserWarning, match=f"{2 * 56} pixels in 1 label images"):
        lev.evaluate(str(ign_img), str(ign_lbl), n, str(tmp_path / "report_ign"))
    # the reference's two refusals
    Image.fromarray(pairs[0][0]).save(img_dir / "im3.png")
    with pytest.raises(ValueError, match="must be equal"):
        lev.evaluate(str(img_dir), str(lbl_dir), n, str(out_dir))
    Image.fromarray(pairs[1][1]).save(lbl_dir / "im3.png")             # a (33, 47) label beside a (40, 56) prediction
    with pytest.raises(ValueError):
        lev.evaluate(str(img_dir), str(lbl_dir), n, str(out_dir))
    assert len(os.listdir(out_dir)) == 1
