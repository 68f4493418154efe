"""-m gpu: training data of the tissue head on the device -- ldiff_op_seg_sample and ldiff_op_seg_intensity against the float64 restatements of
tests/nnunet_data_ref.py (pinned to scipy by tests/test_cpu_nnunet_data.py) within the bounds derived there, and PatchLoader feeding nnunet_train.Trainer.

Stores: three cases with C = 3 (40 x 56; 33 x 47, odd strides; 24 x 24, smaller than the patch), and one 40 x 56 case with C = 1.  Patches 32 x 32
(three scales) and 30 x 34 (two scales).  One batch of eight samples covers the integer crop hanging over two borders, mirrored copies, rotation + scale
+ mirror, a window about half outside, a window wholly outside, and a case smaller than the patch in both modes."""
import json
import math
import os

import numpy as np
import pytest
import torch

import nnunet_data_ref as ref
from ldiffusion_amd import nnunet, nnunet_train
from ldiffusion_amd import nnunet_data as nd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
SCHEMES = ["ZScoreNormalization", "RescaleTo01Normalization", "NoNormalization"]
N_HEADS = 4
PATCHES = [((32, 32), 3), ((30, 34), 2)]
# pixels of the batch below whose label vote has a weight within 1e-3 of 0.5 in the float64 restatement (counted on the CPU; 8 x 1024 and 8 x 1020 pixels)
NEAR_HALF = {(32, 32): 4, (30, 34): 4}


def blob_labels(H, W, seed):
    """A four-label map of smooth blobs: thresholds of a low-pass random field."""
    g = torch.Generator().manual_seed(seed)
    f = torch.nn.functional.avg_pool2d(torch.randn((1, 1, H + 8, W + 8), generator=g), 9, 1)[0, 0]
    f = (f - f.mean()) / f.std()
    return (torch.bucketize(f, torch.tensor([-0.6, 0.2, 0.9]))).to(torch.uint8).numpy()


def make_cases(shapes, C, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, (H, W) in enumerate(shapes):
        img = torch.nn.functional.avg_pool2d(torch.randn((1, C, H + 2, W + 2), generator=g), 3, 1)[0] * 60 + 120
        img = img.clamp(0, 255)
        out.append((img.to(torch.uint8) if i == 0 else img.float(), blob_labels(H, W, seed + 10 + i)))
    return out


def batch_table(patch):
    """Eight hand-made samples (the rules are draw_batch's: spatial_matrix builds every row)."""
    h, w = patch
    rows = [  # case, loader crop's first index, angle, zoom, flip, modified
        (0, (-5, 40), 0.0, 1.0, (False, False), False),      # integer crop over the top and right borders
        (1, (10, -6), 0.0, 1.0, (True, True), False),        # mirrored copy over the bottom and left borders of the odd-stride case
        (0, (4, 12), 0.7, 0.8, (True, False), True),         # rotation + scale + mirror, inside
        (1, (14, 28), -2.3, 1.3, (False, True), True),       # about half outside
        (2, (-120, -90), 1.1, 1.2, (False, False), True),    # wholly outside
        (2, (-4, -4), 2.9, 0.75, (False, False), True),      # the case smaller than the patch, resampled
        (2, (-3, -5), 0.0, 1.0, (False, True), False),       # ... and copied
        (0, (6, 20), 0.0, 1.37, (False, False), True),       # scale alone
    ]
    s = np.zeros(len(rows), nd.SAMPLE_DTYPE)
    for i, (case, lb, angle, zoom, flip, modified) in enumerate(rows):
        s[i]["case_index"] = case
        s[i]["m"], s[i]["copy"] = nd.spatial_matrix((h, w), (h, w), lb, angle, zoom, flip, modified)
    return s


@pytest.fixture(scope="module")
def store3():
    return nd.CaseStore(make_cases([(40, 56), (33, 47), (24, 24)], 3, 100), SCHEMES, N_HEADS, DEV)


@pytest.fixture(scope="module")
def store1():
    return nd.CaseStore(make_cases([(40, 56)], 1, 200), SCHEMES[:1], N_HEADS, DEV)


@pytest.fixture(scope="module")
def sampled(store3):
    """One launch per patch shape and its float64 reference, shared by the sampling, label and target tests."""
    out = {}
    for patch, n_scales in PATCHES:
        table = batch_table(patch)
        s_dev, _ = nd.upload_tables(table, np.zeros((len(table), 3), nd.CHAN_DTYPE), DEV)
        data, targets = nd.sample_patches(store3, s_dev, len(table), patch, n_scales)
        torch.cuda.synchronize()
        out[patch] = (table, data.cpu().numpy(), [t.cpu().numpy() for t in targets])
    return out


@pytest.mark.parametrize("patch", [p for p, _ in PATCHES])
def test_sampling_against_float64(store3, sampled, patch):
    """Copy-mode samples are the normalised crop bit for bit; the others lie within the derived bound of the cubic restatement
    (ref.cubic_sample: the 16-term sum's rounding plus the coordinate rounding through the spline's derivative)."""
    table, data, _ = sampled[patch]
    h, w = patch
    worst, outside = 0.0, []
    for b, s in enumerate(table):
        ci = int(s["case_index"])
        raw, coef, seg = store3.raw(ci).cpu().numpy(), store3.coefficients(ci).cpu().numpy(), store3.labels(ci).cpu().numpy()
        if s["copy"]:
            want, _ = ref.copy_crop(raw, seg, s["m"], h, w)
            assert np.array_equal(data[b], want), f"sample {b}: a copy-mode sample must equal the normalised crop with zero fill"
            continue
        y, x, ey, ex = ref.coordinates(s["m"], h, w)
        want, bound, edge = ref.cubic_sample(coef, y, x, ey, ex)
        assert not edge.any(), "a test coordinate sits on the border of validity"
        err = np.abs(data[b].astype(np.float64) - want)
        H, W = seg.shape
        inside = (y >= 0) & (y <= H - 1) & (x >= 0) & (x <= W - 1)
        outside.append(1 - inside.mean())
        ratio = (err[:, inside] / bound[:, inside]).max() if inside.any() else 0.0
        worst = max(worst, ratio)
        assert (err <= bound).all(), f"sample {b}: worst error / bound {ratio:.3f}"
        assert (data[b][:, ~inside] == 0).all()
    print(f"[seg_sample {h}x{w}] worst measured / bound = {worst:.3f}; outside fractions {[round(v, 2) for v in outside]}")
    assert max(outside) == 1.0 and any(0.3 < v < 0.7 for v in outside) and min(outside) == 0.0


def test_single_channel_store(store1):
    table = batch_table((32, 32))[[0, 2, 7]]
    s_dev, _ = nd.upload_tables(table, np.zeros((3, 1), nd.CHAN_DTYPE), DEV)
    data, targets = nd.sample_patches(store1, s_dev, 3, (32, 32), 1)
    data = data.cpu().numpy()
    raw, coef, seg = store1.raw(0).cpu().numpy(), store1.coefficients(0).cpu().numpy(), store1.labels(0).cpu().numpy()
    assert data.shape == (3, 1, 32, 32) and len(targets) == 1
    assert np.array_equal(data[0], ref.copy_crop(raw, seg, table[0]["m"], 32, 32)[0])
    for b in (1, 2):
        y, x, ey, ex = ref.coordinates(table[b]["m"], 32, 32)
        want, bound, _ = ref.cubic_sample(coef, y, x, ey, ex)
        assert (np.abs(data[b] - want) <= bound).all()


@pytest.mark.parametrize("patch", [p for p, _ in PATCHES])
def test_labels_against_the_vote(store3, sampled, patch):
    """Equal to the restatement except where a label's weight is within 1e-3 of 0.5 there; at most 1 % of the pixels may be set aside like that."""
    table, _, targets = sampled[patch]
    h, w = patch
    near_total = 0
    for b, s in enumerate(table):
        seg = store3.labels(int(s["case_index"])).cpu().numpy()
        got = targets[0][b, 0]
        if s["copy"]:
            assert np.array_equal(got, ref.copy_crop(np.zeros((1,) + seg.shape, np.float32), seg, s["m"], h, w)[1]), f"sample {b}"
            continue
        y, x, ey, ex = ref.coordinates(s["m"], h, w)
        H, W = seg.shape
        assert not ((np.abs(y) <= 1e-4) | (np.abs(y - (H - 1)) <= 1e-4) | (np.abs(x) <= 1e-4) | (np.abs(x - (W - 1)) <= 1e-4)).any()
        want, near = ref.vote_labels(seg, y, x, N_HEADS)
        near_total += int(near.sum())
        assert np.array_equal(got[~near], want[~near]), f"sample {b}: {(got != want)[~near].sum()} labels differ away from a tie"
    print(f"[seg_sample {h}x{w}] {near_total} of {len(table) * h * w} label votes within 1e-3 of 0.5")
    assert near_total == NEAR_HALF[patch] and near_total <= 0.01 * len(table) * h * w
    assert len(np.unique(targets[0])) == N_HEADS


@pytest.mark.parametrize("patch", [p for p, _ in PATCHES])
def test_deep_supervision_targets_are_the_indexed_map(sampled, patch):
    _, _, targets = sampled[patch]
    h, w = patch
    assert len(targets) == dict(PATCHES)[patch]
    for k, t in enumerate(targets):
        assert t.shape == (8, 1, h >> k, w >> k) and t.dtype == np.uint8
        want = targets[0][:, :, ref.ds_indices(k, h)][:, :, :, ref.ds_indices(k, w)]
        assert np.array_equal(t, want), f"scale {k}"


# ---- intensity -------------------------------------------------------------------------------------------------------------------------------
def _planes(B, C, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.nn.functional.avg_pool2d(torch.randn((B, C, h + 2, w + 2), generator=g), 3, 1) * 2.5 + 0.3
    z = torch.randn((B, C, h, w), generator=g)
    return x.contiguous(), z.contiguous()


def _op_tables(op, B, C):
    """Sample 0 carries the operation with per-channel parameters across its range; sample 1 leaves its last channel off."""
    s = np.zeros(B, nd.SAMPLE_DTYPE)
    ch = np.zeros((B, C), nd.CHAN_DTYPE)
    ch["brightness"] = 1.0
    vals = {"blur_sigma": [0.5, 0.73, 1.0, 0.61, 0.95, 0.88], "brightness": [0.75, 1.25, 0.9, 1.1, 0.8, 1.2], "contrast": [0.75, 1.25, 0.9, 1.1, 0.8, 1.2],
            "gamma_inverted": [0.7, 1.5, 0.85, 1.2, 0.95, 1.4], "gamma": [1.5, 0.7, 1.3, 0.8, 1.05, 0.9]}
    names = list(vals) if op == "chain" else ([] if op == "noise" else [op])
    for name in names:
        ch[name] = np.array(vals[name][:B * C], np.float32).reshape(B, C)
    if op in ("noise", "chain"):
        s["noise_sigma"] = [0.1, 0.037][:B]
    for name in vals:   # the last plane: everything off
        ch[name][B - 1, C - 1] = 1.0 if name == "brightness" else 0.0
    return s, ch


def _run(x, z, s, ch, seed=0, use_normal=True):
    data = x.to(DEV).clone()
    s_dev, c_dev = nd.upload_tables(s, ch, DEV)
    nd.augment_intensity_(data, s_dev, c_dev, seed, normal=z.to(DEV) if use_normal else None)
    torch.cuda.synchronize()
    return data.cpu()


def _check(x, z, s, ch, got, what):
    """Every plane within its bound; returns {(b, c): worst error / bound of the plane}."""
    B, C = x.shape[:2]
    ratios = {}
    for b in range(B):
        for c in range(C):
            want, bound = ref.chain(x[b, c].double().numpy(), float(s[b]["noise_sigma"]), z[b, c].double().numpy(), ch[b, c])
            err = np.abs(got[b, c].double().numpy() - want)
            ratios[(b, c)] = float((err / np.maximum(bound, 1e-300)).max())
            assert np.isfinite(got[b, c].numpy()).all()
            assert (err <= bound).all(), f"{what} plane ({b}, {c}): worst error / bound {ratios[(b, c)]:.3f}, max error {err.max():.3e}"
    return ratios


INTENSITY_SHAPES = [(32, 32), (30, 34), (27, 35), (64, 80)]   # float4 walk; ditto, no power of two; scalar walk (945 elements); several loads per thread


@pytest.mark.parametrize("op", ["noise", "blur_sigma", "brightness", "contrast", "gamma_inverted", "gamma", "chain"])
@pytest.mark.parametrize("patch", INTENSITY_SHAPES)
def test_intensity_against_float64(op, patch):
    B, C = 2, 3
    x, z = _planes(B, C, *patch, seed=300)
    s, ch = _op_tables(op, B, C)
    got = _run(x, z, s, ch)
    ratios = _check(x, z, s, ch, got, op)
    # the last plane's own row is off (under "noise" and "chain" it still takes its sample's noise: one rounding): it is reported apart
    on = max(v for k, v in ratios.items() if k != (B - 1, C - 1))
    print(f"[seg_intensity {op} {patch[0]}x{patch[1]}] worst measured / bound = {on:.3f} over the planes that carry it, {ratios[(B - 1, C - 1)]:.3f} on the plane whose row is off")
    if s[B - 1]["noise_sigma"] == 0:
        assert torch.equal(got[B - 1, C - 1], x[B - 1, C - 1]), "a plane whose row is all off must come back untouched"
    again = _run(x, z, s, ch)
    assert torch.equal(got, again), "a second run must be bit-identical"


def test_constant_plane_is_finite_and_within_the_bound():
    B, C, patch = 1, 3, (32, 32)
    x = torch.empty((B, C) + patch)
    x[0, 0], x[0, 1], x[0, 2] = 0.37, -2.5, 0.0
    z = torch.zeros_like(x)
    s, ch = _op_tables("chain", B, C)
    s["noise_sigma"] = 0
    ch[0, C - 1] = ch[0, 0]
    got = _run(x, z, s, ch)
    assert torch.isfinite(got).all()
    _check(x, z, s, ch, got, "constant")
    assert torch.equal(got[0, 2], torch.zeros(patch)), "zeros stay zeros through r = 0 and std = 0"


def test_blur_sigma_outside_the_supported_range():
    """gaussian_filter's radius int(4 sigma + 0.5) is 0 below 0.125: the identity; from 1.875 on (radius above 7) the row counts as off."""
    x, z = _planes(1, 3, 32, 32, seed=301)
    s, ch = _op_tables("blur_sigma", 1, 3)
    ch["blur_sigma"][0] = [0.1, 1.874, 1.875]
    got = _run(x, z, s, ch)
    assert torch.equal(got[0, 0], x[0, 0]) and torch.equal(got[0, 2], x[0, 2])
    want, bound = ref.blur(x[0, 1].double().numpy(), np.float32(1.874))
    assert (np.abs(got[0, 1].double().numpy() - want) <= bound).all() and not torch.equal(got[0, 1], x[0, 1])


def test_table_row_with_a_misaligned_offset_yields_zeros(store3):
    import copy
    table = batch_table((32, 32))[[2, 0]]
    s_dev, _ = nd.upload_tables(table, np.zeros((2, 3), nd.CHAN_DTYPE), DEV)
    for key in ("coef_off", "raw_off"):
        bad = copy.copy(store3)
        rows = store3.table.copy()
        rows[key][0] += 2
        bad.cases_dev = torch.from_numpy(rows.view(np.uint8).reshape(-1).copy()).to(DEV)
        data, targets = nd.sample_patches(bad, s_dev, 2, (32, 32), 3)
        assert not data.any() and not any(t.any() for t in targets), key


def test_philox_noise():
    B, C, patch = 2, 3, (64, 80)
    n = C * patch[0] * patch[1]
    x = torch.zeros((B, C) + patch)
    s = np.zeros(B, nd.SAMPLE_DTYPE)
    ch = np.zeros((B, C), nd.CHAN_DTYPE)
    ch["brightness"] = 1.0
    s["noise_sigma"] = [0.1, 0.05]
    s["philox_offset"] = [1 << 40, 12345]
    a = _run(x, x, s, ch, seed=77, use_normal=False)
    assert torch.equal(a, _run(x, x, s, ch, seed=77, use_normal=False)), "the same (seed, offset) must give the same noise"
    s2 = s.copy()
    s2["philox_offset"] = [(1 << 40) + n, 12345]
    b = _run(x, x, s2, ch, seed=77, use_normal=False)
    assert torch.equal(a[1], b[1]) and not torch.equal(a[0], b[0]) and (a[0] != b[0]).float().mean() > 0.99
    assert not torch.equal(a, _run(x, x, s, ch, seed=78, use_normal=False))
    for i, sigma in enumerate((0.1, 0.05)):
        v = a[i].double().flatten()
        sigma = float(np.float32(sigma))
        mean, var = float(v.mean()), float(v.var(unbiased=False))
        print(f"[philox] sigma {sigma}: mean {mean:.3e} (se {sigma / math.sqrt(n):.3e}), var / sigma^2 {var / sigma ** 2:.4f} (se {math.sqrt(2 / n):.4f})")
        assert abs(mean) <= 5 * sigma / math.sqrt(n)
        assert abs(var - sigma ** 2) <= 5 * sigma ** 2 * math.sqrt(2.0 / n)
    # an odd plane takes the scalar walk: the stream is indexed by element, so a plane of 945 elements draws the first 945 values of the same stream
    xo = torch.zeros((1, 1, 27, 35))
    so, co = s[:1].copy(), ch[:1, :1].copy()
    odd = _run(xo, xo, so, co, seed=77, use_normal=False)
    assert torch.equal(odd.flatten(), a[0].flatten()[:945])


# ---- loader ----------------------------------------------------------------------------------------------------------------------------------
def test_loaders_with_one_seed_agree(store3):
    la, lb = nd.PatchLoader(store3, (32, 32), 6, 3, seed=5), nd.PatchLoader(store3, (32, 32), 6, 3, seed=5)
    lc = nd.PatchLoader(store3, (32, 32), 6, 3, seed=6)
    differs = False
    for _ in range(3):
        a, b, c = next(la), next(lb), next(lc)
        assert a["data"].shape == (6, 3, 32, 32) and a["data"].dtype == torch.float32 and a["data"].is_cuda
        assert [tuple(t.shape) for t in a["target"]] == [(6, 1, 32, 32), (6, 1, 16, 16), (6, 1, 8, 8)] and all(t.dtype == torch.uint8 for t in a["target"])
        assert torch.equal(a["data"], b["data"]) and all(torch.equal(p, q) for p, q in zip(a["target"], b["target"]))
        assert torch.isfinite(a["data"]).all()
        differs |= not torch.equal(a["data"], c["data"])
    assert differs
    with pytest.raises(ValueError, match="not divisible"):
        nd.PatchLoader(store3, (30, 34), 6, 3, seed=5)


def test_validation_loader_yields_exact_crops(store3):
    loader = nd.PatchLoader(store3, (32, 32), 8, 3, seed=9, train=False)
    rng = np.random.default_rng(9)
    for _ in range(2):
        batch = next(loader)
        samples, _ = nd.draw_batch(rng, store3, 8, (32, 32), train=False)
        data, top = batch["data"].cpu().numpy(), batch["target"][0].cpu().numpy()
        for b, s in enumerate(samples):
            ci = int(s["case_index"])
            want, lab = ref.copy_crop(store3.raw(ci).cpu().numpy(), store3.labels(ci).cpu().numpy(), s["m"], 32, 32)
            assert s["copy"] == 1 and np.array_equal(data[b], want) and np.array_equal(top[b, 0], lab)


def test_trainer_steps_on_loader_batches():
    with open(os.path.join(GOLDEN, "nnunet_plans_2d.json")) as f:
        plans = json.load(f)
    with open(os.path.join(GOLDEN, "nnunet_dataset.json")) as f:
        ds = json.load(f)
    spec = nnunet.network_spec(plans, "2d_reduced", ds)
    n_heads, n_scales = spec["n_heads"], spec["n_stages"] - 1
    g = torch.Generator().manual_seed(21)
    cases = []
    for i in range(3):
        img = (torch.nn.functional.avg_pool2d(torch.rand((1, 3, 100, 84), generator=g), 5, 1)[0] * 255).to(torch.uint8)
        cases.append((img, blob_labels(96, 80, 30 + i) % n_heads))
    store = nd.CaseStore(cases, spec["normalization_schemes"], n_heads, DEV, labels=ds["labels"])
    loader = nd.PatchLoader(store, (64, 64), 2, n_scales, seed=3)
    tr = nnunet_train.Trainer(spec, nnunet_train.initial_state_dict(spec, 7), bool(plans["configurations"]["2d"]["batch_dice"]), 10, device=DEV,
                              configuration="2d_reduced")
    losses = []
    for _ in range(3):
        batch = next(loader)
        losses.append(tr.train_step(batch["data"], batch["target"]))
    print(f"[loader -> trainer] losses {[round(v, 4) for v in losses]}, skipped {tr.state.get('skipped_steps', 0)}")
    assert all(math.isfinite(v) for v in losses) and tr.state.get("skipped_steps", 0) == 0
    batch = next(loader)
    val = tr.validation_step(batch["data"], batch["target"])
    assert math.isfinite(val["loss"])
