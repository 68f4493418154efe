"""-m gpu: plan and preprocess of the tissue head's cases on the device -- the ldiff_op_case_* kernels (non-zero box, crop statistics, label counts, apply,
rank to coordinate) against numpy, `CaseStore(build="device")` against the host build with a crop, and the training stage end to end:
`Segmentor.train_tissue_model_nnUNetv2` from PNG lists to a trained-model folder that the inference head reads back.

Shapes sit where the kernels can go wrong: widths that are no multiple of 16 or 64, more rows than one workgroup takes, row strides wider than W, boxes that
touch every border and none, a 1 x 1 case."""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nnunet_prep_ref as ref  # noqa: E402

from ldiffusion_amd import metrics, nnunet, nnunet_data as nd, nnunet_plan as npl  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _image(C, H, W, box, seed):
    """uint8 [C, H, W]: random inside `box` (with zeros sprinkled in), zero outside; the box's corners are non-zero in some channel."""
    rng = np.random.RandomState(seed)
    img = np.zeros((C, H, W), np.uint8)
    y0, y1, x0, x1 = box
    img[:, y0:y1, x0:x1] = rng.randint(0, 256, (C, y1 - y0, x1 - x0)) * (rng.rand(C, y1 - y0, x1 - x0) > 0.3)
    img[C - 1, y0, x1 - 1] = img[0, y1 - 1, x0] = 7
    return img


def _labels(H, W, n_heads, seed):
    """Blocky label map with every class of 0 .. n_heads - 1 somewhere."""
    rng = np.random.RandomState(seed)
    coarse = rng.randint(0, n_heads, ((H + 7) // 8, (W + 4) // 5))
    return np.kron(coarse, np.ones((8, 5), np.int64))[:H, :W].astype(np.uint8)


CASES = {
    "3x70x67 inner box": lambda: (_image(3, 70, 67, (5, 61, 9, 60), 1), (5, 61, 9, 60)),
    "1x130x257 top-left": lambda: (_image(1, 130, 257, (0, 100, 0, 201), 2), (0, 100, 0, 201)),
    "1x130x257 bottom-right": lambda: (_image(1, 130, 257, (17, 130, 64, 257), 3), (17, 130, 64, 257)),
    "3x70x67 full": lambda: (_image(3, 70, 67, (0, 70, 0, 67), 4), (0, 70, 0, 67)),
    "all zero": lambda: (np.zeros((3, 70, 67), np.uint8), (0, 70, 0, 67)),
    "last pixel": lambda: (_image(3, 70, 67, (69, 70, 66, 67), 5), (69, 70, 66, 67)),
    "3x1x1": lambda: (np.array([[[0]], [[9]], [[0]]], np.uint8), (0, 1, 0, 1)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_bbox_stats_counts(name):
    img, want_box = CASES[name]()
    C, H, W = img.shape
    n_heads = 7
    seg = _labels(H, W, n_heads + 2, 11)          # labels 7 and 8 are out of range
    seg_dev = torch.from_numpy(seg).to(DEV)
    for dtype in (torch.uint8, torch.float32):
        dev = torch.from_numpy(img).to(DEV).to(dtype)
        wide = torch.zeros((C, H + 3, W + 29), dtype=dtype, device=DEV)      # the same image as a view of a wider tensor: row stride > W
        wide[:, 2:2 + H, 13:13 + W] = dev
        for x in (dev, wide[:, 2:2 + H, 13:13 + W]):
            box = nd.case_bbox(x)
            assert box == want_box == nnunet.nonzero_bbox(x), (name, dtype)
            st = nd.case_stats(x, box)
            crop = img[:, box[0]:box[1], box[2]:box[3]].astype(np.int64)
            for c in range(C):
                s1, s2 = int(crop[c].sum()), int((crop[c] * crop[c]).sum())
                if dtype == torch.uint8:
                    assert (int(st["sum"][c]), int(st["sumsq"][c])) == (s1, s2)
                else:       # integer-valued floats: every float64 partial sum is exact
                    assert (float(st["sum"][c]), float(st["sumsq"][c])) == (float(s1), float(s2))
                assert (st["min"][c], st["max"][c]) == (crop[c].min(), crop[c].max())
    wide_seg = torch.full((H + 2, W + 70), 3, dtype=torch.uint8, device=DEV)
    wide_seg[1:1 + H, 5:5 + W] = seg_dev
    for s in (seg_dev, wide_seg[1:1 + H, 5:5 + W]):
        rows, prefix, totals = nd.case_counts(s, want_box, n_heads)
        cut = np.minimum(seg[want_box[0]:want_box[1], want_box[2]:want_box[3]], n_heads)
        want_rows = np.stack([np.bincount(r, minlength=n_heads + 1) for r in cut])
        assert np.array_equal(rows.cpu().numpy(), want_rows)
        sel = np.concatenate([want_rows[:, :n_heads], want_rows[:, 1:].sum(1, keepdims=True)], 1)
        want_prefix = np.concatenate([np.zeros((1, n_heads + 1), np.int64), np.cumsum(sel, 0)], 0).T
        assert np.array_equal(prefix.cpu().numpy(), want_prefix)
        assert np.array_equal(totals, np.concatenate([want_prefix[:, -1], [want_rows[:, n_heads].sum()]]))


def test_float_sums_are_reproducible_and_close():
    """float32 input that is no integer: the fixed-order float64 partial sums are bit-identical from run to run and within n 2^-53 sum|x| of math.fsum."""
    import math
    g = torch.Generator().manual_seed(9)
    x = (torch.randn((2, 130, 257), generator=g) * 37.5 + 4).to(DEV)
    box = (3, 129, 1, 250)
    a, b = nd.case_stats(x, box), nd.case_stats(x, box)
    assert a.tobytes() == b.tobytes()
    crop = x[:, 3:129, 1:250].cpu().double().numpy()
    for c in range(2):
        v = crop[c].ravel()
        tol = v.size * 2.0 ** -53
        assert abs(float(a["sum"][c]) - math.fsum(v)) <= tol * math.fsum(np.abs(v))
        assert abs(float(a["sumsq"][c]) - math.fsum(v * v)) <= 2 * tol * math.fsum(v * v)      # each square is itself rounded once
        assert (a["min"][c], a["max"][c]) == (v.min(), v.max())


def test_label_out_of_range_raises_the_case_store_error():
    img = torch.from_numpy(_image(3, 40, 37, (0, 40, 0, 37), 6))
    seg = torch.from_numpy(_labels(40, 37, 3, 2))
    seg[17, 5] = 3
    for build in ("host", "device"):
        with pytest.raises(ValueError, match=r"CaseStore: case 0: labels \[3\] outside \[0, 3\)"):
            nd.CaseStore([(img, seg)], ["ZScoreNormalization"] * 3, 3, device=DEV, build=build)
    with pytest.raises(ValueError, match=r"CaseStore: case 0: labels \[-1\] outside \[0, 3\)"):         # a negative label of a wider integer type
        nd.CaseStore([(img, seg.long() - 4 * (seg == 3))], ["ZScoreNormalization"] * 3, 3, device=DEV, build="device")


@pytest.fixture(scope="module")
def rank_case():
    """[70, 67] labels: class 4 absent, class 5 a single pixel in the last column, class 2 a row with more than 64 hits."""
    seg = _labels(70, 67, 4, 21)
    seg[seg == 2] = 1
    seg[33, :] = 2
    seg[33, 20] = 0
    seg[12, 66] = 5
    img = _image(3, 70, 67, (0, 70, 0, 67), 8)
    return img, seg


@pytest.mark.parametrize("box", [(0, 70, 0, 67), (4, 66, 1, 67)])
def test_rank_to_coord(rank_case, box):
    img, seg = rank_case
    n_heads = 6
    seg_dev, img_dev = torch.from_numpy(seg).to(DEV), torch.from_numpy(img).to(DEV)
    rows, prefix, totals = nd.case_counts(seg_dev, box, n_heads)
    cut, cimg = seg[box[0]:box[1], box[2]:box[3]], img[:, box[0]:box[1], box[2]:box[3]]
    assert totals[4] == 0 and totals[5] == 1 and rows[33 - box[0], 2] > 64
    rng = np.random.RandomState(0)
    for sel in list(range(n_heads)) + [-1]:
        locs = np.argwhere(cut == sel) if sel >= 0 else np.argwhere(cut > 0)
        assert len(locs) == totals[sel if sel >= 0 else n_heads]
        if len(locs) == 0:
            coords, _ = nd.case_rank_to_coord(seg_dev, box, sel, prefix[sel], torch.zeros(0, dtype=torch.int64, device=DEV))
            assert coords.shape == (0, 2)
            with pytest.raises(ValueError, match="ranks span"):
                nd.case_rank_to_coord(seg_dev, box, sel, prefix[sel], torch.zeros(1, dtype=torch.int64, device=DEV))
            continue
        ranks = np.concatenate([rng.permutation(len(locs)), rng.randint(0, len(locs), 40)]).astype(np.int64)   # all ranks, shuffled, then repeats
        for dtype in (torch.uint8, torch.float32):
            coords, values = nd.case_rank_to_coord(seg_dev, box, sel, prefix[sel if sel >= 0 else n_heads], torch.from_numpy(ranks).to(DEV), image=img_dev.to(dtype))
            assert np.array_equal(coords.cpu().numpy(), locs[ranks]), sel
            assert values.dtype == dtype and np.array_equal(values.cpu().numpy(), cimg[:, locs[ranks, 0], locs[ranks, 1]].T.astype(values.cpu().numpy().dtype))
    with pytest.raises(ValueError, match="ranks span"):
        nd.case_rank_to_coord(seg_dev, box, 1, prefix[1], torch.tensor([int(totals[1])], device=DEV))


SCHEME_SETS = [["ZScoreNormalization", "RescaleTo01Normalization", "ZScoreNormalization"], ["RGBTo01Normalization", "NoNormalization", "RGBTo01Normalization"]]


def _device_store(img, seg, schemes, n_heads, **kw):
    return nd.CaseStore([(img, seg)], schemes, n_heads, device=DEV, build="device", **kw)


@pytest.mark.parametrize("schemes", SCHEME_SETS, ids=["zscore+rescale", "rgb+none"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
def test_apply_against_float64(schemes, dtype):
    box = (5, 61, 9, 60)
    img = _image(3, 70, 67, box, 31)
    img[1, 5:61, 9:60] = np.clip(img[1, 5:61, 9:60], 3, 250)
    seg = _labels(70, 67, 5, 32)
    x = torch.from_numpy(img).to(dtype)
    if dtype == torch.float32 and "ZScoreNormalization" in schemes:
        x = x + torch.rand(x.shape, generator=torch.Generator().manual_seed(1)) * (x != 0)      # no integers; the zero frame stays zero
    store = _device_store(x, torch.from_numpy(seg), schemes, 5, prefilter="device")
    assert store.boxes == [box] and store.shape(0) == (56, 51)
    crop = x[:, 5:61, 9:60].numpy()
    stats = nd.case_stats(x.to(DEV), box)
    raw_words = np.ascontiguousarray(stats).view(np.int64).reshape(3, 4)
    sub32, div32 = nd.normalization_scalars(raw_words, dtype, 56 * 51, schemes)
    t, bound = ref.normalize_with_bound(crop, schemes, sub32, div32)
    got = store.raw(0).cpu().numpy()
    err = np.abs(got.astype(np.float64) - t)
    print(f"[case_apply {schemes[0]} {dtype}] worst measured / bound = {(err / bound).max():.3f}; bound max {bound.max():.3e}")
    assert (err <= bound).all()
    for c, scheme in enumerate(schemes):
        if scheme in ("RGBTo01Normalization", "NoNormalization"):
            want = torch.from_numpy(crop[c].astype(np.float32))
            assert torch.equal(store.raw(0)[c].cpu(), want / 255.0 if scheme == "RGBTo01Normalization" else want), scheme
            assert np.array_equal(got[c], t[c].astype(np.float32)), scheme                       # the float64 quotient rounded once
    assert torch.equal(store.labels(0).cpu(), torch.from_numpy(seg[5:61, 9:60]))
    # prefilter="device": the coefficient planes are the spline prefilter of the raw planes; "host": the float64 filter rounded once
    assert torch.equal(store.coefficients(0), nd.spline_prefilter_(store.raw(0).clone()))
    host_pre = _device_store(x, torch.from_numpy(seg), schemes, 5, prefilter="host")
    assert torch.equal(host_pre.raw(0), store.raw(0))
    assert torch.equal(host_pre.coefficients(0).cpu(), torch.from_numpy(nd.spline_coefficients(got).astype(np.float32)))


@pytest.fixture(scope="module")
def three_cases():
    out = []
    for k, (H, W, box) in enumerate([(70, 67, (5, 61, 9, 60)), (130, 257, (0, 100, 0, 201)), (33, 300, (2, 33, 40, 300))]):
        img = _image(3, H, W, box, 40 + k)
        seg = _labels(H, W, 5, 50 + k)
        seg[seg == 3] = 0 if k == 1 else 3       # one case lacks a class
        out.append((torch.from_numpy(img), torch.from_numpy(seg)))
    return out


def test_store_device_build_matches_host_build(three_cases):
    schemes = ["ZScoreNormalization", "RescaleTo01Normalization", "RGBTo01Normalization"]
    host = nd.CaseStore(three_cases, schemes, 5, device=DEV, build="host", crop=True)
    on_host = nd.CaseStore(three_cases, schemes, 5, device=DEV, build="device")
    on_dev = nd.CaseStore([(i.to(DEV), s.to(DEV)) for i, s in three_cases], schemes, 5, device=DEV, build="device")
    assert torch.equal(on_host.arena, on_dev.arena)                       # the pairs may live on either side
    dev = on_dev
    assert np.array_equal(host.table, dev.table) and host.boxes == dev.boxes == [(5, 61, 9, 60), (0, 100, 0, 201), (2, 33, 40, 300)]
    for i, (img, seg) in enumerate(three_cases):
        b = dev.boxes[i]
        assert torch.equal(host.labels(i), dev.labels(i))
        assert set(host.class_locations[i]) == set(dev.class_locations[i]) == {1, 2, 3, 4}
        for c in range(1, 5):
            hl, dl = host.class_locations[i][c], dev.class_locations[i][c]
            assert len(hl) == len(dl) and (len(hl) == 0 or (dl.dtype == hl.dtype and np.array_equal(hl, dl))), (i, c)
        crop = img[:, b[0]:b[1], b[2]:b[3]].numpy()
        raw_words = np.ascontiguousarray(nd.case_stats(img.to(DEV), b)).view(np.int64).reshape(3, 4)
        sub32, div32 = nd.normalization_scalars(raw_words, torch.uint8, crop[0].size, schemes)
        t, bound = ref.normalize_with_bound(crop, schemes, sub32, div32)
        _, host_bound = ref.torch_reduction_bound(crop, schemes, sub32, div32)
        d, h = dev.raw(i).cpu().double().numpy(), host.raw(i).cpu().double().numpy()
        print(f"[store case {i}] device / bound = {(np.abs(d - t) / bound).max():.3f}; host / its bound = {(np.abs(h - t) / host_bound).max():.3f}")
        assert (np.abs(d - t) <= bound).all() and (np.abs(h - t) <= host_bound).all()
        assert torch.equal(dev.raw(i)[1:], host.raw(i)[1:])               # rescale and rgb: the same float32 operations on both sides
    assert len(dev.class_locations[1][3]) == 0
    # the same seed draws the same patches: identical targets, data within the planes' bound (copies) -- compared where no interpolation happens
    la = nd.PatchLoader(host, (32, 48), 4, 3, seed=5, train=False)
    lb = nd.PatchLoader(dev, (32, 48), 4, 3, seed=5, train=False)
    for _ in range(2):
        a, b = next(la), next(lb)
        assert all(torch.equal(x, y) for x, y in zip(a["target"], b["target"]))
        assert torch.equal(a["data"][:, 1:], b["data"][:, 1:])
    ta, tb = nd.PatchLoader(host, (32, 48), 4, 3, seed=6, train=True), nd.PatchLoader(dev, (32, 48), 4, 3, seed=6, train=True)
    a, b = next(ta), next(tb)
    assert all(torch.equal(x, y) for x, y in zip(a["target"], b["target"]))


def test_fingerprint_on_the_device_equals_the_host(three_cases):
    dj = {"channel_names": {"0": "R", "1": "G", "2": "B"}, "labels": {"background": 0, **{f"class{i}": i for i in range(1, 5)}}, "numTraining": 3, "file_ending": ".png"}
    host = npl.extract_fingerprint(three_cases, dj, num_foreground_voxels=3000)
    dev = npl.extract_fingerprint([(i.to(DEV), s.to(DEV)) for i, s in three_cases], dj, num_foreground_voxels=3000)
    assert json.dumps(host) == json.dumps(dev)
    assert host["shapes_after_crop"] == [[1, 56, 51], [1, 100, 201], [1, 31, 260]]


# ---------------------------------------------------------------- end to end
def _write_dataset(root, n=6):
    from PIL import Image
    rng = np.random.RandomState(77)
    levels = np.array(sorted(metrics.PIXEL_TO_LABEL), np.uint8)
    images, labels = [], []
    os.makedirs(root, exist_ok=True)
    for k in range(n):
        H, W = (96, 80) if k % 2 == 0 else (90, 84)
        img = rng.randint(1, 256, (H, W, 3)).astype(np.uint8)
        if k < 2:
            img[:3], img[:, -2:] = 0, 0                                  # a black frame: cropped away
        lab = levels[_labels(H, W, 7, 60 + k)]
        Image.fromarray(img).save(os.path.join(root, f"im{k}.png"))
        Image.fromarray(lab).save(os.path.join(root, f"lb{k}.png"))
        images.append(os.path.join(root, f"im{k}.png"))
        labels.append(os.path.join(root, f"lb{k}.png"))
    return images, labels


def test_train_tissue_model_end_to_end(tmp_path, monkeypatch):
    from PIL import Image
    from ldiffusion_amd.segmentor import Segmentor
    images, labels = _write_dataset(str(tmp_path / "src"))
    for name in ("nnUNet_raw", "nnUNet_preprocessed", "nnUNet_results"):
        (tmp_path / name).mkdir()
        monkeypatch.setenv(name, str(tmp_path / name))
    loaded = []
    monkeypatch.setattr(Segmentor, "load_ldiffusion", lambda self, w, p, **k: loaded.append((w, p)) or (None, None, None))   # mixed sizes: no sampler runs
    seg = Segmentor(None, None, "tissue", 7)
    folder = seg.train_tissue_model_nnUNetv2(1, "weights", "sd", images, labels, images[:2], labels[:2], iterations_per_epoch=2, val_iterations=1,
                                             num_foreground_voxels=6e4)
    assert loaded == [("weights", "sd")]
    assert folder == str(tmp_path / "nnUNet_results" / "Dataset001_Custom" / "nnUNetTrainer__nnUNetPlans__2d")
    pre = tmp_path / "nnUNet_preprocessed" / "Dataset001_Custom"
    files = {n: json.loads((pre / n).read_text()) for n in ("dataset_fingerprint.json", "nnUNetPlans.json", "dataset.json", "splits_final.json")}
    assert files["dataset.json"] == json.loads((tmp_path / "nnUNet_raw" / "Dataset001_Custom" / "dataset.json").read_text())
    assert json.dumps(files["nnUNetPlans.json"]) == json.dumps(npl.plan_experiment(files["dataset_fingerprint.json"], files["dataset.json"], "Dataset001_Custom"))
    assert files["dataset_fingerprint.json"]["shapes_after_crop"][:2] == [[1, 93, 78], [1, 87, 82]]
    assert files["splits_final.json"] == npl.crossval_splits([f"case_{i:03d}" for i in range(6)])
    for name in ("checkpoint_best.pth", "checkpoint_final.pth"):
        ckpt = torch.load(os.path.join(folder, "fold_0", name), map_location="cpu", weights_only=False)
        assert ckpt["init_args"]["configuration"] == "2d" and ckpt["trainer_name"] == "nnUNetTrainer"
    log = seg.training_log
    assert len(log["train_losses"]) == 1 and np.isfinite(log["train_losses"]).all() and np.isfinite(log["val_losses"]).all()
    head = nnunet.load_trained_model_folder(folder, device=DEV)
    case = torch.from_numpy(np.array(Image.open(images[0]).convert("RGB"))).permute(2, 0, 1).float().to(DEV)
    mask = head.predict_mask(case)
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (96, 80) and int(mask.max()) < 7


def test_orchestrator_reaches_the_tissue_trainer(tmp_path, monkeypatch):
    from ldiffusion_amd.ldiffusion import LDiffusionModel
    from ldiffusion_amd.segmentor import Segmentor
    calls = []

    def record(self, epochs, ldiffusion_weight, diffusion_path, **kw):
        calls.append((self.level, self.num_classes, epochs, ldiffusion_weight, diffusion_path, kw))
        return "model-folder"

    monkeypatch.setattr(Segmentor, "train_tissue_model_nnUNetv2", record)
    args = SimpleNamespace(num_epochs=12, diffusion_path="sd", num_classes=7)
    tr = SimpleNamespace(dataset=SimpleNamespace(image_dir=["a.png"], label_dir=["a_l.png"]))
    va = SimpleNamespace(dataset=SimpleNamespace(image_dir=["b.png"], label_dir=["b_l.png"]))
    out = LDiffusionModel(str(tmp_path), "tissue").train(args, component="segmentor", ldiffusion_weight="w", train_loader=tr, val_loader=va, iterations_per_epoch=3)
    assert out == "model-folder"
    assert calls == [("tissue", 7, 2, "w", "sd", dict(train_images=["a.png"], train_labels=["a_l.png"], test_images=["b.png"], test_labels=["b_l.png"], iterations_per_epoch=3))]
    with pytest.raises(NotImplementedError):
        LDiffusionModel(str(tmp_path), "cell").train(args, component="segmentor", ldiffusion_weight="w", train_loader=tr, val_loader=va)
