"""-m gpu: the connected-component kernels (`ldiff_op_cc_label`, `ldiff_op_keep_largest_component`), the device metrics, and the final validation and
postprocessing of the tissue stage end to end.  Every comparison is `torch.equal` (or equality of integers and floats) against the numpy restatement of
tests/nnunet_post_ref.py, which tests/test_cpu_nnunet_post.py checks against scipy and the reference's recorded metrics.

Image sizes straddle the kernels' tile (TH x TW): one pixel, one row and one column longer than two tiles, one short of / one past a tile, exactly a tile,
and several tiles in both axes with ragged edges."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nnunet_post_ref as ref  # noqa: E402

from ldiffusion_amd import _lib, nnunet, nnunet_post as post  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TH, TW = _lib.CC_TILE_H, _lib.CC_TILE_W
KEEP = post.KEEP_LARGEST
SIZES = [(1, 1), (1, 2 * TW + 1), (2 * TH + 1, 1), (TH - 1, TW + 1), (TH, TW), (2 * TH + 1, 3 * TW - 1)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- the kernels on binary contents ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES, ids=lambda v: str(v))
def test_labels_and_largest_component_equal_the_restatement(H, W):
    masks = ref.hand_masks(H, W, TH, TW, seed=H * 1000 + W)
    names = list(masks)
    seg = np.stack([masks[n] for n in names]).astype(np.uint8) * 5           # the member value is 5; all contents as one batch
    labels, sizes = post.cc_label(_dev(seg), 5)
    kept = post.keep_largest_component(_dev(seg), 5)
    assert labels.dtype == torch.int32 and sizes.dtype == torch.int32 and kept.dtype == torch.uint8 and tuple(kept.shape) == seg.shape
    for i, n in enumerate(names):
        lab, sz = ref.label8(masks[n])
        assert torch.equal(labels[i].cpu(), torch.from_numpy(lab)), f"labels of {n!r} at {H} x {W}"
        assert torch.equal(sizes[i].cpu(), torch.from_numpy(sz)), f"sizes of {n!r} at {H} x {W}"
        want = ref.keep_from_labels(seg[i], masks[n], lab, sz, 0)
        assert torch.equal(kept[i].cpu(), torch.from_numpy(want)), f"largest component of {n!r} at {H} x {W}"
        one = post.keep_largest_component(_dev(seg[i]), 5)                    # [H, W] alone: the same image as inside the batch
        assert tuple(one.shape) == (H, W) and torch.equal(one, kept[i]), n


# ---- masks built from multi-valued label maps -------------------------------------------------------------------------------------------------------------
def _label_map(H, W, seed, n=7, cell=3):
    rng = np.random.RandomState(seed)
    coarse = rng.randint(0, n, ((H + cell - 1) // cell, (W + cell - 1) // cell))
    seg = np.kron(coarse, np.ones((cell, cell), np.int64))[:H, :W].astype(np.uint8)
    salt = rng.rand(H, W) < 0.05
    seg[salt] = rng.randint(0, n, int(salt.sum()))
    return seg


@pytest.mark.parametrize("lors", [2, [1, 3], (2, 3, 4), [(1, 2), 6]], ids=str)
@pytest.mark.parametrize("background", [0, 3])
def test_label_maps_labels_lists_and_regions(lors, background):
    H, W = 2 * TH + 1, 3 * TW - 1
    seg = np.stack([_label_map(H, W, 5), _label_map(H, W, 6, cell=7), np.zeros((H, W), np.uint8)])   # three different images, the last without a member
    before = _dev(seg)
    got = post.keep_largest_component(before, lors, background)
    assert torch.equal(before.cpu(), torch.from_numpy(seg)), "seg_in is not modified"
    want = ref.keep_largest(seg, lors, background)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    member = ref.member_mask(seg, lors)
    assert torch.equal(got.cpu()[torch.from_numpy(~member)], torch.from_numpy(seg[~member])), "non-member labels are untouched"
    assert int((want != seg).sum()) > 0
    for i in range(3):                                                        # N = 3 in one call equals three single calls
        assert torch.equal(post.keep_largest_component(before[i], lors, background), got[i])


def test_refusals(lib):
    seg = _dev(_label_map(40, 50, 1))
    with pytest.raises(ValueError, match="seg_out overlaps seg_in"):
        post.keep_largest_component(seg, 1, out=seg)
    with pytest.raises(ValueError, match="seg_out overlaps seg_in"):
        post.keep_largest_component(seg[:30], 1, out=seg[10:])
    with pytest.raises(ValueError, match="uint8 device tensor"):
        post.keep_largest_component(seg.int(), 1)
    with pytest.raises(ValueError, match="background_label=256"):
        post.keep_largest_component(seg, 1, 256)
    with pytest.raises(ValueError, match="does not fit a uint8"):
        post.keep_largest_component(seg, 300)
    out, table, ws = torch.empty_like(seg), post.membership_table(1).to(DEV), torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    call = lambda N, H, W, nbytes: lib.ldiff_op_keep_largest_component(_lib.ptr(seg), _lib.ptr(out), N, H, W, _lib.ptr(table), 0, _lib.ptr(ws), nbytes, _lib.stream_ptr())  # noqa: E731
    for args, word in (((0, 40, 50, 1 << 16), "N=0"), ((1, 0, 50, 1 << 16), "H=0"), ((1, 40, 0, 1 << 16), "W=0"), ((1, 1 << 16, (1 << 14) + 1, 1 << 16), "H \\* W"),
                       ((1, 40, 50, 100), "ws_bytes=100")):
        with pytest.raises(ValueError, match=word):
            _lib.check(call(*args))
    assert lib.ldiff_op_keep_largest_component_ws_bytes(1, 1 << 16, (1 << 14) + 1) == 0 and lib.ldiff_op_keep_largest_component_ws_bytes(0, 4, 4) == 0
    assert lib.ldiff_op_keep_largest_component_ws_bytes(1, 1 << 15, 1 << 15) == 8 * (1 << 30) + 8          # about 8 bytes per pixel
    assert lib.ldiff_op_keep_largest_component_ws_bytes(3, 5, 5) == 8 * 76 + 24


# ---- scale and stability ----------------------------------------------------------------------------------------------------------------------------------
def test_a_1024_square_blob_map_twice():
    g = torch.Generator().manual_seed(11)
    field = torch.nn.functional.interpolate(torch.rand((1, 2, 40, 40), generator=g), size=(1024, 1024), mode="bicubic", align_corners=False)[0].numpy()
    seg = np.where(field[0] > 0.55, 1 + (field[1] > 0.5), 0).astype(np.uint8)     # smooth blobs of classes 1 and 2
    rng = np.random.RandomState(12)
    salt = rng.rand(1024, 1024) < 0.002
    seg[salt] = rng.randint(0, 3, int(salt.sum()))
    mask = ref.member_mask(seg, [1, 2])
    lab, sz = ref.label8(mask)
    assert (sz > 0).sum() > 100 and sz.max() > 20000
    dev = _dev(seg)
    got = post.keep_largest_component(dev, [1, 2])
    assert torch.equal(got.cpu(), torch.from_numpy(ref.keep_from_labels(seg, mask, lab, sz)))
    labels, sizes = post.cc_label(dev, [1, 2])
    assert torch.equal(labels.cpu(), torch.from_numpy(lab)) and torch.equal(sizes.cpu(), torch.from_numpy(sz))
    again = post.keep_largest_component(dev, [1, 2])
    assert torch.equal(again, got) and all(torch.equal(a, b) for a, b in zip(post.cc_label(dev, [1, 2]), (labels, sizes)))


# ---- metrics ----------------------------------------------------------------------------------------------------------------------------------------------
def test_case_metrics_on_device_masks_equal_the_reference_record():
    with open(os.path.join(ROOT, "tests", "golden", "reference_eval_metrics.json")) as f:
        cases = json.load(f)
    assert len(cases) >= 5
    for c in cases:
        lors = [tuple(r) if isinstance(r, list) else r for r in c["labels_or_regions"]]
        want = {post.key_to_label_or_region(k): v for k, v in c["metrics"].items()}
        got = post.case_metrics(_dev(np.array(c["ref"], np.uint8)), _dev(np.array(c["pred"], np.uint8)), lors, c["ignore_label"])
        assert ref.same_metrics(got, want), (c["name"], got, want)


# ---- the stage, end to end ----------------------------------------------------------------------------------------------------------------------------------
def _png(path):
    from PIL import Image
    return np.array(Image.open(path).convert("L"), np.uint8)


@pytest.fixture(scope="module")
def stage(tmp_path_factory):
    """test_gpu_nnunet_prep.py's tiny dataset (six images, fold 0 validates two), one epoch of two iterations, postprocessing=True."""
    import test_gpu_nnunet_prep as prep
    from ldiffusion_amd.segmentor import Segmentor
    tmp = tmp_path_factory.mktemp("post_stage")
    images, labels = prep._write_dataset(str(tmp / "src"))
    with pytest.MonkeyPatch.context() as mp:
        for name in ("nnUNet_raw", "nnUNet_preprocessed", "nnUNet_results"):
            (tmp / name).mkdir()
            mp.setenv(name, str(tmp / name))
        mp.setattr(Segmentor, "load_ldiffusion", lambda self, w, p, **k: (None, None, None))   # mixed sizes: no sampler runs
        seg = Segmentor(None, None, "tissue", 7)
        folder = seg.train_tissue_model_nnUNetv2(1, "weights", "sd", images, labels, images[:2], labels[:2], iterations_per_epoch=2, val_iterations=1,
                                                 num_foreground_voxels=6e4, postprocessing=True)
    raw = tmp / "nnUNet_raw" / "Dataset001_Custom"
    val_keys = json.loads((tmp / "nnUNet_preprocessed" / "Dataset001_Custom" / "splits_final.json").read_text())[0]["val"]
    return dict(tmp=tmp, folder=folder, raw=raw, val_keys=val_keys, images=images, summary=seg.validation_summary)


def test_validation_folder_and_summary(stage):
    val = os.path.join(stage["folder"], "fold_0", "validation")
    keys = stage["val_keys"]
    assert len(keys) == 2
    assert sorted(os.listdir(val)) == sorted([k + ".png" for k in keys] + ["summary.json", "postprocessing.json", "postprocessed"])
    assert sorted(os.listdir(os.path.join(stage["folder"], "fold_0"))) == ["checkpoint_best.pth", "checkpoint_final.pth", "validation"]
    preds = [_png(os.path.join(val, k + ".png")) for k in keys]
    refs = [_png(stage["raw"] / "labelsTr" / (k + ".png")) for k in keys]
    lors = [1, 2, 3, 4, 5, 6]
    summary = post.load_summary_json(os.path.join(val, "summary.json"))
    want_cases = [ref.case_metrics(r, p, lors) for p, r in zip(preds, refs)]
    want = ref.summarize(want_cases)
    assert ref.same_metrics(summary["mean"], want["mean"], ordered=False)
    assert ref.same_metrics({"fg": summary["foreground_mean"]}, {"fg": want["foreground_mean"]}, ordered=False)
    assert len(summary["metric_per_case"]) == 2
    for case, w, k in zip(summary["metric_per_case"], want_cases, keys):
        assert ref.same_metrics(case["metrics"], w, ordered=False) and case["prediction_file"].endswith(k + ".png")
    assert ref.same_metrics(stage["summary"]["mean"], want["mean"])          # what the call kept is what it wrote
    # the predictions are those of the final checkpoint through the predictor's defaults
    head = nnunet.load_trained_model_folder(stage["folder"], 0, "checkpoint_final.pth", device=DEV)
    from PIL import Image
    img = _dev(np.array(Image.open(stage["raw"] / "imagesTr" / (keys[0] + "_0000.png")).convert("RGB"))).permute(2, 0, 1).float()
    assert torch.equal(head.predict_mask(img).cpu(), torch.from_numpy(preds[0]))


def test_recorded_decisions_equal_the_restated_greedy_rule(stage):
    val = os.path.join(stage["folder"], "fold_0", "validation")
    keys = stage["val_keys"]
    preds = [_png(os.path.join(val, k + ".png")) for k in keys]
    refs = [_png(stage["raw"] / "labelsTr" / (k + ".png")) for k in keys]
    lors = [1, 2, 3, 4, 5, 6]
    fns, kwargs, baseline, final, masks = ref.determine_postprocessing(preds, refs, lors, lors)
    record = json.load(open(os.path.join(val, "postprocessing.json")))
    assert record["postprocessing_fns"] == fns and record["postprocessing_kwargs"] == json.loads(json.dumps(kwargs))
    back = {post.key_to_label_or_region(k): v for k, v in record["input_folder"]["mean"].items()}
    assert ref.same_metrics(back, baseline["mean"], ordered=False)
    back = {post.key_to_label_or_region(k): v for k, v in record["postprocessed"]["mean"].items()}
    assert ref.same_metrics(back, final["mean"], ordered=False)
    assert ref.same_metrics({"fg": record["postprocessed"]["foreground_mean"]}, {"fg": final["foreground_mean"]}, ordered=False)
    done = os.path.join(val, "postprocessed")
    assert sorted(os.listdir(done)) == sorted([k + ".png" for k in keys] + ["summary.json"])
    for k, m in zip(keys, masks):
        assert np.array_equal(_png(os.path.join(done, k + ".png")), m)
    assert ref.same_metrics(post.load_summary_json(os.path.join(done, "summary.json"))["mean"], final["mean"], ordered=False)
    assert post.load_postprocessing(os.path.join(val, "postprocessing.json"))[0] == fns


def test_predict_mask_and_folder_inference_with_postprocessing(stage, tmp_path, monkeypatch):
    from PIL import Image
    from ldiffusion_amd.segmentor import Segmentor
    folder = stage["folder"]
    record = os.path.join(folder, "fold_0", "validation", "postprocessing.json")
    head = nnunet.load_trained_model_folder(folder, device=DEV)
    img = _dev(np.array(Image.open(stage["images"][2]).convert("RGB"))).permute(2, 0, 1).float()
    plain = head.predict_mask(img)
    fitted = post.load_postprocessing(record)
    given = ([KEEP, KEEP], [{"labels_or_regions": [1, 2, 3, 4, 5, 6]}, {"labels_or_regions": int(np.bincount(plain.cpu().numpy().ravel()).argmax()), "background_label": 6}])
    for pp in (record, fitted, given):
        fns, kwargs = post.load_postprocessing(pp) if isinstance(pp, str) else pp
        want = ref.apply_postprocessing(plain.cpu().numpy(), fns, kwargs)
        assert torch.equal(head.predict_mask(img, postprocess=pp).cpu(), torch.from_numpy(want))
        assert torch.equal(head.predict_mask(img, batch_tiles=2, postprocess=pp).cpu(), torch.from_numpy(want))
    # folder mode: non-square images skip the diffusion, so only the head and the postprocessing run
    src = tmp_path / "in"
    src.mkdir()
    for i in (2, 3):
        Image.open(stage["images"][i]).save(src / f"img{i}.png")
    monkeypatch.setattr(Segmentor, "load_ldiffusion", lambda self, w, p, **k: (None, None, None))
    seg = Segmentor(None, None, "tissue", 7)
    for pp, out in ((True, tmp_path / "out_true"), (given, tmp_path / "out_given")):
        assert seg.inference_tissue_model_nnUNetv2(str(src), "sd", "weights", folder, output_path=str(out), postprocess=pp) == (None, None)
        fns, kwargs = fitted if pp is True else pp
        for i in (2, 3):
            data = _dev(np.array(Image.open(stage["images"][i]).convert("RGB"))).permute(2, 0, 1).float()
            want = ref.apply_postprocessing(head.predict_mask(data).cpu().numpy(), fns, kwargs)
            assert np.array_equal(_png(out / f"img{i}.png"), want)
    _, single = seg.inference_tissue_model_nnUNetv2(str(src / "img2.png"), "sd", "weights", folder, postprocess=given)
    assert np.array_equal(single, _png(tmp_path / "out_given" / "img2.png"))
    val = os.path.join(folder, "fold_0", "validation")                                                      # the folder entry on the validation masks
    post.apply_postprocessing_to_folder(val, str(tmp_path / "again"), record)
    assert sorted(os.listdir(tmp_path / "again")) == sorted(k + ".png" for k in stage["val_keys"])
    for k in stage["val_keys"]:
        assert np.array_equal(_png(tmp_path / "again" / (k + ".png")), ref.apply_postprocessing(_png(os.path.join(val, k + ".png")), *fitted))


def test_defaults_leave_the_fold_as_it_was_and_a_missing_record_raises(tmp_path, monkeypatch):
    import test_gpu_nnunet_prep as prep
    from ldiffusion_amd.segmentor import Segmentor
    images, labels = prep._write_dataset(str(tmp_path / "src"))
    for name in ("nnUNet_raw", "nnUNet_preprocessed", "nnUNet_results"):
        (tmp_path / name).mkdir()
        monkeypatch.setenv(name, str(tmp_path / name))
    monkeypatch.setattr(Segmentor, "load_ldiffusion", lambda self, w, p, **k: (None, None, None))
    seg = Segmentor(None, None, "tissue", 7)
    folder = seg.train_tissue_model_nnUNetv2(1, "weights", "sd", images, labels, images[:2], labels[:2], iterations_per_epoch=2, val_iterations=1,
                                             num_foreground_voxels=6e4)
    assert sorted(os.listdir(os.path.join(folder, "fold_0"))) == ["checkpoint_best.pth", "checkpoint_final.pth"]
    assert not hasattr(seg, "validation_summary")
    missing = os.path.join(folder, "fold_0", "validation", "postprocessing.json")
    with pytest.raises(FileNotFoundError, match="fold_0/validation/postprocessing.json"):
        seg.inference_tissue_model_nnUNetv2(images[2], "sd", "weights", folder, postprocess=True)
    assert not os.path.exists(missing)
    # validation alone, afterwards, with the best checkpoint: the two masks and the summary, no postprocessing record
    cases = {}
    raw = tmp_path / "nnUNet_raw" / "Dataset001_Custom"
    keys = json.loads((tmp_path / "nnUNet_preprocessed" / "Dataset001_Custom" / "splits_final.json").read_text())[0]["val"]
    from PIL import Image
    for k in keys:
        cases[k] = (_dev(np.array(Image.open(raw / "imagesTr" / (k + "_0000.png")).convert("RGB"))).permute(2, 0, 1).contiguous(), _dev(_png(raw / "labelsTr" / (k + ".png"))))
    summary = post.validate_fold(folder, cases, keys, checkpoint_name="checkpoint_best.pth", batch_tiles=2, io_workers=0)
    val = os.path.join(folder, "fold_0", "validation")
    assert sorted(os.listdir(val)) == sorted([k + ".png" for k in keys] + ["summary.json"])
    want = ref.summarize([ref.case_metrics(_png(raw / "labelsTr" / (k + ".png")), _png(os.path.join(val, k + ".png")), [1, 2, 3, 4, 5, 6]) for k in keys])
    assert ref.same_metrics(summary["mean"], want["mean"])


def test_region_stage_validates_and_writes_region_keys(tmp_path, monkeypatch):
    """The small region setup of tests/test_gpu_nnunet_regions.py (six 64 x 64 images, regions given as grey levels) with postprocessing=True."""
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
    regions = {"any": [100, 150, 50, 200, 250, 255], "high": [200, 250, 255], "top": [255]}
    seg = Segmentor(None, None, "tissue", 7)
    folder = seg.train_tissue_model_nnUNetv2(1, "weights", "sd", images, labels, images[:2], labels[:2], iterations_per_epoch=2, val_iterations=1,
                                             num_foreground_voxels=6e4, regions=regions, regions_class_order=[1, 4, 6], postprocessing=True)
    val = os.path.join(folder, "fold_0", "validation")
    keys = json.loads((tmp_path / "nnUNet_preprocessed" / "Dataset001_Custom" / "splits_final.json").read_text())[0]["val"]
    raw = tmp_path / "nnUNet_raw" / "Dataset001_Custom"
    lors = [(1, 2, 3, 4, 5, 6), (4, 5, 6), (6,)]
    text = json.load(open(os.path.join(val, "summary.json")))
    assert sorted(text["mean"]) == ["(1, 2, 3, 4, 5, 6)", "(4, 5, 6)", "(6,)"]
    preds = [_png(os.path.join(val, k + ".png")) for k in keys]
    refs = [_png(raw / "labelsTr" / (k + ".png")) for k in keys]
    assert all(set(np.unique(p).tolist()) <= {0, 1, 4, 6} for p in preds)
    summary = post.load_summary_json(os.path.join(val, "summary.json"))
    assert ref.same_metrics(summary["mean"], ref.summary_of(preds, refs, lors)["mean"], ordered=False)
    fns, kwargs, baseline, final, masks = ref.determine_postprocessing(preds, refs, lors, [1, 2, 3, 4, 5, 6])   # the first step uses the foreground LABELS
    record = json.load(open(os.path.join(val, "postprocessing.json")))
    assert record["postprocessing_fns"] == fns and record["postprocessing_kwargs"] == json.loads(json.dumps(kwargs))
    assert sorted(record["postprocessed"]["mean"]) == ["(1, 2, 3, 4, 5, 6)", "(4, 5, 6)", "(6,)"]
    for k, m in zip(keys, masks):
        assert np.array_equal(_png(os.path.join(val, "postprocessed", k + ".png")), m)
