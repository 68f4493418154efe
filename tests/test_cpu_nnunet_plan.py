"""CPU (-m "not gpu"): nnU-Net's plan-and-preprocess decisions for the tissue head (ldiffusion_amd/nnunet_plan.py) and the dataset writer
(utils.create_nnunet_dataset), each pinned to what the reference's own code returned (scripts/gen_golden_planner.py records the fixtures; nothing here reads
the reference).  The one unpinned piece is `conv_feature_map_size` (its docstring says why): the plans fixture was recorded with that function in the
place of the reference's VRAM estimate, so everything around it -- topology, reduction loop, batch size, the 5 % cap, keys and key order -- is pinned."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from ldiffusion_amd import _lib, metrics, nnunet, nnunet_data as nd, nnunet_plan as npl

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def planner_golden():
    with open(os.path.join(GOLDEN, "reference_planner.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def fingerprint_golden():
    return dict(np.load(os.path.join(GOLDEN, "reference_fingerprint.npz")))


def synthetic(n_cases, shapes, n_labels, rel=1.0, channel_names=None):
    """The generator's function of the same name: (fingerprint, dataset.json) of a dataset whose cases cycle through `shapes` (h, w)."""
    names = channel_names or {"0": "R", "1": "G", "2": "B"}
    fp = {"spacings": [[999.0, 1.0, 1.0]] * n_cases, "shapes_after_crop": [[1, *shapes[i % len(shapes)]] for i in range(n_cases)],
          "foreground_intensity_properties_per_channel": {k: {"mean": 120.5 + int(k), "median": 119.0, "std": 40.25, "min": 0.0, "max": 255.0, "percentile_99_5": 250.0,
                                                              "percentile_00_5": 3.0} for k in names},
          "median_relative_size_after_cropping": rel}
    dj = {"channel_names": names, "labels": {"background": 0, **{f"class{i}": i for i in range(1, n_labels)}}, "numTraining": n_cases, "file_ending": ".png"}
    return fp, dj


# ---------------------------------------------------------------- fingerprint
def test_foreground_ranks_reproduce_the_reference_samples(fingerprint_golden):
    """collect_foreground_intensities draws rs.choice(foreground_pixels, n, replace=True) per channel from one RandomState(1234): the restated rank draw
    plus a numpy gather gives the same intensities, for a case with a blob and a case without foreground."""
    g = fingerprint_golden
    n = int(g["num_samples"])
    for i in range(2):
        img, seg = g[f"image_{i}"], g[f"seg_{i}"]
        fg = seg > 0
        ranks = npl.foreground_ranks(int(fg.sum()), 3, n)
        for c in range(3):
            want = g[f"samples_{i}_{c}"]
            got = img[c][fg][ranks[c]].astype(np.float32)
            assert got.shape == want.shape and np.array_equal(got, want), f"case {i} channel {c}"
    assert g["samples_1_0"].size == 0 and g["samples_0_0"].size == n


def test_extract_fingerprint_on_the_host_matches_the_reference_run(fingerprint_golden):
    g = fingerprint_golden
    n = int(g["num_samples"])
    dj = {"channel_names": {"0": "R", "1": "G", "2": "B"}, "labels": {"background": 0, "a": 1}, "numTraining": 2, "file_ending": ".png"}
    cases = [(torch.from_numpy(g[f"image_{i}"]), torch.from_numpy(g[f"seg_{i}"])) for i in range(2)]
    fp = npl.extract_fingerprint(cases, dj, num_foreground_voxels=2 * n)
    names = ["mean", "median", "std", "min", "max", "percentile_99_5", "percentile_00_5"]
    for c in range(3):
        assert [fp["foreground_intensity_properties_per_channel"][str(c)][k] for k in names] == list(g["statistics"][c])
    assert list(fp["foreground_intensity_properties_per_channel"][str(0)]) == names
    assert fp["shapes_after_crop"] == [[1, 40, 37], [1, 40, 37]] and fp["spacings"] == [[999.0, 1.0, 1.0]] * 2   # random images: nothing to crop
    assert fp["median_relative_size_after_cropping"] == 1.0
    assert list(fp) == ["spacings", "shapes_after_crop", "foreground_intensity_properties_per_channel", "median_relative_size_after_cropping"]
    json.dumps(fp)
    # a black frame is cropped away: shape, relative size
    img = torch.zeros((3, 20, 30), dtype=torch.uint8)
    img[1, 4:15, 6:27] = 9
    seg = torch.zeros((20, 30), dtype=torch.uint8)
    seg[5:8, 7:9] = 1
    fp = npl.extract_fingerprint([(img, seg)], dj, num_foreground_voxels=10)
    assert fp["shapes_after_crop"] == [[1, 11, 21]] and fp["median_relative_size_after_cropping"] == 11 * 21 / 600
    with pytest.raises(ValueError, match="foreground"):
        npl.extract_fingerprint([(img, torch.zeros_like(seg))], dj, num_foreground_voxels=10)


# ---------------------------------------------------------------- topology and plans
def test_get_pool_and_conv_props_matches_the_reference(planner_golden):
    rows = planner_golden["topology"]
    assert any(r["patch_size"][0] != r["patch_size"][1] for r in rows) and any(min(r["patch_size"]) < 8 for r in rows) and any(r["patch_size"] == [1024, 1024] for r in rows)
    for r in rows:
        got = npl.get_pool_and_conv_props(r["spacing"], np.array(r["patch_size"]), r["min_feature_map_size"], r["max_numpool"])
        got = [[int(v) for v in got[0]], [[int(v) for v in p] for p in got[1]], [[int(v) for v in k] for k in got[2]], [int(v) for v in got[3]], [int(v) for v in got[4]]]
        assert got == r["result"], f"{r['spacing']} {r['patch_size']} cap {r['max_numpool']}"


def test_plan_experiment_matches_the_reference(planner_golden):
    seen = {}
    for row in planner_golden["plans"]:
        args = list(row["synthetic"])
        args[1] = [tuple(s) for s in args[1]]
        fp, dj = synthetic(*args)
        got = npl.plan_experiment(fp, dj, row["dataset_name"], row["gpu_memory_target_in_gb"])
        want = row["plans"]
        assert json.dumps(got) == json.dumps(want), row["name"]          # values, keys and key order
        cfg = got["configurations"]["2d"]
        seen[row["name"]] = (cfg["patch_size"], cfg["batch_size"], len(cfg["pool_op_kernel_sizes"]))
        if any(cfg["use_mask_for_norm"]):                                 # what the head does not cover is refused where it always was, by name
            with pytest.raises(ValueError, match="use_mask_for_norm"):
                nnunet.network_spec(got, "2d", dj)
        elif any(p[0] != p[1] for p in cfg["pool_op_kernel_sizes"]):      # a long thin dataset pools one axis further
            with pytest.raises(ValueError, match="pool_op_kernel_sizes"):
                nnunet.network_spec(got, "2d", dj)
        else:
            spec = nnunet.network_spec(got, "2d", dj)
            assert spec["patch_size"] == tuple(cfg["patch_size"]) and spec["n_heads"] == len(dj["labels"])
    # the figures the restated estimate gives (unpinned: regenerated by the script, recorded here so that a change of the estimate shows)
    assert seen["20 x 1024^2 RGB, 7 labels"] == ([512, 512], 4, 8)
    assert seen["6 x 96x80, 3 labels"] == ([96, 80], 2, 5)
    assert seen["10 x 700x1000, 7 labels"] == ([448, 576], 2, 7)
    assert seen["400 x 1024^2, 7 labels: no 5 % cap"][1] == 12 and seen["3000 x 256^2, 2 labels: batch size from the headroom"][1] > 12


def test_plan_experiment_refuses_a_3d_dataset():
    fp, dj = synthetic(4, [(64, 64)], 3)
    fp["shapes_after_crop"] = [[30, 64, 64]] * 4
    fp["spacings"] = [[1.0, 1.0, 1.0]] * 4
    with pytest.raises(ValueError, match="shapes_after_crop"):
        npl.plan_experiment(fp, dj, "DatasetXXX")


def test_conv_feature_map_size_by_hand():
    """Two stages on 8 x 8, 2 convs each, widths 32 / 64, 3 labels: encoder 2*32*64 + 2*64*16; decoder at 8 x 8: 2*32*64 convs + 32*64 transposed conv + 3*64
    head."""
    got = npl.conv_feature_map_size((8, 8), 2, ((1, 1), (2, 2)), 3, (32, 64), (2, 2), (2,), 3)
    assert got == 2 * 32 * 64 + 2 * 64 * 16 + 2 * 32 * 64 + 32 * 64 + 3 * 64


# ---------------------------------------------------------------- split
def test_crossval_splits_match_sklearn(planner_golden):
    for n, want in planner_golden["splits"].items():
        keys = [f"case_{i:03d}" for i in range(int(n))]
        assert npl.crossval_splits(keys[::-1]) == want, n      # any order in: do_split sorts
    with pytest.raises(ValueError, match="n_splits=5 greater than the number of samples: n_samples=4"):
        npl.crossval_splits([f"case_{i:03d}" for i in range(4)])


# ---------------------------------------------------------------- the store's host build with a crop, the scalars of the device build
def test_case_store_host_crop_flag():
    g = torch.Generator().manual_seed(3)
    img = torch.zeros((3, 30, 41), dtype=torch.uint8)
    img[:, 4:27, 5:33] = torch.randint(1, 256, (3, 23, 28), generator=g).to(torch.uint8)
    seg = torch.zeros((30, 41), dtype=torch.uint8)
    seg[6:12, 8:20], seg[2:4, 0:3] = 2, 1                       # class 1 lies outside the non-zero box
    schemes = ["ZScoreNormalization", "RGBTo01Normalization", "RescaleTo01Normalization"]
    whole = nd.CaseStore([(img, seg)], schemes, 3, device="cpu")
    again = nd.CaseStore([(img, seg)], schemes, 3, device="cpu", build="host", crop=False)
    assert torch.equal(whole.arena, again.arena) and whole.shape(0) == (30, 41) and whole.boxes == [(0, 30, 0, 41)]
    cropped = nd.CaseStore([(img, seg)], schemes, 3, device="cpu", crop=True)
    assert cropped.shape(0) == (23, 28) and cropped.boxes == [(4, 27, 5, 33)]
    direct = nd.CaseStore([(img[:, 4:27, 5:33], seg[4:27, 5:33])], schemes, 3, device="cpu")
    assert torch.equal(cropped.arena, direct.arena) and np.array_equal(cropped.table, direct.table)
    assert len(cropped.class_locations[0][1]) == 0 and len(cropped.class_locations[0][2]) == 72
    with pytest.raises(ValueError, match="build"):
        nd.CaseStore([(img, seg)], schemes, 3, device="cpu", build="gpu")
    with pytest.raises(ValueError, match="needs the store on a GPU"):
        nd.CaseStore([(img, seg)], schemes, 3, device="cpu", build="device")


def test_normalization_scalars_from_exact_sums():
    x = np.array([[3, 250, 7, 7, 0, 255]], np.uint8)
    raw = np.zeros((1, 4), np.int64)
    rec = nd.stats_records(raw, torch.uint8)
    rec["sum"], rec["sumsq"], rec["min"], rec["max"] = int(x.sum()), int((x.astype(np.int64) ** 2).sum()), 0.0, 255.0
    for scheme, want in (("ZScoreNormalization", (np.float32(x.mean(dtype=np.float64)), np.float32(x.std(dtype=np.float64)))), ("RGBTo01Normalization", (0.0, 255.0)),
                         ("RescaleTo01Normalization", (0.0, 255.0)), ("NoNormalization", (0.0, 1.0))):
        sub, div = nd.normalization_scalars(raw, torch.uint8, x.size, [scheme])
        assert (sub[0], div[0]) == want, scheme
    rec["sumsq"] = int(x.sum()) ** 2 // x.size        # a constant plane: std 0 -> the 1e-8 floor
    rec["sum"] = 6 * 7
    rec["sumsq"] = 6 * 49
    assert nd.normalization_scalars(raw, torch.uint8, 6, ["ZScoreNormalization"])[1][0] == np.float32(1e-8)
    rec["max"] = 256.0
    with pytest.raises(ValueError, match="0..255"):
        nd.normalization_scalars(raw, torch.uint8, 6, ["RGBTo01Normalization"])


def test_case_entry_points_refuse_bad_arguments(lib):
    """Argument checks of the ldiff_op_case_* launchers run before anything touches the device."""
    one = C.c_void_p(256)
    assert lib.ldiff_op_case_stats_ws_bytes(3) == 3 * 64 * 32 and lib.ldiff_op_case_stats_ws_bytes(0) == 0 and lib.ldiff_op_case_stats_ws_bytes(17) == 0
    assert lib.ldiff_op_case_bbox(one, 2, 3, 8, 8, 8, 64, one, None) == -1 and b"dtype" in lib.ldiff_last_error()
    assert lib.ldiff_op_case_bbox(one, 0, 17, 8, 8, 8, 64, one, None) == -1 and b"channels" in lib.ldiff_last_error()
    assert lib.ldiff_op_case_bbox(one, 0, 3, 8, 8, 7, 64, one, None) == -1 and b"row_stride" in lib.ldiff_last_error()
    assert lib.ldiff_op_case_bbox(one, 0, 3, 8, 8, 8, 63, one, None) == -1 and b"plane_stride" in lib.ldiff_last_error()
    assert lib.ldiff_op_case_bbox(None, 0, 3, 8, 8, 8, 64, one, None) == -1 and b"null" in lib.ldiff_last_error()
    assert lib.ldiff_op_case_stats(one, 0, 3, 8, 8, 8, 64, 0, 9, 0, 8, one, one, 1 << 20, None) == -1 and b"box" in lib.ldiff_last_error()
    assert lib.ldiff_op_case_stats(one, 0, 3, 8, 8, 8, 64, 0, 8, 0, 8, one, one, 16, None) == -1 and b"ldiff_op_case_stats_ws_bytes" in lib.ldiff_last_error()
    assert lib.ldiff_op_case_counts(one, 8, 8, 8, 0, 8, 0, 8, 33, one, one, one, None) == -1 and b"n_heads" in lib.ldiff_last_error()
    assert lib.ldiff_op_case_counts(one, 8, 8, 8, 2, 2, 0, 8, 7, one, one, one, None) == -1 and b"box" in lib.ldiff_last_error()
    row = _lib.SegCase(0, 512, 1024, 8, 8, 8, 8)
    sub = (C.c_float * 3)(0, 0, 0)
    assert lib.ldiff_op_case_apply(one, 0, 3, 8, 8, 8, 64, one, 8, 0, 8, 0, 8, sub, sub, one, 1024 + 63, C.byref(row), 0, None) == -1 and b"leaves the arena" in lib.ldiff_last_error()
    row.H = 7
    assert lib.ldiff_op_case_apply(one, 0, 3, 8, 8, 8, 64, one, 8, 0, 8, 0, 8, sub, sub, one, 4096, C.byref(row), 0, None) == -1 and b"table row" in lib.ldiff_last_error()
    assert lib.ldiff_op_case_rank_to_coord(one, 8, 8, 8, 0, 8, 0, 8, 300, one, one, 4, one, None, 0, 0, 0, 0, None, None) == -1 and b"selector" in lib.ldiff_last_error()
    assert lib.ldiff_op_case_rank_to_coord(one, 8, 8, 8, 0, 8, 0, 8, 1, one, one, 0, one, None, 0, 0, 0, 0, None, None) == 0   # nothing to do


# ---------------------------------------------------------------- dataset writer
def _write_png(path, arr):
    from PIL import Image
    Image.fromarray(arr).save(path)


def test_create_nnunet_dataset_mixed_sizes(tmp_path, monkeypatch):
    """Mixed image sizes: no diffusion runs (copies), so this needs neither a pipeline nor a GPU."""
    from PIL import Image
    from ldiffusion_amd import utils
    rng = np.random.RandomState(5)
    src = tmp_path / "src"
    src.mkdir()
    levels = np.array(sorted(metrics.PIXEL_TO_LABEL), np.uint8)
    tr_i, tr_l, te_i, te_l = [], [], [], []
    for k, (h, w) in enumerate([(20, 24), (22, 24), (20, 24)]):
        _write_png(src / f"im{k}.png", rng.randint(0, 256, (h, w, 3)).astype(np.uint8))
        lab = levels[rng.randint(0, len(levels), (h, w))]
        lab[0, 0] = 77                                                       # a grey level the table does not name -> 0
        if k == 1:
            lab = lab[::2, ::2]                                              # a label of another size: resized to the image, NEAREST
        _write_png(src / f"lb{k}.png", lab)
        (tr_i if k < 2 else te_i).append(str(src / f"im{k}.png"))
        (tr_l if k < 2 else te_l).append(str(src / f"lb{k}.png"))
    assert utils.check_images_same_size(tr_i) is False and utils.check_images_same_size(te_i) is True
    raw = tmp_path / "raw"
    (raw / "Dataset003_x").mkdir(parents=True)
    (raw / "Datasetabc").mkdir()
    (raw / "notes").mkdir()
    monkeypatch.delenv("nnUNet_raw", raising=False)
    with pytest.raises(RuntimeError, match="nnUNet_raw"):
        utils.create_nnunet_dataset(tr_i, tr_l, te_i, te_l, 7, None, None)
    monkeypatch.setenv("nnUNet_raw", str(raw))
    num, name = utils.create_nnunet_dataset(tr_i, tr_l, te_i, te_l, 7, None, None)
    assert (num, name) == (4, "Dataset004_Custom")
    root = raw / name
    assert sorted(p.name for p in root.iterdir()) == ["dataset.json", "imagesTr", "imagesTs", "labelsTr", "labelsTs"]
    assert sorted(p.name for p in (root / "imagesTr").iterdir()) == ["case_000_0000.png", "case_001_0000.png"]
    assert sorted(p.name for p in (root / "labelsTr").iterdir()) == ["case_000.png", "case_001.png"]
    assert [p.name for p in (root / "imagesTs").iterdir()] == ["caseTs_000_0000.png"] and [p.name for p in (root / "labelsTs").iterdir()] == ["caseTs_000.png"]
    want = {"channel_names": {"0": "R", "1": "G", "2": "B"}, "labels": {"background": 0, **{f"class{i}": i for i in range(1, 7)}}, "numTraining": 2, "file_ending": ".png"}
    assert (root / "dataset.json").read_text() == json.dumps(want, indent=4)
    assert (root / "imagesTr" / "case_001_0000.png").read_bytes() == (src / "im1.png").read_bytes()             # a copy
    for k, out in ((0, root / "labelsTr" / "case_000.png"), (1, root / "labelsTr" / "case_001.png"), (2, root / "labelsTs" / "caseTs_000.png")):
        lab = Image.open(src / f"lb{k}.png").convert("L")
        img = Image.open(src / f"im{k}.png")
        if lab.size != img.size:
            lab = lab.resize(img.size, Image.NEAREST)
        lab = np.array(lab)
        expect = np.zeros_like(lab)
        for level, index in metrics.PIXEL_TO_LABEL.items():
            expect[lab == level] = index
        got = np.array(Image.open(out))
        assert got.dtype == np.uint8 and got.shape == (img.size[1], img.size[0]) and np.array_equal(got, expect), k
    assert utils.create_nnunet_dataset(tr_i, tr_l, te_i, te_l, 3, None, None, raw_dir=str(raw))[1] == "Dataset005_Custom"      # raw_dir wins; numbering goes on
