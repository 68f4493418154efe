"""CPU: the host side of region labels for the tissue head -- the float64 restatement of the region losses (tests/nnunet_region_ref.py) and the label
rule `nnunet.region_spec` against values recorded from the reference's own modules (tests/golden/reference_dc_focal_loss.npz,
scripts/gen_golden_dc_focal_loss.py), the membership table, the refusals, the trained-model folder, the two thresholds of `sigmoid(.) > 0.5`, and the
new entry points' prototypes."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nnunet_region_ref as rref
from ldiffusion_amd import _lib, autograd as ag, nnunet, nnunet_data as nd, nnunet_train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
NPZ = os.path.join(GOLDEN, "reference_dc_focal_loss.npz")


def fixtures():
    with open(os.path.join(GOLDEN, "nnunet_plans_2d.json")) as f:
        plans = json.load(f)
    with open(os.path.join(GOLDEN, "nnunet_dataset.json")) as f:
        ds = json.load(f)
    return plans, ds


REGION_LABELS = {"background": 0, "whole": [1, 2, 3], "core": [2, 3], "enhancing": 3}


def region_dataset(ignore=False, order=(1, 2, 3)):
    plans, ds = fixtures()
    ds["labels"] = dict(REGION_LABELS, **({"ignore": 4} if ignore else {}))
    ds["regions_class_order"] = list(order)
    return plans, ds


@pytest.fixture(scope="module")
def golden():
    return np.load(NPZ)


# ---- 1. the loss -----------------------------------------------------------------------------------------------------------------------------------
def test_fixture_covers_what_the_issue_lists(golden):
    names = {str(c) for c in golden["cases"]}
    assert names == {f"{f}_{i}_{b}" for f in ("focal", "bce") for i in ("plain", "ignore") for b in ("batch", "sample")}
    assert golden["logits"].shape == (2, 3, 6, 5) and golden["logits"].dtype == np.float16
    assert golden["seg"].max() == 3 and 0.3 <= (golden["seg_ignore"] == 4).mean() < 0.5
    assert [str(n) for n in golden["lm.names"]] == ["plain", "with_zero", "permuted"]
    assert "torch.nn.functional" in str(golden["provenance"]) and "NameError" in str(golden["provenance"])
    assert os.path.getsize(NPZ) < 100 * 1024


def _names():
    return [str(c) for c in np.load(NPZ)["cases"]]


@pytest.mark.parametrize("name", _names())
def test_float64_restatement_against_the_reference_loss(golden, name):
    """Both sides ran in float64 on 2 x 3 x 6 x 5 elements: value and gradient agree to float64 rounding (1e-13 relative to 1 asserted).  Ignored pixels'
    gradients are exactly zero on both sides.  The wrong variants and the other form give other numbers."""
    form, ign, bd = name.split("_")
    use_ignore, batch_dice = ign == "ignore", bd == "batch"
    labels = json.loads(str(golden["labels_ignore" if use_ignore else "labels"]))
    rs = nnunet.region_spec(labels, [int(c) for c in golden["regions_class_order"]])
    target = torch.from_numpy(golden["seg_ignore" if use_ignore else "seg"].astype(np.int64))
    z = torch.from_numpy(golden["logits"].astype(np.float64)).requires_grad_(True)
    loss = rref.dc_focal_loss(z, target, rs["table"], batch_dice, use_ignore, form)
    loss.backward()
    want, gwant = float(golden[f"{name}.loss"]), torch.from_numpy(golden[f"{name}.grad"])
    assert abs(float(loss.detach()) - want) <= 1e-13 * max(1.0, abs(want))
    assert ((z.grad - gwant).abs() <= 1e-13 * gwant.abs() + 1e-16).all()
    if use_ignore:
        ignored = (target == 4)[:, None].expand_as(gwant)
        assert ignored.any() and not z.grad[ignored].any() and not gwant[ignored].any()
    other = {"focal": "bce", "bce": "focal"}[form]
    for kw in (dict(form=other), dict(form=form, wrong="norm"), dict(form=form, wrong="M")) + ((dict(form=form, wrong="dice_all"),) if use_ignore else ()):
        assert abs(float(rref.dc_focal_loss(z.detach(), target, rs["table"], batch_dice, use_ignore, **kw)) - want) > 1e-3, kw


def test_the_two_normalisers_differ_by_the_factor_R(golden):
    """compound_losses.py:202 divides the masked sum by the count of annotated PIXELS, :204 takes the mean over B R H W elements: on a target without an
    ignored pixel the focal term of the ignore form is R times the plain one.  The Dice terms are equal."""
    rs = nnunet.region_spec(json.loads(str(golden["labels_ignore"])), [1, 2, 3])
    target = torch.from_numpy(golden["seg"].astype(np.int64))
    z = torch.from_numpy(golden["logits"].astype(np.float64))
    plain = float(golden["focal_plain_batch.loss"])
    with_ignore = float(rref.dc_focal_loss(z, target, rs["table"], True, True, "focal"))
    focal = (with_ignore - plain) / 2   # (3 f - d) - (f - d) = 2 f
    bce = F.binary_cross_entropy_with_logits(z, rref.membership(target, rs["table"], 3)[0], reduction="none")
    p_t = torch.exp(-bce)
    assert abs(focal - float((0.25 * (1 - p_t) ** 2 * bce).mean())) <= 1e-13 and focal > 1e-3
    assert abs(with_ignore - float(rref.dc_focal_loss(z, target, rs["table"], True, False, "focal", wrong="norm"))) <= 1e-13


# ---- 2. the label rule -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plain", "with_zero", "permuted"])
def test_region_spec_against_label_manager(golden, name):
    labels, order = json.loads(str(golden[f"lm.{name}.labels"])), [int(c) for c in golden[f"lm.{name}.order"]]
    rs = nnunet.region_spec(labels, order)
    want_regions = [tuple(r) if isinstance(r, list) else r for r in json.loads(str(golden[f"lm.{name}.foreground_regions"]))]
    assert rs["foreground_regions"] == want_regions and rs["n_heads"] == int(golden[f"lm.{name}.num_segmentation_heads"]) == len(want_regions)
    assert rs["all_labels"] == [int(v) for v in golden[f"lm.{name}.all_labels"]]
    ignore = int(golden[f"lm.{name}.ignore_label"])
    assert rs["ignore_label"] == (None if ignore < 0 else ignore) and rs["regions_class_order"] == order
    table = rs["table"]
    assert table.dtype == np.uint32 and table.shape == (256,)
    for v in range(256):   # the table by its definition
        want = 0
        if v == rs["ignore_label"]:
            want = 1 << 31
        elif v not in rs["all_labels"]:
            want = 1 << 30
        else:
            for r, region in enumerate(want_regions):
                want |= (v in (region if isinstance(region, tuple) else (region,))) << r
        assert int(table[v]) == want, v
    logits = torch.from_numpy(golden["lm.logits"])
    seg = rref.region_segmentation(logits, order, nnunet.REGION_THRESHOLD_F32)
    assert torch.equal(seg, torch.from_numpy(golden[f"lm.{name}.segmentation"])) and set(seg.unique().tolist()) <= set(order) | {0}


def test_region_spec_refusals():
    ok = dict(REGION_LABELS)
    assert nnunet.region_spec(ok, [1, 2, 3])["n_heads"] == 3
    assert nnunet.region_spec(dict(ok, zero=[0, 0]), [1, 2, 3])["n_heads"] == 3, "a region that is only background is dropped"
    assert nnunet.region_spec(dict(ok, ignore=4), [1, 2, 3])["ignore_label"] == 4
    for labels, order, field, what in ((ok, None, "regions_class_order", "missing"), (ok, [1, 2], "regions_class_order", "2 entries for 3"),
                                       (ok, [1, 2, 3, 4], "regions_class_order", "4 entries for 3"), (ok, [1, 2, 300], "regions_class_order", "0 .. 255"),
                                       (dict(ok, ignore=5), [1, 2, 3], "labels", "max(all labels) + 1 = 4"), (dict(ok, ignore=3), [1, 2, 3], "labels", "highest"),
                                       (dict(ok, ignore=[4]), [1, 2, 3], "labels", "integer"), (dict(ok, ignore=4.0), [1, 2, 3], "labels", "integer"),
                                       ({"whole": [1, 2]}, [1], "labels", "background"),
                                       (dict({"background": 0}, **{f"r{i}": [i + 1, i + 2] for i in range(25)}), list(range(25)), "labels", "25 regions")):
        with pytest.raises(ValueError) as e:
            nnunet.region_spec(labels, order)
        assert f"`{field}`" in str(e.value) and what in str(e.value), (labels, str(e.value))
    many = dict({"background": 0}, **{f"r{i}": [i + 1, i + 2] for i in range(24)})
    assert nnunet.region_spec(many, list(range(24)))["n_heads"] == 24


def test_network_spec_takes_regions_only_with_the_keyword():
    plans, ds = region_dataset()
    with pytest.raises(ValueError, match="`labels` defines regions"):
        nnunet.network_spec(plans, "2d_reduced", ds)
    with pytest.raises(ValueError, match="`labels` defines regions"):
        nnunet.network_spec(plans, "2d_reduced", ds, accept_ignore=True)
    with pytest.raises(ValueError, match="regions"):
        nnunet.label_spec(ds["labels"])
    spec = nnunet.network_spec(plans, "2d_reduced", ds, accept_regions=True)
    assert spec["n_heads"] == 3 and spec["regions"] == [(1, 2, 3), (2, 3), 3] and spec["regions_class_order"] == [1, 2, 3] and "ignore_label" not in spec
    assert np.array_equal(spec["region_table"], nnunet.region_spec(ds["labels"], [1, 2, 3])["table"])
    plans, ds = region_dataset(ignore=True, order=(3, 1, 2))
    spec = nnunet.network_spec(plans, "2d_reduced", ds, accept_regions=True)
    assert spec["ignore_label"] == 4 and spec["regions_class_order"] == [3, 1, 2] and int(spec["region_table"][4]) == 1 << 31
    del ds["regions_class_order"]
    with pytest.raises(ValueError, match="`regions_class_order` is missing"):
        nnunet.network_spec(plans, "2d_reduced", ds, accept_regions=True)
    plans, plain = fixtures()   # the keyword changes nothing for plain labels
    assert nnunet.network_spec(plans, "2d_reduced", plain, accept_regions=True) == nnunet.network_spec(plans, "2d_reduced", plain)


def test_trained_model_folder_round_trips_region_labels(tmp_path):
    import nnunet_ref
    plans, ds = region_dataset(ignore=True, order=(3, 1, 2))
    spec = nnunet.network_spec(plans, "2d_reduced", ds, accept_regions=True)
    folder = nnunet_ref.write_model_folder(str(tmp_path / "m"), plans, ds, nnunet_ref.synthetic_state_dict(spec, 1), spec, "2d_reduced")
    got, sd, _ = nnunet.read_trained_model_folder(folder)   # no opt-in to load a folder somebody trained on purpose
    assert set(got) == set(spec) and all(np.array_equal(got[k], spec[k]) if k == "region_table" else got[k] == spec[k] for k in spec)
    heads = [k for k in sd if k.startswith("decoder.seg_layers.") and k.endswith(".weight")]
    assert heads and all(sd[k].shape[0] == 3 for k in heads)
    again = nnunet.write_trained_model_folder(str(tmp_path / "again"), plans, ds)
    text = open(os.path.join(again, "dataset.json")).read()
    assert text == json.dumps(ds, indent=4) and '"regions_class_order"' in text and json.loads(text)["labels"]["whole"] == [1, 2, 3]


def test_case_store_labels_keyword_still_refuses_regions():
    img = torch.zeros((3, 8, 8), dtype=torch.uint8)
    with pytest.raises(ValueError, match="`labels` defines regions"):
        nd.CaseStore([(img, np.zeros((8, 8), np.uint8))], ["ZScoreNormalization"] * 3, 3, device="cpu", labels=dict(REGION_LABELS))


# ---- 3. the thresholds -----------------------------------------------------------------------------------------------------------------------------
def test_thresholds_of_sigmoid_above_one_half():
    """`sigmoid(l) > 0.5` is a step function of the logit; the constants are the largest logit that still compares false, found again here with torch on
    the CPU: float16 by enumeration of every finite value (validation: the sigmoid of the network's float16 output), float32 by bisection (inference:
    sigmoid(l.float())), with the step's neighbourhood enumerated."""
    assert rref.step_of_sigmoid_f16() == nnunet.REGION_THRESHOLD_F16
    assert rref.step_of_sigmoid_f32() == nnunet.REGION_THRESHOLD_F32
    t = torch.tensor([nnunet.REGION_THRESHOLD_F32], dtype=torch.float32)
    up = (t.view(torch.int32) + 1).view(torch.float32)
    assert float(t) == nnunet.REGION_THRESHOLD_F32, "the constant is a float32"
    assert not bool(torch.sigmoid(t) > 0.5) and bool(torch.sigmoid(up) > 0.5)
    lo, hi = (int(torch.tensor([v], dtype=torch.float32).view(torch.int32)) for v in (2.0 ** -27, 2.0 ** -21))
    x = torch.arange(lo, hi, dtype=torch.int32).view(torch.float32)
    assert torch.equal(torch.sigmoid(x) > 0.5, x > nnunet.REGION_THRESHOLD_F32)
    h = torch.tensor([nnunet.REGION_THRESHOLD_F16], dtype=torch.float16)
    assert float(h) == nnunet.REGION_THRESHOLD_F16 and not bool(torch.sigmoid(h) > 0.5) and bool(torch.sigmoid((h.view(torch.int16) + 1).view(torch.float16)) > 0.5)


# ---- 4. the library's surface ------------------------------------------------------------------------------------------------------------------------
NEW = ("ldiff_op_dice_focal_ws_bytes", "ldiff_op_dice_focal_nacc", "ldiff_op_dice_focal", "ldiff_op_dice_focal_stats", "ldiff_op_dice_focal_from_sums",
       "ldiff_op_region_counts_ws_bytes", "ldiff_op_region_counts", "ldiff_op_region_mask_u8")


def test_prototypes_and_exports_of_the_new_entry_points():
    with open(os.path.join(ROOT, "include", "ldiff.h")) as f:
        header = f.read()
    lib = _lib.load()
    kinds = {"int": C.c_int, "float": C.c_float, "int64_t": C.c_int64}
    for name in NEW:
        m = re.search(r"(\w+)\s+" + name + r"\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/ldiff.h"
        res, args = _lib.SIGNATURES[name]
        assert res is kinds[m.group(1)] and hasattr(lib, name)
        want = [C.c_void_p if "*" in a else kinds[a.split()[-2]] for a in (a.strip() for a in m.group(2).split(","))]
        assert args == want, f"{name}: {args} against the header's {want}"
    with open(os.path.join(ROOT, "ldiffusion_amd", "csrc", "kernels_segregion.hip")) as f:
        src = f.read()
    assert not re.search(r"atomic\w*\s*\(", src), "the region kernels reduce through partials in a fixed order"
    assert lib.ldiff_op_dice_focal_nacc(3) == ag.dice_focal_nacc(3) == 27 and lib.ldiff_op_dice_focal_nacc(9) == ag.dice_focal_nacc(9) == 51
    assert lib.ldiff_op_dice_focal_nacc(25) == 0 and lib.ldiff_op_dice_focal_ws_bytes(2, 5184, 25) == 0
    chunks = 2   # 72 x 72 pixels in workgroups of 4096
    assert lib.ldiff_op_dice_focal_ws_bytes(2, 5184, 3) == (2 * 27 + 2 * 8) * 8 + (2 * 8 * 2 + 1 + 2 * chunks * 27) * 4
    assert lib.ldiff_op_region_counts_ws_bytes(2, 5184, 9) == 2 * chunks * 3 * 16 * 4


def test_python_surface():
    import inspect
    for name in ("dice_focal", "dice_focal_stats", "dice_focal_from_sums", "DiceFocalFn", "DiceFocalSumsFn", "region_counts"):
        assert hasattr(ag, name)
    assert inspect.signature(nnunet_train.Trainer.__init__).parameters["region_loss"].default == "focal"
    assert inspect.signature(nnunet.network_spec).parameters["accept_regions"].default is False
    t = nnunet.region_table_tensor(nnunet.region_spec(dict(REGION_LABELS, ignore=4), [1, 2, 3])["table"])
    assert t.dtype == torch.int32 and t.shape == (256,) and int(t[4]) == -(1 << 31) and int(t[3]) == 7 and int(t[5]) == 1 << 30


# ---- 5. the store ----------------------------------------------------------------------------------------------------------------------------------
def test_region_sampling_planes_on_a_cpu_store():
    """class_locations is keyed by the foreground regions (and, with an ignore label, ends with tuple(all_labels)); a region of at most 10000 pixels is
    sampled whole, so its sorted locations are np.argwhere of its membership plane; the walk is sample_foreground_locations' own."""
    rs = nnunet.region_spec(dict(REGION_LABELS, ignore=4), [1, 2, 3])
    rng = np.random.default_rng(5)
    seg = np.kron(rng.integers(0, 5, (10, 9)), np.ones((4, 4), np.int64)).astype(np.uint8)
    img = torch.from_numpy(rng.integers(1, 256, (3, 40, 36)).astype(np.uint8))
    empty = np.full((40, 36), 4, np.uint8)
    store = nd.CaseStore([(img, seg), (img, empty)], ["ZScoreNormalization"] * 3, 3, device="cpu", regions=rs)
    keys = [(1, 2, 3), (2, 3), 3, (0, 1, 2, 3)]
    assert store.regions == keys[:3] and store.ignore_label == 4 and store.annotated == keys[3] and torch.equal(store.labels(0), torch.from_numpy(seg))
    assert list(store.class_locations[0]) == keys and all(len(store.class_locations[1][k]) == 0 for k in keys)
    want = nd.sample_foreground_locations(seg, keys[:3], annotated=keys[3])
    for k in keys:
        got = np.asarray(store.class_locations[0][k])
        plane = np.isin(seg, k)
        assert np.array_equal(got, want[k]) and np.array_equal(got[np.lexsort((got[:, 1], got[:, 0]))], np.argwhere(plane)) and len(got) > 0, k
    rng2 = np.random.default_rng(3)
    for idx in range(8):   # the patch choice goes through the annotated key of a region store
        crop = nd.draw_crop(rng2, store, idx, 8, (16, 16), (16, 16))
        assert crop["case"] == 1 or crop["voxel"] is not None
    bad = seg.copy()
    bad[0, 0] = 9
    with pytest.raises(ValueError, match=r"labels \[9\] outside"):
        nd.CaseStore([(img, bad)], ["ZScoreNormalization"] * 3, 3, device="cpu", regions=rs)
    gap = nnunet.region_spec({"background": 0, "a": [1, 3], "b": 3}, [1, 2])
    with pytest.raises(ValueError, match=r"labels \[2\] are no labels"):
        nd.CaseStore([(img, np.where(seg > 3, 0, seg).astype(np.uint8))], ["ZScoreNormalization"] * 3, 2, device="cpu", regions=gap)
    with pytest.raises(ValueError, match="3 regions, n_heads is 4"):
        nd.CaseStore([(img, seg)], ["ZScoreNormalization"] * 3, 4, device="cpu", regions=rs)


# ---- 6. the stage's keywords -------------------------------------------------------------------------------------------------------------------------
def test_stage_keywords_and_the_dataset_writer(tmp_path):
    import inspect
    from PIL import Image
    from ldiffusion_amd import ldiffusion, utils
    from ldiffusion_amd.segmentor import Segmentor
    for fn in (utils.create_nnunet_dataset, Segmentor.train_tissue_model_nnUNetv2, ldiffusion.LDiffusionModel.train):
        p = inspect.signature(fn).parameters
        assert p["regions"].default is None and p["regions_class_order"].default is None
    base = ["--diffusion-path", "sd", "--image-dir", "i", "--label-dir", "l", "--num-epochs", "20", "--batch-size", "2", "--num-inference-steps", "5", "--num-classes", "7"]
    assert ldiffusion.parse_args(base).regions is None and ldiffusion.parse_args(base + ["--regions", "r.json"]).regions == "r.json"
    rng = np.random.RandomState(2)
    levels = np.array([0, 100, 150, 50], np.uint8)
    images, labels = [], []
    for i, size in enumerate(((16, 16), (16, 24))):   # mixed sizes: plain copies, no sampler
        Image.fromarray(rng.randint(1, 256, size + (3,)).astype(np.uint8)).save(tmp_path / f"im{i}.png")
        Image.fromarray(levels[rng.randint(0, 4, size)]).save(tmp_path / f"lb{i}.png")
        images.append(str(tmp_path / f"im{i}.png"))
        labels.append(str(tmp_path / f"lb{i}.png"))
    raw = tmp_path / "raw"
    raw.mkdir()
    plain = utils.create_nnunet_dataset(images, labels, images[:1], labels[:1], 4, None, None, raw_dir=str(raw))
    by_index = utils.create_nnunet_dataset(images, labels, images[:1], labels[:1], 4, None, None, raw_dir=str(raw), regions={"whole": [1, 2, 3], "core": [2, 3]},
                                           regions_class_order=[1, 2], ignore_pixel=25)
    by_level = utils.create_nnunet_dataset(images, labels, images[:1], labels[:1], 4, None, None, raw_dir=str(raw), regions={"whole": [100, 150, 50], "core": [150, 50]},
                                           regions_class_order=[1, 2])
    read = lambda name: json.loads((raw / name[1] / "dataset.json").read_text())
    assert "regions_class_order" not in read(plain) and read(plain)["labels"] == {"background": 0, "class1": 1, "class2": 2, "class3": 3}
    assert read(by_index)["labels"] == {"background": 0, "whole": [1, 2, 3], "core": [2, 3], "ignore": 4} and read(by_index)["regions_class_order"] == [1, 2]
    assert read(by_level)["labels"] == {"background": 0, "whole": [1, 2, 3], "core": [2, 3]}
    for name in (by_index, by_level):   # the label PNGs keep class indices
        assert (raw / name[1] / "labelsTr" / "case_000.png").read_bytes() == (raw / plain[1] / "labelsTr" / "case_000.png").read_bytes()
    for kw, what in ((dict(regions={"core": [2, 3]}, regions_class_order=[2]), "lie in no region"), (dict(regions={"whole": [1, 2, 3]}), "regions_class_order"),
                     (dict(regions={"whole": [1, 2, 3, 7]}, regions_class_order=[1]), "neither class"), (dict(regions_class_order=[1]), "without `regions`")):
        with pytest.raises(ValueError, match=what):
            utils.create_nnunet_dataset(images, labels, images[:1], labels[:1], 4, None, None, raw_dir=str(raw), **kw)
    assert len(os.listdir(raw)) == 3, "a refused call writes nothing"


def test_train_hands_the_region_keywords_to_the_stage(tmp_path, monkeypatch):
    """LDiffusionModel.train(component="segmentor") at the tissue level: `regions` / `regions_class_order` / `region_loss` as keywords, or read from the JSON file
    `--regions` names, reach Segmentor.train_tissue_model_nnUNetv2; without them the call carries none of the three."""
    import types
    from ldiffusion_amd import ldiffusion, segmentor
    seen = []

    class Probe:
        def __init__(self, *a, **k):
            pass

        def train_tissue_model_nnUNetv2(self, epochs, weight, path, **kw):
            seen.append((epochs, kw))
            return "folder"

    monkeypatch.setattr(ldiffusion, "Segmentor", Probe)
    model = ldiffusion.LDiffusionModel.__new__(ldiffusion.LDiffusionModel)
    model.level = "tissue"
    model._is_main_process = lambda: False
    lists = dict(train_images=["a"], train_labels=["b"], test_images=["c"], test_labels=["d"])
    regions = {"whole": [1, 2, 3], "core": [2, 3]}
    args = types.SimpleNamespace(num_epochs=12, diffusion_path="sd", num_classes=4)
    assert model.train(args, component="segmentor", ldiffusion_weight="w", train_loader=[], val_loader=[], **lists) == "folder"
    assert seen[-1] == (2, lists)
    model.train(args, component="segmentor", ldiffusion_weight="w", train_loader=[], val_loader=[], regions=regions, regions_class_order=[1, 2], **lists)
    assert seen[-1][1] == dict(lists, regions=regions, regions_class_order=[1, 2])
    model.train(args, component="segmentor", ldiffusion_weight="w", train_loader=[], val_loader=[], regions=regions, regions_class_order=[1, 2], region_loss="bce", **lists)
    assert seen[-1][1]["region_loss"] == "bce"
    path = tmp_path / "regions.json"
    path.write_text(json.dumps({"regions": regions, "regions_class_order": [2, 1]}))
    base = ["--diffusion-path", "sd", "--image-dir", "i", "--label-dir", "l", "--num-epochs", "12", "--batch-size", "2", "--num-inference-steps", "5", "--num-classes", "4"]
    parsed = ldiffusion.parse_args(base + ["--regions", str(path)])
    parsed.image_dir = parsed.label_dir = None   # the lists are given: no loader is built
    model.train(parsed, component="segmentor", ldiffusion_weight="w", train_loader=[], val_loader=[], **lists)
    assert seen[-1][1] == dict(lists, regions=regions, regions_class_order=[2, 1])


def test_single_valued_lists_are_plain_labels_to_nnunet():
    """LabelManager.has_regions needs an entry of more than one value: {"top": [1]} alone is read as plain classes.  region_spec refuses such a mapping, so
    create_nnunet_dataset writes no dataset the stage would then refuse, and network_spec(accept_regions=True) refuses it as label_spec does."""
    from ldiffusion_amd import utils
    with pytest.raises(ValueError, match="`labels` defines no region of more than one value"):
        nnunet.region_spec({"background": 0, "top": [1]}, [1])
    plans, ds = fixtures()
    ds["labels"], ds["regions_class_order"] = {"background": 0, "top": [1]}, [1]
    with pytest.raises(ValueError, match="`labels` defines regions"):
        nnunet.network_spec(plans, "2d_reduced", ds, accept_regions=True)
    with pytest.raises(ValueError, match="no region of more than one value"):
        utils.create_nnunet_dataset([], [], [], [], 2, None, None, raw_dir="does-not-matter", regions={"top": [1]}, regions_class_order=[1])
    assert nnunet.region_spec({"background": 0, "any": [1, 2], "top": [2]}, [1, 2])["foreground_regions"] == [(1, 2), (2,)]
