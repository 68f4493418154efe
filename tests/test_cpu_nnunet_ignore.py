"""CPU: the host side of nnU-Net's ignore label for the tissue head -- the float64 restatement of the masked loss (tests/nnunet_ignore_ref.py) against
values recorded from the reference's own modules (tests/golden/reference_dc_ce_loss_ignore.npz, scripts/gen_golden_dc_ce_loss_ignore.py), the
annotated-pixel locations against the reference's sampler (tests/golden/nnunet_class_locations_ignore.npz, scripts/gen_golden_nnunet_data_ignore.py),
the label rule, the patch choice of a store with an ignore label, and the dataset writer's `ignore_pixel`."""
import json
import os

import numpy as np
import pytest
import torch

import nnunet_ignore_ref as iref
from ldiffusion_amd import metrics, nnunet, nnunet_data as nd, nnunet_train

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
SCHEMES = ["ZScoreNormalization"] * 3


def fixtures():
    with open(os.path.join(GOLDEN, "nnunet_plans_2d.json")) as f:
        plans = json.load(f)
    with open(os.path.join(GOLDEN, "nnunet_dataset.json")) as f:
        ds = json.load(f)
    return plans, ds


# ---- 1. the loss -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "reference_dc_ce_loss_ignore.npz"))


def test_fixture_covers_what_the_issue_lists(golden):
    names = [str(c) for c in golden["cases"]]
    assert {int(golden[f"{n}.n_heads"]) for n in names} == {3, 9} and {bool(golden[f"{n}.batch_dice"]) for n in names} == {True, False}
    assert golden["n3.logits0"].shape == (2, 3, 24, 20) and golden["n9.logits1"].shape == (2, 9, 12, 10) and golden["n9.logits0"].dtype == np.float16
    kinds = {n.rsplit("_", 1)[1] for n in names}
    assert kinds == {"blobs", "image", "all", "none"}
    for n in names:
        k, t = int(golden[f"{n}.n_heads"]), golden[f"{n}.target0"]
        frac = (t == k).mean()
        if n.endswith("blobs"):
            assert 0.3 <= frac < 0.4
        elif n.endswith("image"):
            assert (t[1] == k).all() and not (t[0] == k).any()
        else:
            assert frac == (1.0 if n.endswith("all") else 0.0)
    assert os.path.getsize(os.path.join(GOLDEN, "reference_dc_ce_loss_ignore.npz")) < 100 * 1024


def _names():
    return [str(c) for c in np.load(os.path.join(GOLDEN, "reference_dc_ce_loss_ignore.npz"))["cases"]]


@pytest.mark.parametrize("name", _names())
def test_float64_restatement_against_the_reference_loss(golden, name):
    """The reference ran in float64, so the value agrees to float64 rounding (1e-13 relative asserted: sums of at most 960 terms).  The gradients were
    computed in float64 and stored rounded once to float32 (the fixture's size limit): the restatement agrees with the stored value to that one rounding,
    2^-24 relative, plus 1e-15 for float64's own.  Ignored pixels: exactly zero on both sides.  The restatement without the mask must NOT pass."""
    n, batch_dice = int(golden[f"{name}.n_heads"]), bool(golden[f"{name}.batch_dice"])
    weights = [float(w) for w in golden["weights"]]
    logits = [torch.from_numpy(golden[f"n{n}.logits{i}"].astype(np.float64)).requires_grad_(True) for i in range(2)]
    targets = [torch.from_numpy(golden[f"{name}.target{i}"].astype(np.int64)) for i in range(2)]
    loss = iref.deep_supervision_loss_ignore(logits, targets, weights, batch_dice, n)
    if loss.requires_grad:
        loss.backward()
    want = float(golden[f"{name}.loss"])
    assert abs(float(loss.detach()) - want) <= 1e-13 * max(1.0, abs(want)), (float(loss.detach()), want)
    for i, l in enumerate(logits):
        g_ref = torch.from_numpy(golden[f"{name}.grad{i}"].astype(np.float64))
        got = l.grad if l.grad is not None else torch.zeros_like(l)
        ignored = (targets[i] == n)[:, None].expand_as(got)
        assert not got[ignored].any() and not g_ref[ignored].any(), "an ignored pixel has a gradient"
        err = (got - g_ref).abs()
        assert (err <= 2.0 ** -24 * g_ref.abs() + 1e-15).all(), f"{name} scale {i}: max error {err.max():.3e}, gradient scale {g_ref.abs().max():.3e}"
    if name.endswith(("blobs", "image")):   # the plain loss with the ignored pixels called background is another number
        import nnunet_train_ref as ref
        plain = ref.deep_supervision_loss([l.detach() for l in logits], [torch.where(t == n, torch.zeros_like(t), t) for t in targets], weights, batch_dice)
        assert abs(float(plain) - want) > 1e-3
    if name.endswith("all"):
        assert want == -1.0


# ---- 2. the annotated locations -------------------------------------------------------------------------------------------------------------------
def test_sample_foreground_locations_with_the_annotated_key():
    g = np.load(os.path.join(GOLDEN, "nnunet_class_locations_ignore.npz"))
    n = int(g["n_heads"])
    assert int(g["ignore"]) == n and os.path.getsize(os.path.join(GOLDEN, "nnunet_class_locations_ignore.npz")) < 100 * 1024
    key = nd.annotated_key(n)
    assert key == (0, 1, 2)
    for name in ("a", "b"):
        seg = g[f"{name}.seg"]
        assert seg.shape == (40, 36)
        got = nd.sample_foreground_locations(seg, range(1, n), annotated=n)
        assert list(got) == [1, 2, key]
        plain = nd.sample_foreground_locations(seg, range(1, n))
        for c in (1, 2, key):
            want = g[f"{name}.locations_{'annotated' if c == key else c}"][:, 2:]
            assert len(got[c]) == len(want) and (len(want) == 0 or np.array_equal(np.asarray(got[c]), want)), (name, c)
            if c != key:   # the entries before the appended key keep their values
                assert len(plain[c]) == len(got[c]) and (len(want) == 0 or np.array_equal(plain[c], got[c]))
    assert len(g["a.locations_annotated"]) == int((g["a.seg"] < n).sum()) and len(g["b.locations_annotated"]) == 0 and (g["b.seg"] == n).all()


# ---- 3. the label rule -----------------------------------------------------------------------------------------------------------------------------
def test_label_rule():
    assert nnunet.label_spec({"background": 0, "a": 1, "b": 2}) == (3, None)
    assert nnunet.label_spec({"background": 0, "a": 1, "b": 2, "ignore": 3}) == (3, 3)
    for bad, what in (({"background": 0, "a": 1, "ignore": 1}, "highest"), ({"background": 0, "a": 1, "b": 2, "ignore": 2}, "highest"),
                      ({"background": 0, "a": 1, "ignore": 5}, "highest"), ({"background": 0, "a": 1, "ignore": 2.0}, "integer"),
                      ({"background": 0, "a": 1, "ignore": "2"}, "integer"), ({"background": 0, "a": 1, "ignore": True}, "integer"),
                      ({"background": 0, "a": 1, "ignore": [2]}, "regions"), ({"background": 0, "whole": [1, 2], "ignore": 3}, "regions")):
        with pytest.raises(ValueError, match="`labels`") as e:
            nnunet.label_spec(bad)
        assert what in str(e.value), (bad, str(e.value))
    plans, ds = fixtures()
    plain = nnunet.network_spec(plans, "2d_reduced", ds)
    assert "ignore_label" not in plain and plain == nnunet.network_spec(plans, "2d_reduced", ds, accept_ignore=True)
    ds["labels"]["ignore"] = 4
    with pytest.raises(ValueError, match="`labels`.*ignore"):
        nnunet.network_spec(plans, "2d_reduced", ds)           # not asked for: refused as before
    spec = nnunet.network_spec(plans, "2d_reduced", ds, accept_ignore=True)
    assert spec["ignore_label"] == 4 and spec["n_heads"] == 4 and {k: v for k, v in spec.items() if k != "ignore_label"} == plain
    ds["labels"]["ignore"] = 3
    with pytest.raises(ValueError, match="`labels`"):
        nnunet.network_spec(plans, "2d_reduced", ds, accept_ignore=True)


def test_trained_model_folder_round_trips_the_ignore_label(tmp_path):
    import nnunet_ref
    plans, ds = fixtures()
    ds["labels"]["ignore"] = 4
    spec = nnunet.network_spec(plans, "2d_reduced", ds, accept_ignore=True)
    folder = nnunet_ref.write_model_folder(str(tmp_path / "m"), plans, ds, nnunet_ref.synthetic_state_dict(spec, 1), spec, "2d_reduced")
    assert json.load(open(os.path.join(folder, "dataset.json")))["labels"]["ignore"] == 4
    got, sd, _ = nnunet.read_trained_model_folder(folder)
    heads = [k for k in sd if k.startswith("decoder.seg_layers.") and k.endswith(".weight")]
    assert got == spec and got["n_heads"] == 4 and heads and all(sd[k].shape[0] == 4 for k in heads)   # no head for the label: inference cannot emit it
    again = nnunet.write_trained_model_folder(str(tmp_path / "again"), plans, ds)
    assert open(os.path.join(again, "dataset.json")).read() == json.dumps(ds, indent=4)


def test_trainer_refuses_what_is_not_built():
    """Trainer's keyword exists and the data-parallel refusal names both sides; building a Trainer needs the GPU, so the rule is checked on the class."""
    import inspect
    assert inspect.signature(nnunet_train.Trainer.__init__).parameters["ignore_label"].default is None

    class Probe:
        ignore_label, ddp, world = 3, True, 2
    with pytest.raises(NotImplementedError, match=r"ddp=True, ignore_label=3.*world size 2"):
        nnunet_train.Trainer._check_ignore_ddp(Probe)
    Probe.world = 1
    nnunet_train.Trainer._check_ignore_ddp(Probe)
    Probe.world, Probe.ignore_label = 2, None
    nnunet_train.Trainer._check_ignore_ddp(Probe)


# ---- 4. the patch choice ---------------------------------------------------------------------------------------------------------------------------
def _cases(rng):
    """Two 40 x 56 cases with classes 0 .. 2 and the ignore label 3: one partly annotated, one with nothing annotated."""
    img = lambda: (rng.random((3, 40, 56)) * 255).astype(np.uint8)
    a = np.full((40, 56), 3, np.uint8)
    a[5:15, 4:30] = 0
    a[20:30, 30:50] = 1
    a[35:38, 2:6] = 2
    return [(img(), a), (img(), np.full((40, 56), 3, np.uint8))]


def parent_draw_crop(rng, store, sample_idx, batch_size, patch_size, loader_patch, oversample=nd.OVERSAMPLE_FOREGROUND):
    """draw_crop as it stood before the ignore label (the statements of the parent commit), for the comparison of a store without one."""
    ci = int(rng.integers(len(store)))
    lbs, ubs = nd.crop_bounds(store.shape(ci), loader_patch, patch_size)
    forced = nd.do_oversample(sample_idx, batch_size, oversample)
    eligible = [c for c, locs in store.class_locations[ci].items() if len(locs) > 0]
    voxel = None
    if forced and eligible:
        locs = store.class_locations[ci][eligible[int(rng.integers(len(eligible)))]]
        voxel = [int(v) for v in locs[int(rng.integers(len(locs)))]]
        bbox = [max(lbs[d], voxel[d] - loader_patch[d] // 2) for d in range(2)]
    else:
        bbox = [int(rng.integers(lbs[d], ubs[d] + 1)) for d in range(2)]
    return dict(case=ci, forced=forced, voxel=voxel, lbs=lbs, ubs=ubs, bbox_lbs=bbox, loader_patch=tuple(int(v) for v in loader_patch))


def test_draw_crop_with_an_ignore_label():
    labels = {"background": 0, "a": 1, "b": 2, "ignore": 3}
    store = nd.CaseStore(_cases(np.random.default_rng(3)), SCHEMES, 3, device="cpu", labels=labels)
    key = nd.annotated_key(3)
    assert store.ignore_label == 3 and list(store.class_locations[0]) == [1, 2, key] and all(len(v) == 0 for v in store.class_locations[1].values())
    annotated = {tuple(v) for v in np.argwhere(_cases(np.random.default_rng(3))[0][1] < 3)}
    assert {tuple(v) for v in store.class_locations[0][key]} == annotated          # fewer than 10000: every annotated pixel is recorded
    fg = {tuple(v) for c in (1, 2) for v in store.class_locations[0][c]}
    rng = np.random.default_rng(11)
    patch, loader_patch, seen = (16, 16), (24, 24), {"bg_centre": 0, "free": 0, "forced": 0}
    for k in range(4000):
        idx = k % 4                                           # batch of 4 at 0.33: samples 0, 1, 2 are free, sample 3 is forced
        c = nd.draw_crop(rng, store, idx, 4, patch, loader_patch)
        assert c["forced"] == (idx == 3)
        if c["case"] == 1:                                    # nothing annotated: the free crop, forced or not
            assert c["voxel"] is None and all(c["lbs"][d] <= c["bbox_lbs"][d] <= c["ubs"][d] for d in range(2))
            seen["free"] += 1
            continue
        v = tuple(c["voxel"])
        assert c["bbox_lbs"] == [max(c["lbs"][d], v[d] - loader_patch[d] // 2) for d in range(2)]
        if c["forced"]:                                       # a class is present: never the annotated key, so never a background pixel
            assert v in fg
            seen["forced"] += 1
        else:
            assert v in annotated
            seen["bg_centre"] += v not in fg
    assert min(seen.values()) > 100, seen                     # every branch ran, and free samples do land on annotated background
    only_bg = np.full((40, 56), 3, np.uint8)
    only_bg[3:9, 3:9] = 0                                     # background strokes alone: the annotated key is a forced sample's only entry, and is taken
    s2 = nd.CaseStore([(_cases(np.random.default_rng(3))[0][0], only_bg)], SCHEMES, 3, device="cpu", labels=labels)
    c = nd.draw_crop(np.random.default_rng(1), s2, 3, 4, patch, loader_patch)
    assert c["forced"] and 3 <= c["voxel"][0] < 9 and 3 <= c["voxel"][1] < 9
    with pytest.raises(ValueError, match=r"labels \[4\] outside"):
        nd.CaseStore([(_cases(np.random.default_rng(3))[0][0], np.where(only_bg == 0, 4, only_bg))], SCHEMES, 3, device="cpu", labels=labels)
    with pytest.raises(ValueError, match="ignore"):
        nd.CaseStore(_cases(np.random.default_rng(3)), SCHEMES, 4, device="cpu", labels=labels)   # the label must be the first value past the classes


def test_a_store_without_an_ignore_label_draws_what_it_drew():
    rng = np.random.default_rng(5)
    cases = []
    for H, W, fg in ((40, 56, True), (33, 47, True), (50, 50, False)):
        seg = np.zeros((H, W), np.uint8)
        if fg:
            seg[H // 4:H // 2, W // 3:W // 2] = 1
            seg[H // 2:, : W // 4] = 3
        cases.append(((rng.random((3, H, W)) * 255).astype(np.uint8), seg))
    for labels in (None, {"background": 0, "a": 1, "b": 2, "c": 3}):
        store = nd.CaseStore(cases, SCHEMES, 4, device="cpu", labels=labels)
        assert store.ignore_label is None and all(list(cl) == [1, 2, 3] for cl in store.class_locations)
        a, b = np.random.default_rng(21), np.random.default_rng(21)
        for k in range(3000):
            assert nd.draw_crop(a, store, k % 6, 6, (16, 24), (24, 32)) == parent_draw_crop(b, store, k % 6, 6, (16, 24), (24, 32))
        assert a.integers(1 << 30) == b.integers(1 << 30)     # and the streams stand at the same place
    # a whole batch: the tables of the parent's draw order (draw_sample with the parent's crop patched in) are the tables of today
    store = nd.CaseStore(cases, SCHEMES, 4, device="cpu")
    s1, c1 = nd.draw_batch(np.random.default_rng(8), store, 6, (16, 24))
    saved = nd.draw_crop
    nd.draw_crop = parent_draw_crop
    try:
        s2, c2 = nd.draw_batch(np.random.default_rng(8), store, 6, (16, 24))
    finally:
        nd.draw_crop = saved
    assert s1.tobytes() == s2.tobytes() and c1.tobytes() == c2.tobytes()


# ---- 5. the dataset writer -------------------------------------------------------------------------------------------------------------------------
def _write_sources(src, ignore_level=None):
    from PIL import Image
    rng = np.random.RandomState(5)
    src.mkdir()
    levels = np.array(sorted(metrics.PIXEL_TO_LABEL), np.uint8)
    images, labels = [], []
    for k, (h, w) in enumerate([(20, 24), (22, 24), (20, 24)]):          # mixed sizes: plain copies, no sampler runs (as tests/test_cpu_nnunet_plan.py)
        Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(src / f"im{k}.png")
        lab = levels[rng.randint(0, len(levels), (h, w))]
        lab[0, 0] = 77                                                   # a grey level the table does not name -> 0
        if ignore_level is not None:
            lab[5:12, 3:17] = ignore_level
        Image.fromarray(lab).save(src / f"lb{k}.png")
        images.append(str(src / f"im{k}.png"))
        labels.append(str(src / f"lb{k}.png"))
    return images, labels


def _tree(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(root) for f in fs}


def test_create_nnunet_dataset_ignore_pixel(tmp_path):
    from PIL import Image
    from ldiffusion_amd import utils
    level = next(g for g in range(255, 0, -1) if g not in metrics.PIXEL_TO_LABEL and g != 77)
    images, labels = _write_sources(tmp_path / "src", level)
    raws = {}
    for name in ("plain", "none", "ignore"):
        raws[name] = tmp_path / name
        raws[name].mkdir()
    utils.create_nnunet_dataset(images[:2], labels[:2], images[2:], labels[2:], 7, None, None, raw_dir=str(raws["plain"]))
    utils.create_nnunet_dataset(images[:2], labels[:2], images[2:], labels[2:], 7, None, None, raw_dir=str(raws["none"]), ignore_pixel=None)
    num, name = utils.create_nnunet_dataset(images[:2], labels[:2], images[2:], labels[2:], 7, None, None, raw_dir=str(raws["ignore"]), ignore_pixel=level)
    assert (num, name) == (1, "Dataset001_Custom")
    plain, none, ign = (_tree(str(raws[k])) for k in ("plain", "none", "ignore"))
    assert plain == none                                                  # None: every byte written is the call's without the keyword
    want = {"channel_names": {"0": "R", "1": "G", "2": "B"}, "labels": {"background": 0, **{f"class{i}": i for i in range(1, 7)}}, "numTraining": 2, "file_ending": ".png"}
    assert plain["Dataset001_Custom/dataset.json"].decode() == json.dumps(want, indent=4)      # ... and the JSON is the parent's, stated here
    want["labels"]["ignore"] = 7
    assert ign["Dataset001_Custom/dataset.json"].decode() == json.dumps(want, indent=4)
    assert nnunet.label_spec(json.loads(ign["Dataset001_Custom/dataset.json"])["labels"]) == (7, 7)
    assert set(ign) == set(plain) and all(ign[k] == plain[k] for k in plain if "/images" in k)
    for k, out in ((0, "labelsTr/case_000.png"), (1, "labelsTr/case_001.png"), (2, "labelsTs/caseTs_000.png")):
        lab = np.array(Image.open(labels[k]).convert("L"))
        expect = np.zeros_like(lab)
        for g, index in metrics.PIXEL_TO_LABEL.items():
            expect[lab == g] = index
        assert np.array_equal(np.array(Image.open(raws["plain"] / "Dataset001_Custom" / out)), expect)       # the ignored level reads as background without the keyword
        expect[lab == level] = 7
        got = np.array(Image.open(raws["ignore"] / "Dataset001_Custom" / out))
        assert got.dtype == np.uint8 and np.array_equal(got, expect) and (got[5:12, 3:17] == 7).all() and got[0, 0] == 0
    mapped = next(iter(metrics.PIXEL_TO_LABEL))
    for bad in (mapped, 256, -1, 3.5, True):
        with pytest.raises(ValueError, match="ignore_pixel"):
            utils.create_nnunet_dataset(images[:2], labels[:2], images[2:], labels[2:], 7, None, None, raw_dir=str(raws["ignore"]), ignore_pixel=bad)
    assert sorted(os.listdir(raws["ignore"])) == ["Dataset001_Custom"]   # a refused call writes nothing


def test_public_surface_names_the_keyword():
    import inspect
    from ldiffusion_amd import autograd as ag, ldiffusion, utils
    from ldiffusion_amd.segmentor import Segmentor
    for fn in (utils.create_nnunet_dataset, Segmentor.train_tissue_model_nnUNetv2, ldiffusion.LDiffusionModel.train):
        assert inspect.signature(fn).parameters["ignore_pixel"].default is None
    for fn in (ag.dice_ce, ag.dice_ce_stats, ag.dice_ce_from_sums, ag.DiceCeFn.forward, ag.DiceCeSumsFn.forward, ag.dice_ce_nacc):
        assert inspect.signature(fn).parameters["ignore_label"].default is None
    base = ["--diffusion-path", "sd", "--image-dir", "i", "--label-dir", "l", "--num-epochs", "20", "--batch-size", "2", "--num-inference-steps", "5", "--num-classes", "7"]
    assert ldiffusion.parse_args(base).ignore_pixel is None and ldiffusion.parse_args(base + ["--ignore-pixel", "200"]).ignore_pixel == 200
    assert ag.dice_ce_nacc(4) == 26 and ag.dice_ce_nacc(4, 4) == 27 and ag.dice_ce_nacc(9, 9) == 51
