"""Final validation and largest-component postprocessing of the tissue head, without a GPU: the numpy restatement the GPU tests compare against
(tests/nnunet_post_ref.py) is itself checked -- its labelling against scipy.ndimage.label, its metrics against the values recorded from the reference's
`compute_metrics` -- and so are the host parts of ldiffusion_amd.nnunet_post: the counts-to-metrics step, the summary files, the greedy rule on three
constructed scenarios with known answers, and the plumbing of the new keywords (nothing new goes downstream when they are not given)."""
import ctypes as C
import json
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nnunet_post_ref as ref  # noqa: E402

from ldiffusion_amd import _lib, nnunet_post as post  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TH, TW = _lib.CC_TILE_H, _lib.CC_TILE_W
KEEP = "remove_all_but_largest_component_from_segmentation"


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "reference_eval_metrics.json")) as f:
        cases = json.load(f)
    for c in cases:
        c["labels_or_regions"] = [tuple(r) if isinstance(r, list) else r for r in c["labels_or_regions"]]
        c["metrics"] = {post.key_to_label_or_region(k): v for k, v in c["metrics"].items()}
    return cases


# ---- the labelling --------------------------------------------------------------------------------------------------------------------------------------
def _masks():
    out = []
    for i, density in enumerate((0.1, 0.4, 0.7)):
        out.append((f"random {density}", np.random.RandomState(10 + i).rand(45, 70) < density))
    for shape in ((1, 1), (1, 2 * TW + 1), (2 * TH + 1, 1), (TH - 1, TW + 1), (2 * TH + 1, 3 * TW - 1)):
        out += [(f"{name} {shape}", m) for name, m in ref.hand_masks(*shape, TH, TW).items()]
    return out


def test_restated_labelling_equals_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    for name, mask in _masks():
        lab, sizes = ref.label8(mask)
        want, n = ndimage.label(mask, structure=np.ones((3, 3)))
        assert (lab > 0).tolist() == mask.tolist(), name
        roots = np.flatnonzero(sizes.ravel())
        assert roots.size == n, name
        for r in roots:                                           # up to renumbering: each of ours is exactly one of scipy's, named by its first pixel
            comp = lab == r + 1
            assert comp.ravel()[r] and np.flatnonzero(comp.ravel())[0] == r, name
            ids = np.unique(want[comp])
            assert ids.size == 1 and int((want == ids[0]).sum()) == int(comp.sum()) == int(sizes.ravel()[r]), name


def test_hand_cases_are_what_they_claim():
    m = ref.hand_masks(2 * TH + 1, 3 * TW - 1, TH, TW)
    sizes = {k: np.sort(ref.label8(v)[1].ravel()[ref.label8(v)[1].ravel() > 0])[::-1].tolist() for k, v in m.items() if k != "random 0.40"}
    assert sizes["empty"] == [] and sizes["full"] == [(2 * TH + 1) * (3 * TW - 1)] and sizes["single pixel"] == [1]
    assert len(sizes["checkerboard"]) == 1 and len(sizes["serpentine"]) == 1 and sizes["corner diagonal"] == [2]
    assert m["corner diagonal"][TH, TW] and m["corner diagonal"][TH - 1, TW - 1]
    assert sizes["two equal blobs"] == [12, 12, 4] and sizes["tie, smaller box first"] == [8, 8]
    kept = ref.keep_largest(m["two equal blobs"].astype(np.uint8), 1)
    assert kept[1:4, 1:5].all() and int(kept.sum()) == 12                      # the tie keeps the blob that comes first in raster order
    kept = ref.keep_largest(m["tie, smaller box first"].astype(np.uint8), 1)
    assert kept[0:2].sum() == 8 and int(kept.sum()) == 8                       # ... which here is the one with the smaller bounding box
    seg = np.zeros((4, 4), np.uint8)
    assert (ref.keep_largest(seg, [1, 2], 3) == seg).all()                     # an empty mask changes nothing


# ---- metrics --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", _golden(), ids=lambda c: c["name"])
def test_case_metrics_equal_the_reference_record(case):
    r, p = np.array(case["ref"], np.uint8), np.array(case["pred"], np.uint8)
    got = ref.case_metrics(r, p, case["labels_or_regions"], case["ignore_label"])
    assert ref.same_metrics(got, case["metrics"]), (got, case["metrics"])
    # the library's counts-to-metrics step on a confusion matrix counted with numpy through the library's own two tables
    index_of, pl, rl, n = post._luts(case["labels_or_regions"], case["ignore_label"])
    ri, pi = rl.numpy()[r].astype(np.int64), pl.numpy()[p].astype(np.int64)
    keep = ri < n
    conf = np.bincount(ri[keep] * n + pi[keep], minlength=n * n).reshape(n, n)
    got = post.metrics_from_confusion(conf, index_of, case["labels_or_regions"])
    assert ref.same_metrics(got, case["metrics"]), (got, case["metrics"])
    assert all(type(v) is (float if m in ("Dice", "IoU") else int) for d in got.values() for m, v in d.items())
    if case["name"] == "absent":
        assert np.isnan(got[3]["Dice"]) and np.isnan(got[3]["IoU"]) and got[3]["TN"] == r.size
    if case["name"] == "ignore":
        assert got[1]["TP"] + got[1]["FP"] + got[1]["FN"] + got[1]["TN"] == int((r != 3).sum())


def test_summarize_and_summary_json_round_trip(tmp_path):
    cases = [c for c in _golden() if c["name"] in ("regions",)]
    r, p = np.array(cases[0]["ref"], np.uint8), np.array(cases[0]["pred"], np.uint8)
    lors = cases[0]["labels_or_regions"]
    per_case = [{"metrics": ref.case_metrics(r, p, lors), "reference_file": "a", "prediction_file": "b"},
                {"metrics": ref.case_metrics(r.T.copy(), np.zeros_like(p), lors), "reference_file": "c", "prediction_file": "d"},
                {"metrics": ref.case_metrics(np.zeros_like(r), np.zeros_like(p), lors), "reference_file": "e", "prediction_file": "f"}]   # all nan
    summary = post.summarize(per_case)
    want = ref.summarize([c["metrics"] for c in per_case])
    assert ref.same_metrics(summary["mean"], want["mean"]) and ref.same_metrics({"fg": summary["foreground_mean"]}, {"fg": want["foreground_mean"]})
    d = [c["metrics"][(2, 3)]["Dice"] for c in per_case]
    assert np.isnan(d[2]) and summary["mean"][(2, 3)]["Dice"] == (d[0] + d[1]) / 2          # nanmean: the all-background case does not count
    path = str(tmp_path / "summary.json")
    post.save_summary_json(summary, path)
    text = open(path).read()
    assert '"(1, 2, 3)"' in text and '"(2, 3)"' in text and '"3"' in text and text.startswith('{\n    "foreground_mean"')   # sort_keys, indent 4
    back = post.load_summary_json(path)
    assert list(back["mean"]) and set(back["mean"]) == {(1, 2, 3), (2, 3), 3}
    assert ref.same_metrics({k: back["mean"][k] for k in summary["mean"]}, summary["mean"], ordered=False)
    for a, b in zip(back["metric_per_case"], summary["metric_per_case"]):
        assert ref.same_metrics({k: a["metrics"][k] for k in b["metrics"]}, b["metrics"], ordered=False) and a["reference_file"] == b["reference_file"]
    assert post.key_to_label_or_region("(6,)") == (6,) and post.key_to_label_or_region("4") == 4
    # a class absent from every case: its mean is nan, and so is the foreground mean (a plain mean over the classes)
    s = post.summarize([{"metrics": ref.case_metrics(r, p, [1, 9])}])
    assert np.isnan(s["mean"][9]["Dice"]) and np.isnan(s["foreground_mean"]["Dice"]) and s["mean"][9]["TN"] == r.size


# ---- the greedy rule ------------------------------------------------------------------------------------------------------------------------------------
def _greedy_with_the_library_rule(preds, refs, lors, fg):
    """post.greedy_decisions on numpy masks: the library's rule, the restatement's filter and metrics."""
    state = {"masks": list(preds), "trials": 0}
    baseline = ref.summary_of(preds, refs, lors)

    def trial(kw):
        state["trials"] += 1
        masks = [ref.keep_largest(m, **kw) for m in state["masks"]]
        return ref.summary_of(masks, refs, lors), lambda: state.update(masks=masks)

    fns, kwargs, final = post.greedy_decisions(baseline, lors, fg, trial)
    return fns, kwargs, final, state


def _scenario(name):
    truth = np.zeros((24, 24), np.uint8)
    if name == "a":      # the truth plus small islands of class 1
        truth[2:12, 2:12], truth[12:20, 2:12] = 1, 2
        pred = truth.copy()
        pred[22, 22], pred[1, 20:22] = 1, 1
        return [pred, truth.copy()], [truth, truth], [1, 2], [1, 2]
    if name == "b":      # class 2 has two true components, predicted exactly; the islands of class 1 tempt the whole-foreground step
        truth[2:12, 2:12], truth[12:16, 2:12], truth[20, 16:18] = 1, 2, 2     # the second component of class 2 is small: losing it costs less than the islands
        pred = truth.copy()
        pred[0, 15:23], pred[8, 20] = 1, 1
        return [pred], [truth], [1, 2], [1, 2]
    truth[4:14, 4:14] = 1   # c: one foreground class only
    pred = truth.copy()
    pred[20, 20:23] = 1
    return [pred], [truth], [1], [1]


def test_greedy_rule_on_constructed_scenarios():
    # (a) the foreground step is kept, and nothing after it: the classes are clean already
    preds, refs, lors, fg = _scenario("a")
    fns, kwargs, baseline, final, masks = ref.determine_postprocessing(preds, refs, lors, fg)
    assert (fns, kwargs) == ([KEEP], [{"labels_or_regions": [1, 2]}])
    assert all((m == t).all() for m, t in zip(masks, refs)) and final["foreground_mean"]["Dice"] == 1.0 > baseline["foreground_mean"]["Dice"]
    got = _greedy_with_the_library_rule(preds, refs, lors, fg)
    assert got[:2] == (fns, kwargs) and ref.same_metrics(got[2]["mean"], final["mean"]) and got[3]["trials"] == 3
    # (b) the foreground step would delete a true component of class 2: rejected because a class got worse; class 1 alone is kept, class 2 is not
    preds, refs, lors, fg = _scenario("b")
    whole = ref.summary_of([ref.keep_largest(preds[0], [1, 2])], refs, lors)
    base = ref.summary_of(preds, refs, lors)
    assert whole["foreground_mean"]["Dice"] > base["foreground_mean"]["Dice"] and whole["mean"][2]["Dice"] < base["mean"][2]["Dice"] == 1.0
    fns, kwargs, baseline, final, masks = ref.determine_postprocessing(preds, refs, lors, fg)
    assert (fns, kwargs) == ([KEEP], [{"labels_or_regions": 1}]) and (masks[0] == refs[0]).all()
    got = _greedy_with_the_library_rule(preds, refs, lors, fg)
    assert got[:2] == (fns, kwargs) and got[3]["trials"] == 3
    # (c) one entry: the per-class loop is skipped
    preds, refs, lors, fg = _scenario("c")
    fns, kwargs, baseline, final, masks = ref.determine_postprocessing(preds, refs, lors, fg)
    assert (fns, kwargs) == ([KEEP], [{"labels_or_regions": [1]}]) and (masks[0] == refs[0]).all()
    got = _greedy_with_the_library_rule(preds, refs, lors, fg)
    assert got[:2] == (fns, kwargs) and got[3]["trials"] == 1


def test_postprocessing_json_round_trip(tmp_path):
    preds, refs, lors, fg = _scenario("b")
    lors = [(1, 2), 2]
    base = ref.summary_of(preds, refs, lors)
    path = str(tmp_path / "postprocessing.json")
    post.save_postprocessing_json(path, [KEEP, KEEP], [{"labels_or_regions": [1, 2]}, {"labels_or_regions": (1, 2)}], base, base)
    record = json.load(open(path))
    assert sorted(record) == ["input_folder", "postprocessed", "postprocessing_fns", "postprocessing_kwargs"]
    assert sorted(record["input_folder"]) == ["foreground_mean", "mean"] and sorted(record["postprocessed"]["mean"]) == ["(1, 2)", "2"]
    fns, kwargs = post.load_postprocessing(path)
    assert fns == [KEEP, KEEP] and [ref.member_mask(preds[0], kw["labels_or_regions"]).tolist() for kw in kwargs] == [np.isin(preds[0], (1, 2)).tolist()] * 2
    with pytest.raises(FileNotFoundError, match="nowhere"):
        post.load_postprocessing(str(tmp_path / "nowhere" / "postprocessing.json"))
    with pytest.raises(ValueError, match="unknown postprocessing function"):
        post.apply_postprocessing(None, ["something_else"], [{}])


def test_label_lists_follow_the_label_manager():
    assert post.label_lists({"labels": {"background": 0, "a": 1, "b": 2, "c": 3}}) == ([1, 2, 3], [1, 2, 3], None)
    assert post.label_lists({"labels": {"background": 0, "a": 1, "b": 2, "ignore": 3}}) == ([1, 2], [1, 2], 3)
    got = post.label_lists({"labels": {"background": 0, "any": [1, 2, 3], "high": [2, 3], "top": [3], "ignore": 4}, "regions_class_order": [1, 2, 3]})
    assert got == ([(1, 2, 3), (2, 3), (3,)], [1, 2, 3], 4)
    t = post.membership_table([(1, 2), 5]).numpy()
    assert np.flatnonzero(t).tolist() == [1, 2, 5] and np.flatnonzero(post.membership_table((3, 4)).numpy()).tolist() == [3, 4]
    assert np.flatnonzero(post.membership_table(7).numpy()).tolist() == [7]


# ---- the interface --------------------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_and_bound():
    with open(os.path.join(ROOT, "include", "ldiff.h")) as f:
        header = f.read()
    kinds = {"int": C.c_int, "float": C.c_float, "int64_t": C.c_int64}
    for name in ("ldiff_op_keep_largest_component_ws_bytes", "ldiff_op_keep_largest_component", "ldiff_op_cc_label"):
        m = re.search(r"(\w+)\s+" + name + r"\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/ldiff.h"
        res, args = _lib.SIGNATURES[name]
        assert res is kinds[m.group(1)]
        want = [C.c_void_p if "*" in a else kinds[a.split()[-2]] for a in (a.strip() for a in m.group(2).split(","))]
        assert args == want, f"{name}: {args} against the header's {want}"
    assert int(re.search(r"#define LDIFF_CC_TILE_H (\d+)", header).group(1)) == TH and int(re.search(r"#define LDIFF_CC_TILE_W (\d+)", header).group(1)) == TW
    assert int(re.search(r"#define LDIFF_VERSION (\d+)", header).group(1)) >= 215


def test_parse_args_carries_the_new_flags():
    from ldiffusion_amd.ldiffusion import parse_args
    base = ["--diffusion-path", "sd", "--image-dir", "i", "--label-dir", "l", "--num-epochs", "12", "--batch-size", "2", "--num-inference-steps", "5", "--num-classes", "7"]
    a = parse_args(base)
    assert a.validate is False and a.postprocessing is False
    a = parse_args(base + ["--validate", "--postprocessing"])
    assert a.validate is True and a.postprocessing is True


def test_calls_without_the_new_keywords_pass_nothing_new_downstream(tmp_path, monkeypatch):
    from ldiffusion_amd.ldiffusion import LDiffusionModel
    from ldiffusion_amd.segmentor import Segmentor
    calls = []

    def init(self, train_loader, val_loader, level, num_classes):   # the real one asks for a GPU
        self.level, self.num_classes = level, num_classes

    def record(name):
        def fn(self, *a, **kw):
            calls.append((name, a, kw))
            return "out"
        return fn

    monkeypatch.setattr(Segmentor, "__init__", init)
    monkeypatch.setattr(Segmentor, "train_tissue_model_nnUNetv2", record("train"))
    monkeypatch.setattr(Segmentor, "inference_tissue_model_nnUNetv2", record("infer"))
    model = LDiffusionModel.__new__(LDiffusionModel)
    model.level, model.rank, model.diffusion_path = "tissue", 0, "sd"
    args = SimpleNamespace(num_epochs=12, diffusion_path="sd", num_classes=7)
    tr = SimpleNamespace(dataset=SimpleNamespace(image_dir=["a.png"], label_dir=["a_l.png"]))
    va = SimpleNamespace(dataset=SimpleNamespace(image_dir=["b.png"], label_dir=["b_l.png"]))
    lists = dict(train_images=["a.png"], train_labels=["a_l.png"], test_images=["b.png"], test_labels=["b_l.png"])
    assert model.train(args, component="segmentor", ldiffusion_weight="w", train_loader=tr, val_loader=va) == "out"
    assert calls[-1] == ("train", (2, "w", "sd"), lists)
    args_off = SimpleNamespace(num_epochs=12, diffusion_path="sd", num_classes=7, validate=False, postprocessing=False)
    model.train(args_off, component="segmentor", ldiffusion_weight="w", train_loader=tr, val_loader=va)
    assert calls[-1] == ("train", (2, "w", "sd"), lists)
    model.train(args, component="segmentor", ldiffusion_weight="w", train_loader=tr, val_loader=va, validate=True)
    assert calls[-1] == ("train", (2, "w", "sd"), dict(lists, validate=True))
    args_on = SimpleNamespace(num_epochs=12, diffusion_path="sd", num_classes=7, validate=False, postprocessing=True)
    model.train(args_on, component="segmentor", ldiffusion_weight="w", train_loader=tr, val_loader=va, validation_checkpoint="checkpoint_best.pth")
    assert calls[-1] == ("train", (2, "w", "sd"), dict(lists, postprocessing=True, validation_checkpoint="checkpoint_best.pth"))
    model.inference("img.png", "w", "folder", 7)
    assert calls[-1] == ("infer", ("img.png", "sd", "w", "folder"), dict(output_path=None, predictor=None, text_embeddings=None, batch_tiles=None))
    model.inference("img.png", "w", "folder", 7, postprocess=True)
    assert calls[-1][2]["postprocess"] is True and len(calls[-1][2]) == 5
