"""No GPU: the fold ensemble's host side -- the twin of ldiff_op_window_finish_ensemble's arithmetic (tests/fold_ensemble_ref.py) against the reference's own
recorded ensemble (tests/golden/reference_fold_ensemble.npz), fold detection, `load_fold_ensemble`'s refusals, `accumulate_cv_results`, and the keywords
`folds` / `use_folds` from the command line down to the Segmentor."""
import ctypes as C
import json
import os
import re
import shutil
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fold_ensemble_ref as twin  # noqa: E402
import nnunet_post_ref as ref  # noqa: E402
import nnunet_ref  # noqa: E402

from ldiffusion_amd import _lib, nnunet, nnunet_post as post, tiling  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def fixtures():
    with open(os.path.join(GOLDEN, "nnunet_plans_2d.json")) as f:
        plans = json.load(f)
    with open(os.path.join(GOLDEN, "nnunet_dataset.json")) as f:
        ds = json.load(f)
    return plans, ds


# ---- the arithmetic -------------------------------------------------------------------------------------------------------------------------------------
def test_twin_reproduces_the_reference_ensemble_from_the_per_fold_logits():
    """Each fold's logits by the per-tile path on the host (pinned to the reference's predictor by tests/test_cpu_oracle.py), then the twin without a count
    plane: the reference's `prediction += ...; prediction /= 3` bit for bit, on all three cases."""
    z = np.load(os.path.join(GOLDEN, "reference_fold_ensemble.npz"))
    nets = [twin.stand_in_network(w, s) for w, s in zip(z["fold_weights"], z["fold_slopes"])]
    assert len(nets) == 3
    for tag in "abc":
        th, tw, step, mm = z[tag + "_cfg"]
        mirror = None if mm < 0 else tuple(i for i in range(2) if (int(mm) >> i) & 1)
        image = torch.from_numpy(z[tag + "_image"])
        folds = [tiling.predict_sliding_window_return_logits(image, net, 4, (int(th), int(tw)), float(step), True, mirror) for net in nets]
        want = torch.from_numpy(z[tag + "_logits_f16"])
        got, mask, flag = twin.ensemble(folds)
        assert got.dtype == torch.float16 and flag == 0 and torch.equal(got, want), tag
        assert all(not torch.equal(f, want) for f in folds), tag                      # the ensemble is no single fold
        assert mask.dtype == torch.uint8 and tuple(mask.shape) == tuple(want.shape[1:])
        exact = (folds[0].double() + folds[1].double() + folds[2].double()) / 3
        assert int((exact.half().double() != exact).sum()) > 0, tag                  # the last division rounds somewhere


def test_twin_orders_and_flags():
    """A check of the ORACLE itself, not of the library (it passes with or without the feature): the properties the GPU tests rely on the twin to have.
    One fold with a count plane is `acc / cnt`; the flag looks at the folds' logits, not at the sum; the sum runs in fold order."""
    acc = torch.tensor([[[3.0, 40000.0]]], dtype=torch.float16)
    cnt = torch.tensor([[2.0, 1.0]], dtype=torch.float16)
    got, _, flag = twin.ensemble([acc], cnt)
    assert torch.equal(got, acc / cnt) and flag == 0
    got, mask, flag = twin.ensemble([acc, acc], cnt)
    assert flag == 0 and bool(torch.isinf(got[0, 0, 1])) and float(got[0, 0, 0]) == 1.5 and int(mask[0, 1]) == 0   # 40000 + 40000 overflows unflagged
    got, _, flag = twin.ensemble([acc, torch.full_like(acc, float("-inf"))], cnt)
    assert flag == 1
    a, b, c = (torch.tensor([[[v]]], dtype=torch.float16) for v in (2048.0, 1.0, 1.0))
    assert float(twin.ensemble([a, b, c])[0]) * 3 != float(twin.ensemble([b, c, a])[0]) * 3                        # (2048 + 1) + 1 against (1 + 1) + 2048 in float16


def test_entry_point_is_declared_and_bound():
    with open(os.path.join(ROOT, "include", "ldiff.h")) as f:
        header = f.read()
    m = re.search(r"int\s+ldiff_op_window_finish_ensemble\(([^)]*)\)\s*;", header)
    assert m, "ldiff_op_window_finish_ensemble is not declared in include/ldiff.h"
    res, args = _lib.SIGNATURES["ldiff_op_window_finish_ensemble"]
    n_pointers = sum("*" in a for a in m.group(1).split(","))
    assert res is C.c_int and len(args) == len(m.group(1).split(",")) == 19 and n_pointers == 6
    assert int(re.search(r"#define LDIFF_ENSEMBLE_MAX_FOLDS (\d+)", header).group(1)) == tiling.ENSEMBLE_MAX_FOLDS == 8


# ---- folders --------------------------------------------------------------------------------------------------------------------------------------------
def _model_folder(tmp_path, folds=(0, 2), configurations=None, seeds=None):
    plans, ds = fixtures()
    spec = nnunet.network_spec(plans, "2d_reduced", ds)
    path = str(tmp_path / "model")
    nnunet_ref.write_model_folder(path, plans, ds, nnunet_ref.synthetic_state_dict(spec, 1), spec, "2d_reduced")
    for i, f in enumerate(folds):
        os.makedirs(os.path.join(path, f"fold_{f}"), exist_ok=True)
        torch.save({"network_weights": nnunet_ref.checkpoint_like(nnunet_ref.synthetic_state_dict(spec, (seeds or folds)[i] + 1), spec),
                    "init_args": {"configuration": (configurations or ["2d_reduced"] * len(folds))[i], "fold": f}, "trainer_name": "nnUNetTrainer",
                    "inference_allowed_mirroring_axes": (0, 1) if i == 0 else (1,)}, os.path.join(path, f"fold_{f}", "checkpoint_best.pth"))
    if 0 not in folds:
        shutil.rmtree(os.path.join(path, "fold_0"))
    return path, spec


def test_available_folds(tmp_path):
    path, _ = _model_folder(tmp_path, (0, 2))
    os.makedirs(os.path.join(path, "fold_3"))                                          # no checkpoint inside
    os.makedirs(os.path.join(path, "fold_all"))
    shutil.copy(os.path.join(path, "fold_0", "checkpoint_best.pth"), os.path.join(path, "fold_all", "checkpoint_best.pth"))
    os.makedirs(os.path.join(path, "fold_10"))
    shutil.copy(os.path.join(path, "fold_0", "checkpoint_best.pth"), os.path.join(path, "fold_10", "checkpoint_best.pth"))
    assert nnunet.available_folds(path, "checkpoint_best.pth") == [0, 2, 10]           # sorted as numbers, never fold_all
    assert nnunet.available_folds(path, "checkpoint_final.pth") == []


def test_read_fold_ensemble_takes_the_first_folds_settings(tmp_path):
    path, spec = _model_folder(tmp_path, (0, 2))
    folds, got_spec, sds, axes = nnunet.read_fold_ensemble(path)
    assert folds == (0, 2) and len(sds) == 2 and tuple(axes) == (0, 1) and got_spec["features"] == spec["features"]
    assert not torch.equal(sds[0]["encoder.stages.0.0.convs.0.conv.weight"], sds[1]["encoder.stages.0.0.convs.0.conv.weight"])
    folds, _, sds, axes = nnunet.read_fold_ensemble(path, (2, 0))                      # the given order; the first fold's mirror axes
    assert folds == (2, 0) and tuple(axes) == (1,)
    assert nnunet.read_fold_ensemble(path, [2])[0] == (2,)                             # one fold is allowed


def test_load_fold_ensemble_refuses_before_any_device_use(tmp_path, monkeypatch):
    from ldiffusion_amd import models

    def no_device(*a, **k):
        raise AssertionError("a network was built before the folds were checked")
    monkeypatch.setattr(models, "PlainConvUNet", no_device)
    path, spec = _model_folder(tmp_path, (0, 1, 2), configurations=["2d_reduced", "2d", "2d_reduced"])
    with pytest.raises(ValueError, match=r"fold 1: the checkpoint names the configuration '2d'"):
        nnunet.load_fold_ensemble(path, (0, 1, 2))
    ckpt = torch.load(os.path.join(path, "fold_2", "checkpoint_best.pth"), weights_only=False)
    del ckpt["network_weights"]["decoder.transpconvs.0.bias"]
    torch.save(ckpt, os.path.join(path, "fold_2", "checkpoint_best.pth"))
    with pytest.raises(RuntimeError, match=r"fold 2: 1 nnU-Net tensors missing"):
        nnunet.load_fold_ensemble(path, (0, 2))
    with pytest.raises(FileNotFoundError, match="fold 4"):
        nnunet.load_fold_ensemble(path, (0, 4))
    for bad, word in (((0, 0), "twice"), ("all", "all"), ((0, "all"), "all"), ((), "no fold"), ((0, 1.5), "no fold number"), (tuple(range(9)), "at most 8")):
        with pytest.raises(ValueError, match=word):
            nnunet.load_fold_ensemble(path, bad)
    with pytest.raises(ValueError, match="no fold_<n>/checkpoint_final.pth"):
        nnunet.load_fold_ensemble(path, None, "checkpoint_final.pth")
    with pytest.raises(ValueError, match="`use_folds`"):                               # the single-fold readers stay what they were
        nnunet.read_trained_model_folder(path, fold=(0, 1))


# ---- accumulate_cv_results --------------------------------------------------------------------------------------------------------------------------------
def _png(path):
    from PIL import Image
    return np.array(Image.open(path).convert("L"), np.uint8)


def _cv_folder(tmp_path):
    from PIL import Image
    rng = np.random.RandomState(4)
    model, gt = tmp_path / "model", tmp_path / "labelsTr"
    gt.mkdir(parents=True)
    (model).mkdir()
    (model / "dataset.json").write_text(json.dumps({"labels": {"background": 0, "a": 1, "b": 2, "c": 3}, "file_ending": ".png"}))
    (model / "plans.json").write_text(json.dumps({"dataset_name": "Dataset001_Custom"}))
    cases = {0: ["c0", "c1"], 1: ["c2"], 3: ["c3"]}
    for f, keys in cases.items():
        val = model / f"fold_{f}" / "validation"
        val.mkdir(parents=True)
        (val / "summary.json").write_text("{}")                                       # no fold's own summary is copied or read
        for k in keys:
            Image.fromarray(rng.randint(0, 4, (9, 11)).astype(np.uint8)).save(val / (k + ".png"))
            Image.fromarray(rng.randint(0, 4, (9, 11)).astype(np.uint8)).save(gt / (k + ".png"))
    return str(model), str(gt), cases


def test_accumulate_cv_results(tmp_path, monkeypatch):
    model, gt, cases = _cv_folder(tmp_path)
    host_metrics = lambda r, p, lors, ignore=None: ref.case_metrics(r.numpy(), p.numpy(), lors, ignore)   # noqa: E731  the device entry's restatement
    monkeypatch.setattr(post, "case_metrics", host_metrics)
    summary = post.accumulate_cv_results(model, (0, 1, 3), gt, device="cpu")
    merged = os.path.join(model, "crossval_results_folds_0_1_3")
    assert post.crossval_folder(model, (0, 1, 3)) == merged
    assert sorted(os.listdir(merged)) == ["c0.png", "c1.png", "c2.png", "c3.png", "dataset.json", "plans.json", "summary.json"]
    for f, keys in cases.items():
        for k in keys:
            assert np.array_equal(_png(os.path.join(merged, k + ".png")), _png(os.path.join(model, f"fold_{f}", "validation", k + ".png")))
    names = ["c0", "c1", "c2", "c3"]
    want = ref.summarize([ref.case_metrics(_png(os.path.join(gt, k + ".png")), _png(os.path.join(merged, k + ".png")), [1, 2, 3]) for k in names])
    written = post.load_summary_json(os.path.join(merged, "summary.json"))
    for got in (summary, written):
        assert ref.same_metrics(got["mean"], want["mean"], ordered=False)
        assert ref.same_metrics({"fg": got["foreground_mean"]}, {"fg": want["foreground_mean"]}, ordered=False)
        assert [os.path.basename(c["prediction_file"]) for c in got["metric_per_case"]] == [k + ".png" for k in names]
    assert written["metric_per_case"][2]["reference_file"] == os.path.join(gt, "c2.png")
    # the folder is made anew: a stale file does not survive, and the given order names the folder
    open(os.path.join(merged, "stale.png"), "wb").close()
    post.accumulate_cv_results(model, (0, 1, 3), gt, device="cpu")
    assert "stale.png" not in os.listdir(merged)
    post.accumulate_cv_results(model, (3, 0), gt, device="cpu")
    assert sorted(n for n in os.listdir(os.path.join(model, "crossval_results_folds_3_0")) if n.endswith(".png")) == ["c0.png", "c1.png", "c3.png"]
    # the reference's two errors
    with pytest.raises(RuntimeError, match="fold 2 of model .* is missing. Please train it!"):
        post.accumulate_cv_results(model, (0, 2), gt, device="cpu")
    shutil.copy(os.path.join(model, "fold_0", "validation", "c1.png"), os.path.join(model, "fold_1", "validation", "c1.png"))
    with pytest.raises(RuntimeError, match="More than one of your folds has a prediction for case c1.png"):
        post.accumulate_cv_results(model, (0, 1), gt, device="cpu")


def test_accumulate_sub_command(tmp_path, monkeypatch):
    calls = []
    monkeypatch.setattr(post, "accumulate_cv_results", lambda *a, **k: calls.append((a, k)) or "summary")
    assert post.main(["accumulate", "-m", "model", "-f", "0", "2", "-ref", "gt", "--device", "cpu", "-np", "0"]) == "summary"
    assert calls == [(("model", (0, 2), "gt"), dict(device="cpu", io_workers=0))]
    post.main(["accumulate", "-m", "model", "-ref", "gt"])
    assert calls[-1][0][1] == (0, 1, 2, 3, 4)


def test_validate_fold_takes_a_fold(monkeypatch):
    import inspect
    p = inspect.signature(post.validate_fold).parameters["fold"]
    assert p.default == 0 and p.kind is inspect.Parameter.KEYWORD_ONLY


def test_fold_zero_starts_from_the_weights_of_before():
    """`folds=None` calls `initial_state_dict(spec)`, `folds=(0, ...)` calls `initial_state_dict(spec, seed=0)`: the same tensors bit for bit, and fold 1's differ."""
    from ldiffusion_amd import nnunet_train
    plans, ds = fixtures()
    spec = nnunet.network_spec(plans, "2d_reduced", ds)
    default, zero, one = nnunet_train.initial_state_dict(spec), nnunet_train.initial_state_dict(spec, seed=0), nnunet_train.initial_state_dict(spec, seed=1)
    assert list(default) == list(zero) == list(one) and all(torch.equal(default[k], zero[k]) for k in default)
    assert any(not torch.equal(zero[k], one[k]) for k in zero)


# ---- the keywords ---------------------------------------------------------------------------------------------------------------------------------------
def test_parse_args_carries_folds():
    from ldiffusion_amd.ldiffusion import parse_args
    base = ["--diffusion-path", "sd", "--image-dir", "i", "--label-dir", "l", "--num-epochs", "12", "--batch-size", "2", "--num-inference-steps", "5", "--num-classes", "7"]
    assert parse_args(base).folds is None
    assert parse_args(base + ["--folds", "0", "1", "2", "3", "4"]).folds == [0, 1, 2, 3, 4]
    assert parse_args(base + ["--folds", "3", "--validate"]).folds == [3]


def test_calls_without_the_new_keywords_pass_nothing_new_downstream(monkeypatch):
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
    model.train(args, component="segmentor", ldiffusion_weight="w", train_loader=tr, val_loader=va)
    assert calls[-1] == ("train", (2, "w", "sd"), lists)
    model.train(SimpleNamespace(num_epochs=12, diffusion_path="sd", num_classes=7, folds=None), component="segmentor", ldiffusion_weight="w", train_loader=tr, val_loader=va)
    assert calls[-1] == ("train", (2, "w", "sd"), lists)
    model.train(args, component="segmentor", ldiffusion_weight="w", train_loader=tr, val_loader=va, folds=[0, 3])
    assert calls[-1] == ("train", (2, "w", "sd"), dict(lists, folds=(0, 3)))
    model.train(SimpleNamespace(num_epochs=12, diffusion_path="sd", num_classes=7, folds=[1, 2], validate=True), component="segmentor", ldiffusion_weight="w",
                train_loader=tr, val_loader=va)
    assert calls[-1] == ("train", (2, "w", "sd"), dict(lists, folds=(1, 2), validate=True))
    model.inference("img.png", "w", "folder", 7)
    assert calls[-1] == ("infer", ("img.png", "sd", "w", "folder"), dict(output_path=None, predictor=None, text_embeddings=None, batch_tiles=None))
    model.inference("img.png", "w", "folder", 7, use_folds=[0, 1])
    assert calls[-1] == ("infer", ("img.png", "sd", "w", "folder"), dict(output_path=None, predictor=None, text_embeddings=None, batch_tiles=None, use_folds=(0, 1)))


def test_segmentor_refuses_fold_all_and_folds_beyond_the_split(monkeypatch):
    from ldiffusion_amd.segmentor import Segmentor
    seg = Segmentor.__new__(Segmentor)
    for name in ("nnUNet_raw", "nnUNet_preprocessed", "nnUNet_results"):
        monkeypatch.setenv(name, "/nonexistent")
    monkeypatch.setattr(Segmentor, "load_ldiffusion", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the stage began")))
    for bad, word in (("all", "all"), ((0, "all"), "all"), ((0, 5), "beyond"), ((1, 1), "twice"), ((), "no fold")):
        with pytest.raises(ValueError, match=word):
            seg.train_tissue_model_nnUNetv2(1, "w", "sd", ["a"], ["b"], ["a"], ["b"], folds=bad)
    with pytest.raises(ValueError, match="injected `predictor`"):
        seg.inference_tissue_model_nnUNetv2("img.png", "sd", "w", None, predictor=lambda x: x, use_folds=(0, 1))


def test_tissue_head_cache_key_and_postprocessing_record(tmp_path, monkeypatch):
    """`_tissue_head`: without `use_folds` the single-fold loader as before; with it `load_fold_ensemble`, keyed by the folds and every checkpoint's mtime.
    postprocess=True reads the crossval folder's record only for more than one fold."""
    from ldiffusion_amd.segmentor import Segmentor
    path, _ = _model_folder(tmp_path, (0, 2))
    loads = []
    monkeypatch.setattr(nnunet, "load_trained_model_folder", lambda *a, **k: loads.append(("single", a)) or "single-head")
    monkeypatch.setattr(nnunet, "load_fold_ensemble", lambda *a, **k: loads.append(("ensemble", a)) or f"ensemble-{len(loads)}")
    seg = Segmentor.__new__(Segmentor)
    seg.device = "cpu"
    assert seg._tissue_head(path) == "single-head" and loads[-1] == ("single", (path, 0, "checkpoint_best.pth"))
    first = seg._tissue_head(path, (0, 2))
    assert loads[-1] == ("ensemble", (path, (0, 2), "checkpoint_best.pth")) and seg._tissue_head(path, [0, 2]) == first and len(loads) == 2
    ckpt = os.path.join(path, "fold_2", "checkpoint_best.pth")
    os.utime(ckpt, (os.path.getmtime(ckpt) + 5, os.path.getmtime(ckpt) + 5))          # the SECOND fold's checkpoint changed
    assert seg._tissue_head(path, (0, 2)) != first and len(loads) == 3
    assert seg._tissue_head(path, (2, 0)) != first and loads[-1][1][1] == (2, 0)
    for folds, where in (((0, 2), "crossval_results_folds_0_2/postprocessing.json"), ((2,), "fold_2/validation/postprocessing.json"),
                         (None, "fold_0/validation/postprocessing.json")):
        with pytest.raises(FileNotFoundError, match=where):
            seg.inference_tissue_model_nnUNetv2("img.png", "sd", "w", path, postprocess=True, **({} if folds is None else {"use_folds": folds}))
