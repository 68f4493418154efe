"""-m gpu: the fold ensemble of the tissue head -- ldiff_op_window_finish_ensemble through ldiffusion_amd.tiling, nnunet.FoldEnsemble, and the tissue stage
with `folds=` / `use_folds=`.  Every comparison of logits and masks is bit for bit: against the host twin (tests/fold_ensemble_ref.py, pinned to the
reference's recorded ensemble by tests/test_cpu_fold_ensemble.py), against ldiff_op_window_finish, and against the reference's recorded ensemble itself
(tests/golden/reference_fold_ensemble.npz)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fold_ensemble_ref as twin  # noqa: E402
import nnunet_post_ref as ref  # noqa: E402
import nnunet_ref  # noqa: E402

from ldiffusion_amd import _lib, nnunet, nnunet_post as post, tiling  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HP, WP = 24, 64


def _same(a, b):
    """torch.equal with NaN equal to NaN."""
    return torch.equal(torch.nan_to_num(a.float(), nan=12345.0), torch.nan_to_num(b.float(), nan=12345.0))


def _finish(accs, cnt, box, mask_hw=(40, 72), mask_origin=(5, 6)):
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    logits = torch.empty((accs[0].shape[0], box[2], box[3]), dtype=accs[0].dtype, device=DEV)
    mask = torch.zeros(mask_hw, dtype=torch.uint8, device=DEV)
    tiling.window_finish_ensemble(accs, cnt, box, flag, logits=logits, mask=mask, mask_origin=mask_origin)
    return logits.cpu(), mask.cpu(), int(flag.item())


# ---- 1. the kernel against the twin -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("heads", [1, 4, 7])
def test_kernel_equals_the_twin_bit_for_bit(heads, dtype):
    """Extent 24 x 64, K = 1, 2, 3, 5 folds, with and without the count plane; boxes 44 wide at x0 = 4 with the mask at a multiple of 4 (whole vectors) and
    every other combination of width 44 / 45, x0 4 / 5 and mask column 8 / 6 (the element path).  float16-valued accumulators over counts 1 .. 40: the
    quotients, the sums and the last division all round."""
    g = torch.Generator().manual_seed(heads * 10 + (dtype == torch.float16))
    accs = [(torch.randn((heads, HP, WP), generator=g) * 20).half().to(dtype) for _ in range(5)]
    cnt = torch.randint(1, 41, (HP, WP), generator=g).to(dtype)
    dacc, dcnt = [a.to(DEV) for a in accs], cnt.to(DEV)
    rounded = 0
    for K in (1, 2, 3, 5):
        for with_cnt in (True, False):
            for w, x0, mx0 in ((44, 4, 8), (44, 4, 6), (45, 4, 8), (44, 5, 8), (45, 5, 6)):
                box = (3, x0, 20, w)
                want_l, want_m, want_f = twin.ensemble(accs[:K], cnt if with_cnt else None, box)
                got_l, got_m, got_f = _finish(dacc[:K], dcnt if with_cnt else None, box, mask_origin=(5, mx0))
                where = (K, with_cnt, w, x0, mx0)
                assert got_f == want_f == 0 and torch.equal(got_l, want_l), where
                assert torch.equal(got_m[5:25, mx0:mx0 + w], want_m) and int(got_m.sum()) == int(want_m.sum()), where      # nothing outside the mask box
                if K > 1 and dtype == torch.float16:
                    exact = sum(a[:, 3:23, x0:x0 + w].double() / (cnt[3:23, x0:x0 + w].double() if with_cnt else 1.0) for a in accs[:K]) / K
                    rounded += int((want_l.double() != exact).sum())
            only_mask = torch.zeros((40, 72), dtype=torch.uint8, device=DEV)                                                # either output may be left out
            tiling.window_finish_ensemble(dacc[:K], dcnt if with_cnt else None, (3, 4, 20, 44), torch.zeros(1, dtype=torch.int32, device=DEV), mask=only_mask,
                                          mask_origin=(5, 8))
            assert torch.equal(only_mask.cpu()[5:25, 8:52], twin.ensemble(accs[:K], cnt if with_cnt else None, (3, 4, 20, 44))[1])
    assert heads == 1 or int(want_m.max()) > 0
    assert dtype == torch.float32 or rounded > 0


# ---- 2. one fold is window_finish -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_one_fold_with_counts_is_window_finish(dtype):
    g = torch.Generator().manual_seed(21)
    acc = (torch.randn((5, HP, WP), generator=g) * 20).to(dtype)
    acc[2, 10, 9], acc[1, 11, 30] = float("inf"), float("nan")
    cnt = (torch.rand((HP, WP), generator=g) * 30 + 0.5).to(dtype)
    for with_inf in (False, True):
        a = acc.clone()
        if not with_inf:
            a[2, 10, 9] = 1.0
        a, c = a.to(DEV), cnt.to(DEV)
        for box, origin in (((3, 4, 20, 44), (4, 8)), ((2, 5, 21, 45), (5, 6))):
            flag = torch.zeros(1, dtype=torch.int32, device=DEV)
            logits = torch.empty((5, box[2], box[3]), dtype=dtype, device=DEV)
            mask = torch.zeros((40, 72), dtype=torch.uint8, device=DEV)
            tiling.window_finish(a, c, box, flag, logits=logits, mask=mask, mask_origin=origin)
            got_l, got_m, got_f = _finish([a], c, box, mask_origin=origin)
            assert got_f == int(flag.item()) == int(with_inf) and _same(got_l, logits.cpu()) and torch.equal(got_m, mask.cpu()), (with_inf, box)


# ---- 3. special values ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_special_values(dtype):
    g = torch.Generator().manual_seed(31)
    folds = [(torch.randn((4, HP, WP), generator=g) * 5).to(dtype) for _ in range(3)]
    box = (0, 0, HP, WP)

    def run(value, head=2, fold=1):
        f = [t.clone() for t in folds]
        f[fold][head, 7, 9] = value
        want = twin.ensemble(f, None, box)
        got = _finish([t.to(DEV) for t in f], None, box, mask_hw=(HP, WP), mask_origin=(0, 0))
        assert _same(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2] == want[2], value
        return got

    logits, mask, flag = run(float("nan"))
    assert flag == 0 and bool(torch.isnan(logits[2, 7, 9])) and int(mask[7, 9]) == 0                  # a NaN is not inf; the pixel is class 0
    logits, mask, flag = run(float("inf"), head=3)
    assert flag == 1 and float(logits[3, 7, 9]) == float("inf") and int(mask[7, 9]) == 0                # +inf: flagged, class 0 by the arg-max rule
    logits, mask, flag = run(float("-inf"), head=3)
    assert flag == 1 and float(logits[3, 7, 9]) == float("-inf") and int(mask[7, 9]) == int(logits[:3, 7, 9].float().argmax())
    for k in range(3):                                                                                  # the flag looks at every fold
        assert run(float("inf"), fold=k)[2] == 1
    if dtype == torch.float16:                                                                          # the sum overflows, no fold does: not flagged, class 0
        big = [torch.zeros((4, HP, WP), dtype=dtype) for _ in range(2)]
        for t in big:
            t[1, 3, 5] = 40000.0
        logits, mask, flag = _finish([t.to(DEV) for t in big], None, box, mask_hw=(HP, WP), mask_origin=(0, 0))
        assert flag == 0 and float(logits[1, 3, 5]) == float("inf") and int(mask[3, 5]) == 0 and int(mask.sum()) == 0
        ones = torch.ones((HP, WP), dtype=dtype)
        logits, mask, flag = _finish([t.to(DEV) for t in big], ones.to(DEV), box, mask_hw=(HP, WP), mask_origin=(0, 0))
        assert flag == 0 and float(logits[1, 3, 5]) == float("inf")


# ---- 4. the reference's recorded ensemble ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1, 2, "all"])
def test_ensemble_window_reproduces_the_reference_fixture_bit_for_bit(chunk):
    """Cases a, b, c of the reference's predict_logits_from_preprocessed_data over three parameter sets.  The stand-in heads run on the CPU inside the wrappers,
    so only the window kernels do arithmetic on the device."""
    z = np.load(os.path.join(GOLDEN, "reference_fold_ensemble.npz"))
    cpu_nets = [twin.stand_in_network(w, s) for w, s in zip(z["fold_weights"], z["fold_slopes"])]
    nets = [lambda x, n=n: n(x.cpu()).to(DEV) for n in cpu_nets]
    for tag in "abc":
        th, tw, step, mm = z[tag + "_cfg"]
        mirror = None if mm < 0 else tuple(i for i in range(2) if (int(mm) >> i) & 1)
        image = torch.from_numpy(z[tag + "_image"]).to(DEV)
        b = len(tiling.tile_origins(tuple(image.shape[1:]), (int(th), int(tw)), float(step))) if chunk == "all" else chunk
        got = tiling.predict_sliding_window_ensemble(image, nets, 4, (int(th), int(tw)), float(step), True, mirror, batch_tiles=b)
        want = torch.from_numpy(z[tag + "_logits_f16"])
        print(f"ensemble window {tag}, batch_tiles {b}: {int((got.cpu() != want).sum())} of {want.numel()} elements differ from the reference fixture")
        assert got.is_cuda and got.dtype == torch.float16 and torch.equal(got.cpu(), want), tag
        mask = tiling.predict_sliding_window_ensemble(image, nets, 4, (int(th), int(tw)), float(step), True, mirror, batch_tiles=b, return_mask=True)
        assert torch.equal(mask.cpu(), twin.ensemble([want])[1]) and int(mask.max()) > 0
        one = tiling.predict_sliding_window_ensemble(image, nets[:1], 4, (int(th), int(tw)), float(step), True, mirror, batch_tiles=b)      # one network: the batched path
        assert torch.equal(one, tiling.predict_sliding_window_batched(image, nets[0], 4, (int(th), int(tw)), float(step), True, mirror, batch_tiles=b))
    with pytest.raises(RuntimeError, match="Encountered inf in predicted array"):                       # one fold's inf raises, as the reference's per-fold look does
        tiling.predict_sliding_window_ensemble(torch.full((3, 32, 32), 6e4, device=DEV), [lambda x: x[:, :1] * 0.0, lambda x: x[:, :1] * 10.0], 1, (32, 32), 1.0, True, None)


# ---- 5. the library's head ----------------------------------------------------------------------------------------------------------------------------------
def fixtures():
    with open(os.path.join(GOLDEN, "nnunet_plans_2d.json")) as f:
        plans = json.load(f)
    with open(os.path.join(GOLDEN, "nnunet_dataset.json")) as f:
        ds = json.load(f)
    return plans, ds


def _write_folds(path, plans, ds, spec, seeds, mirror_axes=(0, 1)):
    sds = [nnunet_ref.synthetic_state_dict(spec, s) for s in seeds]
    nnunet_ref.write_model_folder(path, plans, ds, sds[0], spec, "2d_reduced", mirror_axes=mirror_axes)
    for f, sd in enumerate(sds):
        os.makedirs(os.path.join(path, f"fold_{f}"), exist_ok=True)
        torch.save({"network_weights": nnunet_ref.checkpoint_like(sd, spec), "init_args": {"configuration": "2d_reduced", "fold": f}, "trainer_name": "nnUNetTrainer",
                    "inference_allowed_mirroring_axes": mirror_axes}, os.path.join(path, f"fold_{f}", "checkpoint_best.pth"))
    return path


def _image():
    g = torch.Generator().manual_seed(77)
    smooth = torch.nn.functional.avg_pool2d(torch.rand((1, 3, 104, 168), generator=g), 9, 1)          # [1, 3, 96, 160]
    image = (smooth[0] * 254 + 1).to(DEV)
    bordered = torch.zeros((3, 120, 200), device=DEV)
    bordered[:, 10:106, 30:190] = image
    return image, bordered


def test_fold_ensemble_of_the_library_head(tmp_path):
    """Three synthetic 2d_reduced folds, image 96 x 160, tile 64 x 64, step 0.5, mirrors (0, 1).  The ensemble's mask is the twin's on the three folds' own
    logits, batched (batch_tiles = 2) and per tile -- the two paths are not compared with each other: their single-fold logits differ by an ulp (the per-tile
    path's device division).  A one-fold ensemble is `TrainedModel.predict_mask`; a zero border goes through the un-crop."""
    plans, ds = fixtures()
    spec = nnunet.network_spec(plans, "2d_reduced", ds)
    folder = _write_folds(str(tmp_path / "model"), plans, ds, spec, (31, 32, 33))
    image, bordered = _image()
    ens = nnunet.load_fold_ensemble(folder, device=DEV)                                               # folds detected
    assert ens.folds == (0, 1, 2) and len(ens.models) == 3 and ens.num_heads == spec["n_heads"] and ens.patch_size == tuple(spec["patch_size"]) and ens.mirror_axes == (0, 1)
    x, box = nnunet.preprocess(image, ens.normalization_schemes)
    assert box == (0, 96, 0, 160)
    nets = [m.network for m in ens.models]
    batched = [tiling.predict_sliding_window_batched(x, n, ens.num_heads, (64, 64), 0.5, True, (0, 1), batch_tiles=2).cpu() for n in nets]
    per_tile = [tiling.predict_sliding_window_return_logits(x, n, ens.num_heads, (64, 64), 0.5, True, (0, 1)).cpu() for n in nets]
    want_b, want_t = twin.ensemble(batched)[1], twin.ensemble(per_tile)[1]
    got_b = ens.predict_mask(image, (64, 64), 0.5, (0, 1), batch_tiles=2)
    got_t = ens.predict_mask(image, (64, 64), 0.5, (0, 1))
    assert got_b.dtype == torch.uint8 and got_b.shape == (96, 160) and torch.equal(got_b.cpu(), want_b) and int(want_b.max()) > 0
    assert torch.equal(got_t.cpu(), want_t)
    assert any(not torch.equal(want_b, twin.ensemble([l])[1]) for l in batched), "the ensemble's mask equals every single fold's"
    assert torch.equal(ens.predict_mask(image, (64, 64), 0.5, batch_tiles=3), got_b)                  # the checkpoint's mirror axes; a short filled last chunk
    xb, box = nnunet.preprocess(bordered, ens.normalization_schemes)                                  # the crop is normalised on its own: its own twin
    assert box == (10, 106, 30, 190)
    want = twin.ensemble([tiling.predict_sliding_window_batched(xb, n, ens.num_heads, (64, 64), 0.5, True, (0, 1), batch_tiles=2).cpu() for n in nets])[1]
    got = ens.predict_mask(bordered, (64, 64), 0.5, (0, 1), batch_tiles=2)
    assert got.shape == (120, 200) and torch.equal(got[10:106, 30:190].cpu(), want) and int(got.sum()) == int(want.sum())
    for m in ens.models:
        m.network.check_finite()
    # one fold
    one = nnunet.load_fold_ensemble(folder, (1,), device=DEV)
    single = nnunet.load_trained_model_folder(folder, 1, device=DEV)
    for bt in (None, 2):
        assert torch.equal(one.predict_mask(bordered, (64, 64), 0.5, (0, 1), batch_tiles=bt), single.predict_mask(bordered, (64, 64), 0.5, (0, 1), batch_tiles=bt)), bt
    # postprocess= goes through the same function
    pp = ([post.KEEP_LARGEST], [{"labels_or_regions": [1, 2, 3]}])
    assert torch.equal(ens.predict_mask(image, (64, 64), 0.5, (0, 1), batch_tiles=2, postprocess=pp), post.apply_postprocessing(got_b.contiguous(), *pp))


def test_fold_ensemble_with_region_labels(tmp_path):
    """The region rule on the ensemble's logits: three nested regions, regions_class_order (3, 1, 2)."""
    plans, ds = fixtures()
    ds["labels"] = {"background": 0, "any": [1, 2, 3], "high": [2, 3], "top": 3}
    ds["regions_class_order"] = [3, 1, 2]
    spec = nnunet.network_spec(plans, "2d_reduced", ds, accept_regions=True)
    folder = _write_folds(str(tmp_path / "model"), plans, ds, spec, (41, 42, 43))
    image, bordered = _image()
    ens = nnunet.load_fold_ensemble(folder, (0, 1, 2), device=DEV)
    assert ens.num_heads == 3 and ens.spec["regions_class_order"] == [3, 1, 2]
    x, box = nnunet.preprocess(bordered, ens.normalization_schemes)
    assert box == (10, 106, 30, 190) and image.shape == (3, 96, 160)
    for bt in (2, None):
        if bt is None:
            folds = [tiling.predict_sliding_window_return_logits(x, m.network, 3, (64, 64), 0.5, True, (0, 1)).cpu() for m in ens.models]
        else:
            folds = [tiling.predict_sliding_window_batched(x, m.network, 3, (64, 64), 0.5, True, (0, 1), batch_tiles=bt).cpu() for m in ens.models]
        logits = twin.ensemble(folds)[0]
        want = nnunet.region_mask_u8(logits.to(DEV), [3, 1, 2], nnunet.REGION_THRESHOLD_F32)
        got = ens.predict_mask(bordered, (64, 64), 0.5, (0, 1), batch_tiles=bt)
        assert got.shape == (120, 200) and torch.equal(got[10:106, 30:190], want) and int(got.sum()) == int(want.sum()), bt
        assert set(got.unique().tolist()) <= {0, 1, 2, 3}


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_field(lib):
    heads = 2
    accs = [torch.ones((heads, HP, WP), device=DEV) for _ in range(9)]
    cnt = torch.ones((HP, WP), device=DEV)
    mask = torch.full((HP, WP), 9, dtype=torch.uint8, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(n_folds=2, null_at=None, heads_=heads, y0=0, h=HP, mh=HP, my0=0):
        table = (C.c_void_p * 9)(*[None if k == null_at else a.data_ptr() for k, a in enumerate(accs)])
        return lib.ldiff_op_window_finish_ensemble(table, n_folds, _lib.ptr(cnt), heads_, HP, WP, y0, 0, h, WP, 0, None, _lib.ptr(mask), mh, WP, my0, 0, _lib.ptr(flag), stream)

    def refused(rc, field):
        assert rc == -1 and field in lib.ldiff_last_error().decode(), (rc, lib.ldiff_last_error())

    refused(call(n_folds=0), "n_folds 0")
    refused(call(n_folds=9), "n_folds 9")
    refused(call(n_folds=3, null_at=1), "acc[1] is null")
    refused(call(heads_=33), "heads")
    refused(call(y0=1), "leaves the padded extent")
    refused(call(h=HP + 1, mh=HP + 1), "leaves the padded extent")
    refused(call(my0=1), "leaves the mask")
    refused(lib.ldiff_op_window_finish_ensemble(None, 1, None, heads, HP, WP, 0, 0, HP, WP, 0, None, None, 0, 0, 0, 0, _lib.ptr(flag), stream), "null argument")
    torch.cuda.synchronize()
    assert int((mask != 9).sum()) == 0 and int(flag.item()) == 0                        # nothing was enqueued
    assert call(n_folds=3, null_at=5) == 0 and call(n_folds=8) == 0                    # entries past n_folds are not read; eight folds are taken
    torch.cuda.synchronize()
    assert int(mask.sum()) == 0
    # the Python surface
    with pytest.raises(ValueError, match="n_folds 0"):
        tiling.window_finish_ensemble([], cnt, (0, 0, HP, WP), flag, mask=mask)
    with pytest.raises(ValueError, match="n_folds 9"):
        tiling.window_finish_ensemble(accs, cnt, (0, 0, HP, WP), flag, mask=mask)
    with pytest.raises(ValueError, match="accumulator 1"):
        tiling.window_finish_ensemble([accs[0], accs[1].half()], cnt, (0, 0, HP, WP), flag, mask=mask)
    with pytest.raises(ValueError, match="accumulator 2"):
        tiling.window_finish_ensemble([accs[0], accs[1], accs[2][:, :, :32]], cnt, (0, 0, HP, WP), flag, mask=mask)
    with pytest.raises(ValueError, match="`cnt`"):
        tiling.window_finish_ensemble(accs[:2], cnt.half(), (0, 0, HP, WP), flag, mask=mask)
    with pytest.raises(ValueError, match="networks"):
        tiling.predict_sliding_window_ensemble(torch.zeros((3, 32, 32), device=DEV), [], 2, (32, 32))


# ---- 7. the stage ---------------------------------------------------------------------------------------------------------------------------------------------
def _png(path):
    from PIL import Image
    return np.array(Image.open(path).convert("L"), np.uint8)


def _run_stage(tmp, **kw):
    import test_gpu_nnunet_prep as prep
    from ldiffusion_amd.segmentor import Segmentor
    images, labels = prep._write_dataset(str(tmp / "src"))
    with pytest.MonkeyPatch.context() as mp:
        for name in ("nnUNet_raw", "nnUNet_preprocessed", "nnUNet_results"):
            (tmp / name).mkdir()
            mp.setenv(name, str(tmp / name))
        mp.setattr(Segmentor, "load_ldiffusion", lambda self, w, p, **k: (None, None, None))   # mixed sizes: no sampler runs
        seg = Segmentor(None, None, "tissue", 7)
        folder = seg.train_tissue_model_nnUNetv2(1, "weights", "sd", images, labels, images[:2], labels[:2], iterations_per_epoch=2, val_iterations=1,
                                                 num_foreground_voxels=6e4, postprocessing=True, **kw)
    splits = json.loads((tmp / "nnUNet_preprocessed" / "Dataset001_Custom" / "splits_final.json").read_text())
    return dict(tmp=tmp, folder=folder, raw=tmp / "nnUNet_raw" / "Dataset001_Custom", splits=splits, images=images, seg=seg)


@pytest.fixture(scope="module")
def stage(tmp_path_factory):
    """tests/test_gpu_nnunet_post.py's stage (six images, one epoch of two iterations, postprocessing=True) with folds=(0, 1)."""
    return _run_stage(tmp_path_factory.mktemp("fold_stage"), folds=(0, 1))


def test_stage_trains_and_validates_each_fold(stage):
    folder, splits = stage["folder"], stage["splits"]
    assert len(splits) == 5 and len(splits[0]["val"]) == 2 and len(splits[1]["val"]) == 1
    for f in (0, 1):
        fold_dir = os.path.join(folder, f"fold_{f}")
        assert sorted(os.listdir(fold_dir)) == ["checkpoint_best.pth", "checkpoint_final.pth", "validation"]
        for name in ("checkpoint_best.pth", "checkpoint_final.pth"):
            assert torch.load(os.path.join(fold_dir, name), map_location="cpu", weights_only=False)["init_args"]["fold"] == f
        assert sorted(os.listdir(os.path.join(fold_dir, "validation"))) == sorted([k + ".png" for k in splits[f]["val"]] + ["summary.json"])   # the fit is on the merged folder
    assert sorted(n for n in os.listdir(folder) if n.startswith("fold_")) == ["fold_0", "fold_1"]
    w0, w1 = (torch.load(os.path.join(folder, f"fold_{f}", "checkpoint_final.pth"), map_location="cpu", weights_only=False)["network_weights"] for f in (0, 1))
    assert any(not torch.equal(w0[k], w1[k]) for k in w0)
    seg = stage["seg"]
    assert sorted(seg.training_logs) == [0, 1] and seg.training_log is seg.training_logs[1]
    assert sorted(seg.validation_summaries) == [0, 1] and seg.validation_summary is seg.validation_summaries[1]
    assert len(seg.validation_summaries[0]["metric_per_case"]) == 2 and len(seg.validation_summaries[1]["metric_per_case"]) == 1


def test_stage_merges_the_folds_and_fits_the_postprocessing_once(stage):
    folder, splits, raw = stage["folder"], stage["splits"], stage["raw"]
    merged = os.path.join(folder, "crossval_results_folds_0_1")
    keys = sorted(splits[0]["val"] + splits[1]["val"])
    assert len(keys) == 3
    assert sorted(os.listdir(merged)) == sorted([k + ".png" for k in keys] + ["dataset.json", "plans.json", "summary.json", "postprocessing.json", "postprocessed"])
    for f in (0, 1):
        for k in splits[f]["val"]:
            assert np.array_equal(_png(os.path.join(merged, k + ".png")), _png(os.path.join(folder, f"fold_{f}", "validation", k + ".png")))
    lors = [1, 2, 3, 4, 5, 6]
    preds = [_png(os.path.join(merged, k + ".png")) for k in keys]
    refs = [_png(raw / "labelsTr" / (k + ".png")) for k in keys]
    want = ref.summarize([ref.case_metrics(r, p, lors) for p, r in zip(preds, refs)])
    summary = post.load_summary_json(os.path.join(merged, "summary.json"))
    assert ref.same_metrics(summary["mean"], want["mean"], ordered=False) and len(summary["metric_per_case"]) == 3
    assert ref.same_metrics({"fg": summary["foreground_mean"]}, {"fg": want["foreground_mean"]}, ordered=False)
    assert ref.same_metrics(stage["seg"].crossval_summary["mean"], want["mean"])
    fns, kwargs, baseline, final, masks = ref.determine_postprocessing(preds, refs, lors, lors)
    record = json.load(open(os.path.join(merged, "postprocessing.json")))
    assert record["postprocessing_fns"] == fns and record["postprocessing_kwargs"] == json.loads(json.dumps(kwargs))
    for k, m in zip(keys, masks):
        assert np.array_equal(_png(os.path.join(merged, "postprocessed", k + ".png")), m)


def test_stage_inference_with_the_folds(stage, tmp_path, monkeypatch):
    from PIL import Image
    from ldiffusion_amd.segmentor import Segmentor
    folder = stage["folder"]
    record = os.path.join(folder, "crossval_results_folds_0_1", "postprocessing.json")
    monkeypatch.setattr(Segmentor, "load_ldiffusion", lambda self, w, p, **k: (None, None, None))   # non-square images skip the diffusion
    seg = Segmentor(None, None, "tissue", 7)
    ens = nnunet.load_fold_ensemble(folder, (0, 1), device=DEV)

    def data(i):
        return torch.from_numpy(np.array(Image.open(stage["images"][i]).convert("RGB"))).to(DEV).permute(2, 0, 1).float()

    want = ens.predict_mask(data(2), postprocess=record).cpu().numpy()
    _, got = seg.inference_tissue_model_nnUNetv2(stage["images"][2], "sd", "weights", folder, use_folds=(0, 1), postprocess=True)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(want, ref.apply_postprocessing(ens.predict_mask(data(2)).cpu().numpy(), *post.load_postprocessing(record)))
    _, batched = seg.inference_tissue_model_nnUNetv2(stage["images"][2], "sd", "weights", folder, use_folds=(0, 1), batch_tiles=2)
    assert np.array_equal(batched, ens.predict_mask(data(2), batch_tiles=2).cpu().numpy())
    assert len(seg._tissue_heads) == 1 and isinstance(next(iter(seg._tissue_heads.values())), nnunet.FoldEnsemble)       # built once for both calls
    src = tmp_path / "in"
    src.mkdir()
    for i in (2, 3):
        Image.open(stage["images"][i]).save(src / f"img{i}.png")
    for extra, out in (({}, tmp_path / "out"), ({"batch_images": 2}, tmp_path / "out_batched")):
        assert seg.inference_tissue_model_nnUNetv2(str(src), "sd", "weights", folder, output_path=str(out), use_folds=(0, 1), postprocess=True, **extra) == (None, None)
        for i in (2, 3):
            assert np.array_equal(_png(out / f"img{i}.png"), ens.predict_mask(data(i), postprocess=record).cpu().numpy()), (extra, i)
    _, fold0 = seg.inference_tissue_model_nnUNetv2(stage["images"][2], "sd", "weights", folder)        # without the keyword: fold 0's head
    assert np.array_equal(fold0, nnunet.load_trained_model_folder(folder, 0, device=DEV).predict_mask(data(2)).cpu().numpy())


def test_stage_without_the_keyword_writes_fold_0_as_before(stage, tmp_path):
    """The same call without `folds`: what tests/test_gpu_nnunet_post.py::test_validation_folder_and_summary expects of the folder; and fold 0 of the
    `folds=(0, 1)` stage started from the same weights, drew the same patches and so wrote the same checkpoint and the same validation masks."""
    s = _run_stage(tmp_path)
    for name in ("checkpoint_final.pth", "checkpoint_best.pth"):
        a, b = (torch.load(os.path.join(d, "fold_0", name), map_location="cpu", weights_only=False)["network_weights"] for d in (s["folder"], stage["folder"]))
        differ = [k for k in a if not torch.equal(a[k], b[k])]
        print(f"fold 0, {name}: {len(differ)} of {len(a)} tensors differ between folds=None and folds=(0, 1)")
        assert list(a) == list(b) and not differ, differ[:3]
    for k in s["splits"][0]["val"]:
        assert np.array_equal(_png(os.path.join(s["folder"], "fold_0", "validation", k + ".png")), _png(os.path.join(stage["folder"], "fold_0", "validation", k + ".png")))
    folder, keys = s["folder"], s["splits"][0]["val"]
    val = os.path.join(folder, "fold_0", "validation")
    assert sorted(n for n in os.listdir(folder)) == ["dataset.json", "fold_0", "plans.json"]
    assert sorted(os.listdir(os.path.join(folder, "fold_0"))) == ["checkpoint_best.pth", "checkpoint_final.pth", "validation"]
    assert sorted(os.listdir(val)) == sorted([k + ".png" for k in keys] + ["summary.json", "postprocessing.json", "postprocessed"])
    assert torch.load(os.path.join(folder, "fold_0", "checkpoint_final.pth"), map_location="cpu", weights_only=False)["init_args"]["fold"] == 0
    assert s["seg"].crossval_summary is None and sorted(s["seg"].validation_summaries) == [0]
    preds = [_png(os.path.join(val, k + ".png")) for k in keys]
    refs = [_png(s["raw"] / "labelsTr" / (k + ".png")) for k in keys]
    want = ref.summarize([ref.case_metrics(r, p, [1, 2, 3, 4, 5, 6]) for p, r in zip(preds, refs)])
    assert ref.same_metrics(post.load_summary_json(os.path.join(val, "summary.json"))["mean"], want["mean"], ordered=False)
    assert ref.same_metrics(s["seg"].validation_summary["mean"], want["mean"])
