"""-m gpu: the batched sliding window of the tissue head -- ldiff_op_window_gather / _accumulate_batch / _finish through ldiffusion_amd.tiling,
TrainedModel.predict_mask(batch_tiles=) and Segmentor.inference_tissue_model_nnUNetv2(batch_tiles=).  Every comparison is bit for bit: against torch.flip of
the padded slices, against the reference's recorded sliding-window output (tests/golden/reference_sliding_window.npz), against the per-tile path's
accumulators, and against the host twin (tests/window_twin.py, pinned to the same fixture by tests/test_cpu_window_plan.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import nnunet_ref
import window_twin
from ldiffusion_amd import _lib, nnunet, tiling
from ldiffusion_amd.pipeline import argmax_mask

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
ALL_AXES = (None, (0,), (1,), (0, 1))


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- 1. gather ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(20, 27), (70, 90)])
def test_gather_equals_flips_of_the_padded_slices(hw):
    """C = 3, tile 32 x 48, step 0.5 (20 x 27 is padded in both axes; 70 x 90 has 12 tiles at origins that are no multiple of 4): every variant list against
    torch.flip of the padded image's slices; a source whose rows and planes are further apart than its extent; the pad exactly zero."""
    g = torch.Generator().manual_seed(hw[0])
    img = torch.randn((3,) + hw, generator=g) - 3.0          # no zeros of its own: a zero in the batch is the pad's
    big = torch.full((3, hw[0] + 3, hw[1] + 5), 7.0)
    big[:, 1:1 + hw[0], 2:2 + hw[1]] = img
    view = big.to(DEV)[:, 1:1 + hw[0], 2:2 + hw[1]]
    assert view.stride(1) > hw[1] and view.stride(0) > hw[0] * view.stride(1)
    for axes in ALL_AXES:
        plan = tiling.window_plan(hw, (32, 48), 0.5, axes, 1)
        want = window_twin.gather(img, plan, plan.origins)
        got = tiling.window_gather(img.to(DEV), plan, plan.origins)
        assert got.shape == (len(plan.origins) * len(plan.variants), 3, 32, 48) and torch.equal(got.cpu(), want), axes
        assert torch.equal(tiling.window_gather(view, plan, plan.origins).cpu(), want), axes
        # the same tiles chunk by chunk into one reused batch, a short last chunk filled with its last tile
        plan5 = tiling.window_plan(hw, (32, 48), 0.5, axes, 5)
        x, M = torch.empty((plan5.batch, 3, 32, 48), device=DEV), len(plan5.variants)
        at = 0
        for origins, n_valid in plan5.chunks:
            tiling.window_gather(view, plan5, origins, out=x)
            assert torch.equal(x[:n_valid * M].cpu(), want[at * M:(at + n_valid) * M])
            assert all(torch.equal(x[k * M:(k + 1) * M], x[(n_valid - 1) * M:n_valid * M]) for k in range(n_valid, 5))
            at += n_valid
    if hw == (20, 27):
        plan = tiling.window_plan(hw, (32, 48), 0.5, None, 1)
        got = tiling.window_gather(view, plan, plan.origins).cpu()
        inside = torch.zeros((32, 48), dtype=torch.bool)
        inside[plan.revert] = True
        assert plan.pad == (6, 10) and bool((got[0].view(torch.int32)[:, ~inside] == 0).all()) and bool((got[0][:, inside] != 0).all())


# ---- 2. accumulate + finish against the reference's recorded output -----------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1, 2, "all"])
def test_batched_window_reproduces_the_reference_fixture_bit_for_bit(chunk):
    """Cases a, b, c of the reference's own predictor code with torch.equal.  The network runs on the CPU inside the wrapper, so only the new kernels do
    arithmetic on the device.  (The per-tile device path is within one fp16 ulp here: torch's device half division; tests/test_gpu_models.py.)"""
    z = np.load(os.path.join(GOLDEN, "reference_sliding_window.npz"))
    cpu_net = window_twin.sw_network(torch.from_numpy(z["head_weight"]))

    def net(x):
        return cpu_net(x.cpu()).to(DEV)
    for tag in "abc":
        th, tw, step, mm = z[tag + "_cfg"]
        mirror = None if mm < 0 else tuple(i for i in range(2) if (int(mm) >> i) & 1)
        b = int(z[tag + "_n_slicers"]) if chunk == "all" else chunk
        got = tiling.predict_sliding_window_batched(torch.from_numpy(z[tag + "_image"]).to(DEV), net, 4, (int(th), int(tw)), float(step), True, mirror, batch_tiles=b)
        ref = torch.from_numpy(z[tag + "_logits_f16"])
        print(f"batched window {tag}, batch_tiles {b}: {int((got.cpu() != ref).sum())} of {ref.numel()} elements differ from the reference fixture")
        assert got.is_cuda and got.dtype == torch.float16 and torch.equal(got.cpu(), ref), tag
    small = torch.from_numpy(z["a_image"])[:, :20, :27].to(DEV)
    out = tiling.predict_sliding_window_batched(small, net, 4, (32, 32), 0.5, True, (0, 1), batch_tiles=1 if chunk == "all" else chunk)
    assert out.shape == (4, 20, 27) and torch.isfinite(out.float()).all()
    assert torch.equal(out.cpu(), tiling.predict_sliding_window_return_logits(small.cpu(), cpu_net, 4, (32, 32), 0.5, True, (0, 1)))
    with pytest.raises(RuntimeError, match="Encountered inf in predicted array"):
        tiling.predict_sliding_window_batched(torch.full((3, 32, 32), 6e4, device=DEV), lambda x: x[:, :1] * 10.0, 1, (32, 32), 1.0, True, None)


# ---- 3. all dtype kinds against the per-tile path -----------------------------------------------------------------------------------------------------
def lookup_network(heads, dtype, seed):
    """Predictions that depend on the input pixel AND on the position inside the tile (a table), through elementwise ops only: every batch entry is
    computed alone, so the per-tile path and any batch see the same values, and a prediction that is not flipped back lands on the wrong table entry."""
    g = torch.Generator().manual_seed(seed)
    wa, wb = (torch.randn((1, heads, 1, 1), generator=g).to(DEV) for _ in range(2))
    table = (torch.randn((1, heads, 32, 32), generator=g) * 3).to(DEV)

    def network(x):
        return (x[:, 0:1] * wa + x[:, 1:2] * wb + table).to(dtype)
    return network


def per_tile_accumulators(image, network, heads, tile_hw, step, axes, acc_dtype):
    """predict_sliding_window_return_logits' loop (its own helpers, its order) stopped before the division."""
    th, tw = tile_hw
    data, _ = tiling.pad_to_tile(image, tile_hw)
    acc = torch.zeros((heads,) + tuple(data.shape[1:]), dtype=acc_dtype, device=data.device)
    cnt = torch.zeros(tuple(data.shape[1:]), dtype=acc_dtype, device=data.device)
    g = tiling.compute_gaussian((th, tw), sigma_scale=1.0 / 8, value_scaling_factor=10, dtype=acc_dtype, device=data.device)
    for y, x in tiling.tile_origins(tuple(data.shape[1:]), tile_hw, step):
        tiling._window_accumulate(acc, cnt, tiling.maybe_mirror_and_predict(network, data[None, :, y:y + th, x:x + tw], axes)[0], g, y, x)
    return acc, cnt


@pytest.mark.parametrize("heads", [1, 4, 7])
@pytest.mark.parametrize("acc_dtype", [torch.float16, torch.float32], ids=["acc16", "acc32"])
@pytest.mark.parametrize("pred_dtype", [torch.float32, torch.float16], ids=["pred32", "pred16"])
def test_accumulators_equal_the_per_tile_path_bit_for_bit(pred_dtype, acc_dtype, heads):
    """80 x 72, tile 32 x 32, steps 0.5 and 0.3 (up to 16 tiles over one pixel), every mirror_axes: acc and cnt equal the per-tile path's before its division,
    whatever batch_tiles (1, 5 with a short filled last chunk, all tiles up to the cap); the logits equal the host's division of those accumulators and, with
    float32 accumulators, the per-tile path's own."""
    image = (torch.randn((3, 80, 72), generator=torch.Generator().manual_seed(heads)) * 2).to(DEV)
    network = lookup_network(heads, pred_dtype, 100 + heads)
    for step in (0.5, 0.3):
        n = len(tiling.tile_origins((80, 72), (32, 32), step))
        for axes in ALL_AXES:
            acc0, cnt0 = per_tile_accumulators(image, network, heads, (32, 32), step, axes, acc_dtype)
            for b in (1, 5, min(n, tiling.WINDOW_MAX_TILES)):
                acc, cnt, plan = tiling.window_accumulate_image(image, network, heads, (32, 32), step, True, axes, acc_dtype, b)
                assert torch.equal(acc, acc0) and torch.equal(cnt, cnt0), (step, axes, b)
            assert int(cnt0.cpu().float().max()) > 0 and len(plan.origins) == n
            logits = tiling.predict_sliding_window_batched(image, network, heads, (32, 32), step, True, axes, acc_dtype, batch_tiles=5)
            assert logits.dtype == acc_dtype and torch.equal(logits.cpu(), acc0.cpu() / cnt0.cpu()), (step, axes)
            if acc_dtype == torch.float32:
                assert torch.equal(logits, tiling.predict_sliding_window_return_logits(image, network, heads, (32, 32), step, True, axes, acc_dtype)), (step, axes)
    # the host twin from the image up (its own gather, average and accumulation), at one setting per case
    acc_t, cnt_t, _ = window_twin.accumulate_image(image.cpu(), lambda x: network(x.to(DEV)).cpu(), heads, (32, 32), 0.3, True, (0, 1), acc_dtype, 5)
    assert torch.equal(acc_t, acc0.cpu()) and torch.equal(cnt_t, cnt0.cpu())


def test_filler_tiles_have_no_effect_and_weightless_accumulation():
    """n_valid < n_tiles: predictions of the filler entries (NaN here) and their origins are never read; g = None is weight 1."""
    heads, M = 3, 2
    g = torch.Generator().manual_seed(3)
    origins = [(0, 0), (5, 17), (16, 8), (16, 8)]
    pred = torch.randn((len(origins) * M, heads, 32, 32), generator=g).to(DEV)
    for acc_dtype in (torch.float32, torch.float16):
        gm = tiling.compute_gaussian((32, 32), 1.0 / 8, 10, acc_dtype, DEV)
        for weight in (gm, None):
            acc, cnt = torch.zeros((heads, 48, 49), dtype=acc_dtype, device=DEV), torch.zeros((48, 49), dtype=acc_dtype, device=DEV)
            tiling.window_accumulate_batch(acc, cnt, pred[:3 * M], weight, origins[:3], 3, [0, 2])
            poisoned = pred.clone()
            poisoned[3 * M:] = float("nan")
            acc2, cnt2 = torch.zeros_like(acc), torch.zeros_like(cnt)
            tiling.window_accumulate_batch(acc2, cnt2, poisoned, weight, origins, 3, [0, 2])
            assert torch.equal(acc, acc2) and torch.equal(cnt, cnt2) and not bool(torch.isnan(acc2.float()).any())
            acc_t, cnt_t = torch.zeros_like(acc, device="cpu"), torch.zeros_like(cnt, device="cpu")
            window_twin.accumulate_chunk(acc_t, cnt_t, pred.cpu(), None if weight is None else weight.cpu(), origins, 3, [0, 2])
            assert torch.equal(acc.cpu(), acc_t) and torch.equal(cnt.cpu(), cnt_t)
            if weight is None:
                assert set(cnt.cpu().float().unique().tolist()) <= {0.0, 1.0, 2.0, 3.0}


# ---- 4. mask ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("acc_dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("w", [44, 45])
def test_finish_mask_follows_the_argmax_rule_and_the_crop_box(acc_dtype, w):
    """Crafted accumulators (w = 44: whole vectors; 45: the element path): the mask equals argmax_mask(logits) placed by uncrop_mask, with a tie (first class),
    a NaN logit (class 0), and a +inf accumulator (flag)."""
    g = torch.Generator().manual_seed(w)
    heads, Hp, Wp, box = 5, 40, 52, (4, 4, 30, w)
    acc = (torch.randn((heads, Hp, Wp), generator=g) * 20).to(acc_dtype)
    cnt = (torch.rand((Hp, Wp), generator=g) * 30 + 0.5).to(acc_dtype)
    acc[:, 10, 9] = torch.tensor([1.0, 7.0, 7.0, -2.0, 7.0]).to(acc_dtype)          # classes 1, 2, 4 tie: class 1
    acc[:, 12, 13] = torch.tensor([1.0, 2.0, 3.0, float("nan"), 1.0]).to(acc_dtype)  # a NaN logit: class 0
    accd, cntd = acc.to(DEV), cnt.to(DEV)

    def run(a):
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        logits = torch.empty((heads, box[2], box[3]), dtype=acc_dtype, device=DEV)
        mask = torch.zeros((50, 64), dtype=torch.uint8, device=DEV)
        tiling.window_finish(a, cntd, box, flag, logits=logits, mask=mask, mask_origin=(8, 12))
        only_mask = torch.zeros_like(mask)
        tiling.window_finish(a, cntd, box, torch.zeros_like(flag), mask=only_mask, mask_origin=(8, 12))
        assert torch.equal(mask, only_mask)
        return logits, mask, int(flag.item())

    logits, mask, flag = run(accd)
    want_logits = (acc / cnt)[:, box[0]:box[0] + box[2], box[1]:box[1] + box[3]]
    assert flag == 0                                                                  # NaN is not inf
    assert torch.equal(torch.nan_to_num(logits.cpu().float(), nan=12345.0), torch.nan_to_num(want_logits.float(), nan=12345.0))
    placed = nnunet.uncrop_mask(argmax_mask(logits[None].float())[0], (8, 8 + box[2], 12, 12 + box[3]), (50, 64))
    assert torch.equal(mask, placed) and torch.equal(mask.cpu()[8:8 + box[2], 12:12 + box[3]], window_twin.argmax_rule(want_logits))
    assert int(mask[8 + 6, 12 + 5]) == 1 and int(mask[8 + 8, 12 + 9]) == 0 and bool(torch.isnan(logits[3, 8, 9]))
    assert int(mask.sum()) == int(mask[8:8 + box[2], 12:12 + box[3]].sum())                        # nothing outside the crop box
    inf = accd.clone()
    inf[2, 20, 21] = float("inf")
    logits, mask, flag = run(inf)
    assert flag == 1 and int(mask[8 + 16, 12 + 17]) == 0 and bool(torch.isinf(logits[2, 16, 17]))
    ninf = accd.clone()
    ninf[2, 20, 21] = float("-inf")
    assert run(ninf)[2] == 1
    outside = accd.clone()
    outside[2, 2, 2] = float("inf")                                                               # outside the box: not looked at
    assert run(outside)[2] == 0


def test_return_mask_of_the_predictor():
    image = (torch.randn((3, 50, 61), generator=torch.Generator().manual_seed(8)) * 2).to(DEV)
    network = lookup_network(4, torch.float32, 9)
    for axes in (None, (0, 1)):
        logits = tiling.predict_sliding_window_batched(image, network, 4, (32, 32), 0.5, True, axes, batch_tiles=4)
        out = torch.zeros((70, 80), dtype=torch.uint8, device=DEV)
        mask = tiling.predict_sliding_window_batched(image, network, 4, (32, 32), 0.5, True, axes, batch_tiles=4, return_mask=True, mask_out=out, mask_origin=(7, 9))
        assert mask is out and torch.equal(mask, nnunet.uncrop_mask(argmax_mask(logits[None].float())[0], (7, 57, 9, 70), (70, 80)))
        plain = tiling.predict_sliding_window_batched(image, network, 4, (32, 32), 0.5, True, axes, batch_tiles=4, return_mask=True)
        assert torch.equal(plain, argmax_mask(logits[None].float())[0]) and int(plain.max()) > 0
    with pytest.raises(RuntimeError, match="Encountered inf in predicted array"):
        tiling.predict_sliding_window_batched(torch.full((3, 32, 32), 6e4, device=DEV), lambda x: x[:, :1] * 10.0, 1, (32, 32), 1.0, True, None, return_mask=True)


# ---- 5. the library's head, end to end -----------------------------------------------------------------------------------------------------------------
def fixtures():
    import json
    with open(os.path.join(GOLDEN, "nnunet_plans_2d.json")) as f:
        plans = json.load(f)
    with open(os.path.join(GOLDEN, "nnunet_dataset.json")) as f:
        ds = json.load(f)
    return plans, ds


def test_predict_mask_batched_equals_the_per_tile_path_with_the_library_head():
    """2d_reduced, image 96 x 160, tile 64 x 64, step 0.5, mirrors (0, 1): 8 tiles x 4 variants.  batch_tiles 1, 2, 3 (the last with a short filled chunk) give the
    per-tile path's mask bit for bit; the second image of the same size re-captures nothing; check_finite stays clean; an all-zero border (the crop box a proper
    sub-rectangle) goes through the finish kernel's un-crop."""
    from ldiffusion_amd.models import PlainConvUNet
    plans, ds = fixtures()
    spec = nnunet.network_spec(plans, "2d_reduced", ds)
    sd = nnunet_ref.synthetic_state_dict(spec, 31)
    g = torch.Generator().manual_seed(77)
    smooth = torch.nn.functional.avg_pool2d(torch.rand((2, 3, 104, 168), generator=g), 9, 1)          # [2, 3, 96, 160]
    images = (smooth * 254 + 1).to(DEV)
    bordered = torch.zeros((3, 120, 200), device=DEV)
    bordered[:, 10:106, 30:190] = images[0]
    ref_model = nnunet.TrainedModel(PlainConvUNet(spec, sd, DEV), spec, (0, 1))
    refs = [ref_model.predict_mask(im, (64, 64), 0.5, (0, 1)) for im in images]
    ref_bordered = ref_model.predict_mask(bordered, (64, 64), 0.5, (0, 1))
    assert nnunet.nonzero_bbox(bordered) == (10, 106, 30, 190) and torch.equal(ref_bordered[10:106, 30:190], refs[0]) and int(refs[0].max()) > 0
    for b in (1, 2, 3):
        model = nnunet.TrainedModel(PlainConvUNet(spec, sd, DEV), spec, (0, 1))
        calls = -(-8 // b)
        got = model.predict_mask(images[0], (64, 64), 0.5, (0, 1), batch_tiles=b)
        assert got.dtype == torch.uint8 and got.shape == (96, 160) and torch.equal(got, refs[0]), b
        assert model.network.graph_replays == calls - 1            # eager, capture + replay, then replays
        got = model.predict_mask(images[1], (64, 64), 0.5, (0, 1), batch_tiles=b)
        assert torch.equal(got, refs[1]), b
        assert model.network.graph_replays == 2 * calls - 1, "the second image of the same size re-captured the graph"
        got = model.predict_mask(bordered, (64, 64), 0.5, (0, 1), batch_tiles=b)
        assert got.shape == (120, 200) and torch.equal(got, ref_bordered), b
        assert model.network.graph_replays == 3 * calls - 1
        model.network.check_finite()


# ---- 6. Segmentor ---------------------------------------------------------------------------------------------------------------------------------------
def test_segmentor_forwards_batch_tiles(tmp_path):
    """inference_tissue_model_nnUNetv2(..., batch_tiles=2) on a trained-model folder, non-square image (no diffusion): the mask of the call without the
    keyword; the same for an injected predictor that accepts a batch, and through LDiffusionModel.inference."""
    from PIL import Image
    import test_gpu_models as tgm
    from ldiffusion_amd import configs, weights
    from ldiffusion_amd.ldiffusion import LDiffusionModel
    from ldiffusion_amd.segmentor import Segmentor
    tiny = dict(ucfg=configs.TINY_UNET, vcfg=configs.TINY_VAE, usd=weights.synthetic_state_dict(weights.unet_param_shapes(configs.TINY_UNET), 42, fp16_values=True),
                vsd=weights.synthetic_state_dict(weights.vae_param_shapes(configs.TINY_VAE), 43, fp16_values=True))
    sd_dir, w_dir, _ = tgm._write_sd_dirs(tmp_path, tiny, torch.float32, torch.float32)
    plans, ds = fixtures()
    plans["configurations"]["2d_reduced"]["patch_size"] = [128, 128]
    spec = nnunet.network_spec(plans, "2d_reduced", ds)
    sd = nnunet_ref.synthetic_state_dict(spec, 41)
    folder = nnunet_ref.write_model_folder(str(tmp_path / "tissue_model"), plans, ds, sd, spec, "2d_reduced", mirror_axes=(1,))
    rng = np.random.default_rng(9)
    rect = tmp_path / "rect.png"
    border = np.zeros((200, 260, 3), np.uint8)
    smooth = torch.nn.functional.avg_pool2d(torch.from_numpy(rng.random((1, 3, 170, 230))).float(), 9, 1, 4)[0].permute(1, 2, 0).numpy()
    border[20:190, 15:245] = np.clip(smooth * 255, 1, 255).astype(np.uint8)
    Image.fromarray(border).save(rect)
    seg = Segmentor(None, None, "tissue", 4)
    _, ref = seg.inference_tissue_model_nnUNetv2(str(rect), str(sd_dir), str(w_dir), folder)
    _, got = seg.inference_tissue_model_nnUNetv2(str(rect), str(sd_dir), str(w_dir), folder, batch_tiles=2)
    assert got.shape == (200, 260) and got.dtype == np.uint8 and np.array_equal(got, ref) and ref.max() > 0 and not ref[:20].any()
    _, via_model = LDiffusionModel(str(sd_dir), "tissue").inference(str(rect), str(w_dir), folder, 4, batch_tiles=2)
    assert np.array_equal(via_model, ref)
    predictor = lookup_network(4, torch.float32, 12)
    _, got_p = seg.inference_tissue_model_nnUNetv2(str(rect), str(sd_dir), str(w_dir), None, predictor=predictor, tile_size=(32, 32), mirror_axes=(0, 1), num_heads=4,
                                                   batch_tiles=7)
    _, one_p = seg.inference_tissue_model_nnUNetv2(str(rect), str(sd_dir), str(w_dir), None, predictor=predictor, tile_size=(32, 32), mirror_axes=(0, 1), num_heads=4,
                                                   batch_tiles=1)
    assert got_p.shape == (200, 260) and got_p.max() > 0 and np.array_equal(got_p, one_p)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_field(lib):
    heads, Hp, Wp, th, tw = 2, 40, 48, 32, 32
    acc, cnt = torch.zeros((heads, Hp, Wp), device=DEV), torch.zeros((Hp, Wp), device=DEV)
    img, x = torch.zeros((3, Hp, Wp), device=DEV), torch.zeros((2, 3, th, tw), device=DEV)
    pred = torch.zeros((2, heads, th, tw), device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)

    def tiles(n_tiles=2, n_valid=2, n_variants=1, variants=(0,), y0=(0, 8), x0=(0, 16)):
        t = _lib.WindowTiles()
        t.n_tiles, t.n_valid, t.n_variants = n_tiles, n_valid, n_variants
        for i, v in enumerate(variants):
            t.variants[i] = v
        for i, (a, b) in enumerate(zip(y0, x0)):
            t.y0[i], t.x0[i] = a, b
        return t

    def accumulate(t, heads_=heads, dtypes=0):
        return lib.ldiff_op_window_accumulate_batch(_lib.ptr(acc), _lib.ptr(cnt), _lib.ptr(pred), None, heads_, Hp, Wp, th, tw, C.byref(t), dtypes, stream())

    def gather(t):
        return lib.ldiff_op_window_gather(_lib.ptr(img), 3, Hp, Wp, Wp, Hp * Wp, 0, 0, Hp, Wp, C.byref(t), th, tw, _lib.ptr(x), stream())

    def refused(rc, field):
        assert rc == -1 and field in lib.ldiff_last_error().decode(), (rc, lib.ldiff_last_error())

    assert accumulate(tiles()) == 0 and gather(tiles()) == 0
    for call in (accumulate, gather):
        refused(call(tiles(n_tiles=_lib.WINDOW_MAX_TILES + 1)), "n_tiles")         # more tiles per launch than the cap
        refused(call(tiles(y0=(0, Hp - th + 1))), "leaves the padded extent")       # a tile leaving the accumulator / the padded image
        refused(call(tiles(x0=(0, Wp - tw + 1))), "x0 = 17")
        refused(call(tiles(y0=(-1, 0))), "y0 = -1")
        refused(call(tiles(n_variants=3, variants=(0, 1, 2))), "n_variants")
        refused(call(tiles(n_variants=2, variants=(0, 4))), "variants[1]")
    refused(accumulate(tiles(n_valid=3)), "n_valid")
    refused(accumulate(tiles(), heads_=33), "heads")
    refused(accumulate(tiles(), dtypes=4), "dtypes")
    assert accumulate(tiles(n_valid=1, y0=(0, 1000))) == 0                              # a filler tile's origin is never used
    fin = lambda heads_=heads, y0=0, h=Hp, mh=Hp, my0=0: lib.ldiff_op_window_finish(_lib.ptr(acc), _lib.ptr(cnt), heads_, Hp, Wp, y0, 0, h, Wp, 0, None, _lib.ptr(x), mh, Wp,
                                                                                     my0, 0, _lib.ptr(flag), stream())
    refused(fin(heads_=33), "heads")
    refused(fin(y0=1), "leaves the padded extent")
    refused(fin(my0=1), "leaves the mask")
    torch.cuda.synchronize()
    want = torch.zeros((Hp, Wp))                                                         # zero predictions, weight 1: only the two accepted calls counted
    want[0:32, 0:32] += 2
    want[8:40, 16:48] += 1
    assert not acc.any() and torch.equal(cnt.cpu(), want)
    # the Python surface
    image = torch.zeros((3, 40, 48))
    net = lambda t: torch.zeros((t.shape[0], heads, th, tw), device=DEV)
    with pytest.raises(ValueError, match="on the device"):
        tiling.predict_sliding_window_batched(image, net, heads, (th, tw))                                     # a host tensor
    with pytest.raises(ValueError, match=r"expected \(8, 2, 32, 32\)"):
        tiling.predict_sliding_window_batched(image.to(DEV), lambda t: net(t)[:4], heads, (th, tw), mirror_axes=(0, 1), batch_tiles=2)   # a prediction of the wrong batch
    with pytest.raises(ValueError, match="device tensor"):
        tiling.predict_sliding_window_batched(image.to(DEV), lambda t: net(t).cpu(), heads, (th, tw))
    with pytest.raises(ValueError, match="num_heads"):
        tiling.predict_sliding_window_batched(image.to(DEV), net, 33, (th, tw))
    with pytest.raises(ValueError, match="batch_tiles"):
        tiling.predict_sliding_window_batched(image.to(DEV), net, heads, (th, tw), batch_tiles=_lib.WINDOW_MAX_TILES + 1)
    with pytest.raises(ValueError, match="float32 or float16"):
        tiling.predict_sliding_window_batched(image.to(DEV), lambda t: net(t).to(torch.bfloat16), heads, (th, tw))
