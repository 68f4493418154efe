"""CPU: the nnU-Net tissue head's host side (ldiffusion_amd/nnunet.py) -- plans -> layer list, what is refused, the checkpoint's key layout,
nnU-Net's preprocessing for a PNG -- and the float64 yardstick of the GPU tests (tests/nnunet_ref.py) against a second statement."""
import copy
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

import nnunet_ref
from ldiffusion_amd import nnunet

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def fixtures():
    with open(os.path.join(GOLDEN, "nnunet_plans_2d.json")) as f:
        plans = json.load(f)
    with open(os.path.join(GOLDEN, "nnunet_dataset.json")) as f:
        ds = json.load(f)
    return plans, ds


# ---- 1. plans -> layer list; refusals ----------------------------------------------------------------------------------------------------------
def test_plans_fixture_resolves_to_the_expected_layer_list():
    plans, ds = fixtures()
    s = nnunet.network_spec(plans, "2d", ds)
    assert s["in_channels"] == 3 and s["n_heads"] == 4 and s["n_stages"] == 7
    assert s["features"] == [32, 64, 128, 256, 512, 512, 512]           # min(32 * 2^i, 512)
    assert s["strides"] == [1, 2, 2, 2, 2, 2, 2]
    assert s["n_conv_encoder"] == [2] * 7 and s["n_conv_decoder"] == [2] * 6
    assert s["patch_size"] == (512, 512) and s["normalization_schemes"] == ["ZScoreNormalization"] * 3
    r = nnunet.network_spec(plans, "2d_reduced", ds)                      # inherits_from: the child's keys win, the rest is the parent's
    assert r["features"] == [32, 64, 128, 256] and r["patch_size"] == (64, 64) and r["normalization_schemes"] == ["ZScoreNormalization"] * 3
    six = nnunet.network_spec(plans, "2d_six", ds)                        # two levels of inheritance
    assert six["features"] == [32, 64, 128, 256, 512, 512] and six["patch_size"] == (128, 128)
    shapes = nnunet.param_shapes(r)
    assert shapes["encoder.stages.0.0.convs.0.conv.weight"] == (32, 3, 3, 3)
    assert shapes["encoder.stages.1.0.convs.0.conv.weight"] == (64, 32, 3, 3)
    assert shapes["decoder.transpconvs.0.weight"] == (256, 128, 2, 2)     # torch's ConvTranspose2d layout: [Cin, Cout, k, k]
    assert shapes["decoder.stages.0.convs.0.conv.weight"] == (128, 256, 3, 3)
    assert shapes["decoder.stages.2.convs.1.norm.bias"] == (32,)
    assert shapes["decoder.seg_layers.2.weight"] == (4, 32, 1, 1)
    assert not any(k.startswith("decoder.seg_layers.") and not k.startswith("decoder.seg_layers.2.") for k in shapes)
    assert len(shapes) == 4 * (8 + 6) + 2 * 3 + 2
    with pytest.raises(ValueError, match="does not exist"):
        nnunet.network_spec(plans, "3d_fullres", ds)


def _edit(path, value, plans=None, ds=None):
    plans0, ds0 = fixtures()
    plans, ds = copy.deepcopy(plans0), copy.deepcopy(ds0)
    tgt = {"plans": plans, "cfg": plans["configurations"]["2d"], "ds": ds}[path[0]]
    tgt[path[1]] = value
    return plans, ds


REFUSED = [
    (("cfg", "UNet_class_name"), "ResidualEncoderUNet", "UNet_class_name"),
    (("cfg", "conv_kernel_sizes"), [[3, 3, 3]] * 7, "conv_kernel_sizes"),
    (("cfg", "conv_kernel_sizes"), [[1, 3]] + [[3, 3]] * 6, "conv_kernel_sizes"),
    (("cfg", "pool_op_kernel_sizes"), [[1, 1], [2, 1]] + [[2, 2]] * 5, "pool_op_kernel_sizes"),
    (("cfg", "pool_op_kernel_sizes"), [[1, 1], [4, 4]] + [[2, 2]] * 5, "pool_op_kernel_sizes"),
    (("cfg", "use_mask_for_norm"), [True, False, False], "use_mask_for_norm"),
    (("plans", "transpose_forward"), [0, 2, 1], "transpose_forward"),
    (("cfg", "normalization_schemes"), ["CTNormalization"] * 3, "normalization_schemes"),
    (("ds", "labels"), {"background": 0, "whole": [1, 2], "core": [2]}, "labels"),
    (("ds", "labels"), {"background": 0, "a": 1, "ignore": 2}, "labels"),
    (("cfg", "previous_stage"), "2d_lowres", "previous_stage"),
    (("cfg", "UNet_base_num_features"), 24, "UNet_base_num_features"),
    (("cfg", "patch_size"), [500, 512], "patch_size"),
]


@pytest.mark.parametrize("path,value,field", REFUSED, ids=[f"{r[2]}-{i}" for i, r in enumerate(REFUSED)])
def test_every_refused_field_raises_with_its_name(path, value, field):
    plans, ds = _edit(path, value)
    with pytest.raises(ValueError, match=f"`{field}`"):
        nnunet.network_spec(plans, "2d", ds)


def test_several_folds_are_refused(tmp_path):
    plans, ds = fixtures()
    spec = nnunet.network_spec(plans, "2d_reduced", ds)
    nnunet_ref.write_model_folder(str(tmp_path / "m"), plans, ds, nnunet_ref.synthetic_state_dict(spec, 1), spec, "2d_reduced")
    with pytest.raises(ValueError, match="`use_folds`"):
        nnunet.read_trained_model_folder(str(tmp_path / "m"), fold=(0, 1))


# ---- 2. the loader's key layout ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compiled", [False, True])
def test_loader_drops_aliases_reports_missing_and_rejects_wrong_shapes(tmp_path, compiled):
    plans, ds = fixtures()
    spec = nnunet.network_spec(plans, "2d_reduced", ds)
    sd = nnunet_ref.synthetic_state_dict(spec, 7)
    full = nnunet_ref.checkpoint_like(sd, spec, compiled)
    assert len(full) > 2 * len(sd)                                         # the aliases are really there
    clean = nnunet.clean_state_dict(full, spec)
    assert set(clean) == set(sd) == set(nnunet.param_shapes(spec))
    assert all(torch.equal(clean[k], sd[k]) for k in sd)
    nnunet.check_state_dict(clean, spec)
    # through the folder, as the predictor reads it
    folder = nnunet_ref.write_model_folder(str(tmp_path / "model"), plans, ds, sd, spec, "2d_reduced", mirror_axes=(1,), compiled=compiled)
    spec2, sd2, axes = nnunet.read_trained_model_folder(folder)
    assert spec2 == spec and set(sd2) == set(sd) and tuple(axes) == (1,)
    missing = dict(clean)
    del missing["decoder.transpconvs.1.bias"]
    with pytest.raises(RuntimeError, match=r"decoder\.transpconvs\.1\.bias"):
        nnunet.check_state_dict(missing, spec)
    wrong = dict(clean)
    wrong["decoder.transpconvs.0.weight"] = wrong["decoder.transpconvs.0.weight"].permute(1, 0, 2, 3).contiguous()   # [Cout, Cin, k, k]: a Conv2d layout
    with pytest.raises(ValueError, match=r"decoder\.transpconvs\.0\.weight.*does not match"):
        nnunet.check_state_dict(wrong, spec)
    extra = dict(clean)
    extra["encoder.stages.0.0.convs.0.dropout.p"] = torch.zeros(1)
    with pytest.raises(ValueError, match="unexpected"):
        nnunet.check_state_dict(extra, spec)


# ---- 3. preprocessing against numpy statements of nnU-Net's formulas ----------------------------------------------------------------------------
def _np_reference(img, schemes):
    """DefaultPreprocessor.run_case_npy for [C, H, W] float32 in numpy: crop_to_nonzero's box, then default_normalization_schemes.py per channel."""
    nz = np.zeros(img.shape[1:], bool)
    for c in range(img.shape[0]):
        nz |= img[c] != 0
    ys, xs = np.where(nz.any(1))[0], np.where(nz.any(0))[0]
    box = (int(ys[0]), int(ys[-1]) + 1, int(xs[0]), int(xs[-1]) + 1)
    data = img[:, box[0]:box[1], box[2]:box[3]].astype(np.float32).copy()
    for c, s in enumerate(schemes):
        x = data[c]
        if s == "ZScoreNormalization":
            data[c] = (x - x.mean()) / max(x.std(), 1e-8)
        elif s == "RGBTo01Normalization":
            data[c] = x / 255.0
        elif s == "RescaleTo01Normalization":
            x = x - x.min()
            data[c] = x / np.clip(x.max(), a_min=1e-8, a_max=None)
    return data, box


def test_preprocessing_matches_numpy_statements_including_a_zero_border():
    rng = np.random.RandomState(3)
    img = np.zeros((3, 70, 90), np.float32)
    img[:, 5:61, 12:83] = rng.randint(0, 256, (3, 56, 71)).astype(np.float32)
    img[:, 5, 12:83] = 0                                                   # a zero row INSIDE the first row of the box in two channels only
    img[2, 5, 40] = 7
    for schemes in (["ZScoreNormalization"] * 3, ["RGBTo01Normalization", "RescaleTo01Normalization", "NoNormalization"]):
        ref, box = _np_reference(img, schemes)
        got, gbox = nnunet.preprocess(torch.from_numpy(img), schemes)
        assert gbox == box == (5, 61, 12, 83)
        assert got.dtype == torch.float32 and tuple(got.shape) == ref.shape
        np.testing.assert_allclose(got.numpy(), ref, rtol=0, atol=2e-6)    # float32 mean / std in two libraries: a few ulp of values of order 1
    # no border: the box is the image; a constant channel: std 0 -> max(std, 1e-8), all zeros
    full = rng.randint(1, 256, (3, 16, 16)).astype(np.float32)
    full[1] = 9.0
    got, box = nnunet.preprocess(torch.from_numpy(full), ["ZScoreNormalization"] * 3)
    assert box == (0, 16, 0, 16) and float(got[1].abs().max()) == 0.0
    # un-crop: label 0 outside the box
    m = torch.full((56, 71), 3, dtype=torch.uint8)
    u = nnunet.uncrop_mask(m, (5, 61, 12, 83), (70, 90))
    assert u.shape == (70, 90) and int(u.sum()) == 3 * 56 * 71 and int(u[:5].sum()) == 0 and int(u[:, 83:].sum()) == 0
    with pytest.raises(ValueError, match="normalization_schemes"):
        nnunet.normalize(torch.from_numpy(full), ["CTNormalization"] * 3)


# ---- 4. the yardstick against a second statement --------------------------------------------------------------------------------------------------
class _Block(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, 3, stride, 1, bias=True)
        self.norm = nn.InstanceNorm2d(cout, eps=1e-5, affine=True)
        self.nonlin = nn.LeakyReLU(0.01)

    def forward(self, x):
        return self.nonlin(self.norm(self.conv(x)))


class _Stack(nn.Module):
    def __init__(self, cin, cout, n, stride):
        super().__init__()
        self.convs = nn.Sequential(*[_Block(cin if i == 0 else cout, cout, stride if i == 0 else 1) for i in range(n)])

    def forward(self, x):
        return self.convs(x)


class _Net(nn.Module):
    """torch.nn modules under the attribute names that give the canonical state-dict keys."""

    def __init__(self, spec):
        super().__init__()
        f, n = spec["features"], spec["n_stages"]
        self.encoder = nn.Module()
        self.encoder.stages = nn.ModuleList([nn.Sequential(_Stack(spec["in_channels"] if s == 0 else f[s - 1], f[s], spec["n_conv_encoder"][s], spec["strides"][s]))
                                             for s in range(n)])
        self.decoder = nn.Module()
        self.decoder.transpconvs = nn.ModuleList([nn.ConvTranspose2d(f[n - 1 - j], f[n - 2 - j], 2, 2) for j in range(n - 1)])
        self.decoder.stages = nn.ModuleList([_Stack(2 * f[n - 2 - j], f[n - 2 - j], spec["n_conv_decoder"][j], 1) for j in range(n - 1)])
        self.decoder.seg_layers = nn.ModuleDict({str(n - 2): nn.Conv2d(f[0], spec["n_heads"], 1)})

    def forward(self, x):
        skips = []
        for st in self.encoder.stages:
            x = st(x)
            skips.append(x)
        for j, (up, st) in enumerate(zip(self.decoder.transpconvs, self.decoder.stages)):
            x = st(torch.cat((up(x), skips[-(j + 2)]), 1))
        return list(self.decoder.seg_layers.values())[0](x)


def test_restatement_agrees_with_torch_nn_modules():
    plans, ds = fixtures()
    spec = nnunet.network_spec(plans, "2d_reduced", ds)
    sd = nnunet_ref.synthetic_state_dict(spec, 11)
    net = _Net(spec).double()
    assert set(net.state_dict()) == set(nnunet.param_shapes(spec))          # the names, and through load_state_dict the shapes
    net.load_state_dict({k: v.double() for k, v in sd.items()})
    x = torch.randn((2, 3, 32, 48), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        a = net(x.double())
    b = nnunet_ref.forward(sd, spec, x, torch.float64)
    assert a.shape == b.shape == (2, 4, 32, 48)
    assert (a - b).abs().max().item() <= 1e-12 * b.abs().max().item()
    # the fp16-storage model moves the result by about fp16's precision, not by nothing and not by a lot
    c = nnunet_ref.forward(sd, spec, x, torch.float64, store=nnunet_ref.fp16_storage)
    rel = (c - b).abs().max().item() / b.abs().max().item()
    assert 1e-5 < rel < 2e-2, rel


# ---- 5. the window's tile is the plans' patch, also under an image that is smaller than it --------------------------------------------------------
def test_predict_mask_pads_a_small_image_to_the_patch(monkeypatch):
    """nnU-Net zero-pads an image smaller than the patch and runs the network on the FULL patch (predict_from_raw_data.py:614); the head must not shrink the
    tile to the image (InstanceNorm statistics and Gaussian weights would change, and a size off the stride grid would be refused by the network)."""
    plans, ds = fixtures()
    spec = nnunet.network_spec(plans, "2d_reduced", ds)          # patch 64 x 64, stride product 8
    seen = []

    def network(x):
        seen.append(tuple(x.shape))
        return torch.stack([x[:, 0], -x[:, 0], x[:, 1] * 0.5, x[:, 2] * 0.25], 1)

    from ldiffusion_amd import segmentor
    monkeypatch.setattr(segmentor, "argmax_mask", lambda logits: logits.argmax(1).to(torch.uint8))   # (the device kernel's host statement: this test runs without a GPU)
    model = nnunet.TrainedModel(network, spec, (0, 1))
    img = torch.zeros((3, 60, 150))
    img[:, 4:55, 10:141] = torch.rand((3, 51, 131), generator=torch.Generator().manual_seed(2)) * 254 + 1   # a 51 x 131 crop: under the patch in one axis, odd in both
    mask = model.predict_mask(img)
    assert mask.shape == (60, 150) and mask.dtype == torch.uint8
    assert seen and all(s == (1, 3, 64, 64) for s in seen)      # every evaluation on a whole patch
    assert len(seen) == 4 * 4                                   # 1 x 4 tiles at step 0.5 over 64 x 131, times the four mirror combinations
    assert not mask[:4].any() and not mask[55:].any() and not mask[:, :10].any() and not mask[:, 141:].any()
    with pytest.raises(ValueError, match="tile_size"):
        model.predict_mask(img, tile_size=(60, 64))
