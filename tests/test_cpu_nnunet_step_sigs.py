"""CPU: tests/nnunet_step_sigs.py -- the trainer's layer signatures against a hand-written list, and the float64 reference of the transposed-conv path against
torch's own conv_transpose2d autograd; the two wrong references must lie far outside the bound on the inputs tests/test_gpu_nnunet_backward.py uses."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import nnunet_step_sigs as ns
from ldiffusion_amd import nnunet

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def spec_of(config):
    with open(os.path.join(GOLDEN, "nnunet_plans_2d.json")) as f:
        plans = json.load(f)
    with open(os.path.join(GOLDEN, "nnunet_dataset.json")) as f:
        ds = json.load(f)
    return nnunet.network_spec(plans, config, ds)


def test_signatures_of_2d_reduced_at_2x64x64():
    """Written out by hand from PlainConvUNet(features 32 / 64 / 128 / 256, two convs per stage, strides 1 / 2 / 2 / 2, 3 input channels, 4 classes)."""
    T = (True, True)
    want = [
        (2, 64, 64, 8, 32, 3, 3, 1, 0) + T, (2, 64, 64, 32, 32, 32, 3, 1, 0) + T,            # encoder, 64 x 64
        (2, 64, 64, 32, 64, 32, 3, 2, 0) + T, (2, 32, 32, 64, 64, 64, 3, 1, 0) + T,          # 32 x 32
        (2, 32, 32, 64, 128, 64, 3, 2, 0) + T, (2, 16, 16, 128, 128, 128, 3, 1, 0) + T,      # 16 x 16
        (2, 16, 16, 128, 256, 128, 3, 2, 0) + T, (2, 8, 8, 256, 256, 256, 3, 1, 0) + T,      # 8 x 8
        (1, 1, 128, 256, 512, 256, 1, 1, 0) + T,                                             # transpconvs.0: 2 * 8 * 8 rows, 256 -> 4 * 128
        (2, 16, 16, 256, 128, 256, 3, 1, 0) + T, (2, 16, 16, 128, 128, 128, 3, 1, 0) + T, (2, 16, 16, 128, 4, 128, 1, 1, 0) + T,
        (1, 1, 512, 128, 256, 128, 1, 1, 0) + T,                                             # transpconvs.1
        (2, 32, 32, 128, 64, 128, 3, 1, 0) + T, (2, 32, 32, 64, 64, 64, 3, 1, 0) + T, (2, 32, 32, 64, 4, 64, 1, 1, 0) + T,
        (1, 1, 2048, 64, 128, 64, 1, 1, 0) + T,                                              # transpconvs.2
        (2, 64, 64, 64, 32, 64, 3, 1, 0) + T, (2, 64, 64, 32, 32, 32, 3, 1, 0) + T, (2, 64, 64, 32, 4, 32, 1, 1, 0) + T,
    ]
    spec = spec_of("2d_reduced")
    assert ns.conv_signatures(spec, 2, 64, 64) == want
    assert ns.norm_signatures(spec, 2, 64, 64) == [(2, 32, 64, 64)] * 2 + [(2, 64, 32, 32)] * 2 + [(2, 128, 16, 16)] * 2 + [(2, 256, 8, 8)] * 2 + \
        [(2, 128, 16, 16)] * 2 + [(2, 64, 32, 32)] * 2 + [(2, 32, 64, 64)] * 2
    assert ns.transpconv_shapes(spec) == [(256, 128), (128, 64), (64, 32)]


def test_counts_of_2d_at_2x128x128():
    """Seven stages 32 ... 512: 14 encoder convs, 6 transposed convs, 12 decoder convs, 6 heads; each decoder stage's second conv repeats the encoder's second
    conv of that level, so 32 of the 38 are distinct.  The 512-wide stages run at 8 x 8, 4 x 4 and 2 x 2."""
    spec = spec_of("2d")
    sigs = ns.conv_signatures(spec, 2, 128, 128)
    assert len(sigs) == 38 and len(set(sigs)) == 32
    assert sum(1 for s in sigs if s[6] == 3) == 26 and sum(1 for s in sigs if s[6] == 3 and s[7] == 2) == 6
    assert sum(1 for s in sigs if s[0] == 1 and s[1] == 1) == 6 and sum(1 for s in sigs if s[4] == 4) == 6
    assert (2, 4, 4, 512, 512, 512, 3, 2, 0, True, True) in sigs and (2, 2, 2, 512, 512, 512, 3, 1, 0, True, True) in sigs
    assert (2, 4, 4, 1024, 512, 1024, 3, 1, 0, True, True) in sigs and (1, 1, 8, 512, 2048, 512, 1, 1, 0, True, True) in sigs
    assert max(s[0] * s[1] * s[2] for s in sigs) == 2 * 128 * 128
    norms = ns.norm_signatures(spec, 2, 128, 128)
    assert len(norms) == 26 and (2, 512, 2, 2) in norms and (2, 512, 8, 8) in norms
    assert ns.transpconv_shapes(spec) == [(512, 512), (512, 512), (512, 256), (256, 128), (128, 64), (64, 32)]
    # at the real configuration the same list, twelve 512 x 512 patches
    real = ns.conv_signatures(spec, 12, 512, 512)
    assert len(real) == 38 and max(s[0] * s[1] * s[2] for s in real) == 12 * 512 * 512


TCONV_CASES = [(ci, co) + m for ci, co in ((512, 512), (512, 256), (256, 128), (128, 64), (64, 32)) for m in ns.TCONV_MAPS]


@pytest.mark.parametrize("cin,cout,B,h,w", TCONV_CASES)
def test_tconv_reference_against_torch_and_the_wrong_references_are_far(cin, cout, B, h, w):
    x, W, b, dy = (t.double() for t in ns.tconv_case(cin, cout, B, h, w))
    ref = ns.tconv_reference(x, W, b, dy)
    xa, Wa, ba = (t.clone().requires_grad_(True) for t in (x, W, b))
    y = F.conv_transpose2d(xa, Wa, ba, stride=2)
    y.backward(dy)
    for name, got in (("y", y.detach()), ("dx", xa.grad), ("dw", Wa.grad), ("db", ba.grad)):
        assert got.shape == ref[name].shape
        assert (got - ref[name]).abs().max() <= 1e-12 * max(1.0, ref[name].abs().max().item()), name
    # the wrong references lie far outside the bounds: the worst element by more than 100 bounds
    for name, wrong, tol in (("y", ref["y_swapped"], ns.f16_bound(ref["y_swapped"], ref["ey"])), ("dx", ref["dx_swapped"], ns.f16_bound(ref["dx_swapped"], ref["edx"])),
                             ("dw", ref["dw_swapped"], ref["edw"]), ("db", ref["db_one_subpixel"], ref["edb"])):
        ratio = ((ref[name] - wrong).abs() / tol).max().item()
        assert ratio > 100.0, f"{name}: the wrong reference is only {ratio:.1f} bounds away"
    # the plans of the direct route enter as chain + partials + 2
    planned = ns.tconv_reference(x, W, b, dy, dw_plan=dict(chain=64, partials=3), db_plan=dict(chain=10, partials=2))
    assert planned["Kdw"] == 69 and torch.allclose(planned["edw"] * ns.gamma(ref["Mpad"]), ref["edw"] * (69 * ns.U), rtol=1e-12, atol=0)
    assert torch.allclose(planned["edb"] * (ns.gamma(ref["M"]) + 3 * ns.U * (1 + ns.gamma(ref["M"]))), ref["edb"] * (14 * ns.U + 3 * ns.U * (1 + 14 * ns.U)), rtol=1e-12, atol=0)
