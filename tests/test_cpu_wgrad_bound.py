"""CPU: the reference and the bound tests/test_gpu_wgrad_direct.py holds ldiff_op_conv_wgrad and ldiff_op_colsum_slabs to (tests/wgrad_bound.py) -- the reference is
torch's conv2d backward, the bound accepts the kernel's order of operations carried out in fp32 and rejects three mutations of it, and the route setting of
ldiffusion_amd.autograd behaves as documented."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wgrad_bound as wb
from ldiffusion_amd import autograd as ag


@pytest.mark.parametrize("k,stride,H,W", [(3, 1, 9, 11), (3, 2, 10, 10), (3, 2, 9, 11), (1, 1, 5, 7)])
def test_reference_is_conv2d_backward(k, stride, H, W):
    """wgrad_reference against torch.autograd of F.conv2d in float64 (padding k // 2), with pad channels in x and dy that must not take part."""
    Cx, Cin, Cy, Cout, B = 8, 5, 16, 11, 2
    x, dy = wb.random_case(B, H, W, Cx, Cy, k, stride, 3)
    w = torch.zeros((Cout, Cin, k, k), dtype=torch.float64, requires_grad=True)
    y = F.conv2d(torch.from_numpy(x[..., :Cin].astype(np.float64)).permute(0, 3, 1, 2), w, None, stride, k // 2)
    assert tuple(y.shape[2:]) == dy.shape[1:3]
    y.backward(torch.from_numpy(dy[..., :Cout].astype(np.float64)).permute(0, 3, 1, 2))
    dw, mag = wb.wgrad_reference(x, dy, Cout, Cin, k, stride)
    assert dw.shape == (Cout, Cin, k, k)
    np.testing.assert_allclose(dw, w.grad.numpy(), rtol=0, atol=1e-12 * mag.max())
    assert (mag >= np.abs(dw) - 1e-12).all()


@pytest.mark.parametrize("B,H,W,C", wb.BOUND_CASES)
def test_bound_accepts_fp32_and_rejects_mutations(B, H, W, C):
    """On the GPU test's own shapes and workgroup count: the kernel's order of operations in fp32 lies inside the bound, which lies well under one fp16
    rounding of the result's magnitude sum; fp16 partials, a tap shifted by one pixel and edge clamping lie outside it."""
    k, stride = 3, 1
    x, dy = wb.random_case(B, H, W, C, C, k, stride, 10 + C + H)
    plan = wb.plan_of(B, H, W, C, C, k, wb.BOUND_WGS)
    assert plan["wgs"] == plan["partials"] == wb.BOUND_WGS and plan["chain"] == -(-plan["tiles"] // 8) * plan["TH"] * 32
    want, mag = wb.wgrad_reference(x, dy, C, C, k, stride)
    tol = wb.bound(mag, plan)
    assert (plan["chain"] + plan["partials"] + 2) * wb.U < 0.25 * 2.0 ** -11, "the bound must lie well under one fp16 rounding"
    honest = wb.wgrad_emulate(x, dy, C, C, k, stride, plan)
    assert (np.abs(honest - want) <= tol).all()
    half = wb.wgrad_emulate(x, dy, C, C, k, stride, plan, partial=np.float16)
    assert (np.abs(half - want) > tol).mean() > 0.2, "the bound accepts partials rounded to fp16"
    shifted = wb.wgrad_emulate(x, dy, C, C, k, stride, plan, shift_tap=(5, 1))
    assert (np.abs(shifted - want)[:, :, 1, 2] > tol[:, :, 1, 2]).mean() > 0.9, "the bound accepts a tap shifted by one pixel"
    assert (np.abs(shifted - want)[:, :, 0, :] <= tol[:, :, 0, :]).all()
    clamped = wb.wgrad_emulate(x, dy, C, C, k, stride, plan, clamp=True)
    edge = np.abs(clamped - want) > tol
    assert edge[:, :, 0, :].mean() > 0.5 and edge[:, :, :, 2].mean() > 0.5, "the bound accepts edge clamping for zero padding"
    assert not edge[:, :, 1, 1].any(), "the centre tap reads no padding"


def test_colsum_bound_accepts_fp32_and_rejects_fp16_partials():
    M, N = 4800, 32
    dy = wb.random_rows(M, N + 8, 5)
    plan = ag.colsum_slabs_plan(M, N)
    assert plan["slabs"] * plan["rows"] >= M > (plan["slabs"] - 1) * plan["rows"] and plan["chain"] == -(-plan["rows"] // plan["row_lanes"]) + plan["row_lanes"]
    want, mag = wb.colsum_reference(dy, N)
    tol = wb.bound(mag, plan)
    assert (np.abs(wb.colsum_emulate(dy, N, plan) - want) <= tol).all()
    assert (np.abs(wb.colsum_emulate(dy, N, plan, partial=np.float16) - want) > tol).mean() > 0.5, "the bound accepts slab sums rounded to fp16"


def test_integer_reference_is_exact_in_fp32():
    """The exact-integer GPU cases rest on 9 M < 2^24: every partial sum of products of integers in [-3, 3] is then an integer fp32 holds."""
    x, dy = wb.int_case(3, 20, 40, 32, 32, 3, 1, 1)
    want, mag = wb.wgrad_reference(x, dy, 32, 32, 3, 1, dtype=np.int64)
    assert 9 * dy.shape[0] * dy.shape[1] * dy.shape[2] < 2 ** 24 and mag.max() < 2 ** 24
    plan = wb.plan_of(3, 20, 40, 32, 32, 3, 3)
    assert np.array_equal(wb.wgrad_emulate(x, dy, 32, 32, 3, 1, plan), want.astype(np.float64))


def test_route_setting():
    assert ag._WGRAD_ROUTE == "staged" and ag.stated_wgrad_route("auto") == "auto", "the module default is the staged route, not stated by anyone"
    assert ag.WGRAD_DIRECT_MIN_ROWS >= 16384
    with ag.wgrad_route("direct"):
        assert ag._WGRAD_ROUTE == "direct" and ag.stated_wgrad_route("auto") == "direct"
        with ag.wgrad_route("staged"):
            assert ag.stated_wgrad_route("auto") == "staged"
        assert ag._WGRAD_ROUTE == "direct"
    assert ag._WGRAD_ROUTE == "staged" and ag.stated_wgrad_route("auto") == "auto"
    prev = ag.set_wgrad_route("auto")
    try:
        assert prev == "staged" and ag._WGRAD_ROUTE == "auto"
    finally:
        ag._WGRAD_ROUTE, ag._WGRAD_ROUTE_STATED = "staged", False
    with pytest.raises(ValueError, match="route"):
        ag.wgrad_route("fused")
    with pytest.raises(ValueError, match="route"):
        ag.set_wgrad_route("fused")
    # the shapes of the planner's network at 512^2 and 256^2 are eligible, the wide stages and upsampling convs are not
    for Cx, Cy, k, s in [(8, 32, 3, 1), (32, 32, 3, 1), (64, 32, 3, 1), (32, 64, 3, 2), (64, 64, 3, 1), (128, 64, 3, 1), (32, 8, 1, 1), (64, 128, 1, 1)]:
        assert ag.wgrad_direct_eligible(k, s, 0, Cx, Cy, Cy, Cx)
    for k, s, ups, Cx, Cy in [(3, 1, 0, 64, 128), (3, 1, 0, 136, 64), (1, 2, 0, 32, 32), (3, 1, 1, 32, 32), (5, 1, 0, 32, 32), (3, 1, 0, 12, 32)]:
        assert not ag.wgrad_direct_eligible(k, s, ups, Cx, Cy, Cy, Cx)
