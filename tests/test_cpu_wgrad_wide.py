"""No GPU: the route names "wide" / "auto-wide", the route decision (autograd.wgrad_entry) against a table written out by hand, the eligibility and plan
statements of the wide direct weight gradient in autograd.py against the library's own (ldiff_op_conv_wgrad_wide_ws_bytes is host code: the library loads
without a device), and the workspace maximum include/ldiff.h states."""
import os
import re

import pytest

from ldiffusion_amd import autograd as ag

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_route_names():
    assert ag.WGRAD_ROUTES[:3] == ("staged", "direct", "auto") and {"wide", "auto-wide"} <= set(ag.WGRAD_ROUTES)
    assert ag.WGRAD_WIDE_MIN_ROWS >= 16384
    start = ag.stated_wgrad_route("none stated")
    with ag.wgrad_route("wide"):
        assert ag.stated_wgrad_route("x") == "wide"
        with ag.wgrad_route("auto-wide"):
            assert ag.stated_wgrad_route("x") == "auto-wide"
            with ag.wgrad_route("staged"):
                assert ag.stated_wgrad_route("x") == "staged"
            assert ag.stated_wgrad_route("x") == "auto-wide"
        assert ag.stated_wgrad_route("x") == "wide"
    assert ag.stated_wgrad_route("none stated") == start
    for bad in ("widest", "auto_wide", ""):
        with pytest.raises(ValueError, match="wgrad route"):
            ag.wgrad_route(bad)
        with pytest.raises(ValueError, match="wgrad route"):
            ag.set_wgrad_route(bad)
    assert ag.stated_wgrad_route("none stated") == start


def test_the_route_keyword_reaches_the_public_interface():
    """`wgrad_route=None` on every layer from LDiffusionModel.train down to TrainableSegNet; LDiffusionModel.train names it (it swallows other keywords)."""
    import inspect

    from ldiffusion_amd import nnunet_train
    from ldiffusion_amd.ldiffusion import LDiffusionModel
    from ldiffusion_amd.segmentor import Segmentor
    for fn in (LDiffusionModel.train, Segmentor.train_tissue_model_nnUNetv2, nnunet_train.Trainer.__init__, nnunet_train.TrainableSegNet.__init__):
        par = inspect.signature(fn).parameters
        assert "wgrad_route" in par and par["wgrad_route"].default is None, fn.__qualname__
    with pytest.raises(ValueError, match="wgrad route"):
        nnunet_train.TrainableSegNet({}, {}, "cpu", wgrad_route="widest")


def test_wide_eligibility_at_the_limits():
    ok = ag.wgrad_wide_eligible   # (k, stride, ups, Cx, Cy, Cout, Cin)
    assert ok(3, 1, 0, 1024, 512, 512, 1024) and ok(3, 2, 0, 8, 8, 1, 1) and ok(1, 1, 0, 512, 2048, 2048, 512) and ok(3, 1, 0, 136, 72, 65, 130)
    assert not ok(3, 1, 0, 1032, 32, 32, 1032) and not ok(3, 1, 0, 32, 520, 520, 32) and not ok(1, 1, 0, 32, 2056, 2056, 32) and ok(1, 1, 0, 32, 520, 520, 32)
    assert not ok(5, 1, 0, 32, 32, 32, 32) and not ok(1, 2, 0, 32, 32, 32, 32) and not ok(3, 3, 0, 32, 32, 32, 32) and not ok(3, 1, 1, 32, 32, 32, 32)
    assert not ok(3, 1, 0, 36, 32, 32, 36) and not ok(3, 1, 0, 32, 36, 36, 32) and not ok(3, 1, 0, 0, 32, 32, 0)
    assert not ok(3, 1, 0, 32, 32, 33, 32) and not ok(3, 1, 0, 32, 32, 32, 33) and not ok(3, 1, 0, 32, 32, 0, 32) and not ok(3, 1, 0, 32, 32, 32, 0)
    # the narrow entry's limits did not move
    assert ag.wgrad_direct_eligible(3, 1, 0, 128, 64, 64, 128) and not ag.wgrad_direct_eligible(3, 1, 0, 136, 64, 64, 136) and not ag.wgrad_direct_eligible(3, 1, 0, 128, 72, 72, 128)


# (k, stride, ups, Cx, Cy, Cout, Cin): one the narrow entry takes, one only the wide entry takes, one neither takes (the conv upsamples its input)
NARROW_LAUNCH, WIDE_LAUNCH, UPS_LAUNCH = (3, 1, 0, 32, 32, 32, 32), (3, 2, 0, 128, 256, 256, 128), (3, 1, 1, 32, 32, 32, 32)
# Written out from the route comment of autograd.py ("which kernels form a conv's weight and bias gradient"), not computed:
# (route, M) -> ((entry of the narrow launch, of the wide launch, of the upsampling launch), slab_bias).  16384 = both *_MIN_ROWS constants.
ROUTE_TABLE = {
    ("staged", 8192): (("staged", "staged", "staged"), False),       # "staged": nothing moves, at any M
    ("staged", 16384): (("staged", "staged", "staged"), False),
    ("direct", 8192): (("narrow", "staged", "staged"), True),        # "direct": the narrow entry wherever eligible, every bias gradient on the slab sum, at any M
    ("direct", 16384): (("narrow", "staged", "staged"), True),
    ("auto", 8192): (("staged", "staged", "staged"), False),         # "auto": "staged" below WGRAD_DIRECT_MIN_ROWS,
    ("auto", 16384): (("narrow", "staged", "staged"), True),         #         "direct" from it on
    ("wide", 8192): (("narrow", "wide", "staged"), True),            # "wide": a direct kernel wherever one takes the shape, the narrow entry first, at any M
    ("wide", 16384): (("narrow", "wide", "staged"), True),
    ("auto-wide", 8192): (("staged", "staged", "staged"), True),     # "auto-wide": every bias gradient on the slab sum whatever M; weights staged below the thresholds,
    ("auto-wide", 16384): (("narrow", "wide", "staged"), True),      #              the narrow entry's launches follow "auto", the wide-only ones go to the wide entry
}


def test_wgrad_entry_against_the_route_comment():
    assert ag.WGRAD_DIRECT_MIN_ROWS == ag.WGRAD_WIDE_MIN_ROWS == 16384, "the table's two M straddle these"
    assert {r for r, _ in ROUTE_TABLE} == set(ag.WGRAD_ROUTES) and len(ROUTE_TABLE) == 2 * len(ag.WGRAD_ROUTES)
    for (route, M), (entries, slab_bias) in ROUTE_TABLE.items():
        for launch, entry in zip((NARROW_LAUNCH, WIDE_LAUNCH, UPS_LAUNCH), entries):
            assert ag.wgrad_entry(route, M, *launch) == (entry, slab_bias), (route, M, launch)
    # a 1 x 1 conv with 2056 output columns: past every direct entry and past the slab column sum's own limit (2048).  slab_bias states what the ROUTE asks
    # for, so it stays True: the launch, not the route decision, tests Cy and falls back to ldiff_op_colsum.
    for route, slab_bias in (("staged", False), ("direct", True), ("wide", True), ("auto-wide", True)):
        assert ag.wgrad_entry(route, 16384, 1, 1, 0, 32, 2056, 2056, 32) == ("staged", slab_bias), route
    # M one below the threshold stays staged
    assert ag.wgrad_entry("auto", 16383, *NARROW_LAUNCH) == ("staged", False) and ag.wgrad_entry("auto-wide", 16383, *WIDE_LAUNCH) == ("staged", True)


CHANNELS = [(136, 32, 3), (32, 72, 3), (128, 128, 3), (64, 136, 3), (256, 128, 3), (512, 256, 3), (1024, 512, 3), (128, 512, 1), (512, 2048, 1), (256, 8, 1), (8, 8, 3),
            (128, 256, 1), (256, 512, 1)]   # (Cx, Cy, k): tests/test_gpu_wgrad_wide.py's, the smallest, and the trainer's transposed convs
MAPS = [(2, 8, 8), (2, 5, 33), (2, 5, 20), (2, 20, 40), (12, 128, 128), (12, 64, 64), (12, 32, 32), (12, 16, 16), (1, 1, 1), (12, 512, 512)]   # (B, Ho, Wo)


def test_plan_equals_the_librarys_and_stays_under_the_stated_maximum(lib):
    hdr = open(os.path.join(ROOT, "include", "ldiff.h")).read()
    cap = int(re.search(r"#define LDIFF_WGRAD_WIDE_MAX_WS_BYTES (\d+)", hdr).group(1))
    assert cap == 1024 * 64 * 32 * 9 * 4
    worst = 0
    for Cx, Cy, k in CHANNELS:
        for B, Ho, Wo in MAPS:
            tiles = ag.wgrad_wide_plan(B, Ho, Wo, Cx, Cy, k, 0)["tiles"]
            for wgs in (0, 1, 3, 8, tiles + 1):
                if wgs > 65535:
                    continue
                plan = ag.wgrad_wide_plan(B, Ho, Wo, Cx, Cy, k, wgs)
                assert plan["ws_bytes"] == lib.ldiff_op_conv_wgrad_wide_ws_bytes(B, Ho, Wo, Cx, Cy, k, wgs) > 0, (Cx, Cy, k, B, Ho, Wo, wgs)
                assert set(plan) == set(ag.wgrad_plan(1, 8, 8, 32, 32, 3, 0))
                assert plan["wgs"] >= 1 and plan["chain"] == -(-plan["tiles"] // plan["wgs"]) * plan["TH"] * 32 and plan["partials"] == plan["wgs"]
                if wgs == 0:
                    assert plan["ws_bytes"] <= cap and plan["wgs"] * plan["slabs"] <= max(1024, plan["slabs"])
                    worst = max(worst, plan["ws_bytes"])
    assert worst == cap, "no test shape reaches the stated maximum: the statement is not tight"
    for args in [(1, 8, 8, 1032, 32, 3, 0), (1, 8, 8, 32, 520, 3, 0), (1, 8, 8, 32, 2056, 1, 0), (1, 8, 8, 32, 32, 5, 0), (1, 8, 8, 32, 32, 3, 65536), (1, 8, 8, 32, 32, 3, -1),
                 (0, 8, 8, 32, 32, 3, 0), (1, 8, 8, 36, 32, 3, 0)]:
        assert lib.ldiff_op_conv_wgrad_wide_ws_bytes(*args) == 0, args
    # every accepted channel count, planned, at a map with more tiles than workgroups
    for k, cymax in ((3, 512), (1, 2048)):
        for Cx in range(8, 1025, 8):
            for Cy in (8, 64, 72, cymax // 2, cymax - 8, cymax):
                plan = ag.wgrad_wide_plan(12, 128, 128, Cx, Cy, k, 0)
                assert plan["ws_bytes"] <= cap and plan["ws_bytes"] == lib.ldiff_op_conv_wgrad_wide_ws_bytes(12, 128, 128, Cx, Cy, k, 0)
