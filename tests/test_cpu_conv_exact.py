"""The inputs of the bit-exact conv / GEMM cases (tests/conv_exact.py) on the CPU: the builders' exactness conditions, the emulator against hand-made
values of epilogue.h's epi_value / epi_store8, and that the inputs DISCRIMINATE -- each wrong rule a kernel could have changes the expected bits in at
least 1 % of the elements it can affect.  The cap is a condition on the inputs: a case that misses it is changed, not the cap."""
import types

import numpy as np
import pytest

import conv_exact as ce


def test_every_kernel_variant_is_pinned_by_a_case():
    """Every name of KERNEL_VARIANTS under the diffusion path's launchers has a regime-E case (or a stated exclusion), and the cases name nothing else: a
    variant added to the table without an exact case fails here."""
    from kernel_routing import KERNEL_VARIANTS as kv
    want = {n for g in ce.EXACT_LAUNCHERS for n in kv[g]}
    have = {c["kernel"] for c in ce.CASES.values() if "E" in c.get("regimes", "E")}
    missing = want - have - set(ce.EXCLUDED)
    assert not missing, f"kernel variants without an exact case: {sorted(missing)}"
    assert not have - want, f"cases name kernels KERNEL_VARIANTS does not list: {sorted(have - want)}"
    assert not (set(ce.EXCLUDED) & have)
    for n in ce.EXCLUDED:
        assert any(n in names for names in kv.values()), f"EXCLUDED names {n}, which KERNEL_VARIANTS does not list"


def test_the_table_contains_the_required_edges():
    cs = [ce.case(n) for n in ce.CASES]
    fam = lambda c: c.kernel.split(",")[0]
    assert any(c.H == 1 and c.W == 1 for c in cs)
    assert any(c.stride == 2 and not c.asym for c in cs) and any(c.stride == 2 and c.asym for c in cs)
    assert any(c.C2 and c.C2 != c.C1 for c in cs) and any(c.pitch for c in cs) and any(c.opsplit for c in cs)
    assert any(c.ups and c.c3d_ups for c in cs) and any(c.ups and (c.H % 2 or c.W % 2) and fam(c) in ("conv3x3<8x8", "conv3x3<8x16") for c in cs)
    assert any(c.sc for c in cs) and any(c.short_runs and "16x16d" in c.kernel for c in cs) and any(c.short_runs and fam(c) == "conv3x3<16x16" for c in cs)
    assert {16} <= {c.splitk for c in cs} and any(c.splitk and (c.K // 64) % c.splitk for c in cs)
    assert {"f32", "f16", "split"} <= {c.out for c in cs} and {"plain", "split"} <= {c.res for c in cs if c.res} and any(c.temb for c in cs)
    for f, tile in (("conv3x3<8x8", (8, 8)), ("conv3x3<8x16", (8, 16)), ("conv3x3<16x16", (16, 16))):   # ragged on both borders for each tile family
        assert any(fam(c) == f and (c.H << 0) % tile[0] and c.W % tile[1] for c in cs), f
    for c in cs:
        if "R" in c.regimes:
            assert c.epi in ("halo", "gemm", "igemm", "reduce") and c.r_out in ("f32", "split")
            assert c.kernel.startswith(("conv3x3<8x8", "conv3x3<8x16", "gemm_dma", "gemm_df", "igemm")) and ",n" not in c.kernel
            assert (c.epi == "reduce") == (c.splitk > 1)
    assert {0, 4} <= {c.r_shift for c in cs if "R" in c.regimes}


def test_emulator_on_hand_made_values():
    """epi_value: v = (sum + addends) * 2^-k, + res hi, + res lo, each an fp32 operation; epi_store8: fp32 | rne16 | hi, lo = rne16(v - hi)."""
    c = types.SimpleNamespace(kernel="igemm<64,64,fast>", epi="igemm", out_shift=4, out="split", stats=False, n_real=0)
    o = types.SimpleNamespace(acc=np.array([[[[4097.0, 100000.0, -3.0]]]]), bias=np.array([0.5, 1.0, 0.25], np.float32), sc_bias=None,
                              temb=np.array([[0.5, 2.0, 0.0]], np.float32), res_hi=np.array([[[[1.0, -2.0, 0.5]]]], np.float16),
                              res_lo=np.array([[[[2.0 ** -12, 0.0, 0.0]]]], np.float16))
    v = ce.value(c, o, "E")
    want = np.array([(4097 + 1.0) / 16 + 1 + 2.0 ** -12, 100003.0 / 16 - 2, -2.75 / 16 + 0.5])
    assert np.array_equal(v.ravel(), want)
    e = ce.expected(c, o, "E")
    hi = want.astype(np.float16)
    assert hi[0] == 257.25 and np.array_equal(e["hi"].ravel(), hi)                     # 257.125 + 2^-12: the tie of spacing 0.25 is broken by the residual's lo half
    assert np.array_equal(e["lo"].ravel(), (want - hi.astype(np.float64)).astype(np.float16))
    assert e["lo"].ravel()[0] == np.float16(-0.125 + 2.0 ** -12) and hi[1] == np.float16(6248.0) and e["lo"].ravel()[1] == np.float16(0.1875)
    # regime R: float32 in the stated order.  2^24 + 1 is not an fp32: (acc + bias) + temb and acc + (bias + temb) differ
    c.out_shift, c.out = 0, "f32"
    o.acc = np.array([[[[2.0 ** 24]]]]); o.bias = np.array([1.0], np.float32); o.temb = np.array([[1.0]], np.float32); o.res_hi = o.res_lo = None
    assert ce.value(c, o, "R").ravel()[0] == np.float32(2.0 ** 24)                     # igemm: (2^24 + 1) -> 2^24 (ties to even), + 1 -> 2^24
    c.epi = "halo"
    assert ce.value(c, o, "R").ravel()[0] == np.float32(2.0 ** 24 + 2)                 # halo: 2^24 + (1 + 1)
    # round toward zero: 2049 -> 2048 either way, 2051 -> 2052 (nearest) but 2050 (toward zero); negative values mirror
    assert list(ce.rtz16(np.array([2049.0, 2051.0, -2051.0, 3.0]))) == [2048.0, 2050.0, -2050.0, 3.0]
    assert list(ce.rne16(np.array([2049.0, 2051.0, -2051.0]))) == [2048.0, 2052.0, -2052.0]


def _changed(a, b):
    return float((np.asarray(a).view(np.uint16 if a.dtype == np.float16 else np.uint32 if a.dtype == np.float32 else np.uint64)
                  != np.asarray(b).view(np.uint16 if b.dtype == np.float16 else np.uint32 if b.dtype == np.float32 else np.uint64)).mean())


def _stored(e):
    return [e[k] for k in ("f32", "hi", "lo") if k in e]


@pytest.mark.parametrize("name", list(ce.CASES))
def test_case_is_exact_and_discriminates(name):
    c, o = ce.build(name, "E")
    ce.check_exact_conditions(c, o)
    good = ce.expected(c, o, "E")
    real = slice(0, c.n_real or c.N)
    shown = {}
    if c.out != "f32" and not c.stats:
        shown["rtz"] = _changed(good["hi"][..., real], ce.expected(c, o, "E", "rtz")["hi"][..., real])
    if c.res and c.out_shift:
        shown["res_before_shift"] = _changed(_stored(good)[0], _stored(ce.expected(c, o, "E", "res_before_shift"))[0])
    if c.res and c.out != "f32" and not c.stats and not c.kernel.startswith("conv3x3<16x16d"):
        shown["round_before_res"] = max(_changed(g, b) for g, b in zip(_stored(good), _stored(ce.expected(c, o, "E", "round_before_res"))))
    if c.kernel.startswith("conv3x3<16x16d") and c.res:      # the declared exception must itself be visible: one rounding gives other bits
        one = ce.rne16(ce.value(c, o, "E", "res_before_shift"))
        shown["two_roundings_of_the_dataflow_residual"] = _changed(good["hi"], one)
    if (c.out == "split" and not c.stats) or c.res == "split":
        shown["lo_dropped"] = max(_changed(g, b) for g, b in zip(_stored(good), _stored(ce.expected(c, o, "E", "lo_dropped"))))
    if c.opsplit:   # the operand's lo half dropped: the contraction over hi alone
        import torch
        import torch.nn.functional as F
        t, b, l, r = c.pads
        hp = np.pad(o.x_hi.repeat(2, 1).repeat(2, 2) if c.ups else o.x_hi, ((0, 0), (t, b), (l, r), (0, 0)))
        acc = F.conv2d(torch.from_numpy(hp).permute(0, 3, 1, 2), torch.from_numpy(o.w).permute(0, 3, 1, 2), stride=c.stride).permute(0, 2, 3, 1).numpy()
        shown["operand_lo_dropped"] = _changed(_stored(good)[0], _stored(ce.expected(c, o, "E", acc=acc))[0])
    acc, n0 = ce.acc_with_one_weight_zeroed(c, o)
    shown["weight_zeroed"] = _changed(_stored(good)[0][..., n0], _stored(ce.expected(c, o, "E", acc=acc))[0][..., n0])
    nb = ce.acc_with_neighbour_halo(c, o)
    if nb is not None:
        acc, (oy, ox) = nb
        shown["halo_from_neighbour"] = _changed(_stored(good)[0][0, oy, ox, real], _stored(ce.expected(c, o, "E", acc=acc))[0][0, oy, ox, real])
    if c.stats:
        bad = ce.expected(c, o, "E", "stats_extra_pixel")["stats"]
        shown["stats_extra_pixel"] = float((bad != good["stats"]).any(-1).mean())
    if "R" in c.regimes:
        cr, orr = ce.build(name, "R")
        gr = ce.expected(cr, orr, "R")
        if cr.temb and cr.epi != "gemm":
            shown["R_addend_order_swapped"] = max(_changed(g, b) for g, b in zip(_stored(gr), _stored(ce.expected(cr, orr, "R", "addend_order_swapped"))))
        if cr.res and cr.out_shift:
            shown["R_res_before_shift"] = max(_changed(g, b) for g, b in zip(_stored(gr), _stored(ce.expected(cr, orr, "R", "res_before_shift"))))
        assert all(np.isfinite(s.astype(np.float64)).all() for s in _stored(gr))
    print(f"[conv-exact] {name}: {c.kernel}, {ce.element_count(c)} elements, weights in [-{o.aw}, {o.aw}]; " + ", ".join(f"{k} {v:.3f}" for k, v in shown.items()))
    weak = {k: v for k, v in shown.items() if v < 0.01}
    assert not weak, f"{name}: the inputs do not show these wrong rules in 1 % of the elements they can affect: {weak}"
