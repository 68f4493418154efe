"""-m "not gpu": the bounds of tests/groupnorm_bound.py, judged on the CPU where the verdicts are known.  Every bound must accept the fp32
emulation of the kernel it is for and reject every wrong reference of the case (tests/test_gpu_groupnorm.py applies the same bounds to the kernels)."""
import pytest
import torch

import groupnorm_bound as gb


@pytest.mark.parametrize("name", list(gb.STATS_CASES))
def test_stats_bound(name):
    """Section 1: the case's shape takes the form it names (launch_gn_stats's predicate); the emulation of that form's summation order is within
    the bound, and at most a quarter of C_STATS by the measure C_STATS was taken from; the wrong references are rejected."""
    case = gb.STATS_CASES[name]
    assert gb.expected_form(case) == case.form
    inp = gb.make_stats_input(case, 7)
    ref = gb.stats_reference(inp["v"], case.groups, case.eps, inp["gamma"], inp["beta"])
    sc, sh = gb.stats_emulation(inp, case)
    r, rc = gb.stats_ratio(sc, sh, ref), gb.stats_c_ratio(sc, sh, ref)
    print(f"[gn-bound] {name}: emulation at {r:.3f} of the bound, error / (u amp) = {rc:.3f}")
    assert r <= 1.0, f"{name}: the bound rejects the emulation ({r:.3f})"
    assert 4 * rc <= gb.C_STATS
    wrong = gb.stats_wrong_references(inp, case)
    assert len(wrong) == 1 + (case.HW > 1) + (case.special in ("const", "vareps"))
    for what, w in wrong:
        assert gb.stats_ratio(sc, sh, w) > 1.0, f"{name}: the bound accepts the wrong reference '{what}'"
        assert gb.stats_ratio(ref.scale, ref.shift, w) > 1.0, f"{name}: the bound accepts the wrong reference '{what}' for the exact result"


def test_c_stats_is_four_times_the_recorded_worst():
    assert gb.C_STATS >= 2.0 and 4 * gb.C_STATS_WORST_EMULATION <= gb.C_STATS <= 4 * gb.C_STATS_WORST_EMULATION + 0.5


def test_stats_cases_cover_both_forms_and_every_option():
    cases = gb.STATS_CASES.values()
    for form in (gb.ONE, gb.TWO):
        mine = [c for c in cases if c.form == form]
        assert any(c.split for c in mine) and any(c.pitch for c in mine) and any(c.eps == 1e-6 for c in mine) and any(c.affine for c in mine)
        assert {c.ratio for c in mine} >= {0.2, 8.0} and {c.special for c in mine} >= {"const", "vareps"}
    assert gb.gn_chunks(33000) == 516 and gb.gn_chunks(2048) == 64     # pix doubled to 64 / 32 pixels per chunk


@pytest.mark.parametrize("L_b,HW", [(32, 1024), (128, 4096)])
def test_fused_bounds(L_b, HW):
    """Section 2 on emulated row-block partials (sequential fp32 chains of L_b values) of an output with its mean at 8 standard deviations: both levels
    accept them and reject one row block's contribution removed; the finalize level needs no larger c than section 1's."""
    g = torch.Generator().manual_seed(L_b)
    B, N = 2, 64
    y = (8.0 + 0.5 * torch.randn((1, 1, N), generator=g) + torch.randn((B, HW, N), generator=g)).to(torch.float16)
    st = gb.emulate_blocks(y, L_b)
    rs, rq = gb.sums_ratio(st, y, L_b)
    assert rs <= 1.0 and rq <= 1.0
    ones, zeros = torch.ones(N), torch.zeros(N)
    ref = gb.stats_reference(y.double(), 32, 1e-5, ones, zeros)

    def fin(s):
        t = s.double().sum(2)                                     # [B, N, 2]
        return gb.finalize_emulation(t[..., 0].reshape(B, 32, -1).sum(2), t[..., 1].reshape(B, 32, -1).sum(2), float(HW * N // 32), 1e-5, ones, zeros)

    sc, sh = fin(st)
    r2, rc = gb.stats_ratio(sc, sh, ref), gb.stats_c_ratio(sc, sh, ref)
    print(f"[gn-bound] blocks of {L_b}: sums at {rs:.4f} / {rq:.4f}, scale / shift at {r2:.3f} of the bound, error / (u amp) = {rc:.3f}")
    assert r2 <= 1.0 and 4 * rc <= gb.C_STATS
    cut = st.clone()
    cut[0, :, -1, :] = 0.0
    ws, wq = gb.sums_ratio(cut, y, L_b)
    assert ws > 1.0 and wq > 1.0 and gb.stats_ratio(*fin(cut), ref) > 1.0


def test_fused_bound_rejects_eps_doubled_where_var_is_eps():
    g = torch.Generator().manual_seed(3)
    y = (0.025 + 3e-3 * torch.randn((2, 256, 64), generator=g)).to(torch.float16)
    ones, zeros = torch.ones(64), torch.zeros(64)
    ref = gb.stats_reference(y.double(), 32, 1e-5, ones, zeros)
    assert (ref.var <= 10 * ref.eps).all()
    t = gb.emulate_blocks(y, 32).double().sum(2)
    sc, sh = gb.finalize_emulation(t[..., 0].reshape(2, 32, -1).sum(2), t[..., 1].reshape(2, 32, -1).sum(2), 256.0 * 2, 1e-5, ones, zeros)
    assert gb.stats_ratio(sc, sh, ref) <= 1.0
    assert gb.stats_ratio(sc, sh, gb.stats_reference(y.double(), 32, 2e-5, ones, zeros)) > 1.0


def _fold_verdicts(case, inp, what):
    x, W, s, t = inp["x"], inp["W"][:case.N], inp["s"], inp["t"]
    bias = inp["bias"][:case.N] if inp["bias"] is not None else None
    ref = gb.fold_reference(x, W, s, t, bias)
    tol = gb.fold_tol(x, W, s, t, bias, ref)
    yf, yu = gb.folded_emulation(x, W, s, t, bias), gb.unfolded_emulation(x, W, s, t, bias)
    rf, ru = gb.ratio(yf, ref, tol), gb.ratio(yu, ref, gb.unfolded_tol(x, W, s, t, bias, ref))
    print(f"[gn-bound] fold {what}: folded emulation at {rf:.3f} of its bound (max error / max|ref| {gb.rel_err(yf, ref):.2e}), "
          f"unfolded at {ru:.3f} of its own ({gb.rel_err(yu, ref):.2e})")
    assert rf <= 1.0, f"{what}: the fold's bound rejects the emulation of the fold ({rf:.3f})"
    assert ru <= 1.0, f"{what}: the unfolded bound rejects the emulation of the prologue route ({ru:.3f})"
    wrong = gb.fold_wrong_references(x, W, s, t, bias)
    assert len(wrong) == (3 if case.B > 1 else 2)
    for name, w in wrong:
        assert gb.ratio(yf, w, tol) > 1.0, f"{what}: the bound accepts the wrong reference '{name}'"
        assert gb.ratio(yu, w, gb.unfolded_tol(x, W, s, t, bias, ref)) > 1.0, f"{what}: the unfolded bound accepts the wrong reference '{name}'"


@pytest.mark.parametrize("name", list(gb.FOLD_CASES))
def test_fold_bound(name):
    case = gb.FOLD_CASES[name]
    assert (case.HW % 64 == 0) == case.folds and case.C % 64 == 0 and case.N % 4 == 0      # gemm_dma_eligible with per-image weights
    _fold_verdicts(case, gb.make_fold_input(case, 3), name)


@pytest.mark.parametrize("regime", list(gb.FOLD_REGIMES))
def test_fold_bound_operand_regimes(regime):
    case = gb.FOLD_CASES["vae_qkv_smallest_map"]
    _fold_verdicts(case, gb.make_fold_input(case, 3, *gb.FOLD_REGIMES[regime]), regime)


def test_folded_bias_chain_length():
    """gamma(K / 64 + 6) in fold_tol: lane l of 64 adds 8 products per trip of the channel loop (c = 8 l + 512 trip), so K / 64 terms at K % 512 == 0
    and at most 8 ceil(K / 512) otherwise -- 8 at K = 320 (K / 64 = 5), 24 at K = 1280 (K / 64 = 20): the emulation's chain must not be longer than
    K / 64 rounded up to whole trips, which the bound's slack over the true error (>= 7 x in every case above) absorbs."""
    for K in (320, 512, 1280):
        trips = (K + 511) // 512
        assert 8 * trips <= K / 64 + 6 + 2
