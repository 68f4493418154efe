"""-m "not gpu": the bounds of tests/transformer_bound.py, judged on the CPU where the verdicts are known.  Every bound must accept the fp32
emulation of the kernel it is for, on every case tests/test_gpu_transformer_block.py runs, and every wrong reference must be rejected by a named
case.  Each test prints the emulation's worst share of the bound (and of the derived part of it: transformer_bound.margin) per case.

Which case kills which wrong reference (the rows of that family in every launch that has them; asserted below and again on the kernels):

    wrong reference                          rejected by                                                   accepted by (and said so beside the case)
    variance / (C - 1)                       benign rows of every LayerNorm launch (C = 8 ... 2560), of     ratio-1000 rows at C >= 640; constant / zero rows
                                             c320, c640, c1280 in particular; every LN+GEMM case
    eps = 0 | 1e-6 | 1e-5 | 1e-3 (not own)   variance-near-eps rows of every launch that has them           benign rows (eps 0, 1e-6), ratio-1000 rows
    one-pass variance in fp32                ratio-1000 rows (split launches: c64 ... c2560_split_row1)     everything with |mean| / std <= 30 at C >= 2056
    statistics without the last trip         benign rows of c520 ... c2560 (C > 512)                        zero rows
    statistics without the lo half           benign rows of the split launches                              constant / zero / outlier rows
    gamma / beta of the next chunk           benign rows of every launch with C > 8                         -
    mean over the pitch                      benign rows of c320_pitched_eps6 (the 3- and 5-row pitched     zero rows
                                             launches: their variance-near-eps and outlier rows)
    tanh-form GELU                           the exhaustive gate sweep (h = 1, -1, 1/3, 100, 6e4), every    h = 2^-14 (the product is below fp16's subnormal step)
                                             gelu-form epilogue case
    quick_gelu in place of gelu              the sweep, every gelu-form epilogue case                       -
    gelu in place of quick_gelu              gemm_dma_act_quick_gelu and its split-output form             -
    value and gate halves swapped            the sweep, gemm_dma_geglu, gemm_df_geglu, lngemm_geglu         -
    erf with a5 changed in its sixth digit   gemm_dma_act_gelu_split_out (3.7 x the bound) ONLY             every fp16 output: its rounding is 50 x the change
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import transformer_bound as tb


def _family_verdicts(got, inp, wrong, tol):
    return {name: {f for f, v in tb.by_family(tb.row_ratio(got, w, tol), inp["fam"]).items() if v > 1.0} for name, w in wrong}


def assert_ln_verdicts(got, inp, case, wrong, tol, what):
    """Every wrong reference is rejected by the rows of its family (transformer_bound.KILLED_BY) where the launch has them, else by some row."""
    verdicts = _family_verdicts(got, inp, wrong, tol)
    for name, killers in verdicts.items():
        fam = tb.KILLED_BY[name]
        if fam in inp["fam"]:
            assert fam in killers, f"{what}: the {fam} rows accept the wrong reference '{name}'"
    return verdicts


@pytest.mark.parametrize("name", list(tb.LN_CASES))
def test_layernorm_bound(name):
    case = tb.LN_CASES[name]
    inp = tb.make_ln_input(case, 7)
    ref = tb.ln_reference(inp["x"], inp["gamma"], inp["beta"], case.eps)
    tol = tb.ln_tol(ref, case.C)
    emu = tb.emulate_layernorm(inp, case.eps).to(torch.float16)
    worst = tb.by_family(tb.row_ratio(emu, ref.a, tol), inp["fam"])
    print(f"[tf-bound] layernorm {name}: emulation at {max(worst.values()):.3f} of the bound, {tb.margin(emu, ref.a, tol):.3f} of its derived part; "
          + ", ".join(f"{f} {v:.3f}" for f, v in worst.items()))
    assert max(worst.values()) <= 1.0, f"{name}: the bound rejects the emulation {worst}"
    for i, f in enumerate(inp["fam"]):
        if f in ("const", "zero"):
            assert torch.equal(emu[i], inp["beta"].to(torch.float16)), f"{name}: row {i} ({f}) is not f16(beta)"
    verdicts = assert_ln_verdicts(emu, inp, case, tb.ln_wrong_references(inp, case), tol, name)
    print(f"[tf-bound] layernorm {name}: " + "; ".join(f"'{w}' rejected by {sorted(k) or 'NO ROW'}" for w, k in verdicts.items()))
    for w, fam in tb.ACCEPTED_AT_HIGH_RATIO.items():          # what a ratio-1000 row accepts, a low-ratio family of the same launch rejects
        if w in verdicts and "ratio1000" in inp["fam"] and "ratio1000" not in verdicts[w] and fam in inp["fam"]:
            assert fam in verdicts[w]


def test_every_wrong_layernorm_is_rejected_by_a_named_case():
    """The conditions: the unbiased variance at C = 320, 640 and 1280, every wrong eps by the variance-near-eps rows, the one-pass variance by the
    |mean| / std = 1000 rows, and none of the wrong references left unrejected."""
    killed = {}
    for name, case in tb.LN_CASES.items():
        inp = tb.make_ln_input(case, 7)
        ref = tb.ln_reference(inp["x"], inp["gamma"], inp["beta"], case.eps)
        emu = tb.emulate_layernorm(inp, case.eps).to(torch.float16)
        for w, fams in _family_verdicts(emu, inp, tb.ln_wrong_references(inp, case), tb.ln_tol(ref, case.C)).items():
            for f in fams:
                killed.setdefault(w, set()).add((name, f))
    for w, by in killed.items():
        print(f"[tf-bound] '{w}' is rejected by {len(by)} (case, family) pairs, e.g. {sorted(by)[:3]}")
    assert set(killed) == set(tb.KILLED_BY) and all(killed.values())
    for c in ("c320", "c640", "c1280"):
        assert (c, "benign") in killed["variance / (C - 1)"]
    for e in ("eps = 0", "eps = 1e-06", "eps = 0.001"):
        assert {c for c, f in killed[e] if f == "vareps"} >= {"c320", "c640", "c1280", "c2560", "c640_rows1_vareps"}
    assert {c for c, f in killed["eps = 1e-05"] if f == "vareps"} >= {"c320_pitched_eps6", "c640_split_eps6"}
    assert {c for c, f in killed["one-pass variance in fp32"] if f == "ratio1000"} >= {"c64", "c320_split", "c1280_split", "c2056_lane0_fifth_trip", "c2560_split_row1"}
    assert ("c320_pitched_eps6", "benign") in killed["mean over the pitch"]


def test_layernorm_cases_cover_what_the_kernel_branches_on():
    cases = tb.LN_CASES.values()
    assert {c.C for c in cases} == {8, 64, 320, 512, 520, 640, 1280, 2048, 2056, 2560}
    assert {c.rows for c in cases} == {1, 3, 4, 5, 513}
    assert {c.layout for c in cases} == {"plain", "pitched", "split"} and {c.eps for c in cases} == {1e-5, 1e-6}
    fams = set()
    for c in cases:
        fams |= set(tb.families_of(c))
    assert fams == set(tb.FAMILIES)
    assert tb.chain_terms(2560) == (40, 6) and tb.chain_terms(8) == (8, 6) and tb.chain_terms(320, tb.LNGEMM_KERNEL) == (80, 2)
    assert tb.c_mean(2560) == 94 and tb.c_mean(320, tb.LNGEMM_KERNEL) == 166
    lin = tb.LIN_CASES.values()
    assert {c.M for c in lin} == {1, 31, 32, 33, 127, 128, 129, 300} and {c.N for c in lin} == {64, 128, 192, 960}
    assert {c.qcols for c in lin} == {0, 64, 320} and {c.split for c in lin} == {True, False} and {c.bias for c in lin} == {True, False}
    assert {c.geglu for c in lin} == {True, False}


@pytest.mark.parametrize("name", list(tb.LIN_CASES))
def test_ln_linear_bound(name):
    """Section b: the emulation of the fused launch and of the two-launch form within the SAME bound against the SAME reference (the fused one also
    with its scaled q columns); the unbiased variance is rejected by the benign rows of every case, a wrong eps by the variance-near-eps rows."""
    case = tb.LIN_CASES[name]
    inp = tb.make_lin_input(case, 11)
    lnref = tb.ln_reference(inp["x"], inp["gamma"], inp["beta"], 1e-5)
    ref, tol = tb.lin_reference(inp, case, lnref=lnref)
    ref1, tol1 = tb.lin_reference(inp, case, qscaled=False, lnref=lnref)
    fused, two = tb.emulate_ln_linear(inp, case), tb.emulate_ln_linear(inp, case, kernel=tb.LN_KERNEL)
    rf, rt = tb.row_ratio(fused, ref, tol).max().item(), tb.row_ratio(two, ref1, tol1).max().item()
    print(f"[tf-bound] ln_linear {name}: fused emulation at {rf:.3f} of the bound ({tb.margin(fused, ref, tol):.3f} of its derived part), two-launch at {rt:.3f} ({tb.margin(two, ref1, tol1):.3f})")
    assert rf <= 1.0 and rt <= 1.0
    lncase = tb.LnCase(320, case.M, "split" if case.split else "plain")
    for w, a in tb.ln_wrong_references(inp, lncase):
        if w != "variance / (C - 1)" and not w.startswith("eps"):
            continue
        wref, _ = tb.lin_reference(inp, case, a=a, lnref=lnref)
        killers = {f for f, v in tb.by_family(tb.row_ratio(fused, wref, tol), inp["fam"]).items() if v > 1.0}
        fam = tb.KILLED_BY[w]
        if fam in inp["fam"] and not (w == "eps = 1e-06" and case.M == 1):
            assert fam in killers, f"{name}: the {fam} rows accept the wrong reference '{w}'"


def test_bounds_reject_a_defective_emulation():
    """The mutation check, kept in the suite: the emulation with its variance divided by C - 1 breaks the LayerNorm bound at C = 320, 640, 1280 and the
    LN+GEMM bound; erf_as with a5 changed in its sixth digit breaks E_ERF by 10 x."""
    for name in ("c320", "c640", "c1280"):
        case = tb.LN_CASES[name]
        inp = tb.make_ln_input(case, 7)
        ref = tb.ln_reference(inp["x"], inp["gamma"], inp["beta"], case.eps)
        bad = tb.emulate_layernorm(inp, case.eps, unbiased=True).to(torch.float16)
        assert tb.by_family(tb.row_ratio(bad, ref.a, tb.ln_tol(ref, case.C)), inp["fam"])["benign"] > 1.0
    case = tb.LIN_CASES["m300_n960_plain"]
    inp = tb.make_lin_input(case, 11)
    ref, tol = tb.lin_reference(inp, case)
    assert tb.row_ratio(tb.emulate_ln_linear(inp, case, unbiased=True), ref, tol).max().item() > 1.0
    worst, _ = tb.erf_error(tb.all_fp16().float().numpy(), tb.A5_SIXTH_DIGIT)
    assert worst > 5 * tb.E_ERF


def test_e_erf_is_twice_the_recorded_worst_of_the_emulation():
    w16, at16 = tb.erf_error(tb.all_fp16().float().numpy())
    w32, at32 = tb.erf_error(tb.epilogue_gates())
    print(f"[tf-bound] 1 + erf_as: worst error of the emulation {w16:.4e} over the fp16 gates (g = {at16:.4f}), {w32:.4e} over the fp32 gates (g = {at32:.4f}); E_ERF = {tb.E_ERF:.3e}")
    assert max(w16, w32) <= tb.E_ERF_WORST_EMULATION * 1.001 and max(w16, w32) >= tb.E_ERF_WORST_EMULATION * 0.999
    assert 2 * tb.E_ERF_WORST_EMULATION <= tb.E_ERF <= 2.02 * tb.E_ERF_WORST_EMULATION
    g = tb.all_fp16().float()
    ge = (tb.emulate_gelu(g).double() - tb.gelu64(g)).abs().max().item()
    assert ge <= tb.GELU_WORST_EMULATION * 1.001
    # the negative tail: -0 below -5.547, where the true value is -8e-8 and smaller
    tail = g[(g < -5.547) & (g > -1.0e4)]
    assert (tb.emulate_gelu(tail) == 0).all() and tb.gelu64(tail).abs().max().item() < 1e-7


def test_geglu_sweep_bound():
    """Section c on the exhaustive sweep (every finite fp16 gate x the six h): the emulation within the bound; outputs whose reference overflows fp16
    are +-inf of the right sign; the tanh form, quick_gelu and the swapped halves are rejected (for every h whose products reach fp16's normal range)."""
    x = tb.geglu_sweep_input()
    C4 = x.shape[1] // 2
    h, g = x[:, :C4].float(), x[:, C4:].float()
    ref = tb.geglu_reference(h, g)
    tol = tb.geglu_tol(h, g, ref)
    emu = (h * tb.emulate_gelu(g)).to(torch.float16)
    cmp_, inf_ = tb.overflow_split(ref, tol)
    assert int(inf_.sum()) > 1000 and int((~cmp_ & ~inf_).sum()) < 50
    assert torch.equal(emu.double()[inf_], torch.sign(ref[inf_]) * float("inf"))
    for i, hv in enumerate(tb.GEGLU_H):
        r = tb.ratio(emu[i], ref[i], tol[i], cmp_[i])
        wr = {n: tb.ratio(emu[i], h[i].double() * w[i], tol[i], cmp_[i]) for n, w in tb.gelu_wrong_references(g)}
        wr["value and gate halves swapped"] = tb.ratio(emu[i], tb.geglu_reference(g, h)[i], tol[i], cmp_[i])
        print(f"[tf-bound] geglu sweep h = {hv:g}: emulation at {r:.3f} of the bound ({tb.margin(emu[i], ref[i], tol[i], mask=cmp_[i]):.3f} of its derived part); wrong references at "
              + ", ".join(f"'{n}' {v:.3g}" for n, v in wr.items()))
        assert r <= 1.0
        assert wr["value and gate halves swapped"] > 1.0 and wr["quick_gelu in place of gelu"] > 1.0
        if hv != 2.0 ** -14:
            assert wr["tanh-form GELU"] > 100.0


@pytest.mark.parametrize("name", list(tb.EPI_CASES))
def test_fused_epilogue_bound(name):
    case = tb.EPI_CASES[name]
    inp = tb.make_epilogue_input(name)
    ref, tol, wrong = tb.epilogue_reference(name, inp)
    emu = tb.emulate_epilogue(name, inp)
    cmp_, inf_ = tb.overflow_split(ref, tol)
    r = tb.ratio(emu, ref, tol, cmp_)
    wr = {n: tb.ratio(emu, w, tol, cmp_) for n, w in wrong}
    print(f"[tf-bound] epilogue {name} ({case.kernel}): emulation at {r:.3f} of the bound ({tb.margin(emu, ref, tol, case.split_out, cmp_):.3f} of its derived part), "
          f"{int(inf_.sum())} overflowing outputs; wrong references at " + ", ".join(f"'{n}' {v:.3g}" for n, v in wr.items()))
    assert r <= 1.0
    assert (torch.isinf(emu.double()[inf_])).all()
    g = inp["g32"]
    assert g.min() < -5.5e4 and g.max() > 5.5e4 and ((g > -12) & (g < 12)).sum() >= 1000
    assert (g.double() != g.to(torch.float16).double()).float().mean() > 0.5, "the bias must move the gates off the fp16 grid"
    for n, v in wr.items():
        if n == "erf with a5 changed in its sixth digit":      # below the rounding of an fp16 output (0.96 ... 1.01 of those bounds): the split output's case
            assert v > 3.0 or not case.split_out, f"{name}: '{n}' at {v:.3f}"
        else:
            assert v > 1.0, f"{name}: the bound accepts the wrong reference '{n}' ({v:.3f})"


def test_references_agree_with_torch_in_float64():
    g = torch.Generator().manual_seed(0)
    for C in (8, 320, 2560):
        x = torch.randn((5, C), generator=g, dtype=torch.float64) * 2 + 0.5
        gam, bet = torch.randn(C, generator=g, dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64)
        for eps in (1e-5, 1e-6):
            e = tb.f32eps(eps)
            assert (tb.ln_reference(x, gam, bet, eps).a - F.layer_norm(x, (C,), gam, bet, e)).abs().max().item() <= 1e-12
    gts = torch.cat([tb.all_fp16().double(), torch.linspace(-12, 12, 100001, dtype=torch.float64)])
    gts = gts[gts.abs() < 1e4]
    assert (tb.gelu64(gts) - F.gelu(gts)).abs().max().item() <= 1e-12
    assert (tb.quick_gelu_reference(gts) - gts * torch.sigmoid(tb.K_QUICK * gts)).abs().max().item() <= 1e-12
    # ... and the A&S formula in float64 is the 1.5e-7 of its name
    x = np.linspace(-6, 6, 200001)
    formula = tb.gelu_as64(torch.from_numpy(x * np.sqrt(2.0)), tb.A_S[4]) / torch.from_numpy(0.5 * x * np.sqrt(2.0)) - 1.0
    assert (formula - torch.special.erf(torch.from_numpy(x))).abs().nan_to_num(0.0).max().item() <= 1.5e-7


def test_flip_allowance():
    """Section b's flip set: a value within t of an fp16 rounding boundary may round the other way (one ulp while t < ulp), any other value may not."""
    a = torch.tensor([1.0 + 2.0 ** -11 - 1e-7, 1.0 + 2.0 ** -11 + 1e-7, 1.0 + 2.0 ** -12, 1.0, 3.0e-8, 100.03125 - 1e-6, 0.0], dtype=torch.float64)
    t = torch.full_like(a, 1e-6)
    t[4] = t[6] = 1e-9
    e = tb.flip_allowance(a, t)
    assert e.tolist() == [2.0 ** -10, 2.0 ** -10, 0.0, 0.0, 2.0 ** -24, 2.0 ** -4, 0.0]
    assert tb.flip_allowance(torch.tensor([1.3], dtype=torch.float64), torch.tensor([2.5 * 2.0 ** -10], dtype=torch.float64)).item() == 3 * 2.0 ** -10
