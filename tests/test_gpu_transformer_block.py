"""-m gpu: the LayerNorm / linear / GEGLU chain of the transformer block against float64 with the derived bounds of tests/transformer_bound.py
(judged on the CPU by tests/test_cpu_transformer_bound.py): ldiff_op_layernorm (layernorm_kernel), ldiff_op_ln_linear (lngemm<320>,
lngemm<320,geglu>) and the two-launch form it replaces, ldiff_op_geglu (geglu_kernel) over every finite fp16 gate, and the fused GELU / GEGLU /
quick_gelu epilogues of gemm_dma, gemm_df and lngemm on inputs that are exact by construction.  Every case states the kernel it is meant for and
fails if the library routes it elsewhere; every case's bound also rejects that case's wrong references (the table of test_cpu_transformer_bound.py).

"of the bound" is max |error| / bound; an fp16 output's own rounding takes that to ~0.99 by its nature, so each line also gives the share of the
DERIVED part of the bound that is used (transformer_bound.margin: what the error exceeds the output's rounding by, over the rest of the bound).

MEASURED (MI355X), worst of the bound / of its derived part, per kernel:
    layernorm_kernel (19 launches)            0.997 / 0.062 (c320_split); per family: benign 0.992, ratio30 0.981, ratio1000 0.981, vareps 0.993, outlier 0.997
    lngemm<320> (8 cases)                     0.779 / 0.142 (m129_n192_split_q64)
    lngemm<320,geglu> (3 cases)               0.575 / 0.044
    layernorm + gemm_dma<64,64> (11 cases)    0.769 / 0.107
    geglu_kernel, 6 x 63,488 gates            0.996 / 0.068 (h = 100); tanh-form GELU at 116-123 x the bound, quick_gelu 4.0e3 x, swapped halves > 3e5 x
    gemm_dma<64,64> GEGLU                     0.986 / 0.047        act_out 2 (gelu) 0.984 / 0.073        act_out 1 (quick_gelu) 0.981 / 0.000
    gemm_dma<64,64> act_out 2, split output   0.470 / 0.135; a5 changed in its sixth digit at 3.71 x the bound (0.96-1.01 of every fp16-output bound)
    gemm_dma<64,64> act_out 1, split output   0.499 / 0.000 (gelu in place of quick_gelu at 1.7e5 x the bound)
    gemm_df<geglu>                            0.993 / 0.110        lngemm<320,geglu> epilogue 0.963 / 0.037
    No derived part is used beyond 0.15: no thin margin.  The kernels' figures equal those of the CPU emulations (tests/test_cpu_transformer_bound.py, same
    seeds) to the digits shown, except the derived parts of three LN+GEMM cases (association of the MFMA sums).  No kernel was changed.
"""
import contextlib
import ctypes as C

import pytest
import torch

import transformer_bound as tb
from kernel_routing import check_route, reached
from ldiffusion_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"


def sp():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@contextlib.contextmanager
def launched(lib):
    """with launched(lib) as names: <launches> -> every profiler row name (kernel_routing.reached keeps the matrix kernels only, and
    "layernorm" is none)."""
    names = set()
    torch.cuda.synchronize()
    lib.ldiff_prof_set_filter(None)
    _lib.prof_collect()
    lib.ldiff_prof_enable(1)
    try:
        yield names
    finally:
        try:
            torch.cuda.synchronize()
            names.update(r["name"] for r in _lib.prof_collect())
        finally:
            lib.ldiff_prof_enable(0)


def device_rows(inp, layout):
    """The rows as the kernel reads them -> (buffer on the device, ldx, x_lo).  split: [hi | lo]; pitched: rows C + 24 apart, NaN in between (the
    kernel must not read it)."""
    hi, lo = inp["hi"], inp["lo"]
    rows, Cc = hi.shape
    if layout == "split":
        return torch.cat([hi, lo], 1).contiguous().to(DEV), 2 * Cc, Cc
    if layout == "pitched":
        buf = torch.full((rows, Cc + tb.PITCH_EXTRA), float("nan"), dtype=torch.float16)
        buf[:, :Cc] = hi
        return buf.to(DEV), Cc + tb.PITCH_EXTRA, 0
    return hi.contiguous().to(DEV), 0, 0


def canaried(rows, cols):
    """An output of NaN with three rows behind its end: every element of the first `rows` must be written, nothing behind them."""
    return torch.full((rows + 3, cols), float("nan"), dtype=torch.float16, device=DEV)


def check_canaries(y, rows, what):
    yc = y.cpu()
    assert torch.isnan(yc[rows:].float()).all(), f"{what}: rows behind the last one were written"
    assert not torch.isnan(yc[:rows].float()).any(), f"{what}: unwritten (or NaN) outputs"
    return yc[:rows]


def family_killers(got, inp, wrong, tol):
    return {name: {f for f, v in tb.by_family(tb.row_ratio(got, w, tol), inp["fam"]).items() if v > 1.0} for name, w in wrong}


# ======================================================================================================================
# a. LayerNorm (ldiff_op_layernorm -> layernorm_kernel)
# ======================================================================================================================
def run_layernorm(lib, inp, layout, eps):
    xd, ldx, x_lo = device_rows(inp, layout)
    rows, Cc = inp["hi"].shape
    gd, bd = inp["gamma"].to(DEV), inp["beta"].to(DEV)
    y = canaried(rows, Cc)
    with launched(lib) as names:
        _lib.check(lib.ldiff_op_layernorm(xd.data_ptr(), ldx, x_lo, y.data_ptr(), rows, Cc, gd.data_ptr(), bd.data_ptr(), eps, sp()))
    assert "layernorm" in names, f"reached {sorted(names)}, the case is meant for layernorm_kernel"
    return check_canaries(y, rows, "layernorm")


@pytest.mark.parametrize("name", list(tb.LN_CASES))
def test_layernorm_against_float64(lib, name):
    """layernorm_kernel against the float64 LayerNorm of the values it sees, within transformer_bound.ln_tol per element, for every row family of the
    launch; constant and all-zero rows equal f16(beta) EXACTLY; nothing is written behind the last row; the bound rejects the case's wrong
    references by the rows of the family that must (transformer_bound.KILLED_BY)."""
    case = tb.LN_CASES[name]
    inp = tb.make_ln_input(case, 7)
    y = run_layernorm(lib, inp, case.layout, case.eps)
    ref = tb.ln_reference(inp["x"], inp["gamma"], inp["beta"], case.eps)
    tol = tb.ln_tol(ref, case.C)
    worst = tb.by_family(tb.row_ratio(y, ref.a, tol), inp["fam"])
    print(f"[tf-err] layernorm {name} (layernorm_kernel, {case.layout}, eps {case.eps:g}): {max(worst.values()):.3f} of the bound, {tb.margin(y, ref.a, tol):.3f} of its derived part; "
          + ", ".join(f"{f} {v:.3f}" for f, v in worst.items()))
    assert max(worst.values()) <= 1.0, f"{name}: {worst}"
    b16 = inp["beta"].to(torch.float16)
    for i, f in enumerate(inp["fam"]):
        if f in ("const", "zero"):
            assert torch.equal(y[i], b16), f"{name}: row {i} ({f}) differs from f16(beta) in {int((y[i] != b16).sum())} channels"
    for w, killers in family_killers(y, inp, tb.ln_wrong_references(inp, case), tol).items():
        fam = tb.KILLED_BY[w]
        if fam in inp["fam"]:
            assert fam in killers, f"{name}: the {fam} rows accept the wrong reference '{w}'"


def test_layernorm_refuses_what_the_kernel_does_not_take(lib):
    """C = 2568 (a sixth trip), C % 8 != 0, a pitch or a lo offset that is no multiple of 8: refused, not mis-computed."""
    x = torch.zeros((4, 8192), dtype=torch.float16, device=DEV)
    y = torch.zeros((4, 4096), dtype=torch.float16, device=DEV)
    gb = torch.zeros(4096, device=DEV)
    for ldx, x_lo, Cc in ((0, 0, 2568), (0, 0, 12), (324, 0, 320), (648, 324, 320), (644, 320, 320)):
        with pytest.raises(ValueError):
            _lib.check(lib.ldiff_op_layernorm(x.data_ptr(), ldx, x_lo, y.data_ptr(), 4, Cc, gb.data_ptr(), gb.data_ptr(), 1e-5, sp()))
    _lib.check(lib.ldiff_op_layernorm(x.data_ptr(), 648, 328, y.data_ptr(), 4, 320, gb.data_ptr(), gb.data_ptr(), 1e-5, sp()))
    torch.cuda.synchronize()


# ======================================================================================================================
# b. LayerNorm into a GEMM (ldiff_op_ln_linear -> lngemm<320>, lngemm<320,geglu>; ldiff_op_layernorm + ldiff_op_conv -> gemm_dma<64,64>)
# ======================================================================================================================
def linear_operands(W, bias, geglu):
    """Weights and bias as the kernels read them (GEGLU: value / gate rows interleaved by 16), rows padded to a multiple of 16."""
    N = W.shape[0]
    if geglu:
        perm = tb.geglu_perm(N // 2)
        W, bias = W[perm], (bias[perm] if bias is not None else None)
    Nrows = (N + 15) // 16 * 16
    wd = torch.zeros((Nrows, W.shape[1]), dtype=torch.float16)
    wd[:N] = W
    bd = None
    if bias is not None:
        bd = torch.zeros(Nrows)
        bd[:N] = bias
        bd = bd.to(DEV)
    return wd.to(DEV), bd, Nrows


def run_ln_linear(lib, inp, M, N, layout, eps, geglu, qcols, qscale):
    xd, ldx, x_lo = device_rows(inp, layout)
    wd, bd, Nrows = linear_operands(inp["W"], inp["bias"], geglu)
    gd, btd = inp["gamma"].to(DEV), inp["beta"].to(DEV)
    Nout = N // 2 if geglu else N
    y = canaried(M, Nout)
    with reached(lib) as names:
        _lib.check(lib.ldiff_op_ln_linear(xd.data_ptr(), ldx, x_lo, M, 320, gd.data_ptr(), btd.data_ptr(), eps, wd.data_ptr(), N, Nrows,
                                          bd.data_ptr() if bd is not None else None, 1 if geglu else 0, y.data_ptr(), Nout, qcols, qscale, sp()))
    check_route(names, "lngemm<320,geglu>" if geglu else "lngemm<320>", f"ln_linear M={M} N={N}")
    return check_canaries(y, M, "ln_linear")


def run_two_launches(lib, inp, M, N, layout, eps, geglu):
    xd, ldx, x_lo = device_rows(inp, layout)
    wd, bd, Nrows = linear_operands(inp["W"], inp["bias"], geglu)
    gd, btd = inp["gamma"].to(DEV), inp["beta"].to(DEV)
    Nout = N // 2 if geglu else N
    n = canaried(M, 320)
    y = canaried(M, Nout)
    a = _lib.ConvArgs()
    a.x, a.C1, a.B, a.Hin, a.Win, a.Hout, a.Wout, a.ks, a.stride = n.data_ptr(), 320, 1, 1, M, 1, M, 1, 1
    a.w, a.N, a.Nrows, a.y, a.ldy, a.geglu = wd.data_ptr(), N, Nrows, y.data_ptr(), Nout, 1 if geglu else 0
    if bd is not None:
        a.bias = bd.data_ptr()
    with reached(lib) as names:
        _lib.check(lib.ldiff_op_layernorm(xd.data_ptr(), ldx, x_lo, n.data_ptr(), M, 320, gd.data_ptr(), btd.data_ptr(), eps, sp()))
        _lib.check(lib.ldiff_op_conv(C.byref(a), sp()))
    check_route(names, "gemm_dma<64,64>", f"layernorm + linear M={M} N={N}")
    check_canaries(n, M, "layernorm of the two-launch form")
    return check_canaries(y, M, "linear of the two-launch form")


@pytest.mark.parametrize("name", list(tb.LIN_CASES))
def test_ln_linear_against_float64(lib, name):
    """The fused launch and the two-launch form against sum_c W16 r16(a) + bias with a the float64 LayerNorm, each within the SAME bound
    (transformer_bound.ln_linear_reference; the fused launch also with its q columns scaled in fp32 before the one rounding); NaN canaries; the
    unbiased variance and a wrong eps are rejected by the rows that must."""
    case = tb.LIN_CASES[name]
    inp = tb.make_lin_input(case, 11)
    layout = "split" if case.split else "plain"
    lnref = tb.ln_reference(inp["x"], inp["gamma"], inp["beta"], 1e-5)
    ref, tol = tb.lin_reference(inp, case, lnref=lnref)
    ref1, tol1 = tb.lin_reference(inp, case, qscaled=False, lnref=lnref)
    fused = run_ln_linear(lib, inp, case.M, case.N, layout, 1e-5, case.geglu, case.qcols, tb.QSCALE if case.qcols else 1.0)
    two = run_two_launches(lib, inp, case.M, case.N, layout, 1e-5, case.geglu)
    wf, wt = tb.by_family(tb.row_ratio(fused, ref, tol), inp["fam"]), tb.by_family(tb.row_ratio(two, ref1, tol1), inp["fam"])
    print(f"[tf-err] ln_linear {name} (lngemm<320{',geglu' if case.geglu else ''}>): {max(wf.values()):.3f} of the bound, {tb.margin(fused, ref, tol):.3f} of its derived part; "
          f"two launches (layernorm + gemm_dma<64,64>): {max(wt.values()):.3f}, {tb.margin(two, ref1, tol1):.3f}; fused by family: " + ", ".join(f"{f} {v:.3f}" for f, v in wf.items()))
    assert max(wf.values()) <= 1.0, f"{name}: fused launch {wf}"
    assert max(wt.values()) <= 1.0, f"{name}: two-launch form {wt}"
    lncase = tb.LnCase(320, case.M, layout)
    for w, a in tb.ln_wrong_references(inp, lncase):
        if w != "variance / (C - 1)" and not w.startswith("eps"):
            continue
        wref, _ = tb.lin_reference(inp, case, a=a, lnref=lnref)
        fam = tb.KILLED_BY[w]
        if fam in inp["fam"] and not (w == "eps = 1e-06" and case.M == 1):
            assert tb.by_family(tb.row_ratio(fused, wref, tol), inp["fam"])[fam] > 1.0, f"{name}: the {fam} rows accept the wrong reference '{w}'"


# ======================================================================================================================
# c. GELU / GEGLU
# ======================================================================================================================
def judge_activation(got, ref, tol, what, split_out=False):
    """got within tol wherever the reference stays inside fp16's range with the bound to spare; +-inf of the right sign where it leaves it."""
    cmp_, inf_ = tb.overflow_split(ref, tol)
    g = got.double()
    assert torch.equal(g[inf_], torch.sign(ref[inf_]) * float("inf")), f"{what}: an overflowing output is not +-inf of the right sign"
    assert torch.isfinite(g[cmp_]).all(), f"{what}: non-finite outputs inside fp16's range"
    return tb.ratio(got, ref, tol, cmp_), tb.margin(got, ref, tol, split_out, cmp_), cmp_


def test_geglu_kernel_every_fp16_gate(lib):
    """geglu_kernel (ldiff_op_geglu launches no other kernel) over every finite fp16 gate -- +-0 and the subnormals included -- against h in {1, -1,
    1/3, 100, 2^-14, 6e4}, one launch [6, 2 x 63,488], judged per element by transformer_bound.geglu_tol; the tanh form, quick_gelu and swapped
    halves are rejected."""
    x = tb.geglu_sweep_input()
    M, C4 = x.shape[0], x.shape[1] // 2
    xd = x.to(DEV)
    y = canaried(M, C4)
    _lib.check(lib.ldiff_op_geglu(xd.data_ptr(), y.data_ptr(), M, C4, sp()))
    torch.cuda.synchronize()
    yc = y.cpu()
    assert torch.isnan(yc[M:].float()).all() and not torch.isnan(yc[:M].float()).any()
    yc = yc[:M]
    h, g = x[:, :C4].float(), x[:, C4:].float()
    ref = tb.geglu_reference(h, g)
    tol = tb.geglu_tol(h, g, ref)
    for i, hv in enumerate(tb.GEGLU_H):
        r, mg, cmp_ = judge_activation(yc[i], ref[i], tol[i], f"h = {hv:g}")
        wr = {n: tb.ratio(yc[i], h[i].double() * w[i], tol[i], cmp_) for n, w in tb.gelu_wrong_references(g)}
        wr["value and gate halves swapped"] = tb.ratio(yc[i], tb.geglu_reference(g, h)[i], tol[i], cmp_)
        print(f"[tf-err] geglu_kernel h = {hv:g}: {r:.3f} of the bound, {mg:.3f} of its derived part; wrong references at " + ", ".join(f"'{n}' {v:.3g}" for n, v in wr.items()))
        assert r <= 1.0, f"h = {hv:g}: {r:.3f} of the bound"
        assert wr["value and gate halves swapped"] > 1.0 and wr["quick_gelu in place of gelu"] > 1.0
        if hv != 2.0 ** -14:
            assert wr["tanh-form GELU"] > 100.0


def run_epilogue(lib, name, inp):
    case = tb.EPI_CASES[name]
    M, K, N = case.M, case.K, case.N
    geglu = case.mode == "geglu"
    Nout = N // 2 if geglu else N
    wd, bd, Nrows = linear_operands(inp["W"], inp["bias"], geglu)
    xd = inp["x"].contiguous().to(DEV)
    y = canaried(M, 2 * Nout if case.split_out else Nout)
    with reached(lib) as names:
        if case.kernel.startswith("lngemm"):
            gd, btd = inp["gamma"].to(DEV), inp["beta"].to(DEV)
            _lib.check(lib.ldiff_op_ln_linear(xd.data_ptr(), 0, 0, M, K, gd.data_ptr(), btd.data_ptr(), 1e-5, wd.data_ptr(), N, Nrows, bd.data_ptr(), 1, y.data_ptr(), Nout, 0, 1.0, sp()))
        else:
            a = _lib.ConvArgs()
            a.x, a.C1, a.B, a.Hin, a.Win, a.Hout, a.Wout, a.ks, a.stride = xd.data_ptr(), K, 1, 1, M, 1, M, 1, 1
            a.w, a.N, a.Nrows, a.bias, a.y, a.ldy = wd.data_ptr(), N, Nrows, bd.data_ptr(), y.data_ptr(), y.shape[1]
            a.geglu, a.act_out, a.y_lo = int(geglu), {"geglu": 0, "quick_gelu": 1, "gelu": 2}[case.mode], Nout if case.split_out else 0
            _lib.check(lib.ldiff_op_conv(C.byref(a), sp()))
    check_route(names, case.kernel, name)
    yc = check_canaries(y, M, name)
    return yc[:, :Nout].double() + yc[:, Nout:].double() if case.split_out else yc


@pytest.mark.parametrize("name", list(tb.EPI_CASES))
def test_fused_epilogue_exact_by_construction(lib, name):
    """One-hot weight rows make every fp32 sum ONE fp16 element of the row, the fp32 bias moves it off the fp16 grid: value and gate of every output
    are known exactly, and the epilogue (GEGLU of gemm_dma / gemm_df / lngemm, act_out 1 | 2 of gemm_dma) is judged by section c per element, the
    gates dense over [-12, 12] with tails to +-6e4.  The split output of act_out = 2 is the one case that resolves erf_as below an fp16 rounding."""
    case = tb.EPI_CASES[name]
    inp = tb.make_epilogue_input(name)
    got = run_epilogue(lib, name, inp)
    ref, tol, wrong = tb.epilogue_reference(name, inp)
    r, mg, cmp_ = judge_activation(got, ref, tol, name, case.split_out)
    wr = {n: tb.ratio(got, w, tol, cmp_) for n, w in wrong}
    print(f"[tf-err] epilogue {name} ({case.kernel}, {case.mode}{', split output' if case.split_out else ''}): {r:.3f} of the bound, {mg:.3f} of its derived part; wrong references at "
          + ", ".join(f"'{n}' {v:.3g}" for n, v in wr.items()))
    assert r <= 1.0, f"{name}: {r:.3f} of the bound"
    for n, v in wr.items():
        if n == "erf with a5 changed in its sixth digit":
            assert v > 1.0 or not case.split_out, f"{name}: '{n}' at {v:.3f}"
        else:
            assert v > 1.0, f"{name}: the bound accepts the wrong reference '{n}' ({v:.3f})"
