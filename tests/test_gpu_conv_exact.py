"""-m gpu: the diffusion path's contraction kernels, bit for bit, on the cases of tests/conv_exact.py: one launch per case and regime through
ldiff_op_conv (split operands through ldiff_op_dup_weights), the stored bytes against the expected bits with torch.equal -- hi and lo halves separately,
fp32 outputs as fp32 -- and the totals of the fused statistics in float64 for equality.  Regime E: integer operands, every sum exact; regime R: the
kernel's own order of fp32 additions on random addends.  The outputs are pre-filled with a sentinel, carry canary rows behind M and eight columns behind
the stored ones; each launch goes through reached() / check_route."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_exact as ce
from kernel_routing import check_route, reached
from ldiffusion_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PARAMS = [(n, r) for n, c in ce.CASES.items() for r in c.get("regimes", "E")]


def sp():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _source(hi, lo, wide):
    """[B, H, W, C] (-> [hi | lo] rows of 2 C where the source is split or read through a pitch)"""
    return _dev(np.concatenate([hi, lo], -1) if wide else hi, torch.float16)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _same(got, want, what):
    """torch.equal on the bit patterns; on failure the count and the first differing index with both patterns"""
    g, w = _bits(got), _bits(want)
    if torch.equal(g, w):
        return
    bad = (g != w).nonzero()
    i = tuple(int(v) for v in bad[0])
    mask = 0xFFFF if g.dtype == torch.int16 else 0xFFFFFFFF
    raise AssertionError(f"{what}: {len(bad)} of {g.numel()} elements differ; first at {i}: got 0x{int(g[i]) & mask:x} ({float(got[i])!r}), "
                         f"expected 0x{int(w[i]) & mask:x} ({float(want[i])!r})")


@pytest.mark.parametrize("name,regime", PARAMS)
def test_conv_exact(lib, name, regime):
    c, o = ce.build(name, regime)
    want = ce.expected(c, o, regime)
    wide = c.opsplit or c.pitch
    keep = []
    a_ = _lib.ConvArgs()
    x1 = _source(o.x_hi[..., :c.C1], o.x_lo[..., :c.C1] if wide else None, wide)
    a_.x, a_.C1, a_.ld1 = x1.data_ptr(), (2 if c.opsplit else 1) * c.C1, 2 * c.C1 if wide else 0
    if c.C2:
        x2 = _source(o.x_hi[..., c.C1:], o.x_lo[..., c.C1:] if wide else None, wide)
        a_.x2, a_.C2, a_.ld2 = x2.data_ptr(), (2 if c.opsplit else 1) * c.C2, 2 * c.C2 if wide else 0
    taps, Nrows = c.ks * c.ks, (c.N + 15) // 16 * 16
    wd = torch.zeros((Nrows, taps * c.Cin), dtype=torch.float16, device=DEV)
    wd[:c.N] = _dev(o.w.reshape(c.N, -1), torch.float16)
    if c.opsplit:   # per tap [a (C1) b (C2)] -> [a a b b]: the contraction over [hi | lo] rows
        wdup = torch.full((Nrows, taps * 2 * c.Cin), float("nan"), dtype=torch.float16, device=DEV)
        _lib.check(lib.ldiff_op_dup_weights(wd.data_ptr(), wdup.data_ptr(), Nrows, taps, c.Cin, c.C1, c.C2, 2 * c.Cin, sp()))
        keep.append(wd)
        wd = wdup
    a_.w, a_.N, a_.Nrows, a_.n_real = wd.data_ptr(), c.N, Nrows, c.n_real
    a_.B, a_.Hin, a_.Win, a_.Hout, a_.Wout = c.B, c.H, c.W, c.Ho, c.Wo
    a_.ks, a_.stride, a_.ups, a_.c3d_ups, a_.pad_t, a_.pad_l = c.ks, c.stride, c.ups, c.c3d_ups, c.pads[0], c.pads[2]
    if c.gn:
        sd, hd = _dev(o.scale, torch.float32), _dev(o.shift, torch.float32)
        keep += [sd, hd]
        a_.gn_scale, a_.gn_shift, a_.silu_in = sd.data_ptr(), hd.data_ptr(), int(c.gn == "silu")
    bd = torch.zeros(Nrows, device=DEV)
    bd[:c.N] = _dev(o.bias, torch.float32)
    a_.bias = bd.data_ptr()
    if c.sc:
        sxd, swd = _dev(o.sc_x, torch.float16), torch.zeros((Nrows, c.sc), dtype=torch.float16, device=DEV)
        swd[:c.N] = _dev(o.sc_w, torch.float16)
        sbd = torch.zeros(Nrows, device=DEV)
        sbd[:c.N] = _dev(o.sc_bias, torch.float32)
        keep += [sxd, swd, sbd]
        a_.sc_x, a_.sc_C, a_.sc_ld, a_.sc_w, a_.sc_bias = sxd.data_ptr(), c.sc, c.sc_pitch, swd.data_ptr(), sbd.data_ptr()
    if c.temb:
        td = _dev(o.temb, torch.float32)
        a_.temb, a_.ld_temb = td.data_ptr(), c.N
    if c.res:
        rd = _dev(np.concatenate([o.res_hi, o.res_lo], -1) if c.res == "split" else o.res_hi, torch.float16)
        a_.res, a_.ld_res, a_.res_lo = rd.data_ptr(), rd.shape[-1], c.N if c.res == "split" else 0
    stored = 2 * c.N if c.out == "split" else c.N
    ldy = stored + ce.PAD_COLS
    y = torch.full((c.M + ce.CANARY_ROWS, ldy), ce.SENTINEL16, dtype=torch.int16, device=DEV)
    if c.out == "f32":
        y = torch.full((c.M + ce.CANARY_ROWS, ldy), ce.SENTINEL16 * 0x10001, dtype=torch.int32, device=DEV)
    a_.y, a_.ldy, a_.y_lo, a_.out_f32 = y.data_ptr(), ldy, c.N if c.out == "split" else 0, int(c.out == "f32")
    a_.splitk, a_.short_runs, a_.out_shift, a_.gemm_df = c.splitk, c.short_runs, c.out_shift, c.gemm_df
    if c.stats:
        R = lib.ldiff_op_conv_stats_blocks(C.byref(a_))
        assert R > 0, f"{name}: the launch takes no fused statistics"
        st = torch.full((c.B, c.N, R, 2), float("nan"), device=DEV)
        a_.stats = st.data_ptr()
    with reached(lib) as names:
        _lib.check(lib.ldiff_op_conv(C.byref(a_), sp()))
    torch.cuda.synchronize()
    check_route(names, c.kernel, f"{name} [{regime}]")
    yv = y.view(torch.float32 if c.out == "f32" else torch.float16)
    fill = ce.SENTINEL16 * 0x10001 if c.out == "f32" else ce.SENTINEL16
    assert bool((y[c.M:] == fill).all()), f"{name}: the rows behind M were written"
    assert bool((y[:, stored:] == fill).all()), f"{name}: the columns behind the stored ones were written"
    got = yv[:c.M].view(c.B, c.Ho, c.Wo, ldy)
    n = 0
    for key, col0 in (("f32", 0), ("hi", 0), ("lo", c.N)):
        if key in want:
            w = torch.from_numpy(want[key]).to(DEV)
            _same(got[..., col0:col0 + c.N], w, f"{name} [{regime}] {key}")     # (the pad column of a narrow launch is expected as zero: bias of the zero row)
            n += w.numel()
    line = f"[conv-exact] {name} [{regime}]: {c.kernel}, {n} elements equal"
    if "stats" in want:
        stc = st.double().cpu()
        assert torch.isfinite(stc).all(), f"{name}: statistics partials left unwritten"
        assert stc.abs().max() < 2 ** 24, f"{name}: a stored partial reaches {stc.abs().max():.0f}: not exact in fp32"
        tot = stc.sum(2)
        wt = torch.from_numpy(want["stats"])
        bad = (tot != wt).nonzero()
        assert len(bad) == 0, (f"{name}: {len(bad)} of {tot.numel()} statistics totals differ; first at {tuple(int(v) for v in bad[0])}: "
                               f"got {tot[tuple(bad[0])].item()!r}, expected {wt[tuple(bad[0])].item()!r}")
        line += f", {tot.numel()} statistics totals equal ({R} partials per channel)"
    print(line)
