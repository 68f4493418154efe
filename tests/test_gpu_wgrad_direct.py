"""GPU (-m gpu): the direct weight gradient and the slab column sum (csrc/kernels_wgrad.hip; ldiff_op_conv_wgrad, ldiff_op_colsum_slabs) and the route setting
of autograd.Conv2dFn -- exact on integer data, within the derived bound of tests/wgrad_bound.py on random data, refusals, and one backward pass of the
tissue-head trainer on the direct route graded as tests/test_gpu_nnunet_train.py grades the whole step.

The column sum on its capped plan (M = 300 007 rows, N = 24: 1024 slabs of 293 rows, 85 row lanes), measured on an MI355X: worst element at 0.003 of the bound
(M = 4800, N = 32 in the same run: 0.021)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nnunet_train_ref as ref
import wgrad_bound as wb
from ldiffusion_amd import _lib, autograd as ag, nnunet, nnunet_train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def sp():
    return _lib.stream_ptr()


def run_wgrad(lib, x, dy, Cout, Cin, k, stride, wgs):
    """numpy NHWC fp16 x, dy -> dw [Cout, Cin, k, k] as a float32 CPU tensor, straight through the C entry points, into NaN-filled buffers."""
    xd, dyd = torch.from_numpy(x).to(DEV), torch.from_numpy(dy).to(DEV)
    B, H, W, Cx = x.shape
    _, Ho, Wo, Cy = dy.shape
    nb = lib.ldiff_op_conv_wgrad_ws_bytes(B, Ho, Wo, Cx, Cy, k, wgs)
    assert nb == ag.wgrad_plan(B, Ho, Wo, Cx, Cy, k, wgs)["ws_bytes"] > 0, "the python statement of the plan and the library's disagree"
    ws = torch.full((nb // 4 + 4,), float("nan"), dtype=torch.float32, device=DEV)
    dw = torch.full((Cout, Cin, k, k), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(lib.ldiff_op_conv_wgrad(_lib.ptr(xd), _lib.ptr(dyd), _lib.ptr(dw), B, H, W, Cx, Ho, Wo, Cy, Cout, Cin, k, stride, wgs, _lib.ptr(ws), nb, sp()))
    torch.cuda.synchronize()
    return dw.cpu()


def run_colsum(lib, dy, N):
    d = torch.from_numpy(dy).to(DEV)
    M, ld = dy.shape
    nb = lib.ldiff_op_colsum_slabs_ws_bytes(M, N)
    assert nb == ag.colsum_slabs_plan(M, N)["ws_bytes"] > 0
    ws = torch.full((nb // 4 + 4,), float("nan"), dtype=torch.float32, device=DEV)
    db = torch.full((N,), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(lib.ldiff_op_colsum_slabs(_lib.ptr(d), _lib.ptr(db), M, N, ld, _lib.ptr(ws), nb, sp()))
    torch.cuda.synchronize()
    return db.cpu()


# ---- 1. exact integers ------------------------------------------------------------------------------------------------------------------------------
CHANNELS = [(8, 3, 32, 32, 3, 1), (32, 32, 32, 32, 3, 1), (64, 64, 32, 32, 3, 1), (32, 32, 64, 64, 3, 2), (64, 64, 64, 64, 3, 1), (128, 128, 64, 64, 3, 1),
            (32, 32, 8, 5, 1, 1), (64, 64, 128, 128, 1, 1)]   # (Cx, Cin, Cy, Cout, k, stride)
SHAPES = [(1, 8, 8), (3, 20, 40), (2, 33, 31)]
SHAPES_S2 = [(2, 18, 18), (2, 17, 19)]
INT_CASES = [(c, s) for c in CHANNELS for s in SHAPES + (SHAPES_S2 if c[5] == 2 else [])]


@pytest.mark.parametrize("chan,shape", INT_CASES)
def test_wgrad_exact_on_integers(lib, chan, shape):
    """Integer data in [-3, 3], pad channels included: every fp32 sum is exact while 9 M < 2^24, so dw equals the integer reference bit for bit -- with the
    planned grid, one workgroup, three (each walks several tiles) and more workgroups than tiles (idle ones contribute exact zeros); garbage in the pad
    channels of x and dy does not leak; a second call into fresh buffers is bit-identical."""
    Cx, Cin, Cy, Cout, k, stride = chan
    B, H, W = shape
    x, dy = wb.int_case(B, H, W, Cx, Cy, k, stride, 7 + Cx + Cy + H)
    M = dy.shape[0] * dy.shape[1] * dy.shape[2]
    assert 9 * M < 2 ** 24
    if Cin < Cx:
        assert np.abs(x[..., Cin:]).sum() > 0
    if Cout < Cy:
        assert np.abs(dy[..., Cout:]).sum() > 0
    want64, _ = wb.wgrad_reference(x, dy, Cout, Cin, k, stride)
    assert np.array_equal(want64, np.rint(want64))
    want = torch.from_numpy(want64.astype(np.int64))
    tiles = ag.wgrad_plan(dy.shape[0], dy.shape[1], dy.shape[2], Cx, Cy, k, 0)["tiles"]
    for wgs in (0, 1, 3, tiles + 5):
        got = run_wgrad(lib, x, dy, Cout, Cin, k, stride, wgs)
        assert got.isfinite().all(), f"wgs={wgs}: non-finite output"
        assert torch.equal(got.to(torch.int64), want) and torch.equal(got, want.float()), f"wgs={wgs}: {(got.double() - want.double()).abs().max():.0f} off at most"
        assert torch.equal(run_wgrad(lib, x, dy, Cout, Cin, k, stride, wgs), got), f"wgs={wgs}: a second call differs"


COLSUM_INT_CASES = [(M, N) for N in (8, 32, 128) for M in (1, 7, 4800, 70000)]
# N / 8 = 3, 5, 129 does not divide 256 (85, 51, 1 row lanes; 1, 1, 127 idle threads; 24 is the seg head's pitch for 17 .. 24 heads) and the widest row the
# entry takes (256 threads a row, one row lane): one row, fewer rows than row lanes, 19 slabs
COLSUM_INT_CASES += [(M, N) for N in (24, 40, 1032, 2048) for M in (1, 7, 4800)]
# more than CS_MAX_SLABS * CS_ROWS = 262 144 rows: the capped plan, 1024 slabs of 293 rows (more than 256: the `2d` plan's M = 12 * 512^2 runs this way), the last of 268
COLSUM_CAPPED_M = 300007
COLSUM_INT_CASES += [(COLSUM_CAPPED_M, N) for N in (8, 24)]


@pytest.mark.parametrize("M,N", COLSUM_INT_CASES)
def test_colsum_slabs_exact_on_integers(lib, M, N):
    ld = N + 8
    dy = np.random.default_rng(M + N).integers(-3, 4, (M, ld)).astype(np.float16)
    assert 3 * M < 2 ** 24
    want = torch.from_numpy(dy[:, :N].astype(np.int64).sum(0))
    got = run_colsum(lib, dy, N)
    assert torch.equal(got.to(torch.int64), want) and torch.equal(got, want.float())
    assert torch.equal(run_colsum(lib, dy, N), got)


# ---- 2. random data against float64 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,Cc", wb.BOUND_CASES)
def test_wgrad_against_float64(lib, B, H, W, Cc):
    """Per element within (L + P + 2) 2^-24 sum |dy x| of float64 on the same fp16 inputs, L and P from the kernel's plan at wgs = 8 (tests/wgrad_bound.py;
    tests/test_cpu_wgrad_bound.py shows what this bound rejects on these very inputs)."""
    k, stride = 3, 1
    x, dy = wb.random_case(B, H, W, Cc, Cc, k, stride, 10 + Cc + H)
    plan = wb.plan_of(B, H, W, Cc, Cc, k, wb.BOUND_WGS)
    want, mag = wb.wgrad_reference(x, dy, Cc, Cc, k, stride)
    got = run_wgrad(lib, x, dy, Cc, Cc, k, stride, wb.BOUND_WGS).double().numpy()
    tol = wb.bound(mag, plan)
    print(f"[wgrad] B={B} {H}x{W} {Cc}->{Cc}: chain {plan['chain']}, partials {plan['partials']}: worst element at {(np.abs(got - want) / tol).max():.3f} of the bound")
    assert (np.abs(got - want) <= tol).all()


def test_colsum_slabs_against_float64(lib):
    """The ABI of the column sum carries no workgroup count: the bound's L and P are those of the library's own plan for M = 4800 (19 slabs)."""
    _colsum_against_float64(lib, 4800, 32)


def test_colsum_slabs_capped_plan_against_float64(lib):
    """The same on the capped plan with N / 8 = 3 threads a row: 1024 slabs of 293 rows over 85 row lanes, so L = 4 + 85 and P = 1024 from the library's plan."""
    plan = ag.colsum_slabs_plan(COLSUM_CAPPED_M, 24)
    assert (plan["slabs"], plan["rows"], plan["row_lanes"], plan["chain"]) == (1024, 293, 85, 89)
    _colsum_against_float64(lib, COLSUM_CAPPED_M, 24)


def _colsum_against_float64(lib, M, N):
    dy = wb.random_rows(M, N + 8, 5)
    plan = ag.colsum_slabs_plan(M, N)
    want, mag = wb.colsum_reference(dy, N)
    got = run_colsum(lib, dy, N).double().numpy()
    tol = wb.bound(mag, plan)
    print(f"[colsum_slabs] M={M} N={N}: chain {plan['chain']}, partials {plan['partials']}: worst element at {(np.abs(got - want) / tol).max():.3f} of the bound")
    assert (np.abs(got - want) <= tol).all()


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument(lib):
    t = torch.zeros(2 * 8 * 8 * 136, dtype=torch.float16, device=DEV)
    dw = torch.zeros(128 * 136 * 9, dtype=torch.float32, device=DEV)
    ws = torch.zeros(1 << 20, dtype=torch.float32, device=DEV)
    big = ws.numel() * 4

    def call(Cx=32, Cy=32, Cout=32, Cin=32, k=3, stride=1, H=8, Ho=8, ws_bytes=big, x=t, dy=t, out=dw, w=ws):
        return lib.ldiff_op_conv_wgrad(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(out), 1, H, H, Cx, Ho, Ho, Cy, Cout, Cin, k, stride, 0, _lib.ptr(w), ws_bytes, sp())

    assert call() == 0
    for kw, name in [(dict(k=5), "k=5"), (dict(k=1, stride=2, Ho=4), "stride=2"), (dict(Cx=136, Cin=136), "Cx=136"), (dict(Cy=72, Cout=72), "Cy=72"),
                     (dict(Cout=33), "Cout=33"), (dict(Cin=33), "Cin=33"), (dict(ws_bytes=64), "ws_bytes=64"), (dict(x=None), "null argument x"),
                     (dict(dy=None), "null argument dy"), (dict(out=None), "null argument dw"), (dict(w=None), "null argument ws"), (dict(Ho=7), "Ho=7")]:
        assert call(**kw) == -1, kw
        assert name in lib.ldiff_last_error().decode(), (kw, lib.ldiff_last_error().decode())
    assert call(k=1, Cy=128, Cout=128) == 0, "Cy = 128 is accepted at k = 1"
    assert lib.ldiff_op_conv_wgrad_ws_bytes(1, 8, 8, 136, 32, 3, 0) == 0 and lib.ldiff_op_conv_wgrad_ws_bytes(1, 8, 8, 32, 72, 3, 0) == 0
    db = torch.zeros(64, dtype=torch.float32, device=DEV)
    for args, name in [((_lib.ptr(t), _lib.ptr(db), 16, 12, 16, _lib.ptr(ws), big), "N=12"), ((_lib.ptr(t), _lib.ptr(db), 16, 16, 8, _lib.ptr(ws), big), "ld=8"),
                       ((_lib.ptr(t), _lib.ptr(db), 16, 16, 16, _lib.ptr(ws), 8), "ws_bytes=8"), ((None, _lib.ptr(db), 16, 16, 16, _lib.ptr(ws), big), "null argument dy")]:
        assert lib.ldiff_op_colsum_slabs(*args, sp()) == -1
        assert name in lib.ldiff_last_error().decode()
    torch.cuda.synchronize()


# ---- 4. the route -----------------------------------------------------------------------------------------------------------------------------------
M_CAP = 2.0          # tests/test_gpu_nnunet_train.py
LOSS_SCALE = 1024.0
ROUTE_CASES = [("2d_reduced", 2, 64, 41), ("2d_reduced", 2, 32, 42)]   # that file's STEP_CASES, at slope 1.0
# Measured on the MI355X on the direct route (DESIGN.md section 7 "Tissue head, training"), per case: (worst ratio over the conv / transposed-conv / head weight
# tensors of max |g - g64| / max |g64| of the library to the fp16-storage model's, worst ratio of the absolute errors over the conv.bias tensors).
# Asserted: twice the measured ratio, at most M_CAP.
#   64^2: worst tensor decoder.stages.1.convs.1.conv.weight, library 6.246e-4 / model 4.200e-4 = 1.487; conv.bias encoder.stages.1.0.convs.1.conv.bias 1.037e-6 / 7.445e-7 = 1.393
#   32^2: worst tensor decoder.transpconvs.2.bias,            library 1.352e-3 / model 8.219e-4 = 1.645; conv.bias encoder.stages.2.0.convs.1.conv.bias 1.037e-6 / 8.252e-7 = 1.256
# Twice each ratio exceeds the cap, so the asserted factor is 2.0 in all four.
MEASURED_DIRECT = {("2d_reduced", 2, 64, 41): (1.487, 1.393), ("2d_reduced", 2, 32, 42): (1.645, 1.256)}
_cases = {}


def _is_contraction_param(name):
    return ".norm." not in name


def route_case(config, B, size, seed):
    key = (config, B, size, seed)
    if key not in _cases:
        with open(os.path.join(GOLDEN, "nnunet_plans_2d.json")) as f:
            plans = json.load(f)
        with open(os.path.join(GOLDEN, "nnunet_dataset.json")) as f:
            ds = json.load(f)
        spec = nnunet.network_spec(plans, config, ds)
        sd = ref.synthetic_state_dict(spec, seed)
        g = torch.Generator().manual_seed(seed + 100)
        x = F.avg_pool2d(torch.randn((B, 3, size + 4, size + 4), generator=g), 5, 1) * 2.2
        n_out = spec["n_stages"] - 1
        targets = ref.label_maps(B, spec["n_heads"], size, n_out, seed + 200)
        weights = nnunet_train.deep_supervision_weights(n_out)
        batch_dice = bool(plans["configurations"]["2d"]["batch_dice"])

        def backward(route):
            tr = nnunet_train.Trainer(spec, sd, batch_dice, 10, device=DEV, slope=1.0)

            def run():
                total = tr.loss(tr.network(x), [t.to(DEV) for t in targets], LOSS_SCALE)
                total.backward()

            if route is None:
                run()
            else:
                with ag.wgrad_route(route):
                    run()
            torch.cuda.synchronize()
            return {k: (None if p.grad is None else p.grad.detach().cpu()) for k, p in tr.network.p.items()}

        runs = {r: backward(r) for r in ("staged", "direct", "auto", None)}
        _, g64 = ref.step_gradients(sd, spec, x, targets, weights, batch_dice, 1.0)
        _, gmod = ref.step_gradients(sd, spec, x, targets, weights, batch_dice, 1.0, storage16=True, loss_scale=LOSS_SCALE)
        _cases.clear()
        _cases[key] = dict(runs=runs, f64=g64, model=gmod)
    return _cases[key]


@pytest.mark.parametrize("config,B,size,seed", ROUTE_CASES)
def test_trainer_auto_and_default_keep_the_staged_route(config, B, size, seed):
    """M <= 2 * 64^2 = 8192 < WGRAD_DIRECT_MIN_ROWS: under "auto" and with no route stated (the trainer's own "auto") every gradient is the staged route's, bit for bit."""
    runs = route_case(config, B, size, seed)["runs"]
    assert B * size * size < ag.WGRAD_DIRECT_MIN_ROWS
    for r in ("auto", None):
        for k, g in runs["staged"].items():
            assert (g is None and runs[r][k] is None) or torch.equal(runs[r][k], g), f"{k} under {r!r} differs from the staged route"


@pytest.mark.parametrize("config,B,size,seed", ROUTE_CASES)
def test_trainer_backward_on_the_direct_route(config, B, size, seed):
    """One backward pass under wgrad_route("direct"): the data gradient is untouched, so every norm parameter's gradient equals the staged run's bit for bit;
    every conv / transposed-conv / head weight and bias is graded as tests/test_gpu_nnunet_train.py grades the whole step at slope 1.0 -- the library's
    max |g - g64| / max |g64| (biases in front of an InstanceNorm: absolute error) against the fp16-storage model's, never against the staged route."""
    c = route_case(config, B, size, seed)
    direct, staged = c["runs"]["direct"], c["runs"]["staged"]
    rows, bias_rows, moved = [], [], 0
    for k, g64 in c["f64"].items():
        assert (g64 is None) == (direct[k] is None)
        if g64 is None:
            continue
        if not _is_contraction_param(k):
            assert torch.equal(direct[k], staged[k]), f"{k}: the direct route changed a gradient it does not compute"
            continue
        moved += int(not torch.equal(direct[k], staged[k]))
        gl, gm_ = direct[k].double() / LOSS_SCALE, c["model"][k]
        if k.endswith(".conv.bias"):
            bias_rows.append((k, (gl - g64).abs().max().item(), (gm_ - g64).abs().max().item()))
        else:
            rows.append((k, ((gl - g64).abs().max() / g64.abs().max()).item(), ((gm_ - g64).abs().max() / g64.abs().max()).item()))
    assert moved > 0, "the direct route produced the staged route's bits everywhere: it did not run"
    worst = max(rows, key=lambda r: r[1] / r[2])
    worst_b = max(bias_rows, key=lambda r: r[1] / r[2])
    print(f"[route] {config} B={B} {size}^2 direct: worst tensor {worst[0]}: lib {worst[1]:.3e} model {worst[2]:.3e} ratio {worst[1] / worst[2]:.3f}; conv.bias worst "
          f"{worst_b[0]}: lib {worst_b[1]:.3e} model {worst_b[2]:.3e} ratio {worst_b[1] / worst_b[2]:.3f}; {moved} tensors differ from the staged run")
    m, mb = (min(M_CAP, 2.0 * v) for v in MEASURED_DIRECT[(config, B, size, seed)])
    for k, e_lib, e_model in rows:
        assert e_lib <= m * e_model, f"{k}: library {e_lib:.3e}, fp16-storage model {e_model:.3e}: {e_lib / e_model:.2f} x (asserted {m:.2f} x)"
    for k, e_lib, e_model in bias_rows:
        assert e_lib <= mb * e_model, f"{k}: library {e_lib:.3e} absolute, fp16-storage model {e_model:.3e}: {e_lib / e_model:.2f} x (asserted {mb:.2f} x)"


def _staged_by_hand(lib, x, dy, weight):
    """The launches autograd.Conv2dFn.backward made before the route setting existed, for dw and db of a stride-1 conv with unpadded channel counts."""
    B, H, W, Cx = x.shape
    Cout, Cin, k, _ = weight.shape
    M, Kc = B * H * W, k * k * Cx
    dyT = torch.empty((Cout, M), dtype=torch.float16, device=DEV)
    _lib.check(lib.ldiff_op_transpose(dy.data_ptr(), dyT.data_ptr(), M, Cout, Cout, M, sp()))
    xcolT = torch.empty((Kc, M), dtype=torch.float16, device=DEV)
    _lib.check(lib.ldiff_op_im2col_t(x.data_ptr(), xcolT.data_ptr(), B, H, W, Cx, k, 1, k // 2, 0, H, W, M, sp()))
    g = ag._conv_call(dyT.view(1, 1, Cout, M), xcolT, Kc, 1, 1, 0, out_f32=True)
    dw = torch.empty(weight.shape, dtype=torch.float32, device=DEV)
    _lib.check(lib.ldiff_op_unpack_wgrad(g.data_ptr(), dw.data_ptr(), Cout, Cin, k, Cx, g.shape[-1], sp()))
    db = torch.empty(Cout, dtype=torch.float32, device=DEV)
    _lib.check(lib.ldiff_op_colsum(dy.data_ptr(), db.data_ptr(), M, Cout, Cout, sp()))
    return dw, db


def _conv_backward(x, dy, w, b, route):
    xg, wg, bg = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)

    def run():
        ag.Conv2dFn.apply(xg, wg, bg, 1, 0).backward(dy)

    if route is None:
        run()
    else:
        with ag.wgrad_route(route):
            run()
    torch.cuda.synchronize()
    return xg.grad, wg.grad, bg.grad


def test_conv2dfn_without_a_route_makes_the_staged_launches(lib):
    """A UNet-like shape (B 2, 8 x 8, 64 -> 64) with no route stated: dw and db are those of the transpose / im2col_t / GEMM / unpack / colsum launches, bit for
    bit; under "direct" the same node gives the direct kernels' values (different bits, same dx)."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn((2, 8, 8, 64), generator=g).to(torch.float16).to(DEV)
    dy = (0.1 * torch.randn((2, 8, 8, 64), generator=g)).to(torch.float16).to(DEV)
    w, b = (0.05 * torch.randn((64, 64, 3, 3), generator=g)).to(DEV), torch.zeros(64, device=DEV)
    dx0, dw0, db0 = _conv_backward(x, dy, w, b, None)
    dw_h, db_h = _staged_by_hand(lib, x, dy, w)
    torch.cuda.synchronize()
    assert torch.equal(dw0, dw_h) and torch.equal(db0, db_h)
    dx1, dw1, db1 = _conv_backward(x, dy, w, b, "direct")
    assert torch.equal(dx1, dx0) and not torch.equal(dw1, dw0)
    want, mag = wb.wgrad_reference(x.cpu().numpy(), dy.cpu().numpy(), 64, 64, 3, 1)
    plan = ag.wgrad_plan(2, 8, 8, 64, 64, 3, 0)
    assert (np.abs(dw1.double().cpu().numpy() - want) <= wb.bound(mag, plan)).all()


# ---- 5. crossover into the direct route under "auto" ------------------------------------------------------------------------------------------------
def test_auto_takes_the_direct_route_from_the_threshold_on(lib):
    """One Conv2dFn backward at M = 16384 rows (B 1, 128 x 128, 32 -> 32): "auto" equals "direct" bit for bit, and both lie within the bound of float64."""
    B, H, W, Cc = 1, 128, 128, 32
    assert B * H * W == 16384 >= ag.WGRAD_DIRECT_MIN_ROWS, "the threshold was raised: this case must move to the new crossover"
    xn, dyn = wb.random_case(B, H, W, Cc, Cc, 3, 1, 21)
    x, dy = torch.from_numpy(xn).to(DEV), torch.from_numpy(dyn).to(DEV)
    g = torch.Generator().manual_seed(4)
    w, b = (0.05 * torch.randn((Cc, Cc, 3, 3), generator=g)).to(DEV), torch.zeros(Cc, device=DEV)
    dxa, dwa, dba = _conv_backward(x, dy, w, b, "auto")
    dxd, dwd, dbd = _conv_backward(x, dy, w, b, "direct")
    dxs, dws, dbs = _conv_backward(x, dy, w, b, "staged")
    assert torch.equal(dwa, dwd) and torch.equal(dba, dbd) and torch.equal(dxa, dxd) and torch.equal(dxa, dxs)
    assert not torch.equal(dwa, dws), "auto stayed on the staged route at the threshold"
    want, mag = wb.wgrad_reference(xn, dyn, Cc, Cc, 3, 1)
    plan = ag.wgrad_plan(B, H, W, Cc, Cc, 3, 0)
    err = np.abs(dwa.double().cpu().numpy() - want)
    wantb, magb = wb.colsum_reference(dyn.reshape(-1, Cc), Cc)
    planb = ag.colsum_slabs_plan(B * H * W, Cc)
    errb = np.abs(dba.double().cpu().numpy() - wantb)
    print(f"[auto] dw at {(err / wb.bound(mag, plan)).max():.3f} of its bound (chain {plan['chain']}, partials {plan['partials']}), db at "
          f"{(errb / wb.bound(magb, planb)).max():.3f} (chain {planb['chain']}, partials {planb['partials']})")
    assert (err <= wb.bound(mag, plan)).all() and (errb <= wb.bound(magb, planb)).all()
