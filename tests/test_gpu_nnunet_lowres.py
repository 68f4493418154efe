"""-m gpu: the low-resolution simulation on the device -- ldiff_op_spline_prefilter and ldiff_op_seg_intensity_lr against the float64 restatements of
tests/nnunet_lowres_ref.py (pinned to scipy by tests/test_cpu_nnunet_lowres.py) within the per-element bounds derived there, the old entry's behaviour
held, and the loader and store keywords.  The references are computed once per module and shared."""
import ctypes as C

import numpy as np
import pytest
import torch

import nnunet_data_ref as ref
import nnunet_lowres_ref as lr
from ldiffusion_amd import _lib
from ldiffusion_amd import nnunet_data as nd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(32, 32), (30, 34), (27, 35), (64, 80)]   # float4 walk; ditto, no power of two; scalar walk (945 elements); several loads per thread
ZOOMS = [0.5, 0.53, 0.77, 0.99, 0.0, 1.0]           # per plane of B = 2, C = 3; 0.99 is the identity below 51 samples, 1.0 always


def _planes(B, Cc, h, w, seed):
    return torch.from_numpy(np.stack([lr.step_plane(h, w, seed + i) for i in range(B * Cc)]).reshape(B, Cc, h, w))


def _tables(B, Cc, **columns):
    s = np.zeros(B, nd.SAMPLE_DTYPE)
    ch = np.zeros((B, Cc), nd.CHAN_DTYPE)
    ch["brightness"] = 1.0
    for key, v in columns.items():
        ch[key] = np.asarray(v, np.float32).reshape(B, Cc)
    return s, ch


def _run(x, s, ch, lowres=True, workspace=None):
    data = x.to(DEV).clone()
    s_dev, c_dev = nd.upload_tables(s, ch, DEV)
    nd.augment_intensity_(data, s_dev, c_dev, 0, workspace=workspace, lowres=lowres)
    torch.cuda.synchronize()
    return data.cpu()


# ---- 1. the prefilter alone ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(25, 25), (27, 35), (40, 56), (88, 70), (1, 40), (64, 65), (3, 700)])
def test_prefilter_against_spline_coefficients(shape):
    """Lines below the 64-sample horizon (the exact periodic start), at it, above it (the 64-term start and more than one chunk of the wave scan), a
    single row (axis 0 is then the identity), and rows of more than 320 samples (88 x 70 is below, 3 x 700 above), which do not stay in registers between the two passes."""
    H, W = shape
    x = _planes(1, 2, H, W, seed=11)[0]
    got = nd.spline_prefilter_(x.to(DEV).clone()).cpu()
    torch.cuda.synchronize()
    worst = 0.0
    for p in range(2):
        want, bound = lr.prefilter(x[p].numpy())
        err = np.abs(got[p].double().numpy() - want)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), f"plane {p}: worst error / bound {(err / bound).max():.3f}"
    print(f"[spline_prefilter {H}x{W}] worst measured / bound = {worst:.4f}")
    assert torch.equal(got, nd.spline_prefilter_(x.to(DEV).clone()).cpu()), "a second run must be bit-identical"


def test_prefilter_with_a_row_stride_and_its_refusals():
    H, W, stride = 27, 35, 41
    x = _planes(1, 2, H, W, seed=13)[0]
    buf = torch.full((2, H, stride), 7.0)
    buf[:, :, :W] = x
    dev = buf.to(DEV)
    nd.spline_prefilter_(dev[:, :, :W])
    torch.cuda.synchronize()
    got = dev.cpu()
    assert (got[:, :, W:] == 7.0).all(), "the columns between W and the stride are not touched"
    for p in range(2):
        want, bound = lr.prefilter(x[p].numpy())
        assert (np.abs(got[p, :, :W].double().numpy() - want) <= bound).all()
    lib = _lib.load()
    for args, word in (((2, 0, W, stride), b"H"), ((2, H, 0, stride), b"W"), ((2, H, W, W - 1), b"stride"), ((2, 1 << 15, 1 << 15, 1 << 15), b"H * stride")):
        assert lib.ldiff_op_spline_prefilter(_lib.ptr(dev), *args, None) == -1 and word in lib.ldiff_last_error()
    assert lib.ldiff_op_spline_prefilter(C.c_void_p(dev.data_ptr() + 2), 2, H, W, stride, None) == -1 and b"planes_f32" in lib.ldiff_last_error()
    with pytest.raises(ValueError, match="evenly spaced"):
        nd.spline_prefilter_(dev[:, ::2, :W])


# ---- 2. the step alone ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def step_runs():
    """One launch per shape, every other row off, and its float64 reference."""
    out = {}
    for h, w in SHAPES:
        x = _planes(2, 3, h, w, seed=300)
        s, ch = _tables(2, 3, lowres_zoom=ZOOMS)
        want = [[lr.lowres(x[b, c].numpy(), ch[b, c]["lowres_zoom"]) for c in range(3)] for b in range(2)]
        out[(h, w)] = (x, s, ch, _run(x, s, ch), want)
    return out


@pytest.mark.parametrize("patch", SHAPES)
def test_step_against_float64(step_runs, patch):
    x, s, ch, got, want = step_runs[patch]
    h, w = patch
    worst, on = 0.0, 0
    for b in range(2):
        for c in range(3):
            z = ch[b, c]["lowres_zoom"]
            if not lr.is_on(h, w, z):
                assert torch.equal(got[b, c], x[b, c]), f"plane ({b}, {c}), zoom {z}: off or the identity, must come back untouched"
                continue
            on += 1
            val, bound = want[b][c]
            err = np.abs(got[b, c].double().numpy() - val)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), f"plane ({b}, {c}), zoom {z}: worst error / bound {(err / bound).max():.3f}, max error {err.max():.3e}"
            assert not torch.equal(got[b, c], x[b, c])
    assert on == (4 if patch == (64, 80) else 3)
    print(f"[seg_intensity_lr step {h}x{w}] worst measured / bound = {worst:.4f} over {on} planes")


def test_zoom_out_of_range_leaves_the_plane_untouched():
    x = _planes(1, 3, 32, 32, seed=310)
    s, ch = _tables(1, 3, lowres_zoom=[1.5, -1.0, float("nan")])
    assert torch.equal(_run(x, s, ch), x)
    s, ch = _tables(1, 3, lowres_zoom=[0.01, 1.0, 0.0])   # an empty target (rint(0.32) = 0), the identity, off
    assert torch.equal(_run(x, s, ch), x)


def test_clip_bites_on_the_block_plane():
    """The input on which the float64 reference itself clips (tests/test_cpu_nnunet_lowres.py): the kernel stays inside the bound of the clipped rule."""
    x = torch.from_numpy(lr.block_plane(32, 32))[None, None]
    s, ch = _tables(1, 1, lowres_zoom=[0.77])
    got = _run(x, s, ch)[0, 0].double().numpy()
    want, bound = lr.lowres(x[0, 0].numpy(), np.float32(0.77))
    raw, _ = lr.lowres(x[0, 0].numpy(), np.float32(0.77), clip=False)
    assert (np.abs(got - want) <= bound).all() and int((np.abs(got - raw) > 10 * bound).sum()) >= 8
    assert got.max() <= 3.0 and got.min() >= -2.0


# ---- 3. in the chain -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("patch", SHAPES)
def test_chain_against_float64(patch):
    """Contrast + the step + both gammas on the first sample's planes, within the chain's own (loose: about fifty-fold per gamma) bound; the second
    sample's planes carry contrast, the step and ONE gamma (ORDER_ROWS), where the bound is tight enough to reject the step placed after the gammas."""
    h, w = patch
    x = _planes(2, 3, h, w, seed=320)
    s, ch = _tables(2, 3, contrast=[0.75, 1.25, 0.9, 0, 0, 0], lowres_zoom=[0.5, 0.53, 0.77, 0, 0, 0], gamma_inverted=[0.7, 1.5, 0.85, 0, 0, 0],
                    gamma=[1.5, 0.7, 1.3, 0, 0, 0])
    for c, row in enumerate(lr.ORDER_ROWS):
        ch[1, c] = lr.chan_row(**row)
    got = _run(x, s, ch)
    worst = 0.0
    for b in range(2):
        for c in range(3):
            want, bound = lr.chain(x[b, c].double().numpy(), 0.0, None, ch[b, c])
            g = got[b, c].double().numpy()
            err = np.abs(g - want)
            worst = max(worst, float((err / bound).max()))
            assert np.isfinite(g).all() and (err <= bound).all(), f"plane ({b}, {c}): worst error / bound {(err / bound).max():.3f}"
            wrong, _ = lr.chain(x[b, c].double().numpy(), 0.0, None, ch[b, c], lowres_after_gammas=True)
            if b == 1:
                assert int((np.abs(g - wrong) > 10 * bound).sum()) >= 8, f"plane ({b}, {c}): the step placed after the gammas is not told apart"
            else:
                assert np.abs(g - want).max() < 0.1 * np.abs(g - wrong).max()
    print(f"[seg_intensity_lr chain {h}x{w}] worst measured / bound = {worst:.4f}")


# ---- 4.-6. old behaviour, replay, workspace ------------------------------------------------------------------------------------------------------
def test_old_entry_does_not_read_the_slot_and_lr_with_zeros_is_the_old_entry():
    x, z = _planes(2, 3, 30, 34, seed=330), torch.randn((2, 3, 30, 34), generator=torch.Generator().manual_seed(1))
    s, ch = _tables(2, 3, blur_sigma=[0.5, 0.73, 1.0, 0.61, 0.95, 0], contrast=[0.75, 1.25, 0.9, 1.1, 0.8, 0], gamma_inverted=[0.7, 1.5, 0.85, 1.2, 0.95, 0],
                    gamma=[1.5, 0.7, 1.3, 0.8, 1.05, 0], brightness=[0.75, 1.25, 0.9, 1.1, 0.8, 1.0])
    s["noise_sigma"] = [0.1, 0.037]

    def run(table, lowres):
        data = x.to(DEV).clone()
        s_dev, c_dev = nd.upload_tables(s, table, DEV)
        nd.augment_intensity_(data, s_dev, c_dev, 0, normal=z.to(DEV), lowres=lowres)
        torch.cuda.synchronize()
        return data.cpu()

    with_zoom = ch.copy()
    with_zoom["lowres_zoom"] = np.asarray(ZOOMS[:3] + [0.61, 0.9, 0.5], np.float32).reshape(2, 3)
    old = run(ch, False)
    assert torch.equal(run(with_zoom, False), old), "ldiff_op_seg_intensity must not read lowres_zoom"
    assert torch.equal(run(ch, True), old), "ldiff_op_seg_intensity_lr with the column zero must be ldiff_op_seg_intensity"
    both = run(with_zoom, True)
    assert not torch.equal(both, old)
    assert torch.equal(both, run(with_zoom, True)), "a replay must be bit-identical"


def test_replay_is_bit_identical(step_runs):
    for patch in SHAPES:
        x, s, ch, got, _ = step_runs[patch]
        assert torch.equal(_run(x, s, ch), got)


def test_workspace_one_byte_short_is_refused():
    B, Cc, h, w = 2, 3, 27, 35
    need = int(_lib.load().ldiff_op_seg_intensity_lr_ws_bytes(B, Cc, h, w))
    assert need == B * Cc * (h + 24) * (w + 24) * 4
    x = _planes(B, Cc, h, w, seed=340).to(DEV)
    s, ch = _tables(B, Cc, lowres_zoom=ZOOMS)
    s_dev, c_dev = nd.upload_tables(s, ch, DEV)
    ws = torch.empty(need - 1, dtype=torch.uint8, device=DEV)
    lib = _lib.load()
    rc = lib.ldiff_op_seg_intensity_lr(_lib.ptr(x), _lib.ptr(s_dev), _lib.ptr(c_dev), B, Cc, h, w, None, 0, _lib.ptr(ws), need - 1, _lib.stream_ptr())
    assert rc == -1 and b"ldiff_op_seg_intensity_lr_ws_bytes" in lib.ldiff_last_error()
    # the wrapper replaces a workspace that is too small (one sized for the old entry) by one of the right size
    small = torch.empty(int(lib.ldiff_op_seg_intensity_ws_bytes(B, Cc, h, w)), dtype=torch.uint8, device=DEV)
    assert torch.equal(_run(x.cpu(), s, ch, workspace=small), _run(x.cpu(), s, ch))


# ---- 7. loader and store -------------------------------------------------------------------------------------------------------------------------
def _cases(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for H, W in shapes:
        img = (torch.nn.functional.avg_pool2d(torch.randn((1, 3, H + 2, W + 2), generator=g), 3, 1)[0] * 60 + 120).clamp(0, 255)
        seg = np.zeros((H, W), np.int64)
        seg[H // 4:H // 2, W // 4:W // 2], seg[H // 2:, W // 2:] = 1, 2
        out.append((img.float(), seg))
    return out


SCHEMES = ["ZScoreNormalization", "RescaleTo01Normalization", "NoNormalization"]


@pytest.fixture(scope="module")
def stores():
    cases = _cases([(40, 56), (33, 47), (70, 66)], 100)
    return nd.CaseStore(cases, SCHEMES, 4, DEV), nd.CaseStore(cases, SCHEMES, 4, DEV, prefilter="device")


def test_drawn_tables_through_the_lr_entry():
    B = 8
    seg = np.zeros((40, 56), np.int64)
    seg[10:20, 10:30] = 1
    store = nd.CaseStore([(np.random.default_rng(0).integers(0, 255, (3, 40, 56)).astype(np.uint8), seg)], SCHEMES, 4, device="cpu")
    s, ch = nd.draw_batch(np.random.default_rng(12), store, B, (32, 32), lowres=True)
    on = np.array([[lr.is_on(32, 32, ch[b, c]["lowres_zoom"]) for c in range(3)] for b in range(B)])
    assert on.sum() >= 3 and (ch["lowres_zoom"] > 0).sum() > on.sum(), "the seed's table carries rows that are on and one that is the identity"
    x = _planes(B, 3, 32, 32, seed=350)
    got = _run(x, s, ch)
    zeroed = ch.copy()
    zeroed["lowres_zoom"] = 0
    base = _run(x, s, zeroed)
    assert torch.isfinite(got).all()
    for b in range(B):
        for c in range(3):
            assert torch.equal(got[b, c], base[b, c]) != bool(on[b, c]), (b, c, ch[b, c]["lowres_zoom"])


def test_loaders_with_lowres_agree_under_one_seed(stores):
    la, lb = nd.PatchLoader(stores[0], (32, 32), 6, 3, seed=5, lowres=True), nd.PatchLoader(stores[0], (32, 32), 6, 3, seed=5, lowres=True)
    rng, drawn = np.random.default_rng(5), 0
    for _ in range(3):
        a, b = next(la), next(lb)
        drawn += int((nd.draw_batch(rng, stores[0], 6, (32, 32), lowres=True)[1]["lowres_zoom"] > 0).sum())
        assert a["data"].shape == (6, 3, 32, 32) and torch.isfinite(a["data"]).all()
        assert torch.equal(a["data"], b["data"]) and all(torch.equal(p, q) for p, q in zip(a["target"], b["target"]))
    assert drawn >= 1, "the seed's three batches carry the step at least once"


def test_store_prefiltered_on_the_device(stores):
    host, dev = stores
    worst = 0.0
    for i in range(len(host)):
        assert torch.equal(host.raw(i), dev.raw(i)) and torch.equal(host.labels(i), dev.labels(i))
        raw = host.raw(i).cpu().numpy()
        for c in range(3):
            want, bound = lr.prefilter(raw[c])
            err = np.abs(dev.coefficients(i)[c].double().cpu().numpy() - want)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all()
            # the host store's coefficients are `want` rounded once to float32
            assert (np.abs(dev.coefficients(i)[c].double().cpu().numpy() - host.coefficients(i)[c].double().cpu().numpy()) <= bound + ref.U * np.abs(want)).all()
    print(f"[CaseStore prefilter='device'] worst measured / bound = {worst:.4f}")
    with pytest.raises(ValueError, match="needs the store on a GPU"):
        nd.CaseStore(_cases([(24, 24)], 1), SCHEMES, 4, "cpu", prefilter="device")
