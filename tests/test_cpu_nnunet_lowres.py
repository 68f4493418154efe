"""CPU: the low-resolution simulation's rule and host side -- the float64 restatement of tests/nnunet_lowres_ref.py against scipy.ndimage.zoom (so the
GPU tests can use it without scipy), the integer index rule against scipy's own order-0 index, `lowres_shape`, `draw_sample`'s step 7, the wrong
variants the bounds must tell apart, and the new entry points' prototypes and refusals."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import scipy.ndimage as ndi

import nnunet_lowres_ref as lr
from ldiffusion_amd import _lib
from ldiffusion_amd import nnunet_data as nd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(32, 32), (30, 34), (27, 35), (16, 48)]
ZOOMS = [0.5, 0.53, 0.61, 0.75, 0.77, 0.9, 0.99]


def _scipy_zoom(x, shape, order):
    """skimage.transform.resize(order, mode='edge', anti_aliasing=False) as skimage >= 0.19 calls scipy; the zoom factors reproduce `shape`."""
    out = ndi.zoom(x, [shape[0] / x.shape[0], shape[1] / x.shape[1]], order=order, mode="nearest", grid_mode=True)
    assert out.shape == tuple(shape)
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_against_scipy_zoom(shape):
    x = lr.step_plane(*shape, seed=5).astype(np.float64)
    worst = 0.0
    for z in ZOOMS:
        m = lr.lowres_shape(*shape, z)
        if m == shape:
            assert not lr.is_on(*shape, z)
            continue
        down = _scipy_zoom(x, m, 0)
        d = x[np.ix_(lr.down_index(shape[0], m[0]), lr.down_index(shape[1], m[1]))]
        assert np.array_equal(down, d), (shape, z)   # none of these shapes meets one of scipy's tie indices (test_index_rule_against_scipy)
        want = np.clip(_scipy_zoom(d, shape, 3), d.min(), d.max())
        got, _ = lr.lowres(x, z)
        worst = max(worst, float(np.abs(got - want).max()))
    print(f"[lowres restatement {shape[0]}x{shape[1]}] worst |restatement - scipy| = {worst:.2e}")
    assert worst <= 1e-12


def test_index_rule_against_scipy():
    """floor((i + 1/2) n / m) in integers against the index scipy's order-0 zoom takes (read off by zooming arange(n)): every disagreement sits at an
    exact tie ((2 i + 1) n) % (2 m) == 0 and scipy's index is the rule's minus one; no more than 5 % of the (n, m) pairs disagree at all."""
    pairs = bad = 0
    for n in list(range(4, 130)) + [256, 384, 512, 602, 640]:
        ramp = np.arange(n, dtype=np.float64)
        for m in range((n + 1) // 2, n + 1):
            got = ndi.zoom(ramp, m / n, order=0, mode="nearest", grid_mode=True)
            if got.shape != (m,):
                continue   # scipy's own round(n * (m / n)) gave another length: not this pair's index
            rule = lr.down_index(n, m)
            diff = np.nonzero(got.astype(np.int64) != rule)[0]
            pairs += 1
            bad += len(diff) > 0
            assert (((2 * diff + 1) * n) % (2 * m) == 0).all(), (n, m, diff)
            assert (got.astype(np.int64)[diff] == rule[diff] - 1).all(), (n, m, diff)
    print(f"[lowres index rule] {bad} of {pairs} (n, m) pairs disagree with scipy, all at exact ties, by one")
    assert pairs > 5000 and bad <= 0.05 * pairs


def test_lowres_shape():
    for h, w in SHAPES + [(512, 512), (511, 3)]:
        for z in np.linspace(0.05, 1.0, 381, dtype=np.float32):
            want = (int(np.round(np.float32(h) * np.float32(z))), int(np.round(np.float32(w) * np.float32(z))))
            assert nd.lowres_shape((h, w), z) == want == lr.lowres_shape(h, w, z)
    assert nd.lowres_shape((5, 7), 0.5) == (2, 4)   # 2.5 -> 2, 3.5 -> 4: half to even
    assert not lr.is_on(32, 32, 0.0) and not lr.is_on(32, 32, 1.5) and not lr.is_on(32, 32, -1.0) and not lr.is_on(32, 32, float("nan"))
    assert not lr.is_on(32, 32, 0.99) and lr.is_on(64, 80, 0.99) and not lr.is_on(32, 32, 0.01) and lr.is_on(32, 32, 0.5)


def _case(rng, H, W):
    seg = np.zeros((H, W), np.int64)
    seg[H // 4:H // 2, W // 4:W // 2] = 1
    return rng.integers(0, 255, (3, H, W)).astype(np.uint8), seg


def test_draws():
    rng = np.random.default_rng(12)
    store = nd.CaseStore([_case(rng, 64, 64)], ["ZScoreNormalization"] * 3, 4, device="cpu")
    Cc = store.channels
    # the same generator state: the first six steps are byte-identical, and step 7 consumes exactly 1 + 2 C numbers more
    for idx in range(6):
        a, b = np.random.default_rng(40 + idx), np.random.default_rng(40 + idx)
        s0, c0, _ = nd.draw_sample(a, store, idx, 6, (32, 32))
        s1, c1, _ = nd.draw_sample(b, store, idx, 6, (32, 32), lowres=True)
        assert s0.tobytes() == s1.tobytes()
        c1z = c1.copy()
        c1z["lowres_zoom"] = 0
        assert c0.tobytes() == c1z.tobytes() and (c0["lowres_zoom"] == 0).all()
        a.random(1 + 2 * Cc)
        assert a.bit_generator.state == b.bit_generator.state
    n = 4096
    s, ch = nd.draw_batch(np.random.default_rng(13), store, n, (32, 32), lowres=True)
    s0, ch0 = nd.draw_batch(np.random.default_rng(13), store, 4, (32, 32))
    assert s0[0].tobytes() == s[0].tobytes() and (ch0["lowres_zoom"] == 0).all()

    def close(freq, p, count=n):
        return abs(freq - p) <= 5 * math.sqrt(p * (1 - p) / count)

    z = ch["lowres_zoom"]
    assert close((z > 0).any(1).mean(), 0.25 * (1 - 0.5 ** Cc)) and close((z > 0).mean(), 0.125, Cc * n)
    assert ((z[z > 0] >= 0.5) & (z[z > 0] <= 1.0)).all()
    _, chv = nd.draw_batch(np.random.default_rng(13), store, 64, (32, 32), train=False, lowres=True)
    assert (chv["lowres_zoom"] == 0).all()
    # train=False draws and drops them: the generator ends where the training draw of the same count ends
    a, b = np.random.default_rng(3), np.random.default_rng(3)
    nd.draw_sample(a, store, 0, 6, (32, 32), train=False, lowres=True)
    nd.draw_sample(b, store, 0, 6, (32, 32), train=False)
    b.random(1 + 2 * Cc)
    assert a.bit_generator.state == b.bit_generator.state
    assert (nd.P_LOWRES, nd.P_LOWRES_PER_CHANNEL, nd.LOWRES_ZOOM) == (0.25, 0.5, (0.5, 1.0))


def _far(a, b, bound):
    return int((np.abs(a - b) > 10 * bound).sum())


def test_wrong_variants_exceed_ten_times_the_bound():
    """Each wrong reading of the rule differs from the restatement by more than ten times the kernel's bound on at least 8 elements of a case, so a
    kernel inside the bound cannot be one of them."""
    cases = [(lr.step_plane(h, w, seed=7), z) for (h, w) in SHAPES + [(64, 80)] for z in (0.5, 0.53, 0.77)]
    for name, variant in (("order-1 up-sampling", dict(up_order=1)), ("mirror pad", dict(pad_mode="mirror")), ("non-grid centres", dict(grid=False))):
        counts = [_far(lr.lowres(x, z)[0], lr.lowres(x, z, **variant)[0], lr.lowres(x, z)[1]) for x, z in cases]
        print(f"[lowres variants] {name}: elements beyond 10 x bound per case {counts}")
        assert max(counts) >= 8, name
    x = lr.block_plane(32, 32)
    got, bound = lr.lowres(x, 0.77)
    raw, _ = lr.lowres(x, 0.77, clip=False)
    assert int((raw != got).sum()) >= 8, "the float64 reference itself must clip at least 8 elements"
    assert _far(got, raw, bound) >= 8, "missing clip"
    # the step placed after the gammas.  The chain's bound grows about fifty-fold per gamma (tests/nnunet_data_ref.gamma), so with both gammas on it
    # is too loose to tell the orders apart; the planes that carry contrast, the step and ONE gamma do (ORDER_ROWS, shared with the GPU test)
    for h, w in SHAPES:
        x = lr.step_plane(h, w, seed=7).astype(np.float64)
        for row in lr.ORDER_ROWS:
            ch = lr.chan_row(**row)
            want, bound = lr.chain(x, 0.0, None, ch)
            wrong, _ = lr.chain(x, 0.0, None, ch, lowres_after_gammas=True)
            assert _far(want, wrong, bound) >= 8, ("order", h, w, row)


def test_bound_holds_for_a_float32_run_of_the_same_recursion():
    """The prefilter's bound against a float32 numpy run of the serial recursion (what one thread of the kernel's axis-0 pass does), on both axes."""
    pole, x = np.float32(math.sqrt(3.0) - 2.0), lr.step_plane(40, 88, seed=3)
    c = x.copy()
    for axis in (0, 1):
        v = np.moveaxis(c, axis, 0)
        n = v.shape[0]
        pw = np.array([(math.sqrt(3.0) - 2.0) ** k for k in range(128)]).astype(np.float32)
        wgt = [pw[k] if (n > 64 or k == 0 or k == n - 1) else pw[k] + pw[2 * n - 2 - k] for k in range(min(n, 64))]
        acc = np.zeros(v.shape[1:], np.float32)
        for k, wk in enumerate(wgt):
            acc = acc + wk * v[k]
        cur = acc * (np.float32(6) if n > 64 else np.float32(6) / (np.float32(1) - pw[2 * n - 2]))
        v[0] = cur
        for k in range(1, n):
            v[k] = pole * v[k - 1] + np.float32(6) * v[k]
        v[n - 1] = np.float32(0.28867513459481288) * (pole * v[n - 2] + v[n - 1])
        for k in range(n - 2, -1, -1):
            v[k] = pole * (v[k + 1] - v[k])
    want, bound = lr.prefilter(x)
    ratio = float((np.abs(c.astype(np.float64) - want) / bound).max())
    print(f"[lowres prefilter, float32 numpy] worst error / bound = {ratio:.4f}")
    assert ratio <= 1


def test_prototypes_and_refusals():
    with open(os.path.join(ROOT, "include", "ldiff.h")) as f:
        header = f.read()
    kinds = {"int": C.c_int, "float": C.c_float, "int64_t": C.c_int64, "uint64_t": C.c_uint64}
    for name in ("ldiff_op_seg_intensity_lr_ws_bytes", "ldiff_op_seg_intensity_lr", "ldiff_op_spline_prefilter"):
        m = re.search(r"(\w+)\s+" + name + r"\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/ldiff.h"
        res, args = _lib.SIGNATURES[name]
        assert res is kinds[m.group(1)]
        want = [C.c_void_p if "*" in a else kinds[a.strip().split()[-2]] for a in m.group(2).split(",")]
        assert args == want, f"{name}: {args} against the header's {want}"
    lib = _lib.load()
    for name in ("ldiff_op_seg_intensity_lr_ws_bytes", "ldiff_op_seg_intensity_lr", "ldiff_op_spline_prefilter"):
        assert hasattr(lib, name)
    assert lib.ldiff_op_seg_intensity_lr_ws_bytes(12, 3, 512, 512) == 12 * 3 * 536 * 536 * 4 and lib.ldiff_op_seg_intensity_lr_ws_bytes(2, 3, 27, 35) == 2 * 3 * 51 * 59 * 4
    assert lib.ldiff_op_seg_intensity_lr_ws_bytes(0, 3, 8, 8) == 0
    assert lib.ldiff_op_seg_intensity_ws_bytes(12, 3, 512, 512) == 12 * 3 * 512 * 512 * 4   # the old formula is unchanged
    one = C.c_void_p(16)
    need = 2 * 3 * 56 * 56 * 4
    assert lib.ldiff_op_seg_intensity_lr(one, one, one, 2, 3, 32, 32, None, 0, one, need - 1, None) == -1
    assert b"ldiff_op_seg_intensity_lr_ws_bytes" in lib.ldiff_last_error()
    assert lib.ldiff_op_seg_intensity_lr(None, one, one, 2, 3, 32, 32, None, 0, one, need, None) == -1 and b"null" in lib.ldiff_last_error()
    for args, word in (((one, 2, 0, 8, 8), b"H"), ((one, 2, 8, 0, 8), b"W"), ((one, 2, 8, 8, 7), b"stride"), ((C.c_void_p(18), 2, 8, 8, 8), b"planes_f32"),
                       ((one, 2, 1 << 15, 1 << 15, 1 << 15), b"H * stride")):
        assert lib.ldiff_op_spline_prefilter(*args, None) == -1 and word in lib.ldiff_last_error(), (args[1:], lib.ldiff_last_error())
