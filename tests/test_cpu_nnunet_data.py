"""CPU: the host side of the tissue head's training data (ldiffusion_amd.nnunet_data) -- the float64 restatements of tests/nnunet_data_ref.py against
scipy (so the GPU tests can use them without it), `class_locations` against a fixture recorded from the reference's own `_sample_foreground_locations`
(tests/golden/nnunet_class_locations.npz, scripts/gen_golden_nnunet_data.py), `draw_batch`'s crop rules and distributions, and the prototypes of the new
entry points."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

import nnunet_data_ref as ref
from ldiffusion_amd import _lib
from ldiffusion_amd import nnunet_data as nd

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEMES = ["ZScoreNormalization"] * 3


def _windows(h, w):
    """Four rotated / scaled / mirrored windows over a 40 x 56 image, from inside it to mostly outside."""
    out = []
    for angle, zoom, flip, centre in ((0.4, 0.8, (False, False), (20.0, 28.0)), (-2.1, 1.3, (True, False), (5.0, 50.0)), (1.0, 1.0, (False, True), (38.0, 3.0)),
                                      (3.0, 0.71, (True, True), (-6.0, 60.0))):
        bbox = [centre[0] - (h - 1) / 2.0, centre[1] - (w - 1) / 2.0]
        m, copy = nd.spatial_matrix((h, w), (h, w), bbox, angle, zoom, flip, modified=True)
        assert copy == 0
        out.append(m)
    return out


def test_cubic_sampler_and_prefilter_against_scipy():
    rng = np.random.default_rng(0)
    img = rng.standard_normal((2, 40, 56))
    coef = nd.spline_coefficients(img)
    want = np.stack([ndi.spline_filter(img[c], order=3, mode="mirror") for c in range(2)])
    assert np.abs(coef - want).max() <= 1e-13
    outside = []
    for m in _windows(24, 30):
        y, x, _, _ = ref.coordinates(m, 24, 30)
        got, _, _ = ref.cubic_sample(want, y, x)
        for c in range(2):
            exp = ndi.map_coordinates(img[c], [y, x], order=3, mode="constant", cval=0.0)
            assert np.abs(got[c] - exp).max() <= 1e-13, np.abs(got[c] - exp).max()
        outside.append(float(((y < 0) | (y > 39) | (x < 0) | (x > 55)).mean()))
    assert min(outside) == 0.0 and max(outside) > 0.5, outside


def test_small_axes_of_the_prefilter():
    rng = np.random.default_rng(1)
    for n in (2, 3, 5, 70):
        img = rng.standard_normal((n, 4))
        assert np.abs(nd.spline_coefficients(img[None])[0] - ndi.spline_filter(img, order=3, mode="mirror")).max() <= 1e-13


@pytest.mark.parametrize("sigma", [0.5, 0.62, 0.874, 1.0])
def test_blur_against_gaussian_filter(sigma):
    rng = np.random.default_rng(2)
    x = rng.standard_normal((30, 34))
    got, _ = ref.blur(x, np.float32(sigma))
    assert np.abs(got - ndi.gaussian_filter(x, float(np.float32(sigma)))).max() <= 1e-14


def test_target_indices_against_zoom():
    for n in (32, 64, 96):
        base = np.arange(n, dtype=np.float64)
        for k in (1, 2, 3):
            want = ndi.zoom(base, 0.5 ** k, order=0, mode="nearest", grid_mode=True)
            assert np.array_equal(ref.ds_indices(k, n), want.astype(np.int64)), (n, k)
    assert list(ref.ds_indices(1, 8)) == [1, 3, 5, 7] and list(ref.ds_indices(2, 16)) == [2, 6, 10, 14] and list(ref.ds_indices(3, 16)) == [4, 12]
    assert list(ref.ds_indices(0, 4)) == [0, 1, 2, 3]


def test_label_vote_is_per_label_linear_interpolation():
    """The restatement against scipy's order-1 interpolation of each indicator, as interpolate_img(is_seg=True) runs it."""
    rng = np.random.default_rng(3)
    seg = (rng.random((40, 56)) * 4).astype(np.uint8)
    seg[10:30, 10:40] = 2
    for m in _windows(24, 30):
        y, x, _, _ = ref.coordinates(m, 24, 30)
        got, _ = ref.vote_labels(seg, y, x, 4)
        want = np.zeros(y.shape, np.uint8)
        for c in range(4):
            want[ndi.map_coordinates((seg == c).astype(np.float64), [y, x], order=1, mode="constant", cval=0.0) >= 0.5] = c
        inside = (y >= 0) & (y <= 39) & (x >= 0) & (x <= 55)
        assert np.array_equal(got[inside], want[inside]) and not got[~inside].any()


def test_patch_size_rules():
    assert nd.initial_patch_size((512, 512)) == (602, 602)      # 512 / 0.85
    assert nd.initial_patch_size((32, 32)) == (37, 37)
    assert nd.rotation_range((512, 512)) == math.pi and nd.rotation_range((64, 96)) == math.pi
    r = nd.rotation_range((64, 128))
    assert r == 15.0 / 360 * 2 * np.pi
    want = np.maximum(np.abs(nd.rotate_coords_2d(np.array([64.0, 128.0]), r)), [64, 128]) / 0.85
    assert nd.initial_patch_size((64, 128)) == tuple(int(v) for v in want)
    assert np.allclose(nd.rotate_coords_2d(np.array([1.0, 0.0]), math.pi / 2), [0.0, -1.0], atol=1e-15)
    with pytest.raises(ValueError):
        nd.rotation_range((8, 8, 8))


def test_class_locations_against_the_reference_fixture():
    g = np.load(os.path.join(GOLDEN, "nnunet_class_locations.npz"))
    seg = g["seg"]
    assert seg.shape == (48, 48) and list(g["classes"]) == [1, 2, 3] and len(g["locations_2"]) == 0
    got = nd.sample_foreground_locations(seg, [1, 2, 3])
    for c in (1, 3):
        assert np.array_equal(got[c], g[f"locations_{c}"][:, 2:]) and len(got[c]) == int((seg == c).sum())
    assert len(got[2]) == 0
    store = nd.CaseStore([(np.zeros((3, 48, 48), np.uint8), seg)], SCHEMES, 4, device="cpu")
    assert all(np.array_equal(np.asarray(store.class_locations[0][c]).reshape(-1, 2), g[f"locations_{c}"][:, 2:]) for c in (1, 2, 3))
    # the cap and the floor
    assert [nd._target_num_samples(n) for n in (1, 9999, 10000, 10001, 1000000, 1000001, 2500000)] == [1, 9999, 10000, 10000, 10000, 10001, 25000]


def _case(rng, H, W, C=3, fg=True):
    img = (rng.random((C, H, W)) * 255).astype(np.uint8)
    seg = np.zeros((H, W), np.uint8)
    if fg:
        seg[H // 4:H // 2, W // 3:W // 2] = 1
        seg[H // 2:, : W // 4] = 3
    return img, seg


def test_case_store_refusals_and_layout():
    rng = np.random.default_rng(4)
    img, seg = _case(rng, 20, 24)
    with pytest.raises(ValueError, match=r"labels \[5\] outside \[0, 4\)"):
        nd.CaseStore([(img, np.where(seg == 3, 5, seg))], SCHEMES, 4, device="cpu")
    with pytest.raises(ValueError, match="regions"):
        nd.CaseStore([(img, seg)], SCHEMES, 4, device="cpu", labels={"background": 0, "whole": [1, 2]})
    with pytest.raises(ValueError, match="ignore"):
        nd.CaseStore([(img, seg)], SCHEMES, 4, device="cpu", labels={"background": 0, "a": 1, "ignore": 2})
    img2, seg2 = _case(rng, 33, 47)
    store = nd.CaseStore([(img, seg), (torch.from_numpy(img2).float(), torch.from_numpy(seg2).long())], SCHEMES, 4, device="cpu")
    assert len(store) == 2 and store.shape(1) == (33, 47) and store.table.dtype.itemsize == C.sizeof(_lib.SegCase)
    assert all(int(store.table[i][k]) % 16 == 0 for i in range(2) for k in ("coef_off", "raw_off", "label_off"))
    from ldiffusion_amd import nnunet
    assert torch.equal(store.raw(1), nnunet.normalize(torch.from_numpy(img2).float(), SCHEMES))
    assert torch.equal(store.labels(1), torch.from_numpy(seg2))
    want = ndi.spline_filter(store.raw(1)[2].double().numpy(), order=3, mode="mirror")
    assert np.abs(store.coefficients(1)[2].double().numpy() - want).max() <= 2 * ref.U * np.abs(want).max()


def test_table_dtypes_match_the_c_structs():
    for dt, st in ((nd.CASE_DTYPE, _lib.SegCase), (nd.SAMPLE_DTYPE, _lib.SegSample), (nd.CHAN_DTYPE, _lib.SegChan)):
        assert dt.itemsize == C.sizeof(st)
        assert [(n, dt.fields[n][1]) for n in dt.names] == [(n, getattr(st, n).offset) for n, _ in st._fields_]
    with open(os.path.join(ROOT, "include", "ldiff.h")) as f:
        header = f.read()
    for name, dt in (("ldiff_seg_case", nd.CASE_DTYPE), ("ldiff_seg_sample", nd.SAMPLE_DTYPE), ("ldiff_seg_chan", nd.CHAN_DTYPE)):
        body = re.search(r"typedef struct " + name + r"\s*{([^}]*)}\s*" + name + r"\s*;", header).group(1)
        fields = [re.sub(r"\[\d+\]", "", f.strip()) for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
        assert fields == list(dt.names), (name, fields)


FLIPS = [(False, False), (True, False), (False, True), (True, True)]


@pytest.mark.parametrize("patch,loader_patch", [((32, 32), (37, 37)), ((30, 34), (35, 40)), ((32, 32), (32, 32)), ((16, 48), (19, 56))])
def test_spatial_matrix_against_the_restatement(patch, loader_patch):
    """`spatial_matrix` reproduces the coordinates of the matrix-free restatement (grid, rotation, scale, centre, np.flip): square and non-square
    patches, a loader patch larger by an odd and an even amount, all four mirror combinations, rotation alone, scale alone and both.  A float32 matrix
    entry carries 2^-24 of its size: 1e-5 of a pixel at these coordinates (below 128)."""
    h, w = patch
    for bbox in ((-3, 5), (11, -7)):
        for angle, zoom in ((0.7, 1.0), (-2.6, 1.0), (0.0, 0.73), (0.0, 1.38), (1.9, 0.81), (-0.4, 1.3)):
            for flip in FLIPS:
                m, copy = nd.spatial_matrix(patch, loader_patch, bbox, angle, zoom, flip, modified=True)
                assert copy == 0 and m.dtype == np.float32
                y, x, _, _ = ref.coordinates(m, h, w)
                wy, wx = ref.spatial_coordinates(patch, loader_patch, bbox, angle, zoom, flip)
                assert np.abs(y - wy).max() <= 1e-5 and np.abs(x - wx).max() <= 1e-5, (bbox, angle, zoom, flip, np.abs(y - wy).max(), np.abs(x - wx).max())
        for flip in FLIPS:   # the copy-mode matrix: np.flip of the integer centre crop, exactly
            m, copy = nd.spatial_matrix(patch, loader_patch, bbox, 0.0, 1.0, flip, modified=False)
            assert copy == 1
            y, x, _, _ = ref.coordinates(m, h, w)
            wy, wx = ref.centre_crop_coordinates(patch, loader_patch, bbox, flip)
            assert np.array_equal(y, wy) and np.array_equal(x, wx), (bbox, flip)
            assert m[1] == 0 and m[3] == 0 and abs(m[0]) == 1 and abs(m[4]) == 1 and all(float(v).is_integer() for v in m)
    # the restatement tells a shifted centre, a reversed rotation and a swapped mirror axis apart
    base = ref.spatial_coordinates(patch, loader_patch, (0, 0), 0.7, 0.9, (True, False))
    for other in (ref.spatial_coordinates(patch, loader_patch, (0, 0), -0.7, 0.9, (True, False)), ref.spatial_coordinates(patch, loader_patch, (0, 0), 0.7, 0.9, (False, True))):
        assert np.abs(base[0] - other[0]).max() > 1


def test_draw_batch_matrices_are_the_restatement():
    """The matrices draw_batch emits, from its own draws: the 2 x 2 part gives angle, scale and mirrors back, and with the crop of `draw_sample` the
    restatement gives every coordinate."""
    rng = np.random.default_rng(20)
    store = nd.CaseStore([_case(rng, 40, 56), _case(rng, 24, 24)], SCHEMES, 4, device="cpu")
    g = np.random.default_rng(21)
    patch, loader_patch, seen = (30, 34), nd.initial_patch_size((30, 34)), 0
    for b in range(200):
        s, _, crop = nd.draw_sample(g, store, b % 12, 12, patch)
        m = s["m"].astype(np.float64)
        y, x, _, _ = ref.coordinates(s["m"], *patch)
        lin = m[[0, 1, 3, 4]].reshape(2, 2)
        if s["copy"]:
            flip = (m[0] < 0, m[4] < 0)
            wy, wx = ref.centre_crop_coordinates(patch, loader_patch, crop["bbox_lbs"], flip)
            assert np.array_equal(y, wy) and np.array_equal(x, wx)
            continue
        # undo the mirrors by trying the four combinations: exactly one reproduces a rotation times a positive scale
        hits = 0
        for flip in FLIPS:
            a = lin * np.array([-1.0 if flip[0] else 1.0, -1.0 if flip[1] else 1.0])[None, :]
            if np.linalg.det(a) <= 0 or abs(a[0, 0] - a[1, 1]) > 1e-6 or abs(a[0, 1] + a[1, 0]) > 1e-6:
                continue
            zoom, angle = math.sqrt(np.linalg.det(a)), math.atan2(a[0, 1], a[0, 0])
            wy, wx = ref.spatial_coordinates(patch, loader_patch, crop["bbox_lbs"], angle, zoom, flip)
            hits += bool(np.abs(y - wy).max() <= 1e-4 and np.abs(x - wx).max() <= 1e-4)
        assert hits >= 1, (b, m)
        seen += 1
    assert seen > 40


def test_crop_bounds_are_get_bbox():
    """lbs / ubs of base_data_loader.py:68-80 for a case larger than, equal to and smaller than the loader's patch (37 for a 32 patch: need_to_pad 5)."""
    assert nd.crop_bounds((40, 56), (37, 37), (32, 32)) == ([-3, -3], [40 + 2 + 1 - 37, 56 + 2 + 1 - 37])
    assert nd.crop_bounds((37, 37), (37, 37), (32, 32)) == ([-3, -3], [3, 3])
    assert nd.crop_bounds((24, 24), (37, 37), (32, 32)) == ([-7, -7], [24 + 6 + 1 - 37, 24 + 6 + 1 - 37])   # need_to_pad widened to 13
    assert nd.crop_bounds((40, 24), (32, 32), (32, 32)) == ([0, -4], [8, -4])                               # validation: need_to_pad 0


def test_forced_foreground_rule_and_windows():
    rng = np.random.default_rng(5)
    store = nd.CaseStore([_case(rng, 40, 56), _case(rng, 33, 47), _case(rng, 24, 24), _case(rng, 50, 50, fg=False)], SCHEMES, 4, device="cpu")
    B = 12
    assert [nd.do_oversample(i, B, 0.33) for i in range(B)] == [i >= round(B * 0.67) for i in range(B)]
    assert [nd.do_oversample(i, 2, 0.33) for i in range(2)] == [False, True]
    g = np.random.default_rng(6)
    checked = fallback = 0
    for _ in range(40):
        rows = [nd.draw_sample(g, store, b, B, (32, 32)) for b in range(B)]
        for b, (s, ch, t) in enumerate(rows):
            assert s.dtype == nd.SAMPLE_DTYPE and ch.shape == (3,) and s["case_index"] == t["case"]
            assert t["forced"] == (b >= round(B * 0.67)) and t["loader_patch"] == (37, 37)
            H, W = store.shape(t["case"])
            assert t["lbs"] == nd.crop_bounds((H, W), (37, 37), (32, 32))[0]
            if t["voxel"] is None:
                assert all(t["lbs"][d] <= t["bbox_lbs"][d] <= t["ubs"][d] for d in range(2))
                fallback += t["forced"]
                assert not t["forced"] or t["case"] == 3
                continue
            assert t["forced"] and t["case"] != 3
            assert store.labels(t["case"])[t["voxel"][0], t["voxel"][1]] != 0
            assert t["bbox_lbs"] == [max(t["lbs"][d], t["voxel"][d] - 37 // 2) for d in range(2)]
            if s["copy"]:
                # an unmodified forced sample: the 32-window inside the loader's 37-crop holds the chosen voxel
                m = s["m"].astype(np.float64)
                ys, xs = sorted((m[2], m[0] * 31 + m[2])), sorted((m[5], m[4] * 31 + m[5]))
                assert ys[0] <= t["voxel"][0] <= ys[1] and xs[0] <= t["voxel"][1] <= xs[1]
                checked += 1
    assert checked > 20 and fallback > 5


def test_validation_draw_is_an_exact_crop():
    rng = np.random.default_rng(7)
    store = nd.CaseStore([_case(rng, 40, 56), _case(rng, 24, 24)], SCHEMES, 4, device="cpu")
    samples, chans = nd.draw_batch(np.random.default_rng(8), store, 64, (32, 32), train=False)
    assert (samples["copy"] == 1).all() and (samples["noise_sigma"] == 0).all()
    for name in ("blur_sigma", "contrast", "gamma_inverted", "gamma", "lowres_zoom"):
        assert (chans[name] == 0).all()
    assert (chans["brightness"] == 1).all()
    g = np.random.default_rng(8)   # draw_batch is draw_sample, sample after sample
    for b, s in enumerate(samples):
        s2, ch2, t = nd.draw_sample(g, store, b, 64, (32, 32), train=False)
        assert s2.tobytes() == s.tobytes() and ch2.tobytes() == chans[b].tobytes()
        assert t["loader_patch"] == (32, 32) and list(s["m"]) == [1, 0, t["bbox_lbs"][0], 0, 1, t["bbox_lbs"][1]]
        H, W = store.shape(t["case"])
        assert all(lb == min(0, -((32 - n) // 2)) for lb, n in zip(t["lbs"], (H, W)))


def test_draw_batch_is_deterministic_under_the_seed():
    rng = np.random.default_rng(9)
    store = nd.CaseStore([_case(rng, 40, 56), _case(rng, 24, 24)], SCHEMES, 4, device="cpu")
    a = nd.draw_batch(np.random.default_rng(10), store, 8, (32, 32))
    b = nd.draw_batch(np.random.default_rng(10), store, 8, (32, 32))
    c = nd.draw_batch(np.random.default_rng(11), store, 8, (32, 32))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[0].tobytes() != c[0].tobytes()


def test_distributions_over_4096_draws():
    """Ranges, and each transform's frequency within 5 sqrt(p (1 - p) / n) of its p (the binomial's margin; deterministic under the seed)."""
    rng = np.random.default_rng(12)
    store = nd.CaseStore([_case(rng, 64, 64)], SCHEMES, 4, device="cpu")
    n = 4096
    s, ch = nd.draw_batch(np.random.default_rng(13), store, n, (32, 32))

    def close(freq, p, count=n):
        return abs(freq - p) <= 5 * math.sqrt(p * (1 - p) / count)

    m = s["m"].astype(np.float64)
    lin = m[:, [0, 1, 3, 4]].reshape(n, 2, 2)
    zoom = np.sqrt(np.abs(np.linalg.det(lin)))
    modified = s["copy"] == 0
    assert close(modified.mean(), 1 - 0.8 * 0.8)
    assert (zoom[modified] >= 0.7 - 1e-6).all() and (zoom[modified] <= 1.4 + 1e-6).all()
    scaled = np.abs(zoom - 1) > 1e-6
    assert close(scaled.mean(), 0.2) and close((zoom[scaled] < 1).mean(), 0.5, scaled.sum())
    rotated = modified & (np.abs(lin[:, 0, 1]) > 1e-7)
    assert close(rotated.mean(), 0.2)
    assert np.allclose(np.einsum("nij,nkj->nik", lin, lin), (zoom ** 2)[:, None, None] * np.eye(2), atol=1e-5)   # a rotation (and flips) times the scale
    assert close((np.linalg.det(lin) < 0).mean(), 0.5)            # exactly one axis mirrored
    assert close((lin[:, 0, 0] < 0)[~rotated].mean(), 0.5, (~rotated).sum())
    assert (s["copy"][~modified] == 1).all() and (np.abs(m[~modified][:, [2, 5]] % 1) == 0).all()
    sig = s["noise_sigma"]
    assert close((sig > 0).mean(), 0.1) and sig.max() <= 0.1 and sig.min() >= 0
    assert len(np.unique(s["philox_offset"])) == n
    blur = ch["blur_sigma"]
    assert close((blur > 0).any(1).mean(), 0.2 * (1 - 0.5 ** 3)) and close((blur > 0).mean(), 0.1, 3 * n)
    assert ((blur[blur > 0] >= 0.5) & (blur[blur > 0] <= 1.0)).all()
    br = ch["brightness"]
    assert close((br != 1).all(1).mean(), 0.15) and ((br >= 0.75) & (br <= 1.25)).all() and ((br != 1).all(1) == (br != 1).any(1)).all()
    for name, p, lo, hi in (("contrast", 0.15, 0.75, 1.25), ("gamma_inverted", 0.1, 0.7, 1.5), ("gamma", 0.3, 0.7, 1.5)):
        v = ch[name]
        on = v > 0
        assert close(on.all(1).mean(), p) and (on.all(1) == on.any(1)).all(), name
        assert ((v[on] >= lo) & (v[on] <= hi)).all() and close((v[on] < 1).mean(), 0.5, on.sum()), name
    assert (ch["lowres_zoom"] == 0).all()
    # the first round(n 0.67) samples are free crops, the rest forced
    free = round(n * 0.67)
    assert free == 2744


def test_loader_refuses_an_indivisible_patch():
    with pytest.raises(ValueError, match=r"patch 30 x 34 is not divisible by 2\^\(n_scales - 1\) = 4"):
        nd._scale_shapes((30, 34), 3)
    assert nd._scale_shapes((32, 64), 3) == [(32, 64), (16, 32), (8, 16)]


def test_prototypes_of_the_new_entry_points():
    """Argument counts and kinds of the ctypes table against the declarations of include/ldiff.h; no atomics in the augmentation kernels."""
    with open(os.path.join(ROOT, "include", "ldiff.h")) as f:
        header = f.read()
    kinds = {"int": C.c_int, "float": C.c_float, "int64_t": C.c_int64, "uint64_t": C.c_uint64}
    for name in ("ldiff_op_seg_sample", "ldiff_op_seg_intensity_ws_bytes", "ldiff_op_seg_intensity"):
        m = re.search(r"(\w+)\s+" + name + r"\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/ldiff.h"
        res, args = _lib.SIGNATURES[name]
        assert res is kinds[m.group(1)]
        want = []
        for a in m.group(2).split(","):
            a = a.strip()
            want.append(C.c_void_p if "*" in a else kinds[a.split()[-2]])
        assert args == want, f"{name}: {args} against the header's {want}"
    assert int(re.search(r"#define LDIFF_VERSION (\d+)", header).group(1)) >= 206
    with open(os.path.join(ROOT, "ldiffusion_amd", "csrc", "kernels_segaug.hip")) as f:
        src = f.read()
    assert "atomicAdd" not in src and "atomic" not in src.replace("no atomics", "").replace("No atomics", ""), "the augmentation kernels reduce in a fixed order"


def test_entry_points_refuse_bad_arguments():
    lib = _lib.load()
    assert lib.ldiff_op_seg_intensity_ws_bytes(12, 3, 512, 512) == 12 * 3 * 512 * 512 * 4 and lib.ldiff_op_seg_intensity_ws_bytes(0, 3, 8, 8) == 0
    one = C.c_void_p(16)
    assert lib.ldiff_op_seg_sample(one, 64, one, 1, one, 2, 3, 30, 34, 3, one, one, None) == -1 and b"not divisible" in lib.ldiff_last_error()
    assert lib.ldiff_op_seg_sample(one, 64, one, 1, one, 2, 3, 32, 32, 9, one, one, None) == -1 and b"n_scales" in lib.ldiff_last_error()
    assert lib.ldiff_op_seg_sample(None, 64, one, 1, one, 2, 3, 32, 32, 3, one, one, None) == -1 and b"null" in lib.ldiff_last_error()
    assert lib.ldiff_op_seg_intensity(one, one, one, 2, 3, 32, 32, None, 0, one, 100, None) == -1 and b"workspace" in lib.ldiff_last_error()
    assert lib.ldiff_op_seg_intensity(None, one, one, 2, 3, 32, 32, None, 0, one, 1 << 20, None) == -1 and b"null" in lib.ldiff_last_error()
