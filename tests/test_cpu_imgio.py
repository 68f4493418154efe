"""CPU (-m "not gpu"): the host side of the device image front end (ldiffusion_amd/imgio.py) -- the numpy restatement of Pillow's 8-bit bilinear
resize against `Image.resize(size, Image.BILINEAR)` bit for bit, the coefficient tables, the refusals -- and the host side of the batched dataset pass
(utils.create_nnunet_dataset(batch_images=...)): mixed sizes change nothing, a missing label raises in the caller and leaves no worker thread."""
import ctypes as C
import os
import threading

import numpy as np
import pytest
import torch
from PIL import Image

from ldiffusion_amd import _lib, imgio, utils

# (h, w -> oh, ow): up, down, one pass skipped, 1-pixel sides, mixed up/down, a non-integer reduction, 15x up, the 1000 -> 1024 ratio, the 16x window
PAIRS = [(37, 53, 64, 64), (64, 64, 37, 53), (33, 77, 33, 20), (1, 5, 7, 3), (257, 129, 64, 200), (300, 200, 64, 64), (17, 17, 256, 256), (250, 250, 256, 256),
         (1024, 1024, 64, 64)]


def pil_resize(a, oh, ow):
    return np.asarray(Image.fromarray(a).resize((ow, oh), Image.BILINEAR))


@pytest.mark.parametrize("h,w,oh,ow", PAIRS)
def test_host_restatement_equals_pillow_bit_for_bit(h, w, oh, ow):
    rng = np.random.default_rng(h * 7919 + w * 31 + oh)
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    grey = rng.integers(0, 256, (h, w), dtype=np.uint8)
    assert np.array_equal(imgio.resize_u8_host(rgb, (ow, oh)), pil_resize(rgb, oh, ow))          # mode RGB
    assert np.array_equal(imgio.resize_u8_host(grey, (ow, oh)), pil_resize(grey, oh, ow))        # mode L
    batch = np.stack([rgb, rgb[::-1].copy()])
    got = imgio.resize_u8_host(batch, (ow, oh))
    assert got.shape == (2, oh, ow, 3) and np.array_equal(got[1], pil_resize(batch[1], oh, ow))
    # the extremes pass through exactly: the coefficient rows keep a constant image constant
    for level in (0, 255):
        assert (imgio.resize_u8_host(np.full((h, w, 1), level, np.uint8), (ow, oh)) == level).all()


@pytest.mark.parametrize("n_in,n_out", sorted({(p[1], p[3]) for p in PAIRS} | {(p[0], p[2]) for p in PAIRS} | {(1000, 1024), (2000, 125)}))
def test_tables(n_in, n_out):
    bounds, coef = imgio.coefficients(n_in, n_out)
    taps = int(np.ceil(max(n_in / n_out, 1.0))) * 2 + 1
    assert bounds.shape == (n_out, 2) and coef.shape == (n_out, taps) and bounds.dtype == np.int32 and coef.dtype == np.int32
    first, length = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
    assert (first >= 0).all() and (length >= 1).all() and (first + length <= n_in).all() and (length <= taps).all()     # the bounds stay inside the source
    assert (coef >= 0).all()                                                                                            # bilinear makes no negative weight
    assert (np.abs(coef.sum(1, dtype=np.int64) - (1 << 22)) <= length).all()                                            # each rounding moves a coefficient by <= 1/2 ... 1
    assert not coef[np.arange(taps)[None, :] >= length[:, None]].any()                                                  # zeros behind the window
    assert int((coef.astype(np.int64) * 255).sum(1).max()) + (1 << 21) < 2 ** 31                                        # the sum fits int32
    assert imgio.coefficients(n_in, n_out)[1] is coef and not coef.flags.writeable                                     # cached per pair, never recomputed


def test_refusals_name_the_argument():
    a = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match="x"):
        imgio.resize_u8_host(np.zeros((8, 8, 2), np.uint8), (4, 4))          # channel count
    with pytest.raises(ValueError, match="x"):
        imgio.resize_u8_host(np.zeros((8, 8, 4), np.uint8), (4, 4))
    with pytest.raises(ValueError, match="x"):
        imgio.resize_u8_host(np.zeros((0, 8, 3), np.uint8), (4, 4))          # a side of 0
    with pytest.raises(ValueError, match="x"):
        imgio.resize_u8_host(a.astype(np.float32), (4, 4))
    with pytest.raises(ValueError, match=r"size\[0\]"):
        imgio.resize_u8_host(a, (0, 4))
    with pytest.raises(ValueError, match=r"size\[1\]"):
        imgio.resize_u8_host(a, (4, 0))
    with pytest.raises(ValueError, match="size"):
        imgio.resize_u8_host(a, 4)
    # the window bound: MAX_TAPS = 128 coefficients per row = reductions up to 63x; a 16x reduction is inside it, 64x is not
    assert imgio.MAX_TAPS == 128 and imgio.coefficients(1024, 64)[1].shape[1] == 33 and imgio.coefficients(63 * 4, 4)[1].shape[1] == 127
    with pytest.raises(ValueError, match="size.*taps"):
        imgio.resize_u8_host(np.zeros((64 * 4, 8, 3), np.uint8), (8, 4))
    # the device entries refuse the same before they look for a GPU
    for fn in (imgio.resize_u8, lambda x, s: imgio.resize_normalize(x, s, utils.IMAGENET_MEAN, utils.IMAGENET_STD)):
        with pytest.raises(ValueError, match="x"):
            fn(a, (4, 4))                                                     # not a tensor
        with pytest.raises(ValueError, match="x"):
            fn(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), (4, 4))          # not on the GPU
    with pytest.raises(ValueError, match="x"):
        imgio.resize_u8(torch.zeros((1, 8, 8, 2), dtype=torch.uint8), (4, 4))
    with pytest.raises(ValueError, match="x"):
        imgio.resize_u8(torch.zeros((1, 0, 8, 3), dtype=torch.uint8), (4, 4))
    with pytest.raises(ValueError, match=r"size\[0\]"):
        imgio.resize_u8(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), (0, 4))


def test_library_refuses_naming_the_argument(lib):
    """ldiff_op_resize_u8 validates before it launches: these calls reach no kernel (there is no GPU here) and name what they refuse."""
    call = lambda B, Hs, Ws, Cc, Ho, Wo, ht, vt, tables=1, lut=0, ws=0: lib.ldiff_op_resize_u8(
        C.c_void_p(64), B, Hs, Ws, Cc, Ho, Wo, C.c_void_p(64 * tables), C.c_void_p(64 * tables), ht, C.c_void_p(64 * tables), C.c_void_p(64 * tables), vt,
        C.c_void_p(64 * lut), C.c_void_p(64), C.c_void_p(0), ws, C.c_void_p(0))
    for args, word in (((1, 8, 8, 2, 4, 4, 5, 5), b"C = 2"), ((1, 0, 8, 3, 4, 4, 5, 5), b"Hs = 0"), ((1, 8, 8, 3, 4, 0, 5, 5), b"Wo = 0"),
                       ((1, 8, 8, 3, 4, 4, 129, 5), b"htaps = 129"), ((1, 8, 8, 3, 4, 4, 5, 129), b"vtaps = 129"), ((1, 8, 8, 3, 4, 4, 5, 5), b"ws of 0 bytes"),
                       ((0, 8, 8, 3, 4, 4, 5, 5), b"B = 0")):
        assert call(*args) == -1 and word in lib.ldiff_last_error(), (args, lib.ldiff_last_error())
    assert call(1, 8, 8, 3, 4, 4, 5, 5, tables=0) == -1 and b"hbounds" in lib.ldiff_last_error()
    assert call(1, 8, 8, 1, 4, 4, 5, 5, lut=1) == -1 and b"lut" in lib.ldiff_last_error()
    # the scratch of the uint8 intermediate [B, Hs, Wo, C]: only where two launches follow each other
    assert lib.ldiff_op_resize_u8_ws_bytes(8, 1000, 1000, 3, 1024, 1024, 1) == 8 * 1000 * 1024 * 3
    assert lib.ldiff_op_resize_u8_ws_bytes(2, 33, 77, 3, 33, 20, 0) == 0 and lib.ldiff_op_resize_u8_ws_bytes(2, 33, 77, 3, 33, 20, 1) == 2 * 33 * 20 * 3
    assert lib.ldiff_op_resize_u8_ws_bytes(2, 33, 77, 3, 20, 77, 1) == 0 and lib.ldiff_op_resize_u8_ws_bytes(1, 8, 8, 2, 4, 4, 0) == -1
    assert _lib.SIGNATURES["ldiff_op_resize_u8"][1][-2] is _lib.I64


def _write_dataset(tmp_path, sizes, seed=5):
    rng = np.random.default_rng(seed)
    images, labels = [], []
    for i, (h, w) in enumerate(sizes):
        images.append(str(tmp_path / f"img_{i}.png"))
        labels.append(str(tmp_path / f"lbl_{i}.png"))
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(images[-1])
        Image.fromarray((rng.integers(0, 4, (h, w)) * 60).astype(np.uint8)).save(labels[-1])
    return images, labels


def _tree(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(root) for f in fs}


def test_mixed_sizes_batch_images_changes_nothing(tmp_path):
    """Mixed sizes: no sampler runs (plain copies), so no pipeline is needed and `batch_images` must write exactly the files of the default call."""
    images, labels = _write_dataset(tmp_path, [(40, 48), (32, 32), (40, 48)])
    raw_a, raw_b = tmp_path / "raw_a", tmp_path / "raw_b"
    raw_a.mkdir(), raw_b.mkdir()
    a = utils.create_nnunet_dataset(images[:2], labels[:2], images[2:], labels[2:], 4, None, None, raw_dir=str(raw_a))
    b = utils.create_nnunet_dataset(images[:2], labels[:2], images[2:], labels[2:], 4, None, None, raw_dir=str(raw_b), batch_images=2, io_workers=2)
    assert a == b == (1, "Dataset001_Custom")
    ta, tb = _tree(raw_a), _tree(raw_b)
    assert len(ta) == 7 and ta == tb     # 3 images, 3 labels, dataset.json
    assert not [t for t in threading.enumerate() if t.name.startswith("ldiff-imgio")]


@pytest.mark.parametrize("sizes", [[(40, 48), (32, 32), (40, 48)], [(32, 32), (32, 32), (32, 32)]])
def test_missing_label_raises_in_the_caller_and_leaves_no_thread(tmp_path, sizes):
    """Mixed sizes and one size alike: the labels of a list are written before its images reach the sampler, so a label that is not there raises
    here, in the caller, before a pool exists; nothing is left running."""
    images, labels = _write_dataset(tmp_path, sizes)
    labels[1] = str(tmp_path / "not_there.png")
    raw = tmp_path / "raw"
    raw.mkdir()
    before = threading.active_count()
    with pytest.raises(FileNotFoundError, match="not_there"):
        utils.create_nnunet_dataset(images[:2], labels[:2], images[2:], labels[2:], 4, None, None, raw_dir=str(raw), batch_images=2, io_workers=2)
    assert threading.active_count() == before and not [t for t in threading.enumerate() if t.name.startswith("ldiff-imgio")]


def test_copy_or_convert_images_validates_its_keywords():
    for kw, word in ((dict(batch_images=0), "batch_images"), (dict(batch_images=2, io_workers=17), "io_workers"), (dict(batch_images=2, io_workers=-1), "io_workers")):
        with pytest.raises(ValueError, match=word):
            utils.copy_or_convert_images(["a.png"], ["b.png"], None, None, **kw)
    with pytest.raises(ValueError, match="dst_paths"):
        utils.copy_or_convert_images(["a.png"], [], None, None, batch_images=2)
    assert utils.MAX_IO_WORKERS == 16
