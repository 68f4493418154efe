"""GPU (-m gpu): the device image front end (include/ldiff.h ldiff_op_resize_u8, ldiffusion_amd/imgio.py) against Pillow itself, bit for bit:
`imgio.resize_u8` == `Image.resize(size, Image.BILINEAR)`, `imgio.resize_normalize` == the per-image path's Resize + ToTensor + Normalize expression.
No tolerance anywhere: Pillow's 8-bit rule is integer arithmetic, and the normalisation is a table made by the per-image expression itself."""
import numpy as np
import pytest
import torch
from PIL import Image

from ldiffusion_amd import imgio
from ldiffusion_amd.utils import IMAGENET_MEAN, IMAGENET_STD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (h, w -> oh, ow), as tests/test_cpu_imgio.py: up, down, one pass skipped, 1-pixel sides, mixed, a non-integer reduction, 15x up, the 1000 -> 1024 ratio,
# the 16x window.  Row lengths in bytes that are and are not multiples of 4 (the vertical kernel's two forms), more than one block per row (257 * 3, 256 * 3
# bytes > 1024), windows of 3 to 33 taps.
PAIRS = [(37, 53, 64, 64), (64, 64, 37, 53), (33, 77, 33, 20), (1, 5, 7, 3), (257, 129, 64, 200), (300, 200, 64, 64), (17, 17, 256, 256), (250, 250, 256, 256),
         (1024, 1024, 64, 64)]


def pil_resize(a, oh, ow):
    return np.asarray(Image.fromarray(a).resize((ow, oh), Image.BILINEAR))


def images(B, h, w, c, seed):
    return np.random.default_rng(seed).integers(0, 256, (B, h, w, c), dtype=np.uint8)


@pytest.mark.parametrize("h,w,oh,ow", PAIRS)
def test_resize_u8_equals_pillow(h, w, oh, ow):
    for B, c in ((3, 3), (2, 1)):
        x = images(B, h, w, c, h * 7919 + w * 31 + oh + c)
        ref = np.stack([pil_resize(a[..., 0] if c == 1 else a, oh, ow).reshape(oh, ow, c) for a in x])
        got = imgio.resize_u8(torch.from_numpy(x).to(DEV), (ow, oh))
        assert got.shape == (B, oh, ow, c) and got.dtype == torch.uint8
        assert torch.equal(got.cpu(), torch.from_numpy(ref)), f"B={B} C={c}: {(got.cpu().numpy() != ref).sum()} bytes differ from Pillow"


def test_resize_u8_identity_and_views():
    x = torch.from_numpy(images(2, 19, 23, 3, 1)).to(DEV)
    same = imgio.resize_u8(x, (23, 19))                      # both sides unchanged: a copy, as Image.resize returns one
    assert torch.equal(same, x) and same.data_ptr() != x.data_ptr()
    view = x[:, 1:, 2:]                                       # a view that is not contiguous
    ref = np.stack([pil_resize(a, 40, 9) for a in view.cpu().numpy()])
    assert torch.equal(imgio.resize_u8(view, (9, 40)).cpu(), torch.from_numpy(ref))


@pytest.mark.parametrize("h,w,oh,ow", [(37, 53, 64, 64), (250, 250, 256, 256), (64, 64, 64, 64), (33, 77, 33, 20), (33, 77, 20, 77)])
def test_resize_normalize_equals_the_per_image_expression(h, w, oh, ow):
    """utils.copy_or_convert_image / Segmentor.inference_tissue_model_nnUNetv2: np.float32 / 255.0 on the host, permute, to the device, (x - mean) / std there.
    The first two pairs are the ones to check; the others are the table form's skipped passes (none, vertical, horizontal)."""
    x = images(3, h, w, 3, h + w)
    mean = torch.tensor(IMAGENET_MEAN, device=DEV).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device=DEV).view(1, 3, 1, 1)
    ref = torch.cat([(torch.from_numpy(np.asarray(Image.fromarray(a).resize((ow, oh), Image.BILINEAR), np.float32) / 255.0).permute(2, 0, 1)[None].to(DEV) - mean) / std
                     for a in x])
    got = imgio.resize_normalize(torch.from_numpy(x).to(DEV), (ow, oh), IMAGENET_MEAN, IMAGENET_STD)
    assert got.shape == (3, 3, oh, ow) and got.dtype == torch.float32 and got.is_contiguous()
    assert torch.equal(got, ref), f"{(got != ref).sum().item()} values differ"
    host = np.stack([np.asarray(Image.fromarray(a).resize((ow, oh), Image.BILINEAR), np.float32) / 255.0 for a in x])
    assert torch.equal(imgio.resize_to_tensor(torch.from_numpy(x).to(DEV), (ow, oh)).cpu(), torch.from_numpy(host).permute(0, 3, 1, 2))


def test_planted_faults_break_the_equality():
    """The inputs above can see the two faults a kernel of this rule is most likely to have: on the host restatement, a rounding constant of 0 instead of
    2^21 and a vertical-first pass order each differ from Pillow on the pairs that run both passes."""
    for h, w, oh, ow in ((37, 53, 64, 64), (250, 250, 256, 256), (300, 200, 64, 64)):
        a = images(1, h, w, 3, h * 7919 + w * 31 + oh + 3)[0]
        ref = pil_resize(a, oh, ow)
        assert np.array_equal(imgio.resample_pass_host(imgio.resample_pass_host(a, 1, ow), 0, oh), ref)
        assert not np.array_equal(imgio.resample_pass_host(imgio.resample_pass_host(a, 1, ow, round_const=0), 0, oh, round_const=0), ref)
        assert not np.array_equal(imgio.resample_pass_host(imgio.resample_pass_host(a, 0, oh), 1, ow), ref)


def test_refusals_on_the_device():
    x = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="x"):
        imgio.resize_u8(torch.zeros((1, 8, 8, 2), dtype=torch.uint8, device=DEV), (4, 4))
    with pytest.raises(ValueError, match="x"):
        imgio.resize_normalize(torch.zeros((1, 8, 8, 1), dtype=torch.uint8, device=DEV), (4, 4), IMAGENET_MEAN, IMAGENET_STD)
    with pytest.raises(ValueError, match=r"size\[1\]"):
        imgio.resize_u8(x, (4, 0))
    with pytest.raises(ValueError, match="size.*taps"):
        imgio.resize_u8(torch.zeros((1, 256, 8, 3), dtype=torch.uint8, device=DEV), (8, 4))
    assert imgio.resize_u8(torch.zeros((1, 252, 8, 3), dtype=torch.uint8, device=DEV), (8, 4)).shape == (1, 4, 8, 3)   # 63x: the longest window, 127 taps
