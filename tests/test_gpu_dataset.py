"""GPU (-m gpu): the device-resident dataset (ldiffusion_amd/dataset.py DeviceLoader; include/ldiff.h ldiff_op_label_table_u8 / _gather_labels /
_warmup_labels / _warmup_images) against the host loader and against torch: batches bit for bit in torch's own order, the warm-up labels equal to torch's
bilinear rule, the warm-up images inside a derived float32 bound of the float64 evaluation, batch invariance, and `train(args)` from two folders."""
import csv
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from ldiffusion_amd import dataset, imgio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GREYS = np.array([0, 50, 100, 150, 200, 250, 255, 7], np.uint8)   # the tissue table's keys and one unlisted level


def _write_folders(root, n, sizes, label_hw, seed=5, greys=GREYS):
    rng = np.random.default_rng(seed)
    img_dir, lab_dir = root / "images", root / "labels"
    img_dir.mkdir(), lab_dir.mkdir()
    for i in range(n):
        h, w = sizes[i % len(sizes)]
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(img_dir / f"case_{i:02d}.png")
        Image.fromarray(greys[rng.integers(0, len(greys), label_hw)]).save(lab_dir / f"case_{i:02d}.png")
    return str(img_dir), str(lab_dir)


def _lists(img_dir, lab_dir):
    return sorted(os.path.join(img_dir, f) for f in os.listdir(img_dir)), sorted(os.path.join(lab_dir, f) for f in os.listdir(lab_dir))


@pytest.fixture(scope="module")
def seven(tmp_path_factory):
    """7 images of mixed native sizes, labels 48 x 48, as a host dataset at image_size 32."""
    img_dir, lab_dir = _write_folders(tmp_path_factory.mktemp("seven"), 7, ((40, 56), (64, 64), (33, 47)), (48, 48))
    images, labels = _lists(img_dir, lab_dir)
    return dataset.MedicalSegmentationDataset(images, labels, dataset.default_transform(32), "tissue")


@pytest.fixture(scope="module")
def seven_on_device(seven):
    return dataset.DeviceLoader(seven, batch_size=2, shuffle=True, device=DEV, io_workers=2)


@pytest.mark.parametrize("case", ["shuffle", "drop_last", "rank0", "rank1", "validation"])
def test_loader_parity(seven, seven_on_device, case):
    """DeviceLoader's batches are the host DataLoader's: all three tensors torch.equal, the same order, the same state of torch's generator afterwards."""
    from torch.utils.data import DataLoader, DistributedSampler
    if case in ("rank0", "rank1"):
        kw = dict(batch_size=2, drop_last=True)
        samplers = [DistributedSampler(seven, num_replicas=2, rank=int(case[-1]), shuffle=True, drop_last=True) for _ in range(2)]
        for s in samplers:
            s.set_epoch(3)
        host = DataLoader(seven, sampler=samplers[0], **kw)
        dev = dataset.DeviceLoader(seven, sampler=samplers[1], device=DEV, io_workers=0, **kw)
        n_batches = 1                                                    # 7 -> 3 per rank -> one batch of 2 under drop_last
    else:
        kw = dict(shuffle=dict(batch_size=2, shuffle=True), drop_last=dict(batch_size=2, shuffle=True, drop_last=True), validation=dict(batch_size=1, shuffle=False))[case]
        host = DataLoader(seven, **kw)
        dev = seven_on_device if case == "shuffle" else dataset.DeviceLoader(seven, device=DEV, **kw)
        n_batches = dict(shuffle=4, drop_last=3, validation=7)[case]
    assert len(dev) == len(host) == n_batches and dev.batch_size == host.batch_size and dev.dataset is seven and type(dev.sampler) is type(host.sampler)
    torch.manual_seed(17)
    want = list(host)
    state = torch.get_rng_state()
    torch.manual_seed(17)
    got = list(dev)
    assert torch.equal(torch.get_rng_state(), state)
    assert len(got) == len(want) == n_batches
    for (gi, gm, gl), (wi, wm, wl) in zip(got, want):
        assert gi.is_cuda and gm.is_cuda and gl.is_cuda
        assert gi.dtype == torch.float32 and gm.dtype == torch.int64 and gl.dtype == torch.uint8
        assert gi.shape == wi.shape and gm.shape == wm.shape and gl.shape == wl.shape
        assert torch.equal(gi.cpu(), wi) and torch.equal(gm.cpu(), wm) and torch.equal(gl.cpu(), wl)
    if case == "shuffle":
        assert tuple(got[-1][0].shape) == (1, 3, 32, 32) and tuple(got[0][1].shape) == (2, 48, 48) and tuple(got[0][2].shape) == (2, 1, 48, 48)
        # warmup_batches: the same order and the same draws; its labels are the torch expression of the loop on the loader's own labels
        torch.manual_seed(17)
        warm = list(dev.warmup_batches(8))
        assert torch.equal(torch.get_rng_state(), state) and len(warm) == n_batches
        for (im, lab), (_, _, wl) in zip(warm, want):
            assert tuple(im.shape) == (wl.shape[0], 3, 8, 8) and im.dtype == torch.float32
            assert torch.equal(lab.cpu(), F.interpolate(wl.float(), size=(8, 8), mode="bilinear", align_corners=False).to(torch.uint8))


def test_load_data_on_the_device_is_load_data_on_the_host(seven):
    img_dir, lab_dir = os.path.dirname(seven.image_dir[0]), os.path.dirname(seven.label_dir[0])
    random.seed(2)
    ht, hv, _ = dataset.load_data(img_dir, lab_dir, 2, "tissue", image_size=32)
    random.seed(2)
    dt, dv, sampler = dataset.load_data(img_dir, lab_dir, 2, "tissue", image_size=32, device=DEV, io_workers=0)
    assert sampler is None and isinstance(dt, dataset.DeviceLoader) and isinstance(dv, dataset.DeviceLoader)
    assert dt.dataset.image_dir == ht.dataset.image_dir and dv.dataset.label_dir == hv.dataset.label_dir and len(dt) == len(ht) == 2 and len(dv) == len(hv) == 3
    for host, dev in ((ht, dt), (hv, dv)):
        torch.manual_seed(1)
        want = list(host)
        torch.manual_seed(1)
        for got, ref in zip(dev, want):
            assert all(torch.equal(g.cpu(), r) for g, r in zip(got, ref))


def test_label_errors(seven, tmp_path):
    odd = tmp_path / "odd.png"
    Image.fromarray(np.zeros((48, 40), np.uint8)).save(odd)
    labels = list(seven.label_dir)
    labels[4] = str(odd)
    ds = dataset.MedicalSegmentationDataset(seven.image_dir, labels, dataset.default_transform(32), "tissue")
    with pytest.raises(ValueError, match="odd.png"):
        dataset.DeviceLoader(ds, batch_size=2, device=DEV)
    with pytest.raises(ValueError, match="cache_bytes"):
        dataset.DeviceLoader(seven, batch_size=2, device=DEV, cache_bytes=1)
    with pytest.raises(ValueError, match="Unsupported level"):
        dataset.DeviceLoader(dataset.MedicalSegmentationDataset(seven.image_dir, seven.label_dir, dataset.default_transform(32), "organ"), device=DEV)
    with pytest.raises(ValueError, match="io_workers"):
        dataset.DeviceLoader(seven, device=DEV, io_workers=99)


def test_label_table_kernel():
    """ldiff_op_label_table_u8 on an odd length from an unaligned base (the narrow path), on an aligned one (16-byte path + tail), and in place."""
    g = torch.Generator().manual_seed(3)
    table = torch.from_numpy(dataset.label_table("cell"))
    x = torch.randint(0, 256, (5000 + 13,), generator=g, dtype=torch.uint8)
    xd, td = x.to(DEV), table.to(DEV)
    assert torch.equal(dataset.table_u8(xd, td).cpu(), table[x.long()])
    view = xd[3:4100]
    assert torch.equal(dataset.table_u8(view, td).cpu(), table[x[3:4100].long()])
    dataset.table_u8(xd, td, out=xd)
    assert torch.equal(xd.cpu(), table[x.long()])


@pytest.fixture(scope="module")
def label_store():
    """Label stores of the tested source sizes, values as the tables produce them (0 .. 10), in blocks and in noise."""
    g = torch.Generator().manual_seed(8)
    out = {}
    for h, w in ((128, 128), (24, 24), (16, 16), (8, 8), (48, 24), (100, 100)):
        x = torch.randint(0, 11, (4, h, w), generator=g, dtype=torch.uint8)
        x[1] = torch.randint(0, 11, (1, (h + 6) // 7, (w + 4) // 5), generator=g, dtype=torch.uint8).repeat_interleave(7, 1).repeat_interleave(5, 2)[0, :h, :w]
        x[2] = 255                                                       # the largest byte: the sum of four does not wrap
        out[(h, w)] = x
    return out


@pytest.mark.parametrize("h,w,oh,ow", [(128, 128, 8, 8), (24, 24, 8, 8), (16, 16, 8, 8), (8, 8, 8, 8), (48, 24, 8, 8)])
def test_warmup_labels_equal_torch(lib, label_store, h, w, oh, ow):
    """Integer ratios (16: the workload's 1024 -> 64; 3: odd; 2; 1; 6 x 3: mixed): the kernel == the torch expression evaluated on the CPU, bit for bit."""
    x = label_store[(h, w)]
    idx = torch.tensor([3, 1, 1, 0, 2], dtype=torch.int32)
    assert lib.ldiff_op_warmup_labels_supported(h, w, oh, ow) == 1
    got = dataset.warmup_labels(x.to(DEV), idx.to(DEV), (oh, ow))
    want = F.interpolate(x[idx.long()][:, None].float(), size=(oh, ow), mode="bilinear", align_corners=False).to(torch.uint8)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (5, 1, oh, ow) and torch.equal(got.cpu(), want)


def test_warmup_labels_fallback(lib, label_store):
    """100 -> 12 is no integer ratio: the kernel declines (return code), and the loader's value is the torch expression evaluated on the device."""
    x = label_store[(100, 100)].to(DEV)
    idx = torch.tensor([2, 0, 1], dtype=torch.int32, device=DEV)
    assert lib.ldiff_op_warmup_labels_supported(100, 100, 12, 12) == 0
    out = torch.empty((3, 1, 12, 12), dtype=torch.uint8, device=DEV)
    assert lib.ldiff_op_warmup_labels(x.data_ptr(), 4, 100, 100, idx.data_ptr(), 3, 12, 12, out.data_ptr(), None) == -1
    got = dataset.warmup_labels(x, idx, (12, 12))
    want = F.interpolate(x[idx.long()][:, None].float(), size=(12, 12), mode="bilinear", align_corners=False).to(torch.uint8)
    assert torch.equal(got, want)
    label, mask = dataset.gather_labels(x, idx)
    assert torch.equal(label[:, 0], x[idx.long()]) and torch.equal(mask, x[idx.long()].long()) and mask.dtype == torch.int64


def _image_store(s, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (3, s, s, 3), generator=g, dtype=torch.uint8)
    x[1, :, : s // 2] = 255                                              # an edge of full contrast
    return x


@pytest.mark.parametrize("s,out", [(128, 8), (100, 12), (32, 8), (24, 64)])
def test_warmup_images_against_float64(s, out):
    """ldiff_op_warmup_images against the float64 evaluation of the same table values with the double weights (`imgio.weights`), B = 3 with a repeated index.
    S = 100: rows of 300 bytes are not 16-byte aligned (heads and tails on the narrow path); 24 -> 64: upsampling, support 1.

    Bound: (taps_x + taps_y + 4) * 2^-24 * max|table|.  Every table value t (|t| <= T = max|table|) reaches the output through the horizontal sum
    h = sum_x wx * t and the vertical sum sum_y wy * h.  Per axis: the weight is rounded to float32 once (relative 2^-24), its product once, and the running
    sum once per tap -- at most taps + 1 roundings of magnitude <= 2^-24 * T behind the weight's own, because the weights are non-negative and sum to 1, so that every
    partial sum stays within T (to first order).  That is (taps_x + 2) + (taps_y + 2) units of 2^-24 * T.  (A fused multiply-add only removes roundings.)"""
    cache = _image_store(s, s + out)
    table = dataset.host_normalize_table("cpu")
    idx = torch.tensor([2, 0, 2], dtype=torch.int32)
    got = dataset.warmup_images(cache.to(DEV), idx.to(DEV), (out, out), table.to(DEV))
    bounds, w = imgio.weights(s, out)
    m = np.zeros((out, s))
    for o in range(out):
        m[o, bounds[o, 0]:bounds[o, 0] + bounds[o, 1]] = w[o, :bounds[o, 1]]
    vals = np.stack([table[c].double().numpy()[cache[idx.long()][..., c].numpy()] for c in range(3)], 1)      # [B, 3, S, S]
    want = np.einsum("yh,nchw,xw->ncyx", m, vals, m)
    taps = w.shape[1]
    bound = (2 * taps + 4) * 2.0 ** -24 * float(table.abs().max())
    err = np.abs(got.cpu().double().numpy() - want).max()
    print(f"warmup_images {s} -> {out}: taps {taps}, max |err| = {err:.3e}, bound {bound:.3e}")
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 3, out, out)
    assert torch.equal(got[0], got[2])
    assert err <= bound


def test_batch_invariance(seven_on_device, label_store):
    """The same index drawn alone and inside a batch of 3: equal images and labels, from the warm-up kernels and from the loader's batch path."""
    dev = seven_on_device
    three, one = torch.tensor([5, 2, 6], dtype=torch.int32, device=DEV), torch.tensor([2], dtype=torch.int32, device=DEV)
    for size in ((8, 8), (16, 16), (20, 20)):                            # labels 48 -> 8, 16 (kernel) and 20 (fallback); images 32 -> 8, 16, 20
        assert torch.equal(dataset.warmup_images(dev.images, three, size, dev._table)[1], dataset.warmup_images(dev.images, one, size, dev._table)[0])
        assert torch.equal(dataset.warmup_labels(dev.labels, three, size)[1], dataset.warmup_labels(dev.labels, one, size)[0])
    (l3, m3), (l1, m1) = dataset.gather_labels(dev.labels, three), dataset.gather_labels(dev.labels, one)
    assert torch.equal(l3[1], l1[0]) and torch.equal(m3[1], m1[0])
    big = _image_store(128, 1).to(DEV)
    t = dev._table
    assert torch.equal(dataset.warmup_images(big, torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV), (8, 8), t)[1],
                       dataset.warmup_images(big, torch.tensor([1], dtype=torch.int32, device=DEV), (8, 8), t)[0])


def test_train_from_folders_end_to_end(tmp_path):
    """`train(args, component="ldiffusion")` from two folders of 6 images (96^2, image_size 96, two epochs, batch 2) on the tiny checkpoint of
    test_train_ldiffusion_mirror_end_to_end: the CSV and the checkpoint are written, and the epoch losses agree with a run on the same seeds through the
    injected host loader within 2e-3 relative, the margin that test uses between its two drivers (the two runs differ in the float32 rounding of the 64 x 64 images)."""
    from test_gpu_models import _write_sd_dirs
    from ldiffusion_amd import configs, weights
    from ldiffusion_amd.ldiffusion import LDiffusionModel
    ucfg, vcfg = configs.TINY_UNET, configs.TINY_VAE
    tiny = dict(ucfg=ucfg, vcfg=vcfg, usd=weights.synthetic_state_dict(weights.unet_param_shapes(ucfg), 42, fp16_values=True),
                vsd=weights.synthetic_state_dict(weights.vae_param_shapes(vcfg), 43, fp16_values=True))
    sd_dir, _, _ = _write_sd_dirs(tmp_path, tiny, torch.float32, torch.float32)
    img_dir, lab_dir = _write_folders(tmp_path, 6, ((96, 96),), (96, 96), seed=21, greys=np.array([0, 100, 150], np.uint8))

    def args(root):
        return SimpleNamespace(diffusion_path=str(sd_dir), num_inference_steps=5, batch_size=2, ldiffusion_epochs=2, output_root=str(tmp_path / root), image_dir=img_dir,
                               label_dir=lab_dir, image_size=96, io_workers=2)

    def losses(root):
        rows = list(csv.reader(open(next((tmp_path / root / "train_save" / "loss").glob("*/contrast_loss.csv")))))
        assert rows[0] == ["epoch", "loss"] and [r[0] for r in rows[1:]] == ["1", "2"]
        return [float(r[1]) for r in rows[1:]]

    random.seed(9)
    torch.manual_seed(5)
    saved = LDiffusionModel(str(sd_dir), "tissue").train(args("out"), component="ldiffusion")
    assert saved.startswith(str(tmp_path / "out")) and {"config.json", weights.WEIGHTS_NAME, "proj_weights.pt"} <= set(os.listdir(saved))
    got = losses("out")
    random.seed(9)
    train_loader, val_loader, _ = dataset.load_data(img_dir, lab_dir, 2, "tissue", image_size=96)
    assert len(train_loader) == 2
    torch.manual_seed(5)
    LDiffusionModel(str(sd_dir), "tissue").train(args("out2"), component="ldiffusion", train_loader=train_loader, val_loader=val_loader)
    want = losses("out2")
    print(f"train from folders: epoch losses {got} (device store), {want} (injected host loader)")
    assert all(np.isfinite(got)) and all(abs(a - b) <= 2e-3 * abs(b) for a, b in zip(got, want)), (got, want)
