"""CPU: the host side of the dataset pipeline (ldiffusion_amd/dataset.py; the reference's dataset.py:10-89 and load_data, ldiffusion.py:72-119) -- tables,
convert_labels, the dataset's triple, the transform against the numpy restatement of Pillow's resize and the normalisation table, the split and the batch
order against torch's own loaders and samplers, the double weights of the warm-up reduction against torch in float64, and the command line."""
import importlib.util
import os
import random
import sys
import types

import numpy as np
import pytest
import torch
from PIL import Image

from ldiffusion_amd import dataset, imgio, utils

REFERENCE = os.environ.get("LDIFF_REFERENCE_DIR", "/root/reference")


def _write_folders(tmp_path, n, label_hw=(12, 10), sizes=((14, 18),)):
    """n RGB PNGs (native sizes cycling through `sizes`, (h, w)) and n grey label PNGs holding listed and unlisted grey levels."""
    rng = np.random.default_rng(3)
    img_dir, lab_dir = tmp_path / "images", tmp_path / "labels"
    img_dir.mkdir(), lab_dir.mkdir()
    greys = np.array([0, 50, 100, 150, 200, 250, 255, 25, 75, 7, 201], np.uint8)
    for i in range(n):
        h, w = sizes[i % len(sizes)]
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(img_dir / f"case_{i:02d}.png")
        Image.fromarray(greys[rng.integers(0, len(greys), label_hw)]).save(lab_dir / f"case_{i:02d}.png")
    return str(img_dir), str(lab_dir)


def test_tables_and_convert_labels(tmp_path):
    assert dataset.pixel_to_label == {0: 0, 100: 1, 150: 2, 50: 3, 200: 4, 250: 5, 255: 6}
    assert dataset.pixel_to_label_cell == {25 * k: k for k in range(11)}
    for level, mapping in (("tissue", dataset.pixel_to_label), ("cell", dataset.pixel_to_label_cell)):
        t = dataset.label_table(level)
        assert t.dtype == np.uint8 and t.shape == (256,)
        assert all(int(t[g]) == (mapping[g] if g in mapping else 0) for g in range(256))
    grey = np.array([[0, 50, 100, 150], [200, 250, 255, 7], [25, 75, 201, 1]], np.uint8)   # 7, 201, 1 (and 25 / 75 at the tissue level): unlisted -> 0
    path = tmp_path / "label.png"
    Image.fromarray(grey).save(path)
    assert np.array_equal(dataset.convert_labels(str(path), "tissue"), np.array([[0, 3, 1, 2], [4, 5, 6, 0], [0, 0, 0, 0]], np.uint8))
    assert np.array_equal(dataset.convert_labels(str(path), "cell"), np.array([[0, 2, 4, 6], [8, 10, 0, 0], [1, 3, 0, 0]], np.uint8))
    assert dataset.convert_labels(str(path), "cell").dtype == np.uint8
    with pytest.raises(ValueError, match="Unsupported level"):
        dataset.convert_labels(str(path), "organ")
    with pytest.raises(ValueError, match="Unsupported level"):
        dataset.label_table(None)


def test_getitem_triple(tmp_path):
    img_dir, lab_dir = _write_folders(tmp_path, 2)
    images = sorted(os.path.join(img_dir, f) for f in os.listdir(img_dir))
    labels = sorted(os.path.join(lab_dir, f) for f in os.listdir(lab_dir))
    ds = dataset.MedicalSegmentationDataset(images, labels, dataset.default_transform(16), "tissue")
    assert ds.image_dir is images and ds.label_dir is labels and len(ds) == 2
    image, mask, label = ds[1]
    assert image.dtype == torch.float32 and tuple(image.shape) == (3, 16, 16)
    assert mask.dtype == torch.int64 and tuple(mask.shape) == (12, 10)
    assert label.dtype == torch.uint8 and tuple(label.shape) == (1, 12, 10)
    assert torch.equal(mask, label[0].long()) and torch.equal(label[0], torch.from_numpy(dataset.convert_labels(labels[1], "tissue")))
    plain = dataset.MedicalSegmentationDataset(images, labels, None, "cell")[0][0]         # no transform: ToTensor alone, the native size
    want = torch.from_numpy(np.asarray(Image.open(images[0]).convert("RGB"), np.float32) / 255.0).permute(2, 0, 1)
    assert tuple(plain.shape) == (3, 14, 18) and torch.equal(plain, want)


def _load_reference_dataset():
    """The reference's dataset.py as a module, with empty stand-ins for the imports this environment lacks (nothing of them is called)."""
    path = os.path.join(REFERENCE, "dataset.py")
    stubs = {}
    for name in ("cv2", "torchvision", "torchvision.transforms"):
        if name not in sys.modules:
            stubs[name] = sys.modules[name] = types.ModuleType(name)
    try:
        if "torchvision" in stubs:
            stubs["torchvision"].transforms = sys.modules["torchvision.transforms"]
        spec = importlib.util.spec_from_file_location("_reference_dataset", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    finally:
        for name in stubs:
            sys.modules.pop(name, None)


@pytest.mark.skipif(not os.path.exists(os.path.join(REFERENCE, "dataset.py")), reason="the reference tree is not present")
def test_tables_and_convert_labels_equal_the_reference(tmp_path):
    ref = _load_reference_dataset()
    assert dataset.pixel_to_label == ref.pixel_to_label and dataset.pixel_to_label_cell == ref.pixel_to_label_cell
    path = tmp_path / "label.png"
    Image.fromarray(np.arange(256, dtype=np.uint8).reshape(16, 16)).save(path)               # every grey level once
    for level in ("tissue", "cell"):
        want = ref.convert_labels(str(path), level)
        got = dataset.convert_labels(str(path), level)
        assert got.dtype == want.dtype and np.array_equal(got, want)
        assert np.array_equal(dataset.label_table(level), want.reshape(256))
    with pytest.raises(ValueError) as theirs:
        ref.convert_labels(str(path), "organ")
    with pytest.raises(ValueError) as ours:
        dataset.convert_labels(str(path), "organ")
    assert str(ours.value) == str(theirs.value)


@pytest.mark.parametrize("h,w,size", [(40, 56, 32), (16, 16, 32)])
def test_default_transform_equals_resize_host_and_table(h, w, size):
    """Resize + ToTensor + Normalize on PIL and torch == the numpy restatement of Pillow's resize looked up in `imgio.normalize_table`, bit for bit: the
    device loader serves the second form."""
    rgb = np.random.default_rng(h + size).integers(0, 256, (h, w, 3), dtype=np.uint8)
    got = dataset.default_transform(size)(Image.fromarray(rgb))
    resized = imgio.resize_u8_host(rgb, (size, size))
    table = imgio.normalize_table(utils.IMAGENET_MEAN, utils.IMAGENET_STD, "cpu")
    want = torch.stack([table[c][torch.from_numpy(resized[..., c].astype(np.int64))] for c in range(3)])
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, size, size) and torch.equal(got, want)


def test_load_data_split_and_batch_order(tmp_path):
    from torch.utils.data import DataLoader, DistributedSampler
    img_dir, lab_dir = _write_folders(tmp_path, 10)
    images = sorted(os.path.join(img_dir, f) for f in os.listdir(img_dir))
    labels = sorted(os.path.join(lab_dir, f) for f in os.listdir(lab_dir))
    random.seed(11)
    indices = list(range(10))
    random.shuffle(indices)                                                                  # ldiffusion.py:84-89
    random.seed(11)
    train_loader, val_loader, sampler = dataset.load_data(img_dir, lab_dir, 2, "tissue", image_size=16)
    assert sampler is None and isinstance(train_loader, DataLoader) and isinstance(val_loader, DataLoader)
    assert train_loader.dataset.image_dir == [images[i] for i in indices[:7]] and train_loader.dataset.label_dir == [labels[i] for i in indices[:7]]
    assert val_loader.dataset.image_dir == [images[i] for i in indices[7:]] and val_loader.dataset.label_dir == [labels[i] for i in indices[7:]]
    random.seed(11)
    assert dataset.split_indices(10, 0.7) == (indices[:7], indices[7:])
    assert train_loader.batch_size == 2 and train_loader.drop_last and len(train_loader) == 3 and val_loader.batch_size == 1 and len(val_loader) == 3
    # the batch order under torch's generator: a hand-built DataLoader over the same dataset
    hand = DataLoader(train_loader.dataset, batch_size=2, shuffle=True, drop_last=True)
    torch.manual_seed(4)
    want = [b for b in hand]
    state = torch.get_rng_state()
    torch.manual_seed(4)
    got = [b for b in train_loader]
    assert torch.equal(torch.get_rng_state(), state) and len(got) == len(want) == 3
    for a, b in zip(got, want):
        assert all(torch.equal(x, y) for x, y in zip(a, b)) and tuple(a[0].shape) == (2, 3, 16, 16) and tuple(a[1].shape) == (2, 12, 10) and tuple(a[2].shape) == (2, 1, 12, 10)
    val = [b for b in val_loader]                                                            # unshuffled, batch 1
    assert all(torch.equal(v[0][0], val_loader.dataset[i][0]) for i, v in enumerate(val))
    # two ranks: DistributedSampler's indices, and set_epoch changes them
    for rank in range(2):
        random.seed(11)
        tl, vl, ts = dataset.load_data(img_dir, lab_dir, 2, "tissue", world=2, rank=rank, image_size=16)
        assert isinstance(ts, DistributedSampler) and tl.sampler is ts and ts.shuffle and ts.drop_last and isinstance(vl.sampler, DistributedSampler) and not vl.sampler.shuffle
        ref = DistributedSampler(tl.dataset, num_replicas=2, rank=rank, shuffle=True, drop_last=True)
        assert list(ts) == list(ref) and len(list(ts)) == 3
        first = list(ts)
        ts.set_epoch(1), ref.set_epoch(1)
        assert list(ts) == list(ref) and list(ts) != first
        assert list(vl.sampler) == list(DistributedSampler(vl.dataset, num_replicas=2, rank=rank, shuffle=False))
    os.remove(labels[-1])
    with pytest.raises(AssertionError):
        dataset.load_data(img_dir, lab_dir, 2, "tissue")


@pytest.mark.parametrize("hs,ws,oh,ow", [(128, 128, 8, 8), (100, 100, 12, 12), (130, 70, 8, 8), (40, 40, 64, 64)])
def test_weights_are_torchs_antialiased_bilinear(hs, ws, oh, ow):
    """`imgio.weights` -- the double stage of `imgio.coefficients` -- reproduces F.interpolate(mode="bilinear", antialias=True) in float64 to round-off: the
    warm-up image kernel applies these weights; and `coefficients` is still made from them."""
    import torch.nn.functional as F
    x = torch.rand((1, 2, hs, ws), dtype=torch.float64, generator=torch.Generator().manual_seed(hs + ow))
    want = F.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=False, antialias=True)
    (yb, yw), (xb, xw) = imgio.weights(hs, oh), imgio.weights(ws, ow)
    my, mx = np.zeros((oh, hs)), np.zeros((ow, ws))
    for m, b, w in ((my, yb, yw), (mx, xb, xw)):
        for o in range(m.shape[0]):
            m[o, b[o, 0]:b[o, 0] + b[o, 1]] = w[o, :b[o, 1]]
    got = np.einsum("yh,nchw,xw->ncyx", my, x.numpy(), mx)
    assert np.abs(got - want.numpy()).max() <= 1e-14
    assert yw.dtype == np.float64 and np.allclose(yw.sum(1), 1.0, atol=1e-15) and (yw >= 0).all()
    bounds, coef = imgio.coefficients(hs, oh)
    assert np.array_equal(bounds, yb) and np.array_equal(coef, np.where(np.arange(yw.shape[1])[None] < yb[:, 1:2], (0.5 + yw * (1 << 22)).astype(np.int32), 0))


def test_parse_args():
    from ldiffusion_amd.ldiffusion import parse_args
    argv = ["--diffusion-path", "sd", "--image-dir", "im", "--label-dir", "lb", "--num-epochs", "12", "--batch-size", "8", "--num-inference-steps", "50", "--num-classes", "6"]
    a = parse_args(argv)
    assert (a.diffusion_path, a.image_dir, a.label_dir, a.num_epochs, a.batch_size, a.num_inference_steps, a.num_classes) == ("sd", "im", "lb", 12, 8, 50, 6)
    assert isinstance(a.local_rank, int) and a.local_rank == int(os.environ.get("LOCAL_RANK", -1))
    assert (a.level, a.component, a.ldiffusion_weight) == ("tissue", "all", None)
    b = parse_args(argv + ["--local_rank", "3", "--level", "cell", "--component", "segmentor", "--ldiffusion-weight", "w"])
    assert (b.local_rank, b.level, b.component, b.ldiffusion_weight) == (3, "cell", "segmentor", "w")
    with pytest.raises(SystemExit):
        parse_args(argv[2:])                                                                 # --diffusion-path is required, as in the reference
    with pytest.raises(SystemExit):
        parse_args(argv + ["--num-epochs", "many"])


def test_train_builds_no_loader_before_todays_errors(tmp_path):
    """The orchestrator's errors fire before any file is read: nothing is listed here (the folders do not exist)."""
    from types import SimpleNamespace
    from ldiffusion_amd.ldiffusion import LDiffusionModel
    m = LDiffusionModel.__new__(LDiffusionModel)
    m.level, m.rank, m.world_size, m.is_distributed, m.diffusion_path, m.device = "cell", 0, 1, False, "sd", torch.device("cpu")
    args = SimpleNamespace(image_dir=str(tmp_path / "none"), label_dir=str(tmp_path / "none"), batch_size=2, num_epochs=12, num_classes=3, diffusion_path="sd")
    with pytest.raises(ValueError, match="unknown component"):
        m.train(args, component="both")
    with pytest.raises(NotImplementedError, match="cell_weights="):
        m.train(args)
    with pytest.raises(RuntimeError, match="train_loader"):
        m.train(SimpleNamespace(image_dir=None, label_dir=None))
