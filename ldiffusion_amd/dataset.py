"""The reference's dataset pipeline (dataset.py:10-89, `load_data` of ldiffusion.py:72-119) and its device-resident form.

Host side (imports and runs without a GPU): the two grey-level tables, `convert_labels`, `MedicalSegmentationDataset`, the reference's transform
(`default_transform`: Resize -> ToTensor -> ImageNet Normalize, on PIL and numpy, no torchvision), the split and `load_data`.

Device side: `DeviceLoader` decodes every file ONCE, keeps the Pillow-resized images as uint8 [N, S, S, 3] and the converted labels as uint8 [N, H, W]
on the GPU, and serves batches from there (include/ldiff.h ldiff_op_label_table_u8 / _gather_labels / _warmup_labels / _warmup_images,
csrc/kernels_dataset.hip).  Its index order is torch's own -- a `DataLoader` over `range(N)` with the same batch_size / shuffle / sampler / drop_last is
driven for the index batches -- so for a given state of torch's global generator it yields the host loader's batches, bit for bit and in the same order, and
draws from that generator what the host loader draws.  `warmup_batches(size)` yields what the warm-up step consumes, the `size` x `size` reduction of image
and label, straight from the stored bytes.

Out of scope: `RgbDtmMaskDataset` (dataset.py:91-156 needs cv2.Canny)."""
from __future__ import annotations

import os
import random

import numpy as np
import torch

from .metrics import PIXEL_TO_LABEL as pixel_to_label, PIXEL_TO_LABEL_CELL as pixel_to_label_cell, label_lut   # dataset.py:10-32: one definition, the metrics kernel's
from .utils import IMAGENET_MEAN, IMAGENET_STD, MAX_IO_WORKERS

DEFAULT_CACHE_BYTES = 16 << 30


def label_table(level) -> np.ndarray:
    """uint8 [256]: grey level of a label file -> class index at `level`; levels that are no key map to 0, as `convert_labels` leaves them."""
    return label_lut(level).numpy()   # (raises the reference's ValueError for another level)


def _decode_rgb(path) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as img:
        return np.array(img.convert("RGB"), dtype=np.uint8)   # (np.array: a writable copy, as torch.from_numpy wants it)


def _decode_grey(path) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as img:
        return np.array(img.convert("L"), dtype=np.uint8)


def convert_labels(img_path, level) -> np.ndarray:
    """dataset.py:48-63: the label file as class indices, uint8 [H, W]."""
    table = label_table(level)            # (the reference opens the file first; a bad level raises the same ValueError either way)
    return table[_decode_grey(img_path)]


class default_transform:
    """The reference's transform (ldiffusion.py:73-77) on a PIL image: Resize((size, size)) = Pillow's bilinear resize, ToTensor = `np.float32 / 255.0`,
    Normalize(ImageNet mean, std) = `(x - mean) / std` in torch -- the float arithmetic `imgio.normalize_table` tabulates, so that the table path and this one
    agree bit for bit.  float32 [3, size, size]."""

    def __init__(self, size=1024):
        from .imgio import _side
        self.size = _side("size", size)
        self.mean = torch.tensor(IMAGENET_MEAN).view(3, 1, 1)
        self.std = torch.tensor(IMAGENET_STD).view(3, 1, 1)

    def __call__(self, image):
        from PIL import Image
        image = image.resize((self.size, self.size), Image.BILINEAR)
        x = torch.from_numpy(np.asarray(image, np.float32) / 255.0).permute(2, 0, 1)
        return (x - self.mean) / self.std


def _to_tensor(image):
    return torch.from_numpy(np.asarray(image, np.float32) / 255.0).permute(2, 0, 1).contiguous()


class MedicalSegmentationDataset(torch.utils.data.Dataset):
    """dataset.py:65-89.  `.image_dir` / `.label_dir` are the two file lists (Segmentor.train_tissue_model_nnUNetv2 reads them)."""

    def __init__(self, image_dir_list, label_dir_list, transform=None, level=None):
        self.image_dir = image_dir_list
        self.label_dir = label_dir_list
        self.transform = transform
        self.level = level

    def __len__(self):
        return len(self.image_dir)

    def __getitem__(self, idx):
        from PIL import Image
        with Image.open(self.image_dir[idx]) as img:
            image = img.convert("RGB")
        image = self.transform(image) if self.transform else _to_tensor(image)
        mask = convert_labels(self.label_dir[idx], self.level)
        label = torch.tensor(mask, dtype=torch.uint8).unsqueeze(0)
        mask = torch.tensor(mask, dtype=torch.long)
        return image, mask, label


def split_indices(n, train_ratio):
    """ldiffusion.py:84-89: `random.shuffle` of range(n) on Python's global `random`, cut at int(n * train_ratio) -> (train indices, test indices)."""
    indices = list(range(n))
    random.shuffle(indices)
    split_index = int(n * train_ratio)
    return indices[:split_index], indices[split_index:]


def load_data(image_dir, label_dir, batch_size, level, train_ratio=0.7, world=1, rank=0, device=None, image_size=1024, io_workers=4, cache_bytes=DEFAULT_CACHE_BYTES):
    """ldiffusion.py:72-119 -> (train_loader, val_loader, train_sampler).  Sorted listings of both folders, equal lengths asserted, the split of
    `split_indices`; for world > 1 torch's DistributedSampler (training: shuffle=True, drop_last=True; validation: shuffle=False).  Training batches have
    `batch_size`, shuffled when there is no sampler, drop_last=True; validation has batch 1, unshuffled.  device=None: plain `DataLoader`s over the host
    dataset (num_workers=0); a device: `DeviceLoader`s, the same batches from a store on that device."""
    from torch.utils.data import DataLoader, DistributedSampler
    images = sorted([os.path.join(image_dir, f) for f in os.listdir(image_dir)])
    labels = sorted([os.path.join(label_dir, f) for f in os.listdir(label_dir)])
    assert len(images) == len(labels), f"image_dir holds {len(images)} files and label_dir {len(labels)}: the folders must pair up"
    train_indices, test_indices = split_indices(len(images), train_ratio)
    transform = default_transform(image_size)
    train_dataset = MedicalSegmentationDataset([images[i] for i in train_indices], [labels[i] for i in train_indices], transform, level)
    val_dataset = MedicalSegmentationDataset([images[i] for i in test_indices], [labels[i] for i in test_indices], transform, level)
    train_sampler = val_sampler = None
    if world > 1:
        train_sampler = DistributedSampler(train_dataset, num_replicas=world, rank=rank, shuffle=True, drop_last=True)
        val_sampler = DistributedSampler(val_dataset, num_replicas=world, rank=rank, shuffle=False, drop_last=False)
    if device is None:
        train_loader = DataLoader(train_dataset, batch_size=batch_size, shuffle=train_sampler is None, sampler=train_sampler, num_workers=0, drop_last=True)
        val_loader = DataLoader(val_dataset, batch_size=1, shuffle=False, sampler=val_sampler, num_workers=0)
    else:
        kw = dict(device=device, image_size=image_size, io_workers=io_workers, cache_bytes=cache_bytes)
        train_loader = DeviceLoader(train_dataset, batch_size=batch_size, shuffle=train_sampler is None, sampler=train_sampler, drop_last=True, **kw)
        val_loader = DeviceLoader(val_dataset, batch_size=1, shuffle=False, sampler=val_sampler, **kw)
    return train_loader, val_loader, train_sampler


# ---- the device side ---------------------------------------------------------------------------------------------------------------------------------
_weight_tables: dict = {}


def _weights_on(in_size, out_size, device):
    """(bounds int32 [out, 2], weights float32 [out, taps], taps) of `imgio.weights` on `device`, cached."""
    from . import imgio
    key = (in_size, out_size, str(device))
    t = _weight_tables.get(key)
    if t is None:
        bounds, w = imgio.weights(in_size, out_size)
        t = _weight_tables[key] = (torch.from_numpy(bounds.copy()).to(device), torch.from_numpy(w.astype(np.float32)).contiguous().to(device), w.shape[1])
    return t


def host_normalize_table(device):
    """`imgio.normalize_table(ImageNet)` evaluated on the CPU -- where `default_transform` evaluates the same expression -- and copied to `device`."""
    from . import imgio
    return imgio.normalize_table(IMAGENET_MEAN, IMAGENET_STD, "cpu").to(device)


def table_u8(x, table, out=None):
    """ldiff_op_label_table_u8: uint8 tensor on the GPU through a uint8 [256] table on the same device; `out` may be `x` (in place)."""
    from . import _lib
    import ctypes as C
    if not (isinstance(x, torch.Tensor) and x.dtype == torch.uint8 and x.is_cuda and x.is_contiguous()):
        raise ValueError("x: a contiguous uint8 tensor on the GPU")
    if not (isinstance(table, torch.Tensor) and table.dtype == torch.uint8 and table.numel() == 256 and table.device == x.device):
        raise ValueError("table: uint8 [256] on x's device")
    out = torch.empty_like(x) if out is None else out
    if not (out.dtype == torch.uint8 and out.shape == x.shape and out.device == x.device and out.is_contiguous()):
        raise ValueError("out: a contiguous uint8 tensor of x's shape on x's device")
    _lib.require_gpu()
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().ldiff_op_label_table_u8(_lib.ptr(x), _lib.ptr(out), C.c_int64(x.numel()), _lib.ptr(table.contiguous()), _lib.stream_ptr()))
    return out


def _check_store(cache, idx, ndim, what):
    if not (isinstance(cache, torch.Tensor) and cache.dtype == torch.uint8 and cache.is_cuda and cache.is_contiguous() and cache.dim() == ndim):
        raise ValueError(f"cache: a contiguous uint8 tensor {what} on the GPU")
    if not (isinstance(idx, torch.Tensor) and idx.dtype == torch.int32 and idx.dim() == 1 and idx.numel() >= 1 and idx.device == cache.device):
        raise ValueError("idx: int32 [B] on the cache's device")


def gather_labels(cache, idx):
    """ldiff_op_gather_labels: cache uint8 [N, H, W], idx int32 [B] -> (label uint8 [B, 1, H, W], mask int64 [B, H, W])."""
    from . import _lib
    _check_store(cache, idx, 3, "[N, H, W]")
    N, H, W = cache.shape
    B = idx.numel()
    label = torch.empty((B, 1, H, W), device=cache.device, dtype=torch.uint8)
    mask = torch.empty((B, H, W), device=cache.device, dtype=torch.int64)
    with torch.cuda.device(cache.device):
        _lib.check(_lib.load().ldiff_op_gather_labels(_lib.ptr(cache), N, H, W, _lib.ptr(idx), B, _lib.ptr(label), _lib.ptr(mask), _lib.stream_ptr()))
    return label, mask


def warmup_labels(cache, idx, size):
    """cache uint8 [N, H, W], idx int32 [B] -> uint8 [B, 1, oh, ow] = `F.interpolate(label.float(), (oh, ow), mode="bilinear", align_corners=False).to(uint8)`;
    size = (oh, ow).  Integer ratios: ldiff_op_warmup_labels, exact in integers.  Other sizes: the gathered labels through that torch expression on the device,
    the one the warm-up loop evaluates for a host loader."""
    import torch.nn.functional as F
    from . import _lib
    _check_store(cache, idx, 3, "[N, H, W]")
    N, H, W = cache.shape
    oh, ow = int(size[0]), int(size[1])
    if oh < 1 or ow < 1:
        raise ValueError(f"size = {size!r}: sides of at least 1")
    lib = _lib.load()
    if not lib.ldiff_op_warmup_labels_supported(H, W, oh, ow):
        label, _ = gather_labels(cache, idx)
        return F.interpolate(label.to(torch.float32), size=(oh, ow), mode="bilinear", align_corners=False).to(torch.uint8)
    B = idx.numel()
    out = torch.empty((B, 1, oh, ow), device=cache.device, dtype=torch.uint8)
    with torch.cuda.device(cache.device):
        _lib.check(lib.ldiff_op_warmup_labels(_lib.ptr(cache), N, H, W, _lib.ptr(idx), B, oh, ow, _lib.ptr(out), _lib.stream_ptr()))
    return out


def warmup_images(cache, idx, size, table):
    """ldiff_op_warmup_images: cache uint8 [N, Hs, Ws, 3], idx int32 [B], table float32 [3, 256] -> float32 [B, 3, oh, ow]: the table and the antialiased
    bilinear reduction (`F.interpolate(..., antialias=True)`'s weights, `imgio.weights`) in one pass over the stored bytes; size = (oh, ow)."""
    from . import _lib
    _check_store(cache, idx, 4, "[N, Hs, Ws, 3]")
    N, Hs, Ws, Cc = cache.shape
    if Cc != 3:
        raise ValueError(f"cache: {Cc} channels: 3")
    if not (isinstance(table, torch.Tensor) and table.dtype == torch.float32 and tuple(table.shape) == (3, 256) and table.device == cache.device and table.is_contiguous()):
        raise ValueError("table: contiguous float32 [3, 256] on the cache's device")
    oh, ow = int(size[0]), int(size[1])
    yb, yw, yt = _weights_on(Hs, oh, cache.device)   # a window above MAX_TAPS raises here, naming `size`
    xb, xw, xt = _weights_on(Ws, ow, cache.device)
    B = idx.numel()
    out = torch.empty((B, 3, oh, ow), device=cache.device, dtype=torch.float32)
    with torch.cuda.device(cache.device):
        _lib.check(_lib.load().ldiff_op_warmup_images(_lib.ptr(cache), N, Hs, Ws, _lib.ptr(idx), B, _lib.ptr(table), _lib.ptr(yb), _lib.ptr(yw), yt, _lib.ptr(xb), _lib.ptr(xw), xt,
                                                      oh, ow, _lib.ptr(out), _lib.stream_ptr()))
    return out


class DeviceLoader:
    """A `DataLoader` over a `MedicalSegmentationDataset` whose samples live on the GPU.  At construction every file is decoded once on `io_workers` threads
    (PIL only); each image goes through `imgio.resize_u8` to image_size^2 into `images` uint8 [N, S, S, 3], each label through the grey-level table on the
    device into `labels` uint8 [N, H, W].  Label files of unequal size raise ValueError naming the first offending file (the host loader's collate fails
    there too); a store above `cache_bytes` raises ValueError before anything is decoded: all or nothing.

    `.dataset` (the host dataset), `.sampler`, `.batch_size`, `len()` and iteration are a DataLoader's.  `__iter__` yields
    (image float32 [B, 3, S, S], mask int64 [B, H, W], label uint8 [B, 1, H, W]) on the device, bit-identical to the host loader's batches;
    `warmup_batches(size)` yields (image float32 [B, 3, size, size], label uint8 [B, 1, size, size]) in the same order with the same generator draws."""

    def __init__(self, dataset, batch_size=1, shuffle=False, sampler=None, drop_last=False, *, device, image_size=None, io_workers=4, cache_bytes=DEFAULT_CACHE_BYTES):
        from concurrent.futures import ThreadPoolExecutor
        from torch.utils.data import DataLoader
        from . import _lib, imgio
        from .utils import _image_size
        if isinstance(io_workers, bool) or not isinstance(io_workers, (int, np.integer)) or not 0 <= io_workers <= MAX_IO_WORKERS:
            raise ValueError(f"io_workers = {io_workers!r}: an integer in 0 .. {MAX_IO_WORKERS}")
        if image_size is None:
            image_size = getattr(dataset.transform, "size", None)
        S = imgio._side("image_size", image_size)
        if getattr(dataset.transform, "size", S) != S:
            raise ValueError(f"image_size = {S}: the dataset's transform resizes to {dataset.transform.size}")
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"device = {device}: a GPU (the host loader is load_data(device=None))")
        _lib.require_gpu()
        self.dataset, self.device, self.image_size = dataset, device, S
        N = len(dataset)
        # torch's own index order: a DataLoader over range(N) draws from the global generator what the host loader over the dataset draws
        self._index_loader = DataLoader(range(N), batch_size=batch_size, shuffle=shuffle, sampler=sampler, drop_last=drop_last, num_workers=0)
        self.sampler, self.batch_size, self.drop_last = self._index_loader.sampler, batch_size, drop_last
        table = torch.from_numpy(label_table(dataset.level)).to(device)   # a bad level raises before any file is read
        sizes = [_image_size(p) for p in dataset.label_dir]              # headers alone
        for p, s in zip(dataset.label_dir, sizes):
            if s != sizes[0]:
                raise ValueError(f"label {p}: {s[0]} x {s[1]}, but {dataset.label_dir[0]} is {sizes[0][0]} x {sizes[0][1]}: the labels of a loader have one size")
        W, H = sizes[0] if sizes else (1, 1)
        need = N * (S * S * 3 + H * W)
        if need > cache_bytes:
            raise ValueError(f"cache_bytes = {cache_bytes}: the store of {N} samples ({S} x {S} images, {H} x {W} labels) takes {need} bytes")
        self.images = torch.empty((N, S, S, 3), device=device, dtype=torch.uint8)
        self.labels = torch.empty((N, H, W), device=device, dtype=torch.uint8)
        self._table = host_normalize_table(device)
        pool = ThreadPoolExecutor(max_workers=int(io_workers), thread_name_prefix="ldiff-dataset") if io_workers else None
        try:
            ahead = max(2 * int(io_workers), 1)   # decoded files alive at a time
            jobs = {}

            def submit(i):
                if pool is not None:
                    jobs[i] = (pool.submit(_decode_rgb, dataset.image_dir[i]), pool.submit(_decode_grey, dataset.label_dir[i]))

            for i in range(min(ahead, N)):
                submit(i)
            for i in range(N):   # only the calling thread touches torch and the library
                if pool is not None:
                    fi, fl = jobs.pop(i)
                    rgb, grey = fi.result(), fl.result()
                    if i + ahead < N:
                        submit(i + ahead)
                else:
                    rgb, grey = _decode_rgb(dataset.image_dir[i]), _decode_grey(dataset.label_dir[i])
                if grey.shape != (H, W):
                    raise ValueError(f"label {dataset.label_dir[i]}: decoded to {grey.shape[1]} x {grey.shape[0]}, its header said {W} x {H}")
                self.images[i] = imgio.resize_u8(torch.from_numpy(rgb)[None].to(device), (S, S))[0]
                table_u8(torch.from_numpy(grey).to(device), table, out=self.labels[i])
        finally:
            if pool is not None:
                pool.shutdown(wait=True, cancel_futures=True)

    def __len__(self):
        return len(self._index_loader)

    def _index_batches(self):
        for idx in self._index_loader:   # int64 [B] on the host, from torch's default collate
            yield idx.to(self.device, dtype=torch.int32), idx.to(self.device)

    def __iter__(self):
        from . import imgio
        S = self.image_size
        for idx32, idx64 in self._index_batches():
            image = imgio._resize(self.images.index_select(0, idx64), (S, S), self._table)   # both sides unchanged: the table alone
            label, mask = gather_labels(self.labels, idx32)
            yield image, mask, label

    def warmup_batches(self, size=64):
        size = (size, size) if isinstance(size, (int, np.integer)) else tuple(size)
        for idx32, _ in self._index_batches():
            yield warmup_images(self.images, idx32, size, self._table), warmup_labels(self.labels, idx32, size)
