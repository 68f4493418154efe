"""Training batches for the nnU-Net tissue head, made on the device: what `nnUNetDataLoader2D` and the transforms of
`nnUNetTrainer.get_training_transforms` (nnUNetTrainer.py:674-765) do on a pool of CPU workers, for cases that stay in device memory.

    CaseStore      preprocessed cases in ONE device arena: normalised image, its cubic B-spline coefficients, labels, foreground locations; built on the
                   host, or with `build="device"` by the case kernels below (crop to non-zero, statistics, normalisation, foreground locations)
    case_bbox, case_stats, case_counts, case_rank_to_coord   DefaultPreprocessor.run_case_npy's per-case scans on the device (ldiff_op_case_*)
    draw_batch     every random decision of a batch, on the host, as two parameter tables (numpy structured arrays = the C structs of include/ldiff.h)
    PatchLoader    iterator of {"data": [B, C, h, w] float32, "target": [n_scales x [B, 1, h_k, w_k] uint8]} -- what nnunet_train.Trainer takes.
                   Per batch: one pinned upload of the tables and two launches (ldiff_op_seg_sample, ldiff_op_seg_intensity); nothing synchronises.

With `lowres=True` (draw_sample, draw_batch, augment_intensity_, PatchLoader) the chain is nnU-Net's whole chain: SimulateLowResolutionTransform is
drawn into the table slot `lowres_zoom` and applied between contrast and the gammas by ldiff_op_seg_intensity_lr.  The default, `lowres=False`, is the
chain minus that transform, byte for byte what it was.  The bodies of the transforms live in `batchgenerators`, restated here
from the public package; each rule sits in one function whose docstring names the class it mirrors.

One deliberate difference: nnU-Net crops `initial_patch_size` on the CPU, pads it and transforms that crop; here the kernel samples the case itself, so it
sees the case's pixels where nnU-Net sees the intermediate crop's pad, and the spline coefficients are those of the whole case.  The crop centre, the
admissible crop positions and "outside the case is 0 / background" are nnU-Net's.

Order of draws (ours; `numpy.random`'s legacy stream is not reproduced).  Per sample (`draw_sample`), from the caller's Generator, with or without
`train`:
    1. integers: the case index
    2. integers: the class among those present, then the voxel among its recorded locations (a forced sample of a case with foreground), or the crop's
       first row, then its first column (every other sample).  A store with an ignore label (get_bbox, base_data_loader.py:84-135): a sample that is
       not forced draws ONE voxel among the case's annotated locations instead, and row and column only when the case has none
    3. random(8): rotation gate, angle; scale gate, coin, scale below 1, scale above 1; mirror of axis 0, of axis 1
    4. random(2): noise gate, noise sigma;  integers: the Philox offset
    5. random(5): the per-sample gates of blur, brightness, contrast, gamma on -x, gamma
    6. random((C, 12)): per channel  blur coin, blur sigma | brightness | contrast coin, below 1, above 1 | gamma on -x coin, below 1, above 1 |
       gamma coin, below 1, above 1
    7. only with `lowres=True`: random(1): the per-sample gate of the low-resolution simulation; random((C, 2)): per channel its coin and zoom
A value behind a closed gate, or the unused side of a coin, is drawn and dropped, so a sample always consumes the same count after step 2.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, nnunet

# the C structs of include/ldiff.h (ldiff_seg_case / ldiff_seg_sample / ldiff_seg_chan), field for field
CASE_DTYPE = np.dtype([("coef_off", "<i8"), ("raw_off", "<i8"), ("label_off", "<i8"), ("H", "<i4"), ("W", "<i4"), ("stride", "<i4"), ("label_stride", "<i4")])
SAMPLE_DTYPE = np.dtype([("m", "<f4", (6,)), ("case_index", "<i4"), ("copy", "<i4"), ("noise_sigma", "<f4"), ("reserved", "<u4"), ("philox_offset", "<u8")])
CHAN_DTYPE = np.dtype([("blur_sigma", "<f4"), ("brightness", "<f4"), ("contrast", "<f4"), ("lowres_zoom", "<f4"), ("gamma_inverted", "<f4"), ("gamma", "<f4")])
MAX_SCALES = 8

# nnUNetTrainer.get_training_transforms (:698-727)
P_ROTATION, P_SCALE, SCALE_RANGE = 0.2, 0.2, (0.7, 1.4)
P_NOISE, NOISE_SIGMA = 0.1, (0.0, 0.1)
P_BLUR, P_BLUR_PER_CHANNEL, BLUR_SIGMA = 0.2, 0.5, (0.5, 1.0)
P_BRIGHTNESS, BRIGHTNESS = 0.15, (0.75, 1.25)
P_CONTRAST, CONTRAST = 0.15, (0.75, 1.25)
P_GAMMA_INVERTED, P_GAMMA, GAMMA = 0.1, 0.3, (0.7, 1.5)
P_MIRROR = 0.5
P_LOWRES, P_LOWRES_PER_CHANNEL, LOWRES_ZOOM = 0.25, 0.5, (0.5, 1.0)   # SimulateLowResolutionTransform (:719-722)
OVERSAMPLE_FOREGROUND = 0.33   # nnUNetTrainer.oversample_foreground_percent
SPLINE_PAD = 12                # edge samples a side around the down-sampled plane before its prefilter (scipy's 'nearest' spline extension)


def lowres_shape(patch: Sequence[int], zoom) -> Tuple[int, int]:
    """SimulateLowResolutionTransform's target shape of an [h, w] plane, np.round(shape * zoom), formed as the kernel forms it: the float32 product
    rounded half to even."""
    z = np.float32(zoom)
    return int(np.rint(np.float32(int(patch[0])) * z)), int(np.rint(np.float32(int(patch[1])) * z))


def rotate_coords_2d(coords: np.ndarray, angle: float) -> np.ndarray:
    """batchgenerators.augmentations.utils.rotate_coords_2d: coords [2, ...] times the plain rotation [[cos, -sin], [sin, cos]] from the right,
    (r, c) -> (r cos + c sin, -r sin + c cos)."""
    coords = np.asarray(coords, dtype=np.float64)
    rot = np.array([[math.cos(angle), -math.sin(angle)], [math.sin(angle), math.cos(angle)]])
    return np.dot(coords.reshape(2, -1).transpose(), rot).transpose().reshape(coords.shape)


def rotation_range(patch_size: Sequence[int]) -> float:
    """nnUNetTrainer.configure_rotation_dummyDA_mirroring_and_inital_patch_size (:382-397), 2-D: the half-width r of U(-r, r), pi or 15 degrees."""
    if len(patch_size) != 2:
        raise ValueError(f"rotation_range: 2-D patches only, got {tuple(patch_size)}")
    return 15.0 / 360 * 2.0 * np.pi if max(patch_size) / min(patch_size) > 1.5 else 180.0 / 360 * 2.0 * np.pi


def initial_patch_size(patch_size: Sequence[int]) -> Tuple[int, int]:
    """compute_initial_patch_size.get_patch_size(patch, rot, 0, 0, (0.85, 1.25)) for two dimensions: the extent the patch reaches when turned by
    min(r, 90 degrees), over 0.85, truncated."""
    rot = min(90 / 360 * 2.0 * np.pi, abs(rotation_range(patch_size)))
    coords = np.array(patch_size, dtype=np.float64)
    shape = np.max(np.vstack((np.abs(rotate_coords_2d(coords, rot)), coords)), 0)
    shape /= 0.85
    return tuple(int(v) for v in shape.astype(int))


def spline_coefficients(img: np.ndarray) -> np.ndarray:
    """scipy.ndimage.spline_filter(img, order=3, mode='mirror') over the last two axes, in float64: per axis the recursive filter with pole sqrt(3) - 2 and
    gain 6, the causal pass started from the whole-sample-mirrored sum, the anti-causal pass from its closed form; vectorised over the other axes."""
    out = np.array(img, dtype=np.float64)
    pole = math.sqrt(3.0) - 2.0
    for axis in (-2, -1):
        c = np.moveaxis(out, axis, 0)   # a view: the passes below write through it
        n = c.shape[0]
        if n == 1:
            continue
        c *= (1.0 - pole) * (1.0 - 1.0 / pole)
        horizon = n if n < 64 else 64   # |pole|^64 = 2e-37
        if horizon < n:
            acc = sum((pole ** k) * c[k] for k in range(horizon))
        else:   # the exact sum over one period 2 n - 2 of the mirrored signal
            acc = c[0] + (pole ** (n - 1)) * c[n - 1]
            for k in range(1, n - 1):
                acc = acc + (pole ** k + pole ** (2 * n - 2 - k)) * c[k]
            acc = acc / (1.0 - pole ** (2 * n - 2))
        c[0] = acc
        for k in range(1, n):
            c[k] += pole * c[k - 1]
        c[n - 1] = (pole / (pole * pole - 1.0)) * (c[n - 1] + pole * c[n - 2])
        for k in range(n - 2, -1, -1):
            c[k] = pole * (c[k + 1] - c[k])
    return out


def _target_num_samples(count: int) -> int:
    """default_preprocessor.py:171-172: at most 10,000 locations, at least 1 % of the class."""
    return max(min(10000, count), int(np.ceil(count * 0.01)))


def annotated_key(n_heads: int) -> Tuple[int, ...]:
    """The key of the annotated pixels in `class_locations` of a dataset with an ignore label: tuple(LabelManager.all_labels), every class, background
    included (default_preprocessor.py:99-102; nnUNetDataLoaderBase.annotated_classes_key)."""
    return tuple(range(int(n_heads)))


def sample_foreground_locations(seg: np.ndarray, classes: Sequence[int], seed: int = 1234, annotated: Optional[int] = None) -> dict:
    """DefaultPreprocessor._sample_foreground_locations (default_preprocessor.py:152-178) for plain labels of one [H, W] map: per class a subset of
    np.argwhere(seg == c) chosen without replacement by ONE RandomState(seed) walked through the classes in order; an absent class gets [].
    `annotated` = n_heads of a dataset with an ignore label: one more entry after the classes, key `annotated_key(n_heads)`, drawn by the same
    walk from the pixels of any class 0 .. n_heads - 1 (:99-102), so the entries before it are what they are without it.
    Region labels: `classes` holds LabelManager.foreground_regions (tuples, or single integers), which key the entries as nnU-Net's class_locations are
    keyed; `annotated` is then the key itself, tuple(all_labels)."""
    rndst = np.random.RandomState(seed)
    out = {}
    for c in list(classes) + ([annotated if isinstance(annotated, tuple) else annotated_key(annotated)] if annotated is not None else []):
        key = c if isinstance(c, tuple) else int(c)
        locs = np.argwhere(np.isin(seg, c) if isinstance(c, tuple) else seg == c)
        if len(locs) == 0:
            out[key] = []
            continue
        out[key] = locs[rndst.choice(len(locs), _target_num_samples(len(locs)), replace=False)]
    return out


class CaseStore:
    """Preprocessed training cases resident on the device.  `cases`: pairs (image [C, H, W] uint8 or float32, label map [H, W] of integers); sizes may
    differ.  Each image is normalised by `nnunet.normalize(schemes)`; the arena holds, per case and 16-byte aligned, the cubic B-spline coefficients
    (float32 [C, H, W]), the normalised image itself (float32 [C, H, W], what an unmodified sample copies) and the labels (uint8 [H, W]); `table` is the
    per-case ldiff_seg_case row (offsets, H, W, row strides).  `class_locations[i]`: {class: [n, 2] (row, column)} for the foreground classes
    1 .. n_heads - 1.  `labels`: a dataset.json `labels` mapping, looked at to refuse what the tissue head does not cover and for nnU-Net's ignore
    label (`nnunet.label_spec`; it must equal `n_heads`): the label maps may then carry that value, `ignore_label` holds it (None otherwise), and
    every `class_locations[i]` ends with the entry `annotated_key(n_heads)`, the sampled pixels of any class, which `draw_crop` centres samples on.
    `device="cpu"` keeps the arena on the host: enough for `draw_batch`, not for a PatchLoader.
    `prefilter`: "host" (the default) forms the coefficients by `spline_coefficients` in float64 and rounds them once; "device" uploads the normalised
    image in their place and filters it there (`spline_prefilter_`), so the coefficients carry the float32 filter's own error, a few 1e-6 of the
    image's magnitude (tests/nnunet_lowres_ref.py bounds it), and building the store needs the GPU.
    `build`: "host" (the default) normalises each case on the CPU and finds the foreground with np.argwhere; it does NOT crop to non-zero unless
    `crop=True` (default False: the case is stored whole, as it always was).  "device" takes the same pairs on the device or the host and runs the case
    kernels (ldiff_op_case_*): it CROPS TO NON-ZERO as DefaultPreprocessor.run_case_npy does, forms mean / std / min / max on the host in float64 from the
    kernels' exact sums, normalises into the arena, and fills `class_locations` with what `sample_foreground_locations` returns -- the RandomState is
    walked on the host over the per-class counts, the chosen ranks become pixels on the device.  Pixels that crop_to_nonzero would relabel -1 (background
    outside the non-zero mask) stay 0 in both builds: nnU-Net's RemoveLabelTransform(-1, 0) makes them 0 before the loss.  `boxes[i]`: the crop box
    (y0, y1, x0, x1) of case i in its source image (the full extent without a crop)."""

    def __init__(self, cases, schemes: Sequence[str], n_heads: int, device="cuda:0", labels: Optional[dict] = None, prefilter: str = "host",
                 build: str = "host", crop: bool = False, regions: Optional[dict] = None):
        """`regions`: a `nnunet.region_spec` result -- region labels.  The label maps keep their label values (the loss looks membership up in the
        spec's table); `n_heads` is the number of regions; `class_locations` is keyed by the foreground regions, as nnU-Net's is, and with an ignore label
        ends with the annotated key tuple(all_labels).  `labels=` keeps refusing regions."""
        if prefilter not in ("host", "device"):
            raise ValueError(f"CaseStore: prefilter must be 'host' or 'device', got {prefilter!r}")
        if prefilter == "device" and torch.device(device).type != "cuda":
            raise ValueError("CaseStore: prefilter='device' needs the store on a GPU")
        if build not in ("host", "device"):
            raise ValueError(f"CaseStore: build must be 'host' or 'device', got {build!r}")
        if build == "device" and torch.device(device).type != "cuda":
            raise ValueError("CaseStore: build='device' needs the store on a GPU")
        self.ignore_label = None
        if labels is not None:
            heads, self.ignore_label = nnunet.label_spec(labels)
            if self.ignore_label is not None and heads != int(n_heads):
                raise ValueError(f"CaseStore: `labels` names {heads} classes and the ignore label {self.ignore_label}, n_heads is {n_heads}")
        self.regions = None if regions is None else list(regions["foreground_regions"])
        if regions is not None:
            if labels is not None:
                raise ValueError("CaseStore: `labels` and `regions` exclude each other (`regions` carries the ignore label)")
            if int(n_heads) != int(regions["n_heads"]):
                raise ValueError(f"CaseStore: `regions` defines {regions['n_heads']} regions, n_heads is {n_heads}")
            self.ignore_label = regions["ignore_label"]
            self.region_table = np.asarray(regions["table"], dtype=np.uint32)
            self._top = int(regions["all_labels"][-1]) + 1          # label values run over [0, _top), and _top is the ignore label where there is one
            self.annotated = tuple(int(v) for v in regions["all_labels"]) if self.ignore_label is not None else None
        else:
            self._top = int(n_heads)
            self.annotated = annotated_key(n_heads) if self.ignore_label is not None else None
        lo, hi = (1, nnunet.REGION_MAX) if regions is not None else (2, 32)
        if not lo <= int(n_heads) <= hi:
            raise ValueError(f"CaseStore: n_heads {n_heads} out of range [{lo}, {hi}]")
        cases = list(cases)
        if not cases:
            raise ValueError("CaseStore: no cases")
        self.n_heads, self.schemes = int(n_heads), list(schemes)
        self.device = torch.device(device)
        self.table = np.zeros(len(cases), CASE_DTYPE)
        self.class_locations: List[dict] = []
        self.boxes: List[Tuple[int, int, int, int]] = []
        parts, size = [], 0
        self.channels = None
        if build == "device":
            self._build_on_device(cases, prefilter)
            return
        for i, (img, seg) in enumerate(cases):
            img, seg = torch.as_tensor(img), np.asarray(torch.as_tensor(seg).cpu())
            if img.dim() != 3 or img.dtype not in (torch.uint8, torch.float32):
                raise ValueError(f"CaseStore: case {i}: the image must be [C, H, W] uint8 or float32, got {tuple(img.shape)} of {img.dtype}")
            Cc, H, W = (int(v) for v in img.shape)
            if self.channels is None:
                self.channels = Cc
            if Cc != self.channels or Cc != len(self.schemes):
                raise ValueError(f"CaseStore: case {i} has {Cc} channels; the store has {self.channels} and {len(self.schemes)} normalisation schemes")
            if seg.shape != (H, W) or seg.dtype.kind not in "iu":
                raise ValueError(f"CaseStore: case {i}: the label map must be [{H}, {W}] of integers, got {seg.shape} of {seg.dtype}")
            box = nnunet.nonzero_bbox(img) if crop else (0, H, 0, W)
            self.boxes.append(box)
            if crop:
                img, seg = img[:, box[0]:box[1], box[2]:box[3]], seg[box[0]:box[1], box[2]:box[3]]
                H, W = box[1] - box[0], box[3] - box[2]
            top = self._top if self.ignore_label is None else self._top + 1   # the ignore label is the one value past the classes
            if seg.min() < 0 or seg.max() >= top:
                bad = sorted(int(v) for v in np.unique(seg) if v < 0 or v >= top)
                raise ValueError(f"CaseStore: case {i}: labels {bad[:5]} outside [0, {self._top})")
            self._check_region_values(i, seg)
            raw = nnunet.normalize(img.cpu().to(torch.float32), self.schemes).numpy()
            coef = spline_coefficients(raw).astype(np.float32) if prefilter == "host" else raw
            row = self.table[i]
            row["H"], row["W"], row["stride"], row["label_stride"] = H, W, W, W
            for key, arr in (("coef_off", coef), ("raw_off", raw), ("label_off", seg.astype(np.uint8))):
                size = (size + 15) // 16 * 16
                row[key] = size
                parts.append((size, np.ascontiguousarray(arr).view(np.uint8).reshape(-1)))
                size += parts[-1][1].size
            self.class_locations.append(sample_foreground_locations(seg, self.regions if self.regions is not None else range(1, self.n_heads),
                                                                    annotated=self.annotated if self.regions is not None else
                                                                    (None if self.ignore_label is None else self.n_heads)))
        host = np.zeros((size + 15) // 16 * 16, np.uint8)
        for off, arr in parts:
            host[off:off + arr.size] = arr
        self.arena = torch.from_numpy(host).to(self.device)
        if prefilter == "device":
            for i in range(len(cases)):
                spline_prefilter_(self.coefficients(i))
        self.cases_dev = torch.from_numpy(self.table.view(np.uint8).reshape(-1).copy()).to(self.device)

    def _check_region_values(self, i: int, seg) -> None:
        """Region labels: a value below the top that is no label of the dataset (the table's bit 30) is refused like one outside the range."""
        if self.regions is None:
            return
        values = np.unique(seg.cpu().numpy() if torch.is_tensor(seg) else seg)
        bad = sorted(int(v) for v in values if self.region_table[int(v)] & (1 << 30))
        if bad:
            raise ValueError(f"CaseStore: case {i}: labels {bad[:5]} are no labels of the dataset")

    def _build_on_device(self, cases, prefilter: str):
        """build="device": the case kernels in three rounds with one synchronisation each -- boxes; statistics and label counts over the boxes; then the
        arena is laid out, every case normalised into it and the sampled foreground ranks turned into pixels."""
        dev, nh = self.device, self._top   # the label values counted: the classes, or with regions every value up to the highest label
        ign = self.ignore_label is not None
        counted = nh + 1 if ign else nh   # the ignore label is counted as one more class, so that "no class and not ignored" keeps its own count
        imgs, segs, given = [], [], []
        for i, (img, seg) in enumerate(cases):
            img, seg = torch.as_tensor(img), torch.as_tensor(seg)
            if img.dim() != 3 or img.dtype not in (torch.uint8, torch.float32):
                raise ValueError(f"CaseStore: case {i}: the image must be [C, H, W] uint8 or float32, got {tuple(img.shape)} of {img.dtype}")
            Cc, H, W = (int(v) for v in img.shape)
            if self.channels is None:
                self.channels = Cc
            if Cc != self.channels or Cc != len(self.schemes):
                raise ValueError(f"CaseStore: case {i} has {Cc} channels; the store has {self.channels} and {len(self.schemes)} normalisation schemes")
            if tuple(seg.shape) != (H, W) or seg.dtype.is_floating_point or seg.dtype in (torch.bool, torch.complex64, torch.complex128):
                raise ValueError(f"CaseStore: case {i}: the label map must be [{H}, {W}] of integers, got {tuple(seg.shape)} of {seg.dtype}")
            img, seg = img.to(dev), seg.to(dev)
            given.append(seg)
            if seg.dtype != torch.uint8:   # any other integer type: what does not fit a byte becomes 255, which no head count reaches
                seg = torch.where((seg < 0) | (seg > 255), torch.full_like(seg, 255), seg).to(torch.uint8)
            imgs.append(img if img.stride(-1) == 1 else img.contiguous())
            segs.append(seg if seg.stride(-1) == 1 else seg.contiguous())
        n = len(imgs)
        with torch.cuda.device(dev):
            boxes_dev = torch.empty((n, 4), dtype=torch.int32, device=dev)
            for i in range(n):
                _launch_case_bbox(imgs[i], boxes_dev[i])
            self.boxes = [tuple(int(v) for v in b) for b in boxes_dev.cpu().numpy()]
            stats_dev = torch.empty((n, self.channels, 4), dtype=torch.int64, device=dev)
            totals_dev = torch.empty((n, counted + (3 if ign else 2)), dtype=torch.int32, device=dev)
            ws = torch.empty(max(int(_lib.load().ldiff_op_case_stats_ws_bytes(self.channels)), 16), dtype=torch.uint8, device=dev)
            prefixes = []
            for i in range(n):
                _launch_case_stats(imgs[i], self.boxes[i], stats_dev[i], ws)
                prefixes.append(_launch_case_counts(segs[i], self.boxes[i], counted, totals_dev[i], nh if ign else None)[1])
            stats, totals = stats_dev.cpu().numpy(), totals_dev.cpu().numpy().astype(np.int64)
            size = 0
            norm = []
            for i in range(n):
                if totals[i, counted + 1]:
                    b = self.boxes[i]
                    bad = sorted(int(v) for v in torch.unique(given[i][b[0]:b[1], b[2]:b[3]]).cpu() if v < 0 or v >= counted)   # the error path alone looks at values
                    raise ValueError(f"CaseStore: case {i}: labels {bad[:5]} outside [0, {nh})")
                h, w = self.boxes[i][1] - self.boxes[i][0], self.boxes[i][3] - self.boxes[i][2]
                norm.append(normalization_scalars(stats[i], imgs[i].dtype, h * w, self.schemes))
                row = self.table[i]
                row["H"], row["W"], row["stride"], row["label_stride"] = h, w, w, w
                for key, nbytes in (("coef_off", self.channels * h * w * 4), ("raw_off", self.channels * h * w * 4), ("label_off", h * w)):
                    size = (size + 15) // 16 * 16
                    row[key] = size
                    size += nbytes
            self.arena = torch.zeros((size + 15) // 16 * 16, dtype=torch.uint8, device=dev)
            for i in range(n):
                _launch_case_apply(imgs[i], segs[i], self.boxes[i], norm[i][0], norm[i][1], self.arena, self.table[i], prefilter == "device")
                if prefilter == "device":
                    spline_prefilter_(self.coefficients(i))
                else:
                    self.coefficients(i).copy_(torch.from_numpy(spline_coefficients(self.raw(i).cpu().numpy()).astype(np.float32)))
            if self.regions is not None:   # the membership table on the device, once for all cases
                member_table = torch.from_numpy(self.region_table.astype(np.int64)).to(dev)
                plane_totals = torch.empty(4, dtype=torch.int32, device=dev)
            for i in range(n):   # sample_foreground_locations: ONE RandomState per case walked through the classes; only the counts are needed here
                rndst, picked = np.random.RandomState(1234), {}
                if self.regions is not None:   # per region its binary membership plane, once: a gather through the table, then the class kernels with selector 1
                    b = self.boxes[i]
                    member = member_table[segs[i].long()]
                    if bool((member[b[0]:b[1], b[2]:b[3]] & (1 << 30)).any()):   # one reduction on the device; the error path alone looks at values
                        self._check_region_values(i, segs[i][b[0]:b[1], b[2]:b[3]])
                    for r, region in enumerate(self.regions):
                        plane = ((member >> r) & 1).to(torch.uint8).contiguous()
                        prefix = _launch_case_counts(plane, self.boxes[i], 2, plane_totals)[1]
                        count = int(plane_totals[1])
                        picked[region] = [] if count == 0 else _launch_case_rank(
                            plane, self.boxes[i], 1, prefix[1], torch.from_numpy(rndst.choice(count, _target_num_samples(count), replace=False).astype(np.int64)).to(dev),
                            None)[0]
                for c in (range(1, nh) if self.regions is None else ()):
                    count = int(totals[i, c])
                    if count == 0:
                        picked[c] = []
                        continue
                    ranks = torch.from_numpy(rndst.choice(count, _target_num_samples(count), replace=False).astype(np.int64)).to(dev)
                    picked[c] = _launch_case_rank(segs[i], self.boxes[i], c, prefixes[i][c], ranks, None)[0]
                if ign:   # the same walk goes on to the annotated pixels, `label < n_heads`: the selector -1 - n_heads, its prefix the table's last row
                    count = int(totals[i, counted + 2])
                    picked[self.annotated] = [] if count == 0 else _launch_case_rank(
                        segs[i], self.boxes[i], -1 - nh, prefixes[i][counted + 1],
                        torch.from_numpy(rndst.choice(count, _target_num_samples(count), replace=False).astype(np.int64)).to(dev), None)[0]
                self.class_locations.append({c: (v if isinstance(v, list) else v.cpu().numpy().astype(np.int64)) for c, v in picked.items()})
        self.cases_dev = torch.from_numpy(self.table.view(np.uint8).reshape(-1).copy()).to(dev)

    def __len__(self):
        return len(self.table)

    def shape(self, i: int) -> Tuple[int, int]:
        return int(self.table[i]["H"]), int(self.table[i]["W"])

    def _plane(self, key: str, i: int) -> torch.Tensor:
        H, W = self.shape(i)
        off = int(self.table[i][key])
        return self.arena[off:off + self.channels * H * W * 4].view(torch.float32).view(self.channels, H, W)

    def raw(self, i: int) -> torch.Tensor:
        """The normalised image of case i, float32 [C, H, W] (a view of the arena)."""
        return self._plane("raw_off", i)

    def coefficients(self, i: int) -> torch.Tensor:
        return self._plane("coef_off", i)

    def labels(self, i: int) -> torch.Tensor:
        H, W = self.shape(i)
        off = int(self.table[i]["label_off"])
        return self.arena[off:off + H * W].view(H, W)


def crop_bounds(shape: Sequence[int], loader_patch: Sequence[int], final_patch: Sequence[int]) -> Tuple[List[int], List[int]]:
    """nnUNetDataLoaderBase.get_bbox (base_data_loader.py:68-80): the lowest and highest admissible first index of the loader's crop per axis;
    need_to_pad = loader patch - final patch, widened where the case is smaller than the loader's patch."""
    lbs, ubs = [], []
    for d in range(2):
        pad = int(loader_patch[d]) - int(final_patch[d])
        if pad + shape[d] < loader_patch[d]:
            pad = loader_patch[d] - shape[d]
        lbs.append(-pad // 2)
        ubs.append(shape[d] + pad // 2 + pad % 2 - loader_patch[d])
    return lbs, ubs


def do_oversample(sample_idx: int, batch_size: int, oversample: float) -> bool:
    """nnUNetDataLoaderBase._oversample_last_XX_percent (base_data_loader.py:45-49)."""
    return not sample_idx < round(batch_size * (1 - oversample))


def _two_sided(coin: float, low: float, high: float, lo: float, mid: float, hi: float) -> float:
    """batchgenerators' `if random() < 0.5: U(lo, mid) else: U(mid, hi)` with the two uniforms already drawn in [0, 1)."""
    return lo + low * (mid - lo) if coin < 0.5 else mid + high * (hi - mid)


def draw_crop(rng: np.random.Generator, store: CaseStore, sample_idx: int, batch_size: int, patch_size: Sequence[int], loader_patch: Sequence[int],
              oversample: float = OVERSAMPLE_FOREGROUND) -> dict:
    """The case and the loader's crop of one sample (nnUNetDataLoader2D.generate_train_batch + get_bbox): the case index, whether the sample is forced
    onto foreground, the bounds, the chosen voxel (None for a free crop) and the crop's first index `bbox_lbs`.
    Draws: case index; then class and voxel (forced, and the case has foreground) or row and column of the crop.
    A store with an ignore label (get_bbox :84-135, has_ignore): a sample that is not forced takes one of the case's annotated locations as its
    centre (one draw, the voxel) and falls back to the free crop when the case has none; a forced sample chooses among the entries present with
    the annotated key taken out whenever another entry is there."""
    ci = int(rng.integers(len(store)))
    lbs, ubs = crop_bounds(store.shape(ci), loader_patch, patch_size)
    forced = do_oversample(sample_idx, batch_size, oversample)
    eligible = [c for c, locs in store.class_locations[ci].items() if len(locs) > 0]
    voxel = None
    has_ignore = getattr(store, "ignore_label", None) is not None
    if has_ignore:
        key = getattr(store, "annotated", None) or annotated_key(store.n_heads)   # with regions: tuple(all_labels)
        if not forced:
            eligible = [key] if key in eligible else []
        elif key in eligible and len(eligible) > 1:
            eligible.remove(key)
    if (forced or has_ignore) and eligible:   # get_bbox (:95-132): a class among those present, one of its recorded voxels as the centre
        chosen = eligible[int(rng.integers(len(eligible)))] if forced else eligible[0]   # not forced: the annotated key by rule, nothing to draw
        locs = store.class_locations[ci][chosen]
        voxel = [int(v) for v in locs[int(rng.integers(len(locs)))]]
        bbox = [max(lbs[d], voxel[d] - loader_patch[d] // 2) for d in range(2)]
    else:                     # :85 / :135: anywhere between the bounds (a forced sample of a case without foreground falls back to this)
        bbox = [int(rng.integers(lbs[d], ubs[d] + 1)) for d in range(2)]
    return dict(case=ci, forced=forced, voxel=voxel, lbs=lbs, ubs=ubs, bbox_lbs=bbox, loader_patch=tuple(int(v) for v in loader_patch))


def draw_sample(rng: np.random.Generator, store: CaseStore, sample_idx: int, batch_size: int, patch_size: Sequence[int], train: bool = True,
                oversample: float = OVERSAMPLE_FOREGROUND, lowres: bool = False):
    """Every random decision of one sample, in the module docstring's order: (a SAMPLE_DTYPE record, [C] CHAN_DTYPE records, `draw_crop`'s dict).
    The same numbers are drawn with `train=False`; they are then not used.  `lowres`: step 7, the low-resolution simulation's 1 + 2 C numbers, after
    the others; without it nothing more is drawn and `lowres_zoom` stays 0."""
    h, w = int(patch_size[0]), int(patch_size[1])
    Cc = store.channels
    loader_patch = initial_patch_size((h, w)) if train else (h, w)
    s = np.zeros((), SAMPLE_DTYPE)
    chans = np.zeros(Cc, CHAN_DTYPE)
    chans["brightness"] = 1.0
    crop = draw_crop(rng, store, sample_idx, batch_size, (h, w), loader_patch, oversample)

    u = rng.random(8)   # rotation gate, angle; scale gate, coin, scale below 1, scale above 1; mirror axis 0, axis 1
    rotate, scale = train and u[0] < P_ROTATION, train and u[2] < P_SCALE
    angle = (2.0 * u[1] - 1.0) * rotation_range((h, w)) if rotate else 0.0
    zoom = _two_sided(u[3], u[4], u[5], SCALE_RANGE[0], 1.0, SCALE_RANGE[1]) if scale else 1.0
    flip = [train and u[6] < P_MIRROR, train and u[7] < P_MIRROR]
    s["case_index"] = crop["case"]
    s["m"], s["copy"] = spatial_matrix((h, w), loader_patch, crop["bbox_lbs"], angle, zoom, flip, modified=bool(rotate or scale))
    noise_gate, noise_u = rng.random(2)
    s["philox_offset"] = int(rng.integers(0, 1 << 62))
    gates = rng.random(5)                # blur, brightness, contrast, inverted gamma, gamma: one gate per sample
    per_channel = rng.random((Cc, 12))   # per channel: blur (coin, sigma), brightness, contrast (coin, low, high), gamma on -x (3), gamma (3)
    if lowres:
        lowres_gate, lowres_u = rng.random(1)[0], rng.random((Cc, 2))   # the sample's gate; per channel: coin, zoom
    if not train:
        return s, chans, crop
    s["noise_sigma"] = NOISE_SIGMA[0] + noise_u * (NOISE_SIGMA[1] - NOISE_SIGMA[0]) if noise_gate < P_NOISE else 0.0
    for c in range(Cc):
        v, ch = per_channel[c], chans[c]
        if gates[0] < P_BLUR and v[0] < P_BLUR_PER_CHANNEL:
            ch["blur_sigma"] = BLUR_SIGMA[0] + v[1] * (BLUR_SIGMA[1] - BLUR_SIGMA[0])
        if gates[1] < P_BRIGHTNESS:
            ch["brightness"] = BRIGHTNESS[0] + v[2] * (BRIGHTNESS[1] - BRIGHTNESS[0])
        if gates[2] < P_CONTRAST:
            ch["contrast"] = _two_sided(v[3], v[4], v[5], CONTRAST[0], 1.0, CONTRAST[1])
        if gates[3] < P_GAMMA_INVERTED:
            ch["gamma_inverted"] = _two_sided(v[6], v[7], v[8], GAMMA[0], 1.0, GAMMA[1])
        if gates[4] < P_GAMMA:
            ch["gamma"] = _two_sided(v[9], v[10], v[11], GAMMA[0], 1.0, GAMMA[1])
        if lowres and lowres_gate < P_LOWRES and lowres_u[c, 0] < P_LOWRES_PER_CHANNEL:
            ch["lowres_zoom"] = LOWRES_ZOOM[0] + lowres_u[c, 1] * (LOWRES_ZOOM[1] - LOWRES_ZOOM[0])
    return s, chans, crop


def draw_batch(rng: np.random.Generator, store: CaseStore, batch_size: int, patch_size: Sequence[int], train: bool = True,
               oversample: float = OVERSAMPLE_FOREGROUND, lowres: bool = False):
    """The random decisions of one batch, sample after sample (`draw_sample`): (samples [B] of SAMPLE_DTYPE, channels [B, C] of CHAN_DTYPE).
    `train=False`: no augmentation, the loader's patch is the final patch (need_to_pad = 0), every sample an exact crop.  `lowres`: also draw the
    low-resolution simulation (`draw_sample`'s step 7)."""
    samples = np.zeros(batch_size, SAMPLE_DTYPE)
    chans = np.zeros((batch_size, store.channels), CHAN_DTYPE)
    for b in range(batch_size):
        samples[b], chans[b], _ = draw_sample(rng, store, b, batch_size, patch_size, train, oversample, lowres)
    return samples, chans


def spatial_matrix(patch, loader_patch, bbox_lbs, angle: float, zoom: float, flip, modified: bool):
    """SpatialTransform(random_crop=False, no elastic deformation) + MirrorTransform as one map from the patch index to the case coordinate, float32
    [m00 m01 m02 m10 m11 m12], and the copy flag.  The centred grid g = (i - (h-1)/2, j - (w-1)/2) is rotated (`rotate_coords_2d`) and scaled, and the
    centre of the loader's crop, bbox_lbs + (loader_patch - 1) / 2, is added.  Without rotation and scale batchgenerators takes the integer centre crop
    of the loader's crop instead: translation bbox_lbs + (loader_patch - patch) // 2, flagged as a copy.  A mirrored axis walks its grid backwards
    (every step between the two transforms is pointwise or symmetric, so the flip commutes with them)."""
    h, w = patch
    f = [-1.0 if flip[0] else 1.0, -1.0 if flip[1] else 1.0]
    if not modified:
        ty, tx = (int(bbox_lbs[d]) + (int(loader_patch[d]) - int(patch[d])) // 2 for d in range(2))
        m = [f[0], 0.0, ty + (h - 1 if flip[0] else 0), 0.0, f[1], tx + (w - 1 if flip[1] else 0)]
        return np.array(m, np.float32), 1
    cos, sin = math.cos(angle), math.sin(angle)
    a = np.array([[cos, sin], [-sin, cos]]) * zoom    # (r, c) -> (r cos + c sin, -r sin + c cos), scaled
    a = a * np.array(f)[None, :]
    centre = [bbox_lbs[d] + (loader_patch[d] - 1) / 2.0 for d in range(2)]
    g0 = np.array([(h - 1) / 2.0, (w - 1) / 2.0])
    t = np.array(centre) - a @ g0
    return np.array([a[0, 0], a[0, 1], t[0], a[1, 0], a[1, 1], t[1]], np.float32), 0


# ---- the two launches ------------------------------------------------------------------------------------------------------------------------
def _table_bytes(arr: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(arr).view(np.uint8).reshape(-1)


def upload_tables(samples: np.ndarray, chans: np.ndarray, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """Both tables through ONE pinned staging buffer and one asynchronous copy; returns device views (samples, channels).  The staging buffer comes
    from torch's pinned-memory cache, which hands it out again only after the copy has run."""
    if samples.dtype != SAMPLE_DTYPE or chans.dtype != CHAN_DTYPE:
        raise ValueError("upload_tables: tables must be of SAMPLE_DTYPE and CHAN_DTYPE")
    sb, cb = _table_bytes(samples), _table_bytes(chans)
    stage = torch.empty(sb.size + cb.size, dtype=torch.uint8, pin_memory=True)
    view = stage.numpy()
    view[:sb.size] = sb
    view[sb.size:] = cb
    dev = torch.empty(stage.numel(), dtype=torch.uint8, device=device)
    dev.copy_(stage, non_blocking=True)
    return dev[:sb.size], dev[sb.size:]


def _scale_shapes(patch, n_scales):
    h, w = int(patch[0]), int(patch[1])
    if not 1 <= n_scales <= MAX_SCALES:
        raise ValueError(f"n_scales {n_scales} out of range [1, {MAX_SCALES}]")
    div = 2 ** (n_scales - 1)
    if h % div or w % div:
        raise ValueError(f"patch {h} x {w} is not divisible by 2^(n_scales - 1) = {div} ({n_scales} deep-supervision scales)")
    return [(h >> k, w >> k) for k in range(n_scales)]


def sample_patches(store: CaseStore, samples_dev: torch.Tensor, batch_size: int, patch_size: Sequence[int], n_scales: int):
    """ldiff_op_seg_sample on the current stream: (data [B, C, h, w] float32, [n_scales label maps [B, 1, h_k, w_k] uint8])."""
    _lib.require_gpu()
    shapes = _scale_shapes(patch_size, n_scales)
    h, w = shapes[0]
    B = int(batch_size)
    if samples_dev.numel() != B * SAMPLE_DTYPE.itemsize:
        raise ValueError(f"sample_patches: the sample table holds {samples_dev.numel()} bytes, {B} samples need {B * SAMPLE_DTYPE.itemsize}")
    dev = store.arena.device
    data = torch.empty((B, store.channels, h, w), dtype=torch.float32, device=dev)
    flat = torch.empty(B * sum(a * b for a, b in shapes), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().ldiff_op_seg_sample(_lib.ptr(store.arena), store.arena.numel(), _lib.ptr(store.cases_dev), len(store), _lib.ptr(samples_dev), B,
                                                   store.channels, h, w, n_scales, _lib.ptr(data), _lib.ptr(flat), _lib.stream_ptr()))
    targets, off = [], 0
    for hk, wk in shapes:
        targets.append(flat[off:off + B * hk * wk].view(B, 1, hk, wk))
        off += B * hk * wk
    return data, targets


def augment_intensity_(data: torch.Tensor, samples_dev: torch.Tensor, chans_dev: torch.Tensor, seed: int = 0, normal: Optional[torch.Tensor] = None,
                       workspace: Optional[torch.Tensor] = None, lowres: bool = False) -> torch.Tensor:
    """ldiff_op_seg_intensity in place on `data` [B, C, h, w] float32 (contiguous), on the current stream.  `normal`: the N(0, 1) draws to use, same shape,
    instead of the Philox stream keyed by (seed, each sample's offset).  `lowres`: ldiff_op_seg_intensity_lr instead, which reads `lowres_zoom` and
    takes the larger workspace of ldiff_op_seg_intensity_lr_ws_bytes."""
    _lib.require_gpu()
    if data.dim() != 4 or data.dtype != torch.float32 or not data.is_contiguous() or not data.is_cuda:
        raise ValueError("augment_intensity_: data must be a contiguous float32 [B, C, h, w] device tensor")
    B, Cc, h, w = (int(v) for v in data.shape)
    if samples_dev.numel() != B * SAMPLE_DTYPE.itemsize or chans_dev.numel() != B * Cc * CHAN_DTYPE.itemsize:
        raise ValueError("augment_intensity_: table sizes do not match the batch")
    if normal is not None and (normal.shape != data.shape or normal.dtype != torch.float32 or not normal.is_contiguous() or normal.device != data.device):
        raise ValueError("augment_intensity_: normal must match data")
    lib = _lib.load()
    ws_bytes, op = (lib.ldiff_op_seg_intensity_lr_ws_bytes, lib.ldiff_op_seg_intensity_lr) if lowres else (lib.ldiff_op_seg_intensity_ws_bytes, lib.ldiff_op_seg_intensity)
    need = int(ws_bytes(B, Cc, h, w))
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=data.device)
    with torch.cuda.device(data.device):
        _lib.check(op(_lib.ptr(data), _lib.ptr(samples_dev), _lib.ptr(chans_dev), B, Cc, h, w, _lib.ptr(normal), int(seed) & (2 ** 64 - 1),
                      _lib.ptr(workspace), workspace.numel() * workspace.element_size(), _lib.stream_ptr()))
    return data


def spline_prefilter_(planes: torch.Tensor) -> torch.Tensor:
    """ldiff_op_spline_prefilter in place on `planes` [..., H, W] float32 on the device, on the current stream: scipy.ndimage.spline_filter(order=3,
    mode='mirror') of every [H, W] plane, what `spline_coefficients` is in float64.  The last axis must be dense and the planes evenly spaced, a row
    stride apart per row (a contiguous tensor, or one sliced along W)."""
    _lib.require_gpu()
    if planes.dim() < 2 or planes.dtype != torch.float32 or not planes.is_cuda:
        raise ValueError("spline_prefilter_: planes must be a float32 [..., H, W] device tensor")
    H, W = int(planes.shape[-2]), int(planes.shape[-1])
    stride = int(planes.stride(-2)) if H > 1 else W
    n_planes = int(planes.numel() // max(H * W, 1))
    dense = planes.stride(-1) == 1 or W == 1
    step, size = H * stride, 1
    for d in range(planes.dim() - 3, -1, -1):   # the leading axes must walk the planes in steps of H * stride
        dense = dense and (planes.shape[d] == 1 or planes.stride(d) == step * size)
        size *= int(planes.shape[d])
    if not dense or planes.numel() == 0:
        raise ValueError(f"spline_prefilter_: planes of shape {tuple(planes.shape)} and strides {tuple(planes.stride())} are not evenly spaced rows and planes")
    with torch.cuda.device(planes.device):
        _lib.check(_lib.load().ldiff_op_spline_prefilter(_lib.ptr(planes), n_planes, H, W, stride, _lib.stream_ptr()))
    return planes


# ---- plan and preprocess of one case (kernels_segprep.hip) ---------------------------------------------------------------------------------------
def _case_image(img: torch.Tensor, who: str):
    """(dtype code, C, H, W, row stride, plane stride) of a [C, H, W] uint8 / float32 device tensor whose last axis is dense (a view sliced along H or W
    of a wider tensor is fine)."""
    if img.dim() != 3 or img.dtype not in (torch.uint8, torch.float32) or not img.is_cuda:
        raise ValueError(f"{who}: the image must be a [C, H, W] uint8 or float32 device tensor, got {tuple(img.shape)} of {img.dtype} on {img.device}")
    Cc, H, W = (int(v) for v in img.shape)
    if Cc < 1 or H < 1 or W < 1 or (W > 1 and img.stride(2) != 1):
        raise ValueError(f"{who}: image of shape {tuple(img.shape)} and strides {tuple(img.stride())}: empty, or the last axis is not dense")
    return 0 if img.dtype == torch.uint8 else 1, Cc, H, W, max(int(img.stride(1)), W) if H > 1 else W, int(img.stride(0)) if Cc > 1 else H * max(int(img.stride(1)), W)


def _case_labels(seg: torch.Tensor, who: str, like: Optional[torch.Tensor] = None):
    if seg.dim() != 2 or seg.dtype != torch.uint8 or not seg.is_cuda or (seg.shape[1] > 1 and seg.stride(1) != 1) or seg.numel() == 0:
        raise ValueError(f"{who}: the label map must be a [H, W] uint8 device tensor with a dense last axis, got {tuple(seg.shape)} of {seg.dtype} on {seg.device}")
    if like is not None and (tuple(seg.shape) != tuple(like.shape[1:]) or seg.device != like.device):
        raise ValueError(f"{who}: labels {tuple(seg.shape)} on {seg.device} do not fit the image {tuple(like.shape)} on {like.device}")
    H, W = int(seg.shape[0]), int(seg.shape[1])
    return H, W, max(int(seg.stride(0)), W) if H > 1 else W


def _check_box(box, H: int, W: int, who: str):
    y0, y1, x0, x1 = (int(v) for v in box)
    if not (0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W):
        raise ValueError(f"{who}: box {(y0, y1, x0, x1)} is empty or leaves the {H} x {W} case")
    return y0, y1, x0, x1


def _launch_case_bbox(img: torch.Tensor, out: torch.Tensor) -> None:
    dt, Cc, H, W, rs, ps = _case_image(img, "case_bbox")
    with torch.cuda.device(img.device):
        _lib.check(_lib.load().ldiff_op_case_bbox(_lib.ptr(img), dt, Cc, H, W, rs, ps, _lib.ptr(out), _lib.stream_ptr()))


def case_bbox(img: torch.Tensor) -> Tuple[int, int, int, int]:
    """ldiff_op_case_bbox: `nnunet.nonzero_bbox(img)` -- (y0, y1, x0, x1), ends exclusive, of the pixels where any channel is non-zero; the full extent
    for an all-zero image -- for a [C, H, W] uint8 / float32 image on the device.  Synchronises (the box comes back to the host)."""
    _lib.require_gpu()
    out = torch.empty(4, dtype=torch.int32, device=img.device)
    _launch_case_bbox(img, out)
    return tuple(int(v) for v in out.cpu())


def _launch_case_stats(img: torch.Tensor, box, out: torch.Tensor, ws: torch.Tensor) -> None:
    dt, Cc, H, W, rs, ps = _case_image(img, "case_stats")
    y0, y1, x0, x1 = _check_box(box, H, W, "case_stats")
    with torch.cuda.device(img.device):
        _lib.check(_lib.load().ldiff_op_case_stats(_lib.ptr(img), dt, Cc, H, W, rs, ps, y0, y1, x0, x1, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))


def case_stats(img: torch.Tensor, box) -> np.ndarray:
    """ldiff_op_case_stats: per channel over the box, a numpy record array with `sum`, `sumsq` (python-exact uint64 for a uint8 image, float64 sums in a
    fixed order for a float32 image), `min`, `max` (float64).  Synchronises."""
    _lib.require_gpu()
    out = torch.empty((int(img.shape[0]), 4), dtype=torch.int64, device=img.device)
    ws = torch.empty(max(int(_lib.load().ldiff_op_case_stats_ws_bytes(int(img.shape[0]))), 16), dtype=torch.uint8, device=img.device)
    _launch_case_stats(img, box, out, ws)
    return stats_records(out.cpu().numpy(), img.dtype)


def stats_records(raw: np.ndarray, dtype) -> np.ndarray:
    """The [C, 4] int64 words ldiff_op_case_stats writes, viewed as records: the sums are uint64 for a uint8 image and float64 for a float32 one."""
    kind = "<u8" if dtype == torch.uint8 else "<f8"
    return np.ascontiguousarray(raw).view(np.dtype([("sum", kind), ("sumsq", kind), ("min", "<f8"), ("max", "<f8")])).reshape(-1)


def normalization_scalars(raw_stats: np.ndarray, dtype, n_pixels: int, schemes: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    """(sub [C], div [C]) float32 with which ldiff_op_case_apply states `nnunet.normalize`: out = (x - sub) / div.  Mean and population standard deviation
    are formed here in float64 (exactly, in integers, for a uint8 image) from the kernel's sums and rounded once to float32."""
    rec = stats_records(raw_stats, dtype)
    sub, div = np.zeros(len(schemes), np.float32), np.ones(len(schemes), np.float32)
    for c, scheme in enumerate(schemes):
        mn, mx = float(rec["min"][c]), float(rec["max"][c])
        if scheme == "ZScoreNormalization":
            if dtype == torch.uint8:
                s1, s2, n = int(rec["sum"][c]), int(rec["sumsq"][c]), int(n_pixels)
                mean, var = s1 / n, (n * s2 - s1 * s1) / (n * n)
            else:
                mean = float(rec["sum"][c]) / n_pixels
                var = max(float(rec["sumsq"][c]) / n_pixels - mean * mean, 0.0)
            sub[c], div[c] = mean, max(float(np.float32(math.sqrt(var))), 1e-8)
        elif scheme == "RGBTo01Normalization":
            if mn < 0 or mx > 255:
                raise ValueError("RGBTo01Normalization: pixel values outside 0..255")
            div[c] = 255.0
        elif scheme == "RescaleTo01Normalization":
            sub[c] = mn
            div[c] = max(float(np.float32(mx) - np.float32(mn)), 1e-8)   # the float32 difference, as nnunet.normalize forms it
        elif scheme != "NoNormalization":
            nnunet._refuse("normalization_schemes", f"names {scheme!r}")
    return sub, div


def _launch_case_counts(seg: torch.Tensor, box, n_heads: int, totals: torch.Tensor, n_classes: Optional[int] = None):
    """`n_classes`: ldiff_op_case_counts_classes -- one more prefix row and one more total, for `label < n_classes`; n_heads may then be 33."""
    H, W, ls = _case_labels(seg, "case_counts")
    y0, y1, x0, x1 = _check_box(box, H, W, "case_counts")
    top = 32 if n_classes is None else 33
    if not 1 <= int(n_heads) <= top:
        raise ValueError(f"case_counts: n_heads {n_heads} out of range [1, {top}]")
    if n_classes is not None and not 1 <= int(n_classes) <= int(n_heads):
        raise ValueError(f"case_counts: n_classes {n_classes} out of range [1, {n_heads}]")
    rows = y1 - y0
    row_counts = torch.empty((rows, n_heads + 1), dtype=torch.int32, device=seg.device)
    prefix = torch.empty((n_heads + (1 if n_classes is None else 2), rows + 1), dtype=torch.int32, device=seg.device)
    if totals.numel() != n_heads + (2 if n_classes is None else 3):
        raise ValueError(f"case_counts: totals must hold {n_heads + (2 if n_classes is None else 3)} counts, got {totals.numel()}")
    with torch.cuda.device(seg.device):
        if n_classes is not None:
            _lib.check(_lib.load().ldiff_op_case_counts_classes(_lib.ptr(seg), H, W, ls, y0, y1, x0, x1, int(n_heads), int(n_classes), _lib.ptr(row_counts),
                                                                _lib.ptr(prefix), _lib.ptr(totals), _lib.stream_ptr()))
            return row_counts, prefix
        _lib.check(_lib.load().ldiff_op_case_counts(_lib.ptr(seg), H, W, ls, y0, y1, x0, x1, int(n_heads), _lib.ptr(row_counts), _lib.ptr(prefix), _lib.ptr(totals),
                                                    _lib.stream_ptr()))
    return row_counts, prefix


def case_counts(seg: torch.Tensor, box, n_heads: int):
    """ldiff_op_case_counts on a [H, W] uint8 label map on the device: (row_counts [rows, n_heads + 1] -- per row of the box the pixels of each class,
    then those with a label >= n_heads; row_prefix [n_heads + 1, rows + 1] -- per class, and for `label > 0` at index n_heads, the exclusive prefix of
    the selected pixels over the rows, the last entry the total; totals, a host array [n_heads + 2]: per class, `label > 0`, labels >= n_heads).  The first
    two stay on the device (int32 holding the kernel's uint32 counts: a case has fewer than 2^31 pixels).  Synchronises."""
    _lib.require_gpu()
    totals = torch.empty(int(n_heads) + 2, dtype=torch.int32, device=seg.device)
    row_counts, prefix = _launch_case_counts(seg, box, n_heads, totals)
    return row_counts, prefix, totals.cpu().numpy().astype(np.int64)


def _launch_case_apply(img: torch.Tensor, seg: torch.Tensor, box, sub: np.ndarray, div: np.ndarray, arena: torch.Tensor, row: np.ndarray, write_coef: bool) -> None:
    dt, Cc, H, W, rs, ps = _case_image(img, "case_apply")
    _, _, ls = _case_labels(seg, "case_apply", img)
    y0, y1, x0, x1 = _check_box(box, H, W, "case_apply")
    sub, div = np.ascontiguousarray(sub, np.float32), np.ascontiguousarray(div, np.float32)
    if sub.shape != (Cc,) or div.shape != (Cc,) or arena.dtype != torch.uint8 or not arena.is_contiguous() or arena.device != img.device:
        raise ValueError("case_apply: sub / div must hold one float per channel and the arena be a contiguous uint8 tensor on the image's device")
    FP = _lib.C.POINTER(_lib.C.c_float)
    c_row = _lib.SegCase(*(int(row[k]) for k in ("coef_off", "raw_off", "label_off", "H", "W", "stride", "label_stride")))
    with torch.cuda.device(img.device):
        _lib.check(_lib.load().ldiff_op_case_apply(_lib.ptr(img), dt, Cc, H, W, rs, ps, _lib.ptr(seg), ls, y0, y1, x0, x1, sub.ctypes.data_as(FP), div.ctypes.data_as(FP),
                                                   _lib.ptr(arena), arena.numel(), _lib.C.byref(c_row), int(bool(write_coef)), _lib.stream_ptr()))


def _launch_case_rank(seg: torch.Tensor, box, selector: int, prefix_row: torch.Tensor, ranks: torch.Tensor, image: Optional[torch.Tensor]):
    H, W, ls = _case_labels(seg, "case_rank_to_coord", image)
    y0, y1, x0, x1 = _check_box(box, H, W, "case_rank_to_coord")
    if ranks.dim() != 1 or ranks.dtype != torch.int64 or not ranks.is_contiguous() or ranks.device != seg.device:
        raise ValueError("case_rank_to_coord: ranks must be a contiguous int64 vector on the labels' device")
    if prefix_row.dtype != torch.int32 or tuple(prefix_row.shape) != (y1 - y0 + 1,) or not prefix_row.is_contiguous() or prefix_row.device != seg.device:
        raise ValueError(f"case_rank_to_coord: row_prefix must be the selector's contiguous int32 [{y1 - y0 + 1}] of case_counts")
    n = int(ranks.numel())
    coords = torch.empty((n, 2), dtype=torch.int32, device=seg.device)
    values, dt, Cc, rs, ps = None, 0, 0, 0, 0
    if image is not None:
        dt, Cc, _, _, rs, ps = _case_image(image, "case_rank_to_coord")
        values = torch.empty((n, Cc), dtype=image.dtype, device=seg.device)
    with torch.cuda.device(seg.device):
        _lib.check(_lib.load().ldiff_op_case_rank_to_coord(_lib.ptr(seg), H, W, ls, y0, y1, x0, x1, int(selector), _lib.ptr(prefix_row), _lib.ptr(ranks), n,
                                                           _lib.ptr(coords), _lib.ptr(image), dt, Cc, rs, ps, _lib.ptr(values), _lib.stream_ptr()))
    return coords, values


def case_rank_to_coord(seg: torch.Tensor, box, selector: int, prefix_row: torch.Tensor, ranks: torch.Tensor, image: Optional[torch.Tensor] = None):
    """ldiff_op_case_rank_to_coord: (coords int32 [n, 2], values [n, C] or None), on the device.  coords[k] = np.argwhere(selection)[ranks[k]] inside the
    box, where the selection is `label == selector`, or `label > 0` for selector -1; `prefix_row` = `case_counts(...)[1][selector]` (index n_heads for
    -1); values[k] = image[:, pixel].  Every rank must lie in [0, count): checked here against the prefix' last entry, which synchronises."""
    _lib.require_gpu()
    if ranks.numel():
        lo, hi, count = int(ranks.min()), int(ranks.max()), int(prefix_row[-1])
        if lo < 0 or hi >= count:
            raise ValueError(f"case_rank_to_coord: ranks span [{lo}, {hi}], the selection has {count} pixels")
    return _launch_case_rank(seg, box, selector, prefix_row, ranks, image)


class PatchLoader:
    """nnUNetDataLoader2D + the training transforms as an endless iterator of batches on the store's device:
    {"data": [B, C, h, w] float32, "target": [n_scales tensors [B, 1, h >> k, w >> k] uint8]}, highest resolution first -- what
    `Trainer.train_step`, `validation_step` and `run_training` take.  `train=False` is the validation loader: exact crops, no augmentation.
    The same seed yields the same batches.  `lowres=True` draws and applies the low-resolution simulation too: nnU-Net's whole chain."""

    def __init__(self, store: CaseStore, patch_size: Sequence[int], batch_size: int, n_scales: int, seed: int, train: bool = True,
                 oversample: float = OVERSAMPLE_FOREGROUND, lowres: bool = False):
        if store.arena.device.type != "cuda":
            raise ValueError("PatchLoader: the store must live on a GPU")
        self.shapes = _scale_shapes(patch_size, n_scales)
        self.store, self.patch_size, self.batch_size, self.n_scales = store, (int(patch_size[0]), int(patch_size[1])), int(batch_size), int(n_scales)
        self.train, self.oversample, self.seed, self.lowres = bool(train), float(oversample), int(seed), bool(lowres)
        self.rng = np.random.default_rng(self.seed)
        lib = _lib.load()
        ws_bytes = lib.ldiff_op_seg_intensity_lr_ws_bytes if self.lowres else lib.ldiff_op_seg_intensity_ws_bytes
        need = int(ws_bytes(self.batch_size, store.channels, *self.patch_size))
        self._ws = torch.empty(max(need, 16), dtype=torch.uint8, device=store.arena.device) if self.train else None

    def __iter__(self):
        return self

    def __next__(self) -> dict:
        samples, chans = draw_batch(self.rng, self.store, self.batch_size, self.patch_size, self.train, self.oversample, self.lowres)
        with torch.cuda.device(self.store.arena.device):
            s_dev, c_dev = upload_tables(samples, chans, self.store.arena.device)
            data, targets = sample_patches(self.store, s_dev, self.batch_size, self.patch_size, self.n_scales)
            if self.train:
                augment_intensity_(data, s_dev, c_dev, self.seed, workspace=self._ws, lowres=self.lowres)
        return {"data": data, "target": targets}
