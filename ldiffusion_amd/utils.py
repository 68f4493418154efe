"""Mirrors of the reference's utils.py.  The mask metrics `micro_dice` (:55-82) and `mean_iou_and_per_class` (:84-104): same names, arguments and
return shapes, computed from one confusion matrix counted on the device (ldiffusion_amd/metrics.py) instead of 2-3 masked sums and `.item()`s per class.
The sampler call site (nnU-Net dataset creation): `copy_or_convert_image`, sampler variant V4
(/root/reference/utils.py:176-208), and `copy_or_convert_images`, the same pass batched over a dataset's images behind the device image front end (imgio.py).  Same name, arguments and effect -- a PNG of the one-pass diffusion of the image at `dst_path`, or a plain
copy -- with the arithmetic on the HIP kernels (no CPU fallback: the pipeline shims raise without the library or a GPU)."""
from __future__ import annotations

import shutil

import numpy as np
import torch
from torch import nn

from . import metrics
from .pipeline import LaplaceSampler

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
_samplers: dict = {}


def _sampler(pipeline, unet):
    key = (id(pipeline), id(unet))
    s = _samplers.get(key)
    if s is None or s.pipeline is not pipeline or pipeline.unet is not unet:
        pipeline.unet = unet
        s = _samplers[key] = LaplaceSampler(pipeline)
    return s


def _image_text_embeddings(pipeline, unet, device):
    """The text embeddings `copy_or_convert_image` makes for ONE image (utils.py:193-197), and the UNet the sampler runs: (emb [1, L, D], base)."""
    linear_layer = nn.Linear(768, 1280).to(device)                                               # :193 (randomly initialised on every call, as there)
    ids = torch.tensor(pipeline.tokenizer(["A pathological slide"] * 1)["input_ids"], dtype=torch.long, device=device)
    emb = pipeline.text_encoder(ids)["last_hidden_state"].to(device=device, dtype=torch.float32)
    emb = linear_layer(emb).clone().detach()
    base = getattr(unet, "base_unet", unet)
    if hasattr(unet, "base_unet"):                                                               # the wrapper's rule (segmentor.py:190-202), applied here
        if emb.shape[-1] != unet.cross_attention_dim:                                            # because the fused sampler takes the context up front
            emb = unet.default_text_embeddings
    elif emb.shape[-1] != base.config.cross_attention_dim:
        raise ValueError(f"copy_or_convert_image: text embeddings of width {emb.shape[-1]} for a UNet with cross_attention_dim "
                         f"{base.config.cross_attention_dim} (the reference passes the text-alignment wrapper here)")
    return emb, base


@torch.no_grad()
def copy_or_convert_image(img, src_path, dst_path, pipeline=None, unet=None, use_diffusion=True):
    """utils.py:176-208.  use_diffusion: Resize((1024, 1024)) + ToTensor + ImageNet Normalize (:180-185) -> vae.encode().mean ->
    set_timesteps(1) -> text embeddings of "A pathological slide" through a FRESH nn.Linear(768, 1280) (:193-197; at the reference's call
    site `unet` is the text-alignment wrapper, segmentor.py:183-205 = ldiffusion_amd.segmentor.TextAlignedUNet, which ignores embeddings
    whose width is not the UNet's and uses its cached ones: that is what happens here for SD-v1.5) -> one UNet pass -> scheduler.step ->
    decode_latents -> numpy_to_pil -> save as PNG (:199-206).  Otherwise a plain copy (:207-208)."""
    if not use_diffusion:
        shutil.copy(src_path, dst_path)
        return
    from PIL import Image
    device = pipeline.vae.device if hasattr(pipeline.vae, "device") else torch.device("cuda", torch.cuda.current_device())
    x = torch.from_numpy(np.asarray(img.convert("RGB").resize((1024, 1024), Image.BILINEAR), np.float32) / 255.0).permute(2, 0, 1)[None].to(device)
    mean = torch.tensor(IMAGENET_MEAN, device=device).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device=device).view(1, 3, 1, 1)
    emb, base = _image_text_embeddings(pipeline, unet, device)
    sampler = _sampler(pipeline, base)
    out = sampler.sample((x - mean) / std, emb.to(device=device, dtype=torch.float32)[:1], 1, want_features=False, want_rgb=True)
    rgb = out["rgb"][0].cpu().numpy()
    sampler.check_finite()   # fp16 overflow in either graph raises instead of writing a garbage PNG
    Image.fromarray(rgb).save(dst_path)


MAX_IO_WORKERS = 16


def _decode_rgb(item):
    """A worker's decode: a path or a PIL image -> uint8 [H, W, 3] (PIL only: no torch, no library call)."""
    from PIL import Image
    if isinstance(item, Image.Image):
        return np.asarray(item.convert("RGB"), np.uint8)
    with Image.open(item) as img:
        return np.asarray(img.convert("RGB"), np.uint8)


def _save_rgb(rgb, dst_path):
    from PIL import Image
    Image.fromarray(rgb).save(dst_path)


def _image_size(item):
    from PIL import Image
    if isinstance(item, Image.Image):
        return item.size
    with Image.open(item) as img:   # the header alone: nothing is decoded
        return img.size


class _Inline:
    """What a pool's future is to its caller, for io_workers=0: the call has been made already."""

    def __init__(self, value):
        self.value = value

    def result(self):
        return self.value


@torch.no_grad()
def copy_or_convert_images(imgs, dst_paths, pipeline, unet, *, batch_images, size=(1024, 1024), io_workers=4):
    """`copy_or_convert_image(use_diffusion=True)` over many images, batched: `imgs` (PIL images or paths) -> one PNG each at `dst_paths`.
    Per batch -- up to `batch_images` consecutive images of one source size --: the RGB uint8 arrays stacked, ONE copy to the device,
    `imgio.resize_normalize` (Pillow's bilinear resize to `size` = (width, height), ToTensor and the ImageNet Normalize on the device, bit for bit
    the per-image expression), the text embeddings by `copy_or_convert_image`'s rule per image in image order (a fresh nn.Linear(768, 1280) each: the
    draws from torch's generator keep today's order; a [B, L, D] context when they differ per image, one row when the wrapper's cached ones replace
    them), ONE sampler call, one copy back, `check_finite()` before any file of the batch is written, then `Image.fromarray(rgb).save(dst)` per image.
    For the duration of the call the pipeline runs under `set_plan_batch(batch_images)`; the UNet's and the VAE's previous `.plan_batch` come back in a
    `finally`.  The contract: the PNG of an image depends neither on its position, nor on its neighbours, nor on a short last batch; it is byte for
    byte the file `copy_or_convert_image` writes for that image ALONE under `pipeline.set_plan_batch(batch_images)`.  It is NOT the file of the
    default-plan per-image path (plan batch 0): that one differs by the usual fp16 plan difference (README, "batch-invariant sampling").
    `io_workers` threads (default 4, at most 16) do nothing but PIL work beside the device -- they decode the next batch and encode + save the
    previous one; only the calling thread touches torch or the library; at most two batches of host buffers are alive at a time.  A worker's
    exception is re-raised here after the pool has drained: no thread is left running.  io_workers=0 does everything inline and writes the same bytes.
    The sampler's own limits hold: at 1024^2 the VAE's 3x3 conv takes at most five images per call (the library's ValueError names it; DESIGN.md "Dataset pass")."""
    from concurrent.futures import ThreadPoolExecutor
    from . import imgio
    imgs, dst_paths = list(imgs), list(dst_paths)
    if len(imgs) != len(dst_paths):
        raise ValueError(f"dst_paths: {len(dst_paths)} paths for {len(imgs)} images")
    if isinstance(batch_images, bool) or not isinstance(batch_images, (int, np.integer)) or batch_images < 1:
        raise ValueError(f"batch_images = {batch_images!r}: an integer >= 1")
    if isinstance(io_workers, bool) or not isinstance(io_workers, (int, np.integer)) or not 0 <= io_workers <= MAX_IO_WORKERS:
        raise ValueError(f"io_workers = {io_workers!r}: an integer in 0 .. {MAX_IO_WORKERS}")
    batch_images = int(batch_images)
    if not imgs:
        return
    sizes = [_image_size(im) for im in imgs]
    batches, start = [], 0
    for i in range(1, len(imgs) + 1):   # consecutive runs of one source size, cut at batch_images
        if i == len(imgs) or sizes[i] != sizes[start] or i - start == batch_images:
            batches.append(range(start, i))
            start = i
    device = pipeline.vae.device if hasattr(pipeline.vae, "device") else torch.device("cuda", torch.cuda.current_device())
    base = getattr(unet, "base_unet", unet)
    sampler = _sampler(pipeline, base)
    previous = (base.plan_batch, pipeline.vae.plan_batch)
    pool = ThreadPoolExecutor(max_workers=int(io_workers), thread_name_prefix="ldiff-imgio") if io_workers else None

    def run(fn, *args):   # a worker's task, or the same call inline
        if pool is not None:
            return pool.submit(fn, *args)
        return _Inline(fn(*args))

    try:
        pipeline.set_plan_batch(batch_images)
        decoding = [run(_decode_rgb, imgs[i]) for i in batches[0]]
        saving = []
        for k, batch in enumerate(batches):
            host = np.stack([f.result() for f in decoding])
            x = imgio.resize_normalize(torch.from_numpy(host).to(device), size, IMAGENET_MEAN, IMAGENET_STD)
            del host
            decoding = [run(_decode_rgb, imgs[i]) for i in batches[k + 1]] if k + 1 < len(batches) else []
            embs = [_image_text_embeddings(pipeline, unet, device)[0] for _ in batch]
            if hasattr(unet, "base_unet") and all(e is unet.default_text_embeddings for e in embs):
                ctx = embs[0].to(device=device, dtype=torch.float32)[:1]
            else:
                ctx = torch.cat([e.to(device=device, dtype=torch.float32)[:1] for e in embs], 0)
            out = sampler.sample(x, ctx, 1, want_features=False, want_rgb=True)
            for f in saving:   # the previous batch's files, encoded while this one was enqueued; its buffers go before this batch's arrive
                f.result()
            rgb = out["rgb"].cpu().numpy()
            sampler.check_finite()   # before any file of the batch is written
            saving = [run(_save_rgb, rgb[j], dst_paths[i]) for j, i in enumerate(batch)]
            del rgb
        for f in saving:
            f.result()
    finally:
        if pool is not None:
            pool.shutdown(wait=True, cancel_futures=True)
        base.set_plan_batch(previous[0])
        pipeline.vae.set_plan_batch(previous[1])
        if getattr(base, "_controlnet", None) is not None:
            base._controlnet.set_plan_batch(previous[0])


_warned = False   # utils.py:15: the size warning is printed once


def check_images_same_size(image_paths):
    """utils.py:155-163: True when every image has the same (width, height)."""
    from PIL import Image
    sizes = set()
    for path in image_paths:
        with Image.open(path) as img:
            sizes.add(img.size)
        if len(sizes) > 1:
            return False
    return True


def fix_label_size(img, lbl, img_name, lbl_name):
    """utils.py:17-24: a label image whose size differs from its image's is resized to it with NEAREST (warned about once)."""
    global _warned
    from PIL import Image
    if img.size != lbl.size:
        if not _warned:
            print("\033[91m[WARNING] Some image/label sizes are inconsistent. Labels will be resized to match images.\033[0m")
            _warned = True
        lbl = lbl.resize(img.size, Image.NEAREST)
    return lbl


def convert_and_save_label(lbl, dst_path, mapping):
    """utils.py:165-174: grey levels -> class indices by `mapping` (levels it does not name become 0), saved as an 8-bit PNG."""
    from PIL import Image
    lut = np.zeros(256, np.uint8)
    for level, index in mapping.items():
        lut[int(level)] = index
    Image.fromarray(lut[np.asarray(lbl.convert("L"), np.uint8)]).save(dst_path)


def create_nnunet_dataset(train_images, train_labels, test_images, test_labels, num_classes, pipeline, unet, raw_dir=None, batch_images=None, io_workers=4,
                          ignore_pixel=None, regions=None, regions_class_order=None):
    """utils.py:210-294: the next `DatasetNNN_Custom` under nnUNet_raw (`raw_dir`, else the environment variable nnUNet_raw) with imagesTr / labelsTr /
    imagesTs / labelsTs, `case_%03d_0000.png` + `case_%03d.png` and `caseTs_%03d...`; every image goes through `copy_or_convert_image` -- the
    one-pass diffusion when ALL train and ALL test images share one size, else a plain copy --, every label is resized to its image (NEAREST) and
    mapped through metrics.PIXEL_TO_LABEL; `dataset.json` as the reference writes it.  Returns (new_num, new_dataset_name).
    `batch_images` (None: the per-image path above, byte for byte): with the diffusion on, the images of each list go through
    `copy_or_convert_images(batch_images=..., io_workers=...)` after the list's labels are written -- the files are those of `copy_or_convert_image`
    alone under `pipeline.set_plan_batch(batch_images)`, the labels and dataset.json those of the default call.  With mixed sizes (plain copies) it changes nothing.
    `ignore_pixel` (None: everything above, byte for byte): the grey level of unlabelled pixels in partly annotated label images.  The label PNGs
    carry `num_classes` there and dataset.json gains `"ignore": num_classes` -- nnU-Net's ignore label, the highest value.  A grey level
    metrics.PIXEL_TO_LABEL already maps raises ValueError.
    `regions` (None: everything above, byte for byte): region labels -- a mapping from a region's name to the list of classes it unites, as class
    indices, or as the label images' grey levels (keys of metrics.PIXEL_TO_LABEL) when any value is not a class index; `regions_class_order`: the value
    inference writes per region, in order (nnU-Net's field).  The label PNGs keep class indices; dataset.json carries the region `labels` and
    `regions_class_order`.  Every foreground class must lie in a region (nnU-Net has no head for a label outside all of them); `nnunet.region_spec`
    checks the rest before anything is written."""
    import json
    import os
    from pathlib import Path
    from PIL import Image
    mapping = metrics.PIXEL_TO_LABEL
    if ignore_pixel is not None:
        if isinstance(ignore_pixel, bool) or int(ignore_pixel) != ignore_pixel or not 0 <= int(ignore_pixel) <= 255:
            raise ValueError(f"create_nnunet_dataset: ignore_pixel {ignore_pixel!r} is not a grey level 0 .. 255")
        if int(ignore_pixel) in {int(level) for level in mapping}:
            raise ValueError(f"create_nnunet_dataset: ignore_pixel {int(ignore_pixel)} is the grey level of class {mapping[int(ignore_pixel)]}")
        if not 2 <= int(num_classes) <= 254:
            raise ValueError(f"create_nnunet_dataset: an ignore label needs 2 .. 254 classes, got {num_classes}")
        mapping = {**mapping, int(ignore_pixel): int(num_classes)}
    region_labels = None
    if regions is not None:
        from . import nnunet
        values = [v for r in regions.values() for v in r]
        if any(isinstance(v, bool) or int(v) != v for v in values) or not values:
            raise ValueError("create_nnunet_dataset: `regions` maps names to non-empty lists of integers")
        as_levels = any(not 0 <= int(v) < int(num_classes) for v in values)   # grey levels of the label images, not class indices
        if as_levels and any(int(v) not in metrics.PIXEL_TO_LABEL for v in values):
            raise ValueError(f"create_nnunet_dataset: `regions` holds {sorted({int(v) for v in values if int(v) not in metrics.PIXEL_TO_LABEL})}: neither class "
                             f"indices below {num_classes} nor grey levels of metrics.PIXEL_TO_LABEL")
        region_labels = {"background": 0, **{str(name): [int(metrics.PIXEL_TO_LABEL[int(v)]) if as_levels else int(v) for v in r] for name, r in regions.items()}}
        if "background" in regions or "ignore" in regions:
            raise ValueError("create_nnunet_dataset: `regions` may not name a region `background` or `ignore`")
        outside = sorted(set(range(1, int(num_classes))) - {v for r in region_labels.values() if isinstance(r, list) for v in r})
        if outside:
            raise ValueError(f"create_nnunet_dataset: the classes {outside} lie in no region of `regions`")
        if ignore_pixel is not None:
            region_labels["ignore"] = int(num_classes)
        nnunet.region_spec(region_labels, regions_class_order)   # refuses, naming the field, before anything is written
    elif regions_class_order is not None:
        raise ValueError("create_nnunet_dataset: `regions_class_order` without `regions`")
    raw = raw_dir if raw_dir is not None else os.environ.get("nnUNet_raw")
    if raw is None:
        raise RuntimeError("create_nnunet_dataset: no nnUNet_raw folder: pass raw_dir= or set the environment variable nnUNet_raw")
    raw_path = Path(raw)
    if not raw_path.exists():
        raise FileNotFoundError(f"create_nnunet_dataset: nnUNet_raw = {raw} does not exist")
    use_diffusion = check_images_same_size(train_images) and check_images_same_size(test_images)
    max_num = 0
    for d in raw_path.iterdir():
        if d.is_dir() and d.name.startswith("Dataset"):
            try:
                max_num = max(max_num, int(d.name[7:10]))
            except ValueError:
                continue
    batched = use_diffusion and batch_images is not None
    new_num = max_num + 1
    new_dataset_name = f"Dataset{new_num:03d}_Custom"
    new_path = raw_path / new_dataset_name
    new_path.mkdir(parents=True, exist_ok=False)
    for sub in ("imagesTr", "labelsTr", "imagesTs", "labelsTs"):
        (new_path / sub).mkdir()
    n_train = 0
    for images, labels, stem, img_dir, lbl_dir in ((train_images, train_labels, "case", "imagesTr", "labelsTr"), (test_images, test_labels, "caseTs", "imagesTs", "labelsTs")):
        pending = []
        for idx, (img_path, lbl_path) in enumerate(zip(images, labels)):
            case_id = f"{stem}_{idx:03d}"
            img_path = Path(img_path)
            img = Image.open(img_path) if batched else Image.open(img_path).convert("RGB")   # batched: the size alone is needed here, a worker decodes
            lbl = fix_label_size(img, Image.open(lbl_path).convert("L"), img_path.name, lbl_path)
            if batched:
                pending.append((img_path, new_path / img_dir / f"{case_id}_0000.png"))
            else:
                copy_or_convert_image(img, img_path, new_path / img_dir / f"{case_id}_0000.png", pipeline, unet, use_diffusion)
            convert_and_save_label(lbl, new_path / lbl_dir / f"{case_id}.png", mapping)
            n_train += stem == "case"
            if batched:
                img.close()
        if pending:
            copy_or_convert_images([p for p, _ in pending], [d for _, d in pending], pipeline, unet, batch_images=batch_images, io_workers=io_workers)
    dataset_json = {
        "channel_names": {"0": "R", "1": "G", "2": "B"},
        "labels": {"background": 0, **{f"class{i}": i for i in range(1, num_classes)}, **({} if ignore_pixel is None else {"ignore": int(num_classes)})},
        "numTraining": n_train,
        "file_ending": ".png",
    }
    if region_labels is not None:
        dataset_json["labels"] = region_labels
        dataset_json["regions_class_order"] = [int(c) for c in regions_class_order]
    with open(new_path / "dataset.json", "w") as f:
        json.dump(dataset_json, f, indent=4)
    print(f"create new nnUNet Dataset：{new_dataset_name}")
    return new_num, new_dataset_name


def micro_dice(predicted_labels, true_labels, num_classes=7):
    """utils.py:55-82 (= Segmentor.micro_dice, segmentor.py:114-142): logits [B, C, H, W] and labels [B, H, W] -> (per-class float32 tensor, its mean);
    the whole batch is flattened together and a class absent from both prediction and labels scores 1.  One launch and one copy of C^2 integers per
    image; the figures come back as host tensors (they are for reporting: `.item()`, `.cpu().numpy()` and arithmetic on them work as on the reference's)."""
    m = metrics.score(predicted_labels, true_labels, num_classes)
    return torch.from_numpy(m.dice_per_class.copy()), torch.tensor(m.dice, dtype=torch.float32)


def mean_iou_and_per_class(pred, target, num_classes):
    """utils.py:84-104: (mean IoU as a float, {class: IoU or None}); a class with an empty union is None and left out of the mean, which is 1.0
    when no class is left."""
    m = metrics.score(pred, target, num_classes)
    return m.miou, m.iou_per_class
