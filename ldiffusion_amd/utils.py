"""Mirrors of the reference's utils.py.  The mask metrics `micro_dice` (:55-82) and `mean_iou_and_per_class` (:84-104): same names, arguments and
return shapes, computed from one confusion matrix counted on the device (ldiffusion_amd/metrics.py) instead of 2-3 masked sums and `.item()`s per class.
The sampler call site (nnU-Net dataset creation): `copy_or_convert_image`, sampler variant V4
(/root/reference/utils.py:176-208).  Same name, arguments and effect -- a PNG of the one-pass diffusion of the image at `dst_path`, or a plain
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
    sampler = _sampler(pipeline, base)
    out = sampler.sample((x - mean) / std, emb.to(device=device, dtype=torch.float32)[:1], 1, want_features=False, want_rgb=True)
    rgb = out["rgb"][0].cpu().numpy()
    sampler.check_finite()   # fp16 overflow in either graph raises instead of writing a garbage PNG
    Image.fromarray(rgb).save(dst_path)


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


def create_nnunet_dataset(train_images, train_labels, test_images, test_labels, num_classes, pipeline, unet, raw_dir=None):
    """utils.py:210-294: the next `DatasetNNN_Custom` under nnUNet_raw (`raw_dir`, else the environment variable nnUNet_raw) with imagesTr / labelsTr /
    imagesTs / labelsTs, `case_%03d_0000.png` + `case_%03d.png` and `caseTs_%03d...`; every image goes through `copy_or_convert_image` -- the
    one-pass diffusion when ALL train and ALL test images share one size, else a plain copy --, every label is resized to its image (NEAREST) and
    mapped through metrics.PIXEL_TO_LABEL; `dataset.json` as the reference writes it.  Returns (new_num, new_dataset_name)."""
    import json
    import os
    from pathlib import Path
    from PIL import Image
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
    new_num = max_num + 1
    new_dataset_name = f"Dataset{new_num:03d}_Custom"
    new_path = raw_path / new_dataset_name
    new_path.mkdir(parents=True, exist_ok=False)
    for sub in ("imagesTr", "labelsTr", "imagesTs", "labelsTs"):
        (new_path / sub).mkdir()
    n_train = 0
    for images, labels, stem, img_dir, lbl_dir in ((train_images, train_labels, "case", "imagesTr", "labelsTr"), (test_images, test_labels, "caseTs", "imagesTs", "labelsTs")):
        for idx, (img_path, lbl_path) in enumerate(zip(images, labels)):
            case_id = f"{stem}_{idx:03d}"
            img_path = Path(img_path)
            img = Image.open(img_path).convert("RGB")
            lbl = fix_label_size(img, Image.open(lbl_path).convert("L"), img_path.name, lbl_path)
            copy_or_convert_image(img, img_path, new_path / img_dir / f"{case_id}_0000.png", pipeline, unet, use_diffusion)
            convert_and_save_label(lbl, new_path / lbl_dir / f"{case_id}.png", metrics.PIXEL_TO_LABEL)
            n_train += stem == "case"
    dataset_json = {
        "channel_names": {"0": "R", "1": "G", "2": "B"},
        "labels": {"background": 0, **{f"class{i}": i for i in range(1, num_classes)}},
        "numTraining": n_train,
        "file_ending": ".png",
    }
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
