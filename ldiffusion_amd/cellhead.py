"""The cell head of `LDiffusionModel.inference(level="cell")`: the reference's CellSegClassifier (model/conductor.py:138-233) with its ResNet152
instance classifier on the HIP library (`models.ResNetClassifier`, include/ldiff.h ldiff_resnet_*).

What the reference does per image, restated here:
  1. Cellpose `cyto2` -> an instance label map (third-party; injectable as `instances=`, as the prompt's tokenizer stays `transformers`').
  2. Per instance its bounding box; instances with y2 - y1 < 4 or x2 - x1 < 4 are skipped.
  3. The crop of the ImageNet-NORMALISED image goes through `(patch * 255).astype(np.uint8)` -> ToTensor -> Resize((64, 64)) -> Normalize: a
     second normalisation on top of a wrapping cast.  Per pixel that is a function of the decoded uint8 value alone: `build_lut`.
  4. torchvision ResNet152 without avgpool / fc, `adapter` = Conv2d(2048, 256, 3, padding=1), global average pool, Linear(256, C).
  5. class = top-1 over classes 1 .. C - 1; 6. the instance's pixels are painted with it, everything else is 0.

The architecture is restated from the public torchvision definition (UNPINNED: neither torchvision nor cellpose is available to the test-suite;
DESIGN.md section 2)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import _lib

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
RESNET152_LAYERS = (3, 8, 36, 3)
MAX_CROPS_PER_CALL = 256
_BN = ("weight", "bias", "running_mean", "running_var")


def param_shapes(num_classes, layers=RESNET152_LAYERS, width=64, adapter_channels=256, counters=False):
    """name -> shape of the module's state_dict: `encoder` = Sequential(conv1, bn1, relu, maxpool, layer1..4) of torchvision's ResNet
    (v1.5 bottleneck, expansion 4, `downsample` = (1x1 conv, BatchNorm) in the first block of every layer), `adapter`, `classifier`.
    counters=True adds BatchNorm's `num_batches_tracked` scalars (a checkpoint holds them; the forward does not read them)."""
    shapes = {}

    def bn(prefix, c):
        for v in _BN:
            shapes[f"{prefix}.{v}"] = (c,)
        if counters:
            shapes[f"{prefix}.num_batches_tracked"] = ()

    shapes["encoder.0.weight"] = (width, 3, 7, 7)
    bn("encoder.1", width)
    inplanes = width
    for li, nblocks in enumerate(layers):
        planes = width << li
        for b in range(nblocks):
            p = f"encoder.{4 + li}.{b}"
            shapes[f"{p}.conv1.weight"] = (planes, inplanes, 1, 1)
            bn(f"{p}.bn1", planes)
            shapes[f"{p}.conv2.weight"] = (planes, planes, 3, 3)
            bn(f"{p}.bn2", planes)
            shapes[f"{p}.conv3.weight"] = (4 * planes, planes, 1, 1)
            bn(f"{p}.bn3", 4 * planes)
            if b == 0:
                shapes[f"{p}.downsample.0.weight"] = (4 * planes, inplanes, 1, 1)
                bn(f"{p}.downsample.1", 4 * planes)
            inplanes = 4 * planes
    shapes["adapter.weight"] = (adapter_channels, inplanes, 3, 3)
    shapes["adapter.bias"] = (adapter_channels,)
    shapes["classifier.weight"] = (num_classes, adapter_channels)
    shapes["classifier.bias"] = (num_classes,)
    return shapes


def check_state_dict(sd, num_classes, layers=RESNET152_LAYERS, width=64, adapter_channels=256):
    """Refuses (ValueError, naming the tensor) a state dict that is not this architecture's: unexpected names, missing names, wrong shapes.
    `num_batches_tracked` entries are accepted."""
    want = param_shapes(num_classes, layers, width, adapter_channels)
    extra = [k for k in sd if k not in want and not k.endswith("num_batches_tracked")]
    if extra:
        raise ValueError(f"cell classifier checkpoint: unexpected tensors {extra[:5]}{' ...' if len(extra) > 5 else ''}")
    missing = [k for k in want if k not in sd]
    if missing:
        raise ValueError(f"cell classifier checkpoint: missing tensors {missing[:5]}{' ...' if len(missing) > 5 else ''}")
    for k, shape in want.items():
        if tuple(sd[k].shape) != tuple(shape):
            raise ValueError(f"cell classifier checkpoint: {k} has shape {tuple(sd[k].shape)}, expected {tuple(shape)}")
    return True


def infer_spec(sd):
    """(num_classes, layers, width, adapter_channels) from a state dict's names and shapes."""
    for k in ("encoder.0.weight", "adapter.weight", "classifier.weight"):
        if k not in sd:
            raise ValueError(f"cell classifier checkpoint: {k} is missing")
    layers = []
    for li in range(4):
        blocks = {int(k.split(".")[2]) for k in sd if k.startswith(f"encoder.{4 + li}.") and k.split(".")[2].isdigit()}
        if not blocks or blocks != set(range(len(blocks))):
            raise ValueError(f"cell classifier checkpoint: encoder.{4 + li} has no consecutive blocks 0..n-1")
        layers.append(len(blocks))
    return int(sd["classifier.weight"].shape[0]), tuple(layers), int(sd["encoder.0.weight"].shape[0]), int(sd["adapter.weight"].shape[0])


def read_cellclassifier(path):
    """`segmentor_weight/cellclassifier.pth` (the module's state_dict, torch.load(weights_only=True) as segmentor.py:497) -> state dict, checked
    against the architecture its own shapes imply.  `path` is the folder or the file."""
    if os.path.isdir(path):
        path = os.path.join(path, "cellclassifier.pth")
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: expected a state_dict, got {type(sd).__name__}")
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
    check_state_dict(sd, *infer_spec(sd))
    return sd


def _instance_table(labels):
    """(ids [n] int64 ascending: every value of the map, inv [H * W]: index of each pixel's id, keep [n] bool, boxes [n, 4] int64)."""
    if labels.dim() != 2:
        raise ValueError(f"instance_boxes: label map must be [H, W], got {list(labels.shape)}")
    labels = labels.to(torch.int64)
    H, W = labels.shape
    ids, inv = torch.unique(labels, return_inverse=True)
    inv = inv.reshape(-1)
    n = ids.numel()
    dev = labels.device
    # the background is most of a slide and would be hundreds of thousands of atomic updates of ONE address: only the instances' pixels are reduced
    fg = torch.nonzero(labels.reshape(-1) != 0).reshape(-1)
    idx = inv[fg]
    ys, xs = (fg // W).to(torch.int32), (fg % W).to(torch.int32)
    y1 = torch.full((n,), H, dtype=torch.int32, device=dev).scatter_reduce(0, idx, ys, "amin")
    y2 = torch.full((n,), -1, dtype=torch.int32, device=dev).scatter_reduce(0, idx, ys, "amax")
    x1 = torch.full((n,), W, dtype=torch.int32, device=dev).scatter_reduce(0, idx, xs, "amin")
    x2 = torch.full((n,), -1, dtype=torch.int32, device=dev).scatter_reduce(0, idx, xs, "amax")
    keep = (ids != 0) & (y2 - y1 >= 4) & (x2 - x1 >= 4)
    return ids, inv, keep, torch.stack([x1, y1, x2, y2], 1)


def instance_boxes(labels):
    """Bounding boxes of a label map, on the tensor's device: (ids [n] int64 ascending, boxes [n, 4] int32 = x1, y1, x2, y2 inclusive) of every
    instance id != 0 except those with y2 - y1 < 4 or x2 - x1 < 4 (conductor.py:192-198: np.unique order, np.where extrema, the skip rule)."""
    ids, _, keep, boxes = _instance_table(labels)
    return ids[keep].contiguous(), boxes[keep].to(torch.int32).contiguous()


def build_lut(mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """uint8 [3, 256]: what a decoded grey level u of channel c becomes on the reference's way into the classifier -- normalised in float32
    ((u / 255 - mean_c) / std_c, segmentor.py:505-509, 533), then `(patch * 255).astype(np.uint8)` (conductor.py:201): the float is truncated
    towards zero and WRAPS modulo 256 (most normalised values are negative or above 1).  The wrap is what numpy does on x86-64 (checked
    against numpy 2.2.6, contiguous and strided arrays); C leaves an out-of-range float -> uint8 conversion undefined, so it is restated here
    explicitly as trunc then modulo, not delegated to a cast."""
    u = np.arange(256, dtype=np.float32) / np.float32(255.0)
    lut = np.empty((3, 256), np.uint8)
    for c in range(3):
        v = ((u - np.float32(mean[c])) / np.float32(std[c])) * np.float32(255.0)
        lut[c] = (np.trunc(v).astype(np.int64) % 256).astype(np.uint8)
    return lut


def instance_targets(label_map, mask, num_classes):
    """The training target of every kept instance (the instances and the order of `instance_boxes`): int64 [n], the majority class among the classes
    1 .. C - 1 of the mask's pixels under the instance, a tie to the lowest class, -1 where the instance covers no foreground pixel of the mask.
    A mask of another size than the label map is resized with nearest neighbour first, as the reference's MicroDiceLoss resizes its targets
    (model/loss.py:144-145: F.interpolate(mode="nearest"))."""
    label_map = torch.as_tensor(label_map)
    mask = torch.as_tensor(mask).to(label_map.device)
    if mask.dim() != 2:
        raise ValueError(f"instance_targets: mask must be [H, W], got {list(mask.shape)}")
    if tuple(mask.shape) != tuple(label_map.shape):
        mask = torch.nn.functional.interpolate(mask[None, None].float(), size=tuple(label_map.shape), mode="nearest")[0, 0]
    mask = mask.to(torch.int64).reshape(-1)
    ids, inv, keep, _ = _instance_table(label_map)
    C_ = int(num_classes)
    fg = (mask >= 1) & (mask < C_)
    counts = torch.zeros((ids.numel(), C_), dtype=torch.int64, device=label_map.device)
    counts.view(-1).scatter_add_(0, inv[fg] * C_ + mask[fg], torch.ones(int(fg.sum()), dtype=torch.int64, device=label_map.device))
    counts = counts[keep][:, 1:]
    best = counts.max(dim=1).values
    first = (counts == best[:, None]).to(torch.int64).argmax(dim=1)      # the first maximum = the lowest class of a tie
    return torch.where(best > 0, first + 1, torch.full_like(first, -1))


def ema_update(state_dict, bn_layout, batch_mean, batch_var, momentum=0.1):
    """What one training-mode forward does to the BatchNorms' buffers in torch: running = (1 - momentum) * running + momentum * batch, in float32, the
    variance being the UNBIASED batch variance (`ResNetClassifier.forward_train` returns that), and `num_batches_tracked` += 1 (int64).
    `bn_layout`: (prefix, offset, channels) per BatchNorm; batch_mean / batch_var: flat [T].  Updates `state_dict` in place and returns it."""
    bm = torch.as_tensor(batch_mean).detach().to("cpu", torch.float32)
    bv = torch.as_tensor(batch_var).detach().to("cpu", torch.float32)
    m = torch.tensor(momentum, dtype=torch.float32)
    for prefix, off, ch in bn_layout:
        for name, batch in (("running_mean", bm), ("running_var", bv)):
            run = state_dict[f"{prefix}.{name}"].detach().to("cpu", torch.float32)
            # torch's kernel: running = momentum * batch + (1 - momentum) * running
            state_dict[f"{prefix}.{name}"] = m * batch[off:off + ch] + (1 - m) * run
        k = f"{prefix}.num_batches_tracked"
        state_dict[k] = (torch.as_tensor(state_dict[k]).to(torch.int64) if k in state_dict else torch.zeros((), dtype=torch.int64)) + 1
    return state_dict


def _default_instances():
    """Cellpose `cyto2`, built lazily as conductor.py:156-160, 180 does; RuntimeError naming `instances=` where cellpose is not installed."""
    try:
        from cellpose import models as cp_models
    except Exception as e:   # noqa: BLE001
        raise RuntimeError("CellSegClassifier: cellpose is not installed, so the instance label map cannot be computed here; pass "
                           "`instances=` (a callable: normalised HWC float32 image -> int label map [H, W], 0 = background)") from e
    model = cp_models.CellposeModel(pretrained_model="cyto2", gpu=True)

    def run(image_np):
        masks, _, _ = model.eval(image_np, diameter=None, channels=[0, 0])
        return masks
    return run


class CellSegClassifier:
    """`head(model_input [1, 3, H, W] normalised float) -> [1, C, H, W]` one-hot float, the protocol of `Segmentor.inference_cell_model(head=)`,
    and `predict_mask(rgb_u8 [H, W, 3] uint8, labels=None, instances=None) -> uint8 [H, W]` on the device.  `instances`: callable mapping the normalised HWC
    float32 image (numpy) to an int label map; absent, Cellpose `cyto2` if it imports, else RuntimeError.
    input_norm=False is the input convention of the reference's TRAINING loop (segmentor.py:263-268, 280-283): the head is handed the augmented image in
    [0, 1], not the ImageNet-normalised one, so `(patch * 255).astype(np.uint8)` is the identity on grey levels (the identity table) and `instances` gets
    the [0, 1] image.  train=True builds the classifier with `ResNetClassifier(train=True)`."""

    def __init__(self, num_classes, state_dict, device=None, instances=None, layers=None, width=None, adapter_channels=None, crop_size=64, input_norm=True, train=False):
        from .models import ResNetClassifier
        nc, lay, wid, ad = infer_spec(state_dict)
        layers = tuple(layers) if layers is not None else lay
        width = width if width is not None else wid
        adapter_channels = adapter_channels if adapter_channels is not None else ad
        if int(num_classes) != nc:
            raise ValueError(f"CellSegClassifier: num_classes = {num_classes}, the checkpoint's classifier has {nc} rows")
        if not 2 <= int(num_classes) <= 256:
            raise ValueError(f"CellSegClassifier: num_classes = {num_classes} outside 2..256 (the mask is uint8)")
        check_state_dict(state_dict, num_classes, layers, width, adapter_channels)
        self.num_classes = int(num_classes)
        self.crop_size = int(crop_size)
        self.net = ResNetClassifier(num_classes, state_dict, device, layers, width, adapter_channels, train=train)
        self.device = self.net.device
        self.input_norm = bool(input_norm)
        self._instances = instances   # the default of this head; predict_mask(instances=) / head(x, instances=) name another for ONE call
        self._cellpose = None
        self._lut = torch.from_numpy(build_lut() if self.input_norm else build_lut((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))).to(self.device)
        self._mean = (C.c_double * 3)(*IMAGENET_MEAN)
        self._std = (C.c_double * 3)(*IMAGENET_STD)

    def _label_map(self, rgb_u8, instances=None):
        instances = instances if instances is not None else self._instances
        if instances is None:
            if self._cellpose is None:
                self._cellpose = _default_instances()
            instances = self._cellpose
        mean = torch.tensor(IMAGENET_MEAN, device=rgb_u8.device, dtype=torch.float32)
        std = torch.tensor(IMAGENET_STD, device=rgb_u8.device, dtype=torch.float32)
        image = rgb_u8.to(torch.float32) / 255.0
        if self.input_norm:
            image = (image - mean) / std
        image = image.cpu().numpy()     # what the reference hands self.model (segmentor.py:533-535; the training loop: the [0, 1] image, :265)
        labels = instances(image)
        return labels if torch.is_tensor(labels) else torch.from_numpy(np.asarray(labels).astype(np.int64))

    def crops(self, rgb_u8, boxes):
        """[n, S, S, 8] float16: the classifier's input for `boxes` (ldiff_op_crop_resize_norm)."""
        H, W = rgb_u8.shape[:2]
        n, S = boxes.shape[0], self.crop_size
        out = torch.empty((n, S, S, 8), dtype=torch.float16, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().ldiff_op_crop_resize_norm(_lib.ptr(rgb_u8), H, W, _lib.ptr(boxes), n, _lib.ptr(self._lut), S, self._mean, self._std,
                                                             _lib.ptr(out), _lib.stream_ptr()))
        return out

    @torch.no_grad()
    def classify(self, rgb_u8, boxes):
        """(logits [n, C] float32, labels [n] int32) of the instances in `boxes` [n, 4] int32, at most MAX_CROPS_PER_CALL crops per launch sequence."""
        logits, labels = [], []
        for i in range(0, boxes.shape[0], MAX_CROPS_PER_CALL):
            lo, la = self.net(self.crops(rgb_u8, boxes[i:i + MAX_CROPS_PER_CALL].contiguous()))
            logits.append(lo)
            labels.append(la)
        return torch.cat(logits), torch.cat(labels)

    @torch.no_grad()
    def predict_mask(self, rgb_u8, labels=None, instances=None):
        if rgb_u8.dim() != 3 or rgb_u8.shape[2] != 3 or rgb_u8.dtype != torch.uint8:
            raise ValueError(f"predict_mask: rgb_u8 must be uint8 [H, W, 3], got {rgb_u8.dtype} {list(rgb_u8.shape)}")
        rgb_u8 = rgb_u8.to(self.device).contiguous()
        if labels is None:
            labels = self._label_map(rgb_u8, instances)
        labels = torch.as_tensor(labels).to(self.device)
        if tuple(labels.shape) != tuple(rgb_u8.shape[:2]):
            raise ValueError(f"predict_mask: label map {list(labels.shape)} against image {list(rgb_u8.shape[:2])}")
        ids, inv, keep, boxes = _instance_table(labels)
        if not bool(keep.any()):
            return torch.zeros(labels.shape, dtype=torch.uint8, device=self.device)
        _, cls = self.classify(rgb_u8, boxes[keep].to(torch.int32).contiguous())
        paint = torch.zeros(ids.numel(), dtype=torch.uint8, device=self.device)
        paint[keep] = cls.to(torch.uint8)      # (num_classes <= 256)
        return paint[inv].reshape(labels.shape)

    @torch.no_grad()
    def __call__(self, model_input, instances=None):
        if model_input.dim() != 4 or model_input.shape[0] != 1 or model_input.shape[1] != 3:
            raise ValueError(f"CellSegClassifier: input must be [1, 3, H, W], got {list(model_input.shape)}")
        mean = torch.tensor(IMAGENET_MEAN, device=model_input.device, dtype=torch.float32).view(3, 1, 1)
        std = torch.tensor(IMAGENET_STD, device=model_input.device, dtype=torch.float32).view(3, 1, 1)
        rgb = ((model_input[0].to(torch.float32) * std + mean) * 255.0).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()   # the decoded uint8 image
        mask = self.predict_mask(rgb, instances=instances)
        return torch.nn.functional.one_hot(mask.to(torch.int64), self.num_classes).permute(2, 0, 1)[None].to(torch.float32)
