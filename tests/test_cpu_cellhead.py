"""CPU: the cell head's host side (ldiffusion_amd/cellhead.py) -- checkpoint names and shapes, what is refused, instance boxes, the lookup table of
the reference's wrapping cast -- and the float64 yardstick of the GPU tests (tests/resnet_ref.py) against a second statement built from torch.nn
modules, plus the BatchNorm fold the library performs at load time."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import resnet_ref
from ldiffusion_amd import cellhead

LAYERS, WIDTH, ADAPTER, NC = (1, 1, 2, 1), 16, 32, 4


# ---- 1. the restatement against a second statement assembled from modules; load_state_dict(strict=True) pins the names ----------------------------
class Bottleneck(nn.Module):
    def __init__(self, inplanes, planes, stride, down):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, 4 * planes, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(4 * planes)
        self.relu = nn.ReLU()
        self.downsample = nn.Sequential(nn.Conv2d(inplanes, 4 * planes, 1, stride, bias=False), nn.BatchNorm2d(4 * planes)) if down else None

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return self.relu(out + (x if self.downsample is None else self.downsample(x)))


class Classifier(nn.Module):
    def __init__(self, layers, width, adapter, nc):
        super().__init__()
        mods = [nn.Conv2d(3, width, 7, 2, 3, bias=False), nn.BatchNorm2d(width), nn.ReLU(), nn.MaxPool2d(3, 2, 1)]
        inplanes = width
        for li, n in enumerate(layers):
            blocks = []
            for b in range(n):
                blocks.append(Bottleneck(inplanes, width << li, 2 if (b == 0 and li > 0) else 1, b == 0))
                inplanes = 4 * (width << li)
            mods.append(nn.Sequential(*blocks))
        self.encoder = nn.Sequential(*mods)
        self.adapter = nn.Conv2d(inplanes, adapter, 3, padding=1)
        self.classifier = nn.Linear(adapter, nc)

    def forward(self, x):
        return self.classifier(F.adaptive_avg_pool2d(self.adapter(self.encoder(x)), (1, 1)).flatten(1))


def test_restatement_matches_a_module_statement_and_the_names_load_strictly():
    sd = resnet_ref.synthetic_state_dict(LAYERS, WIDTH, NC, 3, adapter_channels=ADAPTER)
    m = Classifier(LAYERS, WIDTH, ADAPTER, NC).double().eval()
    names = set(m.state_dict())
    assert names == set(cellhead.param_shapes(NC, LAYERS, WIDTH, ADAPTER, counters=True))
    full = dict(sd, **{k: torch.tensor(0) for k in names if k.endswith("num_batches_tracked")})
    m.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in full.items()}, strict=True)
    x = torch.randn((3, 3, 64, 64), generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    with torch.no_grad():
        want = m(x)
    got = resnet_ref.forward(sd, LAYERS, x, torch.float64)
    assert got.shape == (3, NC)
    assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    # ResNet152's own shapes: 155 convs and 155 BatchNorms in the trunk + adapter + classifier
    full152 = cellhead.param_shapes(7)
    assert sum(1 for k in full152 if k.endswith("running_var")) == 155 and full152["adapter.weight"] == (256, 2048, 3, 3)
    assert full152["encoder.6.35.conv2.weight"] == (256, 256, 3, 3) and full152["encoder.7.0.downsample.0.weight"] == (2048, 1024, 1, 1)
    assert full152["encoder.4.0.downsample.0.weight"] == (256, 64, 1, 1) and "encoder.4.1.downsample.0.weight" not in full152


# ---- 2. the fold the library performs on the host against F.batch_norm ---------------------------------------------------------------------------
def test_batchnorm_fold_against_batch_norm():
    """w' = w gamma / sqrt(var + eps), b' = beta - mean gamma / sqrt(var + eps) in double (csrc/model_cls.hip fold()) gives conv(x, w') + b' == bn(conv(x, w))."""
    g = torch.Generator().manual_seed(2)
    w = torch.randn((24, 16, 3, 3), generator=g, dtype=torch.float64)
    gamma, beta = 1 + 0.2 * torch.randn(24, generator=g, dtype=torch.float64), torch.randn(24, generator=g, dtype=torch.float64)
    mean, var = torch.randn(24, generator=g, dtype=torch.float64), 0.5 + torch.rand(24, generator=g, dtype=torch.float64)
    x = torch.randn((2, 16, 9, 7), generator=g, dtype=torch.float64)
    want = F.batch_norm(F.conv2d(x, w, None, 2, 1), mean, var, gamma, beta, False, 0.0, 1e-5)
    s = gamma / torch.sqrt(var + 1e-5)
    got = F.conv2d(x, w * s[:, None, None, None], beta - mean * s, 2, 1)
    assert (got - want).abs().max().item() <= 1e-13 * want.abs().max().item()
    wrong = F.conv2d(x, w * (gamma / torch.sqrt(var + 1e-3))[:, None, None, None], beta - mean * s, 2, 1)
    assert (wrong - want).abs().max().item() > 1e-5


# ---- 3. instance boxes against the reference-style loop -------------------------------------------------------------------------------------------
def reference_boxes(masks):
    """The loop of the reference's CellSegClassifier.forward over np.unique / np.where."""
    ids, boxes = [], []
    for inst in np.unique(masks):
        if inst == 0:
            continue
        ys, xs = np.where(masks == inst)
        y1, y2, x1, x2 = ys.min(), ys.max(), xs.min(), xs.max()
        if y2 - y1 < 4 or x2 - x1 < 4:
            continue
        ids.append(int(inst))
        boxes.append((int(x1), int(y1), int(x2), int(y2)))
    return ids, boxes


def label_map():
    m = np.zeros((40, 52), np.int64)
    m[2:7, 3:8] = 5          # 5 x 5: kept (y2 - y1 = 4)
    m[2:6, 10:20] = 9        # 4 rows: skipped
    m[10:20, 10:14] = 2      # 4 columns: skipped
    m[10:20, 14:19] = 3      # touches instance 2, 5 columns: kept
    m[25:40, 30:52] = 40     # reaches the border
    m[30:33, 35:38] = 41     # a small one inside another's box: skipped
    yy, xx = np.mgrid[:40, :52]
    m[(yy - 8) ** 2 + (xx - 40) ** 2 <= 30] = 17   # a disc
    return m


def test_instance_boxes_against_the_reference_loop():
    m = label_map()
    ids, boxes = cellhead.instance_boxes(torch.from_numpy(m))
    rids, rboxes = reference_boxes(m)
    assert ids.tolist() == rids and boxes.tolist() == [list(b) for b in rboxes]
    assert boxes.dtype == torch.int32 and 9 not in rids and 2 not in rids and 41 not in rids and {3, 5, 17, 40} <= set(rids)
    ids0, boxes0 = cellhead.instance_boxes(torch.zeros((8, 8), dtype=torch.int32))
    assert ids0.numel() == 0 and tuple(boxes0.shape) == (0, 4)


# ---- 4. the lookup table against numpy's own cast -------------------------------------------------------------------------------------------------
def test_build_lut_against_numpy_cast():
    lut = cellhead.build_lut()
    assert lut.shape == (3, 256) and lut.dtype == np.uint8
    u = np.arange(256, dtype=np.uint8)
    img = np.stack([u, u, u], -1)[None]                                                                  # [1, 256, 3]
    x = torch.from_numpy(img).permute(2, 0, 1).float().div(255)                                          # ToTensor
    x = (x - torch.tensor(cellhead.IMAGENET_MEAN).view(3, 1, 1)) / torch.tensor(cellhead.IMAGENET_STD).view(3, 1, 1)   # Normalize (float32)
    patch = x.permute(1, 2, 0).numpy()
    with np.errstate(invalid="ignore"):
        cast = (patch * 255).astype(np.uint8)                                                            # conductor.py:201
    assert np.array_equal(cast[0].T, lut)
    assert lut[0, 0] != 0 and (np.diff(lut[0].astype(int)) < 0).any()                                    # it wraps: not monotonic


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_check_state_dict_refusals():
    sd = resnet_ref.synthetic_state_dict(LAYERS, WIDTH, NC, 4, adapter_channels=ADAPTER)
    assert cellhead.check_state_dict(sd, NC, LAYERS, WIDTH, ADAPTER)
    assert cellhead.infer_spec(sd) == (NC, LAYERS, WIDTH, ADAPTER)
    assert cellhead.check_state_dict(dict(sd, **{"encoder.1.num_batches_tracked": torch.tensor(3)}), NC, LAYERS, WIDTH, ADAPTER)
    with pytest.raises(ValueError, match="unexpected.*fc.weight"):
        cellhead.check_state_dict(dict(sd, **{"fc.weight": torch.zeros(1)}), NC, LAYERS, WIDTH, ADAPTER)
    with pytest.raises(ValueError, match="missing.*encoder.5.0.bn2.running_var"):
        cellhead.check_state_dict({k: v for k, v in sd.items() if k != "encoder.5.0.bn2.running_var"}, NC, LAYERS, WIDTH, ADAPTER)
    with pytest.raises(ValueError, match="adapter.weight has shape"):
        cellhead.check_state_dict(dict(sd, **{"adapter.weight": torch.zeros((ADAPTER, 8 * WIDTH * 4, 1, 1))}), NC, LAYERS, WIDTH, ADAPTER)
    with pytest.raises(ValueError, match="missing"):
        cellhead.check_state_dict(sd, NC, (1, 1, 3, 1), WIDTH, ADAPTER)


def test_read_cellclassifier_roundtrip(tmp_path):
    sd = resnet_ref.synthetic_state_dict(LAYERS, WIDTH, NC, 5, adapter_channels=ADAPTER)
    torch.save({("module." + k): v for k, v in sd.items()}, tmp_path / "cellclassifier.pth")
    back = cellhead.read_cellclassifier(str(tmp_path))
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    torch.save({k: v for k, v in sd.items() if k != "classifier.bias"}, tmp_path / "cellclassifier.pth")
    with pytest.raises(ValueError, match="classifier.bias"):
        cellhead.read_cellclassifier(str(tmp_path / "cellclassifier.pth"))


def test_inference_cell_model_without_head_or_weights_still_raises(tmp_path):
    from ldiffusion_amd.segmentor import Segmentor
    seg = Segmentor.__new__(Segmentor)      # (the constructor wants a GPU; the refusal comes before anything touches one)
    seg.level, seg.num_classes, seg.device = "cell", 3, torch.device("cpu")
    with pytest.raises(RuntimeError, match="cellclassifier.pth"):
        seg.inference_cell_model("x.png", "sd", "w", None)
    with pytest.raises(RuntimeError, match="head="):
        seg.inference_cell_model("x.png", "sd", "w", str(tmp_path))     # a folder without cellclassifier.pth


def test_missing_cellpose_names_the_instances_argument(monkeypatch):
    import sys
    monkeypatch.setitem(sys.modules, "cellpose", None)      # `import cellpose` raises ImportError, whether or not the package is installed
    with pytest.raises(RuntimeError, match="instances="):
        cellhead._default_instances()
