"""The cell head's instance classifier restated in plain torch (helper of the cell-head tests; TEST INFRASTRUCTURE ONLY).

Follows the public architecture of torchvision's ResNet (v1.5 bottleneck: 1x1 -> 3x3 carrying the stride -> 1x1 to four times the planes, each
followed by BatchNorm, ReLU after the first two and after the residual add; `downsample` = 1x1 strided conv + BatchNorm in the first block of
every layer) without avgpool / fc, then Conv2d(4 * 8 * width, adapter, 3, padding=1), the mean over the map and a Linear layer.  torchvision is
on no machine the suite runs on, so this is an independent restatement; tests/test_cpu_cellhead.py checks it against a
second statement assembled from torch.nn modules.

BatchNorm is NOT folded here (eval mode, eps 1e-5, F.batch_norm on the running statistics): the library's host-side fold is part of what the
tests check.  `dtype` is the arithmetic of the whole forward.  `store` (optional) is applied to every conv weight, to the input and to every
tensor a module of the plain graph hands on (conv, BatchNorm, ReLU, add, pooling outputs): `fp16_storage` makes it the fp16-storage model of the
GPU tests -- float64 arithmetic with everything that would live in memory under `torch.autocast(fp16)` rounded to fp16 once."""
import torch
import torch.nn.functional as F

from ldiffusion_amd import cellhead

EPS = 1e-5


def fp16_storage(t):
    return t.to(torch.float16).to(t.dtype)


def _bn(sd, p, x, store):
    return store(F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, EPS))


def _conv(sd, p, x, stride, pad, store):
    return store(F.conv2d(x, store(sd[p + ".weight"]), sd.get(p + ".bias"), stride=stride, padding=pad))


def forward(sd, layers, x, dtype=torch.float64, store=None, return_features=False, trace=None):
    """x [B, 3, S, S] -> logits [B, C] in `dtype` (return_features: the pooled adapter features [B, A] instead).  `trace`: optional dict that
    receives max |value| per stage."""
    store = store or (lambda t: t)
    sd = {k: v.to(dtype) for k, v in sd.items() if v.is_floating_point()}
    h = store(x.to(dtype))
    h = store(F.relu(_bn(sd, "encoder.1", _conv(sd, "encoder.0", h, 2, 3, store), store)))
    h = F.max_pool2d(h, 3, 2, 1)
    if trace is not None:
        trace["stem"] = h.abs().max().item()
    for li, nblocks in enumerate(layers):
        for b in range(nblocks):
            p = f"encoder.{4 + li}.{b}"
            stride = 2 if (b == 0 and li > 0) else 1
            t = store(F.relu(_bn(sd, p + ".bn1", _conv(sd, p + ".conv1", h, 1, 0, store), store)))
            t = store(F.relu(_bn(sd, p + ".bn2", _conv(sd, p + ".conv2", t, stride, 1, store), store)))
            t = _bn(sd, p + ".bn3", _conv(sd, p + ".conv3", t, 1, 0, store), store)
            idn = h
            if p + ".downsample.0.weight" in sd:
                idn = _bn(sd, p + ".downsample.1", _conv(sd, p + ".downsample.0", h, stride, 0, store), store)
            h = store(F.relu(t + idn))
        if trace is not None:
            trace[f"layer{li + 1}"] = h.abs().max().item()
    h = _conv(sd, "adapter", h, 1, 1, store)
    feat = store(h.mean((2, 3)))
    if return_features:
        return feat
    return F.linear(feat, sd["classifier.weight"], sd["classifier.bias"])


def labels_of(logits):
    """1 + argmax over classes 1 .. C - 1 (the reference's top-1 of softmax[:, 1:] + 1)."""
    return logits[:, 1:].argmax(1) + 1


def synthetic_state_dict(layers, width, num_classes, seed, bn3_gain=0.25, adapter_channels=256, fp16_values=True):
    """Seeded weights: He-scaled convs, BatchNorm gamma ~ 1 except bn3's ~ bn3_gain (a residual branch that adds a fraction of the stream, as trained
    networks have; with bn3_gain = 1 the stream of a 50-block network grows past fp16's range: the overflow case), beta ~ 0 +- 0.1, running mean ~ 0 +-
    0.1, running var in [1, 1.2].  Conv values fp16-representable."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in cellhead.param_shapes(num_classes, layers, width, adapter_channels).items():
        if name.endswith("running_var"):
            t = 1.0 + 0.2 * torch.rand(shape, generator=g)
        elif name.endswith("running_mean"):
            t = 0.1 * torch.randn(shape, generator=g)
        elif len(shape) == 4:
            t = torch.randn(shape, generator=g) * (2.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
            t = t.to(torch.float16).float() if fp16_values else t
        elif name.startswith("classifier.weight"):
            t = torch.randn(shape, generator=g) / shape[1] ** 0.5
        elif name.endswith(".weight"):   # BatchNorm gamma
            t = (bn3_gain if ".bn3." in name else 1.0) * (1.0 + 0.1 * torch.randn(shape, generator=g))
        else:                            # BatchNorm beta, adapter / classifier bias
            t = 0.1 * torch.randn(shape, generator=g)
        sd[name] = t
    return sd


def fit_classifier(sd, feats, seed):
    """A deep random network gives every crop the same class.  Replaces the classifier by rows that are random directions on the given (float64)
    features centred over the crops: weight = R / spread, bias = -weight . mean, so that the logits of the crops scatter around 0 with O(1) spread."""
    g = torch.Generator().manual_seed(seed)
    C, A = sd["classifier.weight"].shape
    mean = feats.double().mean(0)
    spread = (feats.double() - mean).norm(dim=1).mean().clamp_min(1e-12)
    w = torch.randn((C, A), generator=g, dtype=torch.float64) / spread
    out = dict(sd)
    out["classifier.weight"] = w.float()
    out["classifier.bias"] = (-(w.float().double() @ mean)).float()
    return out


def to_nhwc8(x):
    """[B, 3, S, S] -> [B, S, S, 8] float16, channels 3..7 zero: the classifier's input layout."""
    B, C, H, W = x.shape
    out = torch.zeros((B, H, W, 8), dtype=torch.float16)
    out[..., :C] = x.permute(0, 2, 3, 1).to(torch.float16)
    return out
