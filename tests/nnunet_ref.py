"""nnU-Net v2 `PlainConvUNet` (2-D) forward restated in plain torch (helper of the tissue-head tests; TEST INFRASTRUCTURE ONLY).

Follows the public algorithm of `dynamic_network_architectures.architectures.unet.PlainConvUNet` as nnU-Net's get_network_from_plans
configures it: per encoder stage conv3x3 (bias; the first with the stage's stride) -> InstanceNorm2d(eps 1e-5, affine) -> LeakyReLU(0.01), repeated
n_conv times; per decoder stage ConvTranspose2d(kernel = stride), cat((upsampled, skip), 1), the conv blocks again; the last 1x1 seg layer (deep
supervision off).  That package is on no machine the suite runs on, so this is an independent restatement, not a recording;
tests/test_cpu_nnunet.py checks it against a second statement assembled from torch.nn modules.

`dtype` is the arithmetic of the whole forward.  `store` (optional) is applied to every weight, to the input and to every tensor a module of the
plain graph hands on (conv / transposed-conv outputs, the normalised + activated tensors): `fp16_storage` makes it the fp16-storage model of the GPU
tests -- float64 arithmetic with everything that would live in memory under `torch.autocast(fp16)` rounded to fp16 once."""
import torch
import torch.nn.functional as F

from ldiffusion_amd import nnunet

EPS, SLOPE = 1e-5, 0.01


def fp16_storage(t):
    return t.to(torch.float16).to(t.dtype)


def _block(sd, prefix, x, stride, store):
    y = store(F.conv2d(x, store(sd[prefix + ".conv.weight"]), sd[prefix + ".conv.bias"], stride=stride, padding=1))
    y = F.instance_norm(y, weight=sd[prefix + ".norm.weight"], bias=sd[prefix + ".norm.bias"], eps=EPS)
    return store(F.leaky_relu(y, SLOPE))


def forward(sd, spec, x, dtype=torch.float64, store=None):
    """x [B, C, H, W] -> logits [B, heads, H, W] in `dtype`."""
    store = store or (lambda t: t)
    sd = {k: v.to(dtype) for k, v in sd.items()}
    h = store(x.to(dtype))
    n = spec["n_stages"]
    skips = []
    for s in range(n):
        for i in range(spec["n_conv_encoder"][s]):
            h = _block(sd, f"encoder.stages.{s}.0.convs.{i}", h, spec["strides"][s] if i == 0 else 1, store)
        skips.append(h)
    for j in range(n - 1):
        st = spec["strides"][n - 1 - j]
        up = store(F.conv_transpose2d(h, store(sd[f"decoder.transpconvs.{j}.weight"]), sd[f"decoder.transpconvs.{j}.bias"], stride=st))
        h = torch.cat((up, skips[n - 2 - j]), 1)
        for i in range(spec["n_conv_decoder"][j]):
            h = _block(sd, f"decoder.stages.{j}.convs.{i}", h, 1, store)
    return F.conv2d(h, store(sd[f"decoder.seg_layers.{n - 2}.weight"]), sd[f"decoder.seg_layers.{n - 2}.bias"])


def synthetic_state_dict(spec, seed, fp16_values=True, gain=1.0):
    """Seeded weights with He-like scale (activations stay O(1) through the InstanceNorms), norm weights around 1, values fp16-representable."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in nnunet.param_shapes(spec).items():
        if name.endswith("norm.weight"):
            t = 1.0 + 0.2 * torch.randn(shape, generator=g)
        elif name.endswith("bias"):
            t = 0.1 * torch.randn(shape, generator=g)
        elif "transpconvs" in name:
            t = torch.randn(shape, generator=g) * (gain / shape[0]) ** 0.5
        else:
            t = torch.randn(shape, generator=g) * (gain * 2.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
        sd[name] = t.to(torch.float16).float() if fp16_values else t
    return sd


def checkpoint_like(sd, spec, compiled=False):
    """The key set a real checkpoint's `network_weights` holds: the canonical names plus the `all_modules` views, the decoder's reference to the encoder
    and every deep-supervision head, optionally behind `_orig_mod.`."""
    out = dict(sd)
    for k, v in sd.items():
        for part, idx in ((".conv.", 0), (".norm.", 1)):
            if part in k and ".convs." in k:
                out[k.replace(part, f".all_modules.{idx}.")] = v
    for k in list(out):
        if k.startswith("encoder."):
            out["decoder." + k] = out[k]
    n, f = spec["n_stages"], spec["features"]
    for j in range(n - 2):
        out[f"decoder.seg_layers.{j}.weight"] = torch.zeros((spec["n_heads"], f[n - 2 - j], 1, 1))
        out[f"decoder.seg_layers.{j}.bias"] = torch.zeros((spec["n_heads"],))
    return {("_orig_mod." + k if compiled else k): v for k, v in out.items()}


def write_model_folder(path, plans, dataset_json, sd, spec, configuration="2d", mirror_axes=(0, 1), compiled=False):
    """A trained-model folder as nnU-Net leaves it: dataset.json, plans.json, fold_0/checkpoint_best.pth."""
    import json
    import os
    os.makedirs(os.path.join(path, "fold_0"), exist_ok=True)
    with open(os.path.join(path, "dataset.json"), "w") as f:
        json.dump(dataset_json, f)
    with open(os.path.join(path, "plans.json"), "w") as f:
        json.dump(plans, f)
    torch.save({"network_weights": checkpoint_like(sd, spec, compiled), "init_args": {"configuration": configuration}, "trainer_name": "nnUNetTrainer",
                "inference_allowed_mirroring_axes": mirror_axes}, os.path.join(path, "fold_0", "checkpoint_best.pth"))
    return path
