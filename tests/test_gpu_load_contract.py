"""-m gpu: the one checkpoint-load contract of the six handle families (csrc/weight_store.hip, csrc/model.h "checkpoint loading"), at the tests' tiny
configurations.  Tensors go straight through `ldiff_<family>_load`: the Python shims filter unknown names and squeeze 1x1 attention convs before the
library sees them."""
import ctypes as C
import json
import os

import pytest
import torch

import nnunet_ref
import resnet_ref
from ldiffusion_amd import configs, models, nnunet, weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TEXT_CFG = dict(vocab_size=300, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, hidden_act="quick_gelu", max_position_embeddings=77)
TEXT_PROJ = 64
RESNET = dict(layers=(1, 1, 2, 1), width=16, adapter=64, S=32, classes=4)


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _segnet_spec():
    with open(os.path.join(GOLDEN, "nnunet_plans_2d.json")) as f:
        plans = json.load(f)
    with open(os.path.join(GOLDEN, "nnunet_dataset.json")) as f:
        ds = json.load(f)
    return nnunet.network_spec(plans, "2d_reduced", ds)


CLASSES = {"unet": models.UNet2DConditionModel, "controlnet": models.ControlNetModel, "vae": models.AutoencoderKL, "segnet": models.PlainConvUNet,
           "resnet": models.ResNetClassifier, "textenc": models.CLIPTextModel}


def _family(name):
    """(checkpoint in the library's names, build(cls, sd) -> handle, run(handle) -> its outputs as a tuple) of a family at its tiny configuration."""
    if name in ("unet", "controlnet"):
        cfg = configs.TINY_UNET if name == "unet" else configs.TINY_CONTROLNET
        x, ctx = _rand((1, 4, 8, 8), 1).to(DEV), _rand((1, 5, cfg["cross_attention_dim"]), 2, 0.5).to(DEV)
        cond = torch.rand((1, 3, 64, 64), generator=torch.Generator().manual_seed(3)).to(DEV)
        if name == "unet":
            return weights.synthetic_state_dict(weights.unet_param_shapes(cfg), 42), lambda cls, sd: cls(cfg, sd, DEV), lambda net: (net(x, 501, ctx).sample,)

        def run(net):
            down, mid = net(x, 501, ctx, cond, return_dict=False)
            return tuple(down) + (mid,)
        return weights.synthetic_state_dict(weights.controlnet_param_shapes(cfg), 44), lambda cls, sd: cls(cfg, sd, DEV), run
    if name == "vae":
        cfg = configs.TINY_VAE
        z, img = _rand((1, cfg["latent_channels"], 8, 8), 4, 0.3).to(DEV), torch.rand((1, 3, 32, 32), generator=torch.Generator().manual_seed(5)).to(DEV)
        return (weights.normalize_vae_keys(weights.synthetic_state_dict(weights.vae_param_shapes(cfg), 43)), lambda cls, sd: cls(cfg, sd, DEV),
                lambda net: (net.decode(z).sample, net.encode(img).latent_dist.mean))
    if name == "segnet":
        spec = _segnet_spec()
        x = _rand((1, spec["in_channels"], 64, 64), 6).to(DEV)
        return nnunet_ref.synthetic_state_dict(spec, 41), lambda cls, sd: cls(spec, sd, DEV), lambda net: (net(x),)
    if name == "resnet":
        r = RESNET
        x = resnet_ref.to_nhwc8(_rand((2, 3, r["S"], r["S"]), 7)).to(DEV)
        return (resnet_ref.synthetic_state_dict(r["layers"], r["width"], r["classes"], 22, 0.25, r["adapter"]),
                lambda cls, sd: cls(r["classes"], sd, DEV, r["layers"], r["width"], r["adapter"]), lambda net: tuple(net(x)))
    assert name == "textenc"
    ids = torch.randint(0, TEXT_CFG["vocab_size"], (2, 5), generator=torch.Generator().manual_seed(8))

    def build(cls, sd):   # the projection goes through load_projection, which states its width
        enc = cls(TEXT_CFG, {k: v for k, v in sd.items() if not k.startswith("proj.")}, DEV)
        return enc.load_projection({"weight": sd["proj.weight"], "bias": sd["proj.bias"]}) if "proj.weight" in sd else enc
    return weights.synthetic_state_dict(weights.clip_text_param_shapes(TEXT_CFG, TEXT_PROJ), 9), build, lambda net: (net.project(ids),)


def _lenient(cls):
    """The class with the shim's check for missing tensors turned off: built from an empty checkpoint it is a handle with nothing loaded."""
    class Lenient(cls):
        def load_state_dict(self, sd, strict=True):
            return cls.load_state_dict(self, sd, strict=False)
    return Lenient


def raw_load(net, name, t, dtype=None):
    """ldiff_<family>_load on the tensor as it is -> (status, message)."""
    t = t.detach().cpu().contiguous()
    shape = (C.c_int64 * max(t.dim(), 1))(*t.shape)
    code = models._DTYPES[t.dtype] if dtype is None else dtype
    rc = net._fn("load")(net._h, name.encode(), C.c_void_p(t.data_ptr()), code, shape, t.dim())
    return rc, net._lib.ldiff_last_error().decode()


def _exact_in_16_bits(sd):
    """The checkpoint with every value rounded to bfloat16 and what fp16 cannot hold as a normal number flushed: exact in float32, float16 and bfloat16."""
    out = {}
    for k, v in sd.items():
        v = v.to(torch.bfloat16).float()
        v = torch.where(v.abs() < 2.0 ** -14, torch.zeros_like(v), v).clamp(-60000.0, 60000.0).to(torch.bfloat16).float()
        assert torch.equal(v.to(torch.float16).float(), v) and torch.equal(v.to(torch.bfloat16).float(), v)
        out[k] = v
    return out


@pytest.mark.parametrize("name", list(CLASSES))
def test_one_load_contract(name):
    sd, build, run = _family(name)
    sd = _exact_in_16_bits(sd)
    net = build(_lenient(CLASSES[name]), {})
    fn = net._fn
    registered = len(sd) - (2 if name == "textenc" else 0)   # (the text encoder's projection is registered by its first tensor)
    assert fn("missing")(net._h) == registered
    # refusals: an unknown name, a known name with one extent off, a dtype code outside F32 / F16 / BF16
    rc, msg = raw_load(net, "no.such.tensor", torch.zeros(3))
    assert rc == -1 and "unexpected tensor name" in msg, (rc, msg)
    probe = next(k for k, v in sd.items() if v.dim() in (1, 4))   # (registered with the shape the checkpoint states it in)
    good = list(sd[probe].shape)
    bad = [good[0] + 1] + good[1:]
    rc, msg = raw_load(net, probe, torch.zeros(bad))
    assert rc == -1 and "does not match expected" in msg, (rc, msg)
    assert "[" + ",".join(map(str, bad)) + "]" in msg and "[" + ",".join(map(str, good)) + "]" in msg, msg
    rc, msg = raw_load(net, probe, sd[probe], dtype=7)
    assert rc == -1 and "unsupported dtype" in msg, (rc, msg)
    assert fn("missing")(net._h) == registered, "a refused load must not count as loaded"
    # the checkpoint without its third-listed tensor
    third = list(sd)[2]
    for k, v in sd.items():
        if k != third:
            rc, msg = raw_load(net, k, v)
            assert rc == 0, (k, msg)
    assert fn("missing")(net._h) == 1 and fn("missing_name")(net._h, 0).decode() == third
    assert raw_load(net, third, sd[third])[0] == 0 and fn("missing")(net._h) == 0
    if name == "textenc":
        net.projection_dim = TEXT_PROJ   # (the shim's own record of what load_projection loaded)
    # the same values as float32, float16 and bfloat16 tensors: bit-identical forwards
    ref = [t.clone() for t in run(net)]
    net.check_finite()
    for dt in (torch.float16, torch.bfloat16):
        other = build(CLASSES[name], {k: v.to(dt) for k, v in sd.items()})
        got = run(other)
        other.check_finite()
        assert len(got) == len(ref) and all(torch.equal(g, r) for g, r in zip(got, ref)), f"{name}: a {dt} checkpoint gives other bits than the float32 one"
    assert all(bool(torch.isfinite(r.float()).all()) for r in ref)


def test_matrix_rule_takes_1x1_convs_as_rank_2_or_rank_4():
    """The mid-block attention projections of the tiny VAE as [C, C] and as [C, C, 1, 1] (what older diffusers checkpoints hold): bit-identical results."""
    cfg = configs.TINY_VAE
    sd = weights.synthetic_state_dict(weights.vae_param_shapes(cfg), 43, fp16_values=True)
    z, img = _rand((1, cfg["latent_channels"], 8, 8), 4, 0.3).to(DEV), torch.rand((1, 3, 32, 32), generator=torch.Generator().manual_seed(5)).to(DEV)
    run = lambda vae: (vae.decode(z).sample.clone(), vae.encode(img).latent_dist.mean.clone())
    ref = run(models.AutoencoderKL(cfg, sd, DEV))
    proj = [k for k in weights.normalize_vae_keys(sd) if ".attentions." in k and k.endswith(".weight") and "group_norm" not in k]
    assert len(proj) == 8 and all(sd[k].dim() == 2 for k in proj)   # q, k, v, out of the encoder's and the decoder's mid block
    vae = models.AutoencoderKL(cfg, {k: (v * 0.5 if k in proj else v) for k, v in sd.items()}, DEV)
    assert not torch.equal(run(vae)[0], ref[0])
    for k in proj:
        rc, msg = raw_load(vae, k, sd[k][:, :, None, None])
        assert rc == 0, (k, msg)
    got = run(vae)
    vae.check_finite()
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


def test_exact_rule_refuses_another_rank():
    """The classifier's tensors are registered under the exact rule: the same elements in another rank are refused."""
    r = RESNET
    sd = resnet_ref.synthetic_state_dict(r["layers"], r["width"], r["classes"], 22, 0.25, r["adapter"])
    net = models.ResNetClassifier(r["classes"], sd, DEV, r["layers"], r["width"], r["adapter"])
    w, w1 = sd["adapter.weight"], sd["encoder.4.0.conv1.weight"]
    assert w.dim() == 4 and w1.dim() == 4 and w1.shape[2:] == (1, 1)
    for name, wrong in (("adapter.weight", w.reshape(w.shape[0], -1)), ("adapter.weight", w.reshape(w.shape[0], w.shape[1], -1)),
                        ("encoder.4.0.conv1.weight", w1[:, :, 0, 0])):   # (the last: what the matrix rule would take)
        rc, msg = raw_load(net, name, wrong)
        assert rc == -1 and "does not match expected" in msg and "resnet_load" in msg, (rc, msg)
    assert net._fn("missing")(net._h) == 0
