"""Drop-in `unet` / `vae` objects backed by the gfx950 HIP library.

They expose exactly the duck-typed surface the reference touches:
  unet(sample, timestep, encoder_hidden_states, ...) -> obj with `.sample` and `[0]`
      /root/reference/segmentor.py:103,205,444,526   ldiffusion.py:160,238   pixel_latent_vector.py:78
  unet.config.cross_attention_dim                     segmentor.py:33,188    ldiffusion.py:142
  UNet2DConditionModel.from_pretrained(dir) / .eval() / .to(device, dtype=) / .save_pretrained(dir)
                                                      segmentor.py:79        ldiffusion.py:139,273
  controlnet(sample=, timestep=, encoder_hidden_states=, controlnet_cond=, return_dict=False) -> (list of 12 tensors, tensor)
                                                      segmentor.py:357-363   (ControlNetModel below; the reference imports diffusers' class)
  vae.encode(x).latent_dist.mean / .sample();  vae.decode(z).sample;  .to() / .eval()
                                                      segmentor.py:99,339,379,437,519   ldiffusion.py:228,240
All arithmetic runs in libldiff_hip.so; there is no torch/CPU fallback path.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from types import SimpleNamespace

import torch

from . import _lib, configs, weights

_DTYPES = {torch.float32: _lib.F32, torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}


def _load_state_dict(lib, load_fn, handle, sd, expected_names):
    unexpected = [k for k in sd if k not in expected_names]
    if unexpected:
        raise ValueError(f"unexpected tensors in checkpoint: {unexpected[:5]}{' ...' if len(unexpected) > 5 else ''}")
    for name, t in sd.items():
        t = t.detach().to("cpu").contiguous()
        if t.dtype not in _DTYPES:
            t = t.to(torch.float32)
        shape = (C.c_int64 * t.dim())(*t.shape)
        _lib.check(load_fn(handle, name.encode(), C.c_void_p(t.data_ptr()), _DTYPES[t.dtype], shape, t.dim()))


class _Output:
    """`.sample` and `[0]`, like diffusers' BaseOutput subclasses."""

    def __init__(self, sample):
        self.sample = sample

    def __getitem__(self, i):
        return (self.sample,)[i]


def _fill_unet_cfg(cfg: dict) -> "_lib.UNetCfg":
    """ldiff_unet_cfg from a validated UNet-shaped config dict (the UNet's own, or a ControlNet's trunk view)."""
    c = _lib.UNetCfg()
    c.in_channels, c.out_channels = cfg["in_channels"], cfg["out_channels"]
    boc = cfg["block_out_channels"]
    c.n_blocks = len(boc)
    for i, v in enumerate(boc):
        c.block_out_channels[i] = v
        c.down_has_attn[i] = int(cfg["down_block_types"][i] == "CrossAttnDownBlock2D")
        c.up_has_attn[i] = int(cfg["up_block_types"][i] == "CrossAttnUpBlock2D")
    c.layers_per_block = cfg["layers_per_block"]
    c.heads = cfg["attention_head_dim"]
    c.cross_attention_dim = cfg["cross_attention_dim"]
    c.norm_num_groups = cfg["norm_num_groups"]
    c.norm_eps = cfg["norm_eps"]
    c.flip_sin_to_cos = int(cfg["flip_sin_to_cos"])
    c.freq_shift = float(cfg["freq_shift"])
    return c


def _tensor_key(t):
    """Identity of a tensor's current contents: what set_context / set_cond cache by."""
    return (t.data_ptr(), tuple(t.shape), t._version, t.dtype, t.device)


class _Handle:
    """What the handle classes share.  A subclass names its entry points (`ldiff_<_prefix>_*`) and the noun its messages use, creates `self._h` and
    overrides `_param_shapes` / `_after_load`."""
    _prefix = None
    _noun = None

    def _fn(self, name):
        return getattr(self._lib, f"ldiff_{self._prefix}_{name}")

    def _param_shapes(self):
        """Names (and shapes) of the tensors a checkpoint may carry."""
        return self._shapes

    def _after_load(self, sd):
        """What the class keeps or forgets once `sd` is on the device."""

    def load_state_dict(self, sd, strict=True):
        _load_state_dict(self._lib, self._fn("load"), self._h, sd, self._param_shapes())
        n = self._fn("missing")(self._h)
        if n and strict:
            names = [self._fn("missing_name")(self._h, i).decode() for i in range(min(n, 5))]
            raise RuntimeError(f"{n} {self._noun} tensors missing from the checkpoint, e.g. {names}")
        self._after_load(sd)

    def check_finite(self):
        """Synchronises the current stream (the VAE: and its decode side stream) and raises NonFiniteError if work enqueued so far on this handle
        produced a non-finite activation (fp16 overflow -- e.g. a decoder fed z / 0.18215 of un-scaled latents; include/ldiff.h "Non-finite detection")."""
        _lib.check(self._fn("check_finite")(self._h, _lib.stream_ptr()))
        return self

    def eval(self):
        return self

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._fn("destroy")(self._h)
                self._h = None
        except Exception:
            pass


class _GraphHandle(_Handle):
    """A handle whose forward goes through the hipGraph replay cache (include/ldiff.h ldiff_*_set_graph)."""

    def set_graph(self, on: bool):
        """hipGraph replay of the forward's launch sequence (default on)."""
        _lib.check(self._fn("set_graph")(self._h, int(bool(on))))
        return self

    @property
    def graph_replays(self) -> int:
        return int(self._fn("graph_replays")(self._h))


class UNet2DConditionModel(_GraphHandle):
    _prefix, _noun = "unet", "UNet"

    def __init__(self, cfg: dict, state_dict, device=None):
        _lib.require_gpu()
        cfg = configs.with_defaults(cfg, configs.UNET_DEFAULTS)   # fields a config.json may omit get diffusers' defaults
        configs.validate_unet_config(cfg)
        self._cfg = dict(cfg)
        self.config = SimpleNamespace(**cfg)
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.dtype = torch.float32
        self._lib = _lib.load()
        c = _fill_unet_cfg(cfg)
        self._controlnet = None
        self._h = C.c_void_p()
        _lib.check(self._lib.ldiff_unet_create(C.byref(self._h), C.byref(c), self.device.index or 0))
        self._host_sd = None
        self._ctx_key = None
        self.plan_batch = 0
        self.load_state_dict(state_dict)

    def set_precision(self, mode: int):
        """Storage policy of the graph (include/ldiff.h ldiff_unet_set_precision): 0 all-fp16, 1 split residual stream (default),
        2 every contraction operand split."""
        _lib.check(self._lib.ldiff_unet_set_precision(self._h, int(mode)))
        return self

    def set_plan_batch(self, n: int):
        """Batch-invariant mode (include/ldiff.h ldiff_unet_set_plan_batch): with n >= 1 every launch is planned as if the batch were n, so an image gets
        bit-identical outputs in any batch B <= n (B > n raises ValueError); 0 (default) plans every launch from its own batch.  An attached ControlNet
        needs the same n.  Kept in `plan_batch`; returns self."""
        _lib.check(self._lib.ldiff_unet_set_plan_batch(self._h, int(n)))
        self.plan_batch = int(n)
        self._ctx_key = None   # the context's K / V are planned too: projected again by the next call
        return self

    @property
    def graph_nodes(self) -> int:
        """Kernel launches of the currently captured forward (0 before the first capture)."""
        return int(self._lib.ldiff_unet_graph_nodes(self._h))

    # ---- checkpoint surface ----
    def _param_shapes(self):
        return weights.unet_param_shapes(self._cfg)

    def _after_load(self, sd):
        self._host_sd = {k: v.detach().to("cpu") for k, v in sd.items()}
        self._ctx_key = None

    @classmethod
    def from_pretrained(cls, path, subfolder=None, device=None, **_ignored):
        if subfolder:
            path = os.path.join(path, subfolder)
        cfg, sd = weights.load_model_dir(path)
        return cls(cfg, sd, device=device)

    def save_pretrained(self, path):
        weights.save_model_dir(path, self._cfg, self._host_sd)

    def state_dict(self):
        return dict(self._host_sd)

    def parameters(self):
        return iter(self._host_sd.values())

    def to(self, *args, **kwargs):
        dt = kwargs.get("dtype", None)
        for a in args:
            if isinstance(a, torch.dtype):
                dt = a
        if dt not in (None, torch.float32):
            raise ValueError("the HIP UNet keeps the reference's float32 boundary (fp16 storage is internal)")
        return self

    # ---- forward ----
    def set_context(self, encoder_hidden_states: torch.Tensor):
        ehs = encoder_hidden_states
        if ehs.dim() != 3 or ehs.shape[-1] != self._cfg["cross_attention_dim"]:
            raise ValueError(f"encoder_hidden_states must be [B, L, {self._cfg['cross_attention_dim']}], got {tuple(ehs.shape)}")
        key = _tensor_key(ehs)
        if key == self._ctx_key:
            return
        e = ehs.detach().to(self.device, dtype=torch.float32).contiguous()
        _lib.check(self._lib.ldiff_unet_set_context(self._h, _lib.ptr(e), e.shape[0], e.shape[1], _lib.stream_ptr()))
        self._ctx_key = key
        self._ctx_keepalive = (e, ehs)  # holding the source keeps its storage (and thus the cache key) from being recycled

    # ---- ControlNet ----
    def attach_controlnet(self, controlnet: "ControlNetModel", conditioning_scale: float = 1.0):
        """Run `controlnet` inside this UNet's forward (include/ldiff.h ldiff_unet_attach_controlnet): `unet(x, t, ctx, controlnet_cond=c)` then
        equals `unet(x, t, ctx, *controlnet(x, t, ctx, c, conditioning_scale))` in one call, without the thirteen fp32 tensors in between."""
        if not isinstance(controlnet, ControlNetModel):
            raise TypeError("attach_controlnet takes a ldiffusion_amd.models.ControlNetModel")
        _lib.check(self._lib.ldiff_unet_attach_controlnet(self._h, controlnet._h, float(conditioning_scale)))
        self._controlnet = controlnet   # (also keeps the borrowed handle alive)
        return self

    def detach_controlnet(self):
        _lib.check(self._lib.ldiff_unet_attach_controlnet(self._h, None, 1.0))
        self._controlnet = None
        return self

    def __call__(self, sample, timestep, encoder_hidden_states, *args, **kwargs):
        down_res, mid_res = kwargs.get("down_block_additional_residuals"), kwargs.get("mid_block_additional_residual")
        cond = kwargs.get("controlnet_cond")
        if cond is not None and self._controlnet is None:
            raise ValueError("controlnet_cond= needs an attached ControlNet (attach_controlnet)")
        if self._controlnet is not None:
            if cond is None:
                raise ValueError("a ControlNet is attached: pass controlnet_cond= (or detach_controlnet())")
            if down_res is not None or mid_res is not None:
                raise ValueError("additional residuals cannot be combined with an attached ControlNet")
            self._controlnet.set_context(encoder_hidden_states)
            self._controlnet.set_cond(cond)
        if sample.dim() != 4 or sample.shape[1] != self._cfg["in_channels"]:
            raise ValueError(f"sample must be [B, {self._cfg['in_channels']}, h, w], got {tuple(sample.shape)}")
        B = sample.shape[0]
        if encoder_hidden_states.shape[0] not in (1, B):
            raise ValueError(f"encoder_hidden_states batch {encoder_hidden_states.shape[0]} does not match sample batch {B}")
        self.set_context(encoder_hidden_states)
        x = sample.detach().to(self.device, dtype=torch.float32).contiguous()
        out = torch.empty((B, self._cfg["out_channels"], x.shape[2], x.shape[3]), device=self.device, dtype=torch.float32)
        if down_res is not None or mid_res is not None:   # ControlNet inputs (segmentor.py:357-375): added to the skips / the mid output
            keep = [t.detach().to(self.device, dtype=torch.float32).contiguous() for t in (down_res or [])]
            shapes = self._skip_shapes(B, x.shape[2], x.shape[3])
            if keep and [tuple(t.shape) for t in keep] != shapes:
                raise ValueError(f"down_block_additional_residuals must have the shapes of the skip tensors {shapes}")
            mid = mid_res.detach().to(self.device, dtype=torch.float32).contiguous() if mid_res is not None else None
            if mid is not None and tuple(mid.shape) != shapes[-1]:
                raise ValueError(f"mid_block_additional_residual must be {shapes[-1]}")
            arr = (C.c_void_p * max(len(keep), 1))(*[t.data_ptr() for t in keep])
            _lib.check(self._lib.ldiff_unet_set_additional_residuals(self._h, arr, len(keep), _lib.ptr(mid)))
            self._residual_keepalive = (keep, mid)
        _lib.check(self._lib.ldiff_unet_forward(self._h, _lib.ptr(x), B, x.shape[2], x.shape[3], float(timestep), _lib.ptr(out), _lib.stream_ptr()))
        return _Output(out)

    forward = __call__

    def _skip_shapes(self, B, h, w):
        """Shapes of the skip tensors in stack order (conv_in, then every resnet/attention output and downsampler of the down path)."""
        boc, lpb = self._cfg["block_out_channels"], self._cfg["layers_per_block"]
        shapes = [(B, boc[0], h, w)]
        for i, c in enumerate(boc):
            shapes += [(B, c, h, w)] * lpb
            if i != len(boc) - 1:
                h, w = h // 2, w // 2
                shapes.append((B, c, h, w))
        return shapes


class ControlNetOutput:
    """`.down_block_res_samples` / `.mid_block_res_sample`, like diffusers' ControlNetOutput."""

    def __init__(self, down, mid):
        self.down_block_res_samples = down
        self.mid_block_res_sample = mid

    def __getitem__(self, i):
        return (self.down_block_res_samples, self.mid_block_res_sample)[i]


class ControlNetModel(_Handle):
    """diffusers' ControlNetModel for SD-v1.5-style configs on the HIP library (include/ldiff.h ldiff_controlnet_*): what
    `Segmentor.ldiffusion_augment_for_multimodal` calls at /root/reference/segmentor.py:357-363."""
    _prefix, _noun = "controlnet", "ControlNet"

    def __init__(self, cfg: dict, state_dict, device=None):
        _lib.require_gpu()
        cfg = configs.with_defaults(cfg, configs.CONTROLNET_DEFAULTS)
        configs.validate_controlnet_config(cfg)
        self._cfg = dict(cfg)
        self._trunk_cfg = configs.controlnet_trunk_config(cfg)
        self.config = SimpleNamespace(**cfg)
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.dtype = torch.float32
        self._lib = _lib.load()
        c = _fill_unet_cfg(self._trunk_cfg)
        emb = list(cfg["conditioning_embedding_out_channels"])
        self._h = C.c_void_p()
        _lib.check(self._lib.ldiff_controlnet_create(C.byref(self._h), C.byref(c), cfg["conditioning_channels"], (C.c_int * len(emb))(*emb), len(emb),
                                                     self.device.index or 0))
        self._host_sd = None
        self._ctx_key = None
        self._cond_key = None
        self.plan_batch = 0
        self.load_state_dict(state_dict)

    def set_precision(self, mode: int):
        _lib.check(self._lib.ldiff_controlnet_set_precision(self._h, int(mode)))
        self._cond_key = None   # (the embedding's first layer follows the storage policy)
        return self

    def set_plan_batch(self, n: int):
        """As UNet2DConditionModel.set_plan_batch (include/ldiff.h ldiff_controlnet_set_plan_batch): trunk, zero convs and conditioning embedding."""
        _lib.check(self._lib.ldiff_controlnet_set_plan_batch(self._h, int(n)))
        self.plan_batch = int(n)
        self._ctx_key = None    # both are planned too: computed again by the next call
        self._cond_key = None
        return self

    def _param_shapes(self):
        return weights.controlnet_param_shapes(self._cfg)

    def _after_load(self, sd):
        self._host_sd = {k: v.detach().to("cpu") for k, v in sd.items()}
        self._ctx_key = None
        self._cond_key = None

    @classmethod
    def from_pretrained(cls, path, subfolder=None, device=None, **_ignored):
        if subfolder:
            path = os.path.join(path, subfolder)
        cfg, sd = weights.load_model_dir(path)
        return cls(cfg, sd, device=device)

    def save_pretrained(self, path):
        weights.save_model_dir(path, self._cfg, self._host_sd)

    def state_dict(self):
        return dict(self._host_sd)

    def parameters(self):
        return iter(self._host_sd.values())

    def to(self, *args, **kwargs):
        dt = kwargs.get("dtype", None)
        for a in args:
            if isinstance(a, torch.dtype):
                dt = a
        if dt not in (None, torch.float32):
            raise ValueError("the HIP ControlNet keeps the reference's float32 boundary (fp16 storage is internal)")
        return self

    def set_context(self, encoder_hidden_states: torch.Tensor):
        ehs = encoder_hidden_states
        if ehs.dim() != 3 or ehs.shape[-1] != self._cfg["cross_attention_dim"]:
            raise ValueError(f"encoder_hidden_states must be [B, L, {self._cfg['cross_attention_dim']}], got {tuple(ehs.shape)}")
        key = _tensor_key(ehs)
        if key == self._ctx_key:
            return
        e = ehs.detach().to(self.device, dtype=torch.float32).contiguous()
        _lib.check(self._lib.ldiff_controlnet_set_context(self._h, _lib.ptr(e), e.shape[0], e.shape[1], _lib.stream_ptr()))
        self._ctx_key = key
        self._ctx_keepalive = (e, ehs)

    def set_cond(self, controlnet_cond: torch.Tensor):
        """Runs the conditioning embedding (once per image: cached by the identity key `set_context` uses)."""
        c = controlnet_cond
        if c.dim() != 4 or c.shape[1] != self._cfg["conditioning_channels"]:
            raise ValueError(f"controlnet_cond must be [B, {self._cfg['conditioning_channels']}, H, W], got {tuple(c.shape)}")
        key = _tensor_key(c)
        if key == self._cond_key:
            return
        x = c.detach().to(self.device, dtype=torch.float32).contiguous()
        _lib.check(self._lib.ldiff_controlnet_set_cond(self._h, _lib.ptr(x), x.shape[0], x.shape[2], x.shape[3], _lib.stream_ptr()))
        self._cond_key = key
        self._cond_keepalive = (x, c)

    def _skip_shapes(self, B, h, w):
        return UNet2DConditionModel._skip_shapes(self, B, h, w)

    def __call__(self, sample, timestep, encoder_hidden_states, controlnet_cond, conditioning_scale=1.0, guess_mode=False, return_dict=True, **unsupported):
        if guess_mode:
            raise ValueError("guess_mode=True is not supported")
        extra = [k for k, v in unsupported.items() if v is not None]
        if extra:
            raise ValueError(f"unsupported ControlNet arguments: {extra}")
        if sample.dim() != 4 or sample.shape[1] != self._cfg["in_channels"]:
            raise ValueError(f"sample must be [B, {self._cfg['in_channels']}, h, w], got {tuple(sample.shape)}")
        B = sample.shape[0]
        if encoder_hidden_states.shape[0] not in (1, B):
            raise ValueError(f"encoder_hidden_states batch {encoder_hidden_states.shape[0]} does not match sample batch {B}")
        if controlnet_cond.shape[0] not in (1, B):
            raise ValueError(f"controlnet_cond batch {controlnet_cond.shape[0]} does not match sample batch {B}")
        self.set_context(encoder_hidden_states)
        self.set_cond(controlnet_cond)
        x = sample.detach().to(self.device, dtype=torch.float32).contiguous()
        shapes = self._skip_shapes(B, x.shape[2], x.shape[3])
        down = [torch.empty(s, device=self.device, dtype=torch.float32) for s in shapes]
        mid = torch.empty(shapes[-1], device=self.device, dtype=torch.float32)
        arr = (C.c_void_p * len(down))(*[t.data_ptr() for t in down])
        _lib.check(self._lib.ldiff_controlnet_forward(self._h, _lib.ptr(x), B, x.shape[2], x.shape[3], float(timestep), float(conditioning_scale), arr, len(down),
                                                      _lib.ptr(mid), _lib.stream_ptr()))
        return ControlNetOutput(down, mid) if return_dict else (down, mid)

    forward = __call__


class _LatentDist:
    """DiagonalGaussianDistribution surface: `.mean`, `.sample()` (segmentor.py:99,339)."""

    def __init__(self, moments):
        self.mean, logvar = torch.chunk(moments, 2, dim=1)
        self.logvar = torch.clamp(logvar, -30.0, 20.0)
        self.std = torch.exp(0.5 * self.logvar)

    def sample(self, generator=None):
        noise = torch.randn(self.mean.shape, generator=generator, device=self.mean.device, dtype=self.mean.dtype)
        return self.mean + self.std * noise

    def mode(self):
        return self.mean


class AutoencoderKL(_Handle):
    _prefix, _noun = "vae", "VAE"

    def __init__(self, cfg: dict, state_dict, device=None, range_shift: int = 0):
        _lib.require_gpu()
        cfg = configs.with_defaults(cfg, configs.VAE_DEFAULTS)    # e.g. `scaling_factor` (decode_latents reads vae.config.scaling_factor)
        configs.validate_vae_config(cfg)
        self._cfg = dict(cfg)
        self.config = SimpleNamespace(**cfg)
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.dtype = torch.float32
        self._lib = _lib.load()
        c = _lib.VaeCfg()
        c.in_channels, c.out_channels, c.latent_channels = cfg["in_channels"], cfg["out_channels"], cfg["latent_channels"]
        boc = cfg["block_out_channels"]
        c.n_blocks = len(boc)
        for i, v in enumerate(boc):
            c.block_out_channels[i] = v
        c.layers_per_block = cfg["layers_per_block"]
        c.norm_num_groups = cfg["norm_num_groups"]
        c.scaling_factor = cfg["scaling_factor"]
        self._h = C.c_void_p()
        _lib.check(self._lib.ldiff_vae_create(C.byref(self._h), C.byref(c), self.device.index or 0))
        self.load_state_dict(state_dict)
        self.range_shift = 0
        self.plan_batch = 0
        if range_shift:
            self.set_range_shift(range_shift)

    @classmethod
    def from_pretrained(cls, path, subfolder=None, device=None, range_shift: int = 0, **_ignored):
        if subfolder:
            path = os.path.join(path, subfolder)
        cfg, sd = weights.load_model_dir(path)
        return cls(cfg, sd, device=device, range_shift=range_shift)

    def load_state_dict(self, sd, strict=True):
        super().load_state_dict(weights.normalize_vae_keys(sd), strict)

    def _param_shapes(self):
        return weights.vae_param_shapes(self._cfg)

    def _after_load(self, sd):
        self._host_sd = {k: v.detach().to("cpu") for k, v in sd.items()}

    def save_pretrained(self, path):
        weights.save_model_dir(path, self._cfg, self._host_sd)

    def set_precision(self, encoder: int = 2, decoder: int = 0):
        """Storage policy of the encoder / decoder graphs (include/ldiff.h ldiff_vae_set_precision).  The current pair is kept in
        `precision` so that a caller that changes it for one call can put back what was there."""
        _lib.check(self._lib.ldiff_vae_set_precision(self._h, int(encoder), int(decoder)))
        self.precision = (int(encoder), int(decoder))
        return self

    def set_range_shift(self, k: int):
        """Decoder range shift (include/ldiff.h ldiff_vae_set_range_shift): the decoder stores its activations times 2^-k, for checkpoints whose decoder
        activations pass fp16's +-65504.  0 <= k <= 16 (else ValueError); the encoder is unaffected.  Kept in `range_shift`; returns self."""
        _lib.check(self._lib.ldiff_vae_set_range_shift(self._h, int(k)))
        self.range_shift = int(k)
        return self

    def set_plan_batch(self, n: int):
        """Batch-invariant mode of the encoder and the decoder (include/ldiff.h ldiff_vae_set_plan_batch): with n >= 1 an image's moments, sample and
        uint8 image are bit-identical in any batch B <= n (B > n raises ValueError); 0 (default) = off.  Kept in `plan_batch`; returns self."""
        _lib.check(self._lib.ldiff_vae_set_plan_batch(self._h, int(n)))
        self.plan_batch = int(n)
        return self

    def fit_range_shift(self, z, z_scale=None, step: int = 2, k_max: int = 16):
        """Decodes `z` (times z_scale, default 1 / scaling_factor as decode_latents) at k = 0, step, 2 step, ... until check_finite passes, leaves that k
        set and returns it.  If k_max (0..16) still overflows, the range shift is put back as it was and NonFiniteError is raised."""
        if step < 1 or not 0 <= k_max <= 16:
            raise ValueError(f"fit_range_shift: step must be >= 1 and k_max in 0..16 (got step={step}, k_max={k_max})")
        z_scale = 1.0 / self.config.scaling_factor if z_scale is None else z_scale
        self.check_finite()   # (earlier work must not be blamed on the first candidate)
        prev = self.range_shift
        ks = list(range(0, k_max + 1, step))
        if ks[-1] != k_max:
            ks.append(k_max)
        for i, k in enumerate(ks):
            self.set_range_shift(k)
            self._decode(z, z_scale, want_image=True)
            try:
                self.check_finite()
                return k
            except _lib.NonFiniteError:
                if i == len(ks) - 1:
                    self.set_range_shift(prev)
                    raise

    def to(self, *args, **kwargs):
        return self

    @property
    def scale_factor(self):
        return 2 ** (len(self._cfg["block_out_channels"]) - 1)

    def encode(self, x):
        if x.dim() != 4 or x.shape[1] != self._cfg["in_channels"]:
            raise ValueError(f"image batch must be [B, {self._cfg['in_channels']}, H, W], got {tuple(x.shape)}")
        x = x.detach().to(self.device, dtype=torch.float32).contiguous()
        B, _, H, W = x.shape
        f = self.scale_factor
        mom = torch.empty((B, 2 * self._cfg["latent_channels"], H // f, W // f), device=self.device, dtype=torch.float32)
        _lib.check(self._lib.ldiff_vae_encode(self._h, _lib.ptr(x), B, H, W, _lib.ptr(mom), _lib.stream_ptr()))
        return SimpleNamespace(latent_dist=_LatentDist(mom))

    def _decode(self, z, z_scale, want_sample=False, want_image=False, want_rgb=False, luma=None, slot=0):
        if z.dim() != 4 or z.shape[1] != self._cfg["latent_channels"]:
            raise ValueError(f"latents must be [B, {self._cfg['latent_channels']}, h, w], got {tuple(z.shape)}")
        z = z.detach().to(self.device, dtype=torch.float32).contiguous()
        B, _, h, w = z.shape
        f = self.scale_factor
        H, W = h * f, w * f
        sample = torch.empty((B, self._cfg["out_channels"], H, W), device=self.device, dtype=torch.float32) if want_sample else None
        image = torch.empty((B, H, W, 3), device=self.device, dtype=torch.float32) if want_image else None
        rgb = torch.empty((B, H, W, 3), device=self.device, dtype=torch.uint8) if want_rgb else None
        n_slots = luma.shape[1] if luma is not None else 0
        _lib.check(self._lib.ldiff_vae_decode(self._h, _lib.ptr(z), B, h, w, float(z_scale), _lib.ptr(sample), _lib.ptr(image), _lib.ptr(rgb),
                                              _lib.ptr(luma), n_slots, slot, _lib.stream_ptr()))
        return sample, image, rgb

    def decode(self, z):
        sample, _, _ = self._decode(z, 1.0, want_sample=True)
        return SimpleNamespace(sample=sample)


class PlainConvUNet(_GraphHandle):
    """nnU-Net v2's 2-D PlainConvUNet on the HIP library (include/ldiff.h ldiff_segnet_*): the network nnUNetPredictor runs inside its sliding
    window at /root/reference/segmentor.py:463-488.  `spec` comes from `nnunet.network_spec`; `state_dict` carries the canonical names
    (`nnunet.clean_state_dict` drops a checkpoint's aliases).  `net(x [B, C, h, w] float32 on the device) -> logits [B, heads, h, w]` in
    `out_dtype` (float32 default; float16 is what the reference's autocast hands the sliding window)."""
    _prefix, _noun = "segnet", "nnU-Net"

    def __init__(self, spec: dict, state_dict, device=None, out_dtype=torch.float32):
        from . import nnunet
        _lib.require_gpu()
        self.spec = dict(spec)
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.out_dtype = out_dtype
        self._lib = _lib.load()
        n = spec["n_stages"]
        arr = lambda v: (C.c_int * len(v))(*[int(i) for i in v])
        self._h = C.c_void_p()
        _lib.check(self._lib.ldiff_segnet_create(C.byref(self._h), spec["in_channels"], n, arr(spec["features"]), arr(spec["strides"]),
                                                 arr(spec["n_conv_encoder"]), arr(spec["n_conv_decoder"]), spec["n_heads"], self.device.index or 0))
        self._shapes = nnunet.param_shapes(spec)
        self.load_state_dict(state_dict)

    def _after_load(self, sd):
        self._host_sd = {k: v.detach().to("cpu") for k, v in sd.items()}

    def state_dict(self):
        return dict(self._host_sd)

    def to(self, *args, **kwargs):
        return self

    @torch.no_grad()
    def __call__(self, x):
        if x.dim() != 4 or x.shape[1] != self.spec["in_channels"]:
            raise ValueError(f"PlainConvUNet: input must be [B, {self.spec['in_channels']}, h, w], got {list(x.shape)}")
        if self.out_dtype not in (torch.float32, torch.float16):
            raise ValueError("PlainConvUNet: out_dtype must be float32 or float16")
        x = x.to(self.device, torch.float32).contiguous()
        B, _, h, w = x.shape
        out = torch.empty((B, self.spec["n_heads"], h, w), dtype=self.out_dtype, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.ldiff_segnet_forward(self._h, _lib.ptr(x), B, h, w, _lib.ptr(out), _DTYPES[self.out_dtype], _lib.stream_ptr()))
        return out

    forward = __call__


class ResNetClassifier(_GraphHandle):
    """The cell head's instance classifier on the HIP library (include/ldiff.h ldiff_resnet_*): torchvision's ResNet trunk (ResNet152: layers
    (3, 8, 36, 3), width 64) without avgpool / fc, `adapter` conv, mean over the map, linear head -- `encoder` / `adapter` / `classifier` of
    the reference's CellSegClassifier.  `state_dict` carries the module's own names (`cellhead.param_shapes`); every BatchNorm is folded into
    its conv at load.  `net(crops [B, S, S, 8] float16 NHWC on the device, channels 3..7 zero) -> (logits [B, C] float32, labels [B] int32)`,
    labels = 1 + argmax(logits[:, 1:]).
    train=True (ldiff_resnet_set_train, chosen before the load): the handle also keeps the un-folded conv matrices and every BatchNorm's gamma / beta, and offers
    `forward_train(crops) -> (features [B, A] float32, batch_mean [T] float32, batch_var [T] float32)` -- the trunk with batch statistics over all B crops, as
    torch's modules compute in `.train()`; batch_var is the UNBIASED variance, T the channels of all BatchNorms -- and `bn_layout`, the list of (checkpoint
    prefix, offset on that axis, channels) in forward order.  The eval-mode call is unchanged bit for bit.  Running statistics are never touched here: see
    `cellhead.ema_update`."""
    _prefix, _noun = "resnet", "classifier"

    def __init__(self, num_classes: int, state_dict, device=None, layers=(3, 8, 36, 3), width=64, adapter_channels=256, train=False):
        from . import cellhead
        _lib.require_gpu()
        self.num_classes, self.layers, self.width, self.adapter_channels = int(num_classes), tuple(int(v) for v in layers), int(width), int(adapter_channels)
        if len(self.layers) != 4:
            raise ValueError(f"ResNetClassifier: layers must have 4 entries, got {layers}")
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self._lib = _lib.load()
        self._h = C.c_void_p()
        _lib.check(self._lib.ldiff_resnet_create(C.byref(self._h), (C.c_int * 4)(*self.layers), self.width, self.adapter_channels, self.num_classes,
                                                 self.device.index or 0))
        self._shapes = cellhead.param_shapes(self.num_classes, self.layers, self.width, self.adapter_channels, counters=True)
        self.train_mode = bool(train)
        if self.train_mode:
            self.set_train(True)
        self.bn_channels = int(self._lib.ldiff_resnet_bn_channels(self._h))
        self.bn_layout = []
        name, off, ch = C.c_char_p(), C.c_int64(), C.c_int()
        i = 0
        while self._lib.ldiff_resnet_bn_entry(self._h, i, C.byref(name), C.byref(off), C.byref(ch)) == 0:
            self.bn_layout.append((name.value.decode(), int(off.value), int(ch.value)))
            i += 1
        self.load_state_dict(state_dict)

    def set_train(self, on: bool):
        """ldiff_resnet_set_train: only before the tensors are loaded (RuntimeError afterwards: the fold consumes the host tensors)."""
        _lib.check(self._lib.ldiff_resnet_set_train(self._h, int(bool(on))))
        self.train_mode = bool(on)
        return self

    def to(self, *args, **kwargs):
        return self

    @torch.no_grad()
    def forward_train(self, crops, want_logits=False):
        """One training-mode pass over all B crops (ldiff_resnet_forward_train): (features [B, A] f32, batch_mean [T] f32, batch_var [T] f32 unbiased);
        want_logits=True appends (logits [B, C] f32, labels [B] i32) of the current linear head."""
        if crops.dim() != 4 or crops.shape[1] != crops.shape[2] or crops.shape[3] != 8 or crops.dtype != torch.float16:
            raise ValueError(f"ResNetClassifier: crops must be float16 [B, S, S, 8] (NHWC, channels 3..7 zero), got {crops.dtype} {list(crops.shape)}")
        crops = crops.to(self.device).contiguous()
        B, S = crops.shape[0], crops.shape[1]
        stats = torch.empty((2, self.bn_channels), dtype=torch.float32, device=self.device)
        feats = torch.empty((B, self.adapter_channels), dtype=torch.float32, device=self.device)
        logits = torch.empty((B, self.num_classes), dtype=torch.float32, device=self.device) if want_logits else None
        labels = torch.empty((B,), dtype=torch.int32, device=self.device) if want_logits else None
        with torch.cuda.device(self.device):
            _lib.check(self._lib.ldiff_resnet_forward_train(self._h, _lib.ptr(crops), B, S, _lib.ptr(stats), _lib.ptr(feats), _lib.ptr(logits), _lib.ptr(labels),
                                                            _lib.stream_ptr()))
        return (feats, stats[0], stats[1]) + ((logits, labels) if want_logits else ())

    @torch.no_grad()
    def __call__(self, crops):
        if crops.dim() != 4 or crops.shape[1] != crops.shape[2] or crops.shape[3] != 8 or crops.dtype != torch.float16:
            raise ValueError(f"ResNetClassifier: crops must be float16 [B, S, S, 8] (NHWC, channels 3..7 zero), got {crops.dtype} {list(crops.shape)}")
        crops = crops.to(self.device).contiguous()
        B, S = crops.shape[0], crops.shape[1]
        logits = torch.empty((B, self.num_classes), dtype=torch.float32, device=self.device)
        labels = torch.empty((B,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.ldiff_resnet_forward(self._h, _lib.ptr(crops), B, S, _lib.ptr(logits), _lib.ptr(labels), _lib.stream_ptr()))
        return logits, labels

    forward = __call__


class CLIPTextModel(_GraphHandle):
    """transformers' CLIPTextModel on the HIP library (include/ldiff.h ldiff_textenc_*): `pipeline.text_encoder` of the reference's prompt path
    (/root/reference/segmentor.py:55-60,348-350, pixel_latent_vector.py:65-67, utils.py:193-195, ldiffusion.py:213-216).  `cfg` is
    text_encoder/config.json, `state_dict` carries transformers' own keys (with or without the `text_model.` prefix: `weights.clip_text_loader_name`).  `enc(input_ids)["last_hidden_state"]` is float32 [B, L, hidden] on the
    device; with a projection loaded (`load_projection`), `enc.project(input_ids)` returns `proj(last_hidden_state)` from the same library call.
    No pooled output, no attention_mask (the reference passes none)."""
    _prefix, _noun = "textenc", "text encoder"

    def __init__(self, cfg: dict, state_dict, device=None):
        c = weights.clip_text_config(cfg)   # refusals happen here, before the library is touched
        _lib.require_gpu()
        self.config = SimpleNamespace(**{**cfg, **c})
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self._lib = _lib.load()
        tc = _lib.TextEncCfg(int(c["vocab_size"]), int(c["hidden_size"]), int(c["intermediate_size"]), int(c["num_hidden_layers"]), int(c["num_attention_heads"]),
                             int(c["max_position_embeddings"]), weights.CLIP_TEXT_ACTS[c["hidden_act"]], float(c["layer_norm_eps"]))
        self._h = C.c_void_p()
        _lib.check(self._lib.ldiff_textenc_create(C.byref(self._h), C.byref(tc), self.device.index or 0))
        self._shapes = weights.clip_text_param_shapes(c)
        self.projection_dim = None
        self.load_state_dict(weights.normalize_clip_text_keys(state_dict))

    @classmethod
    def from_pretrained(cls, path, device=None, **_ignored):
        cfg, sd = weights.load_model_dir(path)
        return cls(cfg, sd, device=device)

    def load_projection(self, state_dict):
        """`nn.Linear(hidden, cross_attention_dim).load_state_dict(proj_weights.pt, strict=True)` of the reference (segmentor.py:45-48): exactly
        `weight` and `bias`; anything else is refused by key, as torch refuses it."""
        keys = set(state_dict)
        if keys != {"weight", "bias"}:
            raise RuntimeError(f"Error(s) in loading state_dict for the text projection: unexpected {sorted(keys - {'weight', 'bias'})}, missing {sorted({'weight', 'bias'} - keys)}")
        w, b = state_dict["weight"], state_dict["bias"]
        if w.dim() != 2 or w.shape[1] != self.config.hidden_size or tuple(b.shape) != (w.shape[0],):
            raise RuntimeError(f"text projection: weight {list(w.shape)} / bias {list(b.shape)} do not fit hidden_size = {self.config.hidden_size}")
        if self.projection_dim not in (None, w.shape[0]):
            raise RuntimeError(f"text projection: this encoder already holds a projection to {self.projection_dim} channels")
        self._shapes = weights.clip_text_param_shapes(vars(self.config), w.shape[0])
        self.load_state_dict({"proj.weight": w, "proj.bias": b})
        self.projection_dim = int(w.shape[0])
        return self

    @property
    def graph_nodes(self) -> int:
        """Kernel launches of the currently captured forward (0: none captured yet)."""
        return int(self._lib.ldiff_textenc_graph_nodes(self._h))

    def to(self, *args, **kwargs):
        return self

    def _run(self, input_ids, project, out_dtype):
        if out_dtype not in (torch.float32, torch.float16):
            raise ValueError("CLIPTextModel: out_dtype must be float32 or float16")
        ids = torch.as_tensor(input_ids)
        if ids.dim() != 2 or ids.is_floating_point():
            raise ValueError(f"CLIPTextModel: input_ids must be an integer tensor [B, L], got {ids.dtype} {list(ids.shape)}")
        if project and self.projection_dim is None:
            raise RuntimeError("CLIPTextModel: no projection loaded (load_projection)")
        ids = ids.detach().to("cpu", torch.int32).contiguous()   # the tokenizer's output is host data; the library validates and stages it
        B, L = ids.shape
        out = torch.empty((B, L, self.projection_dim if project else self.config.hidden_size), dtype=out_dtype, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.ldiff_textenc_forward(self._h, C.cast(ids.data_ptr(), C.POINTER(C.c_int32)), B, L, int(bool(project)), _lib.ptr(out), _DTYPES[out_dtype],
                                                       _lib.stream_ptr()))
        return out

    @torch.no_grad()
    def __call__(self, input_ids, attention_mask=None, out_dtype=torch.float32, **unsupported):
        if attention_mask is not None:
            raise ValueError("CLIPTextModel: attention_mask is not supported (the reference never passes one; pass attention_mask=None)")
        if unsupported:
            raise ValueError(f"CLIPTextModel: unsupported arguments {sorted(unsupported)}")
        return {"last_hidden_state": self._run(input_ids, False, out_dtype)}

    forward = __call__

    @torch.no_grad()
    def project(self, input_ids, out_dtype=torch.float32):
        """`proj(text_encoder(input_ids)["last_hidden_state"])` in one library call: [B, L, cross_attention_dim], ready for `unet.set_context`."""
        return self._run(input_ids, True, out_dtype)
