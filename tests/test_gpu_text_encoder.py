"""-m gpu: the CLIP text encoder on the HIP library (csrc/kernels_text.hip, csrc/model_text.hip, models.CLIPTextModel) against `transformers`
run in fp32 on the CPU, and its attention kernel against a float64 causal softmax with the per-element bound of tests/attention_bound.py.

Bound of the whole encoder (test_encoder_matches_transformers_fp32).  It cannot be derived on paper through 2-3 layers of LayerNorm; the rule is: measure
the worst max |hip - ref| / max |ref| over the 18 (config, B, L) cases below (fp32 output, fp32 `transformers` on the CPU as the reference) and assert at twice
the measured value rounded up to one digit, never above the project's parity figure 1e-3 (CAP).
Measured on an MI355X (each case prints its figures, [textenc-err] lines): `last_hidden_state` 2.0e-4 .. 3.67e-4 (worst: hidden 64 / quick_gelu, B = 3, L = 5;
CLIP-L width 2.0e-4 .. 3.64e-4), projection 2.3e-4 .. 3.72e-4 (worst: hidden 128 / gelu, B = 3, L = 77).  Worst of all: 3.72e-4, twice that 7.4e-4, so
TOL = 8e-4.  An fp16 output adds its one rounding, 2^-11 of the value, on top (measured 2.9e-4 .. 4.96e-4).
The yardstick, `CLIPTextModel.half()` run by torch on the same GPU on the same ids against the same reference: 8.9e-4 .. 1.73e-3 over the 18 cases, 2.8 to 5.1
times the library's error in every case -- the split residual stream and split GEMM operands are not worse than it, they are better.  (With single fp16 GEMM
operands the library had measured 8.3e-4 / 1.08e-3 on hidden 128 / gelu, B = 1, L = 5: the yardstick's own level, and over the cap.)"""
import ctypes as C
import json
import math
import os

import pytest
import torch

import attention_bound as ab
from ldiffusion_amd import _lib, configs, models, weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP = 1e-3
TOL = 8e-4          # twice the measured worst case 3.72e-4, rounded up to one digit (module docstring); never above CAP
H16 = 2.0 ** -11
SENTINEL = -30000.0


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------------
ATTN_CASES = [(1, 1, 1, 16), (2, 4, 5, 16), (1, 1, 33, 32), (1, 2, 16, 64), (1, 2, 17, 64), (3, 12, 77, 64), (1, 1, 128, 128)]
KERNEL = "xattn<short-kv>"   # the contract text_attn<d> shares: one key tile (T = 1), p rounded once to nearest, the row sum from the unrounded p in fp32


def _run_attn(lib, qkv, B, heads, L, d, spare=4):
    """qkv [B L, 3 hidden] f16 on the device -> (o [B L, hidden], the `spare` canary rows behind it)."""
    hidden = heads * d
    out = torch.full((B * L + spare, hidden), SENTINEL, dtype=torch.float16, device=DEV)
    _lib.check(lib.ldiff_op_text_attention(_lib.ptr(qkv), 3 * hidden, hidden, _lib.ptr(out), hidden, B, heads, L, d, 1.0 / math.sqrt(d), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return out[:B * L], out[B * L:]


def _fused(q, k, v):
    """[B, heads, L, d] x 3 -> the fused projection layout [B L, 3 heads d] f16."""
    B, heads, L, d = q.shape
    rows = lambda t: t.permute(0, 2, 1, 3).reshape(B * L, heads * d)
    return torch.cat([rows(q), rows(k), rows(v)], 1).to(torch.float16).to(DEV).contiguous()


def _causal_reference(q, k, v, scale):
    """float64 causal softmax and its bound, row by row: query i against keys 0..i (q, k, v [N, L, d])."""
    outs = [ab.reference(q[:, i:i + 1], k[:, :i + 1], v[:, :i + 1], scale, KERNEL) for i in range(q.shape[1])]
    return torch.cat([o for o, _ in outs], 1), torch.cat([t for _, t in outs], 1)


@pytest.mark.parametrize("B, heads, L, d", ATTN_CASES)
@pytest.mark.parametrize("regime", ["R0", "R1"])
def test_text_attention_against_float64(lib, B, heads, L, d, regime):
    q, k, v = ab.make_operands(B, B, heads, L, L, d, regime, seed=1000 * L + d)
    o, canary = _run_attn(lib, _fused(q, k, v), B, heads, L, d)
    got = o.cpu().double().reshape(B, L, heads, d).permute(0, 2, 1, 3).reshape(B * heads, L, d)
    flat = lambda t: t.reshape(B * heads, L, d)
    ref, tol = _causal_reference(flat(q), flat(k), flat(v), 1.0 / math.sqrt(d))
    r = ab.ratio(got, ref, tol)
    print(f"[text-attn-err] B={B} heads={heads} L={L} d={d} {regime}: worst error / bound = {r:.3f}")
    assert r <= 1.0
    assert torch.all(canary == SENTINEL), "rows behind row B L of the output were written"
    if L >= 5:   # the test can see a missing mask: the unmasked softmax is outside the causal bound
        full, _ = ab.reference(flat(q), flat(k), flat(v), 1.0 / math.sqrt(d), KERNEL)
        assert ab.ratio(full, ref, tol) > 1.0


# ---- 2. causality is exact -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, heads, L, d", [(2, 4, 5, 16), (1, 2, 17, 64), (3, 12, 77, 64)])
def test_text_attention_is_exactly_causal(lib, B, heads, L, d):
    """Rewriting q, k and v at positions > i leaves the output rows <= i bit-identical, and an image's rows do not depend on its neighbours'."""
    q, k, v = ab.make_operands(B, B, heads, L, L, d, "R0", seed=7)
    base, _ = _run_attn(lib, _fused(q, k, v), B, heads, L, d)
    hidden = heads * d
    for i in sorted({0, L // 2, L - 2}):
        q2, k2, v2 = ab.make_operands(B, B, heads, L, L, d, "R1", seed=8 + i)
        for a, b_ in ((q, q2), (k, k2), (v, v2)):
            b_[:, :, :i + 1] = a[:, :, :i + 1]
        got, _ = _run_attn(lib, _fused(q2, k2, v2), B, heads, L, d)
        assert torch.equal(got.view(B, L, hidden)[:, :i + 1], base.view(B, L, hidden)[:, :i + 1]), i
        assert not torch.equal(got, base)
    if B > 1:
        q2, k2, v2 = (t.clone() for t in (q, k, v))
        for t in (q2, k2, v2):
            t[1] = t[1].flip(1)
        got, _ = _run_attn(lib, _fused(q2, k2, v2), B, heads, L, d)
        keep = [b for b in range(B) if b != 1]
        assert torch.equal(got.view(B, L, hidden)[keep], base.view(B, L, hidden)[keep]) and not torch.equal(got.view(B, L, hidden)[1], base.view(B, L, hidden)[1])


# ---- the whole encoder ----------------------------------------------------------------------------------------------------------------------
CONFIGS = {
    "h64_q": dict(vocab_size=300, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, hidden_act="quick_gelu"),
    "h128_g": dict(vocab_size=300, hidden_size=128, intermediate_size=320, num_hidden_layers=3, num_attention_heads=2, hidden_act="gelu"),
    "clipL": dict(vocab_size=1000, hidden_size=768, intermediate_size=3072, num_hidden_layers=2, num_attention_heads=12, hidden_act="quick_gelu"),
}
PROJ_DIM = {"h64_q": 64, "h128_g": 96, "clipL": 768}
_MODELS = {}


def _hf_model(name, seed=0):
    """`transformers`' CLIPTextModel of CONFIGS[name] in fp32 on the CPU: its own random init under torch.manual_seed, every LayerNorm's gamma / beta moved
    away from 1 / 0, and a projection Linear(hidden, PROJ_DIM)."""
    from transformers import CLIPTextConfig, CLIPTextModel
    c = CONFIGS[name]
    torch.manual_seed(seed)
    hf = CLIPTextModel(CLIPTextConfig(max_position_embeddings=77, bos_token_id=c["vocab_size"] - 2, eos_token_id=c["vocab_size"] - 1, pad_token_id=c["vocab_size"] - 1, **c)).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in hf.named_parameters():
            if "layer_norm" in n:
                p.add_(torch.randn(p.shape, generator=g) * (0.2 if n.endswith("weight") else 0.1))
    proj = {"weight": torch.randn((PROJ_DIM[name], c["hidden_size"]), generator=g) * c["hidden_size"] ** -0.5, "bias": torch.randn((PROJ_DIM[name],), generator=g) * 0.1}
    return hf, proj


def _pair(name):
    """(transformers model, projection, HIP model with the projection loaded), built once per config."""
    if name not in _MODELS:
        hf, proj = _hf_model(name)
        enc = models.CLIPTextModel(hf.config.to_dict(), hf.state_dict(), DEV).load_projection(proj)
        _MODELS[name] = (hf, proj, enc)
    return _MODELS[name]


def _ids(name, B, L, seed):
    return torch.randint(0, CONFIGS[name]["vocab_size"], (B, L), generator=torch.Generator().manual_seed(seed))


def _rel(got, ref):
    return ((got.float().cpu() - ref).abs().max() / ref.abs().max()).item()


def _half(name):
    """The yardstick: the same `transformers` model as .half(), run by torch on the GPU (built once per config)."""
    if name + "/half" not in _MODELS:
        import copy
        _MODELS[name + "/half"] = copy.deepcopy(_pair(name)[0]).half().to(DEV)
    return _MODELS[name + "/half"]


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("L", [5, 20, 77])
def test_encoder_matches_transformers_fp32(name, B, L):
    """Both output dtypes, with and without the fused projection, against fp32 `transformers` on the CPU (the projection's reference: F.linear on
    the fp32 hidden state).  Bound: the module docstring."""
    hf, proj, enc = _pair(name)
    ids = _ids(name, B, L, 100 * B + L)
    with torch.no_grad():
        ref = hf(ids)["last_hidden_state"]
        ref_p = torch.nn.functional.linear(ref, proj["weight"], proj["bias"])
    got = enc(ids)["last_hidden_state"]
    assert got.shape == ref.shape and got.dtype == torch.float32 and got.is_cuda
    got_p = enc.project(ids)
    assert got_p.shape == ref_p.shape and got_p.dtype == torch.float32
    got16, got_p16 = enc(ids, out_dtype=torch.float16)["last_hidden_state"], enc.project(ids, out_dtype=torch.float16)
    assert got16.dtype == got_p16.dtype == torch.float16
    enc.check_finite()
    e = [_rel(got, ref), _rel(got_p, ref_p), _rel(got16, ref), _rel(got_p16, ref_p)]
    with torch.no_grad():
        yard = _rel(_half(name)(ids.to(DEV))["last_hidden_state"], ref)
    print(f"[textenc-err] {name} B={B} L={L}: max |hip - ref| / max |ref|: hidden {e[0]:.3e}, projected {e[1]:.3e}, fp16 out {e[2]:.3e} / {e[3]:.3e}; "
          f"yardstick (transformers .half() on the GPU, hidden) {yard:.3e}")
    assert TOL <= CAP
    assert e[0] <= TOL and e[1] <= TOL
    assert e[2] <= min(TOL + H16, CAP) and e[3] <= min(TOL + H16, CAP)
    # the fp16 output is the fp32 one rounded once
    assert torch.equal(got16, got.to(torch.float16))


def test_encoder_is_exactly_causal_and_batch_independent():
    hf, proj, enc = _pair("h64_q")
    ids = _ids("h64_q", 3, 20, 5)
    base = enc(ids)["last_hidden_state"]
    for i in (0, 7, 18):
        other = ids.clone()
        other[:, i + 1:] = (other[:, i + 1:] + 1 + torch.arange(20 - i - 1)) % CONFIGS["h64_q"]["vocab_size"]
        got = enc(other)["last_hidden_state"]
        assert torch.equal(got[:, :i + 1], base[:, :i + 1]) and not torch.equal(got[:, i + 1:], base[:, i + 1:])
    other = ids.clone()
    other[1] = other[1].flip(0)
    got = enc.project(other)
    assert torch.equal(got[[0, 2]], enc.project(ids)[[0, 2]]) and not torch.equal(got[1], enc.project(ids)[1])


def test_fused_qkv_rows_are_q_then_k_then_v():
    """The library concatenates q_proj | k_proj | v_proj at load (rows [0, H), [H, 2H), [2H, 3H) of the fused operand, the order text_attn<d> reads).  A
    checkpoint whose three projections are exchanged cyclically must give what `transformers` gives for the same exchange, and something else than before:
    a loader that put a matrix into another block would agree with neither."""
    from transformers import CLIPTextModel
    hf, _, enc = _pair("h64_q")
    ids = _ids("h64_q", 2, 20, 11)
    sd = {k: v.clone() for k, v in hf.state_dict().items()}
    for k in list(sd):
        for a, b in (("q_proj", "k_proj"), ("k_proj", "v_proj"), ("v_proj", "q_proj")):
            if f".{a}." in k:
                sd[k] = hf.state_dict()[k.replace(a, b)].clone()
    hf2 = CLIPTextModel(hf.config).eval()
    hf2.load_state_dict(sd)
    with torch.no_grad():
        ref, ref2 = hf(ids)["last_hidden_state"], hf2(ids)["last_hidden_state"]
    got2 = models.CLIPTextModel(hf.config.to_dict(), sd, DEV)(ids)["last_hidden_state"]
    assert _rel(ref2, ref) > 20 * TOL, "the exchange must be visible far above the bound"
    assert _rel(got2, ref2) <= TOL and _rel(enc(ids)["last_hidden_state"], ref) <= TOL


# ---- 4. replay ---------------------------------------------------------------------------------------------------------------------------------
def test_replay_serves_new_ids_bit_for_bit():
    hf, proj, _ = _pair("h64_q")
    enc = models.CLIPTextModel(hf.config.to_dict(), hf.state_dict(), DEV).load_projection(proj)
    a, b, c, other_L = _ids("h64_q", 2, 20, 1), _ids("h64_q", 2, 20, 2), _ids("h64_q", 2, 20, 3), _ids("h64_q", 2, 9, 4)
    enc.set_graph(False)
    eager = {k: enc.project(v).clone() for k, v in (("b", b), ("c", c), ("o", other_L))}
    enc.set_graph(True)
    enc.project(a)                                                  # first use: eager
    assert torch.equal(enc.project(b), eager["b"])                 # second use: captured and replayed
    assert torch.equal(enc.project(c), eager["c"])                 # replay with new ids
    assert enc.graph_replays == 2 and enc.graph_nodes > 0
    assert torch.equal(enc.project(other_L), eager["o"])           # another L: a new configuration
    assert torch.equal(enc.project(other_L), eager["o"]) and torch.equal(enc.project(other_L), eager["o"])
    assert torch.equal(enc.project(b), eager["b"])
    enc.check_finite()


def test_reload_equals_a_fresh_handle():
    """One handle under graph replay: checkpoint A, then checkpoint B whole (tables, layers, projection), then A's token table alone.  After each load the
    outputs equal, bit for bit, the eager output of a fresh handle built from the same tensors, and only B's own graph counts replays: the tables take
    part in the checkpoint generation like every other tensor."""
    name, tok = "h64_q", "text_model.embeddings.token_embedding.weight"
    (hf_a, proj_a), (hf_b, proj_b) = _hf_model(name, seed=0), _hf_model(name, seed=3)
    sd_a, sd_b = (weights.normalize_clip_text_keys(hf.state_dict()) for hf in (hf_a, hf_b))
    ids = _ids(name, 2, 5, 21)
    fresh = lambda sd, proj: models.CLIPTextModel(hf_a.config.to_dict(), sd, DEV).load_projection(proj).set_graph(False).project(ids).clone()
    ref_a, ref_b = fresh(sd_a, proj_a), fresh(sd_b, proj_b)
    ref_ba = fresh({**sd_b, tok: sd_a[tok]}, proj_b)
    assert not torch.equal(ref_a, ref_b) and not torch.equal(ref_b, ref_ba), "the three checkpoints must give different outputs"
    enc = models.CLIPTextModel(hf_a.config.to_dict(), sd_a, DEV).load_projection(proj_a)
    for _ in range(3):                                              # eager, capture + replay, replay
        assert torch.equal(enc.project(ids), ref_a)
    assert enc.graph_replays == 2
    enc.load_state_dict(sd_b)
    enc.load_projection(proj_b)
    for i in range(3):                                              # eager again (another checkpoint generation), capture + replay, replay
        assert torch.equal(enc.project(ids), ref_b), f"forward {i} after the reload differs from a fresh handle's"
    assert enc.graph_replays == 4, "after the reload only B's own graph may count replays"
    enc.load_state_dict({tok: sd_a[tok]})
    for i in range(3):
        assert torch.equal(enc.project(ids), ref_ba), f"forward {i} after the token table's reload differs from a fresh handle's"
    assert enc.graph_replays == 6
    enc.check_finite()


# ---- 5. the shim end to end ------------------------------------------------------------------------------------------------------------------
def _tiny_sd_dirs(tmp_path, hidden=64):
    """An SD directory (tiny UNet / VAE, a character-level CLIP tokenizer, a CLIPTextModel of width `hidden` written by `transformers`) and a fine-tuned
    UNet directory with proj_weights.pt, in the layout the reference reads."""
    from safetensors.torch import save_file
    from transformers import CLIPTextConfig, CLIPTextModel, CLIPTokenizer
    sd_dir, w_dir = tmp_path / "sd", tmp_path / "train_save" / "unet" / "25_01_01"
    ucfg, vcfg = configs.TINY_UNET, configs.TINY_VAE
    usd = weights.synthetic_state_dict(weights.unet_param_shapes(ucfg), 42, fp16_values=True)
    vsd = weights.synthetic_state_dict(weights.vae_param_shapes(vcfg), 43, fp16_values=True)
    for d, cfg, sd in ((sd_dir / "unet", ucfg, usd), (sd_dir / "vae", vcfg, vsd), (w_dir, ucfg, usd)):
        d.mkdir(parents=True)
        json.dump(cfg, open(d / "config.json", "w"))
        save_file({k: v.contiguous() for k, v in sd.items()}, str(d / weights.WEIGHTS_NAME))
    chars = list("abcdefghijklmnopqrstuvwxyz")
    vocab = {c: i for i, c in enumerate(chars)}
    vocab.update({c + "</w>": len(chars) + i for i, c in enumerate(chars)})
    vocab["<|startoftext|>"], vocab["<|endoftext|>"] = len(vocab), len(vocab) + 1
    td = sd_dir / "tokenizer"
    td.mkdir()
    json.dump(vocab, open(td / "vocab.json", "w"))
    open(td / "merges.txt", "w").write("#version: 0.2\n")
    CLIPTokenizer(str(td / "vocab.json"), str(td / "merges.txt")).save_pretrained(str(td))
    torch.manual_seed(0)
    cfg = CLIPTextConfig(vocab_size=len(vocab), hidden_size=hidden, intermediate_size=2 * hidden, num_hidden_layers=2, num_attention_heads=4, max_position_embeddings=77,
                         bos_token_id=vocab["<|startoftext|>"], eos_token_id=vocab["<|endoftext|>"], pad_token_id=vocab["<|endoftext|>"])
    CLIPTextModel(cfg).save_pretrained(str(sd_dir / "text_encoder"))
    g = torch.Generator().manual_seed(77)
    proj = {"weight": torch.randn((ucfg["cross_attention_dim"], hidden), generator=g) * 0.2, "bias": torch.randn((ucfg["cross_attention_dim"],), generator=g) * 0.1}
    torch.save(proj, str(w_dir / "proj_weights.pt"))
    return sd_dir, w_dir, proj


def test_shim_end_to_end_with_the_hip_text_encoder(tmp_path):
    import transformers
    from ldiffusion_amd.pipeline import StableDiffusionImg2ImgPipeline
    from ldiffusion_amd.segmentor import Segmentor
    sd_dir, w_dir, proj = _tiny_sd_dirs(tmp_path)
    seg = Segmentor(None, None, "cell", 3)
    pipeline, unet, vae = seg.load_ldiffusion(str(w_dir), str(sd_dir), text_encoder="hip")
    assert isinstance(pipeline.text_encoder, models.CLIPTextModel) and pipeline.text_encoder.config.hidden_size == 64
    emb = seg._get_text_embeddings("A pathological slide", 2, pipeline, unet)
    tok = transformers.CLIPTokenizer.from_pretrained(str(sd_dir / "tokenizer"))
    enc = transformers.CLIPTextModel.from_pretrained(str(sd_dir / "text_encoder"))
    ids = torch.tensor(tok(["A pathological slide"] * 2)["input_ids"])
    assert ids.shape[1] == 20
    with torch.no_grad():
        ref = torch.nn.functional.linear(enc(ids)["last_hidden_state"], proj["weight"], proj["bias"])
    cad = unet.config.cross_attention_dim
    assert emb.shape == (2, 20, cad) and emb.is_cuda and emb.dtype == torch.float32
    err = _rel(emb, ref)
    print(f"[textenc-err] shim: max |hip - ref| / max |ref| = {err:.3e}")
    assert err <= TOL
    assert unet(torch.zeros((1, 4, 8, 8), device=DEV), 501, emb[:1]).sample.shape == (1, 4, 8, 8)   # the UNet takes it as its context unchanged
    # reference-shaped call sites work unchanged on the library's encoder
    hidden = pipeline.text_encoder(ids.to(DEV))["last_hidden_state"]
    assert hidden.shape == (2, 20, 64) and _rel(hidden, enc(ids)["last_hidden_state"].detach()) <= TOL
    # strict: a proj_weights.pt with a foreign key is refused
    torch.save(dict(proj, extra=torch.zeros(1)), str(w_dir / "proj_weights.pt"))
    with pytest.raises(RuntimeError, match="extra"):
        Segmentor(None, None, "cell", 3).load_ldiffusion(str(w_dir), str(sd_dir), text_encoder="hip")
    # the default loader is today's: a `transformers` model
    default = StableDiffusionImg2ImgPipeline.from_pretrained(str(sd_dir), torch_dtype=torch.float32, device=DEV)
    assert isinstance(default.text_encoder, transformers.CLIPTextModel)
    with pytest.raises(ValueError, match="text_encoder"):
        StableDiffusionImg2ImgPipeline.from_pretrained(str(sd_dir), text_encoder="onnx")


def test_multimodal_sampler_with_the_hip_text_encoder(tmp_path, monkeypatch):
    """Segmentor.ldiffusion_augment_for_multimodal (the call site with ids padded to 77) on a pipeline loaded with text_encoder="hip": the context
    the UNet receives is [1, 77, cross_attention_dim] within the encoder's bound of the `transformers` path's context, and the sampler returns its images."""
    from ldiffusion_amd import models as M
    from ldiffusion_amd.segmentor import Segmentor
    sd_dir, w_dir, proj = _tiny_sd_dirs(tmp_path)
    g = torch.Generator().manual_seed(70)
    rgb, dtm = torch.rand((1, 3, 200, 180), generator=g), torch.rand((1, 1, 200, 180), generator=g)
    eps32 = torch.finfo(torch.float32).eps
    u = torch.rand((1, 4, 32, 32), generator=g) * (2 - eps32) + (eps32 - 1)
    post = torch.randn((1, 4, 32, 32), generator=g)
    monkeypatch.setattr(M._LatentDist, "sample", lambda self, generator=None: self.mean + self.std * post.to(self.mean.device))

    class Recorder:   # the UNet as the sampler calls it, keeping the context it was handed
        def __init__(self, unet):
            self.unet, self.config, self.ctx = unet, unet.config, None

        def __call__(self, sample, t, encoder_hidden_states, **kw):
            self.ctx = encoder_hidden_states.clone()
            return self.unet(sample, t, encoder_hidden_states=encoder_hidden_states, **kw)

    out = {}
    for kind in ("hip", "transformers"):
        seg = Segmentor(None, None, "cell", 3)
        pipeline, unet, vae = seg.load_ldiffusion(str(w_dir), str(sd_dir), text_encoder=kind)
        shapes = unet._skip_shapes(1, 32, 32)

        def controlnet(sample, timestep, encoder_hidden_states, controlnet_cond, return_dict):   # the caller's module: a deterministic stand-in
            gg = torch.Generator().manual_seed(5)
            return [(torch.randn(sh, generator=gg) * 0.1).to(sample.device) for sh in shapes], (torch.randn(shapes[-1], generator=gg) * 0.1).to(sample.device)

        rec = Recorder(unet)
        imgs = seg.ldiffusion_augment_for_multimodal(rgb, dtm, pipeline, rec, vae, controlnet, 1, DEV, u=u)
        out[kind] = (rec.ctx, imgs)
    cad = configs.TINY_UNET["cross_attention_dim"]
    ctx, imgs = out["hip"]
    ref_ctx, ref_imgs = out["transformers"]
    assert ctx.shape == ref_ctx.shape == (1, 77, cad) and ctx.dtype == torch.float32 and ctx.is_cuda
    err = _rel(ctx, ref_ctx.cpu())
    print(f"[textenc-err] multimodal ctx (L = 77): max |hip - transformers| / max |transformers| = {err:.3e}; "
          f"images differ by at most {abs(imgs[0] - ref_imgs[0]).max():.3e}")
    assert err <= TOL
    assert len(imgs) == 1 and imgs[0].shape == (256, 256, 3) and bool((imgs[0] == imgs[0]).all())


def test_hip_text_encoder_without_proj_weights_gets_a_fresh_projection(tmp_path):
    """As the default path: no proj_weights.pt beside the UNet -> a freshly initialised Linear(hidden, cross_attention_dim); one of another width is refused at load."""
    from ldiffusion_amd.segmentor import Segmentor
    sd_dir, w_dir, proj = _tiny_sd_dirs(tmp_path)
    os.remove(str(w_dir / "proj_weights.pt"))
    seg = Segmentor(None, None, "cell", 3)
    pipeline, unet, _ = seg.load_ldiffusion(str(w_dir), str(sd_dir), text_encoder="hip")
    cad = unet.config.cross_attention_dim
    assert pipeline.text_encoder.projection_dim == cad and seg._get_text_embeddings("a slide", 1, pipeline, unet).shape[-1] == cad
    torch.save({"weight": torch.zeros((cad + 8, 64)), "bias": torch.zeros((cad + 8,))}, str(w_dir / "proj_weights.pt"))
    with pytest.raises(RuntimeError, match="cross_attention_dim"):
        Segmentor(None, None, "cell", 3).load_ldiffusion(str(w_dir), str(sd_dir), text_encoder="hip")


# ---- 6. non-finite detection ------------------------------------------------------------------------------------------------------------------
def test_overflow_of_the_residual_stream_is_reported():
    """The last layer's FC2 weight is scaled until the fp32 reference's residual stream leaves fp16's range; the weights themselves stay far inside it."""
    hf, _ = _hf_model("h64_q", seed=5)
    ids = _ids("h64_q", 2, 20, 9)
    sd = {k: v.clone() for k, v in hf.state_dict().items()}
    clean = models.CLIPTextModel(hf.config.to_dict(), sd, DEV)
    clean(ids)
    clean.check_finite()                                            # an unscaled model does not raise
    key = [k for k in sd if k.endswith("layers.1.mlp.fc2.weight")][0]
    with torch.no_grad():
        for _ in range(40):
            stream = hf(ids, output_hidden_states=True)["hidden_states"][-1]
            if stream.abs().max() > 1.5 * 65504:
                break
            hf.state_dict()[key].mul_(2.0)
    assert stream.abs().max() > 1.5 * 65504 and torch.isfinite(stream).all()
    sd[key] = hf.state_dict()[key].clone()
    assert sd[key].abs().max() < 60000, "the overflow must come from the activation, not from a weight beyond fp16's range"
    bad = models.CLIPTextModel(hf.config.to_dict(), sd, DEV)
    bad(ids)
    with pytest.raises(_lib.NonFiniteError):
        bad.check_finite()
    bad(ids[:, :5])
    with pytest.raises(_lib.NonFiniteError):                       # reported at the latest by the next forward on the handle
        torch.cuda.synchronize()
        bad(ids[:, :5])
    torch.cuda.synchronize()
    bad._lib.ldiff_textenc_check_finite(bad._h, _lib.stream_ptr())   # (clear the flag the last call left)


# ---- 7. validation at the ABI -----------------------------------------------------------------------------------------------------------------
def test_abi_refuses_bad_ids_and_lengths(lib):
    hf, proj, enc = _pair("h64_q")
    vocab = CONFIGS["h64_q"]["vocab_size"]
    out = torch.full((2 * 77 * 64,), 7.0, dtype=torch.float32, device=DEV)

    def call(ids, B, L):
        arr = (C.c_int32 * max(len(ids), 1))(*ids)
        return lib.ldiff_textenc_forward(enc._h, arr, B, L, 0, _lib.ptr(out), _lib.F32, _lib.stream_ptr())

    replays, nodes = enc.graph_replays, enc.graph_nodes
    assert call([1, 2, vocab, 3, 4, 5], 2, 3) == -1 and b"ids[0][2]" in lib.ldiff_last_error() and str(vocab).encode() in lib.ldiff_last_error()
    assert call([1, -1], 1, 2) == -1 and b"ids[0][1]" in lib.ldiff_last_error()
    assert call([], 1, 0) == -1 and b"L = 0" in lib.ldiff_last_error()
    assert call([0] * 78, 1, 78) == -1 and b"L = 78" in lib.ldiff_last_error() and b"77" in lib.ldiff_last_error()
    assert lib.ldiff_textenc_forward(enc._h, (C.c_int32 * 2)(1, 2), 1, 2, 0, _lib.ptr(out), _lib.BF16, _lib.stream_ptr()) == -1 and b"out_dtype" in lib.ldiff_last_error()
    torch.cuda.synchronize()
    assert torch.all(out == 7.0) and enc.graph_replays == replays and enc.graph_nodes == nodes   # nothing was launched
    with pytest.raises(ValueError, match="vocab_size"):
        enc(torch.tensor([[0, vocab]]))
    # act_out is the LDS-DMA GEMM's: a launch that kernel does not take is refused, never rerouted
    a = _lib.ConvArgs()
    x, w, y = (torch.zeros(n, dtype=torch.float16, device=DEV) for n in (8 * 72, 16 * 72, 8 * 16))
    a.x, a.w, a.y = x.data_ptr(), w.data_ptr(), y.data_ptr()
    a.C1, a.B, a.Hin, a.Win, a.Hout, a.Wout, a.ks, a.stride, a.N, a.Nrows, a.ldy, a.act_out = 72, 1, 1, 8, 1, 8, 1, 1, 16, 16, 16, 1   # K = 72: no multiple of 64
    assert lib.ldiff_op_conv(C.byref(a), _lib.stream_ptr()) == -1 and b"act_out" in lib.ldiff_last_error()
