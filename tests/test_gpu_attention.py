"""-m gpu: the forward attention kernels (csrc/kernels_attn.hip) against a float64 reference with a per-element error bound
(tests/attention_bound.py), at the layouts, lengths and score regimes the executors give them.

Layouts are the executors' own (csrc/model.hip): self-attention on fused q/k/v rows (ld = 3C, batch stride L * 3C; the VAE mid block is the
same with one head of 512), cross-attention with q rows of C and K / V in one [ctx_L, 2C] buffer per prompt (ldk = ldv = 2C, v = k + C,
kv_bstride 0 when the batch shares one prompt, ctx_L * 2C otherwise), and ldiff_op_attention_prescaled on fused rows.  The output goes to
rows of C + 8 with one spare row per image, prefilled with a sentinel: nothing outside the heads' columns and the Lq rows may change.

Every case states the kernel it is meant for (check_route) and must reject the wrong references of attention_bound: (i) the last key tile
left out, (ii) the first tile's V rows shifted by one key (where a late key holds the mass, R3, (ii') the last tile's instead), and, in
the peaky regime R2, (iii) the fixed-reference arithmetic attn<40,fixref> had (P packed toward zero against the first tile's maximum + 4
binades): the R2 cases can see that defect whatever the device does.  For L >= 1024 the reference covers whole 128-query blocks only:
the first, a middle one and the last (ragged) one of every image and head, against all keys.  [attn-err] lines give the worst error / bound
and the rejection margins; the module's teardown prints the worst ratio per kernel.

test_attention_launches_match_the_case_table runs SD-1.5-width UNet passes and VAE round trips under the profiler: every attention launch
they make must be a row of the case table (launches, flops and bytes per kernel as the table predicts them)."""
import ctypes as C
import math
import zlib

import pytest
import torch

import attention_bound as ab
from ldiffusion_amd import _lib
from kernel_routing import KERNEL_VARIANTS, check_route, reached

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FR, A48, A80, A160 = "attn<40,fixref>", "attn<64,48>", "attn<96,80>", "attn<160,160>"
X, D5, DS = "xattn<short-kv>", "attn<512,128q>", "attn<512,512>"
SENTINEL = -30000.0


# name -> (layout, B, heads, Lq, Lk, d, shared K / V, regime, kernel).  layout: "self" (fused q/k/v rows), "cross" (the [ctx_L, 2C] K / V
# buffer), "pre" (ldiff_op_attention_prescaled on fused rows).  The R0 rows of "self" / "cross" are the launches the executors make.
CASES = {}


def _add(name, *row):
    assert name not in CASES, name
    CASES[name] = row


# self-attention at the UNet's levels: the bench batch (8), one image, and the 1024^2 ROI's 128 x 128 latents; heads = 8
for B, L, d, kern in ((8, 4096, 40, FR), (8, 1024, 80, A80), (8, 256, 160, A160), (8, 64, 160, A160),
                      (1, 4096, 40, FR), (1, 1024, 80, A80), (1, 256, 160, A160), (1, 64, 160, A160),
                      (1, 16384, 40, FR), (1, 4096, 80, A80), (1, 1024, 160, A160),
                      (8, 16384, 40, FR), (8, 4096, 80, A80), (8, 1024, 160, A160)):
    _add(f"self_B{B}_L{L}_d{d}", "self", B, 8, L, L, d, False, "R0", kern)
# cross-attention at the same levels: a 6-token prompt shared by the batch or one per image, a 77-token prompt
for B, Lq, d, kern6, kern77 in ((8, 4096, 40, X, A48), (8, 1024, 80, A80, A80), (8, 256, 160, A160, A160), (8, 64, 160, A160, A160),
                                (8, 16384, 40, X, A48), (8, 4096, 80, X, A80), (8, 1024, 160, A160, A160),
                                (1, 4096, 40, A48, A48), (1, 1024, 80, A80, A80), (1, 256, 160, A160, A160), (1, 64, 160, A160, A160),
                                (1, 16384, 40, A48, A48), (1, 4096, 80, A80, A80), (1, 1024, 160, A160, A160)):
    _add(f"cross_B{B}_Lq{Lq}_d{d}_ctx6_shared", "cross", B, 8, Lq, 6, d, True, "R0", kern6)
    if B > 1:   # (one image: the executor passes kv_bstride 0 whatever the prompt)
        _add(f"cross_B{B}_Lq{Lq}_d{d}_ctx6_per_image", "cross", B, 8, Lq, 6, d, False, "R0", kern6)
    _add(f"cross_B{B}_Lq{Lq}_d{d}_ctx77", "cross", B, 8, Lq, 77, d, True, "R0", kern77)
# VAE mid block: one head of 512 on rows of 1536 (512^2 images: 4,096 tokens, 1024^2: 16,384; <= 64 queries: the d-split kernel)
for B, L, kern in ((8, 4096, D5), (1, 4096, D5), (1, 16384, D5), (8, 64, DS), (1, 64, DS)):
    _add(f"vae_B{B}_L{L}", "self", B, 1, L, L, 512, False, "R0", kern)
# the prescaled form (q arrives times scale * log2 e)
_add("pre_B1_L4096_d40", "pre", 1, 8, 4096, 4096, 40, False, "R0", A48)
_add("pre_B2_L1024_d80", "pre", 2, 8, 1024, 1024, 80, False, "R0", A80)

# score regimes (attention_bound.make_operands)
for reg in ("R2", "R1", "R4"):
    _add(f"{reg}_self_B1_L4096_d40", "self", 1, 8, 4096, 4096, 40, False, reg, FR)
    _add(f"{reg}_self_B1_L4096_d80", "self", 1, 8, 4096, 4096, 80, False, reg, A80)
    _add(f"{reg}_vae_B1_L4096", "self", 1, 1, 4096, 4096, 512, False, reg, D5)
    _add(f"{reg}_pre_B1_L4096_d40", "pre", 1, 8, 4096, 4096, 40, False, reg, A48)
_add("R2_self_B1_L16384_d40", "self", 1, 8, 16384, 16384, 40, False, "R2", FR)
_add("R2_self_B2_L4096_d160", "self", 2, 8, 4096, 4096, 160, False, "R2", A160)
for reg in ("R1", "R4"):
    _add(f"{reg}_self_B2_L256_d160", "self", 2, 8, 256, 256, 160, False, reg, A160)
    _add(f"{reg}_cross_B8_Lq4096_d40_ctx6", "cross", 8, 8, 4096, 6, 40, False, reg, X)
    _add(f"{reg}_cross_B2_Lq1024_d80_ctx77", "cross", 2, 8, 1024, 77, 80, False, reg, A80)
for x in (14, 17, 21):   # late key inside the fixed-reference window (needs > 19 binades: d512, > 20: fixref) and outside it
    _add(f"R3_{x}_self_B2_L1024_d40", "self", 2, 8, 1024, 1024, 40, False, f"R3:{x}", FR)
    _add(f"R3_{x}_vae_B2_L1024", "self", 2, 1, 1024, 1024, 512, False, f"R3:{x}", D5)
    _add(f"R3_{x}_self_B2_L1024_d80", "self", 2, 8, 1024, 1024, 80, False, f"R3:{x}", A80)
_add("R3_21_pre_B2_L1024_d40", "pre", 2, 8, 1024, 1024, 40, False, "R3:21", A48)
_add("R3_21_cross_B2_Lq300_d160_Lk200", "cross", 2, 8, 300, 200, 160, False, "R3:21", A160)
for name, row in (("self_B2_L256_d40", ("self", 2, 8, 256, 256, 40, False, "R5", FR)),
                  ("self_B2_L256_d80", ("self", 2, 8, 256, 256, 80, False, "R5", A80)),
                  ("self_B2_L64_d160", ("self", 2, 8, 64, 64, 160, False, "R5", A160)),
                  ("cross_B8_Lq4096_d40_ctx6", ("cross", 8, 8, 4096, 6, 40, False, "R5", X)),
                  ("vae_B2_L256", ("self", 2, 1, 256, 256, 512, False, "R5", D5)),
                  ("vae_B2_L64", ("self", 2, 1, 64, 64, 512, False, "R5", DS))):
    _add("R5_" + name, *row)

# edges: key counts around one and two 64-key tiles (fixref takes Lk >= 128), d512 at 64 / 65 queries and around its 128-query block
for L in (1, 63, 64, 65, 127, 128, 129):
    _add(f"edge_self_B2_L{L}_d40", "self", 2, 8, L, L, 40, False, "R0", FR if L >= 128 else A48)
    _add(f"edge_cross_B2_Lq300_Lk{L}_d80", "cross", 2, 8, 300, L, 80, False, "R0", A80)
    _add(f"edge_vae_B2_L{L}", "self", 2, 1, L, L, 512, False, "R0", D5 if L > 64 else DS)
# xattn's selector: at most 16 keys, at least 384 workgroups of 64 queries (B * ceil(Lq / 64): 383 at 24,512 queries, 384 at 24,513)
for B, Lq, Lk, kern in ((8, 4096, 16, X), (8, 4096, 17, A48), (1, 24512, 6, A48), (1, 24513, 6, X), (8, 3071, 6, X), (8, 3073, 6, X)):
    _add(f"edge_cross_B{B}_Lq{Lq}_Lk{Lk}_d40", "cross", B, 8, Lq, Lk, 40, True, "R0", kern)
# query counts one off a 16-, 64- and 128-row block
for Lq in (15, 17, 63, 65, 127, 129):
    _add(f"edge_cross_B2_Lq{Lq}_Lk200_d40", "cross", 2, 8, Lq, 200, 40, False, "R0", FR)
    _add(f"edge_cross_B2_Lq{Lq}_Lk77_d80", "cross", 2, 8, Lq, 77, 80, True, "R0", A80)

# wrong references a case cannot see, with the reason (the case then rejects the others)
INVISIBLE = {"(ii)": {**{n: "one key: nothing to shift" for n, r in CASES.items() if r[4] == 1},
                      **{n: "the late key holds all but ~2^-17 of every row's mass; (ii') is rejected instead" for n, r in CASES.items()
                         if r[7] == "R3:21"}}}

WORST = {}    # kernel -> worst error / bound
MARGIN = {}   # wrong reference -> narrowest rejection margin


def sp():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def eval_rows(Lq):
    """The query rows the reference covers: all of them below 1024, else the first, a middle and the last 128-query block."""
    if Lq < 1024:
        return torch.arange(Lq)
    nb = -(-Lq // 128)
    return torch.cat([torch.arange(b * 128, min(Lq, b * 128 + 128)) for b in (0, nb // 2, nb - 1)])


def run_case(lib, name):
    """Launch the case's kernel on the executor's layout -> (got [B, heads, R, d], q [B, heads, R, d], k / v [Bk, heads, Lk, d], scale, names)
    with the reference operands on the device in float32 (fp16-rounded values); checks the output guard."""
    layout, B, heads, Lq, Lk, d, shared, regime, kern = CASES[name]
    Cc = heads * d
    Bk = 1 if shared else B
    q, k, v = ab.make_operands(B, Bk, heads, Lq, Lk, d, regime, zlib.crc32(name.encode()) % 100000)
    scale = 1.0 / math.sqrt(d)
    rows = lambda t: t.permute(0, 2, 1, 3).reshape(t.shape[0], t.shape[2], Cc)   # [B, heads, L, d] -> [B, L, C]
    if layout == "pre":
        q = (q * (scale * ab.LOG2E)).to(torch.float16).float()
        scale = 1.0 / ab.LOG2E
    ldo = Cc + 8
    o = torch.full((B, Lq + 1, ldo), SENTINEL, dtype=torch.float16, device=DEV)
    if layout in ("self", "pre"):
        buf = torch.cat([rows(q), rows(k), rows(v)], -1).to(torch.float16).to(DEV)
        base = buf.data_ptr()
        args = (base, 3 * Cc, base + 2 * Cc, 3 * Cc, base + 4 * Cc, 3 * Cc, o.data_ptr(), ldo, B, heads, Lq, Lk, d, Lq * 3 * Cc, Lk * 3 * Cc, (Lq + 1) * ldo)
    else:
        qd = rows(q).to(torch.float16).to(DEV)
        buf = torch.cat([rows(k), rows(v)], -1).to(torch.float16).to(DEV)
        base = buf.data_ptr()
        args = (qd.data_ptr(), Cc, base, 2 * Cc, base + 2 * Cc, 2 * Cc, o.data_ptr(), ldo, B, heads, Lq, Lk, d, Lq * Cc, 0 if shared else Lk * 2 * Cc,
                (Lq + 1) * ldo)
    with reached(lib) as names:
        if layout == "pre":
            _lib.check(lib.ldiff_op_attention_prescaled(*args, sp()))
        else:
            _lib.check(lib.ldiff_op_attention(*args, scale, sp()))
    torch.cuda.synchronize()
    guard = o.clone()
    guard[:, :Lq, :Cc] = SENTINEL
    assert (guard == SENTINEL).all(), f"{name}: the kernel wrote outside the heads' columns or past row Lq"
    idx = eval_rows(Lq)
    got = o[:, idx.to(DEV), :Cc].view(B, len(idx), heads, d).permute(0, 2, 1, 3).float()
    return got, q[:, :, idx].to(DEV), k.to(DEV), v.to(DEV), scale, names


@pytest.mark.parametrize("name", list(CASES))
def test_attention_against_float64(lib, name):
    layout, B, heads, Lq, Lk, d, shared, regime, kern = CASES[name]
    got, q, k, v, scale, names = run_case(lib, name)
    check_route(names, kern, name)
    N = B * heads
    kk, vv = (t.expand(B, -1, -1, -1).reshape(N, Lk, d) for t in (k, v))
    qq, gg = q.reshape(N, -1, d), got.reshape(N, -1, d)
    ref, tol = ab.reference(qq, kk, vv, scale, kern)
    assert torch.isfinite(gg).all(), f"{name}: non-finite output"
    r = ab.ratio(gg, ref, tol)
    wrong = ab.wrong_references(qq, kk, vv, scale, kern, last_tile_shift=regime.startswith("R3"))
    if regime == "R2":
        wrong.append(("(iii) fixed reference, P toward zero", ab.fixref_emulation(qq, kk, vv, scale), tol))
    rej, seen = [], []
    for wname, wref, wtol in wrong:
        tag = wname.split()[0]
        why = INVISIBLE.get(tag, {}).get(name)
        wr = ab.ratio(gg, wref, wtol)
        rej.append(f"{tag} {wr:.3g}x" + (f" (not asserted: {why})" if why else ""))
        if not why:
            seen.append((wname, wr))
    print(f"[attn-err] {name} on {kern}: {r:.3f} of the bound; wrong refs at {', '.join(rej)} of theirs")
    WORST[kern] = max(WORST.get(kern, 0.0), r)
    for wname, wr in seen:
        MARGIN[wname.split()[0]] = min(MARGIN.get(wname.split()[0], math.inf), wr)
        assert wr > 1.0, f"{name}: the bound does not reject the wrong reference '{wname}' (worst {wr:.3f} of its bound)"
    assert r <= 1.0, f"{name}: error {r:.3f} of the bound on {kern}"


# ------------------------------------------------------------------------------------------------------------------------------------------
# launch accounting: the executors' attention launches are rows of the case table
# ------------------------------------------------------------------------------------------------------------------------------------------
def _sig(row):
    layout, B, heads, Lq, Lk, d, shared, regime, kern = row
    return (layout, B, heads, Lq, Lk, d, shared)


# the launch shapes of the executors: the R0 rows of the self / cross / VAE table (not the regimes, the prescaled op or the edges)
TABLE = {_sig(r): r[-1] for n, r in CASES.items() if r[7] == "R0" and r[0] != "pre" and not n.startswith("edge_")}


def unet_launches(cfg, B, size, ctx_L, ctx_B):
    """The attention launches of one UNet pass: (layout, B, heads, Lq, Lk, d, shared) per launch (ldiff_unet::transformer)."""
    heads, chans, lpb = cfg["attention_head_dim"], cfg["block_out_channels"], cfg["layers_per_block"]
    per_level = [0] * len(chans)
    for i, t in enumerate(cfg["down_block_types"]):
        per_level[i] += lpb if t.startswith("CrossAttn") else 0
    for i, t in enumerate(cfg["up_block_types"]):
        per_level[len(chans) - 1 - i] += lpb + 1 if t.startswith("CrossAttn") else 0
    out = []
    for lvl, n in enumerate(per_level + [1]):   # (+ the mid block, at the lowest level)
        lvl = min(lvl, len(chans) - 1)
        L, d = (size >> lvl) ** 2, chans[lvl] // heads
        out += [("self", B, heads, L, L, d, False), ("cross", B, heads, L, ctx_L, d, ctx_B == 1)] * n
    return out


def predict(launches):
    """{kernel: [launches, flops, bytes]} as the case table and the ProfScope accounting of launch_attention give them."""
    out = {}
    for sig in launches:
        assert sig in TABLE, f"attention launch {sig} is no row of the case table"
        _, B, h, Lq, Lk, d, shared = sig
        acc = out.setdefault(TABLE[sig], [0, 0.0, 0.0])
        acc[0] += 1
        acc[1] += 4.0 * B * h * Lq * Lk * d
        acc[2] += 2.0 * B * h * d * (2.0 * Lq + 2.0 * Lk * (1.0 / B if shared else 1.0))
    return out


def profiled(lib, fn):
    """{attention kernel: [launches, flops, bytes]} of what fn() launches (eagerly: the profiler is on)."""
    torch.cuda.synchronize()
    lib.ldiff_prof_set_filter(None)
    _lib.prof_collect()
    lib.ldiff_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
        rows = _lib.prof_collect()
    finally:
        lib.ldiff_prof_enable(0)
    attn = set(KERNEL_VARIANTS["launch_attention"])
    return {r["name"]: [r["launches"], r["flops"], r["bytes"]] for r in rows if r["name"] in attn}


@pytest.mark.timeout(900)
def test_attention_launches_match_the_case_table(lib):
    """Eager SD-1.5-width UNet passes (B = 1 and 8; a 6-token prompt shared or per image, a 77-token prompt; 64 x 64 and 128 x 128 latents)
    and VAE encode + decode at 512^2 and 1024^2: per attention kernel, the profiler's launches, flops and bytes equal what the case table
    predicts, so an executor launch no case covers fails here."""
    from ldiffusion_amd import configs, weights
    from ldiffusion_amd.models import AutoencoderKL, UNet2DConditionModel
    g = torch.Generator().manual_seed(9)
    ucfg, vcfg = configs.SD15_UNET, configs.SD15_VAE
    unet = UNet2DConditionModel(ucfg, weights.synthetic_state_dict(weights.unet_param_shapes(ucfg), 42, fp16_values=True), DEV)
    for size in (64, 128):
        for B in (1, 8):
            for ctx_L, ctx_B in ((6, 1), (6, B), (77, 1)) if B > 1 else ((6, 1), (77, 1)):
                x = torch.randn((B, 4, size, size), generator=g).to(DEV)
                ctx = (torch.randn((ctx_B, ctx_L, 768), generator=g) * 0.5).to(DEV)
                got = profiled(lib, lambda: unet(x, 501, ctx).sample)
                _compare(f"unet B={B} {size}x{size} ctx {ctx_B}x{ctx_L}", got, predict(unet_launches(ucfg, B, size, ctx_L, ctx_B)))
    del unet
    vae = AutoencoderKL(vcfg, weights.synthetic_state_dict(weights.vae_param_shapes(vcfg), 43, fp16_values=True), DEV)
    for size in (512, 1024):
        img = torch.rand((1, 3, size, size), generator=g).to(DEV)
        L = (size // 8) ** 2
        got = profiled(lib, lambda: vae.decode(vae.encode(img).latent_dist.mean).sample)
        _compare(f"vae {size}^2", got, predict([("self", 1, 1, L, L, 512, False)] * 2))


def _compare(what, got, want):
    print(f"[attn-launches] {what}: " + ", ".join(f"{k} x{v[0]}" for k, v in sorted(got.items())))
    assert set(got) == set(want), f"{what}: kernels {sorted(got)}, the case table predicts {sorted(want)}"
    for kname, (n, fl, by) in want.items():
        gn, gfl, gby = got[kname]
        assert gn == n, f"{what}: {kname} launched {gn} times, the case table predicts {n}"
        assert math.isclose(gfl, fl, rel_tol=1e-12) and math.isclose(gby, by, rel_tol=1e-12), \
            f"{what}: {kname} flops / bytes {gfl:.6g} / {gby:.6g}, the case table predicts {fl:.6g} / {by:.6g}"


def pinned_kernels():
    """Every kernel a case of this file states it reaches (test_gpu_kernels.pinned_kernels takes these in)."""
    return {r[-1] for r in CASES.values()}


def teardown_module(module):
    if WORST:
        print("\n[attn-err] worst measured error / bound per kernel: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))
        print("[attn-err] narrowest rejection margin per wrong reference: " + ", ".join(f"{k} {v:.3g}x" for k, v in sorted(MARGIN.items())))
