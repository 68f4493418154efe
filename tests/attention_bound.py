"""Float64 reference and per-element error bound for the forward attention kernels (csrc/kernels_attn.hip).  Imports without a GPU.

Contract.  u = 2^-24, gamma(n) = 2 n u (as in test_gpu_backward.py).  Per query row, on the fp16-rounded operands:
    S = scale q k^T,  m = max_j S_j,  p_j = exp(S_j - m),  Z = sum_j p_j,  o = sum_j p_j v_j / Z.
A kernel that takes the scores in fp32, rounds each probability ONCE TO NEAREST fp16 relative to the row maximum, sums in fp32 and rounds o
to fp16 is, in every channel c, within
    tol_c = 2^-11 |o_c| + 2^-24
          + (1/Z) sum_j [eS_j p_j |v_jc - o_c| + (2^-11 p_j + 2^-25) w_jc]
          + gamma(Lk + 1) (1/Z) sum_j p_j (|v_jc| + |o_c|) + (T + 2) u |o_c|,          times (1 + 2^-10) for second-order terms,
    eS_j  = gamma(d) scale sum |q| |k_j| + 4u (|S_j| + |m|) + 2u
(the fp32 score sum, the scale * log2(e) multiply, the reference FMA and exp2).  w_jc = |v_jc - o_c| where the row sum comes from the same
rounded P (a ones row of V^T: attn<40,fixref>, and the generic kernel whenever d < DV of its instantiation), |v_jc| where it is the fp32
sum of the unrounded P (xattn<short-kv>, attn<512,*>, the generic kernel at d = DV).  T = the number of key tiles: one fp32 rescale of
the accumulators per tile.  The fixed-reference kernels get no allowance for their lead or rounding mode.

The wrong references the cases must reject (each one's bound is that of the operation it computes):
    (i)   the last key tile left out (64 keys, or the last key when Lk <= 64);
    (ii)  the V rows of the first key tile shifted by one key (row j takes row j + 1's values; the last row of the tile keeps its own);
          (ii') the same for the last key tile, where a late key holds the mass (regime R3);
    (iii) the fixed-reference arithmetic attn<40,fixref> had: reference = the first 64-key tile's maximum + 4 binades, P packed round
          toward zero into fp16 (subnormals kept), the row sum from the same rounded P (fixref_emulation).
"""
import math

import torch

U = 2.0 ** -24
H16 = 2.0 ** -11
LOG2E = 1.4426950408889634
BUDGET = 1 << 25   # float64 elements of the largest [rows, Lk, d] temporary


def gamma(n):
    return 2.0 * n * U


def ones_row_sum(kernel, d):
    """True where `kernel` takes the row sum from the rounded P through a ones row of V^T (w = |v - o|), False where it sums the unrounded
    P in fp32 (w = |v|).  The generic attn<DQK,DV> decides per launch (launch_attn_cfg: d < DV)."""
    if kernel == "attn<40,fixref>":
        return True
    if kernel == "xattn<short-kv>" or kernel.startswith("attn<512,"):
        return False
    dv = int(kernel[:-1].split(",")[1])
    return d < dv


def key_tile(kernel, Lk):
    """Keys per tile of `kernel`: T = ceil(Lk / key_tile)."""
    if kernel == "xattn<short-kv>":
        return max(Lk, 1)
    return 32 if kernel.startswith("attn<512,") else 64


def _rows(q, k, v, scale, ones, T):
    """One chunk: q [N, r, d], k / v [N, Lk, d] (float64) -> o, tol [N, r, d]."""
    d, Lk = q.shape[-1], k.shape[-2]
    S = scale * (q @ k.transpose(-1, -2))
    m = S.amax(-1, keepdim=True)
    p = torch.exp(S - m)
    Z = p.sum(-1, keepdim=True)
    o = (p @ v) / Z
    eS = gamma(d) * scale * (q.abs() @ k.abs().transpose(-1, -2)) + 4 * U * (S.abs() + m.abs()) + 2 * U
    dv = (v.unsqueeze(1) - o.unsqueeze(2)).abs()                      # [N, r, Lk, d]
    t = torch.einsum("nrj,nrjc->nrc", eS * p, dv)
    if ones:
        t += torch.einsum("nrj,nrjc->nrc", H16 * p + 2.0 ** -25, dv)
    else:
        t += (H16 * p + 2.0 ** -25) @ v.abs()
    t += gamma(Lk + 1) * (p @ v.abs() + Z * o.abs())
    tol = (H16 * o.abs() + U + t / Z + (T + 2) * U * o.abs()) * (1 + 2.0 ** -10)
    return o, tol


def reference(q, k, v, scale, kernel):
    """q [N, Lq, d], k / v [N, Lk, d] (any float dtype, the fp16-rounded values) -> (o, tol) float64 [N, Lq, d] on q's device, the
    contract bound of `kernel`.  Chunked over the queries so no temporary exceeds BUDGET elements."""
    q, k, v = q.double(), k.double(), v.double()
    N, Lq, d = q.shape
    Lk = k.shape[1]
    ones, T = ones_row_sum(kernel, d), -(-Lk // key_tile(kernel, Lk))
    r = max(1, BUDGET // max(1, N * Lk * d))
    outs = [_rows(q[:, i:i + r], k, v, scale, ones, T) for i in range(0, Lq, r)]
    return torch.cat([a for a, _ in outs], 1), torch.cat([b for _, b in outs], 1)


def drop_last_tile(k, v):
    """(i): k, v without their last 64 keys (without the last key when Lk <= 64); None when nothing is left."""
    Lk = k.shape[1]
    keep = Lk - 64 if Lk > 64 else Lk - 1
    return None if keep <= 0 else (k[:, :keep], v[:, :keep])


def shift_tile(v, j0=0):
    """(ii): the V rows of the 64-key tile from key j0 shifted by one key: row j takes row j + 1's values (the tile's last row keeps its own)."""
    w = v.clone()
    n = min(j0 + 64, v.shape[1])
    w[:, j0:n - 1] = v[:, j0 + 1:n]
    return w


def wrong_references(q, k, v, scale, kernel, last_tile_shift=False):
    """[(name, o, tol)] of (i) and (ii), each with the bound of the operation it computes; (i) of a single key is all zeros.
    last_tile_shift: also (ii'), the LAST tile's V rows shifted (for rows whose mass sits in a late key, where (ii) cannot show)."""
    out = []
    dk = drop_last_tile(k, v)
    if dk is None:
        z = torch.zeros(q.shape, dtype=torch.float64, device=q.device)
        out.append(("(i) the only key left out", z, z + U))
    else:
        out.append(("(i) last key tile left out",) + reference(q, dk[0], dk[1], scale, kernel))
    out.append(("(ii) first tile's V shifted",) + reference(q, k, shift_tile(v), scale, kernel))
    if last_tile_shift:
        out.append(("(ii') last tile's V shifted",) + reference(q, k, shift_tile(v, (v.shape[1] - 1) // 64 * 64), scale, kernel))
    return out


def _rtz16(e):
    """fp32 -> fp16 rounded toward zero, subnormals kept (v_cvt_pkrtz_f16_f32); e >= 0."""
    h = e.to(torch.float16)
    up = h.float() > e
    return (h.view(torch.int16) - up.to(torch.int16)).view(torch.float16)


def fixref_emulation(q, k, v, scale, lead=4.0, tile=64, rtz=True, ones=True):
    """(iii) the fixed-reference arithmetic, per row in float64 except where the kernel rounds: reference = (maximum over the first `tile`
    keys) + `lead` binades, e = exp2(t - reference) in fp32, packed into fp16 (toward zero, or to nearest with rtz=False), o = sum h v / sum h
    (ones: the row sum from the rounded P) or / the fp32 sum of e."""
    t = (scale * (q.double() @ k.double().transpose(-1, -2))) * LOG2E
    e = torch.exp2(t - (t[..., :tile].amax(-1, keepdim=True) + lead)).float()
    h = (_rtz16(e) if rtz else e.to(torch.float16)).double()
    den = h.sum(-1, keepdim=True) if ones else e.double().sum(-1, keepdim=True)
    return (h @ v.double()) / den


def online_emulation(q, k, v, scale, tile=64, ones=False):
    """An online softmax as the contract assumes it: fp32 scores, a running maximum per `tile` keys, P rounded to nearest fp16, fp32
    accumulators rescaled once per tile, row sums of the rounded P (ones) or of the fp32 P, an fp16 output."""
    q32, k32, v32 = q.float(), k.float(), v.to(torch.float16).float()
    s = (q32 @ k32.transpose(-1, -2)) * (scale * LOG2E)
    mrun = torch.full(s.shape[:-1] + (1,), -1e30)
    acc = torch.zeros(q.shape[:-1] + (v.shape[-1],))
    l = torch.zeros_like(mrun)
    for j0 in range(0, s.shape[-1], tile):
        st = s[..., j0:j0 + tile]
        mnew = torch.maximum(mrun, st.amax(-1, keepdim=True))
        alpha = torch.exp2(mrun - mnew)
        p = torch.exp2(st - mnew)
        ph = p.to(torch.float16).float()
        acc = acc * alpha + ph @ v32[..., j0:j0 + tile, :]
        l = l * alpha + (ph if ones else p).sum(-1, keepdim=True)
        mrun = mnew
    return (acc / l).to(torch.float16)


def ratio(got, ref, tol):
    """max |got - ref| / tol (float64); an element whose bound is 0 must match exactly."""
    err = (got.double() - ref.double()).abs()
    tol = tol.double()
    r = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    return r.max().item() if r.numel() else 0.0


SPIKE = 8.0   # channel-0 value of a spike key (R2, R3): its score above the row's bulk is that of q's channel 0 times SPIKE * scale


def make_operands(B, Bk, heads, Lq, Lk, d, regime, seed):
    """fp16-rounded operands (float32) of one case: q [B, heads, Lq, d], k / v [Bk, heads, Lk, d] (Bk = 1: K / V shared by the batch).
    Score regimes, scale = 1 / sqrt(d):
      R0  q, k, v ~ N(0, 1): scores ~ N(0, 1) nats
      R1  q times 3: a spread of about 3 nats
      R2  one key per (image, head) in the FIRST key tile 7 - 12 nats (uniform per row) above the row's bulk (channel 0 of q and k is reserved
          for it): most of the mass in many small probabilities
      R3:X  a key in the LAST key tile X binades above the row's maximum over the first tile (Lk >= 128)
      R4  V with a common offset of 8 - 20 per channel (separates the |v| and |v - o| terms)
      R5  every key of a head equal: all scores of a row equal, o is the mean of v"""
    g = torch.Generator().manual_seed(seed)
    scale = 1.0 / math.sqrt(d)
    q = torch.randn((B, heads, Lq, d), generator=g)
    k = torch.randn((Bk, heads, Lk, d), generator=g)
    v = torch.randn((Bk, heads, Lk, d), generator=g)
    name, _, arg = regime.partition(":")
    if name == "R1":
        q *= 3.0
    elif name in ("R2", "R3"):
        q[..., 0] = 0.0
        k[..., 0] = 0.0
        if name == "R2":
            j = torch.randint(0, min(64, Lk), (heads,), generator=g)
            k[:, torch.arange(heads), j, 0] = SPIKE
            q[..., 0] = (7.0 + 5.0 * torch.rand((B, heads, Lq), generator=g)) / (SPIKE * scale)
        else:
            assert Lk >= 128, "R3 needs a key tile after the first"
            j = (Lk - 1) // 64 * 64 + torch.randint(0, Lk - (Lk - 1) // 64 * 64, (heads,), generator=g)
            j = torch.minimum(j, torch.full_like(j, Lk - 1))
            k[:, torch.arange(heads), j, 0] = SPIKE
            qr, kr = q.half().float(), k.half().float()
            s = scale * (qr @ kr.transpose(-1, -2))                                       # [B, heads, Lq, Lk] (Bk broadcast)
            m1 = s[..., :64].amax(-1)
            sj = s.gather(-1, j.view(1, heads, 1, 1).expand(B, heads, Lq, 1))[..., 0]
            q[..., 0] = (m1 + float(arg) * math.log(2.0) - sj) / (SPIKE * scale)
    elif name == "R4":
        v += 8.0 + 12.0 * torch.rand((Bk, heads, 1, d), generator=g)
    elif name == "R5":
        k[:] = k[:, :, :1]
    else:
        assert name == "R0", regime
    return tuple(t.to(torch.float16).float() for t in (q, k, v))
