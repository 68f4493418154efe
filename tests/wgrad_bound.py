"""float64 / integer references, error bounds and numpy emulations for the direct weight gradient and the slab column sum (csrc/kernels_wgrad.hip;
ldiff_op_conv_wgrad, ldiff_op_colsum_slabs).  tests/test_cpu_wgrad_bound.py pins the reference to torch's conv2d backward and shows what the bound rejects;
tests/test_gpu_wgrad_direct.py holds the kernels to it.

The bound, per element of dw (and of db):   |kernel - float64| <= (L + P + 2) u  sum |dy x|,   u = 2^-24
  L = the most terms one fp32 accumulator of a workgroup adds, an MFMA's 32-term inner sum counted as 32 terms (ag.wgrad_plan(...)["chain"]: tiles a workgroup
      walks x tile rows x 32; for the column sum ag.colsum_slabs_plan(...)["chain"]: rows a thread adds + the row lanes one LDS pass adds),
  P = the partial sums the finalize adds in order (["partials"]),
  2 = the products are exact in fp32 (fp16 x fp16), the inputs are given: two units of slack for the finalize's last rounding and the store.
This is the standard bound gamma(n) sum |terms| of a sum of n terms in any order, n <= L + P.  Both L and P come from the kernel's own plan of the case;
nothing measured goes into the bound."""
import numpy as np

from ldiffusion_amd import autograd as ag

U = 2.0 ** -24
FIN_GROUPS = 8   # csrc/kernels_wgrad.hip: interleaved chains of the two finalize kernels


def im2col(x, k, stride, Ho, Wo, clamp=False, shift_tap=None):
    """x [B, H, W, C] -> [B, Ho, Wo, k*k, C]: pixel (oy stride - p + ky, ox stride - p + kx) of tap (ky, kx), zero outside the image.
    Mutations: clamp = edge clamping instead of zero padding; shift_tap = (tap, dx): that tap reads dx pixels further right."""
    p = k // 2
    e = p + 1   # one more ring for the shifted-tap mutation
    xp = np.pad(x, ((0, 0), (e, e), (e, e), (0, 0)), mode="edge" if clamp else "constant")
    out = np.empty((x.shape[0], Ho, Wo, k * k, x.shape[3]), dtype=x.dtype)
    for ky in range(k):
        for kx in range(k):
            sx = shift_tap[1] if shift_tap is not None and shift_tap[0] == ky * k + kx else 0
            y0, x0 = e - p + ky, e - p + kx + sx
            out[:, :, :, ky * k + kx] = xp[:, y0:y0 + (Ho - 1) * stride + 1:stride, x0:x0 + (Wo - 1) * stride + 1:stride]
    return out


def wgrad_reference(x, dy, Cout, Cin, k, stride, dtype=np.float64, **mut):
    """(dw [Cout, Cin, k, k], mag = sum |dy x| per element) in `dtype` (np.float64, or np.int64 for integer data) from NHWC arrays x [B,H,W,Cx], dy [B,Ho,Wo,Cy]."""
    B, Ho, Wo, _ = dy.shape
    xc = im2col(x[..., :Cin].astype(dtype), k, stride, Ho, Wo, **mut).reshape(B * Ho * Wo, k * k * Cin)
    d = dy[..., :Cout].astype(dtype).reshape(B * Ho * Wo, Cout)
    dw = (d.T @ xc).reshape(Cout, k, k, Cin).transpose(0, 3, 1, 2)
    mag = (np.abs(d).T @ np.abs(xc)).reshape(Cout, k, k, Cin).transpose(0, 3, 1, 2)
    return np.ascontiguousarray(dw), np.ascontiguousarray(mag)


def bound(mag, plan):
    return (plan["chain"] + plan["partials"] + 2) * U * mag


def tile_rows(B, Ho, Wo, k, plan):
    """Per tile of the kernel's walk, the tile rows as arrays of flat pixel indices m = (b Ho + oy) Wo + ox (at most 32 each)."""
    TH = plan["TH"]
    tiles = []
    if k == 1:
        M = B * Ho * Wo
        for t in range(plan["tiles"]):
            tiles.append([np.arange(m, min(m + 32, M)) for m in range(t * TH * 32, min((t + 1) * TH * 32, M), 32)])
    else:
        for b in range(B):
            for ty in range(-(-Ho // TH)):
                for tx in range(-(-Wo // 32)):
                    tiles.append([(b * Ho + oy) * Wo + np.arange(tx * 32, min(tx * 32 + 32, Wo)) for oy in range(ty * TH, min(ty * TH + TH, Ho))])
    assert len(tiles) == plan["tiles"]
    return tiles


def wgrad_emulate(x, dy, Cout, Cin, k, stride, plan, acc=np.float32, partial=np.float32, **mut):
    """The kernel's order of operations in numpy: workgroup w walks tiles w, w + wgs, ...; per tile row one 32-term inner sum (formed in float64, then one
    rounding to `acc` on the add into the accumulator); the workgroup's block stored as `partial`; the finalize adds the blocks in float32 in its fixed order: FIN_GROUPS interleaved chains, then the chains.
    acc = partial = float32 is the kernel as built; partial = float16 is the mutation 'partials rounded to fp16'."""
    B, Ho, Wo, _ = dy.shape
    xc = im2col(x[..., :Cin].astype(np.float64), k, stride, Ho, Wo, **mut).reshape(B * Ho * Wo, k * k * Cin)
    d = dy[..., :Cout].astype(np.float64).reshape(B * Ho * Wo, Cout)
    tiles = tile_rows(B, Ho, Wo, k, plan)
    chains = [np.zeros((Cout, k * k * Cin), dtype=np.float32) for _ in range(FIN_GROUPS)]
    for w in range(plan["wgs"]):
        a = np.zeros((Cout, k * k * Cin), dtype=acc)
        for t in range(w, len(tiles), plan["wgs"]):
            for row in tiles[t]:
                a = (a.astype(np.float64) + d[row].T @ xc[row]).astype(acc)
        chains[w % FIN_GROUPS] = chains[w % FIN_GROUPS] + a.astype(partial).astype(np.float32)
    total = np.zeros((Cout, k * k * Cin), dtype=np.float32)
    for ch in chains:
        total = total + ch
    return np.ascontiguousarray(total.astype(np.float64).reshape(Cout, k, k, Cin).transpose(0, 3, 1, 2))


def colsum_reference(dy, N, dtype=np.float64):
    """(db [N], mag [N]) over the rows of dy [M, ld]."""
    d = dy[:, :N].astype(dtype)
    return d.sum(0), np.abs(d).sum(0)


def colsum_emulate(dy, N, plan, partial=np.float32):
    """Slab by slab: each of the plan's row lanes adds its alternate rows in float32, the lanes are added in order, the slab's sum is stored as `partial`, the
    finalize adds the slabs in float32 in its fixed order (FIN_GROUPS interleaved chains, then the chains)."""
    d = dy[:, :N].astype(np.float32)
    chains = [np.zeros(N, dtype=np.float32) for _ in range(FIN_GROUPS)]
    rp = plan["row_lanes"]
    for s in range(plan["slabs"]):
        slab = d[s * plan["rows"]:(s + 1) * plan["rows"]]
        a = np.zeros(N, dtype=np.float32)
        for lane in range(rp):
            part = np.zeros(N, dtype=np.float32)
            for r in slab[lane::rp]:
                part = part + r
            a = a + part
        chains[s % FIN_GROUPS] = chains[s % FIN_GROUPS] + a.astype(partial).astype(np.float32)
    total = np.zeros(N, dtype=np.float32)
    for ch in chains:
        total = total + ch
    return total.astype(np.float64)


def int_case(B, H, W, Cx, Cy, k, stride, seed):
    """fp16-exact integer data in [-3, 3] for every channel, the pad channels included (so that they are non-zero garbage where Cin < Cx or Cout < Cy)."""
    rng = np.random.default_rng(seed)
    p = k // 2
    Ho, Wo = (H + 2 * p - k) // stride + 1, (W + 2 * p - k) // stride + 1
    x = rng.integers(-3, 4, (B, H, W, Cx)).astype(np.float16)
    dy = rng.integers(-3, 4, (B, Ho, Wo, Cy)).astype(np.float16)
    return x, dy


def random_case(B, H, W, Cx, Cy, k, stride, seed):
    """fp16 activations around 1 and gradients around 0.1, each with a spread of half its mean: most products share a sign, so the sum is of the size of its
    magnitude sum and a relative error of the result is visible against the bound (zero-mean data cancels to a few percent of the magnitude sum, and a
    bound in terms of it would then hide an fp16 rounding of the result)"""
    rng = np.random.default_rng(seed)
    p = k // 2
    Ho, Wo = (H + 2 * p - k) // stride + 1, (W + 2 * p - k) // stride + 1
    x = (1.0 + 0.5 * rng.standard_normal((B, H, W, Cx))).astype(np.float16)
    dy = (0.1 * (1.0 + 0.5 * rng.standard_normal((B, Ho, Wo, Cy)))).astype(np.float16)
    return x, dy


BOUND_CASES = [(B, H, W, C) for (B, H, W) in ((2, 40, 40), (3, 20, 40)) for C in (32, 64)]   # 32 -> 32 and 64 -> 64, 3 x 3, stride 1
BOUND_WGS = 8


def plan_of(B, Ho, Wo, Cx, Cy, k, wgs):
    return ag.wgrad_plan(B, Ho, Wo, Cx, Cy, k, wgs)


def random_rows(M, ld, seed):
    """the same kind of data for the column sum: fp16 rows [M, ld] around 0.1"""
    return (0.1 * (1.0 + 0.5 * np.random.default_rng(seed).standard_normal((M, ld)))).astype(np.float16)
