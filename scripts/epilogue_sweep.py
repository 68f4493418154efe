"""Bit-level sweep of the row-group epilogues (csrc/epilogue.h, and the copies the halo-tile conv3x3 kernels and the LDS-DMA GEMM keep): every profiler name of launch_conv3x3, launch_gemm_dma and launch_igemm
(tests/kernel_routing.py KERNEL_VARIANTS) under every epilogue setting the kernel accepts, one line per launch:

    <case> | <kernels reached> | y <CRC32 of the whole output buffer, pad columns and lo half included> | stats <CRC32 of the statistics buffer>

The output and statistics buffers are prefilled with a fixed byte pattern, so a store that strays or is dropped changes a CRC.  A launch the library
refuses prints `refused <status>`.  Only ldiff_op_conv / ldiff_op_conv_stats_blocks are used, so the same file runs against any build of the library:

    python scripts/epilogue_sweep.py [--tree PATH]     # PATH: a checkout with a built libldiff_hip.so (default: this one)

Two builds compute the same epilogue if and only if their outputs are identical line for line (profiles/epilogue_refactor_sweep.txt).

Shapes: small, ragged against the tile in rows (288 rows on 64-row tiles, 12 x 24 pixels on 8 x 16 tiles, ...) and in columns (no column count is a
multiple of 16 except where the tile demands it), one column count with N % 8 == 0 (16-byte stores where the kernel has them) and one with
N % 8 == 4 (8-byte stores) per kernel; the 160-column conv tile exists only for N % 160 == 0 and reaches its 8-byte stores through ldy % 8 == 4.
The LDS-DMA GEMM takes no time embedding, so its cases carry none and it has no `bias+temb` line; an explicit split count moves a 128 x 128 implicit-GEMM launch to the 128 x 64 tile
(igemm_tile); the line names the kernel the launch reached, whatever the case was built for."""
import argparse
import ctypes as C
import os
import sys
import zlib

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
opt = ap.parse_args()
sys.path.insert(0, os.path.join(opt.tree, "tests"))
sys.path.insert(0, opt.tree)

import torch  # noqa: E402

from ldiffusion_amd import _lib  # noqa: E402
from kernel_routing import KERNEL_VARIANTS, reached  # noqa: E402

DEV = "cuda:0"
FILL = 0x5A


def up(x, m):
    return (x + m - 1) // m * m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def crc(t):
    return f"{zlib.crc32(t.cpu().numpy().tobytes()) & 0xffffffff:08x}"


# ---- settings: name -> fields (temb / res / split / stats / f32 / shift / splitk / act / geglu / fold) ----
COMMON = [
    ("bias", {}),
    ("bias+temb", dict(temb=1)),
    ("bias+res", dict(res=1)),
    ("split res+out", dict(res=1, split=1)),
    ("stats", dict(temb=1, res=1, stats=1)),
    ("stats split", dict(res=1, split=1, stats=1)),
    ("f32 out", dict(res=1, f32=1)),
    ("shift3+res", dict(res=1, shift=3)),
    ("shift3 split stats", dict(res=1, split=1, stats=1, shift=3)),
    ("splitk2", dict(temb=1, res=1, splitk=2)),
    ("splitk3", dict(res=1, split=1, splitk=3)),
    ("splitk2 stats", dict(res=1, splitk=2, stats=1)),
    ("splitk3 stats split", dict(temb=1, res=1, split=1, splitk=3, stats=1, shift=3)),
]
GEMM_ONLY = [
    ("act1", dict(act=1)),
    ("act2 split", dict(act=2, split=1)),
    ("geglu", dict(geglu=1)),
    ("fold_gn", dict(fold=1, res=1)),
    ("fold_gn split", dict(fold=1, res=1, split=1)),
]


def configs():
    """(label, family, dict(B, H, W, C, N8, N4, ks, stride, gn, ...)) per profiler name"""
    out = []
    for tile, (H, W) in (("8x16", (12, 24)), ("8x8", (8, 12))):
        for bn, (n8, n4) in ((32, (24, 20)), (64, (56, 52)), (128, (136, 132)), (160, (320, None))):
            for gn in (0, 1):
                out.append((f"conv3x3<{tile},{bn}{',gn' if gn else ''}>", "conv", dict(B=2, H=H, W=W, C=64, Csplit=192, N8=n8, N4=n4, ks=3, stride=1, gn=gn)))
    # LDS-DMA GEMM: rows = B * 32 (so that statistics blocks of 32 rows exist), ragged against the 64- / 128-row tile
    for (bm, bn), B, (n8, n4), ng, fold_bhw in (((128, 128), 94, (2040, 2044), 2048, (24, 8, 16)), ((128, 64), 218, (440, 436), 448, (55, 8, 16)), ((64, 64), 9, (120, 116), 128, (5, 8, 8))):
        out.append((f"gemm_dma<{bm},{bn}>", "gemm", dict(B=B, H=4, W=8, C=64, Csplit=192, N8=n8, N4=n4, Ngeglu=ng, fold_bhw=fold_bhw, ks=1, stride=1, gn=0)))
    # implicit GEMM: 3x3 stride 2 (neither the halo-tile kernels nor the LDS-DMA GEMM take it); gen = channels that are no multiple of 64
    for (bm, bn), B, (n8, n4) in (((128, 128), 94, (2040, 2044)), ((128, 64), 218, (440, 436)), ((64, 64), 9, (120, 116))):
        for path, Cc in (("fast", 64), ("gen", 40)):
            for gn in (0, 1):
                out.append((f"igemm<{bm},{bn},{path}{',gn' if gn else ''}>", "igemm", dict(B=B, H=8, W=16, C=Cc, Csplit=Cc, N8=n8, N4=n4, ks=3, stride=2, gn=gn)))
    return out


def run(lib, label, family, cfg, sname, st, N, ldh, rng_seed):
    """one launch; returns the printed fields"""
    rs = np.random.RandomState(rng_seed)
    B, H, W = cfg["fold_bhw"] if st.get("fold") else (cfg["B"], cfg["H"], cfg["W"])
    ks, stride = cfg["ks"], cfg["stride"]
    Cin = cfg["Csplit"] if st.get("splitk") else cfg["C"]
    if st.get("geglu"):
        N, ldh = cfg["Ngeglu"], cfg["Ngeglu"] // 2 + 8
    Ho, Wo = ((H - 1) // stride + 1, (W - 1) // stride + 1) if ks == 3 else (H, W)
    M, K, Nrows = B * Ho * Wo, ks * ks * Cin, up(N, 16)
    keep = []

    def t(a):
        keep.append(dev(a))
        return keep[-1].data_ptr()

    a = _lib.ConvArgs()
    a.x, a.C1 = t(rs.standard_normal((B, H, W, Cin)).astype(np.float16)), Cin
    a.B, a.Hin, a.Win, a.Hout, a.Wout = B, H, W, Ho, Wo
    a.ks, a.stride, a.pad_t, a.pad_l = ks, stride, ks // 2, ks // 2
    w = np.zeros((Nrows, K), np.float16)
    w[:N] = (rs.standard_normal((N, K)) / np.sqrt(K)).astype(np.float16)
    a.w, a.N, a.Nrows, a.n_real = t(w), N, Nrows, N
    a.gemm_df = -1 if ks == 1 else 0
    bias = np.zeros(Nrows, np.float32)
    bias[:N] = 0.1 * rs.standard_normal(N)
    a.bias = t(bias)
    if cfg["gn"] or st.get("fold"):
        a.gn_scale = t((1.0 + 0.2 * rs.standard_normal((B, Cin))).astype(np.float32))
        a.gn_shift = t((0.2 * rs.standard_normal((B, Cin))).astype(np.float32))
        a.silu_in = 0 if st.get("fold") else 1
    a.fold_gn = 1 if st.get("fold") else 0
    if st.get("temb"):
        a.temb, a.ld_temb = t((0.3 * rs.standard_normal((B, N))).astype(np.float32)), N
    split = bool(st.get("split"))
    ld = 2 * ldh if split else ldh
    if st.get("res"):
        r = np.zeros((M, ld), np.float16)
        r[:, :N] = rs.standard_normal((M, N)).astype(np.float16)
        if split:
            r[:, ldh:ldh + N] = (2.0 ** -12 * rs.standard_normal((M, N))).astype(np.float16)
            a.res_lo = ldh
        a.res, a.ld_res = t(r), ld
    f32 = bool(st.get("f32"))
    y = torch.full((M * ld * (4 if f32 else 2),), FILL, dtype=torch.uint8, device=DEV)
    a.y, a.ldy, a.out_f32 = y.data_ptr(), ld, int(f32)
    if split:
        a.y_lo = ldh
    a.out_shift = st.get("shift", 0)
    a.splitk = st.get("splitk", 0)
    a.act_out = st.get("act", 0)
    a.geglu = st.get("geglu", 0)
    stats = None
    if st.get("stats"):
        R = lib.ldiff_op_conv_stats_blocks(C.byref(a))
        stats = torch.full((B * N * max(R, 1) * 2 * 4,), FILL, dtype=torch.uint8, device=DEV)
        a.stats = stats.data_ptr()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    with reached(lib) as names:
        status = lib.ldiff_op_conv(C.byref(a), stream)
    torch.cuda.synchronize()
    what = f"{label} N={N} ld={ld} {sname}" + (" [temb]" if st.get("temb") and "temb" not in sname else "")
    if status != 0:
        return f"{what} | refused {status}", set()
    return f"{what} | {' '.join(sorted(names))} | y {crc(y)} | stats {crc(stats) if stats is not None else '-'}", names


def main():
    lib = _lib.load()
    torch.cuda.set_device(0)
    seen = set()
    for ci, (label, family, cfg) in enumerate(configs()):
        variants = [(cfg["N8"], cfg["N8"] + 8)]                                                        # 16-byte stores where the kernel has them
        variants.append((cfg["N4"], cfg["N4"] + 4) if cfg["N4"] else (cfg["N8"], cfg["N8"] + 4))       # 8-byte stores
        for vi, (N, ldh) in enumerate(variants):
            for si, (sname, st) in enumerate(COMMON + (GEMM_ONLY if family == "gemm" else [])):
                if family == "gemm":   # the LDS-DMA GEMM takes no time embedding (with one the launch goes to the implicit GEMM): its cases carry none
                    if sname == "bias+temb":
                        continue
                    st = {k: v for k, v in st.items() if k != "temb"}
                line, names = run(lib, label, family, cfg, sname, st, N, ldh, 1000 * ci + 100 * vi + si)
                seen |= names
                print(line, flush=True)
    want = set(KERNEL_VARIANTS["launch_conv3x3"]) | set(KERNEL_VARIANTS["launch_gemm_dma"]) | set(KERNEL_VARIANTS["launch_igemm"])
    print("variants not reached:", " ".join(sorted(want - seen)) or "none")


if __name__ == "__main__":
    main()
