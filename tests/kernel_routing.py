"""Which conv / GEMM / attention kernel a launch reaches, through the library's per-launch profiler (ProfScope names, include/ldiff.h
ldiff_prof_*), and the hand-kept inventory of every such kernel the dispatchers can launch.

The library picks a kernel from shape heuristics (plan_conv in csrc/conv_route.hip, launch_attention); a retune of those
heuristics can move a parity case to another kernel without the case failing.  Each kernel case therefore states the kernel it is meant to
test, and `reached()` checks it before the numbers are compared."""
import contextlib

from ldiffusion_amd import _lib

# the matrix-engine kernels this inventory is about, and the two paths of the attention backward (norms, GroupNorm statistics and the
# elementwise kernels are tested bit-exactly elsewhere)
ROUTED_PREFIXES = ("conv3x3<", "igemm<", "gemm_dma<", "gemm_df", "lngemm<", "attn<", "xattn<", "attn_bwd<")


def matrix_kernels(names):
    return {n for n in names if n.startswith(ROUTED_PREFIXES)}


_ACTIVE = []   # name sets of the reached() blocks that are open: an inner block also reports to the outer ones


def _drain():
    got = matrix_kernels(r["name"] for r in _lib.prof_collect())
    for outer in _ACTIVE:
        outer.update(got)


@contextlib.contextmanager
def reached(lib):
    """with reached(lib) as names: <launches>  ->  `names` holds the conv / GEMM / attention kernels the launches ran.

    Profiling is switched off again when the outermost block ends, whatever happens inside: while it is on, the executors run a UNet
    forward eagerly instead of replaying its graph, and later graph-replay tests would no longer test the graph."""
    import torch
    names = set()
    torch.cuda.synchronize()
    if _ACTIVE:
        _drain()
    else:
        lib.ldiff_prof_set_filter(None)
        _lib.prof_collect()                  # drop rows nobody collected
    _ACTIVE.append(names)
    lib.ldiff_prof_enable(1)
    try:
        yield names
    finally:
        try:
            torch.cuda.synchronize()
            _drain()
        finally:
            _ACTIVE.pop()
            if not _ACTIVE:
                lib.ldiff_prof_enable(0)


def check_route(got, expect, what):
    expect = {expect} if isinstance(expect, str) else set(expect)
    assert got == expect, f"{what}: reached {sorted(got)}, the case is meant for {sorted(expect)}"


def _both(*stems):
    return [s + t for s in stems for t in (">", ",gn>")]


# Every profiled conv / GEMM / attention instantiation, grouped by the launcher that runs it (the conv / GEMM ones as plan_conv chooses them).
KERNEL_VARIANTS = {
    # plan_conv -> conv3x3n_selected / conv3x3nt_selected (kernels_conv3x3n.hip): N == 4 stored columns, weights resident in LDS
    "launch_conv3x3n": _both("conv3x3<8x16,n4", "conv3x3<8x16,n3fold"),
    # plan_conv -> conv3x3d_selected (kernels_conv3x3d.hip): GroupNorm + SiLU prologue, or the parity-folded upsample on request
    "launch_conv3x3d": ["conv3x3<16x16d,128,gn>", "conv3x3<16x16d,128,ups>"],
    # plan_conv -> conv3x3p_selected / c3p_bn (kernels_conv3x3p.hip)
    "launch_conv3x3p": ["conv3x3<16x16,64>", "conv3x3<16x16,128>"],
    # plan_conv, otherwise: c3_tile (conv_route.hip) picks 8x16 -> launch_c3w<BN, GN> or 8x8 -> launch_c3<8, 8, BN, GN> and BN
    "launch_conv3x3": _both(*[f"conv3x3<{t},{bn}" for t in ("8x16", "8x8") for bn in (32, 64, 128, 160)]),
    # plan_conv -> gemm_dma_eligible, gemm_dma_tile -> launch_gemm_dma (kernels_gemm.hip)
    "launch_gemm_dma": [f"gemm_dma<{bm},{bn}>" for bm, bn in ((128, 128), (128, 64), (64, 64))],
    # plan_conv -> gemm_dma_eligible and gemm_df_selected -> launch_gemm_df (kernels_gemm_df.hip)
    "launch_gemm_df": ["gemm_df", "gemm_df<geglu>"],
    # plan_conv, otherwise: igemm_tile -> launch_bmn<BM, BN>(fast) -> launch_cfg<BM, BN, FAST, GN> (kernels_igemm.hip)
    "launch_igemm": _both(*[f"igemm<{bm},{bn},{f}" for bm, bn in ((128, 128), (128, 64), (64, 64)) for f in ("fast", "gen")]),
    # ldiff_op_ln_linear -> launch_lngemm (kernels_gemm_ast.hip)
    "launch_lngemm": ["lngemm<320>", "lngemm<320,geglu>"],
    # launch_attention (kernels_attn.hip): xattn_selected, attn_fr40_selected, attn_cfg by head dim, attn_d512_selected, else attn_dsplit
    "launch_attention": ["xattn<short-kv>", "attn<40,fixref>", "attn<32,16>", "attn<32,32>", "attn<64,48>", "attn<64,64>", "attn<96,80>",
                         "attn<96,96>", "attn<128,128>", "attn<160,160>", "attn<512,128q>", "attn<512,512>"],
    # launch_attn_bwd (kernels_bwd.hip): operands staged through LDS when the staging fits and every pitch, stride and pointer is even
    "launch_attn_bwd": ["attn_bwd<staged>", "attn_bwd<direct>"],
}
ALL_VARIANTS = {n for group in KERNEL_VARIANTS.values() for n in group}

# variants no dispatch path can reach: {name: reason}
UNREACHABLE = {}
