"""CPU (-m "not gpu"): the host plan of the batched sliding window (ldiffusion_amd.tiling.window_plan) against tile_origins / pad_to_tile /
maybe_mirror_and_predict, the ctypes mirror of ldiff_window_tiles, and the host twin of the accumulate / finish arithmetic (tests/window_twin.py) against
the reference's own recorded sliding-window output (tests/golden/reference_sliding_window.npz) -- bit for bit, for every chunk size."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import window_twin
from ldiffusion_amd import _lib, tiling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.mark.parametrize("image_hw, tile_hw", [((20, 80), (32, 48)), ((50, 27), (32, 48)), ((20, 27), (32, 48)), ((32, 48), (32, 48)), ((70, 90), (32, 48)),
                                               ((96, 160), (64, 64))])
@pytest.mark.parametrize("step", [1.0, 0.5, 0.3])
def test_window_plan_follows_pad_to_tile_and_tile_origins(image_hw, tile_hw, step):
    plan = tiling.window_plan(image_hw, tile_hw, step, None, 1)
    image = torch.arange(2 * image_hw[0] * image_hw[1], dtype=torch.float32).reshape((2,) + image_hw) + 1.0
    padded, revert = tiling.pad_to_tile(image, tile_hw)
    assert plan.padded_hw == tuple(padded.shape[1:]) and plan.revert == revert and plan.pad == (revert[0].start, revert[1].start)
    assert plan.image_hw == image_hw and plan.tile_hw == tile_hw
    assert torch.equal(padded[(slice(None),) + plan.revert], image)
    assert plan.origins == tiling.tile_origins(plan.padded_hw, tile_hw, step)
    assert all(0 <= y <= plan.padded_hw[0] - tile_hw[0] and 0 <= x <= plan.padded_hw[1] - tile_hw[1] for y, x in plan.origins)
    assert [o for o, n in plan.chunks] == [[o] for o in plan.origins] and all(n == 1 for _, n in plan.chunks)


def test_window_plan_variant_order_is_maybe_mirror_and_predicts():
    assert tiling.mirror_variants(None) == [0]
    assert tiling.mirror_variants((0,)) == [0, 1]
    assert tiling.mirror_variants((1,)) == [0, 2]
    assert tiling.mirror_variants((0, 1)) == [0, 1, 2, 3]
    assert tiling.mirror_variants((1, 0)) == [0, 2, 1, 3]
    # the order in which maybe_mirror_and_predict calls its network: every call's input identifies its flip
    x = torch.arange(2 * 3 * 4, dtype=torch.float32).reshape(1, 2, 3, 4)
    for axes in (None, (0,), (1,), (0, 1), (1, 0)):
        seen = []

        def network(t):
            seen.append(next(m for m in range(4) if torch.equal(t, torch.flip(x, window_twin.flip_dims(m, 2)))))
            return t.clone()
        tiling.maybe_mirror_and_predict(network, x, axes)
        assert seen == tiling.mirror_variants(axes) == tiling.window_plan((3, 4), (3, 4), 0.5, axes, 1).variants, axes
    for bad in ((2,), (0, 0), (), (-1,)):
        with pytest.raises(ValueError, match="mirror_axes"):
            tiling.mirror_variants(bad)


def test_window_plan_chunks_fill_a_short_last_chunk():
    plan = tiling.window_plan((96, 160), (64, 64), 0.5, (0, 1), 4)     # 2 x 4 = 8 tiles: two whole chunks
    assert len(plan.origins) == 8 and [n for _, n in plan.chunks] == [4, 4] and plan.batch == 16
    plan = tiling.window_plan((96, 160), (64, 64), 0.5, (0, 1), 3)     # 3 + 3 + 2: the last chunk repeats its last tile once
    assert [n for _, n in plan.chunks] == [3, 3, 2] and plan.batch == 12
    assert all(len(o) == 3 for o, _ in plan.chunks)
    assert [t for o, n in plan.chunks for t in o[:n]] == plan.origins
    assert plan.chunks[-1][0] == [plan.origins[6], plan.origins[7], plan.origins[7]]
    plan = tiling.window_plan((20, 27), (32, 48), 0.5, (1,), 5)        # one tile in a chunk of five
    assert plan.chunks == [([(0, 0)] * 5, 1)] and plan.batch == 10
    for bad in (0, -1, tiling.WINDOW_MAX_TILES + 1):
        with pytest.raises(ValueError, match="batch_tiles"):
            tiling.window_plan((96, 160), (64, 64), 0.5, None, bad)
    assert tiling.window_plan((96, 160), (64, 64), 0.5, None, tiling.WINDOW_MAX_TILES).batch == tiling.WINDOW_MAX_TILES


def test_window_tiles_mirror_has_the_headers_layout(tmp_path):
    """ldiff_window_tiles (a tagged struct of include/ldiff.h, passed by pointer and copied into the kernels' arguments) against _lib.WindowTiles."""
    hdr = open(os.path.join(ROOT, "include", "ldiff.h")).read()
    assert int(re.search(r"#define LDIFF_WINDOW_MAX_TILES (\d+)", hdr).group(1)) == _lib.WINDOW_MAX_TILES == tiling.WINDOW_MAX_TILES
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ldiff.h"', 'int main(void) {', '  printf(". %zu\\n", sizeof(ldiff_window_tiles));']
    lines += [f'  printf("{f[0]} %zu\\n", offsetof(ldiff_window_tiles, {f[0]}));' for f in _lib.WindowTiles._fields_]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["  return 0;", "}"]))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)
    got = dict((l.split()[0], int(l.split()[1])) for l in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert got["."] == C.sizeof(_lib.WindowTiles)
    for name, _ in _lib.WindowTiles._fields_:
        assert got[name] == getattr(_lib.WindowTiles, name).offset, name
    t = tiling._window_tiles([(1, 2), (3, 4), (3, 4)], 2, [0, 2])
    assert (t.n_tiles, t.n_valid, t.n_variants, list(t.variants)[:2], list(t.y0)[:3], list(t.x0)[:3]) == (3, 2, 2, [0, 2], [1, 3, 3], [2, 4, 4])
    with pytest.raises(ValueError, match="n_tiles"):
        tiling._window_tiles([(0, 0)] * (tiling.WINDOW_MAX_TILES + 1), 1, [0])


@pytest.mark.parametrize("chunk", [1, 2, "all"])
def test_host_twin_reproduces_the_reference_fixture_bit_for_bit(chunk):
    """The arithmetic statement of ldiff_op_window_accumulate_batch / ldiff_op_window_finish, restated on the host, against the outputs of the reference's
    own predictor code (scripts/gen_golden_sliding_window.py): cases a, b, c with torch.equal, whatever the chunk size."""
    z = np.load(os.path.join(GOLD, "reference_sliding_window.npz"))
    net = window_twin.sw_network(torch.from_numpy(z["head_weight"]))
    for tag in "abc":
        th, tw, step, mm = z[tag + "_cfg"]
        mirror = None if mm < 0 else tuple(i for i in range(2) if (int(mm) >> i) & 1)
        image = torch.from_numpy(z[tag + "_image"])
        n = len(tiling.tile_origins(tuple(image.shape[1:]), (int(th), int(tw)), float(step)))
        acc, cnt, plan = window_twin.accumulate_image(image, net, 4, (int(th), int(tw)), float(step), True, mirror, torch.float16, n if chunk == "all" else chunk)
        got = window_twin.finish(acc, cnt, plan)
        assert got.dtype == torch.float16 and torch.equal(got, torch.from_numpy(z[tag + "_logits_f16"])), tag
    # padded image and the inf case of tests/test_cpu_oracle.py
    small = torch.from_numpy(z["a_image"])[:, :20, :27]
    acc, cnt, plan = window_twin.accumulate_image(small, net, 4, (32, 32), 0.5, True, (0, 1), torch.float16, 1 if chunk == "all" else chunk)
    out = window_twin.finish(acc, cnt, plan)
    assert out.shape == (4, 20, 27) and torch.isfinite(out.float()).all()
    assert torch.equal(out, tiling.predict_sliding_window_return_logits(small, net, 4, (32, 32), 0.5, True, (0, 1)))
    with pytest.raises(RuntimeError, match="inf"):
        window_twin.finish(*window_twin.accumulate_image(torch.full((3, 32, 32), 6e4), lambda x: x[:, :1] * 10.0, 1, (32, 32), 1.0, True, None))


@pytest.mark.parametrize("acc_dtype, pred_dtype", list(itertools.product([torch.float16, torch.float32], repeat=2)))
def test_host_twin_equals_the_per_tile_path_on_the_host(acc_dtype, pred_dtype):
    """All four dtype kinds: the twin's accumulators and logits against predict_sliding_window_return_logits' tensor formulation on the host."""
    g = torch.Generator().manual_seed(5)
    image = torch.randn((3, 40, 52), generator=g)
    W = torch.randn((5, 3), generator=g)

    def network(x):
        return torch.einsum("oc,bchw->bohw", W, x.float()).to(pred_dtype)
    for axes in (None, (0,), (1,), (0, 1)):
        ref = tiling.predict_sliding_window_return_logits(image, network, 5, (32, 32), 0.3, True, axes, acc_dtype)
        for b in (1, 3):
            acc, cnt, plan = window_twin.accumulate_image(image, network, 5, (32, 32), 0.3, True, axes, acc_dtype, b)
            assert torch.equal(window_twin.finish(acc, cnt, plan), ref), (axes, b)


def test_argmax_rule_of_the_twin():
    l = torch.tensor([[[1.0, 2.0, float("nan"), float("inf"), -1.0]], [[1.0, 2.0, 5.0, 0.0, float("-inf")]], [[0.5, 3.0, 0.0, 0.0, -1.0]]])
    assert window_twin.argmax_rule(l).tolist() == [[0, 2, 0, 0, 0]]
    assert torch.equal(window_twin.argmax_rule(l), torch.softmax(l, 0).argmax(0).to(torch.uint8))
