"""Plan batch (batch-invariant mode, DESIGN.md "Batch invariance"): what can be checked without a GPU -- the three entry points exist on every layer,
a null handle is an error and not a crash, and parallel.plan_batch is the largest batch any rank submits."""
import os
import re
import subprocess

import pytest

from ldiffusion_amd import _lib, parallel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTERS = ["ldiff_unet_set_plan_batch", "ldiff_vae_set_plan_batch", "ldiff_controlnet_set_plan_batch"]


def test_entry_points_are_exported_declared_and_bound(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ldiff.h")).read(), flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in SETTERS + ["ldiff_op_conv_pb", "ldiff_op_attention_pb", "ldiff_op_gn_stats_pb"]:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared in include/ldiff.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.py"
        assert re.search(r"\sT\s+" + name + r"$", exported, flags=re.M), f"{name} is not exported by the built library"
        assert hasattr(lib, name)
    for name in SETTERS:   # (handle, int n) -> status
        assert _lib.SIGNATURES[name] == (_lib.I, [_lib.P, _lib.I])
    # the op-level form is an entry point of its own: ldiff_conv_args keeps its layout for callers built against it
    assert "plan_batch" not in [f[0] for f in _lib.ConvArgs._fields_] and _lib.SIGNATURES["ldiff_op_conv_pb"][1][1] is _lib.I


@pytest.mark.parametrize("name", SETTERS)
def test_null_handle_is_an_error_not_a_crash(lib, name):
    rc = getattr(lib, name)(None, 1)
    assert rc == -1, f"{name}(NULL, 1) returned {rc}"
    assert b"null handle" in lib.ldiff_last_error()
    with pytest.raises(ValueError):
        _lib.check(rc)


def test_plan_batch_is_the_largest_batch_any_rank_submits():
    """Exhaustive over total 0..40, world 1..8, batch {1, 3, 8} against brute force: every rank's shard (shard_range) cut into batches of `batch`."""
    for total in range(41):
        for world in range(1, 9):
            for batch in (1, 3, 8):
                largest = 0
                for rank in range(world):
                    lo, hi = parallel.shard_range(total, rank, world)
                    for start in range(lo, hi, batch):
                        largest = max(largest, min(batch, hi - start))
                assert parallel.plan_batch(total, world, batch) == largest, (total, world, batch)
    for bad in [(-1, 1, 1), (4, 0, 1), (4, 1, 0)]:
        with pytest.raises(ValueError):
            parallel.plan_batch(*bad)
