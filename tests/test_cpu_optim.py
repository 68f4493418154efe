"""ldiffusion_amd/optim.py, the host side: the chunk rule of the multi-tensor launches, the dynamic loss-scale rule, the two clip coefficients and the
re-exports that keep `ag.adamw_step`, `train.LOSS_SCALE` and the rest working.  Expected values are written out by hand; the shared object is not loaded."""
import pytest

from ldiffusion_amd import autograd as ag
from ldiffusion_amd import optim, train


def test_chunk_list_is_the_hand_written_list():
    C = optim.ADAMW_CHUNK
    assert C == 16384
    assert optim.chunk_list((1, C, C + 1, 3 * C - 7)) == [(0, 0), (1, 0), (2, 0), (2, C), (3, 0), (3, C), (3, 2 * C)]
    assert optim.chunk_list((0,)) == [] and optim.chunk_list(()) == []
    assert optim.chunk_list((5, 0, 5)) == [(0, 0), (2, 0)]   # a size of 0 contributes no chunk; the tensor index still counts it
    assert optim.chunk_list((10,), chunk=4) == [(0, 0), (0, 4), (0, 8)]


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_update_loss_scale_follows_the_hand_written_trace(bad):
    N = optim.LOSS_SCALE_GROWTH_INTERVAL
    assert (optim.LOSS_SCALE, N) == (1024.0, 200)
    st = {"loss_scale": 1024.0}
    assert optim.update_loss_scale(st, bad) is False
    assert (st["loss_scale"], st["skipped_steps"], st["finite_steps"]) == (512.0, 1, 0)
    for k in range(N - 1):
        assert optim.update_loss_scale(st, 3.5) is True
        assert (st["loss_scale"], st["finite_steps"]) == (512.0, k + 1)
    assert optim.update_loss_scale(st, 3.5) is True
    assert (st["loss_scale"], st["finite_steps"], st["skipped_steps"]) == (1024.0, 0, 1)   # doubled, the counter starts over
    for _ in range(N):
        assert optim.update_loss_scale(st, 0.0) is True
        assert st["loss_scale"] == 1024.0                                                     # the cap
    st = {"loss_scale": 2.0}
    seen = []
    for _ in range(3):
        assert optim.update_loss_scale(st, bad) is False
        seen.append(st["loss_scale"])
    assert seen == [1.0, 1.0, 1.0] and st["skipped_steps"] == 3 and st["finite_steps"] == 0   # the floor
    st = {}
    assert optim.update_loss_scale(st, bad) is False and st == {"loss_scale": 512.0, "skipped_steps": 1, "finite_steps": 0}   # a state without a scale starts at LOSS_SCALE


def test_clip_coefficients_are_the_hand_written_values():
    ds, th = optim.clip_coef_deepspeed, optim.clip_coef_torch
    assert ds(0.5, 1.0) == 1.0 and ds(1.0, 1.0) == 1.0 and ds(4.0, 1.0) == 0.25 and ds(3.0, 12) == 1.0 and ds(48.0, 12) == 0.25
    assert ds(1e30, None) == 1.0 and ds(0.0, None) == 1.0
    assert th(6.0, 12.0) == 1.0 and th(0.0, 12.0) == 1.0
    assert th(12.0, 12.0) == 12.0 / 12.000001 < 1.0               # at the threshold torch's 1e-6 already bites
    assert th(48.0, 12.0) == 12.0 / 48.000001
    assert th(48.0, 12.0) == pytest.approx(0.25, rel=1e-7) and th(1e30, 1e30) == 1.0


def test_moved_names_are_re_exported():
    for name in ("adamw_step", "sgd_nesterov_step", "bucket_pack", "sumsq", "sumsq_plan", "SUMSQ_CHAIN", "ADAMW_CHUNK"):
        assert getattr(ag, name) is getattr(optim, name), name
    for name in ("LOSS_SCALE", "LOSS_SCALE_GROWTH_INTERVAL", "update_loss_scale", "clip_coef_deepspeed"):
        assert getattr(train, name) is getattr(optim, name), name
    from ldiffusion_amd import _lib
    assert ag._sp is _lib.stream_ptr
