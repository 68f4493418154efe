"""CPU: the host side of the tissue head's training step -- the float64 restatement of nnU-Net's deep-supervision loss (tests/nnunet_train_ref.py) against
values recorded from the reference's own modules (tests/golden/reference_dc_ce_loss.npz, scripts/gen_golden_dc_ce_loss.py), the deep-supervision weights,
the poly schedule, the parameter names with deep supervision on, the ctypes prototypes of the new entry points, and the GPU case tables against the
pass widths of the reduction kernels' finalize loops."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import nnunet_ref
import nnunet_train_ref as ref
from ldiffusion_amd import _lib, nnunet, nnunet_train

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "reference_dc_ce_loss.npz"))


def _case(golden, name):
    n_scales = sum(1 for k in golden.files if k.startswith(name + ".logits"))
    logits = [torch.from_numpy(golden[f"{name}.logits{i}"].astype(np.float64)).requires_grad_(True) for i in range(n_scales)]
    targets = [torch.from_numpy(golden[f"{name}.target{i}"].astype(np.int64)) for i in range(n_scales)]
    return logits, targets, [float(w) for w in golden[f"{name}.weights"]], bool(golden[f"{name}.batch_dice"])


def test_fixture_covers_what_the_gpu_tests_rely_on(golden):
    names = [str(c) for c in golden["cases"]]
    assert {int(golden[f"{n}.n_heads"]) for n in names} == {4, 7}
    assert {bool(golden[f"{n}.batch_dice"]) for n in names} == {True, False}
    assert [golden[f"{names[0]}.logits{i}"].shape[-1] for i in range(4)] == [32, 16, 8, 4] and golden[f"{names[0]}.logits0"].shape[0] == 2
    absent = [n for n in names if any(len(np.unique(golden[f"{n}.target{i}"])) < int(golden[f"{n}.n_heads"]) for i in range(3))]
    assert absent, "no case in which a foreground class is absent from a graded scale's target"


@pytest.mark.parametrize("name", ["n4_batch", "n4_sample", "n7_batch", "n7_sample_absent"])
def test_float64_restatement_against_the_reference_loss(golden, name):
    """Value and logit gradients to fp32 rounding: the reference ran in fp32, so it carries a few u = 2^-24 of the loss (sums of B H W <= 2048 softmax
    values, added pairwise by torch: 16 u asserted) and, per gradient entry, of the gradient's largest term (1 / (B H W) for the cross-entropy,
    dc / sum for the Dice part: 32 u of w / (B H W) + 2^-20 relative asserted).  The zero-weight scale gets no gradient at all."""
    logits, targets, weights, batch_dice = _case(golden, name)
    loss = ref.deep_supervision_loss(logits, targets, weights, batch_dice)
    loss.backward()
    want = float(golden[f"{name}.loss"])
    assert abs(float(loss.detach()) - want) <= 16 * ref.U * max(1.0, abs(want)), (float(loss.detach()), want)
    for i, (l, w) in enumerate(zip(logits, weights)):
        g_ref = torch.from_numpy(golden[f"{name}.grad{i}"].astype(np.float64))
        if w == 0.0:
            assert l.grad is None and not g_ref.any()
            continue
        B, _, H, W = l.shape
        tol = 32 * ref.U * w / (B * H * W) + 2.0 ** -20 * g_ref.abs()
        err = (l.grad - g_ref).abs()
        assert (err <= tol).all(), f"{name} scale {i}: max error {err.max():.3e}, gradient scale {g_ref.abs().max():.3e}"


def test_restatement_distinguishes_the_options(golden):
    logits, targets, weights, batch_dice = _case(golden, "n4_batch")
    base = float(ref.deep_supervision_loss(logits, targets, weights, batch_dice))
    for kw in (dict(do_bg=True), dict(smooth=1.0)):
        assert abs(float(ref.deep_supervision_loss(logits, targets, weights, batch_dice, **kw)) - base) > 1e-4
    assert abs(float(ref.deep_supervision_loss(logits, targets, weights, not batch_dice)) - base) > 1e-4


def test_deep_supervision_weights(golden):
    w = nnunet_train.deep_supervision_weights(4)
    assert np.allclose(w, golden["n4_batch.weights"], rtol=0, atol=1e-15)
    assert w[-1] == 0.0 and abs(sum(w) - 1.0) < 1e-15
    assert nnunet_train.deep_supervision_weights(6) == [float(v) for v in np.array([32, 16, 8, 4, 2, 0]) / 62]
    assert nnunet_train.deep_supervision_weights(1) == [1.0]


def test_poly_schedule():
    n = 500
    assert nnunet_train.poly_lr(0, 1e-2, n) == 1e-2
    assert nnunet_train.poly_lr(1, 1e-2, n) == 1e-2 * (1 - 1 / n) ** 0.9
    assert nnunet_train.poly_lr(n - 1, 1e-2, n) == 1e-2 * (1 - (n - 1) / n) ** 0.9
    assert 0 < nnunet_train.poly_lr(n - 1, 1e-2, n) < nnunet_train.poly_lr(1, 1e-2, n) < 1e-2


def _spec(config="2d_reduced"):
    with open(os.path.join(GOLDEN, "nnunet_plans_2d.json")) as f:
        plans = json.load(f)
    with open(os.path.join(GOLDEN, "nnunet_dataset.json")) as f:
        ds = json.load(f)
    return nnunet.network_spec(plans, config, ds), plans, ds


@pytest.mark.parametrize("config", ["2d_reduced", "2d"])
def test_param_shapes_with_deep_supervision(config):
    """With deep supervision the name set is what a checkpoint's `network_weights` lists, minus its aliases; the default is unchanged."""
    spec, _, _ = _spec(config)
    plain, deep = nnunet.param_shapes(spec), nnunet.param_shapes(spec, deep_supervision=True)
    assert nnunet.param_shapes(spec, deep_supervision=False) == plain
    assert all(deep[k] == v for k, v in plain.items())
    like = nnunet_ref.checkpoint_like(nnunet_ref.synthetic_state_dict(spec, 0), spec)
    canonical = {k: tuple(v.shape) for k, v in like.items() if ".all_modules." not in k and not k.startswith("decoder.encoder.")}
    assert deep == canonical
    n = spec["n_stages"]
    assert [k for k in deep if k.startswith("decoder.seg_layers.") and k.endswith(".weight")] == [f"decoder.seg_layers.{j}.weight" for j in range(n - 1)]
    assert deep["decoder.seg_layers.0.weight"] == (spec["n_heads"], spec["features"][n - 2], 1, 1)
    init = nnunet_train.initial_state_dict(spec, 3)
    assert {k: tuple(v.shape) for k, v in init.items()} == deep
    assert all(not v.any() for k, v in init.items() if k.endswith(".bias")) and all((v == 1).all() for k, v in init.items() if k.endswith(".norm.weight"))


def test_written_folder_is_read_back(tmp_path):
    spec, plans, ds = _spec()
    path = nnunet.write_trained_model_folder(str(tmp_path / "model"), plans, ds)
    sd = nnunet_train.initial_state_dict(spec, 1)
    torch.save({"network_weights": sd, "init_args": {"configuration": "2d_reduced"}, "trainer_name": "nnUNetTrainer", "inference_allowed_mirroring_axes": (0, 1)},
               os.path.join(path, "fold_0", "checkpoint_best.pth"))
    spec2, sd2, axes = nnunet.read_trained_model_folder(path)
    assert spec2 == spec and axes == (0, 1)
    assert set(sd2) == set(nnunet.param_shapes(spec)) and all(torch.equal(sd2[k], sd[k]) for k in sd2)


def _constant(src, name):
    m = re.search(r"constexpr int [^;]*\b" + name + r" = (\d+)", src)
    assert m, f"{name} is no longer a constexpr int"
    return int(m.group(1))


def test_gpu_case_tables_cross_the_finalize_thresholds():
    """Every finalize of the trainer's streaming reductions covers its partials in passes of a fixed width: the GPU case tables must hold cases beyond one
    pass and beyond two, and thread layouts that leave a workgroup ragged.  The widths are read off the kernels (64 slabs a pass in the InstanceNorm
    finalizes; 256 threads in the loss's, the norm's and the column sum's workgroups), the layouts restated in nnunet_train_ref.in_layout and pinned to the
    library's own workspace sizes (host-only calls), so that a change to a constant cannot quietly move the cases back under a threshold."""
    import test_gpu_nnunet_ddp as D
    import test_gpu_nnunet_ignore as G
    import test_gpu_nnunet_train as T
    import test_gpu_wgrad_direct as W
    from ldiffusion_amd import autograd as ag, optim
    lib = _lib.load()
    with open(os.path.join(ROOT, "ldiffusion_amd", "csrc", "kernels_segtrain.hip")) as f:
        src = f.read()
    with open(os.path.join(ROOT, "ldiffusion_amd", "csrc", "kernels_wgrad.hip")) as f:
        wsrc = f.read()
    assert _constant(src, "IN_ROWS") == ref.IN_ROWS and _constant(src, "DCE_PIX") == 4096
    assert (_constant(wsrc, "CS_ROWS"), _constant(wsrc, "CS_MAX_SLABS")) == (256, 1024)
    assert "for (int r = lane; r < R; r += 64)" in src and "slot < Bd * NACC; slot += 256" in src and "e < Bd * NC; e += 256" in src and "w < P; w += 256" in src
    # InstanceNorm + LeakyReLU
    new = T.IN_LANE_SHAPES + T.IN_WRAP_SHAPES
    assert all(s + (0.01,) in T.IN_CASES for s in new)
    lay = {}
    for B, C, H, W_ in T.IN_SHAPES + new:
        l = lay[(B, C, H, W_)] = ref.in_layout(H * W_, C)
        assert lib.ldiff_op_in_train_ws_bytes(B, H * W_, C) == 4 * (2 * B * l["R"] * C + 2 * B * C), (B, C, H, W_)
    assert all(l["R"] <= 64 and 256 % l["C8"] == 0 for s, l in lay.items() if s in T.IN_SHAPES), "the earlier shapes were the ones below every threshold"
    R = sorted(lay[s]["R"] for s in T.IN_WRAP_SHAPES)
    assert 64 < R[0] <= 128 < R[-1], R                                                  # a second pass; a third
    assert any(lay[s]["R"] > 64 and (s[2] * s[3]) % lay[s]["S"] and s[0] > 1 for s in T.IN_WRAP_SHAPES)   # with a ragged last slab, in a batch
    ragged = [lay[s] for s in T.IN_LANE_SHAPES if lay[s]["C8"] <= 256 and 256 % lay[s]["C8"]]
    assert len({l["nrl"] for l in ragged}) >= 3 and all(l["nrl"] * l["G"] < 256 for l in ragged)          # idle threads, three lane counts
    assert any(l["R"] > 1 for l in ragged) and any(s[2] * s[3] < lay[s]["nrl"] for s in T.IN_LANE_SHAPES)   # over several slabs; fewer rows than row lanes
    assert any(lay[s]["C8"] > 256 for s in T.IN_LANE_SHAPES)                                              # a second pass over the channel vectors
    # Dice + cross-entropy: the plain form's table, the ignore form's, and the split entries'
    wraps = [(n, shape[0]) for n, shape, bd, *_ in T.LOSS_CASES if not bd]
    assert all(B * ag.dice_ce_nacc(n) <= 256 and B * 8 * ((n + 7) // 8) <= 256 for n, B in set(wraps) - set(T.LOSS_WRAP_NB))
    for table, ignore in ((wraps, False), ([(n, B) for _, n, B, _, bd in G.WRAP_CASES if not bd], True)):
        slots = [B * ag.dice_ce_nacc(n, n if ignore else None) for n, B in table]
        coefs = [B * 8 * ((n + 7) // 8) for n, B in table]
        assert any(s > 256 and c <= 256 for s, c in zip(slots, coefs)) and any(s > 512 and c > 256 for s, c in zip(slots, coefs)), (slots, coefs)
        assert all(lib.ldiff_op_dice_ce_ignore_nacc(n) == ag.dice_ce_nacc(n, n) for n, _ in table)
    assert {(n, B) for n, B in T.LOSS_WRAP_NB} == {(n, B) for _, n, B, _, _ in G.WRAP_CASES}
    # the gradient norm
    P = [optim.sumsq_plan(n)[1] for n in D.SUMSQ_WRAP]
    assert min(P) > 256 and max(P) > 768 and max(P) % 256, P
    assert all(lib.ldiff_op_sumsq_ws_bytes(n) == 4 * p for n, p in zip(D.SUMSQ_WRAP, P))
    # the slab column sum
    plans = {(M, N): ag.colsum_slabs_plan(M, N) for M, N in W.COLSUM_INT_CASES}
    assert all(lib.ldiff_op_colsum_slabs_ws_bytes(M, N) == p["ws_bytes"] for (M, N), p in plans.items())
    capped = [(M, N) for (M, N), p in plans.items() if -(-M // 256) > 1024]
    assert capped and all(plans[c]["slabs"] == 1024 and plans[c]["rows"] > 256 and M % plans[c]["rows"] for c in capped for M in [c[0]])
    assert any(256 % (N // 8) for M, N in capped) and len({N for M, N in plans if 256 % (N // 8)}) >= 3 and any(N == 2048 for _, N in plans)
    assert (W.COLSUM_CAPPED_M, 24) in plans


def test_prototypes_of_the_new_entry_points():
    """Argument counts and kinds of the ctypes table against the declarations of include/ldiff.h."""
    with open(os.path.join(ROOT, "include", "ldiff.h")) as f:
        header = f.read()
    kinds = {"int": C.c_int, "float": C.c_float, "int64_t": C.c_int64}
    for name in ("ldiff_op_in_train_ws_bytes", "ldiff_op_in_train_fwd", "ldiff_op_in_train_bwd", "ldiff_op_dice_ce_ws_bytes", "ldiff_op_dice_ce",
                 "ldiff_op_sgd_nesterov_multi"):
        m = re.search(r"(\w+)\s+" + name + r"\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/ldiff.h"
        res, args = _lib.SIGNATURES[name]
        assert res is kinds[m.group(1)]
        want = []
        for a in m.group(2).split(","):
            a = a.strip()
            want.append(C.c_void_p if "*" in a else kinds[a.split()[-2] if len(a.split()) > 1 else a])
        assert args == want, f"{name}: {args} against the header's {want}"
    with open(os.path.join(ROOT, "ldiffusion_amd", "csrc", "kernels_segtrain.hip")) as f:
        src = f.read()
    assert "atomicAdd" not in src, "the training kernels reduce through partials in a fixed order"
