"""CPU: the host side of the data-parallel tissue-head trainer -- the batch split over the ranks (nnunet_train.rank_batch_sizes) against values
computed from the reference's rule, the forced-foreground invariant of the split, the float64 restatement of the per-rank loss (tests/nnunet_ddp_ref.py)
against values recorded from the reference's own modules under a two-rank gloo group (tests/golden/reference_dc_ce_loss_ddp.npz,
scripts/gen_golden_dc_ce_loss_ddp.py), and run_training's epoch reductions and the simultaneous bad-label raise on two gloo ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nnunet_ddp_ref as dref
from ldiffusion_amd import _lib, nnunet_data, nnunet_train

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the split ------------------------------------------------------------------------------------------------------------------------------------
def test_split_table():
    """nnUNetTrainer._set_batch_size_and_oversample's values, and this project's even split where that rule leaves a rank without a sample."""
    rbs = nnunet_train.rank_batch_sizes
    got = rbs(12, 2)
    assert [b for b, _ in got] == [6, 6] and [p for _, p in got] == pytest.approx([0.0, 0.66], abs=1e-12)
    got = rbs(12, 4)
    assert [b for b, _ in got] == [3, 3, 3, 3] and [p for _, p in got] == pytest.approx([0, 0, 0.32, 1.0], abs=1e-12)
    got = rbs(13, 3)
    assert [b for b, _ in got] == [5, 5, 3] and [p for _, p in got] == pytest.approx([0, 1 - (0.67 - 5 / 13) / (5 / 13), 1.0], abs=1e-12)
    assert 0.258 < got[1][1] < 0.259
    assert [b for b, _ in rbs(49, 6)] == [9, 9, 9, 9, 9, 4]
    got = rbs(8, 8)
    assert [b for b, _ in got] == [1] * 8 and [p for _, p in got] == pytest.approx([0, 0, 0, 0, 0, 0.64, 1, 1], abs=1e-12)
    assert [b for b, _ in rbs(12, 8)] == [2, 2, 2, 2, 1, 1, 1, 1]      # the reference's rule: [2, 2, 2, 2, 2, 2, 0, -2]
    assert [b for b, _ in rbs(12, 5)] == [3, 3, 2, 2, 2]               # the reference's rule: [3, 3, 3, 3, 0]
    assert rbs(12, 1) == [(12, pytest.approx(0.33, abs=1e-12))]
    with pytest.raises(ValueError, match="batch size is smaller than the number of GPUs"):
        rbs(3, 4)
    assert "extension" in rbs.__doc__


def test_split_keeps_the_number_of_forced_foreground_samples():
    """For every world up to 8 and every batch from the world size to 49: the ranks' batches sum to the batch, no rank is empty, and the samples in which
    the loaders force foreground (nnunet_data.do_oversample over each rank's indices with its own percentage) are as many as one process forces.
    50 is left out: 50 * 0.67 = 33.5 is a round() tie."""
    for W in range(1, 9):
        for G in range(W, 50):
            split = nnunet_train.rank_batch_sizes(G, W, 0.33)
            assert len(split) == W and sum(b for b, _ in split) == G and min(b for b, _ in split) >= 1, (G, W, split)
            assert all(0.0 <= p <= 1.0 for _, p in split)
            forced = sum(nnunet_data.do_oversample(i, b, p) for b, p in split for i in range(b))
            single = sum(nnunet_data.do_oversample(i, G, 0.33) for i in range(G))
            assert forced == single, (G, W, split, forced, single)


# ---- the per-rank loss against the reference's modules ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "reference_dc_ce_loss_ddp.npz"))


def _case(golden, name):
    n_scales = sum(1 for k in golden.files if k.startswith(f"{name}.rank0.logits"))
    logits = [[torch.from_numpy(golden[f"{name}.rank{r}.logits{i}"].astype(np.float64)) for i in range(n_scales)] for r in range(2)]
    targets = [[torch.from_numpy(golden[f"{name}.rank{r}.target{i}"].astype(np.int64)) for i in range(n_scales)] for r in range(2)]
    return logits, targets, [float(w) for w in golden[f"{name}.weights"]], bool(golden[f"{name}.batch_dice"])


def test_fixture_covers_an_equal_and_an_unequal_split(golden):
    names = [str(c) for c in golden["cases"]]
    assert {int(golden[f"{n}.n_heads"]) for n in names} == {4, 7}
    assert sorted(tuple(int(v) for v in golden[f"{n}.split"]) for n in names if bool(golden[f"{n}.batch_dice"])) == [(2, 2), (3, 1)]
    for n in names:
        assert [golden[f"{n}.rank{r}.logits0"].shape[0] for r in range(2)] == [int(v) for v in golden[f"{n}.split"]]
    assert os.path.getsize(os.path.join(GOLDEN, "reference_dc_ce_loss_ddp.npz")) < 100 * 1024


def _misses(golden, name, variant):
    """Per rank: does `variant` of the restatement miss the fixture's bound, by the value or by a gradient entry?"""
    logits, targets, weights, batch_dice = _case(golden, name)
    out = []
    for r in range(2):
        value, grads = dref.rank_deep_supervision(logits, targets, r, weights, batch_dice, variant)
        want = float(golden[f"{name}.rank{r}.loss"])
        miss = abs(value - want) > dref.fixture_bounds(want, torch.zeros(1), 1.0, 1, 1, 1, 2)[0]
        for i, (g, w) in enumerate(zip(grads, weights)):
            g_ref = torch.from_numpy(golden[f"{name}.rank{r}.grad{i}"].astype(np.float64))
            if w == 0.0:
                assert g is None and not g_ref.any()
                continue
            Br, _, H, W = g.shape
            tol = dref.fixture_bounds(want, g_ref, w, Br, H, W, 2)[1]
            miss = miss or bool(((g - g_ref).abs() > tol).any())
        out.append(miss)
    return out


@pytest.mark.parametrize("name", ["n4_2p2", "n7_3p1", "n4_2p2_sample"])
def test_float64_restatement_against_the_reference_loss_under_two_ranks(golden, name):
    """Value and raw logit gradients of both ranks within the existing fixture test's bound with the Dice factor carried: 16 u max(1, |l|) on the value,
    32 u W w / (B_r H W) + 2^-20 |g| per entry.  (The 3 + 1 case: the reference's own gather cannot run unequal batches; the generator says how it was
    recorded.)"""
    assert _misses(golden, name, "rule") == [False, False]


def test_restatement_tells_the_rule_from_its_neighbours(golden):
    """A cross-entropy averaged over the global batch (on 3 + 1, where the ranks' batches differ), a Dice gradient without the factor W, and Dice
    statistics of the rank alone: each misses the bound on both ranks."""
    assert _misses(golden, "n7_3p1", "global_mean_ce") == [True, True]
    for name in ("n4_2p2", "n7_3p1"):
        assert _misses(golden, name, "no_world_factor") == [True, True]
        assert _misses(golden, name, "local_sums") == [True, True]
    # without batch_dice nothing is gathered: the variants that only touch the gathered term are the rule itself
    assert _misses(golden, "n4_2p2_sample", "no_world_factor") == [False, False] and _misses(golden, "n4_2p2_sample", "local_sums") == [False, False]


# ---- prototypes of the new entry points -------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_and_bound():
    with open(os.path.join(ROOT, "include", "ldiff.h")) as f:
        header = f.read()
    for name in ("ldiff_op_dice_ce_stats", "ldiff_op_dice_ce_from_sums", "ldiff_op_bucket_pack", "ldiff_op_sumsq_ws_bytes", "ldiff_op_sumsq"):
        assert name + "(" in header and name in _lib.SIGNATURES
    from ldiffusion_amd import autograd as ag
    assert ag.dice_ce_nacc(4) == 26 and ag.dice_ce_nacc(11) == 50
    assert ag.sumsq_plan(1) == (ag.SUMSQ_CHAIN, 1) and ag.sumsq_plan(16384) == (ag.SUMSQ_CHAIN, 1) and ag.sumsq_plan(16385) == (ag.SUMSQ_CHAIN, 2)
    assert ag.sumsq_plan(2 ** 20 + 3)[1] == 65


# ---- two gloo ranks: the epoch reductions and the bad-label raise -----------------------------------------------------------------------------------
_WORKER = r"""
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, {root!r})
from ldiffusion_amd import autograd as ag, nnunet_train
dist.init_process_group("gloo")
rank = dist.get_rank()
OUT = {out!r}


class Stub(nnunet_train.Trainer):
    '''run_training and the ddp step's control flow without a device: the steps return numpy values'''
    def __init__(self):
        self.num_epochs, self.current_epoch, self.initial_lr, self._best_ema = 2, 0, 1e-2, None
        self.log = {{"train_losses": [], "val_losses": [], "mean_fg_dice": [], "ema_fg_dice": [], "dice_per_class_or_region": [], "lrs": []}}
        self.ddp, self.group, self._dist, self.world, self.rank = True, None, dist, 2, rank
        self.device, self.n_heads, self._pending, self.saved = torch.device("cpu"), 4, None, []
        self.backward_calls = 0
    def train_step(self, data, targets):
        return float(data)
    def validation_step(self, data, targets):
        return {{"loss": float(data), "tp_hard": np.array([1, 2, 3]) * (rank + 1), "fp_hard": np.array([1, 0, 2]) + rank, "fn_hard": np.array([0, 1, 0]) + 2 * rank}}
    def save_checkpoint(self, filename):
        self.saved.append(os.path.basename(filename))
        open(filename + ".rank%d" % rank, "w").write("x")
    def step_forward(self, data, targets):
        t = torch.zeros((2, ag.dice_ce_nacc(4)), dtype=torch.float64)
        t[:, :24] = 1.0 + rank
        t[1, -1] = float(data)            # the count of labels outside [0, n_heads) of the second graded scale
        self._pending = "stats"
        return t
    def step_backward(self, sums):
        self.backward_calls += 1
        self.sums = sums
        return torch.tensor(0.5 + rank), torch.zeros(4)
    def step_update(self, bucket):
        return True


tr = Stub()
# rank 0 sees losses 1, 2, 3 per epoch, rank 1 sees 10, 20, 30: vstack().mean() = 11; validation losses 4 (rank 0) and 8 (rank 1): mean 6
train = [(1.0 + 9.0 * rank, None), (2.0 + 18.0 * rank, None), (3.0 + 27.0 * rank, None)]
val = [(4.0 + 4.0 * rank, None)]
log = tr.run_training(train, val, OUT, iterations_per_epoch=3, val_iterations=1)
assert log["train_losses"] == [11.0, 11.0], log["train_losses"]
assert log["val_losses"] == [6.0, 6.0], log["val_losses"]
tp, fp, fn = np.array([3, 6, 9]), np.array([3, 1, 5]), np.array([2, 4, 2])     # summed over the two ranks
want = float(np.nanmean(2 * tp / (2 * tp + fp + fn)))
assert abs(log["mean_fg_dice"][0] - want) < 1e-15 and log["mean_fg_dice"][0] == log["mean_fg_dice"][1]
assert tr._best_ema == max(log["ema_fg_dice"]) and tr.current_epoch == 2          # the EMA and the best on every rank
assert (tr.saved[0] == "checkpoint_best.pth" and tr.saved[-1] == "checkpoint_final.pth") if rank == 0 else tr.saved == [], tr.saved
# pooled helpers without a group: one process's values
assert nnunet_train.pooled_train_loss([1.0, 2.0]) == 1.5 and nnunet_train.pooled_validation(val) is val

# the ddp step: a clean step reaches backward with the statistics added in rank order
v = tr._train_step_ddp(0.0, None)
assert tr.backward_calls == 1 and v == 0.5 + rank and torch.equal(tr.sums[:, :24], torch.full((2, 24), 3.0, dtype=torch.float64))
# a bad label on rank 1 only: BOTH ranks raise today's error, before backward, and meet again in the next collective
try:
    tr._train_step_ddp(3.0 * rank, None)
    raise SystemExit("expected ValueError on rank %d" % rank)
except ValueError as e:
    assert "label outside" in str(e)
assert tr.backward_calls == 1 and tr._pending is None
# non-finite statistics on rank 0 only (non-finite logits): the same
try:
    tr._train_step_ddp(float("nan") if rank == 0 else 0.0, None)
    raise SystemExit("expected ValueError on rank %d" % rank)
except ValueError:
    pass
dist.barrier()
dist.destroy_process_group()
open(os.path.join(OUT, "rank%d.ok" % rank), "w").write("ok")
"""


def test_epoch_reductions_and_bad_label_raise_on_two_gloo_ranks(tmp_path):
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT, out=str(tmp_path)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(port), str(script)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=dict(os.environ, OMP_NUM_THREADS="1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert (tmp_path / "rank0.ok").exists() and (tmp_path / "rank1.ok").exists(), r.stdout[-2000:] + r.stderr[-2000:]
    files = sorted(n for n in os.listdir(tmp_path) if n.startswith("checkpoint_"))
    assert files == ["checkpoint_best.pth.rank0", "checkpoint_final.pth.rank0"], files      # only rank 0 writes
