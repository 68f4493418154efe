"""GPU (-m gpu): the data-parallel step of the nnU-Net tissue head (ldiffusion_amd/nnunet_train.py `Trainer(ddp=...)`; csrc/kernels_segtrain.hip) -- the loss
split at its sums, the gradient bucket and its norm, the three phases driven by hand against two ranks over gloo, the averaged gradient against the
float64 tape, and the training stage on two ranks.  The two-rank cases start fresh child processes that share the one GPU over gloo.

u = 2^-24 as in tests/test_gpu_nnunet_train.py, whose cases, bounds and helpers this file imports.

SUMSQ_WRAP (258 and 776 partials, beyond one pass of the norm's finalize), measured on an MI355X: relative error at most 4.45e-8 and 5.21e-8 against the bound
1.73e-6 of those cases, 0.026 and 0.030 of it (the existing sizes in the same run: at most 4.79e-8)."""
import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nnunet_ddp_ref as dref
import nnunet_train_ref as ref
import test_gpu_nnunet_train as T
from ldiffusion_amd import autograd as ag, nnunet, nnunet_train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = ref.U


# ---- (a) world 1 changes nothing -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i64", [False, True], ids=["u8", "i64"])
@pytest.mark.parametrize("batch_dice", [True, False])
@pytest.mark.parametrize("n,shape", [(4, (2, 4, 4)), (7, (1, 24, 40)), (11, (2, 72, 72)), (4, (11, 15, 13)), (17, (11, 72, 64)), (32, (9, 15, 13))])
def test_stats_then_from_sums_at_world_one_is_dice_ce(lib, n, shape, batch_dice, i64):
    """ag.dice_ce_stats followed by ag.DiceCeSumsFn at world = 1 equals ag.dice_ce / ag.DiceCeFn bit for bit, in the loss and in dlogits: the smallest of
    the existing loss shapes, an odd map, and a map of 5184 pixels (two workgroups an image, no multiple of 4096); and test_gpu_nnunet_train.LOSS_WRAP_NB's
    batches, where without batch_dice the sums table has more than 256 slots (the reduce kernel's later passes) and two of the three more than 256
    coefficients: every row carries its sample's exact histogram."""
    B, H, W = shape
    logits, target = T.loss_case(n, B, H, W, False, 900 + n)
    tgt = (target if i64 else target.to(torch.uint8)).to(DEV)
    weight, scale = 4 / 7, 1024.0
    want_loss, want_dl = ag.dice_ce(logits.to(DEV), tgt, n, batch_dice, weight, scale)
    sums = ag.dice_ce_stats(logits.to(DEV), tgt, n, batch_dice)
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (1 if batch_dice else B, ag.dice_ce_nacc(n))
    loss, dl = ag.dice_ce_from_sums(logits.to(DEV), tgt, n, batch_dice, sums, sums, 1, weight, scale)
    assert torch.equal(loss, want_loss) and torch.equal(dl, want_dl)
    # the statistics are what they claim: the label histogram is exact, no label is out of range
    ld = logits.shape[-1]
    hist = torch.stack([(target == c).sum() if batch_dice else (target == c).flatten(1).sum(1) for c in range(n)], -1).double().reshape(-1, n)
    assert torch.equal(sums[:, 2 * ld:2 * ld + n].cpu(), hist) and not sums[:, -1].any()
    # on the tape
    z1 = logits.to(DEV).requires_grad_(True)
    z2 = logits.to(DEV).requires_grad_(True)
    a = ag.DiceCeFn.apply(z1, tgt, n, batch_dice, weight, scale)
    b = ag.DiceCeSumsFn.apply(z2, tgt, n, batch_dice, sums, sums, 1, weight, scale)
    a.backward()
    b.backward()
    assert torch.equal(a.detach(), b.detach()) and torch.equal(z1.grad, z2.grad)


def test_from_sums_refusals(lib):
    logits, target = T.loss_case(4, 2, 4, 4, False, 1)
    sums = ag.dice_ce_stats(logits.to(DEV), target.to(DEV), 4, False)
    with pytest.raises(ValueError, match="stays local"):
        ag.dice_ce_from_sums(logits.to(DEV), target.to(DEV), 4, False, sums, sums, 2)
    with pytest.raises(ValueError, match="elements"):
        ag.dice_ce_from_sums(logits.to(DEV), target.to(DEV), 4, True, sums, sums, 1)
    bad = target.clone()
    bad[0, 0, 0] = 9
    s = ag.dice_ce_stats(logits.to(DEV), bad.to(DEV), 4, True)
    assert float(s[0, -1]) == 1.0
    loss, dl = ag.dice_ce_from_sums(logits.to(DEV), bad.to(DEV), 4, True, s, s, 1)
    assert math.isnan(float(loss)) and torch.isnan(dl[0, 0, 0, :4]).all() and torch.isfinite(dl[1]).all()


# ---- (b) exchanged statistics ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [(2, 2), (3, 1)], ids=["2+2", "3+1"])
@pytest.mark.parametrize("n,size", [(4, 32), (7, 64), (7, 32), (4, 64)])
def test_exchanged_statistics_against_float64(lib, n, size, split):
    """One batch of 4 in two parts: each part's statistics, added in part order, then from_sums per part with world = 2.  Value and every dlogits element
    within nnunet_ddp_ref.kernel_bounds of the float64 restatement of the rule (pinned to the reference's modules by tests/test_cpu_nnunet_ddp.py); the
    bound rejects a global-mean cross-entropy (3 + 1), a missing factor W, and local instead of global sums."""
    weight, scale = 4 / 7, 1024.0
    logits, target = T.loss_case(n, 4, size, size, False, 700 + n + size)
    cuts = [0, split[0], 4]
    pl = [logits[cuts[q]:cuts[q + 1]].contiguous() for q in range(2)]
    pt = [target[cuts[q]:cuts[q + 1]].contiguous() for q in range(2)]
    stats = [ag.dice_ce_stats(pl[q].to(DEV), pt[q].to(DEV), n, True) for q in range(2)]
    total = stats[0].clone()
    total += stats[1]
    ref_logits = [p[..., :n].double().permute(0, 3, 1, 2).contiguous() for p in pl]
    for r in range(2):
        loss, dl = ag.dice_ce_from_sums(pl[r].to(DEV), pt[r].to(DEV), n, True, total, stats[r], 2, weight, scale)
        loss2, dl2 = ag.dice_ce_from_sums(pl[r].to(DEV), pt[r].to(DEV), n, True, total, stats[r], 2, weight, scale)
        assert torch.equal(loss, loss2) and torch.equal(dl, dl2)
        assert not dl[..., n:].any()
        got = dl[..., :n].double().cpu()
        tol_value, tol_of = dref.kernel_bounds(pl, pt, r, n, weight, scale)

        def off(variant):
            v, g = dref.rank_loss(ref_logits, pt, r, True, variant)
            g = (g * (weight * scale)).permute(0, 2, 3, 1)
            return abs(float(loss) - v), (got - g).abs(), tol_of(g)

        dv, err, tol = off("rule")
        print(f"[ddp loss] n={n} {size}^2 split {split} rank {r}: value off by {dv:.2e} (bound {tol_value:.2e}), gradient at {(err / tol).max():.3f} of its bound")
        assert dv <= tol_value and (err <= tol).all()
        wrong = ["no_world_factor", "local_sums"] + (["global_mean_ce"] if split[0] != split[1] else [])
        for variant in wrong:
            dv, err, tol = off(variant)
            assert dv > tol_value or (err > tol).any(), f"the bounds accept {variant}"


# ---- (c) the bucket and its norm -------------------------------------------------------------------------------------------------------------------
SUMSQ_WRAP = [257 * 16384 + 5, 776 * 16384 - 9]   # 258 and 776 partials: the finalize's `w += 256` loop takes a second pass, and three and a ragged fourth


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "4-bytes-off"])
@pytest.mark.parametrize("n", [1, 255, 4097, 2 ** 20 + 3] + SUMSQ_WRAP)
def test_sumsq_against_float64(lib, n, off):
    """ldiff_op_sumsq against float64, relative bound (chain + partials + 2) u from the kernel's own plan (ag.sumsq_plan): `chain` fp32 roundings into a
    partial of non-negative terms, the partials added in double (counted all the same), the square root and the final rounding.  Two calls give equal
    bits; one inf or NaN gives a non-finite result.
    SUMSQ_WRAP, where that count of the double adds would leave the bound too loose to tell anything: (chain + 2) 2^-24 + partials 2^-53.  A partial is a sum
    of non-negative terms through `chain` fp32 roundings: within chain u of itself (first order); the partials are non-negative and added in double,
    2^-53 a step; the square root halves a relative error; one unit each for the square root and the rounding to fp32.  That bound rejects the norm without
    partial 256 (the first of the finalize's second pass), and a bad value inside that partial and inside the last one reaches the result."""
    g = torch.Generator().manual_seed(n + off)
    base = (torch.randn(n + off, generator=g) * 37.0).to(DEV)
    x = base[off:]
    assert x.data_ptr() % 16 == 4 * off and x.is_contiguous()
    a, b = ag.sumsq(x), ag.sumsq(x)
    assert a.dtype == torch.float32 and torch.equal(a, b)
    want = float(x.double().square().sum().sqrt())
    chain, partials = ag.sumsq_plan(n)
    assert partials == lib.ldiff_op_sumsq_ws_bytes(n) // 4
    wrap = n in SUMSQ_WRAP
    bound = (chain + 2) * U + partials * 2.0 ** -53 if wrap else (chain + partials + 2) * U
    print(f"[sumsq] n={n} offset {off}: relative error {abs(float(a) - want) / want:.2e}, bound {bound:.2e}")
    assert abs(float(a) - want) <= bound * want
    spots = [n // 2] + ([n - 1] if n > 4 else [])   # in the scalar tail / the last vector as well
    if wrap:
        head = (4 - off) % 4                         # scalar elements up to the first 16-byte boundary; partial w is elements [head + 16384 w, head + 16384 (w + 1))
        last = -(-((n - head) // 4) // (ag.ADAMW_CHUNK // 4)) - 1
        assert last >= 256
        lo = head + 256 * ag.ADAMW_CHUNK
        without = float((x.double().square().sum() - x[lo:lo + ag.ADAMW_CHUNK].double().square().sum()).sqrt())
        assert abs(float(a) - without) > bound * without, "the bound accepts the norm without partial 256"
        spots += [lo + 5, head + last * ag.ADAMW_CHUNK + 1]
    for bad in (float("inf"), float("nan"), float("-inf")):
        for at in spots:
            y = x.clone() if off == 0 else base.clone()[off:]
            y[at] = bad
            assert not math.isfinite(float(ag.sumsq(y)))


def test_bucket_pack_is_torch_cat(lib):
    """Every gradient that is not None, in order, in one launch: tensors of 1, 7, one chunk, one chunk + 1, 3 chunks - 7 and 4 elements, so that later
    tensors start off the 16-byte grid in the bucket, and a source that is itself 4 bytes off."""
    g = torch.Generator().manual_seed(3)
    sizes = [1, 7, 16384, 16385, 3 * 16384 - 7, 4, 2048]
    grads = [torch.randn(s, generator=g).to(DEV) for s in sizes]
    grads[3] = torch.randn(16386, generator=g).to(DEV)[1:]      # a misaligned source
    grads.insert(2, None)
    grads.append(None)
    grads.append(torch.randn((3, 5, 3, 3), generator=g).to(DEV))
    state = {}
    bucket, offsets = ag.bucket_pack(grads, state)
    want = torch.cat([t.reshape(-1) for t in grads if t is not None])
    assert torch.equal(bucket, want) and offsets[-1] == want.numel() and len(offsets) == len([t for t in grads if t is not None]) + 1
    again, _ = ag.bucket_pack(grads, state, out=torch.zeros_like(bucket))
    assert torch.equal(again, want)
    with pytest.raises(ValueError, match="no gradient"):
        ag.bucket_pack([None, None])


# ---- the trainers of (d) - (f) ---------------------------------------------------------------------------------------------------------------------
def _pair_of_halves(seed=7, size=64):
    """A batch of 4 and its halves A, B."""
    plans, ds = T.fixtures()
    spec = nnunet.network_spec(plans, "2d_reduced", ds)
    g = torch.Generator().manual_seed(seed)
    x = F.avg_pool2d(torch.randn((4, 3, size + 4, size + 4), generator=g), 5, 1) * 2.2
    targets = ref.label_maps(4, spec["n_heads"], size, spec["n_stages"] - 1, seed + 1)
    halves = [(x[:2].contiguous(), [t[:2].contiguous() for t in targets]), (x[2:].contiguous(), [t[2:].contiguous() for t in targets])]
    return spec, bool(plans["configurations"]["2d"]["batch_dice"]), x, targets, halves


def _hand_driven_step(trainers, halves):
    """One data-parallel step of len(trainers) ranks in this process, the two collectives by hand: statistics added in rank order, bucket = sum."""
    tables = [tr.step_forward(*h) for tr, h in zip(trainers, halves)]
    sums = tables[0].clone()
    for t in tables[1:]:
        sums += t
    outs = [tr.step_backward(sums) for tr in trainers]
    bucket = outs[0][1].clone()
    for _, b in outs[1:]:
        bucket += b
    ran = [tr.step_update(bucket.clone()) for tr in trainers]
    return [float(o[0]) for o in outs], bucket, ran


# ---- (d) ddp at world 1 equals the plain trainer ---------------------------------------------------------------------------------------------------
def test_ddp_at_world_one_equals_the_plain_trainer(monkeypatch):
    """With the clip threshold out of reach (both coefficients exactly 1) three steps of Trainer(ddp=True) in one process leave parameters and momentum
    buffers bit-equal to the plain Trainer's: the split loss, the bucket and the SGD launch reading the bucket change nothing.  The ungraded lowest head
    has no gradient, no buffer and does not move.  With the real threshold the two gradient norms (ldiff_op_sumsq over the bucket against torch's
    per-tensor norms) agree within test_sumsq_against_float64's bound."""
    monkeypatch.setattr(nnunet_train, "CLIP_NORM", 1e30)
    plain, x, targets, _, _ = T._trainer(num_epochs=10)
    ddp = T._trainer(num_epochs=10, ddp=True)[0]
    assert ddp.ddp and ddp.world == 1 and not plain.ddp
    start = {k: p.detach().clone() for k, p in ddp.network.p.items()}
    la = [plain.train_step(x, targets) for _ in range(3)]
    lb = [ddp.train_step(x, targets) for _ in range(3)]
    assert la == lb and all(math.isfinite(v) for v in la)
    for (k, p), q in zip(plain.network.p.items(), ddp.network.p.values()):
        assert torch.equal(p.detach(), q.detach()), k
    bp, bd = plain.state["sgd"]["momentum_buffer"], ddp.state["sgd"]["momentum_buffer"]
    assert sorted(bp) == sorted(bd) and all(torch.equal(bp[i], bd[i]) for i in bp)
    for i, k in enumerate(ddp.names):
        if k.startswith("decoder.seg_layers.0."):
            assert ddp.params[i].grad is None and i not in bd and torch.equal(ddp.params[i].detach(), start[k])
        else:
            assert i in bd and not torch.equal(ddp.params[i].detach(), start[k])
    monkeypatch.undo()
    plain.train_step(x, targets)
    ddp.train_step(x, targets)
    chain, partials = ag.sumsq_plan(sum(p.numel() for p in ddp.params))
    bound = (chain + partials + 2) * U
    print(f"[ddp world 1] gradient norm: plain {plain.last_grad_norm:.9g}, ddp {ddp.last_grad_norm:.9g}, relative difference "
          f"{abs(plain.last_grad_norm - ddp.last_grad_norm) / plain.last_grad_norm:.2e}, bound {bound:.2e}")
    assert abs(plain.last_grad_norm - ddp.last_grad_norm) <= bound * plain.last_grad_norm


# ---- (e) two ranks equal the hand-driven step ------------------------------------------------------------------------------------------------------
_STEP_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, {root!r})
sys.path.insert(0, os.path.join({root!r}, "tests"))
import test_gpu_nnunet_ddp as D
from ldiffusion_amd import nnunet_train
dist.init_process_group("gloo")                      # two ranks share cuda:0: gloo moves the CUDA buffers; on a node it is RCCL
rank = dist.get_rank()
spec, batch_dice, x, targets, halves = D._pair_of_halves()
tr = nnunet_train.Trainer(spec, nnunet_train.initial_state_dict(spec, 7), batch_dice, 10, device="cuda:0", configuration="2d_reduced")
assert tr.ddp and tr.world == 2 and tr.rank == rank            # ddp=None follows the launch
losses = [tr.train_step(*halves[rank]) for _ in range(3)]
torch.cuda.synchronize()
out = {{"losses": losses, "params": [p.detach().cpu() for p in tr.params], "bufs": {{i: b.cpu() for i, b in tr.state["sgd"]["momentum_buffer"].items()}}}}
# a loss scale of 2^40 on both ranks: the float16 gradients overflow, both skip, both halve, nothing moves
tr.state["loss_scale"] = 2.0 ** 40
skipped = tr.state.get("skipped_steps", 0)
tr.train_step(*halves[rank])
torch.cuda.synchronize()
out["after_overflow"] = [p.detach().cpu() for p in tr.params]
out["state"] = (tr.state["skipped_steps"] - skipped, tr.state["loss_scale"], tr.state["finite_steps"])
dist.barrier()
dist.destroy_process_group()
torch.save(out, os.path.join({out!r}, "rank%d.pt" % rank))
"""


def _run_two_ranks(tmp_path, text, limit, **extra_env):
    """Two fresh child ranks, each under its own `timeout -k 10`; the exit status is asserted before anything is read."""
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    script = tmp_path / "worker.py"
    script.write_text(text)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(port), "--no-python",
           "timeout", "-k", "10", str(limit), sys.executable, str(script)]
    env = dict(os.environ, OMP_NUM_THREADS="4", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"), **extra_env)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit + 60, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def test_two_ranks_equal_the_hand_driven_step(tmp_path):
    """Three steps of two ddp trainers in this process through the public phases, the collectives done by hand, against two child ranks over gloo running
    `train_step`: both ranks' parameters and momentum buffers are bit-equal to each other and to the hand-driven result, and each rank's losses are its
    hand-driven ones.  Then a loss scale of 2^40 on both ranks: both skip, both halve, nothing moves."""
    spec, batch_dice, x, targets, halves = _pair_of_halves()
    trainers = [nnunet_train.Trainer(spec, nnunet_train.initial_state_dict(spec, 7), batch_dice, 10, device=DEV, configuration="2d_reduced", ddp=True)
                for _ in range(2)]
    for tr in trainers:
        tr.world = 2      # the collectives are this test's
    hand = [_hand_driven_step(trainers, halves) for _ in range(3)]
    assert all(all(ran) for _, _, ran in hand)
    for p, q in zip(trainers[0].params, trainers[1].params):
        assert torch.equal(p.detach(), q.detach())
    _run_two_ranks(tmp_path, _STEP_WORKER.format(root=ROOT, out=str(tmp_path)), 150)
    got = [torch.load(tmp_path / f"rank{r}.pt", weights_only=False) for r in range(2)]
    for r in range(2):
        assert got[r]["losses"] == [h[0][r] for h in hand], (r, got[r]["losses"], [h[0][r] for h in hand])
        for k, p, q in zip(trainers[0].names, trainers[0].params, got[r]["params"]):
            assert torch.equal(p.detach().cpu(), q), f"rank {r}: {k} differs from the hand-driven step"
        bufs = trainers[0].state["sgd"]["momentum_buffer"]
        assert sorted(bufs) == sorted(got[r]["bufs"]) and all(torch.equal(bufs[i].cpu(), got[r]["bufs"][i]) for i in bufs)
        assert got[r]["state"] == (1, 2.0 ** 39, 0)
        assert all(torch.equal(a, b) for a, b in zip(got[r]["params"], got[r]["after_overflow"])), "an overflowing step must leave the parameters bit-unchanged"
    assert all(torch.equal(a, b) for a, b in zip(got[0]["params"], got[1]["params"]))


# ---- (f) the averaged gradient against the float64 tape -------------------------------------------------------------------------------------------
# Measured on the MI355X on step 1 of the hand-driven run of test_two_ranks_equal_the_hand_driven_step ("2d_reduced", He-initialised
# weights of seed 7, sub-batches A and B of 2 x 64^2), per slope: (worst ratio over the graded parameter tensors of the figure of the hand-driven averaged
# gradient to the fp16-storage model's, worst ratio of the absolute errors over the conv.bias tensors), and the same two for the plain Trainer on the
# concatenated batch.  Figures as test_gpu_nnunet_train._check_step takes them.  Asserted: twice the measured ratio, at most M_CAP.
MEASURED_DDP = {1.0: ((1.494, 1.617), (1.659, 1.457)), 0.01: ((1.196, 1.303), (1.239, 1.573))}


def _averaged_gradient_case(slope):
    """Step 1 of test_two_ranks_equal_the_hand_driven_step's hand-driven run -- the same initial weights, the same sub-batches A and B -- with the
    trainers built at `slope` (0.01 is that run itself)."""
    spec, batch_dice, x, targets, halves = _pair_of_halves()
    sd = nnunet_train.initial_state_dict(spec, 7)
    weights = nnunet_train.deep_supervision_weights(spec["n_stages"] - 1)
    assert batch_dice
    trainers = [nnunet_train.Trainer(spec, sd, batch_dice, 10, device=DEV, configuration="2d_reduced", slope=slope, ddp=True, loss_scale=T.LOSS_SCALE)
                for _ in range(2)]
    for tr in trainers:
        tr.world = 2
    tables = [tr.step_forward(*h) for tr, h in zip(trainers, halves)]
    sums = tables[0] + tables[1]
    buckets = [tr.step_backward(sums)[1] for tr in trainers]
    mean = ((buckets[0] + buckets[1]).double() / (2 * T.LOSS_SCALE)).cpu()
    tr = trainers[0]
    ddp_g = {k: None for k in tr.names}
    for j, i in enumerate(tr._live):
        ddp_g[tr.names[i]] = mean[tr._offsets[j]:tr._offsets[j + 1]].view_as(tr.params[i])
    plain = nnunet_train.Trainer(spec, sd, batch_dice, 10, device=DEV, configuration="2d_reduced", slope=slope)
    total = plain.loss(plain.network(x), [t.to(DEV) for t in targets], T.LOSS_SCALE)
    total.backward()
    plain_g = {k: (None if p.grad is None else p.grad.double().cpu() / T.LOSS_SCALE) for k, p in plain.network.p.items()}
    _, g64 = ref.step_gradients(sd, spec, x, targets, weights, batch_dice, slope)
    _, gmod = ref.step_gradients(sd, spec, x, targets, weights, batch_dice, slope, storage16=True, loss_scale=T.LOSS_SCALE)
    return ddp_g, plain_g, g64, gmod


@pytest.mark.parametrize("slope,l2", [(1.0, False), (0.01, True)], ids=["slope1-max", "slope0.01-l2"])
def test_averaged_gradient_against_the_float64_tape(slope, l2):
    """Equal parts make J = (1/W) sum_r CE_r - dice(S) the single-process loss of the concatenated batch, so the hand-driven averaged, unscaled gradient
    of step 1 is graded against nnunet_train_ref.step_gradients on the batch of 4 exactly as _check_step grades the plain trainer: the library's
    figure over the fp16-storage model's per tensor -- slope 1.0 in max terms, slope 0.01 in relative L2, conv biases absolute.

    Measured (MEASURED_DDP): slope 1.0, worst tensor decoder.stages.1.convs.1.norm.bias at 6.264e-04 against the model's 4.192e-04 (1.494 x), conv biases
    1.617 x; the plain Trainer on the concatenated batch 1.659 x and 1.457 x.  Slope 0.01: 1.196 x and 1.303 x; plain 1.239 x and 1.573 x.  The two paths run
    the same kernels on batches of 2 and of 4 and differ by 4e-3 of a tensor's largest entry, the size of either one's error: the figure is a maximum over
    a tensor's entries of fp16-storage noise, and on other weights and data it has been seen near the cap for both paths."""
    ddp_g, plain_g, g64, gmod = _averaged_gradient_case(slope)
    assert all((ddp_g[k] is None) == (g is None) for k, g in g64.items()) and ddp_g["decoder.seg_layers.0.weight"] is None
    figures = []
    for lib_g in (ddp_g, plain_g):
        rows, bias_rows = T._step_figures(dict(f64=g64, lib=lib_g, model=gmod), l2)
        figures.append((rows, bias_rows, max(r[1] / r[2] for r in rows), max(r[1] / r[2] for r in bias_rows)))
    (rows, bias_rows, worst, worst_b), (_, _, p_worst, p_worst_b) = figures
    print(f"[ddp step] slope={slope}: averaged gradient of two ranks: worst ratio {worst:.3f}, conv.bias {worst_b:.3f}; plain Trainer on the batch of 4: "
          f"{p_worst:.3f}, conv.bias {p_worst_b:.3f}")
    measured = MEASURED_DDP[slope][0]
    m, mb = (min(T.M_CAP, 2.0 * v) for v in measured)
    for k, e_lib, e_model in rows:
        assert e_lib <= m * e_model, f"{k}: library {e_lib:.3e}, fp16-storage model {e_model:.3e}: {e_lib / e_model:.2f} x (asserted {m:.2f} x)"
    for k, e_lib, e_model in bias_rows:
        assert e_lib <= mb * e_model, f"{k}: library {e_lib:.3e} absolute, fp16-storage model {e_model:.3e}: {e_lib / e_model:.2f} x (asserted {mb:.2f} x)"


# ---- (g) the stage on two ranks --------------------------------------------------------------------------------------------------------------------
_STAGE_WORKER = r"""
import json, os, sys, torch, torch.distributed as dist
sys.path.insert(0, {root!r})
from ldiffusion_amd.segmentor import Segmentor
dist.init_process_group("gloo")
rank = dist.get_rank()
images, labels = json.load(open(os.path.join({out!r}, "lists.json")))
Segmentor.load_ldiffusion = lambda self, w, p, **k: (None, None, None)       # mixed sizes: no sampler runs
seg = Segmentor(None, None, "tissue", 7)
folder = seg.train_tissue_model_nnUNetv2(1, "weights", "sd", images, labels, images[:2], labels[:2], iterations_per_epoch=2, val_iterations=1, num_foreground_voxels=6e4)
log = seg.training_log
info = dict(folder=folder, loaders=[(l.batch_size, l.oversample, l.seed, l.train) for l in seg.tissue_loaders], train_losses=log["train_losses"],
            val_losses=log["val_losses"], mean_fg_dice=log["mean_fg_dice"])
dist.barrier()
dist.destroy_process_group()
json.dump(info, open(os.path.join({out!r}, "rank%d.json" % rank), "w"))
"""


def test_stage_on_two_ranks(tmp_path):
    """test_gpu_nnunet_prep's end-to-end case as two child ranks: one dataset folder, the single-process plans, rank 1's loaders with its entry of
    rank_batch_sizes and the seeds 2 / 3, one model folder returned by both, pooled logs equal on both, and a checkpoint the inference head reads."""
    import test_gpu_nnunet_prep as P
    from ldiffusion_amd import nnunet_data, nnunet_plan as npl
    images, labels = P._write_dataset(str(tmp_path / "src"))
    (tmp_path / "lists.json").write_text(json.dumps([images, labels]))
    roots = {}
    for name in ("nnUNet_raw", "nnUNet_preprocessed", "nnUNet_results"):
        (tmp_path / name).mkdir()
        roots[name] = str(tmp_path / name)
    _run_two_ranks(tmp_path, _STAGE_WORKER.format(root=ROOT, out=str(tmp_path)), 200, **roots)
    info = [json.loads((tmp_path / f"rank{r}.json").read_text()) for r in range(2)]
    assert os.listdir(tmp_path / "nnUNet_raw") == ["Dataset001_Custom"] and os.listdir(tmp_path / "nnUNet_preprocessed") == ["Dataset001_Custom"]
    folder = str(tmp_path / "nnUNet_results" / "Dataset001_Custom" / "nnUNetTrainer__nnUNetPlans__2d")
    assert info[0]["folder"] == info[1]["folder"] == folder
    pre = tmp_path / "nnUNet_preprocessed" / "Dataset001_Custom"
    files = {n: json.loads((pre / n).read_text()) for n in ("dataset_fingerprint.json", "nnUNetPlans.json", "dataset.json", "splits_final.json")}
    assert json.dumps(files["nnUNetPlans.json"]) == json.dumps(npl.plan_experiment(files["dataset_fingerprint.json"], files["dataset.json"], "Dataset001_Custom"))
    assert files["dataset_fingerprint.json"]["shapes_after_crop"][:2] == [[1, 93, 78], [1, 87, 82]]
    assert files["splits_final.json"] == npl.crossval_splits([f"case_{i:03d}" for i in range(6)])
    split = nnunet_train.rank_batch_sizes(files["nnUNetPlans.json"]["configurations"]["2d"]["batch_size"], 2, nnunet_data.OVERSAMPLE_FOREGROUND)
    for r in range(2):
        (tb, to, ts, tt), (vb, vo, vs, vt) = info[r]["loaders"]
        assert (tb, ts, tt) == (split[r][0], 2 * r, True) and (vb, vs, vt) == (split[r][0], 2 * r + 1, False)
        assert to == pytest.approx(split[r][1], abs=1e-12) and vo == pytest.approx(split[r][1], abs=1e-12)
    for k in ("train_losses", "val_losses", "mean_fg_dice"):
        assert info[0][k] == info[1][k] and len(info[0][k]) == 1 and np.isfinite(info[0][k]).all()
    assert sorted(os.listdir(os.path.join(folder, "fold_0"))) == ["checkpoint_best.pth", "checkpoint_final.pth"]
    head = nnunet.load_trained_model_folder(folder, checkpoint_name="checkpoint_final.pth", device=DEV)
    assert head.spec["n_heads"] == 7
