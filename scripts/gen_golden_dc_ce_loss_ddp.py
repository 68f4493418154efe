"""Generate tests/golden/reference_dc_ce_loss_ddp.npz by running the REFERENCE's own loss modules under a two-rank gloo group on the CPU:
DeepSupervisionWrapper(DC_and_CE_loss({'batch_dice': .., 'smooth': 1e-5, 'do_bg': False, 'ddp': True}, {}, weight_ce=1, weight_dice=1, ignore_label=None,
dice_class=MemoryEfficientSoftDiceLoss), weights) as nnUNetTrainer._build_loss builds it when `is_ddp` holds (/root/reference/model/nnunetv2/training/
nnUNetTrainer/nnUNetTrainer.py:352-374), the sibling of gen_golden_dc_ce_loss.py (same stubbing of the `nnunetv2` package names).  Recorded PER RANK: the
logits, the targets, the rank's loss and the raw logit gradients as loss.backward() leaves them -- before DistributedDataParallel would average anything.
Only inputs and outputs are committed; /root/reference is never read at test time.

The unequal split: the reference's AllGatherGrad all_gathers the [B_r, classes] rows of every rank into tensors shaped like the caller's own, so it
cannot run with B_0 != B_1 at all (gloo aborts on the size mismatch).  For that case alone this script hands the reference's Dice module a gather that
pads the rows with zeros up to the largest batch and slices the incoming gradient back (`PaddedAllGatherGrad` below): zero rows add nothing to the sums,
and the backward is the same all-reduce of identical rows.  Everything else -- softmax, the sums, the Dice formula, the cross-entropy, the wrapper -- is
the reference's code.

    python scripts/gen_golden_dc_ce_loss_ddp.py            # starts its two ranks itself"""
import importlib.util
import os
import socket
import sys
import tempfile
import types

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/model/nnunetv2"
SCALES = (12, 6, 3)
# (name, n_heads, batch_dice, samples per rank): one equal split and one unequal; without batch_dice the reference gathers nothing
CASES = [("n4_2p2", 4, True, (2, 2)), ("n7_3p1", 7, True, (3, 1)), ("n4_2p2_sample", 4, False, (2, 2))]


class PaddedAllGatherGrad(torch.autograd.Function):
    """ddp_allgather.AllGatherGrad for ranks whose batches differ: rows padded with zeros to the largest batch, the gradient sliced back."""

    @staticmethod
    def forward(ctx, tensor, group=None):
        world = dist.get_world_size()
        rows = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
        dist.all_gather(rows, torch.tensor([tensor.shape[0]]))
        padded = torch.zeros((max(int(r) for r in rows),) + tuple(tensor.shape[1:]), dtype=tensor.dtype)
        padded[:tensor.shape[0]] = tensor
        out = [torch.zeros_like(padded) for _ in range(world)]
        dist.all_gather(out, padded)
        ctx.rows = tensor.shape[0]
        return torch.stack(out, dim=0)

    @staticmethod
    def backward(ctx, *grad_output):
        grad_output = torch.cat(grad_output)
        dist.all_reduce(grad_output, op=dist.ReduceOp.SUM)
        return grad_output[dist.get_rank()][:ctx.rows], None


def _modules():
    for pkg in ["nnunetv2", "nnunetv2.utilities", "nnunetv2.training", "nnunetv2.training.loss"]:
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m

    def load(modname, rel):
        spec = importlib.util.spec_from_file_location(modname, os.path.join(REF, rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[modname] = mod
        spec.loader.exec_module(mod)
        return mod

    load("nnunetv2.utilities.ddp_allgather", "utilities/ddp_allgather.py")
    load("nnunetv2.utilities.helpers", "utilities/helpers.py")
    dice = load("nnunetv2.training.loss.dice", "training/loss/dice.py")
    load("nnunetv2.training.loss.robust_ce_loss", "training/loss/robust_ce_loss.py")
    compound = load("nnunetv2.training.loss.compound_losses", "training/loss/compound_losses.py")
    ds = load("nnunetv2.training.loss.deep_supervision", "training/loss/deep_supervision.py")
    return dice, compound, ds


def weights(n):   # nnUNetTrainer.py:364-372
    w = np.array([1 / (2 ** i) for i in range(n)])
    w[-1] = 0
    return w / w.sum()


def worker(rank, port, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=2)
    dice, compound, ds = _modules()
    out = {}
    reference_gather = dice.AllGatherGrad
    for ci, (name, n, batch_dice, split) in enumerate(CASES):
        g = torch.Generator().manual_seed(500 + 10 * ci + rank)
        B = split[rank]
        dice.AllGatherGrad = reference_gather if len(set(split)) == 1 else PaddedAllGatherGrad
        w = weights(len(SCALES))
        logits = [(2.0 * torch.randn((B, n, s, s), generator=g)).to(torch.float16).float().requires_grad_(True) for s in SCALES]
        targets = [torch.randint(0, n, (B, 1, s, s), generator=g).float() for s in SCALES]
        loss_fn = ds.DeepSupervisionWrapper(compound.DC_and_CE_loss({"batch_dice": batch_dice, "smooth": 1e-5, "do_bg": False, "ddp": True}, {}, weight_ce=1,
                                                                    weight_dice=1, ignore_label=None, dice_class=dice.MemoryEfficientSoftDiceLoss), w)
        value = loss_fn(logits, targets)
        value.backward()
        out[f"{name}.rank{rank}.loss"] = np.float32(value.item())
        for i in range(len(SCALES)):
            out[f"{name}.rank{rank}.logits{i}"] = logits[i].detach().numpy().astype(np.float16)      # exact: the values were rounded to fp16 above
            out[f"{name}.rank{rank}.target{i}"] = targets[i][:, 0].numpy().astype(np.uint8)
            out[f"{name}.rank{rank}.grad{i}"] = (logits[i].grad if logits[i].grad is not None else torch.zeros_like(logits[i])).numpy().astype(np.float32)
        print(name, "rank", rank, "loss", value.item(), flush=True)
    np.savez(os.path.join(tmp, f"rank{rank}.npz"), **out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    with tempfile.TemporaryDirectory() as tmp:
        mp.start_processes(worker, args=(port, tmp), nprocs=2, start_method="spawn")
        out = {"cases": np.array([c[0] for c in CASES])}
        for name, n, batch_dice, split in CASES:
            out[f"{name}.n_heads"] = np.int64(n)
            out[f"{name}.batch_dice"] = np.int64(batch_dice)
            out[f"{name}.weights"] = weights(len(SCALES)).astype(np.float64)
            out[f"{name}.split"] = np.array(split, np.int64)
        for rank in range(2):
            with np.load(os.path.join(tmp, f"rank{rank}.npz")) as part:
                out.update({k: part[k] for k in part.files})
    path = os.path.join(ROOT, "tests", "golden", "reference_dc_ce_loss_ddp.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
