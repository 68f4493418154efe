"""CPU: the host side of the cell head's training stage -- the training-mode restatement (tests/resnet_train_ref.py) against torch.nn modules in `.train()`,
cellhead.ema_update against nn.BatchNorm2d, cellhead.instance_targets, the identity-table fact of the training loop's input, the orchestrator's route to
Segmentor.train_cell_model and the rank rule on two gloo ranks."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from torch import nn

import resnet_ref
import resnet_train_ref as tref
from ldiffusion_amd import _lib, cellhead
from test_cpu_cellhead import Classifier

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS, WIDTH, ADAPTER, NCLS = (1, 1, 2, 1), 16, 32, 4


def test_new_entry_points_are_declared_and_bound():
    with open(os.path.join(ROOT, "include", "ldiff.h")) as f:
        header = f.read()
    for name in ("ldiff_op_conv_bn_stats_blocks", "ldiff_op_bn_finalize", "ldiff_op_bn_apply", "ldiff_op_cls_head_feat", "ldiff_resnet_set_train", "ldiff_resnet_bn_channels",
                 "ldiff_resnet_bn_entry", "ldiff_resnet_forward_train"):
        assert name + "(" in header and name in _lib.SIGNATURES
    names = [f[0] for f in _lib.ConvArgs._fields_]
    assert names.index("bn_stats") == names.index("cls_conv") + 1 and names[-1] == "act_out"   # beside its family's fields; the struct's last field stays act_out


def test_bn_layout_of_resnet152():
    layout, T = tref.bn_layout(cellhead.RESNET152_LAYERS, 64)
    assert T == 75712 and len(layout) == 1 + 3 * 50 + 4
    assert layout[0] == ("encoder.1", 0, 64) and layout[1][0] == "encoder.4.0.bn1" and layout[4] == ("encoder.4.0.downsample.1", 64 + 64 + 64 + 256, 256)
    names = {p for p, _, _ in layout}
    shapes = cellhead.param_shapes(NCLS)
    assert names == {k[:-len(".running_mean")] for k in shapes if k.endswith(".running_mean")}


def test_training_restatement_matches_modules_in_train_mode():
    """Two forwards on different batches through the torch.nn statement in .train(): features, running statistics and num_batches_tracked equal the restatement's
    (float64 both; the second forward starts from the first's running statistics)."""
    sd = resnet_ref.synthetic_state_dict(LAYERS, WIDTH, NCLS, 5, adapter_channels=ADAPTER)
    net = Classifier(LAYERS, WIDTH, ADAPTER, NCLS).double()
    net.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
    net.train()
    state = {k: v.clone() for k, v in sd.items()}
    g = torch.Generator().manual_seed(6)
    for step, B in enumerate((3, 5)):
        x = torch.randn((B, 3, 64, 64), generator=g)
        with torch.no_grad():
            want = net(x.double())
        out = tref.forward_train(state, LAYERS, x, torch.float64)
        assert (out["logits"] - want).abs().max().item() <= 1e-10 * want.abs().max().item()
        msd = net.state_dict()
        layout, T = tref.bn_layout(LAYERS, WIDTH)
        for p, o, c in layout:
            for name in ("running_mean", "running_var"):
                assert (out["running"][f"{p}.{name}"] - msd[f"{p}.{name}"]).abs().max().item() <= 1e-12, (p, name)
            assert int(out["running"][f"{p}.num_batches_tracked"]) == int(msd[f"{p}.num_batches_tracked"]) == step + 1
            # the returned batch statistics ARE what moved the running ones: running' = 0.1 batch + 0.9 running
            for name, batch in (("running_mean", out["mean"]), ("running_var", out["var"])):
                ema = 0.1 * batch[o:o + c] + 0.9 * state[f"{p}.{name}"].double()
                assert (ema - msd[f"{p}.{name}"]).abs().max().item() <= 1e-12, (p, name)
        state.update(out["running"])


def test_ema_update_against_batchnorm2d():
    """cellhead.ema_update on the batch statistics of x against what nn.BatchNorm2d's own forward leaves in its buffers (float32).  The mean is torch's bit for
    bit.  The variance differs by how torch sums it in float32: its batch variance is within 64 * 2^-24 relative of the float64 one (a pairwise float32 sum of
    100 values is far inside that), times the momentum, plus one float32 rounding of the result."""
    torch.manual_seed(0)
    bn = nn.BatchNorm2d(16)
    bn.running_mean.normal_()
    bn.running_var.uniform_(0.5, 2.0)
    sd = {f"enc.{k}": v.clone() for k, v in bn.state_dict().items()}
    bn.train()
    for step in range(2):
        x = torch.randn((4, 16, 5, 5)) * 2 + 1
        bn(x)
        mean = x.double().mean((0, 2, 3)).float()
        var = x.double().var((0, 2, 3), unbiased=True).float()
        cellhead.ema_update(sd, [("enc", 0, 16)], mean, var)
        assert sd["enc.running_mean"].dtype == torch.float32 and sd["enc.num_batches_tracked"].dtype == torch.int64
        assert int(sd["enc.num_batches_tracked"]) == int(bn.num_batches_tracked) == step + 1
        assert torch.equal(sd["enc.running_mean"], bn.running_mean)
        tol = 0.1 * 64 * 2.0 ** -24 * var.double() + 2.0 ** -23 * bn.running_var.double().abs()
        assert ((sd["enc.running_var"].double() - bn.running_var.double()).abs() <= tol).all()
        sd["enc.running_var"] = bn.running_var.clone()   # (the next step starts from the same state on both sides)
    sd2 = {"enc.running_mean": torch.zeros(16), "enc.running_var": torch.ones(16)}    # a checkpoint without the counter: it starts at 0
    cellhead.ema_update(sd2, [("enc", 0, 16)], torch.ones(16), torch.ones(16))
    assert int(sd2["enc.num_batches_tracked"]) == 1 and torch.allclose(sd2["enc.running_mean"], torch.full((16,), 0.1))


def test_instance_targets():
    lm = torch.zeros((12, 12), dtype=torch.int64)
    mask = torch.zeros((12, 12), dtype=torch.int64)
    lm[0:5, 0:5] = 3          # 25 pixels: 10 of class 2, 9 of class 1, the rest background -> 2
    mask[0:2, 0:5] = 2
    mask[2, 0:5] = 1
    mask[3, 0:4] = 1
    lm[6:11, 0:5] = 7         # a tie: 5 pixels of class 3, 5 of class 1 -> the lowest class, 1
    mask[6, 0:5] = 3
    mask[7, 0:5] = 1
    lm[0:5, 6:11] = 9         # background only -> -1
    lm[6:11, 6:11] = 12       # class 0 and an out-of-range class only (num_classes = 4): no foreground -> -1
    mask[6:8, 6:11] = 5
    lm[11, 0:3] = 20          # too small an instance: skipped, as instance_boxes skips it
    mask[11, 0:3] = 2
    ids, _ = cellhead.instance_boxes(lm)
    got = cellhead.instance_targets(lm, mask, 4)
    assert ids.tolist() == [3, 7, 9, 12] and got.dtype == torch.int64 and got.tolist() == [2, 1, -1, -1]
    # a mask of another size: nearest-neighbour resize first (model/loss.py:144-145)
    small = mask[::2, ::2].contiguous()
    want = torch.nn.functional.interpolate(small[None, None].float(), size=(12, 12), mode="nearest")[0, 0].long()
    assert cellhead.instance_targets(lm, small, 4).tolist() == cellhead.instance_targets(lm, want, 4).tolist()
    assert cellhead.instance_targets(lm, small, 4).tolist() != [-1, -1, -1, -1]
    assert cellhead.instance_targets(torch.zeros((4, 4), dtype=torch.int64), torch.ones((4, 4), dtype=torch.int64), 4).numel() == 0


def test_identity_table_of_the_training_input():
    """The training loop hands the head the [0, 1] image: `(patch * 255).astype(np.uint8)` of u / 255 is u for every grey level, in numpy's float32."""
    lut = cellhead.build_lut((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    assert lut.shape == (3, 256) and all(np.array_equal(lut[c], np.arange(256, dtype=np.uint8)) for c in range(3))
    u = np.arange(256, dtype=np.uint8)
    assert np.array_equal(((u.astype(np.float32) / 255.0) * 255).astype(np.uint8), u)          # ToTensor's u / 255, then the reference's cast
    assert np.array_equal((((u / 255.0).astype(np.float32)) * 255).astype(np.uint8), u)
    assert not np.array_equal(cellhead.build_lut()[0], u)                                       # the inference side wraps: another table


def _light_segmentor(monkeypatch):
    from ldiffusion_amd.segmentor import Segmentor

    def init(self, train_loader, val_loader, level, num_classes):   # the constructor needs a GPU; the routes under test do not
        self.train_loader, self.val_loader, self.level, self.num_classes = train_loader, val_loader, level, num_classes
    monkeypatch.setattr(Segmentor, "__init__", init)
    return Segmentor


def test_orchestrator_reaches_the_cell_trainer(tmp_path, monkeypatch):
    from ldiffusion_amd.ldiffusion import LDiffusionModel
    Segmentor = _light_segmentor(monkeypatch)
    calls = []

    def model(level):   # (the orchestrator's constructor needs a GPU too; train() reads its level and rank)
        m = LDiffusionModel.__new__(LDiffusionModel)
        m.level, m.rank, m.world_size, m.is_distributed, m.diffusion_path = level, 0, 1, False, str(tmp_path)
        return m

    def record(self, epochs, ldiffusion_weight, diffusion_path, **kw):
        calls.append((self.level, self.num_classes, epochs, ldiffusion_weight, diffusion_path, kw))
        return "cell-folder"

    monkeypatch.setattr(Segmentor, "train_cell_model", record)
    args = SimpleNamespace(num_epochs=13, diffusion_path="sd", num_classes=4)
    fn = lambda image: None   # noqa: E731
    out = model("cell").train(args, component="segmentor", ldiffusion_weight="w", train_loader=[1], val_loader=[2], cell_weights={"a": 1}, instances=fn,
                                                       fit_classifier=False, seed=3)
    assert out == "cell-folder"
    assert calls == [("cell", 4, 3, "w", "sd", dict(cell_weights={"a": 1}, instances=fn, fit_classifier=False, seed=3))]
    with pytest.raises(NotImplementedError, match="cell_weights="):
        model("cell").train(None, component="segmentor", ldiffusion_weight="w")   # raised before anything else is read
    assert len(calls) == 1


_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, {root!r})
from ldiffusion_amd.segmentor import Segmentor
dist.init_process_group("gloo")
rank = dist.get_rank()
OUT = {out!r}
seg = Segmentor.__new__(Segmentor)
seg.train_loader = seg.val_loader = None
seg.level, seg.num_classes = "cell", 4


def trainer(self, epochs, ldiffusion_weight, diffusion_path, **kw):
    open(os.path.join(OUT, "trained.rank%d" % dist.get_rank()), "a").write("x")
    assert kw["cell_weights"] == "ckpt" and kw["fit_classifier"] is True and kw["lr"] == 1e-4 and epochs == 2
    return os.path.join(OUT, "run", "25_01_01")


Segmentor._train_cell_model_rank0 = trainer
got = seg.train_cell_model(2, "w", "sd", cell_weights="ckpt")
assert got == os.path.join(OUT, "run", "25_01_01"), (rank, got)


def failing(self, *a, **k):
    raise ValueError("no instances anywhere")


Segmentor._train_cell_model_rank0 = failing
try:
    seg.train_cell_model(2, "w", "sd", cell_weights="ckpt")
    raise SystemExit("expected RuntimeError on rank %d" % rank)
except RuntimeError as e:
    assert "no instances anywhere" in str(e)
dist.barrier()
dist.destroy_process_group()
open(os.path.join(OUT, "rank%d.ok" % rank), "w").write("ok")
"""


def test_rank_zero_trains_and_every_rank_returns_its_folder(tmp_path):
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
    assert (tmp_path / "trained.rank0").read_text() == "x" and not (tmp_path / "trained.rank1").exists()      # rank 0's trainer ran once, rank 1's never
