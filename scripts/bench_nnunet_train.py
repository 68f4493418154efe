"""One training step of the nnU-Net tissue head (ldiffusion_amd/nnunet_train.Trainer.train_step) against the same step in torch: the same network as torch.nn
modules with deep supervision under torch.autocast(fp16), the deep-supervision Dice + cross-entropy loss in torch ops, GradScaler, clip_grad_norm_(12) and
torch.optim.SGD(momentum 0.99, nesterov) -- what nnUNetTrainer.train_step runs.  Planner-default width (7 stages, 32 .. 512 features, two convs per stage,
tests/golden/nnunet_plans_2d.json "2d") at 512^2 and the plans' batch size.

The two sides alternate inside one call after a warm-up (device-synchronised wall time per step; median, min, max).  Then one library step runs under
torch.profiler and its device time is split by kernel family (by kernel name).  No threshold is asserted on either number.

--ddp: instead, the plain step against the data-parallel step at world size 1 (`Trainer(ddp=True)` in one process: the loss split at its sums, the
gradient bucket, ldiff_op_sumsq, the SGD launch reading the bucket; the collectives are identities), alternating after two warm-ups.  This prices the
data-parallel path's own launches; it says nothing about scaling.

--route R: a second library trainer with `Trainer(wgrad_route=R)` (autograd.WGRAD_ROUTES) joins the alternation -- default route, route R, torch -- and the
profiled step is R's.  The default route's launches are those of a tree without the route, so this is the before / after of a route on one box in one call.

--ignore: instead, the ignore form of the loss (nnU-Net's ignore label, ag.dice_ce(ignore_label=)) against the plain entry.  First the three loss launches
alone on the full-resolution logits' shape [B, size, size, roundup(n_heads, 8)], device-synchronised wall time over 20 calls, several runs alternating:
plain entry | ignore form on the same fully annotated target | ignore form with about 30 % of the pixels ignored (in blocks).  Then the trainer step,
alternating: Trainer() | Trainer(ignore_label=n_heads) on the same targets | the same with about 30 % ignored.

usage: python scripts/bench_nnunet_train.py [--passes 5] [--size 512] [--batch 0 (= the plans')] [--config 2d] [--ddp] [--route auto-wide] [--ignore]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch import nn  # noqa: E402

from ldiffusion_amd import autograd as ag, nnunet, nnunet_train  # noqa: E402

FAMILIES = [("InstanceNorm + LeakyReLU (in_train)", ("in_partial", "in_apply", "in_fwd_finalize", "in_bwd_finalize")),
            ("Dice + cross-entropy (dice_ce)", ("dce_",)),
            ("SGD (sgd_nesterov_multi)", ("sgd_nesterov",)),
            ("direct weight gradient, narrow and wide entry (wgrad_direct + finalize)", ("wgrad_direct", "wgrad_finalize")),
            ("wgrad staging: im2col_t", ("im2col_t",)),
            ("wgrad staging: transpose of dy", ("transpose_rows",)),
            ("bias gradient: column sums of dy (colsum)", ("colsum",)),
            ("wgrad unpack / weight pack", ("unpack_wgrad", "pack_weight", "pack_fwd", "pack_dgrad")),
            ("conv / GEMM kernels (forward, dgrad and the wgrad GEMM)", ("conv", "gemm", "igemm", "tconv", "splitk"))]


class Block(nn.Sequential):
    def __init__(self, cin, cout, stride):
        super().__init__(nn.Conv2d(cin, cout, 3, stride, 1), nn.InstanceNorm2d(cout, eps=1e-5, affine=True), nn.LeakyReLU(0.01, inplace=True))


class TorchPlainConvUNet(nn.Module):
    """PlainConvUNet with deep supervision as torch.nn modules (the wiring of nnunet_train.TrainableSegNet)."""

    def __init__(self, spec):
        super().__init__()
        f, n = spec["features"], spec["n_stages"]
        self.enc = nn.ModuleList([nn.Sequential(*[Block((spec["in_channels"] if s == 0 else f[s - 1]) if i == 0 else f[s], f[s], spec["strides"][s] if i == 0 else 1)
                                                  for i in range(spec["n_conv_encoder"][s])]) for s in range(n)])
        self.up = nn.ModuleList([nn.ConvTranspose2d(f[n - 1 - j], f[n - 2 - j], 2, 2) for j in range(n - 1)])
        self.dec = nn.ModuleList([nn.Sequential(*[Block(2 * f[n - 2 - j] if i == 0 else f[n - 2 - j], f[n - 2 - j], 1) for i in range(spec["n_conv_decoder"][j])])
                                  for j in range(n - 1)])
        self.heads = nn.ModuleList([nn.Conv2d(f[n - 2 - j], spec["n_heads"], 1) for j in range(n - 1)])

    def forward(self, x):
        skips, outs = [], []
        for st in self.enc:
            x = st(x)
            skips.append(x)
        for j, (up, st) in enumerate(zip(self.up, self.dec)):
            x = st(torch.cat((up(x), skips[-(j + 2)]), 1))
            outs.append(self.heads[j](x))
        return outs[::-1]


def dc_ce_loss(logits, target, batch_dice, smooth=1e-5):
    """DC_and_CE_loss(MemoryEfficientSoftDiceLoss(do_bg=False, smooth, batch_dice), CrossEntropyLoss) in torch ops: logits [B, n, H, W], target [B, H, W]."""
    n = logits.shape[1]
    p = torch.softmax(logits, 1)[:, 1:]
    onehot = F.one_hot(target.long(), n).permute(0, 3, 1, 2)[:, 1:].to(p.dtype)
    intersect, sum_pred, sum_gt = (p * onehot).sum((2, 3)), p.sum((2, 3)), onehot.sum((2, 3))
    if batch_dice:
        intersect, sum_pred, sum_gt = intersect.sum(0), sum_pred.sum(0), sum_gt.sum(0)
    dc = (2 * intersect + smooth) / torch.clip(sum_gt + sum_pred + smooth, 1e-8)
    return F.cross_entropy(logits, target.long()) - dc.mean()


def label_maps(B, n_heads, size, n_scales, seed):
    """Smooth label maps (arg-max over smooth random fields), the lower scales by 2x sub-sampling: highest resolution first."""
    g = torch.Generator().manual_seed(seed)
    top = F.avg_pool2d(torch.randn((B, n_heads, size + 6, size + 6), generator=g), 7, 1).argmax(1)
    return [top[:, ::2 ** i, ::2 ** i].contiguous() for i in range(n_scales)]


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--config", default="2d")
    ap.add_argument("--ddp", action="store_true")
    ap.add_argument("--ignore", action="store_true", help="time the loss's ignore form and a trainer with an ignore label against the plain ones")
    ap.add_argument("--route", default=None, help="also time (and profile) a trainer under this weight-gradient route")
    a = ap.parse_args()
    with open(os.path.join(ROOT, "tests", "golden", "nnunet_plans_2d.json")) as f:
        plans = json.load(f)
    with open(os.path.join(ROOT, "tests", "golden", "nnunet_dataset.json")) as f:
        ds = json.load(f)
    spec = nnunet.network_spec(plans, a.config, ds)
    cfg = nnunet.resolve_configuration(plans, a.config)
    B = a.batch or int(cfg["batch_size"])
    batch_dice = bool(cfg.get("batch_dice", False))
    dev = "cuda:0"
    n_out = spec["n_stages"] - 1
    weights = nnunet_train.deep_supervision_weights(n_out)
    g = torch.Generator().manual_seed(1)
    x = (F.avg_pool2d(torch.randn((B, 3, a.size + 4, a.size + 4), generator=g), 5, 1) * 2.2).to(dev)
    targets = [t.to(dev) for t in label_maps(B, spec["n_heads"], a.size, n_out, 2)]
    tr = nnunet_train.Trainer(spec, nnunet_train.initial_state_dict(spec, 0), batch_dice, 1000, device=dev, configuration=a.config)
    if a.ddp:
        td = nnunet_train.Trainer(spec, nnunet_train.initial_state_dict(spec, 0), batch_dice, 1000, device=dev, configuration=a.config, ddp=True)
        for _ in range(2):
            tr.train_step(x, targets); td.train_step(x, targets)
        tp, tdd = [], []
        for _ in range(a.passes):
            tp.append(timed(lambda: tr.train_step(x, targets)))
            tdd.append(timed(lambda: td.train_step(x, targets)))
        f = lambda v: f"median {statistics.median(v):.1f} ms (min {min(v):.1f}, max {max(v):.1f})"
        print(f"{a.config} B={B} {a.size}^2, {a.passes} alternating steps after 2 warm-ups: plain {f(tp)} | ddp at world 1 {f(tdd)} | ddp / plain = "
              f"{statistics.median(tdd) / statistics.median(tp):.3f}; steps: plain {[round(v, 1) for v in tp]}, ddp {[round(v, 1) for v in tdd]}")
        return
    if a.ignore:
        k = spec["n_heads"]
        f = lambda v: f"median {statistics.median(v):.3f} ms (min {min(v):.3f}, max {max(v):.3f})"
        blocks = (torch.rand((B, a.size // 32, a.size // 32), generator=torch.Generator().manual_seed(3)) < 0.3).to(dev)   # 32 x 32 blocks, about 30 % of them
        partly = [torch.where(blocks.repeat_interleave(32 >> min(i, 5), 1).repeat_interleave(32 >> min(i, 5), 2)[:, :t.shape[1], :t.shape[2]], torch.full_like(t, k), t)
                  for i, t in enumerate(targets)]
        ld = (k + 7) // 8 * 8
        logits = torch.zeros((B, a.size, a.size, ld), dtype=torch.float16, device=dev)
        logits[..., :k] = (2.0 * torch.randn((B, a.size, a.size, k), generator=torch.Generator().manual_seed(4))).to(torch.float16).to(dev)
        t8, p8 = targets[0].to(torch.uint8), partly[0].to(torch.uint8)   # the loader's label maps are uint8
        forms = [("plain entry", t8, None), ("ignore form, nothing ignored", t8, k), (f"ignore form, {float((p8 == k).float().mean()):.2f} ignored", p8, k)]
        calls = 20
        for _, t, ign in forms:
            ag.dice_ce(logits, t, k, batch_dice, 1.0, 1024.0, ignore_label=ign)
        times = {name: [] for name, _, _ in forms}
        for _ in range(a.passes):
            for name, t, ign in forms:
                times[name].append(timed(lambda: [ag.dice_ce(logits, t, k, batch_dice, 1.0, 1024.0, ignore_label=ign) for _ in range(calls)]) / calls)
        print(f"dice_ce B={B} {a.size}^2 n_heads={k} batch_dice={batch_dice}, per call (three launches), {a.passes} alternating runs of {calls} calls: "
              + " | ".join(f"{name} {f(v)}" for name, v in times.items()))
        trainers = [("Trainer()", tr, targets),
                    ("Trainer(ignore_label), nothing ignored", nnunet_train.Trainer(spec, nnunet_train.initial_state_dict(spec, 0), batch_dice, 1000, device=dev,
                                                                                    configuration=a.config, ignore_label=k), targets),
                    ("Trainer(ignore_label), 30 % ignored", nnunet_train.Trainer(spec, nnunet_train.initial_state_dict(spec, 0), batch_dice, 1000, device=dev,
                                                                                 configuration=a.config, ignore_label=k), partly)]
        for _ in range(2):
            for _, t, tg in trainers:
                t.train_step(x, tg)
        steps = {name: [] for name, _, _ in trainers}
        for _ in range(a.passes):
            for name, t, tg in trainers:
                steps[name].append(timed(lambda: t.train_step(x, tg)))
        print(f"{a.config} B={B} {a.size}^2 train_step, {a.passes} alternating steps after 2 warm-ups: " + " | ".join(f"{name} {f(v)}" for name, v in steps.items()))
        return
    tnet = TorchPlainConvUNet(spec).to(dev)
    opt = torch.optim.SGD(tnet.parameters(), 1e-2, weight_decay=3e-5, momentum=0.99, nesterov=True)
    scaler = torch.amp.GradScaler("cuda")

    def run_lib():
        return tr.train_step(x, targets)

    trr = None
    if a.route is not None:
        trr = nnunet_train.Trainer(spec, nnunet_train.initial_state_dict(spec, 0), batch_dice, 1000, device=dev, configuration=a.config, wgrad_route=a.route)

    def run_route():
        return trr.train_step(x, targets)

    def run_torch():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            outs = tnet(x)
            loss = sum(w * dc_ce_loss(o, t, batch_dice) for o, t, w in zip(outs, targets, weights) if w != 0.0)
        scaler.scale(loss).backward()
        scaler.unscale_(opt)
        torch.nn.utils.clip_grad_norm_(tnet.parameters(), 12)
        scaler.step(opt)
        scaler.update()
        return float(loss.detach())

    for _ in range(2):
        run_lib(); run_torch()
        if trr is not None:
            run_route()
    tl, tt, tr_ = [], [], []
    for _ in range(a.passes):
        tl.append(timed(run_lib))
        if trr is not None:
            tr_.append(timed(run_route))
        tt.append(timed(run_torch))
    f = lambda v: f"median {statistics.median(v):.1f} ms (min {min(v):.1f}, max {max(v):.1f})"
    if trr is not None:
        print(f"{a.config} B={B} {a.size}^2, {a.passes} alternating steps: library under --route {a.route} {f(tr_)} | {a.route} / default = "
              f"{statistics.median(tr_) / statistics.median(tl):.3f} | {a.route} / torch = {statistics.median(tr_) / statistics.median(tt):.2f}; steps: default "
              f"{[round(v, 1) for v in tl]}, {a.route} {[round(v, 1) for v in tr_]}, torch {[round(v, 1) for v in tt]}; losses of the last step: default {run_lib():.6f}, "
              f"{a.route} {run_route():.6f}")
    print(f"{a.config} B={B} {a.size}^2, {a.passes} alternating steps: library {f(tl)} | torch.nn under autocast(fp16) + torch.optim.SGD {f(tt)} | "
          f"library / torch = {statistics.median(tl) / statistics.median(tt):.2f}; peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB; "
          f"loss scale {tr.state['loss_scale']:g}, skipped steps {tr.state.get('skipped_steps', 0)}")
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        (run_lib if trr is None else run_route)()
        torch.cuda.synchronize()
    rows = [(e.key, getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0), e.count) for e in prof.key_averages()]
    rows = [r for r in rows if r[1] > 0]
    total = sum(r[1] for r in rows)
    fam = {name: [0.0, 0] for name, _ in FAMILIES}
    fam["torch kernels (concat, permutes, zero-insertion, norms, copies)"] = [0.0, 0]
    for key, us, count in rows:
        low = key.lower()
        name = next((n for n, stems in FAMILIES if any(s in low for s in stems)), "torch kernels (concat, permutes, zero-insertion, norms, copies)")
        fam[name][0] += us
        fam[name][1] += count
    print(f"one library step{'' if trr is None else ' under --route ' + a.route} under torch.profiler: {total / 1e3:.1f} ms of device time in {sum(r[2] for r in rows)} launches")
    for name, (us, count) in sorted(fam.items(), key=lambda kv: -kv[1][0]):
        print(f"  {name:<70} {us / 1e3:9.2f} ms  {us / total * 100:5.1f} %  x{count}")
    print("  largest kernels:")
    for key, us, count in sorted(rows, key=lambda r: -r[1])[:12]:
        print(f"    {key[:90]:<90} {us / 1e3:9.2f} ms  x{count}")


if __name__ == "__main__":
    main()
