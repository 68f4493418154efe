"""Training the nnU-Net v2 tissue head on the HIP library: what `Segmentor.train_tissue_model_nnUNetv2` (/root/reference/segmentor.py:163-241) has
nnUNetTrainer do, from a batch to `fold_0/checkpoint_best.pth` -- the file `nnunet.load_trained_model_folder` reads.

Per step (nnUNetTrainer.train_step, nnUNetTrainer.py:883-913):
    outputs = network(data)                       PlainConvUNet with deep supervision: one head per decoder stage          TrainableSegNet
    l = sum_i w_i * DC_and_CE(outputs[i], target[i])   w = 1 / 2^i, the last 0, normalised (:364-372)                      ag.DiceCeFn (ldiff_op_dice_ce)
    scaler.scale(l).backward()                    conv dgrad / wgrad on the forward kernels, InstanceNorm + LeakyReLU backward      ag.Conv2dFn, ag.InstanceNormLReLUFn
    unscale, clip_grad_norm_(12), SGD(0.99, nesterov), scaler.update()                                                      train.finish_step + optim.sgd_nesterov_step
Every contraction, normalisation, activation, loss term and parameter update runs in libldiff_hip.so; torch provides the tape, the channel concat, the
depth-to-space permute behind the transposed conv's GEMM and the global gradient norm.

The trainer takes batches: `data` [B, C, H, W] float32 and `target`, the list the nnU-Net loader supplies, one label map per deep-supervision scale, highest
resolution first; `nnunet_data.PatchLoader` makes them on the device; `Segmentor.train_tissue_model_nnUNetv2` wires planner, stores, loaders and this trainer together.

Data-parallel over a launch's ranks (`Trainer(ddp=...)`; nnUNetTrainer.is_ddp, :86): `rank_batch_sizes` splits the plans' batch, a step is three phases
with two collectives between them --
    step_forward   forward, ag.dice_ce_stats per graded scale            -> all_gather of the [scales, NACC] statistics, added in rank order
    step_backward  ag.DiceCeSumsFn on the summed statistics, backward, optim.bucket_pack   -> all_reduce(SUM) of the flat gradient bucket
    step_update    1 / world folded into the update's device scalar, optim.sumsq for the norm, optim.update_loss_scale, clip coefficient, one SGD launch
-- and `run_training` pools losses and tp / fp / fn over the ranks; rank 0 writes the checkpoints.

Partly annotated labels (`Trainer(ignore_label=k)`, nnU-Net's ignore label: nnUNetTrainer.py:357-359 hands `label_manager.ignore_label` to the loss):
pixels labelled k add nothing to the loss, the gradient or the validation counts (ag.dice_ce(ignore_label=), the ignore form of ldiff_op_dice_ce).
The data-parallel step with an ignore label is NOT built: `Trainer(ddp=True, ignore_label=k)` at a world size above 1 raises NotImplementedError.

Not here: a captured-graph step, ResidualEncoderUNet, region labels.
"""
from __future__ import annotations

import math
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import autograd as ag
from . import metrics, nnunet, optim, train

EPS = 1e-5              # InstanceNorm2d eps (get_network_from_plans: norm_op_kwargs)
SLOPE = 0.01            # LeakyReLU negative_slope, ditto
MOMENTUM = 0.99         # nnUNetTrainer.configure_optimizers (:469-473)
CLIP_NORM = 12.0        # nnUNetTrainer.train_step (:905)
SMOOTH = 1e-5           # nnUNetTrainer._build_loss (:357-359)


def deep_supervision_weights(n: int) -> List[float]:
    """nnUNetTrainer._build_loss (:364-372): 1 / 2^i for the n outputs, the lowest resolution 0, normalised to sum 1."""
    if n < 1:
        raise ValueError("deep_supervision_weights: at least one output")
    w = np.array([1 / (2 ** i) for i in range(n)])
    if n > 1:
        w[-1] = 0
    w = w / w.sum()
    return [float(v) for v in w]


def rank_batch_sizes(global_batch: int, world: int, oversample: float = 0.33):
    """nnUNetTrainer._set_batch_size_and_oversample (:302-347) restated: [(batch_size, oversample_percent)] per rank.  Every rank takes
    ceil(global_batch / world) samples until the batch runs out; a rank whose samples lie wholly below (above) the 1 - oversample mark of the global batch
    forces foreground in none (all) of them, the rank that straddles the mark in the matching fraction of its own.
    This project's extension: the rule leaves ranks with 0 or a negative batch for many worlds (12 over 5, 7 or 8 ranks; the reference would crash
    there).  Where it leaves any rank below 1 the batch is split evenly instead -- the first global_batch mod world ranks take one sample more -- and the
    percentages come from the same interval formula over that split."""
    G, W = int(global_batch), int(world)
    if W < 1:
        raise ValueError(f"rank_batch_sizes: world = {world}")
    if G < W:
        raise ValueError("Cannot run DDP if the batch size is smaller than the number of GPUs... Duh.")
    per = -(-G // W)
    sizes = [per - ((r + 1) * per - G) if (r + 1) * per > G else per for r in range(W)]
    if min(sizes) < 1:
        sizes = [G // W + (1 if r < G % W else 0) for r in range(W)]
    out, low, mark = [], 0, 1 - oversample
    for b in sizes:
        high = low + b
        if high / G < mark:
            pct = 0.0
        elif low / G > mark:
            pct = 1.0
        else:
            pct = 1 - ((mark - low / G) / (high / G - low / G))
        out.append((b, pct))
        low = high
    return out


def poly_lr(epoch: int, initial_lr: float, num_epochs: int, exponent: float = 0.9) -> float:
    """PolyLRScheduler.step (polylr.py:18)."""
    return initial_lr * (1 - epoch / num_epochs) ** exponent


def initial_state_dict(spec: dict, seed: int = 0) -> Dict[str, torch.Tensor]:
    """A fresh network as nnU-Net initialises it (InitWeights_He(1e-2): kaiming_normal_(a = 0.01) on every conv / transposed conv, zero biases; norm
    weights 1, biases 0), from a seeded CPU generator."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in nnunet.param_shapes(spec, deep_supervision=True).items():
        if name.endswith(".norm.weight"):
            sd[name] = torch.ones(shape)
        elif name.endswith(".bias"):
            sd[name] = torch.zeros(shape)
        else:
            fan_in = shape[1] * shape[2] * shape[3]
            sd[name] = torch.randn(shape, generator=g) * math.sqrt(2.0 / ((1 + 0.01 ** 2) * fan_in))
    return sd


class TrainableSegNet(train._Graph):
    """nnU-Net's 2-D PlainConvUNet with deep supervision on the tape: float32 master parameters under the canonical names
    (`nnunet.param_shapes(spec, deep_supervision=True)`), NHWC float16 activations.  `net(x [B, C, H, W] float32)` returns the heads' logits as
    UNetDecoder does with deep supervision on, highest resolution first: n_stages - 1 tensors [B, h, w, roundup(n_heads, 8)] float16 in the layout
    ag.DiceCeFn reads (pad columns zero).  Lower heads missing from `state_dict` (an inference checkpoint cleaned by nnunet.clean_state_dict) start
    from `initial_state_dict`'s values."""

    def __init__(self, spec: dict, state_dict, device="cuda:0", slope: float = SLOPE, wgrad_route: Optional[str] = None):
        """`wgrad_route`: the route of the weight / bias gradients (one of ag.WGRAD_ROUTES); None = "auto"."""
        self.spec = dict(spec)
        self.slope = float(slope)
        if wgrad_route is not None and wgrad_route not in ag.WGRAD_ROUTES:
            raise ValueError(f"wgrad route {wgrad_route!r}: one of {ag.WGRAD_ROUTES}")
        self.wgrad_route = "auto" if wgrad_route is None else wgrad_route
        want = nnunet.param_shapes(spec, deep_supervision=True)
        sd = dict(state_dict)
        unexpected = [k for k in sd if k not in want]
        if unexpected:
            raise ValueError(f"unexpected tensors in the state dict: {unexpected[:5]}")
        fresh = None
        for k, shape in want.items():
            if k not in sd:
                if not k.startswith("decoder.seg_layers."):
                    raise RuntimeError(f"nnU-Net tensor {k} missing from the state dict")
                fresh = fresh if fresh is not None else initial_state_dict(spec)
                sd[k] = fresh[k]
            if tuple(sd[k].shape) != tuple(shape):
                raise ValueError(f"load({k}): shape {list(sd[k].shape)} does not match expected {list(shape)}")
        super().__init__({k: sd[k] for k in want}, device, True)

    def block(self, name, x, stride):
        y = self.conv(name + ".conv", x, stride)
        return ag.InstanceNormLReLUFn.apply(y, self.p[name + ".norm.weight"], self.p[name + ".norm.bias"], EPS, self.slope)

    def tconv(self, name, x):
        """ConvTranspose2d(kernel = stride = 2) as the GEMM tconv2x2_kernel states: y[b, 2i + di, 2j + dj, co] = sum_ci x[b, i, j, ci] W[ci, co, di, dj] + bias[co],
        i.e. a linear layer with the weight viewed as [(di, dj, co), ci], then the 2 x 2 depth-to-space permute; the bias enters once per output pixel."""
        w, b = self.p[name + ".weight"], self.p[name + ".bias"]
        cin, cout = w.shape[0], w.shape[1]
        B, H, W, _ = x.shape
        y = ag.linear(x, w.permute(2, 3, 1, 0).reshape(4 * cout, cin), b.repeat(4))
        return y.view(B, H, W, 2, 2, cout).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * H, 2 * W, cout)

    def __call__(self, x, heads: str = "all"):
        sp = self.spec
        if x.dim() != 4 or x.shape[1] != sp["in_channels"]:
            raise ValueError(f"TrainableSegNet: input must be [B, {sp['in_channels']}, h, w], got {list(x.shape)}")
        div = 1
        for st in sp["strides"]:
            div *= st
        if x.shape[2] % div or x.shape[3] % div:
            raise ValueError(f"TrainableSegNet: input {list(x.shape[2:])} is not divisible by the product of the strides, {div}")
        n = sp["n_stages"]
        # "auto" (the constructor's default): the convs with M = B Ho Wo >= ag.WGRAD_DIRECT_MIN_ROWS take the direct weight gradient and the slab column sum in their
        # backward (the route is kept with each node); a route the caller has stated (ag.wgrad_route, ag.set_wgrad_route) holds instead
        route = ag.wgrad_route(ag.stated_wgrad_route(self.wgrad_route))
        with torch.cuda.device(self.device), route:
            h = train._nhwc16(x.to(self.device, torch.float32))
            skips = []
            for s in range(n):
                for i in range(sp["n_conv_encoder"][s]):
                    h = self.block(f"encoder.stages.{s}.0.convs.{i}", h, sp["strides"][s] if i == 0 else 1)
                skips.append(h)
            outs = []
            for j in range(n - 1):
                up = self.tconv(f"decoder.transpconvs.{j}", h)
                h = torch.cat((up, skips[n - 2 - j]), -1)
                for i in range(sp["n_conv_decoder"][j]):
                    h = self.block(f"decoder.stages.{j}.convs.{i}", h, 1)
                if heads == "all" or j == n - 2:
                    outs.append(self.conv(f"decoder.seg_layers.{j}", h))
        return outs[::-1]

    @torch.no_grad()
    def eval_logits(self, x):
        """The full-resolution head only: [B, n_heads, H, W] float32 (what the network returns with deep supervision off)."""
        out = self(x, heads="top")[0]
        return out[..., :self.spec["n_heads"]].permute(0, 3, 1, 2).float().contiguous()

    def state_dict(self):
        return {k: v.detach().to("cpu").clone() for k, v in self.p.items()}


def _world(dist, group):
    return dist.get_world_size(group) if dist is not None else 1


def pooled_train_loss(losses, dist=None, group=None) -> float:
    """nnUNetTrainer.on_train_epoch_end (:918-921): the mean of the epoch's step losses, under ddp over every rank's
    (`np.vstack(all_gather_object(losses)).mean()`).  `dist` = torch.distributed, or None for one process."""
    losses = np.asarray(losses, dtype=np.float64)
    if _world(dist, group) > 1:
        parts = [None] * dist.get_world_size(group)
        dist.all_gather_object(parts, losses, group=group)
        return float(np.vstack(parts).mean())
    return float(np.mean(losses))


def pooled_validation(val_outputs: List[dict], dist=None, group=None) -> List[dict]:
    """nnUNetTrainer.on_validation_epoch_end under ddp (:1000-1017): tp / fp / fn summed over steps and ranks, the loss the mean over both.  Returns the
    list `Trainer.on_validation_epoch_end` takes: unchanged for one process, one pooled entry under a group."""
    if _world(dist, group) <= 1:
        return val_outputs
    mine = {k: np.sum([o[k] for o in val_outputs], 0) for k in ("tp_hard", "fp_hard", "fn_hard")}
    mine["loss"] = np.asarray([o["loss"] for o in val_outputs], dtype=np.float64)
    parts = [None] * dist.get_world_size(group)
    dist.all_gather_object(parts, mine, group=group)
    out = {k: np.vstack([q[k][None] for q in parts]).sum(0) for k in ("tp_hard", "fp_hard", "fn_hard")}
    out["loss"] = float(np.vstack([q["loss"] for q in parts]).mean())
    return [out]


def _batch(b):
    if isinstance(b, dict):
        return b["data"], b["target"]
    return b[0], b[1]


class _Stream:
    """next() over an iterator, or over an iterable that is started again when it runs out (a list of batches)."""

    def __init__(self, src):
        self.src, self.it = src, iter(src)

    def __next__(self):
        try:
            return next(self.it)
        except StopIteration:
            self.it = iter(self.src)
            return next(self.it)


class Trainer:
    """nnUNetTrainer for the covered architecture.  `spec` = nnunet.network_spec(...); `state_dict` the starting weights (`initial_state_dict`);
    `batch_dice` = the plans' `batch_dice` of the configuration (ConfigurationManager.batch_dice: the 2-D configuration sets it)."""

    def __init__(self, spec: dict, state_dict, batch_dice: bool, num_epochs: int, initial_lr: float = 1e-2, weight_decay: float = 3e-5, device="cuda:0", *,
                 configuration: str = "2d", init_args: Optional[dict] = None, mirror_axes: Optional[Sequence[int]] = (0, 1), loss_scale: Optional[float] = None,
                 slope: float = SLOPE, ddp: Optional[bool] = None, group=None, wgrad_route: Optional[str] = None, ignore_label: Optional[int] = None, region_loss: str = "focal"):
        """A `spec` with `regions` (nnunet.network_spec(accept_regions=True)) trains region labels: one sigmoid head per region, the loss the reference's
        DC_and_Focal_loss (`region_loss="focal"`) or nnU-Net's DC_and_BCE_loss ("bce") on the label map through the spec's membership table, the
        validation counts per region; the ignore label is then the spec's own (max(all labels) + 1).
        `ignore_label`: the dataset's ignore label (spec["ignore_label"] of nnunet.network_spec; it equals n_heads), None for fully annotated labels.
        `ddp`: None follows the launch (a process group of more than one rank: nnUNetTrainer.is_ddp), True / False force it; `group` the process group
        (None: the default one).  ddp at world size 1 is legal: the collectives are identities.  `self.world` is the factor of the Dice gradient and of
        the gradient mean; code that does the two collectives by hand for several trainers in one process sets it to their number."""
        self.spec = dict(spec)
        self.network = TrainableSegNet(spec, state_dict, device, slope, wgrad_route)   # wgrad_route: TrainableSegNet's; None = "auto"
        self.device = self.network.device
        self.batch_dice = bool(batch_dice)
        self.num_epochs, self.initial_lr, self.weight_decay = int(num_epochs), float(initial_lr), float(weight_decay)
        self.n_heads = int(spec["n_heads"])
        self.regions = "regions" in spec
        if region_loss not in ("focal", "bce"):
            raise ValueError(f"Trainer: region_loss {region_loss!r} is neither 'focal' nor 'bce'")
        self.region_loss = region_loss
        if self.regions:
            from . import nnunet
            if ignore_label is not None and ignore_label != spec.get("ignore_label"):
                raise ValueError(f"Trainer: ignore_label {ignore_label} is not the region spec's, {spec.get('ignore_label')} (nnunet.region_spec)")
            ignore_label = spec.get("ignore_label")
            self.region_table = nnunet.region_table_tensor(spec["region_table"], self.device)
        elif ignore_label is not None and int(ignore_label) != self.n_heads:
            raise ValueError(f"Trainer: ignore_label {ignore_label} must be the first value past the classes, n_heads = {self.n_heads} (nnunet.label_spec)")
        self.ignore_label = None if ignore_label is None else int(ignore_label)
        self.weights = deep_supervision_weights(spec["n_stages"] - 1)
        self.names = [k for k, _ in self.network.named_parameters()]
        self.params = self.network.parameters()
        self.state = {"loss_scale": float(loss_scale if loss_scale is not None else train.LOSS_SCALE), "sgd": {}}
        self.current_epoch = 0
        self._best_ema = None
        self.log: Dict[str, list] = {"train_losses": [], "val_losses": [], "mean_fg_dice": [], "ema_fg_dice": [], "dice_per_class_or_region": [], "lrs": []}
        self.init_args = dict(init_args) if init_args is not None else {"configuration": configuration, "fold": 0}
        self.init_args.setdefault("configuration", configuration)
        self.inference_allowed_mirroring_axes = None if mirror_axes is None else tuple(int(a) for a in mirror_axes)
        self._scale_t = torch.ones(1, dtype=torch.float32, device=self.device)
        self._clip_t = torch.ones(1, dtype=torch.float32, device=self.device)
        self.last_grad_norm = None
        self._inv_scale = 1.0
        import torch.distributed as dist
        live = dist.is_available() and dist.is_initialized()
        self.ddp = bool(live and dist.get_world_size(group) > 1) if ddp is None else bool(ddp)
        self.group = group
        self._dist = dist if (self.ddp and live) else None
        self.world = dist.get_world_size(group) if self._dist is not None else 1
        self.rank = dist.get_rank(group) if self._dist is not None else 0
        self._check_ignore_ddp()
        self._pending = None
        self._bucket_state: dict = {}
        self._norm_t = torch.zeros(1, dtype=torch.float32, device=self.device)
        if self._dist is not None and self.world > 1:   # DDP.__init__: everyone starts from rank 0's parameters
            src = dist.get_global_rank(group, 0) if group is not None else 0
            for p in self.params:
                dist.broadcast(p.data, src=src, group=group)

    def _check_ignore_ddp(self):
        """The data-parallel step's ignore form is not built (the Dice statistics of all ranks with each rank's own annotated count); `world` may be
        set after construction by code that does the collectives by hand, so the step's phases ask again."""
        if self.ignore_label is not None and self.ddp and self.world > 1:
            raise NotImplementedError(f"Trainer(ddp=True, ignore_label={self.ignore_label}) at world size {self.world}: the data-parallel step with an "
                                      "ignore label is not built; train on one rank")

    def lr(self, epoch: Optional[int] = None) -> float:
        return poly_lr(self.current_epoch if epoch is None else epoch, self.initial_lr, self.num_epochs)

    def eval_logits(self, x):
        return self.network.eval_logits(x)

    def _targets(self, targets, n):
        if torch.is_tensor(targets):
            targets = [targets]
        if len(targets) < n:
            raise ValueError(f"the loss takes one label map per deep-supervision scale: {n} expected, {len(targets)} given (the loader's job)")
        return list(targets)

    def loss(self, outputs, targets, grad_scale: float = 1.0):
        """DeepSupervisionWrapper(DC_and_CE_loss): sum_i w_i loss_i over the scales whose weight is not 0 (a zero-weight scale is skipped, not multiplied:
        its head receives no gradient at all)."""
        targets = self._targets(targets, len(outputs))
        total = None
        for o, t, w in zip(outputs, targets, self.weights):
            if w == 0.0:
                continue
            if self.regions:
                term = ag.DiceFocalFn.apply(o, t, self.region_table, self.n_heads, self.batch_dice, w, grad_scale, SMOOTH, self.ignore_label is not None,
                                            self.region_loss)
            else:
                term = ag.DiceCeFn.apply(o, t, self.n_heads, self.batch_dice, w, grad_scale, SMOOTH, self.ignore_label)   # the weighted term
            total = term if total is None else total + term
        return total

    def _clipped_sgd(self, grads, norm, lr):
        """The end of both step forms: clip_grad_norm_(CLIP_NORM)'s coefficient from `norm`, the global norm of the UNSCALED gradients, and the update --
        the kernel reads `_scale_t` (1 / scale) and the coefficient as device scalars, the gradients are not rewritten."""
        self.last_grad_norm = norm
        self._clip_t.fill_(optim.clip_coef_torch(norm, CLIP_NORM))
        optim.sgd_nesterov_step(self.params, grads, self.state["sgd"], lr, self.weight_decay, MOMENTUM, self._scale_t, self._clip_t)

    def _update(self, params, grads, opt_state, lr, weight_decay):
        """What follows a finite backward pass of the plain step: train.finish_step has just taken the norm of the scaled gradients for its overflow
        test and left it in the state, so no second pass over the gradients."""
        self._clipped_sgd(grads, float(opt_state["grad_norm"]) * self._inv_scale, lr)

    # ---- the data-parallel step: three phases, the two collectives between them (a test may do those by hand) ----
    def step_forward(self, data, targets) -> torch.Tensor:
        """Phase 1: the forward pass and the loss statistics of every graded scale (weight not 0), highest resolution first.  Returns float64
        [scales, NACC] on the device: per scale sum_pred / intersect / sum_gt per class, the cross-entropy sum and the count of labels outside
        [0, n_heads), over this rank's batch.  The caller adds all ranks' tensors in rank order and hands the sum to `step_backward`."""
        self._check_ignore_ddp()
        for p in self.params:
            p.grad = None
        with torch.cuda.device(self.device):
            outputs = self.network(data)
            self._pending = self._statistics(outputs, self._targets(targets, len(outputs)))
        return self._pending[2]

    def _statistics(self, outputs, targets):
        """(graded scales, their local statistics, the [scales, NACC] table to exchange)"""
        graded = [(o, t, w) for o, t, w in zip(outputs, targets, self.weights) if w != 0.0]
        nacc = ag.dice_focal_nacc(self.n_heads) if self.regions else ag.dice_ce_nacc(self.n_heads, self.ignore_label)
        table = torch.empty((len(graded), nacc), dtype=torch.float64, device=self.device)
        local = []

        def stats(o, t, batch_dice, out=None):
            if self.regions:
                return ag.dice_focal_stats(o, t, self.region_table, self.n_heads, batch_dice, out=out, use_ignore=self.ignore_label is not None,
                                           region_loss=self.region_loss)
            return ag.dice_ce_stats(o, t, self.n_heads, batch_dice, out=out, ignore_label=self.ignore_label)

        for i, (o, t, _) in enumerate(graded):
            if self.batch_dice:
                local.append(stats(o, t, True, table[i]).view(1, nacc))
            else:   # per-sample Dice stays on its rank; the exchanged row carries the bad-label count
                local.append(stats(o, t, False))
                table[i] = local[-1].sum(0)
        return graded, local, table

    def _loss_from_sums(self, graded, local, global_sums, grad_scale):
        total = None
        for i, ((o, t, w), loc) in enumerate(zip(graded, local)):
            if self.regions:
                dsums, world = (global_sums[i], self.world) if self.batch_dice else (loc, 1)
                term = ag.DiceFocalSumsFn.apply(o, t, self.region_table, self.n_heads, self.batch_dice, dsums, loc, world, w, grad_scale, SMOOTH,
                                                self.ignore_label is not None, self.region_loss)
            elif self.batch_dice:
                term = ag.DiceCeSumsFn.apply(o, t, self.n_heads, True, global_sums[i], loc, self.world, w, grad_scale, SMOOTH, self.ignore_label)
            else:
                term = ag.DiceCeSumsFn.apply(o, t, self.n_heads, False, loc, loc, 1, w, grad_scale, SMOOTH, self.ignore_label)
            total = term if total is None else total + term
        return total

    def gather_sums(self, table: torch.Tensor) -> torch.Tensor:
        """Collective 1: all ranks' statistics, added in rank order on every rank (identical bits everywhere)."""
        if self._dist is None or self.world == 1:
            return table
        dist = self._dist
        t = table.cpu() if dist.get_backend(self.group) == "gloo" else table
        parts = [torch.empty_like(t) for _ in range(self.world)]
        dist.all_gather(parts, t, group=self.group)
        total = parts[0].clone()
        for q in parts[1:]:
            total += q
        return total.to(self.device)

    def step_backward(self, global_sums: torch.Tensor):
        """Phase 2: the loss of this rank from the summed statistics (ag.DiceCeSumsFn per graded scale; with `batch_dice` the Dice term is the global
        batch's and its gradient carries the factor world, without it the term stays local), backward at the loss scale, and every gradient packed
        into one flat float32 bucket in one launch.  Returns (loss value as a 0-dim device tensor, bucket)."""
        self._check_ignore_ddp()
        if self._pending is None:
            raise RuntimeError("step_backward: no step_forward is pending")
        graded, local, _ = self._pending
        self._pending = None
        scale = float(self.state["loss_scale"])
        global_sums = global_sums.to(self.device, torch.float64).contiguous()
        with torch.cuda.device(self.device):
            total = self._loss_from_sums(graded, local, global_sums, scale)
            total.backward()
            self._inv_scale = 1.0 / scale
            bucket, self._offsets = optim.bucket_pack([p.grad for p in self.params], self._bucket_state)
        self._live = [i for i, p in enumerate(self.params) if p.grad is not None]
        return total.detach(), bucket

    def reduce_bucket(self, bucket: torch.Tensor) -> torch.Tensor:
        """Collective 2: the sum of all ranks' buckets."""
        if self._dist is not None and self.world > 1:
            self._dist.all_reduce(bucket, group=self.group)
        return bucket

    def step_update(self, bucket: torch.Tensor) -> bool:
        """Phase 3, on the summed bucket (identical bits on every rank, so every rank takes the same branch): the mean over the ranks is the factor
        1 / world in the update's `inv_scale` device scalar and in the norm; the norm (optim.sumsq) of the averaged, unscaled gradient;
        optim.update_loss_scale, as in train.finish_step; `_clipped_sgd`: one SGD launch whose gradient table points into the bucket.  True when the
        update ran."""
        with torch.cuda.device(self.device):
            total = float(optim.sumsq(bucket, self._norm_t))   # of the summed gradients at the loss scale
            self.state["grad_norm"] = total
            if not optim.update_loss_scale(self.state, total):
                return False
            inv = self._inv_scale / self.world
            self._scale_t.fill_(inv)
            grads: list = [None] * len(self.params)
            for j, i in enumerate(self._live):
                grads[i] = bucket[self._offsets[j]:self._offsets[j + 1]].view_as(self.params[i])
            self._clipped_sgd(grads, total * inv, self.lr())
        return True

    def _train_step_ddp(self, data, targets) -> float:
        bad = 3 * 8 * ((self.n_heads + 7) // 8) + 1   # the row's count of labels that are no class (and not the ignore label), in both forms
        sums = self.gather_sums(self.step_forward(data, targets))
        host = sums.cpu()
        if float(host[:, bad].sum()) > 0 or not bool(torch.isfinite(host).all()):   # the gathered count (non-finite logits make the gathered cross-entropy
            # sum non-finite): every rank sees the same tensor, skips the update and raises together -- none is left waiting in a collective
            self._pending = None
            raise ValueError("train_step: the loss is NaN -- a label outside [0, n_heads) (torch's cross_entropy raises there too) or non-finite logits")
        total, bucket = self.step_backward(sums)
        self.step_update(self.reduce_bucket(bucket))
        return float(total)

    def train_step(self, data, targets) -> float:
        """One step; returns the loss.  A non-finite gradient norm (a float16 activation gradient overflowed under the loss scale) skips the update and
        halves the scale, a run of finite steps doubles a lowered scale again: train.finish_step's rule, which this calls.  In ddp mode: the three
        phases and their collectives; the value is this rank's (`run_training` pools them)."""
        if self.ddp:
            return self._train_step_ddp(data, targets)
        for p in self.params:
            p.grad = None
        scale = float(self.state["loss_scale"])
        with torch.cuda.device(self.device):
            outputs = self.network(data)
            total = self.loss(outputs, targets, scale)
            total.backward()
            self._inv_scale = 1.0 / scale
            self._scale_t.fill_(self._inv_scale)
            train.finish_step(self.params, self.state, self.lr(), self.weight_decay, None, update=self._update)
        value = float(total.detach())
        if math.isnan(value):   # the update was skipped: a NaN loss comes with NaN gradients (ldiff_op_dice_ce poisons them)
            raise ValueError("train_step: the loss is NaN -- a label outside [0, n_heads) (torch's cross_entropy raises there too) or non-finite logits")
        return value

    @torch.no_grad()
    def validation_step(self, data, targets) -> dict:
        """nnUNetTrainer.validation_step (:915-989) for plain labels: the loss, and per foreground class tp / fp / fn of the full-resolution arg-max, from
        metrics' confusion kernel (rows = targets, columns = predictions).  With an ignore label (:966-978: the counts are masked by
        `target != ignore_label`) the kernel's own rule does it: a pixel whose target is no class enters no cell, so it is in no tp, fp or fn."""
        with torch.cuda.device(self.device):
            outputs = self.network(data)
            tl = self._targets(targets, 1)
            if len(tl) < len(outputs):
                loss = float("nan")
            elif self.ddp and self.world > 1:   # the reference's validation loss is the same loss object: its Dice term sees all ranks' batches
                graded, local, table = self._statistics(outputs, tl)
                loss = float(self._loss_from_sums(graded, local, self.gather_sums(table).to(self.device), 1.0))
            else:
                loss = float(self.loss(outputs, tl))
            top = tl[0]
            if top.dim() == 4:
                top = top[:, 0]
            if top.is_floating_point():
                top = top.long()
            if self.regions:   # :955-982, region branch: sigmoid(output) > 0.5 on the network's float16 output, all R regions, no background row to drop
                from . import nnunet
                c = ag.region_counts(outputs[0], top.to(self.device), self.region_table, self.n_heads, nnunet.REGION_THRESHOLD_F16).cpu().numpy()
                return {"loss": loss, "tp_hard": c[0], "fp_hard": c[1], "fn_hard": c[2]}
            logits = outputs[0][..., :self.n_heads].permute(0, 3, 1, 2).contiguous()
            conf = metrics.confusion_matrix(logits, top.to(self.device), self.n_heads).sum(0).cpu().numpy()
        tp = np.diag(conf)
        fp, fn = conf.sum(0) - tp, conf.sum(1) - tp
        return {"loss": loss, "tp_hard": tp[1:], "fp_hard": fp[1:], "fn_hard": fn[1:]}

    def on_validation_epoch_end(self, val_outputs: List[dict]) -> float:
        """:991-1025 and nnunet_logger.py:50-51: global Dice per class from the summed counts, its nan-mean, and the 0.9 / 0.1 EMA."""
        tp = np.sum([o["tp_hard"] for o in val_outputs], 0)
        fp = np.sum([o["fp_hard"] for o in val_outputs], 0)
        fn = np.sum([o["fn_hard"] for o in val_outputs], 0)
        with np.errstate(invalid="ignore", divide="ignore"):
            per_class = [float(v) for v in 2 * tp / (2 * tp + fp + fn)]
        mean_fg_dice = float(np.nanmean(per_class))
        ema = self.log["ema_fg_dice"][-1] * 0.9 + 0.1 * mean_fg_dice if self.log["ema_fg_dice"] else mean_fg_dice
        self.log["mean_fg_dice"].append(mean_fg_dice)
        self.log["ema_fg_dice"].append(ema)
        self.log["dice_per_class_or_region"].append(per_class)
        self.log["val_losses"].append(float(np.mean([o["loss"] for o in val_outputs])))
        return mean_fg_dice

    def save_checkpoint(self, filename: str) -> None:
        """The dictionary nnUNetTrainer.save_checkpoint writes (:1056-1077)."""
        bufs = self.state["sgd"].get("momentum_buffer", {})
        opt = {"state": {i: {"momentum_buffer": b.detach().cpu().clone()} for i, b in bufs.items()},
               "param_groups": [{"lr": self.lr(), "momentum": MOMENTUM, "dampening": 0, "weight_decay": self.weight_decay, "nesterov": True,
                                 "maximize": False, "foreach": None, "differentiable": False, "initial_lr": self.initial_lr,
                                 "params": list(range(len(self.params)))}]}
        scaler = {"scale": float(self.state["loss_scale"]), "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": train.LOSS_SCALE_GROWTH_INTERVAL,
                  "_growth_tracker": int(self.state.get("finite_steps", 0))}
        os.makedirs(os.path.dirname(os.path.abspath(filename)), exist_ok=True)
        torch.save({"network_weights": self.network.state_dict(), "optimizer_state": opt, "grad_scaler_state": scaler, "logging": dict(self.log),
                    "_best_ema": self._best_ema, "current_epoch": self.current_epoch + 1, "init_args": self.init_args, "trainer_name": "nnUNetTrainer",
                    "inference_allowed_mirroring_axes": self.inference_allowed_mirroring_axes}, filename)

    def run_training(self, train_batches, val_batches, output_folder: str, iterations_per_epoch: int = 250, val_iterations: int = 50) -> dict:
        """nnUNetTrainer.run_training (:1272-1297): per epoch `iterations_per_epoch` train steps, `val_iterations` validation steps, `checkpoint_best.pth`
        whenever the EMA of the mean foreground Dice reaches a new best (:1046-1049), `checkpoint_final.pth` at the end (:853).  Batches: dicts with
        `data` / `target` (the nnU-Net loader's) or pairs.  `output_folder` is the fold's folder (`<model folder>/fold_0`).  Returns the log."""
        tr, va = _Stream(train_batches), _Stream(val_batches)
        while self.current_epoch < self.num_epochs:
            self.log["lrs"].append(self.lr())
            losses = [self.train_step(*_batch(next(tr))) for _ in range(iterations_per_epoch)]
            self.log["train_losses"].append(pooled_train_loss(losses, self._dist, self.group))
            self.on_validation_epoch_end(pooled_validation([self.validation_step(*_batch(next(va))) for _ in range(val_iterations)], self._dist, self.group))
            ema = self.log["ema_fg_dice"][-1]
            if self._best_ema is None or ema > self._best_ema:   # the pooled values are the same on every rank: so are the EMA and the best
                self._best_ema = ema
                if self.rank == 0:
                    self.save_checkpoint(os.path.join(output_folder, "checkpoint_best.pth"))
            self.current_epoch += 1
        self.current_epoch -= 1   # save_checkpoint stores current_epoch + 1; on_train_end runs after the last on_epoch_end's increment (:853)
        if self.rank == 0:   # nnUNetTrainer.save_checkpoint (:1057): `if self.local_rank == 0`
            self.save_checkpoint(os.path.join(output_folder, "checkpoint_final.pth"))
        self.current_epoch += 1
        if self._dist is not None and self.world > 1:
            self._dist.barrier(group=self.group)
        return self.log
