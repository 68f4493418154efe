"""Host-side mirror of the reference's orchestrator `LDiffusionModel` (/root/reference/ldiffusion.py:31-324) for the
sampling path: same constructor and `inference(...)` signature (cell and tissue levels), same error for an invalid level.
Training: `train_ldiffusion` (ldiffusion.py:121-295) runs on the HIP kernels, forward and backward (`ldiffusion_amd.train`,
parity-tested against torch.autograd over the oracle); what differs from the reference (no ZeRO-3, optional
VGG19 content term, fp16 operands) is listed in its docstring.  The loaders are the reference's (`load_data`, ldiffusion.py:72-119, over
`ldiffusion_amd.dataset`), built from `args.image_dir` / `args.label_dir` where none is injected; for the warm-up they are device-resident
(`dataset.DeviceLoader`).  `parse_args` and `python -m ldiffusion_amd.ldiffusion` are the reference's command line (:19-29,326-331).  The segmentor stage of `train` runs at the tissue level
(`Segmentor.train_tissue_model_nnUNetv2`); at the cell level it raises.
"""
from __future__ import annotations

import argparse
import os

import torch

from .parallel import world_info
from .segmentor import Segmentor


def parse_args(argv=None):
    """ldiffusion.py:19-29: the reference's eight flags, plus --level, --component and --ldiffusion-weight (the reference hard-codes them in its
    `__main__`, :330-331), --ignore-pixel, the grey level of unlabelled pixels in partly annotated tissue labels (not given: fully annotated), and
    --regions, a JSON file {"regions": {name: [grey levels or class indices]}, "regions_class_order": [...]} for region-based tissue training, and
    --validate / --postprocessing, the final validation of the tissue fold and the postprocessing fitted on it (`Segmentor.train_tissue_model_nnUNetv2`'s),
    and --folds, the folds of the five-fold split the tissue stage trains one after the other (not given: fold 0)."""
    parser = argparse.ArgumentParser(description="Diffusion model training parameters")
    parser.add_argument("--local_rank", type=int, default=int(os.environ.get("LOCAL_RANK", -1)))
    parser.add_argument("--diffusion-path", type=str, required=True, help="stable diffusion base model path")
    parser.add_argument("--image-dir", type=str, required=True)
    parser.add_argument("--label-dir", type=str, required=True)
    parser.add_argument("--num-epochs", type=int, required=True)
    parser.add_argument("--batch-size", type=int, required=True)
    parser.add_argument("--num-inference-steps", type=int, required=True)
    parser.add_argument("--num-classes", type=int, required=True)
    parser.add_argument("--level", type=str, default="tissue", choices=("tissue", "cell"))
    parser.add_argument("--component", type=str, default="all", choices=("all", "ldiffusion", "segmentor"))
    parser.add_argument("--ldiffusion-weight", type=str, default=None, help="trained L-Diffusion weights, for --component segmentor")
    parser.add_argument("--ignore-pixel", type=int, default=None, help="grey level of unlabelled pixels in the label images (tissue level): nnU-Net's ignore label")
    parser.add_argument("--regions", type=str, default=None, help="JSON file with `regions` and `regions_class_order` (tissue level): nnU-Net's region labels")
    parser.add_argument("--validate", action="store_true", help="after the tissue training: predict fold 0's validation cases in full, write fold_0/validation/summary.json")
    parser.add_argument("--postprocessing", action="store_true", help="--validate, then fit nnU-Net's largest-component postprocessing: fold_0/validation/postprocessing.json")
    parser.add_argument("--folds", type=int, nargs="+", default=None, help="folds of the five-fold split to train, e.g. --folds 0 1 2 3 4 (tissue level; default: fold 0)")
    return parser.parse_args(argv)


class LDiffusionModel:
    def __init__(self, diffusion_path, level, local_rank=-1, plan_batch=None):
        rank, world, env_local = world_info()                     # ldiffusion.py:34-35,42
        self.world_size, self.rank = world, rank
        self.is_distributed = world > 1
        self.local_rank = int(local_rank if local_rank is not None and local_rank >= 0 else env_local)
        if not torch.cuda.is_available():
            raise RuntimeError("ldiffusion_amd.LDiffusionModel needs a ROCm GPU (the MI355X path has no CPU fallback)")
        torch.cuda.set_device(self.local_rank)
        self.device = torch.device(f"cuda:{self.local_rank}")
        self.diffusion_path = diffusion_path
        self.level = level
        self.linear_layer = None
        self.plan_batch = plan_batch   # batch-invariant mode of the pipelines load_model returns (None: the default, plans from each launch's own batch)

    def _is_main_process(self):
        return self.rank == 0

    def load_model(self, model_path):
        """ldiffusion.py:66-70 -> (pipeline, vae)"""
        from .pipeline import StableDiffusionImg2ImgPipeline
        pipeline = StableDiffusionImg2ImgPipeline.from_pretrained(model_path, torch_dtype=torch.float32, device=self.device)
        if self.plan_batch is not None:
            pipeline.set_plan_batch(self.plan_batch)
        return pipeline, pipeline.vae

    def _reduce_mean(self, value):
        """ldiffusion.py:54-64: mean of a python float over the ranks."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return value
        t = torch.tensor([value], device=self.device, dtype=torch.float64)
        dist.all_reduce(t)
        return float(t.item() / dist.get_world_size())

    def load_data(self, image_dir, label_dir, batch_size, train_ratio=0.7, **kw):
        """ldiffusion.py:72-119 -> (train_loader, val_loader, train_sampler): `dataset.load_data` at the model's level, world, rank and device
        (device-resident loaders; `device=None` among the keywords gives the host DataLoaders).  `image_size`, `io_workers` and `cache_bytes` are handed on."""
        from . import dataset
        kw.setdefault("device", self.device)
        return dataset.load_data(image_dir, label_dir, batch_size, self.level, train_ratio=train_ratio, world=self.world_size, rank=self.rank, **kw)

    def train_ldiffusion(self, args, train_loader, val_loader=None):
        """ldiffusion.py:121-295 on the HIP kernels (forward and backward, ldiffusion_amd.train): per batch Resize(64) -> VAE encode ->
        V5 loop -> InfoNCE loss -> backward -> gradient all-reduce -> clip 1.0 -> AdamW(lr 1e-5, wd 0.01) on UNet + text projection; per epoch
        the mean loss goes to train_save/loss/<yy_mm_dd>/contrast_loss.csv and, when it improved, the UNet (diffusers layout) and
        proj_weights.pt are saved under LDiffusion/train_save/unet/<yy_mm_dd>/ (the layout `Segmentor.load_ldiffusion` reads back).
        Differences, all explicit: replicated parameters + one gradient all-reduce instead of ZeRO-3 with CPU offload; fp16 MFMA operands
        with fp32 accumulation / gradients / master weights instead of fp32 everywhere; the VGG19 content term only when
        `args.vgg_features` (a callable) is given -- ImageNet weights are not available offline, and the loop says so once.
        `train_loader` yields (image [B,3,H,W] float in ToTensor range, _, label [B,1,H,W]) like the reference's PUMA loader.  A loader that has
        `warmup_batches` (dataset.DeviceLoader) is iterated through it instead: it yields the 64x64 image and label of each batch straight from its
        device store (same order, same generator draws), and the two reductions below are not run."""
        import csv
        import time
        from datetime import datetime
        import torch.nn as nn
        import torch.nn.functional as F
        from . import train as T, weights
        from .loss import InfoNceLoss
        num_epochs = int(getattr(args, "ldiffusion_epochs", 10))                     # hard-coded 10 in the reference (:122)
        num_inference_steps = args.num_inference_steps
        root = getattr(args, "output_root", ".")
        self.pipeline, self.vae = self.load_model(args.diffusion_path)
        current_date = datetime.now().strftime("%y_%m_%d")
        csv_dir = os.path.join(root, "train_save", "loss", current_date)
        csv_file = os.path.join(csv_dir, "contrast_loss.csv")
        os.makedirs(csv_dir, exist_ok=True)
        if self._is_main_process():
            with open(csv_file, mode="w", newline="") as f:
                csv.writer(f).writerow(["epoch", "loss"])
        hidden = self.pipeline.text_encoder.config.hidden_size
        cad = self.pipeline.unet.config.cross_attention_dim
        if self.linear_layer is None or self.linear_layer.in_features != hidden or self.linear_layer.out_features != cad:
            self.linear_layer = nn.Linear(hidden, cad)
        self.linear_layer = self.linear_layer.to(self.device, dtype=torch.float32)
        unet = T.TrainableUNet(self.pipeline.unet._cfg, self.pipeline.unet.state_dict(), self.device)
        dec = T.FrozenVAEDecoder(self.vae._cfg, self.vae._host_sd, self.device)
        proj = (self.linear_layer.weight, self.linear_layer.bias)
        loss_obj = InfoNceLoss(vgg_features=getattr(args, "vgg_features", None))
        if loss_obj.vgg is None and self._is_main_process():
            print("[train_ldiffusion] no vgg_features given: the VGG19 content term of InfoNceLoss (model/loss.py:21-42) is left out; "
                  "training on the contrastive term only")
        save_path = os.path.join(root, "LDiffusion", "train_save", "unet", current_date)
        checkpoint = 100
        n_sched = min(int(num_inference_steps / 5), len(self.pipeline.scheduler.alphas_cumprod))
        state, noise_offset = {}, 0   # Philox counters consumed so far: every step draws fresh Laplace noise (the reference samples anew each time)
        # forward + loss + backward as ONE captured HIP graph per step (train.GraphedStep) where the loss is the contrastive term alone and the
        # batch has the captured shape; anything else (content term, a short last batch, more triples than the capture holds) runs eagerly
        use_graph = bool(getattr(args, "use_graph", True)) and loss_obj.vgg is None
        gstep = None
        # The reference's engine is DeepSpeed ZeRO stage 3 (ldiffusion.py:165-193): under a process group every rank owns 1/W of the float32 masters and
        # of the AdamW moments, gradients are reduce-scattered, the parameters all-gathered in front of each forward (train.ShardedAdamW,
        # partition_params).  Created BEFORE the GraphedStep: the parameters move into its flat buffer.  One process: the multi-tensor AdamW.
        opt = T.ShardedAdamW(unet.parameters() + list(proj), lr=1e-5, weight_decay=0.01, partition_params=True) if self.is_distributed else None
        for epoch in range(num_epochs):
            if hasattr(train_loader, "sampler") and hasattr(train_loader.sampler, "set_epoch"):
                train_loader.sampler.set_epoch(epoch)
            total, start = 0.0, time.time()
            from_store = hasattr(train_loader, "warmup_batches")
            for batch in (train_loader.warmup_batches(64) if from_store else train_loader):
                if from_store:
                    image, lab = batch
                else:
                    image, _, label = batch
                    image = F.interpolate(image.to(self.device, dtype=torch.float32), size=(64, 64), mode="bilinear", align_corners=False, antialias=True)
                B = image.shape[0]
                ids = torch.tensor(self.pipeline.tokenizer(["A pathological slide"] * B)["input_ids"], dtype=torch.long, device=self.device)
                with torch.no_grad():
                    text_hidden = self.pipeline.text_encoder(ids)["last_hidden_state"].to(dtype=torch.float32)
                    if not from_store:
                        lab = F.interpolate(label.to(self.device, torch.float32), size=(64, 64), mode="bilinear", align_corners=False).to(torch.uint8)
                    latents = self.vae.encode(image).latent_dist.mean.to(dtype=torch.float32)
                self.pipeline.scheduler.set_timesteps(n_sched, device=self.device)
                ts = [int(t) for t in self.pipeline.scheduler.timesteps]

                def loss_fn(feats, rgb, image=image, lab=lab):
                    contrastive = loss_obj.compute_contrastive_loss(feats, lab)
                    if loss_obj.vgg is None:
                        return contrastive
                    big = F.interpolate(rgb, size=(1024, 1024), mode="bilinear", align_corners=False)
                    return loss_obj.compute_content_loss(image, big) + contrastive

                pairs = None
                if use_graph:
                    pairs = loss_obj.sample_triples(lab.to("cpu"))   # the draws compute_contrastive_loss would make (same torch random stream)
                    n_tr = sum(len(t) for t in pairs)
                    if gstep is None and n_tr > 0:
                        gstep = T.GraphedStep(unet, dec, proj, B, ts, self.pipeline.scheduler.alphas_cumprod, latent_hw=latents.shape[-1],
                                              text_len=text_hidden.shape[1], text_dim=text_hidden.shape[2], max_triples=max(256, 64 * B),
                                              num_negatives=loss_obj.num_negatives, temperature=loss_obj.temperature)
                    # never skipped per rank: a batch without sample triples still runs the (eager) step with zero gradients, so that every rank
                    # enters the same gradient collective (train.run_step)
                    val, _ = T.run_step(gstep, unet, dec, proj, latents, text_hidden, ts, self.pipeline.scheduler.alphas_cumprod, pairs, state,
                                        lr=1e-5, weight_decay=0.01, max_grad_norm=1.0, seed=self.rank, offset=noise_offset, optimizer=opt)
                    total += val
                else:
                    total += T.train_step(unet, dec, proj, latents, text_hidden, ts, self.pipeline.scheduler.alphas_cumprod, None, None, state, lr=1e-5,
                                          weight_decay=0.01, loss_fn=loss_fn, max_grad_norm=1.0, seed=self.rank, offset=noise_offset, optimizer=opt)
                noise_offset += len(ts) * latents.numel()   # v5_features draws offset + i * numel for pass i
            current = self._reduce_mean(total / max(1, len(train_loader)))
            if self._is_main_process():
                print(f"Epoch [{epoch + 1}/{num_epochs}], Loss: {current:.4f}, Elapsed Time: {time.time() - start}s")
            if current < checkpoint:
                if opt is not None:
                    opt.gather()   # (a collective: every rank) the full parameters, for the checkpoint rank 0 writes
                if self._is_main_process():
                    weights.save_model_dir(save_path, self.pipeline.unet._cfg, {k: p.detach().to("cpu") for k, p in unet.p.items()})
                    torch.save({"weight": proj[0].detach().to("cpu"), "bias": proj[1].detach().to("cpu")}, os.path.join(save_path, "proj_weights.pt"))
                checkpoint = current
            if self.is_distributed:
                torch.distributed.barrier()
            if self._is_main_process():
                with open(csv_file, mode="a", newline="") as f:
                    csv.writer(f).writerow([epoch + 1, current])
        del self.pipeline, self.vae
        torch.cuda.empty_cache()
        return save_path

    def train(self, args, component="all", ldiffusion_weight=None, train_loader=None, val_loader=None, wgrad_route=None, cell_weights=None, instances=None,
              ignore_pixel=None, regions=None, regions_class_order=None, region_loss=None, validate=None, postprocessing=None, validation_checkpoint=None,
              folds=None, **_ignored):
        """ldiffusion.py:297-315.  The loaders are injected (`train_loader=`, `val_loader=`), or, with none injected and `args` carrying `image_dir` and
        `label_dir`, built as the reference builds them (`self.load_data(args.image_dir, args.label_dir, args.batch_size)`, with `args.image_size` (1024) and
        `args.io_workers` (4) where present): device-resident for the warm-up, plain host loaders when only the segmentor stage runs (it reads their file lists).
        `component="ldiffusion"` runs the L-Diffusion warm-up on the HIP kernels and returns the saved weight directory.  The segmentor stage
        ("segmentor", or after the warm-up with "all") at level "tissue" is `Segmentor.train_tissue_model_nnUNetv2(args.num_epochs - 10,
        ldiffusion_weight, args.diffusion_path)` with the loaders' `dataset.image_dir` / `label_dir` lists (:306-311) and returns the trained-model
        folder; loaders without such a dataset (plain lists of batches) need the four lists as keyword arguments `train_images`, `train_labels`,
        `test_images`, `test_labels`.  `iterations_per_epoch`, `val_iterations` and `num_foreground_voxels` are handed on too, and so is `wgrad_route`
        (the route of the tissue trainer's weight gradients, `nnunet_train.Trainer`'s keyword; None: its default), and `batch_images` / `io_workers` (the
        batched dataset pass, `utils.create_nnunet_dataset`'s keywords; not given: the per-image pass), and `ignore_pixel` (else `args.ignore_pixel` where
        present; None: fully annotated labels): the grey level of unlabelled pixels, which the tissue stage trains around as nnU-Net's ignore label
        (`Segmentor.train_tissue_model_nnUNetv2`'s keyword; the warm-up reads such pixels as background, as it reads every unmapped level), and `regions` /
        `regions_class_order` (else the file `args.regions` names, where present; None: plain labels): region labels, which the tissue stage trains with one
        sigmoid head per region (`Segmentor.train_tissue_model_nnUNetv2`'s keywords, and so is `region_loss`: None is its default, the focal form), and `validate` /
        `postprocessing` (else `args.validate` / `args.postprocessing` where present and set; None or False: the stage ends at the checkpoints) with
        `validation_checkpoint`: the final validation of the fold and the largest-component postprocessing fitted on it, and `folds` (else `args.folds` where
        present; None: fold 0, and nothing handed on): the folds the tissue stage trains, validates and, with more than one, merges
        (`Segmentor.train_tissue_model_nnUNetv2`'s keyword).  At level "cell" it is
        `Segmentor.train_cell_model(args.num_epochs - 10, ldiffusion_weight, args.diffusion_path, cell_weights=..., instances=...)` (:312-313) and returns
        the folder that holds cellclassifier.pth (None when no epoch validated above 0.0).  `cell_weights` = the CellSegClassifier state dict (or its path)
        the stage starts from: the reference starts from torchvision's ImageNet weights, which it downloads, and this build downloads nothing -- without
        `cell_weights=` the stage raises NotImplementedError.  `instances` = the label-map callable (Cellpose where installed); `fit_classifier`,
        `cache_features`, `lr`, `save_root`, `seed` and `text_embeddings` are handed on."""
        if component not in ("all", "ldiffusion", "segmentor"):
            raise ValueError(f"unknown component {component!r}")
        segmentor_kwargs = {k: _ignored[k] for k in ("train_images", "train_labels", "test_images", "test_labels", "iterations_per_epoch", "val_iterations",
                                                          "num_foreground_voxels", "batch_images", "io_workers") if k in _ignored}
        if train_loader is None and getattr(args, "image_dir", None) is not None and getattr(args, "label_dir", None) is not None:
            if component in ("all", "segmentor") and self.level == "cell" and cell_weights is None:   # before any file is read
                raise NotImplementedError("segmentor training at the cell level (train_cell_model, segmentor.py:243-299) starts from torchvision's downloaded ImageNet "
                                          "weights in the reference; nothing is downloaded here: pass cell_weights= (a CellSegClassifier state dict or its path)")
            kw = {"image_size": getattr(args, "image_size", 1024), "io_workers": getattr(args, "io_workers", 4)}
            if component == "segmentor":
                kw["device"] = None
            train_loader, val_loader, _ = self.load_data(args.image_dir, args.label_dir, args.batch_size, **kw)
        if component in ("all", "ldiffusion"):
            if train_loader is None:
                raise RuntimeError("LDiffusionModel.train: no loaders: pass train_loader=, or args with image_dir and label_dir (the reference's load_data, "
                                   "ldiffusion_amd.dataset)")
            if self._is_main_process():
                print("Starting LDiffusion warming up...")
            ldiffusion_weight = self.train_ldiffusion(args, train_loader, val_loader)
        if component in ("all", "segmentor"):
            if self.level == "cell":
                if cell_weights is None:
                    raise NotImplementedError("segmentor training at the cell level (train_cell_model, segmentor.py:243-299) starts from torchvision's downloaded ImageNet "
                                              "weights in the reference; nothing is downloaded here: pass cell_weights= (a CellSegClassifier state dict or its path); "
                                              f"the L-Diffusion weights are at {ldiffusion_weight!r}")
                if self._is_main_process():
                    print("Starting Segmentor training...")
                cell_kwargs = {k: _ignored[k] for k in ("fit_classifier", "cache_features", "lr", "save_root", "seed", "text_embeddings") if k in _ignored}
                return Segmentor(train_loader, val_loader, self.level, args.num_classes).train_cell_model(args.num_epochs - 10, ldiffusion_weight, args.diffusion_path,
                                                                                                         cell_weights=cell_weights, instances=instances, **cell_kwargs)
            if self.level != "tissue":
                raise ValueError("Invalid level specified. Choose 'tissue' or 'cell'.")
            if self._is_main_process():
                print("Starting Segmentor training...")
            segmentor = Segmentor(train_loader, val_loader, self.level, args.num_classes)
            if "train_images" not in segmentor_kwargs and hasattr(train_loader, "dataset") and hasattr(val_loader, "dataset"):
                # ldiffusion.py:306-311 hands the loaders on; their datasets hold the file lists
                segmentor_kwargs.update(train_images=train_loader.dataset.image_dir, train_labels=train_loader.dataset.label_dir,
                                        test_images=val_loader.dataset.image_dir, test_labels=val_loader.dataset.label_dir)
            if wgrad_route is not None:   # None: the call is the one of before the keyword existed
                segmentor_kwargs["wgrad_route"] = wgrad_route
            if ignore_pixel is None:
                ignore_pixel = getattr(args, "ignore_pixel", None)
            if ignore_pixel is not None:
                segmentor_kwargs["ignore_pixel"] = ignore_pixel
            if regions is None and getattr(args, "regions", None) is not None:
                import json
                with open(args.regions) as f:
                    given = json.load(f)
                regions, regions_class_order = given["regions"], given["regions_class_order"]
            if regions is not None:
                segmentor_kwargs.update(regions=regions, regions_class_order=regions_class_order)
                if region_loss is not None:
                    segmentor_kwargs["region_loss"] = region_loss
            if validate is None:
                validate = getattr(args, "validate", None)
            if postprocessing is None:
                postprocessing = getattr(args, "postprocessing", None)
            if validate:   # not set: the call is the one of before the keywords existed
                segmentor_kwargs["validate"] = True
            if postprocessing:
                segmentor_kwargs["postprocessing"] = True
            if validation_checkpoint is not None and (validate or postprocessing):
                segmentor_kwargs["validation_checkpoint"] = validation_checkpoint
            if folds is None:
                folds = getattr(args, "folds", None)
            if folds is not None:   # None: the call is the one of before the keyword existed
                segmentor_kwargs["folds"] = tuple(folds)
            return segmentor.train_tissue_model_nnUNetv2(args.num_epochs - 10, ldiffusion_weight, args.diffusion_path, **segmentor_kwargs)
        return ldiffusion_weight

    def inference(self, image_path, ldiffusion_weight, segmentor_weight, num_classes, head=None, predictor=None, output_path=None,
                  text_embeddings=None, instances=None, batch_tiles=None, batch_images=None, postprocess=False, use_folds=None,
                  **_readme_kwargs):
        """ldiffusion.py:317-324.  Tissue: `segmentor_weight` = nnU-Net's trained-model folder, as in the reference (the head then runs on the HIP
        library, nnunet.py), or `predictor` = any head callable; cell: `segmentor_weight` = the folder with cellclassifier.pth (the ResNet152
        instance classifier then runs on the HIP library, cellhead.py; `instances` = the label-map callable, Cellpose where installed), or
        `head` = any head callable; `output_path` is the folder-mode argument of the tissue path; `batch_tiles` (tissue) = tiles per head call of the batched
        sliding window, None = one call per tile and mirror variant (Segmentor.inference_tissue_model_nnUNetv2); `batch_images` (tissue, folder mode) = images per
        sampler call, None = one file at a time; `postprocess` (tissue) = nnU-Net's fitted largest-component postprocessing on every mask, True reading
        `<segmentor_weight>/fold_0/validation/postprocessing.json` (Segmentor.inference_tissue_model_nnUNetv2's keyword; False: not handed on); `use_folds` (tissue) = the folds of `segmentor_weight` whose logits are averaged,
        the reference's `use_folds=` (None: fold 0, and not handed on); other README-era keyword arguments (dtm_path)
        are accepted and ignored like the code ignores them."""
        segmentor = Segmentor(train_loader=None, val_loader=None, level=self.level, num_classes=num_classes)
        if self.level == "tissue":
            return segmentor.inference_tissue_model_nnUNetv2(image_path, self.diffusion_path, ldiffusion_weight, segmentor_weight,
                                                             output_path=output_path, predictor=predictor if predictor is not None else head,
                                                             text_embeddings=text_embeddings, batch_tiles=batch_tiles,
                                                             **({} if batch_images is None else {"batch_images": batch_images}),
                                                             **({} if postprocess is False or postprocess is None else {"postprocess": postprocess}),
                                                             **({} if use_folds is None else {"use_folds": tuple(use_folds)}))
        elif self.level == "cell":
            return segmentor.inference_cell_model(image_path, self.diffusion_path, ldiffusion_weight, segmentor_weight, head=head,
                                                  text_embeddings=text_embeddings, instances=instances)
        else:
            raise ValueError("Invalid level specified. Choose 'tissue' or 'cell'.")


def main(argv=None):
    """ldiffusion.py:326-331: `python -m ldiffusion_amd.ldiffusion --diffusion-path ... --image-dir ... --label-dir ...`."""
    args = parse_args(argv)
    if int(os.environ.get("RANK", "0")) == 0:
        print(str(vars(args)))
    trainer = LDiffusionModel(args.diffusion_path, level=args.level, local_rank=args.local_rank)
    return trainer.train(args, component=args.component, ldiffusion_weight=args.ldiffusion_weight)


if __name__ == "__main__":
    main()
