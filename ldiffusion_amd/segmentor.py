"""Host-side mirror of the reference's `Segmentor` for the sampling path (same names, argument meaning and errors).

Mirrors /root/reference/segmentor.py: `_resolve_ldiffusion_dir` (:26-29), `_ensure_ldiffusion_proj` (:31-52),
`_get_text_embeddings` (:54-60), `load_ldiffusion` (:76-84), `ldiffusion_augment` (:86-112), `_UNetTextAlignWrapper`
(:183-205), the sampler part + mask tail of `inference_cell_model` (:490-545) and of `inference_tissue_model_nnUNetv2`
(:388-488).  The segmentation heads themselves (`model/conductor.py`, nnU-Net) are outside the hot-path scope (SURVEY.md
8a/8f): both inference functions take the head as a callable and raise if none is given instead of silently substituting one;
for the tissue level the callable is applied through the device-resident mirror of nnU-Net's sliding-window predictor
(`tiling.predict_sliding_window_return_logits`: Gaussian-weighted fp16 accumulation, mirroring TTA) instead of the reference's
PNG / tmpdir / multiprocess round trip.
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .models import CLIPTextModel as HipCLIPTextModel
from .models import UNet2DConditionModel
from .pipeline import PROMPT, LaplaceSampler, StableDiffusionImg2ImgPipeline, argmax_mask

IMAGENET_MEAN = (0.485, 0.456, 0.406)  # segmentor.py:508
IMAGENET_STD = (0.229, 0.224, 0.225)


class TextAlignedUNet:
    """`_UNetTextAlignWrapper` (segmentor.py:183-205): when `encoder_hidden_states` is None or its last dim differs from
    `cross_attention_dim`, the cached default embeddings are used instead, expanded to the batch."""

    def __init__(self, base_unet, default_text_embeddings):
        self.base_unet = base_unet
        self.default_text_embeddings = default_text_embeddings
        self.cross_attention_dim = base_unet.config.cross_attention_dim
        self.config = base_unet.config

    def __call__(self, sample, timestep, encoder_hidden_states, *args, **kwargs):
        use_fallback = encoder_hidden_states is None or encoder_hidden_states.shape[-1] != self.cross_attention_dim
        if use_fallback:
            emb = self.default_text_embeddings
            if emb.shape[0] != sample.shape[0]:
                emb = emb[:1].expand(sample.shape[0], -1, -1)
            encoder_hidden_states = emb
        return self.base_unet(sample, timestep, encoder_hidden_states.to(sample.device, dtype=torch.float32), *args, **kwargs)

    forward = __call__

    def eval(self):
        return self

    def to(self, *a, **k):
        return self


class Segmentor:
    def __init__(self, train_loader, val_loader, level, num_classes):
        if not torch.cuda.is_available():
            raise RuntimeError("ldiffusion_amd.Segmentor needs a ROCm GPU (no CPU fallback)")
        self.device = torch.device(f"cuda:{torch.cuda.current_device()}")
        self.level = level
        self.num_classes = num_classes
        self.model = None
        self.train_loader, self.val_loader = train_loader, val_loader
        self.ldiffusion_proj = None
        self._sampler = None

    def _resolve_ldiffusion_dir(self, ldiffusion_weight):
        return ldiffusion_weight if os.path.isdir(ldiffusion_weight) else os.path.dirname(ldiffusion_weight)

    def _ensure_ldiffusion_proj(self, pipeline, unet, ldiffusion_weight=None):
        if isinstance(pipeline.text_encoder, HipCLIPTextModel):
            # the library's encoder carries the projection itself (one call, fused behind the final LayerNorm): None is returned, and the callers use
            # `text_encoder.project(ids)`.  As below: proj_weights.pt where there is one, else a freshly initialised Linear(hidden, cross_attention_dim)
            enc, cad = pipeline.text_encoder, unet.config.cross_attention_dim
            if ldiffusion_weight is not None:
                p = os.path.join(self._resolve_ldiffusion_dir(ldiffusion_weight), "proj_weights.pt")
                if os.path.exists(p):
                    enc.load_projection(torch.load(p, map_location="cpu"))
            if enc.projection_dim is None:
                enc.load_projection(nn.Linear(enc.config.hidden_size, cad).state_dict())
            if enc.projection_dim != cad:
                raise RuntimeError(f"text projection: the encoder's projection has {enc.projection_dim} output channels, the UNet's cross_attention_dim is {cad}")
            return None
        hidden = pipeline.text_encoder.config.hidden_size
        cad = unet.config.cross_attention_dim
        if self.ldiffusion_proj is None or self.ldiffusion_proj.in_features != hidden or self.ldiffusion_proj.out_features != cad:
            self.ldiffusion_proj = nn.Linear(hidden, cad).to(self.device, dtype=torch.float32)
        if ldiffusion_weight is not None:
            p = os.path.join(self._resolve_ldiffusion_dir(ldiffusion_weight), "proj_weights.pt")
            if os.path.exists(p):
                self.ldiffusion_proj.load_state_dict(torch.load(p, map_location=self.device), strict=True)
        self.ldiffusion_proj = self.ldiffusion_proj.to(self.device, dtype=torch.float32).eval()
        return self.ldiffusion_proj

    @torch.no_grad()
    def _get_text_embeddings(self, prompt, batch_size, pipeline, unet):
        proj = self._ensure_ldiffusion_proj(pipeline, unet)
        if isinstance(pipeline.text_encoder, HipCLIPTextModel):
            return pipeline.text_encoder.project(pipeline.tokenizer([prompt] * batch_size)["input_ids"])
        ids = torch.tensor(pipeline.tokenizer([prompt] * batch_size)["input_ids"], dtype=torch.long, device=self.device)
        emb = pipeline.text_encoder(ids)["last_hidden_state"].to(dtype=torch.float32)
        return proj(emb).to(dtype=torch.float32)

    def initialize_model(self, level, num_classes):
        if level not in ("tissue", "cell"):
            raise ValueError("Invalid level specified. Choose 'tissue' or 'cell'.")
        raise RuntimeError("the segmentation heads (model/conductor.py, nnU-Net) are outside the MI355X hot-path scope; pass `head=`")

    def micro_dice(self, predicted_labels, true_labels, num_classes=7):
        """segmentor.py:114-142, the figure of the validation loop (:284-289): per-class Dice over the arg-max labels and its mean, from one
        confusion matrix counted on the device (utils.micro_dice is the same function, as in the reference)."""
        from .utils import micro_dice
        return micro_dice(predicted_labels, true_labels, num_classes)

    def load_ldiffusion(self, ldiffusion_weight, diffusion_path, text_encoder="transformers", plan_batch=None):
        """text_encoder="hip": the prompt's CLIP pass and projection run on the library (`StableDiffusionImg2ImgPipeline.from_pretrained`).
        plan_batch=n: batch-invariant mode of the UNet and the VAE (`StableDiffusionImg2ImgPipeline.set_plan_batch`; None leaves the default)."""
        pipeline = StableDiffusionImg2ImgPipeline.from_pretrained(diffusion_path, torch_dtype=torch.float32, device=self.device, text_encoder=text_encoder)
        unet = UNet2DConditionModel.from_pretrained(ldiffusion_weight, device=self.device).eval()
        vae = pipeline.vae
        pipeline.unet = unet
        if plan_batch is not None:
            pipeline.set_plan_batch(plan_batch)
        if pipeline.text_encoder is not None:
            self._ensure_ldiffusion_proj(pipeline, unet, ldiffusion_weight=ldiffusion_weight)
        return pipeline, unet, vae

    def _one_pass(self, images, text_embeddings, pipeline, unet):
        if self._sampler is None or self._sampler.pipeline is not pipeline or pipeline.unet is not unet:
            pipeline.unet = unet
            self._sampler = LaplaceSampler(pipeline)
        return self._sampler.sample(images, text_embeddings, 1, want_features=False, want_rgb=True)

    def build_augmented_dataloader(self, dataloader, augment_fn, pipeline, unet, vae, device, batch_size, category, num_workers=0, generator=None, with_index=False):
        """segmentor.py:144-161: run `augment_fn(inputs, pipeline, unet, vae)` (e.g. `ldiffusion_augment`) once over `dataloader` -- batches
        (inputs, masks, _) -- under no_grad, keep the augmented inputs and the masks on the host, and serve them from a shuffling
        TensorDataset loader of `batch_size`.  `category` only labels the reference's progress bar.  `generator` seeds the shuffle (None: torch's global
        one, as in the reference); with_index=True appends each sample's position in the dataset as a third tensor (what `train_cell_model` keys its caches by)."""
        from torch.utils.data import DataLoader, TensorDataset
        all_aug_inputs, all_masks = [], []
        for inputs, masks, _ in dataloader:
            inputs, masks = inputs.to(device), masks.to(device)
            with torch.no_grad():
                aug_inputs = augment_fn(inputs, pipeline, unet, vae)
            all_aug_inputs.append(aug_inputs.cpu())
            all_masks.append(masks.cpu())
        tensors = [torch.cat(all_aug_inputs, dim=0), torch.cat(all_masks, dim=0)]
        if with_index:
            tensors.append(torch.arange(tensors[0].shape[0]))
        return DataLoader(TensorDataset(*tensors), batch_size=batch_size, shuffle=True, num_workers=num_workers, generator=generator)

    @torch.no_grad()
    def ldiffusion_augment(self, inputs, pipeline, unet, vae, text_embeddings=None):
        """segmentor.py:86-112, batched: encode mean -> set_timesteps(1) -> one UNet pass -> step -> decode -> uint8 ->
        Resize((1024,1024)) + ToTensor.  Returns float [B,3,1024,1024] in [0,1] on the device."""
        if text_embeddings is None:
            text_embeddings = self._get_text_embeddings(PROMPT, 1, pipeline, unet)
        out = self._one_pass(inputs.to(self.device, dtype=torch.float32), text_embeddings, pipeline, unet)
        rgb = out["rgb"]  # [B,H,W,3] u8
        if rgb.shape[1:3] == (1024, 1024):
            return rgb.permute(0, 3, 1, 2).float() / 255.0
        from . import imgio  # other sizes: the reference's PIL bilinear Resize + ToTensor, bit for bit on the device (imgio.resize_u8 behind numpy's float32 / 255.0 as a table)
        return imgio.resize_to_tensor(rgb, (1024, 1024))

    @torch.no_grad()
    def ldiffusion_augment_for_multimodal(self, rgb, dtm, pipeline, unet, vae, controlnet, batch_size, device, u=None, seed=0):
        """segmentor.py:301-386 (sampler variant V7: RGB + depth, ControlNet residuals), per sample as there:
            rgb, dtm -> bilinear 256 x 256;  z = vae.encode(rgb).latent_dist.sample() * 0.18215          (:339)
            depth = bilinear 32 x 32 of dtm, repeated over the 4 latent channels                          (:340-341)
            z_noisy = z + Laplace(0, 1) * depth                                                           (:344-345)
            ctx = proj(text_encoder("A remote sense image", padded to 77))                                (:348-352)
            residuals = controlnet(z_noisy, t, ctx, controlnet_cond = depth x 3)  at set_timesteps(1)     (:355-363)
            eps = unet(z_noisy, t, ctx, down_block_additional_residuals, mid_block_additional_residual)   (:366-372)
            recon = vae.decode((z_noisy - eps * depth) / 0.18215).sample                                  (:375-379)
        Returns the list of [256, 256, 3] float arrays the reference returns (:381-386).  `controlnet` is the caller's module (the reference
        trains none and ships no weights for one: SURVEY 8f): handed a `models.ControlNetModel` it is attached to the UNet for the call and each sample
        is ONE UNet call (the ControlNet's blocks inside it); any other object is called as the reference calls it.  The UNet, the VAE and the Laplace
        transform run on the HIP kernels.
        `u` (optional, [B, 4, 32, 32] uniform draws in (-1, 1)) fixes the Laplace noise (parity is defined given u)."""
        from .pipeline import laplace_noise
        dev = self.device
        proj = self._ensure_ldiffusion_proj(pipeline, unet)
        rgb = F.interpolate(rgb.to(dev, torch.float32), size=(256, 256), mode="bilinear", align_corners=False)
        dtm = F.interpolate(dtm.to(dev, torch.float32), size=(256, 256), mode="bilinear", align_corners=False)
        ids = pipeline.tokenizer(["A remote sense image"], padding="max_length", max_length=77, return_tensors="pt")
        ids = torch.as_tensor(ids["input_ids"] if isinstance(ids, dict) else ids.input_ids, dtype=torch.long, device=dev)
        if proj is None:   # the library's encoder: the projection is fused into the one call
            ctx = pipeline.text_encoder.project(ids)
        else:
            ctx = proj(pipeline.text_encoder(ids)["last_hidden_state"].to(device=dev, dtype=torch.float32)).to(dtype=torch.float32)
        recon = []
        from .models import ControlNetModel, UNet2DConditionModel
        fused = isinstance(controlnet, ControlNetModel) and isinstance(unet, UNet2DConditionModel)
        if fused:
            was_attached = unet._controlnet
            if was_attached is not controlnet:
                unet.attach_controlnet(controlnet)
        for i in range(dtm.shape[0]):
            dtm_i, rgb_i = dtm[i], rgb[i].unsqueeze(0)
            depth_condition = dtm_i.unsqueeze(0).repeat(1, 3, 1, 1)
            latents = vae.encode(rgb_i).latent_dist.sample().to(torch.float32) * 0.18215
            depth = F.interpolate(dtm_i.unsqueeze(0), size=(32, 32), mode="bilinear", align_corners=False).repeat(1, latents.shape[1], 1, 1)
            # z + Laplace(0, 1) * depth: the device transform with unit scale gives z + n, so noise = that minus z
            noise = laplace_noise(torch.zeros_like(latents), 1.0, u=None if u is None else u[i:i + 1].to(dev), seed=seed, offset=i * latents.numel())
            noisy = latents + noise * depth
            pipeline.scheduler.set_timesteps(1, device=dev)
            for t in pipeline.scheduler.timesteps:
                if fused:   # the HIP ControlNet runs inside the UNet's forward: one call, no residual tensors in between
                    eps = unet(noisy, t, encoder_hidden_states=ctx, controlnet_cond=depth_condition).sample
                    continue
                down, mid = controlnet(sample=noisy, timestep=t, encoder_hidden_states=ctx, controlnet_cond=depth_condition, return_dict=False)
                eps = unet(noisy, t, encoder_hidden_states=ctx, down_block_additional_residuals=down, mid_block_additional_residual=mid).sample
            den = noisy - eps * depth
            img = vae.decode(den / 0.18215).sample
            recon.append(img.squeeze(0).permute(1, 2, 0).cpu().numpy())
        if fused and was_attached is not controlnet:
            unet.detach_controlnet()
        return recon

    def train_tissue_model_nnUNetv2(self, epochs, ldiffusion_weight, diffusion_path, train_images=None, train_labels=None, test_images=None, test_labels=None,
                                    num_classes=None, *, iterations_per_epoch=250, val_iterations=50, num_foreground_voxels=None, wgrad_route=None, batch_images=None, io_workers=4,
                                    ignore_pixel=None, regions=None, regions_class_order=None, region_loss="focal", validate=False, postprocessing=False,
                                    validation_checkpoint="checkpoint_final.pth", folds=None):
        """segmentor.py:163-241: the tissue head's training stage, from image lists to a trained-model folder.
        Dataset (:167-205): `load_ldiffusion`, the cached text embeddings of "A pathological slide", the text-alignment wrapper, and
        `utils.create_nnunet_dataset` under nnUNet_raw (the one-pass diffusion of every image when all share one size, else copies).
        Planning (`plan_and_preprocess_entry()`, :207-215): the written PNGs are read back onto the device; `nnunet_plan.extract_fingerprint`,
        `plan_experiment` and `crossval_splits` give dataset_fingerprint.json, nnUNetPlans.json, dataset.json and splits_final.json under
        nnUNet_preprocessed/<dataset>.  The cases themselves are not written there: they stay on the device.
        Training (`get_trainer_from_args(...).run_training()`, :221-241): fold 0's train and validation keys as two `CaseStore(build="device")`, two
        `PatchLoader`s with the plans' patch and batch size, `nnunet_train.Trainer.run_training`; checkpoints under
        nnUNet_results/<dataset>/nnUNetTrainer__nnUNetPlans__2d/fold_0, plans.json and dataset.json beside it.
        `iterations_per_epoch`, `val_iterations`: nnUNetTrainer's 250 / 50.  `num_foreground_voxels`: the fingerprint's sample budget (None: the
        reference's 10e7).  `wgrad_route`: `nnunet_train.Trainer`'s (None: its default).  `batch_images`, `io_workers`: `utils.create_nnunet_dataset`'s
        (None: the per-image dataset pass; an integer: the pass batched behind the device image front end).  `ignore_pixel`: the grey level of
        unlabelled pixels in partly annotated label images (`utils.create_nnunet_dataset`'s): the dataset declares nnU-Net's ignore label, the stores
        draw patches from annotated areas and the trainer leaves those pixels out of loss, gradient and validation counts; None: fully annotated
        labels, the stage as it was.  With an ignore label the stage runs on one rank (the data-parallel step's ignore form is not built).
        `regions`, `regions_class_order` (`utils.create_nnunet_dataset`'s): region labels -- one sigmoid head per region, the reference's Dice + focal loss
        (`region_loss="bce"`: nnU-Net's Dice + BCE), patches oversampled among regions, validation Dice per region; the written folder predicts through
        the region rule.  None: the stage as it was.  The three folders come from the environment variables nnUNet_raw, nnUNet_preprocessed, nnUNet_results.
        Under a process group of more than one rank the stage is data-parallel, as the reference's nnUNetTrainer is under the same launch: rank 0 alone
        writes the dataset, the fingerprint, plans, split and the model folder; `(new_num, dataset_name)` go out by `broadcast_object_list` and a
        barrier; every rank then reads the PNGs and JSONs and builds both stores on its own device; its loaders take its entry of
        `nnunet_train.rank_batch_sizes` (batch and oversample) and the seeds 2 rank / 2 rank + 1; the trainer runs with ddp on.
        `validate` (off: `fold_0/` holds the two checkpoints and nothing else): nnUNetTrainer.perform_actual_validation after the last epoch --
        `nnunet_post.validate_fold` predicts fold 0's validation cases in full with `validation_checkpoint`, writes `fold_0/validation/<key>.png` and
        `summary.json`; the summary is kept as `self.validation_summary`.  `postprocessing` (implies `validate`): nnU-Net's largest-component
        postprocessing fitted on those predictions against labelsTr (`nnunet_post.determine_postprocessing_folder`): `fold_0/validation/postprocessing.json`
        and `fold_0/validation/postprocessed/`, what `inference_tissue_model_nnUNetv2(postprocess=True)` reads.  Rank 0 does both; the others wait.
        `folds` (None: fold 0, the stage as it was): a sequence of distinct fold numbers of the five-fold split, trained one after the other in the given
        order (`nnUNetv2_train ... FOLD` once per fold) from one dataset, fingerprint, plans and split and one read of the cases.  Fold f takes its stores from
        `splits[f]`, `initial_state_dict(spec, seed=f)`, the loader seeds 2 rank + 2 world f and + 1 (fold 0: the seeds of before), `init_args["fold"] = f` and
        writes `fold_<f>/`; under a process group every rank walks the same folds.  With `validate`, each fold is validated after its training
        (`fold_<f>/validation/`); with more than one fold the folds' predictions are then merged and scored again (`nnunet_post.accumulate_cv_results`:
        `crossval_results_folds_<f0>_<f1>.../`, `self.crossval_summary`), and `postprocessing` is fitted ONCE, on the merged folder, as
        find_best_configuration does -- what `inference_tissue_model_nnUNetv2(use_folds=..., postprocess=True)` reads.  `self.training_log` and
        `self.validation_summary` are the last fold's; `self.training_logs[f]` and `self.validation_summaries[f]` hold every fold's.  The fold "all" and
        fold numbers beyond the split (nnU-Net's random 80:20 split) are refused.
        Returns the model folder -- what `inference_tissue_model_nnUNetv2(segmentor_weight=...)` takes -- on every rank."""
        import json
        from PIL import Image
        from . import nnunet, nnunet_data, nnunet_plan, nnunet_train, utils
        roots = {}
        for name in ("nnUNet_raw", "nnUNet_preprocessed", "nnUNet_results"):
            if not os.environ.get(name):
                raise RuntimeError(f"train_tissue_model_nnUNetv2: the environment variable {name} is not set")
            roots[name] = os.environ[name]
        fold_list = (0,) if folds is None else nnunet.check_folds(folds, "folds")
        if any(f >= 5 for f in fold_list):   # nnunet_plan.crossval_splits' five folds
            raise ValueError(f"`folds` names fold {max(fold_list)}: the split has the folds 0 .. 4, and nnU-Net's random 80:20 split for "
                             "fold numbers beyond it is not covered")
        import torch.distributed as dist
        world = dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1
        rank = dist.get_rank() if world > 1 else 0
        print("\033[32m[LDiffusion] Preparing data by L-Diffusion...\033[0m")
        pipeline, unet, _ = self.load_ldiffusion(ldiffusion_weight, diffusion_path)
        if num_classes is None:
            num_classes = self.num_classes
        if train_images is None or train_labels is None or test_images is None or test_labels is None:
            if self.train_loader is None or self.val_loader is None:
                raise ValueError("train_loader/val_loader are required when explicit nnUNet data lists are not provided")
            train_images, train_labels = self.train_loader.dataset.image_dir, self.train_loader.dataset.label_dir
            test_images, test_labels = self.val_loader.dataset.image_dir, self.val_loader.dataset.label_dir
        named = [None, None]
        if rank == 0:   # one writer: W ranks would race for the next free DatasetNNN_* under nnUNet_raw
            aligned_unet = unet
            if utils.check_images_same_size(train_images) and utils.check_images_same_size(test_images):   # only then does a sampler run (utils.py:213)
                self._ensure_ldiffusion_proj(pipeline, unet, ldiffusion_weight=ldiffusion_weight)
                aligned_unet = TextAlignedUNet(unet, self._get_text_embeddings(PROMPT, 1, pipeline, unet))
            batch_kwargs = {} if batch_images is None else dict(batch_images=batch_images, io_workers=io_workers)   # None: the call of before the keyword
            if ignore_pixel is not None:
                batch_kwargs["ignore_pixel"] = ignore_pixel
            if regions is not None:
                batch_kwargs.update(regions=regions, regions_class_order=regions_class_order)
            named = list(utils.create_nnunet_dataset(train_images, train_labels, test_images, test_labels, num_classes, pipeline, aligned_unet,
                                                     raw_dir=roots["nnUNet_raw"], **batch_kwargs))
        if world > 1:
            dist.broadcast_object_list(named, src=0)
            dist.barrier()
        new_num, dataset_name = named

        print("\033[32m[Segmentor-nnUNet] Data preprocessing and plan generation in progress...\033[0m")
        raw_dir = os.path.join(roots["nnUNet_raw"], dataset_name)
        with open(os.path.join(raw_dir, "dataset.json")) as f:
            dataset_json = json.load(f)
        keys = sorted(n[:-len("_0000.png")] for n in os.listdir(os.path.join(raw_dir, "imagesTr")) if n.endswith("_0000.png"))
        cases = {}
        for k in keys:   # NaturalImage2DIO: the PNG's channels first; the label PNG as it is
            img = np.array(Image.open(os.path.join(raw_dir, "imagesTr", k + "_0000.png")).convert("RGB"), np.uint8)
            seg = np.array(Image.open(os.path.join(raw_dir, "labelsTr", k + ".png")).convert("L"), np.uint8)
            cases[k] = (torch.from_numpy(img).permute(2, 0, 1).contiguous().to(self.device), torch.from_numpy(seg).to(self.device))
        budget = {} if num_foreground_voxels is None else {"num_foreground_voxels": num_foreground_voxels}
        pre_dir = os.path.join(roots["nnUNet_preprocessed"], dataset_name)
        os.makedirs(pre_dir, exist_ok=True)

        def save_json(name, obj, sort_keys=True):   # batchgenerators' save_json: indent 4, keys sorted unless the caller says otherwise
            with open(os.path.join(pre_dir, name), "w") as f:
                json.dump(obj, f, indent=4, sort_keys=sort_keys)

        def load_json(name):
            with open(os.path.join(pre_dir, name)) as f:
                return json.load(f)

        if rank == 0:
            save_json("dataset_fingerprint.json", nnunet_plan.extract_fingerprint([cases[k] for k in keys], dataset_json, **budget))
            fingerprint = load_json("dataset_fingerprint.json")   # the planner plans from the file (ExperimentPlanner.__init__ :46): its key order
            plans = nnunet_plan.plan_experiment(fingerprint, dataset_json, dataset_name)
            splits = nnunet_plan.crossval_splits(keys)
            save_json("nnUNetPlans.json", plans, sort_keys=False)
            save_json("dataset.json", dataset_json, sort_keys=False)
            save_json("splits_final.json", splits)
        if world > 1:   # the other ranks plan nothing: they read what rank 0 wrote
            dist.barrier()
            plans, splits = load_json("nnUNetPlans.json"), load_json("splits_final.json")

        print("\033[32m[Segmentor-nnUNet] Training is starting...\033[0m")
        spec = nnunet.network_spec(plans, "2d", dataset_json, accept_ignore=ignore_pixel is not None, accept_regions=regions is not None)
        cfg = plans["configurations"]["2d"]
        if "regions" in spec:
            store_labels = dict(regions=nnunet.region_spec(dataset_json["labels"], dataset_json["regions_class_order"]))
        else:
            store_labels = dict(labels=dataset_json["labels"])
        n_scales = spec["n_stages"] - 1
        if world > 1:
            batch, oversample = nnunet_train.rank_batch_sizes(cfg["batch_size"], world, nnunet_data.OVERSAMPLE_FOREGROUND)[rank]
            extra = {"oversample": oversample}
        else:
            batch, extra = cfg["batch_size"], {}
        model_dir = os.path.join(roots["nnUNet_results"], dataset_name, "nnUNetTrainer__nnUNetPlans__2d")
        if rank == 0:
            nnunet.write_trained_model_folder(model_dir, plans, dataset_json)
        self.training_logs, self.validation_summaries, self.crossval_summary = {}, {}, None
        for f in fold_list:   # one nnUNetv2_train per fold: a fresh network, stores and loaders; `folds=None` makes exactly the calls of before the keyword
            of_fold = {} if folds is None else {"fold": f}
            stores = [nnunet_data.CaseStore([cases[k] for k in splits[f][part]], spec["normalization_schemes"], spec["n_heads"], device=self.device,
                                            prefilter="device", build="device", **store_labels) for part in ("train", "val")]
            first_seed = 2 * rank + 2 * world * f
            loaders = [nnunet_data.PatchLoader(store, spec["patch_size"], batch, n_scales, seed=seed, train=train, **extra)
                       for store, seed, train in ((stores[0], first_seed, True), (stores[1], first_seed + 1, False))]
            self.tissue_loaders = loaders
            ignore = {}
            if spec.get("ignore_label") is not None:   # nnUNetTrainer keeps the dataset.json it was built with, ignore entry included, in the checkpoint's init_args
                ignore = dict(ignore_label=spec["ignore_label"], init_args={"configuration": "2d", "fold": f, "dataset_json": dataset_json})
            if "regions" in spec:
                ignore.update(region_loss=region_loss, init_args={"configuration": "2d", "fold": f, "dataset_json": dataset_json})
            if folds is not None:
                ignore.setdefault("init_args", {"configuration": "2d", "fold": f})
            state = nnunet_train.initial_state_dict(spec) if folds is None else nnunet_train.initial_state_dict(spec, seed=f)
            trainer = nnunet_train.Trainer(spec, state, cfg["batch_dice"], num_epochs=epochs, device=self.device, wgrad_route=wgrad_route, **ignore)
            self.training_log = trainer.run_training(loaders[0], loaders[1], os.path.join(model_dir, f"fold_{f}"), iterations_per_epoch=iterations_per_epoch,
                                                     val_iterations=val_iterations)
            self.training_logs[f] = self.training_log
            if validate or postprocessing:
                from . import nnunet_post
                self.validation_summary = nnunet_post.validate_fold(model_dir, cases, splits[f]["val"], checkpoint_name=validation_checkpoint, io_workers=io_workers,
                                                                    **of_fold)
                self.validation_summaries[f] = self.validation_summary
            del trainer, stores
        if validate or postprocessing:
            fit_dir = os.path.join(model_dir, f"fold_{fold_list[0]}", "validation")
            if len(fold_list) > 1:   # find_best_configuration's order: merge the folds, score the merged folder, fit the postprocessing there
                fit_dir = nnunet_post.crossval_folder(model_dir, fold_list)
                if rank == 0:
                    self.crossval_summary = nnunet_post.accumulate_cv_results(model_dir, fold_list, os.path.join(raw_dir, "labelsTr"), device=self.device,
                                                                              io_workers=io_workers)
            if postprocessing and rank == 0:
                nnunet_post.determine_postprocessing_folder(fit_dir, os.path.join(raw_dir, "labelsTr"), model_dir, device=self.device, io_workers=io_workers)
            if world > 1 and (postprocessing or len(fold_list) > 1):
                dist.barrier()
        return model_dir

    def train_cell_model(self, epochs, ldiffusion_weight, diffusion_path, *, cell_weights, instances=None, fit_classifier=True, cache_features=True, lr=1e-4,
                         save_root=None, seed=None, text_embeddings=None):
        """segmentor.py:243-299, the cell head's training stage; returns the folder that holds the best epoch's `cellclassifier.pth` (what
        `inference_cell_model(segmentor_weight=...)` takes), or None when no epoch's validation Dice beat 0.0 (nothing is written then).

        What the reference's loop does, as its code reads (DESIGN.md section 7 "Cell head, training"):
          1. no parameter ever gets a gradient -- CellSegClassifier.forward (model/conductor.py:175-233) runs encoder and adapter under no_grad, picks classes with
             .item() and paints a fresh leaf tensor, so loss.backward() reaches nothing and AdamW(lr=1e-4) skips every parameter, weight decay included;
          2. the state dict changes all the same: `self.model.train()` puts the trunk's BatchNorms in training mode, every training image's forward normalises
             with the batch statistics of ALL of that image's crops and moves running_mean / running_var (momentum 0.1, unbiased variance) and
             num_batches_tracked; validation then runs in eval mode on those, and the best mean micro_dice (> 0.0) writes the checkpoint;
          3. the loop feeds the head the augmented image in [0, 1], un-normalised (`CellSegClassifier(input_norm=False)`).
        `fit_classifier=False` reproduces exactly that: BatchNorm statistic adaptation plus best-epoch selection.  The default also fits the only parameters the
        reference leaves outside no_grad, `classifier.{weight,bias}`: per training image, logits = features @ W.T + b in fp32 torch, the cross-entropy over the
        instances whose target (`cellhead.instance_targets`: the majority class of the mask under the instance) is >= 1, one step of
        torch.optim.AdamW([W, b], lr=lr) -- the reference's optimizer where a gradient can reach.
        The "Loss" of the epoch lines is the epoch's MEAN CROSS-ENTROPY of those steps (0.0 with fit_classifier=False), NOT the reference's CombinedLoss: that loss
        only reports a number there (nothing depends on it), and it cannot even be evaluated unless num_classes == 4 (model/loss.py:176 hard-codes four class weights).

        `cell_weights` (required): a CellSegClassifier state dict or a path to one.  The reference starts from torchvision's ImageNet weights, which it downloads;
        this build never downloads anything.  `instances`: the label-map callable (Cellpose where installed), called once per image with the [H, W, 3] float32
        image in [0, 1]; its result is kept.  An image without a kept instance changes nothing (the reference returns before the encoder runs).
        `cache_features`: no trunk weight moves, so an image's features and batch statistics are the same in every epoch: they are kept on the host after epoch 1
        (ResNet152: about 0.6 MB of statistics per image) and the running-statistics update and the head steps are replayed from them; validation still runs
        the trunk, whose folded weights change with the running statistics.  The written tensors are bit-identical either way.
        `seed` seeds the loaders' shuffle.  `save_root`: default ./LDiffusion/train_save/cellclassifier; the checkpoint goes to <save_root>/<yy_mm_dd>/.
        Under an initialised process group rank 0 trains, the others wait, and every rank returns the folder name rank 0 broadcasts."""
        import torch.distributed as dist
        kw = dict(cell_weights=cell_weights, instances=instances, fit_classifier=fit_classifier, cache_features=cache_features, lr=lr, save_root=save_root, seed=seed,
                  text_embeddings=text_embeddings)
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return self._train_cell_model_rank0(epochs, ldiffusion_weight, diffusion_path, **kw)
        out = [None, None]   # (folder, error text)
        if dist.get_rank() == 0:
            try:
                out[0] = self._train_cell_model_rank0(epochs, ldiffusion_weight, diffusion_path, **kw)
            except Exception as e:   # noqa: BLE001  (the other ranks must not wait forever)
                out[1] = f"{type(e).__name__}: {e}"
        dist.barrier()
        dist.broadcast_object_list(out, src=0)
        if out[1] is not None:
            raise RuntimeError(f"train_cell_model failed on rank 0: {out[1]}")
        return out[0]

    def _train_cell_model_rank0(self, epochs, ldiffusion_weight, diffusion_path, *, cell_weights, instances, fit_classifier, cache_features, lr, save_root, seed,
                                text_embeddings):
        from datetime import datetime
        from . import cellhead
        print("Training cell-level model...")
        if cell_weights is None:
            raise ValueError("train_cell_model: cell_weights (a CellSegClassifier state dict or the path of one) is required; nothing is downloaded here")
        sd = cell_weights if isinstance(cell_weights, dict) else cellhead.read_cellclassifier(cell_weights)
        nc, layers, width, adapter = cellhead.infer_spec(sd)
        if nc != int(self.num_classes):
            raise ValueError(f"train_cell_model: cell_weights classify {nc} classes, this Segmentor has num_classes = {self.num_classes}")
        cellhead.check_state_dict(sd, nc, layers, width, adapter)
        counters = [k for k, shape in cellhead.param_shapes(nc, layers, width, adapter, counters=True).items() if k.endswith("num_batches_tracked")]
        sd = {k: (v.detach().to("cpu", torch.int64).clone() if k.endswith("num_batches_tracked") else v.detach().to("cpu", torch.float32).clone()) for k, v in sd.items()}
        for k in counters:
            sd.setdefault(k, torch.zeros((), dtype=torch.int64))
        pipeline, unet, vae = self.load_ldiffusion(ldiffusion_weight, diffusion_path)
        current_date = datetime.now().strftime("%y_%m_%d")
        if text_embeddings is None:
            text_embeddings = self._get_text_embeddings(PROMPT, 1, pipeline, unet)
        gens = [None, None]
        if seed is not None:
            gens = [torch.Generator().manual_seed(int(seed)), torch.Generator().manual_seed(int(seed) + 1)]

        def augment(inputs, pipeline, unet, vae):
            return self.ldiffusion_augment(inputs, pipeline, unet, vae, text_embeddings=text_embeddings)

        aug_train_loader = self.build_augmented_dataloader(self.train_loader, augment, pipeline, unet, vae, self.device, batch_size=1, category="Train", generator=gens[0],
                                                           with_index=True)
        aug_val_loader = self.build_augmented_dataloader(self.val_loader, augment, pipeline, unet, vae, self.device, batch_size=1, category="Validation", generator=gens[1],
                                                         with_index=True)

        # the trunk's weights never move: ONE training-mode handle serves every epoch (its running statistics and linear head are not read by forward_train's features)
        trainer = cellhead.CellSegClassifier(nc, sd, self.device, instances=instances, input_norm=False, train=True)
        W = sd["classifier.weight"].clone().requires_grad_(True)
        b = sd["classifier.bias"].clone().requires_grad_(True)
        optimizer = torch.optim.AdamW([W, b], lr=lr) if fit_classifier else None
        label_maps = {"train": {}, "val": {}}
        cache = {}
        self.cell_training_log = {"loss": [], "dice": [], "first_loss": None}

        def to_u8(img):   # [1, 3, H, W] in [0, 1] = u8 / 255 -> the u8 image ((patch * 255).astype(uint8) is the identity on grey levels, cellhead.build_lut)
            return (img[0].permute(1, 2, 0) * 255.0).round().clamp(0, 255).to(torch.uint8).contiguous().to(self.device)

        def label_map(part, idx, head, rgb_u8):
            if idx not in label_maps[part]:
                label_maps[part][idx] = head._label_map(rgb_u8, instances).to(torch.int64).cpu()
            return label_maps[part][idx]

        def train_pass(idx, inputs, masks):
            """(features, batch_mean, batch_var, targets) on the host, or None for an image without a kept instance."""
            rgb_u8 = to_u8(inputs)
            labels = label_map("train", idx, trainer, rgb_u8).to(self.device)
            if tuple(labels.shape) != tuple(rgb_u8.shape[:2]):
                raise ValueError(f"train_cell_model: label map {list(labels.shape)} against image {list(rgb_u8.shape[:2])}")
            ids, boxes = cellhead.instance_boxes(labels)
            if ids.numel() == 0:
                return None
            feats, bm, bv = trainer.net.forward_train(trainer.crops(rgb_u8, boxes))   # all N crops of the image in one batch, as the reference's forward has them
            trainer.net.check_finite()
            targets = cellhead.instance_targets(labels, masks[0].to(self.device), nc)
            return feats.cpu(), bm.cpu(), bv.cpu(), targets.cpu()

        best_dir, checkpoint = None, 0.0
        for epoch in range(epochs):
            losses = []
            for inputs, masks, index in aug_train_loader:
                idx = int(index[0])
                if cache_features and idx in cache:
                    got = cache[idx]
                else:
                    got = train_pass(idx, inputs, masks)
                    if cache_features:
                        cache[idx] = got
                if got is None:
                    continue
                feats, bm, bv, targets = got
                cellhead.ema_update(sd, trainer.net.bn_layout, bm, bv)
                sel = targets >= 1
                if fit_classifier and bool(sel.any()):
                    optimizer.zero_grad()
                    loss = F.cross_entropy(feats[sel] @ W.t() + b, targets[sel])
                    loss.backward()
                    optimizer.step()
                    losses.append(loss.item())
                    if self.cell_training_log["first_loss"] is None:
                        self.cell_training_log["first_loss"] = loss.item()
            avg_running_loss = sum(losses) / len(losses) if losses else 0.0
            print(f"Epoch {epoch + 11}/{epochs + 10}, Loss: {avg_running_loss:.4f}")
            sd["classifier.weight"], sd["classifier.bias"] = W.detach().clone(), b.detach().clone()

            head = cellhead.CellSegClassifier(nc, sd, self.device, instances=instances, input_norm=False)   # eval mode on the current state
            total_dice = 0.0
            for images, labels, index in aug_val_loader:
                rgb_u8 = to_u8(images)
                lm = label_map("val", int(index[0]), head, rgb_u8)
                pred = head.predict_mask(rgb_u8, labels=lm)
                truth = labels.to(self.device)
                if tuple(truth.shape[-2:]) != tuple(pred.shape):
                    truth = F.interpolate(truth[:, None].float(), size=tuple(pred.shape), mode="nearest")[:, 0]
                _, avg_dice = self.micro_dice(predicted_labels=pred[None].contiguous(), true_labels=truth.to(torch.int64).contiguous(), num_classes=nc)
                total_dice += avg_dice.item()
            head.net.check_finite()
            del head
            total_dice = total_dice / len(aug_val_loader)
            self.cell_training_log["loss"].append(avg_running_loss)
            self.cell_training_log["dice"].append(total_dice)
            if total_dice > checkpoint:
                checkpoint = total_dice
                best_dir = os.path.join(save_root if save_root is not None else "./LDiffusion/train_save/cellclassifier", current_date)
                os.makedirs(best_dir, exist_ok=True)
                torch.save({k: v.detach().clone() for k, v in sd.items()}, os.path.join(best_dir, "cellclassifier.pth"))
                print(f"\033[32mNew Best Validation Dice Score: {total_dice:.4f}\033[0m")
            else:
                print(f"Validation Dice Score: {total_dice:.4f}")
        return best_dir

    def _cell_head(self, weight_dir):
        """The cell head of a `segmentor_weight` folder (cellclassifier.pth), built once per (file, mtime)."""
        from . import cellhead
        ckpt = os.path.join(weight_dir, "cellclassifier.pth")
        key = (os.path.abspath(ckpt), os.path.getmtime(ckpt))
        cache = getattr(self, "_cell_heads", None)
        if cache is None:
            cache = self._cell_heads = {}
        if key not in cache:
            cache.clear()
            cache[key] = cellhead.CellSegClassifier(self.num_classes, cellhead.read_cellclassifier(ckpt), self.device)
        return cache[key]

    @torch.no_grad()
    def inference_cell_model(self, image_path, diffusion_path, ldiffusion_weight, segmentor_weight, head=None, text_embeddings=None, instances=None):
        """segmentor.py:490-545.  The cell head is either
        * built from `segmentor_weight`, the folder that holds `cellclassifier.pth` (the reference's CellSegClassifier state_dict, :497), when `head` is
          None: the ResNet152 instance classifier on the HIP library (`cellhead.py`; cached on this Segmentor).  `instances` = the callable that maps
          the normalised HWC float32 image to an int label map (Cellpose `cyto2` in the reference: third-party, built lazily if it imports); or
        * injected: `head(decoded_rgb_float[1,3,1024,1024] normalised) -> logits [1,C,H,W]`.
        Neither: RuntimeError."""
        from PIL import Image
        built = None
        if head is None:
            if not (isinstance(segmentor_weight, (str, os.PathLike)) and os.path.isfile(os.path.join(segmentor_weight, "cellclassifier.pth"))):
                raise RuntimeError("inference_cell_model: the cell head needs `segmentor_weight` to be the folder that holds cellclassifier.pth "
                                   "(CellSegClassifier's state_dict; Cellpose stays third-party: `instances=`), or pass `head=`")
            built = self._cell_head(segmentor_weight)
        pipeline, unet, _ = self.load_ldiffusion(ldiffusion_weight, diffusion_path)
        image = Image.open(image_path).convert("RGB")
        width, height = image.size
        mean = torch.tensor(IMAGENET_MEAN, device=self.device).view(1, 3, 1, 1)
        std = torch.tensor(IMAGENET_STD, device=self.device).view(1, 3, 1, 1)
        x = torch.from_numpy(np.asarray(image.resize((1024, 1024), Image.BILINEAR), np.float32) / 255.0).permute(2, 0, 1)[None].to(self.device)
        x = (x - mean) / std
        if text_embeddings is None:
            text_embeddings = self._get_text_embeddings(PROMPT, 1, pipeline, unet)
        out = self._one_pass(x, text_embeddings, pipeline, unet)
        decoded = Image.fromarray(out["rgb"][0].cpu().numpy())
        self._sampler.check_finite()   # fp16 overflow in either graph raises here instead of yielding a plausible-looking mask
        if built is not None:
            mask = built.predict_mask(out["rgb"][0], instances=instances)   # the decoded uint8 image itself (the head's table restates the reference's float round trip); `instances` holds for this call only
            built.net.check_finite()
            mask = mask.cpu().numpy()
        else:
            model_input = (out["rgb"].permute(0, 3, 1, 2).float() / 255.0 - mean) / std
            logits = head(model_input)
            mask = argmax_mask(logits)[0].cpu().numpy()
        mask = np.array(Image.fromarray(mask.astype(np.uint8)).resize((width, height), resample=Image.NEAREST))
        return decoded.resize((width, height), Image.BILINEAR), mask

    def _tissue_head(self, model_dir, use_folds=None):
        """The nnU-Net head of a trained-model folder, built once per (folder, checkpoint mtime); with `use_folds` the `nnunet.FoldEnsemble` of those folds,
        built once per (folder, folds, every fold's checkpoint mtime)."""
        from . import nnunet
        folds = (0,) if use_folds is None else nnunet.check_folds(use_folds)
        mtimes = []
        for f in folds:
            ckpt = os.path.join(model_dir, f"fold_{f}", "checkpoint_best.pth")
            mtimes.append(os.path.getmtime(ckpt) if os.path.exists(ckpt) else None)
        key = (os.path.abspath(model_dir), mtimes[0]) if use_folds is None else (os.path.abspath(model_dir), folds, tuple(mtimes))
        cache = getattr(self, "_tissue_heads", None)
        if cache is None:
            cache = self._tissue_heads = {}
        if key not in cache:
            cache.clear()
            if use_folds is None:
                cache[key] = nnunet.load_trained_model_folder(model_dir, 0, "checkpoint_best.pth", device=self.device)
            else:
                cache[key] = nnunet.load_fold_ensemble(model_dir, folds, "checkpoint_best.pth", device=self.device)
        return cache[key]

    @staticmethod
    def _check_head_finite(head):
        """An fp16 overflow inside the head (any fold of an ensemble) raises instead of yielding a plausible-looking mask."""
        for model in getattr(head, "models", (head,)):
            model.network.check_finite()

    @torch.no_grad()
    def _tissue_folder_batched(self, head, image_path, output_path, diffusion_path, ldiffusion_weight, text_embeddings, tile_size, tile_step_size, mirror_axes, batch_tiles,
                               batch_images, postprocess=None):
        """Folder mode of `inference_tissue_model_nnUNetv2` with `batch_images`: one pipeline for the folder, the sampler in batches, the head per image."""
        from PIL import Image
        from . import imgio
        if isinstance(batch_images, bool) or not isinstance(batch_images, int) or batch_images < 1:
            raise ValueError(f"batch_images = {batch_images!r}: an integer >= 1")
        names = [n for n in sorted(os.listdir(image_path)) if n.lower().endswith((".png", ".jpg", ".jpeg", ".tif", ".tiff", ".bmp"))]
        axes = "checkpoint" if mirror_axes is None else mirror_axes

        def head_mask(name, data):   # data [3, H, W] float on the device, what the PNG the reference writes would hold
            mask = head.predict_mask(data, tile_size, tile_step_size, axes, batch_tiles=batch_tiles, postprocess=postprocess)
            self._check_head_finite(head)
            Image.fromarray(mask.cpu().numpy()).save(os.path.join(output_path, os.path.splitext(name)[0] + ".png"))

        groups = {}   # source size -> names, in name order
        for name in names:
            with Image.open(os.path.join(image_path, name)) as im:
                w, h = im.size
            if w == h:
                groups.setdefault((w, h), []).append(name)
            else:                                                                             # non-square: no diffusion (segmentor.py:449-450)
                with Image.open(os.path.join(image_path, name)) as im:
                    head_mask(name, torch.from_numpy(np.array(im.convert("RGB"), np.uint8)).to(self.device).permute(2, 0, 1).float())
        if not groups:
            return
        pipeline, unet, _ = self.load_ldiffusion(ldiffusion_weight, diffusion_path)
        previous = (unet.plan_batch, pipeline.vae.plan_batch)
        try:
            pipeline.set_plan_batch(batch_images)
            if text_embeddings is None:
                text_embeddings = self._get_text_embeddings(PROMPT, 1, pipeline, unet)
            for group in groups.values():
                for i in range(0, len(group), batch_images):
                    part = group[i:i + batch_images]
                    host = []
                    for name in part:
                        with Image.open(os.path.join(image_path, name)) as im:
                            host.append(np.asarray(im.convert("RGB"), np.uint8))
                    x = imgio.resize_normalize(torch.from_numpy(np.stack(host)).to(self.device), (1024, 1024), IMAGENET_MEAN, IMAGENET_STD)
                    rgb = self._one_pass(x, text_embeddings, pipeline, unet)["rgb"]           # [b, 1024, 1024, 3] u8, on the device
                    self._sampler.check_finite()   # before any mask of the batch is written
                    for j, name in enumerate(part):
                        head_mask(name, rgb[j].permute(2, 0, 1).float())
        finally:
            unet.set_plan_batch(previous[0])
            pipeline.vae.set_plan_batch(previous[1])

    @torch.no_grad()
    def inference_tissue_model_nnUNetv2(self, image_path, diffusion_path, ldiffusion_weight, segmentor_weight, output_path=None,
                                        predictor=None, text_embeddings=None, tile_size=None, tile_step_size=0.5,
                                        mirror_axes=None, num_heads=None, batch_tiles=None, batch_images=None, postprocess=False, use_folds=None):
        """segmentor.py:388-488.  The tissue head is either
        * built from `segmentor_weight`, a trained-model folder as the reference's nnUNetPredictor reads it (dataset.json, plans.json,
          fold_0/checkpoint_best.pth; :463-468), when `predictor` is None: nnU-Net v2's 2-D PlainConvUNet on the HIP library (`nnunet.py`; cached on this
          Segmentor), with nnU-Net's preprocessing (crop to non-zero, the plans' normalisation) in front of the sliding window, the plans' patch size and
          the checkpoint's mirror axes unless `tile_size` / `mirror_axes` name others, pixels outside the crop box label 0; or
        * injected as `predictor` (then `tile_size` / `mirror_axes` default to (512, 512) / (0, 1), the input is the raw 0..255 image, no crop).
        Neither: RuntimeError.
        * `image_path` a directory: the reference hands the folder to nnU-Net's file predictor and returns `(None, None)`
          (:399-421).  Here `predictor(image_path, output_path)` is called if it accepts two arguments (a file-level predictor),
          else every image of the folder goes through the single-image path and its mask is written as PNG to `output_path`.
        * a single image: Resize(1024) + ImageNet-normalise -> one-pass sampler ONLY when width == height (:427); other aspect
          ratios skip the diffusion and feed the image as it is (:449-450).  The decoded RGB stays on the device, is handed to
          `predictor([1, 3, th, tw] float in 0..255 scale as the PNG would hold) -> [1, heads, th, tw]` tile by tile
          (nnU-Net order, Gaussian fp16 accumulation, mirroring), arg-max on the device, and `(decoded PIL image, uint8 mask)`
          is returned like :486-488.
        * batch_tiles: None = one head call per tile and mirror variant; an integer = the batched sliding window (`tiling.predict_sliding_window_batched`), for the
          library's head and an injected `predictor` alike, in folder mode too.  An injected predictor must then accept a batch,
          `predictor([batch_tiles * M, 3, th, tw]) -> [batch_tiles * M, heads, th, tw]` (M = 1, 2 or 4 mirror variants), and treat its entries independently.
        * batch_images (folder mode of the library's head; None = one call per file, as above): the square images of the folder go through the sampler in
          batches of up to `batch_images`, grouped by source size in name order, behind `imgio.resize_normalize`, under `set_plan_batch(batch_images)` (the
          previous plan batch comes back afterwards); each decoded image then goes to the head as above and `batch_tiles` is unaffected; non-square images
          skip the diffusion as above.  The mask files are those of the per-image path under the same plan batch.
        * postprocess (False: the masks as predicted): True = nnU-Net's fitted postprocessing, read from `<segmentor_weight>/fold_0/validation/postprocessing.json`
          (what `train_tissue_model_nnUNetv2(postprocessing=True)` writes; a missing file raises FileNotFoundError naming the path), or the path of such a
          file, or `(fns, kwargs)`; applied to every finished mask on the device (`nnunet_post.apply_postprocessing`), single image and folder alike.
        * use_folds (the library's head; None = fold 0, the head as above): a sequence of fold numbers = `nnunet.load_fold_ensemble` of
          `fold_<f>/checkpoint_best.pth`, the reference's `use_folds=` (:466): the folds' logits are averaged on the device before the arg-max
          (`tiling.predict_sliding_window_ensemble`), single image, folder and `batch_images` folder alike.  With more than one fold `postprocess=True`
          reads `<segmentor_weight>/crossval_results_folds_<f0>_<f1>.../postprocessing.json`, the record fitted on the folds' merged validation."""
        from PIL import Image
        from . import tiling
        if use_folds is not None:
            from . import nnunet
            use_folds = nnunet.check_folds(use_folds)
            if predictor is not None:
                raise ValueError("inference_tissue_model_nnUNetv2: `use_folds` names folds of `segmentor_weight`; an injected `predictor` has none")
        post = None   # (fns, kwargs), read once
        if postprocess is not None and postprocess is not False:
            from . import nnunet_post
            if postprocess is True:
                weight = os.fspath(segmentor_weight) if isinstance(segmentor_weight, (str, os.PathLike)) else str(segmentor_weight)
                if use_folds is not None and len(use_folds) > 1:
                    postprocess = os.path.join(nnunet_post.crossval_folder(weight, use_folds), "postprocessing.json")
                else:
                    postprocess = os.path.join(weight, f"fold_{0 if use_folds is None else use_folds[0]}", "validation", "postprocessing.json")
            post = nnunet_post.load_postprocessing(postprocess) if isinstance(postprocess, (str, os.PathLike)) else (list(postprocess[0]), list(postprocess[1]))
        keep = {} if post is None else {"postprocess": post}   # nothing new goes downstream without the keyword
        head = None
        if predictor is None:
            if not (isinstance(segmentor_weight, (str, os.PathLike)) and os.path.isfile(os.path.join(segmentor_weight, "plans.json"))):
                raise RuntimeError("inference_tissue_model_nnUNetv2: the nnU-Net tissue head needs `segmentor_weight` to be a trained-model folder "
                                   "(dataset.json, plans.json, fold_0/checkpoint_best.pth), or pass `predictor=`")
            head = self._tissue_head(segmentor_weight) if use_folds is None else self._tissue_head(segmentor_weight, use_folds)
        if head is not None and os.path.isdir(image_path):   # every image of the folder through the same head
            if not output_path:
                raise ValueError("When image_path is a folder, output_path must be specified!")
            os.makedirs(output_path, exist_ok=True)
            if batch_images is not None:
                self._tissue_folder_batched(head, image_path, output_path, diffusion_path, ldiffusion_weight, text_embeddings, tile_size, tile_step_size, mirror_axes,
                                            batch_tiles, batch_images, **keep)
                return None, None
            for name in sorted(os.listdir(image_path)):
                if name.lower().endswith((".png", ".jpg", ".jpeg", ".tif", ".tiff", ".bmp")):
                    _, m = self.inference_tissue_model_nnUNetv2(os.path.join(image_path, name), diffusion_path, ldiffusion_weight, segmentor_weight,
                                                                None, None, text_embeddings, tile_size, tile_step_size, mirror_axes, num_heads, batch_tiles, **keep,
                                                                **({} if use_folds is None else {"use_folds": use_folds}))
                    Image.fromarray(m).save(os.path.join(output_path, os.path.splitext(name)[0] + ".png"))
            return None, None   # batch mode returns no single mask (segmentor.py:421)
        if head is None:
            tile_size = (512, 512) if tile_size is None else tile_size
            mirror_axes = (0, 1) if mirror_axes is None else mirror_axes
        if os.path.isdir(image_path):
            if not output_path:
                raise ValueError("When image_path is a folder, output_path must be specified!")
            import inspect
            try:
                n_args = len(inspect.signature(predictor).parameters)
            except (TypeError, ValueError):
                n_args = 1
            if n_args >= 2:
                predictor(image_path, output_path)
                return None, None
            os.makedirs(output_path, exist_ok=True)
            for name in sorted(os.listdir(image_path)):
                if name.lower().endswith((".png", ".jpg", ".jpeg", ".tif", ".tiff", ".bmp")):
                    _, m = self.inference_tissue_model_nnUNetv2(os.path.join(image_path, name), diffusion_path, ldiffusion_weight, segmentor_weight,
                                                                None, predictor, text_embeddings, tile_size, tile_step_size, mirror_axes, num_heads, batch_tiles, **keep)
                    Image.fromarray(m).save(os.path.join(output_path, os.path.splitext(name)[0] + ".png"))
            return None, None   # batch mode returns no single mask (segmentor.py:421)
        pipeline, unet, _ = self.load_ldiffusion(ldiffusion_weight, diffusion_path)
        image = Image.open(image_path).convert("RGB")
        width, height = image.size
        if width == height:
            mean = torch.tensor(IMAGENET_MEAN, device=self.device).view(1, 3, 1, 1)
            std = torch.tensor(IMAGENET_STD, device=self.device).view(1, 3, 1, 1)
            x = torch.from_numpy(np.asarray(image.resize((1024, 1024), Image.BILINEAR), np.float32) / 255.0).permute(2, 0, 1)[None].to(self.device)
            if text_embeddings is None:
                text_embeddings = self._get_text_embeddings(PROMPT, 1, pipeline, unet)
            rgb = self._one_pass((x - mean) / std, text_embeddings, pipeline, unet)["rgb"]   # [1,1024,1024,3] u8, on the device
            decoded = Image.fromarray(rgb[0].cpu().numpy())
            self._sampler.check_finite()   # fp16 overflow in either graph raises here instead of yielding a plausible-looking mask
        else:                                                                                 # non-square: no diffusion (segmentor.py:449-450)
            rgb = torch.from_numpy(np.array(image, np.uint8))[None].to(self.device)
            decoded = image
        data = rgb[0].permute(2, 0, 1).float()                                                # what the PNG the reference writes would hold
        if head is not None:
            mask = head.predict_mask(data, tile_size, tile_step_size, "checkpoint" if mirror_axes is None else mirror_axes, batch_tiles=batch_tiles, **keep)
            self._check_head_finite(head)
            return decoded, mask.cpu().numpy()
        heads = int(num_heads if num_heads is not None else self.num_classes)
        th, tw = min(tile_size[0], data.shape[1]), min(tile_size[1], data.shape[2])
        if batch_tiles is not None:
            mask = tiling.predict_sliding_window_batched(data, predictor, heads, (th, tw), tile_step_size, True, mirror_axes, batch_tiles=int(batch_tiles), return_mask=True)
        else:
            logits = tiling.predict_sliding_window_return_logits(data, predictor, heads, (th, tw), tile_step_size, True, mirror_axes)
            mask = argmax_mask(logits[None].float())[0]
        if post is not None:
            mask = nnunet_post.apply_postprocessing(mask.contiguous(), *post)
        return decoded, mask.cpu().numpy()
