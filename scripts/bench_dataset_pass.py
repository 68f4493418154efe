"""The one-pass diffusion of a dataset's images (utils.create_nnunet_dataset's image loop) at SD-v1.5 width with synthetic weights, over synthetic
1000 x 1000 PNGs the script makes itself: where the per-image pass spends its time, and images/s of the batched pass against it.
  1. the per-image path (`batch_images=None`: Image.open + convert, PIL resize + numpy + H2D, sampler, D2H, PNG save) split into its stages, the
     device synchronised between them;
  2. images/s for batch_images in {None, 2, 4, 5, 8} x io_workers in {0, 4, 8} (None has no pool: one row), the configurations alternated in one
     process, two warm-up images each, median and min-max over the rounds; a configuration the library refuses is listed with its message;
  3. imgio.resize_normalize alone at 1000^2 -> 1024^2, B = 8, beside the host's Image.resize + numpy + H2D + normalise for the same eight images.
Everything it reads it has written itself, under --workdir (default build/dataset_pass_bench in the repository).
usage: python scripts/bench_dataset_pass.py [--images 32] [--rounds 3] [--out profiles/dataset_pass_bench.txt]"""
import argparse
import os
import shutil
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCHES = (None, 2, 4, 5, 8)   # 5: the most images the sampler takes per call at 1024^2 (the VAE's parity conv3x3 decodes B * 8192 * 4 tile indices, squared times the channel tiles below 2^32); 8 is refused
WORKERS = (0, 4, 8)
PROMPT_IDS = [49406, 320, 24857, 5471, 49407]


class Tok:   # a stand-in tokenizer / text encoder: the wrapper's cached embeddings replace what they make (utils.copy_or_convert_image)
    def __call__(self, prompts, **kw):
        return {"input_ids": [list(PROMPT_IDS) for _ in prompts]}


class Enc:
    def __init__(self, torch):
        self.table = torch.randn((49408, 768), generator=torch.Generator().manual_seed(99)) * 0.5

    def __call__(self, ids):
        return {"last_hidden_state": self.table.to(ids.device)[ids]}


def make_images(np, Image, folder, n, side=1000):
    """Smooth colour fields with mild noise: PNG decode / encode costs nearer a stained slide's than white noise's."""
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:side, 0:side].astype(np.float32) / side
    paths = []
    for i in range(n):
        f = rng.uniform(2, 9, (3, 2))
        field = np.stack([0.5 + 0.35 * np.sin(2 * np.pi * (f[c, 0] * yy + f[c, 1] * xx) + i) for c in range(3)], -1)
        img = np.clip(field * 255 + rng.normal(0, 6, (side, side, 3)), 0, 255).astype(np.uint8)
        paths.append(os.path.join(folder, f"src_{i:03d}.png"))
        Image.fromarray(img).save(paths[-1])
    return paths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workdir", default=os.path.join(ROOT, "build", "dataset_pass_bench"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image

    from ldiffusion_amd import configs, imgio, utils as U, weights
    from ldiffusion_amd.models import AutoencoderKL, UNet2DConditionModel
    from ldiffusion_amd.pipeline import StableDiffusionImg2ImgPipeline
    from ldiffusion_amd.segmentor import TextAlignedUNet
    dev = "cuda:0"
    shutil.rmtree(a.workdir, ignore_errors=True)
    os.makedirs(os.path.join(a.workdir, "out"))
    paths = make_images(np, Image, a.workdir, a.images)
    dsts = [os.path.join(a.workdir, "out", f"dst_{i:03d}.png") for i in range(a.images)]
    ucfg, vcfg = configs.SD15_UNET, configs.SD15_VAE
    unet = UNet2DConditionModel(ucfg, weights.synthetic_state_dict(weights.unet_param_shapes(ucfg), 42, fp16_values=True), dev)
    vae = AutoencoderKL(vcfg, weights.synthetic_state_dict(weights.vae_param_shapes(vcfg), 43, fp16_values=True), dev)
    pipe = StableDiffusionImg2ImgPipeline(vae, unet, tokenizer=Tok(), text_encoder=Enc(torch))
    cached = (torch.randn((1, 77, 768), generator=torch.Generator().manual_seed(7)) * 0.5).to(dev)
    wrapped = TextAlignedUNet(unet, cached)
    lines = [f"# scripts/bench_dataset_pass.py --images {a.images} --rounds {a.rounds}: SD-v1.5 width, synthetic weights, {a.images} synthetic 1000 x 1000 PNGs -> 1024 x 1024; "
             f"{torch.cuda.get_device_name(0)}; Pillow {Image.__version__}"]

    def say(s=""):
        lines.append(s)
        print(s, flush=True)

    def per_image(idx):
        for i in idx:
            U.copy_or_convert_image(Image.open(paths[i]).convert("RGB"), paths[i], dsts[i], pipe, wrapped, True)

    # ---- 1. the per-image path, stage by stage (its own statements, a synchronisation between the stages)
    per_image(range(2))
    sampler = U._sampler(pipe, unet)
    mean = torch.tensor(U.IMAGENET_MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(U.IMAGENET_STD, device=dev).view(1, 3, 1, 1)
    stages = {k: [] for k in ("decode", "resize+H2D", "text", "sampler", "D2H", "save")}
    for i in range(a.images):
        t = [time.perf_counter()]

        def lap():
            torch.cuda.synchronize()
            t.append(time.perf_counter())
        img = Image.open(paths[i]).convert("RGB"); lap()
        x = torch.from_numpy(np.asarray(img.convert("RGB").resize((1024, 1024), Image.BILINEAR), np.float32) / 255.0).permute(2, 0, 1)[None].to(dev); lap()
        emb, base = U._image_text_embeddings(pipe, wrapped, dev); lap()
        out = sampler.sample((x - mean) / std, emb.to(device=dev, dtype=torch.float32)[:1], 1, want_features=False, want_rgb=True); lap()
        rgb = out["rgb"][0].cpu().numpy(); sampler.check_finite(); lap()
        Image.fromarray(rgb).save(dsts[i]); lap()
        for k, (t0, t1) in zip(stages, zip(t, t[1:])):
            stages[k].append((t1 - t0) * 1e3)
    total = sum(statistics.median(v) for v in stages.values())
    say(f"# 1. per-image path, ms per image (median of {a.images}; min - max), share of the sum of medians {total:.1f} ms")
    for k, v in stages.items():
        say(f"{k:>12}: {statistics.median(v):8.2f}  ({min(v):.2f} - {max(v):.2f})  {100 * statistics.median(v) / total:5.1f} %")

    # ---- 2. images/s, the configurations alternated
    cfgs = [(None, None)] + [(b, w) for b in BATCHES[1:] for w in WORKERS]
    rates = {c: [] for c in cfgs}

    def run(c, idx):
        if c[0] is None:
            return per_image(idx)
        U.copy_or_convert_images([paths[i] for i in idx], [dsts[i] for i in idx], pipe, wrapped, batch_images=c[0], io_workers=c[1])

    refused = {}
    for r in range(a.rounds):
        for c in cfgs:
            if c in refused:
                continue
            try:
                run(c, range(max(2, c[0] or 0)))   # two warm-up images (a full batch where that is more: the refusal of a batch size shows here)
            except ValueError as e:
                refused[c] = str(e)
                continue
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(c, range(a.images))
            torch.cuda.synchronize()
            rates[c].append(a.images / (time.perf_counter() - t0))
            print(f"[round {r}] batch_images={c[0]} io_workers={c[1]}: {rates[c][-1]:.3f} images/s", file=sys.stderr, flush=True)
    base_rate = statistics.median(rates[(None, None)])
    say(f"# 2. images/s over {a.images} images (median of {a.rounds} rounds; min - max), ratio of medians to batch_images=None")
    say("# batch_images io_workers | images/s")
    for c in cfgs:
        v = rates[c]
        if c in refused:
            say(f"{str(c[0]):>14} {str(c[1]):>10} | refused by the library: {refused[c]}")
            continue
        say(f"{str(c[0]):>14} {str(c[1]):>10} | {statistics.median(v):7.3f}  ({min(v):.3f} - {max(v):.3f})  x{statistics.median(v) / base_rate:.3f}")

    # ---- 3. the front end alone, B = 8
    host = [np.asarray(Image.open(p).convert("RGB"), np.uint8) for p in paths[:8]]
    stack = np.stack(host)

    def device_front(with_copy):
        x = torch.from_numpy(stack).to(dev) if with_copy else device_front.x
        return imgio.resize_normalize(x, (1024, 1024), U.IMAGENET_MEAN, U.IMAGENET_STD)
    device_front.x = torch.from_numpy(stack).to(dev)

    def host_front():
        xs = [torch.from_numpy(np.asarray(Image.fromarray(h).resize((1024, 1024), Image.BILINEAR), np.float32) / 255.0).permute(2, 0, 1)[None].to(dev) for h in host]
        return [(x - mean) / std for x in xs]

    def wall(fn, reps=10):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), min(ts), max(ts)
    same = torch.equal(device_front(True), torch.cat(host_front()))
    say(f"# 3. Resize + ToTensor + Normalize of eight 1000 x 1000 images -> [8, 3, 1024, 1024] float32 on the device, ms (median of 10; min - max); results equal: {same}")
    for name, fn in (("resize_normalize, uint8 already on the device", lambda: device_front(False)), ("H2D of the uint8 stack + resize_normalize", lambda: device_front(True)),
                     ("host: Image.resize + numpy / 255 + H2D + normalise, per image", host_front)):
        m, lo, hi = wall(fn)
        say(f"{name:>62}: {m:8.2f}  ({lo:.2f} - {hi:.2f})")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    shutil.rmtree(a.workdir, ignore_errors=True)


if __name__ == "__main__":
    main()
