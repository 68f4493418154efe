"""Where the warm-up's data comes from, measured: the reference-style host loader against the device-resident one (ldiffusion_amd/dataset.py), over synthetic
1024 x 1024 PNGs and label PNGs the script makes itself, batch 8.
  1. batches/s of the loader alone, each batch brought to the device: the host DataLoader in one process and with four workers (the reference's setting),
     `DeviceLoader.__iter__` and `DeviceLoader.warmup_batches(64)` after the store is built; the feeds alternated in one process, one warm-up epoch each;
  2. the store's build time over io_workers;
  3. a warm-up epoch at SD-v1.5 width (synthetic weights) fed each way: per batch the 64 x 64 image and label, the VAE encoder and one captured training step
     (train.GraphedStep, as scripts/bench_train.py --graph runs it; the sample triples are fixed -- drawing them is host work every feed pays alike).  --no-step skips it.
Everything it reads it has written itself, under --workdir (default build/warmup_data_bench in the repository).
usage: python scripts/bench_warmup_data.py [--images 32] [--rounds 3] [--no-step] [--out profiles/warmup_data_bench.txt]"""
import argparse
import os
import shutil
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, SIDE = 8, 1024


def make_folders(np, Image, root, n):
    """Smooth colour fields with mild noise (PNG decode costs nearer a stained slide's than white noise's) and blocky label maps of the tissue grey levels."""
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:SIDE, 0:SIDE].astype(np.float32) / SIDE
    greys = np.array([0, 50, 100, 150, 200, 250, 255], np.uint8)
    img_dir, lab_dir = os.path.join(root, "images"), os.path.join(root, "labels")
    os.makedirs(img_dir), os.makedirs(lab_dir)
    for i in range(n):
        f = rng.uniform(2, 9, (3, 2))
        field = np.stack([0.5 + 0.35 * np.sin(2 * np.pi * (f[c, 0] * yy + f[c, 1] * xx) + i) for c in range(3)], -1)
        Image.fromarray(np.clip(field * 255 + rng.normal(0, 6, (SIDE, SIDE, 3)), 0, 255).astype(np.uint8)).save(os.path.join(img_dir, f"case_{i:03d}.png"))
        blocks = greys[rng.integers(0, len(greys), (SIDE // 64, SIDE // 64))]
        Image.fromarray(np.kron(blocks, np.ones((64, 64), np.uint8))).save(os.path.join(lab_dir, f"case_{i:03d}.png"))
    return img_dir, lab_dir


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--workdir", default=os.path.join(ROOT, "build", "warmup_data_bench"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    from PIL import Image
    from torch.utils.data import DataLoader

    from ldiffusion_amd import dataset
    dev = "cuda:0"
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    shutil.rmtree(a.workdir, ignore_errors=True)
    img_dir, lab_dir = make_folders(np, Image, a.workdir, a.images)
    images = sorted(os.path.join(img_dir, f) for f in os.listdir(img_dir))
    labels = sorted(os.path.join(lab_dir, f) for f in os.listdir(lab_dir))
    ds = dataset.MedicalSegmentationDataset(images, labels, dataset.default_transform(SIDE), "tissue")
    lines = [f"# scripts/bench_warmup_data.py --images {a.images} --rounds {a.rounds}: {a.images} synthetic {SIDE} x {SIDE} PNGs + labels, batch {B}; {torch.cuda.get_device_name(0)}; "
             f"Pillow {Image.__version__}; {os.environ.get('OMP_NUM_THREADS', 'unset')} OMP threads"]

    def say(s=""):
        lines.append(s)
        print(s, flush=True)

    # ---- 2. the store's build time (first, so that section 1 has its loader)
    build = {}
    dloader = None
    for r in range(a.rounds):
        for w in (0, 1, 2, 4, 8):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dloader = dataset.DeviceLoader(ds, batch_size=B, shuffle=True, drop_last=True, device=dev, io_workers=w)
            torch.cuda.synchronize()
            build.setdefault(w, []).append(time.perf_counter() - t0)
    store_mb = (dloader.images.numel() + dloader.labels.numel()) / 2 ** 20

    def reduce_host(batch):      # what the warm-up loop does with a loader's batch (ldiffusion.py:200,212,225)
        image, _, label = batch
        image = F.interpolate(image.to(dev, dtype=torch.float32), size=(64, 64), mode="bilinear", align_corners=False, antialias=True)
        return image, F.interpolate(label.to(dev, torch.float32), size=(64, 64), mode="bilinear", align_corners=False).to(torch.uint8)

    host1 = DataLoader(ds, batch_size=B, shuffle=True, drop_last=True, num_workers=0)
    host4 = DataLoader(ds, batch_size=B, shuffle=True, drop_last=True, num_workers=4)
    feeds = {"host DataLoader, 1 process": lambda: (reduce_host(b) for b in host1),
             "host DataLoader, 4 workers": lambda: (reduce_host(b) for b in host4),
             "DeviceLoader.__iter__": lambda: (reduce_host(b) for b in dloader),
             "DeviceLoader.warmup_batches": lambda: dloader.warmup_batches(64)}
    raw = {"host DataLoader, 1 process": lambda: ([t.to(dev) for t in b] for b in host1), "host DataLoader, 4 workers": lambda: ([t.to(dev) for t in b] for b in host4),
           "DeviceLoader.__iter__": lambda: iter(dloader), "DeviceLoader.warmup_batches": lambda: dloader.warmup_batches(64)}

    def epoch(feed, step=None):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        for batch in feed():
            if step is not None:
                step(*batch)
            n += 1
        torch.cuda.synchronize()
        return n, time.perf_counter() - t0

    def table(title, feeds, step=None, unit="batches/s"):
        rates = {k: [] for k in feeds}
        for r in range(a.rounds + 1):        # round 0: warm-up
            for k, feed in feeds.items():
                n, dt = epoch(feed, step)
                if r:
                    rates[k].append((n / dt, dt))
        say(title)
        base = statistics.median(v[0] for v in rates[next(iter(feeds))])
        for k, v in rates.items():
            rs = [x[0] for x in v]
            say(f"{k:>30}: {statistics.median(rs):9.2f} {unit}  ({min(rs):.2f} - {max(rs):.2f})  x{statistics.median(rs) / base:.2f}   epoch {statistics.median(x[1] for x in v) * 1e3:9.1f} ms")

    table(f"# 1. the loader alone, every batch on the device, {a.images // B} batches of {B} per epoch (median of {a.rounds} epochs; min - max), ratio to the first row", raw)
    table("# 1b. the loader and the two 64 x 64 reductions of the warm-up loop (warmup_batches yields them)", feeds)
    say(f"# 2. DeviceLoader construction ({a.images} images + labels decoded, resized and stored: {store_mb:.0f} MiB), seconds (median of {a.rounds}; min - max)")
    for w, v in build.items():
        say(f"{'io_workers=' + str(w):>30}: {statistics.median(v):7.3f}  ({min(v):.3f} - {max(v):.3f})")

    if not a.no_step:
        from ldiffusion_amd import configs, train, weights
        from ldiffusion_amd.models import AutoencoderKL
        from ldiffusion_amd.scheduler import PNDMScheduler
        ucfg, vcfg = configs.SD15_UNET, configs.SD15_VAE
        usd = weights.synthetic_state_dict(weights.unet_param_shapes(ucfg), 42, fp16_values=True)
        vsd = weights.synthetic_state_dict(weights.vae_param_shapes(vcfg), 43, fp16_values=True)
        unet, dec, vae = train.TrainableUNet(ucfg, usd, dev), train.FrozenVAEDecoder(vcfg, vsd, dev), AutoencoderKL(vcfg, vsd, dev)
        del usd, vsd
        g = torch.Generator().manual_seed(0)
        hidden = (torch.randn((B, 6, 768), generator=g) * 0.5).to(dev)
        proj = ((torch.randn((768, 768), generator=g) / 768 ** 0.5).to(dev).requires_grad_(True), torch.zeros(768, device=dev, requires_grad=True))
        sch = PNDMScheduler()
        sch.set_timesteps(1, device=dev)
        ts = [int(t) for t in sch.timesteps]
        eps32 = torch.finfo(torch.float32).eps
        u_list = [(torch.rand((B, 4, 8, 8), generator=g) * (2 - eps32) + (eps32 - 1)).to(dev) for _ in ts]
        pairs = [[(int(torch.randint(0, 4096, (1,), generator=g)), int(torch.randint(0, 4096, (1,), generator=g)), torch.randint(0, 4096, (1024,), generator=g).tolist())
                  for _ in range(8)] for _ in range(B)]
        state = {}
        gstep = train.GraphedStep(unet, dec, proj, B, ts, sch.alphas_cumprod, latent_hw=8, text_len=6, text_dim=768, max_triples=256, num_negatives=1024)

        def step(image, lab):
            with torch.no_grad():
                z = vae.encode(image).latent_dist.mean.to(dtype=torch.float32)
            train.train_step_graphed(gstep, z, hidden, u_list, pairs, state, lr=1e-5)

        fixed = [(torch.randn((B, 3, 64, 64), generator=g).to(dev), None)] * (a.images // B)
        table(f"# 3. a warm-up epoch at SD-v1.5 width ({a.images // B} steps of batch {B}: 64 x 64 batch -> VAE encoder -> captured training step), steps/s; first row: batches already on the device",
              {"no loader (resident batches)": lambda: iter(fixed), **feeds}, step, unit="steps/s")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    del host4
    shutil.rmtree(a.workdir, ignore_errors=True)


if __name__ == "__main__":
    main()
