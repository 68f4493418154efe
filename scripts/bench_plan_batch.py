"""What the plan batch (ldiff_*_set_plan_batch, DESIGN.md "Batch invariance") costs: one UNet pass (hipGraph replay) and one VAE decode at SD-v1.5
size, B in {1, 2, 3, 8}, with n in {0 (default plans), 8 (the bench batch's plans), 1 (planned from one image)}.  One process per configuration
(fresh handles, fresh graphs), all on the same box; device events around warmed-up repetitions; a configuration with B > n > 0 is refused by the
library and not run.
usage: python scripts/bench_plan_batch.py [--reps 20] [--out profiles/plan_batch_cost.txt]      (the table; starts the children)
       python scripts/bench_plan_batch.py --one N [--reps 20]                                   (one JSON line per B for plan batch N)"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCHES = (1, 2, 3, 8)
PLANS = (0, 8, 1)


def one(n, reps):
    import torch

    from ldiffusion_amd import configs, weights
    from ldiffusion_amd.models import AutoencoderKL, UNet2DConditionModel
    dev = "cuda:0"
    ucfg, vcfg = configs.SD15_UNET, configs.SD15_VAE
    unet = UNet2DConditionModel(ucfg, weights.synthetic_state_dict(weights.unet_param_shapes(ucfg), 42, fp16_values=True), dev).set_plan_batch(n)
    vae = AutoencoderKL(vcfg, weights.synthetic_state_dict(weights.vae_param_shapes(vcfg), 43, fp16_values=True), dev).set_plan_batch(n)
    g = torch.Generator().manual_seed(7)
    ctx = (torch.randn((1, 77, 768), generator=g) * 0.5).to(dev)

    def timed(fn):
        for _ in range(3):   # UNet: eager, capture, first replay
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    for B in BATCHES:
        if 0 < n < B:
            continue
        x = torch.randn((B, 4, 64, 64), generator=g).to(dev)
        z = (torch.randn((B, 4, 64, 64), generator=g) * 0.2).to(dev)
        unet_ms = timed(lambda: unet(x, 501, ctx))
        nodes = unet.graph_nodes
        dec_ms = timed(lambda: vae._decode(z, 1.0, want_rgb=True))
        print(json.dumps({"plan_batch": n, "B": B, "unet_ms": round(unet_ms, 3), "unet_graph_nodes": nodes, "vae_decode_ms": round(dec_ms, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", type=int, default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.one is not None:
        return one(a.one, a.reps)
    rows = []
    for n in PLANS:   # a fresh child process per plan batch: nothing of one configuration is warm for the next
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(n), "--reps", str(a.reps)], check=True, capture_output=True, text=True)
        rows += [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    by = {(r["plan_batch"], r["B"]): r for r in rows}
    lines = [f"# scripts/bench_plan_batch.py --reps {a.reps}: SD-v1.5 size, 64 x 64 latents, L = 77; ms per call (mean of {a.reps} after warm-up), n = plan batch",
             "# B | UNet pass, graph replay: n=0  n=8  n=1 | graph nodes: n=0  n=8  n=1 | VAE decode 512 x 512: n=0  n=8  n=1"]
    for B in BATCHES:
        def col(key):
            return "  ".join(f"{by[(n, B)][key]:>8}" if (n, B) in by else "       -" for n in PLANS)
        lines.append(f"{B:>3} | {col('unet_ms')} | {col('unet_graph_nodes')} | {col('vae_decode_ms')}")
    text = "\n".join(lines + [json.dumps(r) for r in rows]) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
