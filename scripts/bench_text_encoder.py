"""The CLIP text encoder on the HIP library (ldiff_textenc, models.CLIPTextModel) against what a user had before it existed: `transformers`'
CLIPTextModel run by torch on the same GPU, in fp32 (what the reference runs) and as .half().  CLIP-L size (49,408 x 768 embeddings, 12 layers,
12 heads, intermediate 3,072) with seeded synthetic weights; last_hidden_state at (B, L) = (1, 5), (1, 77), (8, 77), ids on the host on both sides.

Per shape the four sides -- library eager, library replayed (hipGraph), torch fp32, torch fp16 -- alternate inside one process after a warm-up,
--reps rounds of --inner forwards each (device-synchronised wall time per forward; median, min, max over the rounds).  The launches per pass are the
kernel nodes of the captured graph.  Each side's error against the fp32 `transformers` result on the CPU is printed beside its time, and per shape one
eager pass of the library is broken down by launch name (ldiff_prof_*: HIP events around every launch).

usage: python scripts/bench_text_encoder.py [--reps 20] [--inner 20] [--layers 12] [--out profiles/text_encoder_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ldiffusion_amd import _lib  # noqa: E402
from ldiffusion_amd.models import CLIPTextModel as HipCLIPTextModel  # noqa: E402

SHAPES = ((1, 5), (1, 77), (8, 77))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_text_encoder needs a GPU: a CPU run gives no time")
    from transformers import CLIPTextConfig, CLIPTextModel
    dev = "cuda:0"
    torch.manual_seed(0)
    cfg = CLIPTextConfig(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=args.layers, num_attention_heads=12, max_position_embeddings=77)
    ref = CLIPTextModel(cfg).eval()
    hip_eager = HipCLIPTextModel(cfg.to_dict(), ref.state_dict(), dev).set_graph(False)
    hip_graph = HipCLIPTextModel(cfg.to_dict(), ref.state_dict(), dev).set_graph(True)
    t32 = CLIPTextModel(cfg).eval()
    t32.load_state_dict(ref.state_dict())
    t32 = t32.to(dev)
    t16 = CLIPTextModel(cfg).eval()
    t16.load_state_dict(ref.state_dict())
    t16 = t16.to(dev).half()
    lines = [f"text encoder, CLIP-L size, {args.layers} layers; {args.reps} rounds x {args.inner} forwards per side and shape, sides alternating; ms per forward: median (min .. max)",
             f"device: {torch.cuda.get_device_name(0)}; error = max |x - ref| / max |ref| against fp32 transformers on the CPU"]
    sides = {"hip eager": lambda ids: hip_eager(ids)["last_hidden_state"], "hip replayed": lambda ids: hip_graph(ids)["last_hidden_state"],
             "torch fp32": lambda ids: t32(ids.to(dev))["last_hidden_state"], "torch fp16": lambda ids: t16(ids.to(dev))["last_hidden_state"]}
    with torch.no_grad():
        for B, L in SHAPES:
            ids = torch.randint(0, 49408, (B, L), generator=torch.Generator().manual_seed(B * 100 + L))
            want = ref(ids)["last_hidden_state"]
            err = {}
            for name, fn in sides.items():
                for _ in range(5):
                    out = fn(ids)
                torch.cuda.synchronize()
                err[name] = ((out.float().cpu() - want).abs().max() / want.abs().max()).item()
            times = {name: [] for name in sides}
            for _ in range(args.reps):
                for name, fn in sides.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.inner):
                        fn(ids)
                    torch.cuda.synchronize()
                    times[name].append((time.perf_counter() - t0) * 1e3 / args.inner)
            lines.append(f"(B, L) = ({B}, {L}): {hip_graph.graph_nodes} launches per pass in the captured graph, {hip_graph.graph_replays} replays so far")
            for name in sides:
                t = times[name]
                lines.append(f"    {name:13s} {statistics.median(t):8.3f} ms ({min(t):.3f} .. {max(t):.3f})    error {err[name]:.2e}")
            # where the time goes: one eager pass with every launch between two HIP events (the sum leaves out the gaps between launches)
            lib = _lib.load()
            _lib.prof_collect()
            lib.ldiff_prof_enable(1)
            try:
                hip_eager(ids)
                torch.cuda.synchronize()
            finally:
                lib.ldiff_prof_enable(0)
            rows = sorted(_lib.prof_collect(), key=lambda r: -r["ms"])
            lines.append(f"    one eager pass by launch name, HIP-event time: {sum(r['launches'] for r in rows)} launches, {sum(r['ms'] for r in rows):.3f} ms in all")
            for r in rows:
                lines.append(f"        {r['name']:28s} {r['launches']:4d} x {r['ms'] * 1e3 / r['launches']:7.1f} us = {r['ms']:.3f} ms   {r['bytes'] / max(r['ms'], 1e-9) * 1e-6:8.1f} GB/s")
    hip_eager.check_finite()
    hip_graph.check_finite()
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
