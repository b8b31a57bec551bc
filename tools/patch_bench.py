"""Step time of the sampler at patch_size 1 and 2 -- for the record in profiles/patch_bench.md and DESIGN.md §15.
One process measures ONE variant at the Visual Genome shape (N = 64, valid 30, B = 64, fp32): PB_STEPS Euler steps per sample() call,
S_churn = 0, a fixed coin pattern (every other step runs the self-conditioning forward: 1.5 network forwards per step on average), HIP
events around the whole synchronised call after PB_WARMUP calls, PB_ITERS timed calls; one JSON line with the per-step times.
Variants are alternated by the caller, process by process, in one job (other people's work shares the host, so two variants are only
compared inside one job and against the run-to-run spread of a repeated variant):
    python tools/patch_bench.py p1                  this tree, patch_size 1
    python tools/patch_bench.py p2                  this tree, patch_size 2, the fused E = 96 PatchEmbed and read-out (the default)
    python tools/patch_bench.py p2c                 this tree, patch_size 2, "fused_patch_embed" / "fused_readout" 0: the chain of kernels
    python tools/patch_bench.py p1 --root DIR       another checkout's package and library (e.g. the parent commit, built there)
PB_BATCH=64  PB_STEPS=40  PB_ITERS=5  PB_WARMUP=2  PB_VALID=30 (valid nodes per graph; 64: nothing is padded, so the masked-token
pruning and the pure-window deduplication of patch_size 1 have nothing to skip)"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("variant", choices=["p1", "p2", "p2c"])
ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
from diffusesg_amd import spec as S, synth as Y, weights as W      # noqa: E402
from diffusesg_amd.model import build_network                      # noqa: E402
from diffusesg_amd.sampler import NodeAdjEDMSamplerHip             # noqa: E402

B, STEPS = int(os.environ.get("PB_BATCH", "64")), int(os.environ.get("PB_STEPS", "40"))
ITERS, WARMUP = int(os.environ.get("PB_ITERS", "5")), int(os.environ.get("PB_WARMUP", "2"))
VALID = int(os.environ.get("PB_VALID", "30"))

assert torch.cuda.is_available(), "patch_bench needs the GPU: there is nothing to time without it"
cfg = Y.CONFIGS["vg"]() if args.variant == "p1" else Y.PATCH_CONFIGS["vg_p2"]()
n = cfg.max_node_num
flags = torch.from_numpy(W.synth_flags(B, n, [VALID] * B)).cuda()
net = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")
if args.variant == "p2c":
    net.model._ensure_handle().set_option("fused_patch_embed", 0)
    net.model._ensure_handle().set_option("fused_readout", 0)
smp = NodeAdjEDMSamplerHip(num_steps=STEPS, solver="euler", S_churn=0, self_condition=True)
coins = (np.arange(STEPS) % 2).astype(np.uint8)
run = lambda: smp.sample(net, flags, num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj, seed=1, coins=coins, return_device=True)
for _ in range(WARMUP):
    out = run()
torch.cuda.synchronize()
ms = []
for _ in range(ITERS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = run()
    e1.record()
    e1.synchronize()
    ms.append(e0.elapsed_time(e1) / STEPS)
h = net.model._ensure_handle()
forms = h.patch_forms(B) if hasattr(h, "patch_forms") else None
print(json.dumps({"variant": args.variant, "root": os.path.relpath(os.path.abspath(args.root)), "patch_size": getattr(cfg, "patch_size", 1),
                  "batch": B, "valid": VALID, "steps": STEPS, "net_forwards": int(smp.last_stats["net_forwards"]), "ms_per_step": [round(m, 4) for m in ms],
                  "median_ms_per_step": round(float(np.median(ms)), 4), "min_ms_per_step": round(float(np.min(ms)), 4),
                  "gflop_per_forward": S.flops_per_forward(cfg) / 1e9, "forms": forms,
                  "finite": bool(torch.isfinite(out[0]).all() and torch.isfinite(out[1]).all())}))
