#!/usr/bin/env python3
"""Per-step time of the reverse loop with a guide network attached (autoguidance) next to the plain loop on the same
build.  Reports only, gates nothing; writes profiles/autoguide_bench.md with --out.

Workload: the Visual Genome bits shape (N = 64, 30 valid nodes, 6 adjacency + 12 node channels), B = 64, T = 8 Euler steps,
S_churn = 0, fp32, step graphs on, the initial sample from the library's Philox stream, no coin fired (one network forward per
preconditioned call and per network).  Configurations, all in one process:
  plain          no guide attached
  same           a guide of the main network's size (other weights), every level
  same_half      ... with a sigma_range that covers schedule indices 2 .. 5 (half the levels)
  p2             a patch_size = 2 guide of the same depths (0.27 of the forward's FLOPs, profiles/patch_bench.md), every level
  p2_half        ... with the same sigma_range
Method: every configuration is warmed up (its step bodies captured), then the configurations are timed alternately, A B C D E A B ...,
--reps times each; a timing is a pair of HIP events around one whole sample() call on the current stream, divided by T.  Printed per
configuration: median, min and max of the per-step time, the ratio of its median to plain's, and the forwards of both networks.
--plain-only: the plain configuration alone (no autoguidance entry is touched: the same command times an older build of the library).

Usage:  python tools/autoguide_bench.py [--batch 64] [--steps 8] [--reps 15] [--valid 30] [--plain-only] [--out profiles/autoguide_bench.md]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffusesg_amd import lib as L, synth as Y, weights as W       # noqa: E402
from diffusesg_amd.model import build_network                      # noqa: E402
from diffusesg_amd.sampler import NodeAdjEDMSamplerHip             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--valid", type=int, default=30)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--out", default=None, help="write the markdown report here")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "autoguide_bench needs the GPU"
    B, T = args.batch, args.steps
    cfg = Y.CONFIGS["vg"]()
    n = cfg.max_node_num
    main_net = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")
    flags = torch.from_numpy(W.synth_flags(B, n, args.valid)).cuda()
    smp = NodeAdjEDMSamplerHip(num_steps=T, solver="euler", S_churn=0.0, self_condition=True, dev="cuda", use_graph=True)
    kw = dict(coins=np.zeros(T, np.uint8), seed=5, num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj, return_device=True)
    t_hat = L.sigma_schedule(smp._cfg())[1]
    half = (float(t_hat[min(5, T - 1)]), float(t_hat[min(2, T - 1)]))
    configs = {"plain": None}
    if not args.plain_only:
        same = build_network(cfg, W.synth_state_dict(cfg, 1), device="cuda")
        p2cfg = Y.PATCH_CONFIGS["vg_p2"]()
        p2 = build_network(p2cfg, W.synth_state_dict(p2cfg, 1), device="cuda")
        configs.update({"same": (same, None), "same_half": (same, half), "p2": (p2, None), "p2_half": (p2, half)})

    def call(name):
        if not args.plain_only:
            if configs[name] is None:
                main_net.detach_guide()
            else:
                main_net.attach_guide(configs[name][0], scale=2.0, sigma_range=configs[name][1])
        return smp.sample(main_net, flags, **kw)

    fwd = {}
    for name in configs:   # warm-up: captures the step bodies (attaching drops the guided ones, so every timed call replays or re-captures alike)
        for _ in range(2):
            call(name)
        torch.cuda.synchronize()
        fwd[name] = (smp.last_stats["net_forwards"], getattr(smp, "last_guide_forwards", 0))
    times = {name: [] for name in configs}
    for _ in range(args.reps):
        for name in configs:
            if not args.plain_only:   # attach outside the timed window, and capture the configuration's bodies again
                call(name)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            smp.sample(main_net, flags, **kw)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / T)
    res = {"gpu": torch.cuda.get_device_name(0), "config": f"vg N={n} valid={args.valid} B={B} T={T} euler S_churn=0 fp32 no coin", "reps": args.reps}
    lines = ["| configuration | ms per step (median) | min | max | / plain | main forwards | guide forwards |", "|---|---|---|---|---|---|---|"]
    base = float(np.median(times["plain"]))
    for name, ts in times.items():
        med = float(np.median(ts))
        res[name] = {"median_ms_per_step": med, "min": float(min(ts)), "max": float(max(ts)), "ratio": med / base, "net_forwards": fwd[name][0],
                     "guide_forwards": fwd[name][1]}
        lines.append(f"| {name} | {med:.4f} | {min(ts):.4f} | {max(ts):.4f} | {med / base:.3f} | {fwd[name][0]} | {fwd[name][1]} |")
    print("\n".join(lines))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("# Autoguidance: per-step time with a guide network attached\n\n"
                    f"`tools/autoguide_bench.py` on {res['gpu']}: {res['config']}, {args.reps} alternated repetitions per configuration,\n"
                    "HIP events around one whole `sample()` call, divided by the number of steps.  `same`: a guide of the main network's\n"
                    "size; `p2`: a `patch_size = 2` guide; `_half`: a `sigma_range` covering schedule indices 2 .. 5 of 8.\n\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
