#!/usr/bin/env python3
"""Per-step time of the conditioned reverse loop (NodeAdjEDMSamplerHip.sample_known) next to the unconditioned one (sample) on the
same build.  Reports only, gates nothing.

Workload: the Visual Genome shape (N = 64, 30 valid nodes, 6 adjacency + 12 node channels), B = 64, T = 20 Heun + churn steps,
fp32, step graphs on; init and churn noise from the library's Philox streams, one fixed coin sequence for both loops (so both run
the same number of network forwards).  Conditioned: a random half of the elements known (+-1 values).  The select sits in the
kernel that writes the preconditioned output, so the conditioned loop launches exactly what the unconditioned one does; the
expectation is "equal within run-to-run spread".

Method: both loops are warmed up (their step bodies captured), then timed alternately, A B A B ..., --reps times each; a timing
is a host clock around one whole call ending in a device synchronise, divided by T.  Printed per loop: median, min and max of the
per-step time over the repetitions (the spread), and the ratio of the medians.

Usage:  python tools/complete_bench.py [--batch 64] [--steps 20] [--reps 15] [--valid 30]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffusesg_amd import synth as Y, weights as W                 # noqa: E402
from diffusesg_amd.model import build_network                      # noqa: E402
from diffusesg_amd.sampler import NodeAdjEDMSamplerHip             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--valid", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "complete_bench needs the GPU"
    B, T = args.batch, args.steps
    cfg = Y.CONFIGS["vg"]()
    n = cfg.max_node_num
    net = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")
    smp = NodeAdjEDMSamplerHip(num_steps=T, solver="heun", S_churn=40.0, self_condition=True, dev="cuda", use_graph=True)
    flags_np = W.synth_flags(B, n, args.valid)
    flags = torch.from_numpy(flags_np).cuda()
    coins = (W.coins(31, "cbench", 2 * T - 1) < 0.5).astype(np.uint8)
    known_adj, known_node = (torch.from_numpy(t).cuda() for t in Y.gt_case(cfg, B, args.valid))
    sa, sn = (B, cfg.c_adj, n, n), (B, n, cfg.c_node)
    mask_adj = torch.from_numpy((W.uniform01(31, "cbench/mask_adj", int(np.prod(sa))) < 0.5).reshape(sa)).cuda()
    mask_node = torch.from_numpy((W.uniform01(31, "cbench/mask_node", int(np.prod(sn))) < 0.5).reshape(sn)).cuda()
    kw = dict(coins=coins, seed=5, num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj, return_device=True)
    loops = {"sample": lambda: smp.sample(net, flags, **kw),
             "sample_known": lambda: smp.sample_known(net, flags, known_adj, known_node, mask_adj, mask_node, **kw)}
    stats = {}
    for name, fn in loops.items():   # warm-up: captures the step bodies
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        stats[name] = dict(smp.last_stats)
    times = {name: [] for name in loops}
    for _ in range(args.reps):
        for name, fn in loops.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / T * 1e3)
    res = {"gpu": torch.cuda.get_device_name(0), "config": f"vg N={n} valid={args.valid} B={B} T={T} heun fp32", "reps": args.reps,
           "known_share": 0.5, "net_forwards": {k: v["net_forwards"] for k, v in stats.items()}}
    for name, ts in times.items():
        res[name + "_ms_per_step"] = {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}
    res["ratio_of_medians"] = res["sample_known_ms_per_step"]["median"] / res["sample_ms_per_step"]["median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
