#!/usr/bin/env python3
"""Per-executed-step time of a resampled conditioned run (NodeAdjEDMSamplerHip.sample_known with resample=(10, 3) over the whole
schedule) next to the plain conditioned loop on the same build.  Reports only, gates nothing.

Workload: tools/complete_bench.py's -- the Visual Genome shape (N = 64, 30 valid nodes, 6 adjacency + 12 node channels), B = 64,
T = 20 Heun + churn steps, fp32, step graphs on; init and churn noise from the library's Philox streams, a random half of the elements
known (+-1 values).  The resampled walk executes L = 3 T = 60 steps (each block of ten schedule indices three times).  The plain
loop runs complete_bench's coin sequence, and the walk's coins repeat it per visit -- a preconditioned call at schedule index i gets
the coin the plain loop uses there -- so the walk runs exactly n_resample times the plain loop's network forwards and a step of one
loop costs what the same step of the other does.  A walk changes the rows of the loop's step table, not
the step: the launch sequence per executed step is the plain loop's, so the expectation is "equal within the plain loop's own
run-to-run spread".  Things that would show up here: an extra captured body replayed per step, the schedule-index indirection of
the (scale, shift) row, per-call staging that grows with L.

Method: both loops are warmed up (their step bodies captured), then timed alternately, A B A B ..., --reps times each; a timing
is a host clock around one whole call ending in a device synchronise, divided by the number of EXECUTED steps (T resp. L; the time
per network forward is printed as well).  Printed per loop: median, min and max over the repetitions (the spread), and the ratio of the medians.

Usage:  python tools/resample_bench.py [--batch 64] [--steps 20] [--reps 15] [--valid 30] [--jump 10] [--resample 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffusesg_amd import lib, synth as Y, weights as W           # noqa: E402
from diffusesg_amd.model import build_network                      # noqa: E402
from diffusesg_amd.sampler import NodeAdjEDMSamplerHip             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--valid", type=int, default=30)
    ap.add_argument("--jump", type=int, default=10)
    ap.add_argument("--resample", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "resample_bench needs the GPU"
    B, T = args.batch, args.steps
    cfg = Y.CONFIGS["vg"]()
    n = cfg.max_node_num
    net = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")
    smp = NodeAdjEDMSamplerHip(num_steps=T, solver="heun", S_churn=40.0, self_condition=True, dev="cuda", use_graph=True)
    resample = (args.jump, args.resample)
    sched, _ = lib.walk_steps(smp._cfg(), lib.make_walk_cfg(0, resample, None))
    L = len(sched)
    flags = torch.from_numpy(W.synth_flags(B, n, args.valid)).cuda()
    plain_coins = (W.coins(31, "cbench", 2 * T - 1) < 0.5).astype(np.uint8)
    walk_coins = np.concatenate([plain_coins[2 * i:2 * i + (1 if i == T - 1 else 2)] for i in sched.tolist()])
    known_adj, known_node = (torch.from_numpy(t).cuda() for t in Y.gt_case(cfg, B, args.valid))
    sa, sn = (B, cfg.c_adj, n, n), (B, n, cfg.c_node)
    mask_adj = torch.from_numpy((W.uniform01(31, "cbench/mask_adj", int(np.prod(sa))) < 0.5).reshape(sa)).cuda()
    mask_node = torch.from_numpy((W.uniform01(31, "cbench/mask_node", int(np.prod(sn))) < 0.5).reshape(sn)).cuda()
    kw = dict(seed=5, num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj, return_device=True)
    known = (known_adj, known_node, mask_adj, mask_node)
    loops = {"plain": (T, lambda: smp.sample_known(net, flags, *known, coins=plain_coins, **kw)),
             "resampled": (L, lambda: smp.sample_known(net, flags, *known, coins=walk_coins, resample=resample, **kw))}
    stats = {}
    for name, (_, fn) in loops.items():   # warm-up: captures the step bodies
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        stats[name] = dict(smp.last_stats)
    times = {name: [] for name in loops}
    for _ in range(args.reps):
        for name, (steps, fn) in loops.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    res = {"gpu": torch.cuda.get_device_name(0), "config": f"vg N={n} valid={args.valid} B={B} T={T} heun fp32", "reps": args.reps,
           "known_share": 0.5, "resample": list(resample), "executed_steps": {"plain": T, "resampled": L},
           "net_forwards": {k: v["net_forwards"] for k, v in stats.items()}}
    for name, (steps, _) in loops.items():
        ts = np.array(times[name])
        for what, div in (("ms_per_step", steps), ("ms_per_forward", stats[name]["net_forwards"])):
            res[f"{name}_{what}"] = {"median": float(np.median(ts) / div), "min": float(ts.min() / div), "max": float(ts.max() / div)}
    for what in ("ms_per_step", "ms_per_forward"):
        res[f"ratio_of_medians_{what}"] = res[f"resampled_{what}"]["median"] / res[f"plain_{what}"]["median"]
    p = res["plain_ms_per_step"]
    res["plain_spread"] = (p["max"] - p["min"]) / p["median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
