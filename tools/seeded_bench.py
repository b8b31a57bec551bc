#!/usr/bin/env python3
"""Per-step time of the seeded loop (graph_seeds=, per-graph noise streams) next to the unseeded one on the same build, and what the
option "batch_invariant" costs.  Reports only, gates nothing.

Workload: the Visual Genome shape (N = 64, 30 valid nodes, 6 adjacency + 12 node channels), T = 20 Heun steps with churn
(S_churn = 40), fp32, step graphs on, initial sample and churn noise from the library's Philox streams, one fixed coin sequence for
every loop (so all run the same number of network forwards).

  1. seeded against unseeded, B = 64, batch_invariant = 0: both loops replay the same captured step bodies; the seeded churn kernel
     reads one 8-byte key per thread and subtracts the graph's offset from the element index.  Expectation: equal within the
     unseeded loop's own run-to-run spread, which is printed (max - min over the repetitions, relative to the median).
  2. batch_invariant 0 against 1, seeded, at B = 64 -- 64 * 1024 merged rows: the fused PatchMerging runs either way, the same kernels --
     and at B = 4, where the option forces the fused merge below the 8192 merged rows from which it pays.  Recorded, not bounded.

Method: every loop is warmed up (its step bodies captured), then the two loops of a comparison are timed alternately, A B A B ...,
--reps times each; a timing is a host clock around one whole call ending in a device synchronise, divided by T.  Setting the option
drops the captured bodies, so comparison 2 keeps one network per option value instead of toggling one.

Usage:  python tools/seeded_bench.py [--batch 64] [--small-batch 4] [--steps 20] [--reps 15] [--valid 30]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffusesg_amd import dist as ddist, synth as Y, weights as W  # noqa: E402
from diffusesg_amd.model import build_network                      # noqa: E402
from diffusesg_amd.sampler import NodeAdjEDMSamplerHip             # noqa: E402


def alternate(loops, T, reps):
    """{name: per-step times in ms}: warm up every loop, then time them in turn, reps times each"""
    for fn in loops.values():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
    times = {name: [] for name in loops}
    for _ in range(reps):
        for name, fn in loops.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / T * 1e3)
    return times


def report(title, times, base):
    print(title)
    out = {}
    for name, ts in times.items():
        med = float(np.median(ts))
        out[name] = {"median_ms_per_step": med, "min": float(min(ts)), "max": float(max(ts)), "spread_pct": (max(ts) - min(ts)) / med * 100}
        print(f"  {name:28s} {med:8.4f} ms per step (min {min(ts):.4f}, max {max(ts):.4f}, spread {out[name]['spread_pct']:.2f} %)")
    other = [k for k in times if k != base][0]
    out["ratio_of_medians"] = out[other]["median_ms_per_step"] / out[base]["median_ms_per_step"]
    print(f"  ratio of medians {other} / {base}: {out['ratio_of_medians']:.4f}  "
          f"({(out['ratio_of_medians'] - 1) * 100:+.2f} %; spread of {base}: {out[base]['spread_pct']:.2f} %)")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--small-batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--valid", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "seeded_bench needs the GPU"
    T = args.steps
    cfg = Y.CONFIGS["vg"]()
    n = cfg.max_node_num
    sd = W.synth_state_dict(cfg, 0)
    nets = {0: build_network(cfg, sd, device="cuda"), 1: build_network(cfg, sd, device="cuda")}
    nets[1].model._ensure_handle().set_option("batch_invariant", 1)
    coins = (W.coins(31, "seeded_bench", 2 * T - 1) < 0.5).astype(np.uint8)
    kw = dict(coins=coins, num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj, return_device=True)
    smp = NodeAdjEDMSamplerHip(num_steps=T, solver="heun", S_churn=40.0, self_condition=True, dev="cuda", use_graph=True)

    def loop(net, B, seeded):
        flags = torch.from_numpy(W.synth_flags(B, n, args.valid)).cuda()
        seeds = ddist.graph_seeds(5, 0, B)
        if seeded:
            return lambda: smp.sample(net, flags, graph_seeds=seeds, **kw)
        return lambda: smp.sample(net, flags, seed=5, **kw)

    B, Bs = args.batch, args.small_batch
    res = {"gpu": torch.cuda.get_device_name(0), "config": f"vg N={n} valid={args.valid} T={T} heun S_churn=40 fp32 step graphs", "reps": args.reps}
    res["seeded_vs_unseeded"] = report(f"1. seeded against unseeded, B = {B}, batch_invariant = 0",
                                       alternate({"unseeded": loop(nets[0], B, False), "seeded": loop(nets[0], B, True)}, T, args.reps), "unseeded")
    res["stats"] = dict(smp.last_stats)
    for b in (B, Bs):
        res[f"batch_invariant_B{b}"] = report(f"2. batch_invariant 0 against 1, seeded, B = {b}",
                                              alternate({"batch_invariant=0": loop(nets[0], b, True), "batch_invariant=1": loop(nets[1], b, True)},
                                                        T, args.reps), "batch_invariant=0")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
