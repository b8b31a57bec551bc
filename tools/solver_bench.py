#!/usr/bin/env python3
"""Per-step time of the second-order multistep solver (solver='dpmpp_2m') next to solver='euler' on the same build, and the error of
both against a fine Euler run as the number of steps grows.  Reports only, gates nothing.

Timing workload: the Visual Genome shape (N = 64, 30 valid nodes, 6 adjacency + 12 node channels), B = 64, T = 20 steps, S_churn = 0,
fp32, step graphs on; the initial sample from the library's Philox stream, one fixed coin sequence for both solvers (so both run the
same number of network forwards).  Both solvers make one preconditioned call per step; a multistep step launches the same sequence
with its own update kernel, which reads one more state-sized tensor (the previous denoised estimate).  The expectation is "equal
within run-to-run spread".

Method: both loops are warmed up (their step bodies captured), then timed alternately, A B A B ..., --reps times each; a timing is a
host clock around one whole call ending in a device synchronise, divided by T.  Printed per solver: median, min and max of the per-step
time over the repetitions (the spread), and the ratio of the medians.

Error table: the tiny nets 'nosc' (no self-conditioning) and 'tiny' (self-conditioning, no coin fired), B = 4, valid nodes
[8, 5, 3, 8], inputs synth.sampler_case(cfg, 2, 4, valid, 3, "dpm/<name>", "euler"); max-abs error of each solver at T = 16 .. 128
against solver='euler' at T = 2048, relative to the reference's max |value|.  Synthetic weights: this says how fast the loop converges
to its own limit, nothing about sample quality with trained weights.

Usage:  python tools/solver_bench.py [--batch 64] [--steps 20] [--reps 15] [--valid 30] [--no-table]
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

SOLVERS = ("euler", "dpmpp_2m")


def sampler(T, solver, self_condition=True):
    return NodeAdjEDMSamplerHip(num_steps=T, solver=solver, S_churn=0.0, self_condition=self_condition, dev="cuda", use_graph=True)


def error_table(name, Ts=(16, 32, 64, 128), T_ref=2048):
    cfg = Y.CONFIGS[name]()
    net = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")
    flags, ia, inn, _, _, _ = Y.sampler_case(cfg, 2, 4, [8, 5, 3, 8], 3, f"dpm/{name}", "euler")
    flags, ia, inn = (torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in (flags, ia, inn))

    def run(solver, T):
        out = sampler(T, solver, cfg.self_condition).sample(net, flags, init_adjs=ia, init_nodes=inn, coins=np.zeros(T, np.uint8),
                                                            num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj)
        return [t.double() for t in out]

    ref = run("euler", T_ref)
    rows = {}
    for T in Ts:
        rows[T] = {s: [float((o - r).abs().max() / r.abs().max()) for o, r in zip(run(s, T), ref)] for s in SOLVERS}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--valid", type=int, default=30)
    ap.add_argument("--no-table", action="store_true", help="skip the error-vs-T table")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "solver_bench needs the GPU"
    B, T = args.batch, args.steps
    cfg = Y.CONFIGS["vg"]()
    n = cfg.max_node_num
    net = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")
    flags = torch.from_numpy(W.synth_flags(B, n, args.valid)).cuda()
    coins = (W.coins(31, "sbench", T) < 0.5).astype(np.uint8)
    kw = dict(coins=coins, seed=5, num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj, return_device=True)
    smps = {s: sampler(T, s) for s in SOLVERS}
    loops = {s: (lambda s=s: smps[s].sample(net, flags, **kw)) for s in SOLVERS}
    stats = {}
    for name, fn in loops.items():   # warm-up: captures the step bodies
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        stats[name] = dict(smps[name].last_stats)
    times = {name: [] for name in loops}
    for _ in range(args.reps):
        for name, fn in loops.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / T * 1e3)
    res = {"gpu": torch.cuda.get_device_name(0), "config": f"vg N={n} valid={args.valid} B={B} T={T} S_churn=0 fp32", "reps": args.reps,
           "net_forwards": {k: v["net_forwards"] for k, v in stats.items()}}
    for name, ts in times.items():
        res[name + "_ms_per_step"] = {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}
        print(f"{name:9s} {np.median(ts):8.4f} ms per step (min {min(ts):.4f}, max {max(ts):.4f}, spread {(max(ts) - min(ts)) / np.median(ts) * 100:.2f} %)")
    res["ratio_of_medians"] = res["dpmpp_2m_ms_per_step"]["median"] / res["euler_ms_per_step"]["median"]
    print(f"ratio of medians dpmpp_2m / euler {res['ratio_of_medians']:.4f}")
    if not args.no_table:
        res["error_vs_T"] = {}
        print("max-abs error against euler at T = 2048, relative to its max |value| (adj / node)")
        print("| T | nosc Euler | nosc 2M | tiny Euler | tiny 2M |")
        tabs = {name: error_table(name) for name in ("nosc", "tiny")}
        for T_ in tabs["nosc"]:
            cells = [f"{tabs[name][T_][s][0]:.2e} / {tabs[name][T_][s][1]:.2e}" for name in ("nosc", "tiny") for s in SOLVERS]
            print(f"| {T_} | " + " | ".join(cells) + " |")
        res["error_vs_T"] = {name: {str(T_): row for T_, row in tab.items()} for name, tab in tabs.items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
