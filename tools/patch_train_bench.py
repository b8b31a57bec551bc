#!/usr/bin/env python3
"""Time per training iteration and per value_and_input_grad call at the Visual Genome shape, B = 64, for patch_size 1 (`vg`) and
patch_size 2 (`vg_p2`) -- tools/time_train.py's method: a host clock around calls that end in a device synchronise, the
self-conditioning coin forced so that the two kinds of iteration are timed apart.  Every shape is warmed up first; the patch sizes are
timed alternately in `--rounds` rounds of `--iters` calls each, and the spread over the rounds is reported next to the median, so that
a difference can be read against the run-to-run spread.  Synthetic weights: nothing is said about convergence or sample quality.

  python tools/patch_train_bench.py [--batch 64] [--iters 8] [--rounds 3] [--patch-sizes 1,2] [--root DIR] [--out profiles/patch_train_bench.md]

--root DIR imports the package of another tree (a build of another commit) instead of this one: with --patch-sizes 1 it gives that
build's p = 1 times under the same method, for the comparison with the parent commit.  The table is printed and appended to --out (--out "" prints only)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--patch-sizes", default="1,2")
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "patch_train_bench.md"))
    ap.add_argument("--label", default="this build")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    from diffusesg_amd import synth as Y, weights as W
    from diffusesg_amd.model import build_network
    from diffusesg_amd.train import AdamHip, EMAHip, NodeAdjEDMObjectiveGeneratorHip, NodeAdjRainbowLossHip, train_one_iteration
    assert torch.cuda.is_available(), "patch_train_bench needs the GPU: a CPU run gives no time"
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    B = args.batch
    cfg1, flags, ca, cn, rnd, ea, en, coin = Y.train_case("vg", B=B)
    nets = {}
    for p in [int(v) for v in args.patch_sizes.split(",")]:
        cfg = cfg1 if p == 1 else Y.PATCH_CONFIGS[f"vg_p{p}"]()
        model = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")
        nets[p] = dict(model=model, opt=AdamHip(model), emas=[EMAHip(model, beta=0.9999)])
    gen = NodeAdjEDMObjectiveGeneratorHip(precond="edm", sigma_dist="edm", other_params=None, dev="cuda", symmetric_noise=False)
    lf = NodeAdjRainbowLossHip(edge_loss_weight=1.0, node_loss_weight=1.0, flag_reweight=False, objective="edm")
    a, x, f = T(ca), T(cn), T(flags)
    sig = torch.full((B,), 1.5, device="cuda")
    ga, gx = torch.randn_like(a), torch.randn_like(x)

    def run(p, kind):
        n = nets[p]
        real = np.random.rand
        np.random.rand = lambda *v: 0.9 if kind == "iteration, no self-cond pass" else 0.1
        try:
            if kind.startswith("iteration"):
                train_one_iteration(n["model"], gen, lf, n["opt"], n["emas"], a, x, f, iou_loss_weight=1.0, iou_loss_type="giou")
            else:
                n["model"].value_and_input_grad(a, x, f, sig, grad_outputs=(ga, gx), coin=False)
        finally:
            np.random.rand = real

    kinds = ("iteration, no self-cond pass", "iteration, with self-cond pass", "value_and_input_grad")
    times = {(p, k): [] for p in nets for k in kinds}
    for p in nets:                      # warm-up: every shape the timed windows use
        for k in kinds:
            for _ in range(2):
                run(p, k)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k in kinds:
            for p in nets:              # the patch sizes alternate inside a round
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(args.iters):
                    run(p, k)
                torch.cuda.synchronize()
                times[(p, k)].append((time.perf_counter() - t0) / args.iters)
    lines = [f"Visual Genome shape, B = {B}, {args.label}: {args.rounds} rounds of {args.iters} calls, ms per call, median (min .. max over rounds)", "",
             "| call | " + " | ".join(f"p = {p}" for p in nets) + (" | p = 2 / p = 1 |" if 1 in nets and 2 in nets else " |"),
             "|---|" + "---|" * (len(nets) + (1 if 1 in nets and 2 in nets else 0))]
    for k in kinds:
        cells = [f"{1e3 * statistics.median(times[(p, k)]):.1f} ({1e3 * min(times[(p, k)]):.1f} .. {1e3 * max(times[(p, k)]):.1f})" for p in nets]
        if 1 in nets and 2 in nets:
            cells.append(f"{statistics.median(times[(2, k)]) / statistics.median(times[(1, k)]):.2f}")
        lines.append(f"| {k} | " + " | ".join(cells) + " |")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(text + "\n\n")


if __name__ == "__main__":
    main()
