"""Timing of content guidance (dsg_sample_guided_content) -- for the record in profiles/guide_content_bench.md and DESIGN.md §17.
At the Visual Genome bits shape (N = 64, C_adj = 6, C_node = 12), B = 64, 8 Euler steps each, S_churn = 0, the self-conditioning coin
never firing, captured step bodies, both clips on, all in one process:
  the plain step (sampler.sample),
  the box-guided step (sampler.sample_guided with the three box losses: the parent's form),
  the content-guided step at K = 1, 4, 16 items per graph (full triplets) next to the same box guide, in both forms of the content
  kernel (one block per graph; the (graph, item) grid), forced through DSG_CONTENT_GRID = 0 / 1,
  the one-hot widths (C_adj = 51, C_node = 154, Cl = 150) at K = 4: the same network geometry with those channel counts, its own plain step.
HIP-event times over GC_ITERS iterations after GC_WARMUP, median (and minimum); one JSON line at the end.
    python tools/guide_content_bench.py [--md profiles/guide_content_bench.md] [--package-root DIR] [--parent-json FILE ...]
--package-root DIR imports diffusesg_amd from DIR (a checkout of another commit with its library built): variants that commit lacks
are left out, which is how the parent commit is timed alternately with this one; --parent-json adds such runs' JSON lines to the record.
GC_BATCH=64  GC_ITERS=20  GC_WARMUP=3  GC_ONEHOT=1"""
import argparse
import dataclasses
import json
import os
import sys

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--md", default=None)
ap.add_argument("--package-root", default=None)
ap.add_argument("--parent-json", nargs="*", default=[])
ap.add_argument("--own-json", nargs="*", default=[])
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.package_root) if args.package_root else os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from diffusesg_amd import guide, synth as Y, weights as W          # noqa: E402
from diffusesg_amd.model import build_network                      # noqa: E402
from diffusesg_amd.sampler import NodeAdjEDMSamplerHip             # noqa: E402

ITERS, WARMUP, B = int(os.environ.get("GC_ITERS", "20")), int(os.environ.get("GC_WARMUP", "3")), int(os.environ.get("GC_BATCH", "64"))
STEPS, N_NODE_TYPE, N_ADJ_TYPE = 8, 150, 51
HAS_CONTENT = hasattr(guide, "ContentGuide")
FORMS = (("block", "0"), ("grid", "1"))   # one block per graph / the (graph, item) grid


def timed(fn):
    for _ in range(WARMUP):
        fn()
    ms = []
    for _ in range(ITERS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms))


def items(K, rng):
    return [[(int(rng.integers(N_NODE_TYPE)), int(rng.integers(N_ADJ_TYPE)), int(rng.integers(N_NODE_TYPE))) for _ in range(K)] for _ in range(B)]


def measure(cfg, encoding, ks, with_box_only):
    n = cfg.max_node_num
    valid = [max(1, n - (7 * b) % (n // 2)) for b in range(B)]   # ragged: between half and all of the nodes
    flags = torch.from_numpy(W.synth_flags(B, n, valid)).cuda()
    net = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")
    rng = np.random.default_rng(0)
    sel = torch.from_numpy((rng.random((B, n)) < 0.5).astype(np.uint8))
    lo = rng.uniform(0.0, 0.5, (B, n, 2))
    rects = torch.from_numpy(np.concatenate([lo, lo + 0.4], -1).astype(np.float32))
    box = guide.BoxGuide(overlap=1.0, region=(sel, rects), align=0.5, tau=0.05)
    smp = NodeAdjEDMSamplerHip(num_steps=STEPS, solver="euler", S_churn=0, self_condition=cfg.self_condition)
    kw = dict(seed=1, coins=np.zeros(STEPS, np.uint8), return_device=True)
    plain = lambda: smp.sample(net, flags, num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj, **kw)
    t = {"plain": timed(plain)}
    if with_box_only:
        t["guided"] = timed(lambda: smp.sample_guided(net, flags, box, 1.0, clip_ratio=1.0, **kw))
    if HAS_CONTENT:
        for K in ks:
            cg = guide.ContentGuide(items(K, rng), N_NODE_TYPE, N_ADJ_TYPE, node_encoding=encoding, edge_encoding=encoding, tau=0.5, clip_ratio=1.0)
            for form, env in FORMS:   # both forms of the content kernel: the plan reads the variable at every call, bodies are keyed by the form
                os.environ["DSG_CONTENT_GRID"] = env
                t[f"content_k{K}_{form}"] = timed(lambda cg=cg: smp.sample_guided(net, flags, box, 1.0, clip_ratio=1.0, content=cg, **kw))
            del os.environ["DSG_CONTENT_GRID"]
    t["plain_again"] = timed(plain)   # again: the drift of the job
    del net
    torch.cuda.empty_cache()
    return t, (min(valid), max(valid))


vg = Y.CONFIGS["vg"]()
t, vr = measure(vg, "bits", (1, 4, 16), True)
row = dict(B=B, steps=STEPS, iters=ITERS, package_root=args.package_root or ".", has_content=HAS_CONTENT)


def fill(prefix, t):
    base = min(t["plain"][0], t["plain_again"][0])
    for name, (med, mn) in t.items():
        row[prefix + name + "_step_ms"] = med / STEPS
        if name not in ("plain", "plain_again"):
            row[prefix + name + "_over_plain"] = med / base
            row[prefix + name + "_more_per_call_us"] = (med - t["guided"][0]) / STEPS * 1e3
            row[prefix + name + "_over_guided"] = med / t["guided"][0]


fill("", t)
if HAS_CONTENT and os.environ.get("GC_ONEHOT", "1") != "0":
    to, _ = measure(dataclasses.replace(vg, c_adj=N_ADJ_TYPE, c_node=N_NODE_TYPE + 4), "one_hot", (4,), True)
    fill("onehot_", to)


def table(prefix, ks):
    out = ["| variant | step | against the plain step | more per call than the box-guided step |", "|---|---|---|---|",
           f"| plain | {row[prefix + 'plain_step_ms']:.3f} ms (again: {row[prefix + 'plain_again_step_ms']:.3f} ms) | 1 | |",
           f"| box-guided (the parent's form) | {row[prefix + 'guided_step_ms']:.3f} ms | x{row[prefix + 'guided_over_plain']:.4f} | |"]
    for K in ks:
        for form, what in (("block", "one block per graph"), ("grid", "grid form")):
            k = f"{prefix}content_k{K}_{form}"
            out.append(f"| box + content, K = {K}, {what} | {row[k + '_step_ms']:.3f} ms | x{row[k + '_over_plain']:.4f} | "
                       f"{row[k + '_more_per_call_us']:+.1f} us (x{row[k + '_over_guided']:.4f}) |")
    return out


def reading(row):
    """the closing section of the record, from the figures above"""
    pct = lambda k: 100.0 * (row[k + "_over_guided"] - 1.0)
    oh = "onehot_content_k4_block_over_guided" in row
    out = ["## Reading", "",
           "* One block per graph is B blocks with the items one after another: on top of the box-guided step "
           f"{pct('content_k1_block'):.1f} % at K = 1, {pct('content_k4_block'):.1f} % at K = 4, {pct('content_k16_block'):.1f} % at K = 16"
           + (f", {pct('onehot_content_k4_block'):.1f} % at the one-hot widths with K = 4." if oh else "."),
           f"* The grid form, the default: {pct('content_k1_grid'):.1f} % at K = 1, {pct('content_k4_grid'):.1f} % at K = 4, {pct('content_k16_grid'):.1f} % at K = 16"
           + (f", {pct('onehot_content_k4_grid'):.1f} % at the one-hot widths with K = 4." if oh else "."),
           "* Both forms give the same bits (`tests/test_content_guide.py::test_both_forms_give_the_same_bits`); the one-block form is kept for",
           "  this comparison only."]
    return out


if HAS_CONTENT:
    lines = [
        "# Content guidance: cost of a guided step",
        "",
        f"`python tools/guide_content_bench.py` (GC_ITERS={ITERS}, GC_WARMUP={WARMUP}) on one MI355X: the vg network (`N = 64`, `C_adj = 6`,",
        f"`C_node = 12`, labels and predicates in bits), `B = {B}`, ragged graphs of {vr[0]} to {vr[1]} valid nodes, {STEPS} Euler steps, `S_churn = 0`, the",
        "self-conditioning coin never firing, captured step bodies; HIP-event medians, all variants in one process.  The box guide carries its",
        "three losses (overlap 1, region on half of the nodes, alignment 0.5) with its clip on; the content guide has K full triplets per graph,",
        "`tau = 0.5`, weight 1 and its own clip on, and runs NEXT TO the box guide.  Both forms of the content kernel are timed, each forced",
        "through `DSG_CONTENT_GRID`: one block per graph, and the grid form (K x B blocks for the item phase, N^2/512 x B for the pair-major phase, then one block per graph).",
        ""] + table("", (1, 4, 16))
    if "onehot_plain_step_ms" in row:
        lines += ["", f"The one-hot widths (`C_adj = {N_ADJ_TYPE}`, `C_node = {N_NODE_TYPE + 4}`, `Cl = {N_NODE_TYPE}`; the same network geometry with those channel "
                  f"counts; a graph's adjacency estimate is {4.0 * N_ADJ_TYPE * 64 * 64 / 1e6:.2f} MB: streamed, not held on chip):", ""] + table("onehot_", (4,))
    lines += ["", "Ratios against the plain step use the smaller of its two timings; the two differ by the drift of the job, which is the spread a",
              "difference has to clear."]
    runs = [(what, [json.loads(open(p).read().strip().splitlines()[-1]) for p in paths]) for what, paths in (("parent", args.parent_json), ("this commit", args.own_json)) if paths]
    if runs:
        lines += ["", "The parent commit and this one, run alternately in one job (each line a process of its own, this tool with `--package-root`):", "",
                  "| run | plain step | box-guided step |", "|---|---|---|"]
        for what, rs in runs:
            for k, r in enumerate(rs):
                lines.append(f"| {what}, run {k + 1} | {r['plain_step_ms']:.3f} ms (again: {r['plain_again_step_ms']:.3f} ms) | {r['guided_step_ms']:.3f} ms |")
        lines.append(f"| this commit, the run above | {row['plain_step_ms']:.3f} ms (again: {row['plain_again_step_ms']:.3f} ms) | {row['guided_step_ms']:.3f} ms |")
    lines += [""] + reading(row)
    lines.append("")
    if args.md:
        with open(args.md, "w") as f:
            f.write("\n".join(lines))
    print("\n".join(lines))
print(json.dumps(row))
