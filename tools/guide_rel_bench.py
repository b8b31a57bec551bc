"""Timing of the relation term of box guidance (dsg_sample_guided_rel) -- for the record in profiles/guide_rel_bench.md and DESIGN.md §14.
At the Visual Genome shape, B = 64, 8 Euler steps each, S_churn = 0, the self-conditioning coin never firing, all in one process:
  the plain step (sampler.sample),
  the guided step without relations (sampler.sample_guided with the three box losses: the parent's form),
  the guided step with the relation term, kinds given,
  the guided step with the relation term, kinds decoded from the adjacency estimate of every call,
  the same with a sparse table (6 of the 51 predicates carry a kind: closer to a real vocabulary; GR_SPARSE=0 leaves it out).
HIP-event times over GR_ITERS iterations after GR_WARMUP, median (and minimum); one JSON line at the end.
    python tools/guide_rel_bench.py [--md profiles/guide_rel_bench.md] [--kernel-stats <rocprofv3 --kernel-trace --stats kernel_stats.csv>]
--md writes the record; --kernel-stats adds the time per launch of the guide kernels from a kernel trace of this tool (a run of its own:
tracing slows the events down; trace with GR_SPARSE=0 so that a kernel's average is over one variant).
GR_BATCH=64  GR_ITERS=20  GR_WARMUP=3  GR_CONFIG=vg  GR_SPARSE=1"""
import argparse
import csv
import json
import os
import re
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from diffusesg_amd import guide, synth as Y, weights as W          # noqa: E402
from diffusesg_amd.model import build_network                      # noqa: E402
from diffusesg_amd.sampler import NodeAdjEDMSamplerHip             # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--md", default=None)
ap.add_argument("--kernel-stats", default=None)
args = ap.parse_args()
ITERS, WARMUP = int(os.environ.get("GR_ITERS", "20")), int(os.environ.get("GR_WARMUP", "3"))
NAME, B = os.environ.get("GR_CONFIG", "vg"), int(os.environ.get("GR_BATCH", "64"))
STEPS, N_ADJ_TYPE = 8, 51


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


cfg = Y.CONFIGS[NAME]()
n = cfg.max_node_num
valid = [max(1, n - (7 * b) % (n // 2)) for b in range(B)]   # ragged: between half and all of the nodes
flags_np = W.synth_flags(B, n, valid)
flags = torch.from_numpy(flags_np).cuda()
net = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")
rng = np.random.default_rng(0)
sel = torch.from_numpy((rng.random((B, n)) < 0.5).astype(np.uint8))
lo = rng.uniform(0.0, 0.5, (B, n, 2))
rects = torch.from_numpy(np.concatenate([lo, lo + 0.4], -1).astype(np.float32))
box = dict(overlap=1.0, region=(sel, rects), align=0.5, tau=0.05)
table = rng.integers(0, guide.REL_KINDS, N_ADJ_TYPE).astype(np.uint8)   # every predicate means something: the densest the term gets
table[0] = 0
kinds = torch.from_numpy(table[rng.integers(0, N_ADJ_TYPE, (B, n, n))])
guides = {"guided": guide.BoxGuide(**box),
          "given": guide.BoxGuide(relations=kinds, relation_margin=0.02, **box),
          "decoded": guide.BoxGuide(relations=guide.SpatialRules(table, N_ADJ_TYPE, "bits"), relation_margin=0.02, **box)}
sparse = np.zeros(N_ADJ_TYPE, np.uint8)
sparse[[3, 11, 19, 27, 35, 43]] = [guide.REL_ABOVE, guide.REL_BELOW, guide.REL_INSIDE, guide.REL_ON, guide.REL_LEFT_OF, guide.REL_CONTAINS]
if os.environ.get("GR_SPARSE", "1") != "0":
    guides["decoded_sparse"] = guide.BoxGuide(relations=guide.SpatialRules(sparse, N_ADJ_TYPE, "bits"), relation_margin=0.02, **box)
smp = NodeAdjEDMSamplerHip(num_steps=STEPS, solver="euler", S_churn=0, self_condition=cfg.self_condition)
kw = dict(seed=1, coins=np.zeros(STEPS, np.uint8), return_device=True)
plain = lambda: smp.sample(net, flags, num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj, **kw)
t = {"plain": timed(plain)}
for name, g in guides.items():
    t[name] = timed(lambda g=g: smp.sample_guided(net, flags, g, 1.0, clip_ratio=1.0, **kw))
t["plain_again"] = timed(plain)   # again: the drift of the job
base = min(t["plain"][0], t["plain_again"][0])
row = dict(config=NAME, B=B, steps=STEPS, iters=ITERS, adjacency_mb_per_call=4.0 * B * cfg.c_adj * n * n / 1e6)
for name, (med, mn) in t.items():
    row[name + "_step_ms"] = med / STEPS
for name in guides:
    row[name + "_over_plain"] = t[name][0] / base
    row[name + "_per_call_us"] = (t[name][0] - base) / STEPS * 1e3
for name in [k for k in guides if k != "guided"]:
    row[name + "_over_guided"] = t[name][0] / t["guided"][0]
    row[name + "_more_per_call_us"] = (t[name][0] - t["guided"][0]) / STEPS * 1e3

kernels = []
if args.kernel_stats:
    for r in csv.DictReader(open(args.kernel_stats)):
        name = re.sub(r"\(.*", "", r["Name"]).replace("void ", "").replace("dsg::", "")
        if name.startswith(("box_guide", "graph_diff_norm", "elem_kernel<EulerGuided")):
            kernels.append((name, int(r["Calls"]), float(r["AverageNs"]) / 1e3))
    row["kernels_us"] = {k: us for k, _c, us in kernels}

lines = [
    "# Box guidance, the relation term: cost of a guided step",
    "",
    f"`python tools/guide_rel_bench.py` (GR_ITERS={ITERS}, GR_WARMUP={WARMUP}) on one MI355X: the {NAME} network, `B = {B}`, ragged graphs of "
    f"{min(valid)} to {max(valid)} valid nodes, {STEPS} Euler steps, `S_churn = 0`, the self-conditioning coin never firing, captured step",
    "bodies, the clip on; HIP-event medians, all variants in one process.  Every guide carries the three box losses (overlap 1, region on",
    f"half of the nodes, alignment 0.5, `tau = 0.05`); the relation term has weight 1, margin 0.02 and a table in which {int((table != 0).sum())} of "
    f"the {N_ADJ_TYPE} predicates carry a kind, so nearly every live pair contributes.  The decoded pass reads {row['adjacency_mb_per_call']:.1f} MB",
    "of adjacency estimate per call.",
    "",
    "| variant | step | against the plain step | more per call |",
    "|---|---|---|---|",
    f"| plain | {row['plain_step_ms']:.3f} ms (again: {row['plain_again_step_ms']:.3f} ms) | 1 | |",
]
for name, what in (("guided", "guided, no relations (the parent's form)"), ("given", "guided, relations given"), ("decoded", "guided, relations decoded"),
                   ("decoded_sparse", "guided, relations decoded, 6 of 51 predicates carry a kind")):
    if name in guides:
        lines.append(f"| {what} | {row[name + '_step_ms']:.3f} ms | x{row[name + '_over_plain']:.4f} | +{row[name + '_per_call_us']:.1f} us |")
lines += ["",
          "Against the guided step without relations: " + ", ".join(
              f"{name.replace('_', ' ')} x{row[name + '_over_guided']:.4f} ({row[name + '_more_per_call_us']:+.1f} us per call)" for name in guides if name != "guided")
          + ".  Ratios against the plain step use the smaller",
          "of its two timings; the two differ by the drift of the job, which is the spread a difference has to clear."]
if kernels:
    lines += ["", "A kernel trace of the same tool (`rocprofv3 --kernel-trace --stats`, a run of its own), average per launch:", "",
              "| kernel | launches | time per launch |", "|---|---|---|"]
    lines += [f"| `{k}` | {c} | {us:.1f} us |" for k, c, us in sorted(kernels)]
lines.append("")
if args.md:
    with open(args.md, "w") as f:
        f.write("\n".join(lines))
print("\n".join(lines))
print(json.dumps(row))
