"""Timing of box guidance through the skip path (dsg_sample_guided) -- for the record in profiles/guide_skip_bench.md and DESIGN.md §13.
At the Visual Genome shape, 8 Euler steps each, S_churn = 0, the self-conditioning coin never firing, all in one process:
  the plain step (sampler.sample),
  the skip-guided step (sampler.sample_guided, all three box losses) with the clip and without,
  the eager input-space guided step (guide.guided_sample with the same loss as a torch closure).
HIP-event times over GS_ITERS iterations after GS_WARMUP, median (and minimum); one JSON line at the end.
GS_BATCHES=64  GS_ITERS=10  GS_WARMUP=3  GS_CONFIG=vg  GS_EAGER=1 (0: skip the eager loop)"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from diffusesg_amd import guide, synth as Y, weights as W          # noqa: E402
from diffusesg_amd.model import build_network                      # noqa: E402
from diffusesg_amd.sampler import NodeAdjEDMSamplerHip             # noqa: E402

ITERS, WARMUP = int(os.environ.get("GS_ITERS", "10")), int(os.environ.get("GS_WARMUP", "3"))
NAME = os.environ.get("GS_CONFIG", "vg")
EAGER = os.environ.get("GS_EAGER", "1") != "0"
STEPS = 8


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


out = {"config": NAME, "iters": ITERS, "steps": STEPS, "rows": []}
for B in [int(b) for b in os.environ.get("GS_BATCHES", "64").split(",")]:
    cfg = Y.CONFIGS[NAME]()
    n = cfg.max_node_num
    valid = [max(1, n - (7 * b) % (n // 2)) for b in range(B)]   # ragged: between half and all of the nodes
    flags = torch.from_numpy(W.synth_flags(B, n, valid)).cuda()
    net = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")
    rng = np.random.default_rng(0)
    sel = torch.from_numpy((rng.random((B, n)) < 0.5).astype(np.uint8))
    lo = rng.uniform(0.0, 0.5, (B, n, 2))
    rects = torch.from_numpy(np.concatenate([lo, lo + 0.4], -1).astype(np.float32))
    bg = guide.BoxGuide(overlap=1.0, region=(sel, rects), align=0.5, tau=0.05)
    smp = NodeAdjEDMSamplerHip(num_steps=STEPS, solver="euler", S_churn=0, self_condition=cfg.self_condition)
    coins = np.zeros(STEPS, np.uint8)
    kw = dict(seed=1, coins=coins, return_device=True)
    t_plain = timed(lambda: smp.sample(net, flags, num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj, **kw))
    t_clip = timed(lambda: smp.sample_guided(net, flags, bg, 1.0, clip_ratio=1.0, **kw))
    t_noclip = timed(lambda: smp.sample_guided(net, flags, bg, 1.0, clip_ratio=None, **kw))
    t_plain2 = timed(lambda: smp.sample(net, flags, num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj, **kw))   # again: the drift of the job
    t_eager = None
    if EAGER:
        loss_fn = bg.torch_loss(flags)
        orig = np.random.rand
        np.random.rand = lambda *a: 0.9   # the eager loop draws its coins from NumPy: never firing, like `coins` above
        try:
            t_eager = timed(lambda: guide.guided_sample(net, smp, flags, loss_fn, 1.0, clip_ratio=1.0, seed=1))
        finally:
            np.random.rand = orig
    plain = min(t_plain[0], t_plain2[0])
    row = dict(B=B, plain_step_ms=t_plain[0] / STEPS, plain_again_step_ms=t_plain2[0] / STEPS, guided_clip_step_ms=t_clip[0] / STEPS,
               guided_noclip_step_ms=t_noclip[0] / STEPS, guided_clip_over_plain=t_clip[0] / plain, guided_noclip_over_plain=t_noclip[0] / plain,
               per_call_clip_us=(t_clip[0] - plain) / STEPS * 1e3, per_call_noclip_us=(t_noclip[0] - plain) / STEPS * 1e3,
               eager_step_ms=None if t_eager is None else t_eager[0] / STEPS, eager_over_plain=None if t_eager is None else t_eager[0] / plain)
    out["rows"].append(row)
    print(f"{NAME} B={B}, {STEPS} Euler steps, per step: plain {row['plain_step_ms']:.3f} ms (again {row['plain_again_step_ms']:.3f}) | skip-guided with clip "
          f"{row['guided_clip_step_ms']:.3f} ms (x{row['guided_clip_over_plain']:.4f}, +{row['per_call_clip_us']:.1f} us per call) | without clip "
          f"{row['guided_noclip_step_ms']:.3f} ms (x{row['guided_noclip_over_plain']:.4f}, +{row['per_call_noclip_us']:.1f} us per call)"
          + ("" if t_eager is None else f" | eager input-space guided {row['eager_step_ms']:.3f} ms (x{row['eager_over_plain']:.2f})"), flush=True)
print(json.dumps(out))
