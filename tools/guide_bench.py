"""Timing of the input-gradient entry and of guided sampling -- for the record in profiles/ and DESIGN.md §11.
  dsg_precond_vjp (forward in training form + backward without weight gradients) against dsg_train_step_grads (the same with them)
  and against dsg_precond (the sampling path's forward), at the Visual Genome shape;
  a guided sampler step against a plain one (8 Euler steps each, self-conditioning coin never firing).
HIP-event times over GB_ITERS iterations after GB_WARMUP, median; one JSON line at the end.
GB_BATCHES=64  GB_ITERS=10  GB_WARMUP=3  GB_CONFIG=vg"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from diffusesg_amd import guide, synth as Y, weights as W          # noqa: E402
from diffusesg_amd.model import build_network                      # noqa: E402
from diffusesg_amd.sampler import NodeAdjEDMSamplerHip             # noqa: E402
from diffusesg_amd.train import NodeAdjEDMObjectiveGeneratorHip, NodeAdjRainbowLossHip, train_step_grads   # noqa: E402

T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
ITERS, WARMUP = int(os.environ.get("GB_ITERS", "10")), int(os.environ.get("GB_WARMUP", "3"))
NAME = os.environ.get("GB_CONFIG", "vg")


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


class _NoCoin:
    def __enter__(self):
        self.orig = np.random.rand
        np.random.rand = lambda *a: 0.9

    def __exit__(self, *a):
        np.random.rand = self.orig


out = {"config": NAME, "iters": ITERS, "rows": []}
for B in [int(b) for b in os.environ.get("GB_BATCHES", "64").split(",")]:
    cfg, flags, ca, cn, rnd, ea, en, _coin = Y.train_case(NAME, B=B)
    net = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")
    gen = NodeAdjEDMObjectiveGeneratorHip(precond="edm", sigma_dist="edm", other_params=None, dev="cuda", symmetric_noise=False)
    lf = NodeAdjRainbowLossHip(edge_loss_weight=1.0, node_loss_weight=1.0, flag_reweight=False, objective="edm")
    a, x, f = T(ca), T(cn), T(flags)
    na, nx, _, ta, tx, (_cs, _co, _ci, _cn, sigmas, weights) = gen.get_input_output(a, x, f)
    g = (torch.randn_like(na), torch.randn_like(nx))
    loss_fn = guide.box_overlap_loss(f)
    with _NoCoin():
        t_step = timed(lambda: train_step_grads(net, lf, na, nx, f, sigmas, ta, tx, weights, iou_loss_weight=1.0, iou_loss_type="giou"))
        t_vjp = timed(lambda: net.value_and_input_grad(na, nx, f, sigmas, grad_outputs=g, coin=False))
        t_cb = timed(lambda: net.value_and_input_grad(na, nx, f, sigmas, loss_fn=loss_fn, coin=False))
        t_fwd = timed(lambda: net(na, nx, f, sigmas))
        steps = 8
        smp = NodeAdjEDMSamplerHip(num_steps=steps, solver="euler", S_churn=0, self_condition=cfg.self_condition)
        t_plain = timed(lambda: smp.sample(net, f, seed=1, num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj, return_device=True))
        t_guided = timed(lambda: guide.guided_sample(net, smp, f, loss_fn, 1.0, seed=1))
    row = dict(B=B, train_step_grads_ms=t_step[0], precond_vjp_ms=t_vjp[0], precond_vjp_callback_ms=t_cb[0], precond_ms=t_fwd[0],
               vjp_over_train_step=t_vjp[0] / t_step[0], vjp_over_precond=t_vjp[0] / t_fwd[0],
               plain_step_ms=t_plain[0] / steps, guided_step_ms=t_guided[0] / steps, guided_over_plain=t_guided[0] / t_plain[0])
    out["rows"].append(row)
    print(f"{NAME} B={B}: dsg_train_step_grads {t_step[0]:.2f} ms | dsg_precond_vjp {t_vjp[0]:.2f} ms (x{row['vjp_over_train_step']:.3f} of the "
          f"training step; with a torch loss callback {t_cb[0]:.2f} ms) | dsg_precond {t_fwd[0]:.2f} ms (vjp = x{row['vjp_over_precond']:.2f})\n"
          f"   sampler step, {steps} Euler steps: plain {row['plain_step_ms']:.2f} ms, guided {row['guided_step_ms']:.2f} ms "
          f"(x{row['guided_over_plain']:.2f})", flush=True)
print(json.dumps(out))
