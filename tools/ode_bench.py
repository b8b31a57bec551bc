"""Timing of the probability-flow ODE encoder -- for the record in profiles/ode_bench.md and DESIGN.md §12.  Not part of any test.
  encode without a probe (forwards only), encode with a device-drawn Rademacher probe (forward + input-gradient backward + the probe,
  assemble and per-graph contraction kernels per evaluation), and the same number of bare dsg_precond_vjp calls on the same inputs, in
  one process, alternating, at the Visual Genome shape.  The new kernels' share is (run with probe - bare calls) / run with probe: the
  state updates, the probe draw, the contraction and whatever the loop adds around the calls.
Host clock around work that ends in a device synchronise; OB_REPS repetitions after OB_WARMUP, median and spread; one JSON line at the end.
OB_BATCH=16  OB_STEPS=32  OB_SOLVER=heun  OB_REPS=5  OB_WARMUP=2  OB_CONFIG=vg"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from diffusesg_amd import lib, ode, synth as Y, weights as W      # noqa: E402
from diffusesg_amd.model import build_network                      # noqa: E402
from diffusesg_amd.sampler import NodeAdjEDMSamplerHip             # noqa: E402

NAME = os.environ.get("OB_CONFIG", "vg")
B, STEPS, SOLVER = int(os.environ.get("OB_BATCH", "16")), int(os.environ.get("OB_STEPS", "32")), os.environ.get("OB_SOLVER", "heun")
REPS, WARMUP = int(os.environ.get("OB_REPS", "5")), int(os.environ.get("OB_WARMUP", "2"))

cfg = Y.CONFIGS[NAME]()
n = cfg.max_node_num
valid = [max(2, (n * (3 + (7 * b) % 11)) // 16) for b in range(B)]          # ragged: 3/16 .. 13/16 of the nodes
flags = W.synth_flags(B, n, valid)
sign = lambda v: np.where(v >= 0, np.float32(1), np.float32(-1)).astype(np.float32)
adj = W.mask_adj(sign(W.normal(41, "odebench/adj", (B, cfg.c_adj, n, n))), flags)
node = W.mask_node(sign(W.normal(41, "odebench/node", (B, n, cfg.c_node))), flags)
T = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
a, x, f = T(adj), T(node), T(flags)
net = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")
smp = NodeAdjEDMSamplerHip(num_steps=STEPS, solver=SOLVER, S_churn=0, self_condition=cfg.self_condition)
t_eval, _ = lib.ode_evals(smp._cfg(), lib.make_ode_cfg("encode", "rademacher"))
seeds = list(range(100, 100 + B))
g = (torch.ones_like(a), torch.ones_like(x))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def bare():
    for t in t_eval:
        net.value_and_input_grad(a, x, f, float(t), grad_outputs=g, coin=False)


runs = {"encode_no_probe": lambda: ode.run(net, smp, a, x, f, "encode"),
        "encode_probe": lambda: ode.run(net, smp, a, x, f, "encode", "rademacher", seeds),
        "bare_vjp_calls": bare}
ms = {k: [] for k in runs}
for r in range(WARMUP + REPS):
    for k, fn in runs.items():          # alternating: the three share whatever the machine does meanwhile
        t = wall(fn)
        if r >= WARMUP:
            ms[k].append(t)
med = {k: float(np.median(v)) for k, v in ms.items()}
share = (med["encode_probe"] - med["bare_vjp_calls"]) / med["encode_probe"]
out = dict(config=NAME, B=B, steps=STEPS, solver=SOLVER, n_evals=int(len(t_eval)), reps=REPS, median_ms=med,
           min_ms={k: float(np.min(v)) for k, v in ms.items()}, max_ms={k: float(np.max(v)) for k, v in ms.items()},
           new_kernels_share=share, per_eval_ms={k: med[k] / len(t_eval) for k in med})
print(f"{NAME} B={B} T={STEPS} {SOLVER} ({len(t_eval)} evaluations): encode without a probe {med['encode_no_probe']:.1f} ms | with a probe "
      f"{med['encode_probe']:.1f} ms | {len(t_eval)} bare dsg_precond_vjp calls {med['bare_vjp_calls']:.1f} ms | new kernels' share "
      f"{100 * share:.1f} %", flush=True)
print(json.dumps(out))
