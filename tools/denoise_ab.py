"""dev helper: dsg_denoise on caller tensors, VG shape: time per call (HIP events around `calls` back-to-back forwards), `rounds` times.
    python tools/denoise_ab.py [--option NAME A B] [--batch 64] [--valid 64] [--rounds 4] [--calls 30] [--dump FILE]
Without --option: this tree's library as it is (run the parent's checkout and this one in alternating processes).  With it: the
option alternating between the two values on one handle, and whether the two values' outputs are bit-identical.
--valid 64: all-true flags, every list is full.  --dump FILE: the outputs (adj, node) as an .npz, for a comparison across trees."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from diffusesg_amd import spec as S
from diffusesg_amd import weights as W
from diffusesg_amd.model import build_network

ap = argparse.ArgumentParser()
ap.add_argument("--option", nargs=3, metavar=("NAME", "A", "B"), default=None)
ap.add_argument("--dump", default=None)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--valid", type=int, default=64)
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--calls", type=int, default=30)
args = ap.parse_args()

cfg = S.vg_config()
net = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda").model
B, n = args.batch, cfg.max_node_num
flags = W.synth_flags(B, n, args.valid)
T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
adj = T(W.mask_adj(W.normal(3, "denoise_ab/adj", (B, cfg.c_adj, n, n)), flags))
node = T(W.mask_node(W.normal(3, "denoise_ab/node", (B, n, cfg.c_node)), flags))
fl, c_noise = T(flags), T(np.linspace(-1.4, 1.1, B).astype(np.float32))
net(adj, node, fl, c_noise)
h = net._ensure_handle()
name = args.option[0] if args.option else None
values = (int(args.option[1]), int(args.option[2])) if args.option else (None,)
times, outs = {v: [] for v in values}, {}
for r in range(args.rounds):
    for v in values:
        if name:
            h.set_option(name, v)
        for _ in range(3):
            out = net(adj, node, fl, c_noise)
        outs[v] = [t.clone() for t in out]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            net(adj, node, fl, c_noise)
        e1.record()
        torch.cuda.synchronize()
        times[v].append(e0.elapsed_time(e1) * 1e3 / args.calls)
for v in values:
    print((f"{name} {v}: " if name else "") + "us per call " + "  ".join(f"{t:.1f}" for t in times[v])
          + f"   min {min(times[v]):.1f} max {max(times[v]):.1f}")
if name:
    print("outputs bit-identical:", all(torch.equal(x, y) for x, y in zip(outs[values[0]], outs[values[1]])))
if args.dump:
    np.savez(args.dump, adj=outs[values[-1]][0].cpu().numpy(), node=outs[values[-1]][1].cpu().numpy())
