#!/usr/bin/env python3
"""Write tests/golden/input_grad.npz: the reference's own NodeAdjPrecond.forward under its autograd, with the noisy adjacency and node
inputs requiring grad -- D and dL/d adjs, dL/d nodes for the cases of diffusesg_amd.synth.INPUT_GRAD_CASES.

Development machines only (it imports the reference through the helpers of tools/gen_golden.py: portable generator, `timm` shim);
nothing at run time reads the reference.  The file holds data only: D (strided for the full-size networks) and the full gradients.
The self-conditioning coin is pinned to "does not fire" (the given tensors, or None, are the self-conditioning input, constants as
the reference detaches them); autograd runs on one thread so that its accumulation order, and with it the file, is reproducible.

Usage:  python tools/gen_input_grad_golden.py [--out tests/golden]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G                       # noqa: E402
from diffusesg_amd import synth as Y         # noqa: E402
from diffusesg_amd import guide              # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(G.REPO, "tests", "golden"))
    args = ap.parse_args()
    DiffuseSG, NodeAdjPrecond, _ = G._import_reference()
    import model.precond.precond as P
    torch.set_num_threads(1)
    res, nets = {}, {}
    for tag, (name, valid, _sig, _sc, cot, stride) in Y.INPUT_GRAD_CASES.items():
        cfg, flags, adj, node, sig, sc_adj, sc_node, g_adj, g_node, stride = Y.input_grad_case(tag)
        if name not in nets:
            nets[name] = G.build_ref_net(DiffuseSG, cfg)
        pre = NodeAdjPrecond("edm", nets[name], cfg.self_condition, symmetric_noise=False).eval()
        a_in, n_in = G.squeeze_like_ref(cfg, adj, node)
        a_t, n_t = G.t(a_in.copy()).requires_grad_(True), G.t(n_in.copy()).requires_grad_(True)
        sa = sn = None
        if sc_adj is not None:
            sa, sn = (G.t(v.copy()) for v in G.squeeze_like_ref(cfg, sc_adj, sc_node))
        real = np.random.rand
        P.np.random.rand = lambda: 0.9   # the coin does not fire
        try:
            Da, Dn = pre(a_t, n_t, G.t(flags), G.t(sig), sa, sn)
        finally:
            P.np.random.rand = real
        if cot == "overlap":
            loss = guide.box_overlap_loss()(Da, Dn)
        else:
            ga, gn = G.squeeze_like_ref(cfg, g_adj, g_node)
            loss = (G.t(ga) * Da).sum() + (G.t(gn) * Dn).sum()
        loss.backward()
        Da, Dn = Da.detach().numpy(), Dn.detach().numpy()
        res[f"{tag}/D_adj"] = np.ascontiguousarray(Da[..., ::stride, ::stride])
        res[f"{tag}/D_node"] = Dn
        res[f"{tag}/grad_adj"] = a_t.grad.numpy()
        res[f"{tag}/grad_node"] = n_t.grad.numpy()
        res[f"{tag}/loss"] = np.float64(loss.item())
        f = flags.astype(bool)
        pad = ~(f[:, :, None] & f[:, None, :])
        gpad = a_t.grad.numpy().reshape(len(valid), cfg.c_adj, cfg.max_node_num, cfg.max_node_num)[np.broadcast_to(pad[:, None], (len(valid), cfg.c_adj) + pad.shape[1:])]
        print(f"{tag}: max|D_adj| {np.abs(Da).max():.3f} max|grad_adj| {np.abs(a_t.grad.numpy()).max():.3e} max|grad_node| "
              f"{np.abs(n_t.grad.numpy()).max():.3e} max|grad_adj| at padded pairs {np.abs(gpad).max() if gpad.size else 0.0:.3e}")
    path = os.path.join(args.out, "input_grad.npz")
    np.savez_compressed(path, **res)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
