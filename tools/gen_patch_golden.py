#!/usr/bin/env python3
"""Generate the patch_size > 1 golden vectors (tests/golden/fwd_patch_<name>.npz, sampler_patch.npz) from the reference's own modules.

DEV-CONTAINER ONLY, like tools/gen_golden.py, whose import shim, weight loader (build_ref_net: it passes `patch_size` and asserts
the keys, shapes and constant buffers of diffusesg_amd/spec.py against the reference's state_dict) and replaying sampler driver it
reuses.  Only the output vectors are committed; inputs are regenerated from diffusesg_amd/synth.py (PATCH_CONFIGS, patch_fwd_case).

Per configuration: both outputs with and without self-conditioning, and three intermediates of the self-conditioned forward in
token- / pixel-major layouts -- PatchEmbed's output [B, R^2, E], the final norm's output [B, R^2, E] and the read-out's output
transposed to pixel order [B, N^2, E] -- whole ('inter/<tap>') for the small nets, as row samples ('rows/<tap>') for the two
configurations of synth.PATCH_ROW_SAMPLED: synth.inter_rows of the flattened rows for patch_embed and read_out, and for the norm the
rows of the tokens that own the sampled read_out pixels (synth.patch_owner_rows), so that the read-out formulas can be checked on
them.  'sd_keys' / 'sd_shapes': the reference's state_dict keys and shapes (zero-padded to rank 4).

Usage:  python tools/gen_patch_golden.py [--out tests/golden]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gen_golden import _import_reference, build_ref_net, case_inputs, run_ref_sampler, squeeze_like_ref, t   # noqa: E402
from diffusesg_amd import synth as Y                                                                         # noqa: E402


def gen_forward(DiffuseSG, out):
    for name, mk in Y.PATCH_CONFIGS.items():
        cfg = mk()
        net = build_ref_net(DiffuseSG, cfg)
        B, n, R, E = 2, cfg.max_node_num, cfg.token_res, cfg.embed_dim
        flags, adj, node, sc_adj, sc_node = case_inputs(cfg, B, Y.PATCH_VALID[name], 1, f"fwd/{name}")
        c_noise = Y.FWD_C_NOISE[:B].copy()
        inter, hooks = {}, []

        def mk_hook(key):
            def h(_m, _i, o):
                inter[key] = o.detach().numpy().copy()
            return h
        hooks.append(net.patch_embed.register_forward_hook(mk_hook("patch_embed")))
        hooks.append(net.norm.register_forward_hook(mk_hook("norm")))
        hooks.append(net.read_out.register_forward_hook(mk_hook("read_out")))
        a_in, n_in = squeeze_like_ref(cfg, adj, node)
        res = {}
        with torch.no_grad():
            if cfg.self_condition:
                sa_in, sn_in = squeeze_like_ref(cfg, sc_adj, sc_node)
                oa, on = net(t(a_in.copy()), t(n_in.copy()), t(flags), t(c_noise), t(sa_in.copy()), t(sn_in.copy()))
                res["sc_adj_out"], res["sc_node_out"] = oa.numpy(), on.numpy()
                taps = dict(inter)
            oa, on = net(t(a_in.copy()), t(n_in.copy()), t(flags), t(c_noise), None, None)
            res["nosc_adj_out"], res["nosc_node_out"] = oa.numpy(), on.numpy()
            if not cfg.self_condition:
                taps = dict(inter)
        for h in hooks:
            h.remove()
        pe, nm = taps["patch_embed"].reshape(B * R * R, E), taps["norm"].reshape(B * R * R, E)
        assert taps["read_out"].shape == (B, E, n, n), taps["read_out"].shape
        ro = taps["read_out"].transpose(0, 2, 3, 1).reshape(B * n * n, E)
        if name in Y.PATCH_ROW_SAMPLED:
            res["rows/patch_embed"] = pe[Y.inter_rows(B * R * R)]
            res["rows/read_out"] = ro[Y.inter_rows(B * n * n)]
            res["rows/norm"] = nm[Y.patch_owner_rows(cfg, B)]
        else:
            res["inter/patch_embed"], res["inter/norm"], res["inter/read_out"] = pe.reshape(B, R * R, E), nm.reshape(B, R * R, E), ro.reshape(B, n * n, E)
        sd = net.state_dict()
        keys = sorted(sd.keys())
        res["sd_keys"] = np.array(keys)
        res["sd_shapes"] = np.array([list(sd[k].shape) + [0] * (4 - sd[k].dim()) for k in keys], np.int64)
        res["c_noise"], res["valid"] = c_noise, np.array(Y.PATCH_VALID[name])
        path = os.path.join(out, f"fwd_patch_{name}.npz")
        np.savez_compressed(path, **res)
        print(f"fwd_patch_{name}: adj {res['nosc_adj_out'].shape} max|adj| {np.abs(res['nosc_adj_out']).max():.3f} "
              f"{os.path.getsize(path)} bytes")


def gen_sampler(DiffuseSG, NodeAdjPrecond, NodeAdjEDMSampler, out):
    cfg, res = Y.PATCH_CONFIGS["tiny_p2"](), {}
    for (tag, T, solver, churn) in Y.PATCH_SAMPLER_RUNS:
        a, nd, sig, used = run_ref_sampler(NodeAdjEDMSampler, NodeAdjPrecond, DiffuseSG, cfg, T=T, B=4, valid=Y.SAMPLER_VALID, seed=3,
                                           tag=f"smp_patch/{tag}", solver=solver, S_churn=churn)
        res[f"{tag}_adj"], res[f"{tag}_node"], res[f"{tag}_coins_used"] = a, nd, np.array(used)
        print(f"sampler_patch {tag}: max|adj| {np.abs(a).max():.3f} coins used {used}")
    np.savez_compressed(os.path.join(out, "sampler_patch.npz"), **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
    args = ap.parse_args()
    torch.manual_seed(0)
    DiffuseSG, NodeAdjPrecond, NodeAdjEDMSampler = _import_reference()
    gen_forward(DiffuseSG, args.out)
    gen_sampler(DiffuseSG, NodeAdjPrecond, NodeAdjEDMSampler, args.out)


if __name__ == "__main__":
    main()
