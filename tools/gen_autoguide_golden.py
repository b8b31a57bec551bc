#!/usr/bin/env python3
"""Generate tests/golden/autoguide.npz: autoguidance through the reference's own modules.

DEV-CONTAINER ONLY, like tools/gen_golden.py, whose import shim (the disclosed three-symbol `timm` stub) and replay helpers it reuses.

Two reference networks per pair (diffusesg_amd/synth.py: AUTOGUIDE_PAIRS), synthetic fan-in-scaled weights with seeds 0 (main) and 1
(guide), each inside the reference's NodeAdjPrecond.  `Composite` wraps the two into the one module that IS the feature's definition:
it draws one coin per call from the generator the reference draws from, forces that outcome on both wrapped calls, and returns
D~ = D_m + (s_b - 1)(D_m - D_g) in float32 torch operations.  The wrapped module then runs
  * through the reference's own NodeAdjEDMSampler.sample with replayed churn noise and coins: B = 3, ragged flags with a single-node
    graph, s = 2, T = 8 Heun with churn and T = 8 Euler ('<pair>_<run>_adj' / '_node', '_coins_used');
  * once per sigma of (80, 1.5, 0.002) and coin outcome, with a self-conditioning input ('<pair>_s<i>_coin<c>_adj' / '_node'), and for
    pair a also the two legs on their own ('a_s<i>_coin<c>_main_*', '_guide_*'), which the host test's restatement of the combine needs.
Stored next to the outputs: the inputs ('in/...'), so that the fixture can be read without the portable generator.

Usage:  python tools/gen_autoguide_golden.py [--out tests/golden]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gen_golden import _Replay, _import_reference, squeeze_like_ref, t   # noqa: E402
from diffusesg_amd import spec as S                                      # noqa: E402
from diffusesg_amd import synth as Y                                     # noqa: E402
from diffusesg_amd import weights as W                                   # noqa: E402


def build_ref_net(DiffuseSG, cfg, seed):
    """gen_golden.build_ref_net with the configuration's own head counts (the narrow guide has 2 and 4)"""
    net = DiffuseSG(img_size=cfg.max_node_num, in_chans=cfg.c_adj + 2 * cfg.c_node, patch_size=cfg.patch_size, embed_dim=cfg.embed_dim,
                    depths=list(cfg.depths), num_heads=list(cfg.num_heads), window_size=cfg.window_size, mlp_ratio=4., drop_rate=0.,
                    attn_drop_rate=0., drop_path_rate=0.0, self_condition=cfg.self_condition, symmetric_noise=False,
                    out_chans_adj=cfg.c_adj, out_chans_node=cfg.c_node)
    ref_sd, mine = net.state_dict(), W.synth_state_dict(cfg, seed)
    assert set(ref_sd.keys()) == set(mine.keys()), (set(ref_sd) ^ set(mine))
    for k, v in ref_sd.items():
        assert tuple(v.shape) == tuple(mine[k].shape), (k, v.shape, mine[k].shape)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in mine.items()}, strict=True)
    return net.eval()


class Composite(torch.nn.Module):
    """Two NodeAdjPrecond behind one call: one coin per call, forced on both; D~ = D_m + (s_b - 1)(D_m - D_g)."""

    def __init__(self, P, main, guide, scale, sigma_range=None):
        super().__init__()
        self.P, self.main, self.guide, self.scale, self.sigma_range = P, main, guide, float(scale), sigma_range
        self.last = None

    @staticmethod
    def round_sigma(sigma):
        return torch.as_tensor(sigma)

    def forward(self, adjs, nodes, node_flags, sigmas, self_cond_adjs=None, self_cond_nodes=None):
        draw = self.P.np.random.rand
        c = draw()                          # the call's one draw, in the reference's draw order
        self.P.np.random.rand = lambda: c   # ... and its outcome for both networks
        try:
            ma, mn = self.main(adjs, nodes, node_flags, sigmas, self_cond_adjs, self_cond_nodes)
            ga, gn = self.guide(adjs, nodes, node_flags, sigmas, self_cond_adjs, self_cond_nodes)
        finally:
            self.P.np.random.rand = draw
        sig = torch.as_tensor(sigmas, dtype=torch.float32).reshape(-1)
        sb = torch.full_like(sig, self.scale)
        if self.sigma_range is not None:
            lo, hi = self.sigma_range
            sb = torch.where((sig >= lo) & (sig <= hi), sb, torch.ones_like(sb))
        sm1 = sb - 1.0
        self.last = (ma, mn, ga, gn)
        return ma + sm1.view(-1, 1, 1, 1) * (ma - ga), mn + sm1.view(-1, 1, 1) * (mn - gn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
    args = ap.parse_args()
    torch.manual_seed(0)
    DiffuseSG, NodeAdjPrecond, NodeAdjEDMSampler = _import_reference()
    import model.precond.precond as P
    cfg = S.tiny_config()
    res = {}
    main_net = NodeAdjPrecond("edm", build_ref_net(DiffuseSG, cfg, Y.AUTOGUIDE_MAIN_SEED), True, symmetric_noise=False).eval()
    for pair in Y.AUTOGUIDE_PAIRS:
        gcfg = Y.autoguide_guide_config(pair)
        guide_net = NodeAdjPrecond("edm", build_ref_net(DiffuseSG, gcfg, Y.AUTOGUIDE_GUIDE_SEED), True, symmetric_noise=False).eval()
        comp = Composite(P, main_net, guide_net, Y.AUTOGUIDE_SCALE).eval()
        # the composite call at three noise levels, coin off and on
        for si in range(len(Y.PRECOND_SIGMAS)):
            sigma, flags, adj, node, sc_adj, sc_node = Y.autoguide_precond_case(si)
            sig = np.full((3,), sigma, np.float32)
            if pair == "a":
                res[f"in/pre{si}_adj"], res[f"in/pre{si}_node"], res[f"in/pre{si}_sc_adj"], res[f"in/pre{si}_sc_node"] = adj, node, sc_adj, sc_node
            for coin in (0, 1):
                real = P.np.random.rand
                P.np.random.rand = lambda: 0.25 if coin else 0.75
                try:
                    with torch.no_grad():
                        da, dn = comp(t(adj.copy()), t(node.copy()), t(flags), t(sig), t(sc_adj.copy()), t(sc_node.copy()))
                finally:
                    P.np.random.rand = real
                key = f"{pair}_s{si}_coin{coin}"
                res[key + "_adj"], res[key + "_node"] = da.numpy(), dn.numpy()
                if pair == "a":
                    for nm, v in zip(("main_adj", "main_node", "guide_adj", "guide_node"), comp.last):
                        res[f"{key}_{nm}"] = v.numpy()
        # trajectories through the reference's own sampler, noise and coins replayed
        for (tag, T, solver, churn) in Y.AUTOGUIDE_RUNS:
            flags, init_adj, init_node, noise_adj, noise_node, coin_vals = Y.autoguide_sampler_case(tag, T, solver)
            smp = NodeAdjEDMSampler(num_steps=T, solver=solver, S_churn=churn, clip_samples=True, clip_samples_min=-1.0, clip_samples_max=1.0,
                                    clip_samples_scope="x_0", dev="cpu", objective="edm", self_condition=True, symmetric_noise=False)
            noise = []
            for i in range(T):   # draw order inside one step: adjacency first, then nodes
                noise += [noise_adj[i], noise_node[i]]
            rn, rc = _Replay(noise), _Replay(coin_vals)
            real_rl, real_rand = torch.randn_like, P.np.random.rand
            torch.randn_like = lambda x, **kw: torch.from_numpy(rn.pop().reshape(tuple(x.shape)).copy()).to(x.dtype)
            P.np.random.rand = lambda: float(rc.pop())
            try:
                ia, inn = squeeze_like_ref(cfg, init_adj, init_node)
                adjs, nodes = smp.sample(comp, t(flags), init_adjs=t(ia.copy()), init_nodes=t(inn.copy()), flag_node_multi_channel=True,
                                         flag_adj_multi_channel=True, num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj)
            finally:
                torch.randn_like, P.np.random.rand = real_rl, real_rand
            res[f"{pair}_{tag}_adj"], res[f"{pair}_{tag}_node"], res[f"{pair}_{tag}_coins_used"] = adjs.numpy(), nodes.numpy(), np.array(rc.i)
            if pair == "a":
                res[f"in/{tag}_init_adj"], res[f"in/{tag}_init_node"] = init_adj, init_node
                res[f"in/{tag}_noise_adj"], res[f"in/{tag}_noise_node"], res[f"in/{tag}_coins"] = noise_adj, noise_node, (coin_vals < 0.5).astype(np.uint8)
            print(f"autoguide {pair} {tag}: max|adj| {np.abs(adjs.numpy()).max():.3f} coins used {rc.i}")
    res["in/flags"], res["scale"] = W.synth_flags(3, cfg.max_node_num, Y.AUTOGUIDE_VALID), np.float32(Y.AUTOGUIDE_SCALE)
    path = os.path.join(args.out, "autoguide.npz")
    np.savez_compressed(path, **res)
    print(f"autoguide.npz: {len(res)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
