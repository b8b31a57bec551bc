#!/usr/bin/env python3
"""Write tests/golden/train_patch.npz: the reference's own modules at patch_size 2 and 4 under its autograd -- training iterations,
input gradients and one probability-flow ODE run -- for tests/test_patch_train.py (GPU) and tests/test_patch_train_host.py (CPU).

DEVELOPMENT MACHINES ONLY, like tools/gen_golden.py, whose helpers import the reference (portable generator's weights, `timm` shim);
nothing at test time reads the reference.  The file holds data only.

Training cases (diffusesg_amd/synth.py: PATCH_TRAIN_CASES, B = 4), gen_golden.gen_train_backward's recipe and storage format: the
objective's draws and the self-conditioning coin replayed, the trainer's IoU term restated (iou_loss_weight = 1; 0 for `nosc_p2`, whose
one node channel leaves no box channels), autograd on one thread; per case the loss, the preconditioned outputs, the total gradient
norm clip_grad_norm_ reports, per parameter its L2 norm and every stride-th element (<= 256).  For PATCH_TRAIN_ADAM_CASE also the
parameters after torch.optim.Adam(lr 2e-4).step() on the clipped gradients, and -- for the CPU test of the composed edges -- the whole
gradients of PATCH_TRAIN_EDGE_PARAMS with the activations around them: PatchEmbed's assembled input image and the gradient at its
convolution's output, read_out.0's input and the gradient at its output.

Input-gradient cases (PATCH_INPUT_GRAD_CASES), tools/gen_input_grad_golden.py's recipe: NodeAdjPrecond.forward with the noisy inputs
requiring grad, the coin pinned to "does not fire"; D, loss, grad_adj, grad_node; for PATCH_INPUT_GRAD_EDGE_CASE also the gradient at
PatchEmbed's convolution output.

ODE case (patch_ode_case), tools/gen_ode_golden.py's recipe and classes: float64 autograd, no self-conditioning, a recorded probe, and
the discrepancy of the reference's own float32 run against it, from which the test's bars are formed.

Usage:  python tools/gen_patch_train_golden.py [--out tests/golden]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G                       # noqa: E402
import gen_ode_golden as O                   # noqa: E402
from diffusesg_amd import guide              # noqa: E402
from diffusesg_amd import lib                # noqa: E402
from diffusesg_amd import ode                # noqa: E402

Y = G.Y


def _box_convert_cxcywh_xyxy(b):
    cx, cy, w, h = b.unbind(-1)
    return torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], dim=-1)


def _box_iou_diag(a, b):
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    lt, rb = torch.max(a[:, :2], b[:, :2]), torch.min(a[:, 2:], b[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[:, 0] * wh[:, 1]
    return inter / (area_a + area_b - inter)


class _EdgeTaps:
    """the tensors around PatchEmbed's convolution and read_out.0 of the LAST (differentiated) call of the network"""

    def __init__(self, net):
        self.t = {}
        self.hooks = [net.patch_embed.proj.register_forward_hook(self._keep("pe")), net.read_out[0].register_forward_hook(self._keep("ro0"))]

    def _keep(self, tag):
        def hook(mod, inp, outp):
            if outp.requires_grad:
                outp.retain_grad()
                self.t[tag + "_in"], self.t[tag + "_out"] = inp[0], outp
        return hook

    def remove(self):
        for h in self.hooks:
            h.remove()


def gen_train(DiffuseSG, NodeAdjPrecond, res):
    import model.precond.precond as P
    from loss.rainbow_loss import NodeAdjRainbowLoss
    from runner.objectives.edm import NodeAdjEDMObjectiveGenerator
    t = G.t
    for case in Y.PATCH_TRAIN_CASES:
        cfg, flags, clean_adj, clean_node, rnd, eps_adj, eps_node, coin = Y.patch_train_case(case)
        net = G.build_ref_net(DiffuseSG, cfg)
        model = NodeAdjPrecond("edm", net, cfg.self_condition, symmetric_noise=False)
        model.train()
        gen = NodeAdjEDMObjectiveGenerator(precond="edm", sigma_dist="edm", other_params=None, dev="cpu", symmetric_noise=False)
        draws = G._Replay([rnd, eps_adj, eps_node])

        def fake_randn(*size, **kw):
            return torch.from_numpy(np.ascontiguousarray(draws.pop()).copy())

        def fake_randn_like(x, **kw):
            return torch.from_numpy(np.ascontiguousarray(draws.pop()).reshape(tuple(x.shape)).copy()).to(x.dtype)
        taps = _EdgeTaps(net)
        real_r, real_rl, real_rand = torch.randn, torch.randn_like, P.np.random.rand
        torch.randn, torch.randn_like = fake_randn, fake_randn_like
        P.np.random.rand = lambda: coin
        try:
            ca, cn = G.squeeze_like_ref(cfg, clean_adj.copy(), clean_node.copy())
            adjs_gt, nodes_gt, node_flags = t(ca), t(cn), t(flags)
            net_input_a, net_input_x, net_cond, net_target_a, net_target_x, (c_skip, c_out, c_in, c_noise, sigmas, weights) = \
                gen.get_input_output(adjs_gt, nodes_gt, node_flags)
            optimizer = torch.optim.Adam(model.parameters(), lr=2.0e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
            optimizer.zero_grad(set_to_none=True)
            net_output_a, net_output_x = model(adjs=net_input_a, nodes=net_input_x, node_flags=node_flags, sigmas=sigmas)
        finally:
            torch.randn, torch.randn_like, P.np.random.rand = real_r, real_rl, real_rand
            taps.remove()
        loss_func = NodeAdjRainbowLoss(edge_loss_weight=1.0, node_loss_weight=1.0, flag_reweight=False, objective="edm")
        reg_loss_adj, reg_loss_node = loss_func(net_pred_a=net_output_a, net_pred_x=net_output_x, net_target_a=net_target_a,
                                                net_target_x=net_target_x, net_cond=net_cond, adjs_perturbed=net_input_a,
                                                adjs_gt=adjs_gt, x_perturbed=net_input_x, x_gt=nodes_gt, node_flags=node_flags,
                                                loss_weight=weights, reduction='none')
        iou_loss_weight = 1.0 if cfg.c_node >= 4 else 0.0
        if iou_loss_weight:
            ob = _box_convert_cxcywh_xyxy((net_output_x[..., -4:] + 1.0) / 2.0).clamp(min=0.0, max=1.0)
            tb = _box_convert_cxcywh_xyxy((net_target_x[..., -4:] + 1.0) / 2.0).clamp(min=0.0, max=1.0)
            node_iou_loss = -(_box_iou_diag(ob.view(-1, 4), tb.view(-1, 4)).view(-1)) ** 2.0
            node_flags_t = node_flags.view(-1)
            node_iou_loss = (node_iou_loss * node_flags_t.to(torch.float32)).view(-1, node_flags.shape[1])
            node_iou_loss = node_iou_loss.sum(dim=-1) / node_flags_t.sum(dim=-1).to(torch.float32)
            reg_loss_node = reg_loss_node + iou_loss_weight * node_iou_loss * weights
        loss = reg_loss_adj.mean() + reg_loss_node.mean()
        torch.set_num_threads(1)   # autograd's index_add / scatter accumulations are order-dependent across threads
        loss.backward()
        torch.set_num_threads(8)
        total_norm = torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=10.0, norm_type=2)   # the norm BEFORE clipping
        res[f"{case}_loss"], res[f"{case}_coin"] = np.array(float(loss.detach())), np.array(coin)
        res[f"{case}_iou_loss_weight"] = np.array(iou_loss_weight)
        res[f"{case}_total_grad_norm"] = np.array(float(total_norm))
        res[f"{case}_pred_adj"], res[f"{case}_pred_node"] = net_output_a.detach().numpy().copy(), net_output_x.detach().numpy().copy()
        scale = min(1.0, 10.0 / (float(total_norm) + 1e-6))
        names, norms = [], []
        for k, p_ in model.named_parameters():
            assert p_.grad is not None, k
            g_ = (p_.grad / scale).numpy().reshape(-1)
            stride = max(1, -(-g_.size // Y.PATCH_TRAIN_MAX_SAMPLE))
            res[f"{case}_gparam/{k}"] = g_[::stride].copy()
            names.append(k); norms.append(float(np.sqrt((g_.astype(np.float64) ** 2).sum())))
            if case == Y.PATCH_TRAIN_ADAM_CASE and k[len("model."):] in Y.PATCH_TRAIN_EDGE_PARAMS:
                res[f"{case}_gfull/{k}"] = g_.reshape(tuple(p_.shape)).copy()
        res[f"{case}_gparam_names"], res[f"{case}_gparam_norms"] = np.array(names), np.array(norms)
        if case == Y.PATCH_TRAIN_ADAM_CASE:
            for tag in ("pe", "ro0"):
                res[f"{case}_{tag}_in"] = taps.t[tag + "_in"].detach().numpy().copy()
                res[f"{case}_{tag}_dout"] = taps.t[tag + "_out"].grad.numpy().copy()   # (activation gradients are not clipped)
            optimizer.step()   # on the clipped gradients (trainer_node_adj.py:170-171)
            for k, p_ in model.named_parameters():
                v_ = p_.detach().numpy().reshape(-1)
                res[f"{case}_param_after/{k}"] = v_[::max(1, -(-v_.size // 256))].copy()
        print(f"train patch {case}: loss {float(loss.detach()):.6f}, |grad| {float(total_norm):.5f} over {len(names)} tensors, coin {coin:.1f}, "
              f"iou weight {iou_loss_weight}", flush=True)


def gen_input_grad(DiffuseSG, NodeAdjPrecond, res):
    import model.precond.precond as P
    torch.set_num_threads(1)
    nets = {}
    for tag, (name, valid, _sig, _sc, cot) in Y.PATCH_INPUT_GRAD_CASES.items():
        cfg, flags, adj, node, sig, sc_adj, sc_node, g_adj, g_node = Y.patch_input_grad_case(tag)
        if name not in nets:
            nets[name] = G.build_ref_net(DiffuseSG, cfg)
        pre = NodeAdjPrecond("edm", nets[name], cfg.self_condition, symmetric_noise=False).eval()
        a_in, n_in = G.squeeze_like_ref(cfg, adj, node)
        a_t, n_t = G.t(a_in.copy()).requires_grad_(True), G.t(n_in.copy()).requires_grad_(True)
        sa = sn = None
        if sc_adj is not None:
            sa, sn = (G.t(v.copy()) for v in G.squeeze_like_ref(cfg, sc_adj, sc_node))
        taps = _EdgeTaps(nets[name])
        real = np.random.rand
        P.np.random.rand = lambda: 0.9   # the coin does not fire
        try:
            Da, Dn = pre(a_t, n_t, G.t(flags), G.t(sig), sa, sn)
        finally:
            P.np.random.rand = real
            taps.remove()
        if cot == "overlap":
            loss = guide.box_overlap_loss()(Da, Dn)
        else:
            ga, gn = G.squeeze_like_ref(cfg, g_adj, g_node)
            loss = (G.t(ga) * Da).sum() + (G.t(gn) * Dn).sum()
        loss.backward()
        res[f"igrad/{tag}/D_adj"], res[f"igrad/{tag}/D_node"] = Da.detach().numpy(), Dn.detach().numpy()
        res[f"igrad/{tag}/grad_adj"], res[f"igrad/{tag}/grad_node"] = a_t.grad.numpy(), n_t.grad.numpy()
        res[f"igrad/{tag}/loss"] = np.float64(loss.item())
        if tag == Y.PATCH_INPUT_GRAD_EDGE_CASE:
            res[f"igrad/{tag}/pe_dout"] = taps.t["pe_out"].grad.numpy().copy()
        print(f"input grad patch {tag}: max|D_adj| {np.abs(Da.detach().numpy()).max():.3f} max|grad_adj| {np.abs(a_t.grad.numpy()).max():.3e} "
              f"max|grad_node| {np.abs(n_t.grad.numpy()).max():.3e}", flush=True)
    torch.set_num_threads(8)


def gen_ode(DiffuseSG, NodeAdjPrecond, res):
    import model.precond.precond as P
    torch.set_num_threads(1)
    cfg, flags, adj, node, p_adj, p_node = Y.patch_ode_case()
    T, solver = Y.PATCH_ODE_RUN
    dims = ode.graph_dims(flags, cfg.c_adj, cfg.c_node)
    refs = {torch.float64: O.Ref(G.build_ref_net(DiffuseSG, cfg).double(), cfg, flags, torch.float64),
            torch.float32: O.RefPrecond32(G.build_ref_net(DiffuseSG, cfg), cfg, flags, NodeAdjPrecond, P)}
    scfg = lib.make_sampler_cfg(T, solver, S_churn=0.0)
    _t_eval, w = lib.ode_evals(scfg, lib.make_ode_cfg("encode", "rademacher"))
    _, lv, _, _ = lib.sigma_schedule(scfg)
    out = {}
    for dt, R in refs.items():
        c = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dt)
        la, ln, tr = R.run(c(adj), c(node), T, solver, "encode", c(p_adj), c(p_node))
        x2 = (la.double().reshape(R.B, -1) ** 2).sum(1) + (ln.double().reshape(R.B, -1) ** 2).sum(1)
        logp, _ = ode.assemble_logp(x2.numpy(), tr.double().numpy(), w, dims, float(lv[0]), float(lv[-1]))
        out[dt] = dict(la=la.double().numpy(), ln=ln.double().numpy(), n=tr.double().numpy(), logp=logp)
    r64, r32 = out[torch.float64], out[torch.float32]
    lat64 = np.concatenate([r64["la"].reshape(-1), r64["ln"].reshape(-1)])
    lat32 = np.concatenate([r32["la"].reshape(-1), r32["ln"].reshape(-1)])
    live = dims > 0
    res["ode/latent_adj"], res["ode/latent_node"], res["ode/n"], res["ode/logp"] = r64["la"], r64["ln"], r64["n"], r64["logp"]
    res["ode/worst_latent"] = np.float64(np.abs(lat32 - lat64).max() / np.abs(lat64).max())
    res["ode/worst_n"] = np.float64(np.abs(r32["n"] - r64["n"]).max() / np.abs(r64["n"]).max())
    res["ode/worst_logp"] = np.float64((np.abs(r32["logp"] - r64["logp"])[live] / np.abs(r64["logp"])[live]).max())
    print(f"ode patch: logp {r64['logp']} | f32 - f64: latent {res['ode/worst_latent']:.2e} n {res['ode/worst_n']:.2e} logp {res['ode/worst_logp']:.2e}",
          flush=True)
    torch.set_num_threads(8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(G.REPO, "tests", "golden"))
    args = ap.parse_args()
    torch.set_num_threads(8)
    DiffuseSG, NodeAdjPrecond, _ = G._import_reference()
    res = {}
    gen_train(DiffuseSG, NodeAdjPrecond, res)
    gen_input_grad(DiffuseSG, NodeAdjPrecond, res)
    gen_ode(DiffuseSG, NodeAdjPrecond, res)
    path = os.path.join(args.out, "train_patch.npz")
    np.savez_compressed(path, **res)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
