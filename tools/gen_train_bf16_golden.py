#!/usr/bin/env python3
"""Generate tests/golden/train_bf16.npz: one training iteration of the reference's own modules with the arithmetic of the bf16
training mode (dsg_train_set_precision) emulated in-process, for tests/test_train_bf16.py.

DEV-CONTAINER ONLY, like tools/gen_golden.py, whose recipe for the `train_backward` cases this follows: the reference's modules under
the timm shim, the portable generator's weights, the objective's draws and the self-conditioning coin replayed, the trainer's IoU term
restated (iou_loss_weight = 1), single-threaded autograd.

Cases (diffusesg_amd/synth.py: TRAIN_BF16_CASES): `small_b8` (N = 16, depths (2, 1), window 4, B = 8: 2048 / 512 token rows, coin
fired) and `tiny_b8` (B = 8: 512 / 128 rows, coin not fired).  Per case three runs:
  (F)  plain fp32 autograd.
  (E)  the emulation: every nn.Linear named attn.qkv, attn.proj, mlp.fc1, mlp.fc2, downsample.reduction, upsample.pre_linear or
       upsample.post_linear whose call has >= 512 token rows and in / out features that are multiples of 32 runs through an
       autograd function whose forward (y = x W^T) and both backward products (dx = dy W, dW = dy^T x) round their two operands to bf16
       (`.to(torch.bfloat16)`: round to nearest even on the CPU), multiply in float64 and return float32; the bias is added in
       float32 and db = colsum(dy) is taken from the unrounded dy.  In `small_b8` both levels take it, in `tiny_b8` level 0 only.
  (E') (E) again with every noisy-input element multiplied by 1 + 2^-22 u, u = +-1 from the portable generator.
Stored per case: (E)'s loss and total gradient norm, per parameter its norm and strided sample (train_backward.npz's format, <= 256
elements), (F)'s loss, and per tensor e_bf16 = max |g_E - g_F| / max |g_F| and d_flip = max |g_E' - g_E| / max |g_E| over the stored
sample, plus `covered`: 1 for the weight tensors whose products took the emulated route.

d_flip measures how far the emulation moves when rounding decisions flip under last-bit input differences -- the one thing that
separates a correct kernel from the emulation beyond fp32 accumulation.  The test holds the library to 2e-4 + 4 d_flip per tensor and
asks fp32 mode to VIOLATE that on a covered weight; so this tool asserts, per case, that every covered weight tensor with
e_bf16 > 1e-3 has 2e-4 + 4 d_flip <= e_bf16 / 4, and that there is one.

WHAT WAS FOUND: the condition does NOT hold with these networks, and neither remedy brings it about.  The portable generator's
weights make both networks amplify last-bit differences (small_b8: e_bf16 7e-2 ... 4.7e-1, d_flip 1.5e-3 ... 1.3e-2; tiny_b8: e_bf16
4.9e-3 ... 9.9e-3, d_flip 7e-4 ... 3e-3).  At B = 8 with 2^-22: small_b8 26 of 27 covered weights satisfy it
(down_layers.1.blocks.0.mlp.fc2 does not), tiny_b8 none of 9.  B = 16 and a 2^-23 perturbation, each and together: the same counts
(26 of 27, 0 of 9).  So the fixture is written at B = 8 / 2^-22 as specified, the table is printed, and the tool then exits with
the assertion failing -- the condition is kept as stated, not weakened.  The GPU test's own power check (fp32 mode outside
2e-4 + 4 d_flip on at least one covered weight per case) holds all the same: 27 of 27 and 5 of 9 covered weights
(profiles/train_lp_kernel_errors.md).

Usage:  python tools/gen_train_bf16_golden.py [--out tests/golden]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G   # noqa: E402

Y = G.Y
COVERED_SUFFIXES = (".attn.qkv", ".attn.proj", ".mlp.fc1", ".mlp.fc2", ".downsample.reduction", ".upsample.pre_linear", ".upsample.post_linear")


def _r(x):
    return x.to(torch.bfloat16).to(torch.float64)


class _LpLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        x2 = x.reshape(-1, x.shape[-1])
        y = (_r(x2) @ _r(w).t()).to(torch.float32)
        if b is not None:
            y = y + b
        return y.reshape(x.shape[:-1] + (w.shape[0],))

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        x2, dy2 = x.reshape(-1, x.shape[-1]), dy.reshape(-1, dy.shape[-1])
        dx = (_r(dy2) @ _r(w)).to(torch.float32).reshape(x.shape)
        dw = (_r(dy2).t() @ _r(x2)).to(torch.float32)
        db = dy2.sum(0) if ctx.has_bias else None
        return dx, dw, db


def emulate_covered(net, taken):
    """replace the forward of every covered nn.Linear of `net`; `taken`: set filled with the weight names whose calls took the route"""
    for name, mod in net.named_modules():
        if not isinstance(mod, torch.nn.Linear) or not name.endswith(COVERED_SUFFIXES):
            continue

        def fwd(x, mod=mod, name=name):
            rows = x.numel() // x.shape[-1]
            if rows >= 512 and mod.in_features % 32 == 0 and mod.out_features % 32 == 0:
                taken.add(name + ".weight")
                return _LpLinear.apply(x, mod.weight, mod.bias)
            return torch.nn.functional.linear(x, mod.weight, mod.bias)
        mod.forward = fwd


def run_case(DiffuseSG, NodeAdjPrecond, name, emulate, flip):
    """one training iteration up to loss.backward() -> (loss, total norm, {parameter: unclipped gradient (flat)}, taken)"""
    import model.precond.precond as P
    from loss.rainbow_loss import NodeAdjRainbowLoss
    from runner.objectives.edm import NodeAdjEDMObjectiveGenerator
    cfg, flags, clean_adj, clean_node, rnd, eps_adj, eps_node, coin, (u_adj, u_node) = Y.train_bf16_case(name)
    net = G.build_ref_net(DiffuseSG, cfg)
    taken = set()
    if emulate:
        emulate_covered(net, taken)
    model = NodeAdjPrecond("edm", net, cfg.self_condition, symmetric_noise=False)
    model.train()
    gen = NodeAdjEDMObjectiveGenerator(precond="edm", sigma_dist="edm", other_params=None, dev="cpu", symmetric_noise=False)
    draws = G._Replay([rnd, eps_adj, eps_node])
    t = G.t

    def fake_randn(*size, **kw):
        return torch.from_numpy(np.ascontiguousarray(draws.pop()).copy())

    def fake_randn_like(x, **kw):
        return torch.from_numpy(np.ascontiguousarray(draws.pop()).reshape(tuple(x.shape)).copy()).to(x.dtype)
    real_r, real_rl, real_rand = torch.randn, torch.randn_like, P.np.random.rand
    torch.randn, torch.randn_like = fake_randn, fake_randn_like
    P.np.random.rand = lambda: coin
    try:
        adjs_gt, nodes_gt, node_flags = t(clean_adj.copy()), t(clean_node.copy()), t(flags)
        net_input_a, net_input_x, net_cond, net_target_a, net_target_x, (c_skip, c_out, c_in, c_noise, sigmas, weights) = \
            gen.get_input_output(adjs_gt, nodes_gt, node_flags)
        if flip:
            net_input_a = net_input_a * (1.0 + 2.0 ** -22 * t(u_adj).reshape(net_input_a.shape))
            net_input_x = net_input_x * (1.0 + 2.0 ** -22 * t(u_node).reshape(net_input_x.shape))
        net_output_a, net_output_x = model(adjs=net_input_a, nodes=net_input_x, node_flags=node_flags, sigmas=sigmas)
    finally:
        torch.randn, torch.randn_like, P.np.random.rand = real_r, real_rl, real_rand
    loss_func = NodeAdjRainbowLoss(edge_loss_weight=1.0, node_loss_weight=1.0, flag_reweight=False, objective="edm")
    reg_loss_adj, reg_loss_node = loss_func(net_pred_a=net_output_a, net_pred_x=net_output_x, net_target_a=net_target_a,
                                            net_target_x=net_target_x, net_cond=net_cond, adjs_perturbed=net_input_a,
                                            adjs_gt=adjs_gt, x_perturbed=net_input_x, x_gt=nodes_gt, node_flags=node_flags,
                                            loss_weight=weights, reduction='none')

    def box_convert_cxcywh_xyxy(b):
        cx, cy, w, h = b.unbind(-1)
        return torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], dim=-1)

    def box_iou_diag(a, b):
        area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
        area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        lt, rb = torch.max(a[:, :2], b[:, :2]), torch.min(a[:, 2:], b[:, 2:])
        wh = (rb - lt).clamp(min=0)
        inter = wh[:, 0] * wh[:, 1]
        return inter / (area_a + area_b - inter)
    ob = box_convert_cxcywh_xyxy((net_output_x[..., -4:] + 1.0) / 2.0).clamp(min=0.0, max=1.0)
    tb = box_convert_cxcywh_xyxy((net_target_x[..., -4:] + 1.0) / 2.0).clamp(min=0.0, max=1.0)
    node_iou_loss = -(box_iou_diag(ob.view(-1, 4), tb.view(-1, 4)).view(-1)) ** 2.0
    node_flags_t = node_flags.view(-1)
    node_iou_loss = (node_iou_loss * node_flags_t.to(torch.float32)).view(-1, node_flags.shape[1])
    node_iou_loss = node_iou_loss.sum(dim=-1) / node_flags_t.sum(dim=-1).to(torch.float32)
    reg_loss_node = reg_loss_node + 1.0 * node_iou_loss * weights
    loss = reg_loss_adj.mean() + reg_loss_node.mean()
    torch.set_num_threads(1)   # bit-stable accumulation order of autograd (see gen_golden.gen_train_backward)
    loss.backward()
    torch.set_num_threads(8)
    grads = {k: p_.grad.detach().numpy().reshape(-1).copy() for k, p_ in model.named_parameters()}
    total = float(np.sqrt(sum((g_.astype(np.float64) ** 2).sum() for g_ in grads.values())))
    return float(loss.detach()), total, grads, {"model." + k for k in taken}, coin


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(G.REPO, "tests", "golden"))
    args = ap.parse_args()
    torch.set_num_threads(8)
    DiffuseSG, NodeAdjPrecond, _ = G._import_reference()
    res, failed = {}, []
    for name in Y.TRAIN_BF16_CASES:
        loss_f, _, g_f, _, coin = run_case(DiffuseSG, NodeAdjPrecond, name, False, False)
        loss_e, total_e, g_e, taken, _ = run_case(DiffuseSG, NodeAdjPrecond, name, True, False)
        _, _, g_p, taken_p, _ = run_case(DiffuseSG, NodeAdjPrecond, name, True, True)
        assert taken == taken_p and taken
        names, norms, e_bf16, d_flip, covered = [], [], [], [], []
        for k in g_e:
            stride = max(1, -(-g_e[k].size // Y.TRAIN_BF16_MAX_SAMPLE))
            se, sf, sp = g_e[k][::stride], g_f[k][::stride], g_p[k][::stride]
            res[f"{name}_gparam/{k}"] = se.copy()
            names.append(k); norms.append(float(np.sqrt((g_e[k].astype(np.float64) ** 2).sum())))
            e_bf16.append(float(np.abs(se - sf).max()) / max(float(np.abs(sf).max()), 1e-30))
            d_flip.append(float(np.abs(sp - se).max()) / max(float(np.abs(se).max()), 1e-30))
            covered.append(int(k in taken))
        res[f"{name}_loss"], res[f"{name}_loss_f32"] = np.array(loss_e), np.array(loss_f)
        res[f"{name}_coin"], res[f"{name}_total_grad_norm"] = np.array(coin), np.array(total_e)
        res[f"{name}_gparam_names"], res[f"{name}_gparam_norms"] = np.array(names), np.array(norms)
        res[f"{name}_e_bf16"], res[f"{name}_d_flip"], res[f"{name}_covered"] = np.array(e_bf16), np.array(d_flip), np.array(covered)
        # the condition that keeps the power check of tests/test_train_bf16.py from being vacuous (asserted below, once the file is
        # written: the figures stay inspectable where it does not hold)
        strong = [i for i in range(len(names)) if covered[i] and e_bf16[i] > 1e-3]
        if not strong:
            failed.append(f"{name}: no covered weight tensor moves by more than 1e-3 under the emulation")
        failed += [f"{name} {names[i]}: 2e-4 + 4 d_flip = {2e-4 + 4 * d_flip[i]:.2e} > e_bf16 / 4 = {e_bf16[i] / 4:.2e}"
                   for i in strong if not 2e-4 + 4 * d_flip[i] <= e_bf16[i] / 4]
        cov = [i for i in range(len(names)) if covered[i]]
        print(f"train bf16 {name}: loss E {loss_e:.6f} (F {loss_f:.6f}), |grad| {total_e:.5f}, {len(cov)} covered weights of {len(names)} tensors, "
              f"{len(strong)} with e_bf16 > 1e-3; covered e_bf16 {min(e_bf16[i] for i in cov):.2e} .. {max(e_bf16[i] for i in cov):.2e}, "
              f"d_flip max {max(d_flip):.2e} (covered {max(d_flip[i] for i in cov):.2e})")
    np.savez_compressed(os.path.join(args.out, "train_bf16.npz"), **res)
    assert not failed, "every covered weight tensor with e_bf16 > 1e-3 must have 2e-4 + 4 d_flip <= e_bf16 / 4:\n  " + "\n  ".join(failed)


if __name__ == "__main__":
    main()
