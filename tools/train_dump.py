"""dev helper: A/B of the training-form entries between two builds of libdsg.so (a refactor of dsg_api.cpp must not move a value).
  train_dump.py [--lib PATH] OUT          run every case below on the library at PATH (default: the tree's) and write OUT/<case>.npz
  train_dump.py --compare A B [A2]        per array `identical` or the differing count; exit 1 on any difference, except that the
        gradients of attn.relative_position_bias_table (float atomics in no fixed order) may differ by d <= 8 * max(d_plain, 2^-20) of
        the tensor's maximum, d_plain = the difference between A and a second run A2 of the same library (0 without A2)
  train_dump.py [--lib PATH] --host-time  median host time of one dsg_train_step_grads call (vg, B = 2; no synchronise while timed)
Synthetic weights (weights.synth_state_dict(cfg, 0)), seeded inputs (synth.train_case / input_grad_case); nothing from the reference.
Besides the entries the tests run, the cases cover dsg_train_grads (a given dL/dF) and a net of 32 blocks, which takes the un-grouped
affine path (more blocks than one grouped launch holds): no test and no Python caller reaches either."""
import ctypes as C
import dataclasses
import glob
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
TABLE = "relative_position_bias_table"


def compare(a_dir, b_dir, a2_dir=None):
    bad = 0
    for fa in sorted(glob.glob(os.path.join(a_dir, "*.npz"))):
        case = os.path.basename(fa)
        a, b = np.load(fa), np.load(os.path.join(b_dir, case))
        a2 = np.load(os.path.join(a2_dir, case)) if a2_dir else None
        assert sorted(a.files) == sorted(b.files), f"{case}: different arrays"
        for k in a.files:
            nd = int((a[k] != b[k]).sum()) if a[k].shape == b[k].shape else -1
            if nd == 0:
                verdict = "identical"
            elif nd > 0 and k.endswith(TABLE):
                s = max(float(np.abs(a[k]).max()), 1e-30)
                d = float(np.abs(a[k] - b[k]).max()) / s
                d_plain = float(np.abs(a[k] - a2[k]).max()) / s if a2 is not None else 0.0
                fits = d <= 8 * max(d_plain, 2.0 ** -20)
                verdict = f"{nd} differ, d {d:.2e} (d_plain {d_plain:.2e}): {'within' if fits else 'BEYOND'} the atomics' rule"
                bad += 0 if fits else 1
            else:
                verdict = f"DIFFERENT: {nd} of {a[k].size} elements"
                bad += 1
            print(f"{case[:-4]:28s} {k:60s} {verdict}")
    print("A/B:", "no difference beyond the order of the bias tables' atomics" if not bad else f"{bad} arrays differ")
    return 1 if bad else 0


def main(argv):
    if argv and argv[0] == "--compare":
        return compare(*argv[1:4])
    from diffusesg_amd import lib
    if argv and argv[0] == "--lib":
        lib.load(argv[1])
        argv = argv[2:]
    import torch
    from diffusesg_amd import synth as Y, weights as W, train as TR
    from diffusesg_amd.model import build_network
    T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    host = lambda d: {k: v.detach().cpu().numpy() for k, v in d.items() if v is not None}
    gen = TR.NodeAdjEDMObjectiveGeneratorHip(precond="edm", sigma_dist="edm", other_params=None, dev="cuda", symmetric_noise=False)
    lf = TR.NodeAdjRainbowLossHip(edge_loss_weight=1.0, node_loss_weight=1.0, flag_reweight=False, objective="edm")
    nets = {}

    def net_of(name, cfg=None):
        if name not in nets:
            cfg = cfg or Y.CONFIGS[name]()
            nets[name] = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")
        return nets[name]

    def step(net, name, B, coin=None, want_grads=True):
        """one train_step_grads call on the seeded case -> D, both losses and every parameter gradient"""
        if name == "nosc":   # one node channel: no bbox channels for train_case to fill, so the input-gradient case's noisy graphs (B = 2)
            _cfg, flags, adj, node, sig, _sa, _sx, _ga, _gn, _stride = Y.input_grad_case("nosc")
            na, nx, ta, tx, sigmas, weights, case_coin, iou_w = T(adj), T(node), T(np.sign(adj)), T(np.sign(node)), T(sig), None, 0.9, 0.0
        else:
            _cfg, flags, ca, cn, rnd, ea, en, case_coin = Y.train_case(name, B=B)
            na, nx, _c, ta, tx, (_cs, _co, _ci, _cn, sigmas, weights) = gen.get_input_output(T(ca), T(cn), T(flags), rnd_sigma=T(rnd), noise=(T(ea), T(en)))
            iou_w = 1.0
        real, np.random.rand = np.random.rand, (lambda *a: case_coin if coin is None else coin)
        try:
            oa, on, la, ln, grads = TR.train_step_grads(net, lf, na, nx, T(flags), sigmas, ta, tx, weights, iou_loss_weight=iou_w,
                                                        iou_loss_type="giou", want_grads=want_grads)
        finally:
            np.random.rand = real
        return host(dict(D_adj=oa, D_node=on, loss_adj=la, loss_node=ln, **{"g/" + k: v for k, v in grads.items()}))

    def vjp(net, tag, callback):
        _cfg, flags, adj, node, sig, sa, sx, ga, gn, _stride = Y.input_grad_case(tag)
        ga, gn = T(ga), T(gn)
        kw = dict(loss_fn=lambda Da, Dn: (Da * ga.reshape(Da.shape)).sum() + (Dn * gn.reshape(Dn.shape)).sum()) if callback else dict(grad_outputs=(ga, gn))
        Da, Dn, _loss, g_adj, g_node = net.value_and_input_grad(T(adj), T(node), T(flags), T(sig), self_cond_adjs=T(sa), self_cond_nodes=T(sx), coin=False, **kw)
        return host(dict(D_adj=Da, D_node=Dn, grad_adj=g_adj, grad_node=g_node))

    def given_dF(net, name, B, backward):
        """dsg_train_grads through ctypes: F of seeded inputs and, with `backward`, every parameter gradient for a seeded dL/dF"""
        cfg, flags, ca, cn, rnd, _ea, _en, _coin = Y.train_case(name, B=B)
        m = net.model
        h = TR._train_handle(m)
        n = cfg.max_node_num
        ia, ix, c_noise, fl = T(ca), T(cn), T((0.25 * rnd).astype(np.float32)), T(flags)
        dFa, dFn = T(W.normal(5, "dump/dF_adj", (B, cfg.c_adj, n, n))), T(W.normal(5, "dump/dF_node", (B, n, cfg.c_node)))
        Fa, Fn = torch.empty_like(ia), torch.empty_like(ix)
        keys, offs, shapes, total = TR._flat_layout(m)
        flat = torch.zeros(total, device="cuda")
        names = (C.c_char_p * len(keys))(*[k.encode() for k in keys])
        ptrs = (C.c_void_p * len(keys))(*[flat.data_ptr() + 4 * o for o in offs])
        p = lambda t: C.c_void_p(t.data_ptr())
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if backward:
            rc = h.L.dsg_train_grads(h.raw, B, p(ia), p(ix), p(fl), p(c_noise), None, None, p(dFa), p(dFn), p(Fa), p(Fn), len(keys), names, ptrs, st)
        else:
            rc = h.L.dsg_train_grads(h.raw, B, p(ia), p(ix), p(fl), p(c_noise), None, None, None, None, p(Fa), p(Fn), 0, None, None, st)
        h.check(rc, "dsg_train_grads")
        out = dict(F_adj=Fa, F_node=Fn)
        if backward:
            out.update({"g/" + k: flat[o:o + int(np.prod(s))] for k, o, s in zip(keys, offs, shapes)})
        return host(out)

    def self_cond(net, name, B):
        _cfg, flags, ca, cn, rnd, ea, en, _coin = Y.train_case(name, B=B)
        na, nx, _c, _ta, _tx, (_cs, _co, _ci, _cn, sigmas, _w) = gen.get_input_output(T(ca), T(cn), T(flags), rnd_sigma=T(rnd), noise=(T(ea), T(en)))
        m = net.model
        h = TR._train_handle(m)
        _B, a, x, fl, _, _ = m._canon(na, nx, T(flags), None, None)
        sa, sx = torch.empty_like(a), torch.empty_like(x)
        sg = torch.as_tensor(sigmas).to(device="cuda", dtype=torch.float32).reshape(-1).expand(B).contiguous()
        p = lambda t: C.c_void_p(t.data_ptr())
        h.check(h.L.dsg_train_self_cond(h.raw, B, p(a), p(x), p(fl), p(sg), p(sa), p(sx),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)), "dsg_train_self_cond")
        return host(dict(sc_adj=sa, sc_node=sx))

    def block(net, name, prefix, B):
        x, emb, dy = Y.block_case(Y.CONFIGS[name](), prefix, B)
        x_out, gx, ge, grads = TR.swin_block_train(net.model, prefix, T(x), T(emb), T(dy))
        x_fwd, _, _, _ = TR.swin_block_train(net.model, prefix, T(x), T(emb))
        return host(dict(x_out=x_out, x_out_forward_only=x_fwd, grad_x=gx, grad_emb=ge, **{"g/" + k: v for k, v in grads.items()}))

    if argv and argv[0] == "--host-time":
        net = net_of("vg")
        _cfg, flags, ca, cn, rnd, ea, en, _coin = Y.train_case("vg", B=2)
        na, nx, _c, ta, tx, (_cs, _co, _ci, _cn, sigmas, weights) = gen.get_input_output(T(ca), T(cn), T(flags), rnd_sigma=T(rnd), noise=(T(ea), T(en)))
        np.random.rand = lambda *a: 0.9
        call = lambda: TR.train_step_grads(net, lf, na, nx, T(flags), sigmas, ta, tx, weights, iou_loss_weight=1.0, iou_loss_type="giou")
        ts = []
        for it in range(220):
            t0 = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t0)
            torch.cuda.synchronize()   # outside the timed region: an empty queue, so that the call never waits for the GPU
        print(f"host time of train_step_grads (vg, B=2), 200 calls after 20: median {1e3 * np.median(ts[20:]):.3f} ms, min {1e3 * min(ts[20:]):.3f} ms")
        return 0

    out_dir = argv[0]
    os.makedirs(out_dir, exist_ok=True)
    big = dataclasses.replace(Y.CONFIGS["tiny"](), depths=(15, 1))   # 32 blocks: the un-grouped affine path
    cases = [(f"step_{n}_B{B}_coin{c}", lambda n=n, B=B, c=c: step(net_of(n), n, B, c))
             for n, B, c in (("tiny", 4, 0.9), ("tiny", 4, 0.1), ("small", 2, None), ("nosc", 2, None), ("vg", 2, None), ("coco", 1, None))]
    cases += [("step_tiny_no_grads", lambda: step(net_of("tiny"), "tiny", 4, 0.9, want_grads=False)),
              ("self_cond_tiny", lambda: self_cond(net_of("tiny"), "tiny", 4))]
    cases += [(f"vjp_{tag}_{'callback' if cb else 'given'}", lambda tag=tag, cb=cb: vjp(net_of(Y.INPUT_GRAD_CASES[tag][0]), tag, cb))
              for tag in ("tiny_sc", "small", "nosc") for cb in (True, False)]
    cases += [("block_small", lambda: block(net_of("small"), "small", "down_layers.0.blocks.1", 2)),
              ("train_grads_tiny", lambda: given_dF(net_of("tiny"), "tiny", 4, True)),
              ("train_grads_tiny_forward_only", lambda: given_dF(net_of("tiny"), "tiny", 4, False))]
    # growth and reuse on one handle of its own: B = 2, 4, 2, a VJP call, a training step again
    cases += [(f"reuse_{i}_{what}", (lambda B=B: vjp(net_of("reuse"), "tiny_sc", False) if B is None else step(net_of("reuse"), "tiny", B, 0.1)))
              for i, (what, B) in enumerate((("B2", 2), ("B4", 4), ("B2", 2), ("vjp", None), ("B4", 4)))]
    cases += [("ungrouped_32_blocks_B2", lambda: step(net_of("big", big), "tiny", 2, 0.9))]
    net_of("reuse", Y.CONFIGS["tiny"]())
    for name, run in cases:
        t0 = time.time()
        try:
            arrays = run()
        except Exception as e:   # a refusal is a result too: recorded, and compared like the arrays
            arrays = dict(refused=np.frombuffer(f"{type(e).__name__}: {e}".encode(), np.uint8))
            print(f"{name}: REFUSED {e}")
        torch.cuda.synchronize()
        np.savez(os.path.join(out_dir, name + ".npz"), **arrays)
        print(f"{name}: {len(arrays)} arrays, {time.time() - t0:.1f} s", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
