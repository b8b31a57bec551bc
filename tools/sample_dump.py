"""dev helper: A/B of the sampler entries between two builds of libdsg.so (a refactor of the reverse loop must not move a bit).
  sample_dump.py [--lib PATH] OUT     run every case below on the library at PATH (default: the tree's) and write OUT/<case>.npz:
        every output, every snapshot and the three dsg_sample_stats fields
  sample_dump.py --compare A B        per array `identical` or the differing count; exit 1 unless every array is bit-identical and
        every stat equal
Synthetic weights (weights.synth_state_dict(cfg, 0)), seeded inputs; nothing from the reference.  `tiny` and `nosc` (N = 8) at B = 5
with uneven node counts and T = 6; the table of pure-window rows needs pure windows, so its two cases run the N = 32 network of
tests/test_dedup_table.py at B = 3.  The cases reach every instantiation of the elementwise skeleton (csrc/kernels.hip) and every
phase of sample_impl (csrc/dsg_api.cpp): the three solvers with device-drawn and with recorded randomness, the sanity-check mode
with snapshots, known entries, a resampling walk from a base, per-graph seeds alone and with base and known entries, the loop
without step graphs and without any graph, the coins drawn by the library, dsg_gen_noise(_seeded) and dsg_precond."""
import ctypes as C
import glob
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
STEPS = 6
VALID = [8, 3, 5, 7, 6]   # one full graph, one of three nodes


def compare(a_dir, b_dir):
    bad = 0
    files = sorted(glob.glob(os.path.join(a_dir, "*.npz")))
    assert files and len(files) == len(glob.glob(os.path.join(b_dir, "*.npz"))), "different sets of cases"
    for fa in files:
        case = os.path.basename(fa)
        a, b = np.load(fa), np.load(os.path.join(b_dir, case))
        assert sorted(a.files) == sorted(b.files), f"{case}: different arrays"
        for k in a.files:
            same = a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()
            bad += 0 if same else 1
            what = "identical" if same else ("DIFFERENT: %s" % (f"{int((a[k] != b[k]).sum())} of {a[k].size}" if a[k].shape == b[k].shape else "shapes"))
            print(f"{case[:-4]:34s} {k:12s} {what}" + (f"  {a[k].tolist()}" if k == "stats" else ""))
    print("A/B:", f"{len(files)} cases, every array bit-identical, every stat equal" if not bad else f"{bad} arrays differ")
    return 1 if bad else 0


def main(argv):
    if argv and argv[0] == "--compare":
        return compare(argv[1], argv[2])
    from diffusesg_amd import lib
    if argv and argv[0] == "--lib":
        lib.load(argv[1])
        argv = argv[2:]
    import torch
    from diffusesg_amd import spec as S, synth as Y, weights as W
    from diffusesg_amd.model import build_network
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    out_dir = argv[0]
    os.makedirs(out_dir, exist_ok=True)
    T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cfgs = {"tiny": Y.CONFIGS["tiny"](), "nosc": Y.CONFIGS["nosc"](),
            "s": S.ModelConfig(max_node_num=32, c_adj=3, c_node=5, depths=(1, 1, 1), num_heads=(3, 6, 12), window_size=8, self_condition=True)}
    nets = {k: build_network(c, W.synth_state_dict(c, 0), device="cuda") for k, c in cfgs.items()}
    written = []

    def save(name, tensors, stats=None):
        arrays = {f"t{i}": torch.as_tensor(t).detach().cpu().numpy() for i, t in enumerate(tensors) if torch.is_tensor(t)}
        if stats is not None:
            arrays["stats"] = np.array([stats["precond_calls"], stats["net_forwards"], stats["graph_replays"]], np.int64)
        np.savez(os.path.join(out_dir, name + ".npz"), **arrays)
        written.append(name)
        print(f"{name}: {len(arrays)} arrays" + (f", stats {arrays['stats'].tolist()}" if stats is not None else ""), flush=True)

    def inputs(cfg, flags, tag, L):
        """seeded tensors of one call, NOT masked (the loop's own kernels own that): init, churn noise [L], base, known, masks, gt"""
        B, n = flags.shape
        sa, sn = (B, cfg.c_adj, n, n), (B, n, cfg.c_node)
        nrm = lambda what, shp: T(W.normal(91, f"sample_dump/{tag}/{what}", shp))
        bits = lambda what, shp: T(W.coins(91, f"sample_dump/{tag}/{what}", int(np.prod(shp))).reshape(shp) < 0.4)
        return dict(init=(nrm("ia", sa), nrm("in", sn)), noise=(nrm("na", (L,) + sa), nrm("nn", (L,) + sn)),
                    base=(nrm("ba", sa), nrm("bn", sn)), known=(nrm("ka", sa), nrm("kn", sn), bits("ma", sa), bits("mn", sn)),
                    gt=(T(np.sign(W.normal(91, f"sample_dump/{tag}/ga", sa))), T(np.sign(W.normal(91, f"sample_dump/{tag}/gn", sn)))),
                    coins=(W.coins(91, f"sample_dump/{tag}", 2 * L) < 0.5).astype(np.uint8))

    for name in ("tiny", "nosc"):
        cfg, net = cfgs[name], nets[name]
        h = net.model._ensure_handle()
        flags = T(W.synth_flags(len(VALID), cfg.max_node_num, VALID))
        chan = dict(num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj)
        mk = lambda solver="heun", **kw: NodeAdjEDMSamplerHip(num_steps=STEPS, solver=solver, S_churn=0 if solver == "dpmpp_2m" else 40,
                                                              self_condition=cfg.self_condition, dev="cuda", **kw)
        x = inputs(cfg, flags.cpu().numpy(), name, STEPS)
        rec = dict(init_adjs=x["init"][0], init_nodes=x["init"][1], churn_noise=x["noise"], coins=x["coins"])
        for solver in ("heun", "euler", "dpmpp_2m"):
            smp = mk(solver)
            np.random.seed(5)   # the unseeded call's coins come from NumPy's global generator
            save(f"{name}_{solver}_device_noise", smp.sample(net, flags, seed=7, **chan), smp.last_stats)
            save(f"{name}_{solver}_recorded", smp.sample(net, flags, **rec, **chan), smp.last_stats)
        smp = mk()
        save(f"{name}_sanity_snapshots", smp.sample(net, flags, sanity_check_gt_adjs=x["gt"][0], sanity_check_gt_nodes=x["gt"][1], flag_interim_adjs=True,
                                                    max_num_interim_adjs=4, **rec, **chan), smp.last_stats)
        save(f"{name}_multistep_sanity", mk("dpmpp_2m").sample(net, flags, sanity_check_gt_adjs=x["gt"][0], sanity_check_gt_nodes=x["gt"][1], **rec, **chan))
        save(f"{name}_known", smp.sample_known(net, flags, *x["known"], flag_interim_adjs=True, **rec, **chan), smp.last_stats)
        walk = dict(start_step=2, base_adjs=x["base"][0], base_nodes=x["base"][1], resample=(2, 2))
        L = len(lib.walk_steps(smp._cfg(), lib.make_walk_cfg(2, (2, 2), None))[0])
        xw = inputs(cfg, flags.cpu().numpy(), name + "/walk", L)
        save(f"{name}_walk_base_resample", smp.sample_known(net, flags, *x["known"], init_adjs=x["init"][0], init_nodes=x["init"][1], churn_noise=xw["noise"],
                                                            coins=xw["coins"], **walk, **chan), smp.last_stats)
        np.random.seed(6)
        save(f"{name}_walk_device_noise", smp.sample_known(net, flags, *x["known"], seed=11, **walk, **chan), smp.last_stats)
        seeds = [3, 2 ** 63 + 5, 17, 0, 99]
        save(f"{name}_seeded", smp.sample(net, flags, graph_seeds=seeds, coin_seed=4, flag_interim_adjs=True, max_num_interim_adjs=3, **chan), smp.last_stats)
        save(f"{name}_seeded_base_known", smp.sample_known(net, flags, *x["known"], graph_seeds=seeds, coin_seed=4, start_step=1, base_adjs=x["base"][0],
                                                           base_nodes=x["base"][1], **chan), smp.last_stats)
        save(f"{name}_seeded_multistep", mk("dpmpp_2m").sample(net, flags, graph_seeds=seeds, coin_seed=4, **chan))
        h.set_option("loop_graph", 0)
        save(f"{name}_loop_graph_0", smp.sample(net, flags, **rec, **chan), smp.last_stats)
        h.set_option("loop_graph", 1)
        eager = mk(use_graph=False)
        save(f"{name}_use_graph_off", eager.sample(net, flags, **rec, **chan), eager.last_stats)
        # coins == NULL: the library draws them itself (no Python caller does this)
        B, n = flags.shape
        oa, on = torch.empty((B, cfg.c_adj, n, n), device="cuda"), torch.empty((B, n, cfg.c_node), device="cuda")
        stats, scfg, p = lib.DsgSampleStats(), smp._cfg(), (lambda t: C.c_void_p(t.data_ptr()))
        fl8 = flags.to(torch.uint8)
        h.check(h.L.dsg_sample(h.raw, C.byref(scfg), B, p(fl8), None, None, None, None, None, C.c_uint64(21), None, None, None, 0,
                               None, None, p(oa), p(on), C.byref(stats), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "dsg_sample")
        torch.cuda.synchronize()
        save(f"{name}_library_coins", (oa, on), dict(precond_calls=stats.precond_calls, net_forwards=stats.net_forwards, graph_replays=stats.graph_replays))
        save(f"{name}_gen_noise", smp.device_noise(net, flags, stream=3, seed=13))
        save(f"{name}_gen_noise_seeded", smp.device_noise(net, flags, stream=3, graph_seeds=seeds))
        sig = T(np.array([80.0, 1.5, 0.002, 7.0, 0.3], np.float32))
        for coin in (0.9, 0.1):   # without / with the self-conditioning coin's extra pass
            real, np.random.rand = np.random.rand, (lambda *a: coin)
            try:
                save(f"{name}_precond_coin{coin}", net(x["init"][0], x["init"][1], flags, sig))
            finally:
                np.random.rand = real

    # the table of pure-window rows: "dedup_batch" 2 shares one representative across these three graphs
    cfg, net = cfgs["s"], nets["s"]
    h = net.model._ensure_handle()
    flags = T(W.synth_flags(3, 32, [17, 30, 32]))
    x = inputs(cfg, flags.cpu().numpy(), "s", STEPS)
    smp = NodeAdjEDMSamplerHip(num_steps=STEPS, self_condition=True, dev="cuda")
    h.set_option("fused_merge", 2)
    h.set_option("dedup_batch", 2)
    for on in (0, 1):
        h.set_option("dedup_table", on)
        assert h.get_option("dedup_table") == on, "the batch does not share its representative"
        save(f"s_dedup_table_{on}", smp.sample(net, flags, init_adjs=x["init"][0], init_nodes=x["init"][1], churn_noise=x["noise"], coins=x["coins"],
                                               num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj), smp.last_stats)
        assert h.dedup_launch_lists(3, 0)["mode"] == (3 if on else 2)
    torch.cuda.synchronize()
    print(f"{len(written)} cases written to {out_dir}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
