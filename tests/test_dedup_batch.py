"""One computed pure window for the whole batch (option "dedup_batch", include/dsg.h): results.

In the sampler sigma -- and with it every block's (scale, shift) row -- is the same for all graphs of a batch and every network input
is zero at padded pairs, so the argument that gives two pure windows of one graph the same rows gives them to two pure windows of
different graphs as well.  "dedup_batch" 2 computes the batch's first pure window per level, fills from it across graphs, and below
the top of the chain fills only what is read.  All GPU checks go through the C ABI and use no tolerance (torch.equal):
  1. sampler outputs with "dedup_batch" 2 against "dedup_batch" 0 (one representative per graph) and against "dedup_masked" 0 --
     Heun + churn with coins, a full-flag poisoning run between cases, step graphs captured under one kind of list and replayed
     under the other, in both orders (the option does not drop the captured graphs: they are the same); three networks;
  2. the conditioned and the seeded flavours with caller tensors that are non-zero at padded pairs;
  3. seeded with "batch_invariant" 1: graph b of a batch of 3 is the B = 1 run with its seed;
  4. the threshold of the default value 1: one representative from 16 graphs on, per graph below;
  5. dsg_denoise (per-sample noise labels, caller tensors) fills nothing whatever the option says.
CPU, with the oracle: pure windows of two graphs with the same c_noise share their rows at level 0 and at level 1; with different
  c_noise they do not -- why the batch-uniform row is a precondition.
"""
import numpy as np
import pytest

from diffusesg_amd import spec as S
from diffusesg_amd import synth as Y
from diffusesg_amd import weights as W

STEPS = 6
WS = 8
# name -> (configuration, levels that deduplicate with "fused_merge" 2)
#   "vg": the headline network, depths (1, 1, 3, 1): levels 0 and 1 trim their fills, level 2 is the top
#   "d2": N = 64, depths (1, 2, 1): level 1 is the top (a shifted block follows), level 0 trims
#   "s":  N = 32, depths (1, 1, 1): level 1 (2 x 2 windows) is the top, level 0 trims
_specs = {"vg": (lambda: S.vg_config(), 3),
          "d2": (lambda: S.ModelConfig(max_node_num=64, c_adj=3, c_node=5, depths=(1, 2, 1), num_heads=(3, 6, 12), window_size=WS,
                                       self_condition=True), 2),
          "s": (lambda: S.ModelConfig(max_node_num=32, c_adj=3, c_node=5, depths=(1, 1, 1), num_heads=(3, 6, 12), window_size=WS,
                                      self_condition=True), 2)}
_cfgs, _nets = {}, {}


def cfg_for(name):
    if name not in _cfgs:
        _cfgs[name] = _specs[name][0]()
    return _cfgs[name]


def net_for(name):
    from diffusesg_amd.model import build_network
    if name not in _nets:
        cfg = cfg_for(name)
        _nets[name] = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")
    return _nets[name]


def T(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def prefix(n, valid):
    return W.synth_flags(len(valid), n, [min(n, v) for v in valid])


def batches(n):
    scattered = np.zeros((3, n), bool)
    scattered[0, [9, 10, n - 20]] = True
    scattered[1, [n // 2 + 1]] = True
    scattered[2, [0, n - 1]] = True
    no_pure = np.zeros((2, n), bool)
    no_pure[0, ::8] = True
    no_pure[1, 7::8] = True
    return {"edges": prefix(n, [17, 30, 31, 32]),
            "rep_moves": prefix(n, [n // 2 + 1, n // 2 - 2]),   # N = 64: [33, 30] -- level 2's representative in graph 1, level 1's in graph 0
            "only_graph2": prefix(n, [n, n, n // 2 - 2, n]),
            "uneven": prefix(n, [30, 0, n]),
            "scattered": scattered,
            "no_pure": no_pure}


def sample_case(cfg, flags, seed, tag):
    """recorded randomness of one sampler call.  Init and churn noise are NOT masked: the loop's own kernels own that"""
    B, n = flags.shape
    ia = W.normal(seed, f"{tag}/init_adj", (B, cfg.c_adj, n, n))
    inn = W.normal(seed, f"{tag}/init_node", (B, n, cfg.c_node))
    na = np.stack([W.normal(seed, f"{tag}/churn_adj/{i}", (B, cfg.c_adj, n, n)) for i in range(STEPS)])
    nn = np.stack([W.normal(seed, f"{tag}/churn_node/{i}", (B, n, cfg.c_node)) for i in range(STEPS)])
    coins = (W.coins(seed, tag, 2 * STEPS - 1) < 0.5).astype(np.uint8)
    return dict(flags=T(flags), init_adjs=T(ia), init_nodes=T(inn), churn_noise=(T(na), T(nn)), coins=coins)


def run(smp, net, cfg, case):
    import torch
    out = smp.sample(net, case["flags"], init_adjs=case["init_adjs"], init_nodes=case["init_nodes"], churn_noise=case["churn_noise"],
                     coins=case["coins"], num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj)
    return [torch.as_tensor(t).clone() for t in out]


def reset(h):
    for k, v in (("fused_merge", 1), ("batch_invariant", 0), ("dedup_masked", 1), ("dedup_levels", 0), ("dedup_batch", 1)):
        h.set_option(k, v)


def shared_everywhere(h, B, depth):
    """the staged lists are the batch kind: one representative id for all graphs at every level that has a pure window"""
    for lv in range(depth):
        d = h.dedup_level_lists(B, lv)
        assert d["fwd"] >= 0 and len(set(d["rep"].tolist())) == 1
    return True


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["vg", "d2", "s"])
def test_sampler_bit_identical_across_batch_and_per_graph_and_off(name):
    import torch
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    cfg, net = cfg_for(name), net_for(name)
    n, depth = cfg.max_node_num, _specs[name][1]
    h = net.model._ensure_handle()
    smp = NodeAdjEDMSamplerHip(num_steps=STEPS, self_condition=True, dev="cuda")   # Heun + churn, hipGraph on
    cases = {k: sample_case(cfg, f, 53, f"dedup_batch/{name}/{k}") for k, f in batches(n).items()}
    poison = {B: sample_case(cfg, np.ones((B, n), bool), 55, f"dedup_batch/{name}/poison{B}") for B in {len(f) for f in batches(n).values()}}
    try:
        h.set_option("fused_merge", 2)   # the partial-statistics PatchMerging at every size: the whole chain at these batch sizes
        h.set_option("dedup_masked", 0)
        ref = {k: run(smp, net, cfg, c) for k, c in cases.items()}
        h.set_option("dedup_masked", 1)
        assert h.get_option("dedup_levels") == depth
        for first, second in ((0, 2), (2, 0)):
            h.set_option("dedup_levels", 0)     # drops the captured graphs: the next calls capture under `first`'s lists
            h.set_option("dedup_batch", first)  # ... and this one keeps them
            assert h.get_option("dedup_batch") == first
            filled = [0] * depth
            for mode in (first, second):
                h.set_option("dedup_batch", mode)
                for k, c in cases.items():
                    B = c["flags"].shape[0]
                    run(smp, net, cfg, poison[B])   # rewrites every activation row with other values; captures nothing new after the first time
                    got = run(smp, net, cfg, c)
                    assert torch.equal(got[0], ref[k][0]) and torch.equal(got[1], ref[k][1]), \
                        f"{name} {k}: dedup_batch {mode} (graphs captured under {first}) differs from dedup_masked 0"
                    reps = [h.dedup_level_lists(B, lv) for lv in range(depth)]
                    assert all(d["fwd"] >= 0 for d in reps)
                    if mode == 2:
                        assert all(len(set(d["rep"].tolist())) == 1 for d in reps)
                        for lv in range(depth):
                            filled[lv] += len(reps[lv]["copy"])
                    elif k == "only_graph2":
                        assert all(sorted(set(d["rep"].tolist())) == [-1, int(d["rep"][2])] and d["rep"][2] >= 0 for d in reps)
            assert all(f > 0 for f in filled), f"{name}: nothing was filled across the batch at some level: {filled}"
    finally:
        reset(h)


@pytest.mark.gpu
def test_known_values_and_base_at_padded_pairs_and_seeds():
    """The conditioned flavour (partial-noise start) and the seeded one store `valid ? ... : 0` themselves and run at one sigma: both
    share across the batch.  The caller's known tensors, masks and base are non-zero at padded pairs."""
    import torch
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    cfg, net = cfg_for("vg"), net_for("vg")
    n, B = cfg.max_node_num, 3
    flags = T(prefix(n, [n // 2 + 1, 3, 9]))
    ka = T(W.normal(9, "dedup_batch/known/adj", (B, cfg.c_adj, n, n)))           # none of these is masked
    kn = T(W.normal(9, "dedup_batch/known/node", (B, n, cfg.c_node)))
    ba = T(W.normal(9, "dedup_batch/base/adj", (B, cfg.c_adj, n, n)))
    bn = T(W.normal(9, "dedup_batch/base/node", (B, n, cfg.c_node)))
    ma = T(W.normal(9, "dedup_batch/known/mask_adj", (B, cfg.c_adj, n, n)) > 0.3)   # known entries everywhere, padded pairs included
    mn = T(W.normal(9, "dedup_batch/known/mask_node", (B, n, cfg.c_node)) > 0.3)
    smp = NodeAdjEDMSamplerHip(num_steps=STEPS, self_condition=True, dev="cuda")
    L = STEPS - 2
    coins = (W.coins(9, "dedup_batch/known", 2 * L - 1) < 0.5).astype(np.uint8)
    kw = dict(num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj)
    h = net.model._ensure_handle()

    def calls(check):
        out = []
        for call in (lambda: smp.sample_known(net, flags, ka, kn, ma, mn, seed=31, coins=coins, start_step=2, base_adjs=ba, base_nodes=bn, **kw),
                     lambda: smp.sample(net, flags, graph_seeds=[5, 2 ** 40 + 1, 77], coin_seed=3, **kw)):
            out += [torch.as_tensor(t).clone() for t in call()]
            if check:
                assert shared_everywhere(h, B, 3) and all(len(h.dedup_level_lists(B, lv)["copy"]) > 0 for lv in range(3))
        return out
    try:
        h.set_option("fused_merge", 2)
        h.set_option("dedup_masked", 0)
        ref = calls(False)
        h.set_option("dedup_masked", 1)
        h.set_option("dedup_batch", 0)
        per_graph = calls(False)
        h.set_option("dedup_batch", 2)
        got = calls(True)
        for g, p, r in zip(got, per_graph, ref):
            assert torch.equal(g, r) and torch.equal(p, r)
    finally:
        reset(h)


@pytest.mark.gpu
def test_seeded_graph_of_a_batch_is_its_own_b1_run_under_batch_invariant():
    """"batch_invariant" does not restrict the option: the rows are the same whichever graph computed them.  Graph 1 has no valid node
    and graph 2 no pure window at level 2, so in the batch their pure windows come from graph 0's, in the B = 1 runs from their own."""
    import torch
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    cfg, net = cfg_for("vg"), net_for("vg")
    n = cfg.max_node_num
    fl = prefix(n, [30, 0, 33])
    seeds = [11, 2 ** 35 + 7, 5]
    coins = (W.coins(13, "dedup_batch/seeded", 2 * STEPS - 1) < 0.5).astype(np.uint8)
    smp = NodeAdjEDMSamplerHip(num_steps=STEPS, self_condition=True, dev="cuda")
    kw = dict(num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj)
    h = net.model._ensure_handle()
    try:
        h.set_option("batch_invariant", 1)
        h.set_option("dedup_batch", 2)
        assert h.get_option("dedup_levels") == 3
        full = [torch.as_tensor(t).clone() for t in smp.sample(net, T(fl), graph_seeds=seeds, coins=coins, **kw)]
        assert shared_everywhere(h, 3, 3) and int(h.dedup_level_lists(3, 2)["rep"][0]) < 4
        for b in range(3):
            one = [torch.as_tensor(t).clone() for t in smp.sample(net, T(fl[b:b + 1]), graph_seeds=[seeds[b]], coins=coins, **kw)]
            assert torch.equal(full[0][b], one[0][0]) and torch.equal(full[1][b], one[1][0]), f"graph {b} differs from its B = 1 run"
    finally:
        reset(h)


@pytest.mark.gpu
def test_default_value_shares_from_16_graphs_on():
    """N = 32 network.  "dedup_batch" is left at its default 1; "fused_merge" 2 puts level 1 into the chain at these batch sizes (under
    its default the merge_ln form ends the chain behind level 0, which is then the top and may not trim), so level 0 trims."""
    import torch
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    cfg, net = cfg_for("s"), net_for("s")
    n = cfg.max_node_num
    h = net.model._ensure_handle()
    smp = NodeAdjEDMSamplerHip(num_steps=STEPS, self_condition=True, dev="cuda")
    valid = [5, 13, 9, 30, 17, 1, 0, 32, 8, 16, 24, 7, 15, 12, 3, 20]
    nW = (n // WS) ** 2
    try:
        h.set_option("fused_merge", 2)
        assert h.get_option("dedup_batch") == 1
        for B in (16, 4):
            fl = prefix(n, valid[:B])
            case = sample_case(cfg, fl, 61, f"dedup_batch/threshold/{B}")
            h.set_option("dedup_batch", 0)
            ref = run(smp, net, cfg, case)
            per_graph = h.dedup_level_lists(B, 0)
            h.set_option("dedup_batch", 1)
            got = run(smp, net, cfg, case)
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
            d0, d1 = h.dedup_level_lists(B, 0), h.dedup_level_lists(B, 1)
            assert d0["fwd"] >= 0 and d1["fwd"] >= 0
            if B >= 16:
                assert len(set(d0["rep"].tolist())) == 1 and 0 <= d0["rep"][0] < nW, "one representative, in graph 0"
                assert len(set(d1["rep"].tolist())) == 1
                pure0 = B * nW - (len(d0["wins"]) - 1)
                assert 0 < len(d0["copy"]) < pure0 - 1, "level 0's fill is trimmed: fewer entries than pure windows besides the representative"
                assert len(d0["wins"]) < len(per_graph["wins"])
            else:
                assert np.array_equal(d0["rep"], per_graph["rep"]) and np.array_equal(np.sort(d0["copy"]), np.sort(per_graph["copy"]))
                assert all(r < 0 or r // nW == b for b, r in enumerate(d0["rep"].tolist())) and len(set(d0["rep"].tolist())) > 1
    finally:
        reset(h)


@pytest.mark.gpu
def test_denoise_fills_nothing_and_matches_option_0():
    """dsg_denoise: per-sample noise labels and caller tensors (non-zero at padded pairs here): every window of every level is unique."""
    import torch
    cfg, net = cfg_for("d2"), net_for("d2")
    n, B = cfg.max_node_num, 3
    flags = prefix(n, [n // 2 - 1, 3, 0])
    adj = W.normal(7, "dedup_batch/denoise/adj", (B, cfg.c_adj, n, n))   # not masked
    node = W.normal(7, "dedup_batch/denoise/node", (B, n, cfg.c_node))
    sc_adj = W.normal(7, "dedup_batch/denoise/sc_adj", (B, cfg.c_adj, n, n))
    sc_node = W.normal(7, "dedup_batch/denoise/sc_node", (B, n, cfg.c_node))
    c_noise = np.array([-1.2, 0.2, 1.0], np.float32)
    args = (T(adj), T(node), T(flags), T(c_noise), T(sc_adj), T(sc_node))
    h = net.model._ensure_handle()
    try:
        h.set_option("fused_merge", 2)
        h.set_option("dedup_batch", 0)
        ref = [t.clone() for t in net.model(*args)]
        h.set_option("dedup_batch", 2)
        got = [t.clone() for t in net.model(*args)]
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
        for lv in range(2):
            d = h.dedup_level_lists(B, lv)
            nw = ((n >> lv) // WS) ** 2
            assert len(d["copy"]) == 0 and len(d["wins"]) == B * nw and len(d["runs"]) == B * nw * 8 and (d["rep"] == -1).all()
    finally:
        reset(h)


# ---- CPU, with the oracle ----------------------------------------------------------------------------------------------------
def window_rows(tap, B, res, C):
    nwr = res // WS
    return tap.reshape(B, nwr, WS, nwr, WS, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, nwr * nwr, WS * WS, C)


def oracle_taps(c_noise):
    from oracle.oracle import Oracle
    n = 64
    cfg = S.ModelConfig(max_node_num=n, c_adj=3, c_node=5, depths=(1, 1, 1), num_heads=(3, 6, 12), window_size=WS, self_condition=True)
    flags, adj, node, sc_adj, sc_node = Y.case_inputs(cfg, 2, [11, 27], 5, "dedup_batch/oracle")   # masked like the sampler hands them over
    E = cfg.embed_dim
    sizes = {"patch_embed": n * n * E, "down0.block0": n * n * E, "down0": (n // 2) ** 2 * 2 * E, "down1.block0": (n // 2) ** 2 * 2 * E}
    _, _, taps = Oracle(cfg, W.synth_state_dict(cfg, 0)).forward(adj, node, flags, np.asarray(c_noise, np.float32), sc_adj, sc_node, taps=dict(sizes))
    out = {}
    for name, k in (("patch_embed", 0), ("down0.block0", 0), ("down0", 1), ("down1.block0", 1)):
        res = n >> k
        nwr = res // WS
        side = WS << k
        x = window_rows(taps[name], 2, res, E << k)
        pure = []
        for b in range(2):
            blk = flags[b].reshape(nwr, side).any(axis=1)
            pure.append(int(np.flatnonzero(~(blk[:, None] & blk[None, :]).reshape(-1))[0]))
        assert np.array_equal(x[0, pure[0]], x[0, nwr * nwr - 1]), "two pure windows of one graph"
        assert not np.array_equal(x[0, 0], x[0, pure[0]]), "window 0 holds valid pairs"
        out[name] = (x[0, pure[0]], x[1, pure[1]])
    return out


def test_pure_windows_of_two_graphs_share_their_rows_in_the_oracle_at_one_c_noise():
    for name, (a, b) in oracle_taps([0.4, 0.4]).items():
        assert np.array_equal(a, b), f"{name}: a pure window of graph 0 and one of graph 1 differ at the same c_noise"


def test_pure_windows_of_two_graphs_differ_at_different_c_noise():
    for name, (a, b) in oracle_taps([0.4, -0.7]).items():
        assert not np.array_equal(a, b), f"{name}: pure windows of graphs with different noise labels should not share their rows"
