"""The sampler's table of pure-window rows (option "dedup_table", include/dsg.h): results.

Where a batch shares one representative pure window per level ("dedup_batch"), that window's rows depend on the weights and on the
step's (scale, shift) row only.  With "dedup_table" 1 a sampler call computes them once per schedule index ahead of its loop -- with
the down path itself, on all-padding pseudo-batches of B indices, per-sample rows -- and the fill writes the window from the table;
no launch of the loop computes it.  All GPU checks go through the C ABI and use no tolerance (torch.equal); 6 steps, Heun + churn with
coins, "fused_merge" 2 (the whole chain at small batches) and "dedup_batch" 2 (the batch form at 2 - 4 graphs):
  1. sampler outputs with "dedup_table" 1 against 0 and against "dedup_masked" 0 -- prefix, scattered and all-true flags, a full-flag
     poisoning run between cases, both orders of the option: it does not drop the captured step bodies, they are the same and a word
     on the device selects the fill's source; three networks;
  2. the conditioned partially-noised resampling walk (more executed steps than schedule indices), the seeded flavour under
     "batch_invariant" 1 and the multistep solver, caller tensors non-zero at padded pairs;
  3. chunking and growth: B = 4 with 6 steps (two chunks, the second short), B = 8 (more graphs than steps), then more steps on the
     same handle (the table grows), then fewer;
  4. an eager forward (dsg_profile_forward) behind a call that replayed every step body: the build leaves the workspace in the
     sampler's batch-uniform form;
  5. dsg_denoise fills nothing and gives the same bits under both values.
CPU, with the oracle: at one c_noise the windows of an all-padding graph are the pure windows of a mixed graph at levels 0 and 1, with
  and without a self-conditioning input -- what lets a pseudo-batch stand in for the batch.
(The lists: tests/test_dedup_table_lists.py.)
"""
import numpy as np
import pytest

from diffusesg_amd import spec as S
from diffusesg_amd import synth as Y
from diffusesg_amd import weights as W

STEPS = 6
WS = 8
# the three networks of tests/test_dedup_batch.py: name -> (configuration, levels that deduplicate with "fused_merge" 2)
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
    return {"edges": prefix(n, [17, 30, 31, 32]),   # below 24 valid nodes a non-pure coarse window covers pure fine windows
            "rep_moves": prefix(n, [33, 30]),
            "uneven": prefix(n, [30, 0, n]),
            "scattered": scattered,
            "all_true": np.ones((2, n), bool)}      # nothing to fill


def sample_case(cfg, flags, seed, tag, steps=STEPS):
    """recorded randomness of one sampler call.  Init and churn noise are NOT masked: the loop's own kernels own that"""
    B, n = flags.shape
    ia = W.normal(seed, f"{tag}/init_adj", (B, cfg.c_adj, n, n))
    inn = W.normal(seed, f"{tag}/init_node", (B, n, cfg.c_node))
    na = np.stack([W.normal(seed, f"{tag}/churn_adj/{i}", (B, cfg.c_adj, n, n)) for i in range(steps)])
    nn = np.stack([W.normal(seed, f"{tag}/churn_node/{i}", (B, n, cfg.c_node)) for i in range(steps)])
    coins = (W.coins(seed, tag, 2 * steps - 1) < 0.5).astype(np.uint8)
    return dict(flags=T(flags), init_adjs=T(ia), init_nodes=T(inn), churn_noise=(T(na), T(nn)), coins=coins)


def run(smp, net, cfg, case):
    import torch
    out = smp.sample(net, case["flags"], init_adjs=case["init_adjs"], init_nodes=case["init_nodes"], churn_noise=case["churn_noise"],
                     coins=case["coins"], num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj)
    return [torch.as_tensor(t).clone() for t in out]


def reset(h):
    for k, v in (("fused_merge", 1), ("batch_invariant", 0), ("dedup_masked", 1), ("dedup_levels", 0), ("dedup_batch", 1), ("dedup_table", 1)):
        h.set_option(k, v)


def modes(h, B, depth):
    return [h.dedup_launch_lists(B, lv)["mode"] for lv in range(depth)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["vg", "d2", "s"])
def test_sampler_bit_identical_with_the_table_without_it_and_off(name):
    import torch
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    cfg, net = cfg_for(name), net_for(name)
    n, depth = cfg.max_node_num, _specs[name][1]
    h = net.model._ensure_handle()
    smp = NodeAdjEDMSamplerHip(num_steps=STEPS, self_condition=True, dev="cuda")   # Heun + churn, hipGraph on
    cases = {k: sample_case(cfg, f, 71, f"dedup_table/{name}/{k}") for k, f in batches(n).items()}
    poison = {B: sample_case(cfg, np.ones((B, n), bool), 73, f"dedup_table/{name}/poison{B}") for B in {len(f) for f in batches(n).values()}}
    try:
        h.set_option("fused_merge", 2)
        h.set_option("dedup_batch", 2)
        h.set_option("dedup_masked", 0)
        assert h.get_option("dedup_table") == 0, "reported as what runs"
        ref = {k: run(smp, net, cfg, c) for k, c in cases.items()}
        h.set_option("dedup_masked", 1)
        assert h.get_option("dedup_levels") == depth and h.get_option("dedup_table") == 1
        for first, second in ((0, 1), (1, 0)):
            h.set_option("dedup_levels", 0)      # drops the captured graphs: the next calls capture under `first`
            h.set_option("dedup_table", first)   # ... and this one keeps them
            filled = [0] * depth
            for on in (first, second):
                h.set_option("dedup_table", on)
                assert h.get_option("dedup_table") == on
                for k, c in cases.items():
                    B = c["flags"].shape[0]
                    run(smp, net, cfg, poison[B])   # rewrites every activation row with other values
                    got = run(smp, net, cfg, c)
                    assert torch.equal(got[0], ref[k][0]) and torch.equal(got[1], ref[k][1]), \
                        f"{name} {k}: dedup_table {on} (graphs captured under {first}) differs from dedup_masked 0"
                    assert modes(h, B, depth) == [3 if on else 2] * depth
                    if on:
                        for lv in range(depth):
                            filled[lv] += len(h.dedup_launch_lists(B, lv)["copy"])
                        if k == "all_true":
                            assert all(len(h.dedup_launch_lists(B, lv)["copy"]) == 0 for lv in range(depth))
            assert all(f > 0 for f in filled), f"{name}: nothing was filled from the table at some level: {filled}"
    finally:
        reset(h)


@pytest.mark.gpu
def test_flavours_with_caller_tensors_nonzero_at_padded_pairs():
    """Conditioned + partial-noise start + resampling (8 executed steps on 6 schedule indices: the table is indexed by schedule
    index), seeded under "batch_invariant" 1, and the multistep solver.  Known tensors, masks and base are not masked."""
    import torch
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    cfg, net = cfg_for("vg"), net_for("vg")
    n, B = cfg.max_node_num, 3
    flags = T(prefix(n, [n // 2 + 1, 3, 19]))
    ka = T(W.normal(9, "dedup_table/known/adj", (B, cfg.c_adj, n, n)))
    kn = T(W.normal(9, "dedup_table/known/node", (B, n, cfg.c_node)))
    ba = T(W.normal(9, "dedup_table/base/adj", (B, cfg.c_adj, n, n)))
    bn = T(W.normal(9, "dedup_table/base/node", (B, n, cfg.c_node)))
    ma = T(W.normal(9, "dedup_table/known/mask_adj", (B, cfg.c_adj, n, n)) > 0.3)
    mn = T(W.normal(9, "dedup_table/known/mask_node", (B, n, cfg.c_node)) > 0.3)
    smp = NodeAdjEDMSamplerHip(num_steps=STEPS, self_condition=True, dev="cuda")
    ms = NodeAdjEDMSamplerHip(num_steps=STEPS, self_condition=True, dev="cuda", solver="dpmpp_2m", S_churn=0.0)
    coins = (W.coins(9, "dedup_table/flavours", 32) < 0.5).astype(np.uint8)
    kw = dict(num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj)
    h = net.model._ensure_handle()

    def calls(mode):
        out = []
        for call in (lambda: smp.sample_known(net, flags, ka, kn, ma, mn, seed=31, coins=coins, start_step=2, base_adjs=ba, base_nodes=bn,
                                              resample=(2, 2), **kw),
                     lambda: smp.sample(net, flags, graph_seeds=[5, 2 ** 40 + 1, 77], coins=coins, **kw),
                     lambda: ms.sample(net, flags, seed=17, coins=coins, **kw)):
            out += [torch.as_tensor(t).clone() for t in call()]
            if mode is not None:
                assert modes(h, B, 3) == [mode] * 3 and all(len(h.dedup_launch_lists(B, lv)["copy"]) > 0 for lv in range(3))
        return out
    try:
        h.set_option("fused_merge", 2)
        h.set_option("batch_invariant", 1)
        h.set_option("dedup_batch", 2)
        h.set_option("dedup_masked", 0)
        ref = calls(None)
        h.set_option("dedup_masked", 1)
        h.set_option("dedup_table", 0)
        without = calls(2)
        h.set_option("dedup_table", 1)
        got = calls(3)
        for g, p, r in zip(got, without, ref):
            assert torch.equal(g, r) and torch.equal(p, r)
    finally:
        reset(h)


@pytest.mark.gpu
def test_chunks_short_chunks_and_a_table_that_grows():
    """The table is built in chunks of B schedule indices: 6 steps at B = 4 are two chunks, the second short; at B = 8 one short chunk.
    More steps on the same handle grow the table (and drop the step bodies, which bake its address); fewer steps reuse it."""
    import torch
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    cfg, net = cfg_for("s"), net_for("s")
    n = cfg.max_node_num
    h = net.model._ensure_handle()
    valid = {4: [5, 13, 9, 30], 8: [5, 13, 9, 30, 17, 1, 0, 32]}
    plan = [(4, 6), (8, 6), (4, 11), (4, 5), (8, 3)]   # (graphs, steps), in this order on one handle
    samplers = {t: NodeAdjEDMSamplerHip(num_steps=t, self_condition=True, dev="cuda") for t in {t for _, t in plan}}
    cases = {(B, t): sample_case(cfg, prefix(n, valid[B]), 83, f"dedup_table/chunks/{B}/{t}", steps=t) for B, t in plan}
    try:
        h.set_option("fused_merge", 2)
        h.set_option("dedup_batch", 2)
        h.set_option("dedup_table", 0)
        ref = {k: run(samplers[k[1]], net, cfg, c) for k, c in cases.items()}
        h.set_option("dedup_table", 1)
        bytes_at = {}
        for B, t in plan:
            got = run(samplers[t], net, cfg, cases[(B, t)])
            assert torch.equal(got[0], ref[(B, t)][0]) and torch.equal(got[1], ref[(B, t)][1]), f"B = {B}, {t} steps"
            assert modes(h, B, 2) == [3, 3]
            bytes_at[(B, t)] = h.L.dsg_workspace_bytes(h.raw, B)
        assert bytes_at[(4, 11)] > bytes_at[(4, 6)], "the table grew with the step count and is counted"
        assert bytes_at[(4, 5)] == bytes_at[(4, 11)] and bytes_at[(8, 3)] == bytes_at[(8, 6)], "fewer steps keep the table"
    finally:
        reset(h)


@pytest.mark.gpu
def test_eager_forward_behind_a_call_that_only_replayed_its_step_bodies():
    """The second of two identical calls captures nothing: every step body is replayed, so nothing on the host says again which kind
    of forward the workspace runs.  The table build (per-sample pseudo-batches) must leave that word as the sampler had it, or
    dsg_profile_forward -- eager forwards on the lists and the state the run left, `bench.py --full` -- is refused."""
    import ctypes as C
    import torch
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    cfg, net = cfg_for("s"), net_for("s")
    n, B = cfg.max_node_num, 4
    h = net.model._ensure_handle()
    smp = NodeAdjEDMSamplerHip(num_steps=STEPS, self_condition=True, dev="cuda")
    case = sample_case(cfg, prefix(n, [5, 13, 9, 30]), 91, "dedup_table/replay")
    try:
        h.set_option("fused_merge", 2)
        h.set_option("dedup_batch", 2)
        first = run(smp, net, cfg, case)
        second = run(smp, net, cfg, case)
        assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
        assert modes(h, B, 2) == [3, 3]
        ms, cnt, fl = (C.c_double * 5)(), (C.c_int64 * 5)(), (C.c_double * 5)()
        gemm_ms = C.c_double(0.0)
        st = torch.cuda.current_stream().cuda_stream
        h.check(h.L.dsg_profile_forward(h.raw, B, 1, ms, cnt, fl, C.byref(gemm_ms), C.c_void_p(st)), "dsg_profile_forward")
        assert sum(cnt) > 0
    finally:
        reset(h)


@pytest.mark.gpu
def test_denoise_fills_nothing_under_both_values():
    import torch
    cfg, net = cfg_for("d2"), net_for("d2")
    n, B = cfg.max_node_num, 3
    flags = prefix(n, [n // 2 - 1, 3, 0])
    adj = W.normal(7, "dedup_table/denoise/adj", (B, cfg.c_adj, n, n))   # not masked
    node = W.normal(7, "dedup_table/denoise/node", (B, n, cfg.c_node))
    sc_adj = W.normal(7, "dedup_table/denoise/sc_adj", (B, cfg.c_adj, n, n))
    sc_node = W.normal(7, "dedup_table/denoise/sc_node", (B, n, cfg.c_node))
    c_noise = np.array([-1.2, 0.2, 1.0], np.float32)
    args = (T(adj), T(node), T(flags), T(c_noise), T(sc_adj), T(sc_node))
    h = net.model._ensure_handle()
    try:
        h.set_option("fused_merge", 2)
        h.set_option("dedup_batch", 2)
        h.set_option("dedup_table", 0)
        ref = [t.clone() for t in net.model(*args)]
        h.set_option("dedup_table", 1)
        got = [t.clone() for t in net.model(*args)]
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
        for lv in range(2):
            d = h.dedup_launch_lists(B, lv)
            nw = ((n >> lv) // WS) ** 2
            assert d["mode"] == 0 and len(d["copy"]) == 0 and len(d["wins"]) == B * nw and len(d["runs"]) == B * nw * 8
    finally:
        reset(h)


# ---- CPU, with the oracle ----------------------------------------------------------------------------------------------------
def window_rows(tap, B, res, C):
    nwr = res // WS
    return tap.reshape(B, nwr, WS, nwr, WS, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, nwr * nwr, WS * WS, C)


@pytest.mark.parametrize("self_cond", [True, False], ids=["self_cond", "no_self_cond"])
def test_windows_of_an_all_padding_graph_are_the_pure_windows_of_a_mixed_graph_in_the_oracle(self_cond):
    from oracle.oracle import Oracle
    n = 64
    cfg = S.ModelConfig(max_node_num=n, c_adj=3, c_node=5, depths=(1, 1, 1), num_heads=(3, 6, 12), window_size=WS, self_condition=True)
    flags, adj, node, sc_adj, sc_node = Y.case_inputs(cfg, 2, [11, 0], 5, "dedup_table/oracle")   # graph 1: no valid node
    assert not flags[1].any() and not adj[1].any() and not node[1].any() and not sc_adj[1].any()
    E = cfg.embed_dim
    sizes = {"patch_embed": n * n * E, "down0.block0": n * n * E, "down0": (n // 2) ** 2 * 2 * E, "down1.block0": (n // 2) ** 2 * 2 * E}
    sc = (sc_adj, sc_node) if self_cond else (None, None)
    _, _, taps = Oracle(cfg, W.synth_state_dict(cfg, 0)).forward(adj, node, flags, np.asarray([0.4, 0.4], np.float32), *sc, taps=dict(sizes))
    for name, k in (("patch_embed", 0), ("down0.block0", 0), ("down0", 1), ("down1.block0", 1)):
        res = n >> k
        nwr, side = res // WS, WS << k
        x = window_rows(taps[name], 2, res, E << k)
        blk = flags[0].reshape(nwr, side).any(axis=1)
        pure = np.flatnonzero(~(blk[:, None] & blk[None, :]).reshape(-1))
        assert 0 < len(pure) < nwr * nwr and not np.array_equal(x[0, 0], x[0, pure[0]]), "window 0 of the mixed graph holds valid pairs"
        for w in range(nwr * nwr):
            assert np.array_equal(x[1, w], x[0, pure[0]]), f"{name}: window {w} of the all-padding graph differs from a pure window of the mixed graph"
