"""GPU: pure-window deduplication one and two levels up (option "dedup_levels", include/dsg.h).

A pure window of level k lies over 2 x 2 pure windows of level k - 1, PatchMerging is a row-wise function of the 2 x 2 fine rows and an
unshifted block sees positions only inside its window: every pure window of level 1, and of level 2, leaves the merge and the level's
first block with the same 64 rows.  The library computes the unique windows' rows (PatchMerging over a run list, the first block over
the same lists) and fills the others by copy: activation, skip tensor and row statistics.  All checks go through the C ABI and use no
tolerance:
  1. sampler outputs are bit-identical (torch.equal) between "every level", "level 0 only" (the previous behaviour) and
     "dedup_masked" = 0 -- Heun + churn with self-conditioning coins, step graphs captured under one flag pattern and replayed under
     the others, the workspace poisoned by a full-flag run in between, valid counts at every edge at which a list of some level changes
     shape, batches whose run counts are no multiple of a 16-run tile, scattered flags, flags without a pure window; with the
     PatchMerging a small batch takes by default (merge_ln: the levels above 0 do not qualify) and with the partial-statistics form of
     the headline batch ("fused_merge" 2, once through "batch_invariant"), whose "level 0 only" run is the gather GEMM -- so equality
     there is the run-list merge against the gather form, bit for bit;
  2. the conditioned and seeded sampler flavours with caller tensors that are non-zero at padded pairs;
  3. dsg_denoise takes caller tensors and deduplicates nothing, at any level.
"""
import numpy as np
import pytest
import torch

from diffusesg_amd import spec as S
from diffusesg_amd import weights as W

pytestmark = pytest.mark.gpu

STEPS = 6
# name -> (configuration, levels that deduplicate where PatchMerging takes its partial-statistics form)
#   "vg":  the headline network, depths (1, 1, 3, 1): levels 1 (4 x 4 windows) and 2 (2 x 2), a shifted block behind level 2's first;
#          level 3 is one window and has nothing to share
#   "d2":  N = 64, depths (1, 2, 1): a shifted block on a 4 x 4 window grid right behind level 1's deduplicated one -- it mixes
#          neighbouring windows, so behind it pure windows differ and the chain ends: level 2 does not deduplicate
#   "s":   N = 32, depths (1, 1, 1): level 1 on a 2 x 2 window grid; level 2 is one window
_specs = {"vg": (lambda: S.vg_config(), 3),
          "d2": (lambda: S.ModelConfig(max_node_num=64, c_adj=3, c_node=5, depths=(1, 2, 1), num_heads=(3, 6, 12), window_size=8,
                                       self_condition=True), 2),
          "s": (lambda: S.ModelConfig(max_node_num=32, c_adj=3, c_node=5, depths=(1, 1, 1), num_heads=(3, 6, 12), window_size=8,
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
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def set_mode(net, mode):
    """mode: "off" (dedup_masked 0), "l0" (level 0 only), "all" (every qualifying level)"""
    h = net.model._ensure_handle()
    h.set_option("prune_masked", 1)
    h.set_option("dedup_masked", int(mode != "off"))
    h.set_option("dedup_levels", 1 if mode == "l0" else 0)
    assert h.get_option("dedup_masked") == int(mode != "off")   # still 0 / 1
    return h


def prefix(n, valid):
    return W.synth_flags(len(valid), n, valid)


def batches(n):
    """name -> flags [B <= 4, n].  Prefix counts (cut off at n) on either side of every window edge of levels 0, 1 and 2 (8, 16, 32
    nodes), the headline's 30, nothing and everything; "uneven": graphs with different numbers of unique windows, chosen so that the
    run lists of the coarser levels are no whole number of 16-run tiles (checked by the caller) and end in sentinel runs."""
    v = (lambda *c: [min(n, x) for x in c])
    scattered = np.zeros((3, n), bool)
    scattered[0, [9, 10, n - 20]] = True
    scattered[1, [n // 2 + 1]] = True
    scattered[2, [0, n - 1]] = True
    no_pure = np.zeros((2, n), bool)
    no_pure[0, ::8] = True
    no_pure[1, 7::8] = True
    d = {
        "edges_a": prefix(n, v(0, 1, 15, 16)),
        "edges_b": prefix(n, v(17, 30, 31, 32)),
        "edges_c": prefix(n, v(33, 48, 49, 64)),
        "scattered": scattered,
        "no_pure": no_pure,
        "one_of_four": prefix(n, [n, n, v(30)[0], n]),   # only graph 2 has pure windows
    }
    if n == 64:
        d["uneven_a"] = prefix(n, [30, 5, 64])           # level 1: 5 + 2 + 16 unique windows
        d["uneven_b"] = prefix(n, [30, 0, 64])           # level 2: 2 + 1 + 4
    else:
        d["uneven_a"] = prefix(n, [5, 0, 32])            # level 1: 2 + 1 + 4
    return d


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
    out = smp.sample(net, case["flags"], init_adjs=case["init_adjs"], init_nodes=case["init_nodes"], churn_noise=case["churn_noise"],
                     coins=case["coins"], num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj)
    return [torch.as_tensor(t).clone() for t in out]


# merge: the "fused_merge" option (1: the default -- merge_ln at these batch sizes; 2: the partial-statistics form at every size);
# invariant: "batch_invariant" 1 selects that form by itself, with "fused_merge" left at its default
@pytest.mark.parametrize("name,merge,invariant", [("vg", 2, 0), ("vg", 1, 0), ("vg", 1, 1), ("d2", 2, 0), ("d2", 1, 0), ("s", 2, 0), ("s", 1, 0)])
def test_sampler_bit_identical_at_every_depth_of_deduplication(name, merge, invariant):
    cfg, net = cfg_for(name), net_for(name)
    h = net.model._ensure_handle()
    h.set_option("fused_merge", merge)
    h.set_option("batch_invariant", invariant)
    try:
        sampler_modes(name, cfg, net, deep=(merge == 2 or invariant == 1))
    finally:
        h.set_option("fused_merge", 1)
        h.set_option("batch_invariant", 0)
        set_mode(net, "all")


def sampler_modes(name, cfg, net, deep):
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    n = cfg.max_node_num
    planned = _specs[name][1]                 # what the option reports: levels that deduplicate where PatchMerging has its partial-statistics form
    levels = planned if deep else 1           # ... and what these batch sizes do in mode "all" (merge_ln ends the chain behind level 0)
    smp = NodeAdjEDMSamplerHip(num_steps=STEPS, self_condition=True, dev="cuda")   # Heun + churn, hipGraph on
    cases = {k: sample_case(cfg, f, 47, f"dedup_levels/{name}/{k}") for k, f in batches(n).items()}
    poison = {B: sample_case(cfg, np.ones((B, n), bool), 49, f"dedup_levels/{name}/poison{B}") for B in {len(f) for f in batches(n).values()}}
    set_mode(net, "off")
    ref = {k: run(smp, net, cfg, c) for k, c in cases.items()}
    for mode in ("l0", "all"):
        h = set_mode(net, mode)
        assert h.get_option("dedup_levels") == (planned if mode == "all" else 1)
        copied = [0, 0, 0]
        partial_tiles = set()
        for k, c in cases.items():
            # a full-flag run first: it (re)captures nothing after the first time, rewrites every activation row of the workspace with
            # other values, and leaves step graphs that the next call replays with other lists
            B = c["flags"].shape[0]
            run(smp, net, cfg, poison[B])
            for lv in range(3):
                d = h.dedup_level_lists(B, lv)
                assert d is None or len(d["copy"]) == 0, "all-true flags have no pure window"
            got = run(smp, net, cfg, c)
            assert torch.equal(got[0], ref[k][0]) and torch.equal(got[1], ref[k][1]), f"{name} {mode} {k}: deduplicated sample differs"
            for lv in range(3):
                d = h.dedup_level_lists(B, lv)
                on = lv < (levels if mode == "all" else 1)
                if d is None:
                    assert not on
                    continue
                assert (d["fwd"] >= 0) == on, f"{name} {mode} {k}: level {lv} {'not ' if on else ''}deduplicated by the forward"
                if on:
                    copied[lv] += len(d["copy"])
                    if lv > 0 and len(d["runs"]) % 16 != 0:
                        partial_tiles.add(lv)
                    # the copy also moved the row statistics wherever the next launch reads them: the pre-modulated rows' LN1
                    # partials for a following block, the output rows' partials for the next partial-statistics merge
                    if lv > 0:
                        assert d["fwd"] == 1
        for lv in range(levels if mode == "all" else 1):
            assert copied[lv] > 0, f"{name} {mode}: nothing was filled at level {lv}"
        if mode == "all" and levels > 1:
            assert partial_tiles == set(range(1, levels)), "no run list with a partial last tile (sentinel runs) at some level"


def test_known_values_and_base_at_padded_pairs():
    """Every sampler flavour deduplicates at every level: the known-entry select, the partial-noise start and the seeded streams all
    store `valid ? ... : 0` themselves.  Here the caller's known tensors, masks and base are non-zero at padded pairs as well."""
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    cfg, net = cfg_for("vg"), net_for("vg")
    n, B = cfg.max_node_num, 3
    flags = T(prefix(n, [n // 2 - 1, 3, 9]))
    ka = T(W.normal(9, "dedup_levels/known/adj", (B, cfg.c_adj, n, n)))           # none of these is masked
    kn = T(W.normal(9, "dedup_levels/known/node", (B, n, cfg.c_node)))
    ba = T(W.normal(9, "dedup_levels/base/adj", (B, cfg.c_adj, n, n)))
    bn = T(W.normal(9, "dedup_levels/base/node", (B, n, cfg.c_node)))
    ma = T(W.normal(9, "dedup_levels/known/mask_adj", (B, cfg.c_adj, n, n)) > 0.3)   # known entries everywhere, padded pairs included
    mn = T(W.normal(9, "dedup_levels/known/mask_node", (B, n, cfg.c_node)) > 0.3)
    smp = NodeAdjEDMSamplerHip(num_steps=STEPS, self_condition=True, dev="cuda")
    L = STEPS - 2
    coins = (W.coins(9, "dedup_levels/known", 2 * L - 1) < 0.5).astype(np.uint8)
    kw = dict(num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj)

    def calls():
        out = [smp.sample_known(net, flags, ka, kn, ma, mn, seed=31, coins=coins, start_step=2, base_adjs=ba, base_nodes=bn, **kw),
               smp.sample(net, flags, graph_seeds=[5, 2 ** 40 + 1, 77], coin_seed=3, **kw)]
        return [torch.as_tensor(t).clone() for o in out for t in o]
    h = net.model._ensure_handle()
    h.set_option("fused_merge", 2)
    try:
        set_mode(net, "off")
        ref = calls()
        set_mode(net, "l0")
        got0 = calls()
        h = set_mode(net, "all")
        got = calls()
        for lv in range(3):
            d = h.dedup_level_lists(B, lv)
            assert len(d["copy"]) > 0 and d["fwd"] >= 0
        for g, g0, r in zip(got, got0, ref):
            assert torch.equal(g, r) and torch.equal(g0, r)
    finally:
        h.set_option("fused_merge", 1)


def test_denoise_with_caller_tensors_is_not_deduplicated_at_any_level():
    """dsg_denoise: the adjacency is the caller's and the reference does not mask it on entry -- here it is non-zero at padded pairs,
    so pure windows do NOT share their rows.  The option is on, the call stages lists that name every window of every level as unique."""
    cfg, net = cfg_for("d2"), net_for("d2")
    n, B = cfg.max_node_num, 3
    flags = prefix(n, [n // 2 - 1, 3, 0])
    adj = W.normal(7, "dedup_levels/denoise/adj", (B, cfg.c_adj, n, n))   # not masked
    node = W.normal(7, "dedup_levels/denoise/node", (B, n, cfg.c_node))
    sc_adj = W.normal(7, "dedup_levels/denoise/sc_adj", (B, cfg.c_adj, n, n))
    sc_node = W.normal(7, "dedup_levels/denoise/sc_node", (B, n, cfg.c_node))
    c_noise = np.array([-1.2, 0.2, 1.0], np.float32)
    args = (T(adj), T(node), T(flags), T(c_noise), T(sc_adj), T(sc_node))
    h = net.model._ensure_handle()
    h.set_option("fused_merge", 2)
    try:
        set_mode(net, "off")
        ref = [t.clone() for t in net.model(*args)]
        h = set_mode(net, "all")
        got = [t.clone() for t in net.model(*args)]
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
        assert h.get_option("dedup_levels") == 2
        assert h.dedup_level_lists(B, 2) is None   # the chain ends behind level 1's shifted block ("d2" above): no lists for level 2
        for lv in range(2):
            d = h.dedup_level_lists(B, lv)
            nw = ((n >> lv) // 8) ** 2
            assert len(d["copy"]) == 0 and len(d["wins"]) == B * nw and len(d["runs"]) == B * nw * 8 and (d["rep"] == -1).all()
    finally:
        h.set_option("fused_merge", 1)
