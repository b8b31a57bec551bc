"""Option "dedup_qkv" (include/dsg.h): the shifted block behind a deduplicated first block projects QKV of the copied
pure-window rows once.

Behind the fill every pure window of a content class holds the same 64 rows and row statistics, and the QKV projection is row-wise.
Where the distinct rows -- the non-pure windows plus one source pure window per class -- are at most half of all rows
(qk_split_rule), the block runs the projection over the list `qk_runs` and an attention kernel that reads q, k, v through the window
map `qk_src`; otherwise the fused kernel over all rows.  The device picks the form from the staged lists.  Bit-identity rests on
(a) copied rows and statistics being bit-equal, (b) the list GEMM's K order and bias add being the fused kernel's, (c) the attention
phase being the fused kernel's text: all three are held here by torch.equal between "dedup_qkv" 1 and 0, with no tolerance.

CPU: the rule restated in NumPy (lists, map, flag) on the three geometries, and the library's host restatement of the flag.
GPU: the device lists against that rule (the list program runs inside need_lists_kernel; a sampler call stages it), forward and
  sampler outputs under every staging mode with the form the last forward took read back, and one captured step body replayed with
  flag sets that switch the form.
"""
import numpy as np
import pytest

from diffusesg_amd import lib
from diffusesg_amd import spec as S
from diffusesg_amd import weights as W

WS = 8
STEPS = 6
# name -> (configuration, level whose second block is the shifted one behind a deduplicated first block)
#   "n32": N = 32, depths (1, 2): level 1 on a 2 x 2 window grid at C = 192; every shifted window mixes listed and copied rows
#   "d2":  N = 64, depths (1, 2, 1): level 1 on a 4 x 4 grid
#   "vg":  the headline network, depths (1, 1, 3, 1): level 2 on a 2 x 2 grid at C = 384
_specs = {"n32": (lambda: S.ModelConfig(max_node_num=32, c_adj=3, c_node=5, depths=(1, 2), num_heads=(3, 6), window_size=8,
                                        self_condition=True), 1),
          "d2": (lambda: S.ModelConfig(max_node_num=64, c_adj=3, c_node=5, depths=(1, 2, 1), num_heads=(3, 6, 12), window_size=8,
                                       self_condition=True), 1),
          "vg": (lambda: S.vg_config(), 2)}
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


# ---- the rule, restated ------------------------------------------------------------------------------------------------------
def expected(flags, level, mode):
    """mode: 0 every window listed, 1 one source pure window per graph (its first), 2 / 3 one for the batch (the first pure window in
    (graph, window) order).  Returns the listed runs (sorted), the window map [B * nW] and the flag."""
    B, n = flags.shape
    side, res = WS << level, n >> level
    nwr = res // WS
    nW = nwr * nwr
    pure = np.zeros((B, nW), bool)
    if mode != 0:
        for b, f in enumerate(flags):
            pure[b] = ~np.outer(f, f).reshape(nwr, side, nwr, side).any(axis=(1, 3)).reshape(-1)
    first = [int(np.flatnonzero(p)[0]) + b * nW if p.any() else -1 for b, p in enumerate(pure)]
    batch_first = min([x for x in first if x >= 0], default=-1)
    src = np.zeros(B * nW, np.int64)
    for b in range(B):
        cls = batch_first if mode >= 2 else first[b]
        for w in range(nW):
            src[b * nW + w] = cls if pure[b, w] else b * nW + w
    listed = sorted(set(src.tolist()))
    runs = sorted((w // nW) * res * nwr + (((w % nW) // nwr) * WS + p) * nwr + (w % nwr) for w in listed for p in range(WS))
    return dict(runs=np.array(runs, np.int64), src=src, split=len(runs) > 0 and 2 * 8 * len(runs) <= B * res * res, pure=pure)


def flag_sets(n, B=4):
    """name -> flags [B, n]: the headline's 30 / 64 valid nodes scaled to n, scattered flags, an all-false next to an all-true graph, and
    batches that mix graphs below and above half of n so that the listed share falls on either side of the rule's bound"""
    lo, lo2 = 15 * n // 32, 10 * n // 32
    scattered = np.zeros((B, n), bool)
    scattered[0, [1, 3, n // 4 + 1]] = True
    scattered[1 % B, [n // 2 + 1]] = True
    scattered[2 % B, [0, n - 1]] = True
    d = {"prefix": W.synth_flags(B, n, [lo] * B),
         "scattered": scattered,
         "none_and_all": W.synth_flags(B, n, ([0, n, lo, lo2] * B)[:B]),
         "mostly_below": W.synth_flags(B, n, ([lo, 0, 0, n] * B)[:B]),
         "mostly_above": W.synth_flags(B, n, ([lo, n, n, lo2] * B)[:B] if B > 1 else [n])}   # (a single graph: no pure window)
    return d


def test_the_restated_rule():
    L = lib.load()
    # the headline: 64 graphs of 30 valid nodes, level 2 (2 x 2 windows of 32 nodes), one source for the batch: 64 x 64 rows of the
    # non-pure windows + 64 rows of one pure window
    e = expected(W.synth_flags(64, 64, [30] * 64), 2, 2)
    assert 8 * len(e["runs"]) == 4160 and e["split"]
    assert not expected(W.synth_flags(64, 64, [30] * 64), 2, 0)["split"]       # every window listed: the fused form
    assert not expected(W.synth_flags(64, 64, [33] * 64), 2, 2)["split"]       # no pure window at level 2
    rng = np.random.RandomState(5)
    both = set()
    for name, (mk, level) in _specs.items():
        n = mk().max_node_num
        res = n >> level
        nW = (res // WS) ** 2
        sets = dict(flag_sets(n, 4))
        sets.update({f"b3_{k}": v for k, v in flag_sets(n, 3).items()}, b1=flag_sets(n, 1)["prefix"],
                    random=rng.rand(5, n) < 0.15, random_dense=rng.rand(5, n) < 0.6)
        for key, flags in sets.items():
            B = len(flags)
            for mode in (0, 1, 2, 3):
                e = expected(flags, level, mode)
                listed = set()   # windows of the listed runs
                for r in e["runs"].tolist():
                    b, t = divmod(r, res * (res // WS))
                    i, jr = divmod(t, res // WS)
                    listed.add(b * nW + (i // WS) * (res // WS) + jr)
                assert len(e["runs"]) == 8 * len(listed)
                pure = e["pure"].reshape(-1)
                for w in range(B * nW):
                    s = int(e["src"][w])
                    assert s in listed, f"{name} {key} mode {mode}: window {w} reads q, k, v of a window nobody projects"
                    assert s == w or (pure[w] and pure[s]), "only a pure window reads another window, and that one is pure"
                    if mode == 1:
                        assert s // nW == w // nW, "per graph: the (scale, shift) rows differ between graphs"
                assert all(int(e["src"][w]) == w for w in listed)
                assert L.dsg_debug_qk_split(len(e["runs"]), B * res * res) == int(e["split"])
                both.add(bool(e["split"]))
                if mode == 0:
                    assert len(listed) == B * nW and not e["split"]
    assert both == {True, False}
    assert L.dsg_debug_qk_split(0, 1024) == 0 and L.dsg_debug_qk_split(64, 1024) == 1 and L.dsg_debug_qk_split(65, 1024) == 0


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def T(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def sample_case(cfg, flags, seed, tag):
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


DEFAULTS = dict(fused_merge=1, dedup_batch=1, dedup_table=1, dedup_qkv=1, loop_graph=1)
# staging mode -> options ("fused_merge" 2: the partial-statistics PatchMerging at every size, without which the levels above 0 do not
# deduplicate at these batch sizes) and the DedupMode the lists are written for
STAGING = {"graph": (dict(fused_merge=2, dedup_batch=0), 1),
           "batch": (dict(fused_merge=2, dedup_batch=2, dedup_table=0), 2),
           "table": (dict(fused_merge=2, dedup_batch=2, dedup_table=1), 3)}


def restore(h):
    for k, v in DEFAULTS.items():
        h.set_option(k, v)


def check_lists(h, flags, level, mode, tag):
    B = len(flags)
    assert h.dedup_launch_lists(B, level)["mode"] == mode, f"{tag}: lists staged for another mode"
    got, exp = h.dedup_qkv_lists(B, level), expected(flags, level, mode)
    assert got is not None, f"{tag}: no qk lists"
    assert len(set(got["runs"].tolist())) == len(got["runs"]), f"{tag}: duplicate runs"
    assert np.array_equal(np.sort(got["runs"]), exp["runs"]), f"{tag}: qk_runs differs from the rule"
    assert np.array_equal(got["src"], exp["src"]), f"{tag}: qk_src differs from the rule"
    assert got["split"] == exp["split"], f"{tag}: the flag differs from the rule"
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name,B", [("n32", 1), ("n32", 3), ("n32", 4), ("n32", 16), ("d2", 3), ("d2", 4), ("vg", 3), ("vg", 4)])
@pytest.mark.parametrize("staging", ["graph", "batch", "table"])
def test_sampler_bit_identical_and_lists_match_the_rule(name, B, staging):
    import torch
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    cfg, net, level = cfg_for(name), net_for(name), _specs[name][1]
    h = net.model._ensure_handle()
    opts, mode = STAGING[staging]
    smp = NodeAdjEDMSamplerHip(num_steps=STEPS, self_condition=True, dev="cuda")
    cases = {k: (f, sample_case(cfg, f, 61, f"dedup_qkv/{name}/{B}/{k}")) for k, f in flag_sets(cfg.max_node_num, B).items()}
    try:
        for k, v in opts.items():
            h.set_option(k, v)
        h.set_option("dedup_qkv", 0)
        assert h.get_option("dedup_qkv") == 0
        ref = {}
        for k, (f, c) in cases.items():
            ref[k] = run(smp, net, cfg, c)
            assert h.dedup_qkv_lists(B, level)["form"] is None, "option off: the block runs without the switch"
        h.set_option("dedup_qkv", 1)
        assert h.get_option("dedup_qkv") == 1
        forms = set()
        for k, (f, c) in cases.items():
            got = run(smp, net, cfg, c)
            lists = check_lists(h, f, level, mode, f"{name} B={B} {staging} {k}")
            assert lists["form"] == ("split" if lists["split"] else "fused"), f"{k}: the forward did not take the switched block"
            forms.add(lists["form"])
            assert torch.equal(got[0], ref[k][0]) and torch.equal(got[1], ref[k][1]), f"{name} B={B} {staging} {k} ({lists['form']}): sample differs"
        assert forms == {"split", "fused"}, f"forms taken: {forms}"
    finally:
        restore(h)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n32", "d2", "vg"])
def test_denoise_on_unmasked_caller_tensors_keeps_the_fused_form(name):
    import torch
    cfg, net, level = cfg_for(name), net_for(name), _specs[name][1]
    n, B = cfg.max_node_num, 3
    flags = W.synth_flags(B, n, [15 * n // 32, 3, 0])
    args = [W.normal(7, f"dedup_qkv/denoise/{name}/{t}", shp) for t, shp in
            (("adj", (B, cfg.c_adj, n, n)), ("node", (B, n, cfg.c_node)), ("sc_adj", (B, cfg.c_adj, n, n)), ("sc_node", (B, n, cfg.c_node)))]
    c_noise = np.array([-1.2, 0.2, 1.0], np.float32)
    call = (T(args[0]), T(args[1]), T(flags), T(c_noise), T(args[2]), T(args[3]))   # not masked: non-zero at padded pairs
    h = net.model._ensure_handle()
    try:
        h.set_option("fused_merge", 2)
        h.set_option("dedup_qkv", 0)
        ref = [t.clone() for t in net.model(*call)]
        assert h.dedup_qkv_lists(B, level)["form"] is None
        h.set_option("dedup_qkv", 1)
        got = [t.clone() for t in net.model(*call)]
        lists = check_lists(h, flags, level, 0, f"{name} denoise")
        assert lists["form"] == "fused" and not lists["split"] and len(lists["runs"]) == B * (n >> level) ** 2 // 8
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
        # the measurement hook ("dedup_qkv" 2: the split form whatever the share): every window is listed and maps to itself
        h.set_option("dedup_qkv", 2)
        assert h.get_option("dedup_qkv") == 2
        got = [t.clone() for t in net.model(*call)]
        lists = check_lists(h, flags, level, 0, f"{name} denoise, split forced")
        assert lists["form"] == "split" and not lists["split"]
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    finally:
        restore(h)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n32", "vg"])
def test_one_captured_step_body_replayed_with_flag_sets_that_switch_the_form(name):
    """Both forms' launches sit in every captured body and the device picks one from the lists of the call: graphs captured under a
    flag set of one form, replayed under sets of the other form and back, against eager runs of the same calls."""
    import torch
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    cfg, net, level = cfg_for(name), net_for(name), _specs[name][1]
    B = 4
    h = net.model._ensure_handle()
    smp = NodeAdjEDMSamplerHip(num_steps=STEPS, self_condition=True, dev="cuda")
    sets = flag_sets(cfg.max_node_num, B)
    order = ["mostly_above", "prefix", "none_and_all", "mostly_below", "mostly_above", "scattered"]
    cases = {k: sample_case(cfg, sets[k], 67, f"dedup_qkv/replay/{name}/{k}") for k in set(order)}
    try:
        for k, v in STAGING["batch"][0].items():
            h.set_option(k, v)
        h.set_option("dedup_qkv", 1)
        h.set_option("loop_graph", 0)
        eager = {k: run(smp, net, cfg, c) for k, c in cases.items()}
        h.set_option("loop_graph", 1)    # drops nothing that exists; the first call below captures, the others replay
        forms = []
        for k in order:
            got = run(smp, net, cfg, cases[k])
            forms.append(h.dedup_qkv_lists(B, level)["form"])
            assert torch.equal(got[0], eager[k][0]) and torch.equal(got[1], eager[k][1]), f"{name} {k} ({forms[-1]}): replay differs from eager"
        assert forms[0] == "fused" and "split" in forms[1:4] and forms[4] == "fused", forms
    finally:
        restore(h)
