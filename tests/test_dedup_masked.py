"""GPU: pure-window deduplication of the down path (option "dedup_masked", include/dsg.h).

In the sampler every network input is zero at a token (i, j) with a padded endpoint, so all 8 x 8 level-0 windows made of such
tokens leave PatchEmbed and the first Swin block with the same rows; the library computes one of them per graph and copies it.
Checked here, all through the C ABI and without any tolerance:
  1. sampler outputs are bit-identical (torch.equal) to the same handle with the option off -- Heun + churn with self-conditioning
     coins, step graphs captured under one flag pattern and replayed under others, the workspace poisoned by a full-flag run, valid
     counts at every edge where the lists change shape, scattered flags, flags without a pure window, mixed batches; each with the
     PatchMerging the small batch takes (merge_ln) and with the fused one the headline batch takes, which reads the copied partials;
     and the conditioned / partially-noised / seeded sampler flavours with caller tensors that are non-zero at padded pairs;
  2. dsg_denoise takes caller tensors (here: non-zero adjacency at padded pairs) and deduplicates nothing;
  3. dsg_get_option("dedup_masked") reports 0 in every condition in which the option does not act.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from diffusesg_amd import spec as S
from diffusesg_amd import synth as Y
from diffusesg_amd import weights as W

pytestmark = pytest.mark.gpu

STEPS = 6
# "vg": the headline network (N = 64: 8 x 8 windows at level 0, 4 x 4 at level 1); "s": the smallest synthetic configuration that still
# has two window rows at two consecutive levels (N = 32: 4 x 4 and 2 x 2)
_cfgs, _nets = {}, {}


def cfg_for(name):
    if name not in _cfgs:
        _cfgs[name] = S.vg_config() if name == "vg" else S.ModelConfig(max_node_num=32, c_adj=3, c_node=5, depths=(1, 1, 1),
                                                                       num_heads=(3, 6, 12), window_size=8, self_condition=True)
    return _cfgs[name]


def net_for(name):
    from diffusesg_amd.model import build_network
    if name not in _nets:
        cfg = cfg_for(name)
        _nets[name] = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")
    return _nets[name]


def T(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def set_dedup(net, on):
    h = net.model._ensure_handle()
    h.set_option("prune_masked", 1)
    h.set_option("dedup_masked", int(on))
    assert h.get_option("dedup_masked") == int(on)
    return h


def prefix(n, valid):
    return W.synth_flags(len(valid), n, valid)


def batches(n):
    """name -> flags [B <= 4, n].  Prefix counts (cut off at n): every count at which a list changes shape -- nothing valid, one node,
    either side of one window row, of two, of half of N = 64, the headline's 30, everything."""
    v = (lambda *c: [min(n, x) for x in c])
    scattered = np.zeros((3, n), bool)
    scattered[0, [9, 10, n - 20]] = True          # window rows / columns 1 and (n - 20) / 8 valid: pure windows on all sides, none needed in a corner
    scattered[1, [n // 2 + 1]] = True             # a single valid node in the middle
    scattered[2, [0, n - 1]] = True               # the four corner windows are the non-pure ones
    no_pure = np.zeros((2, n), bool)
    no_pure[0, ::8] = True                        # one valid node in every block of 8: no pure window at all
    no_pure[1, 7::8] = True
    return {
        "edges_a": prefix(n, v(0, 1, 7, 8)),
        "edges_b": prefix(n, v(9, 16, 17, 30)),
        "edges_c": prefix(n, v(32, 33, 64)),
        "scattered": scattered,
        "no_pure": no_pure,
        "one_of_four": prefix(n, [n, n, v(30)[0], n]),   # only graph 2 has pure windows
    }


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


# merge: the "fused_merge" option.  1 (the default) fuses PatchMerging from 8192 merged rows on -- B = 64 at N = 64, never at B <= 4 -- and
# below that level 0's block leaves no LayerNorm partials; 2 fuses at every size, which is the path of the headline batch: the block
# leaves (sum, sumsq) pairs in the workspace, the copy has to move them with the rows, and the fused merge reads both for the copied windows
@pytest.mark.parametrize("name,merge", [("vg", 1), ("vg", 2), ("s", 1), ("s", 2)])
def test_sampler_bit_identical_to_full_down_path(name, merge):
    cfg, net = cfg_for(name), net_for(name)
    h = net.model._ensure_handle()
    h.set_option("fused_merge", merge)
    try:
        sampler_on_vs_off(name, cfg, net, merge)
    finally:
        h.set_option("fused_merge", 1)


def sampler_on_vs_off(name, cfg, net, merge):
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    n = cfg.max_node_num
    smp = NodeAdjEDMSamplerHip(num_steps=STEPS, self_condition=True, dev="cuda")   # Heun + churn, hipGraph on
    cases = {k: sample_case(cfg, f, 41, f"dedup/{name}/{k}") for k, f in batches(n).items()}
    poison = {B: sample_case(cfg, np.ones((B, n), bool), 43, f"dedup/{name}/poison{B}") for B in {len(f) for f in batches(n).values()}}
    set_dedup(net, 0)
    ref = {k: run(smp, net, cfg, c) for k, c in cases.items()}
    h = set_dedup(net, 1)
    copied = 0
    for k, c in cases.items():
        # a full-flag run first: it (re)captures nothing after the first time, rewrites every activation row of the workspace with
        # other values, and leaves step graphs that the next call replays with other lists
        B = c["flags"].shape[0]
        run(smp, net, cfg, poison[B])
        assert len(h.dedup_lists(B)["copy"]) == 0, "all-true flags have no pure window"
        got = run(smp, net, cfg, c)
        copied += len(h.dedup_lists(B)["copy"])
        # the copy moved what the consumer reads: rows alone in front of merge_ln, rows and their partials in front of the fused merge
        assert h.dedup_lists(B)["fwd"] == (1 if merge == 2 else 0), f"{name} merge={merge}: the partials were {'not ' if merge == 2 else ''}copied"
        assert torch.equal(got[0], ref[k][0]) and torch.equal(got[1], ref[k][1]), f"{name} {k}: deduplicated sample differs"
        if k == "no_pure":
            assert len(h.dedup_lists(B)["copy"]) == 0
    assert copied > 0, "nothing was deduplicated"


def test_known_values_and_base_at_padded_pairs():
    """Every sampler flavour deduplicates: the known-entry select, the partial-noise start and the seeded streams all store
    `valid ? ... : 0` themselves.  Here the caller's known tensors, masks and base are non-zero at padded pairs as well."""
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    cfg, net = cfg_for("s"), net_for("s")
    n, B = cfg.max_node_num, 3
    flags = T(prefix(n, [n // 2 - 1, 3, 9]))
    ka = T(W.normal(9, "dedup/known/adj", (B, cfg.c_adj, n, n)))           # none of these is masked
    kn = T(W.normal(9, "dedup/known/node", (B, n, cfg.c_node)))
    ba = T(W.normal(9, "dedup/base/adj", (B, cfg.c_adj, n, n)))
    bn = T(W.normal(9, "dedup/base/node", (B, n, cfg.c_node)))
    ma = T(W.normal(9, "dedup/known/mask_adj", (B, cfg.c_adj, n, n)) > 0.3)   # known entries everywhere, padded pairs included
    mn = T(W.normal(9, "dedup/known/mask_node", (B, n, cfg.c_node)) > 0.3)
    smp = NodeAdjEDMSamplerHip(num_steps=STEPS, self_condition=True, dev="cuda")
    L = STEPS - 2
    coins = (W.coins(9, "dedup/known", 2 * L - 1) < 0.5).astype(np.uint8)
    kw = dict(num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj)

    def calls():
        out = [smp.sample_known(net, flags, ka, kn, ma, mn, seed=31, coins=coins, start_step=2, base_adjs=ba, base_nodes=bn, **kw),
               smp.sample(net, flags, graph_seeds=[5, 2 ** 40 + 1, 77], coin_seed=3, **kw)]
        return [torch.as_tensor(t).clone() for o in out for t in o]
    set_dedup(net, 0)
    ref = calls()
    h = set_dedup(net, 1)
    got = calls()
    assert len(h.dedup_lists(B)["copy"]) > 0 and h.dedup_lists(B)["fwd"] == 0
    for g, r in zip(got, ref):
        assert torch.equal(g, r)


def test_denoise_with_caller_tensors_is_not_deduplicated():
    """dsg_denoise: the adjacency is the caller's and the reference does not mask it on entry -- here it is non-zero at padded pairs,
    so pure windows do NOT share their rows.  The option is on, the call stages lists that name every window as unique."""
    cfg, net = cfg_for("s"), net_for("s")
    n, B = cfg.max_node_num, 3
    flags = prefix(n, [n // 2 - 1, 3, 0])
    adj = W.normal(7, "dedup/denoise/adj", (B, cfg.c_adj, n, n))   # not masked
    node = W.normal(7, "dedup/denoise/node", (B, n, cfg.c_node))
    sc_adj = W.normal(7, "dedup/denoise/sc_adj", (B, cfg.c_adj, n, n))
    sc_node = W.normal(7, "dedup/denoise/sc_node", (B, n, cfg.c_node))
    c_noise = np.array([-1.2, 0.2, 1.0], np.float32)
    args = (T(adj), T(node), T(flags), T(c_noise), T(sc_adj), T(sc_node))
    set_dedup(net, 0)
    ref = [t.clone() for t in net.model(*args)]
    h = set_dedup(net, 1)
    got = [t.clone() for t in net.model(*args)]
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    d = h.dedup_lists(B)
    nw = (n // 8) ** 2
    assert len(d["copy"]) == 0 and len(d["wins"]) == B * nw and (d["rep"] == -1).all()


def test_get_option_reports_what_runs():
    from diffusesg_amd.model import build_network
    cfg = cfg_for("s")
    net = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")   # a handle of its own: no workspace yet, every option can be set
    h = set_dedup(net, 1)
    try:
        for opt, val, back in (("prune_masked", 0, 1), ("gemm_split", 1, 0), ("gemm_bf16", 1, 0), ("fused_attn", 0, 1), ("fused_mlp", 0, 1),
                               ("fused_patch_embed", 0, 1), ("dedup_masked", 0, 1)):
            h.set_option(opt, val)
            assert h.get_option("dedup_masked") == 0, f"{opt} = {val}: the deduplication cannot run"
            h.set_option(opt, back)
            assert h.get_option("dedup_masked") == 1
        # debug taps return whole tensors: off, as the pruning is
        buf = torch.zeros(4 * 32 * 32 * 96, device="cuda")
        h.check(h.L.dsg_debug_tap(h.raw, b"down0.block0", C.c_void_p(buf.data_ptr()), buf.numel()), "tap")
        assert h.get_option("dedup_masked") == 0
        h.L.dsg_debug_clear_taps(h.raw)
        assert h.get_option("dedup_masked") == 1
    finally:
        h.L.dsg_debug_clear_taps(h.raw)
        for opt, back in (("prune_masked", 1), ("gemm_split", 0), ("gemm_bf16", 0), ("fused_attn", 1), ("fused_mlp", 1), ("fused_patch_embed", 1)):
            h.set_option(opt, back)
    # windows other than 8 x 8: no lists at all
    tiny = Y.CONFIGS["tiny"]()
    tnet = build_network(tiny, W.synth_state_dict(tiny, 0), device="cuda")
    th = tnet.model._ensure_handle()
    th.set_option("dedup_masked", 1)
    assert th.get_option("dedup_masked") == 0
