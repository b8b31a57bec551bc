"""The list form of the fused read-out (include/dsg_debug.h: dsg_debug_readout_tiles): wherever the masked-token pruning
runs, it computes the 32-token tiles that hold a valid pair from a device-side list, packed four to a block at the front of its grid, and every wave writes the exact zeros of its own positional tile
where that tile holds none.  Tile t is tokens [32 t, 32 t + 32) of the flattened [B * N * N] index; it is listed iff one of its tokens
(b, i, j) has flag_i and flag_j.  Nothing in a tile's arithmetic or in the pooling slots changes, so everything here is torch.equal,
with no tolerance, to the same handle's positional form -- every wave deciding on its own tile, the launch that existed before the
list.  The library has no switch for the read-out alone: the positional form is what runs under "prune_masked" 0, where no launch
takes a list (tests/test_prune_masked.py holds the rest of that forward bit-identical to the pruned one).
  a. the device list is the NumPy restatement of the rule (itself checked on the host against a token-by-token loop), ascending, no
     duplicates;
  b. forward outputs (adj and node), with and without self-conditioning;
  c. the same after the scratch buffers (pool_part and the outputs among them) were filled with NaN and with 1e30: no tile and no
     pooling slot is left unwritten, and the adjacency output at masked pairs is exact zeros;
  d. one captured sampler body replayed under other flags with another count.
Shapes: a tile spans two grid rows (n = 16), one row (n = 32), half a row (n = 64, the headline's pattern) and 1 1/3 rows (n = 24,
N % 32 != 0: tiles straddle rows unevenly); B = 1 at n = 16 is a grid of two blocks.
"""
import numpy as np
import pytest
import torch

from diffusesg_amd import spec as S
from diffusesg_amd import synth as Y
from diffusesg_amd import weights as W

gpu = pytest.mark.gpu

SHAPES = {
    "n16": dict(n=16, depths=(1, 1), heads=(3, 6)),
    "n32": dict(n=32, depths=(1, 1, 1), heads=(3, 6, 12)),
    "n24": dict(n=24, depths=(1,), heads=(3,)),
    "vg": None,
}
CASES = [("n16", 1), ("n16", 2), ("n16", 3), ("n32", 1), ("n32", 2), ("n32", 3), ("n24", 1), ("n24", 2), ("n24", 3), ("vg", 2)]
_cfgs, _nets = {}, {}


def cfg_for(name):
    if name not in _cfgs:
        s = SHAPES[name]
        _cfgs[name] = S.vg_config() if s is None else S.ModelConfig(max_node_num=s["n"], c_adj=3, c_node=5, depths=s["depths"],
                                                                    num_heads=s["heads"], window_size=8, self_condition=True)
    return _cfgs[name]


def net_for(name):
    from diffusesg_amd.model import build_network
    if name not in _nets:
        cfg = cfg_for(name)
        _nets[name] = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")
    return _nets[name]


def T(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ---- the rule ----------------------------------------------------------------------------------------------------------------
def expected_tiles(flags):
    """ascending ids of the 32-token tiles of the flattened [B, n, n] index that hold a pair with flag_i and flag_j"""
    f = np.asarray(flags, bool)
    pair = (f[:, :, None] & f[:, None, :]).reshape(-1)
    pad = (-len(pair)) % 32
    return np.flatnonzero(np.concatenate([pair, np.zeros(pad, bool)]).reshape(-1, 32).any(axis=1)).astype(np.int32)


def prefix(n, B, valid):
    """graph b has its first valid[b] nodes (graphs beyond the list: none)"""
    f = np.zeros((B, n), bool)
    for b, v in enumerate(valid[:B]):
        f[b, :v] = True
    return f


def count_prefixes(n):
    """count -> the shortest prefix v of one graph of n nodes whose tile count is that, for 1, 2, 3 and 5 working tiles: a partly
    filled last working block in each of its three ways, and the same with a full block in front of it"""
    out = {}
    for v in range(1, n + 1):
        out.setdefault(len(expected_tiles(prefix(n, 1, [v]))), v)
    assert all(c in out for c in (1, 2, 3, 5)), (n, sorted(out))
    return {c: out[c] for c in (1, 2, 3, 5)}


def flag_patterns(n, B):
    """name -> flags [B, n]"""
    pats = {"ragged": prefix(n, B, [n // 2 - 1, 3, n]), "full": np.ones((B, n), bool), "none": np.zeros((B, n), bool)}
    scattered = np.zeros((B, n), bool)
    scattered[:, [1, 9, 10]] = True
    scattered[B - 1] = False
    scattered[B - 1, n - 2] = True
    pats["scattered"] = scattered
    empty = prefix(n, B, [n // 2 + 1, n - 3, 5])
    empty[B // 2] = False   # one all-false graph (B = 1: the whole batch)
    pats["empty"] = empty
    for c, v in count_prefixes(n).items():   # graph 0 alone holds the working tiles: the batch's count is c
        pats[f"count{c}"] = prefix(n, B, [v])
    return pats


def test_rule_restatement_on_the_host():
    for n, B in ((16, 1), (16, 3), (24, 2), (32, 2), (64, 2)):
        for name, flags in flag_patterns(n, B).items():
            want = set()
            for b in range(B):
                for i in range(n):
                    for j in range(n):
                        if flags[b, i] and flags[b, j]:
                            want.add(((b * n + i) * n + j) // 32)
            got = expected_tiles(flags)
            assert list(got) == sorted(want), (n, B, name)
            if name.startswith("count"):
                assert len(got) == int(name[5:])
        assert len(expected_tiles(np.zeros((B, n), bool))) == 0
        assert len(expected_tiles(np.ones((B, n), bool))) == B * n * n // 32
    # the headline: 30 valid of 64 nodes, 64 graphs -- the j < 32 half of rows i < 30, 1920 of 8192 tiles
    assert len(expected_tiles(prefix(64, 64, [30] * 64))) == 1920


# ---- the device ----------------------------------------------------------------------------------------------------------------
def set_list(net, on):
    """on: the pruning and with it the read-out's list form; off: the unpruned forward, whose read-out is the positional form"""
    h = net.model._ensure_handle()
    h.set_option("prune_masked", int(on))
    assert h.get_option("prune_masked") == int(on)
    return h


def inputs(cfg, flags, seed, tag):
    B, n = flags.shape
    adj = W.mask_adj(W.normal(seed, f"{tag}/adj", (B, cfg.c_adj, n, n)), flags)
    node = W.mask_node(W.normal(seed, f"{tag}/node", (B, n, cfg.c_node)), flags)
    sc_adj = W.mask_adj(W.normal(seed, f"{tag}/sc_adj", (B, cfg.c_adj, n, n)), flags)
    sc_node = W.mask_node(W.normal(seed, f"{tag}/sc_node", (B, n, cfg.c_node)), flags)
    return adj, node, sc_adj, sc_node


def forward_fn(net, cfg, flags, seed, tag, sc):
    adj, node, sc_adj, sc_node = inputs(cfg, flags, seed, tag)
    c_noise = np.linspace(-1.4, 1.1, len(flags)).astype(np.float32)
    args = (T(adj), T(node), T(flags), T(c_noise)) + ((T(sc_adj), T(sc_node)) if sc else ())
    return lambda: [t.clone() for t in net.model(*args)]


@gpu
@pytest.mark.parametrize("name,B", CASES)
def test_list_and_forward_bit_identical(name, B):
    cfg, net = cfg_for(name), net_for(name)
    n = cfg.max_node_num
    pats = flag_patterns(n, B)
    runs = {(p, sc): forward_fn(net, cfg, f, 19, f"readout_list/{name}/{B}/{p}", sc) for p, f in pats.items() for sc in (False, True)}
    h = set_list(net, 0)
    ref = {k: run() for k, run in runs.items()}
    assert h.readout_tiles(B)["form"] == "pos"
    h = set_list(net, 1)
    for (p, sc), run in runs.items():
        oa, on = run()
        got = h.readout_tiles(B)
        # (a) the list the launch just read
        assert got is not None and got["form"] == "list", f"{name} B={B} {p}: the list form did not run"
        tiles, want = got["tiles"], expected_tiles(pats[p])
        assert np.all(np.diff(tiles) > 0), f"{name} B={B} {p}: the list is not ascending or holds duplicates"
        assert np.array_equal(tiles, want), f"{name} B={B} {p}: device list differs from the rule"
        # (b)
        assert torch.equal(oa, ref[(p, sc)][0]) and torch.equal(on, ref[(p, sc)][1]), f"{name} B={B} {(p, sc)}: list form differs"
    assert all(r["kind"] in ("runs", "windows") for r in h.need_lists(B))   # the tile list is not among the pruning's records
    # (c) stale scratch: NaN, then 1e30, in pool_part, the output buffers and everything else the workspace holds as scratch
    for pattern in (2, 3):
        for k in (("ragged", True), ("scattered", False), ("empty", True), ("none", False), ("count3", False), ("full", True)):
            h.poison(B, pattern)
            oa, on = runs[k]()
            assert torch.equal(oa, ref[k][0]) and torch.equal(on, ref[k][1]), f"{name} B={B} {k}: pattern {pattern} reached the outputs"
            f = T(pats[k[0]])
            masked = ~(f[:, None, :, None] & f[:, None, None, :]).expand_as(oa)
            assert torch.count_nonzero(oa[masked]) == 0, f"{name} B={B} {k}: adjacency output at masked pairs is not exact zeros"


@gpu
@pytest.mark.parametrize("name,B", [("n16", 1), ("n16", 3), ("n32", 2), ("n24", 2)])
def test_captured_body_replayed_under_another_count(name, B):
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    cfg, net = cfg_for(name), net_for(name)
    n, steps = cfg.max_node_num, 3
    smp = NodeAdjEDMSamplerHip(num_steps=steps, self_condition=True, dev="cuda")   # Heun + churn, captured step bodies

    def run(valid, seed):
        flags, ia, inn, na, nn, cv = Y.sampler_case(cfg, steps, B, valid, seed, f"readout_list/smp/{name}/{B}")
        out = smp.sample(net, T(flags), init_adjs=T(ia), init_nodes=T(inn), churn_noise=(T(na), T(nn)), coins=(cv < 0.5).astype(np.uint8),
                         num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj)
        return flags, [torch.as_tensor(t).clone() for t in out]
    first, second = [n // 2 - 2, 3, n][:B], [n, 2, n // 2 + 1][:B]
    set_list(net, 0)
    (_, ref1), (_, ref2) = run(first, 37), run(second, 37)
    h = set_list(net, 1)
    f1, got1 = run(first, 37)
    t1 = h.readout_tiles(B)
    f2, got2 = run(second, 37)   # other flags on the same handle: the captured bodies are replayed with a list of another length
    t2 = h.readout_tiles(B)
    assert t1["form"] == "list" and t2["form"] == "list"
    assert np.array_equal(t1["tiles"], expected_tiles(f1)) and np.array_equal(t2["tiles"], expected_tiles(f2))
    assert len(t1["tiles"]) != len(t2["tiles"])
    for got, ref, what in ((got1, ref1, "first"), (got2, ref2, "second (bodies replayed)")):
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), f"{name} B={B}: {what} sample call differs"
