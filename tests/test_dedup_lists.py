"""The lists of the pure-window deduplication (option "dedup_masked") and the identity they rest on.

GPU, through dsg_debug_dedup_lists (the list program runs on the device, inside need_lists_kernel; a sampler call stages it):
  * unique windows / unique runs / copied windows / representatives against a NumPy restatement of the rule, for prefix, scattered,
    all-true and all-false flags;
  * coverage: every row a stage reads has been written before -- the first block reads only rows PatchEmbed wrote, the copy reads only
    rows the block wrote, and behind the copy every row of the level is written.
CPU, with the oracle: for a prefix-flag graph with masked inputs the rows of two different pure windows are equal after PatchEmbed and
after the level-0 block (the oracle's `down0.block0` tap), position by position inside the window.
"""
import numpy as np
import pytest

from diffusesg_amd import spec as S
from diffusesg_amd import synth as Y
from diffusesg_amd import weights as W

WS = 8


# ---- the rule, restated ------------------------------------------------------------------------------------------------------
def expected(flags):
    """per batch: unique windows, unique runs, copied windows (sorted global ids) and the representative of every graph"""
    B, n = flags.shape
    nwr = n // WS
    nW = nwr * nwr
    wins, runs, copy, rep = [], [], [], []
    for b, f in enumerate(flags):
        valid = np.outer(f, f)                                                        # token (i, j) is valid iff both endpoints are
        pure = ~valid.reshape(nwr, WS, nwr, WS).any(axis=(1, 3)).reshape(-1)          # a window without a valid token
        r = int(np.flatnonzero(pure)[0]) if pure.any() else -1                        # the first pure window stands for all of them
        rep.append(b * nW + r if r >= 0 else -1)
        for w in range(nW):
            if not pure[w] or w == r:
                wins.append(b * nW + w)
                wi, wj = divmod(w, nwr)
                runs += [b * n * nwr + (wi * WS + p) * nwr + wj for p in range(WS)]   # run (i, jr) = 8 tokens of grid row i
            else:
                copy.append(b * nW + w)
    return dict(wins=np.array(sorted(wins)), runs=np.array(sorted(runs)), copy=np.array(sorted(copy)), rep=np.array(rep))


def patterns(n):
    scattered = np.zeros((3, n), bool)
    scattered[0, [9, 10, n - 20]] = True
    scattered[1, [n // 2 + 1]] = True
    scattered[2, [0, n - 1]] = True
    mixed = W.synth_flags(4, n, [n // 2 - 2, 0, n, 1])
    return {"prefix": W.synth_flags(4, n, [7, 8, 9, min(n, 30)]), "scattered": scattered, "all_true": np.ones((2, n), bool),
            "all_false": np.zeros((2, n), bool), "mixed": mixed}


def test_the_restated_rule_on_the_headline_shape():
    """CPU: N = 64 with 30 valid nodes -- 16 of 64 windows hold a valid pair, 48 are pure, 47 of them are copies of window 4."""
    e = expected(W.synth_flags(1, 64, [30]))
    assert len(e["wins"]) == 17 and len(e["copy"]) == 47 and e["rep"][0] == 4 and len(e["runs"]) == 17 * 8
    e = expected(W.synth_flags(1, 64, [20]))   # window rows / columns 0..2 valid
    assert len(e["wins"]) == 10 and e["rep"][0] == 3


@pytest.mark.gpu
@pytest.mark.parametrize("n", [16, 64])
def test_device_lists_match_the_rule(n):
    import torch
    from diffusesg_amd.model import build_network
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    cfg = S.vg_config() if n == 64 else S.ModelConfig(max_node_num=n, c_adj=3, c_node=5, depths=(1, 1), num_heads=(3, 6), window_size=WS,
                                                      self_condition=True)
    net = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")
    h = net.model._ensure_handle()
    assert h.get_option("dedup_masked") == 1
    smp = NodeAdjEDMSamplerHip(num_steps=1, self_condition=True, dev="cuda")
    nwr = n // WS
    for pat, flags in patterns(n).items():
        smp.sample(net, torch.from_numpy(flags).cuda(), num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj, seed=3)
        got = h.dedup_lists(len(flags))
        exp = expected(flags)
        for key in ("wins", "runs", "copy"):
            assert len(set(got[key].tolist())) == len(got[key]), f"{n} {pat} {key}: duplicate entries"
            assert np.array_equal(np.sort(got[key]), exp[key]), f"{n} {pat} {key}: device list differs from the rule"
        assert np.array_equal(got["rep"], exp["rep"]), f"{n} {pat}: representatives differ"
        # coverage, on the device's own lists.  rows of a window w = (wi, wj) of graph b, as runs:
        def runs_of(ws):
            return {(w // (nwr * nwr)) * n * nwr + (((w % (nwr * nwr)) // nwr) * WS + p) * nwr + (w % nwr) for w in ws for p in range(WS)}
        written = set(got["runs"].tolist())                                    # PatchEmbed writes its run list
        assert runs_of(got["wins"].tolist()) <= written, "attention reads a row PatchEmbed did not write"
        assert set(got["runs"].tolist()) <= written                            # the MLP's rows: the same list
        srcs = {int(got["rep"][w // (nwr * nwr)]) for w in got["copy"].tolist()}
        assert -1 not in srcs and runs_of(srcs) <= written, "the copy reads a window nobody computed"
        assert not (set(got["copy"].tolist()) & set(got["wins"].tolist())), "a computed window is overwritten"
        written |= runs_of(got["copy"].tolist())
        assert written == set(range(len(flags) * n * nwr)), "PatchMerging would read a stale row"


def test_pure_windows_share_their_rows_in_the_oracle():
    """CPU: the identity itself, on the oracle's forward (taps `patch_embed` and `down0.block0`)."""
    from oracle.oracle import Oracle
    n = 32
    cfg = S.ModelConfig(max_node_num=n, c_adj=3, c_node=5, depths=(1, 1), num_heads=(3, 6), window_size=WS, self_condition=True)
    B, valid = 2, [11, 3]
    flags, adj, node, sc_adj, sc_node = Y.case_inputs(cfg, B, valid, 5, "dedup/oracle")   # masked like the sampler hands them over
    c_noise = np.array([0.4, -1.1], np.float32)
    T, E = n * n, cfg.embed_dim
    _, _, taps = Oracle(cfg, W.synth_state_dict(cfg, 0)).forward(adj, node, flags, c_noise, sc_adj, sc_node,
                                                                  taps={"patch_embed": T * E, "down0.block0": T * E})
    nwr = n // WS
    for name in ("patch_embed", "down0.block0"):
        x = taps[name].reshape(B, nwr, WS, nwr, WS, E).transpose(0, 1, 3, 2, 4, 5).reshape(B, nwr * nwr, WS * WS, E)   # [b, window, position, c]
        for b in range(B):
            f = flags[b]
            pure = ~np.outer(f, f).reshape(nwr, WS, nwr, WS).any(axis=(1, 3)).reshape(-1)
            idx = np.flatnonzero(pure)
            assert len(idx) >= 2 and not pure.all()
            for w in idx[1:]:
                assert np.array_equal(x[b, w], x[b, idx[0]]), f"{name}: pure windows {idx[0]} and {w} of graph {b} differ"
            assert not np.array_equal(x[b, 0], x[b, idx[0]]), "window 0 holds valid pairs"
    # rows differ by position inside a pure window after the block (relative-position bias), not after PatchEmbed
    pe = taps["patch_embed"].reshape(B, T, E)
    assert np.array_equal(pe[1, n * n - 1], pe[1, n * n - 2])
