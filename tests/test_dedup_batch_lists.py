"""The lists of the pure-window deduplication with one representative for the whole batch (option "dedup_batch").

Where every graph of a batch reads the same (scale, shift) row -- the sampler -- a pure window of one graph has the rows of a pure
window of any other graph, so level k computes ONE pure window for the batch: the first in (graph, window) order.  Level k's unique
windows are every non-pure window plus that one.  The top level of the chain fills every other pure window (its next reader, a shifted
block or a full-row PatchMerging, reads everything); a level below the top fills only the pure windows that lie under a unique window
of level k + 1, because behind its fill only the run-list merge into level k + 1 reads its activation and statistics, and the up path
reads its skip through a coarse list that stays inside non-pure windows.

CPU: the rule restated in NumPy; the headline counts; the chain premise -- every fine window under a unique coarse window is unique
  or filled, wherever the representatives of the two levels lie.
GPU, through dsg_debug_dedup_level_lists: the device lists of every level against the rule, and coverage on the device's own lists --
  the forward's launches replayed on sets of rows: every row a listed launch or a merge reads was written before, every fill source
  was computed, no computed window is overwritten, behind the top level's fill every row is written, and every skip row in the up
  path's coarse list is written.  Once with the whole chain (levels 0, 1 trimmed, level 2 on top) and once with "dedup_levels" 1
  (level 0 is the top and is filled completely).
"""
import numpy as np
import pytest

from diffusesg_amd import spec as S
from diffusesg_amd import weights as W

WS = 8


# ---- the rule, restated ------------------------------------------------------------------------------------------------------
def pure_windows(flags, level):
    """[B, nW] bool: no valid pair under the window"""
    B, n = flags.shape
    side, nwr = WS << level, (n >> level) // WS
    blk = flags.reshape(B, nwr, side).any(axis=2)
    return ~(blk[:, :, None] & blk[:, None, :]).reshape(B, nwr * nwr)


def expected(flags, depth):
    """levels 0 .. depth - 1 of a chain of that depth: per level a dict of sorted global ids wins / runs / copy and the one rep"""
    B, n = flags.shape
    out = []
    for k in range(depth):
        pure = pure_windows(flags, k).reshape(-1)
        rep = int(np.flatnonzero(pure)[0]) if pure.any() else -1
        unique = ~pure
        if rep >= 0:
            unique[rep] = True
        out.append(dict(pure=pure, unique=unique, rep=rep))
    for k in range(depth):
        res = n >> k
        nwr = res // WS
        nW = nwr * nwr
        e = out[k]
        fill = e["pure"] & ~e["unique"]
        if k + 1 < depth:   # below the top: only under a unique window of level k + 1
            ids = np.arange(B * nW)
            b, w = ids // nW, ids % nW
            parent = b * (nW // 4) + (w // nwr // 2) * (nwr // 2) + (w % nwr) // 2
            fill &= out[k + 1]["unique"][parent]
        e["wins"] = np.flatnonzero(e["unique"])
        e["copy"] = np.flatnonzero(fill)
        e["runs"] = np.array(sorted(runs_of_windows(e["wins"].tolist(), res)), np.int64)
    return out


def runs_of_windows(ws, res):
    nwr = res // WS
    nW = nwr * nwr
    return {(w // nW) * res * nwr + (((w % nW) // nwr) * WS + p) * nwr + (w % nwr) for w in ws for p in range(WS)}


def fine_windows_under(w, nwr):
    """the 2 x 2 windows of the finer level (2 nwr per side) under window w (global id) of a level with nwr windows per side"""
    b, v = divmod(w, nwr * nwr)
    wi, wj = divmod(v, nwr)
    return {b * 4 * nwr * nwr + (2 * wi + d) * 2 * nwr + 2 * wj + e for d in (0, 1) for e in (0, 1)}


def fine_runs_under(runs, res):
    """runs of the grid of 2 * res tokens per side that PatchMerging reads for the merged runs `runs` (side res): merged run (b, i, jr)
    gathers fine rows 2 i, 2 i + 1, fine columns 16 jr .. 16 jr + 15"""
    rpr = res // WS
    out = set()
    for r in runs:
        b, t = divmod(r, res * rpr)
        i, jr = divmod(t, rpr)
        out |= {b * (2 * res) * (2 * rpr) + (2 * i + d) * (2 * rpr) + 2 * jr + e for d in (0, 1) for e in (0, 1)}
    return out


def check_chain_premise(flags, depth=3):
    n = flags.shape[1]
    e = expected(flags, depth)
    for k in range(1, depth):
        nwr = (n >> k) // WS
        have = set(e[k - 1]["wins"].tolist()) | set(e[k - 1]["copy"].tolist())
        for w in e[k]["wins"].tolist():
            assert fine_windows_under(w, nwr) <= have, f"level {k} window {w}: a fine window under it is neither unique nor filled"
        assert not (set(e[k]["wins"].tolist()) & set(e[k]["copy"].tolist()))
    return e


def test_headline_counts():
    e = expected(W.synth_flags(64, 64, [30] * 64), 3)
    assert [(len(x["wins"]), len(x["copy"])) for x in e] == [(1025, 3), (257, 3), (65, 191)]
    assert [len(x["runs"]) for x in e] == [1025 * 8, 257 * 8, 65 * 8]
    # per graph (the rule of tests/test_dedup_levels_lists.py) the same batch has 1088 / 320 / 128 unique windows
    assert [64 * (int((~pure_windows(W.synth_flags(1, 64, [30]), k)).sum()) + 1) for k in range(3)] == [1088, 320, 128]
    # level 0 as the top of a chain of one level fills everything else
    e0 = expected(W.synth_flags(64, 64, [30] * 64), 1)[0]
    assert (len(e0["wins"]), len(e0["copy"])) == (1025, 64 * 64 - 1025)


def test_chain_premise_over_prefix_counts_and_mixed_batches():
    for v in range(65):
        check_chain_premise(W.synth_flags(1, 64, [v]))
        check_chain_premise(W.synth_flags(2, 64, [64, v]))       # the representative always sits in the second graph
    # the level-2 representative in a later graph than the level-1 one: graph 0 (33 valid nodes) has no pure window at level 2
    e = check_chain_premise(W.synth_flags(2, 64, [33, 30]))
    assert 0 <= e[1]["rep"] < 16 and e[2]["rep"] >= 4, "level 1: graph 0, level 2: graph 1"
    # ... so the four level-1 windows under level 2's representative are filled from graph 0's window
    assert fine_windows_under(e[2]["rep"], 2) <= set(e[1]["copy"].tolist())
    rng = np.random.default_rng(5)
    for _ in range(60):
        B = int(rng.integers(1, 6))
        if rng.random() < 0.5:
            f = W.synth_flags(B, 64, [int(x) for x in rng.integers(0, 65, B)])
        else:
            f = rng.random((B, 64)) < rng.random((B, 1)) ** 3
        check_chain_premise(np.ascontiguousarray(f, dtype=bool))
        check_chain_premise(np.ascontiguousarray(f, dtype=bool), depth=2)


def patterns(n):
    p = {}
    for name, counts in (("around8", [7, 8, 9, 0]), ("around16", [15, 16, 17, 1]), ("around32", [31, 32, 33, n]), ("rep_moves", [33, 30])):
        p[name] = W.synth_flags(len(counts), n, [min(n, c) for c in counts])
    scattered = np.zeros((3, n), bool)
    scattered[0, [9, 10, n - 20]] = True
    scattered[1, [n // 2 + 1]] = True
    scattered[2, [0, n - 1]] = True
    no_pure = np.zeros((2, n), bool)
    no_pure[0, ::8] = True
    no_pure[1, 7::8] = True
    p.update(only_graph2=W.synth_flags(4, n, [n, n, 30, n]), scattered=scattered, no_pure=no_pure, all_true=np.ones((2, n), bool),
             all_false=np.zeros((2, n), bool))
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("levels", [0, 1])
def test_device_lists_match_the_rule_and_cover_what_is_read(levels):
    import torch
    from diffusesg_amd.model import build_network
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    cfg = S.vg_config()
    n, L = cfg.max_node_num, len(cfg.depths)
    net = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")
    h = net.model._ensure_handle()
    h.set_option("fused_merge", 2)   # the partial-statistics PatchMerging at every size: the form whose run-list variant the levels use
    h.set_option("dedup_batch", 2)
    h.set_option("dedup_levels", levels)
    depth = 3 if levels == 0 else 1
    assert h.get_option("dedup_batch") == 2 and h.get_option("dedup_levels") == depth
    smp = NodeAdjEDMSamplerHip(num_steps=1, self_condition=True, dev="cuda")
    for pat, flags in patterns(n).items():
        B = len(flags)
        smp.sample(net, torch.from_numpy(flags).cuda(), num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj, seed=3)
        need = h.need_lists(B)
        exp = expected(flags, depth)
        below = None
        for k in range(depth):
            res = n >> k
            nwr = res // WS
            got, e = h.dedup_level_lists(B, k), exp[k]
            for key in ("wins", "runs", "copy"):
                assert len(set(got[key].tolist())) == len(got[key]), f"{pat} level {k} {key}: duplicate entries"
                assert np.array_equal(np.sort(got[key]), e[key]), f"{pat} level {k} {key}: device list differs from the rule"
            assert (got["rep"] == e["rep"]).all(), f"{pat} level {k}: one representative id for every graph"
            assert got["fwd"] >= 0, f"{pat}: level {k} was not deduplicated by the forward"
            all_runs = set(range(B * res * nwr))
            runs, wins, copy = set(got["runs"].tolist()), got["wins"].tolist(), got["copy"].tolist()
            if k > 0:   # the merge into level k reads the fine rows under its run list: behind level k - 1's fill
                assert fine_runs_under(runs, res) <= below, f"{pat} level {k}: the merge reads a stale fine row"
            written = set(runs)                                   # PatchEmbed / the merge (x, skip, partials) write the run list
            assert runs_of_windows(wins, res) <= written, f"{pat} level {k}: attention reads a row nobody wrote"
            if copy:
                src = int(got["rep"][0])
                assert src >= 0 and src in set(wins), f"{pat} level {k}: the copy reads a window nobody computed"
            assert not (set(copy) & set(wins)), f"{pat} level {k}: a computed window is overwritten"
            written |= runs_of_windows(copy, res)
            if k == depth - 1:   # the top: its next launch (a shifted block, or a full PatchMerging) reads every row
                assert written == all_runs, f"{pat} level {k}: a later launch would read a stale row"
            if k > 0:   # the skip (written by the merge and the fill alike) is read by the up stage's pre_linear through its coarse list
                coarse = [r for r in need if r["kind"] == "runs" and r["block"] == -2 and r["res"] == res and r["stage"] == L - k]
                read = set(coarse[0]["entries"].tolist()) if coarse else all_runs
                assert read <= written, f"{pat} level {k}: the up path reads a stale skip row"
            below = written
        for k in range(depth, 3):
            assert h.dedup_level_lists(B, k)["fwd"] == -1
