"""The lists of the pure-window deduplication one and two levels up (option "dedup_levels") and the identity they rest on.

A window of level k has 8 x 8 tokens of the grid of N >> k tokens per side and covers 8 << k nodes per side; it is pure when no valid
pair lies under it.  Level k's unique windows are its non-pure ones plus the graph's first pure one; the others are filled by copy.

CPU: the rule restated in NumPy, on the headline shape.
GPU, through dsg_debug_dedup_level_lists (the list program runs inside need_lists_kernel; a sampler call stages it): the lists of every
  level against the rule, and coverage on the device's own lists -- the forward's launches replayed on sets of rows: every row a listed
  launch reads was written before, every fill source was computed, no computed window is overwritten, and behind each fill every row
  that a later launch reads is written (the activation, and the skip rows the up path reads through its coarse lists).
CPU, with the oracle: for a masked-input graph the rows of two pure windows are equal after PatchMerging and after the first block, at
  level 1 and at level 2.
"""
import numpy as np
import pytest

from diffusesg_amd import spec as S
from diffusesg_amd import synth as Y
from diffusesg_amd import weights as W

WS = 8


# ---- the rule, restated ------------------------------------------------------------------------------------------------------
def expected(flags, level):
    """per batch at `level`: unique windows, unique runs, copied windows (sorted global ids) and the representative of every graph"""
    B, n = flags.shape
    side, res = WS << level, n >> level          # nodes under one window side; tokens per grid side
    nwr = res // WS
    nW = nwr * nwr
    wins, runs, copy, rep = [], [], [], []
    for b, f in enumerate(flags):
        valid = np.outer(f, f)
        pure = ~valid.reshape(nwr, side, nwr, side).any(axis=(1, 3)).reshape(-1)      # no valid pair under the window
        r = int(np.flatnonzero(pure)[0]) if pure.any() else -1
        rep.append(b * nW + r if r >= 0 else -1)
        for w in range(nW):
            if not pure[w] or w == r:
                wins.append(b * nW + w)
                wi, wj = divmod(w, nwr)
                runs += [b * res * nwr + (wi * WS + p) * nwr + wj for p in range(WS)]
            else:
                copy.append(b * nW + w)
    return dict(wins=np.array(sorted(wins), np.int64), runs=np.array(sorted(runs), np.int64), copy=np.array(sorted(copy), np.int64),
                rep=np.array(rep))


def test_the_restated_rule_on_the_headline_shape():
    f = W.synth_flags(1, 64, [30])
    e1, e2 = expected(f, 1), expected(f, 2)
    assert (len(e1["wins"]), len(e1["copy"])) == (5, 11)
    assert (len(e2["wins"]), len(e2["copy"])) == (2, 2)
    assert len(e1["runs"]) == 5 * 8 and len(e2["runs"]) == 2 * 8
    f = W.synth_flags(1, 64, [33])
    assert len(expected(f, 2)["copy"]) == 0 and expected(f, 2)["rep"][0] == -1 and len(expected(f, 2)["wins"]) == 4
    assert len(expected(f, 1)["copy"]) > 0
    # a pure window of level k lies over 2 x 2 pure windows of level k - 1: the chain's premise, for every prefix count
    for v in range(65):
        f = W.synth_flags(1, 64, [v])
        for k in (1, 2):
            nwr = (64 >> k) // WS
            fine_copy_or_rep = set(expected(f, k - 1)["copy"].tolist()) | {int(expected(f, k - 1)["rep"][0])}
            for w in expected(f, k)["copy"].tolist() + [int(expected(f, k)["rep"][0])]:
                if w < 0:
                    continue
                wi, wj = divmod(w, nwr)
                assert {(2 * wi + d) * 2 * nwr + 2 * wj + e for d in (0, 1) for e in (0, 1)} <= fine_copy_or_rep


def patterns(n):
    p = {}
    counts = [0, 1, 15, 16, 17, 30, 31, 32, 33, 48, 49, 64]
    for i in range(0, len(counts), 4):
        p[f"prefix{i // 4}"] = W.synth_flags(4, n, [min(n, c) for c in counts[i:i + 4]])
    scattered = np.zeros((3, n), bool)
    scattered[0, [9, 10, n - 20]] = True
    scattered[1, [n // 2 + 1]] = True
    scattered[2, [0, n - 1]] = True
    no_pure = np.zeros((2, n), bool)
    no_pure[0, ::8] = True
    no_pure[1, 7::8] = True
    p.update(scattered=scattered, no_pure=no_pure, all_true=np.ones((2, n), bool), all_false=np.zeros((2, n), bool),
             mixed=W.synth_flags(4, n, [n // 2 - 2, 0, n, 1]))
    return p


def runs_of_windows(ws, res):
    nwr = res // WS
    nW = nwr * nwr
    return {(w // nW) * res * nwr + (((w % nW) // nwr) * WS + p) * nwr + (w % nwr) for w in ws for p in range(WS)}


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


@pytest.mark.gpu
def test_device_lists_of_every_level_match_the_rule_and_cover_what_is_read():
    import torch
    from diffusesg_amd.model import build_network
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    cfg = S.vg_config()
    n, L = cfg.max_node_num, len(cfg.depths)
    net = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")
    h = net.model._ensure_handle()
    h.set_option("fused_merge", 2)   # the partial-statistics PatchMerging at every size: the form whose run-list variant the levels use
    assert h.get_option("dedup_masked") == 1 and h.get_option("dedup_levels") == 3
    smp = NodeAdjEDMSamplerHip(num_steps=1, self_condition=True, dev="cuda")
    for pat, flags in patterns(n).items():
        B = len(flags)
        smp.sample(net, torch.from_numpy(flags).cuda(), num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj, seed=3)
        need = h.need_lists(B)
        assert h.dedup_level_lists(B, 3) is None, "level 3 is a single window: no lists"
        below_all = None
        for k in range(3):
            res = n >> k
            nwr = res // WS
            got, exp = h.dedup_level_lists(B, k), expected(flags, k)
            for key in ("wins", "runs", "copy"):
                assert len(set(got[key].tolist())) == len(got[key]), f"{pat} level {k} {key}: duplicate entries"
                assert np.array_equal(np.sort(got[key]), exp[key]), f"{pat} level {k} {key}: device list differs from the rule"
            assert np.array_equal(got["rep"], exp["rep"]), f"{pat} level {k}: representatives differ"
            assert got["fwd"] >= 0, f"{pat}: level {k} was not deduplicated by the forward"
            all_runs = set(range(B * res * nwr))
            runs, wins, copy = set(got["runs"].tolist()), got["wins"].tolist(), got["copy"].tolist()
            if k > 0:   # the merge into level k reads the fine rows under its run list: behind level k - 1's fill and the blocks after it
                assert fine_runs_under(runs, res) <= below_all, f"{pat} level {k}: the merge reads a stale fine row"
            written = set(runs)                                   # PatchEmbed / the merge (x, skip, partials) write the run list
            assert runs_of_windows(wins, res) <= written, f"{pat} level {k}: attention reads a row nobody wrote"
            srcs = {int(got["rep"][w // (nwr * nwr)]) for w in copy}
            assert -1 not in srcs and runs_of_windows(srcs, res) <= written, f"{pat} level {k}: the copy reads a window nobody computed"
            assert not (set(copy) & set(wins)), f"{pat} level {k}: a computed window is overwritten"
            written |= runs_of_windows(copy, res)
            # behind the fill: the level's next launch (a shifted block, or the next PatchMerging) reads every row of the activation ...
            assert written == all_runs, f"{pat} level {k}: a later launch would read a stale row"
            # ... and the skip (levels >= 1; written by the merge and the fill alike) is read by the up stage's pre_linear through its
            # coarse list, or as a whole where that stage has no list
            if k > 0:
                coarse = [r for r in need if r["kind"] == "runs" and r["block"] == -2 and r["res"] == res and r["stage"] == L - k]
                read = set(coarse[0]["entries"].tolist()) if coarse else all_runs
                assert read <= written, f"{pat} level {k}: the up path reads a stale skip row"
            below_all = written


def test_pure_windows_share_their_rows_one_and_two_levels_up_in_the_oracle():
    """CPU: the identity itself on the oracle's forward -- taps `down0` / `down1` (PatchMerging's output) and `down1.block0` /
    `down2.block0` (the level's first, unshifted block)."""
    from oracle.oracle import Oracle
    n = 64
    cfg = S.ModelConfig(max_node_num=n, c_adj=3, c_node=5, depths=(1, 1, 1), num_heads=(3, 6, 12), window_size=WS, self_condition=True)
    B, valid = 1, [11]
    flags, adj, node, sc_adj, sc_node = Y.case_inputs(cfg, B, valid, 5, "dedup_levels/oracle")   # masked like the sampler hands them over
    c_noise = np.array([0.4], np.float32)
    E = cfg.embed_dim
    sizes = {"down0": (n // 2) ** 2 * 2 * E, "down1.block0": (n // 2) ** 2 * 2 * E, "down1": (n // 4) ** 2 * 4 * E,
             "down2.block0": (n // 4) ** 2 * 4 * E}
    _, _, taps = Oracle(cfg, W.synth_state_dict(cfg, 0)).forward(adj, node, flags, c_noise, sc_adj, sc_node, taps=dict(sizes))
    for name, k in (("down0", 1), ("down1.block0", 1), ("down1", 2), ("down2.block0", 2)):
        res, C = n >> k, E << k
        nwr = res // WS
        x = taps[name].reshape(B, nwr, WS, nwr, WS, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, nwr * nwr, WS * WS, C)
        e = expected(flags, k)
        pure = sorted(e["copy"].tolist() + [int(e["rep"][0])])
        assert len(pure) >= 2 and len(pure) < nwr * nwr
        for w in pure[1:]:
            assert np.array_equal(x[0, w], x[0, pure[0]]), f"{name}: pure windows {pure[0]} and {w} differ"
        assert not np.array_equal(x[0, 0], x[0, pure[0]]), "window 0 holds valid pairs"
