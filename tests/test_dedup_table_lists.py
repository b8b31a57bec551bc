"""The lists of the pure-window deduplication when the batch's representative comes from the sampler's table (option "dedup_table").

dsg_debug_dedup_level_lists keeps reporting the unique windows by meaning -- every non-pure window plus the representative, the fills
without it (tests/test_dedup_batch_lists.py holds that under the default, which is this option on).  dsg_debug_dedup_launch_lists
reports what the launches iterate: the non-pure windows only, and a fill list that also holds the former representative.

GPU: the headline pattern at 16 graphs (256 / 64 / 16 windows launched where 257 / 65 / 17 are reported); the launch-side lists against
  the rule restated here; and coverage on them -- the forward's launches replayed on sets of rows: every row a listed launch or a merge
  reads was written by a listed launch or by a fill, no computed window is overwritten, behind the top level's fill every row is
  written, every pure window that is read is filled, and every skip row in the up path's coarse list is written.
"""
import numpy as np
import pytest

from diffusesg_amd import spec as S
from diffusesg_amd import weights as W

WS = 8


def pure_windows(flags, level):
    """[B * nW] bool: no valid pair under the window"""
    B, n = flags.shape
    side, nwr = WS << level, (n >> level) // WS
    blk = flags.reshape(B, nwr, side).any(axis=2)
    return ~(blk[:, :, None] & blk[:, None, :]).reshape(B * nwr * nwr)


def runs_of_windows(ws, res):
    nwr = res // WS
    nW = nwr * nwr
    return {(w // nW) * res * nwr + (((w % nW) // nwr) * WS + p) * nwr + (w % nwr) for w in ws for p in range(WS)}


def fine_windows_under(w, nwr):
    b, v = divmod(w, nwr * nwr)
    wi, wj = divmod(v, nwr)
    return {b * 4 * nwr * nwr + (2 * wi + d) * 2 * nwr + 2 * wj + e for d in (0, 1) for e in (0, 1)}


def fine_runs_under(runs, res):
    """runs of the grid of 2 * res tokens per side that PatchMerging reads for the merged runs `runs` (side res)"""
    rpr = res // WS
    out = set()
    for r in runs:
        b, t = divmod(r, res * rpr)
        i, jr = divmod(t, rpr)
        out |= {b * (2 * res) * (2 * rpr) + (2 * i + d) * (2 * rpr) + 2 * jr + e for d in (0, 1) for e in (0, 1)}
    return out


def patterns(n):
    p = {}
    for name, counts in (("headline16", [30] * 16), ("around8", [7, 8, 9, 0]), ("around16", [15, 16, 17, 1]), ("around32", [31, 32, 33, n]),
                         ("rep_moves", [33, 30]), ("only_graph2", [n, n, 30, n])):
        p[name] = W.synth_flags(len(counts), n, [min(n, c) for c in counts])
    scattered = np.zeros((3, n), bool)
    scattered[0, [9, 10, n - 20]] = True
    scattered[1, [n // 2 + 1]] = True
    scattered[2, [0, n - 1]] = True
    p.update(scattered=scattered, all_true=np.ones((2, n), bool), all_false=np.zeros((2, n), bool))
    return p


@pytest.mark.gpu
def test_launch_side_lists_leave_the_representative_to_the_fill_and_cover_what_is_read():
    import torch
    from diffusesg_amd.model import build_network
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    cfg = S.vg_config()
    n, L, depth = cfg.max_node_num, len(cfg.depths), 3
    net = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")
    h = net.model._ensure_handle()
    h.set_option("fused_merge", 2)
    h.set_option("dedup_batch", 2)
    assert h.get_option("dedup_table") == 1 and h.get_option("dedup_levels") == depth
    smp = NodeAdjEDMSamplerHip(num_steps=1, self_condition=True, dev="cuda")
    for pat, flags in patterns(n).items():
        B = len(flags)
        smp.sample(net, torch.from_numpy(flags).cuda(), num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj, seed=3)
        need = h.need_lists(B)
        pure = [pure_windows(flags, k) for k in range(depth)]
        below = None
        for k in range(depth):
            res = n >> k
            nwr = res // WS
            got, rep = h.dedup_launch_lists(B, k), h.dedup_level_lists(B, k)
            assert got["mode"] == 3, f"{pat} level {k}: the lists were not written for the table"
            for key in ("wins", "runs", "copy"):
                assert len(set(got[key].tolist())) == len(got[key]), f"{pat} level {k} {key}: duplicate entries"
            wins, runs, copy = got["wins"].tolist(), set(got["runs"].tolist()), got["copy"].tolist()
            # the rule: the launches take the non-pure windows and nothing else
            assert sorted(wins) == np.flatnonzero(~pure[k]).tolist(), f"{pat} level {k}: the launches do not take exactly the non-pure windows"
            assert runs == runs_of_windows(wins, res)
            assert all(pure[k][w] for w in copy), f"{pat} level {k}: a non-pure window is filled"
            # ... and the reported lists name the table's window with the unique ones
            r = int(rep["rep"][0])
            assert r == (int(np.flatnonzero(pure[k])[0]) if pure[k].any() else -1) and (rep["rep"] == r).all()
            assert sorted(rep["wins"].tolist()) == sorted(wins + ([r] if r >= 0 else []))
            assert sorted(rep["copy"].tolist()) == sorted(w for w in copy if w != r)
            if r >= 0:
                assert r in copy and r not in wins, f"{pat} level {k}: the former representative is filled, not computed"
            if pat == "headline16":
                assert (len(wins), len(rep["wins"])) == [(256, 257), (64, 65), (16, 17)][k]
            # what is read: the top level whole; below it, the fine windows under the windows the next level's launches take
            if k == depth - 1:
                read = set(range(B * nwr * nwr))
            else:
                read = set()
                for w in h.dedup_launch_lists(B, k + 1)["wins"].tolist():
                    read |= fine_windows_under(w, nwr // 2)
            assert {w for w in read if pure[k][w]} <= set(copy), f"{pat} level {k}: a pure window that is read is not filled"
            # coverage, replayed on rows
            all_runs = set(range(B * res * nwr))
            if k > 0:   # the merge into level k reads the fine rows under its run list: behind level k - 1's fill
                assert fine_runs_under(runs, res) <= below, f"{pat} level {k}: the merge reads a stale fine row"
            written = set(runs)                                   # PatchEmbed / the merge (x, skip, partials) write the run list
            assert runs_of_windows(wins, res) <= written, f"{pat} level {k}: attention reads a row nobody wrote"
            assert not (set(copy) & set(wins)), f"{pat} level {k}: a computed window is overwritten"
            written |= runs_of_windows(copy, res)                 # the fill: every listed window, from the table
            if k == depth - 1:
                assert written == all_runs, f"{pat} level {k}: a later launch would read a stale row"
            if k > 0:   # the skip is read by the up stage's pre_linear through its coarse list
                coarse = [x for x in need if x["kind"] == "runs" and x["block"] == -2 and x["res"] == res and x["stage"] == L - k]
                rd = set(coarse[0]["entries"].tolist()) if coarse else all_runs
                assert rd <= written, f"{pat} level {k}: the up path reads a stale skip row"
            below = written
