"""CPU: the power of tests/test_f32_kernels.py -- its float64 references and derived bounds (tests/f32_ref.py) on their own.  A correct
fp32 evaluation in ANOTHER summation order (plain float32 torch) must pass every GEMM-form bound with 4x headroom, and a handful of
seeded wrong results -- the mistakes a tiled kernel actually makes -- must fail it, at the smallest and the largest K of the list.  The
numpy packers used for the register-chained kernels are checked index for index against a transcription of the formulas above
pack_mlp_weights / pack_attn_weights (csrc/dsg_api.cpp) on tensors of distinct integers."""
import numpy as np
import pytest
import torch

import f32_ref as R
from f32_ref import GemmCase


def _ids(cases):
    return [c.ident() for c in cases]


@pytest.mark.parametrize("case", R.all_gemm_cases(), ids=_ids(R.all_gemm_cases()))
def test_float32_evaluation_has_4x_headroom(case):
    o = R.make_gemm(case)
    ref, f32 = R.gemm_expect(o), R.gemm_expect(o, torch.float32)
    assert torch.isfinite(ref["C"]).all() and (ref["bC"] > 0).all()
    r = R.worst_ratio(f32["C"], ref["C"], ref["bC"])
    assert r <= 0.25, f"C: float32 evaluation at {r:.2f} of the bound"
    if "C2" in ref:
        r = R.worst_ratio(f32["C2"], ref["C2"], ref["bC2"])
        assert r <= 0.25, f"C2: float32 evaluation at {r:.2f} of the bound"
    if case.epi >= 1:   # statistics of the stored values, accumulated in float32 in another order than float64's
        stored = f32["C"]
        S, Bd = R.stats_expect(stored, case, ref["C"], ref["bC"])
        got = torch.zeros_like(S)
        for t in range(case.tiles_n):
            seg = stored[:, R.GBN * t:min(R.GBN * (t + 1), case.N)]
            got[:, t, 0], got[:, t, 1] = seg.sum(1), (seg * seg).sum(1)
        r = R.worst_ratio(got, S, Bd)
        assert r <= 0.25, f"statistics: float32 sums at {r:.2f} of the bound"


K_LO, K_HI = 32, 768
MUT_BASE = {
    "drop_chunk": [GemmCase(129, 97, K_LO, seed=1), GemmCase(129, 97, K_HI, seed=2), GemmCase(130, 100, K_HI, ln="part", act=R.ACT_GELU, seed=3),
                   GemmCase(130, 100, K_LO, ln="stats", act=R.ACT_SILU, res=True, seed=4)],
    "swap_rows": [GemmCase(129, 97, K_LO, seed=5), GemmCase(129, 97, K_HI, ln="part", res=True, seed=6)],
    "bias_shift": [GemmCase(129, 97, K_LO, act=R.ACT_GELU, seed=7), GemmCase(129, 97, K_HI, ln="stats", seed=8)],
    "drop_partial": [GemmCase(64, 100, K_LO, ln="part", seed=9), GemmCase(64, 100, K_HI, ln="part", act=R.ACT_GELU, seed=10),
                     GemmCase(27, 96, K_HI, ln="part", a4_res=6, B=3, seed=11), GemmCase(27, 96, 128, ln="part", a4_res=6, B=3, seed=12)],
    "neighbour_sample": [GemmCase(300, 100, K_LO, epi=3, mod_T=36, mod_off=8, seed=13), GemmCase(300, 100, K_HI, epi=3, res=True, mod_T=36, mod_off=8, seed=14)],
}
MUT_CASES = [(m, c) for m, cs in MUT_BASE.items() for c in cs]


@pytest.mark.parametrize("mutation,case", MUT_CASES, ids=[f"{m}-{c.ident()}" for m, c in MUT_CASES])
def test_wrong_results_fail_the_bound(mutation, case):
    """(K = 32 has a single k-chunk: dropping it leaves the bias alone.)"""
    o = R.make_gemm(case)
    ref, bad = R.gemm_expect(o), R.gemm_expect(o, mutate=mutation)
    r = R.worst_ratio(bad["C"], ref["C"], ref["bC"])
    assert r > 1.0, f"{mutation} stays inside the bound ({r:.2f})"
    # not by a hair: the bound separates a correct fp32 result from this mistake by orders of magnitude
    assert r > 100.0 * R.worst_ratio(R.gemm_expect(o, torch.float32)["C"], ref["C"], ref["bC"])


@pytest.mark.parametrize("K", [K_LO, K_HI])
@pytest.mark.parametrize("N", [100, 200])
def test_statistics_over_the_whole_tile_fail_the_bound(N, K):
    """a tile's (sum, sumsq) taken over its 96 columns where only N - n0 are valid: the store buffer's padding leaks in"""
    case = GemmCase(130, N, K, epi=1, seed=20 + N)
    o = R.make_gemm(case)
    ref = R.gemm_expect(o)
    tn = case.tiles_n
    stored = torch.randn(case.M, R.GBN * tn, generator=torch.Generator().manual_seed(5)) * 0.01    # what sits behind column N
    stored[:, :N] = R.gemm_expect(o, torch.float32)["C"]
    S, Bd = R.stats_expect(stored, case, ref["C"], ref["bC"])
    bad, _ = R.stats_expect(stored, case, all_96=True)
    assert R.worst_ratio(bad[:, :tn - 1], S[:, :tn - 1], Bd[:, :tn - 1]) == 0.0        # full tiles are the same sums
    assert R.worst_ratio(bad[:, tn - 1], S[:, tn - 1], Bd[:, tn - 1]) > 1.0


def test_run_list_follows_the_contract():
    gen = torch.Generator().manual_seed(0)
    for cnt in R.ROW_COUNTS:
        for stale in (0, 1):
            runs, lst = R.make_run_list(40, cnt, stale, gen)
            assert len(runs) == cnt and runs == sorted(set(runs)) and len(lst) % 16 == 0 and len(lst) >= 16
            head = (cnt + 15) // 16 * 16
            assert lst[:cnt] == runs and all(v == -1 for v in lst[cnt:max(head, 16)])
            assert all(0 <= v < 40 for v in lst[max(head, 16):]) and len(lst) == max(head, 16) + 16 * stale


def test_packers_follow_the_index_formulas():
    """W1p[nt][s][lane][t] = fc1.weight[32nt + (lane&31)][8s + 4(lane>>5) + t]; W2p[nt][ct][g][lane][t] = fc2.weight[32ct + (lane&31)]
    [32nt + 8g + 4(lane>>5) + t]; Wqp / Wpp are the same two patterns on qkv.weight [3C, C] / proj.weight [C, C].
    The loops below transcribe the formulas written above the C++ packers (which need a device); what ties the numpy packers to the
    library itself is the GPU tests, whose kernels read weights packed this way"""
    for C in (96, 192):
        Hd, S, CT, NT = 4 * C, C // 8, C // 32, 4 * C // 32
        w1 = np.arange(Hd * C, dtype=np.float32).reshape(Hd, C)
        w2 = (np.arange(C * Hd, dtype=np.float32) + 0.5).reshape(C, Hd)
        p1, p2 = np.empty(Hd * C, np.float32), np.empty(C * Hd, np.float32)
        for nt in range(NT):
            for s in range(S):
                for lane in range(64):
                    for t in range(4):
                        p1[((nt * S + s) * 64 + lane) * 4 + t] = w1[32 * nt + (lane & 31), 8 * s + 4 * (lane >> 5) + t]
            for ct in range(CT):
                for g in range(4):
                    for lane in range(64):
                        for t in range(4):
                            p2[(((nt * CT + ct) * 4 + g) * 64 + lane) * 4 + t] = w2[32 * ct + (lane & 31), 32 * nt + 8 * g + 4 * (lane >> 5) + t]
        assert np.array_equal(R.pack_rows(w1), p1) and np.array_equal(R.pack_cols(w2), p2)
    C, S, CT, NT, HD = 96, 12, 3, 9, 3
    wq = np.arange(3 * C * C, dtype=np.float32).reshape(3 * C, C)
    wp = (np.arange(C * C, dtype=np.float32) + 0.25).reshape(C, C)
    p1, p2 = np.empty(3 * C * C, np.float32), np.empty(C * C, np.float32)
    for nt in range(NT):
        for s in range(S):
            for lane in range(64):
                for t in range(4):
                    p1[((nt * S + s) * 64 + lane) * 4 + t] = wq[32 * nt + (lane & 31), 8 * s + 4 * (lane >> 5) + t]
    for hd in range(HD):
        for ct in range(CT):
            for g in range(4):
                for lane in range(64):
                    for t in range(4):
                        p2[(((hd * CT + ct) * 4 + g) * 64 + lane) * 4 + t] = wp[32 * ct + (lane & 31), 32 * hd + 8 * g + 4 * (lane >> 5) + t]
    assert np.array_equal(R.pack_rows(wq), p1) and np.array_equal(R.pack_cols(wp), p2)


def test_attention_formula_is_a_softmax_over_keys():
    """the shared attention formula against an independent per-window loop (key-major bias, padded key slots never enter)"""
    gen = torch.Generator().manual_seed(3)
    B, res, ws, shift, heads = 2, 10, 5, 2, 2
    T, Wt, nW, Wp = res * res, ws * ws, (res // ws) ** 2, R.padded(ws)
    qkv = torch.randn(B * T, 3 * 32 * heads, generator=gen, dtype=torch.float64)
    bias = R.make_attn_bias(nW, heads, ws, shift, gen)
    assert bias.shape == (nW, heads, Wp, Wp) and (bias[:, :, Wt:] == -1e30).all()
    got = R.attn_formula(qkv, bias, B, res, ws, shift, heads)
    tok = R.window_tokens(res, ws, shift)
    ref = torch.zeros_like(got)
    x = qkv.view(B, T, 3, heads, 32)
    for b in range(B):
        for w in range(nW):
            for h in range(heads):
                q, k, v = (x[b, tok[w], i, h] for i in range(3))
                s = q @ k.t() + bias[w, h, :Wt, :Wt].double().t()          # [query, key]
                p = torch.softmax(s * np.log(2.0), dim=1)
                ref[b * T + torch.from_numpy(tok[w]), 32 * h:32 * h + 32] = p @ v
    assert float((got - ref).abs().max()) < 1e-12
