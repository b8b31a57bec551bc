"""CPU: the power of tests/test_edge_kernels.py -- its float64 references and bars (tests/edge_ref.py) on their own.  A correct float32
evaluation in its own summation order (plain float32 torch) stays within a quarter of every derived per-element bound; every formula
bar is positive and below FWD_RTOL of the output scale; seeded wrong results -- the index mistakes these kernels can make -- land outside
the bar, more than a hundred times further out than the float32 evaluation; the numpy packers give the fragment orders the formulas in
dsg_finalize_weights (csrc/dsg_api.cpp: the pe_wp and fap / f2p loops) describe; and the committed read-out cases reach the all-masked
shortcut, a wave that mixes valid and masked tokens of one node row, and a row served by both kinds of wave."""
import numpy as np
import pytest
import torch

import edge_ref as X
import f32_ref as R
from util import FWD_RTOL

E = X.E
RO_PATTERN_CASES = [(B, N, Ca, pat) for (B, N, Ca) in X.READOUT_CASES for pat in X.FLAG_PATTERNS]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rows(M, Cc, gen):
    return torch.randn(M, Cc, generator=gen) + 2.0 * (2.0 * torch.rand(M, 1, generator=gen) - 1.0)


def _readout(B, N, Ca, pat, seed=0, **kw):
    gen = _gen(4000 + seed)
    flags = X.make_flags(B, N, pat, seed)
    p = X.make_readout_params(Ca, gen)
    x = _rows(B * N * N, E, gen)
    return flags, p, x, X.readout_expect(x, p, flags, **kw)


# ----------------------------------------------------------------------------------------------------------------------------------
# per-element bounds: the float32 evaluation keeps 4x headroom
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc", sorted(set(X.ROW_C + X.BREAKUP_D)))
def test_row_statistics_bound_has_4x_headroom(Cc):
    x = _rows(64, Cc, _gen(Cc))
    ref = X.row_stats(x.double())
    bound, _ = X.row_stats_bound(x.double())
    assert (bound > 0).all()
    r_st = R.worst_ratio(X.row_stats(x), ref, bound)
    assert r_st <= 0.25, f"(mean, rstd) in float32 at {r_st:.2f} of the bound"
    gam, bet = 1.0 + 0.2 * torch.randn(Cc, generator=_gen(1)), 0.2 * torch.randn(Cc, generator=_gen(2))
    r = R.worst_ratio(R.layer_norm(x, gam, bet), R.layer_norm(x.double(), gam.double(), bet.double()), X.ln_elem_bound(x.double(), gam))
    assert r <= 0.25, f"LayerNorm in float32 at {r:.2f} of the element bound"
    # statistics over one value too few (a lane's last float4 cut short) are far outside
    bad = X.row_stats(x.double()[:, :-1])
    assert R.worst_ratio(bad, ref, bound) > 100.0 * max(r_st, 1e-3)


@pytest.mark.parametrize("B,N,Ca,pat", RO_PATTERN_CASES)
def test_pool_ext_bound_has_4x_headroom(B, N, Ca, pat):
    flags, p, x, e = _readout(B, N, Ca, pat)
    assert torch.isfinite(e["pool64"]).all() and (e["pool_bound"] >= 0).all()
    assert (e["pool64"][:, E + 1:] == 0).all()
    r = R.worst_ratio(e["pool32"], e["pool64"], e["pool_bound"])
    assert r <= 0.25, f"pool_ext in float32 at {r:.2f} of the bound"


@pytest.mark.parametrize("res,Cc,B", [(r, c, b) for r in (16, 32) for c in (96, 192) for b in (1, 3)])
def test_merge_norm_runs_bound_has_4x_headroom(res, Cc, B):
    x, o = X.merge_norm_case(B, res, Cc, _gen(res + Cc + B))
    ref, bound = X.merge_norm_expect(o)
    got, _ = X.merge_norm_expect(o, torch.float32)
    r = R.worst_ratio(got, ref, bound)
    assert r <= 0.25, f"merge_norm_runs in float32 at {r:.2f} of the bound"
    # the statistics of the partials are the gathered row's own
    assert float((ref - R.layer_norm(X.merge_gather(x.double(), B, res))).abs().max()) < 1e-4
    # a missing partial of one fine row; parts x10 / x01 exchanged
    mean, rstd, _, _ = R._ln_terms(o, torch.float64, drop=0)
    bad = (R.logical_A(o).double() - mean[:, None]) * rstd[:, None]
    assert R.worst_ratio(bad, ref, bound) > 100.0 * max(r, 1e-3)
    bad = (X.merge_gather(x.double(), B, res, swap=True) - R._ln_terms(o, torch.float64)[0][:, None]) * R._ln_terms(o, torch.float64)[1][:, None]
    assert R.worst_ratio(bad, ref, bound) > 100.0 * max(r, 1e-3)


# ----------------------------------------------------------------------------------------------------------------------------------
# formula bars and the mistakes they must catch
# ----------------------------------------------------------------------------------------------------------------------------------
def _bar_ok(f64, f32):
    bar, ref_err = R.formula_bar(f64, f32)
    assert 0.0 < bar < FWD_RTOL * float(f64.abs().max()), f"bar {bar:.3e}, cap {FWD_RTOL * float(f64.abs().max()):.3e}"
    return bar, ref_err


def _caught(bad, f64, bar, ref_err, what):
    err = float((bad - f64).abs().max())
    assert err > bar, f"{what} stays inside the bar ({err:.3e} <= {bar:.3e})"
    assert err > 100.0 * ref_err, f"{what}: only {err / ref_err:.1f} x the float32 evaluation's error"


@pytest.mark.parametrize("Ca,Cn,sc", X.PE_CONFIGS)
@pytest.mark.parametrize("B,N", [(3, 5), (2, 8)])
def test_patch_embed_bar_and_mutations(Ca, Cn, sc, B, N):
    gen = _gen(100 * Ca + Cn + N)
    T = N * N
    flags = X.make_flags(B, N, "scattered", N)
    t = X.make_pe_inputs(B, N, Ca, Cn, gen)
    cin = (2 if sc else 1) * (Ca + 2 * Cn)
    p = X.make_pe_params(cin, B, gen)
    for second in (False, True):
        for sc_on in ((False, True) if sc else (False,)):
            f = {dt: X.pe_formula(X.pe_input(t, flags, sc, sc_on, dt), p, T, second, dt) for dt in (torch.float64, torch.float32)}
            bar, ref_err = _bar_ok(f[torch.float64], f[torch.float32])
            bad = lambda **kw: X.pe_formula(X.pe_input(t, flags, sc, sc_on, **kw), p, T, second)
            _caught(bad(unmasked=True), f[torch.float64], bar, ref_err, "node part left unmasked")
            _caught(bad(swap_ij=True), f[torch.float64], bar, ref_err, "node(i) / node(j) halves swapped")
            _caught(X.pe_formula(X.pe_input(t, flags, sc, sc_on), p, T, second, neighbour_row=T), f[torch.float64], bar, ref_err,
                    "a neighbour sample's (scale | shift) row")
            if sc and not sc_on:
                _caught(X.pe_formula(X.pe_input(t, flags, sc, True), p, T, second), f[torch.float64], bar, ref_err,
                        "self-condition channels taken with has_sc == 0")


def test_patch_embed_input_follows_the_channel_order():
    """the gather against a per-token loop: [sc_adj, adj, sc_node(i), node(i), sc_node(j), node(j)]"""
    gen = _gen(5)
    B, N, Ca, Cn = 2, 5, 3, 4
    flags = X.make_flags(B, N, "scattered", 3)
    t = X.make_pe_inputs(B, N, Ca, Cn, gen)
    for sc in (0, 1):
        for sc_on in (False, True):
            got = X.pe_input(t, flags, sc, sc_on).view(B, N, N, -1)
            for b in range(B):
                for i in range(N):
                    for j in range(N):
                        m = float(flags[b, i] and flags[b, j])
                        z = lambda v: v.double() if sc_on else torch.zeros_like(v.double())
                        parts = ([z(t["sc_adj"][b, :, i, j])] if sc else []) + [t["adj"][b, :, i, j].double()]
                        parts += ([m * z(t["sc_node"][b, i])] if sc else []) + [m * t["node"][b, i].double()]
                        parts += ([m * z(t["sc_node"][b, j])] if sc else []) + [m * t["node"][b, j].double()]
                        assert torch.equal(got[b, i, j], torch.cat(parts))


@pytest.mark.parametrize("B,N,Ca,pat", RO_PATTERN_CASES)
def test_readout_bar_and_fold(B, N, Ca, pat):
    flags, p, x, e = _readout(B, N, Ca, pat)
    valid = X.pair_valid(flags)
    assert (e["out64"][~valid[:, None].expand(B, Ca, N, N)] == 0).all()
    if valid.any():
        _bar_ok(e["out64"], e["out32"])
    # the extended pooled vector times [Gn | ga] is the node head's fc1 on the pooled shared representation
    gext = torch.cat([e["fold64"]["Gn"], e["fold64"]["ga"][:, None]], 1)
    assert float((e["pool64"][:, :E + 1] @ gext.t() - e["node64"]).abs().max()) < 1e-10
    # ... and the fold rounded once to float32 stays at float32 accuracy of it
    g32 = torch.cat([e["fold32"]["Gn"], e["fold32"]["ga"][:, None]], 1).double()
    scale = max(float(e["node64"].abs().max()), 1e-30)
    assert float((e["pool64"][:, :E + 1] @ g32.t() - e["node64"]).abs().max()) <= (E + 1 + R.C_EXTRA) * R.U * max(scale, 1.0) * 8


@pytest.mark.parametrize("B,N,Ca", [(3, 5, 3), (2, 40, 3), (5, 20, 3)])
def test_readout_mutations(B, N, Ca):
    flags, p, x, e = _readout(B, N, Ca, "scattered", seed=N)
    bar, ref_err = _bar_ok(e["out64"], e["out32"])
    _, _, _, et = _readout(B, N, Ca, "scattered", seed=N, transposed=True)
    _caught(et["out64"], e["out64"], bar, ref_err, "adjacency output transposed in (i, j)")
    r32 = R.worst_ratio(e["pool32"], e["pool64"], e["pool_bound"])
    f = torch.as_tensor(flags).bool()
    w_rows = f.reshape(-1, 1).expand(B * N, N)
    for what, bad in (("pooling over j that ignores the flags", X.readout_pool(e["xn64"], flags, wgt=w_rows)),
                      ("pooling divided by the valid count", X.readout_pool(e["xn64"], flags, div=f.sum(1).clamp(min=1).repeat_interleave(N)[:, None].double()))):
        r = R.worst_ratio(bad, e["pool64"], e["pool_bound"])
        assert r > 1.0 and r > 100.0 * r32, f"{what}: {r:.2f} of the bound (float32: {r32:.3f})"
    # one pooling slot dropped for a row that straddles two 32-token tiles (every node valid: the first such row has tokens in both)
    flags, p, x, e = _readout(B, N, Ca, "all", seed=N)
    r32 = R.worst_ratio(e["pool32"], e["pool64"], e["pool_bound"])
    w = X.pair_valid(flags).reshape(B * N, N).clone()
    r = next(r for r in range(B * N) if (r * N) // 32 != (r * N + N - 1) // 32)
    w[r] &= (r * N + torch.arange(N)) // 32 == (r * N) // 32
    assert w[r].any() and not w[r].all()
    r = R.worst_ratio(X.readout_pool(e["xn64"], flags, wgt=w), e["pool64"], e["pool_bound"])
    assert r > 1.0 and r > 100.0 * r32, f"a dropped pooling slot: {r:.2f} of the bound (float32: {r32:.3f})"


@pytest.mark.parametrize("Cc", X.ROW_C)
def test_row_pass_bars_and_mutations(Cc):
    gen = _gen(300 + Cc)
    B, T = 3, 3
    M = B * T
    x = _rows(M, Cc, gen)
    gam, bet = 1.0 + 0.2 * torch.randn(Cc, generator=gen), 0.2 * torch.randn(Cc, generator=gen)
    off, ld = 8, 8 + 2 * Cc + 4
    aff = torch.randn(B, ld, generator=gen) * 0.5
    d = lambda *ts: (v.double() for v in ts)
    f64, f32 = X.ln_mod_formula(*d(x, gam, bet, aff), off, T), X.ln_mod_formula(x, gam, bet, aff, off, T)
    bar, ref_err = _bar_ok(f64, f32)
    _caught(X.ln_mod_formula(*d(x, gam, bet, aff), off, T, neighbour_row=T), f64, bar, ref_err, "ln_mod with a neighbour's row")
    f64, f32 = X.modulate(*d(x, aff), off, T), X.modulate(x, aff, off, T)
    bar, ref_err = _bar_ok(f64, f32)
    _caught(X.modulate(*d(x, aff), off, T, neighbour_row=T), f64, bar, ref_err, "mod_stats with a neighbour's row")


@pytest.mark.parametrize("Cc", (96, 128, 192, 384))
@pytest.mark.parametrize("res", (2, 4, 6))
def test_merge_ln_bar_and_mutation(Cc, res):
    gen = _gen(res * 1000 + Cc)
    B = 3
    x = _rows(B * res * res, Cc, gen)
    gam, bet = 1.0 + 0.2 * torch.randn(4 * Cc, generator=gen), 0.2 * torch.randn(4 * Cc, generator=gen)
    f64, f32 = X.merge_ln_formula(x.double(), gam.double(), bet.double(), B, res), X.merge_ln_formula(x, gam, bet, B, res)
    bar, ref_err = _bar_ok(f64, f32)
    _caught(X.merge_ln_formula(x.double(), gam.double(), bet.double(), B, res, swap=True), f64, bar, ref_err, "parts x01 / x10 swapped")


@pytest.mark.parametrize("D", X.BREAKUP_D)
@pytest.mark.parametrize("res", (1, 2, 3, 4))
def test_breakup_ln_bar_and_mutation(D, res):
    gen = _gen(res * 7000 + D)
    B = 3
    y = _rows(B * res * res, D, gen)
    rn = lambda n: torch.randn(n, generator=gen)
    gam, bet, pg, pb = 1.0 + 0.2 * rn(D), 0.2 * rn(D), 1.0 + 0.2 * rn(D // 4), 0.2 * rn(D // 4)
    args64 = [t.double() for t in (y, gam, bet, pg, pb)]
    f64, f32 = X.breakup_formula(*args64, B, res), X.breakup_formula(y, gam, bet, pg, pb, B, res)
    bar, ref_err = _bar_ok(f64, f32)
    _caught(X.breakup_formula(*args64, B, res, swap=True), f64, bar, ref_err, "di / dj swapped")
    # chunk q of coarse token (i, j) lands on fine token (2i + (q & 1), 2j + (q >> 1))
    n = R.layer_norm(args64[0], args64[1], args64[2]).view(B, res, res, 4, D // 4)
    b, i, j, q = B - 1, res - 1, 0, 1
    want = R.layer_norm(n[b, i, j, q][None], args64[3], args64[4])[0]
    got = f64.view(B, 2 * res, 2 * res, D // 4)[b, 2 * i + 1, 2 * j + 0]
    assert float((got - want).abs().max()) < 1e-12


def test_unfused_tail_bars_and_mutations():
    gen = _gen(11)
    B, N, Ee, Ca, Cn = 3, 5, 96, 3, 7
    flags = X.make_flags(B, N, "scattered", 1)
    h = torch.randn(B * N * N, Ee, generator=gen) + 0.5
    W, bias = torch.randn(Ca, Ee, generator=gen) / Ee ** 0.5, torch.randn(Ca, generator=gen) * 0.3
    f64, f32 = X.head_adj_formula(h.double(), W.double(), bias.double(), flags), X.head_adj_formula(h, W, bias, flags)
    bar, ref_err = _bar_ok(f64, f32)
    _caught(f64.transpose(2, 3), f64, bar, ref_err, "adjacency head transposed in (i, j)")
    f64, f32 = X.pool_formula(h.double(), flags), X.pool_formula(h, flags)
    bar, ref_err = _bar_ok(f64, f32)
    _caught(X.pool_formula(h.double(), flags, ignore_flags=True), f64, bar, ref_err, "pooling over j that ignores the flags")
    _caught(X.pool_formula(h.double(), flags, by_count=True), f64, bar, ref_err, "pooling divided by the valid count")
    hn = torch.randn(B * N, Ee, generator=gen)
    Wn, bn = torch.randn(Cn, Ee, generator=gen) / Ee ** 0.5, torch.randn(Cn, generator=gen) * 0.3
    f64, f32 = X.head_node_formula(hn.double(), Wn.double(), bn.double(), flags), X.head_node_formula(hn, Wn, bn, flags)
    bar, ref_err = _bar_ok(f64, f32)
    _caught(X.head_node_formula(hn.double(), Wn.double(), bn.double(), np.ones_like(flags)), f64, bar, ref_err, "node head left unmasked")


# ----------------------------------------------------------------------------------------------------------------------------------
# packers, case lists, copies
# ----------------------------------------------------------------------------------------------------------------------------------
def test_edge_packers_follow_the_index_formulas():
    """pe_wp[nt][s][lane][t] = Wpe_padded[32nt + (lane&31)][8s + 4(lane>>5) + t] (S = Kp / 8); fap the same on Fa [96, 96] (S = 12);
    f2p[nt][g][lane][t] = (lane&31) < Ca ? F2[lane&31][32nt + 8g + 4(lane>>5) + t] : 0 -- the loops of dsg_finalize_weights"""
    for Kp, cin in ((32, 26), (32, 32), (64, 52), (64, 64)):
        S = Kp // 8
        w = (np.arange(E * cin, dtype=np.float32) + 1.0).reshape(E, cin)
        dst = X.pad_k(torch.from_numpy(w), Kp).numpy()
        pk = np.empty(E * Kp, np.float32)
        for nt in range(3):
            for s in range(S):
                for lane in range(64):
                    for t in range(4):
                        pk[((nt * S + s) * 64 + lane) * 4 + t] = dst[32 * nt + (lane & 31), 8 * s + 4 * (lane >> 5) + t]
        assert np.array_equal(R.pack_rows(dst), pk)
    Fa = (np.arange(E * E, dtype=np.float32) + 0.5).reshape(E, E)
    fap = np.empty(E * E, np.float32)
    for nt in range(3):
        for s in range(12):
            for lane in range(64):
                for t in range(4):
                    fap[((nt * 12 + s) * 64 + lane) * 4 + t] = Fa[32 * nt + (lane & 31), 8 * s + 4 * (lane >> 5) + t]
    assert np.array_equal(R.pack_rows(Fa), fap)
    for Ca in (1, 3, 6, 32):
        F2 = (np.arange(Ca * E, dtype=np.float32) + 1.0).reshape(Ca, E)
        f2p = np.zeros(3 * 4 * 64 * 4, np.float32)
        for nt in range(3):
            for g in range(4):
                for lane in range(64):
                    for t in range(4):
                        c = lane & 31
                        f2p[((nt * 4 + g) * 64 + lane) * 4 + t] = F2[c, 32 * nt + 8 * g + 4 * (lane >> 5) + t] if c < Ca else 0.0
        pad = np.zeros((32, E), np.float32)
        pad[:Ca] = F2
        assert np.array_equal(R.pack_cols(pad), f2p)


def test_committed_readout_cases_reach_the_shortcut_and_the_mixed_wave():
    shortcut = mixed = met = 0
    for (B, N, Ca, pat) in RO_PATTERN_CASES:
        s, m, t = X.wave_classes(X.make_flags(B, N, pat))
        shortcut, mixed, met = shortcut + s, mixed + m, met + t
    assert shortcut >= 1 and mixed >= 1 and met >= 1
    # the prefix pattern holds a graph without a valid node and one with a single valid node from B = 3 on
    f = X.make_flags(5, 20, "prefix")
    assert sorted(f.sum(1).tolist()) == [0, 1, 10, 19, 20]
    # rows that straddle tiles, a last tile with 11 rows' worth of tokens, and a second block with one live lane
    assert (3 * 5 * 5) % 32 == 11 and 129 % 128 == 1 and X.readout_segments(33) == 2 and X.readout_segments(34) == 3


def test_window_copy_references():
    """window order t = 8 row + col; a listed window takes its graph's representative; -1, out-of-range and self entries copy nothing"""
    res, B, Cc = 16, 2, 4
    assert X.window_rows(res, 3).tolist()[:9] == [8 * 16 + 8 + k for k in range(8)] + [9 * 16 + 8]
    x = np.arange(B * res * res * Cc, dtype=np.float32).reshape(B * res * res, Cc)
    (out,) = X.broadcast_expect([x], B, res, [1, -1, 99, 4, 5, 2], 5, [0, 5])
    assert np.array_equal(out[X.window_rows(res, 1)], x[X.window_rows(res, 0)])
    assert np.array_equal(out[256 + X.window_rows(res, 0)], x[256 + X.window_rows(res, 1)])
    untouched = np.ones(B * res * res, bool)
    untouched[X.window_rows(res, 1)] = untouched[256 + X.window_rows(res, 0)] = False
    assert np.array_equal(out[untouched], x[untouched])
