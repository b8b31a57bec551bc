"""CPU: the power of tests/test_train_kernels.py -- its float64 references and bars (tests/train_ref.py) on their own.  The explicit
backward formulas equal float64 autograd; a correct fp32 evaluation in ANOTHER summation order (plain float32 torch) passes every
derived product bound with 4x headroom; seeded wrong results -- the mistakes a tiled, sliced kernel actually makes -- fail their bar, by
orders of magnitude where the bar is derived, at both ends of the K lists; and the transcriptions of the launchers' slice arithmetic
that choose the inputs reproduce the edges the cases were written for."""
import pytest
import torch

import train_ref as R
from train_ref import AttnCase, TGemmCase

F64, F32 = torch.float64, torch.float32


def _ids(cases):
    return [c.ident() for c in cases]


# ---- the slice arithmetic -------------------------------------------------------------------------------------------------------
def test_slice_transcriptions_reproduce_the_edges():
    for K, (S, last) in R.TN_K_TABLE.items():
        s, ks, l = R.tn_slices(96, 96, K)
        assert (s, l) == (S, last) and ks % 32 == 0 and (s - 1) * ks < K <= s * ks
    assert R.tn_slices(96, 96, 2049)[1] == 544 and R.tn_slices(96, 96, 2048)[1] == 512
    assert min(256, 9217 // 512) == 18 and R.tn_slices(96, 96, 9217)[0] == 17          # the count drops after rounding kslice
    for K, (S, last) in R.PLAIN_K_TABLE.items():
        s, ks, l = R.plain_slices(33, 33, K)
        assert (s, l) == (S, last) and (s - 1) * ks < K <= s * ks
    assert min(64, 34817 // 1024) == 34 and R.plain_slices(33, 33, 34817)[0] == 33
    assert R.plain_slices(33, 33, 4095)[0] == 1 and R.plain_slices(33, 33, 4096, bias=True)[0] == 1
    # the three forms of the reducer are all reached by the K list on 96 x 96
    assert {R.reducer_lanes(96, 96, R.tn_slices(96, 96, K)[0]) for K in R.TN_K_TABLE} == {1, 4, 16}
    assert R.modulate_chunks(4097) == (64, 65, 2) and R.modulate_chunks(64) == (1, 64, 64) and R.modulate_chunks(65) == (2, 64, 1)
    assert R.ln_bwd_blocks(4097)[2] == 1 and R.ln_bwd_blocks(17) == (5, 4, 1) and R.ln_bwd_blocks(8193)[1] == 12
    assert {R.ln_form(c) for c in R.LN_C} == {(32, 1), (64, 1), (64, 2), (64, 3), (64, 6)}
    for lo, hi in ((128, 132), (256, 260), (512, 516), (768, 772)):                      # both sides of every switch
        assert lo in R.LN_C and hi in R.LN_C and R.ln_form(lo) != R.ln_form(hi)


def test_cases_cover_what_they_claim():
    tn = R.tn_cases()
    assert all(R.expected_route(c)[0] == R.ROUTE_TN for c in tn)
    for K in (2049, 8705):
        assert {c.M for c in tn if c.K == K} >= set(R.TN_M) and {c.N for c in tn if c.K == K} >= set(R.TN_N)
    for mn in ((96, 96), (130, 200)):
        assert {c.K for c in tn if (c.M, c.N) == mn} >= set(R.TN_K_TABLE)
    assert any(c.M == 6 and c.lda == 6 for c in tn) and any(c.lda % 4 and c.ldb % 4 for c in tn)
    assert any(c.pa and c.pc for c in tn) and any(c.pb for c in tn) and any(c.acc for c in tn) and any(not c.colsum for c in tn)
    mf = R.mfma_cases()
    r1 = [c for c in mf if R.expected_route(c)[0] == R.ROUTE_MFMA]
    assert {c.K for c in r1 if c.tb} >= {32, 96, 160, 4, 36, 60} and {c.M for c in r1} == {512, 513, 640}
    assert {c.act for c in r1} == {R.ACT_NONE, R.ACT_GELU_KEEP, R.ACT_DGELU} and any(c.res for c in r1) and any(c.acc for c in r1)
    out = [c for c in mf if R.expected_route(c)[0] == R.ROUTE_PLAIN]
    assert any(c.M == 511 for c in out) and any(c.N == 48 for c in out) and any(c.lda != c.K for c in out)
    pl = R.plain_cases()
    assert {R.expected_route(c)[0] for c in pl} == {R.ROUTE_PLAIN, R.ROUTE_PLAIN_SPLITK}
    assert {(c.ta, c.tb) for c in pl if c.K <= 65} == {(a, b) for a in (False, True) for b in (False, True)}
    for v in R.PLAIN_SIZES:
        assert any(c.M == v for c in pl) and any(c.N == v for c in pl) and any(c.K == v for c in pl)
    assert {c.K for c in pl if R.expected_route(c)[0] == R.ROUTE_PLAIN_SPLITK} >= set(R.PLAIN_K_TABLE)
    at = R.attn_cases()
    for ws in (2, 4, 5, 6, 7, 8, 9, 10, 11):
        assert any(c.ws == ws and c.shift == 0 for c in at) and any(c.ws == ws and c.shift > 0 and c.res == 3 * ws for c in at)
    assert {c.heads for c in at} == {1, 3} and {c.B for c in at} == {1, 3} and any(c.shift == 1 for c in at)
    assert {c[0] for c in R.ln_cases()} >= set(R.LN_M) | {4097, 8193} and {c[1] for c in R.ln_cases()} == set(R.LN_C)
    assert {c[1] for c in R.modulate_cases()} == set(R.MOD_T) and {c[2] for c in R.modulate_cases()} == set(R.MOD_C)


# ---- products ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.all_tgemm_cases(), ids=_ids(R.all_tgemm_cases()))
def test_float32_evaluation_has_4x_headroom(case):
    o = R.make_tgemm(case)
    ref, f32 = R.tgemm_expect(o), R.tgemm_expect(o, F32)
    for k in ("C", "C2", "cs"):
        if k in ref:
            assert torch.isfinite(ref[k]).all() and (ref["b" + k] > 0).all()
            r = R.worst_ratio(f32[k], ref[k], ref["b" + k])
            assert r <= 0.25, f"{k}: float32 evaluation at {r:.2f} of the bound"


MUT_BASE = {   # both K ends of each route's list
    "drop_last_row": [TGemmCase(True, False, 96, 96, 2048, seed=1), TGemmCase(True, False, 96, 96, 32768, seed=2), TGemmCase(True, False, 96, 96, 8705, seed=3),
                      TGemmCase(True, False, 33, 33, 4096, force_plain=True, seed=4), TGemmCase(False, True, 33, 33, 34817, force_plain=True, seed=5),
                      TGemmCase(False, True, 512, 96, 32, bias=True, seed=6), TGemmCase(False, True, 512, 96, 160, bias=True, seed=7),
                      TGemmCase(True, True, 33, 31, 65, seed=8)],
    "drop_chunk": [TGemmCase(True, False, 130, 200, 2048, seed=9), TGemmCase(True, False, 130, 200, 32768, seed=10),
                   TGemmCase(True, False, 33, 33, 4096, force_plain=True, seed=11), TGemmCase(True, False, 33, 33, 34817, force_plain=True, seed=12),
                   TGemmCase(False, False, 640, 96, 384, seed=13), TGemmCase(False, True, 512, 96, 60, bias=True, seed=14),
                   TGemmCase(False, False, 33, 33, 65, seed=15)],
    "swap_rows": [TGemmCase(True, False, 129, 97, 2048, acc=True, seed=16), TGemmCase(True, False, 129, 97, 32768, seed=17),
                  TGemmCase(False, True, 65, 33, 1, bias=True, seed=18), TGemmCase(False, True, 65, 33, 65, seed=19)],
    "colsum_shift": [TGemmCase(True, False, 6, 96, 2048, colsum=True, seed=20), TGemmCase(True, False, 130, 96, 32768, colsum=True, seed=21),
                     TGemmCase(True, False, 33, 33, 31, colsum=True, seed=22), TGemmCase(True, False, 33, 33, 34817, colsum=True, force_plain=True, seed=23)],
}
MUT_CASES = [(m, c) for m, cs in MUT_BASE.items() for c in cs]


@pytest.mark.parametrize("mutation,case", MUT_CASES, ids=[f"{m}-{c.ident()}" for m, c in MUT_CASES])
def test_wrong_products_fail_the_bound(mutation, case):
    o = R.make_tgemm(case)
    ref, bad, f32 = R.tgemm_expect(o), R.tgemm_expect(o, mutate=mutation), R.tgemm_expect(o, F32)
    k = "cs" if mutation == "colsum_shift" else "C"
    r = R.worst_ratio(bad[k], ref[k], ref["b" + k])
    assert r > 1.0, f"{mutation} stays inside the bound ({r:.2f})"
    assert r > 100.0 * R.worst_ratio(f32[k], ref[k], ref["b" + k])


# ---- attention -------------------------------------------------------------------------------------------------------------------
HOST_ATTN = [AttnCase(5, 2, 3, 15, 2, seed=1), AttnCase(11, 5, 1, 33, 1, seed=2), AttnCase(4, 1, 3, 8, 3, seed=3), AttnCase(8, 0, 1, 16, 1, seed=4)]


def test_swin_tokens_are_the_rolled_partition():
    for res, ws, shift in ((8, 4, 0), (8, 4, 1), (15, 5, 2), (33, 11, 5)):
        assert torch.equal(R.swin_tokens(res, ws, shift), torch.from_numpy(R.window_tokens(res, ws, shift)))


@pytest.mark.parametrize("case", HOST_ATTN, ids=_ids(HOST_ATTN))
def test_attention_formulas_equal_autograd(case):
    o = R.make_attn(case)
    out, gq, gt = R.attn_autograd(o)
    e_out, e_q, e_t = R.attn_explicit(o)
    assert float((out - e_out).abs().max()) < 1e-12 and float((gq - e_q).abs().max()) < 1e-12 and float((gt - e_t).abs().max()) < 1e-12
    assert float((R.attn_forward(o) - e_out).abs().max()) < 1e-12
    if case.shift > 0:   # the mask reaches the result: some probabilities are switched off
        assert float((R.attn_explicit(o, mutate="bwd_no_mask")[1] - e_q).abs().max()) > 1e-3


@pytest.mark.parametrize("mutation", R.ATTN_MUTATIONS)
@pytest.mark.parametrize("case", HOST_ATTN[:3], ids=_ids(HOST_ATTN[:3]))
def test_wrong_attention_fails_the_bar(case, mutation):
    o = R.make_attn(case)
    ref, f32, bad = R.attn_explicit(o), R.attn_explicit(o, F32), R.attn_explicit(o, mutate=mutation)
    hit = {"bwd_no_mask": (1, 2), "dk_no_scale": (1,), "dtable_drop_window": (2,), "padded_key": (0, 1, 2)}[mutation]
    for i in range(3):
        bar, ref_err = R.formula_bar(ref[i], f32[i])
        err = float((bad[i] - ref[i]).abs().max())
        if i in hit:
            assert err > 100.0 * bar, f"{mutation}: output {i} moves by {err:.3e}, bar {bar:.3e}"
        else:
            assert err == 0.0


# ---- LayerNorm, modulate ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,C", [(5, 4), (17, 100), (9, 772)])
def test_layernorm_backward_equals_autograd(M, C):
    o = R.ln_inputs(M, C, 1)
    x, gam, bet = o["x"].double().requires_grad_(True), o["gam"].double().requires_grad_(True), o["bet"].double().requires_grad_(True)
    y = torch.nn.functional.layer_norm(x, (C,), gam, bet, R.LN_EPS)
    gx, gg, gb = torch.autograd.grad((y * o["dy"].double()).sum(), (x, gam, bet))
    yf, st = R.ln_fwd(x.detach(), gam.detach(), bet.detach())
    dx, dg, db = R.ln_bwd(x.detach(), gam.detach(), st, o["dy"].double(), o["dx_in"].double())
    assert float((yf - y.detach()).abs().max()) < 1e-12
    assert float((dx - o["dx_in"].double() - gx).abs().max()) < 1e-12 and float((dg - gg).abs().max()) < 1e-12 and float((db - gb).abs().max()) < 1e-12


@pytest.mark.parametrize("B,T,C", [(3, 65, 60), (1, 129, 4)])
def test_modulate_backward_equals_autograd(B, T, C):
    o = R.modulate_inputs(B, T, C, 2)
    x, aff = o["x"].double().requires_grad_(True), o["aff"].double().requires_grad_(True)
    b = torch.arange(B * T) // T
    y = torch.nn.functional.silu(aff[b, C:] + x * (1.0 + aff[b, :C]))
    gx, ga = torch.autograd.grad((y * o["dy"].double()).sum(), (x, aff))
    dx, da = R.modulate_bwd(x.detach(), aff.detach(), o["dy"].double(), T)
    assert float((R.modulate_fwd(x.detach(), aff.detach(), T) - y.detach()).abs().max()) < 1e-12
    assert float((dx - gx).abs().max()) < 1e-12 * max(1.0, float(gx.abs().max())) and float((da - ga).abs().max()) < 1e-12 * max(1.0, float(ga.abs().max()))


@pytest.mark.parametrize("M,C", [(17, 96), (4097, 132)])
def test_dgamma_without_the_last_row_block_fails_the_bar(M, C):
    o = R.ln_inputs(M, C, 3)
    st = R.ln_fwd(o["x"].double(), o["gam"].double(), o["bet"].double())[1].float()
    ref = R.ln_bwd(o["x"].double(), o["gam"].double(), st.double(), o["dy"].double())
    f32 = R.ln_bwd(o["x"], o["gam"], st, o["dy"])
    bad = R.ln_bwd(o["x"].double(), o["gam"].double(), st.double(), o["dy"].double(), drop_rows=R.ln_bwd_blocks(M)[2])
    for i in (1, 2):
        bar, _ = R.formula_bar(ref[i], f32[i])
        assert float((bad[i] - ref[i]).abs().max()) > 100.0 * bar


@pytest.mark.parametrize("B,T,C", [(3, 65, 60), (3, 4097, 4)])
def test_daff_from_the_neighbouring_sample_fails_the_bar(B, T, C):
    o = R.modulate_inputs(B, T, C, 4)
    ref = R.modulate_bwd(o["x"].double(), o["aff"].double(), o["dy"].double(), T)
    f32 = R.modulate_bwd(o["x"], o["aff"], o["dy"], T)
    bad = R.modulate_bwd(o["x"].double(), o["aff"].double(), o["dy"].double(), T, neighbour=True)
    bar, _ = R.formula_bar(ref[1], f32[1])
    assert float((bad[1] - ref[1]).abs().max()) > 100.0 * bar


# ---- Adam ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 3])
def test_adam_without_bias_correction_fails_the_bar(step):
    p, g, m, v = R.adam_inputs(R.ADAM_SIZES, 5)
    hp = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, max_norm=1.0)
    ref, f32 = R.adam_step(p, g, m, v, step, **hp), R.adam_step(p, g, m, v, step, dt=F32, **hp)
    bad = R.adam_step(p, g, m, v, step, bias_correction=False, **hp)
    cat = lambda ts: torch.cat([t.reshape(-1) for t in ts])
    bar, _ = R.formula_bar(cat(ref[0]), cat(f32[0]))
    assert float((cat(bad[0]) - cat(ref[0])).abs().max()) > 100.0 * bar
    # the reference is torch.optim.Adam behind clip_grad_norm_
    q = [t.double().clone().requires_grad_(True) for t in p]
    opt = torch.optim.Adam(q, lr=float(torch.tensor(1e-3)), betas=(float(torch.tensor(0.9)), float(torch.tensor(0.999))),
                           eps=float(torch.tensor(1e-8)), weight_decay=float(torch.tensor(0.01)))
    for s in range(1, step + 1):
        for t, gt in zip(q, g):
            t.grad = gt.double().clone()
        tn = torch.nn.utils.clip_grad_norm_(q, 1.0)
        opt.step()
    if step == 1:
        assert abs(float(tn) - ref[4]) < 1e-12 * ref[4]
        assert float((cat([t.detach() for t in q]) - cat(ref[0])).abs().max()) < 1e-12
