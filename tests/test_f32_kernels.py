"""GPU: the kernels of the DEFAULT fp32 path on their own (csrc/kernels.hip: gemm4_f32_kernel in all its template forms and its fused
QKV + window-attention epilogue, window_attn_kernel, fused_mlp_kernel, fused_attn96_kernel) through the dsg_debug_*_f32 hooks.  EVERY
output element is compared with a float64 evaluation of the same operation on the same fp32 operands (tests/f32_ref.py), at the
smallest shapes that reach each tile edge: one k-chunk, odd chunk counts, a last column tile with one or two of its three slabs, nine
row tiles (the XCD swizzle's second group), sample boundaries inside a tile, sentinel runs, device-side counts.

Output buffers are filled with NaN before the launch and carry padding columns and guard rows: what the kernel must write has to be
finite and inside the bar, everything else -- padding, rows of unlisted runs or windows, rows beyond a device-side count, the guard
rows -- bit-identical afterwards.

Bars (derived in tests/f32_ref.py, none of them from a kernel's output): the GEMM forms get a per-element bound from the float64
reference's own quantities; attention and the fused block kernels get 8x the error of a float32 torch evaluation of the same formula,
capped at 1e-4 of the output scale.  Measured figures per case family: profiles/f32_kernel_errors.md (each test prints its own)."""
import ctypes as C

import numpy as np
import pytest
import torch

import f32_ref as R
from f32_ref import GemmCase

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000
GUARD = 2      # rows behind every output buffer


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev(t, dtype=None):
    return None if t is None else (t if dtype is None else t.to(dtype)).contiguous().cuda()


def _nan(rows, cols):
    return torch.full((rows + GUARD, cols), float("nan"), device="cuda")


def _untouched(buf):
    """[rows, cols] bool: the element still holds the NaN fill, bit for bit"""
    return buf.view(torch.int32).cpu() == NAN_BITS


def _rows_mask(M, runs):
    m = torch.zeros(M + GUARD, dtype=torch.bool)
    if runs is None:
        m[:M] = True
    else:
        for r in runs:
            m[8 * r:8 * r + 8] = True
    return m


def _check_written(buf, N, rows, ref, bound, what):
    """buf [M + GUARD, ld] from the device: rows `rows`, columns < N hold the reference within the bound; all else is untouched"""
    got, keep = buf.cpu(), _untouched(buf)
    must = torch.zeros_like(keep)
    must[rows, :N] = True
    assert keep[~must].all(), f"{what}: {int((~keep[~must]).sum())} elements written outside the rows / columns of the result"
    M = ref.shape[0]
    sel = rows[:M]
    assert torch.isfinite(got[:M][sel][:, :N]).all(), f"{what}: non-finite values in the result"
    r = R.worst_ratio(got[:M][sel][:, :N], ref[sel], bound[sel])
    print(f"F32KGEMM {what} worst |err| / bound = {r:.3f}")
    assert r <= 1.0, f"{what}: {r:.2f} x the derived bound"
    return got


def run_gemm_case(c: GemmCase):
    from diffusesg_amd import lib as L
    lib = L.load()
    o = R.make_gemm(c)
    ref = R.gemm_expect(o)
    a = L.DsgGemmF32Args()
    keep = [_dev(o["A"]), _dev(o.get("A2")), _dev(o["W"]), _dev(o["bias"]), _dev(o.get("ln_stats")), _dev(o.get("ln_part")), _dev(o.get("res")),
            _dev(o.get("mod_aff"))]
    dA, dA2, dW, db, dst, dpt, dres, dmod = keep
    out_C = _nan(c.M, o["ldc"])
    out_C2 = _nan(c.M, o["ldc2"]) if "C2" in ref else None
    out_S = _nan(c.M, 2 * c.tiles_n) if c.epi >= 1 else None
    d_list = d_cnt = None
    if c.cnt >= 0:
        d_list = torch.tensor(o["row_list"], dtype=torch.int32, device="cuda")
        d_cnt = torch.tensor([c.cnt], dtype=torch.int32, device="cuda")
    for name, t in (("A", dA), ("A2", dA2), ("W", dW), ("bias", db), ("ln_stats", dst), ("ln_part", dpt), ("res", dres), ("C", out_C), ("C2", out_C2),
                    ("mod_aff", dmod), ("stats_out", out_S), ("row_list", d_list), ("row_cnt", d_cnt)):
        setattr(a, name, None if t is None else t.data_ptr())
    a.lda, a.lda2, a.K1, a.ln_nparts = o["lda"], o.get("lda2", 0), c.K1, (c.nparts if c.ln == "part" else 0)
    a.ldres, a.ldc, a.ldc2 = (o["ldres"] if c.res else 0), o["ldc"], (o["ldc2"] if out_C2 is not None else 0)
    a.M, a.N, a.K, a.act = c.M, c.N, c.K, c.act
    a.mod_ld, a.mod_off, a.mod_T, a.a4_res = o.get("mod_ld", 0), c.mod_off, c.mod_T, c.a4_res
    rc = lib.dsg_debug_gemm_f32(C.byref(a), None)
    assert rc == 0, f"dsg_debug_gemm_f32 refused {c.ident()} (status {rc})"
    rows = _rows_mask(c.M, o.get("runs") if c.cnt >= 0 else None)
    got_C = _check_written(out_C, c.N, rows, ref["C"], ref["bC"], "C")
    if out_C2 is not None:
        _check_written(out_C2, c.N, rows, ref["C2"], ref["bC2"], "C2")
    if out_S is not None:
        # float64 sums of the values the kernel STORED, over each tile's valid columns only; the bar from the reference's magnitudes
        S, Bd = R.stats_expect(torch.nan_to_num(got_C[:c.M, :c.N]), c, ref["C"], ref["bC"])
        _check_written(out_S, 2 * c.tiles_n, rows, S.reshape(c.M, -1), Bd.reshape(c.M, -1), "stats_out")


def _ids(cases):
    return [c.ident() for c in cases]


@pytest.mark.parametrize("case", R.plain_cases(), ids=_ids(R.plain_cases()))
def test_gemm_plain_forms(case):
    """AMODE 0: LN x {none, GELU, SiLU} x res, ln_stats and ln_part, every M / N / K edge with every variant; the last two cases have
    lda > K, ldc > N, ldres != ldc and a dual store with ldc2 != ldc"""
    run_gemm_case(case)


@pytest.mark.parametrize("case", R.concat_cases(), ids=_ids(R.concat_cases()))
def test_gemm_a2_concat(case):
    """two sources along K with lda2 != lda: (K1, K) = (32, 64), (96, 192) -- an odd chunk count from the first source --, (64, 96)"""
    run_gemm_case(case)


@pytest.mark.parametrize("case", R.ln_part_cases(), ids=_ids(R.ln_part_cases()))
def test_gemm_ln_part(case):
    """LayerNorm statistics from 1, 2, 3, 4 and 8 partial (sum, sumsq) pairs; row means of up to two standard deviations"""
    run_gemm_case(case)


@pytest.mark.parametrize("case", R.train_cases(), ids=_ids(R.train_cases()))
def test_gemm_training_forms(case):
    """ACT_GELU_KEEP: C2 = the pre-activation, C = its GELU; ACT_DGELU: the product times GELU'(res), nothing added"""
    run_gemm_case(case)


@pytest.mark.parametrize("case", R.epi_cases(), ids=_ids(R.epi_cases()))
def test_gemm_epilogue_extensions(case):
    """EPI 1/2/3: row statistics, batch-uniform and per-sample modulate + SiLU (36-row samples in 128-row tiles, mod_off != 0), with and
    without res, C2 = the un-modulated value"""
    run_gemm_case(case)


@pytest.mark.parametrize("case", R.merge_cases(), ids=_ids(R.merge_cases()))
def test_gemm_merge_gather(case):
    """AMODE 1: the PatchMerging gather with LayerNorm(4C) from the fine rows' partials, EPI 0 / 2 / 3, dual store"""
    run_gemm_case(case)


@pytest.mark.parametrize("case", R.rowlist_cases(), ids=_ids(R.rowlist_cases()))
def test_gemm_row_list(case):
    """AMODE 3: only the listed 8-row runs are computed and stored; sentinel runs and tiles beyond the device-side count write nothing"""
    run_gemm_case(case)


def test_gemm_refuses_forms_that_are_not_built():
    """the hook returns DSG_ERR_INVALID (never aborts) where launch_gemm has no kernel"""
    from diffusesg_amd import lib as L
    lib = L.load()
    o = R.make_gemm(GemmCase(16, 96, 32, ln="stats", seed=1))
    dA, dW, dst = _dev(o["A"]), _dev(o["W"]), _dev(o["ln_stats"])
    out_C, out_S = _nan(16, 96), _nan(16, 2)
    d_list = torch.tensor([0, 1] + [-1] * 14, dtype=torch.int32, device="cuda")
    d_cnt = torch.tensor([2], dtype=torch.int32, device="cuda")

    def call(**kw):
        a = L.DsgGemmF32Args()
        a.A, a.W, a.C, a.lda, a.ldc, a.M, a.N, a.K = dA.data_ptr(), dW.data_ptr(), out_C.data_ptr(), 32, 96, 16, 96, 32
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.dsg_debug_gemm_f32(C.byref(a), None)
    assert call() == 0
    assert call(K=40) == L.DSG_ERR_INVALID                                                    # K % 32
    assert call(ln_stats=dst.data_ptr(), stats_out=out_S.data_ptr()) == L.DSG_ERR_INVALID     # statistics behind a LayerNorm prologue
    assert call(act=R.ACT_GELU_KEEP) == L.DSG_ERR_INVALID                                     # no C2 for the kept pre-activation
    assert call(act=R.ACT_DGELU) == L.DSG_ERR_INVALID                                         # no res to differentiate at
    assert call(a4_res=4, M=4, K=128) == L.DSG_ERR_INVALID                                    # the gather needs ln_part
    assert call(row_list=d_list.data_ptr()) == L.DSG_ERR_INVALID                              # a list without its count
    assert call(row_list=d_list.data_ptr(), row_cnt=d_cnt.data_ptr(), act=R.ACT_SILU) == L.DSG_ERR_INVALID
    assert call(act=7) == L.DSG_ERR_INVALID


# ----------------------------------------------------------------------------------------------------------------------------------
# attention and the fused block kernels: the bar is 8x the float32 formula's own error, at most 1e-4 of the output scale
# ----------------------------------------------------------------------------------------------------------------------------------
def _check_formula(family, got, f64, f32, rows=None):
    """got [M, C] (CPU) against the float64 formula on the rows the kernel had to write"""
    bar, ref_err = R.formula_bar(f64, f32)
    sel = slice(None) if rows is None else rows
    assert torch.isfinite(got[sel]).all(), f"{family}: non-finite values in the result"
    err = float((got[sel].double() - f64[sel]).abs().max()) if got[sel].numel() else 0.0
    print(f"F32KERR {family} bar={bar:.3e} ref_err={ref_err:.3e} kern_err={err:.3e} scale={float(f64.abs().max()):.3e}")
    assert err <= bar, f"{family}: max error {err:.3e} above the bar {bar:.3e} (float32 formula: {ref_err:.3e})"


def _qkv_weights(Cc, K, gen):
    W = torch.randn(3 * Cc, K, generator=gen) / K ** 0.5
    W[:Cc] *= 32 ** -0.5 * R.LOG2E                      # q rows arrive pre-scaled by d^-1/2 log2(e)
    bq = torch.randn(3 * Cc, generator=gen) * 0.2
    bq[:Cc] *= 32 ** -0.5 * R.LOG2E
    return W, bq


def _window_rows(B, res, ws, shift, wins):
    """bool [B res^2]: the token rows of the listed windows (b nW + w)"""
    tok, T, nW = R.window_tokens(res, ws, shift), res * res, (res // ws) ** 2
    m = torch.zeros(B * T, dtype=torch.bool)
    for gw in wins:
        m[(gw // nW) * T + torch.from_numpy(tok[gw % nW])] = True
    return m


# (ws, B, res, shift, heads, ln kind, window list, count): the list may hold -1 and stale entries behind the count
EPI4_CASES = [
    (8, 1, 8, 0, 1, "stats", None, 0),              # K = 32: one chunk; the second window of the only tile is absent
    (8, 3, 8, 0, 3, "part", None, 0),               # three windows: the last tile holds one
    (8, 2, 16, 4, 3, "stats", None, 0),
    (8, 1, 16, 4, 6, "part", None, 0),              # K = 192: ln_part with two partials
    (10, 1, 10, 0, 3, "stats", None, 0),
    (10, 2, 20, 5, 3, "part", None, 0),
    (8, 3, 8, 0, 3, "stats", [2, -1, 0, 1], 3),     # odd count, a -1 entry, a stale entry behind the count
    (8, 2, 16, 4, 3, "part", [0, 3, -1, 5, 6, 7, 1], 5),
    (8, 2, 16, 4, 3, "stats", [4, 2], 0),           # count 0: nothing is written
]


@pytest.mark.parametrize("ws,B,res,shift,heads,ln,wlist,wcnt", EPI4_CASES)
def test_gemm_qkv_attn_epilogue(ws, B, res, shift, heads, ln, wlist, wcnt):
    """EPI 4: LayerNorm -> QKV -> softmax(q k^T + bias) v in the GEMM's epilogue, 8 x 8 (two windows per tile) and 10 x 10 windows,
    with and without a window list"""
    from diffusesg_amd import lib as L
    lib = L.load()
    Cc, T, nW = 32 * heads, res * res, (res // ws) ** 2
    K, M = Cc, B * res * res
    gen = torch.Generator().manual_seed(3100 + EPI4_CASES.index((ws, B, res, shift, heads, ln, wlist, wcnt)))     # one seed per case
    x = torch.randn(M, K, generator=gen) + 2.0 * (2.0 * torch.rand(M, 1, generator=gen) - 1.0)
    W, bq = _qkv_weights(Cc, K, gen)
    bias = R.make_attn_bias(nW, heads, ws, shift, gen)
    o = {"case": GemmCase(M, 3 * Cc, K, ln=ln)}
    if ln == "stats":
        xd = x.double()
        o["ln_stats"] = torch.stack([xd.mean(1), (xd.var(1, unbiased=False) + R.LN_EPS) ** -0.5], 1).float()
    else:
        o["ln_part"] = R._partials(x.double())
    f = {}
    for dt in (torch.float64, torch.float32):
        mean, rstd, _, _ = R._ln_terms(o, dt)
        f[dt] = R.qkv_attn_formula(x.to(dt), W.to(dt), bq.to(dt), mean, rstd, bias, B, res, ws, shift, heads)
    dx, dW, dbq, dbias, dst, dpt = _dev(x), _dev(W), _dev(bq), _dev(bias), _dev(o.get("ln_stats")), _dev(o.get("ln_part"))
    out = _nan(M, Cc)
    d_list = d_cnt = None
    if wlist is not None:
        d_list = torch.tensor(wlist + [-1] * 16, dtype=torch.int32, device="cuda")
        d_cnt = torch.tensor([wcnt], dtype=torch.int32, device="cuda")
    rc = lib.dsg_debug_qkv_attn_f32(B, res, ws, shift, heads, K, _p(dx), _p(dW), _p(dbq), _p(dst), _p(dpt), (K + 95) // 96 if ln == "part" else 0,
                                    _p(dbias), _p(d_list), _p(d_cnt), _p(out), None)
    assert rc == 0
    rows = torch.ones(M, dtype=torch.bool) if wlist is None else _window_rows(B, res, ws, shift, [w for w in wlist[:wcnt] if w >= 0])
    keep = _untouched(out)
    assert keep[M:].all() and keep[:M][~rows].all(), "rows of unlisted windows / guard rows were written"
    _check_formula(f"qkv+attn epilogue ws={ws}" + (" window list" if wlist is not None else ""), out.cpu()[:M], f[torch.float64], f[torch.float32], rows)


def test_gemm_qkv_attn_refuses_what_is_not_built():
    from diffusesg_amd import lib as L
    lib = L.load()
    d = torch.zeros(4096, device="cuda")
    lst = torch.zeros(32, dtype=torch.int32, device="cuda")
    args = lambda ws, res, st, wl: (1, res, ws, 0, 1, 32, _p(d), _p(d), _p(d), st, None, 0, _p(d), wl, wl, _p(d), None)
    assert lib.dsg_debug_qkv_attn_f32(*args(4, 8, _p(d), None)) == L.DSG_ERR_INVALID      # only 8 x 8 and 10 x 10 windows
    assert lib.dsg_debug_qkv_attn_f32(*args(8, 8, None, None)) == L.DSG_ERR_INVALID       # no LayerNorm statistics
    assert lib.dsg_debug_qkv_attn_f32(*args(10, 10, _p(d), _p(lst))) == L.DSG_ERR_INVALID # a window list at 10 x 10
    assert lib.dsg_debug_window_attn_f32(1, 6, 3, 0, 1, _p(d), _p(d), _p(d), None) == L.DSG_ERR_INVALID


# units = B * nW * heads, never a multiple of 4 except in the last case; shift 0 and ws / 2
WATTN_CASES = [(1, 6, 2, 0, 3), (1, 6, 2, 1, 1), (3, 4, 4, 0, 1), (1, 12, 4, 2, 1), (3, 5, 5, 0, 3), (1, 15, 5, 2, 1), (1, 8, 8, 0, 3),
               (1, 24, 8, 4, 1), (1, 10, 10, 0, 3), (1, 30, 10, 5, 1), (2, 20, 10, 5, 3)]


@pytest.mark.parametrize("B,res,ws,shift,heads", WATTN_CASES)
def test_window_attn_f32(B, res, ws, shift, heads):
    """window_attn_kernel, fp32 in and out, at every window size it is built for (4-, 16-, 25-token windows in one 32-position tile)"""
    from diffusesg_amd import lib as L
    lib = L.load()
    Cc, M, nW = 32 * heads, B * res * res, (res // ws) ** 2
    gen = torch.Generator().manual_seed(5700 + WATTN_CASES.index((B, res, ws, shift, heads)))
    qkv = torch.randn(M, 3 * Cc, generator=gen)
    qkv[:, :Cc] *= 32 ** -0.5 * R.LOG2E
    bias = R.make_attn_bias(nW, heads, ws, shift, gen)
    f64 = R.attn_formula(qkv.double(), bias, B, res, ws, shift, heads)
    f32 = R.attn_formula(qkv, bias, B, res, ws, shift, heads)
    dq, db, out = _dev(qkv), _dev(bias), _nan(M, Cc)
    assert lib.dsg_debug_window_attn_f32(B, res, ws, shift, heads, _p(dq), _p(db), _p(out), None) == 0
    assert _untouched(out)[M:].all(), "guard rows were written"
    _check_formula(f"window_attn ws={ws}", out.cpu()[:M], f64, f32)


def _mlp_operands(Cc, gen):
    W1 = torch.randn(4 * Cc, Cc, generator=gen) / Cc ** 0.5
    W2 = torch.randn(Cc, 4 * Cc, generator=gen) / (4 * Cc) ** 0.5
    return (1.0 + 0.2 * torch.randn(Cc, generator=gen), 0.2 * torch.randn(Cc, generator=gen), W1, torch.randn(4 * Cc, generator=gen) * 0.3, W2,
            torch.randn(Cc, generator=gen) * 0.3)


MLP_CASES = [(Cc, M, (i + j) % 2, -1) for i, Cc in enumerate((96, 192)) for j, M in enumerate((1, 33, 127, 129, 300))]
MLP_CASES += [(Cc, 320, (i + j) % 2, cnt) for i, Cc in enumerate((96, 192)) for j, cnt in enumerate(R.ROW_COUNTS)]


@pytest.mark.parametrize("Cc,M,stats,cnt", MLP_CASES)
def test_fused_mlp_f32(Cc, M, stats, cnt):
    """fused_mlp_kernel: x <- x + fc2(GELU(fc1(LN(x)))) in place on numpy-packed weights (pins the fragment layout), statistics of
    the rows written, and a run list as the row-mapped GEMM's"""
    from diffusesg_amd import lib as L
    lib = L.load()
    gen = torch.Generator().manual_seed(7700 + MLP_CASES.index((Cc, M, stats, cnt)))
    x = torch.randn(M, Cc, generator=gen) + torch.randn(M, 1, generator=gen)
    gam, bet, W1, b1, W2, b2 = _mlp_operands(Cc, gen)
    f64 = R.mlp_formula(*(t.double() for t in (x, gam, bet, W1, b1, W2, b2)))
    f32 = R.mlp_formula(x, gam, bet, W1, b1, W2, b2)
    runs = d_list = d_cnt = None
    if cnt >= 0:
        runs, lst = R.make_run_list(M // 8, cnt, 1 if cnt in (0, 1, 16) else 0, gen)
        d_list, d_cnt = torch.tensor(lst, dtype=torch.int32, device="cuda"), torch.tensor([cnt], dtype=torch.int32, device="cuda")
    x_io = torch.cat([x, torch.full((GUARD, Cc), float("nan"))]).cuda()
    x_in = x_io.clone()
    out_S = _nan(M, 2) if stats else None
    dev = [_dev(gam), _dev(bet), _dev(torch.from_numpy(R.pack_rows(W1.numpy()))), _dev(b1), _dev(torch.from_numpy(R.pack_cols(W2.numpy()))), _dev(b2)]
    rc = lib.dsg_debug_fused_mlp_f32(M, Cc, _p(x_io), *(_p(t) for t in dev), _p(out_S), _p(d_list), _p(d_cnt), None)
    assert rc == 0
    rows = _rows_mask(M, runs)
    same = (x_io.view(torch.int32) == x_in.view(torch.int32)).cpu()
    assert same[~rows].all(), "rows outside the run list / beyond M were written"
    got = x_io.cpu()[:M]
    _check_formula(f"fused_mlp C={Cc}" + (" run list" if cnt >= 0 else ""), got, f64, f32, rows[:M])
    if stats:
        # sums of the STORED values in float64; the bar from the reference's magnitudes: (C + 8) u sum |v|, times 2 (tests/f32_ref.py)
        bar, _ = R.formula_bar(f64, f32)
        mag = f64.abs() + bar
        S = torch.stack([torch.nan_to_num(got).double().sum(1), torch.nan_to_num(got).double().pow(2).sum(1)], 1)
        Bd = 2 * (Cc + R.C_EXTRA) * R.U * torch.stack([mag.sum(1), (mag * mag).sum(1)], 1)
        _check_written(out_S, 2, rows, S, Bd, "fused_mlp stats_out")
    assert lib.dsg_debug_fused_mlp_f32(M, 384, _p(x_io), *(_p(t) for t in dev), None, None, None, None) == L.DSG_ERR_INVALID


# (B, res, ws, shift, premod, window list, count): MB 1 (ws 4), MB 1 with invalid lanes (ws 5: 25 of 32), MB 2 (ws 8)
ATTN96_CASES = [
    (3, 4, 4, 0, 0, None, 0), (1, 12, 4, 2, 1, None, 0), (3, 5, 5, 0, 1, None, 0), (1, 15, 5, 2, 0, None, 0), (1, 8, 8, 0, 0, None, 0),
    (1, 24, 8, 4, 1, None, 0), (3, 16, 8, 4, 0, None, 0),
    (1, 12, 4, 2, 0, [8, 0, -1, 5, 3, 2], 5), (3, 16, 8, 4, 1, [1, 4, 6, -1, 11, 9, 10], 6), (3, 10, 5, 2, 0, [11, 2, 7, 0], 3),
    (2, 8, 4, 0, 1, [3, 1], 0),
]


@pytest.mark.parametrize("B,res,ws,shift,premod,wlist,wcnt", ATTN96_CASES)
def test_fused_attn96_f32(B, res, ws, shift, premod, wlist, wcnt):
    """fused_attn96_kernel: modulate + SiLU (or an already modulated x), LayerNorm-1, QKV, window attention, proj and the residual in
    place, on numpy-packed weights; per-sample (scale | shift) rows with aff_off != 0; window counts that are no multiple of 4"""
    from diffusesg_amd import lib as L
    lib = L.load()
    Cc, T, nW = 96, res * res, (res // ws) ** 2
    M = B * T
    gen = torch.Generator().manual_seed(9100 + ATTN96_CASES.index((B, res, ws, shift, premod, wlist, wcnt)))
    x = torch.randn(M, Cc, generator=gen) + 0.5 * torch.randn(M, 1, generator=gen)
    aff_off, aff_ld = 8, 8 + 2 * Cc + 4
    aff = torch.randn(B, aff_ld, generator=gen) * 0.5
    gam, bet = 1.0 + 0.2 * torch.randn(Cc, generator=gen), 0.2 * torch.randn(Cc, generator=gen)
    Wq, bq = _qkv_weights(Cc, Cc, gen)
    Wpj, bpj = torch.randn(Cc, Cc, generator=gen) / Cc ** 0.5, torch.randn(Cc, generator=gen) * 0.3
    bias = R.make_attn_bias(nW, 3, ws, shift, gen)
    sc, sh = aff[:, aff_off:aff_off + Cc], aff[:, aff_off + Cc:aff_off + 2 * Cc]
    ops = (x, sc, sh, gam, bet, Wq, bq)
    f64 = R.attn96_formula(*(t.double() for t in ops), bias, Wpj.double(), bpj.double(), B, res, ws, shift, premod)
    f32 = R.attn96_formula(*ops, bias, Wpj, bpj, B, res, ws, shift, premod)
    x_io = torch.cat([x, torch.full((GUARD, Cc), float("nan"))]).cuda()
    x_in = x_io.clone()
    d_list = d_cnt = None
    if wlist is not None:
        d_list = torch.tensor(wlist + [-1] * 16, dtype=torch.int32, device="cuda")
        d_cnt = torch.tensor([wcnt], dtype=torch.int32, device="cuda")
    dev = [_dev(gam), _dev(bet), _dev(torch.from_numpy(R.pack_rows(Wq.numpy()))), _dev(bq), _dev(bias), _dev(torch.from_numpy(R.pack_cols(Wpj.numpy()))),
           _dev(bpj)]
    daff = _dev(aff)
    rc = lib.dsg_debug_fused_attn96_f32(B, res, ws, shift, _p(x_io), _p(daff), aff_ld, aff_off, *(_p(t) for t in dev), premod, _p(d_list), _p(d_cnt), None)
    assert rc == 0
    rows = torch.ones(M, dtype=torch.bool) if wlist is None else _window_rows(B, res, ws, shift, [w for w in wlist[:wcnt] if w >= 0])
    rows_g = torch.cat([rows, torch.zeros(GUARD, dtype=torch.bool)])
    same = (x_io.view(torch.int32) == x_in.view(torch.int32)).cpu()
    assert same[~rows_g].all(), "rows of unlisted windows / guard rows were written"
    _check_formula(f"fused_attn96 ws={ws}" + (" window list" if wlist is not None else ""), x_io.cpu()[:M], f64, f32, rows)
    assert lib.dsg_debug_fused_attn96_f32(1, 10, 10, 0, _p(x_io), _p(daff), aff_ld, aff_off, *(_p(t) for t in dev), 0, None, None, None) == L.DSG_ERR_INVALID
