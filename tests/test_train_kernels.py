"""GPU: the training kernels (csrc/train_kernels.hip) on their own, through the dsg_debug_t_* hooks and dsg_adam_step / dsg_ema_update:
the split-K weight-gradient GEMM on the matrix pipe and its reducer, the activation-side route into the sampling GEMM, the plain
kernel with and without split-K, window attention forward and backward (matrix-pipe and scalar kernel), LayerNorm and modulate
forward and backward, column sums, the grouped launches, multi-tensor Adam and EMA.  EVERY output element is compared with a float64
evaluation of the same operation on the same fp32 operands (tests/train_ref.py), at the smallest shapes that reach each tile, slice
and chunk edge.  Every product asserts the route and the slice count it was written for.

Output buffers are filled with NaN before the launch and carry padding columns and guard rows: what the call must write has to be
finite and inside the bar, everything else bit-identical afterwards.

Bars (tests/train_ref.py, none from a kernel's output): products and column sums get the derived per-element bound; attention,
LayerNorm, modulate, Adam and EMA get 8x the error of a float32 torch evaluation of the same formula, capped at 1e-4 of the output
scale (the forward's row statistics: at least two roundings of the largest one).  Measured figures per case family: profiles/train_kernel_errors.md (each test prints its own)."""
import ctypes as C
import functools

import pytest
import torch

import train_ref as R
from train_ref import F32, F64

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000
GUARD = 2      # rows behind every output buffer
LDS_BYTES = 160 * 1024


def _lib():
    from diffusesg_amd import lib as L
    return L, L.load()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev(t):
    return None if t is None else t.contiguous().cuda()


def _nan(rows, cols=None):
    return torch.full((rows + GUARD,) if cols is None else (rows + GUARD, cols), float("nan"), device="cuda")


def _untouched(buf):
    return buf.view(torch.int32).cpu() == NAN_BITS


def _all_untouched(*bufs):
    return all(bool(_untouched(b).all()) for b in bufs if b is not None)


def _region(buf, rows, cols=None):
    """(values of the region the call had to write, True where everything outside it still holds the NaN fill)"""
    got, keep = buf.cpu(), _untouched(buf)
    must = torch.zeros_like(keep)
    if cols is None:
        must[:rows] = True
        return got[:rows], bool(keep[~must].all())
    must[:rows, :cols] = True
    return got[:rows, :cols], bool(keep[~must].all())


def _check_bound(tag, what, buf, rows, cols, ref, bound):
    got, clean = _region(buf, rows, cols)
    assert clean, f"{what}: elements written outside the result"
    assert torch.isfinite(got).all(), f"{what}: non-finite values in the result"
    r = R.worst_ratio(got, ref, bound)
    print(f"TRKGEMM {tag} {what} worst |err| / bound = {r:.3f}")
    assert r <= 1.0, f"{what}: {r:.2f} x the derived bound"


def _check_formula(tag, what, got, f64, f32, bar_of=R.formula_bar):
    """got (CPU) against the float64 formula; the bar from the float32 evaluation of the same formula"""
    bar, ref_err = bar_of(f64, f32)
    assert got.shape == f64.shape
    assert torch.isfinite(got).all(), f"{what}: non-finite values in the result"
    err = float((got.double() - f64).abs().max()) if got.numel() else 0.0
    print(f"TRKERR {tag} {what} bar={bar:.3e} ref_err={ref_err:.3e} kern_err={err:.3e} ratio={err / (bar + 1e-300):.3f} scale={float(f64.abs().max()):.3e}")
    assert err <= bar, f"{what}: max error {err:.3e} above the bar {bar:.3e} (float32 formula: {ref_err:.3e})"


def _ids(cases):
    return [c.ident() for c in cases]


# ----------------------------------------------------------------------------------------------------------------------------------
# products
# ----------------------------------------------------------------------------------------------------------------------------------
def _call_tgemm(c, o, bufs):
    L, lib = _lib()
    route = (C.c_int32 * 2)(-1, -1)
    rc = lib.dsg_debug_t_gemm(int(c.ta), int(c.tb), _p(bufs["A"]), c.lda, _p(bufs["B"]), c.ldb, _p(bufs["bias"]), _p(bufs["C"]), c.ldc, c.M, c.N, c.K,
                              int(c.acc), _p(bufs["cs"]), _p(bufs["res"]), c.act, _p(bufs["C2"]), int(c.force_plain), route, None)
    return rc, route[0], route[1]


def _tgemm_bufs(c, o):
    bufs = {k: _dev(o[k]) for k in ("A", "B", "bias", "res")}
    bufs["C"] = _nan(c.M, c.ldc)
    if c.acc:
        bufs["C"][:c.M, :c.N] = o["C0"][:, :c.N].cuda()
    bufs["C2"] = _nan(c.M, c.ldc) if c.act == R.ACT_GELU_KEEP else None
    bufs["cs"] = _nan(c.M) if c.colsum else None
    return bufs


def run_tgemm_case(c):
    o = R.make_tgemm(c)
    ref = R.tgemm_expect(o)
    bufs = _tgemm_bufs(c, o)
    rc, route, S = _call_tgemm(c, o, bufs)
    assert rc == 0, f"dsg_debug_t_gemm refused {c.ident()} (status {rc})"
    want = R.expected_route(c)
    assert (route, S) == want, f"{c.ident()}: took route {route} with {S} slices, written for route {want[0]} with {want[1]}"
    tag = f"route{route}-S{S}"
    _check_bound(tag, "C", bufs["C"], c.M, c.N, ref["C"], ref["bC"])
    if bufs["C2"] is not None:
        _check_bound(tag, "C2", bufs["C2"], c.M, c.N, ref["C2"], ref["bC2"])
    if c.colsum:
        _check_bound(tag, "colsum", bufs["cs"], c.M, None, ref["cs"], ref["bcs"])


@pytest.mark.parametrize("case", R.tn_cases(), ids=_ids(R.tn_cases()))
def test_gemm_tn_split_k(case):
    """gemm_tn_f32_kernel + reducer: exact slices, a partial last chunk, last slices of 33, 32, 31 rows and of ONE row, a slice count
    that drops after rounding, 1 / 4 / 16 reduction lanes; M, N, lda, ldb that are no multiples of 4 (M = 6, lda = 6); pitches above
    the widths; accumulate onto a non-zero C; the column sums"""
    run_tgemm_case(case)


@pytest.mark.parametrize("case", R.mfma_cases(), ids=_ids(R.mfma_cases()))
def test_gemm_activation_side_route(case):
    """y = x W^T and dx = dy W through the sampling GEMM: K of 32 / 96 / 160, K = 4 / 36 / 60 through the zero-padded weight image, the
    transposed weight, res, accumulate, both activation forms; just outside the thresholds the plain kernel under the same bound"""
    run_tgemm_case(case)


@pytest.mark.parametrize("case", R.plain_cases(), ids=_ids(R.plain_cases()))
def test_gemm_plain_routes(case):
    """the plain kernel in all four (ta, tb) forms at 1 / 31 / 32 / 33 / 65, and with split-K at K = 4096, 32769, 33793 and 34817"""
    run_tgemm_case(case)


def test_gemm_fallback_refuses_activation_forms_it_cannot_finish():
    """an activation form with ta, with ldc != N or with accumulate (below the matrix-pipe route's thresholds): a status, route 0, nothing written"""
    L, _ = _lib()
    for kw in (dict(ta=True, tb=False, act=R.ACT_GELU_KEEP), dict(ta=False, tb=True, act=R.ACT_GELU_KEEP, pc=3),
               dict(ta=False, tb=False, act=R.ACT_DGELU, acc=True), dict(ta=True, tb=True, act=R.ACT_DGELU)):
        c = R.TGemmCase(M=33, N=32, K=32, seed=900, **kw)
        o = R.make_tgemm(c)
        bufs = _tgemm_bufs(c, o)
        if c.acc:
            bufs["C"] = _nan(c.M, c.ldc)
        rc, route, S = _call_tgemm(c, o, bufs)
        assert rc == L.DSG_ERR_INVALID and route == 0, (c.ident(), rc, route)
        assert _all_untouched(bufs["C"], bufs["C2"]), f"{c.ident()}: a refused call wrote to its outputs"


# ----------------------------------------------------------------------------------------------------------------------------------
# window attention
# ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _attn_ref(c):
    o = R.make_attn(c)
    out, gq, gt = R.attn_autograd(o)
    f32 = R.attn_explicit(o, F32)
    t0 = o["d_table0"]
    return o, (out, gq, t0.double() + gt), (f32[0], f32[1], t0 + f32[2])


def _plain_attn_lds(c, bwd):
    Wt = c.ws * c.ws
    return 4 * ((4 if bwd else 3) * Wt * 33 + (2 if bwd else 1) * Wt * (Wt + 1))


@pytest.mark.parametrize("plain", [0, 1], ids=["mfma", "plain"])
@pytest.mark.parametrize("case", R.attn_cases(), ids=_ids(R.attn_cases()))
def test_window_attention_forward_backward(case, plain):
    """out, d_qkv over every row and d_table ADDED onto a non-zero prior content, against float64 autograd of the Swin definition
    (roll, partition, region slices); windows of 4 ... 121 tokens (padded to 32 / 64 / 128 positions on the matrix pipe)"""
    L, lib = _lib()
    c = case
    o, ref, f32 = _attn_ref(c)
    rows, Cc = c.B * c.res * c.res, 32 * c.heads
    dq, dt, dd = _dev(o["qkv"]), _dev(o["table"]), _dev(o["d_out"])
    out, d_qkv = _nan(rows, Cc), _nan(rows, 3 * Cc)
    d_table = torch.cat([o["d_table0"], torch.full((GUARD, c.heads), float("nan"))]).cuda()
    tag = f"attn-{'plain' if plain else 'mfma'}"
    rc = lib.dsg_debug_t_attn(0, c.B, c.res, c.ws, c.shift, c.heads, _p(dq), _p(dt), _p(out), None, None, None, plain, None)
    assert rc == 0, f"forward refused (status {rc})"
    got, clean = _region(out, rows)
    assert clean, "forward: guard rows written"
    _check_formula(tag, "out", got, ref[0], f32[0])
    rc = lib.dsg_debug_t_attn(1, c.B, c.res, c.ws, c.shift, c.heads, _p(dq), _p(dt), None, _p(dd), _p(d_qkv), _p(d_table), plain, None)
    if plain and _plain_attn_lds(c, True) > LDS_BYTES:
        # the scalar kernel keeps P and dP of a window in LDS: 121 tokens need 182 KB, more than a workgroup can have -- a status, no write
        assert rc != 0 and _all_untouched(d_qkv) and torch.equal(d_table[:-GUARD].cpu(), o["d_table0"])
        return
    assert rc == 0, f"backward refused (status {rc})"
    got, clean = _region(d_qkv, rows)
    assert clean, "backward: guard rows of d_qkv written"
    _check_formula(tag, "d_qkv", got, ref[1], f32[1])
    assert _all_untouched(d_table[-GUARD:]), "backward: rows behind d_table written"
    _check_formula(tag, "d_table", d_table[:-GUARD].cpu(), ref[2], f32[2])


def test_attention_refuses_windows_it_cannot_hold():
    L, lib = _lib()
    d = torch.zeros(4, device="cuda")
    assert lib.dsg_debug_t_attn(0, 1, 12, 12, 0, 1, _p(d), _p(d), _p(d), None, None, None, 0, None) == L.DSG_ERR_INVALID     # 144 tokens
    assert lib.dsg_debug_t_attn(0, 1, 9, 4, 0, 1, _p(d), _p(d), _p(d), None, None, None, 0, None) == L.DSG_ERR_INVALID       # res % ws
    assert lib.dsg_debug_t_attn(1, 1, 8, 4, 0, 1, _p(d), _p(d), None, _p(d), _p(d), None, 0, None) == L.DSG_ERR_INVALID      # no d_table


# ----------------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ----------------------------------------------------------------------------------------------------------------------------------
def _ln_call(bwd, M, Cc, T, x, aff, y_mod, gam, bet, y, stats, dy=None, dx_in=None, dx_out=None, dg=None, db=None):
    _, lib = _lib()
    return lib.dsg_debug_t_ln(bwd, M, Cc, T, _p(x), _p(aff), _p(y_mod), _p(gam), _p(bet), _p(y), _p(stats), _p(dy), _p(dx_in), _p(dx_out), _p(dg), _p(db), None)


@pytest.mark.parametrize("M,Cc", R.ln_cases(), ids=[f"M{m}-C{c}" for m, c in R.ln_cases()])
def test_layernorm_forward_backward(M, Cc):
    """the five <LPR, KV> forms on both sides of every switch; last blocks of one row (M = 1, 5, 9, 17, 4097, 8193); the forward with
    and without the modulate prologue (T = 9: a wave's rows straddle samples); the backward with dx_in null, distinct and aliasing
    dx_out, and with d_gamma or d_beta null"""
    seed = M * 7 + Cc
    o = R.ln_inputs(M, Cc, seed, aff_T=9)
    tag = f"ln-{R.ln_form(Cc)[0]}x{R.ln_form(Cc)[1]}"
    dx_, dgam, dbet, daff, ddy, ddx_in = (_dev(o[k]) for k in ("x", "gam", "bet", "aff", "dy", "dx_in"))
    for with_aff in (False, True):
        x64 = o["x"].double()
        xm64, xm32 = (R.modulate_fwd(x64, o["aff"].double(), 9), R.modulate_fwd(o["x"], o["aff"], 9)) if with_aff else (x64, o["x"])
        y64, st64 = R.ln_fwd(xm64, o["gam"].double(), o["bet"].double())
        y32, st32 = R.ln_fwd(xm32, o["gam"], o["bet"])
        y, stats, y_mod = _nan(M, Cc), _nan(M, 2), (_nan(M, Cc) if with_aff else None)
        rc = _ln_call(0, M, Cc, 9, dx_, daff if with_aff else None, y_mod, dgam, dbet, y, stats)
        assert rc == 0, f"forward refused (status {rc})"
        w = f"{'mod+' if with_aff else ''}"
        for name, buf, r64, r32 in ((w + "y", y, y64, y32), (w + "stats", stats, st64, st32)) + (((w + "y_mod", y_mod, xm64, xm32),) if with_aff else ()):
            got, clean = _region(buf, M)
            assert clean, f"{name}: guard rows written"
            if name.endswith("stats"):
                _check_formula(tag, w + "mean", got[:, 0], r64[:, 0], r32[:, 0], R.stats_bar)
                _check_formula(tag, w + "rstd", got[:, 1], r64[:, 1], r32[:, 1], R.stats_bar)
            else:
                _check_formula(tag, name, got, r64, r32)
    # backward from statistics given in fp32 (the float64 ones, rounded): they are operands
    st = R.ln_fwd(o["x"].double(), o["gam"].double(), o["bet"].double())[1].float()
    dst = _dev(st)
    variants = (("none", True, True), ("distinct", True, False), ("alias", False, True)) if M > 1000 else \
               (("none", True, True), ("distinct", True, True), ("alias", True, True), ("none", False, True), ("distinct", True, False))
    for mode, want_g, want_b in variants:
        din64 = None if mode == "none" else o["dx_in"].double()
        r64 = R.ln_bwd(o["x"].double(), o["gam"].double(), st.double(), o["dy"].double(), din64)
        r32 = R.ln_bwd(o["x"], o["gam"], st, o["dy"], None if mode == "none" else o["dx_in"])
        dx_out = _nan(M, Cc)
        if mode == "alias":
            dx_out[:M] = ddx_in
        dg, db = (_nan(Cc) if want_g else None), (_nan(Cc) if want_b else None)
        rc = _ln_call(1, M, Cc, 1, dx_, None, None, dgam, None, None, dst, ddy, {"none": None, "distinct": ddx_in, "alias": dx_out}[mode], dx_out, dg, db)
        assert rc == 0, f"backward refused (status {rc})"
        w = f"bwd-{mode}-"
        got, clean = _region(dx_out, M)
        assert clean, "dx: guard rows written"
        _check_formula(tag, w + "dx", got, r64[0], r32[0])
        for name, buf, k in (("d_gamma", dg, 1), ("d_beta", db, 2)):
            if buf is not None:
                got, clean = _region(buf, Cc)
                assert clean, f"{name}: written behind its end"
                _check_formula(tag, w + name, got, r64[k], r32[k])


@pytest.mark.parametrize("Cc", [1540, 98])
def test_layernorm_refuses_widths_it_does_not_build(Cc):
    L, _ = _lib()
    o = R.ln_inputs(5, Cc, 1)
    dx_, dgam, dbet, ddy = (_dev(o[k]) for k in ("x", "gam", "bet", "dy"))
    y, stats, dxo, dg, db = _nan(5, Cc), _nan(5, 2), _nan(5, Cc), _nan(Cc), _nan(Cc)
    assert _ln_call(0, 5, Cc, 1, dx_, None, None, dgam, dbet, y, stats) == L.DSG_ERR_INVALID
    st = torch.ones(5, 2, device="cuda")
    assert _ln_call(1, 5, Cc, 1, dx_, None, None, dgam, None, None, st, ddy, None, dxo, dg, db) == L.DSG_ERR_INVALID
    assert _all_untouched(y, stats, dxo), "a refused call wrote to its outputs"


# ----------------------------------------------------------------------------------------------------------------------------------
# modulate, column sums
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,Cc", R.modulate_cases(), ids=[f"B{b}-T{t}-C{c}" for b, t, c in R.modulate_cases()])
def test_modulate_forward_backward(B, T, Cc):
    """silu(shift + x (1 + scale)) and its backward with the chunked d_aff reduction: one chunk, 64 / 65 rows, 64 chunks of 65 rows with
    a last one of two; channel counts around the 64-column block; |u| up to 90"""
    _, lib = _lib()
    o = R.modulate_inputs(B, T, Cc, B * 1000 + T + Cc)
    M, tag = B * T, f"modulate-chunks{R.modulate_chunks(T)[0]}"
    dx_, daff, ddy = (_dev(o[k]) for k in ("x", "aff", "dy"))
    y = _nan(M, Cc)
    assert lib.dsg_debug_t_modulate(0, B, T, Cc, _p(dx_), _p(daff), None, _p(y), None, None) == 0
    got, clean = _region(y, M)
    assert clean, "y: guard rows written"
    _check_formula(tag, "y", got, R.modulate_fwd(o["x"].double(), o["aff"].double(), T), R.modulate_fwd(o["x"], o["aff"], T))
    dxo, d_aff = _nan(M, Cc), _nan(B, 2 * Cc)
    assert lib.dsg_debug_t_modulate(1, B, T, Cc, _p(dx_), _p(daff), _p(ddy), _p(dxo), _p(d_aff), None) == 0
    r64 = R.modulate_bwd(o["x"].double(), o["aff"].double(), o["dy"].double(), T)
    r32 = R.modulate_bwd(o["x"], o["aff"], o["dy"], T)
    for name, buf, rows, k in (("dx", dxo, M, 0), ("d_aff", d_aff, B, 1)):
        got, clean = _region(buf, rows)
        assert clean, f"{name}: guard rows written"
        _check_formula(tag, name, got, r64[k], r32[k])


COLSUM_M, COLSUM_N = (1, 31, 33, 1025, 16385), (1, 63, 64, 65, 200)


@pytest.mark.parametrize("i", range(10))
def test_colsum(i):
    """t_colsum: one row chunk and many, a last chunk of one row, column counts around the 64-column block, ld > N"""
    _, lib = _lib()
    M, N = COLSUM_M[i % 5], COLSUM_N[(i + i // 5) % 5]
    ld = N + (0, 3)[i % 2] + (5 if i >= 5 else 0)
    X = torch.randn(M, ld, generator=torch.Generator().manual_seed(800 + i)) + 0.5
    out = _nan(N)
    assert lib.dsg_debug_t_colsum(_p(_dev(X)), ld, _p(out), M, N, None) == 0
    ref, bound = R.colsum_expect(X[:, :N])
    _check_bound(f"colsum-M{M}-N{N}-ld{ld}", "out", out, N, None, ref, bound)


# ----------------------------------------------------------------------------------------------------------------------------------
# grouped launches
# ----------------------------------------------------------------------------------------------------------------------------------
def _group_shapes(n, gen):
    """different (M, N, K) per problem; the first is the largest in neither M nor N, so the grid comes from two other problems"""
    return [(int(torch.randint(1, 70, (1,), generator=gen)), int(torch.randint(1, 70, (1,), generator=gen)), int(torch.randint(1, 70, (1,), generator=gen)))
            for _ in range(n)]


@pytest.mark.parametrize("n", [1, 13, 32])
@pytest.mark.parametrize("kind", ["NT", "TN", "NN", "NN_SUM", "SUM", "COLSUM"])
def test_grouped_launches(kind, n):
    """every built form of t_gemm_grouped, t_sum_grouped and t_colsum_grouped with 1, 13 and 32 problems of different sizes: the grid is
    sized by the largest, the smaller problems' blocks must write nothing outside their own result"""
    L, lib = _lib()
    gen = torch.Generator().manual_seed(600 + n + 100 * len(kind))
    code = getattr(L, "TGROUP_" + kind)
    shapes = _group_shapes(n, gen)
    if kind == "NN_SUM":
        shapes = [(37, 65, k) for _, _, k in shapes]
    if kind == "SUM":
        shapes = [(3, 171, 1)] * n                      # n_out = 513: no multiple of 256
    probs = (L.DsgTProb * n)()
    keep, cases, outs = [], [], []
    shared = _nan(37, 65 + 3) if kind == "NN_SUM" else None
    for z, (M, N, K) in enumerate(shapes):
        ta, tb = kind in ("TN",), kind in ("NT",)
        c = R.TGemmCase(ta, tb, M, N, K, pa=z % 3, pb=(z + 1) % 2, pc=3, bias=(kind in ("NT", "NN", "NN_SUM") and z % 2 == 0), seed=3000 + 40 * n + z)
        o = R.make_tgemm(c)
        if kind == "SUM":
            Cz = torch.randn(M * N, generator=gen).cuda()
        elif kind == "COLSUM":
            Cz = _nan(N)
        else:
            Cz = shared if shared is not None else _nan(M, c.ldc)
        dA, dB, dbias = _dev(o["A"]), _dev(o["B"]), _dev(o["bias"])
        keep += [dA, dB, dbias, Cz]
        p = probs[z]
        p.A, p.B, p.bias, p.C = dA.data_ptr(), dB.data_ptr(), (dbias.data_ptr() if dbias is not None else None), Cz.data_ptr()
        p.lda, p.ldb, p.ldc, p.M, p.N, p.K = c.lda, c.ldb, c.ldc, M, N, K
        if kind == "COLSUM":        # A = X [M rows, N columns used of lda]
            X = torch.randn(M, N + 2, generator=gen)
            dX = X.cuda()
            keep.append(dX)
            p.A, p.lda = dX.data_ptr(), N + 2
            o["X"] = X[:, :N]
        cases.append((c, o)); outs.append(Cz)
    out_sum = _nan(513) if kind == "SUM" else None
    rc = lib.dsg_debug_t_grouped(code, n, probs, _p(out_sum), 513 if kind == "SUM" else 0, None)
    assert rc == 0, f"refused (status {rc})"
    tag = f"grouped-{kind}-n{n}"
    if kind == "SUM":
        st = torch.stack([t.cpu() for t in outs]).double()
        _check_bound(tag, "out", out_sum, 513, None, st.sum(0), 2 * (n + R.C_EXTRA) * R.U * st.abs().sum(0))
    elif kind == "COLSUM":
        for z, (c, o) in enumerate(cases):
            ref, bound = R.colsum_expect(o["X"])
            _check_bound(tag, f"out[{z}]", outs[z], c.N, None, ref, bound)
    elif kind == "NN_SUM":
        A = torch.cat([R.op_A(o) for _, o in cases], 1)
        Bm = torch.cat([R.op_B(o) for _, o in cases], 0)
        bias = cases[0][1]["bias"].double() if cases[0][0].bias else torch.zeros(65, dtype=F64)
        bound = 2 * (A.shape[1] + R.C_EXTRA) * R.U * (A.abs() @ Bm.abs() + bias.abs())
        _check_bound(tag, "C", shared, 37, 65, A @ Bm + bias, bound)
    else:
        for z, (c, o) in enumerate(cases):
            ref = R.tgemm_expect(o)
            _check_bound(tag, f"C[{z}]", outs[z], c.M, c.N, ref["C"], ref["bC"])


def test_grouped_refuses_the_form_that_is_not_built():
    L, lib = _lib()
    c = R.TGemmCase(True, True, 5, 7, 9, seed=1)
    o = R.make_tgemm(c)
    dA, dB, out = _dev(o["A"]), _dev(o["B"]), _nan(5, 7)
    probs = (L.DsgTProb * 1)()
    p = probs[0]
    p.A, p.B, p.C, p.lda, p.ldb, p.ldc, p.M, p.N, p.K = dA.data_ptr(), dB.data_ptr(), out.data_ptr(), c.lda, c.ldb, 7, 5, 7, 9
    assert lib.dsg_debug_t_grouped(L.TGROUP_TT, 1, probs, None, 0, None) == L.DSG_ERR_INVALID
    assert lib.dsg_debug_t_grouped(L.TGROUP_NN, 0, probs, None, 0, None) == L.DSG_ERR_INVALID
    assert lib.dsg_debug_t_grouped(L.TGROUP_NN, L.T_GROUP_MAX + 1, probs, None, 0, None) == L.DSG_ERR_INVALID
    assert lib.dsg_debug_t_grouped(7, 1, probs, None, 0, None) == L.DSG_ERR_INVALID
    assert _all_untouched(out)


# ----------------------------------------------------------------------------------------------------------------------------------
# Adam behind clip_grad_norm_, EMA
# ----------------------------------------------------------------------------------------------------------------------------------
def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _cat(ts):
    return torch.cat([t.reshape(-1).cpu() for t in ts])


@pytest.mark.parametrize("max_norm", [1.0, 1e6, 0.0], ids=["clip", "noclip", "off"])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("sizes", [R.ADAM_SIZES, (1,) * 300], ids=["chunks", "300x1"])
def test_adam_steps(sizes, wd, max_norm):
    """three steps with carried state; tensors of 1 ... 8193 elements in one call (chunk edges at 4095 / 4096 / 4097) and 300
    one-element tensors (the clip kernel strides tensors by 256); every element of p, m, v and of the gradients scaled in place; the
    total norm against float64.  Each step's operands are the fp32 state the previous step left on the device."""
    _, lib = _lib()
    n = len(sizes)
    p, g, m, v = ([t.cuda() for t in ts] for ts in R.adam_inputs(sizes, 1))
    numel = (C.c_int64 * n)(*sizes)
    hp = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=wd, max_norm=max_norm)
    tag = f"adam-{'x'.join(map(str, sorted(set(sizes))))[:24]}"
    for step in (1, 2, 3):
        if step > 1:
            g = [t.cuda() for t in R.adam_inputs(sizes, step)[1]]
        ops = [[t.cpu().clone() for t in ts] for ts in (p, g, m, v)]
        r64, r32 = R.adam_step(*ops, step, **hp), R.adam_step(*ops, step, dt=F32, **hp)
        norm = C.c_float(-1.0)
        rc = lib.dsg_adam_step(n, _ptrs(p), _ptrs(g), _ptrs(m), _ptrs(v), numel, step, hp["lr"], hp["b1"], hp["b2"], hp["eps"], wd, max_norm, C.byref(norm), None)
        assert rc == 0
        # per-tensor fp32 norms (u each, 2 u after squaring), the sum's rounding to fp32 and the final square root: below 4 u
        print(f"TRKERR {tag} step{step} total_norm rel_err={abs(norm.value - r64[4]) / r64[4]:.3e} bar={4 * R.U:.3e}")
        assert abs(norm.value - r64[4]) <= 4 * R.U * r64[4]
        if max_norm == 1.0:
            assert r64[4] > 1.0            # the clipping is active
        for name, dev, k in (("p", p, 0), ("g", g, 1), ("m", m, 2), ("v", v, 3)):
            _check_formula(tag, f"step{step}-{name}", _cat(dev), _cat(r64[k]), _cat(r32[k]))


def test_ema_update():
    _, lib = _lib()
    sizes = R.ADAM_SIZES + (1,) * 300
    n = len(sizes)
    gen = torch.Generator().manual_seed(77)
    ema, p = [torch.randn(s, generator=gen) for s in sizes], [torch.randn(s, generator=gen) for s in sizes]
    de, dp = [t.cuda() for t in ema], [t.cuda() for t in p]
    numel = (C.c_int64 * n)(*sizes)
    for decay in (0.999, 0.9):
        ops = [t.cpu().clone() for t in de]
        assert lib.dsg_ema_update(n, _ptrs(de), _ptrs(dp), numel, decay, None) == 0
        _check_formula("ema", f"decay{decay}", _cat(de), _cat(R.ema_step(ops, p, decay)), _cat(R.ema_step(ops, p, decay, F32)))
        assert all(torch.equal(a.cpu(), b) for a, b in zip(dp, p)), "the parameters were written"
