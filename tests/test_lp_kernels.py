"""GPU: the two bf16-MFMA GEMMs of csrc/kernels_lp.hip on their own -- gemm_bf16_kernel (option "gemm_bf16") in every template form
launch_gemm_lp builds, on both of its tiles, and gemm_split2_kernel (option "gemm_split") -- through dsg_debug_gemm_lp, which calls
that launcher directly: a refused form is an error here, never a silent run of the fp32 kernel.  EVERY output element is compared
with the float64 reference of tests/lp_ref.py (bf16 mode: the float64 product of the bf16-rounded operands; split mode: of the fp32
operands) inside bars derived there from the reference's own quantities and the formats.  The conversion kernels are pinned bit for bit
through dsg_debug_convert.

As in tests/test_f32_kernels.py, output buffers are filled with NaN before the launch and carry padding columns and guard rows: what
the kernel must write has to be finite and inside the bar, everything else bit-identical afterwards.  The cases (lp_ref: shared with
tests/test_lp_kernels_host.py, which shows that a NumPy emulation of the kernels passes every one of them and twelve seeded mistakes do
not) are the smallest that reach each edge.  Measured figures per case family: profiles/lp_kernel_errors.md (each test prints its own)."""
import ctypes as C

import numpy as np
import pytest
import torch

import edge_ref as X
import f32_ref as R
import lp_ref as P

pytestmark = pytest.mark.gpu

GUARD = 2      # rows behind every output buffer
NAN32, NAN16 = 0x7FC00000, 0x7FC0


def _dev(t):
    return None if t is None else t.contiguous().cuda()


def _nan(rows, cols, dtype=torch.float32):
    return torch.full((rows + GUARD, cols), float("nan"), device="cuda", dtype=dtype)


def _untouched(buf):
    """[rows, cols] bool: the element still holds the NaN fill, bit for bit"""
    if buf.dtype == torch.bfloat16:
        return (buf.view(torch.int16).cpu().to(torch.int32) & 0xFFFF) == NAN16
    return buf.view(torch.int32).cpu() == NAN32


def _check_written(buf, M, N, ref, bound, what):
    """buf [M + GUARD, ld] from the device: rows < M, columns < N hold the reference within the bound; all else is untouched"""
    got, keep = buf.float().cpu(), _untouched(buf)      # (a bf16 buffer is widened: exact)
    must = torch.zeros_like(keep)
    must[:M, :N] = True
    assert keep[~must].all(), f"{what}: {int((~keep[~must]).sum())} elements written outside the rows / columns of the result"
    assert torch.isfinite(got[:M, :N]).all(), f"{what}: non-finite values in the result"
    r = R.worst_ratio(got[:M, :N], ref, bound)
    print(f"LPKGEMM {what} worst |err| / bound = {r:.3f}")
    assert r <= 1.0, f"{what}: {r:.2f} x the derived bound"
    return got


def launch(c: P.LpCase, o, bufs=None, tile=None):
    """one dsg_debug_gemm_lp launch of the case on its operands; returns (status, tile rows used, dict of the output buffers)"""
    from diffusesg_amd import lib as L
    lib = L.load()
    g = c.g
    keep = {k: _dev(o.get(k)) for k in ("A2", "W", "bias", "ln_stats", "ln_part", "res", "mod_aff")}
    keep["A"] = _dev(o["A"].to(torch.bfloat16) if c.a_bf16 else o["A"])
    out = bufs or {"C": _nan(g.M, o["ldc"], torch.bfloat16 if c.c_bf16 else torch.float32),
                   "C2": _nan(g.M, o["ldc2"]) if g.c2 else None,
                   "stats_out": _nan(g.M, 2 * g.tiles_n) if g.epi >= 1 else None}
    a = L.DsgGemmLpArgs()
    for name, t in list(keep.items()) + list(out.items()):
        setattr(a, name, None if t is None else t.data_ptr())
    used = C.c_int32(-1)
    a.tile_used = C.addressof(used)
    a.lda, a.lda2, a.K1, a.ln_nparts = o["lda"], o.get("lda2", 0), g.K1, (g.nparts if g.ln == "part" else 0)
    a.ldres, a.ldc, a.ldc2 = (o["ldres"] if g.res else 0), o["ldc"], (o["ldc2"] if g.c2 else 0)
    a.M, a.N, a.K, a.act = g.M, g.N, g.K, g.act
    a.mod_ld, a.mod_off, a.mod_T = o.get("mod_ld", 0), g.mod_off, g.mod_T
    a.mode, a.tile, a.a_bf16, a.c_bf16 = c.mode, (c.tile if tile is None else tile), int(c.a_bf16), int(c.c_bf16)
    rc = lib.dsg_debug_gemm_lp(C.byref(a), None)
    return rc, used.value, out


def run_case(c: P.LpCase, want_rows=None):
    g = c.g
    o = P.make_lp(c)
    ref = P.lp_expect(o, c)
    rc, used, out = launch(c, o)
    assert rc == 0, f"dsg_debug_gemm_lp refused {c.ident()} (status {rc})"
    assert used == (want_rows or c.tile_rows), f"{c.ident()}: ran the {used}-row tile"
    got_C = _check_written(out["C"], g.M, g.N, ref["C"], ref["bC"], "C")
    if g.c2:
        _check_written(out["C2"], g.M, g.N, ref["C2"], ref["bC2"], "C2")
    if g.epi >= 1:
        # float64 sums of the values the kernel STORED, over each tile's valid columns only; the bar from the reference's magnitudes
        S, Bd = R.stats_expect(torch.nan_to_num(got_C[:g.M, :g.N]), g, ref["C"], ref["bC"])
        _check_written(out["stats_out"], g.M, 2 * g.tiles_n, S.reshape(g.M, -1), Bd.reshape(g.M, -1), "stats_out")
    return out


def _ids(cases):
    return [c.ident() for c in cases]


def _both(f):
    return f(1) + f(2)


@pytest.mark.parametrize("case", _both(P.bf16_plain_cases), ids=_ids(_both(P.bf16_plain_cases)))
def test_bf16_plain_forms(case):
    """LN x {none, GELU, SiLU} x res on the 128-row tile (K step 64: K = 32 and 96 end in a half-valid chunk) and on the 256-row tile (K
    step 32), ln_stats and ln_part, every M / N / K edge; the last two of each tile have lda > K, ldc > N, ldres != ldc and a dual store"""
    run_case(case)


@pytest.mark.parametrize("case", _both(P.bf16_ln_part_cases), ids=_ids(_both(P.bf16_ln_part_cases)))
def test_bf16_ln_part(case):
    """LayerNorm statistics from 1, 2, 3, 4 and 8 partial pairs: the two vector-load forms and the generic loop"""
    run_case(case)


@pytest.mark.parametrize("case", _both(P.bf16_concat_cases), ids=_ids(_both(P.bf16_concat_cases)))
def test_bf16_a2_concat(case):
    """two sources along K, lda2 != lda: (K1, K) = (64, 96), (64, 160), (128, 224)"""
    run_case(case)


@pytest.mark.parametrize("case", _both(P.bf16_epi_cases), ids=_ids(_both(P.bf16_epi_cases)))
def test_bf16_epilogue_extensions(case):
    """EPI 1/2/3: row statistics, batch-uniform and per-sample modulate + SiLU through the LDS row-to-sample table (36-row samples: a
    boundary inside every tile of either height and inside the ragged last one), mod_off != 0, with and without res, C2 un-modulated"""
    run_case(case)


@pytest.mark.parametrize("case", _both(P.bf16_abf_cases), ids=_ids(_both(P.bf16_abf_cases)))
def test_bf16_a_tensor_in_bf16(case):
    """ABF: the A tensor arrives as bf16 and is staged as it is; EPI 0 .. 3, K = 64 and 128"""
    run_case(case)


@pytest.mark.parametrize("case", _both(P.bf16_cbf_cases), ids=_ids(_both(P.bf16_cbf_cases)))
def test_bf16_c_tensor_in_bf16(case):
    """CBF: the result is stored as bf16 behind a LayerNorm from statistics or partials, without activation and with GELU"""
    run_case(case)


@pytest.mark.parametrize("case,rows", P.bf16_rule_cases(), ids=["wide", "narrow"])
def test_bf16_launcher_rule_picks_the_tile(case, rows):
    """tile 0: 512 tiles of 256 x 96 -> the wide tile, fewer -> the narrow one; tile_used reports it"""
    run_case(case, want_rows=rows)


TILE_PAIRS = P.bf16_cases(2)


@pytest.mark.parametrize("case", TILE_PAIRS, ids=_ids(TILE_PAIRS))
def test_bf16_tiles_agree_bit_for_bit(case):
    """both tiles feed the same 16-k MFMA steps in ascending k into one accumulator per output (a half-valid chunk of the 64-deep tile
    adds products of zeros): C, C2 and stats_out are the same bits, NaN fill outside the result included"""
    o = P.make_lp(case)
    outs = []
    for tile in (1, 2):
        rc, used, out = launch(case, o, tile=tile)
        assert rc == 0 and used == 128 * tile
        outs.append(out)
    for k, t in outs[0].items():
        if t is not None:
            it = torch.int16 if t.dtype == torch.bfloat16 else torch.int32
            assert torch.equal(t.view(it), outs[1][k].view(it)), f"{k} differs between the 128-row and the 256-row tile"


@pytest.mark.parametrize("case", P.split_cases(), ids=_ids(P.split_cases()))
def test_split_forms(case):
    """all twelve LN / act / res variants at M = 1, 255, 256, 257 and nine row tiles + 3 (rows past M re-read the last valid row, W
    rows past N the last valid W row), K = 32 (one chunk: every prefetch clamps), 64, 96; two sources; dual store; pitches; the table
    GELU on pre-activations over [-7, 7]; operands with full mid planes"""
    run_case(case)


def test_refused_forms_write_nothing():
    """the literal list of forms launch_gemm_lp refuses (lp_ref.REFUSALS): DSG_ERR_INVALID, tile_used 0, no output touched -- and the
    same calls without the offending field run.  Split with a K1 inside a 32-k chunk is among them: the kernel switches sources at
    chunk K1 / 32 and would read the wrong columns of both, so the launcher refuses it (no caller passes one)."""
    from diffusesg_amd import lib as L
    lib = L.load()
    M, N, Kmax = 300, 100, 128
    gen = torch.Generator().manual_seed(5)
    src = {"A": torch.randn(M, Kmax, generator=gen), "A2": torch.randn(M, Kmax, generator=gen), "W": torch.randn(N, Kmax, generator=gen),
           "ln_stats": torch.stack([torch.zeros(M), torch.ones(M)], 1), "ln_part": torch.ones(M, 2, 2), "res": torch.randn(M, N, generator=gen)}
    dev = {k: v.cuda() for k, v in src.items()}
    dev["A_bf16"] = src["A"].to(torch.bfloat16).cuda()
    outs = {"C": _nan(M, N), "C2": _nan(M, N), "stats_out": _nan(M, 4)}

    def call(mode, **kw):
        a = L.DsgGemmLpArgs()
        K = kw.get("K", 64)
        a.M, a.N, a.K, a.mode, a.lda, a.ldc, a.ldc2, a.ldres, a.lda2 = M, N, K, mode, Kmax, N, N, N, Kmax
        a.A, a.W, a.C = (dev["A_bf16"] if kw.get("a_bf16") else dev["A"]).data_ptr(), dev["W"].data_ptr(), outs["C"].data_ptr()
        for k, v in kw.items():
            if k in ("A2", "ln_stats", "ln_part", "res"):
                setattr(a, k, dev[k].data_ptr())
            elif k in ("C2", "stats_out"):
                setattr(a, k, outs[k].data_ptr())
            else:
                setattr(a, k, v)
        used = C.c_int32(-1)
        a.tile_used = C.addressof(used)
        return lib.dsg_debug_gemm_lp(C.byref(a), None), used.value
    for name, kw in P.REFUSALS:
        rc, used = call(**kw)
        assert rc == L.DSG_ERR_INVALID and used == 0, f"{name}: status {rc}, tile {used}"
        assert all(_untouched(t).all() for t in outs.values()), f"{name}: an output was written"
    # the neighbouring admitted forms run (so each refusal above is about the named field, not about this test's buffers)
    for mode in (1, 2):
        assert call(mode)[0] == 0 and call(mode, A2=True, K1=64, K=128)[0] == 0 and call(mode, ln_stats=True, act=R.ACT_GELU)[0] == 0
    assert call(1, stats_out=True)[0] == 0 and call(1, ln_part=True, ln_nparts=1)[0] == 0
    assert call(1, a_bf16=1, res=True)[0] == 0 and call(1, c_bf16=1, ln_stats=True)[0] == 0
    # the entry's own argument checks
    for kw in (dict(mode=0), dict(mode=3), dict(mode=1, tile=3), dict(mode=2, tile=1), dict(mode=1, K=48), dict(mode=1, act=3), dict(mode=1, reserved=1),
               dict(mode=1, lda=66), dict(mode=1, a_bf16=1, res=True, lda=68), dict(mode=1, ldc=99)):
        assert call(**kw)[0] == L.DSG_ERR_INVALID, kw
    a = L.DsgGemmLpArgs()      # the wide tile below 256 rows
    a.M, a.N, a.K, a.mode, a.tile, a.lda, a.ldc = 255, N, 64, 1, 2, Kmax, N
    a.A, a.W, a.C = dev["A"].data_ptr(), dev["W"].data_ptr(), outs["C"].data_ptr()
    assert lib.dsg_debug_gemm_lp(C.byref(a), None) == L.DSG_ERR_INVALID


# ----------------------------------------------------------------------------------------------------------------------------------
# the conversion kernels, bit for bit
# ----------------------------------------------------------------------------------------------------------------------------------
def _convert(kind, src, n_out, dtype):
    from diffusesg_amd import lib as L
    dst = torch.zeros(n_out + 8, dtype=dtype, device="cuda")      # eight guard elements behind the result
    n = src.numel()
    rc = L.load().dsg_debug_convert(kind, C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), n, None)
    assert rc == 0
    assert int(dst[n_out:].view(torch.int16 if dtype == torch.bfloat16 else torch.int32).abs().sum()) == 0, "wrote past the result"
    return dst[:n_out]


def _values():
    return np.concatenate([P.special_values(), P.random_values()])


def test_convert_round_to_nearest_even_bits():
    """f32_to_bf16_kernel: ties to even in both directions, +-0, denormals, the largest finite values (to inf), +-inf, a random million;
    the quiet NaN stays 0x7fc0 (other payloads are not special-cased: include/dsg_debug.h)"""
    from diffusesg_amd import lib as L
    x = np.concatenate([_values(), np.array([NAN32], np.uint32).view(np.float32)])
    got = _convert(L.CONVERT_BF16, torch.from_numpy(x).cuda(), x.size, torch.bfloat16).view(torch.int16).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, P.bf16_rne_bits(x))
    assert got[-1] == NAN16


def test_convert_split_planes_bits_and_exact_sum():
    """f32_split3_kernel: the three planes are the restatement's bits; they sum back to the input exactly (float64) for 0 and
    |x| >= 2^-110; +-inf gives hi = itself and NaN behind it"""
    from diffusesg_amd import lib as L
    x = _values()
    fin = np.isfinite(x)
    n = x.size
    got = _convert(L.CONVERT_SPLIT3, torch.from_numpy(x).cuda(), 3 * n, torch.bfloat16).view(torch.int16).cpu().numpy().view(np.uint16).reshape(3, n)
    want = P.split3_bits(x)
    for q in range(3):
        assert np.array_equal(got[q][fin], want[q][fin]), f"plane {q}"
    assert np.array_equal(got[0], (x.view(np.uint32) >> 16).astype(np.uint16))
    assert np.isnan(P.widen(got[1][~fin])).all() and np.isnan(P.widen(got[2][~fin])).all()
    tot = sum(P.widen(got[q]).astype(np.float64) for q in range(3))
    big = fin & ((np.abs(x) >= 2.0 ** -110) | (x == 0))
    assert big.sum() > 900_000 and np.array_equal(tot[big], x.astype(np.float64)[big])


def test_convert_widen_is_exact():
    """bf16_to_f32_kernel on all 65536 bit patterns"""
    from diffusesg_amd import lib as L
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    src = torch.from_numpy(bits.view(np.int16)).cuda().view(torch.bfloat16)
    got = _convert(L.CONVERT_WIDEN, src, bits.size, torch.float32).view(torch.int32).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, bits.astype(np.uint32) << 16)


# ----------------------------------------------------------------------------------------------------------------------------------
# the row passes' bf16-tensor forms: the fp32 form's bar plus the bf16 store's half spacing (lp_ref's header)
# ----------------------------------------------------------------------------------------------------------------------------------
def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def _check_bf16_rows(what, out, M, ref, bound, rows=None):
    """out: bf16 [M + GUARD, cols] from the device; rows (bool [M]; all when None) hold ref within bound, everything else the NaN fill"""
    keep, got = _untouched(out), out.float().cpu()
    must = torch.zeros_like(keep)
    must[:M][slice(None) if rows is None else rows] = True
    assert keep[~must].all(), f"{what}: {int((~keep[~must]).sum())} elements written outside the result"
    sel = slice(None) if rows is None else rows
    assert torch.isfinite(got[:M][sel]).all(), f"{what}: non-finite values in the result"
    r = R.worst_ratio(got[:M][sel], ref[sel], bound[sel])
    print(f"LPKROW {what} worst |err| / bound = {r:.3f}")
    assert r <= 1.0, f"{what}: {r:.2f} x the derived bound"


def _formula_bound(f64, f32):
    bar, _ = R.formula_bar(f64, f32)
    return P.with_bf16_store(f64, torch.full_like(f64, bar))


# (B, res, ws, shift, heads): units = B nW heads is never a multiple of 4; every window size the kernel is built for, shift 0 and ws / 2
WATTN_CASES = [(1, 6, 2, 0, 3), (1, 6, 2, 1, 1), (3, 4, 4, 0, 1), (1, 12, 4, 2, 1), (3, 5, 5, 0, 3), (1, 15, 5, 2, 1), (1, 8, 8, 0, 3),
               (1, 24, 8, 4, 1), (1, 10, 10, 0, 3), (1, 30, 10, 5, 1)]


@pytest.mark.parametrize("in_bf16", (0, 1), ids=("out_bf16", "in_out_bf16"))
@pytest.mark.parametrize("B,res,ws,shift,heads", WATTN_CASES)
def test_window_attn_bf16_tensors(B, res, ws, shift, heads, in_bf16):
    from diffusesg_amd import lib as L
    lib = L.load()
    Cc, M, nW = 32 * heads, B * res * res, (res // ws) ** 2
    gen = _gen(5800 + WATTN_CASES.index((B, res, ws, shift, heads)))
    qkv = torch.randn(M, 3 * Cc, generator=gen)
    qkv[:, :Cc] *= 32 ** -0.5 * R.LOG2E
    if in_bf16:
        qkv = torch.from_numpy(P.bf16_rne(qkv.numpy()))      # the tensor's values; the kernel widens them exactly
    bias = R.make_attn_bias(nW, heads, ws, shift, gen)
    f64, f32 = R.attn_formula(qkv.double(), bias, B, res, ws, shift, heads), R.attn_formula(qkv, bias, B, res, ws, shift, heads)
    dq, db, out = _dev(qkv.to(torch.bfloat16) if in_bf16 else qkv), _dev(bias), _nan(M, Cc, torch.bfloat16)
    assert lib.dsg_debug_window_attn_lp(B, res, ws, shift, heads, _p(dq), _p(db), _p(out), in_bf16, 1, None) == 0
    _check_bf16_rows(f"window_attn ws={ws} in_bf16={in_bf16}", out, M, f64, _formula_bound(f64, f32))


def test_window_attn_bf16_input_needs_bf16_output():
    from diffusesg_amd import lib as L
    lib = L.load()
    dq, db, out = torch.zeros(36, 96, device="cuda", dtype=torch.bfloat16), torch.zeros(9, 1, 32, 32, device="cuda"), _nan(36, 32)
    assert lib.dsg_debug_window_attn_lp(1, 6, 2, 0, 1, _p(dq), _p(db), _p(out), 1, 0, None) == L.DSG_ERR_INVALID
    assert _untouched(out).all()
    assert lib.dsg_debug_window_attn_lp(1, 6, 3, 0, 1, _p(dq), _p(db), _p(out), 0, 1, None) == L.DSG_ERR_INVALID      # no 3 x 3 windows
    assert _untouched(out).all()


def _rowlp(lib, kind, B, t, Cc, x, y, g=None, b=None, pg=None, pb=None, aff=None, aff_ld=0, aff_off=0, run_list=None, run_cnt=None):
    return lib.dsg_debug_row_lp(kind, B, t, Cc, _p(x), _p(g), _p(b), _p(pg), _p(pb), _p(aff), aff_ld, aff_off, _p(y), _p(run_list), _p(run_cnt), None)


def _rows(M, Cc, gen):
    return torch.randn(M, Cc, generator=gen) + 2.0 * (2.0 * torch.rand(M, 1, generator=gen) - 1.0)


@pytest.mark.parametrize("res", (2, 6))
@pytest.mark.parametrize("Cc", (96, 192, 384))
def test_merge_ln_bf16_output(Cc, res):
    """PatchMerging's gather + LayerNorm(4C) stored as bf16, B = 3: 3 and 27 merged rows (a last block of three rows)"""
    from diffusesg_amd import lib as L
    lib = L.load()
    gen, B = _gen(res * 1100 + Cc), 3
    M2 = B * (res // 2) ** 2
    x = _rows(B * res * res, Cc, gen)
    gam, bet = 1.0 + 0.2 * torch.randn(4 * Cc, generator=gen), 0.2 * torch.randn(4 * Cc, generator=gen)
    dx, dg, db, y = _dev(x), _dev(gam), _dev(bet), _nan(M2, 4 * Cc, torch.bfloat16)
    assert _rowlp(lib, L.ROWLP_MERGE_LN, B, res, Cc, dx, y, g=dg, b=db) == 0
    f64, f32 = X.merge_ln_formula(x.double(), gam.double(), bet.double(), B, res), X.merge_ln_formula(x, gam, bet, B, res)
    _check_bf16_rows(f"merge_ln C={Cc} res={res}", y, M2, f64, _formula_bound(f64, f32))


def _breakup_operands(D, M, gen):
    rn = lambda n: torch.randn(n, generator=gen)
    return _rows(M, D, gen), 1.0 + 0.2 * rn(D), 0.2 * rn(D), 1.0 + 0.2 * rn(D // 4), 0.2 * rn(D // 4)


@pytest.mark.parametrize("res", (1, 3))
@pytest.mark.parametrize("D", (384, 768, 1536))
def test_breakup_ln_bf16_output(D, res):
    """PatchBreakup's middle with z stored as bf16 (the input row stays fp32), output widths 96, 192, 384, B = 3: 3 and 27 coarse rows"""
    from diffusesg_amd import lib as L
    lib = L.load()
    B = 3
    M, Mf = B * res * res, B * 4 * res * res
    ops = _breakup_operands(D, M, _gen(res * 7100 + D))
    dev, z = [_dev(v) for v in ops], _nan(Mf, D // 4, torch.bfloat16)
    assert _rowlp(lib, L.ROWLP_BREAKUP_LN, B, res, D, dev[0], z, g=dev[1], b=dev[2], pg=dev[3], pb=dev[4]) == 0
    f64, f32 = X.breakup_formula(*(v.double() for v in ops), B, res), X.breakup_formula(*ops, B, res)
    _check_bf16_rows(f"breakup_ln D={D} res={res}", z, Mf, f64, _formula_bound(f64, f32))


@pytest.mark.parametrize("D", (384, 1536))
def test_breakup_ln_bf16_output_run_list(D):
    """a run list over the coarse rows: counts 0, 1 and all, a -1 inside the list; sentinel runs and runs beyond the count write nothing"""
    from diffusesg_amd import lib as L
    lib = L.load()
    B, res = 3, 4
    gen = _gen(8100 + D)
    M, Mf, n_runs = B * res * res, B * 4 * res * res, B * res * res // 8
    ops = _breakup_operands(D, M, gen)
    dev = [_dev(v) for v in ops]
    f64, f32 = X.breakup_formula(*(v.double() for v in ops), B, res), X.breakup_formula(*ops, B, res)
    bound = _formula_bound(f64, f32)
    lst = torch.randperm(n_runs, generator=gen).tolist()
    lst[1] = -1
    d_list = _i32(lst)
    for cnt in (0, 1, n_runs):
        z, d_cnt = _nan(Mf, D // 4, torch.bfloat16), _i32([cnt])
        assert _rowlp(lib, L.ROWLP_BREAKUP_LN, B, res, D, dev[0], z, g=dev[1], b=dev[2], pg=dev[3], pb=dev[4], run_list=d_list, run_cnt=d_cnt) == 0
        rows = X.breakup_rows(B, res, [r for r in lst[:cnt] if r >= 0])
        _check_bf16_rows(f"breakup_ln run list D={D} count {cnt}", z, Mf, f64, bound, rows)


@pytest.mark.parametrize("mod", ("plain", "uniform", "per_sample"))
@pytest.mark.parametrize("ln", (1, 0), ids=("ln", "copy"))
@pytest.mark.parametrize("Cc", (96, 192, 384))
def test_ln_bx(Cc, ln, mod):
    """ln_bx_kernel at M = 1, 3, 4, 5, 9 rows (a sample boundary inside a block of four rows, a last block of one row): the LayerNorm
    without affine, or the plain copy, of the row as bf16 -- of the row the kernel has just modulated in place when aff is given
    (aff_ld = 0: one (scale | shift) row for the batch; per sample: aff_off != 0, aff_ld > 2 C).  The in-place row keeps the fp32 bar."""
    from diffusesg_amd import lib as L
    lib = L.load()
    off, ld = 8, 8 + 2 * Cc + 4
    for B, T in X.ROW_BT:
        gen, M = _gen(2000 + Cc + 10 * B + T), B * T
        x = _rows(M, Cc, gen)
        aff = torch.randn(B if mod == "per_sample" else 1, ld, generator=gen) * 0.5
        x_io = torch.cat([x, torch.full((GUARD, Cc), float("nan"))]).cuda()
        x_in, xn = x_io.clone(), _nan(M, Cc, torch.bfloat16)
        daff = None if mod == "plain" else _dev(aff)
        kind = L.ROWLP_LN_BX if ln else L.ROWLP_COPY_BX
        assert _rowlp(lib, kind, B, T, Cc, x_io, xn, aff=daff, aff_ld=(ld if mod == "per_sample" else 0), aff_off=(0 if mod == "plain" else off)) == 0
        assert torch.equal(x_io[M:].view(torch.int32), x_in[M:].view(torch.int32)), "wrote behind the rows of x"
        stored = x_io.cpu()[:M]
        if mod == "plain":
            assert torch.equal(stored.view(torch.int32), x.view(torch.int32)), "x changed without a modulation"
        else:
            Tm = T if mod == "per_sample" else M
            f64, f32 = X.modulate(x.double(), aff.double(), off, Tm), X.modulate(x, aff, off, Tm)
            bar, _ = R.formula_bar(f64, f32)
            r = R.worst_ratio(stored, f64, torch.full_like(f64, bar))
            print(f"LPKROW ln_bx in-place row C={Cc} {mod} M={M} worst |err| / bound = {r:.3f}")
            assert r <= 1.0
        if ln:
            ref = R.layer_norm(stored.double())
            _check_bf16_rows(f"ln_bx ln C={Cc} {mod} M={M}", xn, M, ref, P.with_bf16_store(ref, X.ln_elem_bound(stored.double())))
        else:
            keep = _untouched(xn)
            assert keep[M:].all(), "guard rows were written"
            got = xn[:M].view(torch.int16).cpu().numpy().view(np.uint16)
            assert np.array_equal(got, P.bf16_rne_bits(stored.numpy())), "the bf16 copy is not the round-to-nearest-even of the stored row"
