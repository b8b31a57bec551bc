"""GPU: the thin form of the list GEMM (csrc/kernels.hip: gemm4_thin_tile, 64 x 96 block tiles, N-waves owning the 32-column slabs
{0, 1} and {2}) against the wide form (128 x 96) on the same inputs, through dsg_debug_gemm_f32 with `reserved` = 1 (wide) and 2 (thin).

The two forms must agree BIT FOR BIT in C, C2 and stats_out -- the whole buffers are compared as int32, so the NaN fill of rows of
unlisted runs, of padding columns and of the guard rows has to survive in both -- because the pruned and deduplicated paths of the
forward are held bit-identical to the full launches.  The thin form is also compared with the float64 reference under the bars of
tests/f32_ref.py, like the wide form in tests/test_f32_kernels.py.

Shapes: a tensor of 32 runs (256 rows); lists of 0, 1, 7, 8, 9, 16, 17 and 32 scattered runs padded with -1 to a multiple of 16, so
that full, partial and skipped 64-row tiles, the last tile's sentinels and (in a list of its own) a tile of sentinels only all occur;
N in {96, 100, 192, 384} (100: a last column tile with one slab and four columns of the next); K in {32, 64, 96, 384}: one chunk, even
and odd chunk counts.  Forms: every instantiation the list launcher admits without LayerNorm -- res x EPI 0..3 (40-row samples, so
sample boundaries fall inside the tiles for EPI 3), the dual store, the A2 concat."""
import ctypes as C

import pytest
import torch

import f32_ref as R
from f32_ref import GemmCase

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000
GUARD = 2      # rows behind every output buffer
RUNS = 32      # runs of the tensor: M = 256 rows
COUNTS = (0, 1, 7, 8, 9, 16, 17, 32)
NS = (96, 100, 192, 384)
KS = (32, 64, 96, 384)

FORMS = [dict(res=r, epi=e, mod_T=40, mod_off=4) for r in (False, True) for e in (0, 1, 2, 3)]
FORMS += [dict(c2=True), dict(c2=True, epi=2, mod_off=4), dict(c2=True, epi=3, mod_T=40),      # dual store (no residual with it)
          dict(K1=32), dict(K1=64, res=True, epi=1)]                                            # A2 concat


def _form_id(f):
    return "-".join(f"{k}{int(v) if isinstance(v, bool) else v}" for k, v in f.items()) or "plain"


def _dev(t):
    return None if t is None else t.contiguous().cuda()


def _nan(rows, cols):
    return torch.full((rows + GUARD, cols), float("nan"), device="cuda")


def _bits(buf):
    return None if buf is None else buf.view(torch.int32).cpu()


def _launch(c, o, dev, form, want_c2, cnt=None):
    """one launch in the given form on NaN-filled outputs -> (status, C, C2, stats_out) as int32 bit patterns on the CPU"""
    from diffusesg_amd import lib as L
    lib = L.load()
    a = L.DsgGemmF32Args()
    out_C = _nan(c.M, o["ldc"])
    out_C2 = _nan(c.M, o["ldc2"]) if want_c2 else None
    out_S = _nan(c.M, 2 * c.tiles_n) if c.epi >= 1 else None
    d_cnt = torch.tensor([c.cnt if cnt is None else cnt], dtype=torch.int32, device="cuda")
    for name, t in (("A", dev["A"]), ("A2", dev["A2"]), ("W", dev["W"]), ("bias", dev["bias"]), ("res", dev["res"]), ("C", out_C), ("C2", out_C2),
                    ("mod_aff", dev["mod_aff"]), ("stats_out", out_S), ("row_list", dev["row_list"]), ("row_cnt", d_cnt)):
        setattr(a, name, None if t is None else t.data_ptr())
    a.lda, a.lda2, a.K1 = o["lda"], o.get("lda2", 0), c.K1
    a.ldres, a.ldc, a.ldc2 = (o["ldres"] if c.res else 0), o["ldc"], (o["ldc2"] if want_c2 else 0)
    a.M, a.N, a.K, a.act = c.M, c.N, c.K, c.act
    a.mod_ld, a.mod_off, a.mod_T = o.get("mod_ld", 0), c.mod_off, c.mod_T
    a.reserved = form
    rc = lib.dsg_debug_gemm_f32(C.byref(a), None)
    return rc, out_C, out_C2, out_S


def _device_operands(o):
    dev = {k: _dev(o.get(k)) for k in ("A", "A2", "W", "bias", "res", "mod_aff")}
    dev["row_list"] = torch.tensor(o["row_list"], dtype=torch.int32, device="cuda")
    return dev


def _rows_mask(M, runs):
    m = torch.zeros(M + GUARD, dtype=torch.bool)
    for r in runs:
        m[8 * r:8 * r + 8] = True
    return m


def _check_written(buf, N, rows, ref, bound, what):
    """buf [M + GUARD, ld]: rows `rows`, columns < N hold the float64 reference within the bound; all else keeps the NaN fill"""
    got, keep = buf.cpu(), _bits(buf) == NAN_BITS
    must = torch.zeros_like(keep)
    must[rows, :N] = True
    assert keep[~must].all(), f"{what}: {int((~keep[~must]).sum())} elements written outside the rows / columns of the result"
    M = ref.shape[0]
    sel = rows[:M]
    assert torch.isfinite(got[:M][sel][:, :N]).all(), f"{what}: non-finite values in the result"
    r = R.worst_ratio(got[:M][sel][:, :N], ref[sel], bound[sel])
    print(f"GEMMTHIN {what} worst |err| / bound = {r:.3f}")
    assert r <= 1.0, f"{what}: {r:.2f} x the derived bound"
    return got


def _compare_forms(c, o, what):
    """wide against thin, bit for bit; thin against float64"""
    ref = R.gemm_expect(o)
    dev = _device_operands(o)
    want_c2 = "C2" in ref
    rc1, C1, C21, S1 = _launch(c, o, dev, 1, want_c2)
    rc2, C2_, C22, S2 = _launch(c, o, dev, 2, want_c2)
    assert rc1 == 0 and rc2 == 0, f"{what}: dsg_debug_gemm_f32 refused a form (wide {rc1}, thin {rc2})"
    for name, w, t in (("C", C1, C2_), ("C2", C21, C22), ("stats_out", S1, S2)):
        if w is None:
            continue
        bw, bt = _bits(w), _bits(t)
        assert torch.equal(bw, bt), f"{what}: {name} differs between the forms in {int((bw != bt).sum())} elements"
    rows = _rows_mask(c.M, o["runs"])
    got_C = _check_written(C2_, c.N, rows, ref["C"], ref["bC"], f"{what} C")
    if want_c2:
        _check_written(C22, c.N, rows, ref["C2"], ref["bC2"], f"{what} C2")
    if S2 is not None:
        S, Bd = R.stats_expect(torch.nan_to_num(got_C[:c.M, :c.N]), c, ref["C"], ref["bC"])
        _check_written(S2, 2 * c.tiles_n, rows, S.reshape(c.M, -1), Bd.reshape(c.M, -1), f"{what} stats_out")


@pytest.mark.parametrize("form", FORMS, ids=[_form_id(f) for f in FORMS])
def test_thin_form_matches_wide_form(form):
    """every list length with every form; N and K walk through their sets so that each form meets each N and each K"""
    f = FORMS.index(form)
    for j, cnt in enumerate(COUNTS):
        N = NS[(f + j) % 4]
        K = (96, 384)[j % 2] if form.get("K1") else KS[(f // 4 + j) % 4]
        c = GemmCase(8 * RUNS, N, K, cnt=cnt, stale=(1 if cnt in (0, 1, 8, 16) else 0), seed=1400 + 10 * f + j, **form)
        _compare_forms(c, R.make_gemm(c), c.ident())


def test_thin_form_sentinels_inside_the_count():
    """-1 entries in front of the count: a 64-row tile with four sentinel runs and one of sentinels only, both below the count"""
    c = GemmCase(8 * RUNS, 192, 64, res=True, epi=3, mod_T=40, mod_off=4, cnt=24, seed=1490)
    o = R.make_gemm(c)
    o["runs"] = [30, 2, 17, 9, 4, 21, 11]
    o["row_list"] = [30, -1, 2, -1, -1, 17, 9, -1] + [-1] * 8 + [4, 21, -1, 11, -1, -1, -1, -1] + [-1] * 8
    _compare_forms(c, o, "sentinels inside the count")


def test_rule_on_either_side_of_its_threshold():
    """reserved = 0: the kernel's own rule.  At N = 384 (four column tiles) the largest list that qualifies fills n_cu / 8 wide row tiles;
    sixteen runs more do not.  Either way the bits are those of the forced forms."""
    from diffusesg_amd import lib as L
    lib = L.load()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    lo = 16 * (n_cu // 8)
    hi = lo + 16
    assert lib.dsg_debug_gemm_form(lo, 384, n_cu) == 2 and lib.dsg_debug_gemm_form(hi, 384, n_cu) == 1
    c = GemmCase(8 * (hi + 16), 384, 32, res=True, epi=1, cnt=hi, seed=1495)
    o = R.make_gemm(c)
    dev = _device_operands(o)
    for cnt in (lo, hi):
        outs = {}
        for frm in (0, 1, 2):
            rc, Cc, _, S = _launch(c, o, dev, frm, False, cnt=cnt)
            assert rc == 0
            outs[frm] = (_bits(Cc), _bits(S))
        for frm in (1, 2):
            assert torch.equal(outs[0][0], outs[frm][0]) and torch.equal(outs[0][1], outs[frm][1]), f"count {cnt}: rule against form {frm}"
        rows = _rows_mask(c.M, o["row_list"][:cnt])
        assert (outs[0][0][~rows] == NAN_BITS).all() and not (outs[0][0][rows] == NAN_BITS).any()


def test_thin_form_is_refused_where_it_is_not_built():
    """form 2 without a list or with LayerNorm on the way in, and an unknown form: DSG_ERR_INVALID, never an abort"""
    from diffusesg_amd import lib as L
    lib = L.load()
    o = R.make_gemm(GemmCase(16, 96, 32, ln="stats", seed=1))
    dA, dW, dst = _dev(o["A"]), _dev(o["W"]), _dev(o["ln_stats"])
    out_C = _nan(16, 96)
    d_list = torch.tensor([0, 1] + [-1] * 14, dtype=torch.int32, device="cuda")
    d_cnt = torch.tensor([2], dtype=torch.int32, device="cuda")

    def call(**kw):
        a = L.DsgGemmF32Args()
        a.A, a.W, a.C, a.lda, a.ldc, a.M, a.N, a.K = dA.data_ptr(), dW.data_ptr(), out_C.data_ptr(), 32, 96, 16, 96, 32
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.dsg_debug_gemm_f32(C.byref(a), None)
    lst = dict(row_list=d_list.data_ptr(), row_cnt=d_cnt.data_ptr())
    assert call(reserved=1) == 0 and call(reserved=2, **lst) == 0
    assert call(reserved=2) == L.DSG_ERR_INVALID                                              # no list
    assert call(reserved=2, ln_stats=dst.data_ptr(), act=R.ACT_GELU, **lst) == L.DSG_ERR_INVALID   # the LayerNorm list form has no thin kernel
    assert call(reserved=1, ln_stats=dst.data_ptr(), act=R.ACT_GELU, **lst) == 0
    assert call(reserved=3) == L.DSG_ERR_INVALID and call(reserved=-1) == L.DSG_ERR_INVALID
