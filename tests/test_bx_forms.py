"""GPU: the bf16 block pipeline's GEMM and fused-MLP kernels (csrc/kernels_bx.hip) on their own, form by form, through
dsg_debug_gemm_bx_args and dsg_debug_mlp_bx_args: the hooks hand the caller's own bf16 tensors to launch_gemm_bx / launch_mlp_bx with
every field of the launcher's argument block -- per-sample modulate rows (MOD 2), mod_off, the second source, pitches, C aliasing the
residual -- and write only what the kernel writes.  EVERY output element is compared with the float64 reference of tests/bx_ref.py
inside bars derived there (gemm_bx: the summation bound on exact products; the fused MLP: the derived per-element bar on exact operands,
tests/test_bx_kernels.py's flat bars on dense ones); what a kernel derives from a row it has just stored (the bf16 copy, the LayerNorm)
is held to THAT row, bit for bit where the kernel rounds the same register.

Every output buffer is filled with NaN, has a pitch wider than the result and GUARD rows behind it: rows < M and columns < N must be
finite and inside the bar, everything else bit-identical afterwards; operands are unchanged unless aliased.  The cases (bx_ref; shared
with tests/test_bx_forms_host.py, which shows that a NumPy emulation passes every one and the seeded mistakes do not) are the smallest
that reach each edge; the four persistence cases are sized from the device's CU count.  Measured figures: profiles/bx_kernel_errors.md
(each test prints its own: BXK <family> <buffer> worst |err| / bound = r)."""
import ctypes as C

import numpy as np
import pytest
import torch

import bx_ref as B

pytestmark = pytest.mark.gpu


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _bf16(t):
    """float32 holding bf16 values -> a bf16 device tensor (exact)"""
    return t.to(torch.bfloat16).contiguous().cuda()


def _from_bits(a):
    """uint32 / uint16 bit patterns -> a float32 / bf16 device tensor with those bits"""
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32).copy()).cuda().view(torch.float32)
    return torch.from_numpy(a.view(np.int16).copy()).cuda().view(torch.bfloat16)


def _to_bits(t):
    if t.dtype == torch.float32:
        return t.view(torch.int32).cpu().numpy().view(np.uint32)
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _report(fam, ident, r):
    for k, v in sorted(r.items()):
        print(f"BXK {fam} {k} worst |err| / bound = {v:.3f}   [{ident}]")
    assert max(r.values()) <= 1.0, f"{ident}: " + ", ".join(f"{k} {v:.3g}" for k, v in r.items() if v > 1.0) + " x the derived bound"


# ----------------------------------------------------------------------------------------------------------------------------------
# gemm_bx_kernel
# ----------------------------------------------------------------------------------------------------------------------------------
def launch_gemm(o, init):
    """one dsg_debug_gemm_bx_args launch of the case: (status, geometry used, the output buffers after as bit patterns)"""
    from diffusesg_amd import lib as L
    lib = L.load()
    c = o["bx"]
    ops = {"A": _bf16(o["A"]), "A2": _bf16(o["A2"]) if c.K1 else None, "W": _bf16(o["W"]), "bias": o["bias"].cuda() if c.bias else None,
           "mod_aff": o["mod_aff"].contiguous().cuda() if c.mod else None}
    bufs = {k: (None if v is None else _from_bits(v)) for k, v in init.items()}
    if c.res:
        ops["res"] = bufs["C"] if c.alias else o["res"].contiguous().cuda()
    before = {k: v.clone() for k, v in ops.items() if v is not None and not (k == "res" and c.alias)}
    a = L.DsgBxGemmArgs()
    for k, t in list(ops.items()) + list(bufs.items()):
        setattr(a, k, _ptr(t))
    geo = C.c_int32(-7)
    a.geo_used = C.addressof(geo)
    a.lda, a.lda2, a.K1, a.ldres, a.ldc, a.ldcb, a.ldc2b = o["lda"], o["lda2"], c.K1, (o["ldres"] if c.res else 0), o["ldc"], o["ldcb"], o["ldc2b"]
    a.M, a.N, a.K, a.act, a.ln_out = c.M, c.N, c.K, c.act, int(c.ln)
    a.mod_ld, a.mod_off, a.mod_T = o.get("mod_ld", 0), c.mod_off, c.T
    rc = lib.dsg_debug_gemm_bx_args(C.byref(a), None)
    for k, t in before.items():
        assert torch.equal(t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32), ops[k].view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)), \
            f"operand {k} changed"
    return rc, geo.value, {k: (None if t is None else _to_bits(t)) for k, t in bufs.items()}


def run_gemm(c):
    o = B.make_gemm(c)
    ref = B.gemm_expect(o)
    init = B.gemm_buffers(o)
    rc, geo, got = launch_gemm(o, init)
    assert rc == 0, f"dsg_debug_gemm_bx_args refused {c.ident()} (status {rc})"
    assert geo == c.geo, f"{c.ident()}: ran geometry {geo}"
    _report(c.fam, c.ident(), B.check_gemm(o, ref, init, got))


GEMM = B.gemm_cases()


@pytest.mark.parametrize("case", GEMM, ids=[c.ident() for c in GEMM])
def test_gemm_bx_forms(case):
    """every epilogue family the forward launches (qkv, fc1, proj, fc2 with and without LayerNorm, the level's last copy, merge,
    pre_linear with two sources, post_linear) on each of the three tile geometries, at M = 1, BM - 1, BM, BM + 1, 8 BM + 1 (nine row
    tiles: the second group of eight ids almost all padding) and 17 BM + 3; N with a half-used last slab; K ending inside a chunk, of
    exactly two chunks, of an odd chunk count, and 1536; MOD 0 / 1 / 2 with mod_off 0 and 2N + 8, 36-row samples at M = 324 and one
    sample; pitches"""
    run_gemm(case)


@pytest.mark.parametrize("which", [0, 1, 2], ids=["geo0", "geo2", "geo3"])
def test_gemm_bx_persistent_second_tile(which):
    """the grid is min(tiles, resident blocks): with nine row-tile groups more than resident blocks a block takes a second tile, and
    the last group of eight ids is all padding but one"""
    run_gemm(B.persistence_cases(_cus())[which])


def test_gemm_bx_refused_forms_write_nothing():
    """bx_ref.REFUSALS: each refused form returns DSG_ERR_INVALID with geo_used == -1 and every output still NaN, and the neighbouring
    admitted form, which differs in the one named field, runs"""
    from diffusesg_amd import lib as L
    lib = L.load()
    M, LD = 300, 400
    gen = torch.Generator().manual_seed(3)
    A, A2, W = (_bf16(torch.randn(r, 256, generator=gen)) for r in (M, M, LD))
    bias, res = torch.randn(LD, generator=gen).cuda(), torch.randn(M, LD, generator=gen).cuda()
    fresh = lambda dt: torch.full((M + B.GUARD, LD), float("nan"), dtype=dt, device="cuda")
    outs = {"C": fresh(torch.float32), "Cb": fresh(torch.bfloat16), "C2b": fresh(torch.bfloat16)}

    def call(kw):
        p = B.refusal_args(kw)
        a = L.DsgBxGemmArgs()
        a.A, a.W, a.bias, a.C = A.data_ptr(), W.data_ptr(), bias.data_ptr(), outs["C"].data_ptr()
        a.M, a.N, a.K, a.act, a.lda, a.ldc, a.ln_out, a.mod_T = p["M"], p["N"], p["K"], p["act"], p["lda"], p["ldc"], int(p["ln"]), 1
        if p["K1"]:
            a.A2, a.lda2, a.K1 = A2.data_ptr(), p["lda2"], p["K1"]
        if p["res"]:
            a.res, a.ldres = res.data_ptr(), LD
        if p["cb"]:
            a.Cb, a.ldcb = outs["Cb"].data_ptr(), p["ldcb"]
        if p["c2b"]:
            a.C2b, a.ldc2b = outs["C2b"].data_ptr(), p["ldc2b"]
        geo = C.c_int32(-7)
        a.geo_used = C.addressof(geo)
        return lib.dsg_debug_gemm_bx_args(C.byref(a), None), geo.value

    def all_nan():
        return all(bool((_to_bits(t) == (B.NAN32 if t.dtype == torch.float32 else B.NAN16)).all()) for t in outs.values())
    for name, ok, bad in B.REFUSALS:
        rc, geo = call(bad)
        assert rc == L.DSG_ERR_INVALID and geo == -1, f"{name}: status {rc}, geometry {geo}"
        assert all_nan(), f"{name}: an output was written"
        rc, geo = call(ok)
        assert rc == 0 and geo == B.gemm_rule(**B.refusal_args(ok)), f"{name}: the admitted neighbour gave status {rc}, geometry {geo}"
        for t in outs.values():
            t.fill_(float("nan"))
    print("BXK refused forms: " + "; ".join(n for n, _, _ in B.REFUSALS))


# ----------------------------------------------------------------------------------------------------------------------------------
# the fused MLP kernels
# ----------------------------------------------------------------------------------------------------------------------------------
def launch_mlp(o, init):
    from diffusesg_amd import lib as L
    lib = L.load()
    c = o["mlp"]
    ops = {("att" if c.proj else "xn"): _bf16(o["in"]), "W1": _bf16(o["W1"]), "W2": _bf16(o["W2"]), "b1": o["b1"].float().cuda(), "b2": o["b2"].float().cuda()}
    if c.proj:
        ops["Wp"], ops["bp"] = _bf16(o["Wp"]), o["bp"].float().cuda()
    if c.mod:
        ops["mod_aff"] = o["mod_aff"].contiguous().cuda()
    bufs = {k: (None if v is None else _from_bits(v)) for k, v in init.items()}
    before = {k: v.clone() for k, v in ops.items()}
    a = L.DsgBxMlpArgs()
    for k, t in list(ops.items()) + list(bufs.items()):
        setattr(a, k, _ptr(t))
    a.out_mode, a.mod_ld, a.mod_off, a.mod_T, a.M, a.C = c.out_mode, o.get("mod_ld", 0), c.mod_off, c.T, c.M, c.C
    a.kernel = getattr(L, "BXK_" + c.selector)
    rc = lib.dsg_debug_mlp_bx_args(C.byref(a), None)
    for k, t in before.items():
        it = torch.int16 if t.dtype == torch.bfloat16 else torch.int32
        assert torch.equal(t.view(it), ops[k].view(it)), f"operand {k} changed"
    return rc, {k: (None if t is None else _to_bits(t)) for k, t in bufs.items()}


def run_mlp(c, device="cpu"):
    o = B.make_mlp(c, device)
    ref = B.mlp_expect(o)
    assert B.mlp_rule(c) == B.MLP_KERNELS[c.kern][2]
    init = B.mlp_buffers(o)
    rc, got = launch_mlp(o, init)
    assert rc == 0, f"dsg_debug_mlp_bx_args refused {c.ident()} (status {rc})"
    if c.exact:
        print(f"BXK exact {c.ident()}: flagged LN-2 {ref['flag_ln']:.3f}, hidden {ref['flag_h']:.3f}; bar < {B.TIGHT:g} scale on {ref['tight']:.3f} of the outputs")
        assert ref["flag_ln"] <= B.FLAG_CAP and ref["flag_h"] <= B.FLAG_CAP and ref["tight"] >= 0.5
    fam = f"{c.kern}{'+proj' if c.proj else ''}{'-exact' if c.exact else '-dense'}"
    _report(fam, c.ident(), B.check_mlp(o, ref, init, got))


DENSE, EXACT = B.mlp_dense_cases(), B.mlp_exact_cases()


@pytest.mark.parametrize("case", DENSE, ids=[c.ident() for c in DENSE])
def test_mlp_bx_dense(case):
    """every kernel launch_mlp_bx can reach, with and without the proj stage, at M = 1, 31, 32, 33, 127, 128, 129, 257 (a wave owns 32
    tokens, a block 128) and 324 in 36-row samples; MOD 0 / 1 / 2, mod_off 0 and 2C + 8, out_mode 0 / 1 / 2.  Dense operands pin
    indexing inside tests/test_bx_kernels.py's bars; the bf16 output is held to the stored row"""
    run_mlp(case)


@pytest.mark.parametrize("case", EXACT, ids=[c.ident() for c in EXACT])
def test_mlp_bx_exact(case):
    """exact operands (bx_ref.exact_mlp_case): the derived per-element bar, about 1e-6 of the output scale where no rounded element
    sits on a bf16 boundary"""
    run_mlp(case)


def test_mlp96r_second_round():
    """mlp96r_bx_kernel deals 32-row tiles to the eight waves of at most one block per CU: with more than 8 CUs tiles a block takes a
    second round (reference in float64 on the device)"""
    run_mlp(B.mlp96r_round2_case(_cus()), device="cuda")


def test_mlp_bx_refused_selectors_write_nothing():
    """the selectors the old hooks refuse are refused here: nothing launched, x and xn_out untouched"""
    from diffusesg_amd import lib as L
    lib = L.load()
    for kern, proj, mod, sel in (("mlp384d", True, 0, "MLP384_WAVE"), ("mlp96", True, 1, "MLP96_RESIDENT"), ("mlp96", False, 0, "MLP96_RESIDENT"),
                                 ("mlp192", False, 0, "MLP384_R3"), ("mlp384d", True, 0, "MLP96_STAGED"), ("mlp96", False, 0, "QA10_WAVE")):
        c = B.MlpCase(kern, proj, 40, mod=mod, out_mode=2, seed=1)
        o = B.make_mlp(c)
        init = B.mlp_buffers(o)
        x, xo = _from_bits(init["x"]), _from_bits(init["xn_out"])
        dev = {k: _bf16(o[k]) for k in ("in", "W1", "W2") + (("Wp",) if proj else ())}
        f32 = {k: o[k].float().cuda() for k in ("b1", "b2") + (("bp",) if proj else ()) + (("mod_aff",) if mod else ())}
        a = L.DsgBxMlpArgs()
        setattr(a, "att" if proj else "xn", dev["in"].data_ptr())
        a.x, a.xn_out, a.W1, a.W2, a.b1, a.b2 = x.data_ptr(), xo.data_ptr(), dev["W1"].data_ptr(), dev["W2"].data_ptr(), f32["b1"].data_ptr(), f32["b2"].data_ptr()
        if proj:
            a.Wp, a.bp = dev["Wp"].data_ptr(), f32["bp"].data_ptr()
        if mod:
            a.mod_aff = f32["mod_aff"].data_ptr()
        a.out_mode, a.mod_T, a.M, a.C, a.kernel = 2, 1, c.M, c.C, getattr(L, "BXK_" + sel)
        assert lib.dsg_debug_mlp_bx_args(C.byref(a), None) == L.DSG_ERR_INVALID, (kern, proj, sel)
        assert np.array_equal(_to_bits(x), init["x"]) and np.array_equal(_to_bits(xo), init["xn_out"]), (kern, proj, sel)
