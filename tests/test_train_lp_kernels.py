"""GPU: the kernels of the training entries' bf16 mode (csrc/train_kernels_lp.hip) on their own, through dsg_debug_t_gemm_lp and
dsg_debug_t_cast_lp: the weight-gradient kernel gemm_tn_bf16_kernel with its split-K reduction and column sums, the two
activation-side forms on the bf16 GEMM with their weight planes and the training epilogues, and the plane builder.

EVERY output element is compared with the float64 product of the operands rounded to bf16 exactly as the kernels round them
(tests/train_lp_ref.py); the bar is the fp32-accumulation bound of tests/train_ref.py on those rounded operands and nothing else.  The
column sums are held to float64 sums of the UNROUNDED dy.  Output buffers are NaN-filled and carry padding columns and guard rows that
must stay untouched; the operands are followed by NaN rows that must not be read (a NaN read from there reaches a checked output:
every k row beyond the extent multiplies into every output).  Every case asserts the route and slice count it was written for.
Measured figures: profiles/train_lp_kernel_errors.md (each test prints its own)."""
import ctypes as C

import numpy as np
import pytest
import torch

import lp_ref
import train_lp_ref as P
import train_ref as R

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000
GUARD = 2


def _lib():
    from diffusesg_amd import lib as L
    return L, L.load()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev_guarded(t):
    """the operand on the device, followed by GUARD rows of NaN"""
    if t is None:
        return None
    t = t.contiguous()
    tail = torch.full((GUARD,) + tuple(t.shape[1:]), float("nan"))
    return torch.cat([t, tail]).cuda()


def _nan(rows, cols=None):
    return torch.full((rows + GUARD,) if cols is None else (rows + GUARD, cols), float("nan"), device="cuda")


def _untouched(buf):
    return buf.view(torch.int32).cpu() == NAN_BITS


def _region(buf, rows, cols=None):
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
    print(f"TLPGEMM {tag} {what} worst |err| / bound = {r:.3f}")
    assert r <= 1.0, f"{what}: {r:.2f} x the derived bound"


def _bufs(c, o):
    bufs = {k: _dev_guarded(o[k]) for k in ("A", "B")}
    bufs["bias"] = None if o["bias"] is None else o["bias"].cuda()
    bufs["res"] = None if o["res"] is None else o["res"].contiguous().cuda()
    bufs["C"] = _nan(c.M, c.ldc)
    if c.acc:
        bufs["C"][:c.M, :c.N] = o["C0"][:, :c.N].cuda()
    bufs["C2"] = _nan(c.M, c.ldc) if c.act == R.ACT_GELU_KEEP else None
    bufs["cs"] = _nan(c.M) if c.colsum else None
    return bufs


def _call(c, bufs, any_rows):
    _, lib = _lib()
    route = (C.c_int32 * 2)(-1, -1)
    rc = lib.dsg_debug_t_gemm_lp(int(c.ta), int(c.tb), _p(bufs["A"]), c.lda, _p(bufs["B"]), c.ldb, _p(bufs["bias"]), _p(bufs["C"]), c.ldc, c.M,
                                 c.N, c.K, int(c.acc), _p(bufs["cs"]), _p(bufs["res"]), c.act, _p(bufs["C2"]), int(any_rows), route, None)
    return rc, route[0], route[1]


def _run(c, any_rows):
    o = P.make(c)
    ref = P.expect(o)
    bufs = _bufs(c, o)
    rc, route, S = _call(c, bufs, any_rows)
    assert rc == 0, f"dsg_debug_t_gemm_lp refused {c.ident()} (status {rc})"
    want = P.expected_route(c, any_rows)
    assert want[0] != 0 and (route, S) == want, f"{c.ident()}: took route {route} with {S} slices, written for route {want[0]} with {want[1]}"
    tag = f"route{route}-S{S}-{c.ident()}"
    _check_bound(tag, "C", bufs["C"], c.M, c.N, ref["C"], ref["bC"])
    if bufs["C2"] is not None:
        _check_bound(tag, "C2", bufs["C2"], c.M, c.N, ref["C2"], ref["bC2"])
    if c.colsum:
        _check_bound(tag, "colsum", bufs["cs"], c.M, None, ref["cs"], ref["bcs"])


def _ids(cases):
    return [c.ident() for c, _ in cases]


@pytest.mark.parametrize("case,any_rows", P.tn_cases(), ids=_ids(P.tn_cases()))
def test_weight_gradient_kernel(case, any_rows):
    """gemm_tn_bf16_kernel + reducer: 1 ... 33 tokens around the 16-deep MFMA step and the 32-row chunk, 513, a last slice of one row, a
    slice count that drops after rounding, 1 / 4 / 16 reduction lanes, out in {32, 96, 288}, in in {32, 96, 384}, pitches above the
    extents, accumulate onto a non-zero gradient, and the column sums of the unrounded dy"""
    S, _, last = R.tn_slices(case.M, case.N, case.K)
    if case.K == 8705:
        assert (S, last) == (17, 1)
    if case.K == 9217:
        assert S == 17 and min(256, case.K // 512) == 18
    if case.M == 96 and case.N == 96 and case.K in (2049, 8705, 32768):
        assert R.reducer_lanes(96, 96, S) == {2049: 1, 8705: 4, 32768: 16}[case.K]
    _run(case, any_rows)


@pytest.mark.parametrize("case,any_rows", P.act_cases(), ids=_ids(P.act_cases()))
def test_activation_side_forms(case, any_rows):
    """y = x W^T on the plane of W and dx = dy W on the plane of W^T, with res, accumulate, ACT_GELU_KEEP (c2 = the pre-activation) and
    ACT_DGELU, at 512, 513 and 2307 rows"""
    _run(case, any_rows)


@pytest.mark.parametrize("case", P.refused_cases(), ids=[c.ident() for c in P.refused_cases()])
def test_shapes_the_route_does_not_take(case):
    """a status, route 0, and nothing written"""
    L, _ = _lib()
    c = case
    o = P.make(c)
    assert P.expected_route(c, False) == (0, 0)
    bufs = _bufs(c, o)
    if c.acc:
        bufs["C"] = _nan(c.M, c.ldc)
    rc, route, S = _call(c, bufs, False)
    assert rc == L.DSG_ERR_INVALID and route == 0, (c.ident(), rc, route)
    for b in (bufs["C"], bufs["C2"], bufs["cs"]):
        assert b is None or bool(_untouched(b).all()), f"{c.ident()}: a refused call wrote to its outputs"


@pytest.mark.parametrize("R_,Cc", [(1, 1), (33, 65), (96, 96), (288, 384), (384, 31)])
def test_plane_builder_bit_for_bit(R_, Cc):
    """W -> bf16 [R, Cc] and, transposed, [Cc, R]: the bit patterns of round-to-nearest-even, ties included; guard elements untouched"""
    _, lib = _lib()
    w = P.cast_inputs(R_, Cc, 7 * R_ + Cc)
    want = torch.from_numpy(lp_ref.bf16_rne_bits(w.numpy()).reshape(R_, Cc).astype(np.int16))
    dw = _dev_guarded(w)
    n = R_ * Cc
    nk = torch.full((n + 8,), -21846, dtype=torch.int16, device="cuda")    # 0xAAAA
    kn = torch.full((n + 8,), -21846, dtype=torch.int16, device="cuda")
    assert lib.dsg_debug_t_cast_lp(_p(dw), R_, Cc, _p(nk), _p(kn), None) == 0
    assert torch.equal(nk[:n].cpu().view(R_, Cc), want)
    assert torch.equal(kn[:n].cpu().view(Cc, R_), want.t())
    assert bool((nk[n:] == -21846).all()) and bool((kn[n:] == -21846).all())
    only = torch.full((n + 8,), -21846, dtype=torch.int16, device="cuda")
    assert lib.dsg_debug_t_cast_lp(_p(dw), R_, Cc, None, _p(only), None) == 0
    assert torch.equal(only[:n].cpu().view(Cc, R_), want.t())
