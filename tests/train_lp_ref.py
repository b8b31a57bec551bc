"""Float64 references, cases and a NumPy emulation for the bf16 mode of the training products (csrc/train_kernels_lp.hip), shared by
tests/test_train_lp_kernels.py (GPU) and tests/test_train_lp_kernels_host.py (CPU: the power of these bars).

Reference: the float64 product of the operands rounded to bf16 EXACTLY as the kernels round them (lp_ref.bf16_rne: round to nearest,
ties to even).  The rounding is restated, not bounded, so the bar is the fp32-accumulation bound alone: the one train_ref.tgemm_expect
derives for gemm_tn_f32_kernel -- (K + 8) u sum |a'_k b'_k|, valid for any summation order (slice partials, MFMA k-steps, the ordered
reduction and its lanes), doubled -- applied to the ROUNDED operands a', b'.  (A product of two bf16 values has 16 significant bits:
exact in fp32, so nothing but the additions rounds.)  The column sums are taken from the UNROUNDED dy, with train_ref's column-sum
bound.  Nothing here comes from a kernel's output."""
from dataclasses import replace

import numpy as np
import torch

import lp_ref
import train_ref as R
from train_ref import ACT_DGELU, ACT_GELU_KEEP, ACT_NONE, F64, TGemmCase

ROUTE_LP_GEMM, ROUTE_LP_TN = 5, 6
STEP = 16   # k per v_mfma_f32_32x32x16_bf16


def rne(t):
    """fp32 tensor -> the fp32 values of its bf16 rounding (RNE, ties to even), bit for bit what bf16_rne_hi gives"""
    return torch.from_numpy(lp_ref.bf16_rne(t.numpy()).reshape(t.shape).copy())


def lp_rule(rows, c0, c1, any_rows=False):
    return (any_rows or rows >= 512) and c0 % 32 == 0 and c1 % 32 == 0


def expected_route(c, any_rows):
    """(route, S) the bf16 route must take for case c; (0, 0): not taken"""
    if c.ta:
        ok = not c.tb and not c.bias and not c.res and c.act == ACT_NONE and lp_rule(c.K, c.M, c.N, any_rows)
        return (ROUTE_LP_TN, R.tn_slices(c.M, c.N, c.K)[0]) if ok else (0, 0)
    ok = lp_rule(c.M, c.N, c.K, any_rows) and c.lda == c.K and c.ldb == (c.K if c.tb else c.N) and not c.colsum
    if c.act != ACT_NONE:
        ok = ok and c.ldc == c.N and not c.acc
    return (ROUTE_LP_GEMM, 1) if ok else (0, 0)


def make(c):
    """train_ref.make_tgemm's operands; the long-K spikes follow the fp32 TN kernel's slices, which are the bf16 kernel's"""
    return R.make_tgemm(c)


def expect(o, mutate=None):
    """train_ref.tgemm_expect on the bf16-rounded operands (C, bC, C2, bC2); cs / bcs from the unrounded A"""
    c = o["case"]
    o2 = dict(o)
    o2["A"], o2["B"] = rne(o["A"]), rne(o["B"])
    out = R.tgemm_expect(o2, F64, mutate)
    if c.colsum:
        A = R.op_A(o, F64)
        out["cs"], out["bcs"] = A.sum(1), 2 * (c.K + R.C_EXTRA) * R.U * A.abs().sum(1)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
TN_OUT, TN_IN = (32, 96, 288), (32, 96, 384)
TN_SHORT_K = (1, 15, 16, 17, 31, 32, 33)     # one MFMA k-step is 16, one staged chunk 32


def tn_cases():
    """(case, any_rows).  Short K through the hook's waived row threshold; 512 + 1; on a 96 x 96 gradient K = 2049 (4 slices, 1
    reduction lane), 8705 (17 slices, the last of ONE row, 4 lanes), 9217 (18 slices by the rule, 17 after the slice length is rounded to
    544) and 32768 (64 slices, 16 lanes); every out and in extent; pitches above the extents; accumulate; column sums"""
    out, i = [], 0
    for j, K in enumerate(TN_SHORT_K):
        out.append((TGemmCase(True, False, TN_OUT[j % 3], TN_IN[(j + 1) % 3], K, pa=(0, 5)[j % 2], pb=(3, 0)[j % 2], pc=(0, 7)[j % 2],
                              colsum=True, acc=bool(j % 2), seed=300 + i), True)); i += 1
    out.append((TGemmCase(True, False, 288, 384, 513, pa=2, pb=1, colsum=True, seed=300 + i), False)); i += 1
    out.append((TGemmCase(True, False, 32, 32, 513, pc=3, acc=True, seed=300 + i), False)); i += 1
    for K in (2049, 8705, 9217, 32768):
        out.append((TGemmCase(True, False, 96, 96, K, colsum=True, acc=(K == 8705), seed=300 + i), False)); i += 1
    out.append((TGemmCase(True, False, 288, 32, 2049, pa=4, pb=4, pc=4, colsum=True, seed=300 + i), False)); i += 1
    out.append((TGemmCase(True, False, 32, 384, 8705, colsum=False, seed=300 + i), False)); i += 1
    return out


ACT_M = (512, 513, 2307)


def act_cases():
    """y = x W^T and dx = dy W at 512, 513 and 2307 rows (one, one-and-a-bit and 18.02 tiles of 128), each with res, with accumulate,
    with ACT_GELU_KEEP and with ACT_DGELU"""
    out, i = [], 0
    for tb in (True, False):
        for m, M in enumerate(ACT_M):
            N, K = ((96, 32), (32, 96), (384, 96))[m] if tb else ((32, 96), (96, 384), (96, 96))[m]
            for kw in (dict(res=True), dict(acc=True), dict(act=ACT_GELU_KEEP), dict(act=ACT_DGELU)):
                out.append((TGemmCase(False, tb, M, N, K, bias=tb, pc=0 if "act" in kw else (0, 4)[i % 2], seed=400 + i, **kw), False)); i += 1
    return out


def refused_cases():
    """shapes the bf16 route does not take: 511 rows, a channel extent that is no multiple of 32, a pitch on x, a pitch on the weight, an
    activation form with accumulate, a weight gradient with 511 tokens / out = 48 / a bias"""
    return [TGemmCase(False, True, 511, 96, 96, bias=True, seed=500), TGemmCase(False, True, 512, 48, 96, seed=501),
            TGemmCase(False, True, 512, 96, 48, seed=502), TGemmCase(False, True, 512, 96, 96, pa=4, seed=503),
            TGemmCase(False, False, 512, 96, 96, pb=4, seed=504), TGemmCase(False, False, 512, 96, 96, act=ACT_DGELU, acc=True, seed=505),
            TGemmCase(True, False, 96, 96, 511, colsum=True, seed=506), TGemmCase(True, False, 48, 96, 513, seed=507),
            TGemmCase(True, False, 96, 96, 513, bias=True, seed=508)]


def cast_inputs(R_, Cc, seed):
    """fp32 [R, Cc] with exact ties between two bf16 values (even and odd neighbours), values next to them, zeros and denormals mixed in"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(R_, Cc, generator=gen)
    bits = x.numpy().view(np.uint32).copy().reshape(-1)
    n = bits.size
    idx = np.arange(n)
    bits[idx % 5 == 0] = (bits[idx % 5 == 0] & 0xFFFF0000) | 0x8000          # exact ties
    bits[idx % 5 == 1] = (bits[idx % 5 == 1] & 0xFFFF0000) | 0x7FFF          # just below
    bits[idx % 5 == 2] = (bits[idx % 5 == 2] & 0xFFFF0000) | 0x8001          # just above
    bits[idx % 37 == 3] = 0
    bits[idx % 41 == 4] = 0x00012345                                         # a denormal
    return torch.from_numpy(bits.view(np.float32).reshape(R_, Cc).copy())


# ------------------------------------------------------------------------------------------------------------------------------
# NumPy emulation of gemm_tn_bf16_kernel + t_splitk_reduce (float32 arithmetic op by op)
# ------------------------------------------------------------------------------------------------------------------------------
MISTAKES = ("trunc", "drop_partial_step", "slice_overlap", "pair_swap_a", "colsum_rounded")


def emulate_tn(o, mistake=None):
    """dict(C [M, N], cs [M]) float32: operands rounded to bf16, products added in fp32 in k-steps of 16 (each step's 16 products summed
    in k order, then added to the slice's accumulator), slices of tn_slices, partials added per reduction lane in slice order and the
    lanes in order, then the prior C when accumulating.  `mistake`: one of MISTAKES"""
    c = o["case"]
    A32, B32 = R.op_A(o, torch.float32).numpy(), R.op_B(o, torch.float32).numpy()   # [M, K], [K, N]
    rnd = (lambda x: lp_ref.widen(lp_ref.bf16_trunc_bits(x)).reshape(x.shape)) if mistake == "trunc" else (lambda x: lp_ref.bf16_rne(x).reshape(x.shape))
    Ar, Br = rnd(A32), rnd(B32)
    if mistake == "pair_swap_a":   # the two k of every packed pair exchanged in A only
        Kp = c.K // 2 * 2
        Ar = Ar.copy(); Ar[:, 0:Kp:2], Ar[:, 1:Kp:2] = Ar[:, 1:Kp:2].copy(), Ar[:, 0:Kp:2].copy()
    S, kslice, _ = R.tn_slices(c.M, c.N, c.K)
    parts, cs_parts = [], []
    for z in range(S):
        kb, ke = z * kslice, min(c.K, (z + 1) * kslice)
        if mistake == "slice_overlap" and z > 0:
            kb -= 1
        if mistake == "drop_partial_step" and ke == c.K and (ke - kb) % STEP:
            ke -= (ke - kb) % STEP
        acc = np.zeros((c.M, c.N), np.float32)
        for k0 in range(kb, ke, STEP):
            step = np.zeros((c.M, c.N), np.float32)
            for k in range(k0, min(k0 + STEP, ke)):
                step = (step + np.outer(Ar[:, k], Br[k]).astype(np.float32)).astype(np.float32)
            acc = (acc + step).astype(np.float32)
        parts.append(acc)
        src = Ar if mistake == "colsum_rounded" else A32
        cs = np.zeros(c.M, np.float32)
        for k in range(kb, ke):
            cs = (cs + src[:, k]).astype(np.float32)
        cs_parts.append(cs)

    def reduce(ps, shape):
        zl = R.reducer_lanes(c.M, c.N, S)
        lanes = []
        for q in range(zl):
            v = np.zeros(shape, np.float32)
            for z in range(q, S, zl):
                v = (v + ps[z]).astype(np.float32)
            lanes.append(v)
        t = np.zeros(shape, np.float32)
        for v in lanes:
            t = (t + v).astype(np.float32)
        return t
    C = reduce(parts, (c.M, c.N))
    if c.acc:
        C = (o["C0"][:, :c.N].numpy() + C).astype(np.float32)
    return {"C": torch.from_numpy(C), "cs": torch.from_numpy(reduce(cs_parts, (c.M,)))}


def with_case(o, **kw):
    o2 = dict(o)
    o2["case"] = replace(o["case"], **kw)
    return o2
