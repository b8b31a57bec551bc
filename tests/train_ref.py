"""Float64 references, bars and operand builders for the training kernels (csrc/train_kernels.hip), shared by
tests/test_train_kernels.py (GPU: the kernels against these, through the dsg_debug_t_* hooks) and tests/test_train_kernels_host.py
(CPU: the power of these checks).  Nothing below is taken from a kernel's output.

Products and column sums get a derived per-element bound, as in tests/f32_ref.py: (K + 8) u (|op(A)| |op(B)| + |bias|), valid for ANY
summation order (so it covers split-K and the order of the reduction lanes), carried through res / accumulate / GELU / GELU' exactly
as f32_ref.gemm_expect does, and doubled; column sums (K + 8) u sum |a|, doubled.  That bound grows with K^2: at K = 32768 it is
0.4 % of sum |a b|, more than one lost row or one lost 32-row chunk of evenly sized operands moves a result.  So the long-K operands
carry SPIKES: the k rows where a slicing mistake loses or doubles data -- the last row, the first row of the last slice, the last row
of the first slice and the row after it -- are K / 16 times larger than the rest (spike_rows), and each of them alone is worth tens of
bounds.  Attention, LayerNorm, modulate, Adam and EMA get f32_ref.formula_bar: 8 x the error of a float32 torch evaluation of the same
closed formula on the same operands, at most 1e-4 of the output scale.

The slice arithmetic (tn_slices, plain_slices, reducer_lanes, ...) is transcribed from the launchers ONLY to choose inputs; the GPU
tests cross-check it against the slice count the hook reports."""
import math
from dataclasses import dataclass

import torch

from f32_ref import (ACT_DGELU, ACT_GELU_KEEP, ACT_NONE, C_EXTRA, DPHI_ABS, GELU_ABS, GELU_LIP, HW_REL, LN_EPS, U, dgelu, formula_bar,  # noqa: F401
                     gelu, window_tokens, worst_ratio)

F64, F32 = torch.float64, torch.float32
ROUTE_MFMA, ROUTE_TN, ROUTE_PLAIN, ROUTE_PLAIN_SPLITK = 1, 2, 3, 4


# ------------------------------------------------------------------------------------------------------------------------------
# slice / chunk arithmetic of the launchers (input choice only)
# ------------------------------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return (a + b - 1) // b


def tn_slices(M, N, K):
    """gemm_tn_f32_kernel's split of K: (S, kslice, rows of the last slice)"""
    tiles = _cdiv(M, 128) * _cdiv(N, 96)
    S = max(1, min(256, 1024 // tiles))
    S = max(1, min(S, K // 512))
    kslice = _cdiv(_cdiv(K, S), 32) * 32
    S = _cdiv(K, kslice)
    return S, kslice, K - (S - 1) * kslice


def plain_slices(M, N, K, bias=False):
    """the plain kernel's split-K (K >= 4096, no bias, fewer than 1024 output tiles): (S, kslice, rows of the last slice)"""
    if K < 4096 or bias or _cdiv(M, 32) * _cdiv(N, 32) >= 1024:
        return 1, 0, K
    S = min(64, K // 1024)
    kslice = _cdiv(_cdiv(K, S), 32) * 32
    S = _cdiv(K, kslice)
    return S, kslice, K - (S - 1) * kslice


def reducer_lanes(M, N, S):
    """slice lanes per output of the split-K reduction: 16, 4 or 1"""
    mn = M * N
    return 16 if (S >= 64 and mn < (1 << 17)) else (4 if (S >= 16 and mn < (1 << 19)) else 1)


def modulate_chunks(T):
    rows_per = max(64, _cdiv(T, 64))
    ch = _cdiv(T, rows_per)
    return ch, rows_per, T - (ch - 1) * rows_per


def ln_bwd_blocks(M):
    blocks = max(1, min(1024, _cdiv(M, 4)))
    rows_per = _cdiv(_cdiv(M, blocks), 4) * 4
    blocks = _cdiv(M, rows_per)
    return blocks, rows_per, M - (blocks - 1) * rows_per


def ln_form(C):
    """(LPR, KV) of the LayerNorm kernels"""
    return (32, 1) if C <= 128 else (64, 1) if C <= 256 else (64, 2) if C <= 512 else (64, 3) if C <= 768 else (64, 6)


def expected_route(c):
    """(route, S) t_gemm must take for case c -- what the case was written for"""
    Kp_ok = c.K % 32 == 0 or (c.tb and c.lda % 4 == 0 and not c.res and not c.acc)
    if not c.force_plain and not c.ta and c.M >= 512 and c.N % 32 == 0 and c.lda == c.K and Kp_ok and (c.K % 32 != 0 or not c.tb or c.ldb == c.K):
        return ROUTE_MFMA, 1
    if not c.force_plain and c.ta and not c.tb and not c.bias and c.K >= 2048:
        return ROUTE_TN, tn_slices(c.M, c.N, c.K)[0]
    S = plain_slices(c.M, c.N, c.K, c.bias)[0]
    return (ROUTE_PLAIN_SPLITK if S > 1 else ROUTE_PLAIN), S


# ------------------------------------------------------------------------------------------------------------------------------
# products
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class TGemmCase:
    ta: bool
    tb: bool
    M: int
    N: int
    K: int
    pa: int = 0            # lda = logical width + pa, likewise ldb, ldc
    pb: int = 0
    pc: int = 0
    bias: bool = False
    acc: bool = False
    res: bool = False
    act: int = ACT_NONE
    colsum: bool = False
    force_plain: bool = False
    seed: int = 0

    @property
    def lda(self):
        return (self.M if self.ta else self.K) + self.pa

    @property
    def ldb(self):
        return (self.K if self.tb else self.N) + self.pb

    @property
    def ldc(self):
        return self.N + self.pc

    def ident(self):
        s = f"{'T' if self.ta else 'N'}{'T' if self.tb else 'N'}-M{self.M}-N{self.N}-K{self.K}"
        if self.pa or self.pb or self.pc: s += f"-pad{self.pa}.{self.pb}.{self.pc}"
        for f, n in ((self.bias, "bias"), (self.acc, "acc"), (self.res, "res"), (self.colsum, "cs"), (self.force_plain, "plain")):
            if f: s += "-" + n
        if self.act: s += f"-act{self.act}"
        return s


def _kslice(c):
    route, S = expected_route(c)
    return (tn_slices(c.M, c.N, c.K) if route == ROUTE_TN else plain_slices(c.M, c.N, c.K, c.bias))[1] or c.K, S


def spike_rows(c):
    """k rows that carry the large values (see the module docstring); none where K is short enough for the bound to see a single row"""
    if c.K < 1024:
        return []
    ks, S = _kslice(c)
    return sorted({c.K - 1, (S - 1) * ks, min(ks, c.K) - 1, min(ks, c.K - 1)})


def make_tgemm(c: TGemmCase):
    """fp32 operands in the physical layouts t_gemm reads; padding columns hold 7 (a wrong stride would pick them up)"""
    gen = torch.Generator().manual_seed(5000 + c.seed)
    opA = torch.randn(c.M, c.K, generator=gen)
    opB = torch.randn(c.K, c.N, generator=gen) / max(c.K, 1) ** 0.5
    for k in spike_rows(c):
        opA[:, k] *= c.K / 16.0
    o = {"case": c}
    A = torch.full((c.K if c.ta else c.M, c.lda), 7.0)
    A[:, :(c.M if c.ta else c.K)] = opA.t() if c.ta else opA
    B = torch.full((c.N if c.tb else c.K, c.ldb), 7.0)
    B[:, :(c.K if c.tb else c.N)] = opB.t() if c.tb else opB
    o["A"], o["B"] = A.contiguous(), B.contiguous()
    o["bias"] = torch.randn(c.N, generator=gen) * 0.3 if c.bias else None
    o["C0"] = torch.randn(c.M, c.ldc, generator=gen) if c.acc else None               # the non-zero C an accumulating call adds to
    o["res"] = torch.randn(c.M, c.ldc, generator=gen) if (c.res or c.act == ACT_DGELU) else None
    return o


def op_A(o, dt=F64):
    c = o["case"]
    return (o["A"][:, :c.M].t() if c.ta else o["A"][:, :c.K]).to(dt)


def op_B(o, dt=F64):
    c = o["case"]
    return (o["B"][:, :c.K].t() if c.tb else o["B"][:, :c.N]).to(dt)


TG_MUTATIONS = ("drop_last_row", "drop_chunk", "swap_rows", "colsum_shift")


def tgemm_expect(o, dtype=F64, mutate=None):
    """dict(C [M,N], C2, cs [M]) in `dtype`, with float64 also the bounds bC, bC2, bcs.  float32: a plain torch evaluation (another
    summation order than any kernel's); `mutate`: one of the wrong results of TG_MUTATIONS (float64), for the host tests"""
    c, dt = o["case"], dtype
    want_b = dt == F64
    A, B = op_A(o, dt), op_B(o, dt)
    bias = o["bias"].to(dt) if c.bias else torch.zeros(c.N, dtype=dt)
    Ap = A
    if mutate == "drop_last_row":
        Ap = A.clone(); Ap[:, c.K - 1] = 0
    elif mutate == "drop_chunk":          # the last 32-row chunk of the first slice (one chunk of K where there are no slices)
        k1 = min(_kslice(c)[0], c.K) if c.K >= 1024 else min(c.K, 32 * max(1, (c.K // 32 + 1) // 2))
        Ap = A.clone(); Ap[:, max(0, k1 - 32):k1] = 0
    y = Ap @ B + bias
    E = (c.K + C_EXTRA) * U * (A.abs() @ B.abs() + bias.abs()) if want_b else None
    out = {}
    R = o["res"][:, :c.N].to(dt) if o["res"] is not None else None
    if c.act == ACT_NONE:
        v, Ev = y, E
    elif c.act == ACT_GELU_KEEP:
        v = gelu(y)
        Ev = GELU_LIP * E + GELU_ABS + U * v.abs() if want_b else None
        out["C2"], out["bC2"] = y, (2 * (E + U * y.abs()) if want_b else None)
    else:   # ACT_DGELU: the product times GELU'(res), nothing added
        g1, phi = dgelu(R)
        v = y * g1
        if want_b:
            dg = DPHI_ABS + (R * phi).abs() * (3 * HW_REL + 2 * U * R * R) + U * g1.abs()
            Ev = g1.abs() * E + y.abs() * dg + U * v.abs()
    if c.res and c.act == ACT_NONE:
        v = v + R
        Ev = Ev + U * v.abs() if want_b else None
    if c.acc:
        v = v + o["C0"][:, :c.N].to(dt)
        Ev = Ev + U * v.abs() if want_b else None
    if mutate == "swap_rows" and c.M > 1:
        v = v.clone(); v[[0, c.M - 1]] = v[[c.M - 1, 0]]
    out["C"], out["bC"] = v, (2 * Ev if want_b else None)
    if c.colsum:
        cs = A.sum(1)
        if mutate == "colsum_shift":
            cs = torch.roll(cs, 1)
        out["cs"], out["bcs"] = cs, (2 * (c.K + C_EXTRA) * U * A.abs().sum(1) if want_b else None)
    return out


def colsum_expect(X, dtype=F64):
    """(sums [N], bound) of X [M, N]"""
    s = X.to(dtype).sum(0)
    return s, 2 * (X.shape[0] + C_EXTRA) * U * X.double().abs().sum(0)


# the K list of gemm_tn_f32_kernel on a 96 x 96 output: K -> (S, rows of the last slice)
TN_K_TABLE = {2048: (4, 512), 2049: (4, 417), 8193: (16, 33), 8705: (17, 1), 8735: (17, 31), 8736: (17, 32), 9217: (17, 513), 32768: (64, 512)}
PLAIN_K_TABLE = {4096: (4, 1024), 32769: (32, 33), 33793: (33, 1), 34817: (33, 1025)}      # on a 33 x 33 output
TN_M = (1, 3, 6, 96, 127, 128, 129, 130)
TN_N = (1, 6, 31, 33, 95, 96, 97, 100, 200)


def tn_cases():
    """route 2.  Every K of the table at (96, 96) and (130, 200); every M and every N at K = 2049 and K = 8705; pitches equal to the
    (odd) widths and larger ones; accumulate; column sums at M that are no multiple of the reducer's 16 / 64 / 256 outputs per block"""
    out, i = [], 0
    for K in TN_K_TABLE:
        out.append(TGemmCase(True, False, 96, 96, K, colsum=bool(i % 2), acc=bool((i // 2) % 2), seed=i)); i += 1
        out.append(TGemmCase(True, False, 130, 200, K, pa=(0, 3)[i % 2], pb=(5, 0)[i % 2], pc=(0, 7)[i % 2], colsum=not bool(i % 2), seed=i)); i += 1
    for K in (2049, 8705):
        for j, M in enumerate(TN_M):
            out.append(TGemmCase(True, False, M, TN_N[(j + (K & 1) + K // 4096) % 9], K, colsum=True, acc=bool(j % 2), pc=(0, 5)[j % 2], seed=i)); i += 1
        for j, N in enumerate(TN_N):
            out.append(TGemmCase(True, False, TN_M[(j + 3) % 8], N, K, pa=(0, 0, 2)[j % 3], pb=(0, 3, 0)[j % 3], colsum=bool(j % 2), seed=i)); i += 1
    out.append(TGemmCase(True, False, 6, 96, 2049, colsum=True, seed=i)); i += 1        # the adjacency head: M = 6, lda = 6
    out.append(TGemmCase(True, False, 6, 6, 8705, colsum=True, acc=True, seed=i)); i += 1
    out.append(TGemmCase(True, False, 6, 100, 32768, colsum=True, seed=i)); i += 1      # 16 reduction lanes, 6 column sums
    return out


def mfma_cases():
    """route 1 (the sampling GEMM) and, just outside its thresholds, the same operands on route 3.  The K = 4 / 36 / 60 operands are
    tensors of exactly M x K floats with M = 640 / 512 / 512: a whole number of the allocator's 512-byte blocks, so the last row ends
    where the allocation ends and the chunk overhang behind it is the buffer descriptor's to stop"""
    out, i = [], 100
    for K in (32, 96, 160):
        out.append(TGemmCase(False, True, (512, 513, 640)[i % 3], (96, 32, 384)[i % 3], K, bias=True, res=bool(i % 2), seed=i)); i += 1
    for K in (4, 36, 60):                                    # the zero-padded weight image with the row overhang
        out.append(TGemmCase(False, True, (512, 640, 512)[i % 3], (96, 32, 96)[i % 3], K, bias=True, pb=(0, 4, 0)[i % 3], seed=i)); i += 1
    for K, N in ((32, 96), (96, 384), (384, 32), (96, 96)):  # the transposed weight
        out.append(TGemmCase(False, False, (513, 512, 640, 512)[i % 4], N, K, pb=(0, 5)[i % 2], acc=bool(i % 2), seed=i)); i += 1
    out.append(TGemmCase(False, True, 513, 96, 96, bias=True, act=ACT_GELU_KEEP, seed=i)); i += 1
    out.append(TGemmCase(False, False, 640, 96, 384, act=ACT_DGELU, seed=i)); i += 1
    out.append(TGemmCase(False, True, 512, 384, 96, bias=True, res=True, pc=4, seed=i)); i += 1
    out.append(TGemmCase(False, True, 512, 96, 160, bias=True, acc=True, seed=i)); i += 1
    # just outside: M = 511, N = 48, lda != K
    out.append(TGemmCase(False, True, 511, 96, 96, bias=True, res=True, seed=i)); i += 1
    out.append(TGemmCase(False, True, 512, 48, 96, bias=True, seed=i)); i += 1
    out.append(TGemmCase(False, True, 512, 96, 96, bias=True, pa=4, seed=i)); i += 1
    out.append(TGemmCase(False, True, 511, 96, 96, bias=True, act=ACT_GELU_KEEP, seed=i)); i += 1
    out.append(TGemmCase(False, False, 511, 96, 384, act=ACT_DGELU, seed=i)); i += 1
    return out


PLAIN_SIZES = (1, 31, 32, 33, 65)


def plain_cases():
    """routes 3 and 4: every (ta, tb) at the tile edges, with bias / accumulate / res / the activation forms; split-K on 33 x 33.
    (accumulate and res never meet K = 1: there the single rounding of the final add, u |v| of a doubled bound, is all there is, and the
    float32 evaluation's headroom is 2x where the host test asks 4x of every case)"""
    out, i = [], 200
    for ta in (False, True):
        for tb in (False, True):
            for j in range(5):
                M, N, K = PLAIN_SIZES[j], PLAIN_SIZES[(j + 1 + ta) % 5], PLAIN_SIZES[(j + 1 + 3 * tb) % 5]
                out.append(TGemmCase(ta, tb, M, N, K, bias=bool(j % 2), acc=(j == 2), res=(j == 3), pa=(0, 3)[j % 2], pb=(2, 0)[j % 2],
                                     pc=(0, 6)[(j // 2) % 2], colsum=(ta and not tb and j % 2 == 0), seed=i)); i += 1
            out.append(TGemmCase(ta, tb, 65, 65, 65, bias=True, seed=i)); i += 1
    out.append(TGemmCase(False, True, 33, 65, 31, bias=True, act=ACT_GELU_KEEP, seed=i)); i += 1
    out.append(TGemmCase(False, False, 65, 33, 32, act=ACT_DGELU, seed=i)); i += 1
    for j, K in enumerate(PLAIN_K_TABLE):
        out.append(TGemmCase(bool(j % 2), bool(j // 2 % 2), 33, 33, K, acc=bool(j % 2), pc=(0, 3)[j % 2], force_plain=True, seed=i)); i += 1
        out.append(TGemmCase(True, False, 33, 33, K, colsum=True, force_plain=True, seed=i)); i += 1
    # the weight-gradient form with the matrix-pipe route switched off: the same operands as a route-2 case
    out.append(TGemmCase(True, False, 96, 96, 2049, colsum=True, force_plain=True, seed=i)); i += 1
    return out


def all_tgemm_cases():
    return tn_cases() + mfma_cases() + plain_cases()


# ------------------------------------------------------------------------------------------------------------------------------
# window attention of the training block
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class AttnCase:
    ws: int
    shift: int
    heads: int
    res: int
    B: int
    seed: int = 0

    def ident(self):
        return f"ws{self.ws}-shift{self.shift}-h{self.heads}-res{self.res}-B{self.B}"


def swin_tokens(res, ws, shift):
    """[nW, ws^2] token of every window position: roll the grid by -shift, then partition (Swin's forward)"""
    grid = torch.arange(res * res).view(res, res)
    if shift > 0:
        grid = torch.roll(grid, shifts=(-shift, -shift), dims=(0, 1))
    n = res // ws
    return grid.view(n, ws, n, ws).permute(0, 2, 1, 3).reshape(n * n, ws * ws)


def swin_rel_index(ws):
    """[ws^2 (query), ws^2 (key)] index into the (2 ws - 1)^2 table (Swin's relative_position_index)"""
    co = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")).flatten(1)
    rel = (co[:, :, None] - co[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += ws - 1
    rel[:, :, 1] += ws - 1
    rel[:, :, 0] *= 2 * ws - 1
    return rel.sum(-1)


def swin_mask(res, ws, shift):
    """[nW, ws^2, ws^2]: -100 where the regions of the rolled grid differ (Swin's attn_mask), 0 elsewhere"""
    n = res // ws
    if shift == 0:
        return torch.zeros(n * n, ws * ws, ws * ws, dtype=F64)
    img = torch.zeros(res, res)
    cnt = 0
    for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img[hs, wsl] = cnt
            cnt += 1
    win = img.view(n, ws, n, ws).permute(0, 2, 1, 3).reshape(n * n, ws * ws)
    d = win[:, None, :] - win[:, :, None]
    return torch.where(d != 0, torch.tensor(-100.0, dtype=F64), torch.tensor(0.0, dtype=F64))


def make_attn(c: AttnCase):
    gen = torch.Generator().manual_seed(7000 + c.seed)
    T, Cc = c.res * c.res, 32 * c.heads
    return {"case": c, "qkv": torch.randn(c.B * T, 3 * Cc, generator=gen), "table": torch.randn((2 * c.ws - 1) ** 2, c.heads, generator=gen),
            "d_out": torch.randn(c.B * T, Cc, generator=gen), "d_table0": torch.randn((2 * c.ws - 1) ** 2, c.heads, generator=gen)}


def _attn_parts(o, dt, qkv):
    c = o["case"]
    T, nW, Wt = c.res * c.res, (c.res // c.ws) ** 2, c.ws * c.ws
    tok = swin_tokens(c.res, c.ws, c.shift)
    xw = qkv.view(c.B, T, 3, c.heads, 32)[:, tok]                                # [B, nW, Wt, 3, heads, 32]
    q, k, v = (xw[..., i, :, :].permute(0, 1, 3, 2, 4) for i in range(3))        # [B, nW, heads, Wt, 32]
    return tok, q, k, v, swin_rel_index(c.ws), swin_mask(c.res, c.ws, c.shift).to(dt), (T, nW, Wt)


def _unwindow(x, tok, B, T, Cc):
    """[B, nW, heads, Wt, 32] -> [B T, C] at the tokens' own rows"""
    inv = torch.empty(T, dtype=torch.long)
    inv[tok.reshape(-1)] = torch.arange(T)
    return x.permute(0, 1, 3, 2, 4).reshape(B, T, Cc)[:, inv].reshape(B * T, Cc)


def attn_forward(o, dt=F64, qkv=None, table=None):
    """out [B T, C]; qkv / table: tensors to differentiate through (defaults: the case's operands in dt)"""
    c = o["case"]
    qkv = o["qkv"].to(dt) if qkv is None else qkv
    table = o["table"].to(dt) if table is None else table
    tok, q, k, v, idx, mask, (T, nW, Wt) = _attn_parts(o, dt, qkv)
    s = q @ k.transpose(-1, -2) / math.sqrt(32.0) + table[idx].permute(2, 0, 1)[None, None] + mask[None, :, None]
    return _unwindow(torch.softmax(s, -1) @ v, tok, c.B, T, 32 * c.heads)


def attn_autograd(o):
    """float64 autograd: (out, d_qkv, d_table) for the upstream gradient d_out"""
    qkv, table = o["qkv"].double().requires_grad_(True), o["table"].double().requires_grad_(True)
    out = attn_forward(o, F64, qkv, table)
    gq, gt = torch.autograd.grad((out * o["d_out"].double()).sum(), (qkv, table))
    return out.detach(), gq, gt


ATTN_MUTATIONS = ("bwd_no_mask", "dk_no_scale", "dtable_drop_window", "padded_key")


def attn_explicit(o, dt=F64, mutate=None):
    """the forward and the backward as explicit formulas in dt: (out, d_qkv, d_table).  dV = P^T dO; dP = dO V^T; dS = P (dP - rowsum(dP
    P)); dQ = dS K / sqrt(32); dK = dS^T Q / sqrt(32); d_table[index(i, j)][h] = sum over samples and windows of dS[i][j]"""
    c = o["case"]
    Cc, sc = 32 * c.heads, 1.0 / math.sqrt(32.0)
    tok, q, k, v, idx, mask, (T, nW, Wt) = _attn_parts(o, dt, o["qkv"].to(dt))
    table = o["table"].to(dt)
    dO = o["d_out"].to(dt).view(c.B, T, c.heads, 32)[:, tok].permute(0, 1, 3, 2, 4)      # [B, nW, heads, Wt, 32]
    bias = table[idx].permute(2, 0, 1)[None, None]

    def probs(with_mask, extra_key):
        s = q @ k.transpose(-1, -2) * sc + bias + (mask[None, :, None] if with_mask else 0)
        if extra_key:     # one padded key (k = 0, no bias, no mask) takes part in the softmax
            s = torch.cat([s, torch.zeros_like(s[..., :1])], -1)
        return torch.softmax(s, -1)[..., :Wt]
    P = probs(True, mutate == "padded_key")
    out = _unwindow(P @ v, tok, c.B, T, Cc)
    Pb = probs(mutate != "bwd_no_mask", mutate == "padded_key")
    dV = Pb.transpose(-1, -2) @ dO
    dP = dO @ v.transpose(-1, -2)
    dS = Pb * (dP - (dP * Pb).sum(-1, keepdim=True))
    dQ, dK = dS @ k * sc, dS.transpose(-1, -2) @ q * (1.0 if mutate == "dk_no_scale" else sc)
    d_qkv = torch.cat([_unwindow(t, tok, c.B, T, Cc) for t in (dQ, dK, dV)], 1)
    dSw = dS
    if mutate == "dtable_drop_window":
        dSw = dS.clone(); dSw[c.B - 1, nW - 1] = 0
    d_table = torch.zeros_like(table).index_add_(0, idx.reshape(-1), dSw.sum((0, 1)).permute(1, 2, 0).reshape(Wt * Wt, c.heads))
    return out, d_qkv, d_table


def attn_cases():
    """every ws with a shift and without; heads 1 and 3; res = ws, 2 ws, 3 ws (3 ws with a shift: all nine windows of the 3 x 3 grid,
    every region pattern); B 1 and 3"""
    out, i = [], 0
    for ws in (2, 4, 5, 6, 7, 8, 9, 10, 11):
        out.append(AttnCase(ws, 0, (1, 3)[i % 2], ws * (1, 2)[(i // 2) % 2], (3, 1)[i % 2], seed=i)); i += 1
        out.append(AttnCase(ws, ws // 2, (3, 1)[i % 2], 3 * ws, (1, 3)[(i // 3) % 2], seed=i)); i += 1
        if ws in (4, 7, 10, 11):
            out.append(AttnCase(ws, 1, 3, 2 * ws, 1, seed=i)); i += 1
    out.append(AttnCase(4, 2, 1, 4, 3, seed=i))        # a single shifted window: three regions along each axis inside it
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# LayerNorm, modulate
# ------------------------------------------------------------------------------------------------------------------------------
def _sigmoid(u):
    return 1.0 / (1.0 + torch.exp(-u))


def modulate_fwd(x, aff, T):
    """silu(shift_b + x (1 + scale_b)); x [B T, C], aff [B, 2C] = (scale | shift)"""
    Cc = x.shape[1]
    b = torch.arange(x.shape[0]) // T
    u = aff[b, Cc:] + x * (aff[b, :Cc] + 1.0)
    return u * _sigmoid(u)


def modulate_bwd(x, aff, dy, T, neighbour=False):
    """(dx, d_aff [B, 2C]): du = dy silu'(u), dx = du (1 + scale), d_aff = (sum_t du x | sum_t du).  neighbour: the wrong d_aff that
    sums the NEXT sample's rows (a host-test mutation)"""
    Cc, Bn = x.shape[1], x.shape[0] // T
    b = torch.arange(x.shape[0]) // T
    sc1 = aff[b, :Cc] + 1.0
    u = aff[b, Cc:] + x * sc1
    sg = _sigmoid(u)
    du = dy * (sg * (1.0 + u * (1.0 - sg)))
    d3, x3 = du.view(Bn, T, Cc), x.view(Bn, T, Cc)
    if neighbour:
        d3, x3 = torch.roll(d3, -1, 0), torch.roll(x3, -1, 0)
    return du * sc1, torch.cat([(d3 * x3).sum(1), d3.sum(1)], 1)


def ln_fwd(x, gam, bet):
    """(y, stats [M, 2] = (mean, rstd))"""
    mu = x.mean(1, keepdim=True)
    d = x - mu
    rstd = (d * d).mean(1, keepdim=True).add(LN_EPS) ** -0.5
    return d * rstd * gam + bet, torch.cat([mu, rstd], 1)


def stats_bar(f64, f32):
    """the bar on the forward's row statistics: formula_bar, but never below two roundings of the largest value -- one row of four
    channels has ONE mean, the float32 evaluation's error on it is a draw between 0 and u |mean|, and a mean summed in another
    order may differ from it by an ulp"""
    bar, ref_err = formula_bar(f64, f32)
    return max(bar, 2.0 * U * float(f64.abs().max())), ref_err


def ln_bwd(x, gam, stats, dy, dx_in=None, drop_rows=0):
    """(dx, d_gamma, d_beta) from the GIVEN statistics: dx = dx_in + rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma.
    drop_rows: the wrong d_gamma / d_beta without the last `drop_rows` rows (a host-test mutation)"""
    xh = (x - stats[:, 0:1]) * stats[:, 1:2]
    g = dy * gam
    dx = stats[:, 1:2] * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    if dx_in is not None:
        dx = dx + dx_in
    n = x.shape[0] - drop_rows
    return dx, (dy[:n] * xh[:n]).sum(0), dy[:n].sum(0)


def ln_inputs(M, C, seed, aff_T=0):
    """rows with means of up to two standard deviations; aff [ceil(M / T), 2C] with aff_T"""
    gen = torch.Generator().manual_seed(9000 + seed)
    x = torch.randn(M, C, generator=gen) + 2.0 * (2.0 * torch.rand(M, 1, generator=gen) - 1.0)
    o = {"x": x, "gam": 1.0 + 0.3 * torch.randn(C, generator=gen), "bet": 0.3 * torch.randn(C, generator=gen),
         "dy": torch.randn(M, C, generator=gen), "dx_in": torch.randn(M, C, generator=gen)}
    if aff_T:
        o["aff"] = 0.5 * torch.randn((M + aff_T - 1) // aff_T, 2 * C, generator=gen)
    return o


def modulate_inputs(B, T, C, seed):
    """|u| up to 90: the first channel's shift is +-90 (the sigmoid saturates on both sides), the rest are moderate"""
    gen = torch.Generator().manual_seed(9500 + seed)
    x = torch.randn(B * T, C, generator=gen)
    aff = 0.5 * torch.randn(B, 2 * C, generator=gen)
    aff[:, C] = torch.tensor([90.0, -90.0, 45.0])[:B] if B > 1 else 90.0
    if C > 1:
        aff[:, C + 1] = -88.0
    x[:, 0] *= 0.01
    return {"x": x, "aff": aff, "dy": torch.randn(B * T, C, generator=gen)}


LN_C = (4, 96, 100, 128, 132, 192, 256, 260, 384, 512, 516, 768, 772, 1536)
LN_M = (1, 3, 4, 5, 9, 17)


def ln_cases():
    """(M, C): every C with a small M, every small M; M = 4097 and 8193 at one width of each kernel form"""
    out = [(LN_M[i % 6], Cc) for i, Cc in enumerate(LN_C)]
    out += [(M, (96, 260)[i % 2]) for i, M in enumerate(LN_M)]
    out += [(4097, 96), (4097, 132), (4097, 516), (4097, 4), (8193, 100), (8193, 772), (8193, 1536), (4097, 384)]
    return out


MOD_T = (1, 63, 64, 65, 129, 4097)
MOD_C = (4, 60, 64, 65, 96, 130)


def modulate_cases():
    """(B, T, C): every T with two widths, every C; B 1 and 3"""
    return [((1, 3)[(i + j) % 2], T, MOD_C[(i + 3 * j) % 6]) for i, T in enumerate(MOD_T) for j in range(2)]


# ------------------------------------------------------------------------------------------------------------------------------
# Adam with clip_grad_norm_, EMA
# ------------------------------------------------------------------------------------------------------------------------------
def adam_step(p, g, m, v, step, lr, b1, b2, eps, wd, max_norm, dt=F64, bias_correction=True):
    """lists of tensors -> (p, g, m, v, total_norm) after one torch.optim.Adam step behind clip_grad_norm_(max_norm) (max_norm <= 0:
    no clipping), every operation in dt.  The hyper-parameters are the fp32 values the entry point receives."""
    f = lambda a: float(torch.tensor(a, dtype=F32))
    lr, b1, b2, eps, wd, max_norm = f(lr), f(b1), f(b2), f(eps), f(wd), f(max_norm)
    g = [t.to(dt) for t in g]
    total = torch.sqrt(sum((t * t).sum() for t in g))
    coef = torch.clamp(max_norm / (total + f(1e-6)), max=1.0) if max_norm > 0 else torch.tensor(1.0, dtype=dt)
    bc1 = 1.0 - b1 ** step if bias_correction else 1.0
    bc2s = math.sqrt(1.0 - b2 ** step) if bias_correction else 1.0
    P, G, Mo, V = [], [], [], []
    for pt, gt, mt, vt in zip(p, g, m, v):
        pt, mt, vt = pt.to(dt), mt.to(dt), vt.to(dt)
        gt = gt * coef.to(dt)
        G.append(gt)
        gr = gt + wd * pt if wd != 0 else gt
        mi = mt + (gr - mt) * (1.0 - b1)
        vi = vt * b2 + (1.0 - b2) * gr * gr
        P.append(pt - (lr / bc1) * (mi / (torch.sqrt(vi) / bc2s + eps)))
        Mo.append(mi); V.append(vi)
    return P, G, Mo, V, float(total)


def ema_step(ema, p, decay, dt=F64):
    d = float(torch.tensor(decay, dtype=F32))
    return [e.to(dt) + (q.to(dt) - e.to(dt)) * (1.0 - d) for e, q in zip(ema, p)]


ADAM_SIZES = (1, 255, 4095, 4096, 4097, 8193)


def adam_inputs(sizes, seed):
    """parameters ~ N(0, 1), gradients with 1e-3 <= |g| <= 1 (log-uniform magnitude, random sign), zero state"""
    gen = torch.Generator().manual_seed(9900 + seed)
    p = [torch.randn(n, generator=gen) for n in sizes]
    g = [10.0 ** (-3.0 * torch.rand(n, generator=gen)) * (2.0 * (torch.rand(n, generator=gen) < 0.5).float() - 1.0) for n in sizes]
    g = [t.clamp(-1.0, 1.0) for t in g]
    return p, g, [torch.zeros(n) for n in sizes], [torch.zeros(n) for n in sizes]
