"""Float64 references, derived error bounds and operand builders for the fp32 hot-path kernels (csrc/kernels.hip), shared by
tests/test_f32_kernels.py (GPU: the kernels against these) and tests/test_f32_kernels_host.py (CPU: the power of these checks).

Every bound below is built from the float64 reference's own quantities and the precision of the formats, never from a kernel's
output.  u = 2^-24 (fp32 unit roundoff).  For C = epi(act(LN?(A) W^T + bias) (+ res)):
  * linear part: (K + 8) u (|A'| |W|^T + |bias|), the standard summation bound, valid for ANY summation order; A' is the normalised
    operand (a - mean) rstd; the 8 pays for the bias add, the store and the operand roundings of the MFMA path;
  * LayerNorm on the way in: the kernel forms a' = a rstd + (-mean rstd) in one FMA from the rounded product mean rstd: two roundings,
    each at most u (|a| + |mean|) rstd, an input perturbation that reaches the output as 2 u ((|A| + |mean|) rstd) |W|^T -- no
    factor K;
  * LayerNorm from partial sums (sum, sumsq per 96 columns, np of them per row): the partials are added in fp32 (np u relative to the
    sum of their magnitudes), mean = sum / K and E[x^2] = sumsq / K cost two roundings each, var = E[x^2] - mean^2 one FMA, so
    d var <= (np + 3) u E[x^2] + 2 |mean| d mean + 2 u mean^2 and d rstd / rstd <= d var / (2 var) -- the condition number
    E[x^2] / var of the one-pass variance -- plus the 1-ulp hardware rsq;
  * activations: the linear bound times the activation's Lipschitz constant (GELU' <= 1.13, SiLU' <= 1.10), plus the approximation
    errors the project pins: GELU 3e-7 absolute (test_gelu_coefficients_in_the_kernel_are_the_fit_scripts), Phi inside GELU' 2.4e-6
    (dgelu_f2's header), hardware exp / rcp / rsq 1 ulp = 1.2e-7 relative (kernels_common.hip.h); exp(-x) is exp2(-x log2 e) and
    the rounding of that product costs |x| u relative;
  * a factor 2 over the sum for the roundings not modelled one by one (residual add, stores, 1 + scale).
Row statistics (sums of 96 stored values, and of their squares) follow the same scheme with K = 96."""
import math
from dataclasses import dataclass

import numpy as np
import torch

from util import FWD_RTOL, window_tokens      # FWD_RTOL: the project's bar on a whole forward; no kernel bar may exceed it

U = 2.0 ** -24
GBM, GBN, GBK = 128, 96, 32
LN_EPS = 1e-5
LOG2E = 1.4426950408889634
ACT_NONE, ACT_GELU, ACT_SILU, ACT_GELU_KEEP, ACT_DGELU = 0, 1, 2, 3, 4
GELU_LIP, SILU_LIP = 1.13, 1.10
GELU_ABS, DPHI_ABS, HW_REL = 3e-7, 2.4e-6, 2.0 ** -23
C_EXTRA = 8          # the c of (K + c) u
C_LN = 2             # roundings of the LayerNorm FMA and of its product mean * rstd


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def dgelu(x):
    phi = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * phi, phi


def silu(x):
    return x * torch.sigmoid(x)


# ------------------------------------------------------------------------------------------------------------------------------
# GEMM forms
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class GemmCase:
    M: int
    N: int
    K: int
    ln: str = "none"      # none | stats (ln_stats [M,2]) | part (ln_part [M][nparts][2])
    act: int = ACT_NONE
    res: bool = False
    K1: int = 0           # > 0: A2 concat, the first source serves k < K1
    c2: bool = False      # dual store
    epi: int = 0          # 0 none, 1 row statistics, 2 batch-uniform modulate + statistics, 3 per-sample modulate + statistics
    mod_T: int = 1
    mod_off: int = 0
    a4_res: int = 0       # > 0: PatchMerging gather from the fine activation [B a4_res^2, K/4]
    B: int = 1
    pad: bool = False     # lda > K, ldc > N, ldres != ldc, ldc2 != ldc
    cnt: int = -1         # >= 0: row list with that many runs (M = 8 * runs of the tensor)
    stale: int = 0        # whole tiles of valid-looking runs behind the padded list (the device-side count stops in front of them)
    seed: int = 0

    @property
    def tiles_n(self):
        return (self.N + GBN - 1) // GBN

    @property
    def nparts(self):     # partials per SOURCE row
        return ((self.K // 4 if self.a4_res else self.K) + 95) // 96

    def ident(self):
        s = f"M{self.M}-N{self.N}-K{self.K}-ln_{self.ln}-act{self.act}-res{int(self.res)}"
        if self.K1: s += f"-K1_{self.K1}"
        if self.c2: s += "-c2"
        if self.epi: s += f"-epi{self.epi}-T{self.mod_T}-off{self.mod_off}"
        if self.a4_res: s += f"-merge{self.a4_res}x{self.B}"
        if self.pad: s += "-pad"
        if self.cnt >= 0: s += f"-cnt{self.cnt}-stale{self.stale}"
        return s


def _partials(X):
    """[R, C] float64 -> [R, ceil(C/96), 2] (sum, sumsq) per 96 columns, rounded to fp32 as a producing kernel stores them"""
    R, Cc = X.shape
    n = (Cc + 95) // 96
    out = torch.zeros(R, n, 2, dtype=torch.float64)
    for t in range(n):
        seg = X[:, 96 * t:96 * (t + 1)]
        out[:, t, 0] = seg.sum(1)
        out[:, t, 1] = (seg * seg).sum(1)
    return out.float()


def make_run_list(n_runs, cnt, stale, gen):
    """ascending runs, -1 up to a multiple of 16 as the contract says, then `stale` tiles of valid runs the count must keep out"""
    perm = torch.randperm(n_runs, generator=gen)
    runs = torch.sort(perm[:cnt]).values.tolist()
    lst = runs + [-1] * ((-len(runs)) % 16)
    if cnt == 0:
        lst = [-1] * 16
    rest = [r for r in range(n_runs) if r not in runs]
    for t in range(stale):
        lst += (rest[16 * t:16 * (t + 1)] + list(range(16)))[:16]
    return runs, lst


def make_gemm(c: GemmCase):
    """fp32 operands of one case on the CPU (seeded), in the physical layouts the kernel reads"""
    gen = torch.Generator().manual_seed(1000 + c.seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    o = {"case": c}
    M, N, K = c.M, c.N, c.K
    if c.a4_res:
        rows, cols = c.B * c.a4_res * c.a4_res, K // 4
        assert M == c.B * (c.a4_res // 2) ** 2
        o["A"] = rn(rows, cols) + 2.0 * (2.0 * torch.rand(rows, 1, generator=gen) - 1.0)
        o["lda"] = cols
    else:
        K1 = c.K1 if c.K1 else K
        o["lda"] = K1 + (12 if (c.pad or c.K1) else 0)
        mean = 2.0 * (2.0 * torch.rand(M, 1, generator=gen) - 1.0) if c.ln != "none" else torch.zeros(M, 1)
        A = torch.full((M, o["lda"]), 7.0)          # padding columns hold a value a wrong stride would pick up
        A[:, :K1] = rn(M, K1) + mean
        o["A"] = A
        if c.K1:
            o["lda2"] = K - K1 + 4
            A2 = torch.full((M, o["lda2"]), -5.0)
            A2[:, :K - K1] = rn(M, K - K1) + mean
            o["A2"] = A2
    o["W"] = rn(N, K) / K ** 0.5
    o["bias"] = rn(N) * 0.3
    Al = logical_A(o).double()
    if c.ln == "stats":
        mu, var = Al.mean(1), Al.var(1, unbiased=False)
        o["ln_stats"] = torch.stack([mu, (var + LN_EPS) ** -0.5], 1).float()
    elif c.ln == "part":
        o["ln_part"] = _partials(o["A"].double()) if c.a4_res else _partials(Al)   # AMODE 1: per FINE row, over its K/4 channels
    o["ldc"] = N + (5 if c.pad else 0)
    o["ldc2"] = N + (9 if c.pad else 0)
    o["ldres"] = N + (3 if c.pad else 0)
    if c.res:
        R = torch.full((M, o["ldres"]), 3.0)
        R[:, :N] = rn(M, N)
        o["res"] = R
    if c.epi >= 2:
        nb = (M + c.mod_T - 1) // c.mod_T if c.epi == 3 else 1
        o["mod_ld"] = (c.mod_off + 2 * N + 5) if c.epi == 3 else 0
        o["mod_aff"] = rn(nb, c.mod_off + 2 * N + 5) * 0.5
    if c.cnt >= 0:
        assert M % 8 == 0
        o["runs"], o["row_list"] = make_run_list(M // 8, c.cnt, c.stale, gen)
    return o


def logical_A(o):
    """the [M, K] operand the product sees: concat along K, or the PatchMerging gather (x00 | x10 | x01 | x11)"""
    c = o["case"]
    if c.a4_res:
        r = c.a4_res
        x = o["A"].view(c.B, r, r, c.K // 4)
        parts = [x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]]
        return torch.cat(parts, -1).reshape(c.M, c.K)
    K1 = c.K1 if c.K1 else c.K
    A = o["A"][:, :K1]
    return torch.cat([A, o["A2"][:, :c.K - K1]], 1) if c.K1 else A


def logical_partials(o, drop=None):
    """[M, np, 2]: the partial sums that make up one logical row's statistics (AMODE 1: its four fine rows')"""
    c, P = o["case"], o["ln_part"]
    if c.a4_res:
        r, n = c.a4_res, P.shape[1]
        x = P.reshape(c.B, r, r, n, 2)
        P = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], 3).reshape(c.M, 4 * n, 2)
    if drop is not None:
        P = torch.cat([P[:, :drop], P[:, drop + 1:]], 1)
    return P


def _ln_terms(o, dt, drop=None):
    """mean, rstd and (float64 only) the bounds on rstd's relative and mean's absolute error"""
    c = o["case"]
    if c.ln == "stats":
        st = o["ln_stats"].to(dt)
        z = torch.zeros_like(st[:, 0])
        return st[:, 0], st[:, 1], z, z
    P = logical_partials(o, drop).to(dt)
    n = P.shape[1]
    sm, sq, sabs = P[..., 0].sum(1), P[..., 1].sum(1), P[..., 0].abs().sum(1)
    mean, msq = sm / c.K, sq / c.K
    var = (msq - mean * mean).clamp(min=0)
    rstd = (var + LN_EPS) ** -0.5
    dmean = (n + 2) * U * sabs / c.K
    dvar = (n + 3) * U * msq + 2 * mean.abs() * dmean + 2 * U * mean * mean
    return mean, rstd, 0.5 * dvar / (var + LN_EPS) + HW_REL, dmean


def _mod_rows(o, dt, neighbour_row=None):
    """(1 + scale, shift) per output row, [M or 1, N]"""
    c = o["case"]
    aff = o["mod_aff"].to(dt)
    if c.epi == 2:
        return 1.0 + aff[0:1, c.mod_off:c.mod_off + c.N], aff[0:1, c.mod_off + c.N:c.mod_off + 2 * c.N]
    b = torch.arange(c.M) // c.mod_T
    if neighbour_row is not None:
        b[neighbour_row] = b[neighbour_row] + (1 if b[neighbour_row] + 1 < aff.shape[0] else -1)
    return 1.0 + aff[b, c.mod_off:c.mod_off + c.N], aff[b, c.mod_off + c.N:c.mod_off + 2 * c.N]


MUTATIONS = ("drop_chunk", "swap_rows", "bias_shift", "drop_partial", "neighbour_sample")


def gemm_expect(o, dtype=torch.float64, mutate=None):
    """The operation in `dtype` on the fp32 operands: dict(C, C2 [M,N]; with float64 also the per-element bounds bC, bC2).
    dtype=float32 is a plain torch evaluation (another summation order than the kernel's or float64's); `mutate` builds one of the
    wrong results of MUTATIONS (float64), for the host tests."""
    c, dt = o["case"], dtype
    want_b = dt == torch.float64
    A, W, bias = logical_A(o).to(dt), o["W"].to(dt), o["bias"].to(dt)
    if mutate == "bias_shift":
        bias = torch.roll(bias, 1)
    Wabs = W.abs()
    if c.ln != "none":
        mean, rstd, drstd, dmean = _ln_terms(o, dt, drop=(0 if mutate == "drop_partial" else None))
        An = (A - mean[:, None]) * rstd[:, None]
        Aenv = (A.abs() + mean.abs()[:, None]) * rstd[:, None]
    else:
        An, Aenv = A, None
    Ap = An
    if mutate == "drop_chunk":
        Ap = An.clone()
        j = (c.K // GBK) // 2
        Ap[:, GBK * j:GBK * (j + 1)] = 0
    y = Ap @ W.t() + bias
    E = None
    if want_b:
        lin = An.abs() @ Wabs.t()
        E = (c.K + C_EXTRA) * U * (lin + bias.abs())
        if c.ln != "none":
            E = E + C_LN * U * (Aenv @ Wabs.t()) + drstd[:, None] * lin + (dmean * rstd)[:, None] * Wabs.sum(1)[None, :]
    out = {}
    R = o["res"][:, :c.N].to(dt) if c.res else None
    if c.act == ACT_NONE:
        v, Ev = y, E
    elif c.act in (ACT_GELU, ACT_GELU_KEEP):
        v = gelu(y)
        Ev = GELU_LIP * E + GELU_ABS + U * v.abs() if want_b else None
        if c.act == ACT_GELU_KEEP:
            out["C2"], out["bC2"] = y, (2 * (E + U * y.abs()) if want_b else None)
    elif c.act == ACT_SILU:
        v = silu(y)
        Ev = SILU_LIP * E + (3 * HW_REL + 2 * U * y.abs()) * v.abs() + U * v.abs() if want_b else None
    else:   # ACT_DGELU: the product times GELU'(res), nothing added
        g1, phi = dgelu(R)
        v = y * g1
        if want_b:
            dg = DPHI_ABS + (R * phi).abs() * (3 * HW_REL + 2 * U * R * R) + U * g1.abs()
            Ev = g1.abs() * E + y.abs() * dg + U * v.abs()
    if c.res and c.act != ACT_DGELU:
        v = v + R
        Ev = Ev + U * v.abs() if want_b else None
    if c.c2 and c.act != ACT_GELU_KEEP:
        out["C2"], out["bC2"] = v, (2 * (Ev + U * v.abs()) if want_b else None)
    if c.epi >= 2:
        sc1, sh = _mod_rows(o, dt, neighbour_row=(c.M // 2 if mutate == "neighbour_sample" else None))
        a = v * sc1 + sh
        w = silu(a)
        if want_b:
            Ea = sc1.abs() * Ev + 2 * U * (v.abs() * sc1.abs() + sh.abs())
            Ev = SILU_LIP * Ea + (3 * HW_REL + 2 * U * a.abs()) * w.abs() + U * w.abs()
        v = w
    if mutate == "swap_rows" and c.M > 1:
        v = v.clone()
        v[[0, c.M - 1]] = v[[c.M - 1, 0]]
    out["C"], out["bC"] = v, (2 * Ev if want_b else None)
    return out


def stats_expect(stored, case, ref=None, bound=None, all_96=False):
    """float64 (sum, sumsq) of the STORED fp32 values over each column tile's valid columns: [M][tiles_n][2], and with the
    reference and its bound the bar on each.  all_96: the wrong sums over the tile's whole 96 columns (a host-test mutation)"""
    M, N, tn = case.M, case.N, case.tiles_n
    S = torch.zeros(M, tn, 2, dtype=torch.float64, device=stored.device)
    Bd = torch.zeros_like(S) if ref is not None else None
    for t in range(tn):
        n0, n1 = GBN * t, (GBN * (t + 1) if all_96 else min(GBN * (t + 1), N))
        seg = stored[:, n0:n1].double()
        S[:, t, 0], S[:, t, 1] = seg.sum(1), (seg * seg).sum(1)
        if ref is not None:
            mag = ref[:, n0:min(n1, N)].abs() + bound[:, n0:min(n1, N)]
            Bd[:, t, 0] = 2 * (GBN + C_EXTRA) * U * mag.sum(1)
            Bd[:, t, 1] = 2 * (GBN + C_EXTRA) * U * (mag * mag).sum(1)
    return S, Bd


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over all elements; NaN anywhere counts as infinite"""
    r = (got.double() - ref).abs() / (bound + 1e-300)
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# window attention and the fused block kernels (same formula in float64 and in float32)
# ------------------------------------------------------------------------------------------------------------------------------
def padded(ws):
    return (ws * ws + 31) // 32 * 32


def make_attn_bias(nW, heads, ws, shift, gen):
    """key-major log2(e)-scaled table [nW | 1][heads][Wp][Wp]: random, -1e30 in the padded key slots, and with a shift the mask value
    -100 log2(e) on a random subset of the entries (the same for every head, as the shifted-window mask is)"""
    Wp, Wt, nWt = padded(ws), ws * ws, (nW if shift > 0 else 1)
    b = torch.randn(nWt, heads, Wp, Wp, generator=gen) * 1.5
    if shift > 0:
        b[(torch.rand(nWt, 1, Wp, Wp, generator=gen) < 0.2).expand(-1, heads, -1, -1)] -= 100.0 * LOG2E
    b[:, :, Wt:, :] = -1.0e30
    return b.contiguous()


def attn_formula(qkv, bias, B, res, ws, shift, heads):
    """softmax_keys(q k^T + bias) v per (window, head) in qkv's dtype: qkv [B res^2, 3 * 32 heads] (q pre-scaled, scores in log2
    units), bias [nW | 1][heads][Wp][Wp] key-major -> [B res^2, 32 heads]"""
    T, Wt, nW = res * res, ws * ws, (res // ws) ** 2
    tok = torch.from_numpy(window_tokens(res, ws, shift)).to(qkv.device)              # [nW, Wt]
    xw = qkv.view(B, T, 3, heads, 32)[:, tok]                                         # [B, nW, Wt, 3, heads, 32]
    q, k, v = (xw[..., i, :, :].permute(0, 1, 3, 2, 4) for i in range(3))             # [B, nW, heads, Wt, 32]
    bt = bias[:, :, :Wt, :Wt].to(qkv.dtype)                                           # [nWt, heads, key, query]
    s = torch.einsum("bwhkd,bwhqd->bwhkq", k, q) + (bt[None] if shift > 0 else bt[None].expand(1, nW, -1, -1, -1))
    e = torch.exp2(s - s.max(dim=3, keepdim=True).values)
    o = torch.einsum("bwhkq,bwhkd->bwhqd", e, v) / e.sum(dim=3)[..., None]
    out = torch.zeros(B, T, heads, 32, dtype=qkv.dtype, device=qkv.device)
    out[:, tok] = o.permute(0, 1, 3, 2, 4)
    return out.view(B * T, 32 * heads)


def layer_norm(x, gam=None, bet=None):
    mu = x.mean(1, keepdim=True)
    y = (x - mu) * ((x - mu).pow(2).mean(1, keepdim=True) + LN_EPS) ** -0.5
    return y if gam is None else y * gam + bet


def qkv_attn_formula(x, W, bqkv, mean, rstd, bias, B, res, ws, shift, heads):
    xn = (x - mean[:, None]) * rstd[:, None]
    return attn_formula(xn @ W.t() + bqkv, bias, B, res, ws, shift, heads)


def mlp_formula(x, gam, bet, W1, b1, W2, b2):
    return x + gelu(layer_norm(x, gam, bet) @ W1.t() + b1) @ W2.t() + b2


def attn96_formula(x, scale, shift_v, gam, bet, Wqkv, bqkv, bias, Wproj, bproj, B, res, ws, shift, premod):
    """scale / shift_v [B, 96] per sample; the attention half of a C = 96 block"""
    T = res * res
    xm = x if premod else silu(shift_v.repeat_interleave(T, 0) + x * (1.0 + scale.repeat_interleave(T, 0)))
    o = attn_formula(layer_norm(xm, gam, bet) @ Wqkv.t() + bqkv, bias, B, res, ws, shift, 3)
    return xm + o @ Wproj.t() + bproj


def formula_bar(f64, f32):
    """the bar of a kernel with no closed-form bound: 8 x the error of the float32 torch evaluation of the same formula against the
    float64 one (the margin pays for another summation order and the 1-ulp exp2 / rcp), never above 1e-4 of the output scale.
    Returns (bar, reference error), both absolute."""
    ref_err = float((f32.double() - f64).abs().max())
    return min(8.0 * ref_err, FWD_RTOL * float(f64.abs().max())), ref_err


# fragment-major weight layouts of the register-chained kernels (the index formulas above pack_mlp_weights / pack_attn_weights)
def pack_rows(W):
    """P[nt][s][lane][t] = W[32 nt + (lane & 31)][8 s + 4 (lane >> 5) + t]  (fc1.weight -> W1p, qkv.weight -> Wqp)"""
    W = np.asarray(W)
    N, K = W.shape
    return np.ascontiguousarray(W.reshape(N // 32, 32, K // 8, 2, 4).transpose(0, 2, 3, 1, 4)).reshape(-1)


def pack_cols(W):
    """P[nt][ct][g][lane][t] = W[32 ct + (lane & 31)][32 nt + 8 g + 4 (lane >> 5) + t]  (fc2.weight -> W2p, proj.weight -> Wpp)"""
    W = np.asarray(W)
    Cc, H = W.shape
    return np.ascontiguousarray(W.reshape(Cc // 32, 32, H // 32, 4, 2, 4).transpose(2, 0, 3, 4, 1, 5)).reshape(-1)


# ------------------------------------------------------------------------------------------------------------------------------
# the GEMM-form cases (shared by the GPU tests and the host tests of the bounds)
# ------------------------------------------------------------------------------------------------------------------------------
PLAIN_M = (1, 127, 128, 129, 1025, 2177)      # 1025: nine row tiles, the second group of eight almost empty; 2177: eighteen
PLAIN_N = (1, 31, 33, 96, 97, 200, 288)       # last column tile with one, two or three of its 32-column slabs in use
PLAIN_K = (32, 64, 96, 160)                   # one chunk (prologue and tail only), even and odd chunk counts


def plain_cases():
    """the twelve LN x {none, GELU, SiLU} x res variants; seven shapes each so that every M, N and K value meets every variant;
    LayerNorm variants alternate between ln_stats and ln_part"""
    out, v = [], 0
    for ln in (False, True):
        for act in (ACT_NONE, ACT_GELU, ACT_SILU):
            for res in (False, True):
                for i in range(7):
                    kind = "none" if not ln else ("stats" if (i + v) % 2 == 0 else "part")
                    out.append(GemmCase(PLAIN_M[(i + v) % 6], PLAIN_N[i], PLAIN_K[(i + v) % 4], ln=kind, act=act, res=res, seed=10 * v + i))
                v += 1
    # leading dimensions that differ from the logical widths, and a dual store with its own pitch
    out.append(GemmCase(129, 97, 64, ln="stats", act=ACT_GELU, res=True, c2=True, pad=True, seed=990))
    out.append(GemmCase(300, 200, 96, res=True, c2=True, pad=True, seed=991))
    return out


def concat_cases():
    out = []
    for i, (K1, K) in enumerate(((32, 64), (96, 192), (64, 96))):   # one chunk each; an odd count from the first source; an odd total
        out.append(GemmCase(129, 97, K, K1=K1, res=True, seed=200 + i))
        out.append(GemmCase(130, 200, K, K1=K1, ln="stats", act=ACT_GELU, seed=210 + i))
        out.append(GemmCase(33, 96, K, K1=K1, ln="part", seed=220 + i))
    return out


def ln_part_cases():
    out = []
    for i, n in enumerate((1, 2, 3, 4, 8)):
        out.append(GemmCase((37, 130, 1, 129, 64)[i], (100, 33, 96, 97, 200)[i], 96 * n, ln="part", act=(ACT_NONE, ACT_GELU, ACT_SILU)[i % 3],
                            res=bool(i % 2), seed=300 + i))
    return out


def train_cases():
    out = []
    for i, (M, N, K) in enumerate(((129, 200, 64), (1, 33, 32), (300, 288, 160), (128, 97, 96))):
        out.append(GemmCase(M, N, K, act=ACT_GELU_KEEP, c2=True, seed=400 + i))
        out.append(GemmCase(M, N, K, act=ACT_DGELU, res=True, seed=410 + i))
    return out


def epi_cases():
    """EPI 1/2/3 on the plain A path: M = 300 with 36-row samples (boundaries inside tiles, not dividing 128), mod_off != 0"""
    out, i = [], 0
    for epi in (1, 2, 3):
        for N in (96, 100, 192, 288):
            out.append(GemmCase(300, N, (64, 96, 32, 160)[i % 4], epi=epi, res=bool(i % 2), c2=bool((i // 2) % 2), mod_T=36, mod_off=8 + 4 * (i % 3),
                                seed=500 + i))
            i += 1
    out.append(GemmCase(300, 100, 64, epi=3, res=True, c2=True, mod_T=36, mod_off=12, pad=True, seed=540))
    out.append(GemmCase(300, 192, 64, epi=1, res=False, c2=True, mod_T=36, seed=541))
    return out


def merge_cases():
    """AMODE 1: M = 12, 27, 128, 144 -- an odd coarse side, a tile boundary inside a sample; K = 128 / 384: one / three chunks per
    part; K = 768: two partials per fine row"""
    out, i = [], 0
    geo = ((4, 3), (6, 3), (16, 2), (24, 1))
    for K in (128, 384, 768):
        for a4, B in geo:
            M = B * (a4 // 2) ** 2
            epi = (0, 2, 3)[i % 3]
            out.append(GemmCase(M, (96, 100, 192, 33)[i % 4], K, ln="part", epi=epi, c2=bool(i % 2), a4_res=a4, B=B, mod_T=(a4 // 2) ** 2,
                                mod_off=4 * (i % 3), seed=600 + i))
            i += 1
    out.append(GemmCase(128, 192, 384, ln="part", epi=0, c2=True, a4_res=16, B=2, seed=640))
    out.append(GemmCase(27, 96, 128, ln="part", epi=3, c2=True, a4_res=6, B=3, mod_T=9, mod_off=8, seed=641))
    return out


ROW_COUNTS = (0, 1, 15, 16, 17, 40)


def rowlist_cases():
    """AMODE 3, every form launch_gemm admits, on a tensor of 40 runs; counts below the list length leave stale tiles behind"""
    forms = [dict(ln="stats", act=ACT_GELU), dict(ln="part", act=ACT_GELU)]
    forms += [dict(res=r, epi=e, mod_T=40, mod_off=4) for r in (False, True) for e in (0, 1, 2, 3)]
    forms += [dict(K1=32), dict(K1=64, res=True, epi=1)]
    out = []
    for f, form in enumerate(forms):
        for j, cnt in enumerate(ROW_COUNTS):
            K = 96 if form.get("K1") else (64, 32, 96)[(f + j) % 3]
            out.append(GemmCase(320, (96, 100, 192)[(f + j) % 3], K, cnt=cnt, stale=(1 if cnt in (0, 1, 16) else 0), seed=700 + 10 * f + j, **form))
    return out


def all_gemm_cases():
    return plain_cases() + concat_cases() + ln_part_cases() + train_cases() + epi_cases() + merge_cases() + rowlist_cases()
