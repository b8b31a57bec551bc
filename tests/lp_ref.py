"""Float64 references, derived bars, operand builders and a NumPy emulation for the two bf16-MFMA GEMMs of csrc/kernels_lp.hip
(gemm_bf16_kernel, option "gemm_bf16"; gemm_split2_kernel, option "gemm_split") and its conversion kernels, shared by
tests/test_lp_kernels.py (GPU: the kernels against these) and tests/test_lp_kernels_host.py (CPU: the power of these checks).
Built on tests/f32_ref.py: the operands come from its make_gemm, the float64 evaluation and every activation / residual / modulate /
statistics term of a bar from its gemm_expect and stats_expect.  Nothing below is taken from a kernel's output.  u = 2^-24.

bf16 mode.  The kernel rounds both operands to bf16 (round to nearest even) and multiplies them on v_mfma_f32_32x32x16_bf16: a product
of two 8-bit significands is exact in fp32, only the accumulation rounds.  So the reference is the float64 product of the ROUNDED
operands and the bar is f32_ref's summation bound (K + 8) u (|A'| |W|^T + |bias|) on them, followed by f32_ref's activation, residual
and modulate terms (gemm_expect is called on the rounded operands as a plain product) -- 2^-8 operand rounding never enters the bar.
  * W' = bf16_rne(W).  Without LayerNorm A' = bf16_rne(A); a bf16 A tensor is widened, which is exact.
  * With LayerNorm the kernel forms a' = fma(a, rstd, -mean rstd) in fp32 and rounds that.  The reference does the same: the FMA in
    float64 (the product of two fp32 values is exact there) rounded to fp32, then to bf16.  With ln_stats, mean and rstd are the given
    fp32 numbers and the restatement is exact.  With ln_part they are f32_ref's float64 values rounded to fp32, and the kernel's own
    (fp32 sums of the partials, 1-ulp hardware rsq) differ from them by f32_ref's partial-sum bounds (d rstd / rstd, d mean).
  * An element of A' can therefore round to the OTHER neighbour in the kernel when its float64 value lies within
        pert = C_LN u (|a| + |mean|) rstd + (d rstd / rstd) |a'| + d mean rstd + u |a'|
    of a bf16 rounding boundary (the midpoint of two neighbours; the last term is the fp32 rounding in front of the bf16 one).  Only
    such an element gets an allowance, added to the bar of its row: (spacing(a') + pert) |w_nk|, spacing = the distance of the two
    neighbours, 2^-8 |a'| < spacing <= 2^-7 |a'|.  (Half a spacing, 2^-8 |a'|, is the distance to the boundary; the operand that
    took the other side is a whole spacing away, so that is what the product moves by.)  The allowance passes through the activation
    and the modulate with their Lipschitz constants and is not doubled like the rounding terms: the move is one exact spacing.  Condition, asserted on the host for every case: at most 1 % of a case's A'
    elements are flagged (measured: < 0.1 %).
  * bf16 C tensor: the kernel rounds its own fp32 result, which is within b of the reference v, to nearest: half a spacing at most.
    bar = b + spacing(|v| + b) / 2, between 2^-9 and 2^-8 of (|v| + b) -- bf16 carries 8 significant bits, so its unit roundoff is
    2^-8 (tests/test_bx_kernels.py uses the flat 2^-8 |v|); 2^-9 is reached only at the top of a binade, and an exact restatement of
    round-to-nearest misses a flat 2^-9 (|v| + b) by 1.9 x.
  * Row statistics: f32_ref.stats_expect on the values the kernel stored (K = 96 summation bound).

split mode.  a = hi + mid + lo exactly, three bf16 values cut by truncation: with s = the bf16 spacing at a (<= 2^-7 |a|),
|mid + lo| < s, |lo| < 2^-8 s.  The kernel sums the products hh, hm, mh, hl, lh, mm and drops ml, lm, ll:
    |a_m w_l| + |a_l w_m| + |a_l w_l| < (2^-7 2^-15 + 2^-15 2^-7 + 2^-30) |a| |w| < 8.1 u |a| |w|,
so the reference is the float64 product of the fp32 operands (f32_ref.gemm_expect as it is, LayerNorm terms included) and the bar is
f32_ref's plus DROP u |A'| |W|^T, DROP = 9, times the activation's Lipschitz constant and f32_ref's final factor 2.  The accumulator
takes 6 K / 16 MFMA results instead of K / 2 fp32-MFMA ones; one MFMA adds 16 exact products, and even a rounding after every group
of four would make 1.5 K roundings, under the 2 (K + 8) the fp32 bound pays for.
The table GELU replaces f32_ref's GELU_ABS by what the table's header states and its fp32 evaluation adds, on v = x Phi~(x):
    |x| (3.2e-8 + PHI_MAX (|x| + 6) u + 4 u) + 6e-9
(3.2e-8: second-order Taylor between nodes; t = x + 6 is rounded to fp32 before the node is subtracted, which moves the evaluation
point by (|x| + 6) u at most and Phi by PHI_MAX = 0.3990 times that; the fp32 table entry and the three fused steps of the Horner
form cost 4 u on a value below 1; 6e-9: Phi clamped beyond |x| = 6); the final product's rounding is f32_ref's u |v| term.

Row passes with a bf16 output (window attention, merge_ln, breakup_ln, ln_bx): the fp32 form's bar b (f32_ref.formula_bar or
edge_ref.ln_elem_bound) plus the same half spacing at |ref| + b; a bf16 input is widened, which is exact, so the reference is evaluated on the
rounded input.  ln_bx normalises the row it has just stored, so its reference is the float64 LayerNorm of the STORED fp32 row; the
in-place row itself keeps the fp32 bar, and its plain bf16 copy is bit for bit the restatement's rounding of the stored row.

Conversions: bit-level NumPy restatements of bf16_rne_hi and split3_bits (uint32 / float32 arithmetic, exact), pinned on the host
against torch's bfloat16 cast and against integer arithmetic on the significand."""
import math
from dataclasses import dataclass, replace

import numpy as np
import torch

import f32_ref as R
from f32_ref import ACT_GELU, ACT_NONE, ACT_SILU, GBN, GemmCase, U

DROP = 9.0
PHI_MAX = 0.3990
TAB_TAYLOR, TAB_CLAMP = 3.2e-8, 6e-9
FLAG_CAP = 0.01
HBK, SBK = 64, 32        # k per chunk: the bf16 kernel's 128-row tile (its 256-row tile steps 32), the split kernel


# ------------------------------------------------------------------------------------------------------------------------------
# bit-level restatements (float32 arrays in, uint16 bit patterns / float32 values out)
# ------------------------------------------------------------------------------------------------------------------------------
def _u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _f32(bits):
    return np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32)


def bf16_rne_bits(x):
    """bf16_rne_hi: bits + 0x7fff + (bit 16), upper half (wraps like the 32-bit add it is; NaN is not special-cased)"""
    u = _u32(x).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFFFFFF) >> 16).astype(np.uint16)


def bf16_trunc_bits(x):
    return (_u32(x) >> 16).astype(np.uint16)


def widen(bits16):
    """bf16 bit patterns -> float32 (exact)"""
    return _f32(np.asarray(bits16).astype(np.uint32) << 16)


def bf16_rne(x):
    return widen(bf16_rne_bits(x))


def split3_bits(x):
    """split3_bits: hi = the upper 16 bits, mid = the upper 16 bits of (x - hi), lo = (x - hi) - mid; both differences are exact"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        h = _u32(x) & np.uint32(0xFFFF0000)
        r1 = x - _f32(h)
        m = _u32(r1) & np.uint32(0xFFFF0000)
        lo = _u32(r1 - _f32(m))
    return (h >> 16).astype(np.uint16), (m >> 16).astype(np.uint16), (lo >> 16).astype(np.uint16)


def split3(x):
    return tuple(widen(p) for p in split3_bits(x))


def special_values():
    """float32: ties to even in both directions, +-0, denormals, the largest finite values (round to inf), +-inf, zero mid / lo planes"""
    bits = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,      # ties: down to the even 0x3f80, up to the even 0x3f82, and negative
            0x3F807FFF, 0x3F808001,                              # just under / over a tie
            0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00008000, 0x00018000, 0x007F8000,      # zeros and denormals (with ties)
            0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF,      # the largest finite values: inf from 0x7f7f8000 on
            0x7F800000, 0xFF800000,
            0x3F800000, 0x3F800100, 0x3F800001, 0x3F80FF00, 0x3F8000FF, 0xC1230000, 0xC1230080]      # zero mid and / or lo plane
    return np.array(bits, dtype=np.uint32).view(np.float32)


def random_values(n=1_000_000, seed=7):
    """random bit patterns over the whole finite range (every exponent, denormals included)"""
    u = np.random.RandomState(seed).randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    return u[(u & 0x7F800000) != 0x7F800000].view(np.float32)


def bf16_spacing(x64):
    """distance of the two bf16 neighbours around |x| (float64 array; 0 where x == 0)"""
    _, ex = np.frexp(np.abs(x64))
    return np.where(x64 == 0, 0.0, np.ldexp(1.0, ex - 8))


def boundary_distance(x64):
    """distance of x from the nearest bf16 rounding boundary (a midpoint of two neighbours)"""
    s = bf16_spacing(x64)
    q = np.abs(x64) / np.where(s == 0, 1.0, s)
    return np.where(s == 0, np.inf, np.abs(q - np.floor(q) - 0.5) * s)


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class LpCase:
    g: GemmCase
    mode: int             # 1 bf16, 2 split
    tile: int = 0         # bf16: 0 the launcher's rule, 1 the 128-row tile, 2 the 256-row tile
    a_bf16: bool = False
    c_bf16: bool = False
    tweak: str = ""       # "midheavy": operands with a full mid plane and positive products; "span": pre-activations over [-7, 7]

    def ident(self):
        s = ("bf16" if self.mode == 1 else "split") + (f"-t{self.tile}" if self.tile else "") + "-" + self.g.ident()
        return s + ("-abf" if self.a_bf16 else "") + ("-cbf" if self.c_bf16 else "") + (f"-{self.tweak}" if self.tweak else "")

    @property
    def tile_rows(self):
        return 256 if (self.mode == 2 or self.tile == 2) else 128

    @property
    def kb(self):
        return SBK if (self.mode == 2 or self.tile == 2) else HBK


def make_lp(c: LpCase):
    """f32_ref.make_gemm's operands; a bf16 A tensor holds bf16 values (o["A"] stays their float32 widening)"""
    o = R.make_gemm(c.g)
    if c.a_bf16:
        o["A"] = torch.from_numpy(bf16_rne(o["A"].numpy()))
    if c.tweak == "midheavy":      # bits 15..8 all ones: mid is as large as it gets; every product positive, so that mid.mid sums coherently
        for k in ("A", "W"):
            b = (_u32(o[k].abs().numpy()) & np.uint32(0xFFFF00FF)) | np.uint32(0x0000FF00)
            o[k] = torch.from_numpy(_f32(b).copy())
    if c.tweak == "span":          # column n's pre-activation sits near -7 + 14 n / (N - 1): both clamped ends and the whole table
        o["W"] = o["W"] * 0.05
        o["bias"] = torch.linspace(-7.0, 7.0, c.g.N)
    return o


VARIANTS = [(ln, act, res) for ln in (False, True) for act in (ACT_NONE, ACT_GELU, ACT_SILU) for res in (False, True)]
BF16_N = (1, 32, 96, 100, 192, 288)
BF16_K = (32, 64, 96, 160)
BF16_M = {1: (1, 127, 128, 129, 256, 300, 9 * 128 + 3), 2: (256, 300, 9 * 256 + 3)}


def bf16_plain_cases(tile):
    """LN x {none, GELU, SiLU} x res on one tile: six shapes per variant so that every M, N and K meets every tile, LayerNorm variants
    alternating between ln_stats and ln_part; the last two have lda > K, ldc > N, ldres != ldc and a dual store"""
    out, Ms = [], BF16_M[tile]
    for v, (ln, act, res) in enumerate(VARIANTS):
        for i in range(len(Ms) if tile == 1 else 6):
            kind = "none" if not ln else ("stats" if (i + v) % 2 == 0 else "part")
            g = GemmCase(Ms[(i + v) % len(Ms)], BF16_N[(i + 2 * v) % 6], BF16_K[(i + v) % 4], ln=kind, act=act, res=res, seed=20 * v + i)
            out.append(LpCase(g, 1, tile))
    out.append(LpCase(GemmCase(300, 100, 96, ln="stats", act=ACT_GELU, res=True, c2=True, pad=True, seed=990), 1, tile))
    out.append(LpCase(GemmCase(257, 192, 160, res=True, c2=True, pad=True, seed=991), 1, tile))
    return out


def bf16_ln_part_cases(tile):
    out = []
    for i, n in enumerate((1, 2, 3, 4, 8)):
        g = GemmCase((300, 257, 256, 385, 300)[i], (100, 32, 96, 192, 1)[i], 96 * n, ln="part", act=(ACT_NONE, ACT_GELU, ACT_SILU)[i % 3],
                     res=bool(i % 2), seed=300 + i)
        out.append(LpCase(g, 1, tile))
    return out


def bf16_concat_cases(tile):
    """(K1, K) = (64, 96): the second source starts the half-valid chunk of the 64-deep tile; (64, 160); (128, 224); lda2 != lda"""
    out = []
    for i, (K1, K) in enumerate(((64, 96), (64, 160), (128, 224))):
        out.append(LpCase(GemmCase(300, 100, K, K1=K1, res=True, seed=200 + i), 1, tile))
        out.append(LpCase(GemmCase(257, 192, K, K1=K1, ln="stats", act=ACT_GELU, c2=True, seed=210 + i), 1, tile))
        out.append(LpCase(GemmCase(256, 96, K, K1=K1, ln="part", seed=220 + i), 1, tile))
    return out


def bf16_epi_cases(tile):
    """f32_ref's EPI 1/2/3 cases: M = 300 in 36-row samples -- sample boundaries inside the 128-row tiles, inside the 256-row tile (at
    rows 36 .. 252) and inside the ragged last tile of both (at row 288) --, mod_off != 0, with and without res and C2, one with pad"""
    return [LpCase(g, 1, tile) for g in R.epi_cases()]


def bf16_abf_cases(tile):
    """bf16 A tensor (the launcher admits it with res, no LayerNorm, no activation): EPI 0 .. 3, K = 64 and 128"""
    out = []
    for e in (0, 1, 2, 3):
        for j, K in enumerate((64, 128)):
            g = GemmCase(300, (100, 192)[j], K, res=True, epi=e, mod_T=36, mod_off=(8 if e >= 2 else 0), seed=800 + 2 * e + j)
            out.append(LpCase(g, 1, tile, a_bf16=True))
    return out


def bf16_cbf_cases(tile):
    """bf16 C tensor behind a LayerNorm from statistics and from partials, without activation and with GELU; one with ldc > N"""
    out = []
    for i, (ln, act) in enumerate((("stats", ACT_NONE), ("stats", ACT_GELU), ("part", ACT_NONE), ("part", ACT_GELU))):
        out.append(LpCase(GemmCase((300, 257)[i % 2], (100, 192)[i // 2], (96, 160, 192, 96)[i], ln=ln, act=act, pad=(i == 3), seed=850 + i), 1, tile,
                          c_bf16=True))
    return out


def bf16_cases(tile):
    return (bf16_plain_cases(tile) + bf16_ln_part_cases(tile) + bf16_concat_cases(tile) + bf16_epi_cases(tile) + bf16_abf_cases(tile) +
            bf16_cbf_cases(tile))


def bf16_rule_cases():
    """the launcher's own choice: 128 x 4 = 512 tiles of 256 x 96 at K = 32 -> the wide tile; 3 x 2 tiles -> the narrow one"""
    return [(LpCase(GemmCase(256 * 128, 384, 32, ln="stats", act=ACT_GELU, seed=900), 1, 0), 256),
            (LpCase(GemmCase(600, 100, 96, res=True, seed=901), 1, 0), 128)]


SPLIT_M = (1, 255, 256, 257, 9 * 256 + 3)
SPLIT_N = (1, 96, 100, 192)
SPLIT_K = (32, 64, 96)


def split_cases():
    """all twelve variants (LayerNorm from ln_stats: the kernel has no other), five shapes each; K = 32 is the single chunk whose
    prefetches all clamp; two sources with (K1, K) = (32, 64) and (96, 192); dual store; pitches; GELU rows spanning [-7, 7]"""
    out = []
    for v, (ln, act, res) in enumerate(VARIANTS):
        for i in range(5):
            g = GemmCase(SPLIT_M[(i + v) % 5], SPLIT_N[(i + 2 * v) % 4], SPLIT_K[(i + v) % 3], ln=("stats" if ln else "none"), act=act, res=res,
                         seed=1000 + 20 * v + i)
            out.append(LpCase(g, 2))
    for i, (K1, K) in enumerate(((32, 64), (96, 192))):
        out.append(LpCase(GemmCase(257, 100, K, K1=K1, res=True, seed=1300 + i), 2))
        out.append(LpCase(GemmCase(300, 192, K, K1=K1, ln="stats", act=ACT_GELU, c2=True, seed=1310 + i), 2))
    out.append(LpCase(GemmCase(257, 100, 96, ln="stats", act=ACT_GELU, res=True, c2=True, pad=True, seed=1320), 2))
    out.append(LpCase(GemmCase(300, 192, 64, res=True, c2=True, pad=True, seed=1321), 2))
    out.append(LpCase(GemmCase(257, 192, 64, act=ACT_GELU, seed=1330), 2, tweak="span"))
    out.append(LpCase(GemmCase(300, 100, 96, ln="stats", act=ACT_GELU, c2=True, seed=1331), 2, tweak="span"))
    out.append(LpCase(GemmCase(257, 100, 32, seed=1340), 2, tweak="midheavy"))
    return out


def all_cases():
    return bf16_cases(1) + bf16_cases(2) + split_cases()


# forms launch_gemm_lp refuses (nothing launched, no output written), as changes to one admitted base call: M = 300, N = 100, K = 64,
# plain product.  Values that are buffers are named ("stats_out", "ln_stats", ...) and filled in by the test.
REFUSALS = [
    ("split with stats_out", dict(mode=2, stats_out=True)),
    ("split with ln_part", dict(mode=2, ln_part=True, ln_nparts=1)),
    ("bf16 LN + stats_out", dict(mode=1, ln_stats=True, stats_out=True)),
    ("bf16 act + stats_out", dict(mode=1, act=ACT_GELU, stats_out=True)),
    ("bf16 A2 with K1 % 64 != 0", dict(mode=1, A2=True, K1=32)),
    ("split A2 with K1 % 32 != 0", dict(mode=2, A2=True, K1=16)),
    ("bf16 a4_res", dict(mode=1, a4_res=4)),
    ("split a4_res", dict(mode=2, a4_res=4)),
    ("a_bf16 without res", dict(mode=1, a_bf16=1)),
    ("a_bf16 with LN", dict(mode=1, a_bf16=1, res=True, ln_stats=True)),
    ("a_bf16 with act", dict(mode=1, a_bf16=1, res=True, act=ACT_GELU)),
    ("a_bf16 with A2", dict(mode=1, a_bf16=1, res=True, A2=True, K1=64, K=128)),
    ("a_bf16 with K % 64 != 0", dict(mode=1, a_bf16=1, res=True, K=96)),
    ("a_bf16 with c_bf16", dict(mode=1, a_bf16=1, c_bf16=1, res=True)),
    ("a_bf16 split", dict(mode=2, a_bf16=1, res=True)),
    ("c_bf16 without LN", dict(mode=1, c_bf16=1)),
    ("c_bf16 with SiLU", dict(mode=1, c_bf16=1, ln_stats=True, act=ACT_SILU)),
    ("c_bf16 with res", dict(mode=1, c_bf16=1, ln_stats=True, res=True)),
    ("c_bf16 with C2", dict(mode=1, c_bf16=1, ln_stats=True, C2=True)),
    ("c_bf16 with stats_out", dict(mode=1, c_bf16=1, ln_stats=True, stats_out=True)),
    ("c_bf16 split", dict(mode=2, c_bf16=1, ln_stats=True)),
]


# ------------------------------------------------------------------------------------------------------------------------------
# references and bars
# ------------------------------------------------------------------------------------------------------------------------------
def _act_lip(act):
    return {ACT_NONE: 1.0, ACT_GELU: R.GELU_LIP, ACT_SILU: R.SILU_LIP}[act]


def bf16_operands(o):
    """the rounded operands of the reference and the allowance bookkeeping: A' [M,K] float32 (bf16 values), W' [N,K], flagged [M,K]
    bool, move [M,K] float64 = (spacing + pert) of the flagged elements, 0 elsewhere"""
    g = o["case"]
    A = R.logical_A(o).double().numpy()
    Wr = bf16_rne(o["W"].numpy())
    if g.ln == "none":
        return bf16_rne(A.astype(np.float32)), Wr, np.zeros(A.shape, bool), np.zeros(A.shape)
    mean, rstd, drstd, dmean = (t.numpy() for t in R._ln_terms(o, torch.float64))
    mean32, rstd32 = mean.astype(np.float32), rstd.astype(np.float32)
    nmr32 = (-mean32.astype(np.float64) * rstd32.astype(np.float64)).astype(np.float32)      # the kernel's rounded product
    a64 = A * rstd32.astype(np.float64)[:, None] + nmr32.astype(np.float64)[:, None]          # the FMA, exact up to float64's own rounding
    Ar = bf16_rne(a64.astype(np.float32))
    pert = (R.C_LN * U * (np.abs(A) + np.abs(mean)[:, None]) * rstd[:, None] + drstd[:, None] * np.abs(a64) + (dmean * rstd)[:, None] +
            U * np.abs(a64))
    flagged = boundary_distance(a64) <= pert
    return Ar, Wr, flagged, np.where(flagged, bf16_spacing(a64) + pert, 0.0)


def with_bf16_store(v, b):
    """the bar of a value stored as bf16 (round to nearest) whose fp32 form has the bar b: b + half a spacing at |v| + b"""
    return b + 0.5 * torch.from_numpy(bf16_spacing((v.abs() + b).numpy()))


def lp_expect(o, c: LpCase):
    """dict(C, bC [, C2, bC2], flagged = the fraction of A' elements with an allowance)"""
    g = o["case"]
    if c.mode == 1:
        Ar, Wr, flagged, move = bf16_operands(o)
        o2 = dict(o)
        o2["case"] = replace(g, ln="none", K1=0)
        o2["A"], o2["W"] = torch.from_numpy(Ar), torch.from_numpy(Wr)
        ref = R.gemm_expect(o2)
        if flagged.any():
            allow = torch.from_numpy(move @ np.abs(Wr.astype(np.float64)).T) * _act_lip(g.act)
            if "C2" in ref:
                ref["bC2"] = ref["bC2"] + allow
            if g.epi >= 2:
                allow = allow * R.SILU_LIP * R._mod_rows(o, torch.float64)[0].abs()
            ref["bC"] = ref["bC"] + allow
        if c.c_bf16:
            ref["bC"] = with_bf16_store(ref["C"], ref["bC"])
        ref["flagged"] = float(flagged.mean())
        return ref
    ref = R.gemm_expect(o)
    A, W = R.logical_A(o).double(), o["W"].double()
    if g.ln != "none":
        mean, rstd, _, _ = R._ln_terms(o, torch.float64)
        A = (A - mean[:, None]) * rstd[:, None]
    extra = DROP * U * (A.abs() @ W.abs().t()) * _act_lip(g.act)
    if g.act == ACT_GELU:       # the table's error in place of GELU_ABS, at the pre-activation y
        y = R.gemm_expect({**o, "case": replace(g, act=ACT_NONE, res=False, c2=False)})["C"].abs()
        extra = extra + y * (TAB_TAYLOR + PHI_MAX * (y + 6.0) * U + 4 * U) + TAB_CLAMP - R.GELU_ABS
    ref["bC"] = ref["bC"] + 2 * extra
    if "C2" in ref:
        ref["bC2"] = ref["bC2"] + 2 * extra
    ref["flagged"] = 0.0
    return ref


# ------------------------------------------------------------------------------------------------------------------------------
# NumPy emulation of the kernels' arithmetic, with one-line mistakes for the host tests
# ------------------------------------------------------------------------------------------------------------------------------
MISTAKES = ("split_drop_mid", "split_no_midmid", "a_trunc", "w_trunc", "half_chunk_full", "k1_chunk_off", "swap_row_blocks", "table_no_m0",
            "stats_all_cols", "mod_before_c2", "cbf_trunc", "wrong_nparts")


def _r32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def _gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(torch.from_numpy(np.ascontiguousarray(x)) / math.sqrt(2.0)).numpy())


def _silu64(x):
    return x / (1.0 + np.exp(-x))


_TAB = None


def gelu_table_f32(x):
    """gelu_lut of kernels_common.hip.h op by op in float32 (as tests/test_abi.py::test_gelu_table_accuracy restates it)"""
    global _TAB
    if _TAB is None:
        xs = -6.0 + np.arange(769) / 64.0
        phi = np.exp(-0.5 * xs * xs) / np.sqrt(2 * np.pi)
        Phi = 0.5 * (1.0 + np.vectorize(math.erf)(xs / math.sqrt(2.0)))
        _TAB = np.stack([Phi, phi, -0.5 * xs * phi], 1).astype(np.float32)
    x = x.astype(np.float32)
    t = np.clip(x + np.float32(6), np.float32(0), np.float32(12)).astype(np.float32)
    r = np.rint(t * np.float32(64)).astype(np.float32)
    d = _r32(r.astype(np.float64) * -0.015625 + t)
    c = _TAB[r.astype(np.int64)]
    return _r32(x.astype(np.float64) * _r32(d.astype(np.float64) * _r32(d.astype(np.float64) * c[..., 2] + c[..., 1]) + c[..., 0]))


def _ln_coeffs(o, mistake):
    """(rstd, -mean rstd) per row in the kernel's fp32 arithmetic; the hardware rsq is stood in for by the rounded exact value"""
    g = o["case"]
    if g.ln == "stats":
        st = o["ln_stats"].numpy()
        mean, rstd = st[:, 0], st[:, 1]
    else:
        P = R.logical_partials(o).numpy()
        n = P.shape[1] - (1 if mistake == "wrong_nparts" else 0)
        f = np.float32
        if n == 2:
            sm, sq = P[:, 0, 0] + P[:, 1, 0], P[:, 0, 1] + P[:, 1, 1]
        elif n == 4:
            sm, sq = (P[:, 0, 0] + P[:, 1, 0]) + (P[:, 2, 0] + P[:, 3, 0]), (P[:, 0, 1] + P[:, 1, 1]) + (P[:, 2, 1] + P[:, 3, 1])
        else:
            sm, sq = np.zeros(g.M, f), np.zeros(g.M, f)
            for t in range(n):
                sm, sq = sm + P[:, t, 0], sq + P[:, t, 1]
        invk = f(1.0) / f(g.K)
        mean = (sm * invk).astype(f)
        var = _r32((sq * invk).astype(f).astype(np.float64) - mean.astype(np.float64) ** 2)
        rstd = _r32(1.0 / np.sqrt((np.maximum(var, f(0)) + f(R.LN_EPS)).astype(f).astype(np.float64)))
    return rstd.astype(np.float32), _r32(-mean.astype(np.float64) * rstd.astype(np.float64))


def _flat_tail(X, ld, rows, k0, k1):
    """columns k0 .. k1 of each row read straight on through the physical row-major buffer (what an unclamped load picks up)"""
    flat = np.concatenate([X.reshape(-1), np.zeros(k1, np.float32)])
    idx = np.arange(rows)[:, None] * ld + np.arange(k0, k1)[None, :]
    return flat[idx]


def emulate(o, c: LpCase, mistake=None):
    """The kernel's arithmetic in NumPy: operands rounded (bf16) or split into planes, fp32 accumulator fed in ascending 16-k steps with
    exact products (float64 inside a step), the epilogue op by op in fp32, bf16 store.  dict(C, C2 or None, stats or None)"""
    g = o["case"]
    M, N, K = g.M, g.N, g.K
    A = R.logical_A(o).numpy().astype(np.float32)
    if mistake == "k1_chunk_off" and g.K1:      # the switch to the second source comes one chunk late: that chunk reads on in the first
        A, w = A.copy(), min(c.kb, K - g.K1)
        A[:, g.K1:g.K1 + w] = _flat_tail(o["A"].numpy(), o["lda"], M, g.K1, g.K1 + w)
        A[:, g.K1 + w:] = o["A2"].numpy()[:, :K - g.K1 - w]
    W = o["W"].numpy().astype(np.float32)
    if g.ln != "none":
        rstd, nmr = _ln_coeffs(o, mistake)
        A = _r32(A.astype(np.float64) * rstd.astype(np.float64)[:, None] + nmr.astype(np.float64)[:, None])
    Kx = K
    if c.mode == 1:
        Ap = [widen((bf16_trunc_bits if mistake == "a_trunc" else bf16_rne_bits)(A))]
        Wp = [widen((bf16_trunc_bits if mistake == "w_trunc" else bf16_rne_bits)(W))]
        if mistake == "half_chunk_full" and K % c.kb:       # the last chunk's invalid half is not zeroed: rows read on in memory
            Kx = (K + c.kb - 1) // c.kb * c.kb
            src = o["A"].numpy() if not g.K1 else None
            tailA = _flat_tail(src, o["lda"], M, K, Kx) if src is not None else np.ones((M, Kx - K), np.float32)
            Ap = [np.concatenate([Ap[0], bf16_rne(tailA)], 1)]
            Wp = [np.concatenate([Wp[0], _flat_tail(Wp[0], K, N, K, Kx)], 1)]
        order = [(0, 0)]
    else:
        Ap, Wp = list(split3(A)), list(split3(W))
        if mistake == "split_drop_mid":
            Ap[1] = np.zeros_like(Ap[1])
        # SPLIT_UNIT_FIRST's order: (a hi, w lo), (a mid, w mid), (a hi, w mid), (a lo, w hi), (a mid, w hi), (a hi, w hi)
        order = [(0, 2), (1, 1), (0, 1), (2, 0), (1, 0), (0, 0)]
        if mistake == "split_no_midmid":
            order.remove((1, 1))
    acc = np.zeros((M, N), np.float32)
    for k in range(0, Kx, 16):
        for ia, iw in order:
            acc = _r32(acc.astype(np.float64) + Ap[ia][:, k:k + 16].astype(np.float64) @ Wp[iw][:, k:k + 16].astype(np.float64).T)
    v = (acc + o["bias"].numpy()[None, :]).astype(np.float32)
    if g.act == ACT_GELU:
        v = gelu_table_f32(v) if c.mode == 2 else _r32(_gelu64(v.astype(np.float64)))
    elif g.act == ACT_SILU:
        v = _r32(_silu64(v.astype(np.float64)))
    if g.res:
        v = (v + o["res"].numpy()[:, :N]).astype(np.float32)
    out = {"C2": v.copy() if g.c2 else None, "stats": None}
    if g.epi >= 2:
        aff = o["mod_aff"].numpy()
        rows = np.arange(M)
        if g.epi == 3:
            b = ((rows % c.tile_rows) if mistake == "table_no_m0" else rows) // g.mod_T
        else:
            b = np.zeros(M, np.int64)
        msc = (aff[b, g.mod_off:g.mod_off + N] + np.float32(1)).astype(np.float32)
        msh = aff[b, g.mod_off + N:g.mod_off + 2 * N]
        v = _r32(_silu64(_r32(v.astype(np.float64) * msc + msh).astype(np.float64)))
        if mistake == "mod_before_c2" and g.c2:
            out["C2"] = v.copy()
    if g.epi >= 1:
        S = np.zeros((M, g.tiles_n, 2), np.float32)
        for t in range(g.tiles_n):
            seg = v[:, GBN * t:GBN * (t + 1)].astype(np.float64)
            if mistake == "stats_all_cols" and seg.shape[1] < GBN:      # the columns past N carry silu(shift) of a neighbouring column
                seg = np.concatenate([seg, np.repeat(seg[:, -1:], GBN - seg.shape[1], 1)], 1)
            S[:, t, 0], S[:, t, 1] = seg.sum(1), (seg * seg).sum(1)
        out["stats"] = S
    if c.c_bf16:
        v = widen((bf16_trunc_bits if mistake == "cbf_trunc" else bf16_rne_bits)(v))
    if mistake == "swap_row_blocks" and M >= 64:      # the two 32-row blocks of the first 64-row wave tile change places
        v = v.copy()
        v[0:32], v[32:64] = v[32:64].copy(), v[0:32].copy()
    out["C"] = v
    return out


def ratios(o, c: LpCase, ref, got):
    """worst |error| / bar of each output of `got` (emulate's layout: C, C2, stats as float32 arrays [M, ...])"""
    g = o["case"]
    r = {"C": R.worst_ratio(torch.from_numpy(got["C"]), ref["C"], ref["bC"])}
    if "C2" in ref:
        r["C2"] = R.worst_ratio(torch.from_numpy(got["C2"]), ref["C2"], ref["bC2"])
    if g.epi >= 1:
        S, Bd = R.stats_expect(torch.from_numpy(got["C"]), g, ref["C"], ref["bC"])
        r["stats"] = R.worst_ratio(torch.from_numpy(got["stats"]), S, Bd)
    return r
