"""Cases, operand builders, float64 references, derived bars and a NumPy emulation for the bf16 block pipeline's GEMM and fused-MLP
kernels (csrc/kernels_bx.hip: gemm_bx_kernel in its three tile geometries; mlp_bx_kernel<96 | 192 | 384>, mlp384_bx_kernel,
mlp384d_bx_kernel, mlp384s_bx_kernel, mlp96r_bx_kernel), shared by tests/test_bx_forms.py (GPU: the kernels against these, through
dsg_debug_gemm_bx_args / dsg_debug_mlp_bx_args, which hand the caller's own bf16 tensors to the launchers) and
tests/test_bx_forms_host.py (CPU: the power of these checks).  Built on f32_ref (summation bound, activation / residual / modulate
terms), edge_ref (LayerNorm element bound) and lp_ref (bf16 bit restatements, with_bf16_store).  Nothing below is taken from a
kernel's output.  u = 2^-24.

gemm_bx.  Both operands are bf16 tensors already: every product is exact in fp32 and only the accumulation rounds, so the reference is
the float64 product of the given operands and the bar is f32_ref's (K + 8) u (|A| |W|^T + |bias|) with its activation, residual and
modulate terms (f32_ref.gemm_expect on the operands as a plain product).  No element is ever flagged: nothing is rounded in front of the
product.  What the kernel derives from a value it has just stored is checked against THAT value: a plain bf16 store next to the fp32 one
is bit for bit the round-to-nearest-even of the stored fp32 word (the kernel rounds the same register), the LayerNorm output is the
float64 LayerNorm of the stored row inside lp_ref.with_bf16_store(edge_ref.ln_elem_bound).  Without an fp32 store the bf16 tensors are
held to the reference: with_bf16_store(ref, bar), and for the LayerNorm the row's bar carried through the normalisation
(ln_bound_perturbed: |dy_i| <= rstd (b_i + mean b) + |y_i| d var / (2 (var + eps)), d var <= 2 mean(|d| (b + mean b)) + mean((b + mean b)^2)).

Fused MLP.  x <- [modulate](x1 + fc2(bf16(GELU(fc1(xn))))), with proj in front x1 = x + att Wp^T + bp and xn = bf16(LayerNorm(x1)), else
x1 = x.  Dense operands (random normal) keep tests/test_bx_kernels.py's flat bars -- 5e-4 (mlp) and 1e-3 (proj + mlp) of the output scale --
because one hidden value that rounds to the other bf16 neighbour moves an output by about 1e-3; they pin indexing.  Exact operands
(exact_mlp_case) make a derived per-element bar possible: weights with eight nonzeros +-2^-e per row, biases on a 1/64 grid, inputs on
1/8 and 1/16 grids, so that every fc1 sum (without proj) and every proj sum and x1 itself (with proj) is exact in fp32 in any order and
each product's summation bound is (8 + 8) u sum |.||.| instead of (K + 8) u.  An element of a rounded tensor is FLAGGED when its float64
value lies within pert of a bf16 rounding boundary (pert: hidden 2 (GELU_LIP fc1 bound + GELU_ABS + u |g|), LayerNorm-2
ln_elem_bound(x1) + u |ln|); only then can the kernel's rounding fall to the other neighbour, and the element gets lp_ref's allowance
(spacing + pert) |w|.  A hidden unit behind a flagged LayerNorm element has moved by up to dg = GELU_LIP times that element's allowance
before its own rounding: it still rounds to the reference's bf16 value unless a boundary lies within dg + pert, and only then gets
the allowance dg + pert + the spacing at the moved magnitude.  The nonzero positions are grouped -- the
eight hidden units an output reads all read the same eight LayerNorm columns -- so that one flagged LayerNorm element widens the bars of
one group of outputs and not of all of them.  Conditions (asserted on the host for every exact case): at most FLAG_CAP of either rounded
tensor flagged; at least half of the output elements with a bar below TIGHT of the output scale."""
from dataclasses import dataclass

import numpy as np
import torch

import edge_ref as X
import f32_ref as R
import lp_ref as P
from f32_ref import ACT_GELU, ACT_NONE, U

GUARD = 2
NAN32, NAN16 = np.uint32(0x7FC00000), np.uint16(0x7FC0)
GEO = {0: (128, 192, 64), 2: (256, 96, 32), 3: (128, 384, 64)}      # geometry -> (row tile, column tile, k chunk)
FLAG_CAP, TIGHT = 0.10, 1e-5
MLP_BAR, PROJMLP_BAR = 5e-4, 1e-3                                    # tests/test_bx_kernels.py's, of the output scale
HOST_CUS = 256                                                      # the CU count the host file sizes the persistence cases with


# ------------------------------------------------------------------------------------------------------------------------------
# gemm_bx: cases
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class BxGemmCase:
    fam: str
    M: int
    N: int
    K: int
    geo: int                  # the geometry the launcher must pick (the table the host file holds the restated rule to)
    bias: bool = True
    act: int = ACT_NONE
    res: bool = False
    alias: bool = False       # C is the residual buffer (updated in place)
    c: bool = True            # fp32 store
    cb: bool = False          # bf16 store (with ln: the LayerNorm of the stored row)
    c2b: bool = False         # bf16 copy of the value before the modulate
    ln: bool = False
    mod: int = 0              # 0 none, 1 batch-uniform (mod_ld == 0), 2 per sample
    mod_off: int = 0
    mod_T: int = 0            # rows per sample (mod 2); 0: M
    K1: int = 0               # > 0: A2 concat
    pad: bool = False         # lda > K, ldres != ldc (unless aliased), ldcb != ldc2b, all wider than the default
    seed: int = 0

    def ident(self):
        s = f"{self.fam}-g{self.geo}-M{self.M}-N{self.N}-K{self.K}"
        if self.K1: s += f"-K1_{self.K1}"
        if self.mod: s += f"-mod{self.mod}-off{self.mod_off}" + (f"-T{self.mod_T}" if self.mod_T else "")
        return s + ("-pad" if self.pad else "")

    @property
    def T(self):
        return self.mod_T if self.mod_T else self.M

    @property
    def instance(self):
        """the template instantiation the launcher runs: (geometry, RES, MOD)"""
        return (self.geo, self.res, self.mod)


FAMILIES = {      # the epilogue combinations the forward launches (run_block_bx, attach_bx_out, the merge / breakup GEMMs of dsg_api.cpp)
    "qkv": dict(cb=True, c=False),
    "fc1": dict(act=ACT_GELU, cb=True, c=False),
    "proj": dict(res=True, alias=True, ln=True, cb=True),
    "fc2": dict(res=True, alias=True, mod=1, ln=True, cb=True),
    "fc2w": dict(res=True, alias=True, mod=1),                      # a row wider than a tile: the modulate without the LayerNorm
    "fc2c": dict(res=True, alias=True, cb=True),                    # the last block of a level: the plain bf16 copy of the stored row
    "merge": dict(bias=False, c2b=True, mod=1, ln=True, cb=True),
    "pre": dict(),                                                  # pre_linear: two sources, fp32 store only
    "post": dict(mod=1, ln=True, cb=True),
    "post0": dict(cb=True),                                         # post_linear in front of a level without blocks: C and its copy
    "mergec": dict(bias=False, cb=True, c2b=True),                 # C, its copy and the pre-modulate copy: Cb takes the direct 8-byte store
    "lnfree": dict(ln=True, cb=True, c=False),                      # LayerNorm output without an fp32 store (one case per geometry)
    "plain": dict(),
}
GEO_N = {0: {"ln": (192,), "wide": (192, 384)}, 2: {"ln": (96,), "wide": (96, 288, 8, 40, 104, 200)}, 3: {"ln": (384,), "wide": ()}}
GEO_K = {0: (72, 96, 128, 192, 320), 2: (64, 96, 160), 3: (72, 96, 128, 192, 320)}


def geo_M(geo):
    bm = GEO[geo][0]
    return (1, bm - 1, bm, bm + 1, 8 * bm + 1, 17 * bm + 3)


def _edge_cases():
    """every family at every M edge of every geometry it runs on, N and K walking their edge lists; MOD alternates 1 / 2 and mod_off
    0 / 2N + 8"""
    out, seed = [], 0
    for geo in (0, 2, 3):
        for fi, (fam, f) in enumerate(FAMILIES.items()):
            if fam in ("lnfree", "plain", "fc2w", "mergec"):
                continue
            Ns = GEO_N[geo]["ln" if f.get("ln") else "wide"]
            if not Ns:
                continue
            for i, M in enumerate(geo_M(geo)):
                N, K = Ns[(i + fi) % len(Ns)], GEO_K[geo][(i + 2 * fi) % len(GEO_K[geo])]
                kw = dict(f)
                if kw.get("mod"):
                    kw["mod"] = 1 + (i + fi) % 2
                    kw["mod_off"] = (0, 2 * N + 8)[(i // 2 + fi) % 2]
                    if kw["mod"] == 2:
                        kw["mod_T"] = (0, 100)[i % 2] if M > 100 else 0
                if fam == "pre":
                    kb = GEO[geo][2]
                    K = (128, 192, 192, 128, 192, 128)[i] if geo == 0 else 96
                    kw["K1"] = ((64, 64, 128, 64, 128, 64)[i] if geo == 0 else (32, 64)[i % 2])
                    assert kw["K1"] % kb == 0
                out.append(BxGemmCase(fam, M, N, K, geo, seed=seed, **kw))
                seed += 1
    return out


def _mod_cases():
    """MOD 0 / 1 / 2 x mod_off on one shape per geometry; MOD 2 with 36-row samples at M = 324 (a sample boundary inside every row tile of
    every geometry and inside the ragged last one) and with one sample; fc2 at N = 768 (the modulate without LayerNorm)"""
    out, seed = [], 500
    for geo, N in ((0, 192), (2, 96), (3, 384)):
        for fam in ("fc2", "merge", "post"):
            for mod, off, T in ((1, 0, 0), (1, 2 * N + 8, 0), (2, 0, 36), (2, 2 * N + 8, 36), (2, 2 * N + 8, 0)):
                out.append(BxGemmCase(fam, 324, N, GEO_K[geo][seed % len(GEO_K[geo])], geo, mod_off=off, mod_T=T, seed=seed,
                                      **{**FAMILIES[fam], "mod": mod}))
                seed += 1
        out.append(BxGemmCase("proj", 324, N, GEO_K[geo][0], geo, seed=seed, **FAMILIES["proj"]))      # RES with MOD 0 at the same shape
        seed += 1
    for i, (M, mod, off, T) in enumerate(((324, 1, 0, 0), (324, 2, 1544, 36), (129, 2, 0, 0), (1025, 1, 1544, 0), (2179, 2, 0, 100), (127, 0, 0, 0))):
        out.append(BxGemmCase("fc2w", M, 768, (128, 192, 72, 96, 320, 128)[i], 0, mod_off=off, mod_T=T, seed=seed, **{**FAMILIES["fc2w"], "mod": mod}))
        seed += 1
    # MOD without a residual and without LayerNorm (merge into a level wider than a tile), and MOD 0 / RES 0 with every store
    for i, (geo, N) in enumerate(((0, 384), (2, 288), (0, 768))):
        for mod in (1, 2):
            out.append(BxGemmCase("merge", 324, N, GEO_K[geo][i], geo, bias=False, c2b=True, mod=mod, mod_off=(2 * N + 8) * (mod - 1), mod_T=36 * (mod - 1),
                                  seed=seed))
            seed += 1
    return out


def _misc_cases():
    out = []
    # LayerNorm without an fp32 store: one per geometry
    for i, (geo, N) in enumerate(((0, 192), (2, 96), (3, 384))):
        out.append(BxGemmCase("lnfree", GEO[geo][0] + 1, N, GEO_K[geo][1], geo, seed=700 + i, **FAMILIES["lnfree"]))
    # Cb without LayerNorm next to C2b: C2b occupies the transposition buffer and Cb leaves by the direct 8-byte store
    for i, (geo, N, M, mod) in enumerate(((0, 384, 129, 0), (2, 200, 257, 0), (0, 192, 324, 1), (2, 288, 324, 2), (2, 8, 300, 0), (0, 768, 1025, 2))):
        out.append(BxGemmCase("mergec", M, N, GEO_K[geo][i % 3], geo, mod=mod, mod_off=(2 * N + 8) * (i % 2), mod_T=36 * (mod == 2), pad=(i == 1),
                              seed=704 + i, **FAMILIES["mergec"]))
    # N % 8 == 4: only the fp32 store is admitted
    out += [BxGemmCase("plain", M, 100, K, 2, seed=710 + i) for i, (M, K) in enumerate(((1, 64), (257, 96), (2049, 160)))]
    out += [BxGemmCase("plain", 129, 100, 96, 2, res=True, seed=714), BxGemmCase("plain", 300, 4, 64, 2, seed=715)]
    # A2: (K1, K) with lda2 != lda
    for i, (K1, K) in enumerate(((64, 128), (64, 192), (128, 192))):
        out.append(BxGemmCase("pre", 300, (192, 384, 576)[i], K, 0, K1=K1, seed=720 + i))
    for i, (K1, K) in enumerate(((32, 96), (64, 96))):
        out.append(BxGemmCase("pre", 300, (288, 200)[i], K, 2, K1=K1, seed=725 + i))
    out.append(BxGemmCase("pre", 300, 192, 96, 0, K1=64, seed=727))      # the second source starts the half-valid chunk
    # pitches: one per epilogue family
    for i, (fam, geo, N, K) in enumerate((("qkv", 2, 288, 96), ("fc1", 0, 384, 72), ("proj", 3, 384, 96), ("fc2", 0, 192, 128), ("fc2w", 0, 768, 96),
                                          ("fc2c", 2, 200, 64), ("merge", 2, 96, 160), ("pre", 0, 192, 128), ("post", 3, 384, 192),
                                          ("post0", 2, 104, 96))):
        kw = dict(FAMILIES[fam])
        if kw.get("mod"):
            kw.update(mod=1 + i % 2, mod_off=2 * N + 8, mod_T=36 * (i % 2))
        if fam == "pre":
            kw["K1"] = 64
        out.append(BxGemmCase(fam, 300, N, K, geo, pad=True, seed=740 + i, **kw))
    # K = 1536: the forward's fc2 depth, at M = BM + 1 (the (K + 8) u bound is wide here: about 1e-4 of sum |a||w|)
    for i, (geo, N) in enumerate(((0, 192), (2, 96), (3, 384))):
        out.append(BxGemmCase("fc2", GEO[geo][0] + 1, N, 1536, geo, mod_off=2 * N + 8, seed=760 + i, **FAMILIES["fc2"]))
    return out


def persistence_grid(geo, n_cu):
    return max(8, n_cu * (1 if geo == 3 else 2) // 8 * 8)


def persistence_cases(n_cu):
    """one per geometry in which a block takes a second tile: the smallest M with round_up8(tiles_m) tiles_n > grid and tiles_m % 8 == 1,
    at the geometry's smallest K"""
    out = []
    for i, (geo, N) in enumerate(((0, 1536), (2, 288), (3, 384))):
        bm, bn, _ = GEO[geo]
        tiles_n, tm = (N + bn - 1) // bn, 1
        while (tm + 7) // 8 * 8 * tiles_n <= persistence_grid(geo, n_cu):
            tm += 8
        fam = "qkv" if geo != 3 else "proj"
        kw = dict(FAMILIES[fam], c=True)
        out.append(BxGemmCase(fam, (tm - 1) * bm + 1, N, 2 * GEO[geo][2], geo, seed=780 + i, **kw))
    return out


def gemm_cases():
    return _edge_cases() + _mod_cases() + _misc_cases()


# forms launch_gemm_bx refuses, each beside the admitted form it differs from in one field.  Base call: M = 300, N = 192, K = 128, bias,
# fp32 store, default pitches.  (name, admitted neighbour, refused form); buffers are named by flags and filled in by the test.
REFUSALS = [
    ("K of one chunk, geo 0", dict(K=128), dict(K=64)),
    ("K of one chunk, geo 2", dict(N=96, K=64), dict(N=96, K=32)),
    ("K % 8 != 0", dict(K=136), dict(K=132, lda=136)),
    ("geo 2 with K % 32 != 0", dict(N=96, K=96), dict(N=96, K=72)),
    ("N % 4 != 0", dict(N=100), dict(N=98, ldc=100)),
    ("bf16 output with N % 8 != 0", dict(N=104, cb=True), dict(N=100, cb=True)),
    ("Cb pitch % 8 != 0", dict(N=96, cb=True, ldcb=104), dict(N=96, cb=True, ldcb=100)),
    ("C2b pitch % 8 != 0", dict(c2b=True, ldc2b=200), dict(c2b=True, ldc2b=196)),
    ("GELU with res", dict(act=ACT_GELU), dict(act=ACT_GELU, res=True)),
    ("ln_out without Cb", dict(ln=True, cb=True), dict(ln=True)),
    ("ln_out at N = 288", dict(N=96, ln=True, cb=True), dict(N=288, ln=True, cb=True)),
    ("A2 with K1 % 64 != 0, geo 0", dict(K1=64), dict(K1=32)),
    ("A2 with K1 % 32 != 0, geo 2", dict(N=96, K1=32), dict(N=96, K1=16)),
    ("lda % 8 != 0", dict(lda=136), dict(lda=132)),
    ("activation 2", dict(act=ACT_GELU), dict(act=2)),
]


def refusal_args(kw):
    """one entry of REFUSALS resolved against the base call: every argument of gemm_rule, and the flags the test fills buffers for"""
    a = dict(M=300, N=192, K=128, lda=256, act=ACT_NONE, res=False, cb=False, c2b=False, ln=False, K1=0, lda2=256)
    a.update(kw)
    a.setdefault("ldc", a["N"] + 4)
    a.setdefault("ldcb", (a["N"] + 15) // 8 * 8)
    a.setdefault("ldc2b", (a["N"] + 15) // 8 * 8)
    return a


def gemm_rule(N, K, lda, act=ACT_NONE, res=False, cb=False, c2b=False, ln=False, K1=0, lda2=8, ldcb=8, ldc2b=8, M=1, ldc=0):
    """bx_gemm_geo of csrc/kernels_bx.hip restated: the tile geometry, or -1 where the launcher refuses"""
    if M < 1 or N < 1 or K < 8 or K % 8 or N % 4 or act not in (ACT_NONE, ACT_GELU):
        return -1
    if lda % 8 or (K1 and (lda2 % 8 or K1 <= 0)):
        return -1
    if (cb or c2b) and (N % 8 or (cb and ldcb % 8) or (c2b and ldc2b % 8)):
        return -1
    if act == ACT_GELU and res:
        return -1
    if ln:
        if not cb or N not in (96, 192, 384):
            return -1
        geo = {96: 2, 192: 0, 384: 3}[N]
    else:
        geo = 0 if N % 192 == 0 else 2
    kb = GEO[geo][2]
    if (K1 and K1 % kb) or (geo == 2 and K % 32) or (K + kb - 1) // kb < 2:
        return -1
    return geo


# ------------------------------------------------------------------------------------------------------------------------------
# gemm_bx: operands, buffers, reference
# ------------------------------------------------------------------------------------------------------------------------------
def _bf(t):
    return t.to(torch.bfloat16).float()


def gemm_pitches(c: BxGemmCase):
    K1 = c.K1 if c.K1 else c.K
    p = dict(lda=K1 + (16 if (c.pad or c.K1) else 0), lda2=(c.K - K1 + 8) if c.K1 else 0, ldc=c.N + (12 if c.pad else 4),
             ldcb=c.N + (16 if c.pad else 8), ldc2b=c.N + (24 if c.pad else 8))
    p["ldres"] = p["ldc"] if c.alias else c.N + (20 if c.pad else 4)
    return p


def make_gemm(c: BxGemmCase):
    """operands of one case on the CPU (seeded): A, A2, W float32 arrays of bf16 values in the physical layouts the kernel reads (padding
    columns hold a value a wrong pitch would pick up), and the f32_ref case the reference is evaluated with"""
    gen = torch.Generator().manual_seed(7000 + c.seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    M, N, K = c.M, c.N, c.K
    K1 = c.K1 if c.K1 else K
    o = {"bx": c, **gemm_pitches(c)}
    o["case"] = R.GemmCase(M, N, K, act=c.act, res=c.res, K1=c.K1, c2=c.c2b, epi=(0, 2, 3)[c.mod], mod_T=c.T, mod_off=c.mod_off)
    A = torch.full((M, o["lda"]), 7.0)
    A[:, :K1] = _bf(rn(M, K1))
    o["A"] = A
    if c.K1:
        A2 = torch.full((M, o["lda2"]), -5.0)
        A2[:, :K - K1] = _bf(rn(M, K - K1))
        o["A2"] = A2
    o["W"] = _bf(rn(N, K) / K ** 0.5)
    o["bias"] = rn(N) * 0.3 if c.bias else torch.zeros(N)
    if c.res:
        Rs = torch.full((M, o["ldres"]), 3.0)
        Rs[:, :N] = rn(M, N)
        o["res"] = Rs
    if c.mod:
        nb = (M + c.T - 1) // c.T if c.mod == 2 else 1
        o["mod_ld"] = (c.mod_off + 2 * N + 12) if c.mod == 2 else 0
        o["mod_aff"] = rn(nb, c.mod_off + 2 * N + 12) * 0.5
    return o


def _nan_buf(rows, ld, dtype):
    return np.full((rows + GUARD, ld), NAN32 if dtype == np.uint32 else NAN16, dtype=dtype)


def gemm_buffers(o):
    """the output buffers before the launch as bit patterns: C uint32 [M + GUARD, ldc], Cb / C2b uint16; NaN everywhere, except that an
    aliased C is the residual buffer (its guard rows NaN)"""
    c = o["bx"]
    b = {"C": None, "Cb": None, "C2b": None}
    if c.c:
        b["C"] = _nan_buf(c.M, o["ldc"], np.uint32)
        if c.alias:
            b["C"][:c.M] = o["res"].numpy().view(np.uint32)
    if c.cb:
        b["Cb"] = _nan_buf(c.M, o["ldcb"], np.uint16)
    if c.c2b:
        b["C2b"] = _nan_buf(c.M, o["ldc2b"], np.uint16)
    return b


def layer_norm64(x):
    return R.layer_norm(x.double())


def ln_bound_perturbed(x64, b):
    """edge_ref.ln_elem_bound of the rows x64, plus what a perturbation of the input within the per-element bar b does to the result"""
    _, (d, rstd, _, _) = X.row_stats_bound(x64)
    var = d.pow(2).mean(1)
    bb = b + b.mean(1, keepdim=True)
    dvar = 2 * (d.abs() * bb).mean(1) + bb.pow(2).mean(1)
    n = d * rstd[:, None]
    return X.ln_elem_bound(x64) + rstd[:, None] * bb + n.abs() * (0.5 * dvar / (var + R.LN_EPS))[:, None]


def gemm_expect(o):
    """f32_ref.gemm_expect on the bf16 operands as a plain product: dict(C, bC [, C2, bC2])"""
    return R.gemm_expect(o)


def _outside_untouched(init, got, M, N):
    keep = init == got
    keep[:M, :N] = True
    return bool(keep.all())


def _ratio(got32, ref, bar):
    return R.worst_ratio(torch.from_numpy(np.ascontiguousarray(got32)), ref, bar)


def check_gemm(o, ref, init, got):
    """every check of one launch.  init / got: the buffers of gemm_buffers before and after (same layout).  Returns {check: worst
    |err| / bound}: bit-for-bit checks and the untouched-outside checks give 0 or inf."""
    c = o["bx"]
    M, N = c.M, c.N
    r = {}
    INF = float("inf")
    stored = None
    for k in ("C", "Cb", "C2b"):
        if init[k] is not None:
            r[k + " outside"] = 0.0 if _outside_untouched(init[k], got[k], M, N) else INF
    if c.c:
        stored = got["C"][:M, :N].view(np.float32)
        r["C"] = _ratio(stored, ref["C"], ref["bC"])
    if c.cb:
        gb = got["Cb"][:M, :N]
        if c.ln:
            if c.c:
                s64 = torch.from_numpy(np.nan_to_num(stored)).double()
                lr = layer_norm64(s64)
                r["Cb ln(stored)"] = _ratio(P.widen(gb), lr, P.with_bf16_store(lr, X.ln_elem_bound(s64)))
            else:
                lr = layer_norm64(ref["C"])
                r["Cb ln(ref)"] = _ratio(P.widen(gb), lr, P.with_bf16_store(lr, ln_bound_perturbed(ref["C"], ref["bC"])))
        elif c.c:
            r["Cb bits"] = 0.0 if np.array_equal(gb, P.bf16_rne_bits(stored)) else INF
        else:
            r["Cb"] = _ratio(P.widen(gb), ref["C"], P.with_bf16_store(ref["C"], ref["bC"]))
    if c.c2b:
        g2 = got["C2b"][:M, :N]
        if c.mod == 0 and c.c:
            r["C2b bits"] = 0.0 if np.array_equal(g2, P.bf16_rne_bits(stored)) else INF
        else:
            r["C2b"] = _ratio(P.widen(g2), ref["C2"], P.with_bf16_store(ref["C2"], ref["bC2"]))
    return r


# ------------------------------------------------------------------------------------------------------------------------------
# NumPy emulation of gemm_bx_kernel, with one-line mistakes for the host tests
# ------------------------------------------------------------------------------------------------------------------------------
GEMM_MISTAKES = ("cb_trunc", "c2b_trunc", "ln_trunc", "half_chunk_full", "k1_chunk_off", "mod_before_c2", "scale_no_1", "neighbour_sample",
                 "mod_off_ignored", "ln_n_minus_4", "ln_premod", "swap_row_blocks")
_r32 = P._r32


def _rne(x, trunc=False):
    return (P.bf16_trunc_bits if trunc else P.bf16_rne_bits)(np.ascontiguousarray(x, dtype=np.float32))


def _acc_steps(acc, A, W):
    """acc += A W^T in ascending 16-k steps: exact products, one fp32 rounding per step"""
    for k in range(0, A.shape[1], 16):
        acc = _r32(acc.astype(np.float64) + A[:, k:k + 16].astype(np.float64) @ W[:, k:k + 16].astype(np.float64).T)
    return acc


def _lane_sums(v, width):
    """(sum, sumsq) per row as the kernels form them: a lane owns the columns 8 j + 4 half + {0..3} of each `width`-wide slab and adds
    them in ascending order in fp32; the two half-waves are added, then the slabs"""
    M, N = v.shape
    sm_t, sq_t = np.zeros(M, np.float32), np.zeros(M, np.float32)
    for s0 in range(0, N, width):
        parts = []
        for half in (0, 1):
            cols = [s0 + 8 * j + 4 * half + t for j in range(width // 8) for t in range(4)]
            sm, sq = np.zeros(M, np.float32), np.zeros(M, np.float32)
            for cidx in cols:
                x = v[:, cidx]
                sm = (sm + x).astype(np.float32)
                sq = _r32(x.astype(np.float64) * x.astype(np.float64) + sq.astype(np.float64))
            parts.append((sm, sq))
        sm_t = (sm_t + (parts[0][0] + parts[1][0]).astype(np.float32)).astype(np.float32)
        sq_t = (sq_t + (parts[0][1] + parts[1][1]).astype(np.float32)).astype(np.float32)
    return sm_t, sq_t


def _ln_rows(v, stats_of=None, n_stats=None, width=96):
    """the kernels' LayerNorm of the rows v in fp32: one-pass variance from lane-local sums, fma(v, rstd, -mean rstd); the hardware
    rsq is stood in for by the rounded exact value.  stats_of / n_stats: the mistakes' statistics source and column count"""
    f = np.float32
    s = np.ascontiguousarray(v if stats_of is None else stats_of).copy()
    if n_stats is not None:
        s[:, n_stats:] = 0
    sm, sq = _lane_sums(s, width)
    invn = f(1.0) / f(v.shape[1])
    mean = (sm * invn).astype(f)
    var = _r32((sq * invn).astype(f).astype(np.float64) - mean.astype(np.float64) ** 2)
    rstd = _r32(1.0 / np.sqrt((np.maximum(var, f(0)) + f(R.LN_EPS)).astype(f).astype(np.float64)))
    nmr = _r32(-mean.astype(np.float64) * rstd.astype(np.float64))
    return _r32(v.astype(np.float64) * rstd.astype(np.float64)[:, None] + nmr.astype(np.float64)[:, None])


def _modulate(v, aff, mod, off, T, N, mistake):
    M = v.shape[0]
    rows = np.arange(M)
    b = rows // T if mod == 2 else np.zeros(M, np.int64)
    if mistake == "neighbour_sample" and mod == 2 and aff.shape[0] > 1:      # the last row of every sample takes the next sample's
        last = (rows % T == T - 1) & (b + 1 < aff.shape[0])
        b = np.where(last, b + 1, b)
    if mistake == "mod_off_ignored":
        off = 0
    one = np.float32(0.0 if mistake == "scale_no_1" else 1.0)
    scl = (aff[b, off:off + N] + one).astype(np.float32)
    sft = aff[b, off + N:off + 2 * N]
    a = _r32(v.astype(np.float64) * scl.astype(np.float64) + sft.astype(np.float64))
    return _r32(P._silu64(a.astype(np.float64)))


def emulate_gemm(o, mistake=None):
    """gemm_bx_kernel's arithmetic in NumPy on the buffers of gemm_buffers: fp32 accumulator fed in ascending k chunks, + bias, GELU,
    + residual, bf16 copy, modulate + SiLU, fp32 store, bf16 store or LayerNorm from lane-local sums.  Returns the buffers after."""
    c = o["bx"]
    M, N, K = c.M, c.N, c.K
    kb = GEO[c.geo][2]
    A = R.logical_A(o).numpy().astype(np.float32)
    W = o["W"].numpy()
    if mistake == "k1_chunk_off" and c.K1:      # the switch to the second source comes one chunk late: that chunk reads on in the first
        A, w = A.copy(), min(kb, K - c.K1)
        A[:, c.K1:c.K1 + w] = P._flat_tail(o["A"].numpy(), o["lda"], M, c.K1, c.K1 + w)
    if mistake == "half_chunk_full" and K % kb:  # the last chunk's invalid part is not zeroed: rows read on in memory
        Kx = (K + kb - 1) // kb * kb
        src, ld, k0 = (o["A2"].numpy(), o["lda2"], K - c.K1) if c.K1 else (o["A"].numpy(), o["lda"], K)
        A = np.concatenate([A, P._flat_tail(src, ld, M, k0, k0 + Kx - K)], 1)
        W = np.concatenate([W, P._flat_tail(W, K, N, K, Kx)], 1)
    acc = _acc_steps(np.zeros((M, N), np.float32), A, W)
    v = (acc + o["bias"].numpy()[None, :]).astype(np.float32)
    if c.act == ACT_GELU:
        v = _r32(P._gelu64(v.astype(np.float64)))
    if c.res:
        v = (v + o["res"].numpy()[:, :N]).astype(np.float32)
    pre = v
    if c.mod:
        v = _modulate(v, o["mod_aff"].numpy(), c.mod, c.mod_off, c.T, N, mistake)
    out = gemm_buffers(o)
    if c.c2b:
        out["C2b"][:M, :N] = _rne(v if mistake == "mod_before_c2" else pre, mistake == "c2b_trunc")
    if c.ln:
        if mistake == "ln_n_minus_4":
            y = _ln_rows(v, n_stats=N - 4)
        elif mistake == "ln_premod":
            y = _ln_rows(pre)
        else:
            y = _ln_rows(v)
        cbv = _rne(y, mistake == "ln_trunc")
    else:
        cbv = _rne(v, mistake == "cb_trunc")
    if mistake == "swap_row_blocks" and M >= 64:      # the two 32-row blocks of the first wave tile change places
        v, cbv = v.copy(), cbv.copy()
        v[0:32], v[32:64] = v[32:64].copy(), v[0:32].copy()
        cbv[0:32], cbv[32:64] = cbv[32:64].copy(), cbv[0:32].copy()
    if c.c:
        out["C"][:M, :N] = v.view(np.uint32)
    if c.cb:
        out["Cb"][:M, :N] = cbv
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# fused MLP: cases
# ------------------------------------------------------------------------------------------------------------------------------
# name -> (C, DSG_BXK_* selector name, kernel launched, has a modulate); with proj the selector of dsg_debug_projmlp_bx
MLP_KERNELS = {
    "mlp96": (96, "DEFAULT", "mlp_bx_kernel<96>", True),
    "mlp192": (192, "DEFAULT", "mlp_bx_kernel<192>", True),
    "mlp384w": (384, "MLP384_WAVE", "mlp_bx_kernel<384>", True),
    "mlp384d": (384, "DEFAULT", "mlp384d_bx_kernel", True),
    "mlp384r3": (384, "MLP384_R3", "mlp384_bx_kernel", True),
    "mlp384s": (384, "MLP384_SOLO", "mlp384s_bx_kernel", True),
    "mlp96r": (96, "MLP96_RESIDENT", "mlp96r_bx_kernel", False),
}
# (kernel, proj) the launcher can select: the one-wave-per-SIMD kernel at C = 384 has no proj form the forward selects, the
# LDS-resident kernel only the proj form without a modulate
MLP_COMBOS = [(k, p) for k in MLP_KERNELS for p in (False, True) if not (k == "mlp384w" and p) and not (k == "mlp96r" and not p)]
MLP_M = (1, 31, 32, 33, 127, 128, 129, 257)


@dataclass(frozen=True)
class MlpCase:
    kern: str
    proj: bool
    M: int
    mod: int = 0
    mod_off: int = 0
    mod_T: int = 0
    out_mode: int = 0
    exact: bool = False
    seed: int = 0

    @property
    def C(self):
        return MLP_KERNELS[self.kern][0]

    @property
    def T(self):
        return self.mod_T if self.mod_T else self.M

    @property
    def selector(self):
        s = MLP_KERNELS[self.kern][1]
        return "MLP96_STAGED" if (self.kern == "mlp96" and self.proj and self.seed % 2) else s      # both names of the staged kernel

    def ident(self):
        s = f"{self.kern}-{'proj' if self.proj else 'mlp'}-M{self.M}-mod{self.mod}-off{self.mod_off}" + (f"-T{self.mod_T}" if self.mod_T else "")
        return s + f"-out{self.out_mode}" + ("-exact" if self.exact else "")


def mlp_dense_cases():
    """every (kernel, proj) at every row count, MOD / mod_off / out_mode walking their values so that each meets each kernel at three
    row counts or more; MOD 2 with 36-row samples at M = 324"""
    out, seed = [], 0
    for ci, (kern, proj) in enumerate(MLP_COMBOS):
        has_mod = MLP_KERNELS[kern][3]
        for i, M in enumerate(MLP_M):
            mod = (i + ci) % 3 if has_mod else 0
            Cc = MLP_KERNELS[kern][0]
            out.append(MlpCase(kern, proj, M, mod=mod, mod_off=(0, 2 * Cc + 8)[(i // 3 + ci) % 2] if mod else 0,
                               mod_T=(0, 36)[i % 2] if (mod == 2 and M > 36) else 0, out_mode=(i // 3 + ci) % 3, seed=seed))
            seed += 1
        if has_mod:
            for off in (0, 2 * MLP_KERNELS[kern][0] + 8):
                out.append(MlpCase(kern, proj, 324, mod=2, mod_off=off, mod_T=36, out_mode=1 + (seed % 2), seed=seed))
                seed += 1
        else:
            out.append(MlpCase(kern, proj, 324, out_mode=1, seed=seed))
            seed += 1
    return out


def mlp_exact_cases():
    """one exact case per kernel x proj x MOD at M = 129, and MOD 2 with 36-row samples at M = 324"""
    out, seed = [], 300
    for kern, proj in MLP_COMBOS:
        Cc, has_mod = MLP_KERNELS[kern][0], MLP_KERNELS[kern][3]
        for mod in ((0, 1, 2) if has_mod else (0,)):
            out.append(MlpCase(kern, proj, 129, mod=mod, mod_off=(2 * Cc + 8) * (mod == 1), mod_T=36 * (mod == 2), out_mode=1 + seed % 2, exact=True, seed=seed))
            seed += 1
        if has_mod:
            out.append(MlpCase(kern, proj, 324, mod=2, mod_off=2 * Cc + 8, mod_T=36, out_mode=1 + seed % 2, exact=True, seed=seed))
            seed += 1
    return out


def mlp96r_round2_case(n_cu):
    """mlp96r deals 32-row tiles to the 8 waves of at most n_cu blocks: more than 8 n_cu tiles and a block takes a second round"""
    return MlpCase("mlp96r", True, 32 * 8 * n_cu + 33, out_mode=1, seed=290)


def mlp_rule(c: MlpCase):
    """launch_mlp_bx and the hooks' selector rule restated: the kernel a case runs, None where refused"""
    Cc, sel = c.C, c.selector
    if not c.proj:
        if sel not in ("DEFAULT", "MLP384_DMA", "MLP384_WAVE", "MLP384_R3", "MLP384_SOLO") or (sel != "DEFAULT" and Cc != 384):
            return None
    else:
        k96 = sel in ("MLP96_STAGED", "MLP96_RESIDENT")
        if sel == "MLP384_WAVE" or (k96 and Cc != 96) or (not k96 and sel != "DEFAULT" and Cc != 384) or (sel == "MLP96_RESIDENT" and c.mod):
            return None
        if sel == "MLP96_RESIDENT":
            return "mlp96r_bx_kernel"
    if Cc != 384:
        return f"mlp_bx_kernel<{Cc}>"
    return {"DEFAULT": "mlp384d_bx_kernel", "MLP384_DMA": "mlp384d_bx_kernel", "MLP384_WAVE": "mlp_bx_kernel<384>", "MLP384_R3": "mlp384_bx_kernel",
            "MLP384_SOLO": "mlp384s_bx_kernel"}[sel]


# ------------------------------------------------------------------------------------------------------------------------------
# fused MLP: operands
# ------------------------------------------------------------------------------------------------------------------------------
def _grouped_weight(rows, cols, row_group, gen):
    """[rows, cols] with 8 nonzeros +-2^-e, e in {1, 2, 3}, per row: row r takes the 8 columns of column group row_group[r] (columns
    8 g .. 8 g + 7 after a seeded permutation of the columns), so every column is hit as soon as every group is"""
    perm = torch.randperm(cols, generator=gen)
    W = torch.zeros(rows, cols)
    e = torch.randint(1, 4, (rows, 8), generator=gen)
    sgn = torch.randint(0, 2, (rows, 8), generator=gen) * 2 - 1
    val = sgn.float() * torch.pow(2.0, -e.float())
    idx = perm[(8 * row_group[:, None] + torch.arange(8)[None, :])]
    W[torch.arange(rows)[:, None], idx] = val
    return W


def exact_mlp_case(c: MlpCase, gen):
    """the exact operands (module docstring).  Column groups: LayerNorm / input column group g (C / 8 of them) feeds the hidden units
    j with j % (C / 8) == g; output n reads eight hidden units of ONE such group, n's own (n % (C / 8)), drawn per group; proj output n reads
    the att columns of a seeded group."""
    Cc, H, M = c.C, 4 * c.C, c.M
    G = Cc // 8
    o = {}
    grid = lambda n, step, lim, *s: (torch.randint(-n, n + 1, s, generator=gen).float() * step).clamp(-lim, lim)
    o["in"] = grid(24, 0.125, 3.0, M, Cc)
    o["x"] = grid(32, 0.0625, 2.0, M, Cc)
    o["W1"] = _grouped_weight(H, Cc, torch.arange(H) % G, gen)
    # W2 row n: eight of the 32 hidden units of group n % G (hidden unit j = g + G i, i < 32); the group's eight outputs share two
    # permutations of its units, so every hidden unit is read twice
    W2 = torch.zeros(Cc, H)
    for g in range(G):
        slots = torch.cat([torch.randperm(32, generator=gen), torch.randperm(32, generator=gen)])
        for t in range(8):
            e = torch.randint(1, 4, (8,), generator=gen)
            sgn = torch.randint(0, 2, (8,), generator=gen) * 2 - 1
            W2[g + G * t, slots[8 * t:8 * t + 8] * G + g] = sgn.float() * torch.pow(2.0, -e.float())
    o["W2"] = W2
    o["b1"] = torch.randint(-64, 65, (H,), generator=gen).float() / 64
    o["b2"] = torch.randint(-64, 65, (Cc,), generator=gen).float() / 64
    if c.proj:
        o["Wp"] = _grouped_weight(Cc, Cc, torch.randperm(Cc, generator=gen) % G, gen)
        o["bp"] = torch.randint(-64, 65, (Cc,), generator=gen).float() / 64
    return o


def make_mlp(c: MlpCase, device="cpu"):
    """operands of one case (seeded, float32 holding bf16 values where the kernel reads bf16): in = xn or att [M, C], x, W1, b1, W2, b2
    [, Wp, bp], mod_aff [nb, mod_ld']"""
    gen = torch.Generator().manual_seed(9000 + c.seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    Cc, M = c.C, c.M
    if c.exact:
        o = exact_mlp_case(c, gen)
    else:
        o = {"in": _bf(rn(M, Cc)), "x": rn(M, Cc), "W1": _bf(rn(4 * Cc, Cc) / Cc ** 0.5), "b1": rn(4 * Cc) * 0.3,
             "W2": _bf(rn(Cc, 4 * Cc) / (4 * Cc) ** 0.5), "b2": rn(Cc) * 0.3}
        if c.proj:
            o["Wp"], o["bp"] = _bf(rn(Cc, Cc) / Cc ** 0.5), rn(Cc) * 0.3
    if c.mod:
        nb = (M + c.T - 1) // c.T if c.mod == 2 else 1
        o["mod_ld"] = (c.mod_off + 2 * Cc + 12) if c.mod == 2 else 0
        o["mod_aff"] = rn(nb, c.mod_off + 2 * Cc + 12) * 0.5
    o = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in o.items()}
    o["mlp"] = c
    return o


def _mod_rows64(o):
    c = o["mlp"]
    aff = o["mod_aff"].double()
    b = (torch.arange(c.M, device=aff.device) // c.T) if c.mod == 2 else torch.zeros(c.M, dtype=torch.long, device=aff.device)
    return 1.0 + aff[b, c.mod_off:c.mod_off + c.C], aff[b, c.mod_off + c.C:c.mod_off + 2 * c.C]


def _spacing_t(x):
    return torch.from_numpy(P.bf16_spacing(x.cpu().numpy())).to(x.device)


def _bdist_t(x):
    return torch.from_numpy(P.boundary_distance(x.cpu().numpy())).to(x.device)


def mlp_expect(o):
    """float64 with the kernel's roundings restated (LayerNorm-2 -> bf16 with proj, hidden -> bf16): dict(x [M, C], bar [M, C], scale
    [, flag_ln, flag_h: fractions flagged; tight: the fraction of outputs with a bar below TIGHT scale]).  Dense cases: the flat bar
    of tests/test_bx_kernels.py; exact cases: the derived per-element bar."""
    c = o["mlp"]
    d = lambda k: o[k].double()
    x, W1, W2, b1, b2 = d("x"), d("W1"), d("W2"), d("b1"), d("b2")
    E1 = torch.zeros_like(x)
    if c.proj:
        x1 = x + d("in") @ d("Wp").t() + d("bp")
        ln = R.layer_norm(x1)
        xnr = _bf(ln.float()).double()
    else:
        x1, xnr = x, d("in")
    h = xnr @ W1.t() + b1
    g = R.gelu(h)
    hr = _bf(g.float()).double()
    v = hr @ W2.t() + b2 + x1
    pre = v
    if c.mod:
        sc1, sh = _mod_rows64(o)
        a = v * sc1 + sh
        v = R.silu(a)
    out = {"x": v, "scale": float(v.abs().max())}
    if not c.exact:
        out["bar"] = torch.full_like(v, (PROJMLP_BAR if c.proj else MLP_BAR) * out["scale"])
        return out
    W1a, W2a = W1.abs(), W2.abs()
    if c.proj:
        assert torch.equal(x1.float().double(), x1), "x1 is not exact in fp32: the operand grids are off"
        pert_ln = X.ln_elem_bound(x1) + U * ln.abs()
        flag_ln = _bdist_t(ln) <= pert_ln
        move_ln = torch.where(flag_ln, _spacing_t(ln) + pert_ln, torch.zeros_like(ln))
        m_h = move_ln @ W1a.t()
        Eh = 16 * U * (xnr.abs() @ W1a.t() + b1.abs())
        out["flag_ln"] = float(flag_ln.double().mean())
    else:
        assert torch.equal(h.float().double(), h), "fc1 is not exact in fp32: the operand grids are off"
        m_h, Eh = torch.zeros_like(h), torch.zeros_like(h)
        out["flag_ln"] = 0.0
    pert_h = 2 * (R.GELU_LIP * Eh + R.GELU_ABS + U * g.abs())
    flag_h = _bdist_t(g) <= pert_h
    dg = R.GELU_LIP * m_h
    # the kernel's g is within dg + pert_h / 2 of the reference's: the two round to the same bf16 value unless a boundary lies that close
    move_h = torch.where(_bdist_t(g) <= dg + pert_h, dg + pert_h + _spacing_t(g.abs() + dg + pert_h), torch.zeros_like(g))
    out["flag_h"] = float(flag_h.double().mean())
    Ev = 16 * U * (hr.abs() @ W2a.t() + b2.abs()) + E1 + U * pre.abs() + move_h @ W2a.t()
    if c.mod:
        Ea = sc1.abs() * Ev + 2 * U * (pre.abs() * sc1.abs() + sh.abs())
        Ev = R.SILU_LIP * Ea + (3 * R.HW_REL + 2 * U * a.abs()) * v.abs() + U * v.abs()
    out["bar"] = 2 * Ev
    out["tight"] = float((out["bar"] < TIGHT * out["scale"]).double().mean())
    return out


def mlp_buffers(o):
    """x (uint32 bits, [M + GUARD, C]: the rows of x, NaN guard rows) and xn_out (uint16, NaN) before the launch"""
    c = o["mlp"]
    xb = _nan_buf(c.M, c.C, np.uint32)
    xb[:c.M] = o["x"].cpu().numpy().view(np.uint32)
    return {"x": xb, "xn_out": _nan_buf(c.M, c.C, np.uint16) if c.out_mode else None}


def check_mlp(o, ref, init, got):
    """{check: worst |err| / bound} of one launch (bit-for-bit and untouched checks: 0 or inf)"""
    c = o["mlp"]
    M = c.M
    INF = float("inf")
    r = {"x guard": 0.0 if np.array_equal(init["x"][M:], got["x"][M:]) else INF}
    stored = got["x"][:M].view(np.float32)
    r["x"] = R.worst_ratio(torch.from_numpy(np.ascontiguousarray(stored)), ref["x"].cpu(), ref["bar"].cpu())
    if c.out_mode:
        r["xn_out guard"] = 0.0 if np.array_equal(init["xn_out"][M:], got["xn_out"][M:]) else INF
        gb = got["xn_out"][:M]
        if c.out_mode == 2:
            r["xn_out bits"] = 0.0 if np.array_equal(gb, P.bf16_rne_bits(stored)) else INF
        else:
            s64 = torch.from_numpy(np.nan_to_num(stored)).double()
            lr = R.layer_norm(s64)
            r["xn_out ln(stored)"] = _ratio(P.widen(gb), lr, P.with_bf16_store(lr, X.ln_elem_bound(s64)))
    return r


# ------------------------------------------------------------------------------------------------------------------------------
# NumPy emulation of the fused MLP kernels, with mistakes
# ------------------------------------------------------------------------------------------------------------------------------
MLP_MISTAKES = ("ln2_trunc", "hid_trunc", "xo_trunc", "hidden_chunk_dropped", "b1_neighbour_chunk", "bp_not_in_stats", "swap_row_blocks",
                "scale_no_1", "neighbour_sample", "mod_off_ignored")


def emulate_mlp(o, mistake=None):
    """the kernels' arithmetic in NumPy: proj in ascending 16-k steps, x1 = (acc + bp) + x, LayerNorm-2 from lane-local sums -> bf16;
    hidden chunks of 32 ascending: (b1 + fc1) -> GELU -> bf16 -> fc2 accumulation (which starts from x1 with proj); + b2 (+ x without
    proj); modulate; fp32 store; bf16 copy or LayerNorm of the stored row"""
    c = o["mlp"]
    M, Cc = c.M, c.C
    n = lambda k: o[k].cpu().numpy()
    x, W1, W2, b1, b2 = n("x"), n("W1"), n("W2"), n("b1"), n("b2")
    if c.proj:
        acc = _acc_steps(np.zeros((M, Cc), np.float32), n("in"), n("Wp"))
        x1 = ((acc + n("bp")[None, :]).astype(np.float32) + x).astype(np.float32)
        stats_of = ((acc + x).astype(np.float32)) if mistake == "bp_not_in_stats" else None
        xn = P.widen(_rne(_ln_rows(x1, stats_of=stats_of, width=Cc), mistake == "ln2_trunc"))
        oacc = x1
    else:
        xn, oacc = n("in"), np.zeros((M, Cc), np.float32)
    H = 4 * Cc
    for hc in range(H // 32):
        if mistake == "hidden_chunk_dropped" and hc == H // 64:
            continue
        sl = slice(32 * hc, 32 * hc + 32)
        bsl = slice(32 * (hc ^ 1), 32 * (hc ^ 1) + 32) if mistake == "b1_neighbour_chunk" else sl
        hacc = _acc_steps(np.repeat(b1[None, bsl], M, 0).astype(np.float32), xn, W1[sl])
        gq = P.widen(_rne(_r32(P._gelu64(hacc.astype(np.float64))), mistake == "hid_trunc"))
        oacc = _acc_steps(oacc, gq, W2[:, sl])
    v = (oacc + b2[None, :]).astype(np.float32)
    if not c.proj:
        v = (v + x).astype(np.float32)
    if c.mod:
        v = _modulate(v, n("mod_aff"), c.mod, c.mod_off, c.T, Cc, mistake)
    out = mlp_buffers(o)
    xo = None
    if c.out_mode:
        xo = _rne(v if c.out_mode == 2 else _ln_rows(v, width=Cc), mistake == "xo_trunc")
    if mistake == "swap_row_blocks" and M >= 64:
        v = v.copy()
        v[0:32], v[32:64] = v[32:64].copy(), v[0:32].copy()
    out["x"][:M] = v.view(np.uint32)
    if c.out_mode:
        out["xn_out"][:M] = xo
    return out
