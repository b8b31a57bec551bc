"""Float64 references, bars and operand builders for the fp32 forward's edge and row kernels (csrc/kernels.hip: the fused PatchEmbed and
read-out, the one-wave-per-row passes, merge_norm_runs, the pure-window copies, the unfused assemble / pool / head tails), shared by
tests/test_edge_kernels.py (GPU: the kernels against these) and tests/test_edge_kernels_host.py (CPU: the power of these checks).
Same rules as tests/f32_ref.py: every formula is written once and evaluated in float64 and in float32 torch, and no bar is built from a
kernel's output.

Bars:
  * formula kernels (PatchEmbed, read-out's adjacency output, ln_mod, merge_ln, breakup_ln, mod_stats' rows, pool, head_adj, head_node):
    f32_ref.formula_bar -- 8 x the error of the float32 torch evaluation of the same formula, at most FWD_RTOL of the output scale.
    The read-out's float32 evaluation is the kernel's chain (two folded products on the fp32 fold), its float64 reference the unfolded one.
  * (mean, rstd) of a row of C values held in registers, two passes, u = 2^-24:
      mean = sum / C          |d mean| <= (C + 8) u mean|x|            (summation in any order, the division; 8 as in f32_ref)
      d_k = x_k - mean        error |d mean| + u |d_k|
      var = sum d_k^2 / C     |d var|  <= (C + 8) u var + 2 |d mean| mean|d|   (sum of non-negative terms; the second term is the
                                          first-order effect of the mean's error and of the rounded differences)
      rstd = rsq(var + eps)   |d rstd| / rstd <= d var / (2 (var + eps)) + 2^-23 (1-ulp hardware rsq) + 2 u (the add, the store)
    times the factor 2 of f32_ref for the roundings not modelled one by one.
  * a normalised element n = d rstd gamma + beta: |d n| <= rstd |gamma| (|d mean| + |d| (d rstd / rstd + 3 u)) + u |n|
  * pool_ext[r, c < 96] = (1 / N) sum_j valid n_j: the elements' errors averaged, plus (N + 8) u (1 / N) sum_j valid |n_j| for the
    product with the rounded 1 / N and the summation over the row's tiles and slots in any order; times 2.  Column 96 is f_i cnt / N: the quotient,
    or the product with a rounded 1 / N -- two roundings, 2 u relative, times 2; columns 97 .. 127 are exact zeros.
  * merge_norm_runs: the "LayerNorm from partial sums" bound of f32_ref's header (f32_ref._ln_terms) on fmaf(x, rstd, -mean rstd).
  * copies (broadcast, harvest, assemble): bit for bit."""
import numpy as np
import torch

import f32_ref as R
from f32_ref import U, LN_EPS, HW_REL, C_EXTRA, gelu, silu, layer_norm

E = 96


# ------------------------------------------------------------------------------------------------------------------------------
# flags
# ------------------------------------------------------------------------------------------------------------------------------
FLAG_PATTERNS = ("all", "prefix", "scattered")


def make_flags(B, N, pattern, seed=0):
    """uint8 [B, N].  prefix: graph b has its first len_b nodes valid, len = (ceil(N/2), 0, 1, N, N-1)[b % 5] -- from B = 3 on a graph
    with no valid node and one with a single one; scattered: each node valid with probability 0.6, at least one in the batch"""
    f = np.zeros((B, N), np.uint8)
    if pattern == "all":
        f[:] = 1
    elif pattern == "prefix":
        lens = ((N + 1) // 2, 0, 1, N, max(N - 1, 1))
        for b in range(B):
            f[b, :lens[b % 5]] = 1
    else:
        rng = np.random.RandomState(77 + seed)
        f[:] = rng.rand(B, N) < 0.6
        if not f.any():
            f[0, 0] = 1
    return f


def pair_valid(flags):
    """bool [B, N, N]: f_i & f_j"""
    f = torch.as_tensor(flags).bool()
    return f[:, :, None] & f[:, None, :]


def wave_classes(flags):
    """what the 32-token waves of the fused C = 96 kernels see: (shortcut, mixed, met) -- the number of waves that hold tokens but no
    valid pair (the read-out's all-masked shortcut), of waves that hold a valid and a masked token of the SAME node row (b, i), and of
    node rows with a valid pair whose tiles are served partly by a shortcut wave and partly by a computing one"""
    B, N = flags.shape
    v = pair_valid(flags).reshape(-1).numpy()
    M = B * N * N
    row = np.arange(M) // N
    shortcut = mixed = 0
    short_tiles = set()
    for t in range((M + 31) // 32):
        sl = slice(32 * t, min(32 * t + 32, M))
        if not v[sl].any():
            shortcut += 1
            short_tiles.add(t)
        else:
            for r in np.unique(row[sl]):
                sel = v[sl][row[sl] == r]
                if sel.any() and not sel.all():
                    mixed += 1
                    break
    met = 0
    for r in range(B * N):
        if v[r * N:(r + 1) * N].any():
            tiles = range((r * N) // 32, (r * N + N - 1) // 32 + 1)
            if any(t in short_tiles for t in tiles):
                met += 1
    return shortcut, mixed, met


# ------------------------------------------------------------------------------------------------------------------------------
# row statistics and LayerNorm: formulas and per-element bounds
# ------------------------------------------------------------------------------------------------------------------------------
def row_stats(x):
    """(mean, rstd) [M, 2] of the rows of x in x's dtype, two passes"""
    mu = x.mean(1, keepdim=True)
    var = (x - mu).pow(2).mean(1)
    return torch.stack([mu[:, 0], (var + LN_EPS) ** -0.5], 1)


def row_stats_bound(x64):
    """per-element bound [M, 2] on a two-pass fp32 (mean, rstd) of the rows of x64 (float64 values of fp32 data), and the pieces the
    element bound below needs"""
    Cc = x64.shape[1]
    mu = x64.mean(1, keepdim=True)
    d = x64 - mu
    var = d.pow(2).mean(1)
    rstd = (var + LN_EPS) ** -0.5
    dmean = (Cc + C_EXTRA) * U * x64.abs().mean(1)
    dvar = (Cc + C_EXTRA) * U * var + 2 * dmean * d.abs().mean(1)
    drel = 0.5 * dvar / (var + LN_EPS) + HW_REL + 2 * U
    return torch.stack([2 * dmean, 2 * rstd * drel], 1), (d, rstd, dmean, drel)


def ln_elem_bound(x64, gam=None):
    """per-element bound [M, C] on a fp32 LayerNorm (d rstd gamma + beta) of the rows of x64"""
    _, (d, rstd, dmean, drel) = row_stats_bound(x64)
    g = torch.ones(x64.shape[1], dtype=torch.float64) if gam is None else gam.double().abs()
    n = d * rstd[:, None] * g
    return 2 * (rstd[:, None] * g * (dmean[:, None] + d.abs() * (drel[:, None] + 3 * U)) + U * n.abs())


def aff_rows(aff, off, Cc, T, M, neighbour_row=None):
    """(1 + scale, shift) [M, C] per row from the per-sample table aff [B, ld]; neighbour_row: that row takes the next sample's (a
    host-test mutation)"""
    b = torch.arange(M) // T
    if neighbour_row is not None:
        b[neighbour_row] = b[neighbour_row] + (1 if b[neighbour_row] + 1 < aff.shape[0] else -1)
    return 1.0 + aff[b, off:off + Cc], aff[b, off + Cc:off + 2 * Cc]


def modulate(x, aff, off, T, neighbour_row=None):
    sc1, sh = aff_rows(aff, off, x.shape[1], T, x.shape[0], neighbour_row)
    return silu(sh + x * sc1)


def ln_mod_formula(x, gam, bet, aff, off, T, neighbour_row=None):
    return modulate(layer_norm(x, gam, bet), aff, off, T, neighbour_row)


def merge_gather(x, B, res, swap=False):
    """[B res^2, C] -> [B (res/2)^2, 4C]: cat[x(2i,2j), x(2i+1,2j), x(2i,2j+1), x(2i+1,2j+1)]; swap: parts x10 / x01 exchanged"""
    v = x.view(B, res, res, -1)
    parts = [v[:, 0::2, 0::2], v[:, 1::2, 0::2], v[:, 0::2, 1::2], v[:, 1::2, 1::2]]
    if swap:
        parts[1], parts[2] = parts[2], parts[1]
    return torch.cat(parts, -1).reshape(B * (res // 2) ** 2, -1)


def merge_ln_formula(x, gam, bet, B, res, swap=False):
    return layer_norm(merge_gather(x, B, res, swap), gam, bet)


def breakup_formula(y, gam, bet, pg, pb, B, res, swap=False):
    """[B res^2, D] -> [B (2 res)^2, D/4]: LN_D, chunk q -> token (2i + (q & 1), 2j + (q >> 1)), LN_{D/4}; swap: di / dj exchanged"""
    D = y.shape[1]
    Co = D // 4
    n = layer_norm(y, gam, bet).view(B, res, res, 4, Co)
    z = torch.zeros(B, 2 * res, 2 * res, Co, dtype=y.dtype)
    for q in range(4):
        di, dj = (q & 1, q >> 1) if not swap else (q >> 1, q & 1)
        z[:, di::2, dj::2] = layer_norm(n[:, :, :, q].reshape(-1, Co), pg, pb).view(B, res, res, Co)
    return z.view(B * 4 * res * res, Co)


def breakup_rows(B, res, runs):
    """bool [B (2 res)^2]: the fine rows the listed coarse runs (8 coarse rows each) write"""
    m = torch.zeros(B, 2 * res, 2 * res, dtype=torch.bool)
    for r in runs:
        for c in range(8 * r, 8 * r + 8):
            b, t = divmod(c, res * res)
            i, j = divmod(t, res)
            m[b, 2 * i:2 * i + 2, 2 * j:2 * j + 2] = True
    return m.view(-1)


def merge_norm_case(B, res, Cc, gen):
    """the fine activation, its (sum, sumsq) partials as a producing kernel stores them, and the GEMM-case record f32_ref's bound reads"""
    x = torch.randn(B * res * res, Cc, generator=gen) + 2.0 * (2.0 * torch.rand(B * res * res, 1, generator=gen) - 1.0)
    o = {"case": R.GemmCase(B * (res // 2) ** 2, 1, 4 * Cc, ln="part", a4_res=res, B=B), "A": x, "ln_part": R._partials(x.double())}
    return x, o


def merge_norm_expect(o, dtype=torch.float64):
    """fmaf(x, rstd, -mean rstd) on the gathered row, statistics from the four fine rows' partials; with float64 also the bound"""
    A = R.logical_A(o).to(dtype)
    mean, rstd, drstd, dmean = R._ln_terms(o, dtype)
    y = (A - mean[:, None]) * rstd[:, None]
    if dtype != torch.float64:
        return y, None
    env = (A.abs() + mean.abs()[:, None]) * rstd[:, None]
    return y, 2 * (R.C_LN * U * env + drstd[:, None] * y.abs() + (dmean * rstd)[:, None] + U * y.abs())


# ------------------------------------------------------------------------------------------------------------------------------
# PatchEmbed
# ------------------------------------------------------------------------------------------------------------------------------
def pe_kp(Ca, Cn, self_cond):
    return ((2 if self_cond else 1) * (Ca + 2 * Cn) + 31) // 32 * 32


def make_pe_inputs(B, N, Ca, Cn, gen):
    """fp32 adjacency [B, Ca, N, N] and node [B, N, Cn] tensors and their self-condition copies; NOT symmetric in (i, j)"""
    rn = lambda *s: torch.randn(*s, generator=gen)
    return dict(adj=rn(B, Ca, N, N), node=rn(B, N, Cn), sc_adj=rn(B, Ca, N, N), sc_node=rn(B, N, Cn))


def pe_input(t, flags, self_cond, sc_on, dtype=torch.float64, unmasked=False, swap_ij=False):
    """the gathered input [B N^2, in_chans]: [sc_adj, adj, sc_node(i), node(i), sc_node(j), node(j)] (without self-conditioning: [adj,
    node(i), node(j)]); node parts times f_i & f_j; self-condition parts zero when sc_on is false.
    unmasked / swap_ij: host-test mutations (the node part left unmasked; the node(i) and node(j) halves exchanged)"""
    adj, node = t["adj"].to(dtype), t["node"].to(dtype)
    B, Ca, N, _ = adj.shape
    Cn = node.shape[2]
    v = pair_valid(flags)[..., None] if not unmasked else torch.ones(B, N, N, 1, dtype=torch.bool)
    zero = torch.zeros((), dtype=dtype)     # a select, as in the kernels: a masked value is +0, never -0
    sca = t["sc_adj"].to(dtype) if sc_on else torch.zeros_like(adj)
    scn = t["sc_node"].to(dtype) if sc_on else torch.zeros_like(node)
    a_parts = ([sca.permute(0, 2, 3, 1)] if self_cond else []) + [adj.permute(0, 2, 3, 1)]
    ni = lambda n: torch.where(v, n[:, :, None, :].expand(B, N, N, Cn), zero)
    nj = lambda n: torch.where(v, n[:, None, :, :].expand(B, N, N, Cn), zero)
    first, second = (ni, nj) if not swap_ij else (nj, ni)
    n_parts = ([first(scn)] if self_cond else []) + [first(node)] + ([second(scn)] if self_cond else []) + [second(node)]
    return torch.cat(a_parts + n_parts, -1).reshape(B * N * N, -1)


def make_pe_params(cin, B, gen, aff_off=8, gap=12):
    """Wpe [96, cin], bias, gamma, beta and the per-sample (scale | shift) table with two rows' worth of offsets: aff_off != 0, a second
    block at aff_off2, aff_ld > aff_off2 + 2 * 96"""
    rn = lambda *s: torch.randn(*s, generator=gen)
    aff_off2 = aff_off + 2 * E + gap
    aff_ld = aff_off2 + 2 * E + 4
    return dict(W=rn(E, cin) / cin ** 0.5, bias=rn(E) * 0.3, gam=1.0 + 0.2 * rn(E), bet=0.2 * rn(E), aff=rn(B, aff_ld) * 0.5,
                aff_ld=aff_ld, aff_off=aff_off, aff_off2=aff_off2)


def pe_formula(inp, p, T, second, dtype=torch.float64, neighbour_row=None):
    """Wpe in + bias -> LayerNorm_96 -> silu(shift + n (1 + scale)) per sample, and the second modulate + SiLU when `second`"""
    c = lambda k: p[k].to(dtype)
    y = inp @ c("W").t() + c("bias")
    o = ln_mod_formula(y, c("gam"), c("bet"), c("aff"), p["aff_off"], T, neighbour_row)
    return modulate(o, c("aff"), p["aff_off2"], T, neighbour_row) if second else o


def pad_k(W, Kp):
    out = torch.zeros(W.shape[0], Kp, dtype=W.dtype)
    out[:, :W.shape[1]] = W
    return out


def runs_rows(M, runs):
    m = torch.zeros(M, dtype=torch.bool)
    for r in runs:
        m[8 * r:8 * r + 8] = True
    return m


# ------------------------------------------------------------------------------------------------------------------------------
# read-out
# ------------------------------------------------------------------------------------------------------------------------------
def readout_segments(N):
    """pool_part slots per node row: the most 32-token tiles a row of N tokens can touch (readout_pool_segments of csrc/kernels.hip)"""
    return (N + 30) // 32 + 1


def make_readout_params(Ca, gen):
    """the unfolded parameters, fp32: read_out.0 as a ConvTranspose2d weight [in, out], read_out.1 / .2 and the heads' linears [out, in]"""
    rn = lambda *s: torch.randn(*s, generator=gen)
    sq = E ** -0.5
    return dict(W0=rn(E, E) * sq, b0=rn(E) * 0.2, W1=rn(E, E) * sq, b1=rn(E) * 0.2, W2=rn(E, E) * sq, b2=rn(E) * 0.2, F1=rn(E, E) * sq, f1=rn(E) * 0.2,
                F2=rn(Ca, E) * sq, f2=rn(Ca) * 0.2, G1=rn(E, E) * sq, gam=1.0 + 0.2 * rn(E), bet=0.2 * rn(E))


def fold_readout(p):
    """a transcription of the folding block of dsg_finalize_weights, in float64: A = W2 W1 W0^T, a = W2 (W1 b0 + b1) + b2, Fa = F1 A,
    fa = F1 a + f1, Gn = G1 A, ga = G1 a"""
    d = {k: v.double() for k, v in p.items()}
    A = d["W2"] @ (d["W1"] @ d["W0"].t())
    a = d["W2"] @ (d["W1"] @ d["b0"] + d["b1"]) + d["b2"]
    return dict(Fa=d["F1"] @ A, fa=d["F1"] @ a + d["f1"], Gn=d["G1"] @ A, ga=d["G1"] @ a)


def readout_shared(xn, p):
    """the reference's chain up to the shared representation, in xn's dtype: s = W2 (W1 (W0^T xn + b0) + b1) + b2"""
    c = lambda k: p[k].to(xn.dtype)
    s = xn @ c("W0") + c("b0")
    s = s @ c("W1").t() + c("b1")
    return s @ c("W2").t() + c("b2")


def adj_layout(o, valid, B, N):
    """token-major [B N^2, Ca] -> the output tensor [B, Ca, N, N], zero where !(f_i & f_j)"""
    return (o.view(B, N, N, -1) * valid[..., None].to(o.dtype)).permute(0, 3, 1, 2).contiguous()


def readout_pool(xn, flags, wgt=None, div=None):
    """pool_ext [B N, 128] from LN(x) [B N^2, 96] in xn's dtype: columns 0 .. 95 = (1 / N) sum_j valid xn[b, i, j], column 96 =
    f_i (#valid in b) / N, the rest zero.  wgt [B N, N] / div: other weights or another divisor (host-test mutations)"""
    B, N = flags.shape
    f = torch.as_tensor(flags).bool()
    wg = (pair_valid(flags).reshape(B * N, N) if wgt is None else wgt).to(xn.dtype)
    pe = torch.zeros(B * N, 128, dtype=xn.dtype)
    s = (xn.view(B * N, N, E) * wg[..., None]).sum(1)
    pe[:, :E] = s / (N if div is None else div)
    cnt = f.sum(1, keepdim=True).expand(B, N).reshape(-1).to(xn.dtype)
    pe[:, E] = f.reshape(-1).to(xn.dtype) * cnt / N
    return pe


def readout_expect(x, p, flags, transposed=False):
    """x [B N^2, 96] fp32 (finite everywhere; the GPU test overwrites the masked tokens' rows with NaN afterwards).  Returns a dict:
    out64 (the unfolded chain in float64), out32 (the two folded products in float32 on the fp32 fold), pool64 / pool32 [B N, 128] and
    pool_bound (per element), node64 = G1 (pooled s) and the fp32 fold itself.  transposed: the (i, j)-transposed output (a mutation)"""
    B, N = flags.shape
    valid = pair_valid(flags)
    x64 = x.double()
    xn64 = layer_norm(x64, p["gam"].double(), p["bet"].double())
    s64 = readout_shared(xn64, p)
    o64 = gelu(s64 @ p["F1"].double().t() + p["f1"].double()) @ p["F2"].double().t() + p["f2"].double()
    fold = fold_readout(p)
    f32 = {k: v.float() for k, v in fold.items()}
    xn32 = layer_norm(x, p["gam"], p["bet"])
    o32 = gelu(xn32 @ f32["Fa"].t() + f32["fa"]) @ p["F2"].t() + p["f2"]
    out = dict(out64=adj_layout(o64, valid, B, N), out32=adj_layout(o32, valid, B, N), fold32=f32, fold64=fold)
    if transposed:
        out["out64"] = out["out64"].transpose(2, 3).contiguous()
    w = valid.reshape(B * N, N)
    out["xn64"] = xn64
    out["pool64"], out["pool32"] = readout_pool(xn64, flags), readout_pool(xn32, flags)
    dn = ln_elem_bound(x64, p["gam"]).view(B * N, N, E)
    wd = w.double()[..., None]
    bound = torch.zeros(B * N, 128, dtype=torch.float64)
    bound[:, :E] = 2 * ((dn * wd).sum(1) / N + (N + C_EXTRA) * U * (xn64.view(B * N, N, E).abs() * wd).sum(1) / N)
    bound[:, E] = 2 * 2 * U * out["pool64"][:, E].abs()
    out["pool_bound"] = bound
    # the node head's input from the unfolded chain: G1 . ((1/N) sum_j valid s) for flagged i (the fold's cross-check)
    ps = (s64.view(B * N, N, E) * wd).sum(1) / N
    out["node64"] = ps @ p["G1"].double().t()
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the unfused tails
# ------------------------------------------------------------------------------------------------------------------------------
def head_adj_formula(h, W, bias, flags):
    B, N = flags.shape
    return adj_layout(h @ W.t() + bias, pair_valid(flags), B, N)


def pool_formula(rep, flags, ignore_flags=False, by_count=False):
    """[B N^2, E] -> [B N, E]: (1/N) sum_j f_i f_j rep; the mutations: the sum over every j, the division by the valid count"""
    B, N = flags.shape
    v = pair_valid(flags).to(rep.dtype)
    f = torch.as_tensor(flags).to(rep.dtype)
    w = f[:, :, None].expand(B, N, N) if ignore_flags else v
    s = (rep.view(B, N, N, -1) * w[..., None]).sum(2)
    div = f.sum(1).clamp(min=1)[:, None, None] if by_count else N
    return (s / div).reshape(B * N, -1)


def head_node_formula(h, W, bias, flags):
    return (h @ W.t() + bias) * torch.as_tensor(flags).reshape(-1, 1).to(h.dtype)


# ------------------------------------------------------------------------------------------------------------------------------
# pure-window copies, by index
# ------------------------------------------------------------------------------------------------------------------------------
def window_rows(res, w):
    """the 64 token indices of 8 x 8 window w of a res x res grid, in window order t = 8 row + col"""
    nwr = res // 8
    i0, j0 = 8 * (w // nwr), 8 * (w % nwr)
    return np.array([(i0 + t // 8) * res + j0 + t % 8 for t in range(64)])


def broadcast_expect(bufs, B, res, copy_list, cnt, rep):
    """representative mode on numpy arrays [B res^2, width] (modified copies are returned): every listed window in [0, B nW) whose graph
    has a representative in range other than itself takes that window's rows"""
    nW, T = (res // 8) ** 2, res * res
    out = [None if a is None else a.copy() for a in bufs]
    for dst in copy_list[:cnt]:
        if dst < 0 or dst >= B * nW:
            continue
        src = rep[dst // nW]
        if src < 0 or src >= B * nW or src == dst:
            continue
        d = (dst // nW) * T + window_rows(res, dst % nW)
        s = (src // nW) * T + window_rows(res, src % nW)
        for a, o in zip(bufs, out):
            if a is not None:
                o[d] = a[s]
    return out


def table_entry(table, idx, off, width):
    """[64, width] view of one part of table entry idx (table [entries, stride] numpy)"""
    return table[idx, off:off + 64 * width].reshape(64, width)


def broadcast_table_expect(bufs, B, res, copy_list, cnt, table, idx, offs, widths):
    nW, T = (res // 8) ** 2, res * res
    out = [None if a is None else a.copy() for a in bufs]
    for dst in copy_list[:cnt]:
        if dst < 0 or dst >= B * nW:
            continue
        d = (dst // nW) * T + window_rows(res, dst % nW)
        for o, off, wd in zip(out, offs, widths):
            if o is not None:
                o[d] = table_entry(table, idx, off, wd)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the committed case lists (shared with the host tests, which check what they reach)
# ------------------------------------------------------------------------------------------------------------------------------
READOUT_CASES = [(129, 1, 1), (1, 1, 3), (3, 5, 3), (2, 8, 6), (5, 20, 3), (1, 33, 6), (1, 34, 1), (2, 40, 3), (1, 64, 6), (2, 8, 32)]
PE_CONFIGS = [(6, 12, 1), (3, 12, 1), (3, 5, 1), (2, 12, 1), (6, 12, 0), (4, 6, 1), (8, 12, 1)]
PE_GRIDS = [(129, 1), (3, 5), (2, 8), (2, 20), (1, 33)]
PE_LIST_CONFIGS = [(6, 12, 1), (3, 12, 1), (3, 5, 1), (2, 12, 1)]     # the four instantiations
ROW_C = (96, 128, 192, 384, 768)
ROW_BT = ((1, 1), (3, 1), (2, 2), (5, 1), (3, 3))                    # M = 1, 3, 4, 5, 9: a sample boundary inside a block of four rows
BREAKUP_D = (384, 512, 768, 1536)
