"""numpy restatements of the edges of the training form at patch_size p > 1 (csrc/train_kernels_patch.hip): the pack /
unpack of PatchEmbed's and read_out.0's weights, the masked adjacency store pair, the node pooling and its backward, the live columns
of PatchEmbed's weight image and the assembly backward.  Every function computes in the dtype of its float inputs (float64 for the
reference, float32 for f32_ref.formula_bar's second evaluation).  No GPU, no torch: imported by GPU and host tests alike.

Token t = ti R + tj (R = N / p) covers the pixels (I, J) = (p ti + a, p tj + b); rows "in (token, a, b) order" have
m = (graph R^2 + t) p^2 + a p + b.  `mut` switches on one deliberate mistake (MUTATIONS) for the tests of the power of the bars."""
import numpy as np

MUTATIONS = ("pe_swap_ab", "ro_swap_ab", "ro_out_in", "token_mask", "mean_over_R", "row_only")


def row_pixels(B, N, p):
    """(graph, I, J) of every row m in (token, a, b) order: three int arrays [B N N]"""
    R, pp = N // p, p * p
    m = np.arange(B * N * N)
    sub, tok = m % pp, m // pp
    t, g = tok % (R * R), tok // (R * R)
    return g, p * (t // R) + sub // p, p * (t % R) + sub % p


def pixel_valid(flags, p, mut=None):
    """[B, N, N] bool: flag_I && flag_J (mut 'token_mask': the flags of the token's first pixel instead)"""
    f = flags.astype(bool)
    if mut == "token_mask":
        f = np.repeat(f[:, ::p], p, axis=1)
    return f[:, :, None] & f[:, None, :]


# ---- PatchEmbed: W [E, Cin, p, p] <-> image [E, Kp], column (a p + b) Cin + c ----
def pe_pack(W, Kp):
    E, Cin, p, _ = W.shape
    img = np.zeros((E, Kp), W.dtype)
    img[:, :p * p * Cin] = W.transpose(0, 2, 3, 1).reshape(E, p * p * Cin)
    return img


def pe_unpack(img, Cin, p, mut=None):
    E = img.shape[0]
    W = img[:, :p * p * Cin].reshape(E, p, p, Cin).transpose(0, 3, 1, 2)
    return np.ascontiguousarray(W.transpose(0, 1, 3, 2) if mut == "pe_swap_ab" else W)


def image_to_tok(x, p, Kp):
    """the assembled image [B, Cin, N, N] as PatchEmbed's input rows [B R^2, Kp] (launch_assemble_patch's layout)"""
    B, Cin, N, _ = x.shape
    R = N // p
    tok = np.zeros((B * R * R, Kp), x.dtype)
    tok[:, :p * p * Cin] = x.reshape(B, Cin, R, p, R, p).transpose(0, 2, 4, 3, 5, 1).reshape(B * R * R, p * p * Cin)
    return tok


def tokens_rows(y):
    """a [B, E, R, R] map as token rows [B R^2, E]"""
    B, E, R, _ = y.shape
    return y.transpose(0, 2, 3, 1).reshape(B * R * R, E)


# ---- read_out.0: W [in, out, p, p] <-> image [in, p^2 out], column (a p + b) out + o ----
def ro0_pack(W, bias):
    Ei, Eo, p, _ = W.shape
    return np.ascontiguousarray(W.transpose(0, 2, 3, 1).reshape(Ei, p * p * Eo)), np.tile(bias, p * p)


def ro0_unpack(img, Eo, p, mut=None):
    Ei = img.shape[0]
    W = img.reshape(Ei, p, p, Eo).transpose(0, 3, 1, 2)
    if mut == "ro_swap_ab":
        W = W.transpose(0, 1, 3, 2)
    if mut == "ro_out_in":
        W = W.transpose(1, 0, 2, 3)
    return np.ascontiguousarray(W)


def pixels_rows(z, p):
    """a [B, E, N, N] map as rows in (token, a, b) order [B N N, E]"""
    B, E, N, _ = z.shape
    g, I, J = row_pixels(B, N, p)
    return z[g, :, I, J]


# ---- the masked adjacency store and its transpose ----
def adj_store(oa, flags, p, mut=None):
    """F [B, Ca, N, N] from oa [B N N, Ca] in (token, a, b) order, exact zeros at masked pixels"""
    B, N = flags.shape
    g, I, J = row_pixels(B, N, p)
    ok = pixel_valid(flags, p, mut)[g, I, J]
    F = np.zeros((B, oa.shape[1], N, N), oa.dtype)
    F[g, :, I, J] = np.where(ok[:, None], oa, 0)
    return F


def adj_store_bwd(dF, flags, p, mut=None):
    B, N = flags.shape
    g, I, J = row_pixels(B, N, p)
    ok = pixel_valid(flags, p, mut)[g, I, J]
    return np.where(ok[:, None], dF[g, :, I, J], 0).astype(dF.dtype)


# ---- node pooling and its backward ----
def pool(rep, flags, p):
    """pool [B, N, E] = (1/N) sum_J valid(I, J) rep[row(I, J)]"""
    B, N = flags.shape
    g, I, J = row_pixels(B, N, p)
    ok = pixel_valid(flags, p)[g, I, J]
    out = np.zeros((B, N, rep.shape[1]), rep.dtype)
    np.add.at(out, (g, I), np.where(ok[:, None], rep, 0))
    return out / rep.dtype.type(N)


def pool_bwd(d_pool, flags, p, mut=None):
    """the term the kernel adds to d_rep [B N N, E]: valid(I, J) d_pool[(b, I)] / N (mut 'mean_over_R': / R)"""
    B, N = flags.shape
    g, I, J = row_pixels(B, N, p)
    ok = pixel_valid(flags, p, mut)[g, I, J]
    div = d_pool.dtype.type(N // p if mut == "mean_over_R" else N)
    return np.where(ok[:, None], d_pool[g, I] / div, 0).astype(d_pool.dtype)


# ---- input gradients: live columns and the assembly backward ----
def live_slots(c_adj, c_node, self_cond):
    """source channel (assemble_kernel's order) of the G = c_adj + 2 c_node live slots (adj | node of the row | node of the column)"""
    nsc, sc = (2, 1) if self_cond else (1, 0)
    return np.concatenate([sc * c_adj + np.arange(c_adj), nsc * c_adj + sc * c_node + np.arange(c_node),
                           nsc * c_adj + nsc * c_node + sc * c_node + np.arange(c_node)])


def live_width(c_adj, c_node, p):
    return (p * p * (c_adj + 2 * c_node) + 31) // 32 * 32


def live_cols(W, c_adj, c_node, self_cond):
    """img [E, Np]: column (a p + b) G + slot = W[e, src(slot), a, b], zeros behind p^2 G"""
    E, _, p, _ = W.shape
    src = live_slots(c_adj, c_node, self_cond)
    img = np.zeros((E, live_width(c_adj, c_node, p)), W.dtype)
    img[:, :p * p * len(src)] = W[:, src].transpose(0, 2, 3, 1).reshape(E, p * p * len(src))
    return img


def assemble_live(adj, node, flags, p, ld):
    """the forward whose transpose assemble_bwd is (c_skip = 0, c_in = 1): the live columns [B R^2, ld] of PatchEmbed's input rows from
    the current adjacency [B, Ca, N, N] and node values [B, N, Cn] -- the adjacency unmasked, the node parts masked per pixel"""
    B, Ca, N, _ = adj.shape
    Cn, R, G = node.shape[2], N // p, adj.shape[1] + 2 * node.shape[2]
    ok = pixel_valid(flags, p)[:, None].astype(adj.dtype)
    nd = np.where(flags.astype(bool)[:, :, None], node, 0)
    row = np.broadcast_to(nd.transpose(0, 2, 1)[:, :, :, None], (B, Cn, N, N)) * ok
    col = np.broadcast_to(nd.transpose(0, 2, 1)[:, :, None, :], (B, Cn, N, N)) * ok
    return image_to_tok(np.concatenate([adj, row, col], 1), p, ld)


def assemble_bwd(d_tok, flags, c_skip, c_in, g_adj, g_node, p, mut=None):
    """(out_adj, out_node, |terms| adj, |terms| node): d_tok [B R^2, ld] with p^2 groups of G per token; the last two are the sums of
    the absolute values of the added terms, for closed-form bars"""
    B, N = flags.shape
    Ca, Cn = g_adj.shape[1], g_node.shape[2]
    R, G, dt = N // p, g_adj.shape[1] + 2 * g_node.shape[2], d_tok.dtype
    d = d_tok[:, :p * p * G].reshape(B, R, R, p, p, G).transpose(0, 1, 3, 2, 4, 5).reshape(B, N, N, G)   # [b, I, J, slot]
    f = flags.astype(bool)
    ok = pixel_valid(flags, p, mut)
    cs, ci = c_skip.astype(dt), c_in.astype(dt)
    t_skip = np.where(ok[:, None], cs[:, None, None, None] * g_adj.astype(dt), 0)
    t_tok = ci[:, None, None, None] * d[..., :Ca].transpose(0, 3, 1, 2)
    w = ok[..., None]
    row = np.where(w, d[..., Ca:Ca + Cn], 0)                              # [b, I, J, c]: pixel (I, J)
    col = np.where(w, d[..., Ca + Cn:].transpose(0, 2, 1, 3), 0)          # [b, I, J, c]: pixel (J, I)
    s = row.sum(2) if mut == "row_only" else row.sum(2) + col.sum(2)
    t_g = np.where(f[:, :, None], cs[:, None, None] * g_node.astype(dt), 0)
    out_node = np.where(f[:, :, None], t_g + ci[:, None, None] * s, 0)
    abs_node = np.abs(t_g) + ci[:, None, None] * (np.abs(row).sum(2) + np.abs(col).sum(2))
    return t_skip + t_tok, out_node, np.abs(t_skip) + np.abs(t_tok), abs_node


def make_flags(B, N, kind):
    """'all'; 'odd': an odd valid count per graph, so that one token has a single valid pixel row; 'one': graph 0 has a single valid node"""
    flags = np.zeros((B, N), np.uint8)
    for b in range(B):
        n = N if kind == "all" else (1 if (kind == "one" and b == 0) else max(1, (N * (b + 1)) // (B + 1)) | 1)
        flags[b, :min(n, N)] = 1
    return flags
