"""The patch_size p > 1 arithmetic of the reference (include/dsg.h: dsg_create_patch), written once and evaluated in float64
and in float32 torch; shared by tests/test_patch_host.py (CPU: the formulas against the reference's recorded intermediates, and the power
of the checks), tests/test_patch_kernels.py (GPU: the new kernels against these) and tests/test_patch.py.  Rules of tests/edge_ref.py:
bars are f32_ref.formula_bar (8 x the float32 evaluation's error, at most FWD_RTOL of the output scale); copies and index maps are
compared bit for bit; no bar is built from a kernel's output.

Notation: R = N / p, token t = ti R + tj, pixel (I, J) = (p ti + a, p tj + b), valid(I, J) = flag_I & flag_J.
  PatchEmbed   y[t, e] = bias[e] + sum_{c,a,b} W[e, c, a, b] img[c, p ti + a, p tj + b]   (W [E, Cin, p, p]; img masked per PIXEL)
  read_out.0   r0[(I, J), o] = b0[o] + sum_i LN(x)[t, i] W0[i, o, a, b]                  (ConvTranspose2d weight [in, out, p, p])
  node head    node_feat[I] = (1/N) sum_J valid(I, J) rep[(I, J)]                        (mean over N pixels, mask per pixel)
  pooled fold  node_feat[I] = flag_I sum_b (F[I mod p, b] s[I, b] + c cnt_b / N),  A = R2 R1, F[a, b] = A W0[:, :, a, b]^T,
               c = A b0 + R2 b1 + b2, s[I, b] = (1/N) sum_tj flag_{p tj + b} LN(x)[I // p, tj], cnt_b = #valid columns = b mod p
Mutations (keyword `mut`) are the mistakes tests/test_patch_host.py shows the bars to catch."""
import numpy as np
import torch

import edge_ref as X
from f32_ref import gelu, silu, layer_norm

MUTATIONS = ("pe_swap_ab", "ro_swap_ab", "ro_out_in", "token_mask", "mean_over_R", "cnt_total")


# ------------------------------------------------------------------------------------------------------------------------------
# index maps
# ------------------------------------------------------------------------------------------------------------------------------
def tab_to_pixel(B, N, p):
    """int64 [B N^2]: the pixel-order row (b N + I) N + J of row m = (b R^2 + t) p^2 + a p + b of the (token, a, b) order"""
    R = N // p
    m = np.arange(B * N * N)
    sub, tok = m % (p * p), m // (p * p)
    t, b = tok % (R * R), tok // (R * R)
    i, j = p * (t // R) + sub // p, p * (t % R) + sub % p
    return (b * N + i) * N + j


def to_tab_order(rows_pixel, B, N, p):
    """[B N^2, C] pixel order -> (token, a, b) order"""
    return rows_pixel[torch.as_tensor(tab_to_pixel(B, N, p))]


def token_valid(flags, p, first_pixel=False):
    """bool [B, R, R]: the token holds a valid pixel (first_pixel: the token's FIRST pixel is valid -- the `token_mask` mistake)"""
    v = X.pair_valid(flags)
    B, N, _ = v.shape
    R = N // p
    v = v.view(B, R, p, R, p)
    return v[:, :, 0, :, 0] if first_pixel else v.any(4).any(2)


def pixel_mask(flags, p, mut=None):
    """bool [B, N, N] the masks of the read-out see: valid(I, J), or under `token_mask` the token's first pixel's"""
    v = X.pair_valid(flags)
    if mut != "token_mask":
        return v
    return token_valid(flags, p, True).repeat_interleave(p, 1).repeat_interleave(p, 2)


# ------------------------------------------------------------------------------------------------------------------------------
# PatchEmbed
# ------------------------------------------------------------------------------------------------------------------------------
def patch_kp(cin, p):
    return (p * p * cin + 31) // 32 * 32


def patch_input(t, flags, p, self_cond, sc_on, dtype=torch.float64, mut=None):
    """[B R^2, p^2 Cin], column (a p + b) Cin + c: edge_ref.pe_input's channels of the token's p^2 pixels side by side"""
    img = X.pe_input(t, flags, self_cond, sc_on, dtype)          # [B N^2, Cin], node parts masked per pixel
    B, N = flags.shape
    R, cin = N // p, img.shape[1]
    if mut == "token_mask":       # the node parts masked by the token's first pixel instead
        un = X.pe_input(t, flags, self_cond, sc_on, dtype, unmasked=True).view(B, N, N, cin)
        m = pixel_mask(flags, p, mut)[..., None]
        nsc = 2 if self_cond else 1
        ca = nsc * t["adj"].shape[1]
        img = torch.cat([un[..., :ca], torch.where(m, un[..., ca:], torch.zeros((), dtype=dtype))], -1).reshape(B * N * N, cin)
    return img.view(B, R, p, R, p, cin).permute(0, 1, 3, 2, 4, 5).reshape(B * R * R, p * p * cin)


def pack_pe_weight(W, Kp=None, mut=None):
    """patch_embed.proj.weight [E, Cin, p, p] -> [E, Kp], column (a p + b) Cin + c, zero padded (dsg_finalize_weights)"""
    if mut == "pe_swap_ab":
        W = W.transpose(2, 3)
    E_, cin, p, _ = W.shape
    w = W.permute(0, 2, 3, 1).reshape(E_, p * p * cin)
    return w if Kp is None else X.pad_k(w, Kp)


def patch_embed_formula(inp, W, bias, gam, bet, aff, aff_off, T, mut=None):
    """inp [B R^2, p^2 Cin] -> conv as one product -> LayerNorm -> silu(shift + n (1 + scale)); T = R^2 tokens per sample"""
    y = inp @ pack_pe_weight(W.to(inp.dtype), mut=mut).t() + bias.to(inp.dtype)
    return X.ln_mod_formula(y, gam.to(inp.dtype), bet.to(inp.dtype), aff.to(inp.dtype), aff_off, T)


# ------------------------------------------------------------------------------------------------------------------------------
# read-out and heads
# ------------------------------------------------------------------------------------------------------------------------------
def readout_r0(xn, W0, b0, B, N, p, mut=None):
    """LN(x) [B R^2, E] -> r0 [B N^2, E] in PIXEL order: the transposed convolution with stride = kernel = p"""
    if mut == "ro_swap_ab":
        W0 = W0.transpose(2, 3)
    if mut == "ro_out_in":
        W0 = W0.transpose(0, 1)
    R, E_ = N // p, xn.shape[1]
    r = torch.einsum("brci,ioxy->brxcyo", xn.view(B, R, R, E_), W0.to(xn.dtype))
    return r.reshape(B * N * N, E_) + b0.to(xn.dtype)


def pack_ro0(W0, b0):
    """read_out.0 [in, out, p, p] -> ([p^2 E, E] row (a p + b) E + o, bias repeated): one product writes rows in (token, a, b) order"""
    E_, _, p, _ = W0.shape
    return W0.permute(2, 3, 1, 0).reshape(p * p * E_, E_), b0.repeat(p * p)


def shared_rep(xn, q, B, N, p, mut=None):
    """the read-out chain [B N^2, E] in pixel order, in xn's dtype; q: W0 [E, E, p, p], b0, W1, b1, W2, b2 (1 x 1 convs as [out, in])"""
    c = lambda k: q[k].to(xn.dtype)
    s = readout_r0(xn, q["W0"], q["b0"], B, N, p, mut)
    s = s @ c("W1").t() + c("b1")
    return s @ c("W2").t() + c("b2")


def adj_head(s, q, flags, p, mut=None):
    """[B, Ca, N, N] = valid (F2 gelu(F1 s + f1) + f2)"""
    c = lambda k: q[k].to(s.dtype)
    B, N = flags.shape
    o = gelu(s @ c("F1").t() + c("f1")) @ c("F2").t() + c("f2")
    return X.adj_layout(o, pixel_mask(flags, p, mut), B, N)


def node_pool(s, flags, p, mut=None):
    """[B N, E]: (1/N) sum_J mask(I, J) s[(I, J)]; `mean_over_R`: divided by R instead"""
    B, N = flags.shape
    m = pixel_mask(flags, p, mut).to(s.dtype)
    div = N // p if mut == "mean_over_R" else N
    return ((s.view(B, N, N, -1) * m[..., None]).sum(2) / div).reshape(B * N, -1)


def node_head(pool, q, flags):
    c = lambda k: q[k].to(pool.dtype)
    return X.head_node_formula(gelu(pool @ c("G1").t() + c("g1")), c("G2"), c("g2"), flags)


def pooled_fold(xn, q, flags, p, mut=None):
    """node_feat [B N, E] through the fold (float64 or float32 as xn): pooling LN(x) per (node row, column parity) first"""
    B, N = flags.shape
    R, E_ = N // p, xn.shape[1]
    d = lambda k: q[k].to(xn.dtype)
    A = d("W2") @ d("W1")
    cc = A @ d("b0") + d("W2") @ d("b1") + d("b2")
    f = torch.as_tensor(flags).to(xn.dtype)                                  # [B, N]
    fb = f.view(B, R, p)                                                     # flag of pixel column p tj + b
    x4 = xn.view(B, R, R, E_)
    s = torch.einsum("bjq,bije->biqe", fb, x4) / N                           # [B, R (ti), p (b), E]
    cnt = fb.sum(1)                                                          # [B, p]: valid columns = b mod p
    if mut == "cnt_total":
        cnt = f.sum(1, keepdim=True).expand(B, p)
    out = torch.zeros(B, N, E_, dtype=xn.dtype)
    W0 = d("W0")
    for a in range(p):
        acc = torch.zeros(B, R, E_, dtype=xn.dtype)
        for b in range(p):
            F = A @ W0[:, :, a, b].t()                                       # [E, E]: r[o] = sum_i F[o, i] xn[i]
            acc = acc + s[:, :, b] @ F.t() + cc * (cnt[:, b] / N)[:, None, None]
        out[:, a::p] = acc
    return (out * f[..., None]).reshape(B * N, E_)


# ------------------------------------------------------------------------------------------------------------------------------
# the fused p = 2 forms (csrc/kernels_patch.hip): packed operands and what the kernels leave
# ------------------------------------------------------------------------------------------------------------------------------
def pack_pe_fused(W, Kps):
    """patch_embed.proj.weight [96, Cin, 2, 2] -> Wp [4][3][Kps / 8][64][4]: per sub-pixel 2 a + b, f32_ref.pack_rows of W[:, :, a, b]
    zero-padded to [96, Kps] (the pe_wp loop of dsg_finalize_weights at patch_size 2)"""
    import f32_ref as R
    return np.concatenate([R.pack_rows(X.pad_k(W[:, :, a, b], Kps).numpy()) for a in range(2) for b in range(2)])


def fold_readout_p2(q):
    """float64: Fa [4][96, 96] (sub = 2 a + b) = F1 W2 W1 W0[:, :, a, b]^T, fa = F1 (W2 (W1 b0 + b1) + b2) + f1 (the same for the four)"""
    d = {k: v.double() for k, v in q.items()}
    A = d["W2"] @ d["W1"]
    c = A @ d["b0"] + d["W2"] @ d["b1"] + d["b2"]
    return dict(Fa=[d["F1"] @ A @ d["W0"][:, :, a, b].t() for a in range(2) for b in range(2)], fa=d["F1"] @ c + d["f1"])


def folded_adj(xn, fold, q, flags):
    """the kernel's chain in xn's dtype on the fold cast to it: [B, Ca, N, N] = valid (F2 gelu(Fa[a, b] LN(x)[t] + fa) + f2), p = 2"""
    B, N = flags.shape
    R = N // 2
    c = lambda v: v.to(xn.dtype)
    o = torch.zeros(B, R, 2, R, 2, q["F2"].shape[0], dtype=xn.dtype)
    for a in range(2):
        for b in range(2):
            h = gelu(xn @ c(fold["Fa"][2 * a + b]).t() + c(fold["fa"])) @ c(q["F2"]).t() + c(q["f2"])
            o[:, :, a, :, b] = h.view(B, R, R, -1)
    return X.adj_layout(o.reshape(B * N * N, -1), X.pair_valid(flags), B, N)


def pool_ext_p2(xn, flags):
    """pool_ext [B N, 256] of the fused p = 2 read-out from LN(x) [B R^2, 96]: row (b, I = 2 ti + a) = (s[ti, 0] | s[ti, 1] | f_I cnt_0 / N
    | f_I cnt_1 / N | 0 ..), s[ti, q] = (1/N) sum_tj f_{2 tj + q} LN(x)[ti, tj] -- zero where neither node row of the token row is valid
    (the kernel replaces the LayerNorm of a token without a valid pixel by zeros; such a row's s is never read: f_I = 0 for both)"""
    B, N = flags.shape
    R, E_ = N // 2, xn.shape[1]
    f = torch.as_tensor(flags).to(xn.dtype)
    fq = f.view(B, R, 2)
    rowok = (fq.sum(2) > 0).to(xn.dtype)                                      # [B, R (ti)]
    s = torch.einsum("bjq,bije->biqe", fq, xn.view(B, R, R, E_)) / N * rowok[:, :, None, None]
    out = torch.zeros(B, N, 256, dtype=xn.dtype)
    out[:, :, :2 * E_] = s.reshape(B, R, 2 * E_).repeat_interleave(2, 1)
    out[:, :, 2 * E_:2 * E_ + 2] = f[:, :, None] * fq.sum(1)[:, None, :] / N
    return out.reshape(B * N, 256)


# ------------------------------------------------------------------------------------------------------------------------------
# the network's own parameters (a state dict of numpy arrays, diffusesg_amd.weights.synth_state_dict)
# ------------------------------------------------------------------------------------------------------------------------------
def sd_params(sd, dtype=torch.float64):
    g = lambda k: torch.from_numpy(np.ascontiguousarray(sd[k])).to(dtype)
    sq = lambda k: g(k)[:, :, 0, 0]
    return dict(Wpe=g("patch_embed.proj.weight"), bpe=g("patch_embed.proj.bias"), gpe=g("patch_embed.norm.weight"), bepe=g("patch_embed.norm.bias"),
                W0=g("read_out.0.weight"), b0=g("read_out.0.bias"), W1=sq("read_out.1.weight"), b1=g("read_out.1.bias"),
                W2=sq("read_out.2.weight"), b2=g("read_out.2.bias"), F1=g("readout_adj_mlp.fc1.weight"), f1=g("readout_adj_mlp.fc1.bias"),
                F2=g("readout_adj_mlp.fc2.weight"), f2=g("readout_adj_mlp.fc2.bias"), G1=g("readout_node_mlp.fc1.weight"),
                g1=g("readout_node_mlp.fc1.bias"), G2=g("readout_node_mlp.fc2.weight"), g2=g("readout_node_mlp.fc2.bias"))


def noise_affine(sd, c_noise, key="patch_embed", dtype=torch.float64):
    """(scale | shift) rows [B, 2 E] of `key`.affine for the noise labels: PositionalEmbedding -> silu(map_layer0) -> silu(map_layer1)
    -> affine (diffusesg.py:500-513, :768-771, :574)"""
    g = lambda k: torch.from_numpy(np.ascontiguousarray(sd[k])).to(dtype)
    E_ = sd["map_layer0.weight"].shape[1]
    half = E_ // 2
    freqs = (1.0 / 10000.0) ** (torch.arange(half, dtype=torch.float32) / half)
    x = torch.as_tensor(c_noise, dtype=torch.float32).ger(freqs).to(dtype)
    emb = torch.cat([x.cos(), x.sin()], 1)
    emb = silu(emb @ g("map_layer0.weight").t() + g("map_layer0.bias"))
    emb = silu(emb @ g("map_layer1.weight").t() + g("map_layer1.bias"))
    return emb @ g(key + ".affine.weight").t() + g(key + ".affine.bias")


def net_patch_embed(sd, cfg, flags, adj, node, sc_adj, sc_node, c_noise, dtype=torch.float64, mut=None):
    """PatchEmbed's output [B R^2, E] from the network inputs (numpy; sc_* None: no self-conditioning input)"""
    q = sd_params(sd, dtype)
    tt = lambda v: torch.from_numpy(np.ascontiguousarray(v))
    t = dict(adj=tt(adj), node=tt(node), sc_adj=tt(sc_adj if sc_adj is not None else np.zeros_like(adj)),
             sc_node=tt(sc_node if sc_node is not None else np.zeros_like(node)))
    inp = patch_input(t, flags, cfg.patch_size, cfg.self_condition, sc_adj is not None, dtype, mut)
    aff = noise_affine(sd, c_noise, dtype=dtype)
    return patch_embed_formula(inp, q["Wpe"], q["bpe"], q["gpe"], q["bepe"], aff, 0, cfg.token_res ** 2, mut)


def net_readout(sd, cfg, flags, xn, dtype=torch.float64, mut=None):
    """(shared rep [B N^2, E] pixel order, adj_out [B, Ca, N, N], node_out [B, N, Cn]) from the final norm's output xn [B R^2, E]"""
    q = sd_params(sd, dtype)
    B, N = flags.shape
    xn = torch.as_tensor(xn).to(dtype).reshape(B * cfg.token_res ** 2, -1)
    s = shared_rep(xn, q, B, N, cfg.patch_size, mut)
    return s, adj_head(s, q, flags, cfg.patch_size, mut), node_head(node_pool(s, flags, cfg.patch_size, mut), q, flags).view(B, N, -1)
