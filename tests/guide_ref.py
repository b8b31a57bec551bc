"""float64 numpy restatements for the input-gradient and guidance tests: the backward of the input assembly fused with the
preconditioning chain (dsg_debug_t_assemble_bwd) with its per-element error bars, and the state algebra of `guided_sample`.
No GPU, no torch: imported by GPU and host tests alike."""
import numpy as np

U = 2.0 ** -24


def slots(c_adj, c_node, self_cond):
    """column of the first (adjacency | node-of-the-row | node-of-the-column) CURRENT-value slot in a token row, and the channel count"""
    nsc, sc = (2, 1) if self_cond else (1, 0)
    return sc * c_adj, nsc * c_adj + sc * c_node, nsc * c_adj + nsc * c_node + sc * c_node, nsc * (c_adj + 2 * c_node)


def assemble_bwd_case(B, N, c_adj, c_node, self_cond, flags_kind, seed=0, pad=3):
    """fp32 operands of one call: d_tok [B N N, ld] with ld = channels + pad (the self-conditioning slots and the padding columns hold
    large values the kernel must not read), flags, per-sample coefficients, g"""
    rng = np.random.default_rng(seed + 1000 * N + 10 * c_adj + B)
    ld = slots(c_adj, c_node, self_cond)[3] + pad
    d_tok = rng.standard_normal((B * N * N, ld)).astype(np.float32)
    a0, r0, c0, _ = slots(c_adj, c_node, self_cond)
    live = np.zeros(ld, bool)
    for o, w in ((a0, c_adj), (r0, c_node), (c0, c_node)):
        live[o:o + w] = True
    d_tok[:, ~live] = 1e30   # read by mistake: the result leaves every bar
    flags = np.zeros((B, N), np.uint8)
    for b in range(B):
        if flags_kind == "all":
            flags[b] = 1
        elif flags_kind == "one":
            flags[b, 0] = 1
        elif flags_kind == "ragged":
            flags[b, :max(1, (N * (b + 1)) // (B + 1))] = 1
        elif flags_kind != "none":
            raise ValueError(flags_kind)
    c_skip = rng.uniform(0.0, 1.0, B).astype(np.float32)
    c_in = rng.uniform(0.01, 2.0, B).astype(np.float32)
    g_adj = rng.standard_normal((B, c_adj, N, N)).astype(np.float32)
    g_node = rng.standard_normal((B, N, c_node)).astype(np.float32)
    return dict(B=B, N=N, c_adj=c_adj, c_node=c_node, self_cond=self_cond, ld=ld, d_tok=d_tok, flags=flags, c_skip=c_skip, c_in=c_in,
                g_adj=g_adj, g_node=g_node)


def assemble_bwd_expect(o):
    """float64 (out_adj, out_node) and their bars (n_terms + 2) u sum|terms|, the terms being the products that are added:
    adjacency: c_skip m g and c_in d_tok (2 terms); node: c_skip g and c_in d_tok for every valid j of the row and of the column"""
    B, N, Ca, Cn = o["B"], o["N"], o["c_adj"], o["c_node"]
    a0, r0, c0, _ = slots(Ca, Cn, o["self_cond"])
    d = o["d_tok"].astype(np.float64).reshape(B, N, N, o["ld"])
    m = o["flags"].astype(np.float64)
    cs, ci = o["c_skip"].astype(np.float64), o["c_in"].astype(np.float64)
    mm = m[:, :, None] * m[:, None, :]                                        # [B, i, j]
    t_skip = cs[:, None, None, None] * mm[:, None] * o["g_adj"].astype(np.float64)
    t_tok = ci[:, None, None, None] * d[..., a0:a0 + Ca].transpose(0, 3, 1, 2)
    out_adj = t_skip + t_tok
    bar_adj = 4 * U * (np.abs(t_skip) + np.abs(t_tok))
    row = d[..., r0:r0 + Cn]                                                  # [B, i, j, c]: token (b, i, j)
    col = d[..., c0:c0 + Cn].transpose(0, 2, 1, 3)                            # [B, i, j, c]: token (b, j, i)
    w = mm[..., None]
    s = (w * row).sum(2) + (w * col).sum(2)
    sabs = (w * np.abs(row)).sum(2) + (w * np.abs(col)).sum(2)
    n_valid = m.sum(1)                                                        # terms per sum
    t_g = cs[:, None, None] * m[:, :, None] * o["g_node"].astype(np.float64)
    out_node = t_g + ci[:, None, None] * s
    n_terms = 1 + 2 * n_valid[:, None, None]
    bar_node = (n_terms + 2) * U * (np.abs(t_g) + ci[:, None, None] * sabs)
    return out_adj, out_node, bar_adj, bar_node


def worst_ratio(got, ref, bar):
    r = np.abs(got.astype(np.float64) - ref) / (bar + 1e-300)
    r = np.where(np.isfinite(r), r, np.inf)
    return float(r.max()) if r.size else 0.0


# ---- guided loop: one preconditioned call and one update in float64 ----
def graph_norm(a, x):
    B = a.shape[0]
    return np.sqrt((a.reshape(B, -1) ** 2).sum(1) + (x.reshape(B, -1) ** 2).sum(1))


def guided_estimate(x_hat, D, grad, w, t, flags, clip_ratio, known=None):
    """(shift, D~) of guided_sample from the recorded x_hat, D (after the select), raw gradient: float64"""
    f = flags.astype(bool)
    fa, fn = (f[:, None, :, None] & f[:, None, None, :]), f[:, :, None]
    xa, xn = (v.astype(np.float64) for v in x_hat)
    Da, Dn = (v.astype(np.float64) for v in D)
    wt2 = float(np.float32(w) * np.float32(t) * np.float32(t))
    sa, sn = np.where(fa, grad[0].astype(np.float64) * wt2, 0.0), np.where(fn, grad[1].astype(np.float64) * wt2, 0.0)
    if clip_ratio is not None:
        ns, nr = graph_norm(sa, sn), graph_norm(xa - Da, xn - Dn)
        fac = np.where(ns > clip_ratio * nr, clip_ratio * nr / np.maximum(ns, 1e-300), 1.0)
        sa, sn = sa * fac[:, None, None, None], sn * fac[:, None, None]
    Ga, Gn = Da - sa, Dn - sn
    if known is not None:
        ka, kn, ma, mn = known
        Ga, Gn = np.where(fa, np.where(ma, ka, Ga), 0.0), np.where(fn, np.where(mn, kn, Gn), 0.0)
    return (sa, sn), (Ga, Gn)


def euler_update(x_hat, G, t, h, flags, ms_coef=0.0, G_prev=None):
    f = flags.astype(bool)
    masks = ((f[:, None, :, None] & f[:, None, None, :]), f[:, :, None])
    inv_t = float(np.float32(1.0) / np.float32(t))
    out = []
    for k in range(2):
        xh, g = x_hat[k].astype(np.float64), G[k].astype(np.float64)
        if ms_coef != 0.0 and G_prev is not None:
            g = g + ms_coef * (g - G_prev[k].astype(np.float64))
        out.append(np.where(masks[k], xh + h * (inv_t * xh - inv_t * g), 0.0))
    return tuple(out)


def heun_update(x_hat, G1, G2, t, h, flags):
    f = flags.astype(bool)
    masks = ((f[:, None, :, None] & f[:, None, None, :]), f[:, :, None])
    inv_t = float(np.float32(1.0) / np.float32(t))
    inv_tp = float(np.float32(1.0) / (np.float32(t) + np.float32(h)))
    out = []
    for k in range(2):
        xh, g1, g2 = x_hat[k].astype(np.float64), G1[k].astype(np.float64), G2[k].astype(np.float64)
        dc = inv_t * xh - inv_t * g1
        xp = xh + h * dc
        dp = inv_tp * xp - inv_tp * g2
        out.append(np.where(masks[k], xh + h * (0.5 * dc + 0.5 * dp), 0.0))
    return tuple(out)
