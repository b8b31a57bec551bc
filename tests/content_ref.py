"""NumPy float64 restatement of content guidance (include/dsg.h: dsg_sample_guided_content) for one guided call: the soft
minimum over the live ordered pairs of a graph, its gradient on the adjacency estimate and on the label channels, the arg-max pair of
every item, the shift with both known masks, the content shift's own clip factor and D~.

Graph b has K items; item k is (s_k [Cl], o_k [Cl], p_k [Ca]) with weights (a_s, a_o, a_p) = w_spo[b, k].  Live pairs: i != j, both nodes
valid.  Entries that are not live are chosen by a select BEFORE any arithmetic, so NaN there reaches nothing.

The keyword switches of `graph_content` / `guided_call` restate MISTAKES; tests/test_content_guide_host.py shows that each of them moves
some output beyond the bars the GPU tests use.

The bars (`bars`) are derived, not tuned.  The kernel evaluates every output in float64 from the float32 inputs and rounds once, so an
element may differ from this reference by
  * one float32 ulp of the reference value (half an ulp of rounding, and the value may sit next to a rounding boundary), plus
  * the float64 error of two correct evaluations that differ in summation order and in their exp / log:  with u = 2^-53,
        n_d = 3 (2 Cl + Ca) + 6 operations behind d_k, so |delta d| <= n_d u d_max,
        the exponent -(d - min d) / tau is off by at most 2 n_d u d_max / tau + 4 u,
        pi_k = exp / sum is off by  rho = 2 (2 n_d u d_max / tau + 8 u) + (N^2 + 8) u  relatively,
        an element  sum_k pi_k 2 a (D - t)  by  (rho + (2 K + 8) u) sum_k |pi_k 2 a (D - t)|,
        L_k = min d - tau log(S / P)  by  n_d u d_max + tau ((N^2 + 8) u + 2 n_d u d_max / tau) + 4 u |L_k|.
d_max is the largest d_k over the graph's live pairs and active items, taken from the reference."""
import numpy as np

F32 = np.float32
U = 2.0 ** -53


def ulp32(v):
    """the float32 spacing at |v|, as float64"""
    with np.errstate(over="ignore"):
        return np.spacing(np.abs(np.asarray(v, np.float64)).astype(F32)).astype(np.float64)


def graph_content(Dn, Da, valid, subj, obj, pred, w_spo, tau, *, swap_so=False, count_diag=False, count_padded=False, no_mean=False,
                  obj_axis=False, no_two=False, no_max_sub=False):
    """one graph: Dn [N, Cl] the label channels of D_node, Da [Ca, N, N], valid [N], subj / obj [K, Cl], pred [K, Ca], w_spo [K, 3] ->
    dict(loss, item_loss [K], g_adj [Ca, N, N], g_label [N, Cl], best [K, 2], abs_adj, abs_label: the sums of |terms| behind each
    gradient element, d_max, n_pairs)"""
    N, Cl = Dn.shape
    Ca = Da.shape[0]
    K = subj.shape[0]
    real = np.asarray(valid).astype(bool)
    v = np.ones(N, dtype=bool) if count_padded else real          # the mistake: padded nodes take part, with an all-zero row
    live = v[:, None] & v[None, :]
    if not count_diag:                                            # the mistake: a node paired with itself
        live = live & ~np.eye(N, dtype=bool)
    readable = real[:, None] & real[None, :] & ~np.eye(N, dtype=bool)
    if count_diag:
        readable = real[:, None] & real[None, :]
    Dn64 = np.where(real[:, None], np.asarray(Dn), 0.0).astype(np.float64)
    Da64 = np.where(readable[None], np.asarray(Da), 0.0).astype(np.float64)
    out = dict(loss=0.0, item_loss=np.zeros(K), g_adj=np.zeros((Ca, N, N)), g_label=np.zeros((N, Cl)), best=-np.ones((K, 2), np.int64),
               abs_adj=np.zeros((Ca, N, N)), abs_label=np.zeros((N, Cl)), d_max=0.0, n_pairs=int(live.sum()))
    P = int(live.sum())
    if P == 0:
        return out
    two = 1.0 if no_two else 2.0                                  # the mistake: the 2 of d(x^2)/dx dropped
    for k in range(K):
        a_s, a_o, a_p = (float(x) for x in w_spo[k])
        if a_s == 0 and a_o == 0 and a_p == 0:
            continue
        s, o, p = subj[k].astype(np.float64), obj[k].astype(np.float64), pred[k].astype(np.float64)
        if swap_so:                                               # the mistake: subject and object exchanged
            s, o, a_s, a_o = o, s, a_o, a_s
        ds = ((Dn64 - s) ** 2).sum(1)
        do = ((Dn64 - o) ** 2).sum(1)
        dp = ((Da64 - p[:, None, None]) ** 2).sum(0)
        d = a_s * ds[:, None] + a_o * do[None, :] + a_p * dp
        dl = np.where(live, d, np.inf)
        m = 0.0 if no_max_sub else float(dl.min())                # the mistake: no max-subtraction
        with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
            ex = np.where(live, np.exp(-(np.where(live, d, 0.0) - m) / tau), 0.0)
            S = ex.sum()
            Lk = m - tau * np.log(S if no_mean else S / P)        # the mistake: no 1/P
            pi = ex / S
            row = pi.sum(1)
            col = pi.sum(1) if obj_axis else pi.sum(0)            # the mistake: the object term summed over the wrong axis
            ta = pi[None] * (two * a_p) * (Da64 - p[:, None, None])
            tl_s = row[:, None] * (two * a_s) * (Dn64 - s)
            tl_o = col[:, None] * (two * a_o) * (Dn64 - o)
        out["item_loss"][k] = Lk
        out["loss"] += Lk
        out["g_adj"] += ta
        out["g_label"] += tl_s + tl_o
        out["abs_adj"] += np.abs(ta)
        out["abs_label"] += np.abs(tl_s) + np.abs(tl_o)
        e = int(np.argmin(dl))                                    # the first minimum: the lowest flat index among equals
        out["best"][k] = (e // N, e % N)
        out["d_max"] = max(out["d_max"], float(np.where(live, d, 0.0).max()))
    return out


def content_loss_grad(D, flags, cfg, **kw):
    """over a batch.  D = (D_adj [B, Ca, N, N], D_node [B, N, Cn]); cfg = dict(Cl, tau, subj [B, K, Cl], obj, pred [B, K, Ca],
    w_spo [B, K, 3]).  Returns dict(loss [B], item_loss [B, K], grad_adj [B, Ca, N, N], grad_label [B, N, Cl], best [B, K, 2], abs_*,
    d_max [B], n_pairs [B]); gradients are zero at entries that are not live"""
    Da, Dn = D
    B = flags.shape[0]
    Cl = cfg["Cl"]
    tau = float(F32(cfg["tau"]))                                  # the descriptor holds float32: that value is the input
    gs = [graph_content(Dn[b][:, :Cl], Da[b], flags[b], cfg["subj"][b], cfg["obj"][b], cfg["pred"][b], cfg["w_spo"][b], tau, **kw)
          for b in range(B)]
    st = lambda key: np.stack([np.asarray(g[key]) for g in gs])
    return dict(loss=st("loss"), item_loss=st("item_loss"), grad_adj=st("g_adj"), grad_label=st("g_label"), best=st("best"),
                abs_adj=st("abs_adj"), abs_label=st("abs_label"), d_max=st("d_max"), n_pairs=st("n_pairs"))


def graph_norm(a, x, flags):
    """2-norm per graph over the live entries of (adjacency [B, C, N, N], node [B, N, C]), selected by the flags (the diagonal of valid
    nodes counts, as in guide.clip_factor's reference norm)"""
    f = flags.astype(bool)
    fa, fn = f[:, None, :, None] & f[:, None, None, :], f[:, :, None]
    B = f.shape[0]
    sq = lambda m, v: (np.where(m, np.asarray(v, np.float64), 0.0) ** 2).reshape(B, -1).sum(1)
    return np.sqrt(sq(fa, a) + sq(fn, x))


def clip_factor(shift_norm, ref_norm, clip_ratio):
    if clip_ratio is None:
        return np.ones_like(shift_norm)
    bound = clip_ratio * ref_norm
    return np.where(shift_norm > bound, bound / np.maximum(shift_norm, np.finfo(np.float32).tiny), 1.0)


def guided_call(x_hat, D, flags, c, cfg, mask_adj=None, mask_node=None, ignore_mask=False, shift_beyond=False, **kw):
    """One preconditioned call: x_hat = (adj, node), D = (adj, node) after the valid mask and the known select, c a number; cfg as
    content_loss_grad's plus w (w_content) and clip_ratio (None: unclipped).  Returns content_loss_grad's dict plus shift_adj,
    shift_label (as applied), factor [B], norms [B, 2], D_guided_adj, D_guided_node (0 at padded entries).
    ignore_mask (the mistake): known entries shifted; shift_beyond (the mistake): the label shift [B, N, Cl] read with the row stride
    C_node - 4, which moves channels >= Cl"""
    Da, Dn = D
    f = flags.astype(bool)
    B, N, Cn = Dn.shape
    Cl = cfg["Cl"]
    r = content_loss_grad(D, flags, cfg, **kw)
    cw = float(F32(c) * F32(cfg["w"]))                           # the float32 product c_i * w_content
    sa, sl = cw * r["grad_adj"], cw * r["grad_label"]
    if not ignore_mask:
        if mask_adj is not None:
            sa = np.where(np.asarray(mask_adj) != 0, 0.0, sa)
        if mask_node is not None:
            sl = np.where(np.asarray(mask_node)[..., :Cl] != 0, 0.0, sl)
    sn = np.sqrt((sa ** 2).reshape(B, -1).sum(1) + (sl ** 2).reshape(B, -1).sum(1))
    if cfg.get("clip_ratio") is None:
        rn, fac = np.zeros_like(sn), np.ones_like(sn)
    else:
        rn = graph_norm(np.where(f[:, None, :, None] & f[:, None, None, :], np.asarray(x_hat[0], np.float64) - Da, 0.0),
                        np.where(f[:, :, None], np.asarray(x_hat[1], np.float64) - Dn, 0.0), flags)
        fac = clip_factor(sn, rn, float(F32(cfg["clip_ratio"])))
    sa, sl = sa * fac[:, None, None, None], sl * fac[:, None, None]
    Ga = np.where(f[:, None, :, None] & f[:, None, None, :], np.asarray(Da, np.float64), 0.0) - sa
    Gn = np.where(f[:, :, None], np.asarray(Dn, np.float64), 0.0)
    if shift_beyond:
        wide = np.zeros(B * N * (Cn - 4))
        wide[:sl.size] = sl.reshape(-1)
        Gn[..., :Cn - 4] -= np.where(f[:, :, None], wide.reshape(B, N, Cn - 4), 0.0)
    else:
        Gn[..., :Cl] -= sl
    r.update(shift_adj=sa, shift_label=sl, factor=fac, norms=np.stack([sn, rn], 1), D_guided_adj=Ga, D_guided_node=Gn)
    return r


def bars(ref, cfg, N, Ca):
    """the per-element bars of loss, item_loss, grad_adj, grad_label (module docstring) from a reference dict"""
    Cl, tau, K = cfg["Cl"], float(F32(cfg["tau"])), cfg["subj"].shape[1]
    n_d = 3 * (2 * Cl + Ca) + 6
    ed = n_d * U * ref["d_max"]                                   # [B] |delta d|
    rho = 2 * (2 * ed / tau + 8 * U) + (N * N + 8) * U
    rel = rho + (2 * K + 8) * U
    e_item = ed[:, None] + tau * ((N * N + 8) * U + 2 * ed[:, None] / tau) + 4 * U * np.abs(ref["item_loss"])
    return dict(grad_adj=ulp32(ref["grad_adj"]) + rel[:, None, None, None] * ref["abs_adj"],
                grad_label=ulp32(ref["grad_label"]) + rel[:, None, None] * ref["abs_label"],
                item_loss=ulp32(ref["item_loss"]) + e_item,
                loss=ulp32(ref["loss"]) + e_item.sum(1) + K * U * np.abs(ref["item_loss"]).sum(1))
