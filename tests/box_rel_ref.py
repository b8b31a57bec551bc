"""NumPy float64 restatement of the relation term of box guidance (include/dsg.h: dsg_sample_guided_rel): L_rel and its
gradient for given kinds, the three decode rules that turn an adjacency estimate into predicates, the predicate -> kind lookup, and one
guided call with all four losses (the other three: tests/box_guide_ref.py).  Pairs that are not live (a padded node, the diagonal)
are chosen by a select, so NaN there reaches nothing.

An entry (i, j) of a kind matrix has SUBJECT i (the row) and OBJECT j (the column).  Lines in guide.py's order: 0 left, 1 centre x,
2 right, 3 top, 4 centre y, 5 bottom; y grows downwards.

The keyword switches of `graph_rel` restate MISTAKES: tests/test_box_rel_host.py shows that each moves the result beyond the bars the
GPU tests use."""
import numpy as np

import box_guide_ref as BR

NONE, LEFT_OF, RIGHT_OF, ABOVE, BELOW, INSIDE, CONTAINS, ON = range(8)
KINDS = 8
S, O = 0, 1   # whose line a term reads: the subject's, the object's


def _terms(kind, flip_y=False, contains_as_inside=False):
    """the elementary terms of a kind: (A, B, with margin, hinged) for h(A - B [+ m]), A and B = (line, S or O)"""
    if flip_y and kind in (ABOVE, BELOW):
        kind = ABOVE + BELOW - kind
    if contains_as_inside and kind == CONTAINS:
        kind = INSIDE
    inside = lambda I, J: [((0, J), (0, I), False, True), ((2, I), (2, J), False, True), ((3, J), (3, I), False, True), ((5, I), (5, J), False, True)]
    return {LEFT_OF: [((1, S), (1, O), True, True)], RIGHT_OF: [((1, O), (1, S), True, True)],
            ABOVE: [((4, S), (4, O), True, True)], BELOW: [((4, O), (4, S), True, True)],
            INSIDE: inside(S, O), CONTAINS: inside(O, S),
            ON: [((5, S), (3, O), False, False), ((0, O), (1, S), False, True), ((1, S), (2, O), False, True)]}[kind]


def graph_rel(d4, valid, kinds, margin=0.0, half=True, swap=False, flip_y=False, margin_sign=1.0, count_diag=False, symmetric=False,
              contains_as_inside=False, on_hinged=False):
    """one graph: d4 [N, 4] the box channels of D, valid [N] bool, kinds [N, N] -> (L_rel, dL_rel/dd4 [N, 4])"""
    N = d4.shape[0]
    v = valid.astype(bool)
    d = np.where(v[:, None], d4, 0.0).astype(np.float64)
    b = d * 0.5 + 0.5
    cx, cy, w, h = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    ln = np.stack([cx - 0.5 * w, cx, cx + 0.5 * w, cy - 0.5 * h, cy, cy + 0.5 * h])
    pair = v[:, None] & v[None, :]
    if not count_diag:
        pair = pair & ~np.eye(N, dtype=bool)
    K = np.asarray(kinds).astype(np.int64)
    if swap:                                   # the mistake: subject and object exchanged
        K = K.T
    if symmetric:                              # the mistake: (j, i) counted with (i, j)'s kind where only (i, j) is set
        K = np.where((K == 0) & (K.T != 0), K.T, K)
    K = np.where(pair & (K >= 0) & (K < KINDS), K, 0)
    m = margin_sign * float(margin)
    gl = np.zeros((BR.LINES, N))
    loss = 0.0
    side = lambda qr: ln[qr[0]][:, None] if qr[1] == S else ln[qr[0]][None, :]
    for kind in range(1, KINDS):
        on = K == kind
        if not on.any():
            continue
        for A, Bq, with_m, hinged in _terms(kind, flip_y, contains_as_inside):
            val = side(A) - side(Bq) + (m if with_m else 0.0)
            if hinged or on_hinged:
                val = np.where(val > 0, val, 0.0)
            val = np.where(on, val, 0.0)
            loss += (val * val).sum()
            for (q, role), sg in ((A, 2.0), (Bq, -2.0)):
                gl[q] += sg * val.sum(1 if role == S else 0)
    gb = np.stack([gl[0] + gl[1] + gl[2], gl[3] + gl[4] + gl[5], 0.5 * (gl[2] - gl[0]), 0.5 * (gl[5] - gl[3])], axis=1)
    return loss, (0.5 if half else 1.0) * gb


def rel_loss_grad(D_node, flags, kinds, margin=0.0, count_padded=False, **kw):
    """(L_rel [B], g [B, N, 4]) over a batch; g is zero at padded nodes.  count_padded (the mistake): padded nodes take part with the
    box of an all-zero row"""
    B, N = flags.shape
    L, g = np.zeros(B), np.zeros((B, N, 4))
    for k in range(B):
        real = flags[k].astype(bool)
        v = np.ones(N, dtype=bool) if count_padded else real
        d4 = np.where(real[:, None], D_node[k, :, -4:], 0.0)
        L[k], gk = graph_rel(d4, v, kinds[k], margin, **kw)
        g[k] = np.where(real[:, None], gk, 0.0)
    return L, g


def loss_grad(D_node, flags, kinds=None, w_rel=0.0, margin=0.0, rel_kw=None, **kw):
    """the whole loss: box_guide_ref.loss_grad (a_o, a_r, a_a, tau, sel, region) + w_rel L_rel"""
    L, g = BR.loss_grad(D_node, flags, **kw)
    if kinds is not None and w_rel != 0:
        Lr, gr = rel_loss_grad(D_node, flags, kinds, margin, **(rel_kw or {}))
        L, g = L + w_rel * Lr, g + w_rel * gr
    return L, g


def guided_call(x_hat, D, flags, c, clip_ratio, mask_node=None, **kw):
    """box_guide_ref.guided_call with the relation term in the loss (kinds=, w_rel=, margin=)"""
    Dn = D[1]
    f = flags.astype(bool)
    L, g = loss_grad(Dn, flags, **kw)
    sh = float(c) * g
    if mask_node is not None:
        sh = np.where(np.asarray(mask_node)[..., -4:] != 0, 0.0, sh)
    sn = np.sqrt((sh ** 2).reshape(f.shape[0], -1).sum(1))
    if clip_ratio is None:
        rn, fac = np.zeros_like(sn), np.ones_like(sn)
    else:
        rn = BR.graph_norm(np.where((f[:, None, :, None] & f[:, None, None, :]), x_hat[0].astype(np.float64) - D[0], 0.0),
                           np.where(f[:, :, None], x_hat[1].astype(np.float64) - Dn, 0.0), flags)
        fac = BR.clip_factor(sn, rn, clip_ratio)
    sh = sh * fac[:, None, None]
    G = np.where(f[:, :, None], Dn.astype(np.float64), 0.0)
    G[..., -4:] -= sh
    return dict(loss=L, grad=g, shift=sh, factor=fac, norms=np.stack([sn, rn], 1), D_guided=G)


# ---- the decode rules (dsg_decode's, on one float32 adjacency estimate [B, C, N, N]) ----
def decode_predicates(adj, encoding, n_type):
    """[B, N, N] int64; entries that are not live are decoded like any other here (the callers select them away)"""
    a = np.asarray(adj, dtype=np.float32)
    C = a.shape[1]
    with np.errstate(invalid="ignore"):
        if encoding == "bits":      # > 0 is bit 1, channel 0 the most significant, clamped to n_type - 1
            v = np.zeros(a[:, 0].shape, np.int64)
            for c in range(C):
                v = (v << 1) | (a[:, c] > 0)
            return np.minimum(v, n_type - 1)
        if encoding == "one_hot":   # the first channel > 0, else 0
            v = np.zeros(a[:, 0].shape, np.int64)
            for c in range(C - 1, -1, -1):
                v = np.where(a[:, c] > 0, c, v)
            return v
        assert encoding == "ddpm" and C == 1
        x = np.clip(a[:, 0], np.float32(-1), np.float32(1))
        out = np.full(x.shape, -1, np.int64)    # a NaN matches no interval
        L = 2.0 / (n_type - 1)                  # Python floats: double
        for i in range(n_type):
            center = -1.0 + i * L
            lo = np.float32(-np.inf) if i == 0 else np.float32(center - L * 0.5)
            hi = np.float32(np.inf) if i == n_type - 1 else np.float32(center + L * 0.5)
            out = np.where((x > lo) & (x <= hi), i, out)
        return out


def kinds_of_predicates(pred, flags, pred_kind):
    """uint8 [B, N, N]: pred_kind[pred] at live pairs with a predicate inside the table, 0 elsewhere"""
    f = flags.astype(bool)
    N = f.shape[1]
    t = np.asarray(pred_kind, dtype=np.uint8)
    live = f[:, :, None] & f[:, None, :] & ~np.eye(N, dtype=bool)[None]
    ok = live & (pred >= 0) & (pred < t.size)
    return np.where(ok, t[np.clip(pred, 0, t.size - 1)], 0).astype(np.uint8)


def decoded_kinds(adj, flags, pred_kind, encoding):
    return kinds_of_predicates(decode_predicates(adj, encoding, len(pred_kind)), flags, pred_kind)
