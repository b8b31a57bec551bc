"""CPU: content guidance (dsg_sample_guided_content) without a GPU -- the float64 restatement of tests/content_ref.py
against float64 torch autograd of guide.py's closure, `label_codes` against the formulas of include/dsg.h, the two properties of the
loss (a step against the gradient lowers it; L_k -> min d_k as tau -> 0), `items_present`, and the mistake switches of the reference:
each of them moves some output beyond the bar the GPU tests hold the kernel to."""
import numpy as np
import pytest
import torch

import content_ref as CR
from diffusesg_amd import guide as G

SHAPES = [(1, 5, 1), (3, 12, 8), (6, 12, 8), (7, 14, 7), (51, 154, 150)]   # (C_adj, C_node, Cl)


def make_flags(N, valid):
    """valid: per graph an int (a prefix of that many nodes) or ('s', n): n nodes scattered over the slots"""
    f = np.zeros((len(valid), N), np.uint8)
    for b, v in enumerate(valid):
        if isinstance(v, tuple):
            f[b, np.random.default_rng(100 + b + v[1]).permutation(N)[:min(v[1], N)]] = 1
        else:
            f[b, :min(v, N)] = 1
    return f


def valid_sets(N):
    """all, a prefix, scattered, one node, none"""
    return [N, max(N - 3, min(N, 2)), ("s", max(N // 2, min(N, 2))), 1, 0]


def case(N, Ca, Cn, Cl, K, valid, seed, tau=1.0, w=1.3, clip=1.0, nan=True, with_mask=False, xh_scale=None):
    """One guided call: float32 x_hat and D near +-1 codes, K items per graph of which some are inactive, some unary, some predicate-only;
    NaN (nan=True) in every padded row and column of D and x_hat, and on the adjacency diagonal of both where no clip reads it.  Returns (x_hat, D, flags, cfg, mask_adj, mask_node)"""
    rng = np.random.default_rng(seed)
    flags = make_flags(N, valid)
    B = flags.shape[0]
    Da = (np.sign(rng.standard_normal((B, Ca, N, N))) + 0.3 * rng.standard_normal((B, Ca, N, N))).astype(np.float32)
    Dn = (np.sign(rng.standard_normal((B, N, Cn))) + 0.3 * rng.standard_normal((B, N, Cn))).astype(np.float32)
    scale = np.ones(B) if xh_scale is None else np.asarray(xh_scale, np.float64)
    xa = (Da + scale[:, None, None, None] * rng.standard_normal(Da.shape)).astype(np.float32)
    xn = (Dn + scale[:, None, None] * rng.standard_normal(Dn.shape)).astype(np.float32)
    subj = np.sign(rng.standard_normal((B, K, Cl))).astype(np.float32)
    obj = np.sign(rng.standard_normal((B, K, Cl))).astype(np.float32)
    pred = np.sign(rng.standard_normal((B, K, Ca))).astype(np.float32)
    w_spo = rng.uniform(0.5, 1.5, (B, K, 3)).astype(np.float32)
    for k in range(K):          # item 1: inactive; item 2: unary; then predicate-only, object-only, the rest full triplets
        if k % 5 == 1:
            w_spo[:, k] = 0
        elif k % 5 == 2:
            w_spo[:, k, 1:] = 0
        elif k % 5 == 3:
            w_spo[:, k, :2] = 0
        elif k % 5 == 4:
            w_spo[:, k, 0] = 0
    if nan:
        pad = flags == 0
        dead = pad[:, None, :, None] | pad[:, None, None, :]
        diag = np.broadcast_to(np.eye(N, dtype=bool)[None, None], Da.shape)
        for v in (Da, xa):    # the clip's norm pass reads the diagonal of valid nodes: NaN there without a clip only
            v[np.broadcast_to(dead, v.shape) | (diag if clip is None else False)] = np.nan
        Dn[pad] = np.nan
        xn[pad] = np.nan
    cfg = dict(Cl=Cl, tau=tau, w=w, clip_ratio=clip, subj=subj, obj=obj, pred=pred, w_spo=w_spo)
    ma = (rng.random(Da.shape) < 0.3) if with_mask else None
    mn = (rng.random(Dn.shape) < 0.3) if with_mask else None
    return (xa, xn), (Da, Dn), flags, cfg, ma, mn


def clean(D, flags):
    """D with 0 where the kernel never reads: torch's closure selects the same entries away, this keeps NaN out of float32 copies"""
    f = flags.astype(bool)
    N = f.shape[1]
    live = f[:, :, None] & f[:, None, :] & ~np.eye(N, dtype=bool)[None]
    return np.where(live[:, None], D[0], 0.0), np.where(f[:, :, None], D[1], 0.0)


def torch_loss_grad(D, flags, cfg, dtype=torch.float64):
    """(loss summed over the batch, dL/dD_adj, dL/dD_node) of guide.content_loss by autograd"""
    Da, Dn = (torch.tensor(np.asarray(v, np.float64), dtype=dtype, requires_grad=True) for v in clean(D, flags))
    fn = G.content_loss(cfg["subj"], cfg["obj"], cfg["pred"], cfg["w_spo"], torch.from_numpy(flags), float(np.float32(cfg["tau"])))
    L = fn(Da, Dn)
    L.backward()
    return float(L.detach()), Da.grad.numpy().astype(np.float64), Dn.grad.numpy().astype(np.float64)


@pytest.mark.parametrize("tau", [0.01, 1.0])
@pytest.mark.parametrize("shape", SHAPES[:4] + [SHAPES[4] + (8,)])
def test_reference_gradient_against_torch_autograd(shape, tau):
    Ca, Cn, Cl = shape[:3]
    for N in ((shape[3],) if len(shape) > 3 else (1, 2, 8, 13)):
        xh, D, flags, cfg, _, _ = case(N, Ca, Cn, Cl, 6, valid_sets(N), seed=N + Ca, tau=tau)
        r = CR.content_loss_grad(D, flags, cfg)
        L, ga, gn = torch_loss_grad(D, flags, cfg)
        sa, sn = max(np.abs(ga).max(), 1e-300), max(np.abs(gn).max(), 1e-300)
        assert abs(r["loss"].sum() - L) <= 1e-11 * max(1.0, abs(L))
        assert np.abs(r["grad_adj"] - ga).max() <= 1e-10 * sa and np.abs(r["grad_label"] - gn[..., :Cl]).max() <= 1e-10 * sn
        assert (gn[..., Cl:] == 0).all(), "nothing outside the label channels"
        f = flags.astype(bool)
        assert (r["grad_label"][~f] == 0).all() and (r["grad_adj"][np.broadcast_to(~(f[:, None, :, None] & f[:, None, None, :]), ga.shape)] == 0).all()
        if N >= 2:
            assert np.abs(r["grad_adj"]).max() > 0 and np.abs(r["grad_label"]).max() > 0
        lone = f.sum(1) < 2
        assert (r["loss"][lone] == 0).all() and (r["grad_adj"][lone] == 0).all() and (r["grad_label"][lone] == 0).all() and (r["best"][lone] == -1).all()


def test_constructed_inputs():
    """a graph that contains the triplet exactly: d = 0 at that pair, the pair is `best`, L_k <= tau log P, and the pull on it vanishes;
    two slots at exactly the same distance share pi evenly"""
    N, Ca, Cl = 6, 6, 8
    ncode, pcode = G.label_codes(150, "bits", Cl), G.label_codes(51, "bits", Ca)
    rng = np.random.default_rng(0)
    qn = rng.integers(0, 150, N)
    qn[[2, 4]] = (17, 99)
    qa = rng.integers(0, 51, (N, N))
    qa[2, 4] = 33
    qa[qa == 33] = 32
    qa[2, 4] = 33
    Dn = np.concatenate([ncode[qn], np.zeros((N, 4), np.float32)], 1)[None]
    Da = pcode[qa].transpose(2, 0, 1)[None]
    flags = np.ones((1, N), np.uint8)
    cg = G.ContentGuide([[(17, 33, 99)]], 150, 51, tau=0.05)
    subj, obj, pred, w_spo = cg.tensors(Ca, Cl)
    cfg = dict(Cl=Cl, tau=0.05, subj=subj, obj=obj, pred=pred, w_spo=w_spo)
    r = CR.content_loss_grad((Da, Dn), flags, cfg)
    assert r["best"][0, 0].tolist() == [2, 4] and 0 <= r["loss"][0] <= float(np.float32(0.05)) * np.log(N * (N - 1)) * (1 + 1e-12)
    assert np.abs(r["grad_adj"][0, :, 2, 4]).max() == 0 and G.items_present(qa[None], qn[None], flags, cg.items).all()
    assert not G.items_present(qa[None], qn[None], flags, [[(17, 32, 99)]]).any() and G.items_present(qa[None], qn[None], flags, [[(None, 33, None)]]).all()
    assert not G.items_present(qa.T[None], qn[None], flags, cg.items).any(), "subject = row, object = column"
    # a tie: two nodes with the subject's label, object and predicate free -> the two rows share the weight evenly
    Dn2 = Dn.copy()
    Dn2[0, 0] = Dn2[0, 2]
    cfg1 = dict(cfg, w_spo=np.array([[[1.0, 0.0, 0.0]]], np.float32))
    r2 = CR.content_loss_grad((Da, Dn2), flags, cfg1)
    g = CR.graph_content(Dn2[0][:, :Cl], Da[0], flags[0], subj[0], obj[0], pred[0], cfg1["w_spo"][0], 0.05)
    assert r2["best"][0, 0].tolist() == [0, 1], "the lowest flat index among equals"
    assert np.array_equal(r2["grad_label"][0, 0], r2["grad_label"][0, 2])


def test_label_codes_against_the_header_formulas():
    for n_type, chans in ((150, 8), (51, 6), (2, 1), (7, 3)):
        c = G.label_codes(n_type, "bits", chans)
        assert c.dtype == np.float32 and c.shape == (n_type, chans)
        for q in range(n_type):
            assert [1.0 if (q >> (chans - 1 - k)) & 1 else -1.0 for k in range(chans)] == c[q].tolist()   # MSB first, 2 b - 1
    c = G.label_codes(7, "one_hot", 7)
    assert np.array_equal(c, 2 * np.eye(7, dtype=np.float32) - 1)
    c = G.label_codes(51, "ddpm", 1)
    assert c.shape == (51, 1) and all(c[i, 0] == np.float32(np.float32(2 * i) / np.float32(50)) - np.float32(1) for i in range(51))
    for bad in (("bits", 150, 7), ("one_hot", 7, 6), ("ddpm", 7, 2)):
        with pytest.raises(ValueError):
            G.label_codes(bad[1], bad[0], bad[2])
    with pytest.raises(ValueError):
        G.ContentGuide([[(150, None, None)]], 150, 51)
    with pytest.raises(ValueError):
        G.ContentGuide([[(1, 2, 3)] * 17], 150, 51)
    cg = G.ContentGuide([[(1, None, None)], []], 150, 51, term_weights=(2.0, 3.0, 4.0))
    s, o, p, w = cg.tensors(6, 8)
    assert w.tolist() == [[[2.0, 0.0, 0.0]], [[0.0, 0.0, 0.0]]] and np.array_equal(s[0, 0], G.label_codes(150, "bits", 8)[1]) and not o.any() and not p.any()


@pytest.mark.parametrize("tau", [0.01, 1.0])
def test_a_step_against_the_gradient_lowers_the_loss(tau):
    xh, D, flags, cfg, _, _ = case(8, 6, 12, 8, 4, [8, 5, ("s", 4)], seed=3, tau=tau)
    r = CR.content_loss_grad(D, flags, cfg)
    Da, Dn = clean(D, flags)
    for eps in (1e-3, 1e-5):
        Dn2 = Dn.astype(np.float64).copy()
        Dn2[..., :8] -= eps * r["grad_label"]
        r2 = CR.content_loss_grad((Da.astype(np.float64) - eps * r["grad_adj"], Dn2), flags, cfg)
        assert (r2["loss"] < r["loss"]).all()


def test_small_tau_is_the_minimum():
    xh, D, flags, cfg, _, _ = case(8, 6, 12, 8, 4, [8, 5], seed=4)
    for tau in (1.0, 1e-2, 1e-4, 1e-6):
        c = dict(cfg, tau=tau)
        r = CR.content_loss_grad(D, flags, c)
        for b in range(2):
            g = CR.graph_content(D[1][b][:, :8], D[0][b], flags[b], c["subj"][b], c["obj"][b], c["pred"][b], c["w_spo"][b], tau)
            P = g["n_pairs"]
            for k in range(4):
                if c["w_spo"][b, k].any():
                    i, j = g["best"][k]
                    s, o, p = c["subj"][b, k].astype(np.float64), c["obj"][b, k].astype(np.float64), c["pred"][b, k].astype(np.float64)
                    a = c["w_spo"][b, k].astype(np.float64)
                    dmin = a[0] * ((D[1][b, i, :8] - s) ** 2).sum() + a[1] * ((D[1][b, j, :8] - o) ** 2).sum() + a[2] * ((D[0][b, :, i, j] - p) ** 2).sum()
                    assert dmin - 1e-9 <= g["item_loss"][k] <= dmin + tau * np.log(P) + 1e-9
        assert np.isfinite(r["item_loss"]).all()


MISTAKES = ["swap_so", "count_diag", "count_padded", "no_mean", "obj_axis", "no_two", "ignore_mask", "shift_beyond", "no_max_sub"]


@pytest.mark.parametrize("mistake", MISTAKES)
def test_each_mistake_moves_an_output_beyond_the_bar(mistake):
    """the GPU test holds loss, item_loss and both gradients to content_ref.bars and shift / D~ to the bit: a restated mistake must
    leave one of them"""
    N, Ca, Cn, Cl, K = 8, 6, 14, 8, 6        # Cl < C_node - 4: channels between the labels and the box exist
    tau = 0.01 if mistake == "no_max_sub" else 1.0
    xh, D, flags, cfg, ma, mn = case(N, Ca, Cn, Cl, K, [8, 5, ("s", 4)], seed=11, tau=tau, nan=False, with_mask=True)
    good = CR.guided_call(xh, D, flags, 0.37, cfg, ma, mn)
    with np.errstate(all="ignore"):
        bad = CR.guided_call(xh, D, flags, 0.37, cfg, ma, mn, **{mistake: True})
    bars = CR.bars(good, cfg, N, Ca)
    worst = 0.0
    for k, bar in bars.items():
        with np.errstate(invalid="ignore"):
            e = np.abs(bad[k] - good[k]) / bar
        worst = max(worst, float(np.where(np.isfinite(e), e, np.inf).max()))
    for k in ("shift_adj", "shift_label", "D_guided_adj", "D_guided_node"):   # bit for bit on the GPU: any float32-visible change counts
        with np.errstate(invalid="ignore"):
            diff = bad[k].astype(np.float32) != good[k].astype(np.float32)
        worst = max(worst, np.inf if diff.any() else 0.0)
    assert worst > 1.0, (mistake, worst)
    for k, bar in bars.items():
        assert np.isfinite(bar).all() and (bar > 0).all() and (bar <= 1e-5 * max(1.0, np.abs(good[k]).max())).all(), k
