"""CPU: the relation term of box guidance (dsg_sample_guided_rel) without a device -- the new symbols, the NumPy float64
restatement (tests/box_rel_ref.py) against torch float64 autograd of guide.box_relation_loss, pairs exactly on a hinge, the three
decode rules, every refusal of the Python surface and of the C entries (they refuse before any device use), and a power check: nine
plausible mistakes each move the gradient beyond ten times the loosest bar the GPU tests (tests/test_box_rel.py) use."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import box_rel_ref as RR
from test_box_guide_host import LOSSES, case
from diffusesg_amd import guide as G
from diffusesg_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dsg_sample_guided_rel", "dsg_debug_box_guide_rel")
LOOSEST_BAR = 1e-4   # the T = 8 trajectory bar; the kernel and the loop-arithmetic bars (about 1e-6) are tighter
MARGIN = 0.05
W_REL = 1.1


def test_new_symbols_declared_exported_loadable():
    hdr = open(os.path.join(ROOT, "include", "dsg.h")).read()
    bench_hdr = open(os.path.join(ROOT, "include", "dsg_debug.h")).read()
    L = lib.load()
    for name in NEW:
        bench = name.startswith("dsg_debug_")   # the kernel's own hook is declared with the test bench
        assert name + "(" in (bench_hdr if bench else hdr) and name in (lib.DEBUG_EXPORTS if bench else lib.EXPORTS)
        getattr(L, name)
    assert "typedef struct dsg_rel_cfg" in hdr and "DSG_REL_GIVEN 0" in hdr and "DSG_REL_DECODED 1" in hdr
    assert int(L.dsg_abi_version()) == lib.ABI_VERSION
    assert C.sizeof(lib.DsgRelCfg) == 40   # two floats, four int32, two pointers: no padding
    assert C.sizeof(lib.DsgGuideCfg) == 48   # untouched
    names = ("NONE", "LEFT_OF", "RIGHT_OF", "ABOVE", "BELOW", "INSIDE", "CONTAINS", "ON")
    for k, name in enumerate(names):
        assert getattr(G, "REL_" + name) == k == getattr(lib, "REL_" + name) == getattr(RR, name)
        assert f"#define DSG_REL_{name} {k}" in hdr


# ---- cases ----
def rel_kinds(flags, seed, which):
    """[B, N, N] uint8 kinds over the WHOLE grid -- padded rows, padded columns and the diagonal carry kinds too, which must not count.
    which: a kind 1..7 (that kind alone on about half of the pairs) or 'mixed' (all kinds, each ordered pair on its own)"""
    rng = np.random.default_rng(seed + 500)
    B, N = flags.shape
    if which == "mixed":
        return rng.integers(0, RR.KINDS, (B, N, N)).astype(np.uint8)
    return np.where(rng.random((B, N, N)) < 0.5, int(which), 0).astype(np.uint8)


WHICH = list(range(1, RR.KINDS)) + ["mixed"]


def rel_guide_of(kw, sel, region, kinds, w_rel=W_REL, margin=MARGIN):
    return G.BoxGuide(overlap=kw.get("a_o", 0.0), align=kw.get("a_a", 0.0), tau=kw.get("tau", 0.05), region_weight=kw.get("a_r", 0.0),
                      region=(torch.from_numpy(sel), torch.from_numpy(region)) if kw.get("a_r", 0.0) else None,
                      relations=None if kinds is None else torch.from_numpy(kinds), relation_weight=w_rel, relation_margin=margin)


def torch_loss_grad(D, flags, sel, region, kw, kinds, dtype, w_rel=W_REL, margin=MARGIN):
    """per-graph loss and dL/dD at the box channels by torch autograd of BoxGuide.torch_loss (with relations), graph by graph"""
    B = D.shape[0]
    L, g = np.zeros(B), np.zeros(D.shape[:2] + (4,))
    for b in range(B):
        fl = torch.from_numpy(flags[b:b + 1])
        x = torch.tensor(D[b:b + 1], dtype=dtype, requires_grad=True)
        val = rel_guide_of(kw, sel[b:b + 1], region[b:b + 1], None if kinds is None else kinds[b:b + 1], w_rel, margin).torch_loss(fl)(None, x)
        gx, = torch.autograd.grad(val, x, allow_unused=True)
        L[b] = float(val.detach())
        g[b] = 0.0 if gx is None else gx[0, :, -4:].double().numpy()
        assert gx is None or float(gx[0, :, :-4].abs().sum()) == 0.0
    return L, g


# ---- the restatement against torch float64 autograd ----
@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("N,c_node,valid", [(1, 4, [1, 0, 1]), (2, 5, [2, 0, 1]), (8, 12, [8, 2, 1]), (8, 4, [0, 5, 8])])
def test_restatement_against_torch_float64(which, N, c_node, valid):
    D, flags, sel, region = case(N, c_node, valid, seed=N)
    kinds = rel_kinds(flags, N, which)
    L, g = RR.rel_loss_grad(D, flags, kinds, MARGIN)
    Lt, gt = torch_loss_grad(D, flags, sel, region, {}, kinds, torch.float64, w_rel=1.0)
    assert np.abs(L - Lt).max() <= 1e-12 * max(1.0, np.abs(Lt).max())
    assert np.abs(g - gt).max() <= 1e-12 * max(1.0, np.abs(gt).max())
    assert (g[flags == 0] == 0).all()
    if N >= 8:
        assert np.abs(g).max() > 0 and L.max() > 0
    if N == 1:
        assert (L == 0).all() and (g == 0).all()   # one node: no pair, whatever sits on the diagonal


def test_restatement_with_the_other_three_losses_and_the_closure_alone():
    D, flags, sel, region = case(8, 5, [8, 5, 3], seed=21)
    kinds = rel_kinds(flags, 21, "mixed")
    kw = LOSSES["all"]
    L, g = RR.loss_grad(D, flags, kinds=kinds, w_rel=W_REL, margin=MARGIN, sel=sel, region=region, **kw)
    Lt, gt = torch_loss_grad(D, flags, sel, region, kw, kinds, torch.float64)
    assert np.abs(L - Lt).max() <= 1e-12 * np.abs(Lt).max() and np.abs(g - gt).max() <= 1e-12 * np.abs(gt).max()
    # box_relation_loss on its own, the whole batch at once, equals the sum over the graphs; without flags every node takes part
    x = torch.tensor(D, requires_grad=True)
    a = G.box_relation_loss(torch.from_numpy(kinds), torch.from_numpy(flags), MARGIN)(None, x)
    a = a.detach()
    assert abs(float(a) - RR.rel_loss_grad(D, flags, kinds, MARGIN)[0].sum()) <= 1e-12 * float(a)
    b = G.box_relation_loss(torch.from_numpy(kinds), None, MARGIN)(None, x).detach()
    assert abs(float(b) - RR.rel_loss_grad(D, np.ones_like(flags), kinds, MARGIN)[0].sum()) <= 1e-12 * float(b) and float(b) > float(a)


def test_restatement_ignores_what_is_not_live():
    D, flags, sel, region = case(8, 5, [8, 5, 3], seed=3)
    kinds = rel_kinds(flags, 3, "mixed")
    Dn = D.copy()
    Dn[flags == 0] = np.nan
    f = flags.astype(bool)
    live = f[:, :, None] & f[:, None, :] & ~np.eye(8, dtype=bool)[None]
    a, b, c = (RR.rel_loss_grad(d, flags, k, MARGIN) for d, k in ((D, kinds), (Dn, kinds), (D, np.where(live, kinds, 0))))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    assert (kinds[~live] != 0).any()
    big = np.where(live, kinds, 0).astype(np.int64)
    big[0, 0, 1] = 8                              # kinds above 7 count as none
    none = big.copy()
    none[0, 0, 1] = 0
    assert np.array_equal(RR.rel_loss_grad(D, flags, big, MARGIN)[1], RR.rel_loss_grad(D, flags, none, MARGIN)[1])


# ---- pairs exactly on a hinge ----
def hinge_case(c_node=5):
    """(D [1, 8, c_node], flags, kinds, margin): every set pair sits exactly on its hinge in float32 and in float64 -- all values are
    small binary fractions.  Box (cx, cy, w, h) -> D = 2 b - 1."""
    m = 0.25
    boxes = np.array([[0.25, 0.25, 0.25, 0.25],     # 0
                      [0.5, 0.25, 0.25, 0.25],      # 1: cx_0 - cx_1 + m = 0: 0 LEFT_OF 1, 1 RIGHT_OF 0
                      [0.25, 0.5, 0.25, 0.25],      # 2: cy_0 - cy_2 + m = 0: 0 ABOVE 2, 2 BELOW 0
                      [0.25, 0.25, 0.25, 0.25],     # 3: identical to 0: 3 INSIDE 0 and 3 CONTAINS 0, every side on its hinge
                      [0.5, 0.5, 0.5, 0.25],        # 4: top = 0.375 = bottom of 0, left = 0.25 = cx_0: 0 ON 4
                      [0.75, 0.75, 0.125, 0.125],   # 5
                      [0.5, 0.5, 0.75, 0.75],       # 6: 5 INSIDE 6 and 6 CONTAINS 1, satisfied with room to spare or on a hinge
                      [0.0, 0.0, 0.0, 0.0]])        # 7: padded
    D = np.zeros((1, 8, c_node))
    D[0, :, -4:] = boxes * 2.0 - 1.0
    flags = np.array([[1, 1, 1, 1, 1, 1, 1, 0]], np.uint8)
    K = np.zeros((1, 8, 8), np.uint8)
    for i, j, k in ((0, 1, RR.LEFT_OF), (1, 0, RR.RIGHT_OF), (0, 2, RR.ABOVE), (2, 0, RR.BELOW), (3, 0, RR.INSIDE), (0, 3, RR.CONTAINS),
                    (0, 4, RR.ON), (5, 6, RR.INSIDE), (6, 1, RR.CONTAINS)):
        K[0, i, j] = k
    return D, flags, K, m


def test_pairs_on_a_hinge_give_exactly_zero():
    D, flags, K, m = hinge_case()
    L, g = RR.rel_loss_grad(D, flags, K, m)
    assert L[0] == 0.0 and (g == 0.0).all()
    for dtype in (torch.float64, torch.float32):
        x = torch.tensor(D, dtype=dtype, requires_grad=True)
        val = G.box_relation_loss(torch.from_numpy(K), torch.from_numpy(flags), m)(None, x)
        gx, = torch.autograd.grad(val, x)
        assert float(val.detach()) == 0.0 and float(gx.abs().max()) == 0.0, dtype
    # and the case does sit on the hinges: the smallest margin above it, or the relation reversed, is felt at once
    assert RR.rel_loss_grad(D, flags, K, m + 2.0 ** -20)[0][0] > 0
    assert RR.rel_loss_grad(D, flags, np.transpose(K, (0, 2, 1)), m)[0][0] > 0


# ---- the decode rules ----
def decode_case(encoding, N, seed, valid=None):
    """(adj float32 [3, C, N, N], flags, pred_kind, n_type): random values with entries of exactly 0.0, -0.0 and NaN among the live
    ones; bits: 6 channels for 51 types (codes 51..63 clamp), one_hot: 7 channels, ddpm: one channel, k = 7 (interval ends included)"""
    C, k = {"bits": (6, 51), "one_hot": (7, 7), "ddpm": (1, 7)}[encoding]
    rng = np.random.default_rng(seed)
    B = 3
    a = rng.uniform(-1.3, 1.3, (B, C, N, N)).astype(np.float32)
    if encoding == "bits":
        a[:, :2][np.broadcast_to(rng.random((B, 1, N, N)) < 0.5, (B, 2, N, N))] = 0.7   # both leading bits set: codes >= 48, many above 50
    if encoding == "ddpm":   # the interval ends as the rule forms them, and their float32 neighbours
        L = 2.0 / (k - 1)
        ends = np.array([np.float32(-1.0 + i * L + s * L * 0.5) for i in range(k) for s in (-1, 1)], np.float32)
        ends = np.concatenate([ends, np.nextafter(ends, np.float32(2)), np.nextafter(ends, np.float32(-2))])
        pick = rng.random((B, N, N)) < 0.4
        a[:, 0][pick] = rng.choice(ends, int(pick.sum()))
    for val in (0.0, -0.0, np.nan):
        a[rng.random(a.shape) < 0.08] = val
    valid = valid or [N, max(N - 1, 1) if N > 2 else 2, min(2, N)]
    flags = np.zeros((B, N), np.uint8)
    for b, v in enumerate(valid):
        flags[b, :v] = 1
    pred_kind = rng.integers(0, RR.KINDS, k).astype(np.uint8)
    pred_kind[0] = 0
    return a, flags, pred_kind, k


@pytest.mark.parametrize("N", [2, 8])
@pytest.mark.parametrize("encoding", ["bits", "one_hot", "ddpm"])
def test_decoded_kinds_follow_the_restated_decode(encoding, N):
    a, flags, pred_kind, k = decode_case(encoding, N, seed=N)
    f = flags.astype(bool)
    live = f[:, :, None] & f[:, None, :] & ~np.eye(N, dtype=bool)[None]
    lv = np.broadcast_to(live[:, None], a.shape)
    if N >= 8:
        assert (lv & (a == 0) & ~np.signbit(a)).any() and (lv & (a == 0) & np.signbit(a)).any() and (lv & np.isnan(a)).any(), \
            "0.0, -0.0 and NaN must all occur at live entries"
    rules = G.SpatialRules(pred_kind, k, encoding)
    pred = RR.decode_predicates(a, encoding, k)
    want = pred_kind[np.clip(pred, 0, k - 1)] * (live & (pred >= 0))
    assert np.array_equal(RR.decoded_kinds(a, flags, pred_kind, encoding), want)
    for src in (torch.from_numpy(a), torch.from_numpy(a).double()):
        got = G.decoded_relation_kinds(src, torch.from_numpy(flags), rules)
        assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want)
    assert np.array_equal(G.relation_kinds_from_graph(torch.from_numpy(pred), torch.from_numpy(flags), pred_kind).numpy(), want)
    if encoding == "bits" and N >= 8:
        raw = sum((a[:, c] > 0).astype(np.int64) << (5 - c) for c in range(6))
        assert (raw[live] > 50).any() and pred.max() == 50                      # codes 51..63 clamp
    if encoding == "ddpm":
        assert ((pred == -1) == np.isnan(a[:, 0])).all()                       # NaN: none
        if N >= 8:
            assert set(np.unique(pred[live])) >= set(range(k))
    if encoding == "one_hot" and N >= 8:
        assert ((a > 0).sum(1)[live] == 0).any() and ((a > 0).sum(1)[live] > 1).any()   # no positive channel, several


def test_decoded_closure_equals_the_given_closure_and_has_no_adjacency_gradient():
    a, flags, pred_kind, k = decode_case("bits", 8, seed=4)
    D, _f, _s, _r = case(8, 12, [8, 7, 2], seed=4)
    rules = G.SpatialRules(pred_kind, k, "bits")
    fl = torch.from_numpy(flags)
    xa = torch.tensor(np.nan_to_num(a).astype(np.float64), requires_grad=True)
    xn = torch.tensor(D, requires_grad=True)
    kinds = RR.decoded_kinds(xa.detach().numpy(), flags, pred_kind, "bits")
    dec = G.BoxGuide(relations=rules, relation_margin=MARGIN).torch_loss(fl)(xa, xn)
    giv = G.BoxGuide(relations=torch.from_numpy(kinds), relation_margin=MARGIN).torch_loss(fl)(None, xn)
    assert float(dec) == float(giv) > 0
    ga, gn = torch.autograd.grad(dec, (xa, xn), allow_unused=True)
    assert ga is None and float(gn[..., :-4].abs().sum()) == 0 and float(gn.abs().max()) > 0   # no gradient through the thresholds


# ---- refusals ----
def test_python_surface_refusals():
    ok = np.zeros(51, np.uint8)
    for bad in (dict(pred_kind=ok, n_adj_type=51, encoding="int"), dict(pred_kind=ok, n_adj_type=0), dict(pred_kind=ok, n_adj_type=50),
                dict(pred_kind=np.full(51, 8), n_adj_type=51), dict(pred_kind=np.full(51, -1), n_adj_type=51),
                dict(pred_kind=np.zeros(51, np.float32), n_adj_type=51), dict(pred_kind=np.zeros((51, 1), np.uint8), n_adj_type=51)):
        with pytest.raises(ValueError):
            G.SpatialRules(**bad)
    K = torch.zeros(3, 8, 8, dtype=torch.uint8)
    for bad in (dict(kinds=K, margin=-0.1), dict(kinds=K, margin=float("nan")), dict(kinds=K, margin=float("inf")), dict(kinds=K.float()),
                dict(kinds=K[0]), dict(kinds=K[:, :, :7]), dict(kinds=K + 8), dict(kinds=K.bool()), dict(kinds=K.to(torch.int64) - 1)):
        with pytest.raises(ValueError):
            G.box_relation_loss(**bad)
    x = torch.zeros(3, 16, 5)
    with pytest.raises(ValueError):
        G.box_relation_loss(K)(None, x)                                              # kinds of another N
    with pytest.raises(ValueError):
        G.box_relation_loss(G.SpatialRules(ok, 51))(None, torch.zeros(3, 8, 5))      # decoded kinds without D_adj
    with pytest.raises(ValueError):
        G.box_relation_loss(G.SpatialRules(ok, 51))(torch.zeros(3, 5, 8, 8), torch.zeros(3, 8, 5))   # 51 types do not fit 5 bits
    with pytest.raises(ValueError):
        G.box_relation_loss(G.SpatialRules(ok[:7], 7, "one_hot"))(torch.zeros(3, 6, 8, 8), torch.zeros(3, 8, 5))
    with pytest.raises(ValueError):
        G.box_relation_loss(G.SpatialRules(ok[:7], 7, "ddpm"))(torch.zeros(3, 2, 8, 8), torch.zeros(3, 8, 5))
    with pytest.raises(TypeError):
        G.decoded_relation_kinds(torch.zeros(3, 6, 8, 8), None, ok)
    with pytest.raises(ValueError):
        G.relation_kinds_from_graph(torch.zeros(3, 8, dtype=torch.int64), None, ok)
    for bad in (dict(relations=K, relation_weight=float("nan")), dict(relations=K, relation_weight=float("inf")),
                dict(relations=K, relation_margin=-1.0), dict(relations=K, relation_margin=float("nan")), dict(relations=K + 8),
                dict(relations=K.float()), dict(relations=K[0])):
        with pytest.raises(ValueError):
            G.BoxGuide(**bad)
    with pytest.raises(ValueError):
        G.BoxGuide(relations=K).relation_descriptor(3, 16, "cpu", 6)                 # kinds of the wrong shape for the batch
    with pytest.raises(ValueError):
        G.BoxGuide(relations=K).relation_descriptor(2, 8, "cpu", 6)
    with pytest.raises(ValueError):
        G.BoxGuide(relations=G.SpatialRules(ok, 51)).relation_descriptor(3, 8, "cpu", 5)
    # what is accepted, and what it describes
    assert G.BoxGuide(overlap=1.0).relation_descriptor(3, 8, "cpu", 6) == (None, None)
    assert G.BoxGuide(relations=K, relation_weight=0.0).relation_descriptor(3, 8, "cpu", 6)[0].w_rel == 0.0   # the library then runs without the term
    r, keep = G.BoxGuide(relations=K + 3, relation_weight=2.0, relation_margin=0.125).relation_descriptor(3, 8, "cpu", 6)
    assert (r.w_rel, r.margin, r.source) == (2.0, 0.125, lib.REL_GIVEN) and r.kinds == keep.data_ptr() and keep.dtype == torch.uint8
    assert keep.shape == (3, 8, 8) and int(keep.min()) == 3
    r, keep = G.BoxGuide(relations=G.SpatialRules(ok + 7, 51)).relation_descriptor(3, 8, "cpu", 6)
    assert (r.w_rel, r.margin, r.source, r.encoding, r.n_adj_type) == (1.0, 0.0, lib.REL_DECODED, 0, 51)
    assert r.pred_kind == keep.ctypes.data and keep.dtype == np.uint8 and keep.tolist() == [7] * 51
    g, _keep = G.BoxGuide(overlap=2.0, relations=K).descriptor(3, 8, "cpu", None)    # the guide descriptor is what it was
    assert (g.w_overlap, g.w_region, g.w_align) == (2.0, 0.0, 0.0)


def _gcfg(o=1.0):
    return lib.DsgGuideCfg(o, 0.0, 0.0, 0.05, 1.0, 0, None, None, None)


def _rcfg(w=1.0, margin=0.0, source=0, encoding=0, n=51, kinds=None, table=None):
    return lib.DsgRelCfg(w, margin, source, encoding, n, 0, kinds, table)


_TAB51 = np.zeros(51, np.uint8)
_TAB8 = np.array([0, 1, 2, 8, 3, 4, 5], np.uint8)
_PT = lambda a: a.ctypes.data


@pytest.mark.parametrize("what,c_adj,c_node,rcfg,word", [
    ("NaN w_rel", 6, 4, _rcfg(w=float("nan"), kinds=64), "w_rel"),
    ("infinite w_rel", 6, 4, _rcfg(w=float("-inf"), kinds=64), "w_rel"),
    ("negative margin", 6, 4, _rcfg(margin=-0.01, kinds=64), "margin"),
    ("NaN margin", 6, 4, _rcfg(margin=float("nan"), kinds=64), "margin"),
    ("negative margin with w_rel = 0", 6, 4, _rcfg(w=0.0, margin=-1.0), "margin"),
    ("source 2", 6, 4, _rcfg(source=2, kinds=64, table=_PT(_TAB51)), "source"),
    ("source -1", 6, 4, _rcfg(source=-1, kinds=64, table=_PT(_TAB51)), "source"),
    ("given without kinds", 6, 4, _rcfg(), "kinds"),
    ("decoded without a table", 6, 4, _rcfg(source=1), "pred_kind"),
    ("decoded with n_adj_type = 0", 6, 4, _rcfg(source=1, n=0, table=_PT(_TAB51)), "n_adj_type"),
    ("decoded with a negative n_adj_type", 6, 4, _rcfg(source=1, n=-3, table=_PT(_TAB51)), "n_adj_type"),
    ("a table entry above 7", 3, 4, _rcfg(source=1, n=7, table=_PT(_TAB8)), "pred_kind[3]"),
    ("an unknown encoding", 6, 4, _rcfg(source=1, encoding=3, table=_PT(_TAB51)), "encoding"),
    ("a negative encoding", 6, 4, _rcfg(source=1, encoding=-1, table=_PT(_TAB51)), "encoding"),
    ("bits that do not hold the types", 5, 4, _rcfg(source=1, table=_PT(_TAB51)), "adjacency channels"),
    ("one_hot with another channel count", 6, 4, _rcfg(source=1, encoding=1, n=7, table=_PT(_TAB51)), "adjacency channels"),
    ("ddpm with two channels", 2, 4, _rcfg(source=1, encoding=2, n=7, table=_PT(_TAB51)), "adjacency channels"),
    ("what the hook without relations refuses: C_node < 4", 6, 3, _rcfg(kinds=64), "C_node"),
    ("past the descriptors: a null tensor", 6, 4, _rcfg(kinds=64), "null argument"),
    ("past the descriptors, decoded: a null tensor", 6, 4, _rcfg(source=1, table=_PT(_TAB51)), "null argument"),
])
def test_kernel_entry_refuses_before_any_launch(what, c_adj, c_node, rcfg, word):
    """every tensor pointer is NULL: a call that got past its argument checks would fail differently (or crash); the refusal names the
    argument"""
    L = lib.load()
    nul = [None] * 6
    rc = L.dsg_debug_box_guide_rel(3, 8, c_adj, c_node, *nul, C.byref(_gcfg()), 1.0, *nul, None, C.byref(rcfg), None)
    assert rc == lib.DSG_ERR_INVALID, what
    assert word in L.dsg_last_error(None).decode(), (what, L.dsg_last_error(None))


def test_entries_refuse_a_missing_guide_and_a_missing_handle():
    L = lib.load()
    nul = [None] * 6
    assert L.dsg_debug_box_guide_rel(3, 8, 6, 4, *nul, None, 1.0, *nul, None, C.byref(_rcfg(kinds=64)), None) == lib.DSG_ERR_INVALID
    assert L.dsg_debug_box_guide_rel(3, 65, 6, 4, *nul, C.byref(_gcfg()), 1.0, *nul, None, None, None) == lib.DSG_ERR_INVALID
    assert "64" in L.dsg_last_error(None).decode()
    # decoded source without a clip, a good table, every tensor NULL
    g = _gcfg()
    g.clip_ratio = lib.GUIDE_CLIP_NONE
    assert L.dsg_debug_box_guide_rel(3, 8, 6, 4, *nul, C.byref(g), 1.0, *nul, None, C.byref(_rcfg(source=1, table=_PT(_TAB51))), None) == lib.DSG_ERR_INVALID
    scfg = lib.make_sampler_cfg(8, "euler", 0.0)
    args = [None, C.byref(scfg), None, 3, None, None, 0] + [None] * 12 + [0, None, None, C.byref(_gcfg()), None, None, None, None, None, None, None]
    assert L.dsg_sample_guided_rel(*args, C.byref(_rcfg(kinds=64))) == lib.DSG_ERR_INVALID   # no handle: nothing to run on


# ---- power: what the bars can see ----
def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_mistakes_move_the_gradient_beyond_the_bars():
    D, flags, sel, region = case(8, 5, [8, 5, 3], seed=11)
    kinds = rel_kinds(flags, 11, "mixed")
    kinds[:, np.arange(8), np.arange(8)] = RR.ON          # a counted diagonal is felt through ON's plain square: (bt_i - t_i)^2 = h_i^2
    kw = LOSSES["all"]
    full = lambda **rel_kw: RR.loss_grad(D, flags, kinds=kinds, w_rel=W_REL, margin=MARGIN, rel_kw=rel_kw, sel=sel, region=region, **kw)[1]
    g = full()
    one_way = np.triu(kinds, 1)                           # only (i, j), i < j, is set
    g_one = RR.loss_grad(D, flags, kinds=one_way, w_rel=W_REL, margin=MARGIN, sel=sel, region=region, **kw)[1]
    moved = {
        "subject and object exchanged": _rel(full(swap=True), g),
        "the y axis flipped": _rel(full(flip_y=True), g),
        "the margin's sign": _rel(full(margin_sign=-1.0), g),
        "the 0.5 of * 0.5 + 0.5 dropped": _rel(full(half=False), g),
        "padded nodes counted": _rel(full(count_padded=True), g),
        "the diagonal counted": _rel(full(count_diag=True), g),
        "a pair counted for (j, i) when only (i, j) is set": _rel(
            RR.loss_grad(D, flags, kinds=one_way, w_rel=W_REL, margin=MARGIN, rel_kw=dict(symmetric=True), sel=sel, region=region, **kw)[1], g_one),
        "CONTAINS treated as INSIDE": _rel(full(contains_as_inside=True), g),
        "ON's plain square hinged": _rel(full(on_hinged=True), g),
    }
    # the guided estimate of one call at a middle noise level moves with the gradient: D~ - D = -c g
    t = float(lib.sigma_schedule(lib.make_sampler_cfg(8, "euler", 0.0))[1][4])
    import box_guide_ref as BR
    c = float(BR.coef(1.5, t))
    f = flags.astype(bool)
    Dn = np.where(f[:, :, None], D, 0.0)
    Da = np.zeros((3, 2, 8, 8))
    right = RR.guided_call((Da, Dn), (Da, Dn), flags, c, None, kinds=kinds, w_rel=W_REL, margin=MARGIN, sel=sel, region=region, **kw)
    wrong = RR.guided_call((Da, Dn), (Da, Dn), flags, c, None, kinds=kinds, w_rel=W_REL, margin=MARGIN, rel_kw=dict(swap=True), sel=sel,
                           region=region, **kw)
    moved["subject and object exchanged, in the guided estimate"] = _rel(wrong["D_guided"], right["D_guided"])
    for what, d in moved.items():
        print(f"BOXREL power: {what}: {d:.3e} of the tensor's maximum (loosest bar {LOOSEST_BAR:.0e})")
        assert d > 10 * LOOSEST_BAR, what
