"""CPU: what tests/test_loss_kernels.py stands on.  The float64 autograd restatement of the training loss (tests/loss_ref.py) reproduces
tests/golden/iou_losses.npz, the reference project's own autograd; the CPU oracle (oracle/dsg_ref.c: dsgref_rainbow_loss and its backward,
whose box_term was derived by the same hand as the kernel's box_iou_term) is held to the GPU test's bars on every case; the case list
reaches every branch it was written for; the random family keeps float32 and float64 on one side of every comparison; every seeded
mistake lands outside the bars; and the objective's float32 arithmetic is bit-exact operation by operation, which a fused
multiply-add is not."""
import types

import numpy as np
import pytest

import loss_ref as R
from diffusesg_amd import synth as Y
from oracle.oracle import Oracle
from util import load

CASES = R.cases()


def make_oracle(N, Ca, Cn):
    """the loss entries of the oracle read the three tensor dimensions only"""
    cfg = types.SimpleNamespace(max_node_num=N, c_adj=Ca, c_node=Cn, embed_dim=96, num_layers=2, depths=(1, 1), num_heads=(3, 6),
                                window_size=1, mlp_ratio=4, self_condition=False)
    return Oracle(cfg, {})


def oracle_outputs(case, iou_type):
    s = case.spec
    orc = make_oracle(s.N, s.Ca, s.Cn)
    la, ln = orc.rainbow_loss(case.pred_adj, case.pred_node, case.tgt_adj, case.tgt_node, case.flags, case.weights, case.edge_w, case.node_w,
                              case.iou_w, iou_type=iou_type)
    ga, gn, fa, fn = orc.rainbow_loss_backward(case.pred_adj, case.pred_node, case.tgt_adj, case.tgt_node, case.flags, case.weights, case.edge_w,
                                               case.node_w, case.iou_w, sigmas=case.sigmas, iou_type=iou_type)
    return {"loss_adj": la, "loss_node": ln, "grad_adj": ga, "grad_node": gn, "grad_F_adj": fa, "grad_F_node": fn}


# ---- the restatement is the reference project's autograd ----------------------------------------------------------------------------
@pytest.mark.parametrize("iou_type", R.IOU_TYPES)
def test_reference_reproduces_the_fixture(iou_type):
    """the fixture is a float32 evaluation under the reference project's autograd: 32 float32 epsilons of the tensor's largest magnitude
    is its resolution over the few dozen operations of a box term (the oracle's own fixture test allows 2e-6 .. 1e-5)"""
    cfg, flags, pred_adj, pred_node, tgt_adj, tgt_node, wts, sigmas = Y.iou_case()
    g = load("iou_losses.npz")
    c = types.SimpleNamespace(pred_adj=pred_adj, pred_node=pred_node, tgt_adj=tgt_adj, tgt_node=tgt_node, flags=flags, weights=wts, sigmas=sigmas,
                              edge_w=float(g["edge_w"]), node_w=float(g["node_w"]), iou_w=float(g["iou_w"]))
    ref = R.evaluate(c, iou_type)
    bar = 32 * float(np.finfo(np.float32).eps)
    for key in ("loss_adj", "loss_node", "grad_adj", "grad_node"):
        e = R.rel_err(g[f"{iou_type}_{key}"], ref[key])
        print(f"LOSSK fixture {iou_type} {key}: rel err {e:.2e} (bar {bar:.2e})")
        assert e <= bar, (iou_type, key, e)
    e = R.rel_err(g[f"{iou_type}_grad_node"][..., -4:], ref["grad_node"][..., -4:])
    assert e <= bar, (iou_type, "box channels", e)
    ev, gap, _ = R.box_events(pred_node, tgt_node, flags)
    assert sum(ev[f"tie corner {t}"] for t in range(4)) == 0 and ev["edge-exact corner at 0"] + ev["edge-exact corner at 1"] == 0   # what it cannot see


# ---- the case list ------------------------------------------------------------------------------------------------------------------
def test_case_list_is_the_one_asked_for():
    sp = R.SPECS
    assert {(s.B, s.N, s.Ca, s.Cn) for s in sp} == {(1, 1, 1, 4), (4, 8, 6, 12), (3, 20, 3, 9), (2, 64, 6, 12), (2, 300, 1, 5)}
    for shape in R.SHAPES:
        assert {s.family for s in sp if (s.B, s.N, s.Ca, s.Cn) == shape} == {"random", "constructed"}
    assert {s.flags for s in sp} == {"ragged", "holes", "full"}
    for v in ("no_weight", "no_sigma", "iou_w0"):
        assert len({(s.B, s.N) for s in sp if s.variant == v}) >= 2
    for c in CASES:
        f = c.flags.astype(bool)
        assert f.sum(-1).min() >= 1
        if c.spec.flags == "holes":
            assert any((np.diff(r.astype(int)) == 1).any() for r in f)                       # a valid node after an invalid one
        if c.spec.flags == "full":
            assert f.all()
        assert (c.weights is None) == (c.spec.variant == "no_weight") and (c.sigmas is None) == (c.spec.variant == "no_sigma")
        assert (c.iou_w == 0.0) == (c.spec.variant == "iou_w0")
    assert any(c.flags.sum(-1).max() > 256 for c in CASES) and any((c.flags.sum(-1) == 1).any() and c.spec.N > 1 for c in CASES)


def test_case_list_reaches_every_branch():
    tot = {}
    for c in CASES:
        if c.iou_w == 0.0:
            continue
        ev, _, extent = R.box_events(c.pred_node, c.tgt_node, c.flags)
        assert extent.min() >= R.MIN_EXTENT, c.name
        for k, v in ev.items():
            tot[k] = tot.get(k, 0) + v
    print("LOSSK events over the case list:", tot)
    for k, v in tot.items():
        assert v >= 1, f"the case list no longer reaches: {k}"
    # every constructed box is met by a valid node of some case
    seen = set()
    for c in CASES:
        if c.spec.family == "constructed" and c.iou_w != 0.0:
            for what, p, g in R.CONSTRUCTED:
                hit = (c.pred_node[..., -4:] == np.float32(R._channels(p))).all(-1) & (c.tgt_node[..., -4:] == np.float32(R._channels(g))).all(-1)
                if (hit & c.flags.astype(bool)).any():
                    seen.add(what)
    assert seen == {w for w, _, _ in R.CONSTRUCTED}


def test_constructed_channels_are_exact():
    for what, p, g in R.CONSTRUCTED:
        for c in (p, g):
            ch = np.array(R._channels(c))
            assert (ch * 64 == np.round(ch * 64)).all(), what                                # multiples of 2^-6
            raw, _ = R.corners(ch.astype(np.float32))
            assert (raw * 32 == np.array(c, np.float64)).all(), what                         # the corners come back exactly


def test_random_family_keeps_every_comparison_apart():
    """float32 and float64 then take the same branch: the float32 evaluation of the reference differs by rounding alone"""
    for c in CASES:
        if c.spec.family == "random":
            ev, gap, extent = R.box_events(c.pred_node, c.tgt_node, c.flags)
            assert gap.min() > R.MARGIN and extent.min() >= R.MIN_EXTENT, (c.name, gap.min(), extent.min())
    tot = {}
    for c in CASES:
        if c.spec.family == "random" and c.iou_w != 0.0:
            for k, v in R.box_events(c.pred_node, c.tgt_node, c.flags)[0].items():
                tot[k] = tot.get(k, 0) + v
    for k in ("clamped corner", "disjoint", "prediction encloses target", "target encloses prediction"):
        assert tot[k] >= 1, k


def test_bars():
    b = R.bars()
    for fam, (bar, disc) in b.items():
        print(f"LOSSK bar {fam}: {bar:.3e} (float32 evaluation of the reference: {disc:.3e}; cap {R.FLOOR[fam]:.0e})")
        assert 0 < disc and bar <= R.FLOOR[fam] and bar == min(16 * disc, R.FLOOR[fam])


# ---- the oracle against float64 autograd -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iou_type", R.IOU_TYPES)
@pytest.mark.parametrize("case", CASES, ids=R.CASE_IDS)
def test_oracle_against_float64_autograd(case, iou_type):
    worst = R.compare(oracle_outputs(case, iou_type), R.reference(case, iou_type))
    print(f"LOSSK oracle {case.name} {iou_type}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for fam, r in worst.items():
        assert r <= 1.0, f"{case.name} {iou_type} {fam}: {r:.2f} x the bar {R.bars()[fam][0]:.2e}"


# ---- power --------------------------------------------------------------------------------------------------------------------------
MISTAKES = {
    "a tie given wholly to the prediction": dict(tie="whole"),
    "a tie dropped": dict(tie="drop"),
    "a tie dropped in type 0 alone (the parent commit)": dict(tie="drop", tie_types=("iou",)),
    "a clamp edge treated as exclusive": dict(clamp_exclusive=True),
    ">= in the open-intersection mask of types 1 to 4": dict(open_ge=True),
    "the IoU term divided by the graph's own node count": dict(per_graph_count=True),
    "a missing 1/B": dict(no_inv_b=True),
    "loss_weight left out of the IoU term": dict(no_iou_loss_weight=True),
    "n for n^2 in the adjacency term": dict(adj_n_not_n2=True),
    "a missing c_out": dict(no_c_out=True),
}


@pytest.mark.parametrize("what", sorted(MISTAKES))
def test_seeded_mistakes_land_outside_the_bars(what):
    kw = MISTAKES[what]
    best, where, caught = 0.0, None, set()
    for c in CASES:
        if c.spec.N > 64:
            continue
        for ty in R.IOU_TYPES:
            worst = R.compare(R.evaluate(c, ty, **kw), R.reference(c, ty))
            r = max(worst.values())
            if r > 1.0:
                caught.add(ty)
            if r > best:
                best, where = r, (c.name, ty, max(worst, key=worst.get))
    print(f"LOSSK power: {what}: {best:.3g} x the bar at {where}; types that see it: {sorted(caught)}")
    assert best > 10.0, what
    if "tie_types" in kw:
        assert caught == set(kw["tie_types"])
    if what == ">= in the open-intersection mask of types 1 to 4":
        assert caught == set(R.IOU_TYPES[1:])
    if what in ("a tie given wholly to the prediction", "a tie dropped", "a clamp edge treated as exclusive"):
        assert caught == set(R.IOU_TYPES)


# ---- the objective with replayed draws ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in CASES if c.spec.variant == "all"], ids=[c.name for c in CASES if c.spec.variant == "all"])
def test_oracle_train_inputs_bit_exact_from_its_sigmas(case):
    s = case.spec
    sig, wts, na, nx = make_oracle(s.N, s.Ca, s.Cn).train_inputs(case.tgt_adj, case.tgt_node, case.flags, case.rnd, case.eps_adj, case.eps_node)
    ref = R.sigma_reference(case.rnd)
    assert np.abs(sig - ref).max() <= 2e-6 * np.abs(ref).max() and (np.abs(sig - ref) <= 2e-6 * ref).all()
    w, a, x = R.train_inputs_from_sigmas(case, sig)
    for got, want in ((wts, w), (na, a), (nx, x)):
        assert np.array_equal(got.view(np.int32), want.view(np.int32))
    f = case.flags.astype(bool)
    assert (na[~np.broadcast_to(f[:, None, :, None] & f[:, None, None, :], na.shape)] == 0).all()
    assert np.array_equal(nx[~f].view(np.int32), case.tgt_node[~f].view(np.int32))


def test_a_fused_multiply_add_is_not_bit_exact():
    """what `rtol` 1e-6 could not see: with the product unrounded the noisy tensors differ in their last bit somewhere, at every shape with
    more than a few hundred elements"""
    n_diff = 0
    for case in CASES:
        if case.spec.variant != "all" or case.spec.N < 8:
            continue
        sig = R.sigma_reference(case.rnd).astype(np.float32)
        w, a, x = R.train_inputs_from_sigmas(case, sig)
        wf, af, xf = R.train_inputs_from_sigmas(case, sig, fused=True)
        f = case.flags.astype(bool)
        da, dx = int((a.view(np.int32) != af.view(np.int32)).sum()), int((x.view(np.int32) != xf.view(np.int32)).sum())
        assert da > 0 and dx > 0, case.name
        assert np.abs(a - af).max() <= 1e-6 * np.abs(a).max()                                # and it is inside the old tolerance
        assert np.array_equal(x[~f], xf[~f])
        n_diff += da + dx
    print(f"LOSSK fused multiply-add: {n_diff} elements differ in their bits")
