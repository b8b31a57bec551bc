"""GPU: the relation term of box guidance (dsg_sample_guided_rel).

1. the guide kernel's relation variant alone (dsg_debug_box_guide_rel) against the float64 restatement of tests/box_rel_ref.py, kinds
   given and decoded, NaN in every padded node row and, for the decoded source, in every adjacency entry that is not live;
2. the decoded source: the kinds the kernel used equal pred_kind[dsg_decode(D)] bit for bit, for the three encodings;
3. in the loop: without a relation term the new entry is dsg_sample_guided bit for bit, replayed bodies equal enqueued ones, the
   loop's arithmetic recomputed in float64 (sanity-check mode), the chain of dsg_precond calls, known and padded entries, batch
   invariance, layout_from_graph under the graph's own predicates, and the eager loop on a network whose Jacobian is exactly zero.

Kernel bar: tests/test_box_guide.py's rule, per case -- 16 x the discrepancy of guide.py's closure under torch float32 autograd on the
CPU against float64 on the same inputs, relative to the tensor's maximum, with a floor of 8 float32 ulp; the shift and D~ bars derive
from it (profiles/guide_rel_errors.md holds the measured figures)."""
import ctypes as C

import numpy as np
import pytest
import torch

import box_rel_ref as RR
import guide_ref as GR
from test_box_guide import SCALE, STEP_RTOL, T8, TRAJ_RTOL, ULP, VALID, _flags, _gt_inputs, _guide, _net, _np, _sampler, dev, valid_sets
from test_box_guide_host import LOSSES, case
from test_box_rel_host import MARGIN, W_REL, WHICH, decode_case, hinge_case, rel_kinds, torch_loss_grad
from diffusesg_amd import lib
from diffusesg_amd import spec as S
from diffusesg_amd import synth as Y
from diffusesg_amd import weights as W

pytestmark = pytest.mark.gpu

N_ADJ_TYPE = 51   # the tiny configuration's 6 adjacency bits


# ---- 1. the kernel alone ----
def run_kernel(xh, D, flags, kw, coef, clip, rel, sel=None, region=None, mask_node=None):
    """dsg_debug_box_guide_rel on float32 device copies; rel = dict(w_rel, margin, kinds | (pred_kind, encoding)) or None.  Returns the
    outputs as float64 arrays and the kinds the kernel used"""
    L = lib.load()
    B, N, cn = D[1].shape
    ca = D[0].shape[1]
    t = [dev(v, torch.float32) for v in (xh[0], xh[1], D[0], D[1])]
    fl = dev(flags.astype(np.uint8))
    mk = None if mask_node is None else dev(mask_node.astype(np.uint8))
    sl = None if sel is None else dev(sel.astype(np.uint8))
    rg = None if region is None else dev(region, torch.float32)
    cfg = lib.DsgGuideCfg(kw.get("a_o", 0.0), kw.get("a_r", 0.0), kw.get("a_a", 0.0), kw.get("tau", 0.05),
                          lib.GUIDE_CLIP_NONE if clip is None else clip, 0, None if sl is None else sl.data_ptr(),
                          None if rg is None else rg.data_ptr(), None)
    keep = rcfg = None
    if rel is not None and "kinds" in rel:
        keep = dev(rel["kinds"].astype(np.uint8))
        rcfg = lib.DsgRelCfg(rel["w_rel"], rel["margin"], lib.REL_GIVEN, 0, 0, 0, keep.data_ptr(), None)
    elif rel is not None:
        keep = np.ascontiguousarray(rel["pred_kind"], dtype=np.uint8)
        rcfg = lib.DsgRelCfg(rel["w_rel"], rel["margin"], lib.REL_DECODED, lib.ENCODINGS[rel["encoding"]], len(keep), 0, None, keep.ctypes.data)
    out = dict(loss=torch.empty(B), grad=torch.empty(B, N, 4), shift=torch.empty(B, N, 4), factor=torch.empty(B), norms=torch.empty(B, 2),
               D_guided=torch.empty(B, N, cn))
    out = {k: v.cuda() for k, v in out.items()}
    kinds_out = torch.full((B, N, N), 255, dtype=torch.uint8).cuda()
    p = lambda x: None if x is None else x.data_ptr()
    rc = L.dsg_debug_box_guide_rel(B, N, ca, cn, *(p(x) for x in t), p(fl), p(mk), C.byref(cfg), float(coef),
                                   *(p(out[k]) for k in ("loss", "grad", "shift", "factor", "norms", "D_guided")),
                                   torch.cuda.current_stream().cuda_stream, None if rcfg is None else C.byref(rcfg), p(kinds_out))
    assert rc == 0, (rc, L.dsg_last_error(None))
    return {k: v.cpu().numpy().astype(np.float64) for k, v in out.items()}, kinds_out.cpu().numpy()


def kernel_bars(D32, flags, sel, region, kw, kinds, w_rel, margin):
    """(loss bar, gradient bar) of one case: 16 x |torch float32 autograd - float64| on the CPU, floor 8 ulp, both of the tensor's maximum"""
    clean = np.where(flags[:, :, None] != 0, D32, 0.0)   # torch's closures multiply by the flags: no NaN for them
    L64, g64 = torch_loss_grad(clean.astype(np.float64), flags, sel, region, kw, kinds, torch.float64, w_rel, margin)
    L32, g32 = torch_loss_grad(clean.astype(np.float64), flags, sel, region, kw, kinds, torch.float32, w_rel, margin)
    bar = lambda a, b: max(16 * float(np.abs(a - b).max()), 8 * ULP * float(np.abs(b).max()))
    return bar(L32, L64), bar(g32, g64), float(np.abs(L32 - L64).max()), float(np.abs(g32 - g64).max())


WORST = {}   # output -> (error / bar, error, bar, case): the largest measured figures, printed by the last kernel test


def check_kernel(got, ref, D32, flags, sel, region, kw, kinds, w_rel, margin, coef, tag):
    bL, bg, dL, dg = kernel_bars(D32, flags, sel, region, kw, kinds, w_rel, margin)
    gmax, dmax = float(np.abs(ref["grad"]).max()), float(np.nanmax(np.abs(np.where(flags[:, :, None] != 0, D32, 0.0)), initial=0.0))
    bars = dict(loss=bL, grad=bg, shift=abs(coef) * bg + 8 * ULP * abs(coef) * gmax,
                factor=8 * ULP, norms=8 * ULP * max(float(np.abs(ref["norms"]).max()), 1e-30))
    bars["D_guided"] = bars["shift"] + 8 * ULP * dmax
    for k, bar in bars.items():
        assert np.isfinite(got[k]).all(), (tag, k)
        err = float(np.abs(got[k] - ref[k]).max())
        print(f"BOXREL kernel {tag} {k}: err {err:.3e} bar {bar:.3e} (torch f32 vs f64: loss {dL:.3e}, grad {dg:.3e})")
        if bar > 0 and err / bar >= WORST.get(k, (-1.0,))[0]:
            WORST[k] = (err / bar, err, bar, tag)
        assert err <= bar, (tag, k, err, bar)
    assert (got["grad"][flags == 0] == 0).all() and (got["shift"][flags == 0] == 0).all() and (got["D_guided"][flags == 0] == 0).all()


def adjacency_for(flags, ca, seed, decoded=None):
    """(D_adj, x_hat_adj) float32 [B, ca, N, N] with NaN wherever a pair is not live: padded rows, padded columns -- and, with the
    decoded source, the diagonal (the clip's norm pass reads the diagonal of valid nodes, so it stays finite without one)"""
    rng = np.random.default_rng(seed + 2000)
    B, N = flags.shape
    Da = rng.uniform(-1.2, 1.2, (B, ca, N, N)).astype(np.float32)
    Da[rng.random(Da.shape) < 0.05] = 0.0
    Da[rng.random(Da.shape) < 0.05] = -0.0
    xa = (Da + rng.standard_normal(Da.shape)).astype(np.float32)
    pad = flags == 0
    dead = pad[:, None, :, None] | pad[:, None, None, :]
    if decoded == "noclip":
        dead = dead | np.eye(N, dtype=bool)[None, None]
    for v in (Da, xa):
        v[np.broadcast_to(dead, v.shape)] = np.nan
    return Da, xa


ENC_CA = {"bits": (6, 51), "one_hot": (7, 7), "ddpm": (1, 7)}


def kernel_case(N, cn, valid, seed, which, others, source, clip=1.0, coef=0.37, with_mask=False):
    """one case of the kernel test.  which: a kind or 'mixed'; others: the key of LOSSES that runs beside the relation term, or None;
    source: 'given', or an encoding -- then the kinds are what the adjacency decodes to under a random predicate -> kind table"""
    D, flags, sel, region = case(N, cn, valid, seed)
    rng = np.random.default_rng(seed + 1000)
    D32 = D.astype(np.float32)
    xn = (D32 + rng.standard_normal(D32.shape)).astype(np.float32)
    for v in (D32, xn):
        v[flags == 0] = np.nan                           # NaN in every padded node row
    kw = LOSSES[others] if others else {}
    use_r = kw.get("a_r", 0.0) != 0
    mask = (rng.random(D32.shape) < 0.3) if with_mask else None
    if source == "given":
        kinds = rel_kinds(flags, seed, which).astype(np.int64)
        if N >= 2:
            kinds[:, 0, 1] = 200                         # kinds above 7 count as none
        Da, xa = adjacency_for(flags, 2, seed)
        rel = dict(w_rel=W_REL, margin=MARGIN, kinds=kinds)
    else:
        ca, k = ENC_CA[source]
        Da, xa = adjacency_for(flags, ca, seed, "noclip" if clip is None else "clip")
        table = rng.integers(0, RR.KINDS, k).astype(np.uint8) if which == "mixed" else np.where(rng.random(k) < 0.6, which, 0).astype(np.uint8)
        kinds = RR.decoded_kinds(Da, flags, table, source).astype(np.int64)
        rel = dict(w_rel=W_REL, margin=MARGIN, pred_kind=table, encoding=source)
    got, used = run_kernel((xa, xn), (Da, D32), flags, kw, coef, clip, rel, sel if use_r else None, region if use_r else None, mask)
    ref = RR.guided_call((xa, xn), (Da.astype(np.float64), D32.astype(np.float64)), flags, np.float32(coef), clip, mask_node=mask,
                         kinds=kinds, w_rel=W_REL, margin=MARGIN, sel=sel, region=region, **kw)
    f = flags.astype(bool)
    live = f[:, :, None] & f[:, None, :] & ~np.eye(N, dtype=bool)[None]
    want = np.where(live & (kinds < RR.KINDS), kinds, 0)
    assert np.array_equal(used, want), "the kinds the kernel used"
    return got, ref, (D32, flags, sel, region, kw, want.astype(np.uint8), mask)


@pytest.mark.parametrize("cn", [4, 5, 12])
@pytest.mark.parametrize("N", [1, 2, 8, 40, 64])
def test_kernel_against_float64(N, cn):
    n_rel = 0
    for vi, valid in enumerate(valid_sets(N)):
        for wi, which in enumerate(WHICH):
            # each kind alone and all kinds mixed, the relation term on its own; the sources and the clip take turns
            source = ("given", "bits", "one_hot", "ddpm")[(wi + vi) % 4]
            clip = (1.0, None)[(wi + vi + N) % 2]
            seed = 10 * N + cn + vi
            got, ref, (D32, flags, sel, region, kw, kinds, _m) = kernel_case(N, cn, valid, seed, which, None, source, clip)
            check_kernel(got, ref, D32, flags, sel, region, kw, kinds, W_REL, MARGIN, 0.37, f"N={N} C={cn} valid={valid} kind={which} {source} clip={clip}")
            n_rel += int(np.abs(ref["grad"]).max() > 0)
        for source in ("given", "bits"):   # ... and together with the other three losses
            got, ref, (D32, flags, sel, region, kw, kinds, _m) = kernel_case(N, cn, valid, 10 * N + cn + vi, "mixed", "all", source, 1.0)
            check_kernel(got, ref, D32, flags, sel, region, kw, kinds, W_REL, MARGIN, 0.37, f"N={N} C={cn} valid={valid} mixed+all {source}")
    if N >= 8:
        assert n_rel >= len(WHICH), "every kind must move the gradient somewhere"


def test_kernel_special_cases():
    """pairs exactly on a hinge give exactly 0 on the device too; a known mask zeroes the shift and leaves D bit-exact; a clipped and an
    unclipped graph both occur; at the end, the largest measured error of every output"""
    D, flags, K, m = hinge_case(5)
    D32 = D.astype(np.float32)
    D32[flags == 0] = np.nan
    Da = np.zeros((1, 2, 8, 8), np.float32)
    got, used = run_kernel((Da, D32), (Da, D32), flags, {}, 1.0, None, dict(w_rel=W_REL, margin=m, kinds=K))
    assert np.array_equal(used, K)
    assert (got["loss"] == 0).all() and (got["grad"] == 0).all() and (got["shift"] == 0).all(), "a pair on its hinge adds exactly 0"
    got2, _ = run_kernel((Da, D32), (Da, D32), flags, {}, 1.0, None, dict(w_rel=W_REL, margin=m + 2.0 ** -20, kinds=K))
    assert (got2["loss"] > 0).all() and np.abs(got2["grad"]).max() > 0
    for source in ("given", "bits"):
        got, ref, (D32, flags, sel, region, kw, kinds, mask) = kernel_case(8, 5, [8, 5, 3], 77, "mixed", "all", source, clip=0.5, coef=2.0, with_mask=True)
        check_kernel(got, ref, D32, flags, sel, region, kw, kinds, W_REL, MARGIN, 2.0, f"special {source}")
        known = mask[..., -4:] & (flags[:, :, None] != 0)
        assert known.any() and (got["shift"][known] == 0).all()
        assert np.array_equal(got["D_guided"][..., -4:][known], D32[..., -4:][known].astype(np.float64))
        other = np.broadcast_to((flags != 0)[:, :, None], D32.shape).copy()
        other[..., -4:] = False
        assert np.array_equal(got["D_guided"][other], D32[other].astype(np.float64))                           # nothing outside the box channels
        assert np.array_equal(got["factor"] < 1, ref["factor"] < 1)
    # without a descriptor, or with w_rel = 0, the hook is dsg_debug_box_guide: the kernel without the term
    D, flags, sel, region = case(8, 5, [8, 5, 3], 5)
    D32 = D.astype(np.float32)
    Da, xa = adjacency_for(flags, 2, 5)
    xn = (D32 + 1).astype(np.float32)
    kw = LOSSES["all"]
    kinds = rel_kinds(flags, 5, "mixed")
    base, used0 = run_kernel((xa, xn), (Da, D32), flags, kw, 0.37, 1.0, None, sel, region)
    zero, used1 = run_kernel((xa, xn), (Da, D32), flags, kw, 0.37, 1.0, dict(w_rel=0.0, margin=MARGIN, kinds=kinds), sel, region)
    with_rel, _ = run_kernel((xa, xn), (Da, D32), flags, kw, 0.37, 1.0, dict(w_rel=W_REL, margin=MARGIN, kinds=kinds), sel, region)
    assert all(np.array_equal(base[k], zero[k]) for k in base) and (used0 == 0).all() and (used1 == 0).all()
    assert not np.array_equal(base["grad"], with_rel["grad"])
    for k, (ratio, err, bar, tag) in sorted(WORST.items()):
        print(f"BOXREL worst {k}: err {err:.3e} = {ratio:.3f} of its bar {bar:.3e} ({tag})")


# ---- 2. the decoded source against dsg_decode ----
@pytest.mark.parametrize("N", [2, 8, 40])
@pytest.mark.parametrize("encoding", ["bits", "one_hot", "ddpm"])
def test_decoded_kinds_are_the_table_of_dsg_decode(encoding, N):
    from diffusesg_amd import io as dio
    a, flags, pred_kind, k = decode_case(encoding, N, seed=N + 1, valid=[N, max(N - 3, 1), min(2, N)])
    B = a.shape[0]
    f = flags.astype(bool)
    live = f[:, :, None] & f[:, None, :] & ~np.eye(N, dtype=bool)[None]
    lv = np.broadcast_to(live[:, None], a.shape)
    if N >= 8:
        assert (lv & (a == 0) & ~np.signbit(a)).any() and (lv & (a == 0) & np.signbit(a)).any() and (lv & np.isnan(a)).any()
    a_poison = a.copy()
    a_poison[~lv] = np.nan                               # nothing that is not live may be read
    cfg = S.ModelConfig(max_node_num=N, c_adj=a.shape[1], c_node=5, depths=(1,), num_heads=(3,), window_size={2: 2, 8: 4, 40: 10}[N],
                        self_condition=False)
    h = lib.Handle(cfg)
    node = np.zeros((B, N, 5), np.float32)
    q_adj, _qn, _bb = dio.decode(h, dev(a), dev(node), dev(flags), k, 2, encoding, "bits")
    h.close()
    q = q_adj.cpu().numpy().astype(np.int64)
    want = np.where(live & (q >= 0), pred_kind[np.clip(q, 0, k - 1)], 0).astype(np.uint8)
    assert np.array_equal(want, RR.decoded_kinds(a, flags, pred_kind, encoding)), "the restatement and dsg_decode"
    D, _f, _s, _r = case(N, 5, [N, 1, 1], N)
    D32 = D.astype(np.float32)
    _got, used = run_kernel((a_poison, D32), (a_poison, D32), flags, {}, 0.5, None, dict(w_rel=1.0, margin=0.0, pred_kind=pred_kind, encoding=encoding))
    assert np.array_equal(used, want)
    if N >= 8:
        assert len(np.unique(used)) >= 4


# ---- 3. in the loop ----
def _rules(seed=1, encoding="bits"):
    from diffusesg_amd.guide import SpatialRules
    t = np.random.default_rng(seed).integers(0, RR.KINDS, N_ADJ_TYPE).astype(np.uint8)
    t[0] = 0
    return SpatialRules(t, N_ADJ_TYPE, encoding)


def _rel_guide(flags_np, source, seed=5, with_others=True, **kw):
    """(BoxGuide with a relation term, the keyword arguments of RR.guided_call that restate it -- without `kinds` where they are decoded,
    the rules or None)"""
    from diffusesg_amd.guide import BoxGuide
    base, gkw = _guide(flags_np, seed)
    args = dict(overlap=base.overlap, align=base.align, tau=base.tau, region_weight=base.region_weight,
                region=(base.region[1], base.region[2])) if with_others else {}
    if not with_others:
        gkw = {}
    gkw = dict(gkw, w_rel=W_REL, margin=MARGIN)
    rules = None
    if source == "given":
        kinds = rel_kinds(flags_np, seed, "mixed")
        gkw["kinds"] = kinds
        rel = torch.from_numpy(kinds)
    else:
        rel = rules = _rules(seed)
    args.update(kw)
    return BoxGuide(relations=rel, relation_weight=W_REL, relation_margin=MARGIN, **args), gkw, rules


def _kinds_now(gkw, rules, D_adj32, flags):
    return gkw["kinds"] if rules is None else RR.decoded_kinds(D_adj32, flags, rules.pred_kind, rules.encoding)


def test_without_a_relation_term_it_is_sample_guided():
    """rel == NULL and w_rel == 0 through dsg_sample_guided_rel equal dsg_sample_guided bit for bit, replayed and enqueued; and the
    bodies of a run with relations, replayed, equal the enqueued ones, for both sources"""
    from diffusesg_amd import guide as G
    cfg = Y.CONFIGS["tiny"]()
    net, fl = _net("tiny"), _flags("tiny")
    flags = fl.numpy()
    plain, _ = _guide(flags)
    kinds = torch.from_numpy(rel_kinds(flags, 5, "mixed"))
    mk = lambda **kw: G.BoxGuide(overlap=plain.overlap, align=plain.align, tau=plain.tau, region_weight=plain.region_weight,
                                 region=(plain.region[1], plain.region[2]), **kw)
    zero = mk(relations=kinds, relation_weight=0.0, relation_margin=MARGIN)
    null = mk(relations=kinds, relation_weight=W_REL, relation_margin=MARGIN)
    # a guide that has relations and describes none: the sampler then hands rel = NULL to dsg_sample_guided_rel
    null.__class__ = type("NullRelGuide", (G.BoxGuide,), {"relation_descriptor": lambda self, *a: (None, None)})
    given, decoded = mk(relations=kinds, relation_weight=W_REL, relation_margin=MARGIN), mk(relations=_rules(), relation_weight=W_REL, relation_margin=MARGIN)
    coins = (np.random.default_rng(3).random(2 * T8) < 0.5).astype(np.uint8)
    rng = np.random.default_rng(4)
    ka = torch.from_numpy(np.sign(rng.standard_normal((3, cfg.c_adj, 8, 8))).astype(np.float32))
    kn = torch.from_numpy((np.sign(rng.standard_normal((3, 8, cfg.c_node))) * 0.7).astype(np.float32))
    ma, mn = torch.from_numpy(rng.random(ka.shape) < 0.4), torch.from_numpy(rng.random(kn.shape) < 0.4)
    h = net.model._ensure_handle()
    old = h.get_option("loop_graph")
    runs = {}
    try:
        for solver in ("heun", "dpmpp_2m"):
            smp = _sampler("tiny", solver)
            for loop_graph in (1, 0):
                h.set_option("loop_graph", loop_graph)
                kw = dict(seed=5, coins=coins, return_device=True, known=(ka, kn, ma, mn), clip_ratio=0.5)
                ref = _np(smp.sample_guided(net, fl, plain, SCALE, **kw))
                for name, g in (("w_rel = 0", zero), ("rel = NULL", null)):
                    got = _np(smp.sample_guided(net, fl, g, SCALE, **kw))
                    assert all(np.array_equal(a, b) for a, b in zip(got, ref)), f"{name} against sample_guided, {solver}, loop_graph {loop_graph}"
                for name, g in (("given", given), ("decoded", decoded)):
                    runs[solver, name, loop_graph] = _np(smp.sample_guided(net, fl, g, SCALE, **kw))
                    assert not np.array_equal(runs[solver, name, loop_graph][1], ref[1]), f"the {name} relation term moves nothing"
            for name in ("given", "decoded"):
                assert all(np.array_equal(a, b) for a, b in zip(runs[solver, name, 1], runs[solver, name, 0])), f"replayed and enqueued bodies differ: {solver} {name}"
    finally:
        h.set_option("loop_graph", old)


def _recompute_gt_run(solver, clip, sched, noise_coef, ms, snaps, trace, gkw, rules, flags, ia, inn, na, nn, ga, gn, smp):
    """every executed step of a sanity-check run in float64 from the state in front of it (tests/test_box_guide.py's, with the relation
    term in the loss); returns the number of clipped calls and the last call"""
    sg, t_hat, _nc, h_step = lib.sigma_schedule(smp._cfg())
    cw = lib.guide_coef(smp._cfg(), SCALE.astype(np.float32))
    T = smp.num_steps
    adjs_ls, nodes_ls = snaps
    x = (ia * np.float32(sg[sched[0]]), inn * np.float32(sg[sched[0]]))
    D = (ga.astype(np.float64), gn.astype(np.float64))
    kinds = _kinds_now(gkw, rules, ga, flags)            # D = gt at every call: one set of kinds
    kw = dict({k: v for k, v in gkw.items() if k != "kinds"}, kinds=kinds)
    n_clipped, prev, r = 0, None, None
    for k, i in enumerate(sched):
        xh = tuple((x[j].astype(np.float32) + np.float32(noise_coef[k]) * (na, nn)[j][k]).astype(np.float32) if noise_coef[k] != 0 else x[j] for j in range(2))
        xh = (W.mask_adj(xh[0], flags), W.mask_node(xh[1], flags))
        r = RR.guided_call(xh, D, flags, cw[i], clip, **kw)
        n_clipped += int((r["factor"] < 1).any())
        G = (D[0], r["D_guided"])
        t, h = float(t_hat[i]), float(h_step[i])
        if solver == "heun" and i != T - 1:
            ref = GR.heun_update(xh, G, G, t, h, flags)          # stage 2 is evaluated at (x_hat, t_hat): the same D, the same shift
        else:
            ref = GR.euler_update(xh, G, t, h, flags, float(ms[k]), prev)
        got = (adjs_ls[k + 1], nodes_ls[k + 1])
        for j, what in enumerate(("adj", "node")):
            s = max(float(np.abs(xh[j]).max()), 1e-30)
            err = float(np.abs(got[j].astype(np.float64) - ref[j]).max()) / s
            assert err <= STEP_RTOL, f"step {k} (schedule index {i}) {what}: {err:.3e}"
        assert np.abs(trace[k].astype(np.float64) - r["loss"]).max() <= 4 * ULP * max(1.0, np.abs(r["loss"]).max()), f"loss trace row {k}"   # float64 inside, rounded once
        prev = G
        x = got
    return n_clipped, r


@pytest.mark.parametrize("clip", [0.02, None])
@pytest.mark.parametrize("solver,source", [("euler", "given"), ("heun", "decoded"), ("dpmpp_2m", "given"), ("euler", "decoded")])
def test_loop_arithmetic_recomputed_in_float64(solver, source, clip):
    flags, ia, inn, na, nn, ga, gn = _gt_inputs()
    net, smp = _net("tiny"), _sampler("tiny", solver)
    guide, gkw, rules = _rel_guide(flags, source)
    a, n, adjs_ls, nodes_ls, trace = _np(smp.sample_guided(
        net, torch.from_numpy(flags), guide, SCALE, clip_ratio=clip, init_adjs=torch.from_numpy(ia), init_nodes=torch.from_numpy(inn),
        churn_noise=(torch.from_numpy(na), torch.from_numpy(nn)), sanity_check_gt_adjs=torch.from_numpy(ga),
        sanity_check_gt_nodes=torch.from_numpy(gn), flag_interim_adjs=True, return_loss_trace=True))
    assert adjs_ls.shape[0] == T8 + 1 and trace.shape == (T8, 3)
    nc = lib.sigma_schedule(smp._cfg())[2]
    ms = lib.multistep_coef(smp._cfg())
    n_clipped, last = _recompute_gt_run(solver, clip, list(range(T8)), nc, ms, (adjs_ls, nodes_ls), trace, gkw, rules, flags, ia, inn, na, nn, ga, gn, smp)
    if clip is not None:
        assert n_clipped > 0, "the clip never engaged: the case does not test it"
    assert np.abs(n.astype(np.float64) - last["D_guided"]).max() <= STEP_RTOL * np.abs(gn).max()
    assert np.abs(last["shift"]).max() > 0
    if clip is not None:
        return
    # unclipped, the relation term is felt half way down: the same run without it is elsewhere (the END of a sanity-check run is
    # gt - c_{T-1} g whatever came before, and c_{T-1} is of the order of 1e-6)
    plain, _ = _guide(flags)
    pn_ls = _np(smp.sample_guided(net, torch.from_numpy(flags), plain, SCALE, clip_ratio=clip, init_adjs=torch.from_numpy(ia),
                                  init_nodes=torch.from_numpy(inn), churn_noise=(torch.from_numpy(na), torch.from_numpy(nn)),
                                  sanity_check_gt_adjs=torch.from_numpy(ga), sanity_check_gt_nodes=torch.from_numpy(gn),
                                  flag_interim_adjs=True))[3]
    k = T8 // 2
    assert np.abs(pn_ls[k] - nodes_ls[k]).max() > 100 * STEP_RTOL * np.abs(nodes_ls[k]).max()


@pytest.mark.parametrize("source", ["given", "decoded"])
def test_walk_recomputed_in_float64(source):
    """a guided resampling walk in the sanity-check mode: the executed steps of dsg_walk_steps, each recomputed in float64"""
    flags, ia, inn, na, nn, ga, gn = _gt_inputs(walk=True)
    net, smp = _net("tiny"), _sampler("tiny", "euler")
    guide, gkw, rules = _rel_guide(flags, source)
    sched, coef = lib.walk_steps(smp._cfg(), lib.make_walk_cfg(0, (2, 2), (2, 6)))
    assert len(sched) == 12 and (np.diff(sched) < 0).any()
    a, n, adjs_ls, nodes_ls, trace = _np(smp.sample_guided(
        net, torch.from_numpy(flags), guide, SCALE, clip_ratio=None, resample=(2, 2), resample_range=(2, 6),
        init_adjs=torch.from_numpy(ia), init_nodes=torch.from_numpy(inn), churn_noise=(torch.from_numpy(na), torch.from_numpy(nn)),
        sanity_check_gt_adjs=torch.from_numpy(ga), sanity_check_gt_nodes=torch.from_numpy(gn), flag_interim_adjs=True, return_loss_trace=True))
    assert trace.shape == (12, 3) and adjs_ls.shape[0] == 13
    _recompute_gt_run("euler", None, sched.tolist(), coef, np.zeros(12), (adjs_ls, nodes_ls), trace, gkw, rules, flags, ia, inn, na, nn, ga, gn, smp)


@pytest.mark.parametrize("source", ["given", "decoded"])
def test_real_network_chain_recomputed_in_float64(source):
    """the real synthetic network: every step's dsg_precond call, shifted and stepped in float64, reproduces the snapshots; with the
    decoded source the kinds follow the adjacency estimate of each call"""
    net, smp, fl = _net("tiny"), _sampler("tiny", "euler", churn=0), _flags("tiny")
    flags = fl.numpy()
    guide, gkw, rules = _rel_guide(flags, source)
    coins = np.zeros(T8, np.uint8)
    a, n, adjs_ls, nodes_ls, trace = _np(smp.sample_guided(net, fl, guide, SCALE, clip_ratio=0.5, seed=13, coins=coins, flag_interim_adjs=True,
                                                           return_loss_trace=True))
    sg, t_hat, _nc, h_step = lib.sigma_schedule(smp._cfg())
    cw = lib.guide_coef(smp._cfg(), SCALE.astype(np.float32))
    hd = net.model._ensure_handle()
    fl8 = fl.to(torch.uint8).cuda()
    B = 3
    sc = (None, None)
    p = lambda v: None if v is None else v.data_ptr()
    seen = []
    for i in range(T8):
        x = (adjs_ls[i] * np.float32(sg[0]), nodes_ls[i] * np.float32(sg[0])) if i == 0 else (adjs_ls[i], nodes_ls[i])
        xa, xn = dev(x[0]), dev(x[1])
        sig = torch.full((B,), float(t_hat[i]), dtype=torch.float32, device="cuda")
        Da, Dn = torch.empty_like(xa), torch.empty_like(xn)
        hd.check(hd.L.dsg_precond(hd.raw, B, p(xa), p(xn), p(fl8), p(sig), p(sc[0]), p(sc[1]), 0, p(Da), p(Dn),
                                  torch.cuda.current_stream().cuda_stream), "dsg_precond")
        torch.cuda.synchronize()
        sc = (Da, Dn)                                      # the self-conditioning input of the next call is D, not D~
        Da32 = Da.cpu().numpy()
        D = (Da32.astype(np.float64), Dn.cpu().numpy().astype(np.float64))
        kinds = _kinds_now(gkw, rules, Da32, flags)
        seen.append(kinds)
        kw = dict({k: v for k, v in gkw.items() if k != "kinds"}, kinds=kinds)
        r = RR.guided_call(x, D, flags, cw[i], 0.5, **kw)
        ref = GR.euler_update(x, (D[0], r["D_guided"]), float(t_hat[i]), float(h_step[i]), flags)
        got = (adjs_ls[i + 1], nodes_ls[i + 1])
        for j, what in enumerate(("adj", "node")):
            err = float(np.abs(got[j].astype(np.float64) - ref[j]).max()) / max(float(np.abs(x[j]).max()), 1e-30)
            print(f"BOXREL chain {source} step {i} {what}: {err:.3e}")
            assert err <= TRAJ_RTOL, (i, what, err)
        lkw = {k: v for k, v in gkw.items() if k in ("a_o", "a_r", "a_a", "tau")}
        bL, _bg, _dL, _dg = kernel_bars(D[1].astype(np.float32), flags.astype(np.uint8), gkw["sel"], gkw["region"], lkw, kinds, W_REL, MARGIN)
        errL = float(np.abs(trace[i].astype(np.float64) - r["loss"]).max())
        print(f"BOXREL chain {source} step {i} loss trace: err {errL:.3e} bar {bL:.3e}")
        assert errL <= bL, (i, errL, bL)
    if source == "decoded":
        assert any(not np.array_equal(seen[0], k) for k in seen[1:]), "the decoded kinds never changed along the run"


def test_known_entries_exact_and_padded_entries_zero():
    cfg = Y.CONFIGS["tiny"]()
    net, fl = _net("tiny"), _flags("tiny")
    flags = fl.numpy()
    rng = np.random.default_rng(4)
    ka = np.sign(rng.standard_normal((3, cfg.c_adj, 8, 8))).astype(np.float32)
    kn = (np.sign(rng.standard_normal((3, 8, cfg.c_node))) * 0.7).astype(np.float32)
    ma, mn = rng.random(ka.shape) < 0.4, rng.random(kn.shape) < 0.4
    known = tuple(torch.from_numpy(v) for v in (ka, kn, ma, mn))
    va, vn = np.broadcast_to(flags[:, None, :, None] & flags[:, None, None, :], ka.shape), np.broadcast_to(flags[:, :, None], kn.shape)
    for solver, source in (("euler", "decoded"), ("heun", "given"), ("dpmpp_2m", "decoded")):
        guide, _gkw, _rules = _rel_guide(flags, source)
        smp = _sampler("tiny", solver)
        coins = (np.random.default_rng(6).random(2 * T8) < 0.5).astype(np.uint8)
        kw = dict(seed=7, coins=coins, flag_interim_adjs=True)
        ga, gn, gal, gnl = _np(smp.sample_guided(net, fl, guide, SCALE, known=known, clip_ratio=0.5, **kw))
        pa, pn, pal, pnl = _np(smp.sample_known(net, fl, *known, num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj, **kw))
        # a known entry's trajectory is a function of its own noise and the known value: the guided run's equals the unguided run's
        # at EVERY step exactly when every guided estimate carried the known value bit for bit
        assert np.array_equal(gal[:, ma & va], pal[:, ma & va]) and np.array_equal(gnl[:, mn & vn], pnl[:, mn & vn]), solver
        assert not np.array_equal(gn[~mn & vn], pn[~mn & vn])
        assert (gal[:, ~va] == 0).all() and (gnl[:, ~vn] == 0).all() and (ga[~va] == 0).all() and (gn[~vn] == 0).all()


def test_batch_invariant_graphs_alone_equal_the_batch():
    from diffusesg_amd.guide import BoxGuide
    net, fl = _net("tiny"), _flags("tiny")
    flags = fl.numpy()
    seeds = [2 ** 64 - 1, 2 ** 32 + 5, 1]
    h = net.model._ensure_handle()
    old = h.get_option("batch_invariant")
    h.set_option("batch_invariant", 1)
    try:
        for solver, source in (("heun", "given"), ("dpmpp_2m", "decoded")):
            smp = _sampler("tiny", solver)
            guide, gkw, rules = _rel_guide(flags, source)
            batch = _np(smp.sample_guided(net, fl, guide, SCALE, clip_ratio=0.5, graph_seeds=seeds, coin_seed=3))
            for b in range(3):
                rel = rules if rules is not None else torch.from_numpy(gkw["kinds"][b:b + 1])
                one_guide = BoxGuide(overlap=guide.overlap, align=guide.align, tau=guide.tau, region_weight=guide.region_weight,
                                     region=(guide.region[1][b:b + 1], guide.region[2][b:b + 1]), relations=rel, relation_weight=W_REL,
                                     relation_margin=MARGIN)
                one = _np(smp.sample_guided(net, fl[b:b + 1], one_guide, SCALE, clip_ratio=0.5, graph_seeds=seeds[b:b + 1], coin_seed=3))
                assert all(np.array_equal(batch[k][b:b + 1], one[k]) for k in range(2)), (solver, source, b)
    finally:
        h.set_option("batch_invariant", old)


def test_layout_from_graph_under_its_own_predicates():
    """layout_from_graph holds every relation: the known select makes the decoded kinds the graph's own at every call, so the decoded
    source equals the given source with pred_kind[q_adj] bit for bit; the labels and relations stay as given, the boxes move"""
    from diffusesg_amd.complete import layout_from_graph
    from diffusesg_amd.guide import BoxGuide, relation_kinds_from_graph
    cfg = Y.CONFIGS["tiny"]()   # 6 adjacency bits, 8 label bits + 4 box channels
    n_node_type, n = 150, cfg.max_node_num
    flags = W.synth_flags(3, n, VALID)
    f = flags.astype(np.int32)
    rng = np.random.default_rng(12)
    q_adj = rng.integers(0, N_ADJ_TYPE, (3, n, n)).astype(np.int32) * f[:, :, None] * f[:, None, :]
    q_adj[:, np.arange(n), np.arange(n)] = 0
    q_node = rng.integers(0, n_node_type, (3, n)).astype(np.int32) * f
    net, smp = _net("tiny"), _sampler("tiny", "heun")
    t = lambda a: torch.from_numpy(a).cuda()
    rules = _rules(3)
    kinds = relation_kinds_from_graph(torch.from_numpy(q_adj), torch.from_numpy(flags), rules)
    assert np.array_equal(kinds.numpy(), RR.kinds_of_predicates(q_adj, flags, rules.pred_kind)) and len(np.unique(kinds.numpy())) == RR.KINDS
    out = {}
    for key, kw in (("plain", {}), ("decoded", dict(guide=BoxGuide(overlap=0.5, relations=rules, relation_margin=MARGIN), guide_scale=SCALE)),
                    ("given", dict(guide=BoxGuide(overlap=0.5, relations=kinds, relation_margin=MARGIN), guide_scale=SCALE))):
        np.random.seed(6)
        out[key] = _np(layout_from_graph(net, smp, t(q_adj), t(q_node), t(flags), N_ADJ_TYPE, n_node_type, seed=22, **kw))
    assert all(np.array_equal(a, b) for a, b in zip(out["decoded"], out["given"]))
    off = flags[:, :, None] & flags[:, None, :] & ~np.eye(n, dtype=bool)[None]
    qa, qn, bb = out["decoded"]
    assert np.array_equal(qn[flags], q_node[flags]) and np.array_equal(qa[off], q_adj[off])
    assert np.isfinite(bb).all() and np.abs(bb[flags] - out["plain"][2][flags]).max() > 1e-3


@pytest.mark.parametrize("solver", ["euler", "heun"])
def test_against_the_eager_loop_with_zero_jacobian(solver):
    """both read-out heads' last linears zeroed: F = 0, the network's Jacobian vanishes, and the in-loop shift is the eager loop's"""
    from diffusesg_amd.guide import BoxGuide, box_relation_loss, guided_sample
    cfg = Y.CONFIGS["tiny"]()
    net, smp, fl = _net("tiny", True), _sampler("tiny", solver), _flags("tiny")
    kinds = torch.from_numpy(rel_kinds(fl.numpy(), 9, "mixed"))
    guide = BoxGuide(relations=kinds, relation_weight=W_REL, relation_margin=MARGIN)
    loss = box_relation_loss(kinds, fl, MARGIN)
    np.random.seed(21)
    got = _np(smp.sample_guided(net, fl, guide, SCALE, clip_ratio=1.0, seed=9, return_device=True))
    np.random.seed(21)
    ref = _np(guided_sample(net, smp, fl, lambda a, x: loss(a, x) * W_REL, SCALE, clip_ratio=1.0, seed=9))
    np.random.seed(21)
    plain = _np(smp.sample(net, fl, seed=9, num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj, return_device=True))
    torch.cuda.synchronize()
    for what, g, r, p in zip(("adj", "node"), got, ref, plain):
        s = float(np.abs(r).max())
        err, moved = float(np.abs(g - r).max()) / s, float(np.abs(g - p).max()) / s
        print(f"BOXREL eager {solver} {what}: |in-loop - eager| {err:.3e}, |guided - unguided| {moved:.3e} of the result's scale")
        assert g.shape == r.shape and err <= TRAJ_RTOL, (what, err)
        if what == "node":
            assert moved > 100 * TRAJ_RTOL, "the guidance moves nothing: the case tests nothing"
