"""GPU: content guidance (dsg_sample_guided_content).

1. the content kernel alone (dsg_debug_content_guide) against the float64 restatement of tests/content_ref.py, every output element:
   loss, item_loss and both gradients inside content_ref.bars (one float32 ulp of the reference value + the float64 term derived from
   the operation count -- not tuned to the kernel), `best` equal to the reference's arg-max, shift and D~ bit for bit from the kernel's
   own g and f_b, the clip factor bit for bit from the kernel's own norms; NaN in every padded row and column and on the diagonal;
2. special cases: a tie, fewer than two valid nodes, known entries, every active item moves the gradient;
3. label_codes = io.encode bit for bit;
4. content=None / w_content = 0 is dsg_sample_guided_rel, scale = 0 the plain sampler (array_equal, graph_replays included);
5. the loop's arithmetic recomputed in float64 (sanity-check mode, a walk, the chain of dsg_precond calls);
6. the eager guided_sample with ContentGuide.torch_loss on a network whose Jacobian is exactly zero;
7.-10. known and padded entries, batch invariance, the refusals, the poisoned workspace.
profiles/guide_kernel_errors.md holds the largest measured error / bar of every output."""
import ctypes as C

import numpy as np
import pytest
import torch

import box_guide_ref as BR
import content_ref as CR
import guide_ref as GR
from test_box_guide import SCALE, STEP_RTOL, T8, TRAJ_RTOL, VALID, _flags, _gt_inputs, _guide, _net, _np, _sampler, dev
from test_content_guide_host import SHAPES, case, valid_sets
from diffusesg_amd import guide as G
from diffusesg_amd import lib
from diffusesg_amd import spec as S
from diffusesg_amd import synth as Y
from diffusesg_amd import weights as W

pytestmark = pytest.mark.gpu

F32 = np.float32
N_NODE_TYPE, N_ADJ_TYPE = 150, 51   # the tiny configuration: 8 label bits in front of the box, 6 adjacency bits


# ---- 1. the kernel alone ----
def make_cfg(cfg):
    keep = tuple(np.ascontiguousarray(cfg[k], dtype=np.float32) for k in ("subj", "obj", "pred", "w_spo"))
    clip = lib.GUIDE_CLIP_NONE if cfg["clip_ratio"] is None else cfg["clip_ratio"]
    return lib.DsgContentCfg(cfg["w"], cfg["tau"], clip, keep[0].shape[1], cfg["Cl"], 0, *(v.ctypes.data for v in keep)), keep


def run_kernel(xh, D, flags, cfg, coef, mask_adj=None, mask_node=None, expect=0):
    """dsg_debug_content_guide on float32 device copies; float outputs as float32 arrays, best as int"""
    L = lib.load()
    B, N, cn = D[1].shape
    ca, K, Cl = D[0].shape[1], cfg["subj"].shape[1], cfg["Cl"]
    t = [dev(v, torch.float32) for v in (xh[0], xh[1], D[0], D[1])]
    fl = dev(flags.astype(np.uint8))
    ma = None if mask_adj is None else dev(mask_adj.astype(np.uint8))
    mn = None if mask_node is None else dev(mask_node.astype(np.uint8))
    ccfg, keep = make_cfg(cfg)
    shapes = dict(loss=(B,), item_loss=(B, K), grad_adj=(B, ca, N, N), grad_label=(B, N, Cl), shift_adj=(B, ca, N, N), shift_label=(B, N, Cl),
                  factor=(B,), norms=(B, 2), best=(B, K, 2), D_guided_adj=(B, ca, N, N), D_guided_node=(B, N, cn))
    out = {k: (torch.full(s, -7, dtype=torch.int32) if k == "best" else torch.full(s, float("nan"))).cuda() for k, s in shapes.items()}
    p = lambda x: None if x is None else x.data_ptr()
    rc = L.dsg_debug_content_guide(B, N, ca, cn, *(p(x) for x in t), p(fl), p(ma), p(mn), C.byref(ccfg), float(coef),
                                   *(p(out[k]) for k in shapes), torch.cuda.current_stream().cuda_stream)
    assert rc == expect, (rc, L.dsg_last_error(None))
    del keep
    return {k: v.cpu().numpy() for k, v in out.items()}


WORST = {}   # output -> (error / bar, error, bar, case)


def check_kernel(got, xh, D, flags, cfg, coef, ma, mn, tag):
    B, N, Cn = D[1].shape
    Ca, Cl = D[0].shape[1], cfg["Cl"]
    ref = CR.guided_call(xh, D, flags, coef, cfg, ma, mn)
    bars = CR.bars(ref, cfg, N, Ca)
    for k, bar in bars.items():
        assert np.isfinite(got[k]).all(), (tag, k)
        ratio = np.abs(got[k].astype(np.float64) - ref[k]) / bar
        w = float(ratio.max())
        if w >= WORST.get(k, (-1.0,))[0]:
            i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
            WORST[k] = (w, float(np.abs(got[k].astype(np.float64) - ref[k])[i]), float(bar[i]), tag)
        assert w <= 1.0, (tag, k, w)
    assert np.array_equal(got["best"], ref["best"]), (tag, "best")
    # shift and D~ bit for bit from the kernel's own g and f_b
    f = flags.astype(bool)
    cw = F32(coef) * F32(cfg["w"])
    fac = got["factor"].astype(F32)
    ua, ul = cw * got["grad_adj"], cw * got["grad_label"]
    if ma is not None:
        ua, ul = np.where(ma, F32(0), ua), np.where(mn[..., :Cl], F32(0), ul)
    assert np.array_equal(got["shift_adj"], fac[:, None, None, None] * ua) and np.array_equal(got["shift_label"], fac[:, None, None] * ul), tag
    va = np.broadcast_to(f[:, None, :, None] & f[:, None, None, :], D[0].shape)
    want_a = np.where(va, D[0] - got["shift_adj"], F32(0))
    want_n = np.where(f[:, :, None], D[1], F32(0)).astype(F32)
    want_n[..., :Cl] = np.where(f[:, :, None], D[1][..., :Cl] - got["shift_label"], F32(0))
    assert np.array_equal(got["D_guided_adj"], want_a, equal_nan=True) and np.array_equal(got["D_guided_node"], want_n), tag
    # the norm of the unclipped shift from the kernel's own entries (float64 sum, another order: one ulp), the reference norm, the factor
    sn = np.sqrt((ua.astype(np.float64) ** 2).reshape(B, -1).sum(1) + (ul.astype(np.float64) ** 2).reshape(B, -1).sum(1))
    assert (np.abs(got["norms"][:, 0] - sn) <= CR.ulp32(sn) + 1e-12 * sn).all(), tag
    assert (np.abs(got["norms"][:, 1] - ref["norms"][:, 1]) <= CR.ulp32(ref["norms"][:, 1]) + 1e-12 * ref["norms"][:, 1]).all(), tag
    if cfg["clip_ratio"] is None:
        assert (fac == 1).all() and (got["norms"][:, 1] == 0).all()
    else:
        bound = F32(cfg["clip_ratio"]) * got["norms"][:, 1]
        with np.errstate(over="ignore"):   # the branch not taken of a graph whose shift is zero
            want_f = np.where(got["norms"][:, 0] > bound, bound / np.maximum(got["norms"][:, 0], np.finfo(F32).tiny), F32(1)).astype(F32)
        assert np.array_equal(fac, want_f), tag
    # zeros where nothing may move
    dead = ~va | np.broadcast_to(np.eye(N, dtype=bool)[None, None], va.shape)
    assert (got["shift_adj"][dead] == 0).all() and (got["grad_adj"][dead] == 0).all() and (got["shift_label"][~f] == 0).all()
    return ref


def kernel_cases(N, shape):
    Ca, Cn, Cl = shape
    n = 0
    for K in (1, 3, 16):
        for tau in (0.01, 1.0):
            with_mask, clip = bool((n + N) % 2), (None if n % 3 == 2 else 1.0)
            yield dict(K=K, tau=tau, with_mask=with_mask, clip=clip, seed=100 * N + 10 * Ca + n)
            n += 1


# the one-hot widths at N = 8 and N = 64 only
KERNEL_GRID = [(N, s) for N in (1, 2, 8, 40, 64) for s in SHAPES if s[0] != 51 or N in (8, 64)]


@pytest.mark.parametrize("N,shape", KERNEL_GRID, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_kernel_against_float64(N, shape):
    Ca, Cn, Cl = shape
    clipped = []
    for c in kernel_cases(N, shape):
        xh, D, flags, cfg, ma, mn = case(N, Ca, Cn, Cl, c["K"], valid_sets(N), c["seed"], tau=c["tau"], clip=c["clip"], with_mask=c["with_mask"],
                                        xh_scale=[1e-3, 30.0, 1.0, 1.0, 1.0])
        got = run_kernel(xh, D, flags, cfg, 0.37, ma, mn)
        check_kernel(got, xh, D, flags, cfg, 0.37, ma, mn, f"N={N} {shape} K={c['K']} tau={c['tau']} mask={c['with_mask']} clip={c['clip']}")
        if c["clip"] is not None and N >= 2:
            clipped.append(got["factor"])
    if N >= 2:
        fs = np.concatenate(clipped)
        assert (fs < 1).any() and (fs == 1).any(), "a clipped and an unclipped graph must both occur"


def test_kernel_special_cases():
    # a tie: nodes 0 and 2 carry the same label row, the item asks for that label only -> the two slots share pi evenly, and the
    # arg-max is the lowest flat index
    xh, D, flags, cfg, _, _ = case(8, 6, 12, 8, 1, [8, 6], seed=5, clip=None)
    D[1][:, 2, :8] = D[1][:, 0, :8]
    cfg["w_spo"][:] = (1.0, 0.0, 0.0)
    got = run_kernel(xh, D, flags, cfg, 1.0)
    ref = check_kernel(got, xh, D, flags, cfg, 1.0, None, None, "tie")
    assert np.array_equal(got["grad_label"][:, 0], got["grad_label"][:, 2]) and np.abs(got["grad_label"][:, 0]).max() > 0
    assert (got["grad_adj"] == 0).all() and np.array_equal(ref["grad_label"][:, 0], ref["grad_label"][:, 2])
    # fewer than two valid nodes: exact zeros, best = -1, the factor 1
    xh, D, flags, cfg, ma, mn = case(8, 6, 12, 8, 3, [1, 0], seed=6)
    got = run_kernel(xh, D, flags, cfg, 1.0)
    for k in ("loss", "item_loss", "grad_adj", "grad_label", "shift_adj", "shift_label"):
        assert (got[k] == 0).all(), k
    assert (got["best"] == -1).all() and (got["factor"] == 1).all()
    # known entries: the shift is zero there and D arrives bit-exact
    xh, D, flags, cfg, ma, mn = case(8, 6, 12, 8, 6, [8, 5, ("s", 4)], seed=7, with_mask=True, clip=0.5, xh_scale=[1e-3, 30.0, 1.0])
    got = run_kernel(xh, D, flags, cfg, 2.0, ma, mn)
    check_kernel(got, xh, D, flags, cfg, 2.0, ma, mn, "known")
    f = flags.astype(bool)
    live = np.broadcast_to((f[:, :, None] & f[:, None, :] & ~np.eye(8, dtype=bool)[None])[:, None], ma.shape)
    assert (ma & live).any() and np.array_equal(got["D_guided_adj"][ma & live], D[0][ma & live]) and (got["shift_adj"][ma & live] == 0).all()
    kn = mn & np.broadcast_to(f[:, :, None], mn.shape)
    assert kn[..., :8].any() and np.array_equal(got["D_guided_node"][kn], D[1][kn])
    assert np.array_equal(got["D_guided_node"][..., 8:][np.broadcast_to(f[:, :, None], (3, 8, 4))], D[1][..., 8:][np.broadcast_to(f[:, :, None], (3, 8, 4))])
    assert (got["factor"] < 1).any() and (got["factor"] == 1).any()
    # every active item moves the gradient somewhere: each item on its own
    xh, D, flags, cfg, _, _ = case(8, 6, 12, 8, 6, [8, 5], seed=8, clip=None)
    n_active = 0
    for k in range(6):
        one = dict(cfg, w_spo=np.where(np.arange(6)[None, :, None] == k, cfg["w_spo"], 0).astype(F32))
        got = run_kernel(xh, D, flags, one, 1.0)
        a_s, a_o, a_p = cfg["w_spo"][0, k]
        if not cfg["w_spo"][0, k].any():
            assert (got["grad_adj"] == 0).all() and (got["grad_label"] == 0).all() and (got["best"][:, k] == -1).all()
            continue
        n_active += 1
        assert (np.abs(got["grad_adj"]).reshape(2, -1).max(1) > 0).all() == bool(a_p != 0), k
        assert (np.abs(got["grad_label"]).reshape(2, -1).max(1) > 0).all() == bool(a_s != 0 or a_o != 0), k
        assert (got["best"][:, k] >= 0).all()
    assert n_active == 5


@pytest.mark.parametrize("K", [1, 2, 16])
def test_both_forms_give_the_same_bits(K, monkeypatch):
    """the two forms of the content kernel -- one block per graph, and the grid of (item, graph) and (round, graph) blocks that runs by
    default; DSG_CONTENT_GRID forces one -- give every output bit for bit, one-hot widths included"""
    for N, (Ca, Cn, Cl) in ((40, (6, 12, 8)), (8, (51, 154, 150))):
        xh, D, flags, cfg, ma, mn = case(N, Ca, Cn, Cl, K, valid_sets(N), seed=31 + K, tau=0.01, clip=1.0, with_mask=True, xh_scale=[1e-3, 30.0, 1.0, 1.0, 1.0])
        out = {}
        for form in ("0", "1"):
            monkeypatch.setenv("DSG_CONTENT_GRID", form)
            out[form] = run_kernel(xh, D, flags, cfg, 0.37, ma, mn)
        monkeypatch.delenv("DSG_CONTENT_GRID")
        dflt = run_kernel(xh, D, flags, cfg, 0.37, ma, mn)
        for k in out["0"]:
            assert np.array_equal(out["0"][k], out["1"][k], equal_nan=True) and np.array_equal(dflt[k], out["0"][k], equal_nan=True), (N, k)
        check_kernel(out["1"], xh, D, flags, cfg, 0.37, ma, mn, f"grid form N={N} K={K}")


def test_zz_report_worst():
    """prints the largest measured error / bar of every output (profiles/guide_kernel_errors.md); runs after the kernel tests"""
    for k, (w, err, bar, tag) in sorted(WORST.items()):
        print(f"CONTENT kernel worst {k}: err/bar {w:.3f} (err {err:.3e}, bar {bar:.3e}) at {tag}")
    assert all(w <= 1.0 for w, *_ in WORST.values())


# ---- 3. label_codes = io.encode ----
@pytest.mark.parametrize("enc", ["bits", "one_hot", "ddpm"])
def test_label_codes_equal_encode(enc):
    from diffusesg_amd import io as dio
    n_adj_type, n_node_type, n = 7, 13, 16
    chans = {"bits": lambda k: int(np.ceil(np.log2(k))), "one_hot": lambda k: k, "ddpm": lambda k: 1}[enc]
    cfg = S.ModelConfig(max_node_num=n, c_adj=chans(n_adj_type), c_node=chans(n_node_type) + 4, depths=(1, 1), num_heads=(3, 6), window_size=4,
                        self_condition=True)
    h = lib.Handle(cfg)
    q_node = (np.arange(n, dtype=np.int32) % n_node_type)[None]
    q_adj = ((np.arange(n * n, dtype=np.int32) * 3) % n_adj_type).reshape(1, n, n)
    flags = np.ones((1, n), np.uint8)
    a, x = dio.encode(h, dev(q_adj), dev(q_node), dev(np.zeros((1, n, 4), F32)), dev(flags), n_adj_type, n_node_type, enc, enc)
    nc, pc = G.label_codes(n_node_type, enc, chans(n_node_type)), G.label_codes(n_adj_type, enc, chans(n_adj_type))
    assert np.array_equal(x[0, :, :-4].cpu().numpy(), nc[q_node[0]]) and np.array_equal(a[0].cpu().numpy(), pc[q_adj[0]].transpose(2, 0, 1))


# ---- loops ----
def _content(flags_np, seed=3, **kw):
    """a ContentGuide for a batch of the tiny configuration with these flags: triplets, a unary item, a predicate-only item, a graph
    with fewer items -- and the dict content_ref takes"""
    B = flags_np.shape[0]
    rng = np.random.default_rng(seed)
    items = []
    for b in range(B):
        row = [(int(rng.integers(N_NODE_TYPE)), int(rng.integers(N_ADJ_TYPE)), int(rng.integers(N_NODE_TYPE))), (int(rng.integers(N_NODE_TYPE)), None, None),
               (None, int(rng.integers(N_ADJ_TYPE)), None)]
        items.append(row[:3 - (b % 2)])
    args = dict(weight=0.7, tau=0.5, clip_ratio=0.3)
    args.update(kw)
    cg = G.ContentGuide(items, N_NODE_TYPE, N_ADJ_TYPE, **args)
    subj, obj, pred, w_spo = cg.tensors(6, 8)
    return cg, dict(Cl=8, tau=args["tau"], w=args["weight"], clip_ratio=args["clip_ratio"], subj=subj, obj=obj, pred=pred, w_spo=w_spo)


def _both(xh, D, flags, c, clip, gkw, ckw):
    """the guided estimate with the box terms and the content term: disjoint channels, independent clips"""
    rb = BR.guided_call(xh, D, flags, c, clip, **gkw)
    rc = CR.guided_call(xh, D, flags, c, ckw)
    Gn = rb["D_guided"].copy()
    Gn[..., :ckw["Cl"]] -= rc["shift_label"]
    return rb, rc, (rc["D_guided_adj"], Gn)


def _recompute(solver, clip, sched, noise_coef, ms, snaps, traces, gkw, ckw, flags, ia, inn, na, nn, ga, gn, smp):
    sg, t_hat, _nc, h_step = lib.sigma_schedule(smp._cfg())
    cw = lib.guide_coef(smp._cfg(), SCALE.astype(F32))
    T = smp.num_steps
    adjs_ls, nodes_ls = snaps
    x = (ia * F32(sg[0]), inn * F32(sg[0]))
    D = (ga.astype(np.float64), gn.astype(np.float64))
    prev, n_clip = None, [0, 0]
    for k, i in enumerate(sched):
        xh = tuple((x[j].astype(F32) + F32(noise_coef[k]) * (na, nn)[j][k]).astype(F32) if noise_coef[k] != 0 else x[j] for j in range(2))
        xh = (W.mask_adj(xh[0], flags), W.mask_node(xh[1], flags))
        rb, rc, Gd = _both(xh, D, flags, cw[i], clip, gkw, ckw)
        n_clip[0] += int((rb["factor"] < 1).any())
        n_clip[1] += int((rc["factor"] < 1).any())
        t, h = float(t_hat[i]), float(h_step[i])
        ref = GR.heun_update(xh, Gd, Gd, t, h, flags) if solver == "heun" and i != T - 1 else GR.euler_update(xh, Gd, t, h, flags, float(ms[k]), prev)
        got = (adjs_ls[k + 1], nodes_ls[k + 1])
        for j, what in enumerate(("adj", "node")):
            err = float(np.abs(got[j].astype(np.float64) - ref[j]).max()) / max(float(np.abs(xh[j]).max()), 1e-30)
            assert err <= STEP_RTOL, f"step {k} (schedule index {i}) {what}: {err:.3e}"
        bL = CR.bars(rc, ckw, flags.shape[1], ga.shape[1])["loss"]
        assert (np.abs(traces[1][k].astype(np.float64) - rc["loss"]) <= bL).all(), f"content trace row {k}"
        assert np.abs(traces[0][k].astype(np.float64) - rb["loss"]).max() <= 4 * BR_ULP * max(1.0, np.abs(rb["loss"]).max())
        prev, x = Gd, got
    return n_clip, rc


BR_ULP = float(np.finfo(F32).eps)


def _gt_kwargs(ia, inn, na, nn, ga, gn):
    return dict(init_adjs=torch.from_numpy(ia), init_nodes=torch.from_numpy(inn), churn_noise=(torch.from_numpy(na), torch.from_numpy(nn)),
                sanity_check_gt_adjs=torch.from_numpy(ga), sanity_check_gt_nodes=torch.from_numpy(gn), flag_interim_adjs=True, return_loss_trace=True)


@pytest.mark.parametrize("clip", [0.02, None])
@pytest.mark.parametrize("solver", ["euler", "heun", "dpmpp_2m"])
def test_loop_arithmetic_recomputed_in_float64(solver, clip):
    flags, ia, inn, na, nn, ga, gn = _gt_inputs()
    net, smp = _net("tiny"), _sampler("tiny", solver)
    guide, gkw = _guide(flags)
    cg, ckw = _content(flags, clip_ratio=clip)
    a, n, adjs_ls, nodes_ls, trace, ctrace = _np(smp.sample_guided(net, torch.from_numpy(flags), guide, SCALE, clip_ratio=clip, content=cg,
                                                                   **_gt_kwargs(ia, inn, na, nn, ga, gn)))
    assert adjs_ls.shape[0] == T8 + 1 and trace.shape == ctrace.shape == (T8, 3)
    nc, ms = lib.sigma_schedule(smp._cfg())[2], lib.multistep_coef(smp._cfg())
    n_clip, last = _recompute(solver, clip, list(range(T8)), nc, ms, (adjs_ls, nodes_ls), (trace, ctrace), gkw, ckw, flags, ia, inn, na, nn, ga, gn, smp)
    if clip is not None:
        assert n_clip[0] > 0 and n_clip[1] > 0, "a clip never engaged: the case does not test it"
    assert np.abs(last["shift_adj"]).max() > 0 and np.abs(last["shift_label"]).max() > 0
    assert np.abs(a.astype(np.float64) - last["D_guided_adj"]).max() <= STEP_RTOL * np.abs(ga).max()   # the last step runs to t = 0


def test_walk_and_step_graph_switch():
    """a content-guided RePaint walk in the sanity-check mode, every executed step recomputed with the coefficient of ITS schedule index;
    and on the real network: replayed content-guided bodies equal enqueued ones"""
    flags, ia, inn, na, nn, ga, gn = _gt_inputs(walk=True)
    net, smp = _net("tiny"), _sampler("tiny", "euler")
    guide, gkw = _guide(flags)
    cg, ckw = _content(flags, clip_ratio=None)
    sched, coef = lib.walk_steps(smp._cfg(), lib.make_walk_cfg(0, (2, 2), (2, 6)))
    a, n, adjs_ls, nodes_ls, trace, ctrace = _np(smp.sample_guided(net, torch.from_numpy(flags), guide, SCALE, clip_ratio=None, content=cg,
                                                                   resample=(2, 2), resample_range=(2, 6), **_gt_kwargs(ia, inn, na, nn, ga, gn)))
    assert ctrace.shape == (12, 3) and adjs_ls.shape[0] == 13
    _recompute("euler", None, sched.tolist(), coef, np.zeros(12), (adjs_ls, nodes_ls), (trace, ctrace), gkw, ckw, flags, ia, inn, na, nn, ga, gn, smp)
    fl = _flags("tiny")
    cg, _ = _content(fl.numpy())
    h = net.model._ensure_handle()
    old = h.get_option("loop_graph")
    runs = {}
    try:
        for solver in ("euler", "heun", "dpmpp_2m"):
            smp = _sampler("tiny", solver)
            coins = (np.random.default_rng(3).random(2 * T8) < 0.5).astype(np.uint8)
            for loop_graph in (1, 0):
                h.set_option("loop_graph", loop_graph)
                runs[loop_graph] = _np(smp.sample_guided(net, fl, guide, SCALE, content=cg, seed=5, coins=coins, return_device=True))
            assert all(np.array_equal(g, r) for g, r in zip(runs[1], runs[0])), f"replayed and enqueued content-guided bodies differ ({solver})"
    finally:
        h.set_option("loop_graph", old)


# ---- 4. off means off ----
@pytest.mark.parametrize("solver", ["euler", "heun", "dpmpp_2m"])
def test_content_off_is_the_box_guided_run(solver):
    cfg = Y.CONFIGS["tiny"]()
    net, smp, fl = _net("tiny"), _sampler("tiny", solver), _flags("tiny")
    guide, _ = _guide(fl.numpy())
    cg, _ = _content(fl.numpy())
    cg0, _ = _content(fl.numpy(), weight=0.0)
    coins = (np.random.default_rng(3).random(2 * T8) < 0.5).astype(np.uint8)
    kw = dict(seed=5, coins=coins, return_device=True)
    ref = _np(smp.sample_guided(net, fl, guide, SCALE, clip_ratio=0.5, **kw))
    st_ref = dict(smp.last_stats)
    for c in (None, cg0):
        got = _np(smp.sample_guided(net, fl, guide, SCALE, clip_ratio=0.5, content=c, **kw))
        assert all(np.array_equal(g, r) for g, r in zip(got, ref)) and smp.last_stats == st_ref
    on = _np(smp.sample_guided(net, fl, guide, SCALE, clip_ratio=0.5, content=cg, **kw))
    assert not np.array_equal(on[0], ref[0]) and not np.array_equal(on[1][..., :8], ref[1][..., :8]) and smp.last_stats == st_ref
    off = smp.sample_guided(net, fl, guide, SCALE, clip_ratio=0.5, content=cg0, return_loss_trace=True, **kw)
    assert len(off) == 4 and (off[3] == 0).all(), "weight = 0: the term is not evaluated, its trace is zeros"
    plain = _np(smp.sample(net, fl, num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj, **kw))
    zero = _np(smp.sample_guided(net, fl, guide, 0.0, content=cg, **kw))
    assert all(np.array_equal(g, r) for g, r in zip(zero, plain)), "scale = 0 is the plain sampler"
    from diffusesg_amd.guide import BoxGuide
    only = _np(smp.sample_guided(net, fl, BoxGuide(), SCALE, content=cg, **kw))   # a content-only run: a guide with every weight 0
    assert not np.array_equal(only[0], plain[0]) and not np.array_equal(only[1][..., :8], plain[1][..., :8])


# ---- 6. against the eager loop ----
@pytest.mark.parametrize("solver", ["euler", "heun"])
def test_against_the_eager_loop_with_zero_jacobian(solver):
    from diffusesg_amd.guide import BoxGuide, guided_sample
    cfg = Y.CONFIGS["tiny"]()
    net, smp, fl = _net("tiny", True), _sampler("tiny", solver), _flags("tiny")
    cg, _ = _content(fl.numpy(), clip_ratio=1.0, weight=1.0)
    np.random.seed(21)
    got = _np(smp.sample_guided(net, fl, BoxGuide(), SCALE, clip_ratio=1.0, content=cg, seed=9, return_device=True))
    np.random.seed(21)
    ref = _np(guided_sample(net, smp, fl, cg.torch_loss(fl), SCALE, clip_ratio=1.0, seed=9))
    np.random.seed(21)
    plain = _np(smp.sample(net, fl, seed=9, num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj, return_device=True))
    torch.cuda.synchronize()
    for what, g, r, p in zip(("adj", "node"), got, ref, plain):
        s = float(np.abs(r).max())
        err, moved = float(np.abs(g - r).max()) / s, float(np.abs(g - p).max()) / s
        print(f"CONTENT eager {solver} {what}: |in-loop - eager| {err:.3e}, |guided - unguided| {moved:.3e} of the result's scale")
        assert g.shape == r.shape and err <= TRAJ_RTOL, (what, err)
        assert moved > 100 * TRAJ_RTOL, "the guidance moves nothing: the case tests nothing"


# ---- 5c. with the real synthetic network ----
def test_real_network_chain_recomputed_in_float64():
    net, smp, fl = _net("tiny"), _sampler("tiny", "euler", churn=0), _flags("tiny")
    flags = fl.numpy()
    guide, gkw = _guide(flags)
    cg, ckw = _content(flags)
    coins = np.zeros(T8, np.uint8)
    a, n, adjs_ls, nodes_ls, trace, ctrace = _np(smp.sample_guided(net, fl, guide, SCALE, clip_ratio=0.5, content=cg, seed=13, coins=coins,
                                                                   flag_interim_adjs=True, return_loss_trace=True))
    sg, t_hat, _nc, h_step = lib.sigma_schedule(smp._cfg())
    cw = lib.guide_coef(smp._cfg(), SCALE.astype(F32))
    hd = net.model._ensure_handle()
    fl8 = fl.to(torch.uint8).cuda()
    sc = (None, None)
    p = lambda v: None if v is None else v.data_ptr()
    for i in range(T8):
        x = (adjs_ls[i] * F32(sg[0]), nodes_ls[i] * F32(sg[0])) if i == 0 else (adjs_ls[i], nodes_ls[i])
        xa, xn = dev(x[0]), dev(x[1])
        sig = torch.full((3,), float(t_hat[i]), dtype=torch.float32, device="cuda")
        Da, Dn = torch.empty_like(xa), torch.empty_like(xn)
        hd.check(hd.L.dsg_precond(hd.raw, 3, p(xa), p(xn), p(fl8), p(sig), p(sc[0]), p(sc[1]), 0, p(Da), p(Dn),
                                  torch.cuda.current_stream().cuda_stream), "dsg_precond")
        torch.cuda.synchronize()
        sc = (Da, Dn)                                      # the self-conditioning input of the next call is D, not D~
        D = (Da.cpu().numpy().astype(np.float64), Dn.cpu().numpy().astype(np.float64))
        rb, rc, Gd = _both(x, D, flags, cw[i], 0.5, gkw, ckw)
        ref = GR.euler_update(x, Gd, float(t_hat[i]), float(h_step[i]), flags)
        for j, what in enumerate(("adj", "node")):
            err = float(np.abs((adjs_ls, nodes_ls)[j][i + 1].astype(np.float64) - ref[j]).max()) / max(float(np.abs(x[j]).max()), 1e-30)
            print(f"CONTENT chain step {i} {what}: {err:.3e}")
            assert err <= TRAJ_RTOL, (i, what, err)
        # D here is the recomputed estimate of another launch sequence: the trace is held to the trajectory bar, of the loss's scale
        errL = float(np.abs(ctrace[i].astype(np.float64) - rc["loss"]).max())
        assert errL <= TRAJ_RTOL * max(1.0, float(np.abs(rc["loss"]).max())), (i, errL)


# ---- 7. / 8. invariants ----
def test_known_entries_exact_and_padded_entries_zero():
    cfg = Y.CONFIGS["tiny"]()
    net, fl = _net("tiny"), _flags("tiny")
    flags = fl.numpy()
    guide, _ = _guide(flags)
    cg, _ = _content(flags)
    rng = np.random.default_rng(4)
    ka = np.sign(rng.standard_normal((3, cfg.c_adj, 8, 8))).astype(F32)
    kn = (np.sign(rng.standard_normal((3, 8, cfg.c_node))) * 0.7).astype(F32)
    ma, mn = rng.random(ka.shape) < 0.4, rng.random(kn.shape) < 0.4
    known = tuple(torch.from_numpy(v) for v in (ka, kn, ma, mn))
    va, vn = np.broadcast_to(flags[:, None, :, None] & flags[:, None, None, :], ka.shape), np.broadcast_to(flags[:, :, None], kn.shape)
    for solver in ("euler", "heun", "dpmpp_2m"):
        smp = _sampler("tiny", solver)
        coins = (np.random.default_rng(6).random(2 * T8) < 0.5).astype(np.uint8)
        kw = dict(seed=7, coins=coins, flag_interim_adjs=True)
        ga, gn, gal, gnl = _np(smp.sample_guided(net, fl, guide, SCALE, known=known, clip_ratio=0.5, content=cg, **kw))
        pa, pn, pal, pnl = _np(smp.sample_known(net, fl, *known, num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj, **kw))
        # a known entry's trajectory is a function of its own noise and the known value: equal at EVERY step exactly when every guided
        # estimate carried the known value bit for bit
        assert np.array_equal(gal[:, ma & va], pal[:, ma & va]) and np.array_equal(gnl[:, mn & vn], pnl[:, mn & vn]), solver
        assert not np.array_equal(ga[~ma & va], pa[~ma & va]) and not np.array_equal(gn[~mn & vn], pn[~mn & vn])
        assert (gal[:, ~va] == 0).all() and (gnl[:, ~vn] == 0).all() and (ga[~va] == 0).all() and (gn[~vn] == 0).all()


def test_a_graph_alone_equals_the_graph_in_a_batch():
    net, fl = _net("tiny"), _flags("tiny")
    flags = fl.numpy()
    cg, _ = _content(flags)
    from diffusesg_amd.guide import BoxGuide
    h = net.model._ensure_handle()
    old = h.get_option("batch_invariant")
    try:
        h.set_option("batch_invariant", 1)
        for solver in ("euler", "dpmpp_2m"):
            smp = _sampler("tiny", solver)
            seeds = [2 ** 64 - 1, 2 ** 32 + 5, 1]
            kw = dict(coin_seed=3, clip_ratio=0.5)
            full = _np(smp.sample_guided(net, fl, BoxGuide(overlap=1.0), SCALE, content=cg, graph_seeds=seeds, **kw))
            for b in range(3):
                one = G.ContentGuide([cg.items[b]], N_NODE_TYPE, N_ADJ_TYPE, weight=cg.weight, tau=cg.tau, clip_ratio=cg.clip_ratio)
                one.n_items = cg.n_items
                alone = _np(smp.sample_guided(net, fl[b:b + 1], BoxGuide(overlap=1.0), SCALE, content=one, graph_seeds=seeds[b:b + 1], **kw))
                assert np.array_equal(alone[0][0], full[0][b]) and np.array_equal(alone[1][0], full[1][b]), (solver, b)
    finally:
        h.set_option("batch_invariant", old)


# ---- 9. refusals ----
def test_refusals_name_the_argument():
    net, smp, fl = _net("tiny"), _sampler("tiny", "euler"), _flags("tiny")
    flags = fl.numpy()
    cg, ckw = _content(flags)
    h = net.model._ensure_handle()
    L = h.L
    B, n = 3, 8
    fl8 = fl.to(torch.uint8).cuda()
    oa, on = torch.empty((B, 6, n, n), device="cuda"), torch.empty((B, n, 12), device="cuda")
    gw = np.ones(T8, F32)
    gcfg = lib.DsgGuideCfg(0, 0, 0, 0.05, 1.0, 0, None, None, gw.ctypes.data)
    scfg = smp._cfg()
    coins = np.zeros(T8, np.uint8)

    def call(ccfg):
        stats = lib.DsgSampleStats()
        return L.dsg_sample_guided_content(h.raw, C.byref(scfg), None, B, fl8.data_ptr(), None, C.c_uint64(5), None, None, None, None, None, None,
                                           coins.ctypes.data, None, None, None, None, None, 0, None, None, C.byref(gcfg), None, None, None,
                                           oa.data_ptr(), on.data_ptr(), C.byref(stats), torch.cuda.current_stream().cuda_stream, None,
                                           None if ccfg is None else C.byref(ccfg), None)

    base = dict(ckw)
    bad_t = {k: base[k].copy() for k in ("subj", "obj", "pred", "w_spo")}
    bad_t["subj"][1, 0, 2] = np.inf
    bad_p = {k: base[k].copy() for k in ("subj", "obj", "pred", "w_spo")}
    bad_p["pred"][0, 0, 0] = np.nan
    neg_w = {k: base[k].copy() for k in ("subj", "obj", "pred", "w_spo")}
    neg_w["w_spo"][2, 0, 1] = -1.0
    bad_o = {k: base[k].copy() for k in ("subj", "obj", "pred", "w_spo")}
    bad_o["obj"][2, 0, 7] = -np.inf
    inf_w = {k: base[k].copy() for k in ("subj", "obj", "pred", "w_spo")}
    inf_w["w_spo"][0, 0, 2] = np.inf
    nan_w = {k: base[k].copy() for k in ("subj", "obj", "pred", "w_spo")}
    nan_w["w_spo"][1, 0, 0] = np.nan
    cases = [(dict(w=np.inf), "w_content"), (dict(w=np.nan), "w_content"), (dict(tau=0.0), "tau"), (dict(tau=np.nan), "tau"),
             (dict(clip_ratio=-1.0), "clip_ratio"), (dict(clip_ratio=np.nan), "clip_ratio"), (dict(Cl=0), "node_chans"), (dict(Cl=9), "node_chans"),
             (bad_t, "subj"), (bad_o, "obj"), (bad_p, "pred"), (neg_w, "w_spo"), (inf_w, "w_spo"), (nan_w, "w_spo")]
    for change, name in cases:
        ccfg, keep = make_cfg(dict(base, **change))
        assert call(ccfg) == lib.DSG_ERR_INVALID and name in L.dsg_last_error(h.raw).decode(), (name, L.dsg_last_error(h.raw))
    for k_items in (0, 17):
        ccfg, keep = make_cfg(base)
        ccfg.n_items = k_items
        assert call(ccfg) == lib.DSG_ERR_INVALID and "n_items" in L.dsg_last_error(h.raw).decode()
    for field in ("subj", "obj", "pred", "w_spo"):
        ccfg, keep = make_cfg(base)
        setattr(ccfg, field, None)
        assert call(ccfg) == lib.DSG_ERR_INVALID and field in L.dsg_last_error(h.raw).decode()
    # what dsg_sample_guided_rel refuses: no weights
    ccfg, keep = make_cfg(base)
    gcfg.weights = None
    assert call(ccfg) == lib.DSG_ERR_INVALID and "weights" in L.dsg_last_error(h.raw).decode()
    gcfg.weights = gw.ctypes.data
    # N > 64: the kernel's hook (no handle), the message naming N
    xh, D, f65, cfg65, _, _ = case(65, 2, 6, 2, 1, [65], seed=1, nan=False)
    run_kernel(xh, D, f65, cfg65, 1.0, expect=lib.DSG_ERR_INVALID)
    assert "N = 65" in lib.load().dsg_last_error(None).decode()
    # the handle is usable afterwards
    ccfg, keep = make_cfg(base)
    assert call(ccfg) == 0 and call(None) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(oa).all() and torch.isfinite(on).all()


# ---- 10. the poisoned workspace ----
def test_poisoned_workspace_changes_no_bit():
    net, fl = _net("tiny"), _flags("tiny")
    flags = fl.numpy()
    guide, _ = _guide(flags)
    cg, _ = _content(flags)
    h = net.model._ensure_handle()
    for solver in ("heun", "dpmpp_2m"):
        smp = _sampler("tiny", solver)
        coins = (np.random.default_rng(6).random(2 * T8) < 0.5).astype(np.uint8)
        kw = dict(seed=7, coins=coins, clip_ratio=0.5, content=cg, return_loss_trace=True, return_device=True)
        ref = _np(smp.sample_guided(net, fl, guide, SCALE, **kw))
        for pattern in (2, 3, 4):
            h.poison(3, pattern, 17)
            got = _np(smp.sample_guided(net, fl, guide, SCALE, **kw))
            assert all(np.array_equal(g, r) for g, r in zip(got, ref)), (solver, pattern)
    assert h.L.dsg_workspace_bytes(h.raw, 3) > 0
