"""GPU: box guidance through the skip path inside the reverse loop (dsg_sample_guided).

1. the guide kernel alone (dsg_debug_box_guide) against the float64 restatement of tests/box_guide_ref.py, NaN in every padded row;
2. the loop's arithmetic without a network (sanity-check mode): every step recomputed in float64 from the snapshots;
3. zero weights are the plain sampler, bit for bit; replayed guided bodies equal enqueued ones;
4. against the eager loop guide.guided_sample on a network whose Jacobian is exactly zero;
5. with the real synthetic network: the chain of dsg_precond calls, shifted and stepped in float64; the loss trace;
6. invariants: known and padded entries, other configurations, a refusal, a resampling walk, batch invariance, layout_from_graph.

Kernel bar, per loss: 16 x the discrepancy of guide.py's closure under torch float32 autograd on the CPU against float64 on the same
inputs, relative to the tensor's maximum, with a floor of 8 float32 ulp (profiles/guide_kernel_errors.md holds the measured figures)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import box_guide_ref as BR
import guide_ref as GR
from test_box_guide_host import LOSSES, box_guide_of, case, torch_loss_grad
from diffusesg_amd import lib
from diffusesg_amd import synth as Y
from diffusesg_amd import weights as W

pytestmark = pytest.mark.gpu

T8 = 8
TRAJ_RTOL = 1e-4    # the project's T = 8 trajectory bar
STEP_RTOL = 1e-6    # one step recomputed in float64, of the state's scale (test_every_step_recomputed_in_float64)
ULP = float(np.finfo(np.float32).eps)
VALID = [8, 5, 3]


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


# ---- 1. the kernel alone ----
def run_kernel(xh, D, flags, kw, coef, clip, sel=None, region=None, mask_node=None):
    """dsg_debug_box_guide on float32 device copies; returns the outputs as float64 arrays"""
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
    out = dict(loss=torch.empty(B), grad=torch.empty(B, N, 4), shift=torch.empty(B, N, 4), factor=torch.empty(B), norms=torch.empty(B, 2),
               D_guided=torch.empty(B, N, cn))
    out = {k: v.cuda() for k, v in out.items()}
    p = lambda x: None if x is None else x.data_ptr()
    rc = L.dsg_debug_box_guide(B, N, ca, cn, *(p(x) for x in t), p(fl), p(mk), C.byref(cfg), float(coef),
                               *(p(out[k]) for k in ("loss", "grad", "shift", "factor", "norms", "D_guided")),
                               torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (rc, L.dsg_last_error(None))
    return {k: v.cpu().numpy().astype(np.float64) for k, v in out.items()}


def kernel_bars(D32, flags, sel, region, kw):
    """(loss bar, gradient bar) of one case: 16 x |torch float32 autograd - float64| on the CPU, floor 8 ulp, both of the tensor's maximum"""
    clean = np.where(flags[:, :, None] != 0, D32, 0.0)   # torch's closures multiply by the flags: no NaN for them
    L64, g64 = torch_loss_grad(clean.astype(np.float64), flags, sel, region, kw, torch.float64)
    L32, g32 = torch_loss_grad(clean.astype(np.float64), flags, sel, region, kw, torch.float32)
    bar = lambda a, b: max(16 * float(np.abs(a - b).max()), 8 * ULP * float(np.abs(b).max()))
    return bar(L32, L64), bar(g32, g64), float(np.abs(L32 - L64).max()), float(np.abs(g32 - g64).max())


def kernel_case(N, cn, valid, seed, which, clip=1.0, coef=0.37, with_mask=False, xh_scale=None):
    D, flags, sel, region = case(N, cn, valid, seed)
    rng = np.random.default_rng(seed + 1000)
    B, ca = len(valid), 2
    D32 = D.astype(np.float32)
    Da = rng.standard_normal((B, ca, N, N)).astype(np.float32)
    scale = np.ones(B) if xh_scale is None else np.asarray(xh_scale, dtype=np.float64)
    xa = (Da + scale[:, None, None, None] * rng.standard_normal(Da.shape)).astype(np.float32)
    xn = (D32 + scale[:, None, None] * rng.standard_normal(D32.shape)).astype(np.float32)
    pad = flags == 0
    for v in (D32, xn):
        v[pad] = np.nan                                  # NaN in every padded row ...
    for v in (Da, xa):
        v[np.broadcast_to(pad[:, None, :, None] | pad[:, None, None, :], v.shape)] = np.nan   # ... and at every padded pair
    mask = (rng.random(D32.shape) < 0.3) if with_mask else None
    kw = LOSSES[which]
    use_r = kw.get("a_r", 0.0) != 0
    got = run_kernel((xa, xn), (Da, D32), flags, kw, coef, clip, sel if use_r else None, region if use_r else None, mask)
    ref = BR.guided_call((xa, xn), (Da.astype(np.float64), D32.astype(np.float64)), flags, np.float32(coef), clip, mask_node=mask,
                         sel=sel, region=region, **kw)
    return got, ref, (D32, flags, sel, region, kw, mask)


def check_kernel(got, ref, D32, flags, sel, region, kw, coef, tag):
    bL, bg, dL, dg = kernel_bars(D32, flags, sel, region, kw)
    gmax, dmax = float(np.abs(ref["grad"]).max()), float(np.nanmax(np.abs(np.where(flags[:, :, None] != 0, D32, 0.0)), initial=0.0))
    bars = dict(loss=bL, grad=bg, shift=abs(coef) * bg + 8 * ULP * abs(coef) * gmax,
                factor=8 * ULP, norms=8 * ULP * max(float(np.abs(ref["norms"]).max()), 1e-30))
    bars["D_guided"] = bars["shift"] + 8 * ULP * dmax
    for k, bar in bars.items():
        assert np.isfinite(got[k]).all(), (tag, k)
        err = float(np.abs(got[k] - ref[k]).max())
        print(f"BOXGUIDE kernel {tag} {k}: err {err:.3e} bar {bar:.3e} (torch f32 vs f64: loss {dL:.3e}, grad {dg:.3e})")
        assert err <= bar, (tag, k, err, bar)
    assert (got["grad"][flags == 0] == 0).all() and (got["shift"][flags == 0] == 0).all() and (got["D_guided"][flags == 0] == 0).all()


def valid_sets(N):
    """valid counts {0, 1, 2, N} spread over batches of three (where N allows it)"""
    sets = [[0, 1, N], [min(2, N), N, 1]]
    return [s for k, s in enumerate(sets) if s not in sets[:k]]


@pytest.mark.parametrize("cn", [4, 5, 12])
@pytest.mark.parametrize("N", [1, 2, 8, 40, 64])
def test_kernel_against_float64(N, cn):
    for vi, valid in enumerate(valid_sets(N)):
        for which in sorted(LOSSES):
            for clip in (1.0, None):
                got, ref, (D32, flags, sel, region, kw, _m) = kernel_case(N, cn, valid, seed=10 * N + cn + vi, which=which, clip=clip)
                check_kernel(got, ref, D32, flags, sel, region, kw, 0.37, f"N={N} C={cn} valid={valid} {which} clip={clip}")


def test_kernel_special_cases():
    """identical boxes, touching boxes and a box of negative extent are in the cases (test_box_guide_host.case); here they are shown to
    be there, a clipped and an unclipped graph both occur, and a known mask zeroes the shift and leaves D bit-exact"""
    got, ref, (D32, flags, sel, region, kw, mask) = kernel_case(8, 5, [8, 5, 3], seed=77, which="all", clip=0.5, coef=2.0, with_mask=True,
                                                                xh_scale=[1e-3, 30.0, 1.0])
    check_kernel(got, ref, D32, flags, sel, region, kw, 2.0, "special")
    assert np.array_equal(D32[0, 0, -4:], D32[0, 1, -4:])                                                  # ties
    b = D32[1, :2, -4:].astype(np.float64) * 0.5 + 0.5
    assert b[0, 0] + 0.5 * b[0, 2] == b[1, 0] - 0.5 * b[1, 2]                                              # touching
    assert (D32[:, 2, -2] * 0.5 + 0.5 < 0).all()                                                           # negative extent
    f = got["factor"]
    print(f"BOXGUIDE kernel special: clip factors {f}, norms {got['norms'].tolist()}")
    assert (f < 1).any() and (f == 1).any(), "a clipped and an unclipped graph must both occur"
    assert np.array_equal(f < 1, ref["factor"] < 1)
    known = mask[..., -4:] & (flags[:, :, None] != 0)
    assert known.any() and (got["shift"][known] == 0).all()
    assert np.array_equal(got["D_guided"][..., -4:][known], D32[..., -4:][known].astype(np.float64))
    other = np.broadcast_to((flags != 0)[:, :, None], D32.shape).copy()
    other[..., -4:] = False
    assert np.array_equal(got["D_guided"][other], D32[other].astype(np.float64))                           # nothing outside the box channels


# ---- networks and samplers ----
@functools.lru_cache(maxsize=None)
def _net(name, zero_heads=False):
    from diffusesg_amd.model import build_network
    cfg = Y.CONFIGS[name]()
    sd = W.synth_state_dict(cfg, 0)
    if zero_heads:   # the last linear of both read-out heads: F = 0 whatever the input, the network's Jacobian vanishes exactly
        hit = [k for k in sd if k.endswith(("readout_adj_mlp.fc2.weight", "readout_adj_mlp.fc2.bias", "readout_node_mlp.fc2.weight", "readout_node_mlp.fc2.bias"))]
        assert len(hit) == 4
        for k in hit:
            sd[k] = np.zeros_like(sd[k])
    return build_network(cfg, sd, device="cuda")


def _sampler(name, solver, churn=None, **kw):
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    cfg = Y.CONFIGS[name]()
    churn = (0 if solver == "dpmpp_2m" else 40) if churn is None else churn
    return NodeAdjEDMSamplerHip(num_steps=T8, solver=solver, S_churn=churn, self_condition=cfg.self_condition, **kw)


def _flags(name, valid=VALID):
    return torch.from_numpy(W.synth_flags(len(valid), Y.CONFIGS[name]().max_node_num, valid))


def _np(ts):
    return tuple(v.detach().cpu().numpy() for v in ts)


def _guide(flags_np, seed=5, **kw):
    """a BoxGuide with all three terms on a batch with these flags (its region: random rectangles on 60 % of the nodes)"""
    from diffusesg_amd.guide import BoxGuide
    B, N = flags_np.shape
    rng = np.random.default_rng(seed)
    sel = (rng.random((B, N)) < 0.6).astype(np.uint8)
    lo = rng.uniform(0.0, 0.5, (B, N, 2))
    region = np.concatenate([lo, lo + rng.uniform(0.1, 0.4, (B, N, 2))], -1).astype(np.float32)
    args = dict(overlap=1.0, align=0.5, tau=0.05, region_weight=0.8)
    args.update(kw)
    return BoxGuide(region=(torch.from_numpy(sel), torch.from_numpy(region)), **args), dict(
        a_o=args["overlap"], a_r=args["region_weight"], a_a=args["align"], tau=args["tau"], sel=sel, region=region.astype(np.float64))


SCALE = np.linspace(3.0, 0.5, T8)


# ---- 2. loop arithmetic without a network ----
@functools.lru_cache(maxsize=None)
def _gt_inputs(walk=False):
    cfg = Y.CONFIGS["tiny"]()
    L = 12 if walk else T8
    flags, ia, inn, na, nn, _cv = Y.sampler_case(cfg, L, 3, VALID, 31, "boxguide/gt")
    rng = np.random.default_rng(8)
    ga = W.mask_adj(rng.uniform(-1, 1, ia.shape).astype(np.float32), flags)
    gn = W.mask_node(rng.uniform(-1, 1, inn.shape).astype(np.float32), flags)
    gn[..., -2:] = W.mask_node(rng.uniform(-0.9, 0.2, gn[..., -2:].shape).astype(np.float32), flags)
    return flags, ia, inn, na, nn, ga, gn


def _recompute_gt_run(solver, clip, sched, noise_coef, ms, snaps, trace, gkw, flags, ia, inn, na, nn, ga, gn, smp):
    """every executed step of a sanity-check run in float64 from the state in front of it; returns the number of clipped calls"""
    sg, t_hat, _nc, h_step = lib.sigma_schedule(smp._cfg())
    cw = lib.guide_coef(smp._cfg(), SCALE.astype(np.float32))
    T = smp.num_steps
    adjs_ls, nodes_ls = snaps
    x = (ia * np.float32(sg[sched[0]]) if sched[0] == 0 else None, inn * np.float32(sg[sched[0]]) if sched[0] == 0 else None)
    D = (ga.astype(np.float64), gn.astype(np.float64))
    n_clipped, prev = 0, None
    L_ref = None
    for k, i in enumerate(sched):
        xh = tuple((x[j].astype(np.float32) + np.float32(noise_coef[k]) * (na, nn)[j][k]).astype(np.float32) if noise_coef[k] != 0 else x[j] for j in range(2))
        xh = (W.mask_adj(xh[0], flags), W.mask_node(xh[1], flags))
        r = BR.guided_call(xh, D, flags, cw[i], clip, **gkw)
        n_clipped += int((r["factor"] < 1).any())
        L_ref = r["loss"]
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
@pytest.mark.parametrize("solver", ["euler", "heun", "dpmpp_2m"])
def test_loop_arithmetic_recomputed_in_float64(solver, clip):
    flags, ia, inn, na, nn, ga, gn = _gt_inputs()
    net, smp = _net("tiny"), _sampler("tiny", solver)
    guide, gkw = _guide(flags)
    a, n, adjs_ls, nodes_ls, trace = smp.sample_guided(
        net, torch.from_numpy(flags), guide, SCALE, clip_ratio=clip, init_adjs=torch.from_numpy(ia), init_nodes=torch.from_numpy(inn),
        churn_noise=(torch.from_numpy(na), torch.from_numpy(nn)), sanity_check_gt_adjs=torch.from_numpy(ga),
        sanity_check_gt_nodes=torch.from_numpy(gn), flag_interim_adjs=True, return_loss_trace=True)
    a, n, adjs_ls, nodes_ls, trace = _np((a, n, adjs_ls, nodes_ls, trace))
    assert adjs_ls.shape[0] == T8 + 1 and trace.shape == (T8, 3)
    nc = lib.sigma_schedule(smp._cfg())[2]
    ms = lib.multistep_coef(smp._cfg())
    n_clipped, last = _recompute_gt_run(solver, clip, list(range(T8)), nc, ms, (adjs_ls, nodes_ls), trace, gkw, flags, ia, inn, na, nn, ga, gn, smp)
    if clip is not None:
        assert n_clipped > 0, "the clip never engaged: the case does not test it"
    if solver == "dpmpp_2m":
        assert np.count_nonzero(ms) > 0
    # the last step runs to t = 0: the state is gt - f c_{T-1} g(gt)
    assert np.abs(n.astype(np.float64) - last["D_guided"]).max() <= STEP_RTOL * np.abs(gn).max()
    assert np.abs(a.astype(np.float64) - ga).max() <= STEP_RTOL * np.abs(ga).max()
    assert np.abs(last["shift"]).max() > 0


def test_walk_indexes_the_coefficient_by_schedule_index():
    """a guided RePaint walk in the sanity-check mode: the executed steps of dsg_walk_steps, each recomputed in float64 with the
    coefficient of ITS schedule index; one loss-trace row per executed step"""
    flags, ia, inn, na, nn, ga, gn = _gt_inputs(walk=True)
    net, smp = _net("tiny"), _sampler("tiny", "euler")
    guide, gkw = _guide(flags)
    sched, coef = lib.walk_steps(smp._cfg(), lib.make_walk_cfg(0, (2, 2), (2, 6)))
    assert len(sched) == 12 and len(set(sched.tolist())) == T8 and (np.diff(sched) < 0).any()
    a, n, adjs_ls, nodes_ls, trace = _np(smp.sample_guided(
        net, torch.from_numpy(flags), guide, SCALE, clip_ratio=None, resample=(2, 2), resample_range=(2, 6),
        init_adjs=torch.from_numpy(ia), init_nodes=torch.from_numpy(inn), churn_noise=(torch.from_numpy(na), torch.from_numpy(nn)),
        sanity_check_gt_adjs=torch.from_numpy(ga), sanity_check_gt_nodes=torch.from_numpy(gn), flag_interim_adjs=True, return_loss_trace=True))
    assert trace.shape == (12, 3) and adjs_ls.shape[0] == 13
    _recompute_gt_run("euler", None, sched.tolist(), coef, np.zeros(12), (adjs_ls, nodes_ls), trace, gkw, flags, ia, inn, na, nn, ga, gn, smp)
    cw = lib.guide_coef(smp._cfg(), SCALE.astype(np.float32))
    k = int(np.argmax(np.diff(sched) < 0)) + 1     # the first executed step behind a jump: its schedule index is not its position
    assert sched[k] != k and abs(cw[sched[k]] - cw[k]) > 1e-3 * abs(cw[k])
    assert np.array_equal(trace, np.broadcast_to(trace[0], trace.shape))   # D = gt at every step: one loss per graph


# ---- 3. zero weights are the plain sampler ----
@pytest.mark.parametrize("solver", ["euler", "heun", "dpmpp_2m"])
def test_zero_weights_are_the_plain_sampler(solver):
    cfg = Y.CONFIGS["tiny"]()
    net, smp, fl = _net("tiny"), _sampler("tiny", solver), _flags("tiny")
    guide, _ = _guide(fl.numpy())
    coins = (np.random.default_rng(3).random(2 * T8) < 0.5).astype(np.uint8)
    rng = np.random.default_rng(4)
    ka = torch.from_numpy(np.sign(rng.standard_normal((3, cfg.c_adj, 8, 8))).astype(np.float32))
    kn = torch.from_numpy((np.sign(rng.standard_normal((3, 8, cfg.c_node))) * 0.7).astype(np.float32))
    ma, mn = torch.from_numpy(rng.random(ka.shape) < 0.4), torch.from_numpy(rng.random(kn.shape) < 0.4)
    h = net.model._ensure_handle()
    old = h.get_option("loop_graph")
    guided = {}
    try:
        for loop_graph in (1, 0):
            h.set_option("loop_graph", loop_graph)
            kw = dict(seed=5, coins=coins, return_device=True)
            ref = _np(smp.sample(net, fl, num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj, **kw))
            got = _np(smp.sample_guided(net, fl, guide, 0.0, **kw))
            assert all(np.array_equal(g, r) for g, r in zip(got, ref)), f"scale = 0 against sample(), loop_graph {loop_graph}"
            refk = _np(smp.sample_known(net, fl, ka, kn, ma, mn, num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj, **kw))
            gotk = _np(smp.sample_guided(net, fl, guide, 0.0, known=(ka, kn, ma, mn), **kw))
            assert all(np.array_equal(g, r) for g, r in zip(gotk, refk)), f"scale = 0 against sample_known(), loop_graph {loop_graph}"
            assert not np.array_equal(ref[1], refk[1])
            guided[loop_graph] = _np(smp.sample_guided(net, fl, guide, SCALE, known=(ka, kn, ma, mn), clip_ratio=0.5, **kw))
            assert not np.array_equal(guided[loop_graph][1], refk[1])
    finally:
        h.set_option("loop_graph", old)
    # guided bodies replayed against guided bodies enqueued
    assert all(np.array_equal(g, r) for g, r in zip(guided[1], guided[0])), "replayed and enqueued guided bodies differ"


# ---- 4. against the eager loop, where the network's Jacobian is exactly zero ----
@pytest.mark.parametrize("solver", ["euler", "heun"])
def test_against_the_eager_loop_with_zero_jacobian(solver):
    from diffusesg_amd.guide import BoxGuide, guided_sample
    cfg = Y.CONFIGS["tiny"]()
    net, smp, fl = _net("tiny", True), _sampler("tiny", solver), _flags("tiny")
    guide = BoxGuide(overlap=1.0)
    np.random.seed(21)
    got = _np(smp.sample_guided(net, fl, guide, SCALE, clip_ratio=1.0, seed=9, return_device=True))
    np.random.seed(21)
    ref = _np(guided_sample(net, smp, fl, guide.torch_loss(fl), SCALE, clip_ratio=1.0, seed=9))
    np.random.seed(21)
    plain = _np(smp.sample(net, fl, seed=9, num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj, return_device=True))
    torch.cuda.synchronize()
    for what, g, r, p in zip(("adj", "node"), got, ref, plain):
        s = float(np.abs(r).max())
        err, moved = float(np.abs(g - r).max()) / s, float(np.abs(g - p).max()) / s
        print(f"BOXGUIDE eager {solver} {what}: |in-loop - eager| {err:.3e}, |guided - unguided| {moved:.3e} of the result's scale")
        assert g.shape == r.shape and err <= TRAJ_RTOL, (what, err)
        if what == "node":
            assert moved > 100 * TRAJ_RTOL, "the guidance moves nothing: the case tests nothing"


# ---- 5. with the real synthetic network ----
def test_real_network_chain_recomputed_in_float64():
    cfg = Y.CONFIGS["tiny"]()
    net, smp, fl = _net("tiny"), _sampler("tiny", "euler", churn=0), _flags("tiny")
    flags = fl.numpy()
    guide, gkw = _guide(flags)
    coins = np.zeros(T8, np.uint8)
    a, n, adjs_ls, nodes_ls, trace = _np(smp.sample_guided(net, fl, guide, SCALE, clip_ratio=0.5, seed=13, coins=coins, flag_interim_adjs=True,
                                                           return_loss_trace=True))
    sg, t_hat, _nc, h_step = lib.sigma_schedule(smp._cfg())
    cw = lib.guide_coef(smp._cfg(), SCALE.astype(np.float32))
    m = net.model
    hd = m._ensure_handle()
    fl8 = fl.to(torch.uint8).cuda()
    B = 3
    sc = (None, None)
    p = lambda v: None if v is None else v.data_ptr()
    bL = None
    for i in range(T8):
        x = (adjs_ls[i] * np.float32(sg[0]), nodes_ls[i] * np.float32(sg[0])) if i == 0 else (adjs_ls[i], nodes_ls[i])
        xa, xn = dev(x[0]), dev(x[1])
        sig = torch.full((B,), float(t_hat[i]), dtype=torch.float32, device="cuda")
        Da, Dn = torch.empty_like(xa), torch.empty_like(xn)
        hd.check(hd.L.dsg_precond(hd.raw, B, p(xa), p(xn), p(fl8), p(sig), p(sc[0]), p(sc[1]), 0, p(Da), p(Dn),
                                  torch.cuda.current_stream().cuda_stream), "dsg_precond")
        torch.cuda.synchronize()
        sc = (Da, Dn)                                      # the self-conditioning input of the next call is D, not D~
        D = (Da.cpu().numpy().astype(np.float64), Dn.cpu().numpy().astype(np.float64))
        r = BR.guided_call(x, D, flags, cw[i], 0.5, **gkw)
        ref = GR.euler_update(x, (D[0], r["D_guided"]), float(t_hat[i]), float(h_step[i]), flags)
        got = (adjs_ls[i + 1], nodes_ls[i + 1])
        for j, what in enumerate(("adj", "node")):
            err = float(np.abs(got[j].astype(np.float64) - ref[j]).max()) / max(float(np.abs(x[j]).max()), 1e-30)
            print(f"BOXGUIDE chain step {i} {what}: {err:.3e}")
            assert err <= TRAJ_RTOL, (i, what, err)
        # bar 1 of the kernel test, on this D
        bL, _bg, _dL, _dg = kernel_bars(D[1].astype(np.float32), flags.astype(np.uint8), gkw["sel"], gkw["region"],
                                        {k: v for k, v in gkw.items() if k not in ("sel", "region")})
        errL = float(np.abs(trace[i].astype(np.float64) - r["loss"]).max())
        print(f"BOXGUIDE chain step {i} loss trace: err {errL:.3e} bar {bL:.3e}")
        assert errL <= bL, (i, errL, bL)


# ---- 6. invariants ----
def test_known_entries_exact_and_padded_entries_zero():
    cfg = Y.CONFIGS["tiny"]()
    net, fl = _net("tiny"), _flags("tiny")
    flags = fl.numpy()
    guide, _ = _guide(flags)
    rng = np.random.default_rng(4)
    ka = np.sign(rng.standard_normal((3, cfg.c_adj, 8, 8))).astype(np.float32)
    kn = (np.sign(rng.standard_normal((3, 8, cfg.c_node))) * 0.7).astype(np.float32)
    ma, mn = rng.random(ka.shape) < 0.4, rng.random(kn.shape) < 0.4
    known = tuple(torch.from_numpy(v) for v in (ka, kn, ma, mn))
    va, vn = np.broadcast_to(flags[:, None, :, None] & flags[:, None, None, :], ka.shape), np.broadcast_to(flags[:, :, None], kn.shape)
    assert (mn & vn)[..., -4:].any() and (~mn & vn)[..., -4:].any()
    for solver in ("euler", "heun", "dpmpp_2m"):
        smp = _sampler("tiny", solver)
        coins = (np.random.default_rng(6).random(2 * T8) < 0.5).astype(np.uint8)
        kw = dict(seed=7, coins=coins, flag_interim_adjs=True)
        ga, gn, gal, gnl = _np(smp.sample_guided(net, fl, guide, SCALE, known=known, clip_ratio=0.5, **kw))
        pa, pn, pal, pnl = _np(smp.sample_known(net, fl, *known, num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj, **kw))
        # a known entry's trajectory is a function of its own noise and the known value: the guided run's equals the unguided run's
        # at EVERY step exactly when every guided estimate carried the known value bit for bit
        assert np.array_equal(gal[:, ma & va], pal[:, ma & va]) and np.array_equal(gnl[:, mn & vn], pnl[:, mn & vn]), solver
        assert np.abs(gn[mn & vn] - kn[mn & vn]).max() <= 1e-5 and np.abs(ga[ma & va] - ka[ma & va]).max() <= 1e-5
        assert not np.array_equal(gn[~mn & vn], pn[~mn & vn])
        assert (gal[:, ~va] == 0).all() and (gnl[:, ~vn] == 0).all() and (ga[~va] == 0).all() and (gn[~vn] == 0).all()


def test_small_runs_and_nosc_is_refused():
    from diffusesg_amd.guide import BoxGuide
    net, smp = _net("small"), _sampler("small", "heun")
    fl = _flags("small", [16, 9, 2])
    guide, _ = _guide(fl.numpy())
    coins = np.zeros(2 * T8, np.uint8)
    g = _np(smp.sample_guided(net, fl, guide, SCALE, seed=3, coins=coins))
    u = _np(smp.sample_guided(net, fl, guide, 0.0, seed=3, coins=coins))
    assert all(np.isfinite(v).all() for v in g) and g[1].shape == (3, 16, 5)
    assert not np.array_equal(g[1][..., -4:], u[1][..., -4:]) and (g[1][~fl.numpy()] == 0).all()
    # C_node = 1: no box channels.  DsgError before anything is launched: the run's counters stay where the last run left them
    net1, smp1, fl1 = _net("nosc"), _sampler("nosc", "euler"), _flags("nosc")
    smp1.sample(net1, fl1, seed=1, num_node_chan=1, num_edge_chan=1)
    before = dict(smp1.last_stats)
    with pytest.raises(lib.DsgError, match="C_node"):
        smp1.sample_guided(net1, fl1, BoxGuide(overlap=1.0), 1.0, seed=1)
    assert smp1.last_stats == before


def test_batch_invariant_graphs_alone_equal_the_batch():
    net, fl = _net("tiny"), _flags("tiny")
    flags = fl.numpy()
    guide, gkw = _guide(flags)
    from diffusesg_amd.guide import BoxGuide
    seeds = [2 ** 64 - 1, 2 ** 32 + 5, 1]
    h = net.model._ensure_handle()
    old = h.get_option("batch_invariant")
    h.set_option("batch_invariant", 1)
    try:
        for solver in ("heun", "dpmpp_2m"):
            smp = _sampler("tiny", solver)
            batch = _np(smp.sample_guided(net, fl, guide, SCALE, clip_ratio=0.5, graph_seeds=seeds, coin_seed=3))
            for b in range(3):
                one_guide = BoxGuide(overlap=1.0, align=0.5, tau=0.05, region_weight=0.8,
                                     region=(torch.from_numpy(gkw["sel"][b:b + 1]), torch.from_numpy(gkw["region"][b:b + 1].astype(np.float32))))
                one = _np(smp.sample_guided(net, fl[b:b + 1], one_guide, SCALE, clip_ratio=0.5, graph_seeds=seeds[b:b + 1], coin_seed=3))
                assert all(np.array_equal(batch[k][b:b + 1], one[k]) for k in range(2)), (solver, b)
    finally:
        h.set_option("batch_invariant", old)


def test_layout_from_graph_passes_the_guide():
    """complete.layout_from_graph with guide= / guide_scale=: scale 0 is the unguided layout bit for bit, a guide moves the boxes and
    leaves the given labels and relations alone"""
    from diffusesg_amd.complete import layout_from_graph
    from diffusesg_amd.guide import BoxGuide
    cfg = Y.CONFIGS["tiny"]()   # 6 adjacency bits, 8 label bits + 4 box channels
    n_adj_type, n_node_type, n = 51, 150, cfg.max_node_num
    flags = W.synth_flags(3, n, VALID)
    f = flags.astype(np.int32)
    rng = np.random.default_rng(12)
    q_adj = rng.integers(0, n_adj_type, (3, n, n)).astype(np.int32) * f[:, :, None] * f[:, None, :]
    q_adj[:, np.arange(n), np.arange(n)] = 0
    q_node = rng.integers(0, n_node_type, (3, n)).astype(np.int32) * f
    net, smp = _net("tiny"), _sampler("tiny", "heun")
    t = lambda a: torch.from_numpy(a).cuda()
    guide = BoxGuide(overlap=1.0, region=([0, 1], (0.1, 0.1, 0.6, 0.6)), align=0.5)
    out = {}
    for key, kw in (("plain", {}), ("zero", dict(guide=guide, guide_scale=0.0)), ("guided", dict(guide=guide, guide_scale=SCALE))):
        np.random.seed(6)
        out[key] = _np(layout_from_graph(net, smp, t(q_adj), t(q_node), t(flags), n_adj_type, n_node_type, seed=22, **kw))
    assert all(np.array_equal(a, b) for a, b in zip(out["zero"], out["plain"]))
    off = flags[:, :, None] & flags[:, None, :] & ~np.eye(n, dtype=bool)[None]
    qa, qn, bb = out["guided"]
    assert np.array_equal(qn[flags], q_node[flags]) and np.array_equal(qa[off], q_adj[off])
    assert np.isfinite(bb).all() and np.abs(bb[flags] - out["plain"][2][flags]).max() > 1e-3
