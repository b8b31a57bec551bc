"""GPU: autoguidance (dsg_attach_guide) -- a second, weaker network inside every preconditioned call,
D~ = fadd(D_m, fmul(s_b - 1, fsub(D_m, D_g))).  Tiny shapes (N = 8, B in {1, 2, 3}); the pairs of diffusesg_amd/synth.py: a -- the same
geometry, b -- a narrower guide (E = 64), c -- a patch_size 2 guide; reference values from tests/golden/autoguide.npz
(tools/gen_autoguide_golden.py: the reference's own modules and sampler around a two-network wrapper).  Every test attaches a guide."""
import ctypes as C

import numpy as np
import pytest
import torch

from diffusesg_amd import autoguide as AG
from diffusesg_amd import lib as L
from diffusesg_amd import spec as S
from diffusesg_amd import synth as Y
from diffusesg_amd import weights as W
from util import FWD_RTOL, assert_close, load

pytestmark = pytest.mark.gpu

CFG = S.tiny_config()
SA, SN = (3, CFG.c_adj, 8, 8), (3, 8, CFG.c_node)
PATTERNS = ((2, 0), (3, 0), (4, 1), (4, 2))   # tests/test_workspace_poison.py: (pattern, seed) compared against pattern 1
_nets = {}


def build(cfg, seed):
    from diffusesg_amd.model import build_network
    return build_network(cfg, W.synth_state_dict(cfg, seed), device="cuda")


def net(name):
    """main: the tiny config, weight seed 0; twin: the same again; a / b / c: the pairs' guides, weight seed 1"""
    if name not in _nets:
        _nets[name] = build(CFG, Y.AUTOGUIDE_MAIN_SEED) if name in ("main", "twin") else build(Y.autoguide_guide_config(name), Y.AUTOGUIDE_GUIDE_SEED)
    return _nets[name]


@pytest.fixture(autouse=True)
def _detach_all():
    yield
    for n in _nets.values():
        n.detach_guide()
        h = n.model._ensure_handle()
        h.set_option("batch_invariant", 0)
        h.set_option("loop_graph", 1)


def T(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def precond(n, adj, node, flags, sig, sca, scn, coin, out=None):
    """dsg_precond with the coin given; out: pre-filled output tensors"""
    m = n.model
    h = m._ensure_handle()
    B, a, x, fl, sa, sx = m._canon(T(adj), T(node), T(flags), T(sca), T(scn))
    sg = T(np.asarray(sig, np.float32))
    oa, on = (torch.empty_like(a), torch.empty_like(x)) if out is None else out
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    h.check(h.L.dsg_precond(h.raw, B, p(a), p(x), p(fl), p(sg), p(sa), p(sx), int(coin), p(oa), p(on),
                            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "dsg_precond")
    torch.cuda.synchronize()
    return oa.cpu().numpy(), on.cpu().numpy()


def make_sampler(T_=8, solver="heun", S_churn=40.0, use_graph=True):
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    return NodeAdjEDMSamplerHip(num_steps=T_, solver=solver, S_churn=S_churn, dev="cuda", objective="edm", self_condition=True,
                                symmetric_noise=False, use_graph=use_graph)


RUNS = {"t8_heun": (8, "heun", 40.0), "t8_euler": (8, "euler", 0.0), "t8_2m": (8, "dpmpp_2m", 0.0)}


def run(n, tag="t8_heun", use_graph=True, rows=slice(None)):
    """the fixture's run `tag` (t8_2m: the Euler run's inputs under the multistep solver) -> adj, node, sampler, coins"""
    T_, solver, churn = RUNS[tag]
    flags, ia, inn, na, nn, cv = Y.autoguide_sampler_case("t8_euler" if tag == "t8_2m" else tag, T_, "euler" if tag == "t8_2m" else solver)
    smp = make_sampler(T_, solver, churn, use_graph)
    coins = (cv < 0.5).astype(np.uint8)
    oa, on = smp.sample(n, T(flags[rows]), init_adjs=T(ia[rows]), init_nodes=T(inn[rows]), churn_noise=(T(na[:, rows]), T(nn[:, rows])), coins=coins,
                        flag_node_multi_channel=True, flag_adj_multi_channel=True, num_node_chan=CFG.c_node, num_edge_chan=CFG.c_adj)
    return oa.numpy(), on.numpy(), smp, coins


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def pre_inputs(si):
    sigma, flags, adj, node, sca, scn = Y.autoguide_precond_case(si)
    return flags, adj, node, sca, scn, np.full((3,), sigma, np.float32)


# ---- 1. a guide with the main network's weights and geometry changes nothing, bit for bit ----
def test_same_weights_is_identity():
    main, twin = net("main"), net("twin")
    flags, adj, node, sca, scn, sig = pre_inputs(1)
    ref_pre = [precond(main, adj, node, flags, sig, sca, scn, c) for c in (0, 1)]
    ref_run = {tag: run(main, tag)[:2] for tag in RUNS}
    main.attach_guide(twin, scale=2.5)
    for c in (0, 1):
        assert same(precond(main, adj, node, flags, sig, sca, scn, c), ref_pre[c]), f"dsg_precond coin {c}"
    for tag in RUNS:
        oa, on, smp, _ = run(main, tag)
        assert same((oa, on), ref_run[tag]), tag
        assert smp.last_guide_forwards == smp.last_stats["net_forwards"] > 0


# ---- 2. scale 1, or an interval without a level: no guide forward, the plain bodies ----
@pytest.mark.parametrize("scale,rng", [(1.0, None), (2.0, (200.0, 300.0)), (2.0, (1e-6, 1e-5))])
def test_no_guided_step_runs_no_guide_forward(scale, rng, monkeypatch, capfd):
    import re
    monkeypatch.setenv("DSG_GRAPH_VERBOSE", "1")
    keys = []
    for attach in (False, True):
        main = build(CFG, 0)   # fresh handles: every body of the run is captured, and reported, now
        if attach:
            main.attach_guide(net("a"), scale=scale, sigma_range=rng)
            assert not AG.guided_steps(make_sampler()._cfg(), rng, scale).any()
        capfd.readouterr()
        oa, on, smp, _ = run(main, "t8_heun")
        keys.append(sorted(int(k) for k in re.findall(r"captured step body key=(\d+)", capfd.readouterr().err)))
        if attach:
            assert same((oa, on), ref) and smp.last_guide_forwards == 0
        ref = (oa, on)
        main.detach_guide()
    assert keys[0] == keys[1] and len(keys[0]) > 0


# ---- 3. one call is the float32 combine of two unattached calls, bit for bit ----
def combine(Dm, Dg, sig, scale, lo, hi):
    s32 = torch.tensor(scale, dtype=torch.float32) - torch.tensor(1.0, dtype=torch.float32)
    sg = torch.from_numpy(np.asarray(sig, np.float32))
    sm1 = torch.where((sg >= lo) & (sg <= hi), s32, torch.zeros(()))
    out = []
    for m, g in zip(Dm, Dg):
        m, g = torch.from_numpy(m), torch.from_numpy(g)
        k = sm1.view((-1,) + (1,) * (m.dim() - 1))
        out.append((m + k * (m - g)).numpy())
    return out


def one_call(pair, coin):
    main, guide = net("main"), net(pair)
    flags, adj, node, sca, scn, _ = pre_inputs(1)
    sig = np.array([80.0, 1.5, 0.002], np.float32)   # sample 1 inside [1, 10], samples 0 and 2 outside
    main.detach_guide()
    Dm, Dg = precond(main, adj, node, flags, sig, sca, scn, coin), precond(guide, adj, node, flags, sig, sca, scn, coin)
    main.attach_guide(guide, scale=2.0, sigma_range=(1.0, 10.0))
    got = precond(main, adj, node, flags, sig, sca, scn, coin)
    return got, Dm, Dg, sig, flags


@pytest.mark.parametrize("coin", [0, 1])
@pytest.mark.parametrize("pair", Y.AUTOGUIDE_PAIRS)
def test_one_call_is_the_combine(pair, coin):
    got, Dm, Dg, sig, flags = one_call(pair, coin)
    want = combine(Dm, Dg, sig, 2.0, 1.0, 10.0)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert not same(got, Dm) and np.array_equal(got[0][[0, 2]], Dm[0][[0, 2]]) and np.array_equal(got[1][[0, 2]], Dm[1][[0, 2]])
    assert not np.array_equal(got[0][1], Dm[0][1])
    f = flags.astype(bool)
    va = f[:, None, :, None] & f[:, None, None, :]
    assert np.all(got[0][~np.broadcast_to(va, got[0].shape)] == 0) and np.all(got[1][~f] == 0)


# ---- 4. the reference's composite: calls and trajectories of the fixture ----
def fixture_calls(pair):
    g, main = load("autoguide.npz"), net("main")
    main.attach_guide(net(pair), scale=float(g["scale"]))
    out = {}
    for si in range(3):
        flags, adj, node, sca, scn, sig = pre_inputs(si)
        for coin in (0, 1):
            out[f"{pair}_s{si}_coin{coin}"] = precond(main, adj, node, flags, sig, sca, scn, coin)
    return g, out


@pytest.mark.parametrize("pair", Y.AUTOGUIDE_PAIRS)
def test_composite_calls_vs_reference(pair):
    g, out = fixture_calls(pair)
    for key, (oa, on) in out.items():
        ea, en = assert_close(oa, g[key + "_adj"], FWD_RTOL, key + " adj"), assert_close(on, g[key + "_node"], FWD_RTOL, key + " node")
        print(f"AUTOGUIDE call {key}: rel err adj {ea:.3e} node {en:.3e} (bar {FWD_RTOL:.0e})")


@pytest.mark.parametrize("tag", ["t8_heun", "t8_euler"])
@pytest.mark.parametrize("pair", Y.AUTOGUIDE_PAIRS)
def test_trajectories_vs_reference(pair, tag):
    g, main = load("autoguide.npz"), net("main")
    main.attach_guide(net(pair), scale=float(g["scale"]))
    oa, on, smp, coins = run(main, tag)
    ea, en = assert_close(oa, g[f"{pair}_{tag}_adj"], 1e-4, f"{pair} {tag} adj"), assert_close(on, g[f"{pair}_{tag}_node"], 1e-4, f"{pair} {tag} node")
    print(f"AUTOGUIDE trajectory {pair} {tag}: rel err adj {ea:.3e} node {en:.3e} (bar 1e-04)")
    used = int(g[f"{pair}_{tag}_coins_used"])
    assert smp.last_stats["precond_calls"] == used
    assert smp.last_stats["net_forwards"] == used + int(coins[:used].sum()) == smp.last_guide_forwards
    assert smp.last_stats["graph_replays"] == smp.last_stats["net_forwards"]


# ---- 5. an interval of middle levels: the predicted forwards, the eager recomputation ----
@pytest.mark.parametrize("pair", ["a", "c"])
def test_interval_against_eager_float64(pair):
    main, guide, scale = net("main"), net(pair), 2.0
    smp0 = make_sampler(8, "euler", 0.0)
    _, t_hat, _, hs = L.sigma_schedule(smp0._cfg())
    rng = (float(t_hat[5]), float(t_hat[2]))   # schedule indices 2 .. 5, bounds included
    guided = AG.guided_steps(smp0._cfg(), rng, scale)
    assert list(np.nonzero(guided)[0]) == [2, 3, 4, 5]
    flags, ia, inn, _, _, cv = Y.autoguide_sampler_case("t8_euler", 8, "euler")
    coins = (cv < 0.5).astype(np.uint8)
    # eager: x <- x + h (x - D~) / t, D~ from unattached dsg_precond calls on both handles, the combine and the update in float64
    main.detach_guide()
    f = flags.astype(bool)
    ma, mn = (f[:, None, :, None] & f[:, None, None, :]).astype(np.float64), f[:, :, None].astype(np.float64)
    xa, xn = ia.astype(np.float64) * float(t_hat[0]) * ma, inn.astype(np.float64) * float(t_hat[0]) * mn
    sca = scn = None
    for i in range(8):
        t = float(t_hat[i])
        sig = np.full((3,), t_hat[i], np.float32)
        a32, n32 = xa.astype(np.float32), xn.astype(np.float32)
        Da, Dn = (d.astype(np.float64) for d in precond(main, a32, n32, flags, sig, sca, scn, coins[i]))
        if guided[i]:
            Ga, Gn = (d.astype(np.float64) for d in precond(guide, a32, n32, flags, sig, sca, scn, coins[i]))
            Da, Dn = Da + (scale - 1.0) * (Da - Ga), Dn + (scale - 1.0) * (Dn - Gn)
        xa, xn = (xa + float(hs[i]) * (xa - Da) / t) * ma, (xn + float(hs[i]) * (xn - Dn) / t) * mn
        sca, scn = Da.astype(np.float32), Dn.astype(np.float32)
    main.attach_guide(guide, scale=scale, sigma_range=rng)
    oa, on, smp, _ = run(main, "t8_euler")
    assert smp.last_guide_forwards == AG.expected_guide_forwards(smp0._cfg(), coins, rng, scale) == 4 + int(coins[2:6].sum())
    assert smp.last_stats["net_forwards"] == 8 + int(coins.sum())
    ea, en = assert_close(oa, xa, 1e-4, "interval adj"), assert_close(on, xn, 1e-4, "interval node")
    print(f"AUTOGUIDE interval {pair}: rel err against the eager float64 loop adj {ea:.3e} node {en:.3e} (bar 1e-04)")


# ---- 6. step graphs on / off, loop_graph = 0; detach restores the plain run ----
@pytest.mark.parametrize("tag", list(RUNS))
def test_step_graphs_on_off_and_detach(tag):
    main = net("main")
    plain = run(main, tag)[:2]
    main.attach_guide(net("b"), scale=2.0, sigma_range=(0.1, 30.0))
    oa, on, smp, _ = run(main, tag, use_graph=True)
    assert smp.last_stats["graph_replays"] == smp.last_stats["net_forwards"] and 0 < smp.last_guide_forwards < smp.last_stats["net_forwards"]
    assert not same((oa, on), plain)
    assert same(run(main, tag, use_graph=False)[:2], (oa, on)), "step graphs off"
    main.model._ensure_handle().set_option("loop_graph", 0)
    assert same(run(main, tag, use_graph=True)[:2], (oa, on)), "loop_graph = 0"
    main.model._ensure_handle().set_option("loop_graph", 1)
    assert same(run(main, tag, use_graph=True)[:2], (oa, on)), "captured again"
    main.detach_guide()
    assert same(run(main, tag)[:2], plain), "after detach"
    assert main.guide_info() is None and main.model._ensure_handle().guide_info()[0] is None


# ---- 7. composition with the other sampler features ----
def _known():
    ka, kn = Y.gt_case(CFG, 3, Y.AUTOGUIDE_VALID)
    ma = (W.uniform01(3, "autoguide/mask/adj", int(np.prod(SA))) < 0.5).astype(np.uint8).reshape(SA)
    mn = (W.uniform01(3, "autoguide/mask/node", int(np.prod(SN))) < 0.5).astype(np.uint8).reshape(SN)
    return ka, kn, ma, mn


@pytest.mark.parametrize("resample", [None, (2, 2)])
def test_known_entries_hold_and_walk_runs(resample):
    main = net("main")
    main.attach_guide(net("c"), scale=2.0)
    flags, ia, inn, _, _, _ = Y.autoguide_sampler_case("t8_heun", 8, "heun")
    ka, kn, ma, mn = _known()
    smp = make_sampler(8, "heun", 40.0)
    oa, on = smp.sample_known(main, T(flags), T(ka), T(kn), T(ma), T(mn), init_adjs=T(ia), init_nodes=T(inn), seed=11, resample=resample,
                              num_node_chan=CFG.c_node, num_edge_chan=CFG.c_adj, return_device=True)
    f = T(flags).bool()
    va, vn = (f[:, None, :, None] & f[:, None, None, :]).expand(SA), f[:, :, None].expand(SN)
    held_a, held_n = T(ma).bool() & va, T(mn).bool() & vn
    assert held_a.any() and held_n.any()
    if resample is None:
        assert torch.equal(oa[held_a], T(ka)[held_a]) and torch.equal(on[held_n], T(kn)[held_n])
    else:   # a resampled walk diffuses the state back up: known entries land as test_resample.py holds them, unattached, to 1e-6
        assert (oa - T(ka))[held_a].abs().max() < 1e-6 and (on - T(kn))[held_n].abs().max() < 1e-6
    assert torch.all(oa[~va] == 0) and torch.all(on[~vn] == 0) and torch.isfinite(oa).all() and torch.isfinite(on).all()
    assert smp.last_guide_forwards == smp.last_stats["net_forwards"] >= (15 if resample is None else 16)


def test_graph_alone_equals_graph_in_batch():
    main, guide = net("main"), net("a")
    for n in (main, guide):
        n.model._ensure_handle().set_option("batch_invariant", 1)
    main.attach_guide(guide, scale=2.0)
    flags = W.synth_flags(3, 8, Y.AUTOGUIDE_VALID)
    seeds = [17, 2 ** 40 + 3, 5]
    smp = make_sampler(8, "heun", 40.0)
    kw = dict(coin_seed=7, flag_node_multi_channel=True, flag_adj_multi_channel=True, num_node_chan=CFG.c_node, num_edge_chan=CFG.c_adj)
    full = smp.sample(main, T(flags), graph_seeds=seeds, **kw)
    assert smp.last_guide_forwards > 0
    for b in range(3):
        alone = smp.sample(main, T(flags[b:b + 1]), graph_seeds=seeds[b:b + 1], **kw)
        assert torch.equal(alone[0][0], full[0][b]) and torch.equal(alone[1][0], full[1][b]), b


def test_content_guided_run_with_equal_weights_is_unchanged():
    from diffusesg_amd import guide as G
    main = net("main")
    flags = W.synth_flags(3, 8, Y.AUTOGUIDE_VALID)
    cg = G.ContentGuide([[(3, 5, 7)], [(1, None, None)], [(None, 2, None), (4, 1, 9)]], 150, 51, weight=0.7, tau=0.5, clip_ratio=0.3)
    smp = make_sampler(8, "heun", 40.0)
    kw = dict(content=cg, seed=9, coin_seed=None)
    np.random.seed(5)
    ref = smp.sample_guided(main, T(flags), G.BoxGuide(), 2.0, **kw)
    main.attach_guide(net("twin"), scale=2.5)
    np.random.seed(5)
    got = smp.sample_guided(main, T(flags), G.BoxGuide(), 2.0, **kw)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]) and smp.last_guide_forwards > 0


# ---- 8. refusals ----
def _variant(**kw):
    base = dict(max_node_num=8, c_adj=6, c_node=12, depths=(1, 1), num_heads=(3, 6), window_size=4, self_condition=True)
    base.update(kw)
    cfg = S.ModelConfig(**base)
    n = build(cfg, 1)
    n.model._ensure_handle()
    return n


def test_refusals_name_the_argument_and_enqueue_nothing(monkeypatch):
    main, guide = net("main"), net("a")
    h, g = main.model._ensure_handle(), guide.model._ensure_handle()
    keep = []

    def refused(gh, scale, lo, hi, word):
        with pytest.raises(L.DsgError) as e:
            h.attach_guide(gh, scale, lo, hi)
        assert f"status {L.DSG_ERR_INVALID}:" in str(e.value) and word in str(e.value), (word, str(e.value))
        assert h.guide_info() == (None, 1.0, 0.0, 0.0)
    inf = float("inf")
    refused(h, 2.0, -inf, inf, "guide == h")
    third = build(CFG, 2)
    g.attach_guide(third.model._ensure_handle(), 2.0, -inf, inf)
    refused(g, 2.0, -inf, inf, "guide has a guide")
    g.detach_guide()
    raw = L.Handle(CFG)
    refused(raw, 2.0, -inf, inf, "not finalized")
    for field, kw in (("max_node_num", dict(max_node_num=16)), ("c_adj", dict(c_adj=5)), ("c_node", dict(c_node=11)),
                      ("self_condition", dict(self_condition=False))):
        v = _variant(**kw)
        keep.append(v)
        refused(v.model._ensure_handle(), 2.0, -inf, inf, field)
    if torch.cuda.device_count() > 1:
        with torch.cuda.device(1):
            other = L.Handle(CFG)
        refused(other, 2.0, -inf, inf, "device")
    refused(g, inf, -inf, inf, "scale")
    refused(g, float("nan"), -inf, inf, "scale")
    refused(g, 2.0, 3.0, 2.0, "sigma_lo")
    refused(g, 2.0, float("nan"), 2.0, "sigma_lo")
    refused(g, 2.0, 1.0, float("nan"), "sigma_hi")
    # the Python layer refuses the same before it reaches the library
    for bad in (dict(scale=inf), dict(sigma_range=(3.0, 2.0)), dict(sigma_range=(float("nan"), 1.0))):
        with pytest.raises(ValueError):
            main.attach_guide(guide, **bad)
    with pytest.raises(ValueError, match="c_adj"):
        main.attach_guide(keep[1])
    assert main.guide_info() is None
    # an entry call whose option combination the guide cannot run (a p = 2 guide created under a precision mode's environment default):
    # the guide's own message, prefixed, before anything is enqueued -- the outputs stay as they were
    monkeypatch.setenv("DSG_GEMM_BF16", "1")
    p2 = build(Y.autoguide_guide_config("c"), 1)
    p2h = p2.model._ensure_handle()
    monkeypatch.delenv("DSG_GEMM_BF16")
    assert p2h.get_option("gemm_bf16") == 1
    main.attach_guide(p2, scale=2.0)
    flags, adj, node, sca, scn, sig = pre_inputs(1)
    out = (torch.full(SA, 7.5, device="cuda"), torch.full(SN, 7.5, device="cuda"))
    with pytest.raises(L.DsgError, match="guide handle: ") as e:
        precond(main, adj, node, flags, sig, sca, scn, 0, out=out)
    assert f"status {L.DSG_ERR_INVALID}:" in str(e.value) and "gemm_bf16" in str(e.value) and "patch_size" in str(e.value)
    torch.cuda.synchronize()
    assert torch.all(out[0] == 7.5) and torch.all(out[1] == 7.5)
    with pytest.raises(L.DsgError, match="guide handle: "):
        run(main, "t8_euler")
    main.detach_guide()
    assert same(precond(main, adj, node, flags, sig, sca, scn, 0), precond(net("twin"), adj, node, flags, sig, sca, scn, 0))


# ---- 9. stale memory in both workspaces ----
@pytest.mark.parametrize("pair", ["a", "c"])
def test_outputs_do_not_depend_on_stale_memory(pair):
    main, guide = net("main"), net(pair)
    h, g = main.model._ensure_handle(), guide.model._ensure_handle()

    def both():
        got = one_call(pair, 1)[0]
        main.attach_guide(guide, scale=2.0)
        flags, adj, node, sca, scn, sig = pre_inputs(0)
        return got + precond(main, adj, node, flags, sig, sca, scn, 1) + run(main, "t8_heun")[:2]
    both()   # every workspace and table exists
    for hh in (h, g):
        hh.poison(3, 1)
    ref = both()
    for pattern, seed in PATTERNS:
        for hh in (h, g):
            hh.poison(3, pattern, seed)
        got = both()
        for k, (x, y) in enumerate(zip(got, ref)):
            assert np.array_equal(x, y), f"output {k} after pattern {pattern} (seed {seed})"
