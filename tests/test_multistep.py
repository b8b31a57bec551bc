"""GPU: the second-order multistep solver, solver='dpmpp_2m' (DSG_SOLVER_DPMPP_2M, include/dsg.h): DPM-Solver++ 2M in EDM variables,
one network forward per step.

The reference has no such solver, so -- like tests/test_resample.py -- it is pinned to paths that are pinned: where its coefficient is 0
the step must BE the Euler step (same kernel, same captured body, same bits); a real run is compared with the same loop re-enacted in
torch float32 around single NodeAdjPrecondHip calls, iterating lib.walk_steps / lib.sigma_schedule / lib.multistep_coef, at the
project's trajectory bar util.FWD_RTOL; and its order is measured against solver='euler' at T = 2048 on the same device.
Shapes: tiny (B = 4, T = 8, recorded coins), nosc (B = 4, T = 6, no self-conditioning), small (B = 3, valid [16, 9, 4], T = 6),
vg (B = 2, valid [30, 11], T = 2..4).  S_churn = 0 throughout: the solver refuses churn."""
import ctypes as C

import numpy as np
import pytest
import torch

from diffusesg_amd import lib
from diffusesg_amd import synth as Y
from diffusesg_amd import weights as W
from util import FWD_RTOL, assert_close, rel_err

pytestmark = pytest.mark.gpu

VALID4 = [8, 5, 3, 8]
_nets = {}


def net_for(name):
    from diffusesg_amd.model import build_network
    if name not in _nets:
        cfg = Y.CONFIGS[name]()
        _nets[name] = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")
    return _nets[name]


def T(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def make_sampler(T_, solver="dpmpp_2m", S_churn=0.0, use_graph=True, self_condition=True):
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    return NodeAdjEDMSamplerHip(num_steps=T_, solver=solver, S_churn=S_churn, dev="cuda", objective="edm",
                                self_condition=self_condition, symmetric_noise=False, use_graph=use_graph)


class Case:
    """Recorded inputs: Y.sampler_case(cfg, Lmax, B, valid, 3, "dpm/<name>", "euler") -- the initial sample does not depend on Lmax; Lmax
    noise slices (read only by the jump-back draws of a walk) and Lmax coins -- and the +-1 known values of Y.gt_case."""

    def __init__(self, name, B, valid, T_, Lmax=None, tag=None, net=None):
        self.name, self.B, self.T = name, B, T_
        self.net = net if net is not None else net_for(name)
        self.cfg = cfg = Y.CONFIGS[name]()
        flags, ia, inn, na, nn, cv = Y.sampler_case(cfg, Lmax or T_, B, valid, 3, tag or f"dpm/{name}", "euler")
        self.coins = (cv < 0.5).astype(np.uint8)
        ka, kn = Y.gt_case(cfg, B, valid)
        self.flags, self.ia, self.inn, self.na, self.nn, self.ka, self.kn = T(flags), T(ia), T(inn), T(na), T(nn), T(ka), T(kn)
        n = cfg.max_node_num
        self.sa, self.sn = (B, cfg.c_adj, n, n), (B, n, cfg.c_node)
        f = self.flags.bool()
        self.va = (f[:, None, :, None] & f[:, None, None, :]).expand(self.sa)   # valid entries
        self.vn = f[:, :, None].expand(self.sn)

    def scfg(self, solver="dpmpp_2m", T_=None):
        return lib.make_sampler_cfg(T_ or self.T, solver, 0.0, 0.05, 50.0, 1.003, 0.002, 80.0, 7.0, False)

    def wcfg(self, **walk):
        return lib.make_walk_cfg(walk.get("start_step", 0), walk.get("resample"), walk.get("resample_range"))

    def steps(self, **walk):
        return lib.walk_steps(self.scfg(), self.wcfg(**walk))

    def sampler(self, solver="dpmpp_2m", use_graph=True, T_=None, S_churn=0.0):
        return make_sampler(T_ or self.T, solver, S_churn, use_graph, self.cfg.self_condition)

    def kw(self, L=None, coins=None, init=True, seed=11):
        d = dict(coins=self.coins if coins is None else coins, num_node_chan=self.cfg.c_node, num_edge_chan=self.cfg.c_adj,
                 return_device=True)
        if init:
            d.update(init_adjs=self.ia, init_nodes=self.inn)
        else:
            d.update(seed=seed)
        if L is not None:   # a walk: its jump-back draws read recorded slices
            d.update(churn_noise=(self.na[:L], self.nn[:L]))
        return d

    def full(self, t_adj, t_node):
        return t_adj.reshape(self.sa), t_node.reshape(self.sn)

    def run(self, solver="dpmpp_2m", use_graph=True, T_=None, S_churn=0.0, **kw):
        smp = self.sampler(solver, use_graph, T_, S_churn)
        oa, on = smp.sample(self.net, self.flags, **(kw or self.kw()))
        return oa.reshape(self.sa).clone(), on.reshape(self.sn).clone(), dict(smp.last_stats)

    def cond(self, ma, mn, solver="dpmpp_2m", use_graph=True, kw=None, **walk):
        smp = self.sampler(solver, use_graph)
        L = len(self.steps(**walk)[0]) if walk else None
        oa, on = smp.sample_known(self.net, self.flags, self.ka, self.kn, ma, mn, **(kw or self.kw(L)), **walk)
        return oa.reshape(self.sa).clone(), on.reshape(self.sn).clone(), dict(smp.last_stats)

    def masks(self, fill):
        return (torch.full(self.sa, fill, dtype=torch.uint8, device="cuda"), torch.full(self.sn, fill, dtype=torch.uint8, device="cuda"))

    def random_masks(self, tag="dpm/mask"):
        na, nn = int(np.prod(self.sa)), int(np.prod(self.sn))
        return (T((W.uniform01(3, f"{tag}/{self.name}/adj", na) < 0.5).astype(np.uint8).reshape(self.sa)),
                T((W.uniform01(3, f"{tag}/{self.name}/node", nn) < 0.5).astype(np.uint8).reshape(self.sn)))


_cases = {}


def case(name):
    if name not in _cases:
        if name == "tiny":
            c = Case("tiny", 4, VALID4, 8, 24)
            assert 0 < int(c.coins[:8].sum()) < 8, "the recorded coins must fire for some calls and not for others"
        elif name == "nosc":
            c = Case("nosc", 4, VALID4, 6)
        elif name == "small":
            c = Case("small", 3, [16, 9, 4], 6)
        else:
            c = Case("vg", 2, [30, 11], 4)
        c.ma, c.mn = c.random_masks()
        _cases[name] = c
    return _cases[name]


def same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 1. steps with coefficient 0 are Euler's ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("name", ["tiny", "nosc"])
def test_euler_steps_are_eulers(name, use_graph, monkeypatch, capfd):
    """T = 1 (the step to t = 0) and T = 2 (first step + the step to t = 0): every coefficient is 0, the run is solver='euler' bit for
    bit with the same stats, and it replays Euler's captured step bodies: none is captured for it"""
    c = case(name)
    for T_, coins in ((1, np.array([1], np.uint8)), (2, np.array([1, 0], np.uint8)), (2, np.array([0, 1], np.uint8))):
        assert np.all(lib.multistep_coef(c.scfg(T_=T_)) == 0)
        e = c.run("euler", use_graph, T_, **c.kw(coins=coins))
        capfd.readouterr()
        monkeypatch.setenv("DSG_GRAPH_VERBOSE", "1")
        m = c.run("dpmpp_2m", use_graph, T_, **c.kw(coins=coins))
        torch.cuda.synchronize()
        monkeypatch.delenv("DSG_GRAPH_VERBOSE")
        err = capfd.readouterr().err
        assert same(m, e) and m[2] == e[2], (T_, coins)
        assert m[2]["precond_calls"] == T_ and m[2]["graph_replays"] == (m[2]["net_forwards"] if use_graph else 0)
        assert "captured step body" not in err, err


# ---- 2. composition ---------------------------------------------------------------------------------------------------------------------
def eager_2m(c, known=None, walk=None, base=None, init=None, coins=None):
    """The multistep loop re-enacted in torch float32 on the device: one row of lib.walk_steps / lib.multistep_coef per executed step,
    t_hat and h from lib.sigma_schedule, one NodeAdjPrecondHip call per network forward with its own coin pinned to 'not fired', the
    known-entry select (known = (mask_adj, mask_node)) in torch.  Returns the final state and the number of network forwards."""
    net, cfg, walk = c.net, c.cfg, walk or {}
    sg, t_hat, nz, hs = lib.sigma_schedule(c.scfg())
    assert np.all(nz == 0)
    sched, jump = c.steps(**walk)
    msc = lib.multistep_coef(c.scfg(), c.wcfg(**walk))
    fa, fn = c.va.float(), c.vn.float()
    coins = c.coins if coins is None else coins
    ia, inn = init or (c.ia, c.inn)

    def select(D):
        D = c.full(*D)
        if known is None:
            return D[0] * fa, D[1] * fn
        return torch.where(known[0].bool(), c.ka, D[0]) * fa, torch.where(known[1].bool(), c.kn, D[1]) * fn

    forwards = [0]

    def P(x, sigma, sc):
        real = np.random.rand
        np.random.rand = lambda: 0.9   # the call's own coin never fires
        forwards[0] += 1
        try:
            return net(x[0], x[1], c.flags, torch.full((c.B,), float(sigma), dtype=torch.float32, device="cuda"), sc[0], sc[1])
        finally:
            np.random.rand = real

    def denoise(x, sigma, sc, coin):
        if coin and cfg.self_condition:
            sc = select(P(x, sigma, sc))
        return select(P(x, sigma, sc))

    ts = float(np.float32(sg[walk.get("start_step", 0)]))
    x = (ia * ts, inn * ts) if base is None else ((base[0] + ia * ts) * fa, (base[1] + inn * ts) * fn)
    sc, D_prev = (None, None), None
    for k, (i, cf, ck) in enumerate(zip(sched.tolist(), jump.tolist(), msc.tolist())):
        th, h = float(t_hat[i]), float(hs[i])
        xh = x if cf == 0 else ((x[0] + cf * c.na[k]) * fa, (x[1] + cf * c.nn[k]) * fn)
        D = denoise(xh, th, sc, coins[k])
        Dt = D if ck == 0 else tuple(a + ck * (a - b) for a, b in zip(D, D_prev))
        x = tuple((a + h * ((a - b) / th)) * f for a, b, f in zip(xh, Dt, (fa, fn)))
        D_prev = D
        sc = D if cfg.self_condition else (None, None)
    return x, forwards[0]


def check_vs_eager(what, got, want):
    ea, en = rel_err(got[0].cpu().numpy(), want[0].cpu().numpy()), rel_err(got[1].cpu().numpy(), want[1].cpu().numpy())
    print(f"{what}: rel err vs the torch re-enactment adj {ea:.3e} node {en:.3e}")
    assert ea <= FWD_RTOL and en <= FWD_RTOL, f"{what}: rel err adj {ea:.3e} node {en:.3e} > {FWD_RTOL:.1e}"


@pytest.mark.parametrize("name", ["tiny", "nosc", "small"])
def test_run_vs_eager_composition(name):
    c = case(name)
    assert np.count_nonzero(lib.multistep_coef(c.scfg())) == c.T - 2
    got = c.run()
    want, forwards = eager_2m(c)
    check_vs_eager(f"{name} T = {c.T}", got, want)
    assert got[2]["precond_calls"] == c.T and got[2]["net_forwards"] == forwards
    e = c.run("euler")
    assert rel_err(got[0].cpu().numpy(), e[0].cpu().numpy()) > 10 * FWD_RTOL, "the second-order steps must differ from Euler's"


@pytest.mark.parametrize("walk", [dict(resample=(2, 3)), dict(start_step=3)], ids=["resample", "partial_start"])
def test_half_known_walk_vs_eager_composition(walk):
    c = case("tiny")
    kw = dict(walk)
    if "start_step" in walk:
        kw.update(base_adjs=c.ka, base_nodes=c.kn)
    got = c.cond(c.ma, c.mn, **kw)
    want, forwards = eager_2m(c, (c.ma, c.mn), walk, base=(c.ka, c.kn) if "start_step" in walk else None)
    check_vs_eager(f"tiny half-known {sorted(walk)}", got, want)
    L = len(c.steps(**walk)[0])
    assert L == (24 if "resample" in walk else 5)
    assert got[2]["precond_calls"] == L and got[2]["net_forwards"] == forwards == L + int(c.coins[:L].sum())
    ka_, kn_ = c.ma.bool() & c.va, c.mn.bool() & c.vn
    assert (got[0] - c.ka)[ka_].abs().max() < 1e-6 and (got[1] - c.kn)[kn_].abs().max() < 1e-6


# ---- 3. bitwise equivalences --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "nosc"])
def test_graph_equals_eager_equals_forward_graph(name):
    c = case(name)
    walk = dict(resample=(2, 3)) if name == "tiny" else {}
    runs = lambda use_graph: (c.run(use_graph=use_graph), c.cond(c.ma, c.mn, use_graph=use_graph, **walk))
    g = runs(True)                                    # step graphs
    e = runs(False)                                   # every kernel launched eagerly
    for a, b in zip(g, e):
        assert same(a, b)
        assert a[2]["graph_replays"] == a[2]["net_forwards"] == b[2]["net_forwards"] and b[2]["graph_replays"] == 0
    h = c.net.model._ensure_handle()
    assert h.get_option("loop_graph") == 1
    h.set_option("loop_graph", 0)
    try:
        f = runs(True)                                # only the network forward is a graph
    finally:
        h.set_option("loop_graph", 1)
    for a, b in zip(f, e):
        assert same(a, b) and a[2]["graph_replays"] == a[2]["net_forwards"] == b[2]["net_forwards"]
    for a, b in zip(runs(True), e):                   # step bodies captured afresh after the option change
        assert same(a, b)


@pytest.mark.parametrize("name", ["tiny", "nosc"])
def test_device_drawn_init_equals_init_handed_in(name):
    c = case(name)
    smp, seed = c.sampler(), 23
    drawn = c.run(**c.kw(init=False, seed=seed))
    ia, inn = smp.device_noise(c.net, c.flags, stream=0, seed=seed)
    kw = c.kw()
    kw.update(init_adjs=ia, init_nodes=inn)
    given = c.run(**kw)
    assert same(drawn, given) and drawn[2] == given[2]
    assert not same(drawn, c.run())


def test_euler_and_heun_unchanged_by_multistep_runs():
    """one fresh handle: solver='euler' and solver='heun' (with churn) calls, multistep runs of every kind (plain, conditioned along a
    walk, eager), then the same calls again: same bits, same stats"""
    from diffusesg_amd.model import build_network
    cfg = Y.CONFIGS["tiny"]()
    net = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")
    c = Case("tiny", 4, VALID4, 8, 24, net=net)
    hc = (W.coins(3, "dpm/heun", 15) < 0.5).astype(np.uint8)
    hkw = dict(c.kw(8, coins=hc))

    def plain():
        return c.run("euler"), c.run("heun", S_churn=40.0, **hkw), c.cond(c.ma_, c.mn_, "euler", resample=(2, 3))

    c.ma_, c.mn_ = c.random_masks()
    before = plain()
    m0 = c.run()
    c.cond(c.ma_, c.mn_, resample=(2, 3))
    c.cond(c.ma_, c.mn_, use_graph=False, start_step=3, base_adjs=c.ka, base_nodes=c.kn)
    after = plain()
    for a, b in zip(before, after):
        assert same(a, b) and a[2] == b[2]
    assert same(c.run(), m0) and not same(m0, before[0])


# ---- 4. conditioning ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "nosc"])
def test_everything_known_is_sanity_mode_nothing_known_is_sample(name):
    c = case(name)
    full = c.cond(*c.masks(1))
    smp = c.sampler()
    kw = c.kw()
    sa, sn = smp.sample(c.net, c.flags, sanity_check_gt_adjs=c.ka, sanity_check_gt_nodes=c.kn, **kw)
    assert same(full, c.full(sa, sn))
    assert (full[0] - c.ka)[c.va].abs().max() < 1e-6 and (full[1] - c.kn)[c.vn].abs().max() < 1e-6
    none = c.cond(*c.masks(0))
    plain = c.run()
    assert same(none, plain) and none[2] == plain[2]
    # the float64 known-answer run takes the Euler branch (D = D_prev = gt): it lands on the known values too
    kw.pop("return_device")
    da, dn = smp.sample(c.net, c.flags, sanity_check_gt_adjs=c.ka, sanity_check_gt_nodes=c.kn, flag_use_double=True, **kw)
    da, dn = c.full(da.cuda(), dn.cuda())
    assert da.dtype == torch.float64 and (da - c.ka)[c.va].abs().max() < 1e-9 and (dn - c.kn)[c.vn].abs().max() < 1e-9


@pytest.mark.parametrize("name,T_", [("tiny", 8), ("small", 6), ("vg", 2), ("vg", 3), ("vg", 4)])
def test_known_entries_land(name, T_):
    c = case(name)
    smp = c.sampler(T_=T_)
    oa, on = smp.sample_known(c.net, c.flags, c.ka, c.kn, c.ma, c.mn, **c.kw(coins=c.coins[:T_]))
    oa, on = c.full(oa, on)
    ka_, kn_ = c.ma.bool() & c.va, c.mn.bool() & c.vn
    ea, en = float((oa - c.ka)[ka_].abs().max()), float((on - c.kn)[kn_].abs().max())
    print(f"{name} T = {T_}: known entries off by adj {ea:.2e} node {en:.2e} (output scale 1)")
    assert ea < 1e-6 and en < 1e-6
    assert torch.all(oa[~c.va] == 0) and torch.all(on[~c.vn] == 0)
    assert torch.isfinite(oa).all() and torch.isfinite(on).all()
    assert smp.last_stats["precond_calls"] == T_


# ---- 5./6. order ----------------------------------------------------------------------------------------------------------------------------
_order = {}


def order_errors(name, Ts):
    """max-abs error of solver='euler' and solver='dpmpp_2m' at every T of Ts against solver='euler' at T = 2048 (computed once), relative
    to the reference's max |value|; inputs Y.sampler_case(cfg, 2, 4, VALID4, 3, "dpm/<name>", "euler"), no churn, no coin fired"""
    if name not in _order:
        c = Case(name, 4, VALID4, 2)
        _order[name] = (c, c.run("euler", T_=2048, **c.kw(coins=np.zeros(2048, np.uint8))), {})
    c, ref, errs = _order[name]
    for T_ in Ts:
        for solver in ("euler", "dpmpp_2m"):
            if (solver, T_) not in errs:
                o = c.run(solver, T_=T_, **c.kw(coins=np.zeros(T_, np.uint8)))
                assert o[2]["precond_calls"] == o[2]["net_forwards"] == T_
                errs[solver, T_] = tuple(rel_err(o[k].cpu().numpy(), ref[k].cpu().numpy()) for k in (0, 1))
    return errs


def test_second_order_without_self_conditioning():
    """nosc: the loop is an ODE solve in x alone.  At equal cost the multistep solver has at most half of Euler's error at T = 32 (float64
    CPU oracle: 0.20 adj / 0.22 node), and doubling T takes its error to at most 0.4 of itself (oracle: 0.26 / 0.22; a first-order method
    gives 0.5).  fp32 noise of the trajectories, about 1e-5, is far below the errors compared (1e-2)."""
    e = order_errors("nosc", (16, 32))
    for k, what in enumerate(("adj", "node")):
        e16, e32, m16, m32 = e["euler", 16][k], e["euler", 32][k], e["dpmpp_2m", 16][k], e["dpmpp_2m", 32][k]
        print(f"nosc {what}: euler T=16 {e16:.3e} T=32 {e32:.3e} | dpmpp_2m T=16 {m16:.3e} T=32 {m32:.3e} | "
              f"2M/Euler at 32 {m32 / e32:.3f}, 2M 32/16 {m32 / m16:.3f}, Euler 32/16 {e32 / e16:.3f}")
    for k, what in enumerate(("adj", "node")):
        assert e["dpmpp_2m", 32][k] <= 0.5 * e["euler", 32][k], what
        assert e["dpmpp_2m", 32][k] <= 0.4 * e["dpmpp_2m", 16][k], what


def test_gain_with_self_conditioning():
    """tiny, coins all 0: the field also depends on the previous D, so the loop stays first order in T -- still, at equal cost the multistep
    solver's error at T = 32 is at most 0.8 of Euler's (float64 CPU oracle: 0.58 adj / 0.43 node).  T = 16 and T = 64 are printed."""
    e = order_errors("tiny", (16, 32, 64))
    for k, what in enumerate(("adj", "node")):
        print(f"tiny {what}: " + ", ".join(f"T={T_} euler {e['euler', T_][k]:.3e} dpmpp_2m {e['dpmpp_2m', T_][k]:.3e} "
                                           f"ratio {e['dpmpp_2m', T_][k] / e['euler', T_][k]:.3f}" for T_ in (16, 32, 64)))
    for k, what in enumerate(("adj", "node")):
        assert e["dpmpp_2m", 32][k] <= 0.8 * e["euler", 32][k], what


# ---- 7. snapshots, stats, refusal -----------------------------------------------------------------------------------------------------------
def test_snapshots_and_stats_count_executed_steps():
    c = case("tiny")
    walk = dict(resample=(2, 3))
    got = c.cond(c.ma, c.mn, **walk)
    kw = c.kw(24)
    kw.pop("return_device")
    smp = c.sampler()
    a, x, a_ls, n_ls = smp.sample_known(c.net, c.flags, c.ka, c.kn, c.ma, c.mn, flag_interim_adjs=True, **kw, **walk)
    assert a_ls.shape == (25,) + c.sa and n_ls.shape == (25,) + c.sn            # init + one snapshot per executed step
    assert torch.equal(a_ls[0], c.ia.cpu()) and torch.equal(a_ls[-1], a) and torch.equal(n_ls[-1], x)
    assert torch.equal(a, got[0].cpu()) and torch.equal(x, got[1].cpu())
    fired = int(c.coins[:24].sum())
    assert smp.last_stats == {"precond_calls": 24, "net_forwards": 24 + fired, "graph_replays": 24 + fired} == got[2]
    a, x, a_ls, n_ls = smp.sample(c.net, c.flags, flag_interim_adjs=True, max_num_interim_adjs=4, **c.kw() | {"return_device": False})
    slots = len(np.unique(np.linspace(0, 8, 4).astype(int).clip(max=7))) + 1
    assert a_ls.shape == (slots,) + c.sa and torch.equal(a_ls[-1], a) and torch.equal(a, c.run()[0].cpu())
    assert smp.last_stats["precond_calls"] == 8 and smp.last_stats["net_forwards"] == 8 + int(c.coins[:8].sum())


def test_churn_is_refused_by_the_library_before_any_launch():
    c = case("tiny")
    smp = c.sampler()
    smp.S_churn = 40.0   # past the constructor's check: the library's own
    with pytest.raises(lib.DsgError, match=f"status {lib.DSG_ERR_INVALID}.*S_churn = 0"):
        smp.sample(c.net, c.flags, **c.kw(8))
    assert smp.last_stats is None
    smp.S_churn = 0.0
    oa, on = smp.sample(c.net, c.flags, **c.kw())
    assert same(c.full(oa, on), c.run())          # and the handle is left usable
