"""GPU: walks over the noise levels (dsg_sample_walk / sample_known(resample=, resample_range=, start_step=, base_*=)): RePaint-style
resampling and the partial-noise start.

The reference has neither, so -- like tests/test_complete.py -- the feature is pinned to paths that are pinned: the trivial walk must
equal today's calls bit for bit, and a real walk is compared with the same loop re-enacted in torch around single NodeAdjPrecondHip
calls, iterating the rows lib.walk_steps returns (schedule index, merged churn coefficient, noise slice = executed step), at the
project's trajectory bar util.FWD_RTOL.  Shapes: tiny (B = 4, T = 8, Heun + churn, resample (2, 3): L = 24), small (B = 3, valid
[16, 9, 4], T = 6, Euler without churn, resample (3, 2)), vg (B = 2, valid [30, 11], T = 2, resample (1, 2): L = 4)."""
import ctypes as C

import numpy as np
import pytest
import torch

from diffusesg_amd import lib
from diffusesg_amd import synth as Y
from diffusesg_amd import weights as W
from util import FWD_RTOL, assert_close, rel_err

pytestmark = pytest.mark.gpu

_nets = {}


def net_for(name):
    from diffusesg_amd.model import build_network
    if name not in _nets:
        cfg = Y.CONFIGS[name]()
        _nets[name] = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")
    return _nets[name]


def T(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def make_sampler(T_, solver="heun", S_churn=40.0, use_graph=True, self_condition=True):
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    return NodeAdjEDMSamplerHip(num_steps=T_, solver=solver, S_churn=S_churn, dev="cuda", objective="edm",
                                self_condition=self_condition, symmetric_noise=False, use_graph=use_graph)


class Case:
    """Recorded inputs for walks of up to Lmax executed steps on a T-step schedule: Y.sampler_case called with T_ = Lmax (Lmax noise
    slices, enough coins), +-1 known values from Y.gt_case.  The plain loop uses the first T slices."""

    def __init__(self, name, B, valid, T_, Lmax, solver="heun", churn=40.0, tag=None, net=None):
        self.name, self.B, self.T, self.solver, self.churn = name, B, T_, solver, churn
        self.net = net if net is not None else net_for(name)
        self.cfg = cfg = Y.CONFIGS[name]()
        flags, ia, inn, na, nn, cv = Y.sampler_case(cfg, Lmax, B, valid, 3, tag or f"rsm/{name}", solver)
        self.coins = (cv < 0.5).astype(np.uint8)
        ka, kn = Y.gt_case(cfg, B, valid)
        self.flags, self.ia, self.inn, self.na, self.nn, self.ka, self.kn = T(flags), T(ia), T(inn), T(na), T(nn), T(ka), T(kn)
        n = cfg.max_node_num
        self.sa, self.sn = (B, cfg.c_adj, n, n), (B, n, cfg.c_node)
        f = self.flags.bool()
        self.va = (f[:, None, :, None] & f[:, None, None, :]).expand(self.sa)   # valid entries
        self.vn = f[:, :, None].expand(self.sn)

    def scfg(self):
        return lib.make_sampler_cfg(self.T, self.solver, self.churn, 0.05, 50.0, 1.003, 0.002, 80.0, 7.0, False)

    def steps(self, **walk):
        return lib.walk_steps(self.scfg(), lib.make_walk_cfg(walk.get("start_step", 0), walk.get("resample"), walk.get("resample_range")))

    def kw(self, L=None, recorded=True, seed=11):
        L = self.T if L is None else L
        d = dict(coins=self.coins, num_node_chan=self.cfg.c_node, num_edge_chan=self.cfg.c_adj, return_device=True)
        if recorded:
            d.update(init_adjs=self.ia, init_nodes=self.inn, churn_noise=(self.na[:L], self.nn[:L]))
        else:
            d.update(seed=seed)
        return d

    def masks(self, fill):
        return (torch.full(self.sa, fill, dtype=torch.uint8, device="cuda"), torch.full(self.sn, fill, dtype=torch.uint8, device="cuda"))

    def random_masks(self, tag="rsm/mask"):
        """W.uniform01 < 0.5 per element"""
        na, nn = int(np.prod(self.sa)), int(np.prod(self.sn))
        return (T((W.uniform01(3, f"{tag}/{self.name}/adj", na) < 0.5).astype(np.uint8).reshape(self.sa)),
                T((W.uniform01(3, f"{tag}/{self.name}/node", nn) < 0.5).astype(np.uint8).reshape(self.sn)))

    def sampler(self, use_graph=True):
        return make_sampler(self.T, self.solver, self.churn, use_graph, self.cfg.self_condition)

    def uncond(self, use_graph=True, **kw):
        smp = self.sampler(use_graph)
        oa, on = smp.sample(self.net, self.flags, **(kw or self.kw()))
        return oa.clone(), on.clone(), dict(smp.last_stats)

    def cond(self, ma, mn, use_graph=True, recorded=True, seed=11, ka=None, kn=None, **walk):
        """sample_known, plain (no walk keyword) or along a walk; recorded randomness sliced to the walk's L"""
        smp = self.sampler(use_graph)
        L = len(self.steps(**walk)[0]) if walk else self.T
        oa, on = smp.sample_known(self.net, self.flags, self.ka if ka is None else ka, self.kn if kn is None else kn, ma, mn,
                                  **self.kw(L, recorded, seed), **walk)
        return oa.clone(), on.clone(), dict(smp.last_stats)


_cases = {}


def tiny_case():
    """tiny with a random half-known mask, its plain conditioned result and its resample=(2, 3) result (computed once)"""
    if "tiny" not in _cases:
        c = Case("tiny", 4, Y.SAMPLER_VALID, 8, 48)
        c.ma, c.mn = c.random_masks()
        c.plain = c.cond(c.ma, c.mn)
        c.walk = dict(resample=(2, 3))
        c.walked = c.cond(c.ma, c.mn, **c.walk)
        _cases["tiny"] = c
    return _cases["tiny"]


def small_case():
    if "small" not in _cases:
        c = Case("small", 3, [16, 9, 4], 6, 12, "euler", 0.0)
        c.ma, c.mn = c.random_masks()
        c.walk = dict(resample=(3, 2), resample_range=(0, 6))
        c.walked = c.cond(c.ma, c.mn, **c.walk)
        _cases["small"] = c
    return _cases["small"]


def vg_case():
    if "vg" not in _cases:
        c = Case("vg", 2, [30, 11], 2, 4, tag="rsm/vg4")
        c.ma, c.mn = c.random_masks()
        c.walk = dict(resample=(1, 2))
        c.walked = c.cond(c.ma, c.mn, **c.walk)
        _cases["vg"] = c
    return _cases["vg"]


CASES = {"tiny": tiny_case, "small": small_case, "vg": vg_case}


def raw_walk(c, wcfg, known, use_graph=True, recorded=True, seed=11):
    """dsg_sample_walk at the C level; known = (ka, kn, ma, mn) with None entries passed as NULL"""
    net = c.net.model
    h = net._ensure_handle()
    scfg = lib.make_sampler_cfg(c.T, c.solver, c.churn, 0.05, 50.0, 1.003, 0.002, 80.0, 7.0, use_graph)
    L = len(lib.walk_steps(scfg, wcfg)[0])
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    fl = c.flags.to(torch.uint8).contiguous()
    oa, on = torch.empty(c.sa, dtype=torch.float32, device="cuda"), torch.empty(c.sn, dtype=torch.float32, device="cuda")
    ia, inn, na, nn = (c.ia, c.inn, c.na[:L].contiguous(), c.nn[:L].contiguous()) if recorded else (None,) * 4
    stats = lib.DsgSampleStats()
    st = torch.cuda.current_stream().cuda_stream
    rc = h.L.dsg_sample_walk(h.raw, C.byref(scfg), C.byref(wcfg), c.B, p(fl), p(ia), p(inn), None, None, p(na), p(nn),
                             C.c_void_p(c.coins.ctypes.data), C.c_uint64(seed), *[p(t) for t in known], None, 0, None, None,
                             p(oa), p(on), C.byref(stats), C.c_void_p(st))
    h.check(rc, "dsg_sample_walk")
    return oa, on, {"precond_calls": stats.precond_calls, "net_forwards": stats.net_forwards, "graph_replays": stats.graph_replays}


# ---- 1. the trivial walk is today's loop ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("recorded", [True, False])
def test_trivial_walk_equals_plain_calls(use_graph, recorded):
    c = tiny_case()
    pa, pn, pst = c.cond(c.ma, c.mn, use_graph, recorded)
    if use_graph and recorded:
        assert torch.equal(pa, c.plain[0]) and torch.equal(pn, c.plain[1])
    zero = (torch.zeros(c.sa, device="cuda"), torch.zeros(c.sn, device="cuda"))
    for walk in (dict(resample=(5, 1)), dict(resample=(2, 3), resample_range=(3, 3)), dict(base_adjs=zero[0], base_nodes=zero[1])):
        oa, on, st = c.cond(c.ma, c.mn, use_graph, recorded, **walk)
        assert torch.equal(oa, pa) and torch.equal(on, pn), sorted(walk)
        assert st == pst
    # all four known pointers NULL at the C level: an unconditioned walk, dsg_sample's result
    ua, un, ust = c.uncond(use_graph, **c.kw(None, recorded))
    oa, on, st = raw_walk(c, lib.make_walk_cfg(0, (5, 1)), (None,) * 4, use_graph, recorded)
    assert torch.equal(oa, ua) and torch.equal(on, un) and st == ust
    assert not torch.equal(ua, pa)


# ---- 2. composition ---------------------------------------------------------------------------------------------------------------
def eager_walk(c, ma, mn, walk, noise=None, init=None, base=None):
    """The conditioned loop along a walk, re-enacted in torch float32 on the device: one row of lib.walk_steps per executed step k --
    the row's schedule index picks t_hat / h (lib.sigma_schedule), the row's noise_coef scales noise slice k -- one NodeAdjPrecondHip
    call per network forward with its own coin pinned to 'not fired', the known-entry select in torch.  noise(k) -> (adj, node) of
    executed step k (default: the recorded slices); base: the partial-noise start, x = mask(base + t_s * init)."""
    net, cfg = c.net, c.cfg
    sg, t_hat, nz, hs = lib.sigma_schedule(c.scfg())
    sched, coef = c.steps(**walk)
    fa, fn = c.va.float(), c.vn.float()
    ka, kn, ba, bn = c.ka, c.kn, ma.bool(), mn.bool()
    noise = noise or (lambda k: (c.na[k], c.nn[k]))
    ia, inn = init or (c.ia, c.inn)

    def select(D):
        return torch.where(ba, ka, D[0].reshape(c.sa)) * fa, torch.where(bn, kn, D[1].reshape(c.sn)) * fn

    def P(x, sigma, sc):
        real = np.random.rand
        np.random.rand = lambda: 0.9   # the call's own coin never fires
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
    sc, call = (None, None), 0
    for k, (i, cf) in enumerate(zip(sched.tolist(), coef.tolist())):
        th, h = float(t_hat[i]), float(hs[i])
        ea, en = noise(k)
        xh = ((x[0] + cf * ea) * fa, (x[1] + cf * en) * fn)
        D1 = denoise(xh, th, sc, c.coins[call]); call += 1
        d1 = tuple((a - b) / th for a, b in zip(xh, D1))
        last = D1
        if c.solver == "euler" or i == c.T - 1:
            x = tuple(a + h * d for a, d in zip(xh, d1))
        else:
            D2 = denoise(xh, th, D1 if cfg.self_condition else (None, None), c.coins[call]); call += 1
            tp = th + h
            xp = tuple(a + h * d for a, d in zip(xh, d1))
            d2 = tuple((a - b) / tp for a, b in zip(xp, D2))
            x = tuple(a + h * (0.5 * p + 0.5 * q) for a, p, q in zip(xh, d1, d2))
            last = D2
        x = (x[0] * fa, x[1] * fn)
        sc = last if cfg.self_condition else (None, None)   # carried over a jump unchanged
    return x, call


def check_vs_eager(what, got, want):
    (oa, on), (ea, en) = got, want
    print(f"{what}: rel err adj {rel_err(oa.cpu().numpy(), ea.cpu().numpy()):.3e} node {rel_err(on.cpu().numpy(), en.cpu().numpy()):.3e}")
    assert_close(oa.cpu().numpy(), ea.cpu().numpy(), FWD_RTOL, f"{what} adj vs eager composition")
    assert_close(on.cpu().numpy(), en.cpu().numpy(), FWD_RTOL, f"{what} node vs eager composition")


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_walk_vs_eager_composition(name):
    c = CASES[name]()
    oa, on, st = c.walked
    (ea, en), calls = eager_walk(c, c.ma, c.mn, c.walk)
    check_vs_eager(f"{name} recorded noise", (oa, on), (ea, en))
    assert st["precond_calls"] == calls


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_walk_vs_eager_composition_device_noise(name):
    """executed step k draws Philox stream k + 1 (stream 0 = the initial sample), whichever schedule index it runs at"""
    c = CASES[name]()
    smp, seed = c.sampler(), 23
    oa, on, _ = c.cond(c.ma, c.mn, recorded=False, seed=seed, **c.walk)
    init = smp.device_noise(c.net, c.flags, stream=0, seed=seed)
    (ea, en), _ = eager_walk(c, c.ma, c.mn, c.walk, noise=lambda k: smp.device_noise(c.net, c.flags, stream=k + 1, seed=seed), init=init)
    check_vs_eager(f"{name} device noise", (oa, on), (ea, en))


# ---- 3. known entries land, padded entries are 0 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "small", "vg"])
def test_known_entries_land_under_resampling(name):
    c = CASES[name]()
    oa, on, _ = c.walked
    ka_, kn_ = c.ma.bool() & c.va, c.mn.bool() & c.vn
    assert (oa - c.ka)[ka_].abs().max() < 1e-6 and (on - c.kn)[kn_].abs().max() < 1e-6
    assert torch.all(oa[~c.va] == 0) and torch.all(on[~c.vn] == 0)
    assert torch.isfinite(oa).all() and torch.isfinite(on).all()
    # everything known: the result is the known tensor
    oa, on, _ = c.cond(*c.masks(1), **c.walk)
    assert (oa - c.ka)[c.va].abs().max() < 1e-6 and (on - c.kn)[c.vn].abs().max() < 1e-6
    assert torch.all(oa[~c.va] == 0) and torch.all(on[~c.vn] == 0)


# ---- 4. resampling does something --------------------------------------------------------------------------------------------------
def test_resampling_changes_the_unknown_entries():
    c = tiny_case()
    fa_, fn_ = ~c.ma.bool() & c.va, ~c.mn.bool() & c.vn
    ea = rel_err(c.walked[0][fa_].cpu().numpy(), c.plain[0][fa_].cpu().numpy())
    en = rel_err(c.walked[1][fn_].cpu().numpy(), c.plain[1][fn_].cpu().numpy())
    print(f"tiny: unknown entries, resampled vs plain conditioned: adj {ea:.3e} node {en:.3e}")
    assert ea > FWD_RTOL and en > FWD_RTOL


# ---- 5. graph == eager -------------------------------------------------------------------------------------------------------------
def test_graph_equals_eager_under_resampling():
    c = tiny_case()
    oa, on, st = c.walked                                   # use_graph, loop_graph = 1
    assert st["graph_replays"] == st["net_forwards"]
    ea, en, est = c.cond(c.ma, c.mn, use_graph=False, **c.walk)
    assert est["graph_replays"] == 0 and est["net_forwards"] == st["net_forwards"]
    assert torch.equal(oa, ea) and torch.equal(on, en)
    h = c.net.model._ensure_handle()
    assert h.get_option("loop_graph") == 1
    h.set_option("loop_graph", 0)
    try:
        fa, fn, fst = c.cond(c.ma, c.mn, use_graph=True, **c.walk)    # only the network forward is a graph
        ga, gn, gst = c.cond(c.ma, c.mn, use_graph=False, **c.walk)
    finally:
        h.set_option("loop_graph", 1)
    assert torch.equal(fa, ea) and torch.equal(fn, en) and torch.equal(ga, ea) and torch.equal(gn, en)
    assert fst["graph_replays"] == fst["net_forwards"] == st["net_forwards"] and gst["graph_replays"] == 0
    ra, rn, _ = c.cond(c.ma, c.mn, use_graph=True, **c.walk)          # step bodies captured afresh after the option change
    assert torch.equal(ra, ea) and torch.equal(rn, en)


# ---- 6. stats ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "small", "vg"])
def test_stats_count_the_walk(name):
    c = CASES[name]()
    st = c.walked[2]
    sched, _ = c.steps(**c.walk)
    calls = sum(2 if (c.solver == "heun" and i != c.T - 1) else 1 for i in sched.tolist())
    assert st["precond_calls"] == calls
    fired = int(c.coins[:calls].sum()) if c.cfg.self_condition else 0
    assert st["net_forwards"] == calls + fired
    assert st["graph_replays"] == st["net_forwards"]
    assert len(sched) == {"tiny": 24, "small": 12, "vg": 4}[name]


# ---- 7. nothing sticky ---------------------------------------------------------------------------------------------------------------
def test_nothing_sticky_and_step_table_growth():
    """one fresh handle, one batch size: plain calls, a walk (the step table grows from 8 to 24 rows and the captured bodies are
    dropped), plain calls again, a longer walk (48 rows), and again"""
    from diffusesg_amd.model import build_network
    cfg = Y.CONFIGS["tiny"]()
    net = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")
    c = Case("tiny", 5, [8, 5, 3, 8, 6], 8, 48, net=net, tag="rsm/sticky")
    ma, mn = c.random_masks("rsm/sep")
    u0, k0 = c.uncond(), c.cond(ma, mn)
    w24 = c.cond(ma, mn, resample=(2, 3))
    u1, k1 = c.uncond(), c.cond(ma, mn)
    assert torch.equal(u1[0], u0[0]) and torch.equal(u1[1], u0[1]) and u1[2] == u0[2]
    assert torch.equal(k1[0], k0[0]) and torch.equal(k1[1], k0[1]) and k1[2] == k0[2]
    w48 = c.cond(ma, mn, resample=(4, 6))                       # L = 48: the table grows between the two
    assert w48[2]["precond_calls"] == 2 * 48 - 6
    u2, k2, w24b = c.uncond(), c.cond(ma, mn), c.cond(ma, mn, resample=(2, 3))
    assert torch.equal(u2[0], u0[0]) and torch.equal(u2[1], u0[1]) and u2[2] == u0[2]
    assert torch.equal(k2[0], k0[0]) and torch.equal(k2[1], k0[1]) and k2[2] == k0[2]
    assert torch.equal(w24b[0], w24[0]) and torch.equal(w24b[1], w24[1]) and w24b[2] == w24[2]
    assert not torch.equal(w24[0], k0[0]) and not torch.equal(w48[0], w24[0])
    # an unconditioned walk leaves nothing behind either
    raw_walk(c, lib.make_walk_cfg(0, (2, 2)), (None,) * 4)
    k3 = c.cond(ma, mn)
    assert torch.equal(k3[0], k0[0]) and torch.equal(k3[1], k0[1])


# ---- 8. partial start -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", [dict(start_step=3), dict(start_step=3, resample=(2, 2), resample_range=(3, 8))], ids=["plain", "resampled"])
def test_partial_noise_start(walk):
    """tiny from index 3, base = the +-1 values of Y.gt_case (which the known entries are held at, so base and known agree)"""
    c = tiny_case()
    sched, _ = c.steps(**walk)
    assert sched[0] == 3 and len(sched) == (5 if "resample" not in walk else 10)
    oa, on, st = c.cond(c.ma, c.mn, base_adjs=c.ka, base_nodes=c.kn, **walk)
    (ea, en), calls = eager_walk(c, c.ma, c.mn, walk, base=(c.ka, c.kn))
    check_vs_eager(f"tiny partial start {sorted(walk)}", (oa, on), (ea, en))
    assert st["precond_calls"] == calls
    ka_, kn_ = c.ma.bool() & c.va, c.mn.bool() & c.vn
    assert (oa - c.ka)[ka_].abs().max() < 1e-6 and (on - c.kn)[kn_].abs().max() < 1e-6
    assert torch.all(oa[~c.va] == 0) and torch.all(on[~c.vn] == 0)


def test_partial_noise_start_needs_a_base():
    c = tiny_case()
    with pytest.raises(ValueError, match="start_step = 3 > 0 needs base_adjs"):
        c.cond(c.ma, c.mn, start_step=3)
    with pytest.raises(lib.DsgError, match=f"status {lib.DSG_ERR_INVALID}.*start_step 3 > 0 needs base_adj"):   # and the library itself
        raw_walk(c, lib.make_walk_cfg(3), (c.ka, c.kn, c.ma, c.mn))


# ---- 9. the jump-back draw --------------------------------------------------------------------------------------------------------------
def test_jump_back_variance_with_device_noise():
    """small net, Euler without churn, everything known, resample (3, 2) on T = 6: walk 0 1 2 | 0 1 2 | 3 4 5 | 3 4 5.  With D = known
    the state is known + t * e throughout; after executed step 3 (index 0 again, the jump from t_3 back to t_0 merged into its churn
    draw) it sits at t_1, and e = (x - known) / t_1 must be a unit Gaussian: 24 * (3 * 256 + 16 * 5) = 20352 elements, sampling error of
    the standard deviation 0.5 %, bar 3 % = six sigma."""
    c = Case("small", 24, [16] * 24, 6, 12, "euler", 0.0, tag="rsm/var")
    assert int(c.va.sum() + c.vn.sum()) >= 20000
    smp = c.sampler()
    ma, mn = c.masks(1)
    a, x, a_ls, n_ls = smp.sample_known(c.net, c.flags, c.ka, c.kn, ma, mn, flag_interim_adjs=True, seed=31, resample=(3, 2),
                                        num_node_chan=c.cfg.c_node, num_edge_chan=c.cfg.c_adj)
    assert a_ls.shape == (13,) + c.sa and n_ls.shape == (13,) + c.sn          # unscaled init + one slot per executed step
    sg = lib.sigma_schedule(c.scfg())[0].astype(np.float32)
    ka, kn, va, vn = c.ka.cpu(), c.kn.cpu(), c.va.cpu(), c.vn.cpu()

    def e_after(k, t):   # slot k + 1 = the state after executed step k, at level t
        return torch.cat([((a_ls[k + 1] - ka) / float(t))[va], ((n_ls[k + 1] - kn) / float(t))[vn]]).double()

    before, after = e_after(2, sg[3]), e_after(3, sg[1])
    sd = float(after.std())
    print(f"jump-back: std of (x - known) / t_next after the first step of the repeated pass {sd:.4f} (before the jump {float(before.std()):.4f}), "
          f"n = {after.numel()}")
    assert abs(sd - 1.0) < 0.03 and abs(float(after.mean())) < 0.03
    # fresh draws, not the old noise rescaled: the two fields are unrelated element by element
    corr = float(((before - before.mean()) * (after - after.mean())).mean() / (before.std() * after.std()))
    diff = float((before - after).abs().mean())
    print(f"jump-back: correlation with the field before the jump {corr:.4f}, mean |difference| {diff:.3f} (independent: 1.128)")
    assert abs(corr) < 0.1 and diff > 0.5
    # and the run still lands on the known values
    assert (a - ka)[va].abs().max() < 1e-6 and (x - kn)[vn].abs().max() < 1e-6


# ---- 10. snapshots count executed steps ---------------------------------------------------------------------------------------------------
def test_snapshots_count_executed_steps():
    c = tiny_case()
    oa, on, _ = c.walked
    kw = c.kw(24)
    kw.pop("return_device")
    smp = c.sampler()
    a, x, a_ls, n_ls = smp.sample_known(c.net, c.flags, c.ka, c.kn, c.ma, c.mn, flag_interim_adjs=True, flag_adj_multi_channel=True, **kw, **c.walk)
    assert a_ls == [None] and n_ls.shape == (25, 4, 8, 12)               # init + one snapshot per executed step
    assert torch.equal(n_ls[0], c.inn.cpu()) and torch.equal(n_ls[-1], x)
    assert torch.equal(a, oa.cpu()) and torch.equal(x, on.cpu())
    for m in (4, 7):
        a, x, a_ls, n_ls = smp.sample_known(c.net, c.flags, c.ka, c.kn, c.ma, c.mn, flag_interim_adjs=True, max_num_interim_adjs=m, **kw, **c.walk)
        slots = len(np.unique(np.linspace(0, 24, m).astype(int).clip(max=23))) + 1
        assert slots == m + 1
        assert a_ls.shape == (slots, 4, 6, 8, 8) and n_ls.shape == (slots, 4, 8, 12)
        assert torch.equal(a_ls[0], c.ia.cpu()) and torch.equal(a_ls[-1], a) and torch.equal(n_ls[-1], x)   # the last slot, taken at L - 1
        assert torch.equal(a, oa.cpu())


# ---- 11. complete.py end to end -----------------------------------------------------------------------------------------------------------
def _int_graphs(cfg, B, valid, n_adj_type, n_node_type, tag):
    n = cfg.max_node_num
    flags = W.synth_flags(B, n, valid)
    f = flags.astype(np.int32)
    q_adj = (W.uniform01(9, f"{tag}/adj", B * n * n) * n_adj_type).astype(np.int32).reshape(B, n, n) * f[:, :, None] * f[:, None, :]
    q_adj[:, np.arange(n), np.arange(n)] = 0
    q_node = (W.uniform01(9, f"{tag}/node", B * n) * n_node_type).astype(np.int32).reshape(B, n) * f
    bbox = (0.1 + 0.8 * W.uniform01(9, f"{tag}/bbox", B * n * 4)).astype(np.float32).reshape(B, n, 4) * flags[:, :, None]
    return flags, q_adj, q_node, bbox


def test_complete_and_vary_end_to_end():
    from diffusesg_amd.complete import complete_scene_graphs, start_step_for_sigma, vary_scene_graphs
    cfg = Y.CONFIGS["tiny"]()   # 6 adjacency bits, 8 label bits + 4 box channels
    n_adj_type, n_node_type, valid = 51, 150, Y.SAMPLER_VALID
    flags, q_adj, q_node, bbox = _int_graphs(cfg, 4, valid, n_adj_type, n_node_type, "rsm/e2e")
    known = np.zeros_like(flags)
    for b, v in enumerate(valid):
        known[b, :(v + 1) // 2] = True   # half of each graph's valid nodes
    net, smp = net_for("tiny"), make_sampler(8)
    np.random.seed(5)
    qa, qn, bb = complete_scene_graphs(net, smp, T(q_adj), T(q_node), T(bbox), T(flags), T(known), n_adj_type, n_node_type, seed=21,
                                       resample=(2, 2))
    assert smp.last_stats["precond_calls"] == 2 * 16 - 2                   # the walk ran: L = 16, index 7 twice
    qa, qn, bb = qa.cpu().numpy(), qn.cpu().numpy(), bb.cpu().numpy()
    assert np.array_equal(qn[known], q_node[known])
    pair = known[:, :, None] & known[:, None, :] & ~np.eye(8, dtype=bool)[None]
    assert pair.sum() > 0 and np.array_equal(qa[pair], q_adj[pair])
    assert np.abs(bb[known] - bbox[known]).max() < 1e-6
    free = flags & ~known
    assert free.sum() > 0 and qn[free].min() >= 0 and qn[free].max() <= n_node_type - 1
    assert np.all(qa[~(flags[:, :, None] & flags[:, None, :])] == 0) and np.all(qn[~flags] == 0)
    # a variation from the last level (t_7 = 0.002): the noised base decodes to itself
    assert start_step_for_sigma(smp, float(smp.sigma_steps[7])) == 7 and start_step_for_sigma(smp, 80.0) == 0
    np.random.seed(6)
    qa, qn, bb = vary_scene_graphs(net, smp, T(q_adj), T(q_node), T(bbox), T(flags), n_adj_type, n_node_type, start_step=7, seed=22)
    assert smp.last_stats["precond_calls"] == 1
    qa, qn, bb = qa.cpu().numpy(), qn.cpu().numpy(), bb.cpu().numpy()
    off = flags[:, :, None] & flags[:, None, :] & ~np.eye(8, dtype=bool)[None]
    assert np.array_equal(qn[flags], q_node[flags]) and np.array_equal(qa[off], q_adj[off])
    assert np.isfinite(bb).all() and np.all(qn[~flags] == 0)
    # from further up, with half of the nodes held
    np.random.seed(7)
    qa, qn, bb = vary_scene_graphs(net, smp, T(q_adj), T(q_node), T(bbox), T(flags), n_adj_type, n_node_type, start_step=4,
                                   known_nodes=T(known), resample=(2, 2), seed=23)
    assert smp.last_stats["precond_calls"] == 2 * 8 - 2                    # indices 4..7 twice
    qa, qn, bb = qa.cpu().numpy(), qn.cpu().numpy(), bb.cpu().numpy()
    assert np.array_equal(qn[known], q_node[known]) and np.array_equal(qa[pair], q_adj[pair]) and np.abs(bb[known] - bbox[known]).max() < 1e-6


# ---- 12. errors -----------------------------------------------------------------------------------------------------------------------------
def test_errors_are_named_before_any_launch():
    c = tiny_case()
    smp = c.sampler()
    args = (c.net, c.flags, c.ka, c.kn, c.ma, c.mn)
    before = smp.last_stats
    for walk, what in ((dict(resample=(0, 2)), "jump_len 0"), (dict(resample=(2, 0)), "n_resample 0"),
                       (dict(resample=(2, 2), resample_range=(2, 9)), r"range \(2, 9\)"), (dict(resample=(2, 2), resample_range=(5, 4)), r"range \(5, 4\)"),
                       (dict(start_step=8, base_adjs=c.ka, base_nodes=c.kn), "start_step 8"),
                       (dict(start_step=4, resample=(2, 2), resample_range=(3, 8), base_adjs=c.ka, base_nodes=c.kn), r"start_step 4,.*range \(3, 8\)")):
        with pytest.raises(lib.DsgError, match=f"bad walk.*{what}"):
            smp.sample_known(*args, **c.kw(8), **walk)
    with pytest.raises(ValueError, match="leading dimensions 8 / 8, expected L = 24"):
        smp.sample_known(*args, **c.kw(8), resample=(2, 3))
    kw = c.kw(24)
    kw["coins"] = c.coins[:2 * 8 - 1]                 # enough for the plain loop, short for the walk
    with pytest.raises(ValueError, match="coins has 15 entries, the walk makes 45"):
        smp.sample_known(*args, **kw, resample=(2, 3))
    with pytest.raises(ValueError, match="base_adjs has shape"):
        smp.sample_known(*args, **c.kw(8), base_adjs=c.ka[:, :1], base_nodes=c.kn)
    with pytest.raises(ValueError, match="base_adjs and base_nodes must both be given"):
        smp.sample_known(*args, **c.kw(8), base_adjs=c.ka)
    assert smp.last_stats is before
    # partial known pointers at the C level
    known = [c.ka, c.kn, c.ma, c.mn]
    for k, what in enumerate(("known_adj", "known_node", "mask_adj", "mask_node")):
        part = list(known)
        part[k] = None
        with pytest.raises(lib.DsgError, match=f"status {lib.DSG_ERR_INVALID}.*all given or all NULL.*{what} is NULL"):
            raw_walk(c, lib.make_walk_cfg(0, (2, 3)), part)
    # and the handle is left usable
    oa, on, _ = c.cond(c.ma, c.mn, **c.walk)
    assert torch.equal(oa, c.walked[0]) and torch.equal(on, c.walked[1])
