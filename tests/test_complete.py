"""GPU: conditional sampling (dsg_sample_known / NodeAdjEDMSamplerHip.sample_known, dsg_encode, diffusesg_amd.complete).

The reference has no completion code, so nothing here is compared with a reference run of the feature.  Instead the feature is pinned
from both ends to paths that ARE pinned to the reference: with no entry known it must equal `sample()` bit for bit, with every entry
known the sanity-check mode (edm.py:372-377), and -- samples never interact -- a batch mixing both checks them side by side with no
tolerance.  A partly known batch is compared with the same loop re-enacted in torch around single NodeAdjPrecondHip calls, at the
project's 1e-4 bar for T = 8 trajectories (util.FWD_RTOL)."""
import numpy as np
import pytest
import torch

from diffusesg_amd import lib
from diffusesg_amd import spec as S
from diffusesg_amd import synth as Y
from diffusesg_amd import weights as W
from util import FWD_RTOL, assert_close, load, rel_err

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
    """Recorded inputs of one run: flags, init, churn noise and coins from Y.sampler_case, +-1 known values from Y.gt_case."""

    def __init__(self, name, B, valid, T_, solver="heun", churn=40.0, tag=None, net=None):
        self.name, self.B, self.T, self.solver, self.churn = name, B, T_, solver, churn
        self.net = net if net is not None else net_for(name)
        self.cfg = cfg = Y.CONFIGS[name]()
        flags, ia, inn, na, nn, cv = Y.sampler_case(cfg, T_, B, valid, 3, tag or f"cmp/{name}", solver)
        self.coins = (cv < 0.5).astype(np.uint8)
        if cfg.self_condition:
            assert self.coins.min() == 0 and self.coins.max() == 1, "the coin sequence must hold both outcomes"
        ka, kn = Y.gt_case(cfg, B, valid)
        self.flags_np = flags
        self.flags, self.ia, self.inn, self.na, self.nn, self.ka, self.kn = T(flags), T(ia), T(inn), T(na), T(nn), T(ka), T(kn)
        n = cfg.max_node_num
        self.sa, self.sn = (B, cfg.c_adj, n, n), (B, n, cfg.c_node)
        f = self.flags.bool()
        self.va = (f[:, None, :, None] & f[:, None, None, :]).expand(self.sa)   # valid entries
        self.vn = f[:, :, None].expand(self.sn)

    def kw(self, recorded=True, seed=None):
        d = dict(coins=self.coins, num_node_chan=self.cfg.c_node, num_edge_chan=self.cfg.c_adj, return_device=True)
        if recorded:
            d.update(init_adjs=self.ia, init_nodes=self.inn, churn_noise=(self.na, self.nn))
        else:
            d.update(seed=seed)
        return d

    def masks(self, fill):
        return (torch.full(self.sa, fill, dtype=torch.uint8, device="cuda"), torch.full(self.sn, fill, dtype=torch.uint8, device="cuda"))

    def random_masks(self, tag="cmp/mask"):
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

    def sanity(self, **kw):
        smp = self.sampler()
        oa, on = smp.sample(self.net, self.flags, sanity_check_gt_adjs=self.ka, sanity_check_gt_nodes=self.kn, **(kw or self.kw()))
        return oa.clone(), on.clone()

    def cond(self, ma, mn, use_graph=True, ka=None, kn=None, **kw):
        smp = self.sampler(use_graph)
        oa, on = smp.sample_known(self.net, self.flags, self.ka if ka is None else ka, self.kn if kn is None else kn, ma, mn,
                                  **(kw or self.kw()))
        return oa.clone(), on.clone(), dict(smp.last_stats)


_cases = {}


def tiny_case():
    """config tiny, B = 4, Y.SAMPLER_VALID, T = 8, Heun with churn; with its unconditioned and sanity-mode results (computed once)"""
    if "tiny" not in _cases:
        c = Case("tiny", 4, Y.SAMPLER_VALID, 8)
        c.ref_uncond = c.uncond()
        c.ref_sanity = c.sanity()
        _cases["tiny"] = c
    return _cases["tiny"]


@pytest.mark.parametrize("use_graph", [True, False])
def test_nothing_known_equals_sample(use_graph):
    c = tiny_case()
    ma, mn = c.masks(0)
    ua, un, ust = c.uncond(use_graph)
    oa, on, st = c.cond(ma, mn, use_graph)
    assert torch.equal(oa, ua) and torch.equal(on, un)
    assert st == ust
    assert torch.equal(ua, c.ref_uncond[0])   # and graph == eager on the unconditioned path, as ever
    # the device Philox path: init and churn noise drawn by the library
    kw = c.kw(recorded=False, seed=11)
    ua, un, ust = c.uncond(use_graph, **kw)
    oa, on, st = c.cond(ma, mn, use_graph, **kw)
    assert torch.equal(oa, ua) and torch.equal(on, un)
    assert st == ust


def test_everything_known_equals_sanity_mode():
    c = tiny_case()
    oa, on, st = c.cond(*c.masks(1))
    assert torch.equal(oa, c.ref_sanity[0]) and torch.equal(on, c.ref_sanity[1])
    # the bar of test_sampler_known_answer_and_snapshots
    assert (oa - c.ka)[c.va].abs().max() < 1e-6 and (on - c.kn)[c.vn].abs().max() < 1e-6
    assert st["net_forwards"] == st["precond_calls"] + int(c.coins.sum())   # the network still runs: only its output is replaced


def test_per_sample_structure_is_exact():
    """sample 0 all unknown, sample 1 all known, samples 2-3 a random half"""
    c = tiny_case()
    ma, mn = c.random_masks()
    ma[0], mn[0] = 0, 0
    ma[1], mn[1] = 1, 1
    oa, on, _ = c.cond(ma, mn)
    assert torch.equal(oa[0], c.ref_uncond[0][0]) and torch.equal(on[0], c.ref_uncond[1][0])
    assert torch.equal(oa[1], c.ref_sanity[0][1]) and torch.equal(on[1], c.ref_sanity[1][1])
    assert not torch.equal(oa[2], c.ref_uncond[0][2]) and not torch.equal(oa[2], c.ref_sanity[0][2])


def test_per_sample_structure_is_exact_at_vg_size():
    """N = 64 indexing and the pruned up path: B = 2, valid [30, 11], T = 2; sample 0 unknown, sample 1 known"""
    c = Case("vg", 2, [30, 11], 2, tag="cmp/vg4")
    ma, mn = c.masks(0)
    ma[1], mn[1] = 1, 1
    ua, un, _ = c.uncond()
    sa, sn = c.sanity()
    oa, on, _ = c.cond(ma, mn)
    assert torch.equal(oa[0], ua[0]) and torch.equal(on[0], un[0])
    assert torch.equal(oa[1], sa[1]) and torch.equal(on[1], sn[1])
    assert (oa[1] - c.ka[1])[c.va[1]].abs().max() < 1e-6 and torch.all(oa[~c.va] == 0) and torch.all(on[~c.vn] == 0)


def eager_known(c, ma, mn):
    """The conditioned loop (edm.py:350-427 with the select on every D) re-enacted in torch float32 on the device: scalars from
    lib.sigma_schedule, one NodeAdjPrecondHip call per network forward with its own coin pinned to 'not fired', the select in torch.
    A fired coin is two explicit calls: sc' = select(P(x_hat, t_hat, sc)), then D = select(P(x_hat, t_hat, sc'))."""
    net, cfg = c.net, c.cfg
    scfg = lib.make_sampler_cfg(c.T, c.solver, c.churn, 0.05, 50.0, 1.003, 0.002, 80.0, 7.0, False)
    sg, t_hat, nz, hs = lib.sigma_schedule(scfg)
    fa, fn = c.va.float(), c.vn.float()
    ka, kn, ba, bn = c.ka, c.kn, ma.bool(), mn.bool()

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

    t0 = float(np.float32(sg[0]))
    x = (c.ia * t0, c.inn * t0)
    sc, call = (None, None), 0
    for i in range(c.T):
        th, h = float(t_hat[i]), float(hs[i])
        xh = ((x[0] + float(nz[i]) * c.na[i]) * fa, (x[1] + float(nz[i]) * c.nn[i]) * fn)
        D1 = denoise(xh, th, sc, c.coins[call]); call += 1
        d1 = tuple((a - b) / th for a, b in zip(xh, D1))
        last = D1
        if c.solver == "euler" or i == c.T - 1:
            x = tuple(a + h * d for a, d in zip(xh, d1))
        else:
            D2 = denoise(xh, th, D1 if cfg.self_condition else (None, None), c.coins[call]); call += 1   # stage 2: (x_hat, t_hat), sc = D1
            tp = th + h
            xp = tuple(a + h * d for a, d in zip(xh, d1))
            d2 = tuple((a - b) / tp for a, b in zip(xp, D2))
            x = tuple(a + h * (0.5 * p + 0.5 * q) for a, p, q in zip(xh, d1, d2))
            last = D2
        x = (x[0] * fa, x[1] * fn)
        sc = last if cfg.self_condition else (None, None)
    return x


def mixed_case(name):
    key = "mixed/" + name
    if key not in _cases:
        if name == "tiny":
            c = tiny_case()
        else:   # 16 nodes, shifted masked blocks; Euler without churn
            c = Case("small", 3, [16, 9, 4], 6, "euler", 0.0)
            c.ref_uncond = c.uncond()
        ma, mn = c.random_masks("cmp/mixed")
        _cases[key] = (c, ma, mn, c.cond(ma, mn))
    return _cases[key]


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_mixed_mask_vs_eager_composition(name):
    c, ma, mn, (oa, on, st) = mixed_case(name)
    ea, en = eager_known(c, ma, mn)
    print(f"{name}: rel err adj {rel_err(oa.cpu().numpy(), ea.cpu().numpy()):.3e} node {rel_err(on.cpu().numpy(), en.cpu().numpy()):.3e}")
    assert_close(oa.cpu().numpy(), ea.cpu().numpy(), FWD_RTOL, f"{name} adj vs eager composition")
    assert_close(on.cpu().numpy(), en.cpu().numpy(), FWD_RTOL, f"{name} node vs eager composition")
    assert st["net_forwards"] == st["precond_calls"] + int(c.coins[:st["precond_calls"]].sum())


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_known_entries_land_and_conditioning_reaches_the_network(name):
    c, ma, mn, (oa, on, _) = mixed_case(name)
    ua, un, _ = c.ref_uncond
    ka_, kn_ = ma.bool() & c.va, mn.bool() & c.vn
    assert (oa - c.ka)[ka_].abs().max() < 1e-6 and (on - c.kn)[kn_].abs().max() < 1e-6
    assert torch.all(oa[~c.va] == 0) and torch.all(on[~c.vn] == 0)
    # unknown valid entries: if they agreed with the unconditioned run to the parity bar, the known context never reached the forward
    fa_, fn_ = ~ma.bool() & c.va, ~mn.bool() & c.vn
    ea, en = rel_err(oa[fa_].cpu().numpy(), ua[fa_].cpu().numpy()), rel_err(on[fn_].cpu().numpy(), un[fn_].cpu().numpy())
    print(f"{name}: unknown entries, conditioned vs unconditioned: adj {ea:.3e} node {en:.3e}")
    assert ea > FWD_RTOL and en > FWD_RTOL


def test_graph_equals_eager_under_conditioning():
    c, ma, mn, (oa, on, st) = mixed_case("tiny")   # use_graph, loop_graph = 1
    assert st["graph_replays"] == st["net_forwards"]
    ea, en, est = c.cond(ma, mn, use_graph=False)
    assert est["graph_replays"] == 0 and est["net_forwards"] == st["net_forwards"]
    assert torch.equal(oa, ea) and torch.equal(on, en)
    h = net_for("tiny").model._ensure_handle()
    assert h.get_option("loop_graph") == 1
    h.set_option("loop_graph", 0)
    try:
        fa, fn, fst = c.cond(ma, mn, use_graph=True)   # only the network forward is a graph
    finally:
        h.set_option("loop_graph", 1)
    assert torch.equal(fa, ea) and torch.equal(fn, en)
    assert fst["graph_replays"] == fst["net_forwards"] == st["net_forwards"]
    ga, gn, _ = c.cond(ma, mn, use_graph=True)         # step bodies captured afresh after the option change
    assert torch.equal(ga, ea) and torch.equal(gn, en)


def test_conditioned_and_unconditioned_step_graphs_do_not_share_a_slot():
    """one handle, one batch size: baseline -> conditioned -> unconditioned -> conditioned"""
    from diffusesg_amd.model import build_network
    cfg = Y.CONFIGS["tiny"]()
    net = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")   # a handle no conditioned call has touched
    c = Case("tiny", 5, [8, 5, 3, 8, 6], 8, net=net)
    base = c.uncond()
    ma, mn = c.random_masks("cmp/sep")
    c1 = c.cond(ma, mn)
    u = c.uncond()
    c2 = c.cond(ma, mn)
    assert torch.equal(u[0], base[0]) and torch.equal(u[1], base[1]) and u[2] == base[2]
    assert torch.equal(c1[0], c2[0]) and torch.equal(c1[1], c2[1])
    assert not torch.equal(c1[0], base[0])


def test_squeezed_single_channel_layouts():
    """config nosc: one channel each, no self-conditioning; known tensors and masks as [B,N,N] / [B,N]"""
    c = Case("nosc", 2, [8, 3], 6)
    ua, un, ust = c.uncond()
    sa, sn = c.sanity()
    assert ua.shape == (2, 8, 8) and un.shape == (2, 8)
    ka, kn = c.ka[:, 0], c.kn[..., 0]
    z = c.masks(0)
    oa, on, st = c.cond(z[0][:, 0], z[1][..., 0], ka=ka, kn=kn)
    assert oa.shape == (2, 8, 8) and on.shape == (2, 8)
    assert torch.equal(oa, ua) and torch.equal(on, un) and st == ust
    o = c.masks(1)
    oa, on, _ = c.cond(o[0][:, 0].bool(), o[1][..., 0].bool(), ka=ka, kn=kn)   # bool masks are taken as well
    assert torch.equal(oa, sa) and torch.equal(on, sn)
    assert (oa - ka)[c.va[:, 0]].abs().max() < 1e-6 and (on - kn)[c.vn[..., 0]].abs().max() < 1e-6


def test_snapshots_under_conditioning():
    c, ma, mn, (oa, on, _) = mixed_case("tiny")
    kw = c.kw()
    kw.pop("return_device")
    smp = c.sampler()
    a, x, a_ls, n_ls = smp.sample_known(c.net, c.flags, c.ka, c.kn, ma, mn, flag_interim_adjs=True, flag_adj_multi_channel=True, **kw)
    assert not a.is_cuda and a_ls == [None] and n_ls.shape == (9, 4, 8, 12)      # init + one snapshot per step, like sample()
    assert torch.equal(n_ls[0], c.inn.cpu()) and torch.equal(n_ls[-1], x)
    assert torch.equal(a, oa.cpu()) and torch.equal(x, on.cpu())
    a, x, a_ls, n_ls = smp.sample_known(c.net, c.flags, c.ka, c.kn, ma, mn, flag_interim_adjs=True, max_num_interim_adjs=4, **kw)
    assert a_ls.shape == (1 + 4, 4, 6, 8, 8) and n_ls.shape == (1 + 4, 4, 8, 12)
    assert torch.equal(a_ls[0], c.ia.cpu()) and torch.equal(a_ls[-1], a) and torch.equal(n_ls[-1], x)


def _enc_cfg(enc, n_adj_type, n_node_type, n=8):
    chans = {"bits": lambda k: int(np.ceil(np.log2(k))), "one_hot": lambda k: k, "ddpm": lambda k: 1}[enc]
    return S.ModelConfig(max_node_num=n, c_adj=chans(n_adj_type), c_node=chans(n_node_type) + 4, depths=(1, 1), num_heads=(3, 6),
                         window_size=4, self_condition=True)


@pytest.mark.parametrize("enc", ["bits", "one_hot", "ddpm"])
def test_encode_vs_reference_fixture_and_round_trip(enc):
    """dsg_encode against the reference's attribute_converter('int' -> enc) (tests/golden/complete_encode.npz,
    tools/gen_complete_golden.py): exactly equal.  The values are +-1, 0 and, for ddpm, 2 i / (k - 1) - 1, which the reference computes
    in float32 op by op (its data loader hands float32 tensors in, attribute_code.py:251) -- compared bit for bit."""
    from diffusesg_amd import io as dio
    g = load("complete_encode.npz")
    n_adj_type, n_node_type = (int(v) for v in g[f"{enc}_types"])
    cfg = _enc_cfg(enc, n_adj_type, n_node_type)
    flags, q_adj, q_node = g["flags"], g[f"{enc}_q_adj"], g[f"{enc}_q_node"]
    B, n = flags.shape
    bbox = W.uniform01(5, "cenc/bbox", B * n * 4).astype(np.float32).reshape(B, n, 4)
    h = lib.Handle(cfg)
    a, x = dio.encode(h, T(q_adj), T(q_node), T(bbox), T(flags), n_adj_type, n_node_type, enc, enc)
    assert a.shape == (B, cfg.c_adj, n, n) and x.shape == (B, n, cfg.c_node) and a.dtype == torch.float32
    assert np.array_equal(a.cpu().numpy(), g[f"{enc}_adj"].reshape(a.shape)), "adj"
    assert np.array_equal(x[..., :-4].cpu().numpy(), g[f"{enc}_node"].reshape(B, n, cfg.c_node - 4)), "node"
    want_box = (torch.from_numpy(bbox) - 0.5) * 2 * torch.from_numpy(flags)[:, :, None]
    assert torch.equal(x[..., -4:].cpu(), want_box), "bbox channels"
    qa, qn, bb = dio.decode(h, a, x, T(flags), n_adj_type, n_node_type, enc, enc)
    off_diag = ~np.eye(n, dtype=bool)[None]
    assert np.array_equal(qa.cpu().numpy() * off_diag, q_adj * off_diag) and np.array_equal(qn.cpu().numpy(), q_node)
    f = torch.from_numpy(flags)
    assert (bb.cpu() - torch.from_numpy(bbox))[f].abs().max() < 1e-6 and torch.all(bb.cpu()[~f] == 0)
    with pytest.raises(lib.DsgError, match="fewer than two types"):
        dio.encode(h, T(q_adj), T(q_node), T(bbox), T(flags), 1, n_node_type, enc, enc)
    h.close()


def _int_graphs(cfg, B, valid, n_adj_type, n_node_type, tag):
    n = cfg.max_node_num
    flags = W.synth_flags(B, n, valid)
    f = flags.astype(np.int32)
    q_adj = (W.uniform01(9, f"{tag}/adj", B * n * n) * n_adj_type).astype(np.int32).reshape(B, n, n) * f[:, :, None] * f[:, None, :]
    q_adj[:, np.arange(n), np.arange(n)] = 0
    q_node = (W.uniform01(9, f"{tag}/node", B * n) * n_node_type).astype(np.int32).reshape(B, n) * f
    bbox = (0.1 + 0.8 * W.uniform01(9, f"{tag}/bbox", B * n * 4)).astype(np.float32).reshape(B, n, 4) * flags[:, :, None]
    return flags, q_adj, q_node, bbox


def test_complete_scene_graphs_and_layout_end_to_end():
    from diffusesg_amd.complete import complete_scene_graphs, layout_from_graph
    cfg = Y.CONFIGS["tiny"]()   # 6 adjacency bits, 8 label bits + 4 box channels
    n_adj_type, n_node_type, valid = 51, 150, Y.SAMPLER_VALID
    flags, q_adj, q_node, bbox = _int_graphs(cfg, 4, valid, n_adj_type, n_node_type, "cmp/e2e")
    known = np.zeros_like(flags)
    for b, v in enumerate(valid):
        known[b, :(v + 1) // 2] = True   # half of each graph's valid nodes
    net, smp = net_for("tiny"), make_sampler(8)
    np.random.seed(5)
    qa, qn, bb = complete_scene_graphs(net, smp, T(q_adj), T(q_node), T(bbox), T(flags), T(known), n_adj_type, n_node_type, seed=21)
    assert qa.is_cuda and qa.dtype == torch.int32 and qa.shape == (4, 8, 8) and qn.shape == (4, 8) and bb.shape == (4, 8, 4)
    qa, qn, bb = qa.cpu().numpy(), qn.cpu().numpy(), bb.cpu().numpy()
    assert np.array_equal(qn[known], q_node[known])
    pair = known[:, :, None] & known[:, None, :] & ~np.eye(8, dtype=bool)[None]
    assert pair.sum() > 0 and np.array_equal(qa[pair], q_adj[pair])
    assert np.abs(bb[known] - bbox[known]).max() < 1e-6
    free = flags & ~known
    assert free.sum() > 0 and qn[free].min() >= 0 and qn[free].max() <= n_node_type - 1
    assert np.all(qa[~(flags[:, :, None] & flags[:, None, :])] == 0) and np.all(qn[~flags] == 0)
    # layout generation: every label and relation given, the boxes generated
    np.random.seed(6)
    qa, qn, bb = layout_from_graph(net, smp, T(q_adj), T(q_node), T(flags), n_adj_type, n_node_type, seed=22)
    qa, qn, bb = qa.cpu().numpy(), qn.cpu().numpy(), bb.cpu().numpy()
    off = flags[:, :, None] & flags[:, None, :] & ~np.eye(8, dtype=bool)[None]
    assert np.array_equal(qn[flags], q_node[flags]) and np.array_equal(qa[off], q_adj[off])
    assert np.isfinite(bb).all() and np.abs(bb[flags] - bbox[flags]).max() > 1e-3   # generated, not copied


def test_errors():
    c = tiny_case()
    ma, mn = c.masks(1)
    net, smp = net_for("tiny"), c.sampler()
    args = [c.ka, c.kn, ma, mn]
    for k, what in enumerate(("known_adj", "known_node", "mask_adj", "mask_node")):
        a = list(args)
        a[k] = None
        with pytest.raises(lib.DsgError, match=f"status {lib.DSG_ERR_INVALID}.*{what} is NULL"):
            smp.sample_known(net, c.flags, *a, **c.kw())
    # a wrong shape is refused in Python, before anything is launched
    before = dict(smp.last_stats) if smp.last_stats else None
    with pytest.raises(ValueError, match="known_adj_mask has shape"):
        smp.sample_known(net, c.flags, c.ka, c.kn, ma[:, :1], mn, **c.kw())
    with pytest.raises(ValueError, match="known_nodes has shape"):
        smp.sample_known(net, c.flags, c.ka, c.kn.reshape(4, -1), ma, mn, **c.kw())
    assert smp.last_stats == before
    # and the handle is left usable, unconditioned
    ua, un, _ = c.uncond()
    assert torch.equal(ua, c.ref_uncond[0]) and torch.equal(un, c.ref_uncond[1])
