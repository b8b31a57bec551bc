"""GPU: patch sizes 2 and 4 end to end (dsg_create_patch through the drop-in Python classes) against the reference's own modules at
`patch_size` 2 and 4 (tests/golden/fwd_patch_*.npz, sampler_patch.npz; tools/gen_patch_golden.py): the forward and its intermediates at
FWD_RTOL, exact zeros at masked entries, the sampler's trajectories at the T = 8 bar of test_sampler_trajectory_vs_reference with and
without captured step bodies, conditional sampling, the options that are off at p > 1 and the entries and options that are refused.
Every test here needs ModelConfig(patch_size=2 | 4), which the library refused before."""
import ctypes as C

import numpy as np
import pytest
import torch

from diffusesg_amd import lib as L
from diffusesg_amd import spec as S
from diffusesg_amd import synth as Y
from diffusesg_amd import weights as W
from util import FWD_RTOL, assert_close, load

pytestmark = pytest.mark.gpu

NAMES = list(Y.PATCH_CONFIGS)
_nets = {}


def net_for(name):
    from diffusesg_amd.model import build_network
    if name not in _nets:
        cfg = Y.PATCH_CONFIGS[name]()
        _nets[name] = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")
    return _nets[name]


def T(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def make_sampler(T_, solver="heun", S_churn=40.0, use_graph=True, clip=True):
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    kw = dict(clip_samples=True, clip_samples_min=-1.0, clip_samples_max=1.0, clip_samples_scope="x_0") if clip else {}
    return NodeAdjEDMSamplerHip(num_steps=T_, solver=solver, S_churn=S_churn, dev="cuda", objective="edm", self_condition=True,
                                symmetric_noise=False, use_graph=use_graph, **kw)


def _check_outputs(cfg, flags, oa, on, g, key, what):
    ea = assert_close(oa.cpu().numpy(), g[f"{key}_adj_out"], FWD_RTOL, f"{what} adj ({key})")
    en = assert_close(on.cpu().numpy(), g[f"{key}_node_out"], FWD_RTOL, f"{what} node ({key})")
    print(f"PATCHFWD {what} {key}: rel err adj {ea:.3e} node {en:.3e} (bar {FWD_RTOL:.0e})")
    n, f = cfg.max_node_num, torch.from_numpy(flags).cuda().bool()
    oa4 = oa.reshape(2, cfg.c_adj, n, n)
    assert torch.all(oa4.permute(0, 2, 3, 1)[~f] == 0) and torch.all(oa4.permute(0, 3, 2, 1)[~f] == 0)
    assert torch.all(on.reshape(2, n, cfg.c_node)[~f] == 0)


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("name", NAMES)
def test_forward_vs_reference_golden(name, fused):
    """with "fused_patch_embed" / "fused_readout" at 1 and at 0: p = 2, E = 96 takes the fused kernels at 1 and the chain at 0, p = 4 the
    chain either way; dsg_debug_patch_forms reports the route the test was written for"""
    cfg, flags, adj, node, sc_adj, sc_node = Y.patch_fwd_case(name)
    g = load(f"fwd_patch_{name}.npz")
    net = net_for(name).model
    h = net._ensure_handle()
    h.set_option("fused_patch_embed", fused)
    h.set_option("fused_readout", fused)
    try:
        oa, on = net(T(adj), T(node), T(flags), T(Y.FWD_C_NOISE))
        _check_outputs(cfg, flags, oa, on, g, "nosc", name)
        if cfg.self_condition:
            oa, on = net(T(adj), T(node), T(flags), T(Y.FWD_C_NOISE), T(sc_adj), T(sc_node))
            _check_outputs(cfg, flags, oa, on, g, "sc", name)
        want = "fused" if fused and cfg.patch_size == 2 and cfg.embed_dim == 96 else "chain"
        assert h.patch_forms(2) == (want, want)
        assert h.patch_forms(7) == (None, None)          # no forward at that batch size yet
    finally:
        h.set_option("fused_patch_embed", 1)
        h.set_option("fused_readout", 1)


@pytest.mark.parametrize("name", NAMES)
def test_forward_intermediates_vs_reference(name):
    """PatchEmbed's output [B, R^2, E] (the fused kernel's at p = 2) and the read-out's [B, N^2, E] in pixel order, through dsg_debug_tap
    (taps take the read-out's chain, as at p = 1)"""
    cfg, flags, adj, node, sc_adj, sc_node = Y.patch_fwd_case(name)
    g = load(f"fwd_patch_{name}.npz")
    shapes = Y.tap_shapes(cfg)
    net = net_for(name).model
    sc = (T(sc_adj), T(sc_node)) if cfg.self_condition else (None, None)
    _, bufs = net.debug_forward(T(adj), T(node), T(flags), T(Y.FWD_C_NOISE), *sc,
                                taps={k: shapes[k][0] * shapes[k][1] for k in ("patch_embed", "read_out")})
    for k in ("patch_embed", "read_out"):
        Tk, Ck = shapes[k]
        got = bufs[k].cpu().numpy().reshape(2 * Tk, Ck)
        if name in Y.PATCH_ROW_SAMPLED:
            e = assert_close(got[Y.inter_rows(2 * Tk)], g["rows/" + k], FWD_RTOL, f"{name} {k}")
        else:
            e = assert_close(got, g["inter/" + k].reshape(2 * Tk, Ck), FWD_RTOL, f"{name} {k}")
        print(f"PATCHFWD {name} tap {k}: rel err {e:.3e} (bar {FWD_RTOL:.0e})")
    assert net._ensure_handle().patch_forms(2) == ("fused" if cfg.patch_size == 2 else "chain", "chain")


def test_p1_handles_report_their_forms():
    """the route report at patch_size 1: the fused kernels where E = 96 has them, the chain when the options are off"""
    from diffusesg_amd.model import build_network
    cfg = Y.CONFIGS["tiny"]()
    net = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda").model
    _, flags, adj, node, _, _ = Y.fwd_case("tiny")
    net(T(adj), T(node), T(flags), T(Y.FWD_C_NOISE))
    h = net._ensure_handle()
    assert h.patch_forms(2) == ("fused", "fused")
    h.set_option("fused_patch_embed", 0)
    h.set_option("fused_readout", 0)
    net(T(adj), T(node), T(flags), T(Y.FWD_C_NOISE))
    assert h.patch_forms(2) == ("chain", "chain")


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("tag,T_,solver,churn", Y.PATCH_SAMPLER_RUNS)
def test_sampler_trajectory_vs_reference(tag, T_, solver, churn, use_graph):
    g = load("sampler_patch.npz")
    cfg = Y.PATCH_CONFIGS["tiny_p2"]()
    flags, ia, inn, na, nn, coin_vals = Y.sampler_case(cfg, T_, 4, Y.SAMPLER_VALID, 3, f"smp_patch/{tag}", solver)
    smp = make_sampler(T_, solver, churn, use_graph)
    coins = (coin_vals < 0.5).astype(np.uint8)
    oa, on = smp.sample(net_for("tiny_p2"), T(flags), init_adjs=T(ia), init_nodes=T(inn), churn_noise=(T(na), T(nn)), coins=coins,
                        flag_node_multi_channel=True, flag_adj_multi_channel=True, num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj)
    ea, en = assert_close(oa.numpy(), g[f"{tag}_adj"], 1e-4, f"{tag} adj"), assert_close(on.numpy(), g[f"{tag}_node"], 1e-4, f"{tag} node")
    print(f"PATCHFWD sampler {tag} graph={int(use_graph)}: rel err adj {ea:.3e} node {en:.3e} (bar 1e-04)")
    used = int(g[f"{tag}_coins_used"])
    assert smp.last_stats["precond_calls"] == used
    assert smp.last_stats["net_forwards"] == used + int(coins[:used].sum())
    if use_graph:
        assert smp.last_stats["graph_replays"] == smp.last_stats["net_forwards"]


def test_sample_known_holds_entries_bit_for_bit():
    cfg = Y.PATCH_CONFIGS["tiny_p2"]()
    B, T_, n = 4, 8, cfg.max_node_num
    flags, ia, inn, na, nn, cv = Y.sampler_case(cfg, T_, B, Y.SAMPLER_VALID, 3, "smp_patch/known", "heun")
    ka, kn = Y.gt_case(cfg, B, Y.SAMPLER_VALID)
    sa, sn = (B, cfg.c_adj, n, n), (B, n, cfg.c_node)
    ma = T((W.uniform01(3, "smp_patch/mask/adj", int(np.prod(sa))) < 0.5).astype(np.uint8).reshape(sa))
    mn = T((W.uniform01(3, "smp_patch/mask/node", int(np.prod(sn))) < 0.5).astype(np.uint8).reshape(sn))
    smp = make_sampler(T_, clip=False)
    oa, on = smp.sample_known(net_for("tiny_p2"), T(flags), T(ka), T(kn), ma, mn, coins=(cv < 0.5).astype(np.uint8), init_adjs=T(ia),
                              init_nodes=T(inn), churn_noise=(T(na), T(nn)), num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj,
                              return_device=True)
    f = T(flags).bool()
    va, vn = (f[:, None, :, None] & f[:, None, None, :]).expand(sa), f[:, :, None].expand(sn)
    held_a, held_n = ma.bool() & va, mn.bool() & vn
    assert held_a.any() and held_n.any()
    assert torch.equal(oa[held_a], T(ka)[held_a]) and torch.equal(on[held_n], T(kn)[held_n])
    assert torch.all(oa[~va] == 0) and torch.all(on[~vn] == 0) and torch.isfinite(oa).all() and torch.isfinite(on).all()
    assert not torch.equal(oa[~ma.bool() & va], T(ka)[~ma.bool() & va])


def test_options_off_and_refused():
    net = net_for("small_p2").model
    h = net._ensure_handle()
    cfg, flags, adj, node, sc_adj, sc_node = Y.patch_fwd_case("small_p2")
    net(T(adj), T(node), T(flags), T(Y.FWD_C_NOISE))
    assert h.get_option("prune_masked") == 0 and h.get_option("dedup_masked") == 0
    for opt in ("gemm_split", "gemm_bf16", "batch_invariant"):
        with pytest.raises(L.DsgError, match="patch_size"):
            h.set_option(opt, 1)
        assert h.get_option(opt) == 0
    # the refusal left the handle as it was
    oa, on = net(T(adj), T(node), T(flags), T(Y.FWD_C_NOISE))
    assert_close(oa.cpu().numpy(), load("fwd_patch_small_p2.npz")["nosc_adj_out"], FWD_RTOL, "after the refusals")
    assert h.L.dsg_workspace_bytes(h.raw, 2) > 4 * 2 * 3 * 16 * 16 * 96       # the read-out chain's B N^2 E buffers are part of it


def test_training_entries_refused_before_anything_runs():
    """the refusal comes ahead of every other argument check, so null arguments reach nothing"""
    h = net_for("tiny_p2").model._ensure_handle()
    lib = h.L
    scfg, ocfg = L.make_sampler_cfg(8, "euler", S_churn=0.0), L.DsgOdeCfg()
    calls = {
        "dsg_train_grads": lambda: lib.dsg_train_grads(h.raw, 2, *([None] * 10), 0, None, None, None),
        "dsg_train_step_grads": lambda: lib.dsg_train_step_grads(h.raw, 2, *([None] * 9), 1.0, 1.0, 0.0, 0, *([None] * 4), 0, None, None, None),
        "dsg_train_self_cond": lambda: lib.dsg_train_self_cond(h.raw, 2, *([None] * 7)),
        "dsg_precond_vjp": lambda: lib.dsg_precond_vjp(h.raw, 2, *([None] * 8), L.GRAD_FN(), None, *([None] * 5)),
        "dsg_ode_run": lambda: lib.dsg_ode_run(h.raw, C.byref(scfg), C.byref(ocfg), 2, *([None] * 12)),
    }
    for name, call in calls.items():
        assert call() == L.DSG_ERR_INVALID, name
        msg = lib.dsg_last_error(h.raw).decode()
        assert "patch_size" in msg and name in msg, msg


def test_odd_coarsest_resolution_is_refused_at_create():
    """COCO's N = 40 at p = 2 on three levels reaches 5 x 5, where the reference's own PatchBreakup fails"""
    cfg = S.ModelConfig(max_node_num=40, c_adj=3, c_node=12, depths=(1, 2, 6), num_heads=(3, 6, 12), window_size=10, patch_size=2)
    with pytest.raises(L.DsgError, match="odd"):
        L.Handle(cfg)
    ok = L.Handle(Y.PATCH_CONFIGS["coco2_p2"]())          # two levels: 20 -> 10
    ok.close()


def test_environment_default_precision_mode_is_refused_and_can_be_cleared(monkeypatch):
    """a p > 1 handle created under DSG_GEMM_BF16=1: the first forward is refused by the plan check with a message naming patch_size;
    unrelated options can still be set, and clearing the mode makes the handle work"""
    from diffusesg_amd.model import build_network
    monkeypatch.setenv("DSG_GEMM_BF16", "1")
    cfg, flags, adj, node, sc_adj, sc_node = Y.patch_fwd_case("tiny_p2")
    net = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda").model
    with pytest.raises(L.DsgError, match="patch_size"):          # (the handle is created by the first call: the variable is still set)
        net(T(adj), T(node), T(flags), T(Y.FWD_C_NOISE))
    monkeypatch.delenv("DSG_GEMM_BF16")
    h = net._ensure_handle()
    assert h.get_option("gemm_bf16") == 1
    h.set_option("loop_graph", 0)            # an unrelated option is not held hostage by the stored mode
    h.set_option("loop_graph", 1)
    h.set_option("gemm_bf16", 0)
    oa, on = net(T(adj), T(node), T(flags), T(Y.FWD_C_NOISE))
    assert_close(oa.cpu().numpy(), load("fwd_patch_tiny_p2.npz")["nosc_adj_out"], FWD_RTOL, "after clearing the mode")
