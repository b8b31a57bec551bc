"""GPU: the training form at patch_size 2 and 4 (dsg_train_enable_patch) against tests/golden/train_patch.npz -- the
reference's own modules under its autograd (tools/gen_patch_train_golden.py): training-step gradients of every parameter, the Adam
step, input gradients on both paths of dsg_precond_vjp, the probability-flow ODE; plus the entry's own properties: dsg_train_self_cond
against the sampling path, poisoned workspaces, the handle state and its refusals, p = 1 bit for bit with the state on and off, and
the checkpoint round trip.  The bars are those of the p = 1 tests of the same quantities (test_hip_parity.py, test_input_grad.py,
test_ode.py, test_workspace_poison.py)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from diffusesg_amd import lib as L
from diffusesg_amd import synth as Y
from diffusesg_amd import weights as W
from util import FWD_RTOL, assert_close, load, rel_err

pytestmark = pytest.mark.gpu

GRAD_RTOL = 2e-4
ODE_MARGIN = 16.0
RPB = "relative_position_bias_table"


def T(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x))


def P(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def fresh_net(name, seed=0, alloc_fill=0):
    from diffusesg_amd.model import build_network
    cfg = (Y.PATCH_CONFIGS.get(name) or Y.CONFIGS[name])()
    net = build_network(cfg, W.synth_state_dict(cfg, seed), device="cuda")
    if alloc_fill:
        net.model._handle = L.Handle(cfg)
        net.model._handle.set_option("debug_alloc_fill", alloc_fill)
        net.model._ensure_handle()
    return net


@functools.lru_cache(maxsize=None)
def net_for(name):
    return fresh_net(name)


def _squeeze(cfg, a, n):
    if a is None:
        return None, None
    return (a[:, 0] if cfg.c_adj == 1 else a), (n[..., 0] if cfg.c_node == 1 else n)


def _objective(case):
    from diffusesg_amd.train import NodeAdjEDMObjectiveGeneratorHip, NodeAdjRainbowLossHip
    cfg, flags, clean_adj, clean_node, rnd, eps_adj, eps_node, coin = Y.patch_train_case(case)
    gen = NodeAdjEDMObjectiveGeneratorHip(precond="edm", sigma_dist="edm", other_params=None, dev="cuda", symmetric_noise=False)
    loss_func = NodeAdjRainbowLossHip(edge_loss_weight=1.0, node_loss_weight=1.0, flag_reweight=False, objective="edm")
    return cfg, flags, clean_adj, clean_node, rnd, eps_adj, eps_node, coin, gen, loss_func


def _with_coin(coin, fn):
    real = np.random.rand
    np.random.rand = lambda: coin
    try:
        return fn()
    finally:
        np.random.rand = real


@pytest.mark.parametrize("case", list(Y.PATCH_TRAIN_CASES))
def test_training_step_gradients_vs_reference_autograd(case):
    """test_hip_parity.py's bars for its tiny cases: outputs 2e-5, loss 2e-4, every parameter's strided sample 2e-4 of its max, norms
    and the total norm 1e-4; the set of gradient names equals the reference's"""
    from diffusesg_amd.train import train_step_grads
    g = load("train_patch.npz")
    cfg, flags, clean_adj, clean_node, rnd, eps_adj, eps_node, coin, gen, loss_func = _objective(case)
    model = net_for(Y.PATCH_TRAIN_CASES[case][0])
    na, nx, cond, ta, tx, (c_skip, c_out, c_in, c_noise, sigmas, weights) = gen.get_input_output(
        T(clean_adj), T(clean_node), T(flags), rnd_sigma=T(rnd), noise=(T(eps_adj), T(eps_node)))
    iou_w = float(g[f"{case}_iou_loss_weight"])
    oa, on, la, ln, grads = _with_coin(float(g[f"{case}_coin"]), lambda: train_step_grads(
        model, loss_func, na, nx, T(flags), sigmas, T(clean_adj), T(clean_node), weights, iou_loss_weight=iou_w))
    assert model.model._handle.patch_training_enabled(), "calling the entry point is the opt-in"
    assert_close(oa.cpu().numpy().reshape(g[f"{case}_pred_adj"].shape), g[f"{case}_pred_adj"], 2e-5, "preconditioned output adj")
    assert_close(on.cpu().numpy().reshape(g[f"{case}_pred_node"].shape), g[f"{case}_pred_node"], 2e-5, "preconditioned output node")
    loss = float(la.mean() + ln.mean())
    print(f"PATCHTRAIN {case}: loss {loss:.6f} (ref {float(g[f'{case}_loss']):.6f})")
    assert abs(loss - float(g[f"{case}_loss"])) <= 2e-4 * abs(float(g[f"{case}_loss"]))
    names = [str(k) for k in g[f"{case}_gparam_names"]]
    assert set(k[len("model."):] for k in names) == set(grads.keys())
    tot, worst, worst_n = 0.0, (0.0, ""), (0.0, "")
    for k, ref_norm in zip(names, g[f"{case}_gparam_norms"]):
        key = k[len("model."):]
        mine = grads[key].cpu().numpy().reshape(-1)
        ref = g[f"{case}_gparam/{k}"]
        stride = max(1, -(-mine.size // Y.PATCH_TRAIN_MAX_SAMPLE))
        worst = max(worst, (float(np.abs(mine[::stride] - ref).max()) / max(float(np.abs(ref).max()), 1e-12), key))
        nrm = float(np.sqrt((mine.astype(np.float64) ** 2).sum()))
        worst_n = max(worst_n, (abs(nrm - float(ref_norm)) / (float(ref_norm) + 1e-5), key))
        assert abs(nrm - float(ref_norm)) <= 1e-4 * float(ref_norm) + 1e-9, (key, nrm, float(ref_norm))
        tot += nrm ** 2
    print(f"PATCHTRAIN {case}: worst sample error {worst[0]:.3e} of max ({worst[1]}), worst norm error {worst_n[0]:.3e} ({worst_n[1]})")
    assert worst[0] <= 2e-4, worst
    assert abs(np.sqrt(tot) - float(g[f"{case}_total_grad_norm"])) <= 1e-4 * float(g[f"{case}_total_grad_norm"])


def test_training_iteration_adam_step_vs_reference():
    """train_one_iteration against the parameters after the reference's Adam step, at test_hip_parity.py's bar; a second iteration sees
    the updated weights"""
    from diffusesg_amd.train import AdamHip, train_one_iteration
    g = load("train_patch.npz")
    case = Y.PATCH_TRAIN_ADAM_CASE
    cfg, flags, clean_adj, clean_node, rnd, eps_adj, eps_node, coin, gen, loss_func = _objective(case)
    model = fresh_net(Y.PATCH_TRAIN_CASES[case][0])
    opt = AdamHip(model, lr=2.0e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    opt_grads = {}
    real_step = opt.step
    opt.step = lambda grads, max_grad_norm=10.0: (opt_grads.update(grads), real_step(grads, max_grad_norm=max_grad_norm))[1]
    it = lambda: train_one_iteration(model, gen, loss_func, opt, None, T(clean_adj), T(clean_node), T(flags), iou_loss_weight=1.0,
                                     rnd_sigma=T(rnd), noise=(T(eps_adj), T(eps_node)))
    loss, ra, rn, sg, total_norm = _with_coin(coin, it)
    opt.step = real_step
    assert abs(float(loss) - float(g[f"{case}_loss"])) <= 2e-4 * abs(float(g[f"{case}_loss"]))
    assert abs(total_norm - float(g[f"{case}_total_grad_norm"])) <= 1e-4 * float(g[f"{case}_total_grad_norm"])
    for k, p_ in model.model.named_parameters():
        mine = p_.data.cpu().numpy().reshape(-1)
        ref = g[f"{case}_param_after/model.{k}"]
        stride = max(1, -(-mine.size // 256))
        err = np.abs(mine[::stride] - ref)
        real_g = np.abs(opt_grads[k].cpu().numpy().reshape(-1)[::stride]) > 1e-6   # (see test_hip_parity.py: Adam's first step is sign-like)
        assert err[real_g].max(initial=0.0) <= 2e-7 + 2e-3 * 2.0e-4, (k, float(err[real_g].max()))
        assert err.max() <= 2.02e-4, (k, float(err.max()))
    loss2, *_ = _with_coin(coin, it)
    assert float(loss2) != float(loss) and np.isfinite(float(loss2))


@functools.lru_cache(maxsize=None)
def _vjp(tag, path="direct"):
    from diffusesg_amd import guide
    name, _valid, _sig, _sc, cot = Y.PATCH_INPUT_GRAD_CASES[tag]
    cfg, flags, adj, node, sig, sc_adj, sc_node, g_adj, g_node = Y.patch_input_grad_case(tag)
    net = net_for(name)
    a, n = _squeeze(cfg, adj, node)
    sa, sn = _squeeze(cfg, sc_adj, sc_node)
    kw = dict(self_cond_adjs=T(sa), self_cond_nodes=T(sn), coin=False)
    if cot == "overlap":
        out = net.value_and_input_grad(T(a), T(n), T(flags), T(sig), loss_fn=guide.box_overlap_loss(), **kw)
    elif path == "direct":
        ga, gn = _squeeze(cfg, g_adj, g_node)
        out = net.value_and_input_grad(T(a), T(n), T(flags), T(sig), grad_outputs=(T(ga), T(gn)), **kw)
    else:
        ga, gn = (T(v).cuda() for v in _squeeze(cfg, g_adj, g_node))
        out = net.value_and_input_grad(T(a), T(n), T(flags), T(sig), loss_fn=lambda Da, Dn: (ga * Da).sum() + (gn * Dn).sum(), **kw)
    torch.cuda.synchronize()
    return tuple(None if v is None else v.cpu().numpy() for v in out)


@pytest.mark.parametrize("tag", list(Y.PATCH_INPUT_GRAD_CASES))
def test_input_gradients_vs_reference_autograd(tag):
    """test_input_grad.py's bars for its tiny cases: D at 1e-4 of max|ref|, both gradients at 2e-4 of each tensor's max, the adjacency
    gradient at padded pairs too, exact zeros at padded nodes, the loss at 2e-4"""
    g = load("train_patch.npz")
    Da, Dn, loss, ga, gn = _vjp(tag)
    e_da, e_dn = rel_err(Da, g[f"igrad/{tag}/D_adj"]), rel_err(Dn, g[f"igrad/{tag}/D_node"])
    e_ga, e_gn = rel_err(ga, g[f"igrad/{tag}/grad_adj"]), rel_err(gn, g[f"igrad/{tag}/grad_node"])
    print(f"PATCHTRAIN input grad {tag}: D adj {e_da:.3e} node {e_dn:.3e} | grad adj {e_ga:.3e} node {e_gn:.3e}")
    assert e_da <= FWD_RTOL and e_dn <= FWD_RTOL, (e_da, e_dn)
    assert e_ga <= GRAD_RTOL and e_gn <= GRAD_RTOL, (e_ga, e_gn)
    cfg, flags = Y.patch_input_grad_case(tag)[:2]
    f = flags.astype(bool)
    pad = np.broadcast_to(~(f[:, :, None] & f[:, None, :])[:, None], (len(f), cfg.c_adj) + (cfg.max_node_num,) * 2)
    ref_pad = g[f"igrad/{tag}/grad_adj"].reshape(pad.shape)[pad]
    assert np.abs(ref_pad).max() > 0, "the fixture's adjacency gradient at padded pairs is zero"
    assert np.abs(ga.reshape(pad.shape)[pad] - ref_pad).max() / np.abs(g[f"igrad/{tag}/grad_adj"]).max() <= GRAD_RTOL
    assert (gn.reshape(len(f), cfg.max_node_num, -1)[~f] == 0).all(), "node gradient of padded nodes"
    if loss is not None:
        assert abs(float(loss) - float(g[f"igrad/{tag}/loss"])) <= 2e-4 * abs(float(g[f"igrad/{tag}/loss"]))


def test_callback_path_equals_direct_path():
    d, c = _vjp("tiny_p2_sc", "direct"), _vjp("tiny_p2_sc", "callback")
    for k in (0, 1, 3, 4):
        assert np.array_equal(d[k], c[k]), f"output {k} differs between the callback and the direct path"
    assert d[2] is None and c[2] is not None


def test_ode_against_the_float64_fixture():
    """test_ode.py's bars: 16 x the discrepancy of the reference's own float32 run against its float64 run, recorded for this case"""
    from diffusesg_amd import ode
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    g = load("train_patch.npz")
    cfg, flags, adj, node, p_adj, p_node = Y.patch_ode_case()
    steps, solver = Y.PATCH_ODE_RUN
    smp = NodeAdjEDMSamplerHip(num_steps=steps, solver=solver, S_churn=0, self_condition=cfg.self_condition)
    r = ode.log_likelihood(net_for(Y.PATCH_ODE_NET), smp, T(adj), T(node), T(flags), probes=(T(p_adj), T(p_node)))
    torch.cuda.synchronize()
    flat = lambda a, n: np.concatenate([np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v, np.float64).reshape(len(flags), -1)
                                        for v in (a, n)], 1)
    lat_ref, n_ref, lp_ref = flat(g["ode/latent_adj"], g["ode/latent_node"]), g["ode/n"], g["ode/logp"]
    e_lat = np.abs(flat(*r["latent"]) - lat_ref).max() / np.abs(lat_ref).max()
    e_n = np.abs(r["net_trace"] - n_ref).max() / np.abs(n_ref).max()
    e_lp = (np.abs(r["logp"] - lp_ref) / np.abs(lp_ref)).max()
    bars = {k: ODE_MARGIN * float(g[f"ode/worst_{k}"]) for k in ("latent", "n", "logp")}
    print(f"PATCHTRAIN ode: latent {e_lat:.3e} (bar {bars['latent']:.3e}) | n_k {e_n:.3e} (bar {bars['n']:.3e}) | logp {e_lp:.3e} (bar {bars['logp']:.3e})")
    assert r["net_trace"].shape == n_ref.shape
    assert e_lat <= bars["latent"] and e_n <= bars["n"] and e_lp <= bars["logp"], (e_lat, e_n, e_lp, bars)


def test_train_self_cond_equals_the_sampling_path():
    """dsg_train_self_cond (training form) against dsg_precond (sampling path, no self-conditioning input, coin not fired) at FWD_RTOL"""
    cfg, flags, adj, node, sig, *_ = Y.patch_input_grad_case("tiny_p2_sc")
    net = net_for("tiny_p2")
    h = net.model._ensure_handle()
    h.enable_patch_training()
    a, x, fl, sg = (T(v).cuda() for v in (adj, node, flags, sig))
    sa, sx = torch.empty_like(a), torch.empty_like(x)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    h.check(h.L.dsg_train_self_cond(h.raw, len(flags), P(a), P(x), P(fl), P(sg), P(sa), P(sx), st), "dsg_train_self_cond")
    Da, Dn = _with_coin(0.9, lambda: net(T(adj), T(node), T(flags), T(sig)))
    e_a, e_n = rel_err(sa.cpu().numpy(), Da.cpu().numpy()), rel_err(sx.cpu().numpy(), Dn.cpu().numpy())
    print(f"PATCHTRAIN self_cond vs dsg_precond: adj {e_a:.3e} node {e_n:.3e}")
    assert e_a <= FWD_RTOL and e_n <= FWD_RTOL
    f = flags.astype(bool)
    assert (sx.cpu().numpy()[~f] == 0).all() and (sa.cpu().numpy()[np.broadcast_to(~(f[:, :, None] & f[:, None, :])[:, None], sa.shape)] == 0).all()


def _poison_run(net, case):
    from diffusesg_amd.train import train_step_grads
    cfg, flags, clean_adj, clean_node, rnd, eps_adj, eps_node, coin, gen, loss_func = _objective(case)
    na, nx, cond, ta, tx, (c_skip, c_out, c_in, c_noise, sigmas, weights) = gen.get_input_output(
        T(clean_adj), T(clean_node), T(flags), rnd_sigma=T(rnd), noise=(T(eps_adj), T(eps_node)))
    oa, on, la, ln, grads = _with_coin(0.1, lambda: train_step_grads(model=net, loss_func=loss_func, net_input_a=na, net_input_x=nx,
                                                                     node_flags=T(flags), sigmas=sigmas, net_target_a=T(clean_adj),
                                                                     net_target_x=T(clean_node), loss_weight=weights, iou_loss_weight=1.0))
    torch.cuda.synchronize()
    keys = sorted(grads)
    return ["D_adj", "D_node", "loss_adj", "loss_node"] + keys, [oa, on, la, ln] + [grads[k] for k in keys]


@pytest.mark.parametrize("case", ["tiny_p2_sc", "small_p4_sc"])
def test_outputs_do_not_depend_on_stale_workspace_memory(case):
    """fresh handles whose every scratch buffer is filled on allocation ("debug_alloc_fill" 2 and 3) give the plain handle's bits; the
    relative-position-bias gradients (float atomics) are held to test_workspace_poison.py's bar, 8 x max(the difference of two plain
    runs, 2^-20) of their maximum"""
    name = Y.PATCH_TRAIN_CASES[case][0]
    names, ref = _poison_run(net_for(name), case)
    _, again = _poison_run(net_for(name), case)
    for fill in (2, 3):
        _, got = _poison_run(fresh_net(name, alloc_fill=fill), case)
        for k, r, a2, v in zip(names, ref, again, got):
            if k.endswith(RPB):
                s = max(float(r.abs().max()), 1e-30)
                d_plain, d = float((a2 - r).abs().max()) / s, float((v - r).abs().max()) / s
                assert d <= 8 * max(d_plain, 2.0 ** -20), f"{k} under fill {fill}: {d:.2e} of its maximum (two plain runs: {d_plain:.2e})"
            else:
                assert torch.equal(v, r), f"{k} differs under debug_alloc_fill {fill}"


def _null_calls(h):
    lib = h.L
    scfg, ocfg = L.make_sampler_cfg(8, "euler", S_churn=0.0), L.DsgOdeCfg()
    return {
        "dsg_train_grads": lambda: lib.dsg_train_grads(h.raw, 2, *([None] * 10), 0, None, None, None),
        "dsg_train_step_grads": lambda: lib.dsg_train_step_grads(h.raw, 2, *([None] * 9), 1.0, 1.0, 0.0, 0, *([None] * 4), 0, None, None, None),
        "dsg_train_self_cond": lambda: lib.dsg_train_self_cond(h.raw, 2, *([None] * 7)),
        "dsg_precond_vjp": lambda: lib.dsg_precond_vjp(h.raw, 2, *([None] * 8), L.GRAD_FN(), None, *([None] * 5)),
        "dsg_ode_run": lambda: lib.dsg_ode_run(h.raw, C.byref(scfg), C.byref(ocfg), 2, *([None] * 12)),
    }


def test_handle_state_and_refusals():
    h = fresh_net("tiny_p2").model._ensure_handle()
    assert not h.patch_training_enabled()
    for name, call in _null_calls(h).items():          # a fresh handle refuses, ahead of every other check, pointing at the new entry
        assert call() == L.DSG_ERR_INVALID, name
        msg = h.L.dsg_last_error(h.raw).decode()
        assert "patch_size" in msg and name in msg and "dsg_train_enable_patch" in msg, msg
    h.enable_patch_training()
    assert h.patch_training_enabled() and h.L.dsg_train_patch_enabled(h.raw) == 1
    for name, call in _null_calls(h).items():          # enabled: the refusal is gone, the null arguments are what is refused now
        assert call() == L.DSG_ERR_INVALID, name
        assert "patch_size" not in h.L.dsg_last_error(h.raw).decode()
    h.set_train_precision("bf16")
    for name, call in _null_calls(h).items():          # enabled + bf16: refused, naming both
        assert call() == L.DSG_ERR_INVALID, name
        msg = h.L.dsg_last_error(h.raw).decode()
        assert "patch_size" in msg and name in msg and "dsg_train_enable_patch" in msg and "DSG_TRAIN_BF16" in msg, msg
    h.set_train_precision("fp32")
    h.enable_patch_training(False)
    assert not h.patch_training_enabled()
    assert _null_calls(h)["dsg_train_grads"]() == L.DSG_ERR_INVALID and "patch_size" in h.L.dsg_last_error(h.raw).decode()
    assert h.L.dsg_train_patch_enabled(None) == 0 and h.L.dsg_train_enable_patch(None, 1) == L.DSG_ERR_INVALID


def test_patch_size_one_is_bit_for_bit_with_the_state_on_and_off():
    from diffusesg_amd.train import NodeAdjEDMObjectiveGeneratorHip, NodeAdjRainbowLossHip, train_step_grads
    cfg, flags, clean_adj, clean_node, rnd, eps_adj, eps_node, coin = Y.train_case("tiny")
    gen = NodeAdjEDMObjectiveGeneratorHip(precond="edm", sigma_dist="edm", other_params=None, dev="cuda", symmetric_noise=False)
    loss_func = NodeAdjRainbowLossHip(edge_loss_weight=1.0, node_loss_weight=1.0, flag_reweight=False, objective="edm")
    na, nx, cond, ta, tx, (c_skip, c_out, c_in, c_noise, sigmas, weights) = gen.get_input_output(
        T(clean_adj), T(clean_node), T(flags), rnd_sigma=T(rnd), noise=(T(eps_adj), T(eps_node)))
    model = fresh_net("tiny")
    h = model.model._ensure_handle()
    runs = []
    for on in (False, True):
        h.enable_patch_training(on)
        assert h.patch_training_enabled() == on
        out = _with_coin(0.3, lambda: train_step_grads(model, loss_func, na, nx, T(flags), sigmas, T(clean_adj), T(clean_node), weights,
                                                       iou_loss_weight=1.0))
        torch.cuda.synchronize()
        runs.append(out)
    for k in range(4):
        assert torch.equal(runs[0][k], runs[1][k])
    for k in runs[0][4]:
        if not k.endswith(RPB):                          # (float atomics: not bit-stable between any two runs)
            assert torch.equal(runs[0][4][k], runs[1][4][k]), k


def test_checkpoint_round_trip(tmp_path):
    """one iteration at tiny_p2 -> the checkpoint the reference's trainer writes -> a fresh network: dsg_precond outputs bit for bit"""
    from diffusesg_amd import io as dio
    from diffusesg_amd.train import AdamHip, train_one_iteration
    case = "tiny_p2"
    cfg, flags, clean_adj, clean_node, rnd, eps_adj, eps_node, coin, gen, loss_func = _objective(case)
    model = fresh_net("tiny_p2")
    opt = AdamHip(model, lr=1e-3)
    loss = _with_coin(coin, lambda: train_one_iteration(model, gen, loss_func, opt, None, T(clean_adj), T(clean_node), T(flags), iou_loss_weight=1.0,
                                                        rnd_sigma=T(rnd), noise=(T(eps_adj), T(eps_node))))[0]
    assert np.isfinite(float(loss))
    path = dio.save_checkpoint(str(tmp_path / "tiny_p2_00001.pth"), model, [], 1, np.float64(loss), np.float64(loss), {"model": {"name": "diffuse_sg"}})
    ckp = dio.load_checkpoint(path)
    assert tuple(ckp["model"]["model.patch_embed.proj.weight"].shape) == (cfg.embed_dim, cfg.in_chans, 2, 2)
    assert tuple(ckp["model"]["model.read_out.0.weight"].shape) == (cfg.embed_dim, cfg.embed_dim, 2, 2)
    _, fl, adj, node, sig, sc_adj, sc_node, _, _ = Y.patch_input_grad_case("tiny_p2_sc")
    call = lambda net: _with_coin(0.9, lambda: net(T(adj), T(node), T(fl), T(sig), T(sc_adj), T(sc_node)))
    want = [t.clone() for t in call(model)]
    fresh = fresh_net("tiny_p2", seed=1)
    dio.load_model(ckp, fresh, "model")
    got = call(fresh)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    init = call(fresh_net("tiny_p2"))
    assert float((init[0] - want[0]).abs().max()) > 1e-5, "training moved nothing"
