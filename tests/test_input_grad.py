"""GPU: input gradients of the preconditioned denoiser (dsg_precond_vjp, NodeAdjPrecondHip.value_and_input_grad) against
tests/golden/input_grad.npz -- the reference's own NodeAdjPrecond under its autograd with the noisy inputs requiring grad
(tools/gen_input_grad_golden.py) -- plus the properties of the entry: callback path == direct path, determinism, D identical to
dsg_train_self_cond, error handling, no trace left in the training entries, and a directional finite difference through the
library's own forward.  Every case runs once per session (module cache); measured figures: profiles/train_kernel_errors.md
("Input gradients")."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from diffusesg_amd import synth as Y
from diffusesg_amd import weights as W
from util import FWD_RTOL, load, rel_err

pytestmark = pytest.mark.gpu

GRAD_RTOL = 2e-4   # the whole-network gradient bar of test_training_step_gradients_vs_reference_autograd
T = torch.from_numpy


@functools.lru_cache(maxsize=None)
def _net(name):
    from diffusesg_amd.model import build_network
    cfg = Y.CONFIGS[name]()
    return build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")


def _t(x):
    return None if x is None else T(np.ascontiguousarray(x))


def _squeeze(cfg, a, n):
    if a is None:
        return None, None
    return (a[:, 0] if cfg.c_adj == 1 else a), (n[..., 0] if cfg.c_node == 1 else n)


@functools.lru_cache(maxsize=None)
def _run(tag, path="direct"):
    """(D_adj, D_node, loss, grad_adj, grad_node) as numpy for a fixture case; path: 'direct' (grad_outputs), 'callback' (loss_fn)"""
    from diffusesg_amd import guide
    name, _valid, _sig, _sc, cot, _stride = Y.INPUT_GRAD_CASES[tag]
    cfg, flags, adj, node, sig, sc_adj, sc_node, g_adj, g_node, _ = Y.input_grad_case(tag)
    net = _net(name)
    a, n = _squeeze(cfg, adj, node)
    sa, sn = _squeeze(cfg, sc_adj, sc_node)
    kw = dict(self_cond_adjs=_t(sa), self_cond_nodes=_t(sn), coin=False)
    if cot == "overlap":
        out = net.value_and_input_grad(_t(a), _t(n), _t(flags), _t(sig), loss_fn=guide.box_overlap_loss(), **kw)
    elif path == "direct":
        ga, gn = _squeeze(cfg, g_adj, g_node)
        out = net.value_and_input_grad(_t(a), _t(n), _t(flags), _t(sig), grad_outputs=(_t(ga), _t(gn)), **kw)
    else:
        ga, gn = (_t(v).cuda() for v in _squeeze(cfg, g_adj, g_node))
        out = net.value_and_input_grad(_t(a), _t(n), _t(flags), _t(sig), loss_fn=lambda Da, Dn: (ga * Da).sum() + (gn * Dn).sum(), **kw)
    torch.cuda.synchronize()
    return tuple(None if v is None else v.cpu().numpy() for v in out)


@pytest.mark.parametrize("tag", list(Y.INPUT_GRAD_CASES))
def test_input_gradients_vs_reference_autograd(tag):
    """D at the forward bar (1e-4 of max|ref|), dL/d adjs and dL/d nodes at 2e-4 of each tensor's max, every case of the fixture.  The
    adjacency gradient is compared at padded pairs too: the network reads the unmasked adjacency input, so it is not zero there (and
    the test insists the fixture's is not).  VG / COCO-Stuff run at B = 1."""
    g = load("input_grad.npz")
    stride = Y.INPUT_GRAD_CASES[tag][5]
    Da, Dn, loss, ga, gn = _run(tag)
    e_da = rel_err(Da[..., ::stride, ::stride], g[f"{tag}/D_adj"])
    e_dn = rel_err(Dn, g[f"{tag}/D_node"])
    e_ga, e_gn = rel_err(ga, g[f"{tag}/grad_adj"]), rel_err(gn, g[f"{tag}/grad_node"])
    print(f"INPUTGRAD {tag}: D adj {e_da:.3e} node {e_dn:.3e} | grad adj {e_ga:.3e} node {e_gn:.3e}")
    assert e_da <= FWD_RTOL and e_dn <= FWD_RTOL, (e_da, e_dn)
    assert e_ga <= GRAD_RTOL, f"dL/d adjs: {e_ga:.3e}"
    assert e_gn <= GRAD_RTOL, f"dL/d nodes: {e_gn:.3e}"
    cfg, flags = Y.input_grad_case(tag)[:2]
    f = flags.astype(bool)
    pad = np.broadcast_to(~(f[:, :, None] & f[:, None, :])[:, None], (len(f), cfg.c_adj) + (cfg.max_node_num,) * 2)
    if pad.any():
        ref_pad = g[f"{tag}/grad_adj"].reshape(pad.shape)[pad]
        assert np.abs(ref_pad).max() > 0, "the fixture's adjacency gradient at padded pairs is zero"
        err = np.abs(ga.reshape(pad.shape)[pad] - ref_pad).max() / np.abs(g[f"{tag}/grad_adj"]).max()
        assert err <= GRAD_RTOL, f"dL/d adjs at padded pairs: {err:.3e}"
        assert (gn.reshape(len(f), cfg.max_node_num, -1)[~f] == 0).all(), "node gradient of padded nodes"
    if loss is not None:
        assert abs(float(loss) - float(g[f"{tag}/loss"])) <= 2e-4 * abs(float(g[f"{tag}/loss"]))


@pytest.mark.parametrize("tag", ["tiny_sc", "nosc"])
def test_callback_path_equals_direct_path(tag):
    d, c = _run(tag, "direct"), _run(tag, "callback")
    for k in (0, 1, 3, 4):
        assert np.array_equal(d[k], c[k]), f"output {k} differs between the callback and the direct path"
    assert d[2] is None and c[2] is not None


def test_two_calls_are_bit_identical():
    first = _run("small")
    _run.cache_clear()
    second = _run("small")
    for k in (0, 1, 3, 4):
        assert np.array_equal(first[k], second[k]), f"output {k} differs between two calls"


def test_D_is_dsg_train_self_cond_bit_for_bit():
    cfg, flags, adj, node, sig, *_ = Y.input_grad_case("tiny_none")
    net = _net("tiny")
    h = net.model._ensure_handle()
    a, x, fl, sg = (_t(v).cuda() for v in (adj, node, flags, sig))
    oa, on = torch.empty_like(a), torch.empty_like(x)
    p = lambda t: C.c_void_p(t.data_ptr())
    h.check(h.L.dsg_train_self_cond(h.raw, len(flags), p(a), p(x), p(fl), p(sg), p(oa), p(on), None), "dsg_train_self_cond")
    torch.cuda.synchronize()
    Da, Dn = _run("tiny_none")[:2]
    assert np.array_equal(Da, oa.cpu().numpy()) and np.array_equal(Dn, on.cpu().numpy())


def test_raising_loss_fn_surfaces_and_the_handle_stays_usable():
    cfg, flags, adj, node, sig, sc_adj, sc_node, g_adj, g_node, _ = Y.input_grad_case("tiny_sc")
    net = _net("tiny")

    class Boom(Exception):
        pass

    def bad(Da, Dn):
        raise Boom("from loss_fn")
    with pytest.raises(Boom, match="from loss_fn"):
        net.value_and_input_grad(_t(adj), _t(node), _t(flags), _t(sig), loss_fn=bad, self_cond_adjs=_t(sc_adj), self_cond_nodes=_t(sc_node),
                                 coin=False)
    out = net.value_and_input_grad(_t(adj), _t(node), _t(flags), _t(sig), grad_outputs=(_t(g_adj), _t(g_node)), self_cond_adjs=_t(sc_adj),
                                   self_cond_nodes=_t(sc_node), coin=False)
    torch.cuda.synchronize()
    ref = _run("tiny_sc")
    assert np.array_equal(out[3].cpu().numpy(), ref[3]) and np.array_equal(out[4].cpu().numpy(), ref[4])


def test_status_codes():
    """fn and grad_D both given, or neither: DSG_ERR_INVALID; a nonzero callback return: DSG_ERR_INVALID; a null tensor: DSG_ERR_INVALID;
    before finalize: DSG_ERR_STATE"""
    from diffusesg_amd import lib as L
    cfg, flags, adj, node, sig, *_ = Y.input_grad_case("tiny_none")
    net = _net("tiny")
    h = net.model._ensure_handle()
    a, x, fl, sg = (_t(v).cuda() for v in (adj, node, flags, sig))
    oa, on, ga, gn = torch.empty_like(a), torch.empty_like(x), torch.zeros_like(a), torch.zeros_like(x)
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    calls = []
    ok_fn = L.GRAD_FN(lambda *args: calls.append(args) or 0)
    bad_fn = L.GRAD_FN(lambda *args: 7)

    def vjp(gd_a, gd_n, fn, adj_=a):
        return h.L.dsg_precond_vjp(h.raw, len(flags), p(adj_), p(x), p(fl), p(sg), None, None, p(gd_a), p(gd_n), fn, None, p(oa), p(on),
                                   p(ga), p(gn), None)
    assert vjp(ga, gn, ok_fn) == L.DSG_ERR_INVALID and not calls, "both"
    assert vjp(None, None, L.GRAD_FN()) == L.DSG_ERR_INVALID, "neither"
    assert vjp(ga, None, L.GRAD_FN()) == L.DSG_ERR_INVALID, "half a cotangent"
    assert vjp(None, None, ok_fn, adj_=None) == L.DSG_ERR_INVALID and not calls, "null input"
    assert vjp(None, None, bad_fn) == L.DSG_ERR_INVALID
    assert b"returned 7" in h.L.dsg_last_error(h.raw)
    fresh = L.Handle(cfg)
    try:
        rc = fresh.L.dsg_precond_vjp(fresh.raw, len(flags), p(a), p(x), p(fl), p(sg), None, None, p(ga), p(gn), L.GRAD_FN(), None, p(oa), p(on),
                                     p(ga), p(gn), None)
        assert rc == -4, f"before finalize: status {rc} (DSG_ERR_STATE is -4)"
    finally:
        fresh.close()
    assert vjp(None, None, ok_fn) == 0 and len(calls) == 1
    torch.cuda.synchronize()


def test_training_entry_is_unchanged_by_a_vjp_call():
    """dsg_train_step_grads after a VJP call on the same handle against a run without it in between: every parameter gradient
    array_equal -- except the relative-position bias tables, which the attention backward accumulates with float atomics in no fixed
    order (profiles/train_kernel_errors.md), so that two plain runs already differ there in the last bits.  Those are held to 8 x the
    larger of the plain-against-plain difference of the same tensor and 16 ulp (2^-20) of the tensor's maximum: a VJP call in between
    may change nothing beyond what the order of the atomics changes anyway."""
    from diffusesg_amd.train import NodeAdjEDMObjectiveGeneratorHip, NodeAdjRainbowLossHip, train_step_grads
    cfg, flags, clean_adj, clean_node, rnd, eps_adj, eps_node, _coin = Y.train_case("tiny")
    net = _net("tiny")
    gen = NodeAdjEDMObjectiveGeneratorHip(precond="edm", sigma_dist="edm", other_params=None, dev="cuda", symmetric_noise=False)
    loss_func = NodeAdjRainbowLossHip(edge_loss_weight=1.0, node_loss_weight=1.0, flag_reweight=False, objective="edm")
    na, nx, _c, ta, tx, (_cs, _co, _ci, _cn, sigmas, weights) = gen.get_input_output(
        T(clean_adj), T(clean_node), T(flags), rnd_sigma=T(rnd), noise=(T(eps_adj), T(eps_node)))

    def step():
        real = np.random.rand
        np.random.rand = lambda: 0.9
        try:
            out = train_step_grads(net, loss_func, na, nx, T(flags), sigmas, T(clean_adj), T(clean_node), weights, iou_loss_weight=1.0)
        finally:
            np.random.rand = real
        torch.cuda.synchronize()
        return {k: v.cpu().numpy().copy() for k, v in out[4].items()}, tuple(v.cpu().numpy().copy() for v in out[:4])
    (plain1, out1), (plain2, _o) = step(), step()
    _run.cache_clear()
    _run("tiny_sc")
    _run("tiny_overlap")
    (after, out3) = step()
    assert all(np.array_equal(a, b) for a, b in zip(out1, out3)), "D or the losses changed"
    tables = [k for k in plain1 if k.endswith("relative_position_bias_table")]
    assert len(tables) == sum(cfg.depths) * 2
    for k in plain1:
        if k in tables:
            s = max(float(np.abs(plain1[k]).max()), 1e-30)
            d_plain, d_vjp = float(np.abs(plain1[k] - plain2[k]).max()) / s, float(np.abs(plain1[k] - after[k]).max()) / s
            print(f"INPUTGRAD unchanged {k}: plain vs plain {d_plain:.2e}, plain vs after a VJP call {d_vjp:.2e} (of the tensor's max)")
            assert d_vjp <= 8 * max(d_plain, 2.0 ** -20), (k, d_vjp, d_plain)
        else:
            assert np.array_equal(plain1[k], plain2[k]), f"{k}: two plain runs differ"
            assert np.array_equal(plain1[k], after[k]), f"{k}: differs after a VJP call"


FD_EPS = 0.03
FD_REF = 1.28e-5        # the reference's own discrepancy (below)
FD_BAR = 4 * FD_REF


def test_directional_finite_difference():
    """L = <a, D(x)> on the `tiny_sc` case, direction v = g / ||g|| (g the VJP result), central difference through the library's own
    forward (dsg_precond_vjp's D, i.e. the training form): |(L(x + eps v) - L(x - eps v)) / (2 eps) - ||g||| / ||g||.
    eps and the bar come from the same experiment on the reference (its float32 NodeAdjPrecond on the CPU, autograd for g, L summed in
    float64): eps = 1e-3 .. 1e-1 gave 1.1e-4, 4.0e-5, 6.3e-5, 1.3e-5, 3e-9 on this case and 4.6e-5, 8.6e-5, 2.6e-5, 5.2e-6, 2.6e-6 on
    `tiny_none` -- rounding noise of L over 2 eps below 0.03, lucky cancellation at 0.1.  eps = 0.03: reference discrepancy 1.28e-5
    (the larger of the two cases); the bar is 4 x that, 5.1e-5, because float32 rounding noise in L is run-dependent."""
    cfg, flags, adj, node, sig, sc_adj, sc_node, g_adj, g_node, _ = Y.input_grad_case("tiny_sc")
    net = _net("tiny")
    _Da, _Dn, _l, ga, gn = _run("tiny_sc")
    nrm = float(np.sqrt((ga.astype(np.float64) ** 2).sum() + (gn.astype(np.float64) ** 2).sum()))
    va, vn = (ga / nrm).astype(np.float32), (gn / nrm).astype(np.float32)

    def L(sign):
        a, n = adj + np.float32(sign * FD_EPS) * va, node + np.float32(sign * FD_EPS) * vn
        Da, Dn = net.value_and_input_grad(_t(a), _t(n), _t(flags), _t(sig), grad_outputs=(_t(g_adj), _t(g_node)), self_cond_adjs=_t(sc_adj),
                                          self_cond_nodes=_t(sc_node), coin=False)[:2]
        return float((T(g_adj).double() * Da.cpu().double()).sum() + (T(g_node).double() * Dn.cpu().double()).sum())
    fd = (L(+1) - L(-1)) / (2 * FD_EPS)
    rel = abs(fd - nrm) / nrm
    print(f"INPUTGRAD finite difference: fd {fd:.7f} vjp {nrm:.7f} rel {rel:.3e} (bar {FD_BAR:.2e}, reference {FD_REF:.2e})")
    assert rel <= FD_BAR
