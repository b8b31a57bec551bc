"""GPU: loss-guided sampling (diffusesg_amd/guide.py) on the tiny (self-conditioning) and nosc (single channels) networks, T = 8.
scale = 0 reproduces `sampler.sample`; every step of a guided run is recomputed in float64 from the recorded trace
(tests/guide_ref.py); known entries arrive bit-exact in every guided estimate; padded entries stay exactly 0; graph b of a seeded
guided batch is the same graph guided alone."""
import functools

import numpy as np
import pytest
import torch

import guide_ref as GR
from diffusesg_amd import synth as Y
from diffusesg_amd import weights as W

pytestmark = pytest.mark.gpu

T8 = 8
TRAJ_RTOL = 1e-4   # the project's T = 8 trajectory bar
VALID = {"tiny": [8, 5, 3], "nosc": [8, 3, 5]}


@functools.lru_cache(maxsize=None)
def _net(name):
    from diffusesg_amd.model import build_network
    cfg = Y.CONFIGS[name]()
    return build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")


def _sampler(name, solver, **kw):
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    cfg = Y.CONFIGS[name]()
    churn = 0 if solver == "dpmpp_2m" else 40
    return NodeAdjEDMSamplerHip(num_steps=T8, solver=solver, S_churn=churn, self_condition=cfg.self_condition, **kw)


def _flags(name):
    return torch.from_numpy(W.synth_flags(len(VALID[name]), Y.CONFIGS[name]().max_node_num, VALID[name]))


def _loss(name):
    from diffusesg_amd import guide
    if name == "tiny":
        return guide.box_overlap_loss()
    return lambda Da, Dn: (Da ** 2).sum() + (Dn ** 3).sum()   # single channels: no boxes


def _np(pair):
    return tuple(v.detach().cpu().numpy() for v in pair)


def _full(name, a, n):
    cfg = Y.CONFIGS[name]()
    B, N = a.shape[0], cfg.max_node_num
    return a.reshape(B, cfg.c_adj, N, N), n.reshape(B, N, cfg.c_node)


@pytest.mark.parametrize("name", ["tiny", "nosc"])
@pytest.mark.parametrize("solver", ["euler", "heun", "dpmpp_2m"])
def test_scale_zero_is_the_plain_sampler(name, solver):
    """scale = 0 against sampler.sample with the same seed and coins, 1e-4 of the result's scale: the loop algebra is the library's;
    what is left is the training-form forward against the sampling-form one"""
    from diffusesg_amd.guide import guided_sample
    cfg = Y.CONFIGS[name]()
    net, smp, fl = _net(name), _sampler(name, solver), _flags(name)
    np.random.seed(7)
    ref = smp.sample(net, fl, seed=5, num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj, return_device=True)
    np.random.seed(7)
    got = guided_sample(net, smp, fl, _loss(name), 0.0, seed=5)
    torch.cuda.synchronize()
    for what, g, r in zip(("adj", "node"), _np(got), _np(ref)):
        err = float(np.abs(g - r).max() / np.abs(r).max())
        print(f"GUIDE scale0 {name} {solver} {what}: {err:.3e}")
        assert g.shape == r.shape and err <= TRAJ_RTOL, (what, err)


def _known(name, fl):
    cfg = Y.CONFIGS[name]()
    B, N = fl.shape[0], cfg.max_node_num
    rng = np.random.default_rng(4)
    ka = np.sign(rng.standard_normal((B, cfg.c_adj, N, N))).astype(np.float32)
    kn = np.sign(rng.standard_normal((B, N, cfg.c_node))).astype(np.float32) * np.float32(0.7)
    ma, mn = rng.random(ka.shape) < 0.4, rng.random(kn.shape) < 0.4
    return ka, kn, ma, mn


@functools.lru_cache(maxsize=None)
def _guided(name, solver, with_known, clip):
    from diffusesg_amd.guide import guided_sample
    net, smp, fl = _net(name), _sampler(name, solver), _flags(name)
    known = _known(name, fl) if with_known else None
    scale = np.linspace(3.0, 0.5, T8)
    np.random.seed(11)
    a, n, trace = guided_sample(net, smp, fl, _loss(name), scale, clip_ratio=clip, seed=9, return_trace=True,
                                known=None if known is None else tuple(torch.from_numpy(k) for k in known))
    torch.cuda.synchronize()
    trace = [{k: (_np(v) if isinstance(v, tuple) else v) for k, v in e.items()} for e in trace]
    return _full(name, *_np((a, n))), trace, known, scale, smp, fl.numpy()


COMPOSE = [("tiny", "euler", True, 0.05), ("tiny", "heun", False, 0.05), ("tiny", "dpmpp_2m", True, None), ("nosc", "heun", True, 0.3)]


@pytest.mark.parametrize("name,solver,with_known,clip", COMPOSE)
def test_every_step_recomputed_in_float64(name, solver, with_known, clip):
    """from the trace: shift and guided estimate from (x_hat, D, gradient, w_i, t_hat) with the clip and the known select, then the
    solver's update from x_hat and the guided estimates -- all in float64, against the loop's float32 state at 1e-6 of its scale"""
    from diffusesg_amd import lib as L
    (fa, fn), trace, known, scale, smp, flags = _guided(name, solver, with_known, clip)
    _sg, t_hat, _nc, h_step = L.sigma_schedule(smp._cfg())
    ms = L.multistep_coef(smp._cfg())
    by_step = {}
    for e in trace:
        by_step.setdefault(e["step"], []).append(e)
    assert sorted(by_step) == list(range(T8))
    n_clipped, prev = 0, None

    def close(got, ref, scale_of, what):
        for k in range(2):
            s = max(float(np.abs(scale_of[k]).max()), 1e-30)
            err = float(np.abs(got[k].astype(np.float64) - ref[k]).max()) / s
            assert err <= 1e-6, f"{what}[{k}]: {err:.3e}"
    for i in range(T8):
        es = by_step[i]
        assert len(es) == (2 if solver == "heun" and i < T8 - 1 else 1)
        G = []
        for e in es:
            assert e["t_hat"] == float(t_hat[i]) and e["w"] == float(np.float32(scale[i]))
            shift, Gi = GR.guided_estimate(e["x_hat"], e["D"], e["grad"], e["w"], e["t_hat"], flags, clip, known)
            raw = GR.guided_estimate(e["x_hat"], e["D"], e["grad"], e["w"], e["t_hat"], flags, None, known)[0]
            n_clipped += int((GR.graph_norm(*shift) < GR.graph_norm(*raw) * (1 - 1e-9)).any())
            close(e["shift"], shift, e["x_hat"], f"step {i} shift")
            close(e["D_guided"], Gi, e["x_hat"], f"step {i} guided estimate")
            G.append(Gi)
        x_hat = es[0]["x_hat"]
        assert all(np.array_equal(es[-1]["x_hat"][k], x_hat[k]) for k in range(2)), "stage 2 is evaluated at (x_hat, t_hat)"
        if len(es) == 2:
            x = GR.heun_update(x_hat, G[0], G[1], float(t_hat[i]), float(h_step[i]), flags)
        else:
            x = GR.euler_update(x_hat, G[0], float(t_hat[i]), float(h_step[i]), flags, float(ms[i]), prev)
        close(es[-1]["x"], x, x_hat, f"step {i} state")
        prev = G[0]
    close((fa, fn), tuple(v.astype(np.float64) for v in by_step[T8 - 1][-1]["x"]), (fa, fn), "returned sample")
    if clip is not None:
        assert n_clipped > 0, "the clip never engaged: the case does not test it"
    if solver == "dpmpp_2m":
        assert np.count_nonzero(ms) > 0


@pytest.mark.parametrize("name,solver,with_known,clip", [c for c in COMPOSE if c[2]])
def test_known_entries_land_bit_exact(name, solver, with_known, clip):
    (fa, fn), trace, (ka, kn, ma, mn), _s, _smp, flags = _guided(name, solver, with_known, clip)
    f = flags.astype(bool)
    va, vn = np.broadcast_to(f[:, None, :, None] & f[:, None, None, :], ka.shape), np.broadcast_to(f[:, :, None], kn.shape)
    assert (ma & va).any() and (mn & vn).any()
    for e in trace:
        for key in ("D", "D_guided"):
            assert np.array_equal(e[key][0][ma & va], ka[ma & va]), f"step {e['step']} {key} adj"
            assert np.array_equal(e[key][1][mn & vn], kn[mn & vn]), f"step {e['step']} {key} node"
    # the last step runs to t = 0: the state becomes the guided estimate up to the update's rounding
    assert np.abs(fa[ma & va] - ka[ma & va]).max() <= 1e-5 and np.abs(fn[mn & vn] - kn[mn & vn]).max() <= 1e-5


@pytest.mark.parametrize("name,solver,with_known,clip", COMPOSE)
def test_padded_entries_stay_zero(name, solver, with_known, clip):
    (fa, fn), trace, _k, _s, _smp, flags = _guided(name, solver, with_known, clip)
    f = flags.astype(bool)
    pa, pn = ~np.broadcast_to(f[:, None, :, None] & f[:, None, None, :], fa.shape), ~np.broadcast_to(f[:, :, None], fn.shape)
    assert pa.any() and pn.any()
    assert (fa[pa] == 0).all() and (fn[pn] == 0).all()
    for e in trace:
        for key in ("x_hat", "D", "shift", "D_guided"):
            assert (e[key][0][pa] == 0).all() and (e[key][1][pn] == 0).all(), f"step {e['step']} {key}"


@pytest.mark.parametrize("name,solver", [("tiny", "heun"), ("nosc", "dpmpp_2m")])
def test_seeded_batch_equals_graphs_alone(name, solver):
    """graph b of a guided batch with graph_seeds equals the same graph guided alone with its seed, under "batch_invariant" (the coin's
    extra pass runs on the sampling path).  The training-form path at these shapes is bit-invariant to the batch size (every product
    stays on the plain kernel, row kernels work per row, torch's per-graph reductions run over the same extent): array_equal."""
    from diffusesg_amd.guide import guided_sample
    net, smp, fl = _net(name), _sampler(name, solver), _flags(name)
    seeds = [2 ** 64 - 1, 2 ** 32 + 5, 1]
    h = net.model._ensure_handle()
    old = h.get_option("batch_invariant")
    h.set_option("batch_invariant", 1)
    try:
        batch = _np(guided_sample(net, smp, fl, _loss(name), 1.5, graph_seeds=seeds, coin_seed=3))
        for b in range(len(seeds)):
            one = _np(guided_sample(net, smp, fl[b:b + 1], _loss(name), 1.5, graph_seeds=seeds[b:b + 1], coin_seed=3))
            d = max(float(np.abs(batch[k][b:b + 1] - one[k]).max()) for k in range(2))
            print(f"GUIDE seeded {name} {solver} graph {b}: max |batch row - alone| = {d:.3e}")
            assert all(np.array_equal(batch[k][b:b + 1], one[k]) for k in range(2)), f"graph {b}: {d:.3e}"
    finally:
        h.set_option("batch_invariant", old)
