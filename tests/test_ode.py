"""GPU: the probability-flow ODE encoder (dsg_ode_run, diffusesg_amd.ode) against tests/golden/ode_likelihood.npz -- the reference
network under torch autograd in float64 (tools/gen_ode_golden.py) -- plus the properties of the entry, the per-graph contraction
kernel on its own through dsg_debug_graph_dot, and the status codes.  The bar of a quantity is 16 x the largest discrepancy of the
reference's own float32 run against its float64 run that the fixture records for it over the cases of the same network; measured
figures: profiles/ode_errors.md.  Every case runs once per session (module cache)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from diffusesg_amd import lib, ode
from diffusesg_amd import synth as Y
from diffusesg_amd import weights as W
from util import load

pytestmark = pytest.mark.gpu

MARGIN = 16.0
T_ = lambda v: torch.from_numpy(np.ascontiguousarray(v))
P_ = lambda t: C.c_void_p(0 if t is None else t.data_ptr())


@functools.lru_cache(maxsize=None)
def _net(name):
    from diffusesg_amd.model import build_network
    cfg = Y.CONFIGS[name]()
    return build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")


def _sampler(name, run):
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    T, solver = Y.ODE_RUNS[run]
    return NodeAdjEDMSamplerHip(num_steps=T, solver=solver, S_churn=0, self_condition=Y.CONFIGS[name]().self_condition)


def _squeeze(cfg, a, n):
    return (a[:, 0] if cfg.c_adj == 1 else a), (n[..., 0] if cfg.c_node == 1 else n)


def _flat(a, n):
    B = a.shape[0]
    a, n = (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v) for v in (a, n))
    return np.concatenate([a.reshape(B, -1), n.reshape(B, -1)], 1).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _ll(name, run):
    """log_likelihood of the fixture's graphs with its recorded probes"""
    cfg, flags, adj, node, p_adj, p_node = Y.ode_case(name)
    a, n = _squeeze(cfg, adj, node)
    r = ode.log_likelihood(_net(name), _sampler(name, run), T_(a), T_(n), T_(flags), probes=(T_(p_adj), T_(p_node)))
    torch.cuda.synchronize()
    return r


CASES = [(name, run) for name in Y.ODE_NETS for run in Y.ODE_RUNS]


@pytest.mark.parametrize("name,run", CASES)
def test_against_the_float64_fixture(name, run):
    g = load("ode_likelihood.npz")
    r = _ll(name, run)
    lat_ref = _flat(g[f"{name}/{run}/latent_adj"], g[f"{name}/{run}/latent_node"])
    n_ref, lp_ref = g[f"{name}/{run}/n"], g[f"{name}/{run}/logp"]
    e_lat = np.abs(_flat(*r["latent"]) - lat_ref).max() / np.abs(lat_ref).max()
    e_n = np.abs(r["net_trace"] - n_ref).max() / np.abs(n_ref).max()
    e_lp = (np.abs(r["logp"] - lp_ref) / np.abs(lp_ref)).max()
    bars = {k: MARGIN * float(g[f"{name}/worst_{k}"]) for k in ("latent", "n", "logp")}
    quad = np.abs((r["weights"][:, None] * r["net_trace"]).sum(0)).max()
    print(f"ODE {name}/{run}: latent {e_lat:.3e} of max (bar {bars['latent']:.3e}) | n_k {e_n:.3e} of max = {np.abs(r['net_trace'] - n_ref).max():.3e} abs "
          f"(bar {bars['n']:.3e}) | logp {e_lp:.3e} of |logp| = {np.abs(r['logp'] - lp_ref).max():.3e} abs (bar {bars['logp']:.3e}) | max |sum w n| {quad:.3f}")
    assert r["net_trace"].shape == n_ref.shape and r["logp"].dtype == np.float64
    assert e_lat <= bars["latent"], f"latent: {e_lat:.3e} > {bars['latent']:.3e}"
    assert e_n <= bars["n"], f"n_k: {e_n:.3e} > {bars['n']:.3e}"
    assert e_lp <= bars["logp"], f"log p: {e_lp:.3e} > {bars['logp']:.3e}"
    assert np.allclose(r["bits_per_dim"], -r["logp"] / (r["dims"] * np.log(2)), rtol=1e-14)


@pytest.mark.parametrize("si", range(len(Y.ODE_EXACT_SIGMAS)))
@pytest.mark.parametrize("name", ["nosc", "tiny"])
def test_exact_net_trace(name, si):
    g = load("ode_likelihood.npz")
    cfg, flags, adj, node, _, _ = Y.ode_case(name)
    a, n = _squeeze(cfg, adj, node)
    got = ode.exact_net_trace(_net(name), T_(a), T_(n), T_(flags), Y.ODE_EXACT_SIGMAS[si], chunk=128)
    ref = g[f"{name}/exact/{si}"]
    err, bar = np.abs(got - ref).max() / np.abs(ref).max(), MARGIN * float(g[f"{name}/worst_n"])
    print(f"ODE exact trace {name} sigma {Y.ODE_EXACT_SIGMAS[si]}: {got} vs {ref}: {err:.3e} of max (bar {bar:.3e})")
    assert err <= bar


@pytest.mark.parametrize("name", Y.ODE_NETS)
def test_round_trip(name):
    """Heun T = 16: decode(encode(x)) keeps every sign of every live entry; its residual is the fixture's float64 residual up to the latent bar"""
    g = load("ode_likelihood.npz")
    cfg, flags, adj, node, _, _ = Y.ode_case(name)
    a, n = _squeeze(cfg, adj, node)
    net, smp = _net(name), _sampler(name, "t16_heun")
    la, ln = ode.encode(net, smp, T_(a), T_(n), T_(flags))
    da, dn = ode.decode(net, smp, la, ln, T_(flags))
    x, rt = _flat(adj, node), _flat(da, dn)
    live = x != 0
    ref_rt = _flat(g[f"{name}/t16_heun/decoded_adj"], g[f"{name}/t16_heun/decoded_node"])
    res, ref_res = np.abs(rt - x)[live].max(), float(g[f"{name}/t16_heun/residual"])
    bar = MARGIN * float(g[f"{name}/worst_latent"]) * np.abs(ref_rt).max()
    print(f"ODE round trip {name}: signs equal {np.mean(np.sign(rt[live]) == x[live]) * 100:.1f} %, residual {res:.5f} (float64 {ref_res:.5f}, bar + {bar:.2e})")
    assert np.array_equal(np.sign(rt[live]), x[live])
    assert (rt[~live] == 0).all()
    assert res <= ref_res + bar


# ---- properties ----
@functools.lru_cache(maxsize=None)
def _prop_runs():
    """tiny, Heun T = 8: (no probe, device Rademacher probe read back, the same again, the recorded probe, device Gaussian probe)"""
    cfg, flags, adj, node, _, _ = Y.ode_case("tiny")
    net, smp = _net("tiny"), _sampler("tiny", "t8_heun")
    seeds = [11, 2 ** 63 + 5, 7]
    args = (net, smp, T_(adj), T_(node), T_(flags), "encode")
    none = ode.run(*args)
    rad = ode.run(*args, "rademacher", seeds, None, True)
    rad2 = ode.run(*args, "rademacher", seeds, None, True)
    rec = ode.run(*args, "rademacher", None, rad[3])
    gau = ode.run(*args, "gaussian", seeds, None, True)
    torch.cuda.synchronize()
    return dict(flags=flags, seeds=seeds, none=none, rad=rad, rad2=rad2, rec=rec, gau=gau, net=net, smp=smp)


def _same(a, b):
    return np.array_equal(a.cpu().numpy().view(np.uint8 if a.dtype == torch.uint8 else (np.uint64 if a.dtype == torch.float64 else np.uint32)),
                          b.cpu().numpy().view(np.uint8 if b.dtype == torch.uint8 else (np.uint64 if b.dtype == torch.float64 else np.uint32)))


def test_no_probe_is_the_probed_run_bit_for_bit():
    r = _prop_runs()
    assert r["none"][2] is None
    for k in (0, 1):
        assert _same(r["none"][k], r["rad"][k]) and _same(r["none"][k], r["gau"][k]) and _same(r["none"][k], r["rec"][k])


def test_two_runs_are_bit_identical():
    r = _prop_runs()
    for k in (0, 1, 2):
        assert _same(r["rad"][k], r["rad2"][k])
    assert _same(r["rad"][3][0], r["rad2"][3][0]) and _same(r["rad"][3][1], r["rad2"][3][1])


def test_recorded_probe_equals_the_device_probe_read_back():
    r = _prop_runs()
    assert _same(r["rec"][2], r["rad"][2])
    assert float(r["rad"][2].abs().max()) > 0


def test_device_probes_are_the_seeded_noise_stream():
    r = _prop_runs()
    na, nn = r["smp"].device_noise(r["net"], T_(r["flags"]), stream=lib.ODE_PROBE_STREAM, graph_seeds=r["seeds"])
    assert _same(r["gau"][3][0], na) and _same(r["gau"][3][1], nn)
    f = r["flags"].astype(bool)
    for draw, eps, live in ((na, r["rad"][3][0], np.broadcast_to((f[:, :, None] & f[:, None, :])[:, None], tuple(na.shape))),
                            (nn, r["rad"][3][1], np.broadcast_to(f[:, :, None], tuple(nn.shape)))):
        draw, eps = draw.cpu().numpy(), eps.cpu().numpy()
        assert np.array_equal(eps[live], np.where(draw[live] >= 0, np.float32(1), np.float32(-1)))
        assert (np.abs(eps[live]) == 1).all() and (eps[~live] == 0).all() and not np.signbit(eps[~live]).any()
    assert (r["rad"][3][0].cpu().numpy() == -1).any() and (r["rad"][3][0].cpu().numpy() == 1).any()


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_batch_invariant_graph_alone_equals_graph_in_a_batch_of_three(name):
    from diffusesg_amd.model import build_network
    cfg, flags, adj, node, p_adj, p_node = Y.ode_case(name)
    pick = [0, 1, 2] if len(flags) >= 3 else [0, 1, 0]
    flags, adj, node, p_adj, p_node = (v[pick] for v in (flags, adj, node, p_adj, p_node))
    net = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")   # its own handle: the option is not left on a shared one
    net.model._ensure_handle().set_option("batch_invariant", 1)
    smp = _sampler(name, "t8_heun")
    full = ode.log_likelihood(net, smp, T_(adj), T_(node), T_(flags), probes=(T_(p_adj), T_(p_node)))
    for b in range(3):
        one = ode.log_likelihood(net, smp, T_(adj[b:b + 1]), T_(node[b:b + 1]), T_(flags[b:b + 1]), probes=(T_(p_adj[b:b + 1]), T_(p_node[b:b + 1])))
        assert _same(one["latent"][0], full["latent"][0][b:b + 1]) and _same(one["latent"][1], full["latent"][1][b:b + 1]), f"graph {b}: latent"
        assert np.array_equal(one["net_trace"][:, 0].view(np.uint64), full["net_trace"][:, b].view(np.uint64)), f"graph {b}: traces"
        assert one["logp"][0].tobytes() == full["logp"][b].tobytes(), f"graph {b}: log p"


def test_replicas_of_n_probes_share_the_latent():
    cfg, flags, adj, node, _, _ = Y.ode_case("tiny")
    r = ode.log_likelihood(_net("tiny"), _sampler("tiny", "t8_euler"), T_(adj), T_(node), T_(flags), graph_seeds=[3, 4, 5], n_probes=2)
    B = len(flags)
    la, ln = r["latent_all"]
    assert la.shape[0] == 2 * B
    assert torch.equal(la[:B], la[B:]) and torch.equal(ln[:B], ln[B:])
    one = ode.log_likelihood(_net("tiny"), _sampler("tiny", "t8_euler"), T_(adj), T_(node), T_(flags), graph_seeds=[3, 4, 5])
    two = ode.log_likelihood(_net("tiny"), _sampler("tiny", "t8_euler"), T_(adj), T_(node), T_(flags),
                             graph_seeds=[(s + ode.SEED_STRIDE) % 2 ** 64 for s in (3, 4, 5)])
    assert np.allclose(r["net_trace"], 0.5 * (one["net_trace"] + two["net_trace"]), rtol=1e-12, atol=1e-12)
    assert r["net_trace"].shape == one["net_trace"].shape and not np.array_equal(one["net_trace"], two["net_trace"])


def test_sample_with_logp_assembles_its_own_traces():
    cfg, flags = Y.ode_case("tiny")[:2]
    smp = _sampler("tiny", "t8_heun")
    r = ode.sample_with_logp(_net("tiny"), smp, T_(flags), [21, 22, 23])
    lv = lib.sigma_schedule(smp._cfg())[1]
    eps = smp.device_noise(_net("tiny"), T_(flags), stream=0, graph_seeds=[21, 22, 23])
    assert torch.equal(r["x_max"][0], eps[0] * lv[0]) and torch.equal(r["x_max"][1], eps[1] * lv[0])
    x2 = (_flat(*r["x_max"]) ** 2).sum(1)
    logp, bpd = ode.assemble_logp(x2, r["net_trace"], r["weights"], r["dims"], float(lv[0]), float(lv[-1]))
    assert np.allclose(r["logp"], logp, rtol=1e-13) and np.allclose(r["bits_per_dim"], bpd, rtol=1e-13)
    assert r["net_trace"].shape == (2 * (smp.num_steps - 1), len(flags)) and np.isfinite(r["logp"]).all()
    f = flags.astype(bool)
    assert (r["node"].cpu().numpy()[~f] == 0).all()


def test_interpolate_ends_are_the_round_trips_and_unequal_shapes_are_refused():
    cfg, flags, adj, node, p_adj, p_node = Y.ode_case("tiny")
    net, smp = _net("tiny"), _sampler("tiny", "t8_heun")
    A, Bg = (T_(adj), T_(node)), (T_(p_adj), T_(p_node))   # the probe tensors serve as a second +-1 graph on the same flags
    out = ode.interpolate(net, smp, A, Bg, T_(flags), [0.0, 0.5, 1.0])
    for (oa, on), src in ((out[0], A), (out[2], Bg)):
        ra, rn = ode.decode(net, smp, *ode.encode(net, smp, *src, T_(flags)), T_(flags))
        assert torch.equal(oa, ra) and torch.equal(on, rn)
    ma, mn = out[1]
    f = flags.astype(bool)
    assert torch.isfinite(ma).all() and torch.isfinite(mn).all() and (mn.cpu().numpy()[~f] == 0).all()
    assert not torch.equal(ma, out[0][0]) and not torch.equal(ma, out[2][0])
    with pytest.raises(ValueError, match="flag row"):
        ode.interpolate(net, smp, A, (T_(p_adj[:2]), T_(p_node[:2])), T_(flags), [0.5])


def test_graph_log_likelihood_goes_through_io_encode():
    from diffusesg_amd import io
    cfg, flags = Y.ode_case("tiny")[:2]
    B, n = len(flags), cfg.max_node_num
    rs = np.random.RandomState(5)
    q_adj, q_node = T_(rs.randint(0, 51, (B, n, n)).astype(np.int32)).cuda(), T_(rs.randint(0, 150, (B, n)).astype(np.int32)).cuda()
    bbox = T_(rs.rand(B, n, 4).astype(np.float32)).cuda()
    net, smp = _net("tiny"), _sampler("tiny", "t8_euler")
    r = ode.graph_log_likelihood(net, smp, q_adj, q_node, bbox, T_(flags), 51, 150, graph_seeds=[1, 2, 3])
    a, x = io.encode(net, q_adj, q_node, bbox, T_(flags), 51, 150)
    want = ode.log_likelihood(net, smp, a, x, T_(flags), graph_seeds=[1, 2, 3])
    assert np.array_equal(r["logp"], want["logp"]) and np.array_equal(r["net_trace"], want["net_trace"])
    assert np.isfinite(r["logp"]).all() and np.isfinite(r["bits_per_dim"]).all()


# ---- the per-graph contraction on its own ----
def _flag_sets(B, N):
    full = np.ones((B, N), np.uint8)
    ragged = np.zeros((B, N), np.uint8)
    for b in range(B):
        ragged[b, :max(1, (N * (b + 2)) // (B + 2))] = 1
    one = np.zeros((B, N), np.uint8)
    one[np.arange(B), (np.arange(B) * 3) % N] = 1
    none = np.zeros((B, N), np.uint8)
    mixed = ragged.copy()
    mixed[0] = 0
    return dict(full=full, ragged=ragged, one=one, none=none, mixed=mixed)


def _graph_dot(aa, an, ba, bn, fl):
    B, Ca, N = aa.shape[0], aa.shape[1], aa.shape[2]
    d = [T_(v).cuda() for v in (aa, an, ba, bn, fl)]
    out = torch.full((B,), float("nan"), dtype=torch.float64, device="cuda")
    rc = lib.load().dsg_debug_graph_dot(B, N, Ca, an.shape[2], *(P_(t) for t in d), P_(out), None)
    assert rc == 0
    return out.cpu().numpy()


@pytest.mark.parametrize("chans", [(1, 1), (6, 12), (51, 154)])
@pytest.mark.parametrize("N", [5, 8, 40, 64])
def test_graph_dot_against_float64(N, chans):
    Ca, Cn = chans
    rs = np.random.RandomState(1000 * N + Ca)
    for B in (1, 3):
        aa, ba = (rs.standard_normal((B, Ca, N, N)).astype(np.float32) for _ in range(2))
        an, bn = (rs.standard_normal((B, N, Cn)).astype(np.float32) for _ in range(2))
        for kind, fl in _flag_sets(B, N).items():
            f = fl.astype(bool)
            la = np.broadcast_to((f[:, :, None] & f[:, None, :])[:, None], aa.shape)
            ln = np.broadcast_to(f[:, :, None], an.shape)
            xa, ya, xn, yn = aa.copy(), ba.copy(), an.copy(), bn.copy()
            for v, live in ((xa, la), (ya, la), (xn, ln), (yn, ln)):
                v[~live] = np.nan   # NaN at every padded entry of both operands
            got = _graph_dot(xa, xn, ya, yn, fl)
            prod = np.concatenate([(aa.astype(np.float64) * ba * la).reshape(B, -1), (an.astype(np.float64) * bn * ln).reshape(B, -1)], 1)
            want, mag = prod.sum(1), np.abs(prod).sum(1)
            dims = ode.graph_dims(fl, Ca, Cn)
            bar = 4.0 * dims * 2.0 ** -52 * mag   # float64 accumulation of exact float32 products: <= d 2^-52 sum |a_j b_j|; 4 x that
            assert np.isfinite(got).all(), (kind, B, got)
            assert np.all(np.abs(got - want) <= bar), (kind, B, np.abs(got - want), bar)
            if kind == "none":
                assert (got == 0).all() and not np.signbit(got).any()
            if B == 3:   # permuting the graphs permutes the outputs bit for bit; a graph alone gives the same bits
                perm = [2, 0, 1]
                gp = _graph_dot(xa[perm], xn[perm], ya[perm], yn[perm], fl[perm])
                assert np.array_equal(gp.view(np.uint64), got[perm].view(np.uint64)), kind
                g1 = _graph_dot(xa[1:2], xn[1:2], ya[1:2], yn[1:2], fl[1:2])
                assert g1.view(np.uint64)[0] == got.view(np.uint64)[1], kind


# ---- status codes ----
def test_refusals_leave_the_handle_usable():
    cfg, flags, adj, node, p_adj, p_node = Y.ode_case("tiny")
    net = _net("tiny")
    h = net.model._ensure_handle()
    L = h.L
    B = len(flags)
    a, x, fl, pa, pn = (T_(v).cuda() for v in (adj, node, flags, p_adj, p_node))
    oa, on = torch.empty_like(a), torch.empty_like(x)
    good = lib.make_sampler_cfg(4, "heun", S_churn=0.0)
    tr = torch.zeros((6, B), dtype=torch.float64, device="cuda")
    seeds = np.array([1, 2, 3], np.uint64)

    def call(scfg=good, ocfg=None, handle=h, x_adj=a, gs=None, probe=(None, None), out=(oa, on), out_probe=(None, None), trace=None):
        ocfg = ocfg or lib.make_ode_cfg("encode", "none")
        return L.dsg_ode_run(handle.raw, C.byref(scfg), C.byref(ocfg), B, P_(fl), P_(x_adj), P_(x), C.c_void_p(0 if gs is None else gs.ctypes.data),
                             P_(probe[0]), P_(probe[1]), P_(out[0]), P_(out[1]), P_(out_probe[0]), P_(out_probe[1]), P_(trace), None)
    rad = lib.make_ode_cfg("encode", "rademacher")
    INV = lib.DSG_ERR_INVALID
    assert call(scfg=lib.make_sampler_cfg(4, "heun")) == INV                              # churn noise
    assert b"S_churn" in L.dsg_last_error(h.raw)
    assert call(scfg=lib.make_sampler_cfg(1, "heun", S_churn=0.0)) == INV                 # T >= 2
    assert call(scfg=lib.make_sampler_cfg(4, "dpmpp_2m", S_churn=0.0)) == INV             # no multistep solver
    assert call(ocfg=lib.DsgOdeCfg(2, 0)) == INV and call(ocfg=lib.DsgOdeCfg(0, 3)) == INV
    assert call(ocfg=rad, trace=tr) == INV                                                # a probe with neither seeds nor recorded tensors
    assert call(ocfg=rad, probe=(pa, None), trace=tr) == INV                              # half a recorded probe
    assert call(ocfg=rad, probe=(None, pn), gs=seeds, trace=tr) == INV
    assert call(ocfg=rad, gs=seeds) == INV                                                # out_net_trace missing
    assert call(ocfg=rad, gs=seeds, trace=tr, out_probe=(oa, None)) == INV                # half an output probe
    assert call(x_adj=None) == INV and call(out=(oa, None)) == INV
    fresh = lib.Handle(cfg)                                                               # before dsg_finalize_weights
    assert call(handle=fresh) == -4
    fresh.close()
    # after every refusal the handle still runs, and gives what an untouched run gives
    assert call(ocfg=rad, probe=(pa, pn), trace=tr) == 0
    torch.cuda.synchronize()
    ref = _ll("tiny", "t8_heun")
    r4 = ode.log_likelihood(net, _sampler("tiny", "t8_heun"), T_(adj), T_(node), T_(flags), probes=(T_(p_adj), T_(p_node)))
    assert np.array_equal(r4["net_trace"], ref["net_trace"]) and torch.equal(r4["latent"][0], ref["latent"][0])
    assert np.isfinite(tr.cpu().numpy()).all() and torch.isfinite(oa).all()
