"""No GPU: the host side of the probability-flow ODE encoder (include/dsg.h, "Probability-flow ODE between the noise levels") --
dsg_ode_evals against its restatement in float64 NumPy, `assemble_logp` on an analytic Gaussian, and the power of the GPU test's bars:
planted faults applied to the fixture's float64 traces must move n_k or log p beyond the bar tests/test_ode.py uses."""
import ctypes as C

import numpy as np
import pytest

from diffusesg_amd import lib, ode
from diffusesg_amd import synth as Y
from util import load

SOLVERS = ("euler", "heun")
DIRECTIONS = ("encode", "decode")
BAR_MARGIN = 16.0   # tests/test_ode.py: 16 x the fixture's largest float32-against-float64 discrepancy over the cases of a network


def expected_evals(T, solver, direction, stage2_at_a=False):
    """levels: the schedule's sigma_steps rounded to float32 (no churn: t_hat is the level); h = fp32(b - a); the weights in float64"""
    sg = lib.sigma_schedule(lib.make_sampler_cfg(T, solver, S_churn=0.0))[0]
    t = sg.astype(np.float32)
    t_eval, w, steps = [], [], []
    for j in range(T - 1):
        k = T - 1 - j if direction == "encode" else j
        a, b = t[k], (t[k - 1] if direction == "encode" else t[k + 1])
        h = np.float32(b - a)
        ah = abs(np.float64(h))
        steps.append((np.float64(a), np.float64(b), ah))
        if solver == "euler":
            t_eval.append(a); w.append(ah / np.float64(a))
        else:
            t_eval += [a, b]
            w += [ah / (2.0 * np.float64(a)), ah / (2.0 * np.float64(a if stage2_at_a else b))]
    return np.array(t_eval, np.float32), np.array(w, np.float64), steps


@pytest.mark.parametrize("T", [2, 3, 8, 50])
@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("solver", SOLVERS)
def test_evals_against_numpy(solver, direction, T):
    t_eval, w = lib.ode_evals(lib.make_sampler_cfg(T, solver, S_churn=0.0), lib.make_ode_cfg(direction, "none"))
    want_t, want_w, steps = expected_evals(T, solver, direction)
    assert len(t_eval) == (2 if solver == "heun" else 1) * (T - 1)
    assert np.array_equal(t_eval.view(np.uint32), want_t.view(np.uint32)), (t_eval, want_t)
    assert np.array_equal(w, want_w), np.abs(w - want_w).max()
    # order: encode climbs from t_min, decode descends from t_max and ends at t_min (there is no step to 0)
    lv = lib.sigma_schedule(lib.make_sampler_cfg(T, solver, S_churn=0.0))[1]
    assert t_eval[0] == (lv[-1] if direction == "encode" else lv[0])
    assert np.all(np.diff(t_eval) >= 0) if direction == "encode" else np.all(np.diff(t_eval) <= 0)
    assert t_eval.min() >= lv[-1] > 0
    # the weights are the solver's quadrature of int dt / t: their sum is that rule applied to 1 / t ...
    rule = sum(ah / a if solver == "euler" else 0.5 * ah * (1.0 / a + 1.0 / b) for a, b, ah in steps)
    assert abs(w.sum() - rule) <= 1e-13 * rule
    # ... which, 1 / t being convex and decreasing, the trapezoid and the left-endpoint rule from below overestimate and the
    # left-endpoint rule from above underestimates
    exact = np.log(np.float64(lv[0]) / np.float64(lv[-1]))
    if solver == "heun" or direction == "encode":
        assert w.sum() > exact
    else:
        assert w.sum() < exact
    # the probe plays no part in the plan
    t2, w2 = lib.ode_evals(lib.make_sampler_cfg(T, solver, S_churn=0.0), lib.make_ode_cfg(direction, "gaussian"))
    assert np.array_equal(t2, t_eval) and np.array_equal(w2, w)


def test_evals_refusals():
    L = lib.load()
    good, ocfg = lib.make_sampler_cfg(8, "heun", S_churn=0.0), lib.make_ode_cfg("encode", "rademacher")
    call = lambda s, o, t=None, w=None, cap=0: int(L.dsg_ode_evals(C.byref(s), C.byref(o), t, w, cap))
    assert call(good, ocfg) == 14
    assert call(lib.make_sampler_cfg(1, "heun", S_churn=0.0), ocfg) == lib.DSG_ERR_INVALID          # T >= 2
    assert call(lib.make_sampler_cfg(8, "dpmpp_2m", S_churn=0.0), ocfg) == lib.DSG_ERR_INVALID      # no multistep solver
    assert call(lib.make_sampler_cfg(8, "heun"), ocfg) == lib.DSG_ERR_INVALID                       # churn noise (S_churn = 40)
    assert call(lib.make_sampler_cfg(8, "euler", S_churn=1.0), ocfg) == lib.DSG_ERR_INVALID
    for bad in (lib.DsgOdeCfg(2, 0), lib.DsgOdeCfg(-1, 0), lib.DsgOdeCfg(0, 3), lib.DsgOdeCfg(0, -1)):
        assert call(good, bad) == lib.DSG_ERR_INVALID
    buf_t, buf_w = np.zeros(14, np.float32), np.zeros(14, np.float64)
    assert call(good, ocfg, buf_t.ctypes.data, buf_w.ctypes.data, 13) == lib.DSG_ERR_INVALID        # cap < n_evals with an array given
    assert call(good, ocfg, buf_t.ctypes.data, None, 14) == 14 and call(good, ocfg, None, buf_w.ctypes.data, 14) == 14
    with pytest.raises(lib.DsgError, match="S_churn"):
        lib.ode_evals(lib.make_sampler_cfg(8, "heun"), ocfg)
    assert C.sizeof(lib.DsgOdeCfg) == 32
    assert lib.ODE_PROBE_STREAM > lib.WALK_MAX_STEPS + 1


def test_assemble_logp_on_the_analytic_gaussian():
    """Data N(0, s^2 I): D = s^2 x / (s^2 + t^2), so n(t) = tr J_D - d c_skip = d (s^2 / (s^2 + t^2) - s_d^2 / (t^2 + s_d^2)) and the ODE's
    solution is x(t) = x_min sqrt((s^2 + t^2) / (s^2 + t_min^2)).  With the prior N(0, t_max^2 I) in place of the exact marginal
    N(0, (s^2 + t_max^2) I), the formula gives log N(x_min; 0, (s^2 + t_min^2) I) + mismatch,
        mismatch = -(d/2) ln(t_max^2 / (s^2 + t_max^2)) - |x_max|^2 / 2 (1 / t_max^2 - 1 / (s^2 + t_max^2)),
    up to the remainder of the T = 256 Heun (trapezoid) quadrature of g(t) = n(t) / t, which is bounded step by step by
    |h|^3 / 12 max_[a,b] |g''|, g'' = d (u''(s^2) - u''(s_d^2)), u''(c) = 2 t (t^2 - 3 c) / (c + t^2)^3."""
    d, s, sd, T = 10, 0.7, ode.SIGMA_D, 256
    x_min = np.linspace(-1.3, 1.1, d)
    t_eval, w = lib.ode_evals(lib.make_sampler_cfg(T, "heun", S_churn=0.0), lib.make_ode_cfg("encode", "rademacher"))
    lv = lib.sigma_schedule(lib.make_sampler_cfg(T, "heun", S_churn=0.0))[1].astype(np.float64)
    t_max, t_min = lv[0], lv[-1]
    te = t_eval.astype(np.float64)
    n = d * (s * s / (s * s + te * te) - sd * sd / (te * te + sd * sd))
    x_max_sq = (x_min ** 2).sum() * (s * s + t_max ** 2) / (s * s + t_min ** 2)
    logp, bpd = ode.assemble_logp([x_max_sq], n[:, None], w, [d], t_max, t_min)
    v = s * s + t_min * t_min
    log_n = -0.5 * d * np.log(2 * np.pi * v) - (x_min ** 2).sum() / (2 * v)
    mismatch = -0.5 * d * np.log(t_max ** 2 / (s * s + t_max ** 2)) - 0.5 * x_max_sq * (1 / t_max ** 2 - 1 / (s * s + t_max ** 2))
    upp = lambda t, c: 2 * t * (t * t - 3 * c) / (c + t * t) ** 3
    rem = 0.0
    for a, b in zip(lv[1:], lv[:-1]):
        tt = np.linspace(a, b, 65)
        rem += (b - a) ** 3 / 12 * 1.1 * np.abs(d * (upp(tt, s * s) - upp(tt, sd * sd))).max()   # 1.1: the maximum is sampled
    err = abs(logp[0] - (log_n + mismatch))
    print(f"analytic Gaussian: log p {logp[0]:.6f}, log N {log_n:.6f}, mismatch {mismatch:.3e}, |err| {err:.3e}, remainder bound {rem:.3e}")
    assert rem < 0.05 and abs(mismatch) < 1e-2
    assert err <= rem
    assert abs(logp[0] - log_n) <= abs(mismatch) + rem
    assert abs(bpd[0] + logp[0] / (d * np.log(2))) < 1e-15
    # a graph with no valid node: log p = 0
    lp0, bpd0 = ode.assemble_logp([0.0], np.zeros((len(w), 1)), w, [0], t_max, t_min)
    assert lp0[0] == 0 and bpd0[0] == 0


# ---- power of the GPU test's bars: planted faults on the fixture's float64 traces ----
def _case(name, run):
    g = load("ode_likelihood.npz")
    cfg, flags = Y.ode_case(name)[:2]
    T, solver = Y.ODE_RUNS[run]
    dims = ode.graph_dims(flags, cfg.c_adj, cfg.c_node)
    n, logp = g[f"{name}/{run}/n"], g[f"{name}/{run}/logp"]
    lat2 = (g[f"{name}/{run}/latent_adj"].reshape(len(flags), -1) ** 2).sum(1) + (g[f"{name}/{run}/latent_node"].reshape(len(flags), -1) ** 2).sum(1)
    bar_n = BAR_MARGIN * float(g[f"{name}/worst_n"]) * np.abs(n).max()
    bar_lp = BAR_MARGIN * float(g[f"{name}/worst_logp"]) * np.abs(logp)
    t_eval, w = lib.ode_evals(lib.make_sampler_cfg(T, solver, S_churn=0.0), lib.make_ode_cfg("encode", "rademacher"))
    lv = lib.sigma_schedule(lib.make_sampler_cfg(T, solver, S_churn=0.0))[1].astype(np.float64)
    return dict(cfg=cfg, flags=flags, T=T, solver=solver, dims=dims, n=n, logp=logp, lat2=lat2, bar_n=bar_n, bar_lp=bar_lp, t_eval=t_eval.astype(np.float64),
                w=w, t_max=lv[0], t_min=lv[-1])


CASES = [(name, run) for name in Y.ODE_NETS for run in Y.ODE_RUNS]


@pytest.mark.parametrize("name,run", CASES)
def test_fixture_is_what_the_formula_gives(name, run):
    """the stored log p is assemble_logp of the stored latent and traces (the GPU test assembles the same way), and sum_k w_k n_k stays small next to the
    closed-form term"""
    c = _case(name, run)
    logp, _ = ode.assemble_logp(c["lat2"], c["n"], c["w"], c["dims"], c["t_max"], c["t_min"])
    assert np.allclose(logp, c["logp"], rtol=1e-12, atol=0)
    # the conditioning of the formula: had the c_skip term stayed in the trace, the quadrature would carry a share of the closed-form
    # term's size (test_power_c_skip_not_removed); the network part alone is a few percent of it at most
    closed = 0.5 * c["dims"] * np.log((c["t_max"] ** 2 + ode.SIGMA_D ** 2) / (c["t_min"] ** 2 + ode.SIGMA_D ** 2))
    assert np.all(np.abs((c["w"][:, None] * c["n"]).sum(0)) < 0.05 * closed)


@pytest.mark.parametrize("name,run", CASES)
def test_power_dropped_entry(name, run):
    """one live entry dropped from a contraction: the sum loses one of its d terms -- on average n_k / d"""
    c = _case(name, run)
    moved = np.abs(c["n"] / c["dims"][None, :]).max()
    assert moved > c["bar_n"], (moved, c["bar_n"])


@pytest.mark.parametrize("name,run", CASES)
def test_power_padded_entries_counted(name, run):
    """padded entries included: d becomes C_adj N^2 + C_node N for every graph -- log p of every ragged graph moves"""
    c = _case(name, run)
    N = c["cfg"].max_node_num
    full = np.full_like(c["dims"], c["cfg"].c_adj * N * N + c["cfg"].c_node * N)
    logp, _ = ode.assemble_logp(c["lat2"], c["n"], c["w"], full, c["t_max"], c["t_min"])
    ragged = c["dims"] < full
    assert ragged.any() and np.all(np.abs(logp - c["logp"])[ragged] > c["bar_lp"][ragged])


@pytest.mark.parametrize("name,run", [cr for cr in CASES if Y.ODE_RUNS[cr[1]][1] == "heun"])
def test_power_stage2_weight(name, run):
    """stage-2 weight |h| / (2a) in place of |h| / (2b)"""
    c = _case(name, run)
    w_bad = expected_evals(c["T"], c["solver"], "encode", stage2_at_a=True)[1]
    assert np.array_equal(expected_evals(c["T"], c["solver"], "encode")[1], c["w"])
    logp, _ = ode.assemble_logp(c["lat2"], c["n"], w_bad, c["dims"], c["t_max"], c["t_min"])
    assert np.all(np.abs(logp - c["logp"]) > c["bar_lp"]), (np.abs(logp - c["logp"]), c["bar_lp"])


@pytest.mark.parametrize("name,run", CASES)
def test_power_c_skip_not_removed(name, run):
    """c_skip |eps|^2 left in the trace: n_k grows by c_skip(t_k) d (a Rademacher probe: |eps|^2 = d)"""
    c = _case(name, run)
    c_skip = ode.SIGMA_D ** 2 / (c["t_eval"] ** 2 + ode.SIGMA_D ** 2)
    n_bad = c["n"] + c_skip[:, None] * c["dims"][None, :]
    assert np.abs(n_bad - c["n"]).max() > c["bar_n"]
    logp, _ = ode.assemble_logp(c["lat2"], n_bad, c["w"], c["dims"], c["t_max"], c["t_min"])
    assert np.all(np.abs(logp - c["logp"]) > c["bar_lp"])


def test_package_exports():
    import diffusesg_amd
    for name in ("encode", "decode", "log_likelihood", "sample_with_logp", "graph_log_likelihood", "exact_net_trace", "interpolate", "assemble_logp"):
        assert name in diffusesg_amd.__all__ and getattr(diffusesg_amd, name) is getattr(ode, name)
