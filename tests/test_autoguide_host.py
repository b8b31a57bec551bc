"""CPU: autoguidance (dsg_attach_guide) without a device -- the declared and bound entries, the Python layer's argument
checks, the host's step-selection rule and forward count, and the fixture (tests/golden/autoguide.npz) against a NumPy float32
restatement of the combine, with the power of the parity bar: the plausible wrong composites all miss it."""
import os
import re

import numpy as np
import pytest

from diffusesg_amd import autoguide as AG
from diffusesg_amd import lib as L
from diffusesg_amd import spec as S
from diffusesg_amd import synth as Y
from diffusesg_amd import weights as W
from util import FWD_RTOL, load, rel_err

ENTRIES = ("dsg_attach_guide", "dsg_detach_guide", "dsg_guide_info", "dsg_guide_forwards")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dsg.h")


def test_header_declares_and_lib_binds_the_entries():
    text = open(HEADER).read()
    for name in ENTRIES:
        assert re.search(r"^int %s\(dsg_handle h[,)]" % name, text, re.M), name
        assert name in L.EXPORTS
    assert "#define DSG_ABI_VERSION 5" in re.sub(r"[ \t]+", " ", text)
    lib = L.load()
    assert lib.dsg_attach_guide.argtypes[2:] == [L.C.c_float] * 3 and len(lib.dsg_guide_info.argtypes) == 5
    # the header says what the attachment does not act on
    doc = text[text.index("Autoguidance"):text.index("int dsg_attach_guide")]
    for word in ("dsg_denoise", "dsg_train_", "dsg_precond_vjp", "dsg_ode_run", "Non-re-entrancy"):
        assert word in doc, word


def _net(**kw):
    from diffusesg_amd.model import build_network
    base = dict(max_node_num=8, c_adj=6, c_node=12, depths=(1, 1), num_heads=(3, 6), window_size=4, self_condition=True)
    base.update(kw)
    return build_network(S.ModelConfig(**base), None, device="cuda")   # no handle until the first forward: nothing here needs a device


def test_attach_guide_argument_validation():
    main, guide = _net(), _net(embed_dim=64, num_heads=(2, 4))
    assert main.guide_info() is None
    main.attach_guide(guide, scale=1.5, sigma_range=(0.5, 20.0))
    info = main.guide_info()
    assert info["guide"] is guide and info["scale"] == 1.5 and info["sigma_range"] == (0.5, 20.0)
    assert "_guide_net" not in dict(main.named_modules()) and set(main.state_dict()) == set(_net().state_dict())
    main.attach_guide(guide)   # defaults: scale 2, every level
    assert main.guide_info()["scale"] == 2.0 and main.guide_info()["sigma_range"] == (-np.inf, np.inf)
    main.detach_guide()
    assert main.guide_info() is None
    with pytest.raises(ValueError, match="itself"):
        main.attach_guide(main)
    with pytest.raises(TypeError):
        main.attach_guide(guide.model)
    for field, kw in (("max_node_num", dict(max_node_num=16)), ("c_adj", dict(c_adj=5)), ("c_node", dict(c_node=11)),
                      ("self_condition", dict(self_condition=False))):
        with pytest.raises(ValueError, match=field):
            main.attach_guide(_net(**kw))
    for bad, word in ((dict(scale=float("inf")), "scale"), (dict(scale=float("nan")), "scale"), (dict(sigma_range=(3.0, 2.0)), "sigma_range"),
                      (dict(sigma_range=(float("nan"), 2.0)), "sigma_range"), (dict(sigma_range=(1.0, float("nan"))), "sigma_range")):
        with pytest.raises(ValueError, match=word):
            main.attach_guide(guide, **bad)
    assert main.guide_info() is None
    third = _net()
    guide.attach_guide(third)
    with pytest.raises(ValueError, match="guide of its own"):
        main.attach_guide(guide)


def _scfg(T=8, solver="heun", churn=40.0):
    return L.make_sampler_cfg(T, solver, churn)


@pytest.mark.parametrize("T,solver,churn", [(8, "heun", 40.0), (8, "euler", 0.0), (18, "dpmpp_2m", 0.0), (50, "heun", 40.0)])
def test_step_selection_rule(T, solver, churn):
    scfg = _scfg(T, solver, churn)
    t64 = L.sigma_schedule(scfg)[1].astype(np.float64)
    assert AG.guided_steps(scfg, None, 2.0).all() and not AG.guided_steps(scfg, None, 1.0).any()
    for lo, hi in ((0.1, 30.0), (float(t64[T // 2]), float(t64[1])), (float(t64[3]), float(t64[3])), (200.0, 300.0),
                   (np.nextafter(np.float32(t64[2]), np.float32(0)), np.nextafter(np.float32(t64[2]), np.float32(100)))):
        lo32, hi32 = np.float32(lo), np.float32(hi)
        want = (t64 >= float(lo32)) & (t64 <= float(hi32))   # float32 values compare exactly in float64
        assert np.array_equal(AG.guided_steps(scfg, (lo, hi), 2.0), want), (lo, hi)
    assert AG.guided_steps(scfg, (float(t64[3]), float(t64[3])), 2.0).sum() == 1   # the bounds are included
    with pytest.raises(ValueError):
        AG.guided_steps(scfg, (2.0, 1.0))


def test_walk_repeats_guided_levels():
    scfg = _scfg(8, "euler", 0.0)
    walk = L.make_walk_cfg(0, (2, 2), None)
    sched = L.walk_steps(scfg, walk)[0]
    t = L.sigma_schedule(scfg)[1]
    g = AG.guided_steps(scfg, (float(t[5]), float(t[2])), 2.0, walk)
    assert len(g) == len(sched) == 16 and np.array_equal(g, (sched >= 2) & (sched <= 5))


@pytest.mark.parametrize("solver,churn", [("heun", 40.0), ("euler", 0.0), ("dpmpp_2m", 0.0)])
def test_expected_guide_forwards(solver, churn):
    T = 8
    scfg = _scfg(T, solver, churn)
    t = L.sigma_schedule(scfg)[1]
    calls = AG.step_calls(scfg)
    assert list(calls) == ([2] * 7 + [1] if solver == "heun" else [1] * 8)
    n = int(calls.sum())
    rng = np.random.default_rng(3)
    for coins in (np.zeros(n, np.uint8), np.ones(n, np.uint8), rng.integers(0, 2, n).astype(np.uint8)):
        assert AG.expected_guide_forwards(scfg, coins, None, 2.0) == n + int(coins.sum())          # every step: what the main network runs
        assert AG.expected_guide_forwards(scfg, coins, None, 1.0) == 0
        assert AG.expected_guide_forwards(scfg, coins, (200.0, 300.0), 2.0) == 0
        assert AG.expected_guide_forwards(scfg, coins, None, 2.0, self_condition=False) == n
        lo, hi = float(t[5]), float(t[2])   # steps 2 .. 5
        first = int(calls[:2].sum())
        inside = int(calls[2:6].sum())
        assert AG.expected_guide_forwards(scfg, coins, (lo, hi), 2.0) == inside + int(coins[first:first + inside].sum())


# ---- the fixture ----
def _combine(m, g, s):
    sm1 = np.float32(s) - np.float32(1.0)
    return (m + sm1 * (m - g).astype(np.float32)).astype(np.float32)


def test_fixture_composite_is_the_float32_combine():
    g = load("autoguide.npz")
    s = float(g["scale"])
    assert s == Y.AUTOGUIDE_SCALE and np.array_equal(g["in/flags"], W.synth_flags(3, 8, Y.AUTOGUIDE_VALID))
    f = g["in/flags"].astype(bool)
    va = np.broadcast_to(f[:, None, :, None] & f[:, None, None, :], (3, 6, 8, 8))
    for si in range(3):
        _, _, adj, node, sca, scn = Y.autoguide_precond_case(si)
        assert np.array_equal(g[f"in/pre{si}_adj"], adj) and np.array_equal(g[f"in/pre{si}_sc_node"], scn)
        for coin in (0, 1):
            key = f"a_s{si}_coin{coin}"
            for part in ("adj", "node"):
                m, gd = g[f"{key}_main_{part}"], g[f"{key}_guide_{part}"]
                assert m.dtype == np.float32 and np.array_equal(g[f"{key}_{part}"], _combine(m, gd, s)), (key, part)
            assert np.all(g[key + "_adj"][~va] == 0) and np.all(g[key + "_node"][~f] == 0)
    for pair in Y.AUTOGUIDE_PAIRS:
        for tag, T, solver, _ in Y.AUTOGUIDE_RUNS:
            assert int(g[f"{pair}_{tag}_coins_used"]) == (T if solver == "euler" else 2 * T - 1)
            assert g[f"{pair}_{tag}_adj"].shape == (3, 6, 8, 8) and np.all(g[f"{pair}_{tag}_adj"][~va] == 0)
    flags, ia, _, na, _, cv = Y.autoguide_sampler_case("t8_heun", 8, "heun")
    assert np.array_equal(g["in/t8_heun_init_adj"], ia) and np.array_equal(g["in/t8_heun_noise_adj"], na)
    assert np.array_equal(g["in/t8_heun_coins"], (cv < 0.5).astype(np.uint8))


def test_the_bar_tells_wrong_composites_apart():
    """D_m and D_g exchanged, s in place of s - 1, a coin that is not shared: each moves the composite beyond the parity bar"""
    g = load("autoguide.npz")
    s = float(g["scale"])
    for si in range(3):
        for coin in (0, 1):
            key = f"a_s{si}_coin{coin}"
            for part in ("adj", "node"):
                ref, m, gd = g[f"{key}_{part}"], g[f"{key}_main_{part}"], g[f"{key}_guide_{part}"]
                other = g[f"a_s{si}_coin{1 - coin}_guide_{part}"]
                wrong = {"exchanged": _combine(gd, m, s), "s for s - 1": _combine(m, gd, s + 1.0), "unshared coin": _combine(m, other, s)}
                for what, w in wrong.items():
                    e = rel_err(w, ref)
                    print(f"AUTOGUIDE power {key} {part} {what}: rel err {e:.3e} (bar {FWD_RTOL:.0e})")
                    assert e > FWD_RTOL, (key, part, what, e)
