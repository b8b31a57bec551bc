"""No GPU: the host side of the second-order multistep solver (solver='dpmpp_2m', DSG_SOLVER_DPMPP_2M) -- dsg_multistep_coef through
lib.multistep_coef against the formula of include/dsg.h restated in NumPy float64, the rules for c_k = 0, the refusals, and the
struct / solver-code plumbing."""
import ctypes as C

import numpy as np
import pytest

from diffusesg_amd import lib


def scfg(T, solver="dpmpp_2m", S_churn=0.0):
    return lib.make_sampler_cfg(T, solver, S_churn)


def walk(s=0, resample=None, rng=None):
    return lib.make_walk_cfg(s, resample, rng)


def expected_coefs(cfg, w):
    """c_k = ln(t_i / t_{i+1}) / (2 ln(t_{i-1} / t_i)) in float64 on the widened float32 levels, rounded once; 0 at k = 0, at index
    T - 1, where the previous executed step was not index i - 1, and where the step draws noise.  Returns (c, why-zero labels)."""
    T = cfg.num_steps
    t = lib.sigma_schedule(cfg)[0].astype(np.float32).astype(np.float64)
    idx, noise = lib.walk_steps(cfg, w)
    c, why = np.zeros(len(idx), np.float32), []
    for k, i in enumerate(idx.tolist()):
        if k == 0:
            why.append("first")
        elif i == T - 1:
            why.append("last index")
        elif idx[k - 1] != i - 1 or noise[k] != 0:
            why.append("jump")
        else:
            why.append("")
            c[k] = np.float32(np.log(t[i] / t[i + 1]) / (np.float64(2.0) * np.log(t[i - 1] / t[i])))
    return c, why


CASES = [(1, walk()), (2, walk()), (8, walk()), (50, walk()), (8, walk(3)), (8, walk(0, (2, 3))), (6, walk(0, (3, 2), (0, 6))),
         (8, walk(0, (3, 2), (0, 6))), (50, walk(7, (6, 2), (9, 44)))]


@pytest.mark.parametrize("T,w", CASES)
def test_coefficients_bit_for_bit(T, w):
    cfg = scfg(T)
    got = lib.multistep_coef(cfg, w)
    want, why = expected_coefs(cfg, w)
    idx, noise = lib.walk_steps(cfg, w)
    assert got.dtype == np.float32 and got.shape == idx.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
    # the zeros: executed step 0, every step at index T - 1, every step behind a jump (it draws the jump-back noise, and its
    # predecessor is not index i - 1); everywhere else a second-order step
    assert got[0] == 0 and np.all(got[idx == T - 1] == 0) and np.all(got[noise != 0] == 0)
    jumps = np.flatnonzero(np.diff(idx) != 1) + 1
    assert np.all(got[jumps] == 0)
    second = np.array([x == "" for x in why])
    assert np.all(got[second] > 0) and np.all(np.isfinite(got))


def test_trivial_walk_is_null_walk_and_counts():
    for T in (1, 2, 8, 50):
        cfg = scfg(T)
        a, b = lib.multistep_coef(cfg), lib.multistep_coef(cfg, walk())
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and len(a) == T
        assert np.count_nonzero(a) == max(T - 2, 0)          # all but the first step and the step to t = 0
    # rho = 7 spaces the levels so that successive log-steps grow: every coefficient is a little above 1/2
    a = lib.multistep_coef(scfg(50))[1:-1]
    assert np.all(a > 0.5) and np.all(a < 1.0)
    # a partial-noise start: its first step is executed step 0
    a = lib.multistep_coef(scfg(8), walk(3))
    assert len(a) == 5 and a[0] == 0 and a[-1] == 0 and np.all(a[1:-1] > 0)
    assert np.array_equal(a[1:-1].view(np.uint32), lib.multistep_coef(scfg(8))[4:-1].view(np.uint32))
    # resample (2, 3) on T = 8: 0 1 | 0 1 | 0 1 | 2 3 | 2 3 | ... -- a repeated pass starts without history, the first pass of a block
    # continues the block before it, and 7 is the last index
    a = lib.multistep_coef(scfg(8), walk(0, (2, 3)))
    F, S = False, True
    assert len(a) == 24 and (a != 0).tolist() == [F, S, F, S, F, S] + [S, S, F, S, F, S] * 2 + [S, F, F, F, F, F]


@pytest.mark.parametrize("solver,churn", [("euler", 0.0), ("euler", 40.0), ("heun", 40.0), ("heun", 0.0)])
def test_other_solvers_get_zeros(solver, churn):
    for w in (None, walk(0, (2, 3))):
        a = lib.multistep_coef(scfg(8, solver, churn), w)
        assert len(a) == (8 if w is None else 24) and np.all(a.view(np.uint32) == 0)


def test_refusals():
    L = lib.load()
    # churn noise at some level: refused at the C level (host helper), by the binding and by the sampler's constructor
    bad = scfg(8, "dpmpp_2m", 40.0)
    assert np.any(lib.sigma_schedule(bad)[2] != 0)
    buf = np.full(8, -7, np.float32)
    assert L.dsg_multistep_coef(C.byref(bad), None, None, 0) == lib.DSG_ERR_INVALID
    assert L.dsg_multistep_coef(C.byref(bad), C.byref(walk()), buf.ctypes.data, 8) == lib.DSG_ERR_INVALID
    assert np.all(buf == -7)
    with pytest.raises(lib.DsgError, match="S_churn = 0"):
        lib.multistep_coef(bad)
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    with pytest.raises(ValueError, match="S_churn = 0"):
        NodeAdjEDMSamplerHip(num_steps=8, solver="dpmpp_2m", S_churn=40.0)
    with pytest.raises(ValueError, match="S_churn = 0"):
        NodeAdjEDMSamplerHip(num_steps=8, solver="dpmpp_2m")                  # the default S_churn is 40
    smp = NodeAdjEDMSamplerHip(num_steps=8, solver="dpmpp_2m", S_churn=0)
    assert smp.solver == "dpmpp_2m" and smp._cfg().heun == 2
    # cap < L: refused, nothing written
    good, w = scfg(8), walk(0, (2, 3))
    buf = np.full(24, -7, np.float32)
    assert L.dsg_multistep_coef(C.byref(good), C.byref(w), buf.ctypes.data, 23) == lib.DSG_ERR_INVALID
    assert np.all(buf == -7)
    assert L.dsg_multistep_coef(C.byref(good), C.byref(w), buf.ctypes.data, 24) == 24 and buf[1] > 0
    assert L.dsg_multistep_coef(C.byref(good), C.byref(w), None, 0) == 24
    # a bad walk, a missing configuration
    assert L.dsg_multistep_coef(C.byref(good), C.byref(walk(9)), None, 0) == lib.DSG_ERR_INVALID
    assert L.dsg_multistep_coef(None, None, None, 0) == lib.DSG_ERR_INVALID
    with pytest.raises(ValueError):
        lib.make_sampler_cfg(8, "dpmpp_3m", 0.0)


def test_structs_solver_codes_and_exports():
    assert C.sizeof(lib.DsgSamplerCfg) == 56
    assert scfg(8, "heun", 40.0).heun == 1 and scfg(8, "euler", 0.0).heun == 0 and scfg(8, "dpmpp_2m", 0.0).heun == 2
    assert lib.SOLVERS == {"euler": 0, "heun": 1, "dpmpp_2m": 2}
    assert "dsg_multistep_coef" in lib.EXPORTS
    assert lib.load().dsg_abi_version() == lib.ABI_VERSION
    # the schedule and the walk do not depend on the solver code
    for f in (lambda c: lib.sigma_schedule(c), lambda c: lib.walk_steps(c, walk(0, (2, 3)))):
        for a, b in zip(f(scfg(8, "euler", 0.0)), f(scfg(8, "dpmpp_2m", 0.0))):
            assert np.array_equal(a, b)
