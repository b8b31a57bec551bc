"""Autoguidance on the host: which steps of a run the library guides and how many forwards its guide network runs,
worked out the way `dsg_sample*` works them out -- no GPU needed.  The attachment itself is `NodeAdjPrecondHip.attach_guide`.

In the loop sigma is batch-uniform, so a step is guided as a whole: iff the scale is not 1 and the float32 `t_hat` of its schedule
index (`dsg_sigma_schedule`) lies in [lo, hi], bounds included, compared as float32.  A guided step runs, per preconditioned call, one
guide forward and one more where the call's coin fired (the guide's own extra self-conditioning pass); a step outside the interval
runs none."""
from __future__ import annotations

import numpy as np

from . import lib as _lib


def sigma_bounds(sigma_range):
    """(lo, hi) as the float32 the library compares with; None: every level"""
    if sigma_range is None:
        return np.float32(-np.inf), np.float32(np.inf)
    lo, hi = np.float32(sigma_range[0]), np.float32(sigma_range[1])
    if np.isnan(lo) or np.isnan(hi) or lo > hi:
        raise ValueError(f"sigma_range = ({lo}, {hi}) needs lo <= hi, neither NaN")
    return lo, hi


def guided_steps(scfg: _lib.DsgSamplerCfg, sigma_range=None, scale: float = 2.0, walk=None) -> np.ndarray:
    """bool [L]: is executed step k of the run (of the walk; None = every schedule index once) autoguided?"""
    _, t_hat, _, _ = _lib.sigma_schedule(scfg)
    sched = np.arange(scfg.num_steps) if walk is None else _lib.walk_steps(scfg, walk)[0]
    lo, hi = sigma_bounds(sigma_range)
    if np.float32(scale) - np.float32(1.0) == 0:
        return np.zeros(len(sched), bool)
    t = t_hat[sched]
    return (t >= lo) & (t <= hi)


def step_calls(scfg: _lib.DsgSamplerCfg, walk=None) -> np.ndarray:
    """int [L]: preconditioned calls of every executed step -- two per Heun step, one for its last schedule index, one otherwise"""
    sched = np.arange(scfg.num_steps) if walk is None else _lib.walk_steps(scfg, walk)[0]
    heun = scfg.heun not in (_lib.SOLVERS["euler"], _lib.SOLVERS["dpmpp_2m"])
    return np.where(heun & (sched != scfg.num_steps - 1), 2, 1)


def expected_guide_forwards(scfg: _lib.DsgSamplerCfg, coins, sigma_range=None, scale: float = 2.0, self_condition: bool = True, walk=None) -> int:
    """`sampler.last_guide_forwards` of a run with these coins (one per preconditioned call, in call order)"""
    guided, calls = guided_steps(scfg, sigma_range, scale, walk), step_calls(scfg, walk)
    coins = np.asarray(coins).astype(bool)
    n, c = 0, 0
    for g, k in zip(guided, calls):
        if g:
            n += int(k) + (int(coins[c:c + k].sum()) if self_condition else 0)
        c += int(k)
    return n
