"""No GPU: the host side of resampling walks -- dsg_walk_steps through lib.walk_steps (sequences, merged jump-back coefficients,
refusals), start_step_for_sigma, and the argument plumbing of diffusesg_amd.complete down to the sampler call."""
import numpy as np
import pytest
import torch

from diffusesg_amd import complete as cmpl
from diffusesg_amd import lib
from diffusesg_amd import spec as S

T6 = 6


def scfg(T=T6, solver="heun", S_churn=40.0):
    return lib.make_sampler_cfg(T, solver, S_churn)


def walk(s=0, resample=None, rng=None):
    return lib.make_walk_cfg(s, resample, rng)


@pytest.mark.parametrize("w,want", [
    (walk(0, (2, 2)), [0, 1, 0, 1, 2, 3, 2, 3, 4, 5, 4, 5]),
    (walk(0, (2, 2), (2, 4)), [0, 1, 2, 3, 2, 3, 4, 5]),
    (walk(1, (2, 2), (1, 0)), [1, 2, 1, 2, 3, 4, 3, 4, 5, 5]),
    (walk(1, (2, 2)), [1, 2, 1, 2, 3, 4, 3, 4, 5, 5]),              # the range defaults to [start_step, T)
    (walk(0, (1, 1)), list(range(6))),
    (walk(0, (4, 1)), list(range(6))),
    (walk(0, (100, 1), (2, 5)), list(range(6))),
    (walk(0, (4, 3)), [0, 1, 2, 3] * 3 + [4, 5] * 3),               # the last block is short
    (walk(0, (5, 2), (3, 3)), list(range(6))),                      # an empty range
    (walk(2, None), [2, 3, 4, 5]),
])
def test_walk_sequences(w, want):
    idx, coef = lib.walk_steps(scfg(), w)
    assert idx.dtype == np.int32 and coef.dtype == np.float32
    assert idx.tolist() == want
    hi = T6 if w.resample_hi <= 0 else w.resample_hi
    assert len(idx) == T6 - w.start_step + (w.n_resample - 1) * (hi - w.resample_lo)


def expected_coefs(cfg, w):
    """the rule of include/dsg.h restated in numpy: the schedule's own float everywhere but at the first step of a repeated pass"""
    T = cfg.num_steps
    sg, _, nz, _ = lib.sigma_schedule(cfg)
    t = np.concatenate([sg.astype(np.float32), np.zeros(1, np.float32)])
    s, j, r, lo = w.start_step, w.jump_len, w.n_resample, w.resample_lo
    hi = T if w.resample_hi <= 0 else w.resample_hi
    idx, coef, jumps = [], [], []
    for i in range(s, lo):
        idx.append(i); coef.append(nz[i]); jumps.append(False)
    for b in range(lo, hi, j):
        e = min(b + j, hi)
        for p in range(r):
            for i in range(b, e):
                jump = p > 0 and i == b
                idx.append(i); jumps.append(jump)
                coef.append(np.float32(np.sqrt(np.float64(t[b]) ** 2 - np.float64(t[e]) ** 2 + np.float64(nz[b]) ** 2)) if jump else nz[i])
    for i in range(hi, T):
        idx.append(i); coef.append(nz[i]); jumps.append(False)
    return np.array(idx, np.int32), np.array(coef, np.float32), np.array(jumps)


@pytest.mark.parametrize("solver,churn", [("heun", 40.0), ("euler", 0.0)])
@pytest.mark.parametrize("T,w", [(6, walk(0, (2, 2))), (6, walk(1, (2, 3), (1, 6))), (8, walk(0, (2, 3))), (6, walk(0, (3, 2), (0, 6))),
                                 (6, walk(0, (4, 3))), (20, walk(0, (10, 3))), (50, walk(7, (6, 2), (9, 44)))])
def test_walk_coefficients_bit_for_bit(solver, churn, T, w):
    cfg = scfg(T, solver, churn)
    idx, coef = lib.walk_steps(cfg, w)
    want_idx, want_coef, jumps = expected_coefs(cfg, w)
    assert np.array_equal(idx, want_idx)
    assert jumps.sum() == (w.n_resample - 1) * len(range(w.resample_lo, T if w.resample_hi <= 0 else w.resample_hi, w.jump_len))
    assert np.array_equal(coef.view(np.uint32), want_coef.view(np.uint32))
    nz = lib.sigma_schedule(cfg)[2]
    assert np.array_equal(coef[~jumps].view(np.uint32), nz[idx[~jumps]].view(np.uint32))   # the very float the schedule returns
    assert np.all(coef[jumps] > 0)          # a jump draws noise even where the schedule's own churn is off
    if churn == 0.0:
        assert np.all(coef[~jumps] == 0)
        # t_e = 0 where the block ends the schedule: without churn the jump from 0 back up to t_b is t_b itself
        sg = lib.sigma_schedule(cfg)[0].astype(np.float32)
        hi = T if w.resample_hi <= 0 else w.resample_hi
        ends = [k for k in np.flatnonzero(jumps) if hi == T and idx[k] + w.jump_len >= T]
        assert len(ends) == (w.n_resample - 1 if hi == T else 0)
        for k in ends:
            assert coef[k] == sg[idx[k]]


@pytest.mark.parametrize("w", [
    walk(-1), walk(6), walk(7),                          # start_step outside [0, T)
    walk(0, (0, 2)), walk(0, (-3, 2)),                   # jump_len < 1
    walk(0, (2, 0)), walk(0, (2, -1)),                   # n_resample < 1
    walk(2, (2, 2), (1, 6)),                             # lo < start_step
    walk(0, (2, 2), (4, 3)),                             # hi < lo
    walk(0, (2, 2), (0, 7)),                             # hi > T
    walk(0, (2, 2), (7, 0)),                             # lo > T
])
def test_walk_range_violations_are_refused(w):
    L = lib.load()
    import ctypes as C
    cfg = scfg()
    assert L.dsg_walk_steps(C.byref(cfg), C.byref(w), None, None, 0) == lib.DSG_ERR_INVALID
    with pytest.raises(lib.DsgError, match=f"status {lib.DSG_ERR_INVALID}.*bad walk"):
        lib.walk_steps(cfg, w)


def test_walk_cap_and_buffer_capacity():
    import ctypes as C
    L = lib.load()
    cfg = scfg(1024, "euler", 0.0)
    assert L.dsg_walk_steps(C.byref(cfg), C.byref(walk(0, (8, 1024))), None, None, 0) == lib.WALK_MAX_STEPS   # exactly the cap
    assert L.dsg_walk_steps(C.byref(cfg), C.byref(walk(0, (8, 1025))), None, None, 0) == lib.DSG_ERR_INVALID
    assert L.dsg_walk_steps(C.byref(cfg), C.byref(walk(0, (8, 2 ** 31 - 1))), None, None, 0) == lib.DSG_ERR_INVALID   # no int32 wrap
    with pytest.raises(lib.DsgError, match="executed steps"):
        lib.walk_steps(cfg, walk(0, (8, 1025)))
    # an output array shorter than L is refused, nothing is written
    idx = np.full(12, -7, np.int32)
    cfg6, w = scfg(), walk(0, (2, 2))
    assert L.dsg_walk_steps(C.byref(cfg6), C.byref(w), idx.ctypes.data, None, 11) == lib.DSG_ERR_INVALID
    assert np.all(idx == -7)
    assert L.dsg_walk_steps(C.byref(cfg6), C.byref(w), idx.ctypes.data, None, 12) == 12 and idx[-1] == 5
    assert L.dsg_walk_steps(None, C.byref(w), None, None, 0) == lib.DSG_ERR_INVALID
    assert L.dsg_walk_steps(C.byref(cfg6), None, None, None, 0) == lib.DSG_ERR_INVALID


def test_structs_and_exports():
    import ctypes as C
    assert C.sizeof(lib.DsgWalkCfg) == 32
    assert "dsg_sample_walk" in lib.EXPORTS and "dsg_walk_steps" in lib.EXPORTS
    assert lib.load().dsg_abi_version() == lib.ABI_VERSION


class StubSampler:
    """records what complete.py hands to sample_known; returns the known tensors as the 'sample'"""

    def __init__(self, sigma_steps=None):
        self.calls = []
        if sigma_steps is not None:
            self.sigma_steps = torch.tensor(sigma_steps, dtype=torch.float64)

    def sample_known(self, net, node_flags, known_adjs, known_nodes, mask_adj, mask_node, **kw):
        self.calls.append(dict(known_adjs=known_adjs, known_nodes=known_nodes, mask_adj=mask_adj, mask_node=mask_node, **kw))
        return known_adjs, known_nodes


def test_start_step_for_sigma():
    smp = StubSampler([80.0, 20.0, 5.0, 1.0, 0.1, 0.002])
    f = cmpl.start_step_for_sigma
    assert f(smp, 100.0) == 0 and f(smp, 80.0) == 0 and f(smp, 79.9) == 1 and f(smp, 5.0) == 2 and f(smp, 4.99) == 3
    assert f(smp, 0.002) == 5
    with pytest.raises(ValueError, match="below"):
        f(smp, 0.001)
    # on the library's own schedule
    sg = lib.sigma_schedule(scfg(8))[0]
    real = StubSampler(sg)
    for i in range(8):
        assert f(real, sg[i]) == i
        assert f(real, sg[i] * (1 + 1e-9)) == i
        if i < 7:
            assert f(real, sg[i] * (1 - 1e-9)) == i + 1


class _Net:
    class model:
        config = S.ModelConfig(max_node_num=4, c_adj=2, c_node=6, depths=(1,), num_heads=(3,), window_size=4, self_condition=True)


@pytest.fixture
def stub_io(monkeypatch):
    """diffusesg_amd.io.encode / decode need the GPU: replaced by shape-correct stand-ins"""
    cfg = _Net.model.config

    def encode(net, q_adj, q_node, bbox, flags, n_adj_type, n_node_type, e_enc, n_enc):
        B, n = q_node.shape
        return (q_adj[:, None].float().expand(B, cfg.c_adj, n, n).contiguous(),
                torch.cat([q_node[:, :, None].float().expand(B, n, cfg.c_node - 4), bbox.float()], -1))

    def decode(net, adj, node, flags, *a, **kw):
        return adj, node, flags

    monkeypatch.setattr(cmpl._io, "encode", encode)
    monkeypatch.setattr(cmpl._io, "decode", decode)


FLAGS = torch.tensor([[1, 1, 1, 0], [1, 1, 0, 0]], dtype=torch.bool)
KNOWN = torch.tensor([[1, 0, 1, 0], [0, 1, 0, 0]], dtype=torch.bool)
Q_ADJ = torch.arange(32, dtype=torch.int32).reshape(2, 4, 4) % 3
Q_NODE = torch.arange(8, dtype=torch.int32).reshape(2, 4)
BBOX = torch.full((2, 4, 4), 0.25)
WALK_KEYS = ("resample", "resample_range", "start_step", "base_adjs", "base_nodes")


def test_complete_passes_the_walk_on(stub_io):
    smp = StubSampler()
    cmpl.complete_scene_graphs(_Net, smp, Q_ADJ, Q_NODE, BBOX, FLAGS, KNOWN, 3, 8, seed=4)
    assert not any(k in smp.calls[-1] for k in WALK_KEYS), "a call without walk arguments must stay on the plain path"
    cmpl.complete_scene_graphs(_Net, smp, Q_ADJ, Q_NODE, BBOX, FLAGS, KNOWN, 3, 8, seed=4, resample=(2, 3), resample_range=(1, 5))
    c = smp.calls[-1]
    assert c["resample"] == (2, 3) and c["resample_range"] == (1, 5) and c["seed"] == 4
    assert "start_step" not in c and "base_adjs" not in c
    cmpl.layout_from_graph(_Net, smp, Q_ADJ, Q_NODE, FLAGS, 3, 8, resample=(4, 2))
    c = smp.calls[-1]
    assert c["resample"] == (4, 2) and "resample_range" not in c
    assert c["mask_node"][..., -4:].sum() == 0 and c["mask_node"][0, :3, :2].all()   # boxes free, labels known
    cmpl.layout_from_graph(_Net, smp, Q_ADJ, Q_NODE, FLAGS, 3, 8)
    assert not any(k in smp.calls[-1] for k in WALK_KEYS)


def test_vary_scene_graphs_plumbing(stub_io):
    smp = StubSampler()
    cmpl.vary_scene_graphs(_Net, smp, Q_ADJ, Q_NODE, BBOX, FLAGS, 3, 8, start_step=3, seed=9)
    c = smp.calls[-1]
    assert c["start_step"] == 3 and c["seed"] == 9 and "resample" not in c and "resample_range" not in c
    assert c["base_adjs"] is c["known_adjs"] and c["base_nodes"] is c["known_nodes"]      # base = the encoded graph
    assert c["base_adjs"].shape == (2, 2, 4, 4) and c["base_nodes"].shape == (2, 4, 6)
    assert c["mask_adj"].sum() == 0 and c["mask_node"].sum() == 0                         # nothing is held
    cmpl.vary_scene_graphs(_Net, smp, Q_ADJ, Q_NODE, BBOX, FLAGS, 3, 8, start_step=2, known_nodes=KNOWN, boxes=False, resample=(2, 2))
    c = smp.calls[-1]
    want_a, want_n = cmpl.completion_masks(_Net.model.config, FLAGS, KNOWN, boxes=False)
    assert torch.equal(c["mask_adj"], want_a) and torch.equal(c["mask_node"], want_n) and want_a.sum() > 0
    assert c["start_step"] == 2 and c["resample"] == (2, 2)
    with pytest.raises(TypeError):
        cmpl.vary_scene_graphs(_Net, smp, Q_ADJ, Q_NODE, BBOX, FLAGS, 3, 8)               # start_step is required
