"""GPU: masked-token pruning of the up path (option "prune_masked", include/dsg.h).

DiffuseSG.forward masks everything it returns with the node flags, window attention does not; so on the way back up a token is
needed only if it lies in a window that a needed token of the next stage lies in.  The library derives lists of needed 8-token runs /
windows on the device and its up-path kernels compute only those.  Checked here, all through the C ABI:
  1. results are bit-identical (torch.equal) to the same handle with the option off -- forward and sampler, ragged / non-prefix /
     all-false / all-true flags, with and without self-conditioning, stale activations in the workspace, reused captured graphs;
  2. the device-side lists are the sets that a NumPy restatement of the rule below gives;
  3. the pruned forward meets the oracle on fresh inputs at the bar of the existing fresh-input test (FWD_RTOL).
"""
import numpy as np
import pytest
import torch

from diffusesg_amd import spec as S
from diffusesg_amd import synth as Y
from diffusesg_amd import weights as W
from util import FWD_RTOL, assert_close

pytestmark = pytest.mark.gpu

WS = 8
# the smallest nets that reach every kernel that takes a list (window 8):
#   a: fused_attn96, fused_mlp<96>, breakup_ln, the post_linear GEMM, the read-out -- one needed window out of four
#   b: the row-mapped GEMMs (pre_linear, post_linear, proj, fc1, fc2) and the QKV + attention window list at C = 192
#   c: the "rows pruned, attention full" block (shifted partition on a 2 x 2 window grid) and the untouched blocks in front of it
SHAPES = {
    "a": dict(n=16, depths=(1, 1), heads=(3, 6), B=3),
    "b": dict(n=32, depths=(1, 1, 1), heads=(3, 6, 12), B=3),
    "c": dict(n=32, depths=(1, 3, 1), heads=(3, 6, 12), B=2),
}
_cfgs, _nets = {}, {}


def cfg_for(name):
    if name not in _cfgs:
        if name == "vg":
            _cfgs[name] = S.vg_config()
        else:
            s = SHAPES[name]
            _cfgs[name] = S.ModelConfig(max_node_num=s["n"], c_adj=3, c_node=5, depths=s["depths"], num_heads=s["heads"],
                                        window_size=WS, self_condition=True)
    return _cfgs[name]


def net_for(name):
    from diffusesg_amd.model import build_network
    if name not in _nets:
        cfg = cfg_for(name)
        _nets[name] = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")
    return _nets[name]


def T(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def flag_patterns(n, B):
    """name -> flags [B, n]: a ragged prefix batch, a non-prefix pattern, a batch with an all-false graph, an all-true batch"""
    ragged = W.synth_flags(B, n, [n // 2 - 1, 3, n][:B] if B >= 3 else [n // 2 - 1, 3])
    scattered = np.zeros((B, n), bool)
    scattered[:, [1, 9, 10]] = True
    scattered[B - 1] = False
    scattered[B - 1, [n - 2]] = True
    empty = ragged.copy()
    empty[0] = False
    return {"ragged": ragged, "scattered": scattered, "empty": empty, "full": np.ones((B, n), bool)}


def inputs(cfg, flags, seed, tag):
    B, n = flags.shape
    adj = W.mask_adj(W.normal(seed, f"{tag}/adj", (B, cfg.c_adj, n, n)), flags)
    node = W.mask_node(W.normal(seed, f"{tag}/node", (B, n, cfg.c_node)), flags)
    sc_adj = W.mask_adj(W.normal(seed, f"{tag}/sc_adj", (B, cfg.c_adj, n, n)), flags)
    sc_node = W.mask_node(W.normal(seed, f"{tag}/sc_node", (B, n, cfg.c_node)), flags)
    return adj, node, sc_adj, sc_node


def set_prune(net, on):
    h = net.model._ensure_handle()
    h.set_option("prune_masked", int(on))
    assert h.get_option("prune_masked") == int(on)
    return h


# ---- 2. the rule, restated on token masks ----------------------------------------------------------------------------------
def to_runs(mask):
    """token mask [res, res] -> run mask [res, res / 8]: a run is 8 consecutive tokens of one grid row"""
    res = mask.shape[0]
    return mask.reshape(res, res // 8, 8).any(axis=2)


def from_runs(runs):
    return np.repeat(runs, 8, axis=1)


def windows_of(mask, shift):
    """windows (wi, wj) of the cyclically shifted 8 x 8 partition that contain a needed token, and all tokens of those windows"""
    res = mask.shape[0]
    nwr = res // WS
    win = np.zeros((nwr, nwr), bool)
    out = np.zeros_like(mask)
    for wi in range(nwr):
        for wj in range(nwr):
            ti = (wi * WS + np.arange(WS) + shift) % res
            tj = (wj * WS + np.arange(WS) + shift) % res
            if mask[np.ix_(ti, tj)].any():
                win[wi, wj] = True
                out[np.ix_(ti, tj)] = True
    return win, out


def expected_lists(cfg, flags):
    """{(kind, stage, block): set of entries} for a batch, by the rule of the module docstring.  block >= 0: a Swin block of up
    stage `stage` ('runs': its proj / MLP rows, 'windows': its attention); -1: the stage's post_linear rows; -2: its pre_linear /
    breakup rows on the coarser grid.  The walk ends at the first block whose attention structurally needs everything."""
    L, N = len(cfg.depths), cfg.max_node_num
    exp = {}

    def add(key, b, ids, per):
        exp.setdefault(key, set()).update(int(b * per + k) for k in ids)
    for b, f in enumerate(flags):
        cur = from_runs(to_runs(np.outer(f, f)))   # last-level output need: runs that contain a valid pair
        stop = False
        for i in range(L - 1, -1, -1):
            lvl = L - 1 - i
            res = N >> lvl
            for j in range(cfg.depths[lvl] - 1, -1, -1):
                shift = 0 if (res <= WS or j % 2 == 0) else WS // 2
                add(("runs", i, j), b, np.flatnonzero(to_runs(cur)), res * res // 8)
                nwr = res // WS
                if nwr == 1 or (shift > 0 and nwr == 2):
                    stop = True
                    break
                win, cur = windows_of(cur, shift)
                add(("windows", i, j), b, np.flatnonzero(win), nwr * nwr)
            if stop or i == 0:
                break
            add(("runs", i, -1), b, np.flatnonzero(to_runs(cur)), res * res // 8)
            parents = cur.reshape(res // 2, 2, res // 2, 2).any(axis=(1, 3))
            cur = from_runs(to_runs(parents))
            add(("runs", i, -2), b, np.flatnonzero(to_runs(cur)), (res // 2) ** 2 // 8)
        # (keys that never received an entry for any sample still have to exist: see below)
    return exp


def check_lists(name, flags):
    cfg = cfg_for(name)
    net = net_for(name)
    h = set_prune(net, 1)
    adj, node, _, _ = inputs(cfg, flags, 5, f"lists/{name}")
    net.model(T(adj), T(node), T(flags), T(np.zeros(len(flags), np.float32)))
    got = h.need_lists(len(flags))
    assert got, "no need lists for a window-8 configuration"
    exp = expected_lists(cfg, flags)
    seen = set()
    for r in got:
        key = (r["kind"], r["stage"], r["block"])
        seen.add(key)
        ents = [int(e) for e in r["entries"]]
        assert len(set(ents)) == len(ents), f"{name} {key}: duplicate entries"
        assert set(ents) == exp.get(key, set()), f"{name} {key}: device list differs from the rule"
    assert {k for k, v in exp.items() if v} <= seen
    return got


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_need_lists_match_the_rule(name):
    s = SHAPES[name]
    for pat, flags in flag_patterns(s["n"], s["B"]).items():
        got = check_lists(name, flags)
        if pat == "full":
            assert all(len(r["entries"]) == r["full"] for r in got), "all-true flags must need everything"
    # one all-false batch: every count is 0
    got = check_lists(name, np.zeros((s["B"], s["n"]), bool))
    assert all(len(r["entries"]) == 0 for r in got)


def test_need_shares_at_the_headline_shape():
    """N = 64, depths (1, 1, 3, 1): with k = ceil(valid / 8), the level-0 windows need (k/8)^2 of their rows (its MLP only the runs with a valid pair), the level-1 block
    (ceil(k/2)/4)^2, level-2 block 2 (ceil(ceil(k/2)/2)/2)^2 -- 25 % everywhere at valid = 30, 14 % at level 0 for valid = 20,
    39 % / 56 % for valid = 40, everything at 64 -- and the level-2 block 1 keeps its whole attention."""
    valid = [8, 20, 30, 40, 64]
    flags = W.synth_flags(len(valid), 64, valid)
    got = check_lists("vg", flags)
    by_key = {(r["kind"], r["stage"], r["block"]): r for r in got}
    assert ("windows", 1, 1) not in by_key and ("runs", 1, 0) not in by_key and not any(k[1] == 0 for k in by_key)

    def share(key, b):
        r = by_key[key]
        per = r["full"] // len(valid)
        return float(np.sum(r["entries"] // per == b)) / per
    for b, v in enumerate(valid):
        k = -(-v // 8)
        k1 = -(-k // 2)
        k2 = -(-k1 // 2)
        l0, l1, l2 = (k / 8) ** 2, (k1 / 4) ** 2, (k2 / 2) ** 2
        want = {("runs", 3, 0): v * k / 512, ("windows", 3, 0): l0, ("runs", 3, -1): l0,    # level 0: MLP rows (v rows of k runs), attention, post_linear
                ("runs", 3, -2): 4 * k * k1 / 128, ("runs", 2, 0): 4 * k * k1 / 128,        # parents [0, 4k)^2: 4k rows of k1 runs
                ("windows", 2, 0): l1, ("runs", 2, -1): l1,                                 # level 1
                ("runs", 2, -2): 4 * k1 * k2 / 32, ("runs", 1, 2): 4 * k1 * k2 / 32,        # parents [0, 4 k1)^2: 4 k1 rows of k2 runs
                ("windows", 1, 2): l2, ("runs", 1, 1): l2}                                  # level 2: block 2's windows, block 1's rows
        for key, w in want.items():
            assert share(key, b) == pytest.approx(w, abs=1e-12), (v, key)
    assert share(("windows", 3, 0), 2) == 0.25 and share(("windows", 2, 0), 2) == 0.25 and share(("runs", 1, 1), 2) == 0.25


# ---- 1. bit-identity against the unpruned path ------------------------------------------------------------------------------
def forward_pair(net, cfg, flags, seed, tag, sc):
    adj, node, sc_adj, sc_node = inputs(cfg, flags, seed, tag)
    c_noise = np.linspace(-1.4, 1.1, len(flags)).astype(np.float32)
    args = (T(adj), T(node), T(flags), T(c_noise)) + ((T(sc_adj), T(sc_node)) if sc else ())
    return lambda: [t.clone() for t in net.model(*args)]


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_forward_bit_identical_to_unpruned(name):
    cfg, net, s = cfg_for(name), net_for(name), SHAPES[name]
    pats = flag_patterns(s["n"], s["B"])
    runs = {(pat, sc): forward_pair(net, cfg, flags, 17, f"prune/{name}/{pat}", sc) for pat, flags in pats.items() for sc in (False, True)}
    poison = forward_pair(net, cfg, pats["full"], 99, f"prune/{name}/poison", True)
    set_prune(net, 0)
    ref = {k: run() for k, run in runs.items()}
    h = set_prune(net, 1)
    for k, run in runs.items():
        oa, on = run()
        assert torch.equal(oa, ref[k][0]) and torch.equal(on, ref[k][1]), f"{name} {k}: pruned forward differs"
        if k[0] == "ragged":
            assert any(len(r["entries"]) < r["full"] for r in h.need_lists(s["B"])), "nothing was pruned"
    # stale rows are not read: a forward with other inputs and all-true flags rewrites every activation row in between
    for k in (("ragged", True), ("scattered", False), ("empty", True)):
        poison()
        oa, on = runs[k]()
        assert torch.equal(oa, ref[k][0]) and torch.equal(on, ref[k][1]), f"{name} {k}: stale rows were read"


# ---- 3. the oracle ----------------------------------------------------------------------------------------------------------
def test_pruned_forward_vs_oracle():
    from oracle.oracle import Oracle
    cfg, net, s = cfg_for("b"), net_for("b"), SHAPES["b"]
    flags = flag_patterns(s["n"], s["B"])["ragged"]
    adj, node, sc_adj, sc_node = inputs(cfg, flags, 23, "prune/oracle")
    c_noise = np.array([-1.5, 0.1, 1.09], np.float32)
    ra, rn = Oracle(cfg, W.synth_state_dict(cfg, 0)).forward(adj, node, flags, c_noise, sc_adj, sc_node)
    set_prune(net, 1)
    oa, on = net.model(T(adj), T(node), T(flags), T(c_noise), T(sc_adj), T(sc_node))
    assert_close(oa.cpu().numpy(), ra, FWD_RTOL, "pruned adj vs oracle")
    assert_close(on.cpu().numpy(), rn, FWD_RTOL, "pruned node vs oracle")


# ---- 4. the sampler: batch-uniform noise labels, captured step bodies reused across flags ------------------------------------
@pytest.mark.parametrize("name,steps", [("a", 8), ("c", 3)])
def test_sampler_bit_identical_and_graphs_reused(name, steps):
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    cfg, net, s = cfg_for(name), net_for(name), SHAPES[name]
    n, B = s["n"], s["B"]
    smp = NodeAdjEDMSamplerHip(num_steps=steps, self_condition=True, dev="cuda")   # Heun + churn, hipGraph on

    def run(valid, seed):
        flags, ia, inn, na, nn, cv = Y.sampler_case(cfg, steps, B, valid, seed, f"prune/smp/{name}")
        out = smp.sample(net, T(flags), init_adjs=T(ia), init_nodes=T(inn), churn_noise=(T(na), T(nn)), coins=(cv < 0.5).astype(np.uint8),
                         num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj)
        return [torch.as_tensor(t).clone() for t in out]
    first, second = [n // 2 - 2, 3, n], [n, 2, n // 2 + 1]
    set_prune(net, 0)
    ref1, ref2 = run(first, 31), run(second, 31)
    set_prune(net, 1)
    got1 = run(first, 31)
    replays = smp.last_stats
    got2 = run(second, 31)   # other flags, same handle: the captured step bodies are replayed with new lists
    for got, ref, what in ((got1, ref1, "first"), (got2, ref2, "second (graphs reused)")):
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), f"{name}: {what} sample call differs"
    assert replays is not None
