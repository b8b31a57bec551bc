"""No output of any entry point may depend on what its workspace held before the call ("what a forward may assume about
its workspace").

The forward leaves rows stale on purpose (masked-token pruning, the three pure-window deduplication paths, the list GEMMs), pads
100-token windows to 128 key slots, and never clears most of its ~40 device buffers nor the buffers it allocates on first use.  That is
correct only if no stale or uninitialised element ever reaches an output, and two test hooks of the library make such a read
deterministic:
  Handle.poison(B, pattern, seed)  (dsg_debug_poison)   fills every scratch buffer that exists -- stale contents between two calls;
  option "debug_alloc_fill"                             fills every scratch buffer as it is allocated -- allocator garbage on first use.
Patterns: 1 zeros, 2 quiet NaN (not written into the five "finite" buffers x, y, att, hid, stats), 3 1e30, 4 pseudo-random finite values.
Buffers read as an index, a count, a byte mask, a seed or an address are never filled: their staleness is test C's, with valid contents.

The assertion, everywhere: the call after pattern 1 gives `ref`; after patterns 2, 3 and 4 (two seeds) every output tensor is
torch.equal to it.  No tolerance -- with one documented exception: the gradients of the relative-position bias tables, which the
attention backward accumulates with float atomics in no fixed order (profiles/train_kernel_errors.md), so that two runs after the SAME
pattern already differ in the last bits; they are held to the bar of test_input_grad.py, 8 x max(zeros-against-zeros difference,
2^-20) of the tensor's maximum.  All randomness is recorded (weights.normal / coins) or a counter-based stream of a given seed.

  A  stale contents: warm-up call, then poison / call / compare per pattern -- every entry point, every configuration, every option set
  B  first use: a fresh handle with "debug_alloc_fill" 2 (and 3) set before its weights are finalised; first calls against A's `ref`
  C  stale state: call X with flags F1, then Y with F2 on one workspace against Y on a handle that never ran X
  D  the recorded intermittent failure of test_dedup_batch.py's [vg] case, replayed on a fresh handle under "debug_alloc_fill"
"""
import ctypes as C
import functools

import numpy as np
import pytest

from diffusesg_amd import spec as S
from diffusesg_amd import synth as Y
from diffusesg_amd import weights as W
from test_dedup_batch import _specs as _dd_specs, batches, prefix

pytestmark = pytest.mark.gpu

STEPS = 4                                             # every step-body graph (first / steady / last x coins) is captured and replayed
PATTERNS = ((2, 0), (3, 0), (4, 1), (4, 2))           # (pattern, seed) compared against pattern 1
DEFAULTS = (("fused_merge", 1), ("batch_invariant", 0), ("prune_masked", 1), ("dedup_masked", 1), ("dedup_levels", 0), ("dedup_batch", 1),
            ("dedup_table", 1), ("fused_rowstats", 1), ("fused_readout", 1), ("gemm_bf16", 0), ("bf16_pipe", 1), ("gemm_split", 0),
            ("loop_graph", 1))
CONFIGS = {"s": _dd_specs["s"][0], "d2": _dd_specs["d2"][0], "vg": _dd_specs["vg"][0], "tiny": S.tiny_config, "coco": S.coco_config}
# option sets beyond the defaults; each on one small configuration and on vg (the bf16 block pipeline: vg and coco)
OPTION_SETS = {
    "prune0": (("prune_masked", 0),),
    "dedup0": (("dedup_masked", 0),),
    "batch0_merge2": (("fused_merge", 2), ("dedup_batch", 0)),
    "batch2_merge2": (("fused_merge", 2), ("dedup_batch", 2)),
    "table0": (("fused_merge", 2), ("dedup_batch", 2), ("dedup_table", 0)),
    "invariant": (("batch_invariant", 1),),
    "rowstats0": (("fused_rowstats", 0),),
    "readout0": (("fused_readout", 0),),             # the faithful read-out chain: reuses y and att
    "bf16_pipe": (("gemm_bf16", 1),),
    "bf16_lp": (("gemm_bf16", 1), ("bf16_pipe", 0)),  # the kernels_lp.hip path
    "split": (("gemm_split", 1),),
}
OPTION_CONFIGS = {k: (("vg", "coco") if k == "bf16_pipe" else ("s", "vg")) for k in OPTION_SETS}


def T(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


@functools.lru_cache(maxsize=None)
def cfg_for(name):
    return CONFIGS[name]()


def fresh_net(name, alloc_fill=0):
    """a network on a handle of its own; alloc_fill: "debug_alloc_fill" set before the weights are uploaded and finalised"""
    from diffusesg_amd import lib
    from diffusesg_amd.model import build_network
    cfg = cfg_for(name)
    net = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda")
    if alloc_fill:
        net.model._handle = lib.Handle(cfg)
        net.model._handle.set_option("debug_alloc_fill", alloc_fill)
    net.model._ensure_handle()
    return net


@functools.lru_cache(maxsize=None)
def net_for(name):
    return fresh_net(name)


def flag_sets(name):
    """name -> flags [B, N]: the batches of test_dedup_batch.py (prefixes straddling window edges, an empty and a full graph, scattered,
    no_pure) + B = 1; "s" also B = 16, where the default "dedup_batch" 1 shares one representative; coco at B = 2; tiny (N = 8) its own"""
    n = cfg_for(name).max_node_num
    if name == "tiny":
        sc = np.zeros((3, n), bool)
        sc[0, [1, 6]] = True
        sc[1, [4]] = True
        sc[2, [0, n - 1]] = True
        return {"edges": prefix(n, [3, 4, 5, 8]), "uneven": prefix(n, [6, 0, 8]), "scattered": sc, "one": prefix(n, [5])}
    if name == "coco":
        b = batches(n)
        return {"rep_moves": b["rep_moves"], "no_pure": b["no_pure"], "uneven2": prefix(n, [0, n]), "edges2": prefix(n, [9, 31]),
                "scattered2": b["scattered"][:2], "one": prefix(n, [11])}
    out = dict(batches(n))
    out["one"] = prefix(n, [n // 2 - 3])
    if name == "s":
        out["sixteen"] = prefix(n, [5, 13, 9, 30, 17, 1, 0, 32, 8, 16, 24, 7, 15, 12, 3, 20])
    return out


def reset(h):
    for k, v in DEFAULTS:
        h.set_option(k, v)


# ---- the entry points: fn(net, cfg, flags [B, N] bool, tag) -> list of output tensors -------------------------------------------------
def _shapes(cfg, flags):
    B, n = flags.shape
    return (B, cfg.c_adj, n, n), (B, n, cfg.c_node)


@functools.lru_cache(maxsize=None)
def _normal(seed, name, shape):
    """a recorded N(0, 1) draw on the device, made once and shared: no call writes its inputs"""
    return T(W.normal(seed, name, shape))


def _pair(cfg, flags, tag, what, seed=71):
    sa, sn = _shapes(cfg, flags)
    return _normal(seed, f"poison/{tag}/{what}_adj", sa), _normal(seed, f"poison/{tag}/{what}_node", sn)   # not masked


def _sigmas(B):
    return T(np.geomspace(0.05, 20.0, B).astype(np.float32))


class _Outs(list):
    names = None   # the tensors' names where one of them needs the bias-table exception (e_train, e_block)


def _out(ts):
    import torch
    torch.cuda.synchronize()
    return _Outs(torch.as_tensor(t).detach().clone() for t in ts if t is not None)


def e_denoise(net, cfg, flags, tag):
    B = flags.shape[0]
    a, x = _pair(cfg, flags, tag, "in")
    sa, sx = _pair(cfg, flags, tag, "sc")
    return _out(net.model(a, x, T(flags), T(np.linspace(-1.2, 1.0, B).astype(np.float32)), sa, sx))


def _precond(net, cfg, flags, tag, with_sc, coin):
    import torch
    m = net.model
    h = m._ensure_handle()
    a, x = _pair(cfg, flags, tag, "in")
    sa, sx = _pair(cfg, flags, tag, "sc") if with_sc else (None, None)
    fl, sg = T(flags.astype(np.uint8)), _sigmas(flags.shape[0])
    oa, on = torch.empty_like(a), torch.empty_like(x)
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    st = torch.cuda.current_stream().cuda_stream
    h.check(h.L.dsg_precond(h.raw, flags.shape[0], p(a), p(x), p(fl), p(sg), p(sa), p(sx), int(coin), p(oa), p(on), C.c_void_p(st)), "dsg_precond")
    return _out([oa, on])


def e_precond_sc(net, cfg, flags, tag):
    return _precond(net, cfg, flags, tag, True, 0)


def e_precond_plain(net, cfg, flags, tag):
    return _precond(net, cfg, flags, tag, False, 0)


def e_precond_coin(net, cfg, flags, tag):
    return _precond(net, cfg, flags, tag, False, 1)   # the self-conditioning pass of a fired coin


def _sampler(**kw):
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    return NodeAdjEDMSamplerHip(num_steps=STEPS, self_condition=True, dev="cuda", **kw)


def _coins(tag, n=4 * STEPS):
    return (W.coins(73, f"poison/{tag}", n) < 0.5).astype(np.uint8)


def _kw(cfg):
    return dict(num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj, return_device=True)


def e_sample(net, cfg, flags, tag):
    """dsg_sample: Heun + churn with recorded noise and self-conditioning coins (the step bodies are hipGraphs under "loop_graph" 1)"""
    sa, sn = _shapes(cfg, flags)
    ia, inn = _pair(cfg, flags, tag, "init")
    na = _normal(75, f"poison/{tag}/churn_adj", (STEPS,) + sa)
    nn = _normal(75, f"poison/{tag}/churn_node", (STEPS,) + sn)
    return _out(_sampler().sample(net, T(flags), init_adjs=ia, init_nodes=inn, churn_noise=(na, nn), coins=_coins(tag), **_kw(cfg)))


def e_sample_nograph(net, cfg, flags, tag):
    h = net.model._ensure_handle()
    h.set_option("loop_graph", 0)
    try:
        return e_sample(net, cfg, flags, tag)
    finally:
        h.set_option("loop_graph", 1)


def _known(cfg, flags, tag):
    sa, sn = _shapes(cfg, flags)
    ka, kn = _pair(cfg, flags, tag, "known")
    ma = _normal(77, f"poison/{tag}/mask_adj", sa) > 0.3
    mn = _normal(77, f"poison/{tag}/mask_node", sn) > 0.3
    return ka, kn, ma, mn


def e_known(net, cfg, flags, tag):
    return _out(_sampler().sample_known(net, T(flags), *_known(cfg, flags, tag), seed=31, coins=_coins(tag), **_kw(cfg)))


def e_walk(net, cfg, flags, tag):
    """dsg_sample_walk: partial-noise start at index 1 and one resampling jump (block (1, 3) run twice: 5 executed steps)"""
    ba, bn = _pair(cfg, flags, tag, "base")
    return _out(_sampler().sample_known(net, T(flags), *_known(cfg, flags, tag), seed=31, coins=_coins(tag), start_step=1, base_adjs=ba,
                                        base_nodes=bn, resample=(2, 2), resample_range=(1, 3), **_kw(cfg)))


def e_seeded(net, cfg, flags, tag):
    B = flags.shape[0]
    return _out(_sampler().sample(net, T(flags), graph_seeds=[5 + 3 * b + (2 ** 40 if b == 1 else 0) for b in range(B)], coins=_coins(tag),
                                  **_kw(cfg)))


def e_multistep(net, cfg, flags, tag):
    return _out(_sampler(solver="dpmpp_2m", S_churn=0.0).sample(net, T(flags), seed=17, coins=_coins(tag), **_kw(cfg)))


def e_ode(net, cfg, flags, tag):
    """dsg_ode_run: Heun, encode, a device-drawn Rademacher probe (forward + input-gradient backward per evaluation)"""
    from diffusesg_amd import ode
    a, x = _pair(cfg, flags, tag, "in")
    B = flags.shape[0]
    oa, on, tr, pr = ode.run(net, _sampler(S_churn=0.0), a, x, T(flags), "encode", "rademacher", graph_seeds=[9 + b for b in range(B)],
                             return_probe=True)
    return _out([oa, on, tr, *pr])


def e_vjp(net, cfg, flags, tag):
    a, x = _pair(cfg, flags, tag, "in")
    sa, sx = _pair(cfg, flags, tag, "sc")
    ga, gn = _pair(cfg, flags, tag, "cot")
    out = net.value_and_input_grad(a, x, T(flags), _sigmas(flags.shape[0]), grad_outputs=(ga, gn), self_cond_adjs=sa, self_cond_nodes=sx,
                                   coin=False)
    return _out(out)


class _Loss:
    edge_loss_weight = 1.0
    node_loss_weight = 1.0


RPB = "relative_position_bias_table"


def e_train(net, cfg, flags, tag):
    """dsg_train_self_cond (the coin fires) + dsg_train_step_grads -> D, the two losses, then every parameter gradient in key order;
    the names of the tensors go along for the bias-table exception"""
    from diffusesg_amd.train import train_step_grads
    a, x = _pair(cfg, flags, tag, "in")
    ta, tx = _pair(cfg, flags, tag, "target")
    B = flags.shape[0]
    real = np.random.rand
    np.random.rand = lambda: 0.1
    try:
        oa, on, la, ln, grads = train_step_grads(net, _Loss(), a, x, T(flags), _sigmas(B), ta, tx, T(np.linspace(0.5, 2.0, B).astype(np.float32)))
    finally:
        np.random.rand = real
    keys = sorted(grads)
    out = _out([oa, on, la, ln] + [grads[k] for k in keys])
    out.names = ["D_adj", "D_node", "loss_adj", "loss_node"] + keys
    return out


def e_block(net, cfg, flags, tag):
    """dsg_block_train, forward and backward of the first block (its scratch is the call's own: only "debug_alloc_fill" reaches it)"""
    from diffusesg_amd.train import BLOCK_PARAM_NAMES, swin_block_train
    blk = "down_layers.0.blocks.0"
    x, emb, dy = Y.block_case(cfg, blk, flags.shape[0])
    x_out, gx, ge, grads = swin_block_train(net.model, blk, T(x), T(emb), T(dy))
    out = _out([x_out, gx, ge] + [grads[k] for k in BLOCK_PARAM_NAMES])
    out.names = ["x_out", "grad_x", "grad_emb"] + list(BLOCK_PARAM_NAMES)
    return out


ENTRIES = {"denoise": e_denoise, "precond_sc": e_precond_sc, "precond_plain": e_precond_plain, "precond_coin": e_precond_coin,
           "sample": e_sample, "sample_nograph": e_sample_nograph, "known": e_known, "walk": e_walk, "seeded": e_seeded,
           "multistep": e_multistep, "ode": e_ode, "vjp": e_vjp, "train": e_train, "block": e_block}
FORWARD_ENTRIES = ("denoise", "precond_sc", "precond_plain", "precond_coin", "sample", "sample_nograph", "known", "walk", "seeded", "multistep")
TRAIN_ENTRIES = ("ode", "vjp", "train", "block")      # training-form kernels: their smallest configurations, 4 x 4 and 8 x 8 windows
CASES_A = [(c, e) for c in CONFIGS for e in FORWARD_ENTRIES] + [(c, e) for c in ("tiny", "s") for e in TRAIN_ENTRIES]


def check_equal(got, ref, what, again=None):
    """every tensor torch.equal; the bias-table gradients (float atomics) at 8 x max(their zeros-against-zeros difference, 2^-20)"""
    import torch
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        name = ref.names[i] if ref.names else str(i)
        if ref.names and name.endswith(RPB):
            s = max(float(r.abs().max()), 1e-30)
            d_plain = float((again[i] - r).abs().max()) / s if again is not None else 0.0
            d = float((g - r).abs().max()) / s
            assert d <= 8 * max(d_plain, 2.0 ** -20), f"{what}: {name} differs by {d:.2e} of its maximum (two plain runs: {d_plain:.2e})"
        else:
            # bit for bit where torch.equal says no: a NaN that is in `ref` too (the loss of a graph without a valid node is 0 / 0)
            bits = {4: torch.int32, 8: torch.int64}[r.element_size()]
            assert torch.equal(g, r) or torch.equal(g.contiguous().view(bits), r.contiguous().view(bits)), f"{what}: output {name} differs from the run after a zero fill " \
                                      f"({int((g != r).sum())} of {r.numel()} elements, {int(torch.isnan(g).sum())} NaN)"


def poisoned_runs(net, cfg, name, entry, fl_name, flags, what):
    """pattern 1 -> ref; patterns 2, 3, 4 (two seeds) must reproduce it"""
    h = net.model._ensure_handle()
    B = flags.shape[0]
    tag = f"{name}/{fl_name}"
    fn = ENTRIES[entry]
    fn(net, cfg, flags, tag)   # warm-up: every first-use buffer of this call exists, its step bodies are captured
    h.poison(B, 1)
    ref = fn(net, cfg, flags, tag)
    again = None
    if ref.names:
        h.poison(B, 1)
        again = fn(net, cfg, flags, tag)
    for pattern, seed in PATTERNS:
        h.poison(B, pattern, seed)
        check_equal(fn(net, cfg, flags, tag), ref, f"{what} {entry} {tag} after pattern {pattern} (seed {seed})", again)
    return ref


# ---- A: stale contents -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,entry", CASES_A, ids=[f"{c}-{e}" for c, e in CASES_A])
def test_a_stale_contents_default_options(name, entry):
    cfg, net = cfg_for(name), net_for(name)
    reset(net.model._ensure_handle())
    for fl_name, flags in flag_sets(name).items():
        poisoned_runs(net, cfg, name, entry, fl_name, flags, "defaults:")


CASES_OPT = [(o, c) for o in OPTION_SETS for c in OPTION_CONFIGS[o]]


@pytest.mark.parametrize("opts,name", CASES_OPT, ids=[f"{o}-{c}" for o, c in CASES_OPT])
def test_a_stale_contents_option_sets(opts, name):
    """the sampler (step graphs, batch-uniform row, every deduplication path), dsg_denoise (per-sample rows, every window unique) and the
    self-conditioning pass of dsg_precond under every option set that selects other kernels or other lists"""
    cfg, net = cfg_for(name), net_for(name)
    h = net.model._ensure_handle()
    try:
        reset(h)
        for k, v in OPTION_SETS[opts]:
            h.set_option(k, v)
        for fl_name, flags in flag_sets(name).items():
            for entry in ("sample", "denoise", "precond_coin"):
                poisoned_runs(net, cfg, name, entry, fl_name, flags, f"{opts}:")
    finally:
        reset(h)


# ---- B: first use ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [2, 3])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_b_first_use_of_a_fresh_handle(name, fill):
    """Every buffer that comes into existence inside these calls -- the workspace, the step tables, the table of pure-window rows, the
    known / seed buffers, the training arenas, dsg_block_train's scratch -- starts as NaN (as 1e30) instead of allocator garbage.  Each
    entry runs on another flag set, so most of them also meet a batch size the handle has not seen."""
    cfg, ref_net = cfg_for(name), net_for(name)
    reset(ref_net.model._ensure_handle())
    sets = list(flag_sets(name).items())
    entries = FORWARD_ENTRIES + (TRAIN_ENTRIES if name in ("tiny", "s") else ())
    net = fresh_net(name, alloc_fill=fill)
    try:
        assert net.model._handle.get_option("debug_alloc_fill") == fill
        for i, entry in enumerate(entries):
            fl_name, flags = sets[i % len(sets)]
            tag = f"{name}/{fl_name}"
            got = ENTRIES[entry](net, cfg, flags, tag)
            h = ref_net.model._ensure_handle()
            h.poison(flags.shape[0], 1)
            ref = ENTRIES[entry](ref_net, cfg, flags, tag)
            again = None
            if ref.names:
                h.poison(flags.shape[0], 1)
                again = ENTRIES[entry](ref_net, cfg, flags, tag)
            check_equal(got, ref, f"first use under debug_alloc_fill {fill}: {entry} {tag}", again)
    finally:
        net.model._handle.close()


# ---- C: stale state --------------------------------------------------------------------------------------------------------------------
def flag_pairs(name):
    """(F1, F2) of one batch size: all live then mostly padded and the reverse; the scattered and the no_pure masks against prefixes"""
    n = cfg_for(name).max_node_num
    f = flag_sets(name)
    full3, pad3 = np.ones((3, n), bool), prefix(n, [3, 0, n // 2 + 1])
    pairs = [("live>padded", full3, pad3), ("padded>live", pad3, full3), ("scattered>uneven", f["scattered"], f["uneven"]),
             ("uneven>scattered", f["uneven"], f["scattered"])]
    if "no_pure" in f:
        pairs += [("no_pure>rep_moves", f["no_pure"], f["rep_moves"]), ("rep_moves>no_pure", f["rep_moves"], f["no_pure"])]
    return pairs


CALL_PAIRS = (("known", "sample"), ("seeded", "sample"), ("ode", "precond_coin"), ("train", "denoise"))
CASES_C = [(c, x, y) for c in ("s", "vg") for x, y in CALL_PAIRS[:2]] + [(c, x, y) for c in ("tiny", "s") for x, y in CALL_PAIRS[2:]]


@pytest.mark.parametrize("name,x,y", CASES_C, ids=[f"{c}-{x}-then-{y}" for c, x, y in CASES_C])
def test_c_stale_state_of_an_earlier_call(name, x, y):
    """flags, need lists, representatives, the control block, known masks, seeds and step rows are never poisoned (a wrong index is a
    fault): here they are stale but valid -- left by call X under flags F1 -- and call Y under F2 must not notice"""
    cfg = cfg_for(name)
    pairs = flag_pairs(name)
    clean = fresh_net(name)           # never runs X
    try:
        ref = {}
        for what, _f1, f2 in pairs:
            clean.model._handle.poison(f2.shape[0], 1)
            ref[what] = ENTRIES[y](clean, cfg, f2, f"{name}/c/{what}")
    finally:
        clean.model._handle.close()
    net = net_for(name)
    reset(net.model._ensure_handle())
    for what, f1, f2 in pairs:
        ENTRIES[x](net, cfg, f1, f"{name}/c/{what}/x")
        check_equal(ENTRIES[y](net, cfg, f2, f"{name}/c/{what}"), ref[what], f"{y} after {x} ({name}, {what})")


# ---- D: the recorded intermittent failure ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [2, 3])
def test_d_dedup_batch_vg_scenario_on_a_fresh_handle(fill):
    """test_dedup_batch.py::test_sampler_bit_identical_across_batch_and_per_graph_and_off[vg] has failed intermittently in whole-suite
    runs ("vg edges: dedup_batch 0 ... differs from dedup_masked 0", profiles/README.md r9, r11, r14).  Its calls in its order, on a
    handle whose every scratch allocation starts as NaN (as 1e30): the "dedup_masked" 0 reference first, on never-used workspaces, then
    "dedup_batch" 0 and 2 with the all-live poisoning sample between the cases."""
    import torch
    import test_dedup_batch as D
    cfg = cfg_for("vg")
    n, depth = cfg.max_node_num, _dd_specs["vg"][1]
    net = fresh_net("vg", alloc_fill=fill)
    h = net.model._handle
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    smp = NodeAdjEDMSamplerHip(num_steps=D.STEPS, self_condition=True, dev="cuda")   # that test's sampler: Heun + churn, hipGraph on
    try:
        cases = {k: D.sample_case(cfg, f, 53, f"dedup_batch/vg/{k}") for k, f in batches(n).items()}
        poison = {B: D.sample_case(cfg, np.ones((B, n), bool), 55, f"dedup_batch/vg/poison{B}") for B in {len(f) for f in batches(n).values()}}
        h.set_option("fused_merge", 2)
        h.set_option("dedup_masked", 0)
        ref = {k: D.run(smp, net, cfg, c) for k, c in cases.items()}
        h.set_option("dedup_masked", 1)
        assert h.get_option("dedup_levels") == depth
        for first, second in ((0, 2), (2, 0)):
            h.set_option("dedup_levels", 0)
            h.set_option("dedup_batch", first)
            for mode in (first, second):
                h.set_option("dedup_batch", mode)
                for k, c in cases.items():
                    B = c["flags"].shape[0]
                    D.run(smp, net, cfg, poison[B])
                    got = D.run(smp, net, cfg, c)
                    assert torch.equal(got[0], ref[k][0]) and torch.equal(got[1], ref[k][1]), \
                        f"vg {k}: dedup_batch {mode} (graphs captured under {first}) differs from dedup_masked 0 under debug_alloc_fill {fill}"
        # ... and the reference itself is what a warm, zero-filled handle gives
        warm = net_for("vg")
        wh = warm.model._ensure_handle()
        try:
            reset(wh)
            wh.set_option("fused_merge", 2)
            for k, c in cases.items():
                wh.poison(c["flags"].shape[0], 1)
                r = D.run(smp, warm, cfg, c)
                assert torch.equal(r[0], ref[k][0]) and torch.equal(r[1], ref[k][1]), f"vg {k}: the dedup_masked 0 reference of the fresh handle"
        finally:
            reset(wh)
    finally:
        h.close()
