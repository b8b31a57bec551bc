"""GPU: dsg_set_option / dsg_get_option / the DSG_* environment defaults on a handle (include/dsg.h; the table itself: tests/test_options_host.py).

  1. round trip: get(set(v)) for probes v in {-1, 0, 1, 2, 3, 7, 100} equals the option's rule, written out below as a literal, on a
     handle that is not finalized (no weights hook, no validation); the bf16_* options under "gemm_bf16" 1, where they are reported;
     "debug_alloc_fill" refuses what lies outside 0..4 and keeps its value; an unknown name is refused.
  2. a rejected option restores the WHOLE option set: "batch_invariant" 1 is refused where the fused read-out is in use and N * N is
     not a multiple of 32 (here 20 * 20 = 400 = 12 * 32 + 16; the rule sits in the read-out stage and is documented with the option).
     Every value dsg_get_option reports is the same before and after, the forward gives the same bits, and under "gemm_bf16" 1 the
     int-valued "bf16_qkv_attn" 2 stays 2 (a snapshot that kept it as a truth value gave 1 back).
  3. environment defaults, in a fresh child process: flags, integers, and values outside an option's range are brought into it like
     dsg_set_option's.  The dedup_* options report 0 wherever the deduplication does not run -- in the bf16 mode, without the fused
     C = 96 attention, for windows other than 8 x 8 -- so the child reads them back on the N = 32 network of tests/test_dedup_table.py
     after switching "gemm_bf16" off and "fused_attn" on.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from diffusesg_amd import lib
from diffusesg_amd import spec as S
from diffusesg_amd import synth as Y
from diffusesg_amd import weights as W
from test_options_host import NAMES, TABLE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBES = (-1, 0, 1, 2, 3, 7, 100)
FLAG = (1, 0, 1, 1, 1, 1, 1)
REFUSED = None
# what dsg_get_option reports after dsg_set_option(name, probe), probe by probe
STORED = {
    "fused_attn": FLAG, "fused_mlp": FLAG, "fused_readout": FLAG, "fused_patch_embed": FLAG, "fused_rowstats": FLAG, "fused_qkv_attn": FLAG,
    "fused_mlp_maxc": PROBES,
    "fused_merge": (1, 0, 1, 2, 2, 2, 2),
    "loop_graph": FLAG, "batch_invariant": FLAG, "gemm_split": FLAG,
    "debug_alloc_fill": (REFUSED, 0, 1, 2, 3, REFUSED, REFUSED),
}
# the same under "gemm_bf16" 1 (E = 96: the block pipeline runs unless "bf16_pipe" is 0); "bf16_act" is reported where it does not run
UNDER_BF16 = {
    "gemm_bf16": FLAG,
    "bf16_pipe": FLAG,
    "bf16_mlp": (0, 0, 1, 2, 3, 6, 6),
    "bf16_qkv_attn": (0, 0, 1, 2, 3, 3, 3),
    "bf16_proj_mlp": FLAG,
    "bf16_readout": FLAG,
}
BF16_ACT_NO_PIPE = (0, 0, 1, 2, 2, 2, 2)
DEFAULTS = {r[0]: r[2] for r in TABLE}


def T(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def round_trip(h, name, expect):
    for v, want in zip(PROBES, expect):
        if want is REFUSED:
            before = h.get_option(name)
            with pytest.raises(lib.DsgError, match=r"0 \(off\) or a pattern 1..4"):
                h.set_option(name, v)
            assert h.get_option(name) == before, (name, v)
        else:
            h.set_option(name, v)
            assert h.get_option(name) == want, (name, v)
    h.set_option(name, DEFAULTS[name])


@pytest.mark.gpu
def test_set_get_round_trip():
    h = lib.Handle(S.tiny_config())   # not finalized: no weights hook, no validation
    try:
        assert {n: h.get_option(n) for n in STORED} == {n: DEFAULTS[n] for n in STORED}
        for name, expect in STORED.items():
            round_trip(h, name, expect)
        h.set_option("gemm_bf16", 1)
        for name, expect in UNDER_BF16.items():
            round_trip(h, name, expect)
            h.set_option("gemm_bf16", 1)
        assert h.get_option("bf16_act") == 0   # the pipeline runs: the option does not act
        h.set_option("bf16_pipe", 0)
        round_trip(h, "bf16_act", BF16_ACT_NO_PIPE)
        unknown = "no_such_option"
        with pytest.raises(lib.DsgError, match="unknown option"):
            h.set_option(unknown, 1)
        with pytest.raises(lib.DsgError, match="unknown option"):
            h.get_option(unknown)
    finally:
        h.close()


@pytest.mark.gpu
def test_rejected_option_restores_every_option():
    import torch
    from diffusesg_amd.model import build_network
    cfg = S.ModelConfig(max_node_num=20, c_adj=3, c_node=5, depths=(1, 1), num_heads=(3, 6), window_size=10, self_condition=True)
    net = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda").model
    flags, adj, node, sc_adj, sc_node = Y.case_inputs(cfg, 2, [20, 13], 5, "options/rejected")
    args = (T(adj), T(node), T(flags), T(np.array([0.3, -0.7], np.float32)), T(sc_adj), T(sc_node))
    forward = lambda: [t.clone() for t in net(*args)]
    forward()   # the workspace of B = 2 exists from here on: dsg_set_option validates the workspaces in use
    h = net._ensure_handle()
    for name, v in (("dedup_levels", 1), ("dedup_batch", 2), ("dedup_qkv", 2), ("fused_merge", 2), ("bf16_act", 1)):
        h.set_option(name, v)
    # ("fused_merge" 2 is another kernel at this size, equal within the parity bar and not bit for bit: the output to hold is this one's)
    kept = forward()
    recorded = {n: h.get_option(n) for n in NAMES}
    assert len(recorded) == 25 and recorded["fused_merge"] == 2
    with pytest.raises(lib.DsgError, match="rejected.*batch_invariant"):
        h.set_option("batch_invariant", 1)
    assert {n: h.get_option(n) for n in NAMES} == recorded
    assert all(torch.equal(a, b) for a, b in zip(forward(), kept))

    h.set_option("gemm_bf16", 1)
    h.set_option("bf16_qkv_attn", 2)
    assert h.get_option("bf16_qkv_attn") == 2
    recorded_bf16 = {n: h.get_option(n) for n in NAMES}
    with pytest.raises(lib.DsgError, match="rejected.*batch_invariant"):
        h.set_option("batch_invariant", 1)
    assert h.get_option("bf16_qkv_attn") == 2
    assert {n: h.get_option(n) for n in NAMES} == recorded_bf16
    h.set_option("gemm_bf16", 0)
    assert all(torch.equal(a, b) for a, b in zip(forward(), kept))


ENV = {"DSG_FUSED_ATTN": "0", "DSG_FUSED_MERGE": "1", "DSG_FUSED_MLP_MAXC": "192", "DSG_LOOP_GRAPH": "0", "DSG_GEMM_BF16": "1", "DSG_BF16_MLP": "9",
       "DSG_BF16_QA": "-3", "DSG_DEDUP_QKV": "2", "DSG_DEDUP_BATCH": "7", "DSG_DEDUP_LEVELS": "-2", "DSG_DEDUP_TABLE": "0"}
ENV_NAMES = ["fused_attn", "fused_merge", "fused_mlp_maxc", "loop_graph", "gemm_bf16", "bf16_mlp", "bf16_qkv_attn", "dedup_qkv", "dedup_batch",
             "dedup_levels", "dedup_table"]
DEDUP_NAMES = ENV_NAMES[-4:]
CHILD = """
import json, sys
from diffusesg_amd import lib, spec as S, weights as W
from diffusesg_amd.model import build_network
names, dedup = json.loads(sys.argv[1]), json.loads(sys.argv[2])
out = {}
h = lib.Handle(S.tiny_config())
out["tiny"] = {n: h.get_option(n) for n in names}
h.set_option("gemm_bf16", 0)
out["tiny_f32"] = {n: h.get_option(n) for n in dedup}
h.close()
cfg = S.ModelConfig(max_node_num=32, c_adj=3, c_node=5, depths=(1, 1, 1), num_heads=(3, 6, 12), window_size=8, self_condition=True)
net = build_network(cfg, W.synth_state_dict(cfg, 0), device="cuda").model
h = net._ensure_handle()
out["s_bf16"] = {n: h.get_option(n) for n in dedup}
h.set_option("gemm_bf16", 0)
h.set_option("fused_attn", 1)
out["s_f32"] = {n: h.get_option(n) for n in dedup + ["dedup_masked"]}
h.set_option("dedup_table", 1)
out["s_table_on"] = h.get_option("dedup_table")
print("RESULT " + json.dumps(out))
"""


@pytest.mark.gpu
def test_environment_defaults():
    env = dict(os.environ, **ENV)
    r = subprocess.run([sys.executable, "-c", CHILD, json.dumps(ENV_NAMES), json.dumps(DEDUP_NAMES)], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads([ln for ln in r.stdout.split("\n") if ln.startswith("RESULT ")][-1][7:])
    off = {n: 0 for n in DEDUP_NAMES}
    # the bf16 mode is on: the deduplication does not run, its four options report 0
    assert out["tiny"] == dict(fused_attn=0, fused_merge=1, fused_mlp_maxc=192, loop_graph=0, gemm_bf16=1, bf16_mlp=6, bf16_qkv_attn=0, **off)
    assert out["tiny_f32"] == off   # 4 x 4 windows, and the fused attention is off: still not running
    assert out["s_bf16"] == off
    # N = 32, 8 x 8 windows, fp32, fused C = 96 kernels: it runs, on levels 0 and 1 ("dedup_levels" -2 -> 0 = every qualifying level: the two
    # whose first block is unshifted on at least 2 x 2 windows); "dedup_qkv" is a flag in the environment; "dedup_batch" 7 -> 2
    assert out["s_f32"] == dict(dedup_masked=1, dedup_qkv=1, dedup_batch=2, dedup_levels=2, dedup_table=0)
    assert out["s_table_on"] == 1   # ... and the 0 was the environment's, not "does not act"
