"""CPU: the description layer at patch_size > 1 (diffusesg_amd/spec.py, synth.py, config.py) against the reference's recorded
state-dict layout, the formulas of tests/patch_ref.py against the reference's recorded intermediates (tests/golden/fwd_patch_*.npz,
tools/gen_patch_golden.py), and the power of those checks: each listed mistake moves an output beyond its bar."""
import hashlib

import numpy as np
import pytest
import torch

import patch_ref as P
from diffusesg_amd import config as dcfg
from diffusesg_amd import spec as S
from diffusesg_amd import synth as Y
from diffusesg_amd import weights as W
from f32_ref import formula_bar
from util import FWD_RTOL, load, rel_err

NAMES = list(Y.PATCH_CONFIGS)
FULL = [n for n in NAMES if n not in Y.PATCH_ROW_SAMPLED]


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_spec_matches_reference_layout(name):
    cfg, g = Y.PATCH_CONFIGS[name](), load(f"fwd_patch_{name}.npz")
    ref = {str(k): tuple(int(v) for v in s[:np.count_nonzero(s)]) for k, s in zip(g["sd_keys"], g["sd_shapes"])}
    mine = {t.key: tuple(t.shape) for t in S.state_dict_spec(cfg)}
    assert mine == ref
    p, e = cfg.patch_size, cfg.embed_dim
    assert mine["patch_embed.proj.weight"] == (e, cfg.in_chans, p, p) and mine["read_out.0.weight"] == (e, e, p, p)
    fan = {t.key: t.fan_in for t in S.state_dict_spec(cfg)}
    assert fan["patch_embed.proj.weight"] == cfg.in_chans * p * p
    assert list(g["valid"]) == Y.PATCH_VALID[name]


def test_geometry_flops_and_yaml():
    vg = Y.PATCH_CONFIGS["vg_p2"]()
    assert vg.token_res == 32 and [vg.level_res(l) for l in range(4)] == [32, 16, 8, 4]
    assert [vg.level_window(l) for l in range(4)] == [8, 8, 8, 4] and vg.block_shift(2, 1) == 0   # res 8 == window: no shift left
    s2 = Y.PATCH_CONFIGS["small_p2"]()
    assert s2.level_res(0) == 8 and s2.block_shift(0, 1) == 2
    s4 = Y.PATCH_CONFIGS["small_p4"]()
    assert s4.token_res == 4 and s4.level_window(0) == 2 and s4.block_shift(0, 1) == 1 and s4.level_window(1) == 2
    # FLOPs, term by term for vg_p2: PatchEmbed 2 R^2 Cin p^2 E, read_out.0 2 R^2 E E p^2, the two 1 x 1 convs and the heads at N^2
    e, n, r, p = 96, 64, 32, 2
    emb = 2 * (e * 512 + 512 * 512) + 2 * 512 * 2 * e
    edge = 2 * r * r * vg.in_chans * p * p * e + 2 * r * r * e * e * p * p + 2 * 2 * n * n * e * e + 2 * n * n * (e * e + e * 6) + 2 * n * (e * e + e * 12)
    p1 = S.vg_config()
    blocks_p1 = S.flops_per_forward(p1) - emb - (2 * n * n * p1.in_chans * e + 3 * 2 * n * n * e * e + 2 * n * n * (e * e + e * 6) + 2 * n * (e * e + e * 12))
    got_blocks = S.flops_per_forward(vg) - emb - edge
    assert got_blocks > 0 and got_blocks < blocks_p1 / 3          # the blocks run on a quarter of the rows (window 4 at the coarsest level)
    assert 3.0 < S.flops_per_forward(p1) / S.flops_per_forward(vg) < 4.0
    y = dcfg.load_yaml("""
dataset: {name: visual_genome, max_node_num: 64}
mcmc: {name: edm, num_steps: 256}
model: {name: diffuse_sg, feature_dims: [96], depths: [1, 1, 3, 1], window_size: 8, patch_size: 2}
train: {node_encoding: bits, edge_encoding: bits, self_cond: true, node_only: false}
""")
    assert dcfg.model_config_from_yaml(y) == vg
    with pytest.raises(NotImplementedError):
        S.ModelConfig(max_node_num=12, c_adj=1, c_node=1, depths=(1,), num_heads=(3,), patch_size=3)
    with pytest.raises(ValueError):
        S.ModelConfig(max_node_num=10, c_adj=1, c_node=1, depths=(1,), num_heads=(3,), patch_size=4)
    shapes = Y.tap_shapes(vg)
    assert shapes["patch_embed"] == (r * r, e) and shapes["read_out"] == (n * n, e) and shapes["down0.block0"] == (r * r, e)
    assert shapes["down3"] == (16, 768) and shapes["up3.block0"] == (r * r, e)


# the patch_size = 1 values of the description layer before patch sizes 2 and 4 existed (measured on that code): name -> flops, params,
# level_res, level_window, block_shift, sha256[:16] of the (key, shape, kind, fan_in) list, sha256[:16] of the sorted tap shapes
P1_PINNED = {
    "tiny": (73754624, 2402756, [8, 4], [4, 4], [[0], [0]], "b9d1ba4a18e3f6de", "f6c009c7b4b903b4"),
    "small": (403635200, 2819488, [16, 8], [4, 4], [[0, 2], [0]], "af6f70e6de6bc85a", "0057e54d70afb915"),
    "nosc": (72975872, 2395732, [8, 4], [4, 4], [[0], [0]], "c677a0f74288cebb", "f6c009c7b4b903b4"),
    "vg": (13300318208, 35813660, [64, 32, 16, 8], [8, 8, 8, 8], [[0], [0], [0, 4, 0], [0]], "18dfb9455db9cb98", "2dffe01be45ee071"),
    "coco": (7361583104, 30693965, [40, 20, 10], [10, 10, 10], [[0], [0, 5], [0, 0, 0, 0, 0, 0]], "af2c37b4fd81c22b", "d858a0ef8a2269e4"),
    "onehot": (82611200, 2484063, [8, 4], [4, 4], [[0], [0]], "ebe8579227f2388e", "f6c009c7b4b903b4"),
}


@pytest.mark.parametrize("name", list(Y.CONFIGS))
def test_patch_size_1_description_is_unchanged(name):
    c = Y.CONFIGS[name]()
    sp = S.state_dict_spec(c)
    sha = lambda o: hashlib.sha256(repr(o).encode()).hexdigest()[:16]
    L = range(c.num_layers)
    got = (S.flops_per_forward(c), S.num_parameters(c), [c.level_res(l) for l in L], [c.level_window(l) for l in L],
           [[c.block_shift(l, j) for j in range(c.depths[l])] for l in L],
           sha([(t.key, tuple(t.shape), t.kind, t.fan_in) for t in sp]), sha(sorted(Y.tap_shapes(c).items())))
    assert got == P1_PINNED[name]
    assert c.patch_size == 1 and c.token_res == c.max_node_num


# ------------------------------------------------------------------------------------------------------------------------------
# the formulas against the reference's own modules
# ------------------------------------------------------------------------------------------------------------------------------
def _case(name):
    cfg, flags, adj, node, sc_adj, sc_node = Y.patch_fwd_case(name)
    return cfg, flags, adj, node, sc_adj, sc_node, W.synth_state_dict(cfg, 0), load(f"fwd_patch_{name}.npz")


def _squeeze(cfg, a, n):
    return (a[:, 0] if cfg.c_adj == 1 else a), (n[..., 0] if cfg.c_node == 1 else n)


@pytest.mark.parametrize("name", NAMES)
def test_formulas_reproduce_reference_intermediates(name):
    cfg, flags, adj, node, sc_adj, sc_node, sd, g = _case(name)
    B, n, R, p = 2, cfg.max_node_num, cfg.token_res, cfg.patch_size
    with_sc = cfg.self_condition
    pe = P.net_patch_embed(sd, cfg, flags, adj, node, sc_adj if with_sc else None, sc_node if with_sc else None, g["c_noise"]).numpy()
    if name in FULL:
        assert rel_err(pe, g["inter/patch_embed"].reshape(B * R * R, -1)) <= FWD_RTOL
        s, oa, on = P.net_readout(sd, cfg, flags, g["inter/norm"])
        assert rel_err(s.numpy(), g["inter/read_out"].reshape(B * n * n, -1)) <= FWD_RTOL
        oa, on = _squeeze(cfg, oa.numpy(), on.numpy())
        key = "sc" if with_sc else "nosc"
        assert rel_err(oa, g[f"{key}_adj_out"]) <= FWD_RTOL and rel_err(on, g[f"{key}_node_out"]) <= FWD_RTOL
        # exact zeros at masked entries, in the reference as in the formulas
        v = (flags[:, :, None] & flags[:, None, :]).astype(bool)
        ga = g[f"{key}_adj_out"].reshape(B, -1, n, n)
        assert np.all(ga.transpose(0, 2, 3, 1)[~v] == 0) and np.all(oa.reshape(B, -1, n, n).transpose(0, 2, 3, 1)[~v] == 0)
    else:
        assert rel_err(pe[Y.inter_rows(B * R * R)], g["rows/patch_embed"]) <= FWD_RTOL
        # the sampled pixel rows of the read-out from the norm rows of their owner tokens: each pixel's own (a, b) slice of read_out.0
        q = P.sd_params(sd)
        px = Y.inter_rows(B * n * n)
        i, j = (px // n) % n, px % n
        xn = torch.from_numpy(g["rows/norm"]).double()
        w0 = q["W0"][:, :, torch.as_tensor(i % p), torch.as_tensor(j % p)]                 # [in, out, rows]
        s = torch.einsum("ri,ior->ro", xn, w0) + q["b0"]
        s = (s @ q["W1"].t() + q["b1"]) @ q["W2"].t() + q["b2"]
        assert rel_err(s.numpy(), g["rows/read_out"]) <= FWD_RTOL


@pytest.mark.parametrize("name", FULL)
def test_pooled_fold_identity(name):
    """pooling LN(x) per (node row, column parity) and pushing it through F[a, b] equals pooling the shared representation"""
    cfg, flags, *_, sd, g = _case(name)
    B, n, p = 2, cfg.max_node_num, cfg.patch_size
    q = P.sd_params(sd)
    xn = torch.from_numpy(g["inter/norm"]).double().reshape(B * cfg.token_res ** 2, -1)
    direct = P.node_pool(P.shared_rep(xn, q, B, n, p), flags, p)
    fold = P.pooled_fold(xn, q, flags, p)
    scale = float(direct.abs().max())
    assert float((fold - direct).abs().max()) <= 1e-12 * scale
    bad = P.pooled_fold(xn, q, flags, p, mut="cnt_total")
    bar, _ = formula_bar(direct, P.node_pool(P.shared_rep(xn.float(), P.sd_params(sd, torch.float32), B, n, p), flags, p))
    assert float((bad - direct).abs().max()) > bar


@pytest.mark.parametrize("name", ["tiny_p2", "small_p2", "small_p4"])
@pytest.mark.parametrize("mut", [m for m in P.MUTATIONS if m != "cnt_total"])
def test_mistakes_move_an_output_beyond_its_bar(name, mut):
    """power: the bar of every compared quantity (float64 formula vs its float32 evaluation, x 8, at most FWD_RTOL of the scale) is
    exceeded by each mistake in at least one of PatchEmbed's output, the adjacency output and the node output"""
    cfg, flags, adj, node, sc_adj, sc_node, sd, g = _case(name)
    args = (sd, cfg, flags, adj, node, sc_adj, sc_node, g["c_noise"])
    moved = []
    pe64, pe32 = P.net_patch_embed(*args), P.net_patch_embed(*args, dtype=torch.float32)
    moved.append(float((P.net_patch_embed(*args, mut=mut) - pe64).abs().max()) > formula_bar(pe64, pe32)[0])
    r64, r32 = P.net_readout(sd, cfg, flags, g["inter/norm"]), P.net_readout(sd, cfg, flags, g["inter/norm"], dtype=torch.float32)
    rm = P.net_readout(sd, cfg, flags, g["inter/norm"], mut=mut)
    for k in (1, 2):
        moved.append(float((rm[k] - r64[k]).abs().max()) > formula_bar(r64[k], r32[k])[0])
    expect = {"pe_swap_ab": (True, False, False), "ro_swap_ab": (False, True, True), "ro_out_in": (False, True, True),
              "token_mask": (True, True, True), "mean_over_R": (False, False, True)}[mut]
    assert tuple(moved) == expect, (mut, moved)
