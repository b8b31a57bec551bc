"""CPU: the edges of the training form at patch_size p > 1 as tests/patch_train_ref.py restates them in float64.

* Every backward is the transpose of its forward: <A x, y> = <x, A^T y> to float64 rounding, for the weight pack / unpack pairs, the
  masked adjacency store pair, the node pooling and the assembly, at p = 2 and 4 with ragged flags.
* The composed edges reproduce the reference's own autograd (tests/golden/train_patch.npz, tools/gen_patch_train_golden.py): the
  gradients of patch_embed.proj.weight / .bias and read_out.0.weight / .bias from the recorded activations around the two
  convolutions, and the input gradients from the recorded gradient at PatchEmbed's output.  The reference computed these last steps
  in float32 from the very tensors the fixture records, so the bar is the closed-form bound of a float32 sum of K products in any
  order, (K + 8) 2^-24 sum |terms|, element by element.
* The power of those bars: (a, b) swapped in either unpack, read_out.0 taken as [out, in], a pixel masked by its token's first pixel,
  the pooling mean over R, the row sum without the column sum each move a result beyond its bar."""
import numpy as np
import pytest

import patch_train_ref as PT
from diffusesg_amd import spec as S
from diffusesg_amd import synth as Y
from diffusesg_amd import weights as W
from util import load

U = 2.0 ** -24
CASE = Y.PATCH_TRAIN_ADAM_CASE
IG = Y.PATCH_INPUT_GRAD_EDGE_CASE


def _dot(a, b):
    return float((a.astype(np.float64) * b.astype(np.float64)).sum())


def _close(lhs, rhs, scale):
    return abs(lhs - rhs) <= 1e-12 * scale


def _rng():
    return np.random.default_rng(11)


@pytest.mark.parametrize("p", [2, 4])
def test_weight_pack_pairs_are_transposes(p):
    r = _rng()
    E, Cin, Kp = 5, 7, (p * p * 7 + 31) // 32 * 32
    Wp, Yi = r.standard_normal((E, Cin, p, p)), r.standard_normal((E, Kp))
    assert _close(_dot(PT.pe_pack(Wp, Kp), Yi), _dot(Wp, PT.pe_unpack(Yi, Cin, p)), np.abs(Wp).sum() * np.abs(Yi).max())
    assert np.array_equal(PT.pe_unpack(PT.pe_pack(Wp, Kp), Cin, p), Wp) and (PT.pe_pack(Wp, Kp)[:, p * p * Cin:] == 0).all()
    Ei, Eo = 6, 3
    W0, b0, Y0 = r.standard_normal((Ei, Eo, p, p)), r.standard_normal(Eo), r.standard_normal((Ei, p * p * Eo))
    img, brep = PT.ro0_pack(W0, b0)
    assert _close(_dot(img, Y0), _dot(W0, PT.ro0_unpack(Y0, Eo, p)), np.abs(W0).sum() * np.abs(Y0).max())
    assert np.array_equal(PT.ro0_unpack(img, Eo, p), W0) and np.array_equal(brep.reshape(p * p, Eo), np.tile(b0, (p * p, 1)))
    # the transposed convolution itself: row (token, a, b) of fy img is sum_i fy[t, i] W0[i, :, a, b]
    B, N = 2, 2 * p
    fy = r.standard_normal((B * (N // p) ** 2, Ei))
    z = (fy @ img + brep).reshape(B * N * N, Eo)
    g, I, J = PT.row_pixels(B, N, p)
    tok = (g * (N // p) + I // p) * (N // p) + J // p
    want = np.einsum("mi,iom->mo", fy[tok], W0[:, :, I % p, J % p]) + b0
    assert np.abs(z - want).max() <= 1e-12


@pytest.mark.parametrize("p,N", [(2, 8), (4, 12), (4, 8)])
@pytest.mark.parametrize("kind", ["all", "odd", "one"])
def test_store_pool_and_assembly_pairs_are_transposes(p, N, kind):
    r = _rng()
    B, Ca, Cn, E = 2, 3, 5, 4
    flags = PT.make_flags(B, N, kind)
    M = B * N * N
    oa, dF = r.standard_normal((M, Ca)), r.standard_normal((B, Ca, N, N))
    F = PT.adj_store(oa, flags, p)
    assert _close(_dot(F, dF), _dot(oa, PT.adj_store_bwd(dF, flags, p)), np.abs(oa).sum() * np.abs(dF).max())
    assert (F[~np.broadcast_to(PT.pixel_valid(flags, p)[:, None], F.shape)] == 0).all()
    rep, d_pool = r.standard_normal((M, E)), r.standard_normal((B, N, E))
    assert _close(_dot(PT.pool(rep, flags, p), d_pool), _dot(rep, PT.pool_bwd(d_pool, flags, p)), np.abs(rep).sum() * np.abs(d_pool).max())
    adj, node = r.standard_normal((B, Ca, N, N)), r.standard_normal((B, N, Cn))
    ld = PT.live_width(Ca, Cn, p)
    Yt = r.standard_normal((B * (N // p) ** 2, ld))
    zero, one = np.zeros(B), np.ones(B)
    ga, gn, _, _ = PT.assemble_bwd(Yt, flags, zero, one, np.zeros_like(adj), np.zeros_like(node), p)
    lhs = _dot(PT.assemble_live(adj, node, flags, p, ld), Yt)
    assert _close(lhs, _dot(adj, ga) + _dot(node, gn), (np.abs(adj).sum() + np.abs(node).sum()) * np.abs(Yt).max())
    assert (gn[~flags.astype(bool)] == 0).all()
    # the pooling mean over R breaks the pair: the forward (launch_pool_patch's formula) divides by N
    bad = _dot(rep, PT.pool_bwd(d_pool, flags, p, mut="mean_over_R"))
    assert not _close(_dot(PT.pool(rep, flags, p), d_pool), bad, np.abs(rep).sum() * np.abs(d_pool).max())


def _edge_grads(g, mut=None):
    """gradients of the four edge parameters from the recorded activations, float64, with their closed-form bars"""
    cfg = Y.patch_train_case(CASE)[0]
    p, E, Cin = cfg.patch_size, cfg.embed_dim, cfg.in_chans
    Kp = (p * p * Cin + 31) // 32 * 32
    tok = PT.image_to_tok(g[f"{CASE}_pe_in"].astype(np.float64), p, Kp)
    d_lin = PT.tokens_rows(g[f"{CASE}_pe_dout"].astype(np.float64))
    K = tok.shape[0]
    out = {"patch_embed.proj.weight": (PT.pe_unpack(d_lin.T @ tok, Cin, p, mut), (K + 8) * U * PT.pe_unpack(np.abs(d_lin).T @ np.abs(tok), Cin, p, mut)),
           "patch_embed.proj.bias": (d_lin.sum(0), (K + 8) * U * np.abs(d_lin).sum(0))}
    fy = PT.tokens_rows(g[f"{CASE}_ro0_in"].astype(np.float64))
    d_z1 = PT.pixels_rows(g[f"{CASE}_ro0_dout"].astype(np.float64), p)
    d_v = d_z1.reshape(fy.shape[0], p * p * E)
    out["read_out.0.weight"] = (PT.ro0_unpack(fy.T @ d_v, E, p, mut), (K + 8) * U * PT.ro0_unpack(np.abs(fy).T @ np.abs(d_v), E, p, mut))
    out["read_out.0.bias"] = (d_z1.sum(0), (d_z1.shape[0] + 8) * U * np.abs(d_z1).sum(0))
    return out


def test_edge_weight_gradients_reproduce_the_reference_autograd():
    g = load("train_patch.npz")
    for k, (got, bar) in _edge_grads(g).items():
        ref = g[f"{CASE}_gfull/model.{k}"].astype(np.float64)
        ratio = float((np.abs(got - ref) / (bar + 1e-300)).max())
        print(f"PATCH TRAIN host {k}: worst |err| / bar {ratio:.3f}, max |ref| {np.abs(ref).max():.3e}")
        assert got.shape == ref.shape and ratio <= 1.0, (k, ratio)


@pytest.mark.parametrize("mut,key", [("pe_swap_ab", "patch_embed.proj.weight"), ("ro_swap_ab", "read_out.0.weight"), ("ro_out_in", "read_out.0.weight")])
def test_a_wrong_unpack_leaves_the_bar(mut, key):
    g = load("train_patch.npz")
    got, bar = _edge_grads(g, mut)[key]
    ref = g[f"{CASE}_gfull/model.{key}"].astype(np.float64)
    assert float((np.abs(got - ref) / (bar + 1e-300)).max()) > 1.0


def _input_grads(g, mut=None):
    cfg, flags, adj, node, sig, _sa, _sn, g_adj, g_node = Y.patch_input_grad_case(IG)
    p, E, Ca, Cn, N = cfg.patch_size, cfg.embed_dim, cfg.c_adj, cfg.c_node, cfg.max_node_num
    Wpe = np.asarray(W.synth_state_dict(cfg, 0)["patch_embed.proj.weight"], np.float64).reshape(E, cfg.in_chans, p, p)
    img = PT.live_cols(Wpe, Ca, Cn, cfg.self_condition)
    d_lin = PT.tokens_rows(g[f"igrad/{IG}/pe_dout"].astype(np.float64))
    s = sig.astype(np.float64)
    c_skip, c_in = 0.25 / (s * s + 0.25), 1.0 / np.sqrt(s * s + 0.25)
    f = flags.astype(bool)
    ga = np.where((f[:, :, None] & f[:, None, :])[:, None], g_adj.astype(np.float64), 0)
    ga_out, gn_out, _, _ = PT.assemble_bwd(d_lin @ img, flags, c_skip, c_in, ga, g_node.astype(np.float64), p, mut)
    _, _, abs_a, abs_n = PT.assemble_bwd(np.abs(d_lin) @ np.abs(img), flags, c_skip, c_in, np.abs(ga), np.abs(g_node.astype(np.float64)), p)
    K = E + 2 * N + 8
    return (ga_out, K * U * abs_a), (gn_out, K * U * abs_n)


def test_input_gradients_reproduce_the_reference_autograd():
    g = load("train_patch.npz")
    (ga, bar_a), (gn, bar_n) = _input_grads(g)
    ref_a, ref_n = g[f"igrad/{IG}/grad_adj"].astype(np.float64), g[f"igrad/{IG}/grad_node"].astype(np.float64)
    ra, rn = float((np.abs(ga - ref_a) / (bar_a + 1e-300)).max()), float((np.abs(gn - ref_n) / (bar_n + 1e-300)).max())
    print(f"PATCH TRAIN host input gradients: worst |err| / bar adj {ra:.3f} node {rn:.3f}")
    assert ra <= 1.0 and rn <= 1.0, (ra, rn)


@pytest.mark.parametrize("mut", ["token_mask", "row_only"])
def test_a_wrong_assembly_backward_leaves_the_bar(mut):
    g = load("train_patch.npz")
    _, (gn, bar_n) = _input_grads(g, mut)
    ref_n = g[f"igrad/{IG}/grad_node"].astype(np.float64)
    assert float((np.abs(gn - ref_n) / (bar_n + 1e-300)).max()) > 1.0


def test_case_tables_and_fixture_agree():
    g = load("train_patch.npz")
    for case, (name, valid, coin) in Y.PATCH_TRAIN_CASES.items():
        cfg = Y.PATCH_CONFIGS[name]()
        assert cfg.patch_size in (2, 4) and len(valid) == 4 and float(g[f"{case}_coin"]) == coin
        keys = {str(k)[len("model."):] for k in g[f"{case}_gparam_names"]}
        want = {t.key for t in S.state_dict_spec(cfg)}
        assert keys <= want and {"patch_embed.proj.weight", "read_out.0.weight"} <= keys
    assert set(Y.PATCH_INPUT_GRAD_CASES) == {k.split("/")[1] for k in g.files if k.startswith("igrad/")}
