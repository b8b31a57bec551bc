"""GPU: the edge kernels of the training form at patch_size p > 1 (csrc/train_kernels_patch.hip) on their own, through the
dsg_debug_t_* hooks of include/dsg_debug.h.  EVERY output element is compared with the float64 restatement of tests/patch_train_ref.py
on the same fp32 operands.

Shapes, the smallest at which the tiling can go wrong: p in {2, 4}; N in {8, 12, 72} (72 crosses the 64-column tile of the assembly
backward, 12 gives R = 3 at p = 4); C_adj in {3, 33} (33 crosses the 32-channel tile); C_node = 5; E in {32, 96}; B = 2.  Flags: all
valid, an odd valid count (one token has a single valid pixel row), one graph with a single valid node.

The packs, the unpacks and the adjacency store pair move values: bit for bit.  The sums (pooling backward, assembly backward) are
held to f32_ref.formula_bar: 8 x the error of the float32 evaluation of the same formula, never above 1e-4 of the output scale.
Every input position that must not be read holds NaN: node values of padded nodes, the pad columns of d_tok, the pad columns of the
weight image on unpack.  Outputs carry NaN guard elements behind them.  Measured figures: profiles/patch_train_kernel_errors.md."""
import ctypes as C

import numpy as np
import pytest
import torch

import f32_ref as FR
import patch_train_ref as PT

pytestmark = pytest.mark.gpu

PS, NS, CAS, CN, ES, B = (2, 4), (8, 12, 72), (3, 33), 5, (32, 96), 2
KINDS = ("all", "odd", "one")
GUARD = 64


def _lib():
    from diffusesg_amd import lib as L
    return L.load()


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _out(n):
    return torch.full((n + GUARD,), float("nan"), device="cuda")


def _take(t, shape):
    n = int(np.prod(shape))
    a = t.cpu().numpy()
    assert np.isnan(a[n:]).all(), "written behind the output"
    return a[:n].reshape(shape)


def _rng(*key):
    return np.random.default_rng(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("Ca", CAS)
def test_patch_embed_weight_pack_and_unpack_bit_for_bit(p, E, Ca):
    Cin = 2 * (Ca + 2 * CN)
    Kp = (p * p * Cin + 31) // 32 * 32
    r = _rng(1, p, E, Ca)
    W = r.standard_normal((E, Cin, p, p)).astype(np.float32)
    img = _out(E * Kp)
    assert _lib().dsg_debug_t_patch_pack(0, 0, E, Cin, p, Kp, _p(_dev(W)), _p(img), None, None, None) == 0
    assert np.array_equal(_take(img, (E, Kp)), PT.pe_pack(W, Kp))
    G = r.standard_normal((E, Kp)).astype(np.float32)
    G[:, p * p * Cin:] = np.nan          # the pad columns of a gradient image are never read
    dW = _out(W.size)
    assert _lib().dsg_debug_t_patch_pack(0, 1, E, Cin, p, Kp, _p(dW), _p(_dev(G)), None, None, None) == 0
    assert np.array_equal(_take(dW, W.shape), PT.pe_unpack(G, Cin, p))


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("E", ES)
def test_read_out_weight_pack_and_unpack_bit_for_bit(p, E):
    r = _rng(2, p, E)
    W, b = r.standard_normal((E, E, p, p)).astype(np.float32), r.standard_normal(E).astype(np.float32)
    img, brep = _out(W.size), _out(p * p * E)
    assert _lib().dsg_debug_t_patch_pack(1, 0, E, E, p, 0, _p(_dev(W)), _p(img), _p(_dev(b)), _p(brep), None) == 0
    want_img, want_b = PT.ro0_pack(W, b)
    assert np.array_equal(_take(img, want_img.shape), want_img) and np.array_equal(_take(brep, want_b.shape), want_b)
    G = r.standard_normal((E, p * p * E)).astype(np.float32)
    dW = _out(W.size)
    assert _lib().dsg_debug_t_patch_pack(1, 1, E, E, p, 0, _p(dW), _p(_dev(G)), None, None, None) == 0
    assert np.array_equal(_take(dW, W.shape), PT.ro0_unpack(G, E, p))


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("Ca", CAS)
@pytest.mark.parametrize("sc", (0, 1))
def test_live_columns_bit_for_bit(p, Ca, sc):
    E, Cin = 32, (2 if sc else 1) * (Ca + 2 * CN)
    W = _rng(3, p, Ca, sc).standard_normal((E, Cin, p, p)).astype(np.float32)
    ld = C.c_int32(0)
    assert _lib().dsg_debug_t_live_cols_patch(E, Ca, CN, sc, p, None, None, C.byref(ld), None) == 0 and ld.value == PT.live_width(Ca, CN, p)
    img = _out(E * ld.value)
    assert _lib().dsg_debug_t_live_cols_patch(E, Ca, CN, sc, p, _p(_dev(W)), _p(img), None, None) == 0
    assert np.array_equal(_take(img, (E, ld.value)), PT.live_cols(W, Ca, CN, bool(sc)))


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("Ca", CAS)
@pytest.mark.parametrize("kind", KINDS)
def test_adjacency_store_pair_bit_for_bit(p, N, Ca, kind):
    r = _rng(4, p, N, Ca, KINDS.index(kind))
    flags = PT.make_flags(B, N, kind)
    M = B * N * N
    oa, dF = r.standard_normal((M, Ca)).astype(np.float32), r.standard_normal((B, Ca, N, N)).astype(np.float32)
    fl = _dev(flags)
    F, d_oa = _out(dF.size), _out(oa.size)
    assert _lib().dsg_debug_t_adj_out_patch(0, B, N, p, Ca, _p(_dev(oa)), _p(fl), _p(F), None, None, None) == 0
    assert _lib().dsg_debug_t_adj_out_patch(1, B, N, p, Ca, None, _p(fl), None, _p(_dev(dF)), _p(d_oa), None) == 0
    gF, gd = _take(F, dF.shape), _take(d_oa, oa.shape)
    assert np.array_equal(gF, PT.adj_store(oa, flags, p)) and np.array_equal(gd, PT.adj_store_bwd(dF, flags, p))
    masked = ~np.broadcast_to(PT.pixel_valid(flags, p)[:, None], dF.shape)
    assert (gF[masked] == 0).all() and not np.signbit(gF[masked]).any(), "masked entries are not exact (positive) zeros"
    g, I, J = PT.row_pixels(B, N, p)
    assert (gd[~PT.pixel_valid(flags, p)[g, I, J]] == 0).all()


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("kind", KINDS)
def test_pooling_backward_every_element(p, N, E, kind):
    r = _rng(5, p, N, E, KINDS.index(kind))
    flags = PT.make_flags(B, N, kind)
    d_pool = r.standard_normal((B, N, E)).astype(np.float32)
    d_rep = r.standard_normal((B * N * N, E)).astype(np.float32)
    acc = _out(d_rep.size)
    acc[:d_rep.size] = _dev(d_rep).reshape(-1)
    assert _lib().dsg_debug_t_pool_bwd_patch(B, N, p, E, _p(_dev(d_pool)), _p(_dev(flags)), _p(acc), None) == 0
    got = _take(acc, d_rep.shape)
    f64 = d_rep.astype(np.float64) + PT.pool_bwd(d_pool.astype(np.float64), flags, p)
    f32 = d_rep + PT.pool_bwd(d_pool, flags, p)
    bar, ref_err = FR.formula_bar(torch.from_numpy(f64), torch.from_numpy(f32))
    err = float(np.abs(got - f64).max())
    print(f"PATCHTRAIN pool_bwd p{p} N{N} E{E} {kind}: |err| {err:.3e} bar {bar:.3e} ratio {err / max(bar, 1e-300):.3f}")
    assert err <= bar
    g, I, J = PT.row_pixels(B, N, p)
    untouched = ~PT.pixel_valid(flags, p)[g, I, J]
    assert np.array_equal(got[untouched], d_rep[untouched]), "a masked pixel's row was changed"


def _asm_case(p, N, Ca, kind, seed=0):
    r = _rng(6, p, N, Ca, KINDS.index(kind), seed)
    flags = PT.make_flags(B, N, kind)
    G, ld = Ca + 2 * CN, PT.live_width(Ca, CN, p) + (32 if seed else 0)
    d_tok = r.standard_normal((B * (N // p) ** 2, ld)).astype(np.float32)
    d_tok[:, p * p * G:] = np.nan
    g_adj = r.standard_normal((B, Ca, N, N)).astype(np.float32)
    g_node = r.standard_normal((B, N, CN)).astype(np.float32)
    g_node[~flags.astype(bool)] = np.nan          # node values of padded nodes are never read
    c_skip, c_in = r.uniform(0.0, 1.0, B).astype(np.float32), r.uniform(0.01, 2.0, B).astype(np.float32)
    return dict(p=p, N=N, Ca=Ca, ld=ld, flags=flags, d_tok=d_tok, g_adj=g_adj, g_node=g_node, c_skip=c_skip, c_in=c_in)


def _asm_call(o, in_place=False):
    dev = {k: _dev(o[k]) for k in ("d_tok", "flags", "c_skip", "c_in", "g_adj", "g_node")}
    oa, on = (dev["g_adj"], dev["g_node"]) if in_place else (_out(o["g_adj"].size), _out(o["g_node"].size))
    rc = _lib().dsg_debug_t_assemble_bwd_patch(B, o["N"], o["p"], o["Ca"], CN, _p(dev["d_tok"]), o["ld"], _p(dev["flags"]), _p(dev["c_skip"]),
                                               _p(dev["c_in"]), _p(dev["g_adj"]), _p(dev["g_node"]), _p(oa), _p(on), None)
    assert rc == 0, f"dsg_debug_t_assemble_bwd_patch: status {rc}"
    if in_place:
        return oa.cpu().numpy(), on.cpu().numpy()
    return _take(oa, o["g_adj"].shape), _take(on, o["g_node"].shape)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("Ca", CAS)
@pytest.mark.parametrize("kind", KINDS)
def test_assembly_backward_every_element(p, N, Ca, kind):
    o = _asm_case(p, N, Ca, kind)
    ga, gn = _asm_call(o)
    with np.errstate(invalid="ignore"):
        r64 = PT.assemble_bwd(o["d_tok"].astype(np.float64), o["flags"], o["c_skip"].astype(np.float64), o["c_in"].astype(np.float64),
                              o["g_adj"].astype(np.float64), o["g_node"].astype(np.float64), p)
        r32 = PT.assemble_bwd(o["d_tok"], o["flags"], o["c_skip"], o["c_in"], o["g_adj"], o["g_node"], p)
    for name, got, f64, f32 in (("adj", ga, r64[0], r32[0]), ("node", gn, r64[1], r32[1])):
        assert np.isfinite(f64).all()
        bar, ref_err = FR.formula_bar(torch.from_numpy(f64), torch.from_numpy(f32.astype(np.float32)))
        err = float(np.abs(got - f64).max())
        print(f"PATCHTRAIN assemble_bwd {name} p{p} N{N} Ca{Ca} {kind}: |err| {err:.3e} bar {bar:.3e} ratio {err / max(bar, 1e-300):.3f}")
        assert np.isfinite(got).all() and err <= bar, (name, err, bar)
    assert (gn[~o["flags"].astype(bool)] == 0).all(), "node gradient of a padded node is not exactly 0"


def test_assembly_backward_repeatable_in_place_and_refusals():
    o = _asm_case(4, 72, 33, "odd", seed=5)          # (a pitch above the live width too)
    a1, n1 = _asm_call(o)
    a2, n2 = _asm_call(o)
    assert np.array_equal(a1, a2) and np.array_equal(n1, n2), "two calls differ"
    a3, n3 = _asm_call(o, in_place=True)              # dsg_precond_vjp's own use: the result overwrites g
    assert np.array_equal(a3, a1) and np.array_equal(n3, n1), "in place differs from out of place"
    d = {k: _dev(o[k]) for k in ("d_tok", "flags", "c_skip", "c_in", "g_adj", "g_node")}
    oa, on = _out(o["g_adj"].size), _out(o["g_node"].size)
    args = lambda N, p, ld: (B, N, p, 33, CN, _p(d["d_tok"]), ld, _p(d["flags"]), _p(d["c_skip"]), _p(d["c_in"]), _p(d["g_adj"]), _p(d["g_node"]),
                             _p(oa), _p(on), None)
    for bad in (args(72, 3, o["ld"]), args(70, 4, o["ld"]), args(72, 4, 16 * 43 - 1)):   # patch size, N % p, a pitch below p^2 G
        assert _lib().dsg_debug_t_assemble_bwd_patch(*bad) == -1
    assert np.isnan(oa.cpu().numpy()).all() and np.isnan(on.cpu().numpy()).all(), "a refused call wrote"
