"""GPU: the kernels of the patch_size > 1 forward on their own (csrc/kernels_patch.hip: assemble_patch_kernel, head_adj_patch_kernel,
pool_patch_kernel, and the fused E = 96, p = 2 forms fused_patch_embed96_p2_kernel, fused_readout96_p2_kernel + pool_finish_p2_kernel)
through the dsg_debug_*_patch_f32 hooks.  EVERY output element is compared with the float64 formulas of
tests/patch_ref.py; the assembly and the (token, a, b) -> (I, J) index maps bit for bit, the two products within f32_ref.formula_bar.

Shapes (N, p, B): (8, 2, 3), (16, 2, 2), (20, 2, 2), (16, 4, 3) -- R^2 = 16 and 100, partially filled last blocks, a graph boundary inside a
block of four rows -- under the flag patterns of edge_ref.make_flags (graphs with no valid node and with a single one from B = 3 on; odd
prefixes put a token with valid and padded pixels in every case).  Conventions of tests/test_edge_kernels.py: outputs are NaN-filled and
carry guard rows; the padded nodes' node / self-condition values and the read-out rows of pixels that are not valid are NaN: a read of
them into a result shows.  Each test prints its worst |err| / bar (lines PATCHK ...); measured figures: profiles/patch_kernel_errors.md."""
import ctypes as C

import numpy as np
import pytest
import torch

import edge_ref as X
import f32_ref as R
import patch_ref as P

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000
GUARD = 2
GRIDS = [(8, 2, 3), (16, 2, 2), (20, 2, 2), (16, 4, 3)]


def _lib():
    from diffusesg_amd import lib as L
    return L, L.load()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _nan(rows, cols):
    return torch.full((rows + GUARD, cols), float("nan"), device="cuda")


def _bits(t):
    return t.contiguous().view(torch.int32).cpu()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _report(family, err, bar, ref_err):
    print(f"PATCHK {family}: max |err| {err:.3e}, bar {bar:.3e} (float32 formula {ref_err:.3e}), |err| / bar = {err / bar if bar > 0 else 0.0:.3f}")


@pytest.mark.parametrize("pattern", X.FLAG_PATTERNS)
@pytest.mark.parametrize("Ca,Cn,self_cond", [(6, 12, 1), (1, 1, 0), (3, 5, 1)])
@pytest.mark.parametrize("N,p,B", GRIDS)
def test_assemble_patch_bit_exact(N, p, B, Ca, Cn, self_cond, pattern):
    """three self-conditioning forms: tensors given and used; tensors given as NaN with the device switch off; no tensors"""
    L, lib = _lib()
    flags = X.make_flags(B, N, pattern, seed=N + p)
    t = X.make_pe_inputs(B, N, Ca, Cn, _gen(11 + N + 7 * p))
    cin = (2 if self_cond else 1) * (Ca + 2 * Cn)
    Kp = P.patch_kp(cin, p)
    R_ = N // p
    pad = ~torch.as_tensor(flags).bool()
    poisoned = {k: v.clone() for k, v in t.items()}
    poisoned["node"][pad] = float("nan")          # a padded node's values never reach a result
    poisoned["sc_node"][pad] = float("nan")
    fl = torch.as_tensor(flags).cuda()
    for mode in ((0, 1, 2) if self_cond else (2,)):
        sc_on = mode == 0
        want = X.pad_k(P.patch_input(t, flags, p, bool(self_cond), sc_on, torch.float32), Kp)
        d = {k: v.cuda() for k, v in poisoned.items()}
        if mode == 1:
            d["sc_adj"].fill_(float("nan")); d["sc_node"].fill_(float("nan"))
        has_sc = torch.tensor([0], dtype=torch.int32, device="cuda") if mode == 1 else None
        out = _nan(B * R_ * R_, Kp)
        rc = lib.dsg_debug_assemble_patch_f32(B, N, p, Ca, Cn, self_cond, Kp, _p(d["adj"]), _p(d["node"]), _p(d["sc_adj"]) if mode < 2 else None,
                                              _p(d["sc_node"]) if mode < 2 else None, _p(has_sc), _p(fl), _p(out), None)
        assert rc == 0
        got = out.cpu()
        assert torch.equal(_bits(got[:B * R_ * R_]), _bits(want)), f"mode {mode}"
        assert (_bits(got[B * R_ * R_:]) == NAN_BITS).all()
    # refusals: a pitch below p^2 Cin, a patch size the library does not know, N no multiple of p
    out = _nan(B * R_ * R_, Kp)
    d = {k: v.cuda() for k, v in t.items()}
    bad = lambda n, pp, kp: lib.dsg_debug_assemble_patch_f32(B, n, pp, Ca, Cn, self_cond, kp, _p(d["adj"]), _p(d["node"]), None, None, None,
                                                             _p(fl), _p(out), None)
    assert bad(N, p, p * p * cin - 1) == L.DSG_ERR_INVALID and bad(N, 3, Kp) == L.DSG_ERR_INVALID and bad(N + 1, p, Kp) == L.DSG_ERR_INVALID
    assert (_bits(out) == NAN_BITS).all()


def test_index_map_is_a_permutation():
    for N, p, B in GRIDS:
        m = P.tab_to_pixel(B, N, p)
        assert np.array_equal(np.sort(m), np.arange(B * N * N))
        R_ = N // p
        k = (1 * R_ * R_ + 2 * R_ + 1) * p * p + 1 * p + 0            # graph 1, token (2, 1), sub-pixel (a, b) = (1, 0)
        assert m[k] == (1 * N + 2 * p + 1) * N + 1 * p + 0


@pytest.mark.parametrize("pattern", X.FLAG_PATTERNS)
@pytest.mark.parametrize("N,p,B", GRIDS)
@pytest.mark.parametrize("E,Ca", [(96, 6), (96, 1), (160, 3)])
def test_head_adj_patch(N, p, B, E, Ca, pattern):
    L, lib = _lib()
    gen = _gen(5 + N + p + E)
    flags = X.make_flags(B, N, pattern, seed=N + p)
    M = B * N * N
    h = torch.randn(M, E, generator=gen)                          # pixel order
    W, bias = torch.randn(Ca, E, generator=gen) / E ** 0.5, torch.randn(Ca, generator=gen) * 0.3
    f64 = X.head_adj_formula(h.double(), W.double(), bias.double(), flags)
    f32 = X.head_adj_formula(h, W, bias, flags)
    valid = X.pair_valid(flags).reshape(M)
    hp = h.clone()
    hp[~valid] = float("nan")                                     # rows of pixels that are not valid are not read into a result
    ht = P.to_tab_order(hp, B, N, p).cuda()
    out = torch.full((B * Ca * N * N + GUARD,), float("nan"), device="cuda")
    dW, db, fl = W.cuda(), bias.cuda(), torch.as_tensor(flags).cuda()
    assert lib.dsg_debug_head_patch_f32(L.HEAD_ADJ, B, N, p, E, Ca, _p(ht), _p(dW), _p(db), _p(fl), _p(out), None) == 0
    got = out.cpu()
    assert (_bits(got[B * Ca * N * N:]) == NAN_BITS).all()
    got = got[:B * Ca * N * N].view(B, Ca, N, N)
    assert torch.isfinite(got).all()
    mask = X.pair_valid(flags)[:, None].expand(B, Ca, N, N)
    assert (_bits(got)[~mask] == 0).all(), "masked entries are exact +0"
    bar, ref_err = R.formula_bar(f64, f32)
    err = float((got.double() - f64).abs().max())
    _report(f"head_adj_patch N={N} p={p} B={B} E={E} Ca={Ca} {pattern}", err, bar, ref_err)
    assert err <= bar


@pytest.mark.parametrize("pattern", X.FLAG_PATTERNS)
@pytest.mark.parametrize("N,p,B", GRIDS)
@pytest.mark.parametrize("E", [96, 160])
def test_pool_patch(N, p, B, E, pattern):
    L, lib = _lib()
    gen = _gen(9 + N + p + E)
    flags = X.make_flags(B, N, pattern, seed=N + p)
    M = B * N * N
    rep = torch.randn(M, E, generator=gen) + 0.5
    f64, f32 = X.pool_formula(rep.double(), flags), X.pool_formula(rep, flags)
    valid = X.pair_valid(flags).reshape(M)
    rp = rep.clone()
    rp[~valid] = float("nan")
    rt = P.to_tab_order(rp, B, N, p).cuda()
    out = _nan(B * N, E)
    fl = torch.as_tensor(flags).cuda()
    assert lib.dsg_debug_head_patch_f32(L.HEAD_POOL, B, N, p, E, 0, _p(rt), None, None, _p(fl), _p(out), None) == 0
    got = out.cpu()
    assert (_bits(got[B * N:]) == NAN_BITS).all()
    got = got[:B * N]
    assert torch.isfinite(got).all()
    rows_off = ~torch.as_tensor(flags).bool().reshape(-1)
    assert (_bits(got)[rows_off] == 0).all(), "rows of padded nodes are exact +0"
    bar, ref_err = R.formula_bar(f64, f32)
    err = float((got.double() - f64).abs().max())
    _report(f"pool_patch N={N} p={p} B={B} E={E} {pattern}", err, bar, ref_err)
    assert err <= bar
    # the mean is over the N pixels of the row, not the R tokens: the other divisor is beyond the bar wherever a node is valid
    if bool(torch.as_tensor(flags).any()):
        assert float((got.double() * p - f64).abs().max()) > bar


def test_head_patch_refusals():
    L, lib = _lib()
    z = torch.zeros(64, device="cuda")
    fl = torch.ones(8, dtype=torch.uint8, device="cuda")
    bad = L.DSG_ERR_INVALID
    assert lib.dsg_debug_head_patch_f32(L.HEAD_NODE, 1, 4, 2, 4, 1, _p(z), _p(z), _p(z), _p(fl), _p(z), None) == bad     # not a kernel of this hook
    assert lib.dsg_debug_head_patch_f32(L.HEAD_ADJ, 1, 4, 3, 4, 1, _p(z), _p(z), _p(z), _p(fl), _p(z), None) == bad      # p = 3
    assert lib.dsg_debug_head_patch_f32(L.HEAD_ADJ, 1, 5, 2, 4, 1, _p(z), _p(z), _p(z), _p(fl), _p(z), None) == bad      # N % p != 0
    assert lib.dsg_debug_head_patch_f32(L.HEAD_ADJ, 1, 4, 2, 4, 1, _p(z), None, None, _p(fl), _p(z), None) == bad         # no weight


# ----------------------------------------------------------------------------------------------------------------------------------
# the fused E = 96, p = 2 forms
# ----------------------------------------------------------------------------------------------------------------------------------
E = X.E
FUSED_GRIDS = [(8, 3), (16, 2), (20, 2), (2, 129)]      # (N, B): R^2 = 16 (a wave spans two graphs), 64, 100 (a last wave of 8 tokens), 1
                                                         # ((2, 129): every token its own graph, a second block of one lane and three padding waves)


@pytest.mark.parametrize("Ca,Cn,self_cond", [(6, 12, 1), (3, 5, 1), (1, 1, 0), (2, 12, 1)])
@pytest.mark.parametrize("N,B", FUSED_GRIDS)
def test_fused_patch_embed_p2(N, B, Ca, Cn, self_cond):
    """Kps 64 / 32 / 32 / 64; every flag pattern, three self-conditioning forms, with and without the first block's modulate on top; the
    padded nodes' node / self-condition values are NaN"""
    L, lib = _lib()
    gen = _gen(300 + 10 * Ca + Cn + N)
    cin = (2 if self_cond else 1) * (Ca + 2 * Cn)
    Kps = (cin + 31) // 32 * 32
    R_ = N // 2
    M, T = B * R_ * R_, R_ * R_
    t = X.make_pe_inputs(B, N, Ca, Cn, gen)
    q = X.make_pe_params(cin, B, gen)
    W4 = torch.randn(E, cin, 2, 2, generator=gen) / (4 * cin) ** 0.5
    dev = [torch.from_numpy(P.pack_pe_fused(W4, Kps)).cuda(), q["bias"].cuda(), q["gam"].cuda(), q["bet"].cuda(), q["aff"].cuda()]
    worst = (0.0, 0.0, 0.0)
    for pattern in X.FLAG_PATTERNS:
        flags = X.make_flags(B, N, pattern, seed=N)
        pad = ~torch.as_tensor(flags).bool()
        fl = torch.as_tensor(flags).cuda()
        for second in (False, True):
            for mode in ((0, 1, 2) if self_cond else (2,)):
                sc_on = mode == 0
                f64, f32 = (P.patch_embed_formula(P.patch_input(t, flags, 2, bool(self_cond), sc_on, dt), W4, q["bias"], q["gam"], q["bet"], q["aff"],
                                                  q["aff_off"], T) for dt in (torch.float64, torch.float32))
                if second:
                    f64, f32 = X.modulate(f64, q["aff"].double(), q["aff_off2"], T), X.modulate(f32, q["aff"], q["aff_off2"], T)
                d = {k: v.clone() for k, v in t.items()}
                d["node"][pad] = float("nan"); d["sc_node"][pad] = float("nan")
                if mode == 1:
                    d["sc_adj"].fill_(float("nan")); d["sc_node"].fill_(float("nan"))
                d = {k: v.cuda() for k, v in d.items()}
                has_sc = torch.tensor([0], dtype=torch.int32, device="cuda") if mode == 1 else None
                out = _nan(M, E)
                rc = lib.dsg_debug_patch_embed_patch_f32(B, N, 2, Ca, Cn, self_cond, Kps, _p(d["adj"]), _p(d["node"]),
                                                         _p(d["sc_adj"]) if mode < 2 else None, _p(d["sc_node"]) if mode < 2 else None, _p(has_sc),
                                                         _p(fl), *(_p(v) for v in dev), q["aff_ld"], q["aff_off"], q["aff_off2"] if second else -1,
                                                         _p(out), None)
                assert rc == 0
                got = out.cpu()
                assert (_bits(got[M:]) == NAN_BITS).all(), "guard rows written"
                got = got[:M]
                assert torch.isfinite(got).all(), f"{pattern} mode {mode}: a padded node's value reached the result"
                bar, ref_err = R.formula_bar(f64, f32)
                err = float((got.double() - f64).abs().max())
                assert err <= bar, f"{pattern} mode {mode} second {second}: {err:.3e} > {bar:.3e}"
                if worst[1] == 0.0 or err / bar >= worst[0] / worst[1]:
                    worst = (err, bar, ref_err)
    _report(f"fused_patch_embed96_p2 N={N} B={B} Ca={Ca} Cn={Cn} sc={self_cond} Kps={Kps}", *worst)
    bad = lambda p, kps: lib.dsg_debug_patch_embed_patch_f32(B, N, p, Ca, Cn, self_cond, kps, _p(d["adj"]), _p(d["node"]), None, None, None, _p(fl),
                                                            *(_p(v) for v in dev), q["aff_ld"], q["aff_off"], -1, _p(out), None)
    assert bad(4, Kps) == L.DSG_ERR_INVALID and bad(2, 96) == L.DSG_ERR_INVALID and bad(2, Kps - 32 if Kps > 32 else 0) == L.DSG_ERR_INVALID


def _readout_params_p2(Ca, gen):
    q = X.make_readout_params(Ca, gen)
    q["W0"] = torch.randn(E, E, 2, 2, generator=gen) * E ** -0.5
    return q


@pytest.mark.parametrize("B,N,Ca", [(3, 8, 6), (2, 16, 3), (2, 20, 1), (129, 2, 3), (2, 8, 32), (1, 64, 6)])
def test_fused_readout_p2(B, N, Ca):
    """against the UNFOLDED chain in float64 (bar: the float32 evaluation of the kernel's folded chain); the rows of x of every token
    without a valid pixel are NaN.  (3, 8): a wave spans two graphs; (2, 20): token rows straddle tiles, a last tile of 8 tokens;
    (129, 2): one token per graph; (1, 64): R = 32, a token row per tile; (2, 8, 32): the fold's limit on C_adj"""
    L, lib = _lib()
    R_ = N // 2
    M, nseg = B * R_ * R_, (R_ + 30) // 32 + 1
    worst_a, worst_p = (0.0, 1.0, 0.0), (0.0, 1.0, 0.0)
    for pattern in X.FLAG_PATTERNS:
        gen = _gen(4100 + N + Ca)
        flags = X.make_flags(B, N, pattern, seed=N)
        q = _readout_params_p2(Ca, gen)
        x = torch.randn(M, E, generator=gen) + 2.0 * (2.0 * torch.rand(M, 1, generator=gen) - 1.0)
        xn64, xn32 = R.layer_norm(x.double(), q["gam"].double(), q["bet"].double()), R.layer_norm(x, q["gam"], q["bet"])
        out64 = P.adj_head(P.shared_rep(xn64, q, B, N, 2), q, flags, 2)
        fold = P.fold_readout_p2(q)
        f32 = dict(Fa=[v.float() for v in fold["Fa"]], fa=fold["fa"].float())
        out32 = P.folded_adj(xn32, f32, q, flags)
        pool64, pool32 = P.pool_ext_p2(xn64, flags), P.pool_ext_p2(xn32, flags)
        tokv = P.token_valid(flags, 2).reshape(-1)
        xd = x.clone()
        xd[~tokv] = float("nan")
        f2pad = torch.zeros(32, E)
        f2pad[:Ca] = q["F2"]
        fap = np.concatenate([R.pack_rows(v.numpy()) for v in f32["Fa"]])
        dev = [xd.cuda(), q["gam"].cuda(), q["bet"].cuda(), torch.from_numpy(fap).cuda(), f32["fa"].cuda(),
               torch.from_numpy(R.pack_cols(f2pad.numpy())).cuda(), q["f2"].cuda(), torch.as_tensor(flags).cuda()]
        out_adj, pool_part, pool_ext = _nan(1, B * Ca * N * N), _nan(B * R_ * nseg * 2, E), _nan(B * N, 256)
        rc = lib.dsg_debug_readout_patch_f32(B, N, 2, Ca, *(_p(v) for v in dev), _p(out_adj), _p(pool_part), _p(pool_ext), None)
        assert rc == 0
        assert (_bits(out_adj.cpu()[1:]) == NAN_BITS).all() and (_bits(pool_part.cpu()[B * R_ * nseg * 2:]) == NAN_BITS).all()
        assert (_bits(pool_ext.cpu()[B * N:]) == NAN_BITS).all(), "guard rows written"
        got = out_adj.cpu()[0].view(B, Ca, N, N)
        assert torch.isfinite(got).all(), "non-finite adjacency output: a row of x without a valid pixel travelled through"
        mask = X.pair_valid(flags)[:, None].expand(B, Ca, N, N)
        assert (_bits(got)[~mask] == 0).all(), "a masked pixel is not an exact +0"
        bar, ref_err = R.formula_bar(out64, out32)
        err = float((got.double() - out64).abs().max())
        assert err <= bar, f"out_adj {pattern}: {err:.3e} > {bar:.3e}"
        if err / bar >= worst_a[0] / worst_a[1]:
            worst_a = (err, bar, ref_err)
        gp = pool_ext.cpu()[:B * N]
        assert torch.isfinite(gp).all()
        assert (gp[:, 194:] == 0).all()
        bar, ref_err = R.formula_bar(pool64, pool32)
        err = float((gp.double() - pool64).abs().max())
        assert err <= bar, f"pool_ext {pattern}: {err:.3e} > {bar:.3e}"
        if err / bar >= worst_p[0] / worst_p[1]:
            worst_p = (err, bar, ref_err)
    _report(f"fused_readout96_p2 out_adj B={B} N={N} Ca={Ca}", *worst_a)
    _report(f"fused_readout96_p2 pool_ext B={B} N={N} Ca={Ca}", *worst_p)


def test_fused_p2_refusals():
    L, lib = _lib()
    d = torch.zeros(1 << 16, device="cuda")
    f = torch.ones(64, dtype=torch.uint8, device="cuda")
    ro = lambda p, N, Ca: lib.dsg_debug_readout_patch_f32(1, N, p, Ca, *([_p(d)] * 7), _p(f), _p(d), _p(d), _p(d), None)
    assert ro(4, 8, 3) == L.DSG_ERR_INVALID and ro(1, 8, 3) == L.DSG_ERR_INVALID     # p = 2 only
    assert ro(2, 7, 3) == L.DSG_ERR_INVALID and ro(2, 8, 33) == L.DSG_ERR_INVALID    # odd N; beyond the fold's 32 output rows
