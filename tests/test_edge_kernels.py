"""GPU: the kernels around the fp32 forward's GEMMs on their own (csrc/kernels.hip: fused_patch_embed96_kernel in its four instantiations
with and without a run list, fused_readout96_kernel + pool_finish_kernel, the one-wave-per-row passes mod_stats / ln_stats / ln_mod /
merge_ln / breakup_ln, merge_norm_runs_kernel, the pure-window copies window_broadcast_kernel<24 | 0> / window_harvest_kernel, and the
unfused chain's assemble / head_adj / pool / head_node) through the dsg_debug_*_f32 hooks.  EVERY output element is compared with a
float64 evaluation of the same operation (tests/edge_ref.py) at the smallest shapes that reach each edge: rows that straddle 32-token
tiles, a partially filled last tile, the padding waves of a last block, sample boundaries inside a block of four rows, sentinel and
out-of-range list entries, device-side counts.

Conventions of tests/test_f32_kernels.py: outputs are NaN-filled and carry guard rows; what a kernel must write is finite and inside
its bar, everything else bit-identical afterwards (for in-place kernels: to a clone of the input).  The read-out's input rows of masked
tokens and the PatchEmbed's unused self-condition tensors are NaN: a read of them shows.  Bars are derived in tests/edge_ref.py, none
from a kernel's output; each test prints its worst |err| / bar (lines EDGEK ...); measured figures: profiles/f32_kernel_errors.md.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import edge_ref as X
import f32_ref as R

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000
GUARD = 2      # rows behind every output buffer
E = X.E


def _lib():
    from diffusesg_amd import lib as L
    return L, L.load()


def _p(t):
    """the device address of a tensor the CALLER keeps alive: a temporary would be freed, and its block reused, before the launch"""
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev(t):
    return None if t is None else t.contiguous().cuda()


def _nan(rows, cols):
    return torch.full((rows + GUARD, cols), float("nan"), device="cuda")


def _bits(t):
    return t.contiguous().view(torch.int32).cpu()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rows(M, Cc, gen):
    return torch.randn(M, Cc, generator=gen) + 2.0 * (2.0 * torch.rand(M, 1, generator=gen) - 1.0)


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


class Worst:
    """the largest |err| / bar of a test, printed once at its end"""

    def __init__(self, family):
        self.family, self.r, self.n = family, 0.0, 0

    def formula(self, got, f64, f32, sel=None, what=""):
        """got (CPU) against the float64 formula under formula_bar, on the elements `sel` (all when None)"""
        bar, ref_err = R.formula_bar(f64, f32)
        g, f = (got, f64) if sel is None else (got[sel], f64[sel])
        assert torch.isfinite(g).all(), f"{self.family} {what}: non-finite values in the result"
        err = float((g.double() - f).abs().max()) if g.numel() else 0.0
        assert err <= bar, f"{self.family} {what}: max error {err:.3e} above the bar {bar:.3e} (float32 formula: {ref_err:.3e})"
        self.r, self.n = max(self.r, err / bar if bar > 0 else 0.0), self.n + 1

    def bound(self, got, ref, bnd, what=""):
        assert torch.isfinite(got).all(), f"{self.family} {what}: non-finite values in the result"
        r = R.worst_ratio(got, ref, bnd)
        assert r <= 1.0, f"{self.family} {what}: {r:.2f} x the derived bound"
        self.r, self.n = max(self.r, r), self.n + 1

    def done(self):
        print(f"EDGEK {self.family}: worst |err| / bar = {self.r:.3f} over {self.n} checks")


def _untouched(buf, must_write=None, what=""):
    """buf (device, NaN-filled before the launch): every element outside the bool mask `must_write` still holds the fill, bit for bit"""
    keep = _bits(buf) == NAN_BITS
    if must_write is None:
        assert keep.all(), f"{what}: {int((~keep).sum())} elements were written"
    else:
        assert keep[~must_write].all(), f"{what}: {int((~keep[~must_write]).sum())} elements written outside the result"


def _rows_written(M, cols, rows=None):
    m = torch.zeros(M + GUARD, cols, dtype=torch.bool)
    if rows is None:
        m[:M] = True
    else:
        m[:M][rows] = True
    return m


# ----------------------------------------------------------------------------------------------------------------------------------
# read-out
# ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _readout_wave_classes():
    tot = np.zeros(3, np.int64)
    for (B, N, Ca) in X.READOUT_CASES:
        for pat in X.FLAG_PATTERNS:
            tot += np.array(X.wave_classes(X.make_flags(B, N, pat)))
    return tuple(int(v) for v in tot)


@pytest.mark.parametrize("B,N,Ca", X.READOUT_CASES)
def test_fused_readout96(B, N, Ca):
    """final LayerNorm + the folded read_out / adjacency-head chain + masked output, and the LN(x) pooling with pool_finish_kernel, against
    the UNFOLDED chain in float64; the rows of x of every masked token are NaN.  (129, 1): every token its own row, a second block with one
    live lane and three padding waves; (3, 5): graph boundaries inside a tile, rows straddling tiles, a last tile with 11 tokens; (1, 33) /
    (1, 34): 2 and 3 pooling slots per row; (2, 8, 32): the fold's limit on C_adj"""
    L, lib = _lib()
    shortcut, mixed, met = _readout_wave_classes()
    assert shortcut >= 1 and mixed >= 1 and met >= 1, "the case set no longer reaches the all-masked shortcut / a mixed wave"
    M, nseg = B * N * N, X.readout_segments(N)
    w_adj, w_pool = Worst(f"fused_readout96 out_adj B={B} N={N} Ca={Ca}"), Worst(f"fused_readout96 pool_ext B={B} N={N} Ca={Ca}")
    for k, pat in enumerate(X.FLAG_PATTERNS):
        gen = _gen(4000)
        flags = X.make_flags(B, N, pat)
        p = X.make_readout_params(Ca, gen)
        x = _rows(M, E, gen)
        e = X.readout_expect(x, p, flags)
        valid = X.pair_valid(flags)
        xd = x.clone()
        xd[~valid.reshape(-1)] = float("nan")          # with masked-token pruning these rows are never computed
        f2pad = torch.zeros(32, E)
        f2pad[:Ca] = p["F2"]
        dev = [_dev(xd), _dev(p["gam"]), _dev(p["bet"]), _dev(torch.from_numpy(R.pack_rows(e["fold32"]["Fa"].numpy()))), _dev(e["fold32"]["fa"]),
               _dev(torch.from_numpy(R.pack_cols(f2pad.numpy()))), _dev(p["f2"]), _dev(torch.from_numpy(flags))]
        out_adj, pool_part, pool_ext = _nan(1, B * Ca * N * N), _nan(B * N * nseg, E), _nan(B * N, 128)
        rc = lib.dsg_debug_readout_f32(B, N, Ca, *(_p(t) for t in dev), _p(out_adj), _p(pool_part), _p(pool_ext), None)
        assert rc == 0, f"dsg_debug_readout_f32 status {rc}"
        _untouched(out_adj, _rows_written(1, B * Ca * N * N), "out_adj")
        _untouched(pool_part[B * N * nseg:], None, "pool_part guard")
        _untouched(pool_ext, _rows_written(B * N, 128), "pool_ext")
        got = out_adj.cpu()[0].view(B, Ca, N, N)
        assert torch.isfinite(got).all(), "non-finite adjacency output: a stale row of x travelled through"
        assert (got[~valid[:, None].expand(B, Ca, N, N)] == 0).all(), "a masked position is not an exact zero"
        w_adj.formula(got, e["out64"], e["out32"], what=pat)
        gp = pool_ext.cpu()[:B * N]
        w_pool.bound(gp, e["pool64"], e["pool_bound"], what=pat)
        w_pool.formula(gp, e["pool64"], e["pool32"], what=pat + " (formula bar)")
    w_adj.done()
    w_pool.done()


def test_fused_readout96_refuses_what_is_not_built():
    L, lib = _lib()
    d = torch.zeros(4096, device="cuda")
    f = torch.ones(8, dtype=torch.uint8, device="cuda")
    args = lambda Ca, x: (1, 2, Ca, x, _p(d), _p(d), _p(d), _p(d), _p(d), _p(d), _p(f), _p(d), _p(d), _p(d), None)
    assert lib.dsg_debug_readout_f32(*args(33, _p(d))) == L.DSG_ERR_INVALID       # beyond the fold's 32 output rows
    assert lib.dsg_debug_readout_f32(*args(3, None)) == L.DSG_ERR_INVALID


# ----------------------------------------------------------------------------------------------------------------------------------
# PatchEmbed and the input assembly
# ----------------------------------------------------------------------------------------------------------------------------------
def _sc_states(sc):
    """(name, the self-condition tensors take part, how they are passed): pointers null; has_sc null with pointers set; *has_sc = 1;
    *has_sc = 0 with NaN-filled tensors.  Without self-conditioning the tensors are never read, whatever has_sc says"""
    if sc:
        return [("null", False), ("no_flag", True), ("one", True), ("zero_nan", False)]
    return [("null", False), ("ignored_nan", False)]


def _sc_dev(state, t):
    """device (sc_adj, sc_node, has_sc) of a state"""
    if state == "null":
        return None, None, None
    if state in ("zero_nan", "ignored_nan"):
        nan = lambda v: torch.full_like(v, float("nan")).cuda()
        return nan(t["sc_adj"]), nan(t["sc_node"]), _i32([0 if state == "zero_nan" else 1])
    return _dev(t["sc_adj"]), _dev(t["sc_node"]), (None if state == "no_flag" else _i32([1]))


@pytest.mark.parametrize("B,N", X.PE_GRIDS)
@pytest.mark.parametrize("Ca,Cn,sc", X.PE_CONFIGS)
def test_fused_patch_embed96(Ca, Cn, sc, B, N):
    """(6, 12, 1), (3, 12, 1): the compile-time forms; (3, 5, 1), (6, 12, 0): Kp 32; (2, 12, 1): the generic Kp 64 form; (4, 6, 1),
    (8, 12, 1): in_chans == Kp.  Every self-condition state, flag pattern, and aff_off2 = -1 / a second offset; aff_off != 0,
    aff_ld > aff_off + 2 * 96.  (129, 1): a second block with one live lane and three padding waves"""
    L, lib = _lib()
    gen = _gen(100 * Ca + Cn + 7 * N + sc)
    M, T, Kp = B * N * N, N * N, X.pe_kp(Ca, Cn, sc)
    cin = (2 if sc else 1) * (Ca + 2 * Cn)
    t = X.make_pe_inputs(B, N, Ca, Cn, gen)
    p = X.make_pe_params(cin, B, gen)
    dev = [_dev(torch.from_numpy(R.pack_rows(X.pad_k(p["W"], Kp).numpy()))), _dev(p["bias"]), _dev(p["gam"]), _dev(p["bet"]), _dev(p["aff"])]
    dadj, dnode = _dev(t["adj"]), _dev(t["node"])
    w = Worst(f"fused_patch_embed96 Ca={Ca} Cn={Cn} sc={sc} Kp={Kp} B={B} N={N}")
    for pat in X.FLAG_PATTERNS:
        flags = X.make_flags(B, N, pat)
        dflags = _dev(torch.from_numpy(flags))
        for second in (False, True):
            ref = {}
            for state, sc_on in _sc_states(sc):
                if sc_on not in ref:
                    ref[sc_on] = [X.pe_formula(X.pe_input(t, flags, sc, sc_on, dt), p, T, second, dt) for dt in (torch.float64, torch.float32)]
                sca, scn, has = _sc_dev(state, t)
                out = _nan(M, E)
                rc = lib.dsg_debug_patch_embed_f32(B, N, Ca, Cn, sc, Kp, _p(dadj), _p(dnode), _p(sca), _p(scn), _p(has), _p(dflags),
                                                   *(_p(v) for v in dev), p["aff_ld"], p["aff_off"], (p["aff_off2"] if second else -1), _p(out),
                                                   None, None, None)
                assert rc == 0, f"dsg_debug_patch_embed_f32 status {rc}"
                _untouched(out, _rows_written(M, E), "x")
                w.formula(out.cpu()[:M], *ref[sc_on], what=f"{pat} {state} second={second}")
    w.done()


@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("N", (8, 16))
@pytest.mark.parametrize("Ca,Cn,sc", X.PE_LIST_CONFIGS)
def test_fused_patch_embed96_run_list(Ca, Cn, sc, N, B):
    """the four LIST instantiations: only the listed runs of 8 tokens are computed, each exactly as without a list; -1 pads, stale runs
    behind the device-side count, rows of unlisted runs untouched"""
    L, lib = _lib()
    gen = _gen(9000 + 100 * Ca + Cn + N + B)
    M, T, Kp = B * N * N, N * N, X.pe_kp(Ca, Cn, sc)
    t = X.make_pe_inputs(B, N, Ca, Cn, gen)
    p = X.make_pe_params(2 * (Ca + 2 * Cn), B, gen)
    dev = [_dev(torch.from_numpy(R.pack_rows(X.pad_k(p["W"], Kp).numpy()))), _dev(p["bias"]), _dev(p["gam"]), _dev(p["bet"]), _dev(p["aff"])]
    dadj, dnode, dsca, dscn, one = _dev(t["adj"]), _dev(t["node"]), _dev(t["sc_adj"]), _dev(t["sc_node"]), _i32([1])
    w = Worst(f"fused_patch_embed96 run list Ca={Ca} Cn={Cn} Kp={Kp} B={B} N={N}")
    for k, cnt in enumerate(R.ROW_COUNTS):
        cnt = min(cnt, M // 8)
        flags = X.make_flags(B, N, X.FLAG_PATTERNS[k % 3])
        second = bool(k % 2)
        f64, f32 = (X.pe_formula(X.pe_input(t, flags, sc, True, dt), p, T, second, dt) for dt in (torch.float64, torch.float32))
        runs, lst = R.make_run_list(M // 8, cnt, 1 if cnt in (0, 1, 16) else 0, gen)
        out, dflags, dlst, dcnt = _nan(M, E), _dev(torch.from_numpy(flags)), _i32(lst), _i32([cnt])
        rc = lib.dsg_debug_patch_embed_f32(B, N, Ca, Cn, sc, Kp, _p(dadj), _p(dnode), _p(dsca), _p(dscn), _p(one), _p(dflags),
                                           *(_p(v) for v in dev), p["aff_ld"], p["aff_off"], (p["aff_off2"] if second else -1), _p(out),
                                           _p(dlst), _p(dcnt), None)
        assert rc == 0, f"dsg_debug_patch_embed_f32 status {rc}"
        rows = X.runs_rows(M, runs)
        _untouched(out, _rows_written(M, E, rows), "x")
        w.formula(out.cpu()[:M], f64, f32, sel=rows, what=f"count {cnt}")
    w.done()


def test_fused_patch_embed96_refuses_what_is_not_built():
    L, lib = _lib()
    d = torch.zeros(1 << 16, device="cuda")
    f = torch.ones(64, dtype=torch.uint8, device="cuda")
    lst, cnt = _i32([0] + [-1] * 15), _i32([1])

    def call(N=8, Ca=3, Cn=5, sc=1, Kp=32, aff_ld=400, aff_off=8, run_list=None, run_cnt=None):
        return lib.dsg_debug_patch_embed_f32(1, N, Ca, Cn, sc, Kp, _p(d), _p(d), None, None, None, _p(f), _p(d), _p(d), _p(d), _p(d), _p(d), aff_ld,
                                             aff_off, -1, _p(d), run_list, run_cnt, None)
    assert call() == 0
    assert call(N=5, run_list=_p(lst), run_cnt=_p(cnt)) == L.DSG_ERR_INVALID      # runs of 8 tokens need N % 8 == 0
    assert call(run_list=_p(lst)) == L.DSG_ERR_INVALID                            # a list without its count
    assert call(Kp=96) == L.DSG_ERR_INVALID                                       # no such fragment count
    assert call(Ca=6, Cn=12, Kp=32) == L.DSG_ERR_INVALID                          # 60 channels do not fit Kp = 32
    assert call(aff_off=6) == L.DSG_ERR_INVALID                                   # 16-byte reads of the (scale | shift) row


@pytest.mark.parametrize("B,N", [(3, 5), (2, 8), (129, 1)])
@pytest.mark.parametrize("Ca,Cn,sc", X.PE_CONFIGS)
def test_assemble(Ca, Cn, sc, B, N):
    """assemble_kernel: the gathered input, zero-padded to Kp (the PatchEmbed's, and one that is no multiple of 32) -- copies, bit for bit"""
    L, lib = _lib()
    gen = _gen(500 + 10 * Ca + Cn + N)
    M = B * N * N
    cin = (2 if sc else 1) * (Ca + 2 * Cn)
    t = X.make_pe_inputs(B, N, Ca, Cn, gen)
    dadj, dnode = _dev(t["adj"]), _dev(t["node"])
    for k, pat in enumerate(X.FLAG_PATTERNS):
        flags = X.make_flags(B, N, pat)
        dflags = _dev(torch.from_numpy(flags))
        for Kp in (X.pe_kp(Ca, Cn, sc), cin + 3):
            for state, sc_on in _sc_states(sc):
                want = X.pad_k(X.pe_input(t, flags, sc, sc_on, torch.float32), Kp)
                sca, scn, has = _sc_dev(state, t)
                out = _nan(M, Kp)
                rc = lib.dsg_debug_assemble_f32(B, N, Ca, Cn, sc, Kp, _p(dadj), _p(dnode), _p(sca), _p(scn), _p(has), _p(dflags), _p(out), None)
                assert rc == 0
                _untouched(out[M:], None, "guard rows")
                assert torch.equal(_bits(out[:M]), _bits(want)), f"assemble {pat} {state} Kp={Kp}: not the gathered input bit for bit"
    assert lib.dsg_debug_assemble_f32(B, N, Ca, Cn, sc, cin - 1, _p(dadj), _p(dnode), None, None, None, _p(dflags), _p(out), None) == L.DSG_ERR_INVALID


# ----------------------------------------------------------------------------------------------------------------------------------
# the unfused read-out tails
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", [(3, 5), (2, 8), (1, 33), (129, 1)])
@pytest.mark.parametrize("Ee", (96, 70))
def test_unfused_tails(Ee, B, N):
    """head_adj, pool and head_node of the fall-back chain: one wave per row over E (E = 70: a second, partial pass of the lane loop)"""
    L, lib = _lib()
    gen = _gen(600 + Ee + N)
    M, Ca, Cn = B * N * N, 3, 7
    h, hn = _rows(M, Ee, gen), _rows(B * N, Ee, gen)
    W, bias = torch.randn(Ca, Ee, generator=gen) / Ee ** 0.5, torch.randn(Ca, generator=gen) * 0.3
    Wn, bn = torch.randn(Cn, Ee, generator=gen) / Ee ** 0.5, torch.randn(Cn, generator=gen) * 0.3
    dh, dhn, dW, db, dWn, dbn = (_dev(v) for v in (h, hn, W, bias, Wn, bn))
    wa, wp, wn = Worst(f"head_adj E={Ee} B={B} N={N}"), Worst(f"pool E={Ee} B={B} N={N}"), Worst(f"head_node E={Ee} B={B} N={N}")
    for pat in X.FLAG_PATTERNS:
        flags = X.make_flags(B, N, pat)
        dflags = _dev(torch.from_numpy(flags))
        valid = X.pair_valid(flags)
        out = _nan(1, B * Ca * N * N)
        assert lib.dsg_debug_head_f32(L.HEAD_ADJ, B, N, Ee, Ca, _p(dh), _p(dW), _p(db), _p(dflags), _p(out), None) == 0
        _untouched(out, _rows_written(1, B * Ca * N * N), "head_adj")
        got = out.cpu()[0].view(B, Ca, N, N)
        assert (got[~valid[:, None].expand(B, Ca, N, N)] == 0).all()
        wa.formula(got, X.head_adj_formula(h.double(), W.double(), bias.double(), flags), X.head_adj_formula(h, W, bias, flags), what=pat)
        out = _nan(B * N, Ee)
        assert lib.dsg_debug_head_f32(L.HEAD_POOL, B, N, Ee, 0, _p(dh), None, None, _p(dflags), _p(out), None) == 0
        _untouched(out, _rows_written(B * N, Ee), "pool")
        wp.formula(out.cpu()[:B * N], X.pool_formula(h.double(), flags), X.pool_formula(h, flags), what=pat)
        out = _nan(B * N, Cn)
        assert lib.dsg_debug_head_f32(L.HEAD_NODE, B, N, Ee, Cn, _p(dhn), _p(dWn), _p(dbn), _p(dflags), _p(out), None) == 0
        _untouched(out, _rows_written(B * N, Cn), "head_node")
        got = out.cpu()[:B * N]
        assert (got[torch.from_numpy(flags).reshape(-1) == 0] == 0).all()
        wn.formula(got, X.head_node_formula(hn.double(), Wn.double(), bn.double(), flags), X.head_node_formula(hn, Wn, bn, flags), what=pat)
    for v in (wa, wp, wn):
        v.done()
    assert lib.dsg_debug_head_f32(3, B, N, Ee, Ca, _p(dh), _p(dW), _p(db), _p(dflags), _p(out), None) == L.DSG_ERR_INVALID
    assert lib.dsg_debug_head_f32(L.HEAD_ADJ, B, N, Ee, Ca, _p(dh), None, _p(db), _p(dflags), _p(out), None) == L.DSG_ERR_INVALID


# ----------------------------------------------------------------------------------------------------------------------------------
# one-wave-per-row passes
# ----------------------------------------------------------------------------------------------------------------------------------
def _row(lib, kind, B, t, Cc, x, g=None, b=None, pg=None, pb=None, aff=None, aff_ld=0, aff_off=0, ln_part=None, nparts=0, y=None, stats=None,
         run_list=None, run_cnt=None):
    return lib.dsg_debug_row_f32(kind, B, t, Cc, _p(x), _p(g), _p(b), _p(pg), _p(pb), _p(aff), aff_ld, aff_off, _p(ln_part), nparts, _p(y), _p(stats),
                                 _p(run_list), _p(run_cnt), None)


@pytest.mark.parametrize("Cc", X.ROW_C)
def test_row_passes(Cc):
    """mod_stats (in place, + statistics of the new row), ln_stats, ln_mod at M = 1, 3, 4, 5, 9 rows -- blocks of four rows with a sample
    boundary inside, a last block with one row --, aff_off != 0 and aff_ld > 2 C"""
    L, lib = _lib()
    wm, ws, wl, wn = Worst(f"mod_stats rows C={Cc}"), Worst(f"mod_stats (mean, rstd) C={Cc}"), Worst(f"ln_stats C={Cc}"), Worst(f"ln_mod C={Cc}")
    off, ld = 8, 8 + 2 * Cc + 4
    for B, T in X.ROW_BT:
        gen = _gen(1000 + Cc + 10 * B + T)
        M = B * T
        x = _rows(M, Cc, gen)
        gam, bet = 1.0 + 0.2 * torch.randn(Cc, generator=gen), 0.2 * torch.randn(Cc, generator=gen)
        aff = torch.randn(B, ld, generator=gen) * 0.5
        daff, dg, db = _dev(aff), _dev(gam), _dev(bet)
        written = _rows_written(M, 2)
        # mod_stats
        x_io = torch.cat([x, torch.full((GUARD, Cc), float("nan"))]).cuda()
        x_in, st = x_io.clone(), _nan(M, 2)
        assert _row(lib, L.ROW_MOD_STATS, B, T, Cc, x_io, aff=daff, aff_ld=ld, aff_off=off, stats=st) == 0
        assert torch.equal(_bits(x_io[M:]), _bits(x_in[M:])), "mod_stats wrote behind its rows"
        _untouched(st, written, "mod_stats stats")
        f64 = X.modulate(x.double(), aff.double(), off, T)
        got = x_io.cpu()[:M]
        wm.formula(got, f64, X.modulate(x, aff, off, T))
        bound, _ = X.row_stats_bound(f64)      # the statistics of the STORED row; the bound from the reference's magnitudes
        ws.bound(st.cpu()[:M], X.row_stats(got.double()), bound)
        # ln_stats
        st = _nan(M, 2)
        assert _row(lib, L.ROW_LN_STATS, B, T, Cc, _dev(x), stats=st) == 0
        _untouched(st, written, "ln_stats")
        bound, _ = X.row_stats_bound(x.double())
        wl.bound(st.cpu()[:M], X.row_stats(x.double()), bound)
        # ln_mod
        y = _nan(M, Cc)
        assert _row(lib, L.ROW_LN_MOD, B, T, Cc, _dev(x), g=dg, b=db, aff=daff, aff_ld=ld, aff_off=off, y=y) == 0
        _untouched(y, _rows_written(M, Cc), "ln_mod")
        wn.formula(y.cpu()[:M], X.ln_mod_formula(x.double(), gam.double(), bet.double(), aff.double(), off, T), X.ln_mod_formula(x, gam, bet, aff, off, T))
    for v in (wm, ws, wl, wn):
        v.done()


def test_row_passes_refuse_what_a_wave_cannot_hold():
    L, lib = _lib()
    d = torch.zeros(1 << 14, device="cuda")
    assert _row(lib, L.ROW_LN_STATS, 1, 1, 1536, d, stats=d) == 0
    assert _row(lib, L.ROW_LN_STATS, 1, 1, 1540, d, stats=d) == L.DSG_ERR_INVALID       # more than 24 values per lane
    assert _row(lib, L.ROW_LN_STATS, 1, 1, 98, d, stats=d) == L.DSG_ERR_INVALID         # float4 pieces
    assert _row(lib, L.ROW_MOD_STATS, 1, 1, 96, d, aff=d, aff_ld=200, aff_off=6, stats=d) == L.DSG_ERR_INVALID
    assert _row(lib, L.ROW_MERGE_LN, 1, 2, 768, d, g=d, b=d, y=d) == L.DSG_ERR_INVALID  # a merged row of 3072 channels
    assert _row(lib, L.ROW_MERGE_LN, 1, 3, 96, d, g=d, b=d, y=d) == L.DSG_ERR_INVALID   # an odd side
    assert _row(lib, L.ROW_BREAKUP_LN, 1, 1, 392, d, g=d, b=d, pg=d, pb=d, y=d) == L.DSG_ERR_INVALID     # chunks of D / 4 in float4 pieces
    assert _row(lib, L.ROW_BREAKUP_LN, 1, 2, 384, d, g=d, b=d, pg=d, pb=d, y=d, run_list=_i32([0])) == L.DSG_ERR_INVALID
    assert _row(lib, L.ROW_MERGE_NORM_RUNS, 1, 8, 96, d, ln_part=d, nparts=1, y=d, run_list=_i32([0]), run_cnt=_i32([0])) == L.DSG_ERR_INVALID
    assert _row(lib, 6, 1, 1, 96, d, stats=d) == L.DSG_ERR_INVALID


@pytest.mark.parametrize("res", (2, 4, 6))
@pytest.mark.parametrize("Cc", (96, 128, 192, 384))
def test_merge_ln(Cc, res):
    """PatchMerging's gather + LayerNorm(4C), B = 3 (M = 3, 12, 27 merged rows); C = 384 is the widest merged row a wave holds (768 is
    refused: test_row_passes_refuse_what_a_wave_cannot_hold)"""
    L, lib = _lib()
    gen = _gen(res * 1000 + Cc)
    B = 3
    M2 = B * (res // 2) ** 2
    x = _rows(B * res * res, Cc, gen)
    gam, bet = 1.0 + 0.2 * torch.randn(4 * Cc, generator=gen), 0.2 * torch.randn(4 * Cc, generator=gen)
    y = _nan(M2, 4 * Cc)
    assert _row(lib, L.ROW_MERGE_LN, B, res, Cc, _dev(x), g=_dev(gam), b=_dev(bet), y=y) == 0
    _untouched(y, _rows_written(M2, 4 * Cc), "merge_ln")
    w = Worst(f"merge_ln C={Cc} res={res}")
    w.formula(y.cpu()[:M2], X.merge_ln_formula(x.double(), gam.double(), bet.double(), B, res), X.merge_ln_formula(x, gam, bet, B, res))
    w.done()


def _breakup_operands(D, M, gen):
    rn = lambda n: torch.randn(n, generator=gen)
    return _rows(M, D, gen), 1.0 + 0.2 * rn(D), 0.2 * rn(D), 1.0 + 0.2 * rn(D // 4), 0.2 * rn(D // 4)


@pytest.mark.parametrize("res", (1, 2, 3, 4))
@pytest.mark.parametrize("D", X.BREAKUP_D)
def test_breakup_ln(D, res):
    """PatchBreakup's middle, B = 3 (M = 3, 12, 27, 48 coarse rows); D = 1536 fills a wave's registers"""
    L, lib = _lib()
    B = 3
    M, Mf = B * res * res, B * 4 * res * res
    ops = _breakup_operands(D, M, _gen(res * 7000 + D))
    z = _nan(Mf, D // 4)
    dev = [_dev(v) for v in ops]
    assert _row(lib, L.ROW_BREAKUP_LN, B, res, D, dev[0], g=dev[1], b=dev[2], pg=dev[3], pb=dev[4], y=z) == 0
    _untouched(z, _rows_written(Mf, D // 4), "breakup_ln")
    w = Worst(f"breakup_ln D={D} res={res}")
    w.formula(z.cpu()[:Mf], X.breakup_formula(*(v.double() for v in ops), B, res), X.breakup_formula(*ops, B, res))
    w.done()


@pytest.mark.parametrize("B,res", [(3, 4), (1, 8)])
@pytest.mark.parametrize("D", (384, 1536))
def test_breakup_ln_run_list(D, B, res):
    """a run list over the coarse rows (8 per run): counts 0, 1 and all, a -1 inside the list, valid-looking runs behind the count"""
    L, lib = _lib()
    gen = _gen(res * 8000 + D)
    M, Mf, n_runs = B * res * res, B * 4 * res * res, B * res * res // 8
    ops = _breakup_operands(D, M, gen)
    dev = [_dev(v) for v in ops]
    f64, f32 = X.breakup_formula(*(v.double() for v in ops), B, res), X.breakup_formula(*ops, B, res)
    lst = torch.randperm(n_runs, generator=gen).tolist()
    lst[1] = -1
    w = Worst(f"breakup_ln run list D={D} B={B} res={res}")
    for cnt in (0, 1, n_runs):
        z = _nan(Mf, D // 4)
        assert _row(lib, L.ROW_BREAKUP_LN, B, res, D, dev[0], g=dev[1], b=dev[2], pg=dev[3], pb=dev[4], y=z, run_list=_i32(lst), run_cnt=_i32([cnt])) == 0
        rows = X.breakup_rows(B, res, [r for r in lst[:cnt] if r >= 0])
        _untouched(z, _rows_written(Mf, D // 4, rows), "breakup_ln")
        w.formula(z.cpu()[:Mf], f64, f32, sel=rows, what=f"count {cnt}")
    w.done()


@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("Cc", (96, 192))
@pytest.mark.parametrize("res", (16, 32))
def test_merge_norm_runs(res, Cc, B):
    """the merge over a run list of merged rows: fmaf(x, rstd, -mean rstd) with the statistics from the four fine rows' partials (one and
    two per row); counts 0, 1 and all; -1 pads, an out-of-range entry, stale entries behind the count"""
    L, lib = _lib()
    gen = _gen(res + Cc + B)
    x, o = X.merge_norm_case(B, res, Cc, gen)
    ref, bound = X.merge_norm_expect(o)
    M2 = B * (res // 2) ** 2
    n_runs, nparts = M2 // 8, (Cc + 95) // 96
    lst = torch.randperm(n_runs, generator=gen).tolist()
    lst[1], lst[2] = -1, n_runs + 3
    dx, dpart = _dev(x), _dev(o["ln_part"])
    w = Worst(f"merge_norm_runs res={res} C={Cc} B={B}")
    for cnt in (0, 1, n_runs):
        y = _nan(M2, 4 * Cc)
        assert _row(lib, L.ROW_MERGE_NORM_RUNS, B, res, Cc, dx, ln_part=dpart, nparts=nparts, y=y, run_list=_i32(lst), run_cnt=_i32([cnt])) == 0
        rows = X.runs_rows(M2, [r for r in lst[:cnt] if 0 <= r < n_runs])
        _untouched(y, _rows_written(M2, 4 * Cc, rows), "merge_norm_runs")
        w.bound(y.cpu()[:M2][rows], ref[rows], bound[rows], what=f"count {cnt}")
    w.done()


# ----------------------------------------------------------------------------------------------------------------------------------
# pure-window copies: bit for bit
# ----------------------------------------------------------------------------------------------------------------------------------
COPY_VARIANTS = [(False, 0), (True, 1), (True, 2), (False, 4), (True, 4), (False, 1)]     # (skip, nparts; 0: no statistics)


def _copy_buffers(B, res, Cc, skip, nparts):
    """distinct values per element, so that a transposed or shifted window shows"""
    n = B * res * res
    x = np.arange(n * Cc, dtype=np.float32).reshape(n, Cc)
    sk = -(np.arange(n * Cc, dtype=np.float32) + 1.0).reshape(n, Cc) if skip else None
    st = (np.arange(n * nparts * 2, dtype=np.float32) * 0.5 + 0.25).reshape(n, 2 * nparts) if nparts else None
    return [x, sk, st]


def _to_dev(bufs):
    return [None if a is None else torch.from_numpy(a).cuda() for a in bufs]


def _same(dev, want, what):
    for d, wv, name in zip(dev, want, ("x", "skip", "stats")):
        if d is not None:
            assert np.array_equal(d.cpu().numpy().view(np.int32), wv.view(np.int32)), f"{what}: {name} differs from the copy built by index"


@pytest.mark.parametrize("Cc", (96, 192, 384))
@pytest.mark.parametrize("res", (8, 16, 32))
def test_window_broadcast_representatives(res, Cc):
    """window_broadcast_kernel<24> (C = 96) and <0>: rep[b] inside graph b, one representative for the batch, rep[b] = -1, src == dst,
    entries of -1 and out of range, a count below the list's length; B = 3"""
    L, lib = _lib()
    B, nW = 3, (res // 8) ** 2
    k0 = (res // 8 + Cc // 96) % len(COPY_VARIANTS)
    for v in range(2):
        skip, nparts = COPY_VARIANTS[(k0 + 3 * v) % len(COPY_VARIANTS)]
        bufs = _copy_buffers(B, res, Cc, skip, nparts)
        reps = {"per graph": [b * nW + (b % nW) for b in range(B)], "batch": [1 * nW + (nW - 1)] * B, "one graph without": [0, -1, 2 * nW + nW - 1],
                "out of range": [B * nW, -1, -5]}
        for name, rep in reps.items():
            fill = [w for w in range(B * nW) if w not in rep]
            lst = [rep[0]] + fill[:2] + [-1, B * nW + 2] + fill[2:] + [rep[-1]]      # its own representative listed: src == dst
            cnt = max(len(lst) - 3, 0)                                              # the last entries lie behind the count
            dev, dlst, dcnt, drep = _to_dev(bufs), _i32(lst), _i32([cnt]), _i32(rep)
            rc = lib.dsg_debug_window_broadcast_f32(B, res, Cc, _p(dev[0]), _p(dev[1]), _p(dev[2]), nparts, _p(dlst), _p(dcnt), _p(drep),
                                                    None, 0, 0, 0, 0, 0, L.DD_GRAPH, 0, 0, None, None)
            assert rc == 0, f"dsg_debug_window_broadcast_f32 status {rc}"
            _same(dev, X.broadcast_expect(bufs, B, res, lst, cnt, rep), f"{name} skip={skip} nparts={nparts}")
    # src == dst for every entry: nothing moves
    dev, dlst, dcnt, drep = _to_dev(bufs), _i32([0] * 4), _i32([4]), _i32([0] * B)
    assert lib.dsg_debug_window_broadcast_f32(B, res, Cc, _p(dev[0]), _p(dev[1]), _p(dev[2]), nparts, _p(dlst), _p(dcnt), _p(drep),
                                              None, 0, 0, 0, 0, 0, L.DD_BATCH, 0, 0, None, None) == 0
    _same(dev, bufs, "src == dst")


def _table(entries, Cc, nparts, skip):
    """[entries + 1 guard entry, stride] of distinct values, and (off_x, off_skip, off_st)"""
    off_x, off_skip = 4, 4 + 64 * Cc
    off_st = off_skip + 64 * Cc + 2
    stride = off_st + 128 * max(nparts, 1) + 6
    stride += (-stride) % 4
    tab = (np.arange((entries + 1) * stride, dtype=np.float32) + 0.125).reshape(entries + 1, stride) * -1.0
    return tab, stride, (off_x, off_skip, off_st)


@pytest.mark.parametrize("Cc", (96, 192, 384))
@pytest.mark.parametrize("res", (8, 16, 32))
def test_window_broadcast_table(res, Cc):
    """table mode: two entries, the step's schedule index selects the entry; a step beyond n_steps - 1 and a schedule index beyond the
    table are clamped; with another mode in *tab.mode the representative is used although a table is given"""
    L, lib = _lib()
    B, nW = 3, (res // 8) ** 2
    skip, nparts = COPY_VARIANTS[(res // 8 + Cc // 96 + 1) % len(COPY_VARIANTS)]
    bufs = _copy_buffers(B, res, Cc, skip, nparts)
    tab, stride, offs = _table(2, Cc, nparts, skip)
    dtab = torch.from_numpy(tab).cuda()
    lst = [B * nW - 1, -1, 0, B * nW, nW]
    lst = list(dict.fromkeys(lst))
    cnt = len(lst) - (1 if len(lst) > 3 else 0)
    sched = (C.c_int32 * 3)(0, 1, 5)
    dlst, dcnt = _i32(lst), _i32([cnt])
    for step, entry in ((0, 0), (1, 1), (2, 1), (9, 1), (-3, 0)):
        dev = _to_dev(bufs)
        rc = lib.dsg_debug_window_broadcast_f32(B, res, Cc, _p(dev[0]), _p(dev[1]), _p(dev[2]), nparts, _p(dlst), _p(dcnt), None,
                                                _p(dtab), 2, stride, *offs, L.DD_TABLE, step, 3, sched, None)
        assert rc == 0, f"dsg_debug_window_broadcast_f32 status {rc}"
        want = X.broadcast_table_expect(bufs, B, res, lst, cnt, tab, entry, offs, (Cc, Cc, 2 * nparts))
        _same(dev, want, f"table step {step}")
    rep = [nW - 1] * B if nW > 1 else [2] * B
    dev, drep = _to_dev(bufs), _i32(rep)
    assert lib.dsg_debug_window_broadcast_f32(B, res, Cc, _p(dev[0]), _p(dev[1]), _p(dev[2]), nparts, _p(dlst), _p(dcnt), _p(drep),
                                              _p(dtab), 2, stride, *offs, L.DD_BATCH, 1, 3, sched, None) == 0
    _same(dev, X.broadcast_expect(bufs, B, res, lst, cnt, rep), "table given, mode DD_BATCH")
    assert torch.equal(_bits(dtab), torch.from_numpy(tab.view(np.int32))), "the table was written"
    bad = lambda **kw: lib.dsg_debug_window_broadcast_f32(B, kw.get("res", res), Cc, _p(dev[0]), _p(dev[1]), _p(dev[2]), nparts, _p(dlst), _p(dcnt),
                                                          kw.get("rep"), kw.get("tab"), 2, stride, *offs, kw.get("mode", L.DD_TABLE), 0, kw.get("n", 3), sched, None)
    assert bad(tab=None) == L.DSG_ERR_INVALID               # the table mode without a table
    assert bad(tab=_p(dtab), n=0) == L.DSG_ERR_INVALID      # no step rows
    assert bad(tab=None, mode=L.DD_BATCH) == L.DSG_ERR_INVALID   # no representatives
    assert bad(tab=_p(dtab), res=12) == L.DSG_ERR_INVALID


@pytest.mark.parametrize("Cc", (96, 192, 384))
@pytest.mark.parametrize("res", (8, 16, 32))
def test_window_harvest(res, Cc):
    """window 0 of each of the first n graphs -> entry g in window order t = 8 row + col (layout checked directly), everything else of the
    table untouched; then the round trip: the harvested entry broadcast into ANOTHER graph's last window gives that graph's rows back"""
    L, lib = _lib()
    B, n, nW = 3, 2, (res // 8) ** 2
    for skip, nparts in (COPY_VARIANTS[(res // 8 + Cc // 96) % 6], COPY_VARIANTS[(res // 8 + Cc // 96 + 2) % 6]):
        bufs = _copy_buffers(B, res, Cc, skip, nparts)
        dev = _to_dev(bufs)
        _, stride, offs = _table(n, Cc, nparts, skip)
        dtab = torch.full((n + 1, stride), float("nan"), device="cuda")
        rc = lib.dsg_debug_window_harvest_f32(n, res, Cc, _p(dev[0]), _p(dev[1]), _p(dev[2]), nparts, _p(dtab), stride, *offs, None)
        assert rc == 0, f"dsg_debug_window_harvest_f32 status {rc}"
        want = np.full((n + 1, stride), NAN_BITS, np.int32).view(np.float32)
        for g in range(n):
            rows = g * res * res + X.window_rows(res, 0)
            for a, off, wd in zip(bufs, offs, (Cc, Cc, 2 * nparts)):
                if a is not None:
                    want[g, off:off + 64 * wd] = a[rows].reshape(-1)
        assert np.array_equal(dtab.cpu().numpy().view(np.int32), want.view(np.int32)), "harvest: not the window's rows in window order / written outside"
        _same(dev, bufs, "harvest sources")
        dst = 2 * nW + nW - 1
        sched, dlst, dcnt = (C.c_int32 * 1)(1), _i32([dst]), _i32([1])
        rc = lib.dsg_debug_window_broadcast_f32(B, res, Cc, _p(dev[0]), _p(dev[1]), _p(dev[2]), nparts, _p(dlst), _p(dcnt), None,
                                                _p(dtab), n, stride, *offs, L.DD_TABLE, 0, 1, sched, None)
        assert rc == 0
        back = [None if a is None else a.copy() for a in bufs]
        for a, o in zip(bufs, back):
            if a is not None:
                o[2 * res * res + X.window_rows(res, nW - 1)] = a[1 * res * res + X.window_rows(res, 0)]
        _same(dev, back, "harvest -> broadcast round trip")
    assert lib.dsg_debug_window_harvest_f32(0, res, Cc, _p(dev[0]), None, None, 0, _p(dtab), stride, *offs, None) == L.DSG_ERR_INVALID
