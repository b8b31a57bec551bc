"""CPU: the power of tests/test_bx_forms.py's checks, on tests/bx_ref.py alone.  The case lists are well formed and reach every
gemm_bx_kernel instantiation and every fused-MLP kernel x MOD x proj the launchers can select; the launchers' decisions (geometry,
kernel, refusal) restated in Python agree with the cases' table; a NumPy emulation of the kernels' arithmetic (fp32 accumulation in
ascending k chunks, bf16 roundings where the kernels have them, LayerNorm from lane-local sum / sum-of-squares) sits inside every bar of
every case through the very check functions the GPU file calls; the exact cases meet their two conditions; and each seeded mistake lands
outside at least one case's bar.  Which case catches which mistake is printed (profiles/bx_kernel_errors.md lists them)."""
import numpy as np
import pytest
import torch

import bx_ref as B
from diffusesg_amd import lib

GEMM = B.gemm_cases()
PERSIST = B.persistence_cases(B.HOST_CUS)
DENSE, EXACT = B.mlp_dense_cases(), B.mlp_exact_cases()


def test_gemm_case_list_is_well_formed():
    ids = [c.ident() for c in GEMM + PERSIST]
    assert len(set(ids)) == len(ids)
    # every <geometry, RES, MOD> instantiation of launch_gemm_bx
    assert {c.instance for c in GEMM} == {(g, r, m) for g in (0, 2, 3) for r in (False, True) for m in (0, 1, 2)}
    for geo in (0, 2, 3):
        mine = [c for c in GEMM if c.geo == geo]
        fams = {c.fam for c in mine}
        for fam in fams - {"lnfree", "plain", "fc2w", "pre", "mergec"}:     # every epilogue family at every M edge of the geometry
            assert set(B.geo_M(geo)) <= {c.M for c in mine if c.fam == fam}, (geo, fam)
        assert set(B.GEO_K[geo]) | {1536} <= {c.K for c in mine}
        wide = set(B.GEO_N[geo]["wide"]) | set(B.GEO_N[geo]["ln"])
        assert wide <= {c.N for c in mine}
        assert any(c.fam == "lnfree" for c in mine) and any(c.pad for c in mine)
        # MOD 2 with 36-row samples at M = 324 and with one sample; both offsets for MOD 1 and MOD 2
        for mod in (1, 2):
            assert {0, 1} == {int(c.mod_off > 0) for c in mine if c.mod == mod}
        assert any(c.mod == 2 and c.M == 324 and c.mod_T == 36 for c in mine) and any(c.mod == 2 and c.mod_T == 0 for c in mine)
    # Cb without LayerNorm next to C2b (the direct 8-byte store), MOD 0 / 1 / 2, on both geometries that have the form
    assert {(c.geo, c.mod) for c in GEMM if c.cb and c.c2b and c.c and not c.ln} >= {(0, 0), (0, 1), (0, 2), (2, 0), (2, 2)}
    assert any(c.N == 100 and not (c.cb or c.c2b) for c in GEMM) and any(c.N == 768 and c.mod and not c.ln for c in GEMM)
    assert {(c.K1, c.K) for c in GEMM if c.K1 and c.geo == 0} >= {(64, 128), (64, 192), (128, 192)}
    assert {(c.K1, c.K) for c in GEMM if c.K1 and c.geo == 2} >= {(32, 96), (64, 96)}
    for c in GEMM + PERSIST:
        p = B.gemm_pitches(c)
        assert p["lda"] % 8 == 0 and p["lda2"] % 8 == 0 and p["ldc"] % 4 == 0 and p["ldres"] % 4 == 0 and c.mod_off % 4 == 0
        assert p["ldc"] > c.N and (not (c.cb or c.c2b) or (p["ldcb"] > c.N and p["ldc2b"] > c.N and p["ldcb"] % 8 == 0 and p["ldc2b"] % 8 == 0))
        assert not c.alias or (c.res and c.c and p["ldres"] == p["ldc"])
        if c.pad:
            assert p["lda"] > (c.K1 or c.K) and (c.alias or p["ldres"] != p["ldc"]) and p["ldcb"] != p["ldc2b"]
        if c.K1:
            assert p["lda2"] != p["lda"]
        if c not in PERSIST:
            assert c.M <= 17 * 256 + 3


def test_persistence_cases_take_a_second_tile():
    for n_cu in (B.HOST_CUS, 304, 64, 8):
        for c in B.persistence_cases(n_cu):
            bm, bn, kb = B.GEO[c.geo]
            tm, tn = (c.M + bm - 1) // bm, (c.N + bn - 1) // bn
            grid = B.persistence_grid(c.geo, n_cu)
            assert tm % 8 == 1 and (tm + 7) // 8 * 8 * tn > grid and c.K == 2 * kb
            assert (tm - 8 + 7) // 8 * 8 * tn <= grid, "not the smallest such M"
    assert [c.M for c in PERSIST] == [8193, 43009, 32769]
    assert B.mlp96r_round2_case(B.HOST_CUS).M == 65569 and (65569 + 31) // 32 > 8 * B.HOST_CUS


def _rule(c):
    p = B.gemm_pitches(c)
    return B.gemm_rule(c.N, c.K, p["lda"], c.act, c.res, c.cb, c.c2b, c.ln, c.K1, p["lda2"], p["ldcb"], p["ldc2b"], c.M)


def test_launcher_decisions_agree_with_the_table():
    for c in GEMM + PERSIST:
        assert _rule(c) == c.geo, c.ident()
    for name, ok, bad in B.REFUSALS:
        a, b = B.refusal_args(ok), B.refusal_args(bad)
        assert B.gemm_rule(**a) >= 0, name
        assert B.gemm_rule(**b) == -1, name
    for c in DENSE + EXACT + [B.mlp96r_round2_case(B.HOST_CUS)]:
        assert B.mlp_rule(c) == B.MLP_KERNELS[c.kern][2], c.ident()
    # the selectors the two hooks refuse
    for kern, proj, mod in (("mlp384w", True, 0), ("mlp96r", True, 1), ("mlp96r", False, 0)):
        assert B.mlp_rule(B.MlpCase(kern, proj, 8, mod=mod)) is None
    assert {"dsg_debug_gemm_bx_args", "dsg_debug_mlp_bx_args"} <= set(lib.DEBUG_EXPORTS)


def test_mlp_case_lists_are_well_formed():
    ids = [c.ident() for c in DENSE + EXACT]
    assert len(set(ids)) == len(ids)
    for kern, proj in B.MLP_COMBOS:
        mods = (0, 1, 2) if B.MLP_KERNELS[kern][3] else (0,)
        d = [c for c in DENSE if (c.kern, c.proj) == (kern, proj)]
        e = [c for c in EXACT if (c.kern, c.proj) == (kern, proj)]
        assert set(B.MLP_M) <= {c.M for c in d}
        assert {c.mod for c in d} == set(mods) == {c.mod for c in e if c.M == 129}
        assert {c.out_mode for c in d} == {0, 1, 2}
        if len(mods) == 3:
            assert {0, 1} == {int(c.mod_off > 0) for c in d if c.mod}
            assert any(c.M == 324 and c.mod == 2 and c.mod_T == 36 for c in d) and any(c.M == 324 and c.mod == 2 and c.mod_T == 36 for c in e)
        for c in d + e:
            assert c.mod_off % 4 == 0 and c.mod_off in (0, 2 * c.C + 8)
    assert {(c.kern, c.proj) for c in DENSE} == set(B.MLP_COMBOS) and len(B.MLP_COMBOS) == 12


FAMS = sorted({c.fam for c in GEMM})


@pytest.mark.parametrize("fam", FAMS)
def test_emulation_sits_inside_every_gemm_bar(fam):
    worst = {}
    for c in [c for c in GEMM if c.fam == fam]:
        o = B.make_gemm(c)
        r = B.check_gemm(o, B.gemm_expect(o), B.gemm_buffers(o), B.emulate_gemm(o))
        assert max(r.values()) <= 1.0, (c.ident(), r)
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"BXHOST gemm {fam}: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


@pytest.mark.parametrize("kern,proj", B.MLP_COMBOS, ids=[f"{k}-{'proj' if p else 'mlp'}" for k, p in B.MLP_COMBOS])
def test_emulation_sits_inside_every_mlp_bar_and_exact_cases_meet_their_conditions(kern, proj):
    worst = {}
    for c in [c for c in DENSE + EXACT if (c.kern, c.proj) == (kern, proj)]:
        o = B.make_mlp(c)
        ref = B.mlp_expect(o)
        if c.exact:
            print(f"BXHOST exact {c.ident()}: flagged LN-2 {ref['flag_ln']:.3f}, hidden {ref['flag_h']:.3f}; bar < {B.TIGHT:g} scale on "
                  f"{ref['tight']:.3f} of the outputs; median bar {float(ref['bar'].median()):.2e} at scale {ref['scale']:.1f}")
            assert ref["flag_ln"] <= B.FLAG_CAP and ref["flag_h"] <= B.FLAG_CAP, c.ident()
            assert ref["tight"] >= 0.5, c.ident()
        r = B.check_mlp(o, ref, B.mlp_buffers(o), B.emulate_mlp(o))
        assert max(r.values()) <= 1.0, (c.ident(), r)
        for k, v in r.items():
            key = ("exact " if c.exact else "dense ") + k
            worst[key] = max(worst.get(key, 0.0), v)
    print(f"BXHOST mlp {kern} proj={int(proj)}: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


def _gemm_shortlist():
    return [c for c in GEMM if 64 <= c.M <= 400]


@pytest.mark.parametrize("mistake", B.GEMM_MISTAKES)
def test_seeded_gemm_mistake_lands_outside_a_bar(mistake):
    for c in _gemm_shortlist():
        o = B.make_gemm(c)
        got, good = B.emulate_gemm(o, mistake), B.emulate_gemm(o)
        if all(got[k] is None or np.array_equal(got[k], good[k]) for k in got):
            continue      # the mistake does not bear on this form
        r = B.check_gemm(o, B.gemm_expect(o), B.gemm_buffers(o), got)
        bad = {k: v for k, v in r.items() if v > 1.0}
        if bad:
            k = max(bad, key=bad.get)
            print(f"BXHOST mistake {mistake}: caught by {c.ident()} ({k}: {bad[k]:.3g} x the bar)")
            return
    pytest.fail(f"no case catches {mistake}")


@pytest.mark.parametrize("mistake", B.MLP_MISTAKES)
def test_seeded_mlp_mistake_lands_outside_a_bar(mistake):
    short = [c for c in EXACT if c.kern == "mlp96"] + [c for c in DENSE if c.kern == "mlp96" and c.M >= 127]
    for c in short:
        o = B.make_mlp(c)
        got, good = B.emulate_mlp(o, mistake), B.emulate_mlp(o)
        if all(got[k] is None or np.array_equal(got[k], good[k]) for k in got):
            continue
        r = B.check_mlp(o, B.mlp_expect(o), B.mlp_buffers(o), got)
        bad = {k: v for k, v in r.items() if v > 1.0}
        if bad:
            k = max(bad, key=bad.get)
            print(f"BXHOST mistake {mistake}: caught by {c.ident()} ({k}: {bad[k]:.3g} x the bar)")
            return
    pytest.fail(f"no case catches {mistake}")


def test_truncation_of_the_hidden_tensor_is_far_outside_the_exact_bars():
    """the point of the exact operands: the dense bars (5e-4 of the scale) cannot see a truncated hidden tensor, the derived ones can"""
    c = next(c for c in EXACT if c.kern == "mlp384d" and not c.proj and c.mod == 0)
    o = B.make_mlp(c)
    ref = B.mlp_expect(o)
    got = B.emulate_mlp(o, "hid_trunc")["x"][:c.M].view(np.float32)
    ratio = ((torch.from_numpy(got.copy()).double() - ref["x"]).abs() / ref["bar"]).median()
    print(f"BXHOST hid_trunc on {c.ident()}: median |err| / bar = {float(ratio):.0f}")
    assert ratio > 20
    d = next(c for c in DENSE if c.kern == "mlp384d" and not c.proj and c.M == 129)
    od = B.make_mlp(d)
    rd = B.check_mlp(od, B.mlp_expect(od), B.mlp_buffers(od), B.emulate_mlp(od, "hid_trunc"))
    print(f"BXHOST hid_trunc on {d.ident()} (dense bar): {rd['x']:.3f} x the bar")
