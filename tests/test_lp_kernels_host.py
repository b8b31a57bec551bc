"""CPU: the power of the checks of tests/test_lp_kernels.py (the bf16 and split-bf16 GEMMs of csrc/kernels_lp.hip against float64).
A NumPy emulation of each kernel's arithmetic (lp_ref.emulate: bf16 rounding of A' and W or the three truncated planes, fp32
accumulation in ascending 16-k steps, the six split products in the kernel's order, the epilogue op by op in fp32, the bf16 store) stays
inside every bar of every case the GPU tests run; the allowance for A' elements next to a rounding boundary reaches at most 1 % of a
case's elements; and each of twelve one-line mistakes seeded into the emulation lands outside the bar of the cases named below.  The
bit-level restatements of bf16_rne_hi and split3_bits are pinned against torch's bfloat16 cast and exact integer arithmetic."""
import numpy as np
import pytest
import torch

import lp_ref as P

CASES = P.all_cases()
BY_ID = {c.ident(): c for c in CASES}


def test_case_names_are_unique_and_cover_the_edges():
    assert len(BY_ID) == len(CASES)
    for tile in (1, 2):
        cs = [c for c in CASES if c.mode == 1 and c.tile == tile]
        assert {c.g.M for c in cs} >= set(P.BF16_M[tile]) and {c.g.N for c in cs} >= set(P.BF16_N) and {c.g.K for c in cs} >= set(P.BF16_K)
        assert {(c.g.ln != "none", c.g.act, c.g.res) for c in cs if not (c.g.epi or c.a_bf16 or c.c_bf16)} == set(P.VARIANTS)
        assert {c.g.nparts for c in cs if c.g.ln == "part"} >= {1, 2, 3, 4, 8}
        assert {(c.g.K1, c.g.K) for c in cs if c.g.K1} == {(64, 96), (64, 160), (128, 224)}
        assert {(c.g.epi, c.g.res) for c in cs if c.g.epi and not c.a_bf16} == {(e, r) for e in (1, 2, 3) for r in (False, True)}
        assert {(c.g.epi, c.g.K) for c in cs if c.a_bf16} == {(e, K) for e in (0, 1, 2, 3) for K in (64, 128)}
        assert {(c.g.ln, c.g.act) for c in cs if c.c_bf16} == {(ln, a) for ln in ("stats", "part") for a in (P.ACT_NONE, P.ACT_GELU)}
    sp = [c for c in CASES if c.mode == 2]
    assert {c.g.M for c in sp} >= set(P.SPLIT_M) and {c.g.N for c in sp} >= set(P.SPLIT_N) and {c.g.K for c in sp} >= set(P.SPLIT_K)
    assert {(c.g.ln != "none", c.g.act, c.g.res) for c in sp} >= set(P.VARIANTS)
    assert {(c.g.K1, c.g.K) for c in sp if c.g.K1} == {(32, 64), (96, 192)}


@pytest.mark.parametrize("case", CASES, ids=[c.ident() for c in CASES])
def test_emulation_is_inside_every_bar(case):
    o = P.make_lp(case)
    ref = P.lp_expect(o, case)
    assert ref["flagged"] <= P.FLAG_CAP, f"{100 * ref['flagged']:.2f} % of the A' elements carry the rounding-boundary allowance"
    r = P.ratios(o, case, ref, P.emulate(o, case))
    assert max(r.values()) <= 1.0, r


def test_span_cases_reach_the_table_clamp_and_both_ends():
    for c in CASES:
        if c.tweak == "span":
            o = P.make_lp(c)
            y = P.R.gemm_expect({**o, "case": P.replace(c.g, act=P.ACT_NONE, res=False, c2=False)})["C"]
            assert float(y.min()) < -6.0 and float(y.max()) > 6.0 and float(y.abs().min()) < 0.1


# each mistake of lp_ref.MISTAKES and the cases that must notice it
MISTAKE_CASES = {
    "split_drop_mid": ["split-M257-N192-K32-ln_none-act0-res0", "split-M257-N100-K32-ln_none-act0-res0-midheavy"],
    "split_no_midmid": ["split-M257-N100-K32-ln_none-act0-res0-midheavy", "split-M257-N192-K32-ln_none-act0-res0"],
    "a_trunc": ["bf16-t1-M256-N192-K32-ln_none-act0-res0", "bf16-t2-M300-N100-K96-ln_stats-act1-res1-c2-pad"],
    "w_trunc": ["bf16-t1-M129-N192-K160-ln_none-act0-res1", "bf16-t2-M300-N100-K64-ln_none-act0-res1-epi2-T36-off8-abf"],
    "half_chunk_full": ["bf16-t1-M256-N288-K32-ln_none-act0-res1", "bf16-t1-M300-N100-K96-ln_stats-act1-res1-c2-pad"],
    "k1_chunk_off": ["bf16-t1-M300-N100-K224-ln_none-act0-res1-K1_128", "bf16-t2-M256-N96-K96-ln_part-act0-res0-K1_64",
                     "split-M257-N100-K64-ln_none-act0-res1-K1_32"],
    "swap_row_blocks": ["bf16-t1-M129-N100-K160-ln_none-act0-res0", "bf16-t2-M300-N192-K32-ln_none-act0-res0-c2-epi3-T36-off12",
                        "split-M257-N192-K32-ln_none-act0-res0"],
    "table_no_m0": ["bf16-t1-M300-N288-K160-ln_none-act0-res1-c2-epi3-T36-off16", "bf16-t2-M300-N288-K160-ln_none-act0-res1-c2-epi3-T36-off16"],
    "stats_all_cols": ["bf16-t1-M300-N100-K96-ln_none-act0-res1-epi1-T36-off12", "bf16-t2-M300-N100-K64-ln_none-act0-res1-epi3-T36-off8-abf"],
    "mod_before_c2": ["bf16-t1-M300-N288-K160-ln_none-act0-res1-c2-epi2-T36-off12", "bf16-t2-M300-N192-K32-ln_none-act0-res0-c2-epi3-T36-off12"],
    "cbf_trunc": ["bf16-t1-M257-N100-K160-ln_stats-act1-res0-cbf", "bf16-t2-M300-N192-K192-ln_part-act0-res0-cbf"],
    "wrong_nparts": ["bf16-t1-M256-N288-K160-ln_part-act0-res0", "bf16-t2-M257-N32-K192-ln_part-act1-res1"],
}


def test_binding_struct_matches_header_layout():
    import ctypes as C
    from diffusesg_amd import lib
    assert C.sizeof(lib.DsgGemmLpArgs) == 14 * 8 + 20 * 4      # dsg_gemm_lp_args: fourteen pointers, twenty int32
    assert lib.DsgGemmLpArgs.tile_used.offset == 13 * 8 and lib.DsgGemmLpArgs.lda.offset == 14 * 8 and lib.DsgGemmLpArgs.c_bf16.offset == 14 * 8 + 19 * 4
    assert {"dsg_debug_gemm_lp", "dsg_debug_convert"} <= set(lib.DEBUG_EXPORTS)


def test_every_mistake_has_its_cases():
    assert set(MISTAKE_CASES) == set(P.MISTAKES) and len(P.MISTAKES) >= 10
    assert all(i in BY_ID for ids in MISTAKE_CASES.values() for i in ids)


@pytest.mark.parametrize("mistake,ident", [(m, i) for m, ids in MISTAKE_CASES.items() for i in ids])
def test_seeded_mistake_lands_outside(mistake, ident):
    """truncation against round-to-nearest can differ by at most one spacing, i.e. 2 x the half spacing the bar grants ("cbf_trunc": 1.9 x);
    every other mistake is outside by a factor of 2.8 (the missing mid.mid product on random operands) to 1e7"""
    case = BY_ID[ident]
    o = P.make_lp(case)
    ref = P.lp_expect(o, case)
    r = P.ratios(o, case, ref, P.emulate(o, case, mistake))
    print(f"LPMISTAKE {mistake} {ident} worst |err| / bound = {max(r.values()):.3g}")
    assert max(r.values()) > 1.5, r


# ------------------------------------------------------------------------------------------------------------------------------
# the bit-level restatements
# ------------------------------------------------------------------------------------------------------------------------------
def test_bf16_rne_restatement_matches_torch():
    for x in (P.special_values(), P.random_values()):
        mine = P.bf16_rne_bits(x)
        theirs = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(mine, theirs)
    assert P.bf16_rne_bits(np.array([0x7FC00000], np.uint32).view(np.float32))[0] == 0x7FC0      # the quiet NaN stays itself
    assert P.bf16_rne_bits(np.array([0x7FFF8000], np.uint32).view(np.float32))[0] == 0x8000      # an all-ones payload carries out: -0


def test_bf16_rne_restatement_matches_integer_arithmetic():
    """round to nearest even on the 24-bit significand, in Python integers"""
    x = np.concatenate([P.special_values()[:-7], P.random_values(20000)])
    x = x[np.isfinite(x)]
    for v, got in zip(x.view(np.uint32).tolist(), P.bf16_rne_bits(x).tolist()):
        mag, sign = v & 0x7FFFFFFF, v >> 31
        q, rem = mag >> 16, mag & 0xFFFF
        q += 1 if (rem > 0x8000 or (rem == 0x8000 and (q & 1))) else 0      # the carry may run into the exponent: that IS the next binade / inf
        assert got == (sign << 15) | q, hex(v)


def test_split3_restatement_is_an_exact_truncating_split():
    x = np.concatenate([P.special_values(), P.random_values()])
    x = x[np.isfinite(x)]
    h, m, lo = P.split3(x)
    tot, big = h.astype(np.float64) + m.astype(np.float64) + lo.astype(np.float64), (np.abs(x) >= 2.0 ** -110) | (x == 0)
    assert np.array_equal(tot[big], x.astype(np.float64)[big])
    assert (np.abs(tot - x)[~big] < 2.0 ** -133).all()      # a bf16 denormal ends at 2^-133: lower bits of such a lo (or mid) plane are cut
    assert np.array_equal(P.split3_bits(x)[0], (x.view(np.uint32) >> 16).astype(np.uint16))      # hi is the upper half: truncation
    # each plane holds the next 8 bits of the significand: |mid| < spacing(hi), |lo| < 2^-8 spacing(hi) (normal numbers)
    nrm = np.abs(x) >= 2.0 ** -100
    s = P.bf16_spacing(x.astype(np.float64))
    assert (np.abs(m.astype(np.float64))[nrm] < s[nrm]).all() and (np.abs(lo.astype(np.float64))[nrm] < s[nrm] * 2.0 ** -8).all()
    assert ((m == 0) | (np.sign(m) == np.sign(x))).all() and ((lo == 0) | (np.sign(lo) == np.sign(x))).all()      # the terms share a's sign
    # integer arithmetic on one value: 1 + 2^-8 + 2^-23 -> hi 1, mid 2^-8, lo 2^-23
    one = np.array([0x3F808001], np.uint32).view(np.float32)
    assert [float(p[0]) for p in P.split3(one)] == [1.0, 2.0 ** -8, 2.0 ** -23]


def test_boundary_distance_and_spacing():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7, 2.0 - 2.0 ** -8, 0.75, 0.0])
    assert np.array_equal(P.bf16_spacing(x), np.array([2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 2.0 ** -8, 0.0]))
    d = P.boundary_distance(x)
    assert d[0] == 2.0 ** -8 and d[1] == 0.0 and d[2] == 2.0 ** -8 and d[3] == 0.0 and np.isinf(d[5])
