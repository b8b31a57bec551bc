"""CPU: the power of the bars tests/test_train_lp_kernels.py holds gemm_tn_bf16_kernel to (tests/train_lp_ref.py).

A NumPy emulation of the kernel -- operands rounded to bf16, fp32 sums in 16-deep steps, split-K slices, the ordered lane reduction --
stays inside every bar of every weight-gradient case, and each seeded mistake lands outside one: truncation instead of
round-to-nearest, a dropped partial last k-step, two slices overlapping by one row, the two k of a packed pair exchanged in one operand
only, and column sums taken from the rounded values."""
import pytest

import train_lp_ref as P
import train_ref as R

# the long-K cases cost seconds each in NumPy: the emulation runs all short ones and the two slice-edge cases
HOST_CASES = [(c, a) for c, a in P.tn_cases() if c.K <= 2049 or (c.K in (8705, 9217) and c.M == 96)]


def _ratios(o, got):
    ref = P.expect(o)
    c = o["case"]
    r = {"C": R.worst_ratio(got["C"], ref["C"], ref["bC"])}
    if c.colsum:
        r["cs"] = R.worst_ratio(got["cs"], ref["cs"], ref["bcs"])
    return r


@pytest.mark.parametrize("case,any_rows", HOST_CASES, ids=[c.ident() for c, _ in HOST_CASES])
def test_emulation_stays_inside_every_bar(case, any_rows):
    o = P.make(case)
    r = _ratios(o, P.emulate_tn(o))
    print(f"TLPHOST {case.ident()} " + " ".join(f"{k}={v:.3f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r


def _case(K, **kw):
    for c, _ in P.tn_cases():
        if c.K == K and all(getattr(c, k) == v for k, v in kw.items()):
            return c
    raise AssertionError(f"no weight-gradient case with K = {K} {kw}")


# the case each mistake is looked for in: where the cases were written to see it
SEEDED = [("trunc", _case(33), "C"),                       # short K: the bound is a few 1e-6 of sum |a b|, truncation moves 2^-9 of every term
          ("drop_partial_step", _case(17), "C"),           # 16 + 1 tokens: the second k-step holds one row
          ("drop_partial_step", _case(513, M=32), "C"),
          ("slice_overlap", _case(8705), "C"),             # the first row of the last slice is a spike row
          ("slice_overlap", _case(2049, M=96), "C"),
          ("pair_swap_a", _case(16), "C"),
          ("pair_swap_a", _case(33), "C"),
          ("colsum_rounded", _case(33), "cs"),
          ("colsum_rounded", _case(15), "cs")]


@pytest.mark.parametrize("mistake,case,where", SEEDED, ids=[f"{m}-{c.ident()}" for m, c, _ in SEEDED])
def test_seeded_mistake_lands_outside(mistake, case, where):
    assert mistake in P.MISTAKES
    o = P.make(case)
    good, bad = _ratios(o, P.emulate_tn(o)), _ratios(o, P.emulate_tn(o, mistake))
    print(f"TLPHOST {mistake} {case.ident()} correct {good[where]:.3f} mistaken {bad[where]:.3f}")
    assert good[where] <= 1.0 < bad[where], (good, bad)


def test_expected_routes_of_the_cases():
    """the cases are written for the routes they name"""
    for c, any_rows in P.tn_cases():
        assert P.expected_route(c, any_rows)[0] == P.ROUTE_LP_TN, c.ident()
        assert any_rows == (c.K < 512)
    for c, any_rows in P.act_cases():
        assert P.expected_route(c, any_rows) == (P.ROUTE_LP_GEMM, 1), c.ident()
    for c in P.refused_cases():
        assert P.expected_route(c, False) == (0, 0), c.ident()
