"""CPU: the list GEMM's form rule (csrc/kernels.h: gemm_thin_rule, the function the kernel evaluates on the device-side count) through
dsg_debug_gemm_form: 2 (thin, 64-row tiles) iff the wide form's ceil(cnt / 16) x ceil(N / 96) tiles of 128 x 96 would occupy at most
half of the n_cu compute units, else 1 (wide)."""
from diffusesg_amd import lib as L


def rule(cnt, N, n_cu):
    """the rule restated: thin iff  ceil(cnt / 16) * ceil(N / 96) <= n_cu / 2  and the CU count is known"""
    wide_tiles = -(-cnt // 16) * -(-N // 96)
    return 2 if n_cu > 0 and 2 * wide_tiles <= n_cu else 1


def test_rule_over_a_grid_of_counts_widths_and_cu_counts():
    lib = L.load()
    n = 0
    for n_cu in (0, 1, 2, 8, 64, 104, 255, 256, 304):
        for N in (1, 95, 96, 97, 100, 192, 384, 768, 1536):
            for cnt in list(range(0, 70)) + [127, 128, 129, 496, 511, 512, 513, 527, 528, 1024, 2047, 2048, 2049, 8192, 32768]:
                assert lib.dsg_debug_gemm_form(cnt, N, n_cu) == rule(cnt, N, n_cu), (cnt, N, n_cu)
                n += 1
    assert n > 6000


def test_unknown_cu_count_is_never_thin():
    lib = L.load()
    for cnt in (0, 1, 16, 512, 4096):
        for N in (96, 384, 1536):
            assert lib.dsg_debug_gemm_form(cnt, N, 0) == 1
            assert lib.dsg_debug_gemm_form(cnt, N, -4) == 1


def test_headline_launches():
    """VG shape, B = 64, 30 of 64 nodes valid: the seven N = 384 list launches carry 512 runs (32 x 4 = 128 wide tiles on 256 CUs) and
    qualify; one row tile more (528 runs, 132 tiles) does not; the same 512 runs at N = 1536 (fc1's width) would not either"""
    lib = L.load()
    assert lib.dsg_debug_gemm_form(512, 384, 256) == 2
    assert lib.dsg_debug_gemm_form(513, 384, 256) == 1
    assert lib.dsg_debug_gemm_form(528, 384, 256) == 1
    assert lib.dsg_debug_gemm_form(512, 1536, 256) == 1
    assert "dsg_debug_gemm_form" in L.DEBUG_EXPORTS
