"""CPU: the C-ABI library loads and exports every symbol include/dsg.h and include/dsg_debug.h declare; the host-only schedule helper
matches the reference's sigma tables; the state-dict layout matches the golden generator's check."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from diffusesg_amd import lib, spec
from diffusesg_amd import synth as Y
from util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    return set(re.findall(r"\b(dsg_[a-z_0-9]+)\s*\(", hdr)) - {"dsg_handle_s"}


def _is_bench(name):
    return name.startswith(("dsg_debug_", "dsg_profile_"))


def test_header_symbols_exported():
    """each header against its own list, both ways; the product header declares no test or measurement hook, the test-bench header
    nothing else; the library exports all of both"""
    product, bench = _declared("dsg.h"), _declared("dsg_debug.h")
    assert product == set(lib.EXPORTS), product ^ set(lib.EXPORTS)
    assert bench == set(lib.DEBUG_EXPORTS), bench ^ set(lib.DEBUG_EXPORTS)
    assert len(set(lib.EXPORTS)) == len(lib.EXPORTS) and len(set(lib.DEBUG_EXPORTS)) == len(lib.DEBUG_EXPORTS)
    assert not [n for n in product if _is_bench(n)]
    assert not [n for n in bench if not _is_bench(n)]
    hdr = open(os.path.join(ROOT, "include", "dsg.h")).read()
    assert "dsg_debug_" not in hdr and "dsg_profile_" not in hdr and not re.search(r"#\s*include\s*\"dsg_debug\.h\"", hdr)
    L = lib.load()
    for name in product | bench:
        assert hasattr(L, name), f"libdsg.so does not export {name}"
    assert b"gfx950" in L.dsg_version()
    assert L.dsg_abi_version() == lib.ABI_VERSION == int(re.search(r"#define DSG_ABI_VERSION (\d+)", hdr).group(1)) == 5


@pytest.mark.parametrize("lang", ["c", "c++"])
@pytest.mark.parametrize("includes", [("dsg.h",), ("dsg_debug.h",), ("dsg.h", "dsg_debug.h")])
def test_headers_compile_on_their_own(lang, includes, tmp_path):
    """each public header is self-contained C and C++: the host compiler's syntax pass over a file that only includes it
    (dsg_debug.h with and without dsg.h in front)"""
    names = ("gcc", "cc", "clang", "/opt/rocm/lib/llvm/bin/clang") if lang == "c" else ("g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++")
    cc = next((shutil.which(n) for n in names if shutil.which(n)), None)
    assert cc, "no host compiler"
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text("".join(f'#include "{h}"\n' for h in includes))
    r = subprocess.run([cc, "-x", lang, "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_bx_kernel_selectors_are_checked():
    """a kernel name a bf16-pipeline hook cannot honour for the shape is DSG_ERR_INVALID, not ignored: the check runs ahead of any
    device call, so no GPU is needed (the operand pointers are never read)"""
    L = lib.load()
    buf = (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p)
    mlp = lambda Cc, mod, k: L.dsg_debug_mlp_bx(8, Cc, p, p, p, p, p, p, p if mod else None, 0, None, k, 0, None, None)
    proj = lambda Cc, mod, k: L.dsg_debug_projmlp_bx(8, Cc, p, p, p, p, p, p, p, p, p if mod else None, 0, None, k, 0, None, None)
    qa = lambda ws, k: L.dsg_debug_qkv_attn_bx(1, 2 * ws, ws, 0, 3, p, p, p, p, p, k, 0, None, None)
    bad = lib.DSG_ERR_INVALID
    for k in (lib.BXK_MLP384_DMA, lib.BXK_MLP384_WAVE, lib.BXK_MLP384_R3, lib.BXK_MLP384_SOLO):
        assert mlp(96, 0, k) == bad and mlp(192, 1, k) == bad and proj(96, 0, k) == bad
    assert proj(384, 0, lib.BXK_MLP384_WAVE) == bad                     # the proj form has no one-wave-per-SIMD kernel
    for k in (lib.BXK_MLP96_STAGED, lib.BXK_MLP96_RESIDENT, lib.BXK_QA10_WAVE, lib.BXK_QA10_HEAD, 9, -1):
        assert mlp(96, 0, k) == bad and mlp(384, 0, k) == bad           # not kernels of the plain MLP hook
    for k in (lib.BXK_MLP96_STAGED, lib.BXK_MLP96_RESIDENT):
        assert proj(192, 0, k) == bad and proj(384, 0, k) == bad
    assert proj(96, 1, lib.BXK_MLP96_RESIDENT) == bad                   # the LDS-resident kernel has no modulate
    for k in (lib.BXK_QA10_WAVE, lib.BXK_QA10_HEAD):
        assert qa(8, k) == bad and qa(4, k) == bad
    assert qa(10, lib.BXK_MLP384_DMA) == bad and qa(10, 9) == bad and proj(96, 0, 9) == bad


@pytest.mark.parametrize("T", [50, 100, 256, 1000])
def test_sigma_schedule_matches_reference(T):
    g = load("sampler.npz")
    sg, th, nz, hs = lib.sigma_schedule(lib.make_sampler_cfg(T))
    np.testing.assert_allclose(sg, g[f"sigma_steps_{T}"], rtol=1e-14, atol=0)
    t = sg.astype(np.float32)
    # churn only inside [S_min, S_max]; never when it is off (a fused multiply-add would leave a residue here)
    off = (t < np.float32(0.05)) | (t > np.float32(50))
    assert np.all(nz[off] == 0) and np.all(th[off] == t[off])
    assert np.all(nz[~off] > 0)
    _, th0, nz0, _ = lib.sigma_schedule(lib.make_sampler_cfg(T, S_churn=0.0))
    assert np.all(nz0 == 0) and np.array_equal(th0, t)
    assert hs[-1] == -th[-1]   # t_N = 0 (edm.py:319)


def test_structs_match_header_layout():
    assert C.sizeof(lib.DsgConfig) == 4 * (5 + 8 + 8 + 3)
    assert C.sizeof(lib.DsgSamplerCfg) == 56
    assert C.sizeof(lib.DsgSampleStats) == 24
    assert C.sizeof(lib.DsgGemmF32Args) == 13 * 8 + 16 * 4      # dsg_gemm_f32_args: thirteen pointers, sixteen int32
    assert lib.DsgGemmF32Args.lda.offset == 13 * 8 and lib.DsgGemmF32Args.reserved.offset == 13 * 8 + 15 * 4
    assert C.sizeof(lib.DsgGemmLpArgs) == 14 * 8 + 20 * 4       # dsg_gemm_lp_args: fourteen pointers (tile_used last), twenty int32
    assert lib.DsgGemmLpArgs.tile_used.offset == 13 * 8 and lib.DsgGemmLpArgs.lda.offset == 14 * 8
    assert lib.DsgGemmLpArgs.mode.offset == 14 * 8 + 16 * 4 and lib.DsgGemmLpArgs.c_bf16.offset == 14 * 8 + 19 * 4
    assert C.sizeof(lib.DsgTProb) == 4 * 8 + 6 * 4              # dsg_t_prob: four pointers, six int32
    assert lib.DsgTProb.C.offset == 3 * 8 and lib.DsgTProb.lda.offset == 4 * 8 and lib.DsgTProb.K.offset == 4 * 8 + 5 * 4


def test_param_counts_and_flops():
    assert spec.num_parameters(spec.vg_config()) == 35_813_660      # SURVEY §6 (measured from the reference)
    assert spec.num_parameters(spec.coco_config()) == 30_693_965
    assert spec.num_parameters(spec.tiny_config()) == 2_402_756
    assert abs(spec.flops_per_forward(spec.vg_config()) / 13.30e9 - 1) < 0.01
    assert abs(spec.flops_per_forward(spec.coco_config()) / 7.36e9 - 1) < 0.01


def test_channel_table():
    vg, coco = spec.sg_channels("visual_genome", "bits"), spec.sg_channels("coco_stuff", "bits")
    assert (vg["c_adj"], vg["c_node"], vg["in_chans"]) == (6, 12, 30)
    assert (coco["c_adj"], coco["c_node"], coco["in_chans"]) == (3, 12, 27)
    d = spec.sg_channels("visual_genome", "ddpm")
    assert (d["c_adj"], d["c_node"], d["in_chans"]) == (1, 5, 11)
    o = spec.sg_channels("visual_genome", "one_hot")
    assert (o["c_adj"], o["c_node"], o["in_chans"]) == (51, 154, 359)


def test_module_state_dict_keys_match_spec():
    from diffusesg_amd.model import build_network
    for name in ("tiny", "small", "vg"):
        cfg = Y.CONFIGS[name]()
        m = build_network(cfg, device="cpu")
        keys = set(m.state_dict().keys())
        assert keys == {"model." + t.key for t in spec.state_dict_spec(cfg)}
    assert len(build_network(spec.vg_config(), device="cpu").state_dict()) == 247


def test_no_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from diffusesg_amd.model import build_network
    from diffusesg_amd import weights as W
    cfg = spec.tiny_config()
    net = build_network(cfg, W.synth_state_dict(cfg, 0), device="cpu")
    flags, adj, node, _, _ = Y.case_inputs(cfg, 2, [8, 5], 1, "x")
    with pytest.raises(lib.DsgError):
        net.model(torch.from_numpy(adj), torch.from_numpy(node), torch.from_numpy(flags), torch.zeros(2))


def test_gelu_table_accuracy():
    """numpy restatement of the table-driven GELU of csrc/kernels.hip (gelu_lut): nodes every 1/64 on [-6,6] holding
    (Phi, phi, -x*phi/2), second-order Taylor from the nearest node.  Max abs error vs an fp64 exact-erf GELU."""
    from scipy.special import erfc
    xs = np.linspace(-6.0, 6.0, 769)
    phi = np.exp(-0.5 * xs * xs) / np.sqrt(2 * np.pi)
    tab = np.stack([0.5 * erfc(-xs / np.sqrt(2)), phi, -0.5 * xs * phi], 1).astype(np.float32)
    x = np.concatenate([np.linspace(-9, 9, 400001), np.random.RandomState(0).randn(200000) * 2]).astype(np.float32)
    t = np.clip(x + np.float32(6), np.float32(0), np.float32(12)).astype(np.float32)
    r = np.rint(t * np.float32(64)).astype(np.float32)
    d = (r * np.float32(-0.015625) + t).astype(np.float32)
    c = tab[r.astype(np.int64)]
    g = (x * (d * (d * c[:, 2] + c[:, 1]) + c[:, 0])).astype(np.float32)
    ref = 0.5 * x.astype(np.float64) * erfc(-x.astype(np.float64) / np.sqrt(2))
    assert np.abs(g - ref).max() < 6e-7      # same level as an fp32 evaluation of the erf formula (4.5e-7)
