"""CPU: in-loop box guidance (dsg_sample_guided) without a device -- the new symbols, dsg_guide_coef against float64, the refusals that
need no device, the NumPy float64 restatement of the three box losses and their gradients (tests/box_guide_ref.py) against torch
float64 autograd of guide.py's closures, and a power check: five plausible mistakes each move the gradient or the guided estimate
beyond the loosest bar the GPU tests (tests/test_box_guide.py) use."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import box_guide_ref as BR
from diffusesg_amd import guide as G
from diffusesg_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dsg_guide_coef", "dsg_sample_guided", "dsg_debug_box_guide")
LOOSEST_BAR = 1e-4   # the T = 8 trajectory bar; the kernel and the loop-arithmetic bars (about 1e-6) are tighter


def test_new_symbols_declared_exported_loadable():
    hdr = open(os.path.join(ROOT, "include", "dsg.h")).read()
    bench_hdr = open(os.path.join(ROOT, "include", "dsg_debug.h")).read()
    L = lib.load()
    for name in NEW:
        bench = name.startswith("dsg_debug_")   # the kernel's own hook is declared with the test bench
        assert name + "(" in (bench_hdr if bench else hdr) and name in (lib.DEBUG_EXPORTS if bench else lib.EXPORTS)
        getattr(L, name)
    assert "typedef struct dsg_guide_cfg" in hdr and "DSG_GUIDE_CLIP_NONE" in hdr
    assert int(L.dsg_abi_version()) == lib.ABI_VERSION
    assert C.sizeof(lib.DsgGuideCfg) == 48   # five floats, one int32, three pointers: no padding


def _scfg(T, solver="euler", churn=0.0):
    return lib.make_sampler_cfg(T, solver, churn, 0.05, 50.0, 1.003, 0.002, 80.0, 7.0, True)


@pytest.mark.parametrize("T,churn", [(1, 0.0), (8, 0.0), (8, 40.0), (256, 40.0)])
def test_guide_coef_against_float64(T, churn):
    scfg = _scfg(T, "heun", churn)
    t_hat = lib.sigma_schedule(scfg)[1]
    w = np.random.default_rng(T).standard_normal(T).astype(np.float32) * 3
    w[0] = 0.0
    got = lib.guide_coef(scfg, w)
    ref = BR.coef(w, t_hat)
    assert got.dtype == np.float32 and got.shape == (T,)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    assert (np.abs(got.astype(np.float64) - ref) <= 2 * ulp).all(), np.abs(got - ref) / ulp
    assert got[0] == 0.0


def test_guide_coef_refusals():
    L, scfg = lib.load(), _scfg(8)
    out = np.empty(8, np.float32)
    ok = np.ones(8, np.float32)
    for bad in (np.nan, np.inf, -np.inf):
        w = ok.copy()
        w[3] = bad
        assert L.dsg_guide_coef(C.byref(scfg), w.ctypes.data, out.ctypes.data, 8) == lib.DSG_ERR_INVALID
        with pytest.raises(lib.DsgError):
            lib.guide_coef(scfg, w)
    assert L.dsg_guide_coef(C.byref(scfg), ok.ctypes.data, out.ctypes.data, 7) == lib.DSG_ERR_INVALID
    assert L.dsg_guide_coef(C.byref(scfg), None, out.ctypes.data, 8) == lib.DSG_ERR_INVALID
    assert L.dsg_guide_coef(None, ok.ctypes.data, out.ctypes.data, 8) == lib.DSG_ERR_INVALID
    with pytest.raises(lib.DsgError):
        lib.guide_coef(scfg, np.ones(5, np.float32))
    assert L.dsg_guide_coef(C.byref(scfg), ok.ctypes.data, out.ctypes.data, 8) == 8


def _cfg(o=1.0, r=0.0, a=0.0, tau=0.05, clip=1.0, sel=None, region=None):
    return lib.DsgGuideCfg(o, r, a, tau, clip, 0, sel, region, None)


@pytest.mark.parametrize("what,c_node,cfg,word", [
    ("C_node < 4", 3, _cfg(), "C_node"),
    ("tau <= 0 with the alignment loss", 4, _cfg(a=1.0, tau=0.0), "tau"),
    ("negative tau with the alignment loss", 4, _cfg(a=1.0, tau=-0.05), "tau"),
    ("region weight without sel / region", 4, _cfg(r=1.0), "sel"),
    ("region weight without region", 4, _cfg(r=1.0, sel=64), "region"),
    ("NaN loss weight", 4, _cfg(o=float("nan")), "w_overlap"),
    ("infinite loss weight", 4, _cfg(a=float("inf")), "w_align"),
    ("negative clip_ratio", 4, _cfg(clip=-0.5), "clip_ratio"),
    ("NaN clip_ratio", 4, _cfg(clip=float("nan")), "clip_ratio"),
])
def test_kernel_entry_refuses_before_any_launch(what, c_node, cfg, word):
    """every pointer is NULL: a call that got past its argument checks would fail differently (or crash); the refusal names the argument"""
    L = lib.load()
    rc = L.dsg_debug_box_guide(3, 8, 2, c_node, None, None, None, None, None, None, C.byref(cfg), 1.0, None, None, None, None, None, None, None)
    assert rc == lib.DSG_ERR_INVALID, what
    assert word in L.dsg_last_error(None).decode(), (what, L.dsg_last_error(None))
    assert L.dsg_debug_box_guide(3, 8, 2, 4, None, None, None, None, None, None, None, 1.0, None, None, None, None, None, None, None) == lib.DSG_ERR_INVALID
    assert L.dsg_debug_box_guide(3, 65, 2, 4, None, None, None, None, None, None, C.byref(_cfg()), 1.0, None, None, None, None, None, None, None) == lib.DSG_ERR_INVALID


def test_python_surface_refusals():
    with pytest.raises(ValueError):
        G.BoxGuide(align=1.0, tau=0.0)
    with pytest.raises(ValueError):
        G.BoxGuide(overlap=float("nan"))
    with pytest.raises(ValueError):
        G.BoxGuide(region=(0, (0.5, 0.1, 0.2, 0.9)))        # empty rectangle
    with pytest.raises(ValueError):
        G.BoxGuide(region=(torch.zeros(3, 8), torch.zeros(3, 8, 4))).region_tensors(3, 16)
    with pytest.raises(ValueError):
        G.BoxGuide(region=(9, (0.1, 0.1, 0.9, 0.9))).region_tensors(3, 8)
    g, keep = G.BoxGuide(overlap=2.0, region=([1, 2], (0.1, 0.2, 0.8, 0.9)), align=0.5, tau=0.1).descriptor(3, 8, "cpu", None)
    assert (g.w_overlap, g.w_region, g.w_align) == (2.0, 1.0, 0.5) and g.clip_ratio == lib.GUIDE_CLIP_NONE
    assert keep[0].tolist() == [[0, 1, 1, 0, 0, 0, 0, 0]] * 3 and np.allclose(keep[1][:, 1].numpy(), [0.1, 0.2, 0.8, 0.9])
    from diffusesg_amd.sampler import NodeAdjEDMSamplerHip
    with pytest.raises(ValueError):
        NodeAdjEDMSamplerHip(num_steps=8, solver="dpmpp_2m", S_churn=40)   # the multistep solver with churn: refused as ever


# ---- the float64 restatement against torch float64 autograd of guide.py's closures ----
def case(N, c_node, valid, seed, special=True):
    """D_node [B, N, c_node] float64 (finite everywhere), flags, sel, region: random boxes plus, where the graph has the nodes, two
    identical boxes (ties), two touching boxes and a box of negative extent"""
    rng = np.random.default_rng(seed)
    B = len(valid)
    D = rng.uniform(-1.0, 1.0, (B, N, c_node))
    D[..., -2:] = rng.uniform(-0.9, 0.2, (B, N, 2))   # extents 0.05 .. 0.6: plenty of overlaps
    flags = np.zeros((B, N), np.uint8)
    for b, v in enumerate(valid):
        flags[b, :v] = 1
        if special and v >= 2 and b % 3 == 0:
            D[b, 1, -4:] = D[b, 0, -4:]                                   # identical: every min / max of the pair is a tie
        if special and v >= 2 and b % 3 == 1:
            D[b, 0, -4:] = [-0.5, 0.0, -0.5, 0.0]                         # [0.125, 0.375] x [0.25, 0.75]
            D[b, 1, -4:] = [0.0, 0.0, -0.5, 0.0]                          # [0.375, 0.625] x ...: touching, relu's argument is 0
        if special and v >= 3:
            D[b, 2, -2] = -1.2                                            # width -0.1
    sel = (rng.random((B, N)) < 0.6).astype(np.uint8)
    lo = rng.uniform(0.0, 0.5, (B, N, 2))
    region = np.concatenate([lo, lo + rng.uniform(0.1, 0.4, (B, N, 2))], -1).astype(np.float32).astype(np.float64)   # the library takes float32
    return D, flags, sel, region


LOSSES = {"overlap": dict(a_o=1.3), "region": dict(a_r=0.7), "align": dict(a_a=0.9, tau=0.05), "all": dict(a_o=1.3, a_r=0.7, a_a=0.9, tau=0.05)}


def box_guide_of(kw, sel, region):
    return G.BoxGuide(overlap=kw.get("a_o", 0.0), align=kw.get("a_a", 0.0), tau=kw.get("tau", 0.05), region_weight=kw.get("a_r", 0.0),
                      region=(torch.from_numpy(sel), torch.from_numpy(region)) if kw.get("a_r", 0.0) else None)


def torch_loss_grad(D, flags, sel, region, kw, dtype):
    """per-graph loss and dL/dD at the box channels by torch autograd of BoxGuide.torch_loss, graph by graph"""
    B = D.shape[0]
    L, g = np.zeros(B), np.zeros(D.shape[:2] + (4,))
    for b in range(B):
        fl = torch.from_numpy(flags[b:b + 1])
        x = torch.tensor(D[b:b + 1], dtype=dtype, requires_grad=True)
        val = box_guide_of(kw, sel[b:b + 1], region[b:b + 1]).torch_loss(fl)(None, x)
        gx, = torch.autograd.grad(val, x, allow_unused=True)
        L[b] = float(val.detach())
        g[b] = 0.0 if gx is None else gx[0, :, -4:].double().numpy()
        assert gx is None or float(gx[0, :, :-4].abs().sum()) == 0.0
    return L, g


@pytest.mark.parametrize("which", sorted(LOSSES))
@pytest.mark.parametrize("N,c_node,valid", [(1, 4, [1, 0, 1]), (2, 5, [2, 2, 1]), (8, 12, [8, 5, 3]), (40, 4, [40, 2, 0]), (64, 5, [64, 33, 1])])
def test_restatement_against_torch_float64(which, N, c_node, valid):
    D, flags, sel, region = case(N, c_node, valid, seed=N)
    kw = LOSSES[which]
    L, g = BR.loss_grad(D, flags, sel=sel, region=region, **kw)
    Lt, gt = torch_loss_grad(D, flags, sel, region, kw, torch.float64)
    assert np.abs(L - Lt).max() <= 1e-12 * max(1.0, np.abs(Lt).max())
    assert np.abs(g - gt).max() <= 1e-12 * max(1.0, np.abs(gt).max())
    assert (g[flags == 0] == 0).all()
    if N >= 8:
        assert np.abs(g).max() > 0


def test_restatement_ignores_padded_rows():
    D, flags, sel, region = case(8, 5, [8, 5, 3], seed=3)
    Dn = D.copy()
    Dn[flags == 0] = np.nan
    for kw in LOSSES.values():
        a, b = BR.loss_grad(D, flags, sel=sel, region=region, **kw), BR.loss_grad(Dn, flags, sel=sel, region=region, **kw)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_region_index_form_is_box_region_loss():
    D, flags, _, _ = case(8, 5, [8, 5, 3], seed=5)
    x = torch.tensor(D, requires_grad=True)
    fl = torch.from_numpy(flags)
    rect = (0.2, 0.3, 0.6, 0.7)
    a = G.BoxGuide(region=([1, 4], rect)).torch_loss(fl)(None, x)
    b = G.box_region_loss([1, 4], rect, fl)(None, x)
    a, b = a.detach(), b.detach()
    assert float(a) == float(b) and float(a) > 0
    sel, rc = G.BoxGuide(region=([1, 4], rect)).region_tensors(3, 8)
    L, _ = BR.loss_grad(D, flags, sel=sel.numpy(), region=rc.numpy().astype(np.float64), a_r=1.0)
    assert abs(L.sum() - float(a)) <= 1e-6 * float(a)   # the rectangle went through float32


# ---- power: what the bars can see ----
def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_mistakes_move_the_result_beyond_the_bars():
    D, flags, sel, region = case(8, 5, [8, 5, 3], seed=11)
    kw = LOSSES["all"]
    _, g = BR.loss_grad(D, flags, sel=sel, region=region, **kw)
    moved = {
        "a tie given wholly to one side": _rel(BR.loss_grad(D, flags, sel=sel, region=region, tie="first", **kw)[1], g),
        "the 0.5 of * 0.5 + 0.5 dropped": _rel(BR.loss_grad(D, flags, sel=sel, region=region, half=False, **kw)[1], g),
        "padded nodes counted": _rel(BR.loss_grad(D, flags, sel=sel, region=region, count_padded=True, **kw)[1], g),
    }
    # the guided estimate of one call at a middle noise level
    scfg = _scfg(8)
    t = float(lib.sigma_schedule(scfg)[1][4])
    rng = np.random.default_rng(2)
    f = flags.astype(bool)
    Da = np.where(f[:, None, :, None] & f[:, None, None, :], rng.standard_normal((3, 2, 8, 8)), 0.0)
    Dn = np.where(f[:, :, None], D, 0.0)
    xh = (Da + t * rng.standard_normal(Da.shape), Dn + t * rng.standard_normal(Dn.shape))
    right = BR.guided_call(xh, (Da, Dn), flags, BR.coef(1.5, t), None, sel=sel, region=region, **kw)
    wrong = BR.guided_call(xh, (Da, Dn), flags, BR.coef(1.5, t, with_cskip=False), None, sel=sel, region=region, **kw)
    moved["c_skip left out of c_i"] = _rel(wrong["D_guided"], right["D_guided"])
    # the self-conditioning input of the next call is D; feeding it the guided estimate moves it by the shift itself
    moved["the shift also applied to the self-conditioning input"] = _rel(right["D_guided"], Dn)
    for what, d in moved.items():
        print(f"BOXGUIDE power: {what}: {d:.3e} of the tensor's maximum (loosest bar {LOOSEST_BAR:.0e})")
        assert d > 10 * LOOSEST_BAR, what
