"""GPU: the backward of the input assembly fused with the preconditioning chain (t_assemble_bwd_kernel, csrc/train_kernels.hip) on
its own, through dsg_debug_t_assemble_bwd.  EVERY output element is compared with the float64 restatement of tests/guide_ref.py on
the same fp32 operands, inside the derived bar (n_terms + 2) 2^-24 sum|terms|.  Shapes: N below, at and above the 64-column tile and
not a multiple of anything (5, 8, 40, 64 = 1 block column tile; the channel tile of 32 is crossed by C_adj = 51), all four channel
forms, the assembly's layout with and without self-conditioning slots, B = 1 and 3, the four flag patterns: the full product.  The columns the kernel
must not read (self-conditioning slots, pitch padding) hold 1e30.  Outputs carry NaN-filled guard rows.

Plus: repeated calls are bit-identical (no atomics, one summation order); the result may be written over g in place; PatchEmbed's
dx product at the Visual Genome / COCO-Stuff widths takes the MFMA route once its weight image is padded to 32 columns."""
import ctypes as C

import numpy as np
import pytest
import torch

import guide_ref as GR

pytestmark = pytest.mark.gpu

CHANNELS = [(6, 12), (3, 12), (1, 5), (51, 154)]
NS = [5, 8, 40, 64]


def _lib():
    from diffusesg_amd import lib as L
    return L.load()


def _p(t):
    return C.c_void_p(t.data_ptr())


def _call(o, out_adj=None, out_node=None, g_dev=None):
    dev = {k: torch.from_numpy(o[k]).cuda() for k in ("d_tok", "flags", "c_skip", "c_in", "g_adj", "g_node")}
    if g_dev is not None:
        dev["g_adj"], dev["g_node"] = g_dev
    na, nn = o["g_adj"].size, o["g_node"].size
    oa = torch.full((na + 64,), float("nan"), device="cuda") if out_adj is None else out_adj
    on = torch.full((nn + 64,), float("nan"), device="cuda") if out_node is None else out_node
    rc = _lib().dsg_debug_t_assemble_bwd(o["B"], o["N"], o["c_adj"], o["c_node"], int(o["self_cond"]), _p(dev["d_tok"]), o["ld"],
                                         _p(dev["flags"]), _p(dev["c_skip"]), _p(dev["c_in"]), _p(dev["g_adj"]), _p(dev["g_node"]),
                                         _p(oa), _p(on), None)
    assert rc == 0, f"dsg_debug_t_assemble_bwd: status {rc}"
    return oa, on


def _cases():
    """the full product: N x channels x self-conditioning slots x B x flag pattern"""
    return [(N, ch, sc, B, fk) for N in NS for ch in CHANNELS for sc in (False, True) for B in (1, 3)
            for fk in ("all", "one", "none", "ragged")]


@pytest.mark.parametrize("N,ch,sc,B,fk", _cases(), ids=lambda v: str(v).replace(" ", ""))
def test_assemble_bwd_every_element(N, ch, sc, B, fk):
    o = GR.assemble_bwd_case(B, N, ch[0], ch[1], sc, fk)
    ref_a, ref_n, bar_a, bar_n = GR.assemble_bwd_expect(o)
    oa, on = _call(o)
    na, nn = ref_a.size, ref_n.size
    ga, gn = oa.cpu().numpy(), on.cpu().numpy()
    assert np.isnan(ga[na:]).all() and np.isnan(gn[nn:]).all(), "written behind the outputs"
    ra = GR.worst_ratio(ga[:na].reshape(ref_a.shape), ref_a, bar_a)
    rn = GR.worst_ratio(gn[:nn].reshape(ref_n.shape), ref_n, bar_n)
    print(f"ASMBWD N{N} C{ch} sc{int(sc)} B{B} {fk}: worst |err| / bar adj {ra:.3f} node {rn:.3f}")
    assert ra <= 1.0, f"adjacency gradient: {ra:.2f} x the derived bar"
    assert rn <= 1.0, f"node gradient: {rn:.2f} x the derived bar"
    f = o["flags"].astype(bool)
    assert (gn[:nn].reshape(ref_n.shape)[~f] == 0).all(), "node gradient of a padded node is not exactly 0"


@pytest.mark.parametrize("N,ch,sc", [(40, (3, 12), True), (8, (51, 154), False)])
def test_assemble_bwd_repeatable_and_in_place(N, ch, sc):
    o = GR.assemble_bwd_case(3, N, ch[0], ch[1], sc, "ragged", seed=5)
    a1, n1 = _call(o)
    a2, n2 = _call(o)
    na, nn = o["g_adj"].size, o["g_node"].size
    assert torch.equal(a1[:na], a2[:na]) and torch.equal(n1[:nn], n2[:nn]), "two calls differ"
    ga, gn = torch.from_numpy(o["g_adj"]).cuda().reshape(-1), torch.from_numpy(o["g_node"]).cuda().reshape(-1)
    a3, n3 = _call(o, out_adj=ga, out_node=gn, g_dev=(ga, gn))   # dsg_precond_vjp's own use: the result overwrites g
    assert torch.equal(a3, a1[:na]) and torch.equal(n3, n1[:nn]), "in place differs from out of place"


@pytest.mark.parametrize("name,live", [("vg", 30), ("coco", 27)])
def test_patch_embed_dx_product_takes_the_mfma_route(name, live):
    """d_tok = d_pe_lin [M0, E] W_img [E, 32]: the live columns (C_adj + 2 C_node = 30 / 27) padded to 32 in the WEIGHT image take
    route 1 (the MFMA GEMM); the unpadded width would fall to the plain kernel (route 3), which is why the image is padded"""
    from diffusesg_amd import synth as Y
    cfg = Y.CONFIGS[name]()
    assert cfg.c_adj + 2 * cfg.c_node == live
    E, M0, Np = cfg.embed_dim, cfg.max_node_num ** 2, (live + 31) // 32 * 32
    rng = np.random.default_rng(3)
    A = torch.from_numpy(rng.standard_normal((M0, E)).astype(np.float32)).cuda()
    Wimg = np.zeros((E, Np), np.float32)
    Wimg[:, :live] = rng.standard_normal((E, live)).astype(np.float32)
    Wd = torch.from_numpy(Wimg).cuda()
    out = torch.full((M0, Np), float("nan"), device="cuda")
    route = (C.c_int32 * 2)(-1, -1)
    rc = _lib().dsg_debug_t_gemm(0, 0, _p(A), E, _p(Wd), Np, None, _p(out), Np, M0, Np, E, 0, None, None, 0, None, 0, route, None)
    assert rc == 0 and route[0] == 1, f"padded product took route {route[0]}"
    ref = A.double().cpu().numpy() @ Wimg.astype(np.float64)
    bar = (E + 8) * GR.U * (np.abs(A.cpu().numpy()).astype(np.float64) @ np.abs(Wimg).astype(np.float64)) + 1e-30
    got = out.cpu().numpy()
    assert GR.worst_ratio(got[:, :live], ref[:, :live], bar[:, :live]) <= 1.0
    assert (got[:, live:] == 0).all(), "the padded columns of the image are zero: so is their product"
    out2 = torch.empty((M0, live), device="cuda")
    Wn = Wd[:, :live].contiguous()
    rc = _lib().dsg_debug_t_gemm(0, 0, _p(A), E, _p(Wn), live, None, _p(out2), live, M0, live, E, 0, None, None, 0, None, 0, route, None)
    assert rc == 0 and route[0] == 3, f"unpadded product took route {route[0]} (expected the plain kernel)"
