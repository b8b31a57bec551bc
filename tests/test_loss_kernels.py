"""GPU: the kernels every training step starts from, on their own (csrc/kernels.hip: rainbow_loss_kernel, rainbow_loss_backward_kernel with
box_iou_term, train_inputs_kernel) through dsg_rainbow_loss, dsg_rainbow_loss_backward and dsg_train_inputs.  EVERY output element is
compared with the float64 autograd reference of tests/loss_ref.py on its shared case list: one node, the fixture's shape, the `vg` shape,
N = 300 (the strided loops and the 256-slot tree), ragged / holed / full flags, every optional argument absent once, and for all five
iou_loss_types a random box family and a constructed one whose corners tie, sit exactly on 0 or 1, leave [0, 1], touch, miss and enclose.

Conventions of tests/test_f32_kernels.py: outputs are NaN-filled and carry guard elements that must stay NaN.  Beyond the bars: padded
gradient entries are exactly 0; a second launch on the same inputs and a third one with NaN in every padded entry of the predictions and
the targets give the same bits (fixed summation order, choice by select).  The objective's weights and noisy tensors are bit-identical to
NumPy float32 evaluated operation by operation from the kernel's own sigmas.  The bars come from tests/loss_ref.py (16 x the float32
evaluation of the reference, capped by the fixture test's bars), none from a kernel's output; tests/test_loss_kernels_host.py shows what
they can see.  Lines LOSSK ... print the figures; measured ones: profiles/loss_kernel_errors.md."""
import ctypes as C

import numpy as np
import pytest
import torch

import loss_ref as R

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000
GUARD = 8      # elements behind every output buffer
CASES = R.cases()
OBJECTIVE_CASES = [c for c in CASES if c.spec.variant == "all"]


def _lib():
    from diffusesg_amd import lib as L
    return L, L.load()


def _p(t):
    """the device address of a tensor the CALLER keeps alive"""
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev(a):
    return None if a is None else torch.tensor(np.asarray(a)).cuda()


def _out(n):
    return torch.full((n + GUARD,), float("nan"), device="cuda")


def _take(buf, shape, what):
    """the result of a NaN-filled buffer with guard elements: the guards still hold the fill, bit for bit"""
    host = buf.cpu()
    n = int(np.prod(shape))
    assert (host[n:].view(torch.int32) == NAN_BITS).all(), f"{what}: written past its end"
    return host[:n].numpy().reshape(shape).copy()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nan_padded(case):
    """predictions and targets with NaN in every padded entry"""
    f = case.flags.astype(bool)
    fa = np.broadcast_to(f[:, None, :, None] & f[:, None, None, :], case.pred_adj.shape)
    fx = np.broadcast_to(f[:, :, None], case.pred_node.shape)
    nan = np.float32("nan")
    return [np.where(m, a, nan) for a, m in ((case.pred_adj, fa), (case.pred_node, fx), (case.tgt_adj, fa), (case.tgt_node, fx))]


def run_loss(case, iou_type, tensors=None):
    """one launch of both entries -> dict of NumPy outputs (None where an output is not asked for)"""
    L, lib = _lib()
    s = case.spec
    pa, px, ta, tx = (_dev(a) for a in (tensors or (case.pred_adj, case.pred_node, case.tgt_adj, case.tgt_node)))
    fl, w, sg = _dev(case.flags), _dev(case.weights), _dev(case.sigmas)
    code = L.iou_loss_type_code(iou_type)
    la, ln = _out(s.B), _out(s.B)
    rc = lib.dsg_rainbow_loss(s.B, s.N, s.Ca, s.Cn, _p(pa), _p(px), _p(ta), _p(tx), _p(fl), _p(w), case.edge_w, case.node_w, case.iou_w, code,
                              _p(la), _p(ln), _stream())
    assert rc == 0, f"dsg_rainbow_loss: status {rc}"
    ga, gx = _out(pa.numel()), _out(px.numel())
    fa, fx = (_out(pa.numel()), _out(px.numel())) if sg is not None else (None, None)
    rc = lib.dsg_rainbow_loss_backward(s.B, s.N, s.Ca, s.Cn, _p(pa), _p(px), _p(ta), _p(tx), _p(fl), _p(w), case.edge_w, case.node_w, case.iou_w,
                                       code, _p(sg), _p(ga), _p(gx), _p(fa), _p(fx), _stream())
    assert rc == 0, f"dsg_rainbow_loss_backward: status {rc}"
    torch.cuda.synchronize()
    out = {"loss_adj": _take(la, (s.B,), "loss_adj"), "loss_node": _take(ln, (s.B,), "loss_node"),
           "grad_adj": _take(ga, case.pred_adj.shape, "grad_adj"), "grad_node": _take(gx, case.pred_node.shape, "grad_node"),
           "grad_F_adj": None if fa is None else _take(fa, case.pred_adj.shape, "grad_F_adj"),
           "grad_F_node": None if fx is None else _take(fx, case.pred_node.shape, "grad_F_node")}
    return out


def _same_bits(a, b, what):
    for k in a:
        assert (a[k] is None) == (b[k] is None)
        if a[k] is not None:
            assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), f"{what}: {k} differs in {int((a[k].view(np.int32) != b[k].view(np.int32)).sum())} elements"


@pytest.fixture(scope="module")
def worst():
    """family -> the largest |err| / bar of the file, printed once at its end"""
    w = {}
    yield w
    for fam in R.FAMILIES:
        if fam in w:
            bar, disc = R.bars()[fam]
            print(f"\nLOSSK summary {fam}: bar {bar:.3e} (float32 reference {disc:.3e}), worst |err| / bar = {w[fam][0]:.3f} at {w[fam][1]}")
    if "sigma_ulp" in w:
        print(f"LOSSK summary sigmas: worst rel err {w['sigma_rel'][0]:.3e} (bar 2e-6), {w['sigma_ulp'][0]:.2f} ulp at {w['sigma_ulp'][1]}")


@pytest.mark.parametrize("iou_type", R.IOU_TYPES)
@pytest.mark.parametrize("case", CASES, ids=R.CASE_IDS)
def test_loss_and_backward_against_float64_autograd(case, iou_type, worst):
    got = run_loss(case, iou_type)
    ratios = R.compare(got, R.reference(case, iou_type))
    print(f"LOSSK {case.name} {iou_type}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    for fam, r in ratios.items():
        if r > worst.get(fam, (0.0, None))[0]:
            worst[fam] = (r, f"{case.name} {iou_type}")
    # padded entries of the gradients are exactly 0
    f = case.flags.astype(bool)
    pad_a = ~np.broadcast_to(f[:, None, :, None] & f[:, None, None, :], case.pred_adj.shape)
    for k in ("grad_adj", "grad_F_adj"):
        assert got[k] is None or (got[k][pad_a] == 0).all(), k
    for k in ("grad_node", "grad_F_node"):
        assert got[k] is None or (got[k][~f] == 0).all(), k
    # the summation order is fixed, and both kernels choose by select: NaN in a padded entry reaches nothing
    _same_bits(got, run_loss(case, iou_type), "a second launch on the same inputs")
    _same_bits(got, run_loss(case, iou_type, _nan_padded(case)), "NaN in every padded entry")
    for fam, r in ratios.items():
        assert r <= 1.0, f"{case.name} {iou_type} {fam}: {r:.2f} x the bar {R.bars()[fam][0]:.2e}"


@pytest.mark.parametrize("case", OBJECTIVE_CASES, ids=[c.name for c in OBJECTIVE_CASES])
def test_train_inputs_replayed_draws(case, worst):
    """sigmas against exp in float64 of the float32-rounded argument (the existing 2e-6 relative bar; the worst error in ulp is recorded);
    then, from the kernel's own sigmas, weights and both noisy tensors bit for bit against NumPy float32 operation by operation --
    fl(fl(s s) + 0.25) / fl(fl(0.5 s)^2), fl(clean + fl(eps s)) -- which a contracted multiply-add does not pass (host test)"""
    L, lib = _lib()
    s = case.spec
    ca, cx, fl = _dev(case.tgt_adj), _dev(case.tgt_node), _dev(case.flags)
    rnd, ea, ex = _dev(case.rnd), _dev(case.eps_adj), _dev(case.eps_node)
    sig, wts, na, nx = _out(s.B), _out(s.B), _out(ca.numel()), _out(cx.numel())
    rc = lib.dsg_train_inputs(s.B, s.N, s.Ca, s.Cn, _p(ca), _p(cx), _p(fl), _p(rnd), _p(ea), _p(ex), C.c_uint64(0), _p(sig), _p(wts), _p(na), _p(nx),
                              _stream())
    assert rc == 0
    torch.cuda.synchronize()
    sig, wts = _take(sig, (s.B,), "sigmas"), _take(wts, (s.B,), "weights")
    na, nx = _take(na, case.tgt_adj.shape, "noisy_adj"), _take(nx, case.tgt_node.shape, "noisy_node")
    ref = R.sigma_reference(case.rnd)
    rel, ulp = float((np.abs(sig - ref) / ref).max()), float(R.ulp_err(sig, ref).max())
    print(f"LOSSK train_inputs {case.name}: sigmas rel err {rel:.3e}, {ulp:.2f} ulp")
    for key, v in (("sigma_rel", rel), ("sigma_ulp", ulp)):
        if v >= worst.get(key, (-1.0, None))[0]:
            worst[key] = (v, case.name)
    assert rel <= 2e-6
    w, a, x = R.train_inputs_from_sigmas(case, sig)
    for got, want, what in ((wts, w, "weights"), (na, a, "noisy_adj"), (nx, x, "noisy_node")):
        diff = got.view(np.int32) != want.view(np.int32)
        assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} elements differ from float32 operation by operation"
    f = case.flags.astype(bool)
    assert (na[~np.broadcast_to(f[:, None, :, None] & f[:, None, None, :], na.shape)].view(np.int32) == 0).all()   # +0.0
    assert np.array_equal(nx[~f].view(np.int32), case.tgt_node[~f].view(np.int32))
