"""No GPU: the host side of loss-guided sampling (diffusesg_amd/guide.py) -- the three ready-made losses against independent float64
restatements (value and autograd gradient, CPU), argument checks, the clip arithmetic, the handling of the guidance weights, and
the float64 restatement of the guided estimate that the GPU tests rely on (tests/guide_ref.py)."""
import numpy as np
import pytest
import torch

import guide_ref as GR
from diffusesg_amd import guide


def _nodes(B=3, N=6, C=9, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, C, generator=g, dtype=torch.float64) * 0.6
    return x.to(dtype)


def _box64(D_node):
    b = D_node.double()[..., -4:] * 0.5 + 0.5
    cx, cy, w, h = b.unbind(-1)
    return cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, cx, cy


def _overlap64(D_node, flags):
    l, t, r, bt, _, _ = _box64(D_node)
    tot = torch.zeros((), dtype=torch.float64)
    B, N = l.shape
    for b in range(B):
        for i in range(N):
            for j in range(i + 1, N):
                if flags is not None and not (flags[b, i] and flags[b, j]):
                    continue
                iw = torch.clamp(torch.min(r[b, i], r[b, j]) - torch.max(l[b, i], l[b, j]), min=0)
                ih = torch.clamp(torch.min(bt[b, i], bt[b, j]) - torch.max(t[b, i], t[b, j]), min=0)
                tot = tot + iw * ih
    return tot


def _region64(D_node, idx, region, flags):
    l, t, r, bt, _, _ = _box64(D_node)
    x0, y0, x1, y1 = region
    tot = torch.zeros((), dtype=torch.float64)
    for b in range(l.shape[0]):
        for i in idx:
            if flags is not None and not flags[b, i]:
                continue
            tot = tot + torch.clamp(x0 - l[b, i], min=0) ** 2 + torch.clamp(y0 - t[b, i], min=0) ** 2 \
                + torch.clamp(r[b, i] - x1, min=0) ** 2 + torch.clamp(bt[b, i] - y1, min=0) ** 2
    return tot


def _align64(D_node, flags, tau):
    l, t, r, bt, cx, cy = _box64(D_node)
    tot = torch.zeros((), dtype=torch.float64)
    B, N = l.shape
    for b in range(B):
        ok = [i for i in range(N) if flags is None or flags[b, i]]
        if len(ok) < 2:
            continue
        for line in (l, cx, r, t, cy, bt):
            for i in ok:
                d2 = torch.stack([(line[b, i] - line[b, j]) ** 2 for j in ok if j != i])
                tot = tot + (-tau * torch.logsumexp(-d2 / tau, 0) + tau * np.log(len(ok) - 1))
    return tot


FLAGS = torch.tensor([[1, 1, 1, 1, 1, 1], [1, 1, 1, 0, 0, 0], [1, 0, 0, 0, 0, 0]], dtype=torch.uint8)


@pytest.mark.parametrize("flags", [None, FLAGS], ids=["noflags", "ragged"])
@pytest.mark.parametrize("which", ["overlap", "region", "align"])
def test_losses_against_float64(which, flags):
    x32 = _nodes().requires_grad_(True)
    x64 = x32.detach().double().requires_grad_(True)
    if which == "overlap":
        mine, ref = guide.box_overlap_loss(flags)(None, x32), _overlap64(x64, flags)
    elif which == "region":
        reg = (0.1, 0.2, 0.55, 0.6)
        mine, ref = guide.box_region_loss([0, 2], reg, flags)(None, x32), _region64(x64, [0, 2], reg, flags)
    else:
        mine, ref = guide.box_alignment_loss(flags, tau=0.05)(None, x32), _align64(x64, flags, 0.05)
    mine.backward()
    ref.backward()
    assert float(ref.detach()) > 0
    assert abs(float(mine.detach()) - float(ref.detach())) <= 1e-5 * float(ref.detach())
    scale = float(x64.grad.abs().max())
    assert scale > 0
    assert float((x32.grad.double() - x64.grad).abs().max()) <= 1e-5 * scale
    assert (x32.grad[..., :-4] == 0).all(), "only the box channels carry gradient"
    if flags is not None:
        assert (x32.grad[~flags.bool()] == 0).all(), "padded nodes take no part"


def test_losses_run_in_float64_too_and_alignment_vanishes_when_aligned():
    x = _nodes(dtype=torch.float64)
    assert guide.box_overlap_loss()(None, x).dtype == torch.float64
    x[..., -4:] = torch.tensor([0.1, -0.2, 0.3, 0.4], dtype=torch.float64)   # every box the same: every line coincides
    assert abs(float(guide.box_alignment_loss()(None, x))) < 1e-12
    assert float(guide.box_region_loss(1, (0.0, 0.0, 1.0, 1.0))(None, x)) == 0.0


def test_argument_checks():
    with pytest.raises(ValueError):
        guide.box_region_loss(0, (0.5, 0.0, 0.5, 1.0))
    with pytest.raises(ValueError):
        guide.box_region_loss(-1, (0.0, 0.0, 1.0, 1.0))
    with pytest.raises(ValueError):
        guide.box_region_loss(9, (0.0, 0.0, 1.0, 1.0))(None, _nodes())
    with pytest.raises(ValueError):
        guide.box_overlap_loss()(None, torch.zeros(2, 5, 3))
    with pytest.raises(ValueError):
        guide.box_alignment_loss(tau=0.0)
    with pytest.raises(TypeError):
        guide.guided_sample(object(), None, torch.ones(1, 8), lambda a, n: n.sum(), 1.0)
    with pytest.raises(ValueError):
        guide.clip_factor(torch.ones(2), torch.ones(2), -1.0)


def test_guidance_weights():
    w = guide.guidance_weights(0.25, 5)
    assert w.dtype == np.float32 and w.shape == (5,) and (w == np.float32(0.25)).all()
    ramp = np.linspace(0, 1, 5)
    for form in (ramp, list(ramp), torch.from_numpy(ramp)):
        assert np.array_equal(guide.guidance_weights(form, 5), ramp.astype(np.float32))
    assert (guide.guidance_weights(0, 3) == 0).all()
    for bad in (np.ones(4), np.ones((5, 1)), [1.0, float("nan"), 1, 1, 1], float("inf")):
        with pytest.raises(ValueError):
            guide.guidance_weights(bad, 5)


def test_clip_arithmetic():
    sn = torch.tensor([0.0, 1.0, 4.0, 4.0, 3.0], dtype=torch.float64)
    rn = torch.tensor([1.0, 2.0, 2.0, 0.0, 3.0], dtype=torch.float64)
    f = guide.clip_factor(sn, rn, 1.0)
    assert torch.equal(f, torch.tensor([1.0, 1.0, 0.5, 0.0, 1.0], dtype=torch.float64))   # inside: untouched; outside: onto the bound
    assert torch.equal(guide.clip_factor(sn, rn, None), torch.ones(5, dtype=torch.float64))
    assert torch.equal(guide.clip_factor(sn, rn, 0.5), torch.tensor([1.0, 1.0, 0.25, 0.0, 0.5], dtype=torch.float64))
    assert bool((f * sn <= 1.0 * rn + 1e-15).all())
    assert torch.isfinite(guide.clip_factor(torch.zeros(2), torch.zeros(2), 1.0)).all()


def test_float64_restatement_of_the_guided_estimate():
    """tests/guide_ref.py against the definition: an unclipped shift is w t^2 mask(grad); a clipped one has norm r ||x_hat - D|| per
    graph; known entries win; padded entries are 0"""
    rng = np.random.default_rng(0)
    B, N, Ca, Cn = 2, 4, 2, 5
    flags = np.array([[1, 1, 1, 1], [1, 1, 0, 0]], np.uint8)
    sh_a, sh_n = (B, Ca, N, N), (B, N, Cn)
    xh = (rng.standard_normal(sh_a).astype(np.float32), rng.standard_normal(sh_n).astype(np.float32))
    D = (rng.standard_normal(sh_a).astype(np.float32), rng.standard_normal(sh_n).astype(np.float32))
    g = (rng.standard_normal(sh_a).astype(np.float32), rng.standard_normal(sh_n).astype(np.float32))
    f = flags.astype(bool)
    fa, fn = (f[:, None, :, None] & f[:, None, None, :]), f[:, :, None]
    (sa, sn), (Ga, Gn) = GR.guided_estimate(xh, D, g, 0.5, 2.0, flags, None)
    assert np.allclose(sa, np.where(fa, g[0] * 2.0, 0)) and np.allclose(Gn, D[1] - np.where(fn, g[1] * 2.0, 0))
    (sa, sn), _ = GR.guided_estimate(xh, D, g, 50.0, 2.0, flags, 0.3)
    assert np.allclose(GR.graph_norm(sa, sn), 0.3 * GR.graph_norm(xh[0] - D[0].astype(np.float64), xh[1] - D[1].astype(np.float64)))
    ka, kn = np.full(sh_a, 7.0), np.full(sh_n, -7.0)
    ma, mn = rng.random(sh_a) < 0.5, rng.random(sh_n) < 0.5
    _, (Ga, Gn) = GR.guided_estimate(xh, D, g, 0.5, 2.0, flags, 1.0, known=(ka, kn, ma, mn))
    assert (Ga[ma & fa] == 7.0).all() and (Gn[mn & np.broadcast_to(fn, sh_n)] == -7.0).all()
    assert (Ga[~np.broadcast_to(fa, sh_a)] == 0).all() and (Gn[~np.broadcast_to(fn, sh_n)] == 0).all()
