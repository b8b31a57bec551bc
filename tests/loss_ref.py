"""Float64 reference of the kernels every training step starts from (include/dsg.h: dsg_train_inputs, dsg_rainbow_loss,
dsg_rainbow_loss_backward), the case list the CPU and the GPU tests share, and the bars.

The loss is a plain torch restatement, dtype selectable, of what the header promises: the masked, weighted MSE terms of
NodeAdjRainbowLoss(reduction='none'), the trainer's bounding-box block for the five iou_loss_types with its division of the per-graph
sums by the number of valid nodes of the WHOLE batch, loss = mean_b(loss_adj) + mean_b(loss_node), and grad_F = c_out(sigma_b) * grad.
Every gradient comes from `backward()` through torch.maximum / torch.minimum / clamp / atan: nothing here is a derived chain rule, which is
the point -- the kernel (csrc/kernels.hip: box_iou_term) and the CPU oracle (oracle/dsg_ref.c: box_term) were derived by one hand.

The keyword switches of `evaluate` restate MISTAKES (tests/test_loss_kernels_host.py shows that each moves an output beyond the bars):
  tie='whole' | 'drop'   a tie of a maximum / minimum given wholly to the prediction / dropped (tie_types: the loss types it applies to)
  clamp_exclusive        the clamp to [0, 1] passes the gradient only strictly inside
  open_ge                `>=` in the open-intersection mask of types 1 to 4
  per_graph_count        the IoU term divided by the graph's own node count, not the batch total
  no_inv_b               the 1/B of the batch mean left out of the gradients
  no_iou_loss_weight     loss_weight left out of the IoU term
  adj_n_not_n2           n for n^2 in the adjacency term
  no_c_out               grad_F = grad
"""
import functools
import math
from dataclasses import dataclass

import numpy as np
import torch

from diffusesg_amd import spec as S

IOU_TYPES = ("iou", "giou", "giou_squared", "diou", "ciou")   # DSG_IOU_* 0 .. 4
EDGE_W, NODE_W, IOU_W = 1.5, 0.5, 0.75                         # exact in float32
EPS = 1e-7
MARGIN = 1e-4      # the random family: whatever a max, min, clamp or > compares differs by more than this
MIN_EXTENT = 0.05  # widths and heights after the clamp (a collapsed box is NaN under 'ciou' in torchvision itself)
FLOOR = {"loss_adj": 2e-5, "loss_node": 2e-5, "grad_adj": 1e-5, "grad_node_box": 1e-5, "grad_node_rest": 1e-5}   # the fixture test's bars
FAMILIES = tuple(FLOOR)


# ----------------------------------------------------------------------------------------------------------------------------------
# the loss
# ----------------------------------------------------------------------------------------------------------------------------------
class _TieExt(torch.autograd.Function):
    """maximum / minimum whose backward hands the prediction `share` of a tie (autograd: 0.5) -- the seeded mistakes only"""

    @staticmethod
    def forward(ctx, a, b, is_max, share):
        ctx.save_for_backward(a, b)
        ctx.is_max, ctx.share = is_max, share
        return torch.maximum(a, b) if is_max else torch.minimum(a, b)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        win = (a > b) if ctx.is_max else (a < b)
        wa = torch.where(win, 1.0, torch.where(a == b, ctx.share, 0.0)).to(g.dtype)
        return g * wa, g * (1.0 - wa), None, None


class _ClampOpen(torch.autograd.Function):
    """clamp to [0, 1] whose backward is open at both edges -- a seeded mistake"""

    @staticmethod
    def forward(ctx, v):
        ctx.save_for_backward(v)
        return v.clamp(min=0.0, max=1.0)

    @staticmethod
    def backward(ctx, g):
        v, = ctx.saved_tensors
        return g * ((v > 0.0) & (v < 1.0)).to(g.dtype)


def _ext(tie):
    if tie == "split":
        return torch.maximum, torch.minimum
    share = {"whole": 1.0, "drop": 0.0}[tie]
    return (lambda a, b: _TieExt.apply(a, b, True, share)), (lambda a, b: _TieExt.apply(a, b, False, share))


def _xyxy(ch4, clamp_exclusive=False):
    """the last four node channels -> clamped corners: (x + 1) / 2 -> cxcywh -> xyxy -> clamp[0, 1]"""
    b = (ch4 + 1.0) / 2.0
    cx, cy, w, h = b.unbind(-1)
    v = torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)
    return _ClampOpen.apply(v) if clamp_exclusive else v.clamp(min=0.0, max=1.0)


def box_term(p, g, iou_type, tie="split", open_ge=False):
    """per-box loss of clamped corners p (prediction), g (target), [..., 4]:
      'iou'   -(box_iou)^2, box_iou = inter / (area_p + area_g - inter), inter = prod((min(rb) - max(lt)).clamp(min=0))
      others  torchvision.ops' generalized_ / distance_ / complete_box_iou_loss(reduction='none'), eps = 1e-7: the intersection only
              where both overlaps are open, iou = inter / (union + eps); 'giou_squared' squares the first"""
    mx, mn = _ext(tie)
    x1, y1, x2, y2 = p.unbind(-1)
    x1g, y1g, x2g, y2g = g.unbind(-1)
    area_p, area_g = (x2 - x1) * (y2 - y1), (x2g - x1g) * (y2g - y1g)
    if iou_type == "iou":
        w = (mn(x2, x2g) - mx(x1, x1g)).clamp(min=0.0)
        h = (mn(y2, y2g) - mx(y1, y1g)).clamp(min=0.0)
        inter = w * h
        iou = inter / (area_p + area_g - inter)
        return -(iou ** 2.0)
    xk1, yk1, xk2, yk2 = mx(x1, x1g), mx(y1, y1g), mn(x2, x2g), mn(y2, y2g)
    mask = ((yk2 >= yk1) & (xk2 >= xk1)) if open_ge else ((yk2 > yk1) & (xk2 > xk1))
    inter = torch.where(mask, (xk2 - xk1) * (yk2 - yk1), torch.zeros_like(x1))
    union = area_p + area_g - inter
    iou = inter / (union + EPS)
    xc1, yc1, xc2, yc2 = mn(x1, x1g), mn(y1, y1g), mx(x2, x2g), mx(y2, y2g)
    if iou_type in ("giou", "giou_squared"):
        area_c = (xc2 - xc1) * (yc2 - yc1)
        loss = 1.0 - (iou - (area_c - union) / (area_c + EPS))
        return loss ** 2.0 if iou_type == "giou_squared" else loss
    diag = (xc2 - xc1) ** 2 + (yc2 - yc1) ** 2 + EPS
    dist = ((x2 + x1) / 2.0 - (x1g + x2g) / 2.0) ** 2 + ((y2 + y1) / 2.0 - (y1g + y2g) / 2.0) ** 2
    loss = 1.0 - iou + dist / diag
    if iou_type == "diou":
        return loss
    assert iou_type == "ciou", iou_type
    v = (4.0 / math.pi ** 2) * (torch.atan((x2g - x1g) / (y2g - y1g)) - torch.atan((x2 - x1) / (y2 - y1))) ** 2
    with torch.no_grad():
        alpha = v / (1.0 - iou + v + EPS)
    return loss + alpha * v


def evaluate(case, iou_type, dtype=torch.float64, tie="split", tie_types=IOU_TYPES, clamp_exclusive=False, open_ge=False,
             per_graph_count=False, no_inv_b=False, no_iou_loss_weight=False, adj_n_not_n2=False, no_c_out=False):
    """-> dict of float64 NumPy arrays: loss_adj [B], loss_node [B], grad_adj, grad_node, grad_F_adj | None, grad_F_node | None"""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    pa, px = t(case.pred_adj).requires_grad_(True), t(case.pred_node).requires_grad_(True)
    ta, tx = t(case.tgt_adj), t(case.tgt_node)
    f = torch.from_numpy(case.flags.astype(bool))
    B, N = f.shape
    Ca, Cn = pa.shape[1], px.shape[2]
    w = torch.ones(B, dtype=dtype) if case.weights is None else t(case.weights)
    n = f.sum(-1).to(dtype)
    fa = f[:, None, :, None] & f[:, None, None, :]
    zero = torch.zeros((), dtype=dtype)
    sq_a = torch.where(fa, (pa - ta) ** 2 * w[:, None, None, None], zero)
    sq_x = torch.where(f[:, :, None], (px - tx) ** 2 * w[:, None, None], zero)
    loss_adj = sq_a.sum(dim=(1, 2, 3)) / (n if adj_n_not_n2 else n ** 2) / Ca * case.edge_w
    loss_node = sq_x.sum(dim=(1, 2)) / n / Cn * case.node_w
    if case.iou_w != 0.0:
        safe = torch.zeros(4, dtype=dtype)   # a padded row's box is not read: a well-formed one takes its place before any division
        p = _xyxy(torch.where(f[:, :, None], px[..., -4:], safe), clamp_exclusive)
        g = _xyxy(torch.where(f[:, :, None], tx[..., -4:], safe))
        per_node = box_term(p, g, iou_type, tie if iou_type in tie_types else "split", open_ge)
        per_graph = torch.where(f, per_node, zero).sum(-1) / (n if per_graph_count else f.sum().to(dtype))
        loss_node = loss_node + case.iou_w * per_graph * (1.0 if no_iou_loss_weight else w)
    total = loss_adj.mean() + loss_node.mean()
    total.backward()
    scale = float(B) if no_inv_b else 1.0
    out = {"loss_adj": loss_adj.detach(), "loss_node": loss_node.detach(), "grad_adj": pa.grad * scale, "grad_node": px.grad * scale,
           "grad_F_adj": None, "grad_F_node": None}
    if case.sigmas is not None:
        sg = t(case.sigmas)
        c_out = torch.ones_like(sg) if no_c_out else sg * 0.5 / torch.sqrt(sg * sg + 0.25)
        out["grad_F_adj"], out["grad_F_node"] = out["grad_adj"] * c_out[:, None, None, None], out["grad_node"] * c_out[:, None, None]
    return {k: None if v is None else v.double().numpy() for k, v in out.items()}


def split_families(res):
    """the output families of the bars: grad_node's box channels apart from the others (None where a family has no element)"""
    gn = res["grad_node"]
    return {"loss_adj": res["loss_adj"], "loss_node": res["loss_node"], "grad_adj": res["grad_adj"], "grad_node_box": gn[..., -4:],
            "grad_node_rest": gn[..., :-4] if gn.shape[-1] > 4 else None}


def family_of_output(key):
    """output name -> the families its elements belong to, as (family, selector) pairs; grad_F_* share the bars of grad_*"""
    key = key.replace("grad_F_", "grad_")
    if key == "grad_node":
        return (("grad_node_box", lambda a: a[..., -4:]), ("grad_node_rest", lambda a: a[..., :-4]))
    return ((key, lambda a: a),)


def rel_err(got, ref):
    ref = np.asarray(ref, np.float64)
    if ref.size == 0:
        return 0.0
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


# ----------------------------------------------------------------------------------------------------------------------------------
# what the boxes of a case reach (plain float64 arithmetic on the corners, apart from the autograd code above)
# ----------------------------------------------------------------------------------------------------------------------------------
def corners(ch4):
    b = (np.asarray(ch4, np.float64) + 1.0) / 2.0
    raw = np.stack([b[..., 0] - 0.5 * b[..., 2], b[..., 1] - 0.5 * b[..., 3], b[..., 0] + 0.5 * b[..., 2], b[..., 1] + 0.5 * b[..., 3]], -1)
    return raw, np.clip(raw, 0.0, 1.0)


def box_events(pred_node, tgt_node, flags):
    """counts over the valid nodes, and the smallest difference between two quantities that a max / min / clamp / > compares"""
    v = np.asarray(flags).astype(bool)
    rp, p = (a[v] for a in corners(pred_node[..., -4:]))
    rg, g = (a[v] for a in corners(tgt_node[..., -4:]))
    dw = np.minimum(p[:, 2], g[:, 2]) - np.maximum(p[:, 0], g[:, 0])
    dh = np.minimum(p[:, 3], g[:, 3]) - np.maximum(p[:, 1], g[:, 1])
    on_edge, out = (rp == 0.0) | (rp == 1.0), (rp < 0.0) | (rp > 1.0)
    same = (p == g).all(-1)
    pw, ph, gw, gh = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1], g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
    ev = {f"tie corner {t}": int(((p[:, t] == g[:, t]) & ~out[:, t]).sum()) for t in range(4)}   # ties whose share reaches the prediction
    ev.update({
        "all four corners tie": int(same.sum()),
        "one corner ties alone": int((((p == g) & ~out).sum(-1) == 1).sum()),
        "edge-exact corner at 0": int((rp == 0.0).sum()), "edge-exact corner at 1": int((rp == 1.0).sum()),
        "edge-exact corner, target's equal": int((on_edge & (p == g)).sum()), "edge-exact corner, target's elsewhere": int((on_edge & (p != g)).sum()),
        "clamped corner": int(out.sum()),
        "both clamped onto one edge": int((out & ((rg < 0.0) | (rg > 1.0)) & (p == g)).sum()),
        "touching": int((((dw == 0.0) & (dh > 0.0)) | ((dh == 0.0) & (dw > 0.0))).sum()), "touching at a corner": int(((dw == 0.0) & (dh == 0.0)).sum()),
        "disjoint": int(((dw < 0.0) | (dh < 0.0)).sum()),
        "prediction encloses target": int(((p[:, :2] <= g[:, :2]).all(-1) & (p[:, 2:] >= g[:, 2:]).all(-1) & ~same).sum()),
        "target encloses prediction": int(((g[:, :2] <= p[:, :2]).all(-1) & (g[:, 2:] >= p[:, 2:]).all(-1) & ~same).sum()),
        "equal aspect ratios": int(((pw * gh == gw * ph) & ~same).sum()),
    })
    gaps = np.concatenate([np.abs(p - g), np.abs(rp), np.abs(rp - 1.0), np.abs(rg), np.abs(rg - 1.0), np.abs(dw)[:, None], np.abs(dh)[:, None]], 1)
    extent = np.stack([pw, ph, gw, gh], 1)
    return ev, gaps.min(1), extent.min(1)


# ----------------------------------------------------------------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------------------------------------------------------------
_U = 1.0 / 32.0   # the constructed corners are multiples of 2^-5, so the channels x1 + x2 - 1 and 2 (x2 - x1) - 1 are multiples of 2^-5 too:
                  # every channel and every corner is exact in float32 and in float64
CONSTRUCTED = [   # (what, prediction corners, target corners) in units of 1/32; corners beyond 0 .. 32 are clamped
    ("prediction equals target", (8, 8, 24, 24), (8, 8, 24, 24)),
    ("x1 ties alone", (8, 8, 24, 24), (8, 4, 20, 28)),
    ("y1 ties alone", (8, 8, 24, 24), (4, 8, 20, 28)),
    ("x2 ties alone", (8, 8, 24, 24), (12, 4, 24, 28)),
    ("y2 ties alone", (8, 8, 24, 24), (12, 4, 28, 24)),
    ("x1 and y2 tie", (8, 8, 24, 24), (8, 4, 16, 24)),
    ("x1 exactly 0, target's too", (0, 8, 16, 24), (0, 6, 20, 20)),
    ("x1 exactly 0, target's elsewhere", (0, 8, 16, 24), (4, 6, 20, 20)),
    ("x2 exactly 1, target's too", (16, 8, 32, 24), (12, 6, 32, 20)),
    ("x2 exactly 1, target's elsewhere", (16, 8, 32, 24), (12, 6, 28, 20)),
    ("y1 exactly 0, target's too", (8, 0, 24, 16), (6, 0, 20, 20)),
    ("y2 exactly 1, target's elsewhere", (8, 16, 24, 32), (6, 12, 20, 30)),
    ("x1 exactly 0, target clamped onto 0", (0, 8, 16, 24), (-3, 6, 20, 20)),
    ("x1 below 0", (-4, 8, 16, 24), (2, 6, 20, 20)),
    ("x2 above 1", (16, 8, 36, 24), (12, 6, 30, 20)),
    ("y1 below 0", (8, -2, 24, 16), (6, 3, 20, 20)),
    ("y2 above 1", (8, 12, 24, 40), (6, 10, 20, 30)),
    ("both clamped onto x = 0", (-4, 8, 16, 24), (-2, 6, 20, 20)),
    ("both clamped onto x = 1", (16, 8, 36, 24), (12, 6, 34, 20)),
    ("both clamped onto y = 1", (8, 16, 24, 34), (6, 12, 20, 40)),
    ("touching in x", (4, 8, 12, 24), (12, 10, 20, 22)),
    ("touching in y", (8, 4, 24, 12), (10, 12, 22, 20)),
    ("touching at a corner", (4, 4, 12, 12), (12, 12, 20, 20)),
    ("disjoint in both directions", (2, 2, 8, 8), (16, 16, 28, 30)),
    ("disjoint in x alone", (2, 8, 8, 24), (16, 10, 28, 20)),
    ("prediction encloses target", (4, 4, 28, 28), (10, 12, 20, 18)),
    ("target encloses prediction", (10, 12, 20, 18), (4, 4, 28, 28)),
    ("encloses, sharing two sides", (4, 4, 28, 28), (4, 4, 20, 18)),
    ("equal aspect ratios, equal sizes", (4, 4, 20, 12), (10, 10, 26, 18)),
    ("equal aspect ratios, other size", (4, 4, 20, 12), (8, 8, 32, 20)),
]


def _channels(c):
    x1, y1, x2, y2 = (v * _U for v in c)
    return [x1 + x2 - 1.0, y1 + y2 - 1.0, 2.0 * (x2 - x1) - 1.0, 2.0 * (y2 - y1) - 1.0]


@dataclass(frozen=True)
class Spec:
    B: int
    N: int
    Ca: int
    Cn: int
    family: str            # 'random' | 'constructed'
    flags: str = "ragged"  # 'ragged' | 'holes' | 'full'
    variant: str = "all"   # 'all' | 'no_weight' | 'no_sigma' | 'iou_w0'

    @property
    def name(self):
        return f"B{self.B}-N{self.N}-Ca{self.Ca}-Cn{self.Cn}-{self.family}-{self.flags}-{self.variant}"


def _vg():
    c = S.vg_config()
    return (2, c.max_node_num, c.c_adj, c.c_node)


SHAPES = [(1, 1, 1, 4), (4, 8, 6, 12), (3, 20, 3, 9), _vg(), (2, 300, 1, 5)]
SPECS = [Spec(*s, family=fam) for s in SHAPES for fam in ("random", "constructed")] + [
    Spec(*SHAPES[2], family="random", flags="holes"), Spec(*SHAPES[1], family="constructed", flags="holes"),
    Spec(*SHAPES[1], family="random", flags="full"),
    Spec(*SHAPES[1], family="constructed", variant="no_weight"), Spec(*SHAPES[4], family="random", variant="no_weight"),
    Spec(*SHAPES[2], family="constructed", variant="no_sigma"), Spec(*SHAPES[3], family="random", variant="no_sigma"),
    Spec(*SHAPES[1], family="random", variant="iou_w0"), Spec(*SHAPES[2], family="constructed", variant="iou_w0"),
]


def make_flags(B, N, kind, rng):
    f = np.zeros((B, N), np.uint8)
    for b in range(B):
        if kind == "full" or N == 1:
            f[b] = 1
        elif kind == "ragged":   # prefixes: all, one, and lengths in between
            f[b, :(N, 1, (N + 1) // 2, N - 1)[b % 4]] = 1
        else:                    # holes, the first and the last node among them in some graph
            f[b] = rng.random(N) < 0.6
            f[b, b % N] = 1
            f[b, 0 if b % 2 else N - 1] = 0
    assert f.sum(-1).min() >= 1
    return f


class Case:
    pass


def _random_boxes(rng, tgt_node, pred_node, flags):
    """a family like synth.iou_case's: target channels in (-0.8, 0.8), predictions spread wide enough to leave [0, 1], to miss and to
    enclose their targets; a valid node whose box comes within MARGIN of a branch, or is thinner than MIN_EXTENT, is drawn again"""
    B, N = flags.shape
    todo = np.ones((B, N), bool)
    for _ in range(100):
        k = int(todo.sum())
        if k == 0:
            return
        t4 = ((2.0 * rng.random((k, 4)) - 1.0) * 0.8).astype(np.float32)
        p4 = t4 + np.float32(0.7) * rng.standard_normal((k, 4)).astype(np.float32)
        p4[:, 2:] = np.maximum(p4[:, 2:], np.float32(-0.9))
        p4[:, :2] = np.clip(p4[:, :2], np.float32(-0.85), np.float32(0.85))
        tgt_node[todo, -4:], pred_node[todo, -4:] = t4, p4
        _, gap, extent = box_events(pred_node, tgt_node, np.ones((B, N), bool))
        todo = ((gap <= MARGIN) | (extent < MIN_EXTENT)).reshape(B, N)
    raise AssertionError("no draw keeps every comparison apart")


@functools.lru_cache(maxsize=None)
def make_case(spec):
    rng = np.random.default_rng(1000 + SPECS.index(spec))
    B, N, Ca, Cn = spec.B, spec.N, spec.Ca, spec.Cn
    c = Case()
    c.spec, c.name = spec, spec.name
    c.flags = make_flags(B, N, spec.flags, rng)
    c.tgt_adj = np.sign(rng.standard_normal((B, Ca, N, N))).astype(np.float32)
    c.pred_adj = (c.tgt_adj + 0.4 * rng.standard_normal((B, Ca, N, N))).astype(np.float32)
    c.tgt_node = np.sign(rng.standard_normal((B, N, Cn))).astype(np.float32)
    c.pred_node = (c.tgt_node + 0.4 * rng.standard_normal((B, N, Cn))).astype(np.float32)
    if spec.family == "random":
        _random_boxes(rng, c.tgt_node, c.pred_node, c.flags)
    else:   # the constructed boxes in turn over the VALID nodes, starting at another one in every case
        k = SPECS.index(spec) * 7
        for b in range(B):
            for i in range(N):
                what, p, g = CONSTRUCTED[k % len(CONSTRUCTED)]
                c.pred_node[b, i, -4:], c.tgt_node[b, i, -4:] = _channels(p), _channels(g)
                k += int(c.flags[b, i])
    c.weights = None if spec.variant == "no_weight" else (0.5 + 2.0 * rng.random(B)).astype(np.float32)
    c.sigmas = None if spec.variant == "no_sigma" else np.exp(1.2 * rng.standard_normal(B) - 1.2).astype(np.float32)
    c.edge_w, c.node_w, c.iou_w = EDGE_W, NODE_W, (0.0 if spec.variant == "iou_w0" else IOU_W)
    # the objective's replayed draws at the same shape
    c.rnd = rng.standard_normal(B).astype(np.float32)
    c.eps_adj = rng.standard_normal((B, Ca, N, N)).astype(np.float32)
    c.eps_node = rng.standard_normal((B, N, Cn)).astype(np.float32)
    for a in (c.flags, c.tgt_adj, c.pred_adj, c.tgt_node, c.pred_node, c.weights, c.sigmas, c.rnd, c.eps_adj, c.eps_node):
        if a is not None:
            a.setflags(write=False)
    return c


def cases():
    return [make_case(s) for s in SPECS]


CASE_IDS = [s.name for s in SPECS]


@functools.lru_cache(maxsize=None)
def _reference(spec, iou_type, f32):
    return evaluate(make_case(spec), iou_type, torch.float32 if f32 else torch.float64)


def reference(case, iou_type, f32=False):
    """the shared, cached reference of a case: computed once, never written to"""
    return _reference(case.spec, iou_type, bool(f32))


@functools.lru_cache(maxsize=None)
def bars():
    """family -> (bar, float32 discrepancy): 16 x the largest difference between the float32 and the float64 evaluation of this reference
    over the RANDOM cases (relative to the family's largest magnitude in the case; 16 is the margin tests/test_ode.py uses over a
    reference's own float32 error), never looser than the bars of the fixture test.  The constructed cases use the same bars: their
    own float32 discrepancy is zero by construction and sets none."""
    disc = dict.fromkeys(FAMILIES, 0.0)
    for spec in SPECS:
        if spec.family != "random":
            continue
        for ty in IOU_TYPES:
            a, b = split_families(_reference(spec, ty, True)), split_families(_reference(spec, ty, False))
            for fam in FAMILIES:
                if b[fam] is not None and np.abs(b[fam]).max() > 0:
                    disc[fam] = max(disc[fam], rel_err(a[fam], b[fam]))
    return {fam: (min(16.0 * disc[fam], FLOOR[fam]), disc[fam]) for fam in FAMILIES}


def compare(got, ref):
    """got, ref: dicts of outputs (None = not produced) -> {family: worst |err| / bar}; the caller asserts <= 1"""
    worst = {}
    for key, r in ref.items():
        assert (got[key] is None) == (r is None), key
        if r is None:
            continue
        for fam, sel in family_of_output(key):
            rr = sel(r)
            if rr.size == 0:
                continue
            g = sel(np.asarray(got[key], np.float64).reshape(r.shape))
            assert np.isfinite(g).all(), f"{key}: non-finite values"
            worst[fam] = max(worst.get(fam, 0.0), rel_err(g, rr) / bars()[fam][0])
    return worst


# ----------------------------------------------------------------------------------------------------------------------------------
# dsg_train_inputs with replayed draws
# ----------------------------------------------------------------------------------------------------------------------------------
F32 = np.float32


def sigma_reference(rnd):
    """exp in float64 of the float32-rounded argument fl(fl(r * 1.2) + (-1.2))"""
    arg = (np.asarray(rnd, F32) * F32(1.2)) + F32(-1.2)
    assert arg.dtype == F32
    return np.exp(arg.astype(np.float64))


def train_inputs_from_sigmas(case, sigmas, fused=False):
    """weights, noisy_adj, noisy_node in float32 operation by operation from GIVEN float32 sigmas:
    fl(fl(s s) + 0.25) / fl(fl(0.5 s)^2) and fl(clean + fl(eps s)); invalid adjacency entries 0, invalid node entries the clean value.
    fused (the mistake: a contracted multiply-add): the product unrounded, one rounding at the end"""
    s = np.asarray(sigmas, F32)
    f = case.flags.astype(bool)
    fa = f[:, None, :, None] & f[:, None, None, :]
    sd = s * F32(0.5)
    if fused:
        w = ((s.astype(np.float64) * s + 0.25).astype(F32) / (sd * sd)).astype(F32)
        na = (case.tgt_adj.astype(np.float64) + case.eps_adj.astype(np.float64) * s[:, None, None, None]).astype(F32)
        nx = (case.tgt_node.astype(np.float64) + case.eps_node.astype(np.float64) * s[:, None, None]).astype(F32)
    else:
        w = (s * s + F32(0.25)) / (sd * sd)
        na = case.tgt_adj + case.eps_adj * s[:, None, None, None]
        nx = case.tgt_node + case.eps_node * s[:, None, None]
    assert w.dtype == na.dtype == nx.dtype == F32
    return w, np.where(fa, na, F32(0.0)), np.where(f[:, :, None], nx, case.tgt_node)


def ulp_err(got, ref64):
    """|got - ref| in units of the float32 spacing at ref"""
    return np.abs(np.asarray(got, np.float64) - ref64) / np.spacing(np.abs(ref64).astype(F32)).astype(np.float64)
