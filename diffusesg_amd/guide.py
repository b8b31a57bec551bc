"""Loss-guided sampling on top of `NodeAdjPrecondHip.value_and_input_grad` (`dsg_precond_vjp`), and three ready-made box losses.

`guided_sample` is an eager reverse loop for the solvers 'euler', 'heun' and 'dpmpp_2m' built from the library's own pieces: the
schedule of `dsg_sigma_schedule`, the Philox noise streams of `device_noise`, the coin draws of the sampler and the multistep
coefficients of `dsg_multistep_coef`.  The state algebra is torch float32 elementwise arithmetic on the device, written operation by
operation like the loop kernels of the library, so that with scale = 0 the loop is `sampler.sample` up to the difference between the
training-form and the sampling-form forward.

Per preconditioned call the denoised estimate is shifted against the gradient of the loss,

    D~ = D - w_i * t_hat^2 * mask(grad_{x_hat} L(D(x_hat, t_hat)))

which is the score identity  grad log p_t(x) = (D - x) / t^2  with  -grad L  added to the score.  No trained weights ship with the
project: what guidance does to sample quality is not validated here.

The losses read boxes the way `io.decode` does: the last four node channels, * 0.5 + 0.5, (cx, cy, w, h).  They are plain torch and
run on any device.

`box_relation_loss` is the fourth: a pairwise loss on box pairs that makes them agree with the spatial relation between them, the
pairs and their kinds given as a matrix or decoded from the adjacency estimate through a predicate -> kind table (`SpatialRules`).

`BoxGuide` names a weighted sum of the box losses for the guidance that runs INSIDE the library's loop
(`NodeAdjEDMSamplerHip.sample_guided`, `dsg_sample_guided`): the same shift with the network's Jacobian dropped from
grad_{x_hat} L(D) = (c_skip I + c_out dF/dx_hat)^T dL/dD, evaluated by a HIP kernel with analytic gradients -- no backward, no
training-form forward, step graphs and walks as in `sample()`.  It is an approximation of the shift above, exact only where the
network's Jacobian vanishes; `BoxGuide.torch_loss` hands the same loss to `guided_sample`, the through-the-network form.

`ContentGuide` is the in-loop guide of the label and predicate channels (`sample_guided(content=...)`, `dsg_sample_guided_content`,
DESIGN.md §17): "samples that contain these triplets", a soft minimum over all node slots; `content_loss` is its torch form,
`label_codes` the value-space codes it aims at, `items_present` the check on decoded graphs.
"""
from __future__ import annotations

import numpy as np
import torch

from . import lib as _lib
from .model import NodeAdjPrecondHip
from .sampler import check_graph_seeds

SOLVERS = ("euler", "heun", "dpmpp_2m")


# ---- losses ---------------------------------------------------------------------------------------------------------
def _boxes(D_node):
    """[B, N, 4] (cx, cy, w, h) in [0, 1] from the node estimate [B, N, C_node] (io.decode: last four channels * 0.5 + 0.5)"""
    if D_node.dim() != 3 or D_node.shape[-1] < 4:
        raise ValueError(f"box losses need a node tensor [B, N, C_node >= 4], got {tuple(D_node.shape)}")
    return D_node[..., -4:] * 0.5 + 0.5


def _corners(b):
    return b[..., 0] - 0.5 * b[..., 2], b[..., 1] - 0.5 * b[..., 3], b[..., 0] + 0.5 * b[..., 2], b[..., 1] + 0.5 * b[..., 3]


def box_region_loss(node_idx, region, node_flags=None):
    """Squared hinge that pulls the box of node `node_idx` (an index, or a list of them) inside the rectangle region = (x0, y0, x1, y1)
    in [0, 1] coordinates: the sum over graphs and the four sides of relu(overshoot)^2.  `node_flags` [B, N] (optional): graphs in
    which the node is padding contribute nothing."""
    x0, y0, x1, y1 = (float(v) for v in region)
    if not (x0 < x1 and y0 < y1):
        raise ValueError(f"box_region_loss: empty region {region}")
    idx = [int(node_idx)] if isinstance(node_idx, (int, np.integer)) else [int(k) for k in node_idx]
    if not idx or min(idx) < 0:
        raise ValueError(f"box_region_loss: bad node index {node_idx}")

    def loss(D_adj, D_node):
        b = _boxes(D_node)
        if max(idx) >= b.shape[1]:
            raise ValueError(f"box_region_loss: node index {max(idx)} is outside the {b.shape[1]} nodes")
        b = b[:, idx]
        l, t, r, bt = _corners(b)
        over = torch.relu(x0 - l) ** 2 + torch.relu(y0 - t) ** 2 + torch.relu(r - x1) ** 2 + torch.relu(bt - y1) ** 2
        if node_flags is not None:
            over = over * node_flags.to(device=over.device)[:, idx].to(over.dtype)
        return over.sum()
    return loss


def box_overlap_loss(node_flags=None):
    """Sum over graphs and unordered pairs of valid nodes of the intersection area of their boxes (negative extents clamped to 0):
    the differentiable form of the evaluator's overlap metric.  `node_flags` [B, N] (optional): padded nodes take no part; without it
    every node does (the denoised estimate of a padded node is all zeros, a box of extent 0.5 at the centre)."""
    def loss(D_adj, D_node):
        b = _boxes(D_node)
        l, t, r, bt = _corners(b)
        iw = torch.relu(torch.minimum(r[:, :, None], r[:, None, :]) - torch.maximum(l[:, :, None], l[:, None, :]))
        ih = torch.relu(torch.minimum(bt[:, :, None], bt[:, None, :]) - torch.maximum(t[:, :, None], t[:, None, :]))
        area = iw * ih
        n = b.shape[1]
        pair = torch.triu(torch.ones(n, n, dtype=torch.bool, device=b.device), diagonal=1)
        if node_flags is not None:
            f = node_flags.to(device=b.device).bool()
            pair = pair[None] & f[:, :, None] & f[:, None, :]
        return (area * pair.to(area.dtype)).sum()
    return loss


def box_alignment_loss(node_flags=None, tau=0.05):
    """Alignment of a layout: for every valid node and each of the six lines (left, centre x, right, top, centre y, bottom), a soft
    minimum over the other nodes of the squared distance between the same lines, summed.  The soft minimum is
    -tau log sum_j exp(-d_ij^2 / tau) + tau log(n - 1): 0 for a node whose line coincides with every other node's, and close to the
    squared distance to the nearest one when tau is small against it."""
    tau = float(tau)
    if tau <= 0:
        raise ValueError("box_alignment_loss: tau must be positive")

    def loss(D_adj, D_node):
        b = _boxes(D_node)
        l, t, r, bt = _corners(b)
        lines = torch.stack([l, b[..., 0], r, t, b[..., 1], bt], dim=1)          # [B, 6, N]
        d2 = (lines[..., :, None] - lines[..., None, :]) ** 2                    # [B, 6, N, N]
        n = b.shape[1]
        other = ~torch.eye(n, dtype=torch.bool, device=b.device)
        valid = torch.ones(b.shape[:2], dtype=torch.bool, device=b.device) if node_flags is None else node_flags.to(device=b.device).bool()
        pair = (other[None] & valid[:, :, None] & valid[:, None, :])[:, None]    # [B, 1, N, N]
        cnt = pair.sum(-1).clamp(min=1).to(d2.dtype)                             # [B, 1, N]
        z = torch.where(pair, -d2 / tau, torch.full_like(d2, -float("inf")))
        has = pair.any(-1)
        z = torch.where(has[..., None], z, torch.zeros_like(z))                  # rows without a partner: finite, dropped below
        soft = -tau * torch.logsumexp(z, dim=-1) + tau * torch.log(cnt)
        return (soft * has.to(soft.dtype)).sum()
    return loss


def box_region_loss_nodes(sel, rects, node_flags=None):
    """`box_region_loss` with one rectangle per node: sel [B, N] (bool or integer, nonzero = the node is constrained), rects [B, N, 4]
    (x0, y0, x1, y1); the sum over selected (and, with `node_flags`, valid) nodes of the four squared overshoots."""
    def loss(D_adj, D_node):
        b = _boxes(D_node)
        if tuple(sel.shape) != tuple(b.shape[:2]) or tuple(rects.shape) != tuple(b.shape[:2]) + (4,):
            raise ValueError(f"box_region_loss_nodes: sel {tuple(sel.shape)} / rects {tuple(rects.shape)} do not fit nodes {tuple(b.shape[:2])}")
        l, t, r, bt = _corners(b)
        rc = rects.to(device=b.device, dtype=b.dtype)
        over = torch.relu(rc[..., 0] - l) ** 2 + torch.relu(rc[..., 1] - t) ** 2 + torch.relu(r - rc[..., 2]) ** 2 + torch.relu(bt - rc[..., 3]) ** 2
        on = sel.to(device=b.device) != 0
        if node_flags is not None:
            on = on & node_flags.to(device=b.device).bool()
        return torch.where(on, over, torch.zeros_like(over)).sum()
    return loss


# ---- spatial relations between node pairs -----------------------------------------------------------
# The kind of an ordered pair (subject i = the row, object j = the column of a kind matrix); DSG_REL_* of include/dsg.h
REL_NONE, REL_LEFT_OF, REL_RIGHT_OF, REL_ABOVE, REL_BELOW, REL_INSIDE, REL_CONTAINS, REL_ON = range(8)
REL_KINDS = 8


class SpatialRules(object):
    """A predicate -> kind table for relation guidance whose kinds are DECODED from the adjacency estimate at every preconditioned call:
    pred_kind [n_adj_type] integers in 0..7 (the REL_* constants), `encoding` the run's edge encoding ('bits' | 'one_hot' | 'ddpm').
    Which predicate means what is the caller's knowledge of the dataset's vocabulary; no table ships with the project."""

    def __init__(self, pred_kind, n_adj_type, encoding="bits"):
        if encoding not in _lib.ENCODINGS:
            raise ValueError(f"SpatialRules: encoding should be 'bits', 'one_hot' or 'ddpm', got {encoding!r}")
        self.n_adj_type, self.encoding = int(n_adj_type), encoding
        if self.n_adj_type < 1:
            raise ValueError(f"SpatialRules: n_adj_type = {n_adj_type} must be >= 1")
        t = np.asarray(pred_kind.detach().cpu().numpy() if isinstance(pred_kind, torch.Tensor) else pred_kind)
        if t.shape != (self.n_adj_type,) or not np.issubdtype(t.dtype, np.integer):
            raise ValueError(f"SpatialRules: pred_kind must hold {self.n_adj_type} integers (one kind per predicate), got shape {t.shape} {t.dtype}")
        if t.min() < 0 or t.max() >= REL_KINDS:
            raise ValueError(f"SpatialRules: pred_kind holds a kind outside 0..{REL_KINDS - 1}")
        self.pred_kind = np.ascontiguousarray(t, dtype=np.uint8)


def _live_pairs(node_flags, B, n, device):
    """[B, N, N] bool: both nodes valid, off the diagonal"""
    off = ~torch.eye(n, dtype=torch.bool, device=device)
    if node_flags is None:
        return off[None].expand(B, n, n)
    f = node_flags.to(device=device) != 0
    return off[None] & f[:, :, None] & f[:, None, :]


def _decode_predicates(D_adj, rules):
    """[B, N, N] int64 predicates of the adjacency estimate [B, C_adj, N, N] ([B, N, N]: one channel) by `dsg_decode`'s rule for the
    encoding, evaluated on the float32 value as the library holds it; -1 where the ddpm rule meets a NaN"""
    a = D_adj.detach().to(torch.float32)
    if a.dim() == 3:
        a = a[:, None]
    C, k = a.shape[1], rules.n_adj_type
    if rules.encoding == "bits":
        if C > 30 or (1 << C) < k:
            raise ValueError(f"decoded relations: {k} predicates in bits do not fit {C} adjacency channels")
        w = torch.tensor([1 << (C - 1 - c) for c in range(C)], dtype=torch.int64, device=a.device)
        return ((a > 0).to(torch.int64) * w[None, :, None, None]).sum(1).clamp(max=k - 1)   # MSB first, clamped
    if rules.encoding == "one_hot":
        if C != k:
            raise ValueError(f"decoded relations: one_hot needs one adjacency channel per predicate, got {C} channels for {k}")
        return torch.argmax((a > 0).to(torch.int64), dim=1)   # the first positive channel, 0 when none is
    if C != 1:
        raise ValueError(f"decoded relations: ddpm needs one adjacency channel, got {C}")
    x = a[:, 0].clamp(-1.0, 1.0)
    out = torch.full(x.shape, -1, dtype=torch.int64, device=a.device)
    L = 2.0 / (k - 1) if k > 1 else float("inf")   # Python floats: double, like the reference's
    for i in range(k):
        center = -1.0 + i * L if k > 1 else -1.0
        lo = -float("inf") if i == 0 else float(np.float32(center - L * 0.5))
        hi = float("inf") if i == k - 1 else float(np.float32(center + L * 0.5))
        out = torch.where((x > lo) & (x <= hi), torch.full_like(out, i), out)   # ascending, the last match wins; NaN matches nothing
    return out


def relation_kinds_from_graph(q_adj, node_flags, pred_kind):
    """uint8 [B, N, N] kinds of an integer graph: pred_kind[q_adj] at live pairs (both nodes valid, off the diagonal), REL_NONE
    elsewhere and where the predicate is outside the table.  pred_kind: a sequence of kinds, or a `SpatialRules`."""
    table = pred_kind.pred_kind if isinstance(pred_kind, SpatialRules) else np.asarray(pred_kind)
    q = torch.as_tensor(q_adj)
    if q.dim() != 3 or q.shape[1] != q.shape[2]:
        raise ValueError(f"relation_kinds_from_graph: q_adj must be [B, N, N], got {tuple(q.shape)}")
    t = torch.as_tensor(np.ascontiguousarray(table, dtype=np.uint8), device=q.device)
    q = q.to(torch.int64)
    ok = (q >= 0) & (q < t.numel()) & _live_pairs(node_flags, q.shape[0], q.shape[1], q.device)
    return torch.where(ok, t[q.clamp(0, t.numel() - 1)], torch.zeros((), dtype=torch.uint8, device=q.device))


def decoded_relation_kinds(D_adj, node_flags, rules):
    """uint8 [B, N, N]: the kinds the guide kernel's decoded source uses on this adjacency estimate -- every live entry decoded to a
    predicate by the rule of `rules.encoding`, then `rules.pred_kind[predicate]`.  No gradient: the kinds are constants of the call."""
    if not isinstance(rules, SpatialRules):
        raise TypeError("decoded_relation_kinds needs a SpatialRules")
    with torch.no_grad():
        return relation_kinds_from_graph(_decode_predicates(D_adj, rules), node_flags, rules)


def _check_kinds(kinds, who):
    k = torch.as_tensor(kinds)
    if k.dim() != 3 or k.shape[1] != k.shape[2] or k.dtype.is_floating_point or k.dtype == torch.bool:
        raise ValueError(f"{who}: kinds must be an integer tensor [B, N, N], got {tuple(k.shape)} {k.dtype}")
    if k.numel() and (int(k.min()) < 0 or int(k.max()) >= REL_KINDS):
        raise ValueError(f"{who}: kinds holds an entry outside 0..{REL_KINDS - 1}")
    return k


def box_relation_loss(kinds, node_flags=None, margin=0.0):
    """Agreement of box pairs with the spatial relation between them: the sum over graphs and ORDERED pairs (subject i, object j),
    i != j, of a squared hinge h(v) = relu(v)^2 chosen by kinds[b, i, j] (boxes (cx, cy, w, h), lines l, r, t, bt; y grows downwards):
        LEFT_OF h(cx_i - cx_j + m)   RIGHT_OF h(cx_j - cx_i + m)   ABOVE h(cy_i - cy_j + m)   BELOW h(cy_j - cy_i + m)
        INSIDE  h(l_j - l_i) + h(r_i - r_j) + h(t_j - t_i) + h(bt_i - bt_j)       CONTAINS: INSIDE with i and j exchanged
        ON      (bt_i - t_j)^2 + h(l_j - cx_i) + h(cx_i - r_j)
    kinds: an integer tensor [B, N, N] of REL_* constants, or a `SpatialRules` -- then the kinds are recomputed from D_adj at every
    call (`decoded_relation_kinds`), under no_grad.  margin m >= 0; `node_flags` [B, N] (optional): padded nodes take no part."""
    m = float(margin)
    if not (m >= 0 and np.isfinite(m)):
        raise ValueError(f"box_relation_loss: margin = {margin} must be >= 0 and finite")
    rules = kinds if isinstance(kinds, SpatialRules) else None
    given = None if rules is not None else _check_kinds(kinds, "box_relation_loss")

    def loss(D_adj, D_node):
        b = _boxes(D_node)
        B, n = b.shape[:2]
        if rules is not None:
            if D_adj is None:
                raise ValueError("box_relation_loss: decoded kinds need D_adj")
            K = decoded_relation_kinds(D_adj, node_flags, rules).to(b.device)
        else:
            K = given.to(b.device)
        if tuple(K.shape) != (B, n, n):
            raise ValueError(f"box_relation_loss: kinds {tuple(K.shape)} do not fit nodes {(B, n)}")
        K = torch.where(_live_pairs(node_flags, B, n, b.device), K.to(torch.int64), torch.zeros((), dtype=torch.int64, device=b.device))
        l, t, r, bt = _corners(b)
        cx, cy = b[..., 0], b[..., 1]
        S, O = (lambda v: v[:, :, None]), (lambda v: v[:, None, :])   # the subject's / the object's line on the [B, i, j] grid
        h = lambda v: torch.relu(v) ** 2
        inside = lambda I, J: h(J(l) - I(l)) + h(I(r) - J(r)) + h(J(t) - I(t)) + h(I(bt) - J(bt))
        terms = {REL_LEFT_OF: lambda: h(S(cx) - O(cx) + m), REL_RIGHT_OF: lambda: h(O(cx) - S(cx) + m),
                 REL_ABOVE: lambda: h(S(cy) - O(cy) + m), REL_BELOW: lambda: h(O(cy) - S(cy) + m),
                 REL_INSIDE: lambda: inside(S, O), REL_CONTAINS: lambda: inside(O, S),
                 REL_ON: lambda: (S(bt) - O(t)) ** 2 + h(O(l) - S(cx)) + h(S(cx) - O(r))}
        total = b.sum() * 0.0
        for kind, term in terms.items():
            on = K == kind
            if bool(on.any()):
                v = term()
                total = total + torch.where(on, v, torch.zeros_like(v)).sum()
        return total
    return loss


class BoxGuide(object):
    """L = overlap * L_overlap + region_weight * L_region + align * L_align + relation_weight * L_rel on the boxes of the node estimate,
    always with the node flags (padded nodes take no part): the loss of in-loop guidance (`NodeAdjEDMSamplerHip.sample_guided`).
      overlap, align: weights of `box_overlap_loss` / `box_alignment_loss(tau=tau)`; 0 = the term is not evaluated.
      region: None, or (sel [B, N], rects [B, N, 4]) -- one rectangle (x0, y0, x1, y1) per selected node, `box_region_loss_nodes` --
              or (node_idx, rect) -- `box_region_loss`'s form: the same rectangle for that node (or those nodes) in every graph.
      region_weight: weight of the region term where `region` is given.
      relations: None, an integer tensor [B, N, N] of REL_* kinds (subject = row, object = column), or a `SpatialRules` -- the kinds are
              then decoded on the device from the adjacency estimate of every call; `box_relation_loss` with `relation_margin`.
      relation_weight: weight of the relation term where `relations` is given."""

    def __init__(self, overlap=0.0, region=None, align=0.0, tau=0.05, region_weight=1.0, relations=None, relation_weight=1.0,
                 relation_margin=0.0):
        self.overlap, self.align, self.tau = float(overlap), float(align), float(tau)
        self.region_weight = float(region_weight) if region is not None else 0.0
        self.relation_weight = float(relation_weight) if relations is not None else 0.0
        self.relation_margin = float(relation_margin)
        for name, v in (("overlap", self.overlap), ("align", self.align), ("region_weight", self.region_weight), ("tau", self.tau),
                        ("relation_weight", self.relation_weight)):
            if not np.isfinite(v):
                raise ValueError(f"BoxGuide: {name} = {v} is not finite")
        if self.align != 0 and not self.tau > 0:
            raise ValueError("BoxGuide: tau must be positive")
        if not (self.relation_margin >= 0 and np.isfinite(self.relation_margin)):
            raise ValueError(f"BoxGuide: relation_margin = {relation_margin} must be >= 0 and finite")
        self.relations = None
        if relations is not None:
            self.relations = relations if isinstance(relations, SpatialRules) else _check_kinds(relations, "BoxGuide")
        self.region = None
        if region is not None:
            if len(region) != 2:
                raise ValueError("BoxGuide: region = (sel [B, N], rects [B, N, 4]) or (node_idx, (x0, y0, x1, y1))")
            a, r = region
            if isinstance(a, (torch.Tensor, np.ndarray)) and np.ndim(a) == 2:
                self.region = ("nodes", torch.as_tensor(a), torch.as_tensor(r).to(torch.float32))
            else:
                idx = [int(a)] if isinstance(a, (int, np.integer)) else [int(k) for k in a]
                x0, y0, x1, y1 = (float(v) for v in r)
                if not (x0 < x1 and y0 < y1):
                    raise ValueError(f"BoxGuide: empty region {r}")
                if not idx or min(idx) < 0:
                    raise ValueError(f"BoxGuide: bad node index {a}")
                self.region = ("index", idx, (x0, y0, x1, y1))

    def region_tensors(self, B, n, device="cpu"):
        """(sel uint8 [B, n], rects float32 [B, n, 4]) of the region term on `device`, None without one; ValueError on a shape that
        does not fit the batch."""
        if self.region is None:
            return None
        if self.region[0] == "nodes":
            sel, rc = self.region[1], self.region[2]
            if tuple(sel.shape) != (B, n) or tuple(rc.shape) != (B, n, 4):
                raise ValueError(f"BoxGuide: region sel {tuple(sel.shape)} / rects {tuple(rc.shape)}, expected ({B}, {n}) / ({B}, {n}, 4)")
            return (sel != 0).to(device=device, dtype=torch.uint8).contiguous(), rc.to(device=device, dtype=torch.float32).contiguous()
        _, idx, rect = self.region
        if max(idx) >= n:
            raise ValueError(f"BoxGuide: node index {max(idx)} is outside the {n} nodes")
        sel = torch.zeros((B, n), dtype=torch.uint8)
        sel[:, idx] = 1
        rc = torch.zeros((B, n, 4), dtype=torch.float32)
        rc[:, idx] = torch.tensor(rect, dtype=torch.float32)
        return sel.to(device), rc.to(device)

    def descriptor(self, B, n, device, clip_ratio=1.0):
        """(`lib.DsgGuideCfg` without its weights, the device tensors it points at -- keep them alive over the call)"""
        reg = self.region_tensors(B, n, device)
        clip = _lib.GUIDE_CLIP_NONE if clip_ratio is None else float(clip_ratio)
        g = _lib.DsgGuideCfg(self.overlap, self.region_weight, self.align, self.tau, clip, 0,
                             None if reg is None else reg[0].data_ptr(), None if reg is None else reg[1].data_ptr(), None)
        return g, reg

    def relation_descriptor(self, B, n, device, c_adj):
        """(`lib.DsgRelCfg`, what it points at -- keep it alive over the call) of the relation term, (None, None) without one;
        ValueError on kinds that do not fit the batch or a table that does not fit the adjacency channels."""
        if self.relations is None:
            return None, None
        if isinstance(self.relations, SpatialRules):
            r = self.relations
            C, k = int(c_adj), r.n_adj_type
            if (r.encoding == "one_hot" and C != k) or (r.encoding == "ddpm" and C != 1) or (r.encoding == "bits" and (C > 30 or (1 << C) < k)):
                raise ValueError(f"BoxGuide: relations in {r.encoding} with {k} predicates do not fit {C} adjacency channels")
            return _lib.DsgRelCfg(self.relation_weight, self.relation_margin, _lib.REL_DECODED, _lib.ENCODINGS[r.encoding], k, 0, None,
                                  r.pred_kind.ctypes.data), r.pred_kind
        if tuple(self.relations.shape) != (B, n, n):
            raise ValueError(f"BoxGuide: relations {tuple(self.relations.shape)}, expected ({B}, {n}, {n})")
        kd = self.relations.to(device=device, dtype=torch.uint8).contiguous()
        return _lib.DsgRelCfg(self.relation_weight, self.relation_margin, _lib.REL_GIVEN, 0, 0, 0, kd.data_ptr(), None), kd

    def torch_loss(self, node_flags):
        """The same loss as a `guide.py` closure loss(D_adj, D_node) -> scalar, for `guided_sample` and the tests."""
        terms = []
        if self.overlap != 0:
            terms.append((self.overlap, box_overlap_loss(node_flags)))
        if self.region is not None and self.region_weight != 0:
            if self.region[0] == "nodes":
                terms.append((self.region_weight, box_region_loss_nodes(self.region[1], self.region[2], node_flags)))
            else:
                terms.append((self.region_weight, box_region_loss(self.region[1], self.region[2], node_flags)))
        if self.align != 0:
            terms.append((self.align, box_alignment_loss(node_flags, self.tau)))
        if self.relations is not None and self.relation_weight != 0:
            terms.append((self.relation_weight, box_relation_loss(self.relations, node_flags, self.relation_margin)))

        def loss(D_adj, D_node):
            total = _boxes(D_node).sum() * 0.0
            for wgt, fn in terms:
                total = total + fn(D_adj, D_node) * wgt
            return total
        return loss


# ---- content guidance: samples that contain given triplets -------------------------------------------
def label_codes(n_type, encoding, chans):
    """float32 [n_type, chans]: the value-space code of every integer label 0..n_type-1 under `encoding`, `dsg_encode`'s three rules --
    'bits': the MSB-first binary digits b of the label over `chans` channels, 2 b - 1; 'one_hot': 2 onehot - 1 over chans = n_type
    channels; 'ddpm': 2 i / (n_type - 1) - 1 in one channel, float32 operation by operation."""
    n_type, chans = int(n_type), int(chans)
    if n_type < 1 or chans < 1:
        raise ValueError(f"label_codes: n_type = {n_type} and chans = {chans} must be >= 1")
    q = np.arange(n_type, dtype=np.int64)
    if encoding == "bits":
        if chans > 30 or (1 << chans) < n_type:
            raise ValueError(f"label_codes: {n_type} labels do not fit {chans} bits")
        b = (q[:, None] >> (chans - 1 - np.arange(chans))[None, :]) & 1
        return np.where(b != 0, np.float32(1), np.float32(-1)).astype(np.float32)
    if encoding == "one_hot":
        if chans != n_type:
            raise ValueError(f"label_codes: one_hot needs chans = n_type, got {chans} and {n_type}")
        return np.where(np.eye(n_type, dtype=bool), np.float32(1), np.float32(-1)).astype(np.float32)
    if encoding == "ddpm":
        if chans != 1 or n_type < 2:
            raise ValueError(f"label_codes: ddpm needs one channel and at least two labels, got {chans} and {n_type}")
        v = (2 * q).astype(np.float32) / np.float32(n_type - 1) - np.float32(1)
        return v.astype(np.float32)[:, None]
    raise ValueError("encoding should be 'ddpm', 'bits' or 'one_hot'")


def _code_chans(n_type, encoding, chans, what):
    """the channel count `encoding` implies for n_type labels in a tensor with `chans` channels for them; ValueError if it does not fit"""
    if (encoding == "one_hot" and chans != n_type) or (encoding == "ddpm" and chans != 1) or \
            (encoding == "bits" and (chans < 1 or chans > 30 or (1 << chans) < n_type)):
        raise ValueError(f"ContentGuide: {n_type} {what} in {encoding} do not fit {chans} channels")
    return chans


def content_loss(subj, obj, pred, w_spo, node_flags, tau):
    """L_content as a differentiable torch closure loss(D_adj, D_node) -> scalar (the through-the-network form of content guidance):
    subj / obj [B, K, Cl], pred [B, K, C_adj] targets in value space, w_spo [B, K, 3] = (a_s, a_o, a_p) >= 0.  Per graph and item the soft
    minimum -tau log mean exp(-d / tau) over the live ordered pairs (i != j, both valid) of
        d(i, j) = a_s |D_node[i, :Cl] - s|^2 + a_o |D_node[j, :Cl] - o|^2 + a_p |D_adj[:, i, j] - p|^2,
    summed over active items (a weight > 0) and graphs; a graph without a live pair adds exactly 0.  Entries that are not live are
    selected away before they are read."""
    tau = float(tau)
    if not tau > 0:
        raise ValueError("content_loss: tau must be positive")
    subj, obj, pred, w_spo = (torch.as_tensor(v) for v in (subj, obj, pred, w_spo))
    Cl = subj.shape[-1]

    def loss(D_adj, D_node):
        dt, dv = D_node.dtype, D_node.device
        s, o, p, a = (v.to(device=dv, dtype=dt) for v in (subj, obj, pred, w_spo))
        n = D_node.shape[1]
        f = node_flags.to(device=dv).bool()
        live = f[:, :, None] & f[:, None, :] & ~torch.eye(n, dtype=torch.bool, device=dv)[None]          # [B, N, N]
        zero = torch.zeros((), dtype=dt, device=dv)
        Dn = torch.where(f[:, :, None], D_node[..., :Cl], zero)
        Da = torch.where(live[:, None], D_adj, zero)
        ds = ((Dn[:, None] - s[:, :, None]) ** 2).sum(-1)                                                 # [B, K, N]
        do = ((Dn[:, None] - o[:, :, None]) ** 2).sum(-1)
        dp = torch.stack([((Da - p[:, k, :, None, None]) ** 2).sum(1) for k in range(p.shape[1])], dim=1)  # [B, K, N, N]
        d = a[:, :, 0, None, None] * ds[:, :, :, None] + a[:, :, 1, None, None] * do[:, :, None, :] + a[:, :, 2, None, None] * dp
        cnt = live.flatten(1).sum(1)
        has = cnt > 0
        z = torch.where(live[:, None], -d / tau, torch.full_like(d, -float("inf")))
        z = torch.where(has[:, None, None, None], z, torch.zeros_like(z))     # graphs without a pair: finite, dropped below
        soft = -tau * (torch.logsumexp(z.flatten(2), dim=-1) - torch.log(cnt.clamp(min=1).to(dt))[:, None])   # [B, K]
        on = (a.sum(-1) > 0) & has[:, None]
        return torch.where(on, soft, torch.zeros_like(soft)).sum()
    return loss


class ContentGuide(object):
    """"Samples that contain these triplets": the loss of content guidance inside the library's loop (`sample_guided(content=...)`,
    `dsg_sample_guided_content`) -- a soft minimum over all node slots on the label and predicate channels, so that the
    caller names labels, never slots.
      items: per graph a list of (subject_label | None, predicate | None, object_label | None), integers as `io.encode` takes them;
             None drops that term: (l, None, None) is "some node has label l", (None, p, None) "some pair carries predicate p".  Shorter
             lists are padded with inactive items; at most `lib.CONTENT_MAX_ITEMS` per graph.
      n_node_type, n_adj_type, node_encoding, edge_encoding: how labels and predicates are coded (`label_codes`).
      weight: w_content, the weight of the term; tau: the temperature of the soft minimum, in units of squared code distance (two 'bits'
             codes that differ in one bit are 4 apart); clip_ratio: the content shift's own clip against ||x_hat - D||, None: unclipped;
      term_weights: (subject, predicate, object) weights of the three squared distances of an item.
    No trained weights ship with the project: what this does to sample quality is not validated."""

    def __init__(self, items, n_node_type, n_adj_type, node_encoding="bits", edge_encoding="bits", weight=1.0, tau=0.5, clip_ratio=1.0,
                 term_weights=(1.0, 1.0, 1.0)):
        self.n_node_type, self.n_adj_type = int(n_node_type), int(n_adj_type)
        self.node_encoding, self.edge_encoding = node_encoding, edge_encoding
        for e in (node_encoding, edge_encoding):
            if e not in _lib.ENCODINGS:
                raise ValueError("encoding should be 'ddpm', 'bits' or 'one_hot'")
        self.weight, self.tau = float(np.float32(weight)), float(np.float32(tau))   # as the descriptor holds them: float32
        if not np.isfinite(self.weight):
            raise ValueError(f"ContentGuide: weight = {weight} is not finite")
        if not (self.tau > 0 and np.isfinite(self.tau)):
            raise ValueError(f"ContentGuide: tau = {tau} must be positive")
        if clip_ratio is not None and not float(clip_ratio) >= 0:
            raise ValueError(f"ContentGuide: clip_ratio must be >= 0 or None, got {clip_ratio}")
        self.clip_ratio = None if clip_ratio is None else float(np.float32(clip_ratio))
        tw = tuple(float(v) for v in term_weights)
        if len(tw) != 3 or not all(np.isfinite(v) and v >= 0 for v in tw):
            raise ValueError(f"ContentGuide: term_weights = {term_weights} must be three finite weights >= 0 (subject, predicate, object)")
        self.term_weights = tw
        self.items = []
        for b, lst in enumerate(items):
            row = []
            for it in lst:
                if len(it) != 3:
                    raise ValueError(f"ContentGuide: item {it} of graph {b} is not (subject, predicate, object)")
                s, p, o = (None if v is None else int(v) for v in it)
                for v, k, what in ((s, self.n_node_type, "subject label"), (o, self.n_node_type, "object label"), (p, self.n_adj_type, "predicate")):
                    if v is not None and not 0 <= v < k:
                        raise ValueError(f"ContentGuide: {what} {v} of graph {b} is outside 0..{k - 1}")
                row.append((s, p, o))
            if len(row) > _lib.CONTENT_MAX_ITEMS:
                raise ValueError(f"ContentGuide: graph {b} has {len(row)} items, at most {_lib.CONTENT_MAX_ITEMS}")
            self.items.append(row)
        self.n_items = max(1, max((len(r) for r in self.items), default=1))

    def tensors(self, c_adj, node_chans):
        """(subj [B, K, Cl], obj [B, K, Cl], pred [B, K, C_adj], w_spo [B, K, 3] = (a_s, a_o, a_p)) float32 NumPy arrays; a dropped term
        and a padding item have weight 0 and an all-zero target"""
        Cl = _code_chans(self.n_node_type, self.node_encoding, int(node_chans), "node labels")
        Ca = _code_chans(self.n_adj_type, self.edge_encoding, int(c_adj), "predicates")
        ncode, pcode = label_codes(self.n_node_type, self.node_encoding, Cl), label_codes(self.n_adj_type, self.edge_encoding, Ca)
        B, K = len(self.items), self.n_items
        subj, obj = np.zeros((B, K, Cl), np.float32), np.zeros((B, K, Cl), np.float32)
        pred, w = np.zeros((B, K, Ca), np.float32), np.zeros((B, K, 3), np.float32)
        a_s, a_p, a_o = self.term_weights
        for b, row in enumerate(self.items):
            for k, (s, p, o) in enumerate(row):
                if s is not None:
                    subj[b, k], w[b, k, 0] = ncode[s], a_s
                if o is not None:
                    obj[b, k], w[b, k, 1] = ncode[o], a_o
                if p is not None:
                    pred[b, k], w[b, k, 2] = pcode[p], a_p
        return subj, obj, pred, w

    def descriptor(self, B, cfg, node_chans=None):
        """(`lib.DsgContentCfg`, the host arrays it points at -- keep them alive over the call) for a batch of B graphs of the network
        configuration `cfg` (c_adj, c_node); node_chans defaults to c_node - 4, the label channels in front of the box"""
        if len(self.items) != B:
            raise ValueError(f"ContentGuide: items for {len(self.items)} graphs, the batch has {B}")
        Cl = int(cfg.c_node) - 4 if node_chans is None else int(node_chans)
        if Cl < 1 or Cl > int(cfg.c_node) - 4:
            raise ValueError(f"ContentGuide: node_chans = {Cl} must be 1..C_node-4 = {int(cfg.c_node) - 4}")
        keep = tuple(np.ascontiguousarray(v) for v in self.tensors(cfg.c_adj, Cl))
        clip = _lib.GUIDE_CLIP_NONE if self.clip_ratio is None else self.clip_ratio
        c = _lib.DsgContentCfg(self.weight, self.tau, clip, self.n_items, Cl, 0, *(v.ctypes.data for v in keep))
        return c, keep

    def torch_loss(self, node_flags, node_chans=None):
        """weight * L_content as a `guide.py` closure loss(D_adj, D_node) -> scalar, for `guided_sample` and the tests; the channel
        counts are read off the tensors it is called with (node_chans defaults to C_node - 4)"""
        wgt, fns = self.weight, {}

        def loss(D_adj, D_node):
            key = (int(D_adj.shape[1]), int(D_node.shape[-1]) - 4 if node_chans is None else int(node_chans))
            if key not in fns:
                fns[key] = content_loss(*self.tensors(*key), node_flags, self.tau)
            return fns[key](D_adj, D_node) * wgt
        return loss


def items_present(q_adj, q_node, node_flags, items):
    """Host check on decoded integer graphs (q_adj [B, N, N], q_node [B, N] as `io.decode` returns them): bool [B, K], K the longest
    item list -- whether graph b has an ordered pair (i, j), i != j, both valid, with q_node[i] = subject, q_adj[i, j] = predicate and
    q_node[j] = object, a None leaving its term free.  Like the loss it reads pairs: a graph with fewer than two valid nodes holds
    nothing.  Padding and all-None items count as present."""
    qa, qn, f = (np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v) for v in (q_adj, q_node, node_flags))
    B, n = qn.shape[0], qn.shape[1]
    if len(items) != B:
        raise ValueError(f"items_present: items for {len(items)} graphs, the batch has {B}")
    K = max(1, max((len(r) for r in items), default=1))
    out = np.ones((B, K), dtype=bool)
    f = f.astype(bool)
    for b, row in enumerate(items):
        live = f[b][:, None] & f[b][None, :] & ~np.eye(n, dtype=bool)
        for k, (s, p, o) in enumerate(row):
            if s is None and p is None and o is None:
                continue
            hit = live.copy()
            if s is not None:
                hit &= (qn[b] == int(s))[:, None]
            if o is not None:
                hit &= (qn[b] == int(o))[None, :]
            if p is not None:
                hit &= qa[b].reshape(n, n) == int(p)
            out[b, k] = bool(hit.any())
    return out


# ---- host arithmetic of the guided loop (no GPU needed) -------------------------------------------------------------
def guidance_weights(scale, T: int) -> np.ndarray:
    """w_i float32 [T] from `scale`: a number (the same weight at every level) or T of them (list, ndarray, tensor)."""
    if isinstance(scale, torch.Tensor):
        scale = scale.detach().cpu().numpy()
    w = np.asarray(scale, dtype=np.float64)
    if w.ndim == 0:
        w = np.full(T, float(w))
    if w.shape != (T,):
        raise ValueError(f"scale must be a number or {T} weights (one per schedule index), got shape {w.shape}")
    if not np.all(np.isfinite(w)):
        raise ValueError("scale must be finite")
    return w.astype(np.float32)


def clip_factor(shift_norm, ref_norm, clip_ratio):
    """Per-graph factor in (0, 1] that rescales a shift of 2-norm `shift_norm` so that it never exceeds clip_ratio * ref_norm
    (ref_norm = ||x_hat_b - D_b||); 1 where the shift is already inside, or where clip_ratio is None.  Tensors [B] in, [B] out."""
    if clip_ratio is None:
        return torch.ones_like(shift_norm)
    r = float(clip_ratio)
    if not r >= 0:
        raise ValueError(f"clip_ratio must be >= 0 or None, got {clip_ratio}")
    bound = r * ref_norm
    return torch.where(shift_norm > bound, bound / shift_norm.clamp(min=torch.finfo(shift_norm.dtype).tiny), torch.ones_like(shift_norm))


def _graph_norm(a, x):
    return torch.sqrt((a * a).flatten(1).sum(1) + (x * x).flatten(1).sum(1))


# ---- the loop -------------------------------------------------------------------------------------------------------
def guided_sample(net, sampler, node_flags, loss_fn, scale, *, clip_ratio=1.0, known=None, seed=None, graph_seeds=None,
                  coin_seed=None, return_trace=False):
    """Sample with the denoised estimate of every preconditioned call shifted against grad_x L(D(x, sigma)) (module docstring).

    net: the NodeAdjPrecondHip of build_network(); sampler: a NodeAdjEDMSamplerHip (schedule, solver, churn, seed, self-conditioning).
    loss_fn(D_adj, D_node) -> scalar, as in `value_and_input_grad`.  scale: w, or one w_i per schedule index.  clip_ratio = r: per
    graph the shift is rescaled so that its 2-norm never exceeds r * ||x_hat_b - D_b||; None: unclipped.
    known = (known_adj, known_node, mask_adj, mask_node): the exact select of `sample_known`, applied after the shift (known entries
    win).  The self-conditioning input of the next call is the estimate after the select and before the shift.
    seed / graph_seeds / coin_seed: as in `sampler.sample`.  Heun's stage 2 is evaluated at (x_hat, t_hat) like the reference's and
    guided the same way; 'dpmpp_2m' extrapolates the guided estimate.
    Returns (adjs, nodes) on the device (single channels squeezed); with return_trace also a list with one dict per preconditioned call:
    step, stage, t_hat, w, x_hat, D (after the select), grad, shift (as applied), D_guided, and x (the state after the call's update, in
    the entry of a step's last call) -- (adj, node) pairs of device tensors."""
    if not isinstance(net, NodeAdjPrecondHip):
        raise TypeError("guided_sample needs the NodeAdjPrecondHip network returned by build_network()")
    if sampler.solver not in SOLVERS:
        raise ValueError(sampler.solver)
    if not callable(loss_fn):
        raise TypeError("loss_fn must be callable: loss_fn(D_adj, D_node) -> scalar tensor")
    T = sampler.num_steps
    w_all = guidance_weights(scale, T)
    if clip_ratio is not None and not float(clip_ratio) >= 0:
        raise ValueError(f"clip_ratio must be >= 0 or None, got {clip_ratio}")
    m = net.model
    cfg, dev = m.config, m._dev
    B, n = node_flags.shape[0], cfg.max_node_num
    gs = None
    if graph_seeds is not None:
        if seed is not None:
            raise ValueError("give seed= (one noise stream over the whole batch) or graph_seeds= (one per graph), not both")
        gs = check_graph_seeds(graph_seeds, B)
    elif coin_seed is not None:
        raise ValueError("coin_seed= belongs to graph_seeds=; an unseeded call draws its coins from the NumPy global generator")
    sa, sn = (B, cfg.c_adj, n, n), (B, n, cfg.c_node)
    if known is not None:
        if len(known) != 4 or any(k is None for k in known):
            raise ValueError("known = (known_adj, known_node, mask_adj, mask_node)")
        ka = known[0].to(device=dev, dtype=torch.float32).reshape(sa)
        kn = known[1].to(device=dev, dtype=torch.float32).reshape(sn)
        ma = (known[2].to(device=dev) != 0).reshape(sa)
        mn = (known[3].to(device=dev) != 0).reshape(sn)
    scfg = sampler._cfg()
    sigma_steps, t_hat, noise_coef, h_step = _lib.sigma_schedule(scfg)
    ms_coef = _lib.multistep_coef(scfg)
    heun = sampler.solver == "heun"
    n_calls = 2 * T - 1 if heun else T
    if gs is not None:
        coins = sampler.draw_coins_seeded(n_calls, sampler.seed if coin_seed is None else coin_seed)
    else:
        coins = sampler.draw_coins(n_calls)
    f = node_flags.to(device=dev).bool()
    fa, fn = (f[:, None, :, None] & f[:, None, None, :]), f[:, :, None]
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    mask = lambda a, x: (torch.where(fa, a, zero), torch.where(fn, x, zero))
    noise = lambda stream: sampler.device_noise(net, node_flags, stream=stream, seed=seed, graph_seeds=gs)
    fl8 = f.to(torch.uint8).contiguous()
    f32 = np.float32
    # per-step scalars: float32 values held as Python floats (exact), so that torch applies them as float32 scalars, tensor on the left

    def denoise(xa, xn, t, w, sc, coin):
        """one guided preconditioned call at (x_hat, t): (D after the select, D~, trace entry)"""
        sca, scn = sc
        if net.self_condition and coin:   # precond.py:90-98: the estimate of a no-grad extra pass becomes the self-conditioning input
            with torch.no_grad():
                sig = torch.full((B,), float(t), dtype=torch.float32, device=dev)
                p = lambda v: None if v is None else v.data_ptr()
                hd = m._ensure_handle()
                ca, cx = torch.empty(sa, dtype=torch.float32, device=dev), torch.empty(sn, dtype=torch.float32, device=dev)
                hd.check(hd.L.dsg_precond(hd.raw, B, p(xa), p(xn), p(fl8), p(sig), p(sca), p(scn), 0, p(ca), p(cx),
                                          torch.cuda.current_stream(dev).cuda_stream), "dsg_precond")
                if known is not None:
                    ca, cx = mask(torch.where(ma, ka, ca), torch.where(mn, kn, cx))
                sca, scn = ca, cx
        Da, Dn, _, ga, gn = net.value_and_input_grad(xa, xn, node_flags, float(t), loss_fn=loss_fn, self_cond_adjs=sca,
                                                     self_cond_nodes=scn, coin=False)
        with torch.no_grad():
            Da, Dn, ga, gn = Da.reshape(sa), Dn.reshape(sn), ga.reshape(sa), gn.reshape(sn)
            if known is not None:
                Da, Dn = mask(torch.where(ma, ka, Da), torch.where(mn, kn, Dn))
            wt2 = float(f32(w) * f32(t) * f32(t))
            sha, shn = mask(ga * wt2, gn * wt2)
            fac = clip_factor(_graph_norm(sha, shn), _graph_norm(xa - Da, xn - Dn), clip_ratio)
            sha, shn = sha * fac[:, None, None, None], shn * fac[:, None, None]
            Ga, Gn = Da - sha, Dn - shn
            if known is not None:
                Ga, Gn = mask(torch.where(ma, ka, Ga), torch.where(mn, kn, Gn))
        entry = dict(t_hat=float(t), w=float(w), x_hat=(xa, xn), D=(Da, Dn), grad=(ga, gn), shift=(sha, shn), D_guided=(Ga, Gn)) if return_trace else None
        return (Da, Dn), (Ga, Gn), entry

    trace = []
    with torch.no_grad():
        ia, inn = noise(0)
        xa, xn = mask(ia * float(f32(sigma_steps[0])), inn * float(f32(sigma_steps[0])))   # x0 = init * sigma(t0) (edm.py:326, :346-347)
    sc = (None, None)
    prev = None   # the previous step's guided estimate (dpmpp_2m)
    call = 0
    for i in range(T):
        t, hs, inv_t, nc, mc = float(t_hat[i]), float(h_step[i]), float(f32(1.0) / f32(t_hat[i])), float(noise_coef[i]), float(ms_coef[i])
        with torch.no_grad():
            if nc != 0:
                ea, en = noise(i + 1)
                xha, xhn = mask(xa + ea * nc, xn + en * nc)   # edm.py:361-366
            else:
                xha, xhn = mask(xa, xn)
        D1, G1, e1 = denoise(xha, xhn, t, float(w_all[i]), sc, bool(coins[call]))
        call += 1
        euler = not heun or i == T - 1
        with torch.no_grad():
            if euler:
                Ta, Tn = G1
                if mc != 0 and prev is not None:   # D~ + c (D~ - D~prev): DPM-Solver++ 2M on the guided estimate
                    Ta, Tn = Ta + (Ta - prev[0]) * mc, Tn + (Tn - prev[1]) * mc
                xa, xn = mask(xha + (xha * inv_t - Ta * inv_t) * hs, xhn + (xhn * inv_t - Tn * inv_t) * hs)   # edm.py:384-385, :395-396
                sc_next, last = D1, e1
        if not euler:
            # stage 2 re-evaluates at (x_hat, t_hat) with self-cond = the stage-1 estimate (edm.py:400-405)
            D2, G2, e2 = denoise(xha, xhn, t, float(w_all[i]), D1 if net.self_condition else (None, None), bool(coins[call]))
            call += 1
            with torch.no_grad():
                inv_tp = float(f32(1.0) / (f32(t) + f32(hs)))
                upd = []
                for xh, g1, g2 in ((xha, G1[0], G2[0]), (xhn, G1[1], G2[1])):
                    dc = xh * inv_t - g1 * inv_t
                    xp = xh + dc * hs
                    dp = xp * inv_tp - g2 * inv_tp
                    upd.append(xh + (dc * 0.5 + dp * 0.5) * hs)                                       # edm.py:414-422
                xa, xn = mask(*upd)
            sc_next, last = D2, e2
            if return_trace:
                e1.update(step=i, stage=1)
                trace.append(e1)
        if return_trace:
            last.update(step=i, stage=1 if euler else 2, x=(xa, xn))
            trace.append(last)
        prev = G1
        sc = sc_next if net.self_condition else (None, None)
    out = m._shape_out(xa, xn)
    return (out[0], out[1], trace) if return_trace else out
