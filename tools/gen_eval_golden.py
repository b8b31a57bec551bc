#!/usr/bin/env python3
"""Generate tests/golden/eval_metrics.npz from the reference's own SceneGraphEvaluator (R/evaluation/bbox_metrics.py).

DEV-CONTAINER ONLY: needs a checkout of the reference; nothing at run time imports this script.  The inputs are built here
from a fixed seed and stored in the npz next to the reference's outputs (they are small: 24 x 20 scenes).

How the reference is imported (two disclosed stubs, neither touches an evaluated number):
  * `pyemd` is not installed; R/evaluation/mmd.py imports it for the `gaussian_emd` kernel only, and only `gaussian` is
    evaluated here.  An empty module object is registered so the import statement resolves.
  * networkx 3.4 removed `from_numpy_matrix`, which adjs_to_graphs (R/evaluation/stats.py:187) calls; it is aliased to
    `from_numpy_array`, its replacement with the same behaviour for a 2-D array.

Cases (see _bbox_case): VG-like (150 classes, N = 62) and COCO-like (171 classes, N = 33) scene sets with three class-weight
vectors and None, the all-ones "no node type" call of sg_go_sampling, empty scenes, invalid boxes (x2 or y2 = 0), scene pairs
without a common class, IoUs one float32 step either side of a threshold (and exactly on 0.5), a class-weight union summing to
0 (NaN), graphs without edges, and the three MMDs.

Usage:  python tools/gen_eval_golden.py --ref <reference checkout>/DiffuseSG [--out tests/golden/eval_metrics.npz]
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _import_reference(ref_dir):
    import networkx as nx
    sys.modules.setdefault("pyemd", types.ModuleType("pyemd"))
    nx.from_numpy_matrix = nx.from_numpy_array
    sys.path.insert(0, ref_dir)
    from evaluation.bbox_metrics import SceneGraphEvaluator
    from evaluation.bbox_utils import Evaluator
    return SceneGraphEvaluator, Evaluator


def _cxcywh_to_xyxy(b):
    cx, cy, w, h = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([cx - np.float32(0.5) * w, cy - np.float32(0.5) * h, cx + np.float32(0.5) * w, cy + np.float32(0.5) * h], -1)


def _edge_box(Evaluator, thr, above):
    """A detection (0, 0, a, a) whose float32 IoU with the ground truth (0, 0, 1, 1) is the float32 next to `thr` (float64)
    on the given side: IoU = (a + 1)^2 / 4 with the +1 areas."""
    gt = (np.float32(0), np.float32(0), np.float32(1), np.float32(1))
    a = np.float32(2 * np.sqrt(thr) - 1)
    for _ in range(200):
        q = Evaluator.iou((np.float32(0), np.float32(0), a, a), gt)
        if (q >= thr) == above:
            # one step towards the threshold must flip the side: then `a` is the float32 box closest to it on this side
            b = np.nextafter(a, np.float32(-1) if above else np.float32(2))
            if (Evaluator.iou((np.float32(0), np.float32(0), b, b), gt) >= thr) != above:
                return a, q
            a = b
        else:
            a = np.nextafter(a, np.float32(2) if above else np.float32(-1))
    raise RuntimeError(f"no box next to IoU {thr}")


def _bbox_case(rng, Evaluator, X, Y, N, n_cls, palette):
    """Generated / reference scene sets: references random, generated ones perturbed copies (so that matches happen),
    plus the special rows described in the module docstring."""
    def scenes(S):
        box = _cxcywh_to_xyxy(np.concatenate([rng.uniform(0.1, 0.9, (S, N, 2)), rng.uniform(0.05, 0.6, (S, N, 2))], -1)
                              .astype(np.float32)).clip(0.0, 1.0).astype(np.float32)
        cls = rng.choice(palette, size=(S, N)).astype(np.int64)
        nn = rng.integers(1, N + 1, S)
        flag = (np.arange(N)[None, :] < nn[:, None]).astype(np.float32)
        return box, cls, flag

    br, cr, fr = scenes(Y)
    src = rng.integers(0, Y, X)
    bg = (br[src] + rng.normal(0, 0.03, (X, N, 4))).clip(0.0, 1.0).astype(np.float32)
    cg = np.where(rng.uniform(size=(X, N)) < 0.2, rng.choice(palette, size=(X, N)), cr[src]).astype(np.int64)
    fg = np.where(rng.uniform(size=(X, N)) < 0.1, 1.0 - fr[src], fr[src]).astype(np.float32)
    # empty scenes
    fg[0] = 0
    fr[0] = 0
    # invalid boxes: x2 = 0 or y2 = 0 on flagged nodes
    bg[1, ::2, 2] = 0
    bg[1, 1::2, 3] = 0
    br[1, ::3, 2] = 0
    # no common class: scene pair (2, 2) draws from disjoint class ranges
    cg[2] = rng.integers(0, 5, N)
    cr[2] = rng.integers(5, 10, N)
    # classes whose area weight is 0 (n_cls-10 .. n_cls-1) only: the weighted union of pair (3, 3) sums to 0
    cg[3] = rng.integers(n_cls - 10, n_cls, N)
    cr[3] = rng.integers(n_cls - 10, n_cls, N)
    # IoUs one float32 step either side of a threshold on nodes 0..7 of generated / reference scenes 4..7
    thr = np.linspace(0.05, 0.5, 10)
    for s in range(4, 8):
        for j, (t, above) in enumerate((t, above) for t in (thr[5], thr[7], thr[8], thr[9]) for above in (True, False)):
            a, q = _edge_box(Evaluator, t, above)
            bg[s, j] = (0, 0, a, a)
            br[s, j] = (0, 0, 1, 1)
            cg[s, j] = cr[s, j] = palette[0]
            fg[s, j] = fr[s, j] = 1
    print("IoU type:", type(q), "(float32 under NumPy 2)")
    # exact IoUs on the last node: 0.75, 0.5625, 0.5 (= the last threshold), and an invalid reference box (y2 = 0)
    for s, gbox, rbox in ((4, (0, 0, 1, 0.5), (0, 0, 1, 1)), (5, (0, 0, 1, 1), (0, 0, 0.5, 0.5)),
                          (6, (0, 0, 0.5, 1), (0.5, 0, 1, 1)), (7, (0, 0, 1, 1), (0, 0, 1, 0))):
        bg[s, N - 1], br[s, N - 1] = gbox, rbox
        cg[s, N - 1] = cr[s, N - 1] = palette[1]
        fg[s, N - 1] = fr[s, N - 1] = 1
    assert Evaluator.iou(tuple(np.float32(v) for v in (0, 0, 0.5, 1)), tuple(np.float32(v) for v in (0.5, 0, 1, 1))) == 0.5
    return bg, cg, fg, br, cr, fr


def _weights(rng, n_cls):
    area = rng.uniform(0.01, 1.0, n_cls)
    area[n_cls - 10:] = 0.0
    area /= area.sum()
    freq = rng.integers(1, 1000, n_cls).astype(np.float64)
    freq /= freq.sum()
    return [np.ones_like(area), area, freq]


def _graphs(rng, B, N, K, p):
    adj = np.where(rng.uniform(size=(B, N, N)) < p, rng.integers(1, K, (B, N, N)), 0)
    adj = np.triu(adj, 1)
    adj = adj + adj.transpose(0, 2, 1)
    return adj.astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference's DiffuseSG/ directory")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "eval_metrics.npz"))
    args = ap.parse_args()
    SGE, Evaluator = _import_reference(args.ref)
    rng = np.random.default_rng(20261016)
    g = {"iou_thresholds": np.linspace(0.05, 0.5, 10)}

    for name, X, Y, N, n_cls in (("vg", 24, 20, 62, 150), ("coco", 24, 20, 33, 171)):
        palette = rng.choice(n_cls - 10, 12, replace=False)
        bg, cg, fg, br, cr, fr = _bbox_case(rng, Evaluator, X, Y, N, n_cls, palette)
        w = _weights(rng, n_cls)
        T = torch.from_numpy
        f1 = SGE.compute_bbox_f1(T(bg), T(cg), T(fg), T(br), T(cr), T(fr), w)
        f1_none = SGE.compute_bbox_f1(T(bg), T(cg), T(fg), T(br), T(cr), T(fr), class_weight_ls=None)
        ones_g, ones_r = torch.ones_like(T(cg)), torch.ones_like(T(cr))
        f1_nt = SGE.compute_bbox_f1(T(bg), ones_g, T(fg), T(br), ones_r, T(fr), class_weight_ls=None).squeeze(2)
        print(f"{name}: f1 {f1.shape}, nan {int(np.isnan(f1).sum())}, zero {int((f1 == 0).sum())}, "
              f"mean {np.nanmean(f1):.4f}; unweighted mean {f1_none.mean():.4f}; no-node-type mean {f1_nt.mean():.4f}")
        assert np.isnan(f1[3, 3, 1]) and np.all(f1[2, 2] == 0) and np.all(f1[0] == 0)
        g.update({f"{name}_box_gen": bg, f"{name}_cls_gen": cg, f"{name}_flag_gen": fg, f"{name}_box_ref": br,
                  f"{name}_cls_ref": cr, f"{name}_flag_ref": fr, f"{name}_weights": np.stack(w), f"{name}_f1": f1,
                  f"{name}_f1_none": f1_none, f"{name}_f1_no_node_type": f1_nt})

    # MMDs: VG-like graphs (150 node types, 51 edge types, N = 62); some graphs have no edge, one whole set has none
    B_gen, B_ref, N, Kn, Ke = 24, 20, 62, 150, 51
    fg = (np.arange(N)[None] < rng.integers(1, N + 1, B_gen)[:, None]).astype(np.float32)
    fr = (np.arange(N)[None] < rng.integers(1, N + 1, B_ref)[:, None]).astype(np.float32)
    fr[0] = 0
    ng = rng.integers(0, Kn, (B_gen, N))
    nr = rng.integers(0, 20, (B_ref, N))
    eg = _graphs(rng, B_gen, N, Ke, 0.02)
    er = _graphs(rng, B_ref, N, Ke, 0.05)
    eg[[1, 5, 9]] = 0
    er[[2, 3]] = 0
    eg[4, 3, 3] = 7                       # a self-loop: an edge type, not a degree
    er[6, :, 40:] = 0
    er[6, 40:, :] = 0                     # nodes without edges: removed from the degree histogram
    T = torch.from_numpy
    node = SGE.compute_node_type_mmd(T(ng), T(nr), T(fg), T(fr), Kn, ["gaussian"])
    edge = SGE.compute_edge_type_mmd(T(eg), T(er), T(fg), T(fr), Ke, ["gaussian"])
    edge_empty = SGE.compute_edge_type_mmd(T(np.zeros_like(eg)), T(er), T(fg), T(fr), Ke, ["gaussian"])
    deg = SGE.compute_node_degree_mmd(T(eg), T(er), ["gaussian"])
    print("node type mmd", node, "edge type mmd", edge, "(no generated edge:", edge_empty, ") degree mmd", deg)
    assert edge_empty["gaussian"] == -1.0
    g.update({"mmd_flag_gen": fg, "mmd_flag_ref": fr, "mmd_node_gen": ng, "mmd_node_ref": nr, "mmd_edge_gen": eg.astype(np.uint8),
              "mmd_edge_ref": er.astype(np.uint8), "mmd_num_node_types": np.int64(Kn), "mmd_num_edge_types": np.int64(Ke),
              "mmd_node_type": np.float64(node["gaussian"]), "mmd_edge_type": np.float64(edge["gaussian"]),
              "mmd_degree": np.float64(deg["gaussian"]["degree"]), "mmd_degree_average": np.float64(deg["gaussian"]["average"])})
    np.savez_compressed(args.out, **g)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
