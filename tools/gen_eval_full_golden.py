#!/usr/bin/env python3
"""Generate tests/golden/eval_full.npz from the reference's own SceneGraphEvaluator (R/evaluation/bbox_metrics.py): the layout
metrics of compute_bbox_ioa, compute_triplet_tv_dist, the F1 summaries of sg_go_sampling and one whole evaluation block.

DEV-CONTAINER ONLY: needs a checkout of the reference; nothing at run time imports this script.  The inputs are built here from
a fixed seed and stored in the npz next to the reference's outputs.  The reference is imported as tools/gen_eval_golden.py does
(its two disclosed stubs: an empty `pyemd` module, and networkx's removed `from_numpy_matrix` aliased to `from_numpy_array`).
torchvision is not installed here, so the evaluation block converts boxes with diffusesg_amd.evaluate.cxcywh_to_xyxy, which
tests/test_eval_metrics.py::test_cxcywh_to_xyxy holds to torchvision's operations.

Cases:
  * layouts: a VG-like (N = 62) and a COCO-like (N = 33) set of 40 layouts, handed to the reference as torch tensors as
    sg_go_sampling does.  Layouts 0-9: a single box, two disjoint boxes, two touching boxes, two identical boxes, zero-area boxes
    among others, only zero-area boxes, overlapping boxes of side 5e-5 (the np.isclose branch of the IoU), coordinates on
    multiples of 1/64 (half-pixel rounding), all N boxes, flags that are not a prefix.  10-38: random.  39: empty (the
    perceptual call runs on layouts 0-38: the reference raises on an empty one).
  * triplets: 40 graphs, 12 node types, 50 predicates, a dictionary of 2426 random keys; triplet_to_count as all keys and as the
    first 100; int64 and float32 inputs; a graph without edges, edges on unflagged nodes, a diagonal entry; an all-zero batch
    and a batch whose triplets are all novel.
  * F1 summaries: the 12 numbers of sg_go_sampling from the reference's F1 matrices of a 16 x 12 case, the area-weighted one
    with a NaN row.
  * one evaluate_samples case: the reference's calls in sg_go_sampling's order (sampler_node_adj.py:445-552).
The script asserts that every metric has a value for more than half of each layout set and None for at least one layout, and
that the main triplet case has at least a fifth of its triplets in the dictionary and a tenth novel.  It prints the reference's
seconds per layout and per (graph x key).

Usage:  python tools/gen_eval_full_golden.py --ref <reference checkout>/DiffuseSG [--out tests/golden/eval_full.npz]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_eval_golden import _import_reference                  # noqa: E402
from diffusesg_amd.evaluate import cxcywh_to_xyxy              # noqa: E402

METRICS = ("vanilla_iou", "perceptual_iou", "overlap", "alignment")
T = torch.from_numpy


def _random_boxes(rng, n):
    b = np.concatenate([rng.uniform(0.05, 0.95, (n, 2)), rng.uniform(0.02, 0.5, (n, 2))], -1).astype(np.float32)
    return cxcywh_to_xyxy(T(b)).clip(0.0, 1.0).numpy()


def _layout_set(rng, B, N):
    box = np.zeros((B, N, 4), np.float32)
    flag = np.zeros((B, N), bool)

    def put(i, rows, at=None):
        rows = np.asarray(rows, np.float32).reshape(-1, 4)
        at = np.arange(len(rows)) if at is None else at
        box[i, at], flag[i, at] = rows, True

    put(0, [[0.2, 0.3, 0.6, 0.7]])
    put(1, [[0.1, 0.1, 0.3, 0.3], [0.5, 0.5, 0.9, 0.8]])
    put(2, [[0.25, 0.25, 0.5, 0.75], [0.5, 0.25, 0.75, 0.75]])
    put(3, [[0.2, 0.2, 0.7, 0.6], [0.2, 0.2, 0.7, 0.6]])
    z = _random_boxes(rng, 9)
    z[::3, 2] = z[::3, 0]                                  # zero width
    z[1::3, 3] = z[1::3, 1]                                # zero height
    put(4, z)
    z = _random_boxes(rng, 6)
    z[:, 2] = z[:, 0]
    put(5, z)
    s = np.float32(5e-5)
    put(6, [[0.5, 0.5, 0.5 + s, 0.5 + s], [0.5 + s / 2, 0.5 + s / 2, 0.5 + 3 * s / 2, 0.5 + 3 * s / 2], [0.5, 0.5, 0.5 + s, 0.5 + s]])
    k = np.sort(rng.integers(0, 65, (12, 2, 2)), axis=1)   # [n, (lo, hi), (x, y)] in 1/64 steps: half pixels on a 32 canvas
    put(7, np.concatenate([k[:, 0], k[:, 1]], -1) / 64.0)
    put(8, _random_boxes(rng, N))
    at = np.sort(rng.choice(N, 11, replace=False))
    box[9] = _random_boxes(rng, N)                         # boxes on unflagged nodes too
    flag[9, at] = True
    for i in range(10, B - 1):
        n = int(rng.integers(2, N + 1))
        put(i, _random_boxes(rng, n))
        if i % 4 == 0:                                     # sparse layouts: few, small boxes
            n = int(rng.integers(2, 5))
            box[i], flag[i] = 0, False
            b = np.concatenate([rng.uniform(0.1, 0.9, (n, 2)), rng.uniform(0.02, 0.15, (n, 2))], -1).astype(np.float32)
            put(i, cxcywh_to_xyxy(T(b)).clip(0.0, 1.0).numpy())
    return box, flag                                       # layout B-1 stays empty


def _layout_case(SGE, g, name, box, flag):
    B = len(box)
    tb, tf = T(box), T(flag)
    secs = {}
    for m, metric in enumerate(METRICS):
        kw = {"flag_" + metric: True}
        n = B - 1 if metric == "perceptual_iou" else B     # get_perceptual_iou raises on the empty layout
        t0 = time.perf_counter()
        vals = SGE.compute_bbox_ioa(tb[:n], tf[:n], canvas_size=32, **kw)
        secs[metric] = (time.perf_counter() - t0) / n
        mean = SGE.compute_bbox_ioa(tb[:n], tf[:n], canvas_size=32, return_mean=True, **kw)
        valid = np.array([len(SGE.compute_bbox_ioa(tb[i:i + 1], tf[i:i + 1], canvas_size=32, **kw)) == 1 for i in range(n)])
        vals = np.array([np.asarray(v) for v in vals])
        assert valid.sum() == len(vals) and valid.sum() > n / 2 and (~valid).sum() >= 1, (name, metric, valid.sum(), n)
        print(f"{name} {metric}: {valid.sum()} of {n} valued, dtype {vals.dtype}, mean {float(mean):.6g} ({np.asarray(mean).dtype})")
        g[f"{name}_{metric}"] = vals.astype(np.float64)    # float32 values (IoU, overlap) are stored exactly
        g[f"{name}_{metric}_valid"] = valid
        g[f"{name}_{metric}_mean"] = np.float64(mean)
    try:
        SGE.compute_bbox_ioa(tb, tf, canvas_size=32, flag_perceptual_iou=True)
        raise SystemExit("the reference accepted an empty layout")
    except ValueError:
        pass
    g[f"{name}_box"], g[f"{name}_flag"] = box, flag
    print(f"{name}: reference seconds per layout (torch inputs, mean {flag.sum(1).mean():.1f} boxes): "
          + ", ".join(f"{k} {v:.4f}" for k, v in secs.items()))


def _graphs(rng, B, N, n_types, n_pred, p):
    edge = np.where(rng.uniform(size=(B, N, N)) < p, rng.integers(1, n_pred + 1, (B, N, N)), 0).astype(np.int64)
    node = rng.integers(0, n_types, (B, N)).astype(np.int64)
    return edge, node


def _triplet_dict(rng, n_types, n_pred, n_keys):
    ids = rng.choice(n_types * n_types * n_pred, n_keys, replace=False)
    keys = np.stack([ids // (n_types * n_pred), ids // n_pred % n_types, ids % n_pred + 1], -1)
    freq = rng.integers(1, 500, n_keys).astype(np.float64)
    return keys, freq / freq.sum()


def _triplet_case(SGE, g, rng):
    B, N, n_types, n_pred, n_keys = 40, 62, 12, 50, 2426
    keys, freq = _triplet_dict(rng, n_types, n_pred, n_keys)
    d = {tuple(int(v) for v in k): float(f) for k, f in zip(keys, freq)}
    edge, node = _graphs(rng, B, N, n_types, n_pred, 0.03)
    flag = np.arange(N)[None] < rng.integers(1, N + 1, B)[:, None]   # edges lie on unflagged nodes too: the flags are ignored
    edge[0] = 0                                                       # a graph without edges
    edge[1, 5, 5] = 7                                                 # a diagonal entry
    g.update(trip_keys=keys.astype(np.int16), trip_freq=freq, trip_edge=edge.astype(np.uint8), trip_node=node.astype(np.uint8),
             trip_flag=flag)
    everything = list(d.keys())
    t0 = time.perf_counter()
    out_all = SGE.compute_triplet_tv_dist(T(edge), T(node), T(flag), d, everything)
    secs = time.perf_counter() - t0
    out_100 = SGE.compute_triplet_tv_dist(T(edge), T(node), T(flag), d, everything[:100])
    out_f32 = SGE.compute_triplet_tv_dist(T(edge).float(), T(node).float(), T(flag), d, everything)
    assert out_f32 == out_all
    hist = SGE._get_triplet_type_hist(T(edge), T(node), T(flag), allowed_triplet=d.keys(), reject_novel_triplet=True)
    counts = np.stack(hist).sum(0).astype(np.int64)
    total = int((edge != 0).sum())
    novelty = float(out_all[3])
    assert counts.sum() >= total / 5 and novelty >= 0.1 and (counts == 0).any()
    assert abs(novelty - (total - counts.sum()) / total) < 1e-12
    print(f"triplets: {total} in {B} graphs, {counts.sum()} in the dictionary, novelty {novelty:.4f}, {int((counts == 0).sum())} of "
          f"{n_keys} keys never generated; reference {secs:.3f} s = {secs / (B * n_keys):.3e} s per (graph x key)")
    g.update(trip_counts=counts, trip_novel=np.int64(total - counts.sum()), trip_out_all=np.array(out_all, np.float64),
             trip_out_100=np.array(out_100, np.float64), trip_out_f32=np.array(out_f32, np.float64))
    zero = SGE.compute_triplet_tv_dist(T(np.zeros_like(edge[:4])), T(node[:4]), T(flag[:4]), d, everything[:100])
    g["trip_out_zero"] = np.array(zero, np.float64)
    g["trip_node_novel"] = (node[:6] + n_types).astype(np.uint8)      # node types 12..23: no key has them
    novel = SGE.compute_triplet_tv_dist(T(edge[:6]), T(node[:6] + n_types), T(flag[:6]), d, everything[:100])
    assert novel[3] == 1.0
    g["trip_out_novel"] = np.array(novel, np.float64)
    print("triplets: all-zero batch", zero, "all-novel batch", novel)


def _f1_scenes(rng, X, Y, N, n_cls):
    br = np.concatenate([rng.uniform(0.1, 0.9, (Y, N, 2)), rng.uniform(0.05, 0.6, (Y, N, 2))], -1).astype(np.float32)   # cxcywh
    cr = rng.integers(0, n_cls - 4, (Y, N)).astype(np.int64)
    fr = np.arange(N)[None] < rng.integers(1, N + 1, Y)[:, None]
    src = rng.integers(0, Y, X)
    bg = (br[src] + rng.normal(0, 0.02, (X, N, 4))).astype(np.float32)
    cg = np.where(rng.uniform(size=(X, N)) < 0.2, rng.integers(0, n_cls - 4, (X, N)), cr[src]).astype(np.int64)
    fg = np.where(rng.uniform(size=(X, N)) < 0.1, ~fr[src], fr[src])
    fg[:, 0] = True                                                   # no empty layout: the perceptual IoU refuses one
    return bg, cg, fg, br, cr, fr


def _f1_summaries(mats):
    out = {}
    for name, m in mats.items():
        out[f"{name}_f1_avg_max"] = m.max(axis=-1).mean()
        out[f"{name}_f1_avg_mean"] = m.mean(axis=-1).mean()
        out[f"{name}_f1_avg_median"] = np.median(m, axis=-1).mean()
    return out


def _f1_case(SGE, g, rng):
    """The 12 summaries of sampler_node_adj.py:533-546; generated scene 3 and reference scene 3 hold only classes whose area
    weight is 0, so row 3 of the area-weighted matrix holds a NaN."""
    X, Y, N, n_cls = 16, 12, 20, 30
    bg, cg, fg, br, cr, fr = _f1_scenes(rng, X, Y, N, n_cls)
    bg, br = (cxcywh_to_xyxy(T(b)).clip(0.0, 1.0).numpy() for b in (bg, br))
    cg[3] = cr[3] = rng.integers(n_cls - 4, n_cls, N)
    area = rng.uniform(0.01, 1.0, n_cls)
    area[n_cls - 4:] = 0.0
    freq = rng.integers(1, 1000, n_cls).astype(np.float64)
    w = [np.ones(n_cls), area / area.sum(), freq / freq.sum()]
    f1 = SGE.compute_bbox_f1(T(bg), T(cg), T(fg), T(br), T(cr), T(fr), w)
    nt = SGE.compute_bbox_f1(T(bg), torch.ones_like(T(cg)), T(fg), T(br), torch.ones_like(T(cr)), T(fr), class_weight_ls=None).squeeze(2)
    summ = _f1_summaries({"vanilla": f1[..., 0], "area": f1[..., 1], "freq": f1[..., 2], "no_node_type": nt})
    print("F1 summaries:", {k: float(v) for k, v in summ.items()}, "NaN rows (area):", np.flatnonzero(np.isnan(f1[..., 1]).any(1)))
    assert np.isnan(summ["area_f1_avg_max"]) and not np.isnan(summ["vanilla_f1_avg_max"]) and not np.isnan(f1[..., 1]).all()
    g.update(f1_box_gen=bg, f1_cls_gen=cg.astype(np.uint8), f1_flag_gen=fg, f1_box_ref=br, f1_cls_ref=cr.astype(np.uint8), f1_flag_ref=fr,
             f1_weights=np.stack(w), f1_mat=f1, f1_mat_no_node_type=nt, f1_summary_keys=np.array(list(summ.keys())),
             f1_summary=np.array(list(summ.values()), np.float64))


def _samples_case(SGE, g, rng):
    """sg_go_sampling's evaluation block, call by call (sampler_node_adj.py:445-552)."""
    X, Y, N, Kn, Ke = 14, 10, 16, 12, 9
    bg, cg, fg, br, cr, fr = _f1_scenes(rng, X, Y, N, Kn + 4)
    ag, _ = _graphs(rng, X, N, Kn, Ke - 1, 0.08)
    ar, _ = _graphs(rng, Y, N, Kn, Ke - 1, 0.1)
    ag[2] = 0
    vk, vf = _triplet_dict(rng, Kn, Ke - 1, 300)
    tk, tf = _triplet_dict(rng, Kn, Ke - 1, 500)
    val_d = {tuple(int(v) for v in k): float(f) for k, f in zip(vk, vf)}
    train_d = {tuple(int(v) for v in k): float(f) for k, f in zip(tk, tf)}
    to_count = list(train_d.keys())[:50]
    area = rng.uniform(0.01, 1.0, Kn)
    freq = rng.integers(1, 1000, Kn).astype(np.float64)
    g.update(es_adj_gen=ag.astype(np.uint8), es_node_gen=cg.astype(np.uint8), es_box_gen=bg, es_flag_gen=fg, es_adj_gt=ar.astype(np.uint8),
             es_node_gt=cr.astype(np.uint8), es_box_gt=br, es_flag_gt=fr, es_val_keys=vk.astype(np.int16), es_val_freq=vf,
             es_train_keys=tk.astype(np.int16), es_train_freq=tf, es_n_to_count=np.int64(len(to_count)), es_area=area, es_freq=freq,
             es_num_node_types=np.int64(Kn), es_num_edge_types=np.int64(Ke))
    adjs, adjs_gt, nodes, nodes_gt, flags, flags_gt = T(ag), T(ar), T(cg), T(cr), T(fg), T(fr)
    h, res = SGE(), {}
    mmd_kernels = ["gaussian"]
    for kernel, val_par in h.compute_node_degree_mmd(adjs, adjs_gt, mmd_kernels).items():
        for key, val in val_par.items():
            res[f"node_{key}_mmd_{kernel}"] = val
    for kernel, val in h.compute_node_type_mmd(nodes, nodes_gt, flags, flags_gt, Kn, mmd_kernels).items():
        res[f"node_type_mmd_{kernel}"] = val
    for kernel, val in h.compute_edge_type_mmd(adjs, adjs_gt, flags, flags_gt, Ke, mmd_kernels).items():
        res[f"edge_type_mmd_{kernel}"] = val
    for tag, d in (("val", val_d), ("train", train_d)):
        out = h.compute_triplet_tv_dist(adjs, nodes, flags, d, to_count)
        for key, v in zip(("tv_dist_rej", "tv_dist_all", "tv_dist_full", "novelty"), out):
            res[f"triplet_{key}_{tag}"] = v
    pred_bbox = cxcywh_to_xyxy(T(bg)).clip(min=0.0, max=1.0)
    gt_bbox = cxcywh_to_xyxy(T(br)).clip(min=0.0, max=1.0)
    blt = {}
    for key, kw in (("iou_blt", "flag_vanilla_iou"), ("iou_percp_blt", "flag_perceptual_iou"), ("overlap_blt", "flag_overlap"),
                    ("alignment_blt", "flag_alignment")):
        blt[f"pred_{key}"] = h.compute_bbox_ioa(pred_bbox, flags, canvas_size=32, return_mean=True, **{kw: True})
        blt[f"gt_{key}"] = h.compute_bbox_ioa(gt_bbox, flags_gt, canvas_size=32, return_mean=True, **{kw: True})
    res.update({k: blt[k] for k in sorted(blt, key=lambda k: not k.startswith("pred"))})    # the CSV lists pred, then gt (:649-656)
    weight_by_area, weight_by_freq = area / np.sum(area), freq / np.sum(freq)
    weights = [np.ones_like(weight_by_area), weight_by_area, weight_by_freq]
    mat_f1 = h.compute_bbox_f1(pred_bbox, nodes, flags, gt_bbox, nodes_gt, flags_gt, weights)
    vanilla, m_area, m_freq = [np.squeeze(arr, axis=2) for arr in np.dsplit(mat_f1, 3)]
    dummy_x_gen, dummy_x_gt = torch.ones_like(nodes) * flags, torch.ones_like(nodes_gt) * flags_gt    # mask_nodes(ones, flags)
    nt = h.compute_bbox_f1(pred_bbox, dummy_x_gen, flags, gt_bbox, dummy_x_gt, flags_gt, class_weight_ls=None).squeeze(2)
    res.update(_f1_summaries({"vanilla": vanilla, "area": m_area, "freq": m_freq, "no_node_type": nt}))
    res = {k: float(v) for k, v in res.items()}
    print("evaluate_samples:", res)
    assert len(res) == 32 and not any(np.isnan(v) for v in res.values())
    g["es_keys"], g["es_values"] = np.array(list(res.keys())), np.array(list(res.values()), np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference's DiffuseSG/ directory")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "eval_full.npz"))
    args = ap.parse_args()
    SGE, _ = _import_reference(args.ref)
    rng = np.random.default_rng(20261017)
    g = {}
    for name, N in (("vg", 62), ("coco", 33)):
        box, flag = _layout_set(rng, 40, N)
        _layout_case(SGE, g, name, box, flag)
    _triplet_case(SGE, g, rng)
    _f1_case(SGE, g, rng)
    _samples_case(SGE, g, rng)
    np.savez_compressed(args.out, **g)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")
    assert os.path.getsize(args.out) <= 200_000


if __name__ == "__main__":
    main()
