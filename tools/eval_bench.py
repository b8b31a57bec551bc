#!/usr/bin/env python3
"""Time the on-device sample evaluation (diffusesg_amd.evaluate) at X generated x Y reference scene graphs on one GPU.
Reports only, gates nothing.

  * bbox F1: the matrix kernel alone (device events around dsg_eval_bbox_f1 over the whole [X, Y] window), and the whole
    SceneGraphEvaluatorHip.compute_bbox_f1 call (prep, kernel, copy of the float64 matrix to the host), for the weighted call of
    sg_go_sampling (three class-weight vectors, 150 VG-like classes) and its "no node type" call (one class, no weights).
  * node-type, edge-type and node-degree MMD: the whole call each.
  * the rest of sg_go_sampling's evaluation (SceneGraphEvaluatorHipFull): the whole calls of compute_bbox_ioa (one metric, and
    the four from one launch), compute_triplet_tv_dist (--triplet-keys random keys over 150 node types x 50 predicates),
    compute_bbox_f1_stats (weighted and "no node type"), and evaluate_samples (the whole block from device tensors).

Inputs: VG-like scenes (N = 62) from a fixed seed: references random, generated ones perturbed copies of random references.
--classes-used K draws the classes from K of the 150 (fewer: more same-class boxes at the same node, i.e. more IoUs per pair).

Usage:  python tools/eval_bench.py [--x 4096] [--y 4096] [--reps 3] [--classes-used 150] [--triplet-keys 20000]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffusesg_amd import lib                                                          # noqa: E402
from diffusesg_amd import evaluate as E                                                # noqa: E402
from diffusesg_amd.evaluate import SceneGraphEvaluatorHip as SGE, cxcywh_to_xyxy       # noqa: E402
from diffusesg_amd.evaluate import SceneGraphEvaluatorHipFull as SGF, evaluate_samples  # noqa: E402


def scenes(rng, X, Y, N, n_cls, dev, used):
    box = cxcywh_to_xyxy(torch.from_numpy(np.concatenate([rng.uniform(0, 1, (Y, N, 2)), rng.uniform(0.02, 0.5, (Y, N, 2))], -1)
                                          .astype(np.float32))).clamp(0.0, 1.0)
    palette = rng.choice(n_cls, used, replace=False)
    cls = torch.from_numpy(rng.choice(palette, (Y, N)))
    flag = torch.from_numpy((np.arange(N)[None] < rng.integers(1, N + 1, Y)[:, None]).astype(np.float32))
    src = torch.from_numpy(rng.integers(0, Y, X))
    gbox = (box[src] + torch.from_numpy(rng.normal(0, 0.02, (X, N, 4)).astype(np.float32))).clamp(0.0, 1.0)
    gcls = torch.where(torch.from_numpy(rng.uniform(size=(X, N)) < 0.2), torch.from_numpy(rng.choice(palette, (X, N))), cls[src])
    return [t.to(dev) for t in (gbox, gcls, flag[src], box, cls, flag)]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--x", type=int, default=4096)
    ap.add_argument("--y", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--classes-used", type=int, default=150, help="classes the scenes draw from (fewer: more same-class matches per pair)")
    ap.add_argument("--triplet-keys", type=int, default=20000, help="keys of the triplet dictionary")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "eval_bench needs the GPU"
    dev = torch.device("cuda:0")
    X, Y, N, n_cls, reps = args.x, args.y, 62, 150, args.reps
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    a = scenes(rng, X, Y, N, n_cls, dev, args.classes_used)
    w = [np.ones(n_cls), rng.uniform(0, 1, n_cls), rng.uniform(0, 1, n_cls)]
    res = {"X": X, "Y": Y, "N": N, "classes": n_cls, "classes_used": args.classes_used, "gpu": torch.cuda.get_device_name(0)}

    # kernel alone: one launch over the whole window, device events
    wt = torch.from_numpy(np.stack(w)).to(dev)
    gen = E._BoxSet(a[0], a[1], a[2] != 0, N, n_cls, wt, dev)
    ref = E._BoxSet(a[3], a[4], a[5] != 0, N, n_cls, wt, dev)
    out = torch.empty(X, Y, 3, dtype=torch.float64, device=dev)
    thr = (C.c_double * 10)(*E.IOU_THRESHOLDS.tolist())
    L = lib.load()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    launch = lambda: L.dsg_eval_bbox_f1(gen.buf.data_ptr(), X, ref.buf.data_ptr(), Y, N, n_cls, 3, wt.data_ptr(), 10, thr, 0, X, 0, Y,
                                        out.data_ptr(), stream)
    assert launch() == 0
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ks = []
    for _ in range(reps):
        ev[0].record()
        launch()
        ev[1].record()
        torch.cuda.synchronize()
        ks.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    res["f1_kernel_s"] = min(ks)
    res["f1_kernel_pairs_per_s"] = X * Y / min(ks)
    res["f1_mean"] = float(out[..., 0].mean())
    res["f1_nonzero_share"] = float((out[..., 0] > 0).double().mean())

    t, _ = timed(lambda: SGE.compute_bbox_f1(*a, w), reps)
    res["f1_call_weighted_s"] = t
    res["f1_call_weighted_pairs_per_s"] = X * Y / t
    ones_g, ones_r = torch.ones_like(a[1]), torch.ones_like(a[4])
    t, _ = timed(lambda: SGE.compute_bbox_f1(a[0], ones_g, a[2], a[3], ones_r, a[5], None), reps)
    res["f1_call_no_node_type_s"] = t
    res["f1_call_no_node_type_pairs_per_s"] = X * Y / t

    Ke = 51
    adj_r = torch.where(torch.rand(Y, N, N, device=dev) < 0.03, torch.randint(1, Ke, (Y, N, N), device=dev), 0)
    adj_g = torch.where(torch.rand(X, N, N, device=dev) < 0.03, torch.randint(1, Ke, (X, N, N), device=dev), 0)
    adj_r, adj_g = adj_r.triu(1) + adj_r.triu(1).transpose(1, 2), adj_g.triu(1) + adj_g.triu(1).transpose(1, 2)
    res["mmd_node_type_s"], _ = timed(lambda: SGE.compute_node_type_mmd(a[1], a[4], a[2], a[5], n_cls, ["gaussian"]), reps)
    res["mmd_edge_type_s"], _ = timed(lambda: SGE.compute_edge_type_mmd(adj_g, adj_r, a[2], a[5], Ke, ["gaussian"]), reps)
    res["mmd_degree_s"], _ = timed(lambda: SGE.compute_node_degree_mmd(adj_g, adj_r, ["gaussian"]), reps)

    # the rest of the evaluation block: whole calls
    for metric in ("vanilla_iou", "perceptual_iou", "overlap", "alignment"):
        res[f"ioa_{metric}_s"], _ = timed(lambda: SGF.compute_bbox_ioa(a[0], a[2], canvas_size=32, return_mean=True, **{"flag_" + metric: True}), reps)
    res["ioa_four_metrics_s"], _ = timed(lambda: E.layout_metrics(a[0], a[2], 32, check_perceptual=True), reps)
    n_pred = Ke - 1
    ids = rng.choice(n_cls * n_cls * n_pred, args.triplet_keys, replace=False)
    freq = rng.integers(1, 500, args.triplet_keys).astype(np.float64)
    keys = zip((ids // (n_cls * n_pred)).tolist(), (ids // n_pred % n_cls).tolist(), (ids % n_pred + 1).tolist())
    triplet_dict = dict(zip(keys, (freq / freq.sum()).tolist()))
    to_count = list(triplet_dict.keys())[:1000]
    res["triplet_keys"] = len(triplet_dict)
    res["triplet_tv_s"], _ = timed(lambda: SGF.compute_triplet_tv_dist(adj_g, a[1], a[2], triplet_dict, to_count), reps)
    res["triplet_novelty"] = float(SGF.compute_triplet_tv_dist(adj_g, a[1], a[2], triplet_dict, to_count)[3])
    res["f1_stats_weighted_s"], _ = timed(lambda: SGF.compute_bbox_f1_stats(*a, w), reps)
    res["f1_stats_no_node_type_s"], _ = timed(lambda: SGF.compute_bbox_f1_stats(a[0], ones_g, a[2], a[3], ones_r, a[5], None), reps)
    to_cxcywh = lambda b: torch.cat([(b[..., :2] + b[..., 2:]) / 2, b[..., 2:] - b[..., :2]], -1)
    res["evaluate_samples_s"], _ = timed(lambda: evaluate_samples(adj_g, a[1], to_cxcywh(a[0]), a[2], adj_r, a[4], to_cxcywh(a[3]), a[5], n_cls,
                                                                  Ke, triplet_dict, triplet_dict, to_count, w[1], w[2]), reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
