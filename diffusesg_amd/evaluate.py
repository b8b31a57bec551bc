"""On-device sample evaluation: a drop-in for the reference's SceneGraphEvaluator (R/evaluation/bbox_metrics.py).

SceneGraphEvaluatorHip: the metrics whose cost grows with (generated graphs) x (reference graphs) -- the bounding-box F1 matrix
and the Gaussian MMDs of the node-type, edge-type and node-degree histograms (csrc/eval_kernels.hip, pinned by
tests/golden/eval_metrics.npz).  SceneGraphEvaluatorHipFull adds the rest of what sg_go_sampling evaluates: the triplet TV
distances, the four layout metrics of compute_bbox_ioa and the row statistics of the F1 matrix (csrc/sgstat_kernels.hip, pinned
by tests/golden/eval_full.npz); evaluate_samples is that whole evaluation block as one call.  Entries: include/dsg.h ("Sample
evaluation", "Scene-graph statistics").  There is no CPU path: without the GPU every method fails."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import lib

# measure_two_sets_of_bboxes' default iou_range (bbox_metrics.py:64); passed to the device as these exact float64 values
IOU_THRESHOLDS = np.linspace(0.05, 0.5, 10)

_KERNELS = ("gaussian", "gaussian_emd", "gaussian_tv")

# device memory of one streamed block of F1 rows ([rows, Y, W] float64)
_F1_BLOCK_BYTES = 256 << 20


def cxcywh_to_xyxy(boxes):
    """torchvision.ops.box_convert(boxes, in_fmt='cxcywh', out_fmt='xyxy') (torchvision is not a dependency here): the same
    elementwise operations in the same order, so the same float32 results."""
    cx, cy, w, h = boxes.unbind(-1)
    return torch.stack((cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h), dim=-1)


def _device(*xs) -> torch.device:
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    if not torch.cuda.is_available():
        raise lib.DsgError("SceneGraphEvaluatorHip needs the MI355X: no GPU is visible (there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _tensor(x, dev) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        return x.to(dev)
    if isinstance(x, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    raise NotImplementedError(type(x))   # as the reference's _torch_to_numpy_helper


def _int32(x: torch.Tensor) -> torch.Tensor:
    if x.is_floating_point():
        x = torch.floor(x)   # torch.histogram's unit bins
    return x.to(torch.int32).contiguous()


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _check(rc: int, what: str):
    if rc != 0:
        raise lib.DsgError(f"{what}: status {rc}")


def _kernel_names(kernel_ls):
    names = kernel_ls if isinstance(kernel_ls, list) else [kernel_ls]
    assert all(k in _KERNELS for k in names)   # retrieve_kernerls (bbox_metrics.py:127-135)
    for k in names:
        if k != "gaussian":
            raise NotImplementedError(f"MMD kernel '{k}': only 'gaussian' runs on the device")
    return names


def _pad_nodes(x: torch.Tensor, n: int) -> torch.Tensor:
    """Zero-pad the node axis (dim 1) to n: padded nodes are unflagged."""
    if x.shape[1] == n:
        return x
    shape = list(x.shape)
    shape[1] = n - shape[1]
    return torch.cat([x, x.new_zeros(shape)], dim=1)


def _hist_mmd(ref: torch.Tensor, gen: torch.Tensor) -> np.float64:
    """compute_mmd(ref, gen, gaussian) of feature-major [L, n] float64 histograms (already normalised)."""
    L = max(ref.shape[0], gen.shape[0])
    ref = torch.nn.functional.pad(ref, (0, 0, 0, L - ref.shape[0])).contiguous()
    gen = torch.nn.functional.pad(gen, (0, 0, 0, L - gen.shape[0])).contiguous()
    dev = ref.device
    nr, ng = ref.shape[1], gen.shape[1]
    ws = torch.empty(2 * nr + ng, dtype=torch.float64, device=dev)
    out = torch.empty(4, dtype=torch.float64, device=dev)
    _check(lib.load().dsg_eval_hist_mmd(nr, ref.data_ptr(), nr, ng, gen.data_ptr(), ng, L, ws.data_ptr(), out.data_ptr(), _stream(dev)),
           "dsg_eval_hist_mmd")
    return np.float64(out.cpu().numpy()[0])


def _type_hist(types, flags, K: int, edges: bool, dev):
    """([K or K-1, B] float64 normalised histograms, [B] raw counts) of _get_node_type_hist / _get_edge_type_hist."""
    t = _int32(_tensor(types, dev))
    f = (_tensor(flags, dev) != 0).to(torch.uint8).contiguous()
    B, N = f.shape
    rows = K - 1 if edges else K
    hist = torch.empty(rows, B, dtype=torch.float64, device=dev)
    sums = torch.empty(B, dtype=torch.float64, device=dev)
    _check(lib.load().dsg_eval_type_hist(B, N, K, int(edges), t.data_ptr(), f.data_ptr(), hist.data_ptr(), B, sums.data_ptr(),
                                         _stream(dev)), "dsg_eval_type_hist")
    return hist, sums


def _degree_hist(adjs, dev):
    a = _tensor(adjs, dev).to(torch.float32).contiguous()
    B, N = a.shape[0], a.shape[-1]
    hist = torch.empty(N, B, dtype=torch.float64, device=dev)
    sums = torch.empty(B, dtype=torch.float64, device=dev)
    _check(lib.load().dsg_eval_degree_hist(B, N, a.data_ptr(), hist.data_ptr(), B, sums.data_ptr(), _stream(dev)), "dsg_eval_degree_hist")
    return hist


class _BoxSet:
    """One scene set prepared on the device (dsg_eval_bbox_prep)."""

    def __init__(self, boxes, types, flags, N, n_classes, weights, dev):
        L = lib.load()
        self.S = int(flags.shape[0])
        b = _pad_nodes(boxes.to(torch.float32), N).contiguous()
        t = _pad_nodes(_int32(types), N).contiguous()
        f = _pad_nodes((flags != 0).to(torch.uint8), N).contiguous()
        W = 1 if weights is None else weights.shape[0]
        self.buf = torch.empty(L.dsg_eval_bbox_prep_bytes(self.S, N, W), dtype=torch.uint8, device=dev)
        _check(L.dsg_eval_bbox_prep(self.S, N, n_classes, b.data_ptr(), t.data_ptr(), f.data_ptr(), W,
                                    None if weights is None else weights.data_ptr(), self.buf.data_ptr(), _stream(dev)),
               "dsg_eval_bbox_prep")


def _f1_blocks(node_bbox_gen, node_types_gen, node_flags_gen, node_bbox_ref, node_types_ref, node_flags_ref, class_weight_ls):
    """(X, Y, W, blocks) of one compute_bbox_f1 call: `blocks` yields (x0, x1, device block [rows, Y, W] float64) for consecutive
    rows of the F1 matrix, each valid until the next one is asked for; None when either set is empty."""
    dev = _device(node_bbox_gen, node_types_gen, node_flags_gen, node_bbox_ref, node_types_ref, node_flags_ref)
    bg, tg, fg, br, tr, fr = (_tensor(x, dev) for x in (node_bbox_gen, node_types_gen, node_flags_gen, node_bbox_ref,
                                                        node_types_ref, node_flags_ref))
    X, Y = int(fg.shape[0]), int(fr.shape[0])
    W = 1 if class_weight_ls is None else len(class_weight_ls)
    if X == 0 or Y == 0:
        return X, Y, W, None
    fg, fr = fg != 0, fr != 0
    if class_weight_ls is not None:
        assert tr.max() <= len(class_weight_ls[0]), "The number of classes in the ground truth set is larger than the number of classes in the dataset."
        assert tg.max() <= len(class_weight_ls[0]), "The number of classes in the generated set is larger than the number of classes in the dataset."
    used = torch.cat([tg[fg].reshape(-1), tr[fr].reshape(-1)])
    lo = int(used.min()) if used.numel() else 0
    hi = int(used.max()) if used.numel() else 0
    if lo < 0:
        raise ValueError(f"negative class id {lo} on a flagged node")
    if class_weight_ls is not None:
        n_classes = len(class_weight_ls[0])
        if hi >= n_classes:
            raise IndexError(f"class id {hi} has no class weight ({n_classes} classes)")
        weights = torch.as_tensor(np.stack([np.asarray(w, dtype=np.float64) for w in class_weight_ls]), device=dev).contiguous()
    else:
        n_classes, weights = hi + 1, None
    if n_classes > 192:
        raise ValueError(f"{n_classes} classes: the device evaluator covers up to 192")
    N = max(int(fg.shape[1]), int(fr.shape[1]))
    if N > 255:
        raise ValueError(f"{N} nodes: the device evaluator covers up to 255")
    gen = _BoxSet(bg, tg, fg, N, n_classes, weights, dev)
    ref = _BoxSet(br, tr, fr, N, n_classes, weights, dev)

    def blocks():
        thr = (C.c_double * len(IOU_THRESHOLDS))(*IOU_THRESHOLDS.tolist())
        rows = max(1, min(X, _F1_BLOCK_BYTES // (Y * W * 8)))
        blk = torch.empty(rows, Y, W, dtype=torch.float64, device=dev)
        L = lib.load()
        for x0 in range(0, X, rows):
            x1 = min(X, x0 + rows)
            _check(L.dsg_eval_bbox_f1(gen.buf.data_ptr(), X, ref.buf.data_ptr(), Y, N, n_classes, W,
                                      None if weights is None else weights.data_ptr(), len(IOU_THRESHOLDS), thr, x0, x1, 0, Y,
                                      blk.data_ptr(), _stream(dev)), "dsg_eval_bbox_f1")
            yield x0, x1, blk

    return X, Y, W, blocks()


def hip_evaluator(base, full=False):
    """`base` (the reference's SceneGraphEvaluator class) with its four pairwise metrics replaced by the device ones below; every
    other method (compute_bbox_ioa, compute_triplet_tv_dist, ...) stays the reference's own.  Usage in the reference:
    `eval_helper = hip_evaluator(SceneGraphEvaluator)()`.  With full=True compute_triplet_tv_dist and compute_bbox_ioa are the
    device ones of SceneGraphEvaluatorHipFull too, and compute_bbox_f1_stats is added."""
    if full:
        return type(base.__name__ + "HipFull", (SceneGraphEvaluatorHipFull, base), {})
    return type(base.__name__ + "Hip", (SceneGraphEvaluatorHip, base), {})


class SceneGraphEvaluatorHip:
    """SceneGraphEvaluator's pairwise metrics on the GPU: the same static methods, argument lists and return types
    (R/evaluation/bbox_metrics.py:283-440).  Inputs may be torch tensors (CPU or CUDA) or numpy arrays."""

    @staticmethod
    def compute_bbox_f1(node_bbox_gen, node_types_gen, node_flags_gen, node_bbox_ref, node_types_ref, node_flags_ref,
                        class_weight_ls=None):
        """[X, Y, W] float64 numpy: mean F1 over the IoU thresholds between generated scene x and reference scene y for each
        class-weight vector (W = 1 without weights).  Boxes x1 y1 x2 y2 (float32 on the device), [B, N, 4]."""
        X, Y, W, blocks = _f1_blocks(node_bbox_gen, node_types_gen, node_flags_gen, node_bbox_ref, node_types_ref, node_flags_ref,
                                     class_weight_ls)
        if blocks is None:
            return np.zeros((X, Y, W))
        out = np.empty((X, Y, W), dtype=np.float64)
        for x0, x1, blk in blocks:
            out[x0:x1] = blk[: x1 - x0].cpu().numpy()
        return out

    @staticmethod
    def compute_node_type_mmd(node_types_gen, node_types_ref, node_flags_gen, node_flags_ref, num_node_types: int, kernel_ls):
        """{'gaussian': mmd} of the per-graph node-type histograms (bbox_metrics.py:300-323)."""
        names = _kernel_names(kernel_ls)
        dev = _device(node_types_gen, node_types_ref, node_flags_gen, node_flags_ref)
        h_ref, s_ref = _type_hist(node_types_ref, node_flags_ref, num_node_types, False, dev)
        h_gen, s_gen = _type_hist(node_types_gen, node_flags_gen, num_node_types, False, dev)
        assert s_ref.sum().item() == (_tensor(node_flags_ref, dev) != 0).sum().item()   # sanity check
        assert s_gen.sum().item() == (_tensor(node_flags_gen, dev) != 0).sum().item()   # sanity check
        return {k: _hist_mmd(h_ref, h_gen) for k in names}

    @staticmethod
    def compute_edge_type_mmd(edge_types_gen, edge_types_ref, node_flags_gen, node_flags_ref, num_edge_types: int, kernel_ls):
        """{'gaussian': mmd} of the per-graph edge-type histograms (bbox_metrics.py:325-348); graphs without an edge are left
        out, and -1.0 when either side has none left."""
        names = _kernel_names(kernel_ls)
        dev = _device(edge_types_gen, edge_types_ref, node_flags_gen, node_flags_ref)
        h_ref, s_ref = _type_hist(edge_types_ref, node_flags_ref, num_edge_types, True, dev)
        h_gen, s_gen = _type_hist(edge_types_gen, node_flags_gen, num_edge_types, True, dev)
        h_ref, h_gen = h_ref[:, s_ref > 0], h_gen[:, s_gen > 0]
        if h_ref.shape[1] == 0 or h_gen.shape[1] == 0:
            return {k: -1.0 for k in names}
        return {k: _hist_mmd(h_ref, h_gen) for k in names}

    @staticmethod
    def compute_node_degree_mmd(edge_types_gen, edge_types_ref, kernel_ls):
        """{'gaussian': {'degree': mmd, 'average': mmd}} (bbox_metrics.py:285-298 through eval_torch_batch, stats.py:284-296)."""
        names = _kernel_names(kernel_ls)
        dev = _device(edge_types_gen, edge_types_ref)
        h_ref, h_gen = _degree_hist(edge_types_ref, dev), _degree_hist(edge_types_gen, dev)
        out = {}
        for k in names:
            v = _hist_mmd(h_ref, h_gen)
            out[k] = {"degree": v, "average": np.mean([v])}
        return out


# ---------------------------------------------------------------------------------------------------------------------------
# the rest of sg_go_sampling's evaluation: triplet TV, layout metrics, F1 row statistics (csrc/sgstat_kernels.hip)
# ---------------------------------------------------------------------------------------------------------------------------
_KEY_BITS = 21            # bits per field of a packed triplet key (kSgstatKeyBits)
_ROWSTATS_MAX_Y = 16384   # an F1 row held in LDS (kSgstatMaxRow); longer rows are reduced by NumPy on the host
_LAYOUT_METRICS = ("vanilla_iou", "perceptual_iou", "overlap", "alignment")   # row order of dsg_sgstat_layout's output


def _integral(x, dev, what) -> torch.Tensor:
    t = _tensor(x, dev)
    if t.is_floating_point() and not bool((t == torch.floor(t)).all()):
        raise ValueError(f"{what} must be integer-valued")
    return t


def _in_key_range(t: torch.Tensor, what):
    if t.numel() and (t.min().item() < 0 or t.max().item() >= 1 << _KEY_BITS):
        raise ValueError(f"{what} outside [0, 2^{_KEY_BITS}): not representable in a packed triplet key")


def _pack_triplet_keys(keys):
    """(sorted packed keys int64, position of each among the usable keys int32, indices of the usable keys in `keys`' order); a
    key that no integer triplet in range can equal is not usable (its count stays 0)."""
    arr = np.array([tuple(k) for k in keys]).reshape(-1, 3)
    ok = np.ones(len(arr), dtype=bool)
    if arr.dtype.kind == "f":
        ok &= (arr == np.floor(arr)).all(1)
        arr = np.where(ok[:, None], arr, 0)
    arr = arr.astype(np.int64)
    ok &= ((arr >= 0) & (arr < 1 << _KEY_BITS)).all(1)
    usable = np.flatnonzero(ok)
    packed = (arr[:, 0] << (2 * _KEY_BITS) | arr[:, 1] << _KEY_BITS | arr[:, 2])[usable]
    order = np.argsort(packed, kind="stable")
    return packed[order], order.astype(np.int32), usable


def triplet_counts(edge_types, node_types, triplet_keys):
    """(counts int64 [len(triplet_keys)] in the keys' order, novel int): _get_triplet_type_hist summed over the graphs.  Every
    non-zero entry of edge_types [B, N, N] is the triplet (node_types[b, i], node_types[b, j], edge_types[b, i, j]); node flags
    play no part and a diagonal entry counts, as in the reference."""
    dev = _device(edge_types, node_types)
    e = _integral(edge_types, dev, "edge_types")
    t = _integral(node_types, dev, "node_types")
    keys = list(triplet_keys)
    counts = np.zeros(len(keys), dtype=np.int64)
    if e.numel() == 0:
        return counts, 0
    _in_key_range(e, "edge type")
    nz = e != 0
    _in_key_range(t[nz.any(2) | nz.any(1)], "node type of an edge")
    B, N = int(e.shape[0]), int(e.shape[-1])
    e, t = e.to(torch.int32).contiguous(), t.to(torch.int32).contiguous()
    sk, pos, usable = _pack_triplet_keys(keys) if keys else (np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int64))
    n = len(sk)
    d_keys, d_pos = torch.from_numpy(sk).to(dev), torch.from_numpy(pos).to(dev)
    out = torch.empty(n + 1, dtype=torch.int64, device=dev)   # counts of the usable keys, then novel
    _check(lib.load().dsg_sgstat_triplet_counts(B, N, e.data_ptr(), t.data_ptr(), n, d_keys.data_ptr() if n else None,
                                                d_pos.data_ptr() if n else None, out.data_ptr() if n else None,
                                                out.data_ptr() + 8 * n, _stream(dev)), "dsg_sgstat_triplet_counts")
    host = out.cpu().numpy()
    counts[usable] = host[:-1]
    return counts, int(host[-1])


def triplet_tv_from_counts(counts, novel, triplet_dict, triplet_to_count):
    """The four values of compute_triplet_tv_dist from the summed histogram: bbox_metrics.py:350-369, where the per-graph novel
    columns are only ever summed, so their total stands in for them."""
    n = len(counts)
    tv_pred_triplet_hist_rej = counts / np.sum(counts) if counts.sum() > 0 else np.zeros(n)
    total = counts.sum() + novel
    tv_pred_triplet_hist_all = np.concatenate([counts, [novel]]) / total if total > 0 else np.zeros(n)
    tv_gt_triplet_hist = np.array(list(triplet_dict.values()))
    diff_rej = tv_gt_triplet_hist - tv_pred_triplet_hist_rej
    diff_all = tv_gt_triplet_hist - tv_pred_triplet_hist_all[:len(tv_gt_triplet_hist)]
    diff_full = np.concatenate([diff_all, tv_pred_triplet_hist_all[len(tv_gt_triplet_hist):]])
    triplet_tv_dist_rej = np.abs(diff_rej[:len(triplet_to_count)]).sum()
    triplet_tv_dist_all = np.abs(diff_all[:len(triplet_to_count)]).sum()
    triplet_tv_dist_full = np.abs(diff_full).sum()
    triplet_novelty = np.abs(tv_pred_triplet_hist_all[len(tv_gt_triplet_hist):]).sum()
    return triplet_tv_dist_rej, triplet_tv_dist_all, triplet_tv_dist_full, triplet_novelty


def layout_metrics(bbox_ls, node_flags, canvas_size=32, check_perceptual=False):
    """(values [4, B] float64, valid [4, B] bool) in the order of _LAYOUT_METRICS: all four per-layout metrics of
    compute_bbox_ioa in one launch; valid is False where the reference's function returns None.  check_perceptual applies
    get_perceptual_iou's own input checks (AssertionError for a coordinate outside [0, 1], ValueError for an empty layout)."""
    dev = _device(bbox_ls, node_flags)
    b = _tensor(bbox_ls, dev).to(torch.float32).contiguous()
    f = (_tensor(node_flags, dev) != 0)
    B, N = int(f.shape[0]), int(f.shape[1])
    if not 1 <= int(canvas_size) <= 64:
        raise ValueError(f"canvas_size {canvas_size}: the device evaluator covers 1..64")
    if N > 255:
        raise ValueError(f"{N} nodes: the device evaluator covers up to 255")
    if B == 0 or N == 0:
        if check_perceptual and B:
            raise ValueError("zero-size array to reduction operation minimum which has no identity")
        return np.zeros((4, B)), np.zeros((4, B), dtype=bool)
    if check_perceptual:
        empty = ~f.any(1)
        bad = (~((b >= 0) & (b <= 1)).all(-1) & f).any(1)
        first = torch.stack([empty, bad]).cpu().numpy()
        if first.any():
            i = int(np.flatnonzero(first.any(0))[0])
            if first[0, i]:
                raise ValueError("zero-size array to reduction operation minimum which has no identity")   # layout.min()
            raise AssertionError(f"layout {i}: coordinates outside [0, 1]")
    values = torch.empty(4, B, dtype=torch.float64, device=dev)
    valid = torch.empty(4, B, dtype=torch.uint8, device=dev)
    f8 = f.to(torch.uint8).contiguous()
    _check(lib.load().dsg_sgstat_layout(B, N, b.data_ptr(), f8.data_ptr(), int(canvas_size), values.data_ptr(), valid.data_ptr(),
                                        _stream(dev)), "dsg_sgstat_layout")
    return values.cpu().numpy(), valid.cpu().numpy() != 0


def _f1_row_stats(blk: torch.Tensor, mx, mean, med, arg):
    """max / mean / median / arg-max over axis 1 of a device block [rows, Y, W] into the [rows, W] device tensors."""
    rows, Y, W = blk.shape
    if Y <= _ROWSTATS_MAX_Y:
        _check(lib.load().dsg_sgstat_f1_rowstats(rows, Y, W, blk.data_ptr(), mx.data_ptr(), mean.data_ptr(), med.data_ptr(),
                                                 arg.data_ptr(), _stream(blk.device)), "dsg_sgstat_f1_rowstats")
        return
    m = blk.cpu().numpy()   # a row too long for LDS: the copy and NumPy
    for dst, v in ((mx, m.max(1)), (mean, m.mean(1)), (med, np.median(m, 1)), (arg, m.argmax(1).astype(np.int32))):
        dst.copy_(torch.from_numpy(v))


class SceneGraphEvaluatorHipFull(SceneGraphEvaluatorHip):
    """SceneGraphEvaluatorHip plus the remaining methods sg_go_sampling calls, with the reference's argument lists
    (R/evaluation/bbox_metrics.py:337-376, 443-483): `hip_evaluator(SceneGraphEvaluator, full=True)()`."""

    @staticmethod
    def compute_triplet_tv_dist(edge_types_gen, node_types_gen, node_flags_gen, triplet_dict, triplet_to_count):
        """(triplet_tv_dist_rej, triplet_tv_dist_all, triplet_tv_dist_full, triplet_novelty).  As in the reference node_flags_gen
        is not used and a diagonal entry of edge_types_gen is a triplet.  Inputs must be integer-valued: a non-integral float
        raises ValueError (the reference would count it as a novel triplet), and so does an edge type, or the node type of an
        edge's end, outside [0, 2^21)."""
        counts, novel = triplet_counts(edge_types_gen, node_types_gen, triplet_dict.keys())
        return triplet_tv_from_counts(counts, novel, triplet_dict, triplet_to_count)

    @staticmethod
    def compute_bbox_ioa(bbox_ls, node_flags, canvas_size=32, flag_vanilla_iou=False, flag_perceptual_iou=False, flag_overlap=False,
                         flag_alignment=False, return_mean=False):
        """The per-layout values (float64; the reference's IoU and overlap are float32 sums of the same pair terms) of the one
        metric whose flag is set, layouts for which the reference returns None dropped; or their np.mean.  Boxes x1 y1 x2 y2,
        [B, N, 4]; up to 255 nodes, canvas_size 1..64."""
        flags = [flag_vanilla_iou, flag_perceptual_iou, flag_overlap, flag_alignment]
        assert sum(flags) == 1, "Only one flag can be True."
        m = [bool(x) for x in flags].index(True)
        values, valid = layout_metrics(bbox_ls, node_flags, canvas_size, check_perceptual=bool(flag_perceptual_iou))
        metric_per_bbox_ls = list(values[m][valid[m]])
        if return_mean:
            return np.mean(metric_per_bbox_ls)
        return metric_per_bbox_ls

    @staticmethod
    def compute_bbox_f1_stats(node_bbox_gen, node_types_gen, node_flags_gen, node_bbox_ref, node_types_ref, node_flags_ref,
                              class_weight_ls=None, return_matrix=False):
        """{'max', 'mean', 'median' (float64), 'argmax' (int64)}, each [X, W]: the reductions over the reference axis of
        compute_bbox_f1's matrix (.max(1), .mean(1), np.median(., 1), .argmax(1)), taken on the device block by block; the matrix
        itself comes to the host only with return_matrix=True (key 'matrix')."""
        X, Y, W, blocks = _f1_blocks(node_bbox_gen, node_types_gen, node_flags_gen, node_bbox_ref, node_types_ref, node_flags_ref,
                                     class_weight_ls)
        if Y == 0:
            raise ValueError("zero-size array to reduction operation maximum which has no identity")
        out = {"max": np.zeros((X, W)), "mean": np.zeros((X, W)), "median": np.zeros((X, W)), "argmax": np.zeros((X, W), np.int64)}
        if return_matrix:
            out["matrix"] = np.zeros((X, Y, W))
        if blocks is None:
            return out
        mx = mean = med = arg = None
        for x0, x1, blk in blocks:
            if mx is None:
                mx, mean, med = (torch.empty(X, W, dtype=torch.float64, device=blk.device) for _ in range(3))
                arg = torch.empty(X, W, dtype=torch.int32, device=blk.device)
            _f1_row_stats(blk[: x1 - x0], mx[x0:x1], mean[x0:x1], med[x0:x1], arg[x0:x1])
            if return_matrix:
                out["matrix"][x0:x1] = blk[: x1 - x0].cpu().numpy()
        out.update(max=mx.cpu().numpy(), mean=mean.cpu().numpy(), median=med.cpu().numpy(), argmax=arg.cpu().numpy().astype(np.int64))
        return out


def evaluate_samples(adjs_gen, nodes_gen, bbox_gen, flags_gen, adjs_gt, nodes_gt, bbox_gt, flags_gt, num_node_types, num_edge_types,
                     val_triplet_dict, train_triplet_dict, triplet_to_count, weight_by_area, weight_by_freq, canvas_size=32):
    """The evaluation block of sg_go_sampling (R/runner/sampler/sampler_node_adj.py:445-552) on the device, as one call: a dict
    with the keys the reference writes to eval_results.csv (:627-669).

    adjs_* [B, N, N] decoded edge types, nodes_* [B, N] decoded node types, bbox_* [B, N, 4] cxcywh boxes, flags_* [B, N]; torch
    tensors (CPU or CUDA) or numpy arrays.  *_triplet_dict: {(subject type, object type, predicate): frequency} of the validation
    and training sets; triplet_to_count: the triplets of the truncated distances (only its length is used, as in the reference).
    weight_by_area / weight_by_freq: per node type, normalised here to sum to 1 as lines 508-512 do."""
    H = SceneGraphEvaluatorHipFull
    dev = _device(adjs_gen, nodes_gen, bbox_gen, flags_gen, adjs_gt, nodes_gt, bbox_gt, flags_gt)
    adjs_gen, nodes_gen, bbox_gen, flags_gen, adjs_gt, nodes_gt, bbox_gt, flags_gt = (
        _tensor(x, dev) for x in (adjs_gen, nodes_gen, bbox_gen, flags_gen, adjs_gt, nodes_gt, bbox_gt, flags_gt))
    mmd_kernels = ["gaussian"]
    res = {}
    for kernel, val_par in H.compute_node_degree_mmd(adjs_gen, adjs_gt, mmd_kernels).items():
        for key, val in val_par.items():
            res[f"node_{key}_mmd_{kernel}"] = val
    for kernel, val in H.compute_node_type_mmd(nodes_gen, nodes_gt, flags_gen, flags_gt, num_node_types, mmd_kernels).items():
        res[f"node_type_mmd_{kernel}"] = val
    for kernel, val in H.compute_edge_type_mmd(adjs_gen, adjs_gt, flags_gen, flags_gt, num_edge_types, mmd_kernels).items():
        res[f"edge_type_mmd_{kernel}"] = val

    # one histogram per dictionary; both are counted from the same generated graphs
    for tag, triplet_dict in (("val", val_triplet_dict), ("train", train_triplet_dict)):
        rej, all_, full, novelty = H.compute_triplet_tv_dist(adjs_gen, nodes_gen, flags_gen, triplet_dict, triplet_to_count)
        res.update({f"triplet_tv_dist_rej_{tag}": rej, f"triplet_tv_dist_all_{tag}": all_, f"triplet_tv_dist_full_{tag}": full,
                    f"triplet_novelty_{tag}": novelty})

    # always xyxy for the bounding-box metrics (:479-480)
    pred_bbox = cxcywh_to_xyxy(bbox_gen.to(torch.float32)).clip(min=0.0, max=1.0)
    gt_bbox = cxcywh_to_xyxy(bbox_gt.to(torch.float32)).clip(min=0.0, max=1.0)
    for tag, box, flags in (("pred", pred_bbox, flags_gen), ("gt", gt_bbox, flags_gt)):
        values, valid = layout_metrics(box, flags, canvas_size, check_perceptual=True)   # the four metrics from one launch
        for m, key in enumerate(("iou_blt", "iou_percp_blt", "overlap_blt", "alignment_blt")):
            res[f"{tag}_{key}"] = np.mean(list(values[m][valid[m]]))

    weight_by_area = np.asarray(weight_by_area, dtype=np.float64)
    weight_by_area = weight_by_area / np.sum(weight_by_area)
    weight_by_freq = np.asarray(weight_by_freq, dtype=np.float64)
    weight_by_freq = weight_by_freq / np.sum(weight_by_freq)
    weights = [np.ones_like(weight_by_area), weight_by_area, weight_by_freq]
    st = H.compute_bbox_f1_stats(pred_bbox, nodes_gen, flags_gen, gt_bbox, nodes_gt, flags_gt, weights)
    dummy_x_gen = torch.ones_like(nodes_gen) * (flags_gen != 0)   # mask_nodes(torch.ones_like(.), flags)
    dummy_x_gt = torch.ones_like(nodes_gt) * (flags_gt != 0)
    nt = H.compute_bbox_f1_stats(pred_bbox, dummy_x_gen, flags_gen, gt_bbox, dummy_x_gt, flags_gt, class_weight_ls=None)
    for name, s, w in (("vanilla", st, 0), ("area", st, 1), ("freq", st, 2), ("no_node_type", nt, 0)):
        for key in ("max", "mean", "median"):
            res[f"{name}_f1_avg_{key}"] = s[key][:, w].mean()
    return res
