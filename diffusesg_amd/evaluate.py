"""On-device sample evaluation: a drop-in for the reference's SceneGraphEvaluator (R/evaluation/bbox_metrics.py) for the
metrics whose cost grows with (generated graphs) x (reference graphs): the bounding-box F1 matrix and the Gaussian MMDs of
the node-type, edge-type and node-degree histograms.  Kernels: csrc/eval_kernels.hip through include/dsg.h ("Sample
evaluation"); pinned to the reference by tests/golden/eval_metrics.npz.  There is no CPU path: without the GPU every method
fails."""
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


def hip_evaluator(base):
    """`base` (the reference's SceneGraphEvaluator class) with its four pairwise metrics replaced by the device ones below; every
    other method (compute_bbox_ioa, compute_triplet_tv_dist, ...) stays the reference's own.  Usage in the reference:
    `eval_helper = hip_evaluator(SceneGraphEvaluator)()`."""
    return type(base.__name__ + "Hip", (SceneGraphEvaluatorHip, base), {})


class SceneGraphEvaluatorHip:
    """SceneGraphEvaluator's pairwise metrics on the GPU: the same static methods, argument lists and return types
    (R/evaluation/bbox_metrics.py:283-440).  Inputs may be torch tensors (CPU or CUDA) or numpy arrays."""

    @staticmethod
    def compute_bbox_f1(node_bbox_gen, node_types_gen, node_flags_gen, node_bbox_ref, node_types_ref, node_flags_ref,
                        class_weight_ls=None):
        """[X, Y, W] float64 numpy: mean F1 over the IoU thresholds between generated scene x and reference scene y for each
        class-weight vector (W = 1 without weights).  Boxes x1 y1 x2 y2 (float32 on the device), [B, N, 4]."""
        dev = _device(node_bbox_gen, node_types_gen, node_flags_gen, node_bbox_ref, node_types_ref, node_flags_ref)
        bg, tg, fg, br, tr, fr = (_tensor(x, dev) for x in (node_bbox_gen, node_types_gen, node_flags_gen, node_bbox_ref,
                                                            node_types_ref, node_flags_ref))
        X, Y = int(fg.shape[0]), int(fr.shape[0])
        W = 1 if class_weight_ls is None else len(class_weight_ls)
        if X == 0 or Y == 0:
            return np.zeros((X, Y, W))
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
        thr = (C.c_double * len(IOU_THRESHOLDS))(*IOU_THRESHOLDS.tolist())
        out = np.empty((X, Y, W), dtype=np.float64)
        rows = max(1, min(X, _F1_BLOCK_BYTES // (Y * W * 8)))
        blk = torch.empty(rows, Y, W, dtype=torch.float64, device=dev)
        L = lib.load()
        for x0 in range(0, X, rows):
            x1 = min(X, x0 + rows)
            _check(L.dsg_eval_bbox_f1(gen.buf.data_ptr(), X, ref.buf.data_ptr(), Y, N, n_classes, W,
                                      None if weights is None else weights.data_ptr(), len(IOU_THRESHOLDS), thr, x0, x1, 0, Y,
                                      blk.data_ptr(), _stream(dev)), "dsg_eval_bbox_f1")
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
