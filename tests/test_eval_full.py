"""The rest of the on-device evaluation (diffusesg_amd.evaluate.SceneGraphEvaluatorHipFull and evaluate_samples,
csrc/sgstat_kernels.hip) against the reference's SceneGraphEvaluator as recorded in tests/golden/eval_full.npz
(tools/gen_eval_full_golden.py): the layout metrics of compute_bbox_ioa, compute_triplet_tv_dist, the F1 row statistics and the
whole evaluation block of sg_go_sampling.

CPU: the new C entries are declared, exported and loadable, and a NumPy restatement of the reference's algorithms (kept in this
file, written from R/evaluation/blt_utils.py and bbox_metrics.py) reproduces the golden.  GPU: the device results match the
golden and, on random sets, the restatement; repeated calls are bit-identical.

Bars.  Exact: triplet counts, the novel count and the two truncated TV distances; every perceptual IoU and its mean; F1 row
max, median and arg-max; every validity flag and list length.  ATOL = 1e-12 absolute (float64 sums taken in another order):
full TV distance, novelty, alignment, F1 row means and summaries.  IoU and overlap: the device and the restatement sum the same
float32 pair terms in float64 (RTOL_SUM = 1e-12 relative between them), the reference sums them in float32, NumPy's pairwise
sum: for up to 2016 positive terms at most 15 + 3 + 7 additions inside a 128-block, 4 levels above it and the division, <= 30
roundings of 2^-24 each, hence RTOL_F32 = 32 * 2^-24 per layout and 64 * 2^-24 for the float32 mean over the layouts."""
import os
import re

import numpy as np
import pytest
import torch

from diffusesg_amd import lib
from diffusesg_amd import evaluate as E
from diffusesg_amd.evaluate import SceneGraphEvaluatorHip, SceneGraphEvaluatorHipFull as SGF, evaluate_samples, hip_evaluator
from util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SGSTAT_SYMBOLS = ["dsg_sgstat_triplet_counts", "dsg_sgstat_layout", "dsg_sgstat_f1_rowstats"]
METRICS = ("vanilla_iou", "perceptual_iou", "overlap", "alignment")
ATOL, MMD_ATOL = 1e-12, 1e-10            # MMD_ATOL: the bar of tests/test_eval_metrics.py for the same MMD calls
RTOL_SUM = 1e-12
RTOL_F32, RTOL_F32_MEAN = 32 * 2.0 ** -24, 64 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------------
# NumPy restatement of the reference
# ------------------------------------------------------------------------------------------------------------------------
def _area32(x0, y0, x1, y1):
    return np.maximum(np.float32(0), x1 - x0) * np.maximum(np.float32(0), y1 - y0)


def np_layout(layout, canvas=32):
    """The four blt_utils metrics of one layout [n, 4] float32 -> [iou, perceptual, overlap, alignment], None as in the
    reference; pair terms in float32, sums in float64."""
    b = np.asarray(layout, np.float32).reshape(-1, 4)
    n = len(b)
    out = [None, None, None, None]
    i, j = np.triu_indices(n, 1)
    p, q = b[i], b[j]
    inter = _area32(np.maximum(p[:, 0], q[:, 0]), np.maximum(p[:, 1], q[:, 1]), np.minimum(p[:, 2], q[:, 2]), np.minimum(p[:, 3], q[:, 3]))
    union = _area32(*p.T) + _area32(*q.T) - inter
    assert inter.dtype == np.float32 and union.dtype == np.float32
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = np.where(np.abs(union.astype(np.float64)) <= 1e-8, np.float32(0), inter / union)   # np.isclose(union, 0.)
    if (iou > 0).any():
        out[0] = iou[iou > 0].astype(np.float64).sum() / (iou > 0).sum()
    if (inter > 0).any():
        out[2] = inter[inter > 0].astype(np.float64).sum()
    if n >= 2:
        r = np.round(b * np.float32(canvas)).astype(int)      # half to even
        cover = np.zeros((canvas, canvas), int)
        for x0, y0, x1, y1 in r:
            cover[x0:x1, y0:y1] += 1
        if (cover > 0).sum():
            out[1] = (cover > 1).sum() / (cover > 0).sum()
        two = np.float32(2)
        left = (np.abs(b[:, None, 0] - b[None, :, 0]) + np.abs(b[:, None, 1] - b[None, :, 1])) / two
        right = (np.abs(b[:, None, 2] - b[None, :, 2]) + np.abs(b[:, None, 3] - b[None, :, 3])) / two
        cx, cy = (b[:, 0] + b[:, 2]) / two, (b[:, 1] + b[:, 3]) / two
        centre = (np.abs(cx[:, None] - cx[None]) + np.abs(cy[:, None] - cy[None])) / two
        d = np.minimum(np.minimum(left, centre), right).astype(np.float64) + np.diag(np.full(n, np.inf))
        assert left.dtype == np.float32
        out[3] = d.min(1).sum()
    return out


def np_layout_set(box, flag):
    """(values [4, B] float64, valid [4, B] bool)."""
    rows = [np_layout(b[f != 0]) for b, f in zip(box, flag)]
    valid = np.array([[r[m] is not None for r in rows] for m in range(4)])
    values = np.array([[0.0 if r[m] is None else r[m] for r in rows] for m in range(4)])
    return values, valid


def np_triplet_counts(edge, node, keys):
    """(counts [n_keys] int64 in the keys' order, novel): every non-zero entry of edge [B, N, N] is a triplet."""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    b, i, j = np.nonzero(edge)
    trip = np.stack([node[b, i], node[b, j], edge[b, i, j]], -1).astype(np.int64)
    pack = lambda t: t[:, 0] << 42 | t[:, 1] << 21 | t[:, 2]
    pk, pt = pack(keys), pack(trip)
    order = np.argsort(pk)
    at = np.searchsorted(pk[order], pt)
    hit = (at < len(pk)) & (pk[order][np.minimum(at, len(pk) - 1)] == pt) if len(pk) else np.zeros(len(pt), bool)
    counts = np.bincount(order[at[hit]], minlength=len(pk)).astype(np.int64)
    return counts, int((~hit).sum())


def np_triplet_tv(counts, novel, freq, n_to_count):
    """compute_triplet_tv_dist's reduction (bbox_metrics.py:350-369) with the novel columns summed into one."""
    n = len(counts)
    rej = counts / counts.sum() if counts.sum() > 0 else np.zeros(n)
    all_ = np.concatenate([counts, [novel]]) / (counts.sum() + novel) if counts.sum() + novel > 0 else np.zeros(n)
    diff_rej, diff_all = freq - rej, freq - all_[:n]
    return (np.abs(diff_rej[:n_to_count]).sum(), np.abs(diff_all[:n_to_count]).sum(),
            np.abs(np.concatenate([diff_all, all_[n:]])).sum(), np.abs(all_[n:]).sum())


def np_rowstats(m):
    """max, mean, median, argmax over axis 1 of [X, Y, W]."""
    with np.errstate(invalid="ignore"):
        return {"max": m.max(1), "mean": m.mean(1), "median": np.median(m, 1), "argmax": m.argmax(1)}


def _dict(keys, freq):
    return {tuple(int(v) for v in k): float(f) for k, f in zip(keys, freq)}


def _assert_nan_close(got, want, atol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(np.nan_to_num(got), np.nan_to_num(want), rtol=0, atol=atol)


def _check_layout_against_golden(g, name, values, valid, what):
    """values / valid [4, B] against the reference's lists; returns the largest relative differences of IoU and overlap."""
    worst = {}
    for m, metric in enumerate(METRICS):
        want, wv = g[f"{name}_{metric}"], g[f"{name}_{metric}_valid"]
        n = len(wv)
        assert np.array_equal(valid[m][:n], wv), (what, metric)
        got = values[m][:n][wv]
        assert len(got) == len(want)
        mean, wmean = np.mean(got), float(g[f"{name}_{metric}_mean"])
        if metric == "perceptual_iou":
            assert np.array_equal(got, want) and mean == wmean, (what, metric)
        elif metric == "alignment":
            np.testing.assert_allclose(got, want, rtol=0, atol=ATOL)
            assert abs(mean - wmean) <= ATOL
        else:
            rel = np.abs(got - want) / want
            worst[metric] = (float(rel.max()), abs(mean - wmean) / wmean)
            print(f"{what} {name} {metric}: max rel diff per layout {rel.max():.3e}, of the mean {abs(mean - wmean) / wmean:.3e}")
            assert rel.max() <= RTOL_F32 and abs(mean - wmean) / wmean <= RTOL_F32_MEAN, (what, metric)
    return worst


# ------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------
def test_sgstat_symbols_declared_exported_and_loadable():
    hdr = open(os.path.join(ROOT, "include", "dsg.h")).read()
    declared = set(re.findall(r"\b(dsg_sgstat_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(SGSTAT_SYMBOLS) and set(SGSTAT_SYMBOLS) <= set(lib.EXPORTS)
    L = lib.load()
    for name in SGSTAT_SYMBOLS:
        assert hasattr(L, name)
    assert L.dsg_abi_version() == lib.ABI_VERSION


def test_sgstat_entries_refuse_bad_arguments():
    """DSG_ERR_INVALID before any launch: no GPU needed (the pointers are never dereferenced)."""
    L, p = lib.load(), 4096
    assert L.dsg_sgstat_layout(1, 256, p, p, 32, p, p, None) == -1        # N > 255
    assert L.dsg_sgstat_layout(1, 62, p, p, 65, p, p, None) == -1         # canvas > 64
    assert L.dsg_sgstat_layout(1, 62, p, p, 0, p, p, None) == -1
    assert L.dsg_sgstat_layout(0, 62, p, p, 32, p, p, None) == -1
    assert L.dsg_sgstat_layout(1, 62, None, p, 32, p, p, None) == -1
    assert L.dsg_sgstat_triplet_counts(0, 62, p, p, 1, p, p, p, p, None) == -1
    assert L.dsg_sgstat_triplet_counts(1, 62, p, p, -1, p, p, p, p, None) == -1
    assert L.dsg_sgstat_triplet_counts(1, 62, p, p, 1, None, p, p, p, None) == -1
    assert L.dsg_sgstat_triplet_counts(1, 62, p, p, 0, None, None, None, None, None) == -1   # novel is always needed
    assert L.dsg_sgstat_f1_rowstats(1, 16385, 1, p, p, p, p, p, None) == -1                  # a row longer than LDS
    assert L.dsg_sgstat_f1_rowstats(1, 16, 9, p, p, p, p, p, None) == -1
    assert L.dsg_sgstat_f1_rowstats(0, 16, 1, p, p, p, p, p, None) == -1
    assert L.dsg_sgstat_f1_rowstats(1, 16, 1, p, None, p, p, p, None) == -1


@pytest.mark.parametrize("name", ["vg", "coco"])
def test_numpy_restatement_matches_golden_layouts(name):
    g = load("eval_full.npz")
    box, flag = g[f"{name}_box"], g[f"{name}_flag"]
    assert len(box) == 40 and not flag[-1].any()                       # the last layout is the empty one
    for metric in METRICS:                                             # the fixture does not stand on empty ground
        v = g[f"{name}_{metric}_valid"]
        assert v.sum() > len(v) / 2 and (~v).sum() >= 1 and len(g[f"{name}_{metric}"]) == v.sum()
    values, valid = np_layout_set(box, flag)
    _check_layout_against_golden(g, name, values, valid, "restatement")
    # the special layouts: a single box has no metric; touching boxes align but do not overlap; tiny boxes overlap but their
    # IoU falls to np.isclose; half pixels round to even
    assert not valid[:, 0].any() and valid[:, 2].tolist() == [False, True, False, True]
    assert valid[:, 6].tolist() == [False, False, True, True] and valid[:, 5].tolist() == [False, False, False, True]
    assert values[0, 3] == 1.0 and valid[:, 3].all() and valid[:, 8].all()
    assert np.all(g[f"{name}_box"][7] * 64 == np.round(g[f"{name}_box"][7] * 64))


def test_numpy_restatement_matches_golden_triplets():
    g = load("eval_full.npz")
    keys, freq = g["trip_keys"].astype(np.int64), g["trip_freq"]
    edge, node = g["trip_edge"].astype(np.int64), g["trip_node"].astype(np.int64)
    assert 2000 <= len(keys) <= 3000 and not edge[0].any() and edge[1, 5, 5] != 0
    assert (edge[~g["trip_flag"]] != 0).any()                          # edges on unflagged nodes
    counts, novel = np_triplet_counts(edge, node, keys)
    assert np.array_equal(counts, g["trip_counts"]) and novel == int(g["trip_novel"])
    total = counts.sum() + novel
    assert counts.sum() >= total / 5 and novel >= total / 10 and (counts == 0).any()
    for tag, n in (("all", len(keys)), ("100", 100), ("f32", len(keys))):
        got, want = np_triplet_tv(counts, novel, freq, n), g[f"trip_out_{tag}"]
        assert got[0] == want[0] and got[1] == want[1]
        assert abs(got[2] - want[2]) <= ATOL and abs(got[3] - want[3]) <= ATOL
    z = np_triplet_tv(*np_triplet_counts(np.zeros_like(edge[:4]), node[:4], keys), freq, 100)
    assert z[:2] == tuple(g["trip_out_zero"][:2]) and np.abs(np.array(z[2:]) - g["trip_out_zero"][2:]).max() <= ATOL and z[3] == 0
    c, nv = np_triplet_counts(edge[:6], g["trip_node_novel"].astype(np.int64), keys)
    assert c.sum() == 0 and nv > 0
    v = np_triplet_tv(c, nv, freq, 100)
    assert v[:2] == tuple(g["trip_out_novel"][:2]) and np.abs(np.array(v[2:]) - g["trip_out_novel"][2:]).max() <= ATOL and v[3] == 1.0
    # the host half of the product is the same reduction
    for a, b in zip(E.triplet_tv_from_counts(counts, novel, _dict(keys, freq), range(100)), g["trip_out_100"]):
        assert abs(a - b) <= ATOL


def test_numpy_restatement_matches_golden_f1_summaries():
    g = load("eval_full.npz")
    mats = {"vanilla": g["f1_mat"][..., 0], "area": g["f1_mat"][..., 1], "freq": g["f1_mat"][..., 2], "no_node_type": g["f1_mat_no_node_type"]}
    want = dict(zip(g["f1_summary_keys"].tolist(), g["f1_summary"]))
    assert len(want) == 12 and np.isnan(want["area_f1_avg_max"]) and not np.isnan(want["freq_f1_avg_median"])
    for name, m in mats.items():
        s = np_rowstats(m[..., None])
        for key in ("max", "mean", "median"):
            _assert_nan_close(s[key][:, 0].mean(), want[f"{name}_f1_avg_{key}"], ATOL)


def test_numpy_restatement_matches_golden_evaluation_block():
    """The triplet and layout keys of the evaluate_samples case (its MMD and F1 keys need the device)."""
    g = load("eval_full.npz")
    want = dict(zip(g["es_keys"].tolist(), g["es_values"]))
    assert len(want) == 32
    for tag in ("val", "train"):
        keys, freq = g[f"es_{tag}_keys"].astype(np.int64), g[f"es_{tag}_freq"]
        counts, novel = np_triplet_counts(g["es_adj_gen"].astype(np.int64), g["es_node_gen"].astype(np.int64), keys)
        got = np_triplet_tv(counts, novel, freq, int(g["es_n_to_count"]))
        assert got[0] == want[f"triplet_tv_dist_rej_{tag}"] and got[1] == want[f"triplet_tv_dist_all_{tag}"]
        assert abs(got[2] - want[f"triplet_tv_dist_full_{tag}"]) <= ATOL and abs(got[3] - want[f"triplet_novelty_{tag}"]) <= ATOL
    for tag, side in (("pred", "gen"), ("gt", "gt")):
        box = E.cxcywh_to_xyxy(torch.from_numpy(g[f"es_box_{side}"])).clip(min=0.0, max=1.0).numpy()
        values, valid = np_layout_set(box, g[f"es_flag_{side}"])
        _check_block_layout_keys(want, tag, values, valid)


def _check_block_layout_keys(want, tag, values, valid):
    for m, key in enumerate(("iou_blt", "iou_percp_blt", "overlap_blt", "alignment_blt")):
        got, w = np.mean(values[m][valid[m]]), want[f"{tag}_{key}"]
        if m == 1:
            assert got == w
        elif m == 3:
            assert abs(got - w) <= ATOL
        else:
            assert abs(got - w) / w <= RTOL_F32_MEAN


def test_hip_evaluator_full_overrides_the_two_methods():
    class Ref:   # stands in for the reference's SceneGraphEvaluator
        @staticmethod
        def compute_bbox_ioa(*a, **k):
            return "ioa"

        @staticmethod
        def compute_triplet_tv_dist(*a, **k):
            return "tv"

        @staticmethod
        def plot(*a, **k):
            return "plot"

    ev = hip_evaluator(Ref, full=True)()
    assert isinstance(ev, Ref) and isinstance(ev, SGF) and ev.plot() == "plot"
    for m in ("compute_triplet_tv_dist", "compute_bbox_ioa", "compute_bbox_f1_stats"):
        assert getattr(type(ev), m) is getattr(SGF, m)
    for m in ("compute_bbox_f1", "compute_node_type_mmd", "compute_edge_type_mmd", "compute_node_degree_mmd"):
        assert getattr(type(ev), m) is getattr(SceneGraphEvaluatorHip, m)
    # the default keeps the base's, and the pairwise class itself has none of the new methods
    plain = hip_evaluator(Ref)()
    assert plain.compute_bbox_ioa() == "ioa" and plain.compute_triplet_tv_dist() == "tv" and not isinstance(plain, SGF)
    for m in ("compute_triplet_tv_dist", "compute_bbox_ioa", "compute_bbox_f1_stats"):
        assert not hasattr(SceneGraphEvaluatorHip, m)
    with pytest.raises(AssertionError):   # exactly one flag, as in the reference (checked before the device is touched)
        SGF.compute_bbox_ioa(np.zeros((1, 2, 4), np.float32), np.ones((1, 2), bool), flag_overlap=True, flag_alignment=True)
    with pytest.raises(AssertionError):
        SGF.compute_bbox_ioa(np.zeros((1, 2, 4), np.float32), np.ones((1, 2), bool))


def test_triplet_key_packing():
    sk, pos, usable = E._pack_triplet_keys([(3, 2, 1), (1, 2, 3), (1 << 21, 0, 1), (1, 2, 2), (-1, 0, 0), (0, 0, (1 << 21) - 1)])
    assert usable.tolist() == [0, 1, 3, 5] and np.all(np.diff(sk) > 0)
    assert sk.tolist() == [(1 << 21) - 1, 1 << 42 | 2 << 21 | 2, 1 << 42 | 2 << 21 | 3, 3 << 42 | 2 << 21 | 1]
    assert usable[pos].tolist() == [5, 3, 1, 0]


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------
def _kinds(*arrays):
    """The same inputs as numpy arrays, CPU tensors and CUDA tensors."""
    yield "numpy", arrays
    yield "cpu tensor", tuple(torch.from_numpy(a) for a in arrays)
    yield "cuda tensor", tuple(torch.from_numpy(a).to("cuda:0") for a in arrays)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["vg", "coco"])
def test_device_layouts_match_golden(name):
    g = load("eval_full.npz")
    box, flag = g[f"{name}_box"], g[f"{name}_flag"]
    rv, rvalid = np_layout_set(box, flag)
    for kind, (b, f) in _kinds(box, flag):
        values, valid = E.layout_metrics(b, f, 32)
        assert values.dtype == np.float64 and values.shape == (4, 40)
        _check_layout_against_golden(g, name, values, valid, f"device ({kind})")
        # against the float64 restatement: the same float32 terms, summed in float64 in another order
        assert np.array_equal(valid, rvalid)
        assert np.array_equal(values[1], rv[1])
        np.testing.assert_allclose(values[[0, 2]], rv[[0, 2]], rtol=RTOL_SUM, atol=0)
        np.testing.assert_allclose(values[3], rv[3], rtol=0, atol=ATOL)
        for m, metric in enumerate(METRICS):
            kw = {"flag_" + metric: True}
            n = 39 if metric == "perceptual_iou" else 40
            ls = SGF.compute_bbox_ioa(b[:n], f[:n], canvas_size=32, **kw)
            assert isinstance(ls, list) and np.array_equal(np.array(ls), values[m][:n][valid[m][:n]])
            assert SGF.compute_bbox_ioa(b[:n], f[:n], canvas_size=32, return_mean=True, **kw) == np.mean(ls)
        with pytest.raises(ValueError):    # get_perceptual_iou's layout.min() on the empty layout
            SGF.compute_bbox_ioa(b, f, canvas_size=32, flag_perceptual_iou=True)
    with pytest.raises(AssertionError):    # its assert on the coordinate range
        SGF.compute_bbox_ioa(box[:5] * np.float32(1.5), flag[:5], flag_perceptual_iou=True)
    big = box[:5] * np.float32(1.5)        # the other metrics take any box
    assert len(SGF.compute_bbox_ioa(big, flag[:5], flag_vanilla_iou=True)) == sum(np_layout(b[f])[0] is not None for b, f in zip(big, flag[:5])) >= 1
    # other canvas sizes against the restatement
    for canvas in (1, 7, 64):
        values, valid = E.layout_metrics(box[:39], flag[:39], canvas)
        want = [np_layout(b[f], canvas)[1] for b, f in zip(box[:39], flag[:39])]
        assert valid[1].tolist() == [w is not None for w in want]
        assert values[1][valid[1]].tolist() == [w for w in want if w is not None]
    with pytest.raises(ValueError):
        E.layout_metrics(box, flag, 65)


@pytest.mark.gpu
def test_device_triplets_match_golden():
    g = load("eval_full.npz")
    keys, freq = g["trip_keys"].astype(np.int64), g["trip_freq"]
    d = _dict(keys, freq)
    everything = list(d.keys())
    edge, node, flag = g["trip_edge"].astype(np.int64), g["trip_node"].astype(np.int64), g["trip_flag"]

    def check(got, want):
        assert got[0] == want[0] and got[1] == want[1]
        assert abs(got[2] - want[2]) <= ATOL and abs(got[3] - want[3]) <= ATOL

    for variant in (lambda a: a, lambda a: a.astype(np.float32), lambda a: a.astype(np.int32), lambda a: a.astype(np.uint8)):
        for kind, (e, t, f) in _kinds(variant(edge), variant(node), flag):
            counts, novel = E.triplet_counts(e, t, d.keys())
            assert counts.dtype == np.int64 and np.array_equal(counts, g["trip_counts"]) and novel == int(g["trip_novel"]), kind
            check(SGF.compute_triplet_tv_dist(e, t, f, d, everything), g["trip_out_all"])
            check(SGF.compute_triplet_tv_dist(e, t, f, d, everything[:100]), g["trip_out_100"])
    check(SGF.compute_triplet_tv_dist(np.zeros_like(edge[:4]), node[:4], flag[:4], d, everything[:100]), g["trip_out_zero"])
    nn = g["trip_node_novel"].astype(np.int64)
    check(SGF.compute_triplet_tv_dist(edge[:6], nn, flag[:6], d, everything[:100]), g["trip_out_novel"])
    assert E.triplet_counts(edge[:6], nn, d.keys())[0].sum() == 0
    # an empty dictionary: everything is novel; keys that no triplet can equal stay at 0
    assert E.triplet_counts(edge, node, [])[1] == int((edge != 0).sum())
    odd = [(-1, 0, 1), tuple(keys[0]), (1 << 21, 0, 1), tuple(keys[1])]
    c, nv = E.triplet_counts(edge, node, odd)
    assert c.tolist() == [0, int(g["trip_counts"][0]), 0, int(g["trip_counts"][1])] and c.sum() + nv == int((edge != 0).sum())
    # refused inputs
    bad = edge.astype(np.float32)
    bad[3, 1, 2] = 2.5
    with pytest.raises(ValueError):
        SGF.compute_triplet_tv_dist(bad, node, flag, d, everything)
    bad = node.copy()
    bad[1, 5] = -1                       # node 5 of graph 1 carries the diagonal entry
    with pytest.raises(ValueError):
        SGF.compute_triplet_tv_dist(edge, bad, flag, d, everything)
    bad = edge.copy()
    bad[2, 0, 1] = 1 << 21
    with pytest.raises(ValueError):
        SGF.compute_triplet_tv_dist(bad, node, flag, d, everything)
    unused = node.copy()
    unused[0] = -1                       # graph 0 has no edge: its node types are never looked at
    assert np.array_equal(E.triplet_counts(edge, unused, d.keys())[0], g["trip_counts"])


@pytest.mark.gpu
def test_device_f1_stats_match_golden():
    g = load("eval_full.npz")
    a = [g[f"f1_{k}"] for k in ("box_gen", "cls_gen", "flag_gen", "box_ref", "cls_ref", "flag_ref")]
    a[1], a[4] = a[1].astype(np.int64), a[4].astype(np.int64)
    w = list(g["f1_weights"])
    want = dict(zip(g["f1_summary_keys"].tolist(), g["f1_summary"]))
    for kind, arrs in _kinds(*a):
        st = SGF.compute_bbox_f1_stats(*arrs, w, return_matrix=True)
        ones = [arrs[0], torch.ones_like(torch.as_tensor(arrs[1])), arrs[2], arrs[3], torch.ones_like(torch.as_tensor(arrs[4])), arrs[5]]
        nt = SGF.compute_bbox_f1_stats(*ones, class_weight_ls=None, return_matrix=True)
        for s, mat in ((st, g["f1_mat"]), (nt, g["f1_mat_no_node_type"][..., None])):
            _assert_nan_close(s["matrix"], mat, ATOL)
            own = np_rowstats(s["matrix"])                              # exact against NumPy on the device's own matrix
            for key in ("max", "median", "argmax"):
                assert np.array_equal(s[key], own[key], equal_nan=True), (kind, key)
            _assert_nan_close(s["mean"], own["mean"], ATOL)
            assert s["argmax"].dtype == np.int64 and s["max"].shape == mat.shape[::2]
            ref = np_rowstats(mat)                                      # and within the F1 bar of the reference's matrix
            for key in ("max", "mean", "median"):
                _assert_nan_close(s[key], ref[key], ATOL)
        assert np.isnan(st["max"][3, 1]) and st["argmax"][3, 1] == 3   # the NaN of row 3 sits in column 3
        for name, s, k in (("vanilla", st, 0), ("area", st, 1), ("freq", st, 2), ("no_node_type", nt, 0)):
            for key in ("max", "mean", "median"):
                _assert_nan_close(s[key][:, k].mean(), want[f"{name}_f1_avg_{key}"], ATOL)
        assert "matrix" not in SGF.compute_bbox_f1_stats(*arrs, w)


@pytest.mark.gpu
def test_device_evaluate_samples_matches_golden():
    g = load("eval_full.npz")
    want = dict(zip(g["es_keys"].tolist(), g["es_values"]))
    val_d, train_d = _dict(g["es_val_keys"], g["es_val_freq"]), _dict(g["es_train_keys"], g["es_train_freq"])
    to_count = list(train_d.keys())[:int(g["es_n_to_count"])]
    arrays = [g["es_adj_gen"].astype(np.int64), g["es_node_gen"].astype(np.int64), g["es_box_gen"], g["es_flag_gen"],
              g["es_adj_gt"].astype(np.int64), g["es_node_gt"].astype(np.int64), g["es_box_gt"], g["es_flag_gt"]]
    first = None
    for kind, arrs in _kinds(*arrays):
        got = evaluate_samples(*arrs, int(g["es_num_node_types"]), int(g["es_num_edge_types"]), val_d, train_d, to_count,
                               g["es_area"], g["es_freq"])
        assert list(got.keys()) == list(want.keys()), kind             # the reference's CSV keys, in its order
        for k, w in want.items():
            v = float(got[k])
            if "mmd" in k:
                assert abs(v - w) <= MMD_ATOL, (kind, k, v, w)
            elif "tv_dist_rej" in k or "tv_dist_all" in k or "iou_percp" in k:
                assert v == w, (kind, k, v, w)
            elif k.endswith("iou_blt") or k.endswith("overlap_blt"):
                assert abs(v - w) / w <= RTOL_F32_MEAN, (kind, k, v, w)
            else:                                                      # full TV, novelty, alignment, F1 summaries
                assert abs(v - w) <= ATOL, (kind, k, v, w)
        first = first or got
        assert got == first                                            # the input kind changes no bit


def _random_layouts(rng, B, N):
    b = np.concatenate([rng.uniform(0.0, 1.0, (B, N, 2)), rng.uniform(0.0, 0.5, (B, N, 2))], -1).astype(np.float32)
    box = E.cxcywh_to_xyxy(torch.from_numpy(b)).clip(min=0.0, max=1.0).numpy()
    box[rng.uniform(size=(B, N)) < 0.05, 2] = 0.0                      # some empty boxes
    flag = rng.uniform(size=(B, N)) < rng.uniform(0.0, 1.0, (B, 1))    # any subset of the nodes, some layouts empty
    flag[:4] = True
    return box, flag


@pytest.mark.gpu
def test_device_layouts_random_2048_match_restatement_and_repeat_bit_identical():
    rng = np.random.default_rng(5)
    B, N = 2048, 62
    box, flag = _random_layouts(rng, B, N)
    values, valid = E.layout_metrics(torch.from_numpy(box).to("cuda:0"), torch.from_numpy(flag).to("cuda:0"), 32)
    rv, rvalid = np_layout_set(box, flag)
    assert np.array_equal(valid, rvalid) and valid.mean() > 0.5 and not valid.all(1).any()
    assert np.array_equal(values[1], rv[1])
    np.testing.assert_allclose(values[[0, 2]], rv[[0, 2]], rtol=RTOL_SUM, atol=0)
    np.testing.assert_allclose(values[3], rv[3], rtol=0, atol=ATOL)
    again = E.layout_metrics(box, flag, 32)
    assert np.array_equal(values, again[0]) and np.array_equal(valid, again[1])
    # the node bound of the kernel: 255 boxes in one layout
    box, flag = _random_layouts(rng, 3, 255)
    values, valid = E.layout_metrics(box, flag, 32)
    rv, rvalid = np_layout_set(box, flag)
    assert np.array_equal(valid, rvalid) and np.array_equal(values[1], rv[1])
    np.testing.assert_allclose(values[[0, 2]], rv[[0, 2]], rtol=RTOL_SUM, atol=0)
    np.testing.assert_allclose(values[3], rv[3], rtol=0, atol=ATOL)
    with pytest.raises(ValueError):
        E.layout_metrics(np.zeros((1, 256, 4), np.float32), np.ones((1, 256), bool), 32)


@pytest.mark.gpu
def test_device_triplets_random_2048_match_restatement_and_repeat_bit_identical():
    rng = np.random.default_rng(6)
    B, N, n_types, n_pred, n_keys = 2048, 62, 40, 50, 20000
    ids = rng.choice(n_types * n_types * n_pred, n_keys, replace=False)
    keys = np.stack([ids // (n_types * n_pred), ids // n_pred % n_types, ids % n_pred + 1], -1)
    freq = rng.integers(1, 500, n_keys).astype(np.float64)
    d = _dict(keys, freq / freq.sum())
    edge = np.where(rng.uniform(size=(B, N, N)) < 0.03, rng.integers(1, n_pred + 1, (B, N, N)), 0).astype(np.int32)
    node = rng.integers(0, n_types, (B, N)).astype(np.int32)
    e, t = torch.from_numpy(edge).to("cuda:0"), torch.from_numpy(node).to("cuda:0")
    counts, novel = E.triplet_counts(e, t, d.keys())
    rc, rn = np_triplet_counts(edge, node, keys)
    assert np.array_equal(counts, rc) and novel == rn and rc.sum() > 0.2 * (rc.sum() + rn) and rn > 0.1 * (rc.sum() + rn)
    got = SGF.compute_triplet_tv_dist(e, t, None, d, range(1000))
    want = np_triplet_tv(rc, rn, np.array(list(d.values())), 1000)
    assert got[0] == want[0] and got[1] == want[1] and abs(got[2] - want[2]) <= ATOL and abs(got[3] - want[3]) <= ATOL
    assert got == SGF.compute_triplet_tv_dist(e, t, None, d, range(1000))
    again = E.triplet_counts(e, t, d.keys())
    assert np.array_equal(counts, again[0]) and novel == again[1]


def _rowstats_entry(m):
    """dsg_sgstat_f1_rowstats on a host block [rows, Y, W]."""
    dev = torch.device("cuda:0")
    blk = torch.from_numpy(m).to(dev)
    rows, _, W = m.shape
    mx, mean, med = (torch.full((rows, W), -7.0, dtype=torch.float64, device=dev) for _ in range(3))
    arg = torch.full((rows, W), -7, dtype=torch.int32, device=dev)
    E._f1_row_stats(blk, mx, mean, med, arg)
    torch.cuda.synchronize()
    return {"max": mx.cpu().numpy(), "mean": mean.cpu().numpy(), "median": med.cpu().numpy(), "argmax": arg.cpu().numpy()}


@pytest.mark.gpu
@pytest.mark.parametrize("Y", [1, 2, 3, 230, 255, 256, 257, 4096, 8193, 16384])
def test_device_rowstats_exact(Y, monkeypatch):
    """Odd and even lengths, ties, negative values, NaNs; Y = 8193 and 16384 need more than 64 KiB of LDS."""
    rng = np.random.default_rng(Y)
    rows, W = 5, 3
    m = rng.uniform(0.0, 1.0, (rows, Y, W))
    m[1] = np.round(m[1] * 4) / 4                      # many ties, the maximum repeated
    m[2] = rng.normal(0.0, 1.0, (Y, W))                # negative values
    m[3] = 0.0                                         # the F1 matrix's usual row: all zero
    m[3, Y // 2:, 0] = rng.uniform(0, 1, Y - Y // 2)   # ... and half zero
    m[4, rng.integers(0, Y, 2), 1] = np.nan            # NaNs in one column of one row
    got, want = _rowstats_entry(m), np_rowstats(m)
    for key in ("max", "median", "argmax"):
        assert np.array_equal(got[key], want[key], equal_nan=True), key
    _assert_nan_close(got["mean"], want["mean"], ATOL)
    assert np.isnan(got["max"][4, 1]) and got["argmax"][4, 1] == np.flatnonzero(np.isnan(m[4, :, 1]))[0]
    again = _rowstats_entry(m)
    assert all(np.array_equal(got[k], again[k], equal_nan=True) for k in got)
    if Y == 230:                                       # a row too long for the kernel goes through NumPy
        monkeypatch.setattr(E, "_ROWSTATS_MAX_Y", 100)
        host = _rowstats_entry(m)
        assert all(np.array_equal(host[k], want[k], equal_nan=True) for k in host)


def _random_scenes(rng, S, N, n_cls, palette):
    b = np.concatenate([rng.uniform(0.0, 1.0, (S, N, 2)), rng.uniform(0.02, 0.5, (S, N, 2))], -1).astype(np.float32)
    box = E.cxcywh_to_xyxy(torch.from_numpy(b)).clamp(0.0, 1.0).numpy()
    cls = rng.choice(palette, (S, N)).astype(np.int64)
    flag = (np.arange(N)[None] < rng.integers(0, N + 1, S)[:, None]).astype(np.uint8)
    return box, cls, flag


@pytest.mark.gpu
def test_device_f1_stats_equal_numpy_on_the_matrix_in_blocks(monkeypatch):
    rng = np.random.default_rng(11)
    N, n_cls, X, Y = 33, 171, 301, 230
    palette = rng.choice(n_cls, 10, replace=False)
    bg, cg, fg = _random_scenes(rng, X, N, n_cls, palette)
    br, cr, fr = _random_scenes(rng, Y, N, n_cls, palette)
    w = [np.ones(n_cls), rng.uniform(0, 1, n_cls)]
    want = np_rowstats(SGF.compute_bbox_f1(bg, cg, fg, br, cr, fr, w))
    assert (want["max"] > 0).mean() > 0.5
    whole = SGF.compute_bbox_f1_stats(bg, cg, fg, br, cr, fr, w)
    monkeypatch.setattr(E, "_F1_BLOCK_BYTES", 37 * Y * 2 * 8)          # streamed in blocks of 37 rows
    tiled = SGF.compute_bbox_f1_stats(bg, cg, fg, br, cr, fr, w, return_matrix=True)
    for s in (whole, tiled):
        for key in ("max", "median", "argmax"):
            assert s[key].shape == (X, 2) and np.array_equal(s[key], want[key]), key
        np.testing.assert_allclose(s["mean"], want["mean"], rtol=0, atol=ATOL)
    assert all(np.array_equal(whole[k], tiled[k]) for k in whole)      # the block size changes no bit
    assert np.array_equal(tiled["matrix"], SGF.compute_bbox_f1(bg, cg, fg, br, cr, fr, w))
