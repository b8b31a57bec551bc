"""No GPU: the host side of conditional sampling -- the element masks of a completion, the encode fixture, the export list."""
import numpy as np
import pytest
import torch

from diffusesg_amd import lib
from diffusesg_amd import spec as S
from diffusesg_amd.complete import completion_masks
from util import load


def _cfg():
    # N = 4, two adjacency channels, two label channels + four box channels
    return S.ModelConfig(max_node_num=4, c_adj=2, c_node=6, depths=(1,), num_heads=(3,), window_size=4, self_condition=True)


# sample 0: three valid nodes, nodes 0 and 2 given; sample 1: two valid nodes, node 1 given -- and node 3, which is padded
FLAGS = torch.tensor([[1, 1, 1, 0], [1, 1, 0, 0]], dtype=torch.bool)
KNOWN = torch.tensor([[1, 0, 1, 0], [0, 1, 0, 1]], dtype=torch.bool)
AMONG = [[[1, 0, 1, 0], [0, 0, 0, 0], [1, 0, 1, 0], [0, 0, 0, 0]],
         [[0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]]
ALL = [[[1, 1, 1, 0], [1, 1, 1, 0], [1, 1, 1, 0], [0, 0, 0, 0]],
       [[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]]
NODE_ROWS = [[1, 0, 1, 0], [0, 1, 0, 0]]   # KNOWN restricted to valid nodes


def _node_mask(labels, boxes):
    rows = torch.tensor(NODE_ROWS, dtype=torch.uint8)[:, :, None]
    chan = torch.tensor([labels, labels, boxes, boxes, boxes, boxes], dtype=torch.uint8)[None, None, :]
    return rows * chan


@pytest.mark.parametrize("edges,pairs", [("among_known", AMONG), ("all", ALL), ("none", np.zeros((2, 4, 4), int).tolist())])
def test_completion_masks_edge_modes(edges, pairs):
    ma, mn = completion_masks(_cfg(), FLAGS, KNOWN, edges=edges)
    assert ma.dtype == torch.uint8 and mn.dtype == torch.uint8 and not ma.is_cuda
    assert ma.shape == (2, 2, 4, 4) and mn.shape == (2, 4, 6)
    want = torch.tensor(pairs, dtype=torch.uint8)[:, None].expand(2, 2, 4, 4)
    assert torch.equal(ma, want)
    assert torch.equal(mn, _node_mask(1, 1))


@pytest.mark.parametrize("labels,boxes", [(True, True), (True, False), (False, True), (False, False)])
def test_completion_masks_label_and_box_switches(labels, boxes):
    ma, mn = completion_masks(_cfg(), FLAGS, KNOWN, labels=labels, boxes=boxes)
    assert torch.equal(mn, _node_mask(int(labels), int(boxes)))
    assert torch.equal(ma[:, 0], torch.tensor(AMONG, dtype=torch.uint8))   # the switches do not touch the edges


def test_completion_masks_reject_bad_arguments():
    with pytest.raises(ValueError):
        completion_masks(_cfg(), FLAGS, KNOWN, edges="some")
    with pytest.raises(ValueError):
        completion_masks(_cfg(), FLAGS, KNOWN[:, :3])
    no_boxes = S.ModelConfig(max_node_num=4, c_adj=2, c_node=4, depths=(1,), num_heads=(3,), window_size=4, self_condition=True)
    with pytest.raises(ValueError, match="box channels"):
        completion_masks(no_boxes, FLAGS, KNOWN)


def test_encode_fixture_keys_and_shapes():
    g = load("complete_encode.npz")
    B, N = 3, 8
    assert g["flags"].shape == (B, N) and g["flags"].dtype == bool
    assert g["flags"].sum(1).tolist() == [8, 5, 1]
    chans = {"bits": lambda k: int(np.ceil(np.log2(k))), "one_hot": lambda k: k, "ddpm": lambda k: None}
    for enc in ("bits", "one_hot", "ddpm"):
        n_adj_type, n_node_type = (int(v) for v in g[f"{enc}_types"])
        ca, cn = chans[enc](n_adj_type), chans[enc](n_node_type)
        assert g[f"{enc}_q_adj"].shape == (B, N, N) and g[f"{enc}_q_adj"].dtype == np.int32
        assert g[f"{enc}_q_node"].shape == (B, N) and g[f"{enc}_q_node"].dtype == np.int32
        assert g[f"{enc}_adj"].shape == ((B, N, N) if ca is None else (B, ca, N, N)) and g[f"{enc}_adj"].dtype == np.float32
        assert g[f"{enc}_node"].shape == ((B, N) if cn is None else (B, N, cn)) and g[f"{enc}_node"].dtype == np.float32
        assert g[f"{enc}_q_adj"].max() == n_adj_type - 1 and g[f"{enc}_q_node"].max() == n_node_type - 1
    assert tuple(g["bits_types"]) == (51, 150)


def test_new_entries_are_exported():
    assert "dsg_sample_known" in lib.EXPORTS and "dsg_encode" in lib.EXPORTS
