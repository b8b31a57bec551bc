"""Conditional sampling on top of `NodeAdjEDMSamplerHip.sample_known` (`dsg_sample_known`): scene-graph completion and layout
generation from a graph.  The reference has neither; its loop has the mechanism in degenerate form -- `sanity_check_gt_*`
(R/runner/mcmc_sampler/edm.py:372-377) replaces the denoiser's output everywhere -- and completion is that replacement applied to the
entries an element mask selects.

  completion_masks       which elements of the state are known, from a per-node "this node is given" table
  complete_scene_graphs  integer graphs in -> encode -> sample_known -> decode -> completed integer graphs out
  layout_from_graph      all labels and relations known, the boxes generated
  vary_scene_graphs      a variation of a given graph: start part-way down the noise levels from a noised copy of it
  start_step_for_sigma   the schedule index at which the noise level has come down to a given sigma

`resample=(jump_len, n_resample)` / `resample_range=(lo, hi)` run the loop along a resampling walk (RePaint-style: each block of
jump_len noise levels is run n_resample times, the state diffused back up in between -- `sample_known`'s keywords).
"""
from __future__ import annotations

import torch

from . import io as _io

EDGE_MODES = ("among_known", "none", "all")


def completion_masks(cfg, node_flags, known_nodes, *, labels=True, boxes=True, edges="among_known"):
    """Element masks of a completion -> (mask_adj uint8 [B,C_adj,N,N], mask_node uint8 [B,N,C_node]), nonzero = known.
    known_nodes: bool [B,N], the given nodes (padded nodes never count).  labels / boxes: whether a given node's label channels (the
    first C_node - 4) / box channels (the last four) are known.  edges: 'among_known' -- entry (i, j) is known iff both nodes are;
    'none'; 'all' -- every entry between valid nodes.  Pure torch on the tensors' own device (CPU tensors work)."""
    if edges not in EDGE_MODES:
        raise ValueError(f"edges should be one of {EDGE_MODES}")
    n = cfg.max_node_num
    if cfg.c_node <= 4:
        raise ValueError(f"C_node = {cfg.c_node}: the node rows must hold label channels and four box channels")
    flags = node_flags.bool()
    known = known_nodes.bool()
    if flags.shape != known.shape or flags.dim() != 2 or flags.shape[1] != n:
        raise ValueError(f"node_flags {tuple(node_flags.shape)} and known_nodes {tuple(known_nodes.shape)} must both be [B, {n}]")
    known = known & flags
    B = flags.shape[0]
    if edges == "among_known":
        pair = known[:, :, None] & known[:, None, :]
    elif edges == "all":
        pair = flags[:, :, None] & flags[:, None, :]
    else:
        pair = torch.zeros((B, n, n), dtype=torch.bool, device=flags.device)
    mask_adj = pair[:, None].expand(B, cfg.c_adj, n, n).to(torch.uint8).contiguous()
    mask_node = torch.zeros((B, n, cfg.c_node), dtype=torch.uint8, device=flags.device)
    if labels:
        mask_node[:, :, :cfg.c_node - 4] = known[:, :, None].to(torch.uint8)
    if boxes:
        mask_node[:, :, cfg.c_node - 4:] = known[:, :, None].to(torch.uint8)
    return mask_adj, mask_node


def complete_scene_graphs(net, sampler, q_adj, q_node, bbox, node_flags, known_nodes, n_adj_type, n_node_type, *,
                          encoding="bits", labels=True, boxes=True, edges="among_known", seed=None, resample=None, resample_range=None,
                          graph_seeds=None, coin_seed=None, guide=None, guide_scale=1.0):
    """Scene-graph completion: the labels / boxes of the nodes `known_nodes` marks and the relations `edges` selects are held at the
    values in q_adj [B,N,N], q_node [B,N] (integer types) and bbox [B,N,4] (in [0,1]); everything else is generated.  Values at
    unknown entries are ignored.  Returns the decoded batch (q_adj int32 [B,N,N], q_node int32 [B,N], bbox float32 [B,N,4]) on the
    device.  `net`: the NodeAdjPrecondHip network with bbox channels, `sampler`: a NodeAdjEDMSamplerHip; `encoding` is the
    network's edge and node encoding; `resample` / `resample_range`: the resampling walk (default: none); `graph_seeds` / `coin_seed`:
    per-graph noise streams, as `NodeAdjEDMSamplerHip.sample` takes them; `guide` (a `guide.BoxGuide`) / `guide_scale`:
    in-loop box guidance of the generated boxes (`sample_guided`; known boxes stay exactly as given)."""
    cfg = getattr(net, "module", net).model.config
    known_adj, known_node = _io.encode(net, q_adj, q_node, bbox, node_flags, n_adj_type, n_node_type, encoding, encoding)
    mask_adj, mask_node = completion_masks(cfg, node_flags.to(known_adj.device), known_nodes.to(known_adj.device),
                                           labels=labels, boxes=boxes, edges=edges)
    if guide is not None:
        adj, node = sampler.sample_guided(net, node_flags, guide, guide_scale,
                                          known=(known_adj, known_node, mask_adj, mask_node), seed=seed, return_device=True,
                                          flag_adj_multi_channel=True, **_walk_kw(resample, resample_range), **_seed_kw(graph_seeds, coin_seed))
        return _io.decode(net, adj, node, node_flags, n_adj_type, n_node_type, encoding, encoding, bbox=True)
    adj, node = sampler.sample_known(net, node_flags, known_adj, known_node, mask_adj, mask_node, seed=seed, return_device=True,
                                     flag_node_multi_channel=True, flag_adj_multi_channel=True,
                                     num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj, **_walk_kw(resample, resample_range),
                                     **_seed_kw(graph_seeds, coin_seed))
    return _io.decode(net, adj, node, node_flags, n_adj_type, n_node_type, encoding, encoding, bbox=True)


def _walk_kw(resample, resample_range, **more):
    """the walk keywords of sample_known that are not at their defaults (a call without any stays on the plain path)"""
    kw = dict(more)
    if resample is not None:
        kw["resample"] = resample
    if resample_range is not None:
        kw["resample_range"] = resample_range
    return kw


def _seed_kw(graph_seeds, coin_seed):
    """the per-graph seed keywords of sample_known that are given (a call without any is the one it was before they existed)"""
    kw = {}
    if graph_seeds is not None:
        kw["graph_seeds"] = graph_seeds
    if coin_seed is not None:
        kw["coin_seed"] = coin_seed
    return kw


def layout_from_graph(net, sampler, q_adj, q_node, node_flags, n_adj_type, n_node_type, *, encoding="bits", seed=None, resample=None,
                      resample_range=None, graph_seeds=None, coin_seed=None, guide=None, guide_scale=1.0):
    """Layout generation from a graph: every label and every relation is known, the bounding boxes are generated.  Returns the
    decoded batch like `complete_scene_graphs`; its q_adj / q_node equal the inputs at valid nodes (off the diagonal).  `guide` /
    `guide_scale`: in-loop box guidance of the layout, as in `complete_scene_graphs`."""
    B, n = node_flags.shape[0], q_node.shape[-1]
    free_boxes = torch.full((B, n, 4), 0.5, dtype=torch.float32)   # placeholder: the box channels are unknown
    return complete_scene_graphs(net, sampler, q_adj, q_node, free_boxes, node_flags, node_flags.bool(), n_adj_type, n_node_type,
                                 encoding=encoding, labels=True, boxes=False, edges="all", seed=seed, resample=resample,
                                 resample_range=resample_range, graph_seeds=graph_seeds, coin_seed=coin_seed, guide=guide,
                                 guide_scale=guide_scale)


def start_step_for_sigma(sampler, sigma):
    """The smallest schedule index i with sampler.sigma_steps[i] <= sigma: where a partial-noise start at noise level `sigma` begins
    (the levels fall with the index).  ValueError when sigma lies below the last level."""
    below = (sampler.sigma_steps <= float(sigma)).nonzero()
    if below.numel() == 0:
        raise ValueError(f"sigma = {sigma} is below the schedule's last level {float(sampler.sigma_steps[-1])}")
    return int(below[0])


def vary_scene_graphs(net, sampler, q_adj, q_node, bbox, node_flags, n_adj_type, n_node_type, *, start_step, known_nodes=None,
                      encoding="bits", labels=True, boxes=True, edges="among_known", resample=None, seed=None,
                      graph_seeds=None, coin_seed=None):
    """A variation of given scene graphs (SDEdit-style): the encoded graph is noised to the level of schedule index `start_step`
    (`start_step_for_sigma`) and denoised from there, so the result keeps as much of the input's structure as that noise level leaves.
    q_adj [B,N,N], q_node [B,N], bbox [B,N,4] as `complete_scene_graphs`; returns the decoded batch like it.  Nothing is held when
    `known_nodes` is None; otherwise the entries `completion_masks` selects stay at the input's values (the base is the input itself,
    so base and known values agree).  `resample`: resampling walk over the executed part of the schedule."""
    cfg = getattr(net, "module", net).model.config
    base_adj, base_node = _io.encode(net, q_adj, q_node, bbox, node_flags, n_adj_type, n_node_type, encoding, encoding)
    held = node_flags.bool() & False if known_nodes is None else known_nodes
    mask_adj, mask_node = completion_masks(cfg, node_flags.to(base_adj.device), held.to(base_adj.device),
                                           labels=labels, boxes=boxes, edges=edges if known_nodes is not None else "none")
    adj, node = sampler.sample_known(net, node_flags, base_adj, base_node, mask_adj, mask_node, seed=seed, return_device=True,
                                     flag_node_multi_channel=True, flag_adj_multi_channel=True,
                                     num_node_chan=cfg.c_node, num_edge_chan=cfg.c_adj,
                                     **_walk_kw(resample, None, start_step=int(start_step), base_adjs=base_adj, base_nodes=base_node),
                                     **_seed_kw(graph_seeds, coin_seed))
    return _io.decode(net, adj, node, node_flags, n_adj_type, n_node_type, encoding, encoding, bbox=True)
