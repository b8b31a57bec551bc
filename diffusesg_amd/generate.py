"""Generate S graphs reproducibly: per-graph seeds, any batch size, any number of GPUs.

Graph k of a request has the seed `dist.graph_seed(base_seed, first_index + k)` and draws its noise from its own stream
(`NodeAdjEDMSamplerHip.sample(graph_seeds=...)`, `dsg_sample_seeded`); with the handle's option "batch_invariant" on, which `generate`
sets for its duration, the kernels that compute it do not depend on the batch either.  So graph k comes out bit for bit the same
whether it is generated alone, in a batch of 64, first or last, on one GPU or on eight (DESIGN.md §10 states what the guarantee covers).

Ranks take contiguous index ranges, all S graphs are generated, and the results are collected with the one all-gather of
`dist.gather_results`.  `plan` is the batching plan as a pure function.
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch
import torch.distributed as tdist

from . import dist as _dist


def plan(S: int, batch_size: int, rank: int = 0, world: int = 1) -> Dict:
    """How `generate` splits S graphs over `world` ranks and batches of at most `batch_size`.

    Every rank gets a contiguous range [lo, hi) of ceil(S / world) indices (the last ranks fewer, possibly none) and runs the same
    number `n_batches` of batches of the same size `batch` = min(batch_size, ceil(S / world)): one workspace, one set of captured step
    bodies, and equal shards for the single all-gather.  `batches` lists, per batch, (start, count): the request index of its first
    graph and how many real graphs it holds; the remaining batch - count rows, always at the END of a batch and only behind the
    rank's last real graph, are pads (empty graphs).  `shard_len` = n_batches * batch rows per rank go into the gather, of which the
    first hi - lo are real."""
    if S < 1 or batch_size < 1 or world < 1 or not 0 <= rank < world:
        raise ValueError(f"plan: need S >= 1, batch_size >= 1, 0 <= rank < world (S = {S}, batch_size = {batch_size}, rank = {rank}, world = {world})")
    per = -(-S // world)
    lo = min(rank * per, S)
    hi = min(lo + per, S)
    batch = min(int(batch_size), per)
    n_batches = -(-per // batch)
    batches = []
    for k in range(n_batches):
        start = min(lo + k * batch, hi)
        batches.append((start, min(batch, hi - start)))
    return {"lo": lo, "hi": hi, "batch": batch, "n_batches": n_batches, "shard_len": n_batches * batch, "batches": batches}


def _rank_world():
    if tdist.is_available() and tdist.is_initialized():
        return tdist.get_rank(), tdist.get_world_size()
    return 0, 1


@torch.no_grad()
def generate(net, sampler, node_flags, *, batch_size, base_seed, coin_seed=None, first_index=0, known=None, return_device=False):
    """Generate one graph per row of node_flags [S, N]; returns (adj, node) in request order, on every rank, in the layouts
    `sampler.sample` returns (single channels squeezed), on the host unless `return_device`.

    net, sampler: the NodeAdjPrecondHip network and a NodeAdjEDMSamplerHip.  Graph k has the seed
    `dist.graph_seed(base_seed, first_index + k)`: `generate(node_flags[5:8], first_index=5)` regenerates graphs 5..7 of the full run.
    coin_seed: the run's self-conditioning coin sequence (default: sampler.seed), the same for every batch.  known: the four tensors
    of `sample_known` (known_adjs, known_nodes, known_adj_mask, known_node_mask) with leading dimension S, sliced per batch.
    World size and rank come from torch.distributed when it is initialised (`plan`); a ragged last batch is padded with empty graphs,
    and batches that hold no real graph at all are not launched."""
    model = getattr(net, "module", net)
    cfg = model.model.config
    n, ca, cn = cfg.max_node_num, cfg.c_adj, cfg.c_node
    S = node_flags.shape[0]
    rank, world = _rank_world()
    pl = plan(S, batch_size, rank, world)
    b, D = pl["batch"], ca * n * n + n * cn
    handle = model.model._ensure_handle()
    previous = handle.get_option("batch_invariant")
    handle.set_option("batch_invariant", 1)
    shard = None
    try:
        for k, (start, count) in enumerate(pl["batches"]):
            if count == 0:
                continue
            flags = torch.zeros((b,) + tuple(node_flags.shape[1:]), dtype=node_flags.dtype, device=node_flags.device)
            flags[:count] = node_flags[start:start + count]
            seeds = np.zeros(b, dtype=np.uint64)   # a pad is an empty graph: it draws nothing, whatever its seed
            seeds[:count] = _dist.graph_seeds(base_seed, first_index + start, count)
            kw = dict(graph_seeds=seeds, coin_seed=coin_seed, return_device=True, num_node_chan=cn, num_edge_chan=ca)
            if known is None:
                adj, node = sampler.sample(net, flags, **kw)
            else:
                kn = []
                for t in known:
                    pad = torch.zeros((b,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
                    pad[:count] = t[start:start + count]
                    kn.append(pad)
                adj, node = sampler.sample_known(net, flags, *kn, **kw)
            packed = _dist.pack_results(adj, node)
            if shard is None:
                shard = torch.zeros((pl["shard_len"], D), dtype=packed.dtype, device=packed.device)
            shard[k * b:k * b + count] = packed[:count]
    finally:
        handle.set_option("batch_invariant", previous)
    if shard is None:   # a rank without any graph still takes part in the gather
        shard = torch.zeros((pl["shard_len"], D), dtype=torch.float32, device=model.model._dev if world > 1 else "cpu")
    everything = _dist.gather_results(shard)
    rows = []
    for r in range(world):   # drop every rank's pads: its real rows lead its shard
        pr = plan(S, batch_size, r, world)
        rows.append(everything[r * pl["shard_len"]:r * pl["shard_len"] + pr["hi"] - pr["lo"]])
    adj, node = _dist.unpack_results(torch.cat(rows), ca, n, cn)
    if ca == 1:
        adj = adj[:, 0]
    if cn == 1:
        node = node[..., 0]
    return (adj, node) if return_device else (adj.cpu(), node.cpu())
