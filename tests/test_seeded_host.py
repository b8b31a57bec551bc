"""CPU: the host side of reproducible generation -- seed derivation (dist.graph_seed / graph_seeds), the batching plan
(generate.plan), the seed checks of the sampler, and generate() over two gloo ranks with a stand-in sampler on CPU tensors."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from diffusesg_amd import dist as ddist
from diffusesg_amd import generate as gen
from diffusesg_amd import spec


def test_graph_seeds_vectorised_matches_scalar():
    for base, start in [(0, 0), (1234, 7), (2 ** 64 - 1, 2 ** 64 - 3), (2 ** 63, 2 ** 32 - 2)]:
        v = ddist.graph_seeds(base, start, 6)
        assert v.dtype == np.uint64 and v.shape == (6,)
        assert [int(x) for x in v] == [ddist.graph_seed(base, start + i) for i in range(6)]
    # SplitMix64's published first output for state 0, and the definition splitmix64(splitmix64(base) + k)
    assert ddist._splitmix64(0) == 0xE220A8397B1DCDAF
    assert ddist.graph_seed(5, 3) == ddist._splitmix64((ddist._splitmix64(5) + 3) % 2 ** 64)
    assert ddist.graph_seeds(5, 0, 0).shape == (0,)


def test_graph_seeds_do_not_collide():
    a = ddist.graph_seeds(1234, 0, 10 ** 6)
    assert np.unique(a).size == a.size, "10^6 consecutive indices share a seed"
    b = ddist.graph_seeds(1235, 0, 10 ** 5)
    assert np.intersect1d(a[:10 ** 5], b).size == 0, "bases one apart share a seed in their first 10^5"
    assert np.intersect1d(a, b).size == 0


@pytest.mark.parametrize("S,batch,world", [(11, 4, 1), (11, 4, 2), (7, 8, 3), (1, 4, 2)])
def test_plan(S, batch, world):
    plans = [gen.plan(S, batch, r, world) for r in range(world)]
    covered = []
    for p in plans:
        assert 0 <= p["lo"] <= p["hi"] <= S
        covered += list(range(p["lo"], p["hi"]))
    assert covered == list(range(S)), "the ranks' ranges must be disjoint, ordered and cover [0, S)"
    assert len({(p["n_batches"], p["batch"], p["shard_len"]) for p in plans}) == 1, "every rank runs the same number of equal batches"
    for p in plans:
        assert p["batch"] <= batch and len(p["batches"]) == p["n_batches"] and p["shard_len"] == p["n_batches"] * p["batch"]
        real = []
        for k, (start, count) in enumerate(p["batches"]):
            assert 0 <= count <= p["batch"]
            real += list(range(start, start + count))
            if count < p["batch"]:   # a pad: only behind the rank's last real graph
                assert start + count == p["hi"]
                assert all(c == 0 for _, c in p["batches"][k + 1:])
        assert real == list(range(p["lo"], p["hi"]))
    with pytest.raises(ValueError):
        gen.plan(0, 4)
    with pytest.raises(ValueError):
        gen.plan(4, 4, 2, 2)


def test_check_graph_seeds():
    from diffusesg_amd.sampler import check_graph_seeds
    want = [0, 1, 2 ** 32 + 5, 2 ** 64 - 1]
    for given in (want, np.array(want, dtype=np.uint64), np.array(want, dtype=object), tuple(want)):
        got = check_graph_seeds(given, 4)
        assert got.dtype == np.uint64 and got.flags["C_CONTIGUOUS"] and [int(x) for x in got] == want
    assert [int(x) for x in check_graph_seeds(torch.tensor([3, 2 ** 62]), 2)] == [3, 2 ** 62]
    for bad in ([1, 2, 3], [1, 2, 3, 4, 5], [0, 1, 2, -1], [0, 1, 2, 2 ** 64], np.array([0, 1, 2, -1]), torch.tensor([0, 1, 2, -1]),
                np.zeros((2, 2), dtype=np.uint64)):
        with pytest.raises(ValueError):
            check_graph_seeds(bad, 4)
    for bad in ([0.0, 1.0, 2.0, 3.0], np.zeros(4, dtype=np.float32), torch.zeros(4), [True, False, True, True]):
        with pytest.raises(TypeError):
            check_graph_seeds(bad, 4)


# ---- generate() with a stand-in sampler: output a deterministic function of each graph's seed and flags -----------------------------
class _Handle:
    def __init__(self):
        self.value, self.log = 0, []

    def get_option(self, name):
        assert name == "batch_invariant"
        return self.value

    def set_option(self, name, value):
        assert name == "batch_invariant"
        self.value = value
        self.log.append(value)


class _Inner:
    def __init__(self):
        self.config, self._dev, self.handle = spec.tiny_config(), torch.device("cpu"), _Handle()

    def _ensure_handle(self):
        return self.handle


class _Net:
    def __init__(self):
        self.model = _Inner()


class _Sampler:
    """what NodeAdjEDMSamplerHip.sample(graph_seeds=...) promises: row b depends on seed b, flags b and the coin seed only"""
    seed = 1234

    def __init__(self):
        self.batches = []

    def _one(self, cfg, flags, seed, coin_seed, shift=0.0):
        g = torch.Generator().manual_seed((int(seed) ^ (self.seed if coin_seed is None else int(coin_seed))) % 2 ** 63)
        n = cfg.max_node_num
        f = flags.bool()
        a = (torch.randn(cfg.c_adj, n, n, generator=g) + shift) * (f[:, None] & f[None, :])
        x = (torch.randn(n, cfg.c_node, generator=g) + shift) * f[:, None]
        return a, x

    def sample(self, net, flags, *, graph_seeds, coin_seed, return_device, num_node_chan, num_edge_chan):
        cfg = net.model.config
        assert net.model.handle.value == 1, "generate must switch batch_invariant on around every sampler call"
        assert return_device and (num_node_chan, num_edge_chan) == (cfg.c_node, cfg.c_adj) and len(graph_seeds) == flags.shape[0]
        self.batches.append(flags.shape[0])
        out = [self._one(cfg, flags[b], graph_seeds[b], coin_seed) for b in range(flags.shape[0])]
        return torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])

    def sample_known(self, net, flags, ka, kn, ma, mn, **kw):
        a, x = self.sample(net, flags, **kw)
        return torch.where(ma.bool(), ka, a), torch.where(mn.bool(), kn, x)


def _flags(S=11):
    valid = [8, 3, 1, 6, 5, 2, 7, 4, 8, 1, 5][:S]
    return torch.tensor([[1] * v + [0] * (8 - v) for v in valid], dtype=torch.uint8)


def test_generate_single_process():
    net, smp, fl = _Net(), _Sampler(), _flags()
    ref = gen.generate(net, smp, fl, batch_size=4, base_seed=77, coin_seed=5)
    assert smp.batches == [4, 4, 4] and net.model.handle.log == [1, 0]
    assert ref[0].shape == (11, 6, 8, 8) and ref[1].shape == (11, 8, 12)
    cfg = net.model.config
    for k in (0, 3, 10):
        a, x = smp._one(cfg, fl[k], ddist.graph_seed(77, k), 5)
        assert torch.equal(ref[0][k], a) and torch.equal(ref[1][k], x), f"graph {k} did not get seed graph_seed(77, {k})"
    for bs in (11, 1, 64):
        got = gen.generate(net, _Sampler(), fl, batch_size=bs, base_seed=77, coin_seed=5)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    part = gen.generate(net, _Sampler(), fl[5:8], batch_size=2, base_seed=77, coin_seed=5, first_index=5)
    assert torch.equal(part[0], ref[0][5:8]) and torch.equal(part[1], ref[1][5:8])
    other = gen.generate(net, _Sampler(), fl, batch_size=4, base_seed=78, coin_seed=5)
    assert not torch.equal(other[0], ref[0])
    # known tensors are sliced per batch along with the flags; the option goes back to what it was, also when it was on
    ka, kn = torch.full((11, 6, 8, 8), 2.0), torch.full((11, 8, 12), 3.0)
    ma, mn = torch.zeros(11, 6, 8, 8, dtype=torch.uint8), torch.zeros(11, 8, 12, dtype=torch.uint8)
    ma[7, 0, 0, 1], mn[9, 0, 2] = 1, 1
    net.model.handle.value = 1
    kn_out = gen.generate(net, _Sampler(), fl, batch_size=4, base_seed=77, coin_seed=5, known=(ka, kn, ma, mn))
    assert net.model.handle.value == 1
    assert kn_out[0][7, 0, 0, 1] == 2.0 and kn_out[1][9, 0, 2] == 3.0
    ma[7, 0, 0, 1], mn[9, 0, 2] = 0, 0
    free = gen.generate(net, _Sampler(), fl, batch_size=4, base_seed=77, coin_seed=5, known=(ka, kn, ma, mn))
    assert torch.equal(free[0], ref[0]) and torch.equal(free[1], ref[1])


def test_generate_restores_the_option_after_an_error():
    class Boom(_Sampler):
        def sample(self, *a, **kw):
            raise RuntimeError("boom")
    net = _Net()
    with pytest.raises(RuntimeError):
        gen.generate(net, Boom(), _flags(), batch_size=4, base_seed=1)
    assert net.model.handle.value == 0 and net.model.handle.log == [1, 0]


def _gen_worker(rank, world, port, S, batch, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        smp = _Sampler()
        adj, node = gen.generate(_Net(), smp, _flags(S), batch_size=batch, base_seed=77, coin_seed=5)
        q.put((rank, adj.numpy(), node.numpy(), smp.batches))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("S,batch", [(11, 4), (1, 4)])
def test_generate_world2_gloo(S, batch):
    """two ranks, contiguous halves (6 + 5 graphs; or 1 + 0: a rank without a graph still joins the gather): every rank ends with the
    world-1 result"""
    ref = gen.generate(_Net(), _Sampler(), _flags(S), batch_size=batch, base_seed=77, coin_seed=5)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gen_worker, args=(r, 2, port, S, batch, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for rank, adj, node, batches in res:
        assert np.array_equal(adj, ref[0].numpy()) and np.array_equal(node, ref[1].numpy()), f"rank {rank} holds another result"
    if S == 11:
        assert res[0][3] == [4, 4] and res[1][3] == [4, 4]   # 6 and 5 graphs in two batches of four each, pads at the end
    else:
        assert res[0][3] == [1] and res[1][3] == []          # a batch of pads only is not launched
