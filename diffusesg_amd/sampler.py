"""Drop-in counterpart of `runner.mcmc_sampler.edm.NodeAdjEDMSampler` (R/runner/mcmc_sampler/edm.py:231-445).

Same constructor kwargs as `get_mc_sampler` passes (R/utils/sampling_utils.py:15-23), same `sample(...)`
signature and return convention (CPU tensors; 4-tuple with `[None]` in slot 3 when interim snapshots of a
multi-channel adjacency are requested, edm.py:439-443).  The T-step loop itself runs inside libdsg.so
(`dsg_sample`): per-step scalars are computed on the host up front, no device->host sync happens inside the
loop (the reference's per-step `.item()` logging, edm.py:433-434, is dropped), and the network forward is
replayed from a captured hipGraph.

Beyond the reference's solvers 'euler' and 'heun': solver='dpmpp_2m', a second-order multistep step (DPM-Solver++ 2M in EDM
variables) at one network forward per step -- the Euler step on the denoised estimate extrapolated from the previous step's.  It
needs S_churn = 0 (ValueError otherwise); include/dsg.h (dsg_multistep_coef), DESIGN.md §9.

Per-graph seeds (`graph_seeds=`, `coin_seed=` of `sample`, `sample_known`, `device_noise`; `dsg_sample_seeded`): every graph draws its
noise from its own stream, so its result does not depend on the batch it is generated in (`diffusesg_amd.generate`).
"""
from __future__ import annotations

import ctypes as C
import logging
from typing import Optional

import numpy as np
import torch

from . import lib as _lib
from .model import NodeAdjPrecondHip


def check_graph_seeds(graph_seeds, B: int) -> np.ndarray:
    """`graph_seeds` (list, ndarray or tensor of B integers in [0, 2**64)) as a contiguous uint64 array; ValueError / TypeError before
    anything is launched.  Values go through Python integers: no silent wrap of a negative or a too large seed."""
    if isinstance(graph_seeds, torch.Tensor):
        if graph_seeds.is_floating_point() or graph_seeds.is_complex() or graph_seeds.dtype == torch.bool:
            raise TypeError(f"graph_seeds must hold integers, got a {graph_seeds.dtype} tensor")
        graph_seeds = graph_seeds.detach().cpu().numpy()
    if isinstance(graph_seeds, np.ndarray):
        if graph_seeds.dtype.kind not in "iuO":
            raise TypeError(f"graph_seeds must hold integers, got dtype {graph_seeds.dtype}")
        vals = graph_seeds.reshape(-1).tolist() if graph_seeds.ndim == 1 else None
    else:
        vals = list(graph_seeds)
    if vals is None or len(vals) != B:
        raise ValueError(f"graph_seeds must be one seed per graph: expected {B} of them in one dimension, got "
                         f"{'shape ' + str(tuple(graph_seeds.shape)) if vals is None else len(vals)}")
    out = np.empty(B, dtype=np.uint64)
    for k, v in enumerate(vals):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"graph_seeds[{k}] = {v!r} is not an integer")
        if not 0 <= int(v) < 2 ** 64:
            raise ValueError(f"graph_seeds[{k}] = {int(v)} is outside [0, 2**64)")
        out[k] = int(v)
    return out


class NodeAdjEDMSamplerHip(object):
    def __init__(self, *, sigma_min=None, sigma_max=None, solver="heun", discretization="edm", schedule="linear",
                 scaling="none", C_1=0.001, C_2=0.008, M=1000, alpha=1,
                 num_steps=256, S_churn=40, S_min=0.05, S_max=50, S_noise=1.003,
                 clip_samples=False, clip_samples_min=None, clip_samples_max=None, clip_samples_scope="x_0",
                 self_condition=True, dev="cuda", objective="edm", symmetric_noise=False, use_graph=True):
        assert clip_samples_scope == "x_0"
        assert solver in ["euler", "heun", "dpmpp_2m"]
        assert objective in ["diffusion", "score", "edm"]
        if discretization != "edm" or schedule != "linear" or scaling != "none" or alpha != 1:
            raise NotImplementedError("only discretization='edm', schedule='linear', scaling='none', alpha=1 "
                                      "(what get_mc_sampler builds, sampling_utils.py:15-23)")
        if symmetric_noise:
            raise NotImplementedError("symmetric_noise=True is not used for scene graphs (sampling_utils.py:23)")
        if solver == "dpmpp_2m" and S_churn != 0:
            # the second-order multistep solver follows the probability-flow ODE: churn noise between two steps breaks its history
            raise ValueError(f"solver='dpmpp_2m' needs S_churn = 0 (got S_churn = {S_churn}): it reuses the previous step's denoised "
                             f"estimate, which churn noise invalidates; use solver='heun' or 'euler' with churn")
        self.solver, self.num_steps = solver, int(num_steps)
        self.S_churn, self.S_min, self.S_max, self.S_noise = S_churn, S_min, S_max, S_noise
        self.sigma_min = 0.002 if sigma_min is None else sigma_min   # edm_params.sigma_min_sampling
        self.sigma_max = 80.0 if sigma_max is None else sigma_max
        self.self_condition = self_condition
        self.dev = dev
        # stored but never applied by the reference loop either (mcmc_sampler/__init__.py:24-26)
        self.clip_samples, self.clip_samples_min, self.clip_samples_max = clip_samples, clip_samples_min, clip_samples_max
        self.symmetric_noise = False
        self.use_graph = use_graph
        self.seed = 1234
        self.last_stats = None
        self.last_guide_forwards = None   # autoguidance (net.attach_guide): the guide network's forwards in the last run
        self.sigma_steps = torch.from_numpy(_lib.sigma_schedule(self._cfg())[0])

    def _cfg(self) -> _lib.DsgSamplerCfg:
        return _lib.make_sampler_cfg(self.num_steps, self.solver, float(self.S_churn), float(self.S_min), float(self.S_max),
                                     float(self.S_noise), float(self.sigma_min), float(self.sigma_max), 7.0, self.use_graph)

    @staticmethod
    def adj_to_int(adjs_cont, node_flags, threshold):
        f = node_flags.to(adjs_cont.dtype)
        m = f.unsqueeze(-1) * f.unsqueeze(-2)
        if adjs_cont.dim() == 4:
            m = m.unsqueeze(1)
        return (adjs_cont >= threshold).to(adjs_cont.dtype) * m

    @staticmethod
    def get_num_edges(adjs_cont, node_flags, threshold):
        return (NodeAdjEDMSamplerHip.adj_to_int(adjs_cont, node_flags, threshold) > 0.0).sum([-1, -2]).float() / 2.0

    def draw_coins(self, n_calls: int) -> np.ndarray:
        """One `np.random.rand() < 0.5` per preconditioned call, in call order -- the same draws, from the same
        global NumPy generator, the reference makes inside NodeAdjPrecond.forward (precond.py:90)."""
        if not self.self_condition:
            return np.zeros(n_calls, dtype=np.uint8)
        return np.array([np.random.rand() < 0.5 for _ in range(n_calls)], dtype=np.uint8)

    def draw_coins_seeded(self, n_calls: int, coin_seed: int) -> np.ndarray:
        """The coins of a seeded run (`graph_seeds=` without `coins=`): Bernoulli(0.5) from a generator of their own, seeded with
        `coin_seed` -- the NumPy global generator is not touched, the call stays a pure function of its arguments."""
        if not self.self_condition:
            return np.zeros(n_calls, dtype=np.uint8)
        return (np.random.default_rng(int(coin_seed)).random(n_calls) < 0.5).astype(np.uint8)

    @torch.no_grad()
    def device_noise(self, model, node_flags, stream: int = 0, seed=None, graph_seeds=None):
        """The library's Philox stream `stream` for this batch, on the device: stream 0 is what `sample()` uses as
        gen_init_sample (edm.py:257-289: masked, unscaled), stream i+1 its churn noise of step i (edm.py:361-364).
        `graph_seeds` (B integers in [0, 2**64)): the per-graph streams instead -- row b is what `seed=graph_seeds[b]` gives for that
        graph alone (`dsg_gen_noise_seeded`)."""
        net = getattr(model, "module", model).model
        B = node_flags.shape[0]
        if graph_seeds is not None:
            if seed is not None:
                raise ValueError("device_noise: give seed= (one stream over the batch) or graph_seeds= (one per graph), not both")
            gs = check_graph_seeds(graph_seeds, B)
        h, cfg, dev = net._ensure_handle(), net.config, net._dev
        n = cfg.max_node_num
        fl = node_flags.to(device=dev).to(torch.uint8).contiguous()
        a = torch.empty((B, cfg.c_adj, n, n), dtype=torch.float32, device=dev)
        x = torch.empty((B, n, cfg.c_node), dtype=torch.float32, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        if graph_seeds is not None:
            h.check(h.L.dsg_gen_noise_seeded(h.raw, B, C.c_void_p(fl.data_ptr()), C.c_void_p(gs.ctypes.data), int(stream),
                                             C.c_void_p(a.data_ptr()), C.c_void_p(x.data_ptr()), C.c_void_p(st)), "dsg_gen_noise_seeded")
            return a, x
        h.check(h.L.dsg_gen_noise(h.raw, B, C.c_void_p(fl.data_ptr()), C.c_uint64(self.seed if seed is None else int(seed)),
                                  int(stream), C.c_void_p(a.data_ptr()), C.c_void_p(x.data_ptr()), C.c_void_p(st)), "dsg_gen_noise")
        return a, x

    @torch.no_grad()
    def _sample_sanity_double(self, model, node_flags, init_adjs, init_nodes, gt_adjs, gt_nodes, flag_interim_adjs, max_num_interim_adjs,
                              flag_adj_multi_channel, churn_noise, seed):
        """The float64 known-answer run (flag_use_double=True with sanity_check_gt_*; edm.py:318-445 with the denoiser bypassed): pure
        elementwise loop algebra on the device in torch float64 -- no network, hence no kernel of libdsg.so, is involved.  Returns
        float64 CPU tensors like the reference."""
        net = getattr(model, "module", model).model
        cfg, dev = net.config, net._dev
        B, n, T = node_flags.shape[0], cfg.max_node_num, self.num_steps
        f = node_flags.to(device=dev).bool()
        fa, fn = (f[:, None, :, None] & f[:, None, None, :]), f[:, :, None]
        sa, sn = (B, cfg.c_adj, n, n), (B, n, cfg.c_node)
        D = lambda t, shp: t.to(device=dev, dtype=torch.float64).reshape(shp)
        ga, gn = D(gt_adjs, sa) * fa, D(gt_nodes, sn) * fn                                   # edm.py:381-382 (masked in place)
        if init_adjs is None or init_nodes is None:                                          # gen_init_sample, edm.py:257-289
            gen = torch.Generator(device=dev).manual_seed(int(self.seed if seed is None else seed))
            init_adjs = torch.randn(sa, generator=gen, device=dev) * fa
            init_nodes = torch.randn(sn, generator=gen, device=dev) * fn
        ia, inn = D(init_adjs, sa), D(init_nodes, sn)
        t_steps = torch.cat([self.sigma_steps.to(torch.float64), torch.zeros(1, dtype=torch.float64)])   # sigma(t) = t, t_N = 0
        xa, xn = ia * t_steps[0], inn * t_steps[0]
        snaps_a, snaps_n = [ia.cpu()], [inn.cpu()]
        ts_snap = np.arange(T) if max_num_interim_adjs is None else np.linspace(0, T, max_num_interim_adjs).astype(int).clip(max=T - 1)
        for i in range(T):
            t_cur, t_next = float(t_steps[i]), float(t_steps[i + 1])
            gamma = min(self.S_churn / T, np.sqrt(2) - 1) if self.S_min <= t_cur <= self.S_max else 0
            t_hat = t_cur + gamma * t_cur
            coef = max(t_hat ** 2 - t_cur ** 2, 0.0) ** 0.5 * self.S_noise
            if churn_noise is not None:
                ea, en = D(churn_noise[0][i], sa), D(churn_noise[1][i], sn)
            else:
                ea, en = torch.randn_like(xa), torch.randn_like(xn)
            xha, xhn = (xa + coef * ea) * fa, (xn + coef * en) * fn                            # edm.py:356-366
            h = t_next - t_hat
            da, dn = ((xha - ga) / t_hat) * fa, ((xhn - gn) / t_hat) * fn                     # edm.py:384-387
            if self.solver != "heun" or i == T - 1:   # 'dpmpp_2m': D = D_prev = gt, the multistep step is the Euler step
                xa, xn = xha + h * da, xhn + h * dn                                           # edm.py:394-396
            else:
                t_prime = t_hat + h
                dpa, dpn = ((xha + h * da) - ga) / t_prime, ((xhn + h * dn) - gn) / t_prime   # edm.py:414-417 (stage 2 returns the GT again)
                xa, xn = xha + h * (0.5 * da + 0.5 * dpa), xhn + h * (0.5 * dn + 0.5 * dpn)
            xa, xn = xa * fa, xn * fn
            if flag_interim_adjs and i in ts_snap:
                snaps_a.append(xa.cpu()); snaps_n.append(xn.cpu())
        self.last_stats = {"precond_calls": 0, "net_forwards": 0, "graph_replays": 0}
        self.last_guide_forwards = 0
        sq_a = (lambda t: t[:, 0]) if cfg.c_adj == 1 else (lambda t: t)
        sq_n = (lambda t: t[..., 0]) if cfg.c_node == 1 else (lambda t: t)
        adjs, nodes = sq_a(xa.cpu()), sq_n(xn.cpu())
        if flag_interim_adjs:
            nodes_ls = torch.stack([sq_n(t) for t in snaps_n])
            if flag_adj_multi_channel:
                return adjs, nodes, [None], nodes_ls
            return adjs, nodes, torch.stack([sq_a(t) for t in snaps_a]), nodes_ls
        return adjs, nodes

    @torch.no_grad()
    def sample(self, model, node_flags, init_adjs=None, init_nodes=None,
               sanity_check_gt_adjs=None, sanity_check_gt_nodes=None,
               flag_interim_adjs=False, max_num_interim_adjs=None, flag_use_double=False,
               flag_node_multi_channel=False, flag_adj_multi_channel=False,
               num_node_chan=150, num_edge_chan=51, churn_noise=None, coins=None, seed=None, return_device=False,
               graph_seeds=None, coin_seed=None):
        """See NodeAdjEDMSampler.sample (edm.py:291).  Extra keyword-only knobs (not in the reference):
        `churn_noise=(adj [T,B,..], node [T,B,..])` and `coins` replay recorded randomness (parity tests);
        `seed` seeds the on-device Philox streams (default self.seed; the reference seeds torch per rank,
        arg_parser.py:293-294 -- set `sampler.seed = base_seed + rank`); `return_device=True` skips the final `.cpu()`.
        `graph_seeds` (B integers in [0, 2**64); list, ndarray or tensor): per-graph noise streams (`dsg_sample_seeded`) -- graph b
        draws what `seed=graph_seeds[b]` gives it at B = 1, wherever it sits in whichever batch; not together with `seed`.  The
        self-conditioning coins, one sequence per run, then come from `coins` or from `np.random.default_rng(coin_seed)`
        (`coin_seed` defaults to self.seed); the NumPy global generator is not touched."""
        if isinstance(model, (torch.nn.DataParallel, torch.nn.parallel.DistributedDataParallel)):
            model = model.module
        if graph_seeds is not None and (flag_use_double or sanity_check_gt_adjs is not None or sanity_check_gt_nodes is not None):
            raise ValueError("graph_seeds= is not available in the sanity-check mode (sanity_check_gt_* / flag_use_double)")
        if flag_use_double:
            # What the reference does with this kwarg (edm.py:320-323, :342-344, :378-380): the loop's state and time steps become float64
            # and the denoiser's output is cast up.  With a real (fp32) network the reference FAILS in its first preconditioned call --
            # the float64 state meets float32 weights ("mat1 and mat2 must have the same dtype, but got Double and Float"; checked by
            # running the reference) -- so the only form that works there is the sanity check, where the denoiser is
            # bypassed (edm.py:372-377).  Mirrored: the same RuntimeError without the ground truth, the float64 loop with it.
            if sanity_check_gt_adjs is None or sanity_check_gt_nodes is None:
                raise RuntimeError("flag_use_double=True: mat1 and mat2 must have the same dtype, but got Double and Float "
                                   "(the reference's float64 sampler state cannot be fed to its float32 network either; "
                                   "only the sanity-check form, which bypasses the network, runs in float64)")
            return self._sample_sanity_double(model, node_flags, init_adjs, init_nodes, sanity_check_gt_adjs, sanity_check_gt_nodes,
                                              flag_interim_adjs, max_num_interim_adjs, flag_adj_multi_channel, churn_noise, seed)
        return self._sample_hip(model, node_flags, init_adjs, init_nodes, sanity_check_gt_adjs, sanity_check_gt_nodes, None,
                                flag_interim_adjs, max_num_interim_adjs, flag_adj_multi_channel, num_node_chan, num_edge_chan,
                                churn_noise, coins, seed, return_device, None, graph_seeds, coin_seed)

    @torch.no_grad()
    def sample_known(self, model, node_flags, known_adjs, known_nodes, known_adj_mask, known_node_mask, *,
                     init_adjs=None, init_nodes=None, flag_interim_adjs=False, max_num_interim_adjs=None,
                     flag_node_multi_channel=False, flag_adj_multi_channel=False,
                     num_node_chan=150, num_edge_chan=51, churn_noise=None, coins=None, seed=None, return_device=False,
                     resample=None, resample_range=None, start_step=0, base_adjs=None, base_nodes=None,
                     graph_seeds=None, coin_seed=None):
        """Conditional sampling (`dsg_sample_known`; not in the reference): `sample()` with the entries selected by the masks held at
        the known values -- scene-graph completion, or layout generation when every label and relation is known and the boxes are not.
        known_adjs / known_adj_mask: [B,C_adj,N,N], known_nodes / known_node_mask: [B,N,C_node] (or squeezed, [B,N,N] / [B,N], for
        single-channel networks); masks are bool or integer, nonzero = known; the known values are in the network's value space
        (`diffusesg_amd.io.encode`).  Everything else, and the return convention, as `sample()`: no entry known gives `sample()`'s
        result bit for bit, every entry known its sanity-check mode's.

        A walk over the noise levels (`dsg_sample_walk`, `dsg_walk_cfg` in include/dsg.h); with every one of these at its default the
        call is the one above, on the same path as ever:
          resample=(jump_len, n_resample)  RePaint-style resampling: the schedule is cut into blocks of jump_len indices and each
                block is run n_resample times in a row, the state diffused back up to the block's first level in between;
          resample_range=(lo, hi)  the schedule indices the blocks partition (default: from start_step to the end; hi <= 0 = the end);
          start_step, base_adjs, base_nodes  partial-noise start: the run begins at schedule index start_step from
                base + sigma_steps[start_step] * eps (eps = init_* or the library's stream 0); base_* in the network's value space,
                shapes of known_*.  start_step > 0 needs a base.  Making the base agree with the known values at known entries is
                the caller's business.
        The walk executes L = T - start_step + (n_resample - 1)(hi - lo) steps (`lib.walk_steps`): recorded churn_noise has leading
        dimension L, coins one entry per preconditioned call of the walk, snapshots count executed steps.
        `graph_seeds`, `coin_seed`: per-graph noise streams, as in `sample()`."""
        if isinstance(model, (torch.nn.DataParallel, torch.nn.parallel.DistributedDataParallel)):
            model = model.module
        walk = None
        if resample is not None or resample_range is not None or start_step != 0 or base_adjs is not None or base_nodes is not None:
            walk = dict(resample=resample, resample_range=resample_range, start_step=start_step, base_adjs=base_adjs, base_nodes=base_nodes)
        return self._sample_hip(model, node_flags, init_adjs, init_nodes, None, None,
                                (known_adjs, known_nodes, known_adj_mask, known_node_mask),
                                flag_interim_adjs, max_num_interim_adjs, flag_adj_multi_channel, num_node_chan, num_edge_chan,
                                churn_noise, coins, seed, return_device, walk, graph_seeds, coin_seed)

    @torch.no_grad()
    def sample_guided(self, model, node_flags, guide, scale, *, clip_ratio=1.0, known=None,
                      resample=None, resample_range=None, start_step=0, base_adjs=None, base_nodes=None,
                      graph_seeds=None, coin_seed=None, return_loss_trace=False, content=None,
                      init_adjs=None, init_nodes=None, sanity_check_gt_adjs=None, sanity_check_gt_nodes=None,
                      flag_interim_adjs=False, max_num_interim_adjs=None, flag_adj_multi_channel=False,
                      num_node_chan=None, num_edge_chan=None, churn_noise=None, coins=None, seed=None, return_device=False):
        """Box guidance through the skip path, inside the loop (`dsg_sample_guided`; not in the reference): `sample()` /
        `sample_known()` with the denoised estimate of every preconditioned call shifted against the gradient of `guide`'s box loss,
            D~ = D - f_b c_i dL/dD,   c_i = w_i t^2 c_skip(t),
        the guidance of `guide.guided_sample` with the network's Jacobian dropped: an approximation (exact where that Jacobian
        vanishes) that costs one small kernel per call, no backward, and keeps step graphs, walks, known entries and per-graph seeds.
        guide: a `diffusesg_amd.guide.BoxGuide` (with `relations=`: the pairwise relation term, `dsg_sample_guided_rel`);
        scale: w, or one w_i per schedule index; clip_ratio = r: per graph the shift never exceeds r ||x_hat_b - D_b||, None: unclipped.  known = (known_adjs, known_nodes, known_adj_mask, known_node_mask) as in
        `sample_known` (known entries win and stay bit-exact); resample / resample_range / start_step / base_*: its walk;
        graph_seeds / coin_seed and everything after them: as in `sample()` (sanity_check_gt_*: the sanity-check mode, the guide then
        runs on the ground truth; not with known or graph_seeds).  Channel counts default to the network's.
        content: None, or a `diffusesg_amd.guide.ContentGuide` -- content guidance (`dsg_sample_guided_content`): a second
        shift, on the label and predicate channels, towards samples that contain the guide's triplets; it shares `scale` with the box
        terms and has a weight, a temperature and a clip of its own.  A content-only run passes guide=BoxGuide().
        scale = 0 gives `sample()` / `sample_known()` exactly.  Returns what `sample()` returns; with return_loss_trace a float32 CPU
        tensor [L, B] more: L(D) at the stage-1 call of every executed step -- and, with `content`, a second one behind it: L_content(D)."""
        from .guide import BoxGuide, ContentGuide, guidance_weights
        if isinstance(model, (torch.nn.DataParallel, torch.nn.parallel.DistributedDataParallel)):
            model = model.module
        if not isinstance(guide, BoxGuide):
            raise TypeError("sample_guided needs a diffusesg_amd.guide.BoxGuide (arbitrary losses: guide.guided_sample)")
        if content is not None and not isinstance(content, ContentGuide):
            raise TypeError("sample_guided: content must be a diffusesg_amd.guide.ContentGuide or None")
        if clip_ratio is not None and not float(clip_ratio) >= 0:
            raise ValueError(f"clip_ratio must be >= 0 or None, got {clip_ratio}")
        w = guidance_weights(scale, self.num_steps)
        gt = sanity_check_gt_adjs is not None or sanity_check_gt_nodes is not None
        if gt and (known is not None or graph_seeds is not None):
            raise ValueError("sample_guided: sanity_check_gt_* go with neither known= nor graph_seeds=")
        if known is not None and (len(known) != 4 or any(k is None for k in known)):
            raise ValueError("known = (known_adjs, known_nodes, known_adj_mask, known_node_mask)")
        walk = None
        if resample is not None or resample_range is not None or start_step != 0 or base_adjs is not None or base_nodes is not None:
            walk = dict(resample=resample, resample_range=resample_range, start_step=start_step, base_adjs=base_adjs, base_nodes=base_nodes)
        cfg = model.model.config if isinstance(model, NodeAdjPrecondHip) else None
        return self._sample_hip(model, node_flags, init_adjs, init_nodes, sanity_check_gt_adjs, sanity_check_gt_nodes, known,
                                flag_interim_adjs, max_num_interim_adjs, flag_adj_multi_channel,
                                cfg.c_node if num_node_chan is None and cfg is not None else num_node_chan,
                                cfg.c_adj if num_edge_chan is None and cfg is not None else num_edge_chan,
                                churn_noise, coins, seed, return_device, walk, graph_seeds, coin_seed,
                                guide=(guide, w, clip_ratio, bool(return_loss_trace), content))

    def _sample_hip(self, model, node_flags, init_adjs, init_nodes, sanity_check_gt_adjs, sanity_check_gt_nodes, known,
                    flag_interim_adjs, max_num_interim_adjs, flag_adj_multi_channel, num_node_chan, num_edge_chan,
                    churn_noise, coins, seed, return_device, walk=None, graph_seeds=None, coin_seed=None, guide=None):
        """The loop inside libdsg.so: `dsg_sample`, or `dsg_sample_known` when `known` = (adjs, nodes, adj mask, node mask); with
        `walk` (the walk keywords of `sample_known`) `dsg_sample_walk`; with `graph_seeds` `dsg_sample_seeded`, whatever else is given;
        with `guide` = (BoxGuide, weights [T], clip_ratio, return_loss_trace, ContentGuide | None) `dsg_sample_guided` (`_rel` with
        relations, `_content` with a ContentGuide), whatever else is given."""
        if not isinstance(model, NodeAdjPrecondHip):
            raise TypeError("NodeAdjEDMSamplerHip needs the NodeAdjPrecondHip network returned by build_network()")
        gs = None
        if graph_seeds is not None:   # refused here, before the handle is touched and anything is launched
            if seed is not None:
                raise ValueError("give seed= (one noise stream over the whole batch) or graph_seeds= (one per graph), not both")
            gs = check_graph_seeds(graph_seeds, node_flags.shape[0])
        elif coin_seed is not None:
            raise ValueError("coin_seed= belongs to graph_seeds=; an unseeded call draws its coins from the NumPy global generator")
        net = model.model
        h = net._ensure_handle()
        cfg = net.config
        assert num_node_chan == cfg.c_node and num_edge_chan == cfg.c_adj, "channel counts do not match the network"
        B, n, T = node_flags.shape[0], cfg.max_node_num, self.num_steps
        dev = net._dev
        fl = node_flags.to(device=dev).to(torch.uint8).contiguous()

        def prep(x, shape):
            return None if x is None else x.to(device=dev, dtype=torch.float32).reshape(shape).contiguous()
        sa, sn = (B, cfg.c_adj, n, n), (B, n, cfg.c_node)
        if init_adjs is None or init_nodes is None:
            init_adjs = init_nodes = None  # both are redrawn together (edm.py:325-329)
        ia, inn = prep(init_adjs, sa), prep(init_nodes, sn)
        ga, gn = prep(sanity_check_gt_adjs, sa), prep(sanity_check_gt_nodes, sn)

        # shapes are checked here, before anything is launched: the library only sees pointers
        def prep_known(x, shape, what, dtype):
            if x is None:
                return None   # the library refuses a missing tensor (DSG_ERR_INVALID)
            full = tuple(shape)
            squeezed = tuple(d for k, d in enumerate(shape) if not (d == 1 and k in (1, len(shape) - 1)))
            if tuple(x.shape) not in (full, squeezed):
                raise ValueError(f"sample_known: {what} has shape {tuple(x.shape)}, expected {full}"
                                 + (f" or {squeezed}" if squeezed != full else ""))
            if dtype is torch.uint8:
                x = x != 0
            return x.to(device=dev).to(dtype).reshape(shape).contiguous()
        if known is not None:
            ka = prep_known(known[0], sa, "known_adjs", torch.float32)
            kn = prep_known(known[1], sn, "known_nodes", torch.float32)
            ma = prep_known(known[2], sa, "known_adj_mask", torch.uint8)
            mn = prep_known(known[3], sn, "known_node_mask", torch.uint8)
        na = nn_ = None
        L = T   # executed steps
        n_calls = T if self.solver != "heun" else 2 * T - 1
        wcfg = ba = bn = None
        if walk is not None:
            # the walk, the base and the sizes of the recorded randomness: all refused here, before anything is launched
            wcfg = _lib.make_walk_cfg(walk["start_step"], walk["resample"], walk["resample_range"])
            sched, _ = _lib.walk_steps(self._cfg(), wcfg)
            L = len(sched)
            n_calls = L if self.solver != "heun" else int(2 * L - np.count_nonzero(sched == T - 1))
            if (walk["base_adjs"] is None) != (walk["base_nodes"] is None):
                raise ValueError("sample_known: base_adjs and base_nodes must both be given")
            if wcfg.start_step > 0 and walk["base_adjs"] is None:
                raise ValueError(f"sample_known: start_step = {wcfg.start_step} > 0 needs base_adjs / base_nodes (the graph the run starts from)")
            ba = prep_known(walk["base_adjs"], sa, "base_adjs", torch.float32)
            bn = prep_known(walk["base_nodes"], sn, "base_nodes", torch.float32)
            if churn_noise is not None and (churn_noise[0].shape[0] != L or churn_noise[1].shape[0] != L):
                raise ValueError(f"sample_known: churn_noise has leading dimensions {churn_noise[0].shape[0]} / {churn_noise[1].shape[0]}, "
                                 f"expected L = {L}: one slice per executed step of the walk")
            if coins is not None and np.size(coins) < n_calls:
                raise ValueError(f"sample_known: coins has {np.size(coins)} entries, the walk makes {n_calls} preconditioned calls")
        if churn_noise is not None:
            na, nn_ = prep(churn_noise[0], (L,) + sa), prep(churn_noise[1], (L,) + sn)
        if coins is None and gs is not None:
            coins = self.draw_coins_seeded(n_calls, self.seed if coin_seed is None else coin_seed)
        if coins is None:
            coins = self.draw_coins(n_calls) if ga is None else np.zeros(n_calls, np.uint8)
        coins = np.ascontiguousarray(coins, dtype=np.uint8)
        assert coins.size >= n_calls
        # snapshot schedule (edm.py:333-337, :429-432)
        snap_steps = None
        snap_a = snap_n = None
        if flag_interim_adjs:
            if max_num_interim_adjs is None:
                ts = np.arange(L)
            else:
                ts = np.linspace(0, L, max_num_interim_adjs).astype(int).clip(max=L - 1)
            snap_steps = np.ascontiguousarray(np.unique(ts), dtype=np.int32)
            snap_n = torch.empty((len(snap_steps),) + sn, dtype=torch.float32, device=dev)
            if not flag_adj_multi_channel:
                snap_a = torch.empty((len(snap_steps),) + sa, dtype=torch.float32, device=dev)
        oa = torch.empty(sa, dtype=torch.float32, device=dev)
        on = torch.empty(sn, dtype=torch.float32, device=dev)
        stats = _lib.DsgSampleStats()
        scfg = self._cfg()
        st = torch.cuda.current_stream(dev).cuda_stream
        p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
        seed_v = self.seed if seed is None else int(seed)
        if flag_interim_adjs and ia is None:
            # The reference's own call (sampler_node_adj.py:166-177) passes init_adjs=None with flag_interim_adjs=True and
            # reads slot 0 of the snapshot list as the UNSCALED initial sample (edm.py:326-337).  Draw the library's
            # init stream (noise stream 0) into caller-visible buffers first; handing them back in is bit-identical
            # to letting dsg_sample draw them itself.
            ia = torch.empty(sa, dtype=torch.float32, device=dev)
            inn = torch.empty(sn, dtype=torch.float32, device=dev)
            if gs is not None:
                h.check(h.L.dsg_gen_noise_seeded(h.raw, B, p(fl), C.c_void_p(gs.ctypes.data), 0, p(ia), p(inn), C.c_void_p(st)),
                        "dsg_gen_noise_seeded")
            else:
                h.check(h.L.dsg_gen_noise(h.raw, B, p(fl), C.c_uint64(seed_v), 0, p(ia), p(inn), C.c_void_p(st)), "dsg_gen_noise")
        snap_args = (C.c_void_p(0 if snap_steps is None else snap_steps.ctypes.data),
                     0 if snap_steps is None else len(snap_steps), p(snap_a), p(snap_n))
        trace = ctrace = None
        if guide is not None:
            bg, gw, clip_ratio, want_trace, cg = guide
            gw = np.ascontiguousarray(gw, dtype=np.float32)
            gcfg, g_keep = bg.descriptor(B, n, dev, clip_ratio)   # shapes refused here, before anything is launched
            gcfg.weights = gw.ctypes.data
            rcfg, r_keep = bg.relation_descriptor(B, n, dev, cfg.c_adj)   # ... and the relation term's kinds / table
            if want_trace:
                trace = torch.empty((L, B), dtype=torch.float32, device=dev)
            ka, kn, ma, mn = (ka, kn, ma, mn) if known is not None else (None,) * 4
            key = seed_v if gs is None else (self.seed if coin_seed is None else int(coin_seed))
            g_args = (h.raw, C.byref(scfg), C.byref(wcfg) if wcfg is not None else None, B, p(fl),
                      C.c_void_p(0 if gs is None else gs.ctypes.data), C.c_uint64(key & (2 ** 64 - 1)),
                      p(ia), p(inn), p(ba), p(bn), p(na), p(nn_), C.c_void_p(coins.ctypes.data),
                      p(ka), p(kn), p(ma), p(mn), *snap_args, C.byref(gcfg), p(ga), p(gn), p(trace),
                      p(oa), p(on), C.byref(stats), C.c_void_p(st))
            if cg is not None:   # shapes and codes refused here, before anything is launched
                ccfg, c_keep = cg.descriptor(B, cfg)
                if want_trace:   # zeros: with weight = 0 the call is dsg_sample_guided_rel, which writes no content trace
                    ctrace = torch.zeros((L, B), dtype=torch.float32, device=dev)
                h.check(h.L.dsg_sample_guided_content(*g_args, None if rcfg is None else C.byref(rcfg), C.byref(ccfg), p(ctrace)),
                        "dsg_sample_guided_content")
                del c_keep
            elif bg.relations is None:   # a guide without relations makes the call it made
                h.check(h.L.dsg_sample_guided(*g_args), "dsg_sample_guided")
            else:
                h.check(h.L.dsg_sample_guided_rel(*g_args, None if rcfg is None else C.byref(rcfg)), "dsg_sample_guided_rel")
            del g_keep, r_keep
        elif gs is not None:
            ka, kn, ma, mn = (ka, kn, ma, mn) if known is not None else (None,) * 4
            coin_seed_v = self.seed if coin_seed is None else int(coin_seed)   # (the coins are always handed over: not read by the library)
            h.check(h.L.dsg_sample_seeded(h.raw, C.byref(scfg), C.byref(wcfg) if wcfg is not None else None, B, p(fl),
                                          C.c_void_p(gs.ctypes.data), C.c_uint64(coin_seed_v & (2 ** 64 - 1)),
                                          p(ia), p(inn), p(ba), p(bn), p(na), p(nn_), C.c_void_p(coins.ctypes.data),
                                          p(ka), p(kn), p(ma), p(mn), *snap_args,
                                          p(oa), p(on), C.byref(stats), C.c_void_p(st)), "dsg_sample_seeded")
        elif walk is not None:
            ka, kn, ma, mn = (ka, kn, ma, mn) if known is not None else (None,) * 4
            h.check(h.L.dsg_sample_walk(h.raw, C.byref(scfg), C.byref(wcfg), B, p(fl), p(ia), p(inn), p(ba), p(bn), p(na), p(nn_),
                                        C.c_void_p(coins.ctypes.data), C.c_uint64(seed_v),
                                        p(ka), p(kn), p(ma), p(mn), *snap_args,
                                        p(oa), p(on), C.byref(stats), C.c_void_p(st)), "dsg_sample_walk")
        elif known is None:
            h.check(h.L.dsg_sample(h.raw, C.byref(scfg), B, p(fl), p(ia), p(inn), p(na), p(nn_),
                                   C.c_void_p(coins.ctypes.data), C.c_uint64(seed_v),
                                   p(ga), p(gn), *snap_args,
                                   p(oa), p(on), C.byref(stats), C.c_void_p(st)), "dsg_sample")
        else:
            h.check(h.L.dsg_sample_known(h.raw, C.byref(scfg), B, p(fl), p(ia), p(inn), p(na), p(nn_),
                                         C.c_void_p(coins.ctypes.data), C.c_uint64(seed_v),
                                         p(ka), p(kn), p(ma), p(mn), *snap_args,
                                         p(oa), p(on), C.byref(stats), C.c_void_p(st)), "dsg_sample_known")
        self.last_stats = {"precond_calls": stats.precond_calls, "net_forwards": stats.net_forwards,
                           "graph_replays": stats.graph_replays}
        self.last_guide_forwards = h.guide_forwards()
        logging.info("Done with EDM-NodeAdj MCMC (HIP).")
        if cfg.c_adj == 1:
            oa = oa[:, 0]
        if cfg.c_node == 1:
            on = on[..., 0]
        extra = () if trace is None else (trace.cpu(),) if ctrace is None else (trace.cpu(), ctrace.cpu())
        if return_device:
            return (oa, on) + extra if extra else (oa, on)
        adjs, nodes = oa.cpu(), on.cpu()
        if extra:
            # the guided call's returns carry the loss trace behind what `sample()` returns
            if flag_interim_adjs:
                sq_n = (lambda t: t[..., 0]) if cfg.c_node == 1 else (lambda t: t)
                sq_a = (lambda t: t[:, :, 0]) if cfg.c_adj == 1 else (lambda t: t)
                nodes_ls = sq_n(torch.cat([inn.cpu().reshape((1,) + sn), snap_n.cpu()]))
                adjs_ls = [None] if flag_adj_multi_channel else sq_a(torch.cat([ia.cpu().reshape((1,) + sa), snap_a.cpu()]))
                return (adjs, nodes, adjs_ls, nodes_ls) + extra
            return (adjs, nodes) + extra
        if flag_interim_adjs:
            # torch.stack(nodes_ls) of edm.py:441-443: slot 0 = unscaled init, then one entry per snapshot step
            sq_n = (lambda t: t[..., 0]) if cfg.c_node == 1 else (lambda t: t)
            sq_a = (lambda t: t[:, :, 0]) if cfg.c_adj == 1 else (lambda t: t)
            nodes_ls = sq_n(torch.cat([inn.cpu().reshape((1,) + sn), snap_n.cpu()]))
            if flag_adj_multi_channel:
                return adjs, nodes, [None], nodes_ls
            adjs_ls = sq_a(torch.cat([ia.cpu().reshape((1,) + sa), snap_a.cpu()]))
            return adjs, nodes, adjs_ls, nodes_ls
        return adjs, nodes
