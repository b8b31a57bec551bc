"""Probability-flow ODE encoder on top of `dsg_ode_run`: the latent of a graph, the graph of a latent, and the log-likelihood the model
assigns to a graph (include/dsg.h, "Probability-flow ODE between the noise levels").

The ODE dx/dt = f(x, t) = mask((x - D(x, t)) / t) runs between the sampler's noise levels t_0 = t_max > ... > t_{T-1} = t_min on the
training-form denoiser WITHOUT self-conditioning.  `encode` integrates t_min -> t_max (graph -> latent), `decode` t_max -> t_min; there
is no step to 0.  With a Hutchinson probe eps the run also returns, per evaluation, the net trace n = c_in c_out eps^T J_F eps, and

    log p_{t_min}(x_min) = -(d/2) ln(2 pi t_max^2) - |x_max|^2 / (2 t_max^2) + (d/2) ln((t_max^2 + s_d^2) / (t_min^2 + s_d^2)) - sum_k w_k n_k

(`assemble_logp`, float64 on the host; s_d = 0.5).  The prior is the sampler's N(0, t_max^2 I), not the exact marginal: for data
N(0, s^2 I) the value differs from log N(x; 0, (s^2 + t_min^2) I) by (d/2) ln(t_max^2 / (s^2 + t_max^2)), the known prior mismatch.
With synthetic weights the numbers say nothing about scene graphs; the arithmetic is pinned by tests/golden/ode_likelihood.npz.

`sampler` is a NodeAdjEDMSamplerHip; only its schedule (num_steps, sigma_min, sigma_max, S_churn = 0) and solver ('euler' | 'heun')
are read.  Here 'heun' is the true trapezoid, stage 2 evaluated at (x', t_next)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _lib

SIGMA_D = 0.5
SEED_STRIDE = 0x9E3779B97F4A7C15   # replica r of a graph probes with seed + r * SEED_STRIDE mod 2^64


def graph_dims(node_flags, c_adj: int, c_node: int) -> np.ndarray:
    """d_b = C_adj n_b^2 + C_node n_b: the live entries of every graph, int64 [B]"""
    n = np.asarray(node_flags).astype(bool).sum(-1).astype(np.int64)
    return c_adj * n * n + c_node * n


def assemble_logp(x_max_sq, net_trace, weights, dims, t_max: float, t_min: float, sigma_d: float = SIGMA_D):
    """The host formula, float64 NumPy, no GPU: x_max_sq [B] = |x_max|^2 over the live entries, net_trace [n_evals, B], weights
    [n_evals] (dsg_ode_evals), dims [B] -> (logp [B], bits_per_dim [B]).  A graph with d = 0: log p = 0, bits/dim = 0."""
    x2 = np.asarray(x_max_sq, np.float64)
    n = np.asarray(net_trace, np.float64)
    w = np.asarray(weights, np.float64)
    d = np.asarray(dims, np.float64)
    t_max, t_min, sd2 = float(t_max), float(t_min), float(sigma_d) ** 2
    quad = (w[:, None] * n).sum(0) if n.size else np.zeros_like(d)
    logp = (-0.5 * d * np.log(2.0 * np.pi * t_max * t_max) - x2 / (2.0 * t_max * t_max)
            + 0.5 * d * np.log((t_max * t_max + sd2) / (t_min * t_min + sd2)) - quad)
    logp = np.where(d > 0, logp, 0.0)
    bpd = np.where(d > 0, -logp / (np.maximum(d, 1.0) * np.log(2.0)), 0.0)
    return logp, bpd


def _net(net):
    return getattr(net, "module", net)


def _plan(sampler, direction: str, probe: str):
    scfg = sampler._cfg()
    ocfg = _lib.make_ode_cfg(direction, probe)
    t_eval, w = _lib.ode_evals(scfg, ocfg)
    _, t_hat, _, _ = _lib.sigma_schedule(scfg)
    return scfg, ocfg, t_eval, w, float(t_hat[0]), float(t_hat[-1])


def run(net, sampler, adjs, nodes, node_flags, direction: str, probe: str = "none", graph_seeds=None, probes=None,
        return_probe: bool = False):
    """One `dsg_ode_run`: (end_adj, end_node, net_trace [n_evals, B] float64 device tensor | None, (probe_adj, probe_node) | None).
    probes = (adj, node): a recorded probe (it wins over graph_seeds)."""
    import torch
    from .sampler import check_graph_seeds
    pre = _net(net)
    m = pre.model
    h = m._ensure_handle()
    if int(getattr(h.cfg, "patch_size", 1)) > 1:
        h.enable_patch_training()   # calling this is the opt-in to the training form at patch_size > 1
    scfg, ocfg, t_eval, _w, _, _ = _plan(sampler, direction, probe)
    B, a, x, fl, pa, px = m._canon(adjs, nodes, node_flags, None if probes is None else probes[0], None if probes is None else probes[1])
    gs = None if graph_seeds is None else check_graph_seeds(graph_seeds, B)
    oa, on = torch.empty_like(a), torch.empty_like(x)
    tr = torch.empty((len(t_eval), B), dtype=torch.float64, device=a.device) if probe != "none" else None
    ea, en = (torch.empty_like(a), torch.empty_like(x)) if (return_probe and probe != "none") else (None, None)
    st = torch.cuda.current_stream(m._dev).cuda_stream
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    rc = h.L.dsg_ode_run(h.raw, C.byref(scfg), C.byref(ocfg), B, p(fl), p(a), p(x), C.c_void_p(0 if gs is None else gs.ctypes.data),
                         p(pa), p(px), p(oa), p(on), p(ea), p(en), p(tr), C.c_void_p(st))
    h.check(rc, "dsg_ode_run")
    return (*m._shape_out(oa, on), tr, None if ea is None else m._shape_out(ea, en))


def encode(net, sampler, adjs, nodes, node_flags):
    """graph at t_min -> latent at t_max (lat_adjs, lat_nodes): no probe, no backward"""
    return run(net, sampler, adjs, nodes, node_flags, "encode")[:2]


def decode(net, sampler, lat_adjs, lat_nodes, node_flags):
    """latent at t_max -> state at t_min (there is no step to 0)"""
    return run(net, sampler, lat_adjs, lat_nodes, node_flags, "decode")[:2]


def _sq_norm(adj, node, B):
    return (adj.double().reshape(B, -1) ** 2).sum(1) + (node.double().reshape(B, -1) ** 2).sum(1)


def log_likelihood(net, sampler, adjs, nodes, node_flags, graph_seeds=None, probes=None, probe: str = "rademacher", n_probes: int = 1):
    """log p_{t_min} of every graph under the model: dict(logp [B] float64, bits_per_dim [B], latent (adj, node), net_trace
    [n_evals, B] float64, dims [B], weights [n_evals], t_eval [n_evals]) -- NumPy but the latent.

    n_probes = K replicates every graph K times in the batch with seeds seed + r * 0x9E3779B97F4A7C15 mod 2^64 and averages the K
    traces.  The trajectory does not depend on the probe, so the replicas' latents are equal (replica 0's is returned).  This costs 2K
    network passes per evaluation where one forward shared among the K backwards would cost 1 + K; the shared forward is not built."""
    import torch
    from .sampler import check_graph_seeds
    pre = _net(net)
    cfg = pre.model.config
    B = node_flags.shape[0]
    K = int(n_probes)
    if K < 1:
        raise ValueError("n_probes must be >= 1")
    if probes is not None and K != 1:
        raise ValueError("recorded probes go with n_probes = 1")
    if probes is None and graph_seeds is None:
        raise ValueError("log_likelihood needs graph_seeds (device-drawn probes) or probes = (adj, node)")
    rep = lambda t: t if K == 1 else torch.cat([t] * K, 0)
    gs = None
    if probes is None:
        base = check_graph_seeds(graph_seeds, B)
        gs = np.array([(int(s) + r * SEED_STRIDE) % (1 << 64) for r in range(K) for s in base], dtype=np.uint64)
    _, _, t_eval, w, t_max, t_min = _plan(sampler, "encode", probe)
    la, ln, tr, _ = run(net, sampler, rep(torch.as_tensor(adjs)), rep(torch.as_tensor(nodes)), rep(torch.as_tensor(node_flags)), "encode",
                        probe, gs, probes)
    trace = tr.cpu().numpy().reshape(len(t_eval), K, B).mean(1)
    dims = graph_dims(node_flags.cpu().numpy() if hasattr(node_flags, "cpu") else node_flags, cfg.c_adj, cfg.c_node)
    x2 = _sq_norm(la[:B], ln[:B], B).cpu().numpy()
    logp, bpd = assemble_logp(x2, trace, w, dims, t_max, t_min)
    return dict(logp=logp, bits_per_dim=bpd, latent=(la[:B], ln[:B]), latent_all=(la, ln), net_trace=trace, dims=dims, weights=w,
                t_eval=t_eval)


def sample_with_logp(net, sampler, node_flags, graph_seeds, probe: str = "rademacher"):
    """The sampler's stream-0 initial state t_0 eps of every graph (per-graph seeds), decoded along the ODE with traces:
    dict(adj, node: the states at t_min; logp, bits_per_dim, net_trace, dims, weights) -- the log p of the decoded states."""
    pre = _net(net)
    cfg = pre.model.config
    B = node_flags.shape[0]
    _, _, t_eval, w, t_max, t_min = _plan(sampler, "decode", probe)
    ea, en = sampler.device_noise(net, node_flags, stream=0, graph_seeds=graph_seeds)
    xa, xn = ea * np.float32(t_max), en * np.float32(t_max)
    oa, on, tr, _ = run(net, sampler, xa, xn, node_flags, "decode", probe, graph_seeds)
    trace = tr.cpu().numpy()
    dims = graph_dims(node_flags.cpu().numpy(), cfg.c_adj, cfg.c_node)
    logp, bpd = assemble_logp(_sq_norm(xa, xn, B).cpu().numpy(), trace, w, dims, t_max, t_min)
    return dict(adj=oa, node=on, logp=logp, bits_per_dim=bpd, net_trace=trace, dims=dims, weights=w, x_max=(xa, xn))


def graph_log_likelihood(net, sampler, q_adj, q_node, bbox, node_flags, n_adj_type: int, n_node_type: int, edge_encoding: str = "bits",
                         node_encoding: str = "bits", **kw):
    """log_likelihood of integer graphs (q_adj [B,N,N], q_node [B,N], bbox [B,N,4] | None) through `io.encode`"""
    from . import io
    a, x = io.encode(net, q_adj, q_node, bbox, node_flags, n_adj_type, n_node_type, edge_encoding, node_encoding)
    return log_likelihood(net, sampler, a, x, node_flags, **kw)


def exact_net_trace(net, adjs, nodes, node_flags, sigma: float, chunk: int = 64) -> np.ndarray:
    """sum over the live entries j of (J_D^T e_j - c_skip e_j)_j at (x, sigma), exactly: one basis cotangent e_j per live entry, `chunk`
    of them per call (the graph replicated in the batch).  float64 [B].  d network passes per graph: small networks only.

    The cotangents go through the input-gradient chain of `value_and_input_grad` (`dsg_precond_vjp`) as `dsg_ode_run` runs it: a
    recorded probe e_j on a two-level schedule whose lower level is `sigma`, one Euler evaluation.  Its trace row is e_j^T (J_D^T e_j -
    c_skip e_j) with the c_skip term never formed -- taking (J_D^T e_j)_j from `value_and_input_grad` and subtracting c_skip afterwards
    cancels seven digits at sigma = 0.002, where c_skip is 1 - 1.6e-5 and the entries of the network part are of the order of 1e-5."""
    import torch
    from .sampler import NodeAdjEDMSamplerHip
    pre = _net(net)
    cfg = pre.model.config
    n, B = cfg.max_node_num, node_flags.shape[0]
    _, a, x, fl, _, _ = pre.model._canon(adjs, nodes, node_flags, None, None)
    smp = NodeAdjEDMSamplerHip(num_steps=2, solver="euler", S_churn=0, sigma_min=float(sigma), sigma_max=2.0 * float(sigma),
                               self_condition=cfg.self_condition)
    na, nn = cfg.c_adj * n * n, n * cfg.c_node
    out = np.zeros(B, np.float64)
    f = fl.cpu().numpy().astype(bool)
    for b in range(B):
        live_a = np.broadcast_to((f[b][:, None] & f[b][None, :])[None], (cfg.c_adj, n, n)).reshape(-1)
        live_n = np.broadcast_to(f[b][:, None], (n, cfg.c_node)).reshape(-1)
        idx = np.concatenate([np.nonzero(live_a)[0], na + np.nonzero(live_n)[0]])
        for c0 in range(0, len(idx), chunk):
            js = torch.as_tensor(idx[c0:c0 + chunk], device=a.device)
            R = len(js)
            g = torch.zeros((R, na + nn), dtype=torch.float32, device=a.device)
            g[torch.arange(R, device=a.device), js] = 1.0
            ga, gn = g[:, :na].reshape(R, cfg.c_adj, n, n).contiguous(), g[:, na:].reshape(R, n, cfg.c_node).contiguous()
            tr = run(net, smp, a[b:b + 1].expand(R, -1, -1, -1), x[b:b + 1].expand(R, -1, -1), fl[b:b + 1].expand(R, -1), "encode",
                     "rademacher", None, (ga, gn))[2]
            out[b] += float(tr[0].sum().item())
    return out


def _slerp(za, zb, w):
    """spherical interpolation of two flat vectors per graph (rows), weight w of zb; falls back to the line where they are parallel"""
    import torch
    na, nb = za.norm(dim=1, keepdim=True).clamp_min(1e-30), zb.norm(dim=1, keepdim=True).clamp_min(1e-30)
    cos = ((za / na) * (zb / nb)).sum(1, keepdim=True).clamp(-1.0, 1.0)
    om = torch.acos(cos)
    so = torch.sin(om)
    lin = so.abs() < 1e-6
    so = torch.where(lin, torch.ones_like(so), so)
    ca = torch.where(lin, 1.0 - w, torch.sin((1.0 - w) * om) / so)
    cb = torch.where(lin, w, torch.sin(w * om) / so)
    return ca * za + cb * zb


def interpolate(net, sampler, graph_a, graph_b, node_flags, weights):
    """encode both graphs, interpolate the latents spherically per graph, decode: a list of (adj, node) states at t_min, one per weight
    (the weight of graph_b).  Both graphs share node_flags: one flag row per pair, refused otherwise."""
    import torch
    (aa, an), (ba, bn) = graph_a, graph_b
    if tuple(aa.shape) != tuple(ba.shape) or tuple(an.shape) != tuple(bn.shape) or aa.shape[0] != node_flags.shape[0]:
        raise ValueError("interpolate: both graphs must have the same shapes and one flag row each (equal flag rows for a and b)")
    B = node_flags.shape[0]
    za_a, za_n = encode(net, sampler, aa, an, node_flags)
    zb_a, zb_n = encode(net, sampler, ba, bn, node_flags)
    cut = za_a.reshape(B, -1).shape[1]
    za = torch.cat([za_a.reshape(B, -1), za_n.reshape(B, -1)], 1).double()
    zb = torch.cat([zb_a.reshape(B, -1), zb_n.reshape(B, -1)], 1).double()
    out = []
    for w in weights:
        z = _slerp(za, zb, torch.full((B, 1), float(w), dtype=torch.float64, device=za.device)).float()
        out.append(decode(net, sampler, z[:, :cut].reshape(za_a.shape), z[:, cut:].reshape(za_n.shape), node_flags))
    return out
