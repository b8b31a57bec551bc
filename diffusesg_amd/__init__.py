"""diffusesg_amd: MI355X-native scene-graph diffusion sampler (denoiser forward + EDM reverse loop).

The product is libdsg.so (diffusesg_amd/csrc, include/dsg.h); this package is the thin Python host
side mirroring the reference's `model/` and `runner/mcmc_sampler/` callables."""
from .spec import ModelConfig, tiny_config, vg_config, coco_config  # noqa: F401

__all__ = ["ModelConfig", "tiny_config", "vg_config", "coco_config",
           "guided_sample", "box_region_loss", "box_overlap_loss", "box_alignment_loss", "box_relation_loss",
           "encode", "decode", "log_likelihood", "sample_with_logp", "graph_log_likelihood", "exact_net_trace", "interpolate",
           "assemble_logp"]

_GUIDE = ("guided_sample", "box_region_loss", "box_overlap_loss", "box_alignment_loss", "box_relation_loss")
_ODE = ("encode", "decode", "log_likelihood", "sample_with_logp", "graph_log_likelihood", "exact_net_trace", "interpolate", "assemble_logp")


def __getattr__(name):
    # loss-guided sampling (diffusesg_amd.guide) pulls in torch: resolved on first use, so that `import diffusesg_amd` stays light
    if name in _GUIDE:
        from . import guide
        return getattr(guide, name)
    # the probability-flow ODE encoder (diffusesg_amd.ode): latents and log-likelihood of graphs
    if name in _ODE:
        from . import ode
        return getattr(ode, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
