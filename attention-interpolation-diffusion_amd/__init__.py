"""attention-interpolation-diffusion_amd — MI355X-native (gfx950 / CDNA4) interpolated attention
for diffusion (AID / PAID): a drop-in for the attention-processor hot path of
QY-H00/attention-interpolation-diffusion.

The directory name contains hyphens; import the package through the ``aid_amd`` alias module at
the repository root (``import aid_amd``).

Layout:  csrc/ (HIP kernels + C ABI, built to libaid_hip.so)  ·  _lib.py (ctypes binding)  ·
ops.py (tensor-level entry points)  ·  processors.py (the reference's AttnProcessor classes)  ·
interp.py (coefficients, slerp / lerp initialisation)  ·  attn_shim.py (diffusers stand-ins)  ·
dist.py (frame sharding over RCCL)  ·  loop.py (denoising-loop harness)  ·  sequence.py (batch assembly of
interpolate_single / N-frame interpolate)  ·  endpoint_store.py (recorded end points: render further frames between them)  ·  keyframe_store.py (key frames recorded once: render between any two)  ·  pipelines.py (the reference's pipeline classes over components)  ·  prior.py (Beta-prior exploration of the coefficient path; automatic choice of the Beta prior)  ·  metrics.py (smoothness metrics of a sequence).
"""
from .interp import (generate_beta_tensor, grid_weights, linear_interpolation, nested_slerp, simplex_weights, slerp,
                     spherical_interpolation)
from .processors import (CornerInterpolatedAttnProcessor, KeyframeBlendAttnProcessor, HipAttnProcessor, HipIPAdapterAttnProcessor, InnerInterpolatedAttnProcessor,
                         InnerInterpolatedIPAttnProcessor, InterpolatedAttnProcessor, OuterInterpolatedAttnProcessor,
                         OuterInterpolatedIPAttnProcessor, ScaleControlIPAttnProcessor, activate_aid,
                         clear_text_kv_cache, clear_weight_caches, deactivate_aid, load_aid, load_aid_ip_adapter)
from .attn_shim import AttnShim, AttnStackUNet, IPAdapterShim
from . import ops, _lib, sequence, loop, dist, metrics, prior, pipelines, endpoint_store, keyframe_store
from .endpoint_store import EndpointStore
from .keyframe_store import KeyframeBlend, KeyframeStore
from .ops import get_f32_attn_precision, set_f32_attn_precision
from .metrics import (adjacent_distances, compute_gini, compute_lpips, compute_smoothness_and_consistency,
                      separate_source_and_interpolated_images, smoothness_and_consistency_of)
from .prior import BetaPriorExplorer, BetaPriorPipeline, GaussianProcessUCB, bayesian_prior_selection
from .pipelines import (DDIMSchedulerLite, InterpolationStableDiffusionPipeline,
                        InterpolationStableDiffusionXLPipeline, StackDenoiser)

__all__ = [
    "generate_beta_tensor", "linear_interpolation", "slerp", "spherical_interpolation", "grid_weights", "simplex_weights", "nested_slerp",
    "CornerInterpolatedAttnProcessor", "KeyframeBlendAttnProcessor",
    "InterpolatedAttnProcessor", "OuterInterpolatedAttnProcessor", "InnerInterpolatedAttnProcessor",
    "OuterInterpolatedIPAttnProcessor", "InnerInterpolatedIPAttnProcessor", "ScaleControlIPAttnProcessor",
    "HipAttnProcessor", "HipIPAdapterAttnProcessor", "load_aid", "load_aid_ip_adapter", "activate_aid", "deactivate_aid",
    "clear_text_kv_cache", "clear_weight_caches",
    "AttnShim", "AttnStackUNet", "IPAdapterShim", "ops", "set_f32_attn_precision", "get_f32_attn_precision",
    "BetaPriorPipeline", "BetaPriorExplorer", "InterpolationStableDiffusionPipeline", "InterpolationStableDiffusionXLPipeline", "DDIMSchedulerLite", "StackDenoiser",
    "EndpointStore", "KeyframeStore", "KeyframeBlend",
    "bayesian_prior_selection", "GaussianProcessUCB", "compute_lpips", "compute_gini",
    "compute_smoothness_and_consistency", "separate_source_and_interpolated_images", "adjacent_distances",
    "smoothness_and_consistency_of",
]
__version__ = "0.1.0"
