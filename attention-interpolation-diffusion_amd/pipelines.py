"""Pipeline surface of the reference over the HIP attention path.

``InterpolationStableDiffusionPipeline`` / ``InterpolationStableDiffusionXLPipeline`` keep the method names and keyword
arguments of the reference's pipelines —

    load_aid(t, is_fused, atype)                        pipeline_interpolated_sd.py:950-970
    load_aid_ip_adapter(..., t, is_fused, early)        :972-1007
    activate_aid(it) / deactivate_aid()                 :1008-1017
    interpolate_single(it, prompt_start, prompt_end, latent_start, latent_end, image_start, image_end,
                       guide_prompt, warmup_ratio, is_fused, atype, init, ...)           :1407-1963, sdxl :1693-2411
    interpolate(latent_start, latent_end, prompt_start, prompt_end, guide_prompt, negative_prompt, size,
                num_inference_steps, warmup_ratio, early, late, alpha, beta, guidance_scale)
                                                        gradio_src/pipeline_interpolated_stable_diffusion.py:163-304

— and run the same host logic: batch ``[start, interior ..., end]``, slerp'd latents, lerp / slerp / guide-prompt
embeddings, the conditional pass with AID on for ``i < int(T * warmup_ratio)`` and the unconditional pass plain,
``uncond + gs * (text - uncond)``, scheduler step.  Everything the reference inherits from diffusers (UNet, scheduler,
VAE, text / image encoders — "Copied from diffusers" in the reference, out of scope per SURVEY.md §2) is a COMPONENT
handed to the constructor, duck-typed on the diffusers interfaces:

    unet(sample, t, encoder_hidden_states=..., added_cond_kwargs=..., return_dict=False)[0]
        + ``attn_processors`` / ``set_attn_processor``          scheduler.set_timesteps / timesteps / scale_model_input /
    step(noise, t, latents, return_dict=False)[0] / init_noise_sigma          vae.decode(latents, return_dict=False)[0]
    encode_prompt(prompt, negative_prompt) -> (cond, uncond)   [SDXL: (cond, uncond, pooled, negative_pooled)]

so ``from_pipe(diffusers_pipeline)`` wraps a loaded diffusers pipeline where diffusers exists, and the tests / the build
image (no diffusers, no weights) use :class:`DDIMSchedulerLite` and :class:`StackDenoiser` — a stand-in UNet whose blocks
are the ordered attention layers of the real UNet (``AttnStackUNet``) on a chained residual stream.

MI355X-first: ``interpolate`` runs the two passes of a step as ONE UNet call ``[cond ; uncond]`` by default (the AID
processors treat the second half as plain riders), every attention call is one library call, and the interior frames of
a guide-prompt run share one projected text context (``ctx_index``).
"""
from __future__ import annotations

import inspect
import warnings

from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import nn

from . import ops
from . import processors as P
from ._lib import KF_MAX_ROWS
from .attn_shim import AttnStackUNet
from .interp import (corner_rows_of, weight_rows_of, generate_beta_tensor, linear_interpolation, nested_slerp, slerp,
                     spherical_interpolation)
from .endpoint_store import EndpointStore, run_settings, run_signature
from .keyframe_store import KeyframePair, KeyframeStore
from .loop import EARLY_MODES, install_blend_processors, install_corner_processors, install_sequence_processors, set_aid_active, set_ctx_index, set_endpoint_store, set_keyframe_store
from .sequence import SequenceBatch, prepare_sequence, prepare_single


# ---------------------------------------------------------------------------------------------
# components used where diffusers is absent
# ---------------------------------------------------------------------------------------------
class DDIMSchedulerLite:
    """DDIM on the scaled-linear beta schedule of SD / SDXL — the published update
    x_{t-1} = sqrt(a_{t-1}) x0 + sqrt(1 - a_{t-1} - s^2) eps + s z with x0 = (x_t - sqrt(1 - a_t) eps) / sqrt(a_t) and
    s^2 = eta^2 (1 - a_{t-1}) / (1 - a_t) (1 - a_t / a_{t-1}) (Song et al. 2021, eq. 12 and 16; deterministic at the default eta = 0)
    — behind the diffusers scheduler interface the pipelines use (third-party there; north_star names 50-step DDIM).
    ``set_timesteps(timesteps=[...])`` takes a custom table (descending integers in [0, num_train_timesteps)); there is no
    ``sigmas`` keyword, as on diffusers' DDIMScheduler."""
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 steps_offset: int = 1):
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float64) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.num_train_timesteps = num_train_timesteps
        self.steps_offset = steps_offset
        self.timesteps = torch.arange(num_train_timesteps - 1, -1, -1)
        self.num_inference_steps = num_train_timesteps
        self._prev: Optional[Dict[int, int]] = None        # custom table: timestep -> the next one (-1 behind the last)

    def set_timesteps(self, num_inference_steps: Optional[int] = None, device=None, timesteps: Optional[Sequence[int]] = None):
        if timesteps is not None:
            if num_inference_steps is not None:
                raise ValueError("pass num_inference_steps or timesteps, not both")
            tl = timesteps.tolist() if torch.is_tensor(timesteps) else list(timesteps)
            if not tl or any(int(t) != t for t in tl):
                raise ValueError("timesteps must be a non-empty list of integers")
            tl = [int(t) for t in tl]
            if any(a <= b for a, b in zip(tl, tl[1:])) or tl[-1] < 0 or tl[0] >= self.num_train_timesteps:
                raise ValueError(f"timesteps must be descending integers in [0, {self.num_train_timesteps}); got {tl}")
            ts = torch.tensor(tl, dtype=torch.int64)
            self.timesteps = ts.to(device) if device is not None else ts
            self.num_inference_steps = len(tl)
            self._prev = dict(zip(tl, tl[1:] + [-1]))
            return
        if num_inference_steps is None:
            raise ValueError("pass num_inference_steps or timesteps")
        self._prev = None
        ratio = self.num_train_timesteps // num_inference_steps
        ts = (torch.arange(0, num_inference_steps) * ratio).flip(0) + self.steps_offset      # "leading" spacing
        self.timesteps = ts.to(device) if device is not None else ts
        self.num_inference_steps = num_inference_steps

    def scale_model_input(self, sample, timestep=None):
        return sample

    def step(self, model_output, timestep, sample, eta: float = 0.0, generator=None, return_dict: bool = False, **kwargs):
        t = int(timestep)
        prev = t - self.num_train_timesteps // self.num_inference_steps if self._prev is None else self._prev[t]
        a_t = self.alphas_cumprod[t]
        a_p = self.alphas_cumprod[prev] if prev >= 0 else torch.tensor(1.0, dtype=torch.float64)
        a_t, a_p = float(a_t), float(a_p)
        eps = model_output.to(torch.float32)
        x = sample.to(torch.float32)
        x0 = (x - (1 - a_t) ** 0.5 * eps) / a_t ** 0.5
        if eta == 0.0:
            out = (a_p ** 0.5 * x0 + (1 - a_p) ** 0.5 * eps).to(sample.dtype)
            return (out,)
        var = float(eta) ** 2 * (1 - a_p) / (1 - a_t) * (1 - a_t / a_p)
        gdev = generator.device if generator is not None else sample.device       # a host generator seeds a device run, as in diffusers
        z = torch.randn(sample.shape, generator=generator, device=gdev, dtype=torch.float32).to(sample.device)
        out = (a_p ** 0.5 * x0 + max(1 - a_p - var, 0.0) ** 0.5 * eps + var ** 0.5 * z).to(sample.dtype)
        return (out,)


class StackDenoiser(nn.Module):
    """Stand-in UNet for the build image: latents ``[N, 4, h, w]`` are lifted to the token streams of every resolution
    level by fixed linear maps, run through the ordered attention layers of the real UNet (``AttnStackUNet``; per block
    ``h += attn1(norm(h))``, ``h += attn2(norm(h), ctx)``) and projected back to a noise prediction.  All the arithmetic
    between the attention calls of the real UNet (convs, MLPs, time embedding) is third-party and absent here; the
    attention layers are exactly the ones the reference wraps.  ``sublayers``: "fused" = one library call per layer,
    "steps" = torch LayerNorm / processor call / torch add."""

    def __init__(self, model: str = "sd15", dtype=torch.float16, device=None, seed: int = 1002, scale_down: int = 16,
                 latent_hw: Tuple[int, int] = (16, 16), sublayers: str = "fused", head_div: int = 1):
        super().__init__()
        self.stack = AttnStackUNet(model, dtype=dtype, device=device, seed=seed, scale_down=scale_down, head_div=head_div)
        self.stack.sublayers = sublayers
        self.latent_hw = latent_hw
        self.in_channels = 4
        dev = self.stack.layers[0].to_q.weight.device
        g = torch.Generator(device=dev).manual_seed(seed + 1)
        n_lat = 4 * latent_hw[0] * latent_hw[1]
        self.lift, self.drop = nn.ParameterDict(), nn.ParameterDict()
        for (s, c) in self.stack.level_shapes():
            key = f"{s}_{c}"
            self.lift[key] = nn.Parameter((torch.randn(n_lat, s * 8, generator=g, device=dev) / n_lat ** 0.5).to(dtype),
                                          requires_grad=False)
            self.drop[key] = nn.Parameter((torch.randn(s * 8, n_lat, generator=g, device=dev) / (s * 8) ** 0.5).to(dtype),
                                          requires_grad=False)
        self.time_scale = 1.0 / 1000.0

    # diffusers' processor surface
    @property
    def attn_processors(self):
        return self.stack.attn_processors

    def set_attn_processor(self, processor):
        self.stack.set_attn_processor(processor)

    @property
    def dtype(self):
        return self.stack.layers[0].to_q.weight.dtype

    @property
    def device(self):
        return self.stack.layers[0].to_q.weight.device

    def forward(self, sample, timestep=None, encoder_hidden_states=None, added_cond_kwargs=None, return_dict=False, **kw):
        n = sample.shape[0]
        flat = sample.reshape(n, -1).to(self.dtype)
        # the timestep is used as a device scalar (no host read): the call can be captured into a hipGraph and replayed with
        # another timestep in the same buffer, like a real UNet's timestep embedding
        tshift = None
        if timestep is not None:
            tshift = (timestep if torch.is_tensor(timestep) else torch.tensor(float(timestep))).to(flat.device, torch.float32) * self.time_scale
        xs = {}
        for (s, c) in self.stack.level_shapes():
            tok = (flat @ self.lift[f"{s}_{c}"]).view(n, s, 8)                       # [N, S, 8] tokens ...
            wide = tok.repeat(1, 1, c // 8)                                          # ... tiled to the level width
            xs[(s, c)] = (wide if tshift is None else wide + tshift).contiguous()
        ehs = encoder_hidden_states
        if added_cond_kwargs and added_cond_kwargs.get("image_embeds") is not None:  # IP-Adapter UNets hand (text, [ip])
            ehs = (encoder_hidden_states, list(added_cond_kwargs["image_embeds"]))
        hs = self.stack(xs, ehs)
        out = torch.zeros_like(flat)
        for (s, c) in self.stack.level_shapes():
            h = hs[(s, c)].view(n, s, c // 8, 8).mean(dim=2)                          # [N, S, 8]
            out = out + h.reshape(n, s * 8) @ self.drop[f"{s}_{c}"]
        out = (out / len(self.stack.level_shapes())).view_as(sample).to(sample.dtype)
        return (out,)


# ---------------------------------------------------------------------------------------------
class _PassGraphs:
    """hipGraph capture of the distinct UNet passes of ONE denoising run (the loop it serves is
    pipeline_interpolated_sd.py:1834-1907).  A run has at most three kinds of pass — conditional with AID on, conditional
    plain, unconditional (or the two batched variants) — each launching a few hundred kernels per call.  The first call of
    a kind runs once eagerly (lazy kernel attributes, coefficient buffers, workspaces, the text K / V cache), is captured, and
    every later step only copies the step's inputs (scaled latents, timestep) into the captured buffers and replays.
    ``activate_aid(it)`` rewrites the coefficient buffers in place, so a replay reads the live schedule.

    What a replay FREEZES: every Python-side decision of the first call of a pass kind — the frame -> context map
    (``ctx_index``), ``plain_tail``, the IP-Adapter scales, which processor object sits on which layer, and the unmerged LoRA
    adapters: their active set, their scalings (``cross_attention_kwargs["scale"]`` included) and the packed factors (lora.py).  A
    ``callback_on_step_end`` that swaps processors or embeddings between steps has no effect on replayed passes: run such loops
    with ``use_graphs=False``.  Each pass kind also holds a private pool with one UNet pass of activations.

    A UNet whose forward cannot be captured (a host synchronisation or a host -> device copy inside it) does not abort the
    run: the failed capture is abandoned, graphs are switched off for the rest of the run (``self.enabled = False``,
    ``self.fallback_reason`` says why) and the pass runs eagerly."""

    def __init__(self, enabled: bool):
        self.enabled = bool(enabled)
        self.fallback_reason: Optional[str] = None
        self._ent: Dict[Any, Tuple] = {}
        self._cap = None
        self._ws = ops.WorkspaceOwner()          # the captures' workspaces go when this object (and its graphs) goes

    def _capture(self, fn: Callable, inputs: Dict[str, torch.Tensor]):
        static = {k: v.clone() for k, v in inputs.items()}
        cur = torch.cuda.current_stream()
        if self._cap is None:
            self._cap = torch.cuda.Stream()         # warm-up AND capture stream: the capture adopts the warm-up's workspace (ops.workspace)
        cap = self._cap
        cap.wait_stream(cur)
        with torch.cuda.stream(cap):
            fn(**static)
        cur.wait_stream(cap)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with self._ws, torch.cuda.graph(graph, stream=cap):
            out = fn(**static)
        return graph, static, out

    @staticmethod
    def _key(key):
        """A captured pass holds the kernels of the float32 matmul precision it was captured under (the processors read
        ``torch.get_float32_matmul_precision()`` per call) and of the attention core's precision (``ops.set_f32_attn_precision``): a
        change of either re-captures instead of replaying stale graphs, changing it back replays the old ones."""
        return (key, ops.f32_split_code(), ops.f32_attn_split_code())

    def run(self, key, fn: Callable, **inputs: torch.Tensor):
        if not self.enabled:
            return fn(**inputs)
        key = self._key(key)
        ent = self._ent.get(key)
        if ent is None:
            try:
                ent = self._capture(fn, inputs)
            except RuntimeError as e:           # what a foreign UNet does that a stream capture forbids surfaces as RuntimeError
                # (hipErrorStreamCaptureUnsupported & co. through torch); anything else is a bug and propagates.  The fallback is
                # loud: a run that silently lost its graphs is a large performance regression
                self.enabled = False
                self.fallback_reason = f"{type(e).__name__}: {e}"
                self._ent.clear()
                self._ws.release()              # the graphs are gone (and so is the failed capture): their workspaces too
                warnings.warn("hipGraph capture of a UNet pass failed, the run continues eagerly: " + self.fallback_reason,
                              RuntimeWarning, stacklevel=3)
                try:
                    torch.cuda.synchronize()    # an invalidated capture may leave a sticky error behind: report it, do not hide it
                except RuntimeError as e2:
                    raise RuntimeError(f"device unusable after a failed stream capture ({self.fallback_reason})") from e2
                return fn(**inputs)
            self._ent[key] = ent
        graph, static, out = ent
        for k, v in inputs.items():
            static[k].copy_(v)
        graph.replay()
        return out                      # captured output buffer: consume it before the same kind of pass runs again


def _use_graphs(flag: Optional[bool], device: torch.device) -> bool:
    return (device.type == "cuda" and torch.cuda.is_available()) if flag is None else bool(flag)


def _retrieve_timesteps(scheduler, num_inference_steps: Optional[int], device, timesteps=None, sigmas=None) -> Tuple[Any, int]:
    """``scheduler.set_timesteps`` with a custom ``timesteps`` or ``sigmas`` table where one is given (pipeline_interpolated_sd.py:111-154,
    called at :1716): returns ``(scheduler.timesteps, len(scheduler.timesteps))``.  Both given, or a scheduler whose ``set_timesteps``
    lacks the keyword, raises ``ValueError``."""
    if timesteps is not None and sigmas is not None:
        raise ValueError("pass only one of `timesteps` and `sigmas` to set a custom schedule")
    for name, table in (("timesteps", timesteps), ("sigmas", sigmas)):
        if table is None:
            continue
        if name not in inspect.signature(scheduler.set_timesteps).parameters:
            raise ValueError(f"{type(scheduler).__name__}.set_timesteps takes no `{name}`: this scheduler does not support a custom "
                             f"{name} schedule")
        scheduler.set_timesteps(device=device, **{name: table})
        return scheduler.timesteps, len(scheduler.timesteps)
    scheduler.set_timesteps(num_inference_steps, device=device)
    return scheduler.timesteps, num_inference_steps


def _extra_step_kwargs(scheduler, eta: float, generator) -> Dict[str, Any]:
    """``eta`` / ``generator`` for ``scheduler.step``, each only where its signature accepts it (pipeline_interpolated_sd.py:782-795): not
    every scheduler is DDIM."""
    accepted = inspect.signature(scheduler.step).parameters
    extra: Dict[str, Any] = {}
    if "eta" in accepted:
        extra["eta"] = eta
    if "generator" in accepted:
        extra["generator"] = generator
    return extra


def _check_rescale(guidance_rescale: float) -> float:
    r = float(guidance_rescale)
    if not 0.0 <= r <= 1.0:
        raise ValueError(f"guidance_rescale must be in [0, 1]; got {guidance_rescale}")
    return r


def _guided_noise(noise_text: torch.Tensor, noise_unc: torch.Tensor, gs: float, rescale: float) -> torch.Tensor:
    """Classifier-free guidance (pipeline_interpolated_sd.py:1892) and, with ``rescale > 0`` (:1896-1902), the guidance rescale: then
    both in one launch of the library (``ops.cfg_rescale``: the two noise tensors may be the halves of one batched output).  With
    ``rescale == 0`` the torch expression the loops have always run."""
    if rescale > 0.0:
        return ops.cfg_rescale(noise_text, noise_unc, gs, rescale)
    return noise_unc + gs * (noise_text - noise_unc)


def _dev_scalar(t, device: torch.device) -> torch.Tensor:
    """The step's timestep as a device tensor (graph input); schedulers hand out device or host scalars."""
    if torch.is_tensor(t):
        return t if t.device == device else t.to(device)
    return torch.tensor(t, device=device)


# ---------------------------------------------------------------------------------------------
class InterpolationStableDiffusionPipeline:
    """See the module docstring.  ``encode_prompt`` (callable) turns a prompt string into ``(cond, uncond)`` embeddings
    ``[1, L, Cc]``; without it pass embeddings directly (``embeds_start`` / ``embeds_end`` / ``embeds_guide``)."""

    is_xl = False
    default_guidance_scale = 7.5

    def __init__(self, unet, scheduler, vae=None, encode_prompt: Optional[Callable] = None,
                 encode_image: Optional[Callable] = None, vae_scaling_factor: float = 0.18215):
        self.unet, self.scheduler, self.vae = unet, scheduler, vae
        self._encode_prompt, self._encode_image = encode_prompt, encode_image
        self.vae_scaling_factor = vae_scaling_factor
        self._guidance_scale = self.default_guidance_scale
        self._guidance_rescale = 0.0
        self._aid_early: Optional[str] = None

    # -- wrapping a loaded diffusers pipeline (only where diffusers is importable) -----------------
    @classmethod
    def from_pipe(cls, pipe):
        """Take ``unet / scheduler / vae / encode_prompt`` from a loaded diffusers (SD or SDXL) pipeline."""
        def enc(prompt, negative_prompt=None, lora_scale=None):
            out = pipe.encode_prompt(prompt, pipe._execution_device, 1, True, negative_prompt=negative_prompt,
                                     lora_scale=lora_scale) \
                if not cls.is_xl else pipe.encode_prompt(prompt=prompt, device=pipe._execution_device,
                                                         num_images_per_prompt=1, do_classifier_free_guidance=True,
                                                         negative_prompt=negative_prompt, lora_scale=lora_scale)
            return out
        sf = getattr(getattr(pipe.vae, "config", None), "scaling_factor", 0.18215)
        enc_img = None
        if hasattr(pipe, "prepare_ip_adapter_image_embeds"):
            def enc_img(image):
                """(negative, positive) image embeddings of one image, as the reference takes them from diffusers'
                prepare_ip_adapter_image_embeds with classifier-free guidance on (pipeline_interpolated_sd.py:1763-1802)."""
                embeds = pipe.prepare_ip_adapter_image_embeds(image, None, pipe._execution_device, 1, True)[0]
                neg, pos = embeds.chunk(2)
                return neg, pos
        obj = cls(pipe.unet, pipe.scheduler, pipe.vae, encode_prompt=enc, encode_image=enc_img, vae_scaling_factor=sf)
        obj._load_ip_adapter = getattr(pipe, "load_ip_adapter", None)      # diffusers' loader: load_aid_ip_adapter(path, ...) uses it
        obj._pipe = pipe                                                  # its LoRA loader methods (load_lora_weights & co.) below
        return obj

    # -- LoRA (diffusers' StableDiffusionLoraLoaderMixin of the wrapped pipeline, pipeline_interpolated_sd.py:283-299) ----------------
    # Each method changes adapter weights or their state in place; the caches derived from weights are dropped after it, like
    # _load_ip_adapter does.  Unmerged adapters run inside the projection GEMMs (lora.py); fuse_lora() folds them into the weights.
    def _lora_call(self, name: str, *args, **kwargs):
        fn = getattr(getattr(self, "_pipe", None), name, None)
        if fn is None:
            raise RuntimeError(f"{name} is diffusers' LoRA loader: wrap a diffusers pipeline with from_pipe")
        out = fn(*args, **kwargs)
        P.clear_weight_caches()
        return out

    def load_lora_weights(self, *args, **kwargs):
        return self._lora_call("load_lora_weights", *args, **kwargs)

    def set_adapters(self, *args, **kwargs):
        return self._lora_call("set_adapters", *args, **kwargs)

    def fuse_lora(self, *args, **kwargs):
        return self._lora_call("fuse_lora", *args, **kwargs)

    def unfuse_lora(self, *args, **kwargs):
        return self._lora_call("unfuse_lora", *args, **kwargs)

    def enable_lora(self, *args, **kwargs):
        return self._lora_call("enable_lora", *args, **kwargs)

    def disable_lora(self, *args, **kwargs):
        return self._lora_call("disable_lora", *args, **kwargs)

    # -- the reference's AID methods ----------------------------------------------------------------
    def load_aid(self, t: Optional[float] = 0.5, is_fused: bool = True, atype: str = "fused_outer", **kw):
        P.load_aid(self.unet, t=t, is_fused=is_fused, atype=atype, **kw)
        self._aid_early = atype

    def load_aid_ip_adapter(self, pretrained_model_name_or_path_or_dict=None, subfolder=None, weight_name=None,
                            t: Optional[float] = 0.5, is_fused: bool = True,
                            image_encoder_folder: Optional[str] = "image_encoder", early: str = "fused_outer", **kwargs):
        """pipeline_interpolated_sd.py:972-1007.  Loading the adapter weights is diffusers' ``load_ip_adapter``
        (third-party): it is called on the wrapped pipeline / UNet when that offers it; a UNet whose IP-Adapter
        processors are already installed (``AttnStackUNet.load_ip_adapter`` in the build image) is wrapped as is."""
        loader = getattr(self.unet, "load_ip_adapter_weights", None) or getattr(self, "_load_ip_adapter", None)
        if pretrained_model_name_or_path_or_dict is not None:
            if loader is None:
                raise RuntimeError("loading IP-Adapter weights needs diffusers' load_ip_adapter (wrap a diffusers pipeline "
                                   "with from_pipe), or install the adapter on the UNet first")
            loader(pretrained_model_name_or_path_or_dict, subfolder=subfolder, weight_name=weight_name,
                   image_encoder_folder=image_encoder_folder, **kwargs)
        P.load_aid_ip_adapter(self.unet, t=t, is_fused=is_fused, early=early)
        self._aid_early = early

    def activate_aid(self, it: float):
        P.activate_aid(self.unet, it)

    def deactivate_aid(self):
        P.deactivate_aid(self.unet)

    @property
    def guidance_scale(self):
        return self._guidance_scale

    @property
    def guidance_rescale(self):
        return self._guidance_rescale

    @property
    def do_classifier_free_guidance(self):
        return self._guidance_scale > 1

    # -- helpers ---------------------------------------------------------------------------------------
    def _embed(self, prompt, negative_prompt, given, lora_scale=None):
        if given is not None:
            return tuple(given)
        if prompt is None or self._encode_prompt is None:
            raise ValueError("pass a prompt and an `encode_prompt` component, or the embeddings themselves "
                             "(embeds_start / embeds_end / embeds_guide)")
        if lora_scale is not None:          # cross_attention_kwargs["scale"] -> encode_prompt(lora_scale=) (pipeline_interpolated_sd.py:1647-1686)
            return tuple(self._encode_prompt(prompt, negative_prompt, lora_scale=lora_scale))
        return tuple(self._encode_prompt(prompt, negative_prompt))

    def prepare_latents(self, batch_size, num_channels_latents, height, width, dtype, device, generator, latents=None):
        """pipeline_interpolated_sd.py:881-920: N(0, 1) * scheduler.init_noise_sigma unless given."""
        if latents is None:
            shape = (batch_size, num_channels_latents, height, width)
            latents = torch.randn(shape, generator=generator, dtype=torch.float32).to(device=device, dtype=dtype)
        else:
            latents = latents.to(device=device, dtype=dtype)
        return latents * getattr(self.scheduler, "init_noise_sigma", 1.0)

    def _added_cond(self, pooled, n: int, image_embeds=None) -> Optional[Dict[str, Any]]:
        return None if image_embeds is None else {"image_embeds": image_embeds}

    def _unet(self, latents, t, ctx, added, cross_attention_kwargs=None):
        if cross_attention_kwargs is not None:      # diffusers' UNet applies its "scale" to the LoRA layers for the call
            return self.unet(latents, t, encoder_hidden_states=ctx, added_cond_kwargs=added,
                             cross_attention_kwargs=cross_attention_kwargs, return_dict=False)[0]
        return self.unet(latents, t, encoder_hidden_states=ctx, added_cond_kwargs=added, return_dict=False)[0]

    def _decode(self, latents, output_type: str):
        if output_type == "latent" or self.vae is None:
            return latents
        image = self.vae.decode(latents / self.vae_scaling_factor, return_dict=False)[0]
        if output_type == "pt":
            return image
        return ((image / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1) * 255).to(torch.uint8).cpu().numpy()

    # -- interpolate_single (batch 3) ---------------------------------------------------------------------
    @torch.no_grad()
    def interpolate_single(self, it: float = 0.5, prompt_start: Optional[str] = None, prompt_end: Optional[str] = None,
                           latent_start: Optional[torch.Tensor] = None, latent_end: Optional[torch.Tensor] = None,
                           image_start=None, image_end=None, guide_prompt: Optional[str] = None,
                           warmup_ratio: float = 0.5, is_fused: bool = True, atype: str = "outer", init: str = "linear",
                           height: Optional[int] = None, width: Optional[int] = None, num_inference_steps: int = 50,
                           timesteps: Optional[List[int]] = None, sigmas: Optional[List[float]] = None,
                           guidance_scale: Optional[float] = None, negative_prompt=None,
                           num_images_per_prompt: Optional[int] = 1, eta: float = 0.0, generator=None,
                           latents: Optional[torch.Tensor] = None, prompt_embeds=None, negative_prompt_embeds=None,
                           ip_adapter_image=None, ip_adapter_image_embeds=None, output_type: Optional[str] = "pil",
                           return_dict: bool = True, cross_attention_kwargs: Optional[Dict[str, Any]] = None,
                           guidance_rescale: float = 0.0, clip_skip: Optional[int] = None,
                           callback_on_step_end: Optional[Callable] = None,
                           callback_on_step_end_tensor_inputs: Sequence[str] = ("latents",),
                           # build-specific: embeddings instead of prompt strings / images
                           embeds_start=None, embeds_end=None, embeds_guide=None,
                           image_embeds_start=None, image_embeds_end=None, use_graphs: Optional[bool] = None,
                           endpoints: Optional[EndpointStore] = None, **kwargs):
        """Batch ``[start, target(it), end]`` through the denoising loop (pipeline_interpolated_sd.py:1407-1963).
        ``is_fused`` / ``atype`` are accepted and ignored exactly like the reference (:1418-1419):
        behaviour is set by ``load_aid``.  ``image_embeds_start / _end``: (negative, positive) image-embedding pairs
        ``[1, 1, emb]`` in place of ``image_start`` / ``image_end`` PIL images (whose encoding is diffusers' job).
        ``use_graphs`` (build-specific; None = on a GPU): the three kinds of UNet pass of the loop are captured into
        hipGraphs at their first step and replayed afterwards (:class:`_PassGraphs`); results are bit-identical to eager.
        ``endpoints`` (build-specific): an :class:`EndpointStore`.  Empty, the run RECORDS the two end points into it (a normal run,
        bit-identical outputs); recorded under the same end points and settings, the run REPLAYS: only the frame at ``it`` goes
        through the UNet, its AID steps attend to the stored end-point keys / values, and the end points' outputs come from the
        stored latents — the return value has the usual three frames.  Anything else raises ``ValueError`` naming what differs.
        ``timesteps`` / ``sigmas``: a custom schedule handed to ``scheduler.set_timesteps`` (:111-154, :1716); the step count and the
        warm-up count ``int(T * warmup_ratio)`` then follow the table's length.  ``eta`` / ``generator`` reach ``scheduler.step`` where
        its signature takes them (:782-795); ``eta != 0`` with ``endpoints`` raises.  ``guidance_rescale`` > 0 (:1896-1902): the guided
        noise of every step is rescaled to the text pass's spread (arXiv 2305.08891 §3.4), in one launch with the guidance itself."""
        if image_start is not None and image_end is None:
            raise ValueError("Please provide both `image_start` and `image_end` to interpolate, or only `image_end` to "
                             "control the scale.")                                     # pipeline_interpolated_sd.py:1608-1612
        if (image_start is not None or image_end is not None) and self._encode_image is None:
            raise ValueError("image inputs need an `encode_image` component; pass image_embeds_start / image_embeds_end")
        if eta != 0.0 and endpoints is not None:
            raise ValueError("eta != 0 with an end-point store: a stochastic trajectory cannot be recorded once and replayed (run with "
                             "eta = 0, or without `endpoints`)")
        gr = _check_rescale(guidance_rescale)
        gs = self.default_guidance_scale if guidance_scale is None else guidance_scale
        self._guidance_scale, self._guidance_rescale = gs, gr
        dev, dtype = self._unet_device_dtype()
        cak = cross_attention_kwargs
        ls = cak.get("scale", None) if cak is not None else None
        cond_s, unc_s = self._split(self._embed(prompt_start, negative_prompt, embeds_start, ls))
        cond_e, unc_e = self._split(self._embed(prompt_end, negative_prompt, embeds_end, ls))
        guide = None
        if guide_prompt is not None or embeds_guide is not None:
            guide = self._split(self._embed(guide_prompt, negative_prompt, embeds_guide, ls))
        h = height or self._latent_hw()[0] * 8
        w = width or self._latent_hw()[1] * 8
        nc = getattr(self.unet, "in_channels", 4)
        latent_start = self.prepare_latents(1, nc, h // 8, w // 8, dtype, dev, generator, latent_start)
        latent_end = self.prepare_latents(1, nc, h // 8, w // 8, dtype, dev, generator, latent_end)
        batch = prepare_single(it, latent_start, latent_end, cond_s[0], cond_e[0], unc_s[0], unc_e[0],
                               None if guide is None else guide[0][0], None if guide is None else guide[1][0], init=init)
        pooled = self._pooled_single(cond_s, cond_e, unc_s, unc_e, guide, it, init)
        img = self._image_embeds_single(image_start, image_end, image_embeds_start, image_embeds_end, it, init, dev, dtype)
        _, num_inference_steps = _retrieve_timesteps(self.scheduler, num_inference_steps, dev, timesteps, sigmas)      # :1716
        extra_step_kwargs = _extra_step_kwargs(self.scheduler, eta, generator)         # :1750
        warmup_steps = int(num_inference_steps * warmup_ratio)                         # :1831
        lat = batch.latents
        cond, unc = batch.cond.to(dev, dtype), batch.uncond.to(dev, dtype)
        graphs = _PassGraphs(_use_graphs(use_graphs, dev))
        P.clear_weight_caches()              # caches derived from weights live for ONE run (in-place weight edits are invisible to their keys)
        ep_mode, n_run = None, 3
        if endpoints is not None:
            if img is not None:
                raise NotImplementedError("an end-point store with IP-Adapter image inputs: the store holds the text processors' "
                                          "self-attention keys / values only")
            early_mode, fusion = self._installed_aid_mode()
            sig = run_signature(latent_start=latent_start, latent_end=latent_end, embeds_start=cond_s[0], embeds_end=cond_e[0],
                                embeds_negative=[unc_s[0], unc_e[0]], embeds_pooled=self._pooled_inputs(cond_s, cond_e, unc_s, unc_e),
                                embeds_guide=[] if guide is None else [g_ for pair in guide for g_ in pair],
                                num_inference_steps=num_inference_steps, warmup_ratio=warmup_ratio, early=early_mode, late="self",
                                fusion=fusion, guidance_scale=gs, dtype=dtype, timesteps=self.scheduler.timesteps, unet=self.unet,
                                lora_scale=ls, guidance_rescale=gr)
            if endpoints.recorded:
                endpoints.begin_replay(sig, dev)
                ep_mode, n_run = "replay", 1
                ectx = torch.cat([cond[0:1], cond[2:3]]).contiguous()
                lat, cond, unc = lat[1:2], cond[1:2].contiguous(), unc[1:2].contiguous()
                if pooled is not None:
                    pooled = (pooled[0][1:2], pooled[1][1:2])
                set_endpoint_store(self.unet, endpoints, endpoint_ctx=ectx, coef=[it])
            else:
                endpoints.begin_record(sig, warmup_steps, dev)
                ep_mode = "record"
                set_endpoint_store(self.unet, endpoints)

        # loop-invariant conditioning, moved to the device once (the reference rebuilds the dict every step, :1850-1867)
        added_c = self._added_cond(None if pooled is None else pooled[0], n_run, None if img is None else img[0])
        added_u = self._added_cond(None if pooled is None else pooled[1], n_run, None if img is None else img[1])

        def cond_pass(x, t):
            return self._unet(x, t, cond, added_c, cak)

        def uncond_pass(x, t):
            return self._unet(x, t, unc, added_u, cak)

        try:
            for i, t in enumerate(self.scheduler.timesteps):
                x = self.scheduler.scale_model_input(lat, t)
                td = _dev_scalar(t, dev) if graphs.enabled else t
                if i < warmup_steps:                                                       # :1845-1848
                    if ep_mode == "replay":
                        set_aid_active(self.unet, True)        # the processors hold the interior coefficient alone (set above)
                    else:
                        self.activate_aid(it)
                    if ep_mode is not None:
                        endpoints.set_step(i)
                else:
                    self.deactivate_aid()
                key = ("cond", i < warmup_steps) if ep_mode is None else ("cond", i < warmup_steps, ep_mode)
                noise_text = graphs.run(key, cond_pass, x=x, t=td)
                self.deactivate_aid()                                                      # :1870
                noise_unc = graphs.run(("uncond",), uncond_pass, x=x, t=td)
                noise = _guided_noise(noise_text, noise_unc, gs, gr)                       # :1892-1902
                lat = self.scheduler.step(noise, t, lat, **extra_step_kwargs, return_dict=False)[0]        # :1905-1907
                if callback_on_step_end is not None:
                    out = callback_on_step_end(self, i, t, {"latents": lat}) or {}
                    lat = out.pop("latents", lat)
            if ep_mode == "record":
                endpoints.finish_record(torch.cat([lat[0:1], lat[2:3]]))
            elif ep_mode == "replay":
                lat = torch.cat([endpoints.latents[0:1], lat, endpoints.latents[1:2]], dim=0)
        finally:
            if ep_mode is not None:
                endpoints.abort()                # (no-op after finish_record; a failed recording leaves nothing behind)
                set_endpoint_store(self.unet, None)
        image = self._decode(lat, "latent" if output_type == "latent" else ("np" if output_type in ("pil", "np") else output_type))
        return {"images": image} if return_dict else (image, None)

    # -- N-frame interpolate (gradio) -------------------------------------------------------------------
    @torch.no_grad()
    def interpolate(self, latent_start: torch.Tensor, latent_end: torch.Tensor, prompt_start: Optional[str] = None,
                    prompt_end: Optional[str] = None, guide_prompt: Optional[str] = None, negative_prompt: str = "",
                    size: int = 7, num_inference_steps: int = 25, warmup_ratio: float = 0.5,
                    early: str = "fused_outer", late: str = "self", alpha: Optional[float] = None,
                    beta: Optional[float] = None, guidance_scale: Optional[float] = None,
                    # build-specific
                    embeds_start=None, embeds_end=None, embeds_guide=None, batched_cfg: bool = True,
                    output_type: str = "np", coef: Optional[Sequence[float]] = None, use_graphs: Optional[bool] = None,
                    cross_attention_kwargs: Optional[Dict[str, Any]] = None, endpoints: Optional[EndpointStore] = None,
                    guidance_rescale: float = 0.0, image_start=None, image_end=None, image_embeds_start=None,
                    image_embeds_end=None, init: str = "linear"):
        """gradio_src/pipeline_interpolated_stable_diffusion.py:163-304 with the root pipelines' warm-up count
        (``i < int(T * warmup_ratio)`` with 0-based ``i``).  ``late`` must be "self" (plain
        attention) or one of the AID modes.  ``batched_cfg``: the two passes of a step run as one UNet call.
        ``coef`` (build-specific, ``[0, t_1, ..., 1]``): render the frames at THESE coefficients the way
        ``interpolate_single(t_k)`` would — latents slerp'd and embeddings lerp'd at ``t_k``, attention coefficient
        ``t_k`` — in one N-frame run (the Beta-prior exploration fills several gaps per run with it, prior.py).
        ``use_graphs``, ``cross_attention_kwargs`` and ``endpoints`` as in ``interpolate_single`` (a replay renders the ``size - 2``
        interior frames; a store recorded by either method replays in the other); ``guidance_rescale`` (build-specific here) as in
        ``interpolate_single``.  The processors ``load_aid`` / ``load_aid_ip_adapter`` installed are put
        back when the run ends (the run works with its own N-frame processors).
        ``image_start`` / ``image_end`` / ``image_embeds_start`` / ``image_embeds_end`` / ``init`` (build-specific here) as in
        ``interpolate_single``, for a UNet whose IP-Adapter is loaded: frame k attends with ``mix(start, end, t_k)`` of the positive
        (conditional pass) and of the negative (unconditional pass) image embeddings, ``t_k`` its coefficient and ``mix`` ``torch.lerp``
        for ``init == "linear"``, else ``slerp``; only ``image_end`` = scale control.  The adapter layers then run the IP processor
        ``early`` / ``late`` name (``install_sequence_processors(ip_adapter=)``), every other layer the text processors.  With several
        adapters, ``ip_adapter_masks`` or a foreign processor kept by ``load_aid_ip_adapter(keep_original=True)`` the two passes of a step
        run as two UNet calls whatever ``batched_cfg`` says.  ``endpoints`` with images raises."""
        if early not in EARLY_MODES or (late != "self" and late not in EARLY_MODES):
            raise ValueError(f"early / late must be in {EARLY_MODES} (late also 'self')")
        if (image_start is not None and image_end is None) or \
                (image_embeds_start is not None and image_end is None and image_embeds_end is None):   # pipeline_interpolated_sd.py:1608-1612
            raise ValueError("Please provide both `image_start` and `image_end` to interpolate, or only `image_end` to "
                             "control the scale.")
        if (image_start is not None or image_end is not None) and self._encode_image is None:
            raise ValueError("image inputs need an `encode_image` component; pass image_embeds_start / image_embeds_end")
        with_images = image_end is not None or image_embeds_end is not None
        if with_images and endpoints is not None:
            raise NotImplementedError("an end-point store with IP-Adapter image inputs: the store holds the text processors' "
                                      "self-attention keys / values only")
        gs = self.default_guidance_scale if guidance_scale is None else guidance_scale
        gr = _check_rescale(guidance_rescale)
        dev, dtype = self._unet_device_dtype()
        cak = cross_attention_kwargs
        ls = cak.get("scale", None) if cak is not None else None
        cond_s, unc_s = self._split(self._embed(prompt_start, negative_prompt, embeds_start, ls))
        cond_e, unc_e = self._split(self._embed(prompt_end, negative_prompt, embeds_end, ls))
        guide = None
        if guide_prompt is not None or embeds_guide is not None:
            guide = self._split(self._embed(guide_prompt, negative_prompt, embeds_guide, ls))
        batch = prepare_sequence(latent_start.to(dev, dtype), latent_end.to(dev, dtype), cond_s[0], cond_e[0], unc_s[0],
                                 unc_e[0], size=size, guide_emb=None if guide is None else guide[0][0],
                                 uncond_guide=None if guide is None else guide[1][0],
                                 num_inference_steps=num_inference_steps, alpha=alpha, beta=beta)
        pooled = self._pooled_sequence(cond_s, cond_e, unc_s, unc_e, guide, size)
        if coef is not None:
            ts = [float(t) for t in coef]
            if len(ts) != size or ts[0] != 0.0 or ts[-1] != 1.0:
                raise ValueError("coef must be [0, ..., 1] with `size` entries")
            l0, l1 = latent_start.to(dev, dtype), latent_end.to(dev, dtype)
            batch.latents = torch.cat([l0] + [slerp(l0, l1, t) for t in ts[1:-1]] + [l1], dim=0)
            batch.coef = torch.tensor(ts, dtype=torch.float32)
            if guide is None:
                batch.cond = linear_interpolation(cond_s[0], cond_e[0], ts=ts)
                batch.uncond = linear_interpolation(unc_s[0], unc_e[0], ts=ts)
                if pooled is not None:
                    pooled = (linear_interpolation(cond_s[1], cond_e[1], ts=ts), linear_interpolation(unc_s[1], unc_e[1], ts=ts))
        img = self._image_embeds_sequence(image_start, image_end, image_embeds_start, image_embeds_end, batch.coef, init, dev, dtype) \
            if with_images else None
        ip_variant = None if img is None else \
            ("interpolate" if image_start is not None or image_embeds_start is not None else "scale_control")
        self.scheduler.set_timesteps(num_inference_steps, device=dev)
        warmup_steps = int(num_inference_steps * warmup_ratio)
        installed = dict(self.unet.attn_processors)          # what load_aid / load_aid_ip_adapter put there: restored at the end
        ep_mode, full_size = None, size
        if endpoints is not None:
            if size < 3:
                raise ValueError("an end-point store needs at least one interior frame (size >= 3)")
            sig = run_signature(latent_start=latent_start.to(dev, dtype), latent_end=latent_end.to(dev, dtype), embeds_start=cond_s[0],
                                embeds_end=cond_e[0], embeds_negative=[unc_s[0], unc_e[0]],
                                embeds_pooled=self._pooled_inputs(cond_s, cond_e, unc_s, unc_e),
                                embeds_guide=[] if guide is None else [g_ for pair in guide for g_ in pair],
                                num_inference_steps=num_inference_steps, warmup_ratio=warmup_ratio,
                                early=early.split("_")[1], late=late, fusion=early.startswith("fused"), guidance_scale=gs, dtype=dtype,
                                timesteps=self.scheduler.timesteps, unet=self.unet, lora_scale=ls, guidance_rescale=gr)
            if endpoints.recorded:
                endpoints.begin_replay(sig, dev)
                ep_mode = "replay"
            else:
                endpoints.begin_record(sig, warmup_steps if late == "self" else num_inference_steps, dev)
                ep_mode = "record"
        try:
            cond, unc = batch.cond.to(dev, dtype), batch.uncond.to(dev, dtype)
            idx = [int(i) for i in batch.ctx_index.tolist()] if batch.n_distinct_ctx != size else None
            lat = batch.latents
            n_distinct = batch.n_distinct_ctx
            run_coef, ectx = batch.coef, None
            if ep_mode == "replay":          # the batch holds the interior frames only; the end points' text contexts ride behind theirs
                ectx = torch.cat([cond[0:1], cond[-1:]]).contiguous()
                lat, cond, unc = lat[1:-1], cond[1:-1].contiguous(), unc[1:-1].contiguous()
                run_coef = batch.coef[1:-1]
                if pooled is not None:
                    pooled = (pooled[0][1:-1], pooled[1][1:-1])
                if idx is not None:          # guide prompt: the interior frames share ONE context
                    idx, n_distinct = [j - 1 for j in idx[1:-1]], n_distinct - 2
                size = size - 2
            procs = {}
            for mode in {early} | ({late} - {"self"}):
                install_sequence_processors(self.unet, size, early=mode, alpha=alpha, beta=beta,
                                            num_inference_steps=num_inference_steps, coef=run_coef, ip_adapter=ip_variant)
                if isinstance(endpoints, KeyframePair):      # (interpolate_between: the pair's two frames of a KeyframeStore)
                    set_keyframe_store(self.unet, endpoints.store, between=(endpoints.a, endpoints.b), endpoint_ctx=ectx)
                elif ep_mode is not None:
                    set_endpoint_store(self.unet, endpoints, endpoint_ctx=ectx)
                procs[mode] = dict(self.unet.attn_processors)
            if img is not None and batched_cfg:
                # riders stand for the de-activated pass of ONE unmasked adapter on the package's own processor; elsewhere (several
                # adapters, ip_adapter_masks, a kept foreign processor) the two passes run as two UNet calls — the same result
                masks = None if cak is None else cak.get("ip_adapter_masks")
                batched_cfg = all(p_.riders_supported(masks) for ps in procs.values() for p_ in ps.values()
                                  if isinstance(p_, P._IPBase))
            graphs = _PassGraphs(_use_graphs(use_graphs, dev))
            ctx_both = torch.cat([cond, unc]) if batched_cfg else None      # ONE tensor for the whole run: the text K / V cache keys on it
            if batched_cfg:
                added_both = self._added_cond(None if pooled is None else torch.cat(pooled), 2 * size) if img is None else \
                    self._added_cond(None if pooled is None else torch.cat(pooled), 2 * size,
                                     [torch.cat([p_, n_]) for p_, n_ in zip(*img)])      # image rows [cond frames ; uncond frames]
            elif img is None:
                added_c = self._added_cond(None if pooled is None else pooled[0], size)
                added_u = self._added_cond(None if pooled is None else pooled[1], size)
            else:
                added_c = self._added_cond(None if pooled is None else pooled[0], size, img[0])
                added_u = self._added_cond(None if pooled is None else pooled[1], size, img[1])

            def both_pass(x, t):
                return self._unet(torch.cat([x, x]), t, ctx_both, added_both, cak)

            def cond_pass(x, t):
                return self._unet(x, t, cond, added_c, cak)

            def uncond_pass(x, t):
                return self._unet(x, t, unc, added_u, cak)

            for i, t in enumerate(self.scheduler.timesteps):
                x = self.scheduler.scale_model_input(lat, t)
                td = _dev_scalar(t, dev) if graphs.enabled else t
                mode = early if i < warmup_steps else late
                self.unet.set_attn_processor(procs[mode] if mode != "self" else procs[early])
                if ep_mode is not None and mode != "self":
                    endpoints.set_step(i)
                gkey = (mode,) if ep_mode is None else (mode, ep_mode)
                if batched_cfg:
                    # (the IP processors that compute de-activated themselves — scale control — need to know their riders there too)
                    set_aid_active(self.unet, mode != "self", plain_tail=size if mode != "self" or img is not None else 0)
                    set_ctx_index(self.unet, None if idx is None else idx + [j + n_distinct for j in idx])
                    both = graphs.run(("both",) + gkey, both_pass, x=x, t=td)
                    noise_text, noise_unc = both[:size], both[size:]
                else:
                    set_ctx_index(self.unet, idx)
                    set_aid_active(self.unet, mode != "self")
                    noise_text = graphs.run(("cond",) + gkey, cond_pass, x=x, t=td)
                    set_aid_active(self.unet, False)
                    noise_unc = graphs.run(("uncond",) + gkey, uncond_pass, x=x, t=td)
                noise = _guided_noise(noise_text, noise_unc, gs, gr)
                lat = self.scheduler.step(noise, t, lat, return_dict=False)[0]
            if ep_mode == "record":
                endpoints.finish_record(torch.cat([lat[0:1], lat[-1:]]))
            elif ep_mode == "replay":
                lat = torch.cat([endpoints.latents[0:1], lat, endpoints.latents[1:2]], dim=0)
        finally:
            if ep_mode is not None:
                endpoints.abort()                # (no-op after finish_record; a failed recording leaves nothing behind)
            set_ctx_index(self.unet, None)
            self.unet.set_attn_processor(installed)
        return self._decode(lat, output_type)

    # -- interpolate_save_gpu (gradio): the sequence bayesian_prior_selection scores ---------------------------------------------
    @torch.no_grad()
    def interpolate_save_gpu(self, latent_start: torch.Tensor, latent_end: torch.Tensor, prompt_start: Optional[str] = None,
                             prompt_end: Optional[str] = None, guide_prompt: Optional[str] = None, negative_prompt: str = "",
                             size: int = 7, num_inference_steps: int = 25, warmup_ratio: float = 0.5,
                             early: str = "fused_outer", late: str = "self", alpha: Optional[float] = None,
                             beta: Optional[float] = None, init: str = "linear", guidance_scale: Optional[float] = None,
                             # build-specific
                             endpoints: Optional[EndpointStore] = None, **kwargs):
        """gradio_src/pipeline_interpolated_stable_diffusion.py:307-392: ``size`` frames at the coefficients
        ``generate_beta_tensor(size, alpha, beta)`` (both default to ``num_inference_steps``), each interior frame rendered the way
        ``interpolate_single(t_k)`` renders it.  The reference makes ``size - 2`` batch-3 runs, each denoising the two end points
        again; here it is ONE ``interpolate(coef=[0, *t, 1])`` run — and with a recorded ``endpoints`` store a replay of the interior
        frames alone.  Returns what ``interpolate`` returns (a numpy array of ``size`` frames for the default ``output_type``);
        ``kwargs`` are ``interpolate``'s build-specific ones (``embeds_start``, ``output_type``, ``use_graphs``, ...).
        ``init="denoising"`` (the reference's ``denoising_interpolate`` baseline) and the spherical embedding mix raise
        ``NotImplementedError``."""
        if init == "denoising":
            raise NotImplementedError('init="denoising": the reference\'s denoising_interpolate baseline is not part of this package')
        if init != "linear":
            raise NotImplementedError(f"init={init!r}: the N-frame run mixes the text embeddings linearly (init=\"linear\")")
        if alpha is None:
            alpha = num_inference_steps
        if beta is None:
            beta = num_inference_steps
        coef = [float(t) for t in generate_beta_tensor(size, alpha=alpha, beta=beta)]
        coef[0], coef[-1] = 0.0, 1.0
        return self.interpolate(latent_start, latent_end, prompt_start, prompt_end, guide_prompt=guide_prompt,
                                negative_prompt=negative_prompt, size=size, num_inference_steps=num_inference_steps,
                                warmup_ratio=warmup_ratio, early=early, late=late, guidance_scale=guidance_scale, coef=coef,
                                endpoints=endpoints, **kwargs)

    # -- corner-weighted interpolation among up to eight end points ----------------------
    @torch.no_grad()
    def interpolate_corners(self, latents, prompts: Optional[Sequence[str]] = None, weights=None,
                            embeds: Optional[Sequence[tuple]] = None, guide_prompt: Optional[str] = None, embeds_guide=None,
                            negative_prompt: Optional[str] = None, early: str = "fused_outer", late: str = "self",
                            warmup_ratio: float = 0.5, num_inference_steps: int = 50, timesteps: Optional[List[int]] = None,
                            sigmas: Optional[List[float]] = None, eta: float = 0.0, guidance_scale: Optional[float] = None,
                            guidance_rescale: float = 0.0, generator=None, frame_latents: Optional[torch.Tensor] = None,
                            use_graphs: Optional[bool] = None, output_type: str = "pil", **image_inputs):
        """Build-specific: N frames interpolated among M <= 8 end points ("corners") in one run — a 2 x 2 morph grid between four
        prompts or seeds (``grid_weights``), a prompt with three components (``simplex_weights``).  ``latents`` [M, C, h, w] (or M
        tensors [1, C, h, w]) and ``prompts`` / ``embeds`` (one per corner, as ``interpolate`` takes ``prompt_start`` /
        ``embeds_start``) describe the corners; ``weights`` [N, M] the frames: rows non-negative, summing to 1 within 1e-6, and for
        every corner a frame whose row is exactly one-hot — that frame IS the corner (``corner_rows[m]``, the first such frame), the
        corner frames sit in the batch as the two end points of ``interpolate`` do.  Anything else raises ``ValueError`` naming the row.
        Frame latents: ``nested_slerp`` of the corner latents in corner order (``slerp(x_0, x_1, c)`` for M = 2), or ``frame_latents``
        [N, C, h, w].  Conditional, negative (and SDXL pooled) embeddings of a frame: the weight-mixed corner embeddings; with a guide
        prompt every frame that is not a corner takes the guide's, shared through ``ctx_index`` as in ``interpolate``.  The two
        passes of a step run as one UNet call ``[cond N ; uncond N]``, the second half as plain riders.  ``early`` / ``late`` /
        ``warmup_ratio`` / ``timesteps`` / ``sigmas`` / ``eta`` / ``generator`` / ``guidance_rescale`` / ``use_graphs`` as in
        ``interpolate_single`` and ``interpolate``.  IP-Adapter image inputs raise ``NotImplementedError``."""
        for name in image_inputs:
            if name in ("image_start", "image_end", "image_embeds_start", "image_embeds_end", "images", "image_embeds",
                        "ip_adapter_image", "ip_adapter_image_embeds"):
                raise NotImplementedError(f"interpolate_corners takes no image inputs ({name}): the IP-Adapter image branches "
                                          "interpolate between two end points only")
            raise TypeError(f"interpolate_corners() got an unexpected keyword argument {name!r}")
        if early not in EARLY_MODES or (late != "self" and late not in EARLY_MODES):
            raise ValueError(f"early / late must be in {EARLY_MODES} (late also 'self')")
        lats = [latents[i:i + 1] for i in range(latents.shape[0])] if torch.is_tensor(latents) else list(latents)
        m = len(lats)
        w, corner_rows = corner_rows_of(weights, m)
        n = w.shape[0]
        for what, seq in (("prompts", prompts), ("embeds", embeds)):
            if seq is not None and len(seq) != m:
                raise ValueError(f"interpolate_corners needs one entry of {what} per corner: {len(seq)} for {m} corners")
        gs = self.default_guidance_scale if guidance_scale is None else guidance_scale
        gr = _check_rescale(guidance_rescale)
        self._guidance_scale, self._guidance_rescale = gs, gr
        dev, dtype = self._unet_device_dtype()
        sides = [self._split(self._embed(None if prompts is None else prompts[i], negative_prompt,
                                         None if embeds is None else embeds[i])) for i in range(m)]
        guide = None
        if guide_prompt is not None or embeds_guide is not None:
            guide = self._split(self._embed(guide_prompt, negative_prompt, embeds_guide))
        onehot = [int(torch.nonzero(w[i] == 1.0)[0]) if bool((w[i] == 1.0).any()) and int((w[i] != 0).sum()) == 1 else None
                  for i in range(n)]

        def mixed(slot: int, side: int):
            """[N, ...]: corner tensors ``sides[.][side][slot]`` mixed with the weight rows (a one-hot row takes its corner's bits)."""
            src = [sides[c][side][slot] for c in range(m)]
            acc = torch.float64 if src[0].dtype == torch.float64 else torch.float32
            stack = torch.cat([t_.to(acc) for t_ in src], dim=0)
            rows = []
            for i in range(n):
                if onehot[i] is not None:
                    rows.append(src[onehot[i]])
                else:
                    rows.append(torch.tensordot(w[i].to(stack.device, acc), stack, dims=1).unsqueeze(0).to(src[0].dtype))
            return torch.cat(rows, dim=0)

        idx = None
        if guide is not None and any(o is None for o in onehot):
            # one context row per frame, as interpolate hands them over; ctx_index names the distinct ones — the M corners', then the
            # guide's, which every frame that is not a corner shares (its keys / values are projected once)
            cond = torch.cat([guide[0][0] if o is None else sides[o][0][0] for o in onehot], dim=0)
            unc = torch.cat([guide[1][0] if o is None else sides[o][1][0] for o in onehot], dim=0)
            idx = [m if o is None else o for o in onehot]
            pooled = None
            if len(sides[0][0]) > 1:
                pooled = tuple(torch.cat([(guide[s_][1] if o is None else sides[o][s_][1]) for o in onehot], dim=0) for s_ in (0, 1))
        else:
            cond, unc = mixed(0, 0), mixed(0, 1)
            pooled = (mixed(1, 0), mixed(1, 1)) if len(sides[0][0]) > 1 else None
        n_distinct = m + 1
        cond, unc = cond.to(dev, dtype), unc.to(dev, dtype)
        if frame_latents is not None:
            if tuple(frame_latents.shape) != (n,) + tuple(lats[0].shape[1:]):
                raise ValueError(f"frame_latents must be [{n}, ...] like the corner latents; got {tuple(frame_latents.shape)}")
            lat = frame_latents.to(dev, dtype)
        else:
            cl = [l_.to(dev, dtype) for l_ in lats]
            lat = torch.cat([nested_slerp(cl, w[i]) for i in range(n)], dim=0)
        _, num_inference_steps = _retrieve_timesteps(self.scheduler, num_inference_steps, dev, timesteps, sigmas)
        extra_step_kwargs = _extra_step_kwargs(self.scheduler, eta, generator)
        warmup_steps = int(num_inference_steps * warmup_ratio)
        installed = dict(self.unet.attn_processors)
        try:
            procs = {}
            for mode in {early} | ({late} - {"self"}):
                install_corner_processors(self.unet, w, corner_rows, early=mode)
                procs[mode] = dict(self.unet.attn_processors)
            graphs = _PassGraphs(_use_graphs(use_graphs, dev))
            ctx_both = torch.cat([cond, unc])               # ONE tensor for the whole run: the text K / V cache keys on it
            added_both = self._added_cond(None if pooled is None else torch.cat(pooled), 2 * n)
            idx_both = None if idx is None else idx + [j + n_distinct for j in idx]

            def both_pass(x, t):
                return self._unet(torch.cat([x, x]), t, ctx_both, added_both)

            for i, t in enumerate(self.scheduler.timesteps):
                x = self.scheduler.scale_model_input(lat, t)
                td = _dev_scalar(t, dev) if graphs.enabled else t
                mode = early if i < warmup_steps else late
                self.unet.set_attn_processor(procs[mode] if mode != "self" else procs[early])
                set_aid_active(self.unet, mode != "self", plain_tail=n if mode != "self" else 0)
                set_ctx_index(self.unet, idx_both)
                both = graphs.run(("both", mode), both_pass, x=x, t=td)
                noise = _guided_noise(both[:n], both[n:], gs, gr)
                lat = self.scheduler.step(noise, t, lat, **extra_step_kwargs, return_dict=False)[0]
        finally:
            set_ctx_index(self.unet, None)
            self.unet.set_attn_processor(installed)
        return self._decode(lat, "latent" if output_type == "latent" else ("np" if output_type in ("pil", "np") else output_type))

    # -- key frames: record once, render between any two --------------------------------
    @torch.no_grad()
    def record_keyframes(self, store: KeyframeStore, names: Sequence[str], latents, prompts: Optional[Sequence[str]] = None,
                         embeds: Optional[Sequence[tuple]] = None, negative_prompt: str = "", num_inference_steps: int = 25,
                         warmup_ratio: float = 0.5, aid_steps: Optional[int] = None, guidance_scale: Optional[float] = None,
                         use_graphs: Optional[bool] = None, cross_attention_kwargs: Optional[Dict[str, Any]] = None,
                         output_type: str = "np", guidance_rescale: float = 0.0):
        """Denoise the K key frames ``names`` as ONE plain classifier-free-guidance batch (``latents`` [K, C, h, w] or K tensors
        [1, C, h, w]; ``prompts`` or ``embeds``, one per frame, as ``interpolate`` takes ``prompt_start`` / ``embeds_start``) and record
        them into ``store``: at every self-attention layer of the conditional pass of the first ``aid_steps`` steps (default
        ``int(num_inference_steps * warmup_ratio)``; pass ``num_inference_steps`` to allow ``late`` AID modes) each frame's k / V^T
        goes into its own store — one PUT launch beside the projections — and each frame's inputs and final latent are kept.  That is
        everything ``interpolate_between`` needs of a frame, whichever partner, direction or early mode it is rendered with.  A
        name the store already holds raises; further frames may be recorded later under the same settings.  More than 8 frames
        (``AID_KF_MAX_ROWS``, what one launch moves) are recorded in runs of up to 8.  ``guidance_rescale`` as in ``interpolate_single``: it
        is part of what the frames are recorded under (a replay under another value raises).  Returns the decoded key frames."""
        names = [str(n) for n in names]
        k = len(names)
        lats = [latents[i:i + 1] for i in range(k)] if torch.is_tensor(latents) else list(latents)
        for what, seq in (("latents", lats), ("prompts", prompts), ("embeds", embeds)):
            if seq is not None and len(seq) != k:
                raise ValueError(f"record_keyframes needs one entry of {what} per name: {len(seq)} for {k} names")
        if len(set(names)) != k:
            raise ValueError(f"record_keyframes needs distinct names, one per frame; got {names}")
        for n in names:
            if n in store:
                raise ValueError(f"key frame {n!r} is already recorded: remove({n!r}) it first")
        if k > KF_MAX_ROWS:
            outs = []
            for g0 in range(0, k, KF_MAX_ROWS):
                sl = slice(g0, g0 + KF_MAX_ROWS)
                outs.append(self.record_keyframes(store, names[sl], lats[sl], None if prompts is None else prompts[sl],
                                                  None if embeds is None else embeds[sl], negative_prompt, num_inference_steps,
                                                  warmup_ratio, aid_steps, guidance_scale, use_graphs, cross_attention_kwargs, output_type,
                                                  guidance_rescale=guidance_rescale))
            return torch.cat(outs) if torch.is_tensor(outs[0]) else np.concatenate(outs)
        gs = self.default_guidance_scale if guidance_scale is None else guidance_scale
        gr = _check_rescale(guidance_rescale)
        dev, dtype = self._unet_device_dtype()
        cak = cross_attention_kwargs
        ls = cak.get("scale", None) if cak is not None else None
        embs = [self._embed(None if prompts is None else prompts[i], negative_prompt, None if embeds is None else embeds[i], ls)
                for i in range(k)]
        sides = [self._split(e) for e in embs]
        cond = torch.cat([s_[0][0] for s_ in sides]).to(dev, dtype).contiguous()
        unc = torch.cat([s_[1][0] for s_ in sides]).to(dev, dtype).contiguous()
        pooled = (torch.cat([s_[0][1] for s_ in sides]), torch.cat([s_[1][1] for s_ in sides])) if len(sides[0][0]) > 1 else None
        lat0 = torch.cat([l_.to(dev, dtype) for l_ in lats])
        self.scheduler.set_timesteps(num_inference_steps, device=dev)
        n_aid = int(num_inference_steps * warmup_ratio) if aid_steps is None else int(aid_steps)
        if not 1 <= n_aid <= num_inference_steps:
            raise ValueError(f"aid_steps must be in 1 .. num_inference_steps ({num_inference_steps}); got {n_aid}")
        settings = run_settings(num_inference_steps=num_inference_steps, guidance_scale=gs, dtype=dtype,
                                timesteps=self.scheduler.timesteps, unet=self.unet, lora_scale=ls, guidance_rescale=gr)
        installed = dict(self.unet.attn_processors)          # restored at the end, as interpolate does
        store.begin_record(names, settings, n_aid, dev)
        try:
            # plain attention through the AID processors' own plain path (no wrapped original): the call that takes the store
            P.clear_weight_caches()
            procs = {}
            for name in installed:
                procs[name] = P.OuterInterpolatedAttnProcessor(size=2, original_attn=None)
                procs[name].activated = False
            self.unet.set_attn_processor(procs)
            set_ctx_index(self.unet, None)
            graphs = _PassGraphs(_use_graphs(use_graphs, dev))
            added_c = self._added_cond(None if pooled is None else pooled[0], k)
            added_u = self._added_cond(None if pooled is None else pooled[1], k)

            def cond_pass(x, t):
                return self._unet(x, t, cond, added_c, cak)

            def uncond_pass(x, t):
                return self._unet(x, t, unc, added_u, cak)

            lat = lat0
            for i, t in enumerate(self.scheduler.timesteps):
                x = self.scheduler.scale_model_input(lat, t)
                td = _dev_scalar(t, dev) if graphs.enabled else t
                rec = i < n_aid
                if rec:                                       # the conditional pass of an AID step is what a later pair attends to
                    set_keyframe_store(self.unet, store, record=names)
                    store.set_step(i)
                noise_text = graphs.run(("cond", rec), cond_pass, x=x, t=td)
                set_keyframe_store(self.unet, None)
                noise_unc = graphs.run(("uncond",), uncond_pass, x=x, t=td)
                noise = _guided_noise(noise_text, noise_unc, gs, gr)
                lat = self.scheduler.step(noise, t, lat, return_dict=False)[0]
            store.finish_record(lat0, embs, lat)
        finally:
            store.abort()                        # (no-op after finish_record; a failed recording leaves nothing of itself behind)
            set_ctx_index(self.unet, None)
            self.unet.set_attn_processor(installed)
        return self._decode(lat, output_type)

    def interpolate_between(self, store: KeyframeStore, a: str, b: str, size: int = 7, coef: Optional[Sequence[float]] = None,
                            guide_prompt: Optional[str] = None, embeds_guide=None, negative_prompt: str = "",
                            early: str = "fused_outer", late: str = "self", warmup_ratio: float = 0.5,
                            alpha: Optional[float] = None, beta: Optional[float] = None, batched_cfg: bool = True,
                            output_type: str = "np", use_graphs: Optional[bool] = None,
                            num_inference_steps: Optional[int] = None, guidance_scale: Optional[float] = None,
                            cross_attention_kwargs: Optional[Dict[str, Any]] = None, guidance_rescale: float = 0.0):
        """Render ``size`` frames from key frame ``a`` to key frame ``b`` of ``store``: the ``size - 2`` interior frames go through the
        UNet exactly as in an ``interpolate(..., endpoints=<recorded store>)`` replay — latents and embeddings of the two frames come
        from the store, their AID steps attend to the frames' recorded keys / values — and the two end frames are the stored final
        latents.  ``(b, a)`` renders the reverse direction from the same recordings; any ``early`` mode does.  ``num_inference_steps``
        / ``guidance_scale`` default to the store's; ``guidance_rescale`` must be the recording's (a store recorded under a non-zero
        rescale keeps the pair ``(guidance_scale, guidance_rescale)`` in its ``guidance_scale`` setting).  An unknown name raises ``KeyError``; a run that needs more AID steps than were
        recorded, or whose step count, guidance scale, dtype, timesteps, UNet or LoRA state differ from the recording's, raises
        ``ValueError`` naming what differs."""
        fa, fb = store[a], store[b]
        pair = store.between(a, b)
        steps = store.settings["num_inference_steps"] if num_inference_steps is None else num_inference_steps
        if guidance_scale is None:
            gs = store.settings["guidance_scale"]
            gs = gs[0] if isinstance(gs, tuple) else gs
        else:
            gs = guidance_scale
        return self.interpolate(fa.latent, fb.latent, guide_prompt=guide_prompt, negative_prompt=negative_prompt, size=size,
                                num_inference_steps=steps, warmup_ratio=warmup_ratio, early=early, late=late, alpha=alpha, beta=beta,
                                guidance_scale=gs, embeds_start=fa.embeds, embeds_end=fb.embeds, embeds_guide=embeds_guide,
                                batched_cfg=batched_cfg, output_type=output_type, coef=coef, use_graphs=use_graphs,
                                cross_attention_kwargs=cross_attention_kwargs, endpoints=pair, guidance_rescale=guidance_rescale)

    def interpolate_chain(self, store: KeyframeStore, names: Sequence[str], size: int = 7, **kwargs):
        """``interpolate_between`` for every consecutive pair of ``names``, in order, joined with each shared key frame once:
        ``(K - 1) (size - 1) + 1`` frames for K names.  ``kwargs`` are ``interpolate_between``'s."""
        names = list(names)
        if len(names) < 2:
            raise ValueError("a chain needs at least two key frames")
        for n in names:
            store[n]
        parts = [self.interpolate_between(store, names[i], names[i + 1], size=size, **kwargs) for i in range(len(names) - 1)]
        parts = parts[:1] + [p_[1:] for p_ in parts[1:]]
        return torch.cat(parts) if torch.is_tensor(parts[0]) else np.concatenate(parts)

    # -- key frames: render frames blended among up to eight of them -------------------
    @torch.no_grad()
    def interpolate_among(self, store: KeyframeStore, names: Sequence[str], weights, guide_prompt: Optional[str] = None,
                          embeds_guide=None, negative_prompt: str = "", early: str = "fused_outer", late: str = "self",
                          warmup_ratio: float = 0.5, frame_latents: Optional[torch.Tensor] = None, max_frames: Optional[int] = None,
                          num_inference_steps: Optional[int] = None, guidance_scale: Optional[float] = None,
                          guidance_rescale: float = 0.0, use_graphs: Optional[bool] = None,
                          cross_attention_kwargs: Optional[Dict[str, Any]] = None, output_type: str = "np", **image_inputs):
        """Render N frames blended among the M <= 8 recorded key frames ``names`` of ``store`` — ``interpolate_corners`` whose corners
        are recorded: only the frames that are not a key frame go through the UNet, their AID steps attend to the key frames' recorded
        keys / values.  ``weights`` [N, M] (columns in the order of ``names``): rows non-negative, summing to 1 within 1e-6, anything
        else raises ``ValueError`` naming the row (``grid_weights`` / ``simplex_weights`` give such rows).  A frame whose row is exactly
        one-hot IS that key frame: its output is the stored final latent and it is not rendered.  Every other frame starts from the
        ``nested_slerp`` of the key frames' stored initial latents (or its row of ``frame_latents`` [N, C, h, w]) with the weight-mixed
        key-frame embeddings, exactly as ``interpolate_corners`` mixes them; with a guide prompt every rendered frame shares the
        guide's context.  One UNet call ``[cond n ; uncond n]`` per step over the rendered frames only, the second half as plain
        riders; ``max_frames`` renders them in runs of at most that many, joined in weight-row order.  ``num_inference_steps`` /
        ``guidance_scale`` default to the store's; settings that differ from the recording's, or a run that needs more AID steps than
        were recorded, raise ``ValueError`` as ``interpolate_between`` does.  IP-Adapter image inputs raise ``NotImplementedError``."""
        for name in image_inputs:
            if name in ("image_start", "image_end", "image_embeds_start", "image_embeds_end", "images", "image_embeds",
                        "ip_adapter_image", "ip_adapter_image_embeds"):
                raise NotImplementedError(f"interpolate_among takes no image inputs ({name}): the IP-Adapter image branches "
                                          "interpolate between two end points only")
            raise TypeError(f"interpolate_among() got an unexpected keyword argument {name!r}")
        if early not in EARLY_MODES or (late != "self" and late not in EARLY_MODES):
            raise ValueError(f"early / late must be in {EARLY_MODES} (late also 'self')")
        blend = store.among(names)
        m = len(blend.names)
        w = weight_rows_of(weights, m)
        n_all = w.shape[0]
        if max_frames is not None and int(max_frames) < 1:
            raise ValueError(f"max_frames must be None or >= 1; got {max_frames}")
        frames = [store[n_] for n_ in blend.names]
        onehot = [int(torch.nonzero(w[i] == 1.0)[0]) if bool((w[i] == 1.0).any()) and int((w[i] != 0).sum()) == 1 else None
                  for i in range(n_all)]
        render = [i for i in range(n_all) if onehot[i] is None]
        if frame_latents is not None and tuple(frame_latents.shape) != (n_all,) + tuple(frames[0].latent.shape[1:]):
            raise ValueError(f"frame_latents must be [{n_all}, ...] like the key frames' latents; got {tuple(frame_latents.shape)}")
        steps = store.settings["num_inference_steps"] if num_inference_steps is None else num_inference_steps
        if guidance_scale is None:
            gs = store.settings["guidance_scale"]
            gs = gs[0] if isinstance(gs, tuple) else gs
        else:
            gs = guidance_scale
        gr = _check_rescale(guidance_rescale)
        self._guidance_scale, self._guidance_rescale = gs, gr
        dev, dtype = self._unet_device_dtype()
        cak = cross_attention_kwargs
        ls = cak.get("scale", None) if cak is not None else None
        sides = [self._split(self._embed(None, negative_prompt, f_.embeds, ls)) for f_ in frames]
        guide = None
        if guide_prompt is not None or embeds_guide is not None:
            guide = self._split(self._embed(guide_prompt, negative_prompt, embeds_guide, ls))
        self.scheduler.set_timesteps(steps, device=dev)
        warmup_steps = int(steps * warmup_ratio)
        sig = dict(run_settings(num_inference_steps=steps, guidance_scale=gs, dtype=dtype, timesteps=self.scheduler.timesteps,
                                unet=self.unet, lora_scale=ls, guidance_rescale=gr), warmup_ratio=float(warmup_ratio), late=late)
        corner_ctx = torch.cat([s_[0][0] for s_ in sides]).to(dev, dtype).contiguous()
        cl = [f_.latent.to(dev, dtype) for f_ in frames]

        def mixed(rows, slot: int, side: int):
            """[n, ...]: key-frame tensors ``sides[.][side][slot]`` mixed with the weight rows ``rows`` (none of them one-hot)."""
            src = [sides[c][side][slot] for c in range(m)]
            acc = torch.float64 if src[0].dtype == torch.float64 else torch.float32
            stack = torch.cat([t_.to(acc) for t_ in src], dim=0)
            return torch.cat([torch.tensordot(w[i].to(stack.device, acc), stack, dims=1).unsqueeze(0).to(src[0].dtype) for i in rows])

        out = [None] * n_all
        finals = blend.latents
        for i in range(n_all):
            if onehot[i] is not None:
                out[i] = finals[onehot[i]:onehot[i] + 1].to(dev, dtype)
        group = len(render) if max_frames is None else int(max_frames)
        installed = dict(self.unet.attn_processors)          # restored at the end, as interpolate does
        for g0 in range(0, len(render), max(group, 1)):
            rows = render[g0:g0 + group]
            n = len(rows)
            if guide is not None:     # one context row per frame, as interpolate hands them over; ctx_index names the ONE distinct row
                cond, unc = guide[0][0].expand(n, -1, -1), guide[1][0].expand(n, -1, -1)
                idx = [0] * n
                pooled = (guide[0][1].expand(n, -1), guide[1][1].expand(n, -1)) if len(sides[0][0]) > 1 else None
            else:
                cond, unc, idx = mixed(rows, 0, 0), mixed(rows, 0, 1), None
                pooled = (mixed(rows, 1, 0), mixed(rows, 1, 1)) if len(sides[0][0]) > 1 else None
            cond, unc = cond.to(dev, dtype).contiguous(), unc.to(dev, dtype).contiguous()
            lat = frame_latents[rows].to(dev, dtype) if frame_latents is not None else \
                torch.cat([nested_slerp(cl, w[i]) for i in rows], dim=0)
            blend.begin_replay(sig, dev)
            try:
                procs = {}
                for mode in {early} | ({late} - {"self"}):
                    install_blend_processors(self.unet, w[rows], blend, early=mode, corner_ctx=corner_ctx)
                    procs[mode] = dict(self.unet.attn_processors)
                graphs = _PassGraphs(_use_graphs(use_graphs, dev))
                ctx_both = torch.cat([cond, unc])           # ONE tensor for the whole run: the text K / V cache keys on it
                added_both = self._added_cond(None if pooled is None else torch.cat(pooled), 2 * n)
                idx_both = None if idx is None else idx + [j + 1 for j in idx]

                def both_pass(x, t):
                    return self._unet(torch.cat([x, x]), t, ctx_both, added_both, cak)

                for i, t in enumerate(self.scheduler.timesteps):
                    x = self.scheduler.scale_model_input(lat, t)
                    td = _dev_scalar(t, dev) if graphs.enabled else t
                    mode = early if i < warmup_steps else late
                    self.unet.set_attn_processor(procs[mode] if mode != "self" else procs[early])
                    if mode != "self":
                        blend.set_step(i)
                    set_aid_active(self.unet, mode != "self", plain_tail=n if mode != "self" else 0)
                    set_ctx_index(self.unet, idx_both)
                    both = graphs.run(("both", mode), both_pass, x=x, t=td)
                    noise = _guided_noise(both[:n], both[n:], gs, gr)
                    lat = self.scheduler.step(noise, t, lat, return_dict=False)[0]
                for j, i in enumerate(rows):
                    out[i] = lat[j:j + 1]
            finally:
                blend.abort()
                set_ctx_index(self.unet, None)
                self.unet.set_attn_processor(installed)
        return self._decode(torch.cat(out, dim=0), output_type)

    # -- small shape helpers (overridden by the XL class) ----------------------------------------------
    def _installed_aid_mode(self):
        """("outer" | "inner", is_fused) of the AID processors ``load_aid`` installed — what ``interpolate_single`` renders with."""
        for proc in self.unet.attn_processors.values():
            if isinstance(proc, P.InterpolatedAttnProcessor) and proc._mode is not None:
                return proc._mode, bool(proc.is_fused)
        raise RuntimeError("no AID processors installed: call load_aid first")

    def _pooled_inputs(self, cond_s, cond_e, unc_s, unc_e):
        """The pooled embeddings a run's signature covers (SDXL), [] for SD."""
        return [e[1] for e in (cond_s, cond_e, unc_s, unc_e) if len(e) > 1]

    def _split(self, embs):
        """(cond, uncond) -> ((cond,), (uncond,)); the XL class carries pooled embeddings in slot 1."""
        return (embs[0],), (embs[1],)

    def _pooled_single(self, cond_s, cond_e, unc_s, unc_e, guide, it, init):
        return None

    def _pooled_sequence(self, cond_s, cond_e, unc_s, unc_e, guide, size):
        return None

    def _image_embeds_single(self, image_start, image_end, ies, iee, it, init, dev, dtype):
        """pipeline_interpolated_sd.py:1763-1802: [start x3, target x3, end x3] image embeddings ``[9, 1, emb]`` for the
        conditional pass and their negative counterparts for the unconditional one; only ``image_end`` given = scale
        control (the start rows are the NEGATIVE embeddings of the end image)."""
        if image_end is not None and iee is None:
            iee = self._encode_image(image_end)
        if image_start is not None and ies is None:
            ies = self._encode_image(image_start)
        if iee is None:
            return None
        neg_e, pos_e = (t_.to(dev, dtype).expand(3, *t_.shape[1:]) for t_ in iee)
        if ies is None:
            neg_s, pos_s = neg_e, neg_e
        else:
            neg_s, pos_s = (t_.to(dev, dtype).expand(3, *t_.shape[1:]) for t_ in ies)
        mix = (lambda a, b: torch.lerp(a, b, it)) if init == "linear" else (lambda a, b: slerp(a, b, it))
        pos = torch.cat([pos_s, mix(pos_s, pos_e), pos_e], dim=0)
        neg = torch.cat([neg_s, mix(neg_s, neg_e), neg_e], dim=0)
        return [pos], [neg]

    def _image_embeds_sequence(self, image_start, image_end, ies, iee, coef, init, dev, dtype):
        """``_image_embeds_single`` evaluated at every coefficient of an N-frame run, one row per frame: ``([pos], [neg])`` with
        ``pos`` = ``[pos_start, mix(pos_start, pos_end, t_1), ..., pos_end]`` for the conditional pass and ``neg`` likewise for the
        unconditional one (one list entry per adapter: a pair may hold lists of tensors); only the end image given = scale control
        (the start rows are the NEGATIVE embeddings of the end image)."""
        if image_end is not None and iee is None:
            iee = self._encode_image(image_end)
        if image_start is not None and ies is None:
            ies = self._encode_image(image_start)
        as_list = (lambda e: [t_.to(dev, dtype) for t_ in (e if isinstance(e, (list, tuple)) else [e])])
        neg_e, pos_e = as_list(iee[0]), as_list(iee[1])
        neg_s, pos_s = (neg_e, neg_e) if ies is None else (as_list(ies[0]), as_list(ies[1]))
        ts = [float(t) for t in coef.tolist()]
        mix = (lambda a, b, t: torch.lerp(a, b, t)) if init == "linear" else (lambda a, b, t: slerp(a, b, t))

        def frames(a, b):
            return torch.cat([a] + [mix(a, b, t) for t in ts[1:-1]] + [b], dim=0).contiguous()
        return [frames(a, b) for a, b in zip(pos_s, pos_e)], [frames(a, b) for a, b in zip(neg_s, neg_e)]

    def _unet_device_dtype(self):
        p = next(self.unet.parameters())
        return p.device, p.dtype

    def _latent_hw(self):
        return getattr(self.unet, "latent_hw", None) or (getattr(getattr(self.unet, "config", None), "sample_size", 64),) * 2


class InterpolationStableDiffusionXLPipeline(InterpolationStableDiffusionPipeline):
    """SDXL variant (pipeline_interpolated_sdxl.py:1693-2411): ``encode_prompt`` returns
    ``(cond, uncond, pooled, negative_pooled)``; the pooled text embeddings and the micro-conditioning ``time_ids`` ride
    in ``added_cond_kwargs`` of every UNet call (:2230-2272).  The interior frame's pooled embedding is the guide
    prompt's or the lerp / slerp of the end points', like the token embeddings (:1998-2040)."""

    is_xl = True
    default_guidance_scale = 5.0

    def __init__(self, *a, original_size=(1024, 1024), crops_coords_top_left=(0, 0), target_size=(1024, 1024), **kw):
        super().__init__(*a, **kw)
        self.time_ids = torch.tensor([list(original_size) + list(crops_coords_top_left) + list(target_size)],
                                     dtype=torch.float32)

    def _split(self, embs):
        if len(embs) != 4:
            raise ValueError("SDXL needs (cond, uncond, pooled, negative_pooled) embeddings")
        return (embs[0], embs[2]), (embs[1], embs[3])

    def _pooled_single(self, cond_s, cond_e, unc_s, unc_e, guide, it, init):
        mix = (lambda a, b: torch.lerp(a, b, it)) if init == "linear" else (lambda a, b: slerp(a, b, it))
        pos = torch.cat([cond_s[1], guide[0][1] if guide else mix(cond_s[1], cond_e[1]), cond_e[1]], dim=0)
        neg = torch.cat([unc_s[1], guide[1][1] if guide else mix(unc_s[1], unc_e[1]), unc_e[1]], dim=0)
        return pos, neg

    def _pooled_sequence(self, cond_s, cond_e, unc_s, unc_e, guide, size):
        if guide:
            pos = torch.cat([cond_s[1]] + [guide[0][1]] * (size - 2) + [cond_e[1]], dim=0)
            neg = torch.cat([unc_s[1]] + [guide[1][1]] * (size - 2) + [unc_e[1]], dim=0)
        else:
            pos = linear_interpolation(cond_s[1], cond_e[1], size=size)
            neg = linear_interpolation(unc_s[1], unc_e[1], size=size)
        return pos, neg

    def _added_cond(self, pooled, n: int, image_embeds=None):
        dev, dtype = self._unet_device_dtype()
        added = {"text_embeds": pooled.to(dev, dtype), "time_ids": self.time_ids.to(dev, dtype).expand(n, -1)}
        if image_embeds is not None:
            added["image_embeds"] = image_embeds
        return added
