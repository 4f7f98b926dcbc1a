"""Denoising-loop harness around the AID processors (host orchestration rows of SURVEY.md §2).

Mirrors the control flow of the reference loops:
  * N-frame batch, one frame per coefficient — gradio ``interpolate``
    (gradio_src/pipeline_interpolated_stable_diffusion.py:163-304);
  * warm-up rule of the root pipelines — AID on for the CONDITIONAL pass of steps
    ``i < int(num_inference_steps * warmup_ratio)`` (0-based), de-activated otherwise, and always
    de-activated for the UNCONDITIONAL pass (pipeline_interpolated_sd.py:1831, 1845-1848, 1870;
    SURVEY.md App. D1: the build follows root, not gradio's off-by-one);
  * classifier-free guidance ``uncond + gs * (text - uncond)`` (pipeline_interpolated_sd.py:1892).
The UNet is anything exposing diffusers' ``attn_processors`` / ``set_attn_processor`` and being
callable as ``unet(sample, encoder_hidden_states)`` — a real diffusers UNet2DConditionModel wrapped
by the caller, or :class:`AttnStackUNet` (attention calls only) in the benchmark.

MI355X-first: the three distinct passes of the loop (conditional+AID, conditional plain,
unconditional plain) are captured once into hipGraphs and replayed per step, so the 32 (SD1.5) /
140 (SDXL) x 3 kernel launches of a pass cost one graph launch on the host.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional, Sequence, Tuple

import torch

from .processors import (CornerInterpolatedAttnProcessor, KeyframeBlendAttnProcessor, HipAttnProcessor, HipIPAdapterAttnProcessor, InnerInterpolatedAttnProcessor,
                         InnerInterpolatedIPAttnProcessor, InterpolatedAttnProcessor, OuterInterpolatedAttnProcessor,
                         OuterInterpolatedIPAttnProcessor, ScaleControlIPAttnProcessor, cache_generation, clear_weight_caches)

EARLY_MODES = ("pure_inner", "fused_inner", "pure_outer", "fused_outer")


IP_VARIANTS = ("interpolate", "scale_control")


def _adapter_of(cur):
    """The IP-Adapter state (``to_k_ip`` / ``to_v_ip`` / ``scale`` / ``num_tokens``) behind an installed processor — the processor
    itself or the ``ip_attn`` of an IP AID processor — or None for a layer without an adapter."""
    for holder in (cur, getattr(cur, "ip_attn", None)):
        if holder is not None and hasattr(holder, "to_k_ip"):
            return holder
    return None


def install_sequence_processors(unet, size: int, early: str = "fused_outer", alpha: Optional[float] = None,
                                beta: Optional[float] = None, num_inference_steps: int = 50,
                                coef: Optional[torch.Tensor] = None, ip_adapter: Optional[str] = None) -> None:
    """One AID processor per attention layer for an N-frame sequence; Beta(alpha, beta) coefficients with
    alpha = beta = num_inference_steps by default (gradio_src/...stable_diffusion.py:203-206, 237-260).
    ``coef`` overrides the schedule (used by the frame-sharded layout: the local rows of the global
    schedule).
    ``ip_adapter`` (None = text processors on every layer): the layers that hold an IP-Adapter — their installed processor, or its
    ``ip_attn``, has ``to_k_ip`` — get the IP variant instead: "interpolate" = ``OuterInterpolatedIPAttnProcessor`` for an outer
    ``early`` (``is_fused`` from ``early``) / ``InnerInterpolatedIPAttnProcessor`` for ``fused_inner`` (``pure_inner`` raises what the
    processor raises), "scale_control" = ``ScaleControlIPAttnProcessor`` (an outer ``early``).  Their ``ip_attn`` is the layer's
    ``HipIPAdapterAttnProcessor`` — the installed one, or one sharing the installed adapter's weights and scale list; a foreign
    processor kept by ``load_aid_ip_adapter(keep_original=True)`` stays.  Every other layer gets the text processor as without
    ``ip_adapter``.  A UNet without any adapter layer raises ``ValueError``."""
    if early not in EARLY_MODES:
        raise ValueError(f"early must be one of {EARLY_MODES}")
    if ip_adapter is not None:
        if ip_adapter not in IP_VARIANTS:
            raise ValueError(f"ip_adapter must be one of {IP_VARIANTS} or None, got {ip_adapter!r}")
        if ip_adapter == "scale_control" and not early.endswith("outer"):
            raise ValueError(f"scale control (only `image_end`) interpolates the text attention outer: early must be 'pure_outer' or "
                             f"'fused_outer', got {early!r}")
        if ip_adapter == "interpolate" and early == "pure_inner":
            raise RuntimeError("InnerInterpolatedIPAttnProcessor needs is_fused=True when image embeddings are "
                               "passed: the reference's image branch multiplies un-split keys "
                               "(batch1 dim mismatch in bmm, interpolation.py:525)")
        if not any(_adapter_of(cur) is not None for cur in unet.attn_processors.values()):
            raise ValueError("image inputs need a loaded IP-Adapter: no attention layer of the UNet holds one (load_ip_adapter / "
                             "load_aid_ip_adapter first)")
    alpha = num_inference_steps if alpha is None else alpha
    beta = num_inference_steps if beta is None else beta
    cls = OuterInterpolatedAttnProcessor if early.endswith("outer") else InnerInterpolatedAttnProcessor
    ip_cls = ScaleControlIPAttnProcessor if ip_adapter == "scale_control" else \
        OuterInterpolatedIPAttnProcessor if early.endswith("outer") else InnerInterpolatedIPAttnProcessor
    current = dict(unet.attn_processors)
    clear_weight_caches()                    # (see processors.py: in-place weight edits are invisible to the cache keys)
    procs = {}
    for name, cur in current.items():
        # (a given schedule may hold ONE coefficient — the interior frame of an end-point-store replay; the Beta schedule it
        #  replaces needs two points)
        kw = dict(size=size if coef is None else max(size, 2), is_fused=early.startswith("fused"), alpha=alpha, beta=beta)
        adapter = _adapter_of(cur) if ip_adapter is not None else None
        if adapter is not None:
            if not isinstance(adapter, HipIPAdapterAttnProcessor) and (adapter is cur or getattr(adapter, "weights_only", False)):
                adapter = HipIPAdapterAttnProcessor.wrap(adapter)
            p = ip_cls(ip_attn=adapter, **kw)
        else:
            p = cls(original_attn=HipAttnProcessor(), **kw)
        if coef is not None:
            assert coef.numel() == size
            p.size = size
            p.coef = coef.detach().to(torch.float32).cpu().clone()
        procs[name] = p
    unet.set_attn_processor(procs)


def install_corner_processors(unet, weights, corner_rows: Sequence[int], early: str = "fused_outer") -> None:
    """One ``CornerInterpolatedAttnProcessor`` per attention layer: frame i of the batch interpolates among the corner frames
    ``corner_rows`` with the weight row ``weights[i]`` (``[size, M]``, M <= 8), in the mode ``early`` names.  Every processor gets its own
    copy of the weights (edit them per processor, or install again).  IP-Adapter layers are refused: the image branches interpolate
    between two end points."""
    if early not in EARLY_MODES:
        raise ValueError(f"early must be one of {EARLY_MODES}")
    current = dict(unet.attn_processors)
    if any(_adapter_of(cur) is not None for cur in current.values()):
        raise NotImplementedError("corner-weighted AID on a UNet with IP-Adapter layers: the image branches interpolate between two "
                                  "end points only")
    clear_weight_caches()
    w = torch.as_tensor(weights, dtype=torch.float32).detach().cpu()
    procs = {}
    for name in current:
        procs[name] = CornerInterpolatedAttnProcessor(w.clone(), corner_rows, mode=early.split("_")[1],
                                                      is_fused=early.startswith("fused"), original_attn=HipAttnProcessor())
    unet.set_attn_processor(procs)


def install_blend_processors(unet, weights, blend, early: str = "fused_outer", corner_ctx: Optional[torch.Tensor] = None) -> None:
    """One ``KeyframeBlendAttnProcessor`` per attention layer: local frame i blends the recorded key frames of ``blend``
    (``KeyframeStore.among(names)``) with the weight row ``weights[i]`` (``[N_local, M]``), in the mode ``early`` names.  Each processor
    learns its layer's name in the store (its key in ``attn_processors``) and gets its own copy of the weights; ``corner_ctx``
    [M, L, Cc] — the key frames' cond contexts — serves the cross-attention layers.  IP-Adapter layers are refused, as for
    ``install_corner_processors``."""
    if early not in EARLY_MODES:
        raise ValueError(f"early must be one of {EARLY_MODES}")
    current = dict(unet.attn_processors)
    if any(_adapter_of(cur) is not None for cur in current.values()):
        raise NotImplementedError("a key-frame blend on a UNet with IP-Adapter layers: the image branches interpolate between two "
                                  "end points only")
    clear_weight_caches()
    w = torch.as_tensor(weights, dtype=torch.float32).detach().cpu()
    procs = {}
    for name in current:
        procs[name] = KeyframeBlendAttnProcessor(w.clone(), blend, mode=early.split("_")[1], is_fused=early.startswith("fused"),
                                                 original_attn=HipAttnProcessor(), layer=name, corner_ctx=corner_ctx)
    unet.set_attn_processor(procs)


def set_aid_active(unet, active: bool, plain_tail: int = 0) -> None:
    """N-frame analogue of activate_aid / deactivate_aid that keeps the coefficient schedule
    (the reference's activate(t) resets coef to [0, t, 1] for its batch-3 loop).  ``plain_tail`` frames
    appended after the interpolated ones run plain attention in the same call (batched CFG)."""
    for proc in unet.attn_processors.values():
        if isinstance(proc, InterpolatedAttnProcessor):
            proc.activated = bool(active)
            proc.plain_tail = int(plain_tail)


def set_ctx_index(unet, ctx_index: Optional[Sequence[int]]) -> None:
    """Tell every processor which row of ``encoder_hidden_states`` each frame of the next UNet call uses
    (None = one context per frame).  See InterpolatedAttnProcessor.ctx_index."""
    idx = None if ctx_index is None else [int(i) for i in ctx_index]
    for proc in unet.attn_processors.values():
        if hasattr(proc, "ctx_index"):
            proc.ctx_index = idx
        inner = getattr(proc, "original_attn", None)
        if inner is not None and hasattr(inner, "ctx_index"):
            inner.ctx_index = idx


def set_endpoint_store(unet, store, endpoint_ctx: Optional[torch.Tensor] = None, coef=None) -> None:
    """Attach an ``EndpointStore`` (endpoint_store.py) to every AID processor of ``unet`` for one run — or detach it (``store=None``).
    Each processor learns its layer's name in the store (its key in ``attn_processors``).  ``endpoint_ctx`` [2, L, Cc]: the text
    contexts of the two end-point frames, for the cross-attention calls of a REPLAY run; ``coef``: the interior coefficients a replay
    processor holds (its batch has no end points).  IP-Adapter processors refuse a store at their first call."""
    for name, proc in unet.attn_processors.items():
        if isinstance(proc, InterpolatedAttnProcessor):
            had = getattr(proc, "endpoint_store", None) is not None
            proc.endpoint_store = store
            proc.endpoint_layer = name if store is not None else None
            if store is not None or had:              # (the exchange layout's own endpoint_ctx is left alone)
                proc.endpoint_ctx = endpoint_ctx
            if coef is not None:
                proc.coef = torch.as_tensor(coef, dtype=torch.float32).detach().cpu().clone()


def set_keyframe_store(unet, store, record: Optional[Sequence[str]] = None, between: Optional[Tuple[str, str]] = None,
                       endpoint_ctx: Optional[torch.Tensor] = None, coef=None) -> None:
    """Attach a ``KeyframeStore`` (keyframe_store.py) to every AID processor of ``unet`` for one pass or run — or detach it
    (``store=None``).  ``record=[names]``: the store is recording those frames (``begin_record``), the processors' plain self-attention
    calls put rows 0 .. K-1 of their batch into them.  ``between=(a, b)``: the store is replaying that pair (``between(a, b).begin_replay``),
    ``endpoint_ctx`` [2, L, Cc] holds the two frames' text contexts for the cross-attention calls and ``coef`` the interior
    coefficients, as in ``set_endpoint_store``.  A processor holds either kind of store, never both; IP-Adapter processors refuse a
    store at their first call."""
    if store is not None:
        if (record is None) == (between is None):
            raise ValueError("set_keyframe_store takes record=[names] or between=(a, b)")
        want = "record" if record is not None else "replay"
        if store.mode != want:
            raise RuntimeError(f"the key-frame store is not in a {want} run (begin_record / between(a, b).begin_replay come first)")
        if record is not None and list(record) != list(store._pending):
            raise ValueError(f"the store is recording {list(store._pending)}, not {list(record)}")
        if between is not None and tuple(between) != tuple(store._pair):
            raise ValueError(f"the store is replaying {tuple(store._pair)}, not {tuple(between)}")
    for name, proc in unet.attn_processors.items():
        if isinstance(proc, InterpolatedAttnProcessor):
            if store is not None and getattr(proc, "endpoint_store", None) is not None:
                raise RuntimeError("the processor holds an end-point store: a processor takes an EndpointStore or a KeyframeStore, "
                                   "not both (set_endpoint_store(unet, None) first)")
            had = getattr(proc, "keyframe_store", None) is not None
            proc.keyframe_store = store
            if store is not None or had:
                proc.endpoint_layer = name if store is not None else None
                proc.endpoint_ctx = endpoint_ctx
            if coef is not None:
                proc.coef = torch.as_tensor(coef, dtype=torch.float32).detach().cpu().clone()


def _record_stream(out, stream) -> None:
    if torch.is_tensor(out):
        out.record_stream(stream)
    elif isinstance(out, dict):
        for v in out.values():
            _record_stream(v, stream)
    elif isinstance(out, (tuple, list)):
        for v in out:
            _record_stream(v, stream)


def fork_join(first: Callable, second: Callable, side: "torch.cuda.Stream"):
    """``first()`` on the current stream and ``second()`` on ``side``, concurrently; both have finished (for the current stream) on
    return.  Inside a stream capture the fork and the join become edges of the graph.  The two callables run one after the other on
    the host, so Python-side state they toggle (``set_aid_active``) is seen in program order; what ``second`` returns was allocated on
    ``side`` and is handed to the current stream (``record_stream``; captured allocations live in the graph's pool)."""
    cur = torch.cuda.current_stream()
    side.wait_stream(cur)
    gen = cache_generation()
    a = first()
    if cache_generation() != gen:
        # ``first`` (re)built a lazily shared tensor on the current stream — a text K / V projection, folded LayerNorm weights (cold
        # caches, new prompt tensors on a reused loop, a clear_weight_caches() in between): ``second`` reads it on the side stream, so
        # the side stream is ordered behind everything ``first`` has enqueued.  One step loses its overlap; no step races.
        side.wait_stream(cur)
    with torch.cuda.stream(side):
        b = second()
    cur.wait_stream(side)
    if not torch.cuda.is_current_stream_capturing():
        _record_stream(b, cur)
    return a, b


class AidDenoiseLoop:
    """Replays the per-step attention work of an interpolation run.

    step(i): conditional pass (AID on while i < warmup_steps) + unconditional pass (plain) + CFG
    combine of the two pass outputs.  ``use_graphs`` captures the passes into hipGraphs.
    """

    def __init__(self, unet, sample, cond, uncond, num_inference_steps: int = 50, warmup_ratio: float = 0.5,
                 guidance_scale: float = 7.5, use_graphs: bool = True, combine: Optional[Callable] = None,
                 batched_cfg: bool = False, ctx_index: Optional[Sequence[int]] = None, concurrent_cfg: bool = False,
                 guidance_rescale: float = 0.0):
        """``batched_cfg``: run the conditional and the unconditional pass of a step as ONE UNet call over the
        batch [cond frames ; uncond frames] (how stock diffusers pipelines do classifier-free guidance).  The
        AID processors treat the second half as plain riders (negative coefficients), so the result equals the
        reference's two separate calls while every GEMM sees twice the rows and the launch count halves."""
        """``ctx_index`` (frame -> row of ``cond`` / ``uncond``): the sequence shares text contexts (PAID guide
        prompt, sequence.py); ``cond`` / ``uncond`` then hold the DISTINCT contexts only."""
        """``cond`` / ``uncond`` may be ``(text, [image_embeds])`` tuples — the ``encoder_hidden_states`` an IP-Adapter UNet
        hands its attention layers (interpolation.py:259-266); the two passes then run as two UNet calls."""
        """``concurrent_cfg``: when the two passes of a step cannot share one UNet call (IP-Adapter contexts), run them as two UNet
        calls on two STREAMS — forked and joined inside one hipGraph when ``use_graphs`` — instead of back to back: the passes are
        independent, every kernel of one overlaps the other's (half the rows per kernel, both halves in flight).  Same results."""
        """``guidance_rescale`` > 0: the default combine rescales the guided output of every frame to the text pass's spread
        (pipeline_interpolated_sd.py:92-108, 1892-1902) — guidance and rescale in one launch (``ops.cfg_rescale``), in every layout."""
        self.unet, self.sample, self.cond, self.uncond = unet, sample, cond, uncond
        self.batched_cfg = batched_cfg
        self.concurrent_cfg = concurrent_cfg and not batched_cfg
        self._side = None
        first = next(iter(sample.values())) if isinstance(sample, dict) else sample
        self.n_frames = first.shape[0]
        self.ctx_index = None if ctx_index is None else [int(i) for i in ctx_index]
        if self.ctx_index is not None and len(self.ctx_index) != self.n_frames:
            raise ValueError("ctx_index needs one entry per frame")
        if isinstance(cond, tuple):
            if batched_cfg or ctx_index is not None:
                raise ValueError("(text, [image_embeds]) contexts run as two separate passes without ctx_index")
        elif self.ctx_index is None and cond.shape[0] != self.n_frames:
            raise ValueError("one context per frame expected (or pass ctx_index)")
        self.ctx_index2 = None
        if batched_cfg:
            dup = (lambda t: torch.cat([t, t], dim=0))
            self.sample2 = {k: dup(v) for k, v in sample.items()} if isinstance(sample, dict) else dup(sample)
            self.ctx2 = torch.cat([cond, uncond], dim=0)
            if self.ctx_index is not None:
                self.ctx_index2 = self.ctx_index + [i + cond.shape[0] for i in self.ctx_index]
        self.num_inference_steps = num_inference_steps
        self.warmup_steps = int(num_inference_steps * warmup_ratio)        # pipeline_interpolated_sd.py:1831
        self.guidance_scale = guidance_scale
        self.guidance_rescale = float(guidance_rescale)
        if not 0.0 <= self.guidance_rescale <= 1.0:
            raise ValueError(f"guidance_rescale must be in [0, 1]; got {guidance_rescale}")
        self.use_graphs = use_graphs
        self.combine = combine or self._cfg
        self._graphs: Dict[Tuple[str, int], torch.cuda.CUDAGraph] = {}
        self.fallback_reason: Optional[str] = None        # set when a capture failed and the loop went eager
        from . import ops
        self._ws = ops.WorkspaceOwner()          # the captures' workspaces are dropped with this loop (and its graphs)
        self._warmed: set = set()
        self._cap = None
        self._outs: Dict[Tuple[str, int], object] = {}

    def _cfg(self, text, uncond):
        if isinstance(text, dict):
            return {k: self._cfg(text[k], uncond[k]) for k in text}
        if self.guidance_rescale > 0.0:
            from . import ops
            return ops.cfg_rescale(text, uncond, self.guidance_scale, self.guidance_rescale)
        return uncond + self.guidance_scale * (text - uncond)

    # -- the three distinct passes ---------------------------------------------------------------
    def _pass(self, which: str):
        set_ctx_index(self.unet, self.ctx_index2 if which.startswith("both") else self.ctx_index)
        if which == "both_aid":
            set_aid_active(self.unet, True, plain_tail=self.n_frames)
            return self.unet(self.sample2, self.ctx2)
        if which == "both_plain":
            set_aid_active(self.unet, False)
            return self.unet(self.sample2, self.ctx2)
        if which.startswith("pair"):                    # cond pass on the current stream, uncond pass on the side stream
            if self._side is None:
                self._side = torch.cuda.Stream()

            def cond_pass():
                set_aid_active(self.unet, which == "pair_aid", plain_tail=0)
                return self.unet(self.sample, self.cond)

            def uncond_pass():
                set_aid_active(self.unet, False)
                return self.unet(self.sample, self.uncond)
            from . import ops
            self._warm_pair(which, cond_pass, uncond_pass)
            with ops.cu_share(2):                       # two launch streams share the device: every call of both passes plans with half the CUs
                return fork_join(cond_pass, uncond_pass, self._side)
        if which == "cond_aid":
            set_aid_active(self.unet, True, plain_tail=0)
            return self.unet(self.sample, self.cond)
        set_aid_active(self.unet, False)
        return self.unet(self.sample, self.cond if which == "cond_plain" else self.uncond)

    def _warm_pair(self, which: str, cond_pass: Callable, uncond_pass: Callable) -> None:
        """The first forked step of a kind on cold caches: ``cond_pass`` fills lazily built shared state on the current
        stream — the folded LayerNorm weights, the text K / V cache — that ``uncond_pass`` reads on the side stream, and ``fork_join``
        orders the side stream behind the fork point only.  So the pair runs ONCE back to back on the current stream first (outputs
        dropped); every forked step after that finds the caches filled.  (Graph mode warms up the same way before its capture.)"""
        if torch.cuda.is_current_stream_capturing():
            return                                      # the eager warm-up of _run() has been here already
        key = (which, cache_generation())               # caches cleared / refilled since: warm again (fork_join guards the rest)
        if key in self._warmed:
            return
        cond_pass()
        uncond_pass()
        self._warmed = {(which, cache_generation())}

    @staticmethod
    def _graph_key(which: str, unet=None):
        """A graph holds the kernels of the float32 matmul precision and of the attention core's precision it was captured under —
        and, where a key-frame store with another storage than "native" is attached to ``unet`` (``set_keyframe_store``), that store's
        copy launch: its storage joins the key."""
        from . import ops
        key = (which, ops.f32_split_code(), ops.f32_attn_split_code())
        for proc in (getattr(unet, "attn_processors", None) or {}).values():
            storage = getattr(getattr(proc, "keyframe_store", None), "storage", "native")
            if storage != "native":
                return key + (storage,)
        return key

    def _run(self, which: str):
        if not self.use_graphs:
            return self._pass(which)
        gk = self._graph_key(which, self.unet)
        g = self._graphs.get(gk)
        if g is None:
            cur = torch.cuda.current_stream()
            if self._cap is None:
                self._cap = torch.cuda.Stream()         # warm-up AND capture stream of this loop: the capture adopts the warm-up's workspace
            cap = self._cap
            cap.wait_stream(cur)
            with torch.cuda.stream(cap):                # warm-up: lazy kernel attributes, coef caches, workspaces (ops.workspace)
                self._pass(which)
            cur.wait_stream(cap)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            try:
                with self._ws, torch.cuda.graph(g, stream=cap):
                    self._outs[gk] = self._pass(which)
            except RuntimeError as e:
                # a pass that cannot be captured (a collective of the end-point-exchange layout on a stack whose RCCL does not record
                # into graphs, a foreign UNet that synchronises): the loop goes on eagerly, loudly (pipelines._PassGraphs does the same)
                import warnings
                self.use_graphs = False
                self.fallback_reason = f"{type(e).__name__}: {e}"
                self._graphs.clear()
                self._outs.clear()
                self._ws.release()
                warnings.warn("hipGraph capture of a pass failed, the loop continues eagerly: " + self.fallback_reason, RuntimeWarning,
                              stacklevel=3)
                try:
                    torch.cuda.synchronize()
                except RuntimeError as e2:
                    raise RuntimeError(f"device unusable after a failed stream capture ({self.fallback_reason})") from e2
                return self._pass(which)
            self._graphs[gk] = g
        g.replay()
        return self._outs[gk]

    def aid_on(self, i: int) -> bool:
        return i < self.warmup_steps

    def step(self, i: int):
        if self.batched_cfg:
            both = self._run("both_aid" if self.aid_on(i) else "both_plain")
            n = self.n_frames
            if isinstance(both, dict):
                return self.combine({k: v[:n] for k, v in both.items()}, {k: v[n:] for k, v in both.items()})
            return self.combine(both[:n], both[n:])
        if self.concurrent_cfg:
            text, unc = self._run("pair_aid" if self.aid_on(i) else "pair_plain")
            return self.combine(text, unc)
        text = self._run("cond_aid" if self.aid_on(i) else "cond_plain")
        unc = self._run("uncond")
        return self.combine(text, unc)
