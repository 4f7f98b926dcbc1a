"""End-point K / V^T store: render further frames between RECORDED end points.

The two end-point frames of an AID run need nothing from the interior frames — with coefficient 0 or 1 every mode is plain attention
of that frame (the fact ``dist.py`` relies on when it replicates them on every rank) — so for the same inputs their trajectory is the
same in every run.  An :class:`EndpointStore` keeps, from ONE run, what the interior frames of any later run need of them:

* per self-attention layer, the projected keys and transposed values of the two end points at every AID step,
  ``k_store [n_steps, 2, S C]`` / ``vt_store [n_steps, 2, C round_up(S, 8)]`` (``aid_processor_ep_fwd`` puts them there in the
  recording run and gets them from there in a replaying one; cross-attention needs nothing stored: the end points' text contexts are
  loop-invariant and ride behind the local contexts of a replay call);
* the end points' final latents;
* the signature of the run it was recorded under: a replay under anything else raises.

``pipe.interpolate_single(it, ..., endpoints=store)`` / ``pipe.interpolate(..., endpoints=store)`` record into an empty store (a
normal run, bit-identical outputs) and replay from a recorded one: only the requested interior frames go through the UNet.
"""
from __future__ import annotations

import hashlib
from typing import Any, Dict, List, Optional, Tuple

import torch

from . import lora, ops

# what a store is recorded under, in the order a mismatch is reported
SIGNATURE_FIELDS = ("latent_start", "latent_end", "embeds_start", "embeds_end", "embeds_negative", "embeds_pooled", "embeds_guide",
                    "num_inference_steps", "warmup_ratio", "early", "late", "fusion", "guidance_scale", "dtype", "f32_precision",
                    "timesteps", "lora", "unet")


def tensor_digest(*tensors: Optional[torch.Tensor]) -> Optional[str]:
    """Content digest (sha256 over shape, dtype and bytes) of tensors; None entries are skipped, all None gives None."""
    ts = [t for t in tensors if t is not None]
    if not ts:
        return None
    h = hashlib.sha256()
    for t in ts:
        t = t.detach()
        h.update(repr((tuple(t.shape), str(t.dtype))).encode())
        h.update(t.to("cpu").contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def lora_state(unet) -> Tuple:
    """The unmerged LoRA adapters a run would compute with: per wrapped projection its active adapters, their scalings and the
    (address, version) of their factors — what ``lora.pack`` keys its packs on."""
    out = []
    mods = unet.named_modules() if hasattr(unet, "named_modules") else ()
    for name, m in mods:
        if lora.is_lora_layer(m):
            acts = lora.active(m)
            out.append((name, tuple(acts), tuple(lora._tkey(m.lora_A[a].weight) + lora._tkey(m.lora_B[a].weight) for a, _ in acts)))
    return tuple(out)


class StepIndex:
    """The device step index of a store (shared with keyframe_store.KeyframeStore): ONE int32 on the device that the copy kernels read,
    and its host copy.  The owner sets ``n_steps``."""

    _step: Optional[torch.Tensor] = None
    step = -1                                      # host copy of the device index
    n_steps = 0

    def _ensure_step(self, device: torch.device) -> None:
        if self._step is None or self._step.device != torch.device(device):
            self._step = torch.zeros(1, dtype=torch.int32, device=device)
            self.step = 0

    @property
    def step_tensor(self) -> torch.Tensor:
        return self._step

    def set_step(self, i: int) -> None:
        """Name the AID step the next calls record into / replay from: ONE int32 on the device rewritten in place, stream-ordered
        and outside the captured graphs (as ``activate(t)`` rewrites the coefficient buffers) — a replayed graph reads the live index."""
        i = int(i)
        if not 0 <= i < max(self.n_steps, 1):
            raise IndexError(f"step {i} outside the store's {self.n_steps} AID steps")
        if self._step is None:
            raise RuntimeError("set_step before the run began (begin_record / begin_replay)")
        if self._step.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("set_step inside a stream capture: the index is rewritten between replays, not inside the graph")
        if i != self.step:
            self._step.fill_(i)
            self.step = i


class EndpointStore(StepIndex):
    """See the module docstring.  ``max_bytes``: a record that would need more raises ``ValueError`` naming the bytes needed, before
    the buffer that crosses the limit is allocated — and what the refused record had allocated so far is dropped, so nothing of it
    stays.  One store serves one pair of end points; ``clear()`` empties it for another."""

    def __init__(self, max_bytes: Optional[int] = None):
        if max_bytes is not None and int(max_bytes) < 0:
            raise ValueError("max_bytes must be None or >= 0")
        self.max_bytes = None if max_bytes is None else int(max_bytes)
        self._step: Optional[torch.Tensor] = None
        self.clear()

    # -- state ------------------------------------------------------------------------------------------------------------------
    def clear(self) -> None:
        """Back to an empty store (the next run with it records).  Graphs captured against its buffers must be gone."""
        self.layers: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}
        self.latents: Optional[torch.Tensor] = None
        self.signature: Optional[Dict[str, Any]] = None
        self.n_steps = 0
        self.mode: Optional[str] = None            # "record" / "replay" while a run uses the store
        self.recorded = False
        self.step = -1                             # host copy of the device index

    @property
    def nbytes(self) -> int:
        """Bytes of device memory the store holds: every layer's two buffers and the final latents."""
        n = sum(k.numel() * k.element_size() + v.numel() * v.element_size() for k, v in self.layers.values())
        return n + (0 if self.latents is None else self.latents.numel() * self.latents.element_size())

    @staticmethod
    def layer_bytes(n_steps: int, l: int, c: int, dtype: torch.dtype) -> int:
        """Bytes of one self-attention layer with ``l`` tokens of width ``c``: n_steps * 2 * (l c + c round_up(l, 8)) elements."""
        k_fs, vt_fs = ops.endpoint_block_sizes(l, c)
        return n_steps * 2 * (k_fs + vt_fs) * (torch.finfo(dtype).bits // 8)

    # -- a run ------------------------------------------------------------------------------------------------------------------
    def begin_record(self, signature: Dict[str, Any], n_steps: int, device: torch.device) -> None:
        if self.recorded or self.mode is not None:
            raise RuntimeError("the store is in use or already holds a recorded run: clear() it first")
        self.signature, self.n_steps, self.mode = dict(signature), int(n_steps), "record"
        self._ensure_step(device)

    def finish_record(self, latents: torch.Tensor) -> None:
        """``latents`` [2, ...]: the final latents of the begin and the end frame."""
        need = self.nbytes + latents.numel() * latents.element_size()
        self._refuse_over(need)
        self.latents = latents.detach().clone()
        self.mode, self.recorded = None, True

    def abort(self) -> None:
        """A recording run that did not finish leaves nothing behind; a replaying one leaves the store as it was."""
        if self.mode == "record":
            self.clear()
        self.mode = None

    def begin_replay(self, signature: Dict[str, Any], device: torch.device) -> None:
        if not self.recorded:
            raise RuntimeError("the store is empty: the first run with it records")
        if self.mode is not None:
            raise RuntimeError("the store is in use by another run")
        self.check(signature)
        self.mode = "replay"
        self._ensure_step(device)

    def check(self, signature: Dict[str, Any]) -> None:
        """Raise ``ValueError`` naming the FIRST field (``SIGNATURE_FIELDS`` order) in which ``signature`` differs from the recorded one."""
        for f in SIGNATURE_FIELDS:
            if self.signature.get(f) != signature.get(f):
                raise ValueError(f"the end-point store was recorded under a different {f}: a store replays only between the end points "
                                 f"and under the settings it was recorded with (recorded {_short(self.signature.get(f))}, this run "
                                 f"{_short(signature.get(f))}); clear() it to record again")

    # -- per-layer buffers ------------------------------------------------------------------------------------------------------
    def _refuse_over(self, need: int) -> None:
        if self.max_bytes is not None and need > self.max_bytes:
            if self.mode == "record":
                self.clear()
            raise ValueError(f"the end-point store needs {need} bytes, max_bytes is {self.max_bytes}")

    def slot(self, layer: str, l: int, c: int, dtype: torch.dtype, device: torch.device) -> Tuple[torch.Tensor, torch.Tensor]:
        """(k_store, vt_store) of a self-attention layer with ``l`` tokens of width ``c``; allocated at the layer's first recorded call."""
        k_fs, vt_fs = ops.endpoint_block_sizes(l, c)
        hit = self.layers.get(layer)
        if hit is None:
            if self.mode != "record":
                raise RuntimeError(f"the end-point store holds no rows of layer {layer!r}: it was recorded on another UNet or another mode")
            if self.n_steps < 1:
                raise RuntimeError("an AID call in a run that was announced without AID steps")
            self._refuse_over(self.nbytes + self.layer_bytes(self.n_steps, l, c, dtype))
            if torch.device(device).type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the first recorded call of a layer allocates its store: run the pass once eagerly before capturing")
            hit = (torch.empty(self.n_steps, 2, k_fs, dtype=dtype, device=device),
                   torch.empty(self.n_steps, 2, vt_fs, dtype=dtype, device=device))
            self.layers[layer] = hit
        k_store, vt_store = hit
        if tuple(k_store.shape[1:]) != (2, k_fs) or tuple(vt_store.shape[1:]) != (2, vt_fs) or k_store.dtype != dtype \
                or k_store.device != torch.device(device):
            raise ValueError(f"layer {layer!r}: the store holds blocks of {k_store.shape[2]} / {vt_store.shape[2]} {k_store.dtype} elements "
                             f"on {k_store.device}, this call needs {k_fs} / {vt_fs} {dtype} on {device} (another resolution, dtype or device)")
        return hit

    def ep_args(self, layer: str, l: int, c: int, dtype: torch.dtype, device: torch.device) -> dict:
        """The ``ep`` dictionary of ``ops.processor_ep_fwd`` for one call of ``layer`` in the run the store is in."""
        if self.mode is None:
            raise RuntimeError("the end-point store is attached to a processor outside a run (begin_record / begin_replay)")
        k_store, vt_store = self.slot(layer, l, c, dtype, device)
        return dict(k_store=k_store, vt_store=vt_store, step=self._step, mode=self.mode)


def _short(v) -> str:
    s = repr(v)
    return s if len(s) <= 24 else s[:21] + "..."


def run_settings(*, num_inference_steps: int, guidance_scale: float, dtype: torch.dtype, timesteps, unet, lora_scale=None,
                 guidance_rescale: float = 0.0) -> Dict[str, Any]:
    """The settings of a run that an end point's own trajectory depends on (shared with keyframe_store.py): the settings themselves,
    the float32 precision codes in force, the LoRA adapters' state and the identity of the UNet.  A non-zero ``guidance_rescale``
    changes the trajectory like the guidance scale does and rides in its entry: the pair ``(guidance_scale, guidance_rescale)``
    instead of the bare scale."""
    ts = timesteps.detach().to("cpu").tolist() if torch.is_tensor(timesteps) else [float(t) for t in timesteps]
    return {
        "num_inference_steps": int(num_inference_steps),
        "guidance_scale": float(guidance_scale) if float(guidance_rescale) == 0.0 else (float(guidance_scale), float(guidance_rescale)),
        "dtype": str(dtype),
        "f32_precision": (ops.f32_split_code(), ops.f32_attn_split_code()) if dtype == torch.float32 else (0, 0),
        "timesteps": tuple(ts), "lora": (lora_state(unet), None if lora_scale is None else float(lora_scale)),
        "unet": (type(unet).__name__, id(unet)),
    }


def run_signature(*, latent_start, latent_end, embeds_start, embeds_end, embeds_negative: List[Optional[torch.Tensor]],
                  embeds_pooled: List[Optional[torch.Tensor]], embeds_guide: List[Optional[torch.Tensor]], num_inference_steps: int,
                  warmup_ratio: float, early: str, late: str, fusion: bool, guidance_scale: float, dtype: torch.dtype, timesteps,
                  unet, lora_scale=None, guidance_rescale: float = 0.0) -> Dict[str, Any]:
    """The signature a pipeline run records / replays under (``SIGNATURE_FIELDS``): content digests of the tensors, the settings
    themselves, the float32 precision codes in force, the LoRA adapters' state and the identity of the UNet."""
    sig = {
        "latent_start": tensor_digest(latent_start), "latent_end": tensor_digest(latent_end),
        "embeds_start": tensor_digest(embeds_start), "embeds_end": tensor_digest(embeds_end),
        "embeds_negative": tensor_digest(*embeds_negative), "embeds_pooled": tensor_digest(*embeds_pooled),
        "embeds_guide": tensor_digest(*embeds_guide), "warmup_ratio": float(warmup_ratio),
        "early": str(early), "late": str(late), "fusion": bool(fusion),
        **run_settings(num_inference_steps=num_inference_steps, guidance_scale=guidance_scale, dtype=dtype, timesteps=timesteps,
                       unet=unet, lora_scale=lora_scale, guidance_rescale=guidance_rescale),
    }
    return {f: sig[f] for f in SIGNATURE_FIELDS}
