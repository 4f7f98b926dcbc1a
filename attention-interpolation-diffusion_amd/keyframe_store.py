"""Key-frame store: record key frames ONCE, render between any two of them.

An end point's trajectory depends on neither its partner nor the AID mode nor the fusion flag: with coefficient 0 or 1 every mode is
plain attention of that frame.  So what :class:`~.endpoint_store.EndpointStore` keeps per PAIR can be kept per FRAME, and one
recording serves every pair that contains the frame — a chain A -> B -> C, a hub with five partners — in both directions and under
every early mode.  A :class:`KeyframeStore` holds named key frames; per frame

* per self-attention layer, the projected keys and transposed values of the frame at every recorded AID step,
  ``k_store [n_steps, S C]`` / ``vt_store [n_steps, C round_up(S, 8)]`` (half of a pair slot; ``aid_processor_kf_fwd`` puts them there
  in the recording run and gets the two frames of a pair from there in a replaying one);
* the frame's inputs — initial latent, cond / uncond (and pooled) embeddings — and its final latent;

and per store ONE device step index and ONE set of run settings (``SETTINGS_FIELDS``): every frame is recorded under them, and a
replay under anything else raises.

``pipe.record_keyframes(store, names, ...)`` records; ``pipe.interpolate_between(store, a, b)`` / ``pipe.interpolate_chain(store,
[a, b, c])`` replay: only the interior frames go through the UNet.  ``pipe.interpolate_among(store, names, weights)`` renders frames
blended among up to eight of the recorded frames (``among`` / :class:`KeyframeBlend`): the cells of a morph grid, of
which only those that are not a key frame go through the UNet.

``KeyframeStore(storage="q8")`` keeps the K / V^T blocks in an 8-bit block format instead of the storage dtype (DESIGN.md §3.6e,
include/aid_hip.h): 32 int8 elements share one power-of-two exponent byte — 8.25 bits per element, 0.516x of a 16-bit store and
0.258x of a float32 one.  It is LOSSY and OPT-IN: the recording launch quantises, the replaying one dequantises, and every stored
element comes back within ``|y - x| <= 2^(e-1) < a / 127`` of what was recorded, ``a`` the largest magnitude of its block of 32
(relative L2 about 8e-3 on normal data).  The recording run itself is not touched — its frames and final latents are bit for bit a
native store's — and neither is anything behind the dequantising launch; only the interior frames a replay renders move, by what
DESIGN.md §3.6e measures against the fp64 loop.  Latents, embeddings and final latents stay unquantised.  Use it when the stores do
not fit otherwise (twelve SDXL key frames: 126 GB native, 65 GB q8); keep ``"native"`` (the default, unchanged) where a replay must
reproduce the full run to the storage dtype's own precision.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple

import torch

from . import ops
from .endpoint_store import StepIndex, _short

# what every frame of a store is recorded under, in the order a mismatch is reported
SETTINGS_FIELDS = ("num_inference_steps", "guidance_scale", "dtype", "f32_precision", "timesteps", "lora", "unet")


def _bytes(*tensors: Optional[torch.Tensor]) -> int:
    return sum(t.numel() * t.element_size() for t in tensors if t is not None)


class Keyframe:
    """One recorded key frame: ``layers[name] = (k_store, vt_store)``; ``latent`` the initial latent, ``embeds`` the frame's
    embeddings as the pipeline's ``encode_prompt`` returns them — (cond, uncond) or SDXL's (cond, uncond, pooled, negative_pooled);
    ``final`` the final latent."""

    def __init__(self):
        self.layers: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}
        self.latent: Optional[torch.Tensor] = None
        self.embeds: Tuple[torch.Tensor, ...] = ()
        self.final: Optional[torch.Tensor] = None

    @property
    def nbytes(self) -> int:
        return sum(_bytes(k, v) for k, v in self.layers.values()) + _bytes(self.latent, self.final, *self.embeds)


class KeyframeStore(StepIndex):
    """See the module docstring.  ``max_bytes``: a recording that would need more raises ``ValueError`` naming the bytes needed, before
    the buffer that crosses the limit is allocated — and what the refused recording had allocated so far is dropped; the frames
    recorded earlier stay.  ``storage``: "native" (the K / V^T blocks verbatim, in the storage dtype) or "q8" (8-bit blocks: lossy, about
    half the bytes of a 16-bit store — see the module docstring); a store has one storage for its life."""

    def __init__(self, max_bytes: Optional[int] = None, storage: str = "native"):
        if max_bytes is not None and int(max_bytes) < 0:
            raise ValueError("max_bytes must be None or >= 0")
        if storage not in ops.KF_STORAGES:
            raise ValueError(f"storage must be 'native' or 'q8'; got {storage!r}")
        self._storage = storage
        self.max_bytes = None if max_bytes is None else int(max_bytes)
        self._step: Optional[torch.Tensor] = None
        self.clear()

    # -- state ------------------------------------------------------------------------------------------------------------------
    def clear(self) -> None:
        """Back to an empty store.  Graphs captured against its buffers must be gone."""
        self.frames: Dict[str, Keyframe] = {}
        self.settings: Optional[Dict[str, Any]] = None
        self.n_steps = 0                           # AID steps every frame is recorded for
        self.mode: Optional[str] = None            # "record" / "replay" while a run uses the store
        self._pending: Dict[str, Keyframe] = {}    # the frames of the recording in progress, in batch order
        self._pair: Optional[Tuple[str, str]] = None
        self.step = -1

    @property
    def storage(self) -> str:
        """"native" or "q8": how the K / V^T blocks are kept (fixed at construction)."""
        return self._storage

    @property
    def names(self) -> List[str]:
        return list(self.frames)

    def __contains__(self, name: str) -> bool:
        return name in self.frames

    def __getitem__(self, name: str) -> Keyframe:
        try:
            return self.frames[name]
        except KeyError:
            raise KeyError(f"the key-frame store holds no frame {name!r} (it holds {self.names})") from None

    def remove(self, name: str) -> None:
        """Drop one key frame (its buffers go with it); the last one takes the store's settings along."""
        if self.mode is not None:
            raise RuntimeError("the store is in use by a run")
        self[name]
        del self.frames[name]
        if not self.frames:
            self.settings, self.n_steps = None, 0

    @property
    def nbytes(self) -> int:
        """Bytes the store holds: every frame's buffers, inputs and final latent (the frames of a recording in progress included)."""
        return sum(f.nbytes for f in self.frames.values()) + sum(f.nbytes for f in self._pending.values())

    def frame_bytes(self, name: str) -> int:
        """Bytes of one recorded key frame: its layers' buffers (``layer_bytes`` each), its inputs and its final latent."""
        return self[name].nbytes

    @staticmethod
    def layer_bytes(n_steps: int, l: int, c: int, dtype: torch.dtype, storage: str = "native") -> int:
        """Bytes of one self-attention layer of ONE key frame with ``l`` tokens of width ``c``: n_steps * (l c + c round_up(l, 8))
        elements — half of ``EndpointStore.layer_bytes``.  ``storage="q8"``: n_steps * (q8_block_bytes(l c) + q8_block_bytes(c
        round_up(l, 8))) bytes, whatever the dtype."""
        k_fs, vt_fs = ops.endpoint_block_sizes(l, c)
        if storage == "q8":
            return n_steps * (ops.q8_block_bytes(k_fs) + ops.q8_block_bytes(vt_fs))
        if storage != "native":
            raise ValueError(f"storage must be 'native' or 'q8'; got {storage!r}")
        return n_steps * (k_fs + vt_fs) * (torch.finfo(dtype).bits // 8)

    # -- settings ---------------------------------------------------------------------------------------------------------------
    def check(self, settings: Dict[str, Any], aid_steps: int) -> None:
        """Raise ``ValueError`` naming the FIRST setting (``SETTINGS_FIELDS`` order) in which a run differs from the recorded one, or
        ``aid_steps`` if it needs more AID steps than the frames were recorded for."""
        for f in SETTINGS_FIELDS:
            if self.settings.get(f) != settings.get(f):
                raise ValueError(f"the key-frame store was recorded under a different {f}: its frames replay (and further frames are "
                                 f"recorded) only under the settings of the first recording (recorded {_short(self.settings.get(f))}, "
                                 f"this run {_short(settings.get(f))}); clear() it to record again")
        if int(aid_steps) > self.n_steps:
            raise ValueError(f"the key-frame store was recorded with too few aid_steps: this run needs {int(aid_steps)} AID steps, the "
                             f"frames hold {self.n_steps} (record with aid_steps={int(aid_steps)} or more)")

    # -- a recording run --------------------------------------------------------------------------------------------------------
    def begin_record(self, names: Sequence[str], settings: Dict[str, Any], aid_steps: int, device: torch.device) -> None:
        names = [str(n) for n in names]
        if self.mode is not None:
            raise RuntimeError("the store is in use by another run")
        if not names or len(set(names)) != len(names):
            raise ValueError(f"record_keyframes needs distinct names, one per frame; got {names}")
        for n in names:
            if n in self.frames:
                raise ValueError(f"key frame {n!r} is already recorded: remove({n!r}) it first")
        if int(aid_steps) < 1:
            raise ValueError("a key frame is recorded for at least one AID step")
        if self.frames:
            self.check(settings, 0)
            if int(aid_steps) != self.n_steps:
                raise ValueError(f"the key-frame store was recorded under a different aid_steps: its frames hold {self.n_steps} AID "
                                 f"steps, this recording asks for {int(aid_steps)}")
        else:
            self.settings, self.n_steps = dict(settings), int(aid_steps)
        self.mode = "record"
        self._pending = {n: Keyframe() for n in names}
        self._ensure_step(device)

    def finish_record(self, latents: torch.Tensor, embeds: Sequence[Tuple[torch.Tensor, ...]], final: torch.Tensor) -> None:
        """``latents`` / ``final`` [K, ...]: the initial and the final latents of the recorded frames, ``embeds[i]`` the embeddings
        of frame i, in the order of ``begin_record``'s names."""
        if self.mode != "record":
            raise RuntimeError("finish_record outside a recording run")
        keep = lambda t: t.detach().clone()                            # noqa: E731
        parts = [(keep(latents[i:i + 1]), tuple(keep(t) for t in embeds[i]), keep(final[i:i + 1])) for i in range(len(self._pending))]
        self._refuse_over(self.nbytes + sum(_bytes(l_, f_, *e_) for l_, e_, f_ in parts))
        for frame, (l_, e_, f_) in zip(self._pending.values(), parts):
            frame.latent, frame.embeds, frame.final = l_, e_, f_
        self.frames.update(self._pending)
        self._pending, self.mode = {}, None

    def abort(self) -> None:
        """A recording run that did not finish leaves nothing of itself behind; a replaying one leaves the store as it was."""
        if self.mode == "record":
            self._drop_pending()
        self.mode, self._pair = None, None

    def _drop_pending(self) -> None:
        self._pending = {}
        if not self.frames:
            self.settings, self.n_steps = None, 0

    def _refuse_over(self, need: int) -> None:
        if self.max_bytes is not None and need > self.max_bytes:
            if self.mode == "record":
                self._drop_pending()
                self.mode = None
            raise ValueError(f"the key-frame store needs {need} bytes, max_bytes is {self.max_bytes}")

    # -- a replaying run --------------------------------------------------------------------------------------------------------
    def between(self, a: str, b: str) -> "KeyframePair":
        """The pair (begin = ``a``, end = ``b``) as the end points of one replaying run (``pipe.interpolate(..., endpoints=pair)``)."""
        self[a], self[b]
        if a == b:
            raise ValueError(f"a pair needs two different key frames; got {a!r} twice")
        return KeyframePair(self, str(a), str(b))

    def among(self, names: Sequence[str]) -> "KeyframeBlend":
        """1 .. 8 distinct recorded key frames as the corners of one blending run (``pipe.interpolate_among``): the M-frame sibling of
        ``between``.  The order of ``names`` is the order of the weight columns."""
        if isinstance(names, str):
            raise ValueError(f"among() takes a sequence of key-frame names; got the string {names!r}")
        names = [str(n) for n in names]
        if not 1 <= len(names) <= ops.MAX_CORNERS:
            raise ValueError(f"a blend takes 1 .. {ops.MAX_CORNERS} key frames; got {len(names)}")
        for n in names:
            self[n]
        if len(set(names)) != len(names):
            raise ValueError(f"a blend needs distinct key frames; got {names}")
        return KeyframeBlend(self, names)

    # -- per-layer buffers ------------------------------------------------------------------------------------------------------
    def kf_args(self, layer: str, l: int, c: int, dtype: torch.dtype, device: torch.device) -> dict:
        """The ``kf`` dictionary of ``ops.processor_kf_fwd`` for one call of ``layer`` in the run the store is in: RECORD, the frames of
        the recording as rows 0 .. K-1 of the batch (their buffers are allocated at the layer's first recorded call); REPLAY, the
        stores of the pair's begin and end frame; BLEND (``among``), the stores of the M key frames in weight-column order — the ``kf``
        of ``ops.processor_kf_blend_fwd``."""
        k_fs, vt_fs = ops.endpoint_block_sizes(l, c)
        q8 = self._storage == "q8"
        if self.mode == "record":
            entries = []
            for row, frame in enumerate(list(self._pending.values())):
                hit = frame.layers.get(layer)
                if hit is None:
                    self._refuse_over(self.nbytes + self.layer_bytes(self.n_steps, l, c, dtype, self._storage))
                    if torch.device(device).type == "cuda" and torch.cuda.is_current_stream_capturing():
                        raise RuntimeError("the first recorded call of a layer allocates its stores: run the pass once eagerly before "
                                           "capturing")
                    hit = (torch.empty(self.n_steps, ops.q8_block_bytes(k_fs), dtype=torch.uint8, device=device),
                           torch.empty(self.n_steps, ops.q8_block_bytes(vt_fs), dtype=torch.uint8, device=device)) if q8 else \
                          (torch.empty(self.n_steps, k_fs, dtype=dtype, device=device),
                           torch.empty(self.n_steps, vt_fs, dtype=dtype, device=device))
                    frame.layers[layer] = hit
                self._check_block(layer, hit, k_fs, vt_fs, dtype, device, self._storage)
                entries.append((hit[0], hit[1], row))
            return self._kf(entries, "record")
        if self.mode in ("replay", "blend"):
            entries = []
            for name in self._pair:
                hit = self.frames[name].layers.get(layer)
                if hit is None:
                    raise RuntimeError(f"key frame {name!r} holds no rows of layer {layer!r}: it was recorded on another UNet")
                self._check_block(layer, hit, k_fs, vt_fs, dtype, device, self._storage)
                entries.append((hit[0], hit[1], 0))
            return self._kf(entries, self.mode)
        raise RuntimeError("the key-frame store is attached to a processor outside a run (record_keyframes / interpolate_between / "
                           "interpolate_among)")

    def _kf(self, entries, mode: str) -> dict:
        """(a native store's dictionary is what it always was; a q8 store's names its storage)"""
        kf = dict(entries=entries, step=self._step, mode=mode)
        if self._storage != "native":
            kf["storage"] = self._storage
        return kf

    @staticmethod
    def _check_block(layer, hit, k_fs, vt_fs, dtype, device, storage: str = "native") -> None:
        k_store, vt_store = hit
        if storage == "q8":
            kb, vb = ops.q8_block_bytes(k_fs), ops.q8_block_bytes(vt_fs)
            if k_store.shape[1] != kb or vt_store.shape[1] != vb or k_store.dtype != torch.uint8 or k_store.device != torch.device(device):
                raise ValueError(f"layer {layer!r}: the q8 store holds block rows of {k_store.shape[1]} / {vt_store.shape[1]} bytes "
                                 f"({k_store.dtype}) on {k_store.device}, this call needs {kb} / {vb} bytes ({k_fs} / {vt_fs} elements) "
                                 f"on {device} (another resolution or device)")
            return
        if k_store.shape[1] != k_fs or vt_store.shape[1] != vt_fs or k_store.dtype != dtype or k_store.device != torch.device(device):
            raise ValueError(f"layer {layer!r}: the store holds blocks of {k_store.shape[1]} / {vt_store.shape[1]} {k_store.dtype} elements "
                             f"on {k_store.device}, this call needs {k_fs} / {vt_fs} {dtype} on {device} (another resolution, dtype or device)")


class KeyframePair:
    """Two key frames of a :class:`KeyframeStore` as the recorded end points of ONE replaying run: what the pipelines' ``endpoints=``
    reads of an ``EndpointStore`` (``recorded``, ``begin_replay``, ``set_step``, ``latents``, ``abort``), answered from the two frames."""

    recorded = True
    _mode = "replay"             # what the store's ``mode`` is during the run; a subclass (KeyframeBlend) sets its own and ``_names``

    def __init__(self, store: KeyframeStore, a: str, b: str):
        self.store, self.a, self.b = store, a, b

    def _names(self) -> Tuple[str, ...]:
        """The key frames of the run, as ``store._pair`` holds them during it."""
        return (self.a, self.b)

    @property
    def mode(self) -> Optional[str]:
        return self.store.mode

    @property
    def n_steps(self) -> int:
        return self.store.n_steps

    @property
    def latents(self) -> torch.Tensor:
        """[2, ...]: the final latents of the begin and the end frame."""
        return torch.cat([self.store[self.a].final, self.store[self.b].final], dim=0)

    def begin_replay(self, signature: Dict[str, Any], device: torch.device) -> None:
        """``signature``: ``endpoint_store.run_signature`` of the run.  Of it the store's settings must match and the run's AID steps
        (``int(T * warmup_ratio)``, or ``T`` with a late AID mode) must have been recorded; the pair, the mode and the fusion flag are
        free."""
        st = self.store
        if st.mode is not None:
            raise RuntimeError("the store is in use by another run")
        t = int(signature["num_inference_steps"])
        st.check(signature, int(t * float(signature["warmup_ratio"])) if signature.get("late") == "self" else t)
        st.mode, st._pair = self._mode, self._names()
        st._ensure_step(device)

    def set_step(self, i: int) -> None:
        self.store.set_step(i)

    def abort(self) -> None:
        self.store.abort()

    def kf_args(self, layer: str, l: int, c: int, dtype: torch.dtype, device: torch.device) -> dict:
        return self.store.kf_args(layer, l, c, dtype, device)


class KeyframeBlend(KeyframePair):
    """M <= 8 key frames of a :class:`KeyframeStore` as the corners of ONE blending run (``KeyframeStore.among``): ``begin_replay``
    (the same settings and AID-step check), ``set_step`` and ``abort`` are the pair's; ``latents`` are the M final latents and
    ``kf_args`` names the M stores of a layer (``mode="blend"``)."""

    _mode = "blend"

    def __init__(self, store: KeyframeStore, names: Sequence[str]):
        self.store, self.names = store, tuple(names)

    def _names(self) -> Tuple[str, ...]:
        return self.names

    @property
    def latents(self) -> torch.Tensor:
        """[M, ...]: the final latents of the key frames, in weight-column order."""
        return torch.cat([self.store[n].final for n in self.names], dim=0)
