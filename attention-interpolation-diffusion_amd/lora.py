"""Unmerged LoRA adapters on the attention projections (diffusers' PEFT backend).

With ``pipe.load_lora_weights(...)`` diffusers wraps ``attn.to_q`` / ``to_k`` / ``to_v`` / ``to_out[0]`` in PEFT ``lora.Linear``
layers whose forward is ``base_layer(x) + sum_active lora_B(lora_A(dropout(x))) * scaling[adapter]``.  The processors of this
package never call those modules: they read the weights by pointer, and a wrapper's ``weight`` is its base layer's.  This module
finds the wrappers (duck typing: peft is not imported) and turns their active adapters into the two operands the library adds to
the projection's GEMM accumulator (include/aid_hip.h, AidProcessorArgs.lora_* / AidGemmProblem.lr_*):

    A_pack [R, in]   the adapters' lora_A weights stacked by rows, each multiplied by its scaling
    B_pack [out, R]  their lora_B weights side by side
    R = round_up(sum r_a, 64); the padding rows / columns are zero.

PEFT's forward decision table is mirrored: ``disable_adapters`` -> base only (a merged layer is unmerged first, as PEFT's forward
does); ``merged`` -> base only (the deltas already sit in the base weight); otherwise every active adapter present in ``lora_A``.
What the packs cannot express raises NotImplementedError: ``lora_bias``, dropout with p > 0 in training mode and the old
``LoRACompatibleLinear.lora_layer``.

DoRA (``use_dora[adapter]`` with ``lora_magnitude_vector[adapter].weight`` of shape [out]).  In eval mode PEFT computes
``g o (x W^T + s B A x) + bias`` with the row gain ``g[n] = magnitude[n] / ||W[n, :] + s (B A)[n, :]||`` (no gradient, no epsilon),
and re-materialises ``B A`` and the norm on every forward.  The gain depends on weights only: the pack of a DoRA layer also holds
``gain`` (fp32 [out], ``ops.dora_gain`` — one HIP launch per pack), keyed additionally by the base weight's and the magnitude's
(data_ptr, _version), and the projection GEMM multiplies its fp32 accumulator by it before the epilogue (AidGemmProblem.lr_row_scale).
Refused (NotImplementedError naming DoRA): the flag without a magnitude vector; a DoRA adapter active together with any other
adapter of the layer (PEFT feeds the running result into the next adapter's DoRA term; not restated); a quantised or
``fan_in_fan_out`` base layer.  There is no CPU fallback for the gain.
"""
from __future__ import annotations

import weakref
from typing import List, NamedTuple, Optional, Tuple

import torch
from torch import nn

RANK_ALIGN = 64          # the library's low-rank K segment runs in whole 64-wide K tiles
MAX_RANK = 512           # AidGemmProblem.lr_k <= 512

# per wrapper module: (key, LoraPack); per attention module: (key, LoraArgs).  Dropped by processors.clear_weight_caches().
_PACK_CACHE: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()
_ARGS_CACHE: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


class LoraPack(NamedTuple):
    a: torch.Tensor          # [R, in]  scaling folded in
    b: torch.Tensor          # [out, R]
    rank: int                # R (a multiple of 64)
    key: tuple               # what the pack was built from (names, scalings, factor versions, dtype, device; DoRA: W and magnitude too)
    gain: Optional[torch.Tensor] = None      # DoRA: fp32 [out] row gain of the projection's accumulator


class LoraArgs(NamedTuple):
    """Operands of one processor call (ops.processor_fwd(lora=...)); a rank of 0 = no adapter on that projection."""
    down_x: Optional[torch.Tensor]      # [r_q (+ r_k + r_v for self-attention), c]
    down_ctx: Optional[torch.Tensor]    # [r_k + r_v, cc] (cross-attention)
    down_o: Optional[torch.Tensor]      # [r_o, c]
    up: Tuple[Optional[torch.Tensor], ...]     # B_pack of q, k, v, o
    ranks: Tuple[int, int, int, int]
    key: tuple
    gains: Tuple[Optional[torch.Tensor], ...] = (None, None, None, None)      # DoRA row gains of q, k, v, o (fp32 [c])


def is_lora_layer(mod) -> bool:
    """A PEFT ``lora.Linear``-like wrapper (base_layer + lora_A / lora_B module dicts)."""
    return mod is not None and hasattr(mod, "base_layer") and hasattr(mod, "lora_A") and hasattr(mod, "lora_B")


def _flag(d, name: str) -> bool:
    """PEFT keeps use_dora / lora_bias as {adapter: bool} dicts."""
    return bool(d.get(name, False)) if isinstance(d, dict) else False


def dora_magnitude(mod, a: str) -> Optional[torch.Tensor]:
    """The magnitude vector of adapter ``a`` when it is a DoRA adapter (None for plain LoRA).  Raises NotImplementedError for a DoRA
    layer the HIP path does not compute."""
    if not _flag(getattr(mod, "use_dora", {}), a):
        return None
    mv = getattr(mod, "lora_magnitude_vector", None)
    try:
        mag = mv[a].weight if mv is not None and a in mv else None
    except (TypeError, AttributeError):
        mag = None
    n_out = int(mod.lora_B[a].weight.shape[0])
    if not torch.is_tensor(mag) or tuple(mag.shape) != (n_out,):
        raise NotImplementedError(f"DoRA adapter {a!r} without a lora_magnitude_vector of shape [{n_out}]")
    w = mod.base_layer.weight
    if getattr(mod, "fan_in_fan_out", False):
        raise NotImplementedError(f"DoRA adapter {a!r} on a fan_in_fan_out layer")
    if not torch.is_floating_point(w) or hasattr(w, "quant_state") or tuple(w.shape) != (n_out, int(mod.lora_A[a].weight.shape[1])):
        raise NotImplementedError(f"DoRA adapter {a!r} on a quantised base layer")
    return mag


def active(mod) -> List[Tuple[str, float]]:
    """(adapter name, scaling) of the adapters PEFT's forward would add on ``mod`` — [] for a plain layer, a disabled or a merged
    wrapper.  Raises NotImplementedError for what the HIP path does not compute."""
    if getattr(mod, "lora_layer", None) is not None:
        raise NotImplementedError("LoRACompatibleLinear.lora_layer (the pre-PEFT diffusers LoRA) is not supported: load the adapter "
                                  "through the PEFT backend or fuse it (fuse_lora())")
    if not is_lora_layer(mod):
        return []
    if getattr(mod, "disable_adapters", False):
        if getattr(mod, "merged", False):          # PEFT's forward unmerges a merged layer whose adapters were disabled
            mod.unmerge()
            from .processors import clear_weight_caches
            clear_weight_caches()
        return []
    if getattr(mod, "merged", False):
        return []
    names = mod.active_adapters
    if isinstance(names, str):
        names = [names]
    out = []
    for a in names:
        if a not in mod.lora_A:
            continue
        dora_magnitude(mod, a)                     # raises for a DoRA adapter that cannot be computed
        if _flag(getattr(mod, "lora_bias", {}), a):
            raise NotImplementedError(f"adapter {a!r} has lora_bias: the HIP path does not compute it")
        drops = getattr(mod, "lora_dropout", None)
        drop = drops[a] if drops is not None and a in drops else None
        if isinstance(drop, nn.Dropout) and drop.p > 0 and drop.training:
            raise NotImplementedError(f"adapter {a!r}: LoRA dropout p = {drop.p} in training mode (call .eval())")
        out.append((a, float(mod.scaling[a])))
    if len(out) > 1 and any(_flag(getattr(mod, "use_dora", {}), a) for a, _ in out):
        raise NotImplementedError("a DoRA adapter active together with another adapter of the layer (" +
                                  ", ".join(repr(a) for a, _ in out) + "): PEFT chains them through the running result")
    return out


def _tkey(t: torch.Tensor) -> tuple:
    try:
        v = t._version
    except Exception:                 # inference-mode tensor: no version counter, the address alone is the key
        v = None
    return (t.data_ptr(), v, tuple(t.shape), t.dtype)


def pack(mod, dtype: torch.dtype, device: torch.device) -> Optional[LoraPack]:
    """The (A_pack, B_pack) of ``mod``'s active adapters in ``dtype`` (cached), or None without any.  A DoRA layer's pack also holds
    its row gain."""
    acts = active(mod)
    if not acts:
        return None
    key = (tuple(acts), tuple(_tkey(mod.lora_A[a].weight) + _tkey(mod.lora_B[a].weight) for a, _ in acts), dtype, str(device))
    mag = dora_magnitude(mod, acts[0][0])          # a DoRA adapter is the only active one (active())
    if mag is not None:
        key += (_tkey(mod.base_layer.weight), _tkey(mag))
    ent = _PACK_CACHE.get(mod)
    if ent is not None and ent[0] == key:
        return ent[1]
    from . import processors
    processors._CACHE_GEN[0] += 1                 # a rebuilt shared tensor: loop.fork_join orders its fill before the other stream
    fa = [mod.lora_A[a].weight for a, _ in acts]
    fb = [mod.lora_B[a].weight for a, _ in acts]
    r_tot = sum(int(w.shape[0]) for w in fa)
    rank = (r_tot + RANK_ALIGN - 1) // RANK_ALIGN * RANK_ALIGN
    if rank > MAX_RANK:
        raise NotImplementedError(f"total LoRA rank {r_tot} of the active adapters exceeds {MAX_RANK}")
    n_in, n_out = int(fa[0].shape[1]), int(fb[0].shape[0])
    with torch.no_grad():
        a_pack = torch.zeros(rank, n_in, dtype=dtype, device=device)
        b_pack = torch.zeros(n_out, rank, dtype=dtype, device=device)
        row = 0
        for (_, s), wa, wb in zip(acts, fa, fb):
            r = int(wa.shape[0])
            a_pack[row:row + r] = (wa.detach().to(device=device, dtype=torch.float32) * s).to(dtype)
            b_pack[:, row:row + r] = wb.detach().to(device=device, dtype=dtype)
            row += r
        gain = None
        if mag is not None:                        # DoRA: gain = magnitude / ||W + s B A||_row, from the numbers the GEMM multiplies
            from . import ops
            gain = ops.dora_gain(mod.base_layer.weight.detach(), a_pack, b_pack, mag.detach().to(device=device, dtype=dtype).contiguous())
    p = LoraPack(a_pack, b_pack, rank, key, gain)
    _PACK_CACHE[mod] = (key, p)
    return p


def projections(attn):
    """to_q, to_k, to_v, to_out[0] of an attention module (None where it has no such layer)."""
    out = getattr(attn, "to_out", None)
    return (getattr(attn, "to_q", None), getattr(attn, "to_k", None), getattr(attn, "to_v", None), out[0] if out else None)


def any_lora(attn) -> bool:
    """Is any projection of ``attn`` a LoRA wrapper (active or not)?"""
    return any(is_lora_layer(m) or getattr(m, "lora_layer", None) is not None for m in projections(attn))


def args(attn, dtype: torch.dtype, device: torch.device, cross: bool, kv: bool = True) -> Optional[LoraArgs]:
    """Operands of a processor call on ``attn`` (None: no active adapter).  ``kv=False``: the keys / values come from the text-K/V
    cache, whose projections already hold their adapter terms, so k / v get rank 0 here."""
    if not any_lora(attn):
        return None
    packs = [pack(m, dtype, device) for m in projections(attn)]
    if not kv:
        packs[1] = packs[2] = None
    if all(p is None for p in packs):
        return None
    key = (cross,) + tuple(None if p is None else p.key for p in packs)
    ent = _ARGS_CACHE.get(attn)
    if ent is not None and ent[0] == key:
        return ent[1]
    pq, pk, pv, po = packs
    ranks = tuple(0 if p is None else p.rank for p in packs)
    x_parts = [p.a for p in ((pq,) if cross else (pq, pk, pv)) if p is not None]
    ctx_parts = [p.a for p in (pk, pv) if p is not None] if cross else []
    with torch.no_grad():
        down_x = torch.cat(x_parts, 0).contiguous() if x_parts else None
        down_ctx = torch.cat(ctx_parts, 0).contiguous() if ctx_parts else None
    from . import processors
    processors._CACHE_GEN[0] += 1
    la = LoraArgs(down_x, down_ctx, None if po is None else po.a, tuple(None if p is None else p.b for p in packs), ranks, key,
                  tuple(None if p is None else p.gain for p in packs))
    _ARGS_CACHE[attn] = (key, la)
    return la


def kv_packs(attn, dtype: torch.dtype, device: torch.device) -> Tuple[Optional[LoraPack], Optional[LoraPack]]:
    """The k / v packs of ``attn`` (None, None without LoRA): the text-K/V cache projects with them and keys on them."""
    if not any_lora(attn):
        return None, None
    _, mk, mv, _ = projections(attn)
    return pack(mk, dtype, device), pack(mv, dtype, device)


def clear() -> None:
    _PACK_CACHE.clear()
    _ARGS_CACHE.clear()
