"""A test double of PEFT's DoRA ``lora.Linear`` (``use_dora=True``), restated from PEFT's published behaviour on top of
tests/peft_double.py: peft is absent from the build image and the GPU box.  What is added to the plain double:

  * ``lora_magnitude_vector`` (a ModuleDict of modules with a ``weight`` of shape [out]) and ``use_dora[adapter] = True``;
  * the DoRA forward in eval mode: ``weight_norm = ||W + s B A||_row`` (detached, no epsilon), ``g = magnitude / weight_norm``,
    ``result = base(x) + (g - 1) * (base(x) - bias) + g * lora_B(lora_A(x)) * s``;
  * ``merge`` writes ``round(g o (W + s B A))`` into the base weight and remembers g, ``unmerge`` divides by it and subtracts the delta.

The magnitude is NOT PEFT's initial value (the row norm itself, which makes g = 1 and would hide a dropped gain): it is the row norm
times U(0.5, 1.5)."""
from __future__ import annotations

from typing import Dict, Iterable, Tuple

import torch
from torch import nn

from peft_double import LoraLinear


class _Magnitude(nn.Module):
    def __init__(self, weight: torch.Tensor):
        super().__init__()
        self.weight = nn.Parameter(weight, requires_grad=False)


class DoraLinear(LoraLinear):
    def __init__(self, base: nn.Linear):
        super().__init__(base)
        self.lora_magnitude_vector = nn.ModuleDict()
        self.fan_in_fan_out = False
        self._dora_factor: Dict[str, torch.Tensor] = {}

    def _wide(self, t: torch.Tensor) -> torch.Tensor:
        """fp32 for 16-bit storage, the storage type otherwise (the arithmetic type of the double)."""
        return t.detach().to(torch.promote_types(t.dtype, torch.float32))

    def _weight_norm(self, a: str) -> torch.Tensor:
        w = self.base_layer.weight
        delta = (self._wide(self.lora_B[a].weight) @ self._wide(self.lora_A[a].weight)) * self.scaling[a]
        return torch.linalg.norm(self._wide(w) + delta, dim=1).to(w.dtype)

    def get_delta_weight(self, a: str) -> torch.Tensor:
        wa, wb = self.lora_A[a].weight, self.lora_B[a].weight
        return ((self._wide(wb) @ self._wide(wa)) * self.scaling[a]).to(wa.dtype)

    def update_layer(self, name: str, r: int, lora_alpha: float, dropout: float = 0.0, generator=None, use_dora: bool = True):
        super().update_layer(name, r, lora_alpha, dropout, generator)
        if use_dora:
            self.use_dora[name] = True
            w = self.base_layer.weight
            jitter = 0.5 + torch.rand(w.shape[0], generator=generator)
            self.lora_magnitude_vector[name] = _Magnitude((self._wide(self._weight_norm(name)).cpu() * jitter).to(w.dtype).to(w.device))

    def merge(self, adapter_names: Iterable[str] = None) -> None:
        for a in (adapter_names or self.active_adapters):
            if a not in self.lora_A or a in self.merged_adapters:
                continue
            if not self.use_dora.get(a, False):
                super().merge([a])
                continue
            w = self.base_layer.weight
            g = self._wide(self.lora_magnitude_vector[a].weight) / self._wide(self._weight_norm(a))
            self._dora_factor[a] = g
            w.data.copy_((g.view(-1, 1) * (self._wide(w.data) + self._wide(self.get_delta_weight(a)))).to(w.dtype))
            self.merged_adapters.append(a)

    def unmerge(self) -> None:
        while self.merged_adapters:
            a = self.merged_adapters.pop()
            w = self.base_layer.weight
            if a in self._dora_factor:
                g = self._dora_factor.pop(a)
                w.data.copy_((self._wide(w.data) / g.view(-1, 1) - self._wide(self.get_delta_weight(a))).to(w.dtype))
            else:
                w.data -= self.get_delta_weight(a)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.disable_adapters or self.merged:
            return super().forward(x)
        result = self.base_layer(x)
        dt = result.dtype
        for a in self.active_adapters:
            if a not in self.lora_A:
                continue
            xa = x.to(self.lora_A[a].weight.dtype)
            low = self.lora_B[a](self.lora_A[a](self.lora_dropout[a](xa)))
            if not self.use_dora.get(a, False):
                result = result + low * self.scaling[a]
                continue
            g = (self.lora_magnitude_vector[a].weight / self._weight_norm(a)).view(1, -1)
            bias = self.base_layer.bias
            base_wo_bias = result if bias is None else result - bias
            result = result + (g - 1) * base_wo_bias + g * low * self.scaling[a]
        return result.to(dt)


def wrap_attention_dora(attn, adapters: Dict[str, Tuple[int, float]], targets=("to_q", "to_k", "to_v", "to_out"), seed: int = 0):
    """Like peft_double.wrap_attention with DoRA adapters; returns {target: DoraLinear}."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for t in targets:
        base = attn.to_out[0] if t == "to_out" else getattr(attn, t)
        lin = DoraLinear(base)
        for name, (r, alpha) in adapters.items():
            lin.update_layer(name, r, alpha, generator=g)
        lin.set_adapter(list(adapters))
        if t == "to_out":
            attn.to_out[0] = lin
        else:
            setattr(attn, t, lin)
        out[t] = lin
    return out


def effective_weight_dora(mod) -> torch.Tensor:
    """fp64 g64 o (W + s B A) of a DoRA wrapper with one active adapter, g64 = magnitude / ||W + s B A||_row, everything from the
    dtype-rounded factors; the plain effective weight for anything else (a plain layer, a disabled / merged wrapper, plain LoRA)."""
    from peft_double import effective_weight
    w = effective_weight(mod)
    if not hasattr(mod, "lora_magnitude_vector") or mod.disable_adapters or mod.merged:
        return w
    acts = [a for a in mod.active_adapters if a in mod.lora_A]
    if len(acts) != 1 or not mod.use_dora.get(acts[0], False):
        return w
    mag = mod.lora_magnitude_vector[acts[0]].weight.detach().double().cpu()
    return (mag / torch.linalg.norm(w, dim=1)).view(-1, 1) * w
