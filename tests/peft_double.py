"""A test double of PEFT's ``lora.Linear`` (what diffusers' PEFT backend wraps attn.to_q / to_k / to_v / to_out[0] in), restated
from PEFT's published behaviour, like tests/diffusers_double.py restates diffusers: peft is absent from the build image and the GPU
box.  What is restated is what the processors can get wrong:

  * the attribute protocol: ``base_layer``, ``lora_A`` / ``lora_B`` / ``lora_dropout`` (ModuleDicts keyed by adapter name),
    ``scaling`` (dict), ``active_adapters``, ``disable_adapters``, ``merged``, ``use_dora``, ``lora_bias``;
  * ``weight`` / ``bias`` return the BASE layer's tensors (so a processor that reads weights by pointer silently drops the adapters);
  * the forward decision table: disabled -> base (a merged layer is unmerged first); merged -> base; otherwise
    ``base(x) + sum_active lora_B(lora_A(dropout(x))) * scaling[a]``;
  * ``merge`` / ``unmerge`` (in-place edits of ``base_layer.weight.data``), ``set_adapter``, ``set_scale``, ``scale_layer`` /
    ``unscale_layer``."""
from __future__ import annotations

from typing import Dict, Iterable, Sequence, Tuple, Union

import torch
from torch import nn


class LoraLinear(nn.Module):
    def __init__(self, base: nn.Linear):
        super().__init__()
        self.base_layer = base
        self.lora_A = nn.ModuleDict()
        self.lora_B = nn.ModuleDict()
        self.lora_dropout = nn.ModuleDict()
        self.scaling: Dict[str, float] = {}
        self.r: Dict[str, int] = {}
        self.lora_alpha: Dict[str, float] = {}
        self.use_dora: Dict[str, bool] = {}
        self.lora_bias: Dict[str, bool] = {}
        self._active_adapter: Union[str, Sequence[str]] = "default"
        self._disable_adapters = False
        self.merged_adapters = []

    # ---- protocol ---------------------------------------------------------------------------------
    @property
    def weight(self) -> torch.Tensor:
        return self.base_layer.weight

    @property
    def bias(self):
        return self.base_layer.bias

    @property
    def merged(self) -> bool:
        return bool(self.merged_adapters)

    @property
    def disable_adapters(self) -> bool:
        return self._disable_adapters

    @property
    def active_adapters(self):
        return [self._active_adapter] if isinstance(self._active_adapter, str) else list(self._active_adapter)

    def update_layer(self, name: str, r: int, lora_alpha: float, dropout: float = 0.0, generator=None):
        w = self.base_layer.weight
        kw = dict(dtype=w.dtype, device=w.device)
        self.lora_A[name] = nn.Linear(w.shape[1], r, bias=False, **kw)
        self.lora_B[name] = nn.Linear(r, w.shape[0], bias=False, **kw)
        with torch.no_grad():       # lora_B is zero at PEFT's init; random here so that the adapter shows
            self.lora_A[name].weight.copy_(torch.randn(r, w.shape[1], generator=generator) / w.shape[1] ** 0.5)
            self.lora_B[name].weight.copy_(torch.randn(w.shape[0], r, generator=generator) / r ** 0.5)
        self.lora_dropout[name] = nn.Dropout(dropout) if dropout > 0 else nn.Identity()
        self.r[name], self.lora_alpha[name] = r, lora_alpha
        self.scaling[name] = lora_alpha / r
        self.use_dora[name] = False
        self.lora_bias[name] = False

    def set_adapter(self, names: Union[str, Sequence[str]]) -> None:
        self._active_adapter = names

    def enable_adapters(self, enabled: bool) -> None:
        self._disable_adapters = not enabled

    def set_scale(self, adapter: str, scale: float) -> None:
        self.scaling[adapter] = scale * self.lora_alpha[adapter] / self.r[adapter]

    def scale_layer(self, scale: float) -> None:
        for a in self.active_adapters:
            if a in self.lora_A:
                self.scaling[a] *= scale

    def unscale_layer(self, scale=None) -> None:
        for a in self.active_adapters:
            if a not in self.lora_A:
                continue
            if scale is None:
                self.scaling[a] = self.lora_alpha[a] / self.r[a]
            else:
                self.scaling[a] /= scale

    def get_delta_weight(self, a: str) -> torch.Tensor:
        wa, wb = self.lora_A[a].weight, self.lora_B[a].weight
        return ((wb.float() @ wa.float()) * self.scaling[a]).to(wa.dtype)

    def merge(self, adapter_names: Iterable[str] = None) -> None:
        for a in (adapter_names or self.active_adapters):
            if a in self.lora_A and a not in self.merged_adapters:
                self.base_layer.weight.data += self.get_delta_weight(a)
                self.merged_adapters.append(a)

    def unmerge(self) -> None:
        while self.merged_adapters:
            a = self.merged_adapters.pop()
            self.base_layer.weight.data -= self.get_delta_weight(a)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.disable_adapters:
            if self.merged:
                self.unmerge()
            return self.base_layer(x)
        if self.merged:
            return self.base_layer(x)
        result = self.base_layer(x)
        dt = result.dtype
        for a in self.active_adapters:
            if a not in self.lora_A:
                continue
            xa = x.to(self.lora_A[a].weight.dtype)
            result = result + self.lora_B[a](self.lora_A[a](self.lora_dropout[a](xa))) * self.scaling[a]
        return result.to(dt)


def wrap_attention(attn, adapters: Dict[str, Tuple[int, float]], targets=("to_q", "to_k", "to_v", "to_out"), seed: int = 0,
                   active=None):
    """Wrap the projections of a diffusers-style attention module the way ``load_lora_weights`` does: ``adapters`` maps name ->
    (rank, alpha); ``targets`` names the projections (to_out = to_out[0]).  Returns {target: LoraLinear}."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for t in targets:
        base = attn.to_out[0] if t == "to_out" else getattr(attn, t)
        lin = LoraLinear(base)
        for name, (r, alpha) in adapters.items():
            lin.update_layer(name, r, alpha, generator=g)
        lin.set_adapter(list(adapters) if active is None else active)
        if t == "to_out":
            attn.to_out[0] = lin
        else:
            setattr(attn, t, lin)
        out[t] = lin
    return out


def effective_weight(mod) -> torch.Tensor:
    """fp64 W + sum_active scaling * B A of a wrapper (or a plain layer's weight), from the dtype-rounded factors."""
    if not hasattr(mod, "lora_A"):
        return mod.weight.detach().double().cpu()
    w = mod.base_layer.weight.detach().double().cpu()
    if mod.disable_adapters or mod.merged:
        return w
    for a in mod.active_adapters:
        if a in mod.lora_A:
            w = w + mod.scaling[a] * (mod.lora_B[a].weight.detach().double().cpu() @ mod.lora_A[a].weight.detach().double().cpu())
    return w
