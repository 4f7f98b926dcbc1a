"""Inputs for the tests of the IP-Adapter segment kernel (aid_ip_attn_kernel, csrc/aid_attn_ip.hip), shared by the CPU test of the
cases themselves (tests/test_ip_segment_cases.py) and the GPU tests (tests/test_hip_ip_segments.py).

``score_case`` draws q, k, v ~ N(0, 1) and, for every kind but "random", overwrites channel 0 of every head: query row r gets
b_r = linspace(-3, 3, s)[r], key j gets a_j, so the score of (row r, key j) gains a_j b_r / sqrt(d):

    "random"  channel 0 left as drawn                 baseline
    "steps"   a_j = 12 sqrt(d) (j // 32)              rows with b > 0 raise their maximum at every 32-key score tile of the kernel (the
                                                      rescale alpha = exp2((m_old - m_new) c2) gets as small as e^-36), rows with
                                                      b < 0 have it in the first tile; one 32-row wave tile holds both signs
    "ramp"    a_j = 0.25 sqrt(d) j                    the maximum moves a little at every tile and earlier tiles keep a measurable weight
                                                      (about 4 effective keys): a lost rescale of the row sum is a wrong number
    "level"   a_j = 20 sqrt(d)                        the whole row is shifted by 20 b_r (-60 .. +60 nat); the softmax does not change

The largest |k| is 12 sqrt(160) 8 = 1214 (t = 257), so float16 holds every case.

``emulate`` restates the kernel's arithmetic in torch on the CPU: fp32 scores, a running maximum over 32-key tiles, P = exp2((s - m) c2)
rounded to the storage type, the row sum over the ROUNDED P, fp32 accumulation with the alpha rescale, one rounding of the result.
Against ``ip_multi_ref.attention`` (fp64 on the same rounded inputs) at s = 160, two frames, two heads, the largest figure over
d = 40 / 64 / 80 / 160 and t = 33 / 70 / 257 is (tests/test_ip_segment_cases.py prints them; bounds TOL 1e-3 / 8e-3, WORST 4e-2 / 0.25):

                 fp16 rel-L2 / worst     bf16 rel-L2 / worst
    "random"     2.69e-4 / 3.86e-3       2.16e-3 / 2.38e-2
    "steps"      2.41e-4 / 2.55e-3       1.92e-3 / 2.06e-2
    "ramp"       2.29e-4 / 2.16e-3       1.86e-3 / 1.88e-2
    "level"      2.68e-4 / 2.60e-3       2.17e-3 / 2.06e-2

At s = 160, t = 70 about 75 rows per (frame, head) raise their tile maximum at every tile and about 78 lower it ("steps" and "ramp";
at t = 257 the same over the eight whole tiles of "ramp", whose 0.25 b step does not lift a last tile of one key over the 32 before it).
"""
import math

import numpy as np
import torch

KINDS = ("random", "steps", "ramp", "level")
KEY_COUNTS = list(range(1, 73)) + [95, 96, 97, 127, 128, 129, 257]
ROW_COUNTS = [1, 31, 32, 33, 127, 128, 129, 160, 257, 300]
LOG2E = 1.4426950408889634


def round_up(x: int, a: int) -> int:
    return (x + a - 1) // a * a


def row_levels(s: int) -> torch.Tensor:
    """b_r of the query rows, float32 [s]."""
    return torch.linspace(-3.0, 3.0, s)


def key_levels(kind: str, d: int, t: int) -> torch.Tensor:
    j = torch.arange(t, dtype=torch.float32)
    if kind == "steps":
        return 12.0 * math.sqrt(d) * torch.div(j, 32, rounding_mode="floor")
    if kind == "ramp":
        return 0.25 * math.sqrt(d) * j
    if kind == "level":
        return torch.full((t,), 20.0 * math.sqrt(d))
    raise ValueError(kind)


def pack_vt(v: torch.Tensor) -> torch.Tensor:
    """V^T [r, c, round_up(t, 8)] of v [r, t, c] with NaN in the pad columns."""
    r, t, c = v.shape
    vt = torch.full((r, c, round_up(t, 8)), float("nan"), dtype=v.dtype)
    vt[:, :, :t] = v.transpose(1, 2)
    return vt


def score_case(kind: str, dtype: torch.dtype, d: int, n: int, s: int, t: int, heads: int, seed: int):
    """(q [n, s, heads d], k [n, t, heads d], v [n, t, heads d], vt [n, heads d, round_up(t, 8)]) on the CPU, rounded to ``dtype``."""
    g = torch.Generator().manual_seed(seed)
    c = heads * d
    q, k, v = (torch.randn(n, rows, c, generator=g) for rows in (s, t, t))
    if kind != "random":
        q.view(n, s, heads, d)[..., 0] = row_levels(s)[None, :, None]
        k.view(n, t, heads, d)[..., 0] = key_levels(kind, d, t)[None, :, None]
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    return q, k, v, pack_vt(v)


def tile_maxima(q: torch.Tensor, k: torch.Tensor, heads: int) -> np.ndarray:
    """fp64 maxima of the scaled scores over every 32-key tile: [n, heads, s, ceil(t / 32)]."""
    n, s, c = q.shape
    t, d = k.shape[1], c // heads
    qh = q.double().view(n, s, heads, d).permute(0, 2, 1, 3)
    kh = k.double().view(n, t, heads, d).permute(0, 2, 3, 1)
    sc = (qh @ kh) / math.sqrt(d)
    return np.stack([sc[..., j:j + 32].amax(-1).numpy() for j in range(0, t, 32)], axis=-1)


def emulate(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, dtype: torch.dtype, c2=None, rounded=True) -> torch.Tensor:
    """softmax(q k^T / sqrt(d)) v as the kernel computes it (see the module docstring); q [n, s, c], k / v [n, t, c] -> [n, s, c].
    ``c2``: the kernel's exponent factor when it is not d^-0.5 log2(e); ``rounded=False`` returns the fp32 block before the rounding."""
    n, s, c = q.shape
    t, d = k.shape[1], c // heads
    c2 = float(np.float32(np.float32(d ** -0.5) * np.float32(LOG2E))) if c2 is None else float(np.float32(c2))
    qh = q.float().view(n, s, heads, d).permute(0, 2, 1, 3)
    kh = k.float().view(n, t, heads, d).permute(0, 2, 1, 3)
    vh = v.float().view(n, t, heads, d).permute(0, 2, 1, 3)
    sc = qh @ kh.transpose(2, 3)                                               # fp32, unscaled: c2 enters inside the exp2
    mx = torch.full((n, heads, s, 1), float("-inf"))
    ls = torch.zeros(n, heads, s, 1)
    oc = torch.zeros(n, heads, s, d)
    for j in range(0, t, 32):
        tile = sc[..., j:j + 32]
        mn = torch.maximum(mx, tile.amax(-1, keepdim=True))
        alpha = torch.exp2((mx - mn) * c2)                                      # first tile: exp2(-inf) = 0 on zeros
        oc, ls, mx = oc * alpha, ls * alpha, mn
        nm = -mx * c2
        e = (tile.double() * c2 + nm.double()).float()                          # one rounding, like v_fma_f32
        p = torch.exp2(e).to(dtype).float()
        ls = ls + p.sum(-1, keepdim=True)
        oc = oc + p @ vh[:, :, j:j + 32]
    o = (oc * (1.0 / ls)).permute(0, 2, 1, 3).reshape(n, s, c)
    return o.to(dtype) if rounded else o
