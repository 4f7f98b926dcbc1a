"""The 8-bit block format of the key-frame store (``storage="q8"``, include/aid_hip.h) restated in numpy — a plain module, imported by
the q8 tests.

A block row of ``n`` elements (``n`` a positive multiple of 8) is ``block_bytes(n) = round_up(n + ceil(n / 32), 16)`` bytes: ``n`` int8,
one exponent byte per block of 32 consecutive elements, bytes up to the 16-byte boundary that nobody reads or writes (the restatement
leaves them 0).  Of a V^T block — rows of ``ld`` columns — only the first ``cols`` columns of every row are stored: a pad column's int8
is 0, it takes no part in its block's maximum and it comes back as +0, whatever it held (NaN included).

Per block: ``a`` = max |x| over the stored elements, ``e`` the smallest integer with 127 * 2^e >= a clamped to [-126, 120], exponent byte
``e + 127``, ``q = clamp(rne(x * 2^-e), -127, 127)``; the value that comes back is ``q * 2^e``, exact in f16, bf16 and f32.

Everything here is float64 / integer arithmetic on exact fp32 inputs: ``e`` comes from ``frexp`` and one exact compare, the product
``x * 2^-e`` is exact in float64, ``np.rint`` rounds half to even.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

E_MIN, E_MAX = -126, 120


def round_up(x: int, a: int) -> int:
    return (x + a - 1) // a * a


def n_blocks(n: int) -> int:
    return (n + 31) // 32


def stored_bytes(n: int) -> int:
    """Bytes of a block row that are read and written: the int8 elements and the exponent bytes."""
    return n + n_blocks(n)


def block_bytes(n: int) -> int:
    return 0 if n < 8 or n % 8 else round_up(stored_bytes(n), 16)


def _stored_mask(n: int, ld: Optional[int], cols: Optional[int]) -> np.ndarray:
    if ld is None:
        return np.ones(n, dtype=bool)
    assert ld % 8 == 0 and n % ld == 0 and 1 <= cols <= ld
    return (np.arange(n) % ld) < cols


def exponents(x: np.ndarray, ld: Optional[int] = None, cols: Optional[int] = None) -> np.ndarray:
    """int [ceil(n / 32)]: the exponent ``e`` of every block of the float32 vector ``x`` (pad columns masked out)."""
    x = np.asarray(x, dtype=np.float32).ravel()
    n = x.size
    xs = np.where(_stored_mask(n, ld, cols), x, np.float32(0))
    xs = np.concatenate([xs, np.zeros(n_blocks(n) * 32 - n, dtype=np.float32)]).reshape(-1, 32)
    a = np.abs(xs).max(axis=1).astype(np.float64)
    _, ex = np.frexp(a)                                   # a = m 2^ex, m in [0.5, 1)
    e0 = ex.astype(np.int64) - 7                          # 127 * 2^e0 = 1.984375 * 2^(ex - 1): the candidate below or at a's binade
    e = np.where(a > np.ldexp(127.0, np.clip(e0, -1000, 1000)), e0 + 1, e0)
    e = np.where(a == 0, E_MIN, e)
    return np.clip(e, E_MIN, E_MAX)


def quantise(x: np.ndarray, ld: Optional[int] = None, cols: Optional[int] = None) -> np.ndarray:
    """uint8 [block_bytes(n)]: the block row of the float32 vector ``x`` (trailing pad bytes 0)."""
    x = np.asarray(x, dtype=np.float32).ravel()
    n = x.size
    assert block_bytes(n) > 0, n
    e = exponents(x, ld, cols)
    xs = np.where(_stored_mask(n, ld, cols), x, np.float32(0)).astype(np.float64)
    scale = np.ldexp(1.0, -np.repeat(e, 32)[:n])
    q = np.clip(np.rint(xs * scale), -127, 127).astype(np.int8)
    out = np.zeros(block_bytes(n), dtype=np.uint8)
    out[:n] = q.view(np.uint8)
    out[n:n + n_blocks(n)] = (e + 127).astype(np.uint8)
    return out


def split(b: np.ndarray, n: int) -> Tuple[np.ndarray, np.ndarray]:
    """(q int [n], e int [ceil(n / 32)]) of a block row."""
    b = np.asarray(b, dtype=np.uint8).ravel()
    return b[:n].view(np.int8).astype(np.int64), b[n:n + n_blocks(n)].astype(np.int64) - 127


def dequantise(b: np.ndarray, n: int, ld: Optional[int] = None, cols: Optional[int] = None) -> np.ndarray:
    """float32 [n]: what GET writes for the block row ``b`` — q * 2^e (exact in float32), +0 in the pad columns."""
    q, e = split(b, n)
    y = np.ldexp(q.astype(np.float64), np.repeat(e, 32)[:n])
    y32 = y.astype(np.float32)
    assert np.array_equal(y32.astype(np.float64), y)
    return np.where(_stored_mask(n, ld, cols), y32, np.float32(0))


# ---- torch front ends (bf16 has no numpy type: the values travel as exact float32) -------------------------------------------------
def quantise_t(t: torch.Tensor, ld: Optional[int] = None, cols: Optional[int] = None) -> torch.Tensor:
    """uint8 [block_bytes(t.numel())] (CPU) of a tensor of any of the three storage dtypes."""
    return torch.from_numpy(quantise(t.detach().float().cpu().numpy().ravel(), ld, cols))


def dequantise_t(b: torch.Tensor, n: int, dtype: torch.dtype, ld: Optional[int] = None, cols: Optional[int] = None) -> torch.Tensor:
    """[n] of ``dtype`` (CPU); the conversion is exact, and checked to be."""
    y = torch.from_numpy(dequantise(b.detach().cpu().numpy(), n, ld, cols))
    out = y.to(dtype)
    assert torch.equal(out.float(), y), "q * 2^e is not representable in the storage dtype"
    return out


def roundtrip_t(t: torch.Tensor, ld: Optional[int] = None, cols: Optional[int] = None) -> torch.Tensor:
    """dequantise(quantise(t)) in t's dtype and shape (CPU), pad columns +0."""
    return dequantise_t(quantise_t(t, ld, cols), t.numel(), t.dtype, ld, cols).reshape(t.shape)
