"""fp64 restatement of classifier-free guidance with guidance rescale (a plain module; include/aid_hip.h: aid_cfg_rescale).

Per sample i, over the e elements of the sample:

    c    = u + gs (t - u)                    t = text[i], u = uncond[i]
    s_t  = std(t),  s_c = std(c)             unbiased (divide by e - 1), as torch.std
    out  = c (phi s_t / s_c + (1 - phi))

evaluated in numpy float64 on the inputs AS STORED (rounded to their dtype already) and with the two scalars as the C ABI receives
them (C floats).  Written from the formula (arXiv 2305.08891 §3.4); nothing is rounded on the way.
"""
from __future__ import annotations

import numpy as np
import torch


def _np64(a) -> np.ndarray:
    if torch.is_tensor(a):
        return a.detach().to("cpu").double().numpy()
    return np.asarray(a, np.float64)


def cfg_rescale(text, uncond, gs: float, phi: float):
    """(out, s_t, s_c): out [n, ...] float64; the two spreads per sample [n]."""
    t, u = _np64(text), _np64(uncond)
    assert t.shape == u.shape and t.ndim >= 2
    gs, phi = float(np.float32(gs)), float(np.float32(phi))
    n = t.shape[0]
    tf, uf = t.reshape(n, -1), u.reshape(n, -1)
    c = uf + gs * (tf - uf)
    s_t, s_c = tf.std(axis=1, ddof=1), c.std(axis=1, ddof=1)
    out = c * (phi * s_t / s_c + (1.0 - phi))[:, None]
    return out.reshape(t.shape), s_t, s_c


def storage_ulp(ref: np.ndarray, dtype: torch.dtype) -> np.ndarray:
    """The spacing of ``dtype`` at |ref| (the subnormal spacing below the smallest normal number)."""
    mant, emin = {torch.float16: (10, -14), torch.bfloat16: (7, -126)}[dtype]
    a = np.abs(np.asarray(ref, np.float64))
    ex = np.floor(np.log2(np.maximum(a, 2.0 ** emin)))
    return 2.0 ** (ex - mant)


def element_bound(ref: np.ndarray, dtype: torch.dtype) -> np.ndarray:
    """What ONE rounding of an fp32 result to a 16-bit ``dtype`` may differ from ``ref`` by: half a unit in the last place relative —
    2^-11 |ref| (float16), 2^-8 |ref| (bfloat16) — plus one storage ulp of slack for the fp32 arithmetic in front of the rounding (its
    ~1e-6 relative error can move a result across a rounding boundary, never further)."""
    half = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}[dtype]
    return half * np.abs(ref) + storage_ulp(ref, dtype)
