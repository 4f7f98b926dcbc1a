"""Attention-mask patterns with fully masked 64-key tiles, shared by the CPU test of the oracle (tests/test_oracle_attn_mask.py) and
the GPU tests of the score-bias kernels (tests/test_hip_attn_mask_range.py).

Shape: N = 4 frames (frame 3 rides PLAIN inside INNER / OUTER launches), S = 40 query rows (one whole 32-row block and a ragged one),
L = 150 keys (two whole 64-key tiles and a ragged one of 22), H = 2 heads.  ``keep`` is True where a key is live."""
import numpy as np
import torch

from oracle import aid_oracle as O

N, S, L, H = 4, 40, 150, 2
COEF = [0.0, 0.35, 1.0, -1.0]                   # frame 3 = PLAIN rider
MODES = ("plain", "inner", "outer")
PATTERNS = "ABCDEFG"
VALUES = ("m10000", "finfo_min", "neg_inf")


def keep_of(pattern: str) -> torch.Tensor:
    """bool [N, 1, L] (the same for every query row) or [N, S, L] (per row)."""
    key = torch.arange(L)
    if pattern == "A":                          # the first tile fully masked
        keep = key >= 64
    elif pattern == "B":                        # only the ragged tile is live
        keep = key >= 128
    elif pattern == "C":                        # a fully masked middle tile after a live one
        keep = (key < 64) | (key >= 128)
    elif pattern == "D":                        # tile 1 partly masked, the ragged tile fully masked
        keep = key < 70
    elif pattern == "F":                        # one live key, the last
        keep = key == L - 1
    elif pattern in "EG":                       # row r masks keys < (37 r) % 150: inside one wave's 32 rows a fully masked first
        row = torch.arange(S)                   # tile, a partly masked one and an untouched one
        keep = key[None, :] >= ((37 * row) % L)[:, None]
        if pattern == "G":
            keep[::5] = False                   # every fifth row has no live key at all
        return keep[None].expand(N, S, L).clone()
    else:
        raise ValueError(pattern)
    return keep[None, None].expand(N, 1, L).clone()


# fully masked query rows per frame that each pattern is meant to have
DEAD_ROWS = {"A": 0, "B": 0, "C": 0, "D": 0, "E": 0, "F": 0, "G": 8}


def low_of(value: str, dtype: torch.dtype) -> float:
    return {"m10000": -10000.0, "finfo_min": torch.finfo(dtype).min, "neg_inf": float("-inf")}[value]


def additive(keep: torch.Tensor, value: str, dtype: torch.dtype) -> torch.Tensor:
    """The additive mask a caller hands over: 0 on live keys, the mask value elsewhere."""
    m = torch.zeros(keep.shape, dtype=dtype)
    m[~keep] = low_of(value, dtype)
    return m


def oracle_mask(keep: torch.Tensor, value: str) -> np.ndarray:
    """What the fp64 oracle gets for the same mask, [N, 1, R, L]: -10000 as it stands, finfo.min and -inf as -1e30 (weight exactly 0
    next to a live key, like tests/test_hip_parity.py::test_attention_core_with_score_bias)."""
    low = -10000.0 if value == "m10000" else -1e30
    return np.where(keep.numpy(), 0.0, low)[:, None]


def live_rows(keep: torch.Tensor) -> np.ndarray:
    """bool [N, S]: the query row has at least one live key."""
    return np.broadcast_to(keep.any(dim=-1).numpy(), (N, S)).copy()


def oracle_out(q64, k64, v64, d: int, mode: str, m64: np.ndarray) -> np.ndarray:
    """fp64 oracle output [N, S, H d] of the launch the GPU tests make: frames 0 .. 2 interpolate between 0 and 2 (pure INNER / OUTER),
    frame 3 rides PLAIN; ``mode == "plain"`` runs every frame PLAIN."""
    if mode == "plain":
        return O.attn_core(q64, k64, v64, H, d ** -0.5, "plain", False, None, mask=m64)
    coef = np.asarray(COEF[:3], np.float64)
    ref = np.empty((N, S, H * d))
    ref[:3] = O.attn_core(q64[:3], k64[:3], v64[:3], H, d ** -0.5, mode, False, coef, mask=m64[:3])
    ref[3:] = O.attn_core(q64[3:], k64[3:], v64[3:], H, d ** -0.5, "plain", False, None, mask=m64[3:])
    return ref
