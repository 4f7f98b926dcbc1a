"""Host-side preparation of an interpolation sequence: Beta-scheduled coefficients and the
latent / embedding initialisation.  Same names, arguments and behaviour as the reference
(prior.py:481-502, interpolation.py:807-918).  These run once per sequence on small tensors
and are not kernel targets."""
from __future__ import annotations

from typing import Optional

import torch
from torch import FloatTensor


def generate_beta_tensor(size: int, alpha: float = 3, beta: float = 3) -> torch.FloatTensor:
    """[x_0 .. x_{n-1}] with F(x_i) = i/(n-1) for the Beta(alpha, beta) CDF F (prior.py:481-502)."""
    from scipy.stats import beta as beta_distribution
    prob_values = [i / (size - 1) for i in range(size)]
    return torch.tensor(beta_distribution.ppf(prob_values, alpha, beta), dtype=torch.float32)


def linear_interpolation(l1: FloatTensor, l2: FloatTensor, ts: Optional[FloatTensor] = None,
                         size: int = 5) -> FloatTensor:
    """(size, *) linear interpolation between (1, *) tensors (interpolation.py:807-835)."""
    assert l1.shape == l2.shape, "shapes of l1 and l2 must match"
    if ts is None:
        ts = [i / (size - 1) for i in range(size)]
    return torch.cat([torch.lerp(l1, l2, t) for t in ts], dim=0)


def spherical_interpolation(l1: FloatTensor, l2: FloatTensor, size=5) -> FloatTensor:
    """(size, *) spherical interpolation between (1, *) tensors (interpolation.py:838-858)."""
    assert l1.shape == l2.shape, "shapes of l1 and l2 must match"
    return torch.cat([slerp(l1, l2, i / (size - 1)) for i in range(size)], dim=0)


def slerp(v0: FloatTensor, v1: FloatTensor, t, threshold=0.9995):
    """Row-wise (last dim) spherical linear interpolation with a lerp fallback for rows that are
    (anti-)colinear (|cos| > threshold) or contain a zero vector (NaN cosine)
    (interpolation.py:861-918)."""
    assert v0.shape == v1.shape, "shapes of v0 and v1 must match"
    n0 = torch.norm(v0, dim=-1, keepdim=True)
    n1 = torch.norm(v1, dim=-1, keepdim=True)
    dot = ((v0 / n0) * (v1 / n1)).sum(-1)
    mag = dot.abs()
    gotta_lerp = mag.isnan() | (mag > threshold)
    lerped = torch.lerp(v0, v1, t)
    theta_0 = dot.arccos().unsqueeze(-1)
    sin_theta_0 = theta_0.sin()
    theta_t = theta_0 * t
    s0 = (theta_0 - theta_t).sin() / sin_theta_0
    s1 = theta_t.sin() / sin_theta_0
    slerped = s0 * v0 + s1 * v1
    return torch.where(gotta_lerp.unsqueeze(-1), lerped, slerped)


# ---- corner-weighted sequences (build-specific) ------------------------------------------------------------------
def grid_weights(rows: int, cols: int) -> torch.FloatTensor:
    """Bilinear weights of a ``rows`` x ``cols`` grid of frames (row-major) over four corners ordered top-left, top-right,
    bottom-left, bottom-right: ``[rows * cols, 4]``, every row sums to 1.  A grid of one row (column) sits on the top (left) edge."""
    if rows < 1 or cols < 1:
        raise ValueError("grid_weights needs rows >= 1 and cols >= 1")
    out = torch.zeros(rows * cols, 4, dtype=torch.float64)
    for r in range(rows):
        v = r / (rows - 1) if rows > 1 else 0.0
        for c in range(cols):
            u = c / (cols - 1) if cols > 1 else 0.0
            out[r * cols + c] = torch.tensor([(1 - v) * (1 - u), (1 - v) * u, v * (1 - u), v * u], dtype=torch.float64)
    return out.to(torch.float32)


def simplex_weights(m: int, steps: int) -> torch.FloatTensor:
    """The lattice points of the (m - 1)-simplex with ``steps`` divisions per edge — all non-negative integer vectors of sum
    ``steps``, divided by ``steps`` — as weight rows ``[C(steps + m - 1, m - 1), m]``, corners included (the one-hot rows), ordered
    with the first corner's weight descending, then the second's, ..."""
    if m < 1 or steps < 1:
        raise ValueError("simplex_weights needs m >= 1 and steps >= 1")

    def compositions(total: int, parts: int):
        if parts == 1:
            yield (total,)
            return
        for first in range(total, -1, -1):
            for rest in compositions(total - first, parts - 1):
                yield (first,) + rest
    return (torch.tensor(list(compositions(steps, m)), dtype=torch.float64) / steps).to(torch.float32)


def nested_slerp(xs, w) -> FloatTensor:
    """One frame's latent among M corner latents ``xs`` ((1, *) tensors) for its weight row ``w``: ``acc = x_0``; for m >= 1,
    ``acc = slerp(acc, x_m, w_m / (w_0 + ... + w_m))``, corners being skipped while the running sum is 0 (the first corner with a
    weight starts the chain).  ``slerp(x_0, x_1, c)`` for M = 2 and w = (1 - c, c); ``x`` when all corners are ``x``."""
    ws = [float(v) for v in (w.tolist() if torch.is_tensor(w) else w)]
    if len(ws) != len(xs) or not ws:
        raise ValueError("nested_slerp needs one weight per corner")
    acc, run = xs[0], ws[0]
    for x, wm in zip(xs[1:], ws[1:]):
        if run == 0.0:
            acc, run = x, wm
            continue
        run += wm
        if wm != 0.0:
            acc = slerp(acc, x, wm / run)
    return acc


def weight_rows_of(weights, m: int) -> torch.Tensor:
    """``weights`` as a float32 CPU tensor [N, m] after the row checks of a corner-weighted run: rows non-negative, finite and summing
    to 1 within 1e-6; anything else raises ``ValueError`` naming the row."""
    if weights is None:
        raise ValueError("pass weights [N, M]: one row of corner weights per frame (grid_weights / simplex_weights build common ones)")
    w = torch.as_tensor(weights, dtype=torch.float32).detach().cpu()
    if not 1 <= m <= 8:
        raise ValueError(f"a run interpolates among 1 .. 8 corners; got {m}")
    if w.ndim != 2 or w.shape[1] != m or w.shape[0] < 1:
        raise ValueError(f"weights must be [N, {m}] (one column per corner); got {tuple(w.shape)}")
    for i in range(w.shape[0]):
        row = w[i]
        if not bool(torch.isfinite(row).all()) or bool((row < 0).any()):
            raise ValueError(f"weights row {i} has a negative or non-finite entry: {row.tolist()}")
        if abs(float(row.to(torch.float64).sum()) - 1.0) > 1e-6:
            raise ValueError(f"weights row {i} sums to {float(row.to(torch.float64).sum())}, not 1: {row.tolist()}")
    return w


def corner_rows_of(weights, m: int):
    """Checks the weight matrix of a corner-weighted run over ``m`` corners and finds the corner frames: returns (``weights`` as a
    float32 CPU tensor [N, m], ``corner_rows``) with ``corner_rows[c]`` the first frame whose row is exactly one-hot at ``c``.  Rows must
    be non-negative and sum to 1 within 1e-6, and every corner needs such a frame; anything else raises ``ValueError`` naming the row
    (or the corner)."""
    w = weight_rows_of(weights, m)
    rows = []
    for c in range(m):
        hit = [i for i in range(w.shape[0]) if float(w[i, c]) == 1.0 and int((w[i] != 0).sum()) == 1]
        if not hit:
            raise ValueError(f"no frame's weights row is exactly one-hot at corner {c}: the corner frames sit in the batch, so every "
                             "corner needs a row with a single 1")
        rows.append(hit[0])
    return w, rows
