"""Smoothness metrics of an interpolation sequence (reference ``utils.py:108-213``): neighbour distances under a perceptual
model, their Gini index, and the triple ``(1 - gini, mean, max)`` that ``bayesian_prior_selection`` maximises (prior.py).

The perceptual model is a component the caller passes in — ``lpips_model(img_a, img_b)`` on normalised NCHW frames, the call
the reference makes to ``lpips.LPIPS`` — exactly as ``BetaPriorPipeline`` takes its CLIP tower through ``model=``.
``adjacent_distances`` / ``smoothness_and_consistency_of`` (build-specific) serve runs whose frames are not images
(``output_type="latent"``, pipelines without a VAE) with a caller-supplied distance.

A handful of small torch ops once per evaluation; nothing here is a kernel target.
"""
from __future__ import annotations

from typing import Callable, Tuple

import numpy as np
import torch

LPIPS_MEAN = (0.485, 0.456, 0.406)
LPIPS_STD = (0.229, 0.224, 0.225)


def _host_vector(values) -> np.ndarray:
    """Distances as a float64 numpy vector, with ONE device-to-host transfer when they are device scalars."""
    values = list(values)
    if values and all(torch.is_tensor(v) for v in values):
        return torch.stack([v.detach().reshape(()) for v in values]).double().cpu().numpy()
    return np.array([float(v) for v in values], dtype=np.float64)


def compute_lpips(images, lpips_model) -> np.ndarray:
    """Perceptual distance of each neighbouring pair of ``images`` (N, H, W, C) -> numpy [N - 1] (utils.py:108-139).

    The frames go to the model's device as float, NCHW, normalised per channel with the ImageNet mean / std — on whatever range
    they come in, uint8 0 .. 255 included: the reference's arithmetic, kept.  The reference brings every pair's
    distance to the host on its own (``.item()``); here the whole vector crosses once."""
    ref = next(iter(lpips_model.parameters()), None) if hasattr(lpips_model, "parameters") else None
    device = ref.device if ref is not None else torch.device("cpu")
    x = (images if torch.is_tensor(images) else torch.as_tensor(np.asarray(images))).to(device).float()
    x = torch.permute(x, (0, 3, 1, 2))
    mean = torch.tensor(LPIPS_MEAN, dtype=x.dtype, device=device).view(1, -1, 1, 1)
    std = torch.tensor(LPIPS_STD, dtype=x.dtype, device=device).view(1, -1, 1, 1)
    x = (x - mean) / std
    with torch.no_grad():
        ds = [torch.as_tensor(lpips_model(x[i:i + 1], x[i + 1:i + 2])).reshape(-1)[0] for i in range(x.shape[0] - 1)]
    if not ds:
        return np.array([])
    return torch.stack(ds).cpu().numpy().astype(np.float64)      # (float32 values widened, as ``.item()`` widens them)


def compute_gini(distances) -> float:
    """Gini index of the distances, ``sum_ij |d_i - d_j| / (2 n^2 mean)``; 0.0 for fewer than two entries (utils.py:142-168).
    One outer difference of the sorted vector; the two sums run left to right in the vector's own precision (``cumsum``), so a
    float32 vector rounds where the reference's running sums round."""
    d = np.sort(np.asarray(distances))
    n = d.size
    if n < 2:
        return 0.0
    if d.dtype.kind != "f":
        d = d.astype(np.float64)
    spread = np.cumsum(np.abs(d[:, None] - d[None, :]).ravel())[-1]
    return spread / (2 * n * n * (np.cumsum(d)[-1] / n))


def smoothness_and_consistency_of(distances) -> Tuple[float, float, float]:
    """``(1 - gini, mean, max)`` of a vector of neighbour distances (utils.py:184-188)."""
    d = np.asarray(distances, dtype=np.float64)
    return 1 - compute_gini(d), np.mean(d), np.max(d)


def compute_smoothness_and_consistency(images, lpips_model) -> Tuple[float, float, float]:
    """``(smoothness, consistency, max_inception_distance)`` of ``images`` (N, H, W, C) (utils.py:171-188)."""
    return smoothness_and_consistency_of(compute_lpips(images, lpips_model))


def separate_source_and_interpolated_images(images) -> Tuple[np.ndarray, np.ndarray]:
    """``(source [2, ...], interpolation [N - 2, ...])``: first and last frame, and the rest (utils.py:191-212)."""
    if len(images) < 2:
        raise ValueError("The input array should have at least two elements.")
    return np.array([images[0], images[-1]]), images[1:-1]


def adjacent_distances(frames, distance: Callable) -> np.ndarray:
    """``distance(frames[i], frames[i + 1])`` for every neighbouring pair -> numpy [N - 1] (build-specific).  ``distance`` returns a
    0-dim tensor or a float; ``frames`` is anything indexable (a latent stack, a list of images).  Device scalars cross to the host
    in one transfer."""
    with torch.no_grad():
        return _host_vector(distance(frames[i], frames[i + 1]) for i in range(len(frames) - 1))
