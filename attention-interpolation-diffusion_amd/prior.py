"""Beta-prior exploration of the interpolation path (reference ``prior.py:35-340``).

The reference's ``BetaPriorPipeline`` grows a set of interpolation coefficients ``xs`` one at a time: it takes the widest
perceptual gap (CLIP cosine distance between neighbouring frames), places the next coefficient at the Beta-CDF midpoint
of that gap, renders it with a batch-3 ``interpolate_single`` run, and refits Beta(alpha, beta) to the cumulative
distances.  Here the same search runs over a *generator callback* — ``generate(ts) -> (frames, features)`` renders the
frames at the coefficients ``ts`` (one N-frame AID run over ``[0, *ts, 1]`` on the HIP path: the processors take any
coefficient vector) — so it does not depend on diffusers / CLIP being importable, and with ``batch > 1`` several gaps are
filled per run instead of one batch-3 run per point.  With ``batch = 1`` the sequence of coefficients, distances and
fitted parameters is the reference's (pinned against the reference in ``tests/test_prior.py``).

``bayesian_prior_selection`` (prior.py:343-478) chooses the Beta prior itself: a Gaussian-process search over (alpha, beta) for the
smoothest sequence, every evaluation a replay between end points recorded once.

Host-side logic only (numpy / scipy); nothing here touches the GPU.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch
from scipy.optimize import curve_fit
from scipy.stats import beta as beta_distribution

from .interp import generate_beta_tensor
from .metrics import adjacent_distances, compute_gini, compute_lpips, smoothness_and_consistency_of


def clip_distance(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """1 - cosine similarity of two [1, D] feature rows (prior.py:18-22)."""
    return 1 - torch.nn.functional.cosine_similarity(a, b)[0]


def update_alpha_beta(xs: Sequence[float], ds: Sequence[float]) -> Tuple[float, float]:
    """Beta(alpha, beta) whose CDF, sampled at the explored coefficients ``xs``, follows the share of the total perceptual
    distance covered up to each of them (prior.py:35-56): least squares from (1, 1), both parameters kept positive."""
    total = sum(ds)
    # accumulated in the precision of the distances themselves (fp32 CLIP distances in the reference's runs): the fitted
    # parameters move at the 1e-7 level with the rounding of these targets, and the goldens pin them
    share = np.asarray(np.cumsum([0] + [d / total for d in ds]))
    fit, _ = curve_fit(beta_distribution.cdf, np.asarray(xs), share, p0=[1.0, 1.0],
                       bounds=([1e-6, 1e-6], [np.inf, np.inf]))
    return fit[0], fit[1]


def next_point(xs: Sequence[float], ds: Sequence[float], alpha: float, beta_param: float,
               uniform: bool = False, rank: int = 0) -> Tuple[int, float]:
    """(segment index, coefficient) of the next point (prior.py:74-90).  ``rank`` > 0 selects the rank-th widest gap
    (batched exploration); rank 0 is the reference's choice."""
    order = np.argsort(-np.asarray([float(d) for d in ds]), kind="stable")
    idx = int(np.argmax(ds)) if rank == 0 else int(order[rank])
    f_a = beta_distribution.cdf(xs[idx], alpha, beta_param)
    f_b = beta_distribution.cdf(xs[idx + 1], alpha, beta_param)
    t = beta_distribution.ppf((f_a + f_b) / 2, alpha, beta_param)
    if uniform:                                                   # the reference's uniform variant (:86-88), quirk kept
        if rank == 0:
            idx = int(np.argmax(np.array(xs) - np.array([0] + list(xs[:-1])))) - 1
        t = (xs[idx] + xs[idx + 1]) / 2
    return idx, float(t)


def extract_uniform_points(ds: Sequence[float], interpolation_size: int) -> List[int]:
    """Frames at (roughly) equal arc length: walk the gaps and emit the gap index every time the distance accumulated since
    the last emitted frame reaches total / (size - 1) (prior.py:201-210; the reference emits the index of the GAP, quirk kept)."""
    quota = sum(ds) / (interpolation_size - 1)
    picks, walked = [0], 0
    for gap, length in enumerate(ds):
        walked += length
        if walked >= quota:
            picks.append(gap)
            walked = 0
    return picks


# ---- smoothest path through the explored frames (prior.py:212-297) ----------------------------------------------------------
# Task: among the increasing node sequences 0 = p_0 < ... < p_{n-1} = m - 1 pick one whose edge weights w[p_k][p_{k+1}] fit
# into the narrowest window.  The reference bisects the window width D to 1e-6 and, per trial D, slides a window
# [w_min, w_min + D] over the sorted distinct weights — ONLY windows that end inside the weight range (it stops at the first
# w_min + D > W[-1], prior.py:258-259) — running a greedy label DP per window.  That predicate is NOT "D >= the exact
# threshold": a window that needs the largest weight is feasible only when some distinct weight sits exactly D below W[-1] or
# lower, ties and small graphs make it non-monotone, and the reference returns None for about a quarter of small random graphs
# (tests/golden/prior_goldens.npz `path*` pins 232 randomised cases, 60 of them None).  Formulation here:
#   1. the reference's scalar bisection, trial by trial, on its real predicate — "some window [w, w + D], w a distinct weight,
#      w + D <= W[-1], carries an n-node path" — where a window's test is a boolean reachability product (inside a window of
#      width D every path's spread is <= D, so the reference's label DP succeeds exactly when a path exists);
#   2. one label pass in the first feasible window of the last feasible trial, level-synchronous and vectorised over the
#      predecessors, with parent pointers instead of stored paths.  Labels and tie-breaks are the reference's (keep, per
#      (node, length), the partial path of smallest spread; among equals the smallest predecessor index), so the picked path
#      is identical.
def _edges_in(weights: np.ndarray, lo: float, hi: float) -> np.ndarray:
    """Upper-triangular mask of the existing edges whose weight lies in [lo, hi]."""
    m = weights.shape[0]
    return np.triu(np.ones((m, m), dtype=bool), 1) & (weights != -1) & (weights >= lo) & (weights <= hi)


def _reachable(mask: np.ndarray, n: int) -> bool:
    """Is node m - 1 reachable from node 0 in exactly n - 1 steps over the edges of ``mask``?"""
    front = np.zeros(mask.shape[0], dtype=bool)
    front[0] = True
    for _ in range(n - 1):
        front = (front.astype(np.int64) @ mask.astype(np.int64)) > 0
        if not front.any():
            return False
    return bool(front[-1])


def _first_window(D: float, n: int, weights: np.ndarray, W: np.ndarray) -> Optional[float]:
    """Lower end of the first window the reference's scan accepts for trial width D (prior.py:256-295), or None."""
    for w_lo in W:
        if w_lo + D > W[-1]:
            break                                    # the reference never tries a window that ends beyond the largest weight
        if _reachable(_edges_in(weights, w_lo, w_lo + D), n):
            return float(w_lo)
    return None


def _label_pass(n: int, weights: np.ndarray, mask: np.ndarray, width: float) -> Optional[List[int]]:
    """One sweep of (max, min) labels over path lengths 1 .. n inside one window; returns the path to node m - 1."""
    m = weights.shape[0]
    top = np.full((n + 1, m), np.nan)            # label of the kept partial path ending in node j with l nodes
    low = np.full((n + 1, m), np.nan)
    parent = np.full((n + 1, m), -1, dtype=np.int64)
    alive = np.zeros((n + 1, m), dtype=bool)
    top[1, 0], low[1, 0], alive[1, 0] = -np.inf, np.inf, True
    for l in range(1, n):
        src = np.flatnonzero(alive[l])
        if src.size == 0:
            return None
        for j in range(1, m):
            cand = src[(src < j) & mask[src, j]]
            if cand.size == 0:
                continue
            w = weights[cand, j]
            hi_, lo_ = np.maximum(top[l, cand], w), np.minimum(low[l, cand], w)
            spread = hi_ - lo_
            ok = spread <= width
            if not ok.any():
                continue
            k = int(np.argmin(np.where(ok, spread, np.inf)))          # first minimum = smallest predecessor index
            top[l + 1, j], low[l + 1, j], parent[l + 1, j], alive[l + 1, j] = hi_[k], lo_[k], cand[k], True
    if not alive[n, m - 1]:
        return None
    path, node = [m - 1], m - 1
    for l in range(n, 1, -1):
        node = int(parent[l, node])
        path.append(node)
    return path[::-1]


def find_minimal_spread_and_path(n: int, m: int, weights) -> Tuple[Optional[float], Optional[List[int]]]:
    """(window width, node path) of the smoothest n-node path 0 -> m - 1 through the explored frames — what the reference's
    bisection + window scan returns (prior.py:223-297), including ``(None, None)`` where the reference finds nothing."""
    weights = np.asarray(weights, dtype=np.float64)
    iu = np.triu_indices(m, 1)
    present = weights[iu]
    W = np.unique(present[present != -1])
    low, high = 0.0, float(W[-1] - W[0])
    width, start = None, None
    while high - low > 1e-6:
        D = (low + high) / 2
        w_lo = _first_window(D, n, weights, W)
        if w_lo is not None:
            high, width, start = D, D, w_lo
        else:
            low = D
    if width is None:
        return None, None
    return width, _label_pass(n, weights, _edges_in(weights, start, start + width), width)


def extract_uniform_points_plus(features: Sequence[torch.Tensor], interpolation_size: int,
                                distance: Callable = clip_distance) -> Optional[List[int]]:
    """Smoothest path of ``interpolation_size`` frames through the explored ones (prior.py:212-221)."""
    m = len(features)
    weights = np.full((m, m), -1.0)
    for a in range(m - 1):
        for b in range(a + 1, m):
            weights[a, b] = float(distance(features[a], features[b]))       # float() also brings a device scalar to the host
    return find_minimal_spread_and_path(interpolation_size, m, weights)[1]


class BetaPriorExplorer:
    """``explore_with_beta`` / ``generate_interpolation`` (prior.py:119-340) over a generator callback.

    ``generate(ts)`` renders the frames at coefficients ``ts`` (strictly inside (0, 1), ascending) between the two fixed
    end points and returns ``(frames, features)`` — one entry per element of ``[0, *ts, 1]``, features as [1, D]
    tensors.  The reference calls its pipeline once per new point (batch 3); ``batch`` > 1 fills that many gaps per call.
    """

    def __init__(self, generate: Callable[[List[float]], Tuple[list, List[torch.Tensor]]],
                 distance: Callable = clip_distance):
        self.generate = generate
        self._distance = distance

    def distance(self, a, b):
        """Distance of two feature rows as a HOST scalar: features (and the cosine) stay on the frames' device, the search
        decisions (widest gap, curve fit) are host arithmetic on 0-dim fp32 values like the reference's."""
        d = self._distance(a, b)
        return d.detach().cpu() if torch.is_tensor(d) and d.device.type != "cpu" else d

    def explore(self, exploration_size: int = 16, init_alpha: float = 3, init_beta: float = 3, uniform: bool = False,
                batch: int = 1):
        frames, features = self.generate([0.5])
        frames, features = list(frames), list(features)
        xs = [0.0, 0.5, 1.0]
        ds = [self.distance(features[0], features[1]), self.distance(features[1], features[2])]
        alpha, beta_param = init_alpha, init_beta
        while len(xs) < exploration_size:
            picks = []
            for rank in range(min(batch, len(ds), exploration_size - len(xs))):
                idx, t = next_point(xs, ds, alpha, beta_param, uniform=uniform, rank=rank)
                if t < 0 or t > 1:
                    break
                picks.append((idx, t))
            if not picks:
                break
            picks.sort(key=lambda p: p[1])
            new_frames, new_feats = self.generate([t for _, t in picks])
            for k, (idx, t) in sorted(enumerate(picks), key=lambda e: -e[1][0]):     # insert from the back: indices stay valid
                f = new_feats[1 + k]
                d1, d2 = self.distance(features[idx], f), self.distance(features[idx + 1], f)
                frames.insert(idx + 1, new_frames[1 + k])
                features.insert(idx + 1, f)
                xs.insert(idx + 1, t)
                del ds[idx]
                ds.insert(idx, d1)
                ds.insert(idx + 1, d2)
            alpha, beta_param = update_alpha_beta(xs, ds)
            if uniform:
                alpha, beta_param = 1, 1
        return frames, features, ds, xs, alpha, beta_param

    def generate_interpolation(self, interpolation_size: int = 7, **explore_kwargs):
        frames, features, ds, xs, alpha, beta_param = self.explore(**explore_kwargs)
        idxs = extract_uniform_points_plus(features, interpolation_size, self.distance)
        self.frames, self.ds, self.xs, self.alpha, self.beta_param = frames, ds, xs, alpha, beta_param   # prior.py:332-338
        return [frames[i] for i in idxs]


class BetaPriorPipeline:
    """The reference's ``BetaPriorPipeline`` (prior.py:12-340) over this package's pipeline classes: same constructor
    shape (``pipe``, ``model_ID``) and methods (``_compute_clip``, ``_get_feature``, ``explore_with_beta``,
    ``generate_interpolation``; attributes ``images / ds / xs / alpha / beta_param`` after a run, :332-338).

    Feature extractor: ``model`` = anything with ``get_image_features(pixel_values) -> [B, D]`` (transformers'
    ``CLIPModel`` when its weights are available — third-party; ``model_ID`` is tried through ``from_pretrained`` only if
    no model is given) plus an optional ``preprocess``; features and the cosine distances stay on the device the frames
    are on (the reference moves every frame through CPU PIL preprocessing).
    Rendering: ``pipe.interpolate_single(t, ...)`` per new point like the reference, or — ``batch`` > 1 — one N-frame
    ``pipe.interpolate`` run over ``[0, *ts, 1]`` filling several gaps at once (the processors take any coefficient vector).
    ``reuse_endpoints`` (build-specific): every render of an exploration runs between the same two end points, so the first one
    records them into an ``EndpointStore`` and the later ones replay it — only the new frames go through the UNet.
    """

    def __init__(self, pipe, model_ID: str = "openai/clip-vit-base-patch32", model=None, preprocess=None,
                 reuse_endpoints: bool = False):
        if model is None:
            from transformers import CLIPImageProcessor, CLIPModel      # needs the checkpoint on disk (no network here)
            model = CLIPModel.from_pretrained(model_ID)
            preprocess = preprocess or CLIPImageProcessor.from_pretrained(model_ID)
        self.model, self.preprocess, self.pipe = model, preprocess, pipe
        self.reuse_endpoints = bool(reuse_endpoints)
        self.endpoints = None                          # the store of the exploration in progress (reuse_endpoints)

    def _compute_clip(self, embedding_a, embedding_b):
        return clip_distance(embedding_a, embedding_b)

    @torch.no_grad()
    def _get_feature(self, image):
        """CLIP image feature of one frame, [1, D] (prior.py:24-33).  With a ``preprocess`` component the frame goes through
        it the way the reference calls transformers' ``CLIPImageProcessor``: ``preprocess(image, return_tensors="pt"
        [, do_rescale=False for numpy frames]).pixel_values`` — float frames in [0, 1] must not be rescaled again; uint8
        frames (what this package's pipelines return for ``output_type="np"``) keep the processor's 1/255 rescale.  The
        pixel tensor is then moved to the feature model's device and dtype."""
        if self.preprocess is not None:
            kw = {"return_tensors": "pt"}
            if isinstance(image, np.ndarray) and image.dtype.kind == "f":
                kw["do_rescale"] = False
            out = self.preprocess(image, **kw)
            image = getattr(out, "pixel_values", None)
            if image is None:
                image = out["pixel_values"] if isinstance(out, dict) else out
        if not torch.is_tensor(image):
            image = torch.as_tensor(np.asarray(image))
        if image.ndim == 3:
            image = image[None]
        ref = next(iter(self.model.parameters()), None) if hasattr(self.model, "parameters") else None
        if ref is not None:
            image = image.to(ref.device, ref.dtype) if image.is_floating_point() else image.to(ref.device)
        return self.model.get_image_features(image)

    def _render(self, ts, prompt_start, prompt_end, negative_prompt, latent_start, latent_end, num_inference_steps, kw):
        """Frames at ``[0, *ts, 1]``: batch-3 ``interpolate_single`` for one point (the reference's call, prior.py:94-104),
        an N-frame ``interpolate`` with the coefficient vector for several."""
        if self.endpoints is not None:
            kw = dict(kw, endpoints=self.endpoints)
        if len(ts) == 1:
            out = self.pipe.interpolate_single(ts[0], prompt_start=prompt_start, prompt_end=prompt_end,
                                               negative_prompt=negative_prompt, latent_start=latent_start,
                                               latent_end=latent_end, num_inference_steps=num_inference_steps, **kw)
            frames = out["images"] if isinstance(out, dict) else out.images
        else:
            # the N-frame run renders with the mode load_aid / load_aid_ip_adapter selected (the batch-3 call above does too).  Image
            # prompts (image_start / image_end / image_embeds_start / image_embeds_end / init in ``kw``) go to ``interpolate`` as they go
            # to ``interpolate_single``: each frame attends with the image embeddings mixed at its coefficient; "scale_control" is
            # only ``image_end`` over the outer text interpolation
            early = getattr(self.pipe, "_aid_early", None)
            if early not in ("pure_inner", "fused_inner", "pure_outer", "fused_outer"):
                early = "fused_outer"
            frames = self.pipe.interpolate(latent_start, latent_end, prompt_start, prompt_end,
                                           negative_prompt=negative_prompt, size=len(ts) + 2, early=early,
                                           num_inference_steps=num_inference_steps, coef=[0.0] + list(ts) + [1.0], **kw)
        frames = [frames[i] for i in range(len(ts) + 2)]
        return frames, [self._get_feature(f) for f in frames]

    def explore_with_beta(self, prompt_start, prompt_end, negative_prompt, latent_start, latent_end,
                          num_inference_steps=28, exploration_size=16, init_alpha=3, init_beta=3, uniform=False,
                          batch: int = 1, **kwargs):
        kwargs.pop("early", None)                      # accepted and ignored like the reference
        if self.reuse_endpoints:                       # one store per exploration: its first render records, the others replay
            from .endpoint_store import EndpointStore
            self.endpoints = EndpointStore()
        ex = BetaPriorExplorer(lambda ts: self._render(ts, prompt_start, prompt_end, negative_prompt, latent_start,
                                                       latent_end, num_inference_steps, kwargs), self._compute_clip)
        return ex.explore(exploration_size, init_alpha, init_beta, uniform=uniform, batch=batch)

    def generate_interpolation(self, prompt_start, prompt_end, negative_prompt, latent_start, latent_end,
                               num_inference_steps=28, exploration_size=16, init_alpha=3, init_beta=3,
                               interpolation_size=7, uniform=False, **kwargs):
        images, features, ds, xs, alpha, beta_param = self.explore_with_beta(
            prompt_start, prompt_end, negative_prompt, latent_start, latent_end, num_inference_steps, exploration_size,
            init_alpha, init_beta, uniform=uniform, **kwargs)
        idxs = extract_uniform_points_plus(features, interpolation_size, self._compute_clip)
        self.images, self.ds, self.xs, self.alpha, self.beta_param = images, ds, xs, alpha, beta_param
        return [images[i] for i in idxs]


# ---- automatic choice of the Beta prior (prior.py:343-478) --------------------------------------------------------------
class GaussianProcessUCB:
    """A small deterministic Gaussian-process / upper-confidence-bound maximiser over a box (numpy / scipy only) — the default
    optimiser of ``bayesian_prior_selection``, where the reference uses ``bayes_opt.BayesianOptimization``.

    ``register(point, score)`` adds an observation (duplicates allowed), ``suggest()`` returns the next point to evaluate: the
    maximiser of ``mean + kappa * std`` of a zero-mean GP on the standardised scores, Matern-5/2 kernel over the unit box, over a
    ``grid`` x ``grid`` set of candidates (one per cell, placed inside its cell by the generator ``random_state`` seeds).  The
    kernel's length scale is the one of ``length_scales`` (fractions of the box; none shorter than a fifth of it — below the spacing of
    the nine probes the mean falls back to the prior between observations and the search only explores) with the largest marginal
    likelihood.  All state is the instance's own:
    two instances with the same ``random_state`` fed the same observations propose the same points."""

    def __init__(self, bounds: Sequence[Tuple[float, float]], random_state: int = 1, kappa: float = 2.576, grid: int = 49,
                 length_scales: Sequence[float] = (0.2, 0.3, 0.5, 0.7, 1.0), jitter: float = 1e-6):
        self.lo = np.array([float(b[0]) for b in bounds])
        self.hi = np.array([float(b[1]) for b in bounds])
        if np.any(self.hi < self.lo):
            raise ValueError("bounds must be (low, high) pairs with low <= high")
        self.kappa, self.grid, self.jitter = float(kappa), int(grid), float(jitter)
        self.length_scales = tuple(float(l) for l in length_scales)
        self._rng = np.random.RandomState(random_state)
        self.points: List[Tuple[float, ...]] = []
        self.scores: List[float] = []

    def register(self, point: Sequence[float], score: float) -> None:
        self.points.append(tuple(float(p) for p in point))
        self.scores.append(float(score))

    @property
    def max(self) -> Tuple[Tuple[float, ...], float]:
        """(point, score) of the best observation; the first of equals."""
        i = int(np.argmax(self.scores))
        return self.points[i], self.scores[i]

    def _unit(self, x: np.ndarray) -> np.ndarray:
        span = np.where(self.hi > self.lo, self.hi - self.lo, 1.0)
        return (x - self.lo) / span

    @staticmethod
    def _matern52(a: np.ndarray, b: np.ndarray, length: float) -> np.ndarray:
        r = np.sqrt(np.maximum(((a[:, None, :] - b[None, :, :]) ** 2).sum(-1), 0.0)) * (np.sqrt(5.0) / length)
        return (1.0 + r + r * r / 3.0) * np.exp(-r)

    def _candidates(self) -> np.ndarray:
        """One candidate per cell of the grid over the unit box, at a seeded place inside its cell."""
        g, dim = self.grid, len(self.lo)
        cells = np.stack(np.meshgrid(*([np.arange(g)] * dim), indexing="ij"), -1).reshape(-1, dim)
        return (cells + self._rng.uniform(size=cells.shape)) / g

    def suggest(self) -> Tuple[float, ...]:
        from scipy.linalg import cho_factor, cho_solve, solve_triangular
        cand = self._candidates()
        if not self.points:
            u = cand[self._rng.randint(len(cand))]
            return tuple(float(v) for v in self.lo + u * (self.hi - self.lo))
        x = self._unit(np.asarray(self.points, dtype=np.float64))
        y = np.asarray(self.scores, dtype=np.float64)
        spread = y.std()
        y = (y - y.mean()) / (spread if spread > 0 else 1.0)
        best = None
        for length in self.length_scales:
            k = self._matern52(x, x, length) + self.jitter * np.eye(len(x))
            fac = cho_factor(k, lower=True)
            a = cho_solve(fac, y)
            evidence = -0.5 * float(y @ a) - float(np.log(np.diag(fac[0])).sum())
            if best is None or evidence > best[0]:
                best = (evidence, length, fac, a)
        _, length, fac, a = best
        ks = self._matern52(cand, x, length)
        mean = ks @ a
        v = solve_triangular(fac[0], ks.T, lower=True)
        std = np.sqrt(np.maximum(1.0 - (v * v).sum(0), 0.0))
        u = cand[int(np.argmax(mean + self.kappa * std))]
        return tuple(float(v_) for v_ in self.lo + u * (self.hi - self.lo))


def _check_selection_init(init: str) -> None:
    if init == "denoising":
        raise NotImplementedError('init="denoising": the reference\'s denoising_interpolate baseline is not part of this package')
    if init != "linear":
        raise NotImplementedError(f"init={init!r}: the N-frame run mixes the text embeddings linearly (init=\"linear\")")


_SELECTION_PIPE_KWARGS = ("embeds_start", "embeds_end", "embeds_guide", "output_type", "guidance_scale", "use_graphs",
                          "cross_attention_kwargs", "init")


class SmoothnessObjective:
    """The black-box objective of ``bayesian_prior_selection`` (prior.py:387-416) and the run it stands on: ``prime()`` is the
    ``interpolate_single(0.5)`` run that fixes the prior gate and ``init_smoothness``; ``__call__(alpha, beta)`` the gated score;
    ``render(pairs)`` the frame sequences of several (alpha, beta) — one pipeline run per pair, or ONE replay run for all of them
    (``batched=True``: the interior coefficients concatenated into one ``coef`` vector, each pair's frames sliced back out);
    ``measure(frames)`` the triple (smoothness, consistency, maximum distance).

    ``reuse_endpoints``: ``prime()`` records the two end points into an ``EndpointStore`` and every rendered sequence replays it —
    only the ``size - 2`` interior frames go through the UNet, the end-point frames are the recorded ones."""

    def __init__(self, pipe, latent1, latent2, prompt1, prompt2, lpips_model=None, guide_prompt=None, negative_prompt="",
                 size: int = 3, num_inference_steps: int = 25, warmup_ratio: float = 1, early: str = "fused_outer",
                 late: str = "self", distance: Optional[Callable] = None, reuse_endpoints: bool = True, **pipe_kwargs):
        from .loop import EARLY_MODES
        if early == "vfused":                # the reference's stale default (its own pipeline has no such mode): the pipelines' default
            early = "fused_outer"
        if early not in EARLY_MODES or (late != "self" and late not in EARLY_MODES):
            raise ValueError(f"early / late must be in {EARLY_MODES} (late also 'self')")
        unknown = sorted(set(pipe_kwargs) - set(_SELECTION_PIPE_KWARGS))
        if unknown:
            raise TypeError(f"unexpected keyword arguments {unknown}; the pipeline calls take {_SELECTION_PIPE_KWARGS}")
        _check_selection_init(pipe_kwargs.get("init", "linear"))
        if size < 3:
            raise ValueError("size must be at least 3: two end points and an interior frame")
        if distance is None and lpips_model is None:
            raise ValueError("pass an `lpips_model`, or a `distance` for frames that are not images")
        self.pipe, self.size, self.early, self.late = pipe, int(size), early, late
        self.lpips_model, self.distance = lpips_model, distance
        self.reuse_endpoints = bool(reuse_endpoints)
        self.endpoints = None
        self.init_smoothness = self.init_distances = self.large_alpha_prior = None
        self.renders = 0                                 # pipeline runs made, the prime run included
        self._common = dict(latent_start=latent1, latent_end=latent2, prompt_start=prompt1, prompt_end=prompt2,
                            guide_prompt=guide_prompt, negative_prompt=negative_prompt,
                            num_inference_steps=num_inference_steps, warmup_ratio=warmup_ratio, early=early, late=late,
                            **pipe_kwargs)

    # -- scoring ----------------------------------------------------------------------------------------------------------------
    def distances(self, frames) -> np.ndarray:
        if self.distance is not None:
            return adjacent_distances(frames, self.distance)
        return compute_lpips(frames, self.lpips_model)

    def measure(self, frames) -> Tuple[float, float, float]:
        return smoothness_and_consistency_of(self.distances(frames))

    # -- rendering --------------------------------------------------------------------------------------------------------------
    def prime(self):
        """The ``t = 0.5`` run: neighbour distances of its three frames, ``init_smoothness``, and which side of alpha = beta the
        prior allows.  With ``reuse_endpoints`` the run records the end points (a normal run, bit-identical outputs)."""
        kw = dict(self._common)
        installed = getattr(self.pipe, "_aid_early", None)
        if installed is not None and (installed != self.early or self.late != "self"):
            # this package's interpolate_single renders with the mode load_aid installed and plain attention afterwards
            raise ValueError(f"the t = 0.5 run would render with the installed mode {installed!r} / 'self', the evaluations with "
                             f"{self.early!r} / {self.late!r}: call load_aid(atype={self.early!r}) and keep late='self'")
        if self.reuse_endpoints:
            from .endpoint_store import EndpointStore
            self.endpoints = EndpointStore()
            kw["endpoints"] = self.endpoints
        out = self.pipe.interpolate_single(it=0.5, **kw)
        self.renders += 1
        frames = out["images"] if isinstance(out, dict) else getattr(out, "images", out)
        self.init_distances = self.distances(frames)
        self.init_smoothness = 1 - compute_gini(self.init_distances)
        self.large_alpha_prior = bool(self.init_distances[0] < self.init_distances[1])
        return frames

    def allowed(self, alpha: float, beta_param: float) -> bool:
        """Does the prior let (alpha, beta) be rendered?  (alpha == beta is answered by ``init_smoothness``.)"""
        return alpha > beta_param if self.large_alpha_prior else alpha < beta_param

    def coefficients(self, alpha: float, beta_param: float) -> List[float]:
        return [float(t) for t in generate_beta_tensor(self.size, alpha, beta_param)]

    def render(self, pairs: Sequence[Tuple[float, float]], batched: bool = False) -> list:
        """The ``size``-frame sequence of every (alpha, beta) of ``pairs``."""
        pairs = list(pairs)
        if self.reuse_endpoints and self.endpoints is None:
            raise RuntimeError("render before prime(): the t = 0.5 run records the end points")
        ep = {"endpoints": self.endpoints} if self.reuse_endpoints else {}
        if not batched:
            out = []
            for a, b in pairs:
                out.append(self.pipe.interpolate_save_gpu(size=self.size, alpha=a, beta=b, **self._common, **ep))
                self.renders += 1
            return out
        if not self.reuse_endpoints:
            raise ValueError("a batched render shares the recorded end points among its candidates: it needs reuse_endpoints")
        if not pairs:
            return []
        k = self.size - 2
        inner = [t for a, b in pairs for t in self.coefficients(a, b)[1:-1]]
        kw = {n: v for n, v in self._common.items() if n != "init"}
        frames = self.pipe.interpolate(size=len(inner) + 2, coef=[0.0] + inner + [1.0], **kw, **ep)
        self.renders += 1
        last = len(inner) + 1
        return [frames[[0] + list(range(1 + j * k, 1 + (j + 1) * k)) + [last]] for j in range(len(pairs))]

    def release(self) -> None:
        """Drop the recorded end points."""
        if self.endpoints is not None:
            self.endpoints.clear()
            self.endpoints = None

    def __call__(self, alpha: float, beta_param: float, frames=None) -> Tuple[float, bool]:
        """(score, rendered) of one (alpha, beta): 0 on the side the prior refuses and ``init_smoothness`` on the diagonal, both
        without rendering; else the smoothness of the rendered sequence (``frames``: already rendered by a batched run)."""
        if alpha == beta_param:
            return self.init_smoothness, False
        if not self.allowed(alpha, beta_param):
            return 0, False
        if frames is None:
            frames = self.render([(alpha, beta_param)])[0]
        return self.measure(frames)[0], True


def bayesian_prior_selection(interpolation_pipe, latent1, latent2, prompt1, prompt2, lpips_model, guide_prompt=None,
                             negative_prompt="", size=3, num_inference_steps=25, warmup_ratio=1, early="vfused", late="self",
                             target_score=0.9, n_iter=15, p_min=None, p_max=None, *, distance: Optional[Callable] = None,
                             reuse_endpoints: bool = True, batch_probes: bool = True, optimizer=None,
                             return_trace: bool = False, **pipe_kwargs):
    """Choose the Beta prior (alpha, beta) of an interpolation by maximising the smoothness ``1 - gini`` of the perceptual
    distances between neighbouring frames (prior.py:343-478): same positional signature, defaults and decision structure.

    One ``interpolate_single(0.5)`` run gives the prior — alpha > beta when the middle frame is nearer the first end point — and
    the score of every alpha == beta.  The 3 x 3 grid ``{p_min, (p_min + p_max) / 2, p_max}^2`` is probed alpha-major and the FIRST
    probe that reaches ``target_score`` is returned; then at most ``n_iter`` proposals of the optimiser follow, one at a time, until
    the best score reaches the target; the best point evaluated is returned.  ``p_min = 1``, ``p_max = warmup_ratio *
    num_inference_steps`` unless given.  ``early="vfused"`` (the reference's stale default) means ``"fused_outer"``.

    Build-specific, keyword-only: ``distance(frame_a, frame_b)`` scores frames that are not images (then ``lpips_model`` may be
    None).  ``reuse_endpoints``: the first run records the two end points (``EndpointStore``), every rendered evaluation replays them
    — ``size - 2`` frames through the UNet instead of ``size``; ``False`` renders every evaluation in full.  ``batch_probes``: the
    probes that need rendering share ONE replay run, made before the scan (which still reads the scores in the reference's order);
    needs ``reuse_endpoints``.  ``optimizer``: an object with ``suggest() -> (alpha, beta)`` and ``register((alpha, beta), score)``
    (default :class:`GaussianProcessUCB`, ``random_state=1``).  ``return_trace``: also return the list of ``(alpha, beta, score,
    rendered)`` in evaluation order.  ``pipe_kwargs`` (``embeds_start``, ``embeds_end``, ``embeds_guide``, ``output_type``,
    ``guidance_scale``, ``use_graphs``, ``cross_attention_kwargs``) reach the pipeline calls unchanged."""
    if batch_probes and not reuse_endpoints:
        raise ValueError("batch_probes renders the probes in one replay run between the recorded end points: it needs "
                         "reuse_endpoints=True")
    objective = SmoothnessObjective(interpolation_pipe, latent1, latent2, prompt1, prompt2, lpips_model, guide_prompt=guide_prompt,
                                    negative_prompt=negative_prompt, size=size, num_inference_steps=num_inference_steps,
                                    warmup_ratio=warmup_ratio, early=early, late=late, distance=distance,
                                    reuse_endpoints=reuse_endpoints, **pipe_kwargs)
    trace: List[Tuple[float, float, float, bool]] = []

    def result(alpha, beta_param):
        return ((alpha, beta_param), trace) if return_trace else (alpha, beta_param)

    try:
        objective.prime()
        if p_min is None:
            p_min = 1
        if p_max is None:
            p_max = warmup_ratio * num_inference_steps
        if optimizer is None:
            optimizer = GaussianProcessUCB(((p_min, p_max), (p_min, p_max)), random_state=1)

        def evaluate(alpha, beta_param, frames=None):
            score, rendered = objective(alpha, beta_param, frames)
            trace.append((alpha, beta_param, score, rendered))
            optimizer.register((alpha, beta_param), score)
            return score

        axis = [p_min, (p_min + p_max) / 2, p_max]
        probes = [(a, b) for a in axis for b in axis]                    # alpha-major (prior.py:459-460)
        ready = {}
        # (the first probe is the diagonal point (p_min, p_min): when init_smoothness already reaches the target the scan ends there and,
        # as in the reference, nothing is rendered)
        if batch_probes and not objective.init_smoothness >= target_score:
            need = [p for p in dict.fromkeys(probes) if p[0] != p[1] and objective.allowed(*p)]
            ready = dict(zip(need, objective.render(need, batched=True)))
        for alpha, beta_param in probes:
            if evaluate(alpha, beta_param, ready.get((alpha, beta_param))) >= target_score:
                return result(alpha, beta_param)
        for _ in range(n_iter):
            alpha, beta_param = optimizer.suggest()
            evaluate(alpha, beta_param)
            if max(s for _, _, s, _ in trace) >= target_score:
                break
        alpha, beta_param, _, _ = max(trace, key=lambda e: e[2])         # the first of equals, like ``optimizer.max``
        return result(alpha, beta_param)
    finally:
        objective.release()
