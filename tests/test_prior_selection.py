"""CPU: the automatic choice of the Beta prior (reference prior.py:343-478, utils.py:108-213).

(1) The metric functions against outputs of the reference's own ``utils.py`` (tests/golden/selection_goldens.npz; inputs regenerate
    from the seeds in make_selection_goldens.py, whose LPIPS stand-in is used here too).
(2) The decision structure of ``bayesian_prior_selection`` over a fake pipeline that counts its calls and returns frames from a
    table — a frame is the position of its coefficient on a piecewise-linear path, the distance of two frames the difference of
    their positions — so every score below is known in closed form.
(3) The default optimiser on the issue's four quadratic bowls behind the prior gate."""
import numpy as np
import pytest
import torch

import aid_amd
import make_selection_goldens as G
from aid_amd import metrics as M
from aid_amd import prior as PR
from aid_amd.interp import generate_beta_tensor

GOLD = np.load(G.os.path.join(G.HERE, "selection_goldens.npz"))


# ---- (1) metrics ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(G.gini_vectors()))
def test_compute_gini_against_the_reference(name):
    got = M.compute_gini(G.gini_vectors()[name])
    assert abs(float(got) - float(GOLD[f"gini_{name}"])) <= 1e-12
    if name in ("empty", "one"):
        assert got == 0.0


@pytest.mark.parametrize("name", sorted(G.image_stacks()))
def test_lpips_path_against_the_reference(name):
    images, model = G.image_stacks()[name], G.TinyLPIPS()
    d = M.compute_lpips(images, model)
    assert isinstance(d, np.ndarray) and d.shape == (4,)
    assert np.abs(d - GOLD[f"lpips_{name}"]).max() <= 2e-6
    triple = np.array(M.compute_smoothness_and_consistency(images, model), dtype=np.float64)
    assert np.abs(triple - GOLD[f"triple_{name}"]).max() <= 2e-6
    assert np.abs(np.array(M.smoothness_and_consistency_of(d)) - triple).max() == 0


def test_uint8_images_are_normalised_on_their_own_range():
    """The reference subtracts the ImageNet mean from 0 .. 255 values as they are: the same picture as uint8 and as
    float 0 .. 1 does NOT give the same distances."""
    images = G.image_stacks()["uint8_path"]
    model = G.TinyLPIPS()
    assert not np.allclose(M.compute_lpips(images, model), M.compute_lpips(images / 255.0, model), rtol=1e-2)


def test_separate_source_and_interpolated_images():
    images = np.arange(5 * 2 * 2 * 3).reshape(5, 2, 2, 3)
    source, inner = M.separate_source_and_interpolated_images(images)
    assert np.array_equal(source, images[[0, 4]]) and np.array_equal(inner, images[1:4])
    with pytest.raises(ValueError, match="at least two elements"):
        M.separate_source_and_interpolated_images(images[:1])


def test_adjacent_distances_takes_tensor_and_float_distances():
    frames = torch.tensor([[0.0], [0.25], [1.0]])
    as_tensor = M.adjacent_distances(frames, lambda a, b: (b - a).abs().sum())
    as_float = M.adjacent_distances([f for f in frames], lambda a, b: float((b - a).abs().sum()))
    assert as_tensor.dtype == np.float64 and np.array_equal(as_tensor, [0.25, 0.75]) and np.array_equal(as_float, as_tensor)
    s, c, m = M.smoothness_and_consistency_of(as_tensor)
    assert s == pytest.approx(1 - 0.25) and c == pytest.approx(0.5) and m == 0.75      # gini of two = |d0 - d1| / (2 (d0 + d1))


def test_package_root_exports():
    for name in ("bayesian_prior_selection", "GaussianProcessUCB", "compute_lpips", "compute_gini", "compute_smoothness_and_consistency",
                 "separate_source_and_interpolated_images", "adjacent_distances", "smoothness_and_consistency_of"):
        assert name in aid_amd.__all__ and hasattr(aid_amd, name)


# ---- (2) decision structure -----------------------------------------------------------------------------------------------------------
class FakePipe:
    """Counts its calls; a frame is ``[position(t)]`` of its coefficient on the piecewise-linear path through ``knots``."""

    def __init__(self, knots):
        self.ts, self.ps = zip(*knots)
        self.calls = []

    def _frames(self, ts):
        return np.array([[np.interp(t, self.ts, self.ps)] for t in ts])

    def interpolate_single(self, it, **kw):
        self.calls.append(("interpolate_single", dict(kw, it=it)))
        return {"images": self._frames([0.0, it, 1.0])}

    def interpolate_save_gpu(self, **kw):
        self.calls.append(("interpolate_save_gpu", kw))
        return self._frames([float(t) for t in generate_beta_tensor(kw["size"], kw["alpha"], kw["beta"])])

    def interpolate(self, **kw):
        self.calls.append(("interpolate", kw))
        assert len(kw["coef"]) == kw["size"]
        return self._frames(kw["coef"])

    def names(self):
        return [n for n, _ in self.calls]


def distance(a, b):
    return abs(float(b[0] - a[0]))


def t_mid(alpha, beta):
    return float(generate_beta_tensor(3, alpha, beta)[1])


class ListOptimizer:
    """Proposes the points of a list, in order; records what it is told."""

    def __init__(self, points):
        self.points, self.suggested, self.registered = list(points), 0, []

    def suggest(self):
        self.suggested += 1
        return self.points[self.suggested - 1]

    def register(self, point, score):
        self.registered.append((tuple(point), score))


LARGE = [(0.0, 0.0), (0.5, 0.25), (1.0, 1.0)]          # the middle frame is nearer the start: alpha > beta is allowed
# the middle frame is nearer the end (alpha < beta allowed), and the frame of (alpha, beta) = (1, 13) sits exactly half way
SMALL = [(0.0, 0.0), (t_mid(1, 13), 0.5), (0.5, 0.8), (1.0, 1.0)]


def select(pipe, **kw):
    kw.setdefault("distance", distance)
    return PR.bayesian_prior_selection(pipe, "l1", "l2", "p1", "p2", None, return_trace=True, **kw)


@pytest.mark.parametrize("reuse", [True, False])
def test_objective_gate_and_diagonal_render_nothing(reuse):
    for knots, refused, allowed in ((LARGE, (3.0, 7.0), (7.0, 3.0)), (SMALL, (7.0, 3.0), (3.0, 7.0))):
        pipe = FakePipe(knots)
        obj = PR.SmoothnessObjective(pipe, "l1", "l2", "p1", "p2", distance=distance, size=5, reuse_endpoints=reuse)
        obj.prime()
        assert pipe.names() == ["interpolate_single"] and pipe.calls[0][1]["it"] == 0.5
        assert (pipe.calls[0][1].get("endpoints") is not None) == reuse
        assert obj.large_alpha_prior == (knots is LARGE)
        d = abs(knots[-2][1] - 0.5) * 2                                  # |d0 - d1| of the t = 0.5 run (d0 + d1 = 1)
        assert obj.init_smoothness == pytest.approx(1 - d / 2)
        assert obj(*refused) == (0, False) and pipe.names() == ["interpolate_single"]
        score, rendered = obj(4.0, 4.0)                                 # size = 5: still the three-frame score, as in the reference
        assert score == obj.init_smoothness and not rendered and pipe.names() == ["interpolate_single"]
        score, rendered = obj(*allowed)
        assert rendered and pipe.names() == ["interpolate_single", "interpolate_save_gpu"]
        call = pipe.calls[1][1]
        assert (call["alpha"], call["beta"], call["size"]) == (*allowed, 5)
        assert (call.get("endpoints") is obj.endpoints) if reuse else ("endpoints" not in call)
        frames = pipe._frames([float(t) for t in generate_beta_tensor(5, *allowed)])
        assert score == pytest.approx(1 - M.compute_gini(np.abs(np.diff(frames[:, 0]))))


@pytest.mark.parametrize("steps,ratio,axis", [(25, 1, [1, 13.0, 25]), (20, 0.5, [1, 5.5, 10.0])])
def test_default_bounds_and_alpha_major_probe_order(steps, ratio, axis):
    pipe = FakePipe(LARGE)
    opt = ListOptimizer([])
    (alpha, beta), trace = select(pipe, num_inference_steps=steps, warmup_ratio=ratio, target_score=2.0, n_iter=0, optimizer=opt,
                                  batch_probes=False)
    assert [(a, b) for a, b, _, _ in trace] == [(a, b) for a in axis for b in axis]
    assert [p for p, _ in opt.registered] == [(a, b) for a in axis for b in axis]
    # rendered: exactly the probes on the allowed side, one run each, in scan order
    rendered = [(a, b) for a, b, _, r in trace if r]
    assert rendered == [(axis[1], axis[0]), (axis[2], axis[0]), (axis[2], axis[1])]
    assert [(c["alpha"], c["beta"]) for n, c in pipe.calls if n == "interpolate_save_gpu"] == rendered
    assert pipe.names() == ["interpolate_single"] + ["interpolate_save_gpu"] * 3
    assert all(s == 0 for a, b, s, _ in trace if a < b)
    assert (alpha, beta) == max(trace, key=lambda e: e[2])[:2]
    (a2, b2), t2 = select(FakePipe(LARGE), num_inference_steps=steps, warmup_ratio=ratio, target_score=2.0, n_iter=0, p_min=2, p_max=4)
    assert [(a, b) for a, b, _, _ in t2] == [(a, b) for a in (2, 3.0, 4) for b in (2, 3.0, 4)]


@pytest.mark.parametrize("batch", [False, True])
def test_first_probe_that_reaches_the_target_is_returned(batch):
    pipe = FakePipe(SMALL)
    opt = ListOptimizer([])
    (alpha, beta), trace = select(pipe, target_score=0.9, optimizer=opt, batch_probes=batch)
    # probe 1 = (1, 1): the t = 0.5 run's 1 - |0.8 - 0.2| / 2 = 0.7, not rendered; probe 2 = (1, 13): its frame sits half way, score 1
    assert (alpha, beta) == (1, 13.0)
    assert [(a, b, r) for a, b, _, r in trace] == [(1, 1, False), (1, 13.0, True)]
    assert trace[0][2] == pytest.approx(0.7) and trace[1][2] == pytest.approx(1.0)
    assert opt.suggested == 0
    if batch:
        # ONE replay run, made before the scan, with the interior frames of the three probes the prior allows
        assert pipe.names() == ["interpolate_single", "interpolate"]
        call = pipe.calls[1][1]
        assert call["coef"] == pytest.approx([0.0, t_mid(1, 13), t_mid(1, 25), t_mid(13, 25), 1.0]) and call["size"] == 5
        assert call["endpoints"] is pipe.calls[0][1]["endpoints"]
    else:
        assert pipe.names() == ["interpolate_single", "interpolate_save_gpu"]


@pytest.mark.parametrize("batch", [False, True])
def test_nothing_is_rendered_when_the_first_probe_ends_the_search(batch):
    """The first probe (p_min, p_min) scores init_smoothness: at the target the selection returns it after the t = 0.5 run alone."""
    pipe = FakePipe(LARGE)
    (alpha, beta), trace = select(pipe, target_score=0.75, batch_probes=batch)        # init_smoothness = 1 - |0.25 - 0.75| / 2
    assert (alpha, beta) == (1, 1) and [(a, b, r) for a, b, _, r in trace] == [(1, 1, False)]
    assert pipe.names() == ["interpolate_single"]


def test_batched_probes_give_the_scores_of_single_runs():
    (p1, t1) = select(FakePipe(LARGE), size=5, target_score=2.0, n_iter=0, batch_probes=True)
    (p2, t2) = select(FakePipe(LARGE), size=5, target_score=2.0, n_iter=0, batch_probes=False)
    assert p1 == p2 and t1 == t2 and sum(r for _, _, _, r in t1) == 3


def test_at_most_n_iter_proposals_and_argmax_of_the_trace():
    pipe = FakePipe(LARGE)
    pts = [(20.0, 3.0), (6.0, 18.0), (9.0, 9.0), (24.0, 2.0), (12.0, 5.0), (3.0, 2.0)]
    opt = ListOptimizer(pts)
    (alpha, beta), trace = select(pipe, target_score=2.0, n_iter=4, optimizer=opt)
    assert opt.suggested == 4 and len(trace) == 9 + 4
    assert [(a, b) for a, b, _, _ in trace[9:]] == pts[:4]
    assert [r for _, _, _, r in trace[9:]] == [True, False, False, True]         # refused side and diagonal: not rendered
    assert opt.registered == [((a, b), s) for a, b, s, _ in trace]
    best = max(s for _, _, s, _ in trace)
    assert (alpha, beta) == next((a, b) for a, b, s, _ in trace if s == best)
    # 1 prime run + 1 batched probe run + the 2 rendered proposals
    assert pipe.names() == ["interpolate_single", "interpolate", "interpolate_save_gpu", "interpolate_save_gpu"]


def test_loop_stops_once_the_target_is_reached():
    pipe = FakePipe(LARGE)
    t_half = 0.5 + 0.25 / 1.5                                             # position(t) = 0.5 on the segment (0.5, 0.25) - (1, 1)
    # find an (alpha, 1) whose median is t_half: the median of Beta(alpha, 1) is 0.5 ** (1 / alpha)
    alpha_hit = float(np.log(0.5) / np.log(t_half))
    assert t_mid(alpha_hit, 1.0) == pytest.approx(t_half, abs=1e-6)
    opt = ListOptimizer([(5.0, 9.0), (alpha_hit, 1.0), (20.0, 2.0), (21.0, 2.0)])
    (alpha, beta), trace = select(pipe, target_score=0.999, n_iter=4, optimizer=opt)
    assert opt.suggested == 2 and len(trace) == 11 and (alpha, beta) == (alpha_hit, 1.0)
    assert trace[-1][2] >= 0.999 and max(s for _, _, s, _ in trace[:-1]) < 0.999


def test_vfused_means_fused_outer_and_other_names_raise():
    pipe = FakePipe(LARGE)
    select(pipe, target_score=2.0, n_iter=1, optimizer=ListOptimizer([(9.0, 2.0)]))
    assert {n for n in pipe.names()} == {"interpolate_single", "interpolate", "interpolate_save_gpu"}
    assert all(c["early"] == "fused_outer" and c["late"] == "self" for _, c in pipe.calls)
    pipe = FakePipe(LARGE)
    select(pipe, early="pure_inner", target_score=2.0, n_iter=0)
    assert all(c["early"] == "pure_inner" for _, c in pipe.calls)
    for bad in (dict(early="vfuse"), dict(early="self"), dict(late="fused")):
        pipe = FakePipe(LARGE)
        with pytest.raises(ValueError, match="early / late must be in"):
            select(pipe, **bad)
        assert pipe.calls == []


def test_installed_mode_must_be_the_one_the_evaluations_render_with():
    """This package's interpolate_single renders with the mode load_aid installed (``pipe._aid_early``) and ignores ``early=``."""
    pipe = FakePipe(LARGE)
    pipe._aid_early = "fused_inner"
    with pytest.raises(ValueError, match="load_aid"):
        select(pipe)                                                   # "vfused" = fused_outer
    with pytest.raises(ValueError, match="load_aid"):
        select(pipe, early="fused_inner", late="fused_inner")
    assert pipe.calls == []
    select(pipe, early="fused_inner", target_score=2.0, n_iter=0)
    assert len(pipe.calls) == 2


def test_arguments_reach_the_pipeline_through_keywords():
    pipe = FakePipe(LARGE)
    es, ee = object(), object()
    PR.bayesian_prior_selection(pipe, "l1", "l2", "p1", "p2", None, "guide", "neg", 3, 10, 0.5, "fused_inner", "self", 2.0, 1,
                                distance=distance, optimizer=ListOptimizer([(4.0, 2.0)]), embeds_start=es, embeds_end=ee,
                                output_type="latent", guidance_scale=3.0, use_graphs=False)
    assert pipe.names() == ["interpolate_single", "interpolate", "interpolate_save_gpu"]
    for _, c in pipe.calls:
        assert (c["latent_start"], c["latent_end"], c["prompt_start"], c["prompt_end"]) == ("l1", "l2", "p1", "p2")
        assert (c["guide_prompt"], c["negative_prompt"], c["num_inference_steps"], c["warmup_ratio"]) == ("guide", "neg", 10, 0.5)
        assert c["embeds_start"] is es and c["embeds_end"] is ee and c["output_type"] == "latent"
        assert c["guidance_scale"] == 3.0 and c["use_graphs"] is False and c["early"] == "fused_inner"
    with pytest.raises(TypeError, match="height"):
        select(FakePipe(LARGE), height=64)


def test_refused_arguments():
    with pytest.raises(NotImplementedError, match="denoising"):
        select(FakePipe(LARGE), init="denoising")
    with pytest.raises(ValueError, match="reuse_endpoints"):
        select(FakePipe(LARGE), batch_probes=True, reuse_endpoints=False)
    with pytest.raises(ValueError, match="lpips_model"):
        PR.bayesian_prior_selection(FakePipe(LARGE), "l1", "l2", "p1", "p2", None)
    pipe = FakePipe(LARGE)
    select(pipe, reuse_endpoints=False, batch_probes=False, target_score=2.0, n_iter=0)
    assert pipe.names() == ["interpolate_single"] + ["interpolate_save_gpu"] * 3
    assert all("endpoints" not in c for _, c in pipe.calls)


def test_lpips_model_path_scores_image_frames():
    """Without ``distance`` the frames go through compute_lpips with the model given."""
    rng = np.random.RandomState(8)
    first, last = rng.uniform(size=(1, 8, 8, 3)), rng.uniform(size=(1, 8, 8, 3))

    class ImagePipe(FakePipe):
        def _frames(self, ts):
            pos = super()._frames(ts)[:, 0][:, None, None, None]
            return (((1 - pos) * first + pos * last) * 255).astype(np.uint8)

    pipe = ImagePipe(LARGE)
    (alpha, beta), trace = PR.bayesian_prior_selection(pipe, "l1", "l2", "p1", "p2", G.TinyLPIPS(), target_score=2.0, n_iter=0,
                                                       return_trace=True)
    d = M.compute_lpips(pipe._frames([0.0, 0.5, 1.0]), G.TinyLPIPS())
    assert d[0] != d[1] and trace[0][2] == pytest.approx(1 - M.compute_gini(d))
    assert (alpha > beta) == bool(d[0] < d[1]) and sum(r for _, _, _, r in trace) == 3
    assert all(s == 0 for a, b, s, _ in trace if a != b and (a > b) != bool(d[0] < d[1]))


# ---- (3) the default optimiser ----------------------------------------------------------------------------------------------------------
def _bowl(a, b):
    return lambda x, y: 0 if x < y else 0.5 if x == y else 1 - ((x - a) ** 2 + (y - b) ** 2) / (2 * 24 ** 2)


def _search(f, random_state=1, n_iter=15):
    opt = PR.GaussianProcessUCB(((1, 25), (1, 25)), random_state=random_state)
    trace = []
    for x in (1, 13.0, 25):
        for y in (1, 13.0, 25):
            trace.append((x, y, f(x, y)))
            opt.register((x, y), f(x, y))
    for _ in range(n_iter):
        x, y = opt.suggest()
        assert 1 <= x <= 25 and 1 <= y <= 25
        trace.append((x, y, f(x, y)))
        opt.register((x, y), f(x, y))
    return opt, trace


@pytest.mark.parametrize("a,b", [(17, 6), (20, 9), (8, 3), (22, 16)])
def test_default_optimizer_finds_the_bowl_behind_the_gate(a, b):
    opt, trace = _search(_bowl(a, b))
    (x, y), best = opt.max
    assert best == max(s for _, _, s in trace) and best > max(s for _, _, s in trace[:9])
    assert abs(x - a) <= 1.0 and abs(y - b) <= 1.0, (x, y)
    _, again = _search(_bowl(a, b))
    assert again == trace                                                 # same random_state: identical traces, no global state
    np.random.seed(123)                                                   # ... whatever numpy's global generator holds
    _, third = _search(_bowl(a, b))
    assert third == trace


def test_default_optimizer_is_what_the_selection_uses():
    """With no ``optimizer`` the selection's proposals are GaussianProcessUCB(random_state=1)'s over [p_min, p_max]^2."""
    (alpha, beta), trace = select(FakePipe(LARGE), target_score=2.0, n_iter=3)
    opt = PR.GaussianProcessUCB(((1, 25), (1, 25)), random_state=1)
    for a, b, s, _ in trace[:9]:
        opt.register((a, b), s)
    for a, b, s, _ in trace[9:]:
        assert opt.suggest() == (a, b)
        opt.register((a, b), s)
    assert len(trace) == 12 and (alpha, beta) == opt.max[0]
