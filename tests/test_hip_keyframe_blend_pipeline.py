"""GPU: ``interpolate_among`` end to end — four key frames recorded as one batch into a KeyframeStore, a 3 x 3 morph grid rendered
from the recordings — on the stack of tests/test_hip_keyframe_store.py: ``StackDenoiser("sd15", scale_down=16, latent_hw=(8, 8))``,
6 steps, warm-up 0.5.

Yardstick: the fp64 oracle loop of the FULL live ``interpolate_corners`` run of the same grid (the loop of
tests/test_hip_corners_pipeline.py: every attention layer in fp64, the four corner frames in the batch), on the five rendered cells
1, 3, 4, 5, 7.  The four corner cells are the stored final latents, bit for bit.

Bounds: 1.3 x a value measured once on an MI355X (the project's rule for loop-depth bounds).  For native stores that value is the
rel-L2 of the live HIP ``interpolate_corners`` run of the grid against the loop (LIVE_MEASURED: the path without a store, which this
pull request does not touch); a q8 store is lossy and has no such twin, so its value is the q8 blend's own, measured once
(Q8_MEASURED), as tests/test_hip_keyframe_q8.py does for the two-frame replay.  Measured:

    early mode     dtype   live run     native blend   q8 blend     M = 2 (tl, br), native
    fused_outer    f16     2.044e-3     2.017e-3       2.037e-3     1.940e-3
    fused_inner    f16     2.079e-3     2.077e-3       2.049e-3     2.035e-3
    fused_outer    f32     1.317e-6     1.307e-6       3.010e-4     1.360e-6
    fused_inner    f32     1.294e-6     1.294e-6       2.094e-4     1.320e-6

(in f16 the quantisation disappears in the storage dtype's own error; in f32 a q8 blend is a 2e-4 .. 3e-4 blend, as a q8 replay is.)
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import aid_amd  # noqa: E402
from aid_amd.keyframe_store import KeyframeStore  # noqa: E402
from aid_amd.pipelines import DDIMSchedulerLite, InterpolationStableDiffusionPipeline, StackDenoiser  # noqa: E402
from util import rel_l2, to_np64  # noqa: E402

DEV = "cuda:0"
F16, F32 = torch.float16, torch.float32
STEPS, RATIO = 6, 0.5
NAMES = ["tl", "tr", "bl", "br"]
EARLY = ["fused_outer", "fused_inner"]
RENDER = [1, 3, 4, 5, 7]
CORNER_CELLS = {0: 0, 2: 1, 6: 2, 8: 3}
PAIR_C = [0.25, 0.5, 0.75]
LIVE_MEASURED = {("fused_outer", F16): 2.044e-3, ("fused_inner", F16): 2.079e-3, ("fused_outer", F32): 1.317e-6, ("fused_inner", F32): 1.294e-6}
Q8_MEASURED = {("fused_outer", F16): 2.037e-3, ("fused_inner", F16): 2.049e-3, ("fused_outer", F32): 3.010e-4, ("fused_inner", F32): 2.094e-4}


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == F16 else torch.int32)


def _bound(early, dtype, storage):
    return 1.3 * (Q8_MEASURED if storage == "q8" else LIVE_MEASURED)[(early, dtype)]


class _Runs:
    """Everything the tests of one dtype share, run once: the recordings, the live runs, the blends, the oracle loops."""

    def __init__(self, dtype):
        from test_hip_corners_pipeline import CornerOracleDenoiser
        from test_hip_depth_and_pipelines import OracleDenoiser
        self.dtype = dtype
        hip = StackDenoiser("sd15", dtype=dtype, device=DEV, scale_down=16, latent_hw=(8, 8))
        g = torch.Generator().manual_seed(41)
        self.lats = lats = torch.randn(4, 4, 8, 8, generator=g).to(dtype)
        cc = hip.stack.cross_dim
        rd = lambda t: tuple(e.to(dtype).float() for e in t)     # noqa: E731   every run sees the dtype-rounded embeddings
        self.embs = embs = [rd((torch.randn(1, 77, cc, generator=g), torch.randn(1, 77, cc, generator=g))) for _ in range(4)]
        self.pipe = pipe = InterpolationStableDiffusionPipeline(hip, DDIMSchedulerLite())
        pipe.load_aid(t=0.5, is_fused=True, atype="fused_outer")
        self.installed = dict(hip.attn_processors)
        self.w = w = aid_amd.grid_weights(3, 3)
        rkw = dict(num_inference_steps=STEPS, warmup_ratio=RATIO, output_type="latent")
        self.stores = {}
        for storage in ("native", "q8"):
            self.stores[storage] = st = KeyframeStore(storage=storage)
            pipe.record_keyframes(st, NAMES, lats, embeds=embs, **rkw)
        gs = pipe.default_guidance_scale
        ckw = dict(weights=w, num_inference_steps=STEPS, warmup_ratio=RATIO, guidance_scale=gs, output_type="latent")
        self.live = {e: pipe.interpolate_corners(lats, embeds=embs, early=e, **ckw).clone() for e in EARLY}
        akw = dict(warmup_ratio=RATIO, output_type="latent")
        self.among = {(e, s): pipe.interpolate_among(self.stores[s], NAMES, w, early=e, **akw).clone()
                      for e in EARLY for s in ("native", "q8")}
        self.among_eager = pipe.interpolate_among(self.stores["native"], NAMES, w, early="fused_outer", use_graphs=False, **akw).clone()
        self.among_graphs = pipe.interpolate_among(self.stores["native"], NAMES, w, early="fused_outer", use_graphs=True, **akw).clone()
        self.in_runs = pipe.interpolate_among(self.stores["native"], NAMES, w, early="fused_outer", max_frames=2, **akw).clone()
        wp = torch.tensor([[1 - c, c] for c in PAIR_C])
        self.pair = {e: pipe.interpolate_among(self.stores["native"], ["tl", "br"], wp, early=e, **akw).clone() for e in EARLY}
        self.processors_after = dict(hip.attn_processors)
        # the fp64 loops (they read the processors installed on the HIP denoiser): the live grid, and the two-end-point run tl -> br
        dbl = [tuple(t.double() for t in pair) for pair in embs]
        ora = InterpolationStableDiffusionPipeline(CornerOracleDenoiser(hip), DDIMSchedulerLite())
        self.ref = {e: ora.interpolate_corners(lats.double(), embeds=dbl, early=e, **ckw).numpy() for e in EARLY}
        two = InterpolationStableDiffusionPipeline(OracleDenoiser(hip), DDIMSchedulerLite())
        self.ref_pair = {e: two.interpolate(lats[0:1].double(), lats[3:4].double(), size=5, coef=[0.0] + PAIR_C + [1.0],
                                            embeds_start=dbl[0], embeds_end=dbl[3], early=e, num_inference_steps=STEPS,
                                            warmup_ratio=RATIO, guidance_scale=gs, output_type="latent").numpy() for e in EARLY}
        pipe.load_aid(t=0.5, is_fused=True, atype="fused_outer")   # (the oracle runs toggled the shared processors)
        err = lambda out, e: rel_l2(to_np64(out[RENDER]), self.ref[e][RENDER])      # noqa: E731
        self.figures = {}
        for e in EARLY:
            self.figures[e] = dict(live=err(self.live[e], e), native=err(self.among[(e, "native")], e), q8=err(self.among[(e, "q8")], e),
                                   pair=rel_l2(to_np64(self.pair[e]), self.ref_pair[e][1:4]))
            print(f"[keyframe blend] {dtype} {e}: rel-L2 vs the fp64 loop, rendered cells: "
                  + ", ".join(f"{k} {v:.3e}" for k, v in self.figures[e].items()))
        print(f"[keyframe blend] {dtype}: stores {self.stores['native'].nbytes} / {self.stores['q8'].nbytes} bytes for 4 key frames")


_RUNS = {}


@pytest.fixture(params=[F16, F32], ids=["f16", "f32"])
def runs(request):
    if request.param not in _RUNS:
        _RUNS[request.param] = _Runs(request.param)
    return _RUNS[request.param]


@pytest.mark.parametrize("storage", ["native", "q8"])
@pytest.mark.parametrize("early", EARLY)
def test_a_grid_from_four_recorded_key_frames_against_the_oracle_loop_of_the_live_run(runs, early, storage):
    out = runs.among[(early, storage)]
    st = runs.stores[storage]
    assert out.shape == (9, 4, 8, 8) and bool(torch.isfinite(out).all())
    for cell, c in CORNER_CELLS.items():                     # the corner cells are the stored final latents, bit for bit
        assert torch.equal(_bits(out[cell:cell + 1]), _bits(st[NAMES[c]].final)), cell
    fig = runs.figures[early]
    bound = _bound(early, runs.dtype, storage)
    print(f"rendered cells {early} {storage}: blend {fig[storage]:.3e}, live run {fig['live']:.3e}, bound {bound:.3e}")
    assert fig[storage] < bound, (fig, bound)
    assert st.mode is None


@pytest.mark.parametrize("early", EARLY)
def test_two_key_frames_are_the_two_end_point_replay(runs, early):
    """M = 2 with rows (1 - c, c) against the fp64 loop of ``interpolate(tl, br, coef=[0, c.., 1])`` — the loop that bounds
    ``interpolate_between`` for that pair — within the bound of the grid."""
    fig = runs.figures[early]
    bound = _bound(early, runs.dtype, "native")
    print(f"pair (tl, br) {early}: blend {fig['pair']:.3e}, bound {bound:.3e}")
    assert runs.pair[early].shape == (3, 4, 8, 8) and fig["pair"] < bound, (fig, bound)


def test_max_frames_stays_within_the_bound_frame_by_frame(runs):
    out, ref = runs.in_runs, runs.ref["fused_outer"]
    bound = _bound("fused_outer", runs.dtype, "native")
    for cell, c in CORNER_CELLS.items():
        assert torch.equal(_bits(out[cell:cell + 1]), _bits(runs.stores["native"][NAMES[c]].final))
    for cell in RENDER:
        err = rel_l2(to_np64(out[cell]), ref[cell])
        print(f"max_frames=2, cell {cell}: {err:.3e} (bound {bound:.3e}; the live run's cell {rel_l2(to_np64(runs.live['fused_outer'][cell]), ref[cell]):.3e})")
        assert err < bound, (cell, err, bound)


def test_graphs_on_and_off_agree_and_the_processors_are_restored(runs):
    assert torch.equal(_bits(runs.among_graphs), _bits(runs.among_eager))
    assert runs.processors_after == runs.installed
    assert all(s.mode is None for s in runs.stores.values())


def test_refusals_on_the_device_path(runs):
    pipe, st, w = runs.pipe, runs.stores["native"], runs.w
    kw = dict(output_type="latent")
    installed = dict(pipe.unet.attn_processors)
    with pytest.raises(ValueError, match="different num_inference_steps"):      # a store recorded under another step count
        pipe.interpolate_among(st, NAMES, w, num_inference_steps=STEPS + 2, **kw)
    with pytest.raises(ValueError, match="too few aid_steps"):                  # a late AID mode needs every step recorded
        pipe.interpolate_among(st, NAMES, w, late="fused_outer", **kw)
    with pytest.raises(ValueError, match="1 .. 8 key frames; got 9"):
        pipe.interpolate_among(st, NAMES + [f"x{i}" for i in range(5)], torch.full((1, 9), 1 / 9), **kw)
    assert st.mode is None and dict(pipe.unet.attn_processors) == installed
    again = pipe.interpolate_among(st, NAMES, w, early="fused_outer", warmup_ratio=RATIO, **kw)
    assert torch.equal(_bits(again), _bits(runs.among[("fused_outer", "native")]))
