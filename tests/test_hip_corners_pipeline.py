"""GPU: ``interpolate_corners`` end to end over the stand-in denoiser (StackDenoiser("sd15") at its scaled-down size), HIP against the
same loop with every attention layer evaluated in fp64 (tests/corners_ref.py around the sublayer arithmetic of
tests/test_hip_depth_and_pipelines.py), graphs on and off, and a 2 x 2 grid whose four frames are the corners themselves.

Bound of the final latents.  The two-end-point ``interpolate`` at the same model size, dtype, step count, frame count, warm-up ratio
and guidance scale measures TWO_POINT (rel-L2 against its own fp64 loop, on an MI355X; ``test_two_end_point_baseline`` re-measures it
and holds it to 1.3 x that, the project's convention).  Three corners are two passes of the attention core per OUTER layer call: one
accumulating pass more, one rounding of ``out`` more per AID layer call — the corner run gets 2 x TWO_POINT.
Measured: two end points 7.64e-4 (fp16) / 6.52e-3 (bf16), three corners 7.29e-4 / 5.77e-3."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import aid_amd  # noqa: E402
import corners_ref as R  # noqa: E402
from aid_amd.pipelines import DDIMSchedulerLite, InterpolationStableDiffusionPipeline, StackDenoiser  # noqa: E402
from oracle import aid_oracle as O  # noqa: E402
from test_hip_depth_and_pipelines import OracleDenoiser, _embs, _oracle_layer, _w  # noqa: E402
from util import rel_l2, to_np64  # noqa: E402

DEV = "cuda:0"
STEPS, RATIO, GS = 4, 0.5, 2.0
TWO_POINT = {torch.float16: 7.64e-4, torch.bfloat16: 6.52e-3}     # measured: see the module docstring
ids_dt = lambda d: str(d).split(".")[-1]  # noqa: E731


class CornerOracleDenoiser(OracleDenoiser):
    """OracleDenoiser for corner processors: an activated layer is ``h + corners_processor(LayerNorm(h), ctx)`` in fp64, the riders
    of the call (the unconditional half) plain attention; a de-activated one the plain oracle layer."""

    def forward(self, sample, timestep=None, encoder_hidden_states=None, added_cond_kwargs=None, return_dict=False, **kw):
        st = self.hip.stack
        n = sample.shape[0]
        flat = sample.reshape(n, -1).double().numpy()
        tshift = 0.0 if timestep is None else float(timestep) * self.hip.time_scale
        hs = {}
        for (s, c) in st.level_shapes():
            tok = (flat @ to_np64(self.hip.lift[f"{s}_{c}"])).reshape(n, s, 8)
            hs[(s, c)] = np.tile(tok, (1, 1, c // 8)) + tshift
        ctx = encoder_hidden_states.double().numpy()
        assert ctx.shape[0] == n
        for i, (m, nrm, (s, c, heads, is_cross)) in enumerate(zip(st.layers, st.norms, st.shapes)):
            proc = m.processor
            h = hs[(s, c)]
            if not proc.activated:
                hs[(s, c)] = _oracle_layer(st, i, h, ctx, "plain", False, None)
                continue
            assert isinstance(proc, aid_amd.CornerInterpolatedAttnProcessor) and proc.ctx_index is None
            hn = O.layer_norm(h, to_np64(nrm.weight), to_np64(nrm.bias), nrm.eps)
            w = _w(m, heads)
            wts = np.concatenate([proc.weights.double().numpy(), np.zeros((proc.plain_tail, proc.weights.shape[1]))])
            hs[(s, c)] = h + R.corners_processor(hn, ctx if is_cross else None, w.wq, w.wk, w.wv, w.wo, w.bo, heads, proc.mode,
                                                 proc.is_fused, wts, proc.corner_rows, n_plain=proc.plain_tail)
        out = np.zeros_like(flat)
        for (s, c) in st.level_shapes():
            hm = hs[(s, c)].reshape(n, s, c // 8, 8).mean(axis=2)
            out = out + hm.reshape(n, s * 8) @ to_np64(self.hip.drop[f"{s}_{c}"])
        return (torch.from_numpy(out / len(st.level_shapes())).view_as(sample),)


def _setup(dtype, m, seed):
    hip = StackDenoiser("sd15", dtype=dtype, device=DEV, scale_down=16, latent_hw=(8, 8))
    g = torch.Generator().manual_seed(seed)
    lats = torch.randn(m, 4, 8, 8, generator=g).to(dtype)
    embs = [tuple(e.to(dtype).float() for e in _embs(g, 768)) for _ in range(m)]
    return hip, lats, embs


def _dbl(embs):
    return [tuple(e.double() for e in pair) for pair in embs]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=ids_dt)
def test_two_end_point_baseline(dtype):
    """What the corner bound is derived from: the two-end-point ``interpolate`` of six frames against its own fp64 loop."""
    hip, lats, embs = _setup(dtype, 2, 31)
    kw = dict(size=6, num_inference_steps=STEPS, warmup_ratio=RATIO, early="fused_outer", guidance_scale=GS, output_type="latent")
    out = InterpolationStableDiffusionPipeline(hip, DDIMSchedulerLite()).interpolate(lats[0:1], lats[1:2], embeds_start=embs[0],
                                                                                     embeds_end=embs[1], **kw)
    d = _dbl(embs)
    ref = InterpolationStableDiffusionPipeline(OracleDenoiser(hip), DDIMSchedulerLite()).interpolate(
        lats[0:1].double(), lats[1:2].double(), embeds_start=d[0], embeds_end=d[1], **kw)
    err = rel_l2(to_np64(out), ref.numpy())
    print(f"[corners-pipeline] two end points {ids_dt(dtype)}: rel-L2 {err:.3e}")
    assert err < 1.3 * TWO_POINT[dtype], err


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=ids_dt)
def test_three_corners_end_to_end_vs_fp64_loop(dtype):
    hip, lats, embs = _setup(dtype, 3, 32)
    w = aid_amd.simplex_weights(3, 2)                                # six frames, the corners at frames 0, 3 and 5
    kw = dict(weights=w, num_inference_steps=STEPS, warmup_ratio=RATIO, guidance_scale=GS, output_type="latent")
    pipe = InterpolationStableDiffusionPipeline(hip, DDIMSchedulerLite())
    out = pipe.interpolate_corners(lats, embeds=embs, use_graphs=True, **kw)
    eager = pipe.interpolate_corners(lats, embeds=embs, use_graphs=False, **kw)
    assert out.shape == (6, 4, 8, 8) and torch.isfinite(out).all()
    assert torch.equal(out, eager)                                   # graphs on and off: the same bits
    ora = InterpolationStableDiffusionPipeline(CornerOracleDenoiser(hip), DDIMSchedulerLite())
    ref = ora.interpolate_corners(lats.double(), embeds=_dbl(embs), **kw)
    err = rel_l2(to_np64(out), ref.numpy())
    print(f"[corners-pipeline] three corners {ids_dt(dtype)}: rel-L2 {err:.3e} (bound {2 * TWO_POINT[dtype]:.3e})")
    assert err < 2 * TWO_POINT[dtype], err


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=ids_dt)
def test_grid_of_corners_is_every_frame_run_alone(dtype):
    """grid_weights(2, 2): four frames, each a corner.  In fused OUTER a corner frame's own pass is plain attention (the fused
    shortcut) and the other pass adds 0 x its result: every frame is bit-equal to the same frame run alone through the plain
    processors (one frame and its unconditional rider, no AID step)."""
    hip, lats, embs = _setup(dtype, 4, 33)
    pipe = InterpolationStableDiffusionPipeline(hip, DDIMSchedulerLite())
    kw = dict(num_inference_steps=STEPS, guidance_scale=GS, output_type="latent")
    out = pipe.interpolate_corners(lats, embeds=embs, weights=aid_amd.grid_weights(2, 2), warmup_ratio=RATIO, **kw)
    for j in range(4):
        alone = pipe.interpolate_corners(lats[j:j + 1], embeds=[embs[j]], weights=torch.ones(1, 1), warmup_ratio=0.0, **kw)
        assert torch.equal(out[j], alone[0]), (j, rel_l2(to_np64(out[j]), to_np64(alone[0])))
