"""Corner-weighted AID: the host side, without a GPU.

The weight helpers, the nested slerp, ``interpolate_corners`` (both pipeline classes) over the recording stub UNet of
tests/test_pipelines.py — batch layout, corner rows, guide prompt, warm-up toggling, every refusal — the device-buffer bookkeeping of
``CornerInterpolatedAttnProcessor.weights``, and the fp64 reference of the corner tests (tests/corners_ref.py) against the oracle of the
two-end-point form."""
import numpy as np
import pytest
import torch

import aid_amd
import corners_ref
from aid_amd.pipelines import DDIMSchedulerLite, InterpolationStableDiffusionPipeline, InterpolationStableDiffusionXLPipeline
from oracle import aid_oracle
from test_pipelines import RecordingUNet, _manual


# ---- weight helpers ----------------------------------------------------------------------------------------------------------------
def _is_one_hot(row, c):
    return float(row[c]) == 1.0 and int((row != 0).sum()) == 1


@pytest.mark.parametrize("rows,cols", [(2, 2), (3, 4), (1, 2), (2, 1), (1, 1), (5, 1)])
def test_grid_weights(rows, cols):
    w = aid_amd.grid_weights(rows, cols)
    assert tuple(w.shape) == (rows * cols, 4) and w.dtype == torch.float32
    assert bool((w >= 0).all()) and torch.allclose(w.sum(1), torch.ones(rows * cols), atol=1e-6)
    # corners TL, TR, BL, BR sit at the grid's corners, exactly one-hot — where the grid has that corner
    assert _is_one_hot(w[0], 0)
    if cols > 1:
        assert _is_one_hot(w[cols - 1], 1)
    if rows > 1:
        assert _is_one_hot(w[(rows - 1) * cols], 2)
    if rows > 1 and cols > 1:
        assert _is_one_hot(w[rows * cols - 1], 3)
    if rows == 1:            # one row: the top edge, a lerp between TL and TR
        assert bool((w[:, 2:] == 0).all())
        assert torch.allclose(w[:, 1], torch.linspace(0, 1, cols) if cols > 1 else torch.zeros(1))
    if cols == 1:            # one column: the left edge
        assert bool((w[:, 1] == 0).all()) and bool((w[:, 3] == 0).all())
    if (rows, cols) == (3, 4):
        assert torch.allclose(w[1 * 4 + 1], torch.tensor([0.5 * 2 / 3, 0.5 / 3, 0.5 * 2 / 3, 0.5 / 3]))
    with pytest.raises(ValueError):
        aid_amd.grid_weights(0, 2)


@pytest.mark.parametrize("m,steps", [(1, 1), (2, 4), (3, 2), (3, 3), (4, 2), (8, 1)])
def test_simplex_weights(m, steps):
    from math import comb
    w = aid_amd.simplex_weights(m, steps)
    assert tuple(w.shape) == (comb(steps + m - 1, m - 1), m) and w.dtype == torch.float32
    assert bool((w >= 0).all()) and torch.allclose(w.sum(1), torch.ones(w.shape[0]), atol=1e-6)
    assert len({tuple(r) for r in w.tolist()}) == w.shape[0]                    # distinct lattice points
    assert torch.allclose(torch.round(w * steps), w * steps, atol=1e-6)          # multiples of 1 / steps
    for c in range(m):
        assert sum(_is_one_hot(r, c) for r in w) == 1
    if (m, steps) == (2, 4):
        assert torch.allclose(w[:, 1], torch.linspace(0, 1, 5))
    with pytest.raises(ValueError):
        aid_amd.simplex_weights(0, 2)


def test_nested_slerp():
    g = torch.Generator().manual_seed(3)
    xs = [torch.randn(1, 4, 8, 8, generator=g) for _ in range(4)]
    for c in (0.0, 0.25, 0.5, 0.9, 1.0):
        assert torch.allclose(aid_amd.nested_slerp(xs[:2], [1 - c, c]), aid_amd.slerp(xs[0], xs[1], c), atol=1e-6, rtol=0)
    # identical corners: x, whatever the weights
    for w in ([0.2, 0.3, 0.5], [0.0, 0.0, 1.0], [1 / 3, 1 / 3, 1 / 3]):
        assert torch.allclose(aid_amd.nested_slerp([xs[0]] * 3, w), xs[0], atol=1e-6)
    # a one-hot row is the corner itself, bit for bit; leading zero weights are skipped
    for m in range(4):
        assert torch.equal(aid_amd.nested_slerp(xs, [1.0 if i == m else 0.0 for i in range(4)]), xs[m])
    assert torch.allclose(aid_amd.nested_slerp(xs, [0.0, 0.0, 0.6, 0.4]), aid_amd.slerp(xs[2], xs[3], 0.4), atol=1e-6)
    # the chain: slerp(slerp(x0, x1, w1 / (w0 + w1)), x2, w2)
    want = aid_amd.slerp(aid_amd.slerp(xs[0], xs[1], 0.3 / 0.5), xs[2], 0.5)
    assert torch.allclose(aid_amd.nested_slerp(xs[:3], [0.2, 0.3, 0.5]), want, atol=1e-6)
    with pytest.raises(ValueError):
        aid_amd.nested_slerp(xs[:3], [0.5, 0.5])


# ---- interpolate_corners over the recording stub ------------------------------------------------------------------------------------
class CornerRecordingUNet(RecordingUNet):
    """RecordingUNet that also notes the corner processors' rows, weights and mode of every call."""

    def forward(self, sample, t, encoder_hidden_states=None, added_cond_kwargs=None, return_dict=False):
        procs = [p for p in self.attn_processors.values() if isinstance(p, aid_amd.CornerInterpolatedAttnProcessor)]
        out = super().forward(sample, t, encoder_hidden_states, added_cond_kwargs, return_dict)
        self.calls[-1].update(n_corner_procs=len(procs), n_procs=len(self.attn_processors), ctx_rows=encoder_hidden_states.shape[0],
                              rows=procs[0].corner_rows if procs else None, weights=procs[0].weights.clone() if procs else None,
                              mode=(procs[0].mode, procs[0].is_fused) if procs else None)
        return out


def _corner_inputs(m, seed, xl=False):
    g = torch.Generator().manual_seed(seed)
    lats = torch.randn(m, 4, 4, 4, generator=g)
    mk = lambda: (torch.randn(1, 7, 12, generator=g), torch.randn(1, 7, 12, generator=g)) + \
        ((torch.randn(1, 6, generator=g), torch.randn(1, 6, generator=g)) if xl else ())      # noqa: E731
    return lats, [mk() for _ in range(m)], mk()


def _mix(ts, w):
    return torch.cat([torch.tensordot(w[i], torch.cat(ts), dims=1).unsqueeze(0) for i in range(w.shape[0])])


def test_interpolate_corners_layout_corner_rows_and_toggling():
    unet = CornerRecordingUNet()
    pipe = InterpolationStableDiffusionPipeline(unet, DDIMSchedulerLite())
    pipe.load_aid(t=0.5, is_fused=True, atype="fused_inner")
    installed = dict(unet.attn_processors)
    lats, embs, _ = _corner_inputs(3, 5)
    w = aid_amd.simplex_weights(3, 2)                                           # 6 frames; corners at frames 0, 3, 5
    lat = pipe.interpolate_corners(lats, embeds=embs, weights=w, num_inference_steps=8, warmup_ratio=0.5, guidance_scale=2.0,
                                   output_type="latent")
    assert lat.shape == (6, 4, 4, 4)
    calls = unet.calls
    assert len(calls) == 8 and all(c["n"] == 12 and c["ctx_rows"] == 12 for c in calls)      # ONE call per step: [cond 6 ; uncond 6]
    assert [c["active"] for c in calls] == [True] * 4 + [False] * 4
    assert [c["tail"] for c in calls] == [6] * 4 + [0] * 4                      # the uncond half rides as plain_tail
    assert all(c["n_corner_procs"] == c["n_procs"] for c in calls)
    assert all(c["rows"] == [0, 3, 5] and c["mode"] == ("outer", True) and torch.equal(c["weights"], w) for c in calls)
    assert all(c["ctx_index"] is None for c in calls)
    cond, unc = _mix([e[0] for e in embs], w), _mix([e[1] for e in embs], w)
    lat0 = torch.cat([aid_amd.nested_slerp([lats[i:i + 1] for i in range(3)], w[i]) for i in range(6)])
    assert torch.equal(lat0[3], lats[1]) and torch.equal(lat0[5], lats[2])
    want = _manual(lat0, cond, unc, 8, 0.5, 2.0, DDIMSchedulerLite())
    assert torch.allclose(lat, want, atol=1e-5)
    assert dict(unet.attn_processors) == installed                              # what load_aid installed is back
    # frame_latents overrides the nested slerp; late = an AID mode keeps the processors on; inner / pure from `early`
    unet.calls.clear()
    fl = torch.randn(6, 4, 4, 4, generator=torch.Generator().manual_seed(9))
    lat = pipe.interpolate_corners(lats, embeds=embs, weights=w, frame_latents=fl, num_inference_steps=4, warmup_ratio=0.5,
                                   early="pure_inner", late="fused_outer", guidance_scale=2.0, output_type="latent")
    assert [c["mode"] for c in unet.calls] == [("inner", False)] * 2 + [("outer", True)] * 2
    assert all(c["active"] and c["tail"] == 6 for c in unet.calls)
    assert torch.allclose(lat, _manual(fl, cond, unc, 4, 1.0, 2.0, DDIMSchedulerLite()), atol=1e-5)


def test_interpolate_corners_guide_prompt_shares_one_context():
    unet = CornerRecordingUNet()
    pipe = InterpolationStableDiffusionPipeline(unet, DDIMSchedulerLite())
    lats, embs, guide = _corner_inputs(3, 6)
    w = aid_amd.simplex_weights(3, 2)
    lat = pipe.interpolate_corners(lats, embeds=embs, weights=w, embeds_guide=guide, num_inference_steps=4, guidance_scale=2.0,
                                   output_type="latent")
    calls = unet.calls
    # four distinct contexts per pass: the three corners', then the guide's, shared by every frame that is not a corner
    assert all(c["ctx_rows"] == 12 and c["ctx_index"] == [0, 3, 3, 1, 3, 2, 4, 7, 7, 5, 7, 6] for c in calls)
    hot = [0, None, None, 1, None, 2]
    cond = torch.cat([guide[0] if o is None else embs[o][0] for o in hot])
    unc = torch.cat([guide[1] if o is None else embs[o][1] for o in hot])
    lat0 = torch.cat([aid_amd.nested_slerp([lats[i:i + 1] for i in range(3)], w[i]) for i in range(6)])
    assert torch.allclose(lat, _manual(lat0, cond, unc, 4, 0.5, 2.0, DDIMSchedulerLite()), atol=1e-5)
    # a 2 x 2 grid has no frame that is not a corner: the guide prompt has nobody to guide, one context per frame
    unet.calls.clear()
    lats4, embs4, _ = _corner_inputs(4, 7)
    pipe.interpolate_corners(lats4, embeds=embs4, weights=aid_amd.grid_weights(2, 2), embeds_guide=guide, num_inference_steps=2,
                             output_type="latent")
    assert all(c["ctx_index"] is None and c["n"] == 8 and c["rows"] == [0, 1, 2, 3] for c in unet.calls)


def test_interpolate_corners_xl_mixes_the_pooled_embeddings():
    unet = CornerRecordingUNet()
    seen = []
    orig = unet.forward

    def spy(sample, t, encoder_hidden_states=None, added_cond_kwargs=None, return_dict=False):
        seen.append(added_cond_kwargs["text_embeds"].clone())
        return orig(sample, t, encoder_hidden_states, added_cond_kwargs, return_dict)
    unet.forward = spy
    pipe = InterpolationStableDiffusionXLPipeline(unet, DDIMSchedulerLite())
    lats, embs, _ = _corner_inputs(3, 8, xl=True)
    w = torch.tensor([[1, 0, 0], [0, 1, 0], [0.25, 0.25, 0.5], [0, 0, 1]], dtype=torch.float32)
    out = pipe.interpolate_corners(lats, embeds=embs, weights=w, num_inference_steps=2, output_type="latent")
    assert out.shape == (4, 4, 4, 4) and pipe.guidance_scale == 5.0
    assert all(c["added"] == ["text_embeds", "time_ids"] and c["rows"] == [0, 1, 3] for c in unet.calls)
    want = torch.cat([_mix([e[2] for e in embs], w), _mix([e[3] for e in embs], w)])
    assert torch.allclose(seen[0], want, atol=1e-6) and torch.equal(seen[0][1], embs[1][2][0])


def test_interpolate_corners_refusals():
    unet = CornerRecordingUNet()
    pipe = InterpolationStableDiffusionPipeline(unet, DDIMSchedulerLite())
    lats, embs, _ = _corner_inputs(3, 10)
    good = aid_amd.simplex_weights(3, 2)
    run = lambda w_, **kw: pipe.interpolate_corners(lats, embeds=embs, weights=w_, num_inference_steps=2, output_type="latent", **kw)  # noqa: E731
    bad = good.clone()
    bad[1] = torch.tensor([0.7, 0.5, -0.2])
    with pytest.raises(ValueError, match="row 1"):
        run(bad)
    bad = good.clone()
    bad[4] = torch.tensor([0.0, 0.5, 0.6])
    with pytest.raises(ValueError, match="row 4"):
        run(bad)
    bad = good.clone()
    bad[3] = torch.tensor([0.0, 0.999, 0.001])                                  # nearly one-hot is not the corner frame
    with pytest.raises(ValueError, match="corner 1"):
        run(bad)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        run(aid_amd.grid_weights(2, 2))
    with pytest.raises(ValueError, match="weights"):
        run(None)
    with pytest.raises(ValueError, match="per corner"):
        pipe.interpolate_corners(lats, embeds=embs[:2], weights=good, num_inference_steps=2)
    with pytest.raises(ValueError, match="frame_latents"):
        run(good, frame_latents=torch.zeros(5, 4, 4, 4))
    with pytest.raises(ValueError, match="early"):
        run(good, early="nope")
    with pytest.raises(ValueError, match="1 .. 8"):
        pipe.interpolate_corners(torch.zeros(9, 4, 4, 4), embeds=embs * 3, weights=torch.eye(9), num_inference_steps=2)
    for name in ("image_start", "image_end", "image_embeds_end", "ip_adapter_image"):
        with pytest.raises(NotImplementedError, match="image"):
            run(good, **{name: object()})
    with pytest.raises(TypeError):
        run(good, size=7)
    assert not unet.calls                                                       # every refusal came before the first UNet call
    # a UNet with IP-Adapter layers
    ip_unet = aid_amd.AttnStackUNet("sd15", dtype=torch.float32, scale_down=64, channel_div=8)
    ip_unet.load_ip_adapter(num_tokens=4, scale=0.5)
    before = dict(ip_unet.attn_processors)
    with pytest.raises(NotImplementedError, match="IP-Adapter"):
        aid_amd.loop.install_corner_processors(ip_unet, good, [0, 3, 5])
    assert dict(ip_unet.attn_processors) == before


# ---- the processor ------------------------------------------------------------------------------------------------------------------
def test_processor_weights_buffer_is_rewritten_in_place():
    w = aid_amd.simplex_weights(3, 2)
    p = aid_amd.CornerInterpolatedAttnProcessor(w.clone(), [0, 3, 5], mode="outer", is_fused=True)
    assert isinstance(p, aid_amd.InterpolatedAttnProcessor) and p.size == 6 and p.activated and p.plain_tail == 0
    assert not p.weights.is_cuda and tuple(p.weights.shape) == (6, 3)
    cpu = torch.device("cpu")
    buf = p._weights_device(cpu, 6)
    ptr = buf.data_ptr()
    assert buf.dtype == torch.float32 and torch.equal(buf, w)
    new = w.clone()
    new[1] = torch.tensor([0.1, 0.2, 0.7])
    p.weights = new                                                             # assignment: the buffer is brought up to date at once
    assert buf.data_ptr() == ptr and torch.equal(buf, new)
    p.weights[2, 0], p.weights[2, 2] = 0.25, 0.75                               # in-place edit: seen at the next call
    assert p._weights_device(cpu, 6) is buf and buf.data_ptr() == ptr
    assert buf[2].tolist() == [0.25, 0.0, 0.75]
    # riders: another layout, its own buffer, rows of the riders zero; the batch must fit
    p.plain_tail = 6
    both = p._weights_device(cpu, 12)
    assert both.data_ptr() != ptr and tuple(both.shape) == (12, 3) and torch.equal(both[:6], buf) and not both[6:].any()
    p.weights = w.clone()
    assert torch.equal(buf, w) and torch.equal(both[:6], w)                     # every layout follows an assignment
    with pytest.raises(RuntimeError, match="must match"):
        p._weights_device(cpu, 11)
    for bad in (w[:5], -w, torch.full((6, 3), float("nan")), w[:, :2]):
        with pytest.raises(ValueError):
            p.weights = bad
    with pytest.raises(ValueError):
        aid_amd.CornerInterpolatedAttnProcessor(torch.eye(9), list(range(9)))
    with pytest.raises(ValueError):
        aid_amd.CornerInterpolatedAttnProcessor(w, [0, 3, 6])
    with pytest.raises(ValueError):
        aid_amd.CornerInterpolatedAttnProcessor(w, [0, 3, 5], mode="plain")
    p.deactivate()
    assert not p.activated
    p.activate(0.3)
    assert p.activated and torch.equal(p.weights, w)


def test_processor_refusals():
    w = aid_amd.grid_weights(2, 2)
    attn = aid_amd.AttnShim(64, 1, 64)
    x, ctx = torch.zeros(4, 16, 64), torch.zeros(4, 7, 64)

    def proc():
        return aid_amd.CornerInterpolatedAttnProcessor(w, [0, 1, 2, 3])
    with pytest.raises(RuntimeError, match="no CPU path"):
        proc()(attn, x)
    with pytest.raises(NotImplementedError, match="IP-Adapter"):
        proc()(attn, x, (ctx, [torch.zeros(4, 4, 64)]))
    for name in ("endpoint_store", "keyframe_store", "endpoint_exchange"):
        p = proc()
        setattr(p, name, object())
        with pytest.raises(NotImplementedError):
            p(attn, x)
    p = proc()
    p.plain_tail = 3
    with pytest.raises(RuntimeError, match="must match"):
        p(attn, x)


# ---- the reference of the corner tests against the two-end-point oracle ----------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "pure"])
@pytest.mark.parametrize("mode", ["outer", "inner"])
def test_corners_ref_is_the_oracle_for_two_corners(mode, fused):
    rng = np.random.default_rng(11)
    n, s, l, heads, d = 5, 9, 11, 2, 8
    q = rng.standard_normal((n, s, heads * d))
    k = rng.standard_normal((n, l, heads * d))
    v = rng.standard_normal((n, l, heads * d))
    c = np.array([0.0, 0.3, 0.55, 0.8, 1.0])
    w = np.stack([1 - c, c], axis=1)
    want = aid_oracle.attn_core(q, k, v, heads, d ** -0.5, mode, fused, c, 0, n - 1)
    got = corners_ref.corners_core(q, k, v, heads, d ** -0.5, mode, fused, w, [0, n - 1])
    assert np.abs(got - want).max() <= 1e-12
    # riders are plain attention, their weight rows unread; swapped corners with swapped weights are the same frames
    plain = aid_oracle.attn_core(q, k, v, heads, d ** -0.5, "plain", False, None)
    w_nan = w.copy()
    w_nan[3:] = np.nan
    got = corners_ref.corners_core(q, k, v, heads, d ** -0.5, mode, fused, w_nan[:, ::-1], [n - 1, 0], n_plain=2)
    assert np.abs(got[:3] - want[:3]).max() <= 1e-12 and np.abs(got[3:] - plain[3:]).max() <= 1e-12
