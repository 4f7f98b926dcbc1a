"""Key-frame blend: the host side, without a GPU.

``KeyframeStore.among`` / ``KeyframeBlend`` (validation, ``kf_args`` in blend mode for native and q8 stores, the refusals of
``begin_replay``) and ``interpolate_among`` (both pipeline classes) over the recording stub UNet of tests/test_pipelines.py — weight-row
validation, one-hot rows that are not rendered, ``max_frames`` grouping, guide prompt, the image keyword refusal and the restoration of
the processors after an exception.  The toy denoiser has no attention call: the processors' state alone is observed."""
import pytest
import torch

import aid_amd
from aid_amd import ops
from aid_amd.keyframe_store import Keyframe, KeyframeBlend, KeyframeStore
from test_pipelines import RecordingUNet, _manual


# ---- KeyframeStore.among / KeyframeBlend --------------------------------------------------------------------------------------------
SETTINGS = dict(num_inference_steps=6, guidance_scale=7.5, dtype=torch.float16, f32_precision=None, timesteps=(5, 4, 3, 2, 1, 0),
                lora=None, unet=1)


def _filled(names, storage="native", n_steps=3, l=12, c=16, dtype=torch.float16):
    """A store that holds ``names`` with one layer "L" of [l, c] keys, as a recording leaves it (CPU tensors: nothing is launched)."""
    st = KeyframeStore(storage=storage)
    k_fs, vt_fs = ops.endpoint_block_sizes(l, c)
    st.settings, st.n_steps = dict(SETTINGS), n_steps
    for i, n in enumerate(names):
        f = Keyframe()
        if storage == "q8":
            f.layers["L"] = (torch.zeros(n_steps, ops.q8_block_bytes(k_fs), dtype=torch.uint8),
                             torch.zeros(n_steps, ops.q8_block_bytes(vt_fs), dtype=torch.uint8))
        else:
            f.layers["L"] = (torch.zeros(n_steps, k_fs, dtype=dtype), torch.zeros(n_steps, vt_fs, dtype=dtype))
        f.latent, f.final, f.embeds = torch.full((1, 4, 2, 2), float(i)), torch.full((1, 4, 2, 2), 10.0 + i), ()
        st.frames[n] = f
    return st


def test_among_takes_one_to_eight_distinct_recorded_names():
    names = [f"k{i}" for i in range(9)]
    st = _filled(names)
    b = st.among(["k2", "k0", "k5"])
    assert isinstance(b, KeyframeBlend) and b.names == ("k2", "k0", "k5") and b.store is st and b.recorded and b.n_steps == 3
    assert st.among(["k1"]).names == ("k1",) and len(st.among(names[:8]).names) == 8
    assert torch.equal(b.latents, torch.cat([st[n].final for n in ("k2", "k0", "k5")])) and b.latents.shape[0] == 3
    with pytest.raises(KeyError, match="holds no frame 'zz'"):
        st.among(["k0", "zz"])
    with pytest.raises(ValueError, match="distinct"):
        st.among(["k0", "k1", "k0"])
    with pytest.raises(ValueError, match="1 .. 8 key frames; got 9"):
        st.among(names)
    with pytest.raises(ValueError, match="1 .. 8 key frames; got 0"):
        st.among([])
    with pytest.raises(ValueError, match="sequence of key-frame names"):
        st.among("k0")


@pytest.mark.parametrize("storage", ["native", "q8"])
def test_kf_args_in_blend_mode_names_the_stores_in_weight_column_order(storage):
    st = _filled(["a", "b", "c", "d"], storage)
    b = st.among(["c", "a", "d"])
    sig = dict(SETTINGS, warmup_ratio=0.5, late="self")
    with pytest.raises(RuntimeError, match="outside a run"):
        b.kf_args("L", 12, 16, torch.float16, torch.device("cpu"))
    b.begin_replay(sig, torch.device("cpu"))
    assert st.mode == "blend" and b.mode == "blend"
    kf = b.kf_args("L", 12, 16, torch.float16, torch.device("cpu"))
    assert kf["mode"] == "blend" and kf["step"] is st._step and (kf.get("storage") == "q8") == (storage == "q8")
    assert ("storage" in kf) == (storage == "q8")
    assert len(kf["entries"]) == 3
    for (k_, v_, row), name in zip(kf["entries"], ("c", "a", "d")):
        assert k_ is st[name].layers["L"][0] and v_ is st[name].layers["L"][1] and row == 0
    b.set_step(2)
    assert st.step == 2
    # every entry goes through _check_block: another resolution is refused, whichever entry it is
    with pytest.raises(ValueError, match="another resolution"):
        b.kf_args("L", 16, 16, torch.float16, torch.device("cpu"))
    st["d"].layers["L"] = (st["d"].layers["L"][0][:, :-16].contiguous(), st["d"].layers["L"][1])
    with pytest.raises(ValueError, match="layer 'L'"):
        b.kf_args("L", 12, 16, torch.float16, torch.device("cpu"))
    with pytest.raises(RuntimeError, match="holds no rows of layer 'M'"):
        b.kf_args("M", 12, 16, torch.float16, torch.device("cpu"))
    b.abort()
    assert st.mode is None and st._pair is None


def test_begin_replay_refuses_other_settings_too_few_aid_steps_and_a_store_in_use():
    st = _filled(["a", "b", "c"])
    b = st.among(["a", "b", "c"])
    sig = dict(SETTINGS, warmup_ratio=0.5, late="self")
    with pytest.raises(ValueError, match="different num_inference_steps"):
        b.begin_replay(dict(sig, num_inference_steps=8), torch.device("cpu"))
    with pytest.raises(ValueError, match="different guidance_scale"):
        b.begin_replay(dict(sig, guidance_scale=3.0), torch.device("cpu"))
    with pytest.raises(ValueError, match="different dtype"):
        b.begin_replay(dict(sig, dtype=torch.bfloat16), torch.device("cpu"))
    # int(6 * 0.5) = 3 AID steps are recorded: a ratio of 0.7 needs 4, a late AID mode all 6
    with pytest.raises(ValueError, match="too few aid_steps: this run needs 4"):
        b.begin_replay(dict(sig, warmup_ratio=0.7), torch.device("cpu"))
    with pytest.raises(ValueError, match="too few aid_steps: this run needs 6"):
        b.begin_replay(dict(sig, late="fused_outer"), torch.device("cpu"))
    assert st.mode is None
    b.begin_replay(sig, torch.device("cpu"))
    with pytest.raises(RuntimeError, match="in use by another run"):
        st.among(["a", "b"]).begin_replay(sig, torch.device("cpu"))
    with pytest.raises(RuntimeError, match="in use by another run"):
        st.between("a", "b").begin_replay(sig, torch.device("cpu"))
    b.abort()
    st.between("a", "b").begin_replay(sig, torch.device("cpu"))          # the pair form is what it was
    assert st.mode == "replay" and st._pair == ("a", "b")
    st.abort()


# ---- interpolate_among over the recording stub ---------------------------------------------------------------------------------------
class BlendRecordingUNet(RecordingUNet):
    """RecordingUNet that also notes the blend processors' weights, mode, key frames and layer names of every call."""

    def forward(self, sample, t, encoder_hidden_states=None, added_cond_kwargs=None, return_dict=False):
        procs = {k: p for k, p in self.attn_processors.items() if isinstance(p, aid_amd.KeyframeBlendAttnProcessor)}
        out = super().forward(sample, t, encoder_hidden_states, added_cond_kwargs, return_dict)
        first = next(iter(procs.values())) if procs else None
        self.calls[-1].update(n_blend_procs=len(procs), n_procs=len(self.attn_processors), ctx_rows=encoder_hidden_states.shape[0],
                              weights=None if first is None else first.weights.clone(),
                              mode=None if first is None else (first.mode, first.is_fused),
                              names=None if first is None else first.blend.names,
                              layers_ok=all(p.endpoint_layer == k for k, p in procs.items()),
                              corner_ctx=None if first is None else first.corner_ctx,
                              store_mode=None if first is None else first.blend.store.mode, step=None if first is None else first.blend.store.step)
        return out


def _recorded(xl=False, k=4, steps=4, seed=6):
    unet = BlendRecordingUNet()
    cls = aid_amd.InterpolationStableDiffusionXLPipeline if xl else aid_amd.InterpolationStableDiffusionPipeline
    pipe = cls(unet, aid_amd.DDIMSchedulerLite())
    pipe.load_aid(t=0.5, is_fused=True, atype="fused_outer")
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(k, 4, 4, 4, generator=g)
    mk = lambda: (torch.randn(1, 7, 12, generator=g), torch.randn(1, 7, 12, generator=g)) + \
        ((torch.randn(1, 6, generator=g), torch.randn(1, 6, generator=g)) if xl else ())      # noqa: E731
    emb = [mk() for _ in range(k)]
    names = [f"k{i}" for i in range(k)]
    st = KeyframeStore()
    pipe.record_keyframes(st, names, lat, embeds=emb, num_inference_steps=steps, output_type="latent")
    del unet.calls[:]
    return unet, pipe, st, names, lat, emb


def _mix(ts, w):
    return torch.cat([torch.tensordot(w[i], torch.cat(ts), dims=1).unsqueeze(0) for i in range(w.shape[0])])


@pytest.mark.parametrize("xl", [False, True], ids=["sd", "sdxl"])
def test_a_grid_renders_its_inner_cells_only_and_takes_the_corner_cells_from_the_store(xl):
    unet, pipe, st, names, lat, emb = _recorded(xl)
    installed = dict(unet.attn_processors)
    steps, gs = 4, pipe.default_guidance_scale
    w = aid_amd.grid_weights(3, 3)                                             # corner cells 0, 2, 6, 8 are exactly one-hot
    out = pipe.interpolate_among(st, names, w, output_type="latent")
    assert out.shape == (9, 4, 4, 4)
    for cell, c in ((0, 0), (2, 1), (6, 2), (8, 3)):
        assert torch.equal(out[cell:cell + 1], st[names[c]].final)
    calls = unet.calls
    render = [1, 3, 4, 5, 7]
    # ONE call per step over the five rendered frames and their riders; AID on for int(4 * 0.5) steps; no key frame in the batch
    assert [c["n"] for c in calls] == [10] * steps and all(c["ctx_rows"] == 10 for c in calls)
    assert [c["active"] for c in calls] == [True, True, False, False] and [c["tail"] for c in calls] == [5, 5, 0, 0]
    assert all(c["n_blend_procs"] == c["n_procs"] and c["layers_ok"] and c["names"] == tuple(names) for c in calls)
    assert all(torch.equal(c["weights"], w[render]) and c["mode"] == ("outer", True) and c["ctx_index"] is None for c in calls)
    assert all(c["store_mode"] == "blend" for c in calls) and [c["step"] for c in calls[:2]] == [0, 1]
    assert all(torch.equal(c["corner_ctx"], torch.cat([e[0] for e in emb])) for c in calls)
    if xl:
        assert all(c["added"] == ["text_embeds", "time_ids"] for c in calls)
    # (the toy denoiser has no attention: a rendered cell is the plain loop on its mixed inputs)
    cond, unc = _mix([e[0] for e in emb], w[render]), _mix([e[1] for e in emb], w[render])
    lat0 = torch.cat([aid_amd.nested_slerp([lat[i:i + 1] for i in range(4)], w[i]) for i in render])
    want = _manual(lat0, cond, unc, steps, 0.5, gs, aid_amd.DDIMSchedulerLite())
    assert torch.allclose(out[render], want, atol=1e-5)
    assert dict(unet.attn_processors) == installed and st.mode is None
    # frame_latents overrides the nested slerp; another early mode; a late AID mode needs every step recorded
    del unet.calls[:]
    fl = torch.randn(9, 4, 4, 4, generator=torch.Generator().manual_seed(9))
    out2 = pipe.interpolate_among(st, names, w, frame_latents=fl, early="pure_inner", output_type="latent")
    assert all(c["mode"] == ("inner", False) for c in unet.calls)
    assert torch.allclose(out2[render], _manual(fl[render], cond, unc, steps, 0.5, gs, aid_amd.DDIMSchedulerLite()), atol=1e-5)
    with pytest.raises(ValueError, match="too few aid_steps"):
        pipe.interpolate_among(st, names, w, late="fused_outer", output_type="latent")
    with pytest.raises(ValueError, match="frame_latents must be"):
        pipe.interpolate_among(st, names, w, frame_latents=fl[:5], output_type="latent")
    assert dict(unet.attn_processors) == installed and st.mode is None


def test_max_frames_renders_in_runs_and_joins_them_in_weight_row_order():
    unet, pipe, st, names, lat, emb = _recorded()
    w = aid_amd.grid_weights(3, 3)
    whole = pipe.interpolate_among(st, names, w, output_type="latent")
    del unet.calls[:]
    parts = pipe.interpolate_among(st, names, w, max_frames=2, output_type="latent")
    # five rendered frames in runs of 2, 2, 1 — each with its riders, four steps each
    assert [c["n"] for c in unet.calls] == [4] * 4 + [4] * 4 + [2] * 4
    got = [c["weights"] for c in unet.calls[::4]]
    assert torch.equal(got[0], w[[1, 3]]) and torch.equal(got[1], w[[4, 5]]) and torch.equal(got[2], w[[7]])
    assert torch.allclose(parts, whole, atol=1e-6) and torch.equal(parts[[0, 2, 6, 8]], whole[[0, 2, 6, 8]])
    with pytest.raises(ValueError, match="max_frames"):
        pipe.interpolate_among(st, names, w, max_frames=0)
    # every row one-hot: nothing is rendered
    del unet.calls[:]
    only = pipe.interpolate_among(st, names[:2], torch.eye(2)[[1, 0, 1]], output_type="latent")
    assert not unet.calls and torch.equal(only, torch.cat([st["k1"].final, st["k0"].final, st["k1"].final]))


def test_a_guide_prompt_gives_every_rendered_frame_the_guides_context():
    unet, pipe, st, names, lat, emb = _recorded()
    g = torch.Generator().manual_seed(2)
    guide = (torch.randn(1, 7, 12, generator=g), torch.randn(1, 7, 12, generator=g))
    w = aid_amd.simplex_weights(3, 2)                                          # 6 frames, three of them key frames
    out = pipe.interpolate_among(st, names[:3], w, embeds_guide=guide, output_type="latent")
    assert out.shape == (6, 4, 4, 4)
    assert all(c["n"] == 6 and c["ctx_rows"] == 6 and c["ctx_index"] == [0, 0, 0, 1, 1, 1] for c in unet.calls)


def test_weight_rows_are_validated_and_named():
    unet, pipe, st, names, lat, emb = _recorded()
    bad = aid_amd.grid_weights(2, 2).clone()
    with pytest.raises(ValueError, match=r"weights must be \[N, 3\]"):
        pipe.interpolate_among(st, names[:3], bad)
    bad[2, 0] = -0.25
    with pytest.raises(ValueError, match="weights row 2 has a negative"):
        pipe.interpolate_among(st, names, bad)
    bad = aid_amd.grid_weights(2, 2).clone()
    bad[1] = torch.tensor([0.5, 0.25, 0.0, 0.0])
    with pytest.raises(ValueError, match="weights row 1 sums to 0.75"):
        pipe.interpolate_among(st, names, bad)
    bad[1] = torch.tensor([float("nan"), 0.0, 0.0, 0.0])
    with pytest.raises(ValueError, match="weights row 1 has a negative or non-finite"):
        pipe.interpolate_among(st, names, bad)
    with pytest.raises(ValueError, match="pass weights"):
        pipe.interpolate_among(st, names, None)
    with pytest.raises(KeyError, match="holds no frame 'nope'"):
        pipe.interpolate_among(st, ["k0", "nope"], torch.eye(2))
    with pytest.raises(ValueError, match="1 .. 8 key frames"):
        pipe.interpolate_among(st, [], torch.zeros(1, 0))
    with pytest.raises(ValueError, match="early / late"):
        pipe.interpolate_among(st, names, aid_amd.grid_weights(2, 2), early="outer")
    assert not unet.calls and st.mode is None


def test_settings_that_differ_from_the_recordings_raise():
    unet, pipe, st, names, lat, emb = _recorded()
    w = aid_amd.grid_weights(2, 3)
    with pytest.raises(ValueError, match="different num_inference_steps"):
        pipe.interpolate_among(st, names, w, num_inference_steps=6)
    with pytest.raises(ValueError, match="different guidance_scale"):
        pipe.interpolate_among(st, names, w, guidance_scale=2.0)
    with pytest.raises(ValueError, match="different guidance_scale"):
        pipe.interpolate_among(st, names, w, guidance_rescale=0.5)
    with pytest.raises(ValueError, match="too few aid_steps"):
        pipe.interpolate_among(st, names, w, warmup_ratio=0.75)
    assert not unet.calls and st.mode is None


@pytest.mark.parametrize("name", ["image_start", "image_end", "image_embeds_end", "ip_adapter_image"])
def test_image_keywords_are_refused(name):
    unet, pipe, st, names, lat, emb = _recorded()
    with pytest.raises(NotImplementedError, match="interpolate_among takes no image inputs"):
        pipe.interpolate_among(st, names, aid_amd.grid_weights(2, 2), **{name: object()})
    with pytest.raises(TypeError, match="unexpected keyword argument 'size'"):
        pipe.interpolate_among(st, names, aid_amd.grid_weights(2, 2), size=3)


def test_processors_ctx_index_and_the_store_are_restored_after_an_exception():
    unet, pipe, st, names, lat, emb = _recorded()
    installed = dict(unet.attn_processors)

    class Boom(RuntimeError):
        pass

    real = unet.forward
    state = {}

    def failing(sample, t, encoder_hidden_states=None, added_cond_kwargs=None, return_dict=False):
        if len(unet.calls) == 1:
            state["mode"], state["procs"] = st.mode, dict(unet.attn_processors)
            raise Boom("second step")
        return real(sample, t, encoder_hidden_states, added_cond_kwargs, return_dict)

    unet.forward = failing
    guide = (torch.randn(1, 7, 12), torch.randn(1, 7, 12))
    with pytest.raises(Boom):
        pipe.interpolate_among(st, names, aid_amd.grid_weights(3, 3), embeds_guide=guide, output_type="latent")
    assert state["mode"] == "blend" and all(isinstance(p, aid_amd.KeyframeBlendAttnProcessor) for p in state["procs"].values())
    assert dict(unet.attn_processors) == installed and st.mode is None and st._pair is None
    assert all(getattr(p, "ctx_index", None) is None for p in installed.values())
    unet.forward = real
    out = pipe.interpolate_among(st, names, aid_amd.grid_weights(3, 3), output_type="latent")        # the store serves the next run
    assert out.shape == (9, 4, 4, 4)


# ---- the blend processor's own checks ------------------------------------------------------------------------------------------------
def test_blend_processor_takes_local_weight_rows_and_refuses_what_the_corner_processor_refuses():
    st = _filled(["a", "b", "c"])
    b = st.among(["a", "b", "c"])
    w = torch.tensor([[0.2, 0.3, 0.5], [0.0, 1.0, 0.0]])
    p = aid_amd.KeyframeBlendAttnProcessor(w, b, mode="inner", is_fused=False, layer="L")
    assert p.size == 2 and p.mode == "inner" and not p.is_fused and p.endpoint_layer == "L" and p.blend is b and p.activated
    assert torch.equal(p.weights, w) and isinstance(p, aid_amd.CornerInterpolatedAttnProcessor)
    p.weights = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.0]])                # same semantics as the parent's attribute
    with pytest.raises(ValueError, match="weights has 3 rows"):
        p.weights = torch.zeros(3, 3)
    with pytest.raises(ValueError, match="non-negative"):
        p.weights = torch.tensor([[1.0, -1.0, 0.0], [0.5, 0.5, 0.0]])
    with pytest.raises(ValueError, match="2 columns; the blend holds 3"):
        aid_amd.KeyframeBlendAttnProcessor(torch.eye(2), b)
    with pytest.raises(ValueError, match="mode must be"):
        aid_amd.KeyframeBlendAttnProcessor(w, b, mode="plain")
    attn = aid_amd.AttnShim(16, 2, 12, dtype=torch.float32)
    x = torch.randn(2, 12, 16)
    with pytest.raises(NotImplementedError, match="IP-Adapter layer"):
        p(attn, x, encoder_hidden_states=(torch.randn(2, 7, 12), [torch.randn(2, 1, 4, 12)]))
    p.endpoint_exchange = object()
    with pytest.raises(NotImplementedError, match="endpoint_exchange with a key-frame blend"):
        p(attn, x)
    p.endpoint_exchange = None
    with pytest.raises(NotImplementedError, match="CPU tensor"):
        p(aid_amd.AttnShim(16, 2, None, dtype=torch.float32), x)
