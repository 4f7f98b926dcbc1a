"""guidance_rescale / timesteps / sigmas / eta: the host side, without a GPU.

``aid_cfg_rescale``'s declaration, export and argument table (fake aligned pointers and a NULL stream: every check runs before the
launch, and the device is asked for last), ``ops.cfg_rescale`` on CPU tensors, ``_retrieve_timesteps``, the custom table and the eta
of ``DDIMSchedulerLite``, how the stores' signatures carry the rescale, and the pipeline surface on the recording stub UNet of
tests/test_pipelines.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import cfg_rescale_ref as R
from aid_amd import _lib, ops
from aid_amd.endpoint_store import SIGNATURE_FIELDS, EndpointStore, run_settings, run_signature
from aid_amd.keyframe_store import SETTINGS_FIELDS
from aid_amd.loop import AidDenoiseLoop
from aid_amd.pipelines import (DDIMSchedulerLite, InterpolationStableDiffusionPipeline, InterpolationStableDiffusionXLPipeline,
                               _retrieve_timesteps)
from test_pipelines import RecordingUNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "attention-interpolation-diffusion_amd", "csrc")
HEADER = open(os.path.join(ROOT, "include", "aid_hip.h")).read()
ARG, DTYPE, SHAPE, NO_DEVICE = -1, -2, -3, -6
T, U, O = 0x10000, 0x20000, 0x30000


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_the_version_stays():
    """(fails on the parent commit: the symbol is new)"""
    assert re.search(r"^int\s+aid_cfg_rescale\s*\(const void\* text, const void\* uncond, void\* out, int32_t n, int64_t e,", HEADER,
                     flags=re.M)
    assert "pipeline_interpolated_sd.py:92-108, 1892-1902" in HEADER
    lib = _lib.load()
    assert "aid_cfg_rescale" in _lib.ABI_SYMBOLS and hasattr(lib, "aid_cfg_rescale")
    assert lib.aid_abi_version() == 10 and _lib.AID_ABI_VERSION == 10 and re.search(r"#define AID_ABI_VERSION 10\b", HEADER)


def _call(text=T, uncond=U, out=O, n=3, e=256, ts=256, us=256, os_=256, gs=7.5, phi=0.7, dtype=_lib.DTYPE_F16):
    return _lib.load().aid_cfg_rescale(text, uncond, out, n, e, ts, us, os_, gs, phi, dtype, None)


@pytest.mark.parametrize("kw,code", [
    (dict(text=None), ARG), (dict(uncond=None), ARG), (dict(out=None), ARG), (dict(n=-1), ARG),
    (dict(ts=255), ARG), (dict(us=255), ARG), (dict(os_=255), ARG), (dict(ts=0), ARG), (dict(os_=-256), ARG),
    (dict(phi=-0.1), ARG), (dict(phi=1.5), ARG), (dict(phi=float("nan")), ARG), (dict(phi=float("inf")), ARG),
    # partial overlap of out with an input: shifted by one row of 16 bytes, by one sample, the same base under another stride, an
    # input that begins inside out
    (dict(out=T + 16), ARG), (dict(out=T + 512), ARG), (dict(out=T, os_=512), ARG), (dict(out=U, ts=256, us=264, os_=256), ARG),
    (dict(out=T - 512), ARG), (dict(out=U - 2), ARG), (dict(out=U + 3 * 512 - 2), ARG),
    (dict(e=1, ts=1, us=1, os_=1), SHAPE), (dict(e=0, ts=0, us=0, os_=0), SHAPE), (dict(e=-4), SHAPE),
    (dict(text=T + 1), SHAPE), (dict(uncond=U + 1), SHAPE), (dict(out=O + 1), SHAPE),
    (dict(text=T + 2, dtype=_lib.DTYPE_F32), SHAPE), (dict(out=O + 2, dtype=_lib.DTYPE_F32), SHAPE),
    (dict(dtype=3), DTYPE), (dict(dtype=-1), DTYPE)])
def test_argument_errors_return_their_codes_before_any_launch(kw, code):
    """A launch with these fake pointers and a NULL stream would fault."""
    assert _call(**kw) == code


@pytest.mark.parametrize("kw", [
    dict(), dict(phi=0.0), dict(phi=1.0), dict(gs=1.0), dict(dtype=_lib.DTYPE_BF16), dict(dtype=_lib.DTYPE_F32), dict(e=2, ts=2, us=2, os_=2),
    dict(out=T), dict(out=U),                                 # out IS an input: same base, same stride
    dict(uncond=T + 3 * 512, out=T, ts=256, us=256),          # the two halves of one [2 n, e] tensor, in place on the first
    dict(text=T + 2, uncond=U + 6, out=O + 10),               # 2-byte aligned is aligned for a 16-bit dtype
    dict(ts=264, us=300, os_=259),                            # padded strides
    dict(out=T + 3 * 512), dict(out=T - 3 * 512)])            # out right behind / right in front of an input
def test_a_valid_call_passes_every_check_and_asks_for_the_device_last(kw):
    """n = 0 launches nothing and is AID_OK whatever else is passed (the checks run first: see the error table); with n > 0 the
    call gets as far as the device, which a machine without one answers with AID_ERR_NO_DEVICE.  Where there IS a device the
    fake pointers must not reach it, so only the n = 0 half runs there."""
    assert _call(n=0, **kw) == 0
    if not torch.cuda.is_available():
        assert _call(**kw) == NO_DEVICE


def test_error_checks_come_before_the_empty_call_returns():
    assert _call(n=0, phi=2.0) == ARG and _call(n=0, e=1, ts=1, us=1, os_=1) == SHAPE and _call(n=0, dtype=9) == DTYPE


def test_the_three_instantiations_use_no_scratch_and_the_reduction_scratch_only():
    """aid_cfg.resources.txt at this commit: f16 45 VGPRs, bf16 44, f32 46; no AGPRs, no scratch, no spills, 128 bytes of LDS (two
    floats per wave of a 1024-thread workgroup), 8 waves per SIMD."""
    path = os.path.join(CSRC, "aid_cfg.resources.txt")
    assert os.path.exists(path), f"{path} not there: build the library first (python -c 'import __graft_entry__ as g; g.build()')"
    blocks = open(path).read().split("Name: ")[1:]
    names = [b.split()[0] for b in blocks]
    assert len(blocks) == 3 and all("aid_cfg_rescale_kernel" in n for n in names) and len(set(names)) == 3
    for b in blocks:
        num = lambda key: int(re.search(re.escape(key) + r": (\d+)", b).group(1))   # noqa: E731
        assert num("ScratchSize [bytes/lane]") == 0 and num("VGPRs Spill") == 0 and num("SGPRs Spill") == 0
        assert num("AGPRs") == 0 and num("LDS Size [bytes/block]") == 128
        assert num("VGPRs") <= 64 and num("Occupancy [waves/SIMD]") == 8


# ---- ops ---------------------------------------------------------------------------------------------------------------------------
def test_ops_cfg_rescale_refuses_cpu_tensors_and_bad_layouts():
    t, u = torch.randn(3, 4, 8, 8), torch.randn(3, 4, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.cfg_rescale(t, u, 7.5, 0.7)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.cfg_rescale(t, u, 7.5, 0.7, out=t)
    assert ops._sample_layout(t, "t") == (3, 256, 256)
    assert ops._sample_layout(torch.randn(6, 4, 8, 8)[3:], "t") == (3, 256, 256)
    assert ops._sample_layout(torch.randn(3, 600)[:, :256], "t") == (3, 256, 600)
    assert ops._sample_layout(torch.randn(1, 4, 8, 8), "t") == (1, 256, 256)
    with pytest.raises(ValueError, match="contiguous"):
        ops._sample_layout(torch.randn(3, 8, 32).transpose(1, 2), "t")
    with pytest.raises(ValueError, match=r"\[n, \.\.\.\]"):
        ops._sample_layout(torch.randn(256), "t")


def test_the_restatement_is_the_reference_formula():
    """cfg_rescale_ref against the textbook two-step form on float64 tensors (torch.std is unbiased), and its limits."""
    g = torch.Generator().manual_seed(5)
    t, u = torch.randn(4, 4, 6, 6, generator=g, dtype=torch.float64) + 3, torch.randn(4, 4, 6, 6, generator=g, dtype=torch.float64) - 3
    for gs, phi in ((7.5, 0.5), (1.0, 1.0), (3.0, 0.0)):
        c = u + gs * (t - u)
        st, sc = t.std(dim=(1, 2, 3), keepdim=True), c.std(dim=(1, 2, 3), keepdim=True)
        want = phi * (c * (st / sc)) + (1 - phi) * c
        got, s_t, s_c = R.cfg_rescale(t, u, gs, phi)
        assert np.allclose(got, want.numpy(), rtol=1e-12, atol=0) and np.allclose(s_t, st.flatten().numpy()) and (s_c > 0).all()
    assert np.array_equal(R.cfg_rescale(t, u, 3.0, 0.0)[0], (u + 3.0 * (t - u)).numpy())
    full = R.cfg_rescale(t, u, 7.5, 1.0)[0]
    assert np.allclose(full.reshape(4, -1).std(axis=1, ddof=1), t.reshape(4, -1).std(dim=1).numpy(), rtol=1e-12)   # the spread of text
    assert R.storage_ulp(np.array([1.0, 1.5, 2.0, 1e-9]), torch.float16).tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -24]
    assert R.storage_ulp(np.array([1.0, 3.0]), torch.bfloat16).tolist() == [2.0 ** -7, 2.0 ** -6]


# ---- scheduler ---------------------------------------------------------------------------------------------------------------------
class _NoTable:
    """A scheduler whose set_timesteps takes neither keyword."""
    timesteps = torch.arange(3)

    def set_timesteps(self, num_inference_steps, device=None):
        self.n = num_inference_steps


def test_retrieve_timesteps():
    s = DDIMSchedulerLite()
    with pytest.raises(ValueError, match="only one of"):
        _retrieve_timesteps(s, None, None, timesteps=[9, 5, 1], sigmas=[1.0, 0.5])
    with pytest.raises(ValueError, match="_NoTable"):
        _retrieve_timesteps(_NoTable(), None, None, timesteps=[9, 5, 1])
    with pytest.raises(ValueError, match="DDIMSchedulerLite.*sigmas"):
        _retrieve_timesteps(s, 50, None, sigmas=[1.0, 0.5])
    ts, n = _retrieve_timesteps(s, 50, None, timesteps=[801, 401, 1])
    assert n == 3 and ts.tolist() == [801, 401, 1] and s.num_inference_steps == 3
    ts, n = _retrieve_timesteps(s, 5, None)
    assert n == 5 and ts.tolist() == [801, 601, 401, 201, 1]
    plain = _NoTable()
    assert _retrieve_timesteps(plain, 7, None)[1] == 7 and plain.n == 7


def test_ddim_custom_timesteps_round_trip_and_are_checked():
    s, d = DDIMSchedulerLite(), DDIMSchedulerLite()
    d.set_timesteps(10)
    s.set_timesteps(timesteps=d.timesteps.tolist())
    assert torch.equal(s.timesteps, d.timesteps) and s.num_inference_steps == 10
    g = torch.Generator().manual_seed(1)
    x, eps = torch.randn(3, 4, 8, 8, generator=g), torch.randn(3, 4, 8, 8, generator=g)
    for t in d.timesteps:                                     # the default table handed in as a custom one: the same steps
        assert torch.equal(s.step(eps, t, x)[0], d.step(eps, t, x)[0])
    s.set_timesteps(timesteps=torch.tensor([901, 500, 20]))
    assert s.timesteps.tolist() == [901, 500, 20] and s._prev == {901: 500, 500: 20, 20: -1}
    ac = s.alphas_cumprod
    x0 = (x.double() - (1 - ac[500]) ** 0.5 * eps.double()) / ac[500] ** 0.5
    assert torch.allclose(s.step(eps, 500, x)[0].double(), ac[20] ** 0.5 * x0 + (1 - ac[20]) ** 0.5 * eps.double(), atol=1e-5)
    assert torch.allclose(s.step(eps, 20, x)[0].double(),
                          (x.double() - (1 - ac[20]) ** 0.5 * eps.double()) / ac[20] ** 0.5, atol=1e-5)      # behind the last one: a = 1
    for bad in ([1, 5, 9], [9, 9, 1], [1000, 5], [5, -1], [], [5.5, 1]):
        with pytest.raises(ValueError):
            s.set_timesteps(timesteps=bad)
    with pytest.raises(ValueError):
        s.set_timesteps(10, timesteps=[9, 1])
    with pytest.raises(ValueError):
        s.set_timesteps()
    s.set_timesteps(10)                                       # and back to the default table
    assert torch.equal(s.timesteps, d.timesteps) and s._prev is None
    assert "sigmas" not in inspect.signature(s.set_timesteps).parameters


def test_ddim_eta_zero_is_the_step_it_was_and_eta_follows_the_published_variance():
    s = DDIMSchedulerLite()
    s.set_timesteps(10)
    g = torch.Generator().manual_seed(2)
    for dtype in (torch.float32, torch.float16):
        x, eps = torch.randn(3, 4, 8, 8, generator=g).to(dtype), torch.randn(3, 4, 8, 8, generator=g).to(dtype)
        for t in (901, 401, 1):
            # the step as the parent commit computed it, written out
            a_t, a_p = float(s.alphas_cumprod[t]), (float(s.alphas_cumprod[t - 100]) if t >= 100 else 1.0)
            x0 = (x.float() - (1 - a_t) ** 0.5 * eps.float()) / a_t ** 0.5
            was = (a_p ** 0.5 * x0 + (1 - a_p) ** 0.5 * eps.float()).to(dtype)
            assert torch.equal(s.step(eps, t, x)[0], was)
            assert torch.equal(s.step(eps, t, x, eta=0.0, generator=torch.Generator().manual_seed(3))[0], was)
            assert torch.equal(s.step(eps, torch.tensor(t), x, return_dict=False, eta=0.0)[0], was)
    x, eps, t, eta = x.float(), eps.float(), 401, 0.5
    a_t, a_p = float(s.alphas_cumprod[401]), float(s.alphas_cumprod[301])
    var = eta ** 2 * (1 - a_p) / (1 - a_t) * (1 - a_t / a_p)
    out = s.step(eps, t, x, eta=eta, generator=torch.Generator().manual_seed(4))[0]
    again = s.step(eps, t, x, eta=eta, generator=torch.Generator().manual_seed(4))[0]
    other = s.step(eps, t, x, eta=eta, generator=torch.Generator().manual_seed(5))[0]
    assert torch.equal(out, again) and not torch.equal(out, other)
    z = torch.randn(x.shape, generator=torch.Generator().manual_seed(4))
    x0 = (x - (1 - a_t) ** 0.5 * eps) / a_t ** 0.5
    assert torch.allclose(out, a_p ** 0.5 * x0 + (1 - a_p - var) ** 0.5 * eps + var ** 0.5 * z, atol=1e-5)
    assert 0 < var < 1 - a_p


# ---- stores ------------------------------------------------------------------------------------------------------------------------
def _sig(**kw):
    g = torch.Generator().manual_seed(6)
    lat = [torch.randn(1, 4, 4, 4, generator=g) for _ in range(2)]
    emb = [torch.randn(1, 7, 12, generator=g) for _ in range(4)]
    unet = torch.nn.Linear(2, 2)
    base = dict(latent_start=lat[0], latent_end=lat[1], embeds_start=emb[0], embeds_end=emb[1], embeds_negative=emb[2:], embeds_pooled=[],
                embeds_guide=[], num_inference_steps=6, warmup_ratio=0.5, early="outer", late="self", fusion=True, guidance_scale=7.5,
                dtype=torch.float16, timesteps=torch.tensor([801, 401, 1]), unet=unet)
    return run_signature(**dict(base, **kw)), unet


def test_store_signatures_carry_the_rescale_inside_guidance_scale():
    parent, unet = _sig()                                     # the call of the parent commit: no guidance_rescale keyword
    zero, _ = _sig(unet=unet, guidance_rescale=0.0)
    resc, _ = _sig(unet=unet, guidance_rescale=0.7)
    assert zero == parent and list(zero) == list(SIGNATURE_FIELDS) and zero["guidance_scale"] == 7.5 \
        and isinstance(zero["guidance_scale"], float)
    assert resc != zero and resc["guidance_scale"] == (7.5, 0.7)
    assert {f for f in SIGNATURE_FIELDS if resc[f] != zero[f]} == {"guidance_scale"}
    kw = dict(num_inference_steps=6, guidance_scale=5.0, dtype=torch.float16, timesteps=[801, 401, 1], unet=unet)
    st0, st7 = run_settings(**kw), run_settings(guidance_rescale=0.7, **kw)
    assert set(st0) == set(SETTINGS_FIELDS) == set(st7) and st0 == run_settings(guidance_rescale=0.0, **kw)
    assert st0["guidance_scale"] == 5.0 and st7["guidance_scale"] == (5.0, 0.7)
    store = EndpointStore()
    store.begin_record(resc, 3, torch.device("cpu"))
    store.finish_record(torch.zeros(2, 4, 4, 4))
    store.check(resc)
    with pytest.raises(ValueError, match="different guidance_scale"):
        store.check(zero)


# ---- pipelines on the recording stub -------------------------------------------------------------------------------------------------
def _stub_pipe():
    g = torch.Generator().manual_seed(0)
    unet = RecordingUNet()
    pipe = InterpolationStableDiffusionPipeline(unet, DDIMSchedulerLite())
    pipe.load_aid(t=0.5, is_fused=True, atype="fused_inner")
    l0, l1 = torch.randn(1, 4, 4, 4, generator=g), torch.randn(1, 4, 4, 4, generator=g)
    es, ee = (torch.randn(1, 7, 12, generator=g), torch.randn(1, 7, 12, generator=g)), \
             (torch.randn(1, 7, 12, generator=g), torch.randn(1, 7, 12, generator=g))
    kw = dict(latent_start=l0, latent_end=l1, embeds_start=es, embeds_end=ee, warmup_ratio=0.4, guidance_scale=3.0, output_type="latent")
    return pipe, unet, kw


def test_guidance_rescale_reaches_the_op_instead_of_being_refused():
    """(fails on the parent commit: NotImplementedError.)  The stub UNet lives on the CPU, so the op's own refusal of CPU tensors is
    what the run ends in — after the two UNet passes of the first step."""
    pipe, unet, kw = _stub_pipe()
    with pytest.raises(RuntimeError, match="no CPU path"):
        pipe.interpolate_single(0.3, num_inference_steps=10, guidance_rescale=0.7, **kw)
    assert len(unet.calls) == 2 and pipe.guidance_rescale == 0.7 and pipe.guidance_scale == 3.0
    with pytest.raises(RuntimeError, match="no CPU path"):
        pipe.interpolate(kw["latent_start"], kw["latent_end"], embeds_start=kw["embeds_start"], embeds_end=kw["embeds_end"], size=4,
                         num_inference_steps=4, output_type="latent", guidance_rescale=0.7)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="guidance_rescale"):
            pipe.interpolate_single(0.3, num_inference_steps=10, guidance_rescale=bad, **kw)
    out0 = pipe.interpolate_single(0.3, num_inference_steps=10, guidance_rescale=0.0, **kw)["images"]
    out = pipe.interpolate_single(0.3, num_inference_steps=10, **kw)["images"]
    assert torch.equal(out0, out) and pipe.guidance_rescale == 0.0


@pytest.mark.parametrize("cls", [InterpolationStableDiffusionPipeline, InterpolationStableDiffusionXLPipeline])
def test_the_build_specific_keyword_is_on_every_entry(cls):
    for name in ("interpolate_single", "interpolate", "record_keyframes", "interpolate_between"):
        p = inspect.signature(getattr(cls, name)).parameters["guidance_rescale"]
        assert p.default == 0.0, name
    assert isinstance(cls.guidance_rescale, property)
    assert inspect.signature(AidDenoiseLoop.__init__).parameters["guidance_rescale"].default == 0.0


def test_custom_timesteps_set_the_step_and_warm_up_counts():
    pipe, unet, kw = _stub_pipe()
    out = pipe.interpolate_single(0.3, timesteps=[801, 601, 401, 201, 1], **kw)["images"]       # (num_inference_steps stays at its default 50)
    assert [c["t"] for c in unet.calls[0::2]] == [801, 601, 401, 201, 1] and len(unet.calls) == 10
    assert [c["active"] for c in unet.calls[0::2]] == [True, True, False, False, False]          # int(5 * 0.4)
    unet.calls.clear()
    same = pipe.interpolate_single(0.3, num_inference_steps=5, **kw)["images"]                   # the default 5-step table IS that list
    assert torch.equal(out, same)
    unet.calls.clear()
    pipe.interpolate_single(0.3, timesteps=[901, 500, 20], **kw)
    assert [c["t"] for c in unet.calls[0::2]] == [901, 500, 20] and [c["active"] for c in unet.calls[0::2]] == [True, False, False]
    with pytest.raises(ValueError, match="DDIMSchedulerLite.*sigmas"):
        pipe.interpolate_single(0.3, sigmas=[14.6, 1.0, 0.0], **kw)
    with pytest.raises(ValueError, match="only one of"):
        pipe.interpolate_single(0.3, timesteps=[9, 1], sigmas=[14.6, 0.0], **kw)


def test_eta_reaches_the_scheduler_and_is_refused_with_a_store():
    pipe, unet, kw = _stub_pipe()
    run = lambda seed, eta: pipe.interpolate_single(0.3, num_inference_steps=6, eta=eta,                  # noqa: E731
                                                    generator=torch.Generator().manual_seed(seed), **kw)["images"]
    a, b, c, d = run(7, 0.5), run(7, 0.5), run(8, 0.5), run(7, 0.0)
    assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, d) and torch.isfinite(a).all()
    assert torch.equal(d, pipe.interpolate_single(0.3, num_inference_steps=6, generator=torch.Generator().manual_seed(7), **kw)["images"])
    n = len(unet.calls)
    with pytest.raises(ValueError, match="eta"):
        pipe.interpolate_single(0.3, num_inference_steps=6, eta=0.3, endpoints=EndpointStore(), **kw)
    assert len(unet.calls) == n                               # refused before anything ran

    class Euler(DDIMSchedulerLite):                           # a scheduler whose step takes neither keyword gets neither
        def step(self, model_output, timestep, sample, return_dict=False):
            return super().step(model_output, timestep, sample)

    pipe.scheduler = Euler()
    assert torch.equal(pipe.interpolate_single(0.3, num_inference_steps=6, eta=0.5, **kw)["images"], d)
