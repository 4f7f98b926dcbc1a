"""GPU: classifier-free guidance with guidance rescale in one launch (aid_cfg_rescale) and the pipeline arguments it
serves (guidance_rescale, timesteps, eta).

(1) The kernel against the fp64 restatement (tests/cfg_rescale_ref.py) for float16 / bfloat16 / float32 at the smallest sizes at which
    it can go wrong:  e = 2 (the minimum), 4 (a 1x1 latent), 252 (4 9 7: no multiple of 8 — every sample but the first misaligned, the
    scalar loop alone), 256, 4092 (16-byte body plus scalar tail), 16384 (more than one walk of the 1024-lane workgroup), 65536 (the SDXL
    latent);  n = 1, 3, 17;  gs = 1, 7.5;  rescale 0 (through the ABI), 0.7, 1.  Inputs N(0, 1) plus an offset of +-3 per sample, which
    a one-pass variance would not survive in fp32.
    BOUNDS, derived: the result is ONE rounding of an fp32 value, so every element is within 2^-11 |ref| (float16) / 2^-8 |ref| (bfloat16)
    plus one storage ulp for the fp32 arithmetic in front of the rounding (cfg_rescale_ref.element_bound); float32: the project's
    1e-5 rel-L2 / 1e-4 worst-element pair (tests/util.py: rel_l2 / worst).
(2) Layouts: the halves of one [2 n, e] tensor, out = text, out = uncond, padded strides between NaN gaps and guard bands
    (tests/guarded.py).  (3) Capture into a hipGraph.
(4) Pipelines on StackDenoiser("sd15", scale_down=16, latent_hw=(8, 8)), 6 steps, warm-up 0.5, float16 and float32, against the fp64
    oracle loop of tests/test_hip_depth_and_pipelines.py with the combine replaced by the restatement.
    E2E_MEASURED: rel-L2 of the rendered frames against that loop under guidance_rescale = 0.7, measured once on an MI355X; the bound
    is 1.3 x it.  The same set-up without the rescale measures the figures beside it in DESIGN.md §3.7a.
"""
import numpy as np
import pytest
import torch

import cfg_rescale_ref as R
from guarded import Guarded, round_up
from util import rel_l2, to_np64, worst

pytestmark = pytest.mark.gpu

import aid_amd  # noqa: E402
from aid_amd import ops  # noqa: E402
from aid_amd.keyframe_store import KeyframeStore  # noqa: E402
from aid_amd.loop import AidDenoiseLoop, install_sequence_processors  # noqa: E402
from aid_amd.pipelines import DDIMSchedulerLite, InterpolationStableDiffusionPipeline, StackDenoiser  # noqa: E402

DEV = "cuda:0"
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DTYPES = [F16, BF16, F32]
IDS = ["f16", "bf16", "f32"]
SIZES = [2, 4, 252, 256, 4092, 16384, 65536]


def _inputs(n, e, dtype, seed=0):
    """(text, uncond) [n, e] on the CPU, rounded to ``dtype``: N(0, 1) plus +3 / -3 on alternating samples."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * n + e)
    off = torch.tensor([3.0 if i % 2 == 0 else -3.0 for i in range(n)]).view(n, 1)
    return (torch.randn(n, e, generator=g) + off).to(dtype), (torch.randn(n, e, generator=g) + off).to(dtype)


def _check(out, text, uncond, gs, phi, dtype, what=""):
    ref, s_t, s_c = R.cfg_rescale(text, uncond, gs, phi)
    assert (s_c > 0).all() and (s_t > 0).all(), what            # the restatement's own spread, before anything is compared
    got = to_np64(out)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    if dtype == F32:
        r, w = rel_l2(got, ref), worst(got, ref)
        assert r < 1e-5 and w < 1e-4, (what, r, w)
    else:
        over = np.abs(got - ref) - R.element_bound(ref, dtype)
        assert (over <= 0).all(), (what, int((over > 0).sum()), float(over.max()), float(np.abs(ref).flat[int(over.argmax())]))


# ---- (1) the kernel against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", SIZES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_kernel_against_the_restatement(dtype, e):
    for n in (1, 3, 17):
        t, u = _inputs(n, e, dtype)
        td, ud = t.to(DEV), u.to(DEV)
        for gs in (1.0, 7.5):
            for phi in (0.0, 0.7, 1.0):
                out = ops.cfg_rescale(td, ud, gs, phi)
                assert out.shape == t.shape and out.dtype == dtype and out.is_contiguous()
                _check(out, t, u, gs, phi, dtype, f"n {n} e {e} gs {gs} phi {phi}")
        assert torch.equal(td, t.to(DEV)) and torch.equal(ud, u.to(DEV))      # inputs are inputs


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_four_dimensional_latents_and_rescale_zero_is_the_plain_combine(dtype):
    """[n, 4, h, w] tensors as the pipelines hand them over; rescale 0 is the plain combine rounded once (the eager torch expression
    rounds three times in a 16-bit dtype: compared to a few storage roundings, not to the bit)."""
    g = torch.Generator().manual_seed(3)
    t, u = torch.randn(5, 4, 9, 7, generator=g).to(dtype).to(DEV), torch.randn(5, 4, 9, 7, generator=g).to(dtype).to(DEV)
    out = ops.cfg_rescale(t, u, 7.5, 0.7)
    assert out.shape == (5, 4, 9, 7)
    _check(out, t.cpu(), u.cpu(), 7.5, 0.7, dtype)
    plain = ops.cfg_rescale(t, u, 7.5, 0.0)
    _check(plain, t.cpu(), u.cpu(), 7.5, 0.0, dtype)
    eps = {F16: 2.0 ** -10, BF16: 2.0 ** -7, F32: 2.0 ** -23}[dtype]
    assert rel_l2(to_np64(plain), to_np64(u + 7.5 * (t - u))) < 8 * eps
    with pytest.raises(RuntimeError, match="aid_cfg_rescale"):
        ops.cfg_rescale(t, u, 7.5, 1.5)                                        # the ABI's own range check
    with pytest.raises(ValueError, match="one shape and dtype"):
        ops.cfg_rescale(t, u[:4], 7.5, 0.7)
    with pytest.raises(ValueError, match="one shape and dtype"):
        ops.cfg_rescale(t, u.float() if dtype != F32 else u.half(), 7.5, 0.7)


# ---- (2) layouts ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", [252, 4092, 16384])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_halves_of_one_tensor_and_out_aliasing_an_input(dtype, e):
    n = 3
    t, u = _inputs(n, e, dtype, seed=1)
    both = torch.cat([t, u]).to(DEV)                                           # a batched-CFG UNet output [2 n, e]
    base = ops.cfg_rescale(t.to(DEV), u.to(DEV), 7.5, 0.7)
    _check(base, t, u, 7.5, 0.7, dtype)
    snap = both.clone()
    halves = ops.cfg_rescale(both[:n], both[n:], 7.5, 0.7)                     # (the second half's samples are aligned differently:
    _check(halves, t, u, 7.5, 0.7, dtype)                                      # another walk, held to the restatement, not to `base`)
    assert torch.equal(both, snap)
    a, b = t.to(DEV), u.to(DEV)
    assert ops.cfg_rescale(a, b, 7.5, 0.7, out=a) is a and torch.equal(a, base) and torch.equal(b, u.to(DEV))      # out = text
    a, b = t.to(DEV), u.to(DEV)
    assert ops.cfg_rescale(a, b, 7.5, 0.7, out=b) is b and torch.equal(b, base) and torch.equal(a, t.to(DEV))      # out = uncond
    ops.cfg_rescale(both[:n], both[n:], 7.5, 0.7, out=both[:n])                # in place on the first half of the batched output
    assert torch.equal(both[:n], halves) and torch.equal(both[n:], snap[n:])
    both.copy_(snap)
    ops.cfg_rescale(both[:n], both[n:], 7.5, 0.7, out=both[n:])
    assert torch.equal(both[n:], halves) and torch.equal(both[:n], snap[:n])
    with pytest.raises(RuntimeError, match="aid_cfg_rescale"):                 # partial overlap: refused before any launch
        ops.cfg_rescale(both[:n], both[n:], 7.5, 0.7, out=both[1:n + 1])


@pytest.mark.parametrize("pad", ["aligned", "odd"])
@pytest.mark.parametrize("e", [252, 4092])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_padded_strides_between_nan_gaps_and_guard_bands(dtype, e, pad):
    """Sample strides above e: "aligned" keeps every sample 16-byte aligned (16-byte body plus scalar tail on each), "odd" leaves most
    samples misaligned (the scalar loop).  Inputs sit between NaN, the output between sentinels: nothing outside the n x e elements
    is read into the result or written."""
    n = 5
    strides = [round_up(e, 8) + 8 * k for k in (1, 2, 3)] if pad == "aligned" else [e + 3, e + 1, e + 7]
    t, u = _inputs(n, e, dtype, seed=2)
    gt = Guarded(n, 1, e, dtype, DEV, fs=strides[0], kind="input").set(t.view(n, 1, e))
    gu = Guarded(n, 1, e, dtype, DEV, fs=strides[1], kind="input").set(u.view(n, 1, e))
    go = Guarded(n, 1, e, dtype, DEV, fs=strides[2], kind="output")
    assert gt.view.stride(0) == strides[0] and go.view.stride(0) == strides[2]
    out = ops.cfg_rescale(gt.view, gu.view, 7.5, 0.7, out=go.view)
    torch.cuda.synchronize()
    assert out is go.view
    assert go.untouched(go.layout.region_mask()) == "" and gt.inputs_unchanged() == "" and gu.inputs_unchanged() == ""
    _check(go.view.reshape(n, e), t, u, 7.5, 0.7, dtype)


# ---- (3) capture ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_captured_and_replayed_on_changed_inputs(dtype):
    n, e = 7, 4 * 16 * 16
    both = torch.zeros(2 * n, e, dtype=dtype, device=DEV)
    t, u = _inputs(n, e, dtype, seed=3)
    both.copy_(torch.cat([t, u]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.cfg_rescale(both[:n], both[n:], 7.5, 0.7)                          # (warm-up: the library's lazy state, the allocator)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = ops.cfg_rescale(both[:n], both[n:], 7.5, 0.7)
    for seed in (4, 5):
        t, u = _inputs(n, e, dtype, seed=seed)
        both.copy_(torch.cat([t, u]))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ops.cfg_rescale(t.to(DEV), u.to(DEV), 7.5, 0.7)), seed
        _check(out, t, u, 7.5, 0.7, dtype)


# ---- (4) pipelines --------------------------------------------------------------------------------------------------------------------
STEPS, RATIO, GS, PHI = 6, 0.5, 7.5, 0.7
# rel-L2 of the rendered frames against the fp64 loop under guidance_rescale = 0.7, measured once on an MI355X (the same set-up without
# the rescale: DESIGN.md §3.7a); the tests hold 1.3 x these
E2E_MEASURED = {("single", F16): 1.896e-3, ("n5", F16): 1.958e-3, ("single", F32): 1.241e-6, ("n5", F32): 1.271e-6}
# custom timesteps without the rescale: the bounds this set-up has had (tests/test_hip_depth_and_pipelines.py PIPE_BOUND, 3 - 6 steps;
# tests/test_hip_keyframe_store.py PIPE_MEASURED, float32: 1.3 x 1.38e-6)
TABLE_BOUND = {F16: 2.5e-3, F32: 1.8e-6}


def _ref_combine(text, uncond, gs, phi, out=None):
    """ops.cfg_rescale of the fp64 loop: the restatement on the loop's float64 CPU tensors."""
    return torch.from_numpy(R.cfg_rescale(text, uncond, gs, phi)[0])


class _Runs:
    """What the pipeline tests of one dtype share: the denoiser, its inputs, and every run and oracle loop, each computed once."""

    def __init__(self, dtype):
        from test_hip_depth_and_pipelines import OracleDenoiser
        self.dtype = dtype
        self.hip = hip = StackDenoiser("sd15", dtype=dtype, device=DEV, scale_down=16, latent_hw=(8, 8))
        g = torch.Generator().manual_seed(41)
        self.l0, self.l1 = torch.randn(1, 4, 8, 8, generator=g).to(dtype), torch.randn(1, 4, 8, 8, generator=g).to(dtype)
        rd = lambda t: tuple(e.to(dtype).float() for e in t)     # noqa: E731   every run sees the dtype-rounded embeddings
        cc = hip.stack.cross_dim
        self.es, self.ee = (rd((torch.randn(1, 77, cc, generator=g), torch.randn(1, 77, cc, generator=g))) for _ in range(2))
        self.pipe = InterpolationStableDiffusionPipeline(hip, DDIMSchedulerLite())
        self.ora = InterpolationStableDiffusionPipeline(OracleDenoiser(hip), DDIMSchedulerLite())
        self._memo = {}

    def _load(self):
        self.pipe.load_aid(t=0.5, is_fused=True, atype="fused_outer")          # (oracle runs and N-frame runs toggle / replace the processors)

    def single(self, **kw):
        key = ("single",) + tuple(sorted((k, repr(v)) for k, v in kw.items()))
        if key not in self._memo:
            self._load()
            self._memo[key] = self.pipe.interpolate_single(0.3, latent_start=self.l0, latent_end=self.l1, embeds_start=self.es,
                                                           embeds_end=self.ee, num_inference_steps=STEPS, warmup_ratio=RATIO,
                                                           guidance_scale=GS, output_type="latent", **kw)["images"].clone()
        return self._memo[key]

    def n5(self, **kw):
        key = ("n5",) + tuple(sorted((k, repr(v)) for k, v in kw.items()))
        if key not in self._memo:
            self._memo[key] = self.pipe.interpolate(self.l0, self.l1, embeds_start=self.es, embeds_end=self.ee, size=5,
                                                    num_inference_steps=STEPS, warmup_ratio=RATIO, guidance_scale=GS, output_type="latent",
                                                    **kw).clone()
        return self._memo[key]

    def ref(self, which, **kw):
        """The fp64 loop of ``single`` / ``n5`` with the same keywords; its combine is the restatement."""
        key = ("ref", which) + tuple(sorted((k, repr(v)) for k, v in kw.items()))
        if key not in self._memo:
            dbl = lambda t: tuple(e.double() for e in t)               # noqa: E731
            real = ops.cfg_rescale
            ops.cfg_rescale = _ref_combine
            try:
                self._load()
                common = dict(embeds_start=dbl(self.es), embeds_end=dbl(self.ee), num_inference_steps=STEPS, warmup_ratio=RATIO,
                              guidance_scale=GS, output_type="latent", **kw)
                if which == "single":
                    out = self.ora.interpolate_single(0.3, latent_start=self.l0.double(), latent_end=self.l1.double(), **common)["images"]
                else:
                    out = self.ora.interpolate(self.l0.double(), self.l1.double(), size=5, **common)
            finally:
                ops.cfg_rescale = real
            self._memo[key] = out.numpy()
        return self._memo[key]


_RUNS = {}


@pytest.fixture(params=[F16, F32], ids=["f16", "f32"])
def runs(request):
    if request.param not in _RUNS:
        _RUNS[request.param] = _Runs(request.param)
    return _RUNS[request.param]


@pytest.mark.parametrize("which", ["single", "n5"])
def test_rescaled_runs_against_the_fp64_loop(runs, which):
    out = getattr(runs, which)(guidance_rescale=PHI)
    ref = runs.ref(which, guidance_rescale=PHI)
    err = rel_l2(to_np64(out), ref)
    print(f"[cfg rescale] {runs.dtype} {which}: rel-L2 vs the fp64 loop under guidance_rescale {PHI}: {err:.3e}")
    assert out.shape == ((3, 4, 8, 8) if which == "single" else (5, 4, 8, 8)) and torch.isfinite(out).all()
    assert not torch.equal(out, getattr(runs, which)())                        # the rescale does something
    assert err < 1.3 * E2E_MEASURED[(which, runs.dtype)], err


def test_rescale_zero_is_the_run_without_the_keyword_graphs_on_and_off(runs):
    for graphs in (True, False):
        assert torch.equal(runs.single(guidance_rescale=0.0, use_graphs=graphs), runs.single(use_graphs=graphs)), graphs
        assert torch.equal(runs.n5(guidance_rescale=0.0, use_graphs=graphs), runs.n5(use_graphs=graphs)), graphs
    assert torch.equal(runs.single(use_graphs=True), runs.single()) and torch.equal(runs.single(use_graphs=False), runs.single())
    assert runs.pipe.guidance_rescale == 0.0


def test_batched_and_two_pass_runs_agree_under_the_rescale(runs):
    """One batched call per step (the op reads the two halves of its output in place) against the reference's two calls, to the bound
    these layouts have between them without the rescale: bit for bit in float16 (tests/test_hip_depth_and_pipelines.py).  In float32
    the stand-in denoiser's own torch matmuls see 10 rows in one layout and 5 in the other and need not sum in the same order, so no
    test holds the two layouts to the bit there; each is held to the fp64 loop's bound, which puts them within twice that of each other."""
    one, two = runs.n5(guidance_rescale=PHI), runs.n5(guidance_rescale=PHI, batched_cfg=False)
    if runs.dtype == F16:
        assert torch.equal(one, two)
    else:
        bound = 1.3 * E2E_MEASURED[("n5", runs.dtype)]
        err, apart = rel_l2(to_np64(two), runs.ref("n5", guidance_rescale=PHI)), rel_l2(to_np64(two), to_np64(one))
        print(f"[cfg rescale] {runs.dtype} two-pass run vs the fp64 loop {err:.3e}, vs the batched run {apart:.3e}")
        assert err < bound and apart < 2 * bound, (err, apart)
    assert torch.equal(runs.n5(guidance_rescale=PHI), runs.n5(guidance_rescale=PHI, use_graphs=False))
    assert torch.equal(runs.single(guidance_rescale=PHI), runs.single(guidance_rescale=PHI, use_graphs=False))


@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
def test_loop_layouts_batched_two_pass_and_fork_join_agree(dtype):
    """AidDenoiseLoop(guidance_rescale=0.7): batched CFG, two passes back to back and two passes on two streams (loop.fork_join) give
    the same bits (as they do without the rescale, tests/test_hip_parity.py / test_hip_two_stream_passes.py), and those bits are the
    restatement of the two pass outputs to the kernel's bound."""
    n, steps = 5, 4
    unet = aid_amd.AttnStackUNet("sd15", dtype=dtype, device=DEV, scale_down=16)
    install_sequence_processors(unet, n, early="fused_outer", num_inference_steps=steps)
    g = torch.Generator().manual_seed(8)
    xs = {lv: torch.randn(n, lv[0], lv[1], generator=g).to(dtype).to(DEV) for lv in unet.level_shapes()}
    cond = torch.randn(n, unet.text_len, unet.cross_dim, generator=g).to(dtype).to(DEV)
    unc = torch.randn(n, unet.text_len, unet.cross_dim, generator=g).to(dtype).to(DEV)
    kw = dict(num_inference_steps=steps, guidance_scale=GS, use_graphs=False)
    outs = []
    for layout in (dict(batched_cfg=True), dict(), dict(concurrent_cfg=True)):
        loop = AidDenoiseLoop(unet, xs, cond, unc, guidance_rescale=PHI, **kw, **layout)
        res = [loop.step(i) for i in (0, steps - 1)]
        torch.cuda.synchronize()
        outs.append([{k: v.clone() for k, v in r.items()} for r in res])
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            for k in a:
                assert torch.equal(a[k], b[k]), k
    passes = AidDenoiseLoop(unet, xs, cond, unc, combine=lambda t, u: (t, u), **kw)
    for i, got in zip((0, steps - 1), outs[0]):
        text, uncond = passes.step(i)
        for k in got:
            _check(got[k], text[k].cpu(), uncond[k].cpu(), GS, PHI, dtype, f"step {i} level {k}")
    with pytest.raises(ValueError, match="guidance_rescale"):
        AidDenoiseLoop(unet, xs, cond, unc, guidance_rescale=1.5, **kw)


def test_key_frames_recorded_under_the_rescale_replay_under_it_only(runs):
    pipe, dtype = runs.pipe, runs.dtype
    store = KeyframeStore()
    kw = dict(num_inference_steps=STEPS, warmup_ratio=RATIO, guidance_scale=GS, output_type="latent")
    pipe.record_keyframes(store, ["a", "b"], torch.cat([runs.l0, runs.l1]), embeds=[runs.es, runs.ee], guidance_rescale=PHI, **kw)
    assert store.settings["guidance_scale"] == (GS, PHI)
    out = pipe.interpolate_between(store, "a", "b", size=5, warmup_ratio=RATIO, output_type="latent", guidance_rescale=PHI)
    bits = lambda t: t.contiguous().view(torch.int16 if dtype == F16 else torch.int32)      # noqa: E731
    assert out.shape == (5, 4, 8, 8)
    assert torch.equal(bits(out[0:1]), bits(store["a"].final)) and torch.equal(bits(out[4:5]), bits(store["b"].final))
    # the interior frames are held to the full run's bound, as every replay is (tests/test_hip_keyframe_store.py)
    err = rel_l2(to_np64(out[1:4]), runs.ref("n5", guidance_rescale=PHI)[1:4])
    print(f"[cfg rescale] {dtype} key-frame replay under guidance_rescale {PHI}, interior frames: {err:.3e}")
    assert err < 1.3 * E2E_MEASURED[("n5", dtype)], err
    for kwargs in (dict(), dict(guidance_rescale=0.0), dict(guidance_rescale=0.5)):
        with pytest.raises(ValueError, match="different guidance_scale"):
            pipe.interpolate_between(store, "a", "b", size=5, warmup_ratio=RATIO, output_type="latent", **kwargs)
    assert store.mode is None and store.names == ["a", "b"]
    plain = KeyframeStore()
    pipe.record_keyframes(plain, ["a", "b"], torch.cat([runs.l0, runs.l1]), embeds=[runs.es, runs.ee], **kw)
    assert plain.settings["guidance_scale"] == GS
    with pytest.raises(ValueError, match="different guidance_scale"):
        pipe.interpolate_between(plain, "a", "b", size=5, warmup_ratio=RATIO, output_type="latent", guidance_rescale=PHI)


def test_custom_timesteps_against_the_fp64_loop_on_that_table(runs):
    table = DDIMSchedulerLite()
    table.set_timesteps(STEPS)
    every_second = table.timesteps.tolist()[::2]
    assert every_second == [831, 499, 167]
    out = runs.single(timesteps=every_second)
    ref = runs.ref("single", timesteps=every_second)
    err = rel_l2(to_np64(out), ref)
    print(f"[cfg rescale] {runs.dtype} custom timesteps {every_second}: rel-L2 vs the fp64 loop {err:.3e}")
    assert out.shape == (3, 4, 8, 8) and not torch.equal(out, runs.single())
    assert err < TABLE_BOUND[runs.dtype], err


def test_eta_with_a_seeded_generator_is_reproducible(runs):
    """(No parity claim: the noise stream is torch's.)"""
    gen = lambda seed: torch.Generator(device=DEV).manual_seed(seed)           # noqa: E731
    runs._load()
    run = lambda g: runs.pipe.interpolate_single(0.3, latent_start=runs.l0, latent_end=runs.l1, embeds_start=runs.es,      # noqa: E731
                                                 embeds_end=runs.ee, num_inference_steps=STEPS, warmup_ratio=RATIO, guidance_scale=GS,
                                                 output_type="latent", eta=0.5, generator=g)["images"].clone()
    a, b, c = run(gen(11)), run(gen(11)), run(torch.Generator().manual_seed(11))       # (a host generator seeds a device run too)
    assert torch.equal(a, b) and torch.isfinite(a).all() and torch.isfinite(c).all()
    assert not torch.equal(a, runs.single()) and not torch.equal(c, runs.single())
