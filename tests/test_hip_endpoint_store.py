"""GPU: the end-point K / V^T store — the copy kernel (aid_endpoint_rows) under guarded buffers, the library call
(aid_processor_ep_fwd: RECORD bit-identical to aid_processor_fwd, REPLAY against the fp64 oracle of the FULL batch at the existing
path's per-call bounds), one captured replay call addressing another slot at every graph replay, and the pipelines' ``endpoints=``.

Bounds of the library call: tests/util.py TOL / WORST (16-bit) and test_hip_f32.py's 1e-5 / 1e-4 (float32) — the bounds of
aid_processor_fwd itself: the replay path adds no arithmetic, only a different GEMM tile plan for a smaller m.

Bounds of the pipelines' replay: 1.3 x the rel-L2 the FULL, non-replay run of the same stack, dtype and step count measures for the
same frames against the same fp64 oracle loop (PIPE_MEASURED below, measured once on an MI355X)."""
import ctypes as C

import numpy as np
import pytest
import torch

from guarded import Guarded
from oracle import aid_oracle as O
from util import TOL, WORST, rel_l2, to_np64, worst

pytestmark = pytest.mark.gpu

import aid_amd  # noqa: E402
from aid_amd import _lib, lora, ops  # noqa: E402
from aid_amd.endpoint_store import EndpointStore  # noqa: E402
from aid_amd.pipelines import DDIMSchedulerLite, InterpolationStableDiffusionPipeline, StackDenoiser  # noqa: E402

DEV = "cuda:0"
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
TOL_ALL = {**TOL, F32: 1e-5}
WORST_ALL = {**WORST, F32: 1e-4}


def _close(got, ref, dtype, what=""):
    got = to_np64(got)
    assert np.isfinite(got).all(), what
    e, w = rel_l2(got, ref), worst(got, ref)
    print(f"{what}: rel-L2 {e:.3e} (bound {TOL_ALL[dtype]:.0e}), worst {w:.3e} (bound {WORST_ALL[dtype]:.0e})")
    assert e < TOL_ALL[dtype] and w < WORST_ALL[dtype], (what, e, w)


# ---- the copy kernel ----------------------------------------------------------------------------------------------------------------
N_STEPS, F = 3, 5


def _call_tensors(l, c, dtype, seed):
    """A call's k [F, l, c] and vt [F, c, lp] as guarded inputs with every element of the strides finite (the whole block moves)."""
    lp = (l + 7) // 8 * 8
    g = torch.Generator().manual_seed(seed)
    k = Guarded(F, l, c, dtype, DEV, kind="input").set(torch.randn(F, l, c, generator=g))
    vt = Guarded(F, c, lp, dtype, DEV, kind="input").set(torch.randn(F, c, lp, generator=g))
    return k, vt, lp


def _stores(l, c, lp, dtype):
    return (Guarded(N_STEPS, 2, l * c, dtype, DEV, kind="output"), Guarded(N_STEPS, 2, c * lp, dtype, DEV, kind="output"))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("dtype", [F16, BF16, F32], ids=["f16", "bf16", "f32"])
@pytest.mark.parametrize("l,c", [(33, 40), (77, 320), (257, 64)])
def test_put_then_get_moves_exactly_the_four_blocks(l, c, dtype):
    """Ragged lp and 16-byte chunk counts that are no multiple of the workgroup: PUT rows (0, 4) into slot 1, GET the slot into rows
    (3, 1) of another call's tensors — bit for bit, nothing outside the addressed slot / the two destination rows written, inputs
    unchanged."""
    k, vt, lp = _call_tensors(l, c, dtype, 1)
    ks, vs = _stores(l, c, lp, dtype)
    step = torch.tensor([1], dtype=torch.int32, device=DEV)
    ops.endpoint_rows(k.view, vt.view, ks.view, vs.view, step, "put", 0, F - 1)
    torch.cuda.synchronize()
    for st, src, what in ((ks, k, "k_store"), (vs, vt, "vt_store")):
        assert st.untouched(st.layout.region_mask(frames=[1])) == "", what
        assert torch.equal(_bits(st.view[1, 0]), _bits(src.view[0].reshape(-1))) and torch.equal(_bits(st.view[1, 1]), _bits(src.view[F - 1].reshape(-1)))
        assert src.inputs_unchanged() == "", what
    ks.snapshot(), vs.snapshot()
    k2 = Guarded(F, l, c, dtype, DEV, kind="output")
    vt2 = Guarded(F, c, lp, dtype, DEV, kind="output")
    ops.endpoint_rows(k2.view, vt2.view, ks.view, vs.view, step, "get", 3, 1)
    torch.cuda.synchronize()
    for dst, src, st, what in ((k2, k, ks, "k"), (vt2, vt, vs, "vt")):
        assert dst.untouched(dst.layout.region_mask(frames=[1, 3])) == "", what
        assert torch.equal(_bits(dst.view[3]), _bits(src.view[0])) and torch.equal(_bits(dst.view[1]), _bits(src.view[F - 1])), what
        assert st.inputs_unchanged() == "", what


def test_the_same_argument_struct_addresses_the_slot_the_device_index_names():
    """Launched again after ONLY the device step index changed, the same AidEndpointRows goes to the other slot; an index outside
    [0, n_steps) moves nothing."""
    l, c, dtype = 33, 40, F16
    k, vt, lp = _call_tensors(l, c, dtype, 2)
    ks, vs = _stores(l, c, lp, dtype)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = _lib.AidEndpointRows()
    a.k, a.vt, a.k_store, a.vt_store, a.step = k.ptr, vt.ptr, ks.ptr, vs.ptr, step.data_ptr()
    a.k_fs, a.vt_fs, a.row_begin, a.row_end, a.n_steps, a.direction, a.dtype = l * c, c * lp, 1, 2, N_STEPS, _lib.EP_PUT, _lib.DTYPE_F16
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    for bad in (N_STEPS, -1, 1 << 20):
        step.fill_(bad)
        assert lib.aid_endpoint_rows(C.byref(a), stream) == 0
        torch.cuda.synchronize()
        assert ks.untouched(ks.layout.region_mask(frames=[])) == "" and vs.untouched(vs.layout.region_mask(frames=[])) == "", bad
    step.fill_(2)
    assert lib.aid_endpoint_rows(C.byref(a), stream) == 0
    torch.cuda.synchronize()
    assert ks.untouched(ks.layout.region_mask(frames=[2])) == "" and vs.untouched(vs.layout.region_mask(frames=[2])) == ""
    step.fill_(0)
    assert lib.aid_endpoint_rows(C.byref(a), stream) == 0
    torch.cuda.synchronize()
    assert ks.untouched(ks.layout.region_mask(frames=[0, 2])) == "" and vs.untouched(vs.layout.region_mask(frames=[0, 2])) == ""
    for s in (0, 2):
        assert torch.equal(_bits(ks.view[s, 0]), _bits(k.view[1].reshape(-1))) and torch.equal(_bits(vs.view[s, 1]), _bits(vt.view[2].reshape(-1)))
    # GET with an index out of range writes nothing either
    k2, vt2 = Guarded(F, l, c, dtype, DEV, kind="output"), Guarded(F, c, lp, dtype, DEV, kind="output")
    a.k, a.vt, a.direction = k2.ptr, vt2.ptr, _lib.EP_GET
    step.fill_(N_STEPS)
    assert lib.aid_endpoint_rows(C.byref(a), stream) == 0
    torch.cuda.synchronize()
    assert k2.untouched(k2.layout.region_mask(frames=[])) == "" and vt2.untouched(vt2.layout.region_mask(frames=[])) == ""


# ---- the library call ---------------------------------------------------------------------------------------------------------------
COEF = [0.0, 0.2, 0.5, 0.8, 1.0]
N = len(COEF)
SHAPES = [(40, 320, 8), (33, 128, 2), (24, 640, 8), (16, 1280, 8)]          # head dims 40, 64, 80, 160
MODES = [("outer", False), ("outer", True), ("inner", False), ("inner", True)]


class _Layer:
    """One self-attention layer's inputs on the device and its fp64 oracle, built once per (shape, dtype)."""

    def __init__(self, s, c, heads, dtype, seed=5):
        g = torch.Generator().manual_seed(seed + s + c)
        rnd = lambda *sh, sc=1.0: (torch.randn(*sh, generator=g) * sc).to(dtype)      # noqa: E731
        self.s, self.c, self.heads, self.dtype = s, c, heads, dtype
        self.x = rnd(N, s, c).to(DEV)
        self.riders = rnd(2, s, c).to(DEV)
        self.w = [rnd(c, c, sc=c ** -0.5).to(DEV) for _ in range(4)]
        self.bo = rnd(c, sc=0.1).to(DEV)
        self.coef = torch.tensor(COEF).to(dtype).float()
        self.w64 = O.AttnWeights(*(to_np64(t) for t in self.w), to_np64(self.bo), heads=heads)
        self._ref = {}

    def ref(self, mode, fused):
        """fp64 oracle of the FULL batch, computed once per mode and left unchanged."""
        key = (mode, fused)
        if key not in self._ref:
            fn = O.outer_attention if mode == "outer" else O.inner_attention
            self._ref[key] = fn(to_np64(self.x), None, self.w64, self.coef.numpy().astype(np.float64), fused)
            self._ref[key].setflags(write=False)
        return self._ref[key]

    def store(self, n_steps=2):
        k_fs, vt_fs = ops.endpoint_block_sizes(self.s, self.c)
        return dict(k_store=torch.full((n_steps, 2, k_fs), float("nan"), dtype=self.dtype, device=DEV),
                    vt_store=torch.full((n_steps, 2, vt_fs), float("nan"), dtype=self.dtype, device=DEV),
                    step=torch.zeros(1, dtype=torch.int32, device=DEV))

    def record(self, st, mode, fused, x=None, **kw):
        return ops.processor_ep_fwd(self.x if x is None else x, *self.w, self.bo, self.heads, ep=dict(st, mode="record"), mode=mode,
                                    fused=fused, coef=self.coef.to(DEV), begin=0, end=N - 1, **kw)

    def replay(self, st, mode, fused, rows, x=None, riders=0, **kw):
        x = (self.x if x is None else x)[rows].contiguous()
        coef = self.coef[rows]
        if riders:
            x = torch.cat([x, self.riders[:riders]])
            coef = torch.cat([coef, -torch.ones(riders)])
        return ops.processor_ep_fwd(x, *self.w, self.bo, self.heads, ep=dict(st, mode="replay"), mode=mode, fused=fused,
                                    coef=coef.to(DEV), n_plain=riders, **kw)


_LAYERS = {}


def _layer(s, c, heads, dtype):
    key = (s, c, heads, dtype)
    if key not in _LAYERS:
        _LAYERS[key] = _Layer(s, c, heads, dtype)
    return _LAYERS[key]


@pytest.mark.parametrize("dtype", [F16, BF16, F32], ids=["f16", "bf16", "f32"])
@pytest.mark.parametrize("s,c,heads", SHAPES, ids=["d40", "d64", "d80", "d160"])
@pytest.mark.parametrize("mode,fused", MODES, ids=["pure_outer", "fused_outer", "pure_inner", "fused_inner"])
def test_record_is_the_plain_call_and_replay_meets_its_bounds(mode, fused, s, c, heads, dtype):
    L = _layer(s, c, heads, dtype)
    st = L.store()
    st["step"].fill_(1)
    y_plain = ops.processor_fwd(L.x, None, *L.w, L.bo, heads, mode=mode, fused=fused, coef=L.coef.to(DEV), begin=0, end=N - 1)
    y_rec = L.record(st, mode, fused)
    assert torch.equal(_bits(y_rec), _bits(y_plain))                                  # RECORD: y bit for bit
    assert torch.isnan(st["k_store"][0].float()).all() and torch.isfinite(st["k_store"][1].float()).all()    # slot 1 alone was written
    assert torch.isnan(st["vt_store"][0].float()).all()
    ref = L.ref(mode, fused)
    _close(y_rec, ref, dtype, "record (the full batch)")
    _close(L.replay(st, mode, fused, slice(1, 4)), ref[1:4], dtype, "replay of frames 1..3")
    _close(L.replay(st, mode, fused, slice(2, 3)), ref[2:3], dtype, "replay of frame 2 alone")


@pytest.mark.parametrize("mode,fused", [("outer", True), ("inner", False)], ids=["fused_outer", "pure_inner"])
def test_replay_with_cfg_riders(mode, fused):
    """The unconditional half of a batched classifier-free-guidance step rides in the replay call with negative coefficients."""
    L = _layer(33, 128, 2, F16)
    st = L.store()
    L.record(st, mode, fused)
    y = L.replay(st, mode, fused, slice(1, 4), riders=2)
    ref = np.concatenate([L.ref(mode, fused)[1:4], O.plain_attention(to_np64(L.riders), None, L.w64)])
    _close(y, ref, F16, "replay of frames 1..3 + 2 PLAIN riders")


# ---- the library call at shapes that reach the production engines ---------------------------------------------------------------------
# SHAPES above stay at S <= 40 (resident, text-key, one tile of the streaming kernel).  These reach the ping-pong kernel by the default
# rule (S = 1024, d = 64: the path of the SDXL self-attention layers) and alone under ATTN_V2 = 1, the streaming program-order kernel
# with several key tiles and query blocks (d = 40, d = 160) and the fp32 kernel.  (s, c, heads, dtype, mode, fused, knobs, variant)
def _engine_cases():
    out = []
    for dt in (BF16, F16):
        for mode in ("outer", "inner"):
            out.append((1024, 64, 1, dt, mode, True, {}, f"aid_attn_pp<d64,{mode}>"))
    for mode in ("outer", "inner"):
        out.append((512, 128, 2, BF16, mode, False, {"ATTN_V2": 1}, f"aid_attn_pp<d64,{mode}>"))
    for dt in (F16, F32):
        for mode, fused in MODES:
            out.append((200, 80, 2, dt, mode, fused, {}, "aid_attn_f32" if dt == F32 else "d40"))
    out.append((136, 160, 1, BF16, "outer", True, {}, "d160"))
    ids = {F16: "f16", BF16: "bf16", F32: "f32"}
    return [pytest.param(*c, id=f"s{c[0]}-c{c[1]}-{ids[c[3]]}-{'fused' if c[5] else 'pure'}_{c[4]}") for c in out]


def _assert_variant(variant, what):
    name = ops.last_attn_variant()
    if variant.startswith("aid_attn_"):
        assert name == variant, (what, name)
    else:
        assert name.startswith("aid_attn<") and f",{variant}," in name, (what, name)


def _poison_workspace(byte):
    """Fill the library workspace of the current stream (one buffer reused by every call) with ``byte``."""
    ops.workspace(1, torch.device(DEV)).fill_(byte)


@pytest.mark.parametrize("s,c,heads,dtype,mode,fused,knobs,variant", _engine_cases())
def test_replay_on_the_production_engines(s, c, heads, dtype, mode, fused, knobs, variant, tuning):
    """Record, then replay frames 1..3 and frame 2 alone against the fp64 oracle of the full batch, the engine asserted by name after
    each replay call; the S = 1024 shape also with two CFG riders.  (Nothing is compared bit for bit across record and replay: the
    smaller m takes another GEMM tile plan.)"""
    for name, value in knobs.items():
        tuning(name, value)
    L = _layer(s, c, heads, dtype)
    st = L.store()
    L.record(st, mode, fused)
    ref = L.ref(mode, fused)
    y = L.replay(st, mode, fused, slice(1, 4))
    _assert_variant(variant, "frames 1..3")
    _close(y, ref[1:4], dtype, "replay of frames 1..3")
    y = L.replay(st, mode, fused, slice(2, 3))
    _assert_variant(variant, "frame 2 alone")
    _close(y, ref[2:3], dtype, "replay of frame 2 alone")
    if s == 1024:
        y = L.replay(st, mode, fused, slice(1, 4), riders=2)
        _assert_variant(variant, "frames 1..3 + 2 riders")
        _close(y, np.concatenate([ref[1:4], O.plain_attention(to_np64(L.riders), None, L.w64)]), dtype, "replay of frames 1..3 + 2 riders")


@pytest.mark.parametrize("mode", ["outer", "inner"])
@pytest.mark.parametrize("s", [75, 512], ids=lambda s: f"s{s}")
def test_replay_does_not_depend_on_stale_workspace(s, mode):
    """The two stored rows live in the workspace behind the projected ones (S = 75: V^T rows with pad columns).  After a larger call
    has left its data there, the same replay on a workspace of 0xFF bytes (NaN) and on one of zeros gives equal, finite bits (as
    test_hip_memory_contracts.py::test_processor_output_does_not_depend_on_stale_workspace)."""
    c, heads, dtype = 128, 2, BF16
    L = _layer(s, c, heads, dtype)
    st = L.store()
    L.record(st, mode, True)
    big = torch.randn(N, 2 * s + 256, c, device=DEV).to(dtype)
    outs = []
    for byte in (0xFF, 0x00):
        ops.processor_fwd(big, None, *L.w, L.bo, heads, mode=mode, fused=True, coef=L.coef.to(DEV), begin=0, end=N - 1)
        _poison_workspace(byte)
        outs.append(L.replay(st, mode, True, slice(1, 4), riders=1).clone())
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), "the replay depends on the workspace contents"
    ref = np.concatenate([L.ref(mode, True)[1:4], O.plain_attention(to_np64(L.riders[:1]), None, L.w64)])
    _close(outs[0], ref, dtype, "replay on a poisoned workspace")


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_replay_with_a_lora_segment(dtype):
    """Unmerged LoRA adapters on q / k / v: the same code path; the oracle computes with W + B A."""
    s, c, heads, r = 40, 320, 8, 64
    L = _layer(s, c, heads, dtype)
    g = torch.Generator().manual_seed(3)
    a_ = [(torch.randn(r, c, generator=g) * c ** -0.5).to(dtype).to(DEV) for _ in range(3)]
    b_ = [(torch.randn(c, r, generator=g) * 0.25 * r ** -0.5).to(dtype).to(DEV) for _ in range(3)]
    la = lora.LoraArgs(torch.cat(a_).contiguous(), None, None, (b_[0], b_[1], b_[2], None), (r, r, r, 0), ("test",))
    w64 = O.AttnWeights(*(to_np64(w) + to_np64(b) @ to_np64(a) for w, a, b in zip(L.w[:3], a_, b_)), to_np64(L.w[3]), to_np64(L.bo),
                        heads=heads)
    ref = O.outer_attention(to_np64(L.x), None, w64, L.coef.numpy().astype(np.float64), True)
    st = L.store()
    y_rec = L.record(st, "outer", True, lora=la)
    y_plain = ops.processor_fwd(L.x, None, *L.w, L.bo, heads, mode="outer", fused=True, coef=L.coef.to(DEV), begin=0, end=N - 1, lora=la)
    assert torch.equal(_bits(y_rec), _bits(y_plain))
    _close(L.replay(st, "outer", True, slice(1, 4), lora=la), ref[1:4], dtype, "replay with LoRA")


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("folded", [True, False], ids=["folded", "own_pass"])
def test_replay_with_layernorm_and_residual(dtype, folded):
    """h + attn(LayerNorm(h)) in one call (the fused sublayer), the LayerNorm folded into the projections or as its own pass."""
    s, c, heads = 33, 128, 2
    L = _layer(s, c, heads, dtype)
    g = torch.Generator().manual_seed(4)
    gamma = (1 + 0.1 * torch.randn(c, generator=g)).to(dtype).to(DEV)
    beta = (0.1 * torch.randn(c, generator=g)).to(dtype).to(DEV)
    kw = dict(ln=(gamma, beta, 1e-5))
    if folded:
        const = torch.zeros(6, c, dtype=torch.float32, device=DEV)
        fq, const[0], const[1] = ops.ln_fold(L.w[0], gamma, beta)
        fk, const[2], const[3] = ops.ln_fold(L.w[1], gamma, beta)
        fv, const[4], const[5] = ops.ln_fold(L.w[2], gamma, beta)
        kw["ln_folded"] = (fq, fk, fv, const)
    x64 = to_np64(L.x)
    ref = x64 + O.inner_attention(O.layer_norm(x64, to_np64(gamma), to_np64(beta), 1e-5), None, L.w64, L.coef.numpy().astype(np.float64), True)
    st = L.store()
    y_rec = L.record(st, "inner", True, residual=L.x, **kw)
    y_plain = ops.processor_fwd(L.x, None, *L.w, L.bo, heads, mode="inner", fused=True, coef=L.coef.to(DEV), begin=0, end=N - 1,
                                residual=L.x, **kw)
    assert torch.equal(_bits(y_rec), _bits(y_plain))
    x_mid = L.x[1:4].contiguous()
    y = ops.processor_ep_fwd(x_mid, *L.w, L.bo, heads, ep=dict(st, mode="replay"), mode="inner", fused=True, coef=L.coef[1:4].to(DEV),
                             residual=x_mid, **kw)
    _close(y, ref[1:4], dtype, "replay with LayerNorm + residual")


# ---- graph capture ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,fused", [("outer", True), ("inner", True)], ids=["fused_outer", "fused_inner"])
def test_one_captured_replay_call_reads_the_slot_of_the_live_step_index(mode, fused):
    """Record two steps with different x, capture ONE replay call, replay the graph after writing 0 and after writing 1 into the
    device step index: each result is the eager replay call of that step, bit for bit, and the two differ."""
    L = _layer(33, 128, 2, F16)
    st = L.store(n_steps=2)
    x1 = (L.x.float() * 0.5 + 0.25).to(F16)
    for i, x in enumerate((L.x, x1)):
        st["step"].fill_(i)
        L.record(st, mode, fused, x=x)
    x_mid = L.x[2:3].contiguous()                          # the SAME interior frame at both steps: only the stored rows differ
    coef = L.coef[2:3].to(DEV)
    call = lambda out=None: ops.processor_ep_fwd(x_mid, *L.w, L.bo, L.heads, ep=dict(st, mode="replay"), mode=mode, fused=fused,   # noqa: E731
                                                 coef=coef, out=out)
    eager = []
    for i in range(2):
        st["step"].fill_(i)
        eager.append(call().clone())
    assert not torch.equal(eager[0], eager[1])
    side = torch.cuda.Stream()
    out = torch.empty_like(x_mid)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(out)                                         # eager warm-up on the capture stream (workspace)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call(out)
    for i in (0, 1, 0):
        st["step"].fill_(i)                               # stream-ordered, outside the graph; no node update
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(eager[i])), i
    del graph


# ---- pipelines ----------------------------------------------------------------------------------------------------------------------
STEPS, RATIO = 6, 0.5
# rel-L2 against the fp64 oracle loop that the FULL (non-replay) run measures on StackDenoiser("sd15", scale_down=16, latent_hw=(8, 8)),
# 6 steps, warm-up ratio 0.5, for the frames the replay renders — interpolate_single(0.3): frame 1 of [0, 0.3, 1];
# interpolate(size=5): frames 1..3.  Measured once on an MI355X; the replay is held to 1.3 x these (the project's convention).
PIPE_MEASURED = {
    ("single", F16): 2.107e-3,        # (the replay measures the same 2.107e-3: bound 2.739e-3)
    ("single", F32): 1.204e-6,        # (replay 1.268e-6; bound 1.565e-6)
    ("n5", F16): 1.933e-3,            # (replay 1.933e-3; bound 2.513e-3)
    ("n5", F32): 1.283e-6,            # (replay 1.256e-6; bound 1.668e-6)
}


def _embs(g, cc):
    return torch.randn(1, 77, cc, generator=g), torch.randn(1, 77, cc, generator=g)


class _Runs:
    """Everything the pipeline tests of one dtype share, run once: the plain runs, the recording run, the replays, the oracle loops."""

    def __init__(self, dtype):
        from test_hip_depth_and_pipelines import OracleDenoiser
        self.dtype = dtype
        hip = StackDenoiser("sd15", dtype=dtype, device=DEV, scale_down=16, latent_hw=(8, 8))
        g = torch.Generator().manual_seed(21)
        l0, l1 = torch.randn(1, 4, 8, 8, generator=g).to(dtype), torch.randn(1, 4, 8, 8, generator=g).to(dtype)
        rd = lambda t: tuple(e.to(dtype).float() for e in t)     # noqa: E731   every run sees the dtype-rounded embeddings
        es, ee = rd(_embs(g, hip.stack.cross_dim)), rd(_embs(g, hip.stack.cross_dim))
        self.pipe = pipe = InterpolationStableDiffusionPipeline(hip, DDIMSchedulerLite())
        pipe.load_aid(t=0.5, is_fused=True, atype="fused_outer")
        self.kw = kw = dict(latent_start=l0, latent_end=l1, embeds_start=es, embeds_end=ee, num_inference_steps=STEPS, warmup_ratio=RATIO,
                            output_type="latent")
        self.nkw = nkw = dict(embeds_start=es, embeds_end=ee, num_inference_steps=STEPS, warmup_ratio=RATIO, early="fused_outer",
                              output_type="latent")
        self.l0, self.l1, self.es, self.ee = l0, l1, es, ee
        single = lambda it, **k: pipe.interpolate_single(it, **dict(kw, **k))["images"].clone()      # noqa: E731
        self.plain_05 = single(0.5)
        self.store = EndpointStore()
        self.record_05 = single(0.5, endpoints=self.store)
        self.nbytes = self.store.nbytes
        self.full_03 = single(0.3)
        self.replay_03 = single(0.3, endpoints=self.store)
        self.replay_03_eager = single(0.3, endpoints=self.store, use_graphs=False)
        self.full_n5 = pipe.interpolate(l0, l1, size=5, **nkw).clone()
        self.replay_n5 = pipe.interpolate(l0, l1, size=5, endpoints=self.store, **nkw).clone()
        self.replay_n5_eager = pipe.interpolate(l0, l1, size=5, endpoints=self.store, use_graphs=False, **nkw).clone()
        self.plain_05_again = single(0.5)
        # the fp64 oracle loops of the FULL batches (they read the processors installed on the HIP denoiser)
        ora = InterpolationStableDiffusionPipeline(OracleDenoiser(hip), DDIMSchedulerLite())
        dbl = lambda t: tuple(e.double() for e in t)               # noqa: E731
        okw = dict(latent_start=l0.double(), latent_end=l1.double(), embeds_start=dbl(es), embeds_end=dbl(ee), num_inference_steps=STEPS,
                   warmup_ratio=RATIO, output_type="latent")
        self.ref_03 = ora.interpolate_single(0.3, **okw)["images"].numpy()
        self.ref_n5 = ora.interpolate(l0.double(), l1.double(), size=5, **dict(nkw, embeds_start=dbl(es), embeds_end=dbl(ee))).numpy()
        pipe.load_aid(t=0.5, is_fused=True, atype="fused_outer")   # (the oracle runs toggled the shared processors)
        self.figures = {
            "single": dict(full=rel_l2(to_np64(self.full_03[1:2]), self.ref_03[1:2]), replay=rel_l2(to_np64(self.replay_03[1:2]), self.ref_03[1:2])),
            "n5": dict(full=rel_l2(to_np64(self.full_n5[1:4]), self.ref_n5[1:4]), replay=rel_l2(to_np64(self.replay_n5[1:4]), self.ref_n5[1:4])),
        }
        print(f"[endpoint store] {dtype}: store {self.nbytes} bytes; rel-L2 vs the fp64 oracle loop, interior frames: {self.figures}")


_RUNS = {}


@pytest.fixture(params=[F16, F32], ids=["f16", "f32"])
def runs(request):
    if request.param not in _RUNS:
        _RUNS[request.param] = _Runs(request.param)
    return _RUNS[request.param]


def test_recording_run_is_the_run_without_the_keyword(runs):
    assert runs.record_05.shape == (3, 4, 8, 8)
    assert torch.equal(_bits(runs.record_05), _bits(runs.plain_05))
    st = runs.store
    assert st.recorded and st.mode is None and st.n_steps == int(STEPS * RATIO)
    shapes = [(s, c) for (s, c, h, cross) in runs.pipe.unet.stack.shapes if not cross]
    assert len(st.layers) == len(shapes) == 16                     # every self-attention layer of SD1.5, no cross-attention layer
    assert st.nbytes == sum(EndpointStore.layer_bytes(st.n_steps, s, c, runs.dtype) for s, c in shapes) + st.latents.numel() * st.latents.element_size()
    assert torch.equal(st.latents, torch.cat([runs.plain_05[0:1], runs.plain_05[2:3]]))


def test_replay_of_one_frame_against_the_oracle_loop_of_the_full_batch(runs):
    out = runs.replay_03
    assert out.shape == (3, 4, 8, 8)
    # the end points come from the stored latents: the recorded run's rows, bit for bit
    assert torch.equal(_bits(out[0]), _bits(runs.record_05[0])) and torch.equal(_bits(out[2]), _bits(runs.record_05[2]))
    fig = runs.figures["single"]
    bound = 1.3 * PIPE_MEASURED[("single", runs.dtype)]
    print(f"interior frame: replay {fig['replay']:.3e}, full run {fig['full']:.3e}, bound {bound:.3e}")
    assert fig["replay"] < bound, fig


def test_replay_of_three_frames_from_the_same_store(runs):
    out = runs.replay_n5
    assert out.shape == (5, 4, 8, 8)
    assert torch.equal(_bits(out[0]), _bits(runs.record_05[0])) and torch.equal(_bits(out[4]), _bits(runs.record_05[2]))
    fig = runs.figures["n5"]
    bound = 1.3 * PIPE_MEASURED[("n5", runs.dtype)]
    print(f"interior frames: replay {fig['replay']:.3e}, full run {fig['full']:.3e}, bound {bound:.3e}")
    assert fig["replay"] < bound, fig


def test_replay_with_graphs_equals_replay_without(runs):
    assert torch.equal(_bits(runs.replay_03), _bits(runs.replay_03_eager))
    assert torch.equal(_bits(runs.replay_n5), _bits(runs.replay_n5_eager))


def test_a_run_without_the_keyword_after_the_replays_reproduces_itself(runs):
    assert torch.equal(_bits(runs.plain_05_again), _bits(runs.plain_05))
    assert all(p.endpoint_store is None and p.endpoint_ctx is None for p in runs.pipe.unet.attn_processors.values())


def test_a_changed_prompt_embedding_raises(runs):
    es = (runs.es[0].clone(), runs.es[1])
    es[0][0, 5, 7] += 0.125
    with pytest.raises(ValueError, match="recorded under a different embeds_start"):
        runs.pipe.interpolate_single(0.3, endpoints=runs.store, **dict(runs.kw, embeds_start=es))
    with pytest.raises(ValueError, match="recorded under a different num_inference_steps"):
        runs.pipe.interpolate_single(0.3, endpoints=runs.store, **dict(runs.kw, num_inference_steps=STEPS + 2))
    with pytest.raises(ValueError, match="recorded under a different latent_end"):
        runs.pipe.interpolate(runs.l0, runs.l0, size=5, endpoints=runs.store, **runs.nkw)
    assert runs.store.recorded and runs.store.mode is None
    assert torch.equal(_bits(runs.pipe.interpolate_single(0.3, endpoints=runs.store, **runs.kw)["images"]), _bits(runs.replay_03))
