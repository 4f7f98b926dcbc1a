"""GPU: unmerged LoRA adapters on the attention projections (ABI v9).  The GEMM's low-rank segment against fp64 on every engine that
carries it (and the engines that are planned around it), and whole processor calls on PEFT-wrapped projections against the fp64 oracle
evaluated on the effective weights  W + sum_a s_a B_a A_a  (x W^T + sum_a s_a (x A_a^T) B_a^T is that product in exact arithmetic).
The processor cases fail on a library / package that reads the base weights only (it returns oracle(W))."""
import numpy as np
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

import aid_amd  # noqa: E402
from aid_amd import ops  # noqa: E402
from oracle import aid_oracle as O  # noqa: E402
from peft_double import effective_weight, wrap_attention  # noqa: E402
from util import TOL, TOL_GEMM, WORST, rel_l2, to_np64, worst  # noqa: E402

DEV = torch.device("cuda:0")
TOL_GEMM32 = 1e-5


@pytest.fixture
def knobs():
    set_ = []

    def put(name, value):
        ops.set_tuning(name, value)
        set_.append(name)
    yield put
    for name in set_:
        ops.set_tuning(name, -1)


def _t(shape, dtype, g, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


# engine -> (knobs, variants it may report)
ENGINES = {
    "edge": ({}, ("edge",)),
    "lockstep128": ({"GEMM_VARIANT": 7, "GEMM_LS": 0}, ("lockstep128",)),
    "lockstep128x4": ({"GEMM_VARIANT": 7, "GEMM_LS": 1}, ("lockstep128x4",)),
    # the ping-pong and row-stationary engines do not carry the segment: forcing them must leave the group on the lock-step engine
    "pingpong(forced)": ({"GEMM_VARIANT": 31, "GEMM_LS": 0}, ("lockstep128",)),
    "pingpong288(forced)": ({"GEMM_VARIANT": 31, "GEMM_TRI": 1, "GEMM_LS": 0}, ("lockstep128",)),
    "rowstat(forced)": ({"GEMM_RS": 1, "GEMM_LS": 0}, ("lockstep128",)),
}


GEMM_CASES = [(dt, e) for dt in (torch.float16, torch.bfloat16) for e in ENGINES] + [(torch.float32, "lockstep128")]   # f32: one engine


@pytest.mark.parametrize("dtype,engine", GEMM_CASES)
@pytest.mark.parametrize("r", [64, 128, 192])
def test_gemm_low_rank_segment_matches_fp64(dtype, engine, r, knobs):
    kn, variants = ENGINES[engine]
    for k_, v_ in kn.items():
        knobs(k_, v_)
    g = torch.Generator().manual_seed(r)
    m, n = 640, 320
    k = 72 if engine == "edge" else 640
    x, w = _t((m, k), dtype, g), _t((n, k), dtype, g, 0.05)
    u, bp = _t((m, r + 64), dtype, g), _t((n, r + 8), dtype, g, 0.05)       # padded rows: lr_lda / lr_ldb > lr_k
    bias, res = _t((n,), dtype, g), _t((m, n), dtype, g)
    c = torch.full((m, n), float("nan"), dtype=dtype, device=DEV)
    ops.gemm_nt([dict(a=x, b=w, c=c, bias=bias, residual=res, m=m, n=n, k=k, lda=k, ldb=k, ldc=n,
                      lr=dict(a=u, b=bp, k=r, lda=r + 64, ldb=r + 8))])
    torch.cuda.synchronize()
    if dtype != torch.float32:
        assert ops.last_gemm_variant() in variants, ops.last_gemm_variant()
    acc = to_np64(x) @ to_np64(w).T + to_np64(u)[:, :r] @ to_np64(bp)[:, :r].T + to_np64(bias)
    want = torch.from_numpy(acc).to(dtype).double().numpy() + to_np64(res)
    tol = TOL_GEMM32 if dtype == torch.float32 else 2 * TOL_GEMM[dtype]
    assert rel_l2(to_np64(c), want) < tol
    assert worst(to_np64(c), want) < (1e-4 if dtype == torch.float32 else WORST[dtype])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("form", ["flat_trans", "batched"])
def test_value_projection_forms_carry_the_segment(dtype, form, knobs):
    """V^T of a frame stack with a LoRA on to_v, in both forms the library plans (the flat transposed one is rewritten into the batched
    one for the lock-step engine: the low-rank operands swap roles with it) and batched strided operands."""
    g = torch.Generator().manual_seed(5)
    f, l, cc, c, r = 3, 72, 256, 128, 64
    e, wv = _t((f, l, cc), dtype, g), _t((c, cc), dtype, g, 0.05)
    av, bv = _t((r, cc), dtype, g, 0.05), _t((c, r), dtype, g, 0.05)
    u = torch.empty(f * l, r, dtype=dtype, device=DEV)
    ops.gemm_nt([dict(a=e, b=av, c=u, m=f * l, n=r, k=cc, lda=cc, ldb=cc, ldc=r)])
    lp = (l + 7) // 8 * 8
    vt = torch.full((f, c, lp), float("nan"), dtype=dtype, device=DEV)
    if form == "flat_trans":
        p = dict(a=e, b=wv, c=vt, m=f * l, n=c, k=cc, lda=cc, ldb=cc, ldc=lp, stride_c=c * lp, trans_rows=l,
                 lr=dict(a=u, b=bv, k=r, lda=r, ldb=r))
    else:
        p = dict(a=wv, b=e, c=vt, m=c, n=l, k=cc, lda=cc, ldb=cc, ldc=lp, batch=f, stride_a=0, stride_b=l * cc, stride_c=c * lp,
                 lr=dict(a=bv, b=u, k=r, lda=r, ldb=r, stride_a=0, stride_b=l * r))
    ops.gemm_nt([p])
    torch.cuda.synchronize()
    un = torch.from_numpy(to_np64(e).reshape(f * l, cc) @ to_np64(av).T).to(dtype).double().numpy()
    v = to_np64(e) @ to_np64(wv).T + (un @ to_np64(bv).T).reshape(f, l, c)
    want = torch.from_numpy(v.transpose(0, 2, 1)).to(dtype).double().numpy()
    tol = TOL_GEMM32 if dtype == torch.float32 else 2 * TOL_GEMM[dtype]
    assert rel_l2(to_np64(vt[:, :, :l]), want) < tol


# ---- processor calls on PEFT-wrapped projections ---------------------------------------------------------------------------------
def _weights(attn):
    return O.AttnWeights(*(effective_weight(m).numpy() for m in (attn.to_q, attn.to_k, attn.to_v, attn.to_out[0])),
                         to_np64(attn.to_out[0].bias), heads=attn.heads)


def _attn(c, heads, cc, dtype, adapters, targets, seed=0):
    torch.manual_seed(seed)
    attn = aid_amd.AttnShim(c, heads, cc, dtype=dtype, device=DEV)
    wrap_attention(attn, adapters, targets=targets, seed=seed)
    for m in (attn.to_q, attn.to_k, attn.to_v, attn.to_out[0]):
        if hasattr(m, "lora_A"):
            m.to(DEV)
    return attn


CASES = [   # (c, heads, cross dim, adapters, targets)
    (320, 8, None, {"a": (8, 8.0)}, ("to_q", "to_k", "to_v", "to_out")),                  # SD 1.5 d = 40, rank 8
    (640, 8, 768, {"a": (64, 32.0)}, ("to_q", "to_k", "to_v", "to_out")),                 # SD 1.5 d = 80, cross, rank 64
    (1280, 8, None, {"a": (128, 64.0)}, ("to_q", "to_v")),                                # SD 1.5 d = 160, subset, rank 128
    (640, 10, 2048, {"a": (8, 8.0), "b": (16, 4.0)}, ("to_q", "to_k", "to_v", "to_out")), # SDXL d = 64, two stacked adapters
    (640, 10, None, {"a": (64, 16.0)}, ("to_k", "to_out")),                               # SDXL d = 64, self, subset
]


PROC_KINDS = [(dt, k) for dt in (torch.float16, torch.bfloat16) for k in ("fused_outer", "inner", "outer", "fused_inner")] + \
    [(torch.float32, k) for k in ("fused_outer", "inner")]                 # float32: two modes cover its kernels


@pytest.mark.parametrize("dtype,kind", PROC_KINDS)
@pytest.mark.parametrize("case", range(len(CASES)))
def test_processor_with_unmerged_lora_matches_the_oracle_on_effective_weights(dtype, case, kind):
    c, heads, cc, adapters, targets = CASES[case]
    attn = _attn(c, heads, cc, dtype, adapters, targets, seed=case)
    g = torch.Generator().manual_seed(case + 10)
    n, s, l = 5, 96, 77
    x = _t((n, s, c), dtype, g)
    ctx = _t((n, l, cc), dtype, g) if cc else None
    fused = kind.startswith("fused")
    mode = kind.split("_")[-1]
    cls = aid_amd.OuterInterpolatedAttnProcessor if mode == "outer" else aid_amd.InnerInterpolatedAttnProcessor
    proc = cls(size=n, is_fused=fused, alpha=50, beta=50)
    y = proc(attn, x, encoder_hidden_states=ctx)
    fn = O.outer_attention if mode == "outer" else O.inner_attention
    coef = proc.coef.to(dtype).float().numpy()
    ref = fn(to_np64(x), None if ctx is None else to_np64(ctx), _weights(attn), coef, fused)
    tol = 1e-4 if dtype == torch.float32 else TOL[dtype]
    assert rel_l2(to_np64(y), ref) < tol
    assert worst(to_np64(y), ref) < (1e-3 if dtype == torch.float32 else WORST[dtype])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("cross", [False, True])
def test_fused_sublayer_with_lora_takes_the_unfolded_layernorm(dtype, cross):
    c, heads, cc = 640, 10, 768
    attn = _attn(c, heads, cc if cross else None, dtype, {"a": (64, 32.0)}, ("to_q", "to_k", "to_v", "to_out"), seed=3)
    norm = nn.LayerNorm(c, dtype=dtype, device=DEV)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        norm.weight.copy_(1 + 0.1 * torch.randn(c, generator=g))
        norm.bias.copy_(0.1 * torch.randn(c, generator=g))
    x = _t((5, 96, c), dtype, g)
    ctx = _t((5, 77, cc), dtype, g) if cross else None
    proc = aid_amd.OuterInterpolatedAttnProcessor(size=5, is_fused=True, alpha=50, beta=50)
    y = proc.fused_sublayer(attn, norm, x, ctx)
    xn = to_np64(x)
    h = torch.from_numpy(O.layer_norm(xn, to_np64(norm.weight), to_np64(norm.bias), norm.eps)).to(dtype).double().numpy()
    ref = xn + O.outer_attention(h, None if ctx is None else to_np64(ctx), _weights(attn), proc.coef.to(dtype).float().numpy(), True)
    assert rel_l2(to_np64(y), ref) < 2 * TOL[dtype]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_ip_adapter_processor_with_lora(dtype):
    c, heads, cc, t = 640, 10, 768, 4
    attn = _attn(c, heads, cc, dtype, {"a": (64, 32.0)}, ("to_q", "to_k", "to_v", "to_out"), seed=7)
    ipp = aid_amd.HipIPAdapterAttnProcessor(hidden_size=c, cross_attention_dim=cc, num_tokens=(t,), scale=0.6).to(DEV, dtype)
    g = torch.Generator().manual_seed(8)
    x, text, ip = _t((3, 96, c), dtype, g), _t((3, 77, cc), dtype, g), _t((3, t, cc), dtype, g)
    y = ipp(attn, x, encoder_hidden_states=(text, [ip]))
    ipw = O.IPWeights(to_np64(ipp.to_k_ip[0].weight), to_np64(ipp.to_v_ip[0].weight), 0.6, t)
    ref = O.ip_adapter_attention(to_np64(x), to_np64(text), to_np64(ip), _weights(attn), ipw)
    assert rel_l2(to_np64(y), ref) < TOL[dtype]


# ---- behaviour ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ["no_active_adapter", "disabled", "merged"])
@pytest.mark.parametrize("cross", [False, True])
def test_inactive_or_merged_adapters_are_bit_identical_to_plain_linear(state, cross):
    dtype, c, heads, cc = torch.float16, 640, 10, 768
    attn = _attn(c, heads, cc if cross else None, dtype, {"a": (64, 32.0)}, ("to_q", "to_k", "to_v", "to_out"), seed=11)
    mods = (attn.to_q, attn.to_k, attn.to_v, attn.to_out[0])
    for m in mods:
        if state == "no_active_adapter":
            m.set_adapter("other")
        elif state == "disabled":
            m.enable_adapters(False)
        else:
            m.merge()
    plain = aid_amd.AttnShim(c, heads, cc if cross else None, dtype=dtype, device=DEV)
    with torch.no_grad():
        for dst, src in zip((plain.to_q, plain.to_k, plain.to_v, plain.to_out[0]), mods):
            dst.weight.copy_(src.weight)
        plain.to_out[0].bias.copy_(attn.to_out[0].bias)
    g = torch.Generator().manual_seed(12)
    x = _t((5, 96, c), dtype, g)
    ctx = _t((5, 77, cc), dtype, g) if cross else None
    p1 = aid_amd.OuterInterpolatedAttnProcessor(size=5, is_fused=True)
    p2 = aid_amd.OuterInterpolatedAttnProcessor(size=5, is_fused=True)
    assert torch.equal(p1(attn, x, encoder_hidden_states=ctx), p2(plain, x, encoder_hidden_states=ctx))


def test_scale_change_between_cross_attention_calls_misses_the_text_kv_cache():
    dtype, c, heads, cc = torch.float16, 640, 10, 768
    attn = _attn(c, heads, cc, dtype, {"a": (64, 32.0)}, ("to_q", "to_k", "to_v", "to_out"), seed=13)
    g = torch.Generator().manual_seed(14)
    x, ctx = _t((5, 96, c), dtype, g), _t((5, 77, cc), dtype, g)
    proc = aid_amd.OuterInterpolatedAttnProcessor(size=5, is_fused=True)
    y1 = proc(attn, x, encoder_hidden_states=ctx)
    for m in (attn.to_k, attn.to_v):                       # only the k / v adapters: the cached keys / values must be re-projected
        m.scale_layer(0.25)
    y2 = proc(attn, x, encoder_hidden_states=ctx)
    assert not torch.equal(y1, y2)
    ref = O.outer_attention(to_np64(x), to_np64(ctx), _weights(attn), proc.coef.to(dtype).float().numpy(), True)
    assert rel_l2(to_np64(y2), ref) < TOL[dtype]


# ---- memory contract of the low-rank operands (tests/guarded.py) -------------------------------------------------------------------
def _mask(gd, rows, cols):
    """bool [numel] of the elements (row < rows, column < cols) of frame 0 of a Guarded buffer."""
    L = gd.layout
    m = torch.zeros(L.numel, dtype=torch.bool)
    idx = L.front + torch.arange(rows)[:, None] * L.ld + torch.arange(cols)[None, :]
    m[idx.flatten()] = True
    return m


LR_CONTRACT = [(dt, e) for dt in (torch.float16, torch.bfloat16) for e in ("edge", "lockstep128", "lockstep128x4")] + \
    [(torch.float32, "f32")]


@pytest.mark.parametrize("dtype,engine", LR_CONTRACT)
def test_gemm_low_rank_operands_memory_contract(dtype, engine, knobs):
    """Ragged m / n (row clamping of the low-rank tiles), NaN in the columns past lr_k of both low-rank operands, in the row gaps of
    every operand and in the guard bands; C starts as the sentinel: exactly [m, round_up(n, 4)) is written, the pad column is +0,
    the inputs are unchanged and the valid region matches fp64."""
    from guarded import Guarded
    for k_, v_ in ENGINES.get(engine, ({}, ()))[0].items():
        knobs(k_, v_)
    m, n, r = 301, 203, 128
    k = 72 if engine == "edge" else 128
    g = torch.Generator().manual_seed(31)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(dtype)    # noqa: E731
    A = Guarded(1, m, k, dtype, DEV, ld=k + 8).set(rnd(m, k))
    B = Guarded(1, n, k, dtype, DEV, ld=k + 8).set(rnd(n, k, sc=0.05))
    LA = Guarded(1, m, r, dtype, DEV, ld=r + 64).set(rnd(m, r))
    LB = Guarded(1, n, r, dtype, DEV, ld=r + 8).set(rnd(n, r, sc=0.05))
    R = Guarded(1, m, n, dtype, DEV, ld=208).set(rnd(m, n))
    bias = rnd(n).to(DEV)
    C = Guarded(1, m, n, dtype, DEV, ld=208, kind="output")
    ops.gemm_nt([dict(a=A.view[0], b=B.view[0], c=C.view[0], bias=bias, residual=R.view[0], m=m, n=n, k=k, lda=A.ld, ldb=B.ld,
                      ldc=C.ld, lr=dict(a=LA.view[0], b=LB.view[0], k=r, lda=LA.ld, ldb=LB.ld))])
    torch.cuda.synchronize()
    if dtype != torch.float32:
        assert ops.last_gemm_variant() == engine, ops.last_gemm_variant()
    acc = to_np64(A.view[0]) @ to_np64(B.view[0]).T + to_np64(LA.view[0]) @ to_np64(LB.view[0]).T + to_np64(bias)
    want = torch.from_numpy(acc).to(dtype).double().numpy() + to_np64(R.view[0])
    got = to_np64(C.view[0])
    assert np.isfinite(got).all()
    assert rel_l2(got, want) < (TOL_GEMM32 if dtype == torch.float32 else 2 * TOL_GEMM[dtype])
    n4 = (n + 3) // 4 * 4
    writable = _mask(C, m, n4)
    assert C.untouched(writable) == ""
    assert C.pad_is_zero(writable & ~_mask(C, m, n)) == ""
    for gd in (A, B, LA, LB, R):
        assert gd.inputs_unchanged() == ""


# ---- the plain processor (de-activated passes) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("cross", [False, True])
def test_plain_processor_call_and_sublayer_with_lora(dtype, cross):
    c, heads, cc = 640, 10, 768
    attn = _attn(c, heads, cc if cross else None, dtype, {"a": (8, 8.0), "b": (64, 16.0)}, ("to_q", "to_k", "to_v", "to_out"), seed=21)
    g = torch.Generator().manual_seed(22)
    x = _t((4, 96, c), dtype, g)
    ctx = _t((4, 77, cc), dtype, g) if cross else None
    proc = aid_amd.HipAttnProcessor()
    w = _weights(attn)
    y = proc(attn, x, encoder_hidden_states=ctx)
    ref = O.plain_attention(to_np64(x), None if ctx is None else to_np64(ctx), w)
    assert rel_l2(to_np64(y), ref) < TOL[dtype] and worst(to_np64(y), ref) < WORST[dtype]
    norm = nn.LayerNorm(c, dtype=dtype, device=DEV)
    with torch.no_grad():
        norm.weight.copy_(1 + 0.1 * torch.randn(c, generator=g))
        norm.bias.copy_(0.1 * torch.randn(c, generator=g))
    y = proc.fused_sublayer(attn, norm, x, ctx)
    xn = to_np64(x)
    h = torch.from_numpy(O.layer_norm(xn, to_np64(norm.weight), to_np64(norm.bias), norm.eps)).to(dtype).double().numpy()
    ref = xn + O.plain_attention(h, None if ctx is None else to_np64(ctx), w)
    assert rel_l2(to_np64(y), ref) < 2 * TOL[dtype]


def test_lora_on_to_out_alone_keeps_the_layernorm_fold():
    from aid_amd import processors as P
    attn = _attn(640, 10, None, torch.float16, {"a": (8, 8.0)}, ("to_out",), seed=23)
    norm = nn.LayerNorm(640, dtype=torch.float16, device=DEV)
    assert P._ln_folded(attn, norm, False) is not None
    attn = _attn(640, 10, None, torch.float16, {"a": (8, 8.0)}, ("to_v",), seed=23)
    assert P._ln_folded(attn, norm, False) is None


# ---- pipelines over the stand-in UNet with wrapped layers ------------------------------------------------------------------------------
def _lora_stack(model, dtype, seed, r=8):
    from aid_amd.pipelines import StackDenoiser
    hip = StackDenoiser(model, dtype=dtype, device=DEV, scale_down=16 if model == "sd15" else 64, latent_hw=(8, 8))
    for i, m in enumerate(hip.stack.layers):
        wrap_attention(m, {"a": (r, r / 4.0)}, seed=seed + i)      # scaling 1 / 4: a style adapter's share of the weights
    return hip


def _oracle_weights_of(hip):
    """Point the fp64 oracle loop of test_hip_depth_and_pipelines at the EFFECTIVE weights of the wrapped layers (its weight cache is
    keyed by module; OracleDenoiser reads it through _w)."""
    import test_hip_depth_and_pipelines as D
    for m in hip.stack.layers:
        D._W64[id(m)] = (m, _weights(m))


@pytest.mark.parametrize("model,dtype,atype", [("sd15", torch.float16, "fused_inner"), ("sdxl", torch.bfloat16, "fused_outer")])
def test_interpolate_single_with_unmerged_lora_graphs_and_oracle(model, dtype, atype):
    from aid_amd.pipelines import DDIMSchedulerLite, InterpolationStableDiffusionPipeline, InterpolationStableDiffusionXLPipeline
    from test_hip_depth_and_pipelines import PIPE_BOUND, OracleDenoiser, _embs
    hip = _lora_stack(model, dtype, 40)
    cls = InterpolationStableDiffusionXLPipeline if model == "sdxl" else InterpolationStableDiffusionPipeline
    g = torch.Generator().manual_seed(41)
    l0, l1 = torch.randn(1, 4, 8, 8, generator=g), torch.randn(1, 4, 8, 8, generator=g)
    rd = lambda t: tuple(e.to(dtype).float() for e in t)     # noqa: E731
    es, ee = rd(_embs(g, hip.stack.cross_dim, model == "sdxl")), rd(_embs(g, hip.stack.cross_dim, model == "sdxl"))
    pipe = cls(hip, DDIMSchedulerLite())
    pipe.load_aid(t=0.5, is_fused=True, atype=atype)
    kw = dict(latent_start=l0, latent_end=l1, embeds_start=es, embeds_end=ee, num_inference_steps=3, warmup_ratio=0.5,
              output_type="latent")
    captured = pipe.interpolate_single(0.35, use_graphs=True, **kw)["images"]
    eager = pipe.interpolate_single(0.35, use_graphs=False, **kw)["images"]
    assert torch.isfinite(captured).all() and torch.equal(captured, eager)
    _oracle_weights_of(hip)
    ora = cls(OracleDenoiser(hip), DDIMSchedulerLite())
    ref = ora.interpolate_single(0.35, latent_start=l0.to(dtype).double(), latent_end=l1.to(dtype).double(),
                                 embeds_start=tuple(e.double() for e in es), embeds_end=tuple(e.double() for e in ee),
                                 num_inference_steps=3, warmup_ratio=0.5, output_type="latent")["images"]
    assert rel_l2(to_np64(captured), ref.numpy()) < PIPE_BOUND[dtype]


@pytest.mark.parametrize("batched", [True, False])
def test_n_frame_interpolate_with_unmerged_lora_graphs_and_merged_weights(batched):
    from aid_amd.pipelines import DDIMSchedulerLite, InterpolationStableDiffusionPipeline
    from test_hip_depth_and_pipelines import PIPE_BOUND, _embs
    dtype = torch.float16
    hip = _lora_stack("sd15", dtype, 50)
    g = torch.Generator().manual_seed(51)
    l0, l1 = torch.randn(1, 4, 8, 8, generator=g).to(dtype), torch.randn(1, 4, 8, 8, generator=g).to(dtype)
    rd = lambda t: tuple(e.to(dtype).float() for e in t)     # noqa: E731
    es, ee, eg = (rd(_embs(g, hip.stack.cross_dim)) for _ in range(3))
    pipe = InterpolationStableDiffusionPipeline(hip, DDIMSchedulerLite())
    pipe.load_aid(t=0.5, is_fused=True, atype="fused_inner")
    kw = dict(embeds_start=es, embeds_end=ee, embeds_guide=eg, size=5, num_inference_steps=4, warmup_ratio=0.5,
              early="fused_outer", guidance_scale=4.0, output_type="latent", batched_cfg=batched)
    captured = pipe.interpolate(l0, l1, use_graphs=True, **kw)
    eager = pipe.interpolate(l0, l1, use_graphs=False, **kw)
    assert torch.isfinite(captured).all() and torch.equal(captured, eager)
    for m in hip.stack.layers:                            # the same adapters merged into the weights (fuse_lora): the same run
        for lin in (m.to_q, m.to_k, m.to_v, m.to_out[0]):
            lin.merge()
    merged = pipe.interpolate(l0, l1, use_graphs=True, **kw)
    assert not torch.equal(merged, captured)              # different roundings ...
    assert rel_l2(to_np64(captured), to_np64(merged)) < 2 * PIPE_BOUND[dtype]     # ... of the same arithmetic (each within the bound of fp64)
