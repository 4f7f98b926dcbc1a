"""GPU: DoRA adapters on the attention projections (ABI v10).  The gain kernel against fp64, the GEMM's row gain on every engine that
carries the low-rank segment against fp64, whole processor calls on DoRA-wrapped projections against the fp64 oracle evaluated on the
effective weights  g o (W + s B A)  (tests/peft_dora_double.py), and the caches.  The processor cases fail on a package that refuses
DoRA (NotImplementedError) and on one that drops the gain (the magnitudes are the row norms times U(0.5, 1.5)).

Every test prints the rel-L2 it measured before it asserts; DESIGN.md §3.6b "DoRA" is where those figures are recorded."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import aid_amd  # noqa: E402
from aid_amd import _lib, lora, ops  # noqa: E402
from guarded import Guarded  # noqa: E402
from oracle import aid_oracle as O  # noqa: E402
from peft_double import wrap_attention  # noqa: E402
from peft_dora_double import effective_weight_dora, wrap_attention_dora  # noqa: E402
from util import TOL, TOL_GEMM, WORST, rel_l2, to_np64, worst  # noqa: E402

DEV = torch.device("cuda:0")
TOL_GEMM32 = 1e-5
DTYPES = [torch.float16, torch.bfloat16, torch.float32]


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


def _gain(n, g):
    return (0.5 + torch.rand(n, generator=g)).to(DEV)           # fp32, U(0.5, 1.5)


def _gemm_tol(dtype):
    return (TOL_GEMM32, 1e-4) if dtype == torch.float32 else (2 * TOL_GEMM[dtype], WORST[dtype])


# ---- aid_dora_gain ---------------------------------------------------------------------------------------------------------------------
N_OUT, N_IN, LDW = 200, 328, 336


def _gain_inputs(dtype, rank, seed, n_out=N_OUT, n_in=N_IN):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n_out, n_in, generator=g).to(dtype)
    a = (torch.randn(rank, n_in, generator=g) / n_in ** 0.5).to(dtype)
    b = (torch.randn(n_out, rank, generator=g) / rank ** 0.5).to(dtype)
    mag = (torch.linalg.norm(w.float(), dim=1) * (0.5 + torch.rand(n_out, generator=g))).to(dtype)
    t = w.double() + b.double() @ a.double()
    want = (mag.double() / torch.linalg.norm(t, dim=1)).numpy()
    return w, a, b, mag, want


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rank", [64, 192])
def test_dora_gain_matches_fp64(dtype, rank):
    w, a, b, mag, want = _gain_inputs(dtype, rank, rank)
    wbuf = torch.full((N_OUT, LDW), float("nan"), dtype=dtype, device=DEV)
    wbuf[:, :N_IN] = w.to(DEV)
    got = ops.dora_gain(wbuf[:, :N_IN], a.to(DEV), b.to(DEV), mag.to(DEV))
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == (N_OUT,)
    err = rel_l2(to_np64(got), want)
    print(f"dora_gain {dtype} rank {rank}: rel-L2 {err:.3e}")
    assert err <= TOL_GEMM32


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rank", [64, 192])
def test_dora_gain_memory_contract(dtype, rank):
    """NaN in the pad columns of w and in every guard band: nothing outside w [n_out, n_in] / a_pack / b_pack / magnitude is read;
    the output starts as the sentinel: exactly n_out floats are written."""
    w, a, b, mag, want = _gain_inputs(dtype, rank, 100 + rank)
    W = Guarded(1, N_OUT, N_IN, dtype, DEV, ld=LDW).set(w)
    A = Guarded(1, rank, N_IN, dtype, DEV).set(a)
    B = Guarded(1, N_OUT, rank, dtype, DEV).set(b)
    M = Guarded(1, 1, N_OUT, dtype, DEV).set(mag)
    G = Guarded(1, 1, N_OUT, torch.float32, DEV, kind="output")
    rc = _lib.load().aid_dora_gain(W.ptr, A.ptr, B.ptr, M.ptr, G.ptr, N_OUT, N_IN, LDW, rank, ops._dtype_code(W.view),
                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    got = to_np64(G.view[0, 0])
    assert np.isfinite(got).all()
    assert rel_l2(got, want) <= TOL_GEMM32
    assert G.untouched(G.layout.region_mask()) == ""
    for gd in (W, A, B, M):
        assert gd.inputs_unchanged() == ""


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rank", [64, 512])
@pytest.mark.parametrize("n_out", [1, 3, 203])
@pytest.mark.parametrize("n_in", [8, 1280, 2048, 4096])
def test_dora_gain_rank_rows_and_widths(dtype, rank, n_out, n_in):
    """The edges of the kernel's three loops: the maximum rank 512 next to 64; n_out below DORA_ROWS = 4 and not a multiple of it (the
    last workgroup clamps its rows and drops their results); n_in of one 16-byte chunk (one wave, 63 idle lanes for 16-bit storage), of
    3 and 4 waves (1280 / 8 = 160, 2048 / 8 = 256 chunks) and of two chunks per lane (4096), rows of w 8 elements apart from the next
    (NaN in the pad).  The output is a NaN-prefilled buffer of n_out + 4 floats: exactly n_out are written.  Bound: TOL_GEMM32."""
    w, a, b, mag, want = _gain_inputs(dtype, rank, 7 * rank + n_out + n_in, n_out, n_in)
    ldw = n_in + 8
    wbuf = torch.full((n_out, ldw), float("nan"), dtype=dtype, device=DEV)
    wbuf[:, :n_in] = w.to(DEV)
    a, b, mag = a.to(DEV), b.to(DEV), mag.to(DEV)
    out = torch.full((n_out + 4,), float("nan"), dtype=torch.float32, device=DEV)
    rc = _lib.load().aid_dora_gain(wbuf.data_ptr(), a.data_ptr(), b.data_ptr(), mag.data_ptr(), out.data_ptr(), n_out, n_in, ldw, rank,
                                   ops._dtype_code(wbuf), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    got = to_np64(out[:n_out])
    assert np.isfinite(got).all()
    err = rel_l2(got, want)
    print(f"dora_gain {dtype} rank {rank} n_out {n_out} n_in {n_in}: rel-L2 {err:.3e}")
    assert err <= TOL_GEMM32
    assert bool(torch.isnan(out[n_out:]).all()), "written behind n_out"


# ---- GEMM with a row gain ---------------------------------------------------------------------------------------------------------------
ENGINES = {
    "edge": ({}, "edge"),
    "lockstep128": ({"GEMM_VARIANT": 7, "GEMM_LS": 0}, "lockstep128"),
    "lockstep128x4": ({"GEMM_VARIANT": 7, "GEMM_LS": 1}, "lockstep128x4"),
}
GEMM_CASES = [(dt, e) for dt in (torch.float16, torch.bfloat16) for e in ENGINES] + [(torch.float32, "f32")]


def _set_engine(engine, knobs):
    for k_, v_ in ENGINES.get(engine, ({}, ""))[0].items():
        knobs(k_, v_)


def _round(x64, dtype):
    return torch.from_numpy(x64).to(dtype).double().numpy()


@pytest.mark.parametrize("dtype,engine", GEMM_CASES)
def test_gemm_row_scale_by_column_matches_fp64(dtype, engine, knobs):
    """Side 2 (the weight operand is b): m and n ragged across several 128-tiles, padded low-rank rows, bias, residual and a scale; the
    gain sits in a guarded buffer (NaN around its n floats).  fp32 runs its 64-tile kernel at this shape."""
    _set_engine(engine, knobs)
    g = torch.Generator().manual_seed(3)
    m, n, r = 200, 192, 64
    k = 72 if engine == "edge" else 320
    x, w = _t((m, k), dtype, g), _t((n, k), dtype, g, 0.5)                 # scale * accumulator, bias and residual of one size
    u, bp = _t((m, r + 64), dtype, g), _t((n, r + 8), dtype, g, 0.5)
    bias, res = _t((n,), dtype, g), _t((m, n), dtype, g)
    gain = Guarded(1, 1, n, torch.float32, DEV).set(_gain(n, g))
    c = torch.full((m, n), float("nan"), dtype=dtype, device=DEV)
    ops.gemm_nt([dict(a=x, b=w, c=c, bias=bias, residual=res, m=m, n=n, k=k, lda=k, ldb=k, ldc=n, scale=0.125,
                      lr=dict(a=u, b=bp, k=r, lda=r + 64, ldb=r + 8, row_scale=gain.view[0, 0], scale_side=2))])
    torch.cuda.synchronize()
    if dtype != torch.float32:
        assert ops.last_gemm_variant() == ENGINES[engine][1], ops.last_gemm_variant()
    acc = to_np64(x) @ to_np64(w).T + to_np64(u)[:, :r] @ to_np64(bp)[:, :r].T
    want = _round(0.125 * to_np64(gain.view[0, 0])[None, :] * acc + to_np64(bias), dtype) + to_np64(res)
    tol, wtol = _gemm_tol(dtype)
    err = rel_l2(to_np64(c), want)
    print(f"gemm row_scale side 2 {dtype} {engine}: rel-L2 {err:.3e}")
    assert np.isfinite(to_np64(c)).all()
    assert err < tol and worst(to_np64(c), want) < wtol
    assert gain.inputs_unchanged() == ""
    no_gain = _round(0.125 * acc + to_np64(bias), dtype) + to_np64(res)
    assert rel_l2(to_np64(c), no_gain) > 0.05                    # a dropped gain shows at these magnitudes


@pytest.mark.parametrize("dtype,engine", GEMM_CASES)
def test_gemm_row_scale_by_row_shared_by_batches_matches_fp64(dtype, engine, knobs):
    """Side 1 (the weight operand is a, shared by the batches: the V^T[f] = Wv E_f^T form): one gain of m floats for both batches."""
    _set_engine(engine, knobs)
    g = torch.Generator().manual_seed(4)
    m, n, r, nb = 200, 192, 64, 2
    k = 72 if engine == "edge" else 320
    w, e = _t((m, k), dtype, g, 0.5), _t((nb, n, k), dtype, g)
    bw, u = _t((m, r + 8), dtype, g, 0.5), _t((nb, n, r + 64), dtype, g)
    bias, res = _t((n,), dtype, g), _t((nb, m, n), dtype, g)
    gain = Guarded(1, 1, m, torch.float32, DEV).set(_gain(m, g))
    c = torch.full((nb, m, n), float("nan"), dtype=dtype, device=DEV)
    ops.gemm_nt([dict(a=w, b=e, c=c, bias=bias, residual=res, m=m, n=n, k=k, lda=k, ldb=k, ldc=n, scale=0.125, batch=nb,
                      stride_a=0, stride_b=n * k, stride_c=m * n,
                      lr=dict(a=bw, b=u, k=r, lda=r + 8, ldb=r + 64, stride_a=0, stride_b=n * (r + 64),
                              row_scale=gain.view[0, 0], scale_side=1))])
    torch.cuda.synchronize()
    if dtype != torch.float32:
        assert ops.last_gemm_variant() == ENGINES[engine][1], ops.last_gemm_variant()
    acc = to_np64(w)[None] @ to_np64(e).transpose(0, 2, 1) + to_np64(bw)[None, :, :r] @ to_np64(u)[:, :, :r].transpose(0, 2, 1)
    want = _round(0.125 * to_np64(gain.view[0, 0])[None, :, None] * acc + to_np64(bias), dtype) + to_np64(res)
    tol, wtol = _gemm_tol(dtype)
    err = rel_l2(to_np64(c), want)
    print(f"gemm row_scale side 1 {dtype} {engine}: rel-L2 {err:.3e}")
    assert np.isfinite(to_np64(c)).all()
    assert err < tol and worst(to_np64(c), want) < wtol
    assert gain.inputs_unchanged() == ""


def test_gemm_row_scale_on_the_big_fp32_tile():
    """At least 512 tiles of 128 x 128 put the fp32 GEMM on its 128-tile kernel (23 x 23 = 529)."""
    dtype = torch.float32
    g = torch.Generator().manual_seed(6)
    m = n = 2944
    k = r = 64
    x, w = _t((m, k), dtype, g), _t((n, k), dtype, g, 0.05)
    u, bp = _t((m, r), dtype, g), _t((n, r), dtype, g, 0.05)
    bias = _t((n,), dtype, g)
    gain = _gain(n, g)
    c = torch.full((m, n), float("nan"), dtype=dtype, device=DEV)
    ops.gemm_nt([dict(a=x, b=w, c=c, bias=bias, m=m, n=n, k=k, lda=k, ldb=k, ldc=n, scale=0.125,
                      lr=dict(a=u, b=bp, k=r, lda=r, ldb=r, row_scale=gain, scale_side=2))])
    torch.cuda.synchronize()
    want = 0.125 * to_np64(gain)[None, :] * (to_np64(x) @ to_np64(w).T + to_np64(u) @ to_np64(bp).T) + to_np64(bias)
    err = rel_l2(to_np64(c), want)
    print(f"gemm row_scale fp32 128-tile: rel-L2 {err:.3e}")
    assert err < TOL_GEMM32 and worst(to_np64(c), want) < 1e-4


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["flat_trans", "batched"])
def test_value_projection_forms_carry_the_gain(dtype, form):
    """V^T of a frame stack with a DoRA adapter on to_v in both forms the library plans: the flat transposed one (side 2, applied before
    the transposition; rewritten into the batched one for the lock-step engine, the side flips with the operands) and the batched one."""
    g = torch.Generator().manual_seed(5)
    f, l, cc, c, r = 3, 72, 256, 128, 64
    e, wv = _t((f, l, cc), dtype, g), _t((c, cc), dtype, g, 0.05)
    av, bv = _t((r, cc), dtype, g, 0.05), _t((c, r), dtype, g, 0.05)
    gain = _gain(c, g)
    u = torch.empty(f * l, r, dtype=dtype, device=DEV)
    ops.gemm_nt([dict(a=e, b=av, c=u, m=f * l, n=r, k=cc, lda=cc, ldb=cc, ldc=r)])
    lp = (l + 7) // 8 * 8
    vt = torch.full((f, c, lp), float("nan"), dtype=dtype, device=DEV)
    if form == "flat_trans":
        p = dict(a=e, b=wv, c=vt, m=f * l, n=c, k=cc, lda=cc, ldb=cc, ldc=lp, stride_c=c * lp, trans_rows=l,
                 lr=dict(a=u, b=bv, k=r, lda=r, ldb=r, row_scale=gain, scale_side=2))
    else:
        p = dict(a=wv, b=e, c=vt, m=c, n=l, k=cc, lda=cc, ldb=cc, ldc=lp, batch=f, stride_a=0, stride_b=l * cc, stride_c=c * lp,
                 lr=dict(a=bv, b=u, k=r, lda=r, ldb=r, stride_a=0, stride_b=l * r, row_scale=gain, scale_side=1))
    ops.gemm_nt([p])
    torch.cuda.synchronize()
    un = _round(to_np64(e).reshape(f * l, cc) @ to_np64(av).T, dtype)
    v = to_np64(gain)[None, None, :] * (to_np64(e) @ to_np64(wv).T + (un @ to_np64(bv).T).reshape(f, l, c))
    want = _round(v.transpose(0, 2, 1), dtype)
    err = rel_l2(to_np64(vt[:, :, :l]), want)
    print(f"value projection {form} {dtype}: rel-L2 {err:.3e}")
    assert err < _gemm_tol(dtype)[0]


def test_row_scale_without_a_segment_is_refused():
    g = torch.Generator().manual_seed(7)
    x, w = _t((64, 64), torch.float16, g), _t((64, 64), torch.float16, g)
    c = torch.empty(64, 64, dtype=torch.float16, device=DEV)
    p = (_lib.AidGemmProblem * 1)()
    q = p[0]
    q.a, q.b, q.c = x.data_ptr(), w.data_ptr(), c.data_ptr()
    q.m, q.n, q.k, q.lda, q.ldb, q.ldc, q.batch = 64, 64, 64, 64, 64, 64, 1
    q.lr_row_scale, q.lr_scale_side = _gain(64, g).data_ptr(), 2
    assert _lib.load().aid_gemm_nt(p, 1, 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == -1


# ---- processor calls on DoRA-wrapped projections ------------------------------------------------------------------------------------------
def _weights(attn):
    return O.AttnWeights(*(effective_weight_dora(m).numpy() for m in (attn.to_q, attn.to_k, attn.to_v, attn.to_out[0])),
                         to_np64(attn.to_out[0].bias), heads=attn.heads)


def _attn(c, heads, cc, dtype, adapters, targets, seed=0, dora=True):
    torch.manual_seed(seed)
    attn = aid_amd.AttnShim(c, heads, cc, dtype=dtype, device=DEV)
    (wrap_attention_dora if dora else wrap_attention)(attn, adapters, targets=targets, seed=seed)
    for m in (attn.to_q, attn.to_k, attn.to_v, attn.to_out[0]):
        if hasattr(m, "lora_A"):
            m.to(DEV)
    return attn


ALL = ("to_q", "to_k", "to_v", "to_out")
CASES = [   # (c, heads, cross dim, adapters, targets)
    (320, 8, None, {"a": (8, 8.0)}, ALL),                       # SD 1.5 d = 40, self, rank 8
    (640, 8, 768, {"a": (64, 32.0)}, ALL),                      # SD 1.5 d = 80, cross, rank 64
    (640, 10, 2048, {"a": (16, 4.0)}, ("to_q", "to_v")),        # SDXL d = 64, cross, rank 16 on a subset
]
PROC_KINDS = [(dt, k) for dt in (torch.float16, torch.bfloat16) for k in ("fused_outer", "inner")] + [(torch.float32, "fused_outer")]


@pytest.mark.parametrize("dtype,kind", PROC_KINDS)
@pytest.mark.parametrize("case", range(len(CASES)))
def test_processor_with_dora_matches_the_oracle_on_effective_weights(dtype, case, kind):
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
    err = rel_l2(to_np64(y), ref)
    print(f"processor DoRA case {case} {dtype} {kind}: rel-L2 {err:.3e}")
    assert err < (1e-4 if dtype == torch.float32 else TOL[dtype])
    assert worst(to_np64(y), ref) < (1e-3 if dtype == torch.float32 else WORST[dtype])


# ---- caches ---------------------------------------------------------------------------------------------------------------------------------
def test_magnitude_edit_between_cross_attention_calls_rebuilds_gain_and_text_kv():
    dtype, c, heads, cc = torch.float16, 640, 10, 768
    attn = _attn(c, heads, cc, dtype, {"a": (64, 32.0)}, ALL, seed=13)
    g = torch.Generator().manual_seed(14)
    x, ctx = _t((5, 96, c), dtype, g), _t((5, 77, cc), dtype, g)
    proc = aid_amd.OuterInterpolatedAttnProcessor(size=5, is_fused=True)
    coef = proc.coef.to(dtype).float().numpy()
    y1 = proc(attn, x, encoder_hidden_states=ctx)
    ref1 = O.outer_attention(to_np64(x), to_np64(ctx), _weights(attn), coef, True)
    assert rel_l2(to_np64(y1), ref1) < TOL[dtype]
    with torch.no_grad():
        for m in (attn.to_k, attn.to_v):                   # only k / v: the cached keys / values must be re-projected with the new gain
            m.lora_magnitude_vector["a"].weight.mul_(1.5)
    y2 = proc(attn, x, encoder_hidden_states=ctx)
    ref2 = O.outer_attention(to_np64(x), to_np64(ctx), _weights(attn), coef, True)
    assert rel_l2(ref1, ref2) > 0.05                       # the edit shows in the oracle ...
    assert rel_l2(to_np64(y2), ref2) < TOL[dtype]          # ... and the second call follows it


@pytest.mark.parametrize("cross", [False, True])
def test_merged_dora_layer_is_bit_identical_to_plain_linear(cross):
    dtype, c, heads, cc = torch.float16, 640, 10, 768
    attn = _attn(c, heads, cc if cross else None, dtype, {"a": (64, 32.0)}, ALL, seed=11)
    mods = (attn.to_q, attn.to_k, attn.to_v, attn.to_out[0])
    for m in mods:
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


@pytest.mark.parametrize("cross", [False, True])
def test_plain_lora_is_unchanged_by_a_dora_call_on_another_module(cross):
    """No stale gain survives: a plain LoRA layer (every lora_gain_* NULL) gives the same bits before and after a DoRA call."""
    dtype, c, heads, cc = torch.float16, 640, 10, 768
    plain = _attn(c, heads, cc if cross else None, dtype, {"a": (64, 32.0)}, ALL, seed=21, dora=False)
    dora = _attn(c, heads, cc if cross else None, dtype, {"a": (64, 32.0)}, ALL, seed=22)
    g = torch.Generator().manual_seed(23)
    x = _t((5, 96, c), dtype, g)
    ctx = _t((5, 77, cc), dtype, g) if cross else None
    proc = aid_amd.OuterInterpolatedAttnProcessor(size=5, is_fused=True)
    la = lora.args(plain, dtype, DEV, cross)
    assert la.gains == (None, None, None, None)
    y1 = proc(plain, x, encoder_hidden_states=ctx).clone()
    yd = proc(dora, x, encoder_hidden_states=ctx)
    assert all(t_ is not None for t_ in lora.args(dora, dtype, DEV, cross, kv=not cross).gains[::3])
    y2 = proc(plain, x, encoder_hidden_states=ctx)
    assert torch.equal(y1, y2) and not torch.equal(yd, y1)
    import peft_double
    w = O.AttnWeights(*(peft_double.effective_weight(m).numpy() for m in (plain.to_q, plain.to_k, plain.to_v, plain.to_out[0])),
                      to_np64(plain.to_out[0].bias), heads=heads)
    ref = O.outer_attention(to_np64(x), None if ctx is None else to_np64(ctx), w, proc.coef.to(dtype).float().numpy(), True)
    assert rel_l2(to_np64(y2), ref) < TOL[dtype]
