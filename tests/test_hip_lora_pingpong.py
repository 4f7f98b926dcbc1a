"""GPU: the low-rank (LoRA) segment and the DoRA row gain on the 256-row ping-pong GEMM engine (knob GEMM_LR_PP), its 128 x 128 tail
tiles included, and the planner's choice for groups with a segment.  The 288-row engine carries no segment (with the
segment its kernel did not fit 256 registers), so GEMM_TRI = 1 must leave a segment group on the 256-row engine; a transposed value
projection with a segment is rewritten into the batched form and runs there.

References are fp64 on the dtype-rounded operands; bounds are those of tests/test_hip_lora.py / test_hip_dora.py (one output rounding:
2 * TOL_GEMM, worst element WORST; processor calls TOL / WORST).  Every case fails on a library without the knob."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import aid_amd  # noqa: E402
from aid_amd import _lib, ops  # noqa: E402
from guarded import Guarded  # noqa: E402
from oracle import aid_oracle as O  # noqa: E402
from peft_double import wrap_attention  # noqa: E402
from peft_dora_double import effective_weight_dora, wrap_attention_dora  # noqa: E402
from util import TOL, TOL_GEMM, WORST, rel_l2, to_np64, worst  # noqa: E402

DEV = torch.device("cuda:0")
DTYPES = [torch.float16, torch.bfloat16]


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


def _round(x64, dtype):
    return torch.from_numpy(x64).to(dtype).double().numpy()


def _pp(knobs, loop=1, tri=0):
    knobs("GEMM_LR_PP", 1)
    knobs("GEMM_PP", loop)
    knobs("GEMM_TRI", tri)
    knobs("GEMM_RS", 0)


def _segment_problem(m, n, k, r, dtype, seed):
    """x w^T + u[:, :r] b[:, :r]^T with padded low-rank rows, bias, residual and a scale; C starts as NaN."""
    g = torch.Generator().manual_seed(seed)
    x, w = _t((m, k), dtype, g), _t((n, k), dtype, g, 0.05)
    u, bp = _t((m, r + 64), dtype, g), _t((n, r + 8), dtype, g, 0.05)
    bias, res = _t((n,), dtype, g), _t((m, n), dtype, g)
    c = torch.full((m, n), float("nan"), dtype=dtype, device=DEV)
    prob = dict(a=x, b=w, c=c, bias=bias, residual=res, m=m, n=n, k=k, lda=k, ldb=k, ldc=n, scale=0.5,
                lr=dict(a=u, b=bp, k=r, lda=r + 64, ldb=r + 8))
    acc = to_np64(x) @ to_np64(w).T + to_np64(u)[:, :r] @ to_np64(bp)[:, :r].T
    want = _round(0.5 * acc + to_np64(bias), dtype) + to_np64(res)
    return prob, c, want


# ---- 1. the segment on each K-loop flavour ---------------------------------------------------------------------------------------------
# (GEMM_PP, GEMM_TRI): the three loops; GEMM_TRI = 1 asks for the 288-row engine, which a segment group must not get
FLAVOURS = [(0, 0), (1, 0), (2, 0), (1, 1)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("loop,tri", FLAVOURS)
@pytest.mark.parametrize("k", [64, 192])
@pytest.mark.parametrize("r", [64, 128, 192])
def test_segment_on_the_256_row_engine_matches_fp64(dtype, loop, tri, k, r, knobs):
    """m = 600: two whole 256-row tiles and a ragged one; n = 320: a whole 256-column tile and a ragged 64.  One, two and three K tiles
    in either segment reach the (N,N), (Y,N) and (Y,Y) bodies of both loops."""
    _pp(knobs, loop, tri)
    prob, c, want = _segment_problem(600, 320, k, r, dtype, seed=100 * k + r)
    ops.gemm_nt([prob])
    torch.cuda.synchronize()
    assert ops.last_gemm_variant() == "pingpong256", ops.last_gemm_variant()
    got = to_np64(c)
    assert np.isfinite(got).all()
    assert rel_l2(got, want) < 2 * TOL_GEMM[dtype]
    assert worst(got, want) < WORST[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_segment_on_the_tail_tiles_of_a_ragged_last_round(dtype, knobs):
    """One CU round of 256-tiles plus 8: the last round is cut into 128 x 128 tiles, which carry the segment like the lock-step kernel.
    m and n ragged, so tail and big tiles both meet the matrix edge."""
    _pp(knobs)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count     # tails need a CU count that is a multiple of 8 (split_pp)
    m, n = 256 * (ncu // 8 + 1) - 40, 256 * 8 - 24                      # ncu + 8 tiles of 256 x 256
    prob, c, want = _segment_problem(m, n, 64, 64, dtype, seed=7)
    ops.gemm_nt([prob])
    torch.cuda.synchronize()
    assert ops.last_gemm_variant() == "pingpong256+tail128", ops.last_gemm_variant()
    got = to_np64(c)
    assert np.isfinite(got).all()
    assert rel_l2(got, want) < 2 * TOL_GEMM[dtype]
    assert worst(got, want) < WORST[dtype]


# ---- 2. transposed values ------------------------------------------------------------------------------------------------------------
def _value_problem(form, dtype, gain=None):
    g = torch.Generator().manual_seed(5)
    f, l, cc, c, r = 3, 96, 256, 256, 64
    e, wv = _t((f, l, cc), dtype, g), _t((c, cc), dtype, g, 0.05)
    av, bv = _t((r, cc), dtype, g, 0.05), _t((c, r), dtype, g, 0.05)
    u = torch.empty(f * l, r, dtype=dtype, device=DEV)
    ops.gemm_nt([dict(a=e, b=av, c=u, m=f * l, n=r, k=cc, lda=cc, ldb=cc, ldc=r)])
    vt = torch.full((f, c, l), float("nan"), dtype=dtype, device=DEV)
    if form == "flat_trans":
        lr = dict(a=u, b=bv, k=r, lda=r, ldb=r)
        if gain is not None:
            lr.update(row_scale=gain, scale_side=2)
        p = dict(a=e, b=wv, c=vt, m=f * l, n=c, k=cc, lda=cc, ldb=cc, ldc=l, stride_c=c * l, trans_rows=l, lr=lr)
    else:
        lr = dict(a=bv, b=u, k=r, lda=r, ldb=r, stride_a=0, stride_b=l * r)
        if gain is not None:
            lr.update(row_scale=gain, scale_side=1)
        p = dict(a=wv, b=e, c=vt, m=c, n=l, k=cc, lda=cc, ldb=cc, ldc=l, batch=f, stride_a=0, stride_b=l * cc, stride_c=c * l, lr=lr)
    torch.cuda.synchronize()
    un = _round(to_np64(e).reshape(f * l, cc) @ to_np64(av).T, dtype)
    v = to_np64(e) @ to_np64(wv).T + (un @ to_np64(bv).T).reshape(f, l, c)
    if gain is not None:
        v = v * to_np64(gain)[None, None, :]
    return p, vt, _round(v.transpose(0, 2, 1), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dora", [False, True])
def test_transposed_value_projection_with_a_segment_runs_on_ping_pong(dtype, dora, knobs):
    """The flat trans_rows form with a segment (and a side-2 gain) asked onto ping-pong: no engine that carries a segment writes
    transposed C, so it is rewritten into the batched form (operands and gain side swap) and runs on the 256-row engine.  Same fp64
    reference as the batched form on the lock-step engine, and the two outputs within one rounding of each other."""
    gain = (0.5 + torch.rand(256, generator=torch.Generator().manual_seed(9))).to(DEV) if dora else None
    _pp(knobs, tri=1)
    p, vt, want = _value_problem("flat_trans", dtype, gain)
    ops.gemm_nt([p])
    torch.cuda.synchronize()
    assert ops.last_gemm_variant() == "pingpong256", ops.last_gemm_variant()
    knobs("GEMM_LR_PP", 0)
    knobs("GEMM_VARIANT", 7)
    p2, vt2, _ = _value_problem("batched", dtype, gain)
    ops.gemm_nt([p2])
    torch.cuda.synchronize()
    assert ops.last_gemm_variant().startswith("lockstep128"), ops.last_gemm_variant()
    assert rel_l2(to_np64(vt), want) < 2 * TOL_GEMM[dtype]
    assert rel_l2(to_np64(vt2), want) < 2 * TOL_GEMM[dtype]
    assert rel_l2(to_np64(vt), to_np64(vt2)) < 2 * TOL_GEMM[dtype]
    if dora:
        p3, _, no_gain = _value_problem("batched", dtype, None)
        assert rel_l2(to_np64(vt), no_gain) > 0.05


# ---- 3. DoRA gain ----------------------------------------------------------------------------------------------------------------------
def _gain(n, g):
    return (0.5 + torch.rand(n, generator=g)).to(DEV)           # fp32, U(0.5, 1.5)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("loop", [0, 1])
def test_row_gain_by_column_on_the_256_row_engine(dtype, loop, knobs):
    _pp(knobs, loop)
    g = torch.Generator().manual_seed(3)
    m, n, k, r = 600, 320, 192, 64
    x, w = _t((m, k), dtype, g), _t((n, k), dtype, g, 0.5)
    u, bp = _t((m, r + 64), dtype, g), _t((n, r + 8), dtype, g, 0.5)
    bias, res = _t((n,), dtype, g), _t((m, n), dtype, g)
    gain = Guarded(1, 1, n, torch.float32, DEV).set(_gain(n, g))
    c = torch.full((m, n), float("nan"), dtype=dtype, device=DEV)
    ops.gemm_nt([dict(a=x, b=w, c=c, bias=bias, residual=res, m=m, n=n, k=k, lda=k, ldb=k, ldc=n, scale=0.125,
                      lr=dict(a=u, b=bp, k=r, lda=r + 64, ldb=r + 8, row_scale=gain.view[0, 0], scale_side=2))])
    torch.cuda.synchronize()
    assert ops.last_gemm_variant() == "pingpong256", ops.last_gemm_variant()
    acc = to_np64(x) @ to_np64(w).T + to_np64(u)[:, :r] @ to_np64(bp)[:, :r].T
    want = _round(0.125 * to_np64(gain.view[0, 0])[None, :] * acc + to_np64(bias), dtype) + to_np64(res)
    got = to_np64(c)
    assert np.isfinite(got).all()
    assert rel_l2(got, want) < 2 * TOL_GEMM[dtype] and worst(got, want) < WORST[dtype]
    assert gain.inputs_unchanged() == ""
    no_gain = _round(0.125 * acc + to_np64(bias), dtype) + to_np64(res)
    assert rel_l2(got, no_gain) > 0.05                           # a dropped gain shows at these magnitudes


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("loop", [0, 1])
def test_row_gain_by_row_shared_by_batches_on_the_256_row_engine(dtype, loop, knobs):
    """Side 1: the weight operand is a, shared by two batches — one gain of m floats for both."""
    _pp(knobs, loop)
    g = torch.Generator().manual_seed(4)
    m, n, k, r, nb = 600, 320, 192, 64, 2
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
    assert ops.last_gemm_variant() == "pingpong256", ops.last_gemm_variant()
    acc = to_np64(w)[None] @ to_np64(e).transpose(0, 2, 1) + to_np64(bw)[None, :, :r] @ to_np64(u)[:, :, :r].transpose(0, 2, 1)
    want = _round(0.125 * to_np64(gain.view[0, 0])[None, :, None] * acc + to_np64(bias), dtype) + to_np64(res)
    got = to_np64(c)
    assert np.isfinite(got).all()
    assert rel_l2(got, want) < 2 * TOL_GEMM[dtype] and worst(got, want) < WORST[dtype]
    assert gain.inputs_unchanged() == ""
    no_gain = _round(0.125 * acc + to_np64(bias), dtype) + to_np64(res)
    assert rel_l2(got, no_gain) > 0.05


# ---- 4. memory contract ----------------------------------------------------------------------------------------------------------------
def _mask(gd, rows, cols):
    L = gd.layout
    m = torch.zeros(L.numel, dtype=torch.bool)
    idx = L.front + torch.arange(rows)[:, None] * L.ld + torch.arange(cols)[None, :]
    m[idx.flatten()] = True
    return m


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("loop", [0, 1])
def test_low_rank_operands_memory_contract_on_the_256_row_engine(dtype, loop, knobs):
    """Ragged m / n (row clamping of the low-rank tiles), NaN past lr_k, in every row gap and in the guard bands; C starts as the
    sentinel: exactly [m, round_up(n, 4)) is written, the pad column is +0, the inputs are unchanged."""
    _pp(knobs, loop)
    m, n, k, r = 601, 331, 128, 128
    g = torch.Generator().manual_seed(31)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(dtype)    # noqa: E731
    A = Guarded(1, m, k, dtype, DEV, ld=k + 8).set(rnd(m, k))
    B = Guarded(1, n, k, dtype, DEV, ld=k + 8).set(rnd(n, k, sc=0.05))
    LA = Guarded(1, m, r, dtype, DEV, ld=r + 64).set(rnd(m, r))
    LB = Guarded(1, n, r, dtype, DEV, ld=r + 8).set(rnd(n, r, sc=0.05))
    R = Guarded(1, m, n, dtype, DEV, ld=336).set(rnd(m, n))
    bias = rnd(n).to(DEV)
    C = Guarded(1, m, n, dtype, DEV, ld=336, kind="output")
    ops.gemm_nt([dict(a=A.view[0], b=B.view[0], c=C.view[0], bias=bias, residual=R.view[0], m=m, n=n, k=k, lda=A.ld, ldb=B.ld,
                      ldc=C.ld, lr=dict(a=LA.view[0], b=LB.view[0], k=r, lda=LA.ld, ldb=LB.ld))])
    torch.cuda.synchronize()
    assert ops.last_gemm_variant() == "pingpong256", ops.last_gemm_variant()
    acc = to_np64(A.view[0]) @ to_np64(B.view[0]).T + to_np64(LA.view[0]) @ to_np64(LB.view[0]).T + to_np64(bias)
    want = _round(acc, dtype) + to_np64(R.view[0])
    got = to_np64(C.view[0])
    assert np.isfinite(got).all()
    assert rel_l2(got, want) < 2 * TOL_GEMM[dtype]
    n4 = (n + 3) // 4 * 4
    writable = _mask(C, m, n4)
    assert C.untouched(writable) == ""
    assert C.pad_is_zero(writable & ~_mask(C, m, n)) == ""
    for gd in (A, B, LA, LB, R):
        assert gd.inputs_unchanged() == ""


# ---- 5. bit stability ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loop", [0, 1, 2])
def test_fifty_segment_launches_are_bit_identical(loop, knobs):
    """A segment tile read before its DMA landed (the second prologue re-points the ring the first loop just released) shows up as a
    launch that differs from the first."""
    _pp(knobs, loop)
    prob, c, want = _segment_problem(600, 320, 192, 192, torch.bfloat16, seed=11)
    ops.gemm_nt([prob])
    torch.cuda.synchronize()
    assert ops.last_gemm_variant() == "pingpong256"
    first = c.clone()
    assert rel_l2(to_np64(first), want) < 2 * TOL_GEMM[torch.bfloat16]
    for i in range(49):
        c.fill_(float("nan"))
        ops.gemm_nt([prob])
        assert torch.equal(c, first), f"launch {i + 2} differs from the first"


# ---- 6. planner ------------------------------------------------------------------------------------------------------------------------
def _profiled(fn):
    lib = _lib.load()
    lib.aid_profile_begin()
    fn()
    buf = (_lib.AidProfileEntry * 512)()
    n = lib.aid_profile_end(buf, 512)
    return [e.kernel.decode() for e in buf[:n]]


def test_cost_rule_sends_a_long_k_segment_launch_to_ping_pong(knobs):
    """7168 x 1280 x 1280 with a rank-64 segment: 140 tiles of 256 x 256, 22 K tiles — the cost model (GEMM_LR_PP = 2) prefers ping-pong
    with or without the two extra tiles (40 us against 0.95 * 45 us on 256 CUs).  GEMM_LR_PP = 0 and the unset knob keep the launch on
    the lock-step engine (the rule is not the default until its cost runs are recorded); same arithmetic either way."""
    dtype = torch.bfloat16
    m, n, k, r = 7168, 1280, 1280, 64
    g = torch.Generator().manual_seed(61)
    x, w = _t((m, k), dtype, g), _t((n, k), dtype, g, 0.03)
    u, bp = _t((m, r), dtype, g), _t((n, r), dtype, g, 0.03)
    c = torch.full((m, n), float("nan"), dtype=dtype, device=DEV)
    prob = dict(a=x, b=w, c=c, m=m, n=n, k=k, lda=k, ldb=k, ldc=n, lr=dict(a=u, b=bp, k=r, lda=r, ldb=r))
    knobs("GEMM_LR_PP", 2)
    names = _profiled(lambda: ops.gemm_nt([prob]))
    torch.cuda.synchronize()
    assert ops.last_gemm_variant().startswith("pingpong2"), ops.last_gemm_variant()
    assert len(names) == 1 and names[0].split("<")[0] == "aid_gemm_nt_pp_kernel_lr", names
    rows = torch.arange(0, m, 97)
    want = _round(to_np64(x[rows]) @ to_np64(w).T + to_np64(u[rows]) @ to_np64(bp).T, dtype)
    assert rel_l2(to_np64(c[rows]), want) < 2 * TOL_GEMM[dtype]
    assert torch.isfinite(c).all()
    for knob in (0, -1):
        ops.set_tuning("GEMM_LR_PP", knob)
        c2 = torch.full((m, n), float("nan"), dtype=dtype, device=DEV)
        ops.gemm_nt([dict(prob, c=c2)])
        torch.cuda.synchronize()
        assert ops.last_gemm_variant().startswith("lockstep128"), (knob, ops.last_gemm_variant())
        assert rel_l2(to_np64(c), to_np64(c2)) < 2 * TOL_GEMM[dtype]


@pytest.mark.parametrize("tri", [0, 1])
def test_forcing_ping_pong_for_plain_groups_leaves_a_small_segment_launch_on_lock_step(tri, knobs):
    """GEMM_VARIANT = 31 forces plain groups only; at 640 x 320 x 640 (six big tiles) the cost model keeps the segment on lock-step."""
    knobs("GEMM_LR_PP", 2)
    knobs("GEMM_VARIANT", 31)
    knobs("GEMM_TRI", tri)
    knobs("GEMM_LS", 0)
    g = torch.Generator().manual_seed(62)
    dtype, m, n, k, r = torch.float16, 640, 320, 640, 64
    x, w = _t((m, k), dtype, g), _t((n, k), dtype, g, 0.05)
    u, bp = _t((m, r), dtype, g), _t((n, r), dtype, g, 0.05)
    c = torch.empty((m, n), dtype=dtype, device=DEV)
    ops.gemm_nt([dict(a=x, b=w, c=c, m=m, n=n, k=k, lda=k, ldb=k, ldc=n, lr=dict(a=u, b=bp, k=r, lda=r, ldb=r))])
    torch.cuda.synchronize()
    assert ops.last_gemm_variant() == "lockstep128", ops.last_gemm_variant()
    ops.gemm_nt([dict(a=x, b=w, c=c, m=m, n=n, k=k, lda=k, ldb=k, ldc=n)])                 # the same launch without a segment is forced
    torch.cuda.synchronize()
    assert ops.last_gemm_variant().startswith("pingpong2"), ops.last_gemm_variant()


# ---- 7. processor calls ----------------------------------------------------------------------------------------------------------------
def _weights(attn):
    return O.AttnWeights(*(effective_weight_dora(m).numpy() for m in (attn.to_q, attn.to_k, attn.to_v, attn.to_out[0])),
                         to_np64(attn.to_out[0].bias), heads=attn.heads)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["fused_outer", "inner"])
@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("dora", [False, True])
def test_processor_with_rank_64_adapters_on_ping_pong_matches_the_oracle(dtype, kind, cross, dora, knobs):
    """An SDXL-width layer (C = 1280, 20 heads of 64) with rank-64 adapters on all four projections, segments asked onto ping-pong."""
    knobs("GEMM_LR_PP", 1)
    c, heads, cc = 1280, 20, 2048 if cross else None
    torch.manual_seed(70 + cross)
    attn = aid_amd.AttnShim(c, heads, cc, dtype=dtype, device=DEV)
    (wrap_attention_dora if dora else wrap_attention)(attn, {"a": (64, 32.0)}, seed=71)
    for mod in (attn.to_q, attn.to_k, attn.to_v, attn.to_out[0]):
        mod.to(DEV)
    g = torch.Generator().manual_seed(72)
    n, s, l = 3, 384, 77
    x = _t((n, s, c), dtype, g)
    ctx = _t((n, l, cc), dtype, g) if cross else None
    fused = kind.startswith("fused")
    mode = kind.split("_")[-1]
    cls = aid_amd.OuterInterpolatedAttnProcessor if mode == "outer" else aid_amd.InnerInterpolatedAttnProcessor
    proc = cls(size=n, is_fused=fused, alpha=50, beta=50)
    out = []
    names = _profiled(lambda: out.append(proc(attn, x, encoder_hidden_states=ctx)))
    y = out[0]
    assert any(nm.split("<")[0] == "aid_gemm_nt_pp_kernel_lr" for nm in names), names
    fn = O.outer_attention if mode == "outer" else O.inner_attention
    coef = proc.coef.to(dtype).float().numpy()
    ref = fn(to_np64(x), None if ctx is None else to_np64(ctx), _weights(attn), coef, fused)
    assert rel_l2(to_np64(y), ref) < TOL[dtype]
    assert worst(to_np64(y), ref) < WORST[dtype]
