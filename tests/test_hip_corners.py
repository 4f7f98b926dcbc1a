"""GPU: corner-weighted AID (include/aid_hip.h) — the mix kernel, the attention core among up to eight corners, the processor call and
a captured graph, against the fp64 reference of tests/corners_ref.py evaluated on the inputs as rounded to the storage dtype.

Bounds.  Mix kernel: one unit in the last place of the storage type at the magnitude of the frame's largest fp64 result (fp32 products
and sum of <= 8 terms, one rounding; f32 storage carries the rounding errors along).  Core and processor: the project's per-call
bounds, rel-L2 of the whole output — fp32 1e-5, fp16 1e-3, bf16 8e-3 (tests/util.py, tests/test_hip_f32.py).  Every accumulating pass of
OUTER rounds ``out`` once more in 16-bit storage; the measured figures (printed per case, largest per dtype and pass count at the end
of the module) stand in DESIGN.md §3.6f.

Six AID frames cannot hold the one-hot rows of more than four corners next to a generic row and a row whose first pair is zero, so
every core case runs ceil(M / 4) calls on the same inputs: each has the one-hot rows of four of the corners, the generic row and the
zero-pair row; together they hold every corner's."""
import ctypes as C

import numpy as np
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

import aid_amd  # noqa: E402
import corners_ref as R  # noqa: E402
from aid_amd import _lib, ops  # noqa: E402
from guarded import SENTINEL_BITS, Guarded, _signed  # noqa: E402
from oracle import aid_oracle as O  # noqa: E402
from util import TOL, rel_l2, to_np64  # noqa: E402

DEV = torch.device("cuda:0")
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DTYPES = [F16, BF16, F32]
ids_dt = lambda d: str(d).split(".")[-1]  # noqa: E731
BOUND = {F16: TOL[F16], BF16: TOL[BF16], F32: 1e-5}
FIGURES = {}                                  # (what, dtype, passes) -> largest rel-L2


def _note(what, dtype, passes, err):
    key = (what, ids_dt(dtype), passes)
    FIGURES[key] = max(FIGURES.get(key, 0.0), err)


@pytest.fixture(scope="module", autouse=True)
def _print_figures():
    yield
    for (what, dt, passes), e in sorted(FIGURES.items()):
        print(f"[corners-figures] {what:10s} {dt:9s} passes {passes}  rel-L2 {e:.2e}")


def _ulp_at(x, dtype):
    """One unit in the last place of ``dtype`` at magnitude ``x`` (normal range)."""
    bits = {F16: 10, BF16: 7, F32: 23}[dtype]
    return 2.0 ** (np.floor(np.log2(x)) - bits)


def _weight_rows(m, hot, g, n_aid=6):
    """[n_aid, m]: the one-hot rows of corners ``hot``, a generic row, a row whose first pair is all zero, generic rows up to n_aid."""
    rows = []
    for c in hot:
        r = torch.zeros(m)
        r[c] = 1.0
        rows.append(r)
    generic = torch.rand(m, generator=g) + 0.05
    rows.append(generic / generic.sum())
    z = torch.rand(m, generator=g) + 0.05
    z[:2] = 0.0
    rows.append(z / z.sum() if m > 2 else torch.zeros(m))
    while len(rows) < n_aid:
        x = torch.rand(m, generator=g) + 0.05
        rows.append(x / x.sum())
    assert len(rows) == n_aid
    return torch.stack(rows).to(torch.float32)


# ================================================================================================================================
# aid_mix_kv
# ================================================================================================================================
MIX_ROWS = [4, 0, 8, 2, 2, 7, 1, 5]          # corner rows of a 9-row k / vt (a duplicate among them)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("m", [1, 2, 3, 8])
def test_mix_kv(m, dtype):
    g = torch.Generator().manual_seed(40 + m)
    l, c, f, n, riders = 72, 80, 9, 7, 2
    k = torch.randn(f, l, c, generator=g).to(dtype).to(DEV)
    vt = torch.randn(f, c, l, generator=g).to(dtype).to(DEV)
    w = torch.cat([_weight_rows(m, [m - 1], g, n_aid=n - riders), torch.full((riders, m), float("nan"))])
    rows = MIX_ROWS[:m]
    k2 = torch.full((n, l, c), 123.0, dtype=dtype, device=DEV)
    vt2 = torch.full((n, c, l), 123.0, dtype=dtype, device=DEV)
    ops.mix_kv(k, vt, w.to(DEV), rows, n_plain=riders, out=(k2, vt2))
    torch.cuda.synchronize()
    assert torch.equal(k2[0], k[rows[m - 1]]) and torch.equal(vt2[0], vt[rows[m - 1]])           # one-hot: the corner's bits
    assert bool((k2[n - riders:] == 123.0).all()) and bool((vt2[n - riders:] == 123.0).all())   # riders keep the sentinel
    if m <= 2:
        assert not k2[2].any() and not vt2[2].any()                                               # every weight zero: +0
    for src, dst in ((k, k2), (vt, vt2)):
        ref = R.mix_rows(to_np64(src), rows, w[:n - riders].double().numpy())
        got = to_np64(dst[:n - riders])
        assert np.isfinite(got).all()
        for i in range(n - riders):
            mx = np.abs(ref[i]).max()
            if mx == 0:
                continue
            err = np.abs(got[i] - ref[i]).max()
            print(f"[mix] m {m} {ids_dt(dtype)} frame {i}: max abs err {err:.3e}  ulp {_ulp_at(mx, dtype):.3e}")
            assert err <= _ulp_at(mx, dtype), (m, dtype, i, err, _ulp_at(mx, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
def test_mix_kv_memory_contract(dtype):
    """Guarded buffers: NaN in every row gap, frame gap and band of k / vt, the sentinel around k2 / vt2.  The whole stride of a mixed
    frame is written (mixed from whatever lies in the gaps), nothing of a rider frame, nothing outside; the inputs are unchanged."""
    g = torch.Generator().manual_seed(77)
    l, c, f, n, riders, m = 24, 40, 5, 5, 2, 3
    rows = [3, 0, 4]
    K = Guarded(f, l, c, dtype, DEV, ld=c + 8, gap_rows=1).set(torch.randn(f, l, c, generator=g))
    VT = Guarded(f, c, l, dtype, DEV, ld=l + 8, gap_rows=1).set(torch.randn(f, c, l, generator=g))
    K2 = Guarded(n, l, c, dtype, DEV, ld=c + 8, gap_rows=1, kind="output")
    VT2 = Guarded(n, c, l, dtype, DEV, ld=l + 8, gap_rows=1, kind="output")
    w = torch.cat([_weight_rows(m, [1], g, n_aid=n - riders), torch.full((riders, m), float("nan"))]).to(DEV)
    arr = (C.c_int32 * m)(*rows)
    _lib.check(_lib.load().aid_mix_kv(K.ptr, VT.ptr, K2.ptr, VT2.ptr, arr, w.data_ptr(), n, riders, m, K.fs, VT.fs,
                                      ops._dtype_code(K.view), ops._stream()), "aid_mix_kv")
    torch.cuda.synchronize()
    mixed = list(range(n - riders))
    for G, src, nrows in ((K2, K, l + 1), (VT2, VT, c + 1)):
        msg = G.untouched(G.layout.region_mask(rows=nrows, c1=G.ld, frames=mixed))
        assert not msg, msg
        assert not src.inputs_unchanged(), src.inputs_unchanged()
        ref = R.mix_rows(to_np64(src.view), rows, w[:n - riders].double().cpu().numpy())
        got = to_np64(G.view[:n - riders])
        assert np.isfinite(got).all()
        assert np.abs(got - ref).max() <= _ulp_at(np.abs(ref).max(), dtype)
        assert torch.equal(G.view[0], src.view[rows[1]])
        # the gap row and the pad columns of a mixed frame were written — with the NaN mixed from what lies there in k / vt, which is
        # not the sentinel's bit pattern
        gaps = G.layout.region_mask(rows=nrows, c1=G.ld, frames=mixed) & ~G.layout.region_mask(frames=mixed)
        bits = G.bits.cpu()[gaps]
        assert gaps.any() and bool((bits != _signed(SENTINEL_BITS[dtype], dtype)).all())
        assert bool(torch.isnan(G.buf.cpu()[gaps].float()).all())


# ================================================================================================================================
# aid_attn_corners_fwd
# ================================================================================================================================
CORE_ROWS = {False: [0, 1, 5, 3, 7, 2, 6, 4], True: [0, 1, 2, 3, 1, 0, 3, 2]}      # self: rows of 8 frames; cross: rows of 4 contexts
KV_MAP = [0, 1, 2, 3, 1, 1, 0, 2]
MODES = [("outer", True), ("outer", False), ("inner", True), ("inner", False)]


def _core_inputs(dtype, d, cross, seed):
    g = torch.Generator().manual_seed(seed)
    heads, s, n = 2, 72, 8
    l, f = (77, 4) if cross else (72, 8)
    c = heads * d
    lp = (l + 7) // 8 * 8
    q = torch.randn(n, s, c, generator=g).to(dtype)
    k = torch.randn(f, l, c, generator=g).to(dtype)
    v = torch.randn(f, l, c, generator=g).to(dtype)
    vt = torch.zeros(f, c, lp, dtype=dtype)
    vt[:, :, :l] = v.transpose(1, 2)
    return g, heads, l, q, k, v, vt


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("cross", [False, True], ids=["self", "cross"])
@pytest.mark.parametrize("d", [64, 40])
@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 8])
def test_attn_corners(m, d, cross, dtype):
    g, heads, l, q, k, v, vt = _core_inputs(dtype, d, cross, 100 * m + d + int(cross))
    n, riders = 8, 2
    kv_map = KV_MAP if cross else None
    rows = CORE_ROWS[cross][:m]
    qd, kd, vtd = q.to(DEV), k.to(DEV), vt.to(DEV)
    map_d = torch.tensor(KV_MAP, dtype=torch.int32, device=DEV) if cross else None
    q64, k64, v64 = to_np64(q), to_np64(k), to_np64(v)
    for hot in [list(range(m))[i:i + 4] for i in range(0, m, 4)]:
        w = torch.cat([_weight_rows(m, hot, g), torch.full((riders, m), float("nan"))])
        wd = w.to(DEV)
        for mode, fused in MODES:
            out = ops.attn_corners_fwd(qd, kd, vtd, heads, l=l, weights=wd, rows=rows, mode=mode, fused=fused, n_plain=riders,
                                       kv_map=map_d)
            got = to_np64(out)
            assert np.isfinite(got).all(), (m, d, cross, dtype, mode, fused)
            ref = R.corners_core(q64, k64, v64, heads, d ** -0.5, mode, fused, w.double().numpy(), rows, riders, kv_map)
            err = rel_l2(got, ref)
            passes = (m + 1) // 2 if mode == "outer" else 1
            _note("core", dtype, passes, err)
            print(f"[core] m {m} d {d} {'cross' if cross else 'self'} {ids_dt(dtype)} {mode} fused {fused} hot {hot}: rel-L2 {err:.3e}")
            assert err < BOUND[dtype], (m, d, cross, dtype, mode, fused, hot, err)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("mode,fused", MODES, ids=lambda v: str(v))
def test_two_corners_are_the_two_end_point_call(mode, fused, dtype):
    """M = 2 with w = (1 - c, c) against ops.attn_fwd on the same inputs, within the per-call bound."""
    g, heads, l, q, k, v, vt = _core_inputs(dtype, 64, False, 7)
    n, riders = 8, 2
    c = torch.tensor([0.0, 0.25, 0.5, 0.75, 0.9, 1.0])
    coef = torch.cat([c, torch.full((riders,), -1.0)]).to(DEV)
    w = torch.cat([torch.stack([1 - c, c], dim=1), torch.zeros(riders, 2)]).to(DEV)
    qd, kd, vtd = q.to(DEV), k.to(DEV), vt.to(DEV)
    two = ops.attn_fwd(qd, kd, vtd, heads, l=l, mode=mode, fused=fused, coef=coef, begin=0, end=5, n_plain=riders)
    got = ops.attn_corners_fwd(qd, kd, vtd, heads, l=l, weights=w, rows=[0, 5], mode=mode, fused=fused, n_plain=riders)
    err = rel_l2(to_np64(got), to_np64(two))
    print(f"[two-corners] {ids_dt(dtype)} {mode} fused {fused}: rel-L2 {err:.3e}")
    assert err < BOUND[dtype]


def test_attn_corners_long_call():
    """S = L = 1024, one head of 64, three frames, three corners, fused outer, bf16: `accumulate` / `frame_scale` on whichever kernel
    the plan picks for a long call."""
    g = torch.Generator().manual_seed(5)
    s, d, n, m = 1024, 64, 3, 3
    q = torch.randn(n, s, d, generator=g).to(BF16)
    k = torch.randn(n, s, d, generator=g).to(BF16)
    v = torch.randn(n, s, d, generator=g).to(BF16)
    w = torch.tensor([[1.0, 0, 0], [0.2, 0.3, 0.5], [0, 0, 1.0]])
    out = ops.attn_corners_fwd(q.to(DEV), k.to(DEV), v.transpose(1, 2).contiguous().to(DEV), 1, l=s, weights=w.to(DEV),
                               rows=[0, 1, 2], mode="outer", fused=True)
    print(f"[long] aid_last_attn_variant: {ops.last_attn_variant()}")
    ref = R.corners_core(to_np64(q), to_np64(k), to_np64(v), 1, d ** -0.5, "outer", True, w.double().numpy(), [0, 1, 2])
    err = rel_l2(to_np64(out), ref)
    _note("long", BF16, 2, err)
    print(f"[long] rel-L2 {err:.3e}")
    assert np.isfinite(to_np64(out)).all() and err < BOUND[BF16]


# ================================================================================================================================
# aid_processor_corners_fwd
# ================================================================================================================================
def _proc_inputs(dtype, cross, seed, n=8):
    g = torch.Generator().manual_seed(seed)
    c, heads, s, l, cc = 128, 2, 72, 77, 96
    t = lambda *shape, sc=1.0: (torch.randn(*shape, generator=g) * sc).to(dtype).to(DEV)  # noqa: E731
    x = t(n, s, c)
    ctx = t(n, l, cc) if cross else None
    kin = cc if cross else c
    wq, wk, wv, wo, bo = t(c, c, sc=c ** -0.5), t(c, kin, sc=kin ** -0.5), t(c, kin, sc=kin ** -0.5), t(c, c, sc=c ** -0.5), t(c, sc=0.1)
    return g, heads, x, ctx, (wq, wk, wv, wo, bo)


PROC_W = torch.tensor([[1, 0, 0], [0.2, 0.3, 0.5], [0, 1, 0], [0, 0, 1], [0, 0.4, 0.6], [0.5, 0.5, 0]], dtype=torch.float32)
PROC_ROWS = [0, 2, 3]


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("mode", ["outer", "inner"])
@pytest.mark.parametrize("cross", [False, True], ids=["self", "cross"])
def test_processor_corners(cross, mode, dtype):
    g, heads, x, ctx, ws = _proc_inputs(dtype, cross, 30 + int(cross))
    riders = 2
    w = torch.cat([PROC_W, torch.full((riders, 3), float("nan"))])
    y = ops.processor_corners_fwd(x, ctx, *ws, heads, weights=w.to(DEV), rows=PROC_ROWS, mode=mode, fused=True, n_plain=riders)
    ref = R.corners_processor(to_np64(x), None if ctx is None else to_np64(ctx), *(to_np64(t_) for t_ in ws), heads, mode, True,
                              w.double().numpy(), PROC_ROWS, riders)
    err = rel_l2(to_np64(y), ref)
    _note("processor", dtype, 2 if mode == "outer" else 1, err)
    print(f"[processor] {'cross' if cross else 'self'} {mode} {ids_dt(dtype)}: rel-L2 {err:.3e}")
    assert np.isfinite(to_np64(y)).all() and err < BOUND[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
def test_processor_corners_with_a_score_bias(dtype):
    """A non-fused attn_bias (diffusers' prepared attention_mask: [N * H, 1, L]) on a cross-attention call with shared contexts."""
    g, heads, x, ctx, ws = _proc_inputs(dtype, True, 41)
    n, riders, l = 8, 2, 77
    ctx4 = ctx[:4].contiguous()
    ctx_map = torch.tensor(KV_MAP, dtype=torch.int32, device=DEV)
    bias = torch.zeros(n * heads, 1, l, dtype=dtype, device=DEV)
    bias[:, :, 60:] = -10000.0
    bias[3:5, :, :9] = -10000.0
    w = torch.cat([PROC_W, torch.full((riders, 3), float("nan"))])
    for mode in ("outer", "inner"):
        y = ops.processor_corners_fwd(x, ctx4, *ws, heads, weights=w.to(DEV), rows=[0, 3, 1], mode=mode, fused=False, n_plain=riders,
                                      ctx_map=ctx_map, attn_bias=bias)
        ref = R.corners_processor(to_np64(x), to_np64(ctx4), *(to_np64(t_) for t_ in ws), heads, mode, False, w.double().numpy(),
                                  [0, 3, 1], riders, KV_MAP, to_np64(bias).reshape(n, heads, 1, l))
        err = rel_l2(to_np64(y), ref)
        print(f"[processor-bias] {mode} {ids_dt(dtype)}: rel-L2 {err:.3e}")
        assert err < BOUND[dtype]
    with pytest.raises(RuntimeError, match="aid_processor_corners_fwd"):       # a bias with fused is refused, as today
        ops.processor_corners_fwd(x, ctx4, *ws, heads, weights=w.to(DEV), rows=[0, 3, 1], mode="outer", fused=True, n_plain=riders,
                                  ctx_map=ctx_map, attn_bias=bias)


@pytest.mark.parametrize("cross", [False, True], ids=["self", "cross"])
def test_corner_processor_with_unmerged_lora(cross):
    """LoRA rank 64 on q / k / v / out (the packs of tests/test_hip_lora.py) through CornerInterpolatedAttnProcessor, against the
    reference on the effective weights.  Bound: that file's, the per-call bound."""
    from test_hip_lora import _attn, _weights
    dtype, c, heads, cc = F16, 128, 2, 96
    attn = _attn(c, heads, cc if cross else None, dtype, {"a": (64, 32.0)}, ("to_q", "to_k", "to_v", "to_out"), seed=21)
    g = torch.Generator().manual_seed(22)
    x = torch.randn(6, 72, c, generator=g).to(dtype).to(DEV)
    ctx = torch.randn(6, 77, cc, generator=g).to(dtype).to(DEV) if cross else None
    for mode in ("outer", "inner"):
        proc = aid_amd.CornerInterpolatedAttnProcessor(PROC_W, PROC_ROWS, mode=mode, is_fused=True)
        y = proc(attn, x, encoder_hidden_states=ctx)
        ew = _weights(attn)
        ref = R.corners_processor(to_np64(x), None if ctx is None else to_np64(ctx), ew.wq, ew.wk, ew.wv, ew.wo, ew.bo, heads, mode,
                                  True, PROC_W.double().numpy(), PROC_ROWS)
        err = rel_l2(to_np64(y), ref)
        print(f"[processor-lora] {'cross' if cross else 'self'} {mode}: rel-L2 {err:.3e}")
        assert err < TOL[dtype]


@pytest.mark.parametrize("dtype", [F16, BF16], ids=ids_dt)
def test_corner_processor_sublayer_with_residual_and_unfolded_layernorm(dtype):
    """``h + attn(norm(h))`` in one call with the LayerNorm as its own pass (ln without ln_folded) and the residual in the out
    projection's epilogue.  LayerNorm(x) is rounded to the storage type before the projections — one rounding more on the call's
    input than the per-call bound counts — so the bound is twice that, as for the two-end-point sublayer (tests/test_hip_lora.py)."""
    g, heads, x, _, ws = _proc_inputs(dtype, False, 51)
    c = x.shape[2]
    gamma = (1 + 0.1 * torch.randn(c, generator=g)).to(dtype).to(DEV)
    beta = (0.1 * torch.randn(c, generator=g)).to(dtype).to(DEV)
    riders = 2
    w = torch.cat([PROC_W, torch.zeros(riders, 3)])
    for mode in ("outer", "inner"):
        y = ops.processor_corners_fwd(x, None, *ws, heads, weights=w.to(DEV), rows=PROC_ROWS, mode=mode, fused=True, n_plain=riders,
                                      ln=(gamma, beta, 1e-5), residual=x)
        xn = to_np64(x)
        h = torch.from_numpy(O.layer_norm(xn, to_np64(gamma), to_np64(beta), 1e-5)).to(dtype).double().numpy()
        ref = R.corners_processor(h, None, *(to_np64(t_) for t_ in ws), heads, mode, True, w.double().numpy(), PROC_ROWS, riders,
                                  residual=xn)
        err = rel_l2(to_np64(y), ref)
        print(f"[processor-ln] {mode} {ids_dt(dtype)}: rel-L2 {err:.3e}")
        assert err < 2 * TOL[dtype]
    # the processor's sublayer form: the same call through fused_sublayer (folded or not, it computes h + attn(norm(h)))
    attn = aid_amd.AttnShim(c, heads, None, dtype=dtype, device=DEV)
    with torch.no_grad():
        for lin, t_ in zip((attn.to_q, attn.to_k, attn.to_v, attn.to_out[0]), ws[:4]):
            lin.weight.copy_(t_)
        attn.to_out[0].bias.copy_(ws[4])
    norm = nn.LayerNorm(c, dtype=dtype, device=DEV)
    with torch.no_grad():
        norm.weight.copy_(gamma)
        norm.bias.copy_(beta)
    proc = aid_amd.CornerInterpolatedAttnProcessor(PROC_W, PROC_ROWS, mode="outer", is_fused=True)
    proc.plain_tail = riders
    y = proc.fused_sublayer(attn, norm, x)
    xn = to_np64(x)
    ref = R.corners_processor(O.layer_norm(xn, to_np64(gamma), to_np64(beta), 1e-5), None, *(to_np64(t_) for t_ in ws), heads, "outer",
                              True, w.double().numpy(), PROC_ROWS, riders, residual=xn)
    assert rel_l2(to_np64(y), ref) < 2 * TOL[dtype]


# ================================================================================================================================
# a captured graph reads live weights
# ================================================================================================================================
@pytest.mark.parametrize("mode", ["outer", "inner"])
def test_captured_corner_call_reads_live_weights(mode):
    dtype = F16
    g, heads, x, _, ws = _proc_inputs(dtype, False, 61, n=6)
    attn = aid_amd.AttnShim(x.shape[2], heads, None, dtype=dtype, device=DEV)
    with torch.no_grad():
        for lin, t_ in zip((attn.to_q, attn.to_k, attn.to_v, attn.to_out[0]), ws[:4]):
            lin.weight.copy_(t_)
        attn.to_out[0].bias.copy_(ws[4])
    proc = aid_amd.CornerInterpolatedAttnProcessor(PROC_W.clone(), PROC_ROWS, mode=mode, is_fused=True)

    def ref(w):
        return R.corners_processor(to_np64(x), None, *(to_np64(t_) for t_ in ws), heads, mode, True, w.double().numpy(), PROC_ROWS)
    cap = torch.cuda.Stream()
    cap.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cap):                          # eager warm-up on the capture stream: workspace, weight buffer
        proc(attn, x)
    torch.cuda.current_stream().wait_stream(cap)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=cap):             # one stream, no parallel branch
        y = proc(attn, x)
    graph.replay()
    torch.cuda.synchronize()
    assert rel_l2(to_np64(y), ref(PROC_W)) < TOL[dtype]
    first = y.clone()
    new = PROC_W.clone()
    new[1] = torch.tensor([0.6, 0.1, 0.3])
    new[4] = torch.tensor([0.5, 0.0, 0.5])
    ptr = proc._weights_device(DEV, 6).data_ptr()
    proc.weights[1] = new[1]                              # edited in place, outside capture: like `coef`, the edit reaches the device
    proc.weights[4] = new[4]                              # buffer — in place — at the processor's next eager call
    eager = proc(attn, x)
    assert proc._weights_device(DEV, 6).data_ptr() == ptr
    graph.replay()
    torch.cuda.synchronize()
    assert rel_l2(to_np64(y), ref(new)) < TOL[dtype] and torch.equal(y, eager)
    assert not torch.equal(y[1], first[1]) and torch.equal(y[0], first[0])
    assert rel_l2(to_np64(y), ref(PROC_W)) > 10 * TOL[dtype]                  # the first weights no longer describe it
    proc.weights = PROC_W.clone()                         # an assignment rewrites the buffer at once: no call in between
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, first)
    with pytest.raises(RuntimeError, match="stream capture"):                  # a change inside a capture is refused, as for `coef`
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g2, stream=cap):
            proc.weights = new
