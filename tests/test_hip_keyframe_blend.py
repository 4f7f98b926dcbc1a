"""GPU: aid_processor_kf_blend_fwd (include/aid_hip.h) — a corner-weighted processor call whose corners are recorded key frames.

The M key frames' stores are filled by aid_processor_kf_fwd / aid_processor_kf_q8_fwd RECORD of a plain batch.  The oracle is
tests/blend_ref.py in fp64 over the local frames with the corners' recorded K / V read back from the stores (the RECORD call's own
k / V rounded to storage; q8: q8_ref.dequantise of the store bytes).  Bounds: the project's per-call ones, rel-L2 of the whole output —
f32 1e-5, f16 1e-3, bf16 8e-3 (tests/util.py, tests/test_hip_corners.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import blend_ref as B  # noqa: E402
import q8_ref as Q  # noqa: E402
from aid_amd import _lib, ops  # noqa: E402
from oracle import aid_oracle as O  # noqa: E402
from util import TOL, rel_l2, to_np64  # noqa: E402

DEV = torch.device("cuda:0")
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DTYPES = [F16, BF16, F32]
ids_dt = lambda d: str(d).split(".")[-1]  # noqa: E731
BOUND = {F16: TOL[F16], BF16: TOL[BF16], F32: 1e-5}
MODES = [("outer", True), ("outer", False), ("inner", True), ("inner", False)]
N_STEPS, STEP = 2, 1
HEADS = 2


def _bits(t):
    return t.contiguous().view({F16: torch.int16, BF16: torch.int16, F32: torch.int32}[t.dtype])


class Layer:
    """One self-attention layer and M key frames recorded into native and into q8 stores at step STEP by RECORD calls of one plain
    batch (the key frames at rows 0 .. M - 1 of it)."""

    def __init__(self, s, d, m, dtype, seed=0, heads=HEADS):
        g = torch.Generator().manual_seed(100 * m + s + d + seed)
        c = heads * d
        rnd = lambda *sh, sc=1.0: (torch.randn(*sh, generator=g) * sc).to(dtype).to(DEV)      # noqa: E731
        self.s, self.c, self.heads, self.m, self.dtype, self.g = s, c, heads, m, dtype, g
        self.w = [rnd(c, c, sc=c ** -0.5) for _ in range(4)]
        self.bo = rnd(c, sc=0.1)
        self.keys = rnd(m, s, c)
        self.x = rnd(6, s, c)                                 # local frames: the calls take the first n of them
        self.k_fs, self.vt_fs = ops.endpoint_block_sizes(s, c)
        self.lp = self.vt_fs // c
        self.step = torch.full((1,), STEP, dtype=torch.int32, device=DEV)
        nan = lambda n: torch.full((N_STEPS, n), float("nan"), dtype=dtype, device=DEV)    # noqa: E731
        byt = lambda n: torch.full((N_STEPS, Q.block_bytes(n)), 0xA5, dtype=torch.uint8, device=DEV)    # noqa: E731
        self.native = [(nan(self.k_fs), nan(self.vt_fs)) for _ in range(m)]
        self.q8 = [(byt(self.k_fs), byt(self.vt_fs)) for _ in range(m)]
        self.record()

    def kf(self, storage, mode):
        st = self.q8 if storage == "q8" else self.native
        d = dict(entries=[(k_, v_, i) for i, (k_, v_) in enumerate(st)], step=self.step, mode=mode)
        if storage == "q8":
            d["storage"] = "q8"
        return d

    def record(self, **kw):
        for storage in ("native", "q8"):
            ops.processor_kf_fwd(self.keys, *self.w, self.bo, self.heads, kf=self.kf(storage, "record"), mode="plain", **kw)
        torch.cuda.synchronize()
        self.snap = [t.clone() for st in (self.native, self.q8) for pair in st for t in pair]

    def stores_unchanged(self):
        now = [t for st in (self.native, self.q8) for pair in st for t in pair]
        return all(torch.equal(_bits(a) if a.dtype != torch.uint8 else a, _bits(b) if b.dtype != torch.uint8 else b)
                   for a, b in zip(now, self.snap))

    def recorded(self, storage):
        """fp64 (k [M, S, C], v [M, S, C]): what the stores hold at STEP."""
        s, c, lp = self.s, self.c, self.lp
        ks, vs = [], []
        for i in range(self.m):
            if storage == "q8":
                k = Q.dequantise(self.q8[i][0][STEP].cpu().numpy(), self.k_fs).astype(np.float64)
                vt = Q.dequantise(self.q8[i][1][STEP].cpu().numpy(), self.vt_fs, lp, s).astype(np.float64)
            else:
                k, vt = to_np64(self.native[i][0][STEP]), to_np64(self.native[i][1][STEP])
            ks.append(k.reshape(s, c))
            vs.append(vt.reshape(c, lp)[:, :s].T)
        return np.stack(ks), np.stack(vs)

    def weights(self, n_local, n_plain):
        """[n_local + n_plain, M]: a generic row; with three local frames also the one-hot row of the last corner and a row whose first
        pair is zero (M > 2; else another generic one).  The riders' rows are NaN: never read."""
        m, g = self.m, self.g
        gen = lambda: (lambda t: t / t.sum())(torch.rand(m, generator=g) + 0.05)     # noqa: E731
        rows = [gen()]
        if n_local == 3:
            hot = torch.zeros(m)
            hot[m - 1] = 1.0
            z = gen()
            if m > 2:
                z[:2] = 0.0
                z = z / z.sum()
            rows += [hot, z]
        return torch.cat([torch.stack(rows).float(), torch.full((n_plain, m), float("nan"))])

    def blend(self, storage, mode, fused, w, n_plain, **kw):
        n = w.shape[0]
        x = self.x[:n].contiguous()
        return ops.processor_kf_blend_fwd(x, *self.w, self.bo, self.heads, kf=self.kf(storage, "blend"), weights=w.to(DEV), mode=mode,
                                          fused=fused, n_plain=n_plain, **kw).clone()

    def ref(self, storage, mode, fused, w, n_plain, ws=None, **kw):
        n = w.shape[0]
        k_rec, v_rec = self.recorded(storage)
        ws = [to_np64(t) for t in self.w] + [to_np64(self.bo)] if ws is None else ws
        return B.blend_processor(to_np64(self.x[:n]), k_rec, v_rec, *ws, self.heads, mode, fused, w.double().numpy(), n_plain, **kw)


@pytest.mark.parametrize("storage", ["native", "q8"])
@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("s,d", [(64, 64), (76, 40), (76, 64), (64, 40)], ids=lambda v: str(v))
@pytest.mark.parametrize("m", [1, 2, 3, 4, 8])
def test_blend_call_against_the_fp64_reference(m, s, d, dtype, storage):
    L = Layer(s, d, m, dtype)
    for mode, fused in MODES:
        for n_local in (1, 3):
            for n_plain in (0, n_local):
                w = L.weights(n_local, n_plain)
                y = L.blend(storage, mode, fused, w, n_plain)
                got = to_np64(y)
                assert np.isfinite(got).all(), (mode, fused, n_local, n_plain)
                err = rel_l2(got, L.ref(storage, mode, fused, w, n_plain))
                print(f"[blend] m {m} s {s} d {d} {ids_dt(dtype)} {storage} {mode} fused {fused} n {n_local}+{n_plain}: rel-L2 {err:.3e}")
                assert err < BOUND[dtype], (m, s, d, dtype, storage, mode, fused, n_local, n_plain, err)
    assert L.stores_unchanged()


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("mode,fused", MODES, ids=lambda v: str(v))
def test_a_q8_blend_is_the_native_blend_of_the_dequantised_blocks(mode, fused, dtype):
    """Behind the read it is the same code: no tolerance is involved."""
    L = Layer(76, 64, 3, dtype, seed=1)
    for i in range(L.m):                                      # the native stores now hold what GET leaves of the q8 blocks
        k = torch.empty(1, L.s, L.c, dtype=dtype, device=DEV)
        vt = torch.empty(1, L.c, L.lp, dtype=dtype, device=DEV)
        ops.keyframe_rows_q8(k, vt, [(L.q8[i][0], L.q8[i][1], 0)], L.step, "get", vt_cols=L.s)
        L.native[i][0][STEP].copy_(k.reshape(-1))
        L.native[i][1][STEP].copy_(vt.reshape(-1))
    w = L.weights(3, 3)
    assert torch.equal(_bits(L.blend("q8", mode, fused, w, 3)), _bits(L.blend("native", mode, fused, w, 3)))


def test_a_long_call():
    """S = 1024, bf16, d = 64, fused OUTER, M = 3: two passes on whichever kernel the plan picks for a long call."""
    L = Layer(1024, 64, 3, BF16, seed=2)
    w = torch.tensor([[0.2, 0.3, 0.5], [0.0, 0.0, 1.0], [0.6, 0.4, 0.0]])
    y = L.blend("native", "outer", True, w, 0)
    variant = ops.last_attn_variant()
    print(f"[blend-long] aid_last_attn_variant: {variant}")
    assert "aid_attn_pp" in variant, variant                  # the case is about the ping-pong kernel's accumulating pass
    err = rel_l2(to_np64(y), L.ref("native", "outer", True, w, 0))
    print(f"[blend-long] rel-L2 {err:.3e}")
    assert np.isfinite(to_np64(y)).all() and err < BOUND[BF16]


@pytest.mark.parametrize("mode", ["outer", "inner"])
def test_blend_with_unmerged_lora(mode):
    """LoRA rank 64 on q / k / v / out (the packs of tests/test_hip_lora.py), RECORD and blend with the same adapters, against the
    reference on the effective weights."""
    from aid_amd import lora as lora_mod
    from test_hip_lora import _attn, _weights
    dtype, d = F16, 64
    L = Layer(76, d, 3, dtype, seed=3)
    attn = _attn(L.c, HEADS, None, dtype, {"a": (64, 32.0)}, ("to_q", "to_k", "to_v", "to_out"), seed=21)
    base = [m_.base_layer for m_ in (attn.to_q, attn.to_k, attn.to_v, attn.to_out[0])]
    L.w = [b.weight.detach().contiguous() for b in base]
    L.bo = base[3].bias.detach().contiguous()
    la = lora_mod.args(attn, dtype, DEV, cross=False)
    assert la is not None
    L.record(lora=la)
    ew = _weights(attn)
    w = L.weights(3, 3)
    y = L.blend("native", mode, True, w, 3, lora=la)
    err = rel_l2(to_np64(y), L.ref("native", mode, True, w, 3, ws=[ew.wq, ew.wk, ew.wv, ew.wo, ew.bo]))
    print(f"[blend-lora] {mode}: rel-L2 {err:.3e}")
    assert err < BOUND[dtype]


@pytest.mark.parametrize("mode", ["outer", "inner"])
def test_blend_with_folded_layernorm_and_residual(mode):
    """h + attn(LayerNorm(h)) in one call, the LayerNorm folded into the projections (RECORD with the same fold): LayerNorm(x) is
    never rounded to storage, so the per-call bound holds as it stands."""
    dtype = F16
    L = Layer(64, 64, 3, dtype, seed=4)
    c = L.c
    g = torch.Generator().manual_seed(4)
    gamma = (1 + 0.1 * torch.randn(c, generator=g)).to(dtype).to(DEV)
    beta = (0.1 * torch.randn(c, generator=g)).to(dtype).to(DEV)
    const = torch.zeros(6, c, dtype=torch.float32, device=DEV)
    fq, const[0], const[1] = ops.ln_fold(L.w[0], gamma, beta)
    fk, const[2], const[3] = ops.ln_fold(L.w[1], gamma, beta)
    fv, const[4], const[5] = ops.ln_fold(L.w[2], gamma, beta)
    kw = dict(ln=(gamma, beta, 1e-5), ln_folded=(fq, fk, fv, const))
    L.record(**kw)
    w = L.weights(3, 3)
    x = L.x[:6].contiguous()
    y = L.blend("native", mode, True, w, 3, residual=x, **kw)
    x64 = to_np64(x)
    k_rec, v_rec = L.recorded("native")
    ws = [to_np64(t) for t in L.w] + [to_np64(L.bo)]
    ref = B.blend_processor(O.layer_norm(x64, to_np64(gamma), to_np64(beta), 1e-5), k_rec, v_rec, *ws, HEADS, mode, True,
                            w.double().numpy(), 3, residual=x64)
    err = rel_l2(to_np64(y), ref)
    print(f"[blend-ln] {mode}: rel-L2 {err:.3e}")
    assert err < BOUND[dtype]


@pytest.mark.parametrize("mode", ["outer", "inner"])
def test_blend_with_a_score_bias(mode):
    """A non-fused attn_bias ([N * H, 1, L]: diffusers' prepared attention_mask) over the one key segment of a pure call; with `fused`
    it is refused, as today."""
    dtype, s = F16, 76
    L = Layer(s, 64, 3, dtype, seed=5)
    n, riders = 6, 3
    bias = torch.zeros(n * HEADS, 1, s, dtype=dtype, device=DEV)
    bias[:, :, 60:] = -10000.0
    bias[3:5, :, :9] = -10000.0
    w = L.weights(3, riders)
    y = L.blend("native", mode, False, w, riders, attn_bias=bias)
    err = rel_l2(to_np64(y), L.ref("native", mode, False, w, riders, mask=to_np64(bias).reshape(n, HEADS, 1, s)))
    print(f"[blend-bias] {mode}: rel-L2 {err:.3e}")
    assert err < BOUND[dtype]
    with pytest.raises(RuntimeError, match="aid_processor_kf_blend_fwd"):
        L.blend("native", mode, True, w, riders, attn_bias=bias)


@pytest.mark.parametrize("storage", ["native", "q8"])
@pytest.mark.parametrize("mode", ["outer", "inner"])
def test_the_call_stays_inside_its_workspace_and_does_not_read_coef_begin_end(mode, storage):
    """The library call itself with a workspace of exactly the size it asks for between two guard bands, and garbage in
    args->coef / begin / end: the bands and the stores are unchanged and y is the wrapper's y, bit for bit."""
    dtype = BF16
    L = Layer(76, 64, 3, dtype, seed=6)
    w = L.weights(3, 3).to(DEV)
    x = L.x[:6].contiguous()
    want = L.blend(storage, mode, True, w, 3)
    kcall, _rows = ops._keyframe_blend_args(dict(L.kf(storage, "blend"), weights=w), 6, L.s, L.c, dtype)
    a = _lib.AidProcessorArgs()
    a.x, a.y = x.data_ptr(), 0
    a.wq, a.wk, a.wv, a.wo, a.bo = (t.data_ptr() for t in (*L.w, L.bo))
    a.n_frames, a.s, a.l, a.c, a.cc, a.heads, a.n_ctx = 6, L.s, L.s, L.c, L.c, HEADS, 6
    a.mode, a.fused, a.dtype, a.n_plain = _lib.MODE_OUTER if mode == "outer" else _lib.MODE_INNER, 1, _lib.DTYPE_BF16, 3
    a.coef, a.begin, a.end = 0xDEAD0, 1234567, -99
    y = torch.empty_like(x)
    a.y = y.data_ptr()
    lib = _lib.load()
    need = lib.aid_processor_kf_blend_workspace_bytes(C.byref(a), C.byref(kcall))
    assert need > 0
    band = 1 << 20
    buf = torch.full((band + need + band,), 0x5A, dtype=torch.uint8, device=DEV)
    a.workspace, a.workspace_bytes = buf.data_ptr() + band, need
    _lib.check(lib.aid_processor_kf_blend_fwd(C.byref(a), C.byref(kcall), ops._stream()), "aid_processor_kf_blend_fwd")
    torch.cuda.synchronize()
    assert bool((buf[:band] == 0x5A).all()) and bool((buf[band + need:] == 0x5A).all())
    assert torch.equal(_bits(y), _bits(want))
    assert L.stores_unchanged()
    a.workspace_bytes = need - 1
    assert lib.aid_processor_kf_blend_fwd(C.byref(a), C.byref(kcall), ops._stream()) == -4
