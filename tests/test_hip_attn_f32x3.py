"""GPU tests of the float32 attention core at "high" (AidAttnArgs.f32_split = 1 / ops.set_f32_attn_precision("high");
aid_attn_f32x3_kernel in csrc/aid_f32x3.hip): K Q'^T and V^T P^T as three bf16 products of the operands' high / low bf16 halves, the
softmax between them unrounded fp32.

Yardsticks: the fp64 oracle on the same float32 inputs, held to the project's bounds for "high" (TOL_F32_HIGH = 3e-5 rel-L2,
WORST_F32_HIGH = 3e-4 of the RMS, tests/test_hip_f32x3.py; the CPU restatement tests/split_attn_ref.py gives 5.9e-6 - 7.5e-6 and
3.3e-5 - 5.2e-5 at these sizes), and ``ref1`` of that restatement (high halves only: the kernel must be 50x closer to fp64 than that).
Measured on an MI355X: DESIGN.md §3.5b.  The package setting and the torch global are set through fixtures that restore them."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import aid_oracle as O
from split_attn_ref import refs
from util import rel_l2, to_np64, worst

pytestmark = pytest.mark.gpu

import aid_amd  # noqa: E402
from aid_amd import _lib, ops  # noqa: E402
from aid_amd import processors as P  # noqa: E402
from aid_amd.pipelines import DDIMSchedulerLite, InterpolationStableDiffusionPipeline, StackDenoiser  # noqa: E402

DEV = "cuda:0"
F32 = torch.float32
TOL_F32_HIGH = 3e-5
WORST_F32_HIGH = 3e-4
SPLIT, EXACT = "aid_attn_f32x3", "aid_attn_f32"
MODES = [("plain", False), ("inner", False), ("inner", True), ("outer", False), ("outer", True)]     # test_hip_f32.py's


@pytest.fixture
def attn_precision():
    prev = ops.get_f32_attn_precision()
    yield ops.set_f32_attn_precision
    ops.set_f32_attn_precision(prev)


@pytest.fixture
def precision():
    prev = torch.get_float32_matmul_precision()
    yield torch.set_float32_matmul_precision
    torch.set_float32_matmul_precision(prev)


def _close_high(got, ref, what):
    got = to_np64(got) if torch.is_tensor(got) else got
    e, w = rel_l2(got, ref), worst(got, ref)
    print(f"[attn_f32x3] {what}: rel-L2 {e:.2e}  worst {w:.2e}")
    assert np.isfinite(got).all(), what
    assert e < TOL_F32_HIGH and w < WORST_F32_HIGH, (what, e, w)
    return e


def _core_inputs(n, s, l, h, d, seed):
    g = torch.Generator().manual_seed(seed)
    c = h * d
    q, k, v = torch.randn(n, s, c, generator=g), torch.randn(n, l, c, generator=g), torch.randn(n, l, c, generator=g)
    return q, k, v, _vt(v)


def _vt(v):
    n, l, c = v.shape
    vt = torch.zeros(n, c, (l + 7) // 8 * 8)
    vt[:, :, :l] = v.transpose(1, 2)
    return vt


def _coef(n):
    return torch.tensor([0.0, 0.3, 1.0]) if n == 3 else torch.from_numpy(O.beta_coefs(n, 3, 3)).float()


# ragged s and l; one tile and many; l not a multiple of 4 / 8 / 32; the single-key tile
@pytest.mark.parametrize("d", [40, 64, 80, 160])
@pytest.mark.parametrize("shape", [(3, 40, 77, 2), (3, 33, 130, 1), (5, 1, 1, 2), (7, 200, 200, 2)], ids=lambda s: "n%d_s%d_l%d_h%d" % s)
def test_attention_core_high_all_modes(d, shape):
    n, s, l, h = shape
    q, k, v, vt = _core_inputs(n, s, l, h, d, seed=d * 1000 + s)
    coef = _coef(n)
    qd, kd, vd, cd = q.to(DEV), k.to(DEV), vt.to(DEV), coef.to(DEV)
    for mode, fused in MODES:
        o = ops.attn_fwd(qd, kd, vd, h, l=l, mode=mode, fused=fused, coef=cd, f32_attn_precision="high")
        assert ops.last_attn_variant() == SPLIT and o.dtype == F32
        ref = O.attn_core(to_np64(q), to_np64(k), to_np64(v), h, d ** -0.5, mode, fused, coef.numpy().astype(np.float64))
        _close_high(o, ref, (d, shape, mode, fused))


@pytest.mark.parametrize("d", [40, 64, 80, 160])
def test_low_halves_are_really_there(d, attn_precision):
    """50x closer to fp64 than the high halves alone; not the exact kernel's bits; "highest" still names the exact kernel; the
    package setting and the keyword pick the same kernel."""
    n, s, l, h = 3, 40, 77, 2
    q, k, v, vt = _core_inputs(n, s, l, h, d, seed=d)
    _, ref1, ref64 = refs(q, k, v, h)
    qd, kd, vd = q.to(DEV), k.to(DEV), vt.to(DEV)
    o = ops.attn_fwd(qd, kd, vd, h, l=l, f32_attn_precision="high")
    assert ops.last_attn_variant() == SPLIT
    e, e1 = _close_high(o, ref64, (d, "plain vs ref64")), rel_l2(ref1, ref64)
    print(f"[attn_f32x3] d {d}: high halves alone {e1:.2e}")
    assert e < e1 / 50, (e, e1)
    o0 = ops.attn_fwd(qd, kd, vd, h, l=l, f32_attn_precision="highest")
    assert ops.last_attn_variant() == EXACT and not torch.equal(o0, o)
    assert torch.equal(ops.attn_fwd(qd, kd, vd, h, l=l), o0) and ops.last_attn_variant() == EXACT      # the default is exact
    attn_precision("high")
    assert torch.equal(ops.attn_fwd(qd, kd, vd, h, l=l), o) and ops.last_attn_variant() == SPLIT


def test_riders_maps_accumulate_and_late_maximum(attn_precision):
    """test_hip_f32.py's setup under "high": PLAIN riders (negative coefficients), begin / end != (0, N-1), kv_map, frame_scale,
    out_scale, accumulate, and a key in the last tile that raises the running reference (the rescale path)."""
    attn_precision("high")
    n, s, l, h, d = 4, 96, 150, 2, 64
    q, k, v, _ = _core_inputs(2 * n, s, l, h, d, seed=5)
    k[:, 149] = q[:, 7] * 3.0
    vt = _vt(v)
    coef = torch.tensor([0.2, 0.0, 1.0, 0.7, -1.0, -1.0, -1.0, -1.0])
    qd, kd, vd = q.to(DEV), k.to(DEV), vt.to(DEV)
    o = ops.attn_fwd(qd, kd, vd, h, l=l, mode="outer", fused=True, coef=coef.to(DEV), begin=1, end=2, n_plain=n)
    assert ops.last_attn_variant() == SPLIT
    q64, k64, v64 = to_np64(q), to_np64(k), to_np64(v)
    ref = np.concatenate([O.attn_core(q64[:n], k64[:n], v64[:n], h, d ** -0.5, "outer", True, coef[:n].numpy().astype(np.float64), begin=1, end=2),
                          O.attn_core(q64[n:], k64[n:], v64[n:], h, d ** -0.5, "plain", False, None)])
    _close_high(o, ref, "riders")
    o = ops.attn_fwd(qd, kd, vd, h, l=l, mode="inner", fused=True, coef=coef.to(DEV), begin=1, end=2, n_plain=n)
    ref = np.concatenate([O.attn_core(q64[:n], k64[:n], v64[:n], h, d ** -0.5, "inner", True, coef[:n].numpy().astype(np.float64), begin=1, end=2),
                          O.attn_core(q64[n:], k64[n:], v64[n:], h, d ** -0.5, "plain", False, None)])
    _close_high(o, ref, "inner riders")
    kv_map = torch.tensor([2, 0, 0, 1, 5, 4, 7, 6], dtype=torch.int32)
    o2 = ops.attn_fwd(qd, kd, vd, h, l=l, mode="plain", kv_map=kv_map.to(DEV))
    _close_high(o2, O.attn_core(q64, k64[kv_map.numpy()], v64[kv_map.numpy()], h, d ** -0.5, "plain", False, None), "kv_map")
    base = torch.randn(2 * n, s, h * d)
    fs = torch.tensor([0.5, 0.0, 1.0, 2.0, 1.0, 1.0, 0.25, 3.0])
    o3 = base.clone().to(DEV)
    ops.attn_fwd(qd, kd, vd, h, l=l, mode="plain", out=o3, accumulate=True, out_scale=0.6, frame_scale=fs.to(DEV))
    assert ops.last_attn_variant() == SPLIT
    _close_high(o3, to_np64(base) + 0.6 * fs.numpy().reshape(-1, 1, 1) * O.attn_core(q64, k64, v64, h, d ** -0.5, "plain", False, None),
                "accumulate")


@pytest.mark.parametrize("d", [40, 160])
def test_score_bias(d, attn_precision):
    """Each layout of ops.score_bias_layout, additive masks, masks written with -inf / finfo.min, PLAIN and pure OUTER (a rider in it),
    against the oracle with the mask."""
    attn_precision("high")
    n, s, l, h = 4, 70, 150, 2
    q, k, v, vt = _core_inputs(n, s, l, h, d, seed=77 + d)
    g = torch.Generator().manual_seed(d)
    coef = torch.tensor([0.0, 0.35, 1.0, -1.0])
    qd, kd, vd = q.to(DEV), k.to(DEV), vt.to(DEV)
    q64, k64, v64 = to_np64(q), to_np64(k), to_np64(v)

    def additive(*shape):
        keep = torch.rand(*shape, generator=g) > 0.4
        keep[..., 0] = True
        return (1.0 - keep.float()) * -10000.0

    def check(m, m64, what):
        o = ops.attn_fwd(qd, kd, vd, h, l=l, bias=m.to(DEV))
        assert ops.last_attn_variant() == SPLIT
        _close_high(o, O.attn_core(q64, k64, v64, h, d ** -0.5, "plain", False, None, mask=m64), (what, "plain"))
        o = ops.attn_fwd(qd, kd, vd, h, l=l, mode="outer", fused=False, coef=coef.to(DEV), begin=0, end=2, n_plain=1, bias=m.to(DEV))
        assert ops.last_attn_variant() == SPLIT
        mm = m64.reshape(n, -1, m64.shape[-2], l)
        ref = np.empty((n, s, h * d))
        ref[:3] = O.attn_core(q64[:3], k64[:3], v64[:3], h, d ** -0.5, "outer", False, coef[:3].numpy().astype(np.float64), mask=mm[:3])
        ref[3:] = O.attn_core(q64[3:], k64[3:], v64[3:], h, d ** -0.5, "plain", False, None, mask=mm[3:])
        _close_high(o, ref, (what, "outer"))
    for shape in ((n * h, 1, l), (n, 1, l), (n, h, s, l), (n, s, l)):
        m = additive(*shape)
        check(m, to_np64(m), shape)
    for low in (float("-inf"), torch.finfo(F32).min):       # such keys weigh exactly 0 (clamped to -1e30 inside the kernel)
        m = additive(n, 1, l)
        m[m < 0] = low
        check(m, np.where(to_np64(m) < 0, -1e30, 0.0), low)


def test_exponent_range(attn_precision):
    """v scaled by 2^30 and by 2^-30 (bf16 halves keep the fp32 exponent: an fp16 split would not), and q scaled so that the scores
    reach +-40 (the split error of a score is relative to |q| |k|; the restatement gives 1.4e-5 / 1.4e-4 here)."""
    attn_precision("high")
    n, s, l, h, d = 3, 40, 77, 2, 64
    q, k, v, vt = _core_inputs(n, s, l, h, d, seed=64)
    coef = _coef(n)
    kd, cd = k.to(DEV), coef.to(DEV)
    ref = O.attn_core(to_np64(q), to_np64(k), to_np64(v), h, d ** -0.5, "outer", True, coef.numpy().astype(np.float64))
    for e in (30, -30):
        o = ops.attn_fwd(q.to(DEV), kd, (vt * 2.0 ** e).to(DEV), h, l=l, mode="outer", fused=True, coef=cd)
        assert ops.last_attn_variant() == SPLIT
        _close_high(to_np64(o) * 2.0 ** -e, ref, f"v x 2^{e}")          # (a power of two: exact in every step)
    q10 = q * 10.0
    sc = np.einsum("nshd,nlhd->nhsl", to_np64(q10).reshape(n, s, h, d), to_np64(k).reshape(n, l, h, d)) * d ** -0.5
    assert sc.max() > 40 and sc.min() < -40
    for mode, fused in (("plain", False), ("outer", True)):
        o = ops.attn_fwd(q10.to(DEV), kd, vt.to(DEV), h, l=l, mode=mode, fused=fused, coef=cd)
        assert ops.last_attn_variant() == SPLIT
        _close_high(o, O.attn_core(to_np64(q10), to_np64(k), to_np64(v), h, d ** -0.5, mode, fused, coef.numpy().astype(np.float64)),
                    f"scores +-40 {mode}")


def test_determinism(attn_precision):
    attn_precision("high")
    n, s, l, h, d = 3, 200, 200, 2, 40
    q, k, v, vt = _core_inputs(n, s, l, h, d, seed=9)
    qd, kd, vd, cd = q.to(DEV), k.to(DEV), vt.to(DEV), _coef(n).to(DEV)
    first = ops.attn_fwd(qd, kd, vd, h, l=l, mode="outer", fused=True, coef=cd).clone()
    assert ops.last_attn_variant() == SPLIT
    for _ in range(19):
        assert torch.equal(ops.attn_fwd(qd, kd, vd, h, l=l, mode="outer", fused=True, coef=cd), first)


@pytest.mark.parametrize("l", [77, 130])
@pytest.mark.parametrize("d", [40, 160])
def test_memory_contract(d, l, monkeypatch):
    """Guarded buffers (tests/guarded.py): NaN around q / k / V^T / the bias and in V^T's pad columns, a sentinel around out, strided
    rows everywhere.  Every mode with a PLAIN rider, kv_map, accumulate with scales, the score bias: fp64 parity at the "high" bounds,
    nothing outside out[:, :s, :c] written, the inputs unchanged (a read outside a row would put NaN into the result)."""
    import test_hip_memory_contracts as M
    from guarded import Guarded

    class SplitArgs(_lib.AidAttnArgs):                       # AttnCall.run fills a fresh AidAttnArgs: this one asks for the split
        def __init__(self):
            super().__init__()
            self.f32_split = 1
    monkeypatch.setattr(_lib, "AidAttnArgs", SplitArgs)

    class Call(M.AttnCall):
        def check(self, name, Og, ref, what):
            assert name == SPLIT, (name, what)
            _close_high(Og.view, ref, (d, l, what))
            M._ok(Og.untouched(Og.layout.region_mask()), *(t.inputs_unchanged() for t in (self.Q, self.K, self.VT)))

    n, h, s = 5, 2, 67
    call = Call(F32, n, s, l, h, d, 4, seed=d * 100 + l)
    coef = [0.0, 0.25, 0.75, 1.0, -1.0]
    k2, vt2 = call.lerp(torch.tensor(coef, dtype=F32, device=DEV), 0, 3)
    for mode, fused in MODES:
        kw = dict(k2=k2, vt2=vt2) if mode == "inner" else {}
        name, Og, ref = call.run(mode, fused, None if mode == "plain" else coef, 0, 3, **kw)
        call.check(name, Og, ref, (mode, fused))
    name, Og, ref = call.run("outer", True, [0.0, 0.5, 0.25, 1.0, 0.75], 0, 3, kv_map=[0, 0, 4, 3, 1])
    call.check(name, Og, ref, "kv_map")
    g = torch.Generator().manual_seed(l)
    base = torch.randn(n, s, call.c, generator=g).to(DEV)
    name, Og, ref = call.run("outer", True, coef, 0, 3, frame_scale=[0.5, 0.0, 1.0, 2.0, 1.5], out_scale=0.6, accumulate=True, base=base)
    call.check(name, Og, ref, "accumulate")
    bias = Guarded(n, s, l, F32, DEV, ld=l + 8).set(torch.randn(n, s, l, generator=g) * 0.5)
    for mode in ("plain", "outer"):
        name, Og, ref = call.run(mode, False, None if mode == "plain" else coef, 0, 3, bias=bias)
        call.check(name, Og, ref, ("bias", mode))
        M._ok(bias.inputs_unchanged())


# ---- processor calls: float32 AttnShim, N = 3 -----------------------------------------------------------------------------------
LAYERS = [(64, 320, 8, None), (64, 320, 8, 768), (16, 1280, 8, 768)]
PMODES = [("plain", False), ("outer", False), ("outer", True), ("inner", False), ("inner", True)]


def _layer(s, c, heads, cc, seed):
    g = torch.Generator().manual_seed(seed)
    attn = aid_amd.AttnShim(c, heads, cc, dtype=F32, device=DEV)
    with torch.no_grad():
        for lin in (attn.to_q, attn.to_k, attn.to_v, attn.to_out[0]):
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) / lin.weight.shape[1] ** 0.5)
        attn.to_out[0].bias.copy_(0.01 * torch.randn(c, generator=g))
    x = torch.randn(3, s, c, generator=g)
    ctx = torch.randn(3, 77, cc, generator=g) if cc else None
    w = O.AttnWeights(*(to_np64(t) for t in (attn.to_q.weight, attn.to_k.weight, attn.to_v.weight, attn.to_out[0].weight,
                                             attn.to_out[0].bias)), heads)
    return attn, x, ctx, w, g


def _proc(mode, fused):
    if mode == "plain":
        return aid_amd.HipAttnProcessor()
    cls = aid_amd.OuterInterpolatedAttnProcessor if mode == "outer" else aid_amd.InnerInterpolatedAttnProcessor
    return cls(t=0.35, is_fused=fused)


def _oracle(mode, fused, x, ctx, w, proc):
    x64, c64 = to_np64(x), None if ctx is None else to_np64(ctx)
    if mode == "plain":
        return O.plain_attention(x64, c64, w)
    coef = proc.coef.numpy().astype(np.float64)
    return (O.outer_attention if mode == "outer" else O.inner_attention)(x64, c64, w, coef, fused)


@pytest.mark.parametrize("layer", LAYERS, ids=lambda l: "s%d_c%d_%s" % (l[0], l[1], "cross" if l[3] else "self"))
def test_processor_calls_vs_oracle(layer, attn_precision, precision):
    """Attention "high" with exact projections, then both "high": against the fp64 oracle; back on "highest" / "highest" the same
    processor object reproduces its first output bit for bit."""
    s, c, heads, cc = layer
    attn, x, ctx, w, _ = _layer(s, c, heads, cc, seed=s + c + (cc or 0))
    xd, cd = x.to(DEV), None if ctx is None else ctx.to(DEV)
    P.clear_text_kv_cache()
    for mode, fused in PMODES:
        proc = _proc(mode, fused)
        first = proc(attn, xd, encoder_hidden_states=cd).clone()
        assert ops.last_attn_variant() == EXACT and ops.last_gemm_variant() == "f32"
        ref = _oracle(mode, fused, x, ctx, w, proc)
        for proj, gemm in (("highest", "f32"), ("high", "f32x3")):
            attn_precision("high")
            precision(proj)
            y = proc(attn, xd, encoder_hidden_states=cd)
            assert ops.last_attn_variant() == SPLIT and ops.last_gemm_variant() == gemm and y.dtype == F32
            _close_high(y, ref, (layer, mode, fused, "projections " + proj))
            assert not torch.equal(y, first)
        attn_precision("highest")
        precision("highest")
        assert torch.equal(proc(attn, xd, encoder_hidden_states=cd), first) and ops.last_attn_variant() == EXACT
    P.clear_text_kv_cache()


def test_ip_adapter_call_vs_oracle(attn_precision, precision):
    """The image branch's launch carries the field too (the last launch of the call names the split kernel)."""
    s, c, heads, cc, tokens = 64, 320, 8, 768, 4
    attn, x, ctx, w, g = _layer(s, c, heads, cc, seed=77)
    ipa = aid_amd.IPAdapterShim(c, cc, num_tokens=tokens, scale=0.7, dtype=F32, device=DEV)
    with torch.no_grad():
        for lin in (ipa.to_k_ip[0], ipa.to_v_ip[0]):
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) / cc ** 0.5)
    ip = torch.randn(3, 1, tokens, cc, generator=g)
    ipw = O.IPWeights(to_np64(ipa.to_k_ip[0].weight), to_np64(ipa.to_v_ip[0].weight), 0.7, tokens)
    proc = aid_amd.HipIPAdapterAttnProcessor.wrap(ipa)
    ref = O.ip_adapter_attention(to_np64(x), to_np64(ctx), to_np64(ip), w, ipw)
    call = lambda: proc(attn, x.to(DEV), encoder_hidden_states=(ctx.to(DEV), [ip.to(DEV)]))      # noqa: E731
    P.clear_text_kv_cache()
    first = call().clone()
    assert ops.last_attn_variant() == EXACT
    for proj in ("highest", "high"):
        attn_precision("high")
        precision(proj)
        y = call()
        assert ops.last_attn_variant() == SPLIT
        _close_high(y, ref, "HipIPAdapterAttnProcessor T=4, projections " + proj)
    attn_precision("highest")
    precision("highest")
    assert torch.equal(call(), first)
    P.clear_text_kv_cache()


def test_interpolate_single_4_steps_graphs_and_switching(attn_precision):
    """The stand-in SD1.5 stack of test_hip_f32x3.py, 4 DDIM steps: under the new setting graph replay == eager bit for bit (the graph
    keys carry the setting: nothing captured under "highest" is replayed), and switching it off again reproduces the original latents
    bit for bit (the old graphs are replayed).  The depth figures are measured, not asserted, here."""
    hip = StackDenoiser("sd15", dtype=F32, device=DEV, scale_down=16, latent_hw=(8, 8), head_div=4)
    g = torch.Generator().manual_seed(20)
    from test_hip_depth_and_pipelines import _embs
    l0, l1 = torch.randn(1, 4, 8, 8, generator=g), torch.randn(1, 4, 8, 8, generator=g)
    es, ee = _embs(g, hip.stack.cross_dim), _embs(g, hip.stack.cross_dim)
    kw = dict(num_inference_steps=4, warmup_ratio=0.5, guidance_scale=5.0, output_type="latent")
    pipe = InterpolationStableDiffusionPipeline(hip, DDIMSchedulerLite())
    pipe.load_aid(t=0.5, is_fused=True, atype="fused_inner")
    run = lambda **o: pipe.interpolate_single(0.35, latent_start=l0, latent_end=l1, embeds_start=es, embeds_end=ee, **kw, **o)["images"].clone()  # noqa: E731
    exact = run(use_graphs=True)
    attn_precision("high")
    out = run(use_graphs=True)
    assert ops.last_attn_variant() == SPLIT
    eager = run(use_graphs=False)
    attn_precision("highest")
    again = run(use_graphs=True)
    assert out.dtype == F32 and out.shape == (3, 4, 8, 8) and torch.isfinite(out).all()
    assert torch.equal(out, eager) and torch.equal(exact, again) and not torch.equal(exact, out)
