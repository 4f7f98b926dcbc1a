"""GPU tests of float32 matmul precision "high" (AidGemmProblem.f32_split = 1; csrc/aid_f32x3.hip): the projection GEMMs of
float32 tensors as three bf16 products of the operands' high / low bf16 halves.

Yardsticks (tests/split_ref.py): ``ref3`` = the three-term value summed in fp64 (only fp32 accumulation order separates the kernel
from it: the project's fp32 GEMM bound TOL_F32 = 1e-5), ``ref64`` = the fp64 product of the float32 inputs (the kernel may not be
further from it than ref3 is, plus that bound), ``ref1`` = one bf16 product (the kernel must be 50x closer to ref64 than that: the
low halves are really in; a missing cross term costs ~1e-3).  Processor calls and the 20-step loop are held against the fp64 oracle
on the same float32 inputs.  The torch global is set through a fixture that restores it."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import aid_oracle as O
from split_ref import refs
from util import rel_l2, to_np64, worst

pytestmark = pytest.mark.gpu

import aid_amd  # noqa: E402
from aid_amd import _lib, ops  # noqa: E402
from aid_amd import processors as P  # noqa: E402
from aid_amd.pipelines import DDIMSchedulerLite, InterpolationStableDiffusionPipeline, StackDenoiser  # noqa: E402

DEV = "cuda:0"
F32 = torch.float32
TOL_F32 = 1e-5             # rel-L2 of two fp32 accumulation orders (tests/test_hip_f32.py)
WORST_F32 = 1e-4
TOL_F32_HIGH = 3e-5        # processor call under "high" vs the fp64 oracle: CPU emulation of the split gives 8.5e-6 - 8.8e-6 for plain
WORST_F32_HIGH = 3e-4      # calls; 3.4x for the interpolated modes and the accumulation order.  Worst element: WORST_F32 / TOL_F32 kept
#                            (measured on an MI355X over every layer and mode below: rel-L2 7.8e-6 - 8.8e-6, worst 3.9e-5 - 5.7e-5)


@pytest.fixture
def precision():
    prev = torch.get_float32_matmul_precision()
    yield torch.set_float32_matmul_precision
    torch.set_float32_matmul_precision(prev)


def _bounds(got, ref3, ref1, ref64, what):
    """The three bounds of a split GEMM result (module docstring); prints the figures first."""
    got = to_np64(got) if torch.is_tensor(got) else got
    assert np.isfinite(got).all(), what
    e3, e64, f3, f1 = rel_l2(got, ref3), rel_l2(got, ref64), rel_l2(ref3, ref64), rel_l2(ref1, ref64)
    print(f"[f32x3] {what}: vs ref3 {e3:.2e}  vs ref64 {e64:.2e}  (ref3 vs ref64 {f3:.2e}, ref1 vs ref64 {f1:.2e})  worst {worst(got, ref3):.2e}")
    assert e3 <= TOL_F32 and worst(got, ref3) < WORST_F32, (what, e3, worst(got, ref3))
    assert e64 <= f3 + TOL_F32, (what, e64, f3)
    assert e64 < f1 / 50, (what, e64, f1)


def _operands(m, n, k, seed, batch=None):
    g = torch.Generator().manual_seed(seed)
    lead = () if batch is None else (batch,)
    return torch.randn(*lead, m, k, generator=g), torch.randn(*lead, n, k, generator=g) / k ** 0.5, g


# (130, 132, 8): one partial K tile; (.., 40): one full tile + a quarter; (.., 72): tiles + tail; (257, 70, 328): many tiles + tail, n % 4 != 0
# (pad columns, scalar epilogue); (64, 320, 320): a projection shape; (4096, 2048, 64): 512 tiles of 128 x 128 = the large-tile rule
SHAPES = [(130, 132, 8), (130, 132, 40), (130, 132, 72), (257, 70, 328), (64, 320, 320), (4096, 2048, 64)]


@pytest.mark.parametrize("mnk", SHAPES, ids=lambda s: "m%d_n%d_k%d" % s)
def test_gemm_split_shapes(mnk):
    """Every shape bare (the 16-byte store path where n % 4 == 0) and with scale + bias + residual."""
    m, n, k = mnk
    a, b, g = _operands(m, n, k, seed=m * 7 + n * 3 + k)
    bias, res = torch.randn(n, generator=g), torch.randn(m, n, generator=g)
    ref3, ref1, ref64 = refs(a, b)
    ad, bd = a.to(DEV), b.to(DEV)
    ldc = (n + 3) // 4 * 4
    y = torch.full((m, ldc), float("nan"), device=DEV)
    ops.gemm_nt([dict(a=ad, b=bd, c=y, m=m, n=n, k=k, lda=k, ldb=k, ldc=ldc, f32_precision="high")])
    assert ops.last_gemm_variant() == "f32x3"
    _bounds(y[:, :n], ref3, ref1, ref64, f"{mnk} bare")
    assert float(y[:, n:].abs().max() if ldc > n else 0.0) == 0.0            # columns [n, round_up(n, 4)) are written with zeros
    y2 = torch.full((m, ldc), float("nan"), device=DEV)
    resd = torch.zeros(m, ldc)
    resd[:, :n] = res
    ops.gemm_nt([dict(a=ad, b=bd, c=y2, bias=bias.to(DEV), residual=resd.to(DEV), m=m, n=n, k=k, lda=k, ldb=k, ldc=ldc, scale=0.5,
                      f32_precision="high")])
    assert ops.last_gemm_variant() == "f32x3"
    full = lambda r: 0.5 * r + to_np64(bias) + to_np64(res)      # noqa: E731
    _bounds(y2[:, :n], full(ref3), full(ref1), full(ref64), f"{mnk} scale/bias/residual")


@pytest.fixture(scope="module")
def small():
    """(130, 132, 72) operands and their references, shared by the single-option cases."""
    a, b, g = _operands(130, 132, 72, seed=72)
    return a, b, torch.randn(132, generator=g), torch.randn(130, 132, generator=g), refs(a, b)


@pytest.mark.parametrize("opt", ["scale", "bias", "residual"])
def test_gemm_split_single_options(small, opt):
    a, b, bias, res, (ref3, ref1, ref64) = small
    m, n, k = 130, 132, 72
    kw = dict(scale=dict(scale=-0.75), bias=dict(bias=bias.to(DEV)), residual=dict(residual=res.to(DEV)))[opt]
    f = dict(scale=lambda r: -0.75 * r, bias=lambda r: r + to_np64(bias), residual=lambda r: r + to_np64(res))[opt]
    y = torch.full((m, n), float("nan"), device=DEV)
    ops.gemm_nt([dict(a=a.to(DEV), b=b.to(DEV), c=y, m=m, n=n, k=k, lda=k, ldb=k, ldc=n, f32_precision="high", **kw)])
    assert ops.last_gemm_variant() == "f32x3"
    _bounds(y, f(ref3), f(ref1), f(ref64), opt)


def test_gemm_split_batched_with_strides_and_residual():
    batch, m, n, k = 3, 130, 70, 72
    a, b, g = _operands(m, n, k, seed=5, batch=batch)
    res = torch.randn(batch, m, n, generator=g)
    ref3, ref1, ref64 = refs(a, b)
    lda, ldb, ldc = k + 8, k + 16, 76                         # padded rows and frame gaps: the strides are really used
    A = torch.full((batch, m + 2, lda), float("nan"))
    B = torch.full((batch, n + 3, ldb), float("nan"))
    A[:, :m, :k], B[:, :n, :k] = a, b
    R = torch.zeros(batch, m + 1, ldc)
    R[:, :m, :n] = res
    Y = torch.full((batch, m + 1, ldc), float("nan"), device=DEV)
    ops.gemm_nt([dict(a=A.to(DEV), b=B.to(DEV), c=Y, residual=R.to(DEV), m=m, n=n, k=k, lda=lda, ldb=ldb, ldc=ldc, batch=batch,
                      stride_a=(m + 2) * lda, stride_b=(n + 3) * ldb, stride_c=(m + 1) * ldc, f32_precision="high")])
    assert ops.last_gemm_variant() == "f32x3"
    _bounds(Y[:, :m, :n], ref3 + to_np64(res), ref1 + to_np64(res), ref64 + to_np64(res), "batch 3")
    assert float(Y[:, :m, n:72].abs().max()) == 0.0 and bool(torch.isnan(Y[:, :m, 72:]).all()) and bool(torch.isnan(Y[:, m:]).all())


def test_gemm_split_transposed_per_frame_and_grouped():
    """trans_rows = 16 with m = 48 (three frames), and a grouped launch of three problems with K = 320, 320 and 768."""
    m, n, k, tr = 48, 70, 40, 16
    a, b, _ = _operands(m, n, k, seed=6)
    ref3, ref1, ref64 = refs(a, b)
    vt = torch.full((m // tr, n, 24), float("nan"), device=DEV)
    ops.gemm_nt([dict(a=a.to(DEV), b=b.to(DEV), c=vt, m=m, n=n, k=k, lda=k, ldb=k, ldc=24, stride_c=n * 24, trans_rows=tr,
                      f32_precision="high")])
    assert ops.last_gemm_variant() == "f32x3"
    tp = lambda r: r.reshape(m // tr, tr, n).transpose(0, 2, 1)      # noqa: E731
    _bounds(vt[:, :, :tr], tp(ref3), tp(ref1), tp(ref64), "trans_rows")
    assert bool(torch.isnan(vt[:, :, tr:]).all())
    probs, want = [], []
    for i, (m_, n_, k_) in enumerate([(192, 320, 320), (231, 320, 320), (154, 320, 768)]):
        a, b, _ = _operands(m_, n_, k_, seed=60 + i)
        y = torch.full((m_, n_), float("nan"), device=DEV)
        probs.append(dict(a=a.to(DEV), b=b.to(DEV), c=y, m=m_, n=n_, k=k_, lda=k_, ldb=k_, ldc=n_, f32_precision="high"))
        want.append(refs(a, b))
    ops.gemm_nt(probs)
    assert ops.last_gemm_variant() == "f32x3"
    for i, (p, r) in enumerate(zip(probs, want)):
        _bounds(p["c"], *r, f"grouped problem {i}")


def test_gemm_split_keeps_the_float32_exponent_range():
    """Rows of A scaled by 2^-30 .. 2^+30: bf16 halves carry the exponent (an fp16 split would flush the small rows and overflow the
    large ones).  Every row is held to the bounds on its own scale."""
    m, n, k = 61, 64, 320
    a, b, _ = _operands(m, n, k, seed=8)
    sc = torch.tensor([2.0 ** e for e in range(-30, 31)])
    ref3, ref1, ref64 = refs(a, b)
    y = torch.full((m, n), float("nan"), device=DEV)
    ops.gemm_nt([dict(a=(a * sc[:, None]).to(DEV), b=b.to(DEV), c=y, m=m, n=n, k=k, lda=k, ldb=k, ldc=n, f32_precision="high")])
    assert ops.last_gemm_variant() == "f32x3"
    _bounds(to_np64(y) / to_np64(sc)[:, None], ref3, ref1, ref64, "rows x 2^(-30 .. 30)")      # (powers of two: exact in every step)


def test_gemm_split_is_deterministic_and_differs_from_exact():
    a, b, _ = _operands(257, 320, 328, seed=9)
    ad, bd = a.to(DEV), b.to(DEV)
    run = lambda prec: ops.linear(ad, bd, f32_precision=prec)      # noqa: E731
    y1, y2 = run("high"), run("high")
    assert ops.last_gemm_variant() == "f32x3" and torch.equal(y1, y2)
    y0 = run("highest")
    assert ops.last_gemm_variant() == "f32" and not torch.equal(y0, y1)
    assert torch.equal(run("medium"), y1)


def _int_case(case):
    """(problem without c, C buffer shape, view of the valid C region, expected values) of a case of the test below; operands in -4 .. 4"""
    g = torch.Generator().manual_seed(ord(case))
    ri = lambda *sh: torch.randint(-4, 5, sh, generator=g).float()      # noqa: E731
    prod = lambda a, b: to_np64(a) @ np.swapaxes(to_np64(b), -1, -2)      # noqa: E731  (integers below 2^53: exact)
    if case == "a":                                        # n % 4 == 0, aligned bias and residual: 16-byte stores
        m, n, k = 130, 132, 72
        a, b, bias, res = ri(m, k), ri(n, k), ri(n), ri(m, n)
        return (dict(a=a, b=b, bias=bias, residual=res, m=m, n=n, k=k, lda=k, ldb=k, ldc=n), (m, n), lambda c: c,
                prod(a, b) + to_np64(bias) + to_np64(res))
    if case == "b":                                        # n % 4 != 0: scalar stores, pad columns [70, 72) zero
        m, n, k, ldc = 257, 70, 328, 72
        a, b, bias, res = ri(m, k), ri(n, k), ri(n), torch.zeros(m, ldc)
        res[:, :n] = ri(m, n)
        return (dict(a=a, b=b, bias=bias, residual=res, scale=0.5, m=m, n=n, k=k, lda=k, ldb=k, ldc=ldc), (m, ldc), lambda c: c[:, :n],
                0.5 * prod(a, b) + to_np64(bias) + to_np64(res)[:, :n])
    if case == "c":                                        # batched, padded rows and frame gaps
        bt, m, n, k = 3, 130, 70, 72
        lda, ldb, ldc = k + 8, k + 16, 76
        A, B, R = torch.full((bt, m + 2, lda), float("nan")), torch.full((bt, n + 3, ldb), float("nan")), torch.zeros(bt, m + 1, ldc)
        a, b, res = ri(bt, m, k), ri(bt, n, k), ri(bt, m, n)
        A[:, :m, :k], B[:, :n, :k], R[:, :m, :n] = a, b, res
        return (dict(a=A, b=B, residual=R, m=m, n=n, k=k, lda=lda, ldb=ldb, ldc=ldc, batch=bt, stride_a=(m + 2) * lda,
                     stride_b=(n + 3) * ldb, stride_c=(m + 1) * ldc), (bt, m + 1, ldc), lambda c: c[:, :m, :n], prod(a, b) + to_np64(res))
    if case == "d":                                        # transposed per frame of 16 rows
        m, n, k, tr = 48, 70, 40, 16
        a, b = ri(m, k), ri(n, k)
        return (dict(a=a, b=b, m=m, n=n, k=k, lda=k, ldb=k, ldc=24, stride_c=n * 24, trans_rows=tr), (m // tr, n, 24),
                lambda c: c[:, :, :tr], prod(a, b).reshape(m // tr, tr, n).transpose(0, 2, 1))
    m, n, k = 4096, 2048, 64                               # "e": 512 tiles of 128 x 128, the large-tile rule
    a, b = ri(m, k), ri(n, k)
    return dict(a=a, b=b, m=m, n=n, k=k, lda=k, ldb=k, ldc=n), (m, n), lambda c: c, prod(a, b)


@pytest.mark.parametrize("case", ["a", "b", "c", "d", "e"])
def test_gemm_exact_and_split_agree_bit_for_bit_on_small_integers(case):
    """Where the split loses nothing the two kernels must agree to the bit, through every epilogue path they share
    (csrc/aid_gemm_f32.hpp).  Operands are integers in -4 .. 4: their low bf16 halves are zero, every product and every partial sum is
    an integer of magnitude <= 16 K <= 5248, exact in fp32 in any order; scale 0.5, integer bias and residual keep it exact.  So
    "highest", "high" and the integer product agree exactly, inside C; around it the buffer keeps its NaN and the pad columns are +0."""
    prob, cshape, valid, want = _int_case(case)
    prob = {k_: v.to(DEV) if torch.is_tensor(v) else v for k_, v in prob.items()}
    got = {}
    for prec, variant in (("highest", "f32"), ("high", "f32x3")):
        c = torch.full(cshape, float("nan"), device=DEV)
        ops.gemm_nt([dict(prob, c=c, f32_precision=prec)])
        assert ops.last_gemm_variant() == variant
        got[prec] = c
    assert torch.equal(valid(got["highest"]), valid(got["high"]))
    assert np.array_equal(valid(got["high"]).cpu().numpy(), want.astype(np.float32))
    for c in got.values():                                 # what lies around the valid region: NaN kept, pad columns zero, in both alike
        rest = c.clone()
        valid(rest).fill_(0.0)
        if case in "bc":
            assert float(rest[..., :prob["m"], 70:72].abs().max()) == 0.0
            rest[..., :prob["m"], 70:72] = float("nan")
        assert bool(torch.isnan(rest).sum() == rest.numel() - valid(rest).numel())


def _exact(got, ref64, what):
    got = to_np64(got)
    assert np.isfinite(got).all() and rel_l2(got, ref64) < TOL_F32 and worst(got, ref64) < WORST_F32, (what, rel_l2(got, ref64))


def test_groups_that_may_not_split_run_exact():
    """"May use": a group with one problem that did not ask, with a low-rank segment or with a folded LayerNorm runs the exact kernel
    — never an error, nothing dropped."""
    m, n, k = 130, 128, 128
    a, b, g = _operands(m, n, k, seed=10)
    ad, bd = a.to(DEV), b.to(DEV)
    ref64 = to_np64(a) @ to_np64(b).T
    mk = lambda **kw: dict(a=ad, b=bd, c=torch.full((m, n), float("nan"), device=DEV), m=m, n=n, k=k, lda=k, ldb=k, ldc=n, **kw)      # noqa: E731
    ps = [mk(f32_precision="high"), mk(f32_precision="highest")]
    ops.gemm_nt(ps)
    assert ops.last_gemm_variant() == "f32"
    for p in ps:
        _exact(p["c"], ref64, "mixed group")
    la, lb = torch.randn(m, 64, generator=g), torch.randn(n, 64, generator=g) / 8
    p = mk(f32_precision="high", lr=dict(a=la.to(DEV), b=lb.to(DEV), k=64, lda=64, ldb=64))
    lib = _lib.load()
    lib.aid_profile_begin()
    ops.gemm_nt([p])
    buf = (_lib.AidProfileEntry * 8)()
    assert lib.aid_profile_end(buf, 8) == 1 and buf[0].kernel.decode() == "aid_gemm_f32_kernel_lr"
    assert ops.last_gemm_variant() == "f32"
    _exact(p["c"], ref64 + to_np64(la) @ to_np64(lb).T, "low-rank segment")
    st = torch.stack([torch.randn(m, generator=g) * 0.3, torch.rand(m, generator=g) * 0.4 + 0.8], dim=1)
    cs, sh = torch.randn(n, generator=g), torch.randn(n, generator=g)
    p = mk(f32_precision="high", ln_stats=st.to(DEV), ln_colsum=cs.to(DEV), ln_shift=sh.to(DEV), ln_side=1)
    ops.gemm_nt([p])
    assert ops.last_gemm_variant() == "f32"
    s64 = to_np64(st)
    _exact(p["c"], s64[:, 1:2] * (ref64 - s64[:, 0:1] * to_np64(cs)[None]) + to_np64(sh)[None], "folded LayerNorm")


def test_bad_field_values_are_argument_errors():
    x = torch.zeros(64, 64, device=DEV)
    h = torch.zeros(64, 64, device=DEV, dtype=torch.bfloat16)
    lib = _lib.load()

    def call(t, split, dt):
        p = (_lib.AidGemmProblem * 1)()
        q = p[0]
        q.a = q.b = q.c = t.data_ptr()
        q.m, q.n, q.k, q.lda, q.ldb, q.ldc, q.batch, q.f32_split = 64, 64, 64, 64, 64, 64, 1, split
        return lib.aid_gemm_nt(p, 1, dt, torch.cuda.current_stream().cuda_stream)
    assert call(x, 2, _lib.DTYPE_F32) == -1 and call(x, -1, _lib.DTYPE_F32) == -1
    assert call(h, 1, _lib.DTYPE_BF16) == -1 and call(h, 0, _lib.DTYPE_BF16) == 0
    assert call(x, 1, _lib.DTYPE_F32) == 0 and ops.last_gemm_variant() == "f32x3"
    torch.cuda.synchronize()


MEM_CASES = [dict(m=131, n=77, k=72, bias=True, scale=0.5), dict(m=257, n=70, k=328, residual=True, ldc=76),
             dict(m=77, n=203, k=64, batch=3, shared_b=False, bias=True, residual=True, ldc=204),
             dict(m=3 * 16, n=61, k=40, trans_rows=16, ldc=24), dict(m=4096, n=2046, k=64, bias=True, ldc=2052, gap_rows=0)]


@pytest.mark.parametrize("kw", MEM_CASES, ids=["bias", "res", "batch", "trans", "bigtile"])
def test_gemm_split_memory_contract(kw):
    """Guarded buffers (tests/guarded.py): NaN around every input, a sentinel around C — nothing outside C[:, :round_up(n, 4)] is
    written, the pad columns are +0, inputs are read inside their rows only.  "bigtile": 32 x 16 tiles of 128 x 128, the large-tile
    rule on 256 CUs, with a ragged last column tile."""
    from test_hip_memory_contracts import GemmCase

    class SplitCase(GemmCase):
        def reference(self, b, rows):                    # the three-term value in place of the fp64 product
            bm = self.B.view[b if self.B.view.shape[0] > 1 else 0]
            ref = refs(self.A.view[b][rows], bm)[0]
            if self.scale is not None:
                ref = ref * self.scale
            if self.bias is not None:
                ref = ref + to_np64(self.bias.view[0, 0])[None, :]
            if self.res is not None:
                ref = ref + to_np64(self.res.view[b][rows])
            return ref

    case = SplitCase(torch.float32, seed=12, **kw)
    case.problem["f32_precision"] = "high"
    ops.gemm_nt([case.problem])
    torch.cuda.synchronize()
    assert ops.last_gemm_variant() == "f32x3"
    case.check()


# ---- processor calls: the global, float32 AttnShim, N = 3 ---------------------------------------------------------------------------
LAYERS = [(64, 320, 8, None), (64, 320, 8, 768), (64, 640, 8, None), (16, 1280, 8, 768)]
MODES = [("plain", False), ("outer", False), ("outer", True), ("inner", False), ("inner", True)]


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


def _close_high(got, ref, what):
    got = to_np64(got)
    e, wst = rel_l2(got, ref), worst(got, ref)
    print(f"[f32x3] processor {what}: rel-L2 {e:.2e}  worst {wst:.2e}")
    assert np.isfinite(got).all() and e < TOL_F32_HIGH and wst < WORST_F32_HIGH, (what, e, wst)


@pytest.mark.parametrize("layer", LAYERS, ids=lambda l: "s%d_c%d_%s" % (l[0], l[1], "cross" if l[3] else "self"))
def test_processor_calls_under_high_vs_oracle(layer, precision):
    s, c, heads, cc = layer
    attn, x, ctx, w, _ = _layer(s, c, heads, cc, seed=s + c + (cc or 0))
    xd, cd = x.to(DEV), None if ctx is None else ctx.to(DEV)
    P.clear_text_kv_cache()
    for mode, fused in MODES:
        proc = _proc(mode, fused)
        precision("high")
        y = proc(attn, xd, encoder_hidden_states=cd)
        assert ops.last_gemm_variant() == "f32x3" and y.dtype == F32
        _close_high(y, _oracle(mode, fused, x, ctx, w, proc), (layer, mode, fused))
        precision("highest")
        y0 = proc(attn, xd, encoder_hidden_states=cd)
        assert ops.last_gemm_variant() == "f32" and not torch.equal(y0, y)
    P.clear_text_kv_cache()


def test_ip_adapter_call_under_high_vs_oracle(precision):
    s, c, heads, cc, tokens = 64, 320, 8, 768, 4
    attn, x, ctx, w, g = _layer(s, c, heads, cc, seed=77)
    ipa = aid_amd.IPAdapterShim(c, cc, num_tokens=tokens, scale=0.7, dtype=F32, device=DEV)
    with torch.no_grad():
        for lin in (ipa.to_k_ip[0], ipa.to_v_ip[0]):
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) / cc ** 0.5)
    ip = torch.randn(3, 1, tokens, cc, generator=g)
    ipw = O.IPWeights(to_np64(ipa.to_k_ip[0].weight), to_np64(ipa.to_v_ip[0].weight), 0.7, tokens)
    proc = aid_amd.HipIPAdapterAttnProcessor.wrap(ipa)
    precision("high")
    y = proc(attn, x.to(DEV), encoder_hidden_states=(ctx.to(DEV), [ip.to(DEV)]))
    assert ops.last_gemm_variant() == "f32x3"
    _close_high(y, O.ip_adapter_attention(to_np64(x), to_np64(ctx), to_np64(ip), w, ipw), "HipIPAdapterAttnProcessor T=4")
    P.clear_text_kv_cache()


def test_text_kv_cache_does_not_leak_across_settings(precision):
    """A "highest" call followed by a "high" call on the same context == a fresh "high" call, bit for bit."""
    attn, x, ctx, _, _ = _layer(64, 320, 8, 768, seed=31)
    xd, cd = x.to(DEV), ctx.to(DEV)
    proc = aid_amd.OuterInterpolatedAttnProcessor(t=0.35, is_fused=True)
    P.clear_text_kv_cache()
    precision("highest")
    y_exact = proc(attn, xd, encoder_hidden_states=cd).clone()
    precision("high")
    y_after = proc(attn, xd, encoder_hidden_states=cd).clone()
    P.clear_text_kv_cache()
    y_fresh = proc(attn, xd, encoder_hidden_states=cd).clone()
    assert torch.equal(y_after, y_fresh) and not torch.equal(y_exact, y_after)
    precision("highest")                                  # ... and back: the exact entry is not served the split keys either
    assert torch.equal(proc(attn, xd, encoder_hidden_states=cd), y_exact)
    P.clear_text_kv_cache()


# ---- depth: 20 DDIM steps ------------------------------------------------------------------------------------------------------
# rel-L2 of the final latents against the fp64 oracle loop, measured on an MI355X: HIGH_DEPTH_MEASURED; asserted at 1.3 x (the
# project's convention) and below the north-star target 1e-3.
HIGH_DEPTH_MEASURED = 8.161e-6                 # ("highest" on the same run: 6.98e-7)
HIGH_DEPTH_BOUND = 1.3 * HIGH_DEPTH_MEASURED    # 1.061e-5


def test_interpolate_single_f32_high_20_steps(precision):
    """test_hip_f32.py's 20-step interpolate_single loop (SD1.5 stack, batch 3, float32) under "high": against the fp64 oracle loop;
    graph replay == eager bit for bit; back on "highest" the same pipeline object reproduces its "highest" latents bit for bit."""
    from test_hip_depth_and_pipelines import OracleDenoiser, _embs
    hip = StackDenoiser("sd15", dtype=F32, device=DEV, scale_down=16, latent_hw=(8, 8), head_div=4)
    g = torch.Generator().manual_seed(20)
    l0, l1 = torch.randn(1, 4, 8, 8, generator=g), torch.randn(1, 4, 8, 8, generator=g)
    es, ee = _embs(g, hip.stack.cross_dim), _embs(g, hip.stack.cross_dim)
    kw = dict(num_inference_steps=20, warmup_ratio=0.5, guidance_scale=5.0, output_type="latent")
    pipe = InterpolationStableDiffusionPipeline(hip, DDIMSchedulerLite())
    pipe.load_aid(t=0.5, is_fused=True, atype="fused_inner")
    run = lambda **o: pipe.interpolate_single(0.35, latent_start=l0, latent_end=l1, embeds_start=es, embeds_end=ee, **kw, **o)["images"].clone()  # noqa: E731
    precision("highest")
    exact = run()
    precision("high")
    out = run(use_graphs=True)
    eager = run(use_graphs=False)
    assert ops.last_gemm_variant() == "f32x3"
    precision("highest")
    again = run()
    assert torch.equal(out, eager) and torch.equal(exact, again) and not torch.equal(exact, out)
    ora = InterpolationStableDiffusionPipeline(OracleDenoiser(hip), DDIMSchedulerLite())
    ref = ora.interpolate_single(0.35, latent_start=l0.double(), latent_end=l1.double(), embeds_start=tuple(e.double() for e in es),
                                 embeds_end=tuple(e.double() for e in ee), **kw)["images"].numpy()
    err, err_exact = rel_l2(to_np64(out), ref), rel_l2(to_np64(exact), ref)
    print(f"[f32x3] 20-step latents vs fp64 loop: high {err:.3e}  highest {err_exact:.3e}")
    assert out.dtype == F32 and out.shape == (3, 4, 8, 8) and torch.isfinite(out).all()
    assert err < 1e-3 and err < HIGH_DEPTH_BOUND, err
