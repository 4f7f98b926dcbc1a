"""Memory contracts of every kernel entry point: which bytes a call reads, which it writes, and what it leaves in the padding
include/aid_hip.h promises to fill.

Every tensor lives in a guarded buffer (tests/guarded.py): inputs have NaN in their row gaps, frame gaps, V^T pad columns and guard
bands, so a kernel that reads past the logical tensor into its arithmetic fails the fp64 comparison; outputs are pre-filled with a
non-canonical NaN sentinel, so a store outside the region a call may write — of any value — fails the bit-level check.  Every case
stays inside the documented requirements (k % 8, lda / ldb % 8, ldc % 4, 16-byte base pointers): nothing here expects a fault.

Each engine / kernel variant is forced with the development knobs and the name it reports (``ops.last_gemm_variant()`` /
``ops.last_attn_variant()``) is asserted, so a heuristic change cannot silently drop coverage.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from guarded import Guarded, round_up
from oracle import aid_oracle as O
from replay_rows import attn_ref as _attn_ref
from util import TOL, TOL_GEMM, WORST, rel_l2, to_np64, worst

pytestmark = pytest.mark.gpu

import aid_amd  # noqa: E402
from aid_amd import _lib, ops  # noqa: E402

DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
ids_dt = lambda d: str(d).split(".")[-1]  # noqa: E731
# fp32 storage: fp32 arithmetic on the matrix pipe (tests/test_hip_f32.py uses the same bounds)
TOL_F32 = {"gemm": 1e-5, "attn": 1e-5, "worst": 1e-4}


def _tol_gemm(dtype):
    return (TOL_F32["gemm"], TOL_F32["worst"]) if dtype == torch.float32 else (TOL_GEMM[dtype], WORST[dtype])


def _tol_attn(dtype):
    return (TOL_F32["attn"], TOL_F32["worst"]) if dtype == torch.float32 else (TOL[dtype], WORST[dtype])


def _ok(*msgs):
    bad = [m for m in msgs if m]
    assert not bad, "\n".join(bad)


# ================================================================================================================================
# GEMM: engine x epilogue x layout
# ================================================================================================================================
LS128 = {"GEMM_VARIANT": 7, "GEMM_LS": 0, "GEMM_RS": 0}
LS128X4 = {"GEMM_VARIANT": 7, "GEMM_LS": 1, "GEMM_RS": 0}
PP256 = {"GEMM_VARIANT": 31, "GEMM_TRI": 0, "GEMM_RS": 0}
PP288 = {"GEMM_VARIANT": 31, "GEMM_TRI": 1, "GEMM_RS": 0}
ROWSTAT = {"GEMM_RS": 1, "GEMM_VARIANT": -1}
DEFAULT = {}

# n % 4 = 1, 2, 3 and n % 8 = 4 (the ragged-column chunk of every epilogue), ldc = round_up(n, 4), + 4 (ldc % 8 = 4: the generic
# epilogue on every tile), round_up(n, 8) + 16
N_RAGGED = (77, 130, 203, 204)


def _ldc_choices(n):
    return (round_up(n, 4), round_up(n, 4) + 4, round_up(n, 8) + 16)


class GemmCase:
    """One AidGemmProblem on guarded buffers, with its fp64 reference and its checks."""

    def __init__(self, dtype, *, m, n, k, batch=1, shared_b=True, lda=None, ldb=None, ldc=None, gap_rows=2, bias=False,
                 scale=None, residual=False, ln_side=0, trans_rows=0, seed=0):
        self.dtype, self.m, self.n, self.k, self.batch = dtype, m, n, k, batch
        self.trans_rows, self.ln_side, self.scale = trans_rows, ln_side, scale
        g = torch.Generator().manual_seed(seed)
        lda = k + 8 if lda is None else lda
        ldb = k + 8 if ldb is None else ldb
        ldc = round_up(n, 4) + 4 if ldc is None else ldc
        self.A = Guarded(batch, m, k, dtype, DEV, ld=lda, gap_rows=gap_rows).set(torch.randn(batch, m, k, generator=g))
        nb = 1 if shared_b else batch
        self.B = Guarded(nb, n, k, dtype, DEV, ld=ldb, gap_rows=gap_rows).set(torch.randn(nb, n, k, generator=g) / k ** 0.5)
        if trans_rows:
            frames = m // trans_rows
            self.Cg = Guarded(frames, n, trans_rows, dtype, DEV, ld=ldc, gap_rows=gap_rows, kind="output")
        else:
            self.Cg = Guarded(batch, m, n, dtype, DEV, ld=ldc, gap_rows=gap_rows, kind="output")
        self.inputs = [self.A, self.B]
        p = dict(a=self.A.view, b=self.B.view, c=self.Cg.view, m=m, n=n, k=k, lda=lda, ldb=ldb, ldc=ldc, batch=batch,
                 stride_a=self.A.fs if batch > 1 else 0, stride_b=self.B.fs if (batch > 1 and not shared_b) else 0,
                 stride_c=self.Cg.fs if (batch > 1 or trans_rows) else 0, trans_rows=trans_rows)
        if scale is not None:
            p["scale"] = scale
        self.bias = self.res = None
        if bias:
            self.bias = Guarded(1, 1, n, dtype, DEV).set(torch.randn(n, generator=g))
            self.inputs.append(self.bias)
            p["bias"] = self.bias.view
        if residual:
            self.res = Guarded(batch, m, n, dtype, DEV, ld=ldc, fs=self.Cg.fs).set(torch.randn(batch, m, n, generator=g))
            self.inputs.append(self.res)
            p["residual"] = self.res.view
        if ln_side:
            act_rows = m if ln_side == 1 else n
            w_rows = n if ln_side == 1 else m
            nst = batch if (ln_side == 1 or not shared_b) else 1
            st = torch.stack([torch.randn(nst * act_rows, generator=g) * 0.3,
                              torch.rand(nst * act_rows, generator=g) * 0.4 + 0.8], dim=1)
            self.stats = Guarded(1, nst * act_rows, 2, torch.float32, DEV).set(st)
            self.colsum = Guarded(1, 1, w_rows, torch.float32, DEV).set(torch.randn(w_rows, generator=g))
            self.shift = Guarded(1, 1, w_rows, torch.float32, DEV).set(torch.randn(w_rows, generator=g) * 0.5)
            self.inputs += [self.stats, self.colsum, self.shift]
            p.update(ln_stats=self.stats.view, ln_colsum=self.colsum.view, ln_shift=self.shift.view, ln_side=ln_side,
                     stride_stats=act_rows if nst > 1 else 0)
        self.problem = p

    def reference(self, b, rows):
        """fp64 C[b][rows, :n] (before the transposition of a trans_rows problem)."""
        a = to_np64(self.A.view[b][rows])
        bm = to_np64(self.B.view[b if self.B.view.shape[0] > 1 else 0])
        ref = a @ bm.T
        if self.ln_side:
            st = to_np64(self.stats.view[0])
            cs, sh = to_np64(self.colsum.view[0, 0]), to_np64(self.shift.view[0, 0])
            if self.ln_side == 1:
                s_ = st[b * self.m:(b + 1) * self.m][rows]
                ref = s_[:, 1:2] * (ref - s_[:, 0:1] * cs[None, :]) + sh[None, :]
            else:
                nb = b if self.stats.view.shape[1] > self.n else 0
                s_ = st[nb * self.n:(nb + 1) * self.n]
                ref = s_[None, :, 1] * (ref - s_[None, :, 0] * cs[rows][:, None]) + sh[rows][:, None]
        if self.scale is not None:
            ref = ref * self.scale
        if self.bias is not None:
            ref = ref + to_np64(self.bias.view[0, 0])[None, :]
        if self.res is not None:                                   # added after the rounding (aid_hip.h)
            ref = to_np64(torch.from_numpy(ref).to(self.dtype)) + to_np64(self.res.view[b][rows])
        return ref

    def check(self, rows_of=None):
        dt, m, n = self.dtype, self.m, self.n
        tol, wst = _tol_gemm(dt)
        L = self.Cg.layout
        if self.trans_rows:                                           # no pad: trans_rows % 8 == 0
            got = self.Cg.view.permute(0, 2, 1).reshape(m, n)         # [frame * key, channel]
            rows = torch.arange(m) if rows_of is None else rows_of(m)
            ref, out = self.reference(0, rows), to_np64(got[rows.to(DEV)])
            writable = L.region_mask()
            pad_msg = ""
        else:
            refs, outs = [], []
            for b in range(self.batch):
                rows = torch.arange(m) if rows_of is None else rows_of(m)
                refs.append(self.reference(b, rows))
                outs.append(to_np64(self.Cg.view[b][rows.to(DEV)]))
            ref, out = np.concatenate(refs), np.concatenate(outs)
            pad = L.region_mask(rows=m, c0=n, c1=round_up(n, 4))
            writable = L.region_mask(rows=m) | pad
            pad_msg = self.Cg.pad_is_zero(pad)
        name = ops.last_gemm_variant()
        assert np.isfinite(out).all(), (name, "NaN / Inf in the valid region")
        err, w = rel_l2(out, ref), worst(out, ref)
        assert err < tol and w < wst, (name, err, w)
        _ok(pad_msg, self.Cg.untouched(writable), *(t.inputs_unchanged() for t in self.inputs))


def _run(tuning, knobs, cases, expect):
    for k_, v_ in knobs.items():
        tuning(k_, v_)
    ops.gemm_nt([c.problem for c in cases])
    torch.cuda.synchronize()
    name = ops.last_gemm_variant()
    assert name == expect, (name, expect)
    return name


def _epilogue_matrix(k, m, batch_m):
    """(id, GemmCase kwargs) for one engine: every epilogue option, each at another ragged n / ldc."""
    out = []
    opts = [("bias_scale", dict(m=m, bias=True, scale=0.5)),
            ("residual", dict(m=m, bias=True, residual=True)),
            ("negscale_res", dict(m=m, scale=-0.75, residual=True)),
            ("ln1", dict(m=m, bias=True, scale=1.25, ln_side=1)),
            ("ln2_vt", dict(m=m, ln_side=2, batch=3, shared_b=False)),
            ("batch_shared_b", dict(m=batch_m, batch=3, bias=True)),
            ("batch_strided_b", dict(m=batch_m, batch=3, shared_b=False, residual=True, scale=0.5)),
            ("ln1_batch", dict(m=batch_m, batch=2, ln_side=1, shared_b=False))]
    for i, (nm, kw) in enumerate(opts):
        n = N_RAGGED[i % 4]
        ldc = _ldc_choices(n)[i % 3]
        kw = dict(kw, n=n, k=k, ldc=ldc, seed=1000 + i)
        out.append((f"{nm}-n{n}-ldc{ldc}", kw))
    return out


ENGINES = [("edge", DEFAULT, 72, 131, 45), ("edge", DEFAULT, 136, 259, 130),
           ("lockstep128", LS128, 128, 301, 77), ("lockstep128x4", LS128X4, 192, 301, 77),
           ("pingpong256", PP256, 128, 517, 100), ("pingpong288", PP288, 128, 611, 100)]
GEMM_CASES = [pytest.param(eng, knobs, kw, id=f"{eng}-k{k}-{cid}")
              for eng, knobs, k, m, bm in ENGINES for cid, kw in _epilogue_matrix(k, m, bm)]


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("engine,knobs,kw", GEMM_CASES)
def test_gemm_engine_epilogue_memory_contract(dtype, engine, knobs, kw, tuning):
    """(a) the valid region within TOL_GEMM / WORST of fp64 and finite, (b) columns [n, round_up(n, 4)) exactly +0 in every valid
    row and batch, (c) the sentinel everywhere else in C's buffer, (d) A, B, bias, residual and the LayerNorm constants untouched."""
    case = GemmCase(dtype, **kw)
    _run(tuning, knobs, [case], engine)
    case.check()


def _tile_edge_rows(m):
    return torch.unique(torch.cat([torch.arange(0, m, 997), torch.arange(127, m, 128), torch.arange(128, m, 128),
                                   torch.arange(287, m, 288), torch.arange(288, m, 288), torch.tensor([m - 1])]))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("n,ldc,opts", [(509, 512, dict(bias=True)), (506, 516, dict(residual=True, scale=0.5)),
                                        (508, 528, dict(ln_side=1))], ids=["n509-bias", "n506-res", "n508-ln1"])
def test_gemm_pingpong_tail_tiles_memory_contract(dtype, n, ldc, opts, tuning):
    """258 big tiles on 256 CUs: 256 run as 256 x 256 ping-pong tiles, the last two are cut into eight 128 x 128 tail tiles of the
    same launch — both stores meet the ragged column edge (the tile counts of test_gemm_engine_selection_and_parity)."""
    case = GemmCase(dtype, m=33000, n=n, k=64, ldc=ldc, gap_rows=0, seed=n, **opts)
    _run(tuning, PP256, [case], "pingpong256+tail128")
    case.check(rows_of=_tile_edge_rows)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("tri,expect", [(0, "pingpong256+side128"), (1, "pingpong288+side128")])
def test_gemm_side_tiles_memory_contract(dtype, tri, expect, tuning):
    """Unequal-K group: the query projection (K = 640) on the ping-pong engine, a V^T = Wv E^T problem (K = 768, n = 77 keys, ldc 84)
    and a key projection with a ragged width as 128 x 128 side tiles of the same launch."""
    main = GemmCase(dtype, m=2050, n=638, k=640, ldc=648, bias=True, seed=1)
    vt = GemmCase(dtype, m=640, n=77, k=768, batch=2, shared_b=False, ldc=84, seed=2)
    kk = GemmCase(dtype, m=154, n=203, k=768, ldc=204, seed=3, residual=True)
    _run(tuning, dict(PP256, GEMM_TRI=tri), [main, vt, kk], expect)
    main.check(rows_of=_tile_edge_rows)
    vt.check()
    kk.check()


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("engine,knobs,kw", [
    ("pingpong288", PP288, dict(m=3 * 96, n=200, k=192, trans_rows=96, ldc=104)),
    ("pingpong288", PP288, dict(m=4 * 80, n=77, k=128, trans_rows=80, ldc=96, ln_side=1, scale=0.5)),
    ("rowstat320", ROWSTAT, dict(m=4 * 64, n=96, k=320, lda=320, ldb=320, trans_rows=64, ldc=72)),
    ("lockstep128", LS128, dict(m=3 * 40, n=130, k=64, trans_rows=40, ldc=48))], ids=["pp288", "pp288-ln1", "rowstat320", "lockstep-batched"])
def test_gemm_transposed_output_memory_contract(dtype, engine, knobs, kw, tuning):
    """trans_rows: V^T[frame][channel][key] with ldc > trans_rows and gap rows between the frames: exactly the [n, trans_rows] block
    of every frame is written."""
    case = GemmCase(dtype, seed=7, **kw)
    _run(tuning, knobs, [case], engine)
    case.check()


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("k,n,ldc,opts", [(320, 96, 104, dict(bias=True, scale=0.5)), (640, 160, 168, dict(residual=True)),
                                          (320, 64, 64, dict(bias=True, residual=True))], ids=["rs320-bias", "rs640-res", "rs320-both"])
def test_gemm_rowstat_memory_contract(dtype, k, n, ldc, opts, tuning):
    """Row-stationary engine (n % 32 == 0, dense activation rows: lda = ldb = k) with a strided C and guard bands."""
    m = 512 if k == 640 else 256
    case = GemmCase(dtype, m=m, n=n, k=k, lda=k, ldb=k, ldc=ldc, seed=k + n, **opts)
    _run(tuning, ROWSTAT, [case], f"rowstat{k}")
    case.check()


@pytest.mark.parametrize("kw", [dict(m=131, n=77, k=72, bias=True, scale=0.5), dict(m=300, n=130, k=128, residual=True, ldc=140),
                                dict(m=77, n=203, k=64, batch=3, shared_b=False, bias=True, ldc=204),
                                dict(m=2 * 40, n=61, k=96, trans_rows=40, ldc=48)], ids=["bias", "res", "batch", "trans"])
def test_gemm_f32_memory_contract(kw, tuning):
    case = GemmCase(torch.float32, seed=11, **kw)
    _run(tuning, DEFAULT, [case], "f32")
    case.check()


# ================================================================================================================================
# attention core, aid_lerp_kv
# ================================================================================================================================
class AttnCall:
    """q / k / V^T / out of one aid_attn_fwd call on guarded buffers: ldq, ldk > c, ldvt = round_up(l, 8) + 8 with NaN pad columns,
    a gap row behind every frame, out with row stride ``ldo`` and the sentinel outside [s, c] of every frame.  ``extra_kv``: K / V^T
    hold that many frames more than q (n_kv = n + extra_kv: the replay layout, end-point rows behind the call's own)."""

    def __init__(self, dtype, n, s, l, h, d, ldo_extra, seed, fill="nan", extra_kv=0):
        self.dtype, self.n, self.s, self.l, self.h, self.d = dtype, n, s, l, h, d
        f = self.n_kv = n + extra_kv
        c = self.c = h * d
        g = torch.Generator().manual_seed(seed)
        self.Q = Guarded(n, s, c, dtype, DEV, ld=c + 8, gap_rows=1, fill=fill).set(torch.randn(n, s, c, generator=g))
        self.K = Guarded(f, l, c, dtype, DEV, ld=c + 16, gap_rows=1, fill=fill).set(torch.randn(f, l, c, generator=g))
        v = torch.randn(f, l, c, generator=g)
        self.VT = Guarded(f, c, l, dtype, DEV, ld=round_up(l, 8) + 8, gap_rows=1, fill=fill).set(v.transpose(1, 2))
        self.ldo = c + ldo_extra
        self.q64, self.k64 = to_np64(self.Q.view), to_np64(self.K.view)
        self.v64 = to_np64(self.VT.view).transpose(0, 2, 1)

    def out_buffer(self):
        return Guarded(self.n, self.s, self.c, self.dtype, DEV, ld=self.ldo, gap_rows=1, kind="output")

    def lerp(self, coef_t, begin, end):
        """aid_lerp_kv into guarded k2 / vt2 (same frame strides as k / vt); checks which frames it wrote."""
        lib = _lib.load()
        K2 = Guarded(self.n, self.l, self.c, self.dtype, DEV, ld=self.K.ld, gap_rows=1, kind="output")
        VT2 = Guarded(self.n, self.c, self.l, self.dtype, DEV, ld=self.VT.ld, gap_rows=1, kind="output")
        _lib.check(lib.aid_lerp_kv(self.K.ptr, self.VT.ptr, K2.ptr, VT2.ptr, coef_t.data_ptr(), self.n, begin, end, self.K.fs,
                                   self.VT.fs, ops._dtype_code(self.Q.view), ops._stream()), "aid_lerp_kv")
        torch.cuda.synchronize()
        coef = coef_t.cpu().numpy()
        interior = [i for i in range(self.n) if 0 < coef[i] < 1]
        # the rule of aid_hip.h: every element of an interior frame's stride is written, nothing of any other frame
        for G, rows in ((K2, self.l + 1), (VT2, self.c + 1)):
            _ok(G.untouched(G.layout.region_mask(rows=rows, c1=G.ld, frames=interior)))
        tol = TOL_F32["gemm"] if self.dtype == torch.float32 else TOL_GEMM[self.dtype]
        for i in interior:
            ci = float(coef[i])
            assert rel_l2(to_np64(K2.view[i]), (1 - ci) * self.k64[begin] + ci * self.k64[end]) < tol
            assert rel_l2(to_np64(VT2.view[i]).T, (1 - ci) * self.v64[begin] + ci * self.v64[end]) < tol
        return K2, VT2

    def run(self, mode, fused, coef=None, begin=0, end=-1, kv_map=None, frame_scale=None, out_scale=1.0, accumulate=False,
            base=None, bias=None, k2=None, vt2=None, f32_split=0):
        """One aid_attn_fwd through the C ABI; returns (variant, out Guarded, fp64 expected [n, s, c]).  ``f32_split`` = 1 (float32
        only): permit the three-term bf16 split (AidAttnArgs.f32_split)."""
        n, s, c, l = self.n, self.s, self.c, self.l
        end = end % self.n_kv
        Og = self.out_buffer()
        if accumulate:
            Og.view.copy_(base)
        dev_t = lambda t, dt: None if t is None else torch.as_tensor(t, dtype=dt).to(DEV)  # noqa: E731
        coef_t, fs_t, map_t = dev_t(coef, torch.float32), dev_t(frame_scale, torch.float32), dev_t(kv_map, torch.int32)
        a = _lib.AidAttnArgs()
        a.q, a.k, a.vt, a.out = self.Q.ptr, self.K.ptr, self.VT.ptr, Og.ptr
        a.coef = None if coef_t is None else coef_t.data_ptr()
        a.frame_scale = None if fs_t is None else fs_t.data_ptr()
        a.kv_map = None if map_t is None else map_t.data_ptr()
        if k2 is not None:
            a.k2, a.vt2 = k2.ptr, vt2.ptr
        a.n_frames, a.n_kv, a.s, a.l, a.heads, a.d = n, self.n_kv, s, l, self.h, self.d
        a.ldq, a.ldk, a.ldvt, a.ldo = self.Q.ld, self.K.ld, self.VT.ld, self.ldo
        a.q_fs, a.k_fs, a.vt_fs, a.o_fs = self.Q.fs, self.K.fs, self.VT.fs, Og.fs
        a.mode, a.fused, a.begin, a.end = ops.MODES[mode], int(fused), begin, end
        a.accumulate, a.dtype = int(accumulate), ops._dtype_code(self.Q.view)
        a.softmax_scale, a.out_scale = float(self.d ** -0.5), float(out_scale)
        a.n_plain = 0 if coef is None else int(sum(1 for x in coef if x < 0))
        if f32_split:
            a.f32_split = int(f32_split)
        bias64 = None
        if bias is not None:
            a.bias, a.bias_fs, a.bias_hs, a.bias_rs = bias.ptr, bias.fs, 0, bias.ld
            bias64 = to_np64(bias.view)
        _lib.check(_lib.load().aid_attn_fwd(C.byref(a), ops._stream()), "aid_attn_fwd")
        torch.cuda.synchronize()
        name = ops.last_attn_variant()
        ref = _attn_ref(self.q64, self.k64, self.v64, self.h, mode, fused, coef, begin, end, kv_map, bias64)
        if frame_scale is not None or out_scale != 1.0:
            ref = ref * out_scale * (np.ones(n) if frame_scale is None else np.asarray(frame_scale))[:, None, None]
        if accumulate:
            ref = ref + to_np64(base)
        return name, Og, ref

    def check(self, name, Og, ref, what):
        tol, wst = _tol_attn(self.dtype)
        out = to_np64(Og.view)
        assert np.isfinite(out).all(), (name, what, "NaN / Inf in the output")
        err, w = rel_l2(out, ref), worst(out, ref)
        assert err < tol and w < wst, (name, what, err, w)
        _ok(Og.untouched(Og.layout.region_mask()), *(t.inputs_unchanged() for t in (self.Q, self.K, self.VT)))


# (variant id, fp32 only, head dim, key count, knobs, output row stride - c, kernel family of every call, name some call must carry)
# ldo = c + 4 (ldo % 8 = 4) wherever the variant takes it; the ping-pong and text-key kernels store 16-byte rows (ldo % 8 = 0)
ATTN_VARIANTS = [
    ("nw4", False, 80, 130, {"ATTN_RES": 0, "ATTN_TX": 0, "ATTN_V2": 0, "ATTN_NW": 4, "ATTN_PIPE": 0}, 4, "aid_attn<", ",nw4>"),
    ("nw8", False, 64, 130, {"ATTN_RES": 0, "ATTN_TX": 0, "ATTN_V2": 0, "ATTN_NW": 8}, 4, "aid_attn<", ",nw8>"),
    ("qb2", False, 40, 130, {"ATTN_RES": 0, "ATTN_TX": 0, "ATTN_V2": 0, "ATTN_QB": 2}, 4, "aid_attn<", ",qb2>"),
    ("pipe", False, 40, 200, {"ATTN_RES": 0, "ATTN_TX": 0, "ATTN_V2": 0, "ATTN_NW": 4, "ATTN_QB": 1, "ATTN_PIPE": 1}, 4, "aid_attn<",
     ",pipe>"),                                                                      # (built for d = 40, l >= 192)
    ("res", False, 40, 77, {"ATTN_RES": 1, "ATTN_TX": 0, "ATTN_V2": 0}, 4, "aid_attn<", ",res>"),
    ("pingpong", False, 64, 512, {"ATTN_V2": 1, "ATTN_TX": 0}, 8, "aid_attn_pp<d64", "aid_attn_pp<d64,outer>"),
    ("textkey", False, 64, 77, {"ATTN_TX": -1, "ATTN_V2": -1, "ATTN_RES": -1}, 8, "aid_attn_tx<d64,", "aid_attn_tx<d64,inner>"),
    ("f32", True, 64, 77, {}, 4, "aid_attn_f32", "aid_attn_f32"),
]
ATTN_MODES = [("plain", False), ("inner", True), ("inner", False), ("outer", True), ("outer", False)]


ATTN_PARAMS = [pytest.param(v, dt, id=f"{v[0]}-{ids_dt(dt)}") for v in ATTN_VARIANTS for dt in ([torch.float32] if v[1] else DTYPES)]


@pytest.mark.parametrize("s", [1, 67], ids=lambda s: f"s{s}")
@pytest.mark.parametrize("variant,dtype", ATTN_PARAMS)
def test_attention_variant_memory_contract(variant, dtype, s, tuning):
    """Every attention variant, forced by its knob and asserted by name, on strided q / k / V^T (NaN in every gap and V^T pad column)
    in PLAIN, INNER and OUTER (fused and pure, interpolated keys from aid_lerp_kv in guarded buffers), with a PLAIN rider frame in every
    INNER / OUTER call; then kv_map, accumulate with frame_scale / out_scale, and the score bias (bias_rs > l, NaN in its gap
    columns).  Each call: fp64 parity, a finite result, the sentinel untouched outside [s, c] of every frame, the inputs unchanged."""
    vid, _, d, l, knobs, ldo_extra, family, must_see = variant
    for k_, v_ in knobs.items():
        tuning(k_, v_)
    n, h = 5, 2
    call = AttnCall(dtype, n, s, l, h, d, ldo_extra, seed=d * 100 + l + s)
    coef = [0.0, 0.25, 0.75, 1.0, -1.0]                 # end points, two interior frames, a PLAIN rider (the uncond half of CFG)
    coef_t = torch.tensor(coef, dtype=torch.float32, device=DEV)
    k2, vt2 = call.lerp(coef_t, 0, 3)
    seen = set()
    for mode, fused in ATTN_MODES:
        c_ = None if mode == "plain" else coef
        kw = dict(k2=k2, vt2=vt2) if mode == "inner" else {}
        name, Og, ref = call.run(mode, fused, c_, 0, 3, **kw)
        assert name.startswith(family), (vid, mode, fused, name)
        seen.add(name)
        call.check(name, Og, ref, (mode, fused))
    assert any(must_see in nm for nm in seen), (vid, seen)
    # kv_map (frames share key rows; the end points 0 and 3 stay their own)
    kv_map = [0, 0, 4, 3, 1]
    for mode, fused in (("plain", False), ("outer", True)):
        name, Og, ref = call.run(mode, fused, None if mode == "plain" else [0.0, 0.5, 0.25, 1.0, 0.75], 0, 3, kv_map=kv_map)
        assert name.startswith(family), (vid, "kv_map", name)
        call.check(name, Og, ref, ("kv_map", mode))
    # accumulate onto finite values inside the region (sentinel outside), per-frame and global output scales
    g = torch.Generator().manual_seed(s + l)
    base = torch.randn(n, s, call.c, generator=g).to(dtype).to(DEV)
    name, Og, ref = call.run("outer", True, coef, 0, 3, frame_scale=[0.5, 0.0, 1.0, 2.0, 1.5], out_scale=0.6, accumulate=True,
                             base=base)
    call.check(name, Og, ref, "accumulate")
    name, Og, ref = call.run("inner", True, coef, 0, 3, frame_scale=[1.0, 0.5, 2.0, 0.25, 1.0], out_scale=-0.5, k2=k2, vt2=vt2)
    call.check(name, Og, ref, "frame_scale")
    # additive score bias: one [s, l] mask per frame, rows l + 8 apart (NaN in the gap columns); not with fused
    if vid in ("nw4", "f32"):
        bias = Guarded(n, s, l, dtype, DEV, ld=l + 8).set(torch.randn(n, s, l, generator=g) * 0.5)
        for mode in ("plain", "inner", "outer"):
            kw = dict(k2=k2, vt2=vt2) if mode == "inner" else {}
            name, Og, ref = call.run(mode, False, None if mode == "plain" else coef, 0, 3, bias=bias, **kw)
            assert ("bias" in name) or dtype == torch.float32, name
            call.check(name, Og, ref, ("bias", mode))
            _ok(bias.inputs_unchanged())


@pytest.mark.parametrize("s", [1, 67], ids=lambda s: f"s{s}")
@pytest.mark.parametrize("variant,dtype", ATTN_PARAMS)
def test_attention_variant_replay_rows_memory_contract(variant, dtype, s, tuning):
    """The replay layout of the end-point / key-frame stores on guarded buffers: K / V^T hold two rows more than q (n_kv = n + 2),
    begin = n, end = n + 1, no frame of the batch is an end point; frame 2 has a coefficient of exactly 1 with own keys that are not
    the end row (one-sided), frame 3 rides PLAIN.  aid_lerp_kv writes into guarded k2 / vt2 of n frames: an interpolated row written
    at ``begin`` / ``end`` would land in the guard band, only frames 0 and 1 may be written.  Then the four AID modes: fp64 parity, a
    finite result, the sentinel untouched outside [s, c] of every frame, the inputs unchanged."""
    vid, _, d, l, knobs, ldo_extra, family, _ = variant
    for k_, v_ in knobs.items():
        tuning(k_, v_)
    n, h = 4, 2
    call = AttnCall(dtype, n, s, l, h, d, ldo_extra, seed=d * 100 + l + s + 1, extra_kv=2)
    coef = [0.25, 0.75, 1.0, -1.0]
    k2, vt2 = call.lerp(torch.tensor(coef, dtype=torch.float32, device=DEV), n, n + 1)
    for mode, fused in ATTN_MODES[1:]:
        kw = dict(k2=k2, vt2=vt2) if mode == "inner" else {}
        name, Og, ref = call.run(mode, fused, coef, n, n + 1, **kw)
        assert name.startswith(family), (vid, mode, fused, name)
        call.check(name, Og, ref, ("replay", mode, fused))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
def test_attention_inputs_poisoned_with_infinity(dtype, tuning):
    """Second pass of the streaming and resident kernels with +Inf (not NaN) in every gap and pad: an Inf that reaches a max or a
    product unmasked shows as NaN / Inf in the output."""
    for knobs, l, d in (({"ATTN_RES": 0, "ATTN_TX": 0, "ATTN_V2": 0}, 130, 64), ({"ATTN_RES": 1, "ATTN_TX": 0, "ATTN_V2": 0}, 77, 80)):
        for k_, v_ in knobs.items():
            tuning(k_, v_)
        call = AttnCall(dtype, 4, 33, l, 2, d, 4, seed=l, fill="inf")
        coef = [0.0, 0.5, 1.0, -1.0]
        k2, vt2 = call.lerp(torch.tensor(coef, device=DEV), 0, 2)
        for mode, fused in ATTN_MODES:
            kw = dict(k2=k2, vt2=vt2) if mode == "inner" else {}
            name, Og, ref = call.run(mode, fused, None if mode == "plain" else coef, 0, 2, **kw)
            call.check(name, Og, ref, (mode, fused, "inf"))


# ================================================================================================================================
# LayerNorm, row statistics, weight folding
# ================================================================================================================================
@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("rows,c", [(1, 8), (7, 24), (33, 320), (77, 648), (5, 1280), (3, 2048)])
def test_layernorm_family_memory_contract(dtype, rows, c):
    """aid_layernorm / aid_ln_stats / aid_ln_fold on contiguous rows between guard bands: parity with fp64, and nothing written
    outside [rows, c] (y, w_folded) / [rows, 2] (stats) / [rows] (colsum, shift)."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(rows * 7 + c)
    dc = ops._dtype_code(torch.empty(0, dtype=dtype))
    X = Guarded(1, rows, c, dtype, DEV).set(torch.randn(rows, c, generator=g) * 2.0 + 0.7)
    gamma = Guarded(1, 1, c, dtype, DEV).set(1.0 + 0.2 * torch.randn(c, generator=g))
    beta = Guarded(1, 1, c, dtype, DEV).set(0.1 * torch.randn(c, generator=g))
    Y = Guarded(1, rows, c, dtype, DEV, kind="output")
    _lib.check(lib.aid_layernorm(X.ptr, gamma.ptr, beta.ptr, Y.ptr, rows, c, 1e-5, dc, ops._stream()), "aid_layernorm")
    ST = Guarded(1, rows, 2, torch.float32, DEV, kind="output")
    _lib.check(lib.aid_ln_stats(X.ptr, ST.ptr, rows, c, 1e-5, dc, ops._stream()), "aid_ln_stats")
    WF = Guarded(1, rows, c, dtype, DEV, kind="output")
    CS = Guarded(1, 1, rows, torch.float32, DEV, kind="output")
    SH = Guarded(1, 1, rows, torch.float32, DEV, kind="output")
    _lib.check(lib.aid_ln_fold(X.ptr, gamma.ptr, beta.ptr, WF.ptr, CS.ptr, SH.ptr, rows, c, dc, ops._stream()), "aid_ln_fold")
    torch.cuda.synchronize()
    x, gm, bt = to_np64(X.view[0]), to_np64(gamma.view[0, 0]), to_np64(beta.view[0, 0])
    ref = O.layer_norm(x, gm, bt, 1e-5)
    assert rel_l2(to_np64(Y.view[0]), ref) < TOL_GEMM[dtype] and worst(to_np64(Y.view[0]), ref) < WORST[dtype]
    mean = x.mean(axis=1)
    rstd = 1.0 / np.sqrt(x.var(axis=1) + 1e-5)
    st = to_np64(ST.view[0])
    assert np.allclose(st[:, 0], mean, rtol=1e-5, atol=1e-5) and np.allclose(st[:, 1], rstd, rtol=1e-4)
    wf = to_np64(WF.view[0])
    assert rel_l2(wf, x * gm[None, :]) < TOL_GEMM[dtype]
    assert np.allclose(to_np64(CS.view[0, 0]), wf.sum(axis=1), rtol=1e-4, atol=1e-3)
    assert np.allclose(to_np64(SH.view[0, 0]), x @ bt, rtol=1e-4, atol=1e-3)
    _ok(*(G.untouched(G.layout.region_mask()) for G in (Y, ST, WF, CS, SH)),
        *(G.inputs_unchanged() for G in (X, gamma, beta)))


# ================================================================================================================================
# processor calls on a poisoned workspace
# ================================================================================================================================
def _poison_workspace(byte):
    """Fill the library workspace of the current stream (ops.workspace: one buffer reused by every call) with ``byte``."""
    ops.workspace(1, torch.device(DEV)).fill_(byte)


def _weights(attn):
    return O.AttnWeights(*(to_np64(t) for t in (attn.to_q.weight, attn.to_k.weight, attn.to_v.weight, attn.to_out[0].weight,
                                                 attn.to_out[0].bias)), heads=attn.heads)


@pytest.mark.parametrize("dtype", DTYPES + [torch.float32], ids=ids_dt)
@pytest.mark.parametrize("cross", [False, True], ids=["self", "cross"])
@pytest.mark.parametrize("s", [1, 75], ids=lambda s: f"s{s}")
def test_processor_output_does_not_depend_on_stale_workspace(dtype, cross, s):
    """The processors reuse one workspace across layers, so stale data is the normal case: after a larger call has left its data
    there, the same call on a workspace of 0xFF bytes (NaN in every dtype) and on one of zeros gives the same bits — finite and
    within TOL of the oracle — for OUTER / INNER, fused and pure."""
    torch.manual_seed(31 + s)
    n, heads, d, l, cc = 5, 2, 64, 77, 96
    c = heads * d
    attn = aid_amd.AttnShim(c, heads, cc if cross else None, dtype=dtype, device=DEV)
    big = torch.randn(n, 4 * s + 256, c, device=DEV).to(dtype)
    x = torch.randn(n, s, c, device=DEV).to(dtype)
    ctx = torch.randn(n, l, cc, device=DEV).to(dtype) if cross else None
    w = _weights(attn)
    xn, cn = to_np64(x), None if ctx is None else to_np64(ctx)
    for cls, fn in ((aid_amd.OuterInterpolatedAttnProcessor, O.outer_attention),
                    (aid_amd.InnerInterpolatedAttnProcessor, O.inner_attention)):
        for fused in (True, False):
            proc = cls(size=n, is_fused=fused, alpha=3, beta=3)
            proc(attn, big, encoder_hidden_states=ctx)                       # leaves stale data of a larger call
            outs = []
            for byte in (0xFF, 0x00):
                _poison_workspace(byte)
                outs.append(proc(attn, x, encoder_hidden_states=ctx).clone())
            assert torch.equal(outs[0], outs[1]), (cls.__name__, fused, "result depends on the workspace contents")
            assert torch.isfinite(outs[0]).all()
            ref = fn(xn, cn, w, proc.coef.to(dtype).float().numpy(), fused)
            assert rel_l2(to_np64(outs[0]), ref) < _tol_attn(dtype)[0], (cls.__name__, fused)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("cross", [False, True], ids=["self", "cross"])
def test_folded_layernorm_sublayer_on_a_poisoned_workspace(dtype, cross):
    """h + attn(LayerNorm(h)) with the LayerNorm folded into the projections (row statistics and V^T live in the workspace)."""
    n, s, heads, d, l, cc = 5, 77, 2, 64, 77, 96
    c = heads * d
    g = torch.Generator().manual_seed(5 + int(cross))
    attn = aid_amd.AttnShim(c, heads, cc if cross else None, dtype=dtype, device=DEV)
    norm = torch.nn.LayerNorm(c, eps=1e-5).to(DEV, dtype)
    with torch.no_grad():
        norm.weight.copy_((1.0 + 0.2 * torch.randn(c, generator=g)).to(dtype))
        norm.bias.copy_((0.1 * torch.randn(c, generator=g)).to(dtype))
    h = (torch.randn(n, s, c, generator=g) * 2.0 + 0.5).to(dtype).to(DEV)
    ctx = torch.randn(n, l, cc, generator=g).to(dtype).to(DEV) if cross else None
    big = (torch.randn(n, 3 * s, c, generator=g)).to(dtype).to(DEV)
    w = _weights(attn)
    hn = O.layer_norm(to_np64(h), to_np64(norm.weight), to_np64(norm.bias), norm.eps)
    for cls, fn in ((aid_amd.OuterInterpolatedAttnProcessor, O.outer_attention),
                    (aid_amd.InnerInterpolatedAttnProcessor, O.inner_attention)):
        proc = cls(size=n, is_fused=True, alpha=3, beta=3)
        proc.fused_sublayer(attn, norm, big, ctx)
        outs = []
        for byte in (0xFF, 0x00):
            _poison_workspace(byte)
            outs.append(proc.fused_sublayer(attn, norm, h, ctx).clone())
        assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0]).all(), cls.__name__
        ref = to_np64(h) + fn(hn, None if ctx is None else to_np64(ctx), w, proc.coef.to(dtype).float().numpy(), True)
        assert rel_l2(to_np64(outs[0]), ref) < TOL[dtype], cls.__name__


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
def test_ip_processors_on_a_poisoned_workspace(dtype):
    """IP-Adapter OUTER / INNER (image keys / values projected into the workspace next to the text ones), ragged s."""
    n, s, heads, d, l, cc, tokens, ip_scale = 3, 45, 2, 64, 77, 96, 4, 0.7
    c = heads * d
    g = torch.Generator().manual_seed(17)
    attn = aid_amd.AttnShim(c, heads, cc, dtype=dtype, device=DEV)
    ipa = aid_amd.IPAdapterShim(c, cc, num_tokens=tokens, scale=ip_scale, dtype=dtype, device=DEV)
    x = torch.randn(n, s, c, generator=g).to(dtype).to(DEV)
    big = torch.randn(n, 4 * s, c, generator=g).to(dtype).to(DEV)
    text = torch.randn(n, l, cc, generator=g).to(dtype).to(DEV)
    ip = torch.randn(n, 1, tokens, cc, generator=g).to(dtype).to(DEV)
    w = _weights(attn)
    ipw = O.IPWeights(to_np64(ipa.to_k_ip[0].weight), to_np64(ipa.to_v_ip[0].weight), ip_scale, tokens)
    for cls, fn in ((aid_amd.OuterInterpolatedIPAttnProcessor, O.outer_ip_attention),
                    (aid_amd.InnerInterpolatedIPAttnProcessor, O.inner_ip_attention)):
        proc = cls(size=n, is_fused=True, alpha=3, beta=3, ip_attn=ipa)
        proc(attn, big, encoder_hidden_states=(text, [ip]))
        outs = []
        for byte in (0xFF, 0x00):
            _poison_workspace(byte)
            outs.append(proc(attn, x, encoder_hidden_states=(text, [ip])).clone())
        assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0]).all(), cls.__name__
        ref = fn(to_np64(x), to_np64(text), to_np64(ip), w, ipw, proc.coef.to(dtype).float().numpy(), True)
        assert rel_l2(to_np64(outs[0]), ref) < TOL[dtype], cls.__name__
