"""GPU: every K-loop depth, loop order and low-rank segment depth of the GEMM tile engines (csrc/aid_gemm.hip) and of the float32
GEMMs.

Each engine moves its operands through an LDS-DMA ring that is guarded only by counted waits (``s_waitcnt vmcnt(N)``); the counts
change with the number of K tiles that remain, so a wrong count shows only at the depth where its branch is taken — as wrong numbers,
never as a fault.  ``nk`` = K / 64 is the number of K tiles; the depths where the prologue, the first steady-state trip and the tail
bodies of a loop sit next to each other (nk = 1 .. 6) are walked here for every loop, on the NoLR kernels production runs and behind
/ inside a low-rank segment of every depth up to lr_k = 512.

Three oracles, strongest first:

1. Exact integers.  Operands, low-rank operands and bias are drawn from {-1, 0, 1}, scale = 1: every product and every fp32 partial
   sum is an integer, exact in any order, and the one rounding to fp16 / bf16 is exact while |result| <= 256 (the bf16 limit).  Each
   case asserts that precondition on the float64 reference first and then compares with ``np.array_equal``: a dropped, duplicated,
   stale or misplaced K tile changes an integer, no tolerance is involved.  C starts as NaN, m and n are ragged.
2. Bit-identity between the loop orders GEMM_PP = 0, 1, 2 (the same MFMAs in the same order per accumulator) and between the two
   lock-step rings, on random-normal operands with bias, scale = 0.5 and a residual.
3. fp64 within TOL_GEMM / WORST (tests/util.py) on the same random-normal case.

Every case asserts ``ops.last_gemm_variant()``: a planner change cannot move the sweep to another kernel unnoticed."""
import functools

import numpy as np
import pytest
import torch

from util import TOL_GEMM, WORST, rel_l2, to_np64, worst

pytestmark = pytest.mark.gpu

from aid_amd import ops  # noqa: E402

DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
ids_dt = lambda d: str(d).split(".")[-1]  # noqa: E731
TOL_GEMM32, WORST32 = 1e-5, 1e-4            # float32 storage (tests/test_hip_f32.py, tests/test_hip_dora.py)
EXACT_LIMIT = 256                           # every integer up to here is a bf16 (8 significant bits) and an fp16 number

# knob sets of tests/test_hip_memory_contracts.py
LS128 = {"GEMM_VARIANT": 7, "GEMM_LS": 0, "GEMM_RS": 0}
LS128X4 = {"GEMM_VARIANT": 7, "GEMM_LS": 1, "GEMM_RS": 0}
PP256 = {"GEMM_VARIANT": 31, "GEMM_TRI": 0, "GEMM_RS": 0}
PP288 = {"GEMM_VARIANT": 31, "GEMM_TRI": 1, "GEMM_RS": 0}
KNOBS = {"lockstep128": LS128, "lockstep128x4": LS128X4, "pingpong256": PP256, "pingpong288": PP288, "edge": {}, "f32": {}}


def _set(tuning, knobs):
    for k_, v_ in knobs.items():
        tuning(k_, v_)


def _launch(problems, expect):
    ops.gemm_nt(problems)
    torch.cuda.synchronize()
    assert ops.last_gemm_variant() == expect, (ops.last_gemm_variant(), expect)


# ---- oracle 1: exact integers ----------------------------------------------------------------------------------------------------------
def _ints(shape, g):
    return torch.randint(-1, 2, shape, generator=g).float()


def _padded(x, ld, dtype):
    """x [.., rows, k] in a buffer with row stride ld > k, NaN in the pad columns"""
    buf = torch.full((*x.shape[:-1], ld), float("nan"))
    buf[..., :x.shape[-1]] = x
    return buf.to(dtype).to(DEV)


def _f64(t):
    return t.double().numpy()


class IntCase:
    """One problem of integers in {-1, 0, 1} with its exact float64 result.  ``rows``: the reference covers those rows only (all
    columns).  ``lr_k``: a low-rank segment with padded rows (lda = lr_k + 64, ldb = lr_k + 8, NaN behind lr_k)."""

    def __init__(self, dtype, m, n, k, seed, *, lr_k=0, ldc=None, rows=None, trans_rows=0, batch=1, residual=False, bias=True):
        g = torch.Generator().manual_seed(seed)
        self.m, self.n, self.trans_rows, self.batch = m, n, trans_rows, batch
        self.rows = torch.arange(m) if rows is None else rows
        bshape = (m, k) if batch == 1 else (batch, m, k)
        a, b = _ints(bshape, g), _ints((n, k) if batch == 1 else (batch, n, k), g)
        ldc = n if ldc is None else ldc
        want = _f64(a[..., self.rows, :]) @ np.swapaxes(_f64(b), -1, -2)
        if trans_rows:
            frames = m // trans_rows
            self.c = torch.full((frames, n, ldc), float("nan"), dtype=dtype, device=DEV)
            stride_c = n * ldc
        else:
            self.c = torch.full((m, ldc) if batch == 1 else (batch, m, ldc), float("nan"), dtype=dtype, device=DEV)
            stride_c = m * ldc if batch > 1 else 0
        p = dict(a=a.to(dtype).to(DEV), b=b.to(dtype).to(DEV), c=self.c, m=m, n=n, k=k, lda=k, ldb=k, ldc=ldc, scale=1.0,
                 batch=batch, stride_a=m * k if batch > 1 else 0, stride_b=n * k if batch > 1 else 0, stride_c=stride_c,
                 trans_rows=trans_rows)
        if lr_k:
            u, bp = _ints((m, lr_k), g), _ints((n, lr_k), g)
            p["lr"] = dict(a=_padded(u, lr_k + 64, dtype), b=_padded(bp, lr_k + 8, dtype), k=lr_k, lda=lr_k + 64, ldb=lr_k + 8)
            want = want + _f64(u[self.rows]) @ _f64(bp).T
        if bias:
            bv = _ints((n,), g)
            p["bias"] = bv.to(dtype).to(DEV)
            want = want + _f64(bv)
        if residual:
            r = _ints(tuple(self.c.shape), g)
            p["residual"] = r.to(dtype).to(DEV)
            assert np.abs(want).max() <= EXACT_LIMIT                        # the rounding in front of the residual add
            want = want + _f64(r)[..., self.rows, :n]
        self.problem, self.want = p, want

    def got(self):
        if self.trans_rows:                                                  # [frame, channel, key] -> [frame * key, channel]
            c = self.c[:, :, :self.trans_rows].permute(0, 2, 1).reshape(self.m, self.n)
            return to_np64(c[self.rows.to(DEV)])
        return to_np64(self.c[..., self.rows.to(DEV), :self.n])

    def check(self, what=""):
        """The precondition on the inputs first (not on the kernel), then exact equality over the whole valid region."""
        assert np.abs(self.want).max() <= EXACT_LIMIT, np.abs(self.want).max()
        got = self.got()
        bad = got != self.want                                               # NaN != x: an element never written counts
        assert np.array_equal(got, self.want), (what, ops.last_gemm_variant(), f"{int(bad.sum())} of {bad.size} elements differ",
                                                "first at", tuple(int(i[0]) for i in np.nonzero(bad)))


# ---- oracles 2 and 3: random-normal operands ------------------------------------------------------------------------------------------
def _normal_problem(dtype, m, n, k, seed):
    """Operands as in test_gemm_engine_selection_and_parity, with bias, scale = 0.5 and a residual; (problem without c, fp64 reference)"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(m, k, generator=g).to(dtype)
    b = (torch.randn(n, k, generator=g) / k ** 0.5).to(dtype)
    bias, res = torch.randn(n, generator=g).to(dtype), torch.randn(m, n, generator=g).to(dtype)
    acc = 0.5 * (to_np64(a) @ to_np64(b).T) + to_np64(bias)
    ref = to_np64(torch.from_numpy(acc).to(dtype)) + to_np64(res)           # the residual is added after the rounding (aid_hip.h)
    p = dict(a=a.to(DEV), b=b.to(DEV), bias=bias.to(DEV), residual=res.to(DEV), m=m, n=n, k=k, lda=k, ldb=k, ldc=n, scale=0.5)
    return p, ref


def _run_normal(p, m, n, dtype, expect):
    c = torch.full((m, n), float("nan"), dtype=dtype, device=DEV)
    _launch([dict(p, c=c)], expect)
    return c


def _within_fp64(c, ref, dtype, what):
    got = to_np64(c)
    assert np.isfinite(got).all(), what
    err, w = rel_l2(got, ref), worst(got, ref)
    assert err < TOL_GEMM[dtype] and w < WORST[dtype], (what, err, w)


# ================================================================================================================================
# A. lock-step rings: Engine<.., NS>::mac, NS = 2 and 4
# ================================================================================================================================
# m = 200, n = 136: a whole tile, a ragged row tile and a ragged column tile
LOCKSTEP_DEPTHS = [("lockstep128", nk) for nk in range(1, 5)] + [("lockstep128x4", nk) for nk in range(1, 7)]


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("engine,nk", LOCKSTEP_DEPTHS, ids=[f"{e}-nk{nk}" for e, nk in LOCKSTEP_DEPTHS])
def test_lockstep_ring_depth_exact_integers(dtype, engine, nk, tuning):
    """NS = 2: the prologue fills min(nk, 1) stages; NS = 4: the regimes nk < 3, = 3, = 4, > 4 of the wait and refill conditions."""
    _set(tuning, KNOBS[engine])
    case = IntCase(dtype, 200, 136, 64 * nk, seed=1000 + nk)
    _launch([case.problem], engine)
    case.check((engine, nk))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("nk", range(1, 7), ids=lambda nk: f"nk{nk}")
def test_lockstep_rings_same_bits_and_fp64_at_every_depth(dtype, nk, tuning):
    """test_lockstep_ring_depths_give_the_same_bits at every short depth: the ring changes how far ahead the loads run, not the sums."""
    p, ref = _normal_problem(dtype, 200, 136, 64 * nk, seed=1100 + nk)
    outs = {}
    for engine in ("lockstep128", "lockstep128x4"):
        _set(tuning, KNOBS[engine])
        outs[engine] = _run_normal(p, 200, 136, dtype, engine)
        _within_fp64(outs[engine], ref, dtype, (engine, nk))
    assert torch.equal(outs["lockstep128"], outs["lockstep128x4"])


# ================================================================================================================================
# B. 256-row ping-pong, NoLR: PingPong::mac (GEMM_PP = 0), mac_rd (1), mac_rd<PRIO> (2)
# ================================================================================================================================
# m = 600: two whole row tiles and 88 rows; n = 320: a whole column tile and 64 columns
PP_LOOPS = [(pp, nk) for pp in (0, 1, 2) for nk in range(1, 7)]


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("pp,nk", PP_LOOPS, ids=[f"pingpong256-pp{pp}-nk{nk}" for pp, nk in PP_LOOPS])
def test_pingpong256_loop_depth_exact_integers(dtype, pp, nk, tuning):
    """mac_rd: nk = 1 runs body (N,N) only, nk = 2 (Y,N) + (N,N), nk >= 3 (Y,Y) ... (Y,N) (N,N); mac: the issue_first guards and
    the retire<P> switch to vmcnt(0) at the last tile."""
    _set(tuning, dict(PP256, GEMM_PP=pp))
    case = IntCase(dtype, 600, 320, 64 * nk, seed=2000 + nk)
    _launch([case.problem], "pingpong256")
    case.check((pp, nk))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("nk", range(1, 7), ids=lambda nk: f"pingpong256-nk{nk}")
def test_pingpong256_loop_orders_same_bits_and_fp64(dtype, nk, tuning):
    """PingPong::half<P> is shared: the three loop orders issue the same MFMAs in the same order per accumulator."""
    p, ref = _normal_problem(dtype, 600, 320, 64 * nk, seed=2100 + nk)
    outs = []
    for pp in (0, 1, 2):
        _set(tuning, dict(PP256, GEMM_PP=pp))
        outs.append(_run_normal(p, 600, 320, dtype, "pingpong256"))
        _within_fp64(outs[-1], ref, dtype, (pp, nk))
    assert torch.equal(outs[0], outs[1]), "GEMM_PP = 0 and 1 differ"
    assert torch.equal(outs[1], outs[2]), "GEMM_PP = 1 and 2 differ"


# ================================================================================================================================
# C. 288-row engine: PingPongX::mac_x<WR, TR>
# ================================================================================================================================
# m = 558: the last tile has 270 rows, its 32-row strip is partly inside the matrix; m = 611: 35 rows, the strip wholly outside
@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("m", [558, 611], ids=lambda m: f"m{m}")
@pytest.mark.parametrize("nk", range(1, 7), ids=lambda nk: f"pingpong288-nk{nk}")
def test_pingpong288_loop_depth_exact_integers(dtype, m, nk, tuning):
    """mac_x<0, false> and <1, false>: both wave groups of every workgroup; waves 0 - 3 count one more DMA (the strip) per K tile."""
    _set(tuning, PP288)
    case = IntCase(dtype, m, 320, 64 * nk, seed=3000 + nk + m)
    _launch([case.problem], "pingpong288")
    case.check((m, nk))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("nk", range(1, 7), ids=lambda nk: f"pingpong288-trans-nk{nk}")
def test_pingpong288_transposed_loop_depth_exact_integers(dtype, nk, tuning):
    """mac_x<0, true> and <1, true>: four frames of 96 rows, C transposed per frame (ldc = 104 > 96; the ABI takes no bias there)."""
    _set(tuning, PP288)
    case = IntCase(dtype, 4 * 96, 200, 64 * nk, seed=3100 + nk, trans_rows=96, ldc=104, bias=False)
    _launch([case.problem], "pingpong288")
    case.check(("trans", nk))
    assert bool(torch.isnan(case.c[:, :, 96:]).all())                       # nothing behind the 96 keys of a channel row


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("nk", [1, 2], ids=lambda nk: f"pingpong288-qkv-nk{nk}")
def test_pingpong288_grouped_qkv_launch_exact_integers(dtype, nk, tuning):
    """The grouped q / k / V^T launch of a self-attention call: three problems over one activation, the third transposed per frame."""
    _set(tuning, PP288)
    frames, s, c = 4, 96, 200
    q = IntCase(dtype, frames * s, c, 64 * nk, seed=3200 + nk)
    k = IntCase(dtype, frames * s, c, 64 * nk, seed=3210 + nk, bias=False)
    vt = IntCase(dtype, frames * s, c, 64 * nk, seed=3220 + nk, trans_rows=s, ldc=104, bias=False)
    for other in (k, vt):                                                    # one activation, as the processor passes it
        other.problem["a"] = q.problem["a"]
        other.want = _f64(q.problem["a"].cpu()) @ _f64(other.problem["b"].cpu()).T
    _launch([q.problem, k.problem, vt.problem], "pingpong288")
    for name, case in (("q", q), ("k", k), ("vt", vt)):
        case.check((name, nk))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("nk", range(1, 7), ids=lambda nk: f"pingpong288-nk{nk}")
def test_pingpong288_loop_depth_fp64(dtype, nk, tuning):
    _set(tuning, PP288)
    p, ref = _normal_problem(dtype, 558, 320, 64 * nk, seed=3300 + nk)
    _within_fp64(_run_normal(p, 558, 320, dtype, "pingpong288"), ref, dtype, nk)


# ================================================================================================================================
# D. tail and side tiles of a ping-pong launch: the NS = 4 ring inside aid_gemm_nt_pp_kernel / aid_gemm_nt_ppx_kernel
# ================================================================================================================================
def _tile_edge_rows(m):
    """Both sides of every 128- and 256-row tile edge, the first and the last row"""
    return torch.unique(torch.cat([torch.arange(127, m, 128), torch.arange(128, m, 128), torch.tensor([0, m - 1])]))


def _tail_shape():
    """One CU round of 256 x 256 tiles plus 8, m and n ragged (test_segment_on_the_tail_tiles_of_a_ragged_last_round): the last
    round is cut into 128 x 128 tiles.  split_pp cuts only where the CU count is a multiple of 8."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    if ncu % 8:
        pytest.skip(f"{ncu} CUs: a ping-pong launch has tail tiles only where the CU count is a multiple of 8")
    return 256 * (ncu // 8 + 1) - 40, 256 * 8 - 24


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("nk", range(1, 6), ids=lambda nk: f"pingpong256+tail128-nk{nk}")
def test_pingpong_tail_tiles_loop_depth_exact_integers(dtype, nk, tuning):
    """Sampled rows on both sides of every 128- and 256-row tile edge, all columns: whichever big tiles the launch cuts up are met."""
    _set(tuning, PP256)
    m, n = _tail_shape()
    case = IntCase(dtype, m, n, 64 * nk, seed=4000 + nk, rows=_tile_edge_rows(m))
    _launch([case.problem], "pingpong256+tail128")
    case.check(("tail", nk))
    assert bool(torch.isfinite(case.c).all())                               # every element of every tile was written


@functools.lru_cache(maxsize=None)
def _side_main(dtype):
    """The query projection of test_gemm_side_tiles_memory_contract (K = 640), shared by every depth of the side problems"""
    return IntCase(dtype, 2050, 638, 640, seed=4100, ldc=648)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("tri,expect", [(0, "pingpong256+side128"), (1, "pingpong288+side128")], ids=["tri0", "tri1"])
@pytest.mark.parametrize("nk", range(1, 6), ids=lambda nk: f"side128-nk{nk}")
def test_pingpong_side_tiles_loop_depth_exact_integers(dtype, tri, expect, nk, tuning):
    """The group of test_gemm_side_tiles_memory_contract with the two side problems (a batched V^T = Wv E^T with 77 keys, ldc 84; a
    key projection with a ragged width and a residual) at K = 64 nk."""
    _set(tuning, dict(PP256, GEMM_TRI=tri))
    main = _side_main(dtype)
    main.c.fill_(float("nan"))
    vt = IntCase(dtype, 640, 77, 64 * nk, seed=4200 + nk, batch=2, ldc=84, bias=False)
    kk = IntCase(dtype, 154, 203, 64 * nk, seed=4300 + nk, ldc=204, residual=True, bias=False)
    _launch([main.problem, vt.problem, kk.problem], expect)
    for name, case in (("main", main), ("vt", vt), ("kk", kk)):
        case.check((name, tri, nk))


# ================================================================================================================================
# E. low-rank segment depth: a second K loop of lr_k / 64 tiles into the same accumulators, on every carrier
# ================================================================================================================================
LR_DEPTHS = [256, 320, 384, 448, 512]
# (id, engine name, knobs, m, n, main K values): K = 128 is an even main nk in front of the segment, 192 an odd one
LR_CARRIERS = [("edge", "edge", {}, 200, 136, (72, 136)),
               ("lockstep128", "lockstep128", LS128, 200, 136, (128, 192)),
               ("lockstep128x4", "lockstep128x4", LS128X4, 200, 136, (128, 192))] + \
              [(f"pingpong256-pp{pp}", "pingpong256", {"GEMM_LR_PP": 1, "GEMM_PP": pp, "GEMM_TRI": 0, "GEMM_RS": 0}, 600, 320, (128, 192))
               for pp in (0, 1, 2)]
LR_CASES = [pytest.param(eng, knobs, m, n, k, r, id=f"{cid}-k{k}-lr{r}")
            for cid, eng, knobs, m, n, ks in LR_CARRIERS for k in ks for r in LR_DEPTHS]


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("engine,knobs,m,n,k,r", LR_CASES)
def test_segment_depth_exact_integers(dtype, engine, knobs, m, n, k, r, tuning):
    """lr_k / 64 = 4 .. 8 K tiles in the segment (GemmLR kernels), behind an even and an odd main loop."""
    _set(tuning, knobs)
    case = IntCase(dtype, m, n, k, seed=5000 + k + r, lr_k=r)
    _launch([case.problem], engine)
    case.check((engine, k, r))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
def test_segment_depth_512_on_the_tail_tiles_exact_integers(dtype, tuning):
    _set(tuning, {"GEMM_LR_PP": 1, "GEMM_TRI": 0, "GEMM_RS": 0})
    m, n = _tail_shape()
    case = IntCase(dtype, m, n, 128, seed=5100, lr_k=512, rows=_tile_edge_rows(m))
    _launch([case.problem], "pingpong256+tail128")
    case.check("tail lr 512")
    assert bool(torch.isfinite(case.c).all())


@pytest.mark.parametrize("k", [128, 192], ids=lambda k: f"f32-k{k}")
@pytest.mark.parametrize("r", LR_DEPTHS, ids=lambda r: f"lr{r}")
def test_segment_depth_float32_exact_integers(k, r):
    case = IntCase(torch.float32, 131, 77, k, seed=5200 + k + r, lr_k=r, ldc=80)
    _launch([case.problem], "f32")
    case.check(("f32", k, r))


LR_GAIN_CASES = [pytest.param(dt, eng, knobs, m, n, ks[-1], id=f"{cid}-{ids_dt(dt)}")
                 for cid, eng, knobs, m, n, ks in LR_CARRIERS for dt in DTYPES] + \
                [pytest.param(torch.float32, "f32", {}, 131, 77, 192, id="f32-float32")]


@pytest.mark.parametrize("dtype,engine,knobs,m,n,k", LR_GAIN_CASES)
def test_segment_depth_512_with_a_row_gain_matches_fp64(dtype, engine, knobs, m, n, k, tuning):
    """The advertised maximum lr_k = 512 with a side-2 DoRA gain, bias, a scale and a residual on random-normal operands; the bounds
    of tests/test_hip_lora_pingpong.py / test_hip_dora.py (16-bit: 2 TOL_GEMM, WORST; float32: 1e-5, 1e-4)."""
    _set(tuning, knobs)
    r = 512
    g = torch.Generator().manual_seed(5300 + k)
    t = lambda *sh, sc=1.0: (torch.randn(*sh, generator=g) * sc).to(dtype).to(DEV)      # noqa: E731
    x, w = t(m, k), t(n, k, sc=0.5)
    u, bp = t(m, r + 64), t(n, r + 8, sc=0.5)
    bias, res = t(n), t(m, n)
    gain = (0.5 + torch.rand(n, generator=g)).to(DEV)
    ldc = (n + 3) // 4 * 4
    c = torch.full((m, ldc), float("nan"), dtype=dtype, device=DEV)
    resb = torch.zeros((m, ldc), dtype=dtype, device=DEV)
    resb[:, :n] = res
    _launch([dict(a=x, b=w, c=c, bias=bias, residual=resb, m=m, n=n, k=k, lda=k, ldb=k, ldc=ldc, scale=0.125,
                  lr=dict(a=u, b=bp, k=r, lda=r + 64, ldb=r + 8, row_scale=gain, scale_side=2))], engine)
    acc = to_np64(x) @ to_np64(w).T + to_np64(u)[:, :r] @ to_np64(bp)[:, :r].T
    pre = 0.125 * to_np64(gain)[None, :] * acc + to_np64(bias)
    want = to_np64(torch.from_numpy(pre).to(dtype)) + to_np64(res)
    got = to_np64(c[:, :n])
    tol, wtol = (TOL_GEMM32, WORST32) if dtype == torch.float32 else (2 * TOL_GEMM[dtype], WORST[dtype])
    err, wst = rel_l2(got, want), worst(got, want)
    print(f"segment 512 + gain {engine} {dtype}: rel-L2 {err:.3e} worst {wst:.3e}")
    assert np.isfinite(got).all()
    assert err < tol and wst < wtol, (engine, err, wst)


# ================================================================================================================================
# F. float32 GEMMs: exact and split kernels at every short K
# ================================================================================================================================
@pytest.mark.parametrize("k", list(range(8, 80, 8)) + [136], ids=lambda k: f"f32-k{k}")
def test_f32_exact_and_split_k_depth_exact_integers(k):
    """Operands in {-1, 0, 1} have no low bf16 half: "highest", "high" and the integer product agree exactly
    (test_gemm_exact_and_split_agree_bit_for_bit_on_small_integers) at every K from one 8-wide step to past two 64-deep tiles."""
    for prec, variant in (("highest", "f32"), ("high", "f32x3")):
        case = IntCase(torch.float32, 131, 77, k, seed=6000 + k, ldc=80)
        case.problem["f32_precision"] = prec
        _launch([case.problem], variant)
        case.check((prec, k))
