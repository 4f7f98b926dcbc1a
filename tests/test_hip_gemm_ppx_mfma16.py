"""The 288-row GEMM engine (PingPongX, csrc/aid_gemm.hip) on 16x16x32 MFMAs: where every accumulator register lands.

The engine computes each wave's 128 x 64 block (and its 32 x 32 block of the strip, tile rows 256 .. 287) as 16 x 16 products:
lane (l15 = lane & 15, kg = lane >> 4) holds row 16 sm + l15, columns 16 sn + 4 kg + e of a block — or, for the transposed (V^T)
instantiation, column 16 sn + l15 and rows 16 sm + 4 kg + e.  Every epilogue knows that layout: the staged fast paths, the generic
edge paths, the transposed store, the folded-LayerNorm fix-ups.  The cases:

1. Placement, exact.  m = 328 (a whole 288-row tile with its strip, a ragged tile of 40 rows), n = 328 (a whole column tile on the
   staged fast path, a ragged one on the edge path), k = 128.  C[m][n] = m % 128, then n % 128 — integers, exact in bf16 and fp16 —
   compared with ``np.array_equal`` on a C pre-filled with NaN: any row, column or block permutation of the layout changes a value.
   The same against the V^T layout.  The ABI takes ``trans_rows % 8 == 0`` only (aid_hip.h), so half of 328 rows (164) is not a
   legal frame length: the transposed cases use frames of 168 rows (m = 336: the frame edge inside the whole tile, 48 ragged rows;
   the per-chunk store path) and of 296 rows (m = 592: frames at least a tile long, the transposed fast store).
2. Every epilogue option, N(0, 1) operands against fp64 within TOL_GEMM / WORST (tests/util.py): bias + scale 0.5 + residual;
   ln_side 1 and 2 with statistics; transposed with ln_side 1.
3. The grouped q / k / V^T launch: three problems over one activation, the third transposed, m = 2 x 288 + 40, k = 64 and 192,
   exact integers in {-1, 0, 1}.
4. CPU only: the fragment address function and the LDS image restated; every ds_read_b128 lane group of every A, B and strip read
   touches 16 distinct 16-byte slots, and the slots a wave reads per K tile are the 64 k of each of its rows, once.

Every GPU case forces the engine and asserts ``ops.last_gemm_variant()``."""
import numpy as np
import pytest
import torch

from util import TOL_GEMM, WORST, rel_l2, to_np64, worst

from aid_amd import ops  # noqa: E402

gpu = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
ids_dt = lambda d: str(d).split(".")[-1]  # noqa: E731
PP288 = {"GEMM_VARIANT": 31, "GEMM_TRI": 1, "GEMM_RS": 0}
M, N, K = 328, 328, 128
TRANS = [(168, 176), (296, 296)]            # (rows per frame, ldc): two frames each
ids_tr = lambda t: f"frame{t[0]}"  # noqa: E731


def _launch(tuning, problems):
    for k_, v_ in PP288.items():
        tuning(k_, v_)
    ops.gemm_nt(problems)
    torch.cuda.synchronize()
    assert ops.last_gemm_variant() == "pingpong288", ops.last_gemm_variant()


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _untrans(c, m, n, rows):
    """[frame, channel, key (ldc)] -> [frame * key, channel]"""
    return c[:, :, :rows].permute(0, 2, 1).reshape(m, n)


# ---- 1. placement ----------------------------------------------------------------------------------------------------------------
def _placement_operands(dtype, m, n, by):
    """A, B with one non-zero k column: C[i][j] = i % 128 (by = "row") or j % 128 ("col")"""
    a, b = torch.zeros(m, K), torch.zeros(n, K)
    a[:, 0] = (torch.arange(m) % 128).float() if by == "row" else 1.0
    b[:, 0] = (torch.arange(n) % 128).float() if by == "col" else 1.0
    want = np.broadcast_to((np.arange(m) % 128)[:, None] if by == "row" else (np.arange(n) % 128)[None, :], (m, n)).astype(np.float64)
    return a.to(dtype).to(DEV), b.to(dtype).to(DEV), want


def _same(got, want):
    bad = got != want                                                        # NaN != x: an element never written counts
    assert np.array_equal(got, want), (f"{int(bad.sum())} of {bad.size} elements differ", "first at",
                                       tuple(int(i[0]) for i in np.nonzero(bad)), "got", got[bad][:4], "want", want[bad][:4])


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("by", ["row", "col"])
def test_placement_exact(dtype, by, tuning):
    a, b, want = _placement_operands(dtype, M, N, by)
    c = _nan((M, N), dtype)
    _launch(tuning, [dict(a=a, b=b, c=c, m=M, n=N, k=K, lda=K, ldb=K, ldc=N, scale=1.0)])
    _same(to_np64(c), want)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("by", ["row", "col"])
@pytest.mark.parametrize("frame", TRANS, ids=ids_tr)
def test_placement_exact_transposed(dtype, by, frame, tuning):
    rows, ldc = frame
    m = 2 * rows
    a, b, want = _placement_operands(dtype, m, N, by)
    c = _nan((2, N, ldc), dtype)
    _launch(tuning, [dict(a=a, b=b, c=c, m=m, n=N, k=K, lda=K, ldb=K, ldc=ldc, stride_c=N * ldc, trans_rows=rows, scale=1.0)])
    _same(to_np64(_untrans(c, m, N, rows)), want)
    assert bool(torch.isnan(c[:, :, rows:]).all())                           # nothing behind the keys of a channel row


# ---- 2. epilogue options ---------------------------------------------------------------------------------------------------------
def _normal_operands(dtype, m, n, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(m, K, generator=g).to(dtype)
    b = (torch.randn(n, K, generator=g) / K ** 0.5).to(dtype)
    return g, a, b, to_np64(a) @ to_np64(b).T


def _ln_constants(g, act_rows, w_rows):
    """(mean, rstd) per activation row, (colsum, shift) per weight row: any numbers — the epilogue is checked, not LayerNorm"""
    st = torch.stack([torch.randn(act_rows, generator=g) * 0.3, torch.rand(act_rows, generator=g) * 0.4 + 0.8], dim=1)
    return st, torch.randn(w_rows, generator=g), torch.randn(w_rows, generator=g) * 0.5


def _within_fp64(got, ref, dtype, what):
    assert np.isfinite(got).all(), what
    err, w = rel_l2(got, ref), worst(got, ref)
    print(f"{what} {ids_dt(dtype)}: rel-L2 {err:.3e} (bound {TOL_GEMM[dtype]:.0e}), worst {w:.3e} (bound {WORST[dtype]:.0e})")
    assert err < TOL_GEMM[dtype] and w < WORST[dtype], (what, err, w)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
def test_bias_scale_residual_fp64(dtype, tuning):
    g, a, b, acc = _normal_operands(dtype, M, N, seed=11)
    bias, res = torch.randn(N, generator=g).to(dtype), torch.randn(M, N, generator=g).to(dtype)
    ref = to_np64(torch.from_numpy(0.5 * acc + to_np64(bias)).to(dtype)) + to_np64(res)     # the residual is added after the rounding
    c = _nan((M, N), dtype)
    _launch(tuning, [dict(a=a.to(DEV), b=b.to(DEV), c=c, bias=bias.to(DEV), residual=res.to(DEV), m=M, n=N, k=K, lda=K, ldb=K, ldc=N,
                          scale=0.5)])
    _within_fp64(to_np64(c), ref, dtype, "bias+scale+residual")


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("side", [1, 2], ids=["ln1", "ln2"])
def test_folded_layernorm_fp64(dtype, side, tuning):
    g, a, b, acc = _normal_operands(dtype, M, N, seed=20 + side)
    st, cs, sh = _ln_constants(g, M if side == 1 else N, N if side == 1 else M)
    s64, c64, h64 = to_np64(st), to_np64(cs), to_np64(sh)
    bias = torch.randn(N, generator=g).to(dtype)
    if side == 1:
        ref = s64[:, 1:2] * (acc - s64[:, 0:1] * c64[None, :]) + h64[None, :]
    else:
        ref = s64[None, :, 1] * (acc - s64[None, :, 0] * c64[:, None]) + h64[:, None]
    ref = 0.5 * ref + to_np64(bias)
    c = _nan((M, N), dtype)
    _launch(tuning, [dict(a=a.to(DEV), b=b.to(DEV), c=c, bias=bias.to(DEV), m=M, n=N, k=K, lda=K, ldb=K, ldc=N, scale=0.5,
                          ln_stats=st.to(DEV), ln_colsum=cs.to(DEV), ln_shift=sh.to(DEV), ln_side=side)])
    _within_fp64(to_np64(c), ref, dtype, f"ln_side {side}")


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("frame", TRANS, ids=ids_tr)
def test_transposed_folded_layernorm_fp64(dtype, frame, tuning):
    rows, ldc = frame
    m = 2 * rows
    g, a, b, acc = _normal_operands(dtype, m, N, seed=30 + rows)
    st, cs, sh = _ln_constants(g, m, N)
    s64 = to_np64(st)
    ref = 0.5 * (s64[:, 1:2] * (acc - s64[:, 0:1] * to_np64(cs)[None, :]) + to_np64(sh)[None, :])
    c = _nan((2, N, ldc), dtype)
    _launch(tuning, [dict(a=a.to(DEV), b=b.to(DEV), c=c, m=m, n=N, k=K, lda=K, ldb=K, ldc=ldc, stride_c=N * ldc, trans_rows=rows,
                          scale=0.5, ln_stats=st.to(DEV), ln_colsum=cs.to(DEV), ln_shift=sh.to(DEV), ln_side=1)])
    _within_fp64(to_np64(_untrans(c, m, N, rows)), ref, dtype, f"transposed ln_side 1, frames of {rows}")
    assert bool(torch.isnan(c[:, :, rows:]).all())


# ---- 3. grouped q / k / V^T ------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("k", [64, 192], ids=lambda k: f"k{k}")
def test_grouped_qkv_exact_integers(dtype, k, tuning):
    m, n, rows, ldc = 2 * 288 + 40, 328, 88, 96                              # 7 frames of 88 rows
    g = torch.Generator().manual_seed(40 + k)
    ints = lambda *shape: torch.randint(-1, 2, shape, generator=g).float()  # noqa: E731
    x, w = ints(m, k), [ints(n, k) for _ in range(3)]
    want = [to_np64(x) @ to_np64(wi).T for wi in w]
    assert max(np.abs(v).max() for v in want) <= 256                         # exact in bf16 and fp16, in any order of the sums
    xd = x.to(dtype).to(DEV)
    cq, ck, cv = _nan((m, n), dtype), _nan((m, n), dtype), _nan((m // rows, n, ldc), dtype)
    base = dict(a=xd, m=m, n=n, k=k, lda=k, ldb=k, scale=1.0)
    _launch(tuning, [dict(base, b=w[0].to(dtype).to(DEV), c=cq, ldc=n), dict(base, b=w[1].to(dtype).to(DEV), c=ck, ldc=n),
                     dict(base, b=w[2].to(dtype).to(DEV), c=cv, ldc=ldc, stride_c=n * ldc, trans_rows=rows)])
    _same(to_np64(cq), want[0])
    _same(to_np64(ck), want[1])
    _same(to_np64(_untrans(cv, m, n, rows)), want[2])
    assert bool(torch.isnan(cv[:, :, rows:]).all())


# ---- 4. CPU: fragment addresses against the LDS image ------------------------------------------------------------------------------
HALF = 128 * 128                             # bytes of a half-tile: 128 rows of 128 B (64 k)
# lanes served together by one ds_read_b128 pass (each 16-byte slot spans 4 of the 64 banks: 16 distinct slots mod 16 = no conflict)
LANE_GROUPS = [[*range(0, 4), *range(12, 16), *range(20, 28)], [*range(4, 12), *range(16, 20), *range(28, 32)],
               [*range(32, 36), *range(44, 48), *range(52, 60)], [*range(36, 44), *range(48, 52), *range(60, 64)]]


def swz(r):
    return (r >> 1) & 7


def frag_addr(region_base, row_base, lane, j):
    """Byte address (inside a parity) of lane's 16 bytes of the fragment over rows row_base .. + 15, k 32 j .. 32 j + 31: logical
    chunk 4 j + kg of row row_base + l15, stored at slot chunk ^ swz(row) of that row (rows count from the region's first row)"""
    l15, kg = lane & 15, lane >> 4
    row = row_base + l15
    return region_base + row * 128 + (((4 * j + kg) ^ swz(row)) << 4)


def wave_reads(wr, wc):
    """Every fragment read of wave (wr, wc) in one K tile: (name, first tile row or column, region base, row inside the region, j)"""
    out = []
    for h in range(2):                       # A half h: tile rows with bit 6 == h; LDS row = 64 (tile row >> 7) + (tile row & 63)
        for eb in range(4):
            out += [("A", wr * 128 + h * 64 + eb * 16, h * HALF, wr * 64 + eb * 16, j) for j in range(2)]
    for jh in range(2):                      # B half jh: tile columns with bit 5 == jh
        for sn in range(2):
            out += [("B", wc * 64 + jh * 32 + sn * 16, (2 + jh) * HALF, wc * 32 + sn * 16, j) for j in range(2)]
    for sm in range(2):                      # the strip: tile rows 256 .. 287
        out += [("X", 256 + sm * 16, 4 * HALF, sm * 16, j) for j in range(2)]
    return out


def test_fragment_reads_are_conflict_free_and_cover_each_row_once():
    for wr in range(2):
        for wc in range(4):
            reads = wave_reads(wr, wc)
            assert len(reads) == 16 + 8 + 4                                  # 8 A per phase, 8 B and 4 strip fragments per K tile
            seen = {}
            for name, first, base, row0, j in reads:
                addr = [frag_addr(base, row0, lane, j) for lane in range(64)]
                assert all(a % 16 == 0 for a in addr)
                for grp in LANE_GROUPS:
                    slots = {(addr[lane] // 16) % 16 for lane in grp}
                    assert len(slots) == 16, (name, first, j, grp, sorted(slots))
                for lane in range(64):                                       # which logical chunk of which row did the lane get?
                    row = row0 + (lane & 15)
                    assert base + row * 128 <= addr[lane] < base + (row + 1) * 128
                    chunk = ((addr[lane] - base - row * 128) >> 4) ^ swz(row)
                    assert chunk == 4 * j + (lane >> 4)                      # k = 8 chunk .. + 7: what the MFMA expects of the lane
                    seen.setdefault((name, first + (lane & 15)), []).append(chunk)
            rows_a = {("A", wr * 128 + r) for r in range(128)}
            cols_b = {("B", wc * 64 + c) for c in range(64)}
            rows_x = {("X", 256 + r) for r in range(32)}
            assert set(seen) == rows_a | cols_b | rows_x
            for key, chunks in seen.items():
                assert sorted(chunks) == list(range(8)), (key, chunks)       # the 64 k of the row, once
