"""GPU: the IP-Adapter segment kernel (aid_ip_attn_kernel, csrc/aid_attn_ip.hip) beyond one workgroup per (frame, head), at every key
count, with eight and more segments per call, and with score levels that make the online-softmax rescale fire.

Every launch goes through ``ops.ip_attn_accumulate``; the reference is ``ip_multi_ref.segments_sum`` (fp64) on the same dtype-rounded
inputs (cases: tests/ip_segment_cases.py, checked on the CPU by tests/test_ip_segment_cases.py); bounds are TOL / WORST of util.py.
Figures are taken per TILE — one (frame, head, 32-row block), the work of one wave — so that one wrong tile cannot hide behind right
ones: ``worst`` is the largest error of the tile over the RMS of the tile's reference.  Every test also asserts that every output
element is finite.  3 heads, 2 or 3 frames with their own K / V unless a test says otherwise.

  a  rows beyond one workgroup: every S of ROW_COUNTS (grids of 9, 18, 27 blocks; 2 blocks for n = heads = 1, S = 129)
  b  rows and frames are independent, bit for bit
  c  one key, 300 rows: out0 + (scale w[row]) v exactly
  d  every key count of KEY_COUNTS, and five of them on guarded buffers
  e  eight segments in one launch, nine in two; every segment's contribution visible
  f  score levels "steps" / "ramp" / "level", alone and beside one another
  g  softmax_scale and q_prescaled

Measured on an MI355X, largest figure per group over d = 40 / 64 / 80 / 160 and over the tiles (rel-L2 / worst):
    a   fp16 2.98e-4 / 2.23e-3   bf16 2.92e-3 / 1.81e-2
    d   fp16 3.10e-4 / 3.73e-3   bf16 2.57e-3 / 3.13e-2
    e   fp16 3.04e-4 / 4.63e-3   bf16 2.43e-3 / 2.08e-2      (the full lists of eight and nine)
    f   fp16 2.87e-4 / 2.92e-3   bf16 2.31e-3 / 3.06e-2
These are the figures of the CPU restatement of the kernel's arithmetic (``ip_segment_cases.emulate``) on the same inputs to two
digits; (b) and (c) hold bit for bit.  The 104 tests of the module take 8 s.  The kernel passed all of them unchanged.

Three in-bounds mutations of the kernel, built apart and never committed, against this module: without ``ls *= alpha`` a, d, e, f and
g fail; with the ragged mask ``> lim`` in place of ``>= lim`` a, c, d, e, f and g fail; with waves 0 / 1 and 2 / 3 of the workgroups
behind the first exchanging tiles while the early exit keeps the wave's own tile, a, e, f and g fail (every S whose last workgroup
runs an odd number of waves).  When the exit follows the exchanged tile as well, every tile is still computed by exactly one wave and
the results are the same bits: no test can tell that form from the kernel."""
import ctypes as C
import functools
import math
from collections import namedtuple

import numpy as np
import pytest
import torch

import ip_segment_cases as IC
from ip_multi_ref import attention, segments_sum
from util import TOL, WORST, rel_l2, to_np64, worst

pytestmark = pytest.mark.gpu

from aid_amd import _lib, ops  # noqa: E402
from guarded import Guarded  # noqa: E402

DEV = torch.device("cuda:0")
DTYPES = [torch.float16, torch.bfloat16]
DIMS = [40, 64, 80, 160]
HEADS = 3
ids_dt = lambda d: str(d).split(".")[-1]  # noqa: E731
on_all = lambda f: pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)(pytest.mark.parametrize("d", DIMS)(f))  # noqa: E731

# one image-key segment on the CPU: k / v [R, t, C], vt [R, C, round_up(t, 8)] (NaN pad columns), w float32 [S] or None
Seg = namedtuple("Seg", "k v vt scale w")
FIGURES = {}


def _dev(seg, rows=slice(None), frames=slice(None)):
    k, vt = (seg.k, seg.vt) if seg.k.shape[0] == 1 else (seg.k[frames], seg.vt[frames])
    return dict(k=k.contiguous().to(DEV), vt=vt.contiguous().to(DEV), scale=seg.scale,
                row_weight=None if seg.w is None else seg.w[rows].contiguous().to(DEV))


def _launch(q, out0, segs, heads=HEADS, rows=slice(None), frames=slice(None), **kw):
    """One ``ip_attn_accumulate`` call over the given rows / frames (contiguous copies); the result on the CPU."""
    out = out0[frames, rows].contiguous().to(DEV, copy=True)
    assert ops.ip_attn_accumulate(q[frames, rows].contiguous().to(DEV), out, [_dev(g, rows, frames) for g in segs], heads, **kw) is out
    torch.cuda.synchronize()
    return out.cpu()


def _contributions(q, segs, heads=HEADS):
    """fp64 [G, N, S, C]: scale_g w_g[row] softmax(q K_g^T / sqrt(d)) V_g of every segment."""
    q64 = to_np64(q)
    return np.stack([segments_sum(q64, [(to_np64(g.k), to_np64(g.v), g.scale, None if g.w is None else to_np64(g.w))], heads)
                     for g in segs])


def _by_tile(x, heads):
    """x [n, s, heads d] as [n, blocks, 32, heads, d] (rows past s: zeros) and the number of elements of every block's tiles."""
    n, s, c = x.shape
    nb = (s + 31) // 32
    t = np.pad(x, ((0, 0), (0, 32 * nb - s), (0, 0))).reshape(n, nb, 32, heads, c // heads)
    return t, np.minimum(32, s - 32 * np.arange(nb)) * (c // heads)


def _tile_norms(x, heads):
    t, _ = _by_tile(x, heads)
    return np.sqrt((t * t).sum((2, 4)))                                             # [n, blocks, heads]


def _tiles(got, ref, heads):
    """(largest rel-L2, largest worst, where) over the (frame, head, 32-row block) tiles."""
    e, count = _by_tile(got - ref, heads)
    en, rn = _tile_norms(got - ref, heads), _tile_norms(ref, heads)
    rel = en / (rn + 1e-30)
    wst = np.abs(e).max((2, 4)) / (rn / np.sqrt(count)[None, :, None] + 1e-30)
    i, j = np.unravel_index(rel.argmax(), rel.shape), np.unravel_index(wst.argmax(), wst.shape)
    return float(rel.max()), float(wst.max()), f"rel-L2 at (frame, block, head) {tuple(map(int, i))}, worst at {tuple(map(int, j))}"


def _check(got, ref, dtype, what, group=None, heads=HEADS, fails=None):
    """Finite, and every tile within TOL / WORST; failures go to ``fails`` (a loop reports all of them) or raise."""
    got = to_np64(got) if torch.is_tensor(got) else got
    r, w, where = _tiles(got, ref, heads)
    msg = f"{what}: tiles rel-L2 {r:.3e} worst {w:.3e} ({where}); tensor rel-L2 {rel_l2(got, ref):.3e} worst {worst(got, ref):.3e}"
    if group is not None and np.isfinite(got).all():
        key = (group, ids_dt(dtype))
        FIGURES[key] = tuple(max(a, b) for a, b in zip(FIGURES.get(key, (0.0, 0.0)), (r, w)))
        msg += f"   [largest of group {group} {key[1]} so far: {FIGURES[key][0]:.2e} / {FIGURES[key][1]:.2e}]"
    print(msg)
    ok = bool(np.isfinite(got).all()) and r < TOL[dtype] and w < WORST[dtype]
    if fails is None:
        assert ok, msg
    elif not ok:
        fails.append(msg)


def _weights(s, seed, zeros):
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(s, generator=g)
    if zeros:
        w[torch.rand(s, generator=g) < 0.4] = 0.0
        w[0] = 0.0
    return w.to(torch.float32)


@functools.lru_cache(maxsize=None)
def _three(dtype, d, n, s, heads=HEADS):
    """q, out0 ~ N(0, 0.3) and three segments of 4, 40 and 70 keys: the first shared by the frames (n_rows = 1), the second with a
    negative scale, the third with a float32 row weight that includes zeros."""
    seed = 1000 * d + s
    segs = []
    for i, (t, scale) in enumerate(((4, 0.7), (40, -0.5), (70, 1.0))):
        q, k, v, vt = IC.score_case("random", dtype, d, n, s, t, heads, seed + i)
        if i == 0:
            k, v, vt = k[:1], v[:1], vt[:1]
        segs.append(Seg(k, v, vt, scale, _weights(s, seed, True) if i == 2 else None))
    out0 = (torch.randn(n, s, heads * d, generator=torch.Generator().manual_seed(seed + 9)) * 0.3).to(dtype)
    return q, out0, tuple(segs)


# ---- a. rows beyond one workgroup ----------------------------------------------------------------------------------------------------
@on_all
def test_a_every_row_count(dtype, d):
    """n = 3, 3 heads, S from 1 to 300: chunks = 1, 2, 3 workgroups per (frame, head), grids of 9, 18 and 27 blocks (fewer than 8 per
    XCD, no multiple of 8); the last workgroup of a (frame, head) runs 1 .. 4 waves.  Onto out = 0 and onto N(0, 0.3) data."""
    fails = []
    for s in IC.ROW_COUNTS:
        q, out0, segs = _three(dtype, d, 3, s)
        image = _contributions(q, segs).sum(0)
        for acc in (False, True):
            o0 = out0 if acc else torch.zeros_like(out0)
            _check(_launch(q, o0, segs), to_np64(o0) + image, dtype, f"S {s} acc={acc}", "a", fails=fails)
    assert not fails, "\n".join(fails)


@on_all
def test_a_two_blocks(dtype, d):
    """n = 1, one head, S = 129: a grid of two blocks, the second with one live wave of one row."""
    q, out0, segs = _three(dtype, d, 1, 129, 1)
    _check(_launch(q, out0, segs, 1), to_np64(out0) + _contributions(q, segs, 1).sum(0), dtype, "S 129, 1 x 1", "a", heads=1)


# ---- b. rows and frames are independent ----------------------------------------------------------------------------------------------
@on_all
def test_b_rows_and_frames_are_independent_bit_for_bit(dtype, d):
    """S = 300 in one launch = the rows [0, 128), [128, 256), [256, 300) in three launches over contiguous copies (with their slices of
    out and row_weight); a frame run alone (n = 1, its own K / V^T rows) = that frame inside the n = 3 launch."""
    q, out0, segs = _three(dtype, d, 3, 300)
    whole = _launch(q, out0, segs)
    assert torch.isfinite(whole).all()
    for rows in (slice(0, 128), slice(128, 256), slice(256, 300)):
        assert torch.equal(_launch(q, out0, segs, rows=rows), whole[:, rows]), rows
    for f in range(3):
        assert torch.equal(_launch(q, out0, segs, frames=slice(f, f + 1)), whole[f:f + 1]), f


# ---- c. one key, many rows -----------------------------------------------------------------------------------------------------------
@on_all
def test_c_one_key_many_rows_exact(dtype, d):
    """t = 1, S = 300, a row weight and scale -1.5: the softmax over one key is exactly 1 (P = exp2 of a rounding-sized number rounds
    to 1 in the storage type, the row sum is 1), so the launch adds (scale w[row]) v in fp32 and rounds once — the product order of
    the kernel, (scale / rowsum) * w first, is the one written here, and the result is equal bit for bit."""
    n, s = 3, 300
    q, k, v, vt = IC.score_case("random", dtype, d, n, s, 1, HEADS, seed=d)
    w = _weights(s, d, False)
    out0 = (torch.randn(n, s, HEADS * d, generator=torch.Generator().manual_seed(d + 1)) * 0.3).to(dtype)
    got = _launch(q, out0, [Seg(k, v, vt, -1.5, w)])
    want = (out0.float() + (-1.5 * w)[None, :, None] * v.float()).to(dtype)
    assert torch.isfinite(got).all()
    assert torch.equal(got, want), f"{(got != want).sum().item()} of {got.numel()} elements differ"


# ---- d. every key count --------------------------------------------------------------------------------------------------------------
@on_all
def test_d_every_key_count(dtype, d):
    """One segment of t keys per launch, t = 1 .. 72 and 95 .. 257: every remainder class of the ragged score tile, of the skipped
    16-key step and of the two guarded 4-key V^T pieces, one to nine score tiles.  S = 70 (two whole row tiles and one of 6 rows);
    V^T has ldvt = round_up(t, 8) and NaN in its pad columns."""
    fails = []
    zero = torch.zeros(2, 70, HEADS * d, dtype=dtype)
    for t in IC.KEY_COUNTS:
        q, k, v, vt = IC.score_case("random", dtype, d, 2, 70, t, HEADS, seed=100 * d + t)
        seg = Seg(k, v, vt, 1.0, None)
        _check(_launch(q, zero, [seg]), _contributions(q, [seg])[0], dtype, f"t {t}", "d", fails=fails)
    assert not fails, "\n".join(fails)


@on_all
def test_d_key_counts_on_guarded_buffers(dtype, d):
    """t = 1, 7, 37, 70, 129 with q, K and V^T in buffers whose pad columns, gap rows and guard bands hold NaN and `out` between
    sentinel bands with a row stride wider than the view: finite and right, no input bit changes, only the view of `out` is written."""
    n, s = 2, 70
    c = HEADS * d
    lib = _lib.load()
    for t in (1, 7, 37, 70, 129):
        q, k, v, _ = IC.score_case("random", dtype, d, n, s, t, HEADS, seed=100 * d + t + 1)
        ldvt = IC.round_up(t, 8)
        qg = Guarded(n, s, c, dtype, DEV, ld=c + 8, gap_rows=1).set(q)
        og = Guarded(n, s, c, dtype, DEV, ld=c + 16, gap_rows=2, kind="output")
        out0 = (torch.randn(n, s, c, generator=torch.Generator().manual_seed(t)) * 0.3).to(dtype)
        og.view.copy_(out0)
        kg = Guarded(n, t, c, dtype, DEV, gap_rows=3).set(k)                                    # rows >= t of every frame: NaN
        vg = Guarded(n, c, t, dtype, DEV, ld=ldvt, gap_rows=1).set(v.transpose(1, 2))           # columns [t, ldvt): NaN
        w = _weights(s, t, False)
        wd = w.to(DEV)
        segs = (_lib.AidIpSegment * 1)()
        e = segs[0]
        e.k, e.vt, e.row_weight = kg.ptr, vg.ptr, wd.data_ptr()
        e.k_fs, e.vt_fs, e.t, e.ldvt, e.n_rows, e.scale = kg.fs, vg.fs, t, ldvt, n, 0.8
        a = _lib.AidIpAttnArgs()
        a.q, a.out, a.segments, a.n_segments = qg.ptr, og.ptr, C.addressof(segs), 1
        a.n_frames, a.s, a.heads, a.d = n, s, HEADS, d
        a.ldq, a.ldo, a.q_fs, a.o_fs = qg.ld, og.ld, qg.fs, og.fs
        a.dtype, a.softmax_scale = ops._dtype_code(qg.view), d ** -0.5
        _lib.check(lib.aid_ip_attn_fwd(C.byref(a), torch.cuda.current_stream().cuda_stream), "aid_ip_attn_fwd")
        torch.cuda.synchronize()
        _check(og.view.cpu(), to_np64(out0) + _contributions(q, [Seg(k, v, None, 0.8, w)])[0], dtype, f"guarded t {t}")
        assert og.untouched(og.layout.region_mask()) == "", t
        for buf in (qg, kg, vg):
            assert buf.inputs_unchanged() == "", t


# ---- e. eight segments, and more than eight ------------------------------------------------------------------------------------------
E_KEYS = (1, 5, 16, 31, 32, 33, 64, 77, 257)
E_SCALES = (0.4, -0.6, 1.0, 0.8, -1.2, 0.9, 1.3, -1.1, 1.5)
E_SHARED = (True, False, False, True, False, True, False, False, False)
E_WEIGHTS = {2: False, 5: True, 7: False, 8: True}           # segment -> row weight with zeros?


@functools.lru_cache(maxsize=None)
def _nine(dtype, d):
    n, s = 2, 160
    segs = []
    for g, t in enumerate(E_KEYS):
        q, k, v, vt = IC.score_case("random", dtype, d, n, s, t, HEADS, seed=10 * d + g)
        if E_SHARED[g]:
            k, v, vt = k[:1], v[:1], vt[:1]
        segs.append(Seg(k, v, vt, E_SCALES[g], _weights(s, g, E_WEIGHTS[g]) if g in E_WEIGHTS else None))
    out0 = (torch.randn(n, s, HEADS * d, generator=torch.Generator().manual_seed(d)) * 0.3).to(dtype)
    contrib = _contributions(q, segs)
    contrib.setflags(write=False)
    return q, out0, tuple(segs), contrib


@pytest.mark.parametrize("count", [8, 9])
@on_all
def test_e_eight_and_nine_segments(dtype, d, count):
    """Eight segments of 1 .. 77 keys (n_rows 1 and n, scales of both signs, row weights on some) are ONE launch, the kernel's limit;
    with a ninth of 257 keys ``ip_attn_accumulate`` makes two launches, and `out` is rounded to the storage type between them: that
    extra rounding is half an ulp of a number of the result's size, as the final one, so the pair stays within TOL (two roundings
    of 2^-12 / 2^-9 relative at the most against bounds of 1e-3 / 8e-3 that one launch meets with a factor 3 to spare).

    Every segment is visible: the list without segment g differs from the full list by that segment's fp64 contribution.  Both
    outputs are rounded at the size of the full result, so the difference is held to TOL / WORST relative to the full reference
    (tile by tile); a segment that the kernel dropped or took twice would miss by its whole contribution, which the test first
    checks to be at least 4 TOL of the full result in every tile's norm."""
    q, out0, segs, contrib = _nine(dtype, d)
    segs, contrib = segs[:count], contrib[:count]
    ref = to_np64(out0) + contrib.sum(0)
    full = _launch(q, out0, segs)
    _check(full, ref, dtype, f"{count} segments", "e")
    fails = []
    for g in range(count):
        rest = _launch(q, out0, segs[:g] + segs[g + 1:])
        low = float((_tile_norms(contrib[g], HEADS) / _tile_norms(ref, HEADS)).min())
        assert low > 4 * TOL[dtype], (g, low)
        # (full - rest) against contrib[g], measured on the scale of the full result: ref with its segment g replaced by the measured one
        _check(ref - contrib[g] + (to_np64(full) - to_np64(rest)), ref, dtype,
               f"{count} segments, without {g} (t {E_KEYS[g]}, smallest share of a tile {low:.3f})", fails=fails)
    assert not fails, "\n".join(fails)


# ---- f. score levels -----------------------------------------------------------------------------------------------------------------
def _classes(s):
    b = IC.row_levels(s).numpy()
    return (("rising", b > 0.5), ("falling", b < -0.5), ("rest", np.abs(b) <= 0.5))


def _check_classes(got, ref, dtype, what, fails):
    got = to_np64(got)
    for name, rows in _classes(ref.shape[1]):
        r, w = rel_l2(got[:, rows], ref[:, rows]), worst(got[:, rows], ref[:, rows])
        print(f"{what} {name} rows: rel-L2 {r:.3e} worst {w:.3e}")
        if not (r < TOL[dtype] and w < WORST[dtype]):
            fails.append(f"{what} {name} rows: rel-L2 {r:.3e} worst {w:.3e}")


@pytest.mark.parametrize("kind", ["steps", "ramp", "level"])
@on_all
def test_f_score_levels(dtype, d, kind):
    """One segment per launch, t = 33 / 70 / 257, S = 160 (rows -3 .. 3: one wave tile holds rising and falling rows).  Bounds per row
    class — rising (b > 0.5: the maximum moves up at every tile and alpha is small), falling (b < -0.5: the maximum is in the first
    tile), the rest — and per tile.  For d = 160 the two channel passes each run their own softmax: a pass that disagreed would put
    channels 96 .. 159 out of bounds.  A second launch gives the same bits."""
    fails = []
    zero = torch.zeros(2, 160, HEADS * d, dtype=dtype)
    for t in (33, 70, 257):
        q, k, v, vt = IC.score_case(kind, dtype, d, 2, 160, t, HEADS, seed=d + t)
        seg = Seg(k, v, vt, 1.0, None)
        got, ref = _launch(q, zero, [seg]), _contributions(q, [seg])[0]
        _check(got, ref, dtype, f"{kind} t {t}", "f", fails=fails)
        _check_classes(got, ref, dtype, f"{kind} t {t}", fails)
        if d == 160:
            for lo, hi in ((0, 96), (96, 160)):
                ch = np.concatenate([np.arange(h * d + lo, h * d + hi) for h in range(HEADS)])
                r = rel_l2(to_np64(got)[..., ch], ref[..., ch])
                print(f"{kind} t {t} channels {lo} .. {hi - 1}: rel-L2 {r:.3e}")
                if not r < TOL[dtype]:
                    fails.append(f"{kind} t {t} channels {lo} .. {hi - 1}: rel-L2 {r:.3e}")
        assert torch.equal(_launch(q, zero, [seg]), got), t
    assert not fails, "\n".join(fails)


@on_all
def test_f_levels_side_by_side(dtype, d):
    """A "steps" (257 keys), a "level" (70) and a "random" (33) segment in ONE launch over the same q: maximum, row sum and
    accumulator of a segment must not leak into the next (after "steps" the maximum of a rising row is 288 nat above its scores in
    "random"; after "level" it is 60 nat off either way)."""
    n, s = 2, 160
    segs = []
    for i, (kind, t, scale) in enumerate((("steps", 257, 1.0), ("level", 70, -0.7), ("random", 33, 0.6))):
        q_i, k, v, vt = IC.score_case(kind, dtype, d, n, s, t, HEADS, seed=d + i)
        if i == 0:
            q = q_i
        segs.append(Seg(k, v, vt, scale, None))
    zero = torch.zeros(n, s, HEADS * d, dtype=dtype)
    got, ref = _launch(q, zero, segs), _contributions(q, segs).sum(0)
    fails = []
    _check(got, ref, dtype, "steps | level | random", "f", fails=fails)
    _check_classes(got, ref, dtype, "steps | level | random", fails)
    for order in ((2, 0, 1), (1, 2, 0)):                       # the same three in another order: the same sum
        _check(_launch(q, zero, [segs[i] for i in order]), ref, dtype, f"order {order}", "f", fails=fails)
    assert torch.equal(_launch(q, zero, segs), got)
    assert not fails, "\n".join(fails)


# ---- g. scale handling ---------------------------------------------------------------------------------------------------------------
@on_all
def test_g_softmax_scale_and_prescaled_q(dtype, d):
    """S = 160, t = 70, "ramp".  softmax_scale = 0.2 in place of d^-0.5; and q already multiplied by d^-0.5 log2(e), rounded to the
    storage type, with q_prescaled: the oracle sees the same rounded q with scale ln 2."""
    n, s, t = 2, 160, 70
    q, k, v, vt = IC.score_case("ramp", dtype, d, n, s, t, HEADS, seed=d + 5)
    seg = Seg(k, v, vt, 0.9, _weights(s, d, False))
    zero = torch.zeros(n, s, HEADS * d, dtype=dtype)
    k64, v64, w64 = to_np64(k), to_np64(v), to_np64(seg.w)[None, :, None]
    ref = 0.9 * w64 * attention(to_np64(q) * (0.2 * math.sqrt(d)), k64, v64, HEADS)          # (the oracle divides by sqrt(d))
    _check(_launch(q, zero, [seg], softmax_scale=0.2), ref, dtype, "softmax_scale 0.2")
    qs = (q.float() * (d ** -0.5 * IC.LOG2E)).to(dtype)
    ref = 0.9 * w64 * attention(to_np64(qs) * (math.log(2.0) * math.sqrt(d)), k64, v64, HEADS)
    _check(_launch(qs, zero, [seg], q_prescaled=True), ref, dtype, "q_prescaled")
