"""CPU: the score cases of tests/ip_segment_cases.py do what the GPU tests of the IP-Adapter segment kernel count on.

* "steps" and "ramp" really move the running maximum of the online softmax: on the inputs ROUNDED to fp16 / bf16 a quarter of the rows
  or more raise their maximum at every 32-key tile, a quarter or more have it in the first tile and lower ones in every later tile, and
  one aligned 32-row block (a wave's tile) holds rows of both sorts.
* Every kind leaves the fp64 reference well conditioned: the kernel's arithmetic restated in torch (``emulate``) stays under the
  project's TOL / WORST against ``ip_multi_ref.attention`` on the same rounded inputs, so those bounds are fair on the GPU."""
import functools

import numpy as np
import pytest
import torch

import ip_segment_cases as IC
from ip_multi_ref import attention
from util import TOL, WORST, rel_l2, to_np64, worst

DTYPES = [torch.float16, torch.bfloat16]
DIMS = [40, 64, 80, 160]
N, S, HEADS = 2, 160, 2
ids_dt = lambda d: str(d).split(".")[-1]  # noqa: E731


@functools.lru_cache(maxsize=None)
def _case(kind, dtype, d, t):
    return IC.score_case(kind, dtype, d, N, S, t, HEADS, seed=7 * d + t)


def test_the_lists():
    assert IC.KEY_COUNTS == list(range(1, 73)) + [95, 96, 97, 127, 128, 129, 257]
    assert IC.ROW_COUNTS == [1, 31, 32, 33, 127, 128, 129, 160, 257, 300]


@pytest.mark.parametrize("t", [33, 70, 257])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
def test_case_layout(dtype, d, t):
    """Shapes, dtype, NaN pad columns of V^T, the overwritten channel, and |k| within float16."""
    for kind in IC.KINDS:
        q, k, v, vt = _case(kind, dtype, d, t)
        c = HEADS * d
        assert q.shape == (N, S, c) and k.shape == (N, t, c) and v.shape == (N, t, c) and vt.shape == (N, c, IC.round_up(t, 8))
        assert {x.dtype for x in (q, k, v, vt)} == {dtype}
        assert torch.equal(vt[:, :, :t], v.transpose(1, 2)) and torch.isnan(vt[:, :, t:]).all()
        assert torch.isfinite(q).all() and torch.isfinite(k).all() and k.abs().max() <= 1216
        if kind != "random":
            assert torch.equal(q.view(N, S, HEADS, d)[0, :, 1, 0], IC.row_levels(S).to(dtype))
            assert torch.equal(k.view(N, t, HEADS, d)[1, :, 0, 0], IC.key_levels(kind, d, t).to(dtype))
    assert torch.equal(_case("steps", dtype, d, t)[0], _case("level", dtype, d, t)[0])       # one q for every levelled kind of a seed


def _sorts(tm):
    """Per (frame, head): number of rows whose tile maxima strictly rise / strictly fall over the tiles of ``tm``, and whether an
    aligned 32-row block holds a row of each sort."""
    rise, fall = (np.diff(tm, axis=-1) > 0).all(-1), (np.diff(tm, axis=-1) < 0).all(-1)
    mixed = np.stack([rise[..., r:r + 32].any(-1) & fall[..., r:r + 32].any(-1) for r in range(0, S, 32)], -1).any(-1)
    return rise.sum(-1), fall.sum(-1), mixed


@pytest.mark.parametrize("kind,t", [("steps", 33), ("steps", 70), ("steps", 257), ("ramp", 70), ("ramp", 257)])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
def test_the_running_maximum_moves(dtype, d, kind, t):
    """Per (frame, head): the rows whose per-tile maxima strictly rise over all tiles and the rows whose maxima strictly fall are each
    at least s / 4, and some aligned 32-row block holds both.  A last tile of ONE key (t = 33, 257) is lifted over the 32 keys before
    it by the 12 b step of "steps", not by the 0.25 b step of "ramp" (about 37 of 160 rows, measured): "ramp" is therefore checked at
    t = 70 over all its tiles and at t = 257 over its eight whole tiles, and not at t = 33."""
    q, k, _, _ = _case(kind, dtype, d, t)
    tm = IC.tile_maxima(q, k, HEADS)
    assert tm.shape[-1] == (t + 31) // 32
    if kind == "ramp" and t % 32 == 1:
        tm = tm[..., :-1]
    rise, fall, mixed = _sorts(tm)
    print(f"{kind} {ids_dt(dtype)} d{d} t{t}: rising rows {rise.min()} .. {rise.max()}, falling {fall.min()} .. {fall.max()} of {S}")
    assert rise.min() >= S / 4 and fall.min() >= S / 4
    assert mixed.all()


FIGURES = {}


@pytest.mark.parametrize("kind", IC.KINDS)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
def test_emulation_of_the_kernel_meets_the_bounds(dtype, d, kind):
    for t in (33, 70, 257):
        q, k, v, _ = _case(kind, dtype, d, t)
        got = to_np64(IC.emulate(q, k, v, HEADS, dtype))
        ref = attention(to_np64(q), to_np64(k), to_np64(v), HEADS)
        r, w = rel_l2(got, ref), worst(got, ref)
        key = (kind, ids_dt(dtype))
        FIGURES[key] = tuple(max(a, b) for a, b in zip(FIGURES.get(key, (0.0, 0.0)), (r, w)))
        print(f"{kind} {ids_dt(dtype)} d{d} t{t}: rel-L2 {r:.2e} worst {w:.2e}   (largest so far for {key}: "
              f"{FIGURES[key][0]:.2e} / {FIGURES[key][1]:.2e})")
        assert np.isfinite(got).all()
        assert r < TOL[dtype], (kind, t, r)
        assert w < WORST[dtype], (kind, t, w)


def test_emulation_is_the_plain_softmax_for_one_tile():
    """t <= 32: one tile, no rescale — the emulation is softmax with P rounded once."""
    q, k, v, _ = IC.score_case("random", torch.float16, 40, 1, 33, 20, 2, seed=3)
    got = to_np64(IC.emulate(q, k, v, 2, torch.float16))
    assert rel_l2(got, attention(to_np64(q), to_np64(k), to_np64(v), 2)) < TOL[torch.float16]
