"""The references of the float32 attention sweeps, without a GPU: on the very inputs tests/test_hip_f32_attn_key_counts.py feeds
the kernels (tests/f32_attn_key_counts.py), the CPU restatement of the three-term split (split_attn_ref.refs: ``ref3``) stays inside the
project's bounds for "high" and a plain float32 evaluation of the same attention inside the bounds of the exact kernel, both against
fp64 — so a GPU failure at one of these key counts means the kernel, not the bound.  The late-maximum inputs are also shown to do
what they are for: in each of tiles 1 and 2 at least 10 % of the (frame, head, row) triples raise their running maximum, and the median
largest softmax weight of a row is below 0.5 (the other keys still matter).

Measured (largest rel-L2 / worst over every key count of KEY_COUNTS; n = 4, s = 40, h = 2):
    d      ref3 vs fp64          float32 vs fp64
    40     6.3e-6 / 6.8e-5       3.2e-7 / 5.0e-6
    64     6.2e-6 / 6.9e-5       3.7e-7 / 8.1e-6
    80     6.1e-6 / 8.9e-5       3.6e-7 / 5.6e-6
    160    6.1e-6 / 7.0e-5       4.7e-7 / 8.3e-6
Late-maximum inputs (s = l = 77, n = 3):
    d      ref3 vs fp64          float32 vs fp64       rows raising in tile 1 / tile 2    median largest weight
    40     4.5e-6 / 4.0e-5       2.8e-7 / 3.6e-6       0.48 / 0.16                        0.25
    64     4.1e-6 / 4.4e-5       3.2e-7 / 4.1e-6       0.52 / 0.18                        0.26
    80     4.0e-6 / 4.5e-5       3.6e-7 / 3.8e-6       0.50 / 0.16                        0.29
    160    4.1e-6 / 4.0e-5       4.3e-7 / 5.2e-6       0.51 / 0.17                        0.27
(The float32 figures depend on the host BLAS's summation order; the bounds leave a factor of ten.)
"""
import numpy as np
import pytest
import torch

import f32_attn_key_counts as K
from replay_rows import attn_ref
from split_attn_ref import refs
from test_hip_attn_f32x3 import TOL_F32_HIGH, WORST_F32_HIGH
from test_hip_f32 import TOL_F32, WORST_F32
from util import rel_l2, to_np64, worst


def test_the_bounds_are_the_projects():
    assert (TOL_F32, WORST_F32, TOL_F32_HIGH, WORST_F32_HIGH) == (1e-5, 1e-4, 3e-5, 3e-4)


def test_the_cases_cover_every_residue_and_seam():
    L, T = K.KEY_COUNTS, K.TILE
    assert len(set(L)) == len(L) == 79 and set(range(1, 73)) <= set(L)
    for tiles in (1, 2):                                         # every residue mod 32 on one and on two tiles
        assert {l % T for l in L if (l + T - 1) // T == tiles} == set(range(T))
    assert {l % T for l in L if (l + T - 1) // T == 3} >= {0, 1, 31} | set(range(1, 9))
    assert {1, 32, 33, 64, 65, 96, 97, 128, 129, 160} <= set(L)   # the tile seams, five tiles
    assert {l % 4 for l in L} == {0, 1, 2, 3} and {l % 8 for l in L} == set(range(8))
    assert K.L_ROWS in L and K.L_ROWS % 4 == 1 and (K.L_ROWS + T - 1) // T == 2
    S = K.ROW_COUNTS
    assert {1, 31, 32, 33, 63, 64, 65, 127, 128, 129} <= set(S) and max(S) > 256
    assert set(K.BIAS_KEY_COUNTS) <= set(L) | {77} and K.DIMS == (40, 64, 80, 160)


def _attn_f32(q, k, v):
    """Plain float32 torch evaluation: the arithmetic the exact kernel's bound allows for."""
    n, s, c = q.shape
    d = c // K.H
    heads = lambda t: t.view(n, t.shape[1], K.H, d).transpose(1, 2)  # noqa: E731
    p = torch.softmax(heads(q) @ heads(k).transpose(-1, -2) * d ** -0.5, dim=-1)
    return (p @ heads(v)).transpose(1, 2).reshape(n, s, c)


def _figures(q, k, v):
    ref3, _, ref64 = refs(q, k, v, K.H)
    assert rel_l2(K.oracle_ref(q, k, v, "plain", False, None), ref64) < 1e-12      # the GPU tests' oracle is the same fp64 attention
    f32 = to_np64(_attn_f32(q, k, v))
    return (rel_l2(ref3, ref64), worst(ref3, ref64)), (rel_l2(f32, ref64), worst(f32, ref64))


@pytest.mark.parametrize("d", K.DIMS)
def test_references_stay_inside_the_bounds_at_every_key_count(d):
    top = np.zeros(4)
    for l in K.KEY_COUNTS:
        (e3, w3), (e1, w1) = _figures(*K.sweep_inputs(d, l))
        assert e3 < TOL_F32_HIGH and w3 < WORST_F32_HIGH, (d, l, "ref3", e3, w3)
        assert e1 < TOL_F32 and w1 < WORST_F32, (d, l, "float32", e1, w1)
        top = np.maximum(top, (e3, w3, e1, w1))
    print(f"[f32_key_counts] d {d}: ref3 {top[0]:.1e} / {top[1]:.1e}   float32 {top[2]:.1e} / {top[3]:.1e}")


@pytest.mark.parametrize("d", K.DIMS)
def test_late_maximum_inputs(d):
    q, k, v = K.late_maximum_inputs(d)
    (e3, w3), (e1, w1) = _figures(q, k, v)
    assert e3 < TOL_F32_HIGH and w3 < WORST_F32_HIGH, (d, "ref3", e3, w3)
    assert e1 < TOL_F32 and w1 < WORST_F32, (d, "float32", e1, w1)
    sc = K.scores64(q, k)                                         # [n, H, s, l]
    T = K.TILE
    assert sc.shape[-1] == K.S_LATE == 2 * T + 13
    m0, m1, m2 = sc[..., :T].max(-1), sc[..., T:2 * T].max(-1), sc[..., 2 * T:].max(-1)
    r1, r2 = float((m1 > m0).mean()), float((m2 > np.maximum(m0, m1)).mean())
    p = np.exp(sc - sc.max(-1, keepdims=True))
    top = float(np.median((p / p.sum(-1, keepdims=True)).max(-1)))
    print(f"[f32_key_counts] late maximum d {d}: ref3 {e3:.1e} / {w3:.1e}   float32 {e1:.1e} / {w1:.1e}   "
          f"raising {r1:.2f} / {r2:.2f}   median largest weight {top:.2f}")
    assert r1 >= 0.10 and r2 >= 0.10, (d, r1, r2)
    assert top < 0.5, (d, top)
    # every position of the ragged last tile is some row's preferred key (in every frame and head)
    best = sc.argmax(-1)
    assert all((best == j).any() for j in range(2 * T, K.S_LATE)), d


@pytest.mark.parametrize("mode,fused", K.MODES[1:])
def test_oracle_ref_with_a_rider_is_the_frame_by_frame_reference(mode, fused):
    """oracle_ref (oracle.aid_oracle.attn_core on the interpolated frames, PLAIN on the rider) against the frame-by-frame fp64
    reference the memory-contract tests use (replay_rows.attn_ref): two restatements, one answer."""
    d, l = 40, 45
    q, k, v = K.sweep_inputs(d, l)
    c32 = np.asarray(K.COEF_SWEEP, np.float32).astype(np.float64)
    want = attn_ref(to_np64(q), to_np64(k), to_np64(v), K.H, mode, fused, c32, K.BEGIN, K.END)
    assert rel_l2(K.oracle_ref(q, k, v, mode, fused, K.COEF_SWEEP), want) < 1e-12
    if not fused:
        b = K.bias_inputs(d, l, K.S_SWEEP)
        want = attn_ref(to_np64(q), to_np64(k), to_np64(v), K.H, mode, False, c32, K.BEGIN, K.END, bias=to_np64(b))
        assert rel_l2(K.oracle_ref(q, k, v, mode, False, K.COEF_SWEEP, mask=b), want) < 1e-12
        assert float((b == -10000.0).float().mean()) > 0.25 and bool((b[..., 0] > -100).all())
