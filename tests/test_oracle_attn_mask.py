"""CPU test of what tests/test_hip_attn_mask_range.py leans on: on every query row that has a live key the fp64 oracle with an additive
mask equals a plain softmax over the live keys only (the masked columns dropped, no mask value anywhere), and each pattern has exactly
the fully masked rows it is meant to have — never more than a quarter of the rows."""
import numpy as np
import pytest
import torch

import attn_mask_cases as M

D = 40


def _inputs():
    g = torch.Generator().manual_seed(5)
    c = M.H * D
    return tuple(torch.randn(M.N, n, c, generator=g).numpy().astype(np.float64) for n in (M.S, M.L, M.L))


def _softmax_rows(x):
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def _dropped(q, k, v, mode, keep):
    """Attention over the live keys only, row by row; rows without a live key stay NaN."""
    out = np.full((M.N, M.S, M.H * D), np.nan)
    keep = np.broadcast_to(keep.numpy(), (M.N, M.S, M.L))
    for f in range(M.N):
        c = M.COEF[f]
        plain = mode == "plain" or c < 0
        for h in range(M.H):
            ch = slice(h * D, (h + 1) * D)
            for r in range(M.S):
                live = np.nonzero(keep[f, r])[0]
                if live.size == 0:
                    continue

                def att(kk, vv):
                    w = _softmax_rows((kk[live][:, ch] @ q[f, r, ch]) * D ** -0.5)
                    return w @ vv[live][:, ch]
                if plain:
                    out[f, r, ch] = att(k[f], v[f])
                elif mode == "outer":
                    out[f, r, ch] = (1 - c) * att(k[0], v[0]) + c * att(k[2], v[2])
                else:
                    out[f, r, ch] = att((1 - c) * k[0] + c * k[2], (1 - c) * v[0] + c * v[2])
    return out


@pytest.mark.parametrize("pattern", M.PATTERNS)
def test_fully_masked_row_counts(pattern):
    keep = M.keep_of(pattern)
    assert keep.shape in ((M.N, 1, M.L), (M.N, M.S, M.L))
    live = M.live_rows(keep)
    dead = (~live).sum(axis=1)
    assert (dead == M.DEAD_ROWS[pattern]).all(), dead
    assert 4 * (~live).sum() <= live.size
    # the tiles the pattern is about (64-key tiles: [0, 64), [64, 128), [128, 150))
    k3 = np.broadcast_to(keep.numpy(), (M.N, M.S, M.L))
    t0, t1, t2 = k3[..., :64].any(-1), k3[..., 64:128].any(-1), k3[..., 128:].any(-1)
    if pattern == "A":
        assert not t0.any() and k3[..., 64:].all()
    if pattern == "B":
        assert not t0.any() and not t1.any() and k3[..., 128:].all()
    if pattern == "C":
        assert k3[..., :64].all() and not t1.any() and k3[..., 128:].all()
    if pattern == "D":
        assert k3[..., :70].all() and not k3[..., 70:].any()
    if pattern == "F":
        assert k3.sum(-1).max() == 1 and k3[..., M.L - 1].all()
    if pattern in "EG":
        first = k3[0, :32]                      # one wave's rows: first tile fully masked / partly masked / untouched
        assert (~first[:, :64].any(-1) & first.any(-1)).any() and (pattern == "G" or first[:, :64].all(-1).any())
        assert (first[:, :64].any(-1) & ~first[:, :64].all(-1)).any()
        assert (live & ~t0 & ~t1 & t2).any()    # ... and rows whose only live keys sit in the ragged tile


@pytest.mark.parametrize("pattern", M.PATTERNS)
def test_oracle_with_mask_equals_softmax_over_live_keys(pattern):
    q, k, v = _inputs()
    keep = M.keep_of(pattern)
    live = M.live_rows(keep)
    masks = {}
    for value in M.VALUES:
        m64 = M.oracle_mask(keep, value)
        low = -10000.0 if value == "m10000" else -1e30
        assert m64.shape == (M.N, 1) + tuple(keep.shape[1:])
        assert ((m64[:, 0] == 0) == keep.numpy()).all() and (m64[:, 0][~keep.numpy()] == low).all()
        masks[low] = m64
        for dtype in (torch.float16, torch.bfloat16, torch.float32):     # what the kernel is handed for the same case
            caller = M.additive(keep, value, dtype)
            assert caller.dtype == dtype and ((caller == 0) == keep).all() and (caller[~keep] == M.low_of(value, dtype)).all()
    assert set(masks) == {-10000.0, -1e30}
    for mode in M.MODES:
        want = _dropped(q, k, v, mode, keep)
        assert np.isfinite(want[live]).all() and np.isnan(want[~live]).all()
        for low, m64 in masks.items():
            got = M.oracle_out(q, k, v, D, mode, m64)
            assert np.isfinite(got).all()
            np.testing.assert_allclose(got[live], want[live], rtol=1e-11, atol=1e-13, err_msg=f"{mode} {low}")
        if pattern == "F":                      # one live key: the output is that key's value row
            np.testing.assert_allclose(want[3], np.broadcast_to(v[3, M.L - 1], (M.S, M.H * D)), rtol=1e-12)
