"""GPU tests of the score-bias kernels (AidAttnArgs.bias = diffusers' attention_mask) on masks that leave whole 64-key tiles without a
live key: the BIAS instantiation of aid_attn_kernel (fp16 / bf16), aid_attn_f32_kernel and aid_attn_f32x3_kernel (fp32, "highest" and
"high").  Patterns, shape and the oracle's view of each mask: tests/attn_mask_cases.py (checked on the CPU by
tests/test_oracle_attn_mask.py).

Per pattern and mode: every output element finite; the rows with a live key against the fp64 oracle on the same rounded inputs
(relative L2 over THOSE rows, so a wrong 32-row block cannot hide behind right ones); rows without a live key a convex combination
of their head's values (and, with -10000, equal to the oracle's: softmax is shift invariant; with finfo.min / -inf the reference's own
answer is uniform weights / NaN, so they are the only rows left out); a second launch gives the same bits.

Measured on an MI355X, largest figure over d, the three mask values and the three modes (rel-L2 / worst):
    pattern A   fp16 3.5e-4 / 3.8e-3   bf16 2.8e-3 / 2.8e-2   fp32 4.5e-7 / 7.5e-6   fp32 "high" 6.0e-6 / 6.6e-5
    pattern B   fp16 3.2e-4 / 2.6e-3   bf16 2.6e-3 / 2.4e-2   fp32 3.4e-7 / 3.8e-6   fp32 "high" 5.5e-6 / 6.1e-5
Before the references of a row were kept as (largest bias) + (rest), patterns A, B, E, F and G gave NaN rows in fp16 / bf16 for all
three values (d = 64 PLAIN: finite, and wrong by 0.3 - 0.7 of the norm with finfo.min / -inf), and the -10000 rows of pattern G missed
the fp32 bound (4e-5 / 6e-4) in both fp32 kernels."""
import functools

import numpy as np
import pytest
import torch

import attn_mask_cases as M
from util import TOL, WORST, rel_l2, to_np64, worst

pytestmark = pytest.mark.gpu

from aid_amd import ops  # noqa: E402

DEV = "cuda:0"
F32 = torch.float32
TOL_F32, WORST_F32 = 1e-5, 1e-4                 # tests/test_hip_f32.py
ids_dt = lambda d: str(d).split(".")[-1]  # noqa: E731


@functools.lru_cache(maxsize=None)
def _inputs(dtype, d):
    g = torch.Generator().manual_seed(150 + d)
    c = M.H * d
    q = torch.randn(M.N, M.S, c, generator=g).to(dtype)
    k = torch.randn(M.N, M.L, c, generator=g).to(dtype)
    v = torch.randn(M.N, M.L, c, generator=g).to(dtype)
    vt = torch.zeros(M.N, c, (M.L + 7) // 8 * 8, dtype=dtype)
    vt[:, :, :M.L] = v.transpose(1, 2)
    return (q.to(DEV), k.to(DEV), vt.to(DEV)), (to_np64(q), to_np64(k), to_np64(v))


@functools.lru_cache(maxsize=None)
def _reference(dtype, d, pattern, mode, low):
    """fp64 oracle output, computed once per (inputs, pattern, mode, the oracle's mask value) and never written to."""
    _, (q64, k64, v64) = _inputs(dtype, d)
    ref = M.oracle_out(q64, k64, v64, d, mode, M.oracle_mask(M.keep_of(pattern), "m10000" if low == -10000.0 else "neg_inf"))
    ref.setflags(write=False)
    return ref


def _value_range(v64, d, mode):
    """[N, 1, H d] bounds of a convex combination of the value rows a frame's softmaxes average: its own (PLAIN frames), the two end
    points' (frames 0 .. 2 of an INNER / OUTER launch)."""
    lo, hi = v64.min(axis=1, keepdims=True), v64.max(axis=1, keepdims=True)
    if mode != "plain":
        lo[:3], hi[:3] = np.minimum(lo[0], lo[2]), np.maximum(hi[0], hi[2])
    return lo, hi


def _ulp_at(x, dtype):
    return torch.finfo(dtype).eps * 2.0 ** np.floor(np.log2(x))


def _single_key_rows(v64, mode):
    """Pattern F: the only live key is the last, so every softmax is that key's value row."""
    last = v64[:, M.L - 1]
    want = last.copy()
    if mode != "plain":
        c = np.asarray(M.COEF[:3])[:, None]
        want[:3] = (1 - c) * last[0] + c * last[2]
    return np.broadcast_to(want[:, None], (M.N, M.S, want.shape[-1]))


@pytest.mark.parametrize("value", M.VALUES)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, F32], ids=ids_dt)
@pytest.mark.parametrize("d", [40, 64, 80, 160])
def test_fully_masked_key_tiles(d, dtype, value):
    (q, k, vt), (q64, k64, v64) = _inputs(dtype, d)
    coef = torch.tensor(M.COEF).to(DEV)
    tol, wtol = (TOL_F32, WORST_F32) if dtype == F32 else (TOL[dtype], WORST[dtype])
    vmax = np.abs(v64).max()
    margin = 1e-5 * vmax if dtype == F32 else 2 * _ulp_at(vmax, dtype)
    low = -10000.0 if value == "m10000" else -1e30
    for precision in (("highest", "high") if dtype == F32 else (None,)):
        for pattern in M.PATTERNS:
            keep = M.keep_of(pattern)
            live = M.live_rows(keep)
            bias = M.additive(keep, value, dtype).to(DEV)
            for mode in M.MODES:
                kw = dict(l=M.L, mode=mode, fused=False, coef=None if mode == "plain" else coef, begin=0, end=2,
                          n_plain=0 if mode == "plain" else 1, bias=bias, f32_attn_precision=precision)
                o = ops.attn_fwd(q, k, vt, M.H, **kw)
                name = ops.last_attn_variant()
                what = (pattern, mode, value, name)
                if dtype == F32:
                    assert name == ("aid_attn_f32x3" if precision == "high" else "aid_attn_f32"), what
                else:
                    assert "bias" in name, what
                got = to_np64(o)
                assert np.isfinite(got).all(), (what, "rows with NaN / inf", np.unique(np.nonzero(~np.isfinite(got))[1])[:8])
                # rows that have a reference: every live row; with -10000 the fully masked rows too
                rows = live if low != -10000.0 else np.ones_like(live)
                assert 4 * (~rows).sum() <= rows.size
                ref = _reference(dtype, d, pattern, mode, low)
                e, w = rel_l2(got[rows], ref[rows]), worst(got[rows], ref[rows])
                print(f"[mask_range] {ids_dt(dtype)} d{d} {value} {pattern} {mode} {name}: rel-L2 {e:.2e} worst {w:.2e}")
                assert e < tol and w < wtol, (what, e, w)
                if pattern == "F":
                    want = _single_key_rows(v64, mode)
                    assert rel_l2(got, want) < tol and worst(got, want) < wtol, (what, rel_l2(got, want), worst(got, want))
                if not live.all():              # fully masked rows: a convex combination of their head's values
                    lo, hi = _value_range(v64, d, mode)
                    dead = got[~live]
                    lo_r = np.broadcast_to(lo, got.shape)[~live]
                    hi_r = np.broadcast_to(hi, got.shape)[~live]
                    assert (dead >= lo_r - margin).all() and (dead <= hi_r + margin).all(), \
                        (what, float((lo_r - dead).max()), float((dead - hi_r).max()), margin)
                assert torch.equal(ops.attn_fwd(q, k, vt, M.H, **kw), o), (what, "second launch differs")
