"""GPU sweeps of the two float32 attention kernels — aid_attn_f32_kernel (exact, csrc/aid_f32.hip) and aid_attn_f32x3_kernel ("high":
three-term bf16 split, csrc/aid_f32x3.hip) — over every key count, row count and late-maximum position at which they take another
path.  Cases and inputs: tests/f32_attn_key_counts.py (the CPU test tests/test_f32_attn_key_counts.py shows that the references alone
stay inside the bounds on these inputs).

Both kernels walk 32-key tiles; what the sweeps reach that the few key counts of test_hip_f32.py / test_hip_attn_f32x3.py do not:
every valid-key count of the ragged last tile on one, two and three tiles (the masks through key_of / key_of_x3, the split kernel's
K rows stored with bits 2 and 3 of the key index exchanged), the element-wise tail of a V^T row at every l % 4 (per 4-key half of an
8-key chunk in the split kernel), the ragged tile in the MIDDLE of the key stream of a fused call (with the next segment's first tile
in flight across it for d <= 80, single-buffered for d = 160), the pad channels of d = 40 / 80, the bias clamp of the ragged tile, every
wave and workgroup seam of the query rows, and the rescale branch with the new maximum at every position of every tile.

Every comparison is against oracle.aid_oracle.attn_core in fp64 on the same float32 inputs, over EVERY output element, at the
project's bounds (exact: TOL_F32 / WORST_F32 of test_hip_f32.py; "high": TOL_F32_HIGH / WORST_F32_HIGH of test_hip_attn_f32x3.py).  The
kernel is forced (f32_split / f32_attn_precision) and its name asserted after every call.

Measured on an MI355X, largest rel-L2 / worst over all cases of the test:
                                    d = 40              d = 64              d = 80              d = 160
    (a) every key count    exact    3.6e-7 / 5.0e-6     4.0e-7 / 6.7e-6     4.1e-7 / 7.1e-6     5.1e-7 / 8.1e-6
                           high     6.3e-6 / 7.3e-5     6.1e-6 / 7.7e-5     6.0e-6 / 9.7e-5     6.0e-6 / 7.7e-5
    (b) every row count    exact    2.6e-7 / 4.5e-6     2.8e-7 / 4.1e-6     5.6e-7 / 4.3e-6     5.7e-7 / 5.6e-6
                           high     6.1e-6 / 9.0e-5     6.0e-6 / 9.6e-5     5.9e-6 / 6.3e-5     5.6e-6 / 7.0e-5
    (c) late maximum       exact    3.3e-7 / 3.7e-6     3.8e-7 / 5.9e-6     3.8e-7 / 5.2e-6     5.1e-7 / 8.6e-6
                           high     4.6e-6 / 4.3e-5     4.2e-6 / 4.6e-5     4.1e-6 / 5.1e-5     4.2e-6 / 4.5e-5
    (d) score bias         exact    2.5e-7 / 3.5e-6     2.7e-7 / 3.7e-6     3.0e-7 / 4.2e-6     3.7e-7 / 6.1e-6
                           high     5.7e-6 / 6.3e-5     5.5e-6 / 7.0e-5     5.6e-6 / 5.6e-5     5.5e-6 / 5.0e-5
    (e) softmax_scale,     exact    2.5e-7 / 2.1e-6     2.7e-7 / 3.6e-6     3.3e-7 / 4.5e-6     3.6e-7 / 4.0e-6
        q_prescaled        high     5.7e-6 / 5.0e-5     5.6e-6 / 4.0e-5     5.5e-6 / 3.5e-5     5.6e-6 / 4.6e-5
The "high" figures are those of the CPU restatement on the same inputs (6.1e-6 - 6.3e-6 / 6.8e-5 - 8.9e-5 over the key counts).  Each
parametrised case runs 1 - 2 s (a) and 0.01 - 0.2 s (b - e).

A test collects its failures and reports all of them, so a wrong tail names every key count it breaks.  Shown to fail on scratch
builds (never committed): masking the split kernel with the exact kernel's key map, storing its K rows without the bit swap, taking a
V^T row's last chunk as a vector when its fourth element is column l, and not resetting the key offset for the second segment.
"""
import numpy as np
import pytest
import torch

import f32_attn_key_counts as K
import test_hip_memory_contracts as M
from guarded import Guarded
from test_hip_attn_f32x3 import TOL_F32_HIGH, WORST_F32_HIGH
from test_hip_f32 import TOL_F32, WORST_F32
from util import rel_l2, to_np64, worst

pytestmark = pytest.mark.gpu

from aid_amd import ops  # noqa: E402

DEV = "cuda:0"
F32 = torch.float32
# kernel id -> (AidAttnArgs.f32_split, f32_attn_precision, the name the launch must report, rel-L2 bound, worst bound)
KERNELS = {"exact": (0, "highest", "aid_attn_f32", TOL_F32, WORST_F32),
           "high": (1, "high", "aid_attn_f32x3", TOL_F32_HIGH, WORST_F32_HIGH)}
kernel_and_dim = lambda f: pytest.mark.parametrize("kernel", list(KERNELS))(pytest.mark.parametrize("d", K.DIMS)(f))  # noqa: E731


class Sweep:
    """Collects the failures of one test (so that a run names EVERY key count that fails, not the first) and its largest figures."""

    def __init__(self, test, kernel, d):
        self.test, self.kernel, self.d = test, kernel, d
        _, _, self.name, self.tol, self.wst = KERNELS[kernel]
        self.bad, self.top = [], np.zeros(2)

    def parity(self, got, ref, name, **what):
        """``got`` [n, s, c] against the fp64 ``ref``: the kernel's name, a finite result, rel-L2 and worst inside the bounds."""
        got = to_np64(got)
        e, w = rel_l2(got, ref), worst(got, ref)
        where = dict(d=self.d, **what, kernel=self.kernel, rel_l2=float("%.2e" % e), worst=float("%.2e" % w))
        if name != self.name:
            self.bad.append(dict(where, ran=name))
        elif not np.isfinite(got).all():
            self.bad.append(dict(where, finite=False))
        elif not (e < self.tol and w < self.wst):
            self.bad.append(where)
        else:
            self.top = np.maximum(self.top, (e, w))

    def contract(self, msgs, **what):
        self.bad += [dict(d=self.d, **what, kernel=self.kernel, memory=m) for m in msgs if m]

    def done(self):
        print(f"[f32_key_counts] {self.test} {self.kernel} d {self.d}: rel-L2 {self.top[0]:.1e}  worst {self.top[1]:.1e}")
        ls = sorted({b["l"] for b in self.bad if "l" in b})
        modes = sorted({(b["mode"], b["fused"]) for b in self.bad})
        assert not self.bad, f"{len(self.bad)} failure(s), key counts {ls}, modes {modes}:\n" + "\n".join(map(str, self.bad[:12]))


def _call(d, l, s):
    """The sweep's inputs in the guarded buffers of the memory-contract tests: strided rows, NaN in every gap, in the gap row behind
    each frame and in the V^T pad columns, the sentinel around ``out`` (ldo = c + 4)."""
    q, k, v = K.sweep_inputs(d, l, s)
    call = M.AttnCall(F32, K.N_SWEEP, s, l, K.H, d, 4, seed=0)
    call.Q.set(q)
    call.K.set(k)
    call.VT.set(v.transpose(1, 2))
    call.q64, call.k64, call.v64 = to_np64(q), to_np64(k), to_np64(v)
    return call, (q, k, v)


def _launch(sw, call, qkv, mode, fused, k2=None, vt2=None, bias=None, mask=None, **what):
    """One launch of the sweep's call (end points 0 and 2, an interior frame, a PLAIN rider): parity with the oracle, nothing written
    outside [s, c] of any frame, the inputs unchanged."""
    coef = None if mode == "plain" else list(K.COEF_SWEEP)
    kw = dict(k2=k2, vt2=vt2) if mode == "inner" else {}
    name, Og, _ = call.run(mode, fused, coef, K.BEGIN, K.END, bias=bias, f32_split=KERNELS[sw.kernel][0], **kw)
    what = dict(l=call.l, s=call.s, mode=mode, fused=fused, **what)
    sw.parity(Og.view, K.oracle_ref(*qkv, mode, fused, K.COEF_SWEEP, mask=mask), name, **what)
    sw.contract([Og.untouched(Og.layout.region_mask())] + [t.inputs_unchanged() for t in (call.Q, call.K, call.VT)], **what)
    if bias is not None:
        sw.contract([bias.inputs_unchanged()], **what)


@kernel_and_dim
def test_every_key_count(kernel, d):
    """(a) l = 1 .. 72, 95, 96, 97, 127, 128, 129, 160 at s = 40: aid_lerp_kv in float32 (its whole-stride rule: AttnCall.lerp) and all five
    modes on guarded buffers."""
    sw = Sweep("every key count", kernel, d)
    coef_t = torch.tensor(K.COEF_SWEEP, dtype=F32, device=DEV)
    for l in K.KEY_COUNTS:
        call, qkv = _call(d, l, K.S_SWEEP)
        k2, vt2 = call.lerp(coef_t, K.BEGIN, K.END)
        for mode, fused in K.MODES:
            _launch(sw, call, qkv, mode, fused, k2, vt2)
    sw.done()


@kernel_and_dim
def test_every_row_count(kernel, d):
    """(b) s = 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130, 257 at l = 45: the row clamp, the store guard and the block decomposition
    (frame, head, query block) at every wave and workgroup seam; PLAIN and fused OUTER."""
    sw = Sweep("every row count", kernel, d)
    for s in K.ROW_COUNTS:
        call, qkv = _call(d, K.L_ROWS, s)
        for mode, fused in (("plain", False), ("outer", True)):
            _launch(sw, call, qkv, mode, fused)
    sw.done()


@kernel_and_dim
def test_late_maximum_at_every_key_position(kernel, d):
    """(c) every query row prefers another key (tests/f32_attn_key_counts.py: late_maximum_inputs), so the running maximum is raised —
    and the accumulators rescaled — at every position of tiles 1 and 2 in some row, and rows that do and do not rescale share a wave.
    All five modes through ops.attn_fwd; a second launch gives the same bits."""
    sw = Sweep("late maximum", kernel, d)
    q, k, v = K.late_maximum_inputs(d)
    qd, kd, vd = q.to(DEV), k.to(DEV), K.vt_of(v).to(DEV)
    cd = torch.tensor(K.COEF_LATE, dtype=F32, device=DEV)
    for mode, fused in K.MODES:
        run = lambda: ops.attn_fwd(qd, kd, vd, K.H, l=K.S_LATE, mode=mode, fused=fused, coef=cd,            # noqa: E731
                                   f32_attn_precision=KERNELS[kernel][1])
        o = run().clone()
        name = ops.last_attn_variant()
        sw.parity(o, K.oracle_ref(q, k, v, mode, fused, K.COEF_LATE), name, l=K.S_LATE, mode=mode, fused=fused)
        again = run()
        if not (torch.equal(again, o) and ops.last_attn_variant() == name):
            sw.bad.append(dict(d=d, mode=mode, fused=fused, kernel=kernel, second_launch="other bits"))
    sw.done()


class _OneRowBias:
    """A guarded [n, 1, l] bias handed to AttnCall.run as the one-row-for-all-queries layout (bias_rs = 0)."""

    def __init__(self, g):
        self.ptr, self.fs, self.ld, self.view, self.inputs_unchanged = g.ptr, g.fs, 0, g.view, g.inputs_unchanged


@kernel_and_dim
def test_score_bias_at_ragged_key_counts(kernel, d):
    """(d) l = 1, 5, 31, 32, 33, 45, 64, 77 at s = 40: the bias of the ragged tile is read through brow[min(t0 + key, l - 1)] with the
    kernel's own key map.  One bias row per query (row stride l + 8, NaN in the gap) and one row for all queries (bias_rs = 0);
    randn * 0.5 with a random third of the keys at -10000; PLAIN, INNER and OUTER (pure), against the oracle with ``mask=``."""
    sw = Sweep("score bias", kernel, d)
    coef_t = torch.tensor(K.COEF_SWEEP, dtype=F32, device=DEV)
    for l in K.BIAS_KEY_COUNTS:
        call, qkv = _call(d, l, K.S_SWEEP)
        k2, vt2 = call.lerp(coef_t, K.BEGIN, K.END)
        per_row, one_row = K.bias_inputs(d, l, K.S_SWEEP), K.bias_inputs(d, l, 1)
        layouts = (("per row", Guarded(K.N_SWEEP, K.S_SWEEP, l, F32, DEV, ld=l + 8).set(per_row), per_row),
                   ("one row", _OneRowBias(Guarded(K.N_SWEEP, 1, l, F32, DEV, ld=l + 8, gap_rows=1).set(one_row)), one_row))
        for layout, bias, mask in layouts:
            for mode in ("plain", "inner", "outer"):
                _launch(sw, call, qkv, mode, False, k2, vt2, bias=bias, mask=mask, layout=layout)
    sw.done()


@kernel_and_dim
def test_prescaled_q_and_softmax_scale(kernel, d):
    """(e) l = 45, s = 40, PLAIN and fused OUTER through ops.attn_fwd: a non-default ``softmax_scale`` against the oracle with that
    scale; ``q_prescaled`` with q * fp32(softmax_scale * log2 e) formed in float32 on the host.

    Exact kernel: the prescaled call gives the bits of the plain call (both form the same single fp32 product per element and feed it
    to the matrix instruction).  Split kernel: not the same bits, for a reason visible in its code — split8 takes the low half as
    bf16(x - high half) with x = q * c2, and under -ffast-math the compiler contracts that into one fused multiply-add
    (v_pk_fma_f32 q, c2, -high) next to the v_pk_mul_f32 that feeds the high half: the plain call's low halves come from the UNROUNDED
    product, the prescaled call's (c2 = 1) from the fp32-rounded one the host formed.  The high halves agree; the low halves differ by
    at most an ulp of bf16 in few elements (measured: outputs up to 3.9e-6 apart, the size of the split's own error).  So for "high" the
    prescaled call is held to the oracle at the bounds instead, like every other call here."""
    sw = Sweep("softmax_scale", kernel, d)
    l, s = K.L_ROWS, K.S_SWEEP
    q, k, v = K.sweep_inputs(d, l, s)
    qd, kd, vd = q.to(DEV), k.to(DEV), K.vt_of(v).to(DEV)
    cd = torch.tensor(K.COEF_SWEEP, dtype=F32, device=DEV)
    c2 = np.float32(d ** -0.5) * np.float32(1.4426950408889634)           # the launcher's fp32 product
    assert c2.dtype == np.float32
    qp = (q * float(c2)).to(DEV)                                           # one fp32 product per element
    scale = 0.37 * d ** -0.5
    for mode, fused in (("plain", False), ("outer", True)):
        kw = dict(l=l, mode=mode, fused=fused, coef=cd, begin=K.BEGIN, end=K.END, n_plain=1, f32_attn_precision=KERNELS[kernel][1])
        o = ops.attn_fwd(qd, kd, vd, K.H, softmax_scale=scale, **kw)
        sw.parity(o, K.oracle_ref(q, k, v, mode, fused, K.COEF_SWEEP, scale=scale), ops.last_attn_variant(), l=l, mode=mode,
                  fused=fused, softmax_scale=0.37)
        o0 = ops.attn_fwd(qd, kd, vd, K.H, **kw).clone()
        sw.parity(o0, K.oracle_ref(q, k, v, mode, fused, K.COEF_SWEEP), ops.last_attn_variant(), l=l, mode=mode, fused=fused)
        o1 = ops.attn_fwd(qp, kd, vd, K.H, q_prescaled=True, **kw)
        sw.parity(o1, K.oracle_ref(q, k, v, mode, fused, K.COEF_SWEEP), ops.last_attn_variant(), l=l, mode=mode, fused=fused,
                  q_prescaled=True)
        same = torch.equal(o0, o1)
        print(f"[f32_key_counts] q_prescaled {kernel} d {d} {mode}: same bits {same}, largest difference {float((o0 - o1).abs().max()):.1e}")
        if kernel == "exact" and not same:
            sw.bad.append(dict(d=d, mode=mode, fused=fused, kernel=kernel, q_prescaled="other bits than the plain call"))
    sw.done()
