"""CPU: the replay-form cases and reference of tests/replay_rows.py.

(1) ``attn_ref`` on the replay form equals ``oracle.aid_oracle.attn_core`` on the classic full batch (the oracle that carries the
goldens); (2) the algebra of the swapped (R5) and the begin == end (R6) cases; (3) the sensitivity argument of the GPU tests: on the
very inputs they use, a result computed with begin / end exchanged, or with the classic convention (rows 0 and n - 1 of the batch as
end points), is at least ten bf16 tolerances away from the right one in EVERY frame — a wrongly addressed result cannot pass the
oracle check, and no kernel has to be made wrong to show it."""
import numpy as np
import pytest
import torch

import replay_rows as R
from oracle import aid_oracle as O
from util import TOL, rel_l2

ids_dt = lambda d: str(d).split(".")[-1]  # noqa: E731
MIS_ADDRESSED = 10 * TOL[torch.bfloat16]             # 0.08 rel-L2 per frame


@pytest.mark.parametrize("set_name", ["R1", "R3", "R4"])
@pytest.mark.parametrize("mode,fused", R.AID_MODES, ids=R.ids_mode)
def test_replay_reference_equals_the_oracle_on_the_classic_batch(mode, fused, set_name):
    batch, form, coef = R.case_inputs("nw4", torch.bfloat16, R.S, set_name)
    n, riders, d = batch["n"], batch["riders"], batch["d"]
    got = R.attn_ref(*R.np64(form), R.H, mode, fused, coef, form["begin"], form["end"])
    q, k, v = R.np64(batch)
    aid = slice(0, n + 2)
    ref = O.attn_core(q[aid], k[aid], v[aid], R.H, d ** -0.5, mode, fused, np.asarray(R.classic_coef(coef)[:n + 2]), 0, n + 1)
    for i in range(n):
        assert rel_l2(got[i], ref[1 + i]) < 1e-12, (i, rel_l2(got[i], ref[1 + i]))
    if riders:
        rd = slice(n + 2, n + 2 + riders)
        plain = O.attn_core(q[rd], k[rd], v[rd], R.H, d ** -0.5, "plain", False, None)
        for i in range(riders):
            assert rel_l2(got[n + i], plain[i]) < 1e-12, ("rider", i)


@pytest.mark.parametrize("mode,fused", R.AID_MODES, ids=R.ids_mode)
def test_swapped_and_equal_end_points(mode, fused):
    """R5: exchanging begin and end equals the unswapped call with 1 - c.  R6 (begin == end): the interpolation between a row and
    itself is that row for any c — plain attention over [own ; row] when fused, over row when pure."""
    _, form, coef = R.case_inputs("nw4", torch.bfloat16, R.S, "R1")
    _, swapped, _ = R.case_inputs("nw4", torch.bfloat16, R.S, "R5")
    _, same, _ = R.case_inputs("nw4", torch.bfloat16, R.S, "R6")
    assert (swapped["begin"], swapped["end"]) == (form["end"], form["begin"]) and same["begin"] == same["end"] == form["begin"]
    q, k, v = R.np64(form)
    a = R.attn_ref(q, k, v, R.H, mode, fused, coef, swapped["begin"], swapped["end"])
    b = R.attn_ref(q, k, v, R.H, mode, fused, [1.0 - c for c in coef], form["begin"], form["end"])
    assert rel_l2(a, b) < 1e-12
    row = same["begin"]
    scale = form["d"] ** -0.5
    for c in (coef, [0.9, 0.0, 1.0]):
        got = R.attn_ref(q, k, v, R.H, mode, fused, c, row, row)
        for i in range(form["n"]):
            kk, vv = (np.concatenate([k[i], k[row]]), np.concatenate([v[i], v[row]])) if fused else (k[row], v[row])
            assert rel_l2(got[i], R.sdpa(q[i], kk, vv, R.H, scale)) < 1e-12, (i, c)


def test_replay_form_moves_rows_and_keeps_bits():
    batch, form, _ = R.case_inputs("textkey", torch.float16, R.S, "R4")
    n, riders = batch["n"], batch["riders"]
    assert (n, riders) == (2, 2) and form["begin"] == 4 and form["end"] == 5
    assert form["q"].shape[0] == n + riders and form["k"].shape[0] == form["vt"].shape[0] == n + riders + 2
    assert form["q_rows"] == [1, 2, 4, 5] and form["kv_rows"] == [1, 2, 4, 5, 0, 3]
    for i, r in enumerate(form["kv_rows"]):
        assert torch.equal(form["k"][i], batch["k"][r]) and torch.equal(form["vt"][i], batch["vt"][r])
    for i, r in enumerate(form["q_rows"]):
        assert torch.equal(form["q"][i], batch["q"][r])
    l = batch["l"]
    assert form["vt"].shape[2] == R.round_up(l, 8) and not form["vt"][:, :, l:].any()
    assert torch.equal(form["vt"][:, :, :l], form["v"].transpose(1, 2))


ENGINE_DTYPES = [pytest.param(e, dt, id=f"{e}-{ids_dt(dt)}") for e in R.ENGINES for dt in R.engine_dtypes(e)]


@pytest.mark.parametrize("mode,fused", R.AID_MODES, ids=R.ids_mode)
@pytest.mark.parametrize("engine,dtype", ENGINE_DTYPES)
def test_a_wrongly_addressed_result_cannot_pass(engine, dtype, mode, fused):
    """A condition on the inputs of the GPU tests, not a measurement of any kernel: for every engine shape, mode and frame of R1 the
    fp64 result with begin / end exchanged, and the one with the classic convention (end points = rows 0 and n - 1 of the batch),
    differ from the right one by at least 10 x TOL[bfloat16] rel-L2.  (Smallest distance over all cases: 0.22 — fused OUTER, the
    frame at c = 0.4 with begin / end exchanged.)"""
    _, form, coef = R.case_inputs(engine, dtype, R.S, "R1")
    q, k, v = R.np64(form)
    n = form["n"]
    right = R.attn_ref(q, k, v, R.H, mode, fused, coef, form["begin"], form["end"])
    exchanged = R.attn_ref(q, k, v, R.H, mode, fused, coef, form["end"], form["begin"])
    classic = R.attn_ref(q, k, v, R.H, mode, fused, coef, 0, n - 1)
    for i in range(n):
        for what, wrong in (("exchanged", exchanged), ("classic", classic)):
            dist = rel_l2(wrong[i], right[i])
            assert dist >= MIS_ADDRESSED, (what, i, dist)
