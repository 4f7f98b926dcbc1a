"""GPU: the ping-pong attention kernel (csrc/aid_attn_pp.hip) with both products as v_mfma_f32_16x16x32.  A wave's 32 query rows are two
16-row blocks, a lane serves one row of each, and a row's keys are spread over four lane groups: the key-row map of the K fragments, the
P hand-over, the row state per block and the cross-group row operations are what these cases aim at.

selection / uniform  inputs whose result is known EXACTLY (tests/attn_pp_mfma16_cases.py; the CPU test of the fp64 oracle on the same
                     inputs is in tests/test_attn_pp_mfma16_layout.py): a wrong key row, a key dropped from or doubled in a product or a
                     row sum changes the rounded output.  The selection scores exceed the head-room of both storage types: raise() runs.
late maximum         the row maximum at every key position of tiles 1 and 2.
row counts           block, wave and workgroup seams, with a sentinel around the output.
modes                park / swap with two rows per lane; the output-side arguments.
walk                 item boundaries with the Q rows read back from LDS in the new fragment order."""
import numpy as np
import pytest
import torch

import attn_pp_mfma16_cases as cases
from guarded import Guarded
from oracle import aid_oracle as O
from util import TOL, WORST, rel_l2, to_np64, worst

pytestmark = pytest.mark.gpu

import aid_amd  # noqa: E402,F401
from aid_amd import ops  # noqa: E402

DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
ids_dt = lambda d: str(d).split(".")[-1]  # noqa: E731


def _dev(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(DEV)


def _vt(v, dtype):
    return _dev(v.transpose(0, 2, 1), dtype)


def _check(got, ref, dtype, what=""):
    got = to_np64(got)
    assert np.isfinite(got).all(), what
    assert rel_l2(got, ref) < TOL[dtype], (what, rel_l2(got, ref))
    assert worst(got, ref) < WORST[dtype], (what, worst(got, ref))


def _core(q64, k64, v64, heads, mode="plain", fused=False, coef=None):
    out = np.zeros_like(q64)
    for h in range(heads):
        sl = slice(64 * h, 64 * h + 64)
        out[:, :, sl] = O.attn_core(q64[:, :, sl], k64[:, :, sl], v64[:, :, sl], 1, 64 ** -0.5, mode, fused, coef)
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("l,heads", [(128, 1), (192, 2)], ids=["l128h1", "l192h2"])
def test_selection_returns_the_target_value_row_bit_for_bit(l, heads, dtype, tuning):
    q, k, v, target = cases.selection(l, heads)
    tuning("ATTN_V2", 1)
    o = ops.attn_fwd(_dev(q, dtype), _dev(k, dtype), _vt(v, dtype), heads, l=l, mode="plain")
    assert ops.last_attn_variant() == "aid_attn_pp<d64>"
    want = cases.selection_expected(v, target, heads)
    got = to_np64(o)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:8].tolist())


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("l,heads", [(128, 1), (192, 2)], ids=["l128h1", "l192h2"])
def test_uniform_weights_count_every_key_once(l, heads, dtype, tuning):
    q, k, v = cases.uniform(l, heads)
    tuning("ATTN_V2", 1)
    o = ops.attn_fwd(_dev(q, dtype), _dev(k, dtype), _vt(v, dtype), heads, l=l, mode="plain")
    assert ops.last_attn_variant() == "aid_attn_pp<d64>"
    got = to_np64(o)
    bad = np.argwhere(got != 1.0)
    assert bad.size == 0, (len(bad), bad[:8].tolist(), got[tuple(bad[0])] if len(bad) else None)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
def test_late_maximum_at_every_key_position(dtype, tuning):
    """Row r's maximum is key 64 + r: every position of tile 1 (rows 0 .. 63) and of tile 2 (rows 64 .. 127); 3 |q|^2 / 8 = 24 (natural)
    = 35 (log2) above the field, beyond f16's head-room."""
    l, s, heads = 192, 128, 2
    g = torch.Generator().manual_seed(7)
    q = torch.randn(2, s, heads * 64, generator=g).to(dtype)
    k = torch.randn(2, l, heads * 64, generator=g).to(dtype)
    k[:, 64:] = (3 * q.float()).to(dtype)
    v = torch.randn(2, l, heads * 64, generator=g).to(dtype)
    tuning("ATTN_V2", 1)
    qd, kd, vtd = q.to(DEV), k.to(DEV), v.transpose(1, 2).contiguous().to(DEV)
    o = ops.attn_fwd(qd, kd, vtd, heads, l=l, mode="plain")
    assert ops.last_attn_variant() == "aid_attn_pp<d64>"
    _check(o, _core(to_np64(q), to_np64(k), to_np64(v), heads), dtype)
    assert torch.equal(o, ops.attn_fwd(qd, kd, vtd, heads, l=l, mode="plain"))


_rc = {}


def _row_count_inputs(dtype):
    if dtype not in _rc:
        g = torch.Generator().manual_seed(11)
        n, smax, l, heads = 3, 257, 128, 2
        q = torch.randn(n, smax, heads * 64, generator=g).to(dtype)
        k = torch.randn(n, l, heads * 64, generator=g).to(dtype)
        v = torch.randn(n, l, heads * 64, generator=g).to(dtype)
        plain = _core(to_np64(q), to_np64(k), to_np64(v), heads)
        coef = np.array([0.0, 1.0, -1.0])                       # two end-point frames and a rider: own keys only in a fused call
        _rc[dtype] = (q, k.to(DEV), v.transpose(1, 2).contiguous().to(DEV), plain, torch.tensor(coef, dtype=torch.float32, device=DEV))
    return _rc[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("s", [1, 15, 16, 17, 31, 32, 33, 97, 255, 257])
def test_row_counts_at_block_wave_and_workgroup_seams(s, dtype, tuning):
    """PLAIN, and a fused OUTER call of two end-point frames and a PLAIN rider (every frame attends over its own keys: the same
    expectation) — l = 128 is no whole trip, so the OUTER call is split and the ping-pong kernel runs its single-segment frames, which
    here are all of them.  The output sits between sentinel bands; frames are adjacent, so a row stored past s lands in the next frame."""
    heads, l = 2, 128
    q, kd, vtd, plain, coef = _row_count_inputs(dtype)
    qd = q[:, :s].contiguous().to(DEV)
    tuning("ATTN_V2", 1)
    for mode in ("plain", "outer"):
        out = Guarded(3, s, heads * 64, dtype, DEV, kind="output")
        kw = dict(mode="plain") if mode == "plain" else dict(mode="outer", fused=True, coef=coef, begin=0, end=1, n_plain=1)
        ops.attn_fwd(qd, kd, vtd, heads, l=l, out=out.view, **kw)
        torch.cuda.synchronize()
        if mode == "plain":
            assert ops.last_attn_variant() == "aid_attn_pp<d64>"
        else:
            assert ops.last_attn_variant().startswith("aid_attn")
        assert out.untouched(out.layout.region_mask()) == ""
        _check(out.view, plain[:, :s], dtype, mode)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("mode,fused", [("outer", True), ("outer", False), ("inner", True), ("inner", False), ("plain", False)],
                         ids=["outer-fused", "outer-pure", "inner-fused", "inner-pure", "plain-kvmap"])
def test_modes_with_two_rows_per_lane(mode, fused, dtype, tuning):
    """l = 512 (whole trips: the ping-pong kernel runs the call alone), s = 300, 5 AID frames with coefficients 0, 1 and interior values
    + 2 riders (negative coefficient); accumulate, frame_scale, out_scale and q_prescaled = False; PLAIN with a key-row map."""
    l, s, heads, n_aid, n = 512, 300, 2, 5, 7
    g = torch.Generator().manual_seed(13)
    q = torch.randn(n, s, heads * 64, generator=g).to(dtype)
    k = torch.randn(n, l, heads * 64, generator=g).to(dtype)
    v = torch.randn(n, l, heads * 64, generator=g).to(dtype)
    base = torch.randn(n, s, heads * 64, generator=g).to(dtype)
    fs = 0.5 + torch.arange(n, dtype=torch.float32) / 4
    cf = torch.tensor([0.0, 0.25, 0.5, 0.8125, 1.0])
    q64, k64, v64 = to_np64(q), to_np64(k), to_np64(v)
    tuning("ATTN_V2", 1)
    out = base.clone().to(DEV)
    common = dict(l=l, out=out, accumulate=True, out_scale=0.7, frame_scale=fs.to(DEV), q_prescaled=False)
    qd, kd, vtd = q.to(DEV), k.to(DEV), v.transpose(1, 2).contiguous().to(DEV)
    if mode == "plain":
        kv_map = torch.tensor([(3 * f + 2) % n for f in range(n)], dtype=torch.int32)
        ops.attn_fwd(qd, kd, vtd, heads, mode="plain", kv_map=kv_map.to(DEV), **common)
        assert ops.last_attn_variant() == "aid_attn_pp<d64>"
        ref = _core(q64, k64[kv_map.long().numpy()], v64[kv_map.long().numpy()], heads)
    else:
        coef = torch.cat([cf, -torch.ones(n - n_aid)])
        ops.attn_fwd(qd, kd, vtd, heads, mode=mode, fused=fused, coef=coef.to(DEV), begin=0, end=n_aid - 1, n_plain=n - n_aid, **common)
        assert ops.last_attn_variant() == f"aid_attn_pp<d64,{mode}>"
        ref = np.concatenate([_core(q64[:n_aid], k64[:n_aid], v64[:n_aid], heads, mode, fused, cf.numpy()),
                              _core(q64[n_aid:], k64[n_aid:], v64[n_aid:], heads)])
    ref = to_np64(base) + 0.7 * to_np64(fs)[:, None, None] * ref
    _check(out, ref, dtype, (mode, fused))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
def test_persistent_walk_reads_the_next_q_rows_back_in_fragment_order(dtype, tuning):
    """20 heads x 14 frames x one q block = 280 items on at most 256 persistent workgroups: some walk two items, the second with Q rows
    that went through LDS.  Sampled rows against the oracle."""
    heads, n, s, l = 20, 14, 256, 512
    if torch.cuda.get_device_properties(0).multi_processor_count >= heads * n:
        pytest.skip("more CUs than items: no workgroup walks two")
    g = torch.Generator(device=DEV).manual_seed(17)
    q = torch.randn(n, s, heads * 64, generator=g, device=DEV).to(dtype)
    k = torch.randn(n, l, heads * 64, generator=g, device=DEV).to(dtype)
    vt = torch.randn(n, heads * 64, l, generator=g, device=DEV).to(dtype)
    tuning("ATTN_V2", 1)
    tuning("ATTN_PIPE", 1)
    o = ops.attn_fwd(q, k, vt, heads, l=l, mode="plain")
    assert ops.last_attn_variant() == "aid_attn_pp<d64>"
    rows = torch.tensor([0, 15, 16, 31, 32, 47, 255], device=DEV)
    for hh in (0, 7, heads - 1):
        sl = slice(hh * 64, hh * 64 + 64)
        ref = O.attn_core(to_np64(q[:, rows][:, :, sl]), to_np64(k[:, :, sl]), to_np64(vt[:, sl, :].transpose(1, 2)), 1, 64 ** -0.5,
                          "plain", False, None)
        _check(o[:, rows][:, :, sl], ref, dtype, hh)
