"""GPU: item boundaries of the persistent ping-pong attention kernel (csrc/aid_attn_pp.hip).  A persistent workgroup walks several
items (256 query rows of one (frame, head)) with the tile stream, the DMA ring and the slot alternation running on across the
boundary.  At a boundary the second wave group stores the finished item, plans the item after next and requests its Q rows in FRONT
of the barrier behind its last M slot (beside the first group's boundary work), the walk hands the planner (head, frame, q block)
directly, and the per-frame records (coefficient, frame scale, key-row map) are scalar loads.  A barrier or a wait in the wrong
place in ONE wave is a wrong key / value tile for all eight, so every mode, both dtypes, whole and partial last q blocks (waves past
the end return early from the store) and one / two trips per key segment are held bit for bit against the same kernel with one item
per workgroup (ATTN_PIPE = 0: no boundary at all), and sampled rows against the fp64 softmax so that identity cannot pass on two
wrong results.

Shape: 20 heads, 14 frames (7 AID frames + 7 PLAIN riders for the interpolated modes), S = 768 / 700 = three q blocks:
3 x 14 x 20 = 840 items, at least three per workgroup on 256 CUs."""
import numpy as np
import pytest
import torch

from oracle import aid_oracle as O
from util import TOL, rel_l2, to_np64

pytestmark = pytest.mark.gpu

import aid_amd  # noqa: E402,F401
from aid_amd import ops  # noqa: E402

DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
ids_dt = lambda d: str(d).split(".")[-1]  # noqa: E731
H, N_AID, FRAMES, NQB = 20, 7, 14, 3
ITEMS = NQB * FRAMES * H
MODES = [("plain", False), ("outer", True), ("outer", False), ("inner", True), ("inner", False)]
ids_mode = lambda m: m if isinstance(m, str) else ("fused" if m else "pure")  # noqa: E731


def _needs_three_items_per_workgroup():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus * 3 > ITEMS:
        pytest.skip(f"{cus} CUs: {ITEMS} items are fewer than three per persistent workgroup")


_cache = {}


def _inputs(s, l, dtype):
    """q, k, vt of the base shape on the device (made once per (s, l, dtype) and never written)."""
    key = (s, l, dtype)
    if key not in _cache:
        g = torch.Generator(device=DEV).manual_seed(1000 * s + l)
        c = H * 64
        q = torch.randn(FRAMES, s, c, generator=g, device=DEV).to(dtype)
        k = torch.randn(FRAMES, l, c, generator=g, device=DEV).to(dtype)
        vt = torch.randn(FRAMES, c, l, generator=g, device=DEV).to(dtype)
        _cache.clear()                                          # one set of inputs alive at a time
        _cache[key] = (q, k, vt)
    return _cache[key]


def _coef(dtype):
    coef = torch.from_numpy(O.beta_coefs(N_AID, 50, 50)).float()
    coef[0], coef[-1] = 0, 1
    return coef.to(dtype).float()


def _args(mode, fused, l, dtype):
    if mode == "plain":
        return dict(l=l, mode="plain")
    cd = torch.cat([_coef(dtype), -torch.ones(FRAMES - N_AID)]).to(DEV)
    return dict(l=l, mode=mode, fused=fused, coef=cd, begin=0, end=N_AID - 1, n_plain=FRAMES - N_AID)


def _oracle_rows(q, k, vt, o, mode, fused, dtype, s):
    """Sampled (head, rows) of every frame against the fp64 oracle of the call's mode."""
    rows = torch.tensor([0, 31, 32, 255, 256, s - 1], device=DEV)
    for hh in (0, H // 2, H - 1):
        sl = slice(hh * 64, hh * 64 + 64)
        q64, k64, v64 = to_np64(q[:, rows][:, :, sl]), to_np64(k[:, :, sl]), to_np64(vt[:, sl, :].transpose(1, 2))
        if mode == "plain":
            ref = O.attn_core(q64, k64, v64, 1, 64 ** -0.5, "plain", False, None)
        else:
            ref = np.concatenate([O.attn_core(q64[:N_AID], k64[:N_AID], v64[:N_AID], 1, 64 ** -0.5, mode, fused, _coef(dtype).numpy()),
                                  O.attn_core(q64[N_AID:], k64[N_AID:], v64[N_AID:], 1, 64 ** -0.5, "plain", False, None)])
        got = to_np64(o[:, rows][:, :, sl])
        for f in range(FRAMES):
            assert rel_l2(got[f], ref[f]) < TOL[dtype], (mode, fused, hh, f, rel_l2(got[f], ref[f]))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("l", [512, 1024], ids=lambda l: f"l{l}")
@pytest.mark.parametrize("s", [768, 700], ids=lambda s: f"s{s}")
@pytest.mark.parametrize("mode,fused", MODES, ids=ids_mode)
def test_persistent_walk_equals_one_item_per_workgroup(mode, fused, s, l, dtype, tuning):
    """ATTN_PIPE = 1 (persistent, item boundaries) against ATTN_PIPE = 0 (one item per workgroup) bit for bit; two consecutive
    persistent runs are equal; sampled rows of the persistent result against the fp64 oracle."""
    _needs_three_items_per_workgroup()
    q, k, vt = _inputs(s, l, dtype)
    args = _args(mode, fused, l, dtype)
    tuning("ATTN_V2", 1)
    tuning("ATTN_PIPE", 1)
    o = ops.attn_fwd(q, k, vt, H, **args)
    assert "aid_attn_pp" in ops.last_attn_variant() and torch.isfinite(o).all()
    o_again = ops.attn_fwd(q, k, vt, H, **args)
    assert torch.equal(o, o_again)
    tuning("ATTN_PIPE", 0)
    o_one = ops.attn_fwd(q, k, vt, H, **args)
    assert "aid_attn_pp" in ops.last_attn_variant()
    assert torch.equal(o, o_one)
    _oracle_rows(q, k, vt, o, mode, fused, dtype, s)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("s", [768, 700], ids=lambda s: f"s{s}")
def test_plain_accumulate_and_frame_scale_across_item_boundaries(s, dtype, tuning):
    """The accumulate path (loads between the stores) and the per-frame scale (a scalar load in the boundary) of ops.attn_fwd:
    persistent against one item per workgroup bit for bit, sampled rows against the oracle."""
    _needs_three_items_per_workgroup()
    l = 512
    q, k, vt = _inputs(s, l, dtype)
    g = torch.Generator(device=DEV).manual_seed(s)
    base = torch.randn(FRAMES, s, H * 64, generator=g, device=DEV).to(dtype)
    fs = (0.25 + torch.arange(FRAMES, dtype=torch.float32) / 8).to(DEV)
    kv_map = torch.tensor([(f * 5 + 3) % FRAMES for f in range(FRAMES)], dtype=torch.int32, device=DEV)
    tuning("ATTN_V2", 1)
    outs = []
    for pipe in (1, 0):
        tuning("ATTN_PIPE", pipe)
        out = base.clone()
        ops.attn_fwd(q, k, vt, H, l=l, mode="plain", kv_map=kv_map, frame_scale=fs, out_scale=0.7, accumulate=True, out=out)
        assert "aid_attn_pp" in ops.last_attn_variant()
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    rows = torch.tensor([0, 31, 32, 255, 256, s - 1], device=DEV)
    idx = kv_map.long()
    for hh in (0, H - 1):
        sl = slice(hh * 64, hh * 64 + 64)
        ref = O.attn_core(to_np64(q[:, rows][:, :, sl]), to_np64(k[idx][:, :, sl]), to_np64(vt[idx][:, sl, :].transpose(1, 2)), 1,
                          64 ** -0.5, "plain", False, None)
        ref = to_np64(base[:, rows][:, :, sl]) + 0.7 * to_np64(fs)[:, None, None] * ref
        assert rel_l2(to_np64(outs[0][:, rows][:, :, sl]), ref) < TOL[dtype], hh


def test_default_rule_sends_plain_1024_keys_to_persistent_workgroups(tuning):
    """No knob: a PLAIN call with 1024 keys runs on the ping-pong kernel when the persistent walk applies (more items than CUs, whole
    8-tile trips) and stays on the program-order kernel with three items; the two kernels agree within the storage type's tolerance."""
    _needs_three_items_per_workgroup()
    dtype, l = torch.bfloat16, 1024
    q, k, vt = _inputs(768, l, dtype)
    o = ops.attn_fwd(q, k, vt, H, l=l, mode="plain")
    assert ops.last_attn_variant() == "aid_attn_pp<d64>"
    ops.attn_fwd(q[:3, :256, :64].contiguous(), k[:3, :, :64].contiguous(), vt[:3, :64].contiguous(), 1, l=l, mode="plain")
    assert "aid_attn_pp" not in ops.last_attn_variant()
    tuning("ATTN_V2", 0)
    o_old = ops.attn_fwd(q, k, vt, H, l=l, mode="plain")
    assert "aid_attn_pp" not in ops.last_attn_variant()
    assert torch.isfinite(o).all() and rel_l2(to_np64(o), to_np64(o_old)) < TOL[dtype]
