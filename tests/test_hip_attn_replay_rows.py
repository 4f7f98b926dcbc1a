"""GPU: the attention core in the REPLAY layout of the end-point / key-frame stores, on every engine (tests/replay_rows.py).

The stores replay a layer with the two recorded end-point rows BEHIND the call's own K / V^T rows: n_kv = n_frames + 2, begin =
n_frames, end = n_frames + 1, no kv_map, no frame of the batch an end point (every AID frame walks two or three key segments), n_frames
may be 1 + a rider.  Each engine re-derives single / one-sided / both-sided, the "own" row and the parked state per frame on the
device, and its host-side hints (plan_attn's n_single, the ping-pong launch's heavy-frame range, the text-key launch's AID count)
assume end points at frames 0 and n_aid - 1.  Every engine is forced by knob and asserted by name on every call.

Per call: (a) finite, per-frame rel-L2 and the call's worst element against the fp64 frame-by-frame reference within the project's
bounds (TOL / WORST; 1e-5 / 1e-4 fp32; TOL_F32_HIGH / WORST_F32_HIGH for the split kernel); (b) RELOCATION, bit for bit: the same
engine on the classic layout [B, interior, E, riders] of the same bits gives exactly the replay result at the interior frames and
the riders (R5: classic begin = E's row, end = 0; R6 has no classic call); (c) the wrong n_plain hint gives the bits of the right
one; (d) two runs give equal bits.  That a wrongly addressed result cannot pass (a) is tests/test_replay_rows.py.

Relocation holds bit for bit on EVERY engine: nw4 (d = 80, 160), nw8, pipe, res, text-key, ping-pong (alone and persistent), the
split plan, f32 and f32x3.  One legitimate dependence: under ATTN_V2 = 1 a call the ping-pong kernel cannot run alone is split, and
the n_plain hint is what plans the ping-pong launch of a PURE call (n_single = n_plain) — with the wrong hint 0 the riders run on the
program-order kernel instead, another accumulation order.  There (pp_split, pure, R4_hint0) the riders keep the oracle check and the
AID frames the bit check.

Largest rel-L2 of a frame / largest worst element of a call over all coefficient sets, the four modes and S in {1, 67, 300}, against
the fp64 reference (never against a kernel's own output), measured on an MI355X; bounds: fp16 1e-3 / 4e-2, bf16 8e-3 / 0.25, fp32
1e-5 / 1e-4, f32x3 3e-5 / 3e-4:

    engine      fp16                   bf16                        engine    fp32
    nw4         5.22e-4 / 1.12e-2      4.19e-3 / 7.64e-2           f32       4.19e-7 / 1.14e-5
    nw4_d160    5.05e-4 / 1.39e-2      4.11e-3 / 8.17e-2           f32x3     1.04e-5 / 2.13e-4
    nw8         4.97e-4 / 9.90e-3      4.14e-3 / 6.33e-2
    pipe        5.95e-4 / 1.38e-2      4.47e-3 / 1.05e-1
    res         5.01e-4 / 8.35e-3      4.92e-3 / 8.15e-2
    textkey     4.17e-4 / 8.07e-3      3.64e-3 / 6.59e-2
    pingpong    6.06e-4 / 1.31e-2      4.48e-3 / 1.51e-1
    pp_split    6.24e-4 / 1.09e-2      4.88e-3 / 9.88e-2
"""
import numpy as np
import pytest
import torch

import replay_rows as R
from util import TOL, WORST, rel_l2, to_np64, worst

pytestmark = pytest.mark.gpu

import aid_amd  # noqa: E402
from aid_amd import ops  # noqa: E402
from test_hip_attn_f32x3 import TOL_F32_HIGH, WORST_F32_HIGH  # noqa: E402

DEV = "cuda:0"
DT = {torch.float16: "f16", torch.bfloat16: "bf16"}
ids_dt = lambda d: str(d).split(".")[-1]  # noqa: E731
ENGINE_DTYPES = [pytest.param(e, dt, id=f"{e}-{ids_dt(dt)}") for e in R.ENGINES for dt in R.engine_dtypes(e)]


def _bounds(engine, dtype):
    if engine == "f32x3":
        return TOL_F32_HIGH, WORST_F32_HIGH
    return (1e-5, 1e-4) if dtype == torch.float32 else (TOL[dtype], WORST[dtype])


def _assert_variant(engine, dtype, mode, fused, n_frames, n_plain, labels):
    """The name the call reports — and, for the split plan, the launches it made (profile labels, as test_hip_attn_plan.py)."""
    name = ops.last_attn_variant()
    if engine == "pp_split":
        # plan_attn: the ping-pong launch is planned when the host counts a single-segment frame: the riders of the hint, and two end
        # points for a fused call of two or more AID frames — which the replay layout does not have: that launch then finds no frame
        # of its own and the program-order launch does everything
        n_single = n_plain + (2 if fused and n_frames - n_plain >= 2 else 0)
        order = f"aid_attn<{DT[dtype]},d64,{mode},nw4>"
        assert name == order, name
        assert labels == ([f"aid_attn_pp<{DT[dtype]},d64,riders>"] if n_single else []) + [order], (labels, n_single)
        return name
    want = {"nw4": ",nw4>", "nw4_d160": "d160", "nw8": ",nw8>", "pipe": ",pipe>", "res": ",res>", "textkey": "aid_attn_tx<d64,"}
    if engine in want:
        assert want[engine] in name, (engine, name)
    else:
        assert name == {"pingpong": f"aid_attn_pp<d64,{mode}>", "f32": "aid_attn_f32", "f32x3": "aid_attn_f32x3"}[engine], name
    return name


def _call(engine, dtype, form, mode, fused, coef, begin, end, n_plain):
    """ops.attn_fwd on a batch / replay form -> output; asserts the variant."""
    lib = aid_amd._lib.load()
    prec = R.ENGINES[engine][4]
    split = engine == "pp_split"
    if split:
        lib.aid_profile_begin()
    o = ops.attn_fwd(form["q"].to(DEV), form["k"].to(DEV), form["vt"].to(DEV), R.H, l=form["l"], mode=mode, fused=fused,
                     coef=torch.tensor(coef, dtype=torch.float32, device=DEV), begin=begin, end=end, n_plain=n_plain,
                     f32_attn_precision=prec)
    labels = None
    if split:
        buf = (aid_amd._lib.AidProfileEntry * 16)()
        cnt = lib.aid_profile_end(buf, 16)
        labels = [e.kernel.decode() for e in buf[:cnt] if e.kernel.decode().startswith("aid_attn")]
    _assert_variant(engine, dtype, mode, fused, form["q"].shape[0], n_plain, labels)
    return o


FIGURES = {}                                                    # (engine, dtype) -> [largest rel-L2 of a frame, largest worst]


def _replay_case(engine, dtype, mode, fused, s, set_name, outs):
    cs = R.COEF_SETS[set_name]
    batch, form, coef = R.case_inputs(engine, dtype, s, set_name)
    n, riders = form["n"], form["riders"]
    hint = cs.get("n_plain", 0)
    what = (engine, ids_dt(dtype), mode, fused, s, set_name)
    o = _call(engine, dtype, form, mode, fused, coef, form["begin"], form["end"], hint)
    assert torch.equal(o, _call(engine, dtype, form, mode, fused, coef, form["begin"], form["end"], hint)), (what, "two runs")
    outs[set_name] = o
    # (a) the fp64 reference
    tol, wst = _bounds(engine, dtype)
    got = to_np64(o)
    assert np.isfinite(got).all(), what
    ref = R.attn_ref(*R.np64(form), R.H, mode, fused, coef, form["begin"], form["end"])
    errs = [rel_l2(got[i], ref[i]) for i in range(n + riders)]
    w = worst(got, ref)
    fig = FIGURES.setdefault((engine, ids_dt(dtype)), [0.0, 0.0])
    fig[0], fig[1] = max(fig[0], max(errs)), max(fig[1], w)
    print(f"[replay] {what} rel-L2 per frame {['%.2e' % e for e in errs]} worst {w:.2e}")
    assert max(errs) < tol and w < wst, (what, errs, w)
    # (c) the n_plain hint is accounting: the wrong one gives the same bits
    if set_name == "R4_hint0":
        rows = slice(0, n) if (engine == "pp_split" and not fused) else slice(None)     # (the module docstring)
        assert torch.equal(o[rows], outs["R4"][rows]), (what, "n_plain hint")
    # (b) the classic layout of the same bits, same engine
    if cs.get("same"):
        return
    cb, ce = (n + 1, 0) if cs.get("swap") else (0, n + 1)
    oc = _call(engine, dtype, batch, mode, fused, R.classic_coef(coef), cb, ce, hint)
    diff = [i for i, r in enumerate(form["q_rows"]) if not torch.equal(o[i], oc[r])]
    assert not diff, (what, "relocation: frames that differ", diff)


@pytest.fixture(scope="module", autouse=True)
def _print_figures():
    """The largest figures of the cases below, per engine and dtype (pytest -s), once the module is through."""
    yield
    for (engine, dt), (e, w) in sorted(FIGURES.items()):
        print(f"[replay-figures] {engine:9s} {dt:9s} rel-L2 {e:.2e}  worst {w:.2e}")


@pytest.mark.parametrize("s", [R.S, 1, 300], ids=lambda s: f"s{s}")
@pytest.mark.parametrize("mode,fused", R.AID_MODES, ids=R.ids_mode)
@pytest.mark.parametrize("engine,dtype", ENGINE_DTYPES)
def test_replay_rows_on_every_engine(engine, dtype, mode, fused, s, tuning):
    """S = 67 (a ragged last tile, more than one key tile per segment): every coefficient set R1 - R6.  S = 1 and S = 300 (several
    query blocks on the program-order kernels, a partial second 256-row item on ping-pong): R4, two frames + two CFG riders."""
    for name, value in R.ENGINES[engine][3].items():
        tuning(name, value)
    outs = {}
    for set_name in (list(R.COEF_SETS) if s == R.S else ["R4", "R4_hint0"]):
        _replay_case(engine, dtype, mode, fused, s, set_name, outs)


# ================================================================================================================================
# the persistent ping-pong walk
# ================================================================================================================================
PH, PL = 20, 512


def _persistent_inputs(n, riders, s, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    c, f = PH * 64, n + riders
    q = torch.randn(f, s, c, generator=g, device=DEV).to(torch.bfloat16)
    k = torch.randn(f + 2, PL, c, generator=g, device=DEV).to(torch.bfloat16)
    vt = torch.randn(f + 2, c, PL, generator=g, device=DEV).to(torch.bfloat16)
    k[f, 5] = (5.0 * q[0, 5].float()).to(torch.bfloat16)               # B's first tile and E's last tile, the same row of frame 0
    k[f + 1, PL - 1] = (5.0 * q[0, 5].float()).to(torch.bfloat16)
    return q, k, vt


@pytest.mark.parametrize("mode", ["outer", "inner"])
@pytest.mark.parametrize("coef,riders,s", [([0.1, 0.3, 0.5, 0.7, 0.9], 3, 700), ([0.4], 1, 1700)], ids=["5+3-s700", "1+1-s1700"])
def test_replay_rows_on_the_persistent_pingpong_walk(coef, riders, s, mode, tuning):
    """Fused OUTER / INNER, bf16, 20 heads, 512 keys: five replay frames + three riders at S = 700 (480 items) and the call that
    renders ONE new frame (+ one rider) at S = 1700 (280 items).  The persistent walk (ATTN_PIPE unset) against one item per
    workgroup (ATTN_PIPE = 0) bit for bit, two persistent runs equal, sampled rows against the fp64 reference."""
    n = len(coef)
    f = n + riders
    items = (s + 255) // 256 * f * PH
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus >= items:
        pytest.skip(f"{cus} CUs: {items} items do not make a persistent walk")
    dtype = torch.bfloat16
    q, k, vt = _persistent_inputs(n, riders, s, seed=s + n)
    cf = R.rounded_coef(coef, dtype) + [-1.0] * riders
    args = dict(l=PL, mode=mode, fused=True, coef=torch.tensor(cf, dtype=torch.float32, device=DEV), begin=f, end=f + 1,
                n_plain=riders)
    tuning("ATTN_V2", 1)
    tuning("ATTN_TX", 0)
    o = ops.attn_fwd(q, k, vt, PH, **args)
    assert ops.last_attn_variant() == f"aid_attn_pp<d64,{mode}>" and torch.isfinite(o).all()
    assert torch.equal(o, ops.attn_fwd(q, k, vt, PH, **args))
    tuning("ATTN_PIPE", 0)
    o_one = ops.attn_fwd(q, k, vt, PH, **args)
    assert ops.last_attn_variant() == f"aid_attn_pp<d64,{mode}>"
    assert torch.equal(o, o_one)
    rows = torch.tensor([0, 5, 31, 32, 255, 256, s - 1], device=DEV)    # (row 5 of frame 0 carries the spikes)
    for hh in (0, PH // 2, PH - 1):
        sl = slice(hh * 64, hh * 64 + 64)
        ref = R.attn_ref(to_np64(q[:, rows][:, :, sl]), to_np64(k[:, :, sl]), to_np64(vt[:, sl, :].transpose(1, 2)), 1, mode, True,
                         cf, f, f + 1)
        got = to_np64(o[:, rows][:, :, sl])
        for i in range(f):
            assert rel_l2(got[i], ref[i]) < TOL[dtype], (mode, hh, i, rel_l2(got[i], ref[i]))
