"""Replay-form attention calls: cases and fp64 reference (no GPU).

The end-point store and the key-frame store replay an attention call with the two recorded end-point rows BEHIND the call's own
K / V^T rows: ``n_kv = n_frames + 2``, ``begin = n_frames``, ``end = n_frames + 1``, no frame of the batch an end point (every AID
frame walks two or three key segments), riders counted in ``n_frames``.  Every earlier caller has begin / end among the frames (the
classic layout ``[B, interior frames, E, riders]``).  ``full_batch`` makes one set of bits in the classic layout, ``replay_form``
moves the same bits into the replay layout, ``attn_ref`` is the frame-by-frame fp64 reference of both.
"""
import functools

import numpy as np
import torch

from util import to_np64


def round_up(x, m):
    return (x + m - 1) // m * m


# ================================================================================================================================
# fp64 reference
# ================================================================================================================================
def sdpa(q, k, v, h, scale, bias=None):
    """fp64 softmax(q k^T * scale + bias) v per head; q [s, c], k / v [L, c], bias [s, L] or None."""
    s, c = q.shape
    d = c // h
    qh, kh, vh = (t.reshape(t.shape[0], h, d).transpose(1, 0, 2) for t in (q, k, v))
    sc = qh @ kh.transpose(0, 2, 1) * scale
    if bias is not None:
        sc = sc + bias[None]
    sc = sc - sc.max(axis=-1, keepdims=True)
    p = np.exp(sc)
    p /= p.sum(axis=-1, keepdims=True)
    return (p @ vh).transpose(1, 0, 2).reshape(s, c)


def attn_ref(q, k, v, h, mode, fused, coef, begin, end, kv_map=None, bias=None):
    """fp64 AID attention (aid_hip.h AidAttnArgs), frame by frame: riders (negative coefficient) attend PLAIN to their own keys.
    k / v may hold more rows than q: ``own``, ``begin`` and ``end`` index them freely."""
    n, _, c = q.shape
    scale = (c // h) ** -0.5
    out = []
    for i in range(n):
        own = i if kv_map is None else int(kv_map[i])
        b_ = None if bias is None else bias[i]
        ci = None if coef is None else float(coef[i])
        if mode == "plain" or ci < 0:
            out.append(sdpa(q[i], k[own], v[own], h, scale, b_))
            continue
        if mode == "inner":
            kc, vc = (1 - ci) * k[begin] + ci * k[end], (1 - ci) * v[begin] + ci * v[end]
            if fused:
                kc, vc = np.concatenate([k[own], kc]), np.concatenate([v[own], vc])
            out.append(sdpa(q[i], kc, vc, h, scale, b_))
        else:
            sides = []
            for e in (begin, end):
                ke, ve = (np.concatenate([k[own], k[e]]), np.concatenate([v[own], v[e]])) if fused else (k[e], v[e])
                sides.append(sdpa(q[i], ke, ve, h, scale, b_))
            out.append((1 - ci) * sides[0] + ci * sides[1])
    return np.stack(out)


# ================================================================================================================================
# inputs
# ================================================================================================================================
@functools.lru_cache(maxsize=8)
def full_batch(n, riders, s, l, h, d, dtype, seed):
    """q / k / v / vt (CPU, rounded to ``dtype``; never written by a caller) in the classic layout [B, n interior frames, E,
    riders...]; V^T zero-padded to round_up(l, 8) columns.  Spiked keys ``k[row, j] = 5 * q[f, r]`` (every index modulo its
    dimension) as in the rescale tests of test_hip_attn_pingpong.py: one in B's first tile and one in E's LAST tile, both aimed at
    the same row of the first interior frame — after that frame's own keys the begin side leaves the parked row reference behind,
    and the end side, which starts again from the parked state, raises it again —, a second one in E's last tile for another
    interior frame, and one in an interior frame's own keys."""
    c = h * d
    f = n + 2 + riders
    e_row = n + 1
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(f, s, c, generator=g).to(dtype)
    k = torch.randn(f, l, c, generator=g).to(dtype)
    v = torch.randn(f, l, c, generator=g).to(dtype)
    interior = lambda i: 1 + i % n  # noqa: E731
    k[0, 5 % l] = (5.0 * q[interior(0), 5 % s].float()).to(dtype)
    k[e_row, (l - 1) % l] = (5.0 * q[interior(0), 5 % s].float()).to(dtype)
    k[e_row, (l - 3) % l] = (5.0 * q[interior(1), 9 % s].float()).to(dtype)
    k[interior(1), 200 % l] = (5.0 * q[interior(1), 17 % s].float()).to(dtype)
    vt = torch.zeros(f, c, round_up(l, 8), dtype=dtype)
    vt[:, :, :l] = v.transpose(1, 2)
    return dict(q=q, k=k, v=v, vt=vt, n=n, riders=riders, s=s, l=l, h=h, d=d, dtype=dtype)


def classic_coef(coef):
    """Coefficients of the classic call for replay coefficients ``coef`` (interior frames, then riders): B gets 0, E gets 1."""
    n = sum(1 for x in coef if x >= 0)
    return [0.0] + list(coef[:n]) + [1.0] + list(coef[n:])


def replay_form(batch, swap=False, same=False):
    """The same bits in the replay layout: q = interior frames, then riders; k / v / vt rows = interior, riders, B, E;
    ``begin = n + riders``, ``end = begin + 1`` (``swap``: exchanged; ``same``: both the B row).  ``q_rows`` / ``kv_rows`` are
    the classic rows the replay rows came from, so that a test can compare against the classic call."""
    n, riders = batch["n"], batch["riders"]
    q_rows = list(range(1, n + 1)) + list(range(n + 2, n + 2 + riders))
    kv_rows = q_rows + [0, n + 1]
    begin = n + riders
    end = begin + 1
    if swap:
        begin, end = end, begin
    if same:
        end = begin
    out = dict(batch, q_rows=q_rows, kv_rows=kv_rows, begin=begin, end=end)
    out["q"] = batch["q"][q_rows].contiguous()
    for name in ("k", "v", "vt"):
        out[name] = batch[name][kv_rows].contiguous()
    return out


def np64(form):
    """fp64 (q, k, v) of a batch or a replay form."""
    return to_np64(form["q"]), to_np64(form["k"]), to_np64(form["v"])


def rounded_coef(coef, dtype):
    """Coefficients rounded to the storage type like the processors do (``proc.coef.to(dtype).float()``); riders stay -1."""
    return torch.tensor(coef, dtype=torch.float32).to(dtype).float().tolist()


# ================================================================================================================================
# cases
# ================================================================================================================================
# coefficient sets: replay coefficients (interior frames, then riders), the n_plain hint, swap / same for replay_form
COEF_SETS = {
    "R1": dict(coef=[0.25, 0.4, 0.75]),                              # (no 0.5: OUTER is symmetric there)
    "R2": dict(coef=[0.4]),                                          # one frame alone
    "R3": dict(coef=[0.0, 0.3, 1.0]),                                # exactly 0 / 1 on frames whose own keys are NOT the end-point row
    "R4": dict(coef=[0.25, 0.75, -1.0, -1.0], n_plain=2),            # two CFG riders
    "R4_hint0": dict(coef=[0.25, 0.75, -1.0, -1.0], n_plain=0),      # ... with the wrong hint
    "R5": dict(coef=[0.25, 0.4, 0.75], swap=True),
    "R6": dict(coef=[0.25, 0.4, 0.75], same=True),                   # begin == end: both sides read the same row
}
AID_MODES = [("outer", False), ("outer", True), ("inner", False), ("inner", True)]
ids_mode = lambda m: m if isinstance(m, str) else ("fused" if m else "pure")  # noqa: E731
H, S = 2, 67

# engine id: (head dim, keys, float32 storage, knobs, f32_attn_precision)
_ORDER = {"ATTN_RES": 0, "ATTN_TX": 0, "ATTN_V2": 0}
ENGINES = {
    "nw4": (80, 130, False, dict(_ORDER, ATTN_NW=4, ATTN_PIPE=0), None),
    "nw4_d160": (160, 130, False, dict(_ORDER, ATTN_NW=4, ATTN_PIPE=0), None),
    "nw8": (64, 130, False, dict(_ORDER, ATTN_NW=8), None),
    "pipe": (40, 200, False, dict(_ORDER, ATTN_NW=4, ATTN_QB=1, ATTN_PIPE=1), None),
    "res": (40, 77, False, {"ATTN_RES": 1, "ATTN_TX": 0, "ATTN_V2": 0}, None),
    "textkey": (64, 77, False, {}, None),
    "pingpong": (64, 512, False, {"ATTN_V2": 1, "ATTN_TX": 0}, None),
    "pp_split": (64, 128, False, {"ATTN_V2": 1, "ATTN_TX": 0}, None),
    "f32": (64, 77, True, {}, None),
    "f32x3": (40, 130, True, {}, "high"),
}


def engine_dtypes(engine):
    return [torch.float32] if ENGINES[engine][2] else [torch.float16, torch.bfloat16]


def case_inputs(engine, dtype, s, set_name):
    """(classic batch, replay form, replay coefficients rounded to ``dtype``) of one (engine shape, coefficient set): the very
    inputs of the GPU tests.  Sets with the same frame counts share the batch."""
    d, l = ENGINES[engine][:2]
    cs = COEF_SETS[set_name]
    n = sum(1 for x in cs["coef"] if x >= 0)
    riders = len(cs["coef"]) - n
    batch = full_batch(n, riders, s, l, H, d, dtype, 1000 * d + l + 7 * s + n)
    form = replay_form(batch, swap=cs.get("swap", False), same=cs.get("same", False))
    return batch, form, rounded_coef(cs["coef"], dtype)
