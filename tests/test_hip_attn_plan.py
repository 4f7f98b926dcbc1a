"""What the attention plan names (GPU): the profile labels of one attention call (``AidProfileEntry.kernel`` — the strings bench.py's
roofline, tools/kbench*.py, tools/stack_breakdown.py and the committed profiles group by), their agreement with
``aid_last_attn_variant()``, and the work attribution of a split call (ping-pong kernel for the single-segment frames + program-order
kernel for the rest).  One case per engine and per variant of the program-order kernel, at the smallest shapes at which each is
still the one chosen; every output is checked against the fp64 oracle so that a label test cannot pass on garbage."""
import numpy as np
import pytest
import torch

from oracle import aid_oracle as O
from util import TOL, WORST, rel_l2, to_np64, worst

pytestmark = pytest.mark.gpu

import aid_amd  # noqa: E402
from aid_amd import ops  # noqa: E402
from test_hip_f32 import TOL_F32, WORST_F32  # noqa: E402

DEV = "cuda:0"
N, H, S = 5, 2, 64
COEF = [0.0, 0.25, 0.75, 1.0, -1.0]                 # frames 0 .. 3 interpolate between 0 and 3, frame 4 rides PLAIN
DT = {torch.float16: "f16", torch.bfloat16: "bf16"}

# id: (d, l, mode, fused, zero score bias, knobs, profile labels in order, last_attn_variant())
CASES = {
    "text_key":       (64, 77, "outer", True, False, {}, ["aid_attn_tx<{dt},d64,outer>"], "aid_attn_tx<d64,outer>"),
    "pingpong_alone": (64, 512, "outer", True, False, {"ATTN_V2": 1, "ATTN_TX": 0}, ["aid_attn_pp<{dt},d64,outer>"], "aid_attn_pp<d64,outer>"),
    "pingpong_plain": (64, 128, "plain", False, False, {"ATTN_V2": 1, "ATTN_TX": 0}, ["aid_attn_pp<{dt},d64>"], "aid_attn_pp<d64>"),
    "split":          (64, 128, "outer", True, False, {"ATTN_V2": 1, "ATTN_TX": 0},
                       ["aid_attn_pp<{dt},d64,riders>", "aid_attn<{dt},d64,outer,nw4>"], "aid_attn<{dt},d64,outer,nw4>"),
    "resident":       (40, 77, "inner", False, False, {}, ["aid_attn<{dt},d40,inner,res>"], None),
    "bias":           (80, 130, "plain", False, True, {"ATTN_TX": 0}, ["aid_attn<{dt},d80,plain,nw4,bias>"], None),
    "qb2":            (40, 130, "plain", False, False, {"ATTN_QB": 2, "ATTN_RES": 0}, ["aid_attn<{dt},d40,plain,nw4,qb2>"], None),
    "nw8":            (64, 130, "outer", True, False, {"ATTN_NW": 8, "ATTN_V2": 0, "ATTN_TX": 0}, ["aid_attn<{dt},d64,outer,nw8>"], None),
    "pipe":           (40, 200, "inner", True, False, {"ATTN_PIPE": 1, "ATTN_RES": 0}, ["aid_attn<{dt},d40,inner,nw4,pipe>"], None),
}                                                   # variant None: a single program-order launch — the string IS the label


def _inputs(l, d, dtype, seed):                     # as tests/test_hip_parity.py::_core_inputs
    g = torch.Generator().manual_seed(seed)
    c = H * d
    q = torch.randn(N, S, c, generator=g).to(dtype)
    k = torch.randn(N, l, c, generator=g).to(dtype)
    v = torch.randn(N, l, c, generator=g).to(dtype)
    vt = torch.zeros(N, c, (l + 7) // 8 * 8, dtype=dtype)
    vt[:, :, :l] = v.transpose(1, 2)
    return q, k, v, vt


def _profiled_call(q, k, vt, l, mode, fused, bias):
    """one ops.attn_fwd under the live profiler -> (output, its aid_attn* entries as (kernel, flops, bytes, flops_executed), variant)"""
    lib = aid_amd._lib.load()
    plain = mode == "plain"
    coef = None if plain else torch.tensor(COEF).to(DEV)
    lib.aid_profile_begin()
    o = ops.attn_fwd(q.to(DEV), k.to(DEV), vt.to(DEV), H, l=l, mode=mode, fused=fused, coef=coef, begin=0, end=3,
                     n_plain=0 if plain else 1, bias=bias)
    variant = ops.last_attn_variant()
    buf = (aid_amd._lib.AidProfileEntry * 64)()
    cnt = lib.aid_profile_end(buf, 64)
    ent = [(e.kernel.decode(), e.flops, e.bytes, e.flops_executed) for e in buf[:cnt] if e.kernel.decode().startswith("aid_attn")]
    return o, ent, variant


def _oracle(q, k, v, d, mode, fused):
    q64, k64, v64 = to_np64(q), to_np64(k), to_np64(v)
    if mode == "plain":
        return O.attn_core(q64, k64, v64, H, d ** -0.5, "plain", False, None)
    coef = np.asarray(COEF[:4], np.float32).astype(np.float64)
    return np.concatenate([O.attn_core(q64[:4], k64[:4], v64[:4], H, d ** -0.5, mode, fused, coef),
                           O.attn_core(q64[4:], k64[4:], v64[4:], H, d ** -0.5, "plain", False, None)])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("case", list(CASES))
def test_attention_profile_labels_and_variant(dtype, case, tuning):
    d, l, mode, fused, with_bias, knobs, labels, variant = CASES[case]
    for name, value in knobs.items():
        tuning(name, value)
    labels = [s.format(dt=DT[dtype]) for s in labels]
    q, k, v, vt = _inputs(l, d, dtype, seed=d * 1000 + l)
    bias = torch.zeros(N, 1, l, dtype=dtype, device=DEV) if with_bias else None
    o, ent, got_variant = _profiled_call(q, k, vt, l, mode, fused, bias)
    assert [e[0] for e in ent] == labels
    assert got_variant == (labels[0] if variant is None else variant.format(dt=DT[dtype]))
    ref = _oracle(q, k, v, d, mode, fused)              # (a bias of zeros changes nothing)
    assert torch.isfinite(o).all()
    err = rel_l2(to_np64(o), ref)
    assert err < TOL[dtype] and worst(to_np64(o), ref) < WORST[dtype], (case, got_variant, err)
    if case != "split":
        return
    # the same call on the program-order kernel alone: one entry, and the two launches of the split call account for exactly its work
    tuning("ATTN_V2", 0)
    o1, ent1, variant1 = _profiled_call(q, k, vt, l, mode, fused, bias)
    assert [e[0] for e in ent1] == labels[1:] and variant1 == labels[1]
    for i, what in ((1, "flops"), (2, "bytes"), (3, "flops_executed")):
        assert ent[0][i] > 0 and ent[1][i] > 0 and ent[0][i] + ent[1][i] == ent1[0][i], (what, ent, ent1)
    assert rel_l2(to_np64(o), to_np64(o1)) < TOL[dtype]


def test_attention_profile_label_f32():
    d, l = 64, 77
    q, k, v, vt = _inputs(l, d, torch.float32, seed=d * 1000 + l)
    o, ent, variant = _profiled_call(q, k, vt, l, "outer", True, None)
    assert [e[0] for e in ent] == ["aid_attn_f32<d64,outer>"] and variant == "aid_attn_f32"
    ref = _oracle(q, k, v, d, "outer", True)
    assert torch.isfinite(o).all() and o.dtype == torch.float32
    assert rel_l2(to_np64(o), ref) < TOL_F32 and worst(to_np64(o), ref) < WORST_F32, (rel_l2(to_np64(o), ref), worst(to_np64(o), ref))
