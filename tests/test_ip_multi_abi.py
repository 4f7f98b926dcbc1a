"""Several IP-Adapters per layer and regional ip_adapter_masks: the host side, without a GPU.

The entry point ``aid_ip_attn_fwd`` and its two structs (declared, exported, laid out as gcc lays them out, argument checks that are
pure host code), ``aid_processor_ip_fwd`` beside an unchanged ``AidProcessorArgs`` and ABI version, how ``HipIPAdapterAttnProcessor`` turns
diffusers' image branches into key segments (against a stand-in library that records what the Python layer hands over; the fp64
restatement of diffusers' semantics is tests/ip_multi_ref.py), and the kernel's resource table."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import aid_amd
from aid_amd import _lib, ops, processors
from ip_multi_ref import row_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "attention-interpolation-diffusion_amd", "csrc")
HEADER = open(os.path.join(ROOT, "include", "aid_hip.h")).read()


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_the_version_stays():
    assert re.search(r"^int\s+aid_ip_attn_fwd\s*\(const AidIpAttnArgs\* args", HEADER, flags=re.M)
    assert re.search(r"^int\s+aid_processor_ip_fwd\s*\(const AidProcessorArgs\* args", HEADER, flags=re.M)
    assert {"aid_ip_attn_fwd", "aid_processor_ip_fwd"} <= set(_lib.ABI_SYMBOLS)
    lib = _lib.load()
    assert hasattr(lib, "aid_ip_attn_fwd") and hasattr(lib, "aid_processor_ip_fwd")
    assert int(re.search(r"#define AID_IP_MAX_SEGMENTS (\d+)", HEADER).group(1)) == _lib.IP_MAX_SEGMENTS == 8
    assert lib.aid_abi_version() == 10 and _lib.AID_ABI_VERSION == 10
    assert re.search(r"#define AID_ABI_VERSION 10\b", HEADER)


def test_new_structs_match_the_header_layout(tmp_path):
    structs = {"AidIpSegment": _lib.AidIpSegment, "AidIpAttnArgs": _lib.AidIpAttnArgs, "AidProcessorArgs": _lib.AidProcessorArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "aid_hip.h"', 'int main(void) {']
    for name, cls in structs.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{name}.{fname} %zu\\n", offsetof({name}, {fname}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for name, cls in structs.items():
        assert int(out[name]) == C.sizeof(cls), name
        for fname, _ in cls._fields_:
            assert int(out[f"{name}.{fname}"]) == getattr(cls, fname).offset, f"{name}.{fname}"
    # the segments travel beside AidProcessorArgs (aid_processor_ip_fwd): the struct is the one of the previous header
    assert [f for f, _ in _lib.AidProcessorArgs._fields_][-1] == "lora_gain_o" and C.sizeof(_lib.AidProcessorArgs) == 440


def _valid_args(n_seg=1, d=64, dtype=_lib.DTYPE_BF16):
    segs = (_lib.AidIpSegment * max(n_seg, 1))()
    for s in segs:
        s.k, s.vt, s.t, s.ldvt, s.n_rows, s.scale = 0x1000, 0x2000, 4, 8, 1, 1.0
    a = _lib.AidIpAttnArgs()
    a.q, a.out, a.segments = 0x3000, 0x4000, C.addressof(segs)
    a.n_segments, a.n_frames, a.s, a.heads, a.d = n_seg, 2, 64, 2, d
    a.ldq = a.ldo = 2 * d
    a.q_fs = a.o_fs = 64 * 2 * d
    a.dtype, a.softmax_scale = dtype, d ** -0.5
    return a, segs


def test_argument_checks_return_codes_without_a_gpu():
    lib = _lib.load()
    assert lib.aid_ip_attn_fwd(None, None) == -1
    a, keep = _valid_args()
    a.q = None
    assert lib.aid_ip_attn_fwd(C.byref(a), None) == -1
    a, keep = _valid_args()
    a.segments = None
    assert lib.aid_ip_attn_fwd(C.byref(a), None) == -1
    a, keep = _valid_args(n_seg=9)                              # more than AID_IP_MAX_SEGMENTS
    assert lib.aid_ip_attn_fwd(C.byref(a), None) == -1
    a, keep = _valid_args(n_seg=0)
    assert lib.aid_ip_attn_fwd(C.byref(a), None) == -1
    a, keep = _valid_args(d=128)                                # head dim 128 stays unsupported
    assert lib.aid_ip_attn_fwd(C.byref(a), None) == -3
    a, keep = _valid_args(dtype=_lib.DTYPE_F32)                 # no float32 segment form
    assert lib.aid_ip_attn_fwd(C.byref(a), None) == -2
    a, keep = _valid_args()
    keep[0].t = 0
    assert lib.aid_ip_attn_fwd(C.byref(a), None) == -1
    a, keep = _valid_args()
    keep[0].n_rows = 3                                          # neither 1 nor n_frames
    assert lib.aid_ip_attn_fwd(C.byref(a), None) == -1
    a, keep = _valid_args()
    keep[0].ldvt = 4                                            # not a multiple of 8
    assert lib.aid_ip_attn_fwd(C.byref(a), None) == -3
    a, keep = _valid_args()
    a.out = 0x4002                                              # 16-byte alignment
    assert lib.aid_ip_attn_fwd(C.byref(a), None) == -3


def test_processor_refuses_segments_outside_their_form():
    """aid_processor_ip_fwd checks everything before its first launch: with a NULL workspace a well-formed call gets as far as
    AID_ERR_WORKSPACE (-4) without a GPU, a malformed one is refused before."""
    lib = _lib.load()
    a = _lib.AidProcessorArgs()
    for f in ("x", "ctx", "wq", "wk", "wv", "wo", "y"):
        setattr(a, f, 0x1000)
    a.n_frames, a.s, a.l, a.c, a.cc, a.heads, a.mode, a.dtype, a.n_ctx = 2, 64, 77, 128, 64, 2, 0, 1, 2
    base = lib.aid_processor_workspace_bytes(C.byref(a))
    assert base > 0
    _, segs = _valid_args()
    call = lambda n=1, p=segs: lib.aid_processor_ip_fwd(C.byref(a), p, n, None)      # noqa: E731
    assert lib.aid_processor_ip_fwd(None, segs, 1, None) == -1
    assert call() == -4 and call(0, None) == -4
    a.attn_bias = 0x1000                                                # allowed with segments (covers the text launch)
    assert call() == -4
    a.attn_bias = None
    assert call(-1) == -1 and call(0) == -1 and call(1, None) == -1
    a.dtype = 2                                                         # float32
    assert call() == -2
    a.dtype, a.ctx = 1, None                                            # self-attention
    assert call() == -1
    a.ctx, a.mode, a.coef = 0x1000, 2, 0x1000                           # an interpolated call
    assert call() == -1
    a.mode = 0
    a.ip, a.wk_ip, a.wv_ip, a.n_ip, a.t_ip, a.ip_mode, a.ip_stride = 0x1000, 0x1000, 0x1000, 2, 4, 2, 4 * 64   # the ip_* branch beside them
    assert lib.aid_processor_fwd(C.byref(a), None) == -4 and call() == -1
    a.ip, a.ip_mode = None, 0
    segs[0].t = 0
    assert call() == -1
    segs[0].t, segs[0].ldvt = 4, 4
    assert call() == -3
    assert lib.aid_processor_workspace_bytes(C.byref(a)) == base        # the workspace never depends on the segments


# ---- segment construction against a recording stand-in ------------------------------------------------------------------------------
class _Recorder:
    """Stands in for libaid_hip.so: records the image segments the Python layer hands to the entry points."""

    def __init__(self):
        self.calls, self.launches, self.gemms = [], [], 0

    @staticmethod
    def _segments(ptr, n, s):
        arr = (_lib.AidIpSegment * n).from_address(ptr) if n else []
        out = []
        for e in arr:
            w = None if not e.row_weight else torch.tensor(list((C.c_float * s).from_address(e.row_weight)), dtype=torch.float64)
            out.append(dict(k=e.k, vt=e.vt, t=e.t, ldvt=e.ldvt, n_rows=e.n_rows, scale=e.scale, k_fs=e.k_fs, vt_fs=e.vt_fs, w=w))
        return out

    def aid_gemm_nt(self, arr, n, dt, stream):
        self.gemms += 1
        return 0

    def aid_processor_workspace_bytes(self, ref):
        return 64

    def aid_processor_fwd(self, ref, stream):
        return self.aid_processor_ip_fwd(ref, None, 0, stream)

    def aid_processor_ip_fwd(self, ref, segs, n, stream):
        a = ref._obj
        self.calls.append(dict(segs=self._segments(segs, n, a.s), ip=a.ip, bias=a.attn_bias, mode=a.mode))
        return 0

    def aid_ip_attn_fwd(self, ref, stream):
        a = ref._obj
        self.launches.append(self._segments(a.segments, a.n_segments, a.s))
        return 0


@pytest.fixture
def rec(monkeypatch):
    lib = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(ops, "_require_gpu", lambda *ts: torch.device("cpu"))
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "workspace", lambda nbytes, dev: torch.empty(nbytes, dtype=torch.uint8))
    processors.clear_weight_caches()
    yield lib
    processors.clear_weight_caches()


DT = torch.float16
N, S, CW, HEADS, CC = 2, 64, 64, 2, 32


def _layer(scales, tokens=(4, 16)):
    attn = aid_amd.AttnShim(CW, HEADS, CC, dtype=DT)
    proc = aid_amd.HipIPAdapterAttnProcessor(hidden_size=CW, cross_attention_dim=CC, num_tokens=tokens, scale=scales, dtype=DT)
    return attn, proc


def _inputs(s=S):
    g = torch.Generator().manual_seed(0)
    return torch.randn(N, s, CW, generator=g).to(DT), torch.randn(N, 7, CC, generator=g).to(DT)


def test_unmasked_adapters_fold_images_into_one_segment_each(rec):
    attn, proc = _layer([0.5, 0.25])
    x, text = _inputs()
    ip = [torch.zeros(N, 3, 4, CC, dtype=DT), torch.zeros(N, 16, CC, dtype=DT)]      # [B, E, T, Cc] and [B, T, Cc]
    proc(attn, x, encoder_hidden_states=(text, ip))
    (call,) = rec.calls
    assert call["ip"] is None and call["mode"] == 0
    assert [(s["t"], s["ldvt"], s["n_rows"], s["scale"], s["w"]) for s in call["segs"]] == [(12, 16, N, 0.5, None), (16, 16, N, 0.25, None)]
    assert call["segs"][0]["k_fs"] == 12 * CW and call["segs"][0]["vt_fs"] == CW * 16
    # the projections are cached for the run: a second call projects nothing, clear_weight_caches() drops them
    n_gemm = rec.gemms
    proc(attn, x, encoder_hidden_states=(text, ip))
    assert rec.gemms == n_gemm and rec.calls[1]["segs"][0]["k"] == call["segs"][0]["k"]
    processors.clear_weight_caches()
    proc(attn, x, encoder_hidden_states=(text, ip))
    assert rec.gemms == 2 * n_gemm
    ip[0].add_(1)                                                                       # an in-place edit of the embeddings misses
    proc(attn, x, encoder_hidden_states=(text, ip))
    assert rec.gemms == 2 * n_gemm + n_gemm // 2


def test_layers_that_share_the_embeddings_keep_their_own_projections(rec):
    """diffusers hands the SAME ip_hidden_states tensors to every cross-attention layer and each layer has its own to_k_ip / to_v_ip:
    after the first step no layer projects again, and a layer's entry is not evicted by its neighbour's."""
    (attn_a, proc_a), (attn_b, proc_b) = _layer([0.5, 0.25]), _layer([0.5, 0.25])
    x, text = _inputs()
    ip = [torch.zeros(N, 4, CC, dtype=DT), torch.zeros(N, 2, 16, CC, dtype=DT)]
    masks = [None, torch.ones(1, 2, 8, 8)]
    gen0 = processors.cache_generation()
    for proc, attn in ((proc_a, attn_a), (proc_b, attn_b)):
        proc(attn, x, encoder_hidden_states=(text, ip), ip_adapter_masks=masks)
    first, gen1 = rec.gemms, processors.cache_generation()
    assert first == 2 * 3 and gen1 > gen0                   # per layer: one unmasked adapter + two masked images
    for _ in range(2):
        for proc, attn in ((proc_a, attn_a), (proc_b, attn_b)):
            proc(attn, x, encoder_hidden_states=(text, ip), ip_adapter_masks=masks)
    assert rec.gemms == first and processors.cache_generation() == gen1
    assert [s["k"] for s in rec.calls[0]["segs"]] == [s["k"] for s in rec.calls[4]["segs"]]
    assert [s["k"] for s in rec.calls[0]["segs"]] != [s["k"] for s in rec.calls[1]["segs"]]


def test_single_unmasked_adapter_keeps_the_ip_form(rec):
    attn, proc = _layer([0.5], tokens=(4,))
    x, text = _inputs()
    proc(attn, x, encoder_hidden_states=(text, [torch.zeros(N, 4, CC, dtype=DT)]))
    (call,) = rec.calls
    assert call["segs"] == [] and call["ip"] is not None


def test_attention_mask_with_image_embeddings_takes_the_segment_form(rec):
    attn, proc = _layer([0.5], tokens=(4,))
    x, text = _inputs()
    mask = torch.zeros(N, 1, 7, dtype=DT)
    proc(attn, x, encoder_hidden_states=(text, [torch.zeros(N, 4, CC, dtype=DT)]), attention_mask=mask)
    (call,) = rec.calls
    assert call["ip"] is None and call["bias"] is not None and [s["t"] for s in call["segs"]] == [4]


@pytest.mark.parametrize("hw,s", [((64, 64), 64), ((48, 80), 60)])
def test_masked_adapter_is_one_segment_per_image_with_the_downsampled_weights(rec, hw, s):
    attn, proc = _layer([0.5, [0.3, 0.7]])
    x, text = _inputs(s)
    g = torch.Generator().manual_seed(1)
    m0 = (torch.rand(1, 1, *hw, generator=g) > 0.5).float()
    m1 = torch.rand(1, 2, *hw, generator=g)
    ip = [torch.zeros(N, 1, 4, CC, dtype=DT), torch.zeros(N, 2, 16, CC, dtype=DT)]
    proc(attn, x, encoder_hidden_states=(text, ip), ip_adapter_masks=[m0, m1])
    (call,) = rec.calls
    segs = call["segs"]
    assert [(v["t"], round(v["scale"], 6)) for v in segs] == [(4, 0.5), (16, 0.3), (16, 0.7)]      # a scalar scale repeats, a list is per image
    for v, (m, e) in zip(segs, ((m0, 0), (m1, 0), (m1, 1))):
        want = torch.from_numpy(row_weights(m[:, e], s, DT))
        assert v["w"].shape == (s,) and torch.equal(v["w"], want)
    # a single tensor [adapters, images, H, W] is split along dim 0
    rec.calls.clear()
    proc.scale[1] = 0.3
    both = torch.cat([m0, m0 * 0.5], 0)
    ip1 = [ip[0], torch.zeros(N, 1, 16, CC, dtype=DT)]
    proc(attn, x, encoder_hidden_states=(text, ip1), ip_adapter_masks=both)
    assert [v["t"] for v in rec.calls[0]["segs"]] == [4, 16]
    assert torch.equal(rec.calls[0]["segs"][1]["w"], torch.from_numpy(row_weights(both[1:2, 0], s, DT)))


def test_a_query_count_the_mask_grid_cannot_tile_is_zero_padded():
    """48 x 80 -> S = 62: mh = int(sqrt(62 / (80 / 48))) = 6 does not divide 62, so mh = 7, mw = 62 // 7 = 8: 56 cells, six zero rows
    behind them.  (mh mw = mh (S // mh) <= S: diffusers' truncate branch cannot be reached.)"""
    m = 0.5 + 0.5 * torch.rand(1, 48, 80, generator=torch.Generator().manual_seed(2))
    w = processors.mask_row_weights(m, 62, DT, torch.device("cpu"))
    assert w.shape == (62,) and w.dtype == torch.float32
    assert torch.equal(w.double(), torch.from_numpy(row_weights(m, 62, DT)))
    assert torch.all(w[56:] == 0) and torch.all(w[:56] > 0)


def test_zero_scales_are_skipped_and_long_lists_run_as_several_launches(rec):
    attn, proc = _layer([0.0, [0.0, 0.0], 0.5], tokens=(4, 4, 4))
    x, text = _inputs()
    ip = [torch.zeros(N, 1, 4, CC, dtype=DT), torch.zeros(N, 2, 4, CC, dtype=DT), torch.zeros(N, 1, 4, CC, dtype=DT)]
    masks = [None, torch.ones(1, 2, 8, 8), None]
    proc(attn, x, encoder_hidden_states=(text, ip), ip_adapter_masks=masks)
    assert [v["scale"] for v in rec.calls[0]["segs"]] == [0.5]
    # ops.ip_attn_accumulate: 11 segments = launches of 8 + 3, in order
    q, out = torch.zeros(N, S, CW, dtype=DT), torch.zeros(N, S, CW, dtype=DT)
    k, vt = torch.zeros(1, 4, CW, dtype=DT), torch.zeros(1, CW, 8, dtype=DT)
    ops.ip_attn_accumulate(q, out, [dict(k=k, vt=vt, scale=float(i)) for i in range(11)], HEADS)
    assert [[v["scale"] for v in l] for l in rec.launches] == [[float(i) for i in range(8)], [8.0, 9.0, 10.0]]
    assert all(v["n_rows"] == 1 for l in rec.launches for v in l)


def test_mask_validation_raises_the_value_errors_of_diffusers(rec):
    attn, proc = _layer([0.5, 0.5])
    x, text = _inputs()
    ip = [torch.zeros(N, 1, 4, CC, dtype=DT), torch.zeros(N, 2, 16, CC, dtype=DT)]
    m0, m1 = torch.ones(1, 1, 8, 8), torch.ones(1, 2, 8, 8)
    call = lambda masks, ip_=ip: proc(attn, x, encoder_hidden_states=(text, ip_), ip_adapter_masks=masks)    # noqa: E731
    with pytest.raises(ValueError, match="Length of ip_adapter_masks"):
        call([m0])
    with pytest.raises(ValueError, match="Length of ip_adapter_masks"):
        call([m0, m1], ip[:1])
    with pytest.raises(ValueError, match="should be a tensor with shape"):
        call([m0, m1[0]])
    with pytest.raises(ValueError, match="should be a tensor with shape"):
        call([m0, "mask"])
    with pytest.raises(ValueError, match="does not match number of ip images"):
        call([m0, m0])
    proc.scale[1] = [0.5, 0.5, 0.5]
    with pytest.raises(ValueError, match="does not match number of scales"):
        call([m0, m1])
    assert rec.calls == []


def test_float32_storage_says_that_the_segment_form_is_16_bit(rec):
    attn = aid_amd.AttnShim(CW, HEADS, CC, dtype=torch.float32)
    proc = aid_amd.HipIPAdapterAttnProcessor(hidden_size=CW, cross_attention_dim=CC, num_tokens=(4, 16), scale=[0.5, 0.5])
    x, text = torch.zeros(N, S, CW), torch.zeros(N, 7, CC)
    ip = [torch.zeros(N, 4, CC), torch.zeros(N, 16, CC)]
    with pytest.raises(NotImplementedError, match="float16 / bfloat16"):
        proc(attn, x, encoder_hidden_states=(text, ip))
    with pytest.raises(NotImplementedError, match="float16 / bfloat16"):
        ops.ip_attn_accumulate(torch.zeros(N, S, CW), torch.zeros(N, S, CW),
                               [dict(k=torch.zeros(1, 4, CW), vt=torch.zeros(1, CW, 8))], HEADS)
    assert rec.calls == [] and rec.gemms == 0
    # no segment to build (every scale 0): the text attention with its mask, as before
    proc.scale[:] = [0.0, 0.0]
    proc(attn, x, encoder_hidden_states=(text, ip), attention_mask=torch.zeros(N, 1, 7))
    (call,) = rec.calls
    assert call["segs"] == [] and call["ip"] is None and call["bias"] is not None


def test_ip_attn_accumulate_checks_the_head_count(rec):
    q = torch.zeros(N, S, 3 * 64 + 8, dtype=DT)
    with pytest.raises(ValueError, match="heads"):
        ops.ip_attn_accumulate(q, q.clone(), [dict(k=torch.zeros(1, 4, 200, dtype=DT), vt=torch.zeros(1, 200, 8, dtype=DT))], 3)


# ---- resources ---------------------------------------------------------------------------------------------------------------------
def test_kernel_resources_no_scratch_and_the_waves_the_launcher_assumes():
    """aid_attn_ip.resources.txt at this commit: d = 40: 133 VGPRs, d = 64: 137 (three waves per SIMD, <= 168); d = 80: 179, d = 160: 202
    (two waves, <= 256); no AGPRs, no scratch, no VGPR or SGPR spills in any of the eight instantiations."""
    path = os.path.join(CSRC, "aid_attn_ip.resources.txt")
    if not os.path.exists(path):
        pytest.skip(f"{path} not there: build the library first (python -c 'import __graft_entry__ as g; g.build()')")
    tab = {}
    for blk in open(path).read().split("Name: ")[1:]:
        num = lambda key: int(re.search(re.escape(key) + r": (\d+)", blk).group(1))   # noqa: E731
        m = re.search(r"aid_ip_attn_kernelIDF16(b?)_?Li(\d+)E", blk.split()[0])
        assert m, blk.split()[0]
        tab[("bf16" if m.group(1) else "f16", int(m.group(2)))] = dict(
            vgpr=num("VGPRs"), agpr=num("AGPRs"), scratch=num("ScratchSize [bytes/lane]"), occ=num("Occupancy [waves/SIMD]"),
            spill=num("VGPRs Spill"), sgpr_spill=num("SGPRs Spill"))
    assert sorted(tab) == sorted((dt, d) for dt in ("f16", "bf16") for d in (40, 64, 80, 160))
    for (dt, d), r in tab.items():
        assert r["scratch"] == 0 and r["spill"] == 0 and r["sgpr_spill"] == 0 and r["agpr"] == 0, (dt, d, r)
        assert r["occ"] >= (3 if d <= 64 else 2), (dt, d, r)
        assert r["vgpr"] <= (168 if d <= 64 else 256), (dt, d, r)
