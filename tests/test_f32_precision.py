"""float32 matmul precision (AidGemmProblem.f32_split / AidProcessorArgs.f32_split): the host side, without a GPU.

``torch.set_float32_matmul_precision("high")`` is honoured by the projection GEMMs of float32 tensors (csrc/aid_f32x3.hip).  Here:
how the Python layer turns the keyword / the torch global into the field, that 16-bit calls never carry it, that the text-K/V cache
and the pass graphs are keyed by it, the library's argument checks (pure host code), the CPU restatement the GPU tests compare
against, and the new object's resource table.  Every test that touches the torch global restores it."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import aid_amd
from aid_amd import _lib, ops
from aid_amd import processors as P
from aid_amd.pipelines import _PassGraphs
from split_ref import refs, split
from util import rel_l2

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "attention-interpolation-diffusion_amd", "csrc")


@pytest.fixture
def precision():
    """Sets the torch global for one test and puts the previous value back (a leaked "high" would change later fp32 tests)."""
    prev = torch.get_float32_matmul_precision()
    yield torch.set_float32_matmul_precision
    torch.set_float32_matmul_precision(prev)


def test_precision_names_map_to_the_field():
    assert ops.f32_split_code("highest") == 0 and ops.f32_split_code("high") == 1 and ops.f32_split_code("medium") == 1
    for bad in ("HIGH", "low", "", 1, 0.5):
        with pytest.raises(ValueError):
            ops.f32_split_code(bad)


def test_none_reads_the_torch_global_at_call_time(precision):
    precision("highest")
    assert ops.f32_split_code() == 0 and ops.f32_split_code(None) == 0
    precision("high")
    assert ops.f32_split_code() == 1
    precision("medium")
    assert ops.f32_split_code() == 1
    assert ops.f32_split_code("highest") == 0          # an explicit value wins over the global


class _FakeLib:
    """Stands in for libaid_hip.so: records the structs the Python layer hands to the two entry points."""

    def __init__(self):
        self.gemm, self.proc = [], []

    def aid_gemm_nt(self, arr, n, dtype, stream):
        self.gemm.append((dtype, [int(arr[i].f32_split) for i in range(n)]))
        return 0

    def aid_processor_workspace_bytes(self, ref):
        return 64

    def aid_processor_fwd(self, ref, stream):
        self.proc.append((int(ref._obj.dtype), int(ref._obj.f32_split)))
        return 0


@pytest.fixture
def fake(monkeypatch):
    """ops on CPU tensors with the library call replaced: only the struct filling runs."""
    lib = _FakeLib()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(ops, "_require_gpu", lambda *ts: torch.device("cpu"))
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "workspace", lambda nbytes, dev: torch.empty(nbytes, dtype=torch.uint8))
    return lib


def _problem(dtype, **kw):
    a, b, c = torch.zeros(8, 8, dtype=dtype), torch.zeros(8, 8, dtype=dtype), torch.zeros(8, 8, dtype=dtype)
    return dict(a=a, b=b, c=c, m=8, n=8, k=8, lda=8, ldb=8, ldc=8, **kw)


def test_gemm_nt_fills_the_field_per_problem(fake, precision):
    precision("highest")
    ops.gemm_nt([_problem(torch.float32), _problem(torch.float32, f32_precision="high"), _problem(torch.float32, f32_precision="medium"),
                 _problem(torch.float32, f32_precision="highest"), _problem(torch.float32, f32_precision=None)])
    assert fake.gemm[-1] == (_lib.DTYPE_F32, [0, 1, 1, 0, 0])
    precision("high")                                   # None / absent follow the global, explicit values do not
    ops.gemm_nt([_problem(torch.float32), _problem(torch.float32, f32_precision="highest"), _problem(torch.float32, f32_precision=None)])
    assert fake.gemm[-1] == (_lib.DTYPE_F32, [1, 0, 1])
    with pytest.raises(ValueError):
        ops.gemm_nt([_problem(torch.float32, f32_precision="fast")])


def test_linear_and_project_kv_pass_the_keyword(fake, precision):
    precision("highest")
    x, w = torch.zeros(4, 8), torch.zeros(8, 8)
    ops.linear(x, w)
    assert fake.gemm[-1][1] == [0]
    ops.linear(x, w, f32_precision="high")
    assert fake.gemm[-1][1] == [1]
    e = torch.zeros(2, 8, 8)
    ops.project_kv(e, w, w, f32_precision="medium")
    assert fake.gemm[-1][1] == [1, 1]
    ops.project_kv(e, w, w)
    assert fake.gemm[-1][1] == [0, 0]
    precision("high")
    ops.linear(x, w)
    ops.project_kv(e, w, w)
    assert fake.gemm[-2][1] == [1] and fake.gemm[-1][1] == [1, 1]
    with pytest.raises(ValueError):
        ops.linear(x, w, f32_precision="tf32")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_16bit_calls_never_set_the_field(fake, precision, dtype):
    precision("high")
    x, w = torch.zeros(3, 8, 64, dtype=dtype), torch.zeros(64, 64, dtype=dtype)
    ops.linear(x, w)
    ops.linear(x, w, f32_precision="high")
    ops.project_kv(x, w, w, f32_precision="medium")
    assert all(split == [0] * len(split) for _, split in fake.gemm) and len(fake.gemm) == 3
    ops.processor_fwd(x, None, w, w, w, w, None, 1)
    ops.processor_fwd(x, None, w, w, w, w, None, 1, f32_precision="high")
    assert [s for _, s in fake.proc] == [0, 0]
    with pytest.raises(ValueError):                     # a bad value is an error whatever the dtype
        ops.processor_fwd(x, None, w, w, w, w, None, 1, f32_precision="tf32")


def test_processor_fwd_fills_the_field(fake, precision):
    x, w = torch.zeros(3, 8, 64), torch.zeros(64, 64)
    precision("highest")
    ops.processor_fwd(x, None, w, w, w, w, None, 1)
    ops.processor_fwd(x, None, w, w, w, w, None, 1, f32_precision="high")
    precision("high")
    ops.processor_fwd(x, None, w, w, w, w, None, 1)
    ops.processor_fwd(x, None, w, w, w, w, None, 1, f32_precision="highest")
    assert fake.proc == [(_lib.DTYPE_F32, 0), (_lib.DTYPE_F32, 1), (_lib.DTYPE_F32, 1), (_lib.DTYPE_F32, 0)]


def test_text_kv_cache_is_keyed_by_the_precision(monkeypatch, precision):
    """Entries projected under one setting do not serve the other; each setting keeps its own entry."""
    calls = []

    def project(ctx, wk, wv, **kw):
        calls.append(torch.get_float32_matmul_precision())
        return torch.zeros(1), torch.zeros(1)
    monkeypatch.setattr(ops, "project_kv", project)
    P.clear_text_kv_cache()
    attn = aid_amd.AttnShim(64, 1, 64, dtype=torch.float32)
    ctx = torch.zeros(3, 8, 64)
    try:
        for setting in ("highest", "high", "highest", "high", "medium"):
            precision(setting)
            assert P._text_kv(attn, ctx, ctx, None, attn.to_k.weight, attn.to_v.weight) is not None
        assert calls == ["highest", "high"]             # ("medium" runs the same split as "high": the same entry)
        half = aid_amd.AttnShim(64, 1, 64, dtype=torch.float16)
        ctx16 = torch.zeros(3, 8, 64, dtype=torch.float16)
        for setting in ("highest", "high"):             # 16-bit projections do not depend on the setting: one entry
            precision(setting)
            P._text_kv(half, ctx16, ctx16, None, half.to_k.weight, half.to_v.weight)
        assert len(calls) == 3
    finally:
        P.clear_text_kv_cache()


def test_pass_graph_key_carries_the_precision(precision):
    precision("highest")
    k0 = _PassGraphs._key("cond_aid")
    precision("high")
    k1 = _PassGraphs._key("cond_aid")
    precision("medium")
    k2 = _PassGraphs._key("cond_aid")
    precision("highest")
    assert k0 != k1 and k1 == k2 and k0 == _PassGraphs._key("cond_aid") and k0 != _PassGraphs._key("uncond")


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    return _lib.load()


def _gemm_struct(split):
    p = (_lib.AidGemmProblem * 1)()
    q = p[0]
    q.a = q.b = q.c = 0x1000
    q.m, q.n, q.k, q.lda, q.ldb, q.ldc, q.batch = 64, 64, 64, 64, 64, 64, 1
    q.f32_split = split
    return p


def test_library_refuses_bad_field_values_before_any_launch():
    """Argument checks are host code: a value outside {0, 1}, or a non-zero value with a 16-bit dtype, is AID_ERR_ARG (-1)."""
    lib = _lib_or_skip()
    assert lib.aid_abi_version() == _lib.AID_ABI_VERSION
    for bad in (2, -1, 255):
        assert lib.aid_gemm_nt(_gemm_struct(bad), 1, _lib.DTYPE_F32, None) == -1
    for dt in (_lib.DTYPE_F16, _lib.DTYPE_BF16):
        assert lib.aid_gemm_nt(_gemm_struct(1), 1, dt, None) == -1
    a = _lib.AidProcessorArgs()
    a.x = a.wq = a.wk = a.wv = a.wo = a.y = 0x1000
    a.n_frames, a.s, a.c, a.heads, a.dtype = 3, 64, 320, 8, _lib.DTYPE_F32
    assert lib.aid_processor_workspace_bytes(C.byref(a)) > 0
    a.f32_split = 1
    assert lib.aid_processor_workspace_bytes(C.byref(a)) > 0       # the split needs no workspace of its own
    n1 = lib.aid_processor_workspace_bytes(C.byref(a))
    a.f32_split = 0
    assert lib.aid_processor_workspace_bytes(C.byref(a)) == n1
    a.f32_split = 2
    assert lib.aid_processor_workspace_bytes(C.byref(a)) == 0 and lib.aid_processor_fwd(C.byref(a), None) == -1
    a.f32_split, a.dtype = 1, _lib.DTYPE_BF16
    assert lib.aid_processor_workspace_bytes(C.byref(a)) == 0 and lib.aid_processor_fwd(C.byref(a), None) == -1


def test_new_fields_take_the_reserved_slots_and_are_zero_by_default():
    """f32_split sits where reserved0 / reserved1 sat (behind cu_share): the struct layouts and the ABI version do not change, and a
    caller that zeroed the reserved fields keeps getting exact products."""
    for cls in (_lib.AidGemmProblem, _lib.AidProcessorArgs):
        names = [f for f, _ in cls._fields_]
        assert names[names.index("cu_share") + 1] == "f32_split" and names.count("f32_split") == 1
        assert cls.f32_split.offset == cls.cu_share.offset + 4 and cls.f32_split.size == 4
        assert cls().f32_split == 0
    assert "reserved0" not in [f for f, _ in _lib.AidGemmProblem._fields_]
    assert "reserved1" not in [f for f, _ in _lib.AidProcessorArgs._fields_]


def test_cpu_restatement_of_the_split():
    """The reference the GPU tests use: both halves are bf16 numbers, hi + lo carries x to ~2^-17, and the three-term product sits
    ~4e-6 from the fp64 product — 500x closer than one bf16 product."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(64, 320, generator=g)
    hi, lo = split(x)
    for h in (hi, lo):
        t = torch.from_numpy(h).float()
        assert torch.equal(t.bfloat16().float(), t)
    assert np.abs(hi + lo - x.numpy().astype(np.float64)).max() <= 2.0 ** -16 * np.abs(x.numpy()).max()
    b = torch.randn(96, 320, generator=g)
    ref3, ref1, ref64 = refs(x, b)
    e3, e1 = rel_l2(ref3, ref64), rel_l2(ref1, ref64)
    assert e3 < 1e-5 and e1 > 1e-3 and e3 < e1 / 50, (e3, e1)


def test_split_kernel_resources():
    """No scratch, no spills, at least two waves per SIMD, both tile sizes present."""
    path = os.path.join(CSRC, "aid_f32x3.resources.txt")
    if not os.path.exists(path):
        pytest.skip(f"{path} not there: build the library first (python -c 'import __graft_entry__ as g; g.build()')")
    tab = {}
    for blk in open(path).read().split("Name: ")[1:]:
        num = lambda key: int(re.search(re.escape(key) + r": (\d+)", blk).group(1))   # noqa: E731
        tab[blk.split()[0]] = dict(vgpr=num("VGPRs"), agpr=num("AGPRs"), scratch=num("ScratchSize [bytes/lane]"),
                                   occ=num("Occupancy [waves/SIMD]"), spill=num("VGPRs Spill"), sgpr_spill=num("SGPRs Spill"))
    kern = {s: r for s, r in tab.items() if "aid_gemm_f32x3_kernel" in s}
    assert sorted(int(re.search(r"kernelILi(\d+)E", s).group(1)) for s in kern) == [64, 128], list(tab)
    for sym, r in kern.items():
        assert r["scratch"] == 0 and r["spill"] == 0 and r["sgpr_spill"] == 0 and r["occ"] >= 2, (sym, r)
        assert r["vgpr"] + r["agpr"] <= 256, (sym, r)      # two waves per SIMD of the 512-register file
