"""Precision of the float32 attention core (AidAttnArgs.f32_split / AidProcessorArgs.f32_attn_split): the host side, without a GPU.

``ops.set_f32_attn_precision("high")`` permits the core to form its two products from bf16 halves (aid_attn_f32x3_kernel,
csrc/aid_f32x3.hip).  The switch is package-level, defaults to "highest" and is independent of the torch global that the projection
GEMMs follow.  Here: how the Python layer turns the keyword / the package setting into the fields, that 16-bit calls never carry them,
that neither switch moves the other's field, the struct slots, the library's argument checks (pure host code), the graph keys, the CPU
restatement the GPU tests compare against, and the new instantiations' resource table.  Every test that changes the package setting or
the torch global restores it."""
import ctypes as C
import os
import re

import pytest
import torch

import aid_amd
from aid_amd import _lib, ops
from aid_amd.loop import AidDenoiseLoop
from aid_amd.pipelines import _PassGraphs
from split_attn_ref import refs
from util import rel_l2

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "attention-interpolation-diffusion_amd", "csrc")


@pytest.fixture
def attn_precision():
    """Sets the package setting for one test and puts the previous value back."""
    prev = ops.get_f32_attn_precision()
    yield ops.set_f32_attn_precision
    ops.set_f32_attn_precision(prev)


@pytest.fixture
def precision():
    prev = torch.get_float32_matmul_precision()
    yield torch.set_float32_matmul_precision
    torch.set_float32_matmul_precision(prev)


def test_names_map_to_codes_and_the_default_is_exact():
    assert ops.F32_ATTN_PRECISIONS == {"highest": 0, "high": 1}
    assert ops.get_f32_attn_precision() == "highest" and aid_amd.get_f32_attn_precision() == "highest"
    assert ops.f32_attn_split_code("highest") == 0 and ops.f32_attn_split_code("high") == 1
    for bad in ("HIGH", "medium", "low", "", 1, 0.5):
        with pytest.raises(ValueError):
            ops.f32_attn_split_code(bad)
        with pytest.raises(ValueError):
            ops.set_f32_attn_precision(bad)
    with pytest.raises(ValueError):
        ops.set_f32_attn_precision(None)
    assert ops.get_f32_attn_precision() == "highest"        # a refused value changes nothing


def test_none_reads_the_package_setting_at_call_time(attn_precision, precision):
    assert ops.f32_attn_split_code() == 0 and ops.f32_attn_split_code(None) == 0
    attn_precision("high")
    assert ops.get_f32_attn_precision() == "high" and ops.f32_attn_split_code() == 1
    assert ops.f32_attn_split_code("highest") == 0          # an explicit value wins over the setting
    aid_amd.set_f32_attn_precision("highest")               # the package-level names are the same functions
    assert ops.f32_attn_split_code() == 0
    precision("high")                                       # the torch global does not move it ...
    assert ops.f32_attn_split_code() == 0 and ops.f32_split_code() == 1
    precision("highest")
    attn_precision("high")                                  # ... and it does not move the projections' code
    assert ops.f32_split_code() == 0 and ops.f32_attn_split_code() == 1


class _FakeLib:
    """Stands in for libaid_hip.so: records the structs the Python layer hands to the entry points."""

    def __init__(self):
        self.attn, self.proc = [], []

    def aid_attn_fwd(self, ref, stream):
        self.attn.append((int(ref._obj.dtype), int(ref._obj.f32_split)))
        return 0

    def aid_lerp_kv(self, *a):
        return 0

    def aid_processor_workspace_bytes(self, ref):
        return 64

    def aid_processor_fwd(self, ref, stream):
        self.proc.append((int(ref._obj.dtype), int(ref._obj.f32_split), int(ref._obj.f32_attn_split)))
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


def _qkv(dtype):
    return torch.zeros(3, 8, 64, dtype=dtype), torch.zeros(3, 8, 64, dtype=dtype), torch.zeros(3, 64, 8, dtype=dtype)


def test_attn_fwd_fills_the_field(fake, attn_precision, precision):
    q, k, vt = _qkv(torch.float32)
    ops.attn_fwd(q, k, vt, 1, l=8)
    ops.attn_fwd(q, k, vt, 1, l=8, f32_attn_precision="high")
    precision("high")                                       # the projections' global is not the core's switch
    ops.attn_fwd(q, k, vt, 1, l=8)
    precision("highest")
    attn_precision("high")
    ops.attn_fwd(q, k, vt, 1, l=8)
    ops.attn_fwd(q, k, vt, 1, l=8, f32_attn_precision="highest")
    coef = torch.tensor([0.0, 0.5, 1.0])
    ops.attn_fwd(q, k, vt, 1, l=8, mode="inner", fused=True, coef=coef)
    assert fake.attn == [(_lib.DTYPE_F32, c) for c in (0, 1, 0, 1, 0, 1)]
    with pytest.raises(ValueError):
        ops.attn_fwd(q, k, vt, 1, l=8, f32_attn_precision="medium")


def test_processor_fwd_fills_both_fields_independently(fake, attn_precision, precision):
    x, w = torch.zeros(3, 8, 64), torch.zeros(64, 64)
    call = lambda **kw: ops.processor_fwd(x, None, w, w, w, w, None, 1, **kw)      # noqa: E731
    call()
    call(f32_attn_precision="high")
    call(f32_precision="high")
    call(f32_precision="high", f32_attn_precision="high")
    attn_precision("high")
    call()
    call(f32_attn_precision="highest")
    precision("high")
    call()
    attn_precision("highest")
    call()
    want = [(0, 0), (0, 1), (1, 0), (1, 1), (0, 1), (0, 0), (1, 1), (1, 0)]
    assert fake.proc == [(_lib.DTYPE_F32, p, a) for p, a in want]
    with pytest.raises(ValueError):
        call(f32_attn_precision="tf32")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_16bit_calls_never_set_the_fields(fake, attn_precision, dtype):
    attn_precision("high")
    q, k, vt = _qkv(dtype)
    ops.attn_fwd(q, k, vt, 1, l=8)
    ops.attn_fwd(q, k, vt, 1, l=8, f32_attn_precision="high")
    assert [s for _, s in fake.attn] == [0, 0]
    x, w = torch.zeros(3, 8, 64, dtype=dtype), torch.zeros(64, 64, dtype=dtype)
    ops.processor_fwd(x, None, w, w, w, w, None, 1)
    ops.processor_fwd(x, None, w, w, w, w, None, 1, f32_attn_precision="high")
    assert [(p, a) for _, p, a in fake.proc] == [(0, 0), (0, 0)]
    with pytest.raises(ValueError):                         # a bad value is an error whatever the dtype
        ops.attn_fwd(q, k, vt, 1, l=8, f32_attn_precision="tf32")
    with pytest.raises(ValueError):
        ops.processor_fwd(x, None, w, w, w, w, None, 1, f32_attn_precision="tf32")


def test_renamed_fields_take_the_reserved_slots_and_are_zero_by_default():
    """AidAttnArgs.f32_split sits where reserved0 sat (behind seg_executed, in front of bias), AidProcessorArgs.f32_attn_split where
    reserved2 sat (behind seg_executed, in front of ln_wq): layouts and ABI version unchanged, a zeroed struct keeps exact products."""
    A, Pr = _lib.AidAttnArgs, _lib.AidProcessorArgs
    na, npr = [f for f, _ in A._fields_], [f for f, _ in Pr._fields_]
    assert na[na.index("seg_executed") + 1] == "f32_split" and na[na.index("f32_split") + 1] == "bias"
    assert A.f32_split.offset == A.seg_executed.offset + 4 and A.f32_split.size == 4 and A.bias.offset == A.f32_split.offset + 4
    assert npr[npr.index("seg_executed") + 1] == "f32_attn_split" and npr[npr.index("f32_attn_split") + 1] == "ln_wq"
    assert Pr.f32_attn_split.offset == Pr.seg_executed.offset + 4 and Pr.f32_attn_split.size == 4
    assert Pr.ln_wq.offset == Pr.f32_attn_split.offset + 4
    assert Pr.f32_split.offset == Pr.cu_share.offset + 4      # the projections' field stays where it was
    assert A().f32_split == 0 and Pr().f32_attn_split == 0
    assert "reserved0" not in na and "reserved2" not in npr and na.count("f32_split") == 1 and npr.count("f32_attn_split") == 1
    assert _lib.AID_ABI_VERSION == 10


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    return _lib.load()


def _attn_struct(split, dtype):
    a = _lib.AidAttnArgs()
    a.q = a.k = a.vt = a.out = 0x1000
    a.n_frames, a.n_kv, a.s, a.l, a.heads, a.d = 3, 3, 64, 64, 8, 40
    a.ldq = a.ldk = a.ldo = 320
    a.ldvt = 64
    a.q_fs = a.k_fs = a.vt_fs = a.o_fs = 64 * 320
    a.dtype, a.softmax_scale, a.out_scale, a.f32_split = dtype, 40 ** -0.5, 1.0, split
    return a


def test_library_refuses_bad_field_values_before_any_launch():
    """Argument checks are host code: a value outside {0, 1}, or a non-zero value with a 16-bit dtype, is AID_ERR_ARG (-1) from
    aid_attn_fwd, aid_processor_fwd and aid_processor_workspace_bytes (0 bytes); the split needs no workspace."""
    lib = _lib_or_skip()
    assert lib.aid_abi_version() == _lib.AID_ABI_VERSION
    for bad in (2, -1, 255):
        assert lib.aid_attn_fwd(C.byref(_attn_struct(bad, _lib.DTYPE_F32)), None) == -1
    for dt in (_lib.DTYPE_F16, _lib.DTYPE_BF16):
        assert lib.aid_attn_fwd(C.byref(_attn_struct(1, dt)), None) == -1
    a = _lib.AidProcessorArgs()
    a.x = a.wq = a.wk = a.wv = a.wo = a.y = 0x1000
    a.n_frames, a.s, a.c, a.heads, a.dtype = 3, 64, 320, 8, _lib.DTYPE_F32
    n0 = lib.aid_processor_workspace_bytes(C.byref(a))
    assert n0 > 0
    a.f32_attn_split = 1
    assert lib.aid_processor_workspace_bytes(C.byref(a)) == n0
    a.f32_split = 1                                         # both switches: still the same workspace
    assert lib.aid_processor_workspace_bytes(C.byref(a)) == n0
    a.f32_split = 0
    for bad in (2, -1, 255):
        a.f32_attn_split = bad
        assert lib.aid_processor_workspace_bytes(C.byref(a)) == 0 and lib.aid_processor_fwd(C.byref(a), None) == -1
    for dt in (_lib.DTYPE_F16, _lib.DTYPE_BF16):
        a.f32_attn_split, a.dtype = 1, dt
        assert lib.aid_processor_workspace_bytes(C.byref(a)) == 0 and lib.aid_processor_fwd(C.byref(a), None) == -1
        a.f32_attn_split = 0
        assert lib.aid_processor_workspace_bytes(C.byref(a)) > 0
    a.dtype, a.f32_attn_split, a.f32_split = _lib.DTYPE_F32, 1, 2          # the projections' check is still there
    assert lib.aid_processor_workspace_bytes(C.byref(a)) == 0 and lib.aid_processor_fwd(C.byref(a), None) == -1


def test_graph_keys_carry_the_attention_precision(attn_precision, precision):
    for key_of in (_PassGraphs._key, AidDenoiseLoop._graph_key):
        attn_precision("highest")
        k0 = key_of("cond_aid")
        attn_precision("high")
        k1 = key_of("cond_aid")
        precision("high")
        k2 = key_of("cond_aid")
        precision("highest")
        attn_precision("highest")
        assert len({k0, k1, k2}) == 3 and key_of("cond_aid") == k0 and key_of("uncond") != k0


def test_text_kv_cache_is_not_keyed_by_the_attention_precision(monkeypatch, attn_precision):
    """The cache holds projections only: one entry serves both settings."""
    from aid_amd import processors as P
    calls = []

    def project(ctx, wk, wv, **kw):
        calls.append(ops.get_f32_attn_precision())
        return torch.zeros(1), torch.zeros(1)
    monkeypatch.setattr(ops, "project_kv", project)
    P.clear_text_kv_cache()
    attn = aid_amd.AttnShim(64, 1, 64, dtype=torch.float32)
    ctx = torch.zeros(3, 8, 64)
    try:
        for setting in ("highest", "high", "highest"):
            attn_precision(setting)
            assert P._text_kv(attn, ctx, ctx, None, attn.to_k.weight, attn.to_v.weight) is not None
        assert calls == ["highest"]
    finally:
        P.clear_text_kv_cache()


def test_cpu_restatement_of_the_split_core():
    """The reference the GPU tests use: the three-term core sits ~6e-6 from the fp64 attention, the high halves alone ~3e-3."""
    g = torch.Generator().manual_seed(0)
    s, l, d, h = 64, 200, 64, 2
    q, k, v = (torch.randn(2, r, h * d, generator=g) for r in (s, l, l))
    ref3, ref1, ref64 = refs(q, k, v, h)
    e3, e1 = rel_l2(ref3, ref64), rel_l2(ref1, ref64)
    assert ref3.shape == (2, s, h * d) and e3 < 1e-5 and e1 > 1e-3 and e3 < e1 / 50, (e3, e1)


def test_split_attention_kernel_resources():
    """Every instantiation aid_attn_f32x3_kernel<D, TWO>: no scratch, no VGPR / SGPR spills, at least the waves per SIMD its
    __launch_bounds__ asks (d 40 / 64: 2; d 80: 2, OUTER 1; d 160: 1) and VGPRs + AGPRs <= 512 / that."""
    path = os.path.join(CSRC, "aid_f32x3.resources.txt")
    if not os.path.exists(path):
        pytest.skip(f"{path} not there: build the library first (python -c 'import __graft_entry__ as g; g.build()')")
    tab = {}
    for blk in open(path).read().split("Name: ")[1:]:
        num = lambda key: int(re.search(re.escape(key) + r": (\d+)", blk).group(1))   # noqa: E731
        m = re.search(r"aid_attn_f32x3_kernelILi(\d+)ELb(\d)E", blk.split()[0])
        if m:
            tab[(int(m.group(1)), bool(int(m.group(2))))] = dict(
                vgpr=num("VGPRs"), agpr=num("AGPRs"), scratch=num("ScratchSize [bytes/lane]"), occ=num("Occupancy [waves/SIMD]"),
                spill=num("VGPRs Spill"), sgpr_spill=num("SGPRs Spill"))
    want = {(40, False): 2, (40, True): 2, (64, False): 2, (64, True): 2, (80, False): 2, (80, True): 1, (160, False): 1, (160, True): 1}
    assert sorted(tab) == sorted(want), sorted(tab)
    for key, waves in want.items():
        r = tab[key]
        assert r["scratch"] == 0 and r["spill"] == 0 and r["sgpr_spill"] == 0, (key, r)
        assert r["occ"] >= waves and r["vgpr"] + r["agpr"] <= 512 // waves, (key, r)
