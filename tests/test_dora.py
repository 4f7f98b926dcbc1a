"""CPU checks of the DoRA support (aid_amd/lora.py, ABI v10): which DoRA layers are accepted and which are refused, the pack's gain and
its cache key, and the host-side argument checks of the library.  The GPU parity is in test_hip_dora.py.  The gain itself has no CPU
path (``ops.dora_gain`` is one HIP launch); the cache tests put a torch stand-in in its place."""
import ctypes

import pytest
import torch
from torch import nn

import aid_amd
from aid_amd import _lib, lora, ops, processors
from peft_dora_double import DoraLinear, effective_weight_dora, wrap_attention_dora

CPU = torch.device("cpu")


def _layer(adapters=(("a", 8, 16.0),), dtype=torch.float32, seed=0, dora=True, bias=False):
    torch.manual_seed(seed)
    lin = DoraLinear(nn.Linear(96, 80, bias=bias, dtype=dtype))
    g = torch.Generator().manual_seed(seed)
    for name, r, alpha in adapters:
        lin.update_layer(name, r, alpha, generator=g, use_dora=dora)
    lin.set_adapter([a[0] for a in adapters])
    return lin


def _torch_gain(w, a_pack, b_pack, magnitude):
    """What aid_dora_gain computes, in torch (fp32 like the kernel)."""
    t = w.float() + b_pack.float() @ a_pack.float()
    return magnitude.float() / torch.linalg.norm(t, dim=1)


@pytest.fixture
def cpu_gain(monkeypatch):
    monkeypatch.setattr(ops, "dora_gain", _torch_gain)
    yield
    lora.clear()


# ---- the double itself: PEFT's DoRA forward is  x (g o (W + s B A))^T + bias ------------------------------------------------------------
def test_double_forward_equals_the_effective_weight():
    lin = _layer(bias=True).double()
    x = torch.randn(5, 96, dtype=torch.float64)
    w = effective_weight_dora(lin)
    assert torch.allclose(lin(x), x @ w.T + lin.base_layer.bias, atol=1e-12)
    g = lin.lora_magnitude_vector["a"].weight / lin._weight_norm("a")
    assert float(g.min()) < 0.8 and float(g.max()) > 1.2               # a dropped gain shows
    w0 = lin.base_layer.weight.detach().clone()
    lin.merge()
    assert torch.allclose(lin.base_layer.weight, w, atol=1e-12) and torch.allclose(lin(x), x @ w.T + lin.base_layer.bias)
    lin.unmerge()
    assert torch.allclose(lin.base_layer.weight, w0, atol=1e-12)


# ---- decision table --------------------------------------------------------------------------------------------------------------------
def test_accepted_dora_layer():
    lin = _layer()
    assert lora.active(lin) == [("a", 2.0)]
    mag = lora.dora_magnitude(lin, "a")
    assert mag is lin.lora_magnitude_vector["a"].weight and tuple(mag.shape) == (80,)
    plain = _layer(dora=False)
    assert lora.active(plain) == [("a", 2.0)] and lora.dora_magnitude(plain, "a") is None


def test_flag_without_magnitude_vector_is_refused():
    lin = _layer()
    del lin.lora_magnitude_vector["a"]
    with pytest.raises(NotImplementedError, match="DoRA"):
        lora.active(lin)
    lin = _layer()
    lin.lora_magnitude_vector["a"].weight = nn.Parameter(torch.ones(80, 1))        # not [out]
    with pytest.raises(NotImplementedError, match="DoRA"):
        lora.active(lin)
    lin = _layer()
    del lin.lora_magnitude_vector                                                   # a wrapper class without the attribute
    with pytest.raises(NotImplementedError, match="DoRA"):
        lora.active(lin)


def test_dora_with_another_active_adapter_is_refused():
    lin = _layer((("a", 8, 16.0), ("b", 4, 4.0)))
    with pytest.raises(NotImplementedError, match="DoRA"):
        lora.active(lin)
    lin.use_dora["b"] = False                                                       # DoRA + plain LoRA: refused too
    with pytest.raises(NotImplementedError, match="DoRA"):
        lora.active(lin)
    lin.set_adapter("a")                                                            # alone: accepted
    assert lora.active(lin) == [("a", 2.0)]
    lin.set_adapter("b")                                                            # the plain one alone: plain LoRA
    assert lora.active(lin) == [("b", 1.0)] and lora.dora_magnitude(lin, "b") is None
    lin.set_adapter(["a", "missing"])                                               # a name without lora_A does not count
    assert lora.active(lin) == [("a", 2.0)]


def test_fan_in_fan_out_and_quantised_bases_are_refused():
    lin = _layer()
    lin.fan_in_fan_out = True
    with pytest.raises(NotImplementedError, match="DoRA.*fan_in_fan_out"):
        lora.active(lin)
    lin = _layer()
    lin.base_layer.weight = nn.Parameter(torch.zeros(80, 96, dtype=torch.int8), requires_grad=False)
    with pytest.raises(NotImplementedError, match="DoRA.*quantised"):
        lora.active(lin)
    lin = _layer()
    lin.base_layer.weight.quant_state = object()                                    # bitsandbytes' marker on a packed weight
    with pytest.raises(NotImplementedError, match="DoRA.*quantised"):
        lora.active(lin)
    lin = _layer()
    lin.base_layer.weight = nn.Parameter(torch.zeros(80 * 96 // 2, 1), requires_grad=False)     # a packed 4-bit weight's shape
    with pytest.raises(NotImplementedError, match="DoRA.*quantised"):
        lora.active(lin)


def test_lora_bias_stays_refused():
    lin = _layer()
    lin.lora_bias["a"] = True
    with pytest.raises(NotImplementedError, match="lora_bias"):
        lora.active(lin)


def test_merged_and_disabled_dora_layers_are_base_only():
    lin = _layer()
    lin.enable_adapters(False)
    assert lora.active(lin) == []
    lin.enable_adapters(True)
    w0 = lin.base_layer.weight.detach().clone()
    lin.merge()
    assert lora.active(lin) == [] and lora.pack(lin, torch.float32, CPU) is None
    lin.enable_adapters(False)                                                      # disabled and merged: unmerged first
    assert lora.active(lin) == [] and not lin.merged
    assert torch.allclose(lin.base_layer.weight, w0, atol=1e-6)


def test_cpu_tensors_still_raise():
    with pytest.raises(RuntimeError, match="no CPU path"):
        lora.pack(_layer(), torch.float32, CPU)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.dora_gain(torch.zeros(8, 8), torch.zeros(64, 8), torch.zeros(8, 64), torch.zeros(8))


def test_ip_projections_stay_refused():
    ip = aid_amd.HipIPAdapterAttnProcessor(hidden_size=64, cross_attention_dim=32)
    ip.to_v_ip[0] = DoraLinear(ip.to_v_ip[0])
    with pytest.raises(NotImplementedError, match="to_v_ip"):
        processors._no_ip_lora(ip)


# ---- the pack: gain and cache key ------------------------------------------------------------------------------------------------------
def test_pack_holds_the_gain_of_the_packed_operands(cpu_gain):
    lin = _layer()
    p = lora.pack(lin, torch.float32, CPU)
    assert p.rank == 64 and p.gain.dtype == torch.float32 and tuple(p.gain.shape) == (80,)
    w = effective_weight_dora(lin)
    want = lin.lora_magnitude_vector["a"].weight.double() / torch.linalg.norm(
        lin.base_layer.weight.double() + p.b.double() @ p.a.double(), dim=1)
    assert torch.allclose(p.gain.double(), want, rtol=1e-5)
    assert torch.allclose(p.gain.double().view(-1, 1) * (lin.base_layer.weight.double() + p.b.double() @ p.a.double()), w, rtol=1e-5)
    assert lora.pack(_layer(dora=False), torch.float32, CPU).gain is None           # plain LoRA: no gain


def test_pack_key_follows_magnitude_weight_factors_and_scale(cpu_gain):
    lin = _layer()
    p0 = lora.pack(lin, torch.float32, CPU)
    assert lora.pack(lin, torch.float32, CPU) is p0

    def rebuilt(prev):
        gen = processors.cache_generation()
        p = lora.pack(lin, torch.float32, CPU)
        assert p is not prev and p.key != prev.key and processors.cache_generation() > gen
        return p
    with torch.no_grad():
        lin.lora_magnitude_vector["a"].weight.mul_(1.5)                             # the magnitude's version
    p1 = rebuilt(p0)
    assert torch.allclose(p1.gain, 1.5 * p0.gain) and torch.equal(p1.a, p0.a)
    with torch.no_grad():
        lin.base_layer.weight.mul_(2.0)                                             # W's version
    p2 = rebuilt(p1)
    assert not torch.allclose(p2.gain, p1.gain)
    with torch.no_grad():
        lin.lora_B["a"].weight.mul_(0.5)                                            # a factor
    p3 = rebuilt(p2)
    assert not torch.allclose(p3.gain, p2.gain)
    lin.set_scale("a", 0.25)                                                        # a new scale
    p4 = rebuilt(p3)
    assert not torch.allclose(p4.gain, p3.gain)
    with torch.no_grad():
        lin.base_layer.weight = nn.Parameter(lin.base_layer.weight.detach().clone())        # a replaced weight: another address
    rebuilt(p4)
    plain = _layer(dora=False)                                                      # plain LoRA keys as before: W is not part of them
    q0 = lora.pack(plain, torch.float32, CPU)
    with torch.no_grad():
        plain.base_layer.weight.mul_(2.0)
    assert lora.pack(plain, torch.float32, CPU) is q0


def test_processor_operands_carry_the_four_gains(cpu_gain):
    attn = aid_amd.AttnShim(128, 2, 64, dtype=torch.float32, device="cpu")
    wrap_attention_dora(attn, {"a": (8, 8.0)}, targets=("to_q", "to_v"))
    la = lora.args(attn, torch.float32, CPU, cross=True)
    assert la.ranks == (64, 0, 64, 0)
    assert la.gains[0] is not None and la.gains[2] is not None and la.gains[1] is None and la.gains[3] is None
    assert tuple(la.gains[0].shape) == (128,) and la.gains[0].dtype == torch.float32
    assert lora.args(attn, torch.float32, CPU, cross=True) is la
    with torch.no_grad():
        attn.to_v.lora_magnitude_vector["a"].weight.mul_(1.5)
    lb = lora.args(attn, torch.float32, CPU, cross=True)
    assert lb is not la and lb.gains[0] is la.gains[0] and torch.allclose(lb.gains[2], 1.5 * la.gains[2])
    pk, pv = lora.kv_packs(attn, torch.float32, CPU)                                # what the text-K/V cache keys on
    assert pk is None and pv.key == lb.key[3]
    assert lora.args(attn, torch.float32, CPU, cross=True, kv=False).gains[2] is None


# ---- host-side argument checks of the library (no launch) --------------------------------------------------------------------------------
def test_abi_version_and_new_fields():
    assert _lib.load().aid_abi_version() == 10 == _lib.AID_ABI_VERSION
    names = [f for f, _ in _lib.AidGemmProblem._fields_]
    assert names[-1] == "lr_row_scale" and "lr_scale_side" in names and "reserved1" not in names
    assert [f for f, _ in _lib.AidProcessorArgs._fields_][-4:] == ["lora_gain_q", "lora_gain_k", "lora_gain_v", "lora_gain_o"]


def _problem():
    p = (_lib.AidGemmProblem * 1)()
    q = p[0]
    q.a = q.b = q.c = 0x1000
    q.m, q.n, q.k, q.lda, q.ldb, q.ldc, q.batch = 64, 64, 64, 64, 64, 64, 1
    q.lr_a = q.lr_b = 0x1000
    q.lr_k = q.lr_lda = q.lr_ldb = 64
    q.lr_row_scale, q.lr_scale_side = 0x1000, 2
    return p, q


def test_gemm_row_scale_argument_refusals():
    lib = _lib.load()
    p, q = _problem()
    q.lr_k = 0                                                                       # a gain without a segment
    assert lib.aid_gemm_nt(p, 1, 0, None) == -1
    for side in (0, 3, -1):
        p, q = _problem()
        q.lr_scale_side = side
        assert lib.aid_gemm_nt(p, 1, 0, None) == -1
    p, q = _problem()
    q.lr_row_scale = 0x1002                                                          # not 4-byte aligned
    assert lib.aid_gemm_nt(p, 1, 0, None) == -1
    p, q = _problem()
    q.ln_stats = q.ln_colsum = q.ln_shift = 0x1000                                   # with the folded LayerNorm (refused for any segment)
    q.ln_side = 1
    assert lib.aid_gemm_nt(p, 1, 0, None) == -1
    p, q = _problem()
    q.trans_rows, q.m, q.ldc, q.lr_scale_side = 8, 64, 8, 1                          # transposed C: the weight operand is b
    assert lib.aid_gemm_nt(p, 1, 0, None) == -1


def test_dora_gain_argument_refusals():
    lib = _lib.load()
    ok = dict(w=0x1000, a=0x1000, b=0x1000, mag=0x1000, gain=0x1000, n_out=80, n_in=96, ldw=96, rank=64, dtype=0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.aid_dora_gain(a["w"], a["a"], a["b"], a["mag"], a["gain"], a["n_out"], a["n_in"], a["ldw"], a["rank"], a["dtype"], None)
    for f in ("w", "a", "b", "mag", "gain"):
        assert call(**{f: None}) == -1
    assert call(dtype=7) == -2
    assert call(n_in=100, ldw=104) == -3                                             # n_in % 8
    assert call(rank=96) == -3 and call(rank=576) == -3                              # rank % 64, rank <= 512
    assert call(ldw=88) == -3                                                        # ldw < n_in
    assert call(w=0x1008) == -3 and call(mag=0x1008) == -3                           # 16-byte bases
    assert call(gain=0x1002) == -1


def _proc_args(**kw):
    a = _lib.AidProcessorArgs()
    for f in ("x", "wq", "wk", "wv", "wo", "y"):
        setattr(a, f, 0x1000)
    a.n_frames, a.s, a.c, a.heads, a.mode, a.dtype = 7, 4096, 640, 10, 0, 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_processor_gain_needs_the_matching_rank():
    lib = _lib.load()
    ws = lambda a: lib.aid_processor_workspace_bytes(ctypes.byref(a))      # noqa: E731  0 = refused by the host-side checks
    ok = dict(lora_r_q=64, lora_down_x=0x1000, lora_up_q=0x1000)
    plain = ws(_proc_args(**ok))
    assert plain > 0 and ws(_proc_args(**ok, lora_gain_q=0x1000)) == plain           # a gain needs no workspace
    assert ws(_proc_args(**ok, lora_gain_k=0x1000)) == 0                             # a gain on a projection without a rank
    assert ws(_proc_args(lora_gain_o=0x1000)) == 0
    assert ws(_proc_args(**ok, lora_gain_q=0x1002)) == 0                             # alignment
