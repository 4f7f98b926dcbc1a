"""CPU checks of the unmerged-LoRA support (aid_amd/lora.py, ABI v9): PEFT's forward decision table, the packed operands, their
cache, the refusals and the host-side argument checks of the library.  The GPU parity is in test_hip_lora.py."""
import ctypes

import pytest
import torch
from torch import nn

import aid_amd
from aid_amd import _lib, lora, processors
from peft_double import LoraLinear, effective_weight, wrap_attention


def _layer(adapters=(("a", 8, 16.0), ("b", 4, 4.0)), dtype=torch.float32, seed=0):
    torch.manual_seed(seed)
    lin = LoraLinear(nn.Linear(96, 80, bias=False, dtype=dtype))
    g = torch.Generator().manual_seed(seed)
    for name, r, alpha in adapters:
        lin.update_layer(name, r, alpha, generator=g)
    lin.set_adapter([a[0] for a in adapters])
    return lin


def _expected(lin, x):
    """base + sum over lora.active(): what the library is handed, evaluated in fp64."""
    y = x.double() @ lin.base_layer.weight.double().T
    for a, s in lora.active(lin):
        y = y + s * (x.double() @ lin.lora_A[a].weight.double().T) @ lin.lora_B[a].weight.double().T
    return y


def test_decision_table_matches_the_wrapper_forward():
    lin = _layer().double()
    x = torch.randn(5, 96, dtype=torch.float64)
    assert torch.allclose(_expected(lin, x), lin(x))                 # every active adapter
    lin.set_adapter("b")
    assert [a for a, _ in lora.active(lin)] == ["b"]
    assert torch.allclose(_expected(lin, x), lin(x))
    lin.set_adapter(["b", "missing"])                                # an active name without lora_A is skipped, like PEFT
    assert [a for a, _ in lora.active(lin)] == ["b"]
    lin.enable_adapters(False)
    assert lora.active(lin) == []
    assert torch.allclose(_expected(lin, x), lin(x))                 # disabled: base only
    lin.enable_adapters(True)
    lin.set_adapter(["a", "b"])
    lin.merge()
    assert lora.active(lin) == []                                    # merged: nothing added twice
    assert torch.allclose(x @ lin.base_layer.weight.T, lin(x))
    lin.enable_adapters(False)                                       # disabled + merged: unmerged first, as PEFT's forward does
    w_merged = lin.base_layer.weight.detach().clone()
    assert lora.active(lin) == [] and not lin.merged
    assert not torch.allclose(w_merged, lin.base_layer.weight)
    assert torch.allclose(lin(x), x @ lin.base_layer.weight.T)


def test_plain_layers_have_no_adapters():
    assert lora.active(nn.Linear(8, 8)) == []
    assert not lora.is_lora_layer(nn.Linear(8, 8))
    assert lora.is_lora_layer(_layer())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_packing_folds_scaling_and_pads_the_rank(dtype):
    lin = _layer()
    p = lora.pack(lin, dtype, torch.device("cpu"))
    assert p.rank == 64 and p.a.shape == (64, 96) and p.b.shape == (80, 64)
    assert p.a.dtype == dtype and p.b.dtype == dtype
    assert p.a.is_contiguous() and p.b.is_contiguous()
    assert torch.count_nonzero(p.a[12:]) == 0 and torch.count_nonzero(p.b[:, 12:]) == 0      # 8 + 4 rows, zero padding
    sa, sb = lin.scaling["a"], lin.scaling["b"]
    assert torch.equal(p.a[:8], (lin.lora_A["a"].weight.float() * sa).to(dtype))
    assert torch.equal(p.a[8:12], (lin.lora_A["b"].weight.float() * sb).to(dtype))
    assert torch.equal(p.b[:, :8], lin.lora_B["a"].weight.to(dtype))
    delta = p.b.double() @ p.a.double()
    want = effective_weight(lin) - lin.base_layer.weight.double()
    eps = {torch.float16: 2e-3, torch.bfloat16: 2e-2, torch.float32: 1e-6}[dtype]
    assert float((delta - want).norm() / want.norm()) < eps


def test_rank_rounds_up_in_64_steps_and_is_bounded():
    assert lora.pack(_layer((("a", 64, 64.0),)), torch.float16, torch.device("cpu")).rank == 64
    assert lora.pack(_layer((("a", 64, 64.0), ("b", 1, 1.0))), torch.float16, torch.device("cpu")).rank == 128
    with pytest.raises(NotImplementedError):
        lora.pack(_layer((("a", 300, 1.0), ("b", 300, 1.0))), torch.float16, torch.device("cpu"))


def test_pack_cache_misses_on_scale_adapter_switch_and_inplace_edit():
    lin = _layer()
    cpu = torch.device("cpu")
    p0 = lora.pack(lin, torch.float16, cpu)
    assert lora.pack(lin, torch.float16, cpu) is p0
    gen = processors.cache_generation()
    lin.set_scale("a", 0.5)                                          # cross_attention_kwargs["scale"] -> scale_layer / set_scale
    p1 = lora.pack(lin, torch.float16, cpu)
    assert p1 is not p0 and not torch.equal(p1.a, p0.a)
    assert processors.cache_generation() > gen                       # a rebuild is a new shared tensor (loop.fork_join)
    lin.set_adapter("b")
    p2 = lora.pack(lin, torch.float16, cpu)
    assert p2 is not p1 and torch.count_nonzero(p2.a[4:]) == 0
    with torch.no_grad():
        lin.lora_A["b"].weight.mul_(2.0)                             # in-place edit: bumps _version
    p3 = lora.pack(lin, torch.float16, cpu)
    assert p3 is not p2 and torch.allclose(p3.a[:4].float(), 2 * p2.a[:4].float(), rtol=1e-2)
    assert lora.pack(lin, torch.bfloat16, cpu) is not p3             # dtype is part of the key
    p4 = lora.pack(lin, torch.float16, cpu)
    processors.clear_weight_caches()
    assert lora.pack(lin, torch.float16, cpu) is not p4


def test_processor_operands_stack_the_down_weights_per_input():
    attn = aid_amd.AttnShim(128, 2, 64, dtype=torch.float16, device="cpu")
    wrap_attention(attn, {"a": (8, 8.0)}, targets=("to_q", "to_k", "to_v", "to_out"))
    la = lora.args(attn, torch.float16, torch.device("cpu"), cross=True)
    assert la.ranks == (64, 64, 64, 64)
    assert la.down_x.shape == (64, 128) and la.down_ctx.shape == (128, 64) and la.down_o.shape == (64, 128)
    assert lora.args(attn, torch.float16, torch.device("cpu"), cross=True) is la
    assert lora.args(attn, torch.float16, torch.device("cpu"), cross=True, kv=False).ranks == (64, 0, 0, 64)
    self_attn = aid_amd.AttnShim(128, 2, None, dtype=torch.float16, device="cpu")
    wrap_attention(self_attn, {"a": (8, 8.0), "b": (16, 4.0)}, targets=("to_k", "to_v"))
    la = lora.args(self_attn, torch.float16, torch.device("cpu"), cross=False)
    assert la.ranks == (0, 64, 64, 0) and la.down_x.shape == (128, 128) and la.down_ctx is None and la.down_o is None
    assert lora.args(aid_amd.AttnShim(128, 2, None, dtype=torch.float16, device="cpu"), torch.float16, torch.device("cpu"),
                     cross=False) is None


def test_refusals():
    lin = _layer()
    lin.use_dora["a"] = True
    with pytest.raises(NotImplementedError, match="DoRA"):
        lora.active(lin)
    lin = _layer()
    lin.lora_bias["b"] = True
    with pytest.raises(NotImplementedError, match="lora_bias"):
        lora.active(lin)
    lin = _layer()
    lin.lora_dropout["a"] = nn.Dropout(0.1)
    lin.eval()
    assert len(lora.active(lin)) == 2                                # dropout is the identity in eval mode
    lin.train()
    with pytest.raises(NotImplementedError, match="dropout"):
        lora.active(lin)
    old = nn.Linear(8, 8)
    old.lora_layer = nn.Linear(8, 8)
    with pytest.raises(NotImplementedError, match="lora_layer"):
        lora.active(old)
    ip = aid_amd.HipIPAdapterAttnProcessor(hidden_size=64, cross_attention_dim=32)
    ip.to_k_ip[0] = LoraLinear(ip.to_k_ip[0])
    with pytest.raises(NotImplementedError, match="to_k_ip"):
        processors._no_ip_lora(ip)


def _proc_args(**kw):
    a = _lib.AidProcessorArgs()
    for f in ("x", "wq", "wk", "wv", "wo", "y"):
        setattr(a, f, 0x1000)
    a.n_frames, a.s, a.c, a.heads, a.mode, a.dtype = 7, 4096, 640, 10, 0, 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_workspace_is_unchanged_at_rank_zero_and_grows_with_ranks():
    lib = _lib.load()
    base = 4 * 7 * 4096 * 640 * 2
    assert lib.aid_processor_workspace_bytes(ctypes.byref(_proc_args())) == base
    a = _proc_args(lora_r_q=64, lora_r_k=128, lora_r_v=64, lora_r_o=64, lora_down_x=0x1000, lora_down_o=0x1000,
                   lora_up_q=0x1000, lora_up_k=0x1000, lora_up_v=0x1000, lora_up_o=0x1000)
    assert lib.aid_processor_workspace_bytes(ctypes.byref(a)) == base + 7 * 4096 * (256 + 64) * 2
    a = _proc_args(ctx=0x1000, cc=768, l=77, n_ctx=7, lora_r_k=64, lora_r_v=64, lora_down_ctx=0x1000, lora_up_k=0x1000,
                   lora_up_v=0x1000)
    cross0 = lib.aid_processor_workspace_bytes(ctypes.byref(_proc_args(ctx=0x1000, cc=768, l=77, n_ctx=7)))
    assert lib.aid_processor_workspace_bytes(ctypes.byref(a)) == cross0 + ((7 * 77 * 128 * 2 + 255) // 256) * 256


def test_processor_lora_argument_refusals():
    lib = _lib.load()
    ws = lambda a: lib.aid_processor_workspace_bytes(ctypes.byref(a))      # noqa: E731  0 = refused by the host-side checks
    ok = dict(lora_r_q=64, lora_down_x=0x1000, lora_up_q=0x1000)
    assert ws(_proc_args(**ok)) > 0
    assert ws(_proc_args(**dict(ok, lora_r_q=96))) == 0                     # rank % 64
    assert ws(_proc_args(**dict(ok, lora_r_q=576))) == 0                    # rank > 512
    assert ws(_proc_args(**dict(ok, lora_up_q=0))) == 0                     # missing operand
    assert ws(_proc_args(**dict(ok, ln_eps=1e-5, ln_wq=0x1000, ln_const=0x1000))) == 0      # LoRA with the folded LayerNorm
    assert ws(_proc_args(**dict(ok, ln_eps=1e-5))) > 0                                      # ... but not with the unfolded one
    cross = dict(ctx=0x1000, cc=768, l=77, n_ctx=7, k_cached=0x1000, vt_cached=0x1000)
    assert ws(_proc_args(**cross, **ok)) > 0                                # LoRA on q with cached keys: fine
    assert ws(_proc_args(**cross, lora_r_k=64, lora_down_ctx=0x1000, lora_up_k=0x1000)) == 0   # on k with cached keys: refused


def test_gemm_lora_argument_refusals():
    lib = _lib.load()
    p = (_lib.AidGemmProblem * 1)()
    q = p[0]
    q.a = q.b = q.c = 0x1000
    q.m, q.n, q.k, q.lda, q.ldb, q.ldc, q.batch = 64, 64, 64, 64, 64, 64, 1
    q.lr_a = q.lr_b = 0x1000
    q.lr_lda = q.lr_ldb = 128
    q.lr_k = 96                                                             # lr_k % 64
    assert lib.aid_gemm_nt(p, 1, 0, None) == -3
    q.lr_k = 576                                                            # > 512
    assert lib.aid_gemm_nt(p, 1, 0, None) == -3
    q.lr_k, q.lr_lda = 64, 68                                               # ld % 8
    assert lib.aid_gemm_nt(p, 1, 0, None) == -3
    q.lr_lda = 64
    q.ln_stats = q.ln_colsum = q.ln_shift = 0x1000                          # with the folded LayerNorm
    q.ln_side = 1
    assert lib.aid_gemm_nt(p, 1, 0, None) == -1
    q.ln_stats = None
    q.lr_b = None                                                           # missing operand
    assert lib.aid_gemm_nt(p, 1, 0, None) == -1


# ---- pipelines: cross_attention_kwargs / lora_scale and the LoRA loader methods of from_pipe -------------------------------------------
class _CakUNet(torch.nn.Module):
    """RecordingUNet (tests/test_pipelines.py) that also takes and records diffusers' ``cross_attention_kwargs``."""

    def __new__(cls):
        from test_pipelines import RecordingUNet

        class U(RecordingUNet):
            def forward(self, sample, t, encoder_hidden_states=None, added_cond_kwargs=None, return_dict=False,
                        cross_attention_kwargs=None):
                self.cak = getattr(self, "cak", []) + [cross_attention_kwargs]
                return super().forward(sample, t, encoder_hidden_states, added_cond_kwargs, return_dict)
        return U()


def _recording_encoder(seen):
    g = torch.Generator().manual_seed(3)
    embs = (torch.randn(1, 7, 12, generator=g), torch.randn(1, 7, 12, generator=g))

    def enc(prompt, negative_prompt=None, **kw):
        seen.append((prompt, kw))
        return embs
    return enc


def test_interpolate_single_forwards_cross_attention_kwargs_and_lora_scale():
    from aid_amd.pipelines import DDIMSchedulerLite, InterpolationStableDiffusionPipeline
    unet, seen = _CakUNet(), []
    pipe = InterpolationStableDiffusionPipeline(unet, DDIMSchedulerLite(), encode_prompt=_recording_encoder(seen))
    pipe.load_aid(t=0.5, is_fused=True, atype="fused_inner")
    g = torch.Generator().manual_seed(0)
    l0, l1 = torch.randn(1, 4, 4, 4, generator=g), torch.randn(1, 4, 4, 4, generator=g)
    cak = {"scale": 0.5}
    pipe.interpolate_single(0.3, prompt_start="a", prompt_end="b", latent_start=l0, latent_end=l1, num_inference_steps=3,
                            output_type="latent", cross_attention_kwargs=cak)
    assert unet.cak == [cak] * 6                                   # every UNet call of the run, conditional and unconditional
    assert seen == [("a", {"lora_scale": 0.5}), ("b", {"lora_scale": 0.5})]
    unet.cak, seen[:] = [], []
    pipe.interpolate_single(0.3, prompt_start="a", prompt_end="b", latent_start=l0, latent_end=l1, num_inference_steps=2,
                            output_type="latent")
    assert unet.cak == [None] * 4 and seen == [("a", {}), ("b", {})]     # without kwargs: the calls the pipelines always made


@pytest.mark.parametrize("batched", [True, False])
def test_n_frame_interpolate_forwards_cross_attention_kwargs(batched):
    from aid_amd.pipelines import DDIMSchedulerLite, InterpolationStableDiffusionPipeline
    unet, seen = _CakUNet(), []
    pipe = InterpolationStableDiffusionPipeline(unet, DDIMSchedulerLite(), encode_prompt=_recording_encoder(seen))
    g = torch.Generator().manual_seed(1)
    l0, l1 = torch.randn(1, 4, 4, 4, generator=g), torch.randn(1, 4, 4, 4, generator=g)
    cak = {"scale": 0.25}
    pipe.interpolate(l0, l1, prompt_start="a", prompt_end="b", guide_prompt="c", size=5, num_inference_steps=2,
                     batched_cfg=batched, output_type="latent", cross_attention_kwargs=cak)
    assert unet.cak and all(c is cak for c in unet.cak)
    assert [kw for _, kw in seen] == [{"lora_scale": 0.25}] * 3


def test_from_pipe_exposes_the_lora_loader_and_drops_weight_caches():
    calls = []

    class FakeVae:
        config = type("C", (), {"scaling_factor": 0.18215})()

    class FakePipe:
        unet, scheduler, vae = object(), object(), FakeVae()
        _execution_device = "cpu"

        def encode_prompt(self, *a, **k):
            calls.append(("encode_prompt", k.get("lora_scale")))
            return ("cond", "uncond")

        def __getattr__(self, name):
            if name in ("load_lora_weights", "set_adapters", "fuse_lora", "unfuse_lora", "enable_lora", "disable_lora"):
                return lambda *a, **k: calls.append((name, a, k)) or name
            raise AttributeError(name)

    pipe = aid_amd.InterpolationStableDiffusionPipeline.from_pipe(FakePipe())
    pipe._encode_prompt("p", None, lora_scale=0.7)
    assert calls[-1] == ("encode_prompt", 0.7)
    for name, a, k in (("load_lora_weights", ("some/lora",), {"adapter_name": "x"}), ("set_adapters", (["x", "y"],),
                                                                                     {"adapter_weights": [0.5, 1.0]}),
                       ("fuse_lora", (), {"lora_scale": 0.8}), ("unfuse_lora", (), {}), ("enable_lora", (), {}),
                       ("disable_lora", (), {})):
        gen = processors.cache_generation()
        assert getattr(pipe, name)(*a, **k) == name
        assert calls[-1] == (name, a, k) and processors.cache_generation() > gen       # clear_weight_caches() ran
    with pytest.raises(RuntimeError, match="from_pipe"):
        aid_amd.InterpolationStableDiffusionPipeline(object(), object()).load_lora_weights("x")
