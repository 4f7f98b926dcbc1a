"""End-point K / V^T store: the host side, without a GPU.

The two new structs against the header as gcc lays it out, every argument error of ``aid_endpoint_rows`` / ``aid_processor_ep_fwd``
with a NULL stream (all checks run before the first launch), ``EndpointStore`` bookkeeping against a stand-in library that records
what the Python layer hands over, the refusals of the processors, and the copy kernel's row of the build's resource table."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import aid_amd
from aid_amd import _lib, endpoint_store, ops, processors
from aid_amd.endpoint_store import SIGNATURE_FIELDS, EndpointStore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "attention-interpolation-diffusion_amd", "csrc")
HEADER = open(os.path.join(ROOT, "include", "aid_hip.h")).read()


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_the_version_stays():
    assert re.search(r"^int\s+aid_endpoint_rows\s*\(const AidEndpointRows\* args", HEADER, flags=re.M)
    assert re.search(r"^int\s+aid_processor_ep_fwd\s*\(const AidProcessorArgs\* args", HEADER, flags=re.M)
    assert re.search(r"^size_t\s+aid_processor_ep_workspace_bytes\s*\(const AidProcessorArgs\* args", HEADER, flags=re.M)
    new = {"aid_endpoint_rows", "aid_processor_ep_fwd", "aid_processor_ep_workspace_bytes"}
    assert new <= set(_lib.ABI_SYMBOLS)
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in new)
    for name, val in (("AID_EP_PUT", _lib.EP_PUT), ("AID_EP_GET", _lib.EP_GET), ("AID_EP_RECORD", _lib.EP_RECORD),
                      ("AID_EP_REPLAY", _lib.EP_REPLAY)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, HEADER).group(1)) == val
    assert lib.aid_abi_version() == 10 and _lib.AID_ABI_VERSION == 10 and re.search(r"#define AID_ABI_VERSION 10\b", HEADER)


def test_new_structs_match_the_header_layout(tmp_path):
    structs = {"AidEndpointRows": _lib.AidEndpointRows, "AidEndpointStore": _lib.AidEndpointStore,
               "AidProcessorArgs": _lib.AidProcessorArgs}
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
    # the store travels beside AidProcessorArgs: that struct is the one of the previous header
    assert [f for f, _ in _lib.AidProcessorArgs._fields_][-1] == "lora_gain_o" and C.sizeof(_lib.AidProcessorArgs) == 440
    assert C.sizeof(_lib.AidEndpointRows) == 80 and C.sizeof(_lib.AidEndpointStore) == 32


def _rows(**kw):
    a = _lib.AidEndpointRows()
    a.k, a.vt, a.k_store, a.vt_store, a.step = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    a.k_fs, a.vt_fs, a.row_begin, a.row_end, a.n_steps, a.direction, a.dtype = 33 * 40, 40 * 40, 0, 4, 3, _lib.EP_PUT, _lib.DTYPE_F16
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("field,value,code", [
    ("k", None, -1), ("vt", None, -1), ("k_store", None, -1), ("vt_store", None, -1), ("step", None, -1),
    ("step", 0x5002, -1), ("row_begin", -1, -1), ("row_end", -1, -1), ("n_steps", 0, -1), ("direction", 2, -1), ("direction", -1, -1),
    ("dtype", 3, -2), ("dtype", -1, -2),
    ("k_fs", 33 * 40 + 4, -3), ("vt_fs", 40 * 40 + 4, -3), ("k_fs", 0, -3), ("vt_fs", -8, -3),
    ("k", 0x1008, -3), ("vt", 0x2004, -3), ("k_store", 0x3002, -3), ("vt_store", 0x4008, -3)])
def test_endpoint_rows_argument_errors_return_their_codes_before_any_launch(field, value, code):
    lib = _lib.load()
    assert lib.aid_endpoint_rows(None, None) == -1
    assert lib.aid_endpoint_rows(C.byref(_rows(**{field: value})), None) == code


def _proc_args(mode=_lib.MODE_OUTER, n=3):
    a = _lib.AidProcessorArgs()
    for f in ("x", "wq", "wk", "wv", "wo", "y", "coef"):
        setattr(a, f, 0x1000)
    a.n_frames, a.s, a.l, a.c, a.cc, a.heads, a.mode, a.dtype, a.n_ctx = n, 40, 40, 320, 320, 8, mode, _lib.DTYPE_F16, n
    a.begin, a.end = 0, n - 1
    return a


def _store(mode=_lib.EP_RECORD, **kw):
    e = _lib.AidEndpointStore()
    e.k_store, e.vt_store, e.step, e.n_steps, e.mode = 0x3000, 0x4000, 0x5000, 3, mode
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def test_processor_ep_checks_everything_before_its_first_launch():
    """With a NULL workspace a well-formed call gets as far as AID_ERR_WORKSPACE (-4) without a GPU; a malformed one is refused before."""
    lib = _lib.load()
    a = _proc_args()
    fwd = lambda a_, e_: lib.aid_processor_ep_fwd(C.byref(a_), None if e_ is None else C.byref(e_), None)      # noqa: E731
    size = lambda a_, e_: lib.aid_processor_ep_workspace_bytes(C.byref(a_), None if e_ is None else C.byref(e_))   # noqa: E731
    base = lib.aid_processor_workspace_bytes(C.byref(a))
    assert base > 0
    assert lib.aid_processor_ep_fwd(None, C.byref(_store()), None) == -1 and lib.aid_processor_ep_workspace_bytes(None, None) == 0
    # ep == NULL is aid_processor_fwd: its checks, its workspace
    assert fwd(a, None) == lib.aid_processor_fwd(C.byref(a), None) == -4 and size(a, None) == base
    bad = _proc_args()
    bad.wq = None
    assert fwd(bad, None) == lib.aid_processor_fwd(C.byref(bad), None) == -1
    # RECORD: the plain call's workspace; REPLAY: two more rows of k and V^T (256-byte aligned regions)
    assert fwd(a, _store()) == -4 and size(a, _store()) == base
    es, s, c, lp, al = 2, 40, 320, 40, lambda x: (x + 255) // 256 * 256
    assert fwd(a, _store(_lib.EP_REPLAY)) == -4
    assert size(a, _store(_lib.EP_REPLAY)) == base - al(3 * s * c * es) - al(3 * c * lp * es) + al(5 * s * c * es) + al(5 * c * lp * es)
    # REPLAY does not read begin / end; RECORD does
    a.begin = a.end = 99
    assert fwd(a, _store(_lib.EP_REPLAY)) == -4 and fwd(a, _store()) == -1 and size(a, _store()) == 0
    a = _proc_args()
    for e in (_store(0), _store(3), _store(k_store=None), _store(vt_store=None), _store(step=None), _store(step=0x5001),
              _store(n_steps=0)):
        assert fwd(a, e) == -1 and size(a, e) == 0
    for e in (_store(k_store=0x3008), _store(vt_store=0x4004)):
        assert fwd(a, e) == -3
    for mode in (_lib.EP_RECORD, _lib.EP_REPLAY):
        p = _proc_args(_lib.MODE_PLAIN)                                   # a plain call has no end points
        assert fwd(p, _store(mode)) == -1
        x = _proc_args()                                                  # cross-attention needs no store
        x.ctx, x.l, x.cc = 0x1000, 77, 64
        assert lib.aid_processor_fwd(C.byref(x), None) == -4 and fwd(x, _store(mode)) == -1
        x.ip, x.wk_ip, x.wv_ip, x.n_ip, x.t_ip, x.ip_mode, x.ip_stride = 0x1000, 0x1000, 0x1000, 3, 4, 2, 4 * 64     # nor the image branch
        assert fwd(x, _store(mode)) == -1
        f = _proc_args()
        f.dtype = 7
        assert fwd(f, _store(mode)) == -2
        f = _proc_args()
        f.c, f.heads = 384, 3                                             # head dim 128
        assert fwd(f, _store(mode)) == -3
    # what aid_processor_fwd accepts beside it is accepted: a mask (pure mode), LoRA ranks
    a = _proc_args()
    a.attn_bias, a.lora_r_q, a.lora_up_q, a.lora_down_x = 0x1000, 64, 0x1000, 0x1000
    assert fwd(a, _store()) == -4 and fwd(a, _store(_lib.EP_REPLAY)) == -4


# ---- EndpointStore bookkeeping ------------------------------------------------------------------------------------------------------
DT = torch.float16
SIG = {f: f"v-{f}" for f in SIGNATURE_FIELDS}


def test_slot_sizes_per_layer_and_nbytes():
    st = EndpointStore()
    assert st.nbytes == 0 and not st.recorded and st.mode is None
    st.begin_record(SIG, 3, torch.device("cpu"))
    k0, v0 = st.slot("down.attn1", 33, 40, DT, "cpu")                # ragged: round_up(33, 8) = 40 value columns
    assert tuple(k0.shape) == (3, 2, 33 * 40) and tuple(v0.shape) == (3, 2, 40 * 40) and k0.dtype == DT
    assert st.nbytes == EndpointStore.layer_bytes(3, 33, 40, DT) == 3 * 2 * (33 * 40 + 40 * 40) * 2
    k1, v1 = st.slot("mid.attn1", 16, 1280, torch.float32, "cpu")
    assert tuple(k1.shape) == (3, 2, 16 * 1280) and tuple(v1.shape) == (3, 2, 1280 * 16)
    assert st.nbytes == 3 * 2 * (33 * 40 + 40 * 40) * 2 + 3 * 2 * 2 * 16 * 1280 * 4
    assert st.slot("down.attn1", 33, 40, DT, "cpu")[0] is k0            # a layer's buffers are allocated once
    with pytest.raises(ValueError, match="another resolution"):
        st.slot("down.attn1", 40, 40, DT, "cpu")
    # the device step index: one int32, rewritten in place
    step = st.step_tensor
    assert step.dtype == torch.int32 and step.numel() == 1
    st.set_step(2)
    assert st.step_tensor is step and int(step) == 2 and st.step == 2
    with pytest.raises(IndexError):
        st.set_step(3)
    st.finish_record(torch.zeros(2, 4, 8, 8, dtype=DT))
    assert st.recorded and st.mode is None and st.nbytes == 3 * 2 * (33 * 40 + 40 * 40) * 2 + 3 * 2 * 2 * 16 * 1280 * 4 + 2 * 4 * 64 * 2
    with pytest.raises(RuntimeError, match="clear"):
        st.begin_record(SIG, 3, torch.device("cpu"))
    st.begin_replay(SIG, torch.device("cpu"))
    assert st.ep_args("mid.attn1", 16, 1280, torch.float32, "cpu")["mode"] == "replay"
    with pytest.raises(RuntimeError, match="holds no rows of layer"):
        st.slot("up.attn1", 16, 1280, torch.float32, "cpu")
    st.abort()
    assert st.recorded and st.mode is None                               # a replay leaves the store as it was
    st.clear()
    assert st.nbytes == 0 and not st.recorded and st.layers == {}


def test_max_bytes_refuses_before_allocation_and_names_the_bytes(monkeypatch):
    one = EndpointStore.layer_bytes(3, 33, 40, DT)
    st = EndpointStore(max_bytes=2 * one - 1)
    st.begin_record(SIG, 3, torch.device("cpu"))
    st.slot("a", 33, 40, DT, "cpu")
    made = []
    real = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: made.append(a) or real(*a, **k))
    with pytest.raises(ValueError, match=rf"needs {2 * one} bytes, max_bytes is {2 * one - 1}"):
        st.slot("b", 33, 40, DT, "cpu")
    assert made == []                                                    # refused before the buffer was allocated ...
    assert st.nbytes == 0 and st.layers == {} and not st.recorded        # ... and the refused record leaves nothing behind
    st = EndpointStore(max_bytes=one)                                    # the final latents count too
    st.begin_record(SIG, 3, torch.device("cpu"))
    st.slot("a", 33, 40, DT, "cpu")
    with pytest.raises(ValueError, match=f"needs {one + 1024} bytes"):
        st.finish_record(torch.zeros(2, 4, 8, 8, dtype=DT))
    with pytest.raises(ValueError):
        EndpointStore(max_bytes=-1)


@pytest.mark.parametrize("field", SIGNATURE_FIELDS)
def test_each_signature_field_mismatch_names_that_field(field):
    st = EndpointStore()
    st.begin_record(SIG, 1, torch.device("cpu"))
    st.finish_record(torch.zeros(2, 4))
    other = dict(SIG)
    other[field] = "something else"
    later = SIGNATURE_FIELDS[SIGNATURE_FIELDS.index(field) + 1:]
    if later:
        other[later[-1]] = "also different"                              # the FIRST differing field is the one named
    with pytest.raises(ValueError, match=rf"recorded under a different {field}:"):
        st.begin_replay(other, torch.device("cpu"))
    assert st.mode is None
    st.begin_replay(dict(SIG), torch.device("cpu"))                      # the matching signature replays


def test_run_signature_digests_contents_not_addresses():
    g = torch.Generator().manual_seed(0)
    lat, emb = torch.randn(1, 4, 8, 8, generator=g), torch.randn(1, 7, 32, generator=g)
    unet = aid_amd.AttnStackUNet("sd15", dtype=DT, scale_down=16)
    kw = dict(latent_start=lat, latent_end=lat + 1, embeds_start=emb, embeds_end=emb * 2, embeds_negative=[emb * 0, emb * 0],
              embeds_pooled=[], embeds_guide=[], num_inference_steps=6, warmup_ratio=0.5, early="outer", late="self", fusion=True,
              guidance_scale=7.5, dtype=DT, timesteps=torch.arange(6), unet=unet)
    a, b = endpoint_store.run_signature(**kw), endpoint_store.run_signature(**dict(kw, embeds_start=emb.clone()))
    assert a == b and tuple(a) == SIGNATURE_FIELDS and a["embeds_pooled"] is None
    edited = emb.clone()
    edited[0, 3, 5] += 1e-3
    c = endpoint_store.run_signature(**dict(kw, embeds_start=edited))
    assert [f for f in SIGNATURE_FIELDS if a[f] != c[f]] == ["embeds_start"]
    d = endpoint_store.run_signature(**dict(kw, unet=aid_amd.AttnStackUNet("sd15", dtype=DT, scale_down=16), timesteps=torch.arange(1, 7)))
    assert [f for f in SIGNATURE_FIELDS if a[f] != d[f]] == ["timesteps", "unet"]


# ---- the Python layer against a recording stand-in ----------------------------------------------------------------------------------
class _Recorder:
    """Stands in for libaid_hip.so: records the store the Python layer hands to aid_processor_ep_fwd."""

    def __init__(self):
        self.calls, self.plain = [], 0

    def aid_processor_workspace_bytes(self, ref):
        return 64

    def aid_processor_ep_workspace_bytes(self, ref, ep):
        return 128

    def aid_processor_fwd(self, ref, stream):
        self.plain += 1
        return 0

    def aid_processor_ep_fwd(self, ref, ep, stream):
        a, e = ref._obj, ep._obj
        self.calls.append(dict(n=a.n_frames, s=a.s, c=a.c, mode=a.mode, ctx=a.ctx, ws=a.workspace_bytes, k_store=e.k_store,
                               vt_store=e.vt_store, step=e.step, n_steps=e.n_steps, ep_mode=e.mode, n_plain=a.n_plain))
        return 0


@pytest.fixture
def rec(monkeypatch):
    lib = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(ops, "_require_gpu", lambda *ts: torch.device("cpu"))
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "workspace", lambda nbytes, dev: torch.empty(nbytes, dtype=torch.uint8))
    yield lib


def test_processor_ep_fwd_hands_the_layers_store_over(rec):
    st = EndpointStore()
    st.begin_record(SIG, 3, torch.device("cpu"))
    c, heads, s = 64, 1, 33
    w = [torch.zeros(c, c, dtype=DT) for _ in range(4)]
    x = torch.zeros(3, s, c, dtype=DT)
    coef = torch.tensor([0.0, 0.5, 1.0])
    ep = st.ep_args("l0", s, c, DT, "cpu")
    ops.processor_ep_fwd(x, *w, None, heads, ep=ep, mode="outer", fused=True, coef=coef)
    (call,) = rec.calls
    k_store, vt_store = st.layers["l0"]
    assert call["k_store"] == k_store.data_ptr() and call["vt_store"] == vt_store.data_ptr() and call["step"] == st.step_tensor.data_ptr()
    assert (call["n_steps"], call["ep_mode"], call["n"], call["ctx"], call["ws"]) == (3, _lib.EP_RECORD, 3, None, 128)
    assert rec.plain == 0                                               # ONE library call per processor call
    with pytest.raises(ValueError, match="interpolated"):
        ops.processor_ep_fwd(x, *w, None, heads, ep=ep, mode="plain")
    with pytest.raises(ValueError, match="self-attention"):
        ops.processor_ep_fwd(x, *w, None, heads, ep=ep, mode="outer", coef=coef, kv_cached=(x, x))
    with pytest.raises(ValueError, match=r"k_store \[n_steps, 2, 2048\]"):
        ops.processor_ep_fwd(x[:, :32].contiguous(), *w, None, heads, ep=ep, mode="outer", coef=coef)
    with pytest.raises(TypeError, match="store holds"):
        ops.processor_ep_fwd(x.float(), *(t.float() for t in w), None, heads, ep=ep, mode="outer", coef=coef)
    with pytest.raises(ValueError, match="'record' or 'replay'"):
        ops.processor_ep_fwd(x, *w, None, heads, ep=dict(ep, mode="put"), mode="outer", coef=coef)
    assert len(rec.calls) == 1


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _recording_store():
    st = EndpointStore()
    st.begin_record(SIG, 2, torch.device("cpu"))
    return st


def test_a_store_on_a_cpu_tensor_is_refused_with_the_reason():
    attn = aid_amd.AttnShim(64, 1, None, dtype=DT)
    proc = aid_amd.OuterInterpolatedAttnProcessor(size=3, is_fused=True)
    assert proc.endpoint_store is None and proc.endpoint_layer is None   # opt-in: absent by default
    proc.endpoint_store = _recording_store()
    with pytest.raises(NotImplementedError, match="CPU tensor"):
        proc(attn, torch.zeros(3, 16, 64, dtype=DT))
    inner = aid_amd.InnerInterpolatedAttnProcessor(size=3)
    inner.endpoint_store = _recording_store()
    with pytest.raises(NotImplementedError, match="CPU tensor"):
        inner(attn, torch.zeros(3, 16, 64, dtype=DT))


def test_a_store_together_with_the_exchange_is_refused():
    attn = aid_amd.AttnShim(64, 1, None, dtype=DT)
    proc = aid_amd.OuterInterpolatedAttnProcessor(size=3)
    proc.endpoint_store, proc.endpoint_exchange = _recording_store(), object()
    with pytest.raises(NotImplementedError, match="endpoint_exchange"):
        proc(attn, torch.zeros(3, 16, 64, dtype=DT))


def test_ip_processors_refuse_a_store(rec):
    attn = aid_amd.AttnShim(64, 1, 32, dtype=DT)
    ip_attn = aid_amd.HipIPAdapterAttnProcessor(hidden_size=64, cross_attention_dim=32, num_tokens=(4,), scale=0.5, dtype=DT)
    for cls in (aid_amd.OuterInterpolatedIPAttnProcessor, aid_amd.InnerInterpolatedIPAttnProcessor, aid_amd.ScaleControlIPAttnProcessor):
        proc = cls(t=0.5, is_fused=True, ip_attn=ip_attn)
        proc.endpoint_store = _recording_store()
        with pytest.raises(NotImplementedError, match="IP-Adapter"):
            proc(attn, torch.zeros(3, 16, 64, dtype=DT), encoder_hidden_states=(torch.zeros(3, 7, 32, dtype=DT), [torch.zeros(9, 1, 4, 32, dtype=DT)]))
    assert rec.calls == [] and rec.plain == 0


def test_set_endpoint_store_names_the_layers_and_detaches():
    unet = aid_amd.AttnStackUNet("sd15", dtype=DT, scale_down=16)
    aid_amd.load_aid(unet, t=0.5)
    st, ectx = _recording_store(), torch.zeros(2, 7, 32)
    aid_amd.loop.set_endpoint_store(unet, st, endpoint_ctx=ectx, coef=[0.3])
    for name, proc in unet.attn_processors.items():
        assert proc.endpoint_store is st and proc.endpoint_layer == name and proc.endpoint_ctx is ectx
        assert proc.coef.tolist() == pytest.approx([0.3])               # a replay processor holds the interior coefficients only
    aid_amd.loop.set_endpoint_store(unet, None)
    assert all(p.endpoint_store is None and p.endpoint_layer is None and p.endpoint_ctx is None for p in unet.attn_processors.values())


def test_pipeline_keyword_refuses_image_inputs_and_a_changed_prompt_before_any_launch():
    hip = aid_amd.StackDenoiser("sd15", dtype=DT, scale_down=16, latent_hw=(8, 8))
    pipe = aid_amd.InterpolationStableDiffusionPipeline(hip, aid_amd.DDIMSchedulerLite())
    pipe.load_aid(t=0.5)
    g = torch.Generator().manual_seed(1)
    l0, l1 = torch.randn(1, 4, 8, 8, generator=g), torch.randn(1, 4, 8, 8, generator=g)
    es, ee = (torch.randn(1, 7, 768, generator=g),) * 2, (torch.randn(1, 7, 768, generator=g),) * 2
    kw = dict(latent_start=l0, latent_end=l1, embeds_start=es, embeds_end=ee, num_inference_steps=4, output_type="latent", use_graphs=False)
    with pytest.raises(NotImplementedError, match="IP-Adapter image inputs"):
        pipe.interpolate_single(0.5, endpoints=EndpointStore(), image_embeds_end=(torch.zeros(1, 1, 8), torch.zeros(1, 1, 8)), **kw)
    # a recorded store whose signature differs raises before the run touches the processors
    st = EndpointStore()
    sig = {f: None for f in SIGNATURE_FIELDS}
    st.begin_record(sig, 2, torch.device("cpu"))
    st.finish_record(torch.zeros(2, 4, 8, 8, dtype=DT))
    with pytest.raises(ValueError, match="recorded under a different latent_start"):
        pipe.interpolate_single(0.5, endpoints=st, **kw)
    with pytest.raises(ValueError, match="recorded under a different latent_start"):
        pipe.interpolate(l0, l1, embeds_start=es, embeds_end=ee, size=5, num_inference_steps=4, output_type="latent", use_graphs=False,
                         endpoints=st)
    assert all(p.endpoint_store is None for p in hip.attn_processors.values()) and st.recorded and st.mode is None


def test_beta_prior_pipeline_takes_reuse_endpoints():
    class _Model:
        def get_image_features(self, x):
            return x.reshape(x.shape[0], -1).float()

    bp = aid_amd.BetaPriorPipeline(pipe=None, model=_Model())
    assert bp.reuse_endpoints is False and bp.endpoints is None
    seen = []

    class _Pipe:
        _aid_early = "fused_outer"

        def interpolate_single(self, t, **kw):
            seen.append(("single", kw.get("endpoints")))
            return {"images": torch.zeros(3, 1, 2, 2)}

        def interpolate(self, *a, **kw):
            seen.append(("n", kw.get("endpoints")))
            return torch.zeros(kw["size"], 1, 2, 2)

    bp = aid_amd.BetaPriorPipeline(pipe=_Pipe(), model=_Model(), reuse_endpoints=True)
    bp._render([0.5], None, None, None, None, None, 4, {})
    assert seen == [("single", None)]                                     # outside an exploration nothing is attached
    bp.endpoints = EndpointStore()
    bp._render([0.5], None, None, None, None, None, 4, {})
    bp._render([0.2, 0.7], None, None, None, None, None, 4, {})
    assert seen[1] == ("single", bp.endpoints) and seen[2] == ("n", bp.endpoints)


# ---- resources ----------------------------------------------------------------------------------------------------------------------
def test_copy_kernel_resources_no_scratch_no_spills():
    """aid_endpoint.resources.txt at this commit: 12 VGPRs, 44 SGPRs, no AGPRs, no scratch, no spills, no LDS, 8 waves per SIMD."""
    path = os.path.join(CSRC, "aid_endpoint.resources.txt")
    if not os.path.exists(path):
        pytest.skip(f"{path} not there: build the library first (python -c 'import __graft_entry__ as g; g.build()')")
    blocks = open(path).read().split("Name: ")[1:]
    assert len(blocks) == 1 and "aid_endpoint_rows_kernel" in blocks[0].split()[0]
    num = lambda key: int(re.search(re.escape(key) + r": (\d+)", blocks[0]).group(1))   # noqa: E731
    assert num("ScratchSize [bytes/lane]") == 0 and num("VGPRs Spill") == 0 and num("SGPRs Spill") == 0
    assert num("AGPRs") == 0 and num("LDS Size [bytes/block]") == 0
    assert num("VGPRs") <= 32 and num("Occupancy [waves/SIMD]") == 8
