"""N-frame ``interpolate`` with IP-Adapter image prompts: the host side, without a GPU.

A recording double of the library stands in for ``libaid_hip.so`` (every entry point returns AID_OK, ``aid_processor_fwd`` keeps what it was
handed); with CPU tensors the "device" buffers — coefficients, ``ip_map``, ``ip_frame_scale``, ``ctx_map``, the image rows — are host
memory and are read back through their addresses.  What is checked: the image branch of every cross-attention call of a run (rows,
map, mode, riders), that self-attention is a text run's, the rider layout of the three IP processors, the refusals, the two-pass
fallback, and that a run without image keywords issues the calls it always issued."""
import ctypes as C

import pytest
import torch

import aid_amd
from aid_amd import _lib, ops, processors
from aid_amd.loop import install_sequence_processors
from aid_amd.pipelines import DDIMSchedulerLite, InterpolationStableDiffusionPipeline, StackDenoiser

DT = torch.float16
IP_SAME, IP_PLAIN = 1, 2
MODE_PLAIN, MODE_INNER, MODE_OUTER = _lib.MODE_PLAIN, _lib.MODE_INNER, _lib.MODE_OUTER


def _read(ptr, n, ctype):
    return None if not ptr else list((ctype * n).from_address(ptr))


def _image_rows(a):
    """The image rows a call is handed, [n_ip, t_ip, cc], copied while the call is in flight (the run frees them afterwards)."""
    out = []
    for r in range(a.n_ip):
        buf = (C.c_uint16 * (a.t_ip * a.cc)).from_address(a.ip + 2 * r * a.ip_stride)
        out.append(torch.frombuffer(buf, dtype=torch.float16).reshape(a.t_ip, a.cc).clone())
    return torch.stack(out)


class _Recorder:
    """Every symbol of the library: returns 0 (AID_OK); the processor entry points record their arguments."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name.startswith("aid_"):
            return (lambda *a, **k: 64) if name.endswith("workspace_bytes") else (lambda *a, **k: 0)
        raise AttributeError(name)

    def aid_abi_version(self):
        return _lib.AID_ABI_VERSION

    def aid_processor_ip_fwd(self, ref, segs, n, stream):
        self.calls.append(dict(self._args(ref._obj), n_segs=n))
        return 0

    def aid_processor_fwd(self, ref, stream):
        self.calls.append(dict(self._args(ref._obj), n_segs=0))
        return 0

    @staticmethod
    def _args(a):
        n = a.n_frames
        d = dict(n=n, cross=bool(a.ctx), mode=a.mode, fused=a.fused, n_plain=a.n_plain, begin=a.begin, end=a.end, n_ctx=a.n_ctx,
                 coef=_read(a.coef, n, C.c_float), ctx_map=_read(a.ctx_map, n, C.c_int32), ip=a.ip, x=a.x, ctx=a.ctx,
                 seg=a.seg_executed, k_cached=a.k_cached)
        if a.ip:
            d.update(n_ip=a.n_ip, t_ip=a.t_ip, ip_mode=a.ip_mode, ip_scale=a.ip_scale, ip_begin=a.ip_begin, ip_end=a.ip_end,
                     ip_stride=a.ip_stride, ip_map=_read(a.ip_map, n, C.c_int32), ip_frame_scale=_read(a.ip_frame_scale, n, C.c_float),
                     wk_ip=a.wk_ip, rows=_image_rows(a))
        return d


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


# ---- a pipeline over the stand-in stack ------------------------------------------------------------------------------------------------
SIZE, T_IP, STEPS = 5, 4, 4


def _pipe(adapter=True, adapters=1):
    den = StackDenoiser("sd15", dtype=DT, scale_down=64, latent_hw=(8, 8), sublayers="steps")
    if adapter:
        den.stack.load_ip_adapter(num_tokens=T_IP, scale=0.5)
        if adapters == 2:                      # a second adapter on every IP layer (diffusers: one processor holding both)
            for m in den.stack.layers:
                p = m.processor
                if hasattr(p, "to_k_ip"):
                    p.to_k_ip.append(torch.nn.Linear(den.stack.cross_dim, p.to_k_ip[0].weight.shape[0], bias=False, dtype=DT))
                    p.to_v_ip.append(torch.nn.Linear(den.stack.cross_dim, p.to_v_ip[0].weight.shape[0], bias=False, dtype=DT))
                    p.scale.append(0.25)
                    p.num_tokens = p.num_tokens + (T_IP,)
    return InterpolationStableDiffusionPipeline(den, DDIMSchedulerLite()), den


def _inputs(den, seed=0):
    g = torch.Generator().manual_seed(seed)
    cc, l = den.stack.cross_dim, den.stack.text_len
    r = lambda *s: torch.randn(*s, generator=g).to(DT)      # noqa: E731
    kw = dict(latent_start=r(1, 4, 8, 8), latent_end=r(1, 4, 8, 8), embeds_start=(r(1, l, cc), r(1, l, cc)),
              embeds_end=(r(1, l, cc), r(1, l, cc)), size=SIZE, num_inference_steps=STEPS, warmup_ratio=0.5, output_type="latent")
    img = dict(image_embeds_start=(r(1, T_IP, cc), r(1, T_IP, cc)), image_embeds_end=(r(1, T_IP, cc), r(1, T_IP, cc)))
    return kw, img


def _n_layers(den):
    return sum(1 for s in den.stack.shapes if s[3]), sum(1 for s in den.stack.shapes if not s[3])


@pytest.mark.parametrize("early", ["fused_outer", "pure_outer", "fused_inner"])
def test_every_cross_attention_call_of_an_image_run_carries_the_image_branch(rec, early):
    """(fails on the parent commit with TypeError: interpolate() got an unexpected keyword argument 'image_embeds_start')"""
    pipe, den = _pipe()
    kw, img = _inputs(den)
    installed = dict(den.attn_processors)
    pipe.interpolate(early=early, **kw, **img)
    assert dict(den.attn_processors) == installed                       # restored
    n_cross, n_self = _n_layers(den)
    assert len(rec.calls) == STEPS * (n_cross + n_self)                 # batched CFG: ONE UNet call per step
    coef = aid_amd.generate_beta_tensor(SIZE, alpha=STEPS, beta=STEPS)
    coef[0], coef[-1] = 0, 1
    want_coef = coef.to(DT).float().tolist() + [-1.0] * SIZE
    pos_s, pos_e, neg_s, neg_e = img["image_embeds_start"][1], img["image_embeds_end"][1], img["image_embeds_start"][0], img["image_embeds_end"][0]
    ts = coef.tolist()
    want_rows = torch.cat([pos_s] + [torch.lerp(pos_s, pos_e, t) for t in ts[1:-1]] + [pos_e]
                          + [neg_s] + [torch.lerp(neg_s, neg_e, t) for t in ts[1:-1]] + [neg_e])
    mode = MODE_OUTER if early.endswith("outer") else MODE_INNER
    per_step = n_cross + n_self
    for step in range(STEPS):
        calls = rec.calls[step * per_step:(step + 1) * per_step]
        aid = step < STEPS // 2
        for c in calls:
            assert c["n"] == 2 * SIZE
            if not c["cross"]:
                assert c["ip"] is None
                continue
            assert c["ip"] is not None and c["t_ip"] == T_IP and c["n_ip"] == 2 * SIZE and c["ip_map"] is None
            assert c["ip_frame_scale"] is None and c["ip_scale"] == 0.5
            assert torch.equal(c["rows"], want_rows)                  # frame k: mix(start, end, t_k); [cond frames ; uncond frames]
            if aid:
                assert (c["mode"], c["fused"], c["n_plain"]) == (mode, int(early.startswith("fused")), SIZE)
                assert c["coef"] == want_coef and (c["begin"], c["end"]) == (0, SIZE - 1)
                if mode == MODE_OUTER:
                    assert (c["ip_mode"], c["ip_begin"], c["ip_end"]) == (IP_SAME, 0, SIZE - 1)
                else:
                    assert c["ip_mode"] == IP_PLAIN
            else:                                                        # de-activated: the adapter's own plain call over 2 N frames
                assert (c["mode"], c["n_plain"], c["ip_mode"]) == (MODE_PLAIN, 0, IP_PLAIN)


def _self_calls(rec):
    keys = ("n", "mode", "fused", "n_plain", "begin", "end", "coef", "ctx_map", "seg")
    return [tuple(c[k] for k in keys) for c in rec.calls if not c["cross"]]


def test_self_attention_calls_are_those_of_a_text_run(rec):
    pipe, den = _pipe()
    kw, img = _inputs(den)
    pipe.interpolate(**kw, **img)
    with_images = _self_calls(rec)
    rec.calls.clear()
    pipe.interpolate(**kw)
    assert with_images == _self_calls(rec) and len(with_images) == STEPS * _n_layers(den)[1]


def test_a_run_without_image_keywords_issues_the_calls_it_always_issued(rec):
    """The recorded sequence of a text run over a stack WITHOUT an adapter, written down from the code as it stood before the image
    keywords: per step one call per layer over [cond ; uncond], AID steps OUTER fused with N riders, the others plain; no image
    branch anywhere, graph-less on the CPU."""
    pipe, den = _pipe(adapter=False)
    kw, _ = _inputs(den)
    for p in den.stack.layers:
        p.processor = aid_amd.HipAttnProcessor()
    pipe.interpolate(**kw)
    n_cross, n_self = _n_layers(den)
    assert len(rec.calls) == STEPS * (n_cross + n_self)
    coef = aid_amd.generate_beta_tensor(SIZE, alpha=STEPS, beta=STEPS)
    coef[0], coef[-1] = 0, 1
    want_coef = coef.to(DT).float().tolist() + [-1.0] * SIZE
    for i, c in enumerate(rec.calls):
        aid = i < (STEPS // 2) * (n_cross + n_self)
        assert c["ip"] is None and c["n_segs"] == 0 and c["n"] == 2 * SIZE and c["ctx_map"] is None
        if aid:
            assert (c["mode"], c["fused"], c["n_plain"], c["begin"], c["end"], c["coef"]) == (MODE_OUTER, 1, SIZE, 0, SIZE - 1, want_coef)
        else:
            assert (c["mode"], c["fused"], c["n_plain"]) == (MODE_PLAIN, 0, 0)
        assert (c["k_cached"] is not None) == c["cross"]                 # text keys / values projected once per run


def test_a_text_run_over_an_adapter_stack_installs_text_processors_and_restores(rec):
    """No image keywords over a stack WITH an adapter: the text processors everywhere, and the installed processors — plain objects
    on the self-attention layers, modules on the adapter layers — are put back (the shim refused to, before this change)."""
    pipe2, den2 = _pipe()
    n_cross, n_self = _n_layers(den2)
    installed = dict(den2.attn_processors)
    pipe2.interpolate(**_inputs(den2)[0])
    assert [(c["ip"], c["mode"], c["n_plain"]) for c in rec.calls] == \
        [(None, MODE_OUTER if i < (STEPS // 2) * (n_cross + n_self) else MODE_PLAIN, SIZE if i < (STEPS // 2) * (n_cross + n_self) else 0)
         for i in range(len(rec.calls))]
    assert dict(den2.attn_processors) == installed


def test_scale_control_run_maps_frames_to_the_end_image_and_scales_by_coefficient(rec):
    pipe, den = _pipe()
    kw, img = _inputs(den)
    neg_e, pos_e = img["image_embeds_end"]
    pipe.interpolate(**kw, image_embeds_end=img["image_embeds_end"])
    coef = aid_amd.generate_beta_tensor(SIZE, alpha=STEPS, beta=STEPS)
    coef[0], coef[-1] = 0, 1
    cv = coef.to(DT).float().tolist()
    cross = [c for c in rec.calls if c["cross"]]
    assert len(cross) == STEPS * _n_layers(den)[0]
    for i, c in enumerate(cross):
        aid = i < (STEPS // 2) * _n_layers(den)[0]
        assert (c["mode"], c["n_plain"]) == ((MODE_OUTER, SIZE) if aid else (MODE_PLAIN, 0))
        assert c["ip_mode"] == IP_PLAIN and c["ip_scale"] == 1.0 and c["n_ip"] == 2 * SIZE
        assert c["ip_map"] == [SIZE - 1] * SIZE + [2 * SIZE - 1] * SIZE
        assert c["ip_frame_scale"] == cv + cv
        rows = c["rows"]
        assert torch.equal(rows[SIZE - 1], pos_e[0]) and torch.equal(rows[2 * SIZE - 1], neg_e[0])
        if aid:
            assert c["coef"] == cv + [-1.0] * SIZE
    with pytest.raises(ValueError, match="outer"):
        pipe.interpolate(early="fused_inner", **kw, image_embeds_end=img["image_embeds_end"])


# ---- the processors ---------------------------------------------------------------------------------------------------------------------
N, S, CW, HEADS, CC, L = 3, 40, 80, 2, 64, 7


def _layer(cls, fused=True, scale=0.5, ip_attn=None):
    attn = aid_amd.AttnShim(CW, HEADS, CC, dtype=DT)
    ipa = ip_attn or aid_amd.HipIPAdapterAttnProcessor(hidden_size=CW, cross_attention_dim=CC, num_tokens=(T_IP,), scale=scale, dtype=DT)
    proc = cls(size=N, is_fused=fused, ip_attn=ipa)
    return attn, proc


@pytest.mark.parametrize("cls", [aid_amd.OuterInterpolatedIPAttnProcessor, aid_amd.InnerInterpolatedIPAttnProcessor,
                                 aid_amd.ScaleControlIPAttnProcessor])
def test_plain_tail_riders_are_accepted(rec, cls):
    """(fails on the parent commit with the ``_frames`` RuntimeError: "got a batch of 6")"""
    attn, proc = _layer(cls)
    proc.plain_tail = N
    x, text, ip = torch.zeros(2 * N, S, CW, dtype=DT), torch.zeros(2 * N, L, CC, dtype=DT), torch.zeros(2 * N, T_IP, CC, dtype=DT)
    y = proc(attn, x, encoder_hidden_states=(text, [ip]))
    assert y.shape == x.shape
    (c,) = rec.calls
    cv = proc.coef.to(DT).float().tolist()
    assert c["n"] == 2 * N and c["n_plain"] == N and c["coef"] == cv + [-1.0] * N and c["n_ip"] == 2 * N
    assert c["seg"] == ops.executed_segments("inner" if cls is aid_amd.InnerInterpolatedIPAttnProcessor else "outer", True,
                                             cv + [-1.0] * N, 2 * N, None, 0, N - 1)
    if cls is aid_amd.ScaleControlIPAttnProcessor:
        assert c["ip_map"] == [N - 1] * N + [2 * N - 1] * N and c["ip_frame_scale"] == cv + cv and c["ip_mode"] == IP_PLAIN
        # the scales follow a new schedule in place (a captured graph holds the buffer's address)
        proc.coef = torch.tensor([0.0, 0.25, 1.0])
        proc(attn, x, encoder_hidden_states=(text, [ip]))
        assert rec.calls[-1]["ip_frame_scale"] == [0.0, 0.25, 1.0] * 2 and rec.calls[-1]["coef"] == [0.0, 0.25, 1.0, -1.0, -1.0, -1.0]
        # de-activated: plain text attention, the same image branch
        proc.deactivate()
        proc(attn, x, encoder_hidden_states=(text, [ip]))
        assert (rec.calls[-1]["mode"], rec.calls[-1]["n_plain"], rec.calls[-1]["ip_map"]) == (MODE_PLAIN, 0, [N - 1] * N + [2 * N - 1] * N)
    else:
        assert c["ip_map"] is None and c["ip_frame_scale"] is None
        assert (c["ip_mode"], c["ip_begin"], c["ip_end"]) == ((IP_SAME, 0, N - 1) if cls is aid_amd.OuterInterpolatedIPAttnProcessor
                                                            else (IP_PLAIN, 0, 2 * N - 1))
    # a batch that is neither N nor N + riders is refused as before
    with pytest.raises(RuntimeError, match="got a batch of 4"):
        proc(attn, x[:4], encoder_hidden_states=(text[:4], [ip[:4]]))


def test_batch_three_without_riders_is_the_call_it_was(rec):
    attn, proc = _layer(aid_amd.ScaleControlIPAttnProcessor)
    x, text, ip = torch.zeros(N, S, CW, dtype=DT), torch.zeros(N, L, CC, dtype=DT), torch.zeros(3 * N, 1, T_IP, CC, dtype=DT)
    proc(attn, x, encoder_hidden_states=(text, [ip]))
    (c,) = rec.calls
    cv = proc.coef.to(DT).float().tolist()
    assert (c["n_ip"], c["ip_map"], c["ip_frame_scale"], c["coef"], c["n_plain"], c["ctx_map"]) == (N, None, cv, cv, 0, None)


def test_ctx_index_shares_text_contexts_beside_the_image_branch(rec):
    attn, proc = _layer(aid_amd.OuterInterpolatedIPAttnProcessor)
    proc.plain_tail = N
    x, ip = torch.zeros(2 * N, S, CW, dtype=DT), torch.zeros(2 * N, T_IP, CC, dtype=DT)
    text = torch.zeros(4, L, CC, dtype=DT)
    proc(attn, x, encoder_hidden_states=(text, [ip]), ctx_index=[0, 1, 1, 2, 3, 3])
    c = rec.calls[-1]
    assert (c["n_ctx"], c["ctx_map"], c["begin"], c["end"]) == (4, [0, 1, 1, 2, 3, 3], 0, 1)
    proc.ctx_index = [0, 0, 1, 2, 2, 3]                      # the attribute, as the text processors take it; set_ctx_index reaches it
    proc(attn, x, encoder_hidden_states=(torch.zeros(2 * N, L, CC, dtype=DT), [ip]))
    c = rec.calls[-1]
    assert (c["n_ctx"], c["ctx_map"], c["begin"], c["end"]) == (4, [0, 0, 1, 2, 2, 3], 0, 1)
    # de-activated, the wrapped adapter processor gets one context per frame
    proc.deactivate()
    proc.ctx_index = None
    proc(attn, x, encoder_hidden_states=(text, [ip]), ctx_index=[0, 1, 1, 2, 3, 3])
    assert (rec.calls[-1]["n_ctx"], rec.calls[-1]["mode"], rec.calls[-1]["ctx_map"]) == (2 * N, MODE_PLAIN, None)


class _Foreign:
    """A processor of somebody else's that holds an adapter (what keep_original=True keeps)."""

    def __init__(self, like):
        self.to_k_ip, self.to_v_ip, self.scale, self.num_tokens = like.to_k_ip, like.to_v_ip, like.scale, like.num_tokens
        self.calls = 0

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None, **kw):
        self.calls += 1
        return torch.zeros_like(hidden_states)


def test_riders_are_refused_where_they_cannot_stand_for_the_deactivated_pass(rec):
    x, text, ip = torch.zeros(2 * N, S, CW, dtype=DT), torch.zeros(2 * N, L, CC, dtype=DT), torch.zeros(2 * N, T_IP, CC, dtype=DT)
    attn, proc = _layer(aid_amd.OuterInterpolatedIPAttnProcessor)
    proc.plain_tail = N
    assert proc.riders_supported() and not proc.riders_supported(ip_adapter_masks=[torch.ones(1, 1, 8, 8)])
    with pytest.raises(RuntimeError, match="two calls"):
        proc(attn, x, encoder_hidden_states=(text, [ip]), ip_adapter_masks=[torch.ones(1, 1, 8, 8)])
    with pytest.raises(RuntimeError, match="two calls"):
        proc(attn, x, encoder_hidden_states=(text, [ip]), attention_mask=torch.zeros(2 * N, 1, L, dtype=DT))
    two = aid_amd.HipIPAdapterAttnProcessor(hidden_size=CW, cross_attention_dim=CC, num_tokens=(T_IP, T_IP), scale=[0.5, 0.25], dtype=DT)
    attn, proc = _layer(aid_amd.InnerInterpolatedIPAttnProcessor, ip_attn=two)
    proc.plain_tail = N
    assert not proc.riders_supported()
    with pytest.raises(RuntimeError, match="two calls"):
        proc(attn, x, encoder_hidden_states=(text, [ip, ip]))
    attn, proc = _layer(aid_amd.ScaleControlIPAttnProcessor, ip_attn=_Foreign(two))
    assert not proc.riders_supported()
    assert rec.calls == []
    # ScaleControl's riders are the frames' unconditional twins: one each
    attn, proc = _layer(aid_amd.ScaleControlIPAttnProcessor)
    proc.plain_tail = 1
    with pytest.raises(RuntimeError, match="one each"):
        proc(attn, x[:4], encoder_hidden_states=(text[:4], [ip[:4]]))


# ---- refusals and the fallback of the pipeline ------------------------------------------------------------------------------------------
def test_interpolate_refuses_what_interpolate_single_refuses(rec):
    pipe, den = _pipe()
    kw, img = _inputs(den)
    installed = dict(den.attn_processors)
    with pytest.raises(ValueError, match="Please provide both `image_start` and `image_end` to interpolate, or only `image_end` to control the scale."):
        pipe.interpolate(**kw, image_start=object())
    with pytest.raises(ValueError, match="Please provide both"):
        pipe.interpolate(**kw, image_embeds_start=img["image_embeds_start"])
    with pytest.raises(ValueError, match="image inputs need an `encode_image` component; pass image_embeds_start / image_embeds_end"):
        pipe.interpolate(**kw, image_start=object(), image_end=object())
    with pytest.raises(RuntimeError, match=r"needs is_fused=True when image embeddings are passed.*interpolation.py:525"):
        pipe.interpolate(early="pure_inner", **kw, **img)
    with pytest.raises(NotImplementedError, match="IP-Adapter image inputs"):
        pipe.interpolate(**kw, **img, endpoints=aid_amd.EndpointStore())
    assert dict(den.attn_processors) == installed and rec.calls == []
    bare, den2 = _pipe(adapter=False)
    for p in den2.stack.layers:
        p.processor = aid_amd.HipAttnProcessor()
    before = dict(den2.attn_processors)
    with pytest.raises(ValueError, match="loaded IP-Adapter"):
        bare.interpolate(**_inputs(den2)[0], **img)
    assert dict(den2.attn_processors) == before


def test_encode_image_component_serves_pil_inputs(rec):
    pipe, den = _pipe()
    kw, img = _inputs(den)
    table = {"a": img["image_embeds_start"], "b": img["image_embeds_end"]}
    pipe._encode_image = table.__getitem__
    pipe.interpolate(**kw, image_start="a", image_end="b")
    got = [(c["ip"] is not None, c.get("n_ip")) for c in rec.calls if c["cross"]]
    assert got and all(g == (True, 2 * SIZE) for g in got)


def test_two_adapters_run_the_two_passes_separately(rec):
    """Riders cannot stand for the de-activated pass of two adapters (it runs both, the activated branch reads adapter 0):
    ``batched_cfg=True`` runs what ``batched_cfg=False`` runs, call for call."""
    pipe, den = _pipe(adapters=2)
    kw, img = _inputs(den)
    img2 = {k: tuple([t, t.flip(1)] for t in v) for k, v in img.items()}          # (negative, positive), a tensor per adapter each
    keys = ("n", "cross", "mode", "fused", "n_plain", "coef", "n_segs", "n_ip", "ip_mode", "ip_map")

    def run(batched):
        rec.calls.clear()
        pipe.interpolate(batched_cfg=batched, **kw, **img2)
        return [tuple(c.get(k) for k in keys) for c in rec.calls]
    with_flag, without = run(True), run(False)
    assert with_flag == without
    n_cross, n_self = _n_layers(den)
    assert len(with_flag) == 2 * STEPS * (n_cross + n_self) and all(c[0] == SIZE and c[4] == 0 for c in with_flag)
    cross = [c for c in rec.calls if c["cross"]]
    aid = [c for c in cross if c["mode"] == MODE_OUTER]
    plain = [c for c in cross if c["mode"] == MODE_PLAIN]
    assert len(aid) == (STEPS // 2) * n_cross and all(c["ip"] is not None and c["n_segs"] == 0 for c in aid)      # adapter 0, activated
    assert len(plain) == (2 * STEPS - STEPS // 2) * n_cross and all(c["ip"] is None and c["n_segs"] == 2 for c in plain)


def test_a_kept_foreign_processor_runs_the_two_passes_separately(rec):
    pipe, den = _pipe()
    kw, img = _inputs(den)
    foreign = []
    for m in den.stack.layers:
        if hasattr(m.processor, "to_k_ip"):
            m.processor = _Foreign(m.processor)
            foreign.append(m.processor)
    aid_amd.load_aid_ip_adapter(den, size=3, keep_original=True)
    pipe.interpolate(**kw, **img)
    # cond AID passes: the library; every de-activated pass of an adapter layer: the foreign processor, N frames at a time
    assert all(f.calls == 2 * STEPS - STEPS // 2 for f in foreign)
    assert all(c["n"] == SIZE and c["n_plain"] == 0 for c in rec.calls)


def test_install_sequence_processors_takes_the_variant_directly(rec):
    _, den = _pipe()
    held = {n: p for n, p in den.attn_processors.items() if hasattr(p, "to_k_ip")}
    install_sequence_processors(den, 5, early="pure_outer", ip_adapter="interpolate")
    procs = den.attn_processors
    for n, p in procs.items():
        if n in held:
            assert type(p) is aid_amd.OuterInterpolatedIPAttnProcessor and p.ip_attn is held[n] and not p.is_fused and p.coef.numel() == 5
            assert p.scale is held[n].scale                              # the SAME list: set_ip_adapter_scale keeps working
        else:
            assert type(p) is aid_amd.OuterInterpolatedAttnProcessor and isinstance(p.original_attn, aid_amd.HipAttnProcessor)
    install_sequence_processors(den, 5, early="fused_inner", ip_adapter="interpolate")      # found again through ip_attn
    assert all(type(p) is aid_amd.InnerInterpolatedIPAttnProcessor and p.ip_attn is held[n] for n, p in den.attn_processors.items() if n in held)
    install_sequence_processors(den, 5, early="fused_outer", ip_adapter="scale_control")
    assert all(type(p) is aid_amd.ScaleControlIPAttnProcessor for n, p in den.attn_processors.items() if n in held)
    install_sequence_processors(den, 5)                                                      # the default: text processors everywhere
    assert all(type(p) is aid_amd.OuterInterpolatedAttnProcessor for p in den.attn_processors.values())
    with pytest.raises(ValueError, match="ip_adapter must be"):
        install_sequence_processors(den, 5, ip_adapter="yes")
    with pytest.raises(ValueError, match="loaded IP-Adapter"):
        install_sequence_processors(den, 5, ip_adapter="interpolate")


def test_beta_prior_batches_carry_the_image_prompt(rec):
    """BetaPriorPipeline._render with several points per render is one ``interpolate`` run: the image keywords reach it."""
    from aid_amd.prior import BetaPriorPipeline
    pipe, den = _pipe()
    kw, img = _inputs(den)
    prior = BetaPriorPipeline(pipe, model=object())
    prior._get_feature = lambda f: f
    frames, _ = prior._render([0.25, 0.5, 0.75], None, None, "", kw["latent_start"], kw["latent_end"], STEPS,
                              dict(embeds_start=kw["embeds_start"], embeds_end=kw["embeds_end"], output_type="latent", **img))
    assert len(frames) == 5
    aid = [c for c in rec.calls if c["cross"] and c["mode"] == MODE_OUTER]
    assert aid and all(c["ip"] is not None and c["n_ip"] == 10 and c["coef"] == [0.0, 0.25, 0.5, 0.75, 1.0] + [-1.0] * 5 for c in aid)
