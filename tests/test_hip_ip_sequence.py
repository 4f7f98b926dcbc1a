"""GPU: N-frame interpolation with IP-Adapter image prompts.

(a) One call of each IP processor with PLAIN rider frames and shared text contexts against ``oracle/aid_oracle.py``: the cond rows are
    ``outer_ip_attention`` / ``inner_ip_attention`` / ``scale_control_ip_attention`` at N frames, the rider rows ``ip_adapter_attention``.
(b) ``interpolate(image_embeds_*)`` end to end over the stand-in denoiser against an fp64 loop WRITTEN OUT HERE (numpy, the oracle's
    functions per layer; no pipelines.py / sequence.py / interp.py): batch, embeddings, the two passes of a step, guidance, DDIM.
    Bound: the SAME configuration without images and without an adapter, against its own fp64 loop, measured in the same test — that
    text path is the project's yardstick — times 1.3.
(c) batched / two-pass, graphs on / off, ``interpolate(size=3, coef=[0, it, 1])`` against ``interpolate_single(it)``, and a plain run
    after an image run.
Measured on an MI355X (rel-L2 of the final latents, image run / text-only yardstick; 6 steps, size 5): sd15 fp16 fused_outer 2.004e-3 /
2.091e-3, fused_inner 2.004e-3 / 2.108e-3, scale control 1.957e-3 / 2.091e-3; sd15 fp32 fused_outer 1.352e-6 / 1.440e-6, fused_inner
1.370e-6 / 1.443e-6, scale control 1.399e-6 / 1.440e-6; sdxl bf16 fused_outer 1.574e-2 / 2.171e-2.  Most of a case's seconds are the
fp64 loops (the oracle's softmax and projections at the widths of the real layers); they are computed once per configuration and
shared by the tests of (b) and (c)."""
import numpy as np
import pytest
import torch

from oracle import aid_oracle as O
from util import TOL, WORST, rel_l2, to_np64, worst

pytestmark = pytest.mark.gpu

import aid_amd  # noqa: E402
from aid_amd.pipelines import (DDIMSchedulerLite, InterpolationStableDiffusionPipeline,  # noqa: E402
                               InterpolationStableDiffusionXLPipeline, StackDenoiser)

DEV = "cuda:0"
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
REL = {F16: TOL[F16], BF16: TOL[BF16], F32: 1e-5}
ABS = {F16: WORST[F16], BF16: WORST[BF16], F32: 1e-4}
MARGIN = 1.3


# ---- (a) one call ------------------------------------------------------------------------------------------------------------------------
N, S, L, CC = 3, 40, 77, 64
CTX_MAPS = {"identity": [0, 1, 2, 3, 4, 5],                      # one context per frame, spelled out as a map
            "guided": [0, 1, 2, 3, 3, 3],                        # [start, guide, end] + riders that share the negative prompt's context
            "none": None}


def _weights(attn, ipa):
    w = O.AttnWeights(*(to_np64(t) for t in (attn.to_q.weight, attn.to_k.weight, attn.to_v.weight, attn.to_out[0].weight,
                                             attn.to_out[0].bias)), heads=attn.heads)
    ipw = O.IPWeights(to_np64(ipa.to_k_ip[0].weight), to_np64(ipa.to_v_ip[0].weight), float(ipa.scale[0]), ipa.num_tokens[0])
    return w, ipw


@pytest.mark.parametrize("dtype", [F16, BF16, F32], ids=["f16", "bf16", "f32"])
@pytest.mark.parametrize("ctx", list(CTX_MAPS))
@pytest.mark.parametrize("t_ip", [4, 16])
@pytest.mark.parametrize("c,heads", [(80, 2), (128, 2)])
def test_riders_and_shared_contexts_per_call(c, heads, t_ip, ctx, dtype):
    _check_call(N, c, heads, t_ip, CTX_MAPS[ctx], dtype, seed=1000 * c + 10 * t_ip + len(ctx))


@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
def test_five_frames_whose_interior_shares_the_guide_context(dtype):
    """[start, guide x 3, end] and their riders: 3 + 3 distinct contexts for 10 frames, the end points' rows are context rows 0 and 2."""
    _check_call(5, 80, 2, 4, [0, 1, 1, 1, 2, 3, 4, 4, 4, 5], dtype, seed=5)


def _check_call(n, c, heads, t_ip, idx, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)                                      # (the layers' weights come from the global generators)
    n_ctx = 2 * n if idx is None else max(idx) + 1
    x = torch.randn(2 * n, S, c, generator=g).to(dtype).to(DEV)
    text = torch.randn(n_ctx, L, CC, generator=g).to(dtype).to(DEV)
    ip = torch.randn(2 * n, t_ip, CC, generator=g).to(dtype).to(DEV)
    attn = aid_amd.AttnShim(c, heads, CC, dtype=dtype, device=DEV)
    ipa = aid_amd.HipIPAdapterAttnProcessor(hidden_size=c, cross_attention_dim=CC, num_tokens=(t_ip,), scale=0.6, dtype=dtype, device=DEV)
    w, ipw = _weights(attn, ipa)
    x64, ip64 = to_np64(x), to_np64(ip)[:, None]
    t64 = to_np64(text)[list(range(2 * n)) if idx is None else idx]
    for cls, fn in ((aid_amd.OuterInterpolatedIPAttnProcessor, O.outer_ip_attention),
                    (aid_amd.InnerInterpolatedIPAttnProcessor, O.inner_ip_attention),
                    (aid_amd.ScaleControlIPAttnProcessor, O.scale_control_ip_attention)):
        proc = cls(size=n, is_fused=True, ip_attn=ipa)
        proc.coef = torch.tensor([0.0, 0.3, 1.0] if n == 3 else [0.0, 0.2, 0.45, 0.8, 1.0])
        proc.plain_tail = n
        y = proc(attn, x, encoder_hidden_states=(text, [ip]), ctx_index=idx)
        coef = proc.coef.to(dtype).float().numpy().astype(np.float64)
        want = fn(x64[:n], t64[:n], ip64[:n], w, ipw, coef, True)
        if cls is aid_amd.ScaleControlIPAttnProcessor:          # rider j: the END rider's image rows at its frame's coefficient
            riders = np.concatenate([O.ip_adapter_attention(x64[n + j:n + j + 1], t64[n + j:n + j + 1], ip64[2 * n - 1:],
                                                            w, O.IPWeights(ipw.wk_ip, ipw.wv_ip, float(coef[j]), t_ip)) for j in range(n)])
        else:
            riders = O.ip_adapter_attention(x64[n:], t64[n:], ip64[n:], w, ipw)
        want = np.concatenate([want, riders])
        got = to_np64(y)
        for part, sl in (("cond", slice(0, n)), ("riders", slice(n, 2 * n))):
            e, wst = rel_l2(got[sl], want[sl]), worst(got[sl], want[sl])
            print(f"{cls.__name__} {part} rel-L2 {e:.3e} worst {wst:.3e}")
            assert e < REL[dtype] and wst < ABS[dtype], (cls.__name__, part, e, wst)


# ---- (b) the fp64 loop -------------------------------------------------------------------------------------------------------------------
class Loop64:
    """The denoising loop of an interpolation run in numpy fp64 over the weights of a HIP ``StackDenoiser``: lifted latents, every
    layer ``h + attn(LayerNorm(h))`` by the oracle, the drop; conditional and unconditional pass of a step as two passes, AID on in
    the conditional pass of the first ``int(steps * warmup_ratio)`` steps; ``uncond + gs (text - uncond)``; DDIM (eta = 0) on SD's
    scaled-linear schedule, "leading" spacing, offset 1.  ``variant``: None (text), "interpolate", "scale_control"."""

    def __init__(self, hip: StackDenoiser):
        self.hip, self.st = hip, hip.stack
        self.w = []
        for m, nrm, (s, c, heads, is_cross) in zip(self.st.layers, self.st.norms, self.st.shapes):
            w = O.AttnWeights(*(to_np64(t) for t in (m.to_q.weight, m.to_k.weight, m.to_v.weight, m.to_out[0].weight, m.to_out[0].bias)),
                              heads=heads)
            ipa = m.processor if hasattr(m.processor, "to_k_ip") else getattr(m.processor, "ip_attn", None)
            ipw = None
            if ipa is not None and hasattr(ipa, "to_k_ip"):
                ipw = O.IPWeights(to_np64(ipa.to_k_ip[0].weight), to_np64(ipa.to_v_ip[0].weight), float(ipa.scale[0]), ipa.num_tokens[0])
            self.w.append((w, ipw, to_np64(nrm.weight), to_np64(nrm.bias), nrm.eps))
        self.lift = {k: to_np64(v) for k, v in hip.lift.items()}
        self.drop = {k: to_np64(v) for k, v in hip.drop.items()}

    def _pass(self, lat, t, text, ip, aid, mode, fused, coef, variant):
        n = lat.shape[0]
        flat = lat.reshape(n, -1)
        hs = {}
        for (s, c) in self.st.level_shapes():
            tok = (flat @ self.lift[f"{s}_{c}"]).reshape(n, s, 8)
            hs[(s, c)] = np.tile(tok, (1, 1, c // 8)) + float(t) * self.hip.time_scale
        for (w, ipw, gam, bet, eps), (s, c, heads, is_cross) in zip(self.w, self.st.shapes):
            h = hs[(s, c)]
            hn = O.layer_norm(h, gam, bet, eps)
            ctx = text if is_cross else None
            if is_cross and ipw is not None and variant == "scale_control":
                a = O.scale_control_ip_attention(hn, ctx, ip, w, ipw, coef, fused, activated=aid)
            elif is_cross and ipw is not None and variant == "interpolate":
                if aid:
                    a = (O.outer_ip_attention if mode == "outer" else O.inner_ip_attention)(hn, ctx, ip, w, ipw, coef, fused)
                else:
                    a = O.ip_adapter_attention(hn, ctx, ip, w, ipw)
            elif aid:
                a = (O.outer_attention if mode == "outer" else O.inner_attention)(hn, ctx, w, coef, fused)
            else:
                a = O.plain_attention(hn, ctx, w)
            hs[(s, c)] = h + a
        out = np.zeros_like(flat)
        for (s, c) in self.st.level_shapes():
            hm = hs[(s, c)].reshape(n, s, c // 8, 8).mean(axis=2)
            out = out + hm.reshape(n, s * 8) @ self.drop[f"{s}_{c}"]
        return (out / len(self.st.level_shapes())).reshape(lat.shape)

    def run(self, lat, cond, unc, coef, steps, gs, early, img=None, variant=None, warmup_ratio=0.5):
        """``lat`` [N, 4, h, w], ``cond`` / ``unc`` [N, L, Cc], ``coef`` [N] (already rounded to the storage dtype), ``img`` =
        (positive rows, negative rows) [N, 1, T, Cc] each."""
        mode, fused = early.split("_")[1], early.startswith("fused")
        ac = np.cumprod(1.0 - np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000) ** 2)
        ts = [int(v) for v in (np.arange(steps) * (1000 // steps))[::-1] + 1]
        warm = int(steps * warmup_ratio)
        pos, neg = img if img is not None else (None, None)
        for i, t in enumerate(ts):
            eps_text = self._pass(lat, t, cond, pos, i < warm, mode, fused, coef, variant)
            eps_unc = self._pass(lat, t, unc, neg, False, mode, fused, coef, variant)
            eps = eps_unc + gs * (eps_text - eps_unc)
            a_t, a_prev = ac[t], (ac[ts[i + 1]] if i + 1 < len(ts) else 1.0)
            x0 = (lat - np.sqrt(1 - a_t) * eps) / np.sqrt(a_t)
            lat = np.sqrt(a_prev) * x0 + np.sqrt(1 - a_prev) * eps
        return lat


STEPS, SIZE, T_IP, SCALE = 6, 5, 4, 0.6


def _denoiser(model, dtype, adapter):
    kw = dict(scale_down=16, latent_hw=(8, 8)) if model == "sd15" else dict(scale_down=64, latent_hw=(8, 8), head_div=5)
    hip = StackDenoiser(model, dtype=dtype, device=DEV, **kw)
    if adapter:
        hip.stack.load_ip_adapter(num_tokens=T_IP, scale=SCALE)
    return hip


def _inputs(model, dtype):
    """Everything a run takes, rounded to the storage dtype once: both sides see the same numbers."""
    g = torch.Generator().manual_seed(31)
    cc = 768 if model == "sd15" else 2048
    r = lambda *s: torch.randn(*s, generator=g).to(dtype)       # noqa: E731
    d = dict(l0=r(1, 4, 8, 8), l1=r(1, 4, 8, 8), es=(r(1, 77, cc), r(1, 77, cc)), ee=(r(1, 77, cc), r(1, 77, cc)),
             img_s=(r(1, T_IP, cc), r(1, T_IP, cc)), img_e=(r(1, T_IP, cc), r(1, T_IP, cc)))      # (negative, positive) image embeddings
    if model == "sdxl":                                         # pooled embeddings ride along (the stand-in does not read them)
        d["es"], d["ee"] = d["es"] + (r(1, 32), r(1, 32)), d["ee"] + (r(1, 32), r(1, 32))
    return d


def _beta_coef(size, steps, dtype):
    coef = aid_amd.generate_beta_tensor(size, alpha=steps, beta=steps)
    coef[0], coef[-1] = 0, 1
    return coef.to(dtype).float().numpy().astype(np.float64), [float(v) for v in coef.tolist()]


def _mix_rows(a, b, ts):
    """[N, 1, T, Cc] fp64: frame k = a + t_k (b - a), the end frames the end points' own rows."""
    a, b = to_np64(a), to_np64(b)
    return np.concatenate([a] + [a + t * (b - a) for t in ts[1:-1]] + [b])[:, None]


def _reference(loop, d, early, variant, ts_lat, ts_emb, coef_attn, ts_img, gs):
    """The fp64 loop's final latents.  Latents slerp'd at ``ts_lat``, text embeddings lerp'd at ``ts_emb``, attention coefficients
    ``coef_attn``, image embeddings mixed at ``ts_img``."""
    l0, l1 = to_np64(d["l0"]), to_np64(d["l1"])
    lat = np.concatenate([l0] + [O.slerp(l0, l1, t) for t in ts_lat[1:-1]] + [l1])
    cond = O.linear_interpolation(to_np64(d["es"][0]), to_np64(d["ee"][0]), ts=ts_emb)
    unc = O.linear_interpolation(to_np64(d["es"][1]), to_np64(d["ee"][1]), ts=ts_emb)
    img = None
    if variant == "interpolate":
        img = (_mix_rows(d["img_s"][1], d["img_e"][1], ts_img), _mix_rows(d["img_s"][0], d["img_e"][0], ts_img))
    elif variant == "scale_control":                            # the start rows are the end image's negative embedding
        img = (_mix_rows(d["img_e"][0], d["img_e"][1], ts_img), _mix_rows(d["img_e"][0], d["img_e"][0], ts_img))
    return loop.run(lat, cond, unc, coef_attn, STEPS, gs, early, img, variant)


_CACHE = {}


def _setup(model, dtype, early, variant):
    """HIP denoisers, the fp64 references of the image run and of the text-only yardstick run, and the yardstick's measured error —
    computed once per configuration and shared by the tests below (never modified)."""
    key = (model, dtype, early, variant)
    if key in _CACHE:
        return _CACHE[key]
    cls = InterpolationStableDiffusionXLPipeline if model == "sdxl" else InterpolationStableDiffusionPipeline
    gs = cls.default_guidance_scale
    d = _inputs(model, dtype)
    coef, ts = _beta_coef(SIZE, STEPS, dtype)
    uniform = [i / (SIZE - 1) for i in range(SIZE)]
    kw = dict(size=SIZE, num_inference_steps=STEPS, warmup_ratio=0.5, early=early, output_type="latent", embeds_start=d["es"],
              embeds_end=d["ee"])
    tkey = (model, dtype, early, None)
    if tkey not in _CACHE:                                      # the yardstick: no images, no adapter
        plain = _denoiser(model, dtype, adapter=False)
        ref_t = _reference(Loop64(plain), d, early, None, uniform, uniform, coef, ts, gs)
        out_t = cls(plain, DDIMSchedulerLite()).interpolate(d["l0"].to(DEV), d["l1"].to(DEV), **kw)
        _CACHE[tkey] = dict(err_text=rel_l2(to_np64(out_t), ref_t))
    err_text = _CACHE[tkey]["err_text"]
    if variant is None:
        return _CACHE[tkey]
    hip = _denoiser(model, dtype, adapter=True)
    ref = _reference(Loop64(hip), d, early, variant, uniform, uniform, coef, ts, gs)
    img = dict(image_embeds_end=d["img_e"])
    if variant == "interpolate":
        img["image_embeds_start"] = d["img_s"]
    ent = dict(pipe=cls(hip, DDIMSchedulerLite()), hip=hip, d=d, kw=kw, img=img, ref=ref, err_text=err_text, gs=gs, loop=None)
    _CACHE[key] = ent
    return ent


def _run(ent, **over):
    d = ent["d"]
    return ent["pipe"].interpolate(d["l0"].to(DEV), d["l1"].to(DEV), **dict(ent["kw"], **ent["img"], **over))


CASES = [("sd15", F16, "fused_outer", "interpolate"), ("sd15", F16, "fused_inner", "interpolate"), ("sd15", F16, "fused_outer", "scale_control"),
         ("sd15", F32, "fused_outer", "interpolate"), ("sd15", F32, "fused_inner", "interpolate"), ("sd15", F32, "fused_outer", "scale_control"),
         ("sdxl", BF16, "fused_outer", "interpolate")]
IDS = [f"{m}-{str(dt)[6:]}-{e}-{v}" for m, dt, e, v in CASES]


@pytest.mark.parametrize("model,dtype,early,variant", CASES, ids=IDS)
def test_image_run_end_to_end_within_the_text_runs_error(model, dtype, early, variant):
    ent = _setup(model, dtype, early, variant)
    out = _run(ent)
    err = rel_l2(to_np64(out), ent["ref"])
    print(f"{model} {dtype} {early} {variant}: image run rel-L2 {err:.3e}, text run {ent['err_text']:.3e}")
    assert out.shape == (SIZE, 4, 8, 8) and ent["err_text"] > 0
    assert err <= MARGIN * ent["err_text"], (err, ent["err_text"])


# ---- (c) consistency ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,dtype,early,variant", [CASES[0], CASES[1], CASES[2], CASES[5]], ids=[IDS[0], IDS[1], IDS[2], IDS[5]])
def test_batched_two_pass_and_graphs_agree(model, dtype, early, variant):
    ent = _setup(model, dtype, early, variant)
    bound = MARGIN * ent["err_text"]
    outs = {}
    for batched in (True, False):
        for graphs in (True, False):
            outs[(batched, graphs)] = o = _run(ent, batched_cfg=batched, use_graphs=graphs).clone()
            err = rel_l2(to_np64(o), ent["ref"])
            print(f"batched_cfg={batched} use_graphs={graphs}: rel-L2 {err:.3e} (bound {bound:.3e})")
            assert err <= bound, (batched, graphs, err, bound)
        assert torch.equal(outs[(batched, True)], outs[(batched, False)])            # a replayed graph is the eager pass, bit for bit


@pytest.mark.parametrize("early,variant", [("fused_outer", "interpolate"), ("fused_inner", "interpolate"), ("fused_outer", "scale_control")])
def test_size_three_with_coef_and_interpolate_single_meet_the_same_loop(early, variant):
    model, dtype, it = "sd15", F16, 0.35
    ent = _setup(model, dtype, early, variant)
    bound = MARGIN * ent["err_text"]
    d, hip, pipe = ent["d"], ent["hip"], ent["pipe"]
    itr = float(torch.tensor(it).to(dtype))
    ts = [0.0, it, 1.0]
    ref = _reference(Loop64(hip), d, early, variant, ts, ts, np.array([0.0, itr, 1.0]), ts, ent["gs"])
    kw = dict(ent["kw"], size=3, coef=ts)
    seq = pipe.interpolate(d["l0"].to(DEV), d["l1"].to(DEV), **kw, **ent["img"])
    installed = dict(hip.attn_processors)
    try:
        pipe.load_aid_ip_adapter(t=0.5, is_fused=True, early=early if variant == "interpolate" else "scale_control")
        single = pipe.interpolate_single(it, latent_start=d["l0"], latent_end=d["l1"], embeds_start=d["es"], embeds_end=d["ee"],
                                         num_inference_steps=STEPS, warmup_ratio=0.5, output_type="latent", **ent["img"])["images"]
    finally:
        hip.set_attn_processor(installed)
    for name, o in (("interpolate(size=3, coef)", seq), ("interpolate_single", single)):
        err = rel_l2(to_np64(o), ref)
        print(f"{name}: rel-L2 {err:.3e} (bound {bound:.3e})")
        assert o.shape == (3, 4, 8, 8) and err <= bound, (name, err, bound)


def test_a_plain_run_after_an_image_run_is_the_plain_run_before_it():
    ent = _setup("sd15", F16, "fused_outer", "interpolate")
    d, pipe, hip = ent["d"], ent["pipe"], ent["hip"]
    installed = dict(hip.attn_processors)
    before = pipe.interpolate(d["l0"].to(DEV), d["l1"].to(DEV), **ent["kw"]).clone()
    _run(ent)
    assert dict(hip.attn_processors) == installed
    after = pipe.interpolate(d["l0"].to(DEV), d["l1"].to(DEV), **ent["kw"])
    assert torch.equal(before, after)


def test_two_adapters_fall_back_to_two_passes_with_the_two_pass_result():
    """Riders cannot stand for the de-activated pass of two adapters: ``batched_cfg=True`` then runs the two passes separately — the
    result of ``batched_cfg=False``, bit for bit."""
    dtype = F16
    hip = _denoiser("sd15", dtype, adapter=True)
    g = torch.Generator(device=DEV).manual_seed(3)
    for m in hip.stack.layers:
        p = m.processor
        if hasattr(p, "to_k_ip"):
            for lst in (p.to_k_ip, p.to_v_ip):
                lin = torch.nn.Linear(768, lst[0].weight.shape[0], bias=False, dtype=dtype, device=DEV)
                with torch.no_grad():
                    lin.weight.copy_((torch.randn(lin.weight.shape, generator=g, device=DEV) / 768 ** 0.5).to(dtype))
                lst.append(lin)
            p.scale.append(0.3)
            p.num_tokens = p.num_tokens + (T_IP,)
    d = _inputs("sd15", dtype)
    two = lambda pair: tuple([t, t.flip(1)] for t in pair)      # noqa: E731   (negative, positive), a tensor per adapter each
    pipe = InterpolationStableDiffusionPipeline(hip, DDIMSchedulerLite())
    kw = dict(size=SIZE, num_inference_steps=STEPS, warmup_ratio=0.5, output_type="latent", embeds_start=d["es"], embeds_end=d["ee"],
              image_embeds_start=two(d["img_s"]), image_embeds_end=two(d["img_e"]))
    a = pipe.interpolate(d["l0"].to(DEV), d["l1"].to(DEV), batched_cfg=True, **kw).clone()
    b = pipe.interpolate(d["l0"].to(DEV), d["l1"].to(DEV), batched_cfg=False, **kw)
    assert torch.isfinite(a).all() and torch.equal(a, b)
