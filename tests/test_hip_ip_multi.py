"""GPU: several IP-Adapters per layer, regional ip_adapter_masks and a text attention_mask beside image embeddings.

``aid_ip_attn_fwd`` (csrc/aid_attn_ip.hip) against fp64 on the same dtype-rounded inputs, its memory contract on guarded buffers, whole
``HipIPAdapterAttnProcessor`` calls against the fp64 restatement of diffusers' IPAdapterAttnProcessor2_0 (tests/ip_multi_ref.py), the
unchanged single-adapter path, the activated IP processors' adapter-0 quirk, and one graph capture.  Bounds: TOL / WORST of util.py."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import aid_amd  # noqa: E402
from aid_amd import _lib, ops  # noqa: E402
from guarded import Guarded  # noqa: E402
from ip_multi_ref import ip_adapter_multi, segments_sum  # noqa: E402
from peft_double import effective_weight, wrap_attention  # noqa: E402
from util import TOL, WORST, rel_l2, to_np64, worst  # noqa: E402

DEV = torch.device("cuda:0")
DTYPES = [torch.float16, torch.bfloat16]


def _rand(shape, dtype, g, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def _segment(r, t, c, dtype, g, ldvt=None):
    """(k [r, t, c], v [r, t, c], vt [r, c, ldvt] with NaN in the pad columns) on the CPU."""
    k, v = _rand((r, t, c), dtype, g), _rand((r, t, c), dtype, g)
    ldvt = (t + 7) // 8 * 8 if ldvt is None else ldvt
    vt = torch.full((r, c, ldvt), float("nan"), dtype=dtype)
    vt[:, :, :t] = v.transpose(1, 2)
    return k, v, vt


def _weights(kind, s, g):
    if kind == "none":
        return None
    w = torch.rand(s, generator=g)
    if kind == "zeros":
        w[torch.rand(s, generator=g) < 0.4] = 0.0
        w[0] = 0.0
    return w.to(torch.float32)


def _check(got, ref, dtype, what=""):
    r, w = rel_l2(got, ref), worst(got, ref)
    print(f"{what} rel-L2 {r:.3e} worst {w:.3e}")
    assert r < TOL[dtype], (what, r)
    assert w < WORST[dtype], (what, w)


# ---- kernel ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("wkind", ["none", "uniform", "zeros"])
@pytest.mark.parametrize("d", [40, 64, 80, 160])
@pytest.mark.parametrize("dtype", DTYPES)
def test_segments_in_one_launch_match_fp64(dtype, d, wkind, accumulate):
    """N = 2, S = 67 (three row tiles, the last of 3 rows), 2 heads; segments of 4, 16 and 33 keys (33: two score tiles, the second of
    one key) in ONE launch, the first shared by the frames (n_rows = 1), the second with a negative scale.  With out = 0 the image term
    alone is measured; otherwise it is added onto N(0, 0.3) data."""
    g = torch.Generator().manual_seed(1000 * d + 7)
    n, s, heads = 2, 67, 2
    c = heads * d
    q = _rand((n, s, c), dtype, g)
    segs, ref = [], []
    for t, scale, r in ((4, 0.7, 1), (16, -0.5, n), (33, 1.0, n)):
        k, v, vt = _segment(r, t, c, dtype, g)
        w = _weights(wkind, s, g)
        segs.append(dict(k=k.to(DEV), vt=vt.to(DEV), scale=scale, row_weight=None if w is None else w.to(DEV)))
        ref.append((to_np64(k), to_np64(v), scale, None if w is None else to_np64(w)))
    out0 = _rand((n, s, c), dtype, g, 0.3) if accumulate else torch.zeros(n, s, c, dtype=dtype)
    out = out0.clone().to(DEV)
    assert ops.ip_attn_accumulate(q.to(DEV), out, segs, heads) is out
    torch.cuda.synchronize()
    _check(to_np64(out), to_np64(out0) + segments_sum(to_np64(q), ref, heads), dtype, f"{dtype} d{d} {wkind} acc={accumulate}")


@pytest.mark.parametrize("d", [40, 64, 80, 160])
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_row_one_key(dtype, d):
    """S = 1, t = 1: the softmax over one key is 1, so the launch adds scale * w * V exactly (one rounding of the sum)."""
    g = torch.Generator().manual_seed(d)
    n, heads = 2, 2
    c = heads * d
    q, out0 = _rand((n, 1, c), dtype, g), _rand((n, 1, c), dtype, g, 0.3)
    k, v, vt = _segment(n, 1, c, dtype, g)
    w = torch.tensor([0.75])
    out = out0.clone().to(DEV)
    ops.ip_attn_accumulate(q.to(DEV), out, [dict(k=k.to(DEV), vt=vt.to(DEV), scale=-1.5, row_weight=w.to(DEV))], heads)
    want = (out0.float() + (-1.5 * 0.75) * v.float()).to(dtype)
    assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize("d", [40, 64, 80, 160])
@pytest.mark.parametrize("dtype", DTYPES)
def test_memory_contract_on_guarded_buffers(dtype, d):
    """q, k, V^T in buffers whose pad columns, gap rows and guard bands hold NaN; `out` between sentinel bands with a row stride wider
    than the view: the result is finite and right, no input bit changes, and only the [n, s, heads d] view of `out` is written."""
    g = torch.Generator().manual_seed(d + 1)
    n, s, heads = 2, 67, 2
    c = heads * d
    lib = _lib.load()
    qg = Guarded(n, s, c, dtype, DEV, ld=c + 8, gap_rows=1).set(_rand((n, s, c), dtype, g))
    og = Guarded(n, s, c, dtype, DEV, ld=c + 16, gap_rows=2, kind="output")
    out0 = _rand((n, s, c), dtype, g, 0.3)
    og.view.copy_(out0)
    segs = (_lib.AidIpSegment * 3)()
    ref, keep = [], []
    for i, (t, scale, r, ldvt) in enumerate(((4, 0.7, 1, 8), (16, -0.5, n, 24), (33, 1.0, n, 40))):
        k, v = _rand((r, t, c), dtype, g), _rand((r, t, c), dtype, g)
        kg = Guarded(r, t, c, dtype, DEV, gap_rows=3).set(k)                       # rows >= t of every frame: NaN
        vg = Guarded(r, c, t, dtype, DEV, ld=ldvt, gap_rows=1).set(v.transpose(1, 2))   # columns [t, ldvt): NaN
        w = _weights("uniform", s, g).to(DEV)
        keep += [kg, vg, w]
        e = segs[i]
        e.k, e.vt, e.row_weight = kg.ptr, vg.ptr, w.data_ptr()
        e.k_fs, e.vt_fs, e.t, e.ldvt, e.n_rows, e.scale = kg.fs, vg.fs, t, ldvt, r, scale
        ref.append((to_np64(k), to_np64(v), scale, to_np64(w)))
    a = _lib.AidIpAttnArgs()
    a.q, a.out, a.segments, a.n_segments = qg.ptr, og.ptr, C.addressof(segs), 3
    a.n_frames, a.s, a.heads, a.d = n, s, heads, d
    a.ldq, a.ldo, a.q_fs, a.o_fs = qg.ld, og.ld, qg.fs, og.fs
    a.dtype, a.softmax_scale = ops._dtype_code(qg.view), d ** -0.5
    _lib.check(lib.aid_ip_attn_fwd(C.byref(a), torch.cuda.current_stream().cuda_stream), "aid_ip_attn_fwd")
    torch.cuda.synchronize()
    got = to_np64(og.view)
    assert np.isfinite(got).all()
    _check(got, to_np64(out0) + segments_sum(to_np64(qg.view), ref, heads), dtype, f"guarded {dtype} d{d}")
    assert og.untouched(og.layout.region_mask()) == ""
    for buf in [qg] + [b for b in keep if isinstance(b, Guarded)]:
        assert buf.inputs_unchanged() == ""


# ---- processor ---------------------------------------------------------------------------------------------------------------------
# (S, C, heads, Cc): d = 40 and d = 64; the third has two workgroups per (frame, head) in the image-segment kernel, and its S = 160 takes
# the zero-padding branch of the mask downsample (32 x 32 -> 13 x 12 = 156 < 160)
SHAPES = [(64, 320, 8, 64), (16, 1280, 20, 64), (160, 128, 2, 64)]
N, L = 3, 77


def _layer(shape, dtype, scales, tokens, seed, lora=False):
    s, c, heads, cc = shape
    torch.manual_seed(seed)
    attn = aid_amd.AttnShim(c, heads, cc, dtype=dtype, device=DEV)
    if lora:
        wrap_attention(attn, {"a": (8, 8.0)}, targets=("to_q", "to_out"), seed=seed)
        for m in (attn.to_q, attn.to_out[0]):
            m.to(DEV)
    proc = aid_amd.HipIPAdapterAttnProcessor(hidden_size=c, cross_attention_dim=cc, num_tokens=tokens, scale=scales).to(DEV, dtype)
    g = torch.Generator().manual_seed(seed + 1)
    x, text = _rand((N, s, c), dtype, g).to(DEV), _rand((N, L, cc), dtype, g).to(DEV)
    return attn, proc, x, text, g


def _oracle(attn, proc, x, text, ips, masks, dtype, attention_mask=None):
    w = tuple(effective_weight(m).numpy() for m in (attn.to_q, attn.to_k, attn.to_v, attn.to_out[0])) + (to_np64(attn.to_out[0].bias),)
    return ip_adapter_multi(to_np64(x), to_np64(text), [to_np64(i) for i in ips], w,
                            [to_np64(m.weight) for m in proc.to_k_ip], [to_np64(m.weight) for m in proc.to_v_ip],
                            list(proc.scale), masks, attn.heads, dtype,
                            None if attention_mask is None else to_np64(attention_mask))


@pytest.mark.parametrize("kind", ["two", "masked", "attention_mask", "lora", "scale0"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_processor_matches_the_fp64_restatement(dtype, shape, kind):
    s, c, heads, cc = shape
    masks = amask = None
    if kind in ("two", "lora"):                          # two adapters, 4 and 16 tokens (and unmerged LoRA on to_q / to_out)
        attn, proc, x, text, g = _layer(shape, dtype, [0.6, 0.4], (4, 16), 1, lora=kind == "lora")
        ips = [_rand((N, 4, cc), dtype, g).to(DEV), _rand((N, 1, 16, cc), dtype, g).to(DEV)]
    elif kind == "masked":                               # the second adapter: two images, a regional mask, one scale per image
        attn, proc, x, text, g = _layer(shape, dtype, [0.6, [0.5, 0.8]], (4, 16), 2)
        ips = [_rand((N, 1, 4, cc), dtype, g).to(DEV), _rand((N, 2, 16, cc), dtype, g).to(DEV)]
        m = torch.zeros(1, 2, 32, 32)
        m[0, 0, :, :16] = 1.0
        m[0, 1, :, 16:] = 1.0
        masks = [None, m]
    elif kind == "attention_mask":                       # a text mask beside ONE adapter: the mask covers the text scores only
        attn, proc, x, text, g = _layer(shape, dtype, [0.7], (4,), 3)
        ips = [_rand((N, 4, cc), dtype, g).to(DEV)]
        amask = torch.zeros(N, 1, L, dtype=dtype)
        amask[:, :, 50:] = -10000.0
        amask[1, :, 20:] = -10000.0
        amask = amask.to(DEV)
    else:                                                # one adapter with scale 0: the text attention alone
        attn, proc, x, text, g = _layer(shape, dtype, [0.0], (4,), 4)
        ips = [_rand((N, 4, cc), dtype, g).to(DEV)]
    y = proc(attn, x, encoder_hidden_states=(text, ips), attention_mask=amask, ip_adapter_masks=masks)
    torch.cuda.synchronize()
    _check(to_np64(y), _oracle(attn, proc, x, text, ips, masks, dtype, amask), dtype, f"{kind} {shape} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_single_unmasked_adapter_is_bit_identical_to_the_ip_form(dtype):
    """One adapter without masks stays on the ip_* form of aid_processor_fwd: the bits of the direct call."""
    shape = SHAPES[0]
    attn, proc, x, text, g = _layer(shape, dtype, [0.7], (4,), 5)
    ip = _rand((N, 4, shape[3]), dtype, g).to(DEV)
    y = proc(attn, x, encoder_hidden_states=(text, [ip]))
    lin = attn.to_out[0]
    want = ops.processor_fwd(x, text, attn.to_q.weight, attn.to_k.weight, attn.to_v.weight, lin.weight, lin.bias, attn.heads, mode="plain",
                             ip=dict(tokens=ip, wk=proc.to_k_ip[0].weight, wv=proc.to_v_ip[0].weight, mode="plain", scale=0.7))
    assert torch.equal(y, want)


@pytest.mark.parametrize("cls", ["outer", "inner", "scale_control"])
def test_activated_ip_processors_read_adapter_0(cls):
    """With two adapters loaded the ACTIVATED processors compute what they compute with adapter 0 alone (the reference reads
    ip_hidden_states[0] / to_k_ip[0] / scale[0]); de-activated, Outer / Inner run every adapter through the wrapped processor."""
    dtype, shape = torch.float16, SHAPES[0]
    attn, both, x, text, g = _layer(shape, dtype, [0.6, 0.4], (4, 16), 6)
    ips = [_rand((N, 4, shape[3]), dtype, g).to(DEV), _rand((N, 16, shape[3]), dtype, g).to(DEV)]
    first = aid_amd.HipIPAdapterAttnProcessor(num_tokens=(4,), scale=[0.6])
    first.to_k_ip, first.to_v_ip = both.to_k_ip[:1], both.to_v_ip[:1]
    kind = {"outer": aid_amd.OuterInterpolatedIPAttnProcessor, "inner": aid_amd.InnerInterpolatedIPAttnProcessor,
            "scale_control": aid_amd.ScaleControlIPAttnProcessor}[cls]
    p2, p1 = kind(t=0.5, is_fused=True, ip_attn=both), kind(t=0.5, is_fused=True, ip_attn=first)
    assert torch.equal(p2(attn, x, encoder_hidden_states=(text, ips)), p1(attn, x, encoder_hidden_states=(text, ips[:1])))
    p2.deactivate()
    p1.deactivate()
    y = p2(attn, x, encoder_hidden_states=(text, ips))
    if cls == "scale_control":                            # (its de-activated form is its own call, adapter 0 again)
        assert torch.equal(y, p1(attn, x, encoder_hidden_states=(text, ips[:1])))
    else:
        _check(to_np64(y), _oracle(attn, both, x, text, ips, None, dtype), dtype, f"de-activated {cls}")


def test_graph_capture_of_a_masked_two_adapter_call():
    dtype, shape = torch.bfloat16, SHAPES[0]
    attn, proc, x, text, g = _layer(shape, dtype, [0.6, [0.5, 0.8]], (4, 16), 7)
    ips = [_rand((N, 1, 4, shape[3]), dtype, g).to(DEV), _rand((N, 2, 16, shape[3]), dtype, g).to(DEV)]
    m = torch.rand(1, 2, 32, 32, generator=g)
    call = lambda: proc(attn, x, encoder_hidden_states=(text, ips), ip_adapter_masks=[None, m])     # noqa: E731
    y_eager = call().clone()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        call()
        with torch.cuda.graph(graph, stream=st):
            y_g = call()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y_g, y_eager)
