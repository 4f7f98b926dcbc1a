"""CPU restatement of the float32 attention core with both products formed from bf16 halves (AidAttnArgs.f32_split = 1,
aid_attn_f32x3_kernel in csrc/aid_f32x3.hip); a plain module, imported by tests/test_f32_attn_precision.py and
tests/test_hip_attn_f32x3.py.  Built on split_ref.split:

    Q' = fp32(Q * softmax_scale * log2(e)),  x = xh + xl  for Q', K, V and the unnormalised probabilities P
    ref3  : S = fp32(Kh Q'h + Kl Q'h + Kh Q'l);  P = fp32(exp2(S - max S));  O = (Ph Vh + Ph Vl + Pl Vh) / sum(P)
            — what the split kernel computes, every sum in fp64, the row sum from the UNSPLIT fp32 P
    ref1  : the same with the high halves only (Kh Q'h, Ph Vh): what a kernel that lost its low halves computes
    ref64 : the plain fp64 attention of the float32 inputs
(The kernel takes its maximum tile by tile and rescales; a restatement with the row's global maximum has the same error model.)
"""
import numpy as np
import torch

from split_ref import split

LOG2E = np.float32(1.4426950408889634)


def _heads(x: np.ndarray, h: int) -> np.ndarray:
    n, r, c = x.shape
    return x.reshape(n, r, h, c // h).transpose(0, 2, 1, 3)             # [n, h, rows, d]


def _merge(x: np.ndarray) -> np.ndarray:
    n, h, r, d = x.shape
    return x.transpose(0, 2, 1, 3).reshape(n, r, h * d)


def _f32(x: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(x.astype(np.float32)))


def refs(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale=None):
    """(ref3, ref1, ref64), each [n, s, c] float64, of PLAIN attention for float32 q [n, s, c], k / v [n, l, c]."""
    d = q.shape[-1] // heads
    scale = d ** -0.5 if scale is None else scale
    c2 = np.float32(scale) * LOG2E                                       # the launcher's fp32 product
    qs = (q.detach().float().cpu() * float(c2))                          # fp32 multiply, like the kernel's
    t = lambda z: np.swapaxes(z, -1, -2)      # noqa: E731
    qh, ql = (_heads(z, heads) for z in split(qs))
    kh, kl = (_heads(z, heads) for z in split(k))
    vh, vl = (_heads(z, heads) for z in split(v))

    def finish(scores, low):
        s32 = scores.astype(np.float32).astype(np.float64)               # the fp32 accumulator
        p = np.exp2(s32 - s32.max(axis=-1, keepdims=True)).astype(np.float32)
        ph, pl = split(_f32(p))
        o = ph @ vh
        if low:
            o = o + ph @ vl + pl @ vh
        return _merge(o / p.astype(np.float64).sum(axis=-1, keepdims=True))

    s1 = qh @ t(kh)
    ref3 = finish(s1 + qh @ t(kl) + ql @ t(kh), True)
    ref1 = finish(s1, False)
    q64, k64, v64 = (_heads(z.detach().cpu().numpy().astype(np.float64), heads) for z in (q, k, v))
    sc = q64 @ t(k64) * scale
    p = np.exp(sc - sc.max(axis=-1, keepdims=True))
    ref64 = _merge((p / p.sum(axis=-1, keepdims=True)) @ v64)
    return ref3, ref1, ref64
