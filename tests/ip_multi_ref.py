"""fp64 restatement of diffusers' ``IPAdapterAttnProcessor2_0`` (0.27 - 0.31) with several adapters per layer, regional
``ip_adapter_masks`` and a text ``attention_mask`` — the yardstick of tests/test_ip_multi_abi.py and tests/test_hip_ip_multi.py
(a plain module; diffusers itself is third-party and not installed where the suite runs).

    q = to_q(x);  o = A(q, to_k(text), to_v(text); attention_mask)            the mask covers the TEXT scores only
    adapter j (ip_j, scale_j, to_k_ip[j], to_v_ip[j], mask_j), skipped when scale_j == 0 or a list of zeros:
        mask_j is None:  o += scale_j * A(q, K(ip_j), V(ip_j))                ip_j [B, E, T, Cc] / [B, T, Cc]: E T tokens, one segment
        mask_j [1, E, H, W]:  for every image e:  o += scale_j[e] * w_je[s] * A(q, K(ip_j[:, e]), V(ip_j[:, e]))
            w_je = IPAdapterMaskProcessor.downsample(mask_j[:, e], B, S, C)[0, :, 0]
    y = to_out(o)
"""
import math

import numpy as np
import torch
import torch.nn.functional as F


def downsample(mask: torch.Tensor, batch_size: int, num_queries: int, value_embed_dim: int) -> torch.Tensor:
    """``IPAdapterMaskProcessor.downsample`` line by line: mask [1, H, W] -> [batch, num_queries, value_embed_dim]."""
    o_h, o_w = mask.shape[1], mask.shape[2]
    ratio = o_w / o_h
    mask_h = int(math.sqrt(num_queries / ratio))
    mask_h = int(mask_h) + int((num_queries % int(mask_h)) != 0)
    mask_w = num_queries // mask_h
    mask_downsample = F.interpolate(mask.unsqueeze(0), size=(mask_h, mask_w), mode="bicubic").squeeze(0)
    if mask_downsample.shape[0] < batch_size:
        mask_downsample = mask_downsample.repeat(batch_size, 1, 1)
    mask_downsample = mask_downsample.view(mask_downsample.shape[0], -1)
    downsampled_area = mask_h * mask_w
    if downsampled_area < num_queries:
        mask_downsample = F.pad(mask_downsample, (0, num_queries - mask_downsample.shape[1]), value=0.0)
    if downsampled_area > num_queries:
        mask_downsample = mask_downsample[:, :num_queries]
    return mask_downsample.view(mask_downsample.shape[0], mask_downsample.shape[1], 1).repeat(1, 1, value_embed_dim)


def row_weights(mask: torch.Tensor, num_queries: int, dtype: torch.dtype) -> np.ndarray:
    """w[s] of one image's mask [1, H, W] as the processor applies it: downsampled, cast to the activation dtype; fp64 [S]."""
    w = downsample(mask.detach().cpu().float(), 1, num_queries, 1)[0, :, 0]
    return w.to(dtype).double().numpy()


def attention(q: np.ndarray, k: np.ndarray, v: np.ndarray, heads: int, bias=None) -> np.ndarray:
    """softmax(q k^T / sqrt(d) + bias) v per head; q [N, S, C], k / v [N or 1, L, C], bias broadcastable to [N, H, S, L]."""
    n, s, c = q.shape
    d = c // heads
    qh = q.reshape(n, s, heads, d).transpose(0, 2, 1, 3)
    kh = np.broadcast_to(k, (n,) + k.shape[1:]).reshape(n, -1, heads, d).transpose(0, 2, 1, 3)
    vh = np.broadcast_to(v, (n,) + v.shape[1:]).reshape(n, -1, heads, d).transpose(0, 2, 1, 3)
    sc = qh @ kh.transpose(0, 1, 3, 2) / math.sqrt(d)
    if bias is not None:
        sc = sc + bias
    sc = sc - sc.max(-1, keepdims=True)
    p = np.exp(sc)
    p /= p.sum(-1, keepdims=True)
    return (p @ vh).transpose(0, 2, 1, 3).reshape(n, s, c)


def segments_sum(q: np.ndarray, segs, heads: int) -> np.ndarray:
    """sum_g scale_g * w_g[s] * A(q, k_g, v_g); segs = [(k [R, t, C], v [R, t, C], scale, w [S] or None)]."""
    out = np.zeros_like(q)
    for k, v, scale, w in segs:
        o = attention(q, k, v, heads) * scale
        if w is not None:
            o = o * np.asarray(w, np.float64)[None, :, None]
        out += o
    return out


def ip_adapter_multi(x, text, ip_states, w, wk_ip, wv_ip, scales, masks, heads, dtype, attention_mask=None) -> np.ndarray:
    """The whole layer in fp64.  x [N, S, C], text [N, L, Cc], ip_states: list of [N, E, T, Cc] / [N, T, Cc] (fp64 numpy);
    w = (wq, wk, wv, wo, bo); wk_ip / wv_ip lists of [C, Cc]; scales: floats or lists; masks: None or a list of None / torch
    [1, E, H, W]; attention_mask: additive [N, 1, L] or None."""
    wq, wk, wv, wo, bo = w
    n, s, _ = x.shape
    q = x @ wq.T
    bias = None if attention_mask is None else np.asarray(attention_mask, np.float64)[:, None, :, :]
    o = attention(q, text @ wk.T, text @ wv.T, heads, bias)
    masks = [None] * len(scales) if masks is None else masks
    for ip, scale, kw, vw, mask in zip(ip_states, scales, wk_ip, wv_ip, masks):
        if isinstance(scale, list):
            if all(v == 0 for v in scale):
                continue
        elif scale == 0:
            continue
        if mask is not None:
            sc = scale if isinstance(scale, list) else [scale] * mask.shape[1]
            for e in range(mask.shape[1]):
                tok = ip[:, e].reshape(n, -1, ip.shape[-1])
                wgt = row_weights(mask[:, e], s, dtype)
                o = o + sc[e] * attention(q, tok @ kw.T, tok @ vw.T, heads) * wgt[None, :, None]
        else:
            tok = ip.reshape(n, -1, ip.shape[-1])
            o = o + scale * attention(q, tok @ kw.T, tok @ vw.T, heads)
    return o @ wo.T + bo
