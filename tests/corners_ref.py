"""fp64 reference of corner-weighted AID (include/aid_hip.h, "Corner-weighted AID"; a plain module, imported by the corner tests).

Corners are rows r_0 .. r_{M-1} of k / v; frame i has the non-negative weight row w[i, 0 .. M):

    OUTER : O_i = sum_m w[i, m] * A(Q_i, [K_i ;] K[r_m], [V_i ;] V[r_m])
    INNER : Kc_i = sum_m w[i, m] * K[r_m]   (same for V);   O_i = A(Q_i, [K_i ;] Kc_i, [V_i ;] Vc_i)

``[K_i ;]`` is present when ``fused``; A(Q, K, V) = softmax(Q K^T * scale) V per head.  The last ``n_plain`` frames are PLAIN riders:
O_i = A(Q_i, K_i, V_i); their weight rows are not read.  Evaluated in float64 on the inputs as the caller rounded them to the storage
dtype; every sum runs in corner order."""
import numpy as np

from oracle.aid_oracle import linear, merge_heads, softmax_attention, split_heads


def mix_rows(x, rows, w):
    """[n, ...] = sum_m w[i, m] * x[rows[m]] for every weight row, summed in corner order (float64)."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    out = np.zeros((w.shape[0],) + x.shape[1:], np.float64)
    for m, r in enumerate(rows):
        out += w[:, m].reshape((-1,) + (1,) * (x.ndim - 1)) * x[r][None]
    return out


def _attend(qh, keys, vals, heads, scale, mask):
    """A(Q_i, [segments of keys], ...) of one frame: ``keys`` / ``vals`` lists of [L, C] segments, concatenated along the keys."""
    kh = split_heads(np.concatenate(keys, axis=0)[None], heads)
    vh = split_heads(np.concatenate(vals, axis=0)[None], heads)
    return merge_heads(softmax_attention(qh, kh, vh, scale, mask))[0]


def corners_core(q, k, v, heads, scale, mode, fused, w, rows, n_plain=0, kv_map=None, mask=None):
    """q [N, S, C], k / v [F, L, C] (v NOT transposed), w [N, M] (rows of the riders ignored), rows: M rows of k / v.
    ``kv_map``: frame -> its own row of k / v (None: identity).  ``mask``: additive score bias [N, H | 1, S | 1, L] (pure modes)."""
    q, k, v = (np.asarray(t, np.float64) for t in (q, k, v))
    w = np.asarray(w, np.float64)
    n = q.shape[0]
    out = np.zeros_like(q)
    for i in range(n):
        own = i if kv_map is None else int(kv_map[i])
        qh = split_heads(q[i:i + 1], heads)
        mk = None if mask is None else np.asarray(mask, np.float64)[i:i + 1]
        if i >= n - n_plain:
            out[i] = _attend(qh, [k[own]], [v[own]], heads, scale, mk)
            continue
        pre_k, pre_v = ([k[own]], [v[own]]) if fused else ([], [])
        if mode == "outer":
            for m, r in enumerate(rows):
                out[i] += w[i, m] * _attend(qh, pre_k + [k[r]], pre_v + [v[r]], heads, scale, mk)
        elif mode == "inner":
            kc = mix_rows(k, rows, w[i:i + 1])[0]
            vc = mix_rows(v, rows, w[i:i + 1])[0]
            out[i] = _attend(qh, pre_k + [kc], pre_v + [vc], heads, scale, mk)
        else:
            raise ValueError(mode)
    return out


def corners_processor(x, ctx, wq, wk, wv, wo, bo, heads, mode, fused, w, rows, n_plain=0, ctx_map=None, mask=None, residual=None):
    """to_out(corners_core(to_q(x), to_k(e), to_v(e))) (+ residual) with e = ctx (cross-attention; ``ctx_map`` frame -> context row)
    or x (self-attention), float64.  ``rows`` are rows of e's projections."""
    x = np.asarray(x, np.float64)
    e = x if ctx is None else np.asarray(ctx, np.float64)
    q, k, v = linear(x, np.asarray(wq, np.float64)), linear(e, np.asarray(wk, np.float64)), linear(e, np.asarray(wv, np.float64))
    d = q.shape[-1] // heads
    o = corners_core(q, k, v, heads, d ** -0.5, mode, fused, w, rows, n_plain, ctx_map, mask)
    y = linear(o, np.asarray(wo, np.float64), None if bo is None else np.asarray(bo, np.float64))
    return y if residual is None else y + np.asarray(residual, np.float64)
