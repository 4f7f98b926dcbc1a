"""fp64 reference of a key-frame blend call (aid_processor_kf_blend_fwd) — a plain module, imported by the blend tests.

The call runs over the LOCAL frames; its corners are the recorded K / V of M key frames.  The reference is corners_ref.corners_core over
the local frames' own projections with the corners' recorded K / V appended as rows n .. n + M - 1 — the oracle's ``linear`` for every
projection, nothing of the library."""
import numpy as np

from corners_ref import corners_core
from oracle.aid_oracle import linear


def blend_processor(x, k_rec, v_rec, wq, wk, wv, wo, bo, heads, mode, fused, w, n_plain=0, mask=None, residual=None):
    """x [N, S, C] local frames (the last ``n_plain`` are riders), k_rec / v_rec [M, S, C] the key frames' recorded keys / values (v NOT
    transposed), w [N, M] (rows of the riders ignored).  Returns to_out(attention) (+ residual), float64."""
    x = np.asarray(x, np.float64)
    k_rec, v_rec = np.asarray(k_rec, np.float64), np.asarray(v_rec, np.float64)
    n, m = x.shape[0], k_rec.shape[0]
    q = linear(x, np.asarray(wq, np.float64))
    k = np.concatenate([linear(x, np.asarray(wk, np.float64)), k_rec])
    v = np.concatenate([linear(x, np.asarray(wv, np.float64)), v_rec])
    d = q.shape[-1] // heads
    o = corners_core(q, k, v, heads, d ** -0.5, mode, fused, w, [n + i for i in range(m)], n_plain, list(range(n)), mask)
    y = linear(o, np.asarray(wo, np.float64), None if bo is None else np.asarray(bo, np.float64))
    return y if residual is None else y + np.asarray(residual, np.float64)
