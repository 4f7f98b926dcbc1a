"""Inputs with exactly known attention results for the ping-pong attention kernel (a plain module: the CPU test of the oracle,
tests/test_attn_pp_mfma16_layout.py, and the GPU test, tests/test_hip_attn_pp_mfma16.py, build the same tensors from it).

selection   K rows are +C / -C times one-hot codes (or zero rows), Q rows +C times one-hot codes: a row's score for its ONE target key is
            C * C = 1024, 0 for the zero rows and the other codes, -1024 for the opposite sign.  With softmax_scale = 1 / 8 the target
            leads by 128 (natural) = 184.7 (log2): every other weight is below 2^-184 of the target's — exp(-128) = 3e-56 in the fp64
            oracle; in the kernel 2^-184 times the largest P underflows the storage type (f16: below 2^-24; bf16, whose P sits 2^-59
            below one: 2^-243) AND fp32, so a tile that came first contributes exactly nothing after the reference moved.  V holds
            nonzero integers of magnitude <= 97 (exact in both storage types), distinct per key: the output IS V[target].
            128 codes serve two key tiles; with l = 192 the frame number rotates which tile holds the zero rows.
uniform     Q = 0: all scores 0, every weight 1 / l.  V[key, channel] = l where key % 64 == channel and key // 64 == the (frame, head)'s
            group, else 0: the output is l * (1 / l) = 1 in every channel if every key enters the product and the row sum exactly once
            (one key less in the sum: l / (l - 1) >= 1.0052, which rounds away from 1 in both storage types)."""
import numpy as np

C_SEL = 32.0
D = 64


def selection(l, heads, s=128):
    """-> q [F, s, heads * 64], k [F, l, heads * 64], v [F, l, heads * 64] (float64, exact in f16 / bf16), target [F, heads, s]."""
    nt = l // 64
    frames = nt if nt > 2 else 2
    q = np.zeros((frames, s, heads * D))
    k = np.zeros((frames, l, heads * D))
    v = np.zeros((frames, l, heads * D))
    target = np.zeros((frames, heads, s), np.int64)
    for f in range(frames):
        for h in range(heads):
            # the two coded tiles of this (frame, head); the third (l = 192) is zero rows
            coded = [(f + h + j) % nt for j in range(2)] if nt > 2 else [0, 1]
            for sign, tile in zip((1.0, -1.0), coded):
                for pos in range(64):
                    k[f, tile * 64 + pos, h * D + pos] = sign * C_SEL
            for r in range(s):
                t = (5 * r + 3 + 37 * (f + h)) % 128                 # 5 is prime to 128: s = 128 rows hit all 128 coded keys
                sign, tile = (1.0, coded[0]) if t < 64 else (-1.0, coded[1])
                q[f, r, h * D + t % 64] = sign * C_SEL
                target[f, h, r] = tile * 64 + t % 64
            for key in range(l):
                val = 1 + (key + 5 * np.arange(D)) % 97
                v[f, key, h * D:(h + 1) * D] = val if key < 97 else -val
    return q, k, v, target


def selection_expected(v, target, heads):
    frames, _, s = target.shape
    out = np.zeros((frames, s, heads * D))
    for f in range(frames):
        for h in range(heads):
            out[f, :, h * D:(h + 1) * D] = v[f, target[f, h], h * D:(h + 1) * D]
    return out


def uniform(l, heads, s=64):
    """-> q, k, v as in ``selection``; the expected output is 1.0 everywhere."""
    nt = l // 64
    frames = nt
    rng = np.random.default_rng(l)
    q = np.zeros((frames, s, heads * D))
    k = np.round(rng.standard_normal((frames, l, heads * D)) * 4) / 4     # any keys: the scores are 0
    v = np.zeros((frames, l, heads * D))
    for f in range(frames):
        for h in range(heads):
            g = (f + h) % nt
            for ch in range(D):
                v[f, 64 * g + ch, h * D + ch] = float(l)
    return q, k, v
