#!/usr/bin/env python3
"""Adding G unmasked IP-Adapter image branches to an attention output: G launches of aid_attn_fwd(accumulate = 1, out_scale) — the only
way before aid_ip_attn_fwd, a pass over q and out per adapter — against ONE launch of aid_ip_attn_fwd on identical q / K / V^T.

Shapes: SDXL IP (8 frames, bf16: S = 4096 / C = 640 / 10 heads, S = 1024 / C = 1280 / 20 heads) and SD1.5 level 0 (fp16, S = 4096,
C = 320, 8 heads), adapters of 4 + 16 image tokens.  Same process, the two forms alternating; each sample is a device-event pair
around one whole addition (G launches / 1 launch); the figure is the median of `--samples` samples per form after a warm-up, with
the quartiles beside it.  Also prints the largest difference between the two results on the same inputs (one rounding instead of G)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import aid_amd  # noqa: E402,F401
from aid_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
SHAPES = [("sdxl", torch.bfloat16, 8, 4096, 640, 10), ("sdxl", torch.bfloat16, 8, 1024, 1280, 20), ("sd15", torch.float16, 8, 4096, 320, 8)]
TOKENS, SCALES = (4, 16), (0.6, 0.4)


def sample(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def quart(v):
    v = sorted(v)
    return v[len(v) // 2], v[len(v) // 4], v[3 * len(v) // 4]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=60)
    args = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    print(f"{'shape':44s} {'G x aid_attn_fwd(accumulate)':>30s} {'1 x aid_ip_attn_fwd':>30s}   ratio   max |diff|")
    for tag, dtype, n, s, c, heads in SHAPES:
        q = torch.randn(n, s, c, generator=g).to(dtype).to(dev)
        base = (0.3 * torch.randn(n, s, c, generator=g)).to(dtype).to(dev)
        kv = []
        for t in TOKENS:
            k = torch.randn(n, t, c, generator=g).to(dtype).to(dev)
            vt = torch.zeros(n, c, (t + 7) // 8 * 8, dtype=dtype, device=dev)
            vt[:, :, :t] = torch.randn(n, c, t, generator=g).to(dtype).to(dev)
            kv.append((k, vt, t))
        segs = [dict(k=k, vt=vt, scale=sc) for (k, vt, t), sc in zip(kv, SCALES)]

        def old(out):
            for (k, vt, t), sc in zip(kv, SCALES):
                ops.attn_fwd(q, k, vt, heads, l=t, out=out, accumulate=True, out_scale=sc)

        def new(out):
            ops.ip_attn_accumulate(q, out, segs, heads)

        o_old, o_new = base.clone(), base.clone()
        old(o_old)
        new(o_new)
        torch.cuda.synchronize()
        diff = float((o_old.float() - o_new.float()).abs().max())
        out = base.clone()
        for _ in range(10):                                            # warm-up of both forms at this shape
            old(out)
            new(out)
        torch.cuda.synchronize()
        t_old, t_new = [], []
        for _ in range(args.samples):
            out.copy_(base)
            t_old.append(sample(lambda: old(out)))
            out.copy_(base)
            t_new.append(sample(lambda: new(out)))
        (mo, lo, ho), (mn, ln, hn) = quart(t_old), quart(t_new)
        print(f"{tag} {str(dtype)[6:]:8s} N={n} S={s:4d} C={c:4d} H={heads:2d} T={'+'.join(map(str, TOKENS))}   "
              f"{mo:8.1f} us [{lo:7.1f} .. {ho:7.1f}]   {mn:8.1f} us [{ln:7.1f} .. {hn:7.1f}]   x{mo / mn:5.2f}   {diff:.3e}", flush=True)


if __name__ == "__main__":
    main()
