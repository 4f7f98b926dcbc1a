#!/usr/bin/env python3
"""Classifier-free guidance with guidance rescale: the one launch (`ops.cfg_rescale`) against the eager torch chain
it replaces — the combine, two per-sample `std` reductions and the rescale / mix, as the reference's loop runs them
(pipeline_interpolated_sd.py:92-108, 1892-1902) — on the two halves of one batched-CFG output `[2 n, 4, h, w]`:
7 x 4 64 64 float16 (SD1.5 latents) and 7 x 4 128 128 bfloat16 (SDXL latents).

The two alternate in ONE process, sample by sample, each between a pair of device events (so a sample covers the launches AND the gaps
between them: the chain is two reductions and about six elementwise launches); reported: the median of `--samples` samples and the quartiles.  Two figures are "apart"
when their quartile ranges do not overlap; otherwise nothing is claimed.

usage (on the GPU, the one step under a time limit of its own):
    timeout -k 10 300 python tools/kbench_cfg_rescale.py [--samples 50] [--out profiles/cfg_rescale.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from aid_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
GS, PHI, WARM = 7.5, 0.7, 10


def eager(text, uncond):
    """The chain in torch, every step in the storage dtype."""
    c = uncond + GS * (text - uncond)
    dims = list(range(1, text.ndim))
    std_text = text.std(dim=dims, keepdim=True)
    std_c = c.std(dim=dims, keepdim=True)
    return PHI * (c * (std_text / std_c)) + (1 - PHI) * c


def quartiles(v):
    v = sorted(v)
    n = len(v)
    return v[n // 2], v[n // 4], v[(3 * n) // 4]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cfg_rescale.txt"))
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"guidance + rescale (gs {GS}, rescale {PHI}) on the halves of one [2 n, 4, h, w] tensor: one launch (aid_cfg_rescale) vs the "
        f"eager torch chain, alternating in one process; median of {args.samples} event-timed samples [lower quartile .. upper quartile]")
    for n, hw, dtype in ((7, 64, torch.float16), (7, 128, torch.bfloat16)):
        both = torch.randn(2 * n, 4, hw, hw, device=dev).to(dtype)
        text, uncond = both[:n], both[n:]
        calls = {"aid_cfg_rescale": lambda: ops.cfg_rescale(text, uncond, GS, PHI), "torch chain": lambda: eager(text, uncond)}
        us = {k: [] for k in calls}
        for i in range(args.samples + WARM):
            for key, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if i >= WARM:
                    us[key].append(e0.elapsed_time(e1) * 1e3)
        a, b = calls["aid_cfg_rescale"]().float(), calls["torch chain"]().float()
        diff = float((a - b).norm() / b.norm())
        say(f"\n{n} x 4 {hw} {hw} {str(dtype).split('.')[-1]} ({n * 4 * hw * hw * both.element_size() // 1024} KB per operand); "
            f"rel-L2 between the two results {diff:.1e}")
        q = {k: quartiles(v) for k, v in us.items()}
        for key in calls:
            m_, lo, hi = q[key]
            say(f"  {key:16s}: {m_:7.1f} us [{lo:7.1f} .. {hi:7.1f}]")
        (k_, klo, khi), (t_, tlo, thi) = q["aid_cfg_rescale"], q["torch chain"]
        apart = khi < tlo or thi < klo
        say(f"  quartile ranges {'are apart' if apart else 'overlap: no claim'}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
