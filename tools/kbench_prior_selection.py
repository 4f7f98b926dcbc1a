#!/usr/bin/env python3
"""bayesian_prior_selection: what one selection costs, on the full-size SD1.5 stand-in stack.

`StackDenoiser("sd15", fp16, scale_down=1)`: every attention layer of the UNet at its real S, C, heads.  One selection = the
`interpolate_single(0.5)` run, the nine probes and `--n-iter` proposals of the default optimiser, `target_score` out of reach so that
every evaluation runs; 25 steps, warm-up ratio 1 (the function's defaults), graphs on, latent frames scored by a fixed linear map and
the cosine distance.  Three evaluation structures, in the same process, alternating, `--repeats` times after one dropped warm-up round:
  * full          `reuse_endpoints=False`: every evaluation a full `size`-frame run (the reference's structure in ONE run per evaluation);
  * replay        `reuse_endpoints=True, batch_probes=False`: every evaluation replays its `size - 2` interior frames;
  * replay+batch  `batch_probes=True` as well: the probes that need rendering share one replay run.
Reported per `size`: wall time of the whole selection (device synchronised before the clock stops), median of the repeats and their
spread (min .. max), the number of evaluations rendered, and the ratios to `full`.

usage (on the GPU):  python tools/kbench_prior_selection.py [--sizes 3 7] [--steps 25] [--n-iter 15] [--repeats 5]
                                                            [--out profiles/prior_selection.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import aid_amd  # noqa: E402
from aid_amd.prior import clip_distance  # noqa: E402

dev = torch.device("cuda:0")
VARIANTS = (("full", dict(reuse_endpoints=False, batch_probes=False)),
            ("replay", dict(reuse_endpoints=True, batch_probes=False)),
            ("replay+batch", dict(reuse_endpoints=True, batch_probes=True)))


def med(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[3, 7])
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--n-iter", type=int, default=15)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prior_selection.txt"))
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    hip = aid_amd.StackDenoiser("sd15", dtype=torch.float16, device=dev, scale_down=1, latent_hw=(16, 16))
    pipe = aid_amd.InterpolationStableDiffusionPipeline(hip, aid_amd.DDIMSchedulerLite())
    pipe.load_aid(t=0.5, is_fused=True, atype="fused_outer")
    g = torch.Generator().manual_seed(0)
    l0, l1 = torch.randn(1, 4, 16, 16, generator=g), torch.randn(1, 4, 16, 16, generator=g)
    es = (torch.randn(1, 77, hip.stack.cross_dim, generator=g), torch.randn(1, 77, hip.stack.cross_dim, generator=g))
    ee = (torch.randn(1, 77, hip.stack.cross_dim, generator=g), torch.randn(1, 77, hip.stack.cross_dim, generator=g))
    w = torch.randn(4 * 16 * 16, 24, generator=g).to(dev)

    def distance(a, b):
        return clip_distance(a.reshape(1, -1).float() @ w, b.reshape(1, -1).float() @ w)

    def select(size, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        (alpha, beta), trace = aid_amd.bayesian_prior_selection(
            pipe, l0, l1, None, None, None, size=size, num_inference_steps=args.steps, target_score=2.0, n_iter=args.n_iter,
            distance=distance, return_trace=True, embeds_start=es, embeds_end=ee, output_type="latent", **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, sum(1 for e in trace if e[3]), len(trace), (alpha, beta)

    say(f"bayesian_prior_selection on the full-size SD1.5 stack, fp16: seconds per selection ({args.steps} steps, warm-up ratio 1, "
        f"9 probes + {args.n_iter} proposals, target out of reach, graphs on, fused_outer); median of {args.repeats} alternating "
        f"repeats [min .. max]")
    for size in args.sizes:
        t = {name: [] for name, _ in VARIANTS}
        info = {}
        for rep in range(args.repeats + 1):                # repeat 0 warms up (lazy kernel attributes, allocator) and is dropped
            for name, kw in VARIANTS:
                sec, rendered, evaluated, picked = select(size, **kw)
                info[name] = (rendered, evaluated, picked)
                if rep:
                    t[name].append(sec)
        say(f"\nsize = {size}: frames through the UNet per rendered evaluation (conditional; each with its CFG rider): "
            f"full {size}, replay {size - 2}")
        base = med(t["full"])
        for name, _ in VARIANTS:
            m_, lo, hi = med(t[name])
            rendered, evaluated, picked = info[name]
            say(f"  {name:13s} {m_:8.3f} s  [{lo:8.3f} .. {hi:8.3f}]   {rendered:2d} of {evaluated} evaluations rendered, picked "
                f"({picked[0]:.2f}, {picked[1]:.2f})   full / this: x{base[0] / m_:.2f}"
                + ("" if name == "full" else f"; spreads {'overlap' if hi >= base[1] else 'do not overlap'}"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
