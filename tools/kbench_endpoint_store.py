#!/usr/bin/env python3
"""End-point K / V^T store: what replaying recorded end points saves, on the full-size stand-in stacks.

Per stack — SD1.5 fp16 and SDXL bf16 (`StackDenoiser(scale_down=1)`: every attention layer of the UNet at its real S, C, heads) —
alternating, `--repeats` times, wall time of a whole pipeline run (graphs on, synchronised at both ends) divided by its steps:
  * `interpolate_single(0.3)`: the full batch of 3, the RECORDING run (its overhead over the plain run), the replay with a batch of 1;
  * `interpolate(size=7)`: the full run against a replay of its 5 interior frames from the same store.
Reported: the median of the repeats and their spread (min .. max).  Then the copy kernel alone (`aid_endpoint_rows`, PUT and GET) at
the two SDXL block sizes: median of `--samples` device-event pairs, achieved GB/s counting every byte read and written.

usage (on the GPU):  python tools/kbench_endpoint_store.py [--steps 8] [--repeats 3] [--out profiles/endpoint_store.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import aid_amd  # noqa: E402
from aid_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
STACKS = [("sd15", torch.float16), ("sdxl", torch.bfloat16)]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def med(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def setup(model, dtype):
    hip = aid_amd.StackDenoiser(model, dtype=dtype, device=dev, scale_down=1, latent_hw=(16, 16))
    cls = aid_amd.InterpolationStableDiffusionXLPipeline if model == "sdxl" else aid_amd.InterpolationStableDiffusionPipeline
    pipe = cls(hip, aid_amd.DDIMSchedulerLite())
    pipe.load_aid(t=0.5, is_fused=True, atype="fused_outer")
    g = torch.Generator().manual_seed(0)
    l0, l1 = torch.randn(1, 4, 16, 16, generator=g), torch.randn(1, 4, 16, 16, generator=g)

    def emb():
        e = (torch.randn(1, 77, hip.stack.cross_dim, generator=g), torch.randn(1, 77, hip.stack.cross_dim, generator=g))
        return e + ((torch.randn(1, 32, generator=g), torch.randn(1, 32, generator=g)) if model == "sdxl" else ())
    return pipe, l0, l1, emb(), emb()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "endpoint_store.txt"))
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"end-point store: ms per step, {args.steps} steps (warm-up ratio 0.5: {args.steps // 2} AID steps), graphs on, fused_outer; "
        f"median of {args.repeats} alternating repeats [min .. max]")
    ctx = {m: setup(m, dt) for m, dt in STACKS}
    t = {m: {k: [] for k in ("single_full", "single_record", "single_replay", "n7_full", "n5_replay")} for m, _ in STACKS}
    nbytes = {}
    for rep in range(args.repeats + 1):                    # repeat 0 warms up (lazy kernel attributes, allocator) and is dropped
        for model, dtype in STACKS:
            pipe, l0, l1, es, ee = ctx[model]
            kw = dict(latent_start=l0, latent_end=l1, embeds_start=es, embeds_end=ee, num_inference_steps=args.steps, warmup_ratio=0.5,
                      output_type="latent")
            nkw = dict(embeds_start=es, embeds_end=ee, num_inference_steps=args.steps, warmup_ratio=0.5, early="fused_outer",
                       output_type="latent")
            store = aid_amd.EndpointStore()
            r = {"single_full": timed(lambda: pipe.interpolate_single(0.3, **kw)),
                 "single_record": timed(lambda: pipe.interpolate_single(0.5, endpoints=store, **kw)),
                 "single_replay": timed(lambda: pipe.interpolate_single(0.3, endpoints=store, **kw)),
                 "n7_full": timed(lambda: pipe.interpolate(l0, l1, size=7, **nkw)),
                 "n5_replay": timed(lambda: pipe.interpolate(l0, l1, size=7, endpoints=store, **nkw))}
            nbytes[model] = store.nbytes
            del store
            if rep:
                for k, v in r.items():
                    t[model][k].append(v / args.steps)
    for model, dtype in STACKS:
        say(f"\n{model} {str(dtype)[6:]}: store of {args.steps // 2} AID steps = {nbytes[model] / 2 ** 30:.2f} GiB "
            f"({nbytes[model] / (args.steps // 2) / 2 ** 30:.2f} GiB per AID step)")
        for k, what in (("single_full", "interpolate_single, full batch 3"), ("single_record", "  the same, recording"),
                        ("single_replay", "  replay, batch 1"), ("n7_full", "interpolate(size=7), full"),
                        ("n5_replay", "  replay of its 5 interior frames")):
            m_, lo, hi = med(t[model][k])
            say(f"  {what:36s} {m_:9.2f} ms / step  [{lo:9.2f} .. {hi:9.2f}]")
        (f, flo, fhi), (r_, rlo, rhi), (c, _, _) = med(t[model]["single_full"]), med(t[model]["single_replay"]), med(t[model]["single_record"])
        say(f"  batch 3 / batch 1: x{f / r_:.2f}; spreads {'overlap' if rhi >= flo else 'do not overlap'}; "
            f"record overhead {100 * (c / f - 1):+.1f} % of the plain run")
        (f, flo, fhi), (r_, rlo, rhi) = med(t[model]["n7_full"]), med(t[model]["n5_replay"])
        say(f"  7 frames / 5 frames: x{f / r_:.2f}; spreads {'overlap' if rhi >= flo else 'do not overlap'}")

    say(f"\ncopy kernel aid_endpoint_rows, bf16, median of {args.samples} launches; bytes = 2 x 2 x (k_fs + vt_fs) x 2 (read + written)")
    for s, c in ((4096, 640), (1024, 1280)):
        k_fs, vt_fs = ops.endpoint_block_sizes(s, c)
        k = torch.randn(3, s, c, device=dev).to(torch.bfloat16)
        vt = torch.randn(3, c, vt_fs // c, device=dev).to(torch.bfloat16)
        ks, vs = torch.empty(4, 2, k_fs, dtype=torch.bfloat16, device=dev), torch.empty(4, 2, vt_fs, dtype=torch.bfloat16, device=dev)
        step = torch.zeros(1, dtype=torch.int32, device=dev)
        for direction in ("put", "get"):
            us = []
            for i in range(args.samples + 5):
                step.fill_(i % 4)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ops.endpoint_rows(k, vt, ks, vs, step, direction, 0, 2)
                e1.record()
                e1.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3)
            m_, lo, hi = med(us[5:])
            say(f"  S={s:4d} C={c:4d} {direction}: {m_:7.1f} us [{lo:7.1f} .. {hi:7.1f}]   {2 * 2 * (k_fs + vt_fs) * 2 / m_ / 1e3:7.1f} GB/s")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
