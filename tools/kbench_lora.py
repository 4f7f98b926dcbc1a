#!/usr/bin/env python3
"""Cost of unmerged LoRA adapters: one batched-CFG pass (7 cond + 7 uncond frames) through every attention layer
of the SD1.5 (fp16) and SDXL (bf16) stacks on the plain HIP processor, without LoRA, with adapters merged into the weights, and with
unmerged adapters of rank 8 / 64 / 128 on to_q / to_k / to_v / to_out of every layer.  Prints ms per pass (eager, CUDA events, the
cross-attention keys / values cached as in a run) and the per-kernel time of one pass from the library's profile entries.
A variant `dR` wraps the layers in DoRA adapters of rank R (tests/peft_dora_double.py): the same launches with a row gain on the
accumulators, plus one `aid_dora_gain` launch per projection when the packs are built — those are timed in the first call and
reported apart.  `--repeats N` runs every variant N times, interleaved, and prints min / median / max per variant.
    python tools/kbench_lora.py [--iters 10] [--variants none,merged,r8,r64,r128] [--repeats 1]
    python tools/kbench_lora.py --variants r64,d64 --repeats 3          # profiles/dora_kbench.txt"""
import argparse
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import aid_amd  # noqa: E402
from peft_double import wrap_attention  # noqa: E402
from peft_dora_double import wrap_attention_dora  # noqa: E402

DEV = torch.device("cuda:0")


def stack(model, dtype, variant):
    unet = aid_amd.AttnStackUNet(model, dtype=dtype, device=DEV)
    unet.set_attn_processor(aid_amd.HipAttnProcessor())
    if variant != "none":
        r = 64 if variant == "merged" else int(variant[1:])
        for i, m in enumerate(unet.layers):
            (wrap_attention_dora if variant[0] == "d" else wrap_attention)(m, {"a": (r, float(r))}, seed=i)
            if variant == "merged":
                for lin in (m.to_q, m.to_k, m.to_v, m.to_out[0]):
                    lin.merge()
    aid_amd.processors.clear_weight_caches()
    return unet


def inputs(unet, n, dtype):
    g = torch.Generator().manual_seed(0)
    xs = {(s, c): torch.randn(n, s, c, generator=g).to(dtype).to(DEV) for (s, c) in unet.level_shapes()}
    ctx = torch.randn(n, unet.text_len, unet.cross_dim, generator=g).to(dtype).to(DEV)
    return xs, ctx


def profiled(lib, fn):
    """{kernel: [launches, ms]} of one call of ``fn`` from the library's profile entries."""
    lib.aid_profile_begin()
    fn()
    buf = (aid_amd._lib.AidProfileEntry * 8192)()
    n = lib.aid_profile_end(buf, 8192)
    per = collections.defaultdict(lambda: [0, 0.0])
    for e in buf[:n]:
        k = e.kernel.decode().split("<")[0]
        per[k][0] += 1
        per[k][1] += e.ms
    return per


def run(model, dtype, variant, iters):
    lib = aid_amd._lib.load()
    with torch.no_grad():
        unet = stack(model, dtype, variant)
        xs, ctx = inputs(unet, 14, dtype)
        first = profiled(lib, lambda: unet(xs, ctx))        # builds the adapter packs (DoRA: the gain launches)
        for _ in range(3):
            unet(xs, ctx)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            unet(xs, ctx)
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / iters
        per = profiled(lib, lambda: unet(xs, ctx))
    if "aid_dora_gain" in first:
        per["aid_dora_gain (first call, once per pack)"] = first["aid_dora_gain"]
    del unet
    torch.cuda.empty_cache()
    return ms, per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--variants", default="none,merged,r8,r64,r128")
    ap.add_argument("--repeats", type=int, default=1)
    args = ap.parse_args()
    variants = args.variants.split(",")
    for model, dtype in (("sd15", torch.float16), ("sdxl", torch.bfloat16)):
        base = None
        times = collections.defaultdict(list)
        for rep in range(args.repeats):
            for variant in variants:
                ms, per = run(model, dtype, variant, args.iters)
                base = ms if base is None else base
                times[variant].append(ms)
                print(f"{model} {str(dtype)[6:]:8s} lora={variant:6s} pass {ms:8.3f} ms  x{ms / base:5.3f}")
                if rep == 0:
                    for k, (cnt, t) in sorted(per.items(), key=lambda kv: -kv[1][1]):
                        print(f"    {k:44s} {cnt:5d} launches {t:8.3f} ms")
                sys.stdout.flush()
        if args.repeats > 1:
            for variant in variants:
                t = sorted(times[variant])
                print(f"{model} {str(dtype)[6:]:8s} lora={variant:6s} min {t[0]:8.3f}  median {t[len(t) // 2]:8.3f}  max {t[-1]:8.3f} ms"
                      f"  spread {t[-1] - t[0]:6.3f} ms over {len(t)} repeats")


if __name__ == "__main__":
    main()
