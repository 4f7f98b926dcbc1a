#!/usr/bin/env python3
"""Key-frame store in 8-bit blocks: the copy launch alone, native (`aid_keyframe_rows`) against q8
(`aid_keyframe_rows_q8`), PUT and GET, at the two SDXL block sizes of tools/kbench_endpoint_store.py (bf16, S = 4096 / C = 640 and
S = 1024 / C = 1280), two rows per launch (what a replay's GET moves).

The four launches alternate in ONE process, sample by sample (native put, q8 put, native get, q8 get, ...), each between a pair of
device events; reported per launch: the median of `--samples` samples, the quartiles, and the achieved GB/s counting every byte read
and written.  Two figures are "apart" when their quartile ranges do not overlap.

usage (on the GPU, the one step under a time limit of its own):
    timeout -k 10 300 python tools/kbench_keyframe_q8.py [--samples 50] [--out profiles/keyframe_q8.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from aid_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
N_ROWS, N_STEPS, WARM = 2, 4, 5


def quartiles(v):
    v = sorted(v)
    n = len(v)
    return v[n // 2], v[n // 4], v[(3 * n) // 4]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyframe_q8.txt"))
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"key-frame copy launch, bf16, {N_ROWS} rows per launch, native vs q8, alternating in one process; median of {args.samples} "
        f"event-timed launches [lower quartile .. upper quartile]; GB/s over every byte read and written")
    for s, c in ((4096, 640), (1024, 1280)):
        k_fs, vt_fs = ops.endpoint_block_sizes(s, c)
        k = torch.randn(3, s, c, device=dev).to(torch.bfloat16)
        vt = torch.randn(3, c, vt_fs // c, device=dev).to(torch.bfloat16)
        native = [(torch.empty(N_STEPS, k_fs, dtype=torch.bfloat16, device=dev), torch.empty(N_STEPS, vt_fs, dtype=torch.bfloat16, device=dev), r)
                  for r in range(N_ROWS)]
        q8 = [(torch.zeros(N_STEPS, ops.q8_block_bytes(k_fs), dtype=torch.uint8, device=dev),
               torch.zeros(N_STEPS, ops.q8_block_bytes(vt_fs), dtype=torch.uint8, device=dev), r) for r in range(N_ROWS)]
        step = torch.zeros(1, dtype=torch.int32, device=dev)
        call_bytes = N_ROWS * (k_fs + vt_fs) * 2
        q8_bytes = N_ROWS * (k_fs + (k_fs + 31) // 32 + vt_fs + (vt_fs + 31) // 32)
        launches = {
            ("native", "put"): (lambda: ops.keyframe_rows(k, vt, native, step, "put"), 2 * call_bytes),
            ("q8", "put"): (lambda: ops.keyframe_rows_q8(k, vt, q8, step, "put", vt_cols=s), call_bytes + q8_bytes),
            ("native", "get"): (lambda: ops.keyframe_rows(k, vt, native, step, "get"), 2 * call_bytes),
            ("q8", "get"): (lambda: ops.keyframe_rows_q8(k, vt, q8, step, "get", vt_cols=s), call_bytes + q8_bytes),
        }
        for i in range(N_STEPS):                              # every slot holds finite data before a GET reads it
            step.fill_(i)
            launches[("native", "put")][0]()
            launches[("q8", "put")][0]()
        us = {key: [] for key in launches}
        for i in range(args.samples + WARM):
            step.fill_(i % N_STEPS)
            for key, (fn, _) in launches.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if i >= WARM:
                    us[key].append(e0.elapsed_time(e1) * 1e3)
        say(f"\nS={s} C={c}: block {k_fs} + {vt_fs} elements; per launch native {2 * call_bytes / 2 ** 20:.1f} MiB, "
            f"q8 {(call_bytes + q8_bytes) / 2 ** 20:.1f} MiB moved")
        q = {key: quartiles(v) for key, v in us.items()}
        for key, (_, nbytes) in launches.items():
            m_, lo, hi = q[key]
            say(f"  {key[0]:6s} {key[1]}: {m_:7.1f} us [{lo:7.1f} .. {hi:7.1f}]   {nbytes / m_ / 1e3:7.1f} GB/s")
        for direction in ("put", "get"):
            (n_, nlo, nhi), (q_, qlo, qhi) = q[("native", direction)], q[("q8", direction)]
            apart = qhi < nlo or nhi < qlo
            say(f"  {direction}: q8 / native = x{q_ / n_:.2f}; quartile ranges {'are apart' if apart else 'overlap'}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
