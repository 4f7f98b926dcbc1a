#!/usr/bin/env python3
"""bench.py with the float32 precision switches set (single GPU): sets the torch global (the projections) and the package's
attention-core setting, then runs bench.py unchanged with the arguments given here, e.g.
    AID_F32_PRECISION=highest AID_F32_ATTN_PRECISION=highest python tools/bench_f32_attn_high.py --workload sd15 --dtype f32 --frames 3 --steps 20
    AID_F32_PRECISION=high    AID_F32_ATTN_PRECISION=highest ...        (projections split: what tools/bench_f32_high.py runs)
    AID_F32_PRECISION=high    AID_F32_ATTN_PRECISION=high    ...        (projections + attention core split; the default here)
16-bit workloads are not affected by either."""
import os
import runpy
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import aid_amd
    torch.set_float32_matmul_precision(os.environ.get("AID_F32_PRECISION", "high"))
    aid_amd.set_f32_attn_precision(os.environ.get("AID_F32_ATTN_PRECISION", "high"))
    sys.argv[0] = os.path.join(ROOT, "bench.py")
    runpy.run_path(sys.argv[0], run_name="__main__")
