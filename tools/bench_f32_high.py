#!/usr/bin/env python3
"""bench.py under torch.set_float32_matmul_precision("high") (single GPU): sets the global, then runs bench.py unchanged with the
arguments given here, e.g.
    python tools/bench_f32_high.py --workload sd15 --dtype f32 --frames 3 --steps 20
Float32 projections then run the three-term bf16 split (csrc/aid_f32x3.hip); 16-bit workloads are not affected."""
import os
import runpy
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    torch.set_float32_matmul_precision(os.environ.get("AID_F32_PRECISION", "high"))
    sys.argv[0] = os.path.join(ROOT, "bench.py")
    sys.path.insert(0, ROOT)
    runpy.run_path(sys.argv[0], run_name="__main__")
