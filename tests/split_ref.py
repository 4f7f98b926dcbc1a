"""CPU restatement of the three-term bf16 split of a float32 GEMM (AidGemmProblem.f32_split = 1, csrc/aid_f32x3.hip); a plain
module, imported by tests/test_f32_precision.py and tests/test_hip_f32x3.py.

    hi = bf16_rne(x),  lo = bf16_rne(x - float(hi))         (torch's float32 -> bfloat16 conversion rounds to nearest even)
    ref3  = hi hi^T + lo hi^T + hi lo^T                     what the split kernel computes, summed in fp64: only the split error
    ref1  = hi hi^T                                         one bf16 product: what a kernel that lost its low halves computes
    ref64 = the fp64 product of the float32 inputs
"""
import numpy as np
import torch


def split(x: torch.Tensor):
    """(hi, lo) of a float32 tensor as float64 numpy arrays."""
    x = x.detach().float().cpu()
    hi = x.bfloat16().float()
    lo = (x - hi).bfloat16().float()
    return hi.numpy().astype(np.float64), lo.numpy().astype(np.float64)


def refs(a: torch.Tensor, b: torch.Tensor):
    """(ref3, ref1, ref64) of a b^T for float32 a [.., m, k], b [.., n, k] (leading batch dimensions broadcast)."""
    ah, al = split(a)
    bh, bl = split(b)
    t = lambda z: np.swapaxes(z, -1, -2)      # noqa: E731
    ref1 = ah @ t(bh)
    ref3 = ref1 + al @ t(bh) + ah @ t(bl)
    a64, b64 = a.detach().cpu().numpy().astype(np.float64), b.detach().cpu().numpy().astype(np.float64)
    return ref3, ref1, a64 @ t(b64)
