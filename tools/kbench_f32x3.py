#!/usr/bin/env python3
"""float32 projections: the three-term bf16 split (aid_gemm_f32x3_kernel, f32_precision="high") against the exact kernel
(aid_gemm_f32_kernel) on the same operands, alternating, three repeats with their spread.

Shapes: the SD1.5 stack at batch 3 (m = 3 S, C = 320 / 640 / 1280 / 1280: the out projection x Wo^T and the grouped q / k / V^T launch
as aid_processor_fwd issues it), the Cc = 768 text projections (k and batched V^T of 3 x 77 tokens), and two SDXL projections.
Prints us and TFLOP/s (2 m n k) per launch; `verdict` = split faster than exact by more than the repeats' spread.
The last row is a launch with a rank-64 low-rank segment (m 3072, n 640, k 640, bias + residual, as tests/test_hip_lora.py builds it):
such a group runs the exact kernel under either setting, so both columns time aid_gemm_f32_kernel_lr."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import aid_amd  # noqa: E402
from aid_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
lib = aid_amd._lib.load()


def timed(fn, iters):
    fn(); fn(); torch.cuda.synchronize(); lib.aid_profile_begin()
    for _ in range(iters):
        fn()
    buf = (aid_amd._lib.AidProfileEntry * 512)()
    n = lib.aid_profile_end(buf, 512)
    return sum(e.ms for e in buf[:n]) / n * 1e3, sum(e.flops for e in buf[:n]) / n, buf[0].kernel.decode()


def ab(tag, problems):
    """problems(prec) -> list of gemm_nt problems"""
    res = {"highest": [], "high": []}
    names = {}
    for _ in range(3):
        for prec in ("highest", "high"):
            ps = problems(prec)
            us, fl, nm = timed(lambda: ops.gemm_nt(ps), 20)
            res[prec].append(us)
            names[prec] = nm
    e, s = res["highest"], res["high"]
    med = lambda v: sorted(v)[1]                                     # noqa: E731
    spread = max(max(e) - min(e), max(s) - min(s))
    verdict = "split" if med(e) - med(s) > spread else "exact"
    print(f"{tag:34s} exact {med(e):8.1f} us [{min(e):.1f} .. {max(e):.1f}] {fl / med(e) / 1e6:6.1f} TF/s | "
          f"split {med(s):8.1f} us [{min(s):.1f} .. {max(s):.1f}] {fl / med(s) / 1e6:6.1f} TF/s | x{med(e) / med(s):5.2f} -> {verdict}"
          f"   ({names['highest']} / {names['high']})", flush=True)


def main():
    g = torch.Generator(device="cpu").manual_seed(0)
    rn = lambda *sh: torch.randn(*sh, generator=g).to(dev)          # noqa: E731
    for tag, n, s, c in (("sd15 L0", 3, 4096, 320), ("sd15 L1", 3, 1024, 640), ("sd15 L2", 3, 256, 1280), ("sd15 mid", 3, 64, 1280),
                         ("sdxl 14336x1280", 14, 1024, 1280), ("sdxl 28672x640", 7, 4096, 640)):
        m = n * s
        x, wq, wk, wv, wo, bo = rn(n, s, c), rn(c, c), rn(c, c), rn(c, c), rn(c, c), rn(c)
        q, k, y = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        vt = torch.empty(n, c, s, device=dev)
        ab(f"{tag} out  m={m} C={c}", lambda prec: [dict(a=x, b=wo, c=y, bias=bo, m=m, n=c, k=c, lda=c, ldb=c, ldc=c, f32_precision=prec)])
        if tag.startswith("sd15"):
            ab(f"{tag} qkv  m={m} C={c}", lambda prec: [
                dict(a=x, b=wq, c=q, m=m, n=c, k=c, lda=c, ldb=c, ldc=c, f32_precision=prec),
                dict(a=x, b=wk, c=k, m=m, n=c, k=c, lda=c, ldb=c, ldc=c, f32_precision=prec),
                dict(a=x, b=wv, c=vt, m=m, n=c, k=c, lda=c, ldb=c, ldc=s, stride_c=c * s, trans_rows=s, f32_precision=prec)])
    l, lp, cc, nctx = 77, 80, 768, 3
    for c in (320, 640, 1280):
        e, wk, wv = rn(nctx, l, cc), rn(c, cc), rn(c, cc)
        k, vt = torch.empty(nctx, l, c, device=dev), torch.empty(nctx, c, lp, device=dev)
        ab(f"text k+vt 3x77 Cc=768 C={c}", lambda prec: [
            dict(a=e, b=wk, c=k, m=nctx * l, n=c, k=cc, lda=cc, ldb=cc, ldc=c, f32_precision=prec),
            dict(a=wv, b=e, c=vt, m=c, n=l, k=cc, lda=cc, ldb=cc, ldc=lp, batch=nctx, stride_a=0, stride_b=l * cc, stride_c=c * lp,
                 f32_precision=prec)])
    m, n, k, r = 3072, 640, 640, 64
    x, w, bias, res, y = rn(m, k), rn(n, k), rn(n), rn(m, n), torch.empty(m, n, device=dev)
    u, bp = rn(m, r + 64), rn(n, r + 8)                              # padded rows: lr_lda / lr_ldb > lr_k
    ab(f"low-rank r={r} m={m} n={n} k={k}", lambda prec: [
        dict(a=x, b=w, c=y, bias=bias, residual=res, m=m, n=n, k=k, lda=k, ldb=k, ldc=n, f32_precision=prec,
             lr=dict(a=u, b=bp, k=r, lda=r + 64, ldb=r + 8))])


if __name__ == "__main__":
    main()
