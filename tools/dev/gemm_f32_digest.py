#!/usr/bin/env python3
"""Development: sha256 of the output buffer of float32 GEMM launches, one line per case — run it on two builds of the library
(AID_LIB_PATH=<other build>/libaid_hip.so for one of them, a fresh process each) and compare the listings: a change that is not meant
to touch the arithmetic of aid_gemm_f32_kernel / aid_gemm_f32x3_kernel leaves every digest as it was.  The buffer is hashed whole:
pad columns, and the NaN-filled rows and columns around C that no launch may write.

Cases (seeded operands): a - e reach each epilogue path — a (130, 132, 72) bias + residual: 16-byte stores; b (257, 70, 328) scale +
bias + residual, ldc 72: scalar stores, zeroed pad columns; c batch 3 of (130, 70, 72), padded strides, residual; d (48, 70, 40)
transposed per frame of 16 rows; e (4096, 2048, 64) bare: 512 tiles of 128 x 128, the big-tile rule — under "highest" and "high";
under "highest" only: a folded LayerNorm on side 1 and on side 2 batched with stride_stats, a rank-64 low-rank segment without gain,
with a gain on side 2, and batched with a gain on side 1.
usage:  python tools/dev/gemm_f32_digest.py"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from aid_amd import ops  # noqa: E402

DEV = torch.device("cuda:0")


def cases():
    """(name, precisions, problem without c, shape of the C buffer)"""
    g = torch.Generator().manual_seed(0)
    rn = lambda *sh: torch.randn(*sh, generator=g).to(DEV)          # noqa: E731
    out = []
    m, n, k = 130, 132, 72
    out.append(("a vec", ("highest", "high"), dict(a=rn(m, k), b=rn(n, k), bias=rn(n), residual=rn(m, n), m=m, n=n, k=k, lda=k, ldb=k, ldc=n),
                (m + 1, n)))
    m, n, k, ldc = 257, 70, 328, 72
    out.append(("b scalar pad", ("highest", "high"), dict(a=rn(m, k), b=rn(n, k), bias=rn(n), residual=rn(m, ldc), scale=0.5, m=m, n=n, k=k,
                                                          lda=k, ldb=k, ldc=ldc), (m + 1, ldc)))
    bt, m, n, k = 3, 130, 70, 72
    lda, ldb, ldc = k + 8, k + 16, 76
    out.append(("c batched strided", ("highest", "high"),
                dict(a=rn(bt, m + 2, lda), b=rn(bt, n + 3, ldb), residual=rn(bt, m + 1, ldc), m=m, n=n, k=k, lda=lda, ldb=ldb, ldc=ldc, batch=bt,
                     stride_a=(m + 2) * lda, stride_b=(n + 3) * ldb, stride_c=(m + 1) * ldc), (bt, m + 1, ldc)))
    m, n, k, tr = 48, 70, 40, 16
    out.append(("d trans_rows", ("highest", "high"), dict(a=rn(m, k), b=rn(n, k), m=m, n=n, k=k, lda=k, ldb=k, ldc=24, stride_c=n * 24,
                                                          trans_rows=tr), (m // tr, n, 24)))
    m, n, k = 4096, 2048, 64
    out.append(("e big tiles", ("highest", "high"), dict(a=rn(m, k), b=rn(n, k), m=m, n=n, k=k, lda=k, ldb=k, ldc=n), (m, n)))

    stats = lambda rows: torch.stack([torch.randn(rows, generator=g) * 0.3, torch.rand(rows, generator=g) * 0.4 + 0.8], dim=1).to(DEV)  # noqa: E731
    m, n, k = 130, 70, 72
    out.append(("ln side 1", ("highest",), dict(a=rn(m, k), b=rn(n, k), bias=rn(n), scale=0.5, m=m, n=n, k=k, lda=k, ldb=k, ldc=72,
                                                ln_stats=stats(m), ln_colsum=rn(n), ln_shift=rn(n), ln_side=1), (m + 1, 72)))
    fr, rows, w = 3, 70, 130                              # Y_f^T = W LayerNorm(x_f)^T: the activation is B
    out.append(("ln side 2 batched", ("highest",),
                dict(a=rn(w, k), b=rn(fr, rows, k), m=w, n=rows, k=k, lda=k, ldb=k, ldc=72, batch=fr, stride_a=0, stride_b=rows * k,
                     stride_c=(w + 1) * 72, ln_stats=stats(fr * rows), ln_colsum=rn(w), ln_shift=rn(w), ln_side=2, stride_stats=rows),
                (fr, w + 1, 72)))
    m, n, k, r = 257, 132, 328, 64
    lr = lambda **kw: dict(a=rn(m, r + 64), b=rn(n, r + 8), k=r, lda=r + 64, ldb=r + 8, **kw)          # noqa: E731
    base = lambda: dict(a=rn(m, k), b=rn(n, k), bias=rn(n), residual=rn(m, n), m=m, n=n, k=k, lda=k, ldb=k, ldc=n)      # noqa: E731
    out.append(("lr 64", ("highest",), dict(base(), lr=lr()), (m + 1, n)))
    out.append(("lr 64 gain side 2", ("highest",), dict(base(), lr=lr(row_scale=rn(n), scale_side=2)), (m + 1, n)))
    bt, n2 = 3, 70                                        # ragged n: the scalar epilogue with the gain by m
    out.append(("lr 64 batched gain side 1", ("highest",),
                dict(a=rn(bt, m, k), b=rn(bt, n2, k), residual=rn(bt, m + 1, 72), scale=0.5, m=m, n=n2, k=k, lda=k, ldb=k, ldc=72, batch=bt,
                     stride_a=m * k, stride_b=n2 * k, stride_c=(m + 1) * 72,
                     lr=dict(a=rn(bt, m, r), b=rn(bt, n2, r), k=r, lda=r, ldb=r, stride_a=m * r, stride_b=n2 * r, row_scale=rn(m), scale_side=1)),
                (bt, m + 1, 72)))
    return out


def main():
    for name, precisions, prob, cshape in cases():
        for prec in precisions:
            c = torch.full(cshape, float("nan"), device=DEV)
            ops.gemm_nt([dict(prob, c=c, f32_precision=prec)])
            torch.cuda.synchronize()
            print(f"{name:28s} {prec:8s} {ops.last_gemm_variant():6s} {hashlib.sha256(c.cpu().numpy().tobytes()).hexdigest()}", flush=True)


if __name__ == "__main__":
    main()
