#!/usr/bin/env python3
"""Development: the 288-row GEMM engine of two BUILDS of the library side by side (tools/dev/pp_boundary_ab.py's method: both loaded
into one process, rounds interleaved, the order rotating and turning).  usage:
    python tools/dev/ppx_mfma16_ab.py parent=path/to/parent/libaid_hip.so new=attention-interpolation-diffusion_amd/libaid_hip.so \
        [--rounds 9] [--iters 20]
Shapes: the SDXL out projection 14336 x 1280 x 1280; the grouped q / k / V^T launch over it (third problem transposed per frame of
1024 rows); 32768 x 1280 x 1280; 4096^3.  bf16 and f16, N(0, 1) operands (weights / sqrt(k)) and zeros: on zeros the chip holds its
top clock and the builds are ranked by cycles, on random operands by the clock the power limit leaves them.
The engine is forced (GEMM_VARIANT = 31, GEMM_TRI = 1, GEMM_RS = 0); the kernel that ran is printed with every line."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from aid_amd import _lib, ops  # noqa: E402

opt = lambda k, d: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d     # noqa: E731
ROUNDS, ITERS = int(opt("--rounds", 9)), int(opt("--iters", 20))
variants = []
for a in sys.argv[1:]:
    if "=" in a and not a.startswith("--"):
        name, path = a.split("=", 1)
        variants.append((name, _lib.bind(path if os.path.isabs(path) else os.path.join(ROOT, path))))
dev = torch.device("cuda:0")


def use(lib):
    _lib._lib = lib
    for k, v in (("GEMM_VARIANT", 31), ("GEMM_TRI", 1), ("GEMM_RS", 0)):
        ops.set_tuning(k, v)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / ITERS


def problems(kind, m, n, k, dt, zeros):
    g = torch.Generator(device=dev).manual_seed(m + n + k)
    mk = (lambda *s: torch.zeros(*s, device=dev)) if zeros else (lambda *s: torch.randn(*s, device=dev, generator=g))
    a = mk(m, k).to(dt)
    if kind == "single":
        c = torch.empty(m, n, device=dev, dtype=dt)
        return [dict(a=a, b=(mk(n, k) / k ** 0.5).to(dt), c=c, m=m, n=n, k=k, lda=k, ldb=k, ldc=n)], [c]
    rows = 1024                                                              # grouped q / k / V^T over one activation
    cs = [torch.empty(m, n, device=dev, dtype=dt), torch.empty(m, n, device=dev, dtype=dt), torch.empty(m // rows, n, rows, device=dev, dtype=dt)]
    ws = [(mk(n, k) / k ** 0.5).to(dt) for _ in range(3)]
    base = dict(a=a, m=m, n=n, k=k, lda=k, ldb=k)
    return [dict(base, b=ws[0], c=cs[0], ldc=n), dict(base, b=ws[1], c=cs[1], ldc=n),
            dict(base, b=ws[2], c=cs[2], ldc=rows, stride_c=n * rows, trans_rows=rows)], cs


for kind, m, n, k in (("single", 14336, 1280, 1280), ("qkv", 14336, 1280, 1280), ("single", 32768, 1280, 1280), ("single", 4096, 4096, 4096)):
    for dt in (torch.bfloat16, torch.float16):
        for zeros in (False, True):
            pr, cs = problems(kind, m, n, k, dt, zeros)
            fn = lambda: ops.gemm_nt(pr)                                      # noqa: E731
            outs, names = {}, {}
            for name, lib in variants:
                use(lib); fn(); fn(); torch.cuda.synchronize()
                names[name] = ops.last_gemm_variant()
                outs[name] = [c.clone() for c in cs]
            res = {name: [] for name, _ in variants}
            for r in range(ROUNDS):
                order = variants[r % len(variants):] + variants[:r % len(variants)]
                for name, lib in (order if r % 2 == 0 else order[::-1]):
                    use(lib)
                    res[name].append(timed(fn))
            first = variants[0][0]
            for name, _ in variants:
                t = res[name]
                num = sum(float((x.float() - y.float()).square().sum()) for x, y in zip(outs[name], outs[first]))
                den = sum(float(y.float().square().sum()) for y in outs[first])
                same = "bit-identical" if all(torch.equal(x, y) for x, y in zip(outs[name], outs[first])) else f"rel L2 {(num / max(den, 1e-30)) ** 0.5:.1e}"
                print(f"{kind:6s} {m}x{n}x{k} {str(dt)[6:]:8s} {'zeros ' if zeros else 'N(0,1)'} {name:7s} {names[name]:12s} median {statistics.median(t):7.1f} us"
                      f"  min {min(t):7.1f}  max {max(t):7.1f}  ratio to {first} {statistics.median(t) / statistics.median(res[first]):.3f}   vs {first}: {same}",
                      flush=True)
            del pr, cs, outs
print("done")
