#!/usr/bin/env python3
"""Development: the ping-pong attention kernel of two BUILDS of the library side by side (tools/dev/pp_boundary_ab.py's method: both
loaded into one process, rounds interleaved, the order rotating and turning).  usage:
    python tools/dev/pp_mfma16_ab.py parent=path/to/parent/libaid_hip.so new=attention-interpolation-diffusion_amd/libaid_hip.so \
        [parent2=path/to/parent/libaid_hip.so new2=...] [--rounds 9] [--iters 8]
Launches (7 AID frames + 7 riders each): fused OUTER and PLAIN at S = 4096 / 10 heads and at S = 1024 / 20 heads, fused INNER at
S = 4096; bf16 and f16; N(0, 1) operands (q * 0.6, already scaled) and zeros: on zeros the chip holds its top clock and the builds are
ranked by cycles, on random operands by the clock the power limit leaves them.  ATTN_V2 = 1 puts every launch on
the ping-pong kernel; the kernel that ran is printed with every line.  A build named twice (parent2=, new2=: the same file under a
second name) gives the spread between repeated rows of one build.
Outputs: rel L2 of every variant against the first, and — the yardstick — of the first variant's ping-pong kernel against its
program-order kernel (ATTN_V2 = 0) on the same call: both differences are reorderings of the same sums."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import aid_amd  # noqa: E402
from aid_amd import _lib, ops  # noqa: E402

opt = lambda k, d: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d     # noqa: E731
ROUNDS, ITERS = int(opt("--rounds", 9)), int(opt("--iters", 8))
variants, bound = [], {}
for a in sys.argv[1:]:
    if "=" in a and not a.startswith("--"):
        name, path = a.split("=", 1)
        path = path if os.path.isabs(path) else os.path.join(ROOT, path)
        if path not in bound:
            bound[path] = _lib.bind(path)
        variants.append((name, bound[path]))
dev = torch.device("cuda:0")


def use(lib, v2=1):
    _lib._lib = lib
    ops.set_tuning("ATTN_V2", v2)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / ITERS


def rel(x, y):
    if torch.equal(x, y):
        return "bit-identical"
    return f"rel L2 {float((x.float() - y.float()).norm() / y.float().norm().clamp_min(1e-30)):.1e}"


n = 7
for dt in (torch.bfloat16, torch.float16):
    for zeros in (False, True):
        for s, h, modes in ((4096, 10, ("outer", "plain", "inner")), (1024, 20, ("outer", "plain"))):
            c = h * 64
            g = torch.Generator(device=dev).manual_seed(s)
            mk = (lambda *sh: torch.zeros(*sh, device=dev)) if zeros else (lambda *sh: torch.randn(*sh, device=dev, generator=g))
            q, k, vt = (mk(2 * n, s, c) * 0.6).to(dt), mk(2 * n, s, c).to(dt), mk(2 * n, c, s).to(dt)
            cf = aid_amd.generate_beta_tensor(n, 50, 50)
            cf[0], cf[-1] = 0, 1
            coef = torch.tensor(cf.to(dt).float().tolist() + [-1.0] * n, device=dev)
            for mode in modes:
                fused = mode != "plain"
                out = torch.empty_like(q)
                kw = dict(l=s, mode=mode, fused=fused, coef=coef if fused else None, begin=0, end=n - 1, out=out, n_plain=n if fused else 0,
                          q_prescaled=True)
                fn = lambda: ops.attn_fwd(q, k, vt, h, **kw)       # noqa: E731
                outs, names = {}, {}
                for name, lib in variants:
                    use(lib); fn(); fn(); torch.cuda.synchronize()
                    names[name] = ops.last_attn_variant()
                    outs[name] = out.clone()
                first = variants[0][0]
                use(variants[0][1], 0); fn(); torch.cuda.synchronize()
                yard = f"{first} against its {ops.last_attn_variant()}: {rel(outs[first], out)}"
                res = {name: [] for name, _ in variants}
                for r in range(ROUNDS):
                    order = variants[r % len(variants):] + variants[:r % len(variants)]
                    for name, lib in (order if r % 2 == 0 else order[::-1]):
                        use(lib)
                        res[name].append(timed(fn))
                for name, _ in variants:
                    t = res[name]
                    print(f"S{s} H{h} {mode:5s} {str(dt)[6:]:8s} {'zeros ' if zeros else 'N(0,1)'} {name:8s} {names[name]:22s} median {statistics.median(t):7.1f} us"
                          f"  min {min(t):7.1f}  max {max(t):7.1f}  ratio to {first} {statistics.median(t) / statistics.median(res[first]):.3f}"
                          f"   vs {first}: {rel(outs[name], outs[first])}", flush=True)
                print(f"S{s} H{h} {mode:5s} {str(dt)[6:]:8s} {'zeros ' if zeros else 'N(0,1)'} yardstick: {yard}", flush=True)
            del q, k, vt
print("done")
