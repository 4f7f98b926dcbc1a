#!/usr/bin/env python3
"""Development: what an item boundary of the persistent ping-pong attention kernel costs — same-process interleaved A/B of several
BUILDS of the library and / or knob settings.  usage:
    python tools/dev/pp_boundary_ab.py parent=path/to/parent/libaid_hip.so new=attention-interpolation-diffusion_amd/libaid_hip.so \
        [vec=tools/dev/libaid_abl.so:ATTN_RES_CHUNKS=612] [--rounds 7] [--iters 8] [--reps 3] [--no-fit] [--no-launches]
A variant is name=library[:KNOB=value,...].  The ablation build (make -C tools/dev) takes ATTN_RES_CHUNKS = 100 + bits: 512 reads the
per-frame records with vector loads (each drained by vmcnt(0)) as the kernel did before round 7.

launches  the four d = 64 self-attention launches of the SDXL stack (7 AID frames + 7 riders, bf16): fused outer and plain at S = 4096 and
          S = 1024, by the default rule and with ATTN_V2 = 1 (plain S = 1024 on the ping-pong kernel); median / min / max us over the rounds.
fit       plain, S = 1024, 20 heads: n = 16 / 32 / 48 frames give every one of the 256 workgroups exactly 5 / 10 / 15 items, key count
          512 / 1024 / 2048 gives 8 / 16 / 32 tiles per item.  time = a + tau * (items * tiles) + beta * (items - 1), least squares over the
          nine points, repeated --reps times: a = start-up, tau = tile period, beta = cost of one item boundary."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import aid_amd  # noqa: E402
from aid_amd import _lib, ops  # noqa: E402

opt = lambda k, d: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d     # noqa: E731
ROUNDS, ITERS, REPS = int(opt("--rounds", 7)), int(opt("--iters", 8)), int(opt("--reps", 3))
KNOBS = ("ATTN_V2", "ATTN_PIPE", "ATTN_RES_CHUNKS")
variants, bound = [], {}
for a in sys.argv[1:]:
    if "=" not in a or a.startswith("--"):
        continue
    name, rest = a.split("=", 1)
    path, _, kn = rest.partition(":")
    path = path if os.path.isabs(path) else os.path.join(ROOT, path)
    if path not in bound:
        bound[path] = _lib.bind(path)
    variants.append((name, bound[path], dict((k, int(v)) for k, v in (kv.split("=") for kv in kn.split(",") if kv))))
dev = torch.device("cuda:0")
dt = torch.bfloat16


def use(lib, knobs, extra=None):
    _lib._lib = lib
    kn = dict(knobs, **(extra or {}))
    for k in KNOBS:
        ops.set_tuning(k, kn.get(k, -1))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / ITERS


def interleaved(cases):
    """cases: [(label, lib, knobs, fn)] -> {label: [us per round]}, every round visits every case once.  The order rotates and turns
    round from round: what a launch costs depends on what ran just before it (the power state a hot or a cool kernel leaves behind:
    measured 5 % between two variants that differ in nothing they execute), so no case keeps the same predecessor."""
    for _, lib, kn, fn in cases:
        use(lib, kn); fn(); fn()
    torch.cuda.synchronize()
    res = {c[0]: [] for c in cases}
    for r in range(ROUNDS):
        order = cases[r % len(cases):] + cases[:r % len(cases)]
        for label, lib, kn, fn in (order if r % 2 == 0 else order[::-1]):
            use(lib, kn)
            res[label].append(timed(fn))
    return res


if "--no-launches" not in sys.argv:
    n = 7
    for s, h in ((4096, 10), (1024, 20)):
        c = h * 64
        g = torch.Generator(device=dev).manual_seed(s)
        q = (torch.randn(2 * n, s, c, device=dev, generator=g) * 0.6).to(dt)
        k = torch.randn(2 * n, s, c, device=dev, generator=g).to(dt)
        vt = torch.randn(2 * n, c, s, device=dev, generator=g).to(dt)
        cf = aid_amd.generate_beta_tensor(n, 50, 50)
        cf[0], cf[-1] = 0, 1
        coef = torch.tensor(cf.to(dt).float().tolist() + [-1.0] * n, device=dev)
        for mode in ("outer", "plain"):
            fused = mode != "plain"
            out = torch.empty_like(q)
            kw = dict(l=s, mode=mode, fused=fused, coef=coef if fused else None, begin=0, end=n - 1, out=out, n_plain=n if fused else 0)
            fn = lambda: ops.attn_fwd(q, k, vt, h, **kw)       # noqa: E731
            cases, names, outs = [], {}, {}
            for v2 in (-1, 1):
                for name, lib, kn in variants:
                    kn2 = dict(kn, ATTN_V2=v2)
                    label = f"{name}{' V2=1' if v2 == 1 else ''}"
                    use(lib, kn2); fn(); torch.cuda.synchronize()
                    names[label] = ops.last_attn_variant()
                    outs[label] = out.clone()
                    cases.append((label, lib, kn2, fn))
            res = interleaved(cases)
            first = cases[0][0]
            for label, _, _, _ in cases:
                r = res[label]
                same = "bit-identical" if torch.equal(outs[label], outs[first]) else \
                    f"rel L2 {float((outs[label].float() - outs[first].float()).norm() / outs[first].float().norm()):.1e}"
                print(f"S{s} H{h} {mode:6s} {label:14s} {names[label]:30s} median {statistics.median(r):8.1f} us  min {min(r):8.1f}  max {max(r):8.1f}"
                      f"   vs {first}: {same}", flush=True)
        del q, k, vt

if "--no-fit" not in sys.argv:
    s, h = 1024, 20
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    frames = (16, 32, 48)
    qs = {n: torch.randn(n, s, h * 64, device=dev).to(dt) for n in frames}
    for rep in range(REPS):
        pts = {v[0]: [] for v in variants}
        for l in (512, 1024, 2048):
            for n in frames:
                q = qs[n]
                k = torch.randn(n, l, h * 64, device=dev).to(dt)
                vt = torch.randn(n, h * 64, l, device=dev).to(dt)
                out = torch.empty_like(q)
                fn = lambda: ops.attn_fwd(q, k, vt, h, l=l, mode="plain", out=out)     # noqa: E731
                res = interleaved([(name, lib, dict(kn, ATTN_V2=1), fn) for name, lib, kn in variants])
                items = 4 * n * h / cus
                for name in res:
                    pts[name].append((items, l // 64, statistics.median(res[name])))
                del k, vt, out
        for name, p in pts.items():
            p = np.asarray(p)
            A = np.stack([np.ones(len(p)), p[:, 0] * p[:, 1], p[:, 0] - 1], axis=1)
            (a_, tau, beta), resid = np.linalg.lstsq(A, p[:, 2], rcond=None)[:2]
            rms = float(np.sqrt(resid[0] / len(p))) if len(resid) else 0.0
            print(f"fit rep {rep} {name:10s} a {a_:6.2f} us  tau {tau:6.3f} us per tile  beta {beta:6.2f} us per item boundary  (rms residual {rms:.2f} us; "
                  f"points " + " ".join(f"{int(i)}x{int(t)}:{u:.1f}" for i, t, u in p) + ")", flush=True)
print("done")
