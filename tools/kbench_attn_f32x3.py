#!/usr/bin/env python3
"""float32 attention core: the three-term bf16 split (aid_attn_f32x3_kernel, f32_attn_precision="high") against the exact kernel
(aid_attn_f32_kernel) on the same tensors, alternating, three repeats with their spread.

Shapes: the SD1.5 stack at batch 3 — self-attention S = L = 4096 d 40, 1024 d 80, 256 d 160, 64 d 160 (8 heads) and the
cross-attention launches of the same levels with L = 77 text keys — and the SDXL d = 64 self-attention at S = L = 1024 (20 heads)
and 4096 (10 heads); plain, fused inner and fused outer each.  Prints us and TFLOP/s (4 S L C per key segment, the library's own
accounting) of the attention launch alone (INNER's aid_lerp_kv launch is not counted); `verdict` = split faster than exact by more
than the repeats' spread — what plan_attn's rule for "high" is held against."""
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
    ent = [e for e in buf[:n] if e.kernel.decode().startswith("aid_attn_f32")]
    return sum(e.ms for e in ent) / len(ent) * 1e3, sum(e.flops for e in ent) / len(ent), ent[0].kernel.decode()


def ab(tag, call, iters):
    res = {"highest": [], "high": []}
    names = {}
    for _ in range(3):
        for prec in ("highest", "high"):
            us, fl, nm = timed(lambda: call(prec), iters)
            res[prec].append(us)
            names[prec] = nm
    e, s = res["highest"], res["high"]
    med = lambda v: sorted(v)[1]                                     # noqa: E731
    spread = max(max(e) - min(e), max(s) - min(s))
    verdict = "split" if med(e) - med(s) > spread else "exact"
    print(f"{tag:38s} exact {med(e):8.1f} us [{min(e):.1f} .. {max(e):.1f}] {fl / med(e) / 1e6:6.1f} TF/s | "
          f"split {med(s):8.1f} us [{min(s):.1f} .. {max(s):.1f}] {fl / med(s) / 1e6:6.1f} TF/s | x{med(e) / med(s):5.2f} -> {verdict}"
          f"   ({names['highest']} / {names['high']})", flush=True)


def main():
    g = torch.Generator(device="cpu").manual_seed(0)
    rn = lambda *sh: torch.randn(*sh, generator=g).to(dev)          # noqa: E731
    shapes = [("sd15 self", 3, 4096, 4096, 8, 40), ("sd15 self", 3, 1024, 1024, 8, 80), ("sd15 self", 3, 256, 256, 8, 160),
              ("sd15 self", 3, 64, 64, 8, 160), ("sd15 cross", 3, 4096, 77, 8, 40), ("sd15 cross", 3, 1024, 77, 8, 80),
              ("sd15 cross", 3, 256, 77, 8, 160), ("sd15 cross", 3, 64, 77, 8, 160), ("sdxl self", 3, 1024, 1024, 20, 64),
              ("sdxl self", 3, 4096, 4096, 10, 64)]
    coef = torch.tensor([0.0, 0.35, 1.0], device=dev)
    for tag, n, s, l, h, d in shapes:
        c, lp = h * d, (l + 7) // 8 * 8
        q, k, vt, out = rn(n, s, c), rn(n, l, c), torch.zeros(n, c, lp, device=dev), torch.empty(n, s, c, device=dev)
        vt[:, :, :l] = rn(n, c, l)
        iters = 5 if s * l >= 4096 * 4096 else 20
        for mode, fused in (("plain", False), ("inner", True), ("outer", True)):
            ab(f"{tag} S={s} L={l} d={d} h={h} {'fused ' if fused else ''}{mode}",
               lambda prec: ops.attn_fwd(q, k, vt, h, l=l, mode=mode, fused=fused, coef=coef, out=out, f32_attn_precision=prec), iters)


if __name__ == "__main__":
    main()
