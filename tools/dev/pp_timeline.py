"""Development: timelines of the ping-pong attention kernel (ablation build: make -C tools/dev, AID_LIB_PATH=tools/dev/libaid_abl.so).
  bit 32   workgroup start-up: shader cycles from kernel entry to [Q requested + DMA issued | first three tiles landed | first product
           done, loop starts | loop done].
  bit 256  one item boundary of a persistent workgroup, per wave group: shader cycles since the barrier behind the finished item's last M
           slot of [finish() done | plan + Q request done | V(0) done | barrier behind it passed | ... V(3) ...], for plain and fused outer
           at S = 1024 and S = 4096 (7 + 7 frames), as built and with + 512 = the per-frame records as vector loads, each drained by vmcnt(0)
           (what the kernel did before round 7).  Group 1 of a persistent workgroup does finish() and plan + Q in FRONT of the barrier
           behind its last M slot: its origin is the end of that M slot and its "plan+Q" column includes the wait at that barrier.
           The stamps cost registers: the OUTER instantiation of the ablation build spills, read
           its rows as relative."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
import aid_amd
from aid_amd import ops
dev = torch.device("cuda:0")
if "--no-startup" not in sys.argv:
    for s_, h in ((1024, 20), (4096, 10)):
        n, d = 14, 64
        c = h * d
        q = torch.randn(n, s_, c, device=dev).to(torch.bfloat16); k = torch.randn(n, s_, c, device=dev).to(torch.bfloat16)
        vt = torch.randn(n, c, s_, device=dev).to(torch.bfloat16); out = torch.zeros_like(q)
        ops.set_tuning("ATTN_V2", 1); ops.set_tuning("ATTN_RES_CHUNKS", 132)
        for rep in range(2):
            out.zero_(); ops.attn_fwd(q, k, vt, h, l=s_, mode="plain", out=out); torch.cuda.synchronize()
        rows = out.view(n, s_ // 32, 32, h, d)[:, :, 0, :, :10].contiguous()
        f = rows.view(torch.int16).view(n, s_ // 32, h, 10).contiguous().view(torch.float32).view(n, s_ // 32, h, 5).float()
        m = f.reshape(-1, 5)[:, :4].mean(0).tolist()
        print(f"S={s_}: issue done {m[0]:8.0f} | 3 tiles landed {m[1]:8.0f} | loop starts {m[2]:8.0f} | loop done {m[3]:8.0f} cycles; tiles {s_ // 64}")

# ---- the item boundary (bit 256) ----
NAMES = ["finish", "plan+Q", "V0", "bar", "V1", "bar", "V2", "bar", "V3", "bar"]
MARK = (0x50504254, 0x4c494e45)
n = 7
for s_, h in ((1024, 20), (4096, 10)):
    d = 64
    c = h * d
    g = torch.Generator(device=dev).manual_seed(s_)
    q = (torch.randn(2 * n, s_, c, device=dev, generator=g) * 0.6).to(torch.bfloat16)
    k = torch.randn(2 * n, s_, c, device=dev, generator=g).to(torch.bfloat16)
    vt = torch.randn(2 * n, c, s_, device=dev, generator=g).to(torch.bfloat16)
    cf = aid_amd.generate_beta_tensor(n, 50, 50)
    cf[0], cf[-1] = 0, 1
    coef = torch.tensor(cf.to(torch.bfloat16).float().tolist() + [-1.0] * n, device=dev)
    for mode in ("plain", "outer"):
        fused = mode != "plain"
        for abl, what in ((256, "as built"), (256 + 512, "vector-loaded records")):
            ops.set_tuning("ATTN_V2", 1); ops.set_tuning("ATTN_RES_CHUNKS", 100 + abl)
            out = torch.zeros_like(q)
            for rep in range(2):
                ops.attn_fwd(q, k, vt, h, l=s_, mode=mode, fused=fused, coef=coef if fused else None, begin=0, end=n - 1, out=out,
                             n_plain=n if fused else 0)
                torch.cuda.synchronize()
            # first row of every wave's 32 rows, first 13 words of head hh: [mark, mark, 11 stamps]
            rows = out.view(2 * n, s_ // 32, 32, h, d)[:, :, 0, :, :26].contiguous()
            w = rows.view(torch.int16).view(2 * n, s_ // 32, h, 26).contiguous().view(torch.int32).view(2 * n, s_ // 32, h, 13).cpu().numpy().astype(np.int64) & 0xffffffff
            grp = (np.arange(s_ // 32) % 8) // 4
            hit = (w[..., 0] == MARK[0]) & (w[..., 1] == MARK[1])
            print(f"S={s_} {mode:5s} {what}: {int(hit.sum())} stamped waves, cycles since the barrier behind the last M slot (mean; step in brackets)")
            for gi in (0, 1):
                sel = hit & (grp[None, :, None] == gi)
                if not sel.any():
                    continue
                st = w[sel][:, 3:].astype(np.float64)           # (stamp 0 is the origin)
                mean = st.mean(0)
                step = np.diff(np.concatenate([[0.0], mean]))
                print(f"   group {gi}: " + "  ".join(f"{nm} {m_:6.0f} [{d_:5.0f}]" for nm, m_, d_ in zip(NAMES, mean, step)))
ops.set_tuning("ATTN_RES_CHUNKS", -1)
