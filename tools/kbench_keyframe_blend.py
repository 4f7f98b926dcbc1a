#!/usr/bin/env python3
"""Cost of the key-frame blend: the fused aid_mix_kv_stores launch against the two launches it replaces
(aid_keyframe_rows[_q8] GET of the M rows + aid_mix_kv on them), and the whole aid_processor_kf_blend_fwd call, fused INNER and
fused OUTER.  Live timing (aid_profile_begin / aid_profile_end), median of 7 calls after 2 warm-up calls, one process.

Shape: the SDXL level-1 self-attention block — S = 4096, C = 640 (10 heads of 64), N = 7 local frames, bf16, M in {2, 4, 8}, native
and q8 stores.  Output: profiles/keyframe_blend.txt holds one run of this tool.

    python tools/kbench_keyframe_blend.py [--s 4096] [--c 640] [--n 7]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aid_amd  # noqa: E402
from aid_amd import _lib, ops  # noqa: E402

DEV = torch.device("cuda:0")
REPS, WARM = 7, 2


def profiled(fn):
    """{kernel name: (ms, bytes)} summed per name over one call of ``fn``."""
    lib = _lib.load()
    lib.aid_profile_begin()
    fn()
    buf = (_lib.AidProfileEntry * 256)()
    cnt = lib.aid_profile_end(buf, 256)
    out = {}
    for e in buf[:cnt]:
        ms, by = out.get(e.kernel.decode(), (0.0, 0.0))
        out[e.kernel.decode()] = (ms + e.ms, by + e.bytes)
    return out


def median_of(fn, pick):
    """Median over REPS calls of (ms, bytes) summed over the entries whose name ``pick`` accepts."""
    rows = []
    for i in range(WARM + REPS):
        ent = profiled(fn)
        if i >= WARM:
            rows.append((sum(ms for k, (ms, _) in ent.items() if pick(k)), sum(b for k, (_, b) in ent.items() if pick(k))))
    return statistics.median(r[0] for r in rows), rows[0][1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--s", type=int, default=4096)
    ap.add_argument("--c", type=int, default=640)
    ap.add_argument("--n", type=int, default=7)
    a = ap.parse_args()
    s, c, n, heads, dtype = a.s, a.c, a.n, a.c // 64, torch.bfloat16
    k_fs, vt_fs = ops.endpoint_block_sizes(s, c)
    lp = vt_fs // c
    g = torch.Generator().manual_seed(0)
    rnd = lambda *sh, sc=1.0: (torch.randn(*sh, generator=g) * sc).to(dtype).to(DEV)      # noqa: E731
    w4 = [rnd(c, c, sc=c ** -0.5) for _ in range(4)]
    bo = rnd(c, sc=0.1)
    x = rnd(n, s, c)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    print(f"# {torch.cuda.get_device_name(0)}; S {s} C {c} heads {heads} N {n} bf16; block k {k_fs} + vt {vt_fs} elements = "
          f"{2 * (k_fs + vt_fs) / 1e6:.2f} MB native, {(ops.q8_block_bytes(k_fs) + ops.q8_block_bytes(vt_fs)) / 1e6:.2f} MB q8; "
          f"median of {REPS} after {WARM} warm-up calls")
    print("# launch: ms and achieved GB/s over the algorithmic bytes of the launch (aid_hip.h)")
    print(f"{'M':>2} {'store':>6} | {'GET ms':>8} {'mix ms':>8} {'pair ms':>8} {'pair GB/s':>9} | {'fused ms':>8} {'GB/s':>7} {'fused/pair':>10} | "
          f"{'call INNER ms':>13} {'call OUTER ms':>13} {'ws INNER MB':>11} {'ws OUTER MB':>11}")
    for m in (2, 4, 8):
        keys = rnd(m, s, c)
        for storage in ("native", "q8"):
            if storage == "q8":
                stores = [(torch.zeros(1, ops.q8_block_bytes(k_fs), dtype=torch.uint8, device=DEV),
                           torch.zeros(1, ops.q8_block_bytes(vt_fs), dtype=torch.uint8, device=DEV)) for _ in range(m)]
            else:
                stores = [(torch.zeros(1, k_fs, dtype=dtype, device=DEV), torch.zeros(1, vt_fs, dtype=dtype, device=DEV)) for _ in range(m)]
            ent = [(k_, v_, i) for i, (k_, v_) in enumerate(stores)]
            kf = dict(entries=ent, step=step, mode="record")
            if storage == "q8":
                kf["storage"] = "q8"
            ops.processor_kf_fwd(keys, *w4, bo, heads, kf=kf, mode="plain")
            wts = torch.rand(n, m, generator=g) + 0.05
            wts = (wts / wts.sum(1, keepdim=True)).float().to(DEV)
            ksc = torch.empty(m, s, c, dtype=dtype, device=DEV)
            vsc = torch.empty(m, c, lp, dtype=dtype, device=DEV)
            k2 = torch.empty(n, s, c, dtype=dtype, device=DEV)
            vt2 = torch.empty(n, c, lp, dtype=dtype, device=DEV)
            get = (lambda: ops.keyframe_rows_q8(ksc, vsc, ent, step, "get", vt_cols=s)) if storage == "q8" else \
                (lambda: ops.keyframe_rows(ksc, vsc, ent, step, "get"))

            def pair():
                get()
                ops.mix_kv(ksc, vsc, wts, list(range(m)), out=(k2, vt2))

            def fused():
                ops.mix_kv_stores(ent, step, wts, (s, c), (c, lp), dtype, storage=storage, vt_cols=s, out=(k2, vt2))

            get_ms, get_b = median_of(pair, lambda k: k.startswith("aid_keyframe_rows"))
            mix_ms, mix_b = median_of(pair, lambda k: k.startswith("aid_mix_kv<"))
            pair_ms, pair_b = median_of(pair, lambda k: True)
            f_ms, f_b = median_of(fused, lambda k: k.startswith("aid_mix_kv_stores"))
            blend = dict(kf, mode="blend")
            calls, wsb = {}, {}
            for mode in ("inner", "outer"):
                fn = lambda: ops.processor_kf_blend_fwd(x, *w4, bo, heads, kf=blend, weights=wts, mode=mode, fused=True)      # noqa: E731
                calls[mode], _ = median_of(fn, lambda k: True)
                a_ = _lib.AidProcessorArgs()
                for f_ in ("x", "wq", "wk", "wv", "wo", "y"):
                    setattr(a_, f_, x.data_ptr())
                a_.n_frames, a_.s, a_.l, a_.c, a_.cc, a_.heads, a_.n_ctx = n, s, s, c, c, heads, n
                a_.mode, a_.fused, a_.dtype = (_lib.MODE_INNER if mode == "inner" else _lib.MODE_OUTER), 1, _lib.DTYPE_BF16
                kb, _keep = ops._keyframe_blend_args(dict(blend, weights=wts), n, s, c, dtype)
                wsb[mode] = _lib.load().aid_processor_kf_blend_workspace_bytes(C.byref(a_), C.byref(kb))
            print(f"{m:>2} {storage:>6} | {get_ms:8.4f} {mix_ms:8.4f} {pair_ms:8.4f} {pair_b / pair_ms / 1e6:9.1f} | {f_ms:8.4f} "
                  f"{f_b / f_ms / 1e6:7.1f} {f_ms / pair_ms:10.3f} | {calls['inner']:13.4f} {calls['outer']:13.4f} "
                  f"{wsb['inner'] / 1e6:11.1f} {wsb['outer'] / 1e6:11.1f}")


if __name__ == "__main__":
    main()
