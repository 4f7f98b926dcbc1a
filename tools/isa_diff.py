#!/usr/bin/env python3
"""Compare two device-assembly files kernel by kernel: did a source change alter the code of the kernels it was not meant to touch?

Make the inputs with the Makefile's flags plus `--cuda-device-only -S`, one file per build:
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffast-math -fno-finite-math-only --cuda-device-only -S csrc/aid_gemm.hip -o new.s
The attention objects take the extra flags csrc/Makefile gives them: `-mllvm -amdgpu-mfma-vgpr-form=1 -ffinite-math-only` for aid_attn.hip
and aid_attn_pp.hip, `-mllvm -amdgpu-mfma-vgpr-form=1` alone for aid_attn_tx.hip.
Per function symbol the instruction stream is kept (comments and directives dropped, local label numbers normalised).  Symbols are
paired after removing what only names the low-rank variant of a GEMM kernel: a `_lr` suffix of the kernel name and the NoLR / GemmLR
template argument; a kernel with the segment (GemmLR anywhere in its symbol) only pairs with one that has it too.  Prints SAME or DIFF
per pair with the line counts; for a DIFF of equal length, the number of differing lines and (--show N) the first N of them.
--mix: under every DIFF, the mnemonics whose instruction counts differ (old -> new).  A DIFF whose list holds only scalar and integer
bookkeeping (s_load_*, s_waitcnt, s_mov_*, v_mov_*, address arithmetic) kept its arithmetic and its memory accesses; one that lists
a v_mfma_*, v_fma_*, v_mul_*, v_add_f32, v_pk_*, v_cvt_*, global_*, ds_* or s_barrier line did not.  No list: same mix, other order
or registers.
usage (CPU only):  python tools/isa_diff.py old.s new.s [--show N] [--mix]"""
import argparse, collections, re


def key(sym):
    """pairing key of a mangled symbol: (name + template arguments without the low-rank markers, carries a segment)"""
    s = re.sub(r"^_ZN3aid\d+", "", sym).replace("_lrI", "I").replace("NS_4NoLRE", "").replace("NS_6GemmLRE", "")
    return s.split("Ev")[0], "GemmLR" in sym


def kernels(path):
    """{pairing key: (symbol, [instruction lines])}"""
    out, sym, body = {}, None, []
    for line in open(path):
        m = re.match(r"\s*\.type\s+(\w+),@function", line)
        if m:
            sym, body = m.group(1), []
        elif line.startswith(".Lfunc_end") and sym:
            out[key(sym)] = (sym, body)
            sym = None
        elif sym:
            t = line.split(";")[0].strip()
            if t and t != sym + ":" and (not t.startswith(".") or t.startswith(".LBB")):
                body.append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s+", " ", t)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--show", type=int, default=0, help="print the first N differing lines of a DIFF of equal length")
    ap.add_argument("--mix", action="store_true", help="print the per-mnemonic instruction counts that differ in a DIFF")
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    for k in sorted(set(old) | set(new)):
        name = k[0] + (" +lr" if k[1] else "")
        if k not in old or k not in new:
            print(f"{'ONLY-OLD' if k in old else 'ONLY-NEW':8s} {name}")
            continue
        bo, bn = old[k][1], new[k][1]
        if bo == bn:
            print(f"SAME     {name}  ({len(bo)} lines)")
            continue
        pairs = [(x, y) for x, y in zip(bo, bn) if x != y] if len(bo) == len(bn) else []
        print(f"DIFF     {name}  ({len(bo)} -> {len(bn)} lines" + (f", {len(pairs)} differ)" if pairs else ")"))
        for x, y in pairs[:a.show]:
            print(f"             {x}   ->   {y}")
        if a.mix:
            co, cn = (collections.Counter(t.split()[0] for t in b if not t.startswith(".LBB")) for b in (bo, bn))
            for mn in sorted(set(co) | set(cn)):
                if co[mn] != cn[mn]:
                    print(f"             {mn:28s} {co[mn]:6d} -> {cn[mn]:6d}")


if __name__ == "__main__":
    main()
