"""Register budgets of the ping-pong GEMM kernels with the low-rank segment (CPU test: reads the table the build leaves next to the
objects, like tests/test_kernel_resources.py).  The 256-row kernel exists with and without the segment (GemmLR / NoLR); the 288-row
kernel has no segment instantiation — with one it did not fit 256 registers — and is the kernel it was."""
import re

from test_kernel_resources import _table


def _pp(tab):
    """(dtype, K-loop flavour, carries the segment) -> resources of aid_gemm_nt_pp_kernel"""
    out = {}
    for sym, r in tab.items():
        m = re.search(r"aid_gemm_nt_pp_kernelIDF16(b?)_?Li(\d)ENS_(4NoLR|6GemmLR)E", sym)
        if m:
            out[("bf16" if m.group(1) else "f16", int(m.group(2)), m.group(3) == "6GemmLR")] = r
    return out


def test_segment_instantiations_of_the_256_row_kernel_keep_two_waves_per_simd():
    pp = _pp(_table("aid_gemm"))
    for dt in ("f16", "bf16"):
        for loop in (0, 1, 2):
            assert (dt, loop, True) in pp, (dt, loop)
            r = pp[(dt, loop, True)]
            assert r["vgpr"] + r["agpr"] <= 256 and r["occ"] >= 2, r
            assert r["scratch"] == 0 and r["spill"] == 0 and r["sgpr_spill"] == 0, r


def test_kernels_without_the_segment_keep_their_registers():
    """213 (256-row) and 248 (288-row) VGPRs, no AGPRs: the counts of the build before the segment existed."""
    tab = _table("aid_gemm")
    pp = _pp(tab)
    for dt in ("f16", "bf16"):
        for loop in (0, 1, 2):
            r = pp[(dt, loop, False)]
            assert (r["vgpr"], r["agpr"], r["scratch"], r["spill"], r["sgpr_spill"]) == (213, 0, 0, 0, 0), (dt, loop, r)
    ppx = {s: r for s, r in tab.items() if "aid_gemm_nt_ppx_kernel" in s}
    assert len(ppx) == 2 and not any("GemmLR" in s for s in ppx), list(ppx)
    for sym, r in ppx.items():
        assert (r["vgpr"], r["agpr"], r["occ"], r["scratch"], r["spill"], r["sgpr_spill"]) == (248, 0, 2, 0, 0, 0), (sym, r)
