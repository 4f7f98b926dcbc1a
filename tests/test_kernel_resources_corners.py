"""CPU: the build's resource table of csrc/aid_corners.hip.  The mix kernel keeps the M corner chunks of a lane in registers (M is a
template parameter): no instantiation may spill or touch scratch, and every (dtype, M) the launcher can pick must be there."""
import re

from test_kernel_resources import _table


def test_corner_kernels_neither_spill_nor_use_scratch():
    tab = _table("aid_corners")
    mix = {}
    for sym, r in tab.items():
        assert r["scratch"] == 0 and r["spill"] == 0 and r["sgpr_spill"] == 0, (sym, r)
        m = re.search(r"aid_mix_kv_kernelI(DF16_|DF16b|f)Li(\d)E", sym)
        if m:
            mix[({"DF16_": "f16", "DF16b": "bf16", "f": "f32"}[m.group(1)], int(m.group(2)))] = r
    assert set(mix) == {(dt, m) for dt in ("f16", "bf16", "f32") for m in range(1, 9)}, sorted(mix)
    assert any("aid_corner_pairs_kernel" in sym for sym in tab)
    assert len(tab) == 25
    # a streaming kernel: the corner chunks (8 fp32 per corner for the 16-bit types) must not cost the occupancy that hides HBM latency
    assert all(r["occ"] >= 4 for r in mix.values()), {k: r["occ"] for k, r in mix.items()}
