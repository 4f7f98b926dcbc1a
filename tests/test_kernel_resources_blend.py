"""CPU: the build's resource table of csrc/aid_keyframe_blend.hip.  aid_mix_kv_stores keeps the M corner chunks of a lane in
registers, as aid_mix_kv does (M is a template parameter): no instantiation may spill or touch scratch, every (dtype, M, storage) the
launcher can pick must be there, and none may need more registers than the first build's table showed."""
import re

from test_kernel_resources import _table

VGPR_BUDGET = 98          # the largest of the first build: bf16, M = 8, q8 stores (native M = 8: 96, as aid_mix_kv's M = 8)


def test_mix_kv_stores_kernels_neither_spill_nor_use_scratch_and_keep_their_registers():
    tab = _table("aid_keyframe_blend")
    mix = {}
    for sym, r in tab.items():
        assert r["scratch"] == 0 and r["spill"] == 0 and r["sgpr_spill"] == 0, (sym, r)
        m = re.search(r"aid_mix_kv_stores_kernelI(DF16_|DF16b|f)Li(\d)ELb([01])E", sym)
        assert m, sym
        mix[({"DF16_": "f16", "DF16b": "bf16", "f": "f32"}[m.group(1)], int(m.group(2)), "q8" if m.group(3) == "1" else "native")] = r
    assert set(mix) == {(dt, m, st) for dt in ("f16", "bf16", "f32") for m in range(1, 9) for st in ("native", "q8")}, sorted(mix)
    assert len(tab) == 48
    over = {k: r["vgpr"] for k, r in mix.items() if r["vgpr"] > VGPR_BUDGET}
    assert not over, over
    # a streaming kernel: the corner chunks must not cost the occupancy that hides HBM latency
    assert all(r["occ"] >= 4 for r in mix.values()), {k: r["occ"] for k, r in mix.items()}
