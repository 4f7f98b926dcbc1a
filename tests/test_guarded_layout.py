"""CPU test of the guarded-buffer helper (tests/guarded.py): layout arithmetic, alignment, region masks and the three checks, on
CPU tensors — the GPU memory-contract tests (tests/test_hip_memory_contracts.py) rely on all of it."""
import pytest
import torch

from guarded import SENTINEL_BITS, TAIL_MIN_BYTES, TAIL_TILE_ROWS, Guarded, Layout, round_up

DTYPES = [torch.float16, torch.bfloat16, torch.float32]
ids_dt = lambda d: str(d).split(".")[-1]  # noqa: E731


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("frames,rows,width,ld,gap", [(1, 5, 77, 88, 0), (3, 40, 77, 96, 3), (2, 1, 8, 8, 1), (4, 300, 1280, 1288, 0)])
def test_layout_strides_alignment_and_guard_sizes(dtype, frames, rows, width, ld, gap):
    es = torch.empty(0, dtype=dtype).element_size()
    L = Layout.make(frames, rows, width, es, ld=ld, gap_rows=gap)
    assert L.ld == ld and L.fs == (rows + gap) * ld
    assert L.aligned16() and (L.front * es) % 16 == 0
    assert L.offset(0, 0, 0) == L.front
    assert L.offset(frames - 1, rows - 1, width - 1) < L.body_end <= L.numel
    tail = L.numel - L.body_end
    assert tail * es >= TAIL_MIN_BYTES and tail >= TAIL_TILE_ROWS * ld
    assert L.where(L.offset(frames - 1, rows - 1, width - 1)) == f"frame {frames - 1} row {rows - 1} col {width - 1}"
    assert L.where(0).startswith("front guard") and L.where(L.numel - 1).startswith("tail guard")
    m = L.region_mask()
    assert int(m.sum()) == frames * rows * width
    m2 = L.region_mask(rows=rows - 1, c0=width, c1=ld)
    assert int(m2.sum()) == frames * (rows - 1) * (ld - width)
    assert not (m & m2).any()


def test_layout_rejects_inconsistent_strides():
    with pytest.raises(ValueError):
        Layout.make(1, 4, 16, 2, ld=8)
    with pytest.raises(ValueError):
        Layout.make(2, 4, 16, 2, ld=16, fs=32)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
def test_output_checks_catch_every_kind_of_stray_store(dtype):
    frames, rows, width, ld = 2, 6, 13, 24
    g = Guarded(frames, rows, width, dtype, "cpu", ld=ld, gap_rows=2, kind="output")
    assert g.view.stride() == (8 * ld, ld, 1) and g.ptr % 16 == 0
    L = g.layout
    vals = L.region_mask()
    pad = L.region_mask(c0=width, c1=round_up(width, 4))
    g.view.copy_(torch.randn(frames, rows, width).to(dtype))
    g.frame_view(width=round_up(width, 4))[:, :, width:] = 0
    assert g.untouched(vals | pad) == "" and g.pad_is_zero(pad) == ""
    # a stray zero / finite value / canonical NaN just past the pad, in a gap row, in the tail guard: each is caught
    for off in (L.offset(1, 3, round_up(width, 4)), L.offset(0, rows, 0), L.body_end + 5, L.front - 1):
        for v in (0.0, 1.5, float("nan")):
            saved = g.bits[off].clone()
            g.buf[off] = v
            msg = g.untouched(vals | pad)
            assert msg and L.where(off) in msg, (off, v, msg)
            g.bits[off] = saved
    assert g.untouched(vals | pad) == ""
    # the pad must be +0: -0 and the sentinel (never written) both fail
    g.buf[L.offset(0, 2, width)] = -0.0
    assert "pad not +0" in g.pad_is_zero(pad)
    g.buf[L.offset(0, 2, width)] = 0.0
    g.bits[L.offset(1, 0, width + 1)] = g.bits[0]          # sentinel bits
    assert "frame 1 row 0 col %d" % (width + 1) in g.pad_is_zero(pad)


@pytest.mark.parametrize("fill", ["nan", "inf"])
def test_input_buffer_is_poisoned_outside_the_view_and_snapshotted(fill):
    dtype = torch.bfloat16
    g = Guarded(3, 4, 10, dtype, "cpu", ld=16, gap_rows=1, fill=fill)
    x = torch.randn(3, 4, 10)
    g.set(x)
    assert torch.equal(g.view.float(), x.to(dtype).float())
    outside = g.buf[~g.layout.region_mask()].float()
    assert (torch.isnan(outside).all() if fill == "nan" else torch.isposinf(outside).all())
    assert g.inputs_unchanged() == ""
    g.buf[g.layout.offset(2, 4, 3)] = 1.0                   # a write into the gap row of the last frame
    assert "frame 2 row 4 col 3" in g.inputs_unchanged()


def test_sentinels_are_non_canonical_nans():
    for dtype, bits in SENTINEL_BITS.items():
        g = Guarded(1, 1, 8, dtype, "cpu", kind="output")
        v = g.buf[:4].float()
        assert torch.isnan(v).all()
        canon = torch.tensor([float("nan")], dtype=dtype)
        ib = g.bits[:1]
        assert int(canon.view(ib.dtype)[0]) != int(ib[0]) and (int(ib[0]) & ((1 << (8 * g.buf.element_size())) - 1)) == bits
