"""Guarded device buffers for the memory-contract tests (a plain module, imported by tests/test_hip_memory_contracts.py).

A ``Guarded`` buffer holds a strided tensor view — ``frames`` x ``rows`` x ``width`` elements, row stride ``ld`` >= width, frame
stride ``fs`` >= rows * ld — between two guard bands.  Every element of the buffer that is not part of the view (the columns
[width, ld) of every row, the gap rows behind every frame, both guard bands) holds a fill value:

* INPUTS are filled with NaN (or +Inf): a kernel that reads one of those elements into its arithmetic poisons its result;
* OUTPUTS are filled with a NON-CANONICAL NaN sentinel (fp16 0x7E5A, bf16 0x7FA5, fp32 0x7FC5A5A5), and the checks compare the
  raw bits through an integer view: a stray store of a zero, of a finite value or of a canonical NaN is caught.

The band behind the view is at least one 288-row tile of ``ld`` elements and at least 1 MiB, so a tile that over-reads or over-writes
lands in the band instead of in unmapped memory.  The view starts 16-byte aligned (the buffer's base is, the front band is a
multiple of 16 bytes, and ``ld`` / ``fs`` are multiples of 16 bytes whenever the caller's are).

The layout arithmetic (``Layout``) is pure integer code and has a CPU test (tests/test_guarded_layout.py); so does the buffer class
itself, on CPU tensors.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import torch

SENTINEL_BITS = {torch.float16: 0x7E5A, torch.bfloat16: 0x7FA5, torch.float32: 0x7FC5A5A5}
_INT_VIEW = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32}
FRONT_BYTES = 4096                      # guard band in front of the view
TAIL_MIN_BYTES = 1 << 20                # ... and behind it: at least this, and at least TAIL_TILE_ROWS rows of ld elements
TAIL_TILE_ROWS = 288


def round_up(x: int, a: int) -> int:
    return (x + a - 1) // a * a


def _signed(bits: int, dtype: torch.dtype) -> int:
    """The sentinel as the signed integer the integer view of ``dtype`` holds."""
    nb = 16 if _INT_VIEW[dtype] == torch.int16 else 32
    return bits - (1 << nb) if bits >= 1 << (nb - 1) else bits


def elem_size(dtype: torch.dtype) -> int:
    return torch.empty(0, dtype=dtype).element_size()


@dataclass(frozen=True)
class Layout:
    """Element offsets of a [frames, rows, width] view with row stride ``ld`` and frame stride ``fs`` inside a buffer of ``numel``
    elements whose first ``front`` elements (and everything from ``front + frames * fs`` on) are guard band."""
    frames: int
    rows: int
    width: int
    ld: int
    fs: int
    front: int
    numel: int
    esize: int

    @staticmethod
    def make(frames: int, rows: int, width: int, esize: int, ld: Optional[int] = None, gap_rows: int = 0,
             fs: Optional[int] = None) -> "Layout":
        ld = width if ld is None else ld
        if ld < width:
            raise ValueError(f"ld {ld} < width {width}")
        fs = rows * ld + gap_rows * ld if fs is None else fs
        if frames > 1 and fs < rows * ld:
            raise ValueError(f"frame stride {fs} < rows * ld = {rows * ld}")
        front = FRONT_BYTES // esize
        body = frames * fs if frames > 1 else max(fs, rows * ld)
        tail = max(TAIL_MIN_BYTES // esize, TAIL_TILE_ROWS * ld)
        return Layout(frames, rows, width, ld, fs, front, front + body + tail, esize)

    @property
    def body_end(self) -> int:
        """One past the last element of the last frame's stride (frame gaps of the last frame included)."""
        return self.front + (self.frames * self.fs if self.frames > 1 else max(self.fs, self.rows * self.ld))

    def offset(self, f: int, r: int, c: int) -> int:
        return self.front + f * self.fs + r * self.ld + c

    def where(self, off: int) -> str:
        """Human-readable position of a buffer element (for failure messages)."""
        if off < self.front:
            return f"front guard [{off - self.front}]"
        if off >= self.body_end:
            return f"tail guard [+{off - self.body_end}]"
        rel = off - self.front
        f, rem = divmod(rel, self.fs) if self.frames > 1 else (0, rel)
        r, c = divmod(rem, self.ld)
        return f"frame {f} row {r} col {c}"

    def region_mask(self, rows: Optional[int] = None, c0: int = 0, c1: Optional[int] = None,
                    frames: Optional[Sequence[int]] = None) -> torch.Tensor:
        """bool [numel] (CPU): the elements (frame in ``frames``, row < rows, c0 <= column < c1)."""
        rows = self.rows if rows is None else rows
        c1 = self.width if c1 is None else c1
        m = torch.zeros(self.numel, dtype=torch.bool)
        if rows <= 0 or c1 <= c0:
            return m
        frames = range(self.frames) if frames is None else frames
        for f in frames:
            start = self.front + f * self.fs
            block = m[start:start + rows * self.ld].view(rows, self.ld)
            block[:, c0:c1] = True
        return m

    def aligned16(self) -> bool:
        return (self.front * self.esize) % 16 == 0


class Guarded:
    """One guarded buffer on ``device`` (see the module docstring).  ``kind`` = "input" (fill NaN / +Inf) or "output" (sentinel)."""

    def __init__(self, frames: int, rows: int, width: int, dtype: torch.dtype, device, *, ld: Optional[int] = None,
                 gap_rows: int = 0, fs: Optional[int] = None, kind: str = "input", fill: str = "nan"):
        self.dtype = dtype
        self.layout = L = Layout.make(frames, rows, width, elem_size(dtype), ld=ld, gap_rows=gap_rows, fs=fs)
        self.buf = torch.empty(L.numel, dtype=dtype, device=device)
        self.bits = self.buf.view(_INT_VIEW[dtype])
        self.kind = kind
        if kind == "output":
            self.bits.fill_(_signed(SENTINEL_BITS[dtype], dtype))
        elif fill == "nan":
            self.buf.fill_(float("nan"))
        elif fill == "inf":
            self.buf.fill_(float("inf"))
        else:
            raise ValueError(fill)
        self.view = torch.as_strided(self.buf, (frames, rows, width), (L.fs, L.ld, 1), L.front)
        assert self.view.data_ptr() % 16 == 0, "view base not 16-byte aligned"
        self._snap: Optional[torch.Tensor] = None

    # ---- addressing ---------------------------------------------------------------------------------------------------------------
    @property
    def ptr(self) -> int:
        return self.view.data_ptr()

    @property
    def ld(self) -> int:
        return self.layout.ld

    @property
    def fs(self) -> int:
        return self.layout.fs

    def frame_view(self, rows: Optional[int] = None, width: Optional[int] = None) -> torch.Tensor:
        """[frames, rows, width] view over the first rows / columns of every frame (the region a call is told about)."""
        L = self.layout
        return torch.as_strided(self.buf, (L.frames, L.rows if rows is None else rows, L.width if width is None else width),
                                (L.fs, L.ld, 1), L.front)

    def set(self, values: torch.Tensor) -> "Guarded":
        """Copy ``values`` ([frames, rows, width] or [rows, width] for one frame) into the view; then snapshot (inputs)."""
        self.view.copy_(values.reshape(self.view.shape).to(self.dtype))
        if self.kind == "input":
            self.snapshot()
        return self

    def snapshot(self) -> None:
        self._snap = self.bits.clone()

    # ---- checks -------------------------------------------------------------------------------------------------------------------
    def _report(self, bad: torch.Tensor, what: str) -> str:
        idx = torch.nonzero(bad.cpu()).flatten()
        if idx.numel() == 0:
            return ""
        pos = [self.layout.where(int(i)) for i in idx[:6]]
        return f"{what}: {idx.numel()} element(s), first at " + "; ".join(pos)

    def untouched(self, writable: torch.Tensor) -> str:
        """'' if every element OUTSIDE ``writable`` (bool [numel] mask) still holds the sentinel, else a description."""
        sent = _signed(SENTINEL_BITS[self.dtype], self.dtype)
        bad = (self.bits != sent) & ~writable.to(self.bits.device)
        return self._report(bad, "written outside the writable region")

    def pad_is_zero(self, pad: torch.Tensor) -> str:
        """'' if every element of ``pad`` (bool [numel] mask) is exactly +0 (bits 0), else a description."""
        bad = (self.bits != 0) & pad.to(self.bits.device)
        return self._report(bad, "pad not +0")

    def inputs_unchanged(self) -> str:
        """'' if no bit of the buffer changed since the last snapshot (``set`` takes it), else a description."""
        assert self._snap is not None, "no snapshot"
        bad = self.bits != self._snap
        return self._report(bad, "input buffer modified")
