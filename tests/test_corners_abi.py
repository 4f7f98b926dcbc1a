"""Corner-weighted AID: the C ABI, without a GPU.

The new struct against the header as gcc lays it out, its mirror and the new prototypes in ``_lib.py``, every refusal of
``aid_mix_kv`` / ``aid_attn_corners_fwd`` / ``aid_processor_corners_fwd`` with a NULL stream (all checks run before the first launch, so
no device is needed), ``corners == NULL`` forwarded to ``aid_processor_fwd``, and the workspace size of a corner processor call."""
import ctypes as C
import os
import re
import subprocess

import pytest

from aid_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "aid_hip.h")).read()
NEW = ("aid_mix_kv", "aid_corners_scratch_bytes", "aid_attn_corners_fwd", "aid_processor_corners_workspace_bytes",
       "aid_processor_corners_fwd")
ARG, DTYPE, SHAPE, WORKSPACE = -1, -2, -3, -4


def test_entry_points_are_declared_exported_and_the_version_stays():
    for name in NEW:
        assert re.search(r"^(int|size_t)\s+%s\s*\(" % name, HEADER, flags=re.M), name
    assert set(NEW) <= set(_lib.ABI_SYMBOLS)
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in NEW)
    assert int(re.search(r"#define AID_MAX_CORNERS\s+(\d+)", HEADER).group(1)) == _lib.MAX_CORNERS == 8
    assert lib.aid_abi_version() == 10 and _lib.AID_ABI_VERSION == 10 and re.search(r"#define AID_ABI_VERSION 10\b", HEADER)
    assert lib.aid_mix_kv.argtypes[4] == C.POINTER(C.c_int32) and len(lib.aid_mix_kv.argtypes) == 13
    assert lib.aid_attn_corners_fwd.argtypes == [C.POINTER(_lib.AidAttnArgs), C.POINTER(_lib.AidCorners), C.c_void_p]
    assert lib.aid_processor_corners_fwd.argtypes == [C.POINTER(_lib.AidProcessorArgs), C.POINTER(_lib.AidCorners), C.c_void_p]
    assert lib.aid_processor_corners_workspace_bytes.restype == C.c_size_t and lib.aid_corners_scratch_bytes.restype == C.c_size_t


def test_struct_matches_the_header_layout_and_the_old_structs_are_unchanged(tmp_path):
    structs = {"AidCorners": _lib.AidCorners, "AidAttnArgs": _lib.AidAttnArgs, "AidProcessorArgs": _lib.AidProcessorArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "aid_hip.h"', 'int main(void) {']
    for name, cls in structs.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{name}.{fname} %zu\\n", offsetof({name}, {fname}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for name, cls in structs.items():
        assert int(out[name]) == C.sizeof(cls), name
        for fname, _ in cls._fields_:
            assert int(out[f"{name}.{fname}"]) == getattr(cls, fname).offset, f"{name}.{fname}"
    assert C.sizeof(_lib.AidCorners) == 40
    assert C.sizeof(_lib.AidProcessorArgs) == 440 and [f for f, _ in _lib.AidProcessorArgs._fields_][-1] == "lora_gain_o"
    assert C.sizeof(_lib.AidAttnArgs) == 216 and [f for f, _ in _lib.AidAttnArgs._fields_][-1] == "bias_rs"


def test_scratch_bytes():
    lib = _lib.load()
    for n, m in ((1, 1), (8, 2), (8, 3), (14, 8), (1000, 5)):
        floats = (1 + 2 * ((m + 1) // 2)) * n
        got = lib.aid_corners_scratch_bytes(n, m)
        assert got >= 4 * floats and got % 256 == 0 and got < 4 * floats + 256, (n, m, got)
    for n, m in ((0, 2), (-1, 2), (4, 0), (4, 9), (4, -1)):
        assert lib.aid_corners_scratch_bytes(n, m) == 0


# ---- aid_mix_kv --------------------------------------------------------------------------------------------------------------------
def _mix(**kw):
    """Arguments of a well-formed aid_mix_kv call (pointers are never dereferenced: every check precedes the launch)."""
    rows = (C.c_int32 * 8)(2, 0, 1, 3, 4, 5, 6, 7)
    a = dict(k=0x1000, vt=0x2000, k2=0x3000, vt2=0x4000, rows=rows, weights=0x5000, n_frames=7, n_plain=2, n_corners=3,
             k_fs=72 * 80, vt_fs=80 * 72, dtype=_lib.DTYPE_F16)
    a.update(kw)
    return a


def _mix_call(a):
    rows = a["rows"] if a["rows"] is not None else C.POINTER(C.c_int32)()
    return _lib.load().aid_mix_kv(a["k"], a["vt"], a["k2"], a["vt2"], rows, a["weights"], a["n_frames"], a["n_plain"], a["n_corners"],
                                  a["k_fs"], a["vt_fs"], a["dtype"], None)


@pytest.mark.parametrize("field,value,code", [
    ("k", None, ARG), ("vt", None, ARG), ("k2", None, ARG), ("vt2", None, ARG), ("rows", None, ARG), ("weights", None, ARG),
    ("n_corners", 0, ARG), ("n_corners", 9, ARG), ("n_corners", -1, ARG), ("n_plain", -1, ARG), ("n_plain", 8, ARG), ("n_frames", 0, ARG),
    ("k_fs", 72 * 80 + 4, SHAPE), ("vt_fs", 80 * 72 + 4, SHAPE), ("k_fs", 0, SHAPE), ("vt_fs", -8, SHAPE),
    ("k", 0x1008, SHAPE), ("vt", 0x2004, SHAPE), ("k2", 0x3008, SHAPE), ("vt2", 0x4002, SHAPE), ("weights", 0x5002, SHAPE),
    ("dtype", 3, DTYPE), ("dtype", -1, DTYPE)])
def test_mix_kv_refusals_return_their_codes_before_any_launch(field, value, code):
    assert _mix_call(_mix(**{field: value})) == code


@pytest.mark.parametrize("m", [1, 3, 8])
def test_mix_kv_checks_every_row(m):
    rows = (C.c_int32 * 8)(*range(8))
    rows[m - 1] = -1                                     # the LAST of m rows is the negative one
    assert _mix_call(_mix(rows=rows, n_corners=m)) == ARG
    if m < 8:                                            # ... and rows past n_corners are not read
        rows[m - 1], rows[m] = 0, -1
        assert _mix_call(_mix(rows=rows, n_corners=m, n_plain=7)) == 0       # (n_plain == n_frames: nothing to launch)


def test_mix_kv_with_every_frame_a_rider_launches_nothing():
    for dt in (_lib.DTYPE_F16, _lib.DTYPE_BF16, _lib.DTYPE_F32):
        assert _mix_call(_mix(n_plain=7, dtype=dt)) == 0


# ---- aid_attn_corners_fwd ----------------------------------------------------------------------------------------------------------
def _attn(mode=_lib.MODE_OUTER, **kw):
    a = _lib.AidAttnArgs()
    a.q, a.k, a.vt, a.out, a.k2, a.vt2 = 0x1000, 0x2000, 0x3000, 0x4000, 0x6000, 0x7000
    a.n_frames, a.n_kv, a.s, a.l, a.heads, a.d = 8, 8, 72, 72, 2, 64
    a.ldq = a.ldk = a.ldo = 128
    a.ldvt = 72
    a.q_fs, a.k_fs, a.vt_fs, a.o_fs = 72 * 128, 72 * 128, 128 * 72, 72 * 128
    a.mode, a.fused, a.dtype, a.softmax_scale, a.n_plain = mode, 1, _lib.DTYPE_BF16, 0.125, 2
    a.begin = a.end = 99                                 # not read
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _corners(m=3, rows=None, **kw):
    c = _lib.AidCorners()
    arr = (C.c_int32 * 8)(*(rows if rows is not None else [2, 0, 1, 3, 4, 5, 6, 7]))
    c.rows, c.weights, c.scratch, c.scratch_bytes, c.n_corners = arr, 0x5000, 0x8000, 4096, m
    for k, v in kw.items():
        setattr(c, k, v)
    c._keep = arr
    return c


def _attn_call(a, c):
    return _lib.load().aid_attn_corners_fwd(None if a is None else C.byref(a), None if c is None else C.byref(c), None)


def test_attn_corners_refusals_return_their_codes_before_any_launch():
    assert _attn_call(None, _corners()) == ARG and _attn_call(_attn(), None) == ARG
    assert _attn_call(_attn(_lib.MODE_PLAIN), _corners()) == ARG
    for m in (0, 9, -1):
        assert _attn_call(_attn(), _corners(m)) == ARG
    null_rows = _corners()
    null_rows.rows = C.POINTER(C.c_int32)()
    assert _attn_call(_attn(), null_rows) == ARG
    assert _attn_call(_attn(), _corners(weights=None)) == ARG and _attn_call(_attn(), _corners(scratch=None)) == ARG
    assert _attn_call(_attn(), _corners(weights=0x5002)) == SHAPE and _attn_call(_attn(), _corners(scratch=0x8008)) == SHAPE
    # rows: negative, and >= n_kv (the last of the m rows; rows past n_corners are not read)
    assert _attn_call(_attn(), _corners(3, [0, 1, -1, 0, 0, 0, 0, 0])) == ARG
    assert _attn_call(_attn(), _corners(3, [0, 1, 8, 0, 0, 0, 0, 0])) == ARG
    assert _attn_call(_attn(n_kv=4, kv_map=0x9000), _corners(2, [3, 4, 0, 0, 0, 0, 0, 0])) == ARG
    assert _attn_call(_attn(n_plain=-1), _corners()) == ARG and _attn_call(_attn(n_plain=9), _corners()) == ARG
    # the pair table: [1 + 2 ceil(M / 2), n_frames] floats
    need = _lib.load().aid_corners_scratch_bytes(8, 3)
    assert _attn_call(_attn(), _corners(scratch_bytes=need - 1)) == WORKSPACE
    # every refusal of aid_attn_fwd, a bias with fused included
    assert _attn_call(_attn(bias=0xA000), _corners()) == ARG
    assert _attn_call(_attn(q=None), _corners()) == ARG and _attn_call(_attn(dtype=7), _corners()) == DTYPE
    assert _attn_call(_attn(d=48), _corners()) == SHAPE and _attn_call(_attn(out=0x4004), _corners()) == SHAPE
    assert _attn_call(_attn(_lib.MODE_INNER, k2=None), _corners()) == ARG
    assert _attn_call(_attn(_lib.MODE_INNER, k_fs=0), _corners()) == SHAPE


# ---- aid_processor_corners_fwd -----------------------------------------------------------------------------------------------------
def _proc(mode=_lib.MODE_OUTER, n=8, cross=False, **kw):
    a = _lib.AidProcessorArgs()
    for f in ("x", "wq", "wk", "wv", "wo", "y"):
        setattr(a, f, 0x1000)
    a.n_frames, a.s, a.l, a.c, a.cc, a.heads, a.mode, a.dtype, a.n_ctx = n, 72, 72, 128, 128, 2, mode, _lib.DTYPE_F16, n
    a.fused, a.n_plain = 1, 2
    a.begin = a.end = 99                                 # coef (NULL), begin and end are not read
    if cross:
        a.ctx, a.ctx_map, a.l, a.cc, a.n_ctx = 0x2000, 0x3000, 77, 96, 4
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_processor_corners_checks_everything_before_its_first_launch():
    """With a NULL workspace a well-formed call gets as far as AID_ERR_WORKSPACE (-4) without a GPU; a malformed one is refused before."""
    lib = _lib.load()
    fwd = lambda a_, c_: lib.aid_processor_corners_fwd(C.byref(a_), None if c_ is None else C.byref(c_), None)          # noqa: E731
    size = lambda a_, c_: lib.aid_processor_corners_workspace_bytes(C.byref(a_), None if c_ is None else C.byref(c_))    # noqa: E731
    assert lib.aid_processor_corners_fwd(None, C.byref(_corners()), None) == ARG
    assert lib.aid_processor_corners_workspace_bytes(None, None) == 0
    for mode in (_lib.MODE_OUTER, _lib.MODE_INNER):
        assert fwd(_proc(mode), _corners()) == WORKSPACE and size(_proc(mode), _corners()) > 0
        assert fwd(_proc(mode, cross=True), _corners(2, [3, 0, 9, 9, 9, 9, 9, 9])) == WORKSPACE
    # corners == NULL is aid_processor_fwd: its checks (coef is NULL here: refused; with a coefficient vector and end points: as far
    # as the workspace), its size
    plain = _proc(_lib.MODE_PLAIN)
    assert fwd(plain, None) == lib.aid_processor_fwd(C.byref(plain), None) == WORKSPACE
    assert size(plain, None) == lib.aid_processor_workspace_bytes(C.byref(plain)) > 0
    assert fwd(_proc(), None) == lib.aid_processor_fwd(C.byref(_proc()), None) == ARG
    two = _proc(coef=0x1000, begin=0, end=7)
    assert fwd(two, None) == lib.aid_processor_fwd(C.byref(two), None) == WORKSPACE
    assert size(two, None) == lib.aid_processor_workspace_bytes(C.byref(two))
    # what a corner call refuses
    assert fwd(plain, _corners()) == ARG and size(plain, _corners()) == 0
    ip = _proc(cross=True, ip=0x4000, wk_ip=0x5000, wv_ip=0x6000, n_ip=8, t_ip=4, ip_mode=_lib.IP_PLAIN, ip_stride=4 * 96)
    assert fwd(ip, _corners(2, [0, 1, 0, 0, 0, 0, 0, 0])) == ARG
    for m in (0, 9):
        assert fwd(_proc(), _corners(m)) == ARG and size(_proc(), _corners(m)) == 0
    assert fwd(_proc(), _corners(weights=None)) == ARG and fwd(_proc(), _corners(weights=0x5002)) == SHAPE
    assert fwd(_proc(), _corners(3, [0, 1, 8, 0, 0, 0, 0, 0])) == ARG            # row >= n_frames (self-attention)
    assert fwd(_proc(cross=True), _corners(2, [3, 4, 0, 0, 0, 0, 0, 0])) == ARG   # row >= n_ctx (cross-attention)
    assert fwd(_proc(n_plain=9), _corners()) == ARG and fwd(_proc(n_plain=-1), _corners()) == ARG
    assert fwd(_proc(attn_bias=0x7000), _corners()) == ARG                        # a bias with fused, as today
    assert fwd(_proc(fused=0, attn_bias=0x7000), _corners()) == WORKSPACE
    assert fwd(_proc(wq=None), _corners()) == ARG and fwd(_proc(dtype=5), _corners()) == DTYPE
    # AidCorners.scratch is not read: the table is carved from the workspace
    assert fwd(_proc(), _corners(scratch=None, scratch_bytes=0)) == WORKSPACE


@pytest.mark.parametrize("cross", [False, True], ids=["self", "cross"])
@pytest.mark.parametrize("m", [1, 2, 3, 8])
def test_processor_corners_workspace_holds_the_call_the_mix_and_the_pair_table(m, cross):
    lib = _lib.load()
    al = lambda x: (x + 255) // 256 * 256                                         # noqa: E731
    n, c, es = 8, 128, 2
    l, lp = (77, 80) if cross else (72, 72)
    rows = [0, 1, 2, 3, 0, 1, 2, 3] if cross else list(range(8))
    table = al(4 * (1 + 2 * ((m + 1) // 2)) * n)
    sizes = {}
    for mode in (_lib.MODE_OUTER, _lib.MODE_INNER):
        a = _proc(mode, cross=cross, coef=0x1000, begin=0, end=1)
        base = lib.aid_processor_workspace_bytes(C.byref(a))
        got = lib.aid_processor_corners_workspace_bytes(C.byref(a), C.byref(_corners(m, rows)))
        assert base > 0 and got >= base + table, (mode, base, got)
        sizes[mode] = (base, got)
    # INNER's call already holds k2 / vt2, one row per frame: the corner call mixes into them
    k2vt2 = al(n * l * c * es) + al(n * c * lp * es)
    assert sizes[_lib.MODE_INNER][0] == sizes[_lib.MODE_OUTER][0] + k2vt2
    assert sizes[_lib.MODE_INNER][1] >= sizes[_lib.MODE_OUTER][0] + k2vt2 + table
