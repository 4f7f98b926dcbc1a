"""Key-frame blend: the C ABI, without a GPU.

The new struct against the header as gcc lays it out, its mirror and the new prototypes in ``_lib.py``, every refusal of
``aid_mix_kv_stores`` / ``aid_processor_kf_blend_fwd`` with a NULL stream (all checks run before the first launch, so no device is
needed and no pointer is dereferenced), ``b == NULL`` forwarded to ``aid_processor_fwd``, and the workspace size of a blend call."""
import ctypes as C
import os
import re
import subprocess

import pytest

from aid_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "aid_hip.h")).read()
NEW = ("aid_mix_kv_stores", "aid_processor_kf_blend_workspace_bytes", "aid_processor_kf_blend_fwd")
ARG, DTYPE, SHAPE, WORKSPACE = -1, -2, -3, -4


def test_entry_points_are_declared_exported_and_the_version_stays():
    for name in NEW:
        assert re.search(r"^(int|size_t)\s+%s\s*\(" % name, HEADER, flags=re.M), name
    assert set(NEW) <= set(_lib.ABI_SYMBOLS)
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in NEW)
    assert lib.aid_abi_version() == 10 and _lib.AID_ABI_VERSION == 10 and re.search(r"#define AID_ABI_VERSION 10\b", HEADER)
    assert _lib.MAX_CORNERS == _lib.KF_MAX_ROWS == 8
    assert lib.aid_mix_kv_stores.argtypes[0] == C.POINTER(_lib.AidKeyframeBlend) and len(lib.aid_mix_kv_stores.argtypes) == 11
    assert lib.aid_processor_kf_blend_fwd.argtypes == [C.POINTER(_lib.AidProcessorArgs), C.POINTER(_lib.AidKeyframeBlend), C.c_void_p]
    assert lib.aid_processor_kf_blend_workspace_bytes.restype == C.c_size_t


def test_struct_matches_the_header_layout_and_the_old_structs_are_unchanged(tmp_path):
    structs = {"AidKeyframeBlend": _lib.AidKeyframeBlend, "AidCorners": _lib.AidCorners, "AidAttnArgs": _lib.AidAttnArgs,
               "AidProcessorArgs": _lib.AidProcessorArgs, "AidKeyframeRow": _lib.AidKeyframeRow}
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
    assert C.sizeof(_lib.AidKeyframeBlend) == 40
    assert C.sizeof(_lib.AidProcessorArgs) == 440 and C.sizeof(_lib.AidAttnArgs) == 216 and C.sizeof(_lib.AidCorners) == 40


# ---- the blend struct ----------------------------------------------------------------------------------------------------------------
def _blend(m=3, **kw):
    """A well-formed AidKeyframeBlend over never-dereferenced pointers; ``k_store_<i>`` / ``vt_store_<i>`` override one entry."""
    rows = (_lib.AidKeyframeRow * 8)()
    for i in range(8):
        rows[i].k_store, rows[i].vt_store, rows[i].row = 0x10000 + 0x100 * i, 0x20000 + 0x100 * i, -7        # `row` is ignored
    b = _lib.AidKeyframeBlend()
    b.rows, b.step, b.weights, b.n_corners, b.n_steps, b.q8 = rows, 0x6000, 0x5000, m, 4, 0
    for k, v in kw.items():
        if k == "rows":
            b.rows = C.POINTER(_lib.AidKeyframeRow)()
        elif k.startswith(("k_store_", "vt_store_")):
            field, i = k.rsplit("_", 1)
            setattr(rows[int(i)], field, v)
        else:
            setattr(b, k, v)
    b._keep = rows
    return b


# what is wrong with the struct itself: the same codes from both entry points
BLEND_REFUSALS = [
    (dict(rows=None), ARG), (dict(step=None), ARG), (dict(weights=None), ARG), (dict(step=0x6002), ARG),
    (dict(k_store_0=None), ARG), (dict(vt_store_2=None), ARG),
    (dict(n_corners=0), ARG), (dict(n_corners=9), ARG), (dict(n_corners=-1), ARG), (dict(n_steps=0), ARG),
    (dict(q8=2), ARG), (dict(q8=-1), ARG),
    (dict(k_store_1=0x10108), SHAPE), (dict(vt_store_2=0x20204), SHAPE), (dict(weights=0x5002), SHAPE),
]


# ---- aid_mix_kv_stores ---------------------------------------------------------------------------------------------------------------
def _mix(**kw):
    a = dict(b=_blend(), k2=0x3000, vt2=0x4000, n_frames=7, n_plain=2, k_fs=72 * 80, vt_fs=80 * 72, vt_ld=72, vt_cols=70,
             dtype=_lib.DTYPE_F16)
    a.update(kw)
    return a


def _mix_call(a):
    return _lib.load().aid_mix_kv_stores(None if a["b"] is None else C.byref(a["b"]), a["k2"], a["vt2"], a["n_frames"], a["n_plain"],
                                         a["k_fs"], a["vt_fs"], a["vt_ld"], a["vt_cols"], a["dtype"], None)


@pytest.mark.parametrize("q8", [0, 1])
@pytest.mark.parametrize("kw,code", BLEND_REFUSALS, ids=lambda v: str(v))
def test_mix_kv_stores_refuses_a_bad_blend_before_any_launch(kw, code, q8):
    if "q8" in kw:
        assert _mix_call(_mix(b=_blend(**kw))) == code
    else:
        assert _mix_call(_mix(b=_blend(q8=q8, **kw))) == code


@pytest.mark.parametrize("field,value,code", [
    ("k2", None, ARG), ("vt2", None, ARG), ("n_frames", 0, ARG), ("n_plain", -1, ARG), ("n_plain", 8, ARG),
    ("k_fs", 72 * 80 + 4, SHAPE), ("vt_fs", 80 * 72 + 4, SHAPE), ("k_fs", 0, SHAPE), ("vt_fs", -8, SHAPE),
    ("k2", 0x3008, SHAPE), ("vt2", 0x4002, SHAPE), ("dtype", 3, DTYPE), ("dtype", -1, DTYPE)])
def test_mix_kv_stores_refusals_return_their_codes_before_any_launch(field, value, code):
    for q8 in (0, 1):
        assert _mix_call(_mix(b=_blend(q8=q8), **{field: value})) == code
    assert _mix_call(_mix(b=None)) == ARG


@pytest.mark.parametrize("kw", [dict(vt_ld=0), dict(vt_ld=4), dict(vt_ld=76, vt_cols=70), dict(vt_ld=56, vt_cols=50),
                                dict(vt_cols=0), dict(vt_cols=73)], ids=lambda v: str(v))
def test_the_pad_column_rules_are_checked_for_q8_stores_only(kw):
    """vt_ld % 8, vt_ld >= 8, vt_fs % vt_ld, 1 <= vt_cols <= vt_ld — the rules of aid_keyframe_rows_q8; a native call does not read
    them (n_plain == n_frames: a well-formed call launches nothing, so it returns 0 without a device)."""
    assert _mix_call(_mix(b=_blend(q8=1), n_plain=7, **kw)) == SHAPE
    assert _mix_call(_mix(b=_blend(q8=0), n_plain=7, **kw)) == 0
    assert _mix_call(_mix(b=_blend(q8=1), n_plain=7)) == 0


@pytest.mark.parametrize("m", [1, 3, 8])
def test_mix_kv_stores_checks_every_entry_and_none_past_the_last(m):
    assert _mix_call(_mix(b=_blend(m, **{f"vt_store_{m - 1}": None}), n_plain=7)) == ARG
    assert _mix_call(_mix(b=_blend(m, **{f"k_store_{m - 1}": 0x10008}), n_plain=7)) == SHAPE
    if m < 8:
        assert _mix_call(_mix(b=_blend(m, **{f"k_store_{m}": None}), n_plain=7)) == 0
    for dt in (_lib.DTYPE_F16, _lib.DTYPE_BF16, _lib.DTYPE_F32):
        assert _mix_call(_mix(b=_blend(m), n_plain=7, dtype=dt)) == 0


# ---- aid_processor_kf_blend_fwd ------------------------------------------------------------------------------------------------------
def _proc(mode=_lib.MODE_OUTER, n=5, **kw):
    a = _lib.AidProcessorArgs()
    for f in ("x", "wq", "wk", "wv", "wo", "y"):
        setattr(a, f, 0x1000)
    a.n_frames, a.s, a.l, a.c, a.cc, a.heads, a.mode, a.dtype, a.n_ctx = n, 76, 76, 128, 128, 2, mode, _lib.DTYPE_F16, n
    a.fused, a.n_plain = 1, 2
    a.begin = a.end = 99                                 # coef (NULL), begin and end are not read
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _fwd(a, b):
    return _lib.load().aid_processor_kf_blend_fwd(None if a is None else C.byref(a), None if b is None else C.byref(b), None)


def _size(a, b):
    return _lib.load().aid_processor_kf_blend_workspace_bytes(None if a is None else C.byref(a), None if b is None else C.byref(b))


@pytest.mark.parametrize("mode", [_lib.MODE_OUTER, _lib.MODE_INNER], ids=["outer", "inner"])
@pytest.mark.parametrize("kw,code", BLEND_REFUSALS, ids=lambda v: str(v))
def test_processor_blend_refuses_a_bad_blend_before_any_launch(kw, code, mode):
    assert _fwd(_proc(mode), _blend(**kw)) == code and _size(_proc(mode), _blend(**kw)) == 0
    if "q8" not in kw:
        assert _fwd(_proc(mode), _blend(q8=1, **kw)) == code and _size(_proc(mode), _blend(q8=1, **kw)) == 0


def test_processor_blend_checks_everything_before_its_first_launch():
    """With a NULL workspace a well-formed call gets as far as AID_ERR_WORKSPACE (-4) without a GPU; a malformed one is refused before."""
    lib = _lib.load()
    assert _fwd(None, _blend()) == ARG and _size(None, _blend()) == 0 and _size(None, None) == 0
    for mode in (_lib.MODE_OUTER, _lib.MODE_INNER):
        for q8 in (0, 1):
            for m in (1, 2, 8):
                assert _fwd(_proc(mode), _blend(m, q8=q8)) == WORKSPACE and _size(_proc(mode), _blend(m, q8=q8)) > 0
        assert _fwd(_proc(mode, fused=0), _blend()) == WORKSPACE
        assert _fwd(_proc(mode, workspace=0x100000, workspace_bytes=_size(_proc(mode), _blend()) - 1), _blend()) == WORKSPACE
    # b == NULL is aid_processor_fwd: its checks (coef is NULL here: refused; with a coefficient vector and end points: as far as the
    # workspace), its size
    plain = _proc(_lib.MODE_PLAIN)
    assert _fwd(plain, None) == lib.aid_processor_fwd(C.byref(plain), None) == WORKSPACE
    assert _size(plain, None) == lib.aid_processor_workspace_bytes(C.byref(plain)) > 0
    assert _fwd(_proc(), None) == lib.aid_processor_fwd(C.byref(_proc()), None) == ARG
    two = _proc(coef=0x1000, begin=0, end=4)
    assert _fwd(two, None) == lib.aid_processor_fwd(C.byref(two), None) == WORKSPACE
    assert _size(two, None) == lib.aid_processor_workspace_bytes(C.byref(two))
    # what a blend call refuses: a PLAIN call, a context, an image branch, n_plain outside [0, n_frames]
    assert _fwd(plain, _blend()) == ARG and _size(plain, _blend()) == 0
    cross = _proc(ctx=0x2000, l=77, cc=96)
    assert _fwd(cross, _blend()) == ARG and _size(cross, _blend()) == 0
    ip = _proc(ctx=0x2000, l=77, cc=96, ip=0x4000, wk_ip=0x5000, wv_ip=0x6000, n_ip=5, t_ip=4, ip_mode=_lib.IP_PLAIN, ip_stride=4 * 96)
    assert _fwd(ip, _blend()) == ARG
    assert _fwd(_proc(ip=0x4000), _blend()) == ARG
    assert _fwd(_proc(n_plain=6), _blend()) == ARG and _fwd(_proc(n_plain=-1), _blend()) == ARG
    assert _fwd(_proc(n_plain=5), _blend()) == WORKSPACE and _fwd(_proc(n_plain=0), _blend()) == WORKSPACE
    # everything aid_processor_fwd checks
    assert _fwd(_proc(attn_bias=0x7000), _blend()) == ARG                        # a bias with fused, as today
    assert _fwd(_proc(fused=0, attn_bias=0x7000), _blend()) == WORKSPACE
    assert _fwd(_proc(wq=None), _blend()) == ARG and _fwd(_proc(dtype=5), _blend()) == DTYPE
    assert _fwd(_proc(heads=3), _blend()) == ARG and _fwd(_proc(c=96, heads=2), _blend()) == SHAPE
    # ARG before DTYPE before SHAPE: a misaligned store behind a bad dtype reports the dtype
    assert _fwd(_proc(dtype=5), _blend(k_store_0=0x10008)) == DTYPE
    # the `row` of an entry is ignored (negative here), entries past n_corners are not read
    assert _fwd(_proc(), _blend(2, k_store_2=None, vt_store_5=0x3)) == WORKSPACE


@pytest.mark.parametrize("dtype", [_lib.DTYPE_F16, _lib.DTYPE_F32], ids=["f16", "f32"])
@pytest.mark.parametrize("m", [1, 2, 3, 8])
def test_blend_workspace_holds_the_call_the_pair_table_and_for_outer_the_key_frame_rows(m, dtype):
    lib = _lib.load()
    al = lambda x: (x + 255) // 256 * 256                                         # noqa: E731
    n, s, c, es = 5, 76, 128, 4 if dtype == _lib.DTYPE_F32 else 2
    lp = 80
    table = al(4 * (1 + 2 * ((m + 1) // 2)) * n)
    for q8 in (0, 1):
        for mode in (_lib.MODE_OUTER, _lib.MODE_INNER):
            a = _proc(mode, coef=0x1000, begin=0, end=1, dtype=dtype)
            base = lib.aid_processor_workspace_bytes(C.byref(a))
            got = _size(_proc(mode, dtype=dtype), _blend(m, q8=q8))
            assert base > 0
            if mode == _lib.MODE_INNER:                                           # no extra rows: the mix reads the stores
                assert got == base + table, (m, q8, base, got)
            else:                                                                 # M more rows of k and of V^T, rounded as carve does
                extra = al((n + m) * s * c * es) - al(n * s * c * es) + al((n + m) * c * lp * es) - al(n * c * lp * es)
                assert got == base + table + extra, (m, q8, base, got)
            assert got % 256 == 0
