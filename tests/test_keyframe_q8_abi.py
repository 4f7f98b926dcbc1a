"""Key-frame store in 8-bit blocks (``storage="q8"``): the host side, without a GPU.

``aid_q8_block_bytes`` against the numpy restatement of the format (tests/q8_ref.py), every argument error of the three entry points
with fake pointers and a NULL stream (all checks run before the first launch), the store's accounting on CPU tensors, the Python
layer against a stand-in library, the three kernel instantiations' rows of the build's resource table, and the restatement itself:
the element bound, the error on normal data, ties and the exponent's boundaries."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import q8_ref as R
from aid_amd import _lib, ops
from aid_amd.keyframe_store import SETTINGS_FIELDS, KeyframeStore
from aid_amd.loop import AidDenoiseLoop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "attention-interpolation-diffusion_amd", "csrc")
HEADER = open(os.path.join(ROOT, "include", "aid_hip.h")).read()


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------
def test_block_bytes_equal_the_restatement():
    lib = _lib.load()
    for n in (8, 24, 32, 40, 1320, 1600, 2621440):
        assert lib.aid_q8_block_bytes(n) == R.block_bytes(n) == ops.q8_block_bytes(n) > 0, n
        assert R.block_bytes(n) % 16 == 0 and 0 <= R.block_bytes(n) - (n + -(-n // 32)) < 16
    for n in (0, 4, 12, -8):
        assert lib.aid_q8_block_bytes(n) == R.block_bytes(n) == ops.q8_block_bytes(n) == 0, n
    assert [R.block_bytes(n) for n in (8, 24, 32, 40, 1320)] == [16, 32, 48, 48, 1376]


def test_entry_points_are_declared_exported_and_the_version_stays(tmp_path):
    assert re.search(r"^size_t\s+aid_q8_block_bytes\s*\(int64_t n_elements\)", HEADER, flags=re.M)
    assert re.search(r"^int\s+aid_keyframe_rows_q8\s*\(const AidKeyframeRowsQ8\* args", HEADER, flags=re.M)
    assert re.search(r"^int\s+aid_processor_kf_q8_fwd\s*\(const AidProcessorArgs\* args", HEADER, flags=re.M)
    assert re.search(r"^size_t\s+aid_processor_kf_q8_workspace_bytes\s*\(const AidProcessorArgs\* args", HEADER, flags=re.M)
    new = {"aid_q8_block_bytes", "aid_keyframe_rows_q8", "aid_processor_kf_q8_fwd", "aid_processor_kf_q8_workspace_bytes"}
    lib = _lib.load()
    assert new <= set(_lib.ABI_SYMBOLS) and all(hasattr(lib, s) for s in new)
    assert lib.aid_abi_version() == 10 and _lib.AID_ABI_VERSION == 10 and re.search(r"#define AID_ABI_VERSION 10\b", HEADER)
    # the new struct as gcc lays it out; the structs beside it are the size they were
    cls = _lib.AidKeyframeRowsQ8
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "aid_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(AidKeyframeRowsQ8));']
    lines += [f'  printf("{f} %zu\\n", offsetof(AidKeyframeRowsQ8, {f}));' for f, _ in cls._fields_] + ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = dict(l.split() for l in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(cls) == 72
    for f, _ in cls._fields_:
        assert int(out[f]) == getattr(cls, f).offset, f
    assert C.sizeof(_lib.AidKeyframeRow) == 24 and C.sizeof(_lib.AidKeyframeRows) == 64 and C.sizeof(_lib.AidKeyframeCall) == 32


def _entries(n=3, **kw):
    arr = (_lib.AidKeyframeRow * max(n, 1))()
    rows = [2, 0, 1] + list(range(3, 16))
    for i in range(n):
        arr[i].k_store, arr[i].vt_store, arr[i].row = 0x10000 + 0x1000 * i, 0x20000 + 0x1000 * i, rows[i]
    for k, v in kw.items():
        setattr(arr[n - 1], k, v)
    return arr


def _rows(n=3, entry=None, **kw):
    a = _lib.AidKeyframeRowsQ8()
    arr = _entries(n, **(entry or {}))
    a.k, a.vt, a.rows, a.step = 0x1000, 0x2000, arr, 0x5000
    a.k_fs, a.vt_fs, a.vt_ld, a.vt_cols = 33 * 40, 40 * 40, 40, 33
    a.n_rows, a.n_steps, a.direction, a.dtype = n, 3, _lib.KF_PUT, _lib.DTYPE_F16
    for k, v in kw.items():
        setattr(a, k, v)
    a._keep = arr
    return a


@pytest.mark.parametrize("field,value,code", [
    ("k", None, -1), ("vt", None, -1), ("rows", None, -1), ("step", None, -1), ("step", 0x5002, -1),
    ("n_rows", 0, -1), ("n_rows", 9, -1), ("n_rows", -1, -1), ("n_steps", 0, -1), ("direction", 2, -1), ("direction", -1, -1),
    ("dtype", 3, -2), ("dtype", -1, -2),
    ("k_fs", 33 * 40 + 4, -3), ("vt_fs", 40 * 40 + 4, -3), ("k_fs", 0, -3), ("vt_fs", -8, -3),
    ("k", 0x1008, -3), ("vt", 0x2004, -3),
    ("vt_ld", 36, -3), ("vt_ld", 0, -3), ("vt_ld", -8, -3), ("vt_ld", 48, -3), ("vt_cols", 0, -3), ("vt_cols", 41, -3), ("vt_cols", -1, -3)])
def test_keyframe_rows_q8_argument_errors_return_their_codes_before_any_launch(field, value, code):
    """(vt_ld 36: no multiple of 8; 48: 1600 % 48 != 0.)  A launch with these fake pointers and a NULL stream would fault."""
    lib = _lib.load()
    assert lib.aid_keyframe_rows_q8(None, None) == -1
    a = _rows()
    if field == "rows":
        a.rows = C.POINTER(_lib.AidKeyframeRow)()
    else:
        setattr(a, field, value)
    assert lib.aid_keyframe_rows_q8(C.byref(a), None) == code


@pytest.mark.parametrize("n", [1, 2, 8])
@pytest.mark.parametrize("field,value,code", [("k_store", None, -1), ("vt_store", None, -1), ("row", -1, -1),
                                              ("k_store", 0x10008, -3), ("vt_store", 0x20004, -3)])
def test_keyframe_rows_q8_checks_every_entry(n, field, value, code):
    assert _lib.load().aid_keyframe_rows_q8(C.byref(_rows(n, entry={field: value})), None) == code


def _proc_args(mode=_lib.MODE_PLAIN, n=3):
    a = _lib.AidProcessorArgs()
    for f in ("x", "wq", "wk", "wv", "wo", "y", "coef"):
        setattr(a, f, 0x1000)
    a.n_frames, a.s, a.l, a.c, a.cc, a.heads, a.mode, a.dtype, a.n_ctx = n, 40, 40, 320, 320, 8, mode, _lib.DTYPE_F16, n
    a.begin, a.end = 0, n - 1
    return a


def _call(mode=_lib.KF_RECORD, n=None, entry=None, **kw):
    n = (3 if mode == _lib.KF_RECORD else 2) if n is None else n
    e = _lib.AidKeyframeCall()
    arr = _entries(n, **(entry or {}))
    e.rows, e.step, e.n_rows, e.n_steps, e.mode = arr, 0x5000, n, 3, mode
    for k, v in kw.items():
        setattr(e, k, v)
    e._keep = arr
    return e


def test_processor_kf_q8_refuses_what_processor_kf_refuses_before_its_first_launch():
    """With a NULL workspace a well-formed call gets as far as AID_ERR_WORKSPACE (-4) without a GPU; every malformed one gets the code
    aid_processor_kf_fwd gives it, and the workspace is that entry point's."""
    lib = _lib.load()
    REC, REP = _lib.KF_RECORD, _lib.KF_REPLAY
    plain, aid = _proc_args(), _proc_args(_lib.MODE_OUTER)
    ref = lambda f: (lambda a_, e_: f(C.byref(a_), None if e_ is None else C.byref(e_), None))               # noqa: E731
    fwd, fwd_native = ref(lib.aid_processor_kf_q8_fwd), ref(lib.aid_processor_kf_fwd)
    size = lambda a_, e_: lib.aid_processor_kf_q8_workspace_bytes(C.byref(a_), None if e_ is None else C.byref(e_))   # noqa: E731
    size_native = lambda a_, e_: lib.aid_processor_kf_workspace_bytes(C.byref(a_), None if e_ is None else C.byref(e_))   # noqa: E731
    assert lib.aid_processor_kf_q8_fwd(None, C.byref(_call()), None) == -1 and lib.aid_processor_kf_q8_workspace_bytes(None, None) == 0
    assert fwd(plain, _call()) == -4 and size(plain, _call()) == lib.aid_processor_workspace_bytes(C.byref(plain)) > 0
    assert fwd(aid, _call(REP)) == -4 and size(aid, _call(REP)) == size_native(aid, _call(REP)) > lib.aid_processor_workspace_bytes(C.byref(aid))
    assert fwd(plain, None) == -4 and size(plain, None) == lib.aid_processor_workspace_bytes(C.byref(plain))     # kf == NULL: aid_processor_fwd
    cross = _proc_args()
    cross.ctx, cross.l, cross.cc = 0x1000, 77, 64
    bad_dtype = _proc_args()
    bad_dtype.dtype = 7
    d128 = _proc_args()
    d128.c, d128.heads = 384, 3
    null_rows = _call()
    null_rows.rows = C.POINTER(_lib.AidKeyframeRow)()
    cases = [(aid, _call(REC)), (_proc_args(_lib.MODE_INNER), _call(REC)), (plain, _call(REP)), (plain, _call(0, n=2)), (aid, _call(3, n=2)),
             (_proc_args(n=12), _call(REC, n=0)), (_proc_args(n=12), _call(REC, n=9)), (aid, _call(REP, n=1)), (aid, _call(REP, n=3)),
             (plain, _call(REC, entry={"row": 3})), (plain, _call(REC, entry={"row": -1})), (plain, _call(REC, entry={"row": 0})),
             (plain, null_rows), (plain, _call(step=None)), (plain, _call(step=0x5001)), (plain, _call(n_steps=0)),
             (plain, _call(entry={"k_store": None})), (aid, _call(REP, entry={"vt_store": None})),
             (plain, _call(entry={"k_store": 0x10008})), (aid, _call(REP, entry={"vt_store": 0x20004})),
             (cross, _call()), (bad_dtype, _call()), (d128, _call())]
    seen = set()
    for a, e in cases:
        code = fwd(a, e)
        assert code == fwd_native(a, e) and code in (-1, -2, -3), code
        assert size(a, e) == size_native(a, e) == 0
        seen.add(code)
    assert seen == {-1, -2, -3}
    far = _proc_args(_lib.MODE_OUTER)                                      # REPLAY reads neither begin / end nor the entries' rows
    far.begin = far.end = 99
    assert fwd(far, _call(REP, entry={"row": 99})) == -4


# ---- store accounting on a CPU device -------------------------------------------------------------------------------------------------
DT = torch.float16
SET = dict({f: f"v-{f}" for f in SETTINGS_FIELDS}, num_inference_steps=6)
CPU = torch.device("cpu")
LAYERS = [("down.attn1", 33, 40), ("mid.attn1", 16, 128)]


def _record(st, names, n_steps=3, layers=LAYERS, dtype=DT):
    st.begin_record(names, SET, n_steps, CPU)
    kfs = [st.kf_args(layer, l, c, dtype, CPU) for layer, l, c in layers]
    k = len(names)
    embeds = [(torch.zeros(1, 7, 32, dtype=dtype), torch.zeros(1, 7, 32, dtype=dtype)) for _ in range(k)]
    st.finish_record(torch.zeros(k, 4, 8, 8, dtype=dtype), embeds, torch.ones(k, 4, 8, 8, dtype=dtype))
    return kfs


def _layer_formula(n_steps, l, c):
    lp = (l + 7) // 8 * 8
    return n_steps * (R.block_bytes(l * c) + R.block_bytes(c * lp))


INPUTS = (2 * 4 * 64 + 2 * 7 * 32) * 2                  # latent, final latent and two embeddings of one frame, fp16


def test_layer_bytes_follow_the_formula_and_the_default_is_todays():
    for dtype in (torch.float16, torch.bfloat16, torch.float32):
        es = torch.finfo(dtype).bits // 8
        for l, c in ((33, 40), (16, 128), (4096, 640), (1024, 1280)):
            lp = (l + 7) // 8 * 8
            assert KeyframeStore.layer_bytes(3, l, c, dtype, storage="q8") == _layer_formula(3, l, c)      # whatever the dtype
            assert KeyframeStore.layer_bytes(3, l, c, dtype) == KeyframeStore.layer_bytes(3, l, c, dtype, "native") \
                == KeyframeStore.layer_bytes(3, l, c, dtype, storage="native") == 3 * (l * c + c * lp) * es
    for l, c in ((4096, 640), (1024, 1280)):                                                               # the SDXL shapes
        q8, native = KeyframeStore.layer_bytes(25, l, c, DT, "q8"), KeyframeStore.layer_bytes(25, l, c, DT)
        assert q8 <= 0.52 * native and q8 <= 0.26 * KeyframeStore.layer_bytes(25, l, c, torch.float32)
        assert q8 == 25 * 2 * (l * c * 33 // 32)
    with pytest.raises(ValueError, match="'native' or 'q8'"):
        KeyframeStore.layer_bytes(3, 33, 40, DT, storage="fp8")


def test_a_bad_storage_raises_and_the_storage_is_fixed_for_life():
    for bad in ("fp8", "Q8", None, 8):
        with pytest.raises(ValueError, match="storage must be 'native' or 'q8'"):
            KeyframeStore(storage=bad)
    assert KeyframeStore().storage == "native" and KeyframeStore(storage="native").storage == "native"
    st = KeyframeStore(max_bytes=10, storage="q8")
    assert st.storage == "q8" and st.max_bytes == 10
    with pytest.raises(AttributeError):
        st.storage = "native"
    st.clear()
    assert st.storage == "q8"


def test_nbytes_is_the_sum_of_the_real_sizes_and_kf_args_carries_the_storage():
    st = KeyframeStore(storage="q8")
    st.begin_record(["a", "b", "c"], SET, 3, CPU)
    kf = st.kf_args("down.attn1", 33, 40, DT, CPU)
    assert kf["storage"] == "q8" and kf["mode"] == "record" and [r for _, _, r in kf["entries"]] == [0, 1, 2] and kf["step"] is st.step_tensor
    for k_store, vt_store, _ in kf["entries"]:
        assert k_store.dtype == vt_store.dtype == torch.uint8
        assert tuple(k_store.shape) == (3, R.block_bytes(33 * 40)) and tuple(vt_store.shape) == (3, R.block_bytes(40 * 40))
    assert len({k.data_ptr() for k, _, _ in kf["entries"]}) == 3
    assert st.nbytes == 3 * _layer_formula(3, 33, 40)
    again = st.kf_args("down.attn1", 33, 40, DT, CPU)
    assert all(x[0] is y[0] and x[1] is y[1] for x, y in zip(kf["entries"], again["entries"]))
    with pytest.raises(ValueError, match="another resolution"):
        st.kf_args("down.attn1", 40, 40, DT, CPU)
    st.abort()
    assert st.nbytes == 0
    _record(st, ["a", "b", "c"])
    one = sum(_layer_formula(3, l, c) for _, l, c in LAYERS) + INPUTS
    assert all(st.frame_bytes(n) == one for n in "abc") and st.nbytes == 3 * one
    assert all(st[n].final.dtype == DT and st[n].latent.dtype == DT and st[n].embeds[0].dtype == DT for n in "abc")   # unquantised
    # through the pair too
    pair = st.between("c", "a")
    pair.begin_replay(dict(SET, warmup_ratio=0.5, late="self", early="outer", fusion=True), CPU)
    kf = pair.kf_args("down.attn1", 33, 40, DT, CPU)
    assert kf["storage"] == "q8" and kf["mode"] == "replay" and kf["entries"][0][0] is st["c"].layers["down.attn1"][0]
    pair.abort()
    # the default store: today's numbers, today's dictionary
    nat = KeyframeStore()
    kfs = _record(nat, ["a", "b", "c"])
    assert all(set(kf) == {"entries", "step", "mode"} for kf in kfs)
    native_one = sum(3 * (l * c + c * ((l + 7) // 8 * 8)) * 2 for _, l, c in LAYERS) + INPUTS
    assert nat.nbytes == 3 * native_one and all(nat.frame_bytes(n) == native_one for n in "abc")
    assert all(k.dtype == DT and tuple(k.shape) == (3, 33 * 40) for k, _ in [nat["a"].layers["down.attn1"]])
    # the settings do not carry the storage: a q8 store replays under exactly the settings a native one does
    assert st.settings == nat.settings == SET and "storage" not in SETTINGS_FIELDS


def test_max_bytes_counts_the_q8_sizes_refuses_before_allocating_and_drops_the_refused_recording(monkeypatch):
    one = sum(_layer_formula(3, l, c) for _, l, c in LAYERS) + INPUTS
    st = KeyframeStore(max_bytes=3 * one - 1, storage="q8")
    _record(st, ["a", "b"])                                             # two q8 frames fit where the limit is below two native ones
    assert st.nbytes == 2 * one < 2 * (sum(KeyframeStore.layer_bytes(3, l, c, DT) for _, l, c in LAYERS))
    made = []
    real = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: made.append(a) or real(*a, **k))
    st.begin_record(["c"], SET, 3, CPU)
    st.kf_args(*LAYERS[0], DT, CPU)
    st.kf_args(*LAYERS[1], DT, CPU)
    assert len(made) == 4 and st.nbytes == 3 * one - INPUTS
    emb = [(torch.zeros(1, 7, 32, dtype=DT), torch.zeros(1, 7, 32, dtype=DT))]
    with pytest.raises(ValueError, match=rf"needs {3 * one} bytes, max_bytes is {3 * one - 1}"):
        st.finish_record(torch.zeros(1, 4, 8, 8, dtype=DT), emb, torch.zeros(1, 4, 8, 8, dtype=DT))
    assert st.names == ["a", "b"] and st.nbytes == 2 * one and st.mode is None
    st = KeyframeStore(max_bytes=3 * _layer_formula(3, 33, 40) + _layer_formula(3, 16, 128), storage="q8")
    st.begin_record(["a", "b", "c"], SET, 3, CPU)
    st.kf_args(*LAYERS[0], DT, CPU)
    del made[:]
    with pytest.raises(ValueError, match="max_bytes is"):
        st.kf_args(*LAYERS[1], DT, CPU)                                 # frame a's buffers fit, frame b's do not
    assert len(made) == 2                                               # ... and were not allocated
    assert st.nbytes == 0 and st.names == [] and st.mode is None and st.settings is None


# ---- the Python layer against a recording stand-in ----------------------------------------------------------------------------------
class _Recorder:
    def __init__(self):
        self.calls, self.rows = [], []

    def aid_processor_kf_workspace_bytes(self, ref, kf):
        return 128

    def aid_processor_kf_q8_workspace_bytes(self, ref, kf):
        return 256

    def aid_processor_kf_fwd(self, ref, kf, stream):
        self.calls.append(("native", ref._obj.workspace_bytes, kf._obj.n_rows))
        return 0

    def aid_processor_kf_q8_fwd(self, ref, kf, stream):
        e = kf._obj
        self.calls.append(("q8", ref._obj.workspace_bytes, e.n_rows, e.n_steps, e.mode, [(e.rows[i].k_store, e.rows[i].vt_store, e.rows[i].row)
                                                                                        for i in range(e.n_rows)]))
        return 0

    def aid_keyframe_rows_q8(self, ref, stream):
        a = ref._obj
        self.rows.append(dict(k=a.k, vt=a.vt, k_fs=a.k_fs, vt_fs=a.vt_fs, vt_ld=a.vt_ld, vt_cols=a.vt_cols, n_steps=a.n_steps,
                              direction=a.direction, dtype=a.dtype, entries=[(a.rows[i].k_store, a.rows[i].vt_store, a.rows[i].row)
                                                                             for i in range(a.n_rows)]))
        return 0


@pytest.fixture
def rec(monkeypatch):
    lib = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(ops, "_require_gpu", lambda *ts: torch.device("cpu"))
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "workspace", lambda nbytes, dev: torch.empty(nbytes, dtype=torch.uint8))
    yield lib


def test_processor_kf_fwd_picks_the_entry_point_from_the_storage(rec):
    c, heads, s = 64, 1, 33
    w = [torch.zeros(c, c, dtype=DT) for _ in range(4)]
    x = torch.zeros(3, s, c, dtype=DT)
    q8, nat = KeyframeStore(storage="q8"), KeyframeStore()
    for st in (q8, nat):
        st.begin_record(["a", "b", "c"], SET, 3, CPU)
    kf = q8.kf_args("l0", s, c, DT, CPU)
    ops.processor_kf_fwd(x, *w, None, heads, kf=kf, mode="plain")
    ops.processor_kf_fwd(x, *w, None, heads, kf=nat.kf_args("l0", s, c, DT, CPU), mode="plain")
    assert rec.calls[0] == ("q8", 256, 3, 3, _lib.KF_RECORD, [(k.data_ptr(), v.data_ptr(), i) for i, (k, v, _) in enumerate(kf["entries"])])
    assert rec.calls[1] == ("native", 128, 3)
    # the stores must be what the storage says they are
    with pytest.raises(TypeError, match="store holds"):
        ops.processor_kf_fwd(x, *w, None, heads, kf=dict(kf, storage="native"), mode="plain")
    with pytest.raises(TypeError, match="store holds"):
        ops.processor_kf_fwd(x, *w, None, heads, kf=dict(nat.kf_args("l0", s, c, DT, CPU), storage="q8"), mode="plain")
    with pytest.raises(ValueError, match=rf"k_store \[n_steps, {R.block_bytes(32 * c)}\]"):
        ops.processor_kf_fwd(x[:, :32].contiguous(), *w, None, heads, kf=kf, mode="plain")
    with pytest.raises(ValueError, match="'native' or 'q8'"):
        ops.processor_kf_fwd(x, *w, None, heads, kf=dict(kf, storage="fp8"), mode="plain")
    assert len(rec.calls) == 2


def test_keyframe_rows_q8_hands_the_entries_and_the_stored_columns_over(rec):
    k, vt = torch.zeros(5, 33, 40, dtype=DT), torch.zeros(5, 40, 40, dtype=DT)
    stores = [(torch.zeros(3, R.block_bytes(33 * 40), dtype=torch.uint8), torch.zeros(3, R.block_bytes(40 * 40), dtype=torch.uint8)) for _ in range(3)]
    step = torch.zeros(1, dtype=torch.int32)
    ops.keyframe_rows_q8(k, vt, [(ks, vs, r) for (ks, vs), r in zip(stores, (3, 0, -1))], step, "get", vt_cols=33)
    ops.keyframe_rows_q8(k, vt, [(stores[0][0], stores[0][1], 1)], step, "put")
    assert rec.rows[0]["entries"] == [(ks.data_ptr(), vs.data_ptr(), r) for (ks, vs), r in zip(stores, (3, 0, 4))]
    assert [rec.rows[0][f] for f in ("k", "vt", "k_fs", "vt_fs", "vt_ld", "vt_cols", "n_steps", "direction", "dtype")] == \
        [k.data_ptr(), vt.data_ptr(), 33 * 40, 40 * 40, 40, 33, 3, _lib.KF_GET, _lib.DTYPE_F16]
    assert (rec.rows[1]["vt_cols"], rec.rows[1]["direction"]) == (40, _lib.KF_PUT)          # default: every column is stored
    with pytest.raises(TypeError, match="store holds"):
        ops.keyframe_rows_q8(k, vt, [(torch.zeros(3, 33 * 40, dtype=DT), torch.zeros(3, 40 * 40, dtype=DT), 0)], step, "put")
    with pytest.raises(ValueError, match="1 .. 8"):
        ops.keyframe_rows_q8(k, vt, [], step, "put")
    with pytest.raises(ValueError, match="'put' or 'get'"):
        ops.keyframe_rows_q8(k, vt, [(stores[0][0], stores[0][1], 0)], step, "record")
    assert len(rec.rows) == 2


def test_a_graph_key_that_outlives_a_run_carries_a_q8_stores_storage():
    class _P:
        keyframe_store = None

    class _U:
        attn_processors = {"a": _P(), "b": _P()}

    base = AidDenoiseLoop._graph_key("cond_aid")
    assert AidDenoiseLoop._graph_key("cond_aid", _U()) == base and len(base) == 3           # no store, a native store: today's key
    _U.attn_processors["b"].keyframe_store = KeyframeStore()
    assert AidDenoiseLoop._graph_key("cond_aid", _U()) == base
    _U.attn_processors["b"].keyframe_store = KeyframeStore(storage="q8")
    assert AidDenoiseLoop._graph_key("cond_aid", _U()) == base + ("q8",)


# ---- resources ----------------------------------------------------------------------------------------------------------------------
def test_the_three_instantiations_use_no_scratch_no_spills_no_lds():
    """aid_keyframe_q8.resources.txt at this commit: f32 24 VGPRs, bf16 26, f16 26; no AGPRs, no scratch, no spills, no LDS, 8 waves
    per SIMD."""
    path = os.path.join(CSRC, "aid_keyframe_q8.resources.txt")
    assert os.path.exists(path), f"{path} not there: build the library first (python -c 'import __graft_entry__ as g; g.build()')"
    blocks = open(path).read().split("Name: ")[1:]
    names = [b.split()[0] for b in blocks]
    assert len(blocks) == 3 and all("aid_keyframe_rows_q8_kernel" in n for n in names) and len(set(names)) == 3
    for b in blocks:
        num = lambda key: int(re.search(re.escape(key) + r": (\d+)", b).group(1))   # noqa: E731
        assert num("ScratchSize [bytes/lane]") == 0 and num("VGPRs Spill") == 0 and num("SGPRs Spill") == 0
        assert num("AGPRs") == 0 and num("LDS Size [bytes/block]") == 0
        assert num("VGPRs") <= 32 and num("Occupancy [waves/SIMD]") == 8


# ---- the restatement itself ---------------------------------------------------------------------------------------------------------
def _roundtrip(x, ld=None, cols=None):
    return R.dequantise(R.quantise(x, ld, cols), x.size, ld, cols)


def test_element_bound_and_the_error_on_normal_data():
    rng = np.random.default_rng(7)
    x = rng.standard_normal(131072).astype(np.float32)
    y = _roundtrip(x)
    err = float(np.linalg.norm(y.astype(np.float64) - x) / np.linalg.norm(x.astype(np.float64)))
    print(f"rel-L2 of the q8 round trip on 131072 N(0, 1) samples: {err:.3e}")
    assert err <= 1e-2                                                    # (8.3e-3)
    # |y - x| <= 2^(e-1) < a / 127 ... on data of every block scale, a short last block included
    n = 32 * 4000 + 8
    scale = np.exp2(np.repeat(rng.integers(-100, 100, size=4001), 32)[:n].astype(np.float64))
    x = (rng.standard_normal(n) * scale).astype(np.float32)
    e = R.exponents(x)
    y = _roundtrip(x).astype(np.float64)
    half = np.ldexp(0.5, np.repeat(e, 32)[:x.size])
    assert (np.abs(y - x) <= half).all()
    a = np.abs(np.concatenate([x, np.zeros(24, np.float32)]).reshape(-1, 32)).max(axis=1).astype(np.float64)
    assert (np.ldexp(127.0, e - 1) < a)[a > 0].all() and (np.ldexp(127.0, e) >= a).all()     # e is minimal: 2^(e-1) < a / 127
    for dtype in (torch.float16, torch.bfloat16, torch.float32):         # the value that comes back is exact in every storage dtype
        t = (torch.randn(4096) * 3).to(dtype)
        R.roundtrip_t(t)                                                  # (asserts the exactness)


def test_ties_round_half_to_even_and_pads_are_not_stored():
    x = np.zeros(32, np.float32)
    x[:8] = [0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 127.0, 126.5]
    q, e = R.split(R.quantise(x), 32)
    assert e.tolist() == [0] and q[:8].tolist() == [0, 2, 2, 0, -2, -2, 127, 126]
    # pad columns: int8 0, no part in the maximum, +0 after the round trip — whatever they hold
    x = np.ones(64, np.float32)
    x[np.arange(64) % 8 >= 3] = np.nan
    b = R.quantise(x, 8, 3)
    q, e = R.split(b, 64)
    assert e.tolist() == [-6, -6] and q.reshape(8, 8)[:, :3].tolist() == [[64] * 3] * 8 and (q.reshape(8, 8)[:, 3:] == 0).all()
    x[np.isnan(x)] = 1e30
    assert np.array_equal(R.quantise(x, 8, 3), b)
    y = R.dequantise(b, 64, 8, 3)
    assert (y.reshape(8, 8)[:, :3] == 1).all() and (y.reshape(8, 8)[:, 3:] == 0).all() and not np.signbit(y).any()
    assert R.split(R.quantise(np.zeros(40, np.float32)), 40)[1].tolist() == [-126, -126]                 # a == 0
    assert len(R.quantise(np.zeros(40, np.float32))) == 48 and R.stored_bytes(40) == 42


def test_exponent_boundaries():
    """a = 127 * 2^k gives e = k, the next float above gives e = k + 1; the clamps."""
    for k in (-126, -125, -30, -3, 0, 1, 17, 119, 120):
        a = np.float32(np.ldexp(127.0, k))
        x = np.zeros(32, np.float32)
        x[9] = -a
        assert R.exponents(x).tolist() == [k], k
        q, _ = R.split(R.quantise(x), 32)
        assert q[9] == -127
        x[9] = np.nextafter(a, np.float32(np.inf))
        assert R.exponents(x).tolist() == [min(k + 1, 120)], k
        x[9] = np.nextafter(a, np.float32(0))
        assert R.exponents(x).tolist() == [k], k
    x = np.zeros(32, np.float32)
    x[0] = np.float32(2.0 ** -140)                                        # below 127 * 2^-126: the lower clamp
    assert R.exponents(x).tolist() == [-126]
    # fp16 subnormals m * 2^-24 with |m| <= 127 come back unchanged (e <= -24)
    m = np.arange(-127, 128, 8)[:32].astype(np.float32)
    x = (m * np.float32(2.0 ** -24)).astype(np.float32)
    assert R.exponents(x).tolist() == [-24] and np.array_equal(_roundtrip(x), x)
    assert np.array_equal(_roundtrip(x / 4), x / 4) and R.exponents(x / 4).tolist() == [-26]
