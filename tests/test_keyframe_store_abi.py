"""Key-frame K / V^T store: the host side, without a GPU.

The new structs against the header as gcc lays it out, every argument error of ``aid_keyframe_rows`` / ``aid_processor_kf_fwd`` with a
NULL stream (all checks run before the first launch), ``KeyframeStore`` bookkeeping against a stand-in library that records what the
Python layer hands over, the refusals of the processors, the copy kernel's row of the build's resource table, and the control flow of
``record_keyframes`` / ``interpolate_between`` / ``interpolate_chain`` (both pipeline classes) over a toy denoiser."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import aid_amd
from aid_amd import _lib, ops
from aid_amd.endpoint_store import EndpointStore
from aid_amd.keyframe_store import SETTINGS_FIELDS, KeyframePair, KeyframeStore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "attention-interpolation-diffusion_amd", "csrc")
HEADER = open(os.path.join(ROOT, "include", "aid_hip.h")).read()


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_the_version_stays():
    assert re.search(r"^int\s+aid_keyframe_rows\s*\(const AidKeyframeRows\* args", HEADER, flags=re.M)
    assert re.search(r"^int\s+aid_processor_kf_fwd\s*\(const AidProcessorArgs\* args", HEADER, flags=re.M)
    assert re.search(r"^size_t\s+aid_processor_kf_workspace_bytes\s*\(const AidProcessorArgs\* args", HEADER, flags=re.M)
    new = {"aid_keyframe_rows", "aid_processor_kf_fwd", "aid_processor_kf_workspace_bytes"}
    assert new <= set(_lib.ABI_SYMBOLS)
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in new)
    for name, val in (("AID_KF_MAX_ROWS", _lib.KF_MAX_ROWS), ("AID_KF_PUT", _lib.KF_PUT), ("AID_KF_GET", _lib.KF_GET),
                      ("AID_KF_RECORD", _lib.KF_RECORD), ("AID_KF_REPLAY", _lib.KF_REPLAY)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, HEADER).group(1)) == val
    assert _lib.KF_MAX_ROWS == 8
    assert lib.aid_abi_version() == 10 and _lib.AID_ABI_VERSION == 10 and re.search(r"#define AID_ABI_VERSION 10\b", HEADER)


def test_new_structs_match_the_header_layout(tmp_path):
    structs = {"AidKeyframeRow": _lib.AidKeyframeRow, "AidKeyframeRows": _lib.AidKeyframeRows, "AidKeyframeCall": _lib.AidKeyframeCall,
               "AidProcessorArgs": _lib.AidProcessorArgs, "AidEndpointRows": _lib.AidEndpointRows, "AidEndpointStore": _lib.AidEndpointStore}
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
    # the stores travel beside AidProcessorArgs; the structs of the previous header are the ones they were
    assert [f for f, _ in _lib.AidProcessorArgs._fields_][-1] == "lora_gain_o" and C.sizeof(_lib.AidProcessorArgs) == 440
    assert C.sizeof(_lib.AidEndpointRows) == 80 and C.sizeof(_lib.AidEndpointStore) == 32
    assert C.sizeof(_lib.AidKeyframeRow) == 24 and C.sizeof(_lib.AidKeyframeRows) == 64 and C.sizeof(_lib.AidKeyframeCall) == 32


def _entries(n=3, **kw):
    """A host array of n AidKeyframeRow with distinct, aligned, non-NULL stores and rows (2, 0, 1, 3, ...); ``kw``: field -> value of
    the LAST entry."""
    arr = (_lib.AidKeyframeRow * max(n, 1))()
    rows = [2, 0, 1] + list(range(3, 16))
    for i in range(n):
        arr[i].k_store, arr[i].vt_store, arr[i].row = 0x10000 + 0x1000 * i, 0x20000 + 0x1000 * i, rows[i]
    for k, v in kw.items():
        setattr(arr[n - 1], k, v)
    return arr


def _rows(n=3, entry=None, **kw):
    a = _lib.AidKeyframeRows()
    arr = _entries(n, **(entry or {}))
    a.k, a.vt, a.rows, a.step = 0x1000, 0x2000, arr, 0x5000
    a.k_fs, a.vt_fs, a.n_rows, a.n_steps, a.direction, a.dtype = 33 * 40, 40 * 40, n, 3, _lib.KF_PUT, _lib.DTYPE_F16
    for k, v in kw.items():
        setattr(a, k, v)
    a._keep = arr
    return a


@pytest.mark.parametrize("field,value,code", [
    ("k", None, -1), ("vt", None, -1), ("rows", None, -1), ("step", None, -1), ("step", 0x5002, -1),
    ("n_rows", 0, -1), ("n_rows", 9, -1), ("n_rows", -1, -1), ("n_steps", 0, -1), ("direction", 2, -1), ("direction", -1, -1),
    ("dtype", 3, -2), ("dtype", -1, -2),
    ("k_fs", 33 * 40 + 4, -3), ("vt_fs", 40 * 40 + 4, -3), ("k_fs", 0, -3), ("vt_fs", -8, -3),
    ("k", 0x1008, -3), ("vt", 0x2004, -3)])
def test_keyframe_rows_argument_errors_return_their_codes_before_any_launch(field, value, code):
    lib = _lib.load()
    assert lib.aid_keyframe_rows(None, None) == -1
    a = _rows()
    if field == "rows":
        a.rows = C.POINTER(_lib.AidKeyframeRow)()
    else:
        setattr(a, field, value)
    assert lib.aid_keyframe_rows(C.byref(a), None) == code


@pytest.mark.parametrize("n", [1, 2, 8])
@pytest.mark.parametrize("field,value,code", [("k_store", None, -1), ("vt_store", None, -1), ("row", -1, -1),
                                              ("k_store", 0x10008, -3), ("vt_store", 0x20004, -3)])
def test_keyframe_rows_checks_every_entry(n, field, value, code):
    """The LAST of n entries is the malformed one: every entry is checked, not the first alone."""
    assert _lib.load().aid_keyframe_rows(C.byref(_rows(n, entry={field: value})), None) == code


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


def test_processor_kf_checks_everything_before_its_first_launch():
    """With a NULL workspace a well-formed call gets as far as AID_ERR_WORKSPACE (-4) without a GPU; a malformed one is refused before."""
    lib = _lib.load()
    REC, REP = _lib.KF_RECORD, _lib.KF_REPLAY
    plain, aid = _proc_args(), _proc_args(_lib.MODE_OUTER)
    fwd = lambda a_, e_: lib.aid_processor_kf_fwd(C.byref(a_), None if e_ is None else C.byref(e_), None)      # noqa: E731
    size = lambda a_, e_: lib.aid_processor_kf_workspace_bytes(C.byref(a_), None if e_ is None else C.byref(e_))   # noqa: E731
    base_plain, base_aid = lib.aid_processor_workspace_bytes(C.byref(plain)), lib.aid_processor_workspace_bytes(C.byref(aid))
    assert base_plain > 0 and base_aid > 0
    assert lib.aid_processor_kf_fwd(None, C.byref(_call()), None) == -1 and lib.aid_processor_kf_workspace_bytes(None, None) == 0
    # kf == NULL is aid_processor_fwd: its checks, its workspace
    for a in (plain, aid):
        assert fwd(a, None) == lib.aid_processor_fwd(C.byref(a), None) == -4 and size(a, None) == lib.aid_processor_workspace_bytes(C.byref(a))
    bad = _proc_args()
    bad.wq = None
    assert fwd(bad, None) == lib.aid_processor_fwd(C.byref(bad), None) == -1
    # RECORD: the plain call's workspace, 1 .. 8 entries
    assert fwd(plain, _call()) == -4 and size(plain, _call()) == base_plain
    assert fwd(plain, _call(n=1)) == -4
    assert fwd(_proc_args(n=8), _call(n=8)) == -4
    # REPLAY: what aid_processor_ep_workspace_bytes gives for a replay — two more rows of k and V^T (256-byte aligned regions)
    ep = _lib.AidEndpointStore()
    ep.k_store, ep.vt_store, ep.step, ep.n_steps, ep.mode = 0x3000, 0x4000, 0x5000, 3, _lib.EP_REPLAY
    assert fwd(aid, _call(REP)) == -4
    assert size(aid, _call(REP)) == lib.aid_processor_ep_workspace_bytes(C.byref(aid), C.byref(ep)) > base_aid
    es, s, c, lp, al = 2, 40, 320, 40, lambda x: (x + 255) // 256 * 256
    assert size(aid, _call(REP)) == base_aid - al(3 * s * c * es) - al(3 * c * lp * es) + al(5 * s * c * es) + al(5 * c * lp * es)
    # REPLAY reads neither begin / end nor the entries' rows
    far = _proc_args(_lib.MODE_OUTER)
    far.begin = far.end = 99
    assert fwd(far, _call(REP, entry={"row": 99})) == -4 and fwd(far, _call(REP, entry={"row": -5})) == -4
    # the mode must fit the call kind
    assert fwd(aid, _call(REC)) == -1 and size(aid, _call(REC)) == 0                    # RECORD on an AID call
    assert fwd(_proc_args(_lib.MODE_INNER), _call(REC)) == -1
    assert fwd(plain, _call(REP)) == -1 and size(plain, _call(REP)) == 0                # REPLAY on a PLAIN call
    for a, m in ((plain, 0), (plain, 3), (aid, 0), (aid, 3)):
        assert fwd(a, _call(m, n=2)) == -1 and size(a, _call(m, n=2)) == 0
    # the number of entries
    for n in (0, 9):
        assert fwd(_proc_args(n=12), _call(REC, n=n)) == -1 and size(_proc_args(n=12), _call(REC, n=n)) == 0
    for n in (0, 1, 3, 8):
        assert fwd(aid, _call(REP, n=n)) == -1 and size(aid, _call(REP, n=n)) == 0
    # RECORD: rows distinct and inside the batch
    for row in (3, 99, -1, 0, 2):                                                        # (rows 2 and 0 are entries 0 and 1)
        assert fwd(plain, _call(REC, entry={"row": row})) == -1, row
    assert fwd(plain, _call(REC, n=2, entry={"row": 1})) == -4
    # pointers
    for mode, a in ((REC, plain), (REP, aid)):
        null_rows = _call(mode)
        null_rows.rows = C.POINTER(_lib.AidKeyframeRow)()
        for e in (null_rows, _call(mode, step=None), _call(mode, step=0x5001), _call(mode, n_steps=0), _call(mode, n_steps=-1),
                  _call(mode, entry={"k_store": None}), _call(mode, entry={"vt_store": None})):
            assert fwd(a, e) == -1 and size(a, e) == 0
        for e in (_call(mode, entry={"k_store": 0x10008}), _call(mode, entry={"vt_store": 0x20004})):
            assert fwd(a, e) == -3
        x = _proc_args(a.mode)                                                           # cross-attention takes no store
        x.ctx, x.l, x.cc = 0x1000, 77, 64
        assert lib.aid_processor_fwd(C.byref(x), None) == -4 and fwd(x, _call(mode)) == -1
        x.ip, x.wk_ip, x.wv_ip, x.n_ip, x.t_ip, x.ip_mode, x.ip_stride = 0x1000, 0x1000, 0x1000, 3, 4, 2, 4 * 64     # nor the image branch
        assert fwd(x, _call(mode)) == -1
        f = _proc_args(a.mode)
        f.dtype = 7
        assert fwd(f, _call(mode)) == -2
        f = _proc_args(a.mode)
        f.c, f.heads = 384, 3                                                            # head dim 128
        assert fwd(f, _call(mode)) == -3
        # what aid_processor_fwd accepts beside it is accepted: a mask, LoRA ranks
        m = _proc_args(a.mode)
        m.attn_bias, m.lora_r_q, m.lora_up_q, m.lora_down_x = 0x1000, 64, 0x1000, 0x1000
        assert fwd(m, _call(mode)) == -4
    # the end-point entry point is what it was: it still refuses PLAIN calls
    ep.mode = _lib.EP_RECORD
    assert lib.aid_processor_ep_fwd(C.byref(plain), C.byref(ep), None) == -1


# ---- KeyframeStore bookkeeping ------------------------------------------------------------------------------------------------------
DT = torch.float16
SET = dict({f: f"v-{f}" for f in SETTINGS_FIELDS}, num_inference_steps=6)
CPU = torch.device("cpu")
LAYERS = [("down.attn1", 33, 40), ("mid.attn1", 16, 128)]


def _record(st, names, n_steps=3, settings=SET, layers=LAYERS, dtype=DT):
    """What a recording run does to the store, on CPU tensors: begin, one kf_args per layer, finish."""
    st.begin_record(names, settings, n_steps, CPU)
    for layer, l, c in layers:
        st.kf_args(layer, l, c, dtype, CPU)
    k = len(names)
    embeds = [(torch.zeros(1, 7, 32, dtype=dtype), torch.zeros(1, 7, 32, dtype=dtype)) for _ in range(k)]
    st.finish_record(torch.zeros(k, 4, 8, 8, dtype=dtype), embeds, torch.ones(k, 4, 8, 8, dtype=dtype))


def _frame_bytes(n_steps=3, layers=LAYERS, dtype=DT):
    es = torch.finfo(dtype).bits // 8
    return sum(KeyframeStore.layer_bytes(n_steps, l, c, dtype) for _, l, c in layers) + (2 * 4 * 64 + 2 * 7 * 32) * es


def test_names_frame_bytes_and_nbytes_are_exact_sums():
    assert KeyframeStore.layer_bytes(3, 33, 40, DT) == 3 * (33 * 40 + 40 * 40) * 2 == EndpointStore.layer_bytes(3, 33, 40, DT) // 2
    st = KeyframeStore()
    assert st.nbytes == 0 and st.names == [] and st.mode is None and st.settings is None
    st.begin_record(["a", "b", "c"], SET, 3, CPU)
    kf = st.kf_args("down.attn1", 33, 40, DT, CPU)                   # ragged: round_up(33, 8) = 40 value columns
    assert kf["mode"] == "record" and [r for _, _, r in kf["entries"]] == [0, 1, 2] and kf["step"] is st.step_tensor
    for k_store, vt_store, _ in kf["entries"]:
        assert tuple(k_store.shape) == (3, 33 * 40) and tuple(vt_store.shape) == (3, 40 * 40) and k_store.dtype == DT
    assert len({k.data_ptr() for k, _, _ in kf["entries"]}) == 3       # every key frame has its own allocation
    again = st.kf_args("down.attn1", 33, 40, DT, CPU)
    assert all(x[0] is y[0] and x[1] is y[1] for x, y in zip(kf["entries"], again["entries"]))    # allocated once per layer
    with pytest.raises(ValueError, match="another resolution"):
        st.kf_args("down.attn1", 40, 40, DT, CPU)
    assert st.names == [] and "a" not in st                            # nothing is recorded before the run finishes
    step = st.step_tensor
    assert step.dtype == torch.int32 and step.numel() == 1
    st.set_step(2)
    assert st.step_tensor is step and int(step) == 2
    with pytest.raises(IndexError):
        st.set_step(3)
    st.abort()
    assert st.nbytes == 0 and st.names == [] and st.settings is None and st.mode is None      # an aborted recording leaves nothing
    _record(st, ["a", "b", "c"])
    assert st.names == ["a", "b", "c"] and "b" in st and st.mode is None and st.n_steps == 3 and st.settings == SET
    assert all(st.frame_bytes(n) == _frame_bytes() for n in st.names)
    assert st.nbytes == sum(st.frame_bytes(n) for n in st.names) == 3 * _frame_bytes()
    _record(st, ["d"])                                                 # further frames under the same settings
    assert st.names == ["a", "b", "c", "d"] and st.nbytes == 4 * _frame_bytes()
    st.remove("b")
    assert st.names == ["a", "c", "d"] and st.nbytes == 3 * _frame_bytes()
    with pytest.raises(KeyError, match="'b'"):
        st.remove("b")
    with pytest.raises(KeyError, match="'zz'"):
        st.frame_bytes("zz")
    st.clear()
    assert st.nbytes == 0 and st.names == [] and st.settings is None and st.n_steps == 0


def test_max_bytes_refuses_before_allocation_and_leaves_nothing_of_the_refused_recording(monkeypatch):
    one = _frame_bytes()
    st = KeyframeStore(max_bytes=3 * one - 1)
    _record(st, ["a", "b"])
    made = []
    real = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: made.append(a) or real(*a, **k))
    st.begin_record(["c"], SET, 3, CPU)
    st.kf_args(*LAYERS[0], DT, CPU)
    assert len(made) == 2
    need = 2 * one + sum(KeyframeStore.layer_bytes(3, l, c, DT) for _, l, c in LAYERS)
    st.kf_args(*LAYERS[1], DT, CPU)
    assert len(made) == 4 and st.nbytes == need
    # the inputs and the final latent count too: they cross the limit
    emb = [(torch.zeros(1, 7, 32, dtype=DT), torch.zeros(1, 7, 32, dtype=DT))]
    with pytest.raises(ValueError, match=rf"needs {3 * one} bytes, max_bytes is {3 * one - 1}"):
        st.finish_record(torch.zeros(1, 4, 8, 8, dtype=DT), emb, torch.zeros(1, 4, 8, 8, dtype=DT))
    assert st.names == ["a", "b"] and st.nbytes == 2 * one and st.mode is None          # the earlier frames stay, the refused one is gone
    # a layer buffer that would cross the limit is refused BEFORE it is allocated, whichever frame of the batch it belongs to
    st = KeyframeStore(max_bytes=3 * KeyframeStore.layer_bytes(3, 33, 40, DT) + KeyframeStore.layer_bytes(3, 16, 128, DT))
    st.begin_record(["a", "b", "c"], SET, 3, CPU)
    st.kf_args(*LAYERS[0], DT, CPU)
    del made[:]
    with pytest.raises(ValueError, match="max_bytes is"):
        st.kf_args(*LAYERS[1], DT, CPU)                                # frame a's buffers fit, frame b's do not
    assert len(made) == 2
    assert st.nbytes == 0 and st.names == [] and st.mode is None and st.settings is None
    with pytest.raises(ValueError):
        KeyframeStore(max_bytes=-1)


def test_a_name_is_recorded_once_and_further_frames_need_the_same_settings():
    st = KeyframeStore()
    _record(st, ["a", "b"])
    with pytest.raises(ValueError, match="'a' is already recorded"):
        st.begin_record(["c", "a"], SET, 3, CPU)
    with pytest.raises(ValueError, match="distinct names"):
        st.begin_record(["c", "c"], SET, 3, CPU)
    with pytest.raises(ValueError, match="different guidance_scale"):
        st.begin_record(["c"], dict(SET, guidance_scale=1.0), 3, CPU)
    with pytest.raises(ValueError, match="different aid_steps"):
        st.begin_record(["c"], SET, 2, CPU)
    assert st.mode is None and st.names == ["a", "b"]


def _sig(steps=6, ratio=0.5, late="self", **kw):
    return dict(SET, num_inference_steps=steps, warmup_ratio=ratio, late=late, early="outer", fusion=True, **kw)


def test_replay_checks_the_aid_steps_and_names_each_differing_setting():
    st = KeyframeStore()
    _record(st, ["a", "b", "c"], n_steps=3)
    with pytest.raises(KeyError, match="'x'"):
        st.between("a", "x")
    with pytest.raises(ValueError, match="two different key frames"):
        st.between("a", "a")
    pair = st.between("c", "a")
    assert isinstance(pair, KeyframePair) and pair.recorded and pair.mode is None
    pair.begin_replay(_sig(), CPU)                                      # int(6 * 0.5) = 3 AID steps: recorded
    assert st.mode == pair.mode == "replay"
    kf = pair.kf_args("down.attn1", 33, 40, DT, CPU)
    assert kf["mode"] == "replay" and len(kf["entries"]) == 2
    assert kf["entries"][0][0] is st["c"].layers["down.attn1"][0] and kf["entries"][1][1] is st["a"].layers["down.attn1"][1]
    assert torch.equal(pair.latents, torch.ones(2, 4, 8, 8, dtype=DT))
    with pytest.raises(RuntimeError, match="holds no rows of layer"):
        pair.kf_args("up.attn1", 33, 40, DT, CPU)
    with pytest.raises(RuntimeError, match="in use"):
        st.between("a", "b").begin_replay(_sig(), CPU)
    pair.abort()
    assert st.mode is None and st.names == ["a", "b", "c"]              # a replay leaves the store as it was
    # too many AID steps: a longer warm-up, or a late AID mode (every step)
    for sig in (_sig(ratio=0.7), _sig(late="fused_inner")):
        with pytest.raises(ValueError, match="too few aid_steps"):
            pair.begin_replay(sig, CPU)
        assert st.mode is None
    pair.begin_replay(_sig(ratio=0.4), CPU)                             # fewer AID steps than recorded is fine
    pair.abort()
    # the mode, the fusion flag and the direction are free; each setting is not
    pair.begin_replay(dict(_sig(), early="inner", fusion=False), CPU)
    pair.abort()
    for f in SETTINGS_FIELDS:
        other = _sig()
        other[f] = "something else"
        later = SETTINGS_FIELDS[SETTINGS_FIELDS.index(f) + 1:]
        if later:
            other[later[-1]] = "also different"                         # the FIRST differing setting is the one named
        if f == "num_inference_steps":
            other[f] = 7
        with pytest.raises(ValueError, match=rf"recorded under a different {f}:"):
            pair.begin_replay(other, CPU)
        assert st.mode is None


# ---- the Python layer against a recording stand-in ----------------------------------------------------------------------------------
class _Recorder:
    """Stands in for libaid_hip.so: records what the Python layer hands to aid_processor_kf_fwd / aid_keyframe_rows."""

    def __init__(self):
        self.calls, self.rows, self.plain = [], [], 0

    def aid_processor_workspace_bytes(self, ref):
        return 64

    def aid_processor_kf_workspace_bytes(self, ref, kf):
        return 128

    def aid_processor_fwd(self, ref, stream):
        self.plain += 1
        return 0

    def aid_processor_kf_fwd(self, ref, kf, stream):
        a, e = ref._obj, kf._obj
        self.calls.append(dict(n=a.n_frames, mode=a.mode, ctx=a.ctx, ws=a.workspace_bytes, step=e.step, n_steps=e.n_steps, kf_mode=e.mode,
                               entries=[(e.rows[i].k_store, e.rows[i].vt_store, e.rows[i].row) for i in range(e.n_rows)]))
        return 0

    def aid_keyframe_rows(self, ref, stream):
        a = ref._obj
        self.rows.append(dict(k=a.k, vt=a.vt, k_fs=a.k_fs, vt_fs=a.vt_fs, n_steps=a.n_steps, direction=a.direction, dtype=a.dtype,
                              entries=[(a.rows[i].k_store, a.rows[i].vt_store, a.rows[i].row) for i in range(a.n_rows)]))
        return 0


@pytest.fixture
def rec(monkeypatch):
    lib = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(ops, "_require_gpu", lambda *ts: torch.device("cpu"))
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "workspace", lambda nbytes, dev: torch.empty(nbytes, dtype=torch.uint8))
    yield lib


def test_processor_kf_fwd_hands_the_frames_stores_over(rec):
    st = KeyframeStore()
    c, heads, s = 64, 1, 33
    w = [torch.zeros(c, c, dtype=DT) for _ in range(4)]
    x = torch.zeros(3, s, c, dtype=DT)
    st.begin_record(["a", "b", "c"], SET, 3, CPU)
    kf = st.kf_args("l0", s, c, DT, CPU)
    ops.processor_kf_fwd(x, *w, None, heads, kf=kf, mode="plain")
    (call,) = rec.calls
    assert call["entries"] == [(k.data_ptr(), v.data_ptr(), i) for i, (k, v, _) in enumerate(kf["entries"])]
    assert (call["n_steps"], call["kf_mode"], call["n"], call["mode"], call["ctx"], call["ws"]) == (3, _lib.KF_RECORD, 3, _lib.MODE_PLAIN, None, 128)
    assert call["step"] == st.step_tensor.data_ptr() and rec.plain == 0            # ONE library call per processor call
    coef = torch.tensor([0.5])
    with pytest.raises(ValueError, match="recorded from a plain call"):
        ops.processor_kf_fwd(x, *w, None, heads, kf=kf, mode="outer", coef=coef)
    with pytest.raises(ValueError, match="self-attention"):
        ops.processor_kf_fwd(x, *w, None, heads, kf=kf, mode="plain", kv_cached=(x, x))
    with pytest.raises(ValueError, match="distinct"):
        ops.processor_kf_fwd(x, *w, None, heads, kf=dict(kf, entries=[kf["entries"][0], kf["entries"][0]]), mode="plain")
    with pytest.raises(ValueError, match=r"k_store \[n_steps, 2048\]"):
        ops.processor_kf_fwd(x[:, :32].contiguous(), *w, None, heads, kf=kf, mode="plain")
    with pytest.raises(TypeError, match="store holds"):
        ops.processor_kf_fwd(x.float(), *(t.float() for t in w), None, heads, kf=kf, mode="plain")
    with pytest.raises(ValueError, match="'record' or 'replay'"):
        ops.processor_kf_fwd(x, *w, None, heads, kf=dict(kf, mode="put"), mode="plain")
    with pytest.raises(ValueError, match="not both"):
        ops.processor_fwd(x, None, *w, None, heads, kf=kf, ep=dict(k_store=x, vt_store=x, step=st.step_tensor, mode="record"))
    st.finish_record(torch.zeros(3, 4, 8, 8, dtype=DT), [(torch.zeros(1, 7, 32, dtype=DT),) * 2] * 3, torch.zeros(3, 4, 8, 8, dtype=DT))
    # replay: the pair's two stores in (begin, end) order; the reverse direction swaps them
    for a, b in (("a", "c"), ("c", "a")):
        pair = st.between(a, b)
        pair.begin_replay(_sig(), CPU)
        kf = pair.kf_args("l0", s, c, DT, CPU)
        ops.processor_kf_fwd(x[:1].contiguous(), *w, None, heads, kf=kf, mode="outer", fused=True, coef=coef)
        call = rec.calls[-1]
        assert call["kf_mode"] == _lib.KF_REPLAY and call["n"] == 1 and call["mode"] == _lib.MODE_OUTER
        assert [e[0] for e in call["entries"]] == [st[a].layers["l0"][0].data_ptr(), st[b].layers["l0"][0].data_ptr()]
        with pytest.raises(ValueError, match="interpolated"):
            ops.processor_kf_fwd(x[:1].contiguous(), *w, None, heads, kf=kf, mode="plain")
        with pytest.raises(ValueError, match="exactly two"):
            ops.processor_kf_fwd(x[:1].contiguous(), *w, None, heads, kf=dict(kf, entries=kf["entries"][:1]), mode="outer", coef=coef)
        st.abort()
    assert len(rec.calls) == 3


def test_keyframe_rows_hands_the_entries_over(rec):
    k, vt = torch.zeros(5, 33, 40, dtype=DT), torch.zeros(5, 40, 40, dtype=DT)
    stores = [(torch.zeros(3, 33 * 40, dtype=DT), torch.zeros(3, 40 * 40, dtype=DT)) for _ in range(3)]
    step = torch.zeros(1, dtype=torch.int32)
    ops.keyframe_rows(k, vt, [(ks, vs, r) for (ks, vs), r in zip(stores, (3, 0, -1))], step, "get")
    (call,) = rec.rows
    assert call["entries"] == [(ks.data_ptr(), vs.data_ptr(), r) for (ks, vs), r in zip(stores, (3, 0, 4))]
    assert (call["k"], call["vt"], call["k_fs"], call["vt_fs"], call["n_steps"], call["direction"], call["dtype"]) == \
        (k.data_ptr(), vt.data_ptr(), 33 * 40, 40 * 40, 3, _lib.KF_GET, _lib.DTYPE_F16)
    with pytest.raises(ValueError, match="1 .. 8"):
        ops.keyframe_rows(k, vt, [], step, "put")
    with pytest.raises(ValueError, match="1 .. 8"):
        ops.keyframe_rows(k, vt, [(stores[0][0], stores[0][1], 0)] * 9, step, "put")
    with pytest.raises(ValueError, match="'put' or 'get'"):
        ops.keyframe_rows(k, vt, [(stores[0][0], stores[0][1], 0)], step, "record")
    with pytest.raises(ValueError, match="same number of steps"):
        ops.keyframe_rows(k, vt, [(stores[0][0], stores[0][1], 0), (stores[1][0][:2], stores[1][1][:2], 1)], step, "put")
    with pytest.raises(ValueError, match="ONE int32"):
        ops.keyframe_rows(k, vt, [(stores[0][0], stores[0][1], 0)], torch.zeros(2, dtype=torch.int32), "put")
    assert len(rec.rows) == 1


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _recording_store(names=("a", "b", "c")):
    st = KeyframeStore()
    st.begin_record(list(names), SET, 2, CPU)
    return st


def test_a_store_on_a_cpu_tensor_is_refused_with_the_reason():
    attn = aid_amd.AttnShim(64, 1, None, dtype=DT)
    for cls in (aid_amd.OuterInterpolatedAttnProcessor, aid_amd.InnerInterpolatedAttnProcessor):
        proc = cls(size=3, is_fused=True)
        assert proc.keyframe_store is None                                 # opt-in: absent by default
        proc.keyframe_store = _recording_store()
        proc.activated = False                                             # key frames are recorded by the plain calls
        with pytest.raises(NotImplementedError, match="a key-frame store on a CPU tensor"):
            proc(attn, torch.zeros(3, 16, 64, dtype=DT))
        proc.activated = True
        with pytest.raises(RuntimeError, match="recorded by a plain batch"):
            proc(attn, torch.zeros(3, 16, 64, dtype=DT))


def test_a_store_together_with_the_exchange_is_refused():
    attn = aid_amd.AttnShim(64, 1, None, dtype=DT)
    proc = aid_amd.OuterInterpolatedAttnProcessor(size=3)
    proc.keyframe_store, proc.endpoint_exchange, proc.activated = _recording_store(), object(), False
    with pytest.raises(NotImplementedError, match="a key-frame store together with endpoint_exchange"):
        proc(attn, torch.zeros(3, 16, 64, dtype=DT))


def test_both_kinds_of_store_on_one_processor_are_refused():
    attn = aid_amd.AttnShim(64, 1, None, dtype=DT)
    ep = EndpointStore()
    ep.begin_record({}, 2, CPU)
    proc = aid_amd.OuterInterpolatedAttnProcessor(size=3)
    proc.keyframe_store, proc.endpoint_store = _recording_store(), ep
    for active in (True, False):
        proc.activated = active
        with pytest.raises(NotImplementedError, match="one kind of store"):
            proc(attn, torch.zeros(3, 16, 64, dtype=DT))
    unet = aid_amd.AttnStackUNet("sd15", dtype=DT, scale_down=16)
    aid_amd.load_aid(unet, t=0.5)
    aid_amd.loop.set_endpoint_store(unet, ep)
    st = _recording_store()
    with pytest.raises(RuntimeError, match="not both"):
        aid_amd.loop.set_keyframe_store(unet, st, record=["a", "b", "c"])
    aid_amd.loop.set_endpoint_store(unet, None)
    aid_amd.loop.set_keyframe_store(unet, st, record=["a", "b", "c"])


def test_ip_processors_refuse_a_store(rec):
    attn = aid_amd.AttnShim(64, 1, 32, dtype=DT)
    ip_attn = aid_amd.HipIPAdapterAttnProcessor(hidden_size=64, cross_attention_dim=32, num_tokens=(4,), scale=0.5, dtype=DT)
    for cls in (aid_amd.OuterInterpolatedIPAttnProcessor, aid_amd.InnerInterpolatedIPAttnProcessor, aid_amd.ScaleControlIPAttnProcessor):
        proc = cls(t=0.5, is_fused=True, ip_attn=ip_attn)
        proc.keyframe_store = _recording_store()
        with pytest.raises(NotImplementedError, match="a key-frame store on an IP-Adapter"):
            proc(attn, torch.zeros(3, 16, 64, dtype=DT), encoder_hidden_states=(torch.zeros(3, 7, 32, dtype=DT), [torch.zeros(9, 1, 4, 32, dtype=DT)]))
    assert rec.calls == [] and rec.plain == 0


def test_set_keyframe_store_names_the_layers_and_detaches():
    unet = aid_amd.AttnStackUNet("sd15", dtype=DT, scale_down=16)
    aid_amd.load_aid(unet, t=0.5)
    st = _recording_store()
    with pytest.raises(ValueError, match="record=\\[names\\] or between"):
        aid_amd.loop.set_keyframe_store(unet, st)
    with pytest.raises(ValueError, match="is recording"):
        aid_amd.loop.set_keyframe_store(unet, st, record=["a"])
    with pytest.raises(RuntimeError, match="not in a replay run"):
        aid_amd.loop.set_keyframe_store(unet, st, between=("a", "b"))
    aid_amd.loop.set_keyframe_store(unet, st, record=["a", "b", "c"])
    for name, proc in unet.attn_processors.items():
        assert proc.keyframe_store is st and proc.endpoint_layer == name and proc.endpoint_store is None
    aid_amd.loop.set_keyframe_store(unet, None)
    assert all(p.keyframe_store is None and p.endpoint_layer is None and p.endpoint_ctx is None for p in unet.attn_processors.values())
    st.abort()
    _record(st, ["a", "b"])
    st.between("b", "a").begin_replay(_sig(), CPU)
    ectx = torch.zeros(2, 7, 32)
    with pytest.raises(ValueError, match="is replaying"):
        aid_amd.loop.set_keyframe_store(unet, st, between=("a", "b"), endpoint_ctx=ectx)
    aid_amd.loop.set_keyframe_store(unet, st, between=("b", "a"), endpoint_ctx=ectx, coef=[0.3])
    for name, proc in unet.attn_processors.items():
        assert proc.keyframe_store is st and proc.endpoint_layer == name and proc.endpoint_ctx is ectx
        assert proc.coef.tolist() == pytest.approx([0.3])                # a replay processor holds the interior coefficients only
    aid_amd.loop.set_keyframe_store(unet, None)
    st.abort()


def test_pipeline_methods_refuse_unknown_names_and_changed_settings_before_any_launch():
    hip = aid_amd.StackDenoiser("sd15", dtype=DT, scale_down=16, latent_hw=(8, 8))
    pipe = aid_amd.InterpolationStableDiffusionPipeline(hip, aid_amd.DDIMSchedulerLite())
    pipe.load_aid(t=0.5)
    installed = dict(hip.attn_processors)
    g = torch.Generator().manual_seed(1)
    lat = torch.randn(2, 4, 8, 8, generator=g).to(DT)
    emb = [(torch.randn(1, 7, 768, generator=g),) * 2 for _ in range(2)]
    sched = aid_amd.DDIMSchedulerLite()
    sched.set_timesteps(4, device=CPU)
    from aid_amd.endpoint_store import run_settings
    settings = run_settings(num_inference_steps=4, guidance_scale=7.5, dtype=DT, timesteps=sched.timesteps, unet=hip)
    st = KeyframeStore()
    st.begin_record(["a", "b"], settings, 2, CPU)
    st.finish_record(lat, emb, lat + 1)
    kw = dict(size=5, output_type="latent", use_graphs=False)
    with pytest.raises(KeyError, match="'x'"):
        pipe.interpolate_between(st, "a", "x", **kw)
    with pytest.raises(KeyError, match="'x'"):
        pipe.interpolate_chain(st, ["a", "b", "x"], **kw)
    with pytest.raises(ValueError, match="different num_inference_steps"):
        pipe.interpolate_between(st, "a", "b", num_inference_steps=6, **kw)
    with pytest.raises(ValueError, match="different guidance_scale"):
        pipe.interpolate_between(st, "a", "b", guidance_scale=3.0, **kw)
    with pytest.raises(ValueError, match="too few aid_steps"):
        pipe.interpolate_between(st, "a", "b", warmup_ratio=0.75, **kw)
    with pytest.raises(ValueError, match="too few aid_steps"):
        pipe.interpolate_between(st, "a", "b", late="fused_outer", **kw)
    other = aid_amd.InterpolationStableDiffusionPipeline(aid_amd.StackDenoiser("sd15", dtype=DT, scale_down=16, latent_hw=(8, 8)),
                                                         aid_amd.DDIMSchedulerLite())
    with pytest.raises(ValueError, match="different unet"):
        other.interpolate_between(st, "a", "b", **kw)
    with pytest.raises(ValueError, match="'a' is already recorded"):
        pipe.record_keyframes(st, ["c", "a"], lat, embeds=emb, num_inference_steps=4, output_type="latent", use_graphs=False)
    with pytest.raises(ValueError, match="one entry of embeds per name"):
        pipe.record_keyframes(st, ["c", "d", "e"], torch.cat([lat, lat[:1]]), embeds=emb, num_inference_steps=4, output_type="latent")
    assert st.mode is None and st.names == ["a", "b"]
    assert dict(hip.attn_processors) == installed
    assert all(p.keyframe_store is None and p.endpoint_store is None for p in hip.attn_processors.values())


# ---- resources ----------------------------------------------------------------------------------------------------------------------
def test_copy_kernel_resources_no_scratch_no_spills():
    """aid_keyframe.resources.txt at this commit: 18 VGPRs, 34 SGPRs, no AGPRs, no scratch, no spills, no LDS, 8 waves per SIMD."""
    path = os.path.join(CSRC, "aid_keyframe.resources.txt")
    if not os.path.exists(path):
        pytest.skip(f"{path} not there: build the library first (python -c 'import __graft_entry__ as g; g.build()')")
    blocks = open(path).read().split("Name: ")[1:]
    assert len(blocks) == 1 and "aid_keyframe_rows_kernel" in blocks[0].split()[0]
    num = lambda key: int(re.search(re.escape(key) + r": (\d+)", blocks[0]).group(1))   # noqa: E731
    assert num("ScratchSize [bytes/lane]") == 0 and num("VGPRs Spill") == 0 and num("SGPRs Spill") == 0
    assert num("AGPRs") == 0 and num("LDS Size [bytes/block]") == 0
    assert num("VGPRs") <= 32 and num("Occupancy [waves/SIMD]") == 8


# ---- the pipelines' control flow over a toy denoiser (no attention call: the processors' state alone) --------------------------------
def _toy(xl=False):
    from test_pipelines import RecordingUNet
    unet = RecordingUNet()
    cls = aid_amd.InterpolationStableDiffusionXLPipeline if xl else aid_amd.InterpolationStableDiffusionPipeline
    pipe = cls(unet, aid_amd.DDIMSchedulerLite())
    pipe.load_aid(t=0.5, is_fused=True, atype="fused_outer")
    return unet, pipe


def test_record_keyframes_runs_a_plain_cfg_batch_and_more_than_eight_frames_in_runs_of_eight():
    from test_pipelines import _manual
    unet, pipe = _toy()
    g = torch.Generator().manual_seed(5)
    k, steps = 9, 4
    lat = torch.randn(k, 4, 4, 4, generator=g)
    emb = [(torch.randn(1, 7, 12, generator=g), torch.randn(1, 7, 12, generator=g)) for _ in range(k)]
    names = [f"k{i}" for i in range(k)]
    installed = dict(unet.attn_processors)
    st = KeyframeStore()
    out = pipe.record_keyframes(st, names, lat, embeds=emb, num_inference_steps=steps, guidance_scale=3.0, output_type="latent")
    assert st.names == names and st.n_steps == 2 and st.mode is None and out.shape == (k, 4, 4, 4)
    # every pass is plain; 8 frames in one run, the ninth in another; cond + uncond per step
    assert [c["n"] for c in unet.calls] == [8] * (2 * steps) + [1] * (2 * steps) and not any(c["active"] for c in unet.calls)
    want = _manual(lat, torch.cat([e[0] for e in emb]), torch.cat([e[1] for e in emb]), steps, 0.0, 3.0, aid_amd.DDIMSchedulerLite())
    assert torch.allclose(out, want, atol=1e-5)
    for i, n in enumerate(names):
        f = st[n]
        assert torch.equal(f.final, out[i:i + 1]) and torch.equal(f.latent, lat[i:i + 1]) and len(f.embeds) == 2
        assert torch.equal(f.embeds[0], emb[i][0]) and f.embeds[0] is not emb[i][0]
    assert dict(unet.attn_processors) == installed and all(p.keyframe_store is None for p in installed.values())
    with pytest.raises(ValueError, match="aid_steps must be in 1 .. num_inference_steps"):
        pipe.record_keyframes(st, ["z"], lat[:1], embeds=emb[:1], num_inference_steps=steps, guidance_scale=3.0, aid_steps=5)
    with pytest.raises(ValueError, match="different aid_steps"):
        pipe.record_keyframes(st, ["z"], lat[:1], embeds=emb[:1], num_inference_steps=steps, guidance_scale=3.0, aid_steps=4)
    assert st.names == names and st.mode is None and dict(unet.attn_processors) == installed


@pytest.mark.parametrize("xl", [False, True], ids=["sd", "sdxl"])
def test_between_and_chain_render_the_interior_frames_only_and_take_the_end_frames_from_the_store(xl):
    unet, pipe = _toy(xl)
    g = torch.Generator().manual_seed(6)
    steps, gs = 4, pipe.default_guidance_scale
    lat = torch.randn(3, 4, 4, 4, generator=g)
    mk = lambda: (torch.randn(1, 7, 12, generator=g), torch.randn(1, 7, 12, generator=g)) + \
        ((torch.randn(1, 6, generator=g), torch.randn(1, 6, generator=g)) if xl else ())      # noqa: E731
    emb = [mk() for _ in range(3)]
    st = KeyframeStore()
    pipe.record_keyframes(st, ["a", "b", "c"], lat, embeds=emb, num_inference_steps=steps, output_type="latent")
    assert all(len(st[n].embeds) == (4 if xl else 2) for n in "abc")
    if xl:
        assert all(c["added"] == ["text_embeds", "time_ids"] for c in unet.calls)
    del unet.calls[:]
    kw = dict(size=5, output_type="latent")
    ab = pipe.interpolate_between(st, "a", "b", **kw)
    # batched CFG: the three interior frames and their unconditional riders, AID on for int(4 * 0.5) steps; no end point in the batch
    assert [c["n"] for c in unet.calls] == [6] * steps and [c["active"] for c in unet.calls] == [True, True, False, False]
    assert all(c["coef"].numel() == 3 and c["tail"] == 3 for c in unet.calls[:2])
    assert ab.shape == (5, 4, 4, 4) and torch.equal(ab[0:1], st["a"].final) and torch.equal(ab[4:5], st["b"].final)
    full = pipe.interpolate(lat[0:1], lat[1:2], embeds_start=emb[0], embeds_end=emb[1], num_inference_steps=steps, guidance_scale=gs, **kw)
    assert torch.allclose(ab[1:4], full[1:4], atol=1e-6)              # (the toy denoiser has no attention: the interior frames are the full run's)
    ba = pipe.interpolate_between(st, "b", "a", **kw)
    assert torch.equal(ba[0:1], st["b"].final) and torch.equal(ba[4:5], st["a"].final)
    bc = pipe.interpolate_between(st, "b", "c", **kw)
    chain = pipe.interpolate_chain(st, ["a", "b", "c"], **kw)
    assert chain.shape == (9, 4, 4, 4) and torch.equal(chain, torch.cat([ab, bc[1:]]))
    with pytest.raises(ValueError, match="at least two"):
        pipe.interpolate_chain(st, ["a"], **kw)
    assert st.mode is None and all(p.keyframe_store is None and p.endpoint_ctx is None for p in unet.attn_processors.values())
