"""Tensor-level entry points over the C ABI (device pointers taken from torch tensors).

PyTorch is plumbing here: it owns device memory and the stream; every FLOP is executed by
``libaid_hip.so``.  All functions enqueue on ``torch.cuda.current_stream()`` and never
synchronise.  Tensors must live on a HIP device and be fp16 / bf16 (the fast kernels) or fp32 (the reference's SD1.x storage type,
correctness-first kernels) — anything else raises.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import threading
import weakref
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import (DTYPE_BF16, DTYPE_F16, DTYPE_F32, EP_GET, EP_PUT, EP_RECORD, EP_REPLAY, IP_MAX_SEGMENTS, IP_NONE, IP_PLAIN, IP_SAME,
                   KF_GET, KF_MAX_ROWS, KF_PUT, KF_RECORD, KF_REPLAY, MAX_CORNERS, MODE_INNER, MODE_OUTER, MODE_PLAIN,
                   AidAttnArgs, AidCorners, AidEndpointRows, AidEndpointStore, AidGemmProblem, AidIpAttnArgs, AidIpSegment, AidKeyframeBlend, AidKeyframeCall,
                   AidKeyframeRow, AidKeyframeRows, AidKeyframeRowsQ8, AidProcessorArgs)

MODES = {"plain": MODE_PLAIN, "inner": MODE_INNER, "outer": MODE_OUTER}
IP_MODES = {"same": IP_SAME, "plain": IP_PLAIN}
EP_MODES = {"record": EP_RECORD, "replay": EP_REPLAY}
EP_DIRECTIONS = {"put": EP_PUT, "get": EP_GET}
KF_MODES = {"record": KF_RECORD, "replay": KF_REPLAY}
KF_DIRECTIONS = {"put": KF_PUT, "get": KF_GET}
KF_STORAGES = ("native", "q8")
SUPPORTED_HEAD_DIMS = (40, 64, 80, 160)


def _dtype_code(t: torch.Tensor) -> int:
    if t.dtype == torch.float16:
        return DTYPE_F16
    if t.dtype == torch.bfloat16:
        return DTYPE_BF16
    if t.dtype == torch.float32:        # the reference's SD1.x default (gradio_src/app.py:62): fp32 tensors, fp32 matrix-pipe arithmetic
        return DTYPE_F32
    raise TypeError(f"the HIP path computes in float16 / bfloat16 / float32; got {t.dtype}")


def _require_16bit(t: torch.Tensor, what: str) -> None:
    if t.dtype == torch.float32:
        raise TypeError(f"{what} is implemented for float16 / bfloat16 storage (the float32 path covers the projections, the attention "
                        "core and the processor call; run the LayerNorm in torch there)")


def _require_gpu(*ts: Optional[torch.Tensor]) -> torch.device:
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("attention-interpolation-diffusion_amd has no CPU path: tensors must be on "
                               f"an MI355X (HIP) device, got device={t.device}")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"tensors on different devices: {dev} vs {t.device}")
    return dev


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


@contextlib.contextmanager
def _on(dev: Optional[torch.device]):
    """Make the tensors' device the current one for the launch: the library enqueues on the CURRENT device's stream and
    keeps its per-kernel attributes per device, so a process that drives several GPUs (or calls with tensors of a
    non-current device) must not launch on the wrong device's stream."""
    if dev is None or dev.index is None or dev.index == torch.cuda.current_device():
        yield
    else:
        with torch.cuda.device(dev):
            yield


def executed_segments(mode: str, fused: bool, coef_vals: Optional[Sequence[float]], n_frames: int,
                      own_rows: Optional[Sequence[int]] = None, begin: int = 0, end: int = -1) -> int:
    """(frame, key segment) passes the attention kernel really runs for one launch — the bookkeeping behind
    ``AidProfileEntry.flops_executed`` (csrc/aid_attn.hip): a PLAIN rider (negative coefficient) and a fused END-POINT
    frame take one pass over their own keys; a coefficient of exactly 0 / 1 drops the zero-weighted side of OUTER."""
    if mode == "plain" or coef_vals is None:
        return n_frames
    own = list(range(n_frames)) if own_rows is None else list(own_rows)
    n_rows = max(own) + 1
    begin, end = begin % n_rows, end % n_rows
    total = 0
    for i in range(n_frames):
        c = coef_vals[i]
        if c < 0 or (fused and ((c == 0 and own[i] == begin) or (c == 1 and own[i] == end))):
            total += 1
        elif mode == "inner":
            total += 2 if fused else 1
        else:
            total += (1 if fused else 0) + (1 if c != 1 else 0) + (1 if c != 0 else 0)
    return total


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


# ---- float32 matmul precision -----------------------------------------------------------------------------------------------
# torch.set_float32_matmul_precision: "highest" = exact fp32 products (the default), "high" = every float32 number taken as the sum of
# two bfloat16 numbers, three bf16 products (AidGemmProblem.f32_split, csrc/aid_f32x3.hip).  "medium" only PERMITS less precision than
# "high"; it runs the same split.  This setting covers the PROJECTIONS of float32 tensors; 16-bit tensors never carry the field.
# The attention core's two products (K Q'^T, V^T P^T) have their own, package-level switch below (set_f32_attn_precision), which does
# NOT follow the torch global: it defaults to "highest" (exact fp32 products, aid_attn_f32_kernel) and "high" permits the same split in
# the core (AidAttnArgs.f32_split / AidProcessorArgs.f32_attn_split, aid_attn_f32x3_kernel).
F32_PRECISIONS = {"highest": 0, "high": 1, "medium": 1}
F32_ATTN_PRECISIONS = {"highest": 0, "high": 1}
_f32_attn_precision = "highest"


def f32_split_code(f32_precision: Optional[str] = None) -> int:
    """AidGemmProblem.f32_split of a float32 launch: ``None`` reads ``torch.get_float32_matmul_precision()`` now."""
    if f32_precision is None:
        f32_precision = torch.get_float32_matmul_precision()
    try:
        return F32_PRECISIONS[f32_precision]
    except (KeyError, TypeError):
        raise ValueError(f"f32_precision must be None, 'highest', 'high' or 'medium'; got {f32_precision!r}") from None


def set_f32_attn_precision(value: str) -> None:
    """Package-level precision of the float32 attention core's two products: "highest" (exact, the default) or "high" (the core may
    form them from bf16 halves).  Independent of ``torch.set_float32_matmul_precision``; read at every call."""
    global _f32_attn_precision
    if not isinstance(value, str) or value not in F32_ATTN_PRECISIONS:
        raise ValueError(f"f32 attention precision must be 'highest' or 'high'; got {value!r}")
    _f32_attn_precision = value


def get_f32_attn_precision() -> str:
    return _f32_attn_precision


def f32_attn_split_code(value: Optional[str] = None) -> int:
    """AidAttnArgs.f32_split / AidProcessorArgs.f32_attn_split of a float32 launch: ``None`` reads the package setting now."""
    if value is None:
        value = _f32_attn_precision
    try:
        return F32_ATTN_PRECISIONS[value]
    except (KeyError, TypeError):
        raise ValueError(f"f32_attn_precision must be None, 'highest' or 'high'; got {value!r}") from None


# ---- scratch memory --------------------------------------------------------------------------------------------------------
# One workspace per (device, stream): kernels on one stream run in order, so reuse is safe.  Stream captures get their OWN workspace,
# keyed by the capture's id (aid_stream_capture_id) and never handed to eager calls or to another capture, even when torch recycles the
# stream handle — a captured graph keeps the address for as long as it can be replayed.  Who keeps the memory alive:
#   * captures of THIS package (``_PassGraphs``, ``AidDenoiseLoop``) run under a ``WorkspaceOwner``: the capture ADOPTS the workspace
#     the eager warm-up on the capture stream left behind (nothing is allocated inside the capture), the owner records the key and
#     drops it when the object that holds the graphs is released or garbage-collected (the adopted workspaces used to
#     live for the life of the process, ~150 MB per captured SDXL pass kind);
#   * a FOREIGN capture (``with torch.cuda.graph(g): unet(...)`` around processor calls) allocates its workspace inside the capture,
#     i.e. from the graph's private pool: the memory belongs to the graph and goes when the graph goes.  The dictionary entry of a
#     finished foreign capture is dropped at the next call on that stream.  (A capture torch's allocator does not know about
#     cannot allocate: it adopts the workspace of an eager warm-up on the capture stream — kept for the life of the process — or
#     gets a RuntimeError that asks for that warm-up.)
_eager_ws: Dict[Tuple[int, int], torch.Tensor] = {}
_capture_ws: Dict[Tuple[int, int, int], torch.Tensor] = {}
_pool_keys: set = set()                      # keys of _capture_ws whose tensor lives in a foreign graph's private pool
_ws_tls = threading.local()


def _drop_capture_keys(keys: set) -> None:
    for k in list(keys):
        _capture_ws.pop(k, None)
    keys.clear()


class WorkspaceOwner:
    """Ties the capture workspaces adopted inside ``with owner:`` blocks to the life of the object that holds the captured graphs:
    ``release()`` — or the garbage collection of the owner — drops them.  Release only when the graphs are gone."""

    def __init__(self):
        self._keys: set = set()
        self._fin = weakref.finalize(self, _drop_capture_keys, self._keys)

    def __enter__(self):
        stack = getattr(_ws_tls, "owners", None)
        if stack is None:
            stack = _ws_tls.owners = []
        stack.append(self)
        return self

    def __exit__(self, *exc):
        _ws_tls.owners.pop()
        return False

    def release(self) -> None:
        _drop_capture_keys(self._keys)

    def __len__(self) -> int:
        return len(self._keys)


def _current_owner() -> Optional[WorkspaceOwner]:
    stack = getattr(_ws_tls, "owners", None)
    return stack[-1] if stack else None


def _capture_id(stream: int) -> int:
    cid = C.c_ulonglong(0)
    _lib.check(_lib.load().aid_stream_capture_id(stream, C.byref(cid)), "aid_stream_capture_id")
    return int(cid.value)


def workspace(nbytes: int, device: torch.device) -> torch.Tensor:
    """Scratch buffer of at least ``nbytes`` for a library call on the current stream of ``device`` (policy above)."""
    dev = device.index if device.index is not None else torch.cuda.current_device()
    stream = _stream()
    cid = _capture_id(stream) if torch.cuda.is_current_stream_capturing() else 0
    for k in [k for k in _pool_keys if k[0] == dev and k[1] == stream and k[2] != cid]:
        _pool_keys.discard(k)                                   # a foreign capture on this stream has ended: its pool owns the memory
        _capture_ws.pop(k, None)
    if cid:
        key = (dev, stream, cid)
        ws = _capture_ws.get(key)
        if ws is not None and ws.numel() >= nbytes:
            return ws
        owner = _current_owner()
        if owner is None and (ws is None or key in _pool_keys):  # foreign capture: the graph's private pool owns its workspace
            # (a later, larger request of the same capture allocates again; the smaller block goes back to that pool, stream-ordered)
            try:
                ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
                _capture_ws[key] = ws
                _pool_keys.add(key)
                return ws
            except RuntimeError:                                # a capture torch's allocator does not know about
                ws = None
        if ws is None:
            ws = _eager_ws.pop((dev, stream), None)             # adopt: eager calls on this stream allocate afresh from now on
            if ws is not None:
                _capture_ws[key] = ws
                if owner is not None:
                    owner._keys.add(key)
        if ws is None or ws.numel() < nbytes:
            raise RuntimeError(
                f"a library call inside a stream capture needs {nbytes} bytes of workspace on a stream that has "
                f"{'none' if ws is None else str(ws.numel()) + ' bytes'}: run the same calls once EAGERLY on the capture stream first "
                "(torch.cuda.graph(g, stream=s) after a warm-up under torch.cuda.stream(s)) — the capture then adopts the warm-up's "
                "workspace")
        return ws
    key = (dev, stream)
    ws = _eager_ws.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _eager_ws[key] = ws
    return ws


def release_workspaces() -> None:
    """Drop every cached workspace (also the ones captured graphs still point into: call it when those graphs are gone)."""
    _eager_ws.clear()
    _capture_ws.clear()
    _pool_keys.clear()


# ---- per-call hint: launch streams that share the device ---------------------------------------------------------------------
_tls = threading.local()


@contextlib.contextmanager
def cu_share(n: int):
    """Inside the block every library call of THIS host thread carries ``cu_share = n`` (AidGemmProblem / AidProcessorArgs, ABI v7):
    n independent launch streams run side by side — the conditional and the unconditional UNet call of a step on two streams — so
    a launch plans with 1 / n of the CUs.  A hint: results never depend on it.  Thread-local: two host threads driving two GPUs (or
    two streams) can hold different values at the same time."""
    n = int(n)
    if not 0 <= n <= 8:
        raise ValueError("cu_share must be in 0 .. 8")
    prev = getattr(_tls, "cu_share", 0)
    _tls.cu_share = n
    try:
        yield
    finally:
        _tls.cu_share = prev


def current_cu_share() -> int:
    return int(getattr(_tls, "cu_share", 0))


# ---------------------------------------------------------------------------------------------
def gemm_nt(problems: Sequence[dict]) -> None:
    """Grouped C = A @ B^T (+ bias) (+ residual, added after the rounding).  Each problem: dict(a=[.., m, k],
    b=[n, k] or [batch, n, k], c=out tensor, bias=None|[n], residual=None|like c, batch=1, m, n, k, lda, ldb, ldc,
    stride_a, stride_b, stride_c[, f32_precision=None|"highest"|"high"|"medium": float32 operands only, ``f32_split_code``])."""
    lib = _lib.load()
    n = len(problems)
    arr = (AidGemmProblem * n)()
    dt = None
    for i, p in enumerate(problems):
        _require_gpu(p["a"], p["b"], p["c"], p.get("bias"), p.get("residual"))
        code = _dtype_code(p["a"])
        if dt is None:
            dt = code
        if code != dt or _dtype_code(p["b"]) != dt or _dtype_code(p["c"]) != dt:
            raise TypeError("all GEMM operands must share one dtype")
        q = arr[i]
        q.a, q.b, q.c = p["a"].data_ptr(), p["b"].data_ptr(), p["c"].data_ptr()
        q.bias = _ptr(p.get("bias"))
        q.residual = _ptr(p.get("residual"))
        q.m, q.n, q.k = p["m"], p["n"], p["k"]
        q.lda, q.ldb, q.ldc = p["lda"], p["ldb"], p["ldc"]
        q.batch = p.get("batch", 1)
        q.scale = float(p.get("scale", 0.0))            # 0 = 1 (zero-initialised structs)
        q.stride_a, q.stride_b, q.stride_c = p.get("stride_a", 0), p.get("stride_b", 0), p.get("stride_c", 0)
        q.trans_rows = int(p.get("trans_rows", 0))      # C transposed per frame of that many rows (aid_hip.h)
        q.cu_share = current_cu_share()
        split = f32_split_code(p.get("f32_precision"))      # (a bad value raises whatever the dtype)
        if dt == DTYPE_F32:
            q.f32_split = split
        if p.get("ln_stats") is not None:       # folded LayerNorm: dict(ln_stats=, ln_colsum=, ln_shift=, ln_side=1|2[, stride_stats=])
            for t_ in (p["ln_stats"], p["ln_colsum"], p["ln_shift"]):
                _require_gpu(t_)
                if t_.dtype != torch.float32 or not t_.is_contiguous():
                    raise TypeError("ln_stats / ln_colsum / ln_shift are contiguous float32 tensors")
            q.ln_stats, q.ln_colsum, q.ln_shift = p["ln_stats"].data_ptr(), p["ln_colsum"].data_ptr(), p["ln_shift"].data_ptr()
            q.ln_side, q.stride_stats = int(p["ln_side"]), int(p.get("stride_stats", 0))
        lr = p.get("lr")
        if lr is not None:      # low-rank second K segment: dict(a=LA [m, k], b=LB [n, k], k=, lda=, ldb=[, stride_a=, stride_b=]
            #                     [, row_scale=fp32 gain of the weight rows (DoRA), scale_side=2 (indexed by n, default) | 1 (by m)])
            _require_gpu(lr["a"], lr["b"])
            if _dtype_code(lr["a"]) != dt or _dtype_code(lr["b"]) != dt:
                raise TypeError("the low-rank operands must have the GEMM's dtype")
            q.lr_a, q.lr_b = lr["a"].data_ptr(), lr["b"].data_ptr()
            q.lr_k, q.lr_lda, q.lr_ldb = int(lr["k"]), int(lr["lda"]), int(lr["ldb"])
            q.lr_stride_a, q.lr_stride_b = int(lr.get("stride_a", 0)), int(lr.get("stride_b", 0))
            rs = lr.get("row_scale")
            if rs is not None:
                _require_gpu(rs)
                side = int(lr.get("scale_side", 2))
                if rs.dtype != torch.float32 or rs.stride(-1) != 1 or rs.numel() != (q.m if side == 1 else q.n):
                    raise TypeError("row_scale is a float32 vector with one entry per weight row (n for scale_side 2, m for 1)")
                q.lr_row_scale, q.lr_scale_side = rs.data_ptr(), side
    with _on(problems[0]["a"].device):
        _lib.check(lib.aid_gemm_nt(arr, n, dt, _stream()), "aid_gemm_nt")


def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None,
           out: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
           f32_precision: Optional[str] = None) -> torch.Tensor:
    """y = x @ w.T + bias (+ residual) on the HIP GEMM (x [..., k] contiguous, w [n, k] contiguous).  ``f32_precision``: float32
    tensors only, None = ``torch.get_float32_matmul_precision()`` (``f32_split_code``)."""
    assert x.is_contiguous() and w.is_contiguous()
    k = x.shape[-1]
    n = w.shape[0]
    m = x.numel() // k
    if out is None:
        out = torch.empty(*x.shape[:-1], n, dtype=x.dtype, device=x.device)
    if residual is not None and (residual.shape != out.shape or residual.dtype != out.dtype or not residual.is_contiguous()):
        raise ValueError("residual must be a contiguous tensor shaped like the output")
    gemm_nt([dict(a=x, b=w, c=out, bias=bias, residual=residual, m=m, n=n, k=k, lda=k, ldb=k, ldc=n, f32_precision=f32_precision)])
    return out


def layernorm(x: torch.Tensor, gamma: Optional[torch.Tensor] = None, beta: Optional[torch.Tensor] = None,
              eps: float = 1e-5, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """LayerNorm over the last dimension on the HIP kernel (fp32 statistics, one rounding)."""
    _require_gpu(x, gamma, beta, out)
    _require_16bit(x, "layernorm")
    if not x.is_contiguous():
        raise ValueError("operands must be contiguous")
    for t_ in (gamma, beta):
        if t_ is not None and (t_.dtype != x.dtype or t_.numel() != x.shape[-1] or not t_.is_contiguous()):
            raise ValueError("gamma / beta must be contiguous [c] tensors of the activation dtype")
    if out is None:
        out = torch.empty_like(x)
    c = x.shape[-1]
    with _on(x.device):
        _lib.check(_lib.load().aid_layernorm(x.data_ptr(), _ptr(gamma), _ptr(beta), out.data_ptr(), x.numel() // c, c,
                                             float(eps), _dtype_code(x), _stream()), "aid_layernorm")
    return out


def ln_stats(x: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """(mean, rstd) per row of x over the last dimension, fp32 [rows, 2] — what the folded LayerNorm needs of x."""
    _require_gpu(x)
    _require_16bit(x, "ln_stats")
    if not x.is_contiguous():
        raise ValueError("operands must be contiguous")
    c = x.shape[-1]
    st = torch.empty(x.numel() // c, 2, dtype=torch.float32, device=x.device)
    with _on(x.device):
        _lib.check(_lib.load().aid_ln_stats(x.data_ptr(), st.data_ptr(), x.numel() // c, c, float(eps), _dtype_code(x),
                                            _stream()), "aid_ln_stats")
    return st


def ln_fold(w: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor]):
    """Fold a LayerNorm's affine part into the Linear that consumes it: returns (w * gamma in the storage dtype,
    colsum fp32 [rows], shift fp32 [rows]) — see AidGemmProblem.ln_* in include/aid_hip.h."""
    _require_gpu(w, gamma, beta)
    _require_16bit(w, "ln_fold")
    if w.ndim != 2 or not w.is_contiguous():
        raise ValueError("w must be a contiguous [rows, c] weight")
    for t_ in (gamma, beta):
        if t_ is not None and (t_.dtype != w.dtype or t_.numel() != w.shape[1] or not t_.is_contiguous()):
            raise ValueError("gamma / beta must be contiguous [c] tensors of the weight dtype")
    wf = torch.empty_like(w)
    cs = torch.empty(w.shape[0], dtype=torch.float32, device=w.device)
    sh = torch.empty_like(cs)
    with _on(w.device):
        _lib.check(_lib.load().aid_ln_fold(w.data_ptr(), _ptr(gamma), _ptr(beta), wf.data_ptr(), cs.data_ptr(), sh.data_ptr(),
                                           w.shape[0], w.shape[1], _dtype_code(w), _stream()), "aid_ln_fold")
    return wf, cs, sh


def dora_gain(w: torch.Tensor, a_pack: torch.Tensor, b_pack: torch.Tensor, magnitude: torch.Tensor) -> torch.Tensor:
    """Row gain of a DoRA adapter (``aid_dora_gain``): ``magnitude / ||W + B_pack A_pack||_row`` as float32 [out].  ``w`` [out, in]
    (rows may be strided), ``a_pack`` [R, in] with the scaling folded in and ``b_pack`` [out, R] as ``lora.pack`` builds them,
    ``magnitude`` [out]; all of one dtype (float16 / bfloat16 / float32)."""
    dev = _require_gpu(w, a_pack, b_pack, magnitude)
    dt = _dtype_code(w)
    if any(t_.dtype != w.dtype for t_ in (a_pack, b_pack, magnitude)):
        raise TypeError("w, a_pack, b_pack and magnitude must share one dtype")
    n_out, n_in = w.shape
    rank = a_pack.shape[0]
    if w.ndim != 2 or w.stride(1) != 1 or tuple(a_pack.shape) != (rank, n_in) or tuple(b_pack.shape) != (n_out, rank) \
            or magnitude.numel() != n_out or not (a_pack.is_contiguous() and b_pack.is_contiguous() and magnitude.is_contiguous()):
        raise ValueError("dora_gain takes w [out, in], a_pack [R, in], b_pack [out, R], magnitude [out] (packs and magnitude contiguous)")
    gain = torch.empty(n_out, dtype=torch.float32, device=w.device)
    with _on(dev):
        _lib.check(_lib.load().aid_dora_gain(w.data_ptr(), a_pack.data_ptr(), b_pack.data_ptr(), magnitude.data_ptr(), gain.data_ptr(),
                                             n_out, n_in, w.stride(0) if n_out > 1 else n_in, rank, dt, _stream()), "aid_dora_gain")
    return gain


def _sample_layout(t: torch.Tensor, what: str) -> Tuple[int, int, int]:
    """(n, e, sample stride in elements) of ``t`` [n, ...] whose samples are contiguous blocks of e elements (dim 0 may be strided)."""
    if t.ndim < 2:
        raise ValueError(f"{what} must be [n, ...] (one sample per row of dim 0); got shape {tuple(t.shape)}")
    n = t.shape[0]
    e = t.numel() // n if n else int(torch.Size(t.shape[1:]).numel())
    expect = 1
    for size, stride in zip(reversed(t.shape[1:]), reversed(t.stride()[1:])):
        if size != 1 and stride != expect:
            raise ValueError(f"{what}: the elements of a sample must be contiguous (shape {tuple(t.shape)}, strides {t.stride()})")
        expect *= size
    return n, e, (t.stride(0) if n > 1 else e)


def cfg_rescale(text: torch.Tensor, uncond: torch.Tensor, guidance_scale: float, guidance_rescale: float,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Classifier-free guidance with guidance rescale in one launch (``aid_cfg_rescale``; pipeline_interpolated_sd.py:92-108,
    1892-1902): per sample ``c = uncond + gs (text - uncond)``, ``out = c (rescale std(text) / std(c) + 1 - rescale)``, fp32 arithmetic,
    one rounding.  ``text`` / ``uncond`` / ``out`` [n, ...] of one shape and dtype (float16 / bfloat16 / float32); dim 0 may be strided
    (the two halves of a batched ``[2 n, ...]`` UNet output are passed as views, no copy), the elements of a sample are contiguous.
    ``out`` may be ``text`` or ``uncond`` itself; it is allocated when None.  Enqueues on the current stream: capturable."""
    dev = _require_gpu(text, uncond, out)
    dt = _dtype_code(text)
    if out is None:
        out = torch.empty(text.shape, dtype=text.dtype, device=text.device)
    if uncond.shape != text.shape or out.shape != text.shape or uncond.dtype != text.dtype or out.dtype != text.dtype:
        raise ValueError("cfg_rescale takes text, uncond and out of one shape and dtype")
    n, e, ts = _sample_layout(text, "text")
    _, _, us = _sample_layout(uncond, "uncond")
    _, _, os_ = _sample_layout(out, "out")
    if n == 0:
        return out
    with _on(dev):
        _lib.check(_lib.load().aid_cfg_rescale(text.data_ptr(), uncond.data_ptr(), out.data_ptr(), n, e, ts, us, os_,
                                               float(guidance_scale), float(guidance_rescale), dt, _stream()), "aid_cfg_rescale")
    return out


def project_kv(e: torch.Tensor, wk: torch.Tensor, wv: torch.Tensor, extra_rows: int = 0,
               lora_k: Optional[Tuple[torch.Tensor, ...]] = None,
               lora_v: Optional[Tuple[torch.Tensor, ...]] = None,
               f32_precision: Optional[str] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """k = e @ wk.T  [F, L, C]  and  V^T = wv @ e^T  [F, C, Lp]  (Lp = L rounded up to 8) in one launch.
    ``extra_rows``: allocate that many more (uninitialised) frame rows behind the F projected ones — room for the
    end-point frames' keys / values a rank receives from their owners (dist.EndpointExchange).
    ``lora_k`` / ``lora_v`` = (A_pack, B_pack[, gain]) (lora.pack): the adapters' terms are added in the same accumulators; e is
    projected down once, U = e [A_k; A_v]^T, in one launch before.  ``gain`` (DoRA, fp32 [C] or None) multiplies the accumulator.
    ``f32_precision``: float32 tensors only, None = ``torch.get_float32_matmul_precision()`` (``f32_split_code``)."""
    f, l, cc = e.shape
    c = wk.shape[0]
    lp = (l + 7) // 8 * 8
    k = torch.empty(f + extra_rows, l, c, dtype=e.dtype, device=e.device)
    vt = torch.empty(f + extra_rows, c, lp, dtype=e.dtype, device=e.device)
    u = None
    gk = lora_k[2] if lora_k is not None and len(lora_k) > 2 else None
    gv = lora_v[2] if lora_v is not None and len(lora_v) > 2 else None
    rk = lora_k[0].shape[0] if lora_k is not None else 0
    rv = lora_v[0].shape[0] if lora_v is not None else 0
    if rk + rv:
        down = torch.cat([p[0] for p in (lora_k, lora_v) if p is not None], 0) if rk and rv else (lora_k or lora_v)[0]
        u = torch.empty(f * l, rk + rv, dtype=e.dtype, device=e.device)
        gemm_nt([dict(a=e, b=down, c=u, m=f * l, n=rk + rv, k=cc, lda=cc, ldb=cc, ldc=rk + rv, f32_precision=f32_precision)])
    if l % 8 == 0:          # flat value projection, transposed epilogue (tile count of the key projection: whole CU rounds)
        pv = dict(a=e, b=wv, c=vt, m=f * l, n=c, k=cc, lda=cc, ldb=cc, ldc=lp, stride_c=c * lp, trans_rows=l)
        if rv:
            pv["lr"] = dict(a=u[:, rk:], b=lora_v[1], k=rv, lda=rk + rv, ldb=rv, row_scale=gv, scale_side=2)
    else:                   # V^T[f] = Wv E_f^T, one batch entry per frame.  Pad columns l .. round_up(l, 4) of V^T are written with
        #                     zeros (aid_hip.h); round_up(l, 4) .. lp are not written, and the attention kernels do not read their values
        pv = dict(a=wv, b=e, c=vt, m=c, n=l, k=cc, lda=cc, ldb=cc, ldc=lp, batch=f, stride_a=0, stride_b=l * cc, stride_c=c * lp)
        if rv:
            pv["lr"] = dict(a=lora_v[1], b=u[:, rk:], k=rv, lda=rv, ldb=rk + rv, stride_b=l * (rk + rv), row_scale=gv, scale_side=1)
    pk = dict(a=e, b=wk, c=k, m=f * l, n=c, k=cc, lda=cc, ldb=cc, ldc=c)
    if rk:
        pk["lr"] = dict(a=u, b=lora_k[1], k=rk, lda=rk + rv, ldb=rk, row_scale=gk, scale_side=2)
    pk["f32_precision"] = pv["f32_precision"] = f32_precision
    gemm_nt([pk, pv])
    return k, vt


def score_bias_layout(bias: torch.Tensor, n: int, heads: int, s: int, l: int, dtype: torch.dtype) -> Tuple[int, int, int]:
    """(frame stride, head stride, row stride) in elements of an additive score bias (AidAttnArgs.bias, ABI v8) given as diffusers
    hands it around: ``[N * H, 1 | S, L]`` (``Attention.prepare_attention_mask``), ``[N, 1 | S, L]`` or ``[N, 1 | H, 1 | S, L]``."""
    if bias.dtype != dtype:
        raise TypeError(f"the score bias must have the activation dtype ({dtype}), got {bias.dtype}")
    if bias.ndim == 3:
        b0, r, ll = bias.shape
        if b0 == n * heads and heads > 1:
            fs, hs = heads * bias.stride(0), bias.stride(0)
        elif b0 == n:
            fs, hs = bias.stride(0), 0
        else:
            raise ValueError(f"score bias of {b0} rows for {n} frames x {heads} heads")
        rs = bias.stride(1)
    elif bias.ndim == 4:
        b0, hx, r, ll = bias.shape
        if b0 != n or hx not in (1, heads):
            raise ValueError(f"score bias must be [N, 1 | H, 1 | S, L]; got {tuple(bias.shape)} for N = {n}, H = {heads}")
        fs, hs, rs = bias.stride(0), (bias.stride(1) if hx > 1 else 0), bias.stride(2)
    else:
        raise ValueError("score bias must be a 3-D or 4-D tensor")
    if ll != l or r not in (1, s) or (ll > 1 and bias.stride(-1) != 1):
        raise ValueError(f"score bias must be [..., 1 | {s}, {l}] with contiguous rows; got {tuple(bias.shape)}")
    return int(fs), int(hs), int(rs if r > 1 else 0)


def attn_fwd(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, heads: int, *, l: int,
             mode: str = "plain", fused: bool = False, coef: Optional[torch.Tensor] = None,
             begin: int = 0, end: int = -1, out: Optional[torch.Tensor] = None,
             accumulate: bool = False, out_scale: float = 1.0,
             frame_scale: Optional[torch.Tensor] = None, kv_map: Optional[torch.Tensor] = None,
             softmax_scale: Optional[float] = None, n_plain: int = 0, seg_executed: int = 0,
             q_prescaled: bool = False, bias: Optional[torch.Tensor] = None,
             f32_attn_precision: Optional[str] = None) -> torch.Tensor:
    """Interpolated attention core (see AidAttnArgs in include/aid_hip.h).
    q [N, S, C], k [F, L, C], vt [F, C, Lp] contiguous; coef / frame_scale fp32 device [N].  ``bias``: additive score bias
    (diffusers' prepared attention_mask, ``score_bias_layout``); not with ``fused``.
    ``f32_attn_precision``: float32 tensors only — the precision of the two products (AidAttnArgs.f32_split), None = the package
    setting at call time (``f32_attn_split_code``)."""
    lib = _lib.load()
    attn_split = f32_attn_split_code(f32_attn_precision)    # (a bad value raises whatever the dtype)
    _require_gpu(q, k, vt, out, coef, frame_scale, kv_map, bias)
    dt = _dtype_code(q)
    if _dtype_code(k) != dt or _dtype_code(vt) != dt:
        raise TypeError("q, k, vt must share one dtype")
    assert q.is_contiguous() and k.is_contiguous() and vt.is_contiguous()
    n, s, c = q.shape
    f = k.shape[0]
    d = c // heads
    if out is None:
        if accumulate:
            raise ValueError("accumulate=True needs an existing `out`")
        out = torch.empty_like(q)
    for t_, nm in ((coef, "coef"), (frame_scale, "frame_scale")):
        if t_ is not None and (t_.dtype != torch.float32 or t_.numel() != n):
            raise ValueError(f"{nm} must be a float32 device tensor with one entry per frame ({n})")
    if kv_map is not None and (kv_map.dtype != torch.int32 or kv_map.numel() != n):
        raise ValueError("kv_map must be an int32 device tensor with one entry per frame")
    a = AidAttnArgs()
    a.q, a.k, a.vt, a.out = q.data_ptr(), k.data_ptr(), vt.data_ptr(), out.data_ptr()
    a.coef, a.frame_scale, a.kv_map = _ptr(coef), _ptr(frame_scale), _ptr(kv_map)
    if mode == "inner":
        # interpolated K / V^T of the interior frames (one streaming launch), read by the attention kernel
        if kv_map is not None or f < n:
            raise ValueError("inner mode needs one key/value row per frame (no kv_map)")
        k2, vt2 = torch.empty_like(k[:n]), torch.empty_like(vt[:n])
        with _on(q.device):
            _lib.check(lib.aid_lerp_kv(k.data_ptr(), vt.data_ptr(), k2.data_ptr(), vt2.data_ptr(), coef.data_ptr(), n,
                                       begin % f, end % f, k.shape[1] * k.shape[2], vt.shape[1] * vt.shape[2], dt,
                                       _stream()), "aid_lerp_kv")
        a.k2, a.vt2 = k2.data_ptr(), vt2.data_ptr()
    a.n_frames, a.n_kv = n, f
    a.s, a.l, a.heads, a.d = s, l, heads, d
    a.ldq, a.ldk, a.ldvt, a.ldo = c, k.shape[2], vt.shape[2], out.shape[2]
    a.q_fs, a.k_fs, a.vt_fs, a.o_fs = s * c, k.shape[1] * k.shape[2], vt.shape[1] * vt.shape[2], s * out.shape[2]
    a.mode, a.fused = MODES[mode], int(bool(fused))
    a.begin, a.end = begin % f, end % f
    a.accumulate, a.dtype = int(bool(accumulate)), dt
    a.softmax_scale = float(d ** -0.5 if softmax_scale is None else softmax_scale)
    a.out_scale = float(out_scale)
    a.n_plain = int(n_plain)
    a.seg_executed = int(seg_executed)
    if bias is not None:
        a.bias = bias.data_ptr()
        a.bias_fs, a.bias_hs, a.bias_rs = score_bias_layout(bias, n, heads, s, l, q.dtype)
    a.q_prescaled = int(bool(q_prescaled))              # q already holds q * softmax_scale * log2(e) (the processor path's q projection)
    if dt == DTYPE_F32:
        a.f32_split = attn_split
    with _on(q.device):
        _lib.check(lib.aid_attn_fwd(C.byref(a), _stream()), "aid_attn_fwd")
    return out


def _ip_segment_array(segments: Sequence[dict], n: int, s: int, c: int, dtype: torch.dtype):
    """The host array of AidIpSegment for ``segments`` (checked against a [n, s, c] query tensor of ``dtype``)."""
    if dtype == torch.float32:
        raise NotImplementedError("several IP-Adapters per layer / ip_adapter_masks (the image-segment form) are implemented for "
                                  "float16 / bfloat16 storage; float32 storage runs one unmasked adapter per layer")
    arr = (AidIpSegment * len(segments))()
    for g, seg in enumerate(segments):
        k, vt, rw = seg["k"], seg["vt"], seg.get("row_weight")
        _require_gpu(k, vt, rw)
        if k.dtype != dtype or vt.dtype != dtype:
            raise TypeError(f"image keys / values must have the activation dtype ({dtype})")
        if k.ndim != 3 or vt.ndim != 3 or not k.is_contiguous() or not vt.is_contiguous():
            raise ValueError("an image segment is (k [R, T, C], vt [R, C, Tp]) as project_kv returns them")
        rows, t = k.shape[0], k.shape[1]
        if rows not in (1, n) or vt.shape[0] != rows or k.shape[2] != c or vt.shape[1] != c or t < 1 or vt.shape[2] < t or vt.shape[2] % 8:
            raise ValueError(f"image segment {g}: k {tuple(k.shape)} / vt {tuple(vt.shape)} do not fit {n} frames of width {c} with t = {t}")
        if rw is not None and (rw.dtype != torch.float32 or rw.numel() != s or not rw.is_contiguous()):
            raise ValueError(f"image segment {g}: row_weight must be a contiguous float32 tensor with one entry per query row ({s})")
        e = arr[g]
        e.k, e.vt, e.row_weight = k.data_ptr(), vt.data_ptr(), _ptr(rw)
        e.k_fs, e.vt_fs = k.shape[1] * k.shape[2], vt.shape[1] * vt.shape[2]
        e.t, e.ldvt, e.n_rows = t, vt.shape[2], rows
        e.scale = float(seg.get("scale", 1.0))
    return arr


def ip_attn_accumulate(q: torch.Tensor, out: torch.Tensor, segments: Sequence[dict], heads: int, *,
                       softmax_scale: Optional[float] = None, q_prescaled: bool = False) -> torch.Tensor:
    """``out += sum_g scale_g * w_g[row] * softmax(q K_g^T * softmax_scale) V_g`` over image-key segments, one launch per
    ``IP_MAX_SEGMENTS`` segments (``aid_ip_attn_fwd``; fp32 accumulation, one rounding per launch).  q / out [N, S, C] contiguous,
    float16 / bfloat16; a segment is dict(k=[R, T, C], vt=[R, C, Tp] (``project_kv``; R = N or 1 = shared by all frames), scale=float,
    row_weight=None | float32 [S])."""
    lib = _lib.load()
    dev = _require_gpu(q, out)
    if q.dtype != out.dtype or q.shape != out.shape or q.ndim != 3 or not q.is_contiguous() or not out.is_contiguous():
        raise ValueError("q and out must be contiguous [N, S, C] tensors of one dtype")
    n, s, c = q.shape
    if heads < 1 or c % heads:
        raise ValueError(f"{c} channels do not split into {heads} heads")
    segments = list(segments)
    arr = _ip_segment_array(segments, n, s, c, q.dtype)
    d = c // heads
    base = C.addressof(arr) if len(segments) else 0
    for g0 in range(0, len(segments), IP_MAX_SEGMENTS):
        a = AidIpAttnArgs()
        a.q, a.out = q.data_ptr(), out.data_ptr()
        a.segments = base + g0 * C.sizeof(AidIpSegment)
        a.n_segments = min(IP_MAX_SEGMENTS, len(segments) - g0)
        a.n_frames, a.s, a.heads, a.d = n, s, heads, d
        a.ldq, a.ldo, a.q_fs, a.o_fs = c, c, s * c, s * c
        a.dtype = _dtype_code(q)
        a.softmax_scale = float(d ** -0.5 if softmax_scale is None else softmax_scale)
        a.q_prescaled = int(bool(q_prescaled))
        with _on(dev):
            _lib.check(lib.aid_ip_attn_fwd(C.byref(a), _stream()), "aid_ip_attn_fwd")
    return out


def set_tuning(name: str, value: int = -1) -> None:
    """Development knob of the library (``aid_set_tuning``): ``value < 0`` hands the choice back to the launch heuristics."""
    _lib.check(_lib.load().aid_set_tuning(name.encode(), int(value)), f"aid_set_tuning({name})")


def get_tuning(name: str) -> int:
    """Current value of a development knob (``aid_get_tuning``); -1 = the launch heuristics decide."""
    import ctypes
    v = ctypes.c_int(0)
    _lib.check(_lib.load().aid_get_tuning(name.encode(), ctypes.byref(v)), f"aid_get_tuning({name})")
    return int(v.value)


def last_attn_variant() -> str:
    return _lib.load().aid_last_attn_variant().decode()


def last_gemm_variant() -> str:
    return _lib.load().aid_last_gemm_variant().decode()


def processor_fwd(x: torch.Tensor, ctx: Optional[torch.Tensor], wq: torch.Tensor, wk: torch.Tensor,
                  wv: torch.Tensor, wo: torch.Tensor, bo: Optional[torch.Tensor], heads: int, *,
                  mode: str = "plain", fused: bool = False, coef: Optional[torch.Tensor] = None,
                  begin: int = 0, end: int = -1, ctx_map: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None, n_plain: int = 0,
                  ln: Optional[Tuple[Optional[torch.Tensor], Optional[torch.Tensor], float]] = None,
                  residual: Optional[torch.Tensor] = None, seg_executed: int = 0,
                  ip: Optional[dict] = None, ln_folded: Optional[tuple] = None,
                  kv_cached: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                  attn_bias: Optional[torch.Tensor] = None, lora=None, f32_precision: Optional[str] = None,
                  f32_attn_precision: Optional[str] = None, ip_segments: Optional[Sequence[dict]] = None,
                  ep: Optional[dict] = None, kf: Optional[dict] = None, corners: Optional[dict] = None) -> torch.Tensor:
    """One whole processor call: y = to_out(AID-attention(to_q(x), to_k(ctx), to_v(ctx)))
    in three launches (grouped q/k/V^T GEMM, attention core, out-proj GEMM).
    ``ln = (gamma, beta, eps)`` computes on LayerNorm(x); ``residual`` is added to the result (the transformer
    block's norm in front of the call and its residual add after it).
    ``ip`` = the IP-Adapter image branch (AidProcessorArgs.ip_*): dict(tokens=[R, T, Cc] tensor whose rows may be a
    strided view, wk=to_k_ip weight, wv=to_v_ip weight, mode="same"|"plain", scale=float, map=int32 device [N] or None,
    frame_scale=fp32 device [N] or None, begin=int, end=int).
    ``ln_folded`` = (wq', wk', wv', const) with ``ln``: the LayerNorm is folded into the projections (wq' etc. from
    ``ln_fold``, wk' / wv' None for cross-attention, const fp32 [6, C] = colsum_q, shift_q, colsum_k, shift_k, colsum_v,
    shift_v): only the row statistics of x are computed, LayerNorm(x) is never written.
    ``kv_cached`` = (k, vt) from ``project_kv(ctx, wk, wv)``: the step-invariant keys / values of a cross-attention layer,
    projected once by the caller; the call then projects the queries only.
    ``attn_bias``: additive score bias of the (text) attention — diffusers' prepared attention_mask (AidProcessorArgs.attn_bias,
    ``score_bias_layout``); the library refuses it together with ``fused`` or ``ip`` (the reference fails there, aid_hip.h).
    ``lora``: unmerged LoRA adapters of the four projections (``lora.LoraArgs``, AidProcessorArgs.lora_*): each projection with a
    rank computes  in W^T + round(in A_pack^T) B_pack^T  in its GEMM accumulator; refused with ``ln_folded`` and, on k / v, with
    ``kv_cached`` (the cached keys must already hold the adapter term).  ``lora.gains`` (DoRA, AidProcessorArgs.lora_gain_*): the
    fp32 row gain of each projection's adapter, or None.
    ``f32_precision``: float32 tensors only — the precision of every projection GEMM of the call (AidProcessorArgs.f32_split), None =
    ``torch.get_float32_matmul_precision()`` at call time.
    ``f32_attn_precision``: float32 tensors only — the precision of the attention core's two products in every attention launch of
    the call (AidProcessorArgs.f32_attn_split), None = the package setting at call time (``f32_attn_split_code``).
    ``ip_segments``: image-key segments (``ip_attn_accumulate``'s dicts; ``aid_processor_ip_fwd``) added to the attention output in
    one launch after the text attention — several IP-Adapters per layer, regional masks as ``row_weight``.  A cross-attention
    ``mode="plain"`` call without ``ip``, float16 / bfloat16; ``attn_bias`` is allowed and covers the text scores only.
    ``ep``: the end-point store of the layer, see ``processor_ep_fwd``.  ``kf``: key-frame stores of the layer, see
    ``processor_kf_fwd`` (one of the two at most; ``kf["mode"] == "blend"``: the corners of a corner-weighted call are recorded key
    frames, see ``processor_kf_blend_fwd``).  ``corners``: a corner-weighted call, see ``processor_corners_fwd`` (no store, no
    image branch; ``coef`` / ``begin`` / ``end`` are not read)."""
    lib = _lib.load()
    split = f32_split_code(f32_precision)
    attn_split = f32_attn_split_code(f32_attn_precision)
    ipt = ip or {}
    dev = _require_gpu(x, ctx, wq, wk, wv, wo, bo, coef, ctx_map, out, residual, attn_bias, *(ln[:2] if ln else ()),
                       ipt.get("tokens"), ipt.get("wk"), ipt.get("wv"), ipt.get("map"), ipt.get("frame_scale"))
    dt = _dtype_code(x)
    for t_ in (ctx, wq, wk, wv, wo, bo):
        if t_ is not None and t_.dtype != x.dtype:
            raise TypeError(f"dtype mismatch: hidden states are {x.dtype}, another operand is {t_.dtype}")
    for t_ in (x, ctx, wq, wk, wv, wo, bo):
        if t_ is not None and not t_.is_contiguous():
            raise ValueError("operands must be contiguous")
    n, s, c = x.shape
    if out is None:
        out = torch.empty_like(x)
    a = AidProcessorArgs()
    a.x, a.ctx = x.data_ptr(), _ptr(ctx)
    a.wq, a.wk, a.wv, a.wo, a.bo = wq.data_ptr(), wk.data_ptr(), wv.data_ptr(), wo.data_ptr(), _ptr(bo)
    a.y, a.coef, a.ctx_map = out.data_ptr(), _ptr(coef), _ptr(ctx_map)
    a.n_frames, a.s, a.c, a.heads = n, s, c, heads
    if ctx is not None:
        a.n_ctx, a.l, a.cc = ctx.shape
    else:
        a.n_ctx, a.l, a.cc = n, s, c
    nkv = a.n_ctx
    a.mode, a.fused = MODES[mode], int(bool(fused))
    a.begin, a.end = begin % nkv, end % nkv
    a.dtype = dt
    a.n_plain = int(n_plain)
    a.seg_executed = int(seg_executed)
    if ip is not None:
        tok = ip["tokens"]
        if ctx is None:
            raise ValueError("the image branch belongs to a cross-attention call (encoder_hidden_states = (text, [ip]))")
        if tok.ndim != 3 or tok.shape[2] != ctx.shape[2] or tok.dtype != x.dtype or tok.stride(2) != 1 \
                or tok.stride(1) != tok.shape[2]:
            raise ValueError("image tokens must be [rows, T, Cc] in the activation dtype with contiguous [T, Cc] rows")
        for t_ in (ip["wk"], ip["wv"]):
            if t_.dtype != x.dtype or not t_.is_contiguous() or tuple(t_.shape) != (c, ctx.shape[2]):
                raise ValueError("to_k_ip / to_v_ip weights must be contiguous [C, Cc] tensors of the activation dtype")
        a.ip, a.wk_ip, a.wv_ip = tok.data_ptr(), ip["wk"].data_ptr(), ip["wv"].data_ptr()
        a.ip_map, a.ip_frame_scale = _ptr(ip.get("map")), _ptr(ip.get("frame_scale"))
        a.n_ip, a.t_ip = tok.shape[0], tok.shape[1]
        a.ip_stride = tok.stride(0) if tok.shape[0] > 1 else tok.shape[1] * tok.shape[2]
        a.ip_mode, a.ip_scale = IP_MODES[ip["mode"]], float(ip.get("scale", 1.0))
        a.ip_begin, a.ip_end = int(ip.get("begin", 0)) % a.n_ip, int(ip.get("end", -1)) % a.n_ip
    if ln is not None:
        _require_16bit(x, "the LayerNorm fusion of processor_fwd")
        g_, b_, eps = ln
        if not eps > 0:
            raise ValueError("LayerNorm eps must be > 0")
        for t_ in (g_, b_):
            if t_ is not None and (t_.dtype != x.dtype or t_.numel() != c or not t_.is_contiguous()):
                raise ValueError("LayerNorm gamma / beta must be contiguous [c] tensors of the activation dtype")
        a.ln_gamma, a.ln_beta, a.ln_eps = _ptr(g_), _ptr(b_), float(eps)
        if ln_folded is not None:
            fq, fk, fv, cst = ln_folded
            _require_gpu(fq, fk, fv, cst)
            if cst.dtype != torch.float32 or tuple(cst.shape) != (6, c) or not cst.is_contiguous():
                raise ValueError("ln_folded constants must be a contiguous float32 [6, C] tensor")
            for t_, ref in ((fq, wq), (fk, wk), (fv, wv)):
                if t_ is not None and (t_.dtype != x.dtype or t_.shape != ref.shape or not t_.is_contiguous()):
                    raise ValueError("folded weights must look like the weights they replace")
            if ctx is None and (fk is None or fv is None):
                raise ValueError("self-attention needs the folded to_k / to_v weights too")
            a.ln_wq, a.ln_wk, a.ln_wv, a.ln_const = fq.data_ptr(), _ptr(fk), _ptr(fv), cst.data_ptr()
    elif ln_folded is not None:
        raise ValueError("ln_folded goes with ln=(gamma, beta, eps)")
    if residual is not None:
        if residual.shape != x.shape or residual.dtype != x.dtype or not residual.is_contiguous():
            raise ValueError("residual must be a contiguous tensor shaped like the hidden states")
        a.residual = residual.data_ptr()
    if kv_cached is not None:
        if ctx is None:
            raise ValueError("cached keys / values belong to a cross-attention call")
        kc, vc = kv_cached
        _require_gpu(kc, vc)
        lp = (ctx.shape[1] + 7) // 8 * 8
        ok = kc.dtype == x.dtype and vc.dtype == x.dtype and kc.is_contiguous() and vc.is_contiguous() \
            and kc.shape[0] >= ctx.shape[0] and vc.shape[0] >= ctx.shape[0] \
            and tuple(kc.shape[1:]) == (ctx.shape[1], c) and tuple(vc.shape[1:]) == (c, lp)
        if not ok:
            raise ValueError("kv_cached must be (k [n_ctx, L, C], vt [n_ctx, C, round_up(L, 8)]) as project_kv returns them")
        a.k_cached, a.vt_cached = kc.data_ptr(), vc.data_ptr()
    if attn_bias is not None:
        a.attn_bias = attn_bias.data_ptr()
        a.attn_bias_fs, a.attn_bias_hs, a.attn_bias_rs = score_bias_layout(attn_bias, n, heads, s, a.l, x.dtype)
    if lora is not None:
        for t_ in (lora.down_x, lora.down_ctx, lora.down_o, *lora.up):
            if t_ is not None:
                _require_gpu(t_)
                if t_.dtype != x.dtype or not t_.is_contiguous():
                    raise ValueError("LoRA packs must be contiguous tensors of the activation dtype")
        a.lora_down_x, a.lora_down_ctx, a.lora_down_o = _ptr(lora.down_x), _ptr(lora.down_ctx), _ptr(lora.down_o)
        a.lora_up_q, a.lora_up_k, a.lora_up_v, a.lora_up_o = (_ptr(t_) for t_ in lora.up)
        a.lora_r_q, a.lora_r_k, a.lora_r_v, a.lora_r_o = lora.ranks
        gains = tuple(getattr(lora, "gains", None) or (None,) * 4)
        for t_, r_ in zip(gains, lora.ranks):
            if t_ is not None:
                _require_gpu(t_)
                if t_.dtype != torch.float32 or not t_.is_contiguous() or t_.numel() != c or not r_:
                    raise ValueError("DoRA gains are contiguous float32 [C] tensors of projections that have a rank")
        a.lora_gain_q, a.lora_gain_k, a.lora_gain_v, a.lora_gain_o = (_ptr(t_) for t_ in gains)
    seg_arr = None
    if ip_segments:
        if ctx is None or mode != "plain" or ip is not None:
            raise ValueError("ip_segments belong to a cross-attention mode='plain' call without the `ip` branch")
        seg_arr = _ip_segment_array(list(ip_segments), n, s, c, x.dtype)
    a.cu_share = current_cu_share()
    if dt == DTYPE_F32:
        a.f32_split = split
        a.f32_attn_split = attn_split
    est = kcall = ccall = None
    if ep is not None and kf is not None:
        raise ValueError("a call takes an end-point store (ep=) or key-frame stores (kf=), not both")
    if corners is not None:
        if ep is not None or kf is not None or ip is not None or seg_arr is not None:
            raise ValueError("a corner-weighted call takes no store and no image branch")
        if mode == "plain":
            raise ValueError("a corner-weighted call is an interpolated (inner / outer) call")
        ccall, _c_rows = _corners_args(corners, n, nkv)                   # (_c_rows: the host array ccall points at, kept alive)
        nbytes = lib.aid_processor_corners_workspace_bytes(C.byref(a), C.byref(ccall))
    elif ep is not None:
        if seg_arr is not None:
            raise ValueError("an end-point store belongs to a self-attention call: no ip_segments")
        est = _endpoint_store_args(ep, s, c, x.dtype)
        nbytes = lib.aid_processor_ep_workspace_bytes(C.byref(a), C.byref(est))
    elif kf is not None and kf.get("mode") == "blend":               # the corners of the call are recorded key frames
        if seg_arr is not None or ip is not None or ctx is not None:
            raise ValueError("key-frame stores belong to a self-attention call: no context, no image branch")
        if mode == "plain":
            raise ValueError("a key-frame blend is an interpolated (inner / outer) call")
        kcall, _kf_rows = _keyframe_blend_args(kf, n, s, c, x.dtype)
        kf_size, kf_fwd, kf_name = lib.aid_processor_kf_blend_workspace_bytes, lib.aid_processor_kf_blend_fwd, "aid_processor_kf_blend_fwd"
        nbytes = kf_size(C.byref(a), C.byref(kcall))
    elif kf is not None:
        if seg_arr is not None:
            raise ValueError("key-frame stores belong to a self-attention call: no ip_segments")
        kcall, _kf_rows = _keyframe_call_args(kf, n, s, c, x.dtype)          # (_kf_rows: the host array kcall points at, kept alive)
        # (the storage of the key-frame stores picks the entry point: the q8 one differs in its copy launch alone)
        kf_size, kf_fwd, kf_name = (lib.aid_processor_kf_q8_workspace_bytes, lib.aid_processor_kf_q8_fwd, "aid_processor_kf_q8_fwd") \
            if kf.get("storage", "native") == "q8" else (lib.aid_processor_kf_workspace_bytes, lib.aid_processor_kf_fwd, "aid_processor_kf_fwd")
        nbytes = kf_size(C.byref(a), C.byref(kcall))
    else:
        nbytes = lib.aid_processor_workspace_bytes(C.byref(a))
    with _on(dev):
        if nbytes == 0:
            # let the library say why
            a.workspace, a.workspace_bytes = None, 0
            if est is not None:
                _lib.check(lib.aid_processor_ep_fwd(C.byref(a), C.byref(est), _stream()), "aid_processor_ep_fwd")
            elif kcall is not None:
                _lib.check(kf_fwd(C.byref(a), C.byref(kcall), _stream()), kf_name)
            elif ccall is not None:
                _lib.check(lib.aid_processor_corners_fwd(C.byref(a), C.byref(ccall), _stream()), "aid_processor_corners_fwd")
            else:
                _lib.check(lib.aid_processor_fwd(C.byref(a), _stream()), "aid_processor_fwd")
            raise RuntimeError("aid_processor_workspace_bytes returned 0")
        ws = workspace(nbytes, dev)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        if est is not None:
            _lib.check(lib.aid_processor_ep_fwd(C.byref(a), C.byref(est), _stream()), "aid_processor_ep_fwd")
        elif kcall is not None:
            _lib.check(kf_fwd(C.byref(a), C.byref(kcall), _stream()), kf_name)
        elif ccall is not None:
            _lib.check(lib.aid_processor_corners_fwd(C.byref(a), C.byref(ccall), _stream()), "aid_processor_corners_fwd")
        elif seg_arr is not None:
            _lib.check(lib.aid_processor_ip_fwd(C.byref(a), C.addressof(seg_arr), len(seg_arr), _stream()), "aid_processor_ip_fwd")
        else:
            _lib.check(lib.aid_processor_fwd(C.byref(a), _stream()), "aid_processor_fwd")
    return out


# ---- end-point K / V^T store (aid_hip.h: aid_endpoint_rows, aid_processor_ep_fwd) ---------------------------------------------------
def endpoint_block_sizes(l: int, c: int) -> Tuple[int, int]:
    """(k_fs, vt_fs): elements of one end-point block of keys [L, C] and of transposed values [C, round_up(L, 8)]."""
    return l * c, c * ((l + 7) // 8 * 8)


def _check_store_tensors(k_store: torch.Tensor, vt_store: torch.Tensor, step: torch.Tensor, k_fs: int, vt_fs: int,
                         dtype: torch.dtype) -> int:
    """Checks a layer's store against the block sizes of a call; returns n_steps."""
    _require_gpu(k_store, vt_store, step)
    if k_store.dtype != dtype or vt_store.dtype != dtype:
        raise TypeError(f"the end-point store holds {k_store.dtype}, the call computes in {dtype}")
    n_steps = k_store.shape[0]
    if k_store.ndim != 3 or vt_store.ndim != 3 or tuple(k_store.shape) != (n_steps, 2, k_fs) or tuple(vt_store.shape) != (n_steps, 2, vt_fs) \
            or not k_store.is_contiguous() or not vt_store.is_contiguous() or n_steps < 1:
        raise ValueError(f"the end-point store must be k_store [n_steps, 2, {k_fs}] / vt_store [n_steps, 2, {vt_fs}], contiguous; got "
                         f"{tuple(k_store.shape)} / {tuple(vt_store.shape)}")
    if step.dtype != torch.int32 or step.numel() != 1:
        raise ValueError("the step index is ONE int32 on the device (rewritten in place between calls)")
    return n_steps


def _endpoint_store_args(ep: dict, l: int, c: int, dtype: torch.dtype) -> AidEndpointStore:
    k_fs, vt_fs = endpoint_block_sizes(l, c)
    est = AidEndpointStore()
    est.n_steps = _check_store_tensors(ep["k_store"], ep["vt_store"], ep["step"], k_fs, vt_fs, dtype)
    est.k_store, est.vt_store, est.step = ep["k_store"].data_ptr(), ep["vt_store"].data_ptr(), ep["step"].data_ptr()
    try:
        est.mode = EP_MODES[ep["mode"]]
    except (KeyError, TypeError):
        raise ValueError(f"ep['mode'] must be 'record' or 'replay'; got {ep.get('mode')!r}") from None
    return est


def endpoint_rows(k: torch.Tensor, vt: torch.Tensor, k_store: torch.Tensor, vt_store: torch.Tensor, step: torch.Tensor,
                  direction: str, row_begin: int = 0, row_end: int = -1) -> None:
    """Move the blocks ``k[row_begin]``, ``k[row_end]``, ``vt[row_begin]``, ``vt[row_end]`` between a call's k [F, L, C] /
    vt [F, C, Lp] and slot ``step[0]`` of a layer's store (``k_store`` [n_steps, 2, L C], ``vt_store`` [n_steps, 2, C Lp]) in one
    launch (``aid_endpoint_rows``): ``direction`` "put" = call -> store, "get" = store -> call.  ``step`` is ONE int32 on the device,
    read by the kernel; an index outside the store moves nothing."""
    dev = _require_gpu(k, vt)
    if k.dtype != vt.dtype or k.ndim != 3 or vt.ndim != 3 or not k.is_contiguous() or not vt.is_contiguous() or k.shape[0] != vt.shape[0]:
        raise ValueError("k [F, L, C] and vt [F, C, Lp] must be contiguous tensors of one dtype with the same number of rows")
    f = k.shape[0]
    a = AidEndpointRows()
    a.k_fs, a.vt_fs = k.shape[1] * k.shape[2], vt.shape[1] * vt.shape[2]
    a.n_steps = _check_store_tensors(k_store, vt_store, step, a.k_fs, a.vt_fs, k.dtype)
    a.k, a.vt, a.k_store, a.vt_store, a.step = k.data_ptr(), vt.data_ptr(), k_store.data_ptr(), vt_store.data_ptr(), step.data_ptr()
    a.row_begin, a.row_end = row_begin % f, row_end % f
    try:
        a.direction = EP_DIRECTIONS[direction]
    except (KeyError, TypeError):
        raise ValueError(f"direction must be 'put' or 'get'; got {direction!r}") from None
    a.dtype = _dtype_code(k)
    with _on(dev):
        _lib.check(_lib.load().aid_endpoint_rows(C.byref(a), _stream()), "aid_endpoint_rows")


def processor_ep_fwd(x: torch.Tensor, wq: torch.Tensor, wk: torch.Tensor, wv: torch.Tensor, wo: torch.Tensor,
                     bo: Optional[torch.Tensor], heads: int, *, ep: dict, **kwargs) -> torch.Tensor:
    """A SELF-attention AID processor call with the end-point store of its layer beside it (``aid_processor_ep_fwd``) — still one
    library call.  ``ep`` = dict(k_store=[n_steps, 2, S C], vt_store=[n_steps, 2, C round_up(S, 8)], step=int32 device [1],
    mode="record" | "replay"); every other keyword is ``processor_fwd``'s (mode, fused, coef, n_plain, ln, residual, ln_folded,
    attn_bias, lora, f32_precision, ...).
    "record": ``processor_fwd`` itself — ``y`` bit for bit — plus the end-point rows ``begin`` / ``end`` of this step's k / V^T put into
    slot ``step[0]``.  "replay": ``x`` holds the LOCAL frames only (interior coefficients, PLAIN riders); the recorded rows of slot
    ``step[0]`` are the end points (``begin`` / ``end`` are not read)."""
    if ep is None:
        raise ValueError("processor_ep_fwd needs the layer's store (ep=...); without one call processor_fwd")
    if kwargs.get("ip") is not None or kwargs.get("ip_segments") or kwargs.get("kv_cached") is not None or kwargs.get("ctx_map") is not None:
        raise ValueError("an end-point store belongs to a self-attention call: no image branch, no cached text keys, no ctx_map")
    if kwargs.get("mode", "plain") == "plain":
        raise ValueError("an end-point store belongs to an interpolated (inner / outer) call")
    return processor_fwd(x, None, wq, wk, wv, wo, bo, heads, ep=ep, **kwargs)


# ---- key-frame K / V^T stores (aid_hip.h: aid_keyframe_rows, aid_processor_kf_fwd) --------------------------------------------------
def q8_block_bytes(n: int) -> int:
    """Bytes of one block row of ``n`` elements in a q8 key-frame store (``aid_q8_block_bytes``): n int8, one exponent byte per 32
    elements, rounded up to 16 bytes; 0 for an ``n`` that is no positive multiple of 8."""
    n = int(n)
    return 0 if n < 8 or n % 8 else (n + (n + 31) // 32 + 15) // 16 * 16


def _check_storage(storage) -> str:
    if storage not in KF_STORAGES:
        raise ValueError(f"storage must be 'native' or 'q8'; got {storage!r}")
    return storage


def _keyframe_row_array(entries, step: torch.Tensor, k_fs: int, vt_fs: int, dtype: torch.dtype, storage: str = "native"):
    """The host array of AidKeyframeRow for ``entries`` = [(k_store [n_steps, k_fs], vt_store [n_steps, vt_fs], row), ...]; returns
    (array, n_steps).  Every key frame's store is its own allocation; all hold the same number of steps.  ``storage`` "q8": the stores
    are uint8 [n_steps, q8_block_bytes(k_fs)] / [n_steps, q8_block_bytes(vt_fs)]."""
    entries = list(entries)
    if storage == "q8":
        dtype, k_fs, vt_fs = torch.uint8, q8_block_bytes(k_fs), q8_block_bytes(vt_fs)
    if not 1 <= len(entries) <= KF_MAX_ROWS:
        raise ValueError(f"one launch moves 1 .. {KF_MAX_ROWS} key-frame rows; got {len(entries)}")
    arr = (AidKeyframeRow * len(entries))()
    n_steps = None
    for i, (k_store, vt_store, row) in enumerate(entries):
        _require_gpu(k_store, vt_store)
        if k_store.dtype != dtype or vt_store.dtype != dtype:
            if storage == "q8":
                raise TypeError(f"the key-frame store holds {k_store.dtype}, a q8 store holds {dtype} block rows")
            raise TypeError(f"the key-frame store holds {k_store.dtype}, the call computes in {dtype}")
        ns = k_store.shape[0]
        if k_store.ndim != 2 or vt_store.ndim != 2 or tuple(k_store.shape) != (ns, k_fs) or tuple(vt_store.shape) != (ns, vt_fs) \
                or not k_store.is_contiguous() or not vt_store.is_contiguous() or ns < 1:
            raise ValueError(f"a key-frame store must be k_store [n_steps, {k_fs}] / vt_store [n_steps, {vt_fs}], contiguous; got "
                             f"{tuple(k_store.shape)} / {tuple(vt_store.shape)}")
        if n_steps is not None and ns != n_steps:
            raise ValueError(f"the key-frame stores of one launch hold the same number of steps; got {n_steps} and {ns}")
        n_steps = ns
        arr[i].k_store, arr[i].vt_store, arr[i].row = k_store.data_ptr(), vt_store.data_ptr(), int(row)
    _require_gpu(step)
    if step.dtype != torch.int32 or step.numel() != 1:
        raise ValueError("the step index is ONE int32 on the device (rewritten in place between calls)")
    return arr, n_steps


def _keyframe_call_args(kf: dict, n_frames: int, l: int, c: int, dtype: torch.dtype):
    k_fs, vt_fs = endpoint_block_sizes(l, c)
    try:
        mode = KF_MODES[kf["mode"]]
    except (KeyError, TypeError):
        raise ValueError(f"kf['mode'] must be 'record' or 'replay'; got {kf.get('mode')!r}") from None
    entries = [(k_, v_, int(r_) % n_frames if mode == KF_RECORD else 0) for k_, v_, r_ in kf["entries"]]
    if mode == KF_REPLAY and len(entries) != 2:
        raise ValueError(f"a replay takes exactly two key-frame stores (begin, end); got {len(entries)}")
    if mode == KF_RECORD and len({r_ for _, _, r_ in entries}) != len(entries):
        raise ValueError("the recorded rows must be distinct")
    arr, n_steps = _keyframe_row_array(entries, kf["step"], k_fs, vt_fs, dtype, _check_storage(kf.get("storage", "native")))
    call = AidKeyframeCall()
    call.rows, call.step, call.n_rows, call.n_steps, call.mode = arr, kf["step"].data_ptr(), len(arr), n_steps, mode
    return call, arr


def keyframe_rows(k: torch.Tensor, vt: torch.Tensor, entries, step: torch.Tensor, direction: str) -> None:
    """Move rows between a call's k [F, L, C] / vt [F, C, Lp] and slot ``step[0]`` of up to 8 key-frame stores in one launch
    (``aid_keyframe_rows``).  ``entries`` = [(k_store [n_steps, L C], vt_store [n_steps, C Lp], row), ...], each store its own
    allocation; ``direction`` "put" = call -> store, "get" = store -> call.  ``step`` is ONE int32 on the device, read by the kernel; an
    index outside the stores moves nothing."""
    dev = _require_gpu(k, vt)
    if k.dtype != vt.dtype or k.ndim != 3 or vt.ndim != 3 or not k.is_contiguous() or not vt.is_contiguous() or k.shape[0] != vt.shape[0]:
        raise ValueError("k [F, L, C] and vt [F, C, Lp] must be contiguous tensors of one dtype with the same number of rows")
    f = k.shape[0]
    a = AidKeyframeRows()
    a.k_fs, a.vt_fs = k.shape[1] * k.shape[2], vt.shape[1] * vt.shape[2]
    arr, a.n_steps = _keyframe_row_array([(k_, v_, int(r_) % f) for k_, v_, r_ in entries], step, a.k_fs, a.vt_fs, k.dtype)
    a.k, a.vt, a.rows, a.step, a.n_rows = k.data_ptr(), vt.data_ptr(), arr, step.data_ptr(), len(arr)
    try:
        a.direction = KF_DIRECTIONS[direction]
    except (KeyError, TypeError):
        raise ValueError(f"direction must be 'put' or 'get'; got {direction!r}") from None
    a.dtype = _dtype_code(k)
    with _on(dev):
        _lib.check(_lib.load().aid_keyframe_rows(C.byref(a), _stream()), "aid_keyframe_rows")


def keyframe_rows_q8(k: torch.Tensor, vt: torch.Tensor, entries, step: torch.Tensor, direction: str, vt_cols: Optional[int] = None) -> None:
    """``keyframe_rows`` with 8-bit block stores (``aid_keyframe_rows_q8``): "put" quantises rows of k [F, L, C] / vt [F, C, Lp] into
    slot ``step[0]`` of ``entries`` = [(k_store uint8 [n_steps, q8_block_bytes(L C)], vt_store uint8 [n_steps, q8_block_bytes(C Lp)],
    row), ...], "get" dequantises them back.  Of every vt row the first ``vt_cols`` columns (default: all Lp) are stored; the others
    are pad — never read, +0 after "get".  LOSSY: per block of 32 elements |y - x| <= 2^(e-1) < max|x| / 127 (include/aid_hip.h)."""
    dev = _require_gpu(k, vt)
    if k.dtype != vt.dtype or k.ndim != 3 or vt.ndim != 3 or not k.is_contiguous() or not vt.is_contiguous() or k.shape[0] != vt.shape[0]:
        raise ValueError("k [F, L, C] and vt [F, C, Lp] must be contiguous tensors of one dtype with the same number of rows")
    f = k.shape[0]
    a = AidKeyframeRowsQ8()
    a.k_fs, a.vt_fs = k.shape[1] * k.shape[2], vt.shape[1] * vt.shape[2]
    a.vt_ld, a.vt_cols = vt.shape[2], vt.shape[2] if vt_cols is None else int(vt_cols)
    arr, a.n_steps = _keyframe_row_array([(k_, v_, int(r_) % f) for k_, v_, r_ in entries], step, a.k_fs, a.vt_fs, k.dtype, "q8")
    a.k, a.vt, a.rows, a.step, a.n_rows = k.data_ptr(), vt.data_ptr(), arr, step.data_ptr(), len(arr)
    try:
        a.direction = KF_DIRECTIONS[direction]
    except (KeyError, TypeError):
        raise ValueError(f"direction must be 'put' or 'get'; got {direction!r}") from None
    a.dtype = _dtype_code(k)
    with _on(dev):
        _lib.check(_lib.load().aid_keyframe_rows_q8(C.byref(a), _stream()), "aid_keyframe_rows_q8")


def processor_kf_fwd(x: torch.Tensor, wq: torch.Tensor, wk: torch.Tensor, wv: torch.Tensor, wo: torch.Tensor,
                     bo: Optional[torch.Tensor], heads: int, *, kf: dict, **kwargs) -> torch.Tensor:
    """A SELF-attention processor call with key-frame stores of its layer beside it (``aid_processor_kf_fwd``) — still one library
    call.  ``kf`` = dict(entries=[(k_store [n_steps, S C], vt_store [n_steps, C round_up(S, 8)], row), ...], step=int32 device [1],
    mode="record" | "replay"[, storage="native" | "q8"]); every other keyword is ``processor_fwd``'s.  With ``storage="q8"`` the stores
    are the uint8 block stores of ``keyframe_rows_q8`` and the call is ``aid_processor_kf_q8_fwd``: the same call with the quantising /
    dequantising copy launch (lossy; "record" still returns ``y`` bit for bit).
    "record": a ``mode="plain"`` call over a batch that holds the key frames — ``processor_fwd`` itself, ``y`` bit for bit — plus rows
    ``row`` of this step's k / V^T put into slot ``step[0]`` of their stores (1 .. 8 entries, distinct rows).  "replay": an
    interpolated call; ``x`` holds the LOCAL frames only (interior coefficients, PLAIN riders), the two entries are the begin and the
    end frame's stores (``row`` is ignored, ``begin`` / ``end`` are not read); swapped, the call renders the reverse direction."""
    if kf is None:
        raise ValueError("processor_kf_fwd needs the layer's key-frame stores (kf=...); without them call processor_fwd")
    if kwargs.get("ip") is not None or kwargs.get("ip_segments") or kwargs.get("kv_cached") is not None or kwargs.get("ctx_map") is not None:
        raise ValueError("key-frame stores belong to a self-attention call: no image branch, no cached text keys, no ctx_map")
    plain = kwargs.get("mode", "plain") == "plain"
    if kf.get("mode") == "record" and not plain:
        raise ValueError("key frames are recorded from a plain call (mode='plain'): an end point's trajectory is plain attention")
    if kf.get("mode") == "replay" and plain:
        raise ValueError("key-frame stores replay into an interpolated (inner / outer) call")
    return processor_fwd(x, None, wq, wk, wv, wo, bo, heads, kf=kf, **kwargs)


# ---- key-frame blend (aid_hip.h: aid_mix_kv_stores, aid_processor_kf_blend_fwd) -----------------------------------------------------
def _keyframe_blend_args(kf: dict, n_frames: int, l: int, c: int, dtype: torch.dtype):
    """AidKeyframeBlend of ``kf`` = dict(entries=[(k_store, vt_store, _), ...], step=int32 device [1], weights=float32 device
    [n_frames, M][, storage="native" | "q8"]) for a call with blocks of [l, c] keys; returns (struct, the host array it points at)."""
    k_fs, vt_fs = endpoint_block_sizes(l, c)
    entries = [(k_, v_, 0) for k_, v_, _ in kf["entries"]]
    if not 1 <= len(entries) <= MAX_CORNERS:
        raise ValueError(f"a call blends 1 .. {MAX_CORNERS} key frames; got {len(entries)}")
    storage = _check_storage(kf.get("storage", "native"))
    arr, n_steps = _keyframe_row_array(entries, kf["step"], k_fs, vt_fs, dtype, storage)
    w = kf.get("weights")
    _require_gpu(w)
    if w is None or w.dtype != torch.float32 or tuple(w.shape) != (n_frames, len(arr)) or not w.is_contiguous():
        raise ValueError(f"weights must be a contiguous float32 device tensor [{n_frames}, {len(arr)}] (one row per local frame, one "
                         f"column per key frame); got {None if w is None else (tuple(w.shape), w.dtype)}")
    b = AidKeyframeBlend()
    b.rows, b.step, b.weights, b.n_corners, b.n_steps, b.q8 = arr, kf["step"].data_ptr(), w.data_ptr(), len(arr), n_steps, int(storage == "q8")
    return b, arr


def mix_kv_stores(entries, step: torch.Tensor, weights: torch.Tensor, shape_k: Sequence[int], shape_vt: Sequence[int], dtype: torch.dtype,
                  n_plain: int = 0, storage: str = "native", vt_cols: Optional[int] = None,
                  out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``k2[i] = sum_m weights[i, m] K_m[step]`` (and V^T -> vt2) for the first ``N - n_plain`` frames, read straight from slot
    ``step[0]`` of M <= 8 key-frame stores in one streaming launch (``aid_mix_kv_stores``) — ``keyframe_rows[_q8]`` "get" followed by
    ``mix_kv``, bit for bit, without the M rows in between.  ``entries`` = [(k_store, vt_store, _), ...] as ``keyframe_rows`` /
    ``keyframe_rows_q8`` (``storage="q8"``) take them, ``shape_k`` = (L, C) and ``shape_vt`` = (C, Lp) the call's blocks, ``dtype`` its
    element type, ``weights`` float32 device [N, M]; q8: of every vt row the first ``vt_cols`` columns (default: all) are stored, the
    others are +0.  Returns (k2 [N, L, C], vt2 [N, C, Lp]) — ``out`` or fresh tensors; the rows of the last ``n_plain`` frames are not
    written.  A step outside the stores writes nothing."""
    (l, c), (c2, lp) = (int(v) for v in shape_k), (int(v) for v in shape_vt)
    if weights.ndim != 2:
        raise ValueError("weights must be [N, M]")
    dev = _require_gpu(weights, step, *(out or ()))
    n = weights.shape[0]
    entries = list(entries)
    storage = _check_storage(storage)
    if not 1 <= len(entries) <= MAX_CORNERS:
        raise ValueError(f"a call blends 1 .. {MAX_CORNERS} key frames; got {len(entries)}")
    arr, n_steps = _keyframe_row_array([(k_, v_, 0) for k_, v_, _ in entries], step, l * c, c2 * lp, dtype, storage)
    if weights.dtype != torch.float32 or weights.shape[1] != len(arr) or not weights.is_contiguous():
        raise ValueError(f"weights must be a contiguous float32 device tensor [N, {len(arr)}]")
    if out is None:
        out = (torch.empty(n, l, c, dtype=dtype, device=dev), torch.empty(n, c2, lp, dtype=dtype, device=dev))
    k2, vt2 = out
    if k2.dtype != dtype or vt2.dtype != dtype or tuple(k2.shape) != (n, l, c) or tuple(vt2.shape) != (n, c2, lp) \
            or not k2.is_contiguous() or not vt2.is_contiguous():
        raise ValueError("out must be (k2 [N, L, C], vt2 [N, C, Lp]) contiguous")
    b = AidKeyframeBlend()
    b.rows, b.step, b.weights, b.n_corners, b.n_steps, b.q8 = arr, step.data_ptr(), weights.data_ptr(), len(arr), n_steps, int(storage == "q8")
    with _on(dev):
        _lib.check(_lib.load().aid_mix_kv_stores(C.byref(b), k2.data_ptr(), vt2.data_ptr(), n, int(n_plain), l * c, c2 * lp, lp,
                                                 lp if vt_cols is None else int(vt_cols), _dtype_code(k2), _stream()), "aid_mix_kv_stores")
    return k2, vt2


def processor_kf_blend_fwd(x: torch.Tensor, wq: torch.Tensor, wk: torch.Tensor, wv: torch.Tensor, wo: torch.Tensor,
                           bo: Optional[torch.Tensor], heads: int, *, kf: dict, weights: torch.Tensor, **kwargs) -> torch.Tensor:
    """A SELF-attention corner-weighted call whose corners are recorded key frames (``aid_processor_kf_blend_fwd``) — still one
    library call.  ``x`` holds the LOCAL frames only (the AID frames, then ``n_plain`` riders); ``kf`` = dict(entries=[(k_store,
    vt_store, _) x M], step=int32 device [1], mode="blend"[, storage="q8"]) names the M <= 8 key frames' stores of the layer,
    ``weights`` float32 device [N, M] the frames' weight rows (as ``processor_corners_fwd``).  mode="outer": one "get" puts the M
    recorded rows behind the local ones and the corner composition runs on them; mode="inner": ``mix_kv_stores`` writes the mixed
    rows straight from the stores.  Every other keyword is ``processor_fwd``'s except ``coef`` / ``begin`` / ``end`` (not read) and
    the contexts, image branches and other stores, which the call does not take."""
    if kf is None or kf.get("mode") != "blend":
        raise ValueError("processor_kf_blend_fwd needs the layer's key-frame stores as kf=dict(..., mode='blend')")
    for name in ("coef", "begin", "end", "ip", "ip_segments", "ep", "corners", "kv_cached", "ctx_map"):
        if kwargs.get(name) is not None:
            raise ValueError(f"a key-frame blend takes no {name}=")
    return processor_fwd(x, None, wq, wk, wv, wo, bo, heads, kf=dict(kf, weights=weights), **kwargs)


# ---- corner-weighted AID (aid_hip.h: aid_mix_kv, aid_attn_corners_fwd, aid_processor_corners_fwd) ------------------------------------
def _corners_args(corners: dict, n_frames: int, n_kv: int, scratch: Optional[torch.Tensor] = None):
    """AidCorners of ``corners`` = dict(weights=float32 device [n_frames, M], rows=M ints) for a call of ``n_frames`` frames over ``n_kv``
    rows of k / V^T (negative rows count from the end); returns (struct, the host row array it points at)."""
    w = corners["weights"]
    rows = [int(r) for r in corners["rows"]]
    _require_gpu(w)
    m = len(rows)
    if not 1 <= m <= MAX_CORNERS:
        raise ValueError(f"a call interpolates among 1 .. {MAX_CORNERS} corners; got {m}")
    if w.dtype != torch.float32 or w.ndim != 2 or tuple(w.shape) != (n_frames, m) or not w.is_contiguous():
        raise ValueError(f"weights must be a contiguous float32 device tensor [{n_frames}, {m}] (one row per frame, one column per corner); "
                         f"got {tuple(w.shape)} {w.dtype}")
    for r in rows:
        if not -n_kv <= r < n_kv:
            raise ValueError(f"corner row {r} outside the {n_kv} rows of k / V^T")
    arr = (C.c_int32 * m)(*[r % n_kv for r in rows])
    c = AidCorners()
    c.rows, c.weights, c.n_corners = arr, w.data_ptr(), m
    if scratch is not None:
        c.scratch, c.scratch_bytes = scratch.data_ptr(), scratch.numel() * scratch.element_size()
    return c, arr


def mix_kv(k: torch.Tensor, vt: torch.Tensor, weights: torch.Tensor, rows: Sequence[int], n_plain: int = 0,
           out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``k2[i] = sum_m weights[i, m] k[rows[m]]`` (and vt -> vt2) for the first ``N - n_plain`` frames in one streaming launch
    (``aid_mix_kv``): k [F, L, C], vt [F, C, Lp] contiguous, ``weights`` float32 device [N, M] with M = len(rows) <= 8.  fp32 products
    and sum in corner order, one rounding; a one-hot row returns the corner's bits.  Returns (k2 [N, L, C], vt2 [N, C, Lp]) — ``out``
    or fresh tensors; the rows of the last ``n_plain`` frames are not written."""
    dev = _require_gpu(k, vt, weights, *(out or ()))
    dt = _dtype_code(k)
    if k.dtype != vt.dtype or k.ndim != 3 or vt.ndim != 3 or not k.is_contiguous() or not vt.is_contiguous() or k.shape[0] != vt.shape[0]:
        raise ValueError("k [F, L, C] and vt [F, C, Lp] must be contiguous tensors of one dtype with the same number of rows")
    if weights.ndim != 2:
        raise ValueError("weights must be [N, M]")
    n = weights.shape[0]
    cn, _rows = _corners_args(dict(weights=weights, rows=rows), n, k.shape[0])
    if out is None:
        out = (torch.empty(n, *k.shape[1:], dtype=k.dtype, device=k.device), torch.empty(n, *vt.shape[1:], dtype=k.dtype, device=k.device))
    k2, vt2 = out
    if k2.dtype != k.dtype or vt2.dtype != k.dtype or tuple(k2.shape) != (n, *k.shape[1:]) or tuple(vt2.shape) != (n, *vt.shape[1:]) \
            or not k2.is_contiguous() or not vt2.is_contiguous():
        raise ValueError("out must be (k2 [N, L, C], vt2 [N, C, Lp]) contiguous, laid out like k / vt")
    with _on(dev):
        _lib.check(_lib.load().aid_mix_kv(k.data_ptr(), vt.data_ptr(), k2.data_ptr(), vt2.data_ptr(), _rows, weights.data_ptr(), n,
                                          int(n_plain), cn.n_corners, k.shape[1] * k.shape[2], vt.shape[1] * vt.shape[2], dt, _stream()),
                   "aid_mix_kv")
    return k2, vt2


def attn_corners_fwd(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, heads: int, *, l: int, weights: torch.Tensor,
                     rows: Sequence[int], mode: str = "outer", fused: bool = False, n_plain: int = 0,
                     out: Optional[torch.Tensor] = None, kv_map: Optional[torch.Tensor] = None,
                     softmax_scale: Optional[float] = None, q_prescaled: bool = False, bias: Optional[torch.Tensor] = None,
                     f32_attn_precision: Optional[str] = None) -> torch.Tensor:
    """The attention core among up to 8 corners (``aid_attn_corners_fwd``): frame i has the non-negative weight row ``weights[i]``
    (float32 device [N, M]) over the corner rows ``rows`` of k / vt,
        outer:  O_i = sum_m w[i, m] A(Q_i, [K_i ;] K[r_m], ..)        inner:  O_i = A(Q_i, [K_i ;] sum_m w[i, m] K[r_m], ..)
    The last ``n_plain`` frames run plain attention (their weight rows are not read).  Outer runs ceil(M / 2) passes of ``attn_fwd``
    (the later ones accumulate, each rounding ``out`` once more); inner one ``mix_kv`` and one pass.  Tensors as ``attn_fwd``; with
    ``kv_map`` the corner rows are rows of k / vt (context rows) and inner mixes one row per frame."""
    lib = _lib.load()
    attn_split = f32_attn_split_code(f32_attn_precision)
    dev = _require_gpu(q, k, vt, out, weights, kv_map, bias)
    dt = _dtype_code(q)
    if _dtype_code(k) != dt or _dtype_code(vt) != dt:
        raise TypeError("q, k, vt must share one dtype")
    if mode not in ("inner", "outer"):
        raise ValueError("a corner-weighted call is mode='inner' or 'outer'")
    assert q.is_contiguous() and k.is_contiguous() and vt.is_contiguous()
    n, s, c = q.shape
    f = k.shape[0]
    d = c // heads
    if out is None:
        out = torch.empty_like(q)
    if kv_map is not None and (kv_map.dtype != torch.int32 or kv_map.numel() != n):
        raise ValueError("kv_map must be an int32 device tensor with one entry per frame")
    nb = int(lib.aid_corners_scratch_bytes(n, len(list(rows))))
    scratch = torch.empty(max(nb, 16), dtype=torch.uint8, device=q.device)
    cn, _rows = _corners_args(dict(weights=weights, rows=rows), n, f, scratch)
    a = AidAttnArgs()
    a.q, a.k, a.vt, a.out = q.data_ptr(), k.data_ptr(), vt.data_ptr(), out.data_ptr()
    a.kv_map = _ptr(kv_map)
    if mode == "inner":
        k2 = torch.empty(n, *k.shape[1:], dtype=k.dtype, device=k.device)
        vt2 = torch.empty(n, *vt.shape[1:], dtype=k.dtype, device=k.device)
        a.k2, a.vt2 = k2.data_ptr(), vt2.data_ptr()
    a.n_frames, a.n_kv = n, f
    a.s, a.l, a.heads, a.d = s, l, heads, d
    a.ldq, a.ldk, a.ldvt, a.ldo = c, k.shape[2], vt.shape[2], out.shape[2]
    a.q_fs, a.k_fs, a.vt_fs, a.o_fs = s * c, k.shape[1] * k.shape[2], vt.shape[1] * vt.shape[2], s * out.shape[2]
    a.mode, a.fused, a.dtype = MODES[mode], int(bool(fused)), dt
    a.softmax_scale = float(d ** -0.5 if softmax_scale is None else softmax_scale)
    a.n_plain = int(n_plain)
    if bias is not None:
        a.bias = bias.data_ptr()
        a.bias_fs, a.bias_hs, a.bias_rs = score_bias_layout(bias, n, heads, s, l, q.dtype)
    a.q_prescaled = int(bool(q_prescaled))
    if dt == DTYPE_F32:
        a.f32_split = attn_split
    with _on(dev):
        _lib.check(lib.aid_attn_corners_fwd(C.byref(a), C.byref(cn), _stream()), "aid_attn_corners_fwd")
    return out


def processor_corners_fwd(x: torch.Tensor, ctx: Optional[torch.Tensor], wq: torch.Tensor, wk: torch.Tensor, wv: torch.Tensor,
                          wo: torch.Tensor, bo: Optional[torch.Tensor], heads: int, *, weights: torch.Tensor, rows: Sequence[int],
                          **kwargs) -> torch.Tensor:
    """One whole processor call among up to 8 corners (``aid_processor_corners_fwd``) — still one library call: ``processor_fwd`` with
    its attention step replaced by ``attn_corners_fwd``'s composition.  ``weights`` float32 device [N, M], ``rows`` the M corner rows of
    k / V^T (frame rows, or context rows with ``ctx_map``); every other keyword is ``processor_fwd``'s (mode="inner" | "outer", fused,
    n_plain, ctx_map, ln, residual, kv_cached, attn_bias, lora, f32_precision, ...) except ``coef`` / ``begin`` / ``end``, which a
    corner-weighted call does not read, and the image branches and stores, which it does not take."""
    for name in ("coef", "begin", "end", "ip", "ip_segments", "ep", "kf"):
        if kwargs.get(name) is not None:
            raise ValueError(f"a corner-weighted call takes no {name}=")
    return processor_fwd(x, ctx, wq, wk, wv, wo, bo, heads, corners=dict(weights=weights, rows=rows), **kwargs)
