"""GPU: aid_mix_kv_stores (include/aid_hip.h) — the INNER mix of a corner-weighted call read straight from key-frame stores, under
guarded buffers.

Oracle 1, bit for bit: the fused launch equals aid_keyframe_rows / aid_keyframe_rows_q8 GET of the M rows into scratch rows followed
by aid_mix_kv on those rows — whole blocks, native pad columns (finite data) included.
Oracle 2, independent: corners_ref.mix_rows in fp64 on the stored values (q8: q8_ref.dequantise of the store bytes), within one unit
in the last place of the storage type at the magnitude of the frame's largest fp64 result — the bound tests/test_hip_corners.py
applies to aid_mix_kv (fp32 products and sum of <= 8 terms, one rounding; f32 storage carries the rounding errors along).

The stores lie between guard bands in one byte buffer each and are compared byte for byte after every launch; k2 / vt2 are `Guarded`
outputs whose rider rows and bands must keep the sentinel."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import corners_ref as R  # noqa: E402
import q8_ref as Q  # noqa: E402
from aid_amd import _lib, ops  # noqa: E402
from guarded import Guarded  # noqa: E402
from util import to_np64  # noqa: E402

DEV = torch.device("cuda:0")
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DTYPES = [F16, BF16, F32]
ids_dt = lambda d: str(d).split(".")[-1]  # noqa: E731
INT = {F16: torch.int16, BF16: torch.int16, F32: torch.int32}
N_STEPS = 3
BLOCKS = [(8, 64, 8, 1), (1320, 1600, 40, 33), (4096, 4096, 64, 64)]          # (k_fs, vt_fs, vt_ld, vt_cols)
BIG = (2621440, 2621440, 4096, 4096)          # 655360 chunks of 16 bytes: more than one pass of the 2048 x 256 lanes of the capped grid
FRONT, TAIL = 4096, 1 << 16


def _b(t, dtype):
    """The bits of ``t`` [frames, ...] as integers [frames, block]."""
    return t.contiguous().view(INT[dtype]).reshape(t.shape[0], -1)


def _ulp_at(x, dtype):
    bits = {F16: 10, BF16: 7, F32: 23}[dtype]
    return 2.0 ** (np.floor(np.log2(x)) - bits)


class Store:
    """One key frame's k or vt store, [N_STEPS, row_bytes] bytes between two guard bands of 0xA5."""

    def __init__(self, row_bytes):
        self.buf = torch.full((FRONT + N_STEPS * row_bytes + TAIL,), 0xA5, dtype=torch.uint8, device=DEV)
        self.bytes = self.buf[FRONT:FRONT + N_STEPS * row_bytes].view(N_STEPS, row_bytes)
        self.snap = None

    def typed(self, dtype):
        return self.bytes.view(dtype)

    def snapshot(self):
        self.snap = self.buf.clone()

    def unchanged(self):
        return torch.equal(self.buf, self.snap)


def _make_stores(m, block, dtype, storage, seed):
    """M key frames' (k, vt) stores with every step filled: native — random finite values, pad columns included; q8 — what
    aid_keyframe_rows_q8 PUT (an existing, tested entry) leaves for random rows."""
    k_fs, vt_fs, vt_ld, vt_cols = block
    g = torch.Generator().manual_seed(seed)
    es = 4 if dtype == F32 else 2
    stores = []
    for _ in range(m):
        if storage == "q8":
            ks, vs = Store(Q.block_bytes(k_fs)), Store(Q.block_bytes(vt_fs))
        else:
            ks, vs = Store(k_fs * es), Store(vt_fs * es)
        stores.append((ks, vs))
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    for st in range(N_STEPS):
        step.fill_(st)
        for ks, vs in stores:
            scale = float(2.0 ** torch.randint(-3, 4, (1,), generator=g).item())
            k = (torch.randn(1, 1, k_fs, generator=g) * scale).to(dtype).to(DEV)
            vt = (torch.randn(1, vt_fs // vt_ld, vt_ld, generator=g) * scale).to(dtype).to(DEV)
            if storage == "q8":
                ops.keyframe_rows_q8(k, vt, [(ks.bytes, vs.bytes, 0)], step, "put", vt_cols=vt_cols)
            else:
                ks.typed(dtype)[st].copy_(k.reshape(-1))
                vs.typed(dtype)[st].copy_(vt.reshape(-1))
    torch.cuda.synchronize()
    for ks, vs in stores:
        ks.snapshot()
        vs.snapshot()
    return stores


def _entries(stores, dtype, storage):
    if storage == "q8":
        return [(ks.bytes, vs.bytes, 0) for ks, vs in stores]
    return [(ks.typed(dtype), vs.typed(dtype), 0) for ks, vs in stores]


def _weights(m, n_mix, n_plain, g):
    """[n_mix + n_plain, m]: the one-hot row of the last corner first when there are four rows, a generic row, a row with corner
    min(1, m - 1) at exactly 0, another generic row; the riders' rows are NaN (never read)."""
    gen = lambda: torch.rand(m, generator=g) + 0.05  # noqa: E731
    if n_mix == 1:
        rows = [gen()]
    else:
        hot = torch.zeros(m)
        hot[m - 1] = 1.0
        z = gen()
        z[min(1, m - 1)] = 0.0
        rows = [hot, gen() / m, z, gen()]
    return torch.cat([torch.stack(rows).float(), torch.full((n_plain, m), float("nan"))])


def _get_then_mix(stores, block, dtype, storage, step, w, n_plain):
    """Oracle 1 and the stored values: (k2, vt2) of GET + aid_mix_kv, and the scratch rows GET filled."""
    k_fs, vt_fs, vt_ld, vt_cols = block
    m = len(stores)
    ksc = torch.full((m, 1, k_fs), 7.0, dtype=dtype, device=DEV)
    vsc = torch.full((m, vt_fs // vt_ld, vt_ld), 7.0, dtype=dtype, device=DEV)
    ent = [(k_, v_, i) for i, (k_, v_, _) in enumerate(_entries(stores, dtype, storage))]
    if storage == "q8":
        ops.keyframe_rows_q8(ksc, vsc, ent, step, "get", vt_cols=vt_cols)
    else:
        ops.keyframe_rows(ksc, vsc, ent, step, "get")
    k2, vt2 = ops.mix_kv(ksc, vsc, w, list(range(m)), n_plain=n_plain)
    return k2, vt2, ksc, vsc


def _launch(stores, block, dtype, storage, step, w, n_plain):
    """The fused launch into guarded outputs; returns (K2, VT2)."""
    k_fs, vt_fs, vt_ld, vt_cols = block
    n, m = w.shape
    kr = k_fs // vt_ld if k_fs % vt_ld == 0 else 1                     # (rows only shape the guard bands: the call knows blocks)
    K2 = Guarded(n, kr, k_fs // kr, dtype, DEV, kind="output")
    VT2 = Guarded(n, vt_fs // vt_ld, vt_ld, dtype, DEV, kind="output")
    ent = _entries(stores, dtype, storage)
    arr = (_lib.AidKeyframeRow * m)()
    for i, (k_, v_, _) in enumerate(ent):
        arr[i].k_store, arr[i].vt_store, arr[i].row = k_.data_ptr(), v_.data_ptr(), -1
    b = _lib.AidKeyframeBlend()
    b.rows, b.step, b.weights, b.n_corners, b.n_steps, b.q8 = arr, step.data_ptr(), w.data_ptr(), m, N_STEPS, int(storage == "q8")
    _lib.check(_lib.load().aid_mix_kv_stores(C.byref(b), K2.ptr, VT2.ptr, n, n_plain, k_fs, vt_fs, vt_ld, vt_cols,
                                             ops._dtype_code(K2.view), ops._stream()), "aid_mix_kv_stores")
    torch.cuda.synchronize()
    return K2, VT2


def _stored_values(stores, block, dtype, storage, st):
    """fp64 [M, k_fs], [M, vt_fs]: what the stores hold at step ``st``, read on the host (q8: q8_ref.dequantise of the bytes)."""
    k_fs, vt_fs, vt_ld, vt_cols = block
    ks64, vs64 = [], []
    for ks, vs in stores:
        if storage == "q8":
            ks64.append(Q.dequantise(ks.bytes[st].cpu().numpy(), k_fs).astype(np.float64))
            vs64.append(Q.dequantise(vs.bytes[st].cpu().numpy(), vt_fs, vt_ld, vt_cols).astype(np.float64))
        else:
            ks64.append(to_np64(ks.typed(dtype)[st]))
            vs64.append(to_np64(vs.typed(dtype)[st]))
    return np.stack(ks64), np.stack(vs64)


def _check(stores, block, dtype, storage, st, n_mix, n_plain, seed, independent=True):
    k_fs, vt_fs, vt_ld, vt_cols = block
    m = len(stores)
    g = torch.Generator().manual_seed(seed)
    w = _weights(m, n_mix, n_plain, g)
    wd = w.to(DEV)
    step = torch.tensor([st], dtype=torch.int32, device=DEV)
    K2, VT2 = _launch(stores, block, dtype, storage, step, wd, n_plain)
    k2r, vt2r, ksc, vsc = _get_then_mix(stores, block, dtype, storage, step, wd, n_plain)
    torch.cuda.synchronize()
    mixed = list(range(n_mix))
    what = (block, ids_dt(dtype), storage, m, st, n_mix, n_plain)
    for G, ref, sc in ((K2, k2r, ksc), (VT2, vt2r, vsc)):
        # the contract: the mixed frames' whole blocks are written, nothing of a rider, nothing outside
        msg = G.untouched(G.layout.region_mask(frames=mixed))
        assert not msg, (what, msg)
        # oracle 1: GET + aid_mix_kv, bit for bit
        assert torch.equal(_b(G.view[:n_mix], dtype), _b(ref[:n_mix], dtype)), what
        if n_mix == 4:                                                  # the one-hot row: the corner's (dequantised) bits
            assert torch.equal(_b(G.view[:1], dtype), _b(sc[m - 1:m], dtype)), what
    if storage == "q8" and vt_cols < vt_ld:                             # pad columns of a q8 V^T block enter as +0
        assert not _b(VT2.view[:n_mix, :, vt_cols:], dtype).any(), what
    for ks, vs in stores:
        assert ks.unchanged() and vs.unchanged(), what
    if independent:                                                     # oracle 2: fp64 on the stored values
        k64, v64 = _stored_values(stores, block, dtype, storage, st)
        for G, src in ((K2, k64), (VT2, v64)):
            ref = R.mix_rows(src, list(range(m)), w[:n_mix].double().numpy())
            got = to_np64(G.view[:n_mix]).reshape(n_mix, -1)
            assert np.isfinite(got).all(), what
            for i in range(n_mix):
                mx = np.abs(ref[i]).max()
                if mx == 0:
                    assert not got[i].any()
                    continue
                err = np.abs(got[i] - ref[i]).max()
                assert err <= _ulp_at(mx, dtype), (what, i, err, _ulp_at(mx, dtype))


@pytest.mark.parametrize("storage", ["native", "q8"])
@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("block", BLOCKS, ids=lambda b: "x".join(map(str, b)))
@pytest.mark.parametrize("m", [1, 2, 3, 5, 8])
def test_mix_kv_stores(m, block, dtype, storage):
    stores = _make_stores(m, block, dtype, storage, seed=1000 * m + block[0])
    for n_mix in (1, 4):
        for n_plain in (0, 2):
            for st in (0, 2):
                _check(stores, block, dtype, storage, st, n_mix, n_plain, seed=17 * m + 5 * n_mix + n_plain + st)


@pytest.mark.parametrize("storage", ["native", "q8"])
def test_a_block_longer_than_one_pass_of_the_capped_grid(storage):
    stores = _make_stores(2, BIG, BF16, storage, seed=9)
    _check(stores, BIG, BF16, storage, 2, 4, 2, seed=3)
    _check(stores, BIG, BF16, storage, 0, 1, 0, seed=4)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dt)
def test_a_zero_weight_corner_is_not_read_into_the_result(dtype):
    """Native stores: corner 1's block of the step is all NaN and every row gives it weight exactly 0 — the result is finite, equals
    the fp64 mix of the other corners within the bound and GET + aid_mix_kv bit for bit."""
    block, m, st = BLOCKS[1], 3, 1
    stores = _make_stores(m, block, dtype, "native", seed=5)
    for s_ in stores[1]:
        s_.typed(dtype)[st].fill_(float("nan"))
        s_.snapshot()
    g = torch.Generator().manual_seed(6)
    w = torch.rand(4, m, generator=g) + 0.05
    w[:, 1] = 0.0
    wd = w.float().to(DEV)
    step = torch.tensor([st], dtype=torch.int32, device=DEV)
    K2, VT2 = _launch(stores, block, dtype, "native", step, wd, 0)
    k2r, vt2r, _, _ = _get_then_mix(stores, block, dtype, "native", step, wd, 0)
    k64, v64 = _stored_values(stores, block, dtype, "native", st)
    for G, ref_bits, src in ((K2, k2r, k64), (VT2, vt2r, v64)):
        got = to_np64(G.view).reshape(4, -1)
        assert np.isfinite(got).all()
        assert torch.equal(_b(G.view, dtype), _b(ref_bits, dtype))
        ref = R.mix_rows(np.nan_to_num(src), [0, 1, 2], w.float().double().numpy())
        for i in range(4):
            assert np.abs(got[i] - ref[i]).max() <= _ulp_at(np.abs(ref[i]).max(), dtype)


@pytest.mark.parametrize("storage", ["native", "q8"])
@pytest.mark.parametrize("bad", [-1, N_STEPS])
def test_a_step_outside_the_stores_writes_nothing(bad, storage):
    block, m = BLOCKS[1], 3
    stores = _make_stores(m, block, F16, storage, seed=8)
    w = _weights(m, 4, 2, torch.Generator().manual_seed(1)).to(DEV)
    step = torch.tensor([bad], dtype=torch.int32, device=DEV)
    K2, VT2 = _launch(stores, block, F16, storage, step, w, 2)
    for G in (K2, VT2):
        msg = G.untouched(torch.zeros(G.layout.numel, dtype=torch.bool))
        assert not msg, msg
    assert all(ks.unchanged() and vs.unchanged() for ks, vs in stores)


def test_the_f32_mix_of_one_corner_is_the_correctly_rounded_product():
    """M = 1 in f32 storage is one product per element: both kernels give round(w * x) — the exact product (it fits a float64) rounded
    ONCE.  csrc/Makefile builds the two objects without floating-point contraction for this: a contracted  p + err  is
    fma(w, x, err), which rounds 2 w x - p and can land one unit off."""
    block, st = BLOCKS[2], 1
    k_fs, vt_fs, vt_ld, _ = block
    stores = _make_stores(1, block, F32, "native", seed=12)
    g = torch.Generator().manual_seed(13)
    w = (torch.rand(4, 1, generator=g) + 0.05).float()
    w[0, 0] = 1.0
    wd = w.to(DEV)
    step = torch.tensor([st], dtype=torch.int32, device=DEV)
    K2, VT2 = _launch(stores, block, F32, "native", step, wd, 0)
    k2r, vt2r, ksc, vsc = _get_then_mix(stores, block, F32, "native", step, wd, 0)           # aid_mix_kv itself on the same rows
    for G, mixed, src in ((K2, k2r, ksc), (VT2, vt2r, vsc)):
        x64 = src.reshape(1, -1).double().cpu()
        want = (w.double() * x64).float()                                                   # exact in float64, one rounding
        assert torch.equal(mixed.reshape(4, -1).cpu().view(torch.int32), want.view(torch.int32))
        assert torch.equal(G.view.contiguous().reshape(4, -1).cpu().view(torch.int32), want.view(torch.int32))
