"""Cases of the float32 attention sweeps (a plain module, no GPU): the key counts, row counts and head dims at which
aid_attn_f32_kernel (csrc/aid_f32.hip) and aid_attn_f32x3_kernel (csrc/aid_f32x3.hip) take another path, and the input constructors
that tests/test_hip_f32_attn_key_counts.py (GPU) and tests/test_f32_attn_key_counts.py (CPU: the references alone stay inside the
bounds on these very numbers) share.

Both kernels walk 32-key tiles (FKT = XKT = 32).  A ragged last tile is masked through the kernel's key map (key_of / key_of_x3), its
V^T rows end in a 16-byte chunk that is read element by element when l % 4 != 0, and in a fused call the ragged tile of the own
segment is followed by tile 0 of the end-point segment.  KEY_COUNTS holds every residue mod 32 on one, two and three tiles, the tile
seams and five tiles; ROW_COUNTS every wave (32 rows) and workgroup (128 rows) seam and three workgroups.
"""
import numpy as np
import torch

from oracle import aid_oracle as O
from util import to_np64

KEY_COUNTS = tuple(range(1, 73)) + (95, 96, 97, 127, 128, 129, 160)
ROW_COUNTS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130, 257)
DIMS = (40, 64, 80, 160)
H = 2
TILE = 32                                            # FKT (aid_f32.hip) = XKT (aid_f32x3.hip)

# the sweep's call: end points 0 and 2, one interior frame, a PLAIN rider
N_SWEEP, S_SWEEP, L_ROWS = 4, 40, 45                 # (L_ROWS: the key count of the row sweep: two tiles, ragged, l % 4 = 1)
COEF_SWEEP = (0.0, 0.3, 1.0, -1.0)
BEGIN, END = 0, 2
# the late-maximum call
N_LATE, S_LATE = 3, 77
COEF_LATE = (0.0, 0.3, 1.0)
MODES = (("plain", False), ("inner", False), ("inner", True), ("outer", False), ("outer", True))
BIAS_KEY_COUNTS = (1, 5, 31, 32, 33, 45, 64, 77)


def round_up(x, m):
    return (x + m - 1) // m * m


def sweep_inputs(d, l, s=S_SWEEP, n=N_SWEEP):
    """float32 q [n, s, H d], k / v [n, l, H d]: randn from a generator seeded by (d, l)."""
    g = torch.Generator().manual_seed(1000 * d + l)
    c = H * d
    return torch.randn(n, s, c, generator=g), torch.randn(n, l, c, generator=g), torch.randn(n, l, c, generator=g)


def late_maximum_inputs(d):
    """s = l = 77: k = r + (4 / sqrt(d)) q with r random, so query row i scores about +4 on key i of its own frame above a unit-variance
    background: every row has its own preferred key, the keys spread over all three tiles and all 13 positions of the ragged last
    one, and the row is still not dominated by it (tests/test_f32_attn_key_counts.py checks both on the fp64 scores)."""
    g = torch.Generator().manual_seed(77000 + d)
    c = H * d
    q = torch.randn(N_LATE, S_LATE, c, generator=g)
    r = torch.randn(N_LATE, S_LATE, c, generator=g)
    v = torch.randn(N_LATE, S_LATE, c, generator=g)
    return q, r + (4.0 / d ** 0.5) * q, v


def bias_inputs(d, l, rows, n=N_SWEEP):
    """Additive score bias [n, rows, l] (rows = s: one row per query; rows = 1: one row for all queries): randn * 0.5, a random third
    of the keys at -10000, key 0 kept."""
    g = torch.Generator().manual_seed(500000 + 1000 * d + 10 * l + rows)
    b = torch.randn(n, rows, l, generator=g) * 0.5
    drop = torch.rand(n, rows, l, generator=g) < 1.0 / 3.0
    drop[..., 0] = False
    b[drop] = -10000.0
    return b


def vt_of(v):
    """V^T [n, c, round_up(l, 8)] with zero pad columns, as ops.attn_fwd takes it."""
    n, l, c = v.shape
    vt = torch.zeros(n, c, round_up(l, 8))
    vt[:, :, :l] = v.transpose(1, 2)
    return vt


def scores64(q, k, scale=None):
    """fp64 scaled scores [n, H, s, l] of PLAIN attention."""
    d = q.shape[-1] // H
    scale = d ** -0.5 if scale is None else scale
    return O.split_heads(to_np64(q), H) @ O.split_heads(to_np64(k), H).transpose(0, 1, 3, 2) * scale


def oracle_ref(q, k, v, mode, fused, coef, scale=None, mask=None, begin=BEGIN, end=END):
    """oracle.aid_oracle.attn_core in fp64 on float32 tensors; frames with a negative coefficient (PLAIN riders, all behind the
    interpolated frames) attend PLAIN to their own keys.  ``mask``: [n, 1 | s, l] or None."""
    q64, k64, v64 = to_np64(q), to_np64(k), to_np64(v)
    d = q64.shape[-1] // H
    scale = d ** -0.5 if scale is None else scale
    m64 = None if mask is None else to_np64(mask)
    plain = lambda a, b: O.attn_core(q64[a:b], k64[a:b], v64[a:b], H, scale, "plain", False, None,          # noqa: E731
                                     mask=None if m64 is None else m64[a:b])
    n = q64.shape[0]
    if mode == "plain":
        return plain(0, n)
    na = sum(1 for x in coef if x >= 0)
    assert all(x < 0 for x in coef[na:]) and begin < na and end < na
    c64 = np.asarray(coef[:na], np.float32).astype(np.float64)                       # the float32 coefficients the kernel reads
    aid = O.attn_core(q64[:na], k64[:na], v64[:na], H, scale, mode, fused, c64, begin=begin, end=end,
                      mask=None if m64 is None else m64[:na])
    return aid if na == n else np.concatenate([aid, plain(na, n)])
