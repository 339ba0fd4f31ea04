"""TEST INFRASTRUCTURE: numpy statement of the NV12 colour rule (include/acrmi.h, DESIGN.md "NV12 input"), independent of
the library: its own literal copy of the five coefficient tables, int64 arithmetic with the int32 range asserted.

For bytes Y, U, V and a row (cy, cub, cug, cvg, cvr, y_off); chroma is nearest (a 2x2 block of luma shares one U, V pair):
    y = max(0, Y - y_off) * cy;  u = U - 128;  v = V - 128;  r = 1 << 19
    R = clamp((y + cvr v + r) >> 20);  G = clamp((y + cug u + cvg v + r) >> 20);  B = clamp((y + cub u + r) >> 20)
with an arithmetic right shift and a clamp to 0..255."""
import numpy as np

from oracle import preprocess as opre

MATRICES = {
    'cv601': (1220542, 2116026, -409993, -852492, 1673527, 16),
    'bt601': (1220945, 2115221, -410793, -852458, 1673555, 16),
    'bt601-full': (1048576, 1858077, -360853, -748826, 1470104, 0),
    'bt709': (1220945, 2215014, -223607, -558796, 1879825, 16),
    'bt709-full': (1048576, 1945738, -196424, -490864, 1651297, 0),
}


def row_of(matrix):
    return tuple(int(c) for c in (MATRICES[matrix] if isinstance(matrix, str) else matrix))


def yuv_to_rgb(Y, U, V, row='cv601'):
    """Arrays (or scalars) of bytes -> (R, G, B) uint8 arrays by the rule."""
    cy, cub, cug, cvg, cvr, y_off = row_of(row)
    y = np.maximum(0, np.asarray(Y, np.int64) - y_off) * cy
    u = np.asarray(U, np.int64) - 128
    v = np.asarray(V, np.int64) - 128
    r = 1 << 19
    sums = (y + cvr * v + r, y + cug * u + cvg * v + r, y + cub * u + r)
    for s in sums:
        assert np.abs(s).max() < 2 ** 31, 'the rule is defined in int32'
    return tuple(np.clip(s >> 20, 0, 255).astype(np.uint8) for s in sums)       # numpy's >> on int64 is arithmetic


def nv12_to_bgr(y, uv, row='cv601'):
    """y uint8 [H,W], uv uint8 [H/2,W] (U at even bytes, V at odd) or [H/2,W/2,2] -> BGR uint8 [H,W,3]."""
    y = np.asarray(y)
    H, W = y.shape
    uv = np.asarray(uv).reshape(H // 2, W // 2, 2)
    U = np.repeat(np.repeat(uv[:, :, 0], 2, 0), 2, 1)
    V = np.repeat(np.repeat(uv[:, :, 1], 2, 0), 2, 1)
    R, G, B = yuv_to_rgb(y, U, V, row)
    return np.stack([B, G, R], -1)


def preprocess(y, uv, row='cv601'):
    """-> (uint8 RGB [512,512,3], offsets float32 [10]): the oracle's pre-processing of the converted frame."""
    return opre.img_preprocess(nv12_to_bgr(y, uv, row))


def random_nv12(H, W, seed):
    """Seeded random bytes over the full 0..255 range -> (y [H,W], uv [H/2,W])."""
    g = np.random.default_rng(seed)
    return g.integers(0, 256, (H, W), dtype=np.uint8), g.integers(0, 256, (H // 2, W), dtype=np.uint8)
