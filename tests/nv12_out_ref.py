"""TEST INFRASTRUCTURE: numpy statement of the NV12 output rule (include/acrmi.h, DESIGN.md "NV12 output"), independent of the
library: its own literal copy of the five coefficient tables, the formula that makes the four bt* rows, int64 arithmetic with
the int32 range asserted.

For a row (cry, cgy, cby, cru, cgu, cbu, crv, cgv, cbv, y_off), an arithmetic right shift and a clamp to 0..255:
    per pixel:      Y = clamp((cry R + cgy G + cby B + (y_off << 20) + (1 << 19)) >> 20)
    per 2x2 block:  R4, G4, B4 = the sums of the four pixels' R, G, B
                    U = clamp((cru R4 + cgu G4 + cbu B4 + (128 << 22) + (1 << 21)) >> 22)
                    V = clamp((crv R4 + cgv G4 + cbv B4 + (128 << 22) + (1 << 21)) >> 22)
Compose: a pixel is changed when its drawn triple differs from what the input rule (tests/nv12_ref.py) makes of the source;
out Y = Y(drawn) for a changed pixel, else the source byte; out U, V = U, V(the block's four drawn triples) when any pixel of
the block is changed, else the source bytes."""
from fractions import Fraction

import numpy as np

import nv12_ref as N

MATRICES = {
    'cv601': (269484, 528482, 102760, -155188, -305135, 460324, 460324, -385875, -74448, 16),
    'bt601': (269262, 528618, 102662, -155423, -305128, 460551, 460551, -385654, -74897, 16),
    'bt601-full': (313524, 615514, 119538, -176932, -347356, 524288, 524288, -439026, -85262, 0),
    'bt709': (191455, 644067, 65019, -105533, -355018, 460551, 460551, -418321, -42230, 16),
    'bt709-full': (222927, 749942, 75707, -120138, -404150, 524288, 524288, -476214, -48074, 0),
}
KR_KB = {'bt601': (Fraction(299, 1000), Fraction(114, 1000)), 'bt709': (Fraction(2126, 10000), Fraction(722, 10000))}


def _round(x):
    """round half away from zero of an exact fraction (no row lands on a half)"""
    x = Fraction(x)
    n = int(abs(x) + Fraction(1, 2))
    return n if x >= 0 else -n


def formula_row(name):
    """round(x * 2^20) of the textbook forms: luma Kr, Kg, Kb (times 219/255 in limited range); chroma
    -0.5 Kr/(1-Kb), -0.5 Kg/(1-Kb), 0.5 for U and 0.5, -0.5 Kg/(1-Kr), -0.5 Kb/(1-Kr) for V (times 224/255 in limited range)."""
    full = name.endswith('-full')
    kr, kb = KR_KB[name.replace('-full', '')]
    kg = 1 - kr - kb
    gy = Fraction(1) if full else Fraction(219, 255)
    gc = Fraction(1) if full else Fraction(224, 255)
    half = Fraction(1, 2)
    coef = [kr * gy, kg * gy, kb * gy,
            -half * kr / (1 - kb) * gc, -half * kg / (1 - kb) * gc, half * gc,
            half * gc, -half * kg / (1 - kr) * gc, -half * kb / (1 - kr) * gc]
    return tuple(_round(c * 2 ** 20) for c in coef) + (0 if full else 16,)


def row_of(matrix):
    return tuple(int(c) for c in (MATRICES[matrix] if isinstance(matrix, str) else matrix))


def row_ok(row):
    """The host's check: y_off in 0..255 and int32 sums."""
    c = [int(v) for v in row]
    if not 0 <= c[9] <= 255:
        return False
    if 255 * sum(abs(v) for v in c[0:3]) + (c[9] << 20) + 2 ** 19 >= 2 ** 31:
        return False
    return 1020 * max(sum(abs(v) for v in c[3:6]), sum(abs(v) for v in c[6:9])) + (128 << 22) + 2 ** 21 < 2 ** 31


def luma(R, G, B, row='cv601'):
    c = row_of(row)
    s = c[0] * np.asarray(R, np.int64) + c[1] * np.asarray(G, np.int64) + c[2] * np.asarray(B, np.int64) + (c[9] << 20) + (1 << 19)
    assert np.abs(s).max() < 2 ** 31, 'the rule is defined in int32'
    return np.clip(s >> 20, 0, 255).astype(np.uint8)


def chroma(R4, G4, B4, row='cv601'):
    """The sums of a block's four R, G, B -> (U, V)."""
    c = row_of(row)
    R4, G4, B4 = (np.asarray(v, np.int64) for v in (R4, G4, B4))
    out = []
    for a, b, d in (c[3:6], c[6:9]):
        s = a * R4 + b * G4 + d * B4 + (128 << 22) + (1 << 21)
        assert np.abs(s).max() < 2 ** 31, 'the rule is defined in int32'
        out.append(np.clip(s >> 22, 0, 255).astype(np.uint8))
    return tuple(out)


def _planes(img, bgr):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3 and img.shape[0] % 2 == 0 and img.shape[1] % 2 == 0
    R, G, B = (img[:, :, 2 - i] if bgr else img[:, :, i] for i in range(3))
    return R.astype(np.int64), G.astype(np.int64), B.astype(np.int64)


def _block_sums(p):
    return p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]


def to_nv12(img, row='cv601', bgr=True):
    """uint8 [H,W,3] -> (y [H,W], uv [H/2,W]) by the rule."""
    R, G, B = _planes(img, bgr)
    U, V = chroma(_block_sums(R), _block_sums(G), _block_sums(B), row)
    return luma(R, G, B, row), np.stack([U, V], -1).reshape(R.shape[0] // 2, R.shape[1])


def compose(y, uv, drawn, row6='cv601', row10='cv601', bgr=True):
    """Source planes y [H,W], uv [H/2,W], the drawn frame [H,W,3] -> (y, uv) of the composed surface."""
    y, uv = np.asarray(y), np.asarray(uv)
    H, W = y.shape
    shown = N.nv12_to_bgr(y, uv, row6)
    if not bgr:
        shown = shown[:, :, ::-1]
    changed = (np.asarray(drawn) != shown).any(-1)
    any_changed = changed[0::2, 0::2] | changed[0::2, 1::2] | changed[1::2, 0::2] | changed[1::2, 1::2]
    new_y, new_uv = to_nv12(drawn, row10, bgr)
    out_y = np.where(changed, new_y, y)
    out_uv = np.where(any_changed[:, :, None], new_uv.reshape(H // 2, W // 2, 2), uv.reshape(H // 2, W // 2, 2))
    return out_y, out_uv.reshape(H // 2, W)


def surface(y, uv):
    return np.concatenate([y, uv], 0)


# ---- rows at the limits of the host's check (tests/test_nv12_out_host.py, tests/test_gpu_nv12_out.py) ----------------------
# The smallest magnitudes the issue's two inequalities refuse: 255 m + (16 << 20) + 2^19 >= 2^31 and
# 1020 m + (128 << 22) + 2^21 >= 2^31
LUMA_LIMIT = -((-(2 ** 31 - (16 << 20) - 2 ** 19)) // 255)
CHROMA_LIMIT = -((-(2 ** 31 - (128 << 22) - 2 ** 21)) // 1020)
assert (LUMA_LIMIT, CHROMA_LIMIT) == (8353656, 1576977)
# rows the host must refuse, with the word its message carries
REFUSED_ROWS = [
    ((1, 1, 1, 1, 1, 1, 1, 1, 1, -1), 'y_off'),
    ((1, 1, 1, 1, 1, 1, 1, 1, 1, 256), 'y_off'),
    ((2 ** 23, 2 ** 20, 0, 0, 0, 0, 0, 0, 0, 0), 'luma'),
    ((-(2 ** 23), -(2 ** 20), 0, 0, 0, 0, 0, 0, 0, 0), 'luma'),
    ((LUMA_LIMIT, 0, 0, 0, 0, 0, 0, 0, 0, 16), 'luma'),
    ((0, -LUMA_LIMIT + 5, -5, 0, 0, 0, 0, 0, 0, 16), 'luma'),
    ((0, 0, 0, CHROMA_LIMIT, 0, 0, 0, 0, 0, 0), 'chroma'),
    ((0, 0, 0, 0, 0, 0, -CHROMA_LIMIT // 3, -CHROMA_LIMIT // 3, -CHROMA_LIMIT // 3, 0), 'chroma'),
    ((-2 ** 31, 0, 0, 0, 0, 0, 0, 0, 0, 0), 'luma'),
]
assert CHROMA_LIMIT % 3 == 0
# the nearest rows it must take
ACCEPTED_ROWS = [
    (1, 1, 1, 1, 1, 1, 1, 1, 1, 0), (1, 1, 1, 1, 1, 1, 1, 1, 1, 255),
    (LUMA_LIMIT - 1, 0, 0, 0, 0, 0, 0, 0, 0, 16), (0, -LUMA_LIMIT + 5, -4, 0, 0, 0, 0, 0, 0, 16),
    (0, 0, 0, CHROMA_LIMIT - 1, 0, 0, 0, 0, 0, 0),
    (0, 0, 0, 0, 0, 0, -CHROMA_LIMIT // 3, -CHROMA_LIMIT // 3, -CHROMA_LIMIT // 3 + 1, 0),
]
