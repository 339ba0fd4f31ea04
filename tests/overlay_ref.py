"""numpy restatement of the key-point skeleton and heat-map views (DESIGN.md "Key-point and heat-map views"; the rules are
written out in include/acrmi.h).  No GPU, no torch: the yardstick csrc/overlay.hip is held to byte for byte.

Skeleton: integers only (numpy int64; with |k| < 16384 and pixel coordinates < 16384 every term fits: u.d and u x d are
below 2^32, |d|^2 below 2^32, 4 (u x d)^2 below 2^38 once |u x d| >= 2^18 is rejected, w^2 |d|^2 below 2^39 for w <= 11).
Heat map: np.float32 arrays throughout, so every operation is rounded on its own, in the order the rule states; canvas, taps,
value, jet and blend are tests/map_view_ref.py's, which segm_ref shares."""
import numpy as np

from map_view_ref import blend, canvas, jet as jet_lut, taps, value

PARENTS = (1, 2, 3, 20, 5, 6, 7, 20, 9, 10, 11, 20, 13, 14, 15, 20, 17, 18, 19, 20, -1)
MAPPER = (4, 3, 2, 1, 8, 7, 6, 5, 12, 11, 10, 9, 16, 15, 14, 13, 20, 19, 18, 17, 0)
COLORS_RGB = ((230, 230, 0), (255, 51, 51), (255, 102, 102), (255, 153, 153),
              (230, 230, 0), (51, 255, 51), (102, 255, 102), (153, 255, 153),
              (230, 230, 0), (255, 153, 51), (255, 178, 102), (255, 204, 153),
              (230, 230, 0), (51, 153, 255), (102, 178, 255), (153, 204, 255),
              (230, 230, 0), (255, 51, 255), (255, 102, 255), (255, 153, 255), (230, 230, 0))
COORD_LIMIT = 16384
CROSS_LIMIT = 1 << 18
F = np.float32


def default_colors(bgr=False):
    c = np.array(COLORS_RGB, np.uint8)
    return np.ascontiguousarray(c[:, ::-1]) if bgr else c


# ---- skeleton ---------------------------------------------------------------------------------------------------------
def snap_hand(kp):
    """kp fp32 [21,2] in MANO order -> (k int64 [21,2] in skeleton order, far bool [21]); None: the hand is not drawn."""
    kp = np.asarray(kp, np.float32)[list(MAPPER)]
    if not np.isfinite(kp).all():
        return None
    far = (np.abs(kp) >= COORD_LIMIT).any(1)
    k = np.where(far[:, None], 0, np.trunc(kp)).astype(np.int64)      # truncation toward zero
    return k, far


def primitives(kp, line_width=3, circle_rad=3):
    """The primitives of one hand in painter's order, dropped ones left out:
    ('bone', (ax, ay), (bx, by), colour index) and ('disc', (kx, ky), colour index)."""
    snapped = snap_hand(kp)
    if snapped is None:
        return []
    k, far = snapped
    prims = []
    for i in range(21):
        p = PARENTS[i]
        if p >= 0:
            if not far[i] and not far[p] and (k[i] != k[p]).any():
                prims.append(('bone', tuple(int(v) for v in k[i]), tuple(int(v) for v in k[p]), p))
        if not far[i]:
            prims.append(('disc', tuple(int(v) for v in k[i]), i))
        if p >= 0 and not far[p]:
            prims.append(('disc', tuple(int(v) for v in k[p]), p))
    return prims


def prim_mask(prim, x, y, line_width=3, circle_rad=3):
    """Coverage of the pixels (x, y) (int64 arrays, broadcast against each other)."""
    if prim[0] == 'disc':
        (kx, ky) = prim[1]
        return (x - kx) ** 2 + (y - ky) ** 2 <= circle_rad * circle_rad + circle_rad
    (ax, ay), (bx, by) = prim[1], prim[2]
    dx, dy = bx - ax, by - ay
    L2 = dx * dx + dy * dy
    ux, uy = x - ax, y - ay
    dot = ux * dx + uy * dy
    cr = np.abs(ux * dy - uy * dx)
    near = cr < CROSS_LIMIT
    cr = np.where(near, cr, 0)
    return (dot >= 0) & (dot <= L2) & near & (4 * cr * cr <= line_width * line_width * L2)


def prim_window(prim, H, W, line_width=3, circle_rad=3):
    """A pixel box outside which the primitive covers nothing (a covered pixel is within r of the centre, respectively within
    w / 2 of the segment), clipped to the image: x0, x1, y0, y1 inclusive, or None."""
    if prim[0] == 'disc':
        xs, ys, m = (prim[1][0],), (prim[1][1],), circle_rad
    else:
        xs, ys, m = (prim[1][0], prim[2][0]), (prim[1][1], prim[2][1]), line_width
    x0, x1, y0, y1 = max(min(xs) - m, 0), min(max(xs) + m, W - 1), max(min(ys) - m, 0), min(max(ys) + m, H - 1)
    return (x0, x1, y0, y1) if x0 <= x1 and y0 <= y1 else None


def draw_hand(img, kp, colors, line_width=3, circle_rad=3, windowed=True):
    """Draws one hand into img (uint8 [H,W,3], modified in place); the last primitive that covers a pixel wins."""
    H, W = img.shape[:2]
    for prim in primitives(kp, line_width, circle_rad):
        box = prim_window(prim, H, W, line_width, circle_rad) if windowed else (0, W - 1, 0, H - 1)
        if box is None:
            continue
        x0, x1, y0, y1 = box
        x = np.arange(x0, x1 + 1, dtype=np.int64)[None, :]
        y = np.arange(y0, y1 + 1, dtype=np.int64)[:, None]
        m = prim_mask(prim, x, y, line_width, circle_rad)
        img[y0:y1 + 1, x0:x1 + 1][m] = colors[prim[-1]]
    return img


def draw_skeletons(kps, images, hand_frame=None, colors=None, line_width=3, circle_rad=3, bgr=False, windowed=True):
    """kps fp32 [M,21,2], images uint8 [N,H,W,3] -> the drawn copy.  Hands are drawn in hand order."""
    kps = np.asarray(kps, np.float32)
    out = np.array(images, np.uint8, copy=True)
    M, N = len(kps), len(out)
    if hand_frame is None:
        hand_frame = np.arange(M) // (M // N)
    colors = default_colors(bgr) if colors is None else np.asarray(colors, np.uint8)
    for m in range(M):
        f = int(hand_frame[m])
        if 0 <= f < N:
            draw_hand(out[f], kps[m], colors, line_width, circle_rad, windowed)
    return out


# ---- heat maps --------------------------------------------------------------------------------------------------------
def jet_lut_formula():
    """The same table from the stated formula in exact rationals: floor(255 clamp(3/2 - |4 t - k|, 0, 1) + 1/2), t = i / 255
    (in floating point t is inexact and the half-way values fall either way)."""
    from fractions import Fraction
    import math
    lut = np.zeros((256, 3), np.uint8)
    for i in range(256):
        t = Fraction(i, 255)
        for c, k in enumerate((3, 2, 1)):
            v = min(max(Fraction(3, 2) - abs(4 * t - k), Fraction(0)), Fraction(1))
            lut[i, c] = math.floor(255 * v + Fraction(1, 2))
    return lut


def heatmap_index(m, H, W, view=None):
    """One map fp32 [h,w] -> (idx uint8 [H,W], inside bool [H,W]); view = (sx, sy, ox, oy) or None."""
    m = np.asarray(m, np.float32)
    h, w = m.shape
    if view is None:
        cx, cy, ok = canvas(W), canvas(H), True
    else:
        sx, sy, ox, oy = (F(v) for v in view)
        cx, cy = canvas(W, (sx, ox)), canvas(H, (sy, oy))
        ok = bool(sx > 0) and bool(sy > 0)
    with np.errstate(invalid='ignore'):
        in_x = (cx >= 0) & (cx < 512) & ok
        in_y = (cy >= 0) & (cy < 512) & ok
    v = value(m, taps(np.where(in_y, cy, F(0)), h), taps(np.where(in_x, cx, F(0)), w))
    with np.errstate(all='ignore'):
        t = v * F(255)
        t = np.where(np.isnan(t), F(0), t)
        idx = np.minimum(np.maximum(t, F(0)), F(255)).astype(np.uint8)      # truncates
    return idx, in_y[:, None] & in_x[None, :]


def draw_heatmaps(maps, images, view=None, weight=0.7, lut=None, bgr=False):
    """maps fp32 [n,h,w], images uint8 [n,H,W,3], view [n,4] or None -> uint8 [n,H,W,3]."""
    images = np.asarray(images, np.uint8)
    lut = jet_lut(bgr) if lut is None else np.asarray(lut, np.uint8)
    n, H, W, _ = images.shape
    out = images.copy()
    for i in range(n):
        idx, inside = heatmap_index(maps[i], H, W, None if view is None else np.asarray(view, np.float32)[i])
        out[i] = np.where(inside[..., None], blend(weight, lut[idx], images[i]), images[i])
    return out


def gaussian_maps(n, h, w, seed, peaks=2):
    """Synthetic centre maps: a few Gaussian peaks of height <= 1 per map, fp32 [n,h,w]."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    m = np.zeros((n, h, w), np.float32)
    for i in range(n):
        for _ in range(peaks):
            cx, cy, s, a = rs.uniform(0, w), rs.uniform(0, h), rs.uniform(1.0, 4.0), rs.uniform(0.3, 1.0)
            m[i] = np.maximum(m[i], (a * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))).astype(np.float32))
    return m


def random_hands(n, H, W, seed, spread=0.25):
    """n plausible hands as fp32 [n,21,2] pixel key points in MANO order: a wrist and five chains of four joints."""
    rs = np.random.RandomState(seed)
    kps = np.zeros((n, 21, 2), np.float32)
    size = min(H, W)
    for m in range(n):
        wrist = rs.uniform(0.15, 0.85, 2) * (W, H)
        ang0 = rs.uniform(0, 2 * np.pi)
        kps[m, 0] = wrist
        for fng in range(5):
            ang = ang0 + (fng - 2) * 0.35 + rs.normal(0, 0.08)
            p = wrist.copy()
            for j in range(4):
                step = size * spread * (0.45 if j == 0 else 0.2) * rs.uniform(0.7, 1.3)
                ang += rs.normal(0, 0.25)
                p = p + step * np.array([np.cos(ang), np.sin(ang)])
                kps[m, 1 + 4 * fng + j] = p
    return kps
