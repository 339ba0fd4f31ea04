"""How a network map is drawn over frames (csrc/map_view_plan.h) restated in numpy, for overlay_ref, region_view_ref and
segm_ref: the view row of an `offsets` row, canvas coordinates, taps, the bilinear value, the jet and the blend.  Everything is
float32, every operation rounded on its own, in the order the rule gives.  No GPU, no torch."""
import numpy as np

F = np.float32


def view_from_offsets(o):
    """`offsets` rows [n,10] -> view rows (sx, sy, ox, oy) [n,4]."""
    o = np.asarray(o, F)
    with np.errstate(all='ignore'):
        return np.stack([o[:, 0] / F(512), o[:, 1] / F(512), o[:, 5] - o[:, 9], o[:, 2] - o[:, 6]], 1).astype(F)


def canvas(size, view=None):
    """Canvas coordinate of the pixels 0..size-1 along one axis; view = (scale, shift) or None."""
    x = np.arange(size, dtype=F) + F(0.5)
    with np.errstate(all='ignore'):
        if view is None:
            return (x * (F(512) / F(size))).astype(F)
        return ((x - F(view[1])) / F(view[0])).astype(F)


def taps(c, n):
    """map_tap: (i0, i1, l0, l1) of canvas coordinates c (finite) on a map of n cells."""
    s = np.maximum(c * (F(n) / F(512)) - F(0.5), F(0)).astype(F)
    i0 = np.minimum(s.astype(np.int64), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    l1 = (s - i0.astype(F)).astype(F)
    l0 = (F(1) - l1).astype(F)
    return i0, i1, l0, l1


def value(m, ty, tx):
    """The bilinear value of map m [h,w] at every (row tap, column tap): fp32 [len(ty), len(tx)]."""
    (y0, y1, ly0, ly1), (x0, x1, lx0, lx1) = ty, tx
    lx0, lx1, ly0, ly1 = lx0[None, :], lx1[None, :], ly0[:, None], ly1[:, None]
    with np.errstate(all='ignore'):
        top = (lx0 * m[np.ix_(y0, x0)]).astype(F) + (lx1 * m[np.ix_(y0, x1)]).astype(F)
        bot = (lx0 * m[np.ix_(y1, x0)]).astype(F) + (lx1 * m[np.ix_(y1, x1)]).astype(F)
        v = (ly0 * top).astype(F) + (ly1 * bot).astype(F)
    assert v.dtype == np.float32
    return v


def jet(bgr=False):
    """byte = clamp(383 - |4 i - 255 k|, 0, 255), k = 3, 2, 1 for red, green, blue: uint8 [256,3]."""
    i = np.arange(256, dtype=np.int64)
    lut = np.stack([np.clip(383 - np.abs(4 * i - 255 * k), 0, 255) for k in (3, 2, 1)], 1).astype(np.uint8)
    return np.ascontiguousarray(lut[:, ::-1]) if bgr else lut


def blend(weight, colour, img):
    """floor(weight * colour + (1 - weight) * img) of uint8 arrays -> uint8."""
    w = F(weight)
    o = np.floor((w * colour.astype(F)).astype(F) + ((F(1) - w) * img.astype(F)).astype(F))
    assert o.dtype == np.float32
    return o.astype(np.uint8)
