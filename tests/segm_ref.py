"""The part segmentation as an output (csrc/segm_plan.h) restated in numpy: labels, the 'segm' view, the
default colours and the mask statistics.  Everything is float32, every operation rounded on its own, in the order the rule
gives; arrays are NHWC as the library takes them.  The map sampling it shares with the heat-map views is tests/map_view_ref.py."""
import numpy as np

from map_view_ref import blend, canvas, jet, taps, value, view_from_offsets  # noqa: F401 (view_from_offsets, jet: for the tests)

F32 = np.float32
NONE = 255


def labels_one(logits, C, H, W, view=None):
    """logits [h,w,>=C] of one frame -> uint8 [H,W]; view = (sx, sy, ox, oy) or None."""
    logits = np.asarray(logits, F32)
    h, w = logits.shape[:2]
    out = np.full((H, W), NONE, np.uint8)
    if view is not None and not (view[0] > 0 and view[1] > 0):
        return out
    cx = canvas(W, None if view is None else (view[0], view[2]))
    cy = canvas(H, None if view is None else (view[1], view[3]))
    with np.errstate(invalid='ignore'):
        okx, oky = (cx >= 0) & (cx < 512), (cy >= 0) & (cy < 512)
    tx, ty = taps(np.where(okx, cx, F32(0)), w), taps(np.where(oky, cy, F32(0)), h)
    best = lab = None
    with np.errstate(all='ignore'):
        for c in range(C):
            v = value(logits[:, :, c], ty, tx)
            if c == 0:
                best, lab = v, np.zeros((H, W), np.uint8)
            else:
                take = v > best
                best = np.where(take, v, best)
                lab[take] = c
    cov = oky[:, None] & okx[None, :]
    out[cov] = lab[cov]
    return out


def labels(logits, C, H, W, view=None):
    """logits [n,h,w,>=C] -> uint8 [n,H,W]; view [n,4] or None."""
    return np.stack([labels_one(logits[i], C, H, W, None if view is None else np.asarray(view, F32)[i]) for i in range(len(logits))])


def default_colors(C=33, bgr=False):
    lut = jet(bgr)
    half = (C - 1) // 2
    tab = np.zeros((C, 3), np.uint8)
    for label in range(1, C):
        i = 128 + 8 * (label - 1) if label <= half else 127 - 8 * (label - 1 - half)
        tab[label] = lut[min(max(i, 0), 255)]
    return tab


def draw(images, lab, C, colors=None, weight=0.7, bgr=False):
    """images uint8 [n,H,W,3], lab uint8 [n,H,W] -> the view."""
    col = default_colors(C, bgr) if colors is None else np.asarray(colors, np.uint8)
    out = np.array(images, np.uint8, copy=True)
    hand = (lab >= 1) & (lab < C)
    out[hand] = blend(weight, col[np.minimum(lab, C - 1)], out)[hand]
    return out


def side_of(label, C):
    """1 right, 0 left, -1 neither."""
    return -1 if label < 1 or label >= C else (1 if label <= (C - 1) // 2 else 0)


def stats(lab, C, ids=None, n_faces=0):
    """lab uint8 [n,H,W] (ids int32 [n,H,W]) -> counts [n,C], boxes [n,2,4] (r, b exclusive), agree [n,2,3] or None."""
    n, H, W = lab.shape
    side = np.array([side_of(v, C) for v in range(256)])
    counts = np.zeros((n, C), np.int32)
    boxes = np.zeros((n, 2, 4), np.int32)
    agree = None if ids is None else np.zeros((n, 2, 3), np.int32)
    for f in range(n):
        for c in range(C):
            counts[f, c] = int((lab[f] == c).sum())
        sd = side[lab[f]]
        for s in (0, 1):
            mask = sd == s
            if mask.any():
                rows, cols = np.where(mask.any(1))[0], np.where(mask.any(0))[0]
                boxes[f, s] = (cols[0], rows[0], cols[-1] + 1, rows[-1] + 1)
            if ids is not None:
                sil = (ids[f] >= 0) & (((ids[f] // n_faces) & 1) == s)
                agree[f, s] = (int((mask & sil).sum()), int(mask.sum()), int(sil.sum()))
    return counts, boxes, agree
