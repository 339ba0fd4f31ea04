"""TEST INFRASTRUCTURE: numpy statement of the region-of-interest rule (DESIGN.md "Regions of interest"), independent of the
library.  It is the reference's image_crop_pad with a bbox (acr/utils.py:1276-1301):

    l, t, r, b = bbox;  h, w = image.shape[:2]
    crop_trbl = (int(max(0, t)), int(max(0, w - r)), int(max(0, h - b)), int(max(0, l)))          # acr/utils.py:1289-1292
    image = Crop(px=crop_trbl, keep_size=False)(image)     # = image[ct : h - cb, cl : w - cr]      # acr/utils.py:1294-1295
    pad_trbl = compute_paddings_to_reach_aspect_ratio(image.shape, 1.0); image = Pad(px=pad_trbl)  # acr/utils.py:1296-1299
    offsets = [*image.shape[:2], *crop_trbl, *pad_trbl]                                            # acr/utils.py:1301

followed by what img_preprocess does with a frame (acr/utils.py:1315-1337: BGR -> RGB, resize to 512 x 512), which
oracle.preprocess.img_preprocess states.  Two departures, both in DESIGN.md: the pad is white as on the reference's demo path
(image_crop_pad itself pads black), and a window without pixels is an error (imgaug's Crop would keep one pixel)."""
import numpy as np

from oracle import preprocess as opre


def crop_trbl(H, W, box):
    l, t, r, b = box
    return int(max(0, t)), int(max(0, W - r)), int(max(0, H - b)), int(max(0, l))


def window(H, W, box):
    """-> (l, t, r, b) of the clamped window, r and b exclusive, or None when it has no pixels."""
    ct, cr, cb, cl = crop_trbl(H, W, box)
    if H - ct - cb <= 0 or W - cl - cr <= 0:
        return None
    return cl, ct, W - cr, H - cb


def offsets(H, W, box):
    """-> float32 [10] = [padded h, padded w, ct, cr, cb, cl, pt, pr, pb, pl], or None for an empty window."""
    win = window(H, W, box)
    if win is None:
        return None
    l, t, r, b = win
    pad = opre.compute_paddings_to_reach_aspect_ratio((b - t, r - l), 1.0)
    S = max(b - t, r - l)
    return np.array([S, S, *crop_trbl(H, W, box), *pad], np.float32)


def preprocess(bgr, box):
    """One BGR uint8 frame [H,W,3] and a box -> (uint8 RGB [512,512,3], offsets float32 [10]): the oracle's pre-processing of
    the window, the crop entries put into its row."""
    H, W = bgr.shape[:2]
    l, t, r, b = window(H, W, box)
    rgb, row = opre.img_preprocess(np.ascontiguousarray(bgr[t:b, l:r]))
    row = row.copy()
    row[2:6] = crop_trbl(H, W, box)
    assert (row == offsets(H, W, box)).all()
    return rgb, row
