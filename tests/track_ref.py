"""Shared by tests/test_track_host.py and tests/test_gpu_track.py: the seeded point mixture and the yardstick of the box rule
(DESIGN.md "Tracking on the device") - acr.utils.boxes_from_keypoints, the numpy function a host loop uses, with the rows that
have no pixels replaced by the whole frame, which is the one clause the device rule adds."""
import numpy as np

from conftest import pkg

FRAMES = [(1, 1), (37, 53), (1080, 1920)]      # H x W
SCALES = [1.0, 1.5, 2.25]
MIN_SIZES = [1, 64, 5000]
SPECIALS = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38], np.float32)


def points(g, k, H, W):
    """k fp32 points for an H x W frame: per coordinate inside the frame, up to 3 frame sizes outside, or an exact integer or
    half; 12 % of the calls get one to three NaN / inf / -inf / 3e38 / -3e38 coordinates on top (mostly the kinds a point is
    dropped for), and 2 % consist of +-3e38 only - the case in which the side is lost against the centre."""
    size = np.array([W, H], np.float64)
    kind = g.choice(3, size=(k, 2), p=[0.6, 0.25, 0.15])
    inside = g.random((k, 2)) * size
    outside = (g.random((k, 2)) * 7 - 3) * size
    halves = np.round((g.random((k, 2)) * 3 - 1) * size * 2) / 2
    pts = np.where(kind == 0, inside, np.where(kind == 1, outside, halves)).astype(np.float32)
    u = g.random()
    if u < 0.02:
        pts[:] = g.choice(SPECIALS[3:], size=(1, 2))
    elif u < 0.14:
        for _ in range(int(g.integers(1, 4))):
            pts[g.integers(0, k), g.integers(0, 2)] = g.choice(SPECIALS, p=[0.35, 0.25, 0.25, 0.075, 0.075])
    return pts


def items(seed, count):
    """[(points fp32 [k,2] with k in 1..42, (H, W), scale, min_size)]"""
    g = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        H, W = FRAMES[int(g.integers(0, len(FRAMES)))]
        out.append((points(g, int(g.integers(1, 43)), H, W), (H, W), SCALES[int(g.integers(0, 3))], MIN_SIZES[int(g.integers(0, 3))]))
    return out


def boxes(point_sets, frame_hw, scale, min_size):
    """boxes_from_keypoints on fp32 point sets (one [k,2] array per item, k may be 0) -> (int32 [n,4] with the rows that have no
    pixels replaced by the whole frame, the bool mask of the replaced rows)."""
    f = pkg('acr.utils').boxes_from_keypoints
    hw = np.broadcast_to(np.asarray(frame_hw, np.int64), (len(point_sets), 2))
    got = f([np.asarray(p, np.float32).astype(np.float64).reshape(-1, 2) for p in point_sets], hw, scale=scale, min_size=min_size)
    empty = (got[:, 2] <= got[:, 0]) | (got[:, 3] <= got[:, 1])
    got[empty] = np.stack([np.zeros_like(hw[:, 0]), np.zeros_like(hw[:, 0]), hw[:, 1], hw[:, 0]], 1)[empty]
    return got, empty
