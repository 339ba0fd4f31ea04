"""Numpy restatement of the views over regions (DESIGN.md "Views over regions"; the rule of csrc/region_view_plan.h), on top of
render_ref and overlay_ref: the yardstick of tests/test_region_view_host.py and tests/test_gpu_region_views.py.  Written from
the rule, not from the kernels.

  view     (sx, sy, ox, oy) = (o[0] / 512, o[1] / 512, o[5] - o[9], o[2] - o[6]) in fp32
  window   l = o[5], t = o[2], r = W - o[3], b = H - o[4] clamped into the frame (NaN -> 0); pixel x is inside when its centre is:
           x0 = ceil(l - 0.5) <= x < x1 = ceil(r - 0.5)
  draws    frame in [0, n_frames), sx > 0, sy > 0, the window has a pixel
  meshes   render_ref's rules with the view of the MESH and the depth value sx / Z (float64 of the fp32 sx and Z)
  heat map per pixel the maximum of overlay_ref.heatmap_index over the regions whose window holds the pixel, then
           overlay_ref.draw_heatmaps' blend
"""
import numpy as np

import overlay_ref as O
import render_ref as R
from map_view_ref import blend, view_from_offsets

F = np.float32


def _clamp(v, hi):
    v, hi = F(v), F(hi)
    return (v if v < hi else hi) if v > 0 else F(0)      # NaN -> 0


def view_row(o):
    return view_from_offsets(np.asarray(o, F)[None])[0]


def region_view(o, frame, n_frames, H, W):
    """-> dict(view fp32 [4], window (x0, x1, y0, y1) with x1 / y1 exclusive, draws bool)."""
    o = np.asarray(o, F)
    v = view_row(o)
    with np.errstate(all='ignore'):
        l, t = _clamp(o[5], W), _clamp(o[2], H)
        r, b = _clamp(F(W) - o[3], W), _clamp(F(H) - o[4], H)
        x0, x1 = int(np.ceil(l - F(0.5))), int(np.ceil(r - F(0.5)))
        y0, y1 = int(np.ceil(t - F(0.5))), int(np.ceil(b - F(0.5)))
    x1, y1 = max(x1, x0), max(y1, y0)
    draws = bool(0 <= frame < n_frames and v[0] > 0 and v[1] > 0 and x0 < x1 and y0 < y1)
    return dict(view=v, window=(x0, x1, y0, y1), draws=draws)


def mesh_frames(flags, offsets, region_frame, n_frames, H, W):
    """flags bool [n,2] -> (mesh_frame int [2n], mesh_view fp32 [2n,4]): what render_region_prep_kernel writes."""
    n = len(offsets)
    mf, mv = -np.ones(2 * n, np.int64), np.zeros((2 * n, 4), F)
    for i in range(n):
        rv = region_view(offsets[i], int(region_frame[i]), n_frames, H, W)
        for h in (0, 1):
            mv[2 * i + h] = rv['view']
            if rv['draws'] and flags[i][h]:
                mf[2 * i + h] = int(region_frame[i])
    return mf, mv


def render(verts, faces, images, mesh_frame, mesh_view, trans=None, colors=None, focal=1265.0, visible_weight=0.9):
    """render_ref.render with one view row per mesh and the depth value sx / Z: the same dict (out, ids, best, second)."""
    verts = np.asarray(verts, F)
    images = np.asarray(images)
    M = verts.shape[0]
    N, H, W, _ = images.shape
    faces_l = list(faces) if isinstance(faces, (list, tuple)) else [faces] * M
    colors = np.asarray([0.94, 0.71, 0.53] if colors is None else colors, np.float64)
    colors = np.broadcast_to(colors, (M, 3)) if colors.ndim == 1 else colors.reshape(M, 3)
    best = np.zeros((N, H, W)); second = np.zeros((N, H, W))
    ids = -np.ones((N, H, W), np.int64)
    shade = np.zeros((N, H, W))
    ys_, xs_ = np.mgrid[0:H, 0:W]
    PX, PY = (xs_ * R.SUB + R.SUB // 2).astype(np.int64), (ys_ * R.SUB + R.SUB // 2).astype(np.int64)
    base = 0
    for m in range(M):
        f = np.asarray(faces_l[m], np.int64)
        n = int(mesh_frame[m])
        sx = F(mesh_view[m][0])
        if 0 <= n < N and sx > 0:
            xi, yi, Z, ok = R.snap(verts[m], None if trans is None else trans[m], mesh_view[m], focal)
            iz = np.float64(sx) / np.where(ok, Z, 1).astype(np.float64)
            sh = R.vertex_shades(verts[m], f)
            for t, (a, b, c) in enumerate(f):
                if not (ok[a] and ok[b] and ok[c]):
                    continue
                x0, y0, x1, y1, x2, y2 = int(xi[a]), int(yi[a]), int(xi[b]), int(yi[b]), int(xi[c]), int(yi[c])
                area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
                if area == 0:
                    continue
                if area < 0:
                    x1, y1, x2, y2, b, c, area = x2, y2, x1, y1, c, b, -area
                lx, hx = max(0, min(x0, x1, x2) // R.SUB - 1), min(W - 1, max(x0, x1, x2) // R.SUB + 1)
                ly, hy = max(0, min(y0, y1, y2) // R.SUB - 1), min(H - 1, max(y0, y1, y2) // R.SUB + 1)
                if lx > hx or ly > hy:
                    continue
                sl = (n, slice(ly, hy + 1), slice(lx, hx + 1))
                px, py = PX[sl[1:]], PY[sl[1:]]
                w0, i0 = R.edge(x1, y1, x2, y2, px, py)
                w1, i1 = R.edge(x2, y2, x0, y0, px, py)
                w2, i2 = R.edge(x0, y0, x1, y1, px, py)
                inside = i0 & i1 & i2
                if not inside.any():
                    continue
                b0, b1, b2 = w0 / float(area), w1 / float(area), w2 / float(area)
                d = b0 * iz[a] + b1 * iz[b] + b2 * iz[c]
                s = (b0 * iz[a] * sh[a] + b1 * iz[b] * sh[b] + b2 * iz[c] * sh[c]) / np.where(inside, d, 1)
                bb, ss, ii, hh = best[sl], second[sl], ids[sl], shade[sl]
                win = inside & (d > bb)
                lose = inside & ~win & (d > ss)
                ss[win] = bb[win]; bb[win] = d[win]; ii[win] = base + t; hh[win] = s[win]
                ss[lose] = d[lose]
        base += len(f)
    out = images.copy()
    cov = ids >= 0
    mesh_of = np.zeros(ids.shape, np.int64)
    bounds = np.cumsum([0] + [len(np.asarray(faces_l[m])) for m in range(M)])
    mesh_of[cov] = np.searchsorted(bounds, ids[cov], side='right') - 1
    w = float(visible_weight)
    val = w * 255.0 * colors[mesh_of] * shade[..., None] + (1.0 - w) * images.astype(np.float64)
    out[cov] = np.clip(np.floor(val[cov]), 0, 255).astype(np.uint8)
    return {'out': out, 'ids': ids, 'best': best, 'second': second}


def heatmap_indices(maps, offsets, region_frame, N, H, W):
    """maps fp32 [n,h,w] -> idx int [N,H,W], -1 where no region covers the pixel."""
    idx = -np.ones((N, H, W), np.int64)
    for i in range(len(maps)):
        f = int(region_frame[i])
        rv = region_view(offsets[i], f, N, H, W)
        if not rv['draws']:
            continue
        one, inside = O.heatmap_index(maps[i], H, W, rv['view'])
        x0, x1, y0, y1 = rv['window']
        win = np.zeros((H, W), bool)
        win[y0:y1, x0:x1] = True
        cover = inside & win
        idx[f][cover] = np.maximum(idx[f][cover], one[cover].astype(np.int64))
    return idx


def draw_region_heatmaps(maps, images, offsets, region_frame, weight=0.7, lut=None, bgr=False):
    """maps fp32 [n,h,w], images uint8 [N,H,W,3] -> uint8 [N,H,W,3]; the blend of overlay_ref.draw_heatmaps."""
    images = np.asarray(images, np.uint8)
    lut = O.jet_lut(bgr) if lut is None else np.asarray(lut, np.uint8)
    N, H, W, _ = images.shape
    idx = heatmap_indices(np.asarray(maps, F), offsets, region_frame, N, H, W)
    return np.where((idx >= 0)[..., None], blend(weight, lut[np.maximum(idx, 0)], images), images)


def roi_offsets(H, W, box):
    """The `offsets` row of box (l, t, r, b) of an H x W frame, as roi_ref.offsets gives it (fp32 [10])."""
    import roi_ref
    return np.asarray(roi_ref.offsets(H, W, box), F)
