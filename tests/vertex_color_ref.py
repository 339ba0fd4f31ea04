"""Numpy restatement of the per-vertex colour rules, the yardstick of tests/test_gpu_vertex_color.py.
Written from the rules, not from the kernels.

  raster   on top of tests/render_ref.py (coverage, depth test, ids, shade as there): the base colour of a covered pixel is the
           perspective-correct interpolation of the colours of its visible triangle's vertices, in float64:
             base_c = (b0 iz0 c0 + b1 iz1 c1 + b2 iz2 c2) / (b0 iz0 + b1 iz1 + b2 iz2)
             out_c  = clip(floor(w 255 base_c shade + (1 - w) img_c), 0, 255), NaN -> 0
  colours  fp32, op for op: flag != 0 -> the flag colour; NaN -> the mesh's base colour; else t = (v - lo) / (hi - lo) clamped
           to [0, 1], i = int(t * 255), with reverse 255 - i, colour = lut[i] / 255
  values   fp32, op for op: hand (b, k, side) against its K partners in ascending rank - left rank k: pairs (b K + k) K + j,
           direction 0; right rank k: pairs (b K + i) K + k, direction 1; m2 = the smallest d2 (strict < from +inf), value =
           sqrt(m2) or NaN when none; flag = any partner with d2 <= m * m and (s < 0 | cross odd)
"""
import numpy as np

import render_ref as R


def default_lut(bgr=False):
    """The default table of the heat-map views (include/acrmi.h): clamp(383 - |4 i - 255 k|, 0, 255), k = 3, 2, 1 for R, G, B."""
    i = np.arange(256, dtype=np.int64)
    lut = np.stack([np.clip(383 - np.abs(4 * i - 255 * k), 0, 255) for k in (3, 2, 1)], 1).astype(np.uint8)
    return np.ascontiguousarray(lut[:, ::-1]) if bgr else lut


def render(verts, faces, images, vcol, mesh_frame=None, trans=None, view=None, focal=1265.0, visible_weight=0.9):
    """render_ref.render with a colour per vertex: vcol [M,V,3].  -> its dict, 'out' painted by the rule above."""
    verts = np.asarray(verts, np.float32)
    images = np.asarray(images)
    vcol = np.asarray(vcol, np.float32).astype(np.float64)
    M = verts.shape[0]
    N = images.shape[0]
    ref = R.render(verts, faces, images, mesh_frame=mesh_frame, trans=trans, view=view, focal=focal, visible_weight=visible_weight)
    faces_l = [np.asarray(f, np.int64) for f in (list(faces) if isinstance(faces, (list, tuple)) else [faces] * M)]
    if mesh_frame is None:
        mesh_frame = np.arange(M) // (M // N)
    bounds = np.cumsum([0] + [len(f) for f in faces_l])
    out = images.copy()
    w = float(visible_weight)
    ids = ref['ids']
    with np.errstate(all='ignore'):
        for m in range(M):
            n = int(mesh_frame[m])
            if n < 0:
                continue
            mine = (ids[n] >= bounds[m]) & (ids[n] < bounds[m + 1])
            if not mine.any():
                continue
            xi, yi, Z, ok = R.snap(verts[m], None if trans is None else trans[m], None if view is None else view[n], focal)
            iz = 1.0 / np.where(ok, Z, 1).astype(np.float64)
            sh = R.vertex_shades(verts[m], faces_l[m])
            ys, xs = np.nonzero(mine)
            local = ids[n][ys, xs] - bounds[m]
            for t in np.unique(local):
                sel = local == t
                y, x = ys[sel], xs[sel]
                a, b, c = (int(i) for i in faces_l[m][t])
                x0, y0, x1, y1, x2, y2 = int(xi[a]), int(yi[a]), int(xi[b]), int(yi[b]), int(xi[c]), int(yi[c])
                area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
                if area < 0:
                    x1, y1, x2, y2, b, c, area = x2, y2, x1, y1, c, b, -area
                px, py = x.astype(np.int64) * R.SUB + R.SUB // 2, y.astype(np.int64) * R.SUB + R.SUB // 2
                e0, i0 = R.edge(x1, y1, x2, y2, px, py)
                e1, i1 = R.edge(x2, y2, x0, y0, px, py)
                e2, i2 = R.edge(x0, y0, x1, y1, px, py)
                assert (i0 & i1 & i2).all(), 'the visible triangle does not cover its pixel'
                w0, w1, w2 = e0 / float(area) * iz[a], e1 / float(area) * iz[b], e2 / float(area) * iz[c]
                d = w0 + w1 + w2
                shade = (w0 * sh[a] + w1 * sh[b] + w2 * sh[c]) / d
                base = (w0[:, None] * vcol[m, a] + w1[:, None] * vcol[m, b] + w2[:, None] * vcol[m, c]) / d[:, None]
                val = np.floor(w * 255.0 * base * shade[:, None] + (1.0 - w) * images[n, y, x].astype(np.float64))
                out[n, y, x] = np.where(np.isnan(val), 0, np.clip(val, 0, 255)).astype(np.uint8)
    return dict(ref, out=out)


def vertex_colors(values, lo, hi, flags=None, base=None, flag_color=(1, 0, 1), lut=None, reverse=False, bgr=False):
    """values [M,V] -> fp32 [M,V,3], op for op in fp32."""
    f32 = np.float32
    v = np.asarray(values, f32)
    M, V = v.shape
    lut = default_lut(bgr) if lut is None else np.asarray(lut, np.uint8)
    base = np.broadcast_to(np.asarray([0.94, 0.71, 0.53] if base is None else base, f32).reshape(-1, 3), (M, 3))
    with np.errstate(all='ignore'):
        t = (v - f32(lo)) / (f32(hi) - f32(lo))
        t = np.where(t < 0, f32(0), np.where(t > 1, f32(1), t)).astype(f32)
        i = np.where(np.isnan(t), 0, (np.where(np.isnan(t), f32(0), t) * f32(255))).astype(np.int64)      # (int) truncates
    if reverse:
        i = 255 - i
    col = (lut[i].astype(f32) / f32(255)).astype(f32)
    col = np.where(np.isnan(v)[..., None], base[:, None, :], col)
    if flags is not None:
        col = np.where((np.asarray(flags) != 0)[..., None], np.asarray(flag_color, f32), col)
    return np.ascontiguousarray(col.astype(f32))


def contact_values(d2, other, B, K, max_depth, surface=False):
    """d2 [B*K*K,2,V] and `other` shaped alike (s fp32, or cross int32 with surface) -> (value fp32, flag int32) [B,K,2,V]."""
    f32 = np.float32
    d2 = np.asarray(d2, f32)
    V = d2.shape[2]
    lim = f32(max_depth) * f32(max_depth)
    value = np.empty((B, K, 2, V), f32)
    flag = np.zeros((B, K, 2, V), np.int32)
    with np.errstate(all='ignore'):
        for b in range(B):
            for k in range(K):
                for side in (0, 1):
                    m2 = np.full(V, np.inf, f32)
                    fl = np.zeros(V, bool)
                    for q in range(K):
                        p = (b * K + k) * K + q if side == 0 else (b * K + q) * K + k
                        d = d2[p, side]
                        m2 = np.where(d < m2, d, m2)
                        inside = (np.asarray(other[p, side]) & 1) != 0 if surface else np.asarray(other[p, side], f32) < 0
                        fl |= (d <= lim) & inside
                    value[b, k, side] = np.where(m2 < np.inf, np.sqrt(m2, dtype=f32), f32(np.nan))
                    flag[b, k, side] = fl
    return value, flag
