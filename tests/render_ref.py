"""Numpy restatement of the mesh overlay's rules (DESIGN.md "Rendering"), the yardstick of tests/test_gpu_render.py.
Written from those rules, not from the kernel: integer coverage (exact), float64 depth and shading, and per pixel the
best and the second-best 1/Z so that a test can tell which pixels an fp32 depth test cannot be asked to order.

Rules restated here:
  camera     P = v + trans (fp32); canvas x = 256 + (f X) / Z, y = 256 + (f Y) / Z (fp32, every operation rounded)
  viewport   x' = x * view[0] + view[2], y' = y * view[1] + view[3] (fp32); identity without a view
  snapping   round-to-nearest of x' * 256 (1/256 pixel); pixel centres at (i + 0.5)
  dropped    zero area; a vertex with Z <= 0.05; a snapped coordinate beyond +-2^22
  coverage   triangle re-oriented to positive area; edge value > 0, or == 0 on a left edge (A > 0) or a top edge
             (A == 0, B > 0) where the edge function is A x + B y + C
  depth      1/Z linear in screen space from the integer edge values; larger wins, strict > (lower face id wins a tie)
  shading    vertex normal = sum of un-normalised face normals over the vertex's incident faces; s = 0.3 + 0.7 |n_z|
             (0.3 when the sum is zero); perspective-correct interpolation
  colour     covered: floor(w 255 base s + (1 - w) img), clipped to [0, 255]; uncovered: img
"""
import numpy as np

SUB = 256
LIMIT = 1 << 22
Z_NEAR = np.float32(0.05)


def ellipsoid(nlat, nlon, semi_axes, centre):
    """Closed lat-long mesh: 2 + (nlat - 1) * nlon vertices, 2 * nlon * (nlat - 1) faces."""
    v = [[0, 0, 1.0]]
    for i in range(1, nlat):
        t = np.pi * i / nlat
        for j in range(nlon):
            p = 2 * np.pi * j / nlon
            v.append([np.sin(t) * np.cos(p), np.sin(t) * np.sin(p), np.cos(t)])
    v.append([0, 0, -1.0])
    v = np.array(v) * np.array(semi_axes) + np.array(centre)
    f = [[0, 1 + j, 1 + (j + 1) % nlon] for j in range(nlon)]
    for i in range(nlat - 2):
        a, b = 1 + i * nlon, 1 + (i + 1) * nlon
        for j in range(nlon):
            j2 = (j + 1) % nlon
            f += [[a + j, b + j, b + j2], [a + j, b + j2, a + j2]]
    last, a = len(v) - 1, 1 + (nlat - 2) * nlon
    f += [[last, a + (j + 1) % nlon, a + j] for j in range(nlon)]
    return v.astype(np.float32), np.array(f, np.int64)


def csr(faces, n_verts):
    """vertex -> faces table: one entry per corner, by face and then by corner."""
    faces = np.asarray(faces, np.int64)
    flat = faces.reshape(-1)
    order = np.argsort(flat, kind='stable')
    row = np.zeros(n_verts + 1, np.int64)
    np.add.at(row, flat + 1, 1)
    return np.cumsum(row), (order // 3)


def snap(verts, trans, view, focal):
    """-> (xi, yi int64 sub-pixel, Z float32, ok bool) per vertex, fp32 arithmetic as the rules state it."""
    v = np.asarray(verts, np.float32)
    t = np.zeros(3, np.float32) if trans is None else np.asarray(trans, np.float32)
    f = np.float32(focal)
    X, Y, Z = v[:, 0] + t[0], v[:, 1] + t[1], v[:, 2] + t[2]
    with np.errstate(all='ignore'):
        x = np.float32(256) + (f * X) / Z
        y = np.float32(256) + (f * Y) / Z
        if view is not None:
            vw = np.asarray(view, np.float32)
            x = x * vw[0] + vw[2]
            y = y * vw[1] + vw[3]
        xs, ys = x * np.float32(SUB), y * np.float32(SUB)
        ok = (Z > Z_NEAR) & (np.abs(xs) <= LIMIT) & (np.abs(ys) <= LIMIT)
    xi = np.where(ok, np.rint(np.where(ok, xs, 0)), 0).astype(np.int64)
    yi = np.where(ok, np.rint(np.where(ok, ys, 0)), 0).astype(np.int64)
    return xi, yi, Z, ok


def vertex_shades(verts, faces):
    v = np.asarray(verts, np.float32).astype(np.float64)
    faces = np.asarray(faces, np.int64)
    fn = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    n = np.zeros_like(v)
    for k in range(3):
        np.add.at(n, faces[:, k], fn)
    ln = np.sqrt((n * n).sum(1))
    nz = np.where(ln > 0, np.abs(n[:, 2]) / np.where(ln > 0, ln, 1), 0.0)
    return 0.3 + 0.7 * nz


def edge(xa, ya, xb, yb, px, py):
    """Edge function of a -> b at (px, py) and the inside mask under the top-left rule."""
    A, B = ya - yb, xb - xa
    e = A * px + B * py + (xa * yb - xb * ya)
    owns = (A > 0) or (A == 0 and B > 0)
    return e, (e > 0) | ((e == 0) & owns)


def render(verts, faces, images, mesh_frame=None, trans=None, colors=None, view=None, focal=1265.0, visible_weight=0.9):
    """verts [M,V,3]; faces: one [F,3] array or a list of M of them; images uint8 [N,H,W,3].
    -> dict(out uint8 [N,H,W,3], ids int64 [N,H,W], best, second float64 [N,H,W])."""
    verts = np.asarray(verts, np.float32)
    images = np.asarray(images)
    M = verts.shape[0]
    N, H, W, _ = images.shape
    faces_l = list(faces) if isinstance(faces, (list, tuple)) else [faces] * M
    if mesh_frame is None:
        mesh_frame = np.arange(M) // (M // N)
    colors = np.asarray([0.94, 0.71, 0.53] if colors is None else colors, np.float64)
    colors = np.broadcast_to(colors, (M, 3)) if colors.ndim == 1 else colors.reshape(M, 3)
    best = np.zeros((N, H, W)); second = np.zeros((N, H, W))
    ids = -np.ones((N, H, W), np.int64)
    shade = np.zeros((N, H, W))
    ys_, xs_ = np.mgrid[0:H, 0:W]
    PX, PY = (xs_ * SUB + SUB // 2).astype(np.int64), (ys_ * SUB + SUB // 2).astype(np.int64)
    base = 0
    for m in range(M):
        f = np.asarray(faces_l[m], np.int64)
        n = int(mesh_frame[m])
        if n >= 0:
            xi, yi, Z, ok = snap(verts[m], None if trans is None else trans[m], None if view is None else view[n], focal)
            iz = 1.0 / np.where(ok, Z, 1).astype(np.float64)
            sh = vertex_shades(verts[m], f)
            for t, (a, b, c) in enumerate(f):
                if not (ok[a] and ok[b] and ok[c]):
                    continue
                x0, y0, x1, y1, x2, y2 = int(xi[a]), int(yi[a]), int(xi[b]), int(yi[b]), int(xi[c]), int(yi[c])
                area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
                if area == 0:
                    continue
                if area < 0:
                    x1, y1, x2, y2, b, c, area = x2, y2, x1, y1, c, b, -area
                lx, hx = max(0, min(x0, x1, x2) // SUB - 1), min(W - 1, max(x0, x1, x2) // SUB + 1)
                ly, hy = max(0, min(y0, y1, y2) // SUB - 1), min(H - 1, max(y0, y1, y2) // SUB + 1)
                if lx > hx or ly > hy:
                    continue
                sl = (n, slice(ly, hy + 1), slice(lx, hx + 1))
                px, py = PX[sl[1:]], PY[sl[1:]]
                w0, i0 = edge(x1, y1, x2, y2, px, py)
                w1, i1 = edge(x2, y2, x0, y0, px, py)
                w2, i2 = edge(x0, y0, x1, y1, px, py)
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


def ambiguous(ref, rel=1e-5):
    """Covered pixels whose best and second-best 1/Z differ by <= rel (relative): fp32 cannot be asked to order those."""
    return (ref['ids'] >= 0) & ((ref['best'] - ref['second']) <= rel * ref['best'])


def contains(xi, yi, tri, px, py):
    """True if the pixel centre (px, py: sub-pixel ints) is inside triangle `tri` (3 vertex ids) under the integer rule."""
    a, b, c = tri
    x0, y0, x1, y1, x2, y2 = int(xi[a]), int(yi[a]), int(xi[b]), int(yi[b]), int(xi[c]), int(yi[c])
    area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
    if area == 0:
        return False
    if area < 0:
        x1, y1, x2, y2 = x2, y2, x1, y1
    return bool(edge(x1, y1, x2, y2, px, py)[1] & edge(x2, y2, x0, y0, px, py)[1] & edge(x0, y0, x1, y1, px, py)[1])
