"""Numpy restatement of the surface contact measure between two meshes (the header comment of
include/acrmi.h; csrc/surface_contact_plan.h), the yardstick of tests/test_gpu_surface_contact.py.  Written from the rule, not
from the kernel, and independent of the library: fp32 arrays, so that every numpy operation is one rounded fp32 operation, in
the order the rule states.  No cull: every vertex meets every face.

  dot(a,b) = (ax*bx + ay*by) + az*bz; a cross component is (a*b) - (c*d); P_m[i] = verts[m,i] + trans[m]
  For the ordered pair (a, b), vertex p = P_a[i] and face f of b with corners A, B, C = P_b[f0], P_b[f1], P_b[f2]:
  closest   (Ericson, Real-Time Collision Detection 5.1.5; every comparison is false on NaN, the first true branch wins)
            ab = B-A, ac = C-A, ap = p-A, d1 = dot(ab,ap), d2 = dot(ac,ap); bp = p-B, d3 = dot(ab,bp), d4 = dot(ac,bp);
            cp = p-C, d5 = dot(ab,cp), d6 = dot(ac,cp); vc = d1*d4 - d3*d2, vb = d5*d2 - d1*d6, va = d3*d6 - d5*d4;
            e43 = d4-d3, e56 = d5-d6
            1. d1<=0 && d2<=0: q = A              2. d3>=0 && d4<=d3: q = B
            3. vc<=0 && d1>=0 && d3<=0: q = A + (d1/(d1-d3))*ab
            4. d6>=0 && d5<=d6: q = C             5. vb<=0 && d2>=0 && d6<=0: q = A + (d2/(d2-d6))*ac
            6. va<=0 && e43>=0 && e56>=0: q = B + (e43/(e43+e56))*(C-B)
            7. otherwise: den = 1/((va+vb)+vc), q = (A + ab*(vb*den)) + ac*(vc*den)
            e = p-q, D2(i,f) = dot(e,e); face[i] = the f with the smallest D2 below +inf, the lowest f on a tie; NaN and +inf
            never win; d2[i] that value, point[i] that face's q; none: face = -1, d2 = +inf, point = 0
  crossings of the ray from p towards +Z: for each face edge u -> v (f0->f1, f1->f2, f2->f0), lo, hi = the positions of
            min(u,v), max(u,v); E = (hi.x-lo.x)*(p.y-lo.y) - (hi.y-lo.y)*(p.x-lo.x); sc = +1 if E >= 0 else -1; the edge's sign
            is sc when u < v, -sc when u > v, 0 when u == v.  The face covers p when its three signs are equal and not zero;
            the ray meets its plane in front of p when o = dot(ap, n), n = ab x ac, and n.z have strictly opposite signs.
            cross[i] = the number of faces that do both; inside: cross[i] odd
  flags     per direction: in contact: face >= 0 and d2 <= r*r; inside: face >= 0, cross odd and d2 <= m*m
  summary   per direction: min d2 with closest = (i, face), the lowest i on a tie, (-1, -1) without one; contact and inside
            counts; depth2 = the largest d2 among the inside vertices, 0 without one
  skipped   a pair with an index < 0 (or >= the number of meshes): face = -1, d2 = +inf, point = 0, cross = 0, zero counts
"""
import numpy as np

F32 = np.float32
INF = F32(np.inf)


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def closest(p, A, B, C):
    """p, A, B, C: lists of three fp32 arrays that broadcast against each other -> (branch 1..7, q as three arrays, D2)."""
    with np.errstate(all='ignore'):
        ab, ac, ap = sub(B, A), sub(C, A), sub(p, A)
        d1, d2 = dot(ab, ap), dot(ac, ap)
        bp = sub(p, B)
        d3, d4 = dot(ab, bp), dot(ac, bp)
        cp = sub(p, C)
        d5, d6 = dot(ab, cp), dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e43 >= 0) & (e56 >= 0)]
        t3, t5, t6 = d1 / (d1 - d3), d2 / (d2 - d6), e43 / (e43 + e56)
        den = F32(1) / ((va + vb) + vc)
        cb = sub(C, B)
        qs = [A, B, [A[k] + t3 * ab[k] for k in range(3)], C, [A[k] + t5 * ac[k] for k in range(3)],
              [B[k] + t6 * cb[k] for k in range(3)], [(A[k] + ab[k] * (vb * den)) + ac[k] * (vc * den) for k in range(3)]]
        shape = np.broadcast(d1, d2).shape
        br = np.full(shape, 7, np.int32)
        for n in range(5, -1, -1):                      # the first true branch wins: assigned last
            br = np.where(conds[n], np.int32(n + 1), br)
        q = [np.select([br == n + 1 for n in range(7)], [np.broadcast_to(qs[n][k], shape) for n in range(7)]).astype(F32)
             for k in range(3)]
        e = sub(p, q)
        return br, q, dot(e, e).astype(F32)


def crossings(P, Pb, faces):
    """P [V,3]: the vertices; Pb, faces: the other mesh -> [V,F] bool: the +Z ray from the vertex crosses the face."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    px, py = P[:, None, 0], P[:, None, 1]
    with np.errstate(all='ignore'):
        signs = []
        for k in range(3):
            u, v = faces[:, k], faces[:, (k + 1) % 3]
            lo, hi = Pb[np.minimum(u, v)][None], Pb[np.maximum(u, v)][None]
            E = (hi[..., 0] - lo[..., 0]) * (py - lo[..., 1]) - (hi[..., 1] - lo[..., 1]) * (px - lo[..., 0])
            sc = np.where(E >= 0, 1, -1)
            signs.append(sc * np.sign(v - u)[None])
        covers = (signs[0] == signs[1]) & (signs[1] == signs[2]) & (signs[0] != 0)
        A, B, C = ([Pb[faces[:, c], k][None] for k in range(3)] for c in range(3))
        ab, ac = sub(B, A), sub(C, A)
        ap = sub([P[:, None, k] for k in range(3)], A)
        n = [ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]]
        o = dot(ap, n)
        front = ((o > 0) & (n[2] < 0)) | ((o < 0) & (n[2] > 0))
    return covers & front


def direction(Pa, Pb, faces):
    """The vertices of a against the faces of mesh b -> (face int32 [V], d2 fp32 [V], point fp32 [V,3], cross int32 [V])."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    V = Pa.shape[0]
    p = [Pa[:, None, k] for k in range(3)]
    A, B, C = ([Pb[faces[:, c], k][None] for k in range(3)] for c in range(3))
    _, q, D2 = closest(p, A, B, C)
    ok = D2 < INF                                       # false for NaN and for +inf
    masked = np.where(ok, D2, INF)
    f = np.argmin(masked, 1)                            # the first (lowest f) of equal minima
    has = ok.any(1)
    i = np.arange(V)
    best = np.where(has, masked[i, f], INF).astype(F32)
    point = np.stack([np.where(has, q[k][i, f], F32(0)) for k in range(3)], 1).astype(F32)
    cross = crossings(Pa, Pb, faces).sum(1).astype(np.int32)
    return np.where(has, f, -1).astype(np.int32), best, point, cross


def summary(face, d2, cross, contact_dist, max_depth):
    """face, d2, cross [2,V] of one pair -> (min_d2 [2], closest [2,2], n_contact [2], n_inside [2], depth2 [2])."""
    with np.errstate(all='ignore'):
        r2 = F32(contact_dist) * F32(contact_dist)
        m2 = F32(max_depth) * F32(max_depth)
    has = face >= 0
    contact = has & (d2 <= r2)
    inside = has & (cross % 2 == 1) & (d2 <= m2)
    min_d2, closest_, depth2 = np.full(2, INF, F32), np.full((2, 2), -1, np.int32), np.zeros(2, F32)
    for k in (0, 1):
        if has[k].any():
            i = int(np.argmin(np.where(has[k], d2[k], INF)))      # lowest i on a tie
            min_d2[k], closest_[k] = d2[k, i], (i, face[k, i])
        if inside[k].any():
            depth2[k] = d2[k][inside[k]].max()
    return min_d2, closest_, contact.sum(1).astype(np.int32), inside.sum(1).astype(np.int32), depth2


def with_params(out, contact_dist, max_depth):
    """The result `out` of mesh_surface_contact at other parameters: the per-vertex outputs do not depend on them."""
    new = {k: v.copy() for k, v in out.items()}
    for p in range(len(out['face'])):
        if (out['face'][p] >= 0).any():
            (new['min_d2'][p], new['closest'][p], new['n_contact'][p], new['n_inside'][p],
             new['depth2'][p]) = summary(out['face'][p], out['d2'][p], out['cross'][p], contact_dist, max_depth)
    return new


def mesh_surface_contact(verts, faces, pairs, trans=None, topo_index=None, contact_dist=0.005, max_depth=0.02):
    """verts [M,V,3]; faces [F,3] or a pair of them chosen per mesh by topo_index [M]; pairs [n,2] -> the dict of
    ops.mesh_surface_contact as numpy arrays: face, d2, cross [n,2,V]; point [n,2,V,3]; min_d2 [n,2]; closest [n,2,2];
    n_contact, n_inside, depth2 [n,2]."""
    verts = np.asarray(verts, F32)
    M, V, _ = verts.shape
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    two = isinstance(faces, (tuple, list)) and len(faces) == 2 and np.ndim(faces[0]) == 2
    topos = list(faces) if two else [faces]
    ti = np.zeros(M, np.int64) if topo_index is None else np.asarray(topo_index, np.int64)
    P = {}

    def prep(m):
        if m not in P:
            with np.errstate(all='ignore'):
                P[m] = verts[m] if trans is None else verts[m] + np.asarray(trans, F32)[m][None, :]
        return P[m], topos[1 if (two and ti[m] == 1) else 0]

    n = len(pairs)
    out = {'face': np.full((n, 2, V), -1, np.int32), 'd2': np.full((n, 2, V), INF, F32), 'point': np.zeros((n, 2, V, 3), F32),
           'cross': np.zeros((n, 2, V), np.int32), 'min_d2': np.full((n, 2), INF, F32), 'closest': np.full((n, 2, 2), -1, np.int32),
           'n_contact': np.zeros((n, 2), np.int32), 'n_inside': np.zeros((n, 2), np.int32), 'depth2': np.zeros((n, 2), F32)}
    for p, (a, b) in enumerate(pairs):
        if a < 0 or b < 0 or a >= M or b >= M:
            continue
        (Pa, fa), (Pb, fb) = prep(int(a)), prep(int(b))
        for k, (X, Y, fy) in enumerate(((Pa, Pb, fb), (Pb, Pa, fa))):
            out['face'][p, k], out['d2'][p, k], out['point'][p, k], out['cross'][p, k] = direction(X, Y, fy)
        (out['min_d2'][p], out['closest'][p], out['n_contact'][p], out['n_inside'][p],
         out['depth2'][p]) = summary(out['face'][p], out['d2'][p], out['cross'][p], contact_dist, max_depth)
    return out
