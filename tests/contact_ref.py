"""Numpy restatement of the contact / interpenetration measure between two meshes (the header comment
of include/acrmi.h), the yardstick of tests/test_gpu_contact.py.  Written from the rule, not from the kernel, and independent
of the library: fp32 arrays, so that every numpy operation is one rounded fp32 operation, in the order the rule states.

  position  P_m[i] = verts[m,i] + trans[m]; without trans the vertex as given
  normal    N_m[i] = sign[m] * sum over the incident faces, in the order of render_ref.csr (by face, then by corner), of
            (v1 - v0) x (v2 - v0) on verts as given; component = (a*b) - (c*d), accumulated from 0; not normalised
  nearest   d = P_a[i] - P_b[j]; d2 = (dx*dx + dy*dy) + dz*dz; nn[i] = argmin_j, lowest j on a tie; NaN and +inf never win;
            none: nn = -1, d2 = +inf, s = 0
  side      s[i] = (dx*Nx + dy*Ny) + dz*Nz with N_b[nn[i]]; contact: d2 <= r*r; inside: s < 0 and d2 <= m*m
  summary   min d2 of direction 0 with its (i, j), lowest i on a tie; contact and inside counts per direction; the largest d2
            among the inside vertices per direction, 0 when none
  skipped   a pair with an index < 0 (or >= the number of meshes): nn = -1, d2 = +inf, s = 0, zero counts, (-1, -1)
"""
import numpy as np

from render_ref import csr

F32 = np.float32
INF = F32(np.inf)


def vertex_normals(verts, faces, sign=1):
    """[V,3] fp32: the signed, un-normalised vertex normals in the table's summation order."""
    v = np.asarray(verts, F32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    V = v.shape[0]
    n = np.zeros((V, 3), F32)
    with np.errstate(all='ignore'):
        if len(faces):
            a = v[faces[:, 1]] - v[faces[:, 0]]
            b = v[faces[:, 2]] - v[faces[:, 0]]
            fn = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                           a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                           a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1).astype(F32)
            row, col = csr(faces, V)
            deg = row[1:] - row[:-1]
            for k in range(int(deg.max()) if V else 0):
                m = np.nonzero(deg > k)[0]
                n[m] = n[m] + fn[col[row[m] + k]]
        return n * F32(-1.0 if sign < 0 else 1.0)


def direction(Pa, Pb, Nb):
    """The vertices of a against mesh b -> (nn int32, d2 fp32, s fp32)."""
    with np.errstate(all='ignore'):
        dx = Pa[:, None, 0] - Pb[None, :, 0]
        dy = Pa[:, None, 1] - Pb[None, :, 1]
        dz = Pa[:, None, 2] - Pb[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        ok = d2 < INF                                   # false for NaN and for +inf
        masked = np.where(ok, d2, INF)
        nn = np.argmin(masked, 1)                       # the first (lowest j) of equal minima
        has = ok.any(1)
        i = np.arange(Pa.shape[0])
        best = np.where(has, masked[i, nn], INF).astype(F32)
        ex, ey, ez = dx[i, nn], dy[i, nn], dz[i, nn]
        s = (ex * Nb[nn, 0] + ey * Nb[nn, 1]) + ez * Nb[nn, 2]
        s = np.where(has, s, F32(0)).astype(F32)
    return np.where(has, nn, -1).astype(np.int32), best, s


def summary(nn, d2, s, contact_dist, max_depth):
    """nn, d2, s [2,V] of one pair -> (sum_f [4] fp32, sum_i [6] int32)."""
    with np.errstate(all='ignore'):
        r2 = F32(contact_dist) * F32(contact_dist)
        m2 = F32(max_depth) * F32(max_depth)
    has = nn >= 0
    contact = has & (d2 <= r2)
    inside = has & (s < 0) & (d2 <= m2)
    sf = np.zeros(4, F32)
    si = np.zeros(6, np.int32)
    if has[0].any():
        i = int(np.argmin(np.where(has[0], d2[0], INF)))      # lowest i on a tie
        sf[0], si[0], si[1] = d2[0, i], i, nn[0, i]
    else:
        sf[0], si[0], si[1] = INF, -1, -1
    for k in (0, 1):
        si[2 + k] = contact[k].sum()
        si[4 + k] = inside[k].sum()
        sf[1 + k] = d2[k][inside[k]].max() if inside[k].any() else 0
    return sf, si


def mesh_contact(verts, faces, pairs, trans=None, topo_index=None, sign=None, contact_dist=0.005, max_depth=0.02):
    """verts [M,V,3]; faces [F,3] or a pair of them chosen per mesh by topo_index [M]; pairs [n,2] -> the dict of
    ops.mesh_contact as numpy arrays: nn, d2, side [n,2,V]; min_d2 [n]; closest [n,2]; n_contact, n_inside [n,2]; depth2
    [n,2]."""
    verts = np.asarray(verts, F32)
    M, V, _ = verts.shape
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    two = isinstance(faces, (tuple, list)) and len(faces) == 2 and np.ndim(faces[0]) == 2
    topos = list(faces) if two else [faces]
    ti = np.zeros(M, np.int64) if topo_index is None else np.asarray(topo_index, np.int64)
    sg = np.ones(M, np.int64) if sign is None else np.asarray(sign, np.int64)
    P, N = {}, {}

    def prep(m):
        if m not in P:
            with np.errstate(all='ignore'):
                P[m] = verts[m] if trans is None else verts[m] + np.asarray(trans, F32)[m][None, :]
            N[m] = vertex_normals(verts[m], topos[1 if (two and ti[m] == 1) else 0], sg[m])
        return P[m], N[m]

    n = len(pairs)
    out = {'nn': np.full((n, 2, V), -1, np.int32), 'd2': np.full((n, 2, V), INF, F32), 'side': np.zeros((n, 2, V), F32),
           'min_d2': np.full(n, INF, F32), 'closest': np.full((n, 2), -1, np.int32), 'n_contact': np.zeros((n, 2), np.int32),
           'n_inside': np.zeros((n, 2), np.int32), 'depth2': np.zeros((n, 2), F32)}
    for p, (a, b) in enumerate(pairs):
        if a < 0 or b < 0 or a >= M or b >= M:
            continue
        (Pa, Na), (Pb, Nb) = prep(int(a)), prep(int(b))
        out['nn'][p, 0], out['d2'][p, 0], out['side'][p, 0] = direction(Pa, Pb, Nb)
        out['nn'][p, 1], out['d2'][p, 1], out['side'][p, 1] = direction(Pb, Pa, Na)
        sf, si = summary(out['nn'][p], out['d2'][p], out['side'][p], contact_dist, max_depth)
        out['min_d2'][p], out['depth2'][p] = sf[0], sf[1:3]
        out['closest'][p], out['n_contact'][p], out['n_inside'][p] = si[0:2], si[2:4], si[4:6]
    return out


def frame_pairs(flags, K):
    """flags [B,K,2] (or [B,2] with K = 1) of the slots -> pairs [B*K*K,2]: (left rank i, right rank j) of row b at index
    (b*K + i)*K + j, mesh (b*K + k)*2 + h; (-1, -1) where either flag is not > 0.5."""
    flags = np.asarray(flags, F32).reshape(-1, K, 2)
    B = flags.shape[0]
    pairs = np.full((B * K * K, 2), -1, np.int32)
    for b in range(B):
        for i in range(K):
            for j in range(K):
                if flags[b, i, 0] > 0.5 and flags[b, j, 1] > 0.5:
                    pairs[(b * K + i) * K + j] = ((b * K + i) * 2, (b * K + j) * 2 + 1)
    return pairs


def same_bits(a, b):
    """fp32 arrays equal bit for bit, except that any NaN equals any NaN (the payload of a NaN is not part of the rule)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(np.uint32)[~na] == b.view(np.uint32)[~nb]).all())
