"""The scoring rule of csrc/score_plan.h in numpy float64, operation for operation and in the same
order: counted points, origins, the lane-strided sums with their fixed tree, Horn's matrix, six cyclic Jacobi sweeps, the
errors, the row outputs, the pair terms and the board.  numpy rounds every float64 operation on its own, as the kernel does."""
import math

import numpy as np

SWEEPS = 6
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
F32_MAX = np.float32(3.4028234e38)


def threads(n):
    return 64 if n <= 64 else 256


def tree_sum(vals, T):
    """vals float64 [n, ...] (zero where a point does not count) -> the plan's sum: thread t adds its points t, t + T, ... in
    ascending order, then v[t] = v[t] + v[t + s] for t < s, s = T/2 .. 1."""
    part = np.zeros((T,) + vals.shape[1:], np.float64)
    for k in range(0, vals.shape[0], T):
        chunk = vals[k:k + T]
        part[:chunk.shape[0]] = part[:chunk.shape[0]] + chunk
    s = T // 2
    while s >= 1:
        part[:s] = part[:s] + part[s:2 * s]
        s //= 2
    return part[0]


def norm3(d):
    """sqrt((dx*dx + dy*dy) + dz*dz) over the last axis."""
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def horn_matrix(S):
    xx, xy, xz, yx, yy, yz, zx, zy, zz = [float(v) for v in np.asarray(S, np.float64).reshape(9)]
    a = [[0.0] * 4 for _ in range(4)]
    a[0][0] = (xx + yy) + zz
    a[1][1] = (xx - yy) - zz
    a[2][2] = (yy - xx) - zz
    a[3][3] = (zz - xx) - yy
    a[0][1] = a[1][0] = yz - zy
    a[0][2] = a[2][0] = zx - xz
    a[0][3] = a[3][0] = xy - yx
    a[1][2] = a[2][1] = xy + yx
    a[1][3] = a[3][1] = zx + xz
    a[2][3] = a[3][2] = yz + zy
    return a


def horn(S, sweeps=SWEEPS):
    """S [3,3] float64 -> (quaternion (w, x, y, z), its eigenvalue).  Python floats are IEEE doubles."""
    a = horn_matrix(S)
    v = [[1.0 if r == k else 0.0 for k in range(4)] for r in range(4)]
    for _ in range(sweeps):
        for p, q in PAIRS:
            apq = a[p][q]
            if apq == 0.0:
                continue
            theta = (a[q][q] - a[p][p]) / (2.0 * apq)
            t = (-1.0 if theta < 0.0 else 1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            a[p][p] = a[p][p] - t * apq
            a[q][q] = a[q][q] + t * apq
            a[p][q] = a[q][p] = 0.0
            for r in range(4):
                if r != p and r != q:
                    arp, arq = a[r][p], a[r][q]
                    a[r][p] = a[p][r] = c * arp - s * arq
                    a[r][q] = a[q][r] = s * arp + c * arq
                vrp, vrq = v[r][p], v[r][q]
                v[r][p] = c * vrp - s * vrq
                v[r][q] = s * vrp + c * vrq
    best = 0
    for k in range(1, 4):
        if a[k][k] > a[best][best]:
            best = k
    return [v[r][best] for r in range(4)], a[best][best]


def quat_matrix(q):
    w, x, y, z = q
    ww, xx, yy, zz = w * w, x * x, y * y, z * z
    xy, xz, yz, wx, wy, wz = x * y, x * z, y * z, w * x, w * y, w * z
    return np.array([[((ww + xx) - yy) - zz, 2.0 * (xy - wz), 2.0 * (xz + wy)],
                     [2.0 * (xy + wz), ((ww - xx) + yy) - zz, 2.0 * (yz - wx)],
                     [2.0 * (xz - wy), 2.0 * (yz + wx), ((ww - xx) - yy) + zz]], np.float64)


def rot(R, pc):
    """(R[a][0]*x + R[a][1]*y) + R[a][2]*z for every row of pc [m,3] -> [m,3]."""
    return np.stack([(R[a, 0] * pc[..., 0] + R[a, 1] * pc[..., 1]) + R[a, 2] * pc[..., 2] for a in range(3)], -1)


def finite32(x):
    with np.errstate(invalid='ignore'):
        return np.abs(x) <= F32_MAX


def row_state(group, n_groups, flag):
    """0: not looked at; 1: a miss; 2: scored.  flag None = flagged."""
    if group < 0 or group >= n_groups:
        return 0
    with np.errstate(invalid='ignore'):
        return 2 if flag is None or bool(np.float32(flag) > np.float32(0.5)) else 1


def origins_of(P, G, valid, root, oP, oG):
    """-> (good, oP float64 [3], oG float64 [3]) of one row."""
    if root >= 0:
        if valid is not None and valid[root] == 0:
            return False, None, None
        oP, oG = P[root], G[root]
    elif oP is None:
        return True, np.zeros(3), np.zeros(3)
    good = bool(finite32(oP).all() and finite32(oG).all())
    return good, oP.astype(np.float64), oG.astype(np.float64)


def placed(oP, trans):
    """oP + trans, and whether trans is finite."""
    if trans is None:
        return False, None
    return bool(finite32(trans).all()), oP + trans.astype(np.float64)


def row_errors(P, G, valid=None, root=-1, oP=None, oG=None, trans=None):
    """One scored row: P, G float32 [n,3] -> {'e_ra', 'e_pa' float32 [n], 'row_f' float32 [4], 'row_i' int32 [2], 'xform' float32
    [8]}."""
    n = P.shape[0]
    T = threads(n)
    with np.errstate(all='ignore'):
        on = finite32(P).all(1) & finite32(G).all(1)
        if valid is not None:
            on &= np.asarray(valid) != 0
        Pd = np.where(on[:, None], P, 0).astype(np.float64)
        Gd = np.where(on[:, None], G, 0).astype(np.float64)
        good, o_p, o_g = origins_of(P, G, valid, root, oP, oG)
        m = tree_sum(np.concatenate([Pd, Gd, on[:, None].astype(np.float64)], 1), T)
        c = int(m[6])
        muP, muG = (m[0:3] / float(c), m[3:6] / float(c)) if c > 0 else (np.zeros(3), np.zeros(3))
        pc, gc = Pd - muP, Gd - muG
        prod = np.stack([pc[:, a] * gc[:, b] for a in range(3) for b in range(3)] +
                        [(pc[:, 0] * pc[:, 0] + pc[:, 1] * pc[:, 1]) + pc[:, 2] * pc[:, 2]], 1)
        if good:
            era = norm3((Pd - o_p) - (Gd - o_g))
        else:
            era = np.zeros(n)
        r = tree_sum(np.where(on[:, None], np.concatenate([prod, era[:, None]], 1), 0.0), T)
        vP = r[9]
        pa = c >= 3 and vP > 0.0
        e_ra = np.where(on & good, era, -1.0).astype(np.float32)
        q, scale, R = [0.0] * 4, -1.0, None
        if pa:
            q, lam = horn(r[:9].reshape(3, 3))
            R = quat_matrix(q)
            scale = lam / vP
            epa = norm3((scale * rot(R, pc) + muG) - Gd)
            w = tree_sum(np.where(on, epa, 0.0), T)
            e_pa = np.where(on, epa, -1.0).astype(np.float32)
        else:
            w = 0.0
            e_pa = np.full(n, -1.0, np.float32)
        c_ra, c_pa = (c if good else 0), (c if pa else 0)
        row_f = np.full(4, -1.0, np.float32)
        if c_ra > 0:
            row_f[0] = np.float32(r[10] / float(c_ra))
        if c_pa > 0:
            row_f[1] = np.float32(w / float(c_pa))
        row_f[2] = np.float32(scale)
        if good:
            ok, pl = placed(o_p, trans)
            if ok:
                row_f[3] = np.float32(norm3(pl - o_g))
        xform = np.zeros(8, np.float32)
        xform[0:4] = np.array(q, np.float64).astype(np.float32)
        xform[4] = np.float32(scale)
        if pa:
            xform[5:8] = (muG - scale * rot(R, muP[None])[0]).astype(np.float32)
    return {'e_ra': e_ra, 'e_pa': e_pa, 'row_f': row_f, 'row_i': np.array([c_ra, c_pa], np.int32), 'xform': xform}


def pose_errors(pred, gt, valid=None, root=-1, origin=None, group=None, flags=None, trans=None, n_groups=1):
    """The operator over N rows: float32 [N,n,3] -> {'e_ra', 'e_pa' [N,n], 'row_f' [N,4], 'row_i' [N,2], 'xform' [N,8], 'pair_err'
    [N // 2]} as acrmi_pose_errors writes them."""
    pred, gt = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    N, n, _ = pred.shape
    out = {'e_ra': np.full((N, n), -1, np.float32), 'e_pa': np.full((N, n), -1, np.float32), 'row_f': np.full((N, 4), -1, np.float32),
           'row_i': np.zeros((N, 2), np.int32), 'xform': np.zeros((N, 8), np.float32), 'pair_err': np.full(N // 2, -1, np.float32)}
    out['xform'][:, 4] = -1
    state = [row_state(0 if group is None else int(group[r]), n_groups, None if flags is None else flags[r]) for r in range(N)]
    side = lambda r: dict(valid=None if valid is None else valid[r], root=root, oP=None if origin is None else origin[0][r],
                          oG=None if origin is None else origin[1][r])
    for r in range(N):
        if state[r] != 2:
            continue
        res = row_errors(pred[r], gt[r], trans=None if trans is None else trans[r], **side(r))
        for k, v in res.items():
            out[k][r] = v
    with np.errstate(all='ignore'):
        for p in range(N // 2):
            l, r = 2 * p, 2 * p + 1
            if state[l] != 2 or state[r] != 2 or trans is None:
                continue
            gl, lP, lG = origins_of(pred[l], gt[l], **side(l))
            gr_, rP, rG = origins_of(pred[r], gt[r], **side(r))
            if not (gl and gr_):
                continue
            okl, pl = placed(lP, trans[l])
            okr, pr = placed(rP, trans[r])
            if okl and okr:
                out['pair_err'][p] = np.float32(norm3((pr - pl) - (rG - lG)))
    return out


def bin_of(e, bin_width, n_bins):
    q = np.float64(e) / np.float64(bin_width)
    return n_bins if q >= float(n_bins) else int(q)


def new_board(n, n_groups, n_bins):
    G = n_groups
    return {'sum_ra': np.zeros((G, n)), 'sum_pa': np.zeros((G, n)), 'cnt_ra': np.zeros((G, n), np.int64),
            'cnt_pa': np.zeros((G, n), np.int64), 'hist': np.zeros((G, n_bins + 1), np.int64), 'scored': np.zeros(G, np.int64),
            'missed': np.zeros(G, np.int64), 'pair_sum': np.zeros((G, G)), 'pair_cnt': np.zeros((G, G), np.int64)}


def board_add(board, e_ra, e_pa, pair_err, group, flags, n_groups, n_bins, bin_width):
    """Adds the float32 outputs of one call to the board: every element continues from its value and adds the outputs >= 0,
    converted to double, in ascending row order."""
    N = e_ra.shape[0]
    grp = [0 if group is None else int(group[r]) for r in range(N)]
    with np.errstate(all='ignore'):
        for r in range(N):
            g = grp[r]
            state = row_state(g, n_groups, None if flags is None else flags[r])
            if state == 0:
                continue
            board['scored' if state == 2 else 'missed'][g] += 1
            for e, s, c in ((e_ra[r], 'sum_ra', 'cnt_ra'), (e_pa[r], 'sum_pa', 'cnt_pa')):
                on = e >= 0
                board[s][g] = np.where(on, board[s][g] + np.where(on, e, 0).astype(np.float64), board[s][g])
                board[c][g] += on
            for e in e_ra[r][e_ra[r] >= 0]:
                board['hist'][g, bin_of(e, bin_width, n_bins)] += 1
        if pair_err is not None:
            for p in range(N // 2):
                gl, gr = grp[2 * p], grp[2 * p + 1]
                if 0 <= gl < n_groups and 0 <= gr < n_groups and pair_err[p] >= 0:
                    board['pair_sum'][gl, gr] = board['pair_sum'][gl, gr] + np.float64(pair_err[p])
                    board['pair_cnt'][gl, gr] += 1
    return board
