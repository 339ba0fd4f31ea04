"""The top-K decode rule restated in numpy, and the seeded maps its tests share.

Test infrastructure, not product: per frame and side the K best candidates of the NMS'd centre map, a flag per rank, the
partner of every flagged hand and the sampled parameters.  Everything is float32 arithmetic that has one answer (a
comparison, one add), so the device result is compared bit for bit.  NaN maps are outside the rule (an order of NaNs is not
defined); the kernel only has to stay inside the maps for them.
"""
import numpy as np

MAP = 64
CONF_THRESH = 0.35
MAX_HAND = 8


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def nms_det(c):
    """c [64,64] float32 -> c * (maxpool5x5(c) == c), the window clipped at the border; the losers are c * 0 (sign kept)."""
    c = np.asarray(c, np.float32)
    pad = np.full((MAP + 4, MAP + 4), -np.inf, np.float32)
    pad[2:-2, 2:-2] = c
    m = c.copy()
    for dy in range(5):
        for dx in range(5):
            m = np.fmax(m, pad[dy:dy + MAP, dx:dx + MAP])
    with np.errstate(invalid='ignore'):
        return np.where(m == c, c, c * np.float32(0.0)).astype(np.float32)


def topk(c, K, thresh=CONF_THRESH):
    """One map -> (flag [K] bool, flat [K] int64, score [K] float32): the first K pixels by det descending, lower flat index
    first on an exact tie (+0 == -0 is a tie); flag = score > thresh (strict); an unflagged rank points at pixel 0."""
    det = nms_det(c).reshape(-1)
    order = np.argsort(-det, kind='stable')[:K]
    score = det[order]
    flag = score > np.float32(thresh)
    return flag, np.where(flag, order, 0).astype(np.int64), score


def partners(flag, flat):
    """flag, flat [K,2] of one frame -> partner [K,2] int64: the flat index of the nearest flagged centre of the OTHER side
    (sqrt(dy^2 + dx^2) in float32 on the integer coordinates, lower rank on a tie), -1 for an unflagged hand, for a hand
    without one and when that distance is > 32."""
    K = flag.shape[0]
    out = np.full((K, 2), -1, np.int64)
    for h in (0, 1):
        for k in range(K):
            if not flag[k, h]:
                continue
            best, bd = -1, np.float32(np.inf)
            for j in range(K):
                if not flag[j, 1 - h]:
                    continue
                dy = np.float32(flat[k, h] // MAP) - np.float32(flat[j, 1 - h] // MAP)
                dx = np.float32(flat[k, h] % MAP) - np.float32(flat[j, 1 - h] % MAP)
                d = np.sqrt(np.float32(dy * dy + dx * dx), dtype=np.float32)
                if best < 0 or d < bd:
                    best, bd = int(flat[j, 1 - h]), d
            if best >= 0 and not bd > np.float32(32.0):
                out[k, h] = best
    return out


def decode_multi(maps, K, thresh=CONF_THRESH):
    """maps: the head dict (NCHW float32 numpy: l/r_center_map [B,1,64,64], l/r_params_maps [B,109,64,64], l/r_prior_maps
    [B,106,64,64]) -> dict of flag [B,K,2] bool, flat_ind [B,K,2] int64, score [B,K,2], partner [B,K,2] int64, params_pred
    [B,K,2,109]: the slot layout, pair k = (left rank k, right rank k)."""
    B = maps['l_center_map'].shape[0]
    flag = np.zeros((B, K, 2), bool)
    flat = np.zeros((B, K, 2), np.int64)
    score = np.zeros((B, K, 2), np.float32)
    partner = np.zeros((B, K, 2), np.int64)
    pred = np.zeros((B, K, 2, 109), np.float32)
    for b in range(B):
        for h, s in enumerate('lr'):
            flag[b, :, h], flat[b, :, h], score[b, :, h] = topk(maps[s + '_center_map'][b, 0], K, thresh)
        partner[b] = partners(flag[b], flat[b])
        for h, s in enumerate('lr'):
            par = np.asarray(maps[s + '_params_maps'][b], np.float32).reshape(109, -1)
            pri = np.asarray(maps[s + '_prior_maps'][b], np.float32).reshape(106, -1)
            for k in range(K):
                v = par[:, flat[b, k, h]].copy()
                if partner[b, k, h] >= 0:
                    v[3:] = v[3:] + pri[:, partner[b, k, h]]      # one float32 add
                pred[b, k, h] = v
    return {'flag': flag, 'flat_ind': flat, 'score': score, 'partner': partner, 'params_pred': pred}


# ---- the seeded centre maps of tests/golden/decode_topk.npz (make_golden_topk.py runs the reference on them) ------------------
# name -> ('uniform', seed, frames) | ('planted', seed, peaks per frame)
TOPK_CASES = {
    'uniform_a': ('uniform', 11, 3),
    'uniform_b': ('uniform', 12, 2),
    'planted_a': ('planted', 21, (0, 1, 3)),
    'planted_b': ('planted', 22, (2, 4, 6)),
    'planted_c': ('planted', 23, (8, 9, 5)),
}
TOPK_KS = (1, 2, 4, 8)


def planted_map(g, n):
    """A zero map with n Gaussian bumps (sigma 1) of distinct heights in (0.45, 0.95), at least 7 pixels apart, border
    positions included -> (map [64,64] float32, [(y, x, height)])."""
    c = np.zeros((MAP, MAP), np.float32)
    peaks = []
    heights = (0.45 + 0.5 * (g.permutation(16)[:n] + g.uniform(0.1, 0.9, n)) / 16).astype(np.float32)
    yy, xx = np.mgrid[0:MAP, 0:MAP]
    while len(peaks) < n:
        y, x = int(g.integers(0, MAP)), int(g.integers(0, MAP))
        if any(max(abs(y - p[0]), abs(x - p[1])) < 7 for p in peaks):
            continue
        a = heights[len(peaks)]
        c = np.maximum(c, (a * np.exp(-((yy - y) ** 2 + (xx - x) ** 2) / 2.0)).astype(np.float32))
        peaks.append((y, x, float(a)))
    return c, peaks


def topk_case_maps(name):
    """-> (centre maps [B,1,64,64] float32, the number of detections above the threshold in each frame)."""
    kind, seed, spec = TOPK_CASES[name]
    g = rng(seed)
    if kind == 'uniform':
        c = g.uniform(0.0, 1.0, (spec, 1, MAP, MAP)).astype(np.float32)
    else:
        c = np.stack([planted_map(g, n)[0] for n in spec])[:, None]
    counts = [int((nms_det(m[0]) > np.float32(CONF_THRESH)).sum()) for m in c]
    return c, counts


def head_maps(center_l, center_r, seed):
    """Centre maps [B,1,64,64] -> the head dict with seeded params / prior maps (NCHW float32)."""
    g = rng(seed)
    B = center_l.shape[0]
    m = {'l_center_map': np.ascontiguousarray(center_l, np.float32), 'r_center_map': np.ascontiguousarray(center_r, np.float32)}
    for s in 'lr':
        m[s + '_params_maps'] = g.normal(0, 0.6, (B, 109, MAP, MAP)).astype(np.float32)
        m[s + '_prior_maps'] = g.normal(0, 0.3, (B, 106, MAP, MAP)).astype(np.float32)
    return m
