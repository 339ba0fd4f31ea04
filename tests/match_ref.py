"""The rule of matching decoded hands to ground truth (csrc/match_plan.h) restated in numpy float64, every
operation rounded on its own: the pair costs, the allowed pairs, the subset recurrence with its tie order, the outputs, the
gather and the board.  The GPU tests compare the kernels with this FOR EQUALITY."""
import itertools

import numpy as np

FLT_MAX = np.float32(3.4028234e38)


def finite(a):
    with np.errstate(invalid='ignore'):
        return np.abs(a) <= FLT_MAX      # (NaN: False)


def pair_costs(pred, truth, valid=None, trans=None):
    """pred [B,K,2,n,D], truth [B,G,2,n,D] float32 -> (cost float64 [B,K,G,2], count [B,K,G,2]); the cost of a pair without a
    counted point is 0 (it is never allowed)."""
    pred, truth = np.asarray(pred, np.float32), np.asarray(truth, np.float32)
    n, D = pred.shape[-2:]
    on = finite(pred).all(-1)[:, :, None] & finite(truth).all(-1)[:, None]      # [B,K,G,2,n]
    if valid is not None:
        on = on & (np.asarray(valid) != 0)[:, None]
    P = pred.astype(np.float64)
    with np.errstate(all='ignore'):
        if trans is not None:
            P = P + np.asarray(trans, np.float32).astype(np.float64)[:, :, :, None, :]
        d = P[:, :, None] - truth.astype(np.float64)[:, None]                   # [B,K,G,2,n,D]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
        if D == 3:
            d2 = d2 + d[..., 2] * d[..., 2]
        dist = np.sqrt(d2)
        total = np.zeros(on.shape[:-1], np.float64)
        for j in range(n):      # ascending j; a point that does not count adds +0
            total = total + np.where(on[..., j], dist[..., j], 0.0)
        count = on.sum(-1)
        cost = np.where(count >= 1, total / np.maximum(count, 1).astype(np.float64), 0.0)
    return cost, count


def allowed_pairs(cost, count, flags=None, truth_valid=None, gate=np.inf, min_points=1):
    """cost, count [B,K,G,2]; flags float32 [B,K,2] or None; truth_valid [B,G,2] or None -> bool [B,K,G,2]."""
    with np.errstate(invalid='ignore'):
        ok = (count >= 1) & (count >= min_points) & np.isfinite(cost) & (cost <= np.float64(np.float32(gate)))
        if flags is not None:
            ok = ok & (np.asarray(flags, np.float32) > np.float32(0.5))[:, :, None]
    if truth_valid is not None:
        ok = ok & (np.asarray(truth_valid) != 0)[:, None]
    return ok


def solve(cost, allow):
    """The recurrence over P problems at once: cost float64 [P,K,G], allow bool [P,K,G] -> (match int32 [P,K], pairs [P], the
    cost sum of the final state [P])."""
    cost, allow = np.asarray(cost, np.float64), np.asarray(allow, bool)
    P, K, G = cost.shape
    S = 1 << G
    ms = np.arange(S)
    cnt = np.full((P, S), -1, np.int64)
    cnt[:, 0] = 0
    total = np.zeros((P, S), np.float64)
    choice = np.full((P, K, S), -1, np.int64)
    with np.errstate(all='ignore'):
        for i in range(K):
            bc, bs, ch = cnt.copy(), total.copy(), np.full((P, S), -1, np.int64)      # prediction i stays unmatched
            for g in range(G):                                                         # g ascending
                bit = 1 << g
                pc = cnt[:, ms ^ bit]
                cand_c, cand_s = pc + 1, total[:, ms ^ bit] + cost[:, i, g][:, None]
                ok = ((ms & bit) != 0)[None] & allow[:, i, g][:, None] & (pc >= 0)
                ok = ok & ((cand_c > bc) | ((cand_c == bc) & (cand_s < bs)))             # a strict improvement only
                bc, bs, ch = np.where(ok, cand_c, bc), np.where(ok, cand_s, bs), np.where(ok, g, ch)
            cnt, total = bc, bs
            choice[:, i] = ch
        best_m, best_c, best_s = np.zeros(P, np.int64), np.full(P, -1, np.int64), np.zeros(P, np.float64)
        for m in range(S):                                                             # m ascending
            ok = (cnt[:, m] >= 0) & ((cnt[:, m] > best_c) | ((cnt[:, m] == best_c) & (total[:, m] < best_s)))
            best_m, best_c, best_s = np.where(ok, m, best_m), np.where(ok, cnt[:, m], best_c), np.where(ok, total[:, m], best_s)
    match = np.full((P, K), -1, np.int32)
    m = best_m.copy()
    rows = np.arange(P)
    for i in range(K - 1, -1, -1):
        g = choice[rows, i, m]
        match[:, i] = g
        m = np.where(g >= 0, m ^ (1 << np.maximum(g, 0)), m)
    return match, best_c, best_s


def match_hands(pred, truth, flags=None, valid=None, truth_valid=None, trans=None, group=None, gate=np.inf, min_points=1):
    """-> {'match' int32 [B,K,2], 'pred_of' int32 [B,G,2], 'cost' float32 [B,K,2], 'counts' int32 [B,2,3], 'group' int32 [B,G,2]}."""
    pred, truth = np.asarray(pred, np.float32), np.asarray(truth, np.float32)
    B, K = pred.shape[:2]
    G = truth.shape[1]
    cost, count = pair_costs(pred, truth, valid, trans)
    allow = allowed_pairs(cost, count, flags, truth_valid, gate, min_points)
    to_p = lambda a: a.transpose(0, 3, 1, 2).reshape(B * 2, K, G)      # a problem is (b, s)
    m, _, _ = solve(to_p(cost), to_p(allow))
    match = m.reshape(B, 2, K).transpose(0, 2, 1).astype(np.int32)
    pred_of = np.full((B, G, 2), -1, np.int32)
    out_cost = np.full((B, K, 2), -1, np.float32)
    for b, i, s in zip(*np.nonzero(match >= 0)):
        pred_of[b, match[b, i, s], s] = i
        out_cost[b, i, s] = np.float32(cost[b, i, match[b, i, s], s])
    flagged = np.ones((B, K, 2), bool) if flags is None else finite_gt_half(flags)
    tv = np.ones((B, G, 2), bool) if truth_valid is None else np.asarray(truth_valid) != 0
    tp = (match >= 0).sum(1)
    counts = np.stack([tp, flagged.sum(1) - tp, tv.sum(1) - tp], -1).astype(np.int32)      # [B,2,3]
    side = np.broadcast_to(np.arange(2, dtype=np.int32), (B, G, 2))
    grp = np.where(tv, side if group is None else np.asarray(group, np.int32), -1).astype(np.int32)
    return {'match': match, 'pred_of': pred_of, 'cost': out_cost, 'counts': counts, 'group': grp}


def finite_gt_half(flags):
    with np.errstate(invalid='ignore'):
        return np.asarray(flags, np.float32) > np.float32(0.5)


def gather(src, index):
    """dst[b,q,s] = src[b, index[b,q,s], s], +0 where the index is outside [0, Ks)."""
    src, index = np.asarray(src), np.asarray(index)
    B, Ks = src.shape[:2]
    dst = np.zeros(index.shape + src.shape[3:], src.dtype)
    for b, q, s in itertools.product(range(B), range(index.shape[1]), range(2)):
        k = int(index[b, q, s])
        if 0 <= k < Ks:
            dst[b, q, s] = src[b, k, s]
    return dst


def accumulate(words, counts, cost):
    """The board after one more call: words int64 [8] (per side TP, FP, FN, the bits of the fp64 cost sum) -> a new array."""
    words = np.array(words, np.int64)
    sums = words.view(np.float64)
    for s in range(2):
        for k in range(3):
            words[4 * s + k] += int(np.asarray(counts)[:, s, k].astype(np.int64).sum())
        v = np.float64(sums[4 * s + 3])
        for c in np.asarray(cost, np.float32)[:, :, s].reshape(-1):      # ascending frame, then prediction
            if c >= 0:
                v = v + np.float64(c)
        sums[4 * s + 3] = v
    return words


def brute_force(cost, allow):
    """The objective by exhaustive enumeration: cost [K,G], allow [K,G] -> (the most pairs, the smallest cost sum among those)."""
    K, G = cost.shape
    best = (0, 0.0)
    for r in range(1, min(K, G) + 1):
        for preds in itertools.combinations(range(K), r):
            for truths in itertools.permutations(range(G), r):
                if all(allow[i, g] for i, g in zip(preds, truths)):
                    total = float(sum(cost[i, g] for i, g in zip(preds, truths)))
                    if r > best[0] or (r == best[0] and total < best[1]):
                        best = (r, total)
    return best
