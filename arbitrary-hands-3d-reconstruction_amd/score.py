"""Host side of scoring against ground truth (the rule: csrc/score_plan.h): the layout of the device
board, its one host visit - the summary arithmetic - and the four score keys of a hand dict.  Pure numpy: nothing here needs
a device."""
import numpy as np

MAX_POINTS, MAX_GROUPS, MAX_BINS = 4000, 16, 4096      # = csrc/score_plan.h
N_BINS, BIN_WIDTH = 100, 0.0005      # 100 bins of 0.5 mm: defaults of PARAMETERS, not measurements
SCORE_KEYS = ('mpjpe', 'pa_mpjpe', 'mpvpe', 'pa_mpvpe')      # what gt= adds to every hand dict


def check_board_params(sets, n_groups, n_bins, bin_width):
    sets = tuple(int(n) for n in sets)
    if not sets or any(not 1 <= n <= MAX_POINTS for n in sets):
        raise ValueError('point sets of 1..%d points' % MAX_POINTS)
    if int(n_groups) != n_groups or not 1 <= n_groups <= MAX_GROUPS:
        raise ValueError('n_groups %r: an integer in 1..%d' % (n_groups, MAX_GROUPS))
    if int(n_bins) != n_bins or not 1 <= n_bins <= MAX_BINS:
        raise ValueError('n_bins %r: an integer in 1..%d' % (n_bins, MAX_BINS))
    bin_width = float(bin_width)
    if not 0 < bin_width < float('inf'):
        raise ValueError('bin_width must be finite and > 0')
    return sets, int(n_groups), int(n_bins), bin_width


def group_words(n, n_bins):
    """8-byte words of one group of a set's board: sum_ra[n] sum_pa[n] cnt_ra[n] cnt_pa[n] hist[n_bins + 1] scored missed."""
    return 4 * n + n_bins + 3


def board_layout(sets, n_groups, n_bins):
    """-> ([word offset of each set's board], word offset of the pair board, words in all): the sets' boards in order, then
    the pair board [n_groups, n_groups, 2]."""
    offs, at = [], 0
    for n in sets:
        offs.append(at)
        at += group_words(n, n_bins) * n_groups
    return offs, at, at + 2 * n_groups * n_groups


def board_arrays(words, sets, n_groups, n_bins):
    """The board's words (int64 [words], on the host) -> ([per set {'sum_ra', 'sum_pa' float64 [G,n], 'cnt_ra', 'cnt_pa' int64
    [G,n], 'hist' int64 [G,n_bins + 1], 'scored', 'missed' int64 [G]}], {'pair_sum' float64 [G,G], 'pair_cnt' int64 [G,G]})."""
    words = np.ascontiguousarray(words, dtype=np.int64)
    offs, pair_at, total = board_layout(sets, n_groups, n_bins)
    if words.shape != (total,):
        raise ValueError('the board holds %d words, its layout %d' % (words.size, total))
    out = []
    for n, at in zip(sets, offs):
        gw = group_words(n, n_bins)
        b = words[at:at + gw * n_groups].reshape(n_groups, gw)
        out.append({'sum_ra': b[:, 0:n].copy().view(np.float64), 'sum_pa': b[:, n:2 * n].copy().view(np.float64),
                    'cnt_ra': b[:, 2 * n:3 * n].copy(), 'cnt_pa': b[:, 3 * n:4 * n].copy(),
                    'hist': b[:, 4 * n:4 * n + n_bins + 1].copy(), 'scored': b[:, 4 * n + n_bins + 1].copy(),
                    'missed': b[:, 4 * n + n_bins + 2].copy()})
    p = words[pair_at:].reshape(n_groups, n_groups, 2)
    return out, {'pair_sum': p[:, :, 0].copy().view(np.float64), 'pair_cnt': p[:, :, 1].copy()}


def _mean(total, count):
    return float(total) / float(count) if count > 0 else float('nan')


def _table(sums, counts):
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(counts > 0, sums / np.maximum(counts, 1), np.nan)


def pck_curve(hist, bin_width):
    """hist int64 [n_bins + 1] (the last bin: everything beyond the range) -> (thresholds [n_bins + 1] = k * bin_width, pck
    [n_bins + 1] = the share of the errors below each threshold, AUC = the trapezoid rule over the bins, divided by the range).
    Without an error the curve and the AUC are nan."""
    hist = np.asarray(hist, np.int64)
    n_bins = hist.shape[0] - 1
    thresholds = np.arange(n_bins + 1, dtype=np.float64) * bin_width
    total = int(hist.sum())
    if total == 0:
        return thresholds, np.full(n_bins + 1, np.nan), float('nan')
    below = np.concatenate(([0], np.cumsum(hist[:n_bins]))).astype(np.float64)
    pck = below / total
    auc = float(((pck[:-1] + pck[1:]) * 0.5).sum() / n_bins)
    return thresholds, pck, auc


def _set_summary(b, rows, bin_width):
    """One set's sums over the groups `rows` (an index array) -> its part of the summary."""
    sra, spa = b['sum_ra'][rows].sum(0), b['sum_pa'][rows].sum(0)
    cra, cpa = b['cnt_ra'][rows].sum(0), b['cnt_pa'][rows].sum(0)
    _, pck, auc = pck_curve(b['hist'][rows].sum(0), bin_width)
    return {'ra': _mean(sra.sum(), cra.sum()), 'pa': _mean(spa.sum(), cpa.sum()), 'per_point_ra': _table(sra, cra),
            'per_point_pa': _table(spa, cpa), 'pck': pck, 'auc': auc, 'n_ra': int(cra.sum()), 'n_pa': int(cpa.sum())}


def summarize(sets_arrays, pair_arrays, names, bin_width):
    """The summary of a board (board_arrays' result): {'thresholds', 'all': {...}, 'groups': [{...} per group]}; each {...} has,
    per set name ('joints', 'verts'): {'ra', 'pa': the mean errors in metres over every counted point - MPJPE / PA-MPJPE of the
    joints, MPVPE / PA-MPVPE of the vertices -, 'per_point_ra', 'per_point_pa' [n], 'pck' [n_bins + 1], 'auc', 'n_ra', 'n_pa'},
    the same four means under 'mpjpe', 'pa_mpjpe', 'mpvpe', 'pa_mpvpe' where the sets are called joints / verts, 'scored',
    'missed' (rows) and 'mrrpe' with 'n_pairs' (a group: the pairs whose LEFT hand is of that group).  'mrrpe_pairs' [G,G] is
    the table by (left group, right group).  A mean without a counted element is nan."""
    G = sets_arrays[0]['scored'].shape[0]
    n_bins = sets_arrays[0]['hist'].shape[1] - 1

    def part(rows, psum, pcnt):
        d = {name: _set_summary(b, rows, bin_width) for name, b in zip(names, sets_arrays)}
        for name, keys in (('joints', ('mpjpe', 'pa_mpjpe')), ('verts', ('mpvpe', 'pa_mpvpe'))):
            if name in d:
                d[keys[0]], d[keys[1]] = d[name]['ra'], d[name]['pa']
        d['scored'] = int(sets_arrays[0]['scored'][rows].sum())
        d['missed'] = int(sets_arrays[0]['missed'][rows].sum())
        d['mrrpe'], d['n_pairs'] = _mean(psum.sum(), pcnt.sum()), int(pcnt.sum())
        return d

    every = np.arange(G)
    return {'thresholds': np.arange(n_bins + 1, dtype=np.float64) * bin_width,
            'all': part(every, pair_arrays['pair_sum'], pair_arrays['pair_cnt']),
            'groups': [part(np.array([g]), pair_arrays['pair_sum'][g], pair_arrays['pair_cnt'][g]) for g in range(G)],
            'mrrpe_pairs': _table(pair_arrays['pair_sum'], pair_arrays['pair_cnt'])}


def hand_score_keys(scores, row):
    """The four score keys of the hand in row `row` (b, k, h flattened) of Engine.score's result on the host: `scores` =
    {'joints': row_f [N,4], 'verts': row_f [N,4] or None}.  nan for a hand without truth (a row that was not scored, or has
    no counted point), and for the vertex keys without vertex truth."""
    def pick(name, col):
        rf = scores.get(name)
        v = np.float32(-1) if rf is None else np.float32(rf[row, col])
        return np.float32(np.nan) if not v >= 0 else v

    return {'mpjpe': pick('joints', 0), 'pa_mpjpe': pick('joints', 1), 'mpvpe': pick('verts', 0), 'pa_mpvpe': pick('verts', 1)}
