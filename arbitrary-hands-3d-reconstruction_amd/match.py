"""Host side of matching decoded hands to ground truth (the rule: csrc/match_plan.h): the layout of the
device board, its one host visit - the summary arithmetic - and the two match keys of a hand dict.  Pure numpy: nothing here
needs a device."""
import numpy as np

MAX_HANDS, MAX_POINTS = 8, 256      # = csrc/match_plan.h
BOARD_WORDS = 8                     # per side TP, FP, FN int64, the matched-cost sum fp64
MATCH_KEYS = ('gt_index', 'match_cost')      # what match= adds to every hand dict
ON_KEYS = ('pj2d_org', 'pj2d', 'joints')     # what Engine.match compares


def board_arrays(words):
    """The board's words (int64 [8]) -> {'tp', 'fp', 'fn' int64 [2], 'cost_sum' float64 [2]}, per side."""
    w = np.ascontiguousarray(words, np.int64)
    if w.shape != (BOARD_WORDS,):
        raise ValueError('a match board has %d words, got %s' % (BOARD_WORDS, list(w.shape)))
    w = w.reshape(2, 4)
    return {'tp': w[:, 0].copy(), 'fp': w[:, 1].copy(), 'fn': w[:, 2].copy(), 'cost_sum': w[:, 3].copy().view(np.float64)}


def _rates(tp, fp, fn, cost_sum):
    nan = float('nan')
    tp, fp, fn = int(tp), int(fp), int(fn)
    return {'tp': tp, 'fp': fp, 'fn': fn,
            'precision': tp / (tp + fp) if tp + fp else nan,
            'recall': tp / (tp + fn) if tp + fn else nan,
            'f1': 2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else nan,
            'mean_cost': float(cost_sum) / tp if tp else nan}


def summarize(arrays):
    """board_arrays -> {'sides': [left, right], 'all': ...}, each {'tp', 'fp', 'fn', 'precision' = TP / (TP + FP), 'recall' = TP
    / (TP + FN), 'f1' = 2 TP / (2 TP + FP + FN), 'mean_cost' = the matched-cost sum / TP}; nan where a denominator is zero."""
    a = arrays
    sides = [_rates(a['tp'][s], a['fp'][s], a['fn'][s], a['cost_sum'][s]) for s in range(2)]
    return {'sides': sides, 'all': _rates(a['tp'].sum(), a['fp'].sum(), a['fn'].sum(), a['cost_sum'][0] + a['cost_sum'][1])}


def hand_match_keys(match, cost, row):
    """The two match keys of the hand in row `row` of the flattened [B,K,2] outputs."""
    return {'gt_index': np.int32(match.reshape(-1)[row]), 'match_cost': np.float32(cost.reshape(-1)[row])}
