"""The rule of csrc/point_plan.h restated in numpy, on top of tests/multi_ref.py: at which pixels the head towers of a side run
when the point heads serve the K best centres of each side.

Test infrastructure, not product.  Integers only, so the check program and the device are compared exactly.
"""
import numpy as np

import multi_ref as M


def distinct(values, lo=0):
    """The values >= lo, each once, in the order of first appearance."""
    out = []
    for v in values:
        v = int(v)
        if v >= lo and v not in out:
            out.append(v)
    return out


def plan(flat, partner):
    """flat, partner [K,2] of one frame (multi_ref.topk / partners) -> {'own': (left, right), 'prior': (left, right)}: per side
    the pixels of its params and cam towers and of its mix (the distinct flat indices; a rank without a detection samples pixel
    0), and the pixels of its prior tower (the distinct partners >= 0)."""
    flat, partner = np.asarray(flat), np.asarray(partner)
    return {'own': tuple(distinct(flat[:, s]) for s in (0, 1)), 'prior': tuple(distinct(partner[:, s]) for s in (0, 1))}


def plan_of_maps(center_l, center_r, K, thresh=M.CONF_THRESH):
    """Two centre maps [64,64] of one frame -> (flag [K,2], flat [K,2], partner [K,2], plan)."""
    flag = np.zeros((K, 2), bool)
    flat = np.zeros((K, 2), np.int64)
    for s, c in enumerate((center_l, center_r)):
        flag[:, s], flat[:, s], _ = M.topk(c, K, thresh)
    partner = M.partners(flag, flat)
    return flag, flat, partner, plan(flat, partner)
