"""The association rule of csrc/assoc_plan.h restated in numpy / plain Python, and the scenarios the
host and GPU tests share.  Integers throughout: the library has to agree exactly.

A side's tracks: {'next_id': int, 'slots': [K dicts or None]}; a live slot is {'id', 'miss', 'cy', 'cx'}."""
import numpy as np

SLOT, FLAG, FLATIND, SCORE, POSES, BETAS = 176, 0, 1, 2, 6, 54


def new_side(K):
    return {'next_id': 0, 'slots': [None] * K}


def detection(flag, v):
    """-> (cy, cx) or None.  A float that fails the range check is never converted."""
    flag, v = np.float32(flag), np.float32(v)
    if not flag > np.float32(0.5):
        return None
    if not (v >= np.float32(0) and v < np.float32(4096)):
        return None
    i = int(v)
    return i >> 6, i & 63


def step(side, rows, gate, max_miss):
    """One frame of one (stream, side): rows [K,>=2] in rank order -> (track_ids [K], perm [K], born [K]); side is updated."""
    K = len(side['slots'])
    dets = [detection(rows[j][FLAG], rows[j][FLATIND]) for j in range(K)]
    slots = side['slots']
    of_slot = [None] * K
    taken = [False] * K
    while True:
        cands = []
        for t in range(K):
            if slots[t] is None or of_slot[t] is not None:
                continue
            for j in range(K):
                if dets[j] is None or taken[j]:
                    continue
                c = (dets[j][0] - slots[t]['cy']) ** 2 + (dets[j][1] - slots[t]['cx']) ** 2
                if c <= gate * gate:
                    cands.append((c, t, j))
        if not cands:
            break
        c, t, j = min(cands)
        of_slot[t], taken[j] = j, True
        slots[t].update(miss=0, cy=dets[j][0], cx=dets[j][1])
    for t in range(K):
        if slots[t] is not None and of_slot[t] is None:
            slots[t]['miss'] += 1
            if max_miss >= 0 and slots[t]['miss'] > max_miss:
                slots[t] = None
    born = [0] * K
    for j in range(K):
        if dets[j] is None or taken[j]:
            continue
        free = [t for t in range(K) if slots[t] is None]
        if free:
            t = free[0]
        else:
            t = max((t for t in range(K) if of_slot[t] is None), key=lambda t: (slots[t]['miss'], -t))
        slots[t] = {'id': side['next_id'], 'miss': 0, 'cy': dets[j][0], 'cx': dets[j][1]}
        side['next_id'] += 1
        of_slot[t], taken[j], born[t] = j, True, 1
    rest = [j for j in range(K) if not taken[j]]
    perm = [of_slot[k] if of_slot[k] is not None else rest.pop(0) for k in range(K)]
    ids = [slots[k]['id'] if of_slot[k] is not None else -1 for k in range(K)]
    return np.array(ids, np.int32), np.array(perm, np.int32), np.array(born, np.int32)


def run(slots, ids, K, gate, max_miss, state=None):
    """The rule on a whole batch: slots [B,K,2,176], ids [B] -> (reordered slots, track_ids [B,K,2], perm [B,K,2], born
    [B,K,2], state).  state: {stream: [left side, right side]}, carried from an earlier call; no smoothing."""
    slots = np.asarray(slots)
    B = slots.shape[0]
    out = slots.copy()
    tids = np.full((B, K, 2), -1, np.int32)
    perm = np.tile(np.arange(K, dtype=np.int32)[None, :, None], (B, 1, 2))
    born = np.zeros((B, K, 2), np.int32)
    state = {} if state is None else state
    for b in range(B):
        s = int(ids[b])
        if s < 0:
            continue
        sides = state.setdefault(s, [new_side(K), new_side(K)])
        for h in (0, 1):
            tids[b, :, h], perm[b, :, h], born[b, :, h] = step(sides[h], slots[b, :, h], gate, max_miss)
            out[b, :, h] = slots[b, perm[b, :, h], h]
    return out, tids, perm, born, state


def make_slots(frames, K, seed=0):
    """frames: per frame (left list, right list) of (cy, cx) or None (a placeholder) or a raw (flag, flatind) pair given as
    {'flag': f, 'flat': v}, in RANK order -> float32 [B,K,2,176] with distinct random contents per row."""
    g = np.random.default_rng(seed)
    B = len(frames)
    s = g.normal(0, 0.3, (B, K, 2, SLOT)).astype(np.float32)
    for b, sides in enumerate(frames):
        for h in (0, 1):
            hands = list(sides[h]) + [None] * (K - len(sides[h]))
            for k, hand in enumerate(hands):
                if hand is None:
                    s[b, k, h, FLAG], s[b, k, h, FLATIND] = 0.0, 0.0
                elif isinstance(hand, dict):
                    s[b, k, h, FLAG], s[b, k, h, FLATIND] = hand['flag'], hand['flat']
                else:
                    s[b, k, h, FLAG], s[b, k, h, FLATIND] = 1.0, float(hand[0] * 64 + hand[1])
    return s


# ---- the scenarios: name -> (K, gate, max_miss, frames of ONE stream) ----
def scenarios():
    sc = {}
    a, b = (10, 10), (40, 40)
    sc['rank_swap'] = (2, 8, 5, [([a, b], []) if t % 2 == 0 else ([b, a], []) for t in range(6)])
    # a jump of exactly `gate` pixels continues (c == gate * gate); 8 px and 1 px more does not (c == 65 = gate * gate + 1)
    sc['gate_on'] = (2, 8, 5, [([(10, 10)], []), ([(10, 18)], []), ([(18, 18)], [])])
    sc['gate_off'] = (2, 8, 5, [([(10, 10)], []), ([(18, 11)], [])])
    for name, gap, mm in (('miss_within', 3, 3), ('miss_beyond', 4, 3), ('miss_never', 40, -1)):
        sc[name] = (2, 8, mm, [([(10, 10), (40, 40)], [])] + [([(40, 40)], [])] * gap + [([(40, 40), (10, 10)], [])])
    sc['eviction'] = (2, 4, 5, [([(5, 5), (50, 50)], []), ([(5, 5)], []), ([(20, 20), (30, 30)], [])])
    # two tracks equidistant from one detection: the lower slot wins; one track equidistant from two detections: the lower rank
    sc['tie_tracks'] = (2, 8, 5, [([(10, 10), (10, 14)], []), ([(10, 12)], [])])
    sc['tie_dets'] = (2, 8, 5, [([(10, 12)], []), ([(10, 14), (10, 10)], [])])
    # greedy takes (track 1, rank 0) at distance 2 and leaves track 0 with rank 1 at 11 > gate 6: track 0 is evicted by a birth.
    # The optimal assignment (track 0 - rank 0 at 4, track 1 - rank 1 at 5) would have kept all three.
    sc['greedy'] = (3, 6, 5, [([(10, 10), (10, 16), (40, 40)], []), ([(10, 14), (10, 21), (40, 40)], [])])
    sc['ordering'] = (3, 8, 0, [([(5, 5), (20, 20), (40, 40)], []), ([(40, 40)], [(7, 7)]), ([(40, 40), (60, 60), (50, 5)], [(7, 7), (30, 30)]),
                                ([(50, 5)], [(30, 30)])])
    nan = float('nan')
    sc['garbage'] = (3, 8, 5, [([(10, 10), {'flag': nan, 'flat': 700.0}, {'flag': 1.0, 'flat': nan}], [{'flag': 1.0, 'flat': -1.0}, (20, 20)]),
                               ([{'flag': 1.0, 'flat': 4096.0}, (10, 11), {'flag': 1.0, 'flat': 1e30}],
                                [{'flag': 0.5, 'flat': 100.0}, {'flag': 1.0, 'flat': float('inf')}, (20, 21)]),
                               ([{'flag': float('inf'), 'flat': 4095.5}, {'flag': 1.0, 'flat': float('-inf')}, (10, 12)],
                                [{'flag': -1.0, 'flat': 5.0}, (20, 22), {'flag': 1.0, 'flat': -0.0}])])
    return sc


def interleaved(K, n=259, seed=3):
    """n frames over three interleaved streams (ids 0, 2, 5 of a table of 6) with -1 frames among them: hands wander, swap
    ranks, vanish and come back.  -> (frames, ids)"""
    g = np.random.default_rng(seed)
    ids = g.choice(np.array([0, 2, 5, -1]), size=n, p=[0.35, 0.3, 0.25, 0.1]).astype(np.int32)
    pos = {s: [[(int(g.integers(4, 60)), int(g.integers(4, 60))) for _ in range(K)] for _ in (0, 1)] for s in (0, 2, 5, -1)}
    frames = []
    for b in range(n):
        s = int(ids[b])
        sides = []
        for h in (0, 1):
            hands = []
            for k in range(K):
                cy, cx = pos[s][h][k]
                cy = int(np.clip(cy + g.integers(-4, 5), 0, 63))
                cx = int(np.clip(cx + g.integers(-4, 5), 0, 63))
                pos[s][h][k] = (cy, cx)
                if g.random() < 0.65:
                    hands.append((cy, cx))
            order = g.permutation(len(hands))
            sides.append([hands[i] for i in order])
        frames.append(tuple(sides))
    return frames, ids
