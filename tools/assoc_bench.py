"""Cost of the tracks (engine.TrackTable) on one GPU, one JSON line.

    python tools/assoc_bench.py [--repeats 30] [--warmup 5] [--rounds 3] [--timeout 600] [--out FILE]

  association alone  HIP events around one call as the caller sees it, median of `repeats`: 64 frames of 64 streams through
                     Engine.associate (order, ids and smoothing) at K = 1, 2, 4, 8 hands per side, next to
                     Engine.smooth(streams=, table=) on the same 64 frames (K = 1 rows) in the same process; and one stream
                     of 64 frames at K = 4 - the serial chain: one workgroup walks all 64 frames.
  fused call         Engine.forward(max_hand=4) and Engine.forward(max_hand=4, tracks=, track_table=) on the bench frames at
                     batch 64 and batch 1 (a context loaded for each), alternated `rounds` times.
The run ends itself after `--timeout` seconds."""
import argparse
import importlib
import json
import os
import signal
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = 'arbitrary-hands-3d-reconstruction_amd'


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4)}


def walk_slots(L, n, K):
    """n frames of K hands per side, all flagged: centres that wander by a pixel or two and swap ranks from frame to frame,
    poses and betas of a random walk."""
    g = np.random.default_rng(0)
    s = np.zeros((n, K, 2, L.SLOT), np.float32)
    s[..., L.SLOT_FLAG] = 1.0
    home = np.stack([8 + 48 * np.arange(K) // max(K - 1, 1), 8 + 6 * np.arange(K)], -1)      # [K,2] (cy, cx), >= 6 px apart
    walk = np.clip(home[None, :, None, :] + np.cumsum(g.integers(-1, 2, (n, K, 2, 2)), 0), 0, 63)
    s[..., L.SLOT_POSES:L.SLOT_POSES + 48] = np.cumsum(g.normal(0, 0.12, (n, K, 2, 48)), 0)
    s[..., L.SLOT_BETAS:L.SLOT_BETAS + 10] = np.cumsum(g.normal(0, 0.05, (n, K, 2, 10)), 0)
    s[..., L.SLOT_FLATIND] = walk[..., 0] * 64 + walk[..., 1]
    for b in range(n):      # rank order changes every frame
        s[b] = s[b, g.permutation(K)]
    return torch.from_numpy(s).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3, help='alternations of the fused variants')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--timeout', type=int, default=600, help='seconds after which the run ends itself')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('assoc_bench needs a GPU: there is no CPU path to time')
    signal.alarm(a.timeout)
    pkg = lambda sub: importlib.import_module(PKG + '.' + sub)
    synth, L, E = pkg('synth'), pkg('_lib'), pkg('engine')
    B = a.batch
    line = {'tool': 'assoc_bench', 'device': torch.cuda.get_device_name(0), 'repeats': a.repeats, 'warmup': a.warmup, 'batch': B,
            'timing': 'HIP events around the call as the caller sees it, median'}
    eng = E.Engine(0)

    # ---- association + smoothing alone ----
    alone = {}
    ids = np.arange(B, dtype=np.int32)
    streams = E.StreamTable(0, B)
    one_hand = walk_slots(L, B, 1)
    work = one_hand[:, 0].clone()
    alone['smooth_streams_%dx1' % B] = timed(lambda: eng.smooth(work, streams=ids, table=streams), a.warmup, a.repeats)
    streams.close()
    for K in (1, 2, 4, 8):
        table = E.TrackTable(0, B, K)
        slots = walk_slots(L, B, K)
        alone['associate_%dx1_K%d' % (B, K)] = timed(lambda: eng.associate(slots, ids, table, smooth=True), a.warmup, a.repeats)
        alone['associate_%dx1_K%d_order_only' % (B, K)] = timed(lambda: eng.associate(slots, ids, table, smooth=False), a.warmup, a.repeats)
        table.close()
    table = E.TrackTable(0, 1, 4)
    slots = walk_slots(L, B, 4)
    chain = np.zeros(B, np.int32)
    alone['associate_1x%d_K4_serial_chain' % B] = timed(lambda: eng.associate(slots, chain, table, smooth=True), a.warmup, a.repeats)
    table.close()
    line['association_alone'] = alone

    # ---- fused call ----
    sd = synth.make_state_dict(seed=0)
    tables = synth.make_mano_tables(seed=1)
    tables['left']['shapedirs'] = tables['left']['shapedirs'].copy()
    tables['left']['shapedirs'][:, 0, :] *= -1
    fused = {}
    K = 4
    for n in (B, 1):      # a context built for the batch it runs, as a caller's would be (the lowering depends on max_batch)
        fe = E.Engine(0)
        fe.load_state_dict(sd, max_batch=n)
        fe.load_mano(tables)
        frames = torch.from_numpy(synth.make_frames(n, seed=0, structured=False)).cuda()
        table = E.TrackTable(0, n, K)
        fid = np.arange(n, dtype=np.int32)
        runs = {'forward_K4': [], 'forward_K4_tracks': []}
        for _ in range(a.rounds):      # the variants alternate, so that a drift of the machine meets both
            runs['forward_K4'].append(timed(lambda: fe.forward(frames, max_hand=K), a.warmup, a.repeats)['median_ms'])
            runs['forward_K4_tracks'].append(timed(lambda: fe.forward(frames, max_hand=K, tracks=fid, track_table=table),
                                                   a.warmup, a.repeats)['median_ms'])
        fused['batch_%d_ms' % n] = runs
        table.close()
        fe.close()
    line['fused'] = fused
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    eng.close()


if __name__ == '__main__':
    main()
