"""Cost of tracking on the device (csrc/track.hip, the device-box window kernels of csrc/preprocess.hip; DESIGN.md "Tracking on
the device") next to the same work through the host, on one GPU, one JSON line.

    python tools/track_bench.py [--repeats 30] [--iters 100] [--runs 3] [--warmup 5] [--frames 64] [--size 480]
                                [--timeout 900] [--out FILE]

(a) One call of 64 regions of 480 x 480, one out of each of 64 frames of 1080 x 1920: ops.preprocess_rois_device (boxes in device
    memory) next to ops.preprocess_rois (boxes on the host), on BGR frames and on NV12 surfaces.  HIP events around the call as
    the caller sees it, median of `repeats`, the two alternated, `runs` runs; the bytes and the offsets rows must be equal.
(b) The video loop frame k -> boxes -> frame k+1 on whole-frame boxes to start with, wall clock per iteration of `iters`
    iterations that end in ONE synchronise:
      host    the loop as it is written without the feature: ops.preprocess_rois, Engine.forward, .cpu() of the flags and
              key points, acr.utils.boxes_from_keypoints
      device  Engine.track_step
      pool    (batch 64) an EnginePool of two: ops.preprocess_rois_device, submit, EnginePool.track_boxes, with the ticket of
              batch k left outstanding behind the submit of batch k + 1
    at batch 1 (one 1080p stream) and batch 64 on one context, alternated, `runs` runs; the boxes after the last iteration
    must be equal.
No ratio is asserted: the tool reports.  The run ends itself after `--timeout` seconds."""
import argparse
import importlib
import json
import os
import signal
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = 'arbitrary-hands-3d-reconstruction_amd'
H, W = 1080, 1920
SCALE, MIN_SIZE = 1.0, 64      # (the synthetic checkpoint spreads its hands wide: at 1.5 every box is the whole frame again)


def pkg(sub):
    return importlib.import_module(PKG + '.' + sub)


def smooth_nv12(n, seed):
    """n NV12 surfaces [n, H*3/2, W] of smooth pictures (tools/roi_bench.py's)."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H * 3 // 2, 0:W].astype(np.float32)
    out = np.empty((n, H * 3 // 2, W), np.uint8)
    for i in range(n):
        a, b, c = g.uniform(0.002, 0.02, 3)
        out[i] = (127.5 + 127.5 * np.sin(a * xx + b * yy + 6.28 * c * i)).astype(np.uint8)
    return torch.from_numpy(out)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternated(fns, warmup, repeats, runs):
    """{name: fn} timed in turn, `repeats` rounds per run -> {name: {'median_ms': [per run], 'min_ms', 'max_ms' of the medians}}"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    med = {k: [] for k in fns}
    for _ in range(runs):
        ms = {k: [] for k in fns}
        for _ in range(repeats):
            for k, fn in fns.items():
                ms[k].append(event_ms(fn))
        for k in fns:
            med[k].append(round(statistics.median(ms[k]), 4))
    return {k: {'median_ms': v, 'min_ms': min(v), 'max_ms': max(v)} for k, v in med.items()}


def host_boxes(out, hw, S, utils):
    """The next boxes through the host: the flags and key points copied back, the numpy rule; a row without pixels (which
    ops.preprocess_rois would refuse) is the whole frame."""
    flags = out['slots'][:, :, S.SLOT_FLAG].cpu().numpy() > 0.5
    pj = out['pj2d_org'].cpu().numpy()
    boxes = utils.boxes_from_keypoints([pj[i][flags[i]].reshape(-1, 2) for i in range(len(pj))], hw, scale=SCALE, min_size=MIN_SIZE)
    empty = (boxes[:, 2] <= boxes[:, 0]) | (boxes[:, 3] <= boxes[:, 1])
    boxes[empty] = (0, 0, hw[1], hw[0])
    return boxes, int(flags.sum())


def loops(frames, eng, pool, iters):
    """({name: fn() -> (seconds per iteration, the boxes after the last iteration as numpy)}, what the host loop saw)"""
    ops, S, utils = pkg('ops'), pkg('_lib'), pkg('acr.utils')
    n = len(frames)
    whole = np.array([[0, 0, W, H]] * n, np.int32)
    whole_dev = torch.from_numpy(whole).cuda()
    stats = {}

    def host(k=iters):
        boxes, hands = whole, 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            rgb, offsets = ops.preprocess_rois(frames, boxes)
            out = eng.forward(rgb, offsets=offsets, project=True)
            boxes, hands = host_boxes(out, (H, W), S, utils)
        torch.cuda.synchronize()
        stats['hands_detected'] = hands
        return (time.perf_counter() - t0) / k, boxes

    def device(k=iters):
        boxes = whole_dev
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            _, boxes, _ = eng.track_step(frames, boxes, frame_hw=(H, W), scale=SCALE, min_size=MIN_SIZE)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k, boxes.cpu().numpy()

    def pooled(k=iters):
        boxes, before = whole_dev, None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            rgb, offsets, _ = ops.preprocess_rois_device(frames, boxes)
            ticket = pool.submit(rgb, offsets=offsets, project=True)
            boxes = pool.track_boxes(ticket, (H, W), scale=SCALE, min_size=MIN_SIZE)
            if before is not None:
                pool.collect(before)
            before = ticket
        pool.collect(before)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k, boxes.cpu().numpy()

    fns = {'host': host, 'device': device}
    if pool is not None:
        fns['pool'] = pooled
    return fns, stats


def time_loops(fns_stats, warmup, runs):
    fns, stats = fns_stats
    for fn in fns.values():
        fn(warmup)
    per = {k: [] for k in fns}
    last = {}
    for _ in range(runs):
        for k, fn in fns.items():
            s, last[k] = fn()
            per[k].append(round(s * 1e3, 4))
    res = {k: {'ms_per_iteration': v, 'min_ms': min(v), 'max_ms': max(v)} for k, v in per.items()}
    res['boxes_equal'] = bool(all((b == last['host']).all() for b in last.values()))
    res['hands_detected_in_the_last_iteration'] = stats['hands_detected']
    res['regions_not_whole_frame'] = int((last['host'] != np.array([0, 0, W, H])).any(1).sum())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--size', type=int, default=480, help='side of the square regions of (a)')
    ap.add_argument('--timeout', type=int, default=900, help='seconds after which the run ends itself')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('track_bench needs a GPU: there is no CPU path to time')
    signal.alarm(a.timeout)
    ops, synth, engine = pkg('ops'), pkg('synth'), pkg('engine')
    n, side = a.frames, a.size
    nv12 = list(smooth_nv12(n, seed=H).cuda().unbind(0))
    bgr = list(ops.nv12_to_bgr(nv12).unbind(0))
    g = np.random.default_rng(0)
    boxes = [(int(l), int(t), int(l) + side, int(t) + side)
             for l, t in zip(g.integers(0, W - side + 1, n), g.integers(0, H - side + 1, n))]
    boxes_dev = torch.tensor(boxes, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    # (a)
    call = alternated({
        'host_boxes_bgr': lambda: ops.preprocess_rois(bgr, boxes),
        'device_boxes_bgr': lambda: ops.preprocess_rois_device(bgr, boxes_dev),
        'host_boxes_nv12': lambda: ops.preprocess_rois(nv12, boxes, pixel_format='nv12'),
        'device_boxes_nv12': lambda: ops.preprocess_rois_device(nv12, boxes_dev, pixel_format='nv12'),
    }, a.warmup, a.repeats, a.runs)
    for frames, kw in ((bgr, {}), (nv12, dict(pixel_format='nv12'))):
        want, want_off = ops.preprocess_rois(frames, boxes, **kw)
        got, got_off, status = ops.preprocess_rois_device(frames, boxes_dev, **kw)
        if not (torch.equal(got, want) and torch.equal(got_off.cpu(), want_off) and int(status.sum()) == 0):
            raise SystemExit('track_bench: the device-box call and the host-box call differ (%s)' % (kw or 'bgr'))
    # (b)
    sd, tables = synth.make_state_dict(seed=10), synth.make_mano_tables(seed=1)
    loop = {}
    for batch in (1, n):
        eng = engine.Engine(0)
        eng.load_state_dict(sd, max_batch=batch)
        eng.load_mano(tables)
        pool = None
        if batch > 1:
            pool = engine.EnginePool(0, n=2)
            pool.load_state_dict(sd, max_batch=batch)
            pool.load_mano(tables)
        loop['batch_%d' % batch] = time_loops(loops(bgr[:batch], eng, pool, a.iters), a.warmup, a.runs)
        if pool is not None:
            pool.close()
        eng.close()
    if not all(v['boxes_equal'] for v in loop.values()):
        raise SystemExit('track_bench: the loops disagree on the boxes: %s' % json.dumps(loop))
    line = {'tool': 'track_bench', 'device': torch.cuda.get_device_name(0), 'repeats': a.repeats, 'iters': a.iters, 'runs': a.runs,
            'warmup': a.warmup, 'frames': n, 'frame_size': [H, W], 'region_size': [side, side], 'scale': SCALE, 'min_size': MIN_SIZE,
            'timing': {'call': 'HIP events around one call of n regions, median of `repeats`, per run',
                       'loop': 'wall clock per iteration of `iters` iterations ending in one synchronise, per run'},
            'call': call, 'loop': loop}
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
