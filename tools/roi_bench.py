"""Cost of region-of-interest pre-processing (csrc/preprocess.hip; DESIGN.md "Regions of interest") next to what a caller had
to do before it existed, on one GPU, one JSON line.

    python tools/roi_bench.py [--repeats 30] [--warmup 5] [--frames 64] [--size 480] [--timeout 600] [--out FILE]

64 regions of 480 x 480, one out of each of 64 frames of 1080 x 1920 (origins spread over the frame, odd ones included), HIP
events around one call as the caller sees it (list handling, ctypes, launches and kernels), median of `repeats`:
  rois_bgr          ops.preprocess_rois on the BGR frames
  crops_bgr         the composition without it: frame[t:b, l:r].contiguous() per region, then ops.preprocess_frames
  rois_nv12         ops.preprocess_rois on the same pictures as NV12 surfaces
  crops_nv12        the composition without it: ops.nv12_to_bgr of the whole surfaces, the crops, ops.preprocess_frames
and whether each pair gave the same bytes.  No ratio is asserted: the tool reports.  The run ends itself after `--timeout`
seconds."""
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


def smooth_nv12(n, H, W, seed):
    """n NV12 surfaces [n, H*3/2, W] of smooth pictures (a video frame is not noise; the kernels' time does not depend on
    the values)."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H * 3 // 2, 0:W].astype(np.float32)
    out = np.empty((n, H * 3 // 2, W), np.uint8)
    for i in range(n):
        a, b, c = g.uniform(0.002, 0.02, 3)
        out[i] = (127.5 + 127.5 * np.sin(a * xx + b * yy + 6.28 * c * i)).astype(np.uint8)
    return torch.from_numpy(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--size', type=int, default=480, help='side of the square regions')
    ap.add_argument('--timeout', type=int, default=600, help='seconds after which the run ends itself')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('roi_bench needs a GPU: there is no CPU path to time')
    signal.alarm(a.timeout)
    ops = importlib.import_module(PKG + '.ops')
    n, H, W, side = a.frames, 1080, 1920, a.size
    nv12 = list(smooth_nv12(n, H, W, seed=H).cuda().unbind(0))
    bgr = list(ops.nv12_to_bgr(nv12).unbind(0))       # the same pictures, packed
    g = np.random.default_rng(0)
    boxes = [(int(l), int(t), int(l) + side, int(t) + side)
             for l, t in zip(g.integers(0, W - side + 1, n), g.integers(0, H - side + 1, n))]
    torch.cuda.synchronize()

    def crops_of(frames):
        return [f[t:b, l:r].contiguous() for f, (l, t, r, b) in zip(frames, boxes)]

    res = {
        'rois_bgr': timed(lambda: ops.preprocess_rois(bgr, boxes), a.warmup, a.repeats),
        'crops_bgr': timed(lambda: ops.preprocess_frames(crops_of(bgr)), a.warmup, a.repeats),
        'rois_nv12': timed(lambda: ops.preprocess_rois(nv12, boxes, pixel_format='nv12'), a.warmup, a.repeats),
        'crops_nv12': timed(lambda: ops.preprocess_frames(crops_of(ops.nv12_to_bgr(nv12))), a.warmup, a.repeats),
    }
    for v in res.values():
        v['ms_per_region'] = round(v['median_ms'] / n, 5)
    want = ops.preprocess_frames(crops_of(bgr))[0]
    res['rois_bgr_equal_crops'] = bool(torch.equal(ops.preprocess_rois(bgr, boxes)[0], want))
    res['rois_nv12_equal_crops'] = bool(torch.equal(ops.preprocess_rois(nv12, boxes, pixel_format='nv12')[0], want))
    line = {'tool': 'roi_bench', 'device': torch.cuda.get_device_name(0), 'repeats': a.repeats, 'warmup': a.warmup, 'frames': n,
            'frame_size': [H, W], 'region_size': [side, side], 'odd_origins': sum(1 for l, t, _, _ in boxes if (l | t) & 1),
            'timing': 'HIP events around one call of n regions, median', 'results': res}
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
