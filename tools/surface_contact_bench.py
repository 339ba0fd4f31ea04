"""Time of the surface contact measure between the hands of a row (Engine.contact(mode='surface')) next
to two figures from the same process, on one GPU, one JSON line.

    python tools/surface_contact_bench.py [--repeats 30] [--warmup 5] [--timeout 600] [--out FILE]

The 64 bench frames (512 x 512) go through Engine.forward once per K = max_hand in (1, 2, 4); every slot is then flagged and
the hands of a row are placed a few centimetres from each other 0.8 m in front of the camera, so that all K * K pairs of every
row are computed: the most work there can be (the geometry of tools/contact_bench.py).  Timed in one process with HIP events
around the calls on one stream - a warm-up, then the median over `repeats`:
  surface   Engine.contact(mode='surface') on those outputs (cam_trans handed in): prep + setup + pair + reduce kernels
  vertex    Engine.contact in its default mode on the same outputs
  forward   Engine.forward(project=True[, max_hand=K]) of those frames: the step that feeds both
Neither the default mode nor the forward path is touched by the surface measure, so those two are also the figures of the
commit before it, taken in the same process.  The run ends itself after `--timeout` seconds."""
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


def pkg(sub):
    return importlib.import_module(PKG + '.' + sub)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--timeout', type=int, default=600, help='seconds after which the run ends itself')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('surface_contact_bench needs a GPU: there is no CPU path to time')
    signal.alarm(a.timeout)
    synth, L, ops = pkg('synth'), pkg('_lib'), pkg('ops')
    eng = pkg('engine').Engine(0)
    eng.load_state_dict(synth.make_state_dict(seed=0), max_batch=64)
    tables = synth.make_mano_tables(seed=1)
    tables['left']['shapedirs'] = tables['left']['shapedirs'].copy()
    tables['left']['shapedirs'][:, 0, :] *= -1
    eng.load_mano(tables)
    B = 64
    frames = torch.from_numpy(synth.make_frames(B, seed=0, structured=False)).cuda()
    line = {'tool': 'surface_contact_bench', 'device': torch.cuda.get_device_name(0), 'repeats': a.repeats, 'warmup': a.warmup,
            'timing': 'HIP events, median', 'frames': B, 'contact_dist': ops.CONTACT_DIST, 'max_depth': ops.CONTACT_MAX_DEPTH,
            'faces': int(np.asarray(tables['left']['faces']).reshape(-1, 3).shape[0])}
    rng = np.random.default_rng(0)
    for K in (1, 2, 4):
        kw = dict(project=True) if K == 1 else dict(project=True, max_hand=K)
        fwd = timed(lambda: eng.forward(frames, **kw), a.warmup, a.repeats)
        out = eng.forward(frames, **kw)
        lead = (B, K, 2)
        out = {k: v.view(lead + tuple(v.shape[len(v.shape) - (1 if k == 'slots' else 2):])) for k, v in out.items()}
        out['slots'][..., L.SLOT_FLAG] = 1.0
        ct = torch.from_numpy((np.array((0, 0, 0.8)) + rng.uniform(-0.03, 0.03, lead + (3,))).astype(np.float32)).cuda()
        sur = timed(lambda: eng.contact(out, max_hand=K, cam_trans=ct, mode='surface'), a.warmup, a.repeats)
        ver = timed(lambda: eng.contact(out, max_hand=K, cam_trans=ct), a.warmup, a.repeats)
        res = eng.contact(out, max_hand=K, cam_trans=ct, mode='surface')
        old = eng.contact(out, max_hand=K, cam_trans=ct)
        # how far the nearest-vertex distance lies above the surface distance, direction 0, in millimetres
        over = (old['d2'][:, 0].sqrt() - res['d2'][:, 0].sqrt()) * 1000
        line['max_hand_%d' % K] = {
            'pairs': B * K * K, 'surface': sur, 'vertex': ver, 'forward': fwd,
            'surface_over_vertex': round(sur['median_ms'] / ver['median_ms'], 2),
            'share_of_forward': round(sur['median_ms'] / fwd['median_ms'], 4),
            'vertex_tests_per_second': round(B * K * K * 2 * 778 * line['faces'] / (sur['median_ms'] * 1e-3), -6),
            'contact_verts_per_pair': round(float(res['n_contact'].float().sum(1).mean()), 1),
            'inside_verts_per_pair': round(float(res['n_inside'].float().sum(1).mean()), 1),
            'vertex_minus_surface_mm_mean': round(float(over.mean()), 3), 'vertex_minus_surface_mm_max': round(float(over.max()), 3)}
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    eng.close()


if __name__ == '__main__':
    main()
