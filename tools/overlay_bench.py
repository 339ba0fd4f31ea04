"""Time of the key-point skeleton and centre heat-map views (Engine.overlay) next to the forward step that feeds them and
the mesh view (Engine.render), on one GPU, one JSON line.

    python tools/overlay_bench.py [--repeats 30] [--warmup 5] [--timeout 600] [--out FILE] [--only 512|1080p]

Two workloads, as tools/render_bench.py: the 64 bench frames at 512 x 512 (drawn into the network input) and 32 frames of
1080p (pre-processed on the GPU, drawn into the original frames).  Everything is timed in one process with HIP events around
the calls on one stream: a warm-up, then the median over `repeats`.  The cost of the skeleton view depends on where the
hands are, and the camera of a synthetic checkpoint is as arbitrary as its weights, so it is reported twice: "detected" =
the network's own flags and key points, whatever they show, and "placed" = every slot drawn (two hands per frame) with
seeded hand-shaped key points that span 100-250 pixels of the 512 canvas.  `floor_ms` = the image traffic at the HBM peak of
8 TB/s: 1 read + 1 write for the skeleton (out of place), 1 read + 2 writes for the heat maps; `x_floor` = measured / floor.
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
HBM_BYTES_PER_S = 8.0e12


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


def hand_keypoints(n, span_px, centre_px, rng):
    """n hand-shaped key-point sets [n,21,2] in MANO order: wrist + five chains of four joints, `span_px` long."""
    kps = np.zeros((n, 21, 2), np.float32)
    for m in range(n):
        a0 = rng.uniform(0, 2 * np.pi)
        kps[m, 0] = centre_px[m]
        for f in range(5):
            ang, p = a0 + (f - 2) * 0.35, centre_px[m].astype(np.float64)
            for j in range(4):
                ang += rng.normal(0, 0.2)
                p = p + span_px[m] * (0.45 if j == 0 else 0.18) * np.array([np.cos(ang), np.sin(ang)])
                kps[m, 1 + 4 * f + j] = p
    return kps


def workload(eng, L, name, net_in, offsets, canvas, bgr, warmup, repeats):
    ops = pkg('ops')
    B, H, W = canvas.shape[:3]
    fwd = timed(lambda: eng.forward(net_in, offsets=offsets, project=True), warmup, repeats)
    out = eng.forward(net_in, offsets=offsets, project=True)
    out['cam_trans'] = ops.cam_trans(out['joints'].view(-1, 21, 3), out['pj2d'].view(-1, 21, 2), focal_length=1265.0).view(B, 2, 3)
    px = canvas.numel()
    res = {'frames': B, 'height': H, 'width': W, 'forward': fwd,
           'floor_ms': {'pj2d': round(2.0 * px / HBM_BYTES_PER_S * 1e3, 4), 'centermap': round(3.0 * px / HBM_BYTES_PER_S * 1e3, 4)}}
    # every slot drawn, hands of 100-250 canvas pixels with their wrists inside the canvas
    rng = np.random.default_rng(0)
    span = rng.uniform(100, 250, 2 * B)
    centre = rng.uniform(0.2, 0.8, (2 * B, 2)) * 512
    k512 = hand_keypoints(2 * B, span, centre, rng)
    placed = dict(out, slots=out['slots'].clone())
    placed['slots'][:, :, L.SLOT_FLAG] = 1.0
    placed['pj2d'] = torch.from_numpy(k512 / 256.0 - 1.0).float().cuda().view(B, 2, 21, 2)
    if offsets is not None:
        v = ops.view_from_offsets(offsets).cpu().numpy().repeat(2, 0)      # x_org = x_512 * sx + ox
        placed['pj2d_org'] = torch.from_numpy(k512 * v[:, None, :2] + v[:, None, 2:]).float().cuda().view(B, 2, 21, 2)
    dst = torch.empty_like(canvas)
    for label, o in (('detected', out), ('placed', placed)):
        r = timed(lambda: eng.overlay(o, canvas, 'pj2d', offsets=offsets, bgr=bgr, dst=dst), warmup, repeats)
        got = eng.overlay(o, canvas, 'pj2d', offsets=offsets, bgr=bgr)
        r['hands'] = int((o['slots'][:, :, L.SLOT_FLAG] > 0.5).sum())
        r['drawn_px_per_frame'] = int((got != canvas).any(-1).sum()) // B
        r['share_of_forward'] = round(r['median_ms'] / fwd['median_ms'], 4)
        r['x_floor'] = round(r['median_ms'] / res['floor_ms']['pj2d'], 2)
        res['pj2d_' + label] = r
    work = canvas.clone()
    res['pj2d_placed_in_place'] = timed(lambda: eng.overlay(placed, work, 'pj2d', offsets=offsets, bgr=bgr, dst=work), warmup, repeats)
    eng.forward(net_in, offsets=offsets, project=True)      # (the resident maps: those of this batch)
    dst2 = torch.empty((2,) + tuple(canvas.shape), dtype=torch.uint8, device=canvas.device)
    r = timed(lambda: eng.overlay(out, canvas, 'centermap', offsets=offsets, bgr=bgr, dst=dst2), warmup, repeats)
    r['share_of_forward'] = round(r['median_ms'] / fwd['median_ms'], 4)
    r['x_floor'] = round(r['median_ms'] / res['floor_ms']['centermap'], 2)
    res['centermap'] = r
    forced = dict(placed)
    z = rng.uniform(1.0, 2.5, (B, 2, 1))
    forced['cam_trans'] = torch.from_numpy(np.concatenate([rng.uniform(-0.14, 0.14, (B, 2, 2)) * z, z], -1).astype(np.float32)).cuda()
    for label, o in (('detected', out), ('placed', forced)):
        r = timed(lambda: eng.render(o, canvas, offsets=offsets, bgr=bgr, dst=dst), warmup, repeats)
        r['share_of_forward'] = round(r['median_ms'] / fwd['median_ms'], 4)
        res['render_' + label] = r
    return name, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--timeout', type=int, default=600, help='seconds after which the run ends itself')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    ap.add_argument('--only', choices=('512', '1080p'), default=None, help='one workload (profiling runs)')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('overlay_bench needs a GPU: there is no CPU path to time')
    signal.alarm(a.timeout)
    synth, L, ops = pkg('synth'), pkg('_lib'), pkg('ops')
    eng = pkg('engine').Engine(0)
    eng.load_state_dict(synth.make_state_dict(seed=0), max_batch=64)
    tables = synth.make_mano_tables(seed=1)
    tables['left']['shapedirs'] = tables['left']['shapedirs'].copy()
    tables['left']['shapedirs'][:, 0, :] *= -1
    eng.load_mano(tables)
    line = {'tool': 'overlay_bench', 'device': torch.cuda.get_device_name(0), 'repeats': a.repeats, 'warmup': a.warmup,
            'timing': 'HIP events, median'}
    if a.only in (None, '512'):
        frames = torch.from_numpy(synth.make_frames(64, seed=0, structured=False)).cuda()
        k, v = workload(eng, L, 'bench64_512', frames, None, frames, False, a.warmup, a.repeats)
        line[k] = v
    if a.only in (None, '1080p'):
        small = synth.make_frames(32, seed=0, structured=False)
        raw = torch.from_numpy(np.ascontiguousarray(np.kron(small, np.ones((1, 4, 4, 1), np.uint8))[:, 484:1564, 64:1984, ::-1])).cuda()
        net_in, offsets = ops.preprocess(raw)
        k, v = workload(eng, L, 'video32_1080p', net_in, offsets, raw, True, a.warmup, a.repeats)
        line[k] = v
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    eng.close()


if __name__ == '__main__':
    main()
