"""Time of the mesh overlay (Engine.render) next to the forward step that feeds it, on one GPU, one JSON line.

    python tools/render_bench.py [--repeats 30] [--warmup 5] [--out FILE]

Two workloads: the 64 bench frames at 512 x 512 (bench.py's frames, drawn into the network input) and 32 frames of 1080p
(pre-processed on the GPU, drawn into the original frames).  Each is timed as bench.py times a step - HIP events around
the calls on one stream, a warm-up, the median over `repeats` - for `forward` alone and for `render` alone, in the same
process.  Rendering cost depends on how many hands there are and how large they are on screen, and the camera of a
synthetic checkpoint is as arbitrary as its weights (seed 0 puts the hands behind the camera: nothing to draw).  So every
workload is reported twice: "detected" = the network's own flags and cam_trans, whatever they show, and "placed" = every
slot drawn (two hands per frame, the most a frame can hold) at seeded translations that make each hand span 100-250
pixels of the 512 canvas, the size the kernels were designed against.  The synthetic MANO tables' faces are random index
triples, so every triangle of such a hand is as long as the hand: a stress case, not what a hand mesh costs.  "closed_mesh"
is therefore timed next to them - ops.render_meshes of two hand-sized closed meshes per frame with well-formed triangles
(the 738-vertex / 1472-face ellipsoids of tests/render_ref.py; MANO has 778 / 1538) at the same translations.  `floor_ms` = the image traffic (read + write of every pixel)
at the HBM peak of MI355X_MICROARCH (8 TB/s); `x_floor` = measured / floor."""
import argparse
import importlib
import json
import os
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


def workload(eng, L, name, net_in, offsets, canvas, bgr, warmup, repeats):
    ops = pkg('ops')
    B = net_in.shape[0]
    fwd = timed(lambda: eng.forward(net_in, offsets=offsets, project=True), warmup, repeats)
    out = eng.forward(net_in, offsets=offsets, project=True)
    out['cam_trans'] = ops.cam_trans(out['joints'].view(-1, 21, 3), out['pj2d'].view(-1, 21, 2), focal_length=1265.0).view(B, 2, 3)
    dst = torch.empty_like(canvas)
    floor = 2.0 * canvas.numel() / HBM_BYTES_PER_S * 1e3
    res = {'frames': B, 'height': int(canvas.shape[1]), 'width': int(canvas.shape[2]), 'forward': fwd,
           'floor_ms': round(floor, 4)}
    forced = dict(out, slots=out['slots'].clone())
    forced['slots'][:, :, L.SLOT_FLAG] = 1.0
    # a hand (~0.2 m) spans 1265 * 0.2 / Z pixels of the canvas: Z in [1.0, 2.5] m = 100-250 px; centres inside the canvas
    rng = np.random.default_rng(0)
    z = rng.uniform(1.0, 2.5, (B, 2, 1))
    xy = rng.uniform(-0.14, 0.14, (B, 2, 2)) * z
    forced['cam_trans'] = torch.from_numpy(np.concatenate([xy, z], -1).astype(np.float32)).cuda()
    verts = out['verts']
    span = (verts.amax(2) - verts.amin(2))[..., :2].amax(-1)      # metres, per hand
    res['placed_hand_span_px'] = [round(float(v), 1) for v in (1265.0 * span / forced['cam_trans'][..., 2]).quantile(
        torch.tensor([0.0, 0.5, 1.0], device=span.device))]
    for label, o in (('detected', out), ('placed', forced)):
        r = timed(lambda: eng.render(o, canvas, offsets=offsets, bgr=bgr, dst=dst), warmup, repeats)
        _, ids = eng.render(o, canvas, offsets=offsets, bgr=bgr, dst=dst, return_ids=True)
        r['hands'] = int((o['slots'][:, :, L.SLOT_FLAG] > 0.5).sum())
        r['covered_px_per_frame'] = int((ids >= 0).sum()) // B
        r['share_of_forward'] = round(r['median_ms'] / fwd['median_ms'], 4)
        r['x_floor'] = round(r['median_ms'] / floor, 2)
        res[label] = r
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import render_ref
    ev, ef = render_ref.ellipsoid(24, 32, (0.05, 0.09, 0.03), (0.0, 0.0, 0.0))
    topo = torch.from_numpy(ops.mesh_topology(ef, len(ev))).cuda()
    everts = torch.from_numpy(ev).cuda()[None].repeat(2 * B, 1, 1)
    kw = dict(mesh_frame=torch.arange(2 * B, dtype=torch.int32).cuda() // 2, trans=forced['cam_trans'].view(-1, 3),
              view=None if offsets is None else ops.view_from_offsets(offsets).cuda(), out=dst)
    r = timed(lambda: ops.render_meshes(everts, topo, canvas, **kw), warmup, repeats)
    r['covered_px_per_frame'] = int((ops.render_meshes(everts, topo, canvas, return_ids=True, **kw)[1] >= 0).sum()) // B
    r['share_of_forward'] = round(r['median_ms'] / fwd['median_ms'], 4)
    r['x_floor'] = round(r['median_ms'] / floor, 2)
    res['closed_mesh'] = r
    in_place = canvas.clone()
    res['placed_in_place'] = timed(lambda: eng.render(forced, in_place, offsets=offsets, bgr=bgr, dst=in_place), warmup, repeats)
    return name, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    ap.add_argument('--only', choices=('512', '1080p'), default=None, help='one workload (profiling runs)')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('render_bench needs a GPU: there is no CPU path to time')
    synth, L, ops = pkg('synth'), pkg('_lib'), pkg('ops')
    eng = pkg('engine').Engine(0)
    eng.load_state_dict(synth.make_state_dict(seed=0), max_batch=64)
    tables = synth.make_mano_tables(seed=1)
    tables['left']['shapedirs'] = tables['left']['shapedirs'].copy()
    tables['left']['shapedirs'][:, 0, :] *= -1
    eng.load_mano(tables)
    line = {'tool': 'render_bench', 'device': torch.cuda.get_device_name(0), 'repeats': a.repeats, 'warmup': a.warmup,
            'timing': 'HIP events, median', 'note': 'synthetic MANO faces are random index triples: more and longer '
            'triangles per pixel than a real hand mesh'}
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
