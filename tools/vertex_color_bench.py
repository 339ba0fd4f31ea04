"""Time of the per-vertex colour views next to the flat overlay and the forward step, on one GPU, one
JSON line.

    python tools/vertex_color_bench.py [--repeats 30] [--warmup 5] [--runs 3] [--out FILE]

The two workloads of tools/render_bench.py - 64 frames of 512 x 512 drawn into the network input, 32 frames of 1080p drawn into
the original frames - with its seeded translations ("placed": two hands per frame, each spanning 100-250 pixels of the 512
canvas) and, for the same reason as there, CLOSED meshes with well-formed triangles in place of the synthetic MANO tables'
random index triples: a 778-vertex / 1552-face lat-long ellipsoid (tests/render_ref.py) loaded as both sides' faces, its
vertices in place of the network's.  Timed as bench.py times a step - HIP events around the calls on one stream, a warm-up, the
median over `repeats` - `runs` times in one process:
  render_flat / render_colored   Engine.render without and with vertex_colors, ALTERNATED call by call
  contact_colors                 Engine.contact_colors alone (acrmi_contact_values + acrmi_vertex_colors)
  contact_view_k1 / _k2          the contact view end to end behind a forward: contact + contact_colors + the coloured render,
                                 at max_hand 1 (Engine.render) and 2 (Engine.render_regions, hands of rank 1 copied from rank 0)
  forward                        Engine.forward of the same frames (max_hand 1)
`colored_over_flat` = the coloured median over the flat one.  The 20 mm of the colour scale are parameters, not measurements."""
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))
PKG = 'arbitrary-hands-3d-reconstruction_amd'


def pkg(sub):
    return importlib.import_module(PKG + '.' + sub)


def _time_once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _stats(ms):
    return {'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4)}


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return _stats([_time_once(fn) for _ in range(repeats)])


def timed_alternated(fa, fb, warmup, repeats):
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(repeats):
        a.append(_time_once(fa))
        b.append(_time_once(fb))
    return _stats(a), _stats(b)


def workload(eng, L, closed, net_in, offsets, canvas, bgr, warmup, repeats):
    B = net_in.shape[0]
    res = {'frames': B, 'height': int(canvas.shape[1]), 'width': int(canvas.shape[2])}
    res['forward'] = timed(lambda: eng.forward(net_in, offsets=offsets, project=True), warmup, repeats)
    out = eng.forward(net_in, offsets=offsets, project=True)
    out = dict(out, slots=out['slots'].clone(), verts=closed[None, None].repeat(B, 2, 1, 1).contiguous())
    out['slots'][:, :, L.SLOT_FLAG] = 1.0
    rng = np.random.default_rng(0)      # the translations of tools/render_bench.py
    z = rng.uniform(1.0, 2.5, (B, 2, 1))
    xy = rng.uniform(-0.14, 0.14, (B, 2, 2)) * z
    ct = np.concatenate([xy, z], -1).astype(np.float32)
    ct[:, 1] = ct[:, 0] + np.float32([0.06, 0.01, 0.02])      # the right hand next to the left one: there is contact to show
    out['cam_trans'] = torch.from_numpy(ct).cuda()
    dst = torch.empty_like(canvas)
    con = eng.contact(out)
    vcol = eng.contact_colors(con, out, bgr=bgr)
    flat, col = timed_alternated(lambda: eng.render(out, canvas, offsets=offsets, bgr=bgr, dst=dst),
                                 lambda: eng.render(out, canvas, offsets=offsets, bgr=bgr, dst=dst, vertex_colors=vcol), warmup, repeats)
    _, ids = eng.render(out, canvas, offsets=offsets, bgr=bgr, dst=dst, vertex_colors=vcol, return_ids=True)
    res['covered_px_per_frame'] = int((ids >= 0).sum()) // B
    res['render_flat'], res['render_colored'] = flat, col
    res['colored_over_flat'] = round(col['median_ms'] / flat['median_ms'], 4)
    res['contact_colors'] = timed(lambda: eng.contact_colors(con, out, bgr=bgr), warmup, repeats)

    def view_k1():
        c = eng.contact(out)
        eng.render(out, canvas, offsets=offsets, bgr=bgr, dst=dst, vertex_colors=eng.contact_colors(c, out, bgr=bgr))

    res['contact_view_k1'] = timed(view_k1, warmup, repeats)
    # max_hand 2: rank 1 a copy of rank 0 shifted by 3 cm; drawn as 2 B regions with the frames' own offsets rows
    two = {k: torch.stack([out[k], out[k]], 1).contiguous() for k in ('slots', 'verts', 'cam_trans')}
    two['cam_trans'][:, 1, :, 0] += 0.03
    rows = (torch.tensor([[512., 512, 0, 0, 0, 0, 0, 0, 0, 0]]).repeat(B, 1) if offsets is None else offsets.cpu()).repeat_interleave(2, 0).cuda()
    region_frame = torch.arange(B, dtype=torch.int32).repeat_interleave(2).cuda()
    flat2 = {k: v.flatten(0, 1) for k, v in two.items()}

    def view_k2():
        c = eng.contact(two, max_hand=2)
        v = eng.contact_colors(c, two, max_hand=2, bgr=bgr)
        eng.render_regions(flat2, canvas, rows, region_frame, bgr=bgr, dst=dst, vertex_colors=v.flatten(0, 1))

    res['contact_view_k2'] = timed(view_k2, warmup, repeats)
    for k in ('contact_view_k1', 'contact_view_k2'):
        res[k]['share_of_forward'] = round(res[k]['median_ms'] / res['forward']['median_ms'], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('vertex_color_bench needs a GPU: there is no CPU path to time')
    import render_ref
    synth, L, ops = pkg('synth'), pkg('_lib'), pkg('ops')
    eng = pkg('engine').Engine(0)
    eng.load_state_dict(synth.make_state_dict(seed=0), max_batch=64)
    ev, ef = render_ref.ellipsoid(9, 97, (0.05, 0.09, 0.03), (0.0, 0.0, 0.0))
    assert ev.shape == (778, 3)
    tables = synth.make_mano_tables(seed=1)
    for side in ('left', 'right'):      # (both sides at once: the two face tables must have one face count)
        tables[side] = dict(tables[side], faces=ef)
    eng.load_mano(tables)
    eng.set_contact_sign(1, 1)      # (the ellipsoid is wound outwards; the derived sign is that of the faces on MANO's template)
    closed = torch.from_numpy(ev).cuda()
    frames = torch.from_numpy(synth.make_frames(64, seed=0, structured=False)).cuda()
    small = synth.make_frames(32, seed=0, structured=False)
    raw = torch.from_numpy(np.ascontiguousarray(np.kron(small, np.ones((1, 4, 4, 1), np.uint8))[:, 484:1564, 64:1984, ::-1])).cuda()
    net_in, offsets = ops.preprocess(raw)
    line = {'tool': 'vertex_color_bench', 'device': torch.cuda.get_device_name(0), 'repeats': a.repeats, 'warmup': a.warmup,
            'timing': 'HIP events, median', 'mesh': 'closed lat-long ellipsoid, 778 vertices, %d faces' % len(ef), 'runs': []}
    for _ in range(a.runs):
        line['runs'].append({'bench64_512': workload(eng, L, closed, frames, None, frames, False, a.warmup, a.repeats),
                             'video32_1080p': workload(eng, L, closed, net_in, offsets, raw, True, a.warmup, a.repeats)})
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    eng.close()


if __name__ == '__main__':
    main()
