"""Time of the part segmentation as an output (Engine.segment: label maps, the 'segm' view, the mask statistics; DESIGN.md
section 23) next to the forward step that feeds it and the centre heat-map view (Engine.overlay), on one GPU, one JSON line.

    python tools/segm_bench.py [--repeats 30] [--warmup 5] [--timeout 600] [--out FILE] [--only 512|1080p]

Two workloads, as tools/overlay_bench.py: the 64 bench frames at 512 x 512 (the network input) and 32 frames of 1080p
(pre-processed on the GPU, labelled and drawn at their own resolution under their offsets rows).  Everything is timed in one
process with HIP events around the calls on one stream: a warm-up, then the median over `repeats`.  Timed: labels + view in one
call, labels alone, the view alone in place, and the statistics with the rasteriser's ids; beside each the same quantities
written in torch ops (interpolate + argmax + table look-up + blend; bincount and reductions of the masks - the 1080p frames with
the view folded into `size=` and a crop, which is not the same rule at the pad's edge and is only timed).  `floor_ms` = the
traffic at the HBM peak of 8 TB/s: the logits read once at 144 bytes per cell (a tile reads a border cell again; not counted),
plus the image read and written, plus the labels; `x_floor` = measured / floor.  The run ends itself after `--timeout`
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


def torch_labels(logits_nchw, H, W, pad):
    """interpolate + argmax; pad = (side, top, left): the frame is the window [top, top + H) x [left, left + W) of a square."""
    if pad is None:
        return torch.nn.functional.interpolate(logits_nchw, size=(H, W), mode='bilinear', align_corners=False).argmax(1)
    side, top, left = pad
    out = []
    for f in logits_nchw.split(4):      # (a square of 1920^2 x 33 floats per frame: a few frames at a time)
        full = torch.nn.functional.interpolate(f, size=(side, side), mode='bilinear', align_corners=False)
        out.append(full[:, :, top:top + H, left:left + W].argmax(1))
    return torch.cat(out)


def torch_view(lab, images, table, weight=0.7):
    col = table[lab]      # [B,H,W,3] float
    hand = (lab > 0)[..., None]
    mixed = torch.floor(weight * col + (1 - weight) * images.float()).to(torch.uint8)
    return torch.where(hand, mixed, images)


def torch_stats(lab, ids, n_faces):
    B, H, W = lab.shape
    flat = lab.reshape(B, -1).long()
    counts = torch.zeros(B, 256, dtype=torch.long, device=lab.device).scatter_add_(1, flat, torch.ones_like(flat))[:, :33]
    ys = torch.arange(H, device=lab.device)[None, :, None].expand(B, H, W)
    xs = torch.arange(W, device=lab.device)[None, None, :].expand(B, H, W)
    res = [counts]
    mesh = torch.div(ids, n_faces, rounding_mode='floor')
    for s, (lo, hi) in enumerate(((17, 32), (1, 16))):
        m = (lab >= lo) & (lab <= hi)
        big = torch.where(m, xs, torch.full_like(xs, W)).amin((1, 2)), torch.where(m, ys, torch.full_like(ys, H)).amin((1, 2))
        small = torch.where(m, xs, torch.full_like(xs, -1)).amax((1, 2)), torch.where(m, ys, torch.full_like(ys, -1)).amax((1, 2))
        sil = (ids >= 0) & ((mesh & 1) == s)
        res += [*big, *small, (m & sil).sum((1, 2)), m.sum((1, 2)), sil.sum((1, 2))]
    return res


def workload(eng, name, net_in, offsets, canvas, bgr, pad, warmup, repeats):
    ops = pkg('ops')
    B, H, W = canvas.shape[:3]
    fwd = timed(lambda: eng.forward(net_in, offsets=offsets, project=True), warmup, repeats)
    out = eng.forward(net_in, offsets=offsets, project=True)
    ids = eng.render(out, canvas, offsets=offsets, bgr=bgr, return_ids=True)[1]
    n_faces = eng._faces['left'].shape[0]
    px = B * H * W
    logits_bytes = B * 256 * 256 * 144
    floor = {'labels_view': (logits_bytes + 7 * px) / HBM_BYTES_PER_S * 1e3, 'labels': (logits_bytes + px) / HBM_BYTES_PER_S * 1e3,
             'view_in_place': (logits_bytes + 6 * px) / HBM_BYTES_PER_S * 1e3, 'stats_ids': 5 * px / HBM_BYTES_PER_S * 1e3}
    res = {'frames': B, 'height': H, 'width': W, 'forward': fwd, 'floor_ms': {k: round(v, 4) for k, v in floor.items()}}

    def row(key, r, floor_key):
        r['share_of_forward'] = round(r['median_ms'] / fwd['median_ms'], 4)
        r['x_floor'] = round(r['median_ms'] / floor[floor_key], 2)
        res[key] = r

    dst = torch.empty_like(canvas)
    row('labels_view', timed(lambda: eng.segment(B, images=canvas, offsets=offsets, bgr=bgr, dst=dst), warmup, repeats), 'labels_view')
    row('labels', timed(lambda: eng.segment(B, images=canvas, offsets=offsets, draw=False), warmup, repeats), 'labels')
    work = canvas.clone()
    row('view_in_place', timed(lambda: eng.segment(B, images=work, offsets=offsets, bgr=bgr, dst=work, labels=False), warmup, repeats),
        'view_in_place')
    seg = eng.segment(B, images=canvas, offsets=offsets, bgr=bgr)
    lab = seg['labels']
    row('stats_ids', timed(lambda: ops.segm_stats(lab, 33, ids=ids, n_faces=n_faces), warmup, repeats), 'stats_ids')
    res['stats_plain'] = timed(lambda: ops.segm_stats(lab, 33), warmup, repeats)
    st = ops.segm_stats(lab, 33, ids=ids, n_faces=n_faces)
    res['hand_px_per_frame'] = int(st['counts'][:, 1:].sum()) // B
    res['drawn_px_per_frame'] = int((seg['view'] != canvas).any(-1).sum()) // B
    res['agree_total'] = st['agree'].sum(0).cpu().numpy().tolist()
    dst2 = torch.empty((2,) + tuple(canvas.shape), dtype=torch.uint8, device=canvas.device)
    r = timed(lambda: eng.overlay(out, canvas, 'centermap', offsets=offsets, bgr=bgr, dst=dst2), warmup, repeats)
    r['share_of_forward'] = round(r['median_ms'] / fwd['median_ms'], 4)
    res['centermap'] = r
    # the same quantities in torch ops, on an NCHW copy of the logits made outside the timed window
    logits = eng.head_maps(B)['segms']
    table = torch.from_numpy(ops.segm_colors(33, bgr).astype(np.float32)).cuda()
    t_lab = torch_labels(logits, H, W, pad)
    if pad is None:
        res['torch_labels_differ'] = int((t_lab != lab).sum())
    res['torch_labels'] = timed(lambda: torch_labels(logits, H, W, pad), 2, 5)
    res['torch_view'] = timed(lambda: torch_view(t_lab, canvas, table), 2, 5)
    res['torch_stats_ids'] = timed(lambda: torch_stats(lab, ids, n_faces), 2, 5)
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
        raise SystemExit('segm_bench needs a GPU: there is no CPU path to time')
    signal.alarm(a.timeout)
    synth, ops = pkg('synth'), pkg('ops')
    eng = pkg('engine').Engine(0)
    eng.load_state_dict(synth.make_state_dict(seed=0), max_batch=64)
    tables = synth.make_mano_tables(seed=1)
    tables['left']['shapedirs'] = tables['left']['shapedirs'].copy()
    tables['left']['shapedirs'][:, 0, :] *= -1
    eng.load_mano(tables)
    line = {'tool': 'segm_bench', 'device': torch.cuda.get_device_name(0), 'repeats': a.repeats, 'warmup': a.warmup,
            'timing': 'HIP events, median', 'tile_px': [64, 16]}      # SEGM_TW x SEGM_TH of csrc/segm_plan.h
    if a.only in (None, '512'):
        frames = torch.from_numpy(synth.make_frames(64, seed=0, structured=False)).cuda()
        k, v = workload(eng, 'bench64_512', frames, None, frames, False, None, a.warmup, a.repeats)
        line[k] = v
    if a.only in (None, '1080p'):
        small = synth.make_frames(32, seed=0, structured=False)
        raw = torch.from_numpy(np.ascontiguousarray(np.kron(small, np.ones((1, 4, 4, 1), np.uint8))[:, 484:1564, 64:1984, ::-1])).cuda()
        net_in, offsets = ops.preprocess(raw)
        k, v = workload(eng, 'video32_1080p', net_in, offsets, raw, True, (1920, 420, 0), a.warmup, a.repeats)
        line[k] = v
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    eng.close()


if __name__ == '__main__':
    main()
