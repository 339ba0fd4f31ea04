"""Time of the two contact measures between the hands of a row (Engine.contact; DESIGN.md sections 19 and 20) next to
comparisons from the same process, on one GPU, one JSON line per mode.

    python tools/contact_bench.py [--mode vertex|surface|both] [--repeats 30] [--warmup 5] [--timeout 600] [--out FILE]

The 64 bench frames (512 x 512) go through Engine.forward once per K = max_hand in (1, 2, 4); every slot is then flagged and
the hands of a row are placed a few centimetres from each other 0.8 m in front of the camera, so that all K * K pairs of every
row are computed: the most work there can be.  Timed in one process with HIP events around the calls on one stream - a
warm-up, then the median over `repeats`.  --mode vertex (the default; the line's tool is 'contact_bench'):
  contact   Engine.contact on those outputs (cam_trans handed in): prep + setup + pair + reduce kernels
  torch     the same quantities written in torch ops on the same tensors: vertex normals by index_add over the faces, the
            [pairs,778,778] squared distances, arg-min, side value, counts and maxima, both directions - what a caller would
            write without the kernels, and without the host visit it would end in
  forward   Engine.forward(project=True[, max_hand=K]) of those frames: the step that feeds it
The torch form is a yardstick for the cost, not for the bits: its summation order is torch's.  --mode surface (the line's tool
is 'surface_contact_bench'):
  surface   Engine.contact(mode='surface') on those outputs
  vertex    Engine.contact in its default mode on the same outputs
  forward   as above
--mode both prints the vertex line, then the surface line; --out then holds both.  The run ends itself after `--timeout`
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


def torch_normals(v, faces, sign):
    """v [n,778,3], faces [F,3] long on the device -> the signed un-normalised vertex normals [n,778,3]."""
    p0, p1, p2 = (v[:, faces[:, k]] for k in range(3))
    fn = torch.cross(p1 - p0, p2 - p0, dim=-1)
    n = torch.zeros_like(v)
    for k in range(3):
        n.index_add_(1, faces[:, k], fn)
    return n * sign


def torch_direction(Pa, Pb, Nb):
    d = [Pa[:, :, None, c] - Pb[:, None, :, c] for c in range(3)]
    d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    best, nn = d2.min(2)
    q = torch.gather(Pb, 1, nn[..., None].expand(-1, -1, 3))
    nb = torch.gather(Nb, 1, nn[..., None].expand(-1, -1, 3))
    e = Pa - q
    return nn, best, (e * nb).sum(-1)


def torch_contact(verts, trans, faces, signs, K, r, m):
    """verts [B,K,2,778,3], trans [B,K,2,3] -> the quantities of Engine.contact for the B*K*K pairs, every pair computed."""
    B = verts.shape[0]
    P = verts + trans[..., None, :]
    N = [torch_normals(verts[:, :, h].reshape(B * K, 778, 3), faces[h], signs[h]).view(B, K, 778, 3) for h in (0, 1)]
    i = torch.arange(K, device=verts.device).repeat_interleave(K)
    j = torch.arange(K, device=verts.device).repeat(K)
    Pl, Pr = P[:, i, 0].reshape(-1, 778, 3), P[:, j, 1].reshape(-1, 778, 3)
    Nl, Nr = N[0][:, i].reshape(-1, 778, 3), N[1][:, j].reshape(-1, 778, 3)
    out = []
    for Pa, Pb, Nb in ((Pl, Pr, Nr), (Pr, Pl, Nl)):
        nn, d2, s = torch_direction(Pa, Pb, Nb)
        inside = (s < 0) & (d2 <= m * m)
        out.append((nn, d2, s, (d2 <= r * r).sum(1), inside.sum(1), torch.where(inside, d2, torch.zeros_like(d2)).amax(1)))
    best, bi = out[0][1].min(1)
    return out, best, bi, torch.gather(out[0][0], 1, bi[:, None])


def vertex_figures(eng, out, K, ct, fwd, a, faces, r, m):
    con = timed(lambda: eng.contact(out, max_hand=K, cam_trans=ct), a.warmup, a.repeats)
    res = eng.contact(out, max_hand=K, cam_trans=ct)
    signs = eng.contact_sign
    tor = timed(lambda: torch_contact(out['verts'], ct, faces, signs, K, r, m), a.warmup, a.repeats)
    ref, best, bi, bj = torch_contact(out['verts'], ct, faces, signs, K, r, m)
    # the two forms describe the same thing (the torch one rounds in its own order: nn may differ on near ties)
    agree = float((ref[0][0] == res['nn'][:, 0]).float().mean())
    return {'pairs': res['nn'].shape[0], 'contact': con, 'torch': tor, 'forward': fwd,
            'torch_over_contact': round(tor['median_ms'] / con['median_ms'], 2),
            'share_of_forward': round(con['median_ms'] / fwd['median_ms'], 4),
            'nn_agreement_with_torch': round(agree, 6),
            'contact_verts_per_pair': round(float(res['n_contact'].float().sum(1).mean()), 1),
            'inside_verts_per_pair': round(float(res['n_inside'].float().sum(1).mean()), 1)}


def surface_figures(eng, out, K, ct, fwd, a, n_faces):
    sur = timed(lambda: eng.contact(out, max_hand=K, cam_trans=ct, mode='surface'), a.warmup, a.repeats)
    ver = timed(lambda: eng.contact(out, max_hand=K, cam_trans=ct), a.warmup, a.repeats)
    res = eng.contact(out, max_hand=K, cam_trans=ct, mode='surface')
    old = eng.contact(out, max_hand=K, cam_trans=ct)
    # how far the nearest-vertex distance lies above the surface distance, direction 0, in millimetres
    over = (old['d2'][:, 0].sqrt() - res['d2'][:, 0].sqrt()) * 1000
    pairs = res['face'].shape[0]
    return {'pairs': pairs, 'surface': sur, 'vertex': ver, 'forward': fwd,
            'surface_over_vertex': round(sur['median_ms'] / ver['median_ms'], 2),
            'share_of_forward': round(sur['median_ms'] / fwd['median_ms'], 4),
            'vertex_tests_per_second': round(pairs * 2 * 778 * n_faces / (sur['median_ms'] * 1e-3), -6),
            'contact_verts_per_pair': round(float(res['n_contact'].float().sum(1).mean()), 1),
            'inside_verts_per_pair': round(float(res['n_inside'].float().sum(1).mean()), 1),
            'vertex_minus_surface_mm_mean': round(float(over.mean()), 3), 'vertex_minus_surface_mm_max': round(float(over.max()), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=('vertex', 'surface', 'both'), default='vertex')
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--timeout', type=int, default=600, help='seconds after which the run ends itself')
    ap.add_argument('--out', default=None, help='also write the JSON line(s) to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('contact_bench needs a GPU: there is no CPU path to time')
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
    faces = [torch.from_numpy(np.asarray(tables[s]['faces'], np.int64).reshape(-1, 3)).cuda() for s in ('left', 'right')]
    r, m = ops.CONTACT_DIST, ops.CONTACT_MAX_DEPTH
    head = {'device': torch.cuda.get_device_name(0), 'repeats': a.repeats, 'warmup': a.warmup, 'timing': 'HIP events, median',
            'frames': B, 'contact_dist': r, 'max_depth': m}
    lines = {'vertex': dict({'tool': 'contact_bench'}, **head),
             'surface': dict({'tool': 'surface_contact_bench'}, **head, faces=int(faces[0].shape[0]))}
    modes = ('vertex', 'surface') if a.mode == 'both' else (a.mode,)
    for mode in modes:      # (each mode on its own pass over K, with its own generator: the scene and the order of a single-mode run)
        rng = np.random.default_rng(0)
        for K in (1, 2, 4):
            kw = dict(project=True) if K == 1 else dict(project=True, max_hand=K)
            fwd = timed(lambda: eng.forward(frames, **kw), a.warmup, a.repeats)
            out = eng.forward(frames, **kw)
            lead = (B, K, 2)
            out = {k: v.view(lead + tuple(v.shape[len(v.shape) - (1 if k == 'slots' else 2):])) for k, v in out.items()}
            out['slots'][..., L.SLOT_FLAG] = 1.0
            ct = torch.from_numpy((np.array((0, 0, 0.8)) + rng.uniform(-0.03, 0.03, lead + (3,))).astype(np.float32)).cuda()
            lines[mode]['max_hand_%d' % K] = (vertex_figures(eng, out, K, ct, fwd, a, faces, r, m) if mode == 'vertex' else
                                               surface_figures(eng, out, K, ct, fwd, a, lines[mode]['faces']))
    text = '\n'.join(json.dumps(lines[mode]) for mode in modes)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    eng.close()


if __name__ == '__main__':
    main()
