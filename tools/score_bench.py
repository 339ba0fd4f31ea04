"""Time of scoring a batch against ground truth (Engine.score) next to two comparisons from the same
process, on one GPU, one JSON line.

    python tools/score_bench.py [--repeats 30] [--warmup 5] [--runs 2] [--timeout 600] [--out FILE]

The 64 bench frames (512 x 512) go through Engine.forward once per K = max_hand in (1, 2, 4); every slot is then flagged, so
that all 64 * K * 2 hands are scored, joints and vertices, and added to a ScoreBoard: the most work there can be.  The truth
is the prediction scaled by 1.05 with 4 mm of noise.  Timed in one process with HIP events around the calls on one stream - a
warm-up, then the median over `repeats`, `runs` times:
  score     Engine.score(out, gt, board=board) (cam_trans handed in): one pose-errors launch over both point sets, two
            accumulate launches
  torch     the same quantities written in torch ops on the same tensors, float64: root-aligned errors, the Umeyama alignment
            through a batched torch.linalg.svd, the per-point sums and counts by group, the histogram, the pair terms - what a
            caller would write without the kernels, WITHOUT the host visit per batch such code usually ends in
  forward   Engine.forward(project=True[, max_hand=K]) of those frames: the step that feeds it, untouched by the scoring path
The torch form is a yardstick for the cost, not for the bits: its summation order and its SVD are torch's.  The run ends
itself after `--timeout` seconds."""
import argparse
import importlib
import json
import os
import signal
import statistics
import sys

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


def torch_set(P, G, oP, oG, group, n_groups, n_bins, bin_width, state):
    """One point set in torch ops: P, G [N,n,3] float64, origins [N,3] -> (e_ra, e_pa [N,n]); the sums go into `state`."""
    e_ra = ((P - oP[:, None]) - (G - oG[:, None])).norm(dim=-1)
    mp, mg = P.mean(1, keepdim=True), G.mean(1, keepdim=True)
    pc, gc = P - mp, G - mg
    U, D, Vt = torch.linalg.svd(gc.transpose(1, 2) @ pc)
    d = torch.ones_like(D)
    d[:, 2] = torch.sign(torch.linalg.det(U) * torch.linalg.det(Vt))
    R = U @ torch.diag_embed(d) @ Vt
    scale = (D * d).sum(1) / (pc * pc).sum((1, 2))
    e_pa = (scale[:, None, None] * (pc @ R.transpose(1, 2)) + mg - G).norm(dim=-1)
    state['sum_ra'].index_add_(0, group, e_ra)
    state['sum_pa'].index_add_(0, group, e_pa)
    state['cnt'].index_add_(0, group, torch.ones_like(e_ra))
    bins = (e_ra / bin_width).long().clamp(max=n_bins) + group[:, None] * (n_bins + 1)
    state['hist'] += torch.bincount(bins.reshape(-1), minlength=n_groups * (n_bins + 1))
    return e_ra, e_pa


def torch_score(out, gt, ct, root, n_bins, bin_width, states):
    N = out['joints'].numel() // 63
    j, gj = out['joints'].reshape(N, 21, 3).double(), gt['joints'].reshape(N, 21, 3).double()
    v, gv = out['verts'].reshape(N, 778, 3).double(), gt['verts'].reshape(N, 778, 3).double()
    group = torch.arange(N, device=j.device) % 2
    oP, oG = j[:, root], gj[:, root]
    res = [torch_set(j, gj, oP, oG, group, 2, n_bins, bin_width, states[0]), torch_set(v, gv, oP, oG, group, 2, n_bins, bin_width, states[1])]
    placed = oP + ct.reshape(N, 3).double()
    rel = ((placed[1::2] - placed[0::2]) - (oG[1::2] - oG[0::2])).norm(dim=-1)
    states[0]['pair'] += rel.sum()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--runs', type=int, default=2)
    ap.add_argument('--timeout', type=int, default=600, help='seconds after which the run ends itself')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('score_bench needs a GPU: there is no CPU path to time')
    signal.alarm(a.timeout)
    synth, L, E, S = pkg('synth'), pkg('_lib'), pkg('engine'), pkg('score')
    eng = E.Engine(0)
    eng.load_state_dict(synth.make_state_dict(seed=0), max_batch=64)
    tables = synth.make_mano_tables(seed=1)
    tables['left']['shapedirs'] = tables['left']['shapedirs'].copy()
    tables['left']['shapedirs'][:, 0, :] *= -1
    eng.load_mano(tables)
    B = 64
    frames = torch.from_numpy(synth.make_frames(B, seed=0, structured=False)).cuda()
    line = {'tool': 'score_bench', 'device': torch.cuda.get_device_name(0), 'repeats': a.repeats, 'warmup': a.warmup, 'runs': a.runs,
            'timing': 'HIP events, median', 'frames': B, 'n_bins': S.N_BINS, 'bin_width': S.BIN_WIDTH,
            'torch_form': 'float64 torch ops with batched torch.linalg.svd; the host visit per batch is left out'}
    gen = torch.Generator(device='cuda').manual_seed(0)
    for K in (1, 2, 4):
        kw = dict(project=True) if K == 1 else dict(project=True, max_hand=K)
        out = eng.forward(frames, **kw)
        lead = (B, K, 2)
        out = {k: v.view(lead + tuple(v.shape[len(v.shape) - (1 if k == 'slots' else 2):])) for k, v in out.items()}
        out['slots'][..., L.SLOT_FLAG] = 1.0
        gt = {k: out[k] * 1.05 + 0.004 * torch.randn(out[k].shape, device='cuda', generator=gen) for k in ('joints', 'verts')}
        ct = torch.tensor((0, 0, 0.8), device='cuda') + 0.03 * torch.randn(lead + (3,), device='cuda', generator=gen)
        board = E.ScoreBoard(0)
        new = lambda n: {'sum_ra': torch.zeros(2, n, dtype=torch.float64, device='cuda'), 'sum_pa': torch.zeros(2, n, dtype=torch.float64, device='cuda'),
                         'cnt': torch.zeros(2, n, dtype=torch.float64, device='cuda'),
                         'hist': torch.zeros(2 * (S.N_BINS + 1), dtype=torch.int64, device='cuda'),
                         'pair': torch.zeros((), dtype=torch.float64, device='cuda')}
        states = [new(21), new(778)]
        runs = []
        for _ in range(a.runs):
            runs.append({'score': timed(lambda: eng.score(out, gt, board=board, max_hand=K, cam_trans=ct), a.warmup, a.repeats),
                         'torch': timed(lambda: torch_score(out, gt, ct, 9, S.N_BINS, S.BIN_WIDTH, states), a.warmup, a.repeats),
                         'forward': timed(lambda: eng.forward(frames, **kw), a.warmup, a.repeats)})
        # the two forms describe the same thing (the torch one rounds in its own order)
        res = eng.score(out, gt, max_hand=K, cam_trans=ct)
        ref = torch_score(out, gt, ct, 9, S.N_BINS, S.BIN_WIDTH, states)
        diff = max(float((res[name]['e_pa'].double() - r[1]).abs().max()) for name, r in zip(('joints', 'verts'), ref))
        best = {k: min(r[k]['median_ms'] for r in runs) for k in ('score', 'torch', 'forward')}
        s = board.summary()['all']
        line['max_hand_%d' % K] = {'hands': B * K * 2, 'runs': runs, 'torch_over_score': round(best['torch'] / best['score'], 2),
                                   'share_of_forward': round(best['score'] / best['forward'], 4),
                                   'largest_e_pa_difference_to_torch_m': diff, 'mpjpe_mm': round(s['mpjpe'] * 1000, 3),
                                   'pa_mpjpe_mm': round(s['pa_mpjpe'] * 1000, 3), 'mpvpe_mm': round(s['mpvpe'] * 1000, 3),
                                   'pa_mpvpe_mm': round(s['pa_mpvpe'] * 1000, 3), 'mrrpe_mm': round(s['mrrpe'] * 1000, 3)}
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    eng.close()


if __name__ == '__main__':
    main()
