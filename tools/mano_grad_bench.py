"""Time of the differentiable ManoLayer (acrmi_mano_backward) next to MANO written in torch ops, on one
GPU, one JSON line.

    python tools/mano_grad_bench.py [--repeats 30] [--warmup 5] [--timeout 600] [--out FILE]

Per call as the caller sees it, HIP events around the calls on one stream, a warm-up, then the median over `repeats`, at
H = 1, 128 and 1024 right hands (center_idx 9, seeded poses and betas on the device):
  forward    ManoLayer(pose, betas) with pose requiring grad: the forward kernel and the autograd node around it
  backward   (verts * c_v).sum() + (joints * c_j).sum() of that call, .backward(): torch's two products and the backward kernel
  both       the two together
  torch_*    the same three through tests/mano_grad_ref.py in float32 on the same device - MANO restated in torch ops with
             torch's autograd, the form a caller has to write without the kernel
  fit        the 300 Adam steps of tests/test_gpu_mano_grad.py::test_it_fits (8 hands), wall clock of the whole loop, through
             ManoLayer and through the torch form
There is no pass mark: the numbers are written down (README.md).  The run ends itself after `--timeout` seconds."""
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))
PKG = 'arbitrary-hands-3d-reconstruction_amd'


def pkg(sub):
    return importlib.import_module(PKG + '.' + sub)


def timed(fn, warmup, repeats, setup=None):
    def once(measure):
        state = setup() if setup else None
        if not measure:
            fn(state)
            return None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(state)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)
    for _ in range(warmup):
        once(False)
    torch.cuda.synchronize()
    ms = [once(True) for _ in range(repeats)]
    return {'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4)}


def fit(forward, steps=300):
    """test_it_fits' loop on `forward(pose, betas) -> joints`: -> (seconds, first loss, last loss)."""
    rng = np.random.RandomState(3)
    with torch.no_grad():
        target = forward(torch.from_numpy((rng.randn(8, 48) * 0.3).astype(np.float32)).cuda(),
                         torch.from_numpy((rng.randn(8, 10) * 0.5).astype(np.float32)).cuda())
    pose = torch.zeros(8, 48, device='cuda', requires_grad=True)
    betas = torch.zeros(8, 10, device='cuda', requires_grad=True)
    opt = torch.optim.Adam([pose, betas], lr=0.02)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    first = None
    for _ in range(steps):
        opt.zero_grad()
        loss = ((forward(pose, betas) - target) ** 2).sum(-1).mean()
        loss.backward()
        opt.step()
        first = loss.detach() if first is None else first
    with torch.no_grad():
        last = ((forward(pose, betas) - target) ** 2).sum(-1).mean()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, float(first), float(last)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--timeout', type=int, default=600, help='seconds after which the run ends itself')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('mano_grad_bench needs a GPU: there is no CPU path to time')
    signal.alarm(a.timeout)
    import mano_grad_ref as ref
    tables = pkg('synth').make_mano_tables(seed=1)
    M = pkg('mano.manolayer')
    layer = M.ManoLayer(tables=tables['right'], center_idx=9, side='right', use_pca=False, flat_hand_mean=False)
    T = ref.as_tables(tables['right'], torch.float32, 'cuda')
    line = {'tool': 'mano_grad_bench', 'device': torch.cuda.get_device_name(0), 'repeats': a.repeats, 'warmup': a.warmup,
            'timing': 'HIP events, median, per call', 'torch_form': 'float32 torch ops + torch autograd on the same device'}
    gen = torch.Generator(device='cuda').manual_seed(0)
    for H in (1, 128, 1024):
        pose = (0.3 * torch.randn(H, 48, device='cuda', generator=gen)).requires_grad_()
        betas = (0.5 * torch.randn(H, 10, device='cuda', generator=gen)).requires_grad_()
        cv, cj = torch.randn(H, 778, 3, device='cuda', generator=gen), torch.randn(H, 21, 3, device='cuda', generator=gen)
        forms = {'': lambda: layer(pose, betas), 'torch_': lambda: ref.mano(T, 'right', pose, betas, 9)}
        res = {}
        for prefix, fwd in forms.items():
            def loss_of(out):
                return (out[0] * cv).sum() + (out[1] * cj).sum()

            def clear():
                pose.grad = betas.grad = None
            res[prefix + 'forward'] = timed(lambda s: fwd(), a.warmup, a.repeats)
            res[prefix + 'backward'] = timed(lambda s: s.backward(), a.warmup, a.repeats, setup=lambda: (clear(), loss_of(fwd()))[1])
            res[prefix + 'both'] = timed(lambda s: loss_of(fwd()).backward(), a.warmup, a.repeats, setup=clear)
            clear()
            loss_of(fwd()).backward()
            res[prefix + 'g_pose'] = pose.grad.clone()
        g, gt = res.pop('g_pose'), res.pop('torch_g_pose')
        res['largest_g_pose_difference_to_torch'] = float((g - gt).abs().max() / gt.abs().max())
        res['torch_over_kernel_both'] = round(res['torch_both']['median_ms'] / res['both']['median_ms'], 2)
        line['H_%d' % H] = res
    free = M.ManoLayer(tables=tables['right'], center_idx=None, side='right', use_pca=False, flat_hand_mean=False)
    for name, fwd in (('fit', lambda p, b: free(p, b)[1]), ('torch_fit', lambda p, b: ref.mano(T, 'right', p, b, None)[1])):
        fit(fwd, steps=10)
        sec, first, last = fit(fwd)
        line[name] = {'seconds': round(sec, 4), 'ms_per_step': round(sec * 1000 / 300, 4), 'loss_first': first, 'loss_last': last,
                      'fold': round(first / last, 1)}
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
