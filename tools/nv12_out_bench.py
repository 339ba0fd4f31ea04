"""Cost of NV12 output (csrc/nv12_out.hip; DESIGN.md "NV12 output") on one GPU, one JSON line.

    python tools/nv12_out_bench.py [--repeats 30] [--warmup 5] [--frames 64] [--timeout 600] [--out FILE]

For 64 frames of 1080 x 1920 and 64 frames of 512 x 512, HIP events around one call as the caller sees it (list handling,
ctypes, launches and kernels, the allocation of the result), median of `repeats`:
  bgr_to_nv12     ops.bgr_to_nv12 on packed BGR frames: 3 bytes in and 1.5 out per pixel
  nv12_compose    ops.nv12_compose of drawn frames over their source surfaces: 4.5 in and 1.5 out
  nv12_to_bgr     ops.nv12_to_bgr on the same frames: the sibling with nearly the plain conversion's traffic
  copy_*          torch copy_ that moves as many bytes, read plus written, as the operator of that name: its floor, timed in
                  the same process; every operator carries `ratio_to_copy`
  abi_*           the C entry point of that operator alone, its argument arrays built once: the launches and the kernels without
                  the Python layer's per-frame work (HIP events around 10 queued calls, a tenth of it; median of `repeats`)
  torch_ops       one formulation of the plain conversion in torch ops, as a caller would write it without this library
                  (float weighted sums, 2x2 mean, round, clamp); `torch_ops_equals_rule` says whether its bytes are the rule's
with the bytes each reads and writes per frame, computed from the shapes.  No ratio is asserted: the tool reports.
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


def abi_calls(ops, nv12, bgr, drawn, out):
    """-> {name: a function that makes the C call of that operator with arrays built here, once}."""
    import ctypes as C
    L = importlib.import_module(PKG + '._lib')
    lib = L.lib()
    n = nv12.shape[0]
    frames, sizes, dev, keep = ops._nv12_frames(nv12)
    _, surfaces, keep_out = ops._nv12_surfaces(out, sizes, dev, 'nv12_out_bench')
    src = (C.c_void_p * n)(*[bgr[i].data_ptr() for i in range(n)])
    drw = (C.c_void_p * n)(*[drawn[i].data_ptr() for i in range(n)])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def plain():
        L.check(lib.acrmi_rgb_to_nv12(src, surfaces, n, None, 1, stream))

    def compose():
        L.check(lib.acrmi_nv12_compose(frames, drw, surfaces, n, None, None, 1, stream))

    plain.keep = compose.keep = (keep, keep_out)
    return {'bgr_to_nv12': plain, 'nv12_compose': compose}


def smooth_nv12(n, H, W, seed):
    """n NV12 surfaces [n, H*3/2, W] of smooth pictures (a video frame is not noise; the kernels' time does not depend on
    the values, only the caches' hit rates on the addresses, which are the same)."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H * 3 // 2, 0:W].astype(np.float32)
    out = np.empty((n, H * 3 // 2, W), np.uint8)
    for i in range(n):
        a, b, c = g.uniform(0.002, 0.02, 3)
        out[i] = (127.5 + 127.5 * np.sin(a * xx + b * yy + 6.28 * c * i)).astype(np.uint8)
    return torch.from_numpy(out)


def torch_bgr_to_nv12(bgr, row10):
    """[n,H,W,3] uint8 BGR -> [n,H*3/2,W] uint8 with torch ops: the coefficients of the row as floats."""
    n, H, W, _ = bgr.shape
    c = [float(v) / 2.0 ** 20 for v in row10[:9]]                                                 # rows Y, U, V over R, G, B
    planes = bgr.permute(0, 3, 1, 2).float()                                                      # [n,3,H,W]: B, G, R
    B, G, R = planes[:, 0], planes[:, 1], planes[:, 2]
    y = (c[0] * R + c[1] * G + c[2] * B + float(row10[9])).round().clamp(0, 255).to(torch.uint8)
    mean = torch.nn.functional.avg_pool2d(planes, 2)                                              # [n,3,H/2,W/2]
    B, G, R = mean[:, 0], mean[:, 1], mean[:, 2]
    u = (c[3] * R + c[4] * G + c[5] * B + 128.0).round().clamp(0, 255).to(torch.uint8)
    v = (c[6] * R + c[7] * G + c[8] * B + 128.0).round().clamp(0, 255).to(torch.uint8)
    return torch.cat([y, torch.stack([u, v], -1).reshape(n, H // 2, W)], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--timeout', type=int, default=600, help='seconds after which the run ends itself')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('nv12_out_bench needs a GPU: there is no CPU path to time')
    signal.alarm(a.timeout)
    ops = importlib.import_module(PKG + '.ops')
    n = a.frames
    row10 = ops.nv12_out_matrix('cv601')
    line = {'tool': 'nv12_out_bench', 'device': torch.cuda.get_device_name(0), 'repeats': a.repeats, 'warmup': a.warmup, 'frames': n,
            'timing': 'HIP events around one call of n frames, median', 'sizes': {}}
    for H, W in ((1080, 1920), (512, 512)):
        px = H * W
        nv12 = smooth_nv12(n, H, W, seed=H).cuda()
        bgr = ops.nv12_to_bgr(nv12)
        drawn = bgr.clone()
        drawn[:, H // 4:H // 2, W // 4:W // 2] = 255 - drawn[:, H // 4:H // 2, W // 4:W // 2]      # something was drawn
        torch.cuda.synchronize()
        traffic = {'bgr_to_nv12': (3 * px, px * 3 // 2), 'nv12_compose': (px * 9 // 2, px * 3 // 2), 'nv12_to_bgr': (px * 3 // 2, 3 * px)}
        calls = {'bgr_to_nv12': lambda: ops.bgr_to_nv12(bgr), 'nv12_compose': lambda: ops.nv12_compose(nv12, drawn),
                 'nv12_to_bgr': lambda: ops.nv12_to_bgr(nv12)}
        res = {}
        for name, fn in calls.items():
            rd, wr = traffic[name]
            half = n * (rd + wr) // 2              # a copy of `half` bytes reads and writes rd + wr bytes a frame
            a_buf = torch.empty(half, dtype=torch.uint8, device='cuda')
            b_buf = torch.empty(half, dtype=torch.uint8, device='cuda')
            copy = timed(lambda: b_buf.copy_(a_buf), a.warmup, a.repeats)
            del a_buf, b_buf
            res[name] = dict(timed(fn, a.warmup, a.repeats), source_bytes_per_frame=rd, written_bytes_per_frame=wr)
            res[name]['ms_per_frame'] = round(res[name]['median_ms'] / n, 5)
            res[name]['gb_per_s'] = round(n * (rd + wr) / res[name]['median_ms'] / 1e6, 1)
            res['copy_' + name] = dict(copy, bytes_copied=half)
            res[name]['ratio_to_copy'] = round(res[name]['median_ms'] / copy['median_ms'], 3)
        out = torch.empty_like(nv12)
        for name, fn in abi_calls(ops, nv12, bgr, drawn, out).items():
            ten = timed(lambda: [fn() for _ in range(10)], a.warmup, a.repeats)
            res['abi_' + name] = {k: round(v / 10, 4) for k, v in ten.items()}
            res['abi_' + name]['ratio_to_copy'] = round(res['abi_' + name]['median_ms'] / res['copy_' + name]['median_ms'], 3)
        del out
        res['torch_ops'] = dict(timed(lambda: torch_bgr_to_nv12(bgr, row10), a.warmup, max(3, a.repeats // 3)),
                                source_bytes_per_frame=3 * px, written_bytes_per_frame=px * 3 // 2)
        res['torch_ops']['ms_per_frame'] = round(res['torch_ops']['median_ms'] / n, 5)
        res['torch_ops']['ratio_to_copy'] = round(res['torch_ops']['median_ms'] / res['copy_bgr_to_nv12']['median_ms'], 3)
        by_rule, by_torch = ops.bgr_to_nv12(bgr[:4]), torch_bgr_to_nv12(bgr[:4], row10)
        res['torch_ops_equals_rule'] = bool(torch.equal(by_rule, by_torch))
        res['torch_ops_bytes_differing'] = int((by_rule != by_torch).sum())
        res['compose_identity_holds'] = bool(torch.equal(ops.nv12_compose(nv12[:4], bgr[:4]), nv12[:4]))
        line['sizes']['%dx%d' % (H, W)] = res
        del nv12, bgr, drawn
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
