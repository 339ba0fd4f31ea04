"""Cost of decoding several hands of each side per frame on one GPU, one JSON line.

    python tools/multi_hand_bench.py [--repeats 30] [--warmup 5] [--timeout 600] [--out FILE]

  decode alone   HIP events around one call as the caller sees it, median of `repeats`, on the resident head maps of a batch of
                 64: Engine.decode (acrmi_decode) and Engine.decode(max_hand=K) for K = 1, 2, 4, 8.
  fused call     Engine.forward with the point heads off and on, Engine.forward(max_hand=K) for K = 1, 2, 4, 8 with the dense
                 heads and, for K = 2, 4, 8, with the point heads at the K best centres (set_point_heads_multi), at batch 64 and
                 at batch 1; the variants alternate `rounds` times.  The K > 1 variants run with a threshold under every
                 value of the maps: every rank has a detection, so the point heads evaluate as many points as they ever do
                 (`tower_points_per_frame` says how many; the dense heads do not depend on the threshold).
  point heads    acrmi_point_heads and acrmi_point_heads_multi (K = 1, 2, 4, 8) alone on the resident maps of the batch of 64,
                 under the same threshold.
  MANO           Engine.mano on the 2 * K * B rows the fused call hands it (placeholders included), for the same K and batches.
The run ends itself after `--timeout` seconds."""
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


ALL_RANKS = -3.0e38      # a threshold every value of an NMS'd centre map passes


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
    ap.add_argument('--rounds', type=int, default=2, help='alternations of the fused variants')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--timeout', type=int, default=600, help='seconds after which the run ends itself')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('multi_hand_bench needs a GPU: there is no CPU path to time')
    signal.alarm(a.timeout)
    pkg = lambda sub: importlib.import_module(PKG + '.' + sub)
    synth, L, E = pkg('synth'), pkg('_lib'), pkg('engine')
    line = {'tool': 'multi_hand_bench', 'device': torch.cuda.get_device_name(0), 'repeats': a.repeats, 'warmup': a.warmup,
            'timing': 'HIP events, median of repeats, one process'}
    sd = synth.make_state_dict(seed=0)
    tables = synth.make_mano_tables(seed=1)
    tables['left']['shapedirs'] = tables['left']['shapedirs'].copy()
    tables['left']['shapedirs'][:, 0, :] *= -1
    fused, mano = {}, {}
    for B in (a.batch, 1):
        frames = torch.from_numpy(synth.make_frames(B, seed=0, structured=False)).cuda()
        eng = E.Engine(0)
        eng.load_state_dict(sd, max_batch=B)
        eng.load_mano(tables)
        if B == a.batch:      # the decode alone, on the head maps of this batch
            eng.backbone_heads(frames)
            alone = {'acrmi_decode': timed(lambda: eng.decode(B), a.warmup, a.repeats)}
            # (Engine.decode(max_hand=1) is acrmi_decode: the new kernel at K = 1 is timed through the C call)
            one = torch.empty(B, 1, 2, L.SLOT, dtype=torch.float32, device='cuda')
            stream = torch.cuda.current_stream().cuda_stream
            alone['max_hand_1'] = timed(lambda: L.check(eng.L.acrmi_decode_multi(eng.ctx, B, 1, one.data_ptr(), stream), eng.ctx),
                                        a.warmup, a.repeats)
            for K in (2, 4, 8):
                alone['max_hand_%d' % K] = timed(lambda: eng.decode(B, max_hand=K), a.warmup, a.repeats)
            line['decode_alone_batch_%d' % B] = alone
            eng.set_conf_thresh(ALL_RANKS)
            heads = {'acrmi_point_heads': timed(lambda: eng.run_point_heads(B), a.warmup, a.repeats)}
            for K in (1, 2, 4, 8):
                call = lambda: L.check(eng.L.acrmi_point_heads_multi(eng.ctx, B, K, stream), eng.ctx)
                heads['max_hand_%d' % K] = timed(call, a.warmup, a.repeats)
            slots = eng.decode(B, max_hand=8)
            flat, flag = slots[..., L.SLOT_FLATIND], slots[..., L.SLOT_FLAG]
            assert bool((flag > 0.5).all())
            line['tower_points_per_frame'] = {'max_hand_%d' % K: round(sum(
                2 * len(set(flat[b, :K, h].tolist())) + len(set(flat[b, :K, 1 - h].tolist())) for b in range(B) for h in (0, 1)) / B, 2)
                for K in (2, 4, 8)}      # an upper bound: every hand has a partner within 32 px
            eng.set_conf_thresh(0.35)
            line['point_heads_alone_batch_%d' % B] = heads

        def forward(point, K):
            eng.set_point_heads(point and K == 1)
            eng.set_point_heads_multi(point and K > 1)
            eng.set_conf_thresh(ALL_RANKS if K > 1 else 0.35)
            try:
                return timed(lambda: eng.forward(frames, max_hand=K), a.warmup, a.repeats)['median_ms']
            finally:
                eng.set_point_heads(False)
                eng.set_point_heads_multi(False)
                eng.set_conf_thresh(0.35)

        def forward_multi_1():      # acrmi_forward_multi with max_hand = 1 (Engine.forward(max_hand=1) is acrmi_forward)
            out = eng.forward(frames)
            stream = torch.cuda.current_stream().cuda_stream
            call = lambda: L.check(eng.L.acrmi_forward_multi(eng.ctx, frames.data_ptr(), B, 1, None, out['slots'].data_ptr(),
                                                             out['verts'].data_ptr(), out['joints'].data_ptr(), None, None, None,
                                                             stream), eng.ctx)
            return timed(call, a.warmup, a.repeats)['median_ms']

        runs = {'forward_dense': [], 'forward_point_heads': [], 'max_hand_1': [], 'max_hand_2': [], 'max_hand_4': [],
                'max_hand_8': [], 'max_hand_2_point_heads': [], 'max_hand_4_point_heads': [], 'max_hand_8_point_heads': []}
        for _ in range(a.rounds):      # the variants alternate, so that a drift of the machine meets all of them
            runs['forward_dense'].append(forward(False, 1))
            runs['forward_point_heads'].append(forward(True, 1))
            runs['max_hand_1'].append(forward_multi_1())
            for K in (2, 4, 8):
                runs['max_hand_%d' % K].append(forward(False, K))
                runs['max_hand_%d_point_heads' % K].append(forward(True, K))
        fused['batch_%d_ms' % B] = runs
        rows = {}
        for K in (1, 2, 4):
            n = 2 * K * B
            poses, betas = torch.randn(n, 48, device='cuda') * 0.3, torch.randn(n, 10, device='cuda') * 0.5
            side = (torch.arange(n) & 1).to(torch.int32).cuda()
            rows['rows_%d' % n] = timed(lambda: eng.mano(poses, betas, side), a.warmup, a.repeats)
        mano['batch_%d' % B] = rows
        eng.close()
    line['fused'] = fused
    line['mano_alone'] = mano
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
