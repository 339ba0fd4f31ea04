"""Cost of per-stream One-Euro smoothing (engine.StreamTable; DESIGN.md "Per-stream smoothing") on one GPU, one JSON line.

    python tools/smooth_bench.py [--repeats 30] [--warmup 5] [--steps 20] [--timeout 600] [--out FILE] [--compare DIR]

  smoothing alone   HIP events around one call as the caller sees it, median of `repeats`: 64 frames of 64 streams through
                    Engine.smooth(streams=, table=); the same 64 frames as ONE stream through Engine.smooth; with --compare,
                    the latter also through the package at DIR (another build, e.g. the parent commit's).
  fused call        batch 64 of the bench frames: Engine.forward without smoothing, then with streams= / table=, on one
                    context (HIP events, median) and on an EnginePool of two (wall clock over `steps` batches in flight as
                    bench.py keeps them, alternating the two variants `rounds` times); with --compare, the un-smoothed
                    forward of DIR's package in the same process as well.
The run ends itself after `--timeout` seconds."""
import argparse
import importlib
import importlib.util
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
PKG = 'arbitrary-hands-3d-reconstruction_amd'


def package(path, name):
    """The package at `path` imported under `name` -> sub-module getter (two builds side by side in one process)."""
    spec = importlib.util.spec_from_file_location(name, os.path.join(path, '__init__.py'), submodule_search_locations=[path])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return lambda sub: importlib.import_module(name + '.' + sub)


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


def smooth_slots(L, n):
    """n frames of a random walk, both hands flagged."""
    g = np.random.default_rng(0)
    s = np.zeros((n, 2, L.SLOT), np.float32)
    s[:, :, L.SLOT_FLAG] = 1.0
    s[:, :, L.SLOT_POSES:L.SLOT_POSES + 48] = np.cumsum(g.normal(0, 0.12, (n, 2, 48)), 0)
    s[:, :, L.SLOT_BETAS:L.SLOT_BETAS + 10] = np.cumsum(g.normal(0, 0.05, (n, 2, 10)), 0)
    return torch.from_numpy(s).cuda()


def pool_ms(pool, frames, steps, streams):
    """Milliseconds per batch with one ticket left outstanding behind a submit."""
    def run(n):
        pend = []
        for _ in range(n):
            pend.append(pool.submit(frames, streams=streams) if streams is not None else pool.submit(frames))
            while len(pend) > 1:
                pool.collect(pend.pop(0))
        for t in pend:
            pool.collect(t)
    run(2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--steps', type=int, default=20, help='batches per timed pool window')
    ap.add_argument('--rounds', type=int, default=3, help='alternations of the pool variants')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--timeout', type=int, default=600, help='seconds after which the run ends itself')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    ap.add_argument('--compare', default=None, help='directory of another build of the package to time next to this one')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('smooth_bench needs a GPU: there is no CPU path to time')
    signal.alarm(a.timeout)
    pkg = lambda sub: importlib.import_module(PKG + '.' + sub)
    other = package(os.path.abspath(a.compare), 'acrmi_compare') if a.compare else None
    synth, L, E = pkg('synth'), pkg('_lib'), pkg('engine')
    B = a.batch
    line = {'tool': 'smooth_bench', 'device': torch.cuda.get_device_name(0), 'repeats': a.repeats, 'warmup': a.warmup,
            'batch': B, 'timing': 'HIP events, median (pool: wall clock per batch)'}

    # ---- smoothing alone ----
    slots = smooth_slots(L, B)
    eng = E.Engine(0)
    table = E.StreamTable(0, B)
    ids = np.arange(B, dtype=np.int32)
    work = slots.clone()
    alone = {'streams_%dx1' % B: timed(lambda: eng.smooth(work, streams=ids, table=table), a.warmup, a.repeats),
             'one_stream_%d' % B: timed(lambda: eng.smooth(work), a.warmup, a.repeats)}
    one_table = E.StreamTable(0, 1)
    alone['one_stream_%d_shared_table' % B] = timed(lambda: eng.smooth(work, streams=np.zeros(B, np.int32), table=one_table),
                                                    a.warmup, a.repeats)
    if other:
        oeng = other('engine').Engine(0)
        alone['compare_one_stream_%d' % B] = timed(lambda: oeng.smooth(work), a.warmup, a.repeats)
    line['smoothing_alone'] = alone

    # ---- fused call ----
    sd = synth.make_state_dict(seed=0)
    tables = synth.make_mano_tables(seed=1)
    tables['left']['shapedirs'] = tables['left']['shapedirs'].copy()
    tables['left']['shapedirs'][:, 0, :] *= -1
    frames = torch.from_numpy(synth.make_frames(B, seed=0, structured=False)).cuda()
    eng.load_state_dict(sd, max_batch=B)
    eng.load_mano(tables)
    fused = {}
    if other:
        oeng.load_state_dict(sd, max_batch=B)
        oeng.load_mano(tables)
    # the variants alternate, so that a drift of the machine meets all of them
    runs = {'forward': [], 'forward_streams': [], 'compare_forward': []}
    for _ in range(a.rounds):
        runs['forward'].append(timed(lambda: eng.forward(frames), a.warmup, a.repeats)['median_ms'])
        runs['forward_streams'].append(timed(lambda: eng.forward(frames, streams=ids, table=table), a.warmup, a.repeats)['median_ms'])
        if other:
            runs['compare_forward'].append(timed(lambda: oeng.forward(frames), a.warmup, a.repeats)['median_ms'])
    fused['one_context_ms'] = {k: v for k, v in runs.items() if v}
    if other:
        oeng.close()
    pool = E.EnginePool(0, n=2, first=eng)
    pool.load_state_dict(None, max_batch=B, lanes=1)
    pool.load_mano(None)
    pool.stream_table(B)
    runs = {'submit': [], 'submit_streams': []}
    for _ in range(a.rounds):
        runs['submit'].append(round(pool_ms(pool, frames, a.steps, None), 4))
        runs['submit_streams'].append(round(pool_ms(pool, frames, a.steps, ids), 4))
    fused['pool_of_two_ms_per_batch'] = runs
    line['fused'] = fused
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    table.close()
    one_table.close()
    pool.close()


if __name__ == '__main__':
    main()
