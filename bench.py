#!/usr/bin/env python
"""ACR hot-path benchmark: frames/s (2-hand mesh) at 512x512, batch 64 per GPU, HRNet-W32 fp32.

    python bench.py --gpus 1 --steps 10 --warmup 3
    python bench.py --gpus 1 --steps 10 --warmup 3 --full                  (+ everything measured behind the headline)
    python bench.py --gpus 1 --steps 10 --warmup 3 --dump-outputs DIR      (+ the last timed step's results as DIR/*.npy)
    python bench.py --gpus N --steps K --warmup W          (spawns its own N ranks: one process per GPU over RCCL)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W          (the driver's form: ranks already exist)

A step = one pass of the whole path (uint8 frames resident in HBM -> backbone -> heads -> decode ->
MANO -> verts/joints, plus for N>1 the RCCL all-gather of every rank's result slots) over one batch of
64 synthetic frames per GPU (weak scaling).  Synthetic seeded checkpoint + MANO tables (the real assets
are not redistributable).  Prints ONE JSON line on rank 0.

A plain run sets up, warms up, times the K steps and prints the headline line.  Everything else the line can carry (the
roofline pass, point heads, one context, cpu_baseline + parity, latency, live PMC, the 16-bit programs, the other configs,
the multi-GPU diagnostics) runs behind the timed region only with --full; the --no-* switches trim that set.
"""
import argparse
import importlib
import json
import os
import sys
import time

# (rounds 2-5 set GPU_MAX_HW_QUEUES=8 here; round 6 measured the runtime's default of 4 equal or better in every scenario of
#  this file - tools/hwq_probe.sh, the package __init__ - so it is no longer touched; export it to experiment)

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
PKG = 'arbitrary-hands-3d-reconstruction_amd'

GFLOP_PER_FRAME = 102.1          # BASELINE.md §3 / SURVEY.md §8d (2*MAC, direct conv + bmm + linear)
PEAK_F32_MFMA_TFLOPS = 157.3     # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, 256 CU @ 2.4 GHz
DOMINANT = 'conv_wino24b_kernel + conv_wino3_kernel + conv_wino2_kernel (3x3 stride-1 convolutions: Winograd F(2x4,3x3) / F(2x2,3x3) on fp32 MFMA)'
MFMA_REDUCTION = {'winograd_f2x2_3x3': 2.25, 'winograd_f2x2_3x3_lds': 2.25, 'winograd_f23x': 1.5, 'winograd_f2x4_3x3': 3.0}   # algorithmic MACs per executed MFMA MAC
PROFILE_TAGS = ('r06', 'r05', 'r04', 'r03', 'r02', 'r01')     # newest committed rocprofv3 summaries first (profiles/, tools/profile_round.sh)


def pkg(sub):
    return importlib.import_module(PKG + '.' + sub)


def _cpu_model():
    try:
        with open('/proc/cpuinfo') as f:
            txt = f.read()
        model = next((l.split(':', 1)[1].strip() for l in txt.splitlines() if l.startswith('model name')), 'unknown')
        cores = set()
        phys = core = None
        for l in txt.splitlines():
            if l.startswith('physical id'):
                phys = l.split(':')[1].strip()
            elif l.startswith('core id'):
                core = l.split(':')[1].strip()
                cores.add((phys, core))
        return model, (len(cores) or None), os.cpu_count()
    except OSError:
        return 'unknown', None, os.cpu_count()


def cpu_baseline(sd, tables):
    """the oracle (CPU restatement of the reference, oracle/; kind "port") on this box's host cores, same
    synthetic frames.  TWO figures: `physical_cores_fps` - n = all physical cores, what 8(d)(ii) asks for
    (one first-touch pass + one timed pass of batch 8: oversubscribed intra-op parallelism makes it the SLOWER figure on the
    2 x 64-core boxes: 1.6 s per batch of 8 at 16 threads, 7.9 s at 128) - and `value` - the best thread count of a probe over
    {8, 16, 32} (first touch + the better of 2 timed passes each, so that one noisy pass cannot pick the count: r4 reported
    3.9 and r5 8.7 frames/s on the same CPU model), then batch 1 and batch 8 with 2 warm-ups + median of 5.  Bounded: ~45 s."""
    import statistics
    from oracle import acr_net, decode as odec, mano as omano
    frames = torch.from_numpy(pkg('synth').make_frames(8, seed=3))
    model, phys, logical = _cpu_model()
    # what else the box's host side was doing (round 6: 4.8 and 9.2 frames/s from the same code and CPU model on two boxes)
    try:
        load0 = os.getloadavg()
        avail = len(os.sched_getaffinity(0))
    except (OSError, AttributeError):
        load0, avail = None, None

    last = {}

    def run(b):
        with torch.no_grad():
            maps = acr_net.network(sd, frames[:b])
        slots = odec.decode(maps)
        vj = [omano.mano_forward(tables[name], name, slots['poses'][:, h], slots['betas'][:, h])[:2]
              for h, name in ((0, 'left'), (1, 'right'))]
        last[b] = (slots, vj)

    def timed(b):
        t0 = time.perf_counter()
        run(b)
        return time.perf_counter() - t0
    prev = torch.get_num_threads()
    cands = sorted({n for n in (8, 16, 32) if n <= (logical or n)})
    probe = {}
    for n in cands:
        torch.set_num_threads(n)
        timed(8)                                   # first touch at this thread count
        probe[n] = min(timed(8), timed(8))
    best = min(probe, key=probe.get)
    phys_fps = None
    nphys = phys if (phys and phys <= (logical or phys)) else None
    if nphys:
        if nphys in probe:
            phys_fps = 8 / probe[nphys]
        else:
            torch.set_num_threads(nphys)
            timed(8)                               # first touch
            phys_fps = 8 / timed(8)
    torch.set_num_threads(best)
    res = {}
    for b in (1, 8):
        timed(b); timed(b)                         # 2 warm-ups
        res[b] = statistics.median(timed(b) for _ in range(5))
    torch.set_num_threads(prev)
    b1, b8 = 1 / res[1], 8 / res[8]
    slots, vj = last[8]
    # the oracle's results on the 8 frames of the timed sample: bench.py compares the HIP path with them (`parity`)
    oracle = {'frames': frames, 'flag': slots['flag'], 'flat_ind': slots['flat_ind'],
              'verts': np.stack([vj[0][0], vj[1][0]], 1), 'joints': np.stack([vj[0][1], vj[1][1]], 1)}
    return oracle, {'value': round(max(b1, b8), 3), 'unit': 'frames/s', 'cores': best, 'kind': 'port',
            'cpu_model': model, 'physical_cores': phys, 'logical_cores': logical,
            'physical_cores_fps': round(phys_fps, 3) if phys_fps else None,
            'physical_cores_note': 'n = all %s physical cores (SURVEY.md 8d(ii)), batch 8, one timed pass after a first-touch pass' % nphys,
            'batch1_fps': round(1 / res[1], 3), 'batch8_fps': round(8 / res[8], 3),
            'thread_probe_s_per_batch8': {str(k): round(v, 3) for k, v in probe.items()},
            'host': {'loadavg_before': [round(x, 2) for x in load0] if load0 else None, 'cpus_available_to_this_process': avail,
                     'note': 'a GPU box\'s host cores are shared: this figure moves with the other tenants, the GPU figures do not'},
            'sample': 'oracle/ (torch-CPU fp32 restatement of the reference) on the same synthetic 512x512 frames; batch 1 '
                      'and batch 8, 2 warm-ups + median of 5 passes each at %d threads (best of %s, 2 timed passes per count); value = '
                      'the better of the two (batch %d)' % (best, sorted(probe), 1 if b1 >= b8 else 8)}


def parity(eng, oracle):
    """BASELINE.md 4 "parity reported alongside": the HIP path on the frames of the cpu_baseline sample against the
    oracle's results for them - max per-vertex / per-joint L2 distance (metres) over the hands both sides detect at the
    same center; decisions that differ are counted, not hidden."""
    L = pkg('_lib')
    out = eng.forward(oracle['frames'].to(eng.device))
    torch.cuda.synchronize()
    slots = out['slots'].cpu().numpy()
    verts, joints = out['verts'].cpu().numpy(), out['joints'].cpu().numpy()
    flag = slots[..., L.SLOT_FLAG] > 0.5
    same = (flag == oracle['flag']) & (~flag | (slots[..., L.SLOT_FLATIND] == oracle['flat_ind']))
    use = same & flag
    dv = np.linalg.norm(verts - oracle['verts'], axis=-1)[use]
    dj = np.linalg.norm(joints - oracle['joints'], axis=-1)[use]
    return {'max_vertex_l2_m': float(dv.max()) if dv.size else None, 'max_joint_l2_m': float(dj.max()) if dj.size else None,
            'frames': int(flag.shape[0]), 'hands_compared': int(use.sum()), 'decisions_differing': int((~same).sum()),
            'against': 'oracle/ (CPU fp32 restatement pinned to the reference) on the cpu_baseline sample frames'}


def reduced_precision(sd, tables, frames, B, steps, warmup, oracle, local_rank, precisions=('fp16x3', 'bf16x3', 'fp16', 'bf16')):
    """Reported NEXT TO the headline, never as it: the reference's --model_precision fp16 branch (acr/model.py:33-37) and
    its bf16 twin as 16-bit programs (packer.lower) on the same frames, same K steps, two contexts in turn like the
    headline; `parity` = against the fp32 oracle (what 16-bit storage costs), not against a 16-bit reference (none
    exists: autocast is CUDA-only).  'fp16x3' = fp32 STORAGE with split operands on the 16-bit matrix pipe (csrc/conv_x3.inc:
    x = hi + lo in f16, three products per MAC, fp32 accumulation) for the 3x3 and 1x1 layers it takes; every other op is
    the fp32 program's."""
    res = {}
    for prec in precisions:
        pool = pkg('engine').EnginePool(local_rank, n=2)
        pool.load_state_dict(sd, max_batch=B, lanes=1, precision=prec)
        pool.load_mano(tables)
        vsets = [pkg('parallel').alloc_result(B, pool.device)[1] for _ in range(2)]

        def run(n):
            pend = []
            for i in range(n):
                pend.append(pool.submit(frames, out=vsets[i % 2]))
                while len(pend) > 1:
                    pool.collect(pend.pop(0))
            for t in pend:
                pool.collect(t)
        run(max(1, warmup))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        eng = pool.engines[0]
        prof = [p for p in eng.profile_ops(frames) if p.get('mode', 0) != pkg('_lib').MODE_POINT]
        conv_ms = sum(p['ms'] for p in prof if p['kind'] in (pkg('_lib').OP_CONV, pkg('_lib').OP_STEM))
        total_ms = sum(p['ms'] for p in prof)
        flops = sum(p['flops'] for p in prof) * B
        # algorithmic HBM bytes of the conv ops: input + output (+ residual) once, in their storage types
        ops_, bufs_ = eng.program['ops'], eng.program['bufs']
        esz = lambda b: 2 if bufs_[b][4] else 4
        conv_bytes = 0
        for p in prof:
            o = ops_[p['idx']]
            if p['kind'] == pkg('_lib').OP_CONV:
                conv_bytes += B * (bufs_[o.in_buf][0] * bufs_[o.in_buf][1] * o.cin * o.groups * esz(o.in_buf) +
                                   bufs_[o.out_buf][0] * bufs_[o.out_buf][1] * o.cout * o.groups * esz(o.out_buf) *
                                   (2 if o.res_buf >= 0 else 1))
        r = {'value': round(B * steps / dt, 2), 'unit': 'frames/s', 'ms_per_step': round(dt / steps * 1e3, 3),
             'dtype': ('f32 storage; 3x3 (stride 1; stride 2 outside the HR fuse hosts) and 1x1 stride-1 layers: operands split into %s hi + lo, 3 products per MAC on '
                       'v_mfma_f32_32x32x16_%s, f32 accumulate; other ops as the fp32 program' % (({'fp16x3': 'f16', 'bf16x3': 'bf16'}[prec],) * 2)
                       if prec.endswith('x3') else
                       {'fp16': 'f16', 'bf16': 'bf16'}[prec] + ' storage, f32 accumulate (v_mfma_f32_32x32x16)'),
             'all_conv_ms_single_stream': round(conv_ms, 3), 'all_ops_ms_single_stream': round(total_ms, 3),
             'mfma_tflops_single_stream': round(flops / (total_ms * 1e-3) / 1e12, 1), 'mfma_peak_tflops': 2500.0,
             'roofline': {'bound': 'hbm', 'achieved': round(conv_bytes / (conv_ms * 1e-3) / 1e9, 1), 'peak': 8000.0, 'unit': 'GB/s',
                          'frac': round(conv_bytes / (conv_ms * 1e-3) / 1e9 / 8000.0, 4),
                          'definition': 'algorithmic bytes of all conv launches (in + out + residual once, storage types) / their '
                                        'single-stream time; at 16x the fp32 matrix rate the layers are HBM / L2 bound'}}
        if oracle is not None:
            r['parity'] = parity(eng, oracle)
        if prec.endswith('x3'):
            res[prec] = r
        else:
            # 16-bit STORAGE programs: not at the 1e-4 m bar (one rounding per layer of every activation) - an ablation of what
            # the reference's autocast-style lowering costs on this network, never a result to use
            res.setdefault('ablation_16bit_storage', {})[prec] = r
        pool.close()
    res['note'] = ('fp16 / bf16: activations between layers f16 / bf16 NHWC, BN-folded weights rounded once, fp32 '
                   'accumulate / bias / residual / ReLU, one rounding per layer; stem, head exits, attention pooling, '
                   'decode, MANO fp32.  fp16x3: activations and weights stay fp32 in memory; conv_x3_kernel splits every '
                   'operand into two f16 numbers (22 bits) and multiplies on the 16-bit matrix pipe - the accuracy of the '
                   'fp32 program at a higher rate; bf16x3: the same with bf16 halves (16 bits, fp32 exponent range).  '
                   'parity is against the FP32 oracle.')
    return res


def config3_video_stream(sd, tables, steps, warmup, local_rank, B=32, H=1080, W=1920):
    """BASELINE.json configs[3], one GPU's shard (batch 128 over 4 GPUs = 32 frames per GPU), END TO END from host memory
    (reference acr/utils.py:1315-1337 -> network): 1080p BGR uint8 frames in PINNED host memory -> H2D on a
    copy stream into one of two device staging buffers -> acrmi_preprocess (BGR->RGB, white square pad, OpenCV's fixed-point
    INTER_CUBIC to 512x512) -> acrmi_forward with the pad geometry in `offsets` (two contexts in turn).  The copy of batch
    k+1 overlaps pre-processing + network of batch k.  Also timed alone, on the same buffers: the H2D copy, the
    pre-processing kernel (HIP events), the network on resident 512x512 frames - `bound_by` names the slowest stage.
    Parity of this path: tests/test_gpu_api.py::test_raw_1080p_batch_end_to_end (all 32 frames vs the oracle)."""
    import ctypes as C
    ops, L = pkg('ops'), pkg('_lib')
    dev = torch.device('cuda', local_rank)
    host = torch.from_numpy(np.random.RandomState(7).randint(0, 256, (B, H, W, 3), dtype=np.uint8)).pin_memory()
    stage = [torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev) for _ in range(2)]
    pool = pkg('engine').EnginePool(local_rank, n=2)
    pool.load_state_dict(sd, max_batch=B, lanes=1)
    pool.load_mano(tables)
    raw = C.c_void_p()
    L.check(L.lib().acrmi_stream_create(local_rank, C.byref(raw)))       # a plain HIP stream (not torch's pool of 32)
    copy_stream = torch.cuda.ExternalStream(raw.value, device=dev)
    cur = torch.cuda.current_stream(dev)
    vsets = [None, None]      # (the contexts allocate slots / verts / joints / verts_camed / pj2d / pj2d_org per batch)
    frame_bytes = H * W * 3

    def run(n):
        copied = [torch.cuda.Event() for _ in range(2)]
        consumed = [None, None]
        pend = []
        for i in range(n):
            j = i % 2
            if consumed[j] is not None:
                copy_stream.wait_event(consumed[j])             # the staging buffer's previous batch has been pre-processed
            with torch.cuda.stream(copy_stream):
                stage[j].copy_(host, non_blocking=True)
                copied[j].record(copy_stream)
            cur.wait_event(copied[j])
            rgb, offs = ops.preprocess(stage[j])
            consumed[j] = torch.cuda.Event()
            consumed[j].record(cur)
            pend.append(pool.submit(rgb, offsets=offs, project=True, out=vsets[j]))
            while len(pend) > 1:
                pool.collect(pend.pop(0))
        for t in pend:
            pool.collect(t)
    try:
        run(max(2, warmup))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        # ---- the stages alone
        with torch.cuda.stream(copy_stream):
            stage[0].copy_(host, non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        with torch.cuda.stream(copy_stream):
            for i in range(steps):
                stage[i % 2].copy_(host, non_blocking=True)
        torch.cuda.synchronize()
        dt_h2d = (time.perf_counter() - t1) / steps
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        rgb, offs = ops.preprocess(stage[0])
        torch.cuda.synchronize()
        e0.record()
        for _ in range(steps):
            rgb, offs = ops.preprocess(stage[0])
        e1.record()
        torch.cuda.synchronize()
        pre_ms = e0.elapsed_time(e1) / steps

        def net(n):
            pend = []
            for i in range(n):
                pend.append(pool.submit(rgb, offsets=offs, project=True, out=vsets[i % 2]))
                while len(pend) > 1:
                    pool.collect(pend.pop(0))
            for t in pend:
                pool.collect(t)
        net(2)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        net(steps)
        torch.cuda.synchronize()
        dt_net = (time.perf_counter() - t2) / steps
    finally:
        pool.close()
        # the pinned block and the staging buffers go FIRST: torch's host allocator records an event on every stream a
        # pinned block was used on when the block is freed - on a stream that has already been destroyed that is a
        # segfault (seen here).  (Rebinding the names also clears the cells the closures above hold.)
        host = stage = rgb = offs = None
        torch.cuda.synchronize()
        L.lib().acrmi_stream_destroy(raw)
    pre_bytes = B * (frame_bytes + 512 * 512 * 3)
    stages = {'h2d': B / dt_h2d, 'preprocess': B / (pre_ms * 1e-3), 'network': B / dt_net}
    return {'value': round(B * steps / dt, 2), 'unit': 'frames/s', 'ms_per_step': round(dt / steps * 1e3, 3),
            'frames_per_gpu': B, 'frame': '%dx%d BGR uint8 (%.2f MB), pinned host memory' % (W, H, frame_bytes / 1e6),
            'h2d_gb_per_s': round(B * frame_bytes / dt_h2d / 1e9, 2), 'h2d_ms_per_batch': round(dt_h2d * 1e3, 3),
            'preprocess_ms_per_frame': round(pre_ms / B, 4), 'preprocess_ms_per_batch': round(pre_ms, 3),
            'preprocess_roofline': {'bound': 'hbm', 'achieved': round(pre_bytes / (pre_ms * 1e-3) / 1e9, 1), 'peak': 8000.0,
                                    'unit': 'GB/s', 'frac': round(pre_bytes / (pre_ms * 1e-3) / 1e9 / 8000.0, 4),
                                    'algorithmic_bytes_per_frame': frame_bytes + 512 * 512 * 3},
            'network_fps_resident_frames': round(B / dt_net, 2),
            'stage_fps_alone': {k: round(v, 1) for k, v in stages.items()},
            'bound_by': min(stages, key=stages.get),
            'pipeline': 'H2D (copy stream, 2 staging buffers) || preprocess + forward (2 contexts in turn); fp32 HRNet-W32',
            'pcie_inclusive': True}


def other_configs(tables, steps, warmup, local_rank):
    """The per-GPU workloads of the BASELINE.json configs the headline does not cover, each on its own synthetic checkpoint,
    two contexts in turn like the headline: configs[1] (batch 32, ResNet-50, "bf16") and configs[4] (batch 64 per GPU,
    HRNet-W48, "fp16", fp16 MANO LBS).  Neither network exists in the reference (its only backbone is HRNet-W32 and
    `--backbone resnet50` is a dead flag, acr/config.py:95): both are build-defined (schema.py) and checked against the
    build's own oracle (tests/test_gpu_h16.py); `parity` quotes metres against the SAME checkpoint run as an fp32 program.
    The REPORTED entry of each config is the program that does its arithmetic in the named 16-bit type AND stays at the
    1e-4 m bar with no decision differing: the split-operand programs (fp32 tensors in HBM, bf16 / f16 operand halves on the
    16-bit matrix pipe, csrc/conv_x3.inc).  The 16-bit STORAGE programs (activations rounded once per layer: 25 mm with 6 of 16
    decisions differing for configs[1], 2.2 mm for configs[4]) are an `ablation`, not a result."""
    synth = pkg('synth')
    res = {'ablation_16bit_storage': {}}
    for name, width, prec, B, mano16, primary in (
            ('configs[1] resnet50 batch32: bf16x3 (bf16 ARITHMETIC on fp32 tensors: split operands, csrc/conv_x3.inc)', 'resnet50', 'bf16x3', 32, False, True),
            ('configs[4] hrnet_w48 batch64 fp16-mano: fp16x3 (f16 ARITHMETIC on fp32 tensors: split operands, csrc/conv_x3.inc)', 48, 'fp16x3', 64, True, True),
            ('configs[1] resnet50 bf16 STORAGE batch32', 'resnet50', 'bf16', 32, False, False),
            ('configs[4] hrnet_w48 fp16 STORAGE batch64 fp16-mano', 48, 'fp16', 64, True, False)):
        try:
            r = _other_config(synth, tables, steps, warmup, local_rank, width, prec, B, mano16)
        except Exception as exc:      # (one of the side configurations failing must not cost the headline line)
            r = {'error': repr(exc)}
        if primary:
            res[name] = r
        else:
            res['ablation_16bit_storage'][name] = r
    return res


def _other_config(synth, tables, steps, warmup, local_rank, width, prec, B, mano16):
    sd = synth.make_state_dict(seed=0, width=width)
    frames = torch.from_numpy(synth.make_frames(B, seed=0, structured=False)).cuda()
    pool = pkg('engine').EnginePool(local_rank, n=2)
    try:
        pool.load_state_dict(sd, max_batch=B, lanes=1, precision=prec)
        pool.load_mano(tables)
        pool.configure(lambda e: e.set_mano_fp16(mano16))
        vsets = [pkg('parallel').alloc_result(B, pool.device)[1] for _ in range(2)]

        def run(n):
            pend = []
            for i in range(n):
                pend.append(pool.submit(frames, out=vsets[i % 2]))
                while len(pend) > 1:
                    pool.collect(pend.pop(0))
            for t in pend:
                pool.collect(t)
        run(max(1, warmup))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        gflop = sum(i['flops'] for i in pool.engines[0].program['op_info'] if i.get('mode', 0) != pkg('_lib').MODE_POINT) / 1e9
        kernels = {}
        for i in pool.engines[0].program['op_info']:
            if i.get('kernel') and i.get('mode', 0) != pkg('_lib').MODE_POINT:
                kernels[i['kernel']] = kernels.get(i['kernel'], 0) + 1
        # what the program costs in metres: the same checkpoint as an fp32 program of this library on 8 structured frames (no
        # reference network exists for these backbones, so the fp32 program - whose kernels and lowering are the
        # reference-pinned ones - is the yardstick; tests/test_gpu_h16.py checks both against the build's own oracle)
        L = pkg('_lib')
        pf = torch.from_numpy(synth.make_frames(8, seed=3)).cuda()
        o16 = pool.engines[0].forward(pf)
        torch.cuda.synchronize()
        o16 = {k: v.cpu().numpy() for k, v in o16.items()}
    finally:
        pool.close()
    e32 = pkg('engine').Engine(local_rank)
    try:
        e32.load_state_dict(sd, max_batch=8, precision='fp32')
        e32.load_mano(tables)
        o32 = {k: v.cpu().numpy() for k, v in e32.forward(pf).items()}
    finally:
        e32.close()
    f16, f32_ = o16['slots'][..., L.SLOT_FLAG] > 0.5, o32['slots'][..., L.SLOT_FLAG] > 0.5
    same = (f16 == f32_) & (~f32_ | (o16['slots'][..., L.SLOT_FLATIND] == o32['slots'][..., L.SLOT_FLATIND]))
    use = same & f32_
    dv = np.linalg.norm(o16['verts'] - o32['verts'], axis=-1)[use]
    worst = float(dv.max()) if dv.size else None
    return {'value': round(B * steps / dt, 2), 'unit': 'frames/s', 'ms_per_step': round(dt / steps * 1e3, 3),
            'precision': prec, 'mano_fp16_lbs': bool(mano16), 'conv_launches_by_kernel': kernels,
            'gflop_per_frame': round(gflop, 1), 'tflops': round(B * steps * gflop / dt / 1e3, 1),
            'gflop_per_frame_source': 'sum of the lowered program\'s algorithmic conv / pooling FLOPs (packer op_info), dense heads',
            'parity': {'max_vertex_l2_m': worst, 'hands_compared': int(use.sum()),
                       'decisions_differing': int((~same).sum()), 'frames': 8,
                       'within_1e-4_m_and_no_decision_differing': bool(worst is not None and worst < 1e-4 and not (~same).any()),
                       'against': 'the SAME checkpoint as an fp32 program of this library (no reference network exists for '
                                  'this backbone); per-op parity of both vs the build\'s own oracle: tests/test_gpu_h16.py'}}


def live_pmc(batch, timeout_s=300, precision='fp32'):
    """the PMC figures of the bench line measured in THIS run instead of read from profiles/ - bench.py
    re-executes itself (one warm-up + one step, one context, one stream) under `rocprofv3 --kernel-trace --pmc ...`, in
    two passes because FETCH_SIZE and WRITE_SIZE do not fit the TCC's counter slots together (MI355X_MICROARCH.md); no
    other trace domain is enabled.  gfx950 correction: FETCH_SIZE x 2 (wide coalesced reads are reported at half),
    WRITE_SIZE as is, both in KiB.  Returns None when rocprofv3 is absent or a pass fails (the caller falls back to the
    committed profiles/ files and says so)."""
    import csv
    import glob
    import re
    import shutil
    import subprocess
    import tempfile
    from collections import defaultdict
    exe = shutil.which('rocprofv3')
    if not exe:
        return None
    passes = [('fetch', ['FETCH_SIZE', 'SQ_BUSY_CU_CYCLES', 'SQ_VALU_MFMA_BUSY_CYCLES']), ('write', ['WRITE_SIZE'])]
    tot = defaultdict(lambda: defaultdict(float))
    cnt = defaultdict(lambda: defaultdict(set))
    tmp = tempfile.mkdtemp(prefix='acrmi_pmc_', dir='/tmp')
    env = dict(os.environ, TMPDIR='/tmp')
    try:
        for tag, counters in passes:
            out = os.path.join(tmp, tag)
            cmd = [exe, '--output-format', 'csv', '--kernel-trace', '--pmc'] + counters + ['-d', out, '-o', 'p', '--', sys.executable,
                   os.path.join(ROOT, 'bench.py'), '--pmc-child', '--batch', str(batch), '--precision', precision]
            r = subprocess.run(cmd, cwd='/tmp', env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=timeout_s)
            if r.returncode != 0:
                return None
            files = glob.glob(os.path.join(out, '**', '*counter_collection.csv'), recursive=True)
            if not files:
                return None
            for path in files:
                with open(path) as f:
                    for row in csv.DictReader(f):
                        name = re.sub(r'\(.*$', '', re.sub(r'^void ', '', row['Kernel_Name'])).replace('acrmi::', '')
                        tot[name][row['Counter_Name']] += float(row['Counter_Value'])
                        cnt[name][row['Counter_Name']].add(row['Dispatch_Id'])
    except Exception:
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    fam = defaultdict(lambda: {'fetch': 0.0, 'write': 0.0, 'launches': 0})
    variants, wsum = {}, defaultdict(lambda: [0.0, 0.0])
    for name, c in tot.items():
        if 'conv_' not in name:
            continue
        base = re.sub(r'<.*', '', name)
        n = len(cnt[name].get('FETCH_SIZE', ())) or len(cnt[name].get('WRITE_SIZE', ()))
        fam[base]['fetch'] += 2.0 * 1024.0 * c.get('FETCH_SIZE', 0.0)
        fam[base]['write'] += 1024.0 * c.get('WRITE_SIZE', 0.0)
        fam[base]['launches'] += n
        busy, mfma = c.get('SQ_BUSY_CU_CYCLES', 0.0), c.get('SQ_VALU_MFMA_BUSY_CYCLES', 0.0)
        if busy >= 1e8:
            variants[name] = {'launches': n, 'mfma_busy_frac': round(mfma / (4 * busy), 4)}
            for k in ('conv_wino' if 'wino' in name else 'conv_direct', 'all_convs'):
                wsum[k][0] += mfma
                wsum[k][1] += 4 * busy
    traffic = {k: {'launches_profiled': v['launches'], 'hbm_bytes_per_launch': round((v['fetch'] + v['write']) / max(1, v['launches'])),
                   'fetch_bytes_per_launch': round(v['fetch'] / max(1, v['launches'])),
                   'write_bytes_per_launch': round(v['write'] / max(1, v['launches']))} for k, v in fam.items()}
    return {'traffic': traffic,
            'mfma_busy': {'definition': 'SQ_VALU_MFMA_BUSY_CYCLES / (4 SIMDs x SQ_BUSY_CU_CYCLES), summed over launches',
                          'cycle_weighted': {k: round(v[0] / v[1], 4) for k, v in wsum.items() if v[1]}, 'variants': variants},
            'source': 'measured in this run: rocprofv3 --kernel-trace --pmc (2 passes) on `bench.py --pmc-child` (1 warm-up + 1 '
                      'step, batch %d, one context, one stream); FETCH_SIZE x 2 (gfx950), WRITE_SIZE exact' % batch}


def pmc_child(batch, precision='fp32'):
    """The workload live_pmc() profiles: the fp32 headline program, one warm-up + one step on one stream."""
    synth = pkg('synth')
    tables = synth.make_mano_tables(seed=1)
    tables['left']['shapedirs'] = tables['left']['shapedirs'].copy()
    tables['left']['shapedirs'][:, 0, :] *= -1
    eng = pkg('engine').Engine(0)
    eng.load_state_dict(synth.make_state_dict(seed=0), max_batch=batch, precision=precision)
    eng.load_mano(tables)
    eng.set_lanes(1)
    frames = torch.from_numpy(synth.make_frames(batch, seed=0, structured=False)).cuda()
    views = pkg('parallel').alloc_result(batch, eng.device)[1]
    for _ in range(2):
        eng.forward(frames, out=views)
    torch.cuda.synchronize()


def latency(eng, frames, views_for, batches=(1, 8), iters=20):
    """Per-call latency at the batch sizes the reference is actually called with (acr/main.py:126-141 runs batch 1)."""
    out = {}
    for b in batches:
        x = frames[:b].contiguous()
        v = views_for(b)
        # lane count / assignment by measurement in this process (Engine.tune_lanes; what acr.model.ACR does at load time)
        (lanes, planned), _ = eng.tune_lanes(b, candidates=(1, 2, 3, 4))
        out['batch%d_lanes' % b] = '%d %s' % (lanes, 'planned from measured op times' if planned else 'structural')
        for _ in range(3):
            eng.forward(x, out=v)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            eng.forward(x, out=v)
        torch.cuda.synchronize()
        out['batch%d_ms' % b] = round((time.perf_counter() - t0) / iters * 1e3, 3)
    return out


def point_heads_rate(set_point_heads, run_steps, B, steps, warmup):
    """Reported NEXT TO the headline, never as it: the same frames -> slots/verts/joints with the
    params/cam/prior head towers evaluated only at the pixels the decode samples (ACRMI_OPT_POINT_HEADS).  The dense
    head maps are not produced in this mode, so `value` above stays the full path."""
    set_point_heads(True)
    try:
        run_steps(max(1, warmup))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_steps(steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    finally:
        set_point_heads(False)
    return {'value': round(B * steps / dt, 2), 'unit': 'frames/s', 'ms_per_step': round(dt / steps * 1e3, 3),
            'note': 'head towers at decoded centers only; same slots/verts/joints within fp32 round-off; '
                    'dense params/prior maps not produced'}


def run_pipelined(n, frames, eng=None, pool=None, runner=None, vsets=None):
    """n steps of the bench's step loop; returns what the last step produced.
      * one context, no pool: eng.forward back to back on the current stream;
      * a pool of contexts (engine.EnginePool): batches submitted in turn, len(pool) - 1 tickets left outstanding behind a
        submit - batch k's tail overlaps batch k+1's head;
      * a ShardedRunner (N > 1): submit queues forward + all-gather of this rank's shard, ONE ticket stays outstanding so
        that batch k's gather overlaps batch k+1's backbone (the runner double-buffers its results: a third outstanding
        ticket would overwrite batch k).
    Module level so that tests/test_parallel_gloo.py can drive the N > 1 loop over gloo with CPU stand-ins."""
    last = None
    if runner is None and pool is None:
        for _ in range(n):
            last = eng.forward(frames, out=vsets[0])
        return last
    pending = []
    depth = 1 if runner is not None else len(pool) - 1     # tickets left outstanding behind a submit
    for i in range(n):
        if runner is not None:
            pending.append((runner, runner.submit(frames)))
        else:
            pending.append((pool, pool.submit(frames, out=vsets[i % len(vsets)])))
        while len(pending) > depth:
            who, t = pending.pop(0)
            last = who.collect(t)
    for who, t in pending:
        last = who.collect(t)
    return last


def multi_gpu_diagnostics(dist, runner, eng, last, B, world, rank, dt_own, steps, cdev, frames_for_rank=None):
    """Collective (every rank calls it, behind the timed region).  Returns on rank 0:
      per_rank_ms_per_step: each rank's own K steps / K, before the closing barrier (a slow GPU / a rank starved of host cores
        shows here; `ms_per_step` of the line is the MAX over ranks incl. the barrier);
      gather_ms: one all-gather of a B-frame shard by itself on the gather stream (hidden behind the next batch in the loop);
      ranks_seen: rank blocks in the last gathered result; ranks_verified: blocks that are BIT-EQUAL to what rank 0 computes
        for that rank's frames (seed = rank) on its own GPU - a wrong-order or stale gather cannot hide."""
    synth = pkg('synth')
    own = torch.tensor([dt_own / steps * 1e3], dtype=torch.float64, device=cdev)
    per = [torch.zeros_like(own) for _ in range(world)]
    dist.all_gather(per, own)
    gather_ms = runner.time_gather(B) if runner is not None else None
    if rank != 0:
        return None
    rows = int(last['slots'].shape[0]) if last is not None else 0
    verified = 0
    if last is not None and rows == world * B:
        for r in range(world):
            f = frames_for_rank(r) if frames_for_rank else torch.from_numpy(synth.make_frames(B, seed=r, structured=False)).to(eng.device)
            want = eng.forward(f)
            if eng.device.type == 'cuda':
                torch.cuda.synchronize()
            verified += int(all(torch.equal(last[k][r * B:(r + 1) * B], want[k]) for k in ('slots', 'verts', 'joints')))
    return {'ranks': world, 'ranks_seen': rows // B if B else 0, 'ranks_verified': verified,
            'per_rank_ms_per_step': [round(float(p.item()), 3) for p in per],
            'gather_ms': round(gather_ms, 4) if gather_ms is not None else None,
            'gather_bytes_per_rank': B * 2 * pkg('parallel').PER_HAND * 4,
            'transport': runner.transport if runner is not None else None,
            'note': 'per_rank = each rank\'s own K steps before the closing barrier; gather_ms = the all-gather alone (hidden behind '
                    'the next batch in the step loop); ranks_verified = gathered blocks bit-equal to rank 0\'s recomputation'}


def self_launch(n_gpus, argv):
    """`python bench.py --gpus N` without a launcher around it (WORLD_SIZE unset): re-executes this file under
    torch.distributed.run with one rank per GPU on 127.0.0.1 and a free port (the reference's counterpart is the
    single-process nn.DataParallel of acr/main.py:61).  Rank 0's JSON line stays the last line of stdout: the children
    inherit it.  Returns the launcher's exit code."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(('127.0.0.1', 0))
        port = so.getsockname()[1]
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')        # dmabuf IPC (RCCL between processes)
    env.setdefault('OMP_NUM_THREADS', '4')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n_gpus),
           '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + list(argv)
    return subprocess.call(cmd, env=env)


class StandInEngine(object):
    """CPU stand-in for engine.Engine behind `--standin` (tests/test_parallel_gloo.py: `bench.py --gpus 2` end to end over
    gloo on a box without GPUs).  NOT a model and not the oracle: slots / verts / joints are cheap deterministic
    functions of the frame bytes, enough to check that every rank ends with every rank's rows in frame order.  The line a
    stand-in run prints says so in `metric` and `data`; it is never a measurement."""
    device = torch.device('cpu')
    comm_ranks = 0

    @staticmethod
    def fill(frames, out):
        f = frames.reshape(frames.shape[0], -1).to(torch.float32)
        key = torch.stack([f.mean(1), f[:, ::4099].sum(1) / 1e3], 1)          # [n, 2]
        out['slots'].copy_(key[:, :, None].expand(-1, -1, out['slots'].shape[2]))
        out['verts'].copy_((key[:, :, None, None] + torch.arange(778.)[None, None, :, None] * 1e-3).expand(-1, -1, -1, 3))
        out['joints'].copy_((key[:, :, None, None] - torch.arange(21.)[None, None, :, None] * 1e-3).expand(-1, -1, -1, 3))

    def forward(self, frames, out=None):
        if out is None:
            out = pkg('parallel').alloc_result(frames.shape[0], self.device)[1]
        self.fill(frames, out)
        return out


def standin_main(args, rank, world):
    """bench.py's N > 1 wiring (process group, ShardedRunner, run_pipelined, barriers, MAX over ranks, one JSON line on rank
    0) with StandInEngine on the CPU over gloo."""
    import torch.distributed as dist
    parallel, synth = pkg('parallel'), pkg('synth')
    use_dist = world > 1
    if use_dist:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group('gloo')
    B = args.batch
    frames = torch.from_numpy(synth.make_frames(B, seed=rank, structured=False))
    eng = StandInEngine()
    vsets = [parallel.alloc_result(B, eng.device)[1]]
    runner = parallel.ShardedRunner(lambda f, v: eng.forward(f, out=v), eng.device) if use_dist else None
    run_pipelined(args.warmup, frames, eng=eng, runner=runner, vsets=vsets)
    if use_dist:
        dist.barrier()
    t0 = time.perf_counter()
    last = run_pipelined(args.steps, frames, eng=eng, runner=runner, vsets=vsets)
    if use_dist:
        dist.barrier()
    dt = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(last, args.dump_outputs)
    ok = True
    multi = None
    if use_dist:
        t = torch.tensor([dt], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()
        if args.full:
            multi = multi_gpu_diagnostics(dist, runner, eng, last, B, world, rank, dt, args.steps, 'cpu',
                                          frames_for_rank=lambda r: torch.from_numpy(synth.make_frames(B, seed=r, structured=False)))
        # every rank holds every rank's rows, in frame order
        for r in range(world):
            want = parallel.alloc_result(B, eng.device)[1]
            StandInEngine.fill(torch.from_numpy(synth.make_frames(B, seed=r, structured=False)), want)
            ok = ok and all(torch.equal(last[k][r * B:(r + 1) * B], want[k]) for k in want)
        flag = torch.tensor([1 if ok else 0])
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        ok = bool(flag.item())
    if rank == 0:
        print(json.dumps({'metric': 'STAND-IN plumbing run (no GPU, no model): not a measurement', 'value': round(world * B * args.steps / dt, 2),
                          'unit': 'frames/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
                          'ms_per_step': round(dt / args.steps * 1e3, 3), 'higher_is_better': True, 'scaling': 'weak',
                          'vs_baseline': None, 'dtype': 'none', 'data': 'stand-in engine on the CPU over gloo',
                          'config': {'workload': 'stand-in', 'frames_per_gpu': B, 'global_batch': B * world,
                                     'parallelism': 'frame-sharded x%d' % world,
                                     'gather': 'gloo all-gather of result slots per batch' if use_dist else 'none (one rank)'},
                          'gathered_rows_ok': ok, 'multi_gpu': multi}), flush=True)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    if not ok:
        raise SystemExit('stand-in run: gathered rows differ from what the ranks produced')


def dump_outputs(last, dirname, limit=64 << 20):
    """--dump-outputs DIR: what the timed path returned for its last step - slots [N,2,176], verts [N,2,778,3], joints
    [N,2,21,3], float32, N = every rank's frames for N > 1 (the gathered rows) - one DIR/<name>.npy each (1.3 MB at batch 64).
    Above `limit` bytes in all, the same fixed, seeded sample of frames is kept of every array (`frames.npy` = their indices).
    The inputs are seeded, so two builds run with the same arguments can be compared array for array."""
    os.makedirs(dirname, exist_ok=True)
    names = ('slots', 'verts', 'joints')
    n = int(last['slots'].shape[0])
    per_frame = sum(last[k][0].numel() * 4 for k in names) if n else 0
    rows = None
    if n * per_frame > limit:
        rows = np.sort(np.random.RandomState(0).choice(n, (limit - 4096) // (per_frame + 8), replace=False))
        np.save(os.path.join(dirname, 'frames.npy'), rows.astype(np.float64))
    for k in names:
        a = last[k].detach().cpu().numpy().astype(np.float32)
        np.save(os.path.join(dirname, k + '.npy'), a if rows is None else a[rows])


def guarded(out, key, fn):
    """A measurement leg BEHIND the timed region must not cost the headline line: a leg that raises
    leaves {'error': ...} under its key and the line is still printed."""
    try:
        v = fn()
        if v is not None:
            out[key] = v
        return v
    except Exception as exc:      # noqa: BLE001 - any failure of a secondary leg is reported, never fatal
        import traceback
        out[key] = {'error': repr(exc), 'where': traceback.format_exc(limit=3).strip().splitlines()[-3:]}
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=64, help='frames per GPU')
    ap.add_argument('--full', action='store_true', help='after the headline, also run the legs behind the timed region: roofline pass, point heads, one context, cpu_baseline + parity, latency, live PMC, reduced precision, other configs, multi-GPU diagnostics (the --no-* switches below trim them)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None, help='write what the last timed step computed (slots / verts / joints, float32) as DIR/<name>.npy')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-latency', action='store_true', help='skip the batch-1 / batch-8 latency measurement (profiling runs)')
    ap.add_argument('--no-point-heads', action='store_true', help='skip the separately reported point-heads variant')
    ap.add_argument('--no-reduced-precision', action='store_true', help='skip the separately reported fp16 / bf16 programs')
    ap.add_argument('--no-pmc', action='store_true', help='do not re-run one step under rocprofv3 --pmc; roofline.traffic / mfma_busy_pmc then come from profiles/')
    ap.add_argument('--pmc-child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--precision', default='fp32', help='fp32 = the headline (BASELINE.json configs[2]); fp16 / bf16 run the 16-bit program as the timed workload - for profiling runs (tools/profile_round.sh), NOT the headline: the line then says so in dtype / config')
    ap.add_argument('--lanes', type=int, default=0, help='HIP streams the independent chains of the program run on (ACRMI_OPT_LANES; 0 = library default, 1 per context with --pipeline >= 2)')
    ap.add_argument('--pipeline', type=int, default=2, help='contexts taking batches in turn on their own streams (engine.EnginePool): the tail of one batch overlaps the head of the next; 1 = one context')
    ap.add_argument('--profile-out', default=None, help='with --full: write the per-op HIP-event timings (JSON) of the roofline pass here')
    ap.add_argument('--leg-timeout', type=int, default=900, help='with --full: seconds the legs BEHIND the timed region (roofline pass, point heads, cpu_baseline, latency, PMC child, other configs) may take before the line is printed without the unfinished ones (0 = no watchdog)')
    ap.add_argument('--standin', action='store_true', help=argparse.SUPPRESS)     # CPU plumbing run over gloo (tests only)
    args = ap.parse_args()

    if args.pmc_child:
        pmc_child(args.batch, args.precision)
        return
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        # no launcher around this process: become the launcher (one rank per GPU), rank 0 of the children prints the line
        raise SystemExit(self_launch(args.gpus, sys.argv[1:]))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world != args.gpus:
        raise SystemExit('--gpus %d but the launcher started %d rank(s) (WORLD_SIZE): they must agree' % (args.gpus, world))
    if args.standin:
        standin_main(args, rank, world)
        return
    torch.cuda.set_device(local_rank)
    dist = None
    # ACRMI_FORCE_DIST=1 exercises the RCCL path (init, all-gather, barriers) even at world size 1 (1-GPU boxes)
    use_dist = world > 1 or os.environ.get('ACRMI_FORCE_DIST') == '1'
    if use_dist:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29517')
        os.environ.setdefault('RANK', '0')
        os.environ.setdefault('WORLD_SIZE', '1')
        import torch.distributed as dist
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        # ACRMI_GATHER=c: the data-path collective is the library's own acrmi_allgather (RCCL through the C ABI), so the process
        # group only carries the unique id, the barriers and the timing reduction - over gloo.  With backend nccl the process
        # would hold TWO RCCL communicators (torch's, created by its first collective, and the library's): measured at world
        # size 1 (tools/allgather_probe.py) a side-stream all-gather next to a running batch then costs +11.4 ms per batch
        # (46.8 vs 35.4 ms) against +0.2 ms with the library's communicator alone - what r2's "slow C transport" was.
        c_transport = os.environ.get('ACRMI_GATHER') == 'c'
        if c_transport:
            dist.init_process_group('gloo')
        else:
            dist.init_process_group('nccl', device_id=torch.device('cuda', local_rank))

    synth, parallel = pkg('synth'), pkg('parallel')
    B = args.batch
    sd = synth.make_state_dict(seed=0)
    tables = synth.make_mano_tables(seed=1)
    tables['left']['shapedirs'] = tables['left']['shapedirs'].copy()
    tables['left']['shapedirs'][:, 0, :] *= -1          # acr/mano_wrapper.py:35
    npipe = max(1, args.pipeline)
    if use_dist:
        npipe = min(npipe, 2)                   # ShardedRunner double-buffers its result sets
    eng = pkg('engine').Engine(local_rank)
    eng.load_state_dict(sd, max_batch=B, precision=args.precision)
    eng.load_mano(tables)
    eng.set_lanes(args.lanes)
    comm_late = os.environ.get('ACRMI_COMM_LATE') == '1'      # (experiment switch: communicator behind the pool's streams)
    if use_dist and os.environ.get('ACRMI_GATHER') == 'c' and not comm_late:
        # the C-ABI transport's own RCCL communicator is created BEFORE the pool's streams exist: a communicator created
        # later lands its internal stream on a hardware queue one of the contexts already uses (r2: 1367 vs 1553 frames/s)
        parallel.init_engine_comm(eng)
    frames = torch.from_numpy(synth.make_frames(B, seed=rank, structured=False)).cuda()   # resident in HBM
    pool = None
    if npipe > 1:
        # two contexts take the batches in turn, each on its own stream (engine.EnginePool): every batch is one context's
        # Engine.forward, the low-occupancy tail of batch k overlaps the head of batch k+1
        pool = pkg('engine').EnginePool(local_rank, n=npipe, first=eng)
        pool.load_state_dict(None, max_batch=B, lanes=args.lanes or 1)
        pool.load_mano(None)

    if use_dist and os.environ.get('ACRMI_GATHER') == 'c' and comm_late:
        parallel.init_engine_comm(eng)
    vsets = [parallel.alloc_result(B, eng.device)[1] for _ in range(npipe)]
    views = vsets[0]
    runner = None
    if use_dist:
        # one all-gather per batch, queued on a side stream into the second of two result buffers: batch k's gather
        # overlaps batch k+1's backbone (parallel.ShardedRunner.submit / collect); every gather of the K timed
        # steps has completed when the closing synchronize returns
        if pool is not None:
            local = lambda f, v: pool.release(pool.submit(f, out=v))      # -> the event the gather waits for
        else:
            local = lambda f, v: eng.forward(f, out=v)
        runner = parallel.ShardedRunner(local, eng.device, engine=eng)

    def run_steps(n):
        return run_pipelined(n, frames, eng=eng, pool=pool, runner=runner, vsets=vsets)

    run_steps(args.warmup)
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    last = run_steps(args.steps)
    torch.cuda.synchronize()
    dt_own = time.perf_counter() - t0          # this rank's K steps, before it waits for the others
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(last, args.dump_outputs)       # before anything behind the timed region reuses the result buffers
    multi = None
    if use_dist:
        cdev = 'cpu' if dist.get_backend() == 'gloo' else 'cuda'
        t = torch.tensor([dt], dtype=torch.float64, device=cdev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()
    if use_dist and args.full:
        # self-diagnosis of a multi-GPU run (no 8-GPU box was available to any round): every rank's own
        # step time, the all-gather by itself, and how many ranks' rows arrived - in the line, so that a first hardware SCALE
        # run that scales badly says where
        multi = multi_gpu_diagnostics(dist, runner, eng, last, B, world, rank, dt_own, args.steps, cdev)

    if rank == 0:
        ms_per_step = dt / args.steps * 1e3
        fps = world * B * args.steps / dt
        L = pkg('_lib')
        prof_box = {}

        def roofline_leg():
            # per-op HIP-event timing of the same program on the same stream (one extra pass)
            prof = [p for p in eng.profile_ops(frames) if p.get('mode', 0) != L.MODE_POINT]   # the dense program as timed
            if args.profile_out:
                with open(args.profile_out, 'w') as f:
                    json.dump(prof, f, indent=0)
            dom = [p for p in prof if p['kind'] == L.OP_CONV and p['ksize'] == 3 and p['stride'] == 1]
            dom_ms = sum(p['ms'] for p in dom)
            dom_flops = sum(p['flops'] for p in dom) * B
            # convolutions = OP_CONV + the uint8 stem + layer1's fused 1x1 pairs (OP_PAIR1X1: conv3 64->256 + residual chained with
            # the next conv1 256->64 - two convolutions in one launch; r4's line counted them as "not convolution")
            conv_kinds = (L.OP_CONV, L.OP_STEM, L.OP_PAIR1X1)
            conv_ms = sum(p['ms'] for p in prof if p['kind'] in conv_kinds)
            total_ms = sum(p['ms'] for p in prof)
            kind_names = {L.OP_FUSESUM: 'hr_fuse_sum', L.OP_BILINEAR2X: 'bilinear2x', L.OP_POW11: 'cam_pow', L.OP_ATTPOOL: 'attention_pool',
                          L.OP_PAREBIAS: 'pare_bias', L.OP_MAXPOOL: 'maxpool', L.OP_U8NORM: 'u8norm', L.OP_POINTHEADS: 'point_heads'}
            non_conv = {}
            for p in prof:
                if p['kind'] not in conv_kinds:
                    k = kind_names.get(p['kind'], 'kind%d' % p['kind'])
                    non_conv[k] = non_conv.get(k, 0.0) + p['ms']
            achieved = dom_flops / (dom_ms * 1e-3) / 1e12
            # `achieved` here counts ALGORITHMIC (direct-convolution) FLOPs; Winograd executes 2.25x (1.5x) fewer of them
            # on the matrix pipe, so this figure can exceed the MFMA peak (reported as algorithmic_* below).
            executed = sum(p['flops'] / MFMA_REDUCTION.get(p.get('algo'), 1.0) for p in dom) * B
            # HBM bytes per launch of the dominant kernel: rocprofv3 PMC passes (FETCH_SIZE x2 gfx950 correction +
            # WRITE_SIZE) of this same command, committed under profiles/ (PMC cannot be sampled from inside bench.py)
            traffic, traffic_src, busy = None, None, None
            for tag in PROFILE_TAGS:
                tpath = os.path.join(ROOT, 'profiles', '%s_hbm_traffic.json' % tag)
                if traffic is None and os.path.exists(tpath):
                    with open(tpath) as f:
                        kk = json.load(f)['kernels']
                        traffic = round((kk.get('conv_wino24b_kernel') or kk.get('conv_wino24_kernel') or kk.get('conv_wino2_kernel') or {}).get('hbm_bytes_per_launch', 0)) or None
                    traffic_src = 'profiles/%s_hbm_traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command)' % tag
                bpath = os.path.join(ROOT, 'profiles', '%s_pmc_mfma.json' % tag)
                if busy is None and os.path.exists(bpath):
                    with open(bpath) as f:
                        busy = json.load(f)
                    busy['source'] = 'profiles/%s_pmc_mfma.json' % tag
            executed_tf = executed / (dom_ms * 1e-3) / 1e12
            # `achieved`/`frac`: what the matrix pipe executes (Winograd F(2x2,3x3) runs 2.25x fewer MACs than the direct
            # form), so frac <= 1 is the share of the fp32 MFMA peak the dominant kernel's MFMAs occupy.  The contract's
            # algorithmic figure (direct-convolution FLOPs / time) is kept next to it as algorithmic_*.
            roofline = {'bound': 'mfma', 'achieved': round(executed_tf, 2), 'peak': PEAK_F32_MFMA_TFLOPS, 'unit': 'TFLOP/s',
                        'frac': round(executed_tf / PEAK_F32_MFMA_TFLOPS, 4),
                        'frac_definition': 'EXECUTED fp32 MFMA FLOP of the dominant kernels / launch time / peak (Winograd F(2x4,3x3) / '
                                           'F(2x2,3x3) execute 3x / 2.25x fewer MACs than the direct form; the algorithmic 2*MAC figure is algorithmic_frac)',
                        'traffic': traffic, 'traffic_source': traffic_src,
                        'kernel': DOMINANT, 'launches_per_step': len(dom),
                        'algorithmic_achieved': round(achieved, 2),
                        'algorithmic_frac': round(achieved / PEAK_F32_MFMA_TFLOPS, 4),
                        'winograd_mac_reduction': {'f2x4_3x3': 3.0, 'f2x2_3x3': 2.25}, 'mfma_busy_pmc': busy,
                        'avg_launch_ms': round(dom_ms / max(1, len(dom)), 4),
                        'algorithmic_gflop_per_launch': round(dom_flops / max(1, len(dom)) / 1e9, 2),
                        'share_of_step_ms': round(dom_ms / total_ms, 3),
                        'whole_path_frac': round(fps / world * GFLOP_PER_FRAME * 1e9 / (PEAK_F32_MFMA_TFLOPS * 1e12), 4),
                        'all_conv_ms': round(conv_ms, 3), 'all_ops_ms': round(total_ms, 3),
                        'non_conv_ms': dict({k: round(v, 3) for k, v in sorted(non_conv.items())}, total=round(total_ms - conv_ms, 3),
                                            note='single-stream HIP-event times of the ops that are not convolutions (decode + MANO run '
                                                 'behind the program: ~0.18 ms more)')}
            prof_box['prof'] = prof
            return roofline

        out = {'metric': 'frames/sec (2-hand mesh) at 512x512 batch-64; vertex L2 vs ref', 'value': round(fps, 2),
               'unit': 'frames/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
               'ms_per_step': round(ms_per_step, 3), 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
               'dtype': {'fp32': 'f32', 'fp16': 'f16 storage / f32 accumulate (NOT the headline precision)', 'bf16': 'bf16 storage / f32 accumulate (NOT the headline precision)',
                         'fp16x3': 'f32 storage, split f16 operands x3 on the 16-bit matrix pipe / f32 accumulate (NOT the headline arithmetic)',
                         'bf16x3': 'f32 storage, split bf16 operands x3 on the 16-bit matrix pipe / f32 accumulate (NOT the headline arithmetic)'}[args.precision], 'data': 'synthetic (seeded random uint8 frames, synthetic checkpoint + MANO tables)',
               'config': {'workload': 'configs[2]: synthetic 512x512 RGB batch=64 per GPU, HRNet-W32 backbone, %s' % args.precision,
                          'frames_per_gpu': B, 'global_batch': B * world, 'parallelism': 'frame-sharded x%d' % world,
                          'gather': (('rccl all-gather of result slots per batch, transport ' + runner.transport) if runner is not None else 'none (one rank)'),
                          'contexts_in_turn': npipe,
                          'gflop_per_frame': GFLOP_PER_FRAME},
               'roofline': None}
        if multi is not None:
            out['multi_gpu'] = multi
        if args.full:
            # Watchdog: a leg behind the timed region that HANGS (a GPU fault inside a library call never returns to Python, so
            # guarded() cannot catch it) must not cost the measured headline either: after --leg-timeout seconds a daemon thread
            # prints the line as far as it got - `post_timeout` says so - and ends the process.  Disarmed when the legs are done.
            import threading

            def _give_up():
                out['post_timeout'] = ('a measurement leg behind the timed region did not return within %d s; the line holds what '
                                       'was finished until then' % args.leg_timeout)
                try:
                    sys.stdout.write(json.dumps(out, default=str) + '\n')
                    sys.stdout.flush()
                finally:
                    os._exit(0)
            watchdog = threading.Timer(args.leg_timeout, _give_up)
            watchdog.daemon = True
            if world == 1 and args.leg_timeout > 0:
                watchdog.start()
            guarded(out, 'roofline', roofline_leg)
            prof = prof_box.get('prof', [])
            if isinstance(out.get('roofline'), dict) and 'error' not in out['roofline']:
                # the contract's figure at top level (VERDICT r5 item 4 iii): whole-path ALGORITHMIC flop rate / the fp32 matrix peak
                out['roofline']['contract_frac'] = out['roofline']['whole_path_frac']
                out['roofline']['contract_frac_definition'] = (
                    'frames/s x %.1f algorithmic GFLOP per frame (SURVEY.md 8d: 2*MAC of the direct form) / %.1f TFLOP/s; above the '
                    'executed `frac` by the Winograd / polyphase MAC reduction, not by skipped work' % (GFLOP_PER_FRAME, PEAK_F32_MFMA_TFLOPS))
            single = world == 1 and not use_dist
            state = {'pool': pool, 'oracle': None}

            def close_pool():
                # everything behind the headline runs single calls on `eng` with the library's lanes: the lane streams must be created
                # AFTER the pool's streams are gone - lanes created while other streams are alive share hardware queues with them
                # (8-10 ms per batch-1 call instead of 3.5; DESIGN.md section 2 "Parallel lanes")
                if state['pool'] is not None:
                    state['pool'].close(keep_first=True)
                    state['pool'] = None

            if world == 1 and not args.no_point_heads and args.precision == 'fp32':
                def point_leg():
                    pl = state['pool']
                    setter = (lambda on: pl.configure(lambda e: e.set_point_heads(on))) if pl is not None else eng.set_point_heads
                    return point_heads_rate(setter, run_steps, B, args.steps, args.warmup)       # (switches the mode back itself)
                guarded(out, 'point_heads', point_leg)
            if single and pool is not None and not args.no_latency:
                def single_leg():
                    # the same K batches on ONE context with the library's lanes (what `value` was before round 2's EnginePool)
                    eng.set_lanes(args.lanes)
                    for _ in range(args.warmup):
                        eng.forward(frames, out=views)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    for _ in range(args.steps):
                        eng.forward(frames, out=views)
                    torch.cuda.synchronize()
                    dt1 = time.perf_counter() - t1
                    return {'value': round(B * args.steps / dt1, 2), 'unit': 'frames/s', 'ms_per_step': round(dt1 / args.steps * 1e3, 3),
                            'note': 'one context, batches back to back on one stream (+ its parallel lanes)'}
                guarded(out, 'single_context', single_leg)
            if single:
                guarded(out, 'pool_close', close_pool)
            if world == 1 and not args.no_cpu_baseline:
                def cpu_leg():
                    state['oracle'], res = cpu_baseline(sd, tables)
                    return res
                guarded(out, 'cpu_baseline', cpu_leg)
                if state['oracle'] is not None:
                    # the headline program (large-batch lowering) on the sample's 8 frames
                    guarded(out, 'parity', lambda: parity(eng, state['oracle']))
            if single and not args.no_latency:
                def latency_leg():
                    # single calls (the way the reference is driven, acr/main.py:126-141: one frame per call), on a context built
                    # for small batches as acr.model.ACR builds it (max_batch <= 8: the packer keeps F(2x2,3x3) for every 3x3
                    # layer).  Measured with every other context and stream of this process gone and BEFORE the later sections
                    # create theirs: lane streams that are created while other streams are alive share hardware queues with them
                    # (9.9 instead of 3.5 ms per batch-1 call with the throughput context still alive; 8 ms with torch's stream
                    # pool alive - DESIGN.md section 2).  The SAME context is re-programmed rather than a new one created: a
                    # context created this late gets lane streams that share hardware queues
                    eng.load_state_dict(sd, max_batch=8, precision=args.precision)
                    eng.set_lanes(0)
                    lat = latency(eng, frames, lambda b: parallel.alloc_result(b, eng.device)[1])
                    lat['context'] = 'max_batch 8 (small-batch lowering: F(2x2,3x3) only)'
                    lat['program_ops_per_call'] = sum(1 for o in eng.program['ops'] if o.mode != 2 and o.kind != 8)
                    lat['launches_note'] = 'one launch per op except attention pooling (3); + decode (1) + MANO (1 per side)'
                    return lat
                guarded(out, 'latency', latency_leg)
                guarded(out, 'engine_close', eng.close)
            if single and not args.no_pmc and args.precision == 'fp32' and isinstance(out.get('roofline'), dict) and 'error' not in out['roofline']:
                def pmc_leg():
                    # counters of THIS box, THIS run (the committed profiles/ figures stay as the fallback, labelled as such)
                    live = live_pmc(B)
                    if live is None:
                        out['roofline']['traffic_source'] = 'committed: ' + str(out['roofline']['traffic_source'])
                        return None
                    fam = {k: v for k, v in live['traffic'].items() if 'wino' in k}
                    top = max(fam, key=lambda k: fam[k]['launches_profiled']) if fam else None      # the family's most-launched kernel
                    t2 = fam[top]['hbm_bytes_per_launch'] if top else None
                    out['roofline']['traffic_kernel'] = top
                    out['roofline']['traffic'] = t2 or out['roofline']['traffic']
                    out['roofline']['traffic_source'] = live['source'] if t2 else out['roofline']['traffic_source']
                    # algorithmic bytes per launch of every conv family (packer: input slice + output + residual once, x frames),
                    # so that wasted re-reads are a printed ratio, not an inference
                    alg = {}
                    for p in prof:
                        if p['kind'] == L.OP_CONV and p.get('kernel'):
                            a = alg.setdefault(p['kernel'], [0.0, 0])
                            a[0] += p['bytes'] * B
                            a[1] += 1
                    for k, v in live['traffic'].items():
                        if k in alg and alg[k][1]:
                            v['algorithmic_bytes_per_launch'] = round(alg[k][0] / alg[k][1])
                            v['launches_per_step'] = alg[k][1]
                            v['traffic_over_algorithmic'] = round(v['hbm_bytes_per_launch'] / max(1.0, alg[k][0] / alg[k][1]), 3)
                    out['roofline']['traffic_per_kernel'] = live['traffic']
                    out['roofline']['traffic_per_kernel_note'] = (
                        'algorithmic_bytes_per_launch / traffic_over_algorithmic attribute ops to kernel families as the packer predicts '
                        'launch_conv routes them at batch 64 on 256 CUs (packer op_info kernel); at another --batch only the '
                        'measured hbm_bytes_per_launch columns are exact' if B == 64 else
                        'batch %d: the op -> kernel attribution behind algorithmic_bytes_per_launch assumes batch 64' % B)
                    out['roofline']['mfma_busy_pmc'] = dict(live['mfma_busy'], source=live['source'])
                    return None
                guarded(out, 'pmc_leg', pmc_leg)
            if single and not args.no_reduced_precision and args.precision == 'fp32':
                guarded(out, 'reduced_precision', lambda: reduced_precision(sd, tables, frames, B, args.steps, args.warmup, state['oracle'], local_rank))
                guarded(out, 'other_configs', lambda: other_configs(tables, args.steps, args.warmup, local_rank))
                if not isinstance(out.get('other_configs'), dict):
                    out['other_configs'] = {}
                # (a host that cannot pin 200 MB must not cost the headline line)
                guarded(out['other_configs'], 'configs[3] 1080p stream, per-GPU shard (32 frames), host memory -> meshes',
                        lambda: config3_video_stream(sd, tables, args.steps, args.warmup, local_rank))
            pool = state['pool']
            watchdog.cancel()
        elif world == 1 and not use_dist:
            # the contexts and their streams go before the interpreter does, as after the legs of --full
            if pool is not None:
                pool.close(keep_first=True)
            eng.close()
        line = json.dumps(out)
    else:
        line = None
    if runner is not None:
        runner.close()             # the library stream the gathers ran on
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    if line is not None:
        try:        # RCCL buffers a version banner in C stdio; push it out before the JSON so the JSON is last
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        sys.stdout.flush()
        print(line, flush=True)      # last line of stdout, after RCCL's own chatter


if __name__ == '__main__':
    main()
