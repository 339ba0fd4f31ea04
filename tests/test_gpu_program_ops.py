"""Every op of the benchmarked programs, at the batches bench.py runs them, against the op-list interpreter.

The kernel that runs an op is chosen from the call's batch and the CU count (conv_mfma.hip launch_conv: conv_wino2's
`few`, the direct kernel's `fine`, conv_p1 only with >= 2 x CUs items; persistent kernels walk items vb, vb + grid, ...
only past 256 workgroups; the XCD-banded item order only when grid % 8 == 0), so the per-op checks at batch 1-3 do not
speak for the launches the benchmark times.  Here each program is lowered as production lowers it (Engine.load_state_dict
with the context's max_batch) but with keep_all=True, one call runs at the benchmarked batch, a few frames of every
buffer are copied back, and oracle.program.check_program re-evaluates every dense op on the GPU's own inputs: each
element within its per-element bound, every channel no op writes still 0.0.  The measured worst ratios per tolerance
class land in per_op_report.json, next to the reports of the other GPU tests.  `pytest -m gpu`."""
import json
import os
import time

import pytest
import torch

import test_gpu_hardening
from conftest import pkg
from oracle import program as oprog

pytestmark = pytest.mark.gpu
REPORT = os.path.join(os.path.dirname(test_gpu_hardening.REPORT), 'per_op_report.json')

# (id, width, precision, checkpoint law, context max_batch, lanes, [(call batch, checked frames)], minimum ops checked)
MATRIX = [
    ('w32_fp32_headline', 32, 'fp32', 'benign', 64, 1, [(64, [0, 31, 63]), (37, [0, 36])], 312),
    ('w32_fp32_headline_hostile', 32, 'fp32', 'hostile', 64, 1, [(64, [0, 63])], 312),
    ('w32_fp32_small_batch', 32, 'fp32', 'benign', 8, None, [(8, [0, 7]), (1, [0])], 322),
    ('w32_fp16x3', 32, 'fp16x3', 'benign', 64, 1, [(64, [0, 63])], 320),
    ('w32_fp16x3_hostile', 32, 'fp16x3', 'hostile', 64, 1, [(64, [0, 63])], 320),
    ('w32_bf16x3', 32, 'bf16x3', 'benign', 64, 1, [(64, [0, 63])], 320),
    ('configs4_w48_fp16x3', 48, 'fp16x3', 'benign', 64, 1, [(64, [0, 63])], 320),
    ('configs1_resnet50_bf16x3', 'resnet50', 'bf16x3', 'benign', 32, 1, [(32, [0, 31])], 82),
]


def _report(key, value):
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    data = {}
    if os.path.exists(REPORT):
        with open(REPORT) as f:
            data = json.load(f)
    data[key] = value
    with open(REPORT, 'w') as f:
        json.dump(data, f, indent=1, sort_keys=True)


@pytest.mark.parametrize('case', MATRIX, ids=lambda c: c[0])
def test_every_op_at_the_benchmarked_batch(case):
    name, width, precision, law, max_batch, lanes, calls, min_checked = case
    torch.set_num_threads(16)
    synth = pkg('synth')
    sd = synth.make_state_dict(seed=0, width=width, law=law)
    frames = synth.make_frames(max(b for b, _ in calls), seed=0, structured=False)      # bench.py's frames
    eng = pkg('engine').Engine(0)
    eng.load_state_dict(sd, max_batch=max_batch, precision=precision, keep_weights=True, keep_all=True)
    if lanes is not None:
        eng.set_lanes(lanes)
    prog = eng.program
    failures = []
    try:
        for B, picks in calls:
            t0 = time.time()
            eng.backbone_heads(torch.from_numpy(frames[:B]).cuda())
            torch.cuda.synchronize()
            idx = torch.tensor(picks, device='cuda')
            bufs = [eng.buffer(i, B).index_select(0, idx).float().cpu() for i in range(len(prog['bufs']))]
            res = oprog.check_program(prog, bufs, torch.from_numpy(frames[picks]), frames=picks)
            worst = sorted(res['rows'], key=lambda r: -r['ratio'] / max(1.0, oprog.ELEMENT_TOL.get(r['class'], 1.0)))[:5]
            _report('%s_B%d' % (name, B), {
                'frames': picks, 'ops_checked': res['checked'], 'ops_checked_through_their_in_place_successor': res['chained'],
                'zero_checked_buffers': res['zero_checked_buffers'], 'worst_ratio_by_class': oprog.worst_by_class(res['rows']),
                'worst_rows': [{k: r[k] for k in ('op', 'class', 'kernel', 'out', 'ratio', 'where', 'rel_err')} for r in worst],
                'failures': res['failures'][:20], 'seconds': time.time() - t0})
            failures += [dict(f, batch=B) for f in res['failures']]
            assert res['checked'] >= min_checked and res['chained'] <= 8, (B, res['checked'], res['chained'])
    finally:
        eng.close()
    assert not failures, failures[:10]
