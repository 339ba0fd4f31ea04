"""GPU tests of tracking on the device (DESIGN.md "Tracking on the device"): the window kernels that read their boxes from
device memory against the host-box call, byte for byte; the box kernel against the numpy rule, integer for integer; and the
loop frame k -> boxes -> frame k+1 on an Engine, an EnginePool and ACR.track_raw_batch against the same loop written through
the host (forward, .cpu(), boxes_from_keypoints, ops.preprocess_rois).  Everything compared is integer or the output of the
same kernels on the same bytes, so every comparison is exact."""
import os
import re

import numpy as np
import pytest
import torch

import nv12_ref as N
import roi_ref as R
import track_ref as T
from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu

SIZES = [(37, 53), (64, 40), (600, 700)]      # H x W: the frames of tests/test_gpu_roi.py
# (frame, (l, t, r, b)): the integer boxes of tests/test_gpu_roi.py's CASES, and the int32 extremes
CASES = [
    (0, (10, 5, 30, 25)),
    (0, (0, 5, 20, 30)), (0, (10, 0, 30, 20)), (0, (20, 5, 53, 30)), (0, (10, 10, 40, 37)),
    (0, (-4, -6, 25, 20)), (0, (30, 20, 60, 45)), (0, (-9, 11, 99, 19)),
    (0, (52, 36, 53, 37)), (0, (7, 9, 8, 10)),
    (0, (11, 3, 12, 33)), (0, (3, 11, 33, 12)),
    (0, (20, 10, 29, 15)), (0, (20, 10, 25, 19)),
    (1, (3, 7, 38, 60)), (1, (0, 0, 40, 1)), (1, (39, 0, 40, 64)), (1, (0, 63, 17, 64)), (1, (-3, 30, 43, 41)),
    (2, (100, 50, 630, 400)), (2, (10, 30, 200, 560)),
    (2, (170, 70, 700, 600)),
    (2, (333, 222, 346, 229)),
    (0, (-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1)), (2, (-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1)),
]
# boxes that leave no pixel of the 37 x 53 frame: no width, no height, inverted, beyond each edge
NO_PIXELS = [(30, 5, 30, 30), (10, 20, 40, 20), (40, 5, 10, 30), (10, 30, 40, 5), (53, 5, 80, 30), (10, 37, 40, 60),
             (-30, 5, 0, 30), (10, -30, 40, 0), (-9, -9, -1, -1)]
NV12_CASES = {
    (16, 12): [(1, 0, 9, 8), (0, 1, 8, 9), (3, 5, 10, 14), (2, 2, 7, 5), (5, 3, 6, 4), (0, 0, 12, 16), (7, 0, 12, 16),
               (0, 9, 12, 16), (-3, -3, 5, 5), (11, 15, 12, 16)],
    (38, 54): [(1, 1, 54, 38), (13, 7, 40, 30), (0, 0, 53, 37), (21, 11, 22, 38), (17, 33, 54, 38), (30, 2, 41, 21)],
}
FH, FW = 96, 160
# The synthetic checkpoint spreads its two hands over 116 x 16 pixels of the 160 x 96 frame: at the defaults (1.5, 64) the box
# is 174 wide and every box is the whole frame again.  At scale 1.0 the boxes are (39, 0, 156, 96) after iteration 0 and differ
# between the two frames from iteration 1 on.
SCALE, MIN_SIZE = 1.0, 32
_cache = {}


def _frames():
    if 'frames' not in _cache:
        host = [np.random.default_rng(1000 * H + W).integers(0, 256, (H, W, 3), dtype=np.uint8) for H, W in SIZES]
        _cache['frames'] = (host, [torch.from_numpy(f).cuda() for f in host])
    return _cache['frames']


def _dev_boxes(boxes):
    return torch.tensor([list(b) for b in boxes], dtype=torch.int32).cuda()


def test_bgr_windows_equal_the_host_box_call_and_the_reference():
    ops = pkg('ops')
    host, dev = _frames()
    boxes, box_frame = [box for _, box in CASES], [f for f, _ in CASES]
    want, want_off = ops.preprocess_rois(dev, boxes, box_frame)
    rgb, offsets, status = ops.preprocess_rois_device(dev, _dev_boxes(boxes), box_frame)
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (len(CASES), 512, 512, 3) and rgb.is_cuda
    assert offsets.dtype == torch.float32 and tuple(offsets.shape) == (len(CASES), 10) and offsets.is_cuda
    assert status.dtype == torch.int32 and tuple(status.shape) == (len(CASES),) and status.is_cuda
    got, rows = rgb.cpu().numpy(), offsets.cpu().numpy()
    for i, (f, box) in enumerate(CASES):
        ref, row = R.preprocess(host[f], box)
        bad_host, bad_ref = int((rgb[i] != want[i]).sum()), int((got[i] != ref).sum())
        print('frame %d box %s: %d bytes differ from the host-box call, %d from the reference' % (f, box, bad_host, bad_ref))
        assert bad_host == 0 and bad_ref == 0, 'region %d (frame %d, box %s)' % (i, f, box)
        assert (rows[i] == row).all() and (rows[i] == want_off[i].numpy()).all(), (i, rows[i], row)
    assert status.cpu().tolist() == [0] * len(CASES)
    # a tensor of equal frames, one box per frame, into tensors the caller owns
    same = torch.stack([dev[0], dev[0].flip(0)])
    out = torch.zeros(2, 512, 512, 3, dtype=torch.uint8, device='cuda')
    off = torch.zeros(2, 10, device='cuda')
    st = torch.full((2,), 7, dtype=torch.int32, device='cuda')
    a, oa, sa = ops.preprocess_rois_device(same, _dev_boxes([(5, 6, 30, 31)] * 2), out=out, offsets=off, status=st)
    assert a is out and oa is off and sa is st
    b, ob = ops.preprocess_rois(same, [(5, 6, 30, 31)] * 2)
    assert torch.equal(a, b) and torch.equal(oa.cpu(), ob) and sa.cpu().tolist() == [0, 0]


def test_boxes_without_pixels_take_the_whole_frame():
    ops = pkg('ops')
    host, dev = _frames()
    good = [(0, (10, 5, 30, 25)), (1, (3, 7, 38, 60))]
    regions = [good[0]]
    for k, box in enumerate(NO_PIXELS):
        regions += [(0, box), good[(k + 1) % 2]]      # every such box between two good regions
    boxes, box_frame = [box for _, box in regions], [f for f, _ in regions]
    rgb, offsets, status = ops.preprocess_rois_device(dev, _dev_boxes(boxes), box_frame)
    whole, whole_off = ops.preprocess_frames([dev[0]])
    want_good, good_off = ops.preprocess_rois(dev, [box for _, box in good], [f for f, _ in good])
    assert (whole_off[0].numpy() == R.offsets(37, 53, (0, 0, 53, 37))).all()
    for i, (f, box) in enumerate(regions):
        if R.window(SIZES[f][0], SIZES[f][1], box) is None:
            assert torch.equal(rgb[i], whole[0]) and torch.equal(offsets[i].cpu(), whole_off[0]) and int(status[i]) == 1, (i, box)
        else:
            j = good.index((f, box))
            assert torch.equal(rgb[i], want_good[j]) and torch.equal(offsets[i].cpu(), good_off[j]) and int(status[i]) == 0, (i, box)
    assert int(status.sum()) == len(NO_PIXELS)


def test_one_region_more_than_a_launch_holds():
    ops = pkg('ops')
    src = open(os.path.join(ROOT, pkg().__name__, 'csrc', 'kernels.h')).read()
    per_launch = int(re.search(r'constexpr int ROIS_PER_LAUNCH = (\d+);', src).group(1))
    n = per_launch + 1
    g = np.random.default_rng(7)
    frames = [torch.from_numpy(g.integers(0, 256, (8, 8, 3), dtype=np.uint8)).cuda() for _ in range(5)]
    box_frame = [int(v) for v in g.integers(0, 5, n)]
    boxes = []
    for _ in range(n):
        l, t = (int(v) for v in g.integers(0, 7, 2))
        boxes.append((l, t, int(g.integers(l + 1, 9)), int(g.integers(t + 1, 9))))
    boxes[per_launch - 1] = (5, 5, 5, 5)      # and one without pixels at the end of the first launch
    host_boxes = list(boxes)
    host_boxes[per_launch - 1] = (0, 0, 8, 8)
    nv12 = [torch.from_numpy(np.concatenate(N.random_nv12(8, 8, s), 0)).cuda() for s in range(5)]
    for src_frames, kw in ((frames, {}), (nv12, dict(pixel_format='nv12'))):
        want, want_off = ops.preprocess_rois(src_frames, host_boxes, box_frame, **kw)
        rgb, offsets, status = ops.preprocess_rois_device(src_frames, _dev_boxes(boxes), box_frame, **kw)
        assert rgb.shape[0] == n and torch.equal(rgb, want) and torch.equal(offsets.cpu(), want_off)
        assert status.cpu().tolist() == [int(i == per_launch - 1) for i in range(n)]


def _pitched(plane, pitch, fill):
    buf = np.full((plane.shape[0], pitch), fill, np.uint8)
    buf[:, :plane.shape[1]] = plane
    return torch.from_numpy(buf).cuda()[:, :plane.shape[1]]


@pytest.mark.parametrize('matrix', ['cv601', 'bt709-full'])
def test_nv12_windows_equal_the_host_box_call(matrix):
    """Odd l, odd t, both odd, odd sizes, edge-touching; pitches above W with a filler that would show; both input forms."""
    ops = pkg('ops')
    for (H, W), boxes in NV12_CASES.items():
        y, uv = N.random_nv12(H, W, 1000 * H + W)
        surface = _pitched(np.concatenate([y, uv], 0), W + 10, 255)
        planes = (_pitched(y, W + 6, 255), _pitched(uv, W + 22, 255))
        n = len(boxes)
        dev_boxes = _dev_boxes(boxes)
        want, want_off = ops.preprocess_rois(surface, boxes, [0] * n, pixel_format='nv12', matrix=matrix)
        got, offsets, status = ops.preprocess_rois_device(surface, dev_boxes, [0] * n, pixel_format='nv12', matrix=matrix)
        for i, box in enumerate(boxes):
            bad = int((got[i] != want[i]).sum())
            print('%dx%d %s box %s: %d differing bytes' % (H, W, matrix, box, bad))
            assert bad == 0, 'box %s of %dx%d' % (box, H, W)
        assert torch.equal(offsets.cpu(), want_off) and status.cpu().tolist() == [0] * n
        two, off2, st2 = ops.preprocess_rois_device([planes, surface], torch.cat([dev_boxes, dev_boxes]), [0] * n + [1] * n,
                                                    pixel_format='nv12', matrix=matrix)
        assert torch.equal(two[:n], want) and torch.equal(two[n:], want) and torch.equal(off2[n:].cpu(), want_off)
        again, _, _ = ops.preprocess_rois_device(_pitched(np.concatenate([y, uv], 0), W + 10, 0), dev_boxes, [0] * n,
                                                 pixel_format='nv12', matrix=matrix)
        assert torch.equal(again, want)
    if matrix != 'cv601':
        other, _, _ = ops.preprocess_rois_device(surface, dev_boxes, [0] * n, pixel_format='nv12')
        assert not torch.equal(other, got), 'the matrix must matter'


def test_track_boxes_equal_the_numpy_rule_exactly():
    ops, S = pkg('ops'), pkg('_lib')
    n = 70
    g = np.random.default_rng(4242)
    hw = np.array([T.FRAMES[i % 3] for i in range(n)], np.int32)
    pj = np.stack([T.points(g, 42, int(H), int(W)).reshape(2, 21, 2) for H, W in hw])
    slots = g.standard_normal((n, 2, S.SLOT)).astype(np.float32)      # everything but the flag is not looked at
    sets = []
    for i in range(n):
        on = [(False, False), (True, False), (False, True), (True, True)][(i // 3) % 4]      # every combination at every frame size
        for h in (0, 1):
            slots[i, h, S.SLOT_FLAG] = 1.0 if on[h] else [0.0, 0.5, np.nan, -1.0][(i + h) % 4]      # 0.5 is not > 0.5
            if not on[h]:
                pj[i, h] = [np.nan, 3e38][(i + h) % 2]      # an unflagged hand's coordinates must not matter
        sets.append(pj[i][list(on)].reshape(-1, 2))
    pj_dev, slots_dev = torch.from_numpy(pj).cuda(), torch.from_numpy(slots).cuda()
    hw_dev = torch.from_numpy(hw).cuda()
    out = torch.zeros(n, 4, dtype=torch.int32, device='cuda')
    replaced = 0
    for scale, min_size in ((1.5, 64), (2.25, 1), (1.0, 5000)):
        want, empty = T.boxes(sets, hw, scale, min_size)
        replaced += int(empty.sum())
        got = ops.track_boxes(pj_dev, slots_dev, hw_dev, scale=scale, min_size=min_size)
        assert got.dtype == torch.int32 and tuple(got.shape) == (n, 4)
        bad = np.nonzero((got.cpu().numpy() != want).any(1))[0]
        print('scale %g min_size %d: %d of %d boxes differ, %d rows replaced' % (scale, min_size, len(bad), n, int(empty.sum())))
        assert not len(bad), [(int(i), got[i].tolist(), want[i].tolist(), sets[i].tolist()) for i in bad[:3]]
        by_list = ops.track_boxes(pj_dev, slots_dev, [tuple(int(v) for v in r) for r in hw], scale=scale, min_size=min_size, out=out)
        assert by_list is out and torch.equal(out, got)      # out= reused by every turn of the loop
    assert replaced >= 1, 'no row without pixels: the clause is not exercised'
    # one (H, W) for all regions
    for H, W in T.FRAMES:
        want, _ = T.boxes(sets, (H, W), 1.5, 64)
        assert (ops.track_boxes(pj_dev, slots_dev, (H, W)).cpu().numpy() == want).all()
    # a frame size that is not positive: (0, 0, 0, 0), which the window kernels turn into the whole frame
    hw_bad = hw_dev.clone()
    hw_bad[3, 0] = 0
    hw_bad[4, 1] = -5
    got = ops.track_boxes(pj_dev, slots_dev, hw_bad).cpu().numpy()
    want, _ = T.boxes(sets, hw, 1.5, 64)
    want[3:5] = 0
    assert (got == want).all()


@pytest.fixture(scope='module')
def near_sd():
    return pkg('synth').make_state_dict(seed=10)      # the checkpoint of tests/test_gpu_roi.py: it detects hands


def _video():
    """Two seeded 96 x 160 frames (those of tests/test_gpu_roi.py's end-to-end test) on the device."""
    if 'video' not in _cache:
        nv12 = [torch.from_numpy(np.concatenate(N.random_nv12(FH, FW, s), 0)).cuda() for s in (11, 12)]
        _cache['video'] = pkg('ops').nv12_to_bgr(nv12)
    return _cache['video']


def _flagged_points(out):
    S = pkg('_lib')
    flags = (out['slots'][:, :, S.SLOT_FLAG] > 0.5).cpu().numpy()
    pj = out['pj2d_org'].cpu().numpy()
    assert pj.dtype == np.float32
    return [pj[i][flags[i]].reshape(-1, 2) for i in range(len(pj))], flags


def _host_loop(eng, frames, iterations):
    """The loop as it is written without this feature: forward, .cpu(), boxes_from_keypoints on the fp32 pj2d_org of the
    flagged hands (a row without pixels would be the whole frame: T.boxes), ops.preprocess_rois.  Computed once."""
    if 'host_loop' not in _cache:
        ops = pkg('ops')
        boxes = np.array([[0, 0, FW, FH]] * 2, np.int32)
        steps = []
        for _ in range(iterations):
            rgb, offsets = ops.preprocess_rois(frames, boxes)
            out = eng.forward(rgb, offsets=offsets, project=True)
            sets, flags = _flagged_points(out)
            nxt, _ = T.boxes(sets, (FH, FW), SCALE, MIN_SIZE)
            steps.append(dict(boxes=boxes, rgb=rgb, out=out, flags=flags, next=nxt))
            boxes = nxt
        assert steps[0]['flags'].any(), 'no hand detected at iteration 0: the loop would show nothing'
        assert (steps[1]['boxes'] != np.array([0, 0, FW, FH])).any(), 'every box of iteration 1 is the whole frame'
        print('host loop: flags %s, boxes %s' % ([s['flags'].tolist() for s in steps], [s['next'].tolist() for s in steps]))
        _cache['host_loop'] = steps
    return _cache['host_loop']


def _same_step(k, want, boxes, rgb, out, nxt):
    assert (boxes.cpu().numpy() == want['boxes']).all(), (k, boxes.tolist(), want['boxes'].tolist())
    assert torch.equal(rgb, want['rgb']), 'iteration %d: the network inputs differ' % k
    for name in ('slots', 'pj2d_org', 'verts'):
        assert torch.equal(out[name], want['out'][name]), 'iteration %d: %s' % (k, name)
    assert (nxt.cpu().numpy() == want['next']).all(), (k, nxt.tolist(), want['next'].tolist())


def test_the_loop_without_a_host_visit(near_sd, mano_tables):
    eng = pkg('engine').Engine(0)
    eng.load_state_dict(near_sd, max_batch=2)
    eng.load_mano(mano_tables)
    frames = _video()
    want = _host_loop(eng, frames, 3)
    boxes = _dev_boxes([(0, 0, FW, FH)] * 2)
    seen = []
    torch.cuda.synchronize()
    # no synchronise between the iterations: under this mode torch raises on every call that waits for the device
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            boxes.sum().item()      # the mode is honoured by this build
        for _ in range(3):
            out, nxt, status = eng.track_step(frames, boxes, scale=SCALE, min_size=MIN_SIZE)
            seen.append((boxes, out['image'], out, nxt, status))
            boxes = nxt
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    for k, (b, rgb, out, nxt, status) in enumerate(seen):
        _same_step(k, want[k], b, rgb, out, nxt)
        assert status.cpu().tolist() == [0, 0]
    eng.close()


def test_the_pool_keeps_a_ticket_outstanding_behind_the_next_submit(near_sd, mano_tables):
    ops = pkg('ops')
    eng = pkg('engine').Engine(0)
    eng.load_state_dict(near_sd, max_batch=2)
    eng.load_mano(mano_tables)
    frames = _video()
    want = _host_loop(eng, frames, 3)
    eng.close()
    pool = pkg('engine').EnginePool(0, n=2)
    pool.load_state_dict(near_sd, max_batch=2)
    pool.load_mano(mano_tables)
    boxes = _dev_boxes([(0, 0, FW, FH)] * 2)
    seen, outs, before = [], [], None
    for k in range(3):
        rgb, offsets, _ = ops.preprocess_rois_device(frames, boxes)
        ticket = pool.submit(rgb, offsets=offsets, project=True)      # batch k is queued ...
        nxt = pool.track_boxes(ticket, (FH, FW), scale=SCALE, min_size=MIN_SIZE)
        if before is not None:
            outs.append(pool.collect(before))                         # ... before batch k - 1 has been collected
        seen.append((boxes, rgb, nxt))
        boxes, before = nxt, ticket
    with pytest.raises(RuntimeError, match='between submit'):
        pool.track_boxes({'slot': 0}, (FH, FW))
    outs.append(pool.collect(before))
    torch.cuda.synchronize()
    for k, ((b, rgb, nxt), out) in enumerate(zip(seen, outs)):
        _same_step(k, want[k], b, rgb, out, nxt)
    pool.close()


def test_track_raw_batch(near_sd, mano_tables):
    cfg, ops, utils = pkg('config'), pkg('ops'), pkg('acr.utils')
    acr = pkg('acr.main').ACR(args_set=cfg.parse_args(['--configs_yml', '/nonexistent.yml', '--renderer', 'hip']),
                              state_dict=near_sd, mano_tables=mano_tables, max_batch=3)
    frames = _video()

    def same_results(got, want):
        assert sorted(got) == sorted(want)
        for p in got:
            assert len(got[p]) == len(want[p])
            for h1, h2 in zip(got[p], want[p]):
                assert sorted(h1) == sorted(h2) and all(np.array_equal(h1[f], h2[f]) for f in h1), p

    def rule(paths, boxes, box_frame):
        meta = utils.img_preprocess_gpu(frames, paths, boxes=boxes, box_frame=box_frame)
        eng = acr.model.engine(meta['image'].shape[0])
        eng.set_point_heads(True)
        try:
            out = eng.forward(meta['image'], offsets=meta['offsets'], project=True)
        finally:
            eng.set_point_heads(False)
        sets, flags = _flagged_points(out)
        return T.boxes(sets, (FH, FW), SCALE, MIN_SIZE)[0], flags

    kw = dict(scale=SCALE, min_size=MIN_SIZE)
    whole = np.array([[0, 0, FW, FH]] * 2, np.int32)
    first, nxt = acr.track_raw_batch(frames, ['a', 'b'], **kw)      # boxes=None: the whole frames
    again, nxt2 = acr.track_raw_batch(frames, ['a', 'b'], boxes=torch.from_numpy(whole).cuda(), **kw)
    same_results(first, again)
    same_results(first, acr.forward_raw_batch(frames, ['a', 'b'], boxes=whole))
    want_next, flags = rule(['a', 'b'], whole, None)
    assert flags.any(), 'no hand detected'
    assert nxt.dtype == torch.int32 and nxt.is_cuda and (nxt.cpu().numpy() == want_next).all() and torch.equal(nxt, nxt2)
    assert (want_next != whole).any(), 'every next box is the whole frame'
    # the second frame of the video: the boxes as they came back, never seen by the host in between
    second, nxt3 = acr.track_raw_batch(frames, ['a', 'b'], boxes=nxt, **kw)
    same_results(second, acr.forward_raw_batch(frames, ['a', 'b'], boxes=want_next))
    assert (nxt3.cpu().numpy() == rule(['a', 'b'], want_next, None)[0]).all()
    # three regions of two frames, NV12 surfaces of the same pictures
    boxes = np.array([(20, 10, 121, 90), (0, 0, 101, 61), (31, 7, 160, 96)], np.int32)
    nv12 = [torch.from_numpy(np.concatenate(N.random_nv12(FH, FW, s), 0)).cuda() for s in (11, 12)]
    got, nxt4 = acr.track_raw_batch(nv12, ['a', 'b', 'c'], boxes=torch.from_numpy(boxes).cuda(), box_frame=[1, 0, 1], pixel_format='nv12',
                                     **kw)
    same_results(got, acr.forward_raw_batch(frames, ['a', 'b', 'c'], boxes=boxes, box_frame=[1, 0, 1]))
    assert (nxt4.cpu().numpy() == rule(['a', 'b', 'c'], boxes, [1, 0, 1])[0]).all()
    with pytest.raises(ValueError, match='one path per region'):
        acr.track_raw_batch(frames, ['a'], boxes=nxt)
    with pytest.raises(ValueError, match='needs boxes'):
        acr.track_raw_batch(frames, ['a', 'b'], box_frame=[0, 1])
