"""GPU tests of region-of-interest pre-processing (the window kernels of csrc/preprocess.hip, DESIGN.md "Regions of
interest").  Everything is integer, so every image is compared byte for byte.  For BGR the yardstick is the numpy statement
of the rule (tests/roi_ref.py over the pre-processing oracle); ops.preprocess_frames runs the same kernel, so equality with
it on a crop made on the host side (frame[t:b, l:r].contiguous()) is an additional property: no neighbouring pixel of the
frame is read.  For NV12 the comparator is nv12_to_rgb_kernel followed by the BGR window kernel on the crop, both other
kernels than the one under test.  All frames are seeded random bytes, so a tap that read a neighbouring pixel of the frame
instead of the window's border or the white pad would change the result."""
import os
import re

import numpy as np
import pytest
import torch

import nv12_ref as N
import roi_ref as R
from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu

SIZES = [(37, 53), (64, 40), (600, 700)]      # H x W
# (frame, (l, t, r, b))
CASES = [
    (0, (10, 5, 30, 25)),                                                      # interior
    (0, (0, 5, 20, 30)), (0, (10, 0, 30, 20)), (0, (20, 5, 53, 30)), (0, (10, 10, 40, 37)),      # touching each edge
    (0, (-4, -6, 25, 20)), (0, (30, 20, 60, 45)), (0, (-9, 11, 99, 19)),       # overhanging: clamped
    (0, (52, 36, 53, 37)), (0, (7, 9, 8, 10)),                                 # 1 x 1: the last pixel, an interior one
    (0, (11, 3, 12, 33)), (0, (3, 11, 33, 12)),                                # a 1-pixel column, a 1-pixel row
    (0, (20, 10, 29, 15)), (0, (20, 10, 25, 19)),                              # 9 x 5 and 5 x 9: up-scaling, odd pad
    (0, (20.5, 10.2, 29.7, 15.0)),                                             # a float box: the window [10:15, 20:30]
    (1, (3, 7, 38, 60)), (1, (0, 0, 40, 1)), (1, (39, 0, 40, 64)), (1, (0, 63, 17, 64)), (1, (-3, 30, 43, 41)),
    (2, (100, 50, 630, 400)), (2, (10, 30, 200, 560)),                         # 530 wide, 530 tall: down-scaling
    (2, (170, 70, 700, 600)),                                                  # a 530 square at the right and bottom edges
    (2, (333, 222, 346, 229)),
]
_cache = {}


def _frames():
    """The seeded frames as numpy (shared, never changed) and on the device."""
    if 'frames' not in _cache:
        host = [np.random.default_rng(1000 * H + W).integers(0, 256, (H, W, 3), dtype=np.uint8) for H, W in SIZES]
        _cache['frames'] = (host, [torch.from_numpy(f).cuda() for f in host])
    return _cache['frames']


def _crop(frame, box):
    l, t, r, b = R.window(frame.shape[0], frame.shape[1], box)
    return frame[t:b, l:r].contiguous()


def test_bgr_windows_equal_the_crop_and_the_reference():
    ops = pkg('ops')
    host, dev = _frames()
    boxes = [box for _, box in CASES]
    box_frame = [f for f, _ in CASES]
    rgb, offsets = ops.preprocess_rois(dev, boxes, box_frame)
    assert tuple(rgb.shape) == (len(CASES), 512, 512, 3) and rgb.dtype == torch.uint8 and tuple(offsets.shape) == (len(CASES), 10)
    crops = [_crop(dev[f], box) for f, box in CASES]
    want, _ = ops.preprocess_frames(crops)
    torch.cuda.synchronize()
    got = rgb.cpu().numpy()
    for i, (f, box) in enumerate(CASES):
        ref, row = R.preprocess(host[f], box)
        bad_crop, bad_ref = int((rgb[i] != want[i]).sum()), int((got[i] != ref).sum())
        print('frame %d box %s: %d bytes differ from the crop, %d from the reference' % (f, box, bad_crop, bad_ref))
        assert bad_crop == 0 and bad_ref == 0, 'region %d (frame %d, box %s)' % (i, f, box)
        assert (offsets[i].numpy() == row).all(), (i, offsets[i], row)
    # a tensor of equal frames is the other form `frames` takes
    same = torch.stack([dev[0], dev[0].flip(0)])
    a, oa = ops.preprocess_rois(same, [(5, 6, 30, 31), (5, 6, 30, 31)])
    b, _ = ops.preprocess_frames([same[0, 6:31, 5:30].contiguous(), same[1, 6:31, 5:30].contiguous()])
    assert torch.equal(a, b) and oa[0].tolist() == [25, 25, 6, 23, 6, 5, 0, 0, 0, 0]


def test_full_frame_box_is_preprocess_frames():
    ops = pkg('ops')
    _, dev = _frames()
    want, want_off = ops.preprocess_frames(dev)
    exact = [(0, 0, W, H) for H, W in SIZES]
    got, off = ops.preprocess_rois(dev, exact)
    assert torch.equal(got, want) and torch.equal(off, want_off)
    over, off = ops.preprocess_rois(dev, [(-5, -7, W + 3, H + 100) for H, W in SIZES])
    assert torch.equal(over, want) and torch.equal(off, want_off)
    one = pkg('acr.utils').img_preprocess(dev[0], bbox=exact[0], single_img_input=True)
    assert torch.equal(one['image'], want[:1]) and torch.equal(one['offsets'], want_off[:1])


def test_regions_share_frames_skip_frames_and_come_in_any_order():
    ops, utils = pkg('ops'), pkg('acr.utils')
    host, dev = _frames()
    boxes = [(100, 50, 300, 200), (5, 5, 30, 30), (400, 300, 700, 600), (20, 1, 50, 33), (0, 0, 64, 64)]
    box_frame = [2, 0, 2, 0, 2]      # frame 2 three times, frame 1 never, out of order
    rgb, offsets = ops.preprocess_rois(dev, boxes, box_frame)
    want, _ = ops.preprocess_frames([_crop(dev[f], box) for f, box in zip(box_frame, boxes)])
    assert torch.equal(rgb, want)
    for i, (f, box) in enumerate(zip(box_frame, boxes)):
        assert (offsets[i].numpy() == R.offsets(host[f].shape[0], host[f].shape[1], box)).all()
    # the frame nothing names is not looked at: a box list that names only frame 1 gives frame 1's window
    only, _ = ops.preprocess_rois(dev, [(3, 7, 38, 60)], torch.tensor([1]))
    assert torch.equal(only[0], ops.preprocess_frames([dev[1][7:60, 3:38].contiguous()])[0][0])
    meta = utils.img_preprocess_gpu(dev, ['a', 'b', 'c', 'd', 'e'], boxes=np.array(boxes), box_frame=np.array(box_frame))
    assert torch.equal(meta['image'], rgb) and torch.equal(meta['offsets'], offsets) and meta['batch_ids'].tolist() == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError, match='region 1'):
        ops.preprocess_rois(dev, [(0, 0, 4, 4), (53, 0, 60, 4)], [0, 0])      # beyond the right edge of the 53-wide frame


def test_one_region_more_than_a_launch_holds():
    ops = pkg('ops')
    src = open(os.path.join(ROOT, pkg().__name__, 'csrc', 'kernels.h')).read()
    per_launch = int(re.search(r'constexpr int ROIS_PER_LAUNCH = (\d+);', src).group(1))
    n = per_launch + 1
    g = np.random.default_rng(7)
    host = [g.integers(0, 256, (8, 8, 3), dtype=np.uint8) for _ in range(5)]
    frames = [torch.from_numpy(f).cuda() for f in host]
    box_frame = [int(v) for v in g.integers(0, 5, n)]
    boxes = []
    for _ in range(n):
        l, t = (int(v) for v in g.integers(0, 7, 2))
        boxes.append((l, t, int(g.integers(l + 1, 9)), int(g.integers(t + 1, 9))))
    rgb, offsets = ops.preprocess_rois(frames, boxes, box_frame)
    want, _ = ops.preprocess_frames([_crop(frames[f], box) for f, box in zip(box_frame, boxes)])
    assert rgb.shape[0] == n
    for i in (0, per_launch - 1, per_launch):      # the first, the last of the first launch, the one of the second launch
        ref, row = R.preprocess(host[box_frame[i]], boxes[i])      # the yardstick: the numpy statement of the rule
        assert (rgb[i].cpu().numpy() == ref).all(), 'region %d' % i
        assert (offsets[i].numpy() == row).all() and (row == R.offsets(8, 8, boxes[i])).all()
    assert torch.equal(rgb, want)      # and no region reads a neighbouring pixel of its frame: the bytes of the crops
    nv12 = [torch.from_numpy(np.concatenate(N.random_nv12(8, 8, s), 0)).cuda() for s in range(5)]
    got, _ = ops.preprocess_rois(nv12, boxes, box_frame, pixel_format='nv12')
    bgr = ops.nv12_to_bgr(nv12)
    assert torch.equal(got, ops.preprocess_frames([_crop(bgr[f], box) for f, box in zip(box_frame, boxes)])[0])


def _pitched(plane, pitch, fill):
    """A strided device view of `plane` inside a buffer whose bytes between the width and the pitch hold `fill`."""
    buf = np.full((plane.shape[0], pitch), fill, np.uint8)
    buf[:, :plane.shape[1]] = plane
    return torch.from_numpy(buf).cuda()[:, :plane.shape[1]]


NV12_CASES = {
    (16, 12): [(1, 0, 9, 8), (0, 1, 8, 9), (3, 5, 10, 14), (2, 2, 7, 5), (5, 3, 6, 4), (0, 0, 12, 16), (7, 0, 12, 16),
               (0, 9, 12, 16), (-3, -3, 5, 5), (11, 15, 12, 16)],
    (38, 54): [(1, 1, 54, 38), (13, 7, 40, 30), (0, 0, 53, 37), (21, 11, 22, 38), (17, 33, 54, 38), (30, 2, 41, 21)],
}


@pytest.mark.parametrize('matrix', ['cv601', 'bt709-full'])
def test_nv12_windows_equal_the_crop_of_the_converted_frame(matrix):
    """Odd l, odd t, both odd, odd sizes, edge-touching; pitches above W with a filler that would show; both input forms."""
    ops = pkg('ops')
    for (H, W), boxes in NV12_CASES.items():
        y, uv = N.random_nv12(H, W, 1000 * H + W)
        surface = _pitched(np.concatenate([y, uv], 0), W + 10, 255)                   # one [H*3/2, W] view, one pitch
        planes = (_pitched(y, W + 6, 255), _pitched(uv, W + 22, 255))                 # (y, uv) with two different pitches
        assert surface.stride(0) == W + 10 and planes[0].stride(0) != planes[1].stride(0)
        bgr_dev = ops.nv12_to_bgr(surface, matrix)[0]
        bgr_ref = torch.from_numpy(N.nv12_to_bgr(y, uv, matrix)).cuda()
        n = len(boxes)
        want_dev, _ = ops.preprocess_frames([_crop(bgr_dev, box) for box in boxes])
        want_ref, _ = ops.preprocess_frames([_crop(bgr_ref, box) for box in boxes])
        got, offsets = ops.preprocess_rois(surface, boxes, [0] * n, pixel_format='nv12', matrix=matrix)
        for i, box in enumerate(boxes):
            bad = int((got[i] != want_ref[i]).sum())
            print('%dx%d %s box %s: %d differing bytes' % (H, W, matrix, box, bad))
            assert bad == 0 and torch.equal(got[i], want_dev[i]), 'box %s of %dx%d' % (box, H, W)
            assert (offsets[i].numpy() == R.offsets(H, W, box)).all()
        two, off2 = ops.preprocess_rois([planes, surface], boxes + boxes, [0] * n + [1] * n, pixel_format='nv12', matrix=matrix)
        assert torch.equal(two[:n], got) and torch.equal(two[n:], got) and torch.equal(off2[:n], offsets)
        # the bytes between W and the pitch are not read: another filler, the same result
        again, _ = ops.preprocess_rois(_pitched(np.concatenate([y, uv], 0), W + 10, 0), boxes, [0] * n, pixel_format='nv12',
                                       matrix=matrix)
        assert torch.equal(again, got)
    if matrix != 'cv601':
        other, _ = ops.preprocess_rois(surface, boxes, [0] * n, pixel_format='nv12')
        assert not torch.equal(other, got), 'the matrix must matter'


@pytest.fixture(scope='module')
def near_sd():
    return pkg('synth').make_state_dict(seed=10)      # the checkpoint of tests/test_gpu_render.py: it detects both hands


def _engine_out(acr, meta):
    """What forward_batch asks of the engine for these network inputs and offsets rows: the fp32 results."""
    eng = acr.model.engine(meta['image'].shape[0])
    eng.set_point_heads(True)
    try:
        return eng.forward(meta['image'], offsets=meta['offsets'], project=True)
    finally:
        eng.set_point_heads(False)


def test_end_to_end_regions_against_crops(near_sd, mano_tables):
    """forward_raw_batch on regions against forward_raw_batch on the crops.  The network inputs are the same bytes, so every
    result field is equal; only the offsets rows differ, by the crop, so pj2d_org differs by (l, t).
    The results are float16, which cannot show 1e-3 pixel: the bound of 1e-3 pixel (one fp32 ulp below 4096 is 4.9e-4; the two
    forms round the same sum in a different order) is asserted on the fp32 pj2d_org of the engine for the same inputs, the
    float16 results are required to be exactly the rounding of those, and region against crop in float16 is held to the
    1e-3 plus half a float16 ulp of either value."""
    cfg, ops, utils, S = pkg('config'), pkg('ops'), pkg('acr.utils'), pkg('_lib')
    acr = pkg('acr.main').ACR(args_set=cfg.parse_args(['--configs_yml', '/nonexistent.yml', '--renderer', 'hip']),
                              state_dict=near_sd, mano_tables=mano_tables, max_batch=3)
    nv12 = [torch.from_numpy(np.concatenate(N.random_nv12(96, 160, s), 0)).cuda() for s in (11, 12)]
    bgr = ops.nv12_to_bgr(nv12)
    assert tuple(bgr.shape) == (2, 96, 160, 3)
    boxes = [(20.5, 10.2, 120.7, 90.0), (-5, -5, 101, 61), (31, 7, 160, 96)]
    box_frame = [1, 0, 1]
    paths = ['a', 'b', 'c']
    windows = [R.window(96, 160, box) for box in boxes]
    assert windows == [(20, 10, 121, 90), (0, 0, 101, 61), (31, 7, 160, 96)]
    crops = [bgr[f][t:b, l:r].contiguous() for f, (l, t, r, b) in zip(box_frame, windows)]
    want = acr.forward_raw_batch(crops, paths)
    got = acr.forward_raw_batch(bgr, paths, boxes=boxes, box_frame=box_frame)
    # fp32, from the engine
    meta = utils.img_preprocess_gpu(bgr, paths, boxes=boxes, box_frame=box_frame)
    meta_crops = utils.img_preprocess_gpu(crops, paths)
    assert torch.equal(meta['image'], meta_crops['image'])
    out, out_crops = _engine_out(acr, meta), _engine_out(acr, meta_crops)
    flags = (out['slots'][:, :, S.SLOT_FLAG] > 0.5).cpu().numpy()
    assert flags.sum() >= 1, 'no hand detected: the comparison would show nothing'
    assert torch.equal(out['slots'], out_crops['slots']) and torch.equal(out['pj2d'], out_crops['pj2d'])
    org, org_crops = out['pj2d_org'].cpu().numpy(), out_crops['pj2d_org'].cpu().numpy()
    shift = np.array([w[:2] for w in windows], np.float32)[:, None, None, :]      # (l, t) per region
    err = np.abs(org.astype(np.float64) - (org_crops.astype(np.float64) + shift))[flags]
    print('hands per region: %s; pj2d_org against the crops + (l, t): max %.3g pixel, largest coordinate %.1f'
          % (flags.sum(1).tolist(), err.max(), np.abs(org[flags]).max()))
    assert np.abs(org[flags]).max() < 4096 and err.max() <= 1e-3
    # the float16 results
    assert sorted(got) == sorted(want) == paths
    for i, p in enumerate(paths):
        assert len(got[p]) == len(want[p]) == int(flags[i].sum())
        for h1, h2 in zip(got[p], want[p]):
            assert sorted(h1) == sorted(h2)
            for k in h1:
                if k != 'pj2d_org':
                    assert np.array_equal(h1[k], h2[k]), (p, k)
            side = int(h1['hand_type'])
            assert np.array_equal(h1['pj2d_org'], org[i, side].astype(np.float16))
            a, b = h1['pj2d_org'].astype(np.float64), h2['pj2d_org'].astype(np.float64) + shift[i, 0, 0]
            tol = 1e-3 + 0.5 * np.spacing(np.abs(h1['pj2d_org'])).astype(np.float64) + \
                0.5 * np.spacing(np.abs(h2['pj2d_org'])).astype(np.float64)
            assert (np.abs(a - b) <= tol).all(), (p, np.abs(a - b).max())
    # NV12 surfaces: the same regions of the same pictures
    got_nv12 = acr.forward_raw_batch(nv12, paths, boxes=boxes, box_frame=box_frame, pixel_format='nv12')
    assert sorted(got_nv12) == paths
    for p in paths:
        assert len(got_nv12[p]) == len(got[p])
        for h1, h2 in zip(got_nv12[p], got[p]):
            assert sorted(h1) == sorted(h2) and all(np.array_equal(h1[f], h2[f]) for f in h1)
    # the skeletons of all regions of a frame over that frame: one drawn frame per source frame
    hand_frame = torch.where(torch.from_numpy(flags), torch.tensor(box_frame)[:, None].expand(3, 2), torch.tensor(-1)).reshape(-1)
    by_hand = ops.draw_skeletons(out['pj2d_org'].reshape(-1, 21, 2).contiguous(), bgr, hand_frame=hand_frame.to(torch.int32), bgr=True)
    for kw in (dict(), dict(pixel_format='nv12')):
        res, views = acr.forward_raw_batch(nv12 if kw else bgr, paths, boxes=boxes, box_frame=box_frame, render=True,
                                           show_items=('pj2d',), **kw)
        assert sorted(views) == ['pj2d'] and tuple(views['pj2d'].shape) == (2, 96, 160, 3)
        assert torch.equal(views['pj2d'], by_hand)
        assert sorted(res) == paths and all(len(res[p]) == len(got[p]) for p in paths)
    assert not torch.equal(by_hand, bgr), 'nothing was drawn'
    # a LIST of frames of different sizes, two of them of one size: drawn per size, returned in input order
    mixed = [bgr[0], bgr[1][:, :128].contiguous(), bgr[1]]
    mixed_frame = [2, 1, 0]
    meta = utils.img_preprocess_gpu(mixed, paths, boxes=boxes, box_frame=mixed_frame)
    out = _engine_out(acr, meta)
    flags = out['slots'][:, :, S.SLOT_FLAG].cpu() > 0.5
    assert flags.sum() >= 1
    frame_of_hand = torch.where(flags, torch.tensor(mixed_frame)[:, None].expand(3, 2), torch.tensor(-1)).reshape(-1)
    kps = out['pj2d_org'].reshape(-1, 21, 2).contiguous()
    res, views = acr.forward_raw_batch(mixed, paths, boxes=boxes, box_frame=mixed_frame, render=True, show_items=('pj2d', 'org_img'))
    assert sorted(views) == ['org_img', 'pj2d'] and views['org_img'] is mixed and len(views['pj2d']) == 3
    for i, frame in enumerate(mixed):      # each frame against ops.draw_skeletons on that frame alone
        alone = torch.where(frame_of_hand == i, 0, -1).to(torch.int32)
        want_i = ops.draw_skeletons(kps, frame[None], hand_frame=alone, bgr=True)[0]
        assert tuple(views['pj2d'][i].shape) == tuple(frame.shape) and torch.equal(views['pj2d'][i], want_i), 'frame %d' % i
    assert sorted(res) == paths
    # views that need a viewport per region are refused, before anything runs
    for kw in (dict(show_items=('mesh',)), dict(show_items=('pj2d', 'centermap')), dict()):
        with pytest.raises(ValueError, match='over regions'):
            acr.forward_raw_batch(bgr, paths, boxes=boxes, box_frame=box_frame, render=True, **kw)
    with pytest.raises(ValueError, match='one path per region'):
        acr.forward_raw_batch(bgr, paths[:2], boxes=boxes, box_frame=box_frame)
